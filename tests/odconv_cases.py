"""Case tables, input generators and fp64 references of tests/test_gpu_odconv_kernels.py (a plain module, imported like
tests/disc_cases.py; checked on the host by tests/test_host_odconv_cases.py).

The kernels under test are the fused ODConv1d / ODConvTranspose1d kernels of csrc/odconv_fused.hip.  One function, od_dispatch, picks
a template instantiation ("arm") of one of five kernels from the shape; `od_arm` restates it - od_make's geometry, the predicates of
od_dispatch and the LDS and grid formulas of the five launchers - as an independent second statement.  tests/test_host_odconv_cases.py
compares it, without a GPU, with what the library itself plans (mv_odconv_cl_plan: the dispatcher's own dry run) over a sweep of
shapes and every row below.  The tables hold, for every arm a valid shape can reach, the smallest shape that selects it, ragged
companions that still select it, and the routes the generator takes to it (regular convs, the data gradient's 2-tap shapes).

Every input is made of small integers: x has exactly `nnz` = 8 / taps non-zero channels of +-1 per time step, bank weights are in
{-1, 0, 1}, alpha holds integers with sum |alpha| <= 3, bank biases are in -3..3.  Every sum is then exact in fp32 in any order -
whether an arm mixes the banks first (cl, mt, sample, stream) or applies alpha to per-bank accumulators (kloop) - and every output is
an integer of magnitude <= 8 * 3 + 9 = 33, a half-integer after LeakyReLU(0.5): at most 8 significant bits, exactly representable in
bf16, fp16 and fp32.  The GPU tests can then ask for bit equality with the fp64 reference.

Paths that no valid shape reaches (the host test's sweep reaches exactly the arms of the tables):
  * od_stream_launch's `nq < 32` tile count: the dispatcher sends ntiles <= 3 (nq <= 48) to the short-sequence arms first, so the
    streaming kernel always sees nq >= 49.  The stream rows start at nq = 49 and 50 instead of "around 32".
  * od_sample_launch / od_mt_launch for fp32 in the big-bank branch: compiled out (`if constexpr (sizeof(T) == 2)`), not instantiated.
Every instantiation od_dispatch names is reached by some row; none is dead.

IMPULSE holds, per arm, the row the impulse tests run on: more than one sample, at least 16 input channels, at least two row blocks,
and at least two column tiles wherever the arm can have them (the S = 2 arms cannot: they only see sequences of one tile) - for mt a
workgroup that walks TL = 2 tiles, for stream waves that walk two tiles in more than one workgroup per sample.
"""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

from disc_cases import (DT_NAME, MV_BF16, MV_ERR_ARG, MV_ERR_DTYPE, MV_ERR_UNSUPPORTED, MV_F16, MV_F32, TORCH_DT, Refused, cdiv, ints,
                        lds_row_stride, lrelu)

ACT_NONE, ACT_LRELU, ACT_TANH = 0, 1, 2
SLOPE = 0.5
LDS_MAX = 160 * 1024
OD_MAXK = 8
FAM = ("cl", "mt", "sample", "kloop", "stream")          # mv_odconv_cl_plan out[0]
OS_NW, OS_RB = 8, 256
OS_RING = 2 * 16 * (OS_RB + 16) + (OS_RB + 16)


# ----------------------------------------------------------------------------------------------- geometry (od_make)
Geom = namedtuple("Geom", "Tout ntaps M nq ksteps nchunks shift_lo")


def od_geom(B, Cin, Tin, Cout, ks, stride, pad, dil, transposed, K, output_padding=0):
    """od_make: output length, taps, GEMM rows M, GEMM columns per sample nq, k-steps (32 k-elements each) - or Refused."""
    if B <= 0 or Cin <= 0 or Cin % 8 or Cout <= 0 or Cout % 8 or Tin <= 0 or ks <= 0 or K < 1 or K > OD_MAXK:
        raise Refused(MV_ERR_UNSUPPORTED)
    if transposed:
        if dil != 1 or stride < 1 or ks % stride or pad < 0 or not 0 <= output_padding < stride:
            raise Refused(MV_ERR_UNSUPPORTED)
        ntaps, M = ks // stride, stride * Cout
        Tout = (Tin - 1) * stride - 2 * pad + ks + output_padding
        nq = Tin + ntaps - 1 + (1 if output_padding else 0)      # output_padding rows come from one more (zero-input) column
        shift_lo = -(ntaps - 1)
    else:
        if stride != 1 or dil < 1 or pad < 0 or output_padding:
            raise Refused(MV_ERR_UNSUPPORTED)
        ntaps, M = ks, Cout
        Tout = Tin + 2 * pad - dil * (ks - 1)
        nq, shift_lo = Tout, -pad
    if Tout <= 0:
        raise ValueError("no output")
    if M % 16:
        raise Refused(MV_ERR_UNSUPPORTED)
    nchunks = ntaps * (Cin // 8)
    return Geom(Tout, ntaps, M, nq, cdiv(nchunks, 4), nchunks, shift_lo)


# ----------------------------------------------------------------------------------------------- the five launchers
# name; family; samples per workgroup; MW, NB, KB-or-CIN, TI = f16 flag; column tile; GEMM rows per workgroup; LDS bytes; grid;
# pooled_out slots per sample; walk = TL (mt: column tiles a workgroup walks) / tpw (stream: 16-column tiles per wave) / 0
Arm = namedtuple("Arm", "name family S MW NB kbc ti16 cols rows lds grid slots walk")


def _xrow(Cin, es):
    """LDS row of an x tile: 16-bit elements, or hi + lo bf16 planes for fp32 storage."""
    return lds_row_stride(4 * Cin if es == 4 else Cin * es, 2)


def _cl(T, es, g, B, Cin, dil, transposed, K, S, MW, NB):
    KB = 4 if K <= 4 else 8
    nrows = NB * 16 + (g.ntaps - 1) * (1 if transposed else dil)
    xb = S * nrows * _xrow(Cin, es)
    ob = S * NB * 16 * (4 * MW * 16 * es + 16)
    lds = 4 * (S * OD_MAXK + S * 4 * MW * 16) + max(xb, ob)
    grid = (cdiv(g.nq, NB * 16), cdiv(g.M // 16, 4 * MW), cdiv(B, S))
    if lds > LDS_MAX or grid[1] > 65535 or grid[2] > 65535:
        return None
    return Arm(f"odconv_cl_kernel<{T},{S},{MW},{NB},{KB}>", "cl", S, MW, NB, KB, 0, NB * 16, 4 * MW * 16, lds, grid, grid[0], 0)


def _mt(T, es, g, B, MW, NB, CIN, ti16=0):
    xb = (NB * 16 + 1) * _xrow(CIN, es)
    ob = NB * 16 * (4 * MW * 16 * es + 16)
    lds = 4 * (OD_MAXK + 4 * MW * 16) + max(xb, ob)
    if lds > 80 * 1024:
        return None
    ntl, gy = cdiv(g.nq, NB * 16), cdiv(g.M // 16, 4 * MW)
    TL = min(max(cdiv(ntl * gy * B, 512), 1), 16)
    grid = (cdiv(ntl, TL), gy, B)
    if gy > 65535 or B > 65535:
        return None
    return Arm(f"odconv_cl_mt_kernel<{T},{MW},{NB},{CIN}" + (",f16>" if ti16 else ">"), "mt", 1, MW, NB, CIN, ti16, NB * 16, 4 * MW * 16,
               lds, grid, grid[0], TL)


def _sample(T, g, B, Cin, Tin, transposed, K, act, CIN=256, NT=17):
    if (not transposed or g.ntaps != 2 or K > 4 or Cin != CIN or g.M % 128 or g.nq > NT * 16 or g.nq <= (NT - 1) * 16 or act > ACT_LRELU
            or Tin * CIN * 2 > 0x7fff0000):
        return None
    lds = 4 * (OD_MAXK + max(CIN, 256)) + (g.nq + 1) * lds_row_stride(CIN * 2, 2)
    if lds > LDS_MAX or B > 65535:
        return None
    return Arm(f"odconv_sample_kernel<{T},{CIN},{NT}>", "sample", 1, 1, NT, CIN, 0, NT * 16, 128, lds, (g.M // 128, B, 1), 1, 0)


def _kloop(T, es, g, B, Cin, Tin, K, S, MW, NB=3):
    PD = 4 if es == 4 else 8
    if g.nq > NB * 16 or K > 4 or Cin % 32 or (Cin // 32) % PD or g.ksteps % PD or g.nchunks != 4 * g.ksteps or g.ntaps > 2:
        return None
    nrows = Tin - g.shift_lo + 1
    xb = S * nrows * _xrow(Cin, es)
    ob = S * NB * 16 * (64 * MW * es + 16)
    lds = 4 * (S * OD_MAXK + S * max(Cin, 256)) + max(xb, ob)
    if lds > LDS_MAX or B * Tin * Cin * es > 0x7fff0000 or cdiv(B, S) > 65535:
        return None
    return Arm(f"odconv_kloop_kernel<{T},{S},{NB},{MW}>", "kloop", S, MW, NB, 4, 0, NB * 16, 4 * MW * 16, lds,
               (cdiv(g.M // 16, 4 * MW), cdiv(B, S), 1), 1, 0)


def _stream(g, B, Tin, Cout, K, CIN, MT, xf16):
    KST = 2 * CIN // 32
    if Tin * OS_RB >= 2 ** 31 or g.Tout * Cout * 4 >= 2 ** 31 or Cout % 16 or K > 4:
        return None
    lds = MT * KST * 2048 + 4 * (OD_MAXK + MT * 16 + OS_NW * MT * 16) + OS_NW * OS_RING
    if lds > LDS_MAX:
        return None
    gy = cdiv(g.M // 16, MT)
    tiles = (g.nq - 1) // 16 if g.nq >= 32 else cdiv(g.nq, 16)   # the odd column goes to the sample's last wave
    wgs = max(256 // (B * gy), 1)
    tpw = max(cdiv(tiles, wgs * OS_NW), 1)
    gx = cdiv(tiles, tpw * OS_NW)
    if gy > 65535 or B > 65535:
        return None
    return Arm(f"odconv_stream_kernel<{CIN},{MT},{'true' if xf16 else 'false'}>", "stream", 1, MT, 1, CIN, int(xf16), 16, MT * 16, lds,
               (gx, gy, B), gx, tpw)


# ----------------------------------------------------------------------------------------------- the dispatcher (od_dispatch)
def od_arm(B, Cin, Tin, Cout, ks, stride, pad, dil, transposed, K, act, has_film, dtype, in_f16, out_pair, output_padding=0):
    """The instantiation mv_odconv_cl_fwd (in_f16: _fwd_in16, out_pair: _fwd_pair) launches for this shape, or Refused(code)."""
    g = od_geom(B, Cin, Tin, Cout, ks, stride, pad, dil, transposed, K, output_padding)
    es = 4 if dtype == MV_F32 else 2
    ntiles = cdiv(g.nq, 16)
    wbytes = K * g.M * g.ksteps * 32 * es
    if in_f16 and (dtype != MV_F32 or ntiles <= 3 or wbytes > 1 << 20):
        raise Refused(MV_ERR_UNSUPPORTED)
    if out_pair and (dtype != MV_F32 or ntiles <= 3 or wbytes > 1 << 20 or Cout != 64 or in_f16):
        raise Refused(MV_ERR_UNSUPPORTED)
    if dtype not in DT_NAME:
        raise Refused(MV_ERR_DTYPE)
    T = DT_NAME[dtype]
    cl = lambda S, MW, NB: _cl(T, es, g, B, Cin, dil, transposed, K, S, MW, NB)
    two_tap = bool(transposed) and g.ntaps == 2 and K <= 4 and not has_film and act <= ACT_LRELU
    arm = None
    if ntiles <= 3:                                      # short sequences, big kernels
        if not has_film and wbytes > 4 << 20 and B >= 2:
            MW = 2 if es == 4 else 1
            arm = _kloop(T, es, g, B, Cin, Tin, K, 2, MW) or _kloop(T, es, g, B, Cin, Tin, K, 1, MW)
        if arm is None and cdiv(B, 2) * cdiv(g.M, 64) * cdiv(ntiles, 3) < 256:
            arm = cl(1, 1, 3)
        arm = arm or cl(2, 1, 3) or cl(1, 1, 3)
    elif wbytes > 1 << 20:                               # big kernels, medium sequences
        if two_tap and Cin == 256 and es == 2:
            if B * (g.M // 128) >= 128:
                arm = _sample(T, g, B, Cin, Tin, transposed, K, act)
            arm = arm or _mt(T, es, g, B, 1, 6, 256)
        arm = arm or cl(1, 2, 9) or cl(1, 1, 3)
    else:                                                # small kernels, long sequences
        if two_tap and Cin in (64, 128):
            if es == 2:
                arm = _mt(T, es, g, B, 2, 8, 64) if Cin == 64 else _mt(T, es, g, B, 2, 4, 128)
            else:
                if in_f16 and Cin == 128:
                    arm = _stream(g, B, Tin, Cout, K, 128, 4, True)
                elif not in_f16 and Cin == 64:
                    arm = _stream(g, B, Tin, Cout, K, 64, 8, False)
                if arm is None:
                    if out_pair:
                        raise Refused(MV_ERR_UNSUPPORTED)
                    MW = 2 if Cin == 64 else 1
                    arm = _mt(T, es, g, B, MW, 4, Cin, 1 if in_f16 else 0)
        if in_f16 or out_pair:                           # only the multi-tile / streaming kernels widen their input / write pair rows
            if arm is None:
                raise Refused(MV_ERR_UNSUPPORTED)
            return arm
        arm = arm or cl(1, 2, 8) or cl(1, 1, 3)
    if arm is None:
        raise Refused(MV_ERR_UNSUPPORTED)
    return arm


# ----------------------------------------------------------------------------------------------- case tables
Case = namedtuple("Case", "arm B Cin Tin Cout ks stride pad dil tr K op dtype in_f16 out_pair film")
MAX_MACS = 2.0e9        # multiply-adds of one fp64 reference: ragged companions above it are left out.  Left out for this reason, all of
                        # the sample-resident arm: B = 17 (2.29 GMAC), T = 270 (271 columns, 2.27) and T = 270 with output_padding
                        # (2.28).  Hand-written rows may be larger: the three sample-resident rows, 16 x 256 (271) x 256 -> 128 x8, are
                        # 2.16 - 2.28 GMAC (checked on the host)


def shape_of(c):
    """The key of the shared fp64 reference: everything but arm, dtype and entry point."""
    return tuple(c[1:12])


def arm_of(c, act=ACT_LRELU):
    return od_arm(c.B, c.Cin, c.Tin, c.Cout, c.ks, c.stride, c.pad, c.dil, c.tr, c.K, act, c.film, c.dtype, c.in_f16, c.out_pair, c.op)


def geom_of(c):
    return od_geom(c.B, c.Cin, c.Tin, c.Cout, c.ks, c.stride, c.pad, c.dil, c.tr, c.K, c.op)


def macs(c):
    g = geom_of(c)
    return c.B * g.nq * g.M * g.ntaps * c.Cin


def case_id(c):
    kind = f"T{c.ks}s{c.stride}" if c.tr else f"C{c.ks}d{c.dil}"
    tail = ("-in16" if c.in_f16 else "") + ("-pair" if c.out_pair else "") + ("-film" if c.film else "") + (f"-op{c.op}" if c.op else "")
    return f"{c.arm}-B{c.B}T{c.Tin}-{c.Cin}to{c.Cout}-{kind}p{c.pad}-K{c.K}{tail}"


def _row(B, Cin, Tin, Cout, ks, stride, pad, dil, tr, K, op=0, in_f16=0, out_pair=0, film=0):
    return (B, Cin, Tin, Cout, ks, stride, pad, dil, tr, K, op, in_f16, out_pair, film)


# Shapes (B, Cin, Tin, Cout, ks, stride, pad, dil, transposed, K[, output_padding, in_f16, out_pair, film]) for 16-bit storage.  The first
# row of an arm is the smallest shape that selects it; rows behind it are other routes to the same arm.
_T16 = [
    # ---- short sequences (at most 3 column blocks)
    _row(2, 512, 32, 264, 4, 2, 1, 1, 1, 4),             # kloop S = 2: 4.3 MB of banks; M = 528, the ninth 64-row block holds one M-tile
    _row(2, 512, 32, 256, 16, 8, 4, 1, 1, 4),            # kloop S = 2: the first upsampler (16.8 MB of banks)
    _row(5, 512, 40, 256, 16, 8, 4, 1, 1, 4),            # kloop S = 2, B odd, T = 40
    _row(2, 1024, 36, 136, 4, 2, 1, 1, 1, 4),            # kloop S = 1: two 1024-channel tiles do not fit 160 KB; M = 272, the fifth
                                                         # 64-row block holds one M-tile
    _row(2, 1024, 36, 64, 16, 8, 4, 1, 1, 4),            # kloop S = 1: two 1024-channel tiles do not fit 160 KB
    _row(3, 2048, 33, 512, 2, 1, 0, 1, 0, 4),            # kloop S = 1: the data gradient of the first upsampler (2-tap conv, 2048 -> 512)
    _row(3, 2048, 34, 512, 2, 1, 0, 1, 0, 4),            # kloop S = 1: the same one column past two 16-column blocks (T <= 40 leaves
                                                         # the 1024-channel rows no block boundary to straddle: they need T >= 36)
    _row(1, 8, 3, 16, 1, 1, 0, 1, 0, 1),                 # cl<1,1,3,4>: the smallest launch there is
    _row(2, 80, 32, 512, 7, 1, 3, 1, 0, 4, film=1),      # cl<1,1,3,4>: input_proj with FiLM
    _row(3, 128, 16, 512, 7, 1, 3, 1, 0, 4, film=1),     # cl<1,1,3,4>: the 48 kHz input_proj
    _row(1, 8, 3, 16, 1, 1, 0, 1, 0, 8),                 # cl<1,1,3,8>
    _row(2, 80, 32, 512, 7, 1, 3, 1, 0, 8, film=1),      # cl<1,1,3,8>: input_proj with 8 banks
    _row(32, 8, 3, 1024, 1, 1, 0, 1, 0, 4),              # cl<2,1,3,4>: 16 x 16 = 256 workgroups of two samples
    _row(32, 16, 5, 1024, 3, 1, 1, 1, 0, 4),             # cl<2,1,3,4>: three taps
    _row(32, 16, 5, 128, 16, 8, 4, 1, 1, 4),             # cl<2,1,3,4>: transposed
    _row(33, 16, 5, 128, 16, 8, 4, 1, 1, 4, op=1),       # cl<2,1,3,4>: transposed, B odd, output_padding
    _row(32, 8, 3, 1024, 1, 1, 0, 1, 0, 8),              # cl<2,1,3,8>
    _row(33, 16, 5, 1024, 3, 1, 1, 1, 0, 8),             # cl<2,1,3,8>: three taps, B odd
    _row(33, 16, 5, 1024, 3, 1, 1, 1, 0, 4),             # cl<2,1,3,4>: three taps, B odd
    # ---- big banks (> 1 MB), more than 3 column blocks
    _row(16, 256, 256, 128, 16, 8, 4, 1, 1, 4),          # sample<256,17>: the second upsampler, 257 columns, B * (M / 128) = 128
    _row(16, 256, 271, 128, 16, 8, 4, 1, 1, 4),          # sample<256,17>: 272 columns
    _row(16, 256, 256, 128, 16, 8, 4, 1, 1, 4, op=1),    # sample<256,17>: 258 columns, the last from output_padding
    _row(1, 256, 49, 144, 4, 2, 1, 1, 1, 4),             # mt<1,6,256>
    _row(15, 256, 256, 128, 16, 8, 4, 1, 1, 4),          # mt<1,6,256>: the second upsampler one sample short of the sample-resident arm
    _row(1, 512, 49, 272, 1, 1, 0, 1, 0, 4),             # cl<1,2,9,4>: 1.06 MB of banks
    _row(1, 512, 49, 512, 3, 1, 1, 1, 0, 4),             # cl<1,2,9,4>: three taps
    _row(1, 256, 49, 144, 4, 2, 1, 1, 1, 4, film=1),     # cl<1,2,9,4>: a 2-tap upsampler with FiLM
    _row(1, 512, 49, 512, 7, 1, 3, 1, 0, 1),             # cl<1,2,9,4>: plain conv (K = 1), ks 7
    _row(1, 512, 49, 144, 1, 1, 0, 1, 0, 8),             # cl<1,2,9,8>
    _row(1, 512, 49, 512, 3, 1, 1, 1, 0, 8),             # cl<1,2,9,8>: three taps
    _row(1, 576, 49, 256, 3, 1, 1, 1, 0, 4),             # cl<1,1,3,4>: the 144-column tile of 576 channels does not fit
    _row(2, 1024, 50, 256, 2, 1, 0, 1, 0, 4),            # cl<1,1,3,4>: the data gradient of the second upsampler (1024 -> 256)
    _row(1, 576, 49, 256, 3, 1, 1, 1, 0, 8),             # cl<1,1,3,8> behind cl<1,2,9,8>
    _row(2, 576, 49, 272, 3, 1, 1, 1, 0, 4),             # cl<1,1,3,4>: two column tiles, five row blocks (the last: one M-tile), two samples
    _row(2, 576, 49, 272, 3, 1, 1, 1, 0, 8),             # cl<1,1,3,8>: the same
    _row(2, 512, 150, 272, 1, 1, 0, 1, 0, 4),            # cl<1,2,9,4>: two column tiles, three row blocks
    _row(2, 512, 150, 144, 1, 1, 0, 1, 0, 8),            # cl<1,2,9,8>: two column tiles, two row blocks
    # ---- small banks, long sequences
    _row(1, 64, 48, 8, 4, 2, 1, 1, 1, 4),                # mt<2,8,64>: M = 16, one M-tile
    _row(2, 64, 200, 64, 4, 2, 1, 1, 1, 4),              # mt<2,8,64>: the last upsampler
    _row(1, 128, 48, 8, 4, 2, 1, 1, 1, 4),               # mt<2,4,128>
    _row(2, 128, 100, 64, 8, 4, 2, 1, 1, 4),             # mt<2,4,128>: the 48 kHz third upsampler (ks 8, stride 4)
    _row(2, 128, 100, 64, 4, 2, 1, 1, 1, 1),             # mt<2,4,128>: plain transposed conv (K = 1)
    _row(1, 8, 49, 16, 1, 1, 0, 1, 0, 1),                # cl<1,2,8,4>
    _row(2, 64, 60, 64, 7, 1, 3, 1, 0, 4),               # cl<1,2,8,4>: ks 7, pad 3
    _row(2, 64, 60, 64, 3, 1, 5, 5, 0, 4),               # cl<1,2,8,4>: dilated (the plain HiFi-GAN resblock convs)
    _row(2, 128, 130, 128, 2, 1, 0, 1, 0, 4),            # cl<1,2,8,4>: the data gradient of the third upsampler (128 -> 128)
    _row(2, 128, 130, 64, 2, 1, 0, 1, 0, 4),             # cl<1,2,8,4>: the data gradient of the last upsampler (128 -> 64)
    _row(2, 64, 60, 64, 4, 2, 1, 1, 1, 4, film=1),       # cl<1,2,8,4>: a 2-tap upsampler with FiLM
    _row(1, 8, 49, 16, 1, 1, 0, 1, 0, 8),                # cl<1,2,8,8>
    _row(2, 64, 60, 64, 4, 2, 1, 1, 1, 8),               # cl<1,2,8,8>: an upsampler with 8 banks
    _row(1, 640, 49, 16, 1, 1, 0, 1, 0, 1),              # cl<1,1,3,4>: 128 columns of 640 channels do not fit
    _row(1, 8, 700, 16, 3, 1, 300, 300, 0, 1),           # cl<1,1,3,4>: a dilation of 300 (728 rows of a 128-column tile) does not fit
    _row(1, 640, 49, 16, 1, 1, 0, 1, 0, 8),              # cl<1,1,3,8> behind cl<1,2,8,8>
    _row(1, 64, 48, 72, 4, 2, 1, 1, 1, 4),               # mt<2,8,64>: M = 144, a second row block with one M-tile (and its TL = 2 walk)
    _row(1, 128, 48, 72, 4, 2, 1, 1, 1, 4),              # mt<2,4,128>: the same
    _row(2, 64, 130, 144, 3, 1, 1, 1, 0, 4),             # cl<1,2,8,4>: two column tiles, two row blocks
    _row(2, 64, 130, 144, 3, 1, 1, 1, 0, 8),             # cl<1,2,8,8>: the same
]
# fp32 storage (split bf16 operands; the streaming kernels use f16 hi + lo)
_T32 = [
    _row(2, 512, 32, 256, 16, 8, 4, 1, 1, 4),            # kloop<2,3,2>
    _row(5, 512, 36, 256, 16, 8, 4, 1, 1, 4),            # kloop<2,3,2>: B odd, the longest T that fits two samples
    _row(3, 1024, 36, 64, 16, 8, 4, 1, 1, 4),            # kloop<1,3,2>: two samples of 1024 channels do not fit from T = 17 on (one: to T = 36)
    _row(3, 512, 37, 256, 16, 8, 4, 1, 1, 4),            # kloop<1,3,2>: two samples of 37 steps do not fit
    _row(5, 512, 40, 256, 16, 8, 4, 1, 1, 4),            # kloop<1,3,2>
    _row(1, 8, 3, 16, 1, 1, 0, 1, 0, 1),                 # cl<1,1,3,4>
    _row(2, 80, 32, 512, 7, 1, 3, 1, 0, 4, film=1),      # cl<1,1,3,4>: input_proj with FiLM
    _row(1, 8, 3, 16, 1, 1, 0, 1, 0, 8),                 # cl<1,1,3,8>
    _row(32, 8, 3, 1024, 1, 1, 0, 1, 0, 4),              # cl<2,1,3,4>
    _row(32, 16, 5, 1024, 3, 1, 1, 1, 0, 4),             # cl<2,1,3,4>: three taps
    _row(32, 8, 3, 1024, 1, 1, 0, 1, 0, 8),              # cl<2,1,3,8>
    _row(1, 256, 49, 272, 1, 1, 0, 1, 0, 4),             # cl<1,2,9,4>: 1.06 MB of banks
    _row(2, 256, 100, 128, 16, 8, 4, 1, 1, 4),           # cl<1,2,9,4>: the second upsampler in fp32
    _row(1, 256, 49, 256, 7, 1, 3, 1, 0, 1),             # cl<1,2,9,4>: plain conv, ks 7
    _row(1, 256, 49, 144, 1, 1, 0, 1, 0, 8),             # cl<1,2,9,8>
    _row(1, 256, 49, 512, 3, 1, 1, 1, 0, 8),             # cl<1,2,9,8>
    _row(1, 288, 49, 512, 3, 1, 1, 1, 0, 4),             # cl<1,1,3,4> behind cl<1,2,9,4>
    _row(1, 288, 49, 512, 3, 1, 1, 1, 0, 8),             # cl<1,1,3,8> behind cl<1,2,9,8>
    _row(1, 64, 48, 16, 4, 2, 1, 1, 1, 4),               # stream<64,8,false>: M = 32 of the workgroup's 128 rows
    _row(2, 64, 200, 64, 4, 2, 1, 1, 1, 4),              # stream<64,8,false>: the last upsampler
    _row(2, 64, 200, 64, 4, 2, 1, 1, 1, 4, out_pair=1),  # stream<64,8,false> writing pair rows
    _row(2, 64, 100, 80, 4, 2, 1, 1, 1, 4),              # stream<64,8,false>: M = 160, the second 128-row block holds two M-tiles
    _row(1, 64, 128, 16, 4, 2, 1, 1, 1, 4),              # stream<64,8,false>: 129 columns, the odd one behind the last wave's only tile
    _row(2, 64, 256, 64, 4, 2, 1, 1, 1, 4),              # stream<64,8,false>: the 257th column (two with output_padding), two workgroups
    _row(33, 64, 256, 64, 16, 8, 4, 1, 1, 4),            # stream<64,8,false>: the 257th column behind two tiles per wave, wgs = 1
    _row(33, 64, 150, 64, 16, 8, 4, 1, 1, 4),            # stream<64,8,false>: wgs = 1, two tiles per wave
    _row(32, 64, 275, 64, 16, 8, 4, 1, 1, 4),            # stream<64,8,false>: two workgroups per sample, two tiles per wave
    _row(1, 128, 48, 16, 4, 2, 1, 1, 1, 4, in_f16=1),    # stream<128,4,true>
    _row(2, 128, 100, 64, 4, 2, 1, 1, 1, 4, in_f16=1),   # stream<128,4,true>: the third upsampler behind an fp16 front
    _row(2, 128, 100, 48, 4, 2, 1, 1, 1, 4, in_f16=1),   # stream<128,4,true>: M = 96, the second 64-row block holds two M-tiles
    _row(1, 128, 128, 16, 4, 2, 1, 1, 1, 4, in_f16=1),   # stream<128,4,true>: 129 columns
    _row(2, 128, 256, 64, 4, 2, 1, 1, 1, 4, in_f16=1),   # stream<128,4,true>: the 257th column
    _row(33, 128, 256, 32, 16, 8, 4, 1, 1, 4, in_f16=1),  # stream<128,4,true>: the 257th column behind two tiles per wave
    _row(33, 128, 150, 32, 16, 8, 4, 1, 1, 4, in_f16=1),  # stream<128,4,true>: wgs = 1, two tiles per wave
    _row(1, 64, 48, 8, 4, 2, 1, 1, 1, 4),                # mt<float,2,4,64>: Cout % 16 != 0 keeps it off the streaming kernel
    _row(1, 128, 48, 8, 4, 2, 1, 1, 1, 4),               # mt<float,1,4,128>
    _row(2, 128, 100, 64, 8, 4, 2, 1, 1, 4),             # mt<float,1,4,128>: the 48 kHz third upsampler
    _row(1, 64, 48, 16, 4, 2, 1, 1, 1, 4, in_f16=1),     # mt<float,2,4,64,f16>
    _row(1, 128, 48, 8, 4, 2, 1, 1, 1, 4, in_f16=1),     # mt<float,1,4,128,f16>: Cout % 16 != 0
    _row(1, 8, 49, 16, 1, 1, 0, 1, 0, 1),                # cl<1,2,8,4>
    _row(2, 64, 60, 64, 7, 1, 3, 1, 0, 4),               # cl<1,2,8,4>: ks 7, pad 3
    _row(2, 64, 60, 64, 3, 1, 5, 5, 0, 1),               # cl<1,2,8,4>: dilated plain conv
    _row(2, 128, 130, 64, 2, 1, 0, 1, 0, 4),             # cl<1,2,8,4>: the data gradient of the last upsampler
    _row(1, 8, 49, 16, 1, 1, 0, 1, 0, 8),                # cl<1,2,8,8>
    _row(2, 64, 60, 64, 4, 2, 1, 1, 1, 8),               # cl<1,2,8,8>
    _row(1, 320, 49, 16, 1, 1, 0, 1, 0, 1),              # cl<1,1,3,4> behind cl<1,2,8,4>
    _row(1, 320, 49, 16, 1, 1, 0, 1, 0, 8),              # cl<1,1,3,8> behind cl<1,2,8,8>
    _row(2, 288, 49, 528, 3, 1, 1, 1, 0, 4),             # cl<1,1,3,4>: two column tiles, nine row blocks (the last: one M-tile), two samples
    _row(2, 288, 49, 528, 3, 1, 1, 1, 0, 8),             # cl<1,1,3,8>: the same
    _row(33, 16, 5, 1024, 3, 1, 1, 1, 0, 4),             # cl<2,1,3,4>: three taps, B odd
    _row(33, 16, 5, 1024, 3, 1, 1, 1, 0, 8),             # cl<2,1,3,8>: three taps, B odd
    _row(2, 256, 150, 272, 1, 1, 0, 1, 0, 4),            # cl<1,2,9,4>: two column tiles, three row blocks
    _row(2, 256, 150, 144, 1, 1, 0, 1, 0, 8),            # cl<1,2,9,8>: two column tiles, two row blocks
    _row(32, 128, 275, 32, 16, 8, 4, 1, 1, 4, in_f16=1),  # stream<128,4,true>: two workgroups per sample, two tiles per wave, four row blocks
    _row(1, 64, 48, 72, 4, 2, 1, 1, 1, 4),               # mt<float,2,4,64>: M = 144, a second row block (and its TL = 2 walk)
    _row(1, 128, 48, 72, 4, 2, 1, 1, 1, 4),              # mt<float,1,4,128>: three row blocks
    _row(1, 64, 48, 72, 4, 2, 1, 1, 1, 4, in_f16=1),     # mt<float,2,4,64,f16>: M = 144
    _row(1, 128, 48, 72, 4, 2, 1, 1, 1, 4, in_f16=1),    # mt<float,1,4,128,f16>: three row blocks
    _row(2, 64, 130, 144, 3, 1, 1, 1, 0, 4),             # cl<1,2,8,4>: two column tiles, two row blocks
    _row(2, 64, 130, 144, 3, 1, 1, 1, 0, 8),             # cl<1,2,8,8>: the same
]


def _mk(shape, dt):
    c = Case("", *shape[:11], dt, *shape[11:])
    return c._replace(arm=arm_of(c).name)


def _selects(c, name):
    try:
        return arm_of(c).name == name and macs(c) <= MAX_MACS
    except (Refused, ValueError):
        return False


def _walk_row(c):
    """mt: the shortest Tin (B = 3) at which a workgroup walks TL = 2 column tiles and the last group holds a single tile."""
    for ntl in range(3, 400, 2):
        t = c._replace(B=3, Tin=(ntl - 1) * arm_of(c).cols + 3)
        try:
            a = arm_of(t)
        except Refused:
            continue
        if a.name == c.arm and a.walk == 2 and cdiv(geom_of(t).nq, a.cols) % 2 == 1:
            return t
    return None


def col_step(arm):
    """Columns between the boundaries the ragged rows straddle: the arm's column tile; for the K-loop and the sample-resident kernel,
    whose single tile holds the whole sample, the 16-column MFMA block inside it."""
    return 16 if arm.family in ("kloop", "sample") else arm.cols


def _companions(c):
    """Ragged variants that still select c's arm, one dimension at a time: B one more (not a multiple of S) and B = 3; nq one past and
    one short of a column-tile multiple; a Cout that leaves the last row block partly empty; output_padding = 1; for mt the TL = 2
    walk with a ragged last group."""
    a, g = arm_of(c), geom_of(c)
    out = []
    cands = [c._replace(B=c.B + 1), c._replace(B=3)]
    step = col_step(a)
    tiles = max(cdiv(g.nq, step), 2 if g.nq > 48 or a.family == "kloop" else 1)
    for nq in ((33, 31, 32) if a.family == "kloop" else (tiles * step + 1, tiles * step - 1, tiles * step)):
        cands.append(c._replace(Tin=c.Tin + nq - g.nq))
    if c.tr and c.stride > 1:
        cands.append(c._replace(op=1))
        cands.append(c._replace(op=1, Tin=c.Tin + tiles * step - 1 - g.nq))     # the padding column alone in the last tile's place
    if a.family == "kloop":                              # the K-loop rows stay within T <= 40 (16.8 MB of banks per row)
        cands = [t for t in cands if t.Tin <= 40]
    per = c.stride if c.tr else 1
    for rows_extra in (16, 8 * per):                     # M = whole row blocks + 16 (or the smallest step Cout allows)
        if rows_extra % per == 0 and (g.M + rows_extra) % a.rows:
            cands.append(c._replace(Cout=c.Cout + rows_extra // per))
    for t in cands:
        if t.Tin > 0 and t != c and t not in out and _selects(t, c.arm):
            out.append(t)
    if a.family == "mt":
        w = _walk_row(c)
        if w is not None and macs(w) <= MAX_MACS and w not in out:
            out.append(w)
    return out


def _build(table, dtypes):
    base, cases = [], []
    for dt in dtypes:
        seen = set()
        for shape in table:
            c = _mk(shape, dt)
            cases.append(c)
            if c.arm not in seen:                        # the first row of an arm is its base row and gets the ragged companions
                seen.add(c.arm)
                base.append(c)
                cases += [t for t in _companions(c) if t not in cases]
            elif c.tr and c.stride > 1 and not c.op:     # another route to the arm: its output_padding variant rides along
                t = c._replace(op=1)
                if _selects(t, c.arm) and t not in cases:
                    cases.append(t)
                if arm_of(c).family == "mt" and c.B == 1:            # and, for mt, its TL = 2 walk
                    w = _walk_row(c)
                    if w is not None and macs(w) <= MAX_MACS and w not in cases:
                        cases.append(w)
    return base, cases


_B16, _C16 = _build(_T16, (MV_BF16, MV_F16))
_B32, _C32 = _build(_T32, (MV_F32,))
BASE = _B16 + _B32                    # one row per arm: the smallest shape that selects it
CASES = _C16 + _C32                   # every row with its companions


def impulse_ok(c):
    """A row the impulse tests can run on: see IMPULSE in the module docstring."""
    a, g = arm_of(c), geom_of(c)
    if not (c.B > 1 and c.Cin >= 16 and g.M > a.rows):
        return False
    if a.family == "mt":
        return a.walk == 2 and g.nq > a.cols * a.walk
    if a.family == "stream":
        return a.walk > 1 and a.grid[0] > 1
    if a.family == "cl" and a.S == 2:
        return True                                      # (sequences of at most 48 columns: one tile)
    return g.nq > col_step(a)


def _impulse_rows():
    rows = []
    for b in BASE:
        ok = [c for c in CASES if c.arm == b.arm and impulse_ok(c)]
        if not ok:
            raise AssertionError(f"no impulse row for {b.arm}")
        rows.append(min(ok, key=macs))
    return rows


IMPULSE = _impulse_rows()


# ----------------------------------------------------------------------------------------------- generators (channels-last, float64)
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def nnz_of(ntaps):
    """Non-zero channels per time step: 8 terms per output element over all taps."""
    return max(1, 8 // ntaps)


def sparse_x(B, Tin, Cin, nnz, seed):
    """[B, Tin, Cin] in {-1, 0, 1} with exactly nnz non-zero channels per time step, drawn per step."""
    g = _gen(seed)
    n = B * Tin
    idx = torch.rand(n, Cin, generator=g).argsort(1)[:, :nnz]
    sign = torch.randint(0, 2, (n, nnz), generator=g).double() * 2 - 1
    x = torch.zeros(n, Cin, dtype=torch.float64)
    x.scatter_(1, idx, sign)
    return x.view(B, Tin, Cin)


def int_alpha(B, K):
    """alpha [B, K] of integers: 2 (odd samples) or 1 on bank b % K, -1 on the next bank (K > 1): sum |alpha| <= 3."""
    a = torch.zeros(B, K, dtype=torch.float64)
    for b in range(B):
        a[b, b % K] = 2.0 if b % 2 else 1.0
        if K > 1:
            a[b, (b + 1) % K] = -1.0
    return a


def inputs(shape):
    """x [B,Tin,Cin], banks [K,Cout,Cin,ks] (conv) / [K,Cin,Cout,ks] (transposed) in {-1,0,1}, bank biases [K,Cout] in -3..3, alpha."""
    B, Cin, Tin, Cout, ks, stride, pad, dil, tr, K, op = shape
    ntaps = ks // stride if tr else ks
    x = sparse_x(B, Tin, Cin, min(nnz_of(ntaps), Cin), 11)
    w = ints((K, Cin, Cout, ks) if tr else (K, Cout, Cin, ks), -1, 1, 12)
    return x, w, ints((K, Cout), -3, 3, 13), int_alpha(B, K)


# ----------------------------------------------------------------------------------------------- fp64 references
def odconv_ref(x_cl, w, alpha, shape, bias=None):
    """y [B,Tout,Cout] in float64: per sample b the (transposed) convolution with the mixed kernel sum_k alpha[b,k] w[k] plus the mixed
    bias sum_k alpha[b,k] bias[k] - as one grouped convolution over the batch."""
    B, Cin, Tin, Cout, ks, stride, pad, dil, tr, K, op = shape
    x = x_cl.double().transpose(1, 2).reshape(1, B * Cin, Tin)
    wb = torch.einsum("bk,k...->b...", alpha.double(), w.double())
    if tr:
        y = F.conv_transpose1d(x, wb.reshape(B * Cin, Cout, ks), None, stride=stride, padding=pad, output_padding=op, groups=B)
    else:
        y = F.conv1d(x, wb.reshape(B * Cout, Cin, ks), None, padding=pad, dilation=dil, groups=B)
    y = y.view(B, Cout, -1).transpose(1, 2).contiguous()
    if bias is not None:
        y = y + (alpha.double() @ bias.double()).unsqueeze(1)
    return y


@functools.lru_cache(maxsize=None)
def reference(shape):
    """(x, w, bias, alpha, y without bias) of a shape, computed once and shared by the dtypes, entry points and activation forms."""
    x, w, b, alpha = inputs(shape)
    return x, w, b, alpha, odconv_ref(x, w, alpha, shape)


def mixed_bias(alpha, bias):
    return (alpha.double() @ bias.double()).unsqueeze(1)


def film_F_of(Cout):
    """FiLM width of the exact tests: the last 8 channels pass through."""
    return max(8, Cout - 8)


def film_inputs(B, Cout, film_F):
    """film_proj [B, 2 film_F]: gamma in {-1, 1, 2}, beta in -3..3 (the kernel computes conv * gamma + beta on channels < film_F)."""
    gam = torch.tensor([-1.0, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (B, film_F), generator=_gen(14))]
    return torch.cat([gam, ints((B, film_F), -3, 3, 15)], 1)


def film_ref(y, film, film_F):
    out = y.clone()
    out[..., :film_F] = y[..., :film_F] * film[:, None, :film_F] + film[:, None, film_F:]
    return out


def pooled_ref(y):
    """Channel sums over time of the stored outputs [B, Cout]."""
    return y.sum(1)


# ----------------------------------------------------------------------------------------------- impulses
def column_edges(c, arm, g):
    """Input time steps on both sides of every column boundary the arm has: its column tile, and for mt the span of TL tiles one
    workgroup walks, for stream the span of a wave (tpw tiles) and of a workgroup (8 waves); the first and the last step."""
    steps = {col_step(arm)}                              # (kloop, sample: the 16-column MFMA blocks inside the one tile)
    if arm.family == "mt":
        steps.add(arm.cols * arm.walk)
    if arm.family == "stream":
        steps |= {16 * arm.walk, 16 * arm.walk * OS_NW}
    ts = {0, c.Tin - 1}
    for s in steps:
        for q in range(s, g.nq + 1, s):
            ts |= {q - 1, q}
    ts = sorted(t for t in ts if 0 <= t < c.Tin)
    if len(ts) > 48:                                     # long walks: the first, middle and last boundaries
        ts = sorted(set(ts[:16] + ts[len(ts) // 2 - 8:len(ts) // 2 + 8] + ts[-16:]))
    return ts


def channel_edges(c, arm):
    """Input channels on both sides of every 8-channel k-chunk boundary, which includes every 32-element k-step boundary and the
    K-loop's blocks of PD k-steps."""
    cs = {0, c.Cin - 1}
    for k in range(8, c.Cin, 8):
        cs |= {k - 1, k}
    return sorted(cs)


def x_impulses(c, arm, g):
    """(b, t, cin): every column edge at the first, a middle and the last channel of the last sample; every channel edge at one
    interior column of the last sample; the first element of the first sample."""
    b = c.B - 1
    ts = column_edges(c, arm, g)
    pts = {(0, 0, 0)}
    for t in ts:
        pts |= {(b, t, 0), (b, t, c.Cin - 1), (b, t, (c.Cin // 2) | 7)}
    tm = ts[len(ts) // 2]
    pts |= {(b, tm, ch) for ch in channel_edges(c, arm)}
    return sorted(pts)


def row_edges(arm, g):
    """GEMM rows: the first, the last, both sides of every row-block (workgroup) boundary and of the first M-tile boundary."""
    rs = {0, g.M - 1, 15, 16} if g.M > 16 else {0, g.M - 1}
    for r in range(arm.rows, g.M, arm.rows):
        rs |= {r - 1, r}
    return sorted(r for r in rs if r < g.M)


def gemm_row_to_weight_index(c, row):
    """(output channel, output phase) of a GEMM row: row = (r, o) for a transposed conv, o for a conv."""
    return (row % c.Cout, row // c.Cout) if c.tr else (row, 0)


def x_impulse_rows(c, g, wb, pt):
    """y of x = delta at pt = (b, t, cin) for the per-sample mixed kernels wb [B, ...]: a list of (output step u, y[b, u, :]), by indexing.
    Transposed: y[b, t * stride - pad + j, o] = wb[b, cin, o, j]; conv: y[b, t + pad - j * dil, o] = wb[b, o, cin, j]."""
    b, t, ch = pt
    rows = []
    for j in range(c.ks):
        u = t * c.stride - c.pad + j if c.tr else t + c.pad - j * c.dil
        if 0 <= u < g.Tout:
            rows.append((u, wb[b, ch, :, j] if c.tr else wb[b, :, ch, j]))
    return rows


def w_impulse_steps(c, g, j):
    """(u, t): output steps u and the input steps t they read through kernel tap j, as index tensors."""
    if c.tr:
        t = torch.arange(c.Tin)
        u = t * c.stride - c.pad + j
    else:
        u = torch.arange(g.Tout)
        t = u - c.pad + j * c.dil
    ok = (u >= 0) & (u < g.Tout) & (t >= 0) & (t < c.Tin)
    return u[ok], t[ok]


# ----------------------------------------------------------------------------------------------- real values, every element bounded
U = {MV_BF16: 2.0 ** -8, MV_F16: 2.0 ** -11, MV_F32: 2.0 ** -24}          # half an ulp of the storage significand
# fp32 storage, split operands: w = wh + wl + ew, x = xh + xl + ex with hi = bf16(v), lo = bf16(v - hi), both round-to-nearest:
# |v - hi| <= 2^-8 |v|, so |lo| <= 2^-8 (1 + 2^-8) |v| and |e| <= 2^-8 |v - hi| <= 2^-16 |v|.  The kernel adds wh xh + wh xl + wl xh; what
# is missing from w x is  wl xl + ew x + w ex - ew ex:  at most (2^-16 (1 + 2^-8)^2 + 2^-16 + 2^-16 + 2^-32) |w| |x| < (3 * 2^-16 + 2^-22)
# |w| |x|.  The mixed weight sum_k alpha_k W_k is formed in fp32 before the split; its K roundings are in the n 2^-24 A term.
C_OP = {MV_BF16: U[MV_BF16], MV_F16: U[MV_F16], MV_F32: 3 * 2.0 ** -16 + 2.0 ** -22}
# The streaming arms split into f16 pieces instead (hi = f16(v), lo = f16(v - hi)): the same derivation with 2^-11 per rounding gives
# 3 * 2^-22 + 2^-30 for fp32 rows (three products, lo * lo dropped) and 2^-22 for fp16 rows (x is exact: a_hi x + a_lo x, nothing dropped).
# The weight pieces are scaled by 2^6 and stay normal; the lo piece of an fp32 x is not scaled, and below 2^-14 it is an f16
# subnormal whose rounding is 2^-25 absolute rather than 2^-11 relative: OS_SUBNORMAL * sum |alpha_k| |W_k| is added for those rows.
C_STREAM = {0: 3 * 2.0 ** -22 + 2.0 ** -30, 1: 2.0 ** -22}             # by in_f16
OS_SUBNORMAL = 2.0 ** -25


def real_inputs(c, seed=41):
    """x ~ N(0,1) and the banks and bank biases of a real, default-initialised ODConv module (both N(0,1)), all rounded to the storage type of the
    case (fp16 x for an in_f16 case) - the exact values the kernel is handed - as float64.  alpha = softmax of random logits, as the
    module's attention produces it."""
    g = _gen(seed)
    sdt = TORCH_DT[c.dtype]
    rnd = lambda t, dt=sdt: t.to(dt).double()
    import hifigan_modified as H
    with torch.random.fork_rng(devices=[]):              # the module draws from the global generator: leave its state as it was
        torch.manual_seed(seed)
        if c.tr:
            m = H.ODConvTranspose1d(c.Cin, c.Cout, c.ks, stride=c.stride, padding=c.pad, output_padding=c.op, K=c.K)
        else:
            m = H.ODConv1d(c.Cin, c.Cout, c.ks, padding=c.pad, dilation=c.dil, K=c.K)
    w = rnd(m.kernels.detach())
    bias = rnd(m.bias.detach())
    x = rnd(torch.randn(c.B, c.Tin, c.Cin, generator=g), torch.float16 if c.in_f16 else sdt)
    alpha = torch.softmax(torch.randn(c.B, c.K, generator=g), 1).float().double()
    return x, w, bias, alpha


def real_bound(c, x, w, bias, alpha):
    """ref and the per-element bound  c_T A + u_T |ref| + n 2^-24 A  with  A = sum_k |alpha_k| (sum |W_k| |x| + |bias_k|) and
    n = taps * Cin + 2 K + 2 fp32 operations per element (the products' accumulation in any order, the K-term mixes of weight and
    bias, the bias add).  c_T = C_OP of the storage type, or C_STREAM for the streaming arms (plus their subnormal term).  One
    departure from a bound over the products alone: A carries |bias_k| as well, because the mixed bias is formed from K rounded
    products in fp32 and, in 16-bit storage, from the same rounded alpha-mix as the weights; it adds at most |bias| (c_T + n 2^-24).
    Derived, not measured; LeakyReLU is 1-Lipschitz and positively homogeneous, so it holds behind it."""
    shape = shape_of(c)
    ref = odconv_ref(x, w, alpha, shape, bias)
    A = odconv_ref(x.abs(), w.abs(), alpha.abs(), shape, bias.abs())
    n = geom_of(c).ntaps * c.Cin + 2 * c.K + 2
    if arm_of(c).family == "stream":
        slack = (C_STREAM[c.in_f16] + n * 2.0 ** -24) * A
        if not c.in_f16:
            slack = slack + OS_SUBNORMAL * odconv_ref(torch.ones_like(x), w.abs(), alpha.abs(), shape)
        return ref, A, slack
    return ref, A, (C_OP[c.dtype] + n * 2.0 ** -24) * A
