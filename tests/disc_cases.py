"""Case tables, input generators and fp64 references of tests/test_gpu_disc_kernels.py (a plain module, imported like
tests/embed_cases.py; checked on the host by tests/test_host_disc_cases.py).

The kernels under test are the channels-last discriminator convolutions of csrc/disc_fused.hip.  Their dispatchers pick one template
instantiation ("arm") from the shape, so the tables below hold, for every arm a valid shape can reach, the smallest shape that selects
it plus ragged companions that still select it.  `fwd_arm` / `wgrad_arm` restate the dispatchers' predicates in Python: they name the
arm of a shape and give its position tile, channel chunk and workgroup split, which the tests use to place impulses on both sides of
every boundary.  The restatement is an independent second statement on purpose: tests/test_host_disc_cases.py compares it, without a
GPU, with what the library itself plans (mv_dconv_cl_fwd_plan, mv_dconv_wgrad_plan) over a sweep of shapes and every row below.

Every input is made of small integers, so every sum is exact in fp32 in any order and every result is an integer (or a half-integer
after LeakyReLU with slope 0.5) of at most 8 significant bits: exactly representable in bf16, fp16 and fp32.  The GPU tests can then
ask for bit equality with the fp64 reference.

The tables hold every forward instantiation the library has: its dispatch table (dconv_fwd_arms16 / dconv_fwd_arms32 in
csrc/disc_fused.hip) lists the 16 arms per 16-bit type and the six fp32 arms below and no others.  Two groups of chunked tiles that no
shape can select are not instantiated: 256-row tiles with 64- or 32-channel chunks outside the nb8 form (256 rows need Cin == 128,
whose chunk is 128), and every 8-wave tile with 32-channel chunks (chunk 32 needs Cin == 32, and `use` is then true only when the
whole-Cin tile exceeds 160 KB - the same size as the chunk-32 tile, which is then refused too).
"""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

MV_F32, MV_BF16, MV_F16 = 0, 1, 2
MV_ERR_ARG, MV_ERR_DTYPE, MV_ERR_UNSUPPORTED = -1, -2, -3
TORCH_DT = {MV_F32: torch.float32, MV_BF16: torch.bfloat16, MV_F16: torch.float16}
DT_NAME = {MV_F32: "float", MV_BF16: "bf16", MV_F16: "f16"}
LDS_MAX = 160 * 1024
SLOPE = 0.5                      # LeakyReLU slope of the exact tests: halving an integer <= 243 keeps 8 significant bits


def cdiv(a, b):
    return -(-a // b)


def lds_row_stride(row_bytes, elem_size):
    """csrc/mfma.h: row stride of an LDS tile (conflict-free 16-bit fragment reads)."""
    if elem_size != 2:
        return row_bytes + 16
    for pad in range(16, 129, 16):
        if (row_bytes + pad) % 128 in (32, 96):
            return row_bytes + pad
    return row_bytes + 16


class Refused(Exception):
    def __init__(self, code):
        super().__init__(code)
        self.code = code


# ----------------------------------------------------------------------------------------------- forward dispatcher
Arm = namedtuple("Arm", "name npos cchunk rows")     # position tile along W, input channels staged at a time, output rows per workgroup


def _whole(T, MW, NB, Cin, Cout, kh, kw, dil):
    """dconv_cl_kernel<T,4,MW,NB>: the whole-Cin tile."""
    xb = kh * (NB * 16 + (kw - 1) * dil) * lds_row_stride(Cin * 2, 2)
    ob = NB * 16 * (4 * MW * 16 * 2 + 16)
    if max(xb, ob) > LDS_MAX or Cin * 2 // 16 > 256:
        return None
    return Arm(f"dconv_cl_kernel<{T},4,{MW},{NB}>", NB * 16, Cin, 4 * MW * 16)


def fwd_arm(B, H, W, Cin, Cout, kh, kw, dil, dtype):
    """The instantiation dconv_fwd_plan names for this shape (mv_dconv_cl_fwd: no fused head), or Refused(code)."""
    if not (B > 0 and H > 0 and W > 0 and Cin % 32 == 0 and Cout % 16 == 0 and kh & 1 and kw & 1):
        raise Refused(MV_ERR_ARG)
    if not (dil >= 1 and (kw - 1) * dil <= 128):
        raise Refused(MV_ERR_ARG)
    halo = (kw - 1) * dil
    if dtype == MV_F32:
        if B * H > 65535:
            raise Refused(MV_ERR_UNSUPPORTED)
        cch = 64 if (kh == 1 and Cin % 64 == 0) else 32
        rows = 128 if Cout >= 128 else (64 if Cout >= 64 else 32)
        if max(2 * kh * (128 + halo) * lds_row_stride(cch * 2, 2), 128 * (rows * 4 + 16)) > LDS_MAX:
            raise Refused(MV_ERR_UNSUPPORTED)
        return Arm(f"dconv_cl_wide_kernel<float,2,{rows // 32},4,{cch},4>", 128, cch, rows)
    T = DT_NAME[dtype]
    if B * H <= 65535:
        full = kh * (128 + halo) * lds_row_stride(Cin * 2, 2)
        big3x3 = kh == 3 and Cin == 128 and Cout >= 256
        use = (full > LDS_MAX or Cin > 128 or (kh == 3 and Cin >= 64 and Cout <= 128) or (kh == 1 and Cin == 64 and Cout == 32) or big3x3)
        nb8 = kh == 3 and Cin % 64 == 0 and Cin >= 128 and Cout >= 128 and W >= 256
        if kh == 3 and Cin % 64 == 0 and Cout % 256 == 0 and W >= 128:
            return Arm(f"dconv_cl_wide_kernel<{T},1,4,8,64,4>", 128, 64, 256)
        if kh == 3 and Cin >= 128 and Cout == 128 and W >= 128:
            return Arm(f"dconv_cl_wide_kernel<{T},1,4,8,32,2>", 128, 32, 128)
        npos = 256 if nb8 else 128
        cchunk = 64 if nb8 else (128 if Cin > 128 else Cin)
        if use and Cin % cchunk == 0 and cchunk in (128, 64, 32):
            xb = kh * (npos + halo) * lds_row_stride(cchunk * 2, 2)
            rows = 256 if (big3x3 or (nb8 and Cout >= 256)) else 128 if Cout >= 128 else (64 if Cout >= 64 else 32)
            if not nb8 and not big3x3:
                while rows > 32 and cdiv(W, npos) * cdiv(Cout, rows) * B * H < 256:
                    rows >>= 1
            if max(xb, npos * (rows * 2 + 16)) <= LDS_MAX:
                if nb8:
                    return Arm(f"dconv_cl_wide_kernel<{T},2,{4 if rows == 256 else 2},8,64,8>", 256, 64, rows)
                ps, mw, nb = {256: (2, 4, 4), 128: (2, 2, 4), 64: (4, 2, 2), 32: (4, 1, 2)}[rows]
                return Arm(f"dconv_cl_wide_kernel<{T},{ps},{mw},{nb},{cchunk},8>", 128, cchunk, rows)
    if B * H > 65535:
        raise Refused(MV_ERR_UNSUPPORTED)
    if Cout >= 256:
        arm = _whole(T, 4, 8, Cin, Cout, kh, kw, dil)
    elif Cout >= 128:
        arm = _whole(T, 2, 8, Cin, Cout, kh, kw, dil) or _whole(T, 2, 4, Cin, Cout, kh, kw, dil)
    else:
        arm = _whole(T, 1, 8, Cin, Cout, kh, kw, dil) or _whole(T, 1, 4, Cin, Cout, kh, kw, dil)
    if arm is None:
        raise Refused(MV_ERR_UNSUPPORTED)
    return arm


# ----------------------------------------------------------------------------------------------- weight-gradient dispatcher
WArm = namedtuple("WArm", "name wt otile wsplit nchunks cpw groups rows_fastest")   # wt / otile: position / output-channel tile


def _split(nchunks, tiles):
    groups = max(1, 256 // tiles)
    groups = min(groups, nchunks)
    cpw = cdiv(nchunks, groups)
    return cpw, cdiv(nchunks, cpw)


def wgrad_arm(B, H, W, Cin, Cout, kh, kw, dil, dtype):
    """The instantiation mv_dconv_wgrad_cl / _pz launch, with its chunking: a chunk is WT positions of one image row, a workgroup
    (blockIdx.z) owns `cpw` consecutive chunks and keeps its accumulators across them."""
    arm = _wgrad_arm(B, H, W, Cin, Cout, kh, kw, dil, dtype)
    if arm.nchunks > 2 ** 30 or (arm.rows_fastest and B * arm.wsplit * (H + 2) > 2 ** 30):     # the kernels index chunks and staged rows with an int
        raise Refused(MV_ERR_UNSUPPORTED)
    return arm


def _wgrad_arm(B, H, W, Cin, Cout, kh, kw, dil, dtype):
    if not (B > 0 and H > 0 and W > 0 and Cin % 8 == 0 and Cout % 8 == 0 and dil >= 1):
        raise Refused(MV_ERR_ARG)
    if dtype == MV_F32:
        if not (dil == 1 and ((kh, kw) == (3, 3) or (kh, kw) == (1, 15))):
            raise Refused(MV_ERR_UNSUPPORTED)
        wt = 64 if kh == 1 else 32
        ws = cdiv(W, wt)
        cpw, groups = _split(B * H * ws, cdiv(Cin, 64) * cdiv(Cout, 64))
        return WArm(f"dconv_wgrad_kernel<float,{kh},{kw},{wt}>", wt, 64, ws, B * H * ws, cpw, groups, False)
    T = DT_NAME[dtype]
    if (kh, kw) == (3, 3):
        if dil != 1:
            raise Refused(MV_ERR_UNSUPPORTED)
        mo = 4 if Cout >= 128 else 2
        ws = cdiv(W, 64)
        cpw, groups = _split(B * H * ws, cdiv(Cin, 64) * cdiv(Cout, 32 * mo))
        return WArm(f"dconv_wgrad3_kernel<{T},{mo}>", 64, 32 * mo, ws, B * H * ws, cpw, groups, True)     # chunk = (sample, strip, row)
    if kh != 1 or kw not in (1, 3, 5, 7, 11, 15) or (kw - 1) * dil > 64:
        raise Refused(MV_ERR_UNSUPPORTED)
    ws = cdiv(W, 128)
    cpw, groups = _split(B * H * ws, cdiv(Cin, 64) * cdiv(Cout, 64))
    return WArm(f"dconv_wgrad_kernel<{T},1,{kw},128>", 128, 64, ws, B * H * ws, cpw, groups, False)


def wgrad_chunk_origin(arm, H, chunk):
    """(b, h, w0) of a chunk index."""
    if arm.rows_fastest:
        st, h = divmod(chunk, H)
        b, wc = divmod(st, arm.wsplit)
    else:
        bh, wc = divmod(chunk, arm.wsplit)
        b, h = divmod(bh, H)
    return b, h, wc * arm.wt


# ----------------------------------------------------------------------------------------------- case tables
Case = namedtuple("Case", "arm B H W Cin Cout kh kw dil dtype")

MAX_MACS = 6e9          # ragged companions above this many multiply-adds are left out; hand-written rows are exempt (the 17 MB k15
                        # row is 16.7 GMAC: 1.6 s of fp64 reference on 8 cores, shared by both 16-bit types)


def case_id(c):
    return f"{c.arm}-B{c.B}H{c.H}W{c.W}-{c.Cin}to{c.Cout}-{c.kh}x{c.kw}d{c.dil}"


# (B, H, W, Cin, Cout, kh, kw, dil) of the smallest shape that selects each 16-bit forward arm (T = bf16 and f16), arm name beside it
_FWD16 = [
    ("dconv_cl_wide_kernel<T,1,4,8,64,4>", (1, 2, 128, 64, 256, 3, 3, 1)),       # direct: 3x3, Cout % 256 == 0, W >= 128
    ("dconv_cl_wide_kernel<T,1,4,8,32,2>", (1, 2, 128, 128, 128, 3, 3, 1)),      # direct: 3x3, Cin >= 128, Cout == 128, W >= 128
    ("dconv_cl_wide_kernel<T,2,4,8,64,8>", (1, 2, 256, 128, 384, 3, 3, 1)),      # nb8, 256 rows: second row tile half empty
    ("dconv_cl_wide_kernel<T,2,2,8,64,8>", (1, 2, 256, 192, 192, 3, 3, 1)),      # nb8, 128 rows: second row tile half empty
    ("dconv_cl_wide_kernel<T,2,4,4,128,8>", (1, 2, 100, 128, 256, 3, 3, 1)),     # big3x3 below W = 128
    ("dconv_cl_wide_kernel<T,2,2,4,128,8>", (24, 11, 5, 128, 128, 3, 3, 1)),     # 128 rows kept: 264 workgroups
    ("dconv_cl_wide_kernel<T,2,2,4,128,8>", (24, 11, 5, 256, 128, 3, 3, 1)),     # the same with two channel chunks
    ("dconv_cl_wide_kernel<T,2,2,4,128,8>", (24, 11, 5, 256, 128, 1, 15, 1)),    # k15 rows narrower than the halo
    ("dconv_cl_wide_kernel<T,2,2,4,128,8>", (24, 1, 1413, 256, 128, 1, 15, 1)),  # k15 at full tiles (17 MB of input, the largest case)
    ("dconv_cl_wide_kernel<T,4,2,2,128,8>", (24, 11, 5, 128, 64, 3, 3, 1)),
    ("dconv_cl_wide_kernel<T,4,2,2,128,8>", (12, 11, 5, 128, 128, 3, 3, 1)),     # halved once: 132 workgroups of 128 rows, 264 of 64
    ("dconv_cl_wide_kernel<T,4,1,2,128,8>", (1, 1, 130, 256, 32, 1, 15, 1)),
    ("dconv_cl_wide_kernel<T,4,1,2,128,8>", (1, 1, 130, 256, 128, 1, 15, 1)),    # a short sequence after the halving loop (128 -> 32)
    ("dconv_cl_wide_kernel<T,2,2,4,64,8>", (24, 11, 5, 64, 128, 3, 3, 1)),
    ("dconv_cl_wide_kernel<T,4,2,2,64,8>", (24, 11, 5, 64, 64, 3, 3, 1)),
    ("dconv_cl_wide_kernel<T,4,1,2,64,8>", (1, 1, 130, 64, 32, 1, 15, 1)),       # kh == 1, 64 -> 32
    ("dconv_cl_wide_kernel<T,4,1,2,64,8>", (1, 2, 130, 64, 128, 3, 3, 1)),       # halved 128 -> 32
    ("dconv_cl_kernel<T,4,4,8>", (1, 1, 130, 32, 256, 1, 15, 1)),
    ("dconv_cl_kernel<T,4,4,8>", (1, 2, 100, 192, 256, 3, 3, 1)),                # Cin % 128 != 0 falls through to the whole-Cin tile
    ("dconv_cl_kernel<T,4,2,8>", (1, 1, 130, 32, 128, 1, 3, 1)),
    ("dconv_cl_kernel<T,4,1,8>", (1, 1, 130, 32, 16, 1, 1, 1)),
    ("dconv_cl_kernel<T,4,1,8>", (1, 2, 130, 96, 64, 3, 3, 1)),                  # Cin = 96 is no chunk size
    ("dconv_cl_kernel<T,4,2,4>", (1, 2, 100, 192, 160, 3, 3, 2)),                # 3 x 132 x 416 B > 160 KB: the 4-block tile
    ("dconv_cl_kernel<T,4,1,4>", (1, 2, 100, 192, 64, 3, 3, 2)),
    ("dconv_cl_kernel<T,4,1,4>", (1, 2, 70, 96, 48, 3, 3, 58)),                  # 3 x 244 x 224 B > 160 KB; W smaller than the halo
]
# the six split-operand fp32 arms: rows 128 / 64 / 32 x chunk 64 (one-row kernels, Cin % 64 == 0) / 32
_FWD32 = [
    ("dconv_cl_wide_kernel<float,2,4,4,64,4>", (1, 1, 130, 64, 128, 1, 15, 1)),
    ("dconv_cl_wide_kernel<float,2,2,4,64,4>", (1, 1, 130, 64, 64, 1, 15, 1)),
    ("dconv_cl_wide_kernel<float,2,1,4,64,4>", (1, 1, 130, 128, 16, 1, 15, 1)),  # half-empty 32-row tile
    ("dconv_cl_wide_kernel<float,2,4,4,32,4>", (1, 2, 130, 64, 144, 3, 3, 1)),   # second row tile holds one M-tile
    ("dconv_cl_wide_kernel<float,2,2,4,32,4>", (1, 2, 130, 32, 64, 3, 3, 1)),
    ("dconv_cl_wide_kernel<float,2,1,4,32,4>", (1, 1, 130, 96, 32, 1, 15, 1)),   # one-row kernel whose Cin is no multiple of 64
]


def _macs(s):
    B, H, W, Cin, Cout, kh, kw, _ = s
    return B * H * W * Cin * Cout * kh * kw


def _companions(shape, arm_of, tile):
    """Ragged variants of a base shape, one dimension at a time, that still select the base shape's arm: W in {1, one side of the
    halo, 127, 128, 129, one past the position tile}, H in {1, 2, 11}, B in {1, 3}."""
    B, H, W, Cin, Cout, kh, kw, dil = shape
    base = arm_of(shape)
    pw = (kw // 2) * dil
    out = []
    cands = [(B, H, w) for w in (1, pw if pw >= 2 else 0, 127, 128, 129, tile + 1) if w > 0]
    cands += [(B, h, W) for h in (1, 2, 11)] + [(b, H, W) for b in (1, 3)]
    for b, h, w in cands:
        s = (b, h, w, Cin, Cout, kh, kw, dil)
        if s == shape or s in out or _macs(s) > MAX_MACS:
            continue
        try:
            if arm_of(s) == base:
                out.append(s)
        except Refused:
            pass
    return out


def _expand(table, dtypes, arm_fn, tile_of, with_companions=lambda name, shape: True):
    cases = []
    for dt in dtypes:
        for name, shape in table:
            arm_of = lambda s, dt=dt: arm_fn(*s, dt).name
            real = name.replace("<T,", f"<{DT_NAME[dt]},")
            extra = _companions(shape, arm_of, tile_of(arm_fn(*shape, dt))) if with_companions(name, shape) else []
            for s in [shape] + extra:
                cases.append(Case(real, *s, dt))
    return cases


FWD_BASE = [Case(n.replace("<T,", f"<{DT_NAME[dt]},"), *s, dt) for dt in (MV_BF16, MV_F16) for n, s in _FWD16] + \
           [Case(n, *s, MV_F32) for n, s in _FWD32]
FWD_CASES = _expand(_FWD16, (MV_BF16, MV_F16), fwd_arm, lambda a: a.npos) + _expand(_FWD32, (MV_F32,), fwd_arm, lambda a: a.npos)

# Weight gradients.  16-bit: the two 3x3 forms (MO = 2 below 128 output channels, 4 from there) and the 1xk kernel for every k; fp32:
# 3x3 and 1x15.  The FIRST row of every arm gets the ragged companions of _companions (W = 1 and H = 1 among them: a strip narrower
# than the halo, no neighbouring rows); its channel counts are no multiples of 64 (24, 40, 72, 136: partly empty channel tiles).
# The rows behind it are taken as they stand:
#   * "split" rows, whose many channel tiles leave few workgroups along the positions, so a workgroup owns several chunks and keeps
#     its accumulators across them: cpw = 2 with a short last workgroup, and deep ones - cpw >= 9 for the 3x3 kernel (its ring of 8 x-row
#     slots wraps, and the walk crosses strips and samples), cpw >= 3 for the double-buffered 1xk and fp32 kernels (a buffer is
#     refilled after it was read).  wgrad_arm gives cpw; test_host_disc_cases.py asserts that these rows exist for every kernel.
#   * for the 1xk kernel, the dilations 3, 5 and the largest with (k - 1) * dil <= 64.
_KDIL = {1: (3, 5), 3: (3, 5, 32), 5: (3, 5, 16), 7: (3, 5, 10), 11: (3, 5, 6), 15: (3, 4)}
_WG16 = [
    ("dconv_wgrad3_kernel<T,2>", (3, 2, 129, 24, 40, 3, 3, 1)),
    ("dconv_wgrad3_kernel<T,2>", (3, 5, 129, 256, 96, 3, 3, 1)),       # split: 45 chunks in pairs
    ("dconv_wgrad3_kernel<T,2>", (3, 11, 321, 512, 96, 3, 3, 1)),      # deep split: 198 chunks, 13 per workgroup
    ("dconv_wgrad3_kernel<T,4>", (3, 2, 129, 72, 136, 3, 3, 1)),
    ("dconv_wgrad3_kernel<T,4>", (3, 5, 129, 256, 256, 3, 3, 1)),      # split: 45 chunks in pairs
    ("dconv_wgrad3_kernel<T,4>", (3, 11, 65, 512, 512, 3, 3, 1)),      # deep split: 66 chunks, 9 per workgroup
    ("dconv_wgrad_kernel<T,1,15,128>", (3, 2, 129, 72, 40, 1, 15, 1)),
    ("dconv_wgrad_kernel<T,1,15,128>", (3, 1, 800, 256, 256, 1, 15, 1)),   # split: 21 chunks in pairs
    ("dconv_wgrad_kernel<T,1,15,128>", (2, 1, 2076, 256, 256, 1, 15, 1)),  # deep split: 34 chunks, 3 per workgroup
    ("dconv_wgrad_kernel<T,1,3,128>", (3, 2, 129, 72, 40, 1, 3, 1)),
    ("dconv_wgrad_kernel<T,1,3,128>", (3, 1, 600, 256, 264, 1, 3, 5)),     # split with a partly empty Cout tile
    ("dconv_wgrad_kernel<T,1,3,128>", (2, 1, 2076, 256, 256, 1, 3, 1)),    # deep split
]
for _k in (1, 5, 7, 11):
    _WG16.append((f"dconv_wgrad_kernel<T,1,{_k},128>", (3, 2, 129, 72, 40, 1, _k, 1)))
    _WG16.append((f"dconv_wgrad_kernel<T,1,{_k},128>", (2, 1, 2076, 256, 256, 1, _k, 1)))     # deep split
for _k, _dils in _KDIL.items():
    for _d in _dils:
        _WG16.append((f"dconv_wgrad_kernel<T,1,{_k},128>", (3, 2, 129, 72, 40, 1, _k, _d)))
_WG32 = [
    ("dconv_wgrad_kernel<float,3,3,32>", (3, 2, 65, 24, 72, 3, 3, 1)),
    ("dconv_wgrad_kernel<float,3,3,32>", (3, 3, 65, 256, 256, 3, 3, 1)),     # split: 27 chunks in pairs
    ("dconv_wgrad_kernel<float,3,3,32>", (2, 5, 100, 256, 256, 3, 3, 1)),    # deep split: 40 chunks, 3 per workgroup
    ("dconv_wgrad_kernel<float,1,15,64>", (3, 2, 129, 40, 24, 1, 15, 1)),
    ("dconv_wgrad_kernel<float,1,15,64>", (3, 1, 400, 256, 256, 1, 15, 1)),  # split: 21 chunks in pairs
    ("dconv_wgrad_kernel<float,1,15,64>", (2, 1, 1040, 256, 256, 1, 15, 1)), # deep split: 34 chunks, 3 per workgroup
]


def _first_of_arm(table):
    seen = set()
    return {(n, s) for n, s in table if not (n in seen or seen.add(n))}


_WG_FIRST16, _WG_FIRST32 = _first_of_arm(_WG16), _first_of_arm(_WG32)
WGRAD_CASES = _expand(_WG16, (MV_BF16, MV_F16), wgrad_arm, lambda a: a.wt, lambda n, s: (n, s) in _WG_FIRST16) + \
              _expand(_WG32, (MV_F32,), wgrad_arm, lambda a: a.wt, lambda n, s: (n, s) in _WG_FIRST32)


def wgrad_split(c):
    """(cpw, ragged): chunks per workgroup of a weight-gradient row, and whether the split is ragged - the last workgroup carries
    fewer chunks and some workgroup's chunks belong to two samples."""
    a = wgrad_arm(*shape_of(c), c.dtype)
    per_sample = a.nchunks // c.B
    crosses = any((g * a.cpw) // per_sample != (min((g + 1) * a.cpw, a.nchunks) - 1) // per_sample for g in range(a.groups))
    return a.cpw, a.nchunks % a.cpw != 0 and crosses


# ----------------------------------------------------------------------------------------------- generators (channels-last, float64)
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def sparse_signs(shape, C, seed, nnz=8):
    """[*shape, C] in {-1, 0, 1} with exactly `nnz` non-zero channels at every position, the channels drawn per position."""
    g = _gen(seed)
    n = 1
    for s in shape:
        n *= s
    idx = torch.rand(n, C, generator=g).argsort(1)[:, :nnz]
    sign = torch.randint(0, 2, (n, nnz), generator=g).double() * 2 - 1
    x = torch.zeros(n, C, dtype=torch.float64)
    x.scatter_(1, idx, sign)
    return x.view(*shape, C)


def ints(shape, lo, hi, seed):
    """Uniform integers in [lo, hi] as float64."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=_gen(seed)).double()


def signed_zero_save(shape, seed):
    """A saved activation with entries from {-2, -1, -0.0, +0.0, 1, 2}: LeakyReLU'(save) = 1 where save >= 0 under the IEEE comparison,
    which -0.0 passes."""
    vals = torch.tensor([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0], dtype=torch.float64)
    return vals[torch.randint(0, 6, tuple(shape), generator=_gen(seed))]


def fwd_inputs(c):
    """x [B,H,W,Cin] sparse signs, w [Cout,Cin,kh,kw] in -2..2, bias [Cout] in -3..3."""
    return (sparse_signs((c.B, c.H, c.W), c.Cin, 11), ints((c.Cout, c.Cin, c.kh, c.kw), -2, 2, 12), ints((c.Cout,), -3, 3, 13))


def dgrad_inputs(c):
    """The act_save form on the same kernel shape: g [B,H,W,Cin] is the gradient w.r.t. the output of a layer with weight
    wl [Cin, Cout, kh, kw] (the kernel's Cin is the layer's Cout), save [B,H,W,Cout] the layer's saved input activation."""
    return (sparse_signs((c.B, c.H, c.W), c.Cin, 21), ints((c.Cin, c.Cout, c.kh, c.kw), -2, 2, 22),
            signed_zero_save((c.B, c.H, c.W, c.Cout), 23))


def wgrad_inputs(c):
    return ints((c.B, c.H, c.W, c.Cin), -1, 1, 31), ints((c.B, c.H, c.W, c.Cout), -1, 1, 32)


# ----------------------------------------------------------------------------------------------- fp64 references
def conv_ref(x_cl, w, bias, dil):
    """Channels-last "same" convolution, stride 1, dilation (1, dil), in float64 on the CPU."""
    kh, kw = w.shape[2:]
    y = F.conv2d(x_cl.double().permute(0, 3, 1, 2), w.double(), None if bias is None else bias.double(), padding=(kh // 2, (kw // 2) * dil),
                 dilation=(1, dil))
    return y.permute(0, 2, 3, 1).contiguous()


def lrelu(v, slope):
    return torch.where(v >= 0, v, v * slope)


def dgrad_ref(g_cl, wl, save, slope, dil):
    """LeakyReLU'(save) * conv^T(g): the transposed convolution written as a convolution with flipped taps and swapped channels."""
    gx = conv_ref(g_cl, wl.flip(2, 3).transpose(0, 1).contiguous(), None, dil)
    return torch.where(save >= 0, gx, gx * slope)


def wgrad_ref(x_cl, g_cl, kh, kw, dil):
    Cin, Cout = x_cl.shape[3], g_cl.shape[3]
    gw = torch.nn.grad.conv2d_weight(x_cl.double().permute(0, 3, 1, 2), (Cout, Cin, kh, kw), g_cl.double().permute(0, 3, 1, 2),
                                     padding=(kh // 2, (kw // 2) * dil), dilation=(1, dil))
    return gw, g_cl.double().sum((0, 1, 2))


@functools.lru_cache(maxsize=None)
def fwd_reference(shape):
    """(x, w, bias, ref without bias) of a forward shape, computed once and shared by the dtypes and activation forms."""
    c = Case("", *shape, 0)
    x, w, b = fwd_inputs(c)
    return x, w, b, conv_ref(x, w, None, c.dil)


@functools.lru_cache(maxsize=None)
def dgrad_reference(shape):
    c = Case("", *shape, 0)
    g, wl, save = dgrad_inputs(c)
    return g, wl, save, dgrad_ref(g, wl, save, SLOPE, c.dil)


@functools.lru_cache(maxsize=None)
def wgrad_reference(shape):
    c = Case("", *shape, 0)
    x, g = wgrad_inputs(c)
    return (x, g) + wgrad_ref(x, g, c.kh, c.kw, c.dil)


def shape_of(c):
    return tuple(c[1:9])


# ----------------------------------------------------------------------------------------------- impulses
def fwd_impulses(c, arm):
    """(b, h, w, cin) of single non-zero inputs: the corners and both sides of every position-tile and channel-chunk boundary."""
    ws = {0, c.W - 1} | {w for w in (arm.npos - 1, arm.npos) if w < c.W}
    cs = {0, c.Cin - 1} | {k for k in (arm.cchunk - 1, arm.cchunk) if k < c.Cin}
    pts = [(0, 0, 0, 0), (c.B - 1, c.H - 1, c.W - 1, c.Cin - 1)]
    pts += [(c.B - 1, 0, w, ch) for w in sorted(ws) for ch in sorted(cs)]
    return sorted(set(pts))


def fwd_impulse_expected(c, w, pt):
    """y of x = delta at pt: y[b, h - dh, w - dw*dil, o] = w[o, cin, ih, iw] with (dh, dw) = (ih - kh/2, iw - kw/2), by indexing."""
    b, h, wq, ch = pt
    y = torch.zeros(c.B, c.H, c.W, c.Cout, dtype=torch.float64)
    for ih in range(c.kh):
        for iw in range(c.kw):
            hh, ww = h - (ih - c.kh // 2), wq - (iw - c.kw // 2) * c.dil
            if 0 <= hh < c.H and 0 <= ww < c.W:
                y[b, hh, ww] = w[:, ch, ih, iw]
    return y


def wgrad_impulses(c, arm):
    """(b, h, w, cout) of single non-zero output gradients: the corners; both sides of the position tile, of the output-channel tile
    and of the sample boundary; both sides of the first workgroup boundary (last position of chunk cpw - 1, first of chunk cpw)."""
    pts = {(0, 0, 0, 0), (c.B - 1, c.H - 1, c.W - 1, c.Cout - 1)}
    for w in (arm.wt - 1, arm.wt):
        if w < c.W:
            pts.add((0, c.H - 1, w, c.Cout // 2))
    for o in (arm.otile - 1, arm.otile):
        if o < c.Cout:
            pts.add((0, 0, c.W // 2, o))
    if c.B > 1:
        pts |= {(0, c.H - 1, c.W - 1, 2), (1, 0, 0, 2)}
    if arm.groups > 1:
        b, h, w0 = wgrad_chunk_origin(arm, c.H, arm.cpw - 1)
        pts.add((b, h, min(w0 + arm.wt, c.W) - 1, 1))
        b, h, w0 = wgrad_chunk_origin(arm, c.H, arm.cpw)
        pts.add((b, h, w0, 1))
    return sorted(pts)


def wgrad_impulse_expected(c, x, pt):
    """gw of g = delta at pt: gw[o, :, ih, iw] = x[b, h + ih - kh/2, w + (iw - kw/2)*dil, :] (the shifted x row), zero elsewhere."""
    b, h, wq, o = pt
    gw = torch.zeros(c.Cout, c.Cin, c.kh, c.kw, dtype=torch.float64)
    for ih in range(c.kh):
        for iw in range(c.kw):
            hh, ww = h + ih - c.kh // 2, wq + (iw - c.kw // 2) * c.dil
            if 0 <= hh < c.H and 0 <= ww < c.W:
                gw[o, :, ih, iw] = x[b, hh, ww]
    return gw


# ----------------------------------------------------------------------------------------------- real-valued forward cases
def real_inputs(c, scale, torch_dtype):
    """x ~ N(0,1) * scale, w ~ N(0, 1/(Cin kh kw)), bias ~ 0.1 N(0,1), all rounded to the storage type (returned as float64)."""
    g = _gen(41)
    rnd = lambda t: t.to(torch_dtype).double()
    x = rnd(torch.randn(c.B, c.H, c.W, c.Cin, generator=g) * scale)
    w = rnd(torch.randn(c.Cout, c.Cin, c.kh, c.kw, generator=g) / (c.Cin * c.kh * c.kw) ** 0.5)
    b = rnd(torch.randn(c.Cout, generator=g) * 0.1)
    return x, w, b


def real_bound(x, w, b, dil):
    """ref = the fp64 convolution of the (already rounded) operands, and the format-independent part of the per-element bound
    u |act(ref)| + n 2^-23 A + 2^-24:  A = the same convolution of absolute values plus |b|, n = Cin kh kw + 1 terms, so the middle
    term is twice the worst-case fp32 summation error in any order; the last covers fp16 subnormal outputs.  The test adds the
    storage term u |act(ref)| (u = half an ulp of the significand); LeakyReLU is 1-Lipschitz, so the bound holds behind it."""
    ref = conv_ref(x, w, b, dil)
    A = conv_ref(x.abs(), w.abs(), b.abs(), dil)
    n = w.shape[1] * w.shape[2] * w.shape[3] + 1
    return ref, n * 2.0 ** -23 * A + 2.0 ** -24


# ----------------------------------------------------------------------------------------------- one-channel layers
def head_ref(x_cl, w, bias):
    """256 -> 1 head: y [B,H,W] = bias + conv(x [B,H,W,C], w [1,C,kh,kw])."""
    return conv_ref(x_cl, w, bias, 1)[..., 0]


def head_dgrad_ref(gy, w, save, slope):
    """gx [B,H,W,C] = LeakyReLU'(save) * conv^T(gy [B,H,W], w [1,C,kh,kw])."""
    return dgrad_ref(gy.unsqueeze(-1), w, save, slope, 1)


def head_wgrad_ref(gy, x_cl, kh, kw):
    """gw [kh*kw][C] (tap-major, as mv_dhead_wgrad writes it) and gb."""
    gw, gb = wgrad_ref(x_cl, gy.unsqueeze(-1), kh, kw, 1)
    return gw[0].reshape(x_cl.shape[3], kh * kw).t().contiguous(), gb


def first_ref(x0, w, bias, slope):
    """1 -> C1 first layer with LeakyReLU: a1 [B,H,W,C1]; w [C1,1,kh,kw]."""
    return lrelu(conv_ref(x0.unsqueeze(-1), w, bias, 1), slope)


def first_dgrad_ref(g1, w):
    return conv_ref(g1, w.flip(2, 3).transpose(0, 1).contiguous(), None, 1)[..., 0]


def first_wgrad_ref(g1, x0, kh, kw):
    gw, gb = wgrad_ref(x0.unsqueeze(-1), g1, kh, kw, 1)
    return gw.reshape(g1.shape[3], kh * kw), gb


def tap_shift_sum(z, kh, kw):
    """mv_dhead_sum without the bias: y[b,h,w] = sum over taps of z[tap][b, h + dh, w + dw] where that position is inside the image."""
    _, B, H, W = z.shape
    y = torch.zeros(B, H, W, dtype=torch.float64)
    for ih in range(kh):
        for iw in range(kw):
            dh, dw = ih - kh // 2, iw - kw // 2
            h_lo, h_hi, w_lo, w_hi = max(0, -dh), min(H, H - dh), max(0, -dw), min(W, W - dw)
            if h_lo < h_hi and w_lo < w_hi:
                y[:, h_lo:h_hi, w_lo:w_hi] += z[ih * kw + iw][:, h_lo + dh:h_hi + dh, w_lo + dw:w_hi + dw]
    return y


def tap_matrix_ref(sc, kh, kw, flip):
    """out [B,H,W,16]: out[pos][tap] = sc[pos + off(tap)] (flip 0) or sc[pos - off(tap)] (flip 1), zero outside and for tap >= kh*kw."""
    B, H, W = sc.shape
    out = torch.zeros(B, H, W, 16, dtype=torch.float64)
    for ih in range(kh):
        for iw in range(kw):
            dh, dw = ih - kh // 2, iw - kw // 2
            if flip:
                dh, dw = -dh, -dw
            for h in range(H):
                if not 0 <= h + dh < H:
                    continue
                w_lo, w_hi = max(0, -dw), min(W, W - dw)
                if w_lo < w_hi:
                    out[:, h, w_lo:w_hi, ih * kw + iw] = sc[:, h + dh, w_lo + dw:w_hi + dw]
    return out
