"""Case tables, fp64 references and dispatcher restatements of tests/test_gpu_front_kernels.py (a plain module like
tests/backward_cases.py, whose generators and `Out` it reuses; checked on the host by tests/test_host_front_cases.py).

The kernels under test are csrc/norm_elem.hip (ODConv attention, generator prologue, GroupNorm, FiLM, scale-shift, activations, avg-pool,
MPD fold, layout transposes, casts, the dense layer, the GRC+LoRA fold) and csrc/conv_generic.hip (mv_conv1d_fwd,
mv_conv_transpose1d_fwd, mv_conv2d_fwd), each entry point called on its own through the C ABI.

Operands are small integers (x in [-4, 4], weights in [-3, 3]), attention rows are multiples of 1/8 that sum to 1, scalars are dyadic
(LeakyReLU slope 1/4, mask_scale 2, GroupNorm mean an integer and rstd a power of two where mv_groupnorm_apply takes them as inputs).
Every term of every sum is then a multiple of a power of two `unit`, and while sum|terms| / unit < 2^24 the fp32 result is exact in any
order, with or without fused multiply-adds.  A result written in a 16-bit type is the one RNE rounding of that exact value, which is
what torch's own conversion of the fp64 reference gives (`stored`): 16-bit outputs are bit-exact too.

Four device functions are not exactly rounded: rsqrtf, expf, tanhf and v / (1 + __expf(-v)).  Outputs behind one of them carry the bound
    u_out |ref| + k 2^-24 sum|terms| + 4 E_FN[fn] |f|
with E_FN the largest relative error of the function measured on an MI355X over the rows' argument range (tools/measure_device_fn.hip;
DESIGN.md lists the figures), |f| the function value scaled by what multiplies it on the way out, and k counted at the case.
"""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

from backward_cases import (ACT_LRELU, ACT_NONE, ACT_SILU, ACT_TANH, DT_NAME, MV_BF16, MV_ERR_ARG, MV_ERR_DTYPE,  # noqa: F401
                            MV_ERR_UNSUPPORTED, MV_F16, MV_F32, TINY, TORCH_DT, U32, U_OUT, Out, Refused, alphas, bounded, cdiv, exact, ints)

SLOPE, MASK_SCALE = 0.25, 2.0
ALL_DT = (MV_BF16, MV_F16, MV_F32)
ACT_FN = {ACT_TANH: "tanh", ACT_SILU: "silu"}
FLT_MIN = 2.0 ** -126
# largest relative error against fp64, measured on an MI355X (tools/measure_device_fn.hip): rsqrtf over [2^-10, 128], expf over [-87, 0],
# tanhf and v / (1 + __expf(-v)) over [-24, 24].  The bounds below use 4 x these; anything above 2^-19 would be a finding.
E_FN = {"rsqrt": 9.212e-8, "exp": 8.272e-8, "tanh": 1.400e-7, "silu": 1.725e-6}
FN_ARG_MAX = 24.0          # tanh / SiLU rows keep their arguments inside the measured range (the host test asserts it)
E_FN_LIMIT = 2.0 ** -19


def stored(out, dt):
    """What a store in type dt leaves of the exact fp64 value: its RNE rounding (the value is an fp32 number, so torch's conversion
    through float rounds once)."""
    return out.ref.to(TORCH_DT[dt]).double()


def proves_exact(out):
    """What makes bit equality a fair demand: all partial sums are multiples of `unit` below 2^24 units."""
    return bool((out.abs_sum / out.unit).max() < 2 ** 24) and bool(((out.ref / out.unit).round() * out.unit == out.ref).all())


def tolerance(out, dt, fn=None, fn_scale=None):
    tol = U_OUT[dt] * out.ref.abs() + out.k * U32 * out.abs_sum + TINY[dt]
    return tol if fn is None else tol + 4 * E_FN[fn] * fn_scale + FLT_MIN      # results below the fp32 normal range may be flushed


def act64(z, act, slope=SLOPE):
    """The four activations in fp64; LeakyReLU as csrc/common.h writes it (v >= 0 ? v : v * slope)."""
    if act == ACT_LRELU:
        return torch.where(z >= 0, z, z * slope)
    if act == ACT_TANH:
        return torch.tanh(z)
    if act == ACT_SILU:
        return z * torch.sigmoid(z)
    return z.clone()


def act_out(pre, pre_abs, unit, act, scale=1.0, add=None):
    """act(pre) * scale + add as an Out (plus the |f| of the bound for tanh / SiLU, else None).  `pre` is exact in fp32 at every row
    (the host test proves it), so only the function's own error, one product and one sum are left: k = 2."""
    f = act64(pre, act) * scale
    ref = f if add is None else f + add
    if act in (ACT_NONE, ACT_LRELU):
        a = pre_abs * abs(scale) + (0 if add is None else add.abs())
        return exact(ref, a, unit * (SLOPE if act == ACT_LRELU else 1.0)), None
    return bounded(ref, f.abs() + (0 if add is None else add.abs()), 2), f.abs()


# =============================================================================================== the generic convolutions
TT, CO_T, CI_T = 128, 32, 8


def conv_lds(xw, ktaps):
    return 4 * (CI_T * xw + CI_T * ktaps * CO_T)


C1 = namedtuple("C1", "name B Cin Cout Tin Tout ks stride pad dil groups K a1 bias act res xs yoff")


def _c1(name, Cin, Cout, Tout, ks, stride=1, pad="same", dil=1, groups=1, K=1, a1=False, bias=True, act=ACT_NONE, res=False, xs=False,
        yoff=0, B=2, extra=0):
    span = (ks - 1) * dil
    pad = {"same": span // 2, "big": span + 2}.get(pad, pad)
    Tin = (Tout - 1) * stride + span + 1 - 2 * pad + extra          # extra < stride: the floor of the output-length rule drops it
    return C1(name, B, Cin, Cout, Tin, Tout, ks, stride, pad, dil, groups, K, a1, bias, act, res, xs, yoff)


CONV1D_CASES = (
    _c1("base-k4-lrelu", 9, 35, 130, 3, K=4, act=ACT_LRELU),                        # cin_g 9 (two staging steps), cout_g 35 (two tiles)
    _c1("t1-ks1", 3, 3, 1, 1, pad=0, bias=False),
    _c1("t127-s2-k7", 8, 32, 127, 7, stride=2, extra=1),
    _c1("t128-d3", 8, 6, 128, 3, dil=3),
    _c1("t129-s4-d3-k7-padbig", 1, 1, 129, 7, stride=4, dil=3, pad="big", extra=3),
    _c1("t130-pad0-k7", 3, 6, 130, 7, pad=0),
    _c1("g2-k8", 6, 12, 129, 3, groups=2, K=8),                                      # cin_g 3, cout_g 6
    _c1("g2-cout35-s2-k4-nobias", 18, 70, 129, 3, stride=2, groups=2, K=4, bias=False),   # cin_g 9, cout_g 35: two tiles a group
    _c1("depthwise", 9, 9, 130, 3, groups=9, act=ACT_LRELU),                         # cin_g 1, cout_g 1
    _c1("depthwise-d3-s2", 8, 8, 127, 7, stride=2, dil=3, groups=8),
    _c1("alpha1-not-one", 3, 6, 129, 3, a1=True),
    _c1("alpha1-not-one-nobias", 3, 6, 33, 3, a1=True, bias=False),
    _c1("k8-nobias", 9, 3, 128, 3, K=8, bias=False),
    _c1("k4-s4", 9, 32, 130, 7, stride=4, K=4),
    _c1("tanh", 3, 6, 129, 3, K=4, act=ACT_TANH),
    _c1("silu", 3, 6, 129, 3, K=4, act=ACT_SILU),
    _c1("res", 9, 35, 130, 3, K=4, act=ACT_LRELU, res=True),
    _c1("res-yslice-xslice", 9, 35, 130, 3, K=4, act=ACT_LRELU, res=True, xs=True, yoff=3),
    _c1("yslice-xslice-d3-s2", 3, 6, 129, 3, stride=2, dil=3, xs=True, yoff=1),
    _c1("res-silu-yslice", 3, 6, 33, 3, act=ACT_SILU, res=True, yoff=2),
    _c1("lds-70592", 3, 5, 20, 63, B=1),                                             # ks 63: above 64 KB of dynamic LDS
)
# (name, (B, Cin, Tin, Cout, Tout, ks, stride, pad, dil, groups, nbanks), alpha given, code)
CONV1D_REFUSED = (
    ("ks160-lds", (1, 3, 200, 5, 41, 160, 1, 0, 1, 1, 1), True, MV_ERR_UNSUPPORTED),
    ("tout+1", (2, 3, 16, 5, 17, 3, 1, 1, 1, 1, 1), True, MV_ERR_ARG), ("tout-1", (2, 3, 16, 5, 15, 3, 1, 1, 1, 1, 1), True, MV_ERR_ARG),
    ("nbanks9", (2, 3, 16, 5, 16, 3, 1, 1, 1, 1, 9), True, MV_ERR_ARG), ("nbanks2-null-alpha", (2, 3, 16, 5, 16, 3, 1, 1, 1, 1, 2), False, MV_ERR_ARG),
    ("cin%groups", (2, 3, 16, 4, 16, 3, 1, 1, 1, 2, 1), True, MV_ERR_ARG), ("B65536", (65536, 3, 16, 5, 16, 3, 1, 1, 1, 1, 1), True, MV_ERR_ARG),
    ("kernel-wider-than-input", (2, 3, 1, 5, 1, 3, 4, 0, 1, 1, 1), True, MV_ERR_ARG),   # numerator -2: C division truncates it to Tout = 1
)


def conv1d_plan(B, Cin, Tin, Cout, Tout, ks, stride, pad, dil, groups, nbanks, alpha=True):
    """mv_conv1d_fwd's host rule restated: (lds bytes, raised limit?, grid) or Refused."""
    if not (B > 0 and Cin > 0 and Cout > 0 and Tin > 0 and ks > 0 and stride > 0 and dil > 0 and pad >= 0):
        raise Refused(MV_ERR_ARG)
    if not (groups > 0 and Cin % groups == 0 and Cout % groups == 0) or not (1 <= nbanks <= 8 and (nbanks == 1 or alpha)):
        raise Refused(MV_ERR_ARG)
    num = Tin + 2 * pad - dil * (ks - 1) - 1
    if num < 0 or Tout != num // stride + 1 or B > 65535 or groups * cdiv(Cout // groups, CO_T) > 65535:
        raise Refused(MV_ERR_ARG)
    lds = conv_lds((TT - 1) * stride + (ks - 1) * dil + 1, ks)
    if lds > 160 * 1024:
        raise Refused(MV_ERR_UNSUPPORTED)
    return lds, lds > 64 * 1024, (cdiv(Tout, TT), groups * cdiv(Cout // groups, CO_T), B)


def _xr(act):
    """(density, lo, hi) of a conv row's x: [-4, 4], or [-1, 1] under tanh / SiLU (arguments inside the measured range)."""
    return (1.0, -1, 1) if act in ACT_FN else (1.0, -4, 4)


def _banks(B, K, a1, seed):
    """alpha [B][K] as the call passes it (None: NULL) and as the reference multiplies."""
    if K > 1:
        a = alphas(B, K, seed)
        return a, a
    if a1:
        a = torch.tensor([[0.5], [1.5], [0.25], [2.0]], dtype=torch.float64)[:B]
        return a, a
    return None, torch.ones(B, 1, dtype=torch.float64)


def conv1d_f64(x, w, bias, am, stride=1, pad=0, dil=1, groups=1):
    """sum_k am[b,k] (conv1d(x[b]; w[k]) + bias[k]) as F.conv1d with the per-sample kernel sum_k am[b,k] w[k] (samples as groups):
    x [B][Cin][Tin], w [K][Cout][Cin / groups][ks], bias [K][Cout] or None, am [B][K]."""
    (B, Cin, Tin), (K, Cout, cin_g, ks) = x.shape, w.shape
    wb = torch.einsum("bk,kocj->bocj", am, w).reshape(B * Cout, cin_g, ks)
    y = F.conv1d(x.reshape(1, B * Cin, Tin), wb, None, stride, pad, dil, B * groups).view(B, Cout, -1)
    return y if bias is None else y + (am @ bias)[:, :, None]


def convT_f64(x, w, bias, am, stride=1, pad=0, opad=0, dil=1):
    """The same for F.conv_transpose1d: w [K][Cin][Cout][ks]."""
    (B, Cin, Tin), (K, _, Cout, ks) = x.shape, w.shape
    wb = torch.einsum("bk,kcoj->bcoj", am, w).reshape(B * Cin, Cout, ks)
    y = F.conv_transpose1d(x.reshape(1, B * Cin, Tin), wb, None, stride, pad, opad, B, dil).view(B, Cout, -1)
    return y if bias is None else y + (am @ bias)[:, :, None]


def conv2d_f64(x, w, bias, ph, pw):
    y = F.conv2d(x, w, None, 1, (ph, pw))
    return y if bias is None else y + bias.view(1, -1, 1, 1)


@functools.lru_cache(maxsize=None)
def conv1d_reference(c):
    """F.conv1d in fp64 with the per-sample kernel sum_k alpha[b,k] W[k] (samples as groups)."""
    x, w = ints((c.B, c.Cin, c.Tin), 201, *_xr(c.act)), ints((c.K, c.Cout, c.Cin // c.groups, c.ks), 202)
    bias = ints((c.K, c.Cout), 203) if c.bias else None
    alpha, am = _banks(c.B, c.K, c.a1, 204)
    res = ints((c.B, c.Cout, c.Tout), 205, lo=-4, hi=4) if c.res else None
    y = conv1d_f64(x, w, bias, am, c.stride, c.pad, c.dil, c.groups)
    ya = conv1d_f64(x.abs(), w.abs(), None if bias is None else bias.abs(), am, c.stride, c.pad, c.dil, c.groups)
    assert y.shape[2] == c.Tout, (c, y.shape)
    out, fs = act_out(y, ya, 1.0 / 8, c.act, add=res)
    return dict(x=x, w=w, bias=bias, alpha=alpha, res=res, y=out, fn_scale=fs, pre=exact(y, ya, 1.0 / 8))


CT = namedtuple("CT", "name B Cin Cout Tin Tout ks stride pad dil opad K a1 bias act")


def _ct(name, Cin, Cout, Tin, stride, ks, pad=0, dil=1, opad=0, K=1, a1=False, bias=True, act=ACT_NONE, B=2):
    pad = (ks - stride) // 2 if pad == "half" else pad
    return CT(name, B, Cin, Cout, Tin, (Tin - 1) * stride - 2 * pad + dil * (ks - 1) + 1 + opad, ks, stride, pad, dil, opad, K, a1, bias, act)


CONVT_CASES = (
    _ct("s1k3", 3, 5, 257, 1, 3), _ct("s1k3-half", 9, 33, 130, 1, 3, pad="half", K=4), _ct("s2k4", 3, 5, 129, 2, 4, K=4, bias=False),
    _ct("s2k4-half-op1", 9, 33, 64, 2, 4, pad="half", opad=1, K=8), _ct("s2k7", 9, 5, 130, 2, 7, opad=1), _ct("s2k7-half-d2", 3, 33, 66, 2, 7, pad="half", dil=2),
    _ct("s3k6", 3, 5, 87, 3, 6, K=4), _ct("s3k6-half-op2", 9, 5, 43, 3, 6, pad="half", opad=2, act=ACT_LRELU), _ct("s3k6-d2", 3, 5, 43, 3, 6, dil=2, opad=2),
    _ct("s4k8", 9, 33, 33, 4, 8, K=4, act=ACT_LRELU), _ct("s4k8-half-op3", 3, 5, 65, 4, 8, pad="half", opad=3, a1=True), _ct("s4k8-d2", 3, 5, 32, 4, 8, dil=2),
    _ct("s8k16", 9, 33, 17, 8, 16, K=4), _ct("s8k16-half-op7", 3, 5, 33, 8, 16, pad="half", opad=7, K=8, bias=False), _ct("s8k16-half-d2", 3, 5, 16, 8, 16, pad="half", dil=2),
    _ct("tin1", 3, 5, 1, 8, 16, pad="half"), _ct("tanh", 3, 5, 33, 2, 4, pad="half", K=4, act=ACT_TANH), _ct("silu", 3, 5, 33, 2, 4, pad="half", K=4, act=ACT_SILU),
)
# (name, (B, Cin, Tin, Cout, Tout, ks, stride, pad, dil, nbanks), alpha given, code): full length 32 at Tin 16, ks 4, stride 2, pad 1
CONVT_REFUSED = (("tout-short", (2, 3, 16, 5, 31, 4, 2, 1, 1, 1), True, MV_ERR_ARG), ("tout-long", (2, 3, 16, 5, 34, 4, 2, 1, 1, 1), True, MV_ERR_ARG),
                 ("nbanks9", (2, 3, 16, 5, 32, 4, 2, 1, 1, 9), True, MV_ERR_ARG), ("nbanks2-null-alpha", (2, 3, 16, 5, 32, 4, 2, 1, 1, 2), False, MV_ERR_ARG),
                 ("B65536", (65536, 3, 16, 5, 32, 4, 2, 1, 1, 1), True, MV_ERR_ARG), ("ks200-lds", (1, 3, 16, 5, 215, 200, 1, 0, 1, 1), True, MV_ERR_UNSUPPORTED))


def convT_plan(B, Cin, Tin, Cout, Tout, ks, stride, pad, dil, nbanks, alpha=True):
    if not (B > 0 and Cin > 0 and Cout > 0 and Tin > 0 and ks > 0 and stride > 0 and dil > 0 and pad >= 0):
        raise Refused(MV_ERR_ARG)
    if not (1 <= nbanks <= 8 and (nbanks == 1 or alpha)):
        raise Refused(MV_ERR_ARG)
    full = (Tin - 1) * stride - 2 * pad + dil * (ks - 1) + 1
    if not (full <= Tout < full + stride and Tout > 0) or B > 65535:
        raise Refused(MV_ERR_ARG)
    xw = (TT - 1 + (ks - 1) * dil) // stride + 2
    lds = conv_lds(xw, ks)
    if lds > 160 * 1024:
        raise Refused(MV_ERR_UNSUPPORTED)
    return lds, xw, (cdiv(Tout, TT), cdiv(Cout, CO_T), B)


def convT_window_is_wide_enough(Tout, ks, stride, pad, dil, xw):
    """conv_transpose1d_fwd_kernel skips a term when xi >= xw: no term of any tile may land there."""
    for u0 in range(0, Tout, TT):
        tlo = (u0 + pad - (ks - 1) * dil) // stride                      # floor division, as the kernel's two branches compute it
        if (u0 + TT - 1 + pad) // stride - tlo >= xw:
            return False
    return True


@functools.lru_cache(maxsize=None)
def convT_reference(c):
    x, w = ints((c.B, c.Cin, c.Tin), 211, *_xr(c.act)), ints((c.K, c.Cin, c.Cout, c.ks), 212)
    bias = ints((c.K, c.Cout), 213) if c.bias else None
    alpha, am = _banks(c.B, c.K, c.a1, 214)
    y = convT_f64(x, w, bias, am, c.stride, c.pad, c.opad, c.dil)
    ya = convT_f64(x.abs(), w.abs(), None if bias is None else bias.abs(), am, c.stride, c.pad, c.opad, c.dil)
    assert y.shape[2] == c.Tout, (c, y.shape)
    out, fs = act_out(y, ya, 1.0 / 8, c.act)
    return dict(x=x, w=w, bias=bias, alpha=alpha, y=out, fn_scale=fs, pre=exact(y, ya, 1.0 / 8))


C2 = namedtuple("C2", "name B Cin Cout H W kh kw ph pw bias act")
CONV2D_CASES = (
    C2("k51-w2", 2, 9, 33, 9, 2, 5, 1, 2, 0, True, ACT_LRELU), C2("k51-w3-pad0", 2, 1, 32, 9, 3, 5, 1, 0, 0, True, ACT_NONE),
    C2("k31-w11", 2, 9, 1, 7, 11, 3, 1, 1, 0, False, ACT_LRELU), C2("k31-w3-pad0", 1, 9, 33, 7, 3, 3, 1, 0, 0, True, ACT_NONE),
    C2("k33-w3", 2, 9, 32, 5, 3, 3, 3, 1, 1, True, ACT_LRELU), C2("k33-w11-pad0", 2, 1, 33, 5, 11, 3, 3, 0, 0, True, ACT_NONE),
    C2("k33-wo130", 1, 9, 33, 3, 130, 3, 3, 1, 1, True, ACT_LRELU), C2("k11-w2", 2, 9, 33, 4, 2, 1, 1, 0, 0, True, ACT_NONE),
    C2("k11-w11-padded", 1, 1, 1, 3, 11, 1, 1, 1, 1, True, ACT_NONE), C2("k33-tanh", 1, 1, 3, 4, 11, 3, 3, 1, 1, True, ACT_TANH),
    C2("k33-silu", 1, 1, 3, 4, 11, 3, 3, 1, 1, True, ACT_SILU),
    C2("rows-65535", 1, 1, 1, 65535, 2, 1, 1, 0, 0, True, ACT_LRELU),                  # B * Ho = 65535: the largest grid.z
)
CONV2D_REFUSED = (("rows-65536", (1, 1, 65536, 2, 1, 1, 1, 0, 0), MV_ERR_ARG), ("ho0", (1, 1, 2, 2, 1, 3, 1, 0, 0), MV_ERR_ARG))   # B Cin H W Cout kh kw ph pw


def conv2d_plan(B, Cin, H, W, Cout, kh, kw, ph, pw):
    Ho, Wo = H + 2 * ph - kh + 1, W + 2 * pw - kw + 1
    if not (B > 0 and Cin > 0 and Cout > 0 and H > 0 and W > 0 and kh > 0 and kw > 0 and ph >= 0 and pw >= 0 and Ho > 0 and Wo > 0 and B * Ho <= 65535):
        raise Refused(MV_ERR_ARG)
    lds = 4 * (CI_T * kh * (TT + kw - 1) + CI_T * kh * kw * CO_T)
    if lds > 160 * 1024:
        raise Refused(MV_ERR_UNSUPPORTED)
    return lds, (cdiv(Wo, TT), cdiv(Cout, CO_T), B * Ho)


@functools.lru_cache(maxsize=None)
def conv2d_reference(c):
    x, w = ints((c.B, c.Cin, c.H, c.W), 221, *_xr(c.act)), ints((c.Cout, c.Cin, c.kh, c.kw), 222)
    bias = ints((1, c.Cout), 223) if c.bias else None
    out, fs = act_out(conv2d_f64(x, w, bias, c.ph, c.pw), conv2d_f64(x.abs(), w.abs(), None if bias is None else bias.abs(), c.ph, c.pw), 1.0, c.act)
    return dict(x=x, w=w, bias=bias, y=out, fn_scale=fs, pre=exact(conv2d_f64(x, w, bias, c.ph, c.pw), conv2d_f64(x.abs(), w.abs(), None if bias is None else bias.abs(), c.ph, c.pw)))


# =============================================================================================== GroupNorm
# A tensor's place in memory: (element offset of the base from a 16-byte boundary, extra elements a channel row, extra elements a sample)
Lay = namedtuple("Lay", "off cs bs")
DENSE = Lay(0, 0, 0)


def strides(lay, C, T):
    cs = T + lay.cs
    return C * cs + lay.bs, cs


def gn_vec(dt, T, lays, C, mask_off=None):
    """The 16-byte predicate of gn_stats_kernel (one tensor) and of gn_apply_kernel and its host copy (x, res, y and the mask)."""
    if dt == MV_F32:
        return False
    for lay in lays:
        if lay is None:
            continue
        bs, cs = strides(lay, C, T)
        if bs % 8 or cs % 8 or (lay.off * 2) % 16:
            return False
    return T % 8 == 0 and (mask_off is None or mask_off % 8 == 0)


def gn_apply_grid(dt, T, lays, C, B, mask_off=None):
    n = cdiv(T, 8) if gn_vec(dt, T, lays, C, mask_off) else T
    return max(1, min(64, cdiv(n, 256))), B * C


GS = namedtuple("GS", "name B C G T lay heavy")
GN_STATS_CASES = (
    GS("vec-t8", 2, 8, 2, 8, DENSE, False), GS("vec-t16-cg1", 2, 4, 4, 16, DENSE, False), GS("vec-t2056-two-passes", 1, 8, 1, 2056, DENSE, False),
    GS("vec-slice-of-8s", 2, 8, 8, 16, Lay(8, 8, 16), False),
    GS("scalar-t7", 2, 8, 1, 7, DENSE, False), GS("scalar-t9", 2, 8, 8, 9, DENSE, False), GS("scalar-base+8B", 2, 8, 2, 16, Lay(4, 0, 0), False),
    GS("scalar-x_cs", 2, 8, 2, 16, Lay(0, 4, 0), False), GS("scalar-x_bs", 2, 8, 2, 16, Lay(0, 0, 4), False),
    GS("offset-heavy", 2, 4, 2, 64, DENSE, True), GS("offset-heavy-scalar", 2, 4, 4, 63, DENSE, True),
)
GN_EPS = 2.0 ** -16


@functools.lru_cache(maxsize=None)
def gn_stats_reference(c, dt):
    """Each group's values are an integer mean m plus deviations that cancel in pairs: the sum is m n exactly, so mean = m whatever n
    is; the centred squares are integers.  var = q / n is one rounding unless n is a power of two, var + eps another, then rsqrtf:
    rstd carries k = 2 and the measured rsqrtf error.  The offset-heavy rows put the values around 1000 (fp32, fp16: step 1) or 1024
    (bf16: step 8, what the type can hold there): sum x^2 in fp32 loses the variance, the kernel's centred second pass does not."""
    cg, n = c.C // c.G, c.C // c.G * c.T
    step, base = ((8.0, 1024.0) if dt == MV_BF16 else (1.0, 1000.0)) if c.heavy else (1.0, 0.0)
    d = torch.zeros(c.B, c.G, n, dtype=torch.float64)
    h = n // 2
    d[:, :, :h] = ints((c.B, c.G, h), 231, lo=(-1 if c.heavy else -3), hi=(1 if c.heavy else 3)) * step
    d[:, :, h:2 * h] = -d[:, :, :h]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(232))
    d = d[:, :, perm]
    m = base + ints((c.B, c.G, 1), 233, lo=-1, hi=1) * step
    x = (d + m).view(c.B, c.C, c.T)
    var = (d * d).sum(2) / n
    rstd = (var + GN_EPS) ** -0.5
    return dict(x=x, mean=exact(m[:, :, 0].clone(), (d + m).abs().sum(2)), sumsq=exact((d * d).sum(2)), var=var, rstd=bounded(rstd, rstd, 2))


GA = namedtuple("GA", "name B C G T act gw gb res mask x y r moff")


def _ga(name, T, act=ACT_LRELU, gw=True, gb=True, res=False, mask=False, x=DENSE, y=DENSE, r=DENSE, moff=0, B=2, C=8, G=2):
    return GA(name, B, C, G, T, act, gw, gb, res, mask, x, y, r if res else None, moff if mask else None)


GN_APPLY_CASES = (
    _ga("vec-t8", 8), _ga("vec-t16-res-mask", 16, res=True, mask=True), _ga("vec-t2056-none", 2056, act=ACT_NONE, mask=True, B=1, C=2, G=1),
    _ga("vec-all-slices-of-8s", 16, res=True, mask=True, x=Lay(8, 8, 16), y=Lay(16, 16, 8), r=Lay(8, 24, 8)),
    _ga("scalar-t7", 7, res=True, mask=True), _ga("scalar-t9", 9, act=ACT_NONE, res=True, mask=True),
    _ga("scalar-x-base", 16, res=True, mask=True, x=Lay(4, 0, 0)), _ga("scalar-y-base", 16, res=True, mask=True, y=Lay(4, 0, 0)),
    _ga("scalar-res-base", 16, res=True, mask=True, r=Lay(4, 0, 0)), _ga("scalar-x_cs", 16, mask=True, x=Lay(0, 4, 0)),
    _ga("scalar-x_bs", 16, mask=True, x=Lay(0, 0, 4)), _ga("scalar-y_cs", 16, res=True, y=Lay(0, 4, 0)), _ga("scalar-y_bs", 16, y=Lay(0, 0, 4)),
    _ga("scalar-r_cs", 16, res=True, r=Lay(0, 4, 0)), _ga("scalar-r_bs", 16, res=True, r=Lay(0, 0, 4)),
    _ga("scalar-res-strided-misaligned", 24, res=True, mask=True, r=Lay(1, 3, 5)),
    _ga("scalar-mask+4B", 16, res=True, mask=True, moff=4), _ga("scalar-mask+1B", 16, mask=True, moff=1), _ga("vec-mask+8B", 16, mask=True, moff=8),
    _ga("no-gw", 16, gw=False, mask=True), _ga("no-gb", 16, gb=False, res=True), _ga("no-gw-gb-scalar", 9, gw=False, gb=False),
    _ga("cg1", 16, mask=True, G=8), _ga("g1", 16, res=True, G=1),
    _ga("scalar-t16400-grid-stride", 16400, mask=True, res=True, x=Lay(4, 0, 0), B=1, C=2, G=1), _ga("vec-t131080-grid-stride", 131080, mask=True, B=1, C=2, G=2),
    _ga("tanh-vec", 16, act=ACT_TANH, res=True, mask=True), _ga("tanh-scalar", 9, act=ACT_TANH, mask=True),
    _ga("silu-vec", 16, act=ACT_SILU, res=True, mask=True), _ga("silu-scalar", 9, act=ACT_SILU, res=True),
)


@functools.lru_cache(maxsize=None)
def gn_apply_reference(c):
    """y = act((x - mean) rstd gw + gb), kept elements times mask_scale and dropped ones zero, plus res.  mean an integer, rstd a
    power of two (1/2 .. 2; 1/8 .. 1/2 under tanh / SiLU so that the arguments stay inside [-6, 6]), gw in {+-1, +-2}: the kernel's
    a = rstd gw, sh = gb - mean a and x a + sh are exact however they are contracted."""
    x = ints((c.B, c.C, c.T), 241, lo=-4, hi=4)
    g = torch.Generator().manual_seed(242)
    mean = torch.randint(-1, 2, (c.B, c.G), generator=g).double()
    rstd = 2.0 ** (torch.randint(-1, 2, (c.B, c.G), generator=g).double() - (2 if c.act in ACT_FN else 0))
    gw, gb = ints((c.C,), 243, lo=-2, hi=2), ints((c.C,), 244, lo=-2, hi=2)
    gw[gw == 0] = 1.0
    res = ints((c.B, c.C, c.T), 245, lo=-4, hi=4) if c.res else None
    mask = None
    if c.mask:                                                    # any non-zero byte keeps: 1, 2, 128, 255 in turn; zeros in every byte lane
        keep = torch.rand((c.B, c.C, c.T), generator=g) < 0.6
        vals = torch.tensor([1, 2, 128, 255], dtype=torch.uint8)[torch.arange(c.B * c.C * c.T) % 4].view(c.B, c.C, c.T)
        mask = torch.where(keep, vals, torch.zeros_like(vals))
    cg = c.C // c.G
    mu, rs = mean.repeat_interleave(cg, 1)[:, :, None], rstd.repeat_interleave(cg, 1)[:, :, None]
    a = rs * (gw[None, :, None] if c.gw else 1.0)
    sh = (gb[None, :, None] if c.gb else 0.0) - mu * a
    pre, pre_abs = x * a + sh, x.abs() * a.abs() + (gb.abs()[None, :, None] if c.gb else 0.0) + (mu * a).abs()
    keepf = (mask != 0).double() * MASK_SCALE if c.mask else None
    f = act64(pre, c.act)
    if keepf is not None:
        f, pre_abs = f * keepf, pre_abs * MASK_SCALE
    ref = f if res is None else f + res
    if c.act in ACT_FN:
        y, fs = bounded(ref, f.abs() + (0 if res is None else res.abs()), 2), f.abs()      # k = 2: the mask_scale product is exact; the sum, one spare
    else:
        y, fs = exact(ref, pre_abs + (0 if res is None else res.abs()), 1.0 / 32), None    # 1/8 (rstd gw) x 1/4 (slope)
    return dict(x=x, mean=mean, rstd=rstd, gw=gw, gb=gb, res=res, mask=mask, y=y, fn_scale=fs, pre=exact(pre, pre_abs, 1.0 / 8))


# =============================================================================================== FiLM, scale-shift, act, avgpool, fold
CAP_N = 2048 * 256 + 3                                            # three elements past the capped grid of 2048 workgroups
FILM_CASES = ((2, 5, 3, 257), (2, 4, 4, 16385), (2, 3, 5, 1), (1, 6, 2, 256))          # (B, C, F, T); 16385 = 64 * 256 + 1: the capped grid
SCALE_SHIFT_CASES = ((2, 5, 257), (1, 3, 16385), (3, 1, 1))
ACT_CASES = tuple((n, act, res) for n, act, res in ((1, ACT_LRELU, False), (CAP_N, ACT_LRELU, True), (CAP_N, ACT_NONE, False), (4099, ACT_NONE, True),
                                                    (4099, ACT_TANH, True), (4099, ACT_SILU, False), (4099, ACT_SILU, True), (4099, ACT_TANH, False)))
AVGPOOL_CASES = ((3, 10, 4), (3, 8, 1), (3, 9, 2), (3, 16387, 1), (2, 65537, 4), (65535, 3, 2), (3, 7, 4), (3, 4, 4))     # (rows, T, s)
MPD_CASES = tuple((rows, P, T) for rows, P, T in ((3, 2, 16), (3, 2, 17), (3, 3, 300), (3, 3, 301), (3, 3, 302), (2, 5, 1000), (2, 5, 1001), (2, 5, 1004),
                                                  (3, 7, 700), (3, 7, 701), (3, 7, 706), (2, 11, 16500), (2, 11, 16501), (2, 11, 16510), (65535, 2, 3), (1, 11, 1)))


@functools.lru_cache(maxsize=None)
def film_reference(B, C, Fd, T):
    """y = gamma x + beta on the first min(C, F) channels (proj = [gamma | beta], F each); the other channels pass through."""
    x, proj = ints((B, C, T), 251, lo=-4, hi=4), ints((B, 2 * Fd), 252)
    gam, bet = torch.ones(B, C, dtype=torch.float64), torch.zeros(B, C, dtype=torch.float64)
    m = min(C, Fd)
    gam[:, :m], bet[:, :m] = proj[:, :m], proj[:, Fd:Fd + m]
    return dict(x=x, proj=proj, y=exact(x * gam[:, :, None] + bet[:, :, None], (x * gam[:, :, None]).abs() + bet.abs()[:, :, None]))


@functools.lru_cache(maxsize=None)
def scale_shift_reference(B, C, T):
    x, s, h = ints((B, C, T), 253, lo=-4, hi=4), ints((B, C), 254), ints((B, C), 255)
    return dict(x=x, scale=s, shift=h, y=exact(x * s[:, :, None] + h[:, :, None], (x * s[:, :, None]).abs() + h.abs()[:, :, None]))


@functools.lru_cache(maxsize=None)
def act_reference(n, act, res):
    """Arguments are multiples of 1/8 in [-6, 6] with both zeros among them."""
    x = ints((n,), 256, lo=-48, hi=48) / 8
    x[:2] = torch.tensor([0.0, -0.0], dtype=torch.float64)[:min(2, n)]
    r = ints((n,), 257, lo=-4, hi=4) if res else None
    y, fs = act_out(x, x.abs(), 1.0 / 8, act, add=r)
    return dict(x=x, res=r, y=y, fn_scale=fs, pre=exact(x, unit=1.0 / 8))


def avgpool_f64(x, s):
    """[..., T] -> [..., T // s]: the mean of each whole window of s; the tail T % s is dropped."""
    To = x.shape[-1] // s
    return x[..., :To * s].reshape(*x.shape[:-1], To, s).sum(-1) / s


def mpd_f64(x, P):
    """[..., T] -> [..., Tp], Tp the next multiple of P, zero-padded on the right (the caller views it as [P][Tp / P])."""
    T = x.shape[-1]
    y = torch.zeros(*x.shape[:-1], T if T % P == 0 else T + (P - T % P), dtype=x.dtype)
    y[..., :T] = x
    return y


@functools.lru_cache(maxsize=None)
def avgpool_reference(rows, T, s):
    x = ints((rows, T), 258, lo=-4, hi=4)
    return dict(x=x, y=exact(avgpool_f64(x, s), avgpool_f64(x.abs(), s), 1.0 / s))


def mpd_reference(rows, P, T):
    """x [rows][T] -> [rows][Tp], Tp the next multiple of P, zero-padded; index[t] = t, or -1 in the padding."""
    Tp = T if T % P == 0 else T + (P - T % P)
    x = ints((rows, T), 259, lo=-4, hi=4)
    x[:, -1] = 3.0                                               # the last real element is never mistaken for padding
    y = mpd_f64(x, P)
    idx = torch.arange(Tp, dtype=torch.int64)
    idx[T:] = -1
    return dict(x=x, y=exact(y), index=idx, Tp=Tp)


# =============================================================================================== mv_cast
def cast_specials():
    """fp32 values whose 16-bit rounding is decided by the rule: ties to even both ways, the two zeros, subnormals, the largest finite
    values, the first values that overflow, infinities and NaN."""
    import struct
    bits = lambda b: struct.unpack("<f", struct.pack("<I", b))[0]
    v = [0.0, -0.0, 1.0, -1.0,
         bits(0x3F808000), bits(0x3F818000), bits(0x3F808001), bits(0x3F807FFF), bits(0xBF808000), bits(0xBF818000),   # bf16 ties: down to even, up to even, just above, just below
         1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -23, -(1.0 + 2.0 ** -11), -(1.0 + 3 * 2.0 ** -11),   # f16 ties
         2.0 ** -24, 2.0 ** -25, 2.0 ** -25 + 2.0 ** -40, 3 * 2.0 ** -25, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -133, 2.0 ** -149, bits(0x00000001),   # f16 / bf16 / fp32 subnormals
         65504.0, 65519.9, 65520.0, -65520.0, 1e5,                 # f16: largest finite, the last value below the tie, the tie (to inf)
         bits(0x7F7F0000), bits(0x7F7F7FFF), bits(0x7F7F8000), bits(0x7F7FFFFF), -bits(0x7F7FFFFF),   # bf16: largest finite, below the tie, the tie and FLT_MAX (to inf)
         float("inf"), float("-inf"), float("nan")]
    return torch.tensor(v, dtype=torch.float32)


# =============================================================================================== layout transposes
def transpose_geometry(entry, B, C, T, Cpad):
    """(R, Cn, ldx, ldy, x_bs, y_bs) transpose_launch gets from each entry: x [batch][R][ldx] -> y [batch][Cn][ldy]."""
    if entry == "nct_to_ntc":
        return C, T, T, C, C * T, T * C
    if entry == "ntc_to_nct":
        return T, C, C, T, T * C, C * T
    if entry == "nct_to_ntc_pad":
        return C, T, T, Cpad, C * T, T * Cpad
    assert entry == "ntc_to_nct_crop"
    return T, C, Cpad, T, T * Cpad, C * T


def transpose_plan(entry, B, C, T, Cpad, dt, xoff=0, yoff=0):
    """Which kernel and grid: the 64 x 64 16-byte kernel needs 16-bit data, five multiples of 8 and two aligned bases."""
    R, Cn, ldx, ldy, x_bs, y_bs = transpose_geometry(entry, B, C, T, Cpad)
    if not (B > 0 and B <= 65535 and R > 0 and Cn > 0 and ldx >= Cn and ldy >= R and cdiv(ldy, 32) <= 65535):
        raise Refused(MV_ERR_ARG)
    if dt != MV_F32 and all(v % 8 == 0 for v in (Cn, ldx, ldy, x_bs, y_bs)) and (xoff * 2) % 16 == 0 and (yoff * 2) % 16 == 0:
        return "16", (cdiv(Cn, 64), cdiv(ldy, 64), B)
    return "32", (cdiv(Cn, 32), cdiv(ldy, 32), B)


# (C, T): every R and Cn of {1, 31, 32, 33, 63, 64, 65, 72} on each side, then shapes the 16-byte kernel takes (both multiples of 8)
TR_SHAPES = ((1, 72), (31, 64), (32, 33), (33, 32), (63, 8), (64, 65), (65, 1), (72, 31), (64, 64), (72, 72), (8, 136), (136, 8), (64, 72), (32, 63), (63, 63))
# (entry, C, T, Cpad, x offset, y offset, what the row breaks): the fast path and each of its terms broken on its own, as far as the
# entry's own arguments allow (Cn = ldx in the forward entries; x_bs and y_bs are products of the other three)
TR_FAST = (("nct_to_ntc_pad", 64, 72, 80, 0, 0, None), ("nct_to_ntc_pad", 60, 72, 64, 0, 0, None), ("nct_to_ntc_pad", 64, 72, 81, 0, 0, "ldy"),
           ("nct_to_ntc_pad", 64, 72, 80, 4, 0, "x base"), ("nct_to_ntc_pad", 64, 72, 80, 0, 4, "y base"), ("nct_to_ntc_pad", 64, 71, 80, 0, 0, "Cn"),
           ("nct_to_ntc_pad", 1, 8, 8, 0, 0, None), ("nct_to_ntc_pad", 8, 136, 72, 0, 0, None), ("nct_to_ntc_pad", 72, 8, 136, 0, 0, None), ("nct_to_ntc_pad", 65, 136, 72, 0, 0, None), ("nct_to_ntc_pad", 31, 33, 33, 0, 0, "Cn"),
           ("ntc_to_nct_crop", 64, 72, 80, 0, 0, None), ("ntc_to_nct_crop", 64, 72, 81, 0, 0, "ldx"), ("ntc_to_nct_crop", 60, 72, 64, 0, 0, "Cn"),
           ("ntc_to_nct_crop", 64, 71, 80, 0, 0, "ldy"), ("ntc_to_nct_crop", 64, 72, 80, 4, 0, "x base"), ("ntc_to_nct_crop", 64, 72, 80, 0, 4, "y base"),
           ("ntc_to_nct_crop", 8, 136, 16, 0, 0, None), ("ntc_to_nct_crop", 31, 33, 40, 0, 0, "Cn"), ("ntc_to_nct_crop", 72, 65, 72, 0, 0, "ldy"),
           ("nct_to_ntc", 64, 72, 0, 4, 0, "x base"), ("ntc_to_nct", 64, 72, 0, 0, 4, "y base"))


def distinct_bits(shape, dt):
    """A tensor whose elements are pairwise distinct, finite and normal in type dt: consecutive bit patterns from 0x0400 up (16-bit
    types hold fewer distinct integers than a tile has elements)."""
    n = 1
    for s in shape:
        n *= s
    if dt == MV_F32:
        return (torch.arange(n, dtype=torch.float32) + 1.0).view(shape)
    assert 0x0400 + n < 0x7800
    return (torch.arange(n, dtype=torch.int32) + 0x0400).to(torch.int16).view(TORCH_DT[dt]).view(shape)


def transpose_reference(entry, x, B, C, T, Cpad):
    """By index: y[b][c][r] = x[b][r][c] for r < R, c < Cn; zero for R <= r < ldy (the padded channels)."""
    R, Cn, ldx, ldy, _, _ = transpose_geometry(entry, B, C, T, Cpad)
    y = torch.zeros(B, Cn, ldy, dtype=x.dtype)
    y[:, :, :R] = x.view(B, R, ldx)[:, :, :Cn].transpose(1, 2)
    return y


# =============================================================================================== mv_linear_fwd
LINEAR_CASES = ((1, 1, 1), (1, 5, 63), (5, 1, 64), (2, 4, 65), (1, 8, 130), (4, 2, 1), (1, 5, 130))       # (M, N, Kd)


@functools.lru_cache(maxsize=None)
def linear_reference(M, N, Kd):
    x, w, b = ints((M, Kd), 261, lo=-4, hi=4), ints((N, Kd), 262), ints((N,), 263)
    return dict(x=x, w=w, b=b, y=exact(F.linear(x, w, b), F.linear(x.abs(), w.abs(), b.abs())), y_nobias=exact(F.linear(x, w), F.linear(x.abs(), w.abs())))


# =============================================================================================== mv_odconv_attn_fwd
AT = namedtuple("AT", "name B C T K pooled bias xoff rail")
ATTN_CASES = (
    AT("one-below-threshold", 3, 63, 256, 4, True, True, 0, False), AT("two-at-threshold", 3, 64, 256, 4, True, True, 0, False),
    AT("one-c64-t255", 3, 64, 255, 4, True, True, 0, False), AT("one-null-pooled-above", 3, 64, 256, 4, False, True, 0, False),
    AT("two-scalar-t253", 3, 65, 253, 4, True, True, 0, False), AT("two-scalar-misaligned", 3, 65, 256, 4, True, True, 1, False),
    AT("two-k1", 2, 64, 256, 1, True, False, 0, False), AT("two-k64", 2, 64, 256, 64, True, True, 0, False), AT("one-k64", 2, 5, 8, 64, True, True, 0, False),
    AT("one-k1-nobias", 3, 5, 8, 1, False, False, 0, False), AT("one-rail", 3, 5, 8, 4, True, True, 0, True), AT("two-rail", 3, 64, 256, 4, True, True, 0, True),
    AT("one-c1-t1", 2, 1, 1, 4, True, True, 0, False), AT("one-c300", 2, 300, 4, 4, True, False, 0, False),
)


def attn_plan(B, C, T, K, pooled, dt, xoff=0):
    """('one',) or ('two', rowmean takes its vector arm, rowmean grid); Refused for K > 64 or more than 64 KB of LDS."""
    if not (B > 0 and C > 0 and T > 0 and 0 < K <= 64) or 4 * (C + K) > 64 * 1024:
        raise Refused(MV_ERR_ARG)
    if pooled and C * T >= 16384:
        esz = 4 if dt == MV_F32 else 2
        return "two", T % (16 // esz) == 0 and (xoff * esz) % 16 == 0, cdiv(B * C, 4)
    return ("one",)


def softmax_out(logit, delta, K):
    """softmax in fp64 with its bound: an argument error delta moves a softmax output by at most a factor e^(2 delta); expf on top
    and bottom (2 x 4 E_FN), K additions, one division and the subtraction of the maximum (k = K + 3, relative to the output itself);
    outputs below the fp32 normal range are flushed or denormal: FLT_MIN on top."""
    a = F.softmax(logit, dim=1)
    return a, a * (2 * delta + 8 * E_FN["exp"] + (K + 3) * U32) + FLT_MIN


@functools.lru_cache(maxsize=None)
def attn_reference(c):
    """pooled = mean_t x: the sum is exact; times 1 / T (one launch) or divided by T (rowmean): exact for a power of two, k = 2 otherwise.
    logits = W pooled + b: exact for exact means, else every term carries the mean's error and C / 64 + 8 roundings of the lane chains
    and the wave tree.  The rail rows put +-80 on the logits through the bias."""
    x, w = ints((c.B, c.C, c.T), 271, lo=-4, hi=4), ints((c.K, c.C), 272)
    b = ints((c.K,), 273) if c.bias else None
    if c.rail:
        b = torch.tensor([80.0, -80.0, 79.0, 0.0], dtype=torch.float64)[:c.K]
    m, ma = x.mean(2), x.abs().mean(2)
    pow2 = c.T & (c.T - 1) == 0
    pooled = exact(m, ma, 1.0 / c.T) if pow2 else bounded(m, ma, 2)
    logit = F.linear(m, w, b)
    la = F.linear(ma, w.abs(), None if b is None else b.abs())
    delta = 0.0 if pow2 else ((2 + c.C // 64 + 8) * U32 * la).max().item()
    alpha, tol = softmax_out(logit, delta, c.K)
    return dict(x=x, w=w, b=b, pooled=pooled, logit=exact(logit, la, 1.0 / c.T) if pow2 else None, alpha=alpha, alpha_tol=tol)


# =============================================================================================== mv_gen_prologue(_in)
PR = namedtuple("PR", "name B C T K ds de cond F2 zero_n film in32 bias")
PRO_NT, PRO_SG = 1024, 8


def _pr(name, B=3, C=20, T=16, K=4, ds=5, de=6, cond=11, F2=24, zero_n=None, film=True, in32=False, bias=True):
    return PR(name, B, C, T, K, ds, de, cond, F2, 5 * B + 3 if zero_n is None else zero_n, film, in32, bias)


PROLOGUE_CASES = (
    _pr("base"), _pr("mel-loop-arm", C=80, T=64), _pr("logits-general-k5", K=5), _pr("logits-general-c257", C=257, T=8), _pr("logits-k64", K=64),
    _pr("film-loop-arm", cond=513), _pr("film-512-register", cond=512), _pr("cond-truncates-emo", cond=8), _pr("cond-truncates-spk", cond=3),
    _pr("cond-zero-pads", cond=16), _pr("spk-only", de=0, cond=5), _pr("emo-only", ds=0, cond=6), _pr("B8", B=8), _pr("B9", B=9), _pr("B1", B=1),
    _pr("F2-16", F2=16), _pr("F2-1", F2=1), _pr("F2-33", F2=33), _pr("zero-0", zero_n=0), _pr("zero-1", zero_n=1), _pr("zero-B-1", zero_n=2),
    _pr("no-film", film=False), _pr("no-bias", bias=False), _pr("fp32-inputs", in32=True), _pr("fp32-inputs-loop-arms", C=80, T=64, cond=513, in32=True),
    _pr("t-odd", T=15), _pr("lds-65280", C=80, T=191, B=2),
)
# (name, overrides, in_dtype or None (= dtype), dtype, null spk, code)
PROLOGUE_REFUSED = (("C1025", dict(C=1025, T=1), None, MV_F32, False, MV_ERR_UNSUPPORTED), ("lds-65920", dict(C=80, T=192), None, MV_BF16, False, MV_ERR_UNSUPPORTED),
                    ("in-bf16-store-f16", {}, MV_BF16, MV_F16, False, MV_ERR_DTYPE), ("null-spk", {}, None, MV_F32, True, MV_ERR_ARG),
                    ("K65", dict(K=65), None, MV_F32, False, MV_ERR_ARG))


def prologue_plan(c):
    """The arms of gen_prologue_kernel a row takes and its launch: Refused as the host refuses."""
    if c.C > PRO_NT:
        raise Refused(MV_ERR_UNSUPPORTED)
    lds_sample = 4 * (c.C * (c.T | 1) + (PRO_NT // c.C) * c.C + c.C)
    lds_film = 4 * PRO_SG * c.cond if c.film else 0
    if max(lds_sample, lds_film) > 64 * 1024:
        raise Refused(MV_ERR_UNSUPPORTED)
    n_film = cdiv(c.F2, PRO_NT // 64) * cdiv(c.B, PRO_SG) if c.film else 0
    return dict(lds=max(lds_sample, lds_film), grid=c.B + n_film, roles=1 + int(n_film > 0), mel="reg" if c.C * c.T <= 4 * PRO_NT else "loop",
                logits="reg" if c.K <= 4 and c.C <= 256 else "general", film=None if not c.film else ("reg" if c.cond <= 512 else "loop"),
                cat="trunc" if c.cond < c.ds + c.de else ("pad" if c.cond > c.ds + c.de else "fit"))


@functools.lru_cache(maxsize=None)
def prologue_reference(c):
    """x_cl = mel transposed; proj = W cat(spk, emo)[:cond] (zero-padded) + b; alpha = softmax(Wa mean_t mel + ba).  With fp32 inputs the
    mel is made of multiples of 1/2048 (13 bits): the 16-bit x_cl rounds them, the means use them whole (exact sums; the logits then
    carry the lane chains' roundings like a row with an inexact mean)."""
    mel = ints((c.B, c.C, c.T), 281, lo=-4, hi=4)
    if c.in32:
        mel = ints((c.B, c.C, c.T), 281, lo=-8192, hi=8192) / 2048
    spk, emo = ints((c.B, max(c.ds, 1)), 282, lo=-4, hi=4)[:, :c.ds], ints((c.B, max(c.de, 1)), 283, lo=-4, hi=4)[:, :c.de]
    aw, ab = ints((c.K, c.C), 284), (ints((c.K,), 285) if c.bias else None)
    fw, fb = ints((c.F2, c.cond), 286), (ints((c.F2,), 287) if c.bias else None)
    cond = torch.zeros(c.B, c.cond, dtype=torch.float64)
    cat = torch.cat([spk, emo], 1)[:, :c.cond]
    cond[:, :cat.shape[1]] = cat
    proj = exact(F.linear(cond, fw, fb), F.linear(cond.abs(), fw.abs(), None if fb is None else fb.abs()))
    m, ma = mel.mean(2), mel.abs().mean(2)
    pow2 = c.T & (c.T - 1) == 0 and not c.in32
    logit, la = F.linear(m, aw, ab), F.linear(ma, aw.abs(), None if ab is None else ab.abs())
    unit = 1.0 / c.T
    delta = 0.0 if pow2 else ((1 + c.C // 64 + 8) * U32 * la).max().item()      # one division, then the lane chains and the wave tree
    alpha, tol = softmax_out(logit, delta, c.K)
    return dict(mel=mel, spk=spk, emo=emo, aw=aw, ab=ab, fw=fw, fb=fb, x_cl=exact(mel.transpose(1, 2).contiguous(), unit=1.0 / 2048 if c.in32 else 1.0), proj=proj,
                logit=exact(logit, la, unit) if pow2 else None, alpha=alpha, alpha_tol=tol)


# =============================================================================================== mv_grc_fold_weights
GRC_CASES = ((64, 64, 3, 4, 16), (64, 64, 3, 1, 16), (64, 64, 3, 2, 16), (32, 16, 5, 2, 1), (16, 32, 1, 1, 16), (64, 20, 5, 4, 16), (8, 8, 1, 2, 1))   # Cin Cout ks groups rank
GRC_REFUSED = ((64, 64, 2, 4, 16), (64, 64, 4, 1, 16), (6, 4, 3, 4, 2))          # even ks; Cin % groups


def grc_fold_plan(Cin, Cout, ks, groups, rank):
    """('lds' | 'global', dynamic LDS bytes, workgroups)."""
    if not (Cin > 0 and Cout > 0 and ks > 0 and ks % 2 and groups > 0 and Cin % groups == 0 and Cout % groups == 0 and rank > 0):
        raise Refused(MV_ERR_ARG)
    flds = 4 * (Cin * rank + rank * Cout + Cout * Cout + Cout * (Cin // groups) * ks)
    return ("lds" if flds <= 48 * 1024 else "global"), flds, cdiv(max(Cout * Cin * ks, Cout), 256)


@functools.lru_cache(maxsize=None)
def grc_fold_reference(Cin, Cout, ks, groups, rank):
    """hifigan_modified/grc_lora.py by index: comb[q][c][j] = conv_w[q][c - g cin_g][j] where c lies in q's group g, plus
    s (A B)[c][q] on the centre tap j = ks // 2 only; w_eff[o] = sum_q proj_w[o][q] comb[q]; b_eff = proj_w conv_b + proj_b.
    Operands in {-1, 0, 1} at density 1/2, s = 1/2."""
    sh = dict(conv_w=(Cout, Cin // groups, ks), conv_b=(Cout,), A=(Cin, rank), Bm=(rank, Cout), proj_w=(Cout, Cout), proj_b=(Cout,))
    i = {n: ints(s, 290 + j, 0.5, -1, 1) for j, (n, s) in enumerate(sh.items())}
    i["s"] = torch.tensor([0.5], dtype=torch.float64)
    cin_g, cout_g = Cin // groups, Cout // groups

    def fold(i):
        comb = torch.zeros(Cout, Cin, ks, dtype=torch.float64)
        for q in range(Cout):
            g = q // cout_g
            comb[q, g * cin_g:(g + 1) * cin_g] = i["conv_w"][q]
        lora = i["A"] @ i["Bm"]                                    # [Cin][Cout]
        comb[:, :, ks // 2] += i["s"] * lora.t()
        return torch.einsum("oq,qcj->ocj", i["proj_w"], comb), i["proj_w"] @ i["conv_b"] + i["proj_b"]
    w, b = fold(i)
    wa, ba = fold({n: v.abs() for n, v in i.items()})
    return i, dict(w_eff=exact(w, wa, 0.5), b_eff=exact(b, ba))
