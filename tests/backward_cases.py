"""Case tables, input generators and fp64 references of tests/test_gpu_backward_kernels.py (a plain module, imported like
tests/disc_cases.py; checked on the host by tests/test_host_backward_cases.py).

The kernels under test are the generator's backward kernels: csrc/backward.hip, mv_grc_fold_bwd / mv_loss_fwd_bwd / mv_scale(_to) of
csrc/train.hip and the per-sample ODConvTranspose bank gradient of csrc/disc_fused.hip with its two layout maps.  Each is called on its
own through the C ABI.

Operands are small integers (|v| <= 3), alpha rows are multiples of 1/8 that sum to 1, scalars are dyadic (lora_scaling 0.5, LeakyReLU
slope 0.5, dropout mask_scale 2, rstd a power of two, mean an integer).  Every term of every sum is then a multiple of a power of two
`unit`, and while sum|terms| / unit < 2^24 every partial sum, in any order and with or without fused multiply-adds, is exact in fp32:
the result equals the fp64 reference bit for bit.  Every reference below is returned as an `Out`:

    ref      the fp64 result
    abs_sum  sum|terms| of the same expression, element by element (fp64)
    unit     the power of two all terms are multiples of (exact outputs)
    k        0: bit equality is claimed (the host test proves abs_sum / unit < 2^24, and for outputs stored in the storage type that
             a round trip through bf16 and fp16 leaves ref unchanged); > 0: the number of fp32 roundings on the kernel's path, counted in
             a comment where the case is made, for the bound |got - ref| <= u_out |ref| + k 2^-24 abs_sum (+ the fp16 subnormal step)
    stored   True: the kernel writes it in the storage type; False: fp32

`wgrad_plan` and `odconvT_plan` restate the two host rules (mv_conv1d_wgrad, mv_odconvT_wgrad_mfma) independently of the library;
tests/test_host_backward_cases.py compares them with the library's own dry runs (mv_conv1d_wgrad_plan, mv_odconvT_wgrad_plan).
"""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

MV_F32, MV_BF16, MV_F16 = 0, 1, 2
MV_ERR_ARG, MV_ERR_DTYPE, MV_ERR_UNSUPPORTED = -1, -2, -3
ACT_NONE, ACT_LRELU, ACT_TANH, ACT_SILU = 0, 1, 2, 3
TORCH_DT = {MV_F32: torch.float32, MV_BF16: torch.bfloat16, MV_F16: torch.float16}
DT_NAME = {MV_F32: "f32", MV_BF16: "bf16", MV_F16: "f16"}
U_OUT = {MV_F32: 2.0 ** -24, MV_BF16: 2.0 ** -8, MV_F16: 2.0 ** -11}     # unit roundoff of a store (round to nearest)
TINY = {MV_F32: 0.0, MV_BF16: 0.0, MV_F16: 2.0 ** -25}                   # half the fp16 subnormal step
U32 = 2.0 ** -24
SLOPE, MASK_SCALE, LORA_S = 0.5, 2.0, 0.5

Out = namedtuple("Out", "ref abs_sum unit k stored")


def cdiv(a, b):
    return -(-a // b)


class Refused(Exception):
    def __init__(self, code):
        super().__init__(code)
        self.code = code


def exact(ref, abs_sum=None, unit=1.0, stored=False):
    return Out(ref, ref.abs() if abs_sum is None else abs_sum, unit, 0, stored)


def bounded(ref, abs_sum, k, stored=False):
    return Out(ref, abs_sum, None, k, stored)


def tolerance(out, dt):
    """Per-element bound of a k > 0 output written in type dt (MV_F32 for the fp32 outputs)."""
    return U_OUT[dt] * out.ref.abs() + out.k * U32 * out.abs_sum + TINY[dt]


def proves_exact(out):
    """What makes torch.equal a fair demand: partial sums fit 24 bits, and a stored result survives both 16-bit types."""
    ok = bool((out.abs_sum / out.unit).max() < 2 ** 24) and bool(((out.ref / out.unit).round() * out.unit == out.ref).all())
    if out.stored:
        ok = ok and all(torch.equal(out.ref.to(TORCH_DT[d]).double(), out.ref) for d in (MV_BF16, MV_F16))
    return ok


# ----------------------------------------------------------------------------------------------- input generators
def ints(shape, seed, density=1.0, lo=-3, hi=3):
    """fp64 integers in [lo, hi], a fraction `density` of them kept (the rest zero)."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(lo, hi + 1, tuple(shape), generator=g).double()
    if density < 1.0:
        v = v * (torch.rand(tuple(shape), generator=g) < density).double()
    return v


def alphas(B, K, seed):
    """[B][K] multiples of 1/8 summing to 1 per row (eight eighths dealt to the K banks; some banks get none)."""
    g = torch.Generator().manual_seed(seed)
    a = torch.zeros(B, K, dtype=torch.float64)
    a.scatter_add_(1, torch.randint(0, K, (B, 8), generator=g), torch.full((B, 8), 0.125, dtype=torch.float64))
    return a


# =============================================================================================== mv_conv1d_wgrad
WG_TT, WG_MAXKS = 64, 16
WgPlan = namedtuple("WgPlan", "tsplit tchunk gx gy gz lds zero_fill per_sample reduce4")


def wgrad_tsplit(B, Cin, Cout, Tout):
    """Time chunks per (sample, tile) of mv_conv1d_wgrad; 1 = one workgroup walks the sample (per-sample mode: the direct store)."""
    tiles = cdiv(Cin, 16) * cdiv(Cout, 16)
    t = max(1, min(cdiv(2048, tiles * B), cdiv(Tout, WG_TT)))
    return cdiv(Tout, cdiv(cdiv(Tout, t), WG_TT) * WG_TT)


def wgrad_lds(ks, stride, dil):
    return 4 * (16 * ((WG_TT - 1) * stride + (ks - 1) * dil + 1) + 16 * WG_TT + 32)


def wgrad_plan(B, Cin, Cout, Tout, ks, stride, dil, nbanks):
    """The host rule of mv_conv1d_wgrad restated: WgPlan or Refused(code)."""
    if not (B > 0 and Cin > 0 and Cout > 0 and Tout > 0 and 0 < ks <= WG_MAXKS and stride > 0 and dil > 0 and 1 <= nbanks <= 8):
        raise Refused(MV_ERR_ARG)
    lds = wgrad_lds(ks, stride, dil)
    if lds > 64 * 1024:
        raise Refused(MV_ERR_UNSUPPORTED)
    tsplit = wgrad_tsplit(B, Cin, Cout, Tout)
    if B * tsplit > 65535:
        raise Refused(MV_ERR_UNSUPPORTED)
    # the chunk length comes from the first guess of the split, the final split from the chunk length
    tiles = cdiv(Cin, 16) * cdiv(Cout, 16)
    guess = max(1, min(cdiv(2048, tiles * B), cdiv(Tout, WG_TT)))
    tchunk = cdiv(cdiv(Tout, guess), WG_TT) * WG_TT
    per_sample = int(nbanks > 1)
    reduce4 = -1 if not per_sample else int(nbanks <= 4 and (Cout * Cin * ks) % 4 == 0)
    return WgPlan(tsplit, tchunk, cdiv(Cin, 16), cdiv(Cout, 16), B * tsplit, lds, int(not per_sample or tsplit > 1), per_sample, reduce4)


WG = namedtuple("WG", "name B Cin Cout Tout ks stride pad dil nbanks density arm")   # arm: (tsplit, zero_fill, reduce4) expected


def _wg(name, B, Cin, Cout, Tout, ks, stride=1, pad=None, dil=1, nbanks=1, density=1.0, arm=None):
    pad = (ks - 1) * dil // 2 if pad is None else pad
    return WG(name, B, Cin, Cout, Tout, ks, stride, pad, dil, nbanks, density, arm)


WG_CASES = (
    # taps: ragged 2 x 2 tiles (Cin 17 -> remainder 1, Cout 18 -> remainder 2), centred padding, two 64-step iterations
    _wg("ks1", 2, 17, 18, 65, 1, arm=(2, 1, -1)), _wg("ks3", 2, 17, 18, 65, 3), _wg("ks7", 2, 17, 18, 65, 7),
    _wg("ks11", 2, 17, 18, 65, 11), _wg("ks16", 2, 17, 18, 65, 16),
    # stride, dilation, padding (none / larger than the halo: both zero-padded ends are read)
    _wg("s2", 2, 17, 18, 65, 3, stride=2), _wg("s8", 2, 17, 18, 65, 3, stride=8), _wg("s2-d3-k7", 2, 17, 18, 65, 7, stride=2, dil=3),
    _wg("d3", 2, 17, 18, 65, 3, dil=3), _wg("d5", 2, 17, 18, 65, 7, dil=5), _wg("pad0", 2, 17, 18, 65, 3, pad=0),
    _wg("pad0-d5", 2, 17, 18, 65, 3, pad=0, dil=5), _wg("pad>halo", 2, 17, 18, 65, 3, pad=4), _wg("pad>halo-s2", 2, 17, 18, 65, 7, stride=2, pad=9),
    # time arms
    _wg("t200-split4", 2, 17, 18, 200, 3, arm=(4, 1, -1)), _wg("t200-split4-k4", 2, 17, 20, 200, 3, nbanks=4, arm=(4, 1, 1)),
    _wg("t200-split2", 16, 128, 128, 200, 3, nbanks=4, density=0.125, arm=(2, 1, 1)),
    _wg("t130-direct", 32, 128, 128, 130, 3, nbanks=4, density=0.125, arm=(1, 0, 1)),
    _wg("t1", 2, 17, 18, 1, 3, arm=(1, 1, -1)), _wg("t63", 2, 17, 18, 63, 3, arm=(1, 1, -1)), _wg("t64", 2, 17, 18, 64, 3, arm=(1, 1, -1)),
    _wg("t65", 2, 17, 20, 65, 3, nbanks=2, arm=(2, 1, 1)), _wg("t64-k2", 2, 17, 20, 64, 3, nbanks=2, arm=(1, 0, 1)),
    _wg("t1-k5", 3, 17, 18, 1, 7, nbanks=5, arm=(1, 0, 0)),
    # output modes and the two reductions
    _wg("k2-reduce4", 3, 17, 20, 65, 3, nbanks=2, arm=(2, 1, 1)), _wg("k4-reduce4", 3, 17, 20, 65, 3, nbanks=4, arm=(2, 1, 1)),
    _wg("k5-generic", 3, 17, 20, 65, 3, nbanks=5, arm=(2, 1, 0)), _wg("k8-generic", 3, 17, 20, 65, 3, nbanks=8, arm=(2, 1, 0)),
    _wg("k4-odd-nelem", 3, 3, 5, 65, 3, nbanks=4, arm=(2, 1, 0)), _wg("k4-nelem%4=2", 2, 17, 18, 65, 3, nbanks=4, arm=(2, 1, 0)),
    # the largest accepted window: stride 8, 16 taps, dilation 30 -> 65344 bytes of LDS
    _wg("lds-65344", 1, 17, 18, 65, 16, stride=8, pad=0, dil=30, density=0.25),
)
WG_REFUSED = (("ks17", (2, 17, 18, 65, 17, 1, 1, 1), MV_ERR_ARG), ("lds-66304", (1, 17, 18, 65, 16, 8, 31, 1), MV_ERR_UNSUPPORTED),
              ("B65536", (65536, 16, 16, 64, 3, 1, 1, 1), MV_ERR_UNSUPPORTED), ("nbanks9", (2, 17, 18, 65, 3, 1, 1, 9), MV_ERR_ARG))


def wg_tin(c):
    """The shortest input that yields Tout outputs."""
    return (c.Tout - 1) * c.stride + (c.ks - 1) * c.dil + 1 - 2 * c.pad


def persample_wgrad(x, gy, ks, stride, pad, dil):
    """F.conv1d autograd in fp64, all samples at once (samples as groups): tiles [B][Cout][Cin][ks]."""
    B, Cin, Tin = x.shape
    Cout, Tout = gy.shape[1:]
    w = torch.zeros(B * Cout, Cin, ks, dtype=torch.float64, requires_grad=True)
    y = F.conv1d(x.reshape(1, B * Cin, Tin), w, None, stride, pad, dil, groups=B)
    assert y.shape[2] == Tout, (y.shape, Tout)
    (gw,) = torch.autograd.grad(y, w, gy.reshape(1, B * Cout, Tout))
    return gw.view(B, Cout, Cin, ks)


def alpha_chain(tiles, tiles_abs, w, alpha, galpha0):
    """gw[k] = sum_b alpha[b,k] tile_b (multiples of 1/8); galpha[b,k] = galpha0 + <tile_b, w[k]>."""
    B, K = alpha.shape
    tb, ta = tiles.reshape(B, -1), tiles_abs.reshape(B, -1)
    gw = exact((alpha.t() @ tb).view(K, *tiles.shape[1:]), (alpha.t() @ ta).view(K, *tiles.shape[1:]), 0.125)
    wf = w.reshape(K, -1)
    return gw, exact(galpha0 + tb @ wf.t(), galpha0.abs() + ta @ wf.abs().t())


@functools.lru_cache(maxsize=None)
def wg_reference(c):
    """Inputs and references of one mv_conv1d_wgrad row: dict with x, gy, w, alpha, galpha0 (inputs), gw, galpha (Out)."""
    Tin = wg_tin(c)
    assert Tin > 0, c
    x, gy = ints((c.B, c.Cin, Tin), 11, c.density), ints((c.B, c.Cout, c.Tout), 12, c.density)
    tiles = persample_wgrad(x, gy, c.ks, c.stride, c.pad, c.dil)
    tabs = persample_wgrad(x.abs(), gy.abs(), c.ks, c.stride, c.pad, c.dil)
    r = dict(x=x, gy=gy, Tin=Tin, tiles=exact(tiles, tabs))
    if c.nbanks == 1:
        r.update(gw=exact(tiles.sum(0), tabs.sum(0)))
        return r
    w, alpha, ga0 = ints((c.nbanks, c.Cout, c.Cin, c.ks), 13), alphas(c.B, c.nbanks, 14), ints((c.B, c.nbanks), 15, lo=-9, hi=9)
    gw, ga = alpha_chain(tiles, tabs, w, alpha, ga0)
    r.update(w=w, alpha=alpha, galpha0=ga0, gw=gw, galpha=ga)
    return r


# the generator's own layers (B, Cin, Cout, Tout, ks, stride, dil, nbanks) -> (tsplit, zero_fill, reduce4): input projection at both
# batch sizes of test_gpu_generator_train_shapes.py, and an upsampler's swapped-role call
WG_KNOWN = (((2, 80, 512, 32, 7, 1, 1, 4), (1, 0, 1)), ((16, 80, 512, 200, 7, 1, 1, 4), (1, 0, 1)), ((2, 80, 512, 200, 7, 1, 1, 4), (4, 1, 1)),
            ((16, 256, 512, 32, 16, 8, 1, 4), (1, 0, 1)))

# reduction alone
REDUCE_CASES = tuple((B, K, n) for B, K, n in ((1, 1, 4), (3, 4, 1024), (3, 4, 1023), (3, 4, 1025), (3, 4, 1028), (33, 4, 1028), (33, 5, 1028),
                                               (3, 8, 1024), (1, 5, 4), (33, 1, 1025), (3, 8, 1023)))


@functools.lru_cache(maxsize=None)
def reduce_reference(B, K, n):
    tiles, w, alpha, ga0 = ints((B, n), 21, lo=-40, hi=40), ints((K, n), 22), alphas(B, K, 23), ints((B, K), 24, lo=-9, hi=9)
    gw, ga = alpha_chain(tiles, tiles.abs(), w, alpha, ga0)
    return dict(tiles=tiles, w=w, alpha=alpha, galpha0=ga0, gw=gw, galpha=ga, reduce4=int(K <= 4 and n % 4 == 0))


# =============================================================================================== mv_bias_grad
BIAS_CASES = tuple((B, C, T, K, has_bias) for B, C, T, K, has_bias in (
    (1, 7, 1, 1, False), (1, 7, 63, 1, False), (1, 7, 64, 4, True), (1, 7, 65, 4, False), (1, 7, 200, 4, True), (40, 3, 65, 4, True),
    (3, 5, 200, 8, True), (40, 3, 1, 1, False)))


@functools.lru_cache(maxsize=None)
def bias_reference(B, C, T, K, has_bias):
    gy, alpha, bias, ga0 = ints((B, C, T), 31), alphas(B, K, 32), ints((K, C), 33), ints((B, K), 34, lo=-9, hi=9)
    rs, ra = gy.sum(2), gy.abs().sum(2)
    a = alpha if K > 1 else torch.ones(B, 1, dtype=torch.float64)
    r = dict(gy=gy, alpha=alpha, bias=bias, galpha0=ga0, rowsum=exact(rs, ra), gbias=exact(a.t() @ rs, a.t() @ ra, 0.125))
    r["galpha"] = exact(ga0 + rs @ bias.t(), ga0.abs() + ra @ bias.abs().t()) if (K > 1 and has_bias) else exact(ga0)
    return r


# =============================================================================================== mv_odconv_attn_bwd, mv_add_rowconst
ATTN_CASES = tuple((B, C, K, T) for B, C, K, T in ((70, 80, 4, 64), (3, 1, 1, 8), (3, 513, 8, 4), (70, 80, 4, 3), (2, 513, 4, 3), (5, 80, 8, 1)))
ROWCONST_CASES = ((3, 1), (3, 255), (2, 256), (2, 257), (2, 16385), (300, 7))


@functools.lru_cache(maxsize=None)
def attn_reference(B, C, K, T):
    alpha, ga, pooled, wa = alphas(B, K, 41), ints((B, K), 42, lo=-9, hi=9), ints((B, C), 43), ints((K, C), 44)
    dot = (alpha * ga).sum(1, keepdim=True)
    gz = alpha * (ga - dot)                                   # multiples of 1/64
    gza = alpha * (ga.abs() + (alpha * ga.abs()).sum(1, keepdim=True))
    s, sa = gz @ wa, gza @ wa.abs()
    if T & (T - 1) == 0:
        gm = exact(s / T, sa / T, 1.0 / (64 * T))
    else:
        gm = bounded(s / T, sa / T, 2)                        # k = 2: 1.f / T on the host, then one multiply (the sum itself is exact)
    return dict(alpha=alpha, galpha=ga, pooled=pooled, wa=wa, gwa=exact(gz.t() @ pooled, gza.t() @ pooled.abs(), 1 / 64),
                gba=exact(gz.sum(0), gza.sum(0), 1 / 64), gm=gm)


# =============================================================================================== mv_groupnorm_bwd
GN_SHAPES = ((2, 8, 2, 64), (2, 8, 2, 63), (2, 8, 2, 65), (3, 6, 3, 8), (1, 2, 1, 131080), (1, 2, 1, 16385))


def gn_inputs(B, C, G, T, seed=51):
    """x, gy, affine: integers; mean an integer and rstd a power of two per (b, g); a keep-mask of bytes (0 / 1, and one 255)."""
    dens = 1.0 if T < 4096 else 0.0625
    g = torch.Generator().manual_seed(seed)
    x, gy = ints((B, C, T), seed, 1.0), ints((B, C, T), seed + 1, dens)
    mean = torch.randint(-1, 2, (B, G), generator=g).double()
    rstd = 2.0 ** torch.randint(-1, 2, (B, G), generator=g).double()
    gw, gb = ints((C,), seed + 2, lo=-2, hi=2), ints((C,), seed + 3, lo=-2, hi=2)
    gw[gw == 0] = 1.0
    mask = (torch.rand((B, C, T), generator=g) < 0.75).to(torch.uint8)
    mask.view(-1)[mask.view(-1).nonzero()[0]] = 255          # any non-zero byte keeps
    return dict(x=x, gy=gy, mean=mean, rstd=rstd, gw=gw, gb=gb, mask=mask)


def gn_z(i, G, use_gw=True, use_gb=True):
    B, C, T = i["x"].shape
    mu, rs = i["mean"].repeat_interleave(C // G, 1)[:, :, None], i["rstd"].repeat_interleave(C // G, 1)[:, :, None]
    xh = (i["x"] - mu) * rs
    z = xh * (i["gw"][None, :, None] if use_gw else 1.0) + (i["gb"][None, :, None] if use_gb else 0.0)
    return xh, z, rs


def gn_dact(z, act):
    """d act / dz in fp64; LeakyReLU with the project's convention (1 at z == +0 and -0)."""
    if act == ACT_LRELU:
        return torch.where(z >= 0, 1.0, SLOPE).double()
    if act == ACT_TANH:
        return 1.0 - torch.tanh(z) ** 2
    if act == ACT_SILU:
        sg = torch.sigmoid(z)
        return sg * (1.0 + z * (1.0 - sg))
    return torch.ones_like(z)


def gn_gz(i, G, act, with_mask, use_gw=True, use_gb=True):
    """gz = gy * mask * mask_scale * act'(z): exact (multiples of 1/2, |.| <= 6) for none / lrelu."""
    _, z, _ = gn_z(i, G, use_gw, use_gb)
    g = i["gy"] * ((i["mask"] != 0).double() * MASK_SCALE if with_mask else 1.0)
    return g * gn_dact(z, act)


def gn_from_gz(i, gz, G, T_chain, use_gw=True, exact_gz=True):
    """The stages behind gz, from a given gz (the exact one, or the kernel's own read back for SiLU / tanh): dgw, dgb [C], gx.
    exact_gz: gz holds multiples of 1/2 -> the sums are exact.  Otherwise the sums carry
      k = T_chain + 16 + B: a thread's serial chain (T_chain adds), product and xh roundings (3), two 6-step wave butterflies and the
      4-wave fold (13), the colsum over B samples (B).
    gx = rstd (gz gw - s1/n - xh s2/n): exact when n = cg T is a power of two and the result has <= 24 bits; the test asks for the
      bound with k = 7 otherwise and for every 16-bit store: 1/n, two products with it, xh * s2/n, two subtractions, and one spare
      for the (1 + u_out) factor the store puts on the fp32 error.  With an inexact gz the k of the sums and the cg adds of the group
      sums come on top, against the sums of absolute values."""
    B, C, T = gz.shape
    cg = C // G
    xh, _, rs = gn_z(i, G, use_gw)
    gam = i["gw"][None, :, None] if use_gw else torch.ones(1, C, 1, dtype=torch.float64)
    dgb_bc, dgw_bc = gz.sum(2), (gz * xh).sum(2)
    dgb_a, dgw_a = gz.abs().sum(2), (gz * xh).abs().sum(2)
    s1 = (gam[:, :, 0] * dgb_bc).view(B, G, cg).sum(2).repeat_interleave(cg, 1)[:, :, None]
    s2 = (gam[:, :, 0] * dgw_bc).view(B, G, cg).sum(2).repeat_interleave(cg, 1)[:, :, None]
    n = cg * T
    gx = rs * (gz * gam - s1 / n - xh * s2 / n)
    if exact_gz:
        gxa = rs * ((gz * gam).abs() + s1.abs() / n + (xh * s2).abs() / n)
        dgw, dgb = exact(dgw_bc.sum(0), dgw_a.sum(0), 0.125), exact(dgb_bc.sum(0), dgb_a.sum(0), 0.5)
        return dict(dgw=dgw, dgb=dgb, gx=bounded(gx, gxa, 7, stored=True), s1=s1, s2=s2)
    # inexact sums: s1 and s2 carry the roundings of their own T-long sums, relative to the sums of absolute values
    k = T_chain + 16 + B
    s1a = (gam[:, :, 0].abs() * dgb_a).view(B, G, cg).sum(2).repeat_interleave(cg, 1)[:, :, None]
    s2a = (gam[:, :, 0].abs() * dgw_a).view(B, G, cg).sum(2).repeat_interleave(cg, 1)[:, :, None]
    gxa = rs * ((gz * gam).abs() + s1a / n + xh.abs() * s2a / n)
    dgw, dgb = bounded(dgw_bc.sum(0), dgw_a.sum(0), k), bounded(dgb_bc.sum(0), dgb_a.sum(0), k)
    return dict(dgw=dgw, dgb=dgb, gx=bounded(gx, gxa, 7 + k + cg, stored=True), s1=s1, s2=s2)


# =============================================================================================== FiLM, linear, avgpool, copy2d, act
FILM_CASES = ((2, 5, 3, 255), (2, 4, 4, 257), (2, 3, 5, 1), (1, 6, 2, 257))          # (B, C, F, T)
LINEAR_CASES = ((2, 300, 1), (37, 5, 64), (1, 1, 1))                                # (M, N, Kd)
AVGPOOL_CASES = ((10, 4), (8, 1), (9, 2), (515, 2))                                 # (T, s)
CONV2D_CASES = ((2, 3, 5, 4, 40, 3, 3, 1, 1), (1, 2, 3, 9, 6, 5, 1, 2, 0), (2, 5, 3, 3, 40, 1, 15, 0, 7))   # B Cin Cout H W kh kw ph pw
LOSS_N = (1, 255, 256, 131073, 4096)


@functools.lru_cache(maxsize=None)
def film_reference(B, C, Fd, T):
    x, gy, proj = ints((B, C, T), 61), ints((B, C, T), 62), ints((B, 2 * Fd), 63)
    gam = torch.ones(B, C, dtype=torch.float64)
    m = min(C, Fd)
    gam[:, :m] = proj[:, :m]
    gp, gpa = torch.zeros(B, 2 * Fd, dtype=torch.float64), torch.zeros(B, 2 * Fd, dtype=torch.float64)
    gp[:, :m], gp[:, Fd:Fd + m] = (gy * x).sum(2)[:, :m], gy.sum(2)[:, :m]
    gpa[:, :m], gpa[:, Fd:Fd + m] = (gy * x).abs().sum(2)[:, :m], gy.abs().sum(2)[:, :m]
    return dict(x=x, gy=gy, proj=proj, gx=exact(gy * gam[:, :, None], stored=True), gproj=exact(gp, gpa))


@functools.lru_cache(maxsize=None)
def linear_reference(M, N, Kd):
    x, w, gy = ints((M, Kd), 71), ints((N, Kd), 72), ints((M, N), 73)
    return dict(x=x, w=w, gy=gy, gx=exact(gy @ w, gy.abs() @ w.abs()), gw=exact(gy.t() @ x, gy.abs().t() @ x.abs()),
                gb=exact(gy.sum(0), gy.abs().sum(0)))


def avgpool_reference(T, s, rows=3):
    gy = ints((rows, T // s), 81)
    gx = torch.zeros(rows, T, dtype=torch.float64)
    gx[:, :(T // s) * s] = gy.repeat_interleave(s, 1) / s            # s is a power of two in every row of the table
    return dict(gy=gy, gx=exact(gx, unit=1.0 / s, stored=True))


def act_reference():
    """y straddles zero and holds +0 and -0; tanh outputs are multiples of 1/4, so 1 - y^2 has 4 fractional bits."""
    y = torch.tensor([-3.0, -1.0, -0.5, -0.25, -0.0, 0.0, 0.25, 0.5, 0.75, 1.0, 2.0, 3.0] * 23, dtype=torch.float64)
    gy = ints(y.shape, 91)
    gy[gy == 0] = 2.0
    yt = y.clamp(-1, 1)
    return dict(y=y, gy=gy, yt=yt, none=exact(gy.clone(), stored=True), lrelu=exact(gy * torch.where(y >= 0, 1.0, SLOPE), unit=0.5, stored=True),
                tanh=exact(gy * (1 - yt * yt), unit=1 / 16, stored=True))


@functools.lru_cache(maxsize=None)
def conv2d_reference(B, Cin, Cout, H, W, kh, kw, ph, pw):
    """F.conv2d autograd in fp64 for the weight gradient; the flip map restated by index."""
    x = ints((B, Cin, H, W), 101)
    Ho, Wo = H + 2 * ph - kh + 1, W + 2 * pw - kw + 1
    gy, w = ints((B, Cout, Ho, Wo), 102), ints((Cout, Cin, kh, kw), 103)

    def wg(a, b):
        wz = torch.zeros(Cout, Cin, kh, kw, dtype=torch.float64, requires_grad=True)
        return torch.autograd.grad(F.conv2d(a, wz, None, 1, (ph, pw)), wz, b)[0]
    return dict(x=x, gy=gy, w=w, gw=exact(wg(x, gy), wg(x.abs(), gy.abs())), wt=exact(w.flip(2, 3).transpose(0, 1).contiguous(), stored=True))


def loss_reference(kind, n, c=1.0, weight=0.5, acc0=5.0):
    """Kinds 0-4 of mv_loss_fwd_bwd.  n a power of two: weight / n is exact and so is everything else.  Otherwise
    gx: k = 2 (the division weight / n, one product); loss: k = 2 + nblocks (the same two, then one atomic add per workgroup)."""
    x, y = ints((n,), 111), ints((n,), 112)
    d = {0: x - c, 1: x - y, 2: 1 - x, 3: 1 + x, 4: x - y}[kind]
    if kind in (0, 4):
        l, g = d * d, 2 * d
    elif kind == 1:
        l, g = d.abs(), torch.sign(d)
    else:
        l, g = d.clamp(min=0), (d > 0).double() * (-1.0 if kind == 2 else 1.0)
    inv = weight / n
    if n & (n - 1) == 0:
        return dict(x=x, y=y, gx=exact(g * inv, unit=inv, stored=True), loss=exact(torch.tensor([acc0 + l.sum() * inv]), torch.tensor([acc0 + l.sum() * inv]), inv))
    nblocks = min(512, cdiv(n, 256))
    return dict(x=x, y=y, gx=bounded(g * inv, (g * inv).abs(), 2, stored=True),
                loss=bounded(torch.tensor([acc0 + l.sum() * inv]), torch.tensor([acc0 + l.sum() * inv]), 2 + nblocks))


# =============================================================================================== mv_grc_fold_bwd
GRC_CASES = ((64, 20, 3, 4, 16), (16, 16, 3, 1, 4), (64, 40, 3, 4, 16))      # (Cin, Cout, ks, groups, rank)
GRC_REFUSED = (64, 64, 3, 1, 16)


def grc_lds(Cin, Cout, ks, groups, rank):
    return 4 * (2 * Cout * Cin * ks + Cin * Cout + 32 + Cout * (Cin // groups) * ks + Cout * Cout + Cin * rank + rank * Cout)


def grc_inputs(Cin, Cout, ks, groups, rank):
    """Sparse operands in {-1, 0, 1} (the scalar gradient sums Cin * Cout products of two inner sums)."""
    sh = dict(g_weff=(Cout, Cin, ks), g_beff=(Cout,), conv_w=(Cout, Cin // groups, ks), conv_b=(Cout,), A=(Cin, rank), Bm=(rank, Cout),
              proj_w=(Cout, Cout), )
    i = {n: ints(s, 120 + j, 0.5, -1, 1) for j, (n, s) in enumerate(sh.items())}
    i["s"] = torch.tensor([LORA_S], dtype=torch.float64)
    return i


def grc_fold(i, groups):
    """The forward fold (norm_elem.hip grc_fold_kernel) in fp64: (w_eff, b_eff)."""
    Wc, A, Bm, P, s = i["conv_w"], i["A"], i["Bm"], i["proj_w"], i["s"]
    Cout, cin_g, ks = Wc.shape
    Cin = cin_g * groups
    comb = torch.zeros(Cout, Cin, ks, dtype=torch.float64)
    for g in range(groups):
        o0, o1 = g * Cout // groups, (g + 1) * Cout // groups
        comb[o0:o1, g * cin_g:(g + 1) * cin_g] = Wc[o0:o1]
    mid = torch.zeros(ks, dtype=torch.float64)
    mid[ks // 2] = 1.0
    comb = comb + s * (A @ Bm).t()[:, :, None] * mid
    return torch.einsum("oq,qcj->ocj", P, comb), P @ i["conv_b"], comb


def grc_reference(Cin, Cout, ks, groups, rank):
    """Closed form of the seven gradients (conv_w, conv_b, A, B, s, proj_w, proj_b) with sum|terms| of each."""
    i = grc_inputs(Cin, Cout, ks, groups, rank)

    def grads(i, absolute):
        f = (lambda t: t.abs()) if absolute else (lambda t: t)
        gw, gb, Wc, bc, A, Bm, P, s = (f(i[n]) for n in ("g_weff", "g_beff", "conv_w", "conv_b", "A", "Bm", "proj_w", "s"))
        _, _, comb = grc_fold({**i, **dict(conv_w=Wc, A=A, Bm=Bm, proj_w=P, s=s)}, groups)
        L, mid, cin_g = A @ Bm, ks // 2, Cin // groups
        gcomb = torch.einsum("oq,ocj->qcj", P, gw)
        g_conv_w = torch.stack([gcomb[o, (o // (Cout // groups)) * cin_g:(o // (Cout // groups) + 1) * cin_g] for o in range(Cout)])
        gL = s * gcomb[:, :, mid].t()                                                        # [Cin][Cout]
        return dict(g_conv_w=g_conv_w, g_conv_b=P.t() @ gb, g_A=gL @ Bm.t(), g_B=A.t() @ gL, g_s=(L * gcomb[:, :, mid].t()).sum().view(1),
                    g_proj_w=torch.einsum("ocj,qcj->oq", gw, comb) + gb[:, None] * bc[None, :], g_proj_b=gb.clone())
    r, a = grads(i, False), grads(i, True)
    return i, {n: exact(r[n], a[n], 0.5) for n in r}


# =============================================================================================== ODConvTranspose bank gradient (MFMA)
def odconvT_plan(B, Tin, Cin, Cout, ks, stride, K, dtype):
    """mv_odconvT_wgrad_mfma's per-sample two-tap plan restated: the twelve integers of mv_dconv_wgrad_plan, or Refused(code)."""
    if not (B > 0 and Tin > 0 and Cin > 0 and Cout > 0 and stride > 0 and 1 <= K <= 8 and ks == 2 * stride):
        raise Refused(MV_ERR_ARG)
    if Cin % 8 or (stride * Cout) % 8:
        raise Refused(MV_ERR_ARG)
    if dtype not in (MV_BF16, MV_F16):
        raise Refused(MV_ERR_UNSUPPORTED)
    wt, halo = 128, 1
    lds = 2 * (wt + wt + halo) * 160
    wsplit = cdiv(Tin, wt)
    nchunks = B * wsplit
    if nchunks > 2 ** 30 or B > 65535:
        raise Refused(MV_ERR_UNSUPPORTED)
    # family 0, TW 2, 128 positions a chunk, 64-channel tiles; a workgroup owns one (tile, sample) and walks its wsplit chunks
    return (0, 2, wt, 64, wsplit, nchunks, wsplit, B, lds, cdiv(stride * Cout, 64), cdiv(Cin, 64), B)


ODT_SHAPES = ((8, 4, 4, 2), (64, 32, 4, 2), (72, 24, 6, 3), (64, 136, 2, 1))          # (Cin, Cout, ks, stride)
# (shape index, B, Tin, K): one, two and three 128-position chunks a sample, both reductions
ODT_CASES = ((0, 1, 1, 1), (0, 3, 127, 4), (0, 3, 128, 5), (0, 1, 129, 8), (0, 3, 257, 4), (1, 3, 129, 4), (1, 1, 257, 8), (2, 3, 127, 5),
             (2, 1, 257, 4), (3, 3, 128, 1), (3, 1, 129, 4))


def odt_pad_grad(g, Tin, stride, pad):
    """g [B][Cout][Tout] -> gp [B][Tin+1][stride*Cout]: row q, channel r*Cout + o = g[o][q*stride + r - pad], zero outside."""
    B, Cout, Tout = g.shape
    gp = torch.zeros(B, (Tin + 1) * stride, Cout, dtype=g.dtype)
    gp[:, pad:pad + Tout] = g.transpose(1, 2)
    return gp.view(B, Tin + 1, stride * Cout)


@functools.lru_cache(maxsize=None)
def odt_reference(si, B, Tin, K):
    """F.conv_transpose1d autograd in fp64, per sample (samples as groups), with the generator's own padding = stride // 2 and
    output_padding = stride % 2 (ks 6, stride 3: the output_padding = 1 geometry; stride 1: neither)."""
    Cin, Cout, ks, stride = ODT_SHAPES[si]
    pad, opad = stride // 2, (stride % 2 if stride > 1 else 0)
    Tout = (Tin - 1) * stride - 2 * pad + ks + opad
    dens = min(1.0, 24.0 / Tin)
    x, g = ints((B, Cin, Tin), 131, dens), ints((B, Cout, Tout), 132, dens)

    def tiles(x, g):
        w = torch.zeros(B * Cin, Cout, ks, dtype=torch.float64, requires_grad=True)
        y = F.conv_transpose1d(x.reshape(1, B * Cin, Tin), w, None, stride, pad, opad, groups=B)
        return torch.autograd.grad(y, w, g.reshape(1, B * Cout, Tout))[0].view(B, Cin, Cout, ks)
    w, alpha, ga0 = ints((K, Cin, Cout, ks), 133), alphas(B, K, 134), ints((B, K), 135, lo=-9, hi=9)
    gw, ga = alpha_chain(tiles(x, g), tiles(x.abs(), g.abs()), w, alpha, ga0)
    return dict(x_cl=x.transpose(1, 2).contiguous(), g=g, gp=odt_pad_grad(g, Tin, stride, pad), w=w, alpha=alpha, galpha0=ga0, gw=gw, galpha=ga,
                pad=pad, Tout=Tout)


def adjoint_weights(w, stride):
    """out[k][c][r*Cout + o][q] = w[k][c][o][q*stride + r]."""
    K, Cin, Cout, ks = w.shape
    return w.view(K, Cin, Cout, 2, stride).permute(0, 1, 4, 2, 3).reshape(K, Cin, stride * Cout, 2).contiguous()


# the generator's upsamplers in 16-bit training (B, Tin, Cin, Cout, ks, stride, K) -> (chunks per sample, grid x, y, z)
ODT_KNOWN = (((16, 32, 512, 256, 16, 8, 4), (1, 32, 8, 16)), ((16, 256, 256, 128, 16, 8, 4), (2, 16, 4, 16)),
             ((16, 2048, 128, 64, 4, 2, 4), (16, 2, 2, 16)), ((16, 4096, 64, 32, 4, 2, 4), (32, 1, 1, 16)))


# =============================================================================================== mv_copy2d
# (name, n, rows_outer, rows_inner, +s_os, +s_rs, +d_os, +d_rs, src element offset, dst element offset): the vector path needs n, the
# four strides (elements) and both addresses to be whole 16-byte pieces; each row after the first falsifies one term.  Base strides are
# multiples of 8 elements, so they are whole pieces in fp32 (4 a piece) and in 16-bit storage (8 a piece) alike.
COPY_CASES = (("vector", 64, 3, 5, 0, 0, 0, 0, 0, 0), ("n", 63, 3, 5, 0, 0, 0, 0, 0, 0), ("s_os", 64, 3, 5, 1, 0, 0, 0, 0, 0),
              ("s_rs", 64, 3, 5, 0, 1, 0, 0, 0, 0), ("d_os", 64, 3, 5, 0, 0, 1, 0, 0, 0), ("d_rs", 64, 3, 5, 0, 0, 0, 1, 0, 0),
              ("src", 64, 3, 5, 0, 0, 0, 0, 1, 0), ("dst", 64, 3, 5, 0, 0, 0, 0, 0, 1),
              ("second-pass", 64 * 256 * 8 + 8, 1, 2, 0, 0, 0, 0, 0, 0), ("second-pass-scalar", 64 * 256 + 1, 2, 1, 0, 0, 0, 0, 0, 0),
              ("one", 1, 1, 1, 0, 0, 0, 0, 0, 0))


def copy_layout(case):
    """Element strides and buffer sizes of a copy2d case: rows are 16 elements apart from each other beyond their length."""
    _, n, ro, ri, a_os, a_rs, b_os, b_rs, s_off, d_off = case
    rs = (n + 7) // 8 * 8 + 16
    s_rs, d_rs = rs + a_rs, rs + 8 + b_rs
    s_os, d_os = ri * s_rs + 8 + a_os, ri * d_rs + 16 + b_os
    return dict(n=n, ro=ro, ri=ri, s_rs=s_rs, d_rs=d_rs, s_os=s_os, d_os=d_os, s_off=s_off, d_off=d_off,
                s_len=ro * s_os + 16, d_len=ro * d_os + 16)


def copy_takes_vector(case, dt):
    L = copy_layout(case)
    epv = 4 if dt == MV_F32 else 8
    return all(v % epv == 0 for v in (L["n"], L["s_rs"], L["d_rs"], L["s_os"], L["d_os"], L["s_off"], L["d_off"]))
