"""The channels-last discriminator kernels of csrc/disc_fused.hip, one entry point at a time through the raw C ABI, against float64
torch on the CPU - bit for bit.  Inputs are small integers (tests/disc_cases.py), so every sum is exact in fp32 in any order and every
result is representable in bf16, fp16 and fp32: one wrong channel in one edge column, a position counted twice or dropped, a bias
added after rounding all change at least one output element and fail torch.equal.  The case tables hold one row per instantiation
the dispatchers can select, with ragged companions; the real-valued tests then bound every element by what the formats allow."""
import ctypes

import numpy as np
import pytest
import torch

import disc_cases as D
from disc_cases import MV_BF16, MV_F16, MV_F32, TORCH_DT

pytestmark = pytest.mark.gpu

ACT_NONE, ACT_LRELU = 0, 1
ALL_DT = (MV_BF16, MV_F16, MV_F32)
DT16 = (MV_BF16, MV_F16)


@pytest.fixture(scope="module")
def L():
    from hifigan_modified import _native
    return _native.lib()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(fn, *args):
    """fn(*args, stream) with every tensor passed as its device address (the tensors stay referenced for the duration of the call)."""
    return fn(*[_p(a) if isinstance(a, torch.Tensor) else a for a in args], _s())


def dev(t, dt):
    return t.to(TORCH_DT[dt]).cuda().contiguous()


def filled(shape, dt, value=float("nan")):
    return torch.full(tuple(shape), value, dtype=TORCH_DT[dt] if isinstance(dt, int) else dt, device="cuda")


def misaligned(t):
    """The same values at an address one element past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device="cuda")
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


def assert_same(got, want, what):
    """Bit equality of every element (as float64 on the CPU), with the first wrong elements named."""
    got = got.detach().double().cpu()
    want = want.double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if torch.equal(got, want):
        return
    bad = (got != want) | torch.isnan(got)
    idx = bad.nonzero()[:6].tolist()
    raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements differ; first (index, got, want): "
                         + "; ".join(f"{tuple(i)} {got[tuple(i)].item()} {want[tuple(i)].item()}" for i in idx))


def pack(L, w, flip, dt, coutp=None, cinp=None):
    """mv_dconv_pack_pad of an fp32 master w [Cout, Cin, kh, kw]."""
    Cout, Cin, kh, kw = w.shape
    coutp, cinp = coutp or Cout, cinp or Cin
    wf = w.float().cuda().contiguous()
    buf = torch.empty(L.mv_dconv_packed_bytes(coutp, cinp, kh, kw, dt), dtype=torch.uint8, device="cuda")
    rc = call(L.mv_dconv_pack_pad, wf, MV_F32, buf, Cout, Cin, kh, kw, coutp, cinp, flip, dt)
    assert rc == 0, rc
    return buf


def conv(L, x, pk, bias, save, y, c, act, slope, Cin=None, Cout=None):
    return call(L.mv_dconv_cl_fwd, x, pk, bias, save, y, c.B, c.H, c.W, Cin or c.Cin, Cout or c.Cout, c.kh, c.kw, c.dil,
                             act, slope, c.dtype)


# =============================================================================================== forward, bit-exact
@pytest.mark.parametrize("c", D.FWD_CASES, ids=D.case_id)
def test_forward_exact(L, c):
    """y = act(conv(x) + bias) with and without bias, without activation and with LeakyReLU(0.5), and the act_save data-gradient form
    (flip = 1 pack of a layer whose output width is this call's Cin; saved activations include +0.0 and -0.0)."""
    shape = D.shape_of(c)
    x, w, b, ref = D.fwd_reference(shape)
    xd, bd, pk = dev(x, c.dtype), dev(b, c.dtype), pack(L, w, 0, c.dtype)
    for bias in (None, bd):
        want = ref if bias is None else ref + b
        for act in (ACT_NONE, ACT_LRELU):
            y = filled((c.B, c.H, c.W, c.Cout), c.dtype)
            assert conv(L, xd, pk, bias, None, y, c, act, D.SLOPE) == 0
            assert_same(y, want if act == ACT_NONE else D.lrelu(want, D.SLOPE), f"{D.case_id(c)} bias={bias is not None} act={act}")
    g, wl, save, gref = D.dgrad_reference(shape)
    pk1 = pack(L, wl, 1, c.dtype)
    y = filled((c.B, c.H, c.W, c.Cout), c.dtype)
    assert conv(L, dev(g, c.dtype), pk1, None, dev(save, c.dtype), y, c, ACT_NONE, D.SLOPE) == 0
    assert_same(y, gref, f"{D.case_id(c)} act_save")


@pytest.mark.parametrize("c", D.FWD_BASE, ids=D.case_id)
def test_forward_impulses(L, c):
    """One non-zero input element - at the corners and on both sides of every position-tile and channel-chunk boundary of the arm -
    must return the matching weight taps around it and exact zeros elsewhere."""
    arm = D.fwd_arm(*D.shape_of(c), c.dtype)
    _, w, _ = D.fwd_inputs(c)
    pk = pack(L, w, 0, c.dtype)
    xd = torch.zeros(c.B, c.H, c.W, c.Cin, dtype=TORCH_DT[c.dtype], device="cuda")
    for pt in D.fwd_impulses(c, arm):
        xd[pt] = 1.0
        y = filled((c.B, c.H, c.W, c.Cout), c.dtype)
        assert conv(L, xd, pk, None, None, y, c, ACT_NONE, 1.0) == 0
        b, h, wq, _ = pt
        want = D.fwd_impulse_expected(c, w, pt)
        lo, hi = max(0, wq - (c.kw // 2) * c.dil), min(c.W, wq + (c.kw // 2) * c.dil + 1)
        assert_same(y[b, :, lo:hi], want[b, :, lo:hi], f"{D.case_id(c)} impulse at {pt}: the window")
        assert int(torch.count_nonzero(y)) == int(torch.count_nonzero(want)) and not bool(torch.isnan(y).any()), (D.case_id(c), pt)
        xd[pt] = 0.0


# =============================================================================================== weight gradient, bit-exact
def _wgrad_call(L, name, xd, gd, gw, gb, ws, c):
    return call(getattr(L, name), xd, gd, gw, gb, ws, c.B, c.H, c.W, c.Cin, c.Cout, c.kh, c.kw, c.dil, c.dtype)


@pytest.mark.parametrize("c", D.WGRAD_CASES, ids=D.case_id)
def test_weight_gradient_exact(L, c):
    """gw and gb of dense sign tensors equal fp64 bit for bit through both entry points; the _pz workspace is zero again on exit and a
    second call on it returns the same bits."""
    x, g, gw_ref, gb_ref = D.wgrad_reference(D.shape_of(c))
    xd, gd = dev(x, c.dtype), dev(g, c.dtype)
    n = c.Cout * c.Cin * c.kh * c.kw
    ws = filled((n + c.Cout,), torch.float32, 7.0)                      # mv_dconv_wgrad_cl clears its own scratch
    gw, gb = filled(gw_ref.shape, torch.float32), filled((c.Cout,), torch.float32)
    assert _wgrad_call(L, "mv_dconv_wgrad_cl", xd, gd, gw, gb, ws, c) == 0
    assert_same(gw, gw_ref, f"{D.case_id(c)} gw")
    assert_same(gb, gb_ref, f"{D.case_id(c)} gb")
    gw2 = filled(gw_ref.shape, torch.float32)
    assert _wgrad_call(L, "mv_dconv_wgrad_cl", xd, gd, gw2, ws[n:], ws, c) == 0    # bias sums right behind the workspace: one fill
    assert_same(gw2, gw_ref, f"{D.case_id(c)} gw (gb behind the workspace)")
    assert_same(ws[n:], gb_ref, f"{D.case_id(c)} gb behind the workspace")
    wz = torch.zeros(n + c.Cout, dtype=torch.float32, device="cuda")
    for nth in (1, 2):
        gw, gb = filled(gw_ref.shape, torch.float32), filled((c.Cout,), torch.float32)
        assert _wgrad_call(L, "mv_dconv_wgrad_cl_pz", xd, gd, gw, gb, wz, c) == 0
        assert_same(gw, gw_ref, f"{D.case_id(c)} _pz call {nth} gw")
        assert_same(gb, gb_ref, f"{D.case_id(c)} _pz call {nth} gb")
        assert int(torch.count_nonzero(wz)) == 0, f"{D.case_id(c)} _pz call {nth}: workspace not zero on exit"


# impulses: the first row of every arm and every row whose workgroups own more than one chunk
_seen = set()
WG_IMPULSE_CASES = [c for c in D.WGRAD_CASES if D.wgrad_split(c)[0] > 1 or not (c.arm in _seen or _seen.add(c.arm))]


@pytest.mark.parametrize("c", WG_IMPULSE_CASES, ids=D.case_id)
def test_weight_gradient_impulses(L, c):
    """One non-zero output gradient - at the corners, on both sides of the position tile and of the first workgroup boundary - must
    return the shifted x row in gw[o] and nothing else; gb is that one element."""
    arm = D.wgrad_arm(*D.shape_of(c), c.dtype)
    x, _ = D.wgrad_inputs(c)
    xd = dev(x, c.dtype)
    gd = torch.zeros(c.B, c.H, c.W, c.Cout, dtype=TORCH_DT[c.dtype], device="cuda")
    n = c.Cout * c.Cin * c.kh * c.kw
    wz = torch.zeros(n + c.Cout, dtype=torch.float32, device="cuda")
    for pt in D.wgrad_impulses(c, arm):
        gd[pt] = 1.0
        gw, gb = filled((c.Cout, c.Cin, c.kh, c.kw), torch.float32), filled((c.Cout,), torch.float32)
        assert _wgrad_call(L, "mv_dconv_wgrad_cl_pz", xd, gd, gw, gb, wz, c) == 0
        assert_same(gw, D.wgrad_impulse_expected(c, x, pt), f"{D.case_id(c)} impulse at {pt} gw")
        want_b = torch.zeros(c.Cout, dtype=torch.float64)
        want_b[pt[3]] = 1.0
        assert_same(gb, want_b, f"{D.case_id(c)} impulse at {pt} gb")
        gd[pt] = 0.0


# =============================================================================================== packs
class _Desc(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("Cout", ctypes.c_int), ("Cin", ctypes.c_int), ("kh", ctypes.c_int),
                ("kw", ctypes.c_int), ("flip", ctypes.c_int), ("dtype", ctypes.c_int)]


def test_multi_pack_equals_single_packs(L):
    """One launch over a table that mixes bf16, fp16 and split-fp32 images, flip 0 and 1: byte-equal to mv_dconv_pack of each."""
    table = [(32, 32, 3, 3, 0, MV_BF16), (64, 32, 1, 15, 1, MV_F16), (16, 64, 3, 3, 0, MV_F32), (128, 96, 1, 3, 1, MV_F32),
             (96, 32, 1, 1, 1, MV_BF16), (256, 32, 5, 1, 0, MV_F16), (48, 160, 1, 7, 0, MV_BF16)]
    assert ctypes.sizeof(_Desc) == 40
    torch.manual_seed(3)
    srcs = [torch.randn(co, ci, kh, kw).cuda().contiguous() for co, ci, kh, kw, _, _ in table]
    sizes = [L.mv_dconv_packed_bytes(co, ci, kh, kw, dt) for co, ci, kh, kw, _, dt in table]
    dsts = [torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda") for n in sizes]
    arr = (_Desc * len(table))(*[_Desc(s.data_ptr(), d.data_ptr(), *row) for s, d, row in zip(srcs, dsts, table)])
    descs = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    assert call(L.mv_dconv_multi_pack, descs, len(table)) == 0
    for s, d, n, (co, ci, kh, kw, flip, dt) in zip(srcs, dsts, sizes, table):
        one = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
        assert call(L.mv_dconv_pack, s, MV_F32, one, co, ci, kh, kw, flip, dt) == 0
        assert torch.equal(d.cpu(), one.cpu()), (co, ci, kh, kw, flip, dt)


@pytest.mark.parametrize("dt", ALL_DT)
@pytest.mark.parametrize("cin,cout,kh,kw", [(20, 60, 3, 3), (60, 20, 1, 15)])
def test_pack_pad_convolution(L, dt, cin, cout, kh, kw):
    """Channel counts padded to the next multiple of 32 (20 -> 32, 60 -> 64): the real output channels equal the unpadded reference,
    the padded ones are exactly 0 - whatever the padded INPUT channels hold, since their weights are zero."""
    cinp, coutp = (cin + 31) // 32 * 32, (cout + 31) // 32 * 32
    c = D.Case("", 2, 2, 131, cinp, coutp, kh, kw, 1, dt)
    x = D.sparse_signs((c.B, c.H, c.W), cin, 51)
    w, b = D.ints((cout, cin, kh, kw), -2, 2, 52), D.ints((cout,), -3, 3, 53)
    ref = D.conv_ref(x, w, b, 1)
    xp = torch.cat([x, D.ints((c.B, c.H, c.W, cinp - cin), -1, 1, 54)], -1)
    bp = torch.cat([b, torch.zeros(coutp - cout, dtype=torch.float64)])
    pk = pack(L, w, 0, dt, coutp, cinp)
    y = filled((c.B, c.H, c.W, coutp), dt)
    assert conv(L, dev(xp, dt), pk, dev(bp, dt), None, y, c, ACT_NONE, 1.0) == 0
    assert_same(y[..., :cout], ref, "real channels")
    assert_same(y[..., cout:], torch.zeros(c.B, c.H, c.W, coutp - cout), "padded channels")


# =============================================================================================== the 256 -> 1 head
HEAD_GEOM = [(3, 3, 2, 1, 37), (3, 3, 1, 3, 130), (3, 3, 3, 11, 17), (1, 15, 3, 1, 131), (1, 15, 1, 3, 5), (1, 15, 2, 11, 33)]   # kh kw B H W


def _head_pack(L, w, kh, kw, dt):
    buf = torch.empty(L.mv_dhead_packed_bytes(256, dt), dtype=torch.uint8, device="cuda")
    wf = w.float().cuda().contiguous()
    assert call(L.mv_dhead_pack, wf, MV_F32, buf, 256, kh, kw, dt) == 0
    return buf


@pytest.mark.parametrize("dt", DT16)
def test_head_pack_from_16_bit_parameters(L, dt):
    """Integer weights held as bf16 / fp16 parameters pack to the same bytes as their fp32 master."""
    w = D.ints((1, 256, 1, 15), -1, 1, 62)
    want = _head_pack(L, w, 1, 15, dt)
    for pdt in DT16:
        buf = torch.empty_like(want)
        assert call(L.mv_dhead_pack, dev(w, pdt), pdt, buf, 256, 1, 15, dt) == 0
        assert torch.equal(buf.cpu(), want.cpu()), pdt


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("kh,kw,B,H,W", HEAD_GEOM)
def test_head_forward_and_sum(L, dt, kh, kw, B, H, W):
    x = D.sparse_signs((B, H, W), 256, 61)
    w, b = D.ints((1, 256, kh, kw), -1, 1, 62), D.ints((1,), -3, 3, 63)
    pk = _head_pack(L, w, kh, kw, dt)
    ws = filled((L.mv_dhead_workspace_bytes(B, H, W) // 4,), torch.float32)
    for bias, want in ((None, D.head_ref(x, w, None)), (b, D.head_ref(x, w, b))):
        y = filled((B, H, W), dt)
        assert call(L.mv_dhead_fwd, dev(x, dt), pk, None if bias is None else dev(bias, dt), ws, y, B, H, W, 256, kh, kw, dt) == 0
        assert_same(y, want, f"head forward {kh}x{kw} bias={bias is not None}")
    # mv_dhead_sum alone, on per-tap partial sums of its own
    z = D.ints((16, B * H * W), -8, 8, 64)
    y = filled((B, H, W), dt)
    assert call(L.mv_dhead_sum, z.float().cuda(), dev(b, dt), y, B, H, W, kh, kw, dt) == 0
    assert_same(y, float(b[0]) + D.tap_shift_sum(z.view(16, B, H, W), kh, kw), f"head sum {kh}x{kw}")


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("kh,kw,B,H,W", HEAD_GEOM)
def test_head_data_gradient(L, dt, kh, kw, B, H, W):
    gy, w = D.ints((B, H, W), -1, 1, 65), D.ints((1, 256, kh, kw), -1, 1, 62)
    save = D.signed_zero_save((B, H, W, 256), 66)
    gx = filled((B, H, W, 256), dt)
    assert call(L.mv_dhead_dgrad, dev(gy, dt), _head_pack(L, w, kh, kw, dt), dev(save, dt), gx, B, H, W, 256, kh, kw, D.SLOPE, dt) == 0
    assert_same(gx, D.head_dgrad_ref(gy, w, save, D.SLOPE), f"head dgrad {kh}x{kw}")


@pytest.mark.parametrize("dt", ALL_DT)
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("kh,kw,B,H,W", [(3, 3, 2, 3, 130), (1, 15, 3, 1, 600), (1, 15, 1, 11, 5)])
def test_head_weight_gradient(L, dt, aligned, kh, kw, B, H, W):
    """Both routes: 16-byte aligned 16-bit x takes dtap_wgrad_kernel, an x one element off (and fp32) dhead_wgrad_kernel."""
    gy, x = D.ints((B, H, W), -1, 1, 67), D.ints((B, H, W, 256), -1, 1, 68)
    gw_ref, gb_ref = D.head_wgrad_ref(gy, x, kh, kw)
    xd = dev(x, dt)
    if not aligned:
        xd = misaligned(xd)
    gw, gb = filled((kh * kw, 256), torch.float32), filled((1,), torch.float32)
    assert call(L.mv_dhead_wgrad, dev(gy, dt), xd, gw, gb, B, H, W, 256, kh, kw, dt) == 0
    assert_same(gw, gw_ref, "head gw")
    assert_same(gb, gb_ref, "head gb")


# =============================================================================================== the 1 -> C1 first layer
FIRST_GEOM = [(3, 3, 32, 2, 2, 1023), (3, 3, 32, 1, 3, 1024), (3, 3, 32, 1, 2, 1025), (1, 15, 32, 2, 1, 1023), (1, 15, 32, 1, 1, 1024),
              (1, 15, 32, 3, 1, 1025), (1, 15, 32, 1, 11, 5), (5, 1, 12, 2, 11, 37), (5, 1, 32, 1, 1, 300)]      # kh kw C1 B H W


@pytest.mark.parametrize("dt", ALL_DT)
@pytest.mark.parametrize("kh,kw,C1,B,H,W", FIRST_GEOM)
def test_first_layer_forward(L, dt, kh, kw, C1, B, H, W):
    """Tiled form (16-bit, C1 = 32, 3x3 and 1x15, around the 1024-position tile) and plain form (5x1, C1 = 12, fp32 storage)."""
    x0, w, b = D.ints((B, H, W), -2, 2, 71), D.ints((C1, 1, kh, kw), -2, 2, 72), D.ints((C1,), -3, 3, 73)
    for bias in (None, b):
        y = filled((B, H, W, C1), dt)
        assert call(L.mv_dfirst_fwd_cl, dev(x0, dt), dev(w, dt), None if bias is None else dev(bias, dt), y, B, H, W, C1, kh, kw,
                                  D.SLOPE, dt) == 0
        assert_same(y, D.first_ref(x0, w, bias, D.SLOPE), f"first forward {kh}x{kw} C1={C1} bias={bias is not None}")


@pytest.mark.parametrize("dt", ALL_DT)
@pytest.mark.parametrize("mfma", [True, False], ids=["mfma", "scalar"])
@pytest.mark.parametrize("kh,kw,B,H,W", [(3, 3, 2, 3, 130), (1, 15, 3, 1, 131), (1, 15, 1, 11, 5), (3, 3, 1, 1, 1)])
def test_first_layer_data_gradient(L, dt, mfma, kh, kw, B, H, W):
    """gx0 through the tap-row MFMA route (a workspace is given; 16-bit storage) and the scalar route (workspace = NULL)."""
    g1, w = D.sparse_signs((B, H, W), 32, 74), D.ints((32, 1, kh, kw), -1, 1, 75)
    ws = filled((L.mv_dfirst_dgrad_workspace_bytes(B, H, W) // 4,), torch.float32) if mfma else None
    gx0 = filled((B, H, W), dt)
    assert call(L.mv_dfirst_dgrad_cl, dev(g1, dt), dev(w, dt), gx0, ws, B, H, W, 32, kh, kw, dt) == 0
    assert_same(gx0, D.first_dgrad_ref(g1, w), f"first dgrad {kh}x{kw}")


@pytest.mark.parametrize("dt", ALL_DT)
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("kh,kw,C1,B,H,W", [(3, 3, 32, 2, 3, 130), (1, 15, 32, 3, 1, 1100), (1, 15, 64, 1, 11, 5), (5, 1, 16, 2, 7, 33)])
def test_first_layer_weight_gradient(L, dt, aligned, kh, kw, C1, B, H, W):
    """Both routes: aligned 16-bit g1 with a 3x3 / 1x15 kernel takes dtap_wgrad_kernel; misaligned g1, fp32 and 5x1 dfirst_wgrad_kernel."""
    g1, x0 = D.ints((B, H, W, C1), -1, 1, 76), D.ints((B, H, W), -2, 2, 77)
    gw_ref, gb_ref = D.first_wgrad_ref(g1, x0, kh, kw)
    gd = dev(g1, dt)
    if not aligned:
        gd = misaligned(gd)
    gw, gb = filled((C1, kh * kw), torch.float32), filled((C1,), torch.float32)
    assert call(L.mv_dfirst_wgrad_cl, gd, dev(x0, dt), gw, gb, B, H, W, C1, kh, kw, dt) == 0
    assert_same(gw, gw_ref, "first gw")
    assert_same(gb, gb_ref, "first gb")


# =============================================================================================== small helpers of the stacks
@pytest.mark.parametrize("dt", ALL_DT)
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("kh,kw,B,H,W", [(3, 3, 2, 3, 37), (1, 15, 2, 1, 131), (1, 15, 1, 2, 5), (3, 3, 1, 1, 1), (5, 3, 1, 4, 9)])
def test_tap_matrix(L, dt, flip, kh, kw, B, H, W):
    sc = D.ints((B, H, W), -3, 3, 81)
    out = filled((B, H, W, 16), dt)
    assert call(L.mv_tap_matrix, dev(sc, dt), out, B, H, W, kh, kw, flip, dt) == 0
    assert_same(out, D.tap_matrix_ref(sc, kh, kw, flip), f"tap matrix {kh}x{kw} flip {flip}")     # columns >= kh*kw are exact zeros


@pytest.mark.parametrize("dt", ALL_DT)
@pytest.mark.parametrize("C", [8, 64, 256])
@pytest.mark.parametrize("rows", [1, 2047, 2049])
def test_colsum(L, dt, C, rows):
    x = D.ints((rows, C), -1, 1, 82)
    out = filled((C,), torch.float32)
    assert call(L.mv_colsum_cl, dev(x, dt), out, rows, C, dt) == 0
    assert_same(out, x.sum(0), f"colsum rows={rows} C={C}")


@pytest.mark.parametrize("dt", ALL_DT)
@pytest.mark.parametrize("C,ch", [(16, 0), (16, 15), (256, 0), (256, 255), (1, 0)])
def test_take_and_put_channel(L, dt, C, ch):
    rows = 1031
    x, g = D.ints((rows, C), -100, 100, 83), D.ints((rows,), -100, 100, 84)
    out = filled((rows,), dt)
    assert call(L.mv_take_channel, dev(x, dt), out, rows, C, ch, dt) == 0
    assert_same(out, x[:, ch], "take_channel")
    y = filled((rows, C), dt)
    assert call(L.mv_put_channel, dev(g, dt), y, rows, C, ch, dt) == 0
    want = torch.zeros(rows, C, dtype=torch.float64)
    want[:, ch] = g
    assert_same(y, want, "put_channel")


# =============================================================================================== real values, every element bounded
_REAL = {}
for _c in D.FWD_BASE:
    if _c.dtype != MV_F32:
        _REAL.setdefault(_c.arm, _c)


@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("c", list(_REAL.values()), ids=D.case_id)
def test_forward_real_values_elementwise(L, c, scale):
    """x ~ N(0,1) * scale, w ~ N(0, 1/(Cin kh kw)), bias ~ 0.1 N(0,1), rounded to the storage type; LeakyReLU slopes 0.1 and 0.0.
    Every element:  |y - act(ref)| <= u |act(ref)| + n 2^-23 A + 2^-24,  u = 2^-8 (bf16) / 2^-11 (fp16): half an ulp of the stored
    significand plus twice the worst-case fp32 summation error (disc_cases.real_bound); none of it is measured.  A kernel that rounds
    twice, keeps a partial sum in 16 bits or adds the bias after the store breaks it at scale 30."""
    x, w, b = D.real_inputs(c, scale, TORCH_DT[c.dtype])
    ref, slack = D.real_bound(x, w, b, c.dil)
    u = 2.0 ** -8 if c.dtype == MV_BF16 else 2.0 ** -11
    xd, bd, pk = dev(x, c.dtype), dev(b, c.dtype), pack(L, w, 0, c.dtype)
    for slope in (0.1, 0.0):
        s32 = float(np.float32(slope))                      # the value the C ABI receives
        y = filled((c.B, c.H, c.W, c.Cout), c.dtype)
        assert conv(L, xd, pk, bd, None, y, c, ACT_LRELU, s32) == 0
        want = D.lrelu(ref, s32)
        err, bound = (y.double().cpu() - want).abs(), u * want.abs() + slack
        ratio = float((err / bound).max())
        print(f"[disc-real] {D.case_id(c)} scale {scale} slope {slope}: worst error / bound {ratio:.3f}")
        assert bool((err <= bound).all()), (D.case_id(c), scale, slope, ratio, int((err > bound).sum()))


# =============================================================================================== refusals (nothing is launched)
SENT = -1024.0                      # exact in bf16, fp16 and fp32


def test_forward_refusals_leave_the_output_alone(L):
    for dt in DT16:
        ok = D.Case("", 1, 2, 40, 32, 32, 3, 3, 1, dt)
        x = filled((1, 2, 40, 64), dt, 1.0)
        pk = torch.zeros(64 * 64 * 9 * 4, dtype=torch.uint8, device="cuda")
        y = filled((1, 2, 40, 64), dt, SENT)
        bad = [(ok._replace(Cin=48), x, "Cin % 32"), (ok._replace(kw=4), x, "even kw"), (ok._replace(kw=3, dil=65), x, "(kw-1)*dil > 128"),
               (ok._replace(kh=1, kw=15, dil=10), x, "(kw-1)*dil > 128"), (ok, misaligned(x), "misaligned x")]
        for c, xx, why in bad:
            assert conv(L, xx, pk, None, None, y, c, ACT_NONE, 1.0) == D.MV_ERR_ARG, why
        hp = torch.zeros(L.mv_dhead_packed_bytes(256, dt), dtype=torch.uint8, device="cuda")
        hws = filled((16 * 80,), torch.float32, SENT)
        rc = call(L.mv_dconv_cl_fwd_head, x, pk, None, y, hp, hws, 3, 3, 1, 2, 40, 32, 128, 3, 3, ACT_LRELU, 0.1, dt)
        assert rc == D.MV_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert bool((y == SENT).all()) and bool((hws == SENT).all())


def test_weight_gradient_refusals_leave_the_outputs_alone(L):
    cases = [(MV_BF16, 3, 3, 2, "16-bit 3x3 with dil_w = 2"), (MV_F16, 3, 3, 2, "16-bit 3x3 with dil_w = 2"), (MV_BF16, 1, 15, 5, "halo 70 > 64"),
             (MV_F16, 1, 3, 33, "halo 66 > 64"), (MV_BF16, 1, 9, 1, "1x9"), (MV_F16, 1, 9, 1, "1x9"), (MV_F32, 1, 7, 1, "fp32 1x7"),
             (MV_F32, 3, 3, 2, "fp32 dilated")]
    for entry in ("mv_dconv_wgrad_cl", "mv_dconv_wgrad_cl_pz"):
        for dt, kh, kw, dil, why in cases:
            c = D.Case("", 1, 2, 40, 64, 64, kh, kw, dil, dt)
            x = filled((1, 2, 40, 64), dt, 1.0)
            n = 64 * 64 * kh * kw
            gw, gb, ws = filled((n,), torch.float32, SENT), filled((64,), torch.float32, SENT), filled((n + 64,), torch.float32, SENT)
            assert _wgrad_call(L, entry, x, x, gw, gb, ws, c) == D.MV_ERR_UNSUPPORTED, (entry, why)
            torch.cuda.synchronize()
            assert bool((gw == SENT).all()) and bool((gb == SENT).all()) and bool((ws == SENT).all()), (entry, why)


def test_fp32_weight_gradient_refusal_is_decided_before_any_fill(L):
    """fp32 3x3 with dil_w = 2 at the smallest shape: MV_ERR_UNSUPPORTED, with workspace and gb untouched - the plan is asked before
    the zero fills for fp32 as for 16-bit storage."""
    c = D.Case("", 1, 1, 8, 8, 8, 3, 3, 2, MV_F32)
    x = filled((1, 1, 8, 8), MV_F32, 1.0)
    n = 8 * 8 * 9
    gw, gb, ws = filled((n,), torch.float32, SENT), filled((8,), torch.float32, SENT), filled((n + 8,), torch.float32, SENT)
    assert _wgrad_call(L, "mv_dconv_wgrad_cl", x, x, gw, gb, ws, c) == D.MV_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((gw == SENT).all()) and bool((gb == SENT).all()) and bool((ws == SENT).all())


def test_head_pack_refusals(L):
    w = torch.zeros(512 * 16, device="cuda")
    out = filled((L.mv_dhead_packed_bytes(512, MV_F32),), torch.uint8, 0x5A)
    assert call(L.mv_dhead_pack, w, MV_F32, out, 256, 3, 3, MV_F32) == D.MV_ERR_UNSUPPORTED       # 16-bit storage only
    for dt in DT16:
        assert call(L.mv_dhead_pack, w, MV_F32, out, 128, 3, 3, dt) == D.MV_ERR_ARG               # C != 256
        assert call(L.mv_dhead_pack, w, MV_F32, out, 512, 3, 3, dt) == D.MV_ERR_ARG
        assert call(L.mv_dhead_pack, w, MV_F32, out, 256, 3, 7, dt) == D.MV_ERR_ARG               # more than 16 taps
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())
