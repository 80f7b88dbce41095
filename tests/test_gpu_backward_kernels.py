"""The generator's backward kernels, one entry point at a time through the raw C ABI, against float64 references on the CPU
(tests/backward_cases.py): csrc/backward.hip, mv_grc_fold_bwd / mv_loss_fwd_bwd / mv_scale(_to) of csrc/train.hip, and the per-sample
ODConvTranspose bank gradient of csrc/disc_fused.hip with its two layout maps.

Operands are small integers and dyadic scalars, so wherever an operation is a sum of products the fp32 result is exact in any order
and the tests ask for bit equality (tests/test_host_backward_cases.py proves that for every row); where a division by a non-power-of-two
or a 16-bit store of a many-bit value makes that impossible, every element is bounded by u_out |ref| + k 2^-24 sum|terms| with k counted
at the case.  Nothing is compared by a norm over a tensor.  Outputs and workspaces start as NaN: a call that must zero-fill does, a
direct store covers every element, a refusal writes nothing; the `+=` buffers (galpha, loss_acc) start from non-zero integers."""
import ctypes
import itertools

import pytest
import torch

import backward_cases as C
from backward_cases import MV_BF16, MV_F16, MV_F32, TORCH_DT

pytestmark = pytest.mark.gpu

ALL_DT = (MV_BF16, MV_F16, MV_F32)
DT16 = (MV_BF16, MV_F16)
dtid = C.DT_NAME.get
f = ctypes.c_float


@pytest.fixture(scope="module")
def L():
    from hifigan_modified import _native
    return _native.lib()


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_error():
    """A kernel fault poisons the context: end the session there instead of sending the remaining tests at the device."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error, stopping: {e}", returncode=3)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(fn, *args):
    """fn(*args, stream) with every tensor passed as its device address."""
    return fn(*[_p(a) if isinstance(a, torch.Tensor) else a for a in args], _s())


def dev(t, dt):
    return t.to(TORCH_DT[dt] if isinstance(dt, int) else dt).cuda().contiguous()


def f32(t):
    return t.float().cuda().contiguous()


def nans(shape, dt=torch.float32):
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    return torch.full(shape, float("nan"), dtype=TORCH_DT[dt] if isinstance(dt, int) else dt, device="cuda")


def offset_view(t, off):
    """The same values at an address `off` elements past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device="cuda")
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
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


def check(got, out, dt, what):
    """An Out of backward_cases: bit equality (k == 0) or the per-element bound; dt is the type `got` was written in."""
    if out.k == 0:
        return assert_same(got.view(out.ref.shape), out.ref, what)
    got = got.detach().double().cpu().view(out.ref.shape)
    tol = C.tolerance(out, dt)
    bad = ~((got - out.ref).abs() <= tol)
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements outside the bound; first {i}: got {got[i].item()} "
                             f"want {out.ref[i].item()} bound {tol[i].item()}")


def untouched(*ts):
    return all(bool(torch.isnan(t.float()).all()) for t in ts)


# =============================================================================================== mv_conv1d_wgrad
def _wgrad(L, c, dt, r, x=None, gy=None, gw=None, ws=None, ga=None):
    """One call on a row's inputs; x / gy may be strided views, gw / ws given buffers.  Returns (rc, gw, galpha, workspace)."""
    x = dev(r["x"], dt) if x is None else x
    gy = dev(r["gy"], dt) if gy is None else gy
    nelem = c.Cout * c.Cin * c.ks
    if c.nbanks == 1:
        gw = nans((c.Cout, c.Cin, c.ks)) if gw is None else gw
        rc = call(L.mv_conv1d_wgrad, x, gy, None, None, gw, None, None, c.B, c.Cin, r["Tin"], c.Cout, c.Tout, c.ks, c.stride, c.pad,
                  c.dil, 1, x.stride(0), x.stride(1), gy.stride(0), gy.stride(1), dt)
        return rc, gw, None, None
    assert L.mv_conv1d_wgrad_workspace_bytes(c.B, c.Cin, c.Cout, c.ks, c.nbanks) == 4 * c.B * nelem
    gw = nans((c.nbanks, c.Cout, c.Cin, c.ks)) if gw is None else gw
    ws = nans(c.B * nelem) if ws is None else ws
    ga = f32(r["galpha0"]) if ga is None else ga
    rc = call(L.mv_conv1d_wgrad, x, gy, dev(r["w"], dt), f32(r["alpha"]), gw, ga, ws, c.B, c.Cin, r["Tin"], c.Cout, c.Tout, c.ks, c.stride,
              c.pad, c.dil, c.nbanks, x.stride(0), x.stride(1), gy.stride(0), gy.stride(1), dt)
    return rc, gw, ga, ws


@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("c", C.WG_CASES, ids=lambda c: c.name)
def test_conv1d_wgrad_exact(L, c, dt):
    """gw (and galpha, added to its pre-filled integers) equal fp64 bit for bit; in per-sample mode the workspace holds every
    sample's tile exactly - zero-filled and added to when the time axis is split, stored once (over NaN) when it is not."""
    r = C.wg_reference(c)
    rc, gw, ga, ws = _wgrad(L, c, dt, r)
    assert rc == 0
    check(gw, r["gw"], MV_F32, f"{c.name} gw")
    if c.nbanks > 1:
        check(ga, r["galpha"], MV_F32, f"{c.name} galpha")
        check(ws, r["tiles"], MV_F32, f"{c.name} per-sample tiles")


@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
def test_conv1d_wgrad_misaligned_gw_takes_generic_reduce(L, dt):
    """nbanks = 4, nelem % 4 == 0, gw one float past a 16-byte boundary: the generic reduction, same bits."""
    c = next(c for c in C.WG_CASES if c.name == "k4-reduce4")
    r = C.wg_reference(c)
    buf = nans(c.nbanks * c.Cout * c.Cin * c.ks + 8)
    gw = buf[1:1 + c.nbanks * c.Cout * c.Cin * c.ks].view(c.nbanks, c.Cout, c.Cin, c.ks)
    assert gw.data_ptr() % 16 == 4
    rc, gw, ga, _ = _wgrad(L, c, dt, r, gw=gw)
    assert rc == 0
    check(gw, r["gw"], MV_F32, "gw at +4 bytes")
    check(ga, r["galpha"], MV_F32, "galpha")
    assert untouched(buf[:1], buf[1 + gw.numel():])


@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("name", ("pad>halo", "t200-split4-k4", "s2-d3-k7"))
def test_conv1d_wgrad_strided_operands(L, name, dt):
    """x and gy as time windows and channel slices of wider NaN-filled buffers: only the window may be read."""
    c = next(c for c in C.WG_CASES if c.name == name)
    r = C.wg_reference(c)
    xb, gb = nans((c.B, c.Cin + 3, r["Tin"] + 5), dt), nans((c.B, c.Cout + 2, c.Tout + 7), dt)
    x, gy = xb[:, 2:2 + c.Cin, 3:3 + r["Tin"]], gb[:, 1:1 + c.Cout, 4:4 + c.Tout]
    x.copy_(dev(r["x"], dt))
    gy.copy_(dev(r["gy"], dt))
    rc, gw, ga, _ = _wgrad(L, c, dt, r, x=x, gy=gy)
    assert rc == 0
    check(gw, r["gw"], MV_F32, f"{name} gw")
    if ga is not None:
        check(ga, r["galpha"], MV_F32, f"{name} galpha")


@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("case", ((0, 3, 127, 4), (2, 3, 127, 5)), ids=("k4s2", "k6s3-opad1"))
def test_conv1d_wgrad_swapped_roles_is_the_transposed_conv_gradient(L, case, dt):
    """functional.py's call for ODConvTranspose1d: x := the output gradient, gy := the layer input, Cin := Cout, ...; the result is
    the gradient of F.conv_transpose1d's [Cin][Cout][ks] banks."""
    Cin, Cout, ks, stride = C.ODT_SHAPES[case[0]]
    _, B, Tin, K = case
    r = C.odt_reference(*case)
    g, x = dev(r["g"], dt), dev(r["x_cl"].transpose(1, 2), dt)
    n = Cin * Cout * ks
    gw, ws, ga = nans((K, Cin, Cout, ks)), nans(B * n), f32(r["galpha0"])
    rc = call(L.mv_conv1d_wgrad, g, x, dev(r["w"], dt), f32(r["alpha"]), gw, ga, ws, B, Cout, r["Tout"], Cin, Tin, ks, stride, r["pad"], 1, K,
              g.stride(0), g.stride(1), x.stride(0), x.stride(1), dt)
    assert rc == 0
    check(gw, r["gw"], MV_F32, "gw")
    check(ga, r["galpha"], MV_F32, "galpha")


@pytest.mark.parametrize("name,shape,code", C.WG_REFUSED, ids=[r[0] for r in C.WG_REFUSED])
def test_conv1d_wgrad_refusals_write_nothing(L, name, shape, code):
    B, Cin, Cout, Tout, ks, stride, dil, nb = shape
    x, gy, w = torch.zeros(64, device="cuda"), torch.zeros(64, device="cuda"), torch.zeros(64, device="cuda")
    gw, ws, ga, al = nans(64), nans(64), nans(64), torch.zeros(64, device="cuda")
    rc = call(L.mv_conv1d_wgrad, x, gy, w, al, gw, ga, ws, B, Cin, 4, Cout, Tout, ks, stride, 0, dil, nb, 4, 4, 4, 4, MV_F32)
    torch.cuda.synchronize()
    assert rc == code and untouched(gw, ws, ga)


@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("a", C.REDUCE_CASES, ids=str)
def test_odconv_wgrad_reduce_alone(L, a, dt):
    B, K, n = a
    r = C.reduce_reference(*a)
    gw, ga = nans((K, n)), f32(r["galpha0"])
    assert call(L.mv_odconv_wgrad_reduce, f32(r["tiles"]), dev(r["w"], dt), f32(r["alpha"]), gw, ga, B, K, n, dt) == 0
    check(gw, r["gw"], MV_F32, f"reduce {a} gw")
    check(ga, r["galpha"], MV_F32, f"reduce {a} galpha")


# =============================================================================================== mv_bias_grad
@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("a", C.BIAS_CASES, ids=str)
def test_bias_grad(L, a, dt):
    """Dense and as a window of a wider buffer; galpha is added to only with K > 1 and a bias."""
    B, Cc, T, K, has_bias = a
    r = C.bias_reference(*a)
    wide = nans((B, Cc + 2, T + 9), dt)
    win = wide[:, 1:1 + Cc, 5:5 + T]
    win.copy_(dev(r["gy"], dt))
    for gy in (dev(r["gy"], dt), win):
        ws, gb, ga = nans(B * Cc), nans((K, Cc)), f32(r["galpha0"])
        rc = call(L.mv_bias_grad, gy, f32(r["alpha"]) if K > 1 else None, dev(r["bias"], dt) if has_bias else None, ws, gb, ga, B, Cc, T, K,
                  gy.stride(0), gy.stride(1), dt)
        assert rc == 0
        check(ws, r["rowsum"], MV_F32, f"bias {a} row sums")
        check(gb, r["gbias"], MV_F32, f"bias {a} gbias")
        check(ga, r["galpha"], MV_F32, f"bias {a} galpha")


# =============================================================================================== attention chain
@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("a", C.ATTN_CASES, ids=str)
def test_odconv_attn_bwd(L, a, dt):
    B, Cc, K, T = a
    r = C.attn_reference(*a)
    gwa, gba, gm = nans((K, Cc)), nans(K), nans((B, Cc))
    rc = call(L.mv_odconv_attn_bwd, f32(r["alpha"]), f32(r["galpha"]), f32(r["pooled"]), dev(r["wa"], dt), gwa, gba, gm, B, Cc, T, K, dt)
    assert rc == 0
    for got, n in ((gwa, "gwa"), (gba, "gba"), (gm, "gm")):
        check(got, r[n], MV_F32, f"attn {a} {n}")


def test_odconv_attn_bwd_refuses_more_than_64k_of_lds(L):
    B, K = 4097, 4                                             # 65552 bytes
    z = torch.zeros(B * K, device="cuda")
    gwa, gba, gm = nans((K, 1)), nans(K), nans((B, 1))
    assert call(L.mv_odconv_attn_bwd, z, z, z, z, gwa, gba, gm, B, 1, 8, K, MV_F32) == C.MV_ERR_ARG
    torch.cuda.synchronize()
    assert untouched(gwa, gba, gm)


@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("rows,T", C.ROWCONST_CASES, ids=str)
def test_add_rowconst(L, rows, T, dt):
    x, v = C.ints((rows, T), 45), C.ints((rows,), 46, lo=-9, hi=9)
    xd = dev(x, dt)
    assert call(L.mv_add_rowconst, xd, f32(v), rows, T, dt) == 0
    assert_same(xd, x + v[:, None], f"rowconst {rows} x {T}")
    assert call(L.mv_add_rowconst, xd, f32(v), 65536, T, dt) == C.MV_ERR_ARG
    assert_same(xd, x + v[:, None], "after the refusal")


# =============================================================================================== mv_groupnorm_bwd
def _gn_call(L, i, sh, dt, act, mask, x=None, gy=None, gw=True, gb=True, dgw=True, dgb=True, maskt=None):
    B, Cc, G, T = sh
    x = dev(i["x"], dt) if x is None else x
    gy = dev(i["gy"], dt) if gy is None else gy
    o = dict(gz=nans((B, Cc, T), dt), ws=nans(2 * B * G + 2 * B * Cc), gx=nans((B, Cc, T), dt), dgw=nans(Cc) if dgw else None,
             dgb=nans(Cc) if dgb else None)
    if mask and maskt is None:
        maskt = i["mask"].cuda()
    o["rc"] = call(L.mv_groupnorm_bwd, x, gy, f32(i["mean"]), f32(i["rstd"]), dev(i["gw"], dt) if gw else None, dev(i["gb"], dt) if gb else None,
                   maskt if mask else None, f(C.MASK_SCALE), act, f(C.SLOPE), o["gz"], o["ws"], o["gx"], o["dgw"], o["dgb"], B, Cc, T, G,
                   x.stride(0), x.stride(1), gy.stride(0), gy.stride(1), dt)
    return o


def _gn_check(o, i, sh, dt, gz_out, tag, use_gw=True, exact_gz=True, T_chain=1):
    """gz against gz_out (an Out, or None when it was checked by the caller); then the later stages from the kernel's own gz."""
    B, Cc, G, T = sh
    if gz_out is not None:
        check(o["gz"], gz_out, dt, f"{tag} gz")
    gz = o["gz"].double().cpu()
    r = C.gn_from_gz(i, gz, G, T_chain, use_gw, exact_gz)
    s12 = o["ws"][:2 * B * G].double().cpu().view(B, G, 2)
    cg = Cc // G
    if exact_gz:
        assert_same(s12[:, :, 0], r["s1"][:, ::cg, 0], f"{tag} s1")
        assert_same(s12[:, :, 1], r["s2"][:, ::cg, 0], f"{tag} s2")
    for n in ("dgw", "dgb"):
        if o[n] is not None:
            check(o[n], r[n], MV_F32, f"{tag} {n}")
    n = cg * T
    if exact_gz and dt == MV_F32 and n & (n - 1) == 0:
        assert_same(o["gx"], r["gx"].ref, f"{tag} gx (n = {n}: exact)")
    else:
        check(o["gx"], r["gx"], dt, f"{tag} gx")
    return r


@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("mask", (False, True), ids=("nomask", "mask"))
@pytest.mark.parametrize("act", (C.ACT_NONE, C.ACT_LRELU), ids=("none", "lrelu"))
@pytest.mark.parametrize("sh", C.GN_SHAPES, ids=str)
def test_groupnorm_bwd_exact(L, sh, act, mask, dt):
    """gz, the (b, g) sums, dgw and dgb are exact at every T (vector and scalar loops, one and two passes); gx is exact in fp32 when
    cg * T is a power of two and inside the derived bound otherwise."""
    i = C.gn_inputs(*sh)
    o = _gn_call(L, i, sh, dt, act, mask)
    assert o["rc"] == 0
    _gn_check(o, i, sh, dt, C.exact(C.gn_gz(i, sh[2], act, mask), unit=0.5, stored=True), f"gn {sh} act{act} mask{mask}")


@pytest.mark.parametrize("dt", (MV_BF16, MV_F32), ids=dtid)
@pytest.mark.parametrize("drop", ("gw", "gb", "dgw", "dgb"))
def test_groupnorm_bwd_null_arguments(L, drop, dt):
    sh = (2, 8, 2, 64)
    i = C.gn_inputs(*sh)
    o = _gn_call(L, i, sh, dt, C.ACT_LRELU, True, **{drop: False})
    assert o["rc"] == 0
    gz = C.gn_gz(i, 2, C.ACT_LRELU, True, use_gw=drop != "gw", use_gb=drop != "gb")
    _gn_check(o, i, sh, dt, C.exact(gz, unit=0.5, stored=True), f"gn without {drop}", use_gw=drop != "gw")


# d act/dz of SiLU and tanh go through __expf, a hardware reciprocal and tanhf: the one measured number of this file.
# |gz - gy mask_scale act'(z)| <= DACT_REL * |gy mask_scale| in fp32; a 16-bit gz adds one rounding of the stored value.
DACT_REL = {C.ACT_SILU: 4 * 3.54e-7, C.ACT_TANH: 4 * 5.83e-8}


@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("act", (C.ACT_SILU, C.ACT_TANH), ids=("silu", "tanh"))
@pytest.mark.parametrize("sh", C.GN_SHAPES[:4], ids=str)
def test_groupnorm_bwd_silu_tanh(L, sh, act, dt):
    """gz element by element against fp64.  fp32 bound = 4 x the largest error measured on an MI355X over these four shapes, relative
    to |gy mask_scale|:   SiLU measured 3.54e-7 -> bound 1.42e-6;   tanh measured 5.83e-8 -> bound 2.33e-7.   16-bit: one rounding of
    the stored value on top.  The later stages take the kernel's own gz, so their sums carry the derived k of gn_from_gz and gx the
    usual bound."""
    i = C.gn_inputs(*sh)
    o = _gn_call(L, i, sh, dt, act, True)
    assert o["rc"] == 0
    want = C.gn_gz(i, sh[2], act, True)
    scale = (i["gy"] * C.MASK_SCALE).abs()
    err = (o["gz"].double().cpu() - want).abs()
    if dt == MV_F32:
        print(f"[gn-dact] act{act} {sh}: max |gz - ref| / |gy mask_scale| = {float((err / scale.clamp(min=1)).max()):.3e}")
    tol = DACT_REL[act] * scale + C.U_OUT[dt] * want.abs() * (dt != MV_F32) + C.TINY[dt]
    bad = ~(err <= tol)
    assert not bool(bad.any()), (int(bad.sum()), float((err - tol).max()))
    T = sh[3]
    _gn_check(o, i, sh, dt, None, f"gn {sh} act{act}", exact_gz=False, T_chain=max(8, C.cdiv(T, 256)))


@pytest.mark.parametrize("dt", DT16, ids=dtid)
@pytest.mark.parametrize("act", (C.ACT_LRELU, C.ACT_SILU), ids=("lrelu", "silu"))
def test_groupnorm_bwd_channel_slices_equal_the_dense_call(L, act, dt):
    """x and gy as channel slices of a wider tensor (functional.py's GRC branches): once at an offset that keeps 16-byte alignment
    (vector path) and once at an odd element offset (scalar path although T % 8 == 0).  Same bits as the dense call."""
    sh = (2, 8, 2, 64)
    B, Cc, G, T = sh
    i = C.gn_inputs(*sh)
    dense = _gn_call(L, i, sh, dt, act, True)
    assert dense["rc"] == 0
    for off in (3 * T, 3 * T + 1)[:1 if act == C.ACT_SILU else 2]:      # SiLU's sums are not exact: only the same (vector) path repeats bits
        views = []
        for n in ("x", "gy"):
            buf = nans(off + B * (Cc + 8) * T + 16, dt)
            v = buf[off:off + B * (Cc + 8) * T].view(B, Cc + 8, T)[:, :Cc]
            v.copy_(dev(i[n], dt))
            views.append(v)
        assert (views[0].data_ptr() % 16 == 0) == (off % 8 == 0)
        o = _gn_call(L, i, sh, dt, act, True, x=views[0], gy=views[1])
        assert o["rc"] == 0
        for n in ("gz", "gx", "dgw", "dgb", "ws"):
            assert torch.equal(o[n], dense[n]), (off, n)


@pytest.mark.parametrize("dt", DT16, ids=dtid)
def test_groupnorm_bwd_mask_four_bytes_into_a_buffer(L, dt):
    """The vector path reads the mask as 8-byte words: a mask that starts 4 bytes into a buffer takes the scalar path and equals
    the aligned call."""
    sh = (2, 8, 2, 64)
    i = C.gn_inputs(*sh)
    dense = _gn_call(L, i, sh, dt, C.ACT_LRELU, True)
    buf = torch.zeros(i["mask"].numel() + 16, dtype=torch.uint8, device="cuda")
    m = buf[4:4 + i["mask"].numel()].view(i["mask"].shape)
    m.copy_(i["mask"])
    assert m.data_ptr() % 8 == 4
    o = _gn_call(L, i, sh, dt, C.ACT_LRELU, True, maskt=m)
    assert o["rc"] == 0 and dense["rc"] == 0
    for n in ("gz", "gx", "dgw", "dgb", "ws"):
        assert torch.equal(o[n], dense[n]), n
    check(o["gz"], C.exact(C.gn_gz(i, 2, C.ACT_LRELU, True), unit=0.5, stored=True), dt, "gz")


def test_groupnorm_bwd_refuses_more_than_65535_rows(L):
    z = torch.zeros(64, device="cuda")
    gz, ws, gx = nans(64), nans(64), nans(64)
    rc = call(L.mv_groupnorm_bwd, z, z, z, z, None, None, None, f(1.0), 0, f(0.5), gz, ws, gx, None, None, 8192, 8, 1, 2, 8, 1, 8, 1, MV_F32)
    torch.cuda.synchronize()
    assert rc == C.MV_ERR_ARG and untouched(gz, ws, gx)


# =============================================================================================== FiLM, linear, avgpool, copy2d, act
@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("a", C.FILM_CASES, ids=str)
def test_film_bwd(L, a, dt):
    """C > F: pass-through channels; F > C: the trailing gproj entries stay zero (the call zero-fills gproj)."""
    B, Cc, Fd, T = a
    r = C.film_reference(*a)
    gx, gp = nans((B, Cc, T), dt), nans((B, 2 * Fd))
    assert call(L.mv_film_bwd, dev(r["x"], dt), dev(r["gy"], dt), dev(r["proj"], dt), gx, gp, B, Cc, T, Fd, dt) == 0
    check(gx, r["gx"], dt, f"film {a} gx")
    check(gp, r["gproj"], MV_F32, f"film {a} gproj")


@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("a", C.LINEAR_CASES, ids=str)
def test_linear_bwd(L, a, dt):
    M, N, Kd = a
    r = C.linear_reference(*a)
    for no_gx, no_gb in ((False, False), (True, False), (False, True)):
        gx, gw, gb = None if no_gx else nans((M, Kd)), nans((N, Kd)), None if no_gb else nans(N)
        assert call(L.mv_linear_bwd, dev(r["x"], dt), dev(r["w"], dt), f32(r["gy"]), gx, gw, gb, M, N, Kd, dt) == 0
        check(gw, r["gw"], MV_F32, f"linear {a} gw")
        if gx is not None:
            check(gx, r["gx"], MV_F32, f"linear {a} gx")
        if gb is not None:
            check(gb, r["gb"], MV_F32, f"linear {a} gb")


@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("T,s", C.AVGPOOL_CASES, ids=str)
def test_avgpool1d_bwd(L, T, s, dt):
    r = C.avgpool_reference(T, s)
    gx = nans((3, T), dt)
    assert call(L.mv_avgpool1d_bwd, dev(r["gy"], dt), gx, 3, T, s, dt) == 0
    check(gx, r["gx"], dt, f"avgpool {T} / {s}")
    assert bool((r["gx"].ref[:, (T // s) * s:] == 0).all())


@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("case", C.COPY_CASES, ids=lambda c: c[0])
def test_copy2d(L, case, dt):
    """Every row lands where the strides say, nothing else of the NaN-filled destination is written; vector and scalar arms."""
    g = C.copy_layout(case)
    src = ((torch.arange(g["s_len"] + 16) % 251) - 125).to(TORCH_DT[dt]).cuda()
    dst = nans(g["d_len"] + 16, dt)
    sv, dv = src[g["s_off"]:], dst[g["d_off"]:]
    rc = call(L.mv_copy2d, sv, dv, g["n"], g["ro"], g["ri"], g["s_os"], g["s_rs"], g["d_os"], g["d_rs"], dt)
    assert rc == 0
    want = torch.full_like(dst, float("nan"))
    for o, r in itertools.product(range(g["ro"]), range(g["ri"])):
        a, b = g["s_off"] + o * g["s_os"] + r * g["s_rs"], g["d_off"] + o * g["d_os"] + r * g["d_rs"]
        want[b:b + g["n"]] = src[a:a + g["n"]]
    assert torch.equal(torch.isnan(dst), torch.isnan(want)) and torch.equal(dst.nan_to_num(7.0), want.nan_to_num(7.0))


def test_copy2d_refuses_more_than_65535_rows(L):
    src, dst = torch.zeros(64, device="cuda"), nans(64)
    assert call(L.mv_copy2d, src, dst, 1, 256, 256, 0, 0, 0, 0, MV_F32) == C.MV_ERR_ARG
    torch.cuda.synchronize()
    assert untouched(dst)


@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
def test_act_bwd_and_the_zero_point(L, dt):
    """none, LeakyReLU(0.5) and tanh from the activation's output.  At y = +0 and y = -0 the project's LeakyReLU derivative is 1
    (every site in csrc/ selects y >= 0 ? 1 : slope); torch's autograd gives `slope` there.  ACT_SILU is refused."""
    r = C.act_reference()
    n = r["y"].numel()
    for act, name, y in ((C.ACT_NONE, "none", r["y"]), (C.ACT_LRELU, "lrelu", r["y"]), (C.ACT_TANH, "tanh", r["yt"])):
        gx = nans(n, dt)
        yd = dev(y, dt)
        assert bool(torch.signbit(yd[(y == 0).cuda()]).any()) and not bool(torch.signbit(yd[(y == 0).cuda()]).all())   # both zeros arrive
        assert call(L.mv_act_bwd, dev(r["gy"], dt), yd, gx, n, act, f(C.SLOPE), dt) == 0
        check(gx, r[name], dt, f"act_bwd {name}")
    at0 = (r["y"] == 0).cuda()
    gx = nans(n, dt)
    assert call(L.mv_act_bwd, dev(r["gy"], dt), dev(r["y"], dt), gx, n, C.ACT_LRELU, f(C.SLOPE), dt) == 0
    z = r["y"].clone().requires_grad_(True)
    torch.nn.functional.leaky_relu(z, C.SLOPE).backward(r["gy"])
    assert torch.equal(gx[at0].double().cpu(), r["gy"][at0.cpu()]) and torch.equal(z.grad[at0.cpu()], C.SLOPE * r["gy"][at0.cpu()])
    gx = nans(n, dt)
    assert call(L.mv_act_bwd, dev(r["gy"], dt), dev(r["y"], dt), gx, n, C.ACT_SILU, f(C.SLOPE), dt) == C.MV_ERR_ARG
    torch.cuda.synchronize()
    assert untouched(gx)


# =============================================================================================== conv2d
@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("a", C.CONV2D_CASES, ids=str)
def test_conv2d_flip_and_wgrad(L, a, dt):
    B, Cin, Cout, H, W, kh, kw, ph, pw = a
    r = C.conv2d_reference(*a)
    wt, gw = nans((Cin, Cout, kh, kw), dt), nans((Cout, Cin, kh, kw))
    assert call(L.mv_conv2d_flip_weights, dev(r["w"], dt), wt, Cout, Cin, kh, kw, dt) == 0
    check(wt, r["wt"], dt, f"conv2d {a} flipped weights")
    assert call(L.mv_conv2d_wgrad, dev(r["x"], dt), dev(r["gy"], dt), gw, B, Cin, H, W, Cout, kh, kw, ph, pw, dt) == 0
    check(gw, r["gw"], MV_F32, f"conv2d {a} gw")


# =============================================================================================== mv_grc_fold_bwd
GRC_OUT = ("g_conv_w", "g_conv_b", "g_A", "g_B", "g_s", "g_proj_w", "g_proj_b")


def _grc_call(L, i, a, dt):
    outs = {n: nans(s) for n, s in zip(GRC_OUT, (i["conv_w"].shape, i["conv_b"].shape, i["A"].shape, i["Bm"].shape, (1,),
                                                 i["proj_w"].shape, i["conv_b"].shape))}
    rc = call(L.mv_grc_fold_bwd, f32(i["g_weff"]), f32(i["g_beff"]), dev(i["conv_w"], dt), dev(i["conv_b"], dt), dev(i["A"], dt),
              dev(i["Bm"], dt), dev(i["s"], dt), dev(i["proj_w"], dt), *[outs[n] for n in GRC_OUT], *a, dt)
    return rc, outs


@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("a", C.GRC_CASES, ids=str)
def test_grc_fold_bwd_exact(L, a, dt):
    """All seven gradients bit for bit, the scalar g_s included; (64, 40, 3, 4, 16) needs 92.5 KB of LDS (the raised-limit path)."""
    i, r = C.grc_reference(*a)
    rc, outs = _grc_call(L, i, a, dt)
    assert rc == 0
    for n in GRC_OUT:
        check(outs[n], r[n], MV_F32, f"grc {a} {n}")


def test_grc_fold_bwd_refuses_more_than_160k_of_lds(L):
    i = C.grc_inputs(*C.GRC_REFUSED)
    rc, outs = _grc_call(L, i, C.GRC_REFUSED, MV_F32)
    torch.cuda.synchronize()
    assert rc == C.MV_ERR_UNSUPPORTED and untouched(*outs.values())


# =============================================================================================== losses, scale
@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("n", C.LOSS_N)
@pytest.mark.parametrize("kind", range(5))
def test_loss_fwd_bwd(L, kind, n, dt):
    """Value added to a pre-filled loss_acc, gx and gy = -gx (kinds 1 and 4); exact for n a power of two, bounded otherwise.
    131073 elements pass the 512-workgroup cap; gx and gy are each NULL once."""
    r = C.loss_reference(kind, n)
    x, y = dev(r["x"], dt), dev(r["y"], dt)
    two = kind in (1, 4)
    for no_gx, no_gy in ((False, False), (True, False), (False, True)):
        acc = torch.full((1,), 5.0, device="cuda")
        gx, gy = None if no_gx else nans(n, dt), nans(n, dt) if (two and not no_gy) else None
        assert call(L.mv_loss_fwd_bwd, x, y if two else None, f(1.0), f(0.5), acc, gx, gy, n, kind, dt) == 0
        check(acc, r["loss"], MV_F32, f"loss kind {kind} n {n}")
        if gx is not None:
            check(gx, r["gx"], dt, f"loss kind {kind} n {n} gx")
        if gy is not None:
            check(gy, r["gx"]._replace(ref=-r["gx"].ref), dt, f"loss kind {kind} n {n} gy")


@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("n", (1, 255, 256, 131073 * 5))
def test_scale_and_scale_to(L, n, dt):
    """The factor by value (0.5) and times a device scalar (0.25); in place and out of place; past the 2048-workgroup cap."""
    x = C.ints((n,), 115)
    fd = torch.tensor([0.25], device="cuda")
    for fdev, k in ((None, 0.5), (fd, 0.125)):
        y = nans(n, dt)
        assert call(L.mv_scale_to, dev(x, dt), y, fdev, f(0.5), n, dt) == 0
        assert_same(y, x * k, f"scale_to n {n}")
        xd = dev(x, dt)
        assert call(L.mv_scale, xd, fdev, f(0.5), n, dt) == 0
        assert_same(xd, x * k, f"scale n {n}")


# =============================================================================================== ODConvTranspose bank gradient on MFMA
@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("shape", C.ODT_SHAPES + ((16, 8, 16, 8),), ids=str)
def test_odconvT_layout_maps_are_permutations(L, shape, dt):
    """mv_odconvT_adjoint_weights against its index restatement; mv_nct_to_ntc_window into a padded, pre-zeroed buffer at row `pad`
    against odt_pad_grad (pad > 0; ks 6 / stride 3 is the output_padding = 1 geometry).  Nothing outside the window is written."""
    Cin, Cout, ks, stride = shape
    K, B, Tin = 3, 2, 37
    w = C.ints((K, Cin, Cout, ks), 141)
    out = nans((K, Cin, stride * Cout, 2), dt)
    assert call(L.mv_odconvT_adjoint_weights, dev(w, dt), out, K, Cin, Cout, ks, stride, dt) == 0
    assert_same(out, C.adjoint_weights(w, stride), f"adjoint weights {shape}")
    pad, opad = stride // 2, (stride % 2 if stride > 1 else 0)
    Tout = (Tin - 1) * stride - 2 * pad + ks + opad
    g = C.ints((B, Cout, Tout), 142)
    rows = (Tin + 1) * stride
    gp = nans((B, rows, Cout), dt)
    win = ctypes.c_void_p(gp.data_ptr() + pad * Cout * gp.element_size())
    assert call(L.mv_nct_to_ntc_window, dev(g, dt), win, B, Cout, Tout, rows * Cout, dt) == 0
    want = C.odt_pad_grad(g, Tin, stride, pad).view(B, rows, Cout)
    assert_same(gp[:, pad:pad + Tout], want[:, pad:pad + Tout], f"window {shape}")
    assert untouched(gp[:, :pad], gp[:, pad + Tout:])


def _odt_call(L, r, shape, B, Tin, K, dt, x_cl=None, gp=None, alpha=None):
    Cin, Cout, ks, stride = shape
    gw, ga = nans((K, Cin, Cout, ks)), f32(r["galpha0"])
    ws = torch.full((L.mv_odconvT_wgrad_workspace_bytes(B, Cin, Cout, ks, K, dt),), 0xFF, dtype=torch.uint8, device="cuda")
    rc = call(L.mv_odconvT_wgrad_mfma, dev(r["x_cl"], dt) if x_cl is None else x_cl, dev(r["gp"], dt) if gp is None else gp, dev(r["w"], dt),
              f32(r["alpha"] if alpha is None else alpha), gw, ga, ws, B, Tin, Cin, Cout, ks, stride, K, dt)
    return rc, gw, ga


@pytest.mark.parametrize("dt", DT16, ids=dtid)
@pytest.mark.parametrize("case", C.ODT_CASES, ids=str)
def test_odconvT_wgrad_mfma_exact(L, case, dt):
    """dconv_wgrad_kernel<T,1,2,128> with per-sample output, the alpha chain and the layout map back: gw and galpha bit for bit with
    the fp64 gradient of F.conv_transpose1d; one, two and three 128-position chunks a sample, remainders in both tile directions."""
    si, B, Tin, K = case
    r = C.odt_reference(*case)
    rc, gw, ga = _odt_call(L, r, C.ODT_SHAPES[si], B, Tin, K, dt)
    assert rc == 0
    check(gw, r["gw"], MV_F32, f"odconvT {case} gw")
    check(ga, r["galpha"], MV_F32, f"odconvT {case} galpha")


@pytest.mark.parametrize("dt", DT16, ids=dtid)
def test_odconvT_wgrad_mfma_impulses(L, dt):
    """A single 1 in x at t in {0, 127, 128, Tin - 1} and a single 1 in gp on row t or t + 1 (the halo row crosses each chunk edge and
    reaches the padded row Tin) under a one-hot alpha: exactly one non-zero element of gw, at [bank][c][o][q * stride + r], and the
    sample's galpha row gains w[:, c, o, j]; the other samples' rows keep their integers."""
    shape = Cin, Cout, ks, stride = C.ODT_SHAPES[0]
    B, Tin, K = 3, 257, 4
    r = C.odt_reference(0, B, Tin, K)
    x = torch.zeros(B, Tin, Cin, dtype=TORCH_DT[dt], device="cuda")
    gp = torch.zeros(B, Tin + 1, stride * Cout, dtype=TORCH_DT[dt], device="cuda")
    alpha = torch.zeros(B, K, dtype=torch.float64)
    alpha[:, 0] = 1.0
    for n, (t, q) in enumerate(itertools.product((0, 127, 128, Tin - 1), (0, 1))):
        b, c, ro, kb = n % B, (3 * n + 1) % Cin, (5 * n + 2) % (stride * Cout), n % K
        alpha[b] = 0.0
        alpha[b, kb] = 1.0
        x[b, t, c] = 1.0
        gp[b, t + q, ro] = 1.0
        rc, gw, ga = _odt_call(L, r, shape, B, Tin, K, dt, x_cl=x, gp=gp, alpha=alpha)
        assert rc == 0
        o, j = ro % Cout, q * stride + ro // Cout
        want = torch.zeros(K, Cin, Cout, ks, dtype=torch.float64)
        want[kb, c, o, j] = 1.0
        assert_same(gw, want, f"impulse x[{b},{t},{c}] gp[{b},{t + q},{ro}]")
        wga = r["galpha0"].clone()
        wga[b] += r["w"][:, c, o, j]
        assert_same(ga, wga, f"impulse galpha at t {t} q {q}")
        x[b, t, c] = 0.0
        gp[b, t + q, ro] = 0.0
        alpha[b] = 0.0
        alpha[b, 0] = 1.0


def test_odconvT_wgrad_mfma_refusals_write_nothing(L):
    """fp32, ks != 2 * stride, Cin % 8 != 0 and a misaligned operand."""
    B, Tin, K = 1, 8, 2
    for Cin, Cout, ks, stride, dt, off, code in ((8, 4, 4, 2, MV_F32, 0, C.MV_ERR_UNSUPPORTED), (8, 4, 5, 2, MV_BF16, 0, C.MV_ERR_ARG),
                                                 (12, 4, 4, 2, MV_BF16, 0, C.MV_ERR_ARG), (8, 4, 4, 2, MV_F16, 1, C.MV_ERR_ARG)):
        x = offset_view(torch.zeros(B, Tin, Cin, dtype=TORCH_DT[dt], device="cuda"), off)
        gp = torch.zeros(B, Tin + 1, stride * Cout, dtype=TORCH_DT[dt], device="cuda")
        w = torch.zeros(K, Cin, Cout, ks, dtype=TORCH_DT[dt], device="cuda")
        gw, ga, ws = nans((K, Cin, Cout, ks)), nans((B, K)), nans(8192)
        rc = call(L.mv_odconvT_wgrad_mfma, x, gp, w, torch.ones(B, K, device="cuda"), gw, ga, ws, B, Tin, Cin, Cout, ks, stride, K, dt)
        torch.cuda.synchronize()
        assert rc == code and untouched(gw, ga, ws), (Cin, Cout, ks, stride, dt, off, rc)
