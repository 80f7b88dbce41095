"""csrc/norm_elem.hip and csrc/conv_generic.hip, one entry point at a time through the raw C ABI, against the float64 references of
tests/front_cases.py: the generic convolutions (the GPU-side reference of the fused-kernel cross-checks), ODConv attention in both
launch forms, the one-launch generator prologue, two-phase GroupNorm, FiLM, scale-shift, activations, avg-pool, the MPD fold, the
layout transposes, casts, the dense layer and the GRC+LoRA weight fold.

Operands are small integers and dyadic scalars: a sum of products is exact in fp32 in any order (tests/test_host_front_cases.py proves
it row by row), a 16-bit store is the one RNE rounding of that exact value, and the tests ask for bit equality in all three storage
types.  Outputs behind rsqrtf, expf, tanhf or the __expf SiLU carry the per-element bound of front_cases.tolerance (4 x the function's
measured error, printed by the test next to what it saw).  Nothing is compared by a norm over a tensor.  Outputs and workspaces start as
NaN; windows and slices sit in NaN-filled larger buffers whose remainder must still be NaN afterwards; a refusal writes nothing.
The helpers are those of tests/test_gpu_backward_kernels.py."""
import ctypes

import pytest
import torch

import front_cases as F
from front_cases import ALL_DT, MV_BF16, MV_F16, MV_F32, TORCH_DT
from test_gpu_backward_kernels import (L, _stop_at_a_gpu_error, assert_same, call, dev, dtid, f, f32, nans, offset_view,  # noqa: F401
                                       untouched)

pytestmark = pytest.mark.gpu
DT16 = (MV_BF16, MV_F16)
name_id = lambda c: c.name if hasattr(c, "name") else str(c[0])


def check(got, out, dt, what, fn=None, fn_scale=None):
    """An Out of front_cases: k == 0 -> the bits of the exact value stored in type dt; else the per-element bound (with the measured
    function term), the largest share of the bound an element used printed beside it."""
    if out.k == 0:
        return assert_same(got.reshape(out.ref.shape), F.stored(out, dt), what)
    got = got.detach().double().cpu().reshape(out.ref.shape)
    tol = F.tolerance(out, dt, fn, fn_scale)
    err = (got - out.ref).abs()
    if fn is not None and dt == MV_F32:
        print(f"[front] {what}: {fn}, largest |got - ref| / bound = {float((err / tol).max()):.3f}")
    bad = ~(err <= tol)
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements outside the bound; first {i}: got {got[i].item()} "
                             f"want {out.ref[i].item()} bound {tol[i].item()}")


def place(t, lay, dt, shape=None):
    """A [B][C][T] tensor (None: left NaN) at layout `lay` inside a NaN-filled buffer: (buffer, strided view, mask of the view's elements)."""
    B, C, T = t.shape if shape is None else shape
    bs, cs = F.strides(lay, C, T)
    buf = nans(lay.off + B * bs + 16, dt)
    v = buf[lay.off:].as_strided((B, C, T), (bs, cs, 1))
    own = torch.zeros(buf.numel(), dtype=torch.bool, device="cuda")
    own[lay.off:].as_strided((B, C, T), (bs, cs, 1)).fill_(True)
    if t is not None:
        v.copy_(dev(t, dt))
    assert buf.data_ptr() % 16 == 0
    return buf, v, own


def opt(t, dt):
    return None if t is None else dev(t, dt)


# =============================================================================================== mv_conv1d_fwd
def _conv1d(L, c, dt):
    r = F.conv1d_reference(c)
    if c.xs:
        _, x, _ = place(r["x"], F.Lay(0, 5, 7), dt)
    else:
        x = dev(r["x"], dt)
    wide = nans((c.B, c.Cout + c.yoff + (2 if c.yoff else 0), c.Tout), dt)
    y = wide[:, c.yoff:c.yoff + c.Cout]
    res = None
    if c.res:
        rw = nans(wide.shape, dt)
        res = rw[:, c.yoff:c.yoff + c.Cout]
        res.copy_(dev(r["res"], dt))
        assert res.stride() == y.stride()
    rc = call(L.mv_conv1d_fwd, x, dev(r["w"], dt), opt(r["bias"], dt), None if r["alpha"] is None else f32(r["alpha"]), res, y, c.B, c.Cin, c.Tin,
              c.Cout, c.Tout, c.ks, c.stride, c.pad, c.dil, c.groups, c.K, c.act, f(F.SLOPE), x.stride(0), x.stride(1), y.stride(0), y.stride(1), dt)
    return rc, r, wide, y


@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("c", F.CONV1D_CASES, ids=name_id)
def test_conv1d_fwd(L, c, dt):
    """Tile edges in time, output and input channels, groups down to depthwise, strides, dilations, paddings, one to eight banks with
    and without the per-bank bias, the residual through y's strides, channel slices on both sides, all four activations, the
    raised-limit LDS arm.  Bit for bit with fp64 except behind tanh / SiLU."""
    rc, r, wide, y = _conv1d(L, c, dt)
    assert rc == 0
    check(y, r["y"], dt, f"conv1d {c.name}", F.ACT_FN.get(c.act), r["fn_scale"])
    assert untouched(wide[:, :c.yoff], wide[:, c.yoff + c.Cout:])


def _refuse_conv(fn, args, head, tail):
    z = torch.zeros(64, device="cuda")
    y = nans(64)
    rc = call(fn, *head(z), y, *args, *tail)
    torch.cuda.synchronize()
    return rc, y


@pytest.mark.parametrize("name,shape,has_alpha,code", F.CONV1D_REFUSED, ids=[r[0] for r in F.CONV1D_REFUSED])
def test_conv1d_fwd_refusals_write_nothing(L, name, shape, has_alpha, code):
    B, Cin, Tin, Cout, Tout, ks, stride, pad, dil, groups, nb = shape
    rc, y = _refuse_conv(L.mv_conv1d_fwd, (B, Cin, Tin, Cout, Tout, ks, stride, pad, dil, groups, nb, 0, f(0.25), Cin * Tin, Tin, Cout * Tout, Tout, MV_F32),
                         lambda z: (z, z, None, z if has_alpha else None, None), ())
    assert rc == code and untouched(y), (name, rc)


# =============================================================================================== mv_conv_transpose1d_fwd
@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("c", F.CONVT_CASES, ids=name_id)
def test_conv_transpose1d_fwd(L, c, dt):
    """Six (stride, ks) pairs, output_padding 0 and stride - 1, padding 0 and (ks - stride) / 2, dilation 1 and 2, outputs past 128 and
    256 steps, ragged channel tiles, banks as in conv1d.  Exact: no term is skipped by the kernel's xi < xw guard."""
    r = F.convT_reference(c)
    y = nans((c.B, c.Cout, c.Tout), dt)
    rc = call(L.mv_conv_transpose1d_fwd, dev(r["x"], dt), dev(r["w"], dt), opt(r["bias"], dt), None if r["alpha"] is None else f32(r["alpha"]), y,
              c.B, c.Cin, c.Tin, c.Cout, c.Tout, c.ks, c.stride, c.pad, c.dil, c.K, c.act, f(F.SLOPE), dt)
    assert rc == 0
    check(y, r["y"], dt, f"convT {c.name}", F.ACT_FN.get(c.act), r["fn_scale"])


@pytest.mark.parametrize("name,shape,has_alpha,code", F.CONVT_REFUSED, ids=[r[0] for r in F.CONVT_REFUSED])
def test_conv_transpose1d_fwd_refusals_write_nothing(L, name, shape, has_alpha, code):
    rc, y = _refuse_conv(L.mv_conv_transpose1d_fwd, (*shape, 0, f(0.25), MV_F32), lambda z: (z, z, None, z if has_alpha else None), ())
    assert rc == code and untouched(y), (name, rc)


# =============================================================================================== mv_conv2d_fwd
@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("c", F.CONV2D_CASES, ids=name_id)
def test_conv2d_fwd(L, c, dt):
    """The discriminator's kernel shapes with their own and with zero padding, the periods as widths, one row of 130 output columns,
    and 65535 rows in grid.z."""
    r = F.conv2d_reference(c)
    y = nans(r["y"].ref.shape, dt)
    rc = call(L.mv_conv2d_fwd, dev(r["x"], dt), dev(r["w"], dt), opt(r["bias"], dt), y, c.B, c.Cin, c.H, c.W, c.Cout, c.kh, c.kw, c.ph, c.pw,
              c.act, f(F.SLOPE), dt)
    assert rc == 0
    check(y, r["y"], dt, f"conv2d {c.name}", F.ACT_FN.get(c.act), r["fn_scale"])


@pytest.mark.parametrize("name,shape,code", F.CONV2D_REFUSED, ids=[r[0] for r in F.CONV2D_REFUSED])
def test_conv2d_fwd_refusals_write_nothing(L, name, shape, code):
    z, y = torch.zeros(64, device="cuda"), nans(64)
    rc = call(L.mv_conv2d_fwd, z, z, None, y, *shape, 0, f(0.25), MV_F32)
    torch.cuda.synchronize()
    assert rc == code and untouched(y)


# =============================================================================================== GroupNorm
@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("c", F.GN_STATS_CASES, ids=name_id)
def test_groupnorm_stats(L, c, dt):
    """mean bit for bit (an integer by construction, at every n); rstd inside k = 2 roundings and the measured rsqrtf error."""
    r = F.gn_stats_reference(c, dt)
    _, x, _ = place(r["x"], c.lay, dt)
    mean, rstd = nans((c.B, c.G)), nans((c.B, c.G))
    assert call(L.mv_groupnorm_stats, x, mean, rstd, c.B, c.C, c.T, c.G, f(F.GN_EPS), x.stride(0), x.stride(1), dt) == 0
    check(mean, r["mean"], MV_F32, f"gn stats {c.name} mean")
    check(rstd, r["rstd"], MV_F32, f"gn stats {c.name} rstd", "rsqrt", r["rstd"].ref)


def _gn_apply(L, c, dt):
    r = F.gn_apply_reference(c)
    _, x, _ = place(r["x"], c.x, dt)
    ybuf, y, yown = place(None, c.y, dt, r["x"].shape)
    res = place(r["res"], c.r, dt)[1] if c.res else None
    mask = None
    if c.mask:
        mb = torch.zeros(r["mask"].numel() + 16, dtype=torch.uint8, device="cuda")
        mask = mb[c.moff:c.moff + r["mask"].numel()]
        mask.copy_(r["mask"].view(-1))
        assert mask.data_ptr() % 8 == c.moff % 8
    rc = call(L.mv_groupnorm_apply, x, f32(r["mean"]), f32(r["rstd"]), dev(r["gw"], dt) if c.gw else None, dev(r["gb"], dt) if c.gb else None, res, mask,
              f(F.MASK_SCALE), y, c.B, c.C, c.T, c.G, c.act, f(F.SLOPE), x.stride(0), x.stride(1), res.stride(0) if c.res else 0, res.stride(1) if c.res else 0,
              y.stride(0), y.stride(1), dt)
    return rc, r, y, ybuf, yown


@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("c", F.GN_APPLY_CASES, ids=name_id)
def test_groupnorm_apply(L, c, dt):
    """The 16-byte arm and the scalar arm by each cause on its own (T, each stride of x / res / y, each base, the mask's address), both
    activation functors, optional affine / residual / mask (keep bytes 1, 2, 128, 255; zeros in every byte lane of both mask words),
    the grid-stride loops.  y is a window of a NaN buffer: nothing else of it is written."""
    rc, r, y, ybuf, yown = _gn_apply(L, c, dt)
    assert rc == 0
    check(y, r["y"], dt, f"gn apply {c.name}", F.ACT_FN.get(c.act), r["fn_scale"])
    assert bool(torch.isnan(ybuf[~yown].float()).all())


def test_groupnorm_refusals_write_nothing(L):
    z = torch.zeros(64, device="cuda")
    y, m, s = nans(64), nans(64), nans(64)
    assert call(L.mv_groupnorm_apply, z, z, z, None, None, None, None, f(1.0), y, 8192, 8, 1, 2, 0, f(0.25), 8, 1, 0, 0, 8, 1, MV_F32) == F.MV_ERR_ARG   # B * C = 65536
    assert call(L.mv_groupnorm_apply, z, z, z, None, None, None, None, f(1.0), y, 2, 8, 1, 3, 0, f(0.25), 8, 1, 0, 0, 8, 1, MV_F32) == F.MV_ERR_ARG      # C % G
    assert call(L.mv_groupnorm_stats, z, m, s, 2, 8, 1, 3, f(1e-5), 8, 1, MV_F32) == F.MV_ERR_ARG
    assert call(L.mv_groupnorm_stats, z, m, s, 2, 8, 1, 2, f(1e-5), 8, 1, 7) == F.MV_ERR_DTYPE
    torch.cuda.synchronize()
    assert untouched(y, m, s)


# =============================================================================================== FiLM, scale-shift, act, avgpool, fold
@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("a", F.FILM_CASES, ids=str)
def test_film_fwd(L, a, dt):
    B, C, Fd, T = a
    r = F.film_reference(*a)
    y = nans((B, C, T), dt)
    assert call(L.mv_film_fwd, dev(r["x"], dt), dev(r["proj"], dt), y, B, C, T, Fd, dt) == 0
    check(y, r["y"], dt, f"film {a}")
    assert call(L.mv_film_fwd, dev(r["x"], dt), dev(r["proj"], dt), y, 65536, 1, T, Fd, dt) == F.MV_ERR_ARG
    check(y, r["y"], dt, "film after the refusal")


@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("a", F.SCALE_SHIFT_CASES, ids=str)
def test_scale_shift_fwd(L, a, dt):
    B, C, T = a
    r = F.scale_shift_reference(*a)
    y = nans((B, C, T), dt)
    assert call(L.mv_scale_shift_fwd, dev(r["x"], dt), dev(r["scale"], dt), dev(r["shift"], dt), y, B, C, T, dt) == 0
    check(y, r["y"], dt, f"scale_shift {a}")
    assert call(L.mv_scale_shift_fwd, dev(r["x"], dt), dev(r["scale"], dt), dev(r["shift"], dt), y, 1, 65536, T, dt) == F.MV_ERR_ARG
    check(y, r["y"], dt, "scale_shift after the refusal")


@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("a", F.ACT_CASES, ids=str)
def test_act_fwd(L, a, dt):
    n, act, res = a
    r = F.act_reference(*a)
    buf = nans(n + 16, dt)
    assert call(L.mv_act_fwd, dev(r["x"], dt), opt(r["res"], dt), buf[8:8 + n], n, act, f(F.SLOPE), dt) == 0
    check(buf[8:8 + n], r["y"], dt, f"act {a}", F.ACT_FN.get(act), r["fn_scale"])
    assert untouched(buf[:8], buf[8 + n:])


@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("a", F.AVGPOOL_CASES, ids=str)
def test_avgpool1d_fwd(L, a, dt):
    rows, T, s = a
    r = F.avgpool_reference(*a)
    To = T // s
    buf = nans(rows * To + 16, dt)
    assert call(L.mv_avgpool1d_fwd, dev(r["x"], dt), buf[8:8 + rows * To], rows, T, s, dt) == 0
    check(buf[8:8 + rows * To], r["y"], dt, f"avgpool {a}")
    assert untouched(buf[:8], buf[8 + rows * To:])
    assert call(L.mv_avgpool1d_fwd, dev(r["x"], dt), buf[:8], 65536, T, s, dt) == F.MV_ERR_ARG
    assert call(L.mv_avgpool1d_fwd, dev(r["x"], dt), buf[:8], rows, s - 1, s, dt) == F.MV_ERR_ARG
    torch.cuda.synchronize()
    assert untouched(buf[:8])


@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("a", F.MPD_CASES, ids=str)
def test_mpd_fold(L, a, dt):
    """Zero padding up to the next multiple of the period; the index map (written from row 0 alone) with -1 in the padding; a NULL
    index is allowed."""
    rows, P, T = a
    r = F.mpd_reference(*a)
    Tp = r["Tp"]
    for with_index in (True, False):
        buf = nans(rows * Tp + 16, dt)
        idx = torch.full((Tp + 2,), -7, dtype=torch.int64, device="cuda")
        assert call(L.mv_mpd_fold, dev(r["x"], dt), buf[8:8 + rows * Tp], idx[1:] if with_index else None, rows, T, P, dt) == 0
        check(buf[8:8 + rows * Tp], r["y"], dt, f"mpd {a}")
        assert untouched(buf[:8], buf[8 + rows * Tp:])
        want = torch.full((Tp + 2,), -7, dtype=torch.int64)
        if with_index:
            want[1:Tp + 1] = r["index"]
        assert torch.equal(idx.cpu(), want)
    y = nans(8, dt)
    assert call(L.mv_mpd_fold, dev(r["x"], dt), y, None, 65536, T, P, dt) == F.MV_ERR_ARG
    torch.cuda.synchronize()
    assert untouched(y)


# =============================================================================================== mv_cast
def _same_bits(got, want, what):
    """Equal as numbers, NaN where NaN is wanted, and the same sign on zeros."""
    g, w = got.double().cpu(), want.double().cpu()
    ok = ((g == w) & (torch.signbit(g) == torch.signbit(w))) | (torch.isnan(g) & torch.isnan(w))
    assert bool(ok.all()), (what, [(i, g[i].item(), w[i].item()) for i in (~ok).nonzero().view(-1)[:6].tolist()])


@pytest.mark.parametrize("dst", ALL_DT, ids=dtid)
@pytest.mark.parametrize("src", ALL_DT, ids=dtid)
def test_cast(L, src, dst):
    """All nine pairs at n = 1 and past the capped grid, then the values that decide the rounding rule (ties to even both ways, both
    zeros, subnormals, the largest finite values, overflow to infinity, NaN)."""
    for n in (1, F.CAP_N):
        x = (F.ints((n,), 301, lo=-300, hi=300) / 4).to(TORCH_DT[src])
        buf = nans(n + 16, dst)
        assert call(L.mv_cast, x.cuda(), src, buf[8:8 + n], dst, n) == 0
        _same_bits(buf[8:8 + n], x.to(TORCH_DT[dst]), f"cast {src}->{dst} n {n}")
        assert untouched(buf[:8], buf[8 + n:])
    sp = F.cast_specials().to(TORCH_DT[src])
    y = torch.zeros(sp.numel(), dtype=TORCH_DT[dst], device="cuda")
    assert call(L.mv_cast, sp.cuda(), src, y, dst, sp.numel()) == 0
    _same_bits(y, sp.to(TORCH_DT[dst]), f"cast {src}->{dst} specials")
    z = nans(8, dst)
    assert call(L.mv_cast, sp.cuda(), 7, z, dst, 8) == F.MV_ERR_DTYPE and call(L.mv_cast, sp.cuda(), src, z, 7, 8) == F.MV_ERR_DTYPE
    torch.cuda.synchronize()
    assert untouched(z)


# =============================================================================================== layout transposes
def _transpose(L, entry, C, T, Cpad, dt, xoff=0, yoff=0, B=3):
    R, Cn, ldx, ldy, x_bs, y_bs = F.transpose_geometry(entry, B, C, T, Cpad)
    x = F.distinct_bits((B, R, ldx), dt)
    want = F.transpose_reference(entry, x, B, C, T, Cpad)
    xd = offset_view(x.cuda(), xoff)
    buf = nans(B * Cn * ldy + 32, dt)
    y = buf[8 + yoff:8 + yoff + B * Cn * ldy]
    fn = getattr(L, "mv_" + entry)
    rc = call(fn, xd, y, B, C, T, *((Cpad,) if "pad" in entry or "crop" in entry else ()), dt)
    assert rc == 0
    bits = torch.int32 if dt == MV_F32 else torch.int16
    assert torch.equal(y.view(bits).cpu(), want.contiguous().view(-1).view(bits)), (entry, C, T, Cpad, F.transpose_plan(entry, B, C, T, Cpad, dt, xoff, yoff))
    assert untouched(buf[:8 + yoff], buf[8 + yoff + B * Cn * ldy:])


@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("shape", F.TR_SHAPES, ids=str)
@pytest.mark.parametrize("entry", ("nct_to_ntc", "ntc_to_nct", "nct_to_ntc_pad", "ntc_to_nct_crop"))
def test_transposes(L, entry, shape, dt):
    """Pairwise distinct elements, batch 3, every tile edge of both kernels; padded channels are zeros written over NaN, cropped input
    columns never appear, nothing outside y is written."""
    C, T = shape
    _transpose(L, entry, C, T, C + 5, dt)
    if entry in ("nct_to_ntc_pad", "ntc_to_nct_crop"):
        _transpose(L, entry, C, T, C, dt)


@pytest.mark.parametrize("dt", DT16, ids=dtid)
@pytest.mark.parametrize("row", F.TR_FAST, ids=lambda r: f"{r[0]}-{r[1]}-{r[2]}-{r[3]}-{r[6]}")
def test_transposes_fast_path_and_each_term_broken(L, row, dt):
    entry, C, T, Cpad, xoff, yoff, _ = row
    _transpose(L, entry, C, T, Cpad, dt, xoff, yoff)


def test_transposes_refusals_write_nothing(L):
    z, y = torch.zeros(64, device="cuda"), nans(64)
    assert call(L.mv_nct_to_ntc_pad, z, y, 2, 4, 4, 3, MV_F32) == F.MV_ERR_ARG
    assert call(L.mv_ntc_to_nct_crop, z, y, 2, 4, 4, 3, MV_F32) == F.MV_ERR_ARG
    assert call(L.mv_nct_to_ntc, z, y, 65536, 1, 1, MV_F32) == F.MV_ERR_ARG
    assert call(L.mv_ntc_to_nct, z, y, 2, 4, 4, 9) == F.MV_ERR_DTYPE
    torch.cuda.synchronize()
    assert untouched(y)


# =============================================================================================== mv_linear_fwd
@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("a", F.LINEAR_CASES, ids=str)
def test_linear_fwd(L, a, dt):
    M, N, Kd = a
    r = F.linear_reference(*a)
    for bias, name in ((dev(r["b"], dt), "y"), (None, "y_nobias")):
        buf = nans(M * N + 16, dt)
        assert call(L.mv_linear_fwd, dev(r["x"], dt), dev(r["w"], dt), bias, buf[8:8 + M * N], M, N, Kd, dt) == 0
        check(buf[8:8 + M * N], r[name], dt, f"linear {a} {name}")
        assert untouched(buf[:8], buf[8 + M * N:])


# =============================================================================================== mv_odconv_attn_fwd
def check_alpha(got, r, what):
    got = got.double().cpu()
    err = (got - r["alpha"]).abs()
    print(f"[front] {what}: exp, largest |alpha - ref| / bound = {float((err / r['alpha_tol']).max()):.3f}")
    bad = ~(err <= r["alpha_tol"])
    assert not bool(bad.any()), (what, got[bad][:4], r["alpha"][bad][:4], r["alpha_tol"][bad][:4])


@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("c", F.ATTN_CASES, ids=name_id)
def test_odconv_attn_fwd(L, c, dt):
    """Both launch forms on both sides of C * T = 16384, rowmean's vector and scalar arms, K = 1 .. 64; pooled is exact for a power of
    two T, alpha inside the softmax bound (logits at +-80 included: the maximum is subtracted)."""
    r = F.attn_reference(c)
    x = offset_view(dev(r["x"], dt), c.xoff)
    alpha, pooled = nans((c.B, c.K)), nans((c.B, c.C)) if c.pooled else None
    assert call(L.mv_odconv_attn_fwd, x, dev(r["w"], dt), opt(r["b"], dt), alpha, pooled, c.B, c.C, c.T, c.K, dt) == 0
    if c.pooled:
        check(pooled, r["pooled"], MV_F32, f"attn {c.name} pooled")
    check_alpha(alpha, r, f"attn {c.name}")


def test_odconv_attn_fwd_refusals_write_nothing(L):
    z = torch.zeros(128, device="cuda")
    alpha, pooled = nans(130), nans(64)
    assert call(L.mv_odconv_attn_fwd, z, z, z, alpha, pooled, 2, 1, 1, 65, MV_F32) == F.MV_ERR_ARG
    assert call(L.mv_odconv_attn_fwd, z, z, z, alpha, pooled, 2, 16384, 1, 4, MV_F32) == F.MV_ERR_ARG       # 65552 bytes of LDS
    assert call(L.mv_odconv_attn_fwd, z, z, z, alpha, pooled, 2, 1, 1, 4, 5) == F.MV_ERR_DTYPE
    torch.cuda.synchronize()
    assert untouched(alpha, pooled)


# =============================================================================================== mv_gen_prologue(_in)
def _prologue(L, c, dt, in_dt, r, null_spk=False, entry_in=True):
    ti = TORCH_DT[in_dt]
    alpha, x_cl = nans((c.B, c.K)), nans((c.B, c.T, c.C), dt)
    proj = nans((c.B, c.F2), dt) if c.film else None
    zb = torch.full((c.zero_n + 8,), 7.0, device="cuda")
    spk = None if (c.ds == 0 or null_spk) else dev(r["spk"], ti)
    emo = None if c.de == 0 else dev(r["emo"], ti)
    args = (dev(r["mel"], ti), dev(r["aw"], dt), opt(r["ab"], dt), spk, emo, dev(r["fw"], dt), opt(r["fb"], dt), alpha, x_cl, proj,
            zb[4:] if c.zero_n else None, ctypes.c_long(c.zero_n), c.B, c.C, c.T, c.K, c.ds, c.de, c.cond, c.F2)
    rc = call(L.mv_gen_prologue_in, *args, in_dt, dt) if entry_in else call(L.mv_gen_prologue, *args, dt)
    return rc, alpha, x_cl, proj, zb


@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("c", F.PROLOGUE_CASES, ids=name_id)
def test_gen_prologue(L, c, dt):
    """Every arm of gen_prologue_kernel, one argument away from the base row: x_cl a bit-exact transpose (RNE-rounded when fp32 inputs
    feed 16-bit storage), film_proj exact, zero_buf zeroed inside its sentinels, alpha inside the softmax bound."""
    r = F.prologue_reference(c)
    in_dt = MV_F32 if c.in32 else dt
    rc, alpha, x_cl, proj, zb = _prologue(L, c, dt, in_dt, r, entry_in=c.in32 or c.name == "base")
    assert rc == 0
    check(x_cl, r["x_cl"], dt, f"prologue {c.name} x_cl")
    if c.film:
        check(proj, r["proj"], dt, f"prologue {c.name} film_proj")
    want = torch.full((c.zero_n + 8,), 7.0)
    want[4:4 + c.zero_n] = 0.0
    assert torch.equal(zb.cpu(), want)
    check_alpha(alpha, r, f"prologue {c.name}")


@pytest.mark.parametrize("name,over,in_dt,dt,null_spk,code", F.PROLOGUE_REFUSED, ids=[r[0] for r in F.PROLOGUE_REFUSED])
def test_gen_prologue_refusals_write_nothing(L, name, over, in_dt, dt, null_spk, code):
    c = F._pr(name, **{**dict(B=2, T=4), **over})
    r = {k: torch.zeros(s) for k, s in dict(mel=(c.B, c.C, c.T), aw=(c.K, c.C), ab=(c.K,), spk=(c.B, c.ds), emo=(c.B, c.de), fw=(c.F2, c.cond),
                                            fb=(c.F2,)).items()}
    rc, alpha, x_cl, proj, zb = _prologue(L, c, dt, dt if in_dt is None else in_dt, r, null_spk)
    torch.cuda.synchronize()
    assert rc == code and untouched(alpha, x_cl, proj) and bool((zb == 7.0).all()), (name, rc)


# =============================================================================================== mv_grc_fold_weights
def _grc(L, a, dt, i):
    Cin, Cout, ks, groups, rank = a
    w, b = nans((Cout, Cin, ks), dt), nans(Cout, dt)
    rc = call(L.mv_grc_fold_weights, *[dev(i[n], dt) for n in ("conv_w", "conv_b", "A", "Bm", "s", "proj_w", "proj_b")], w, b, *a, dt)
    return rc, w, b


@pytest.mark.parametrize("dt", ALL_DT, ids=dtid)
@pytest.mark.parametrize("a", F.GRC_CASES, ids=str)
def test_grc_fold_weights(L, a, dt):
    """The LDS arm (up to exactly 48 KB of operands) and the straight-from-global arm; the LoRA term on the centre tap only."""
    i, r = F.grc_fold_reference(*a)
    rc, w, b = _grc(L, a, dt, i)
    assert rc == 0
    check(w, r["w_eff"], dt, f"grc fold {a} w_eff")
    check(b, r["b_eff"], dt, f"grc fold {a} b_eff")


@pytest.mark.parametrize("a", F.GRC_REFUSED, ids=str)
def test_grc_fold_weights_refusals_write_nothing(L, a):
    i = {n: torch.zeros(64) for n in ("conv_w", "conv_b", "A", "Bm", "s", "proj_w", "proj_b")}
    rc, w, b = _grc(L, a, MV_F32, i)
    torch.cuda.synchronize()
    assert rc == F.MV_ERR_ARG and untouched(w, b)
