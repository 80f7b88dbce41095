"""Host checks of tests/disc_cases.py (no GPU): the tables name the arm the dispatcher restatement selects, the restatement agrees
with the library's own plan queries (mv_dconv_cl_fwd_plan, mv_dconv_wgrad_plan: pure host code), every reachable arm has a row, the
ragged-split rows really split raggedly, and - what keeps the exact GPU tests exact - the fp64 reference of every row's generated
inputs is unchanged by a round trip through bf16 and fp16, with exactly 8 non-zero channels per input position."""
import ctypes

import pytest
import torch

import disc_cases as D

FWD_SHAPES = sorted({D.shape_of(c) for c in D.FWD_CASES})
WG_SHAPES = sorted({D.shape_of(c) for c in D.WGRAD_CASES})

ALL_DT = (D.MV_BF16, D.MV_F16, D.MV_F32)
FWD_GEOMS = ((1, 1, 1), (1, 3, 1), (1, 15, 1), (3, 3, 1), (3, 3, 2), (3, 3, 58))
WG_GEOMS = [(3, 3, 1)] + [(1, k, d) for k in (1, 3, 5, 7, 9, 11, 15) for d in (1, 4, 5)]
# the training shapes of the two discriminator families (B = 64 clips of 8192 samples) and the arms their profiles show; refused shapes
KNOWN_FWD = (((64, 2, 4096, 128, 256, 3, 3, 1), "dconv_cl_wide_kernel<bf16,1,4,8,64,4>"),
             ((64, 2, 4096, 256, 128, 3, 3, 1), "dconv_cl_wide_kernel<bf16,1,4,8,32,2>"),
             ((64, 1, 8192, 128, 256, 1, 15, 1), "dconv_cl_kernel<bf16,4,4,8>"),
             ((64, 1, 8192, 256, 128, 1, 15, 1), "dconv_cl_wide_kernel<bf16,2,2,4,128,8>"),
             ((64, 1, 8192, 64, 32, 1, 15, 1), "dconv_cl_wide_kernel<bf16,4,1,2,64,8>"))
BAD_FWD = (((1, 1, 8, 48, 32, 1, 3, 1), D.MV_ERR_ARG), ((1, 1, 8, 32, 32, 1, 4, 1), D.MV_ERR_ARG), ((1, 1, 8, 32, 32, 1, 3, 65), D.MV_ERR_ARG))
BAD_WG = ((1, 2, 8, 64, 64, 3, 3, 2), (1, 1, 8, 64, 64, 1, 15, 5), (1, 1, 8, 64, 64, 1, 9, 1))
# more than 2^30 chunks (every weight-gradient kernel indexes them with an int), and the issue's small fp32 refusal
HUGE_WG = ((65536, 65536, 8, 8, 8, 3, 3, 1), (65536, 65536, 8, 8, 8, 1, 15, 1), (1, 1, 8, 8, 8, 3, 3, 2))


def _grid(geoms):
    for B, H in ((1, 1), (1, 2), (12, 11), (24, 11)):
        for W in (5, 130, 300):
            for Cin in (24, 32, 64, 96, 128, 192, 256):
                for Cout in (16, 32, 64, 128, 160, 192, 256, 384):
                    for kh, kw, dil in geoms:
                        yield B, H, W, Cin, Cout, kh, kw, dil


def _sweep(arm_fn, dtypes, geoms):
    """Every arm name the dispatcher restatement returns over a grid of valid shapes."""
    names = set()
    for dt in dtypes:
        for shape in _grid(geoms):
            try:
                names.add(arm_fn(*shape, dt).name)
            except D.Refused:
                pass
    return names


@pytest.fixture(scope="module")
def L():
    from hifigan_modified import _native
    return _native.lib()


def _c_fwd(L, shape, dt, head=0, save=0):
    """mv_dconv_cl_fwd_plan: (return code, arm name, the 12 plan ints)."""
    out = (ctypes.c_int * 12)()
    rc = L.mv_dconv_cl_fwd_plan(*shape, dt, head, save, out)
    ps, mw, nb, cch, nwv = out[:5]
    T = D.DT_NAME.get(dt)
    return rc, (f"dconv_cl_wide_kernel<{T},{ps},{mw},{nb},{cch},{nwv}>" if ps else f"dconv_cl_kernel<{T},{nwv},{mw},{nb}>"), list(out)


def _same_fwd(L, shape, dt):
    """The C++ plan against the restatement for one shape: the refusal code, or the arm with its tile; returns the arm's name."""
    rc, name, v = _c_fwd(L, shape, dt)
    try:
        arm = D.fwd_arm(*shape, dt)
    except D.Refused as e:
        assert rc == e.code, (shape, dt, rc, e.code)
        return None
    B, H, W, _, Cout = shape[:5]
    assert rc == 0 and (name, v[5], v[6], v[7]) == tuple(arm), (shape, dt, rc, name, v, arm)
    assert v[8] <= D.LDS_MAX and v[9:] == [D.cdiv(W, arm.npos), D.cdiv(Cout, arm.rows), B * H], (shape, dt, v)
    return name


def _same_wgrad(L, shape, dt):
    out = (ctypes.c_int * 12)()
    rc = L.mv_dconv_wgrad_plan(*shape, dt, out)
    try:
        arm = D.wgrad_arm(*shape, dt)
    except D.Refused as e:
        assert rc == e.code, (shape, dt, rc, e.code)
        return None
    three, tw, wt, otile = out[:4]
    T = D.DT_NAME[dt]
    name = f"dconv_wgrad3_kernel<{T},{otile // 32}>" if three else f"dconv_wgrad_kernel<{T},{shape[5]},{tw},{wt}>"
    assert rc == 0 and (name, wt, otile) + tuple(out[4:8]) == tuple(arm)[:7], (shape, dt, rc, name, list(out), arm)
    assert out[8] <= D.LDS_MAX and list(out[9:]) == [D.cdiv(shape[3], 64), D.cdiv(shape[4], otile), arm.groups], (shape, dt, list(out))
    return name


def test_plan_queries_agree_with_the_restatement(L):
    """mv_dconv_cl_fwd_plan against fwd_arm and mv_dconv_wgrad_plan against wgrad_arm - refusal code, or instantiation, tile and
    split - over the whole sweep grid with both geometry lists and all three storage types, every table row, and the known-answer and
    refusal shapes.  Nothing is left out: a shape the restatement refuses must be refused by the library with the same code.  The
    arms the library's plans name over the sweep are exactly the arms of the tables."""
    rows_f = [(D.shape_of(c), c.dtype) for c in D.FWD_CASES + D.FWD_BASE]
    rows_w = [(D.shape_of(c), c.dtype) for c in D.WGRAD_CASES]
    extra = [(s, dt) for dt in ALL_DT for s in [k for k, _ in KNOWN_FWD] + [b for b, _ in BAD_FWD] + list(BAD_WG) + list(HUGE_WG)
             + [(1, 1, 8, 64, 64, 1, 7, 1)]]
    swept = [(s, dt) for dt in ALL_DT for s in _grid(tuple(FWD_GEOMS) + tuple(WG_GEOMS))]
    fwd = {_same_fwd(L, s, dt) for s, dt in swept}
    wg = {_same_wgrad(L, s, dt) for s, dt in swept}
    for s, dt in rows_f + rows_w + extra:
        _same_fwd(L, s, dt)
        _same_wgrad(L, s, dt)
    assert fwd - {None} == {c.arm for c in D.FWD_CASES} and wg - {None} == {c.arm for c in D.WGRAD_CASES}
    for s, name in KNOWN_FWD:
        assert _c_fwd(L, s, D.MV_BF16)[1] == name
    for s in HUGE_WG:                                        # refused by the plan, so before any fill, for fp32 as for 16-bit storage
        for dt in ALL_DT:
            assert _same_wgrad(L, s, dt) is None and L.mv_dconv_wgrad_plan(*s, dt, (ctypes.c_int * 12)()) == D.MV_ERR_UNSUPPORTED
    assert L.mv_dconv_cl_fwd_plan(1, 1, 8, 32, 32, 1, 3, 1, 7, 0, 0, (ctypes.c_int * 12)()) == D.MV_ERR_DTYPE


def test_fused_head_plans_have_256_row_workgroups(L):
    """mv_dconv_cl_fwd_head (dilation 1, no act_save) over the sweep: an accepted plan has 256 output rows per workgroup - the head
    needs the whole 256-channel output tile - and every shape the forward itself takes is otherwise MV_ERR_UNSUPPORTED.  The head adds
    no instantiation of its own."""
    arms, accepted = set(), 0
    for dt in ALL_DT:
        for shape in _grid(((1, 1, 1), (1, 3, 1), (1, 15, 1), (3, 3, 1))):
            rc, name, v = _c_fwd(L, shape, dt, head=1)
            try:
                D.fwd_arm(*shape, dt)
            except D.Refused as e:
                if e.code == D.MV_ERR_ARG:
                    assert rc == D.MV_ERR_ARG, (shape, dt, rc)
                    continue
            if rc == 0:
                assert v[7] == 256 and shape[4] == 256 and dt != D.MV_F32, (shape, dt, v)
                arms.add(name)
                accepted += 1
            else:
                assert rc == D.MV_ERR_UNSUPPORTED, (shape, dt, rc)
            assert _c_fwd(L, shape, dt, head=1, save=1)[0] == D.MV_ERR_UNSUPPORTED
    assert accepted and arms <= {c.arm for c in D.FWD_CASES}, arms


def test_every_row_names_the_arm_its_shape_selects():
    for c in D.FWD_CASES + D.FWD_BASE:
        assert D.fwd_arm(*D.shape_of(c), c.dtype).name == c.arm, c
    for c in D.WGRAD_CASES:
        assert D.wgrad_arm(*D.shape_of(c), c.dtype).name == c.arm, c


def test_every_reachable_arm_has_rows_and_ragged_companions():
    """The tables name exactly the arms that a sweep of the dispatchers over valid shapes reaches: 16 forward arms per 16-bit type,
    the six fp32 ones, and for the weight gradient the two 3x3 forms and six 1xk kernels per 16-bit type plus the two fp32 forms."""
    fwd = _sweep(D.fwd_arm, ALL_DT, FWD_GEOMS)
    wg = _sweep(D.wgrad_arm, ALL_DT, WG_GEOMS)
    assert len(fwd) == 2 * 16 + 6 and len(wg) == 2 * 8 + 2
    assert {c.arm for c in D.FWD_BASE} == {c.arm for c in D.FWD_CASES} == fwd
    assert {c.arm for c in D.WGRAD_CASES} == wg
    for cases, arm_fn, tile in ((D.FWD_CASES, D.fwd_arm, lambda a: a.npos), (D.WGRAD_CASES, D.wgrad_arm, lambda a: a.wt)):
        for arm in {c.arm for c in cases}:
            rows = [c for c in cases if c.arm == arm]
            assert len({c.W for c in rows}) >= 2, arm      # (the forward arms that need 256 workgroups keep their B x H; the others vary it)
            assert any(c.W % tile(arm_fn(*D.shape_of(c), c.dtype)) for c in rows), arm            # a partly filled position tile
    assert {c.H for c in D.FWD_CASES} >= {1, 2, 11} and {c.B for c in D.FWD_CASES} >= {1, 3}
    for arm in {c.arm for c in D.WGRAD_CASES}:              # every weight-gradient arm: the whole ragged list
        rows = [c for c in D.WGRAD_CASES if c.arm == arm]
        tile = D.wgrad_arm(*D.shape_of(rows[0]), rows[0].dtype).wt
        assert {c.W for c in rows} >= {1, 127, 128, 129, tile + 1} and {c.H for c in rows} >= {1, 2, 11} and {c.B for c in rows} >= {1, 3}, arm
    # the dilations the issue asks for: 1, 3, 5 and the largest with (k - 1) * dil <= 64
    for k, top in ((3, 32), (5, 16), (7, 10), (11, 6), (15, 4)):
        dils = {c.dil for c in D.WGRAD_CASES if c.arm == f"dconv_wgrad_kernel<bf16,1,{k},128>"}
        assert {d for d in (1, 3, 5) if (k - 1) * d <= 64} | {top} <= dils, (k, dils)
        assert (k - 1) * top <= 64 < (k - 1) * (top + 1)
    assert {c.Cin for c in D.WGRAD_CASES} >= {24, 40, 72} and {c.Cout for c in D.WGRAD_CASES} >= {24, 40, 72}


def test_dispatcher_restatement_known_answers():
    """The training shapes of the two discriminator families (B = 64 clips of 8192 samples) against the arms their profiles show."""
    bf = D.MV_BF16
    assert len(KNOWN_FWD) == 5
    for shape, name in KNOWN_FWD:
        assert D.fwd_arm(*shape, bf).name == name
    assert D.lds_row_stride(128, 2) == 160 and D.lds_row_stride(256, 2) == 288 and D.lds_row_stride(64, 2) == 96
    assert len(BAD_FWD) == 3 and len(BAD_WG) == 3
    for bad, code in BAD_FWD:
        with pytest.raises(D.Refused) as e:
            D.fwd_arm(*bad, bf)
        assert e.value.code == code
    for bad in BAD_WG + HUGE_WG:
        with pytest.raises(D.Refused) as e:
            D.wgrad_arm(*bad, bf)
        assert e.value.code == D.MV_ERR_UNSUPPORTED
    with pytest.raises(D.Refused):
        D.wgrad_arm(1, 1, 8, 64, 64, 1, 7, 1, D.MV_F32)


def test_weight_gradient_rows_split_raggedly_and_deeply():
    """Every weight-gradient kernel has a row whose workgroups own 2 chunks with a short last workgroup and a sample boundary inside one,
    and a deep one: 9 or more chunks for the 3x3 kernel (its ring of 8 row slots wraps), 3 or more for the double-buffered kernels."""
    for arm in {c.arm for c in D.WGRAD_CASES}:
        splits = {D.wgrad_split(c) for c in D.WGRAD_CASES if c.arm == arm}
        deep = 9 if "wgrad3" in arm else 3
        assert any(cpw >= deep and ragged for cpw, ragged in splits), (arm, splits)
        if "wgrad3" in arm or ",1,15," in arm or ",1,3," in arm or "float" in arm:
            assert (2, True) in splits, (arm, splits)


def test_sparse_generator_counts_and_covers_every_channel():
    for C in (32, 96, 256):
        x = D.sparse_signs((3, 2, 131), C, 5)
        assert x.shape == (3, 2, 131, C) and set(x.unique().tolist()) == {-1.0, 0.0, 1.0}
        assert torch.equal((x != 0).sum(-1), torch.full((3, 2, 131), 8))
        assert bool(((x != 0).sum((0, 1, 2)) > 0).all())
    s = D.signed_zero_save((4, 64), 1)
    zeros = s[s == 0]
    assert bool(torch.signbit(zeros).any()) and bool((~torch.signbit(zeros)).any()) and bool((s < 0).any()) and bool((s > 0).any())


def _exact16(t):
    return all(torch.equal(t.to(dt).double(), t) for dt in (torch.bfloat16, torch.float16))


def test_forward_references_are_exact_in_both_16_bit_types():
    """For every row: 8 non-zero input channels per position, and the reference of every form the GPU test compares (with and without
    bias, with and without LeakyReLU(0.5), the act_save data gradient) survives bf16 and fp16 unchanged."""
    for shape in FWD_SHAPES:
        x, w, b, ref = D.fwd_reference(shape)
        assert torch.equal((x != 0).sum(-1), torch.full(x.shape[:3], 8)), shape
        assert float(w.abs().max()) <= 2 and float(b.abs().max()) <= 3 and float((ref + b).abs().max()) <= 8 * shape[5] * shape[6] * 2 + 3
        for r in (ref, ref + b):
            assert _exact16(r) and _exact16(D.lrelu(r, D.SLOPE)), shape
        g, wl, save, gref = D.dgrad_reference(shape)
        assert torch.equal((g != 0).sum(-1), torch.full(g.shape[:3], 8)) and _exact16(gref) and _exact16(save), shape
        assert _exact16(x) and _exact16(w) and _exact16(b)
    D.fwd_reference.cache_clear()
    D.dgrad_reference.cache_clear()


def test_weight_gradient_inputs_are_signs_and_sums_stay_exact_in_fp32():
    for shape in WG_SHAPES:
        B, H, W = shape[:3]
        assert B * H * W < 2 ** 24, shape                    # every |sum| <= the number of positions: an exact fp32 integer
        x, g = D.wgrad_inputs(D.Case("", *shape, 0))
        assert set(x.unique().tolist()) <= {-1.0, 0.0, 1.0} and set(g.unique().tolist()) <= {-1.0, 0.0, 1.0}


def test_impulse_expectations_equal_the_convolution():
    """The index formulas of the impulse tests against the fp64 convolution they stand for, on a dilated ragged shape."""
    c = D.Case("", 2, 3, 9, 32, 16, 3, 3, 2, D.MV_BF16)
    _, w, _ = D.fwd_inputs(c)
    for pt in ((0, 0, 0, 0), (1, 2, 8, 31), (1, 1, 4, 7)):
        x = torch.zeros(c.B, c.H, c.W, c.Cin, dtype=torch.float64)
        x[pt] = 1.0
        assert torch.equal(D.fwd_impulse_expected(c, w, pt), D.conv_ref(x, w, None, c.dil))
    xs, _ = D.wgrad_inputs(c)
    for pt in ((0, 0, 0, 0), (1, 2, 8, 15), (1, 1, 4, 7)):
        g = torch.zeros(c.B, c.H, c.W, c.Cout, dtype=torch.float64)
        g[pt] = 1.0
        assert torch.equal(D.wgrad_impulse_expected(c, xs, pt), D.wgrad_ref(xs, g, c.kh, c.kw, c.dil)[0])
    sc = D.ints((2, 3, 5), -3, 3, 9)
    for kh, kw in ((3, 3), (1, 15), (5, 1)):
        t0, t1 = D.tap_matrix_ref(sc, kh, kw, 0), D.tap_matrix_ref(sc, kh, kw, 1)
        assert torch.equal(t0[..., kh * kw // 2], sc) and torch.equal(t1[..., kh * kw // 2], sc)
        assert float(t0[..., kh * kw:].abs().max() if kh * kw < 16 else 0) == 0
        assert torch.equal(t0[..., :kh * kw].flip(-1), t1[..., :kh * kw])          # pos - off(tap) is pos + off(mirrored tap)
