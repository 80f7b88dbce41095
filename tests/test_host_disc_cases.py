"""Host checks of tests/disc_cases.py (no GPU): the tables name the arm the dispatcher restatement selects, every reachable arm has a
row, the ragged-split rows really split raggedly, and - what keeps the exact GPU tests exact - the fp64 reference of every row's
generated inputs is unchanged by a round trip through bf16 and fp16, with exactly 8 non-zero channels per input position."""
import pytest
import torch

import disc_cases as D

FWD_SHAPES = sorted({D.shape_of(c) for c in D.FWD_CASES})
WG_SHAPES = sorted({D.shape_of(c) for c in D.WGRAD_CASES})

def _sweep(arm_fn, dtypes, geoms):
    """Every arm name the dispatcher restatement returns over a grid of valid shapes."""
    names = set()
    for dt in dtypes:
        for B, H in ((1, 1), (1, 2), (12, 11), (24, 11)):
            for W in (5, 130, 300):
                for Cin in (24, 32, 64, 96, 128, 192, 256):
                    for Cout in (16, 32, 64, 128, 160, 192, 256, 384):
                        for kh, kw, dil in geoms:
                            try:
                                names.add(arm_fn(B, H, W, Cin, Cout, kh, kw, dil, dt).name)
                            except D.Refused:
                                pass
    return names


def test_every_row_names_the_arm_its_shape_selects():
    for c in D.FWD_CASES + D.FWD_BASE:
        assert D.fwd_arm(*D.shape_of(c), c.dtype).name == c.arm, c
    for c in D.WGRAD_CASES:
        assert D.wgrad_arm(*D.shape_of(c), c.dtype).name == c.arm, c


def test_every_reachable_arm_has_rows_and_ragged_companions():
    """The tables name exactly the arms that a sweep of the dispatchers over valid shapes reaches: 16 forward arms per 16-bit type,
    the six fp32 ones, and for the weight gradient the two 3x3 forms and six 1xk kernels per 16-bit type plus the two fp32 forms."""
    all_dt = (D.MV_BF16, D.MV_F16, D.MV_F32)
    fwd = _sweep(D.fwd_arm, all_dt, ((1, 1, 1), (1, 3, 1), (1, 15, 1), (3, 3, 1), (3, 3, 2), (3, 3, 58)))
    wg = _sweep(D.wgrad_arm, all_dt, [(3, 3, 1)] + [(1, k, d) for k in (1, 3, 5, 7, 9, 11, 15) for d in (1, 4, 5)])
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
    assert D.fwd_arm(64, 2, 4096, 128, 256, 3, 3, 1, bf).name == "dconv_cl_wide_kernel<bf16,1,4,8,64,4>"
    assert D.fwd_arm(64, 2, 4096, 256, 128, 3, 3, 1, bf).name == "dconv_cl_wide_kernel<bf16,1,4,8,32,2>"
    assert D.fwd_arm(64, 1, 8192, 128, 256, 1, 15, 1, bf).name == "dconv_cl_kernel<bf16,4,4,8>"
    assert D.fwd_arm(64, 1, 8192, 256, 128, 1, 15, 1, bf).name == "dconv_cl_wide_kernel<bf16,2,2,4,128,8>"
    assert D.fwd_arm(64, 1, 8192, 64, 32, 1, 15, 1, bf).name == "dconv_cl_wide_kernel<bf16,4,1,2,64,8>"
    assert D.lds_row_stride(128, 2) == 160 and D.lds_row_stride(256, 2) == 288 and D.lds_row_stride(64, 2) == 96
    for bad, code in (((1, 1, 8, 48, 32, 1, 3, 1), D.MV_ERR_ARG), ((1, 1, 8, 32, 32, 1, 4, 1), D.MV_ERR_ARG),
                      ((1, 1, 8, 32, 32, 1, 3, 65), D.MV_ERR_ARG)):
        with pytest.raises(D.Refused) as e:
            D.fwd_arm(*bad, bf)
        assert e.value.code == code
    for bad in ((1, 2, 8, 64, 64, 3, 3, 2), (1, 1, 8, 64, 64, 1, 15, 5), (1, 1, 8, 64, 64, 1, 9, 1)):
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
