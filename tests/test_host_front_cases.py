"""Host checks of tests/front_cases.py (no GPU).  Every row the GPU file compares bit for bit is proven exact in fp32 in any order
(sum|terms| < 2^24 in units of its granularity, the value itself an fp32 number) and every 16-bit expectation is shown to be the RNE
rounding of that value by an independent bit-level rounding; every other row carries a counted k and a measured function term below
the 2^-19 limit, its pre-activation exact and inside the measured argument range; the case tables reach every arm of
csrc/norm_elem.hip and csrc/conv_generic.hip, asserted through the restated dispatcher rules; the restated references reproduce the
committed goldens of the reference project at the goldens' own tolerance; and two corrupted elements show what a norm cannot see."""
import itertools

import numpy as np
import pytest
import torch

import front_cases as F
from conftest import load_golden
from front_cases import ACT_LRELU, ACT_NONE, ACT_SILU, ACT_TANH, MV_BF16, MV_F16, MV_F32

TOL = 1e-5              # tests/test_oracle_vs_golden.py: fp64 / fp32 restatement against the fp32 reference


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _all_outputs():
    """(label, Out, pre-activation Out or None, act) of every reference the GPU file compares with."""
    for c in F.CONV1D_CASES:
        r = F.conv1d_reference(c)
        yield f"conv1d {c.name}", r["y"], r["pre"], c.act
    for c in F.CONVT_CASES:
        r = F.convT_reference(c)
        yield f"convT {c.name}", r["y"], r["pre"], c.act
    for c in F.CONV2D_CASES:
        r = F.conv2d_reference(c)
        yield f"conv2d {c.name}", r["y"], r["pre"], c.act
    for c in F.GN_APPLY_CASES:
        r = F.gn_apply_reference(c)
        yield f"gn apply {c.name}", r["y"], r["pre"], c.act
    for a in F.ACT_CASES:
        r = F.act_reference(*a)
        yield f"act {a}", r["y"], r["pre"], a[1]
    for c, dt in itertools.product(F.GN_STATS_CASES, F.ALL_DT):
        r = F.gn_stats_reference(c, dt)
        yield f"gn stats {c.name} mean", r["mean"], None, ACT_NONE
        yield f"gn stats {c.name} sumsq", r["sumsq"], None, ACT_NONE
    for a in F.FILM_CASES:
        yield f"film {a}", F.film_reference(*a)["y"], None, ACT_NONE
    for a in F.SCALE_SHIFT_CASES:
        yield f"scale_shift {a}", F.scale_shift_reference(*a)["y"], None, ACT_NONE
    for a in F.AVGPOOL_CASES:
        yield f"avgpool {a}", F.avgpool_reference(*a)["y"], None, ACT_NONE
    for a in F.MPD_CASES:
        yield f"mpd {a}", F.mpd_reference(*a)["y"], None, ACT_NONE
    for a in F.LINEAR_CASES:
        r = F.linear_reference(*a)
        yield f"linear {a}", r["y"], None, ACT_NONE
        yield f"linear {a} nobias", r["y_nobias"], None, ACT_NONE
    for c in F.ATTN_CASES:
        r = F.attn_reference(c)
        if r["pooled"].k == 0:
            yield f"attn {c.name} pooled", r["pooled"], None, ACT_NONE
            yield f"attn {c.name} logits", r["logit"], None, ACT_NONE
    for c in F.PROLOGUE_CASES:
        r = F.prologue_reference(c)
        yield f"prologue {c.name} x_cl", r["x_cl"], None, ACT_NONE
        yield f"prologue {c.name} proj", r["proj"], None, ACT_NONE
        if r["logit"] is not None:
            yield f"prologue {c.name} logits", r["logit"], None, ACT_NONE
    for a in F.GRC_CASES:
        r = F.grc_fold_reference(*a)[1]
        yield f"grc {a} w_eff", r["w_eff"], None, ACT_NONE
        yield f"grc {a} b_eff", r["b_eff"], None, ACT_NONE


def test_every_row_is_exact_or_carries_a_bound():
    """k == 0: bit equality is fair.  k > 0: only behind tanh / SiLU, with k = 2, an exact pre-activation inside the measured range."""
    n_exact = n_bound = 0
    for label, o, pre, act in _all_outputs():
        assert o.ref.dtype == torch.float64 and o.ref.shape == o.abs_sum.shape, label
        assert bool((o.abs_sum + 1e-12 >= o.ref.abs()).all()), label
        if o.k == 0:
            assert F.proves_exact(o), (label, float((o.abs_sum / o.unit).max()))
            assert torch.equal(o.ref.float().double(), o.ref), label          # an fp32 number: torch's conversion to 16 bits rounds once
            n_exact += 1
        else:
            assert act in F.ACT_FN and o.k == 2 and F.proves_exact(pre), label
            assert float(pre.ref.abs().max()) <= F.FN_ARG_MAX, (label, float(pre.ref.abs().max()))
            n_bound += 1
    assert n_exact > 200 and 0 < n_bound < n_exact / 8, (n_exact, n_bound)
    assert all(0 < e < F.E_FN_LIMIT for e in F.E_FN.values()) and set(F.E_FN) == {"rsqrt", "exp", "tanh", "silu"}


def _rne_bf16(v):
    """fp64 tensor of fp32 numbers -> bf16 by integer arithmetic on the fp32 bits: add 0x7FFF + the kept part's last bit, truncate."""
    b = v.float().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return (b & 0xFFFFFFFF).to(torch.int64).apply_(lambda t: t - (1 << 32) if t >= (1 << 31) else t).to(torch.int32).view(torch.float32).double()


def test_sixteen_bit_expectations_are_the_rne_rounding_of_the_exact_value():
    """`stored` (torch's conversion of the fp64 reference) against two independent roundings: integer arithmetic on the bits for bf16,
    numpy's float16 for fp16 - over every exact row that needs rounding at all, and there must be such rows."""
    rounded = {MV_BF16: 0, MV_F16: 0}
    for label, o, _, _ in _all_outputs():
        if o.k or o.ref.numel() > 300000:
            continue
        with np.errstate(over="ignore"):                            # sums of squares pass the fp16 range: infinity in both roundings
            half = torch.from_numpy(o.ref.numpy().astype(np.float32).astype(np.float16).astype(np.float64))
        want = {MV_BF16: _rne_bf16(o.ref), MV_F16: half}
        for dt in (MV_BF16, MV_F16):
            assert torch.equal(F.stored(o, dt), want[dt]), (label, dt)
            rounded[dt] += int((want[dt] != o.ref).sum())
    assert rounded[MV_BF16] > 1000 and rounded[MV_F16] > 100, rounded
    ties = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 257.0, 259.0], dtype=torch.float64)
    assert _rne_bf16(ties).tolist() == [1.0, 1.0 + 2.0 ** -6, -1.0, 256.0, 260.0]


def test_inputs_are_small_integers_dyadic_scalars_and_sixteen_bit_numbers():
    for c in F.CONV1D_CASES:
        r = F.conv1d_reference(c)
        assert float(r["x"].abs().max()) <= 4 and float(r["w"].abs().max()) <= 3 and bool((r["x"] == r["x"].round()).all())
        if r["alpha"] is not None and c.K > 1:
            a = r["alpha"]
            assert bool(((a * 8) == (a * 8).round()).all()) and bool((a.sum(1) == 1).all()) and bool((a >= 0).all())
        if c.a1:
            assert bool((r["alpha"] != 1).all())
    for c, dt in itertools.product(F.GN_STATS_CASES, F.ALL_DT):
        x = F.gn_stats_reference(c, dt)["x"]
        assert torch.equal(x.to(F.TORCH_DT[dt]).double(), x), (c.name, dt)               # the offset-heavy values fit the type
    for c in F.GN_APPLY_CASES:
        r = F.gn_apply_reference(c)
        assert bool((r["mean"] == r["mean"].round()).all()) and bool((torch.log2(r["rstd"]) == torch.log2(r["rstd"]).round()).all())
        if c.mask:
            m = r["mask"].view(-1, c.T)
            lanes = [m[:, l::8] for l in range(min(8, c.T))]
            assert all(bool((l == 0).any()) and bool((l != 0).any()) for l in lanes), c.name   # zeros and keeps in every byte lane of both words
            assert set(m.unique().tolist()) == {0, 1, 2, 128, 255}
    assert F.SLOPE == 0.25 and F.MASK_SCALE == 2.0


# ----------------------------------------------------------------------------------------------- arms: the generic convolutions
def _plan1(c):
    return F.conv1d_plan(c.B, c.Cin, c.Tin, c.Cout, c.Tout, c.ks, c.stride, c.pad, c.dil, c.groups, c.K)


def test_conv1d_rows_reach_every_arm():
    cs = F.CONV1D_CASES
    assert {c.Tout for c in cs} >= {1, 127, 128, 129, 130}
    assert {c.Cout // c.groups for c in cs} >= {1, 3, 6, 32, 35} and {c.Cin // c.groups for c in cs} >= {1, 3, 8, 9}
    assert {c.groups for c in cs} >= {1, 2} and any(c.groups == c.Cin > 1 for c in cs)
    assert {c.stride for c in cs} >= {1, 2, 4} and {c.dil for c in cs} >= {1, 3} and {c.ks for c in cs} >= {1, 3, 7}
    assert any(c.pad == 0 and c.ks > 1 for c in cs) and any(c.pad == (c.ks - 1) * c.dil // 2 > 0 for c in cs) and any(c.pad > (c.ks - 1) * c.dil for c in cs)
    assert any(c.K == 1 and not c.a1 for c in cs) and any(c.K == 1 and c.a1 and c.bias for c in cs)
    assert {(c.K, c.bias) for c in cs} >= {(4, True), (4, False), (8, True), (8, False)}
    assert any(c.res and c.yoff for c in cs) and any(c.res and not c.yoff for c in cs) and any(c.xs for c in cs)
    assert {c.act for c in cs} == {ACT_NONE, ACT_LRELU, ACT_TANH, ACT_SILU}
    assert any((c.Tin + 2 * c.pad - c.dil * (c.ks - 1) - 1) % c.stride for c in cs)            # the floor of the length rule drops a remainder
    plans = {c.name: _plan1(c) for c in cs}
    assert [n for n, p in plans.items() if p[1]] == ["lds-70592"] and plans["lds-70592"][0] == 70592 > 64 * 1024
    assert plans["base-k4-lrelu"][2] == (2, 2, 2) and plans["g2-cout35-s2-k4-nobias"][2] == (2, 4, 2)
    # a residual row whose x strides differ from y's: reading the residual through x's strides would show
    for c in cs:
        if c.res:
            assert (c.Cin * c.Tin, c.Tin) != (c.Cout * c.Tout, c.Tout)
    for name, shape, has_alpha, code in F.CONV1D_REFUSED:
        with pytest.raises(F.Refused) as e:
            F.conv1d_plan(*shape, alpha=has_alpha)
        assert e.value.code == code, name
    assert F.conv_lds(127 + 159 + 1, 160) > 160 * 1024
    assert {r[0] for r in F.CONV1D_REFUSED} >= {"ks160-lds", "tout+1", "tout-1", "nbanks9", "nbanks2-null-alpha", "cin%groups", "B65536"}


def test_conv_transpose_rows_reach_every_arm_and_no_term_is_skipped():
    cs = F.CONVT_CASES
    assert {(c.stride, c.ks) for c in cs} >= {(1, 3), (2, 4), (2, 7), (3, 6), (4, 8), (8, 16)}
    for s in (2, 3, 4, 8):
        assert {c.opad for c in cs if c.stride == s} >= {0, s - 1}
    assert any(c.pad == 0 for c in cs) and any(c.pad == (c.ks - c.stride) // 2 > 0 for c in cs) and {c.dil for c in cs} == {1, 2}
    assert any(128 < c.Tout <= 256 for c in cs) and any(c.Tout > 256 for c in cs)
    assert {c.Cin for c in cs} == {3, 9} and {c.Cout for c in cs} == {5, 33}
    assert {(c.K, c.bias) for c in cs} >= {(1, True), (4, True), (4, False), (8, True), (8, False)} and any(c.a1 for c in cs)
    for c in cs:
        lds, xw, grid = F.convT_plan(c.B, c.Cin, c.Tin, c.Cout, c.Tout, c.ks, c.stride, c.pad, c.dil, c.K)
        assert F.convT_window_is_wide_enough(c.Tout, c.ks, c.stride, c.pad, c.dil, xw), c.name
        assert c.pad < (c.ks - 1) * c.dil                                  # tile 0 starts with negative numerators
    # the staging window is wide enough at any geometry, not only at the rows'
    for stride, ks, dil, pad in itertools.product(range(1, 10), range(1, 20), (1, 2, 3), (0, 1, 5)):
        assert F.convT_window_is_wide_enough(700, ks, stride, pad, dil, (F.TT - 1 + (ks - 1) * dil) // stride + 2)
    for name, shape, has_alpha, code in F.CONVT_REFUSED:
        with pytest.raises(F.Refused) as e:
            F.convT_plan(*shape, alpha=has_alpha)
        assert e.value.code == code, name


def test_conv2d_rows_reach_every_arm():
    cs = F.CONV2D_CASES
    assert {(c.kh, c.kw) for c in cs} >= {(5, 1), (3, 1), (3, 3), (1, 1)}
    for k in ((5, 1), (3, 1), (3, 3)):
        assert {(c.ph, c.pw) for c in cs if (c.kh, c.kw) == k} >= {(k[0] // 2, k[1] // 2), (0, 0)}
    assert {c.W for c in cs} >= {2, 3, 11} and any(c.W + 2 * c.pw - c.kw + 1 == 130 for c in cs)
    assert {c.Cin for c in cs} == {1, 9} and {c.Cout for c in cs} >= {1, 32, 33}
    big = next(c for c in cs if c.name == "rows-65535")
    assert F.conv2d_plan(big.B, big.Cin, big.H, big.W, big.Cout, big.kh, big.kw, big.ph, big.pw)[1][2] == 65535 and (big.Cin, big.Cout, big.W) == (1, 1, 2)
    for name, shape, code in F.CONV2D_REFUSED:
        with pytest.raises(F.Refused) as e:
            F.conv2d_plan(*shape)
        assert e.value.code == code, name


# ----------------------------------------------------------------------------------------------- arms: GroupNorm
def test_groupnorm_rows_reach_every_arm():
    st = {c.name: c for c in F.GN_STATS_CASES}
    vec = {n: F.gn_vec(MV_BF16, c.T, (c.lay,), c.C) for n, c in st.items()}
    assert all(vec[n] == n.startswith("vec") for n in st if not n.startswith("offset")), vec
    assert vec["offset-heavy"] and not vec["offset-heavy-scalar"]
    assert not any(F.gn_vec(MV_F32, c.T, (c.lay,), c.C) for c in st.values())                  # fp32 always takes the scalar arm
    assert {c.T for c in st.values() if vec[c.name]} >= {8, 16, 2056} and 2056 > 256 * 8
    assert {c.T for c in st.values()} >= {7, 9} and {c.C // c.G for c in st.values()} >= {1, 8}
    assert any(c.G == 1 for c in st.values()) and any(c.G == c.C for c in st.values())
    assert (st["scalar-base+8B"].lay.off * 2) % 16 == 8
    ap = {c.name: c for c in F.GN_APPLY_CASES}
    for n, c in ap.items():
        v = F.gn_vec(MV_BF16, c.T, (c.x, c.r, c.y), c.C, c.moff)
        if n.startswith("vec") or n.startswith("scalar"):
            assert v == n.startswith("vec"), n
        assert not F.gn_vec(MV_F32, c.T, (c.x, c.r, c.y), c.C, c.moff)
    # each scalar row has exactly one cause: restoring that one term gives the vector arm back
    one_cause = dict([("scalar-x-base", "x"), ("scalar-y-base", "y"), ("scalar-res-base", "r"), ("scalar-x_cs", "x"), ("scalar-x_bs", "x"),
                      ("scalar-y_cs", "y"), ("scalar-y_bs", "y"), ("scalar-r_cs", "r"), ("scalar-r_bs", "r")])
    for n, field in one_cause.items():
        c = ap[n]._replace(**{field: F.DENSE})
        assert F.gn_vec(MV_F16, c.T, (c.x, c.r, c.y), c.C, c.moff), n
        assert sum(v != 0 for v in getattr(ap[n], field)) == 1, n
    for n in ("scalar-mask+4B", "scalar-mask+1B"):
        c = ap[n]
        assert c.T % 8 == 0 and (c.x, c.y) == (F.DENSE, F.DENSE) and c.moff % 8 and F.gn_vec(MV_F16, c.T, (c.x, c.r, c.y), c.C, 0)
    assert {ap["scalar-mask+4B"].moff, ap["scalar-mask+1B"].moff} == {4, 1} and ap["vec-mask+8B"].moff == 8
    assert {c.act for c in ap.values()} == {ACT_NONE, ACT_LRELU, ACT_TANH, ACT_SILU}
    assert any(not c.gw for c in ap.values()) and any(not c.gb for c in ap.values()) and any(not c.res for c in ap.values()) and any(not c.mask for c in ap.values())
    c = ap["scalar-res-strided-misaligned"]
    assert c.r.off % 8 and c.r.cs and c.r.bs
    # the capped grid (64 workgroups of 256 threads) is passed: the grid-stride loops iterate
    c = ap["scalar-t16400-grid-stride"]
    assert F.gn_apply_grid(MV_BF16, c.T, (c.x, c.r, c.y), c.C, c.B, c.moff) == (64, 2) and c.T == 16400 > 64 * 256
    c = ap["vec-t131080-grid-stride"]
    assert F.gn_apply_grid(MV_BF16, c.T, (c.x, c.r, c.y), c.C, c.B, c.moff) == (64, 2) and c.T // 8 > 64 * 256 and c.B * c.C == 2
    assert F.gn_apply_grid(MV_F32, c.T, (c.x, c.r, c.y), c.C, c.B, c.moff) == (64, 2)


# ----------------------------------------------------------------------------------------------- arms: elementwise, fold, linear
def test_elementwise_rows_reach_every_arm():
    assert {(C > Fd) - (C < Fd) for _, C, Fd, _ in F.FILM_CASES} == {-1, 0, 1} and any(T > 64 * 256 for *_, T in F.FILM_CASES)
    assert F.CAP_N == 2048 * 256 + 3 and any(n == F.CAP_N for n, _, _ in F.ACT_CASES) and any(n == 1 for n, _, _ in F.ACT_CASES)
    assert {a for _, a, _ in F.ACT_CASES} == {ACT_NONE, ACT_LRELU, ACT_TANH, ACT_SILU} and {r for _, _, r in F.ACT_CASES} == {True, False}
    assert {s for _, _, s in F.AVGPOOL_CASES} == {1, 2, 4} and all(any(T % s for _, T, s2 in F.AVGPOOL_CASES if s2 == s) for s in (2, 4))
    assert max(r for r, _, _ in F.AVGPOOL_CASES) == 65535 and any(T // s > 64 * 256 for _, T, s in F.AVGPOOL_CASES)
    for P in (2, 3, 5, 7, 11):
        rem = {T % P for _, p, T in F.MPD_CASES if p == P}
        assert rem >= {0, 1, P - 1}, (P, rem)
    assert max(r for r, _, _ in F.MPD_CASES) == 65535 and any(T > 64 * 256 for _, _, T in F.MPD_CASES)
    assert {Kd for _, _, Kd in F.LINEAR_CASES} >= {1, 63, 64, 65, 130} and {M * N for M, N, _ in F.LINEAR_CASES} >= {1, 5, 8}
    sp = F.cast_specials()
    assert bool(torch.isnan(sp).any()) and bool(torch.isinf(sp).any()) and bool((sp == 0).sum() == 2) and bool(torch.signbit(sp[sp == 0]).any())
    bf, hf = sp.to(torch.bfloat16).float(), sp.to(torch.float16).float()
    fin = torch.isfinite(sp)
    assert bool((torch.isinf(bf) & fin).any()) and bool((torch.isinf(hf) & fin).any())                 # overflow to infinity in both types
    assert bool(((bf > sp) & fin).any()) and bool(((bf < sp) & fin).any()) and bool(((hf > sp) & fin).any()) and bool(((hf < sp) & fin).any())
    assert float(hf[sp == 65504.0]) == 65504.0 and bool(((hf != 0) & (hf.abs() < 2.0 ** -14)).any())     # largest finite, subnormals


def test_transpose_rows_reach_both_kernels_for_every_entry():
    entries = ("nct_to_ntc", "ntc_to_nct", "nct_to_ntc_pad", "ntc_to_nct_crop")
    edge = {1, 31, 32, 33, 63, 64, 65, 72}
    assert {C for C, _ in F.TR_SHAPES} >= edge and {T for _, T in F.TR_SHAPES} >= edge
    kernels = {e: set() for e in entries}
    for e, (C, T), dt in itertools.product(entries, F.TR_SHAPES, F.ALL_DT):
        for Cpad in (C + 5, C):
            k, grid = F.transpose_plan(e, 3, C, T, Cpad, dt)
            kernels[e].add(k)
            assert dt != MV_F32 or k == "32"
    for e, C, T, Cpad, xoff, yoff, broken in F.TR_FAST:
        k, grid = F.transpose_plan(e, 3, C, T, Cpad, MV_BF16, xoff, yoff)
        assert (k == "16") == (broken is None), (e, C, T, Cpad, broken)
        kernels[e].add(k)
        if broken is not None:                                       # one term alone: the row's terms, one mended, give the fast path
            R, Cn, ldx, ldy, x_bs, y_bs = F.transpose_geometry(e, 3, C, T, Cpad)
            terms = {"Cn": Cn % 8, "ldx": ldx % 8, "ldy": ldy % 8, "x base": xoff % 8, "y base": yoff % 8}
            assert terms[broken] and (broken in ("Cn", "ldx", "ldy") or not any(v for n, v in terms.items() if n != broken)), (e, broken, terms)
    assert all(kernels[e] == {"16", "32"} for e in entries), kernels
    assert {r[6] for r in F.TR_FAST} >= {None, "Cn", "ldx", "ldy", "x base", "y base"}
    # padded channels exist and are zeros in the reference; cropped columns exist and are absent from it
    x = F.distinct_bits((3, 60, 72), MV_F32)
    y = F.transpose_reference("nct_to_ntc_pad", x, 3, 60, 72, 64)
    assert y.shape == (3, 72, 64) and bool((y[:, :, 60:] == 0).all()) and bool((y[:, :, :60] != 0).all()) and y[1, 5, 7] == x[1, 7, 5]
    x = F.distinct_bits((3, 72, 64), MV_F32)
    y = F.transpose_reference("ntc_to_nct_crop", x, 3, 60, 72, 64)
    assert y.shape == (3, 60, 72) and not set(x[:, :, 60:].reshape(-1).tolist()) & set(y.reshape(-1).tolist())
    for dt in (MV_BF16, MV_F16):
        b = F.distinct_bits((3, 65, 136), dt)
        assert b.view(torch.int16).unique().numel() == b.numel() and bool(torch.isfinite(b.float()).all()) and bool((b.float() != 0).all())


# ----------------------------------------------------------------------------------------------- arms: attention, prologue, fold
def test_attention_rows_reach_every_arm():
    cs = {c.name: c for c in F.ATTN_CASES}
    plan = {n: F.attn_plan(c.B, c.C, c.T, c.K, c.pooled, MV_BF16, c.xoff) for n, c in cs.items()}
    assert all((plan[n][0] == "two") == n.startswith("two") for n in cs), plan
    assert cs["one-below-threshold"].C * cs["one-below-threshold"].T == 16128 < 16384 == cs["two-at-threshold"].C * cs["two-at-threshold"].T
    assert cs["one-c64-t255"].C * 255 == 16320 and not cs["one-null-pooled-above"].pooled and cs["one-null-pooled-above"].C * cs["one-null-pooled-above"].T >= 16384
    assert plan["two-at-threshold"][1] and not plan["two-scalar-t253"][1] and not plan["two-scalar-misaligned"][1]
    assert cs["two-scalar-t253"].T % 8 and cs["two-scalar-t253"].T % 4 and cs["two-scalar-misaligned"].T % 8 == 0       # one cause each, in every type
    for dt in F.ALL_DT:
        assert not F.attn_plan(3, 65, 253, 4, True, dt)[1] and not F.attn_plan(3, 65, 256, 4, True, dt, 1)[1] and F.attn_plan(3, 65, 256, 4, True, dt)[1]
    assert (cs["two-scalar-t253"].B * cs["two-scalar-t253"].C) % 4
    assert {c.K for c in cs.values()} >= {1, 4, 64} and any(not c.bias for c in cs.values())
    with pytest.raises(F.Refused):
        F.attn_plan(2, 1, 1, 65, True, MV_F32)
    for n in ("one-rail", "two-rail"):
        r = F.attn_reference(cs[n])
        lg = r["logit"].ref
        assert float(lg.max()) > 60 and float(lg.min()) < -60 and float((lg.max(1).values - lg.min(1).values).min()) > 100   # exp without the maximum overflows
    pow2 = [c for c in cs.values() if c.T & (c.T - 1) == 0]
    assert all(F.attn_reference(c)["pooled"].k == 0 for c in pow2) and len(pow2) >= 10


def test_prologue_rows_reach_every_arm_one_argument_from_the_base():
    base = F.PROLOGUE_CASES[0]
    plans = {c.name: F.prologue_plan(c) for c in F.PROLOGUE_CASES}
    assert plans["base"] == dict(lds=plans["base"]["lds"], grid=3 + 2, roles=2, mel="reg", logits="reg", film="reg", cat="fit")
    want = {"mel-loop-arm": ("mel", "loop"), "logits-general-k5": ("logits", "general"), "logits-general-c257": ("logits", "general"),
            "film-loop-arm": ("film", "loop"), "cond-truncates-emo": ("cat", "trunc"), "cond-truncates-spk": ("cat", "trunc"),
            "cond-zero-pads": ("cat", "pad"), "no-film": ("roles", 1)}
    for n, (k, v) in want.items():
        assert plans[n][k] == v, (n, plans[n])
    by = {c.name: c for c in F.PROLOGUE_CASES}
    for n, c in by.items():                                          # each row differs from the base in one argument (two where one implies the other)
        diff = [f for f in F.PR._fields[1:] if getattr(c, f) != getattr(base, f) and not (f == "zero_n" and c.zero_n == 5 * c.B + 3)]
        assert len(diff) <= (1 if n not in ("logits-general-c257", "spk-only", "emo-only", "lds-65280", "fp32-inputs-loop-arms", "mel-loop-arm") else 4), (n, diff)
    assert by["film-512-register"].cond == 512 and plans["film-512-register"]["film"] == "reg" and by["film-loop-arm"].cond == 513
    assert by["cond-truncates-spk"].cond < base.ds and base.ds < by["cond-truncates-emo"].cond < base.ds + base.de
    assert {c.B % 8 for c in by.values()} >= {0, 1, 3} and by["B9"].B > 8
    assert {c.F2 % 16 for c in by.values()} >= {0, 1, 8} and {c.zero_n for c in by.values() if c.B == 3} >= {0, 1, 2, 18}
    assert any(c.zero_n % c.B for c in by.values()) and any(c.in32 for c in by.values()) and by["logits-k64"].K == 64
    assert by["mel-loop-arm"].C * by["mel-loop-arm"].T > 4096 >= base.C * base.T
    assert plans["lds-65280"]["lds"] == 65280
    with pytest.raises(F.Refused):
        F.prologue_plan(F._pr("x", C=80, T=192))
    with pytest.raises(F.Refused):
        F.prologue_plan(F._pr("x", C=1025, T=1))
    r = F.prologue_reference(by["fp32-inputs"])
    for dt in (MV_BF16, MV_F16):
        assert not torch.equal(F.stored(r["x_cl"], dt), r["x_cl"].ref)                # the 16-bit store of the fp32 mel really rounds
    assert {n for n, *_ in F.PROLOGUE_REFUSED} >= {"C1025", "lds-65920", "in-bf16-store-f16", "null-spk"}


def test_grc_fold_rows_reach_both_arms_and_the_centre_tap():
    plans = {a: F.grc_fold_plan(*a) for a in F.GRC_CASES}
    assert plans[(64, 64, 3, 4, 16)][:2] == ("lds", 36864) and plans[(64, 64, 3, 1, 16)][:2] == ("global", 73728)
    assert plans[(64, 64, 3, 2, 16)][:2] == ("lds", 48 * 1024)                       # exactly at the split
    assert {a[3] for a in F.GRC_CASES} >= {1, 2, 4} and {a[2] for a in F.GRC_CASES} >= {1, 3, 5} and {a[4] for a in F.GRC_CASES} >= {1, 16}
    assert any(a[0] != a[1] for a in F.GRC_CASES) and {p[0] for p in plans.values()} == {"lds", "global"}
    for a in F.GRC_REFUSED:
        with pytest.raises(F.Refused):
            F.grc_fold_plan(*a)
    # the LoRA term lands on the centre tap alone: without it only that tap changes
    a = (64, 64, 3, 4, 16)
    i, r = F.grc_fold_reference(*a)
    cin_g, cout_g = 16, 16
    comb = torch.zeros(64, 64, 3, dtype=torch.float64)
    for q, c, j in itertools.product(range(64), range(64), range(3)):
        if c // cin_g == q // cout_g:
            comb[q, c, j] = i["conv_w"][q, c - (c // cin_g) * cin_g, j]
    plain = torch.einsum("oq,qcj->ocj", i["proj_w"], comb)
    d = r["w_eff"].ref - plain
    assert bool((d[:, :, 0] == 0).all()) and bool((d[:, :, 2] == 0).all()) and bool((d[:, :, 1] != 0).any())
    assert torch.equal(d[:, :, 1], 0.5 * i["proj_w"] @ (i["A"] @ i["Bm"]).t())


# ----------------------------------------------------------------------------------------------- the references against the goldens
def _sd(g):
    return {k[3:]: torch.from_numpy(v).double() for k, v in g.items() if k.startswith("sd.")}


@pytest.mark.parametrize("name,kw", [("odconv1d_c16_o8_k3_d2", dict(pad=2, dil=2)), ("odconv1d_c80_o32_k7", dict(pad=3)), ("odconv1d_c8_o8_k5_s2", dict(pad=2, stride=2))])
def test_conv1d_reference_against_the_golden(name, kw):
    g = load_golden(name)
    sd, x = _sd(g), torch.from_numpy(g["x.x"]).double()
    alpha = torch.softmax(torch.nn.functional.linear(x.mean(2), sd["kernel_attention.1.weight"][:, :, 0], sd["kernel_attention.1.bias"]), 1)
    assert rel_l2(alpha, torch.from_numpy(g["alpha"])) < TOL
    y = F.conv1d_f64(x, sd["kernels"], sd["bias"], alpha, **kw)
    assert y.shape == g["y"].shape and rel_l2(y, torch.from_numpy(g["y"])) < TOL


@pytest.mark.parametrize("name,kw", [("odconvT_c16_o8_k16_s8", dict(stride=8, pad=4)), ("odconvT_c8_o8_k4_s2", dict(stride=2, pad=1)),
                                     ("odconvT_c8_o8_k8_s4", dict(stride=4, pad=2)), ("odconvT_c8_o4_k6_s3_op1", dict(stride=3, pad=1, opad=1))])
def test_conv_transpose_reference_against_the_golden(name, kw):
    g = load_golden(name)
    sd, x = _sd(g), torch.from_numpy(g["x.x"]).double()
    alpha = torch.softmax(torch.nn.functional.linear(x.mean(2), sd["kernel_attention.1.weight"][:, :, 0], sd["kernel_attention.1.bias"]), 1)
    y = F.convT_f64(x, sd["kernels"], sd["bias"], alpha, **kw)
    assert y.shape == g["y"].shape and rel_l2(y, torch.from_numpy(g["y"])) < TOL


def test_conv1d_and_avgpool_references_against_the_scale_discriminator_golden():
    g = load_golden("disc1d_s2")
    sd, h = _sd(g), F.avgpool_f64(torch.from_numpy(g["x.x"]).double(), 2)
    one = torch.ones(h.shape[0], 1, dtype=torch.float64)
    for li, idx in enumerate((0, 2, 4, 6, 8)):
        h = F.conv1d_f64(h, sd[f"conv_layers.{idx}.weight"][None], sd[f"conv_layers.{idx}.bias"][None], one, pad=7)
        h = F.act64(h, ACT_LRELU, 0.1) if li < 4 else h
    assert h.shape == g["y"].shape and rel_l2(h, torch.from_numpy(g["y"])) < TOL


def test_conv2d_and_fold_references_against_the_period_discriminator_golden():
    g = load_golden("disc2d_P3")
    sd, x = _sd(g), torch.from_numpy(g["x.x"]).double()
    h = F.mpd_f64(x, 3).view(x.shape[0], 1, 3, -1)
    for li, idx in enumerate((0, 2, 4, 6, 8)):
        h = F.conv2d_f64(h, sd[f"conv_layers.{idx}.weight"], sd[f"conv_layers.{idx}.bias"], 1, 1)
        h = F.act64(h, ACT_LRELU, 0.1) if li < 4 else h
    assert h.shape == g["y"].shape and rel_l2(h, torch.from_numpy(g["y"])) < TOL


# ----------------------------------------------------------------------------------------------- why element by element
def test_a_wrong_tile_edge_passes_the_norms_and_fails_the_new_comparison():
    """(a) The base conv1d row with the output at the first step of the second 128-step tile wrong in one channel of one sample: by a
    whole tap (1.0) the rel-L2 stays inside the 5e-3 the module tests ask of fp16, by one bank's LeakyReLU'd share (1/32) inside the
    1e-4 they ask of fp32.  (b) A GroupNorm row whose last 8-element vector ignores
    the dropout mask in one byte lane: inside the 3e-2 asked of bf16.  Neither is equal."""
    c = F.CONV1D_CASES[0]
    r = F.conv1d_reference(c)
    ref = r["y"].ref
    bad = ref.clone()
    bad[0, 33, 128] += 1.0
    assert 0 < rel_l2(bad, ref) < 5e-3 and not torch.equal(bad, ref)
    bad[0, 33, 128] = ref[0, 33, 128] + 1.0 / 32
    assert 0 < rel_l2(bad, ref) < 1e-4 and not torch.equal(bad, ref)
    c = next(c for c in F.GN_APPLY_CASES if c.name == "vec-t2056-none")
    r = F.gn_apply_reference(c)
    ref = r["y"].ref
    bad = ref.clone()
    dropped = (r["mask"][0, 1, 2048:] == 0).nonzero()[0]
    bad[0, 1, 2048 + int(dropped)] = 2 * r["pre"].ref[0, 1, 2048 + int(dropped)] or 1.0
    assert 0 < rel_l2(bad, ref) < 3e-2 and not torch.equal(bad, ref)
