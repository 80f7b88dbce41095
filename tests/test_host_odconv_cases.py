"""Host checks of tests/odconv_cases.py (no GPU): the dispatcher restatement agrees with the library's own plan query
(mv_odconv_cl_plan: od_dispatch's dry run, pure host code) over a sweep of shapes and every table row, every arm the sweep reaches
has rows, the generator's layers select the arms the comments in od_dispatch name, the plan's slots are what
mv_odconv_cl_pool_floats_in reports, and - what keeps the exact GPU tests exact - the fp64 reference of every row's generated inputs is
unchanged by a round trip through bf16 and fp16.  The per-element bound of the real-valued GPU tests is shown to catch two simulated
faults on the same inputs."""
import ctypes
import itertools

import pytest
import torch

import odconv_cases as C
from odconv_cases import MV_BF16, MV_F16, MV_F32

ALL_DT = (MV_BF16, MV_F16, MV_F32)

# (ks, stride, pad, dil, transposed, output_padding): every layer of the generator at both sample rates (input_proj ks 7; upsamplers
# x8 ks 16, x4 ks 8, x2 ks 4), the same with output_padding, the data gradient's 2-tap conv, and regular convs (1, 3, dilated 3, 11)
GEOMS = ((7, 1, 3, 1, 0, 0), (16, 8, 4, 1, 1, 0), (8, 4, 2, 1, 1, 0), (4, 2, 1, 1, 1, 0), (4, 2, 1, 1, 1, 1), (16, 8, 4, 1, 1, 1), (2, 1, 0, 1, 0, 0),
         (1, 1, 0, 1, 0, 0), (3, 1, 1, 1, 0, 0), (3, 1, 5, 5, 0, 0), (11, 1, 5, 1, 0, 0), (8, 2, 3, 1, 1, 0), (3, 1, 300, 300, 0, 0))
# T: 48 / 49 columns (3 column blocks and the first shape with 4) for 2-tap transposed layers (T = 47, 48) and for "same" convs, the
# K-loop's LDS limit for two samples (36 / 37), the sample-resident window (257 columns, and 273: one past it), long sequences
TS = (5, 36, 37, 47, 48, 256, 272, 700)
BS = (1, 2, 3, 16, 32)
# Cin x Cout put K * M * ksteps * 32 * es on both sides of 1 MB and 4 MB: e.g. 256 -> 128 x8 with K = 4 is exactly 4 MB in 16 bits
# (not above it) and 8 MB in fp32; 256 -> 32 x8 is exactly 1 MB in 16 bits
CINS = (8, 64, 128, 256, 288, 512, 576, 1024)
COUTS = (8, 16, 24, 32, 64, 128, 256)
KS = (1, 4, 8)
FLAGS32 = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0))           # (in_f16, out_pair, has_film)
FLAGS16 = ((0, 0, 0), (0, 0, 1))


HAND = {C._mk(s, dt) for t, dts in ((C._T16, (MV_BF16, MV_F16)), (C._T32, (MV_F32,))) for dt in dts for s in t}      # the hand-written rows


@pytest.fixture(scope="module")
def L():
    from hifigan_modified import _native
    return _native.lib()


def _plan(L, B, Cin, Tin, Cout, Tout, ks, stride, pad, dil, tr, K, act, film, dt, in_f16, out_pair):
    out = (ctypes.c_int * 14)(*([-7] * 14))
    rc = L.mv_odconv_cl_plan(B, Cin, Tin, Cout, Tout, ks, stride, pad, dil, tr, K, act, film, dt, in_f16, out_pair, out)
    return rc, list(out)


def _arm_name(dt, v):
    T = C.DT_NAME.get(dt)
    fam, S, MW, NB, kbc, ti16 = v[:6]
    return {0: f"odconv_cl_kernel<{T},{S},{MW},{NB},{kbc}>", 1: f"odconv_cl_mt_kernel<{T},{MW},{NB},{kbc}" + (",f16>" if ti16 else ">"),
            2: f"odconv_sample_kernel<{T},{kbc},{NB}>", 3: f"odconv_kloop_kernel<{T},{S},{NB},{MW}>",
            4: f"odconv_stream_kernel<{kbc},{MW},{'true' if ti16 else 'false'}>"}[fam]


def _same(L, B, Cin, Tin, Cout, ks, stride, pad, dil, tr, K, act, film, dt, in_f16, out_pair, op):
    """The library's plan against the restatement for one shape: the same refusal code, or the same arm with the same tile, LDS,
    grid, slots and walk - and slots x M is what mv_odconv_cl_pool_floats_in reports.  Returns the arm's name (None: refused)."""
    try:
        g = C.od_geom(B, Cin, Tin, Cout, ks, stride, pad, dil, tr, K, op)
        Tout = g.Tout
    except C.Refused:
        g, Tout = None, Tin
    except ValueError:
        return None
    rc, v = _plan(L, B, Cin, Tin, Cout, Tout, ks, stride, pad, dil, tr, K, act, film, dt, in_f16, out_pair)
    what = (B, Cin, Tin, Cout, ks, stride, pad, dil, tr, K, act, film, dt, in_f16, out_pair, op)
    try:
        arm = C.od_arm(B, Cin, Tin, Cout, ks, stride, pad, dil, tr, K, act, film, dt, in_f16, out_pair, op)
    except C.Refused as e:
        assert rc == e.code and v == [-7] * 14, (what, rc, e.code, v)
        if not out_pair and dt in ALL_DT and not (in_f16 and dt != MV_F32):      # (16-bit storage: pool_floats_in ignores in_f16)
            assert L.mv_odconv_cl_pool_floats_in(B, Cin, Tin, Cout, Tout, ks, stride, pad, dil, tr, K, act, film, dt, in_f16) == 0, what
        return None
    want = [C.FAM.index(arm.family), arm.S, arm.MW, arm.NB, arm.kbc, arm.ti16, arm.cols, arm.rows, arm.lds, *arm.grid, arm.slots, arm.walk]
    assert rc == 0 and v == want and _arm_name(dt, v) == arm.name, (what, rc, v, want, arm.name)
    if not out_pair:
        assert L.mv_odconv_cl_pool_floats_in(B, Cin, Tin, Cout, Tout, ks, stride, pad, dil, tr, K, act, film, dt, in_f16) == arm.slots * g.M, what
        if not in_f16:
            assert L.mv_odconv_cl_pool_floats(B, Cin, Tin, Cout, Tout, ks, stride, pad, dil, tr, K, act, film, dt) == arm.slots * g.M, what
    return arm.name


def _sweep():
    for dt in ALL_DT:
        for (ks, stride, pad, dil, tr, op), K, Cin, Cout, B, Tin in itertools.product(GEOMS, KS, CINS, COUTS, BS, TS):
            if dil == 300 and (Cin > 8 or B > 1):        # the 300-step dilation is there for one LDS fall-through
                continue
            for in_f16, out_pair, film in (FLAGS32 if dt == MV_F32 else FLAGS16):
                yield B, Cin, Tin, Cout, ks, stride, pad, dil, tr, K, C.ACT_LRELU, film, dt, in_f16, out_pair, op


@pytest.fixture(scope="module")
def swept(L):
    """Arm names the plan and the restatement (asserted equal shape by shape) reach over the sweep."""
    names = {_same(L, *s) for s in _sweep()}
    return names - {None}


def test_plan_query_agrees_with_the_restatement_over_the_sweep(L, swept):
    """mv_odconv_cl_plan against od_arm over B x Cin x Cout x layer geometry x K x T x dtype x (in_f16, out_pair, has_film): refusal
    code, or instantiation, tile, LDS, grid, slots; the sweep reaches exactly the arms of the tables."""
    assert swept == {c.arm for c in C.CASES}, (sorted(swept - {c.arm for c in C.CASES}), sorted({c.arm for c in C.CASES} - swept))
    assert len(swept) == 2 * 14 + 16


def test_plan_query_on_rows_flags_and_activations(L):
    """Every table row; tanh and SiLU epilogues (only the cl kernels have them: the 2-tap arms fall through); in_f16 / out_pair with
    16-bit storage and an unknown dtype; a plan never touches `out` when it refuses."""
    for c in C.CASES:
        for act in (C.ACT_NONE, C.ACT_LRELU):
            assert _same(L, c.B, c.Cin, c.Tin, c.Cout, c.ks, c.stride, c.pad, c.dil, c.tr, c.K, act, c.film, c.dtype, c.in_f16, c.out_pair,
                         c.op) == c.arm, c
        if not (c.in_f16 or c.out_pair):
            name = _same(L, c.B, c.Cin, c.Tin, c.Cout, c.ks, c.stride, c.pad, c.dil, c.tr, c.K, C.ACT_TANH, c.film, c.dtype, 0, 0, c.op)
            assert name is None or "odconv_cl_kernel" in name or "kloop" in name, (c, name)
    shape = (2, 64, 200, 64, 4, 2, 1, 1, 1, 4, C.ACT_LRELU, 0)
    for dt in (MV_BF16, MV_F16):
        for in_f16, out_pair in ((1, 0), (0, 1)):
            assert _same(L, *shape, dt, in_f16, out_pair, 0) is None
            assert _plan(L, 2, 64, 200, 64, 400, 4, 2, 1, 1, 1, 4, 1, 0, dt, in_f16, out_pair)[0] == C.MV_ERR_UNSUPPORTED
    assert _plan(L, 2, 64, 200, 64, 400, 4, 2, 1, 1, 1, 4, 1, 0, 7, 0, 0)[0] == C.MV_ERR_DTYPE
    assert _same(L, *shape, 7, 0, 0, 0) is None
    assert L.mv_odconv_cl_plan(2, 64, 200, 64, 400, 4, 2, 1, 1, 1, 4, 1, 0, MV_F32, 0, 0, None) == C.MV_ERR_ARG
    # od_make's refusals: M % 16, Cin % 8, K > 8, a Tout that does not belong to Tin, stride on a regular conv
    for bad in ((1, 64, 50, 8, 50, 3, 1, 1, 1, 0, 4), (1, 60, 50, 16, 50, 3, 1, 1, 1, 0, 4), (1, 64, 50, 16, 50, 3, 1, 1, 1, 0, 9),
                (1, 64, 50, 16, 51, 3, 1, 1, 1, 0, 4), (1, 64, 50, 16, 25, 3, 2, 1, 1, 0, 4), (1, 64, 50, 16, 102, 4, 2, 1, 1, 1, 4)):
        for dt in ALL_DT:
            assert _plan(L, *bad, 1, 0, dt, 0, 0) == (C.MV_ERR_UNSUPPORTED, [-7] * 14), bad


def test_every_row_names_the_arm_its_shape_selects_and_every_arm_has_ragged_rows():
    for c in C.CASES + C.BASE:
        assert C.arm_of(c).name == c.arm and C.arm_of(c, C.ACT_NONE).name == c.arm, c
    assert {c.arm for c in C.BASE} == {c.arm for c in C.CASES} and len(C.BASE) == len({c.arm for c in C.BASE}) == 44
    assert all(c in C.CASES for c in C.BASE)
    for b in C.BASE:
        rows = [c for c in C.CASES if c.arm == b.arm]
        arm, g = C.arm_of(b), C.geom_of(b)
        assert len(rows) >= 2, b.arm                                   # the base row and at least one ragged row
        assert C.macs(b) == min(C.macs(c) for c in rows if c in HAND), b.arm         # the base row is the smallest hand-written one
        nqs = {C.geom_of(c).nq % C.col_step(arm) for c in rows}
        assert len(nqs) >= 2 and nqs & {1, C.col_step(arm) - 1}, (b.arm, nqs)        # a tile entered by one column or one short of full
        if arm.S == 2:
            assert any(c.B % 2 for c in rows), b.arm                   # the second sample of the last workgroup is missing
        if any(c.tr and c.stride > 1 for c in rows) and arm.family != "sample":
            assert any(c.op == 1 for c in rows), b.arm
        if arm.family == "mt":                                         # TL = 2 with a single tile in the last group
            assert any(C.arm_of(c).walk == 2 and C.cdiv(C.geom_of(c).nq, arm.cols) % 2 for c in rows), b.arm
    # a last row block that is partly empty, per family and dtype where the geometry allows one (8 * stride * k rows past a block)
    for fam in ("cl", "mt", "kloop", "stream"):
        for dt in ALL_DT:
            rows = [c for c in C.CASES if c.dtype == dt and C.arm_of(c).family == fam]
            assert not rows or any(C.geom_of(c).M % C.arm_of(c).rows for c in rows), (fam, dt)
    # the sample-resident arm: both ends of its window with B * (M / 128) exactly 128
    for dt in (MV_BF16, MV_F16):
        rows = [c for c in C.CASES if c.arm == f"odconv_sample_kernel<{C.DT_NAME[dt]},256,17>"]
        assert {C.geom_of(c).nq for c in rows} >= {257, 272} and all(c.B * (C.geom_of(c).M // 128) == 128 for c in rows)
    # the streaming arms: the first shapes they see (49 and 50 columns), one workgroup per (sample, row block), several tiles per wave
    for name in ("odconv_stream_kernel<64,8,false>", "odconv_stream_kernel<128,4,true>"):
        rows = [c for c in C.CASES if c.arm == name]
        assert {C.geom_of(c).nq for c in rows} >= {49, 50}
        assert any(256 // (c.B * C.arm_of(c).grid[1]) <= 1 and C.arm_of(c).walk > 1 for c in rows), name
        # the ragged end only the sample's last wave takes: the waves' spans (grid.x * 8 waves * tpw tiles) end before nq - by one column,
        # by two (output_padding), and behind a wave that walks two tiles
        tails = {(C.geom_of(c).nq - C.arm_of(c).grid[0] * C.OS_NW * C.arm_of(c).walk * 16, C.arm_of(c).walk) for c in rows}
        assert {(1, 1), (2, 1), (1, 2)} <= tails, (name, sorted(tails))
    assert any(C.arm_of(c).grid[0] > 1 and C.arm_of(c).walk > 1 for c in C.CASES if c.arm == "odconv_stream_kernel<64,8,false>")
    assert any(c.out_pair for c in C.CASES) and {c.K for c in C.CASES} >= {1, 4, 8}
    # regular convs: ks 7 with pad 3 and a dilated one per storage type; the data gradient's 2-tap shapes of the four upsamplers
    for dt in ALL_DT:
        rows = [c for c in C.CASES if c.dtype == dt and not c.tr]
        assert any(c.ks == 7 and c.pad == 3 for c in rows) and any(c.dil > 1 for c in rows) and any(c.ks == 2 for c in rows)
    two_tap = {(c.Cin, c.Cout) for c in C.CASES if not c.tr and c.ks == 2 and c.dtype == MV_BF16}
    assert two_tap >= {(2048, 512), (1024, 256), (128, 128), (128, 64)}


def test_reference_cost_of_the_tables():
    """No ragged companion above MAX_MACS multiply-adds of fp64 reference; the hand-written rows stay below 2.3 GMAC, the K-loop
    rows within B <= 5, T <= 40, and all references together below 30 GMAC (about 10 s of fp64 convolutions on 8 cores)."""
    for c in C.CASES:
        assert C.macs(c) <= (2.3e9 if c in HAND else C.MAX_MACS), (c, C.macs(c))
        if "kloop" in c.arm:
            assert c.B <= 5 and c.Tin <= 40, c
    per_shape = {C.shape_of(c): C.macs(c) for c in C.CASES}                       # one reference per shape, shared by the dtypes
    assert sum(per_shape.values()) < 30e9 and len(per_shape) < 250, (sum(per_shape.values()), len(per_shape))


# the generator's layers at the benchmark's batch (32 clips x 32 mel frames at 22.05 kHz, x 16 frames of 128 mels at 48 kHz), named
# from the comments in od_dispatch: (B, Cin, Tin, Cout, ks, stride, pad, dil, transposed, K, has_film, in_f16, out_pair) -> arm per
# storage type (16-bit, fp32).  The mixed mode runs fp16 through the second upsampler and hands the third an fp16 stream (in_f16).
KNOWN = (
    ((32, 80, 32, 512, 7, 1, 3, 1, 0, 4, 1, 0, 0), "odconv_cl_kernel<T,1,1,3,4>", "odconv_cl_kernel<float,1,1,3,4>"),      # input_proj: 128 workgroups with S = 2
    ((32, 512, 32, 256, 16, 8, 4, 1, 1, 4, 0, 0, 0), "odconv_kloop_kernel<T,2,3,1>", "odconv_kloop_kernel<float,2,3,2>"),  # ups0: K-loop, S = 2
    ((32, 256, 256, 128, 16, 8, 4, 1, 1, 4, 0, 0, 0), "odconv_sample_kernel<T,256,17>", "odconv_cl_kernel<float,1,2,9,4>"),  # ups1
    ((32, 128, 2048, 64, 4, 2, 1, 1, 1, 4, 0, 0, 0), "odconv_cl_mt_kernel<T,2,4,128>", "odconv_cl_mt_kernel<float,1,4,128>"),  # ups2
    ((32, 128, 2048, 64, 4, 2, 1, 1, 1, 4, 0, 1, 0), None, "odconv_stream_kernel<128,4,true>"),                               # ups2, mixed
    ((32, 64, 4096, 64, 4, 2, 1, 1, 1, 4, 0, 0, 0), "odconv_cl_mt_kernel<T,2,8,64>", "odconv_stream_kernel<64,8,false>"),      # ups3
    ((32, 64, 4096, 64, 4, 2, 1, 1, 1, 4, 0, 0, 1), None, "odconv_stream_kernel<64,8,false>"),                                 # ups3, pair rows
    ((32, 128, 16, 512, 7, 1, 3, 1, 0, 4, 1, 0, 0), "odconv_cl_kernel<T,1,1,3,4>", "odconv_cl_kernel<float,1,1,3,4>"),     # 48 kHz input_proj
    ((32, 512, 16, 256, 16, 8, 4, 1, 1, 4, 0, 0, 0), "odconv_kloop_kernel<T,2,3,1>", "odconv_kloop_kernel<float,2,3,2>"),  # 48 kHz ups0
    ((32, 256, 128, 128, 16, 8, 4, 1, 1, 4, 0, 0, 0), "odconv_cl_mt_kernel<T,1,6,256>", "odconv_cl_kernel<float,1,2,9,4>"),  # 48 kHz ups1: 129 columns
    ((32, 128, 1024, 64, 8, 4, 2, 1, 1, 4, 0, 0, 0), "odconv_cl_mt_kernel<T,2,4,128>", "odconv_cl_mt_kernel<float,1,4,128>"),  # 48 kHz ups2 (k8 s4)
    ((32, 128, 1024, 64, 8, 4, 2, 1, 1, 4, 0, 1, 0), None, "odconv_stream_kernel<128,4,true>"),
)


def test_known_arms_of_the_generator_layers(L):
    assert len(KNOWN) == 12
    for (B, Cin, Tin, Cout, ks, stride, pad, dil, tr, K, film, in_f16, out_pair), n16, n32 in KNOWN:
        for dt in ALL_DT:
            want = n32 if dt == MV_F32 else (n16 and n16.replace("<T,", f"<{C.DT_NAME[dt]},"))
            args = (B, Cin, Tin, Cout, ks, stride, pad, dil, tr, K, C.ACT_LRELU, film, dt, in_f16, out_pair)
            if want is None:
                with pytest.raises(C.Refused):
                    C.od_arm(*args)
            else:
                assert C.od_arm(*args).name == want, (args, want)
            assert _same(L, *args, 0) == want
    assert C.lds_row_stride(1024, 2) == 1056 and C.lds_row_stride(2048, 2) == 2080 and C.lds_row_stride(512, 2) == 544
    g = C.od_geom(32, 512, 32, 256, 16, 8, 4, 1, 1, 4)
    assert g == C.Geom(256, 2, 2048, 33, 32, 128, -1)
    g = C.od_geom(2, 80, 32, 512, 7, 1, 3, 1, 0, 4)
    assert g == C.Geom(32, 7, 512, 32, 18, 70, -3)
    assert C.od_geom(1, 64, 48, 16, 4, 2, 1, 1, 1, 4, 1).nq == 50 and C.od_geom(1, 64, 48, 16, 4, 2, 1, 1, 1, 4, 1).Tout == 97


def _exact16(t):
    return all(torch.equal(t.to(dt).double(), t) for dt in (torch.bfloat16, torch.float16))


def test_references_are_exact_in_both_16_bit_types():
    """For every row: 8 / taps non-zero input channels per step, bank weights in {-1, 0, 1}, integer alpha with sum |alpha| <= 3, and
    the reference of every form the GPU test compares (with and without the mixed bias, with and without LeakyReLU(0.5), behind an
    integer FiLM) survives bf16 and fp16 unchanged; the channel sums handed on stay exact fp32 integers (or halves)."""
    for shape in sorted({C.shape_of(c) for c in C.CASES}):
        B, Cin, Tin, Cout, ks, stride, pad, dil, tr, K, op = shape
        x, w, b, alpha, ref = C.reference(shape)
        ntaps = ks // stride if tr else ks
        assert torch.equal((x != 0).sum(-1), torch.full((B, Tin), min(C.nnz_of(ntaps), Cin))) and float(x.abs().max()) == 1, shape
        assert float(w.abs().max()) <= 1 and float(b.abs().max()) <= 3 and float(alpha.abs().sum(1).max()) <= 3
        assert bool((alpha == alpha.round()).all()) and bool((alpha != 0).any(1).all())
        assert float((ref + C.mixed_bias(alpha, b)).abs().max()) <= 33, shape
        assert _exact16(x) and _exact16(w) and _exact16(b) and _exact16(alpha)
        for r in (ref, ref + C.mixed_bias(alpha, b)):
            assert _exact16(r) and _exact16(C.lrelu(r, C.SLOPE)), shape
            assert float(C.lrelu(r, C.SLOPE).abs().sum(1).max()) < 2 ** 22       # channel sums: exact in fp32 in any order
        if any(c.film for c in C.CASES if C.shape_of(c) == shape):
            F_ = C.film_F_of(Cout)
            fr = C.film_ref(ref + C.mixed_bias(alpha, b), C.film_inputs(B, Cout, F_), F_)
            assert _exact16(fr) and _exact16(C.lrelu(fr, C.SLOPE)) and float(fr.abs().max()) <= 69, shape
    C.reference.cache_clear()


def test_impulse_expectations_equal_the_convolution():
    """The index formulas of the impulse tests against the fp64 reference they stand for: a transposed layer with output_padding, a
    dilated conv and a 2-tap conv."""
    for c in (C.Case("", 2, 16, 9, 8, 8, 4, 2, 1, 1, 4, 1, MV_BF16, 0, 0, 0), C.Case("", 3, 8, 20, 16, 3, 1, 5, 5, 0, 8, 0, MV_BF16, 0, 0, 0),
              C.Case("", 2, 24, 7, 16, 2, 1, 0, 1, 0, 1, 0, MV_BF16, 0, 0, 0)):
        shape, g = C.shape_of(c), C.geom_of(c)
        x, w, _, alpha = C.inputs(shape)
        wb = torch.einsum("bk,k...->b...", alpha, w)
        for pt in ((0, 0, 0), (c.B - 1, c.Tin - 1, c.Cin - 1), (1, c.Tin // 2, 7)):
            xi = torch.zeros_like(x)
            xi[pt] = 1.0
            want = torch.zeros(c.B, g.Tout, c.Cout, dtype=torch.float64)
            for u, v in C.x_impulse_rows(c, g, wb, pt):
                want[pt[0], u] += v
            assert torch.equal(want, C.odconv_ref(xi, w, alpha, shape)), (c, pt)
        xd = C.ints((c.B, c.Tin, c.Cin), -1, 1, 17)
        for row in C.row_edges(C.Arm("", "cl", 1, 1, 3, 4, 0, 48, 16, 0, (1, 1, 1), 1, 0), g):
            o, r = C.gemm_row_to_weight_index(c, row)
            for m in range(g.ntaps):
                j, ch, kb = r + m * c.stride if c.tr else m, (5 * row + 3) % c.Cin, c.K - 1
                wi = torch.zeros_like(w)
                wi[(kb, ch, o, j) if c.tr else (kb, o, ch, j)] = 1.0
                u, t = C.w_impulse_steps(c, g, j)
                want = torch.zeros(c.B, g.Tout, c.Cout, dtype=torch.float64)
                want[:, u, o] = alpha[:, kb, None] * xd[:, t, ch]
                assert torch.equal(want, C.odconv_ref(xd, wi, alpha, shape)), (c, row, m)


def test_impulse_rows_have_the_boundaries_and_the_positions_sit_on_both_sides():
    """Every arm's impulse row has more than one sample, at least 16 channels, at least two row blocks and - unless the arm only
    sees one-tile sequences (the S = 2 arms) - at least two column tiles (16-column blocks for kloop and sample; a TL = 2 walk for
    mt; two tiles per wave and two workgroups per sample for stream); the position sets are not empty on any of these boundaries
    and hold both sides of them."""
    assert [c.arm for c in C.IMPULSE] == [c.arm for c in C.BASE] and all(c in C.CASES for c in C.IMPULSE)
    for c in C.IMPULSE:
        arm, g = C.arm_of(c), C.geom_of(c)
        assert C.impulse_ok(c) and c.B > 1 and c.Cin >= 16 and g.M > arm.rows, c
        ts, step = C.column_edges(c, arm, g), C.col_step(arm)
        assert {0, c.Tin - 1} <= set(ts)
        if not (arm.family == "cl" and arm.S == 2):
            assert g.nq > step and {step - 1, step} <= set(ts), c               # both sides of the first column boundary
            last = (g.nq - 1) // step * step                                      # ... and of the last one that has input on both sides
            last = last if last < c.Tin else last - step
            assert {last - 1, last} <= set(ts), (c, last)
        if arm.family == "mt":
            assert arm.walk == 2 and {2 * arm.cols - 1, 2 * arm.cols} <= set(ts), c    # the boundary between two workgroups' walks
        if arm.family == "stream":
            assert arm.walk > 1 and arm.grid[0] > 1, c
            wave, wg = 16 * arm.walk, 16 * arm.walk * C.OS_NW
            assert {wave - 1, wave, wg - 1, wg} <= set(ts), c
        pts = C.x_impulses(c, arm, g)
        chans = {p[2] for p in pts}
        assert len(range(8, c.Cin, 8)) >= 1 and all({k - 1, k} <= chans for k in range(8, c.Cin, 8)), c    # every k-chunk boundary
        if c.Cin > 32:
            assert {31, 32} <= chans                                              # a k-step boundary
        assert {p[0] for p in pts} >= {0, c.B - 1}
        rows, blocks = C.row_edges(arm, g), list(range(arm.rows, g.M, arm.rows))
        assert blocks and {0, g.M - 1} <= set(rows) and all({r - 1, r} <= set(rows) for r in blocks), c
    # and every arm has table rows with more than one row block, one of them with the last block partly empty where Cout allows it
    for b in C.BASE:
        multi = [c for c in C.CASES if c.arm == b.arm and C.geom_of(c).M > C.arm_of(c).rows]
        assert multi, b.arm
        if C.arm_of(b).family != "sample":                   # (the sample-resident kernel needs M % 128 == 0)
            assert any(C.geom_of(c).M % C.arm_of(c).rows for c in multi), b.arm


def test_the_real_valued_bound_catches_simulated_faults():
    """On the inputs of the real-valued GPU test: the fp32 mode's three-product split arithmetic stays inside the per-element bound,
    the same arithmetic without the weight-lo x activation-hi product exceeds it, and so does - in every storage type - an output
    whose single column is shifted by one step.  Two shapes: 448 terms per element (conv, ks 7) and 1024 (the first upsampler)."""
    import numerics_sim as NS
    for shape in ((2, 64, 60, 64, 7, 1, 3, 1, 0, 4, 0), (2, 512, 32, 256, 16, 8, 4, 1, 1, 4, 0)):
        for dt in ALL_DT:
            c = C.Case("", *shape, dt, 0, 0, 0)
            x, w, bias, alpha = C.real_inputs(c)
            ref, A, slack = C.real_bound(c, x, w, bias, alpha)
            bound = slack + C.U[dt] * ref.abs()
            shifted = ref.clone()
            shifted[:, 5] = ref[:, 4]
            assert bool(((shifted - ref).abs() > bound).any()), (shape, dt)
            if dt != MV_F32:
                continue
            wb = torch.einsum("bk,k...->b...", alpha.float(), w.float())          # the mix, in fp32 as the kernels form it
            eye = torch.eye(c.B, dtype=torch.float64)
            conv = lambda ww, xx: C.odconv_ref(xx, ww, eye, shape[:9] + (c.B, 0))  # B "banks", one per sample
            good = NS.split_product(conv, wb, x) + C.mixed_bias(alpha, bias)
            bad = NS.split_product(conv, wb, x, drop=("lh",)) + C.mixed_bias(alpha, bias)
            assert bool(((good - ref).abs() <= bound).all()), (shape, float(((good - ref).abs() / bound).max()))
            assert bool(((bad - ref).abs() > bound).any()), (shape, float(((bad - ref).abs() / bound).max()))
    # the streaming arms: f16 pieces, held to C_STREAM.  fp32 rows: three products; fp16 rows: x is exact, two products
    for shape, in_f16 in (((2, 64, 200, 64, 4, 2, 1, 1, 1, 4, 0), 0), ((2, 128, 100, 64, 4, 2, 1, 1, 1, 4, 0), 1)):
        c = C.Case("", *shape, MV_F32, in_f16, 0, 0)
        assert C.arm_of(c).family == "stream"
        x, w, bias, alpha = C.real_inputs(c)
        ref, A, slack = C.real_bound(c, x, w, bias, alpha)
        bound = slack + C.U[MV_F32] * ref.abs()
        wb = torch.einsum("bk,k...->b...", alpha.float(), w.float())
        eye = torch.eye(c.B, dtype=torch.float64)
        conv = lambda ww, xx: C.odconv_ref(xx, ww, eye, shape[:9] + (c.B, 0))
        good = NS.split_product(conv, wb, x, split=NS.f16_split) + C.mixed_bias(alpha, bias)
        bad = NS.split_product(conv, wb, x, drop=("lh",), split=NS.f16_split) + C.mixed_bias(alpha, bias)
        assert bool(((good - ref).abs() <= bound).all()), (shape, float(((good - ref).abs() / bound).max()))
        assert bool(((bad - ref).abs() > bound).any()), (shape, float(((bad - ref).abs() / bound).max()))
