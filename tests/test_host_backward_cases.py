"""Host checks of tests/backward_cases.py (no GPU): every table row is proven exact (sum|terms| < 2^24 in units of its granularity, a
stored result unchanged by a round trip through bf16 and fp16) or carries a derived bound with its k; the two rule restatements agree
with the library's own dry runs (mv_conv1d_wgrad_plan, mv_odconvT_wgrad_plan: pure host code) over sweeps with the B x tiles = 2048
boundary and Tin at multiples of 128 +- 1; the named arms of the tables and of the generator's own layers are pinned; arms no call can
reach are asserted as such; and one corrupted tap shows why the GPU tests compare element by element."""
import ctypes
import itertools
import os
import re

import pytest
import torch

import backward_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "a-modified-hifi-gan-vocoder-using-odconv-and-grc-for-expressive-voice-cloning-_amd")


@pytest.fixture(scope="module")
def L():
    from hifigan_modified import _native
    return _native.lib()


def _outs(name, r):
    return [(f"{name}:{n}", o) for n, o in r.items() if isinstance(o, C.Out)]


def _all_outputs():
    """(label, Out) of every reference the GPU file compares with."""
    for c in C.WG_CASES:
        yield from _outs(f"wgrad {c.name}", C.wg_reference(c))
    for a in C.REDUCE_CASES:
        yield from _outs(f"reduce {a}", C.reduce_reference(*a))
    for a in C.BIAS_CASES:
        yield from _outs(f"bias {a}", C.bias_reference(*a))
    for a in C.ATTN_CASES:
        yield from _outs(f"attn {a}", C.attn_reference(*a))
    for a in C.FILM_CASES:
        yield from _outs(f"film {a}", C.film_reference(*a))
    for a in C.LINEAR_CASES:
        yield from _outs(f"linear {a}", C.linear_reference(*a))
    for a in C.AVGPOOL_CASES:
        yield from _outs(f"avgpool {a}", C.avgpool_reference(*a))
    yield from _outs("act", C.act_reference())
    for a in C.CONV2D_CASES:
        yield from _outs(f"conv2d {a}", C.conv2d_reference(*a))
    for kind, n in itertools.product(range(5), C.LOSS_N):
        yield from _outs(f"loss {kind} {n}", C.loss_reference(kind, n))
    for a in C.GRC_CASES:
        yield from _outs(f"grc {a}", C.grc_reference(*a)[1])
    for a in C.ODT_CASES:
        yield from _outs(f"odconvT {a}", C.odt_reference(*a))
    for sh in C.GN_SHAPES:
        i = C.gn_inputs(*sh)
        for act, mask in itertools.product((C.ACT_NONE, C.ACT_LRELU), (False, True)):
            gz = C.gn_gz(i, sh[2], act, mask)
            yield f"gn {sh} {act} {mask}:gz", C.exact(gz, unit=0.5, stored=True)
            yield from _outs(f"gn {sh} {act} {mask}", C.gn_from_gz(i, gz, sh[2], 1))


def test_every_row_is_exact_or_carries_a_bound():
    n_exact = n_bound = 0
    for label, o in _all_outputs():
        assert o.ref.dtype == torch.float64 and o.ref.shape == o.abs_sum.shape, label
        assert bool((o.abs_sum + 1e-12 >= o.ref.abs()).all()), label
        if o.k == 0:
            assert C.proves_exact(o), (label, float((o.abs_sum / o.unit).max()))
            n_exact += 1
        else:
            assert 0 < o.k < 4096 and bool((C.tolerance(o, C.MV_F32) < 1e-2 * (1 + o.abs_sum)).all()), label
            n_bound += 1
    assert n_exact > 250 and 0 < n_bound < n_exact / 4, (n_exact, n_bound)


def test_inputs_are_small_integers_and_dyadic_alphas():
    for c in C.WG_CASES:
        r = C.wg_reference(c)
        for n in ("x", "gy", "w"):
            if n in r:
                assert bool((r[n] == r[n].round()).all()) and float(r[n].abs().max()) <= 3 and bool((r[n] != 0).any())
        if c.nbanks > 1:
            a = r["alpha"]
            assert bool(((a * 8) == (a * 8).round()).all()) and bool((a.sum(1) == 1).all()) and bool((a >= 0).all())
            assert bool((r["galpha0"] != 0).any())                    # the += buffers start from non-zero integers
    i = C.gn_inputs(2, 8, 2, 64)
    assert bool((i["mean"] == i["mean"].round()).all()) and bool((torch.log2(i["rstd"]) == torch.log2(i["rstd"]).round()).all())
    assert int(i["mask"].max()) == 255 and int(i["mask"].min()) == 0


# ----------------------------------------------------------------------------------------------- mv_conv1d_wgrad: restatement == dry run
def _c_wgrad(L, *shape):
    out = (ctypes.c_int * 9)(*([-7] * 9))
    return L.mv_conv1d_wgrad_plan(*shape, out), tuple(out)


def _same_wgrad(L, shape):
    rc, v = _c_wgrad(L, *shape)
    try:
        p = C.wgrad_plan(*shape)
    except C.Refused as e:
        assert rc == e.code and v == (-7,) * 9, (shape, rc, e.code, v)        # a refusal writes nothing
        return None
    assert rc == 0 and v == tuple(p), (shape, rc, v, p)
    return p


def test_wgrad_restatement_equals_the_plan_query(L):
    seen = set()
    for B, (Cin, Cout), Tout, (ks, stride, dil), nb in itertools.product(
            (1, 2, 3, 7, 8, 9, 16, 31, 32, 33, 127, 128, 129, 2048, 2049),
            ((1, 1), (16, 16), (17, 18), (17, 20), (3, 5), (80, 512), (128, 128), (256, 256), (512, 256), (255, 257)),
            (1, 63, 64, 65, 127, 128, 129, 130, 200, 1000, 8192),
            ((1, 1, 1), (3, 1, 1), (3, 1, 5), (7, 2, 3), (11, 1, 1), (16, 8, 1), (16, 8, 30), (16, 8, 31), (17, 1, 1), (0, 1, 1), (3, 0, 1)),
            (1, 2, 4, 5, 8, 9)):
        p = _same_wgrad(L, (B, Cin, Cout, Tout, ks, stride, dil, nb))
        if p is not None:
            seen.add((min(p.tsplit, 3), p.zero_fill, p.per_sample, p.reduce4))
            assert p.tchunk % 64 == 0 and (p.tsplit - 1) * p.tchunk < Tout <= p.tsplit * p.tchunk       # no empty chunk, none missing
            assert p.gz == B * p.tsplit <= 65535
    # every combination of (one / two / more chunks) x (bank mode) exists, except a zero-fill-free single-bank call
    want = {(t, 1, 0, -1) for t in (1, 2, 3)} | {(t, int(t > 1), 1, r) for t in (1, 2, 3) for r in (0, 1)}
    assert seen == want, seen ^ want


def test_wgrad_split_boundary_at_2048_workgroups(L):
    """B x tiles on both sides of 2048: below it the time axis is split, at and above it one workgroup walks the sample."""
    for B, Cin, Cout in ((2047, 16, 16), (2048, 16, 16), (2049, 16, 16), (32, 128, 128), (31, 128, 128), (16, 128, 128), (8, 256, 256),
                         (7, 256, 256), (1024, 32, 16), (1023, 32, 16)):
        p = _same_wgrad(L, (B, Cin, Cout, 130, 3, 1, 1, 4))
        tiles = C.cdiv(Cin, 16) * C.cdiv(Cout, 16)
        assert (p.tsplit == 1) == (B * tiles >= 2048), (B, tiles, p)
        assert p.zero_fill == int(p.tsplit > 1)


@pytest.mark.parametrize("c", C.WG_CASES, ids=lambda c: c.name)
def test_wgrad_rows_select_their_arm(L, c):
    p = _same_wgrad(L, (c.B, c.Cin, c.Cout, c.Tout, c.ks, c.stride, c.dil, c.nbanks))
    assert p is not None and C.wg_tin(c) > 0
    if c.arm is not None:
        assert (p.tsplit, p.zero_fill, p.reduce4) == c.arm, (c, p)


def test_wgrad_named_arms_refusals_and_generator_layers(L):
    arm = {c.name: C.wgrad_plan(c.B, c.Cin, c.Cout, c.Tout, c.ks, c.stride, c.dil, c.nbanks) for c in C.WG_CASES}
    assert (arm["t200-split4"].tsplit, arm["t200-split4"].tchunk) == (4, 64)               # ragged last chunk: 200 - 192 = 8 steps
    assert (arm["t200-split2"].tsplit, arm["t200-split2"].tchunk) == (2, 128)              # second chunk: 72 steps
    assert (arm["t130-direct"].tsplit, arm["t130-direct"].tchunk, arm["t130-direct"].zero_fill) == (1, 192, 0)   # three 64-step iterations
    assert arm["lds-65344"].lds == 65344 and C.wgrad_lds(16, 8, 31) == 66304
    assert {c.ks for c in C.WG_CASES} >= {1, 3, 7, 11, 16} and {c.stride for c in C.WG_CASES} >= {1, 2, 8}
    assert {c.dil for c in C.WG_CASES} >= {1, 3, 5} and {c.Tout for c in C.WG_CASES} >= {1, 63, 64, 65}
    assert {c.nbanks for c in C.WG_CASES} >= {1, 2, 4, 5, 8}
    assert any(c.pad == 0 for c in C.WG_CASES) and any(c.pad > (c.ks - 1) * c.dil for c in C.WG_CASES)
    for name, shape, code in C.WG_REFUSED:
        rc, v = _c_wgrad(L, *shape)
        assert rc == code and v == (-7,) * 9, (name, rc)
    for shape, want in C.WG_KNOWN:
        p = _same_wgrad(L, shape)
        assert (p.tsplit, p.zero_fill, p.reduce4) == want, (shape, p)


def test_wgrad_tsplit_is_the_plan_field(L):
    """wgrad_tsplit (imported by test_gpu_generator_train_shapes.py) is the plan's first field."""
    for B, Cin, Cout, Tout in ((2, 80, 512, 32), (16, 80, 512, 200), (2, 512, 256, 32), (16, 64, 32, 4096)):
        rc, v = _c_wgrad(L, B, Cin, Cout, Tout, 7, 1, 1, 4)
        assert rc == 0 and v[0] == C.wgrad_tsplit(B, Cin, Cout, Tout)


def test_wgrad_kernel_has_no_shared_bank_store():
    """Unreachable and deleted: a conv1d_wgrad_kernel arm that applies the alpha chain itself (nbanks > 1 without per-sample tiles).
    The host derives per_sample from nbanks > 1 in one place and the kernel takes neither banks, alpha nor galpha."""
    src = open(os.path.join(PKG, "csrc", "backward.hip")).read()
    kern = src[src.index("void conv1d_wgrad_kernel("):src.index("// ODConv bank gradients from per-sample tiles")]
    params = kern.split(") {", 1)[0]
    assert not re.search(r"alpha|nbanks|\bw\b", params) and "atomicAdd(galpha" not in kern
    assert src.count("conv1d_wgrad_kernel<T>") == 1 and len(re.findall(r"per_sample = nbanks > 1", src)) == 1


def test_reduce_rows_cover_both_arms():
    arms = {(C.reduce_reference(*a)["reduce4"], a[2] % 4 == 0, a[1] <= 4) for a in C.REDUCE_CASES}
    assert arms == {(1, True, True), (0, False, True), (0, True, False), (0, False, False)}
    assert {a[0] for a in C.REDUCE_CASES} >= {1, 3, 33} and {a[1] for a in C.REDUCE_CASES} >= {1, 4, 5, 8}
    assert {a[2] for a in C.REDUCE_CASES} >= {4, 1023, 1024, 1025, 1028}


# ----------------------------------------------------------------------------------------------- mv_odconvT_wgrad_mfma: restatement == dry run
def _c_odt(L, *shape):
    out = (ctypes.c_int * 12)(*([-7] * 12))
    return L.mv_odconvT_wgrad_plan(*shape, out), tuple(out)


def _same_odt(L, shape):
    rc, v = _c_odt(L, *shape)
    try:
        p = C.odconvT_plan(*shape)
    except C.Refused as e:
        assert rc == e.code and v == (-7,) * 12, (shape, rc, e.code, v)
        return None
    assert rc == 0 and v == p, (shape, rc, v, p)
    return p


def test_odconvT_restatement_equals_the_plan_query(L):
    n = 0
    for B, Tin, (Cin, Cout, ks, stride), K, dt in itertools.product(
            (1, 3, 16, 65535, 65536), (1, 127, 128, 129, 255, 256, 257, 383, 384, 385, 4096),
            C.ODT_SHAPES + ((512, 256, 16, 8), (64, 32, 4, 2), (60, 32, 4, 2), (64, 3, 4, 2), (64, 32, 5, 2), (64, 32, 4, 3), (8, 4, 2, 1)),
            (1, 4, 5, 8, 9), (C.MV_F32, C.MV_BF16, C.MV_F16)):
        p = _same_odt(L, (B, Tin, Cin, Cout, ks, stride, K, dt))
        if p is not None:
            n += 1
            assert p[4] == C.cdiv(Tin, 128) == p[6] and p[7] == p[11] == B and p[5] == B * p[4]      # one workgroup per (tile, sample)
            assert p[8] == 2 * (128 + 129) * 160 <= 160 * 1024
    assert n > 500


def test_odconvT_rows_refusals_and_generator_layers(L):
    for si, B, Tin, K in C.ODT_CASES:
        for dt in (C.MV_BF16, C.MV_F16):
            assert _same_odt(L, (B, Tin, *C.ODT_SHAPES[si], K, dt)) is not None
    assert {C.cdiv(a[2], 128) for a in C.ODT_CASES} == {1, 2, 3} and {a[3] for a in C.ODT_CASES} == {1, 4, 5, 8}
    p = C.odconvT_plan(1, 129, *C.ODT_SHAPES[2], 4, C.MV_BF16)
    assert (p[9], p[10]) == (2, 2) and (3 * 24) % 64 and 72 % 64               # (72, 24, 6, 3): a remainder in both 64-wide tile directions
    p = C.odconvT_plan(1, 129, *C.ODT_SHAPES[3], 4, C.MV_BF16)
    assert (p[9], p[10]) == (3, 1) and 136 % 64
    for shape, code in (((1, 8, 8, 4, 4, 2, 4, C.MV_F32), C.MV_ERR_UNSUPPORTED), ((1, 8, 8, 4, 5, 2, 4, C.MV_BF16), C.MV_ERR_ARG),
                        ((1, 8, 12, 4, 4, 2, 4, C.MV_BF16), C.MV_ERR_ARG), ((1, 8, 8, 4, 4, 2, 9, C.MV_F16), C.MV_ERR_ARG)):
        rc, v = _c_odt(L, *shape)
        assert rc == code and v == (-7,) * 12, (shape, rc)
    for shape, (chunks, gx, gy, gz) in C.ODT_KNOWN:
        p = _same_odt(L, (*shape, C.MV_BF16))
        assert (p[4], p[9], p[10], p[11]) == (chunks, gx, gy, gz), (shape, p)


def test_odconvT_two_tap_form_is_outside_the_discriminator_plan(L):
    """kw = 2 is refused by mv_dconv_wgrad_plan (the all-samples form): only the per-sample query reaches dconv_wgrad_kernel<T,1,2,128>."""
    out = (ctypes.c_int * 12)()
    assert L.mv_dconv_wgrad_plan(1, 1, 128, 8, 8, 1, 2, 1, C.MV_BF16, out) == C.MV_ERR_UNSUPPORTED
    assert _same_odt(L, (1, 128, 8, 4, 4, 2, 1, C.MV_BF16))[:2] == (0, 2)


# ----------------------------------------------------------------------------------------------- other arms, by their host rules
def test_grc_rows_take_both_lds_paths():
    lds = [C.grc_lds(*a) for a in C.GRC_CASES]
    assert lds[0] == 46784 and lds[0] <= 64 * 1024                    # the generator's own shape: 47 KB
    assert lds[1] <= 64 * 1024 < lds[2] == 92544 <= 160 * 1024        # 92.5 KB: the raised-limit path
    assert C.grc_lds(*C.GRC_REFUSED) > 160 * 1024


def test_grc_closed_form_equals_autograd_of_the_fold():
    for a in C.GRC_CASES[:2]:
        i, r = C.grc_reference(*a)
        leaf = {k: v.clone().requires_grad_(True) for k, v in i.items() if k not in ("g_weff", "g_beff")}
        w, b, _ = C.grc_fold(leaf, a[3])
        ((w * i["g_weff"]).sum() + (b * i["g_beff"]).sum()).backward()
        for n, m in (("g_conv_w", "conv_w"), ("g_conv_b", "conv_b"), ("g_A", "A"), ("g_B", "Bm"), ("g_s", "s"), ("g_proj_w", "proj_w")):
            assert torch.equal(leaf[m].grad, r[n].ref), n
        assert float(r["g_s"].ref.abs()) > 0


def test_leaky_relu_zero_point_convention():
    """Every LeakyReLU derivative in csrc/ selects `>= 0 ? 1 : slope`: 1 at +0 and -0, where torch's autograd gives `slope`."""
    z = torch.tensor([0.0, -0.0], dtype=torch.float64, requires_grad=True)
    torch.nn.functional.leaky_relu(z, C.SLOPE).sum().backward()
    assert z.grad.tolist() == [C.SLOPE, C.SLOPE]
    assert C.gn_dact(z.detach(), C.ACT_LRELU).tolist() == [1.0, 1.0]
    r = C.act_reference()
    at0 = r["y"] == 0
    assert int(at0.sum()) >= 2 and torch.equal(r["lrelu"].ref[at0], r["gy"][at0])
    sites = 0
    for f in ("backward.hip", "disc_fused.hip"):
        src = open(os.path.join(PKG, "csrc", f)).read()
        sites += len(re.findall(r">= 0\.f \? 1\.f : \w+", src))
        assert not re.findall(r"> 0\.f \? 1\.f : (slope|ns)\b", src), f
    assert sites >= 2


def test_silu_never_reaches_act_bwd():
    """mv_act_bwd refuses ACT_SILU; functional.py sends SiLU to group_norm only (whose backward recomputes the pre-activation)."""
    src = open(os.path.join(PKG, "hifigan_modified", "functional.py")).read()
    lines = src.splitlines()
    uses = [lines[n - 1] + l for n, l in enumerate(lines) if re.search(r"silu|SILU", l) and "_ACT = " not in l]   # with the call's first line
    assert uses and all(("group_norm(" in l or "groupnorm_" in l) for l in uses), uses
    assert len(re.findall(r"ops\.act_bwd\(", src)) == 4


def test_copy2d_predicate_terms():
    """The copy2d cases falsify each term of the vector predicate in turn."""
    for dt in (C.MV_F32, C.MV_BF16, C.MV_F16):
        vec = {c[0]: C.copy_takes_vector(c, dt) for c in C.COPY_CASES}
        assert vec["vector"] and vec["second-pass"]
        assert not any(vec[n] for n in ("n", "s_rs", "d_rs", "s_os", "d_os", "src", "dst", "second-pass-scalar", "one"))
    L = C.copy_layout(next(c for c in C.COPY_CASES if c[0] == "second-pass"))
    assert L["n"] // 8 > 64 * 256                       # more 16-byte pieces than the 64 x 256 threads of a row's grid


# ----------------------------------------------------------------------------------------------- why element by element
def test_one_wrong_tap_passes_rel_l2_and_fails_the_new_comparison():
    """The bank gradient of the t200-split2 row (4 x 128 x 128 x 3) with two defects.  (a) One element loses one time step of one
    sample (a term gy x = 4 under alpha = 1/8): the whole-tensor rel-L2 is 1.3e-4, inside the 2e-4 that tests/test_gpu_grads.py and
    tests/test_gpu_generator_train_shapes.py ask of fp32 parameter gradients.  (b) One tap of one 16 x 16 tile loses such a step in
    every element (256 elements off by 1/8): rel-L2 5.4e-4, inside every 16-bit parameter bound of the latter file (2.5e-2 and up).
    torch.equal rejects both."""
    c = next(c for c in C.WG_CASES if c.name == "t200-split2")
    ref = C.wg_reference(c)["gw"].ref
    rel = lambda a: float((a - ref).norm() / ref.norm())
    one = ref.clone()
    one[1, 5, 7, 2] -= 4 * 0.125
    assert 0 < rel(one) < 2e-4 and not torch.equal(one, ref) and int((one != ref).sum()) == 1
    tap = ref.clone()
    tap[0, :16, :16, 1] -= 0.125
    assert 2e-4 < rel(tap) < 2.5e-2 and not torch.equal(tap, ref) and int((tap != ref).sum()) == 256
