"""Host checks of tests/mrf_cases.py (no GPU): the restatement of the MRF launchers' decisions agrees with the library's own plan query
(mv_mrf_plan: the dry run of mv_mrf_block_fwd_cl, mv_mrf_chain_fwd_cl and mv_mrf_chain_out_fwd_cl, pure host code) over a sweep of
shapes, types, entries and dilation sets; every plan's partial sums fit the workspace the library asks for; the named shapes of
tests/test_gpu_mrf_arms.py reach the loops they are named for while the older ragged shapes do not; refusals carry their documented
code and leave the plan untouched; and the per-column error that the GPU test bounds sees a one-column defect that the global
rel-L2 of the full-size tests does not."""
import ctypes
import itertools

import pytest
import torch

import mrf_cases as C
from mrf_cases import MV_BF16, MV_F16, MV_F32, MV_F32_W16, MV_F32_W16P, STD

BS = (1, 2, 3, 5, 32, 40, 130, 256)
TS = (1, 15, 16, 17, 48, 100, 127, 128, 129, 200, 255, 256, 257, 511, 512, 513, 600, 700, 1000, 1023, 1024, 1025, 2048, 2049, 3584, 3684,
      4096, 4100, 5000, 8191, 8192, 8193, 10000, 16384, 20000, 32768, 40000, 65536, 100000, 2 ** 23 - 1, 2 ** 23,
      # B x workgroups exactly at and one past the 256 of mrf_geometry, per tile width (B = 1: 256 and 257 tiles of 128, 256, 512 steps),
      # and one column tile past the 256 x 8 wave spans of sr_geometry
      32769, 32896, 65792, 131072, 131584)
ALL_DT = (MV_F32, MV_BF16, MV_F16, MV_F32_W16, MV_F32_W16P)
# one set for every block, and a chain whose blocks differ (hmax and the per-block STD bit)
CHAINS = ((STD,), (STD, STD, STD), ((1, 2, 4), (1, 2, 4)), ((1, 1, 2),), ((1, 3, 7), (1, 3, 7)), ((2, 4, 8), (2, 4, 8), (2, 4, 8)),
          (STD, (1, 2, 4)), ((2, 4, 8), STD, (1, 1, 2)))
UNTOUCHED = [-7] * 20


@pytest.fixture(scope="module")
def L():
    from hifigan_modified import _native
    return _native.lib()


def _ask(L, entry, B, T, dils, dtype, ks=7):
    flat = [d for s in dils for d in s]
    out = (ctypes.c_int * 20)(*UNTOUCHED)
    rc = L.mv_mrf_plan(entry, B, T, len(dils), (ctypes.c_int * len(flat))(*flat), dtype, ks, out)
    return rc, list(out)


def _same(L, entry, B, T, dils, dtype, ks=7):
    """Library plan == restatement for one request; returns the plan as a dict, or None where both refuse with the same code."""
    rc, v = _ask(L, entry, B, T, dils, dtype, ks)
    what = (entry, B, T, dils, C.DT_NAME.get(dtype, dtype), ks)
    try:
        want = C.plan(entry, B, T, dils, dtype, ks)
    except C.Refused as e:
        assert rc == e.code and v == UNTOUCHED, (what, rc, e.code, v)
        return None
    assert rc == 0 and v == [want[k] for k in C.PLAN_FIELDS], (what, rc, dict(zip(C.PLAN_FIELDS, v)), want)
    return want


def test_plan_equals_restatement_over_sweep_and_fits_workspace(L):
    """Every (entry, dtype, chain, B, T) of the sweep: the same refusal or the same plan, field by field; and for every plan
    B * nwg * (32 + 16) floats of partial sums fit mv_mrf_workspace_bytes(B, T, dtype), the region that mrf_chain_ws reserves for them
    (part8 sits B * nwg * 32 floats into it) - for the tile form's nwg and for the streaming form's."""
    seen = set()
    n = 0
    for dt, dils, B, T in itertools.product(ALL_DT, CHAINS, BS, TS):
        entries = (0, 1, 2, 3) if len(dils) == 1 else (1, 2, 3)
        for entry in entries:
            for ks in ((7, 17) if entry == 3 else (7,)):
                p = _same(L, entry, B, T, dils, dt, ks)
                n += 1
                if p is None:
                    continue
                seen.add((p["form"], p["nwaves"], p["ntw"], p["nit"], p["wide"], min(p["tpw"], 9), p["kind"], p["out_family"], p["row_form"]))
                sdt = MV_F32_W16 if dt == MV_F32_W16P else dt
                assert B * p["nwg"] * (32 + 16) * 4 <= L.mv_mrf_workspace_bytes(B, T, sdt), (entry, B, T, dils, dt, p)
                assert p["gx"] == p["nwg"] and p["gy"] == B
    assert n > 20000
    # the sweep reaches every split: nit 1, 2, 4, 8 in each tile form, the wide pass, spans of 1 to more than 8 column tiles, every way
    # a chain ends and every row form the output conv reads
    for arm in ((8, 1), (8, 4), (8, 2)):
        assert {s[3] for s in seen if s[0] == 0 and s[1:3] == arm} == {1, 2, 4, 8}, arm
    assert any(s[4] for s in seen) and {s[5] for s in seen if s[0] == 1} >= set(range(1, 10))
    assert {s[6] for s in seen} == {-1, 0, 1, 2, 3} and {s[8] for s in seen} == {-1, 0, 1, 4} and {s[7] for s in seen} == {-1, 0, 1}


def test_fp32_never_needs_the_4x32_arm(L):
    """mv_mrf_block_fwd_cl and the fp32 chain try <float, 8, 1> and fall back to <float, 4, 2> where its shared tile does not fit
    160 KB.  With halos up to MRF_HMAX = 8 it always fits (138176 + 576 x halo bytes; the wide pass 142272 + 576 x halo), so every
    accepted dilation set runs <float, 8, 1>: the fallback is unreachable from the C ABI, and no GPU test can or needs to cover it."""
    for dil in itertools.product(range(1, 9), repeat=3):
        if C.make_meta(dil) is None:
            continue
        for entry in (0, 1):
            p = _same(L, entry, 40, 3684, (dil,), MV_F32)
            assert (p["nwaves"], p["ntw"], p["nit"]) == (8, 1, 8) and p["lds"] == 138176 + 576 * max(dil) <= C.LDS_MAX
    with pytest.raises(C.Refused):
        C.tile_plan(("float", 8, 1), [(7, 45, False)], True, 1, 16)          # a halo of 45 would be the first that does not fit


def test_named_shapes_reach_their_arms(L):
    """The split shapes of tests/test_gpu_mrf_arms.py show the work split they were chosen for - in the library's plan - and the
    ragged shapes of the older MRF tests all take one tile per worker, which is why the new shapes exist."""
    for B, T in C.OLD_RAGGED:
        for dt, dils in ((MV_F32, (STD,) * 3), (MV_F16, (STD,) * 3), (MV_BF16, (STD,)), (MV_F32_W16, ((1, 2, 4),) * 2)):
            p = _same(L, 1, B, T, dils, dt)
            assert p["form"] == 0 and p["nit"] == 1 and p["wide"] == 0, (B, T, dt, p)
        p = _same(L, 1, B, T, (STD,) * 3, MV_F32_W16)
        assert p["form"] == 1 and p["tpw"] == 1 and p["L"] == 16, (B, T, p)
    for (B, T), arms in C.SPLIT_ARMS.items():
        got = {"fp32": _same(L, 1, B, T, (STD,) * 3, MV_F32), "16bit": _same(L, 1, B, T, (STD,) * 3, MV_F16),
               "w16_tile": _same(L, 1, B, T, ((1, 2, 4),) * 3, MV_F32_W16), "stream": _same(L, 1, B, T, (STD,) * 3, MV_F32_W16)}
        assert _same(L, 1, B, T, (STD,) * 3, MV_BF16)["nit"] == got["16bit"]["nit"]
        for form, want in arms.items():
            assert {k: got[form][k] for k in want} == want, ((B, T), form, got[form])
        assert got["stream"]["form"] == 1 and got["w16_tile"]["form"] == 0
        # the block entry has no wide pass, whatever the shape
        assert _same(L, 0, B, T, (STD,), MV_F32)["wide"] == 0
    # in words, for (40, 3684): tiles of the last workgroup, steps of the last tile, the short span and the idle wave
    B, T = 40, 3684
    nwg, nit = C.mrf_geometry(B, T, 128)
    assert C.cdiv(T, 128) - (nwg - 1) * nit == 5 and T - (C.cdiv(T, 128) - 1) * 128 == 100
    nwg16, nit16 = C.mrf_geometry(B, T, 256)
    assert nwg16 * nit16 - C.cdiv(T, 256) == 1                               # w16 tile form: one idle iteration
    tpw, Ls, nwgs = C.sr_geometry(B, T)
    spans = [min(T, s + Ls) - s for s in range(0, nwgs * 8 * Ls, Ls)]
    assert tpw > 3 and spans.count(Ls) == 46 and spans[46] == 4 and spans[47] <= 0 and len(spans) == 48
    # (40, 3584): 28 tiles, the last workgroup holds 4 = 2 wide iterations of its 4
    assert C.cdiv(3584, 128) - 3 * 8 == 4 and 3584 % 256 == 0
    # the chain + output conv cases of the GPU test: kind, family and rows
    for dt, n, kind, fam, rows in ((MV_F32, 3, C.TAIL_WITH_PARTIALS, 1, C.ROWS_FP32), (MV_F16, 3, C.TAIL_WITH_AB, 0, C.ROWS_FP32),
                                   (MV_BF16, 3, C.TAIL_WITH_AB, 0, C.ROWS_FP32), (MV_F32_W16, 1, C.TAIL_WITH_PARTIALS, 1, C.ROWS_FP32),
                                   (MV_F32_W16, 3, C.TAIL_WITH_PARTIALS, 1, C.ROWS_HL8), (MV_F32_W16P, 3, C.TAIL_WITH_PARTIALS, 1, C.ROWS_PAIR)):
        p = _same(L, 3, 40, 3684, (STD,) * n, dt, 7)
        assert (p["kind"], p["out_family"], p["row_form"]) == (kind, fam, rows), (dt, n, p)
        assert p["launches"] == 2 * n + 1 + (kind == C.TAIL_WITH_AB)
    # the dilation arms: STD false, halo 7 and halo MRF_HMAX, a chain whose blocks differ
    for dil in C.DIL_SETS:
        for dt in (MV_F32, MV_F16, MV_BF16):
            for B, T in C.DIL_SHAPES:
                pb, pc = _same(L, 0, B, T, (dil,), dt), _same(L, 1, B, T, (dil, dil), dt)
                assert pb["std_mask"] == 0 and pc["std_mask"] == 0 and pb["hmax"] == pc["hmax"] == max(dil)
    assert _same(L, 1, 2, 200, (STD, (1, 2, 4)), MV_F32)["std_mask"] == 1
    p = _same(L, 1, 2, 200, (STD, (1, 2, 4)), MV_F32_W16)
    assert p["form"] == 0 and (p["nwaves"], p["ntw"]) == (8, 2) and p["std_mask"] == 1


def test_refusals(L):
    """Documented refusals, each with its code and an untouched plan (checked inside _same)."""
    cases = [
        (0, 2, 200, ((1, 3, 9),), MV_F32, C.MV_ERR_UNSUPPORTED),                 # dilation 9: beyond the prefetch registers
        (1, 2, 200, (STD, (1, 3, 9)), MV_F16, C.MV_ERR_UNSUPPORTED),
        (0, 2, 200, ((0, 1, 2),), MV_F32, C.MV_ERR_UNSUPPORTED),
        (1, 2, 200, ((1, 2, 4),), MV_F32_W16P, C.MV_ERR_UNSUPPORTED),           # pair rows are read by the streaming form only
        (3, 2, 200, (STD,), MV_F32_W16P, C.MV_ERR_UNSUPPORTED, 17),             # a 17-tap output conv takes the tile form
        (1, 1, 2 ** 23, (STD,), MV_F32_W16P, C.MV_ERR_UNSUPPORTED),             # T x 256 bytes reaches 2^31: 32-bit buffer offsets
        (0, 2, 200, (STD,), MV_F32_W16, C.MV_ERR_DTYPE),                         # the block entry has no two-product mode
        (1, 2, 200, (STD,), 9, C.MV_ERR_DTYPE),
        (1, 0, 200, (STD,), MV_F32, C.MV_ERR_ARG), (1, 65536, 200, (STD,), MV_F32, C.MV_ERR_ARG), (1, 2, 0, (STD,), MV_F32, C.MV_ERR_ARG),
        (3, 2, 200, (STD,), MV_F32, C.MV_ERR_ARG, 8),                            # even tap count
        (0, 2, 200, (STD, STD), MV_F32, C.MV_ERR_ARG),
        (1, 2, 200, (STD,) * 9, MV_F32, C.MV_ERR_ARG),
    ]
    for entry, B, T, dils, dt, code, *ks in cases:
        with pytest.raises(C.Refused) as e:
            C.plan(entry, B, T, dils, dt, *ks)
        assert e.value.code == code, (entry, B, T, dils, dt, e.value.code)
        assert _same(L, entry, B, T, dils, dt, *ks) is None
    # three dilations give at most 7 distinct tap offsets, so the 8-offset refusal of mrf_make_meta cannot be reached: every set of
    # dilations in 1 .. 8 is accepted, by every storage type
    for dil in itertools.product(range(1, 9), repeat=3):
        assert C.make_meta(dil) is not None
        for dt in (MV_F32, MV_BF16, MV_F16):
            assert _same(L, 0, 3, 700, (dil,), dt) is not None
    # T x 256 = 2^31 with fp32 rows is not refused: the chain runs its tile form
    p = _same(L, 1, 1, 2 ** 23, (STD,), MV_F32_W16)
    assert p["form"] == 0 and _same(L, 1, 1, 2 ** 23 - 1, (STD,), MV_F32_W16)["form"] == 1


def test_supported_asks_the_plan():
    """MrfFused.supported accepts exactly what the plan accepts: no dilation set reaches a fused entry that would refuse it."""
    import hifigan_modified as H
    from hifigan_modified.fused import MrfFused
    for dil in ((1, 3, 5), (1, 2, 4), (2, 4, 8), (1, 1, 2), (1, 3, 9), (1, 3, 16)):
        blk = H.MultiReceptiveFieldBlock(64, 64, dilations=list(dil))
        assert MrfFused.supported(blk) == (C.make_meta(dil) is not None), dil


def test_per_column_metric_sees_what_global_rel_l2_does_not():
    """One column of 3 x 3684 off by 1e-3 of its rms in all 64 channels, on top of the two-product mode's own error (the simulation
    of the three-block w16 chain): the global rel-L2 moves by about 1e-3 / sqrt(3684) and stays inside the 4e-4 of the full-size
    tests; the per-column maximum leaves MARGIN x the simulation's own maximum."""
    import numerics_sim as S
    from oracle import vocoder_oracle as O
    T = 3684
    _, sds = S.mrf_blocks(0)
    x = C.base_clips(T)
    with torch.no_grad():
        ref = x.double()
        for sd in sds:
            ref = O.mrf_block(ref, {k: v.double() for k, v in sd.items()}, "")
        sim = S.chain_sim(x, sds, 3, "w16")
    e_sim = C.column_error(sim, ref)
    norms = ref[1].pow(2).sum(0).sqrt()
    t = int((norms - norms.median()).abs().argmin())                       # a column of typical size, in the middle clip
    bad = sim.clone()
    bad[1, :, t] += 1e-3 * ref[1, :, t].pow(2).mean().sqrt().float()
    e_bad = C.column_error(bad, ref)
    g_sim, g_bad = C.rel_l2(sim, ref), C.rel_l2(bad, ref)
    ratio = float(e_sim.max() / e_sim.pow(2).mean().sqrt())
    print(f"[mrf-metric] global sim {g_sim:.3e} defect {g_bad:.3e}; per-column max sim {float(e_sim.max()):.3e} defect {float(e_bad.max()):.3e} "
          f"at t={int(e_bad[1].argmax())}; max / rms of the simulation's per-column error {ratio:.2f}")
    assert g_bad < 4e-4 and g_bad - g_sim < 2e-5                           # the full-size check accepts the defect
    assert float(e_bad.max()) > C.MARGIN * float(e_sim.max())              # the per-column check rejects it
    assert int(e_bad[1].argmax()) == t and float(e_sim.max()) <= C.MARGIN * float(e_sim.max())
    assert ratio < 2.5                                                     # the factor behind the three-product bound 5e-5 = 2e-5 x 2.5
