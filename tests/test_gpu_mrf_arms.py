"""The fused MultiReceptiveFieldBlock kernels (csrc/mrf_fused.hip, csrc/mrf_stream.hip) and the chain's fused ending
(csrc/conv_out.hip) per work split and per dilation arm, against the fp64 oracle (oracle/vocoder_oracle.py: grc_lora.py:32-68,
:157-163) on the same, already rounded, input.  tests/mrf_cases.py holds the shapes and says which loop each one reaches; every case
asks the library's plan (mv_mrf_plan) before it calls a fused entry and holds it against the restatement.

Every batch is three distinct seeded clips tiled along B, and the oracle runs on the three clips only.  Every case asserts
  * copies of a clip are bit-identical to its first copy (each sample has its own workgroups and partial-sum slots),
  * two runs are bit-identical,
  * the PER-COLUMN error of the first copies, e[b, t] = ||y[b, :, t] - ref[b, :, t]|| / sqrt(mean_t ||ref[b, :, t]||^2): a wrong halo
    column at a seam between two workers moves a global rel-L2 over T columns by 1 / sqrt(T) of itself
    (tests/test_host_mrf_plan.py shows a defect the full-size checks accept and this one rejects).
Bounds.  Two-product and 16-bit modes: max e_gpu <= 1.5 x max e_sim, e_sim the per-column error of the CPU simulation of the mode's own
roundings (tests/numerics_sim.py::chain_sim) on the same clips, 1.5 the MARGIN of tests/test_gpu_inference_off_unit_scale.py; and the
project's global rel-L2 (4e-4 two-product; 1.5e-3 fp16 and 8e-3 bf16 for single blocks).  Three-product fp32: the simulation has no
accumulation error, so 5e-5 per column = the global 2e-5 of test_mrf_fused_vs_generic_and_golden x 2.5, the ratio of maximum to rms of
per-column rounding noise with room (measured 1.6 - 2.1 on the CPU), and 2e-5 globally.  Every figure is printed before it is
asserted, with the worst column, whether it lies within one halo of a boundary between two workers' spans, and the same figure at
B = 3 of the same clips (the one-tile split that the older tests pin): a ratio that grows with the split points at a seam.

Measured on an MI355X (max per-column error; GPU / simulation where a simulation bounds the mode): the docstrings of the tests.  No
ratio at a split shape exceeds the one at B = 3 of the same clips: they agree to the third digit in every mode.  What the tests did
find: a keep-mask of ones did not reproduce the maskless call bit for bit in fp32 (the compiler fused other multiply-adds in the masked
than in the maskless instantiation of pass 3's last stage); that stage now spells its fmas out (csrc/mrf_fused.hip, stage4)."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mrf_cases as C                         # noqa: E402
import numerics_sim as S                      # noqa: E402
from oracle import vocoder_oracle as O        # noqa: E402

pytestmark = pytest.mark.gpu

STD = C.STD
KS = 7
_MEMO = {}


def _memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


@pytest.fixture(scope="module")
def N():
    import hifigan_modified  # noqa: F401
    from hifigan_modified import _native
    _native.lib()
    return _native


# ------------------------------------------------------------------------------------------------ blocks, references, simulations
def _cpu_blocks(dil):
    return _memo(("cpu", dil), lambda: S.mrf_blocks(0, dilations=dil))


def _sds(dils):
    """State dicts of a chain whose block i has the dilations dils[i]: block i of the three seeded blocks built with that set."""
    return [_cpu_blocks(d)[1][i] for i, d in enumerate(dils)]


def _fused(dils):
    from hifigan_modified.fused import mrf_fused_for
    return [_memo(("gpu", d, i), lambda d=d, i=i: mrf_fused_for(_cpu_blocks(d)[0][i].cuda().train(False))) for i, d in enumerate(dils)]


def _chain(dils):
    from hifigan_modified.fused import MrfChain
    return _memo(("chain", dils), lambda: MrfChain(_fused(dils)))


_ROUND = {"fp32": lambda x: x, "fp16": lambda x: S.EB.q(x, "fp16"), "bf16": lambda x: S.EB.q(x, "bf16"), "pair": S.pair}
# chain mode -> (how the input is rounded before anything sees it, mode code, MrfChain keywords, torch storage type)
MODES = {"three": ("fp32", C.MV_F32, {}, torch.float32), "fp16": ("fp16", C.MV_F16, {}, torch.float16),
         "bf16": ("bf16", C.MV_BF16, {}, torch.bfloat16), "w16": ("fp32", C.MV_F32_W16, dict(w16=True), torch.float32),
         "w16_pair": ("pair", C.MV_F32_W16P, dict(w16=True, x_pair=True), torch.float32),
         "w16_tile": ("fp32", C.MV_F32_W16, dict(w16=True), torch.float32)}


def _input(T, rnd):
    return _memo(("x", T, rnd), lambda: _ROUND[rnd](C.base_clips(T)))


def _oracle(T, dils, rnd):
    """fp64 oracle outputs after block 1 .. len(dils) on the three clips, input rounded as `rnd` says."""
    def run():
        cur, outs = _input(T, rnd).double(), []
        with torch.no_grad():
            for sd, d in zip(_sds(dils), dils):
                cur = O.mrf_block(cur, {k: v.double() for k, v in sd.items()}, "", dilations=d)
                outs.append(cur)
        return outs
    return _memo(("ref", T, dils, rnd), run)


def _sim(T, dils, mode, n):
    """chain_sim of the first n blocks in `mode` on the three clips (None for the three-product mode: its bound is absolute)."""
    if mode == "three":
        return None
    x, sds = C.base_clips(T), _sds(dils)
    if mode == "w16" or n == 1:
        return _memo(("sim", T, dils, mode, n), lambda: S.chain_sim(x, sds, n, mode, dilations=dils))
    # every other mode stores all its rows alike, so n blocks continue the simulation of n - 1
    return _memo(("sim", T, dils, mode, n), lambda: S.chain_sim(_sim(T, dils, mode, n - 1), sds[n - 1:], 1, mode, dilations=dils[n - 1:]))


def _pair_rows(x_cl):
    B, T, Cc = x_cl.shape
    g = x_cl.view(B, T, Cc // 8, 8)
    hi = g.to(torch.float16)
    lo = (g - hi.float()).to(torch.float16)
    return torch.stack([hi, lo], dim=3).contiguous().view(torch.float32).view(B, T, Cc)


def _to_gpu(x3, B, mode):
    """[3, 64, T] clips -> the channels-last batch of B the entry takes in `mode`."""
    rnd, _, _, dt = MODES[mode]
    xc = C.tile_batch(x3, B).cuda().transpose(1, 2).contiguous()
    return _pair_rows(xc) if rnd == "pair" else xc.to(dt)


def _ask(N, entry, B, T, dils, dt, ks=KS):
    """The library's plan for the call that follows, held against the restatement; a refusal here is a defect."""
    flat = [d for s in dils for d in s]
    out = (ctypes.c_int * 20)()
    rc = N.lib().mv_mrf_plan(entry, B, T, len(dils), (ctypes.c_int * len(flat))(*flat), dt, ks, out)
    assert rc == 0, (entry, B, T, dils, dt, rc)
    p = dict(zip(C.PLAN_FIELDS, list(out)))
    assert p == C.plan(entry, B, T, dils, dt, ks), (p, C.plan(entry, B, T, dils, dt, ks))
    return p


def _twice(run, B):
    """Run twice: bit-identical; copies of a clip bit-identical to its first copy.  -> first copies as [3 or B, C, T] fp32 on the CPU."""
    with torch.no_grad():
        y, y2 = run(), run()
    assert torch.equal(y, y2), "two runs differ"
    if B > 3:
        assert torch.equal(y[3:], y[torch.arange(3, B, device=y.device) % 3]), "copies of a clip differ"
    y = y[:3]
    return (y if y.shape[1] == 1 else y.transpose(1, 2)).float().cpu()


def _judge(tag, y, ref, sim, mode, p, T, single_block, y3=None):
    """Print and return the failures of one output: per-column maximum against MARGIN x the simulation's (absolute for the
    three-product mode), global rel-L2 against the project's bound where it has one."""
    nb = y.shape[0]
    ref = ref[:nb]
    e = C.column_error(y, ref)
    g = C.rel_l2(y, ref)
    b, t = divmod(int(e.argmax()), T)
    seam = C.seam_distance(t, p, T)
    if sim is None:
        cb, gb, es = C.THREE_COL, C.THREE_GLOBAL, None
    else:
        es = float(C.column_error(sim[:nb], ref).max())
        cb = C.MARGIN * es
        gb = C.GLOBAL_BOUND[mode] if (mode.startswith("w16") or single_block) else None
    e3 = "" if y3 is None else f" | B=3: max col {float(C.column_error(y3, ref).max()):.3e}"
    print(f"[mrf-arms] {tag}: global {g:.3e} (bound {gb}) max col {float(e.max()):.3e} bound {cb:.3e}"
          + ("" if es is None else f" sim {es:.3e} ratio {float(e.max()) / es:.2f}")
          + f" worst b={b} t={t} {'within' if seam <= p['hmax'] else 'outside'} one halo of a span boundary (distance {seam}){e3}")
    fails = []
    if not bool(torch.isfinite(y).all()):
        fails.append((tag, "not finite"))
    if not float(e.max()) <= cb:
        fails.append((tag, "column", float(e.max()), cb, (b, t)))
    if gb is not None and not g <= gb:
        fails.append((tag, "global", g, gb))
    return fails


def _head():
    """The 7 central taps of the 11-tap head of tests/test_gpu_inference_off_unit_scale.py::_head (seed 3, He scale), bias 0."""
    torch.manual_seed(3)
    w = torch.randn(1, 64, 11) * (2.0 / 11) ** 0.5
    return w[:, :, 2:9].contiguous()


def _pack_head(N, w):
    from hifigan_modified import ops
    w = w.cuda().contiguous()
    wt = torch.empty(N.lib().mv_conv_out_packed_bytes(64, w.shape[2]), device="cuda", dtype=torch.uint8)
    N.call("mv_conv_out_pack_all", ctypes.c_void_p(w.data_ptr()), ops._DT[w.dtype], ctypes.c_void_p(wt.data_ptr()), 64, w.shape[2], ops._stream())
    return wt


# ------------------------------------------------------------------------------------------------ 1. split shapes
@pytest.mark.parametrize("dt", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("B,T", C.SPLIT_SHAPES)
def test_block_entry_split_shapes(N, B, T, dt):
    """mv_mrf_block_fwd_cl where a workgroup walks several tiles: (40, 3684) fp32 nit 8 with a 5-tile last workgroup and a 100-step
    last tile, 16-bit nit 2; (40, 3584) the same splits on whole tiles; (130, 600) fp32 nit 4 with three idle iterations, 16-bit one
    workgroup of two tiles.

    Measured on an MI355X, max per-column error at (40, 3684) | (40, 3584) | (130, 600), and the same at B = 3 of the same clips:
      fp32  7.87e-6 | 7.68e-6 | 6.34e-6 (B = 3: 7.86e-6 | 7.68e-6 | 6.33e-6), global 3.9e-6; worst columns t = 44, 2700, 472
      fp16  5.37e-4 | 5.34e-4 | 4.93e-4 = 1.00 x the simulation at every shape and at B = 3 (global 2.9e-4)
      bf16  4.19e-3 | 4.30e-3 | 3.98e-3 = 1.00 x the simulation at every shape and at B = 3 (global 2.4e-3)
    The worst column lies within one halo of a tile boundary in 5 of the 9 cases, about what chance gives with 16-step wave tiles."""
    mode = "three" if dt == "fp32" else dt
    rnd, code, _, tdt = MODES[mode]
    p = _ask(N, 0, B, T, (STD,), code)
    want = C.SPLIT_ARMS[(B, T)]["fp32" if dt == "fp32" else "16bit"]
    assert {k: p[k] for k in want if k != "wide"} == {k: v for k, v in want.items() if k != "wide"} and p["wide"] == 0
    fz = _fused((STD,))[0]
    x3 = _input(T, rnd)
    xb, x3g = _to_gpu(x3, B, mode), _to_gpu(x3, 3, mode)
    y = _twice(lambda: fz.forward_cl(xb), B)
    y3 = _twice(lambda: fz.forward_cl(x3g), 3)
    fails = _judge(f"block {dt} B={B} T={T} nit={p['nit']} nwg={p['nwg']}", y, _oracle(T, (STD,) * 3, rnd)[0], _sim(T, (STD,) * 3, mode, 1), mode, p, T, True, y3)
    assert not fails, fails


@pytest.mark.parametrize("mode", ["three", "fp16", "bf16", "w16", "w16_pair", "w16_tile"])
@pytest.mark.parametrize("B,T", C.SPLIT_SHAPES)
def test_chain_split_shapes(N, B, T, mode):
    """mv_mrf_chain_fwd_cl, 1 and 3 blocks, materialised, in the three-product, fp16, bf16 and two-product modes (fp32 rows and pair
    rows in: the streaming form; dilations (1, 2, 4): the f32w16 tile form), where a worker walks several tiles:
      (40, 3684)  fp32 nit 8, last workgroup 5 tiles, last tile 100 steps; 16-bit nit 2; w16 tile form nit 4 with one idle iteration;
                  streaming tpw 5 (the ring of three slots wraps), one span of 4 steps, one idle wave
      (40, 3584)  the fp32 chain's wide first pass, whose last workgroup runs 2 of its 4 wide iterations
      (130, 600)  fp32 nit 4 with three idle iterations; streaming one workgroup per sample, spans of 5, the last wave 3 tiles

    Measured on an MI355X - max per-column error, GPU / simulation = ratio, n = 1 | n = 3; the B = 3 figure agrees with the split
    shape's to the third digit in every line (largest difference: three-product n = 3 at (130, 600), 9.28e-6 against 9.06e-6):
      (40, 3684)  three 7.24e-6 | 9.88e-6;  fp16 5.76e-4 / 5.37e-4 = 1.07 | 9.12e-4 / 8.39e-4 = 1.09;  bf16 1.10 | 1.07;
                  w16 3.018e-4 / 3.013e-4 = 1.00 | 5.054e-4 / 5.049e-4 = 1.00;  w16_pair 1.00 | 1.00;  w16_tile 1.00 | 1.00
      (40, 3584)  three 7.29e-6 | 9.90e-6 (wide);  fp16 1.05 | 1.06;  bf16 1.14 | 1.10;  w16, w16_pair, w16_tile 1.00 | 1.00
      (130, 600)  three 6.00e-6 | 9.28e-6;  fp16 1.12 | 1.18;  bf16 1.10 | 1.15;  w16, w16_pair, w16_tile 1.00 | 1.00
    (the 16-bit chains store f in 16 bits between pass B and pass A, which the simulation does not round: hence 1.05 - 1.18, at
    B = 3 as well.)  Worst columns: t = 2898 (18 steps from a span boundary) in every two-product mode at (40, 3684), t = 592 at the
    other two shapes - the same column in the streaming and in the tile form, so it belongs to the clip, not to a seam."""
    rnd, code, kw, tdt = MODES[mode]
    dil = (1, 2, 4) if mode == "w16_tile" else STD
    form = {"three": "fp32", "fp16": "16bit", "bf16": "16bit", "w16": "stream", "w16_pair": "stream", "w16_tile": "w16_tile"}[mode]
    x3 = _input(T, "fp32")                                     # _to_gpu rounds it as the mode's entry stores it
    xb, x3g = _to_gpu(x3, B, mode), _to_gpu(x3, 3, mode)
    fails = []
    for n in (1, 3):
        dils = (dil,) * n
        p = _ask(N, 1, B, T, dils, code)
        want = C.SPLIT_ARMS[(B, T)][form]
        assert {k: p[k] for k in want} == want and p["form"] == (1 if form == "stream" else 0), (p, want)
        chain = _chain((dil,) * 3)
        y = _twice(lambda: chain.forward_cl(xb, n, **kw), B)
        y3 = _twice(lambda: chain.forward_cl(x3g, n, **kw), 3)
        tag = f"chain {mode} n={n} B={B} T={T} " + (f"tpw={p['tpw']} nwg={p['nwg']}" if p["form"] else f"nit={p['nit']} nwg={p['nwg']} wide={p['wide']}")
        fails += _judge(tag, y, _oracle(T, (dil,) * 3, rnd)[n - 1], _sim(T, (dil,) * 3, mode, n), mode, p, T, n == 1, y3)
    assert not fails, fails


@pytest.mark.parametrize("case", ["fp32", "fp16", "bf16", "w16_n1", "w16_n3", "w16_pair"])
def test_chain_out_split_shape(N, case):
    """mv_mrf_chain_out_fwd_cl at (40, 3684) with a 7-tap linear head (ACT_NONE: what is compared is the chain's output seen through
    the conv, not a saturated tanh), against the fp64 conv1d of the oracle chain:
      fp32      TAIL_WITH_PARTIALS, fp32 rows, the nwg of an nit = 8 grid summed by conv_out_affine_mfma_kernel
      fp16/bf16 TAIL_WITH_AB: mrf_affine_kernel + conv_out_affine_kernel<T>
      w16_n1    streaming, one block: fp32 rows;  w16_n3: hl8 rows;  w16_pair: pair rows.

    Measured on an MI355X, max per-column error (one waveform sample against the rms of the waveform), GPU / simulation, B = 40 | B = 3:
      fp32 3.36e-5 | 3.27e-5 (bound 5e-5; global 8.3e-6);  fp16 3.00e-3 / 2.20e-3 = 1.37 | 1.37;  bf16 2.25e-2 / 2.12e-2 = 1.06 | 1.06;
      w16_n1 6.68e-4 / 6.69e-4 = 1.00;  w16_n3 1.175e-3 / 1.163e-3 = 1.01;  w16_pair 1.163e-3 / 1.170e-3 = 0.99"""
    B, T = 40, 3684
    mode, n = {"fp32": ("three", 3), "fp16": ("fp16", 3), "bf16": ("bf16", 3), "w16_n1": ("w16", 1), "w16_n3": ("w16", 3), "w16_pair": ("w16_pair", 3)}[case]
    rnd, code, kw, tdt = MODES[mode]
    dils = (STD,) * n
    p = _ask(N, 3, B, T, dils, code, KS)
    want = {"fp32": (C.TAIL_WITH_PARTIALS, 1, C.ROWS_FP32), "fp16": (C.TAIL_WITH_AB, 0, C.ROWS_FP32), "bf16": (C.TAIL_WITH_AB, 0, C.ROWS_FP32),
            "w16_n1": (C.TAIL_WITH_PARTIALS, 1, C.ROWS_FP32), "w16_n3": (C.TAIL_WITH_PARTIALS, 1, C.ROWS_HL8),
            "w16_pair": (C.TAIL_WITH_PARTIALS, 1, C.ROWS_PAIR)}[case]
    assert (p["kind"], p["out_family"], p["row_form"]) == want, p
    assert p["nit"] == 8 or case != "fp32"
    w = _head()
    wt = _pack_head(N, w)
    from hifigan_modified.fused import MrfChain
    chain = MrfChain(_fused((STD,) * 3)[:n])
    x3 = _input(T, "fp32")
    xb, x3g = _to_gpu(x3, B, mode), _to_gpu(x3, 3, mode)
    y = _twice(lambda: chain.forward_out_cl(xb, wt, 0.0, KS, N.ACT_NONE, **kw), B)
    y3 = _twice(lambda: chain.forward_out_cl(x3g, wt, 0.0, KS, N.ACT_NONE, **kw), 3)
    assert y.shape == (3, 1, T)
    ref = F.conv1d(_oracle(T, (STD,) * 3, rnd)[n - 1], w.double(), padding=KS // 2)
    sim = _sim(T, (STD,) * 3, mode, n)
    if mode in ("fp16", "bf16"):                              # 16-bit rows, the fp32 weight image, a 16-bit waveform
        sim = S.EB.q(F.conv1d(sim, w, padding=KS // 2), mode)
    elif sim is not None:                                     # fp32 storage: hi + lo bf16 operands on both sides
        sim = F.conv1d(S.EB.q(sim, "bf16x2"), S.EB.q(w, "bf16x2"), padding=KS // 2)
    fails = _judge(f"chain+out {case} B={B} T={T}", y, ref, sim, mode, p, T, False, y3)
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ 2. dilation arms
@pytest.mark.parametrize("dt", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("dil", C.DIL_SETS)
@pytest.mark.parametrize("B,T", C.DIL_SHAPES)
def test_dilation_arms(N, B, T, dil, dt):
    """The STD = false instantiations of mrf_kernel (tap table read from MrfMeta at run time) in every storage type, block entry and a
    2-block chain: (1, 2, 4); (1, 1, 2), the fewest taps; (1, 3, 7), halo 7; (2, 4, 8), halo MRF_HMAX = 8, what the prefetch
    registers are sized for.  B = 2 runs the first two of the three clips.

    Measured on an MI355X: fp32 6.1e-6 .. 7.5e-6 (block), 7.8e-6 .. 1.0e-5 (chain) per column, global 3.9e-6 / 4.8e-6; the 16-bit block
    entries 0.95 .. 1.00 x the simulation, the 16-bit chains 1.00 .. 1.26 (bf16, (2, 4, 8), T = 200) for the unmodelled 16-bit f."""
    mode = "three" if dt == "fp32" else dt
    rnd, code, _, tdt = MODES[mode]
    dils = (dil, dil)
    pb, pc = _ask(N, 0, B, T, (dil,), code), _ask(N, 1, B, T, dils, code)
    assert pb["std_mask"] == 0 and pc["std_mask"] == 0 and pb["hmax"] == max(dil)
    x3 = _input(T, "fp32")
    xb = _to_gpu(x3, B, mode)
    ref, fails = _oracle(T, dils, rnd), []
    y = _twice(lambda: _fused(dils)[0].forward_cl(xb), B)
    fails += _judge(f"block {dt} dil={dil} B={B} T={T}", y, ref[0], _sim(T, dils, mode, 1), mode, pb, T, True)
    y = _twice(lambda: _chain(dils).forward_cl(xb, 2), B)
    fails += _judge(f"chain {dt} n=2 dil={dil} B={B} T={T}", y, ref[1], _sim(T, dils, mode, 2), mode, pc, T, False)
    assert not fails, fails


@pytest.mark.parametrize("mode", ["three", "fp16", "w16_tile"])
@pytest.mark.parametrize("B,T", C.DIL_SHAPES)
def test_chain_with_differing_blocks(N, B, T, mode):
    """Block 0 at (1, 3, 5), block 1 at (1, 2, 4): per-block STD (pass A of block 1 applies block 0's affine with its own tap table),
    hmax of the chain; in the two-product mode the chain leaves the streaming form for the f32w16 tile form."""
    rnd, code, kw, tdt = MODES[mode]
    dils = (STD, (1, 2, 4))
    p = _ask(N, 1, B, T, dils, code)
    assert p["form"] == 0 and p["std_mask"] == 1 and p["hmax"] == 5
    xb = _to_gpu(_input(T, "fp32"), B, mode)
    y = _twice(lambda: _chain(dils).forward_cl(xb, 2, **kw), B)
    fails = _judge(f"chain {mode} (1,3,5)+(1,2,4) B={B} T={T}", y, _oracle(T, dils, rnd)[1], _sim(T, dils, mode, 2), mode, p, T, False)
    assert not fails, fails


def test_halo7_fp32_with_eight_tiles_per_workgroup(N):
    """(1, 3, 7) at (40, 3684) in fp32: STD = false with nit = 8 and a 5-tile last workgroup, block entry and 2-block chain.  (The plan
    shows <float, 8, 1>: the <float, 4, 2> fallback is unreachable, tests/test_host_mrf_plan.py.)"""
    B, T, dil = 40, 3684, (1, 3, 7)
    dils = (dil, dil)
    pb, pc = _ask(N, 0, B, T, (dil,), C.MV_F32), _ask(N, 1, B, T, dils, C.MV_F32)
    assert (pb["nwaves"], pb["ntw"], pb["nit"], pb["std_mask"], pb["hmax"]) == (8, 1, 8, 0, 7) and pc["nit"] == 8
    xb = _to_gpu(_input(T, "fp32"), B, "three")
    ref, fails = _oracle(T, dils, "fp32"), []
    fails += _judge("block fp32 dil=(1,3,7) B=40 T=3684", _twice(lambda: _fused(dils)[0].forward_cl(xb), B), ref[0], None, "three", pb, T, True)
    fails += _judge("chain fp32 n=2 dil=(1,3,7) B=40 T=3684", _twice(lambda: _chain(dils).forward_cl(xb, 2), B), ref[1], None, "three", pc, T, False)
    assert not fails, fails


def test_unsupported_dilations_fall_back_to_the_generic_path(N):
    """A dilation set the plan refuses (9 > MRF_HMAX) is refused by MrfFused.supported too, so Fn.mrf_block runs the generic kernels:
    no fused object, and the result is the forced-generic one bit for bit."""
    import hifigan_modified as H
    from hifigan_modified import functional as Fn
    from hifigan_modified.fused import MrfFused, mrf_fused_for
    out = (ctypes.c_int * 20)()
    assert N.lib().mv_mrf_plan(0, 2, 200, 1, (ctypes.c_int * 3)(1, 3, 9), C.MV_F32, 0, out) == C.MV_ERR_UNSUPPORTED
    torch.manual_seed(0)
    blk = H.MultiReceptiveFieldBlock(64, 64, dilations=[1, 3, 9]).cuda().train(False)
    assert not MrfFused.supported(blk) and mrf_fused_for(blk) is None
    x = torch.randn(2, 64, 200, device="cuda")
    with torch.no_grad():
        y, yg = Fn.mrf_block(x, blk), Fn.mrf_block(x, blk, force_generic=True)
        ref = O.mrf_block(x.cpu().double(), {k: v.detach().cpu().double() for k, v in blk.state_dict().items()}, "", dilations=(1, 3, 9))
    assert torch.equal(y, yg) and O.rel_l2(y.cpu(), ref) < 1e-4
    for dil in ((1, 2, 4), (2, 4, 8)):
        assert MrfFused.supported(H.MultiReceptiveFieldBlock(64, 64, dilations=list(dil)))


# ------------------------------------------------------------------------------------------------ 3. the dropout-mask arguments
@pytest.mark.parametrize("dt", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("B,T", [(3, 700), (40, 3684)])
def test_block_entry_dropout_mask(N, B, T, dt):
    """mv_mrf_block_fwd_cl's dropout_mask / mask_scale (part of the ABI; the Python path sends training dropout to the generic
    kernels, so nothing else calls them): keep-mask of mv_dropout_mask(p = 0.1) for the three clips, tiled like the clips, scale
    1 / 0.9, against fp64 GN8(f) * mask * scale + x; and a mask of ones with scale 1 equals the maskless call bit for bit.

    Measured on an MI355X, max per-column error at (3, 700) | (40, 3684): fp32 7.3e-6 | 8.2e-6; fp16 1.01 | 1.00 and bf16 1.00 | 1.00 x
    the simulation.  The mask of ones failed in fp32 before stage 4 spelled out its fmas (module docstring); fp16 and bf16 passed."""
    from hifigan_modified import ops
    mode = "three" if dt == "fp32" else dt
    rnd, code, _, tdt = MODES[mode]
    p = _ask(N, 0, B, T, (STD,), code)
    fz = _fused((STD,))[0]
    x3 = _input(T, rnd)
    xb = _to_gpu(x3, B, mode)
    m3 = torch.empty(3, T, 64, device="cuda", dtype=torch.uint8)
    N.call("mv_dropout_mask", ctypes.c_void_p(m3.data_ptr()), m3.numel(), 0.1, 1234 + T, ops._stream())
    keep = float(m3.float().mean())
    assert set(m3.unique().tolist()) == {0, 1} and abs(keep - 0.9) < 0.01, keep
    mb = m3[torch.arange(B, device="cuda") % 3].contiguous()
    scale = 1.0 / 0.9
    y = _twice(lambda: fz.forward_cl(xb, mask=mb, mask_scale=scale), B)
    mc = m3.transpose(1, 2).cpu()                                  # [3, 64, T]
    sd = {k: v.double() for k, v in _sds((STD,))[0].items()}
    with torch.no_grad():
        ref = O.mrf_block(x3.double(), sd, "", dropout_mask=mc.double(), dropout_p=0.1)
    sim = None
    if mode != "three":
        xq = x3                                                    # already rounded
        n = S.EB.mrf_forward(xq, _sds((STD,))[0], "", STD, mode, mode, "fp32") - xq
        sim = S.EB.q(n * mc.float() * scale + xq, mode)
    fails = _judge(f"block {dt} masked B={B} T={T} keep={keep:.4f}", y, ref, sim, mode, p, T, True)
    ones = torch.ones_like(mb)
    with torch.no_grad():
        assert torch.equal(fz.forward_cl(xb, mask=ones, mask_scale=1.0), fz.forward_cl(xb)), "a mask of ones changes the output"
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ 4. older ragged shapes, for the record
def test_older_ragged_shapes_take_one_tile_per_worker(N):
    """Why the split shapes exist: every ragged (B, T) of test_gpu_mrf_stream.py and the scale / offset sweeps plans nit = 1 and tpw = 1."""
    for B, T in C.OLD_RAGGED:
        assert _ask(N, 1, B, T, (STD,) * 3, C.MV_F32)["nit"] == 1 and _ask(N, 1, B, T, (STD,) * 3, C.MV_F16)["nit"] == 1
        assert _ask(N, 1, B, T, (STD,) * 3, C.MV_F32_W16)["tpw"] == 1
