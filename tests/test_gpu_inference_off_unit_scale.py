"""Inference parity away from the operating point of the published figures (a seeded default-init generator fed randn, whose waveform
is 97 % saturated, whose GroupNorm inputs have zero group mean and whose MRF stream sits at one scale): a head calibrated to an
unsaturated pre-tanh signal, log-mel input, the MRF chain on streams scaled by 2^-12 .. 2^8, GroupNorm inputs whose group mean is up
to 100 x their std, and ODConv attention near one-hot.

References are the oracle in fp64.  Bounds: a split / mixed / 16-bit mode may not exceed the CPU simulation of its own roundings
(tests/numerics_sim.py over tools/error_budget.py) on the same clips by more than a margin - what must be caught is a kernel that is
worse than its format; the fp32 modes keep their unit-scale bounds; the GroupNorm sweep is bounded by max(unit-scale bound of the
path, 4 x the error of the fp32 two-pass oracle against fp64) - the factor 4 is for summation order plus the operand rounding that
the unit-scale bound already holds.  Every figure is printed before it is asserted."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numerics_sim as S                      # noqa: E402
from oracle import vocoder_oracle as O        # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 1.5          # GPU error <= MARGIN x simulated error of the mode's own roundings (chain entries: measured 0.97 .. 1.25)
# full generator, calibrated head: 1.25 x the worst measured GPU / simulation ratio of the mode (any of waveform, mrf2, pre-tanh, on
# randn or log-mel input): mixed_up0 1.17, mixed_up1 1.11, headline 1.10, fp16 1.04, bf16 1.09
MODE_MARGIN = {"mixed_up0": 1.46, "mixed_up1": 1.39, "headline": 1.38, "fp16": 1.30, "bf16": 1.36}
NORTH_STAR = 1e-3


@pytest.fixture(scope="module")
def H():
    import hifigan_modified as H
    from hifigan_modified import _native
    _native.lib()
    return H


def _f64(sd):
    return {k: v.double() for k, v in sd.items()}


def _blocks(H, seed=0):
    return S.mrf_blocks(seed)


def _head(H, seed=3):
    torch.manual_seed(seed)
    w = torch.randn(1, 64, 11) * (2.0 / 11) ** 0.5
    return {"output_proj.weight": w, "output_proj.bias": torch.zeros(1)}


def _pack_head(sd, device="cuda"):
    """(packed fp32 | bf16 | f16 images, bias) of an output conv - what GeneratorFused.out_weights hands to the chain."""
    from hifigan_modified import _native as N, ops
    w = sd["output_proj.weight"].to(device).contiguous()
    C, ks = w.shape[1], w.shape[2]
    wt = torch.empty(N.lib().mv_conv_out_packed_bytes(C, ks), device=device, dtype=torch.uint8)
    N.call("mv_conv_out_pack_all", ctypes.c_void_p(w.data_ptr()), ops._DT[w.dtype], ctypes.c_void_p(wt.data_ptr()), C, ks, ops._stream())
    return wt, float(sd["output_proj.bias"].item())


# ================================================================================================ 1. calibrated head, full C2 size
CLIPS = (0, 7, 13, 31)             # the clips of the existing full-size tests; 0 and 7 are the batch of 2 of the stage-wise entry
HEAD_RMS = 0.3


@pytest.fixture(scope="module")
def c2(H):
    """Per input kind: the B=32 x 32-frame batch, the head calibrated on the oracle's pre-tanh signal of the test clips (zero mean,
    rms 0.3) and the fp64 oracle stages of those clips under that head."""
    out = {}
    for kind in ("randn", "logmel"):
        gen, sd = S.default_generator_sd(0)
        torch.manual_seed(1)
        mel, spk, emo = torch.randn(32, 80, 32), torch.randn(32, 192), torch.randn(32, 384)
        if kind == "logmel":
            mel = S.logmel_like(32, 32)
        idx = list(CLIPS)
        with torch.no_grad():
            ref = O.generator_forward(mel[idx].double(), _f64(sd), "", spk[idx].double(), emo[idx].double(), return_stages=True)
            cal = S.calibrate_head(sd, ref["output_proj"], HEAD_RMS)
            w, b = cal["output_proj.weight"].double(), cal["output_proj.bias"].double()
            pre = F.conv1d(ref["mrf2"], w, b, padding=w.shape[2] // 2)
        ref = dict(mrf2=ref["mrf2"], output_proj=pre, wave=torch.tanh(pre))
        sat = float((ref["wave"].abs() > 0.99).double().mean())
        print(f"[off-rail] {kind}: pre-tanh mean {float(pre.mean()):+.1e} rms {float(pre.pow(2).mean().sqrt()):.3f}, |wave| > 0.99: {sat:.3f}")
        assert sat <= 0.05
        gen.load_state_dict(cal)
        out[kind] = dict(gen=gen.cuda().train(False), sd=cal, mel=mel, spk=spk, emo=emo, ref=ref)
    return out


def _set_mode(gen, mode):
    """-> storage dtype of the inputs."""
    gen.set_mixed_precision(None)
    if mode in ("mixed_up0", "mixed_up1"):
        gen.set_mixed_precision(mode[-3:])
    elif mode == "headline":
        gen.set_mixed_precision("up1", mrf_weights="fp16")
    return {"fp16": torch.float16, "bf16": torch.bfloat16}.get(mode, torch.float32)


@pytest.mark.parametrize("kind", ["randn", "logmel"])
@pytest.mark.parametrize("mode", S.MODES)
def test_calibrated_head_full_c2(H, c2, mode, kind):
    """Every inference mode at BASELINE configs[1]'s full size with the head calibrated to a pre-tanh rms of 0.3 (no saturated
    samples: the waveform error IS the pre-tanh error), on randn and on log-mel input, against the fp64 oracle: the waveform of
    clips 0, 7, 13, 31; mrf2 and the pre-tanh signal (atanh of the waveform - the stage entry does not expose it - on both sides)
    of the stage-wise entry on a batch of 2; bit-identical reruns.  all-fp32: the existing 1e-4.  Every other mode: at most MARGIN x
    the simulation of that mode's own roundings on the same clips.

    Measured on an MI355X, waveform rel-L2 of the four clips, GPU / simulation (randn | log-mel):
      fp32       3.24e-5 / 1.8e-6 | 1.86e-5 / 1.2e-6      (bound 1e-4; the simulation has no accumulation-order error)
      mixed_up0  7.17e-4 / 6.27e-4 = 1.14 | 8.06e-4 / 6.99e-4 = 1.15
      mixed_up1  9.01e-4 / 8.23e-4 = 1.09 | 9.73e-4 / 8.85e-4 = 1.10      (one log-mel clip at 1.00e-3)
      headline   1.051e-3 / 9.89e-4 = 1.06 | 1.090e-3 / 1.001e-3 = 1.09   (per clip 1.03e-3 .. 1.13e-3: north_star's 1e-3 is
                 NOT met off the rail - the 6.3-6.7e-4 at default init is the tanh rail's doing; README.md)
      fp16       2.26e-3 / 2.22e-3 = 1.02 | 1.46e-3 / 1.42e-3 = 1.03
      bf16       1.85e-2 / 1.81e-2 = 1.02 | 1.25e-2 / 1.15e-2 = 1.09
    mrf2 and pre-tanh ratios (batch of 2: clips 0 and 7) lie within 0.02 of the waveform's.

    Sensitivity, shown once with two mutated builds of the library: the hl8 lo plane decoded to half its value fails nine cases of
    test_mrf_chain_scale_sweep (three blocks at k = -12, 4, 8) while every full-size waveform test passes; rstd of the streaming
    chain's GroupNorm(8, 64) x 1.0005 fails the headline case here, 19 scale-sweep and all 20 offset-sweep cases."""
    c = c2[kind]
    gen, ref = c["gen"], c["ref"]
    dt = _set_mode(gen, mode)
    dev = lambda t: t.cuda().to(dt)
    try:
        with torch.no_grad():
            wave = gen(dev(c["mel"]), dev(c["spk"]), dev(c["emo"]))
            again = gen(dev(c["mel"]), dev(c["spk"]), dev(c["emo"]))
            st = gen(dev(c["mel"][[0, 7]]), dev(c["spk"][[0, 7]]), dev(c["emo"][[0, 7]]), return_stages=True)
    finally:
        gen.set_mixed_precision(None)
    assert wave.shape == (32, 1, 8192) and wave.dtype == dt and torch.equal(wave, again)
    assert bool(torch.isfinite(wave.float()).all())
    idx = list(CLIPS)
    sim = S.simulate(mode, c["mel"][idx], c["sd"], c["spk"][idx], c["emo"][idx])
    four = [CLIPS.index(i) for i in (0, 7, 13, 31)]
    two = [CLIPS.index(i) for i in (0, 7)]
    atanh = lambda w: torch.atanh(w.double().clamp(-1 + 1e-7, 1 - 1e-7))
    got = {"wave": (wave[[0, 7, 13, 31]].float().cpu(), four), "mrf2": (st["mrf2"].float().cpu(), two),
           "pre-tanh": (atanh(st["wave"].float().cpu()), two)}
    fig = {}
    for name, (y, rows) in got.items():
        key = "output_proj" if name == "pre-tanh" else name
        r = ref[key][rows]
        s = atanh(sim["wave"][rows]) if name == "pre-tanh" else sim[key][rows]
        fig[name] = (O.rel_l2(y, r), O.rel_l2(s, r))
    per_clip = [O.rel_l2(wave[i:i + 1].float().cpu(), ref["wave"][CLIPS.index(i):CLIPS.index(i) + 1]) for i in (0, 7, 13, 31)]
    print(f"[off-rail] {mode:9s} {kind:6s} head rms {HEAD_RMS}: " +
          "  ".join(f"{n} gpu {g:.3e} sim {s:.3e} ratio {g / max(s, 1e-30):.2f}" for n, (g, s) in fig.items()) +
          f"  per clip {[f'{e:.2e}' for e in per_clip]}  north_star 1e-3: {'met' if max(per_clip) < NORTH_STAR else 'MISSED'}")
    for name, (g, s) in fig.items():
        if mode == "fp32":
            assert g < 1e-4, (name, g)
        else:
            assert g <= MODE_MARGIN[mode] * s, (mode, kind, name, g, s)


# ================================================================================================ 2. MRF chain scale sweep
def _uncentred_err(wave, ref_pre, raw):
    """Error of the pre-tanh signal behind a calibrated head (atanh of the unsaturated waveform) relative to the head's UNCENTRED
    output `raw`, the quantity the output conv sums: ||atanh(wave) - ref_pre|| / ||raw||, over the samples whose reference is off the
    rail (|ref_pre| < 2.5: beyond it atanh of an fp32 waveform amplifies the waveform's own rounding by 1 / (1 - w^2) > 40; the
    calibration fixes the rms, not the outliers - measured 1.1e-3 on GPU and simulation alike with them in, at k = -12, T = 4100)."""
    pre = torch.atanh(wave.double().clamp(-1 + 1e-7, 1 - 1e-7))
    keep = ref_pre.abs() < 2.5
    assert float(keep.double().mean()) > 0.95
    return float((pre - ref_pre)[keep].norm() / raw[keep].norm())


def _pair_rows(x_cl):
    B, T, C = x_cl.shape
    g = x_cl.view(B, T, C // 8, 8)
    hi = g.to(torch.float16)
    lo = (g - hi.float()).to(torch.float16)
    return torch.stack([hi, lo], dim=3).contiguous().view(torch.float32).view(B, T, C)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("B,T", [(2, 48), (3, 700), (2, 4100)])
@pytest.mark.parametrize("k", [-12, -8, -4, 0, 4, 8])
def test_mrf_chain_scale_sweep(H, k, B, T, n):
    """The chain on a stream scaled by 2^k (the absolute scale of the stream that enters the chain is a free parameter of a trained
    model), against the fp64 oracle on the same input.  Three-product mode (bf16 pieces: fp32's exponent range): the unit-scale bound
    2e-5 at every k.  Two-product modes (f16 hi + lo operands, hl8 or pair rows between the blocks): at most MARGIN x the simulation
    of the mode at that k, finite, and for three blocks inside the existing 4e-4 over the whole window (the documented one).  Chain +
    output conv with a head calibrated to rms 0.3: two-product the same on the waveform; three-product the fp32 waveform bound 1e-4 on
    the pre-tanh signal (atanh of the waveform) relative to the UNCENTRED output of the head, which is what the conv sums - the
    calibration removes a mean that is up to 17 x the centred signal at 2^-12, where the blocks' output is nearly constant per channel.

    Measured on an MI355X (GPU = simulation to three digits in the two-product modes at almost every point):
      three-product, 3 blocks: 1.9e-5 (k = -12), 5.5e-6 (k = 0), 6.0e-8 (k = 8); + output conv at most 3e-5 of the uncentred signal
      w16 / w16_pair, 3 blocks: 3.1e-4, 2.9e-4, 3.0e-4, 2.4e-4, 3.0e-5, 1.1e-5 / 1.8e-6 for k = -12 .. 8: inside the existing 4e-4
      over the whole window 2^-12 .. 2^8; + output conv on the calibrated waveform: 1.1e-3, 5.4e-4, 7.4e-4, 4.0e-4, 3.1e-5, 1.2e-5
      (one block at k = -12: 6.5e-3 .. 8.7e-3, GPU = simulation: the single-f16 weights on a stream whose signal sits 2^-12 under the
      biases, amplified by the calibration)."""
    from hifigan_modified.fused import MrfChain, mrf_fused_for
    from hifigan_modified import _native as N
    blks, sds = _blocks(H)
    chain = MrfChain([mrf_fused_for(bk.cuda().train(False)) for bk in blks[:n]])
    torch.manual_seed(T)
    x = torch.randn(B, 64, T) * 2.0 ** k
    xc = x.cuda().transpose(1, 2).contiguous()
    with torch.no_grad():
        ref = x.double()                                   # every sample: the last one has another workgroup tail
        for sd in sds[:n]:
            ref = O.mrf_block(ref, _f64(sd), "")
        head = _head(H)
        head = S.calibrate_head(head, F.conv1d(ref, head["output_proj.weight"].double(), padding=5), HEAD_RMS)
        wh, bh = head["output_proj.weight"], head["output_proj.bias"]
        ref_pre = F.conv1d(ref, wh.double(), bh.double(), padding=5)
        ref_wave = torch.tanh(ref_pre)
        raw = F.conv1d(ref, wh.double(), padding=5)        # the head's output before the calibration's bias removes its mean
        sims = {m: S.chain_sim(x, sds, n, m) for m in ("three", "w16", "w16_pair")}
        wt, bias = _pack_head(head)
        ys = {"three": chain.forward_cl(xc, n), "w16": chain.forward_cl(xc, n, w16=True),
              "w16_pair": chain.forward_cl(_pair_rows(xc), n, w16=True, x_pair=True)}
        waves = {"three": chain.forward_out_cl(xc, wt, bias, 11, N.ACT_TANH), "w16": chain.forward_out_cl(xc, wt, bias, 11, N.ACT_TANH, w16=True)}
    fails = []
    for m, y in ys.items():
        y = y.transpose(1, 2).cpu()
        assert bool(torch.isfinite(y).all()), (m, k)
        g, s = O.rel_l2(y, ref), O.rel_l2(sims[m], ref)
        bound = 2e-5 if m == "three" else MARGIN * s
        if m != "three" and n == 3:
            bound = min(bound, 4e-4)                       # the validated stream-scale window of set_mixed_precision's docstring
        print(f"[scale] k={k:+d} B={B} T={T} n={n} {m:8s} gpu {g:.3e} sim {s:.3e} bound {bound:.3e}")
        if not g <= bound:
            fails.append((m, g, bound))
    for m, w in waves.items():
        w = w.cpu()
        assert bool(torch.isfinite(w).all()), (m, k)
        ops_w = "bf16x3" if m == "three" else "bf16x2"
        sw = torch.tanh(F.conv1d(S.EB.q(sims[m], ops_w), S.EB.q(wh, ops_w), bh, padding=5))
        if m == "three":
            g, s, bound = _uncentred_err(w, ref_pre, raw), _uncentred_err(sw, ref_pre, raw), 1e-4
        else:
            g, s = O.rel_l2(w, ref_wave), O.rel_l2(sw, ref_wave)
            bound = MARGIN * s
        print(f"[scale] k={k:+d} B={B} T={T} n={n} {m:8s} + output conv: gpu {g:.3e} sim {s:.3e} bound {bound:.3e}")
        if not g <= bound:
            fails.append((m + "+out", g, bound))
    assert not fails, fails


# ================================================================================================ 3. GroupNorm offset sweep
GN_BOUND = {"fused_fp32": 2e-5, "fused_fp16": 1.5e-3, "fused_bf16": 8e-3,     # test_mrf_fused_vs_generic_and_golden
            "chain_tile": 5e-5,                                                # fp32 stage bound of test_generator_fused_pipeline_every_stage
            "chain_stream": 4e-4,                                              # test_stream_chain_vs_oracle_ragged
            "chain_tile_out": 1e-4,                                            # fp32 waveform bound, on the uncentred pre-tanh signal
            "chain_stream_out": None,                                          # MARGIN x the simulation of the mode on the same blocks
            "generic": 1e-4}                                                   # TOL[fp32] of test_gpu_parity_generic


@pytest.mark.parametrize("T", [700, 8192])
@pytest.mark.parametrize("which", ["branch", "fusion"])
@pytest.mark.parametrize("r", [0, 3, 10, 30, 100])
def test_groupnorm_offset_sweep(H, r, which, T):
    """GroupNorm inputs whose group mean is r x the group std (tests/numerics_sim.py::offset_biases, applied to every block of a
    3-block chain: to the three 20-channel branch norms, or to the 64-channel norm behind the fusion conv), on every fused path, the
    generic two-pass kernel as a control.  Reference: fp64 oracle.  Floor: the same oracle in fp32 on the CPU (two-pass) against
    fp64.  Bound per path: max(the path's unit-scale bound, 4 x floor).

    The fused kernels form their statistics in a single fp32 pass (csrc/mrf_stream.hip, mrf_fused.hip, conv_out.hip).  As plain
    var = E[x^2] - mu^2 that cancels as r grows (a CPU emulation: error of rstd 1.3e-5 at r = 30, 4.5e-4 at r = 100), and measured
    on an MI355X it did: inside the bounds through r = 10, at r = 30 the fused fp32 block at 2.5e-5 .. 8.0e-5 (bound 2e-5) and the
    tile chain up to 1.2e-4 (bound 5e-5), at r = 100 every fp32-storage path at 3.5e-4 .. 1.6e-3, the generic two-pass control at 4e-6.
    The sums are therefore taken about a pivot, the mean of the group's biases: mv_mrf_pack stores the bias tables minus that mean
    (csrc/mrf_fused.hip, mrf_pack_kernel), so the accumulators hold v - p and f - p and the kernels are as they were.  Measured
    with the pivot, T = 700 | 8192, worst of branch / fusion:
      r = 30:  fused fp32 5.2e-6 | 5.2e-6, tile chain 7.0e-6 | 7.0e-6, streaming chain 2.4e-4, + output conv 1.1e-5 / 4.0e-4
      r = 100: fused fp32 1.0e-5 | 1.0e-5, tile chain 1.4e-5 | 1.4e-5, streaming chain 2.4e-4, + output conv 2.1e-5 / 4.0e-4
               (floor 4e-6 .. 2.6e-5; generic 3.5e-6 .. 4.1e-6; fused fp16 3.4e-4, bf16 2.8e-3 as at r = 0)"""
    from hifigan_modified import functional as Fn, _native as N
    from hifigan_modified.fused import MrfChain, mrf_fused_for
    blks, sds = _blocks(H)
    torch.manual_seed(T + r)
    x = torch.randn(2, 64, T)
    with torch.no_grad():
        cur, refs, floors, sds_r = x.double(), [], [], []
        cur32 = x
        for bk, sd in zip(blks, sds):
            sd_r, ratio = S.offset_biases(sd, "", float(r), cur.float(), which)
            bk.load_state_dict(sd_r)
            sds_r.append(sd_r)
            cur = O.mrf_block(cur, _f64(sd_r), "")
            cur32 = O.mrf_block(cur32, sd_r, "")
            refs.append(cur)
            floors.append(O.rel_l2(cur32, cur))
        head = _head(H)
        head = S.calibrate_head(head, F.conv1d(refs[2], head["output_proj.weight"].double(), padding=5), HEAD_RMS)
        wh, bh = head["output_proj.weight"], head["output_proj.bias"]
        ref_wave = torch.tanh(F.conv1d(refs[2], wh.double(), bh.double(), padding=5))
        floor_wave = O.rel_l2(torch.tanh(F.conv1d(cur32, wh, bh, padding=5)), ref_wave)
        raw = F.conv1d(refs[2], wh.double(), padding=5)
        ref_pre = F.conv1d(refs[2], wh.double(), bh.double(), padding=5)
        sim_wave = torch.tanh(F.conv1d(S.EB.q(S.chain_sim(x, sds_r, 3, "w16"), "bf16x2"), S.EB.q(wh, "bf16x2"), bh, padding=5))
        unit = dict(GN_BOUND, chain_stream_out=MARGIN * O.rel_l2(sim_wave, ref_wave))
        blks = [bk.cuda().train(False) for bk in blks]
        chain = MrfChain([mrf_fused_for(bk) for bk in blks])
        xg = x.cuda()
        xc = xg.transpose(1, 2).contiguous()
        wt, bias = _pack_head(head)
        nct = lambda y: y.transpose(1, 2).float().cpu()
        got = {
            "fused_fp32": (Fn.mrf_block(xg, blks[0]).cpu(), refs[0], floors[0]),
            "fused_fp16": (Fn.mrf_block(xg.half(), blks[0]).float().cpu(), refs[0], floors[0]),
            "fused_bf16": (Fn.mrf_block(xg.bfloat16(), blks[0]).float().cpu(), refs[0], floors[0]),
            "generic": (Fn.mrf_block(xg, blks[0], force_generic=True).cpu(), refs[0], floors[0]),
            "chain_tile": (nct(chain.forward_cl(xc)), refs[2], floors[2]),
            "chain_stream": (nct(chain.forward_cl(xc, w16=True)), refs[2], floors[2]),
            "chain_tile_out": (chain.forward_out_cl(xc, wt, bias, 11, N.ACT_TANH).cpu(), ref_wave, floor_wave),
            "chain_stream_out": (chain.forward_out_cl(xc, wt, bias, 11, N.ACT_TANH, w16=True).cpu(), ref_wave, floor_wave),
        }
    fails = []
    for path, (y, ref, floor) in got.items():
        e = _uncentred_err(y, ref_pre, raw) if path == "chain_tile_out" else O.rel_l2(y, ref)
        bound = max(unit[path], 4 * floor)
        print(f"[gn-offset] r={r:3d} {which:6s} T={T} {path:16s} err {e:.3e} floor {floor:.3e} bound {bound:.3e}{'' if e <= bound else '  OVER'}")
        if not e <= bound:
            fails.append((path, e, bound))
    assert not fails, fails


# ================================================================================================ 4. sharp ODConv attention
@pytest.mark.parametrize("mode", ["fp32", "fp16", "mixed_up1", "bf16"])
def test_sharp_odconv_attention(H, mode):
    """ODConv attention logits x 20 (alpha near one-hot) on log-mel input: the prologue forms alpha from an fp16 mean of an
    offset-heavy mel (mv_gen_prologue for fp16 inputs, mv_gen_prologue_in for the mixed mode's fp32 inputs), the K-loop kernels apply
    alpha to accumulators - through the fused input_proj (+FiLM) and the first two upsamplers, against the fp64 oracle with the
    per-dtype bounds of test_odconv_fused_vs_generic."""
    gen, sd = S.default_generator_sd(0)
    sd = S.sharpen_attention(sd)
    gen.load_state_dict(sd)
    mel = S.logmel_like(4, 32)
    torch.manual_seed(1)
    spk, emo = torch.randn(4, 192), torch.randn(4, 384)
    with torch.no_grad():
        ref = O.generator_forward(mel.double(), _f64(sd), "", spk.double(), emo.double(), return_stages=True)
        a0 = O.odconv_attention(mel.double(), sd["input_proj.kernel_attention.1.weight"].double(), sd["input_proj.kernel_attention.1.bias"].double())
    assert float((a0.max(1).values > 0.99).double().mean()) >= 0.75, a0
    gen = gen.cuda().train(False)
    dt = _set_mode(gen, mode)
    with torch.no_grad():
        st = gen(mel.cuda().to(dt), spk.cuda().to(dt), emo.cuda().to(dt), return_stages=True)
    bound = {"fp32": 2e-5, "fp16": 1.5e-3, "mixed_up1": 1.5e-3, "bf16": 8e-3}[mode]
    errs = {k: O.rel_l2(st[k].float().cpu(), ref[k]) for k in ("film", "up0", "up1")}
    print(f"[sharp-alpha] {mode}: max alpha {[f'{v:.4f}' for v in a0.max(1).values.tolist()]} " + " ".join(f"{k} {e:.3e}" for k, e in errs.items()))
    assert max(errs.values()) < bound, (mode, errs)
