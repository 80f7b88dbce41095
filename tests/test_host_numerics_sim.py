"""Host checks of tests/numerics_sim.py (no GPU): known answers of the format emulations, the calibration conditions that the GPU
tests of tests/test_gpu_inference_off_unit_scale.py rely on, and the simulated headline mix at default init."""
import pytest
import torch

import numerics_sim as S
from oracle import vocoder_oracle as O


def _rt(fn, scale, n=1 << 16):
    x = scale * torch.randn(n, generator=torch.Generator().manual_seed(0))
    return O.rel_l2(fn(x), x)


# rel-L2 of the hl8 round trip of s * randn (65536 values): the 15 bits hold between 2^-4 and 2^8; below, the e4m3 byte underflows
# and the row decays to a plain f16; above 2^9 the clamp at 448 bites
# (the flat part is 4.9e-6 from 2^-3 to 2^6; at its left edge, 2^-4, the smallest values' residuals already underflow: 5.8e-6)
HL8_TABLE = {-16: 1.1e-3, -12: 2.1e-4, -10: 1.8e-4, -8: 6.4e-5, -6: 1.7e-5, -4: 5.8e-6, -3: 4.9e-6, 0: 4.9e-6, 6: 4.9e-6, 8: 6.9e-6,
             10: 1.0e-4, 12: 1.7e-4}


@pytest.mark.parametrize("k", sorted(HL8_TABLE))
def test_hl8_round_trip_table(k):
    e = _rt(S.hl8, 2.0 ** k)
    assert abs(e / HL8_TABLE[k] - 1) < 0.10, (k, e)


def test_hl8_clamp_and_overflow():
    # a residual beyond the byte's range is clamped to 448 / 2048, not turned into NaN by the cast
    hi = torch.tensor([1024.0, -1024.0])
    x = hi + torch.tensor([0.4, -0.4])                  # residual 0.4 * 2048 = 819 > 448 (f16 spacing at 1024 is 1)
    y = S.hl8(x)
    assert torch.equal(y, hi + torch.tensor([448.0 / 2048, -448.0 / 2048]))
    assert bool(torch.isfinite(S.hl8(torch.tensor([500.0 / 2048 + 2.0 ** -30, 65504.0]))).all())
    assert not bool(torch.isfinite(S.hl8(torch.tensor([2.0 ** 17]))).all())      # the hi plane overflows: a known property of f16
    x14 = 2.0 ** 14 * torch.randn(1 << 16, generator=torch.Generator().manual_seed(0))
    assert not bool(torch.isfinite(S.hl8(x14)).all())                            # ... reached by randn at scale 2^14 (4 sigma = 65536)
    # single f16 is the format that "does not fit"
    assert abs(_rt(lambda t: t.half().float(), 1.0) / 2.07e-4 - 1) < 0.10


def test_pair_and_split_bf16_round_trips():
    assert _rt(S.pair, 1.0) < 2.0 ** -21                 # 22 significant bits
    assert _rt(S.pair, 2.0 ** -12) > 2.0 ** -17          # the lo half goes subnormal: the window is about the stream's scale
    for k in (-12, 0, 8):                                # bf16 pieces have fp32's exponent range
        assert _rt(lambda t: S.bf16xN(t, 3), 2.0 ** k) < 2.0 ** -23
        assert 2.0 ** -20 < _rt(lambda t: S.bf16xN(t, 2), 2.0 ** k) < 2.0 ** -16   # 16 bits, at every scale


@pytest.fixture(scope="module")
def clips():
    gen, sd = S.default_generator_sd(0)
    torch.manual_seed(1)
    mel, spk, emo = torch.randn(2, 80, 32), torch.randn(2, 192), torch.randn(2, 384)
    with torch.no_grad():
        ref = O.generator_forward(mel, sd, "", spk, emo, return_stages=True)
    return sd, mel, spk, emo, ref


def test_default_head_is_saturated_and_headline_sim_matches(clips):
    sd, mel, spk, emo, ref = clips
    assert float((ref["wave"].abs() > 0.99).float().mean()) > 0.9          # the operating point the published figures sit on
    sim = S.simulate("headline", mel, sd, spk, emo)
    e = O.rel_l2(sim["wave"], ref["wave"])
    assert abs(e / 6.65e-4 - 1) < 0.10, e                                  # measured on the GPU: 6.3-6.7e-4
    assert O.rel_l2(S.simulate("fp32", mel, sd, spk, emo)["wave"], ref["wave"]) < 1e-4


@pytest.mark.parametrize("rms,share", [(1.0, 0.05), (0.3, 0.05)])
def test_calibrated_head_is_off_the_rail(clips, rms, share):
    sd, mel, spk, emo, ref = clips
    cal = S.calibrate_head(sd, ref["output_proj"], rms)
    with torch.no_grad():
        st = O.generator_forward(mel, cal, "", spk, emo, return_stages=True)
    y = st["output_proj"]
    assert abs(float(y.mean())) < 1e-3 * rms and abs(float(y.pow(2).mean().sqrt()) / rms - 1) < 1e-3
    assert float((st["wave"].abs() > 0.99).float().mean()) <= share
    if rms == 0.3:
        # off the rail the waveform error is the pre-tanh error: the headline mix's real distance to the oracle
        sim = S.simulate("headline", mel, cal, spk, emo)
        ew, ep = O.rel_l2(sim["wave"], st["wave"]), O.rel_l2(sim["output_proj"], y)
        assert abs(ew / ep - 1) < 0.05 and 7e-4 < ew < 1.2e-3, (ew, ep)


def test_logmel_like_statistics():
    mel = S.logmel_like(2, 32)
    assert mel.shape == (2, 80, 32) and bool(torch.isfinite(mel).all())
    assert torch.equal(mel, S.logmel_like(2, 32))
    assert -8.0 < float(mel.mean()) < -2.0 and float(mel.std()) > 1.0


@pytest.mark.parametrize("which", ["branch", "fusion"])
@pytest.mark.parametrize("r", [0, 3, 100])
def test_offset_biases_reach_the_ratio_and_keep_the_output(which, r):
    import hifigan_modified as H
    torch.manual_seed(0)
    sd = {k: v.detach().clone() for k, v in H.MultiReceptiveFieldBlock(64, 64).state_dict().items()}
    torch.manual_seed(2)
    x = torch.randn(2, 64, 300)
    sd_r, ratio = S.offset_biases(sd, "", float(r), x, which)
    assert float((ratio - r).abs().max()) <= 0.2 * max(r, 1)
    sd64, sdr64 = ({k: v.double() for k, v in d.items()} for d in (sd, sd_r))
    with torch.no_grad():
        # (the shifted bias is an fp32 number: its rounding, 2^-24 x r stds per channel, is all that moves the output)
        assert O.rel_l2(O.mrf_block(x.double(), sdr64, ""), O.mrf_block(x.double(), sd64, "")) < 6e-8 * max(r, 1)


def test_sharpened_attention_is_near_one_hot(clips):
    sd = S.sharpen_attention(clips[0])
    mel = S.logmel_like(4, 32)
    a = O.odconv_attention(mel, sd["input_proj.kernel_attention.1.weight"], sd["input_proj.kernel_attention.1.bias"])
    assert float((a.max(1).values > 0.99).float().mean()) >= 0.75, a
