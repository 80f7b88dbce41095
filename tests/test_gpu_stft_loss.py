"""Multi-resolution STFT loss (mv_stft_loss, csrc/stft_loss.hip): value, per-resolution sums and gradient against an fp64 restatement
built from F.pad(reflect) + torch.stft(center=False, periodic Hann) + autograd on the CPU; the clamp's zero gradient; the exact zero
of fake == real; 16-bit waves; operator against direct dispatch; the term inside VocoderTrainer (eager, captured, checkpoint, evaluate).

Tolerances are the mel-loss tests' own: loss (and each sc_r / mag_r recomputed from the sums) relative 1e-4, gradient rel-L2 2e-3.  A
plain fp32 torch restatement of these inputs sits at <= 6e-8 (loss) and <= 2e-5 (gradient) against fp64, so the bounds leave the
reference three orders of room and still catch a wrong bin, a wrong conjugate or a missing window factor."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FLOOR = 1e-7
SMALL = ((64, 16), (128, 32), (32, 8))
CASES = [(SMALL, 2, 256), (((512, 128), (1024, 256), (2048, 512)), 2, 2048), (((2048, 512),), 1, 1024)]


@pytest.fixture(scope="module")
def H():
    import hifigan_modified as H
    from hifigan_modified import _native
    _native.lib()
    return H


def _waves(B, T, seed=0):
    """real, fake: (randn * 0.3).clamp(-1, 1) each, fake silent over [T/4, T/4 + 3T/8) of sample 0."""
    g = torch.Generator().manual_seed(seed)
    real = (torch.randn(B, 1, T, generator=g) * 0.3).clamp(-1, 1)
    fake = (torch.randn(B, 1, T, generator=g) * 0.3).clamp(-1, 1)
    fake[0, 0, T // 4: T // 4 + 3 * T // 8] = 0
    return real, fake


def _mag(x, n_fft, hop, floor):
    pad = (n_fft - hop) // 2
    xp = F.pad(x, (pad, pad), mode="reflect").squeeze(1)
    X = torch.stft(xp, n_fft, hop_length=hop, win_length=n_fft, window=torch.hann_window(n_fft, periodic=True, dtype=x.dtype),
                   center=False, return_complex=True)
    assert X.shape[1:] == (n_fft // 2 + 1, x.shape[-1] // hop)
    P = X.real ** 2 + X.imag ** 2
    return torch.sqrt(torch.clamp(P, min=floor))


def reference(fake, real, resolutions, floor=FLOOR, weight=1.0):
    """fp64 on the CPU: (loss, [(sc_r, mag_r)], d loss / d fake)."""
    fake = fake.detach().double().cpu().requires_grad_(True)
    real = real.detach().double().cpu()
    terms, total = [], 0.0
    for n_fft, hop in resolutions:
        Mf, Mr = _mag(fake, n_fft, hop, floor), _mag(real, n_fft, hop, floor)
        sc = torch.sqrt(((Mr - Mf) ** 2).sum()) / torch.sqrt((Mr ** 2).sum())
        mag = (torch.log(Mf) - torch.log(Mr)).abs().mean()
        terms.append((float(sc.detach()), float(mag.detach())))
        total = total + sc + mag
    loss = weight * total / len(resolutions)
    (grad,) = torch.autograd.grad(loss, fake)
    return float(loss.detach()), terms, grad


_REF = {}


def _ref(case, dtype=torch.float32):
    """The reference of one case (computed once per (case, dtype): the 16-bit tests take the rounded waves)."""
    key = (case, dtype)
    if key not in _REF:
        res, B, T = CASES[case]
        real, fake = _waves(B, T)
        real, fake = real.to(dtype), fake.to(dtype)
        _REF[key] = (real, fake) + reference(fake, real, res)
    return _REF[key]


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _terms_from_sums(sums, resolutions, B, T):
    out = []
    for (n_fft, hop), (s_num, s_den, s_log) in zip(resolutions, sums.double().cpu().tolist()):
        n = B * (n_fft // 2 + 1) * (T // hop)
        out.append((math.sqrt(s_num) / math.sqrt(s_den), s_log / n))
    return out


@pytest.mark.parametrize("case", range(len(CASES)))
def test_value_sums_and_gradient_against_fp64(H, case):
    from hifigan_modified import ops
    res, B, T = CASES[case]
    real, fake, loss_ref, terms_ref, grad_ref = _ref(case)
    loss, sums, gwave = ops.stft_loss(fake.cuda(), real.cuda(), res, FLOOR, 1.0, backward=True)
    assert loss.shape == (1,) and sums.shape == (len(res), 3) and gwave.shape == (B, 1, T) and gwave.dtype == torch.float32
    e_loss = _rel(float(loss), loss_ref)
    terms = _terms_from_sums(sums, res, B, T)
    e_terms = [(_rel(sc, sc_r), _rel(mag, mag_r)) for (sc, mag), (sc_r, mag_r) in zip(terms, terms_ref)]
    e_grad = _rel_l2(gwave.cpu(), grad_ref)
    print(f"[stft] {res} B={B} T={T}: loss {float(loss):.6f} rel {e_loss:.2e}; (sc, mag) rel {e_terms}; gradient rel-L2 {e_grad:.2e}")
    assert e_loss < 1e-4
    assert all(e < 1e-4 for pair in e_terms for e in pair), e_terms
    assert e_grad < 2e-3
    # the weight scales value and gradient; without backward no gradient is formed
    loss_w, _, g_none = ops.stft_loss(fake.cuda(), real.cuda(), res, FLOOR, 2.5, backward=False)
    assert g_none is None and _rel(float(loss_w), 2.5 * loss_ref) < 1e-4


def test_clamped_bins_have_zero_gradient(H):
    """(32, 8) at T = 256: every sample of the silent stretch all of whose covering frames lie inside the stretch has P_fake <= floor
    in every bin of every frame that reaches it, so its gradient is exactly 0.0."""
    from hifigan_modified import ops
    n_fft, hop, T = 32, 8, 256
    real, fake = _waves(2, T)
    lo, hi = T // 4, T // 4 + 3 * T // 8
    pad = (n_fft - hop) // 2
    refl = lambda i: -i if i < 0 else (2 * (T - 1) - i if i >= T else i)
    silent = torch.ones(T, dtype=torch.bool)
    for f in range(T // hop):
        idx = [refl(f * hop - pad + n) for n in range(n_fft)]
        if not all(lo <= i < hi for i in idx):
            silent[idx] = False          # a frame that is not entirely zero: the samples it covers may carry gradient
    silent[:lo] = False
    silent[hi:] = False
    assert int(silent.sum()) > 0
    _, _, gwave = ops.stft_loss(fake.cuda(), real.cuda(), ((n_fft, hop),), FLOOR, 1.0, backward=True)
    g = gwave.cpu()
    assert torch.all(g[0, 0, silent] == 0.0)
    assert torch.isfinite(g).all() and float(g[0, 0, ~silent].abs().max()) > 0 and float(g[1].abs().max()) > 0


@pytest.mark.parametrize("res", [SMALL, CASES[1][0]])
def test_identical_waves_give_exact_zero(H, res):
    from hifigan_modified import ops
    T = 256 if res is SMALL else 2048
    real, _ = _waves(2, T)
    real = real.cuda()
    loss, sums, gwave = ops.stft_loss(real.clone(), real, res, FLOOR, 1.0, backward=True)
    assert float(loss) == 0.0
    assert torch.all(gwave == 0.0)
    assert torch.isfinite(sums).all() and torch.all(sums[:, 0] == 0) and torch.all(sums[:, 2] == 0) and torch.all(sums[:, 1] > 0)


@pytest.mark.parametrize("dtype,half_ulp", [(torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11)])
def test_16bit_waves(H, dtype, half_ulp):
    """The rounded wave upcast to fp64 is the reference's input; the gradient comes back in the wave's dtype: the kernel's bound plus
    the half-ulp of that final cast."""
    from hifigan_modified import functional as Fn
    res, B, T = CASES[0]
    real, fake, loss_ref, _, grad_ref = _ref(0, dtype)
    x = fake.cuda().requires_grad_(True)
    loss = Fn.mr_stft_loss(x, real.cuda(), res, FLOOR)
    loss.backward()
    e_loss, e_grad = _rel(float(loss.detach()), loss_ref), _rel_l2(x.grad.cpu(), grad_ref)
    print(f"[stft] {dtype}: loss rel {e_loss:.2e}, gradient rel-L2 {e_grad:.2e}")
    assert x.grad.dtype == dtype and loss.dtype == torch.float32 and loss.dim() == 0
    assert e_loss < 1e-4
    assert e_grad < 2e-3 + half_ulp


def test_operator_equals_direct_call_and_opcheck(H):
    """The torch operator and the direct autograd.Function run the same launches; the sums and the gradient are accumulated with fp32
    atomics, so two runs agree to summation order: the captured-step rule, rel < 2e-5 + 5 * rel(direct, direct)."""
    from torch.library import opcheck
    from hifigan_modified import functional as Fn
    res, B, T = CASES[0]
    real, fake = _waves(B, T)
    real = real.cuda()
    out = {}
    for tag, mode in (("op", "torch_ops"), ("direct", "direct"), ("again", "direct")):
        Fn.DISPATCH = mode
        try:
            x = fake.cuda().requires_grad_(True)
            loss = Fn.mr_stft_loss(x, real, res, FLOOR, 3.0)
            (2.0 * loss).backward()
            out[tag] = (float(loss), x.grad.clone())
        finally:
            Fn.DISPATCH = "torch_ops"
    assert _rel(out["op"][0], out["direct"][0]) < 2e-5 + 5 * _rel(out["again"][0], out["direct"][0])
    assert _rel_l2(out["op"][1], out["direct"][1]) < 2e-5 + 5 * _rel_l2(out["again"][1], out["direct"][1])
    # upstream gradient 2, weight 3: six times the unit-weight gradient
    assert _rel_l2(out["op"][1].cpu(), 6.0 * reference(fake, real, res)[2]) < 2e-3
    ns = torch.ops.mi355x_vocoder
    opcheck(ns.stft_loss, (fake.cuda().requires_grad_(True), real, [n for n, _ in res], [h for _, h in res], FLOOR, 1.0),
            test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))


# ---- the term inside VocoderTrainer (the configuration of test_gpu_train_graph.py)
CFG = dict(hidden_channels=64, upsample_factors=[4, 2])
HOP = 8
KEYS3 = {"generator_loss", "discriminator_loss", "mel_loss"}


def _trainer(H, use_graph, stft=True, seed=0, **kw):
    torch.manual_seed(seed)
    voc = H.ModifiedHiFiGANVocoder(dropout=0.0, **CFG)
    if stft:
        voc.set_stft_loss(SMALL)
    return H.VocoderTrainer(voc, device=torch.device("cuda"), use_graph=use_graph, **kw)


def _batch(i, B=2, T=64):
    g = torch.Generator().manual_seed(100 + i)
    return (torch.randn(B, 80, T, generator=g).cuda(), (torch.randn(B, 1, T * HOP, generator=g) * 0.5).clamp(-1, 1).cuda(),
            torch.randn(B, 192, generator=g).cuda(), torch.randn(B, 384, generator=g).cuda())


def test_trainer_eager_step_adds_the_weighted_term(H):
    t = _trainer(H, False)
    t.vocoder.set_stft_loss(SMALL, weight=0.5)
    mel, real, spk, emo = _batch(0)
    with torch.no_grad():
        wave = t.vocoder(mel, spk, emo)["generated_waveform"]       # the step's own fake audio: the weights before the update
    out = t.train_step(mel, real, spk, emo)
    assert set(out) == KEYS3 | {"stft_loss"}
    g = {k: float(v) for k, v in t.last_losses[0].items()}
    assert set(g) == {"total_loss", "mpd_loss", "msd_loss", "mpd_fm_loss", "msd_fm_loss", "mel_loss", "stft_loss"}
    ref = reference(wave, real, SMALL)[0]
    total = g["mpd_loss"] + g["msd_loss"] + 10.0 * (g["mpd_fm_loss"] + g["msd_fm_loss"]) + 45.0 * g["mel_loss"] + 0.5 * ref
    print(f"[stft] trainer: stft_loss {g['stft_loss']:.6f} vs fp64 {ref:.6f}; total {g['total_loss']:.6f} vs {total:.6f}")
    assert _rel(g["stft_loss"], ref) < 1e-4 and _rel(out["stft_loss"], ref) < 1e-4
    assert _rel(g["total_loss"], total) < 1e-4 and _rel(out["generator_loss"], total) < 1e-4


def test_trainer_captured_step_equals_eager_step(H):
    """test_gpu_train_graph.py's rule with the term on: six steps (two warm-up, the capture, replays) against eager ones."""
    ta, tb, tc = _trainer(H, False), _trainer(H, True), _trainer(H, False)
    for i in range(6):
        la, lb, lc = (t.train_step(*_batch(i)) for t in (ta, tb, tc))
        assert set(la) == set(lb) == KEYS3 | {"stft_loss"}
        for k in la:
            assert _rel(lb[k], la[k]) < 2e-5 + 5 * _rel(lc[k], la[k]), (i, k, la, lb, lc)
    assert sum(st["graph"] is not None for st in tb._graphs.values()) == 1


def test_trainer_switching_the_term_records_a_second_graph(H):
    t = _trainer(H, True, stft=False, graph_warmup=1)
    for i in range(3):
        assert set(t.train_step(*_batch(i))) == KEYS3
    assert sum(st["graph"] is not None for st in t._graphs.values()) == 1
    t.vocoder.set_stft_loss(SMALL)
    for i in range(3):
        out = t.train_step(*_batch(i))
        assert set(out) == KEYS3 | {"stft_loss"} and all(v == v for v in out.values())
    assert sum(st["graph"] is not None for st in t._graphs.values()) == 2


def test_trainer_checkpoint_and_evaluate(H, tmp_path):
    t = _trainer(H, False)
    t.vocoder.set_stft_loss(((64, 16), (32, 8)), weight=0.25)
    mel, real, spk, emo = _batch(1)
    t.train_step(mel, real, spk, emo)
    ev = t.evaluate(mel, real, spk, emo, weights="live")
    assert set(ev) == {"mel_loss", "stft_loss"} and ev["stft_loss"] > 0
    with torch.no_grad():
        modes = [(m, m.training) for m in t.vocoder.modules()]
        wave = t.vocoder.train(False)(mel, spk, emo)["generated_waveform"]
        for m, flag in modes:
            m.training = flag
    assert _rel(ev["stft_loss"], reference(wave, real, ((64, 16), (32, 8)))[0]) < 1e-4
    path = str(tmp_path / "on.pt")
    t.save_checkpoint(path)
    ck = torch.load(path, weights_only=True)
    assert ck["stft_loss"] == {"resolutions": [[64, 16], [32, 8]], "weight": 0.25}
    fresh = _trainer(H, False, stft=False, seed=1)
    fresh.load_checkpoint(path)
    assert fresh.vocoder.stft_resolutions == ((64, 16), (32, 8)) and fresh.vocoder.stft_weight == 0.25
    # a default trainer: no key in its file, exactly the three keys in its results, and loading its file turns the term off
    plain = _trainer(H, False, stft=False)
    assert set(plain.train_step(mel, real, spk, emo)) == KEYS3
    assert set(plain.evaluate(mel, real, spk, emo, weights="live")) == {"mel_loss"}
    path2 = str(tmp_path / "off.pt")
    plain.save_checkpoint(path2)
    assert "stft_loss" not in torch.load(path2, weights_only=True)
    fresh.load_checkpoint(path2)
    assert fresh.vocoder.stft_resolutions is None
