"""The generator's weight EMA on the arena (optim.ArenaEMA, VocoderTrainer(ema_decay=...)): the two streaming kernels against fp64
and bit-exact properties, the average a trainer keeps of ITS OWN trajectory (eager, captured, with accumulation), the exchange
behind `ema_weights()`, `evaluate`, the checkpoint round trip and the untouched default trainer.

Training is not bit-reproducible between two trainers (loss and weight-gradient sums use fp32 atomics), so every trajectory check
recomputes the average in fp64 from snapshots of the same trainer's arena.

The bound.  One update is ema' = fmaf(w, p - ema, ema): the subtraction and the fused multiply-add each round once, so with
M = max(|p|, |ema|, |ema'|) one update is off by at most 2^-24 * (w * |p - ema| + |ema'|) <= 2^-24 * (2 w + 1) M < 2^-22 * M / 1.3,
and the errors of earlier updates shrink by the decay at every later one.  N updates are therefore within N * 2^-22 * M per element
(M over the whole trajectory), with a margin of at least 1.3x and usually far more: the bounds below are 5 * 2^-22 for the five
updates of the kernel test and 6, 8, 2 and 3 * 2^-22 for trajectories of that many updates."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CFG = dict(hidden_channels=64, upsample_factors=[4, 2])
HOP = 8
U = 2.0 ** -22
SIZES = (1, 7, 8, 1023, 4096 + 5)
OFFSETS = (0, 3)          # element offset inside a larger allocation: 3 gives a misaligned head
PAD = 5                   # elements kept behind the range (and `offset` in front of it): must stay untouched


@pytest.fixture(scope="module")
def H():
    import hifigan_modified as H
    from hifigan_modified import _native
    _native.lib()
    return H


@pytest.fixture(scope="module")
def OPS(H):
    from hifigan_modified.torch_ops import OPS
    return OPS


def _trainer(H, use_graph, dropout=0.0, seed=0, **kw):
    torch.manual_seed(seed)
    voc = H.ModifiedHiFiGANVocoder(dropout=dropout, **CFG)
    return H.VocoderTrainer(voc, device=torch.device("cuda"), use_graph=use_graph, **kw)


def _batch(i, B=2, T=64, dtype=torch.float32):
    g = torch.Generator().manual_seed(100 + i)
    return (torch.randn(B, 80, T, generator=g).cuda().to(dtype), (torch.randn(B, 1, T * HOP, generator=g) * 0.5).clamp(-1, 1).cuda().to(dtype),
            torch.randn(B, 192, generator=g).cuda().to(dtype), torch.randn(B, 384, generator=g).cuda().to(dtype))


def _scaled_randn(n, g):
    scale = torch.tensor([1e-3, 1.0, 1e3])[torch.randint(0, 3, (n,), generator=g)]
    return torch.randn(n, generator=g) * scale


def _carve(values, off):
    """`values` at element offset `off` of a larger GPU allocation filled with a sentinel; returns (whole buffer, view)."""
    big = torch.full((off + values.numel() + PAD,), 7.25, dtype=torch.float32).cuda()
    view = big[off:off + values.numel()]
    view.copy_(values)
    return big, view


def _outside_untouched(big, off, n):
    return bool((big[:off] == 7.25).all()) and bool((big[off + n:] == 7.25).all())


def _warm_decay(decay, n):
    return min(decay, (1 + n) / (10 + n))


def _w(decay):
    return float(np.float32(1.0 - decay))


class _Ref:
    """fp64 recomputation of an EMA over a trainer's own arena snapshots, with the per-element magnitude the bound scales with."""

    def __init__(self, start):
        self.ema = start.double().cpu().clone()
        self.mag = self.ema.abs()
        self.n = 0

    def update(self, p, w):
        p = p.double().cpu()
        self.ema = self.ema + w * (p - self.ema)
        self.mag = torch.maximum(self.mag, torch.maximum(p.abs(), self.ema.abs()))
        self.n += 1

    def check(self, shadow, tag=""):
        err = (shadow.double().cpu() - self.ema).abs()
        bound = self.n * U * self.mag
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"[ema] {tag}: {self.n} updates, worst error / bound {worst:.3f}, max error {float(err.max()):.3e}")
        assert bool((err <= bound).all()), (tag, worst)


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("n", SIZES)
def test_ema_kernel_against_fp64(OPS, n, off):
    g = torch.Generator().manual_seed(1000 * n + off)
    for w in (0.9, 0.1, 1e-3):
        w32 = float(np.float32(w))
        p_host, e_host = _scaled_randn(n, g), _scaled_randn(n, g)
        p_big, p = _carve(p_host, off)
        results = []
        for path in ("value", "device"):
            e_big, e = _carve(e_host, off)
            w_dev = torch.tensor([w32], dtype=torch.float32).cuda()
            for _ in range(5):
                if path == "value":
                    OPS.ema_update_(e, p, None, w32)
                else:
                    OPS.ema_update_(e, p, w_dev, 123.0)             # the float argument is ignored when the tensor is given
            assert _outside_untouched(e_big, off, n) and _outside_untouched(p_big, off, n), (n, off, w, path)
            assert torch.equal(p.cpu(), p_host)
            results.append(e.cpu())
        assert torch.equal(results[0], results[1]), (n, off, w)     # by value and through device memory: the same bits
        ref, mag = e_host.double().numpy(), np.maximum(np.abs(p_host.double().numpy()), np.abs(e_host.double().numpy()))
        for _ in range(5):
            ref = ref + w32 * (p_host.double().numpy() - ref)
            mag = np.maximum(mag, np.abs(ref))
        err = np.abs(results[0].double().numpy() - ref)
        print(f"[ema] kernel n={n} off={off} w={w}: worst error / bound {float((err / (5 * U * mag)).max()):.3f}")
        assert (err <= 5 * U * mag).all(), (n, off, w, float((err / (5 * U * mag)).max()))


def test_ema_kernel_mixed_alignment_and_empty(OPS):
    """ema and p at different offsets modulo 16 bytes (the scalar route), and n = 0 (nothing launched, nothing touched)."""
    g = torch.Generator().manual_seed(5)
    n = 1023
    p_host, e_host = _scaled_randn(n, g), _scaled_randn(n, g)
    p_big, p = _carve(p_host, 1)
    e_big, e = _carve(e_host, 2)
    a_big, a = _carve(e_host, 0)
    pa_big, pa = _carve(p_host, 0)
    OPS.ema_update_(e, p, None, 0.25)
    OPS.ema_update_(a, pa, None, 0.25)
    assert torch.equal(e, a) and _outside_untouched(e_big, 2, n) and _outside_untouched(p_big, 1, n)
    OPS.ema_update_(e[:0], p[:0], None, 0.25)
    OPS.swap_(e[:0], p[:0])
    assert torch.equal(e, a) and torch.equal(p.cpu(), p_host)


# ---------------------------------------------------------------------------------------------------------------- 2. the swap
@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("n", SIZES)
def test_swap_kernel(OPS, n, off):
    g = torch.Generator().manual_seed(2000 * n + off)
    a_host, b_host = _scaled_randn(n, g), _scaled_randn(n, g)
    a_host[0] = float("nan")                  # bits, not values: a NaN travels too
    a_big, a = _carve(a_host, off)
    b_big, b = _carve(b_host, off)
    bits = lambda t: t.cpu().view(torch.int32)
    OPS.swap_(a, b)
    assert torch.equal(bits(a), bits(b_host)) and torch.equal(bits(b), bits(a_host))
    assert _outside_untouched(a_big, off, n) and _outside_untouched(b_big, off, n)
    OPS.swap_(a, b)
    assert torch.equal(bits(a), bits(a_host)) and torch.equal(bits(b), bits(b_host))
    assert _outside_untouched(a_big, off, n) and _outside_untouched(b_big, off, n)


def test_swap_refuses_overlapping_ranges(OPS):
    big = torch.arange(32, dtype=torch.float32).cuda()
    before = big.clone()
    for a, b in ((big[0:8], big[4:12]), (big[4:12], big[0:8]), (big[3:11], big[3:11]), (big[0:16], big[15:31])):
        with pytest.raises(RuntimeError, match="MV_ERR_ARG"):
            OPS.swap_(a, b)
    torch.cuda.synchronize()
    assert torch.equal(big, before)
    OPS.swap_(big[0:16], big[16:32])          # adjacent ranges do not overlap
    assert torch.equal(big[:16], before[16:]) and torch.equal(big[16:], before[:16])


# ---------------------------------------------------------------------------------------------------------------- 3-5. trajectories
def _run_and_check(tr, calls, decay, tag):
    """`calls` train_step calls on changing batches; after each, when the call stepped, the fp64 average moves with the trainer's own
    arena snapshot and the documented warm-up decay.  Returns the reference."""
    gopt = tr.generator_optimizer
    ref = _Ref(gopt.flat_p)
    assert torch.equal(tr.ema.shadow, gopt.flat_p) and tr.ema.num_updates == 0
    for i in range(calls):
        steps_before, shadow_before = gopt.step_count, tr.ema.shadow.clone()
        tr.train_step(*_batch(i))
        if gopt.step_count == steps_before:                       # an accumulating micro-step: no update, the same bits
            assert torch.equal(tr.ema.shadow, shadow_before), (tag, i)
        else:
            ref.update(gopt.flat_p, _w(_warm_decay(decay, ref.n)))
        assert tr.ema.num_updates == ref.n == gopt.step_count, (tag, i)
    ref.check(tr.ema.shadow, tag)
    return ref


def test_eager_trainer_keeps_the_average_of_its_own_trajectory(H):
    tr = _trainer(H, False, dropout=0.1, ema_decay=0.9)
    _run_and_check(tr, 6, 0.9, "eager")
    assert tr.ema.num_updates == 6
    assert not torch.equal(tr.ema.shadow, tr.generator_optimizer.flat_p)


def test_captured_trainer_keeps_the_average_of_its_own_trajectory(H):
    """Two warm-up steps, the capture with its replay, five further replays: with warm-up the decay changes at every step (0.1, 2/11,
    ... 8/17), so a value baked into the graph at the capture would miss the bound by orders of magnitude."""
    tr = _trainer(H, True, graph_warmup=2, ema_decay=0.9)
    _run_and_check(tr, 8, 0.9, "captured")
    assert tr.ema.num_updates == 8
    assert any(st["graph"] is not None for st in tr._graphs.values())


@pytest.mark.parametrize("use_graph", [False, True])
def test_accumulation_updates_once_per_window(H, use_graph):
    kw = dict(graph_warmup=1) if use_graph else {}
    tr = _trainer(H, use_graph, accumulation_steps=2, ema_decay=0.9, **kw)
    _run_and_check(tr, 4, 0.9, f"accumulation, use_graph={use_graph}")
    assert tr.ema.num_updates == 2 and tr.generator_optimizer.step_count == 2
    if use_graph:       # both phases were captured; only "accumulate + step" holds the update
        assert sum(st["graph"] is not None for st in tr._graphs.values()) == 2
        states = {k[-1]: st for k, st in tr._graphs.items()}
        assert states["step"]["gstate"]["ema"] is True and states["accumulate"]["gstate"]["ema"] is False


# ---------------------------------------------------------------------------------------------------------------- 6. ema_weights()
def test_ema_weights_block(H, tmp_path):
    tr = _trainer(H, False, ema_decay=0.9)
    for i in range(3):
        tr.train_step(*_batch(i))
    gopt, gen = tr.generator_optimizer, tr.vocoder.generator.train(False)
    mel, _, spk, emo = _batch(9)
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    ck = torch.load(path, map_location="cuda", weights_only=True)
    torch.manual_seed(77)
    fresh = H.ModifiedHiFiGANVocoder(dropout=0.0, **CFG).generator
    fresh.load_state_dict(ck["ema_generator_state_dict"], strict=True)
    fresh = fresh.cuda().train(False)
    arena, shadow = gopt.flat_p.clone(), tr.ema.shadow.clone()
    with torch.no_grad():
        want = fresh(mel, spk, emo)
        live = gen(mel, spk, emo)
        with tr.ema_weights():
            assert torch.equal(gopt.flat_p, shadow) and torch.equal(tr.ema.shadow, arena)
            inside = gen(mel, spk, emo)
            with pytest.raises(RuntimeError, match="ema_weights"):
                tr.train_step(*_batch(3))
            with pytest.raises(RuntimeError, match="ema_weights"):
                tr.save_checkpoint(path)
        assert torch.equal(inside, want)
        assert not torch.equal(inside, live)
        assert torch.equal(gopt.flat_p, arena) and torch.equal(tr.ema.shadow, shadow)
        assert torch.equal(gen(mel, spk, emo), live)
        # the same when the body raises
        with pytest.raises(KeyError):
            with tr.ema_weights():
                assert torch.equal(gen(mel, spk, emo), want)
                raise KeyError("body")
        assert torch.equal(gopt.flat_p, arena) and torch.equal(tr.ema.shadow, shadow)
        assert torch.equal(gen(mel, spk, emo), live)
    gen.train(True)
    tr.train_step(*_batch(3))                   # and the trainer goes on
    assert tr.ema.num_updates == 4


def test_ema_weights_with_16bit_activations(H):
    """bf16 activations read the arena through its 16-bit image: the image follows the exchange in and out."""
    tr = _trainer(H, False, ema_decay=0.9)
    for i in range(2):
        tr.train_step(*_batch(i, dtype=torch.bfloat16))
    gen = tr.vocoder.generator.train(False)
    mel, _, spk, emo = _batch(9, dtype=torch.bfloat16)
    with torch.no_grad():
        live = gen(mel, spk, emo)
        with tr.ema_weights():
            inside = gen(mel, spk, emo)
        assert not torch.equal(inside, live)
        assert torch.equal(gen(mel, spk, emo), live)


# ---------------------------------------------------------------------------------------------------------------- 7. evaluate
def test_evaluate(H):
    """The mel loss adds its per-frame partial sums with fp32 atomics (128 workgroups here, all terms non-negative), so two runs of the
    same forward agree within 128 * 2^-24 relative, not bit for bit: that is the tolerance against the hand computation."""
    from hifigan_modified import functional as Fn
    tr = _trainer(H, False, dropout=0.1, ema_decay=0.9, dropout_rng="counter")
    for i in range(2):
        tr.train_step(*_batch(i))
    voc, gopt, dopt = tr.vocoder, tr.generator_optimizer, tr.discriminator_optimizer
    mel, real, spk, emo = _batch(9)

    def by_hand():
        flags = [(m, m.training) for m in voc.modules()]
        voc.train(False)
        with torch.no_grad():
            wave = voc(mel, spk, emo)["generated_waveform"]
            loss = float(Fn.mel_l1(wave, voc.log_mel(real), voc.mel_fb, voc.n_fft, voc.hop))
        for m, f in flags:
            m.training = f
        return loss

    tol = 128 * 2.0 ** -24
    want_live = by_hand()
    with tr.ema_weights():
        want_ema = by_hand()
    print(f"[ema] evaluate: mel L1 live {want_live:.6f}, averaged {want_ema:.6f}")
    assert abs(want_live - want_ema) > 4 * tol * want_live        # told apart beyond the summation noise of both

    def state():
        return ([m.training for m in voc.modules()], gopt.flat_p.clone(), tr.ema.shadow.clone(), tr.ema.num_updates, list(gopt.steps),
                gopt.step_count, list(dopt.steps), dopt.step_count, dict(tr.dropout_rng.state_dict()), tr.window.position,
                dopt.flat_p.clone())

    def same(a, b):
        return all(torch.equal(x, y) if torch.is_tensor(x) else x == y for x, y in zip(a, b))

    for training in (True, False):
        voc.train(training)
        before = state()
        got_live = tr.evaluate(mel, real, spk, emo, weights="live")
        got_ema = tr.evaluate(mel, real, spk, emo)                  # the default: "ema"
        assert set(got_live) == set(got_ema) == {"mel_loss"} and isinstance(got_ema["mel_loss"], float)
        assert abs(got_live["mel_loss"] - want_live) <= tol * want_live, (got_live, want_live)
        assert abs(got_ema["mel_loss"] - want_ema) <= tol * want_ema, (got_ema, want_ema)
        assert same(before, state())
        assert voc.training is training
    assert torch.is_grad_enabled()


# ---------------------------------------------------------------------------------------------------------------- 8. checkpoints
def test_checkpoint_round_trip(H, tmp_path):
    path = str(tmp_path / "ema.pt")
    ta = _trainer(H, False, ema_decay=0.9)
    for i in range(3):
        ta.train_step(*_batch(i))
    ta.save_checkpoint(path)
    tb = _trainer(H, False, seed=5, ema_decay=0.5, ema_warmup=False)
    assert not torch.equal(tb.ema.shadow, ta.ema.shadow)
    tb.load_checkpoint(path)
    assert torch.equal(tb.ema.shadow, ta.ema.shadow) and torch.equal(tb.generator_optimizer.flat_p, ta.generator_optimizer.flat_p)
    assert tb.ema.num_updates == ta.ema.num_updates == 3
    assert tb.ema.current_decay() == ta.ema.current_decay() == 4 / 13
    # three more steps of the restored trainer: the fp64 average continues from the restored state
    gopt = tb.generator_optimizer
    ref = _Ref(tb.ema.shadow)
    for i in range(3, 6):
        tb.train_step(*_batch(i))
        ref.update(gopt.flat_p, _w(_warm_decay(0.9, i)))
    assert tb.ema.num_updates == 6
    ref.check(tb.ema.shadow, "restored")


def test_checkpoints_with_and_without_the_keys(H, tmp_path):
    plain_path, ema_path = str(tmp_path / "plain.pt"), str(tmp_path / "ema.pt")
    plain = _trainer(H, False)
    plain.train_step(*_batch(0))
    plain.save_checkpoint(plain_path)
    ck = torch.load(plain_path, map_location="cpu", weights_only=True)
    assert "ema_state" not in ck and "ema_generator_state_dict" not in ck
    # a file without the keys, into an EMA trainer that has already averaged: the average starts over from the loaded weights
    te = _trainer(H, False, seed=3, ema_decay=0.9)
    te.train_step(*_batch(1))
    assert te.ema.num_updates == 1
    te.load_checkpoint(plain_path)
    assert te.ema.num_updates == 0 and torch.equal(te.ema.shadow, te.generator_optimizer.flat_p)
    assert torch.equal(te.generator_optimizer.flat_p, plain.generator_optimizer.flat_p)
    # a file with the keys, into a trainer without EMA
    te.train_step(*_batch(2))
    te.save_checkpoint(ema_path)
    ck = torch.load(ema_path, map_location="cpu", weights_only=True)
    assert set(ck["ema_state"]) == {"decay", "warmup", "num_updates", "shadow"}
    assert set(ck["ema_generator_state_dict"]) == set(te.vocoder.generator.state_dict())
    plain.load_checkpoint(ema_path)
    assert plain.ema is None and torch.equal(plain.generator_optimizer.flat_p, te.generator_optimizer.flat_p)
    plain.train_step(*_batch(3))


# ---------------------------------------------------------------------------------------------------------------- 9. the default
def test_default_trainer_is_untouched(H, tmp_path):
    tr = _trainer(H, False)
    assert tr.ema is None and tr.generator_optimizer.ema is None
    tr.train_step(*_batch(0))
    path = str(tmp_path / "default.pt")
    tr.save_checkpoint(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert set(ck) == {"vocoder_state_dict", "generator_optimizer_state_dict", "discriminator_optimizer_state_dict"}
    tg = _trainer(H, True)                      # a captured step's trainer adds its dropout stream, as before
    tg.save_checkpoint(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert set(ck) == {"vocoder_state_dict", "generator_optimizer_state_dict", "discriminator_optimizer_state_dict", "dropout_rng_state"}


# ---------------------------------------------------------------------------------------------------------------- 10. operators
def test_opcheck_ema_operators(OPS):
    from torch.library import opcheck
    tests = ("test_schema", "test_faketensor")
    c = lambda *s: torch.randn(*s, device="cuda")
    opcheck(OPS.ema_update_, (c(67), c(67), None, 0.1), test_utils=tests)
    opcheck(OPS.ema_update_, (c(67), c(67), torch.full((1,), 0.1, device="cuda"), 0.0), test_utils=tests)
    opcheck(OPS.swap_, (c(67), c(67)), test_utils=tests)
    with pytest.raises(RuntimeError, match="contiguous fp32"):
        OPS.swap_(c(8), c(9))
    with pytest.raises(RuntimeError, match="contiguous fp32"):
        OPS.ema_update_(c(8).half(), c(8), None, 0.1)
    with pytest.raises(RuntimeError, match="cuda"):
        OPS.swap_(torch.zeros(8), torch.zeros(8))
