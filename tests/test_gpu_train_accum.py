"""Gradient accumulation and max_grad_norm clipping in VocoderTrainer (complete_vocoder.py), on the small model of
test_gpu_train_graph.py: a window of N train_step calls is one optimizer step on the window's averaged gradient, eager, captured
(two graphs per input signature: "accumulate" and "accumulate + step") and data parallel (only the window's last call reduces)."""
import os
import socket

import pytest
import torch

from oracle import vocoder_oracle as O

pytestmark = pytest.mark.gpu

CFG = dict(hidden_channels=64, upsample_factors=[4, 2])
HOP = 8
LR = 2e-4


@pytest.fixture(scope="module")
def H():
    import hifigan_modified as H
    from hifigan_modified import _native
    _native.lib()
    assert torch.cuda.is_available(), "GPU tests need cuda:0"
    return H


def _trainer(H, use_graph=False, dropout=0.0, seed=0, freeze_d=False, **kw):
    torch.manual_seed(seed)
    voc = H.ModifiedHiFiGANVocoder(dropout=dropout, **CFG).to("cuda")
    g, d = H.VocoderTrainer.default_optimizers(voc)
    if freeze_d:                                # lr 0, no decay: the discriminators' AdamW update leaves every weight bit for bit
        d.lr, d.weight_decay = 0.0, 0.0
    return H.VocoderTrainer(voc, g, d, device=torch.device("cuda"), use_graph=use_graph, **kw)


def _batch(i, B=2, T=64):
    g = torch.Generator().manual_seed(100 + i)
    return (torch.randn(B, 80, T, generator=g).cuda(), (torch.randn(B, 1, T * HOP, generator=g) * 0.5).clamp(-1, 1).cuda(),
            torch.randn(B, 192, generator=g).cuda(), torch.randn(B, 384, generator=g).cuda())


def _rel(a, b):
    return abs(a - b) / max(abs(a), 1e-12)


def _init_state(H, dropout=0.0, seed=0):
    torch.manual_seed(seed)
    return {k: v.clone() for k, v in H.ModifiedHiFiGANVocoder(dropout=dropout, **CFG).state_dict().items()}


def _upd_dist(t1, t2, init):
    num = den = 0.0
    for (k, p1), (_, p2) in zip(t1.vocoder.state_dict().items(), t2.vocoder.state_dict().items()):
        if p1.is_floating_point() and "embedding_extractor" not in k:
            num += float((p1.double() - p2.double()).pow(2).sum())
            den += float((p1.double().cpu() - init[k].double()).pow(2).sum())
    return (num / den) ** 0.5


def _update_check(name, before, after_hip, after_ref, lr, tol):
    """rel-L2 of the parameter update over a group of tensors + max element difference (test_gpu_train_parity.py)."""
    num = den = 0.0
    worst = 0.0
    for k in after_ref:
        d_h = (after_hip[k].double() - before[k].double())
        d_r = (after_ref[k].double() - before[k].double())
        num += float((d_h - d_r).pow(2).sum())
        den += float(d_r.pow(2).sum())
        worst = max(worst, float((d_h - d_r).abs().max()))
    rel = (num / max(den, 1e-300)) ** 0.5
    assert den > 0, f"{name}: reference update is zero"
    assert rel < tol, f"{name}: update rel-L2 {rel:.3e} (max element diff {worst:.3e})"
    assert worst <= 2.05 * lr, f"{name}: an element moved by more than a sign flip: {worst:.3e}"
    return rel


def _oracle_arena_grads(tr, sd0, batch):
    """Oracle forward + torch autograd on the full batch (the recipe of test_gpu_train_parity.py, discriminators NOT updated between
    the two passes), laid out like each optimizer's arena: (generator fp64 vector, discriminator fp64 vector)."""
    mel, real, spk, emo = (t.cpu() for t in batch)
    P = {k: v.detach().cpu().clone().float().requires_grad_(True) for k, v in sd0.items()
         if k.startswith(("generator.", "discriminators.")) and v.is_floating_point()}
    fake = O.generator_forward(mel, P, "generator.", spk, emo, hidden_channels=64, upsample_factors=(4, 2))
    dl = O.lsgan_discriminator_losses(O.discriminators_forward(real, fake.detach(), P, "discriminators."))
    dl["total_loss"].backward()
    gd = {k: P[k].grad.clone() for k in P if k.startswith("discriminators.") and P[k].grad is not None}
    outs = O.discriminators_forward(real, fake, P, "discriminators.")
    gl = O.lsgan_generator_losses(outs, O.mel_spectrogram(real, hop=HOP).detach(), O.mel_spectrogram(fake, hop=HOP))
    for k in P:
        P[k].grad = None
    gl["total_loss"].backward()
    gg = {k: P[k].grad for k in P if k.startswith("generator.") and P[k].grad is not None}
    names = {id(p): k for k, p in tr.vocoder.named_parameters()}

    def arena(opt, grads):
        out = torch.zeros(opt.numel, dtype=torch.float64)
        for p, o in zip(opt.params, opt.offsets):
            g = grads.get(names[id(p)])
            if g is not None:
                out[o:o + p.numel()] = g.double().reshape(-1)
        return out
    return arena(tr.generator_optimizer, gg), arena(tr.discriminator_optimizer, gd)


def test_accumulated_window_is_the_full_batch_step(H):
    """One step on B = 4 against a two-micro-step window on the same four clips split 2 + 2 (dropout 0, "exact" discriminators):
    the averaged arena gradient (flat_g x 1/N) of each optimizer against the full-batch arena gradient, both measured against the
    oracle gradient (oracle forward + torch autograd on the full batch).  The weight-gradient kernels sum with fp32 atomics, so the
    two differ by summation order only: e_acc <= 1.5 e_full + 1e-6, and e_full under the update bounds of
    test_vocoder_trainer_one_step_matches_oracle_step (0.05 D, 0.08 G).  Inside a window the generator pass sees the discriminators
    of the window's start, in the single step it sees them just updated: the discriminators' optimizer runs at lr 0 / weight decay 0
    in both trainers (its update then leaves every weight bit for bit), so that both generator gradients are taken through the same
    discriminators, the ones the oracle uses.  Measured on an MI355X: generator e_full 2.00e-05, e_acc 2.00e-05;
    discriminators e_full 5.55e-07, e_acc 5.58e-07."""
    from hifigan_modified.optim import WarmupCosineLR
    sd0 = _init_state(H)
    full = _trainer(H, freeze_d=True)
    acc = _trainer(H, freeze_d=True, accumulation_steps=2)
    acc.schedulers = (WarmupCosineLR(acc.generator_optimizer, 10, 100), WarmupCosineLR(acc.discriminator_optimizer, 10, 100))
    batch = _batch(0, B=4)
    full.train_step(*batch)
    out1 = acc.train_step(*(t[:2] for t in batch))
    assert acc.generator_optimizer.step_count == 0 and acc.discriminator_optimizer.step_count == 0
    assert all(s.last_epoch == 0 for s in acc.schedulers)
    for k, v in acc.vocoder.state_dict().items():
        assert torch.equal(v.cpu(), sd0[k]), k                  # nothing moves inside a window
    out2 = acc.train_step(*(t[2:] for t in batch))
    assert set(out1) == set(out2) == {"generator_loss", "discriminator_loss", "mel_loss"}
    og, od = _oracle_arena_grads(full, sd0, batch)
    for name, ref, o_full, o_acc, bound in (("generator", og, full.generator_optimizer, acc.generator_optimizer, 0.08),
                                            ("discriminators", od, full.discriminator_optimizer, acc.discriminator_optimizer, 0.05)):
        e_full = float((o_full.flat_g.double().cpu() - ref).norm() / ref.norm())
        e_acc = float((o_acc.flat_g.double().cpu() * 0.5 - ref).norm() / ref.norm())
        print(f"[accum] {name}: e_full {e_full:.2e}  e_acc {e_acc:.2e}")
        assert e_full < bound, (name, e_full)
        assert e_acc <= 1.5 * e_full + 1e-6, (name, e_acc, e_full)
    for opt in (acc.generator_optimizer, acc.discriminator_optimizer):
        assert opt.step_count == 1 and set(opt.steps) == {1}
    assert all(s.last_epoch == 1 for s in acc.schedulers)      # once per optimizer step, not per call


def test_dropout_masks_differ_between_micro_steps(H):
    """Identical inputs and (inside a window) identical weights: with dropout 0.1 under the counter stream the two micro-steps draw
    different masks, so their losses differ; with dropout 0 they agree to summation order."""
    tr = _trainer(H, dropout=0.1, dropout_rng="counter", accumulation_steps=2)
    c0 = tr.dropout_rng.ctr_base
    a = tr.train_step(*_batch(1))
    c1 = tr.dropout_rng.ctr_base
    b = tr.train_step(*_batch(1))
    assert c0 < c1 < tr.dropout_rng.ctr_base                   # the stream advances on every call
    t0 = _trainer(H, dropout=0.0, accumulation_steps=2)
    a0, b0 = t0.train_step(*_batch(1)), t0.train_step(*_batch(1))
    print(f"[accum] generator loss of two micro-steps on one batch: dropout 0.1 {a['generator_loss']!r} {b['generator_loss']!r}; "
          f"dropout 0 {a0['generator_loss']!r} {b0['generator_loss']!r}")
    assert _rel(a0["generator_loss"], b0["generator_loss"]) < 2e-5
    assert _rel(a["generator_loss"], b["generator_loss"]) > 1e-4


def test_huge_max_grad_norm_is_the_unclipped_trainer(H):
    """max_grad_norm = 1e9 (coefficient exactly 1): two steps against a trainer without the argument, under the summation-order
    bound that test_captured_step_equals_eager_step uses between trainers (a second plain trainer is the noise floor)."""
    init = _init_state(H)
    ta, tb, tc = _trainer(H), _trainer(H, max_grad_norm=1e9), _trainer(H)
    for i in range(2):
        la, lc = ta.train_step(*_batch(i)), tc.train_step(*_batch(i))
        lb = tb.train_step(*_batch(i), return_tensors=True)
        assert set(lb) == set(la) | {"generator_grad_norm", "discriminator_grad_norm"}
        assert float(tb.generator_optimizer._clip_buf[1]) == 1.0 and float(tb.discriminator_optimizer._clip_buf[1]) == 1.0
        for k in la:
            assert _rel(la[k], float(lb[k].detach())) < 2e-5 + 5 * _rel(la[k], lc[k]), (i, k)
    d_clip, d_eager = _upd_dist(ta, tb, init), _upd_dist(ta, tc, init)
    print(f"[clip] update distance after 2 steps: max_grad_norm 1e9 vs none {d_clip:.2e}, none vs none {d_eager:.2e}")
    assert d_clip < 0.02 + 3 * d_eager
    assert set(ta.train_step(*_batch(2), return_tensors=True)) == {"generator_loss", "discriminator_loss", "mel_loss"}


def test_clipped_trainer_step_is_the_half_gradient_step(H):
    """max_grad_norm at half of each optimizer's first-step norm: the returned norms are the fp64 norms of the arenas (1e-5), and the
    parameter update is the unclipped AdamW update from coefficient x g (same state, a copy of the arena, step(grad_scale=coef))."""
    from hifigan_modified.optim import FlatAdamW
    probe = _trainer(H, max_grad_norm=1e9)
    r = probe.train_step(*_batch(0), return_tensors=True)
    n_g, n_d = float(r["generator_grad_norm"]), float(r["discriminator_grad_norm"])
    tr = _trainer(H, max_grad_norm=1.0)
    gopt, dopt = tr.generator_optimizer, tr.discriminator_optimizer
    assert gopt.max_grad_norm == dopt.max_grad_norm == 1.0
    gopt.max_grad_norm, dopt.max_grad_norm = 0.5 * n_g, 0.5 * n_d      # per optimizer; read again at every step
    p0 = {id(o): o.flat_p.clone() for o in (gopt, dopt)}
    r = tr.train_step(*_batch(0), return_tensors=True)
    for name, opt, key, n_probe in (("generator", gopt, "generator_grad_norm", n_g), ("discriminators", dopt, "discriminator_grad_norm", n_d)):
        norm64 = float(torch.linalg.vector_norm(opt.flat_g.double()))
        coef = float(opt._clip_buf[1])
        print(f"[clip] {name}: returned norm {float(r[key])!r}, fp64 norm of the arena {norm64!r}, probe norm {n_probe!r}, coefficient {coef!r}")
        assert r[key].is_cuda and abs(float(r[key]) - norm64) <= 1e-5 * norm64
        assert abs(coef - opt.max_grad_norm / (norm64 + 1e-6)) <= 1e-5 * coef
        # the discriminators' first gradient does not depend on anything clipped: exactly the probe's up to summation order; the
        # generator's is taken through discriminators whose update was clipped, so its norm has moved a little
        assert abs(coef - 0.5) < (1e-4 if opt is dopt else 0.1), (name, coef)
        ps = [torch.nn.Parameter(p0[id(opt)][o:o + p.numel()].view(p.shape).clone()) for p, o in zip(opt.params, opt.offsets)]
        plain = FlatAdamW(ps, lr=opt.lr, betas=opt.betas, eps=opt.eps, weight_decay=opt.weight_decay)
        assert plain.offsets == opt.offsets
        plain.flat_g.copy_(opt.flat_g)
        plain.step(grad_scale=coef, gathered=True)
        assert torch.equal(plain.flat_p, opt.flat_p), name       # g x (1 x coef) in both kernels: the same bits
        assert not torch.equal(plain.flat_p, p0[id(opt)])


def test_captured_window_equals_eager_window(H):
    """accumulation_steps 2, max_grad_norm 1.0, use_graph, graph_warmup 1: eight calls = four optimizer steps on changing batches
    (calls 0-1 eager warm-up of the two phases, 2-3 their captures, 4-7 replays) against an eager trainer with the same arguments,
    a second eager one as the noise floor; form and bounds of test_captured_step_equals_eager_step.  Then the replayed step follows
    the optimizer's max_grad_norm."""
    init = _init_state(H)
    kw = dict(accumulation_steps=2, max_grad_norm=1.0)
    ta, tb, tc = _trainer(H, **kw), _trainer(H, use_graph=True, graph_warmup=1, **kw), _trainer(H, **kw)
    for i in range(8):
        la, lb, lc = (t.train_step(*_batch(i)) for t in (ta, tb, tc))
        for k in la:
            assert _rel(la[k], lb[k]) < 2e-5 + 5 * _rel(la[k], lc[k]), (i, k, la, lb, lc)
    d_graph, d_eager = _upd_dist(ta, tb, init), _upd_dist(ta, tc, init)
    print(f"[accum] update distance after 4 windows: captured vs eager {d_graph:.2e}, eager vs eager {d_eager:.2e}")
    assert d_graph < 0.02 + 3 * d_eager
    for oa, ob in ((ta.generator_optimizer, tb.generator_optimizer), (ta.discriminator_optimizer, tb.discriminator_optimizer)):
        assert oa.steps == ob.steps and oa.step_count == ob.step_count == 4
    graphs = {k: st for k, st in tb._graphs.items() if st["graph"] is not None}
    assert len(graphs) == 2 and len({k[:-1] for k in graphs}) == 1 and {k[-1] for k in graphs} == {"accumulate", "step"}
    # a replay reads the optimizer's CURRENT max_grad_norm (state block, uploaded before the replay)
    gopt = tb.generator_optimizer
    n_before, c_before = float(gopt.grad_norm), float(gopt._clip_buf[1])
    assert abs(c_before - min(1.0, 1.0 / (n_before + 1e-6))) <= 1e-6
    gopt.max_grad_norm = 0.25 * n_before
    for i in (8, 9):
        r = tb.train_step(*_batch(i), return_tensors=True)
    n_after, c_after = float(r["generator_grad_norm"]), float(gopt._clip_buf[1])
    print(f"[accum] replayed clip: max_grad_norm 1.0 norm {n_before!r} coef {c_before!r}; max_grad_norm {gopt.max_grad_norm!r} norm {n_after!r} coef {c_after!r}")
    assert abs(c_after - min(1.0, gopt.max_grad_norm / (n_after + 1e-6))) <= 1e-6 * max(1.0, c_after)
    assert c_after != c_before and len([st for st in tb._graphs.values() if st["graph"] is not None]) == 2
    assert gopt.step_count == 5


def test_checkpoint_only_at_window_boundaries(H, tmp_path):
    init = _init_state(H)
    kw = dict(accumulation_steps=2, max_grad_norm=1.0)
    ta, tb = _trainer(H, **kw), _trainer(H, **kw)
    path = str(tmp_path / "ck.pt")
    ta.train_step(*_batch(0))
    tb.train_step(*_batch(0))
    with pytest.raises(RuntimeError, match="accumulation window"):
        tb.save_checkpoint(path)
    ta.train_step(*_batch(1))
    tb.train_step(*_batch(1))
    tb.save_checkpoint(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["accumulation_steps"] == 2 and ck["max_grad_norm"] == 1.0
    tc = _trainer(H, seed=5, **kw)               # other initial weights: the checkpoint must bring everything
    tc.load_checkpoint(path)
    for i in (2, 3):
        la, lb, lc = (t.train_step(*_batch(i)) for t in (ta, tb, tc))
        for k in la:
            assert _rel(la[k], lc[k]) < 2e-5 + 5 * _rel(la[k], lb[k]), (i, k, la, lb, lc)
    d_resumed, d_eager = _upd_dist(ta, tc, init), _upd_dist(ta, tb, init)
    print(f"[accum] update distance after the window behind a checkpoint: resumed vs uninterrupted {d_resumed:.2e}, eager vs eager {d_eager:.2e}")
    assert d_resumed < 0.02 + 3 * d_eager
    assert tc.generator_optimizer.steps == ta.generator_optimizer.steps and tc.generator_optimizer.step_count == 2


# ------------------------------------------------------------------------------------------------ data parallel
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _inputs4(seed=1, T=64):
    torch.manual_seed(seed)
    return (torch.randn(4, 80, T), (torch.randn(4, 1, T * HOP) * 0.5).clamp(-1, 1), torch.randn(4, 192), torch.randn(4, 384))


def _dp_worker(rank, world, port, q, mode, max_norm):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    from conftest import PKG, ROOT  # noqa: F401  (puts the package on sys.path)
    import hifigan_modified as H
    from hifigan_modified.parallel import GradSynchronizer, broadcast_parameters, init_distributed
    import torch.distributed as dist
    init_distributed("gloo")                    # two ranks share cuda:0; the collective goes through gloo
    dev = torch.device("cuda", 0)
    torch.manual_seed(rank)                     # different initial weights per rank: the broadcast must fix that
    voc = H.ModifiedHiFiGANVocoder(dropout=0.0, **CFG).to(dev)
    broadcast_parameters(voc)
    sync = GradSynchronizer(bucket_mib=1) if mode == "plain" else None
    tr = H.VocoderTrainer(voc, device=dev, mel_mode="stft", bucket_mib=1, grad_sync=sync, accumulation_steps=2, max_grad_norm=max_norm)

    def collectives():
        if mode == "plain":
            return sync.collectives
        return sum(ov.collectives for ov in tr._overlap.values())
    batch = _inputs4()
    counts = []
    for m in range(2):                          # this rank's two micro-batches of one clip: clips 2 rank + m
        i = 2 * rank + m
        tr.train_step(*(t[i:i + 1].to(dev) for t in batch))
        counts.append(collectives())
    sd = {k: v.detach().float().cpu().numpy() for k, v in voc.state_dict().items() if k.startswith(("generator.", "discriminators."))}
    q.put((rank, counts, sd, tr.generator_optimizer.step_count))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["overlap", "plain"])
def test_data_parallel_accumulation_equals_one_rank_full_batch(H, mode):
    """Two gloo ranks on this GPU, each accumulating two micro-batches of one clip, against one rank stepping once on all four
    clips, max_grad_norm set (at half the full-batch norm of each optimizer's first gradient, so the clip is live): update within
    the bounds of test_data_parallel_two_ranks_equal_one_rank_full_batch (rel-L2 0.05 D, 0.08 G).  The discriminators are compared
    with the ordinary full-batch step; the generator with a full-batch step whose discriminators stand still (lr 0), because inside
    a window the generator pass sees the discriminators of the window's start.  No collective on the non-stepping micro-step."""
    import torch.multiprocessing as mp
    batch = tuple(t.cuda() for t in _inputs4())
    probe = _trainer(H, max_grad_norm=1e9)
    sd0 = {k: v.detach().cpu().clone() for k, v in probe.vocoder.state_dict().items()}
    r = probe.train_step(*batch, return_tensors=True)
    max_norm = 0.5 * min(float(r["generator_grad_norm"]), float(r["discriminator_grad_norm"]))
    refs = {}
    for name, freeze in (("discriminators.", False), ("generator.", True)):
        t = _trainer(H, freeze_d=freeze, max_grad_norm=max_norm)
        t.train_step(*batch)
        assert float(t.generator_optimizer._clip_buf[1]) < 1.0 and float(t.discriminator_optimizer._clip_buf[1]) < 1.0
        refs[name] = {k: v.detach().float().cpu() for k, v in t.vocoder.state_dict().items()}

    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r_, world, port, q, mode, max_norm)) for r_ in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=300) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (_, c0, s0, steps0), (_, c1, s1, steps1) = res
    s0 = {k: torch.from_numpy(v) for k, v in s0.items()}
    s1 = {k: torch.from_numpy(v) for k, v in s1.items()}
    assert steps0 == steps1 == 1
    for c in (c0, c1):
        assert c[0] == 0 and c[1] >= 2, c                         # the first micro-step only accumulates locally
    for k in s0:                                                  # both ranks hold the same weights after the window, bit for bit
        assert torch.equal(s0[k], s1[k]), k
    for prefix, tol in (("discriminators.", 0.05), ("generator.", 0.08)):
        ref = refs[prefix]
        keys = [k for k in s0 if k.startswith(prefix) and not torch.equal(ref[k], sd0[k])]
        assert keys
        rel = _update_check(f"DP accumulation {prefix}", sd0, s0, {k: ref[k] for k in keys}, LR, tol)
        print(f"[dp2 x 2 micro-steps vs one rank, {mode}] {prefix} update rel-L2 {rel:.2e}")
