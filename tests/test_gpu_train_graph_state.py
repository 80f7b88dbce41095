"""The captured training step follows the host's per-step state (VocoderTrainer(use_graph=True)): fresh dropout masks at every replay
(the counter-offset Philox stream read from a device state block), a live lr / weight decay and lr schedule (AdamW's inputs read
from a device block refreshed before each replay), and checkpoint resume - including a restored state whose step counts split the
runs the graph was captured with, which must recapture.  Reference: nn.Dropout(0.1) live in train mode (grc_lora.py:151,162), the
warmup + cosine schedule of train_config.yaml:54-72, the checkpoint layout of complete_vocoder.py:463-468.

The mask kernels are checked bit for bit against a numpy restatement of Philox4x32-10 written here; the trainers against eager
trainers from the same seed with the bounds of tests/test_gpu_train_graph.py::test_captured_step_equals_eager_step."""
from ctypes import c_void_p

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CFG = dict(hidden_channels=64, upsample_factors=[4, 2])
HOP = 8
_M32 = np.uint64(0xFFFFFFFF)


@pytest.fixture(scope="module")
def H():
    import hifigan_modified as H
    from hifigan_modified import _native
    _native.lib()
    return H


# ------------------------------------------------------------------------------------------------ numpy Philox4x32-10 restatement
def _philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on uint64 arrays holding 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0) & _M32, np.uint64(k1) & _M32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def _mask_ref(n, p, key, ctr):
    """keep-mask: element block b = i/8 is counter (b lo, b hi, ctr lo, ctr hi) under key (key lo, key hi); 16 bits per element,
    keep iff u >= round(p * 2^16)."""
    nblk = (n + 7) // 8
    blk = np.arange(nblk, dtype=np.uint64)
    r = _philox(blk & _M32, blk >> np.uint64(32), np.full(nblk, ctr & 0xFFFFFFFF, np.uint64), np.full(nblk, ctr >> 32, np.uint64),
                key & 0xFFFFFFFF, key >> 32)
    u = np.empty((nblk, 8), dtype=np.uint64)
    for e in range(8):
        u[:, e] = (r[e >> 1] >> np.uint64(16 * (e & 1))) & np.uint64(0xFFFF)
    thresh = int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))
    return (u.reshape(-1)[:n] >= thresh).astype(np.uint8)


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _mask_dev(N, n, p, state, slot):
    m = torch.empty(n, dtype=torch.uint8, device="cuda")
    N.call("mv_dropout_mask_dev", c_void_p(m.data_ptr()), n, float(p), c_void_p(state.data_ptr()), slot, _stream())
    return m


CASES = [(1000, 0.1, 12345, 0, 0), (4099, 0.25, 2 ** 61 + 7, 2 ** 32 + 5, 3), (7, 0.5, 1, 2 ** 40, 0),
         (3 * 65536 + 5, 0.1, 0x123456789ABCDEF, 17, 2), (8 * 300000, 0.9, 2 ** 62 - 1, 2 ** 33 - 1, 1)]


@pytest.mark.parametrize("n,p,key,ctr_base,slot", CASES)
def test_mask_kernels_equal_philox_restatement(H, n, p, key, ctr_base, slot):
    from hifigan_modified import _native as N
    state = torch.tensor([key, ctr_base], dtype=torch.int64, device="cuda")
    dev = _mask_dev(N, n, p, state, slot).cpu().numpy()
    byval = torch.empty(n, dtype=torch.uint8, device="cuda")
    N.call("mv_dropout_mask_ctr", c_void_p(byval.data_ptr()), n, float(p), key, ctr_base + slot, _stream())
    ref = _mask_ref(n, p, key, ctr_base + slot)
    assert np.array_equal(dev, ref), (n, p, int((dev != ref).sum()))
    assert np.array_equal(byval.cpu().numpy(), ref)
    assert abs(ref.mean() - (1 - p)) < 0.05 + 3 / n ** 0.5


def test_counter_zero_equals_mv_dropout_mask(H):
    from hifigan_modified import _native as N
    for n, key in ((1000, 99), (4099, 2 ** 61 + 3), (13, 5)):
        a = torch.empty(n, dtype=torch.uint8, device="cuda")
        b = torch.empty(n, dtype=torch.uint8, device="cuda")
        N.call("mv_dropout_mask", c_void_p(a.data_ptr()), n, 0.1, key, _stream())
        N.call("mv_dropout_mask_ctr", c_void_p(b.data_ptr()), n, 0.1, key, 0, _stream())
        assert torch.equal(a, b)


def test_captured_mask_follows_uploaded_counter(H):
    """The device-state launch captured in a small graph: bump ctr_base on the host, upload it, replay - the mask is the restatement's at
    the new counter (the slot stays what the capture recorded)."""
    from hifigan_modified import _native as N
    from hifigan_modified.functional import DropoutRNG
    n, p, slot = 5003, 0.1, 2
    rng = DropoutRNG(0x0DDBA11CAFE, 40)
    rng.device_block("cuda")
    state = rng.block.dev.view(torch.int64)
    mask = torch.empty(n, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rng.upload()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        N.call("mv_dropout_mask_dev", c_void_p(mask.data_ptr()), n, float(p), c_void_p(state.data_ptr()), slot, _stream())
    for ctr_base in (40, 41, 2 ** 32 + 9):
        rng.ctr_base = ctr_base
        rng.upload()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(mask.cpu().numpy(), _mask_ref(n, p, rng.key, ctr_base + slot)), ctr_base


def test_dropout_mask_under_counter_rng_eager(H):
    """dropout_mask() under an active DropoutRNG, issued eagerly: slot k of the step is the stream at ctr_base + k."""
    from hifigan_modified import functional as Fn
    rng = Fn.DropoutRNG(777, 2 ** 32 - 1)
    with Fn.use_dropout_rng(rng):
        a = Fn.dropout_mask((2, 64, 37), 0.1, "cuda")
        b = Fn.dropout_mask((2, 64, 37), 0.1, "cuda")
    assert rng.slots_used == 2
    assert np.array_equal(a.reshape(-1).cpu().numpy(), _mask_ref(a.numel(), 0.1, 777, 2 ** 32 - 1))
    assert np.array_equal(b.reshape(-1).cpu().numpy(), _mask_ref(b.numel(), 0.1, 777, 2 ** 32))
    rng.advance()
    assert rng.ctr_base == 2 ** 32 + 1 and Fn._dropout_rng is None


# ------------------------------------------------------------------------------------------------ AdamW with device hyper-parameters
def test_adamw_hp_bit_identical_to_dev_and_opcheck(H):
    from torch.library import opcheck
    from hifigan_modified.torch_ops import OPS as ops      # (registers the operators)
    torch.manual_seed(3)
    n = 70001
    p0, g = torch.randn(n, device="cuda"), torch.randn(n, device="cuda")
    m0, v0 = torch.randn(n, device="cuda") * 0.1, torch.rand(n, device="cuda") * 0.01
    hp = (2e-4, 0.8, 0.99, 1e-8, 1e-4)
    for t in (1, 2, 7, 1000):
        step = torch.full((1,), t, dtype=torch.int32, device="cuda")
        pa, ma, va = p0.clone(), m0.clone(), v0.clone()
        pb, mb, vb = p0.clone(), m0.clone(), v0.clone()
        ops.fused_adamw_dev_(pa, g, ma, va, *hp, step, 0.5)
        ops.fused_adamw_hp_(pb, g, mb, vb, torch.tensor(hp, dtype=torch.float32, device="cuda"), step, 0.5)
        assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb), t
    hpt = torch.tensor(hp, dtype=torch.float32, device="cuda")
    opcheck(ops.fused_adamw_hp_, (p0.clone(), g, m0.clone(), v0.clone(), hpt, torch.ones(1, dtype=torch.int32, device="cuda"), 1.0),
            test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(RuntimeError):
        ops.fused_adamw_hp_(p0.cpu(), g.cpu(), m0.cpu(), v0.cpu(), hpt.cpu(), torch.ones(1, dtype=torch.int32), 1.0)


# ------------------------------------------------------------------------------------------------ trainers
def _vocoder(H, dropout, seed=0):
    torch.manual_seed(seed)
    return H.ModifiedHiFiGANVocoder(dropout=dropout, **CFG).to("cuda")


def _trainer(H, use_graph, dropout=0.1, seed=0, sched=None, lr=2e-5, **kw):
    """lr 2e-5 (a tenth of the default): AdamW moves every parameter by ~lr whatever the gradient's size, so summation-order noise
    that flips a near-zero gradient's sign spreads through the GAN trajectory in proportion to lr - at 2e-4 two runs drift apart by
    ~1e-4 in the losses within five steps; a mask that differs moves that same step's losses by ~1e-2 at any lr."""
    voc = _vocoder(H, dropout, seed)
    gopt, dopt = H.VocoderTrainer.default_optimizers(voc, lr=lr)
    scheds = ()
    if sched is not None:
        from hifigan_modified.optim import WarmupCosineLR
        scheds = (WarmupCosineLR(gopt, *sched), WarmupCosineLR(dopt, *sched))
    return H.VocoderTrainer(voc, gopt, dopt, device=torch.device("cuda"), use_graph=use_graph, schedulers=scheds, **kw)


def _batch(i, B=2, T=64):
    g = torch.Generator().manual_seed(100 + i)
    return (torch.randn(B, 80, T, generator=g).cuda(), (torch.randn(B, 1, T * HOP, generator=g) * 0.5).clamp(-1, 1).cuda(),
            torch.randn(B, 192, generator=g).cuda(), torch.randn(B, 384, generator=g).cuda())


def _rel(a, b):
    return abs(a - b) / max(abs(a), 1e-12)


class _LossCheck:
    """captured (lb) vs eager (la), with a second eager trainer (lc) as the noise floor.  test_captured_step_equals_eager_step's form
    (2e-5 + 5x the eager-vs-eager difference at that step) is too tight once dropout is live: the GAN losses pick up fp32
    summation-order noise from the atomics step by step, and the one eager-vs-eager sample at a step can be far below it (a suite run
    measured 4.5e-5 captured-vs-eager against 1.3e-6 eager-vs-eager at step 4, while the update distance had the captured run closer
    to the eager one than two eager runs are).  So: 1e-4 + 5x the largest eager-vs-eager difference seen so far.  Masks repeated
    from the capture (the keys frozen into the graph) move the losses by orders of magnitude more."""

    def __init__(self):
        self.noise = 0.0

    def __call__(self, i, la, lb, lc):
        self.noise = max([self.noise] + [_rel(la[k], lc[k]) for k in la])
        worst = max(_rel(la[k], lb[k]) for k in la)
        print(f"[train-state] step {i}: captured vs eager {worst:.1e}, eager vs eager (running max) {self.noise:.1e}")
        for k in la:
            assert _rel(la[k], lb[k]) < 1e-4 + 5 * self.noise, (i, k, la, lb, lc)


def _upd_dist(t1, t2, init):
    num = den = 0.0
    for (k, p1), (_, p2) in zip(t1.vocoder.state_dict().items(), t2.vocoder.state_dict().items()):
        if p1.is_floating_point() and "embedding_extractor" not in k:
            num += float((p1.double() - p2.double()).pow(2).sum())
            den += float((p1.double().cpu() - init[k].double()).pow(2).sum())
    return (num / den) ** 0.5


def _init(H, dropout=0.1):
    return {k: v.detach().cpu().clone() for k, v in _vocoder(H, dropout).state_dict().items()}


def _run_pair(H, steps, **kw):
    init = _init(H)
    ta, tb, tc = _trainer(H, False, dropout_rng="counter", **kw), _trainer(H, True, **kw), _trainer(H, False, dropout_rng="counter", **kw)
    assert tb.dropout_rng is not None and tb.dropout_rng.key == ta.dropout_rng.key
    check = _LossCheck()
    for i in range(steps):
        la, lb, lc = ta.train_step(*_batch(i)), tb.train_step(*_batch(i)), tc.train_step(*_batch(i))
        check(i, la, lb, lc)
    assert any(st["graph"] is not None for st in tb._graphs.values())
    d_graph, d_eager = _upd_dist(ta, tb, init), _upd_dist(ta, tc, init)
    print(f"[train-state] update distance after {steps} steps: captured vs eager {d_graph:.2e}, eager vs eager {d_eager:.2e}")
    assert d_graph < 0.02 + 3 * d_eager
    return ta, tb


def test_captured_dropout_equals_eager_dropout(H):
    """dropout 0.1, six steps on changing batches (two eager warm-up steps, the capture, three replays): each replay draws the masks the
    eager counter-stream step draws.  (With the keys frozen into the graph, replays 2+ reuse the capture's masks.)"""
    ta, tb = _run_pair(H, 6)
    assert ta.dropout_rng.ctr_base == tb.dropout_rng.ctr_base > 0
    for oa, ob in ((ta.generator_optimizer, tb.generator_optimizer), (ta.discriminator_optimizer, tb.discriminator_optimizer)):
        assert oa.steps == ob.steps and oa.step_count == ob.step_count == 6


def test_captured_step_follows_lr_schedule(H):
    ta, tb = _run_pair(H, 6, sched=(2, 6, 1e-6))
    for oa, ob in ((ta.generator_optimizer, tb.generator_optimizer), (ta.discriminator_optimizer, tb.discriminator_optimizer)):
        assert oa.lr == ob.lr
    assert ta.schedulers[0].last_epoch == tb.schedulers[0].last_epoch == 6


def test_replay_reads_live_lr_and_weight_decay(H):
    """lr = 0 and weight_decay = 0 set on the host after the capture: the next replay leaves every arena parameter bit for bit, while the
    AdamW moments still move (the step ran; only its inputs changed)."""
    tb = _trainer(H, True)
    for i in range(4):
        tb.train_step(*_batch(i))
    opts = (tb.generator_optimizer, tb.discriminator_optimizer)
    for o in opts:
        o.lr, o.weight_decay = 0.0, 0.0
    before = [(o.flat_p.clone(), o.exp_avg.clone(), o.exp_avg_sq.clone()) for o in opts]
    tb.train_step(*_batch(4))
    torch.cuda.synchronize()
    for o, (p, m, v) in zip(opts, before):
        assert torch.equal(o.flat_p, p)
        assert not torch.equal(o.exp_avg, m) and not torch.equal(o.exp_avg_sq, v)
        assert o.step_count == 5
    for o in opts:
        o.lr = 2e-5
    tb.train_step(*_batch(5))
    torch.cuda.synchronize()
    assert not torch.equal(opts[0].flat_p, before[0][0])


def test_resume_matches_eager_and_split_runs_recapture(H, tmp_path):
    """3 steps, save_checkpoint, 2 steps, load_checkpoint, 3 steps - a captured trainer against an eager one (dropout 0.1, warmup +
    cosine schedule): step counts, optimizer layout and lr exactly, losses within the bounds above.  Then a checkpoint whose
    generator step counts split a run: the captured trainer recaptures and still matches."""
    init = _init(H)
    kw = dict(sched=(2, 12, 1e-6))
    ta, tb, tc = _trainer(H, False, dropout_rng="counter", **kw), _trainer(H, True, **kw), _trainer(H, False, dropout_rng="counter", **kw)
    trs = (ta, tb, tc)
    paths = [str(tmp_path / f"ck{j}.pt") for j in range(3)]
    check = _LossCheck()

    def steps(idx):
        for i in idx:
            la, lb, lc = (t.train_step(*_batch(i)) for t in trs)
            check(i, la, lb, lc)

    def same_state():
        for oa, ob in ((ta.generator_optimizer, tb.generator_optimizer), (ta.discriminator_optimizer, tb.discriminator_optimizer)):
            assert oa.steps == ob.steps and oa.step_count == ob.step_count and oa.lr == ob.lr
            sa, sb = oa.torch_state_dict(), ob.torch_state_dict()
            assert sorted(sa["state"]) == sorted(sb["state"])
            assert all(float(sa["state"][k]["step"]) == float(sb["state"][k]["step"]) for k in sa["state"])
            assert sa["param_groups"][0]["lr"] == sb["param_groups"][0]["lr"]
        assert ta.dropout_rng.state_dict() == tb.dropout_rng.state_dict()

    steps(range(3))
    for t, pth in zip(trs, paths):
        t.save_checkpoint(pth)
    ck = torch.load(paths[1], weights_only=True)
    assert "dropout_rng_state" in ck and len(ck["scheduler_state_dicts"]) == 2
    steps(range(3, 5))
    for t, pth in zip(trs, paths):
        t.load_checkpoint(pth)
    assert tb.generator_optimizer.step_count == 3 and tb.schedulers[0].last_epoch == 3
    same_state()
    steps(range(5, 8))
    same_state()
    assert ta.generator_optimizer.step_count == 6
    d_graph, d_eager = _upd_dist(ta, tb, init), _upd_dist(ta, tc, init)
    print(f"[train-state] resume: update distance captured vs eager {d_graph:.2e}, eager vs eager {d_eager:.2e}")
    assert d_graph < 0.02 + 3 * d_eager

    # a restored state whose counts split the generator's single run: parameter `mid` one step behind the others
    graphs_before = {sig: st["graph"] for sig, st in tb._graphs.items()}
    split = [str(tmp_path / f"split{j}.pt") for j in range(3)]
    for t, src, dst in zip(trs, paths, split):
        t.save_checkpoint(src)
        ck = torch.load(src, weights_only=True)
        gopt = t.generator_optimizer
        mid = gopt.torch_index[len(gopt.params) // 2]
        st = ck["generator_optimizer_state_dict"]["state"][mid]
        st["step"] = st["step"] - 1
        torch.save(ck, dst)
        t.load_checkpoint(dst)
    assert len(tb.generator_optimizer._planned_runs()) == 3
    steps(range(8, 11))
    same_state()
    assert any(st["graph"] is not None and st["graph"] is not graphs_before.get(sig) for sig, st in tb._graphs.items())
    assert len(next(st for st in tb._graphs.values() if st["graph"] is not None)["gstate"]["runs"]) == 3
    d_graph, d_eager = _upd_dist(ta, tb, init), _upd_dist(ta, tc, init)
    print(f"[train-state] split-run resume: update distance captured vs eager {d_graph:.2e}, eager vs eager {d_eager:.2e}")
    assert d_graph < 0.02 + 3 * d_eager
