"""training.GradWindow, the accumulation window both trainers share, driven on the CPU with stub optimizers that record what the
window asks of them: zero_arena(), gather_grads(accumulate=...), step(grad_scale=..., max_grad_norm=...)."""
import pytest
import torch

CALLS = 7


def _stub_cls():
    from hifigan_modified.optim import FlatAdamW

    class StubOpt(FlatAdamW):            # a FlatAdamW to isinstance(), none of its arena: only the calls are recorded
        def __init__(self):
            self.log, self.max_grad_norm, self.flat_g = [], None, torch.zeros(8)

        def zero_arena(self):
            self.log.append(("zero",))

        def gather_grads(self, accumulate=False):
            self.log.append(("gather", accumulate))
            return self.flat_g

        def step(self, **kw):
            self.log.append(("step", kw))

    return StubOpt


def _drive(n_acc, max_grad_norm=None, norm_at_call=None):
    """CALLS train_step-shaped calls on two optimizers; returns (window, per-call records)."""
    from hifigan_modified.training import GradWindow
    Stub = _stub_cls()
    a, b = Stub(), Stub()
    w = GradWindow("T", n_acc, max_grad_norm, grad_sync=False)
    w.adopt(a, b)
    calls = []
    for c in range(CALLS):
        if norm_at_call and c in norm_at_call:
            a.max_grad_norm = norm_at_call[c]
        a.log, b.log = [], []
        x = torch.ones(3, requires_grad=True)
        do_step = w.begin_call((a, b))
        sa = w.backward((x * 2).sum(), a, do_step)
        sb = w.backward((x * 3).sum(), b, do_step)
        if sa is not None:
            w.apply(a, sa)
            w.apply(b, sb)
        w.end_call()
        calls.append(dict(do_step=do_step, scales=(sa, sb), a=list(a.log), b=list(b.log), position=w.position))
    return w, calls


@pytest.mark.parametrize("n_acc", [1, 3])
def test_window_pattern(n_acc):
    w, calls = _drive(n_acc)
    assert [c["do_step"] for c in calls] == [(i % n_acc) == n_acc - 1 for i in range(CALLS)]
    assert [c["position"] for c in calls] == [(i + 1) % n_acc for i in range(CALLS)]
    for i, c in enumerate(calls):
        first = n_acc > 1 and i % n_acc == 0
        for log in (c["a"], c["b"]):
            assert (("zero",) in log) == first, (i, log)            # only at a window's first call, only when N > 1
            assert log.count(("zero",)) <= 1
            if first:
                assert log[0] == ("zero",)                          # before anything is gathered
            assert [e for e in log if e[0] == "gather"] == [("gather", n_acc > 1)]     # accumulate: never for N = 1
            steps = [e[1] for e in log if e[0] == "step"]
            assert len(steps) == (1 if c["do_step"] else 0)
            for kw in steps:
                assert kw == {"grad_scale": 1.0 / n_acc, "gathered": True}          # exactly 1/N (world 1), no max_grad_norm
        assert c["scales"] == ((1.0 / n_acc,) * 2 if c["do_step"] else (None, None))
    assert w.checkpoint_extras() == ({} if n_acc == 1 else {"accumulation_steps": n_acc, "max_grad_norm": None})


@pytest.mark.parametrize("n_acc", [1, 3])
def test_max_grad_norm_is_forwarded_from_the_optimizer_at_every_step(n_acc):
    w, calls = _drive(n_acc, max_grad_norm=2, norm_at_call={4: 0.25})
    assert w.max_grad_norm == 2.0 and w.checkpoint_extras() == {"accumulation_steps": n_acc, "max_grad_norm": 2.0}
    for i, c in enumerate(calls):
        for name, want in (("a", 2.0 if i < 4 else 0.25), ("b", 2.0)):      # adopt() set 2.0 on both; a's own value changes at call 4
            steps = [e[1] for e in c[name] if e[0] == "step"]
            assert len(steps) == (1 if c["do_step"] else 0)
            for kw in steps:
                assert kw == {"grad_scale": 1.0 / n_acc, "gathered": True, "max_grad_norm": want}


def test_boundary_reset_and_default_extras():
    from hifigan_modified.training import GradWindow
    Stub = _stub_cls()
    opt = Stub()
    w = GradWindow("T", 3, None, grad_sync=False)
    w.assert_boundary("VocoderTrainer.save_checkpoint")             # a fresh window is at a boundary
    x = torch.ones(2, requires_grad=True)
    for _ in range(2):
        assert w.backward(x.sum(), opt, w.begin_call((opt,))) is None
        w.end_call()
    for who in ("VocoderTrainer.save_checkpoint", "HiFiGANTrainer.save_checkpoint"):
        with pytest.raises(RuntimeError, match="in the middle of an accumulation window") as e:
            w.assert_boundary(who)
        assert str(e.value).startswith(who + ":") and "2 of 3" in str(e.value)
    w.reset()
    assert w.position == 0
    w.assert_boundary("VocoderTrainer.save_checkpoint")
    assert w.begin_call((opt,)) is False and opt.log[-1] == ("zero",)       # and the next call opens a new window
    assert GradWindow("T", grad_sync=False).checkpoint_extras() == {}


def test_arguments_and_optimizer_kinds():
    from hifigan_modified.training import GradWindow
    for bad in (0, 1.5, -2, True, "2"):
        with pytest.raises(ValueError, match="T: accumulation_steps"):
            GradWindow("T", bad)
    for bad in (0, -1, 0.0, float("nan"), "1"):
        with pytest.raises(ValueError, match="T: max_grad_norm"):
            GradWindow("T", 1, bad)
    assert GradWindow("T").grad_sync is False                       # no process group: no gradient exchange
    plain = torch.optim.SGD([torch.nn.Parameter(torch.zeros(2))], lr=0.5)
    for kw in (dict(accumulation_steps=2), dict(max_grad_norm=1.0)):
        with pytest.raises(ValueError, match="T: .*FlatAdamW.*got a SGD"):
            GradWindow("T", grad_sync=False, **kw).adopt(plain)
    # the defaults take any optimizer: it steps inside backward() on its own .grad tensors, nothing is left for apply()
    w = GradWindow("T", grad_sync=False)
    w.adopt(plain)
    p = plain.param_groups[0]["params"][0]
    assert w.backward((p * torch.tensor([1.0, 2.0])).sum(), plain, w.begin_call((plain,))) is None
    assert torch.equal(p.detach(), torch.tensor([-0.5, -1.0]))
