"""CPU-side checks of the captured-step state work: the warmup + cosine lr schedule (train_config.yaml:54-72: warmup_steps, scheduler
"cosine", min_lr) against torch's LambdaLR with the same factor, its state_dict round trip, the FlatAdamW form (sets `.lr`), the
counter-based dropout stream's host bookkeeping, and the C-ABI entries the captured step launches (declared and exported)."""
import math

import pytest
import torch

# LambdaLR warns when stepped without an optimizer step in between: the comparison steps only the schedules
pytestmark = pytest.mark.filterwarnings("ignore:Detected call of `lr_scheduler.step\\(\\)`")


def _factor(W, S, m):
    def f(s):
        if s < W:
            return (s + 1) / W
        return m + (1 - m) * 0.5 * (1 + math.cos(math.pi * min(1.0, (s - W) / (S - W))))
    return f


def _toy_adamw(lr):
    torch.manual_seed(0)
    return torch.optim.AdamW([torch.nn.Parameter(torch.randn(4, 3)), torch.nn.Parameter(torch.randn(3))], lr=lr)


@pytest.mark.parametrize("W,S,base,min_lr", [(5, 20, 2e-4, 1e-6), (0, 12, 1e-3, 0.0), (3, 4, 5e-4, 5e-5), (2000, 2040, 2e-4, 1e-6)])
def test_warmup_cosine_equals_lambda_lr(W, S, base, min_lr):
    from hifigan_modified.optim import WarmupCosineLR
    a, b = _toy_adamw(base), _toy_adamw(base)
    ours = WarmupCosineLR(a, W, S, min_lr=min_lr)
    ref = torch.optim.lr_scheduler.LambdaLR(b, _factor(W, S, min_lr / base))
    for s in range(S + 10):
        assert abs(a.param_groups[0]["lr"] - b.param_groups[0]["lr"]) <= 1e-12, (s, a.param_groups[0]["lr"], b.param_groups[0]["lr"])
        assert abs(ours.get_last_lr()[0] - ref.get_last_lr()[0]) <= 1e-12
        ours.step()
        ref.step()
    assert abs(a.param_groups[0]["lr"] - min_lr) <= 1e-12          # past total_steps the schedule holds min_lr


def test_warmup_cosine_shape():
    from hifigan_modified.optim import WarmupCosineLR
    opt = _toy_adamw(1e-3)
    sch = WarmupCosineLR(opt, 4, 14, min_lr=1e-5)
    lrs = []
    for _ in range(16):
        lrs.append(opt.param_groups[0]["lr"])
        sch.step()
    assert lrs[:4] == pytest.approx([2.5e-4, 5e-4, 7.5e-4, 1e-3], abs=1e-15)      # linear warmup reaches the base lr at s = W - 1
    assert all(x >= y for x, y in zip(lrs[3:], lrs[4:]))                          # then non-increasing
    assert lrs[14] == pytest.approx(1e-5, abs=1e-15) and lrs[15] == pytest.approx(1e-5, abs=1e-15)


def test_warmup_cosine_state_dict_resumes():
    from hifigan_modified.optim import WarmupCosineLR
    a = _toy_adamw(2e-4)
    sa = WarmupCosineLR(a, 3, 15, min_lr=1e-6)
    for _ in range(5):
        sa.step()
    sd = sa.state_dict()
    tail = []
    for _ in range(12):
        sa.step()
        tail.append(a.param_groups[0]["lr"])
    b = _toy_adamw(7e-3)                                   # a different lr: the restored state decides
    sb = WarmupCosineLR(b, 1, 2)
    sb.load_state_dict(sd)
    assert b.param_groups[0]["lr"] == pytest.approx(WarmupCosineLR(_toy_adamw(2e-4), 3, 15, 1e-6).base_lrs[0] *
                                                    _factor(3, 15, 1e-6 / 2e-4)(5), abs=1e-15)
    resumed = []
    for _ in range(12):
        sb.step()
        resumed.append(b.param_groups[0]["lr"])
    assert resumed == tail


def test_warmup_cosine_drives_flat_adamw_lr():
    """FlatAdamW keeps one lr as `.lr` (no param_groups): the schedule sets it to LambdaLR's values.  (A FlatAdamW arena needs a GPU;
    the schedule only touches `.lr`, so a bare instance stands in for it here.)"""
    from hifigan_modified.optim import FlatAdamW, WarmupCosineLR
    flat = object.__new__(FlatAdamW)
    flat.lr = 2e-4
    ref_opt = _toy_adamw(2e-4)
    sch = WarmupCosineLR(flat, 2, 6, min_lr=1e-6)
    ref = torch.optim.lr_scheduler.LambdaLR(ref_opt, _factor(2, 6, 1e-6 / 2e-4))
    for _ in range(9):
        assert abs(flat.lr - ref_opt.param_groups[0]["lr"]) <= 1e-12
        sch.step()
        ref.step()


def test_warmup_cosine_rejects_bad_lengths():
    from hifigan_modified.optim import WarmupCosineLR
    with pytest.raises(ValueError):
        WarmupCosineLR(_toy_adamw(1e-3), 10, 10)
    with pytest.raises(ValueError):
        WarmupCosineLR(_toy_adamw(1e-3), 10, 5)
    with pytest.raises(ValueError):
        WarmupCosineLR(_toy_adamw(1e-3), -1, 5)


def test_dropout_rng_host_bookkeeping():
    from hifigan_modified.functional import DropoutRNG
    torch.manual_seed(5)
    a = DropoutRNG.from_torch()
    torch.manual_seed(5)
    b = DropoutRNG.from_torch()
    assert a.key == b.key and 0 <= a.key < 2 ** 62 and a.ctr_base == 0
    a.slots_used = 3
    a.advance()
    assert (a.ctr_base, a.slots_used) == (3, 0)
    a.advance(3)
    assert a.ctr_base == 6
    c = DropoutRNG(0)
    c.load_state_dict(a.state_dict())
    assert (c.key, c.ctr_base) == (a.key, 6)


def test_header_declares_and_library_exports_state_entries():
    from hifigan_modified import _native
    protos = _native.declared_symbols()
    for name in ("mv_dropout_mask_ctr", "mv_dropout_mask_dev", "mv_adamw_flat_hp"):
        assert name in protos, name
        assert hasattr(_native.lib(), name), name
    from ctypes import c_float, c_long, c_void_p
    assert protos["mv_dropout_mask_ctr"][1] == [c_void_p, c_long, c_float, c_long, c_long, c_void_p]
    assert protos["mv_dropout_mask_dev"][1] == [c_void_p, c_long, c_float, c_void_p, c_long, c_void_p]
    assert protos["mv_adamw_flat_hp"][1] == [c_void_p] * 4 + [c_long, c_void_p, c_void_p, c_float, c_void_p]


def test_trainer_signature_has_state_options():
    import inspect
    from hifigan_modified import VocoderTrainer
    sig = inspect.signature(VocoderTrainer.__init__)
    assert sig.parameters["dropout_rng"].default is None and "schedulers" in sig.parameters
