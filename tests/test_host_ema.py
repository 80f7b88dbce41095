"""The generator's weight EMA, host side: the two new entry points of the built library, the warm-up decay schedule of
optim.ArenaEMA (pure host arithmetic: the arena here is a stand-in on the CPU) and the argument validation."""
import math
from types import SimpleNamespace

import pytest
import torch

NEW_SYMBOLS = ("mv_ema_update", "mv_swap_f32")


def _ema(decay, **kw):
    from hifigan_modified.optim import ArenaEMA
    opt = SimpleNamespace(numel=16, flat_p=torch.arange(16, dtype=torch.float32), ema=None)
    return ArenaEMA(opt, decay, **kw), opt


def test_new_entry_points_are_declared_and_exported():
    from hifigan_modified import _native
    declared = _native.declared_symbols()
    lib = _native.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
    assert len(declared["mv_ema_update"][1]) == 6 and len(declared["mv_swap_f32"][1]) == 4


def test_shadow_starts_as_a_copy_and_attaches_itself():
    ema, opt = _ema(0.999)
    assert ema.num_updates == 0 and opt.ema is ema
    assert ema.shadow.dtype == torch.float32 and torch.equal(ema.shadow, opt.flat_p)
    assert ema.shadow.data_ptr() != opt.flat_p.data_ptr()


def test_current_decay_follows_the_warmup_formula():
    ema, _ = _ema(0.999)
    for n, want in ((0, 0.1), (1, 2 / 11), (90, 0.91)):
        ema.num_updates = n
        assert ema.current_decay() == want, (n, ema.current_decay())
        assert ema.one_minus_decay().dtype.name == "float32" and float(ema.one_minus_decay()) == float(torch.tensor(1 - want).float())
    # (1 + n) / (10 + n) > 0.999  <=>  n > 8990: below that the ramp, from 8991 on the decay itself, exactly
    for n in (2, 500, 8989):
        ema.num_updates = n
        assert ema.current_decay() == (1 + n) / (10 + n) < 0.999
    ema.num_updates = 8990                       # the ramp reaches 0.999 itself here (8991 / 9000), up to the division's rounding
    assert math.isclose(ema.current_decay(), 0.999, rel_tol=1e-15)
    for n in (8991, 8992, 10 ** 6):
        ema.num_updates = n
        assert (1 + n) / (10 + n) > 0.999 and ema.current_decay() == 0.999


def test_without_warmup_the_decay_is_constant():
    ema, _ = _ema(0.9, warmup=False)
    for n in (0, 1, 5, 10 ** 5):
        ema.num_updates = n
        assert ema.current_decay() == 0.9


def test_state_dict_round_trip_on_the_host():
    ema, _ = _ema(0.99)
    ema.num_updates = 7
    ema.shadow.mul_(0.5)
    sd = ema.state_dict()
    assert set(sd) == {"decay", "warmup", "num_updates", "shadow"} and sd["shadow"].dim() == 1
    other, _ = _ema(0.5, warmup=False)
    other.load_state_dict(sd)
    assert (other.decay, other.warmup, other.num_updates) == (0.99, True, 7) and torch.equal(other.shadow, ema.shadow)
    assert other.current_decay() == ema.current_decay()
    sd["shadow"] = sd["shadow"][:8]
    with pytest.raises(ValueError, match="shadow"):
        other.load_state_dict(sd)


@pytest.mark.parametrize("bad", [0, 1, 0.0, 1.0, -0.1, 1.5, float("nan"), "0.9", True, None])
def test_bad_decay_raises(bad):
    with pytest.raises(ValueError, match="decay"):
        _ema(bad)


def test_trainer_ema_needs_the_flat_arena():
    """A torch.optim optimizer has no arena to average: refused at construction; without ema_decay any optimizer still does."""
    import hifigan_modified as H
    voc = H.ModifiedHiFiGANVocoder(hidden_channels=64, upsample_factors=[4, 2])
    g = torch.optim.AdamW(voc.generator.parameters())
    d = torch.optim.AdamW(voc.discriminators.parameters())
    with pytest.raises(ValueError, match="FlatAdamW"):
        H.VocoderTrainer(voc, g, d, device=torch.device("cpu"), grad_sync=False, ema_decay=0.999)
    tr = H.VocoderTrainer(voc, g, d, device=torch.device("cpu"), grad_sync=False)
    assert tr.ema is None
    with pytest.raises(RuntimeError, match="EMA"):
        with tr.ema_weights():
            pass
    with pytest.raises(RuntimeError, match="EMA"):
        tr.evaluate(torch.zeros(1, 80, 8), torch.zeros(1, 1, 64), weights="ema")
    with pytest.raises(ValueError, match="weights"):
        tr.evaluate(torch.zeros(1, 80, 8), torch.zeros(1, 1, 64), weights="average")
