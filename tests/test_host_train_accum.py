"""Gradient accumulation and max_grad_norm clipping, host side: the trainers' argument validation (before anything touches a GPU)
and the new entry points of the built library."""
import pytest

NEW_SYMBOLS = ("mv_multi_gather_acc", "mv_zero_f32", "mv_grad_norm", "mv_adamw_flat_clip")


def test_trainers_reject_bad_accumulation_and_clip_arguments():
    import hifigan_modified as H
    voc = H.ModifiedHiFiGANVocoder(hidden_channels=64, upsample_factors=[4, 2])
    for bad in (0, 1.5, -2, True, "2"):
        with pytest.raises(ValueError, match="accumulation_steps"):
            H.VocoderTrainer(voc, accumulation_steps=bad)
        with pytest.raises(ValueError, match="accumulation_steps"):
            H.HiFiGANTrainer(None, accumulation_steps=bad)
    for bad in (0, -1, 0.0, float("nan"), "1"):
        with pytest.raises(ValueError, match="max_grad_norm"):
            H.VocoderTrainer(voc, max_grad_norm=bad)
        with pytest.raises(ValueError, match="max_grad_norm"):
            H.HiFiGANTrainer(None, max_grad_norm=bad)


def test_accumulation_needs_the_flat_arena():
    """A torch.optim optimizer has no arena to accumulate or clip on: refused at construction, not at the first step."""
    import torch
    import hifigan_modified as H
    voc = H.ModifiedHiFiGANVocoder(hidden_channels=64, upsample_factors=[4, 2])
    g = torch.optim.AdamW(voc.generator.parameters())
    d = torch.optim.AdamW(voc.discriminators.parameters())
    for kw in (dict(accumulation_steps=2), dict(max_grad_norm=1.0)):
        with pytest.raises(ValueError, match="FlatAdamW"):
            H.VocoderTrainer(voc, g, d, device=torch.device("cpu"), grad_sync=False, **kw)
    H.VocoderTrainer(voc, g, d, device=torch.device("cpu"), grad_sync=False)        # the defaults still take any optimizer


def test_new_entry_points_are_declared_and_exported():
    from hifigan_modified import _native
    declared = _native.declared_symbols()
    lib = _native.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
    assert lib.mv_abi_version() >= 1
