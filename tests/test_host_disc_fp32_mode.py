"""The discriminators' fp32 operand switch (host state only): validation, propagation, state_dict."""
import pytest
import torch


def test_fp32_operand_switch():
    import hifigan_modified as H
    d = H.HiFiGANDiscriminators()
    keys = list(d.state_dict().keys())
    subs = list(d.mpd.discriminators) + list(d.msd.discriminators)
    assert len(subs) == 8
    assert d.fp32_operands == "exact" and all(s.fp32_operands == "exact" for s in subs)
    assert d.set_fp32_operands("split") is d
    assert all(m.fp32_operands == "split" for m in [d, d.mpd, d.msd] + subs)
    assert list(d.state_dict().keys()) == keys and len(list(d.buffers())) == 0
    assert d.mpd.set_fp32_operands("exact") is d.mpd
    assert all(s.fp32_operands == "exact" for s in d.mpd.discriminators)
    assert all(s.fp32_operands == "split" for s in d.msd.discriminators)
    for bad in ("fast", "", None, "Split"):
        with pytest.raises(ValueError):
            d.set_fp32_operands(bad)
    with pytest.raises(ValueError):
        H.Discriminator2D(2).set_fp32_operands("bf16")
    assert H.Discriminator1D(2).set_fp32_operands("split").fp32_operands == "split"
    assert H.MultiScaleDiscriminator().set_fp32_operands("split").fp32_operands == "split"


def test_split_mode_leaves_cpu_and_16bit_routes_alone():
    """CPU tensors never reach the GPU stack; 16-bit storage takes the MFMA stack in either mode."""
    import hifigan_modified as H
    from hifigan_modified import disc_fused
    m = H.Discriminator2D(3).set_fp32_operands("split")
    assert not disc_fused.supported(torch.zeros(1, 1, 30), m)
    assert disc_fused.supported(torch.zeros(1, 1, 30, dtype=torch.bfloat16), H.Discriminator2D(3))
