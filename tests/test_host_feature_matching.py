"""Feature matching over the discriminators' hidden feature maps (fm_mode="features"), host side: the switch, the state_dict, the
C-ABI entries and the fake (meta) kernels of the two new operators."""
import ctypes

import pytest
import torch

_CH = (1, 32, 64, 128, 256, 1)


def test_fm_mode_default_and_setter():
    import hifigan_modified as H
    voc = H.ModifiedHiFiGANVocoder(hidden_channels=64, upsample_factors=[4, 2])
    assert voc.fm_mode == "output"
    assert voc.set_feature_matching("features") is voc and voc.fm_mode == "features"
    assert voc.set_feature_matching("output").fm_mode == "output"
    for bad in ("hidden", "", None, "Features", 1):
        with pytest.raises(ValueError):
            voc.set_feature_matching(bad)
    assert voc.fm_mode == "output"
    assert H.ModifiedHiFiGANVocoder(hidden_channels=64, upsample_factors=[4, 2]).fm_mode == "output"   # not shared through the class


def test_state_dict_keys_unchanged():
    """No new parameters or buffers: the discriminators' keys are the reference's (8 stacks x 5 convs x weight/bias), the vocoder's do
    not change with the mode, and nothing in either names the switch."""
    import hifigan_modified as H
    d = H.HiFiGANDiscriminators()
    expect = [f"{fam}.discriminators.{i}.conv_layers.{c}.{p}" for fam, n in (("mpd", 5), ("msd", 3)) for i in range(n)
              for c in (0, 2, 4, 6, 8) for p in ("weight", "bias")]
    assert list(d.state_dict().keys()) == expect and len(list(d.buffers())) == 0
    voc = H.ModifiedHiFiGANVocoder(hidden_channels=64, upsample_factors=[4, 2])
    keys, nbuf = list(voc.state_dict().keys()), len(list(voc.buffers()))
    voc.set_feature_matching("features")
    assert list(voc.state_dict().keys()) == keys and len(list(voc.buffers())) == nbuf
    assert [k for k in keys if k.startswith("discriminators.")] == ["discriminators." + k for k in expect]
    assert not any("fm" in k.split(".")[-1] for k in keys)


def test_entries_declared_and_exported():
    from hifigan_modified import _native
    decl = _native.declared_symbols()
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name, nargs in (("mv_fm_l1", 7), ("mv_fm_inject", 9)):
        assert name in decl and len(decl[name][1]) == nargs, name
        assert hasattr(lib, name), name


@pytest.mark.parametrize("shape,k", [((2, 1, 3, 40), (3, 3)), ((2, 1, 50), (15,))])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fake_kernels_on_meta(shape, k, dtype):
    import hifigan_modified  # noqa: F401
    from hifigan_modified import torch_ops  # noqa: F401
    ns = torch.ops.mi355x_vocoder
    params = []
    for i in range(5):
        params += [torch.empty(_CH[i + 1], _CH[i], *k, device="meta"), torch.empty(_CH[i + 1], device="meta")]
    x = torch.empty(*shape, device="meta", dtype=dtype)
    out, feats = ns.disc_conv_stack_features(x, 0.1, *params)
    assert out.shape == x.shape and out.dtype == dtype and len(feats) == 4
    for f, c in zip(feats, _CH[1:5]):
        assert tuple(f.shape) == (shape[0], c) + tuple(shape[2:]) and f.dtype == dtype
        cl = f.permute(0, 2, 3, 1) if f.dim() == 4 else f.permute(0, 2, 1)
        assert cl.is_contiguous()                      # a view of the channels-last buffer
    out, fm = ns.disc_conv_stack_fm(x, 0.1, *feats, *params)
    assert out.shape == x.shape and out.dtype == dtype
    assert fm.shape == () and fm.dtype == torch.float32


def test_forward_fm_refuses_foreign_features():
    """forward_fm takes only what features() of the same module returned, at the same input shape and dtype (checked before any kernel)."""
    import hifigan_modified as H
    from hifigan_modified.discriminators import DiscFeatures
    a, b = H.Discriminator2D(3), H.Discriminator2D(3)
    x = torch.zeros(2, 1, 30)
    plain = [torch.zeros(2, c, 3, 10) for c in _CH[1:5]]
    with pytest.raises(ValueError):
        a.forward_fm(x, plain)
    with pytest.raises(ValueError):
        a.forward_fm(x, DiscFeatures(plain, b, x.shape, x.dtype))
    with pytest.raises(ValueError):
        a.forward_fm(x, DiscFeatures(plain, a, (2, 1, 60), x.dtype))
    with pytest.raises(ValueError):
        a.forward_fm(x, DiscFeatures(plain, a, x.shape, torch.bfloat16))
    with pytest.raises(ValueError):
        H.MultiPeriodDiscriminator().forward_fm(x, [plain])
