"""Multi-resolution STFT loss, host side: the C-ABI entry and what it refuses before any launch, the switch on the vocoder, the
shape checks of ops.stft_loss, the operator's fake kernel and its refusing CPU kernel."""
import ctypes

import pytest
import torch

CFG = dict(hidden_channels=64, upsample_factors=[4, 2])
BAD = [
    [(48, 12)],                       # n_fft not a power of two
    [(16, 4)], [(4096, 1024)],        # out of [32, 2048]
    [(64, 128)],                      # hop > n_fft
    [(64, 15)],                       # n_fft - hop odd
    [(64, 0)],
    [],                               # no resolution
    [(64, 16)] * 9,                   # nine
]


def test_entry_declared_and_exported():
    from hifigan_modified import _native
    decl = _native.declared_symbols()
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert "mv_stft_loss" in decl and len(decl["mv_stft_loss"][1]) == 15
    assert hasattr(lib, "mv_stft_loss")


def _call(B, T, res, floor=1e-7, backward=0, gwave=True, dtype=0):
    """mv_stft_loss with dummy non-null pointers: only for argument sets it refuses, which it does before any launch."""
    from hifigan_modified import _native
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    ints = ctypes.c_int * max(len(res), 1)
    return _native.lib().mv_stft_loss(p, p, B, T, len(res), ints(*(n for n, _ in res)), ints(*(h for _, h in res)), floor, 1.0, p, p,
                                      p if gwave else None, backward, dtype, None)


@pytest.mark.parametrize("res", BAD)
def test_entry_refuses_unsupported_resolutions(res):
    assert _call(2, 256, res) == -1                              # MV_ERR_ARG


def test_entry_refuses_lengths_and_arguments():
    assert _call(2, 250, [(64, 16)]) == -1                       # T % hop
    assert _call(2, 16, [(64, 16)]) == -1                        # reflect pad 24 >= T
    assert _call(2, 512, [(2048, 512)]) == -1                    # reflect pad 768 >= T
    assert _call(0, 256, [(64, 16)]) == -1
    assert _call(2, 256, [(64, 16)], floor=0.0) == -1
    assert _call(2, 256, [(64, 16)], backward=1, gwave=False) == -1
    assert _call(2, 256, [(64, 16)], dtype=7) == -2              # MV_ERR_DTYPE


def test_switch_on_the_vocoder():
    import hifigan_modified as H
    from hifigan_modified.complete_vocoder import STFT_DEFAULT_RESOLUTIONS
    assert STFT_DEFAULT_RESOLUTIONS == ((512, 128), (1024, 256), (2048, 512))
    voc = H.ModifiedHiFiGANVocoder(**CFG)
    # off on a fresh vocoder: compute_generator_losses adds its seventh key only under `stft_resolutions is not None`
    assert voc.stft_resolutions is None and voc.stft_config is None
    keys, nbuf = list(voc.state_dict().keys()), len(list(voc.buffers()))
    assert voc.set_stft_loss() is voc
    assert voc.stft_resolutions == STFT_DEFAULT_RESOLUTIONS and voc.stft_weight == 1.0
    assert voc.stft_config == {"resolutions": [[512, 128], [1024, 256], [2048, 512]], "weight": 1.0}
    voc.set_stft_loss([[64, 16], (32, 8)], weight=0.5)
    assert voc.stft_resolutions == ((64, 16), (32, 8)) and voc.stft_weight == 0.5
    assert list(voc.state_dict().keys()) == keys and len(list(voc.buffers())) == nbuf     # host state only
    for bad in BAD:
        with pytest.raises(ValueError) as e:
            voc.set_stft_loss(bad)
        if bad and len(bad) <= 8:
            assert str(tuple(bad[0])) in str(e.value)              # the message names the resolution
    with pytest.raises(ValueError):
        voc.set_stft_loss([(64.5, 16)])
    assert voc.stft_resolutions == ((64, 16), (32, 8))                 # a refused call changes nothing
    assert voc.set_stft_loss(None).stft_resolutions is None
    assert H.ModifiedHiFiGANVocoder(**CFG).stft_resolutions is None    # not shared through the class


def test_ops_checks_before_any_launch():
    from hifigan_modified import ops
    x = torch.zeros(2, 1, 256)
    with pytest.raises(ValueError):
        ops.stft_loss(x, torch.zeros(2, 1, 128), [(64, 16)])
    with pytest.raises(ValueError):
        ops.stft_loss(x, torch.zeros(1, 1, 256), [(64, 16)])
    with pytest.raises(ValueError):
        ops.stft_loss(x.view(2, 256), x.view(2, 256), [(64, 16)])
    with pytest.raises(ValueError):
        ops.stft_loss(x, x.double(), [(64, 16)])
    with pytest.raises(ValueError) as e:
        ops.stft_loss(x, x, [(32, 8), (64, 24)])              # 256 % 24
    assert "(64, 24)" in str(e.value)
    with pytest.raises(ValueError) as e:
        ops.stft_loss(torch.zeros(1, 1, 16), torch.zeros(1, 1, 16), [(64, 16)])
    assert "(64, 16)" in str(e.value)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.stft_loss(x, x, [(64, 16)])                       # everything checks out, but the tensors are not on the GPU


def test_fake_kernel_and_cpu_refusal():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import hifigan_modified  # noqa: F401
    from hifigan_modified import torch_ops  # noqa: F401
    ns = torch.ops.mi355x_vocoder
    for dtype in (torch.float32, torch.bfloat16):
        with FakeTensorMode():
            x = torch.empty(2, 1, 256, dtype=dtype)
            out = ns.stft_loss(x, x.clone(), [64, 32], [16, 8], 1e-7, 1.0)
            assert out.shape == () and out.dtype == torch.float32
        m = torch.empty(2, 1, 256, device="meta", dtype=dtype)
        out = ns.stft_loss(m, m, [64, 32], [16, 8], 1e-7, 1.0)
        assert out.shape == () and out.dtype == torch.float32
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ns.stft_loss(torch.zeros(2, 1, 256), torch.zeros(2, 1, 256), [64], [16], 1e-7, 1.0)
