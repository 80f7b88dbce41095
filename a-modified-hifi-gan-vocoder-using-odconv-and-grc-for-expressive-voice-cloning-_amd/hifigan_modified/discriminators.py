"""Multi-period / multi-scale discriminators on MI355X.

Drop-in for the reference's ``hifigan_modified/discriminators.py``: MultiPeriodDiscriminator :12-28,
MultiScaleDiscriminator :30-46, Discriminator2D :48-84 (zero right-pad + ``view(B,C,period,T//period)``
fold, 5x Conv2d 3x3), Discriminator1D :86-117 (AvgPool1d + 5x Conv1d k15), HiFiGANDiscriminators :119-151.

fp32 operands (fp32 storage only; host state like the generator's set_mixed_precision, no parameters or buffers):
``"exact"`` (the default) runs the generic fp32 kernels; ``"split"`` runs the channels-last MFMA stack with every operand
split into hi + lo bf16 and three products per MAC (disc_fused.py, ~2^-16 relative).
"""
from __future__ import annotations

import weakref
from typing import List

import torch
import torch.nn as nn

from . import functional as Fn

_CH = (1, 32, 64, 128, 256, 1)
FP32_OPERAND_MODES = ("exact", "split")


class _Fp32Operands:
    """`set_fp32_operands(mode)` / `fp32_operands` of every discriminator module: the mode is set on the module and on all the
    discriminator modules inside it."""
    _fp32_operands = "exact"

    @property
    def fp32_operands(self) -> str:
        return self._fp32_operands

    def set_fp32_operands(self, mode: str):
        if mode not in FP32_OPERAND_MODES:
            raise ValueError(f"fp32 operand mode must be one of {FP32_OPERAND_MODES}, got {mode!r}")
        for m in self.modules():
            if isinstance(m, _Fp32Operands):
                m._fp32_operands = mode
        return self


class DiscFeatures(list):
    """The four hidden feature maps `features()` returned, with the module, input shape and dtype they belong to."""

    def __init__(self, feats, owner, shape, dtype):
        super().__init__(feats)
        self.owner, self.shape, self.dtype = weakref.ref(owner), tuple(shape), dtype


class _FeatureMatching:
    """`features(x)` / `forward_fm(x, real_feats)` of one sub-discriminator (HiFi-GAN's feature-matching term over the hidden maps,
    defined by this build: DESIGN.md section 5b); `_fn` is functional.disc2d / disc1d."""

    def features(self, x: torch.Tensor):
        """Under no_grad: (out, feats) with feats = [a_1..a_4], a_l = hidden conv l after its LeakyReLU(0.1), logical shape
        [B,C,H,W] (2D) / [B,C,W] (1D), channels 32, 64, 128, 256."""
        out, feats = self._fn(x, self, "features")
        return out, DiscFeatures(feats, self, x.shape, x.dtype)

    def forward_fm(self, x: torch.Tensor, real_feats):
        """(out, fm): forward(x) and fm = sum_l mean|a_l(x) - real_l| (fp32, 0-dim) with real_feats = features(real)[1] of THIS
        module at the same input shape and dtype, taken as constants."""
        if not isinstance(real_feats, DiscFeatures) or real_feats.owner() is not self:
            raise ValueError("forward_fm: real_feats must be what features() of this very module returned")
        if real_feats.shape != tuple(x.shape) or real_feats.dtype != x.dtype:
            raise ValueError(f"forward_fm: real_feats were taken at {real_feats.shape} {real_feats.dtype}, x is {tuple(x.shape)} {x.dtype}")
        return self._fn(x, self, "fm", real_feats)


class _FeatureMatchingList:
    """List-valued `features` / `forward_fm` over `self.discriminators`."""

    def features(self, x: torch.Tensor):
        return [d.features(x) for d in self.discriminators]

    def forward_fm(self, x: torch.Tensor, real_feats):
        """real_feats: one features()[1] per sub-discriminator (or the (out, feats) pairs features() returned)."""
        if len(real_feats) != len(self.discriminators):
            raise ValueError(f"forward_fm: {len(self.discriminators)} feature lists expected, got {len(real_feats)}")
        return [d.forward_fm(x, r[1] if isinstance(r, tuple) else r) for d, r in zip(self.discriminators, real_feats)]


class Discriminator2D(_FeatureMatching, _Fp32Operands, nn.Module):
    _fn = staticmethod(Fn.disc2d)

    def __init__(self, period: int):
        super().__init__()
        self.period = period
        layers = []
        for i in range(5):
            layers.append(nn.Conv2d(_CH[i], _CH[i + 1], (3, 3), padding=(1, 1)))
            if i < 4:
                layers.append(nn.LeakyReLU(0.1))
        self.conv_layers = nn.Sequential(*layers)  # convs at 0,2,4,6,8 like the reference

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return Fn.disc2d(x, self)


class Discriminator1D(_FeatureMatching, _Fp32Operands, nn.Module):
    _fn = staticmethod(Fn.disc1d)

    def __init__(self, scale: int):
        super().__init__()
        self.scale = scale
        self.downsample = nn.AvgPool1d(scale, stride=scale)
        layers = []
        for i in range(5):
            layers.append(nn.Conv1d(_CH[i], _CH[i + 1], 15, padding=7))
            if i < 4:
                layers.append(nn.LeakyReLU(0.1))
        self.conv_layers = nn.Sequential(*layers)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return Fn.disc1d(x, self)


class MultiPeriodDiscriminator(_FeatureMatchingList, _Fp32Operands, nn.Module):
    def __init__(self, periods: List[int] = [2, 3, 5, 7, 11]):
        super().__init__()
        self.periods = periods
        self.discriminators = nn.ModuleList([Discriminator2D(p) for p in periods])

    def forward(self, x: torch.Tensor) -> List[torch.Tensor]:
        return [d(x) for d in self.discriminators]


class MultiScaleDiscriminator(_FeatureMatchingList, _Fp32Operands, nn.Module):
    def __init__(self, scales: List[int] = [1, 2, 4]):
        super().__init__()
        self.scales = scales
        self.discriminators = nn.ModuleList([Discriminator1D(s) for s in scales])

    def forward(self, x: torch.Tensor) -> List[torch.Tensor]:
        return [d(x) for d in self.discriminators]


class HiFiGANDiscriminators(_Fp32Operands, nn.Module):
    def __init__(self):
        super().__init__()
        self.mpd = MultiPeriodDiscriminator()
        self.msd = MultiScaleDiscriminator()

    def forward(self, real_audio: torch.Tensor, fake_audio: torch.Tensor) -> dict:
        # discriminator step (no gradient flows into either waveform): real and fake ride through every sub-discriminator as
        # ONE batch of 2B - half the launches, twice the grid per launch - and the outputs are split again.  Every op is
        # per-sample, so the values are those of the two separate passes of discriminators.py:127-151.
        if (real_audio.shape == fake_audio.shape and real_audio.dtype == fake_audio.dtype and real_audio.is_cuda
                and torch.is_grad_enabled() and not real_audio.requires_grad and not fake_audio.requires_grad):
            both = Fn.batch_cat(real_audio, fake_audio)
            B = real_audio.shape[0]
            mpd, msd = [Fn.batch_split(o) for o in self.mpd(both)], [Fn.batch_split(o) for o in self.msd(both)]
            return {"mpd_real": [r for r, _ in mpd], "mpd_fake": [f for _, f in mpd],
                    "msd_real": [r for r, _ in msd], "msd_fake": [f for _, f in msd]}
        return {
            "mpd_real": self.mpd(real_audio),
            "mpd_fake": self.mpd(fake_audio),
            "msd_real": self.msd(real_audio),
            "msd_fake": self.msd(fake_audio),
        }
