"""Wave -> mel front end and clip sampler (the step before the path).

The reference ships no vocoder dataset code; its only mel parameters are ``speaker_embedding/ecapa_tdnn.py:163-170``
(n_fft 1024, hop 256, win 1024, 80 mels) and ``configs/eval_config.yaml:23-29`` (fmin 0, fmax 8000).  The front end here
is the same HIP framing + DFT + mel kernel the mel/STFT loss uses (``mv_mel_loss`` with ``want_mel``), so training targets
and the loss agree bit for bit, and no CPU librosa stage sits in front of the GPU.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import functional as Fn
from .mel import mel_filterbank


class MelFrontEnd:
    """log-mel [B, n_mels, T // hop] (fp32) of waveforms [B, 1, T] on the GPU."""

    def __init__(self, sample_rate=22050, n_fft=1024, hop=256, n_mels=80, fmin=0.0, fmax=8000.0, clamp=1e-5, device="cuda"):
        self.n_fft, self.hop, self.clamp = n_fft, hop, clamp
        self.fb = mel_filterbank(sample_rate, n_fft, n_mels, fmin, fmax, device=device)

    def __call__(self, wave: torch.Tensor) -> torch.Tensor:
        if wave.dim() == 2:
            wave = wave.unsqueeze(1)
        return Fn.mel_spectrogram(wave, self.fb, self.n_fft, self.hop, self.clamp)


class ClipSampler:
    """Random fixed-length training clips from a list of utterances (1-D waveforms of any length, host or device memory):
    ``sample(B)`` -> (wave [B,1,clip], mel [B,n_mels,clip//hop]).  Each rank seeds its own generator
    (seed + rank: data-parallel ranks draw different clips); short utterances are zero-padded on the right."""

    def __init__(self, utterances, clip_samples=8192, front_end: MelFrontEnd | None = None, seed=0, rank=0, device="cuda",
                 dtype=torch.float32):
        if not utterances:
            raise ValueError("ClipSampler needs at least one utterance")
        self.utts = [u.reshape(-1) for u in utterances]
        self.clip = int(clip_samples)
        self.fe = front_end
        self.device, self.dtype = device, dtype
        self.gen = torch.Generator().manual_seed(int(seed) + int(rank))

    def draw(self, batch):
        """host-side index draw: [(utterance index, start sample)] - deterministic per (seed, rank)."""
        picks = []
        for _ in range(batch):
            i = int(torch.randint(len(self.utts), (1,), generator=self.gen))
            n = self.utts[i].numel()
            s = int(torch.randint(max(n - self.clip, 0) + 1, (1,), generator=self.gen))
            picks.append((i, s))
        return picks

    def sample(self, batch):
        wave = torch.zeros(batch, 1, self.clip, device=self.device, dtype=torch.float32)
        for r, (i, s) in enumerate(self.draw(batch)):
            seg = self.utts[i][s:s + self.clip]
            wave[r, 0, :seg.numel()] = seg.to(self.device, torch.float32)
        mel = self.fe(wave) if self.fe is not None else None
        return wave.to(self.dtype), mel


# ---------------------------------------------------------------------------------------------- device-side sampler
# One record of mv_clip_gather's table (include/mi355x_vocoder.h; csrc/clip_sampler.hip ClipDesc), 48 bytes.
CLIP_DESC = np.dtype([("src_off", "<i8"), ("src_len", "<i8"), ("pos_q32", "<i8"), ("rate_q32", "<i8"),
                      ("gain", "<f4"), ("noise_std", "<f4"), ("noise_ctr", "<i8")])
assert CLIP_DESC.itemsize == 48
_Q32 = 1 << 32


def resample_table(Z=16, P=256, beta=9.0, rolloff=0.945) -> torch.Tensor:
    """fp32 [Z*P + 1]: one wing of the resampler's low-pass prototype, a Kaiser-windowed sinc
    h(t) = rolloff sinc(rolloff t) I0(beta sqrt(1 - (t/Z)^2)) / I0(beta), sampled at t = k/P for k = 0 .. Z*P (t in source samples at
    rates <= 1; mv_clip_gather stretches it by the rate above 1).  Computed in float64."""
    if Z < 1 or P < 1:
        raise ValueError(f"resample_table: Z and P must be positive, got {Z}, {P}")
    t = np.arange(Z * P + 1, dtype=np.float64) / P
    win = np.i0(beta * np.sqrt(np.maximum(1.0 - (t / Z) ** 2, 0.0))) / np.i0(beta)
    return torch.from_numpy((rolloff * np.sinc(rolloff * t) * win).astype(np.float32))


class DeviceClipSampler:
    """ClipSampler with the corpus resident on the device and the whole batch cut in one HIP launch (mv_clip_gather), with the
    augmentation the reference's training configuration asks for (``configs/train_config.yaml:81-85``: pitch_shift, time_stretch,
    noise_level).  ``sample(B)`` -> (wave [B,1,clip] in `dtype`, mel = front_end(wave)): one host-to-device copy of the B x 48-byte
    record table, one kernel launch, then the mel front end.  With no augmentation and fp32 storage it returns ClipSampler's bits
    for the same seed.

    What the augmentation is: ONE windowed-sinc resampling by a factor `rate` per clip, which moves pitch and tempo together -
    speed perturbation.  The preset of `reference_augmentation()` is +-2 semitones, i.e. about -11 % / +12 % in duration, and so
    covers both reference ranges jointly; independent pitch shift and time stretch (a phase vocoder) are not built.  On top of it a
    gain (uniform in dB) and white Gaussian noise of standard deviation `noise_level`, drawn on the device from Philox4x32-10.

    storage "pcm16" keeps the corpus as 16-bit PCM (half the memory; fp32 utterances are quantised as
    clamp(round(x * 32768), -32768, 32767), int16 utterances are stored raw).  `draw(B)` is host only and returns the records
    (CLIP_DESC): clip picks come from torch.Generator(seed + rank) with exactly ClipSampler.draw's call sequence, the start being
    drawn from max(n - need, 0) + 1 with need = ceil(clip * rate); the augmentation parameters come from a second generator, before
    the picks of each clip.  noise_ctr is a running clip counter, so no two clips of a run share a noise stream."""

    def __init__(self, utterances, clip_samples=8192, front_end: MelFrontEnd | None = None, seed=0, rank=0, device="cuda",
                 dtype=torch.float32, storage="fp32", rate_range=None, gain_db_range=None, noise_level=0.0, p_augment=1.0):
        if not utterances:
            raise ValueError("DeviceClipSampler needs at least one utterance")
        if storage not in ("fp32", "pcm16"):
            raise ValueError(f"DeviceClipSampler: storage must be 'fp32' or 'pcm16', got {storage!r}")
        if rate_range is not None and not 0.5 <= rate_range[0] <= rate_range[1] <= 2.0:
            raise ValueError(f"DeviceClipSampler: rate_range must lie in [0.5, 2], got {rate_range}")
        if not 0.0 <= p_augment <= 1.0 or noise_level < 0:
            raise ValueError("DeviceClipSampler: p_augment must lie in [0, 1] and noise_level must not be negative")
        self.clip = int(clip_samples)
        self.fe = front_end
        self.device, self.dtype, self.storage = device, dtype, storage
        self.rate_range = None if rate_range is None else (float(rate_range[0]), float(rate_range[1]))
        self.gain_db_range = None if gain_db_range is None else (float(gain_db_range[0]), float(gain_db_range[1]))
        self.noise_level, self.p_augment = float(noise_level), float(p_augment)
        self.augments = self.rate_range is not None or self.gain_db_range is not None or self.noise_level > 0
        self.key = int(seed) + int(rank)
        self.gen = torch.Generator().manual_seed(self.key)
        self.aug_gen = torch.Generator().manual_seed(self.key + 0x9E3779B9)
        self.counter = 0
        parts, self.lengths, self.offsets = [], [], []
        for u in utterances:
            u = u.reshape(-1)
            if storage == "pcm16":
                if u.dtype != torch.int16:
                    u = torch.clamp(torch.round(u.to(torch.float32) * 32768.0), -32768, 32767).to(torch.int16)
            else:
                u = u.to(torch.float32) * (1.0 / 32768.0) if u.dtype == torch.int16 else u.to(torch.float32)
            self.offsets.append(sum(self.lengths))
            self.lengths.append(u.numel())
            parts.append(u.to(device))
        self.arena = torch.cat(parts)                    # every utterance back to back, on the device
        self.Z, self.P = 16, 256
        self.table = resample_table(self.Z, self.P).to(device)

    @staticmethod
    def reference_augmentation():
        """The reference's ranges (configs/train_config.yaml:81-85: pitch_shift [-2, 2] semitones, time_stretch [0.9, 1.1],
        noise_level 0.01) as this sampler's arguments: one speed factor in [2^(-2/12), 2^(2/12)] = [0.891, 1.122]."""
        return dict(rate_range=(2 ** (-2 / 12), 2 ** (2 / 12)), noise_level=0.01)

    def draw(self, batch):
        """host-side draw of one batch's records (numpy, CLIP_DESC) - deterministic per (seed, rank)."""
        rec = np.zeros(batch, dtype=CLIP_DESC)
        for r in range(batch):
            rate_q, gain, noise = _Q32, 1.0, 0.0
            if self.augments:
                u = torch.rand(3, generator=self.aug_gen, dtype=torch.float64).tolist()     # always three: the stream does not depend on the outcome
                if u[0] < self.p_augment:
                    if self.rate_range is not None:
                        lo, hi = math.log(self.rate_range[0]), math.log(self.rate_range[1])
                        rate_q = min(max(int(round(math.exp(lo + u[1] * (hi - lo)) * _Q32)), _Q32 // 2), 2 * _Q32)
                    if self.gain_db_range is not None:
                        gain = 10.0 ** ((self.gain_db_range[0] + u[2] * (self.gain_db_range[1] - self.gain_db_range[0])) / 20.0)
                    noise = self.noise_level
            need = (self.clip * rate_q + _Q32 - 1) >> 32                       # ceil(clip * rate) source samples
            i = int(torch.randint(len(self.lengths), (1,), generator=self.gen))
            n = self.lengths[i]
            s = int(torch.randint(max(n - need, 0) + 1, (1,), generator=self.gen))
            rec[r] = (self.offsets[i], n, s << 32, rate_q, gain, noise, self.counter)
            self.counter += 1
        return rec

    def picks(self, rec):
        """[(utterance index, start sample)] of records, ClipSampler.draw's form."""
        return [(self.offsets.index(int(o)), int(p) >> 32) for o, p in zip(rec["src_off"], rec["pos_q32"])]

    def gather(self, rec):
        """records -> wave [B,1,clip] in `dtype`: one host-to-device copy, one launch."""
        from . import ops
        descs = torch.from_numpy(rec.view(np.int64).reshape(len(rec), 6)).to(self.device)
        return ops.clip_gather(self.arena, descs, self.table, self.Z, self.P, self.clip, self.key, self.dtype)

    def sample(self, batch):
        wave = self.gather(self.draw(batch))
        mel = self.fe(wave) if self.fe is not None else None
        return wave, mel

    def state_dict(self):
        return {"gen": self.gen.get_state(), "aug_gen": self.aug_gen.get_state(), "counter": self.counter}

    def load_state_dict(self, sd):
        self.gen.set_state(sd["gen"])
        self.aug_gen.set_state(sd["aug_gen"])
        self.counter = int(sd["counter"])
