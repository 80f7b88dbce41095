"""ConditionedHiFiGAN + single-optimizer trainer on MI355X.

Drop-in for the reference's ``hifigan_modified/conditioned_hifigan.py``: ``ConditionedHiFiGAN`` (:23-208: generator +
MPD + MSD container, ``forward(mel, audio_clip, speaker_emb, emotion_emb)``, ``get_model_info``, ``save_model`` /
``load_model``) and ``HiFiGANTrainer`` (:210-299: one AdamW over generator AND discriminators, loss = 45 L1(fake, real)
+ 45 MSE(mel(fake), mel) + hinge(MPD) + hinge(MSD)).

The reference's speaker / emotion encoders are external models that are disabled upstream (``speaker_encoder = None``,
:69-75) and substitute ``torch.randn`` embeddings (:111-113): here embeddings must be passed explicitly; asking for
extraction from an audio clip raises.  Two upstream defects are replaced by their evident intent:
``compute_mel_spectrogram`` returns noise (:269-274) -> the STFT kernel; ``compute_adversarial_loss`` is handed a list
(:241,257) -> hinge applied per sub-discriminator and summed.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import functional as Fn
from .generator import HiFiGANGenerator
from .mel import mel_filterbank


class ConditionedHiFiGAN(nn.Module):
    def __init__(self, mel_channels=80, speaker_embedding_dim=192, emotion_embedding_dim=384, hidden_channels=512,
                 kernel_size=7, upsample_factors=[8, 8, 2, 2], resblock_kernel_sizes=[3, 7, 11],
                 resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], groups=4, lora_rank=16, dropout=0.1,
                 device="cuda"):
        super().__init__()
        self.device = device
        self.mel_channels = mel_channels
        self.speaker_embedding_dim, self.emotion_embedding_dim = speaker_embedding_dim, emotion_embedding_dim
        self.generator = HiFiGANGenerator(mel_channels=mel_channels, hidden_channels=hidden_channels,
                                          kernel_size=kernel_size, upsample_factors=upsample_factors,
                                          resblock_kernel_sizes=resblock_kernel_sizes,
                                          resblock_dilation_sizes=resblock_dilation_sizes, groups=groups,
                                          lora_rank=lora_rank, dropout=dropout)
        self.speaker_encoder = None
        self.emotion_encoder = None
        self.sample_rate = 16000
        self.training_config = {
            "mel_channels": mel_channels, "speaker_embedding_dim": speaker_embedding_dim,
            "emotion_embedding_dim": emotion_embedding_dim, "hidden_channels": hidden_channels,
            "kernel_size": kernel_size, "upsample_factors": upsample_factors,
            "resblock_kernel_sizes": resblock_kernel_sizes, "resblock_dilation_sizes": resblock_dilation_sizes,
            "groups": groups, "lora_rank": lora_rank, "dropout": dropout,
        }

    def extract_speaker_embedding(self, audio_clip):
        raise RuntimeError("speaker encoder (ECAPA-TDNN, external) is out of scope: pass speaker_emb explicitly "
                           "(the reference returns torch.randn here, conditioned_hifigan.py:111-113)")

    def extract_emotion_embedding(self, audio_clip):
        raise RuntimeError("emotion encoder (Emotion2Vec, external) is out of scope: pass emotion_emb explicitly "
                           "(the reference returns torch.randn here, conditioned_hifigan.py:131-133)")

    def forward(self, mel, audio_clip=None, speaker_emb=None, emotion_emb=None):
        if speaker_emb is None and audio_clip is not None:
            speaker_emb = self.extract_speaker_embedding(audio_clip)
        if emotion_emb is None and audio_clip is not None:
            emotion_emb = self.extract_emotion_embedding(audio_clip)
        return self.generator(mel, speaker_emb, emotion_emb)

    def get_discriminator_outputs(self, real_audio, fake_audio):
        return self.generator.get_discriminator_outputs(real_audio, fake_audio)

    def get_model_info(self):
        total = sum(p.numel() for p in self.parameters())
        trainable = sum(p.numel() for p in self.parameters() if p.requires_grad)
        return {"total_parameters": total, "trainable_parameters": trainable,
                "architecture": "Enhanced HiFi-GAN with ODconv + GRC+LoRA",
                "conditioning": "FiLM with ECAPA-TDNN + Emotion2Vec", "config": self.training_config}

    def save_model(self, path):
        torch.save({"model_state_dict": self.state_dict(), "config": self.training_config,
                    "model_info": self.get_model_info()}, path)

    def load_model(self, path):
        ck = torch.load(path, map_location=self.device, weights_only=True)
        self.load_state_dict(ck["model_state_dict"])
        return ck.get("config", {}), ck.get("model_info", {})


class HiFiGANTrainer:
    """conditioned_hifigan.py:210-299.  One optimizer over G + MPD + MSD (`FlatAdamW`, lr 2e-4, torch AdamW defaults).

    `accumulation_steps=N`: a window is N consecutive `train_step` calls; each adds its gradients to the optimizer's flat buffer
    (zeroed by a kernel at the window's start) and the last one steps on the sum times 1/N (and, data parallel, is the only one
    that reduces).  `max_grad_norm=x`: the averaged gradient is clipped to global L2 norm x before the update
    (torch.nn.utils.clip_grad_norm_ semantics, on the device: `optimizer.grad_norm`).  `save_checkpoint` inside a window raises."""

    def __init__(self, model, learning_rate=2e-4, device="cuda", sample_rate=22050, n_fft=1024, grad_sync=None, bucket_mib=8,
                 accumulation_steps=1, max_grad_norm=None):
        from .optim import FlatAdamW
        from .training import GradWindow
        self.window = w = GradWindow("HiFiGANTrainer", accumulation_steps, max_grad_norm, grad_sync, bucket_mib)
        self.accumulation_steps, self.max_grad_norm = w.accumulation_steps, w.max_grad_norm
        self.grad_sync, self._overlap = w.grad_sync, w.overlap     # (data parallel by default when torch.distributed is up)
        self.model = model
        self.device = device
        g = model.generator.generator
        self.optimizer = FlatAdamW(model.parameters(), lr=learning_rate, exclude=list(g.unused_parameters()))
        w.adopt(self.optimizer)
        hop = 1
        for f in g.upsample_factors:
            hop *= f
        self.n_fft, self.hop = n_fft, hop
        self.mel_fb = mel_filterbank(sample_rate, n_fft, model.mel_channels, device=next(model.parameters()).device)

    def compute_mel_spectrogram(self, audio):
        return Fn.mel_spectrogram(audio, self.mel_fb, self.n_fft, self.hop)

    def compute_adversarial_loss(self, disc_outputs, target_is_real):
        """hinge, per sub-discriminator, summed (conditioned_hifigan.py:262-265)."""
        fn = Fn.hinge_g if target_is_real else Fn.hinge_d_fake
        if isinstance(disc_outputs, (list, tuple)):
            return sum(fn(o) for o in disc_outputs)
        return fn(disc_outputs)

    def compute_losses(self, real_audio, fake_audio, mel_input):
        gen = self.model.generator
        mpd_fake, msd_fake = gen.mpd(fake_audio), gen.msd(fake_audio)
        losses = {
            "feature_loss": Fn.l1(fake_audio, real_audio),
            "mel_loss": self._mel_mse(fake_audio, mel_input),
            "mpd_loss": self.compute_adversarial_loss(mpd_fake, True),
            "msd_loss": self.compute_adversarial_loss(msd_fake, True),
        }
        total = (losses["feature_loss"] * 45.0 + losses["mel_loss"] * 45.0 + losses["mpd_loss"] * 1.0
                 + losses["msd_loss"] * 1.0)
        return total, losses

    def _mel_mse(self, fake_audio, mel_input):
        """MSE(log-mel(fake), mel_input) through the differentiable STFT kernel (conditioned_hifigan.py:237-238)."""
        return Fn.mel_mse(fake_audio, mel_input, self.mel_fb, self.n_fft, self.hop)

    @property
    def _micro(self):
        return self.window.position

    def train_step(self, mel_input, real_audio, speaker_emb=None, emotion_emb=None):
        do_step = self.window.begin_call((self.optimizer,))     # a new window: the arena starts from zero, every micro-step adds
        self.optimizer.zero_grad()
        fake_audio = self.model(mel_input, speaker_emb=speaker_emb, emotion_emb=emotion_emb)
        total, breakdown = self.compute_losses(real_audio, fake_audio, mel_input)
        scale = self.window.backward(total, self.optimizer, do_step)
        self.window.end_call()
        if scale is not None:
            self.window.apply(self.optimizer, scale)
        return total.item(), breakdown

    def save_checkpoint(self, path, epoch, loss):
        self.window.assert_boundary("HiFiGANTrainer.save_checkpoint")
        ck = {"epoch": epoch, "model_state_dict": self.model.state_dict(),
              "optimizer_state_dict": self.optimizer.torch_state_dict(), "loss": loss}   # torch.optim.AdamW's layout
        ck.update(self.window.checkpoint_extras())      # informational; a default trainer's keys are unchanged
        torch.save(ck, path)
