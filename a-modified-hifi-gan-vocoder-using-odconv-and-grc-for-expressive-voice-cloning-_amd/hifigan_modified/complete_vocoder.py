"""Complete vocoder system + two-optimizer trainer on MI355X.

Drop-in for the reference's ``hifigan_modified/complete_vocoder.py``: ``ModifiedHiFiGANVocoder`` (:21-184: generator +
discriminators, LSGAN + output-L1 "feature matching" + mel-L1 losses, weights 10 / 45) and ``VocoderTrainer``
(:186-248: G forward once -> D step on the detached fake -> G step with the discriminators re-evaluated).

Differences, all documented in DESIGN.md: the generator is the one ``conditioned_hifigan`` is written against (SURVEY.md
§A; the reference's current-source generator does not construct); the embedding extractor (``embedding_extractors.py``)
runs frozen (eval statistics, no gradient) with its one broken layer resized, see that module; the mel term is a real log-mel/STFT L1
(``mel_mode="stft"``) instead of the reference's ``generated_mel = mel`` placeholder (``mel_mode="placeholder"``
reproduces that: the term is then identically zero); `fm_mode="features"` (opt-in) extends the reference's
output-only "feature matching" L1 to every hidden feature map of every sub-discriminator, HiFi-GAN's definition of the term;
`set_stft_loss` (opt-in) adds a multi-resolution STFT loss of the fake against the real waveform to the generator's total.
"""
from __future__ import annotations

import contextlib
import os
from typing import Dict, Optional

import torch
import torch.nn as nn

from . import functional as Fn
from . import ops
from .discriminators import HiFiGANDiscriminators
from .embedding_extractors import EmbeddingExtractor
from .generator import ModifiedHiFiGANGenerator
from .mel import mel_filterbank


FM_MODES = ("output", "features")
STFT_DEFAULT_RESOLUTIONS = ops.STFT_DEFAULT_RESOLUTIONS     # ((512, 128), (1024, 256), (2048, 512)): (n_fft, hop)


class ModifiedHiFiGANVocoder(nn.Module):
    fm_mode = "output"          # host state, not a parameter or buffer: set_feature_matching; the trainer's checkpoint stores it
    stft_resolutions = None     # host state like fm_mode: set_stft_loss; None = the term is off
    stft_weight = 1.0           # untuned

    def __init__(self, input_channels: int = 80, hidden_channels: int = 512,
                 speaker_embedding_dim: int = 192, emotion_embedding_dim: int = 256,
                 sample_rate: int = 22050, n_fft: int = 1024, hop: Optional[int] = None, **generator_kwargs):
        super().__init__()
        self.generator = ModifiedHiFiGANGenerator(mel_channels=input_channels, hidden_channels=hidden_channels,
                                                  speaker_embedding_dim=speaker_embedding_dim,
                                                  emotion_embedding_dim=emotion_embedding_dim, **generator_kwargs)
        self.discriminators = HiFiGANDiscriminators()
        self.embedding_extractor = EmbeddingExtractor(speaker_embedding_dim=speaker_embedding_dim,
                                                      emotion_embedding_dim=emotion_embedding_dim)     # complete_vocoder.py:39-42
        self.fm_weight = 10.0
        self.mel_weight = 45.0
        hop_total = 1
        for f in self.generator.upsample_factors:
            hop_total *= f
        self.n_fft, self.hop = n_fft, hop or hop_total
        self.register_buffer("mel_fb", mel_filterbank(sample_rate, n_fft, input_channels), persistent=False)

    def forward(self, mel_spectrogram, speaker_embedding=None, emotion_embedding=None,
                extract_embeddings: bool = True) -> Dict[str, torch.Tensor]:
        if extract_embeddings and (speaker_embedding is None or emotion_embedding is None):     # complete_vocoder.py:65-69
            spk, emo = self.embedding_extractor(mel_spectrogram)
            speaker_embedding = spk if speaker_embedding is None else speaker_embedding
            emotion_embedding = emo if emotion_embedding is None else emotion_embedding
        wave = self.generator(mel_spectrogram, speaker_embedding, emotion_embedding)
        return {"generated_waveform": wave, "speaker_embedding": speaker_embedding, "emotion_embedding": emotion_embedding}

    def set_feature_matching(self, mode: str):
        """"output" (the default): the reference's term, L1 between the discriminators' final outputs (complete_vocoder.py:118,127).
        "features": per sub-discriminator that L1 plus sum_l mean|a_l(fake) - a_l(real).detach()| over its four hidden feature maps
        (a_l: hidden conv l after its LeakyReLU; each mean over all elements of the map, the MPD fold's zero padding included)."""
        if mode not in FM_MODES:
            raise ValueError(f"feature-matching mode must be one of {FM_MODES}, got {mode!r}")
        self.fm_mode = mode
        return self

    def set_stft_loss(self, resolutions=STFT_DEFAULT_RESOLUTIONS, weight: float = 1.0):
        """Multi-resolution STFT loss in the generator's total (Yamamoto et al. 2020; off by default, `resolutions=None` turns it
        off again): `stft_loss` = the mean over the (n_fft, hop) resolutions of spectral convergence + log-magnitude L1 of
        `fake_audio` against `real_audio` (a constant), with the mel term's framing; the total gains weight * stft_loss.  The
        default weight 1.0 is untuned.  The definition and what is supported: mv_stft_loss in the header; ValueError names a
        resolution that is not."""
        if resolutions is None:
            self.stft_resolutions = None
        else:
            self.stft_resolutions = ops.stft_resolutions(resolutions)
        self.stft_weight = float(weight)
        return self

    @property
    def stft_config(self):
        """None when the term is off, else {"resolutions": [[n_fft, hop], ...], "weight": w} (plain lists: what a checkpoint stores)."""
        if self.stft_resolutions is None:
            return None
        return {"resolutions": [list(r) for r in self.stft_resolutions], "weight": self.stft_weight}

    def get_discriminator_outputs(self, real_audio, fake_audio):
        return self.discriminators(real_audio, fake_audio)

    def log_mel(self, audio):
        """log-mel [B, n_mels, T/hop] of a waveform (HIP STFT kernel)."""
        return Fn.mel_spectrogram(audio, self.mel_fb, self.n_fft, self.hop)

    # ---- losses (complete_vocoder.py:89-184)
    def compute_generator_losses(self, real_audio, fake_audio, mel_spectrogram, generated_mel=None):
        """generated_mel tensor -> L1(generated_mel, mel_spectrogram) like the reference; None -> the mel of
        `fake_audio` is taken by the STFT kernel and compared with `mel_spectrogram` (a log-mel target)."""
        D = self.discriminators
        if self.fm_mode == "features":
            # the real pass keeps its hidden maps (no gradient), the fake pass adds their L1 per stack (forward_fm)
            mpd_real, msd_real = D.mpd.features(real_audio), D.msd.features(real_audio)
            mpd_pairs = D.mpd.forward_fm(fake_audio, mpd_real)
            msd_pairs = D.msd.forward_fm(fake_audio, msd_real)
            mpd_fake, msd_fake = [o for o, _ in mpd_pairs], [o for o, _ in msd_pairs]
            mpd_fm = sum(Fn.l1(f, r) + h for (r, _), (f, h) in zip(mpd_real, mpd_pairs))
            msd_fm = sum(Fn.l1(f, r) + h for (r, _), (f, h) in zip(msd_real, msd_pairs))
        else:
            with torch.no_grad():               # D(real) only enters through .detach() (complete_vocoder.py:118,123)
                mpd_real, msd_real = D.mpd(real_audio), D.msd(real_audio)
            mpd_fake, msd_fake = D.mpd(fake_audio), D.msd(fake_audio)
            mpd_fm = sum(Fn.l1(f, r) for r, f in zip(mpd_real, mpd_fake))
            msd_fm = sum(Fn.l1(f, r) for r, f in zip(msd_real, msd_fake))
        mpd_loss = sum(Fn.mse_const(f, 1.0) for f in mpd_fake)
        msd_loss = sum(Fn.mse_const(f, 1.0) for f in msd_fake)
        if generated_mel is None:
            mel_loss = Fn.mel_l1(fake_audio, mel_spectrogram, self.mel_fb, self.n_fft, self.hop)
        else:
            mel_loss = Fn.l1(generated_mel, mel_spectrogram)
        total = mpd_loss + msd_loss + self.fm_weight * (mpd_fm + msd_fm) + self.mel_weight * mel_loss
        losses = {"total_loss": total, "mpd_loss": mpd_loss, "msd_loss": msd_loss, "mpd_fm_loss": mpd_fm,
                  "msd_fm_loss": msd_fm, "mel_loss": mel_loss}
        if self.stft_resolutions is not None:
            losses["stft_loss"] = Fn.mr_stft_loss(fake_audio, real_audio, self.stft_resolutions)
            losses["total_loss"] = total + self.stft_weight * losses["stft_loss"]
        return losses

    def compute_discriminator_losses(self, real_audio, fake_audio):
        out = self.discriminators(real_audio, fake_audio)
        mpd_real = sum(Fn.mse_const(o, 1.0) for o in out["mpd_real"])
        mpd_fake = sum(Fn.mse_const(o, 0.0) for o in out["mpd_fake"])
        msd_real = sum(Fn.mse_const(o, 1.0) for o in out["msd_real"])
        msd_fake = sum(Fn.mse_const(o, 0.0) for o in out["msd_fake"])
        return {"total_loss": mpd_real + mpd_fake + msd_real + msd_fake, "mpd_real_loss": mpd_real,
                "mpd_fake_loss": mpd_fake, "msd_real_loss": msd_real, "msd_fake_loss": msd_fake}


class VocoderTrainer:
    """complete_vocoder.py:186-248.  Optimizers: anything with zero_grad()/step(); `FlatAdamW` (optim.py) is the native
    one and is what `default_optimizers` builds (lr 2e-4, betas (0.8, 0.99), wd 1e-4: configs/train_config.yaml:54-72).

    Data parallel (one process per GPU, torch.distributed initialised): `grad_sync="overlap"` (the default when the world
    size is > 1) reduces each optimizer's gradient buckets UNDER its backward (parallel.OverlappedGradSync); a
    `parallel.GradSynchronizer` instance reduces the flat buffer after the backward instead; `grad_sync=False` never reduces.
    `train_step` returns host floats like the reference (:229-233); `return_tensors=True` keeps device tensors and skips the
    device synchronisation a `.item()` costs.

    `dropout_rng="counter"` (the default with `use_graph`) draws the MRF dropout masks from a counter-based stream
    (functional.DropoutRNG, key from torch's CPU generator at construction): a captured step then draws fresh masks at every replay,
    the same ones the eager step would.  `"torch"` (the default otherwise) draws each mask's key from torch's CPU generator as
    before - under capture those keys are frozen into the graph.  `schedulers`: lr schedules (e.g. optim.WarmupCosineLR), stepped
    after every train_step, eager or replayed.  The dropout stream and the schedules are saved in the checkpoint.

    fp32 training with the discriminators on the matrix cores: `vocoder.discriminators.set_fp32_operands("split")` with fp32
    activations runs both discriminator families on split-operand MFMA kernels (every operand hi + lo bf16, ~2^-16 relative) instead
    of the generic fp32 kernels (the default "exact"); 16-bit activations are not affected.

    `accumulation_steps=N` (configs/train_config.yaml: gradient_accumulation_steps): a window is N consecutive `train_step` calls.
    Every call runs the full forward / backward in the reference's order and adds its gradients to both optimizers' flat buffers
    (zeroed by a kernel at the window's start); both optimizers step only on the window's last call, on the window's sum times 1/N.
    The weights are constant inside a window, so the generator pass of every micro-step sees the discriminators of the window's
    START (in the reference's single step it sees them just updated): the ordinary meaning of accumulation for a two-optimizer step.
    The dropout stream advances on every call, the schedulers and the optimizers' step counts once per window; under data parallel
    only the last call of a window reduces.  `max_grad_norm=x` (configs/incremental_train_config.yaml): each optimizer's gradient
    - averaged over the window and over the ranks - is clipped to global L2 norm x before its update, like
    torch.nn.utils.clip_grad_norm_ on that optimizer's parameters; the norm and the coefficient stay on the device
    (`optimizer.grad_norm`; with `return_tensors=True` the stepping call also returns `generator_grad_norm` /
    `discriminator_grad_norm`), and a captured step follows `optimizer.max_grad_norm` at every replay.  Both need FlatAdamW
    optimizers.  With `use_graph` a window replays two graphs per input signature: "accumulate" and "accumulate + step".
    `save_checkpoint` inside a window raises; `load_checkpoint` starts a new window.

    `ema_decay=d` (None, the default: no average, no launch, no checkpoint key): `trainer.ema` (optim.ArenaEMA) keeps the exponential
    moving average of the generator's arena, updated by one streaming launch right after every generator update - once per optimizer
    step, so once per accumulation window, eager or captured (the captured step reads this step's decay from the optimizer's state
    block); `ema_warmup` ramps the decay as min(d, (1 + n) / (10 + n)).  Needs a FlatAdamW generator optimizer.  Under data parallel
    every rank averages its own (identical) weights.  `with trainer.ema_weights():` runs its body with the averaged weights in the
    generator (an exchange on entry, the same exchange on exit; no train_step inside), `evaluate(..., weights="ema" | "live")` is a
    no-grad validation pass, and the checkpoint gains `ema_state` and `ema_generator_state_dict` (a complete generator state_dict
    with the averaged weights: what inference loads).

    `vocoder.set_stft_loss(...)` (off by default): the step's result, `evaluate()` and the checkpoint gain `stft_loss` only while the
    term is on, and a captured step records one graph per configuration of it."""

    def __init__(self, vocoder: ModifiedHiFiGANVocoder, generator_optimizer=None, discriminator_optimizer=None,
                 device=None, mel_mode: str = "stft", grad_sync=None, bucket_mib: int = 8, use_graph: bool = False,
                 graph_warmup: int = 2, dropout_rng: Optional[str] = None, schedulers=(), accumulation_steps: int = 1,
                 max_grad_norm: Optional[float] = None, ema_decay: Optional[float] = None, ema_warmup: bool = True):
        from .training import GradWindow
        self.window = w = GradWindow("VocoderTrainer", accumulation_steps, max_grad_norm, grad_sync, bucket_mib)
        self.accumulation_steps, self.max_grad_norm = w.accumulation_steps, w.max_grad_norm
        self.grad_sync, self.bucket_mib, self._overlap = w.grad_sync, w.bucket_mib, w.overlap
        device = device or torch.device("cuda")
        self.vocoder = vocoder.to(device)
        self.device = device
        if generator_optimizer is None or discriminator_optimizer is None:
            generator_optimizer, discriminator_optimizer = self.default_optimizers(self.vocoder)
        self.generator_optimizer = generator_optimizer
        self.discriminator_optimizer = discriminator_optimizer
        w.adopt(generator_optimizer, discriminator_optimizer)
        self.mel_mode = mel_mode
        self._d_params = list(self.vocoder.discriminators.parameters())
        # use_graph: after `graph_warmup` eager steps at a given input signature the whole step (G forward, D step, G step, both
        # AdamW launches, every weight re-pack) is captured into ONE HIP graph and replayed: the step is ~1000 launches, more than
        # half of them shorter than the ~5 us it takes to issue one (single process, FlatAdamW optimizers only; static shapes)
        self.use_graph = use_graph
        self.graph_warmup = graph_warmup
        self._graphs = {}                    # (input signature[, phase]) -> the captured step's state (_graph_step)
        self._gstream = None                 # the side stream of warm-up, capture and replay (created with the first captured step)
        self.last_losses = None              # (generator, discriminator) loss dicts of the last eager step
        dropout_rng = dropout_rng or ("counter" if use_graph else "torch")
        if dropout_rng not in ("torch", "counter"):
            raise ValueError(f"VocoderTrainer: dropout_rng must be 'torch' or 'counter', got {dropout_rng!r}")
        self.dropout_rng = Fn.DropoutRNG.from_torch() if dropout_rng == "counter" else None
        self.schedulers = tuple(s for s in schedulers if s is not None)
        self.ema = None
        self._ema_swapped = False            # inside `with ema_weights()`: the arena holds the average, the shadow the live weights
        if ema_decay is not None:
            from .optim import ArenaEMA, FlatAdamW
            if not isinstance(generator_optimizer, FlatAdamW):
                raise ValueError("VocoderTrainer: ema_decay averages FlatAdamW's parameter arena; the generator optimizer is a "
                                 f"{type(generator_optimizer).__name__}")
            self.ema = ArenaEMA(generator_optimizer, ema_decay, warmup=ema_warmup)

    @staticmethod
    def default_optimizers(vocoder, lr=2e-4, betas=(0.8, 0.99), weight_decay=1e-4):
        from .optim import FlatAdamW
        g = FlatAdamW(vocoder.generator.parameters(), lr=lr, betas=betas, weight_decay=weight_decay,
                      exclude=list(vocoder.generator.unused_parameters()))
        d = FlatAdamW(vocoder.discriminators.parameters(), lr=lr, betas=betas, weight_decay=weight_decay)
        return g, d

    @property
    def _micro(self):
        return self.window.position

    def overlap_sync(self, opt):
        """The OverlappedGradSync of a FlatAdamW optimizer (created on first use), or None when overlap is off."""
        return self.window.overlap_sync(opt)

    def _apply_step(self, opt, scale):
        """The (clipped) FlatAdamW update, then the stepped module's conv packs."""
        self.window.apply(opt, scale)
        if not torch.cuda.is_current_stream_capturing():
            from . import disc_fused
            disc_fused._packs.refresh_owned(opt)     # all conv packs of the stepped module in one launch
        # (captured step: each pack is recorded where the next forward misses its cache - the batched refresh would upload a new
        #  pointer table from pageable memory, which a capture does not allow)

    def train_step(self, mel_spectrogram, real_audio, speaker_embedding=None, emotion_embedding=None,
                   return_tensors: bool = False) -> Dict[str, float]:
        if self._ema_swapped:
            raise RuntimeError("VocoderTrainer.train_step inside `with ema_weights()`: the generator holds the averaged weights")
        mel_spectrogram = mel_spectrogram.to(self.device)
        real_audio = real_audio.to(self.device)
        # (a new window: both arenas start from zero, every micro-step adds)
        do_step = self.window.begin_call((self.discriminator_optimizer, self.generator_optimizer))
        if self.use_graph and self._graph_ok():
            res = self._graph_step(mel_spectrogram, real_audio, speaker_embedding, emotion_embedding, do_step)
        else:
            res = self._step(mel_spectrogram, real_audio, speaker_embedding, emotion_embedding, do_step)
        self.window.end_call()
        if do_step:
            for sch in self.schedulers:
                sch.step()
        if not return_tensors:
            return self.to_floats(res)             # complete_vocoder.py:229-233 returns .item() floats
        if do_step and self.max_grad_norm is not None:
            res = dict(res, generator_grad_norm=self.generator_optimizer.grad_norm,
                       discriminator_grad_norm=self.discriminator_optimizer.grad_norm)
        return res

    def _step(self, mel_spectrogram, real_audio, speaker_embedding, emotion_embedding, do_step=True):
        """One step under the trainer's dropout stream; an eager step advances the stream by the masks it drew (a captured one leaves
        that to each replay)."""
        rng = self.dropout_rng
        if rng is None:
            return self._step_body(mel_spectrogram, real_audio, speaker_embedding, emotion_embedding, do_step)
        rng.slots_used = 0
        with Fn.use_dropout_rng(rng):
            out = self._step_body(mel_spectrogram, real_audio, speaker_embedding, emotion_embedding, do_step)
        if not torch.cuda.is_current_stream_capturing():
            rng.advance()
        return out

    def _step_body(self, mel_spectrogram, real_audio, speaker_embedding, emotion_embedding, do_step=True):
        """One step in the reference's order (complete_vocoder.py:207-226); returns device tensors.  do_step=False (a micro-step
        inside an accumulation window): the same passes, the gradients only accumulate."""
        out = self.vocoder(mel_spectrogram, speaker_embedding, emotion_embedding)
        fake_audio = out["generated_waveform"]
        # discriminator step on the detached fake
        self.discriminator_optimizer.zero_grad()
        d_losses = self.vocoder.compute_discriminator_losses(real_audio, fake_audio.detach())
        # (inside an accumulation window the weights are constant: the discriminators' update waits until the generator's gradients
        #  of the window's last micro-step exist too)
        defer = self.accumulation_steps > 1
        d_scale = self.window.backward(d_losses["total_loss"], self.discriminator_optimizer, do_step)   # complete_vocoder.py:217-218
        if d_scale is not None and not defer:
            self._apply_step(self.discriminator_optimizer, d_scale)
        # generator step: discriminators re-evaluated after their update; their own weight gradients are not needed
        # (the reference accumulates and then zeroes them at the next D step)
        self.generator_optimizer.zero_grad()
        for p in self._d_params:
            p.requires_grad_(False)
        try:
            if self.mel_mode == "stft":
                target = self.vocoder.log_mel(real_audio)
                g_losses = self.vocoder.compute_generator_losses(real_audio, fake_audio, target, None)
            else:   # the reference's placeholder: generated_mel = mel_spectrogram -> the term is zero
                g_losses = self.vocoder.compute_generator_losses(real_audio, fake_audio, mel_spectrogram, mel_spectrogram)
            g_scale = self.window.backward(g_losses["total_loss"], self.generator_optimizer, do_step)       # :225-226
            if g_scale is not None:
                if defer:
                    self._apply_step(self.discriminator_optimizer, d_scale)
                self._apply_step(self.generator_optimizer, g_scale)
                if self.ema is not None:
                    self.ema.update()          # once per optimizer step: only the call that steps reaches this line
        finally:
            for p in self._d_params:
                p.requires_grad_(True)
        self.last_losses = (g_losses, d_losses)
        res = {"generator_loss": g_losses["total_loss"], "discriminator_loss": d_losses["total_loss"],
               "mel_loss": g_losses["mel_loss"]}
        if "stft_loss" in g_losses:
            res["stft_loss"] = g_losses["stft_loss"]
        return res

    # ---- captured step
    def _graph_ok(self):
        from .optim import FlatAdamW
        import torch.distributed as dist
        single = not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)
        return single and not self.grad_sync and isinstance(self.generator_optimizer, FlatAdamW) and \
            isinstance(self.discriminator_optimizer, FlatAdamW)

    def _graph_step(self, mel, real, spk, emo, do_step=True):
        sig = tuple((tuple(t.shape), t.dtype) if t is not None else None for t in (mel, real, spk, emo))
        # one graph per (input signature, phase); with accumulation the phases are "accumulate" and "accumulate + step", each with its
        # own warm-up steps; the optimizers' state (runs, state block, step counts) belongs to the stepping phase only
        key = sig if self.accumulation_steps == 1 else sig + ("step" if do_step else "accumulate",)
        if self.vocoder.fm_mode != "output":
            key = key + (("fm", self.vocoder.fm_mode),)    # a mode change after a capture records its own graph
        if self.vocoder.stft_resolutions is not None:      # (likewise: the resolutions and the weight are baked into the launches)
            key = key + (("stft", self.vocoder.stft_resolutions, self.vocoder.stft_weight),)
        st = self._graphs.get(key)
        if st is None:
            st = self._graphs[key] = {"warm": 0, "graph": None}
        # warm-up steps and the capture share ONE side stream: autograd pins every parameter's AccumulateGrad node to the stream it
        # was first used on, and a node pinned to the default stream would pull the capture back onto it (and invalidate it)
        if self._gstream is None:
            self._gstream = torch.cuda.Stream()
        if st["graph"] is None and st["warm"] < self.graph_warmup:
            return self._graph_warm(st, (mel, real, spk, emo), do_step)
        gopt, dopt = self.generator_optimizer, self.discriminator_optimizer
        if st["graph"] is not None and do_step and not (gopt.runs_match(st["gstate"]) and dopt.runs_match(st["dstate"])):
            # a restored optimizer state split or merged the runs of equal step count that this graph updates: recapture
            torch.cuda.synchronize()              # (its last replay may still be running on the pool it frees)
            st["graph"] = st["out"] = st["gstate"] = st["dstate"] = None
        if st["graph"] is None:
            self._graph_capture(st, (mel, real, spk, emo), do_step)
        return self._graph_replay(st, (mel, real, spk, emo), do_step)

    def _graph_warm(self, st, inputs, do_step):
        """One eager step on the side stream: packs weights, sets launch attributes, sizes every cache."""
        st["warm"] += 1
        gs = self._gstream
        gs.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(gs):
            out = self._step(*inputs, do_step)
        torch.cuda.current_stream().wait_stream(gs)
        return out

    def _graph_capture(self, st, inputs, do_step):
        """Record one step on static copies of `inputs` into st["graph"]; st["gstate"] / st["dstate"]: what the optimizers need to
        replay it.  A configuration that cannot be captured turns use_graph off and raises."""
        gopt, dopt, rng = self.generator_optimizer, self.discriminator_optimizer, self.dropout_rng
        st["inputs"] = [None if t is None else t.to(self.device).clone() for t in inputs]
        self.last_losses = None               # (loss tensors keep last step's autograd graph alive)
        # every cached cast / packed weight must MISS inside the capture: a hit bakes the pointer of a buffer that the replays never
        # rewrite (the 16-bit discriminator heads: packed after the warm-up step's update, read again - stale - by every replay's
        # discriminator step; D loss 1.2 % off from the second replay on), a miss records the pack kernel itself
        from . import ops as _ops
        _ops.bump_param_epoch()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        if os.environ.get("MV_GRAPH_DOT"):
            graph.enable_debug_mode()
        gopt.capture_begin(stepping=do_step)
        dopt.capture_begin(stepping=do_step)
        if rng is not None:
            rng.device_block(self.device)     # allocated before the capture: the graph keeps its address
        try:
            with torch.cuda.graph(graph, stream=self._gstream):
                st["out"] = self._step(*st["inputs"], do_step)
            st["gstate"], st["dstate"] = gopt.capture_end(), dopt.capture_end()
            st["dropout_slots"] = rng.slots_used if rng is not None else 0
        except Exception:
            gopt._capture = dopt._capture = None
            self.use_graph = False            # this configuration cannot be captured: stay eager (and say so once)
            raise
        st["graph"] = graph
        if os.environ.get("MV_GRAPH_DOT"):
            graph.debug_dump(os.environ["MV_GRAPH_DOT"])

    def _graph_replay(self, st, inputs, do_step):
        gopt, dopt, rng, gs = self.generator_optimizer, self.discriminator_optimizer, self.dropout_rng, self._gstream
        for dst, src in zip(st["inputs"], inputs):
            if dst is not None:
                dst.copy_(src)
        # replayed on the trainer's own stream, fenced against the caller's: on this ROCm build a ~1000-node graph replayed on a stream
        # that also carries other eager training work between replays went wrong from its second replay on (MSD gradients, then NaN) -
        # with the other work on a different stream, or nothing in between, it does not (tests/test_gpu_train_graph.py interleaves
        # an eager trainer with a captured one)
        cur = torch.cuda.current_stream()
        gs.wait_stream(cur)
        with torch.cuda.stream(gs):
            # the host's per-step state (step counts + 1, lr and the other AdamW inputs, the dropout stream's counter) -> the state
            # blocks the graph reads, on the replay's stream: a few hundred bytes, asynchronously
            if do_step:
                dopt.before_replay(st["dstate"])
                gopt.before_replay(st["gstate"])
            if rng is not None:
                rng.upload()
            st["graph"].replay()
        cur.wait_stream(gs)
        if do_step:
            dopt.after_replay(st["dstate"])
            gopt.after_replay(st["gstate"])
        if rng is not None:
            rng.advance(st["dropout_slots"])
        return st["out"]

    @staticmethod
    def to_floats(losses):
        """Host read-back of a loss dict (one device synchronisation)."""
        return {k: float(v.detach()) if torch.is_tensor(v) else float(v) for k, v in losses.items()}

    # ---- the averaged generator
    @contextlib.contextmanager
    def ema_weights(self):
        """Run the body with the averaged weights in the generator: one exchange of the arena and the average on entry, the same
        exchange on exit (also when the body raises), which restores both bit for bit."""
        if self.ema is None:
            raise RuntimeError("VocoderTrainer.ema_weights: this trainer keeps no EMA (ema_decay=None)")
        if self._ema_swapped:
            raise RuntimeError("VocoderTrainer.ema_weights: already inside the block")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("VocoderTrainer.ema_weights: the exchange is not part of a captured graph")
        self.ema.swap()
        self._ema_swapped = True
        try:
            yield self
        finally:
            self.ema.swap()
            self._ema_swapped = False

    def evaluate(self, mel_spectrogram, real_audio, speaker_embedding=None, emotion_embedding=None, weights: str = "ema"):
        """One validation pass (train_config.yaml: eval_steps): the vocoder's forward in eval mode under no_grad, with the averaged
        ("ema") or the live generator weights; returns {"mel_loss": mel L1 of the generated waveform against the log-mel of
        `real_audio`} as a host float, and next to it "stft_loss" while that term is on.  Leaves the modules' training flags as they were and touches neither the dropout stream nor
        the accumulation window, the optimizers or the schedules."""
        if weights not in ("ema", "live"):
            raise ValueError(f"VocoderTrainer.evaluate: weights must be 'ema' or 'live', got {weights!r}")
        if weights == "ema" and self.ema is None:
            raise RuntimeError("VocoderTrainer.evaluate: weights='ema' on a trainer that keeps no EMA (ema_decay=None)")
        voc = self.vocoder
        mel_spectrogram, real_audio = mel_spectrogram.to(self.device), real_audio.to(self.device)
        modes = [(m, m.training) for m in voc.modules()]
        voc.train(False)
        try:
            with torch.no_grad(), (self.ema_weights() if weights == "ema" else contextlib.nullcontext()):
                wave = voc(mel_spectrogram, speaker_embedding, emotion_embedding)["generated_waveform"]
                loss = Fn.mel_l1(wave, voc.log_mel(real_audio), voc.mel_fb, voc.n_fft, voc.hop)
                stft = None if voc.stft_resolutions is None else Fn.mr_stft_loss(wave, real_audio, voc.stft_resolutions)
        finally:
            for m, flag in modes:
                m.training = flag
        return {"mel_loss": float(loss)} if stft is None else {"mel_loss": float(loss), "stft_loss": float(stft)}

    def ema_generator_state_dict(self):
        """A complete generator state_dict with the arena parameters at their averaged values, every other entry live."""
        if self._ema_swapped:
            raise RuntimeError("VocoderTrainer: inside `with ema_weights()` the arena and the average are exchanged")
        gen = self.vocoder.generator
        sd = {k: v.detach().clone() for k, v in gen.state_dict().items()}
        for name, view in self.ema.named_tensors(gen):
            sd[name] = view.clone()
        return sd

    def save_checkpoint(self, path: str):
        self.window.assert_boundary("VocoderTrainer.save_checkpoint")
        if self._ema_swapped:
            raise RuntimeError("VocoderTrainer.save_checkpoint inside `with ema_weights()`: the generator holds the averaged weights")
        ck = {"vocoder_state_dict": self.vocoder.state_dict(),
              # torch.optim.AdamW's layout, so the reference's own load path (complete_vocoder.py:463-468) reads the file too
              "generator_optimizer_state_dict": self.generator_optimizer.torch_state_dict(),
              "discriminator_optimizer_state_dict": self.discriminator_optimizer.torch_state_dict()}
        # extra keys (the reference's load path ignores them): the dropout stream and the lr schedules
        if self.dropout_rng is not None:
            ck["dropout_rng_state"] = self.dropout_rng.state_dict()
        if self.schedulers:
            ck["scheduler_state_dicts"] = [s.state_dict() for s in self.schedulers]
        if self.vocoder.fm_mode != "output":             # (a default trainer's file keeps the reference's keys)
            ck["fm_mode"] = self.vocoder.fm_mode
        if self.vocoder.stft_config is not None:
            ck["stft_loss"] = self.vocoder.stft_config
        ck.update(self.window.checkpoint_extras())
        if self.ema is not None:
            ck["ema_state"] = self.ema.state_dict()
            ck["ema_generator_state_dict"] = self.ema_generator_state_dict()
        torch.save(ck, path)

    def load_checkpoint(self, path: str):
        if self._ema_swapped:
            raise RuntimeError("VocoderTrainer.load_checkpoint inside `with ema_weights()`")
        ck = torch.load(path, map_location=self.device, weights_only=True)
        self.vocoder.load_state_dict(ck["vocoder_state_dict"])
        self.generator_optimizer.load_state_dict(ck["generator_optimizer_state_dict"])
        self.discriminator_optimizer.load_state_dict(ck["discriminator_optimizer_state_dict"])
        if self.dropout_rng is not None and "dropout_rng_state" in ck:
            self.dropout_rng.load_state_dict(ck["dropout_rng_state"])
        for sch, sd in zip(self.schedulers, ck.get("scheduler_state_dicts", ())):
            sch.load_state_dict(sd)
        self.vocoder.set_feature_matching(ck.get("fm_mode", "output"))     # (no key: the reference's term)
        stft = ck.get("stft_loss")                                         # (no key: the term is off)
        self.vocoder.set_stft_loss(None) if stft is None else self.vocoder.set_stft_loss(stft["resolutions"], stft["weight"])
        self.window.reset()                  # a checkpoint is always a window boundary
        if self.ema is not None:             # (a file's EMA keys mean nothing to a trainer without one)
            if "ema_state" in ck:
                self.ema.load_state_dict(ck["ema_state"])
            else:                            # a file from a trainer without EMA: the average starts over from the loaded weights
                self.ema.reset()
