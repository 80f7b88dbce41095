"""Timing of one full training step (variant B: G fwd -> D step -> G step) at a given batch.
usage: bench_train.py [B] [mel frames] [fp32|bf16|fp16] [--graph] [--accum N] [--max-grad-norm X] [--fm MODE] [--ema DECAY] [--stft] [--steps K] [--warmup W]
--graph: the captured step (VocoderTrainer(use_graph=True)); --accum / --max-grad-norm: the trainer's accumulation_steps / max_grad_norm;
--fm output|features: the vocoder's feature-matching mode (set_feature_matching); --ema DECAY: the trainer's ema_decay (the generator's
weight EMA, one more streaming launch per optimizer step); --stft: the multi-resolution STFT loss at its default resolutions
(set_stft_loss).
The time is per train_step CALL (with --accum N an optimizer step is N calls); the last line is one JSON object."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "a-modified-hifi-gan-vocoder-using-odconv-and-grc-for-expressive-voice-cloning-_amd"))
import torch
import hifigan_modified as H

ap = argparse.ArgumentParser()
ap.add_argument("B", nargs="?", type=int, default=2)
ap.add_argument("Tm", nargs="?", type=int, default=32)
ap.add_argument("dtype", nargs="?", default="fp32", choices=["bf16", "fp16", "fp32"])
ap.add_argument("--graph", action="store_true")
ap.add_argument("--accum", type=int, default=1)
ap.add_argument("--max-grad-norm", type=float, default=None)
ap.add_argument("--fm", default="output", choices=["output", "features"])
ap.add_argument("--ema", type=float, default=None)
ap.add_argument("--stft", action="store_true")
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
a = ap.parse_args()
B, Tm = a.B, a.Tm
dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
torch.manual_seed(0)
voc = H.ModifiedHiFiGANVocoder().set_feature_matching(a.fm)
if a.stft:
    voc.set_stft_loss()
kw = {}
if a.graph:
    kw["use_graph"] = True
if a.accum != 1:
    kw["accumulation_steps"] = a.accum
if a.max_grad_norm is not None:
    kw["max_grad_norm"] = a.max_grad_norm
if a.ema is not None:
    kw["ema_decay"] = a.ema
tr = H.VocoderTrainer(voc, device=torch.device("cuda"), **kw)
mel = torch.randn(B, 80, Tm, device="cuda").to(dt)
real = torch.randn(B, 1, Tm * 256, device="cuda").clamp(-1, 1).to(dt)
spk, emo = torch.randn(B, 192, device="cuda").to(dt), torch.randn(B, 384, device="cuda").to(dt)
warm = a.warmup + (3 if a.graph else 0)          # a captured step: its eager warm-up steps and the capture come first
for i in range(warm * a.accum):
    out = tr.train_step(mel, real, spk, emo, return_tensors=True)
torch.cuda.synchronize()
print({k: float(v) for k, v in out.items()})
t0 = time.perf_counter()
n = a.steps * a.accum
for i in range(n):
    tr.train_step(mel, real, spk, emo, return_tensors=True)
torch.cuda.synchronize()
dtm = (time.perf_counter() - t0) / n
print(f"B={B} T={Tm*256} {dt}: {dtm*1e3:.1f} ms/step  -> {B*Tm*256/dtm:,.0f} samples/s")
print(json.dumps({"B": B, "samples": Tm * 256, "dtype": a.dtype, "graph": a.graph, "accum": a.accum, "max_grad_norm": a.max_grad_norm, "fm": a.fm, "ema": a.ema, "stft": a.stft,
                  "calls": n, "ms_per_step": round(dtm * 1e3, 3)}))
