"""Shared numerics helpers of the off-unit-scale tests (a plain module, imported like tests/embed_cases.py): CPU emulations of the
16-bit side formats, a simulation of each inference mode's own roundings (tools/error_budget.py), and constructions that move a
seeded default-init generator to where a trained one operates - a head whose pre-tanh signal is centred and unsaturated, GroupNorm
inputs whose group mean is a multiple of their std, a mel with log-mel statistics.  Everything here runs on the CPU."""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import error_budget as EB                    # noqa: E402
from oracle import vocoder_oracle as O       # noqa: E402


# ------------------------------------------------------------------------------------------------ format round trips
def hl8(t):
    """csrc/mfma.h hl8 row: f16 hi + e4m3 byte of (v - hi) * 2048, clamped to +-448."""
    return EB.q(t.float(), "hl8")


def pair(t):
    """Pair row / two-product operand: f16 hi + f16 lo."""
    return EB.q(t.float(), "fp16x2")


def bf16xN(t, n):
    """Split bf16 operand with n pieces (n = 3: the fp32 mode's operands)."""
    return EB.q(t.float(), f"bf16x{n}")


# ------------------------------------------------------------------------------------------------ inference modes
MODES = ("fp32", "mixed_up0", "mixed_up1", "headline", "fp16", "bf16")
_EARLY = ["mel", "input_proj", "up0", "up1", "up2", "up3"]


def mode_tables(mode):
    """(act, wgt, cmode, kwargs) of tools/error_budget.forward for one inference mode of ModifiedHiFiGANGenerator:
    fp32       fp32 storage, three bf16 pieces per MFMA operand everywhere
    mixed_upN  fp16 storage and operands through upN, fp32 storage with three-piece operands behind
    headline   set_mixed_precision("up1", mrf_weights="fp16"): fp16 through up1; hi + lo bf16 operands in up2, up3 and the output
               conv; the MRF chain with f16 hi + lo activation operands x single-f16 weights and hl8 rows after mrf0 and mrf1
    fp16/bf16  16-bit storage and operands everywhere, the waveform included."""
    act = {s: "fp32" for s in EB.STAGES}
    wgt = {l: "fp32" for l in EB.LAYERS}
    kw = {}
    if mode in ("fp16", "bf16"):
        act = {s: mode for s in EB.STAGES}
        wgt = {l: mode for l in EB.LAYERS}
        return act, wgt, [mode] * 3, kw
    split = "bf16x3"
    act = {s: split for s in EB.STAGES}
    wgt = {l: split for l in EB.LAYERS}
    act["wave"] = "fp32"
    cm = [split] * 3
    if mode == "fp32":
        return act, wgt, cm, kw
    n_early = {"mixed_up0": 3, "mixed_up1": 4, "headline": 4}[mode]
    for s in _EARLY[:n_early]:
        act[s] = "fp16"
    for l in EB.LAYERS[:n_early - 1]:
        wgt[l] = "fp16"
    if mode == "headline":
        act.update(up2="bf16x2", up3="fp32", mrf0="hl8", mrf1="hl8", mrf2="bf16x2")
        wgt.update(up2="bf16x2", up3="bf16x2", mrf0="fp16", mrf1="fp16", mrf2="fp16", out="bf16x2")
        cm = ["fp16x2"] * 3
        kw = dict(opmode="fp16x2")
    return act, wgt, cm, kw


def simulate(mode, mel, sd, spk, emo):
    """The oracle's arithmetic in fp32 with the mode's roundings injected -> dict(wave, output_proj (pre-tanh), mrf0..mrf2)."""
    act, wgt, cm, kw = mode_tables(mode)
    st = {}
    with torch.no_grad():
        wave, pre = EB.forward(mel, sd, spk, emo, (8, 8, 2, 2), act, wgt, cm, stages=st, **kw)
    st["wave"], st["output_proj"] = wave, pre
    return st


def chain_sim(x, sds, n, mode, dilations=(1, 3, 5)):
    """n chained MultiReceptiveFieldBlocks (state dicts `sds`, x [B, 64, T] fp32) with the roundings of one MrfChain entry:
    three     forward_cl(x): three bf16 pieces per operand, fp32 rows between the blocks
    w16       forward_cl(x, w16=True): f16 hi + lo operands x single-f16 weights, hl8 rows between the blocks (x' and f)
    w16_pair  forward_cl(pair rows, w16=True, x_pair=True): the same with pair rows in, between the blocks and out
    w16_tile  forward_cl(x, w16=True) at dilations other than (1, 3, 5): the tile form of the same operands, fp32 rows throughout
    fp16/bf16 forward_cl(x in 16-bit storage): weights, operands, the concat and every stored row in that type (x is rounded first).
    dilations: one set for every block, or one set per block."""
    per_block = isinstance(dilations[0], (tuple, list))
    with torch.no_grad():
        if mode == "w16_pair":
            x = pair(x)
        elif mode in ("fp16", "bf16"):
            x = EB.q(x, mode)
        for i in range(n):
            last = i == n - 1
            dil = tuple(dilations[i]) if per_block else dilations
            if mode == "three":
                x = EB.mrf_forward(x, sds[i], "", dil, "bf16x3", "bf16x3", "fp32", opmode="bf16x3")
            elif mode == "w16":
                x = EB.mrf_forward(x, sds[i], "", dil, "fp16", "fp16x2", "fp32" if last else "hl8", opmode="fp16x2", fmode="hl8")
            elif mode == "w16_pair":
                x = EB.mrf_forward(x, sds[i], "", dil, "fp16", "fp16x2", "fp16x2", opmode="fp16x2")
            elif mode == "w16_tile":
                x = EB.mrf_forward(x, sds[i], "", dil, "fp16", "fp16x2", "fp32", opmode="fp16x2")
            elif mode in ("fp16", "bf16"):
                x = EB.mrf_forward(x, sds[i], "", dil, mode, mode, mode)
            else:
                raise ValueError(mode)
    return x


# ------------------------------------------------------------------------------------------------ operating points
def calibrate_head(sd, ref_pre_tanh, rms):
    """State dict whose output_proj is rescaled so that the oracle's pre-tanh signal on the clips that gave `ref_pre_tanh` has
    zero mean and the given rms: y' = s * (y - mean y), s = rms / std y."""
    y = ref_pre_tanh.double()
    mean = y.mean()
    s = rms / (y - mean).pow(2).mean().sqrt()
    out = dict(sd)
    out["output_proj.weight"] = (sd["output_proj.weight"].double() * s).to(sd["output_proj.weight"].dtype)
    out["output_proj.bias"] = ((sd["output_proj.bias"].double() - mean) * s).to(sd["output_proj.bias"].dtype)
    return out


def _gn_inputs(x, sd, prefix, dilations):
    """fp64: the GroupNorm inputs of one MRF block on x - [v_0, v_1, v_2] (each [B, 20, T]) and f [B, 64, T]."""
    sd = {k: v.double() for k, v in sd.items() if k.startswith(prefix)}
    x = x.double()
    vs, branches = [], []
    for j, d in enumerate(dilations):
        p = f"{prefix}conv_layers.{j}."
        Wc = sd[p + "conv.weight"]
        k = Wc.shape[2]
        h = F.conv1d(x, Wc, sd[p + "conv.bias"], padding=(k - 1) * d // 2, dilation=d, groups=x.shape[1] // Wc.shape[1])
        u = h + sd[p + "lora_scaling"] * torch.einsum("bct,co->bot", x, sd[p + "lora_A"] @ sd[p + "lora_B"])
        vs.append(F.conv1d(u, sd[p + "output_projection.weight"], sd[p + "output_projection.bias"]))
        branches.append(O.grc_lora_block(x, sd, p, d))
    f = F.conv1d(torch.cat(branches, 1), sd[prefix + "fusion.weight"], sd[prefix + "fusion.bias"])
    return vs, f


def group_ratio(t, groups):
    """mean / std per (sample, group) of a GroupNorm input [B, C, T] -> [B, groups]."""
    B, C, T = t.shape
    g = t.double().reshape(B, groups, -1)
    return g.mean(2) / g.var(2, unbiased=False).sqrt()


def offset_biases(sd, block, r, x, which, dilations=(1, 3, 5)):
    """State dict in which the biases in front of the GroupNorms of the MRF block with key prefix `block` are shifted so that, on the
    block input x [B, 64, T], the group mean of the GroupNorm input is r x the group std: which = "branch" shifts
    conv_layers.j.output_projection.bias (the three 20-channel GroupNorm inputs v: 5 groups of 4 channels), which = "fusion" shifts
    fusion.bias (the 64-channel GroupNorm input f: 8 groups of 8).  The shift comes from one fp64 oracle pass; a bias is shared by
    the batch, so the shift uses the batch means of the groups' mean and std.  The achieved ratio is checked on every (sample, group): within 20 % of r (of 1 for
    r < 1).  Returns (state dict, achieved ratios).  A constant added in front of a GroupNorm leaves the block's output as it was."""
    vs, f = _gn_inputs(x, sd, block, dilations)
    out = dict(sd)

    def shift(t, key):
        B, C, T = t.shape
        groups = O.norm_groups_for(C)
        g = t.reshape(B, groups, -1)
        delta = (r * g.var(2, unbiased=False).sqrt().mean(0) - g.mean(2).mean(0)).repeat_interleave(C // groups)
        out[key] = (sd[key].double() + delta).to(sd[key].dtype)
        ratio = group_ratio(t + (out[key].double() - sd[key].double()).view(1, C, 1), groups)
        assert float((ratio - r).abs().max()) <= 0.2 * max(r, 1.0), (key, r, ratio)
        return ratio

    if which == "branch":
        ratios = [shift(v, f"{block}conv_layers.{j}.output_projection.bias") for j, v in enumerate(vs)]
        return out, torch.stack(ratios)
    if which == "fusion":
        return out, shift(f, block + "fusion.bias")
    raise ValueError(which)


def logmel_like(B, T, seed=0):
    """Deterministic log-mel [B, 80, T]: a few harmonics of a gliding fundamental with a syllable-rate envelope plus noise, through
    oracle.mel_spectrogram - the statistics a vocoder sees (mean about -5, a strong per-channel offset), not randn's."""
    g = torch.Generator().manual_seed(seed)
    n = T * 256
    t = torch.arange(n, dtype=torch.float64) / 22050.0
    waves = []
    for b in range(B):
        f0 = 110.0 + 40.0 * b + 30.0 * torch.sin(2 * torch.pi * (1.5 + 0.5 * b) * t)
        ph = 2 * torch.pi * torch.cumsum(f0, 0) / 22050.0
        w = sum(a * torch.sin(h * ph) for h, a in ((1, 0.5), (2, 0.3), (3, 0.2), (5, 0.1), (8, 0.05)))
        env = 0.55 + 0.45 * torch.sin(2 * torch.pi * (3.0 + b) * t)
        waves.append(0.3 * env * w + 0.01 * torch.randn(n, generator=g, dtype=torch.float64))
    wave = torch.stack(waves)[:, None]
    return O.mel_spectrogram(wave).float().contiguous()


def mrf_blocks(seed=0, dilations=(1, 3, 5)):
    """Three seeded 64-channel MultiReceptiveFieldBlocks with non-trivial GroupNorm affines and biases, on the CPU, and their state
    dicts - the blocks of the chain tests (tests/test_gpu_mrf_stream.py, tests/test_gpu_inference_off_unit_scale.py)."""
    import hifigan_modified as H
    torch.manual_seed(seed)
    blks = [H.MultiReceptiveFieldBlock(64, 64, dilations=list(dilations)) for _ in range(3)]
    for bk in blks:
        for p in bk.parameters():
            if p.dim() == 1 and p.numel() in (20, 64):
                p.data.add_(0.3 * torch.randn_like(p))        # non-trivial GroupNorm affines and biases
    return blks, [{k: v.detach().clone() for k, v in bk.state_dict().items()} for bk in blks]


def default_generator_sd(seed=0):
    import hifigan_modified as H
    torch.manual_seed(seed)
    gen = H.ModifiedHiFiGANGenerator()
    return gen, {k: v.detach().clone() for k, v in gen.state_dict().items()}


def sharpen_attention(sd, factor=20.0):
    """Every ODConv's attention logits x factor (kernel_attention.1.weight; the bias is zero at init): alpha goes near one-hot."""
    out = dict(sd)
    for k in sd:
        if k.endswith("kernel_attention.1.weight"):
            out[k] = sd[k] * factor
    return out


# ------------------------------------------------------------------------------------------------ split-operand products
def bf16_split(t):
    """csrc/mfma.h Mma<float>::split: hi = bf16(v), lo = bf16(v - hi), both round-to-nearest; returned as float64."""
    hi = t.float().bfloat16().double()
    lo = (t.double() - hi).float().bfloat16().double()
    return hi, lo


def f16_split(t):
    """The streaming kernels' pieces: hi = f16(v), lo = f16(v - hi), round-to-nearest, f16 subnormals kept; as float64."""
    hi = t.float().half().double()
    lo = (t.double() - hi).float().half().double()
    return hi, lo


def split_product(bilinear, w, x, drop=(), split=None):
    """The fp32 storage mode's product of two split operands under a bilinear map (a convolution, a GEMM), in float64:
    bilinear(wh, xh) + bilinear(wh, xl) + bilinear(wl, xh); the lo * lo term is never formed.  `drop` names terms a faulty kernel
    loses ("hl": weight hi x activation lo, "lh": weight lo x activation hi); `split` = f16_split for the streaming kernels."""
    split = split or bf16_split
    wh, wl = split(w)
    xh, xl = split(x)
    terms = {"hh": (wh, xh), "hl": (wh, xl), "lh": (wl, xh)}
    return sum(bilinear(a, b) for k, (a, b) in terms.items() if k not in drop)
