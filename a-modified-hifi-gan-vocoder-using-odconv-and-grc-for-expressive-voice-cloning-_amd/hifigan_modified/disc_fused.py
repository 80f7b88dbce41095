"""Channels-last MFMA path of one discriminator stack (forward + backward): 16-bit storage, or fp32 storage in "split" mode.

One ``torch.autograd.Function`` runs all five layers of a Discriminator2D / Discriminator1D
(discriminators.py:56-66, :97-107): first layer (1 -> 32) and head (256 -> 1) as small dedicated kernels, the three
wide layers on MFMA (``mv_dconv_cl_fwd``), their data gradients with the same kernel on flipped weights (LeakyReLU'
fused in the epilogue) and their weight gradients with the transposed-LDS-read GEMM (``mv_dconv_wgrad_cl``).
fp32 storage runs here only when the module's `fp32_operands` is "split" (discriminators.py): the wide layers then use the
split-operand kernels (every operand hi + lo bf16, three products per MAC, fp32 accumulation, ~2^-16 relative); the first layer,
the head's weight gradient and the first layer's gradients use their fp32 VALU kernels, and the head's forward and data gradient
ride the wide conv zero-padded to 32 channels.  The default "exact" mode keeps the generic fp32 kernels (functional.disc2d / disc1d).
"""
from __future__ import annotations

from ctypes import c_void_p

import torch
from torch.autograd import Function

from . import _native as N
from . import ops

_P = lambda t: None if t is None else c_void_p(t.data_ptr())


class _PackCache(ops.DerivedCache):
    """Packed weights per (parameter, kind): the builders of the discriminator stacks' MFMA operand images."""

    def refresh_owned(self, opt):
        """After `opt.step()` (flat-arena AdamW): re-pack every plain conv pack whose fp32 master belongs to `opt` with ONE launch and
        mark the entries current - instead of one pack launch per layer and direction as the layers run."""
        import numpy as np
        ents = []
        for key, e in self.d.items():
            kind, p = key[1], e[0][0]()
            if (p is None or not isinstance(kind, tuple) or len(kind) != 2 or kind[0] not in (torch.bfloat16, torch.float16, torch.float32)
                    or p.dtype != torch.float32 or not p.is_contiguous() or not opt.owns(p)):
                continue
            w = _as4d(p)
            if w.shape[0] % 16 or w.shape[1] % 32:
                continue
            ents.append((key, p, e[2], kind, w.shape))
        if not ents:
            return 0
        sig = tuple((id(p), p.data_ptr(), buf.data_ptr()) for _, p, buf, _, _ in ents)
        hit = self.__dict__.setdefault("_mp", {}).get(id(opt))
        if hit is None or hit[0] != sig:
            d = np.zeros(len(ents), dtype=[("src", "u8"), ("dst", "u8"), ("cout", "i4"), ("cin", "i4"), ("kh", "i4"), ("kw", "i4"),
                                           ("flip", "i4"), ("dtype", "i4")])
            for i, (_, p, buf, kind, shp) in enumerate(ents):
                d[i] = (p.data_ptr(), buf.data_ptr(), shp[0], shp[1], shp[2], shp[3], int(kind[1]), ops._DT[kind[0]])
            table = torch.from_numpy(d.view(np.uint8).reshape(-1)).to(ents[0][1].device)
            hit = self._mp[id(opt)] = (sig, table)
        N.call("mv_dconv_multi_pack", _P(hit[1]), len(ents), ops._stream())
        for key, *_ in ents:
            self.mark_current(key)
        return len(ents)

    def get(self, param, dtype, flip):
        return self.lookup(param, (dtype, flip), lambda: _pack(_as4d(param).detach(), dtype, flip))

    def head_padded(self, wparam, bparam, dtype, flip, pad_to=32):
        """The [1,C,kh,kw] head zero-padded to `pad_to` output channels, packed for the MFMA conv (forward: flip 0, with the
        padded bias; data gradient: flip 1)."""
        def build():
            w = _as4d(wparam).detach()
            wp = torch.zeros(pad_to, *w.shape[1:], device=w.device, dtype=w.dtype)   # parameter-sized host-side glue
            wp[0] = w[0]
            buf = _pack(wp, dtype, flip)
            bias = torch.zeros(pad_to, device=w.device, dtype=dtype)
            bias[0:1] = bparam.detach().to(dtype)
            return buf, bias
        return self.lookup(wparam, ("headpad", dtype, flip), build)

    def head_mfma(self, param, dtype):
        """[1,C,kh,kw] head -> the tap-row MFMA operators of mv_dhead_fwd / mv_dhead_dgrad."""
        def build():
            w = _as4d(param).detach().contiguous()
            C, kh, kw = w.shape[1], w.shape[2], w.shape[3]
            buf = torch.empty(N.lib().mv_dhead_packed_bytes(C, ops._DT[dtype]), dtype=torch.uint8, device=w.device)
            N.call("mv_dhead_pack", _P(w), ops._DT[w.dtype], _P(buf), C, kh, kw, ops._DT[dtype], ops._stream())
            return buf
        return self.lookup(param, ("headmfma", dtype), build)

    def head(self, param):
        """[1,C,kh,kw] (or [1,C,k]) -> fp32 [taps][C]."""
        def build():
            w = _as4d(param).detach().contiguous()
            C, taps = w.shape[1], w.shape[2] * w.shape[3]
            wt = torch.empty(taps, C, device=w.device, dtype=torch.float32)
            N.call("mv_conv_out_pack", _P(w), ops._DT[w.dtype], _P(wt), C, taps, ops._stream())
            return wt
        return self.lookup(param, "head", build)


def _pack(w4, dtype, flip):
    """[Cout,Cin,kh,kw] -> the MFMA conv's packed image (flip = 1: the data-gradient operator)."""
    Cout, Cin, kh, kw = w4.shape
    w4 = w4.contiguous()
    buf = torch.empty(N.lib().mv_dconv_packed_bytes(Cout, Cin, kh, kw, ops._DT[dtype]), dtype=torch.uint8, device=w4.device)
    N.call("mv_dconv_pack", _P(w4), ops._DT[w4.dtype], _P(buf), Cout, Cin, kh, kw, int(flip), ops._DT[dtype], ops._stream())
    return buf


_packs = _PackCache()


def _as4d(w):
    return w if w.dim() == 4 else w.unsqueeze(2)        # Conv1d [O,C,k] -> [O,C,1,k]


def _cl_buffers(feats):
    """Logical [B,C,H,W] / [B,C,W] feature views (disc_features) -> their channels-last buffers; raises when a tensor is not such a view."""
    bufs = []
    for f in feats:
        b = f.permute(0, 2, 3, 1) if f.dim() == 4 else f.permute(0, 2, 1)
        if not b.is_contiguous():
            raise ValueError("feature matching: the real features must be the channels-last views that disc_features returns")
        bufs.append(b if f.dim() == 4 else b.unsqueeze(1))
    return bufs


def _logical(a, xdim):
    """Channels-last buffer [B,H,W,C] -> the logical [B,C,H,W] (or [B,C,W]) view of it."""
    return a.permute(0, 3, 1, 2) if xdim == 4 else a.view(a.shape[0], a.shape[2], a.shape[3]).permute(0, 2, 1)


class _Stack:
    """The one forward body and the one backward body of a discriminator stack.  `real` (optional): the real waveform's four hidden
    feature maps as channels-last buffers - the forward then also returns fm = sum_l mean|a_l - real_l| (fp32, 0-dim) and the backward
    adds that term's gradient to g right behind the data gradient that produces it (mv_fm_inject)."""

    @staticmethod
    def forward(ctx, x0, slope, params, real=None):
        """x0 [B,1,H,W] (MPD fold) or [B,1,W] (MSD, pooled); params = w1,b1,...,w5,b5.  Returns (out, acts, fm or None)."""
        ws = [_as4d(p) for p in params[0::2]]
        bs = list(params[1::2])
        dt = x0.dtype
        x0 = x0.contiguous()
        B = x0.shape[0]
        H, W = (x0.shape[2], x0.shape[3]) if x0.dim() == 4 else (1, x0.shape[2])
        kh, kw = ws[0].shape[2], ws[0].shape[3]
        st, dev = ops._stream, x0.device
        cast = lambda t: _cache.get(t, dt)
        acts = []
        C1 = ws[0].shape[0]
        a = torch.empty(B, H, W, C1, device=dev, dtype=dt)
        N.call("mv_dfirst_fwd_cl", _P(x0), _P(cast(params[0])), _P(cast(bs[0])), _P(a), B, H, W, C1, kh, kw, float(slope), ops._dt(x0), st())
        acts.append(a)
        C4 = ws[4].shape[1]
        hkh, hkw = ws[4].shape[2], ws[4].shape[3]
        mfma_head = C4 == 256 and hkh * hkw <= 16 and dt != torch.float32     # fp32: the padded-conv head below
        zws, head_fused = None, False
        for li in (1, 2, 3):
            Cout, Cin = ws[li].shape[0], ws[li].shape[1]
            y = torch.empty(B, H, W, Cout, device=dev, dtype=dt)
            if li == 3 and mfma_head and Cout == 256 and dt != torch.float32:
                # the head's per-tap partial sums come out of the last conv's epilogue tile (LDS): its 256-channel output is not read back
                zws = torch.empty(16, B * H * W, device=dev, dtype=torch.float32)
                rc = N.lib().mv_dconv_cl_fwd_head(_P(acts[-1]), _P(_packs.get(params[2 * li], dt, 0)), _P(cast(bs[li])), _P(y),
                                                  _P(_packs.head_mfma(params[8], dt)), _P(zws), hkh, hkw, B, H, W, Cin, Cout, kh, kw,
                                                  N.ACT_LRELU, float(slope), ops._dt(x0), st())
                if rc != N.MV_ERR_UNSUPPORTED:   # no 256-row variant for this geometry - separate launches below
                    N.check(rc, "mv_dconv_cl_fwd_head")
                    head_fused = True
            if not (li == 3 and head_fused):
                N.call("mv_dconv_cl_fwd", _P(acts[-1]), _P(_packs.get(params[2 * li], dt, 0)), _P(cast(bs[li])), None, _P(y), B, H, W, Cin, Cout,
                       kh, kw, 1, N.ACT_LRELU, float(slope), ops._dt(x0), st())
            acts.append(y)
        out = torch.empty((B, 1, H, W) if x0.dim() == 4 else (B, 1, W), device=dev, dtype=dt)
        if head_fused:
            N.call("mv_dhead_sum", _P(zws), _P(cast(bs[4])), _P(out), B, H, W, hkh, hkw, ops._dt(x0), st())
        elif mfma_head:
            # head (C4 -> 1): taps on the MFMA rows, x read once (mv_dhead_fwd)
            zws = torch.empty(16, B * H * W, device=dev, dtype=torch.float32) if zws is None else zws
            N.call("mv_dhead_fwd", _P(acts[-1]), _P(_packs.head_mfma(params[8], dt)), _P(cast(bs[4])), _P(zws), _P(out), B, H, W, C4,
                   kh, kw, ops._dt(x0), st())
        else:
            # generic width: MFMA conv with the output zero-padded to 32 channels, then channel 0 is extracted
            hp, hb = _packs.head_padded(params[8], bs[4], dt, 0)
            y32 = torch.empty(B, H, W, 32, device=dev, dtype=dt)
            N.call("mv_dconv_cl_fwd", _P(acts[-1]), _P(hp), _P(hb), None, _P(y32), B, H, W, C4, 32, kh, kw, 1, N.ACT_NONE, float(slope),
                   ops._dt(x0), st())
            N.call("mv_take_channel", _P(y32), _P(out), B * H * W, 32, 0, ops._dt(x0), st())
        fm = None
        if real is not None:
            for a, r in zip(acts, real):
                if r.shape != a.shape or r.dtype != a.dtype:
                    raise ValueError(f"feature matching: real feature {tuple(r.shape)} {r.dtype} does not match the stack's "
                                     f"{tuple(a.shape)} {a.dtype}")
            fm = ops._scalars.take(dev)
            for a, r in zip(acts, real):
                ops.fm_l1(a, r, acc=fm)
            fm = fm.view(())
        ctx.geom = (B, H, W, kh, kw, float(slope), x0.dim())
        ctx.save_for_backward(x0, *acts, *params, *(real or ()))
        return out, acts, fm

    @staticmethod
    def backward(ctx, gy, gfm=None, first_param=2):
        """Gradients (x0, *params).  gfm: the incoming gradient of fm (device scalar) - None skips the injection.  first_param: where
        the parameters start among the Function's forward arguments (ctx.needs_input_grad)."""
        B, H, W, kh, kw, slope, xdim = ctx.geom
        saved = ctx.saved_tensors
        x0, acts, params, real = saved[0], list(saved[1:5]), list(saved[5:15]), list(saved[15:])
        if gfm is None:
            real = []
        else:
            gfm = gfm.reshape(1).float()
        inject = lambda g, l: ops.fm_inject(g, acts[l], real[l], gfm, slope) if real else g
        if gy is None:                                     # only fm was used
            gy = ops._zeros((B, 1, H, W) if xdim == 4 else (B, 1, W), device=x0.device, dtype=x0.dtype)
        ws = [_as4d(p) for p in params[0::2]]
        bs = list(params[1::2])
        dt, dev, st = x0.dtype, x0.device, ops._stream
        gy = gy.contiguous()
        need = ctx.needs_input_grad
        need_w = any(need[first_param:])
        grads = [None] * 10
        f32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
        to = lambda g, p: (g.view(p.shape) if g.dtype == p.dtype else ops.cast(g.view(p.shape).contiguous(), p.dtype))
        # ---- head
        C4 = ws[4].shape[1]
        if need_w:
            taps = kh * kw
            if taps <= 16 and C4 % 8 == 0 and dt != torch.float32:
                # gw[tap][c] = sum_pos G[pos][tap] x[pos][c] with G = the flipped tap matrix of gy: a 1x1 weight-gradient GEMM
                # on the MFMA kernel; the centre column of G sums to the bias gradient
                tm = torch.empty(B, H, W, 16, device=dev, dtype=dt)
                N.call("mv_tap_matrix", _P(gy), _P(tm), B, H, W, kh, kw, 1, ops._dt(gy), st())
                gw16, gb16 = ops.dconv_wgrad_cl(acts[3], tm, 1, 1, want_bias=True)
                gwt = gw16.view(16, C4)[:taps]
                gb5 = gb16[taps // 2:taps // 2 + 1]
            else:
                gwt, gb5 = f32(taps, C4), f32(1)
                N.call("mv_dhead_wgrad", _P(gy), _P(acts[3]), _P(gwt), _P(gb5), B, H, W, C4, kh, kw, ops._dt(gy), st())
            gw5 = f32(C4, taps)                          # [taps][C] -> [C][taps] with our own transpose kernel
            N.call("mv_ntc_to_nct", _P(gwt), _P(gw5), 1, C4, taps, N.MV_F32, st())
            grads[8], grads[9] = to(gw5, params[8]), to(gb5, params[9])
        g = torch.empty(B, H, W, C4, device=dev, dtype=dt)
        if C4 == 256 and kh * kw <= 16 and dt != torch.float32:
            N.call("mv_dhead_dgrad", _P(gy), _P(_packs.head_mfma(params[8], dt)), _P(acts[3]), _P(g), B, H, W, C4, kh, kw, slope,
                   ops._dt(gy), st())
        else:
            g32 = torch.empty(B, H, W, 32, device=dev, dtype=dt)
            N.call("mv_put_channel", _P(gy), _P(g32), B * H * W, 32, 0, ops._dt(gy), st())
            hpf, _ = _packs.head_padded(params[8], bs[4], dt, 1)
            N.call("mv_dconv_cl_fwd", _P(g32), _P(hpf), None, _P(acts[3]), _P(g), B, H, W, 32, C4, kh, kw, 1, N.ACT_NONE, slope,
                   ops._dt(gy), st())
        g = inject(g, 3)
        # ---- wide layers 4, 3, 2 (indices 3, 2, 1)
        for li in (3, 2, 1):
            Cout, Cin = ws[li].shape[0], ws[li].shape[1]
            if need_w:
                gw, gb = f32(Cout, Cin, kh, kw), f32(Cout)
                ops.wgrad_cl_into(acts[li - 1], g, gw, gb, B, H, W, Cin, Cout, kh, kw, 1)
                grads[2 * li], grads[2 * li + 1] = to(gw, params[2 * li]), to(gb, params[2 * li + 1])
            gprev = torch.empty(B, H, W, Cin, device=dev, dtype=dt)
            N.call("mv_dconv_cl_fwd", _P(g), _P(_packs.get(params[2 * li], dt, 1)), None, _P(acts[li - 1]), _P(gprev), B, H, W, Cout, Cin,
                   kh, kw, 1, N.ACT_NONE, slope, ops._dt(g), st())
            g = inject(gprev, li - 1)
        # ---- first layer
        C1 = ws[0].shape[0]
        if need_w:
            taps = kh * kw
            if taps <= 16 and C1 % 8 == 0 and dt != torch.float32:
                # gw[o][tap] = sum_pos g1[pos][o] X[pos][tap] with X = the tap matrix of x0 (1x1 weight-gradient GEMM on MFMA)
                tm = torch.empty(B, H, W, 16, device=dev, dtype=dt)
                N.call("mv_tap_matrix", _P(x0), _P(tm), B, H, W, kh, kw, 0, ops._dt(g), st())
                gw16, gb1 = ops.dconv_wgrad_cl(tm, g, 1, 1, want_bias=True)
                gw1 = f32(C1, taps)
                ops.copy_rows(gw16.view(1, C1, 16), gw1.view(1, C1, taps))
            else:
                gw1, gb1 = f32(C1, taps), f32(C1)
                N.call("mv_dfirst_wgrad_cl", _P(g), _P(x0), _P(gw1), _P(gb1), B, H, W, C1, kh, kw, ops._dt(g), st())
            grads[0], grads[1] = to(gw1, params[0]), to(gb1, params[1])
        gx0 = None
        if need[0]:
            gx0 = torch.empty_like(x0)
            ws = torch.empty(N.lib().mv_dfirst_dgrad_workspace_bytes(B, H, W) // 4, device=dev, dtype=torch.float32)
            N.call("mv_dfirst_dgrad_cl", _P(g), _P(_cache.get(params[0], dt)), _P(gx0), _P(ws), B, H, W, C1, kh, kw, ops._dt(g), st())
        return (gx0, *grads)


class _DiscStack(Function):
    @staticmethod
    def forward(ctx, x0, slope, *params):
        return _Stack.forward(ctx, x0, slope, params)[0]

    @staticmethod
    def backward(ctx, gy):
        gx0, *grads = _Stack.backward(ctx, gy)
        return (gx0, None, *grads)


class _DiscStackFM(Function):
    """(x0, slope, real_feats, *params) -> (out, fm): the stack's output and fm = sum_l mean|a_l - real_l| over its four hidden
    feature maps, real_feats = the real waveform's maps from disc_features (constants: D(real).detach())."""

    @staticmethod
    def forward(ctx, x0, slope, real_feats, *params):
        ctx.set_materialize_grads(False)
        out, _, fm = _Stack.forward(ctx, x0, slope, params, _cl_buffers(real_feats))
        return out, fm

    @staticmethod
    def backward(ctx, gy, gfm):
        gx0, *grads = _Stack.backward(ctx, gy, gfm, first_param=3)
        return (gx0, None, None, *grads)


class _Discard:
    """Context of a forward whose saved tensors nobody will ask for."""

    def save_for_backward(self, *ts):
        pass


def _features(x0, slope, *params):
    out, acts, _ = _Stack.forward(_Discard(), x0, slope, params)
    return out, [_logical(a, x0.dim()) for a in acts]


_cache = ops._ParamCache()


def supported(x, blk) -> bool:
    """16-bit storage always; fp32 storage when the stack's `fp32_operands` is "split" (on the GPU)."""
    if x.dtype in (torch.bfloat16, torch.float16):
        return True
    return x.dtype == torch.float32 and x.is_cuda and getattr(blk, "fp32_operands", "exact") == "split"


def _params(blk):
    params = []
    for c in (blk.conv_layers[i] for i in (0, 2, 4, 6, 8)):
        params += [c.weight, c.bias]
    return params


def disc_stack(x0, blk, slope=0.1):
    from . import functional as Fn
    if Fn.DISPATCH == "torch_ops":
        return Fn._t().OPS.disc_conv_stack(x0, float(slope), *_params(blk))
    return _DiscStack.apply(x0, slope, *_params(blk))


def disc_features(x0, blk, slope=0.1):
    """The stack under no_grad: (out, [a_1..a_4]), a_l = hidden conv l after its LeakyReLU with logical shape [B,C,H,W] / [B,C,W], a
    permuted view of the stack's channels-last buffer."""
    from . import functional as Fn
    with torch.no_grad():
        if Fn.DISPATCH == "torch_ops":
            out, feats = Fn._t().OPS.disc_conv_stack_features(x0, float(slope), *_params(blk))
            return out, list(feats)
        return _features(x0, slope, *_params(blk))


def disc_stack_fm(x0, blk, real_feats, slope=0.1):
    """(out, fm) of _DiscStackFM."""
    from . import functional as Fn
    if Fn.DISPATCH == "torch_ops":
        return Fn._t().OPS.disc_conv_stack_fm(x0, float(slope), *real_feats, *_params(blk))
    return _DiscStackFM.apply(x0, slope, list(real_feats), *_params(blk))
