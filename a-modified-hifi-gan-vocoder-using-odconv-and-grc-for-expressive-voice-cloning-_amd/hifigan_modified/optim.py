"""Flat-arena AdamW (torch.optim.AdamW semantics: conditioned_hifigan.py:219, train_config.yaml:65-68).

All trainable parameters of a group live in ONE fp32 buffer (each nn.Parameter becomes a view of it), so an
optimizer step is a single HIP launch (mv_adamw_flat and its _hp / _clip forms: one kernel, csrc/train.hip) and the
data-parallel exchange is an all-reduce of ONE flat gradient buffer, cut into buckets.  Gradients produced by backward are
gathered into the flat buffer by one multi-tensor launch (mv_multi_gather; mv_multi_gather_acc inside an accumulation window).
Parameters that never receive a gradient (the unused ODConv attention heads) are left out of the arena exactly
like torch.optim skips ``grad is None``.
"""
from __future__ import annotations

import math
from ctypes import c_void_p

import numpy as np
import torch

from . import _native as N
from . import ops

_DESC = np.dtype([("src", np.uint64), ("dst_off", np.int64), ("n", np.int64), ("dtype", np.int32), ("pad", np.int32)])


class DeviceStateBlock:
    """A few bytes of per-step state that a captured training step reads from device memory, refreshed from the host before every
    replay: the host stays the single source of truth (step counts, lr and the other AdamW hyper-parameters, the dropout stream's
    counter) and the graph keeps only the block's address.  The upload is an asynchronous H2D copy from a small ring of pinned
    buffers on the current (replay) stream; a buffer is rewritten only after the event recorded behind its last copy has completed,
    so a host that runs ahead of the device never overwrites bytes still in flight."""

    RING = 4

    def __init__(self, nbytes, device):
        self.dev = torch.zeros(nbytes, dtype=torch.uint8, device=device)   # allocated outside any capture: its address is what graphs keep
        self._ring = [[torch.zeros(nbytes, dtype=torch.uint8).pin_memory(), None] for _ in range(self.RING)]
        self._next = 0

    def upload(self, values: np.ndarray):
        raw = np.ascontiguousarray(values).view(np.uint8).reshape(-1)
        if raw.size != self.dev.numel():
            raise ValueError(f"DeviceStateBlock: {raw.size} bytes for a {self.dev.numel()}-byte block")
        slot = self._ring[self._next % self.RING]
        self._next += 1
        if slot[1] is not None:
            slot[1].synchronize()
        slot[0].numpy()[:] = raw
        self.dev.copy_(slot[0], non_blocking=True)
        ev = slot[1] or torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev.device))
        slot[1] = ev


class FlatAdamW:
    def __init__(self, params, lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, exclude=()):
        excl = {id(p) for p in exclude}
        params = list(params)
        keep = [i for i, p in enumerate(params) if p.requires_grad and id(p) not in excl]
        self.torch_index = keep                  # position of each arena parameter in the list a torch.optim optimizer would enumerate
        self.params = [params[i] for i in keep]
        if not self.params:
            raise ValueError("FlatAdamW: no trainable parameters")
        dev = self.params[0].device
        if dev.type != "cuda" or any(p.device != dev or p.dtype != torch.float32 for p in self.params):
            raise RuntimeError("FlatAdamW needs fp32 parameters on one GPU (move the model first)")
        self.lr, self.betas, self.eps, self.weight_decay = lr, tuple(betas), eps, weight_decay
        self.offsets, off = [], 0
        for p in self.params:
            self.offsets.append(off)
            off += (p.numel() + 7) // 8 * 8          # keep every view (and its 16-bit shadow) 16-byte aligned
        self.numel = off
        self.flat_p = torch.zeros(off, device=dev, dtype=torch.float32)
        self.flat_g = torch.zeros(off, device=dev, dtype=torch.float32)
        self.exp_avg = torch.zeros(off, device=dev, dtype=torch.float32)
        self.exp_avg_sq = torch.zeros(off, device=dev, dtype=torch.float32)
        with torch.no_grad():
            for p, o in zip(self.params, self.offsets):
                view = self.flat_p[o:o + p.numel()].view(p.shape)
                ops.copy_rows(p.detach().reshape(1, 1, -1), view.view(1, 1, -1))
                p.data = view
        self.step_count = 0                  # optimizer steps taken (the largest per-parameter count)
        self.steps = [0] * len(self.params)  # per parameter, like torch.optim.AdamW's state[p]['step']: a parameter whose .grad is None
        #                                      in a step is left untouched, so its bias correction lags the others'
        self._n_all = len(params)            # parameters a torch.optim optimizer would enumerate (param_groups[0]['params'])
        self._capture = None                 # state of a captured training step (capture_begin / capture_end)
        self.ema = None                      # the ArenaEMA averaging this arena, if any (it attaches itself)
        # 16-bit shadows of the arena (one per activation dtype in use): refreshed by ONE cast launch per optimizer step, so
        # the ~200 per-parameter casts of a training step disappear; ops._ParamCache hands out views of them
        self._shadows = {}
        self._shadow_state = None            # (param epoch, per-parameter _version list) the shadows correspond to
        self._index = {id(p): i for i, p in enumerate(self.params)}
        ops.register_shadow_owner(self, self.params)
        self._descs = np.zeros(len(self.params), dtype=_DESC)
        self._descs["dst_off"] = self.offsets
        self._descs["n"] = [p.numel() for p in self.params]
        self._has_grad = None        # per parameter, set by the gathers of the current step (None = every parameter)
        self._pin_ring = {"slots": [], "next": 0}    # pinned staging buffers of the eager descriptor uploads (_upload)
        self._tables = []            # the last descriptor tables on the device, kept alive until their launches have consumed them
        # max_grad_norm clipping (step(max_grad_norm=...)): the value a captured step's replays read (before_replay uploads it) and the
        # trainers pass; None = no clipping.  grad_norm: the last step's gradient norm, a 0-d device tensor (never read by the host here)
        self.max_grad_norm = None
        self.grad_norm = None
        self._clip_buf = None        # fp32 {norm, coef} + the norm kernel's workspace, allocated at the first clipped step

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            p.grad = None

    def zero_arena(self):
        """Start of an accumulation window: the flat gradient buffer is zeroed (by a kernel, also inside a captured step) and no
        parameter has a gradient yet; the gathers of the window then run with accumulate=True."""
        from .torch_ops import OPS
        OPS.zero_(self.flat_g)
        self._has_grad = [False] * len(self.params)

    def _fill_descs(self, d, i0, accumulate, unknown):
        """Source pointer and dtype of descriptor rows `d` (parameters i0 .. i0 + len(d) - 1) from their .grad - a missing one is a
        NULL source - and the has-gradient bookkeeping: a parameter has a gradient when this gather gave it one or, accumulating,
        when an earlier one since the last overwrite / zero_arena() did.  `unknown`: what the parameters count as while no gather of
        this step has said (self._has_grad is None)."""
        if self._has_grad is None:
            self._has_grad = [unknown] * len(self.params)
        for j, p in enumerate(self.params[i0:i0 + len(d)]):
            g = p.grad
            self._has_grad[i0 + j] = (g is not None) or (accumulate and self._has_grad[i0 + j])
            if g is None:
                d["src"][j], d["dtype"][j] = 0, 0
            else:
                if not g.is_contiguous():
                    g = g.contiguous()
                    p.grad = g
                d["src"][j], d["dtype"][j] = g.data_ptr(), ops._DT[g.dtype]

    def _gather(self, d, accumulate):
        table = self._upload(d)
        n, max_len = len(d), int(d["n"].max())
        if accumulate:
            from .torch_ops import OPS
            OPS.multi_gather_acc_(table, n, max_len, self.flat_g)       # mv_multi_gather_acc
        else:
            N.call("mv_multi_gather", c_void_p(table.data_ptr()), n, max_len, c_void_p(self.flat_g.data_ptr()), ops._stream())
        self._tables = self._tables[-64:] + [table]   # keep alive until the launches have consumed them

    def gather_grads(self, accumulate=False):
        """param.grad tensors (fresh per backward) -> flat fp32 buffer; missing grads contribute zeros.  accumulate=True adds to the
        buffer instead (micro-steps of an accumulation window): a missing grad then adds nothing, and a parameter counts as having a
        gradient when any gather since the last overwrite / zero_arena() gave it one."""
        self._fill_descs(self._descs, 0, accumulate, unknown=False)     # every parameter is asked: nothing is taken on trust
        self._gather(self._descs, accumulate)
        return self.flat_g

    def _upload(self, descs):
        """Descriptor table -> device.  Under stream capture the copy becomes a node of the HIP graph: its source is a pinned
        host buffer that lives (unchanged) as long as the graph does - the gradient addresses it holds are the capture pool's, which
        every replay reuses."""
        raw = torch.from_numpy(descs.view(np.uint8).reshape(-1).copy())
        cap = self._capture
        if cap is not None:
            if not cap["pinned"]:
                raise RuntimeError("FlatAdamW: more gradient gathers in the captured step than capture_begin() prepared tables for")
            pin = cap["pinned"].pop()           # pinned BEFORE the capture began (host allocations invalidate a capture)
            pin[:raw.numel()].copy_(raw)
            cap["keep"].append(pin)
            return pin[:raw.numel()].to(self.flat_g.device, non_blocking=True)
        # eager path: a ring of pinned staging buffers, so that the copy is a real asynchronous H2D (from pageable memory it is staged
        # synchronously - a host stall per bucket while the backward is producing the next gradients).  A slot is reused only after the
        # copy that last read it has completed (event per slot; in steady state it has, long ago).
        ring, n = self._pin_ring, raw.numel()
        if len(ring["slots"]) < 16:
            ring["slots"].append([torch.empty(max(n, 4096), dtype=torch.uint8).pin_memory(), None])
            slot = ring["slots"][-1]
        else:
            slot = ring["slots"][ring["next"] % 16]
            ring["next"] += 1
            if slot[1] is not None:
                slot[1].synchronize()
            if slot[0].numel() < n:
                slot[0] = torch.empty(n, dtype=torch.uint8).pin_memory()
        slot[0][:n].copy_(raw)
        dev = slot[0][:n].to(self.flat_g.device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.flat_g.device))
        slot[1] = ev
        return dev

    def gather_range(self, i0, i1, accumulate=False):
        """Gather the gradients of parameters i0..i1-1 only (one launch): the per-bucket form used by
        parallel.OverlappedGradSync while the backward is still running.  Missing gradients contribute zeros; accumulate=True adds
        to the buffer like gather_grads(accumulate=True)."""
        d = self._descs[i0:i1].copy()
        self._fill_descs(d, i0, accumulate, unknown=True)       # the other buckets' parameters count as having one until asked
        self._gather(d, accumulate)

    def _runs(self, has=None):
        """Maximal runs (i0, i1) of consecutive parameters that share a step count, over the parameters with has[i] (None: all)."""
        runs, i, n = [], 0, len(self.params)
        while i < n:
            if has is not None and not has[i]:
                i += 1
                continue
            j = i + 1
            while j < n and (has is None or has[j]) and self.steps[j] == self.steps[i]:
                j += 1
            runs.append((i, j))
            i = j
        return runs

    def _clip_slots(self):
        """fp32 device buffer: [0] the gradient norm, [1] the clip coefficient, then the norm kernel's workspace."""
        if self._clip_buf is None:
            from .torch_ops import GRAD_NORM_WS_WORDS
            self._clip_buf = torch.zeros(2 + GRAD_NORM_WS_WORDS, device=self.flat_p.device, dtype=torch.float32)
            self.grad_norm = self._clip_buf[0]
        return self._clip_buf

    def step(self, grad_scale=1.0, gathered=False, max_grad_norm=None):
        """One AdamW update from the flat gradient buffer times grad_scale (1/world x 1/accumulation steps).  max_grad_norm: clip the
        scaled gradient's global L2 norm to it first (torch.nn.utils.clip_grad_norm_ over this optimizer's parameters): ONE norm over
        the whole arena - parameters without a gradient hold zeros there - whose coefficient every run of the update multiplies in on
        the device; `self.grad_norm` is that norm as a device tensor.  None: no norm, the unclipped kernels."""
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"FlatAdamW.step: max_grad_norm must be positive, got {max_grad_norm}")
        if not gathered:
            self.gather_grads()
        # torch.optim.AdamW leaves a parameter whose .grad is None untouched (no weight decay, no moment decay, no step): update only
        # the runs of parameters that received a gradient this step and share a step count - one launch when all did, the usual case
        runs = self._runs(self._has_grad)
        from .torch_ops import OPS
        cap = self._capture
        clip = None
        if max_grad_norm is not None:
            clip = self._clip_slots() if cap is None else self._clip_buf
            if cap is None:
                OPS.grad_norm(self.flat_g, clip, None, float(max_grad_norm), float(grad_scale))
            else:           # captured: max_norm is word 5 of the state block, refreshed from self.max_grad_norm before every replay
                if self.max_grad_norm is None or self._clip_buf is None:
                    raise RuntimeError("FlatAdamW: set optimizer.max_grad_norm before capture_begin() of a step that clips")
                cap["clip"] = True
                OPS.grad_norm(self.flat_g, clip, cap["block"].dev.view(torch.float32)[5:6], 0.0, float(grad_scale))
        for (i0, i1) in runs:   # torch.ops.mi355x_vocoder.fused_adamw_ (in place on the arena slices; mv_adamw_flat)
            t = self.steps[i0] + 1
            off = self.offsets[i0]
            cnt = (self.numel if i1 == len(self.params) else self.offsets[i1]) - off
            args = (self.flat_p[off:off + cnt], self.flat_g[off:off + cnt], self.exp_avg[off:off + cnt], self.exp_avg_sq[off:off + cnt],
                    float(self.lr), float(self.betas[0]), float(self.betas[1]), float(self.eps), float(self.weight_decay))
            if cap is None:
                if clip is None:
                    OPS.fused_adamw_(*args, int(t), float(grad_scale))
                else:
                    OPS.fused_adamw_clip_(*args[:4], None, None, *args[4:], int(t), float(grad_scale), clip[1:2])
                for k in range(i0, i1):
                    self.steps[k] = t
            else:
                # being captured (nothing executes now): the run's step count and the hyper-parameters are read from the state block
                # that before_replay() refreshes from the host; the host's counts move in after_replay()
                r = len(cap["runs"])
                if r >= len(cap["planned"]):
                    raise RuntimeError("FlatAdamW: the captured step does not update the arena as one run per step count")
                blk = cap["block"].dev
                if clip is None:
                    OPS.fused_adamw_hp_(*args[:4], blk.view(torch.float32)[:5], blk.view(torch.int32)[8 + r:9 + r], float(grad_scale))
                else:
                    OPS.fused_adamw_clip_(*args[:4], blk.view(torch.float32)[:5], blk.view(torch.int32)[8 + r:9 + r], 0.0, 0.0, 0.0, 0.0,
                                          0.0, 0, float(grad_scale), clip[1:2])
                cap["runs"].append((i0, i1))
        self.step_count = max(self.steps)
        self._has_grad = None
        ops.bump_param_epoch(self)       # in-place arena update: cached casts / packed weights of THESE parameters must refresh
        self._refresh_shadows()

    # ---- captured training steps (VocoderTrainer / HiFiGANTrainer with use_graph): everything the step launches is recorded once
    def capture_begin(self, stepping=True):
        """Call right before a training step is captured into a HIP graph (torch.cuda.graph): the gathers' descriptor tables become
        pinned and persistent, and AdamW reads its hyper-parameters and per-run step counts from a device state block (int32 words:
        0-4 fp32 {lr, beta1, beta2, eps, weight_decay}, 5 fp32 max_grad_norm (read by the gradient norm of a clipped step, 0 otherwise),
        6 fp32 one minus the EMA decay of this step (read by ArenaEMA.update's kernel; 0 without an attached EMA), 7 unused, 8 + r the
        count of run r) that before_replay() refreshes.  The norm and the clip coefficient themselves are
        written by the device into a buffer of their own (allocated here, before the capture).  stepping=False: the captured body
        only gathers (a micro-step inside an accumulation window) - no update, no runs, nothing to refresh."""
        dev = self.flat_p.device
        planned = self._planned_runs() if stepping else []
        block = DeviceStateBlock(4 * (8 + len(planned)), dev)
        nbytes = self._descs.nbytes
        pinned = [torch.empty(nbytes, dtype=torch.uint8).pin_memory() for _ in range(4)]
        if self.max_grad_norm is not None:
            self._clip_slots()
        self._capture = {"keep": [], "block": block, "runs": [], "planned": planned, "pinned": pinned, "clip": False,
                         "stepping": stepping, "ema": False}

    def _planned_runs(self):
        """Runs of equal step count over ALL parameters (a captured step must give every parameter of the arena a gradient)."""
        return self._runs()

    def capture_end(self):
        cap, self._capture = self._capture, None
        if cap is None:
            return None
        if cap["runs"] != cap["planned"]:
            raise RuntimeError("FlatAdamW: the captured step left parameters without a gradient: a captured step must update every "
                               "parameter of the arena")
        return {"keep": cap["keep"], "block": cap["block"], "runs": cap["runs"], "clip": cap["clip"], "stepping": cap["stepping"],
                "ema": cap["ema"]}

    def runs_match(self, state):
        """True while the host's step counts still form the runs the captured step was recorded with (a restored state can split or
        merge them: such a graph must be recaptured, not replayed)."""
        return self._planned_runs() == state["runs"]

    def before_replay(self, state):
        """Write this step's inputs into the captured step's state block (asynchronously, on the current stream): each run's step
        count + 1 and the current lr / betas / eps / weight_decay, exactly what the eager step would pass."""
        if not self.runs_match(state):
            raise RuntimeError("FlatAdamW: the step counts no longer form the captured runs: recapture the step")
        words = np.zeros(8 + len(state["runs"]), dtype=np.int32)
        words[:5].view(np.float32)[:] = (self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay)
        if state.get("clip"):
            if self.max_grad_norm is None or not self.max_grad_norm > 0:
                raise RuntimeError("FlatAdamW: the captured step clips its gradient norm: max_grad_norm must stay a positive number")
            words[5:6].view(np.float32)[:] = self.max_grad_norm
        if self.ema is not None:              # the same block, the same upload: this update's 1 - decay (warm-up moves it every step)
            words[6:7].view(np.float32)[:] = self.ema.one_minus_decay()
        words[8:] = [self.steps[i0] + 1 for (i0, _) in state["runs"]]
        state["block"].upload(words)

    def after_replay(self, state):
        """Host-side bookkeeping after one replay of a captured step: step counts and cache epochs."""
        for (i0, i1) in state["runs"]:
            for k in range(i0, i1):
                self.steps[k] += 1
        self.step_count = max(self.steps)
        if state.get("ema"):                  # the replayed step contained the EMA update
            self.ema.num_updates += 1
        ops.bump_param_epoch(self)
        self._shadow_state = (self._state_epoch(), [p._version for p in self.params])   # the replay refreshed the shadows itself

    def _refresh_shadows(self):
        for dt, sh in self._shadows.items():
            N.call("mv_cast", c_void_p(self.flat_p.data_ptr()), N.MV_F32, c_void_p(sh.data_ptr()), ops._DT[dt], self.numel, ops._stream())
        self._shadow_state = (self._state_epoch(), [p._version for p in self.params])

    def _state_epoch(self):
        return (ops._FINE[0], getattr(self, "_epoch", 0))

    def owns(self, p):
        i = self._index.get(id(p))
        return i is not None and self.params[i] is p

    def shadow_view(self, p, dtype):
        """The `dtype` copy of parameter p as a view of the arena's shadow, or None when p was modified behind the arena's back
        (load_state_dict / copy_ since the last refresh) - the caller then casts it the slow way."""
        i = self._index.get(id(p))
        if i is None or self.params[i] is not p:
            return None
        st = self._shadow_state
        if dtype not in self._shadows or st is None or st[0] != self._state_epoch() or st[1][i] != p._version:
            if st is not None and st[0] == self._state_epoch() and st[1][i] != p._version:
                return None
            if dtype not in self._shadows:
                self._shadows[dtype] = torch.empty(self.numel, device=self.flat_p.device, dtype=dtype)
            self._refresh_shadows()
            if self._shadow_state[1][i] != p._version:
                return None
        o = self.offsets[i]
        return self._shadows[dtype][o:o + p.numel()].view(p.shape)

    def torch_state_dict(self):
        """The same state in torch.optim.AdamW's layout (what the reference's load path expects)."""
        state = {}
        for k, (p, o, ti) in enumerate(zip(self.params, self.offsets, self.torch_index)):
            if self.steps[k] == 0:
                continue                      # torch creates a parameter's state at its first update
            state[ti] = {"step": torch.tensor(float(self.steps[k])), "exp_avg": self.exp_avg[o:o + p.numel()].view(p.shape).clone(),
                         "exp_avg_sq": self.exp_avg_sq[o:o + p.numel()].view(p.shape).clone()}
        n_all = self._n_all
        group = {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "params": list(range(n_all))}
        return {"state": state, "param_groups": [group]}

    def state_dict(self):
        return {"step": self.step_count, "steps": list(self.steps), "exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone(),
                "lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay}

    def load_state_dict(self, sd):
        """Accepts this class's flat layout, or a torch.optim.AdamW state_dict ({'state': {i: {step, exp_avg, exp_avg_sq}},
        'param_groups': [...]}, the 'optimizer_state_dict' of a reference checkpoint: conditioned_hifigan.py:292-299) built over
        the same parameter list: entry i belongs to the i-th parameter the torch optimizer enumerated (self.torch_index)."""
        if "state" in sd and "param_groups" in sd:
            g0 = sd["param_groups"][0]
            self.lr, self.betas, self.eps = g0.get("lr", self.lr), tuple(g0.get("betas", self.betas)), g0.get("eps", self.eps)
            self.weight_decay = g0.get("weight_decay", self.weight_decay)
            self.exp_avg.zero_()
            self.exp_avg_sq.zero_()
            self.steps = [0] * len(self.params)
            with torch.no_grad():
                for k, (p, o, ti) in enumerate(zip(self.params, self.offsets, self.torch_index)):
                    st = sd["state"].get(ti, sd["state"].get(str(ti)))
                    if st is None:
                        continue
                    if st["exp_avg"].numel() != p.numel():
                        raise ValueError(f"optimizer state {ti}: {tuple(st['exp_avg'].shape)} does not fit parameter {tuple(p.shape)}")
                    self.exp_avg[o:o + p.numel()].copy_(st["exp_avg"].reshape(-1))
                    self.exp_avg_sq[o:o + p.numel()].copy_(st["exp_avg_sq"].reshape(-1))
                    self.steps[k] = int(st["step"])
            self.step_count = max(self.steps) if self.steps else 0
            return
        self.step_count = int(sd["step"])
        self.steps = [int(x) for x in sd["steps"]] if "steps" in sd else [self.step_count] * len(self.params)
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.lr, self.betas, self.eps, self.weight_decay = sd["lr"], tuple(sd["betas"]), sd["eps"], sd["weight_decay"]


class ArenaEMA:
    """Exponential moving average of one FlatAdamW arena (the generator's weights): `shadow`, an fp32 buffer laid out like
    `opt.flat_p`, follows it by ONE streaming launch per optimizer step (mv_ema_update: shadow += w * (flat_p - shadow), w = 1 - decay).
    warmup: the decay of update number n (from 0) is min(decay, (1 + n) / (10 + n)), so the average leaves its initial value quickly
    and only later becomes slow; formed on the host in Python floats, w = float32(1 - that).  Inside a captured step the kernel reads
    w from word 6 of the optimizer's state block, which FlatAdamW.before_replay refreshes with the rest of the block; the host's
    `num_updates` moves in after_replay.  The arena's padding words are averaged too: zeros on both sides."""

    def __init__(self, opt, decay, warmup=True):
        if isinstance(decay, bool) or not isinstance(decay, (int, float, np.floating)) or not 0.0 < decay < 1.0:
            raise ValueError(f"ArenaEMA: decay must be a number in (0, 1), got {decay!r}")
        self.opt, self.decay, self.warmup = opt, float(decay), bool(warmup)
        self.shadow = torch.empty(opt.numel, device=opt.flat_p.device, dtype=torch.float32)
        self.reset()
        opt.ema = self

    def reset(self):
        """The average starts over from the arena's current weights."""
        self.shadow.copy_(self.opt.flat_p)          # device to device
        self.num_updates = 0

    def current_decay(self):
        """The decay the NEXT update uses."""
        if not self.warmup:
            return self.decay
        return min(self.decay, (1 + self.num_updates) / (10 + self.num_updates))

    def one_minus_decay(self):
        return np.float32(1.0 - self.current_decay())

    def update(self):
        from .torch_ops import OPS
        opt = self.opt
        cap = opt._capture
        if cap is None:
            OPS.ema_update_(self.shadow, opt.flat_p, None, float(self.one_minus_decay()))
            self.num_updates += 1
        else:       # being captured (nothing executes now): w comes from the state block, the count moves in after_replay()
            cap["ema"] = True
            OPS.ema_update_(self.shadow, opt.flat_p, cap["block"].dev.view(torch.float32)[6:7], 0.0)

    def swap(self):
        """Exchange the arena and the average (one launch): the modules then compute with the averaged weights, and every cast and
        packed weight derived from the arena follows.  Twice restores both buffers bit for bit."""
        from .torch_ops import OPS
        OPS.swap_(self.opt.flat_p, self.shadow)
        ops.bump_param_epoch(self.opt)
        self.opt._refresh_shadows()

    def named_tensors(self, module=None):
        """(name, view of the average with the parameter's shape) per arena parameter.  The names are `module`'s (named_parameters)
        for the arena parameters it holds; without a module, the parameters' positions in the arena."""
        if module is None:
            names = {id(p): str(i) for i, p in enumerate(self.opt.params)}
        else:
            names = {id(p): n for n, p in module.named_parameters()}
        return [(names[id(p)], self.shadow[o:o + p.numel()].view(p.shape))
                for p, o in zip(self.opt.params, self.opt.offsets) if id(p) in names]

    def state_dict(self):
        return {"decay": self.decay, "warmup": self.warmup, "num_updates": self.num_updates, "shadow": self.shadow.clone()}

    def load_state_dict(self, sd):
        if sd["shadow"].numel() != self.shadow.numel():
            raise ValueError(f"ArenaEMA: a shadow of {sd['shadow'].numel()} elements does not fit an arena of {self.shadow.numel()}")
        self.decay, self.warmup, self.num_updates = float(sd["decay"]), bool(sd["warmup"]), int(sd["num_updates"])
        self.shadow.copy_(sd["shadow"].reshape(-1))


class WarmupCosineLR:
    """Linear warmup, then cosine decay to `min_lr` (train_config.yaml:54-72: learning_rate 2e-4, warmup_steps 2000, scheduler
    "cosine", min_lr 1e-6), host side, in the shape of torch's LRScheduler: step() / get_last_lr() / state_dict() /
    load_state_dict().  After s completed step() calls the lr is base_lr * f(s) with m = min_lr / base_lr and
        f(s) = (s + 1) / W                                              s < W
        f(s) = m + (1 - m) * (1 + cos(pi * min(1, (s - W) / (S - W)))) / 2    otherwise.
    It sets `optimizer.lr` on a FlatAdamW and every group's 'lr' on a torch.optim optimizer; a captured training step picks the
    value up at its next replay (FlatAdamW.before_replay)."""

    def __init__(self, optimizer, warmup_steps, total_steps, min_lr=0.0):
        if warmup_steps < 0:
            raise ValueError(f"WarmupCosineLR: warmup_steps must be >= 0, got {warmup_steps}")
        if total_steps <= warmup_steps:
            raise ValueError(f"WarmupCosineLR: total_steps ({total_steps}) must exceed warmup_steps ({warmup_steps})")
        self.optimizer = optimizer
        self.warmup_steps, self.total_steps, self.min_lr = int(warmup_steps), int(total_steps), float(min_lr)
        groups = getattr(optimizer, "param_groups", None)
        if groups is not None:
            self.base_lrs = [g.setdefault("initial_lr", g["lr"]) for g in groups]
        else:
            self.base_lrs = [optimizer.lr]
        self.last_epoch = 0
        self._apply()

    def factor(self, s, base_lr):
        W, S = self.warmup_steps, self.total_steps
        if s < W:
            return (s + 1) / W
        m = self.min_lr / base_lr
        return m + (1 - m) * 0.5 * (1 + math.cos(math.pi * min(1.0, (s - W) / (S - W))))

    def _apply(self):
        lrs = [b * self.factor(self.last_epoch, b) for b in self.base_lrs]
        groups = getattr(self.optimizer, "param_groups", None)
        if groups is not None:
            for g, lr in zip(groups, lrs):
                g["lr"] = lr
        else:
            self.optimizer.lr = lrs[0]
        self._last_lr = lrs

    def step(self):
        self.last_epoch += 1
        self._apply()

    def get_last_lr(self):
        return list(self._last_lr)

    def state_dict(self):
        return {"last_epoch": self.last_epoch, "base_lrs": list(self.base_lrs), "warmup_steps": self.warmup_steps,
                "total_steps": self.total_steps, "min_lr": self.min_lr}

    def load_state_dict(self, sd):
        self.last_epoch, self.base_lrs = int(sd["last_epoch"]), [float(b) for b in sd["base_lrs"]]
        self.warmup_steps, self.total_steps, self.min_lr = int(sd["warmup_steps"]), int(sd["total_steps"]), float(sd["min_lr"])
        self._apply()
