"""The accumulation window both trainers share (``VocoderTrainer``, ``HiFiGANTrainer``).

A window is `accumulation_steps` consecutive `train_step` calls.  Every call's gradients are added to the optimizers' flat
buffers (zeroed by a kernel at the window's first call); only the last call reduces across the ranks and updates, on the
window's sum times 1/N, clipped to `max_grad_norm` when one is set.  With the defaults (N = 1, no norm) every call is a
whole window: nothing is zeroed, the gathers overwrite, every call steps.

Per call:   do_step = w.begin_call(opts); scale = w.backward(loss, opt, do_step); [w.apply(opt, scale)]; w.end_call()
"""
from __future__ import annotations

import numpy as np


class GradWindow:
    def __init__(self, who, accumulation_steps=1, max_grad_norm=None, grad_sync=None, bucket_mib=8):
        """`who`: the trainer's name in error messages.  The two keywords (configs/train_config.yaml: gradient_accumulation_steps;
        configs/incremental_train_config.yaml: max_grad_norm): a whole number of micro-steps >= 1 and a positive norm (or None: no
        clipping).  grad_sync: "overlap" (the default when the world size is > 1) reduces each optimizer's buckets UNDER its
        backward (parallel.OverlappedGradSync); a parallel.GradSynchronizer reduces the flat buffer after it; False never reduces."""
        if isinstance(accumulation_steps, bool) or not isinstance(accumulation_steps, (int, np.integer)) or accumulation_steps < 1:
            raise ValueError(f"{who}: accumulation_steps must be an integer >= 1, got {accumulation_steps!r}")
        if max_grad_norm is not None and (isinstance(max_grad_norm, bool) or not isinstance(max_grad_norm, (int, float, np.floating))
                                          or not max_grad_norm > 0):
            raise ValueError(f"{who}: max_grad_norm must be a positive number or None, got {max_grad_norm!r}")
        self.who = who
        self.accumulation_steps = int(accumulation_steps)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.position = 0                    # position of the next train_step call inside its window
        if grad_sync is None:
            import torch.distributed as dist
            grad_sync = "overlap" if (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1) else False
        self.grad_sync = grad_sync
        self.bucket_mib = bucket_mib
        self.overlap = {}                    # id(optimizer) -> its OverlappedGradSync

    def adopt(self, *opts):
        """The trainer's optimizers: accumulation and clipping work on FlatAdamW's arena (refused here, not at the first step), and
        each optimizer takes the trainer's max_grad_norm (a captured step reads the optimizer's own value at every replay)."""
        from .optim import FlatAdamW
        if self.accumulation_steps == 1 and self.max_grad_norm is None:
            return
        for opt in opts:
            if not isinstance(opt, FlatAdamW):
                raise ValueError(f"{self.who}: accumulation_steps > 1 and max_grad_norm work on FlatAdamW's gradient arena; "
                                 f"got a {type(opt).__name__}")
            if self.max_grad_norm is not None:
                opt.max_grad_norm = self.max_grad_norm

    def overlap_sync(self, opt):
        """The OverlappedGradSync of a FlatAdamW optimizer (created on first use), or None when overlap is off."""
        if self.grad_sync != "overlap" and self.grad_sync is not True:
            return None
        ov = self.overlap.get(id(opt))
        if ov is None:
            from .parallel import OverlappedGradSync
            ov = self.overlap[id(opt)] = OverlappedGradSync(opt, bucket_mib=self.bucket_mib)
        return ov

    def begin_call(self, opts):
        """Start of a train_step call: a new window (N > 1) zeroes the arenas of `opts`, in that order.  Returns do_step: whether
        this call is the window's last (always, without accumulation)."""
        if self.accumulation_steps > 1 and self.position == 0:
            for opt in opts:
                opt.zero_arena()
        return self.position == self.accumulation_steps - 1

    def backward(self, loss, opt, do_step):
        """loss.backward() + the gather into the arena (adding, inside a window) + the data-parallel gradient mean, which only the
        call that steps takes.  Returns the gradient scale for `apply` (1/world x 1/N), or None when there is no update to make:
        do_step is False, or `opt` is a plain torch optimizer (defaults only), which has stepped here on its reduced .grad tensors."""
        from .optim import FlatAdamW
        if not isinstance(opt, FlatAdamW):
            loss.backward()
            if self.grad_sync:
                import torch.distributed as dist
                w = dist.get_world_size()
                for g in opt.param_groups:
                    for p in g["params"]:
                        if p.grad is not None:
                            dist.all_reduce(p.grad)
                            p.grad.div_(w)
            opt.step()
            return None
        acc = self.accumulation_steps > 1
        ov = self.overlap_sync(opt)
        if ov is not None:
            ov.begin(accumulate=acc, reduce=do_step)     # buckets reduce while autograd is still producing the other gradients
            loss.backward()
            scale = ov.finish()
        else:
            loss.backward()
            flat = opt.gather_grads(accumulate=acc)
            scale = 1.0
            if self.grad_sync and do_step:
                self.grad_sync.start(flat)
                scale = self.grad_sync.finish()
        return scale * (1.0 / self.accumulation_steps) if do_step else None

    def apply(self, opt, scale):
        """The FlatAdamW update from the gathered (and reduced) arena, clipped when the trainer has a max_grad_norm."""
        if self.max_grad_norm is None:
            opt.step(grad_scale=scale, gathered=True)
        else:           # the optimizer's own value: it may be changed between steps (a captured step reads it at every replay)
            opt.step(grad_scale=scale, gathered=True, max_grad_norm=opt.max_grad_norm)

    def end_call(self):
        self.position = (self.position + 1) % self.accumulation_steps

    def reset(self):
        """Back to a window boundary (a loaded checkpoint is always one)."""
        self.position = 0

    def assert_boundary(self, who):
        if self.position != 0:
            raise RuntimeError(f"{who}: in the middle of an accumulation window ({self.position} of {self.accumulation_steps} "
                               "micro-steps taken): the partial gradient sums are not part of a checkpoint - save after the call "
                               "that steps")

    def checkpoint_extras(self):
        """Informational checkpoint keys (the constructor's arguments decide on load); a default trainer writes none."""
        if self.accumulation_steps == 1 and self.max_grad_norm is None:
            return {}
        return {"accumulation_steps": self.accumulation_steps, "max_grad_norm": self.max_grad_norm}
