"""detectron2.solver: `build_lr_scheduler` for the schedule the reference configures (configs/Base.yaml:1-9:
WarmupMultiStepLR, linear warm-up; tools/train_net.py:125 builds it, :248 steps it once per iteration).

    lr(it) = base_lr * gamma ** #{milestones <= it} * f(it),   f(it) = wf * (1 - it/W) + it/W  for it < W, else 1

(SURVEY.md Appendix A.16).  Works on any optimizer with `param_groups` (FlatSGD reads each group's "lr" at step time).

`maybe_add_gradient_clipping` / `GradientClipType`: detectron2.solver.build's SOLVER.CLIP_GRADIENTS (contract in its docstring)."""
import bisect
import copy
import math
from enum import Enum

import torch


class WarmupMultiStepLR:
    def __init__(self, optimizer, milestones, gamma=0.1, warmup_factor=0.001, warmup_iters=1000, warmup_method="linear",
                 last_epoch=-1):
        if list(milestones) != sorted(milestones):
            raise ValueError("Milestones should be a list of increasing integers. Got {}".format(milestones))
        if warmup_method not in ("linear", "constant"):
            raise ValueError("Unknown warmup method: {}".format(warmup_method))
        self.optimizer, self.milestones, self.gamma = optimizer, list(milestones), gamma
        self.warmup_factor, self.warmup_iters, self.warmup_method = warmup_factor, warmup_iters, warmup_method
        self.base_lrs = [g.setdefault("initial_lr", g["lr"]) for g in optimizer.param_groups]
        self.last_epoch = last_epoch
        self.step()

    def _factor(self, it):
        if it >= self.warmup_iters:
            return 1.0
        if self.warmup_method == "constant":
            return self.warmup_factor
        alpha = it / self.warmup_iters
        return self.warmup_factor * (1 - alpha) + alpha

    def get_lr(self):
        k = bisect.bisect_right(self.milestones, self.last_epoch)
        return [b * self._factor(self.last_epoch) * self.gamma ** k for b in self.base_lrs]

    def get_last_lr(self):
        return [g["lr"] for g in self.optimizer.param_groups]

    def step(self):
        self.last_epoch += 1
        for g, lr in zip(self.optimizer.param_groups, self.get_lr()):
            g["lr"] = lr

    def state_dict(self):
        return {"last_epoch": self.last_epoch, "base_lrs": self.base_lrs}

    def load_state_dict(self, sd):
        self.last_epoch, self.base_lrs = sd["last_epoch"], list(sd["base_lrs"])
        for g, lr in zip(self.optimizer.param_groups, self.get_lr()):
            g["lr"] = lr


class WarmupCosineLR(WarmupMultiStepLR):
    def __init__(self, optimizer, max_iters, **kw):
        self.max_iters = max_iters
        super().__init__(optimizer, [], **kw)

    def get_lr(self):
        f = self._factor(self.last_epoch)
        return [b * f * 0.5 * (1.0 + math.cos(math.pi * self.last_epoch / self.max_iters)) for b in self.base_lrs]


def build_lr_scheduler(cfg, optimizer):
    name = cfg.SOLVER.LR_SCHEDULER_NAME
    kw = dict(warmup_factor=cfg.SOLVER.WARMUP_FACTOR, warmup_iters=cfg.SOLVER.WARMUP_ITERS, warmup_method=cfg.SOLVER.WARMUP_METHOD)
    if name == "WarmupMultiStepLR":
        steps = [x for x in cfg.SOLVER.STEPS if x <= cfg.SOLVER.MAX_ITER]
        return WarmupMultiStepLR(optimizer, steps, cfg.SOLVER.GAMMA, **kw)
    if name == "WarmupCosineLR":
        return WarmupCosineLR(optimizer, cfg.SOLVER.MAX_ITER, **kw)
    raise ValueError("Unknown LR scheduler: {}".format(name))


# ---- SOLVER.CLIP_GRADIENTS: detectron2.solver.build.maybe_add_gradient_clipping ---------------------------------------------------
class GradientClipType(Enum):
    VALUE = "value"
    NORM = "norm"


def _create_gradient_clipper(clip_cfg):
    """-> per-parameter clipper of torch's functions (the class-swap path for optimizers other than the flat ones)"""
    clip_cfg = copy.deepcopy(clip_cfg)
    kind = GradientClipType(clip_cfg.CLIP_TYPE)

    def clip_grad_norm(p):
        torch.nn.utils.clip_grad_norm_(p, clip_cfg.CLIP_VALUE, clip_cfg.NORM_TYPE)

    def clip_grad_value(p):
        torch.nn.utils.clip_grad_value_(p, clip_cfg.CLIP_VALUE)

    return {GradientClipType.VALUE: clip_grad_value, GradientClipType.NORM: clip_grad_norm}[kind]


def _with_gradient_clipping(optimizer_type, per_param_clipper):
    def step(self, closure=None):
        for group in self.param_groups:
            for p in group["params"]:
                per_param_clipper(p)
        return super(type(self), self).step(closure)
    return type(optimizer_type.__name__ + "WithGradientClip", (optimizer_type,), {"step": step})


def maybe_add_gradient_clipping(cfg, optimizer):
    """SOLVER.CLIP_GRADIENTS {ENABLED, CLIP_TYPE, CLIP_VALUE, NORM_TYPE}, as cubercnn/solver/build.py:68 applies it last.

    Contract (detectron2 v0.6 semantics, restated; not verifiable in this container, detectron2 is not installed here):
      * ENABLED False: `optimizer` is returned unchanged.
      * ENABLED True: the optimizer's class is swapped for a subclass whose step() clips EACH parameter on its own before the parent's
        step: `for group in param_groups: for p in group["params"]: clipper(p)`.  `optimizer` may also be a class: the subclass is
        returned.
      * CLIP_TYPE "value": torch.nn.utils.clip_grad_value_(p, CLIP_VALUE) = grad.clamp_(-v, v); NaN stays NaN.
      * CLIP_TYPE "norm": torch.nn.utils.clip_grad_norm_(p, CLIP_VALUE, NORM_TYPE) on the single tensor: n = vector_norm(grad,
        NORM_TYPE) (inf = max |grad|), coef = min(CLIP_VALUE / (n + 1e-6), 1), grad *= coef always (a coef of 1 is an exact no-op).
        A NaN in the gradient makes n and coef NaN; an Inf makes coef 0 (inf * 0 = NaN in that element).
      * any other CLIP_TYPE: ValueError (GradientClipType(...)).
      * the clip acts on the gradient before weight decay, momentum or Adam's moments; under DDP on the averaged gradient; in the
        reference loop inside optimizer.step() (tools/train_net.py:250), i.e. after the NaN scan (:222-233) and never on a skipped
        iteration.

    The flat optimizers of cubercnn/solver/build.py (FlatSGD / FlatAdam) are not swapped: `arm_clipping` turns on the fused form --
    per-parameter norms of the flat gradient bucket in two launches (with the deferred 1/world of the exchange folded in), the
    coefficient or the clamp applied by the update kernels as they read the gradient.  The one difference from the reference: the
    clipped gradient is not written back, p.grad keeps the unclipped (averaged) gradient."""
    clip = cfg.SOLVER.CLIP_GRADIENTS
    if not clip.ENABLED:
        return optimizer
    kind = GradientClipType(clip.CLIP_TYPE)
    armed = (kind.value, float(clip.CLIP_VALUE), float(clip.NORM_TYPE))
    if isinstance(optimizer, torch.optim.Optimizer):
        optimizer_type = type(optimizer)
    else:
        if not (isinstance(optimizer, type) and issubclass(optimizer, torch.optim.Optimizer)):
            raise TypeError(f"expected a torch.optim.Optimizer or a subclass of it, got {optimizer!r}")
        optimizer_type = optimizer
    if hasattr(optimizer_type, "arm_clipping"):               # the fused flat-bucket optimizers
        if optimizer_type is optimizer:
            def __init__(self, *args, **kw):
                optimizer_type.__init__(self, *args, **kw)
                self.arm_clipping(*armed)
            return type(optimizer_type.__name__ + "WithGradientClip", (optimizer_type,), {"__init__": __init__})
        optimizer.arm_clipping(*armed)
        return optimizer
    clipped_type = _with_gradient_clipping(optimizer_type, _create_gradient_clipper(clip))
    if optimizer_type is optimizer:
        return clipped_type
    optimizer.__class__ = clipped_type
    return optimizer
