"""Optimisers.  `KerasAdam` is the rule of `tf.keras.optimizers.Adam`, what the reference's model scripts train with
(models/bls2017.py:243-245): epsilon = 1e-7, added to sqrt(v) and not to the bias-corrected sqrt(v_hat), both bias
corrections folded into the step size.  `torch.optim.Adam` is a different rule (epsilon 1e-8 on sqrt(v_hat)) and runs
as a series of passes over every tensor; here device parameters take one kernel per `KERAS_ADAM_CAPACITY` tensors
(ops/train_ops.py, csrc/train.hip)."""
from __future__ import annotations

import torch

from .ops import train_ops

__all__ = ["KerasAdam"]


class KerasAdam(torch.optim.Optimizer):
    """`KerasAdam(params, lr=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7)`.  Per-parameter state: `exp_avg`,
    `exp_avg_sq`; the step count `step` is kept per group, and `group["lr"]` may be changed between steps."""

    def __init__(self, params, lr=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7):
        if lr < 0.0:
            raise ValueError(f"lr must not be negative, got {lr}")
        if not 0.0 <= beta_1 < 1.0 or not 0.0 <= beta_2 < 1.0:
            raise ValueError(f"beta_1 and beta_2 must be in [0, 1), got {beta_1} and {beta_2}")
        if epsilon < 0.0:
            raise ValueError(f"epsilon must not be negative, got {epsilon}")
        super().__init__(params, dict(lr=lr, beta_1=beta_1, beta_2=beta_2, epsilon=epsilon, step=0))

    @torch.no_grad()
    def step(self, closure=None, *, skip=None):
        """One step over every parameter that has a gradient.  `skip`: an int32 device tensor of one element or None;
        while it is nonzero the parameters and the state stay as they are (the step count still advances).  Nothing
        here waits for the device."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            by_device = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                for name, t in (("parameter", p), ("gradient", p.grad)):
                    if t.dtype != torch.float32:
                        raise TypeError(f"KerasAdam: a {name} of shape {tuple(t.shape)} is {t.dtype}, float32 is needed")
                    if t.is_sparse or not t.is_contiguous():
                        raise ValueError(f"KerasAdam: a {name} of shape {tuple(t.shape)} is not contiguous")
                state = self.state[p]
                if not state:
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                lists = by_device.setdefault(p.device, ([], [], [], []))
                for lst, t in zip(lists, (p, p.grad, state["exp_avg"], state["exp_avg_sq"])):
                    lst.append(t)
            if not by_device:
                continue
            group["step"] += 1
            for lists in by_device.values():
                train_ops.keras_adam(*lists, lr=group["lr"], beta_1=group["beta_1"], beta_2=group["beta_2"],
                                     epsilon=group["epsilon"], step=group["step"], skip=skip)
        return loss
