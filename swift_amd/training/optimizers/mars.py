"""MARS (variance-reduced AdamW / Lion, arXiv 2411.10438) with the constructor contract, defaults, ``param_groups`` and
``state_dict()`` layout of reference src/swift/training/optimizers/mars.py:107-305, so optimizer state travels between
the two in both directions.  Per-parameter state: ``step``, ``exp_avg``, ``last_grad``, ``exp_avg_sq`` (+ ``max_exp_avg_sq``
under amsgrad; + ``previous_grad`` once the exact form has been used).

The rule, per parameter tensor with gradient ``g`` and the previous step's gradient ``g'``:

    MARS rule (``g.ndim == 2`` exactly, or ``optimize_1d``):
        c   = g + gamma * beta1 / (1 - beta1) * (g - g')
        c   = c / ||c||           only if the whole-tensor norm exceeds 1
        m   = beta1 * m + (1 - beta1) * c
        mars-adamw:  v = beta2 * v + (1 - beta2) * c^2
                     p -= lr * (wd * p + m / ((sqrt(v) / sqrt(1 - beta2^t) + eps) * (1 - beta1^t)))
        mars-lion:   p -= lr * (wd * p + sign(m))
        mars-shampoo (2-D): p -= lr * (wd * p + sqrt(max(1, rows / cols)) * NewtonSchulz(m / (1 - beta1)))
    AdamW-1d rule (everything else: norms, biases, the 3-D ``pos_embed``), with ``betas_1d`` and ``weight_decay_1d``:
        the same moments and denominator on g itself, step lr * lr_1d_factor

Quirks kept on purpose: ``lr_1d_factor = lr_1d / lr`` is fixed at construction and multiplies the *scheduled* group ``lr``;
``betas_1d`` and the 1-d weight decay are optimizer-level, not per group (with ``optimize_1d`` the optimizer-level
``weight_decay`` would be the 1-d decay, but then no tensor takes the 1-d rule); ``eps`` joins after the
``1 / sqrt(bias_correction2)`` scaling and the sum is multiplied by ``bias_correction1``.

One deliberate difference: ``last_grad`` is storage of its own.  The reference keeps a *reference* to the step's gradient
tensor, which is right only because its ``zero_grad(set_to_none=True)`` allocates fresh gradients every step.  Here every
``param.grad`` is a view of one flat buffer that is cleared in place and overwritten by the next backward pass: an aliased
``last_grad`` would always equal the current gradient and silently switch the variance-reduction term off.

``mars-adamw`` and ``mars-lion`` run on any device through torch ops (on fp32 device parameters the trainer replaces this
sequence by ``swiftk_mars_ema_step``, training/fused_optim.py).  ``mars-shampoo`` is accepted, and its Newton-Schulz
iteration runs in plain torch (bf16 matmuls, no ``torch.compile``).
"""
from __future__ import annotations

import math

import torch
from torch.optim.optimizer import Optimizer

MARS_TYPES = ("mars-adamw", "mars-lion", "mars-shampoo")


def newton_schulz(M: torch.Tensor, steps: int = 5, eps: float = 1e-7) -> torch.Tensor:
    """Quintic Newton-Schulz orthogonalisation in bf16 (the iteration of Muon), on the wide orientation of ``M``."""
    a, b, c = 3.4445, -4.7750, 2.0315
    X = M.bfloat16() / (M.norm() + eps)
    tall = M.size(0) > M.size(1)
    if tall:
        X = X.T
    for _ in range(steps):
        A = X @ X.T
        B = A @ X
        X = a * X + b * B + c * A @ B
    if tall:
        X = X.T
    return X.to(M.dtype)


def _adam_denom(second: torch.Tensor, beta1: float, beta2: float, step, eps: float) -> torch.Tensor:
    bias1, bias2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    return second.sqrt().mul(1 / math.sqrt(bias2)).add(eps).mul(bias1)


class MARS(Optimizer):
    def __init__(self, params, lr=3e-3, betas=(0.95, 0.99), eps=1e-8, weight_decay=0.0, amsgrad=False, gamma=0.025,
                 is_approx=True, mars_type="mars-adamw", optimize_1d=False, lr_1d=3e-3, betas_1d=(0.9, 0.95),
                 weight_decay_1d=0.1):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        assert mars_type in MARS_TYPES, "MARS type not supported"
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, mars_type=mars_type,
                        gamma=gamma, optimize_1d=optimize_1d, weight_decay_1d=weight_decay_1d)
        super().__init__(params, defaults)
        # optimizer-level settings: the step reads these, not the per-group copies above
        self.eps, self.lr, self.weight_decay, self.amsgrad = eps, lr, weight_decay, amsgrad
        self.step_num = 0
        self.is_approx = is_approx
        self.gamma, self.mars_type, self.optimize_1d = gamma, mars_type, optimize_1d
        self.lr_1d_factor = lr_1d / lr
        self.weight_decay_1d, self.betas_1d = weight_decay_1d, betas_1d

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("amsgrad", False)

    # -- the exact form (is_approx=False): the caller evaluates the PREVIOUS batch at the current weights, stores that
    #    gradient with update_previous_grad(), and after the step moves it into last_grad with update_last_grad()
    @torch.no_grad()
    def update_last_grad(self):
        if self.is_approx:
            return
        for group in self.param_groups:
            for p in group["params"]:
                state = self.state[p]
                if "last_grad" not in state:
                    state["last_grad"] = torch.zeros_like(p)
                state["last_grad"].copy_(state["previous_grad"])

    @torch.no_grad()
    def update_previous_grad(self):
        if self.is_approx:
            return
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                if "previous_grad" not in state:
                    state["previous_grad"] = torch.zeros_like(p)
                state["previous_grad"].copy_(p.grad)

    def uses_mars_rule(self, p: torch.Tensor) -> bool:
        """The MARS rule applies to exactly-2-D tensors (or to all under ``optimize_1d``); the rest take the AdamW-1d rule."""
        return bool(self.optimize_1d) or p.ndim == 2

    def _mars_update(self, p, grad, state, group, step):
        beta1, beta2 = group["betas"]
        lr, wd = group["lr"], group["weight_decay"]
        m, v = state["exp_avg"], state["exp_avg_sq"]
        c = (grad - state["last_grad"]).mul(self.gamma * (beta1 / (1.0 - beta1))).add(grad)
        norm = torch.norm(c)
        if norm > 1.0:
            c = c / norm
        m.mul_(beta1).add_(c, alpha=1.0 - beta1)
        kind = self.mars_type
        if kind == "mars-adamw" or (kind == "mars-shampoo" and grad.ndim != 2):
            v.mul_(beta2).addcmul_(c, c, value=1.0 - beta2)
            second = v
            if group["amsgrad"]:
                second = torch.max(state["max_exp_avg_sq"], v, out=state["max_exp_avg_sq"])
            direction = m.div(_adam_denom(second, beta1, beta2, step, self.eps))
        elif kind == "mars-lion":
            direction = m.sign()
        else:  # mars-shampoo on a matrix
            factor = max(1, grad.size(0) / grad.size(1)) ** 0.5
            direction = newton_schulz(m.mul(1.0 / (1.0 - beta1)), eps=self.eps).mul(factor)
        p.add_(-lr * torch.mul(p, wd).add(direction))

    def _adamw_1d_update(self, p, grad, state, group, step):
        beta1, beta2 = self.betas_1d
        wd = self.weight_decay if self.optimize_1d else self.weight_decay_1d
        m, v = state["exp_avg"], state["exp_avg_sq"]
        m.mul_(beta1).add_(grad, alpha=1.0 - beta1)
        v.mul_(beta2).addcmul_(grad, grad, value=1.0 - beta2)
        second = v
        if group["amsgrad"]:
            second = torch.max(state["max_exp_avg_sq"], v, out=state["max_exp_avg_sq"])
        direction = m.div(_adam_denom(second, beta1, beta2, step, self.eps))
        p.add_(-group["lr"] * self.lr_1d_factor * torch.mul(p, wd).add(direction))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        step = self.step_num
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                grad = p.grad
                if grad.is_sparse:
                    raise RuntimeError("MARS does not support sparse gradients")
                state = self.state[p]
                if len(state) <= 1:  # fresh, or holding nothing but previous_grad
                    state["step"] = 0
                    state["exp_avg"] = torch.zeros_like(p)
                    state["last_grad"] = torch.zeros_like(p)
                    state["exp_avg_sq"] = torch.zeros_like(p)
                    if group["amsgrad"]:
                        state["max_exp_avg_sq"] = torch.zeros_like(p)
                step = state["step"] = int(state["step"]) + 1
                if self.uses_mars_rule(grad):
                    self._mars_update(p, grad, state, group, step)
                else:
                    self._adamw_1d_update(p, grad, state, group, step)
                if self.is_approx:
                    state["last_grad"].copy_(grad)  # a copy: see the module docstring
        self.step_num = step
        return loss
