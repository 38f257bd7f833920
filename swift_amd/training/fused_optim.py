"""The optimisation step of ``Trainer._backward_step`` (reference training/trainer.py:219-247) as one HIP kernel.

The reference runs ``nan_to_num`` per gradient, ``torch.optim.AdamW.step()`` (about ten ``_foreach`` passes) and a
``lerp`` per EMA tensor: three sweeps over 226 M parameters and their moments.  ``FusedAdamEMA`` drives
``swiftk_adamw_ema_step`` instead: one pass that sanitises the gradient, applies the Adam / AdamW rule with the
optimizer's own hyper-parameters (``param_groups`` stay the source of truth: the LR schedule writes ``g["lr"]`` there)
and updates the EMA copy.  The torch optimizer object keeps owning the state: ``exp_avg`` / ``exp_avg_sq`` of every
parameter are views of two flat buffers and ``step`` is a shared counter tensor, so ``optimizer.state_dict()`` /
``load_state_dict()`` and the checkpoint format (trainer.py:522-535) are unchanged.

``FusedMarsEMA`` is the same arrangement for the MARS optimizer (training/optimizers/mars.py) on ``swiftk_mars_ema_step``:
two launches (per-chunk sums of squares of ``c_t``, then the update with the whole-tensor norm) where the torch-op class
runs about twenty ops and one device-to-host sync per parameter tensor.  ``last_grad`` is a third flat buffer of its own,
never a view of the gradient buffer, which the trainer clears in place.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from .._lib import (MARS_ADAMW, MARS_LION, MARS_RULE_ADAMW_1D, MARS_RULE_MARS, OPT_MAX_GROUPS, MarsChunk, MarsHyper, OptChunk,
                    OptHyper, SwiftkError, check, lib)
from .optimizers.mars import MARS

CHUNK = 16384


_MARS_TYPES = {"mars-adamw": MARS_ADAMW, "mars-lion": MARS_LION}


def _mars_supported(optimizer) -> bool:
    """MARS in its approximate form, mars-adamw / mars-lion, no amsgrad, fp32 device parameters, one (beta1, beta2) for all of
    at most OPT_MAX_GROUPS groups (``eps``, ``gamma``, the type and the 1-d settings are optimizer-level in MARS)."""
    gs = optimizer.param_groups
    if optimizer.mars_type not in _MARS_TYPES or not optimizer.is_approx or not 1 <= len(gs) <= OPT_MAX_GROUPS:
        return False
    for g in gs:
        if g.get("amsgrad") or tuple(g["betas"]) != tuple(gs[0]["betas"]):
            return False
        if any((not p.is_cuda) or p.dtype != torch.float32 for p in g["params"]):
            return False
    return True


def supported(optimizer) -> bool:
    """Plain Adam / AdamW on device parameters (no amsgrad / maximize / capturable / differentiable variants), or MARS
    (see ``_mars_supported``)."""
    if type(optimizer) is MARS:
        return _mars_supported(optimizer)
    if type(optimizer) not in (torch.optim.Adam, torch.optim.AdamW):
        return False
    gs = optimizer.param_groups
    if not 1 <= len(gs) <= OPT_MAX_GROUPS:
        return False
    b, e = gs[0]["betas"], gs[0]["eps"]
    for g in gs:
        if g.get("amsgrad") or g.get("maximize") or g.get("capturable") or g.get("differentiable"):
            return False
        if tuple(g["betas"]) != tuple(b) or g["eps"] != e:  # one (beta1, beta2, eps) per launch
            return False
        if any((not p.is_cuda) or p.dtype != torch.float32 for p in g["params"]):
            return False
    return True


def make(optimizer, net_params, ema_params, grad_flat):
    """The fused step that covers ``optimizer`` (``supported(optimizer)`` must hold)."""
    cls = FusedMarsEMA if type(optimizer) is MARS else FusedAdamEMA
    return cls(optimizer, net_params, ema_params, grad_flat)


class FusedAdamEMA:
    def __init__(self, optimizer, net_params: Sequence[torch.nn.Parameter], ema_params: Optional[Sequence[torch.Tensor]],
                 grad_flat: torch.Tensor):
        """``net_params`` in the order of ``grad_flat`` (every ``param.grad`` is a view of it); ``ema_params`` aligned with
        ``net_params`` (or None)."""
        if type(optimizer) is MARS or not supported(optimizer):
            raise SwiftkError("FusedAdamEMA needs torch.optim.Adam / AdamW on fp32 device parameters")
        self.opt = optimizer
        self.decoupled = type(optimizer) is torch.optim.AdamW
        dev = grad_flat.device
        group_of = {}
        for gi, g in enumerate(optimizer.param_groups):
            for p in g["params"]:
                group_of[id(p)] = gi
        n = grad_flat.numel()
        self.m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.v = torch.zeros(n, dtype=torch.float32, device=dev)
        self.step_t = torch.zeros((), dtype=torch.float32)
        chunks, off = [], 0
        self._keep = []
        for i, p in enumerate(net_params):
            if id(p) not in group_of:
                raise SwiftkError("every trainable parameter must be in one of the optimizer's param_groups")
            if not p.is_contiguous():
                raise SwiftkError("parameters must be contiguous")
            e = None if ema_params is None else ema_params[i]
            if e is not None and (e.shape != p.shape or not e.is_contiguous() or e.dtype != torch.float32):
                raise SwiftkError("EMA tensors must mirror the parameters (shape, fp32, contiguous)")
            st = optimizer.state.get(p, {})
            mv, vv = self.m[off:off + p.numel()].view_as(p), self.v[off:off + p.numel()].view_as(p)
            if "exp_avg" in st:  # resumed run: adopt the loaded moments (trainer.py:104-116)
                mv.copy_(st["exp_avg"])
                vv.copy_(st["exp_avg_sq"])
                self.step_t.fill_(float(st["step"]))
            optimizer.state[p] = {"step": self.step_t, "exp_avg": mv, "exp_avg_sq": vv}
            for s in range(0, p.numel(), CHUNK):
                k = min(CHUNK, p.numel() - s)
                chunks.append((p.data_ptr() + 4 * s, 0 if e is None else e.data_ptr() + 4 * s, off + s, k, group_of[id(p)]))
            off += p.numel()
        assert off == n
        arr = (OptChunk * len(chunks))()
        for j, (pp, ee, fo, k, gi) in enumerate(chunks):
            arr[j].p, arr[j].ema, arr[j].flat_off, arr[j].n, arr[j].group = pp, ee or None, fo, k, gi
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        self.table = host.to(dev)
        self.n_chunks = len(chunks)
        self.grad_flat = grad_flat
        self._touched = tuple(net_params) + tuple(e for e in (ema_params or ()) if e is not None)

    def step(self, ema_beta: float) -> None:
        """One fused step with the CURRENT ``param_groups`` hyper-parameters; bumps the parameters' version counters so
        the engines rebuild their GEMM-operand copies."""
        self.step_t += 1
        t = float(self.step_t)
        g0 = self.opt.param_groups[0]
        b1, b2 = g0["betas"]
        h = OptHyper()
        for gi, g in enumerate(self.opt.param_groups):
            h.lr[gi], h.weight_decay[gi] = float(g["lr"]), float(g["weight_decay"])
            h.step_size[gi] = float(g["lr"]) / (1.0 - b1 ** t)
        h.beta1, h.beta2, h.eps = float(b1), float(b2), float(g0["eps"])
        h.one_minus_beta1, h.one_minus_beta2 = 1.0 - b1, 1.0 - b2  # rounded from the double, as torch's lerp_ / addcmul_ weights
        h.bias2_sqrt = (1.0 - b2 ** t) ** 0.5
        h.ema_beta = float(ema_beta)
        h.decoupled = int(self.decoupled)
        check(lib().swiftk_adamw_ema_step(self.table.data_ptr(), self.n_chunks, self.grad_flat.data_ptr(), self.m.data_ptr(),
                                          self.v.data_ptr(), C.byref(h), torch.cuda.current_stream().cuda_stream),
              "swiftk_adamw_ema_step")
        # the kernel wrote through raw pointers: bump the version counters torch would have bumped, so the engines
        # (SwinEngine.refresh and friends compare (data_ptr, _version) stamps) rebuild their GEMM-operand copies
        ts = self._touched
        torch._C._autograd._unsafe_set_version_counter(ts, tuple(t._version + 1 for t in ts))


class FusedMarsEMA:
    def __init__(self, optimizer, net_params: Sequence[torch.nn.Parameter], ema_params: Optional[Sequence[torch.Tensor]],
                 grad_flat: torch.Tensor):
        """Arguments as for ``FusedAdamEMA``.  Per-parameter state keeps the class's keys: ``step`` (shared), ``exp_avg``,
        ``last_grad``, ``exp_avg_sq``."""
        if type(optimizer) is not MARS or not supported(optimizer):
            raise SwiftkError("FusedMarsEMA needs MARS (mars-adamw / mars-lion, is_approx, no amsgrad) on fp32 device parameters")
        self.opt = optimizer
        dev = grad_flat.device
        group_of = {}
        for gi, g in enumerate(optimizer.param_groups):
            for p in g["params"]:
                group_of[id(p)] = gi
        n = grad_flat.numel()
        self.m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.v = torch.zeros(n, dtype=torch.float32, device=dev)
        self.last = torch.zeros(n, dtype=torch.float32, device=dev)
        self.step_t = torch.zeros((), dtype=torch.float32)
        chunks, off = [], 0
        self.rules = []
        for ti, p in enumerate(net_params):
            if id(p) not in group_of:
                raise SwiftkError("every trainable parameter must be in one of the optimizer's param_groups")
            if not p.is_contiguous():
                raise SwiftkError("parameters must be contiguous")
            e = None if ema_params is None else ema_params[ti]
            if e is not None and (e.shape != p.shape or not e.is_contiguous() or e.dtype != torch.float32):
                raise SwiftkError("EMA tensors must mirror the parameters (shape, fp32, contiguous)")
            st = optimizer.state.get(p, {})
            sl = slice(off, off + p.numel())
            mv, vv, lv = self.m[sl].view_as(p), self.v[sl].view_as(p), self.last[sl].view_as(p)
            if "exp_avg" in st:  # resumed run: adopt the loaded moments and last gradient (trainer.py:104-116)
                mv.copy_(st["exp_avg"])
                vv.copy_(st["exp_avg_sq"])
                lv.copy_(st["last_grad"])
                self.step_t.fill_(float(st["step"]))
            optimizer.state[p] = {"step": self.step_t, "exp_avg": mv, "last_grad": lv, "exp_avg_sq": vv}
            rule = MARS_RULE_MARS if optimizer.uses_mars_rule(p) else MARS_RULE_ADAMW_1D
            self.rules.append(rule)
            first, count = len(chunks), -(-p.numel() // CHUNK)
            for s in range(0, p.numel(), CHUNK):
                k = min(CHUNK, p.numel() - s)
                chunks.append((p.data_ptr() + 4 * s, 0 if e is None else e.data_ptr() + 4 * s, off + s, k, group_of[id(p)], ti,
                               first, count, rule))
            off += p.numel()
        assert off == n
        arr = (MarsChunk * len(chunks))()
        for j, (pp, ee, fo, k, gi, ti, first, count, rule) in enumerate(chunks):
            c = arr[j]
            c.p, c.ema, c.flat_off, c.n, c.group = pp, ee or None, fo, k, gi
            c.tensor, c.first_chunk, c.tensor_chunks, c.rule = ti, first, count, rule
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        self.table = host.to(dev)
        self.n_chunks = len(chunks)
        self.partials = torch.empty(self.n_chunks, dtype=torch.float32, device=dev)  # written in full by the first launch
        self.norms = torch.zeros(len(net_params), dtype=torch.float32, device=dev)   # ||c_t|| per tensor of the last step
        self.grad_flat = grad_flat
        self._touched = tuple(net_params) + tuple(e for e in (ema_params or ()) if e is not None)

    def step(self, ema_beta: float) -> None:
        """One fused step with the CURRENT ``param_groups`` learning rates and weight decays; bumps the parameters' version
        counters so the engines rebuild their GEMM-operand copies.  Nothing here waits for the device."""
        self.step_t += 1
        t = float(self.step_t)
        o = self.opt
        o.step_num = int(t)
        b1, b2 = o.param_groups[0]["betas"]
        b1d, b2d = o.betas_1d
        h = MarsHyper()
        for gi, g in enumerate(o.param_groups):
            h.neg_lr[gi], h.neg_lr_1d[gi] = -g["lr"], -g["lr"] * o.lr_1d_factor
            h.weight_decay[gi] = float(g["weight_decay"])
        h.beta1, h.one_minus_beta1, h.beta2, h.one_minus_beta2 = b1, 1.0 - b1, b2, 1.0 - b2
        h.bias1, h.inv_bias2_sqrt = 1.0 - b1 ** t, 1.0 / (1.0 - b2 ** t) ** 0.5
        h.beta1_1d, h.one_minus_beta1_1d, h.beta2_1d, h.one_minus_beta2_1d = b1d, 1.0 - b1d, b2d, 1.0 - b2d
        h.bias1_1d, h.inv_bias2_sqrt_1d = 1.0 - b1d ** t, 1.0 / (1.0 - b2d ** t) ** 0.5
        h.weight_decay_1d = float(o.weight_decay if o.optimize_1d else o.weight_decay_1d)
        h.gamma_ratio = o.gamma * (b1 / (1.0 - b1))
        h.eps, h.ema_beta = float(o.eps), float(ema_beta)
        h.mars_type, h.n_groups = _MARS_TYPES[o.mars_type], len(o.param_groups)
        check(lib().swiftk_mars_ema_step(self.table.data_ptr(), self.n_chunks, self.grad_flat.data_ptr(), self.m.data_ptr(),
                                         self.v.data_ptr(), self.last.data_ptr(), self.partials.data_ptr(),
                                         self.norms.data_ptr(), C.byref(h), torch.cuda.current_stream().cuda_stream),
              "swiftk_mars_ema_step")
        ts = self._touched  # (raw-pointer writes: see FusedAdamEMA.step)
        torch._C._autograd._unsafe_set_version_counter(ts, tuple(t._version + 1 for t in ts))
