"""Preconditioner wrappers that own the network (mirror reference src/swift/models/precond.py:39-151).

``PassPrecond`` = identity scaling + channel-concat of the condition.  The concat of
precond.py:139-141 is not materialised: the sources go to the patch-gather kernel as separate
pointers.  ``EDMPrecond`` (precond.py:39-98) puts its input scaling c_in into the same gather (a per-sample factor
on source 0) and its output combination c_skip x + c_out F into the un-patchify epilogue: one fused network call.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..config import instantiate
from .abstract import AbstractNetwork


def _2d_resolution(x) -> np.ndarray:
    """An int or an (H, W) pair -> ``np.array([H, W])``, the type callers of the reference read from ``net.img_resolution``
    (precond.py:9-18)."""
    hw = np.broadcast_to(np.asarray(x, dtype=int).reshape(-1), (2,)) if np.ndim(x) == 0 else np.asarray(x, dtype=int)
    if hw.shape != (2,):
        raise AssertionError(f"img_resolution must be an int or a pair, got {x!r}")
    return np.array(hw)


def _process_auxiliary(auxiliary, auxiliary_dim, batch_size, device):
    """scalar / [1] / [B] / None -> [B|1, auxiliary_dim]  (precond.py:21-31).  None stands for a zero lead time (one row that the
    network broadcasts); a Python number is materialised by a fill kernel rather than a pageable host-to-device copy (capturable
    into a HIP graph); tensors on another device are brought over without a host stall."""
    if not auxiliary_dim:
        return None
    dev = torch.device(device)
    if auxiliary is None:
        return torch.zeros(1, auxiliary_dim, device=dev)
    if isinstance(auxiliary, (int, float)):
        aux = torch.full((), float(auxiliary), dtype=torch.float32, device=dev)
    else:
        aux = auxiliary if torch.is_tensor(auxiliary) else torch.as_tensor(auxiliary)
        if aux.device != dev:  # (the trainer keeps lead times on the host; pinned loader batches copy asynchronously)
            aux = aux.to(dev, non_blocking=True)
    if aux.numel() == 1 and aux.dim() <= 1:  # one value for the whole batch
        aux = aux.reshape(1).expand(batch_size)
    return aux.reshape(-1, auxiliary_dim)


class PassPrecond(torch.nn.Module):
    def __init__(
        self,
        model_config,
        img_resolution,
        img_channels: int,
        condition_channels: int = 0,
        auxiliary_dim: int = 0,
        sigma_min: float = 0.0,
        sigma_max: float = float("inf"),
        sigma_data: float = 1.0,
    ):
        super().__init__()
        self.img_resolution = _2d_resolution(img_resolution)
        self.img_channels = img_channels
        self.condition_channels = condition_channels
        self.auxiliary_dim = auxiliary_dim
        self.sigma_min, self.sigma_max, self.sigma_data = sigma_min, sigma_max, sigma_data
        self.model_config = model_config
        self.model: AbstractNetwork = instantiate(
            model_config,
            img_resolution=[int(v) for v in self.img_resolution],
            in_channels=img_channels + condition_channels,
            out_channels=img_channels,
            auxiliary_dim=auxiliary_dim,
            _convert_="object",
        )

    def forward(self, x, t, condition=None, auxiliary=None, **model_kwargs):
        """x [B,C,H,W], t [B], condition [B,Cc,H,W] -> F [B,C,H,W]  (precond.py:133-148).

        Extra keyword arguments beyond the reference's ``jvp`` / ``return_logvar``:
        ``x_scale`` (multiplies x inside the patch gather: x_t / sigma_d) and ``xt, alpha, beta``
        (out = alpha*xt + beta*F fused into the un-patchify) used by the samplers.
        """
        aux = _process_auxiliary(auxiliary, self.auxiliary_dim, x.size(0), x.device)
        model_kwargs.pop("jvp", None)
        x_scale = model_kwargs.pop("x_scale", 1.0)
        srcs, scales = [x], [x_scale]
        if condition is not None and self.condition_channels > 0:
            # additive extension: a (state, forcings) pair is accepted as-is, saving the caller's concat
            parts = list(condition) if isinstance(condition, (tuple, list)) else [condition]
            assert sum(p.shape[1] for p in parts) == self.condition_channels
            srcs += parts
            scales += [1.0] * len(parts)
        return self.model.forward_sources(srcs, scales, t.flatten(), aux, **model_kwargs)

    def round_sigma(self, sigma):
        return torch.as_tensor(sigma)


class EDMPrecond(torch.nn.Module):
    """EDM preconditioning (precond.py:39-98): D(x; sigma) = c_skip x + c_out F(c_in x, ln(sigma) / 4) with
    c_skip = sd^2 / (sigma^2 + sd^2), c_out = sigma sd / sqrt(sigma^2 + sd^2), c_in = 1 / sqrt(sigma^2 + sd^2).

    Same constructor kwargs, attributes and state-dict keys (``model.*``) as the reference.  ``c_in * x`` is the patch
    gather's per-sample scale of source 0 and ``c_skip x + c_out F`` the un-patchify epilogue (alpha = c_skip, beta = c_out,
    xt = x), so a forward is one fused network call; only [B]-sized coefficient math runs as torch ops, and a device sigma
    needs no host sync.
    """

    def __init__(
        self,
        model_config,
        img_resolution,
        img_channels: int,
        condition_channels: int = 0,
        auxiliary_dim: int = 0,
        sigma_min: float = 0.0,
        sigma_max: float = float("inf"),
        sigma_data: float = 0.5,
    ):
        super().__init__()
        self.img_resolution = _2d_resolution(img_resolution)
        self.img_channels = img_channels
        self.condition_channels = condition_channels
        self.auxiliary_dim = auxiliary_dim
        self.sigma_min, self.sigma_max, self.sigma_data = sigma_min, sigma_max, sigma_data
        self.model_config = model_config
        self.model: AbstractNetwork = instantiate(
            model_config,
            img_resolution=[int(v) for v in self.img_resolution],
            in_channels=img_channels + condition_channels,
            out_channels=img_channels,
            auxiliary_dim=auxiliary_dim,
            _convert_="object",
        )

    def _sources(self, x, condition):
        srcs, scales = [x], [1.0]
        if condition is not None and self.condition_channels > 0:
            parts = list(condition) if isinstance(condition, (tuple, list)) else [condition]
            assert sum(p.shape[1] for p in parts) == self.condition_channels
            srcs += parts
            scales += [1.0] * len(parts)
        return srcs, scales

    def forward(self, x, sigma, condition=None, auxiliary=None, **model_kwargs):
        """x [B,C,H,W], sigma (a number, a 0-d / [1] tensor or a [B] tensor), condition [B,Cc,H,W] -> D [B,C,H,W].

        The samplers pass ``xt, alpha, beta`` (numbers or [B] tensors) for a different fused output, alpha*xt + beta*F,
        with F the raw network output at (c_in(sigma) x, c_noise(sigma)).  A number sigma keeps the coefficients on the host
        (c_in becomes the gather's scalar source scale); a tensor sigma gives device [B] coefficients."""
        B, dev = x.size(0), x.device
        aux = _process_auxiliary(auxiliary, self.auxiliary_dim, B, dev)
        model_kwargs.pop("jvp", None)
        xt, alpha, beta = model_kwargs.pop("xt", None), model_kwargs.pop("alpha", None), model_kwargs.pop("beta", None)
        sd = float(self.sigma_data)
        srcs, scales = self._sources(x, condition)

        def vec(v):
            return torch.full((B,), float(v), dtype=torch.float32, device=dev) if not torch.is_tensor(v) else \
                v.to(dev, torch.float32, non_blocking=True).reshape(-1).expand(B).contiguous()

        if isinstance(sigma, (int, float)):
            sg = torch.tensor(float(sigma), dtype=torch.float32)  # fp32 host arithmetic, as the reference's fp32 tensors
            s2 = sg * sg + sd * sd
            c_in, c_noise = float(1 / s2.sqrt()), float(sg.log() / 4)
            c_skip, c_out = float(sd * sd / s2), float(sg * sd / s2.sqrt())
            scales[0] = c_in
            t, s0 = torch.full((B,), c_noise, dtype=torch.float32, device=dev), None
        else:
            sg = sigma if torch.is_tensor(sigma) else torch.as_tensor(sigma)
            sg = sg.to(dev, torch.float32, non_blocking=True).reshape(-1)
            if sg.numel() == 1:
                sg = sg.expand(B)
            if sg.numel() != B:
                raise ValueError(f"sigma must be a number, a 0-d / [1] tensor or a [{B}] tensor, got shape {tuple(sigma.shape)}")
            s2 = sg * sg + sd * sd
            s0, t = torch.rsqrt(s2).contiguous(), (torch.log(sg) / 4).contiguous()
            c_skip, c_out = sd * sd / s2, sg * sd * s0
        if alpha is None and beta is None and xt is None:  # D = c_skip x + c_out F
            xt, alpha, beta = x, c_skip, c_out
        alpha = None if alpha is None else vec(alpha)
        beta = None if beta is None else vec(beta)
        if xt is not None:
            xt = xt.contiguous().float()
        return self.model.forward_sources(srcs, scales, t, aux, xt=xt, alpha=alpha, beta=beta, src0_scale=s0, **model_kwargs)

    def round_sigma(self, sigma):
        return torch.as_tensor(sigma)
