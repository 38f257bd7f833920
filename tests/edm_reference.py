"""TEST INFRASTRUCTURE: a plain PyTorch-CPU restatement of the reference's three EDM functions on top of
``oracle.swinv2.OracleNet`` (whose call is the bare network F(x, t, condition, auxiliary)).

  * ``precond``      -- models/precond.py:72-92   (EDMPrecond.forward)
  * ``time_steps``   -- generating/diffusion.py:32-48 (the rho grid of edm_sampler, in a given dtype)
  * ``edm_sampler``  -- generating/diffusion.py:10-92 (fp32 state; churn noise from ``randn_like``)
  * ``edm_loss``     -- training/loss.py:95-114 with the draws (sigma [B,1,1,1], z) injected

tests/test_edm_cpu.py pins every one of them to tests/golden/edm_tiny.npz, which the reference itself produced
(tools/make_golden.py); the GPU tests then measure the product against them.
"""
from __future__ import annotations

import math

import numpy as np
import torch


def precond(net, x, sigma, condition=None, auxiliary=None, sigma_data=None, **kw):
    sd = net.sigma_data if sigma_data is None else sigma_data
    sigma = torch.as_tensor(sigma, dtype=x.dtype).reshape(-1, 1, 1, 1)
    c_skip = sd ** 2 / (sigma ** 2 + sd ** 2)
    c_out = sigma * sd / (sigma ** 2 + sd ** 2).sqrt()
    c_in = 1 / (sd ** 2 + sigma ** 2).sqrt()
    c_noise = (sigma.log() / 4).flatten()
    if c_noise.numel() == 1:
        c_noise = c_noise.expand(x.shape[0])
    F = net(c_in * x, c_noise, condition, auxiliary, **kw)
    return c_skip * x + c_out * F


def time_steps(num_steps, sigma_min, sigma_max, rho=7, dtype=torch.float32):
    step_indices = torch.arange(num_steps, dtype=dtype)
    t = (sigma_max ** (1 / rho) + step_indices / (num_steps - 1) * (sigma_min ** (1 / rho) - sigma_max ** (1 / rho))) ** rho
    return torch.cat([t, torch.zeros_like(t[:1])])


@torch.no_grad()
def edm_sampler(net, latents, condition=None, auxiliary=None, randn_like=torch.randn_like, num_steps=18, sigma_min=0.002,
                sigma_max=80, rho=7, S_churn=0, S_min=0, S_max=float("inf"), S_noise=1, grid_dtype=torch.float32, **kw):
    """fp32 state; the grid, gamma, t_hat, sqrt(t_hat^2 - t^2) and t_next - t_hat in ``grid_dtype`` (the reference's
    ``denoise_dtype``: bf16 under its bf16 sampler)."""
    sigma_min = max(sigma_min, net.sigma_min)
    sigma_max = min(sigma_max, net.sigma_max)
    t_steps = time_steps(num_steps, sigma_min, sigma_max, rho, grid_dtype)
    x_next = latents.float() * t_steps[0].float()
    for i, (t_cur, t_next) in enumerate(zip(t_steps[:-1], t_steps[1:])):
        x_cur = x_next
        gamma = min(S_churn / num_steps, np.sqrt(2) - 1) if S_min <= t_cur <= S_max else 0
        t_hat = t_cur + gamma * t_cur
        x_hat = x_cur + (t_hat ** 2 - t_cur ** 2).sqrt().float() * S_noise * randn_like(x_cur)
        denoised = precond(net, x_hat, t_hat.float(), condition, auxiliary, **kw)
        d_cur = (x_hat - denoised) / t_hat.float()
        x_next = x_hat + (t_next - t_hat).float() * d_cur
        if i < num_steps - 1:
            denoised = precond(net, x_next, t_next.float(), condition, auxiliary, **kw)
            d_prime = (x_next - denoised) / t_next.float()
            x_next = x_hat + (t_next - t_hat).float() * (0.5 * d_cur + 0.5 * d_prime)
    return x_next


def edm_loss(net, x, sigma, z, w_var, w_lat, sigma_data, condition=None, auxiliary=None):
    sigma = sigma.reshape(-1, 1, 1, 1)
    weight = (sigma ** 2 + sigma_data ** 2) / (sigma * sigma_data) ** 2
    D = precond(net, x + z * sigma, sigma, condition, auxiliary, sigma_data=sigma_data)
    return (weight * (w_var * w_lat * (D - x) ** 2)).sum(dim=1).mean()


def lognormal_sigma(B: int, P_mean: float, P_std: float, generator=None) -> torch.Tensor:
    return torch.exp(torch.randn([B, 1, 1, 1], generator=generator) * P_std + P_mean)


__all__ = ["precond", "time_steps", "edm_sampler", "edm_loss", "lognormal_sigma", "math"]
