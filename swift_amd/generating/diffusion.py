"""TrigFlow / sCM samplers on the gfx950 engine (mirrors reference src/swift/generating/diffusion.py).

Same solver names, keyword arguments and time grids as the reference's ``DiffusionSampler``
(scm_solver :417-461, dpm_solver_2s :355-415).  Differences in *how*, not *what*:
  * ``x_t / sigma_d`` is folded into the patch-gather kernel and the state update
    ``cos(t) x_t - sin(t) sigma_d F`` (or the Euler step) into the un-patchify epilogue, so a
    1-step sCM sample is exactly one fused network call;
  * the remaining state arithmetic (re-noising, Heun average) runs in ``swiftk_axpby``;
  * the time grid is built on the host in fp32 with the same torch ops as the reference and
    read back once (no per-step device->host sync).
``dpm_solver`` (:289-353, the in-training validation solver) is built the same way, and so is ``edm_sampler`` (:10-92,
the stochastic Heun sampler of EDM nets): c_in in the gather, every Euler / Heun update in the epilogue.  ablation_sampler
and scm_solve2 are out of scope.
"""
from __future__ import annotations

import contextlib
import math
from typing import Callable, Optional, Sequence

import torch

from .. import ops


@contextlib.contextmanager
def engine_for(module, dtype, device_type: str = "cuda"):
    """Select the compute engine of ``denoise_dtype`` for the calls inside the block: torch.bfloat16 = the bf16 MFMA engine
    (through autocast, as the reference's ``autocast(dtype=denoise_dtype)``, diffusion.py:457), torch.float32 = the
    exact-fp32 engine, the string "bf16x3" = the fp32-grade engine built from three bf16 products per GEMM (fp32
    activations; what ``generate --dtype bf16x3`` runs)."""
    model = getattr(module, "model", module)
    x3 = isinstance(dtype, str) and dtype == "bf16x3"
    if isinstance(dtype, str) and not x3:
        raise ValueError(f"denoise_dtype {dtype!r}: expected torch.float32, torch.bfloat16 or 'bf16x3'")
    prev = getattr(model, "fp32_engine", None)
    if x3:
        model.fp32_engine = "bf16x3"
    try:
        with torch.autocast(device_type, enabled=(dtype == torch.bfloat16), dtype=torch.bfloat16):
            yield
    finally:
        if x3:
            model.fp32_engine = prev


def _log_sigma_grid(num_steps: int, sigma_min: float, sigma_max: float, sigma_data: float) -> torch.Tensor:
    lo, hi = torch.log(torch.tensor(sigma_min)), torch.log(torch.tensor(sigma_max))
    u = torch.linspace(1, 0, num_steps)
    return torch.atan(torch.exp(lo + u * (hi - lo)) / sigma_data)


def scm_time_steps(num_steps, sigma_min, sigma_max, sigma_data, intermediates=None) -> torch.Tensor:
    """diffusion.py:434-449 (host tensor, fp32)."""
    if num_steps == 1:
        t = torch.tensor([torch.pi / 2])
    else:
        t = _log_sigma_grid(num_steps, sigma_min, sigma_max, sigma_data)
    t = torch.cat([t, torch.zeros(1)])
    if num_steps == 2 and intermediates is None:
        t = torch.tensor([t[0], 1.1, 0.0])
    elif intermediates:
        t = torch.cat([t[:1], torch.as_tensor(intermediates, dtype=torch.float32), t[-1:]])
    return t


def edm_time_steps(num_steps: int, sigma_min: float, sigma_max: float, rho: float, dtype: torch.dtype = torch.float32
                   ) -> torch.Tensor:
    """diffusion.py:37-48: the rho grid with t_N = 0 appended, in ``dtype`` arithmetic (host tensor; bf16 under the bf16
    engine, as the reference's ``torch.arange(num_steps, dtype=denoise_dtype)``)."""
    step_indices = torch.arange(num_steps, dtype=dtype)
    t = (sigma_max ** (1 / rho) + step_indices / (num_steps - 1) * (sigma_min ** (1 / rho) - sigma_max ** (1 / rho))) ** rho
    return torch.cat([t, torch.zeros_like(t[:1])])


class DiffusionSampler:
    def __init__(self, net):
        self.net = net

    def _module(self):
        return getattr(self.net, "module", self.net)  # net may be DDP (diffusion.py:433)

    def _call(self, x_t, t_scalar: torch.Tensor, condition, auxiliary, alpha: float, beta: float, dtype):
        """alpha * x_t + beta * net(x_t / sigma_d, t, condition, auxiliary) in one fused launch sequence."""
        B = x_t.shape[0]
        dev = x_t.device
        sd = self._module().sigma_data
        tt = torch.full((B,), float(t_scalar), dtype=torch.float32, device=dev)
        a = torch.full((B,), float(alpha), dtype=torch.float32, device=dev)
        b = torch.full((B,), float(beta), dtype=torch.float32, device=dev)
        with engine_for(self._module(), dtype, dev.type):
            return self.net(x_t, tt, condition, auxiliary, x_scale=1.0 / sd, xt=x_t, alpha=a, beta=b)

    @torch.no_grad()
    def scm_solver(self, latents: torch.Tensor, condition=None, auxiliary=None, randn_like: Callable = torch.randn_like,
                   num_steps: int = 2, intermediates: Optional[Sequence[float]] = None, sigma_min: float = 0.002,
                   sigma_max: float = 80.0, denoise_dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """Multistep consistency sampler (diffusion.py:417-461)."""
        sd = self._module().sigma_data
        ts = scm_time_steps(num_steps, sigma_min, sigma_max, sd, intermediates)
        cos, sin = torch.cos(ts), torch.sin(ts)  # fp32, as the reference's device-side torch.cos/sin
        x_t = latents.contiguous().float() if sd == 1.0 else (latents * sd).contiguous().float()
        for i in range(len(ts) - 1):
            if i > 0:
                noise = randn_like(x_t).contiguous()
                x_t = ops.axpby(float(sin[i]) * sd, noise, float(cos[i]), x_t)
            x_t = self._call(x_t, ts[i], condition, auxiliary, float(cos[i]), -float(sin[i]) * sd, denoise_dtype)
        return x_t

    @torch.no_grad()
    def dpm_solver_2s(self, latents: torch.Tensor, condition=None, auxiliary=None, randn_like: Callable = torch.randn_like,
                      num_steps: int = 20, sigma_min: float = 0.002, sigma_max: float = 80.0, S_churn: float = 0.0,
                      S_min: float = 0.0, S_max: float = 1.57, S_noise: float = 1.0,
                      denoise_dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """DPM-Solver++ 2S / Heun on the TrigFlow ODE (diffusion.py:355-415): 2*num_steps-1 network calls."""
        sd = self._module().sigma_data
        ts = torch.cat([_log_sigma_grid(num_steps, sigma_min, sigma_max, sd), torch.zeros(1)])
        x_t = (latents * sd).contiguous().float()
        for k in range(num_steps):
            s, t = ts[k], ts[k + 1]
            dt = float((t - s) * sd)  # fp32 (t - s), then * sigma_d as in "delta * sigma_data * F"
            x_e = self._call(x_t, s, condition, auxiliary, 1.0, dt, denoise_dtype)  # x + delta*sd*F_s
            if k < num_steps - 1:
                # x + delta*sd*0.5*(F_s + F_t) = 0.5*(x + x_e) + 0.5*delta*sd*F_t, with F_t evaluated at x_e
                half = ops.axpby(0.5, x_t, 0.5, x_e)
                B, dev = x_t.shape[0], x_t.device
                tt = torch.full((B,), float(t), dtype=torch.float32, device=dev)
                a = torch.ones(B, dtype=torch.float32, device=dev)
                b = torch.full((B,), 0.5 * dt, dtype=torch.float32, device=dev)
                with engine_for(self._module(), denoise_dtype, dev.type):
                    x_t = self.net(x_e, tt, condition, auxiliary, x_scale=1.0 / sd, xt=half, alpha=a, beta=b)
            else:
                x_t = x_e
        return x_t

    @torch.no_grad()
    def dpm_solver(self, latents: torch.Tensor, condition=None, auxiliary=None, randn_like: Callable = torch.randn_like,
                   num_steps: int = 20, use_pp: bool = True, sigma_min: float = 0.002, sigma_max: float = 80.0, rho: float = 7,
                   denoise_dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """DPM-Solver(++) multistep on the TrigFlow ODE, EDM rho grid (diffusion.py:289-353): num_steps network calls; the
        first and last steps are first-order (DDIM), the others add the 2nd-order correction from the previous prediction."""
        sd = self._module().sigma_data
        ramp = torch.linspace(0, 1, num_steps)
        lo, hi = sigma_min ** (1 / rho), sigma_max ** (1 / rho)
        ts = torch.atan((hi + ramp * (lo - hi)) ** rho / sd)
        ts = torch.cat([ts, torch.zeros_like(ts[:1])])
        logtan = lambda u: torch.log(torch.tan(torch.clamp(u, 1e-4, 1.569)))
        x_t = (latents * sd).contiguous().float()
        t_prev = pred_prev = None
        for k in range(num_steps):
            s, t = ts[k], ts[k + 1]
            delta = s - t
            F = self._call(x_t, s, condition, auxiliary, 0.0, 1.0, denoise_dtype)        # F_s itself
            nxt = ops.axpby(float(torch.cos(delta)), x_t, -float(torch.sin(delta)) * sd, F)
            if use_pp:
                pred, denom = ops.axpby(float(torch.cos(s)), x_t, -float(torch.sin(s)) * sd, F), float(torch.sin(s))
            else:
                pred, denom = ops.axpby(float(torch.sin(s)), x_t, float(torch.cos(s)) * sd, F), float(torch.cos(s))
            if not (k == 0 or k == num_steps - 1):
                r_s = (logtan(s) - logtan(t_prev)) / (logtan(s) - logtan(t))
                coef = float(torch.sin(delta) / (2 * r_s * max(denom, 1e-3)))
                corr = ops.axpby(coef, pred_prev, -coef, pred)
                nxt = ops.axpby(1.0, nxt, 1.0 if use_pp else -1.0, corr)
            t_prev, pred_prev, x_t = s, pred, nxt
        return x_t

    @torch.no_grad()
    def edm_sampler(self, latents: torch.Tensor, condition=None, auxiliary=None, randn_like: Callable = torch.randn_like,
                    num_steps: int = 18, sigma_min: float = 0.002, sigma_max: float = 80, rho: float = 7, S_churn: float = 0,
                    S_min: float = 0, S_max: float = float("inf"), S_noise: float = 1, pipeline_engine: bool = False,
                    denoise_dtype=torch.bfloat16) -> torch.Tensor:
        """EDM stochastic Heun sampler (diffusion.py:10-92, Algorithm 2 of the EDM paper): 2*num_steps-1 network calls.

        The grid, gamma and t_hat are computed as the reference computes them, in ``denoise_dtype`` arithmetic (bf16 under
        the bf16 engine, fp32 for torch.float32 and "bf16x3"), on the host.  The state stays fp32 throughout (the reference
        keeps it in ``denoise_dtype``, i.e. bf16 under the bf16 engine).  Each step maps onto the fused call
        alpha * xt + beta * F(c_in(sigma) x, ln(sigma) / 4) with host scalars, with h = t_next - t_hat and
        c_skip / c_out of the noise level the network sees:
          churn   x_hat = x + sqrt(t_hat^2 - t^2) S_noise eps               (one ``randn_like`` per step, even at gamma = 0)
          Euler   x' = (1 + h (1 - c_skip) / t_hat) x_hat - (h c_out / t_hat) F(x_hat)      (= D at the last step, t_next = 0)
          Heun    x  = [0.5 x_hat + (0.5 + 0.5 h (1 - c_skip') / t_next) x'] - (0.5 h c_out' / t_next) F(x')
        with 1 - c_skip = sigma^2 / (sigma^2 + sd^2) formed directly.  No device-to-host read inside the loop."""
        if pipeline_engine:
            raise NotImplementedError("edm_sampler(pipeline_engine=True) is a placeholder in the reference as well")
        mod = self._module()
        sigma_min = max(sigma_min, mod.sigma_min)
        sigma_max = min(sigma_max, mod.sigma_max)
        gdt = torch.bfloat16 if denoise_dtype == torch.bfloat16 else torch.float32
        ts = edm_time_steps(num_steps, sigma_min, sigma_max, rho, gdt)
        sd = float(mod.sigma_data)
        dev = latents.device
        x = (latents.float() * float(ts[0])).contiguous()

        def call(x_in, sigma, xt, alpha, beta):
            with engine_for(mod, denoise_dtype, dev.type):
                return self.net(x_in, sigma, condition, auxiliary, xt=xt, alpha=alpha, beta=beta)

        for i in range(num_steps):
            t_cur, t_next = ts[i], ts[i + 1]
            gamma = min(S_churn / num_steps, math.sqrt(2) - 1) if bool(S_min <= t_cur <= S_max) else 0
            t_hat = t_cur + gamma * t_cur
            eps = randn_like(x)  # (drawn at gamma = 0 too: the noise streams stay aligned with the reference's)
            c = float((t_hat ** 2 - t_cur ** 2).sqrt()) * S_noise
            x_hat = ops.axpby(1.0, x, c, eps.contiguous().float()) if c != 0.0 else x
            th, tn, h = float(t_hat), float(t_next), float(t_next - t_hat)
            s2 = th * th + sd * sd
            a = 1.0 + h * (th * th / s2) / th
            b = -h * (th * sd / math.sqrt(s2)) / th
            x_e = call(x_hat, th, x_hat, a, b)  # Euler step
            if i < num_steps - 1:
                s2n = tn * tn + sd * sd
                half = ops.axpby(0.5, x_hat, 0.5 + 0.5 * h * (tn * tn / s2n) / tn, x_e)
                x = call(x_e, tn, half, 1.0, -0.5 * h * (tn * sd / math.sqrt(s2n)) / tn)  # 2nd-order correction
            else:
                x = x_e
        return x
