"""TEST INFRASTRUCTURE: plain PyTorch-CPU restatements of the tangent-pass and training-glue operations whose kernels
tests/test_gpu_tangent_kernels.py checks one by one.

  * ``modnorm_tangent``        -- ModulatedNorm + residual and its tangent (include/swiftk.h: swiftk_modnorm_jvp), fp64, with a
                                  keyword that leaves out one named term of the tangent
  * ``modnorm_tangent_fp32``   -- the same formula in fp32, two-pass and in the one-pass shifted form of the 32-rows-per-block
                                  pair kernel: the yardstick of the GPU tolerances (a restatement of the mathematics)
  * ``pair_quantise``          -- the value a (bf16 hi, 8-bit lo) pair holds for an fp32 value (csrc/common.h: lo8_insert)
  * ``silu_tangent`` / ``silu_grad``, ``timestep_embed_tangent``, ``scm_target``, ``rmse_sums`` -- small closed forms
  * ``make_norm_case``         -- seeded inputs of the norm tests with four hostile rows

tests/test_tangent_reference_cpu.py pins every one of them to ``torch.func.jvp`` / autograd of the oracle's own expressions, and
asserts that each additive term of the tangent is a visible share of the whole on these inputs.
"""
from __future__ import annotations

import torch

TERMS = ("mean_dy", "n_mean_ndy", "dsc", "dsh", "gamma_dn")
HOSTILE_ROWS = 4  # rows 0..3 of the first sample


def bf16_round(v: torch.Tensor) -> torch.Tensor:
    return v.to(torch.bfloat16).to(v.dtype)


def _per_row(m: torch.Tensor, rows_per_sample: int) -> torch.Tensor:
    return m.repeat_interleave(rows_per_sample, 0)


def modnorm_tangent(y, dy, x, dx, gamma, beta, mod, dmod, rows_per_sample, eps=1e-6, drop=None, dtype=torch.float64):
    """x += LN(y)(1+sc)+sh;  dx += gamma dn (1+sc) + LN(y) dsc + dsh,  dn = (dy - mean(dy) - n mean(n dy)) rstd.
    y, dy, x, dx [M, d]; mod = (sc | sh), dmod = (dsc | dsh) [B, 2d]; sample b owns rows b rps .. (b+1) rps - 1.
    ``drop``: one of TERMS, left out of the tangent (the sensitivity condition of the tests)."""
    assert drop is None or drop in TERMS
    y, dy, x, dx, gamma, beta, mod, dmod = (v.to(dtype) for v in (y, dy, x, dx, gamma, beta, mod, dmod))
    d = y.shape[1]
    sc, sh = _per_row(mod[:, :d], rows_per_sample), _per_row(mod[:, d:2 * d], rows_per_sample)
    dsc, dsh = _per_row(dmod[:, :d], rows_per_sample), _per_row(dmod[:, d:2 * d], rows_per_sample)
    mu = y.mean(1, keepdim=True)
    c = y - mu
    rstd = 1.0 / torch.sqrt((c * c).mean(1, keepdim=True) + eps)
    n = c * rstd
    t = dy
    if drop != "mean_dy":
        t = t - dy.mean(1, keepdim=True)
    if drop != "n_mean_ndy":
        t = t - n * (n * dy).mean(1, keepdim=True)
    dn = t * rstd
    ln = n * gamma + beta
    x_new = x + ln * (1 + sc) + sh
    dx_new = dx.clone()
    if drop != "gamma_dn":
        dx_new = dx_new + gamma * dn * (1 + sc)
    if drop != "dsc":
        dx_new = dx_new + ln * dsc
    if drop != "dsh":
        dx_new = dx_new + dsh
    return x_new, dx_new


def modnorm_tangent_fp32(y, dy, x, dx, gamma, beta, mod, dmod, rows_per_sample, eps=1e-6, one_pass=False):
    """The same in fp32 arithmetic.  ``one_pass``: the statistics from the four sums of t = y - y[:, 0] (sum t, sum t^2,
    sum dy, sum t dy) and the per-column constants A = gamma (1+sc), B = beta (1+sc) + sh, C = gamma dsc, D = beta dsc + dsh,
    as the 32-rows-per-block pair kernel forms them; otherwise mean, then centred variance, then mean(n dy)."""
    f = torch.float32
    if not one_pass:
        return modnorm_tangent(y, dy, x, dx, gamma, beta, mod, dmod, rows_per_sample, eps, dtype=f)
    y, dy, x, dx, gamma, beta, mod, dmod = (v.to(f) for v in (y, dy, x, dx, gamma, beta, mod, dmod))
    d = y.shape[1]
    sc1 = 1.0 + mod[:, :d]
    A, Bc = _per_row(gamma * sc1, rows_per_sample), _per_row(beta * sc1 + mod[:, d:2 * d], rows_per_sample)
    C, D = _per_row(gamma * dmod[:, :d], rows_per_sample), _per_row(beta * dmod[:, :d] + dmod[:, d:2 * d], rows_per_sample)
    inv_d = torch.tensor(1.0 / d, dtype=f)
    t = y - y[:, :1]
    q1, q2 = t.sum(1, keepdim=True), (t * t).sum(1, keepdim=True)
    q3, q4 = dy.sum(1, keepdim=True), (t * dy).sum(1, keepdim=True)
    mt = q1 * inv_d
    rstd = 1.0 / torch.sqrt((q2 * inv_d - mt * mt).clamp_min(0.0) + eps)
    mdy, mndy = q3 * inv_d, rstd * (q4 - mt * q3) * inv_d
    n = (t - mt) * rstd
    dn = (dy - mdy - n * mndy) * rstd
    return x + (n * A + Bc), dx + (dn * A + (n * C + D))


def pair_quantise(v: torch.Tensor, parts: bool = False):
    """The fp32 value a (bf16 hi, 8-bit lo) pair holds for fp32 ``v``: hi = bf16(v), byte = round((v - hi) 2^(142 - E)) + 128
    saturated to [0, 255] (E = hi's biased exponent, ulp(hi) / 256 = 2^(E - 142)), value = hi + (byte - 128) 2^(E - 142).
    ``parts``: also return (hi, byte)."""
    v = v.to(torch.float32)
    hi = v.to(torch.bfloat16)
    E = (hi.contiguous().view(torch.int16).to(torch.int32) >> 7) & 0xFF
    # (the scalings in fp64, where 2^(+-142) is an ordinary number: every product below is exact, as ldexpf's is)
    byte = (torch.ldexp((v - hi.float()).double(), 142 - E) + 128.0).round().clamp(0.0, 255.0)  # (ties to even, as the convert)
    val = (hi.double() + torch.ldexp(byte - 128.0, E - 142)).float()
    return (val, hi, byte.to(torch.uint8)) if parts else val


def silu_grad(z: torch.Tensor) -> torch.Tensor:
    """d silu(z) / dz = s + z s (1 - s), s = sigmoid(z); fp64."""
    z = z.double()
    s = torch.sigmoid(z)
    return s + z * s * (1 - s)


def silu_tangent(z: torch.Tensor, dz: torch.Tensor):
    """(silu(z), silu'(z) dz) in fp64."""
    z = z.double()
    return z * torch.sigmoid(z), silu_grad(z) * dz.double()


def timestep_embed_tangent(t, dt, freqs, d: int, timestep_weight: float = 1.0, dtype=torch.float64):
    """d/dt of [sin | cos](t w f) along dt: [cos | -sin](t w f) * w f * dt, [B, d]; zero in the last column when d is odd.
    ``dtype`` float32 evaluates the same expression in fp32 (the argument t w f is rounded before cos / sin see it)."""
    t, dt, freqs = t.to(dtype), dt.to(dtype), freqs.to(dtype)
    half = d // 2
    w = torch.tensor(timestep_weight, dtype=dtype)
    arg = (t[:, None] * w) * freqs[None, :half]
    out = torch.zeros(t.shape[0], d, dtype=dtype)
    fac = (w * freqs[None, :half]) * dt[:, None]
    out[:, :half] = torch.cos(arg) * fac
    out[:, half:2 * half] = -torch.sin(arg) * fac
    return out


def scm_target(F, dxt, xt_over_sd, dF, t, r: float, sigma_data: float):
    """g = -cos^2 t (sd F - dxt) - r (cos t sin t x_t + sd dF), x_t = xt_over_sd sd;  target = F + g / (rms_b(g) + 0.1).
    All [B, per_sample], t [B]; fp64.  Returns (target, g)."""
    F, dxt, xt_over_sd, dF, t = (v.double() for v in (F, dxt, xt_over_sd, dF, t))
    c, s = torch.cos(t)[:, None], torch.sin(t)[:, None]
    g = -(c * c) * (sigma_data * F - dxt) - r * ((c * s) * (xt_over_sd * sigma_data) + sigma_data * dF)
    rms = g.square().mean(1, keepdim=True).sqrt()
    return F + g / (rms + 0.1), g


def rmse_sums(y, t, w_lat):
    """sq[0] = sum (y - t)^2 over everything, sq[1 + c] = sum_{b,h,w} w_lat[h] (y - t)^2; y, t [B, C, H, W]; fp64 [1 + C]."""
    e2 = (y.double() - t.double()).square()
    return torch.cat([e2.sum().reshape(1), (e2 * w_lat.double()[None, None, :, None]).sum(dim=(0, 2, 3))])


def make_norm_case(d: int, rows_per_sample: int, B: int, seed: int, bf16_rows: bool = True) -> dict:
    """Inputs of the ModulatedNorm tangent tests (fp32 CPU tensors): y = 2 randn + 0.5, dy = 0.7 randn + 0.3, both rounded to
    bf16 (``bf16_rows`` False: the benign rows keep their fp32 values); x / dx of std 1 / 0.5; gamma = 1 + 0.1 randn,
    beta = 0.1 randn; mod = 0.3 randn, dmod = 0.2 randn, [B, 2d].  Rows 0..3 of the first sample are hostile:
      0: element 0 = 300 (an outlier in the element the one-pass form shifts by)
      1: 40 + 0.01 randn (bf16 spacing at 40 is 0.25: a constant row after rounding, variance 0, rstd = 1 / sqrt(eps))
      2: zero except one element 1e-3
      3: element 7 = -500 (an outlier elsewhere)."""
    assert rows_per_sample >= HOSTILE_ROWS and d >= 8
    g = torch.Generator().manual_seed(seed)
    rn = lambda *shape: torch.randn(*shape, generator=g)
    M = B * rows_per_sample
    y, dy = 2.0 * rn(M, d) + 0.5, 0.7 * rn(M, d) + 0.3
    x, dx = rn(M, d), 0.5 * rn(M, d)
    gamma, beta = 1.0 + 0.1 * rn(d), 0.1 * rn(d)
    mod, dmod = 0.3 * rn(B, 2 * d), 0.2 * rn(B, 2 * d)
    r1 = 40.0 + 0.01 * rn(d)
    yb, dyb = bf16_round(y), bf16_round(dy)
    if bf16_rows:
        y, dy = yb, dyb
    else:
        y[:HOSTILE_ROWS], dy[:HOSTILE_ROWS] = yb[:HOSTILE_ROWS], dyb[:HOSTILE_ROWS]
    y[0, 0] = 300.0
    y[1] = bf16_round(r1)
    y[2] = 0.0
    y[2, 5] = bf16_round(torch.tensor(1e-3))
    y[3, 7] = -500.0
    return dict(y=y, dy=dy, x=x, dx=dx, gamma=gamma, beta=beta, mod=mod, dmod=dmod, rows_per_sample=rows_per_sample)


def benign(v: torch.Tensor) -> torch.Tensor:
    """The rows of a [M, d] tensor that make_norm_case left benign."""
    return v[HOSTILE_ROWS:]


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def row_err(a: torch.Tensor, b: torch.Tensor) -> float:
    """max|a - b| / max|b| of one row (the score of a hostile row)."""
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
