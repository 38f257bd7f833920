"""TEST INFRASTRUCTURE: plain PyTorch-CPU restatements of the tangent-pass and training-glue operations whose kernels
tests/test_gpu_tangent_kernels.py checks one by one.

  * ``modnorm_tangent``        -- ModulatedNorm + residual and its tangent (include/swiftk.h: swiftk_modnorm_jvp), fp64, with a
                                  keyword that leaves out one named term of the tangent
  * ``modnorm_tangent_fp32``   -- the same formula in fp32, two-pass and in the one-pass shifted form of the 32-rows-per-block
                                  pair kernel: the yardstick of the GPU tolerances (a restatement of the mathematics)
  * ``pair_quantise``          -- the value a (bf16 hi, 8-bit lo) pair holds for an fp32 value (csrc/common.h: lo8_insert)
  * ``qknorm_tangent``, ``swiglu_tangent`` -- swiftk_qknorm_jvp / swiftk_swiglu_jvp standing alone, with their input builders
  * ``silu_tangent`` / ``silu_grad``, ``timestep_embed_tangent``, ``scm_target``, ``rmse_sums`` -- small closed forms
  * ``make_norm_case``         -- seeded inputs of the norm tests with four hostile rows

tests/test_tangent_reference_cpu.py pins every one of them to ``torch.func.jvp`` / autograd of the oracle's own expressions, and
asserts that each additive term of the tangent is a visible share of the whole on these inputs.
"""
from __future__ import annotations

import math

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


LN100 = math.log(100.0)
QKNORM_JVP_CASES = ((3, 3, 80), (3, 3, 88), (3, 3, 96), (129, 12, 88))   # (M, heads, head_dim): 18 vectors (one ragged block), 3096 (193.5)


def qknorm_tangent(qkv, dqkv, scale, heads, hd, dtype=torch.float64):
    """What swiftk_qknorm_jvp leaves for qkv, dqkv [M, heads * 3 * hd] (columns head-major, then q | k | v):
    x-hat = tau x / n,  d x-hat = tau / n (dx - x (x . dx) / n^2),  n = max(|x|, 1e-12),  tau = exp(min(scale_h, ln 100)) for q and 1
    for k; v and dv pass through.  Returns (qkvh, dqkvh [M, heads, 3, hd], rn [M, heads, 3] = 1 / n, 1 for v)."""
    M = qkv.shape[0]
    x, dx = qkv.to(dtype).view(M, heads, 3, hd), dqkv.to(dtype).view(M, heads, 3, hd)
    n = x.norm(dim=-1).clamp_min(1e-12)
    n[:, :, 2] = 1.0
    f = 1.0 / n
    f[:, :, 0] = f[:, :, 0] * scale.to(dtype).clamp(max=LN100).exp().view(1, heads)
    c = (x * dx).sum(-1) / (n * n)
    c[:, :, 2] = 0.0
    return f[..., None] * x, f[..., None] * (dx - x * c[..., None]), 1.0 / n


def qknorm_jvp_inputs(M, heads, hd, seed):
    """fp32 (qkv, dqkv [M, 3 heads hd], scale [heads]): qkv = 0.7 randn, dqkv = randn; the last head's scale is ln 200 (clamped at
    ln 100), head 0's ln 10; two all-zero primal vectors with their tangents left nonzero -- q of head 0 in the last row (tangent
    tau dq 1e12) and k of the last head in row 0 (tangent dk 1e12)."""
    g = torch.Generator().manual_seed(seed)
    qkv, dqkv = 0.7 * torch.randn(M, 3 * heads * hd, generator=g), torch.randn(M, 3 * heads * hd, generator=g)
    base = torch.log(torch.tensor([10.0, 3.0, 30.0, 60.0, 1.0, 99.0, 50.0, 20.0, 15.0, 5.0, 47.0, 200.0]))
    scale = base[:heads].clone()
    scale[heads - 1] = math.log(200.0)
    v = qkv.view(M, heads, 3, hd)
    v[M - 1, 0, 0] = 0.0
    v[0, heads - 1, 1] = 0.0
    return qkv, dqkv, scale


def zero_vectors(M, heads):
    """(row, head, part) of the all-zero vectors qknorm_jvp_inputs plants."""
    return ((M - 1, 0, 0), (0, heads - 1, 1))


def swiglu_tangent(h, dh, dtype=torch.float64):
    """SwiGLU and its tangent on interleaved (gate_j, up_j) columns, in ``dtype`` (fp32: torch's own evaluation of the kernel's
    formulas in the kernel's order): s = 1 / (1 + exp(-g)), out = g s u, d out = (s + g s (1 - s)) dg u + g s du.
    Returns (out, d out, scale of out, scale of d out): the sums of the absolute terms an evaluation adds up --
    |g s u| and (|s| + |g s (1 - s)|) |dg u| + |g s du| (the factor s + g s (1 - s) vanishes at g = -1.2784645)."""
    h, dh = h.to(dtype), dh.to(dtype)
    g, u, dg, du = h[:, 0::2], h[:, 1::2], dh[:, 0::2], dh[:, 1::2]
    s = 1.0 / (1.0 + torch.exp(-g))
    out = g * s * u
    dout = (s + g * s * (1.0 - s)) * dg * u + g * s * du
    return out, dout, out.abs(), (s.abs() + (g * s * (1.0 - s)).abs()) * (dg * u).abs() + (g * s * du).abs()


def bf16_round_once(v64: torch.Tensor) -> torch.Tensor:
    """fp64 -> the nearest bf16 value (ties to even) in ONE rounding, returned as fp64.  The usual route fp64 -> fp32 -> bf16 rounds
    twice: with bf16 operands an exact result often lies within 2^-24 of a bf16 tie, the fp32 step lands on the tie, and the second
    rounding then goes to the even neighbour instead of the nearer one."""
    v = v64.double()
    e = torch.frexp(v.abs().clamp_min(2.0 ** -126))[1] - 1                # floor(log2 |v|)
    q = torch.ldexp(v, 7 - e)                                             # exact: |q| in [128, 256)
    return torch.ldexp(torch.round(q), e - 7)                             # torch.round: halves to even


def bf16_score_once(got: torch.Tensor, ref64: torch.Tensor):
    """(worst |got - bf16(ref)| in bf16 ulps of bf16(ref), share of elements that differ from it), bf16(ref) rounded once."""
    want = bf16_round_once(ref64)
    e = torch.frexp(want.abs().clamp_min(2.0 ** -126))[1] - 1
    ulp = torch.ldexp(torch.ones_like(want), e - 7)
    return float(((got.double() - want).abs() / ulp).max()), float((got.double() != want).double().mean())


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
