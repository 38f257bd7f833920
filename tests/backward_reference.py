"""TEST INFRASTRUCTURE: plain PyTorch-CPU closed forms (fp64 unless ``dtype`` says otherwise) of the training backward and loss
kernels of swift_amd/csrc/train_kernels.hip.  Each takes exactly the arrays its kernel is given -- for ``qknorm_bwd`` the
normalised ``qkvh``, its gradient and the saved ``rn``, not the raw projection -- so that a comparison measures the kernel's own
error and nothing upstream of it.

  * ``swiglu_fwd`` / ``swiglu_bwd``   -- h [M, 2 mlp] with (gate_j, up_j) interleaved; the backward also returns the scales the
                                         errors are measured against (|d u| for dgate: the factor s + g s (1 - s) vanishes at g = -1.2784645)
  * ``qknorm_bwd``                    -- backward of the cosine-attention prologue, per (row, head, q | k | v) vector
  * ``modnorm_bwd`` / ``modnorm_bwd_fp32`` -- ModulatedNorm backward; the fp32 restatement in the two-pass form of the row kernel
                                         and in the one-pass form (shifted by the row's first element) of the one-kernel form
  * ``crps``, ``trigflow_prep``, ``trigflow_loss``, ``edm_prep``, ``edm_loss`` -- losses with their gradients
  * ``ensemble_sums``                 -- the four latitude-weighted sums per (sample, variable)
  * ``adam_ema_step``                 -- nan_to_num, Adam / AdamW and the EMA lerp on one tensor
  * ``condition``                     -- sum|term| / |sum term|
  * input builders shared by tests/test_backward_reference_cpu.py and tests/test_gpu_backward_kernels.py

tests/test_backward_reference_cpu.py pins every closed form to autograd of the oracle's own expressions.
"""
from __future__ import annotations

import math

import torch

LN100 = math.log(100.0)
PLANTED_GATES = (-100.0, -30.0, -1.2784645, 0.0, 30.0, 100.0)
F64 = torch.float64


def rnd(shape, seed, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * std


def condition(terms: torch.Tensor, dim=None) -> torch.Tensor:
    """sum|term| / |sum term| (over ``dim``, or everything)."""
    t = terms.double()
    if dim is None:
        return t.abs().sum() / t.sum().abs().clamp_min(1e-300)
    return t.abs().sum(dim) / t.sum(dim).abs().clamp_min(1e-300)


# ------------------------------------------------------------------------------------------ SwiGLU

def swiglu_fwd(h, dtype=F64):
    h = h.to(dtype)
    g, u = h[:, 0::2], h[:, 1::2]
    return g * torch.sigmoid(g) * u


def swiglu_bwd(h, d, dtype=F64):
    """(dgate, dup, |d u|, |d g s|): dh[:, 2j] = d u (s + g s (1 - s)), dh[:, 2j+1] = d g s, s = sigmoid(gate)."""
    h, d = h.to(dtype), d.to(dtype)
    g, u = h[:, 0::2], h[:, 1::2]
    s = torch.sigmoid(g)
    return d * u * (s + g * s * (1 - s)), d * g * s, (d * u).abs(), (d * g * s).abs()


def swiglu_inputs(M, mlp, seed):
    """fp32 h [M, 2 mlp] (gates 2 randn, ups randn; the last row's first gates are PLANTED_GATES) and d [M, mlp]."""
    h, d = rnd((M, 2 * mlp), seed), rnd((M, mlp), seed + 1)
    h[:, 0::2] *= 2.0
    k = min(len(PLANTED_GATES), mlp)
    h[M - 1, 0:2 * k:2] = torch.tensor(PLANTED_GATES[:k])
    return h, d


def bf16_ulp(v: torch.Tensor) -> torch.Tensor:
    """The spacing of bf16 numbers at |v| (v holds bf16 values; 2^-133 below the normal range)."""
    e = torch.frexp(v.double().abs().clamp_min(2.0 ** -126))[1] - 1
    return torch.ldexp(torch.ones_like(v, dtype=F64), e - 7)


def bf16_score(got: torch.Tensor, ref64: torch.Tensor):
    """(worst |got - bf16(ref)| in ulps of bf16(ref), share of elements that differ from bf16(ref) at all)."""
    want = ref64.float().bfloat16()  # (fp64 -> fp32 -> bf16: a double rounding only within 2^-29 of a tie)
    diff = (got.double() - want.double()).abs()
    return float((diff / bf16_ulp(want)).max()), float((got.double() != want.double()).double().mean())


# ------------------------------------------------------------------------------------------ QK-norm backward

def prenorm_fwd(raw, scale, heads, hd):
    """What SWIFTK_EPI_QKNORM stores for raw [M, heads * 3 * hd] (columns head-major, then q | k | v): (qkvh, rn [M, 3 heads])."""
    M = raw.shape[0]
    v = raw.double().view(M, heads, 3, hd)
    rn = 1.0 / v.norm(dim=-1).clamp_min(1e-12)
    rn[:, :, 2] = 1.0
    tau = scale.double().clamp(max=LN100).exp().view(1, heads)
    out = v * rn[..., None]
    out[:, :, 0] = out[:, :, 0] * tau[..., None]
    return out.reshape(M, -1), rn.reshape(M, -1)


def qknorm_bwd(qkvh, dqkvh, rn, scale, heads, hd):
    """dq = tau rn (dqh - u (u . dqh)), u = qh / tau;  dk = rn (dkh - kh (kh . dkh));  dv = dvh;
    dscale_h = tau sum_tokens (u . dqh) below the clamp at ln 100, 0 at and above it.
    Returns (dqkv [M, 3 heads hd], dscale [heads], sum_tokens |tau u . dqh| [heads])."""
    M = qkvh.shape[0]
    a, d = qkvh.double().view(M, heads, 3, hd), dqkvh.double().view(M, heads, 3, hd)
    r = rn.double().view(M, heads, 3)
    s = scale.double()
    tau = s.clamp(max=LN100).exp().view(1, heads)
    out = d.clone()
    u = a[:, :, 0] / tau[..., None]
    dot = (u * d[:, :, 0]).sum(-1)
    out[:, :, 0] = (tau * r[:, :, 0])[..., None] * (d[:, :, 0] - u * dot[..., None])
    k = a[:, :, 1]
    out[:, :, 1] = r[:, :, 1][..., None] * (d[:, :, 1] - k * (k * d[:, :, 1]).sum(-1, keepdim=True))
    terms = tau * dot
    live = (s < LN100).double()
    return out.reshape(M, -1), terms.sum(0) * live, terms.abs().sum(0)


QKNORM_SHAPES = ((12, 88, torch.bfloat16), (16, 80, torch.bfloat16), (4, 96, torch.bfloat16), (2, 64, torch.bfloat16), (2, 64, torch.float32))
QKNORM_ROWS = (1, 5, 512)
QKNORM_LONG = (8192, 12, 88, torch.bfloat16)  # 294,912 vectors: the grid-stride loop's second trip, filled to one eighth


def qknorm_cases():
    """(M, heads, head_dim, dtype, seed) of every QK-norm backward case."""
    out = [(M, h, hd, dt, 300 + 10 * i + j) for i, (h, hd, dt) in enumerate(QKNORM_SHAPES) for j, M in enumerate(QKNORM_ROWS)]
    return out + [(*QKNORM_LONG, 399)]


def qknorm_inputs(M, heads, hd, seed, dt):
    """(qkvh, dqkvh, rn, scale) as the kernel gets them: the forward of a random projection, stored in ``dt``; the gradient in
    ``dt`` (randn + 2 x the vector's own direction, so that the per-head sums behind dscale do not cancel); rn fp32; scale
    with heads below, at (head 1) and above (the last head) ln 100."""
    raw, dq = rnd((M, 3 * heads * hd), seed, 0.7), rnd((M, 3 * heads * hd), seed + 1)
    rv = raw.view(M, 3 * heads, hd)
    dq = (dq.view(M, 3 * heads, hd) + 2.0 * rv / rv.norm(dim=-1, keepdim=True)).reshape(M, -1)
    base = torch.log(torch.tensor([10.0, 3.0, 30.0, 200.0, 1.0, 10.0, 50.0, 99.0, 101.0, 5.0, 20.0, 10.0, 7.0, 2.0, 60.0, 40.0]))
    scale = base[:heads].clone().float()
    at = torch.tensor(4.605170185988092, dtype=torch.float32)  # the kernel's own constant
    if heads > 2:
        scale[1], scale[heads - 1] = at, math.log(200.0)
    else:  # two heads: head 0 below, head 1 at (even seeds) or above (odd seeds)
        scale[1] = math.log(200.0) if seed % 2 else at
    qkvh, rn = prenorm_fwd(raw, scale, heads, hd)
    return qkvh.float().to(dt), dq.to(dt), rn.float(), scale


# ------------------------------------------------------------------------------------------ ModulatedNorm backward

MODNORM_HOSTILE = 4  # rows 0..3 of the first sample (row 4 of g is zero)


def _per_row(m, rps):
    return m.repeat_interleave(rps, 0)


def modnorm_bwd(y, g, gamma, beta, mod, rps, eps=1e-6):
    """out = LN(y; gamma, beta) (1 + sc_b) + sh_b with upstream g.  Returns dict: dy [M, d], dgamma, dbeta [d], dmod [B, 2d] and the
    sums of absolute terms behind each column sum (agamma, abeta, amod)."""
    y, g, gamma, beta, mod = (v.double() for v in (y, g, gamma, beta, mod))
    M, d = y.shape
    B = M // rps
    sc1 = 1.0 + _per_row(mod[:, :d], rps)
    c = y - y.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt((c * c).mean(1, keepdim=True) + eps)
    n = c * rstd
    dn = g * sc1 * gamma
    dy = rstd * (dn - dn.mean(1, keepdim=True) - n * (dn * n).mean(1, keepdim=True))
    tg, tb = g * sc1 * n, g * sc1
    ts, th = (g * (n * gamma + beta)).view(B, rps, d), g.view(B, rps, d)
    return dict(dy=dy, dgamma=tg.sum(0), dbeta=tb.sum(0), dmod=torch.cat([ts.sum(1), th.sum(1)], 1),
                agamma=tg.abs().sum(0), abeta=tb.abs().sum(0), amod=torch.cat([ts.abs().sum(1), th.abs().sum(1)], 1))


def modnorm_bwd_fp32(y, g, gamma, mod, rps, eps=1e-6, one_pass=False):
    """dy in fp32 arithmetic.  ``one_pass``: from the four sums of t = y - y[:, 0] (sum t, sum t^2, sum dn, sum dn t), as the
    one-kernel form; otherwise the mean of t, the centred variance, then the two means (the row kernel of the two-kernel form)."""
    f = torch.float32
    y, g, gamma, mod = (v.to(f) for v in (y, g, gamma, mod))
    d = y.shape[1]
    w = _per_row((1.0 + mod[:, :d]) * gamma, rps)
    dn = g * w
    inv_d = torch.tensor(1.0 / d, dtype=f)
    epsf = torch.tensor(eps, dtype=f)
    if one_pass:
        t = y - y[:, :1]
        q1, q2 = t.sum(1, keepdim=True), (t * t).sum(1, keepdim=True)
        q3, q4 = dn.sum(1, keepdim=True), (dn * t).sum(1, keepdim=True)
        mt = q1 * inv_d
        rstd = 1.0 / torch.sqrt((q2 * inv_d - mt * mt).clamp_min(0.0) + epsf)
        s1, s2 = q3 * inv_d, rstd * (q4 - mt * q3) * inv_d
        n = (t - mt) * rstd
    else:
        t = y - y[:, :1]
        c = t - t.sum(1, keepdim=True) * inv_d
        rstd = 1.0 / torch.sqrt((c * c).sum(1, keepdim=True) * inv_d + epsf)
        n = c * rstd
        s1, s2 = dn.sum(1, keepdim=True) * inv_d, (dn * n).sum(1, keepdim=True) * inv_d
    return rstd * (dn - s1 - n * s2)


def modnorm_inputs(d, rps, B, seed, bf16, offset_row=False):
    """fp32 CPU inputs: y = 2 randn + 0.3 (bf16 values when ``bf16``), g randn, gamma = 1 + 0.1 randn, beta = 0.1 randn,
    mod = 0.3 randn [B, 2d].  Planted in the first sample: row 0 constant; row 1 with its first element 1000 x the spread of
    the rest; row 2 (``offset_row``: fp32 only) a common offset 300 with spread 0.02; row 3 an outlier away from element 0;
    row 4 of g all zero."""
    assert rps >= 8
    M = B * rps
    y, g = 2.0 * rnd((M, d), seed) + 0.3, rnd((M, d), seed + 1)
    gamma, beta = 1.0 + 0.1 * rnd((d,), seed + 2), 0.1 * rnd((d,), seed + 3)
    mod = 0.3 * rnd((B, 2 * d), seed + 4)
    y[0] = 1.75
    y[1, 0] = 2000.0
    if offset_row:
        y[2] = 300.0 + 0.02 * rnd((d,), seed + 5)
    y[3, min(7, d - 1)] = -500.0
    g[4] = 0.0
    if bf16:
        y = y.bfloat16().float()
    return y, g, gamma, beta, mod


def row_rel_l2(got, ref):
    """Per row |got - ref| / |ref| (rows of ref that are all zero: inf unless got is all zero too)."""
    got, ref = got.double(), ref.double()
    num, den = (got - ref).norm(dim=-1), ref.norm(dim=-1)
    return torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num > 0, torch.full_like(num, float("inf")), torch.zeros_like(num)))


# ------------------------------------------------------------------------------------------ losses

def _w(w_var, w_lat):
    return w_var.double().view(1, -1, 1, 1) * w_lat.double().view(1, 1, -1, 1)


def crps(preds, target, w_var, w_lat, alpha, gscale=1.0):
    """loss = 1/(B H W) sum w (mean_i |x_i - y| - cs sum_{i != j} |x_i - x_j|), cs = (1 - (1 - alpha)/m) / (2 m (m - 1));
    preds [m, B, C, H, W].  Returns (loss, gscale dloss/dpreds, the per-element scale gscale w / (B H W) of a gradient element);
    sign(0) = 0, as torch's abs."""
    x, y = preds.double(), target.double()
    m, B, C, H, W = x.shape
    w = _w(w_var, w_lat)
    cs = (1.0 - (1.0 - alpha) / m) / (2.0 * m * (m - 1))
    inv = 1.0 / (B * H * W)
    skill = (x - y).abs().sum(0) / m
    spread = torch.zeros_like(y)
    ga = torch.zeros_like(x)
    for a in range(m):
        for b in range(m):
            spread += (x[a] - x[b]).abs()
            ga[a] += torch.sign(x[a] - x[b])
    loss = inv * (w * (skill - cs * spread)).sum()
    dp = gscale * inv * w * (torch.sign(x - y) / m - 2.0 * cs * ga)
    return loss, dp, (gscale * inv * w).expand_as(y)


def trigflow_prep(x, z, t, sd):
    """(x_t / sd, v_t): x_t = cos t x + sin t sd z,  v_t = cos t sd z - sin t x;  t [B]."""
    x, z = x.double(), z.double() * sd
    c, s = torch.cos(t.double()).view(-1, 1, 1, 1), torch.sin(t.double()).view(-1, 1, 1, 1)
    return (c * x + s * z) / sd, c * z - s * x


def trigflow_loss(F, vt, logvar, w_var, w_lat, sd, gscale=1.0):
    """loss = 1/(B H W) sum [exp(-lv_b) w (sd F - v)^2 + lv_b].  Returns dict(loss, dF, dlogvar [B], terms [B, per_sample] of
    dlogvar, wr = the scale gscale 2 sd exp(-lv) w (|sd F| + |v|) / (B H W) of a dF element: the operands of its one subtraction)."""
    F, vt = F.double(), vt.double()
    B, C, H, W = F.shape
    lv = torch.zeros(B, dtype=F64) if logvar is None else logvar.double()
    iv = torch.exp(-lv).view(B, 1, 1, 1)
    w = _w(w_var, w_lat)
    inv = 1.0 / (B * H * W)
    r = sd * F - vt
    loss = inv * (iv * w * r * r + lv.view(B, 1, 1, 1)).sum()
    dF = gscale * inv * 2.0 * sd * iv * w * r
    terms = (gscale * inv * (1.0 - iv * w * r * r)).reshape(B, -1)
    return dict(loss=loss, dF=dF, dlogvar=terms.sum(1), terms=terms, wr=gscale * inv * 2.0 * sd * iv * w * ((sd * F).abs() + vt.abs()))


def edm_prep(x, z, sigma, sd):
    """c_in (x + sigma z), c_in = 1 / sqrt(sigma^2 + sd^2);  sigma [B]."""
    sg = sigma.double().view(-1, 1, 1, 1)
    return (x.double() + sg * z.double()) / torch.sqrt(sg * sg + sd * sd)


def edm_loss(F, x, z, sigma, w_var, w_lat, sd, gscale=1.0):
    """loss = 1/(B H W) sum lambda_b w (D - x)^2, D = c_skip (x + sigma z) + c_out F.  Returns (loss, dF, the scale
    gscale 2 w lambda c_out (|c_out F| + |c_skip sigma z| + |(1 - c_skip) x|) / (B H W) of a dF element)."""
    F, x, z = F.double(), x.double(), z.double()
    B, C, H, W = F.shape
    sg = sigma.double().view(B, 1, 1, 1)
    s2 = sg * sg + sd * sd
    c_skip, c_out = sd * sd / s2, sg * sd / torch.sqrt(s2)
    lam = s2 / (sg * sd) ** 2
    w = _w(w_var, w_lat)
    inv = 1.0 / (B * H * W)
    r = c_skip * (x + sg * z) + c_out * F - x
    loss = inv * (lam * w * r * r).sum()
    k = gscale * inv * 2.0 * lam * w * c_out
    return loss, k * r, k * ((c_out * F).abs() + (c_skip * sg * z).abs() + ((1 - c_skip) * x).abs())


def loss_weights(C, H, seed):
    from oracle import loss as oloss
    g = torch.Generator().manual_seed(seed)
    return torch.rand(C, generator=g) + 0.1, oloss.latitude_weights(H).reshape(-1)


SHAPE_SMALL = (3, 5, 7, 11)        # distinct odd extents
SHAPE_PAST_CAP = (4, 69, 64, 64)   # 1,130,496 elements: past the 4096 x 256 grid cap, ragged second trip
SHAPE_WORKLOAD = (2, 69, 128, 256) # the workload's 2,260,992 elements per sample
SD = 0.8


def trigflow_inputs(shape, seed):
    """fp32 dict: x, z, t [B], the closed-form (xt, vt) rounded to fp32, F = (vt + 0.7 randn) / SD (residual of std 0.7: the terms
    1 - exp(-lv) w r^2 behind dlogvar keep one sign mostly), logvar, w_var, w_lat."""
    B, C, H, W = shape
    x, z = rnd(shape, seed), rnd(shape, seed + 1)
    t = torch.linspace(0.4, 1.3, B)
    lv = torch.linspace(0.2, -0.3, B)
    xt, vt = (v.float() for v in trigflow_prep(x, z, t, SD))
    F = (vt + 0.7 * rnd(shape, seed + 2)) / SD
    w_var, w_lat = loss_weights(C, H, seed + 3)
    return dict(x=x, z=z, t=t, xt=xt, vt=vt, F=F, lv=lv, w_var=w_var, w_lat=w_lat)


def exact_crps_inputs(seed=0):
    """m = 2, alpha = 1, (B, C, H, W) = (2, 16, 256, 256): n = 2^21, members and target in {-1, 0, 1}, weights 1.  Every term
    w (skill - cs spread) is a multiple of 1/4 in [-1/2, 2] and 1/(B H W) = 2^-17, so partial sums in any order are integers
    times one quantum, fewer than 2^24 of them: fp32 addition is exact whatever the order."""
    g = torch.Generator().manual_seed(seed)
    shape = (2, 16, 256, 256)
    preds = torch.randint(-1, 2, (2, *shape), generator=g).float()
    target = torch.randint(-1, 2, shape, generator=g).float()
    return preds, target, torch.ones(shape[1]), torch.ones(shape[2])


# ------------------------------------------------------------------------------------------ ensemble sums

def ensemble_sums(pred, y, w_lat):
    """out[b, v] = (sum w (mean_n x - y)^2, sum_n sum w |x_n - y|, sum_{n, n'} sum w |x_n - x_n'|, sum w var_n(x) unbiased);
    pred [B, N, V, H, W], y [B, V, H, W], w_lat [H]."""
    x, y = pred.double(), y.double()
    w = w_lat.double().view(1, 1, -1, 1)
    N = x.shape[1]
    a0 = (w * (x.mean(1) - y) ** 2).sum((-2, -1))
    a1 = (w.unsqueeze(1) * (x - y.unsqueeze(1)).abs()).sum((1, 3, 4))
    a2 = torch.zeros_like(a0)
    for n in range(N):
        a2 += (w.unsqueeze(1) * (x - x[:, n:n + 1]).abs()).sum((1, 3, 4))
    a3 = (w * x.var(dim=1)).sum((-2, -1))
    return torch.stack([a0, a1, a2, a3], -1)


# ------------------------------------------------------------------------------------------ Adam / AdamW + EMA

def adam_ema_step(p, g, m, v, ema, lr, wd, b1, b2, eps, t, ema_beta, decoupled):
    """One step of torch.optim.AdamW (``decoupled``) or torch.optim.Adam with L2 weight decay on nan_to_num(g), then
    ema <- p.lerp(ema, ema_beta).  Returns (g_sanitised, p, m, v, ema) in fp64."""
    p, g, m, v = (a.double() for a in (p, g, m, v))
    g = torch.nan_to_num(g, nan=0.0, posinf=1e5, neginf=-1e5)
    gi = g
    if decoupled:
        p = p * (1.0 - lr * wd)
    else:
        gi = g + wd * p
    m = m + (gi - m) * (1.0 - b1)
    v = v * b2 + (1.0 - b2) * gi * gi
    denom = v.sqrt() / math.sqrt(1.0 - b2 ** t) + eps
    p = p - (lr / (1.0 - b1 ** t)) * (m / denom)
    e = None if ema is None else p + ema_beta * (ema.double() - p)
    return g, p, m, v, e
