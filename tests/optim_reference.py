"""fp64 closed forms, the fp32 torch-op yardstick, the per-chunk score and the designs for the two kernels that write the
parameters: swiftk_adamw_ema_step and swiftk_mars_ema_step (include/swiftk.h; swift_amd/training/fused_optim.py).

A *case* is ONE step from a stated fp32 state (p, ema, exp_avg, exp_avg_sq, last_grad), a gradient, a step count t and the
hyper-parameters as Python doubles.  Three things take that step: ``rule(case)``, the rule as documented in include/swiftk.h in
float64 on the fp32 inputs; ``torch_ops(case)``, the reference's own fp32 op sequence on the CPU (torch.optim.Adam / AdamW with
foreach=False or the MARS class, nan_to_num before it, Tensor.lerp after it); and the kernel.  Cases that continue another one
("t2") start from the yardstick's fp32 result of the first, so every scored step has one shared starting state.

The score, per chunk of <= 16384 elements (the kernels' unit of work) and per quantity q in dp = p_new - p_old, m, v,
de = e_new - e_old (differences taken in float64 from the stored fp32 values):

    err   = ||q - q_ref||_2 / ||q_ref||_2
    floor = ||2^-24 |stored value| ||_2 / ||q_ref||_2         (the half-ulp with which p, e, m and v are stored)
    pass:   err_kernel <= 4 * max(err_yardstick, floor)

4 is what tests/test_gpu_tangent_kernels.py and the hostile-row tests give a kernel that may contract multiply-adds differently
from torch.  A chunk whose q_ref is zero everywhere passes only on an exactly zero q.  Nothing here looks at a kernel's output
to set a bound, and no element is left out of a score (mars-lion leaves exp_avg_sq alone: there v is compared bit for bit with
its starting value instead).
"""
import functools
import math
from dataclasses import dataclass, field, replace
from typing import List, Optional

import torch

CHUNK = 16384
FACTOR = 4.0
HALF_ULP = 2.0 ** -24
ADAM_KINDS = ("adam", "adamw")
MARS_KINDS = ("mars-adamw", "mars-lion")
QUANTITIES = ("dp", "m", "v", "de")
EMA_HALFLIFE_BETA = 0.5 ** (64 / 500000)  # batch 64 at ema_halflife_kimg 500


@dataclass
class Case:
    name: str
    kind: str                       # adam | adamw | mars-adamw | mars-lion
    shapes: list
    group_of: list                  # param_groups index per tensor
    groups: list                    # [(lr, weight_decay)] per group
    betas: tuple
    eps: float
    t: int                          # the step count OF this step (bias corrections use beta ** t)
    ema_beta: float
    P: list
    E: list                         # entries may be None (no EMA copy)
    M: list
    V: list
    G: list
    L: Optional[list] = None        # last_grad (MARS)
    gamma: float = 0.025
    betas_1d: tuple = (0.9, 0.95)
    lr0: float = 3e-3               # MARS constructor lr: lr_1d_factor = lr_1d / lr0
    lr_1d: float = 3e-3
    weight_decay_1d: float = 0.1
    exact: bool = False             # one right answer, bit for bit

    @property
    def mars(self):
        return self.kind in MARS_KINDS

    def mars_rule(self, ti):
        return self.mars and len(self.shapes[ti]) == 2

    def scores_v(self, ti):
        return not (self.kind == "mars-lion" and self.mars_rule(ti))


@dataclass
class Result:
    P: list = field(default_factory=list)
    E: list = field(default_factory=list)
    M: list = field(default_factory=list)
    V: list = field(default_factory=list)
    L: list = field(default_factory=list)
    G: list = field(default_factory=list)       # the gradient as the step leaves it: sanitised
    norms: list = field(default_factory=list)   # ||c_t|| per tensor, 0 under the AdamW-1d rule (and for Adam / AdamW)


def numel(shape):
    return math.prod(shape)


def chunk_table(case):
    """The kernels' work list: one row per <= CHUNK consecutive elements of one tensor, flat offsets cumulative."""
    rows, off = [], 0
    for ti, sh in enumerate(case.shapes):
        n, first = numel(sh), len(rows)
        for s in range(0, n, CHUNK):
            rows.append(dict(tensor=ti, start=s, n=min(CHUNK, n - s), flat_off=off + s, group=case.group_of[ti], first=first,
                             count=-(-n // CHUNK), rule=0 if case.mars_rule(ti) else 1))
        off += n
    return rows


def sanitise(g):
    """nan_to_num(nan=0, posinf=1e5, neginf=-1e5), spelled out (every replacement is exact in fp32)."""
    inf = float("inf")
    g = torch.where(g != g, torch.zeros_like(g), g)
    g = torch.where(g == inf, torch.full_like(g, 1e5), g)
    return torch.where(g == -inf, torch.full_like(g, -1e5), g)


# ------------------------------------------------------------------------------------------------ the rule, closed form
WRONG = ("eps_first", "neighbour_group", "omb2", "clip_ge", "clip_always", "lerp_single")


def _tensor_step(case, ti, gi, dtype, wrong):
    b1, b2 = case.betas
    t, eps = case.t, case.eps
    lr, wd = case.groups[gi]
    f = lambda x: x.to(dtype).flatten()
    p0, g, m, v = f(case.P[ti]), f(sanitise(case.G[ti])), f(case.M[ti]), f(case.V[ti])
    off = 1.0 + 1e-4 if wrong == "omb2" else 1.0
    norm = 0.0
    if not case.mars:
        if case.kind == "adamw":
            p, ge = p0 * (1.0 - lr * wd), g
        else:
            p, ge = p0, g + wd * p0
        m = m + (ge - m) * (1.0 - b1)
        v = v * b2 + ((1.0 - b2) * off) * ge * ge
        bs = math.sqrt(1.0 - b2 ** t)
        denom = (v.sqrt() + eps) / bs if wrong == "eps_first" else v.sqrt() / bs + eps
        p = p - (lr / (1.0 - b1 ** t)) * (m / denom)
    else:
        if case.mars_rule(ti):
            c = g + (case.gamma * (b1 / (1.0 - b1))) * (g - f(case.L[ti]))
            norm = float(c.norm())
            clip = norm >= 1.0 if wrong == "clip_ge" else (True if wrong == "clip_always" else norm > 1.0)
            if clip:
                c = c / norm
            adam = case.kind == "mars-adamw"
        else:
            c, adam = g, True
            b1, b2 = case.betas_1d
            lr, wd = lr * (case.lr_1d / case.lr0), case.weight_decay_1d
        m = m * b1 + (1.0 - b1) * c
        if adam:
            v = v * b2 + ((1.0 - b2) * off) * c * c
            ib = 1.0 / math.sqrt(1.0 - b2 ** t)
            root = (v.sqrt() + eps) * ib if wrong == "eps_first" else v.sqrt() * ib + eps
            d = m / (root * (1.0 - b1 ** t))
        else:
            d = torch.sign(m)
        p = p0 - lr * (p0 * wd + d)
    e = None
    if case.E[ti] is not None:
        e0, beta = f(case.E[ti]), case.ema_beta
        # p.lerp(e, beta) in torch's two-sided form: exact at beta = 0 and at beta = 1
        e = p + beta * (e0 - p) if (beta < 0.5 or wrong == "lerp_single") else e0 - (e0 - p) * (1.0 - beta)
    return p, e, m, v, g, norm


def rule(case, dtype=torch.float64, wrong=None):
    """The step as include/swiftk.h documents it.  float64 is the reference; float32 is a plain restatement of a kernel, and
    ``wrong`` turns it into one of the deliberately wrong variants the score has to reject."""
    out = Result()
    for ti, sh in enumerate(case.shapes):
        p, e, m, v, g, norm = _tensor_step(case, ti, case.group_of[ti], dtype, wrong)
        if wrong == "neighbour_group" and ti == 0:  # the tensor's second chunk reads the next group's lr and weight decay
            q = _tensor_step(case, ti, (case.group_of[ti] + 1) % len(case.groups), dtype, None)
            sl = slice(CHUNK, 2 * CHUNK)
            p[sl] = q[0][sl]
            if e is not None:
                e[sl] = q[1][sl]
        out.P.append(p), out.E.append(e), out.M.append(m), out.V.append(v), out.G.append(g), out.L.append(g)
        out.norms.append(norm)
    return out


# -------------------------------------------------------------------------------------------------------- the yardstick
def torch_ops(case, dtype=torch.float32):
    """The reference's sequence with torch ops on the CPU: nan_to_num, the optimizer class's step, lerp."""
    from swift_amd.training.optimizers.mars import MARS
    P = [torch.nn.Parameter(p.to(dtype).clone()) for p in case.P]
    Gs = [torch.nan_to_num(g, nan=0.0, posinf=1e5, neginf=-1e5).to(dtype) for g in case.G]
    groups = [dict(params=[P[i] for i in range(len(P)) if case.group_of[i] == gi], lr=lr, weight_decay=wd)
              for gi, (lr, wd) in enumerate(case.groups)]
    if case.mars:
        opt = MARS(groups, lr=case.lr0, betas=case.betas, eps=case.eps, gamma=case.gamma, mars_type=case.kind,
                   lr_1d=case.lr_1d, betas_1d=case.betas_1d, weight_decay_1d=case.weight_decay_1d)
    else:
        cls = torch.optim.AdamW if case.kind == "adamw" else torch.optim.Adam
        opt = cls(groups, betas=case.betas, eps=case.eps, foreach=False)
    for i, p in enumerate(P):
        st = {"exp_avg": case.M[i].to(dtype).clone(), "exp_avg_sq": case.V[i].to(dtype).clone()}
        if case.mars:
            st["step"], st["last_grad"] = case.t - 1, case.L[i].to(dtype).clone()
        else:
            st["step"] = torch.tensor(float(case.t - 1))
        opt.state[p] = st
        p.grad = Gs[i].clone()
    opt.step()
    out = Result()
    with torch.no_grad():
        for i, p in enumerate(P):
            st = opt.state[p]
            out.P.append(p.detach().flatten())
            out.E.append(None if case.E[i] is None else p.detach().lerp(case.E[i].to(dtype), case.ema_beta).flatten())
            out.M.append(st["exp_avg"].flatten()), out.V.append(st["exp_avg_sq"].flatten())
            out.L.append(st["last_grad"].flatten() if case.mars else Gs[i].flatten())
            out.G.append(Gs[i].flatten())
            out.norms.append(0.0)
    return out


# ------------------------------------------------------------------------------------------------------------ the score
def chunk_norms(x):
    n = x.numel()
    k = -(-n // CHUNK)
    if k * CHUNK != n:
        x = torch.nn.functional.pad(x, (0, k * CHUNK - n))
    return x.view(k, CHUNK).pow(2).sum(1).sqrt()


def _quantity(case, res, q, ti):
    """(q, the stored value whose half-ulp is the floor) of tensor ti in float64, or None where q does not apply."""
    d = lambda x: x.double().flatten()
    if q == "dp":
        return d(res.P[ti]) - d(case.P[ti]), d(res.P[ti])
    if q == "m":
        return d(res.M[ti]), d(res.M[ti])
    if q == "v":
        return (d(res.V[ti]), d(res.V[ti])) if case.scores_v(ti) else None
    if case.E[ti] is None:
        return None
    return d(res.E[ti]) - d(case.E[ti]), d(res.E[ti])


def errors(case, got, ref):
    """{(q, tensor): per-chunk relative L2 error of ``got`` against ``ref``}; inf where q_ref is zero and q is not."""
    out = {}
    for q in QUANTITIES:
        for ti in range(len(case.shapes)):
            b = _quantity(case, ref, q, ti)
            if b is None:
                continue
            a = _quantity(case, got, q, ti)[0]
            num, den = chunk_norms(a - b[0]), chunk_norms(b[0])
            exact = torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, float("inf")))
            out[q, ti] = torch.where(den > 0, num / den.clamp_min(1e-300), exact)
    return out


def floors(case, ref):
    out = {}
    for q in QUANTITIES:
        for ti in range(len(case.shapes)):
            b = _quantity(case, ref, q, ti)
            if b is not None:
                den = chunk_norms(b[0])
                out[q, ti] = torch.where(den > 0, HALF_ULP * chunk_norms(b[1]) / den.clamp_min(1e-300), torch.zeros_like(den))
    return out


def judge(case, got, yard, ref):
    """(failures, worst): every (q, tensor, chunk, err_kernel, err_yardstick, floor) that misses
    err_kernel <= FACTOR * max(err_yardstick, floor), and per quantity the chunk with the largest
    err_kernel / max(err_yardstick, floor) as (ratio, err_kernel, err_yardstick, floor, tensor, chunk)."""
    ek, ey, fl = errors(case, got, ref), errors(case, yard, ref), floors(case, ref)
    fails, worst = [], {}
    for (q, ti), k in ek.items():
        allow = torch.maximum(ey[q, ti], fl[q, ti])
        ok = k <= FACTOR * allow   # a NaN fails
        for ci in torch.nonzero(~ok).flatten().tolist():
            fails.append((q, ti, ci, float(k[ci]), float(ey[q, ti][ci]), float(fl[q, ti][ci])))
        ratio = torch.where(k == 0, torch.zeros_like(k), k / allow)  # (k > 0 on allow == 0 is inf: a failure above)
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
        ci = int(ratio.argmax())
        w = (float(ratio[ci]), float(k[ci]), float(ey[q, ti][ci]), float(fl[q, ti][ci]), ti, ci)
        if q not in worst or w[0] > worst[q][0]:
            worst[q] = w
    return fails, worst


def describe(case, worst):
    return f"{case.name}: " + "; ".join(f"{q} kernel {w[1]:.2e} yardstick {w[2]:.2e} floor {w[3]:.2e} ratio {w[0]:.2f}"
                                        for q, w in worst.items())


# ---------------------------------------------------------------------------------------------------------- the designs
SHAPES = [(300, 1000), (1056,), (413, 379), (33, 7), (160, 900)]   # 19 + 1 + 10 + 1 + 9 = 40 chunks; 413 * 379 is odd, so the
GROUP_OF = [0, 1, 2, 1, 0]                                        # last two tensors' flat offsets are off the 16-byte boundary
GROUPS = [(2e-3, 0.05), (7e-4, 0.2), (3e-3, 0.0)]
MARS_GSCALE = [1.0, 1.0, 1.0, 1.0, 0.1]   # ||c_t|| > 1 on tensors 0 and 2, < 1 on 3 and 4
LION_SHAPES = [(5632, 1056), (1056,), (33, 7)]                    # 363 + 1 + 1 chunks
LARGE_SHAPES = [(2 * 3413, 1280), (33, 7)]                        # 534 + 1 chunks


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _lr_of(case_groups, group_of, ti):
    return case_groups[group_of[ti]][0]


def random_case(name, kind, seed, t, betas=None, eps=1e-8, ema_beta=0.9, g_std=1e-2, shapes=SHAPES, group_of=GROUP_OF,
                groups=GROUPS, grad=None, no_ema=(3,)):
    """A random design: p within a few lr of zero, e near p, and for t > 1 moments preloaded to the steady state of the
    quantity they average (c_t after its clip for MARS, g otherwise)."""
    mars = kind in MARS_KINDS
    if betas is None:
        betas = (0.95, 0.99) if mars else (0.9, 0.95)
    gen = _gen(seed)
    rn = lambda sh: torch.randn(sh, generator=gen)
    P, E, M, V, G, L = [], [], [], [], [], []
    for ti, sh in enumerate(shapes):
        lr = _lr_of(groups, group_of, ti)
        p = rn(sh) * (3 * lr)
        P.append(p)
        e = p + rn(sh) * (2 * lr)
        E.append(None if ti in no_ema else e)
        scale = g_std * (MARS_GSCALE[ti] if mars and shapes is SHAPES else 1.0)
        g = grad(sh, gen) if grad is not None else rn(sh) * scale
        G.append(g)
        last = rn(sh) * scale if t > 1 else torch.zeros(sh)
        L.append(last)
        if t == 1:
            M.append(torch.zeros(sh)), V.append(torch.zeros(sh))
            continue
        b1, b2 = betas
        c = g.double()
        if mars and len(sh) == 2:
            c = c + 0.025 * (b1 / (1 - b1)) * (c - last.double())
            c = c / max(1.0, float(c.norm()))
        elif mars:
            b1, b2 = 0.9, 0.95
        r = float(c.pow(2).mean().sqrt())
        M.append(rn(sh) * (r * math.sqrt((1 - b1) / (1 + b1))))
        V.append((r * r * (1 - b2 ** (t - 1))) * (1 + 0.3 * (2 * torch.rand(sh, generator=gen) - 1)))
    return Case(name=name, kind=kind, shapes=list(shapes), group_of=list(group_of), groups=list(groups), betas=betas, eps=eps,
                t=t, ema_beta=ema_beta, P=P, E=E, M=M, V=V, G=G, L=L if mars else None)


def follow(first, name, seed, grad=None, g_std=1e-2, groups=None, ema_beta=0.3):
    """The step after ``first``: starts from the yardstick's fp32 state, takes a fresh gradient, and by default uses other
    learning rates (the schedule writes param_groups[i]["lr"] between steps)."""
    y = torch_ops(first)
    gen = _gen(seed)
    if groups is None:
        groups = [(lr * (0.5 + 0.75 * gi), wd) for gi, (lr, wd) in enumerate(first.groups)]
    back = lambda xs: [None if x is None else x.view(sh).clone() for x, sh in zip(xs, first.shapes)]
    G = []
    for ti, sh in enumerate(first.shapes):
        scale = g_std * (MARS_GSCALE[ti] if first.mars and first.shapes == SHAPES else 1.0)
        G.append(grad(ti, sh, gen) if grad is not None else torch.randn(sh, generator=gen) * scale)
    return replace(first, name=name, t=first.t + 1, groups=groups, ema_beta=ema_beta, P=back(y.P), E=back(y.E), M=back(y.M),
                   V=back(y.V), L=back(y.L) if first.mars else None, G=G)


def _small_grad(sh, gen):
    """|g| log-uniform in [1e-13, 1e-9], random sign: with eps 1e-11 the place where eps joins decides the update."""
    mag = 10.0 ** (-13 + 4 * torch.rand(sh, generator=gen, dtype=torch.float64))
    sign = torch.where(torch.rand(sh, generator=gen) < 0.5, -1.0, 1.0)
    return (mag * sign).float()


def _plant_nonfinite(case):
    nan, inf = float("nan"), float("inf")
    G = [g.clone() for g in case.G]
    G[0].view(-1)[CHUNK * 3] = nan           # a chunk's first element
    G[0].view(-1)[CHUNK * 5 - 1] = inf       # a chunk's last element
    G[0].view(-1)[CHUNK * 18 + 7] = -inf     # the short last chunk
    G[1][7] = nan
    G[2].view(-1)[-2] = inf                  # 413 * 379 = 4 * 39131 + 3: the dword tail of the last chunk
    G[2].view(-1)[CHUNK * 9] = -inf
    G[3].view(-1)[4] = -inf
    G[4].view(-1)[0] = inf                   # dword path (flat offset off the 16-byte boundary)
    G[4].view(-1)[-1] = nan
    return replace(case, G=G)


def _lion_grad(std):
    def grad(sh, gen):
        mag = std * (0.5 + torch.rand(sh, generator=gen))
        return torch.where(torch.rand(sh, generator=gen) < 0.5, -mag, mag)
    return grad


def _exact_adam(kind):
    """Zero moments, t = 1, betas (0.5, 0.75), eps 0, power-of-two lr and weight decay in eight groups, g = +-2^k, p and e small
    multiples of lr: m = g / 2, v = g^2 / 4, sqrt(1 - beta2) = 1 / 2, step_size = 2 lr, p_new = p (1 - lr wd) - lr sign(g) and
    e_new = e - (e - p_new) / 2 without one rounding.  (Adam's L2 term would make g + wd p inexact: Adam runs with wd 0.)"""
    lens = [1, 3, 4, 5, 255, 256, 257, 16383, 16384, 2 * CHUNK + 5, 3, 4]   # 14 chunks; offsets fall off the boundary at once
    shapes = [(n,) for n in lens]
    group_of = [i % 8 for i in range(len(lens))]
    groups = [(2.0 ** -(6 + i), 2.0 ** -(1 + i % 4) if kind == "adamw" else 0.0) for i in range(8)]
    gen = _gen(11)
    P, E, G, chunk = [], [], [], 0
    for ti, n in enumerate(lens):
        lr = groups[group_of[ti]][0]
        i = torch.arange(n)
        ci = chunk + i // CHUNK                      # the chunk's place in the table
        k = (i % CHUNK) % 37 - 18 + ci % 5           # exponent: the element's place in its chunk, and the chunk
        sign = 1.0 - 2.0 * (((i % CHUNK) // 37 + ci) % 2)
        G.append((sign * torch.pow(torch.tensor(2.0, dtype=torch.float64), k.double())).float())
        P.append(torch.randint(-8, 9, (n,), generator=gen).float() * lr)
        E.append(None if ti % 4 == 2 else torch.randint(-8, 9, (n,), generator=gen).float() * lr)
        chunk += -(-n // CHUNK)
    Z = [torch.zeros(n) for n in lens]
    return Case(name=f"exact-{kind}", kind=kind, shapes=shapes, group_of=group_of, groups=groups, betas=(0.5, 0.75), eps=0.0, t=1,
                ema_beta=0.5, P=P, E=E, M=Z, V=[z.clone() for z in Z], G=G, exact=True)


def _exact_mars(kind, side, clipped):
    """beta1 0.5 and gamma 1 make gamma_ratio 1, so with last_grad 0 c = 2 g; |c| = 1 / side on side^2 elements sums, exactly
    and in any order, to a norm of 1.0 (not clipped), 2 / side to 2.0 (scale 1 / 2).  The 1-D tensor takes the AdamW-1d rule
    with betas_1d (0.5, 0.75) on power-of-two gradients; everything downstream is exact as in the AdamW design."""
    n = side * side
    shapes, group_of = [(side, side), (1056,)], [0, 1]
    groups = [(2.0 ** -8, 2.0 ** -3), (2.0 ** -10, 2.0 ** -2)]
    gen = _gen(13)
    i = torch.arange(n)
    sign = (1.0 - 2.0 * ((i % 3 + i // CHUNK) % 2)).float()
    g2 = sign * ((2.0 if clipped else 1.0) / side / 2.0)
    j = torch.arange(1056)
    g1 = ((1.0 - 2.0 * (j % 2)) * torch.pow(torch.tensor(2.0, dtype=torch.float64), (j % 29 - 14).double())).float()
    ints = lambda m: torch.randint(-8, 9, (m,), generator=gen).float()
    P = [(ints(n) * groups[0][0]).view(side, side), ints(1056) * 2.0 ** -11]
    E = [(ints(n) * groups[0][0]).view(side, side), ints(1056) * 2.0 ** -11]
    Z = lambda: [torch.zeros(side, side), torch.zeros(1056)]
    return Case(name=f"exact-{kind}-{side}-norm{2 if clipped else 1}", kind=kind, shapes=shapes, group_of=group_of, groups=groups,
                betas=(0.5, 0.75), eps=0.0, t=1, ema_beta=0.5, P=P, E=E, M=Z(), V=Z(), L=Z(), G=[g2.view(side, side), g1],
                gamma=1.0, betas_1d=(0.5, 0.75), lr0=2.0 ** -8, lr_1d=2.0 ** -9, weight_decay_1d=2.0 ** -2, exact=True)


def exact_norm(case, ti):
    return 0.0 if not case.mars_rule(ti) else float(case.name.rsplit("norm", 1)[1])


EMA_BETAS = {"0": 0.0, "0.3": 0.3, "0.5": 0.5, "0.9": 0.9, "halflife": EMA_HALFLIFE_BETA, "1": 1.0}
_BUILDERS = {}


def _register():
    B = _BUILDERS
    for kind in ADAM_KINDS + ("mars-adamw",):
        seed = 100 + 10 * (ADAM_KINDS + MARS_KINDS).index(kind)
        B[f"{kind}-t1"] = functools.partial(random_case, f"{kind}-t1", kind, seed, 1)
        B[f"{kind}-t2"] = lambda kind=kind, seed=seed: follow(case(f"{kind}-t1"), f"{kind}-t2", seed + 1)
        B[f"{kind}-t1000"] = functools.partial(random_case, f"{kind}-t1000", kind, seed + 2, 1000)
        B[f"{kind}-t100000"] = functools.partial(random_case, f"{kind}-t100000", kind, seed + 3, 100000)
        B[f"{kind}-nonfinite"] = lambda kind=kind, seed=seed: replace(
            _plant_nonfinite(follow(case(f"{kind}-t1"), "", seed + 4)), name=f"{kind}-nonfinite")
        B[f"{kind}-zero"] = lambda kind=kind, seed=seed: _zero_case(kind, seed + 5)
    for kind in ADAM_KINDS:
        seed = 200 + 10 * ADAM_KINDS.index(kind)
        for b2 in (0.95, 0.99, 0.999):
            for t in (1, 1000):
                n = f"{kind}-beta{b2}-t{t}"
                B[n] = functools.partial(random_case, n, kind, seed + t % 7, t, betas=(0.9, b2), eps=1e-11)
        B[f"{kind}-small-t1"] = functools.partial(random_case, f"{kind}-small-t1", kind, seed + 8, 1, betas=(0.9, 0.99), eps=1e-11,
                                                  grad=_small_grad)
        B[f"{kind}-small-t2"] = lambda kind=kind, seed=seed: follow(case(f"{kind}-small-t1"), f"{kind}-small-t2", seed + 9,
                                                                    grad=lambda ti, sh, gen: _small_grad(sh, gen))
    for kind in ("adamw", "mars-adamw"):
        for tag, beta in EMA_BETAS.items():
            n = f"{kind}-ema{tag}"
            B[n] = functools.partial(random_case, n, kind, 300 + len(tag), 1000, ema_beta=beta)
    B["mars-lion-s1"] = functools.partial(random_case, "mars-lion-s1", "mars-lion", 400, 1, shapes=LION_SHAPES, group_of=[0, 1, 1],
                                          groups=GROUPS[:2], grad=_lion_grad(1e-3), no_ema=())
    B["mars-lion-s2"] = _lion_second
    B["mars-adamw-large"] = functools.partial(random_case, "mars-adamw-large", "mars-adamw", 500, 1000, shapes=LARGE_SHAPES,
                                              group_of=[0, 1], groups=GROUPS[:2], g_std=1e-3, no_ema=())
    for kind in ADAM_KINDS:
        B[f"exact-{kind}"] = functools.partial(_exact_adam, kind)
    for kind in MARS_KINDS:
        for side in (256, 4096):
            for clipped in (False, True):
                B[f"exact-{kind}-{side}-norm{2 if clipped else 1}"] = functools.partial(_exact_mars, kind, side, clipped)


def _zero_case(kind, seed):
    """g = 0 on zero moments, eps > 0: m and v stay +0, p_new = p (1 - lr wd) under the decoupled rules and p under Adam with
    wd 0; the 1-D tensor's p is 0 and stays 0."""
    groups = [(lr, 0.0) for lr, _ in GROUPS] if kind == "adam" else GROUPS
    c = random_case(f"{kind}-zero", kind, seed, 1, groups=groups, grad=lambda sh, gen: torch.zeros(sh))
    c.P[1] = torch.zeros_like(c.P[1])
    return c


def _lion_second():
    """g2 has the sign of g1 and |g2| >= |g1|, so c2 = g2 + k (g2 - g1) and with it the first moment keep g1's sign: every
    sign(m) is determined (lion_margin, asserted by the CPU test)."""
    first = case("mars-lion-s1")

    def grad(ti, sh, gen):
        return first.G[ti] * (1.0 + torch.rand(sh, generator=gen))
    return follow(first, "mars-lion-s2", 401, grad=grad)


def lion_margin(c):
    """min over MARS-rule elements of |m_new| / rms(m_new) in float64."""
    r = rule(c)
    return min(float(r.M[ti].abs().min() / r.M[ti].pow(2).mean().sqrt()) for ti in range(len(c.shapes)) if c.mars_rule(ti))


_register()
BIG = tuple(n for n in _BUILDERS if "-4096-" in n)             # 4^12 elements, 67 MB per buffer: built on demand, never cached
NAMES = tuple(n for n in _BUILDERS if n not in BIG)
SEQUENCES = {                                                  # steps a fused-class object takes one after the other
    **{k: (f"{k}-t1", f"{k}-t2") for k in ADAM_KINDS + ("mars-adamw",)},   # the second with other learning rates
    **{f"{k}-small": (f"{k}-small-t1", f"{k}-small-t2") for k in ADAM_KINDS},
    "mars-lion": ("mars-lion-s1", "mars-lion-s2"),
}


@functools.lru_cache(maxsize=None)
def _cached(name):
    return _BUILDERS[name]()


def case(name):
    return _BUILDERS[name]() if name in BIG else _cached(name)


@functools.lru_cache(maxsize=None)
def references(name):
    """(float64 rule, fp32 yardstick) of a cached case: computed once, shared, never modified."""
    c = case(name)
    return rule(c), torch_ops(c)
