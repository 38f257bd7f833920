"""TEST INFRASTRUCTURE: fields, yardsticks and scores for the two metric-sum kernels of swift_amd/csrc/train_kernels.hip,
``swiftk_ensemble_sums`` (every RMSE / CRPS / spread-skill number of evaluation_metrics.json) and ``swiftk_rmse_sums`` (the
checkpoint RMSE of training/validate.py).

The fp64 truths are ``backward_reference.ensemble_sums`` and ``tangent_reference.rmse_sums``; nothing here restates them.

  * ``ensemble_terms_fp32``  -- the kernel's per-point arithmetic in torch fp32 on the CPU (member order, sequential sums,
                                ``/ (float)N``, ``/ (float)(N - 1)``), as the four weighted term planes.  ``shifted=False`` takes
                                the mean of the members as they are, ``shifted=True`` about the first member: d_n = x_n - x_0,
                                m = mean(d_n), (m - (y - x_0))^2 and sum (d_n - m)^2.  A yardstick, never the code under test.
  * ``rmse_terms_fp32``      -- the same for the two term planes of ``swiftk_rmse_sums``.
  * ``device_order_sum``     -- adds a term plane in fp32 in the (lane, wave, block) order of the kernels' launches.
  * field builders, seeded; each gives (pred [B, N, V, H, W], y [B, V, H, W], w_lat [H]) in fp32.  The latitudes run from -78 to
    84 degrees, so they are not symmetric about the equator and a flipped or wrong row index changes every result.
      physical  the variable slots hold different families (offset +- member spread, truth within a spread of the centre):
                280 +- 0.3, 5e4 +- 30, 3e-6 +- 3e-7, 0 +- 10 -- a (b, v) routing or member-stride error is a gross miss
      hostile   280 +- 0.01, 1e5 +- 3, 2e5 +- 1, 2e5 +- 0.1: offset / spread from 2.8e4 to 2e6
      planted   a physical field in which the members of variable 1 all agree (sums 2 and 3 must be exactly 0.0), in variable
                0 one member equals the truth at every 7th point and all members equal it at every 11th, and the truth of
                variable 3 lies 1000 spreads outside the ensemble
      exact     integers with one right answer in any summation order: weights 2 (every third row) and 1,
                x_n = c + (N - 1) e_n with c = 3 + (b V + v), e zero-sum (+a, -a, zeros; a in {1, 2} and the two places drawn
                per point), y = c + an integer in [-3, 3].  Then mean = c, every term and every partial sum is a
                whole number below 2^24.  A point with e != 0 puts 4 a (N - 1)^2 w into the pair-spread sum, which alone would pass 2^24
                on 8481 points from N = 16 on, so e is non-zero on every s-th point (s the smallest stride that keeps every sum
                below 2^24 whatever is drawn; 1 up to N = 9 there), the stride's phase shifted by 5 (b V + v); c, the amplitudes, the places, y and the
                phase differ by (b, v), the one weight vector of a call cannot, so each of the B V 4 outputs has its own value.
    and for ``swiftk_rmse_sums`` (y [B, C, H, W], T [B, days, C, H, W] whose slice [:, 1] is the truth, the other days NaN):
      rmse_physical  channels alternate 2e5 +- 50 with differences of order 1 and 280 +- 5 with differences of order 0.3
      rmse_exact     integers, differences (c + 1) x {-3 .. 3}, the weights above
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import backward_reference as br
import tangent_reference as tr

F32, F64 = torch.float32, torch.float64
F32_TOL = 1e-5           # the suite's bound on an fp32 sum of non-negative terms: 1e-5 x the sum of the absolute terms
ARITH_TOL = 1e-6         # what the per-point arithmetic alone may cost: a tenth of it
MEMBERS = (2, 8, 9, 16, 17, 64)          # both ends of the three instantiations (<= 8, <= 16, <= 64 members in registers)
SHAPE_ONE_BLOCK = (2, 4, 7, 11)          # 77 points: one partly filled workgroup per (b, v)
SHAPE_BLOCKS = (2, 4, 19, 67)            # 1273 points: 5 workgroups, the last ragged, no second trip
SHAPE_PAST_CAP = (2, 4, 33, 257)         # 8481 points: 34 workgroups wanted, 32 run, 289 threads take a ragged second trip
SHAPES = (SHAPE_ONE_BLOCK, SHAPE_BLOCKS, SHAPE_PAST_CAP)
ENSEMBLE_BLOCK_CAP, RMSE_BLOCK_CAP = 32, 64
RMSE_SHAPE = (3, 2, 33, 257)             # 25443 points per channel against 64 x 256 = 16384 before the stride loop
RMSE_DAYS = 3

PHYSICAL = ((280.0, 0.3), (5e4, 30.0), (3e-6, 3e-7), (0.0, 10.0))
HOSTILE = ((280.0, 0.01), (1e5, 3.0), (2e5, 1.0), (2e5, 0.1))
PLANTED_AGREE_VAR, PLANTED_POINTS_VAR, PLANTED_FAR_VAR = 1, 0, 3
RMSE_FAMILIES = ((2e5, 50.0, 1.0), (280.0, 5.0, 0.3))   # offset, variation of the field, size of the differences


def lats(H):
    return np.linspace(-78.0, 84.0, H)


def lat_weights(H):
    """cos(lat) / mean(cos(lat)) rounded to fp32, exactly what eval/metrics.py hands the kernel for ``lats(H)``."""
    w = np.cos(np.deg2rad(lats(H)))
    return torch.from_numpy(w / w.mean()).float()


def exact_weights(H):
    return torch.where(torch.arange(H) % 3 == 0, 2.0, 1.0).float()


def _seed(kind, N, shape):
    return 1000 * ("physical", "hostile", "planted", "exact").index(kind) + 10 * N + shape[2]


def _family_field(families, N, shape, seed):
    B, V, H, W = shape
    assert V == len(families)
    g = torch.Generator().manual_seed(seed)
    off = torch.tensor([f[0] for f in families], dtype=F64).view(1, V, 1, 1)
    sp = torch.tensor([f[1] for f in families], dtype=F64).view(1, V, 1, 1)
    centre = off + sp * torch.randn(B, V, H, W, generator=g, dtype=F64)
    pred = centre.unsqueeze(1) + sp.unsqueeze(1) * torch.randn(B, N, V, H, W, generator=g, dtype=F64)
    y = centre + sp * torch.randn(B, V, H, W, generator=g, dtype=F64)
    return pred.float(), y.float(), lat_weights(H)


def physical(N, shape=SHAPE_PAST_CAP):
    return _family_field(PHYSICAL, N, shape, _seed("physical", N, shape))


def hostile(N, shape=SHAPE_PAST_CAP):
    return _family_field(HOSTILE, N, shape, _seed("hostile", N, shape))


def planted(N, shape=SHAPE_PAST_CAP):
    pred, y, w = _family_field(PHYSICAL, N, shape, _seed("planted", N, shape))
    B, V, H, W = shape
    pred[:, :, PLANTED_AGREE_VAR] = pred[:, :1, PLANTED_AGREE_VAR]
    i = torch.arange(H * W)
    pv, yv = pred[:, :, PLANTED_POINTS_VAR].reshape(B, N, H * W), y[:, PLANTED_POINTS_VAR].reshape(B, H * W)
    one = i[i % 7 == 3]
    pv[:, one % N, one] = yv[:, one]             # one member (which one changes from point to point) equals the truth
    every = i[i % 11 == 5]
    pv[:, :, every] = yv[:, None, every]         # all members equal the truth
    pred[:, :, PLANTED_POINTS_VAR] = pv.view(B, N, H, W)
    y[:, PLANTED_FAR_VAR] += 1000.0 * PHYSICAL[PLANTED_FAR_VAR][1]
    return pred, y, w


def planted_one_member_points(shape):
    i = torch.arange(shape[2] * shape[3])
    return i[i % 7 == 3], i[i % 11 == 5]


def _exact_with_stride(N, shape, seed, stride):
    B, V, H, W = shape
    hw = H * W
    g = torch.Generator().manual_seed(seed)
    bv = torch.arange(B * V).view(B, V)
    c = (3 + bv).double()
    amp = torch.randint(1, 3, (B, V, hw), generator=g).double()
    p = torch.randint(0, N, (B, V, hw), generator=g)
    q = (p + 1 + torch.randint(0, N - 1, (B, V, hw), generator=g)) % N     # a second place, never the first
    i = torch.arange(hw).view(1, 1, hw)
    active = ((i + 5 * bv.view(B, V, 1)) % stride == 0).double()
    a = amp * active
    e = torch.zeros(B, N, V, hw, dtype=F64)
    e.scatter_(1, p.unsqueeze(1), a.unsqueeze(1))
    e.scatter_(1, q.unsqueeze(1), -a.unsqueeze(1))
    pred = c.view(B, 1, V, 1) + (N - 1) * e
    y = c.view(B, V, 1) + torch.randint(-3, 4, (B, V, hw), generator=g).double()
    return pred.view(B, N, V, H, W).float(), y.view(B, V, H, W).float(), exact_weights(H)


def exact_stride(N, shape):
    """The smallest stride of the points with e != 0 at which the largest sum (pair spread: 4 a (N - 1)^2 w per such point, a <= 2,
    w 4/3 on average; bounded here with a = 2 and w = 2 on every point) stays below 2^24."""
    hw = shape[2] * shape[3]
    s = 1
    while 16 * (N - 1) ** 2 * ((hw + s - 1) // s + 1) >= 2 ** 24:
        s += 1
    return s


def _exact_case(N, shape):
    for k in range(100):   # drawn again (seed + 100000, ...) until each of the B V 4 sums has its own value
        pred, y, w = _exact_with_stride(N, shape, _seed("exact", N, shape) + 100000 * k, exact_stride(N, shape))
        ref = br.ensemble_sums(pred, y, w)
        if ref.unique().numel() == shape[0] * shape[1] * 4:
            return pred, y, w, ref
    raise AssertionError(f"no exact case with {shape[0] * shape[1] * 4} different sums at N = {N}, {shape}")


def exact(N, shape=SHAPE_PAST_CAP):
    return _exact_case(N, shape)[:3]


BUILDERS = dict(physical=physical, hostile=hostile, planted=planted, exact=exact)


@functools.lru_cache(maxsize=None)
def case(kind, N, shape=SHAPE_PAST_CAP):
    """(pred, y, w_lat, fp64 truth [B, V, 4]) of a builder, computed once and shared (treat as read-only)."""
    if kind == "exact":
        return _exact_case(N, shape)
    pred, y, w = BUILDERS[kind](N, shape)
    return pred, y, w, br.ensemble_sums(pred, y, w)


def offset_over_spread(pred):
    """Per variable: median |x| over the median unbiased standard deviation of the members."""
    x = pred.double()
    sd = x.std(dim=1)
    V = x.shape[2]
    return torch.stack([x[:, :, v].abs().median() / sd[:, v].median() for v in range(V)])


# ------------------------------------------------------------------------------------------ the kernel's arithmetic in fp32

def ensemble_terms_fp32(pred, y, w_lat, shifted):
    """[4, B, V, H, W] fp32: w (mean - y)^2, w sum_n |x_n - y|, w 2 sum_{k < n} |x_n - x_k|, w sum_n (x_n - mean)^2 / (N - 1), every
    operation one fp32 rounding in the order of ensemble_sums_kernel (products are rounded before they are added: the device may
    fuse some, which is worth less than one rounding each)."""
    x, t = pred.to(F32), y.to(F32)
    B, N, V, H, W = x.shape
    w = w_lat.to(F32).view(1, 1, H, 1).expand(B, V, H, W)
    fN, fN1 = torch.tensor(float(N), dtype=F32), torch.tensor(float(N - 1), dtype=F32)
    if shifted:
        d = [x[:, n] - x[:, 0] for n in range(N)]
        ty = t - x[:, 0]
    else:
        d, ty = [x[:, n] for n in range(N)], t
    m = torch.zeros_like(t)
    for n in range(N):
        m = m + d[n]
    m = m / fN
    e, sp, var = torch.zeros_like(t), torch.zeros_like(t), torch.zeros_like(t)
    for n in range(N):
        e = e + (x[:, n] - t).abs()
        c = d[n] - m
        var = var + c * c
        for k in range(n):
            sp = sp + (x[:, n] - x[:, k]).abs()
    r = m - ty
    return torch.stack([w * r * r, w * e, w * 2.0 * sp, w * var / fN1])


def rmse_terms_fp32(y, t, w_lat):
    """[2, B, C, H, W] fp32: (y - t)^2 and w (y - t)^2 in the order of rmse_sums_kernel."""
    d = y.to(F32) - t.to(F32)
    w = w_lat.to(F32).view(1, 1, -1, 1)
    return torch.stack([d * d, (w * d * d).expand_as(d)])


def sums64(terms):
    """Term planes [k, B, V, H, W] -> their fp64 grid sums [B, V, k]."""
    return terms.double().sum((-2, -1)).permute(1, 2, 0)


def device_order_sum(plane, cap):
    """One flat fp32 term plane added in fp32 the way a 256-thread launch of min(ceil(n / 256), cap) workgroups adds it: each thread
    its grid-stride elements in turn, the 64 lanes of a wave in an xor tree, the four waves in order, the workgroups one after
    another into the output (the atomics' order is not fixed; any order must do for an exact design)."""
    v = plane.reshape(-1).to(F32)
    n = v.numel()
    G = min((n + 255) // 256, cap)
    trips = (n + G * 256 - 1) // (G * 256)
    v = torch.cat([v, torch.zeros(trips * G * 256 - n, dtype=F32)]).view(trips, G, 4, 64)
    acc = torch.zeros(G, 4, 64, dtype=F32)
    for j in range(trips):
        acc = acc + v[j]
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, :, lane ^ o]
    blocks = ((acc[:, 0, 0] + acc[:, 1, 0]) + acc[:, 2, 0]) + acc[:, 3, 0]
    out = torch.zeros((), dtype=F32)
    for k in range(G):
        out = out + blocks[k]
    return out


def shuffled_sum(plane, seed):
    """The plane added in fp32, one element after another, in a shuffled order."""
    v = plane.reshape(-1).to(F32)
    v = v[torch.randperm(v.numel(), generator=torch.Generator().manual_seed(seed))]
    return torch.cumsum(v, 0, dtype=F32)[-1]


def rel_err(got, ref):
    """|got - ref| / |ref| per entry in fp64; 0 where both are 0, inf where only the truth is."""
    got, ref = got.double(), ref.double()
    num = (got - ref).abs()
    return torch.where(ref != 0, num / ref.abs().clamp_min(1e-300), torch.where(num > 0, torch.full_like(num, float("inf")), torch.zeros_like(num)))


# ------------------------------------------------------------------------------------------ swiftk_rmse_sums

def _rmse_wrap(y, t):
    B, C, H, W = y.shape
    T = torch.full((B, RMSE_DAYS, C, H, W), float("nan"), dtype=F32)
    T[:, 1] = t
    return T


def rmse_physical(shape=RMSE_SHAPE, seed=7):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    fam = [RMSE_FAMILIES[c % len(RMSE_FAMILIES)] for c in range(C)]
    col = lambda k: torch.tensor([f[k] for f in fam], dtype=F64).view(1, C, 1, 1)
    t = col(0) + col(1) * torch.randn(B, C, H, W, generator=g, dtype=F64)
    y = t + col(2) * torch.randn(B, C, H, W, generator=g, dtype=F64)
    return y.float(), _rmse_wrap(y, t.float()), lat_weights(H)


def rmse_exact(shape=RMSE_SHAPE, seed=8):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(100, 200, (B, C, H, W), generator=g).double()
    y = t + torch.randint(-3, 4, (B, C, H, W), generator=g).double() * (1 + torch.arange(C)).view(1, C, 1, 1)
    return y.float(), _rmse_wrap(y, t.float()), exact_weights(H)


@functools.lru_cache(maxsize=None)
def rmse_case(kind):
    """(y, T, w_lat, fp64 truth [1 + C]) with T[:, 1] the truth field."""
    y, T, w = dict(physical=rmse_physical, exact=rmse_exact)[kind]()
    return y, T, w, tr.rmse_sums(y, T[:, 1], w)
