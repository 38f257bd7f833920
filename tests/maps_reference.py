"""References for ``swiftk_ensemble_maps`` (include/swiftk.h): per-pixel bias, squared error, fair CRPS and member variance of an
ensemble against the verifying fields, and the regional means ``generate --maps`` takes of them.  A helper module of the maps
tests (no test here).

``exact``         the four terms of every pixel in rational arithmetic.  fp32 values are integer multiples of 2^-149, so with the
                  members X_m and the truth Y as Python integers in that unit, S = sum X_m, a = sum |X_m - Y| and
                  p = sum_{m < m'} |X_m - X_m'| the terms are the fractions (S - N Y) / N, ((S - N Y) / N)^2,
                  ((N - 1) a - p) / (N (N - 1)) and sum (N X_m - S)^2 / (N^2 (N - 1)); each is rounded once, to fp64, by Python's
                  correctly rounded int / int.
``emulate``       numpy fp64 in precisely the documented order (numpy rounds every operation separately and never fuses).
``emulate_fp32``  the same formulas and order in fp32: what a torch one-liner on the fp32 fields amounts to.
``bound``         the forward-error bound of ``emulate`` (and of the kernel, which does the same operations) against ``exact``.
``regions`` / ``region_scores``  the regional reduction, written with plain loops.

The bound.  u = 2^-53, gamma_k = k u / (1 - k u): a chain of k rounded operations on terms t_i errs by at most gamma_k sum |t_i|
(Higham, Accuracy and Stability, lemma 3.1 and section 4.2: each term passes through at most k roundings).  For a pixel with
members x_m, truth y, N members, A = sum |x_m|, P = N (N - 1) / 2 pairs:

bias.      s takes N - 1 rounded additions (0 + x_0 is exact), the quotient one, the difference one: N + 1 operations on the terms
           x_m / N and y, so |error| <= gamma_{N+1} (A / N + |y|) =: B.  The mean alone, N operations: delta <= gamma_N A / N.
mse.       The kernel squares its own e' = e + (error <= B): e'^2 - e^2 = (e' - e)(e' + e), at most B (2 |e| + B), and the product
           rounds once more, u e'^2 <= u (|e| + B)^2.
crps.      Each |x_m - y| is one rounding and joins a through at most N - 1 additions, the quotient is one more: N + 1 operations on
           a / N.  Each |x_m - x_m'| likewise: P + 1 on p / (N (N - 1)); (double)(N (N - 1)) is exact.  The final difference is one
           more on both: max(N, P) + 2 operations on the terms, whose absolute sum is a / N + p / (N (N - 1)).
variance.  The kernel centres on its own mean' = mean + delta.  sum (x_m - mean - delta)^2 = sum (x_m - mean)^2 + N delta^2
           exactly, because the exact deviations add up to zero: the wrong centre adds N delta^2 / (N - 1) <= 2 delta^2 and nothing
           to first order.  On top, each d_m rounds once (twice in its square), each product once, N - 1 additions, one quotient:
           N + 3 operations on non-negative terms whose sum is that variance.

Two more operations are counted in every chain: one for the reference's own rounding to fp64 (u |term|), one because the
magnitudes below are themselves evaluated in fp64 (relative error under gamma_{N^2}, 2e-13: far below one part in k).  Nothing in
the bound is measured.
"""
import math

import numpy as np

U = 2.0 ** -53
STATISTICS = ["bias", "mse", "crps", "variance"]
KINDS = ("normal", "t280", "z2e5", "const")
PHYSICAL = {"t280": (280.0, 0.01), "z2e5": (2e5, 0.1)}   # offset and member spread: the hostile families of metric_sums_reference.py
_SCALE = 149                                              # fp32 values are integers in units of 2^-149


def make(kind, shape, seed=0):
    """(pred [n, N, V, H, W], y [n, V, H, W]) fp32.  ``normal``: standard normal members and truth.  ``t280`` / ``z2e5``: the design
    of tests/metric_sums_reference.py -- a centre offset + spread g per pixel, members and truth each the centre + spread g'
    (280 +- 0.01 K, 2e5 +- 0.1 m^2/s^2).  ``const``: identical members 280 + 30 g, the truth one spread away."""
    n, N, V, H, W = shape
    r = np.random.default_rng(seed)
    g = r.standard_normal(shape)
    gy = r.standard_normal((n, V, H, W))
    if kind == "normal":
        x, t = g, gy
    elif kind in PHYSICAL:
        off, sp = PHYSICAL[kind]
        centre = off + sp * r.standard_normal((n, V, H, W))
        x, t = centre[:, None] + sp * g, centre + sp * gy
    elif kind == "const":
        x, t = np.broadcast_to(280.0 + 30.0 * g[:, :1], shape), 280.0 + 30.0 * gy
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(t, dtype=np.float32)


def _ints(a):
    """The values in units of 2^-149 as Python integers (an object array): the scaling is a power of two and exact in fp64."""
    return np.frompyfunc(int, 1, 1)(np.asarray(a, dtype=np.float32).astype(np.float64) * 2.0 ** _SCALE)


def exact(pred, y):
    """pred [n, N, V, H, W], y [n, V, H, W] fp32 -> [n, 4, V, H, W] fp64: the exact terms, each rounded once."""
    N = pred.shape[1]
    X, Y = _ints(pred), _ints(y)
    aabs = np.frompyfunc(abs, 1, 1)
    S = X.sum(axis=1)
    E = S - N * Y                                              # N (mean - y)
    a = aabs(X - Y[:, None]).sum(axis=1)
    p = 0 * S
    for m in range(N):
        for k in range(m + 1, N):
            p = p + aabs(X[:, m] - X[:, k])
    D = N * X - S[:, None]
    Vn = (D * D).sum(axis=1)                                   # N^2 (N - 1) variance
    one, two = 1 << _SCALE, 1 << (2 * _SCALE)
    f = lambda fn, *arrs: np.frompyfunc(fn, len(arrs), 1)(*arrs).astype(np.float64)
    return np.stack([f(lambda e: e / (N * one), E),
                     f(lambda e: (e * e) / (N * N * two), E),
                     f(lambda a_, p_: ((N - 1) * a_ - p_) / (N * (N - 1) * one), a, p),
                     f(lambda v: v / (N * N * (N - 1) * two), Vn)], axis=1)


def _terms(pred, y, dt):
    N = pred.shape[1]
    x, t = pred.astype(dt), y.astype(dt)
    s, a = np.zeros(t.shape, dtype=dt), np.zeros(t.shape, dtype=dt)
    for m in range(N):
        s = s + x[:, m]
        d = x[:, m] - t
        a = a + np.abs(d)
    mean = s / dt(N)
    e = mean - t
    v, p = np.zeros(t.shape, dtype=dt), np.zeros(t.shape, dtype=dt)
    for m in range(N):
        d = x[:, m] - mean
        q = d * d
        v = v + q
    for m in range(N):
        for k in range(m + 1, N):
            d = x[:, m] - x[:, k]
            p = p + np.abs(d)
    a_n = a / dt(N)
    p_n = p / dt(N * (N - 1))
    return np.stack([e, e * e, a_n - p_n, v / dt(N - 1)], axis=1)


def emulate(pred, y, acc=None):
    """[n, 4, V, H, W] fp64 by the kernel's order of arithmetic in numpy fp64; with ``acc`` (such an array) ``acc + terms``, one
    rounded add per element (a new array: ``acc`` is left alone)."""
    t = _terms(pred, y, np.float64)
    return t if acc is None else acc + t


def emulate_fp32(pred, y):
    """The same formulas in the same order in fp32, widened to fp64 at the end."""
    return _terms(pred, y, np.float32).astype(np.float64)


def gamma(k):
    return k * U / (1.0 - k * U)


def bound(N, x, y):
    """Per-pixel forward-error bounds [n, 4, V, H, W] of the documented fp64 arithmetic against ``exact`` (module docstring):
    x [n, N, V, H, W] the members, y [n, V, H, W] the truth."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    assert x.shape[1] == N
    P = N * (N - 1) // 2
    A = np.abs(x).sum(axis=1)
    Bb = gamma(N + 1 + 2) * (A / N + np.abs(y))
    e = np.abs(x.sum(axis=1) / N - y) + Bb                     # an upper bound of |e|
    Bm = Bb * (2.0 * e + Bb) + 3.0 * U * (e + Bb) ** 2        # the product's rounding and the two extra operations
    a = np.abs(x - y[:, None]).sum(axis=1)
    p = np.zeros_like(a)
    for m in range(N):
        for k in range(m + 1, N):
            p = p + np.abs(x[:, m] - x[:, k])
    Bc = gamma(max(N, P) + 2 + 2) * (a / N + p / (N * (N - 1)))
    delta = gamma(N + 2) * A / N
    var = ((x - x.mean(axis=1, keepdims=True)) ** 2).sum(axis=1) / (N - 1)
    Bv = gamma(N + 3 + 2) * (var + 2.0 * delta ** 2) + 2.0 * delta ** 2
    return np.stack([Bb, Bm, Bc, Bv], axis=1)


def within(got, ref, bnd):
    """(every element within its bound, the largest error / bound over the elements with a positive bound)."""
    e = np.abs(np.asarray(got, dtype=np.float64) - ref)
    pos = bnd > 0
    return bool(np.all(e <= bnd)), float(np.max(e[pos] / bnd[pos])) if pos.any() else 0.0


# ------------------------------------------------------------------------------------------ the regional reduction
REGIONS = {"global": lambda la: True, "tropics": lambda la: abs(la) <= 20.0, "n_extratropics": lambda la: la >= 20.0,
           "s_extratropics": lambda la: la <= -20.0}


def regions(maps, lat):
    """maps [..., H, W] fp64 -> {region: [...]}: sum_h w_h mean_w maps / sum_h w_h over the region's rows, w_h = cos(lat_h), in
    correctly rounded sums (``math.fsum``); a region without rows is left out."""
    maps = np.asarray(maps, dtype=np.float64)
    lead = maps.shape[:-2]
    H, W = maps.shape[-2:]
    flat = maps.reshape(-1, H, W)
    out = {}
    for name, inside in REGIONS.items():
        rows = [h for h in range(H) if inside(float(lat[h]))]
        if not rows:
            continue
        w = [math.cos(math.radians(float(lat[h]))) for h in rows]
        wsum = math.fsum(w)
        vals = [math.fsum(wh * float(flat[i, h, c]) for wh, h in zip(w, rows) for c in range(W)) / (W * wsum)
                for i in range(flat.shape[0])]
        out[name] = np.array(vals).reshape(lead)
    return out


def region_scores(mean_maps, lat, variables, interval):
    """IC-mean maps [steps, 4, nv, H, W] fp64 -> the dictionary of evaluation_regions.json: region -> ``bias_`` / ``rmse_`` /
    ``crps_`` / ``spread_`` / ``ssr_<var>_<lead>h``, with rmse = sqrt(mean mse), spread = sqrt(mean variance), ssr = spread / rmse."""
    res = {}
    for region, m in regions(mean_maps, lat).items():            # m [steps, 4, nv]
        out = res.setdefault(region, {})
        for j in range(m.shape[0]):
            for i, v in enumerate(variables):
                tag = f"{v}_{(j + 1) * interval}h"
                rmse, spread = math.sqrt(m[j, 1, i]), math.sqrt(m[j, 3, i])
                out[f"bias_{tag}"], out[f"rmse_{tag}"], out[f"crps_{tag}"] = float(m[j, 0, i]), rmse, float(m[j, 2, i])
                out[f"spread_{tag}"], out[f"ssr_{tag}"] = spread, (spread / rmse if rmse > 0 else float("nan"))
    return res


def region_abs(mean_maps, lat):
    """The same reduction of |maps|: the scale of a regional mean's summation error ([steps, 4, nv] per region)."""
    return regions(np.abs(mean_maps), lat)
