"""Reference of ``swiftk_event_table`` (include/swiftk.h), a brute-force Brier score, and the case generators of the event tests.

Definition.  pred [n, N, V, H, W], y [n, V, H, W], thr [E, H, W] fp32, ev_var [E], ev_dir [E] integers, w [H] fp64.  Event e is
``x > thr[e]`` (ev_dir 0) or ``x < thr[e]`` (nonzero) on channel ev_var[e], strict IEEE comparisons of the fp32 values.  At a pixel
(h, w) whose thr[e,h,w] is not NaN let k = #{m: event(x_m)} and o = event(y): the pixel is counted in cell (k, o).

``reference`` counts with numpy integers, c [n, E, H, N + 1, 2], and then forms out[i,e,k,o] = sum over h ascending of
w[h] * float64(c_h[k][o]) with a Python loop over h, product and sum separate numpy float64 operations (numpy has no fused
multiply-add): the order of arithmetic the contract documents, so the kernel must agree bit for bit -- there is no rounding
freedom to bound.  ``brier_direct`` takes the weighted mean of (k / N - o)^2 over the unmasked pixels straight from the
definition, without any table.
"""
import numpy as np


def lat_of(H):
    """Cell-centre latitudes of an H-row grid (no pole row: every weight is positive)."""
    return -90.0 + (np.arange(H, dtype=np.float64) + 0.5) * (180.0 / H)


def lat_weights(lat):
    w = np.cos(np.deg2rad(np.asarray(lat, dtype=np.float64)))
    return w / w.mean()


def _events(pred, y, thr, ev_var, ev_dir):
    """(k [n, E, H, W] int64, o [n, E, H, W] int64, valid [E, H, W] bool)."""
    pred, y, thr = np.asarray(pred), np.asarray(y), np.asarray(thr)
    assert pred.dtype == y.dtype == thr.dtype == np.float32 and pred.ndim == 5 and y.shape == pred.shape[:1] + pred.shape[2:]
    n, N, V, H, W = pred.shape
    E = len(ev_var)
    assert thr.shape == (E, H, W) and len(ev_dir) == E
    k, o = np.zeros((n, E, H, W), dtype=np.int64), np.zeros((n, E, H, W), dtype=np.int64)
    with np.errstate(invalid="ignore"):   # (comparisons with the NaN of a masked pixel)
        for e in range(E):
            v, t = int(ev_var[e]), thr[e]
            assert 0 <= v < V
            x, yy = pred[:, :, v], y[:, v]
            k[:, e] = ((x < t) if ev_dir[e] else (x > t)).sum(1)
            o[:, e] = (yy < t) if ev_dir[e] else (yy > t)
    return k, o, ~np.isnan(thr)


def counts(pred, y, thr, ev_var, ev_dir):
    """The integer row tables c [n, E, H, N + 1, 2]: the unmasked pixels of row h with k members in the event and outcome o."""
    k, o, valid = _events(pred, y, thr, ev_var, ev_dir)
    N = np.asarray(pred).shape[1]
    c = np.zeros(k.shape[:3] + (N + 1, 2), dtype=np.int64)
    for kk in range(N + 1):
        for oo in range(2):
            c[:, :, :, kk, oo] = ((k == kk) & (o == oo) & valid[None]).sum(-1)
    return c


def reference(pred, y, thr, ev_var, ev_dir, w):
    """-> [n, E, N + 1, 2] fp64 in the documented order: rows ascending, product and sum rounded separately."""
    c = counts(pred, y, thr, ev_var, ev_dir)
    w = np.asarray(w, dtype=np.float64)
    acc = np.zeros(c.shape[:2] + c.shape[3:], dtype=np.float64)
    for h in range(c.shape[2]):
        term = w[h] * c[:, :, h].astype(np.float64)
        acc = acc + term
    return acc


def brier_direct(pred, y, thr, ev_var, ev_dir, w):
    """-> [n, E] fp64: sum of w[h] (k / N - o)^2 over the unmasked pixels / sum of w[h] over them (``math.fsum``-free numpy sums:
    the terms are non-negative and at most a few thousand)."""
    k, o, valid = _events(pred, y, thr, ev_var, ev_dir)
    N = np.asarray(pred).shape[1]
    wt = np.asarray(w, dtype=np.float64)[None, None, :, None] * valid[None]
    with np.errstate(divide="ignore", invalid="ignore"):
        return (wt * (k / np.float64(N) - o) ** 2).sum((-2, -1)) / np.broadcast_to(wt, k.shape).sum((-2, -1))


# ------------------------------------------------------------------------------------------------------- case generators
def make(kind, shape, E, seed=0):
    """(pred [n, N, V, H, W], y [n, V, H, W], thr [E, H, W]) fp32 of one of the kinds; thresholds are scalars broadcast unless the
    kind says otherwise."""
    n, N, V, H, W = shape
    rng = np.random.default_rng(seed)
    thr = np.zeros((E, H, W))
    if kind == "random":      # a per-pixel bias wider than the member spread: every k and both outcomes occur
        base = rng.standard_normal((n, 1, V, H, W)) * 1.5
        pred, y = base + rng.standard_normal(shape), base[:, 0] + rng.standard_normal((n, V, H, W))
        thr += rng.uniform(-0.3, 0.3, (E, 1, 1))
    elif kind == "identical":  # all members the same field: only k = 0 and k = N
        one = rng.standard_normal((n, 1, V, H, W))
        pred, y = np.broadcast_to(one, shape), rng.standard_normal((n, V, H, W))
    elif kind == "masked":     # a NaN band of rows and scattered NaN pixels in the threshold fields
        pred, y = rng.standard_normal(shape), rng.standard_normal((n, V, H, W))
        thr = rng.standard_normal((E, H, W)) * 0.5
        thr[:, H // 3:H // 3 + max(1, H // 4)] = np.nan
        thr[rng.random((E, H, W)) < 0.1] = np.nan
    elif kind == "t280":       # physical magnitude: 280 +- 0.01 K against 280
        pred, y = 280.0 + 0.01 * rng.standard_normal(shape), 280.0 + 0.01 * rng.standard_normal((n, V, H, W))
        thr += 280.0
    else:
        raise ValueError(kind)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return f(pred), f(y), f(thr)


def on_threshold(shape, ev_var, seed=0):
    """Design (b): event e sits on a channel whose members and truth all equal its threshold t_e (0 with both signs of zero for
    the first event of a channel, 2.5 + channel otherwise) -- one threshold per channel, so events sharing a channel share it."""
    n, N, V, H, W = shape
    pred, y = np.zeros(shape, dtype=np.float32), np.zeros((n, V, H, W), dtype=np.float32)
    level = [0.0 if v == ev_var[0] else 2.5 + v for v in range(V)]
    for v in range(V):
        pred[:, :, v], y[:, v] = level[v], level[v]
    pred[:, ::2, ev_var[0]] = -0.0                      # -0 members against a +0 threshold (and +0 members against it)
    y[:, ev_var[0], ::2] = -0.0
    thr = np.stack([np.full((H, W), level[v], dtype=np.float32) for v in ev_var])
    return pred, y, thr
