"""Numpy statements of the sampler sweep's scoring (a helper, not a test): what ``swiftk_sweep_sse`` and
``swift_amd.eval.sampler`` are checked against.

``sweep_rows`` is the restatement the kernel is specified by (include/swiftk.h): per element the reference's fp32 arithmetic
with every rounding written out, per (sample, channel) an fp64 sum of the latitude-weighted squares.  ``reference_lines``
repeats the reference's own lines on ``C``-channel ``X`` -- ``v * s + m`` (data/era5.py:131, through ``unstandardize_x`` /
``unstandardize_t``, data/era5.py:155-170, residual means zero: data/era5.py:100), ``Y = X + Y``, ``T = X + T``,
``np.sum(w_lat * (Y - T) ** 2, axis=(0, 2, 3))`` (eval/sampler.py:97-105) -- and serves to cross-check the first
(tests/test_sweep_cpu.py): the two differ in the order of the fp64 additions only.
"""
import numpy as np

F = np.float32


def sweep_terms(x, y, t, mx, sx, st, w_lat, fused_x: bool = False):
    """[B, C, H, W] fp64 terms w_lat[h] * (double)q.  x [B, >=C, H, W], y / t [B, C, H, W], mx / sx / st [C], all fp32;
    w_lat [H] fp64.  ``fused_x``: xp as ONE rounding of x sx + mx (what a contracted multiply-add computes) instead of two."""
    y, t = np.asarray(y, F), np.asarray(t, F)
    C = y.shape[1]
    x = np.asarray(x, F)[:, :C]
    m, s, r = (np.asarray(v, F).reshape(1, C, 1, 1) for v in (mx, sx, st))
    if fused_x:  # the product of two fp32 values is exact in fp64; one rounding to fp32 after the addition
        xp = (x.astype(np.float64) * s.astype(np.float64) + m.astype(np.float64)).astype(F)
    else:
        xs = (x * s).astype(F)           # fl(x sx)
        xp = (xs + m).astype(F)          # fl(fl(x sx) + mx)
    xp = np.where(s == 0, np.broadcast_to(m, xp.shape), xp).astype(F)   # sx == 0: xp = mx (the zeroed SST channel)
    yr, tr = (y * r).astype(F), (t * r).astype(F)
    yp, tp = (xp + yr).astype(F), (xp + tr).astype(F)
    d = (yp - tp).astype(F)
    q = (d * d).astype(F)
    assert q.dtype == F
    return np.asarray(w_lat, np.float64).reshape(1, 1, -1, 1) * q.astype(np.float64)


def sweep_rows(x, y, t, mx, sx, st, w_lat, fused_x: bool = False):
    """[B, C] fp64: the sum of every (sample, channel)'s terms."""
    return sweep_terms(x, y, t, mx, sx, st, w_lat, fused_x).sum(axis=(2, 3))


def reference_lines(X, Y, T, mx, sx, st, w_lat):
    """The reference's lines, literally, on C-channel X: [C] fp64 sums over the batch and the grid."""
    C = Y.shape[1]
    m, s, r = (np.asarray(v, F).reshape(C, 1, 1) for v in (mx, sx, st))
    zero = np.zeros_like(r)
    w_lat = np.asarray(w_lat, np.float64)[None, None, :, None]
    X = np.asarray(X, F) * s + m           # unstandardize_x: v * s + m
    Y = np.asarray(Y, F) * r + zero        # unstandardize_t (residual means are zero)
    T = np.asarray(T, F) * r + zero
    assert X.dtype == Y.dtype == T.dtype == F
    # if residual
    Y = X + Y
    T = X + T
    return np.sum(w_lat * (Y - T) ** 2, axis=(0, 2, 3))


def random_case(seed, B, C, H, W, extra=2):
    """(x [B, C + extra, H, W], y, t, mx, sx, st, w_lat) with a non-uniform w_lat."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, C + extra, H, W)).astype(np.float32)
    y, t = (rng.standard_normal((B, C, H, W)).astype(np.float32) for _ in range(2))
    # means of both kinds: far above x sx (temperatures: the product's rounding vanishes in the sum) and of its own size (winds:
    # there a contracted x sx + mx rounds differently from the two-rounding form)
    mx = np.where(np.arange(C) % 2 == 0, 270.0 + rng.standard_normal(C), rng.standard_normal(C)).astype(np.float32)
    sx = (1.0 + np.abs(rng.standard_normal(C))).astype(np.float32)
    st = (0.1 + np.abs(rng.standard_normal(C))).astype(np.float32)
    w = np.cos(np.deg2rad(np.linspace(-88.0, 88.0, H)))
    return x, y, t, mx, sx, st, w / w.mean()
