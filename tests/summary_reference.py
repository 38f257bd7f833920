"""References for ``swiftk_ensemble_summary`` (include/swiftk.h): per-pixel mean, spread and quantiles of an ensemble.  A helper
module of the summary tests (no test here).

``reference_exact``   mean and unbiased variance of a pixel's members in rational arithmetic.  fp32 values are integer multiples
                      of 2^-149, so the member sum S, the deviations N x_m - S and the sum of their squares are Python integers
                      and the two statistics the fractions S / (N 2^149) and sqrt(sum (N x_m - S)^2 / (N^2 (N - 1))) / 2^149
                      (numerator and denominator kept as integers: ``fractions.Fraction`` without a gcd per operation); the
                      square root is an integer square root carrying 128 extra bits.  Each is rounded once, to fp64, on the way
                      out, by Python's correctly rounded int / int.
``quantiles_emulated``  ``np.sort`` over the members, then the definition's three fp64 operations a + g (b - a), then one cast.
``emulate64`` / ``emulate32``  the documented order of arithmetic of mean and spread in numpy fp64 / fp32 (numpy rounds every
                      operation separately and never fuses).

The bounds.  u = 2^-53, x_m the N members of a pixel, A = mean_m |x_m|, e = N u A.

mean.  The kernel adds the members in fp64 in member order: N - 1 rounded additions of partial sums of at most N A, error at most
(N - 1) u N A to first order; the division by N leaves (N - 1) u A and adds u |mean| <= u A: at most e before the cast.  The cast
to fp32 adds half an fp32 ulp of the value, at most 2^-24 |mean| for a normal result, 2^-150 < 2^-149 for a subnormal one:

    bound_mean   = 2^-24 |mean| + 2 e + 2^-149

spread.  Let delta <= e be the error of mean64.  sum (x_m - mean - delta)^2 = sum (x_m - mean)^2 + N delta^2 because the exact
deviations add up to zero, so the wrong centre moves the spread s by at most sqrt(N / (N - 1)) delta <= 2 e and by nothing to
first order.  The rounded arithmetic on top: each d_m once (2 u on its square), each product once (u), N - 1 additions ((N - 1) u),
the division (u): (N + 3) u relative on the variance, half of that on its root, u more for the root itself: below (N + 5) u s / 2.

    bound_spread = 2^-24 s + (N + 5) u s + 2 e + 2^-149

Each bound is half an fp32 ulp of the exact value plus the first-order fp64 error with a factor 2 of room (the one rounding of
the reference on its way to fp64, u |value|, disappears in that room).  Nothing in them is measured.  The half-ulp term dominates
by eight orders of magnitude, so error / bound cannot pass 1 unless the fp64 part is exceeded.
"""
from math import isqrt

import numpy as np

U = 2.0 ** -53
MEMBERS = (2, 3, 12, 13, 50, 64)              # the CPU checks' ensemble sizes
KINDS = ("normal", "t280", "z500", "mixed", "const")
_SCALE = 149                                  # fp32 values are integers in units of 2^-149
_EXTRA = 128                                  # extra bits of the integer square root


def make(kind, shape, seed=0):
    """pred [n, N, V, H, W] fp32: ``normal`` fields; ``t280`` 280 + 1e-2 noise (a temperature under a small spread); ``z500``
    5.5e4 + 30 noise (a geopotential height); ``mixed`` every value a normal draw times 10^U(-6, 5); ``const`` identical members."""
    n, N, V, H, W = shape
    r = np.random.default_rng(seed)
    g = r.standard_normal(shape)
    if kind == "normal":
        x = g
    elif kind == "t280":
        x = 280.0 + 1e-2 * g
    elif kind == "z500":
        x = 5.5e4 + 30.0 * g
    elif kind == "mixed":
        x = g * 10.0 ** r.uniform(-6.0, 5.0, size=shape)
    elif kind == "const":
        x = np.broadcast_to(280.0 + 30.0 * g[:, :1], shape)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, dtype=np.float32)


def _ints(pred):
    """The values in units of 2^-149 as Python integers (an object array): the scaling is a power of two and exact in fp64."""
    return np.frompyfunc(int, 1, 1)(pred.astype(np.float64) * 2.0 ** _SCALE)


def reference_exact(pred):
    """pred [n, N, V, H, W] fp32 -> (mean, spread, A), each [n, V, H, W] fp64: the exact mean, the exact unbiased standard
    deviation and the exact mean of |x_m|, each rounded once to fp64."""
    N = pred.shape[1]
    xi = _ints(pred)
    S = xi.sum(axis=1)
    D = N * xi - S[:, None]
    Vn = (D * D).sum(axis=1)                                       # N^2 (N - 1) variance, in units of 2^-298
    Aabs = np.frompyfunc(abs, 1, 1)(xi).sum(axis=1)
    den = N * N * (N - 1)

    def mean_of(s):                                                # (Python rounds int / int correctly: Fraction(s, d) without the gcd)
        return s / (N << _SCALE)

    def root_of(v):                                                # sqrt(v / den) 2^-149 = isqrt(v den 4^EXTRA) / (den 2^(149 + EXTRA))
        return isqrt(v * den << (2 * _EXTRA)) / (den << (_SCALE + _EXTRA))

    f = lambda fn, a: np.frompyfunc(fn, 1, 1)(a).astype(np.float64)
    return f(mean_of, S), f(root_of, Vn), f(mean_of, Aabs)


def bound_mean(mean, A, N):
    return 2.0 ** -24 * np.abs(mean) + 2.0 * N * U * A + 2.0 ** -149


def bound_spread(s, A, N):
    return 2.0 ** -24 * s + (N + 5) * U * s + 2.0 * N * U * A + 2.0 ** -149


def worst(got, ref, bound):
    """(every element within its bound, the largest error / bound); ``got`` is widened to fp64 first, which is exact."""
    e = np.abs(np.asarray(got, dtype=np.float64) - ref)
    return bool(np.all(e <= bound)), float(np.max(e / bound))


def quantiles_emulated(pred, lo, frac):
    """pred [n, N, V, H, W] fp32, the table of ``quantile_table`` -> [n, Q, V, H, W] fp32 by the definition: members sorted
    ascending, a = x_(lo), b = x_(min(lo + 1, N - 1)), (float)(a + g (b - a)) with difference, product and sum rounded to fp64."""
    N = pred.shape[1]
    xs = np.sort(pred, axis=1).astype(np.float64)
    out = []
    for l, g in zip(np.asarray(lo).tolist(), np.asarray(frac, dtype=np.float64)):
        l = min(max(int(l), 0), N - 1)
        a, b = xs[:, l], xs[:, min(l + 1, N - 1)]
        d = b - a
        p = g * d
        out.append((a + p).astype(np.float32))
    return np.stack(out, 1) if out else np.empty((pred.shape[0], 0) + pred.shape[2:], dtype=np.float32)


def _emulate(pred, dt):
    N = pred.shape[1]
    x = pred.astype(dt)
    s = np.zeros(pred.shape[:1] + pred.shape[2:], dtype=dt)
    for m in range(N):
        s = s + x[:, m]
    mean = s / dt(N)
    v = np.zeros_like(s)
    for m in range(N):
        d = x[:, m] - mean
        p = d * d
        v = v + p
    return mean.astype(np.float32), np.sqrt(v / dt(N - 1)).astype(np.float32)


def emulate64(pred):
    """(mean, spread) fp32 [n, V, H, W] by the kernel's order of arithmetic in numpy fp64."""
    return _emulate(pred, np.float64)


def emulate32(pred):
    """The same order of arithmetic in fp32: what a torch one-liner on the fp32 fields amounts to."""
    return _emulate(pred, np.float32)
