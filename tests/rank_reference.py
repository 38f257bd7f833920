"""Exact reference of ``swiftk_rank_histogram`` (include/swiftk.h), its per-bin error bound, an fp64 emulation of the kernel's
order of arithmetic, and the case generators of the rank-histogram tests.

Definition.  pred [n, N, V, H, W], y [n, V, H, W] fp32, w [H] fp64.  At pixel (h, w) of plane (i, v) let b = #{m: x_m < y} and
e = #{m: x_m == y} (IEEE comparisons: -0 ties with +0).  The pixel adds w[h] / (e + 1) to every bin r with b <= r <= b + e:
the usual rank without ties; with ties the unit mass is spread evenly over the ranks the truth could take.  Hence
sum_r out[i, v, r] = W sum_h w[h], and an all-equal plane gives every bin the same value.

``reference`` evaluates this exactly: integer counts T_h[e][r], ``fractions.Fraction`` per bin with ``Fraction(float(w[h]))``
for the weights, rounded to fp64 once at the end.

Bound.  ``bound(H, N)`` = (H + N + 8) 2^-53, relative, per bin.  The kernel counts in exact integers; floating point enters in
three places, all fp64: row[r] = sum over e ascending of T_h[e][r] / (e + 1), acc[r] += w[h] * row[r], rows added in ascending
h.  Every term is non-negative, so relative errors do not amplify: at most N + 1 rounded quotients and N additions per row,
one product per row, H - 1 additions over rows -- (H + N + 1) u to first order.  The remaining 7 u is margin for the final
rounding of the reference and for a fused multiply-add in place of product and sum.  Nothing in it is measured.  A bin that
is exactly 0 in the reference is a sum of zeros in the kernel: exactly 0.0.
"""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53


def lat_of(H):
    """Cell-centre latitudes of an H-row grid (no pole row: every weight is positive)."""
    return -90.0 + (np.arange(H, dtype=np.float64) + 0.5) * (180.0 / H)


def lat_weights(lat):
    w = np.cos(np.deg2rad(np.asarray(lat, dtype=np.float64)))
    return w / w.mean()


def bound(H, N):
    """Relative, per bin."""
    return (H + N + 8) * U


def tables(pred, y):
    """The integer tables T [n, V, H, N + 1 (e), N + 1 (r)]: pixels of row h with tie size e whose range [b, b + e] covers r."""
    pred, y = np.asarray(pred), np.asarray(y)
    assert pred.dtype == np.float32 and y.dtype == np.float32 and pred.ndim == 5 and y.shape == pred.shape[:1] + pred.shape[2:]
    n, N, V, H, W = pred.shape
    b = (pred < y[:, None]).sum(1)                                   # [n, V, H, W]
    e = (pred == y[:, None]).sum(1)
    r = np.arange(N + 1)
    covers = (b[..., None] <= r) & (r <= (b + e)[..., None])         # [n, V, H, W, r]
    T = np.zeros((n, V, H, N + 1, N + 1), dtype=np.int64)
    for k in range(N + 1):
        T[:, :, :, k] = (covers & (e[..., None] == k)).sum(3)
    return T


def reference(pred, y, w):
    """pred [n, N, V, H, W], y [n, V, H, W] fp32, w [H] fp64 -> [n, V, N + 1] fp64: the definition evaluated exactly, one rounding."""
    T = tables(pred, y)
    n, V, H, B, _ = T.shape
    wf = [Fraction(float(x)) for x in np.asarray(w, dtype=np.float64)]
    out = np.zeros((n, V, B), dtype=np.float64)
    for i in range(n):
        for v in range(V):
            for r in range(B):
                s = Fraction(0)
                for h in range(H):
                    col = T[i, v, h, :, r]
                    q = sum((Fraction(int(col[k]), int(k) + 1) for k in np.nonzero(col)[0]), Fraction(0))  # (python ints)
                    s += wf[h] * q
                out[i, v, r] = float(s)
    return out


def emulate(pred, y, w):
    """The kernel's order of arithmetic in fp64: per row the quotients T_h[e][r] / (e + 1) added over e ascending, one product
    with w[h], rows added in ascending h (product and sum rounded separately: numpy has no fused multiply-add)."""
    T = tables(pred, y).astype(np.float64)
    n, V, H, B, _ = T.shape
    w = np.asarray(w, dtype=np.float64)
    acc = np.zeros((n, V, B), dtype=np.float64)
    for h in range(H):
        row = np.zeros((n, V, B), dtype=np.float64)
        for k in range(B):
            row = row + T[:, :, h, k] / np.float64(k + 1)
        acc = acc + w[h] * row
    return acc


def within(got, ref, H, N):
    """(every bin within the bound and zero bins exactly zero, worst error / bound)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err, lim = np.abs(got - ref), bound(H, N) * ref
    ok = bool(np.all(err <= lim)) and bool(np.all(got[ref == 0.0] == 0.0))
    worst = float(np.max(err[ref > 0] / lim[ref > 0])) if np.any(ref > 0) else 0.0
    return ok, worst


# ------------------------------------------------------------------------------------------------------- case generators
def make(kind, shape, seed=0):
    """(pred [n, N, V, H, W], y [n, V, H, W]) fp32 of one of the kinds."""
    n, N, V, H, W = shape
    rng = np.random.default_rng(seed)
    if kind == "gauss":      # tie-free (asserted by the tests that rely on it)
        pred, y = rng.standard_normal(shape), rng.standard_normal((n, V, H, W))
    elif kind == "ties":     # values from {0, 1, 2}: every tie size occurs
        pred, y = rng.integers(0, 3, shape), rng.integers(0, 3, (n, V, H, W))
    elif kind == "const":    # every member equals the truth (with -0 among the members: it ties with +0)
        pred, y = np.full(shape, 0.0), np.full((n, V, H, W), 0.0)
        pred[:, ::2] = -0.0
    elif kind == "below":    # truth below every member: bin 0
        pred, y = rng.standard_normal(shape), np.full((n, V, H, W), -100.0)
    elif kind == "above":    # truth above every member: bin N
        pred, y = rng.standard_normal(shape), np.full((n, V, H, W), 100.0)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(pred, dtype=np.float32), np.ascontiguousarray(y, dtype=np.float32)


# (n, N, V, H, W): N = 1 and the maximum, a row shorter than a wave, a width that is no multiple of 64 and exceeds 256, more rows
# than any row group, n V > 1
SHAPES = [(1, 1, 1, 1, 1), (2, 2, 3, 3, 20), (1, 12, 2, 5, 257), (2, 64, 1, 4, 96), (1, 7, 2, 130, 64)]
