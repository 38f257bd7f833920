"""numpy reference of ``swiftk_zonal_power`` (include/swiftk.h), its per-bin error bound, two emulations of the kernel's order of
arithmetic (fp64 and fp32), and the case generators of the spectrum tests.

Definition.  A plane is x[h, w], H latitudes, W longitudes (W even), wavenumbers k = 0 .. W/2, K = W/2 + 1:

    X_h(k) = sum_w x[h,w] exp(-2 pi i k w / W)
    P_h(k) = c_k |X_h(k)|^2 / W^2,  c_0 = c_{W/2} = 1, otherwise 2         (one-sided: sum_k P_h(k) = mean_w x[h,w]^2)
    P(k)   = (1/H) sum_h w_lat[h] P_h(k),  w_lat = cos(lat) / mean(cos(lat))

With G > 1 the transform is taken of the mean over G consecutive planes.  The reference is ``np.fft.rfft`` of the fp32 input
widened to fp64.

Bound.  bound_k = eps sqrt(ref_k T) + eps^2 T with T = sum_k ref_k and eps = (16 W + 2 H + 4 G) 2^-53:
|X^|^2 - |X|^2 = 2 Re(conj(X) d) + |d|^2 with |d| <= gamma_W sum_w |x| <= gamma_W W rms_row; Cauchy-Schwarz over the rows gives
sqrt(ref_k T); 2 H and 4 G cover the sum over rows and the member mean; the 16 is an eightfold margin over the first-order 2 W u
for the table's own rounding and the reference's.  Nothing in it is measured.
"""
import numpy as np

U = 2.0 ** -53


def lat_of(H):
    """Cell-centre latitudes of an H-row grid (no pole row: every weight is positive)."""
    return -90.0 + (np.arange(H, dtype=np.float64) + 0.5) * (180.0 / H)


def lat_weights(lat):
    w = np.cos(np.deg2rad(np.asarray(lat, dtype=np.float64)))
    return w / w.mean()


def twiddle(W):
    a = 2.0 * np.pi * np.arange(W, dtype=np.float64) / W
    return np.stack([np.cos(a), np.sin(a)], 1)


def one_sided(W):
    c = np.full(W // 2 + 1, 2.0)
    c[0] = c[-1] = 1.0
    return c


def reference(x, lat, group=1):
    """x [n, G, V, H, W] (or [n, V, H, W] with group 1) fp32 -> [n, V, K] fp64."""
    x = np.asarray(x)
    assert x.dtype == np.float32
    if x.ndim == 4 and group == 1:
        x = x[:, None]
    n, G, V, H, W = x.shape
    assert G == group and W % 2 == 0
    xm = x.astype(np.float64).mean(axis=1)
    p = one_sided(W) * np.abs(np.fft.rfft(xm, axis=-1)) ** 2 / float(W) ** 2          # [n, V, H, K]
    return (lat_weights(lat).reshape(1, 1, H, 1) * p).sum(axis=2) / H


def weighted_mean_square(x, lat, group=1):
    """What a spectrum sums to (Parseval): the latitude-weighted mean square of the (member-mean) plane, [n, V] fp64."""
    x = np.asarray(x)
    if x.ndim == 4 and group == 1:
        x = x[:, None]
    xm = x.astype(np.float64).mean(axis=1)
    return (lat_weights(lat).reshape(1, 1, -1, 1) * xm * xm).mean(axis=(2, 3))


def eps_of(G, H, W):
    return (16 * W + 2 * H + 4 * G) * U


def bound(ref, G, H, W):
    """Per-bin absolute bound for spectra ``ref`` [..., K] of planes of shape (G, H, W)."""
    e = eps_of(G, H, W)
    T = ref.sum(axis=-1, keepdims=True)
    return e * np.sqrt(ref * T) + e * e * T


def emulate(x, lat, group=1, dtype=np.float64):
    """The kernel's order of arithmetic in ``dtype``: members added in member order and multiplied by 1/G, a direct sum over w
    with the table entry (k w) mod W, squares, rows added in row order.  (No fused multiply-add: numpy has none.)"""
    x = np.asarray(x)
    if x.ndim == 4 and group == 1:
        x = x[:, None]
    n, G, V, H, W = x.shape
    K = W // 2 + 1
    t = twiddle(W).astype(dtype)
    wl = lat_weights(lat).astype(dtype)
    xs = x[:, 0].astype(dtype)
    for g in range(1, G):
        xs = xs + x[:, g].astype(dtype)
    if G > 1:
        xs = xs * dtype(1.0 / G)
    k = np.arange(K)
    re, im = np.zeros((n, V, H, K), dtype), np.zeros((n, V, H, K), dtype)
    for w in range(W):
        idx = (k * w) % W
        re = re + xs[..., w, None] * t[idx, 0]
        im = im + xs[..., w, None] * t[idx, 1]
    p = re * re + im * im
    acc = np.zeros((n, V, K), dtype)
    for h in range(H):
        acc = acc + wl[h] * p[:, :, h]
    assert acc.dtype == dtype
    return one_sided(W).astype(dtype) * acc / dtype(float(W) * W * H)


# ------------------------------------------------------------------------------------------------------- case generators
def make(kind, shape, seed=0):
    """fp32 [n, G, V, H, W] of one of the four kinds; phases and noise from ``seed``."""
    n, G, V, H, W = shape
    rng = np.random.default_rng(seed)
    w = np.arange(W, dtype=np.float64)
    if kind == "rand":
        x = rng.standard_normal(shape)
    elif kind == "red":  # power falls as k^-3
        ks = np.arange(1, W // 2 + 1, dtype=np.float64)
        phi = rng.uniform(0, 2 * np.pi, (n, G, V, H, 1, ks.size))
        x = (ks ** -1.5 * np.cos(2 * np.pi * ks * w[:, None] / W + phi)).sum(-1)
    elif kind == "hostile":  # a temperature-like mean of 280 under two waves of 1e-2, one at the top of the spectrum
        phi = rng.uniform(0, 2 * np.pi, (n, G, V, H, 1))
        x = 280.0 + 0.01 * np.cos(2 * np.pi * 5 * w / W + phi) + 0.01 * np.cos(2 * np.pi * (W // 2 - 1) * w / W)
    elif kind == "const":
        x = np.full(shape, 3.25)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, dtype=np.float32)


# (kind, (n, G, V, H, W)): the smallest shapes at which the kernel can go wrong
GPU_CASES = [("rand", (2, 1, 2, 3, 8)),        # K = 5, fewer rows than a row group
             ("rand", (2, 3, 2, 5, 12)),       # non-power-of-two wrap of the table index, odd H, member mean
             ("red", (1, 1, 1, 4, 64)),        # steep spectrum
             ("hostile", (1, 1, 1, 4, 64)),    # large mean under small waves
             ("red", (2, 1, 3, 128, 256)),     # the workload's plane size
             ("hostile", (2, 1, 3, 128, 256)),
             ("const", (1, 4, 1, 2, 256))]     # ensemble-mean path at the workload's row width
# the shapes the emulations are run at on the CPU (the direct sum in numpy is slow at 128 x 256)
CPU_CASES = [("rand", (2, 1, 2, 3, 8)), ("rand", (2, 3, 2, 5, 12)), ("red", (1, 1, 1, 4, 64)), ("hostile", (1, 1, 1, 4, 64)),
             ("hostile", (1, 1, 1, 2, 256)), ("red", (1, 1, 1, 2, 256))]
