"""The yardstick of the zonal-power tests, checked on the CPU: the numpy reference obeys Parseval and places a harmonic where it
belongs, an emulation of the kernel's order of arithmetic in fp64 stays inside the per-bin bound of tests/spectrum_reference.py
on every case, and the same emulation in fp32 breaks it on every case -- the bound has teeth, and an fp32 transform would not do."""
import numpy as np
import pytest

import spectrum_reference as sp

CASES = sp.CPU_CASES + [c for c in sp.GPU_CASES if c not in sp.CPU_CASES]
IDS = [f"{kind}-{'x'.join(map(str, shape))}" for kind, shape in CASES]


@pytest.mark.parametrize("kind,shape", CASES, ids=IDS)
def test_reference_obeys_parseval(kind, shape):
    n, G, V, H, W = shape
    x, lat = sp.make(kind, shape, seed=3), sp.lat_of(H)
    ref = sp.reference(x, lat, group=G)
    assert ref.shape == (n, V, W // 2 + 1) and ref.dtype == np.float64 and np.all(ref >= 0)
    ms = sp.weighted_mean_square(x, lat, group=G)
    print("Parseval, worst relative difference", np.max(np.abs(ref.sum(-1) - ms) / ms))
    np.testing.assert_allclose(ref.sum(-1), ms, rtol=1e-13, atol=0)


def test_reference_puts_a_harmonic_into_its_bin():
    """a cos(2 pi k0 w / W + phase) on every row: a^2 / 2 in bin k0 (the weights' mean is 1) to fp32 rounding of the input."""
    H, W, k0, a = 6, 48, 7, 0.75
    w = np.arange(W)
    x = (a * np.cos(2 * np.pi * k0 * w / W + np.linspace(0, 3, H)[:, None])).astype(np.float32).reshape(1, 1, H, W)
    ref = sp.reference(x, sp.lat_of(H))[0, 0]
    assert ref[k0] == pytest.approx(a * a / 2, rel=1e-6)
    assert np.all(np.delete(ref, k0) < 1e-12 * ref[k0])


def test_reference_of_a_constant_plane():
    H, W, c = 5, 12, 3.25
    ref = sp.reference(np.full((1, 1, H, W), c, np.float32), sp.lat_of(H))[0, 0]
    assert ref[0] == pytest.approx(c * c, rel=1e-14) and np.all(ref[1:] <= sp.bound(ref, 1, H, W)[1:])


@pytest.mark.parametrize("kind,shape", CASES, ids=IDS)
def test_fp64_emulation_is_inside_the_bound_and_fp32_is_not(kind, shape):
    n, G, V, H, W = shape
    x, lat = sp.make(kind, shape, seed=3), sp.lat_of(H)
    ref = sp.reference(x, lat, group=G)
    bnd = sp.bound(ref, G, H, W)
    e64 = np.abs(sp.emulate(x, lat, group=G, dtype=np.float64) - ref)
    e32 = np.abs(sp.emulate(x, lat, group=G, dtype=np.float32).astype(np.float64) - ref)
    print(f"{kind} {shape}: fp64 emulation worst error / bound {np.max(e64 / bnd):.3g}, fp32 emulation {np.max(e32 / bnd):.3g}")
    assert np.all(e64 <= bnd)
    assert np.max(e32 / bnd) > 1.0
    if kind == "red":  # power falls as k^-3: the bound implies 1e-5 relative in every bin k >= 1
        assert np.all(bnd[..., 1:] <= 1e-5 * ref[..., 1:])
        print("  red, bins k >= 1: worst relative error", np.max(e64[..., 1:] / ref[..., 1:]))
        assert np.all(e64[..., 1:] <= 1e-5 * ref[..., 1:])
