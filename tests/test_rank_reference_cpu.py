"""Properties of the exact rank-histogram reference of tests/rank_reference.py on the CPU, at the shapes the GPU test uses: what a
histogram sums to, invariance under a permutation of the members, the constant plane, the truth outside the ensemble, and the
fp64 emulation of the kernel's order of arithmetic against the bound derived there."""
from fractions import Fraction

import numpy as np
import pytest

import rank_reference as rr

IDS = ["x".join(map(str, s)) for s in rr.SHAPES]


def _weights(H):
    return rr.lat_weights(rr.lat_of(H))


@pytest.mark.parametrize("shape", rr.SHAPES, ids=IDS)
def test_each_row_sums_to_the_weight_of_the_plane(shape):
    n, N, V, H, W = shape
    w = _weights(H)
    total = float(W * sum(Fraction(float(x)) for x in w))
    for kind in ("gauss", "ties"):
        pred, y = rr.make(kind, shape, seed=1)
        ref = rr.reference(pred, y, w)
        assert ref.shape == (n, V, N + 1) and ref.dtype == np.float64 and np.all(ref >= 0)
        # N + 1 bins, each rounded once, added in fp64: (2 N + 2) u relative
        assert np.all(np.abs(ref.sum(-1) - total) <= (2 * N + 2) * rr.U * total)
    # tie-free data with unit weights: the bins are pixel counts
    pred, y = rr.make("gauss", shape, seed=1)
    assert not np.any(pred == y[:, None])
    ref = rr.reference(pred, y, np.ones(H))
    assert np.array_equal(ref, np.round(ref)) and np.all(ref.sum(-1) == H * W)
    counts = np.stack([((pred < y[:, None]).sum(1) == r).sum((-1, -2)) for r in range(N + 1)], -1)
    assert np.array_equal(ref, counts.astype(np.float64))


@pytest.mark.parametrize("shape", rr.SHAPES, ids=IDS)
def test_the_order_of_the_members_does_not_matter(shape):
    n, N, V, H, W = shape
    w = _weights(H)
    pred, y = rr.make("ties", shape, seed=2)
    perm = np.random.default_rng(3).permutation(N)
    assert np.array_equal(rr.reference(pred, y, w), rr.reference(np.ascontiguousarray(pred[:, perm]), y, w))


@pytest.mark.parametrize("shape", rr.SHAPES, ids=IDS)
def test_a_constant_plane_fills_every_bin_alike(shape):
    n, N, V, H, W = shape
    w = _weights(H)
    pred, y = rr.make("const", shape)
    ref = rr.reference(pred, y, w)
    assert np.all(ref == ref[..., :1])
    assert np.all(ref == float(W * sum(Fraction(float(x)) for x in w) / (N + 1)))


@pytest.mark.parametrize("shape", rr.SHAPES, ids=IDS)
def test_truth_outside_the_ensemble_fills_one_end_bin(shape):
    n, N, V, H, W = shape
    w = _weights(H)
    total = float(W * sum(Fraction(float(x)) for x in w))
    for kind, full in (("below", 0), ("above", N)):
        pred, y = rr.make(kind, shape, seed=4)
        ref = rr.reference(pred, y, w)
        assert np.all(ref[..., full] == total)
        assert np.all(np.delete(ref, full, axis=-1) == 0.0)


@pytest.mark.parametrize("shape", rr.SHAPES, ids=IDS)
def test_the_kernels_order_of_arithmetic_stays_within_the_bound(shape):
    n, N, V, H, W = shape
    w = _weights(H)
    for kind in ("gauss", "ties", "const", "below", "above"):
        pred, y = rr.make(kind, shape, seed=5)
        ok, worst = rr.within(rr.emulate(pred, y, w), rr.reference(pred, y, w), H, N)
        print(f"{kind} {shape}: worst error / bound {worst:.3g}")
        assert ok
    # with unit weights and no ties nothing is rounded at all
    pred, y = rr.make("gauss", shape, seed=5)
    assert np.array_equal(rr.emulate(pred, y, np.ones(H)), rr.reference(pred, y, np.ones(H)))


def test_negative_zero_ties_with_zero_and_ties_share_the_mass():
    """One pixel, three members (-0, 1, -1) against the truth +0: b = 1, e = 1 -> half the weight in bins 1 and 2."""
    pred = np.array([-0.0, 1.0, -1.0], dtype=np.float32).reshape(1, 3, 1, 1, 1)
    y = np.zeros((1, 1, 1, 1), dtype=np.float32)
    assert rr.reference(pred, y, np.array([0.75])).tolist() == [[[0.0, 0.375, 0.375, 0.0]]]
