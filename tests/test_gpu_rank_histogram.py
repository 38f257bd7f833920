"""-m gpu: ``swiftk_rank_histogram`` / ``swift_amd.eval.metrics.rank_histogram`` on the MI355X against the exact reference of
tests/rank_reference.py: tie-free counts bit for bit, tie-heavy fields within the per-bin bound derived there (nothing in it is
measured) with zero bins exactly zero, the constant plane, the truth outside the ensemble, independence of batch size and slot,
a complete write of ``out``, refusals before any launch."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import rank_reference as rr

pytestmark = pytest.mark.gpu
IDS = ["x".join(map(str, s)) for s in rr.SHAPES]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def _run(dev, pred, y, lat):
    from swift_amd.eval.metrics import rank_histogram
    out = rank_histogram(torch.from_numpy(pred).to(dev), torch.from_numpy(y).to(dev), lat)
    torch.cuda.synchronize()
    return out


def _raw(dev, pred, y, w):
    """The C entry with explicit weights (``w`` need not come from latitudes) into a NaN-filled ``torch.empty`` buffer."""
    from swift_amd import _lib
    n, N, V, H, W = pred.shape
    p, t = torch.from_numpy(pred).to(dev), torch.from_numpy(y).to(dev)
    wl = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).to(dev)
    out = torch.empty(n, V, N + 1, dtype=torch.float64, device=dev)
    out.fill_(float("nan"))
    _lib.check(_lib.lib().swiftk_rank_histogram(p.data_ptr(), t.data_ptr(), wl.data_ptr(), out.data_ptr(), n, N, V, H, W,
                                                torch.cuda.current_stream().cuda_stream), "swiftk_rank_histogram")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("shape", rr.SHAPES, ids=IDS)
def test_tie_free_fields_with_unit_weights_give_the_integer_counts(dev, shape):
    n, N, V, H, W = shape
    pred, y = rr.make("gauss", shape, seed=1)
    assert not np.any(pred == y[:, None])
    got = _raw(dev, pred, y, np.ones(H))
    counts = np.stack([((pred < y[:, None]).sum(1) == r).sum((-1, -2)) for r in range(N + 1)], -1).astype(np.float64)
    assert got.shape == (n, V, N + 1) and np.array_equal(got, counts)


@pytest.mark.parametrize("shape", rr.SHAPES, ids=IDS)
def test_tie_heavy_fields_within_the_bound(dev, shape):
    n, N, V, H, W = shape
    lat = rr.lat_of(H)
    pred, y = rr.make("ties", shape, seed=2)
    ref = rr.reference(pred, y, rr.lat_weights(lat))
    out = _run(dev, pred, y, lat)
    assert out.dtype == torch.float64 and tuple(out.shape) == (n, V, N + 1) and out.is_cuda
    ok, worst = rr.within(out.cpu().numpy(), ref, H, N)
    print(f"ties {shape}: worst error / bound {worst:.3g}")
    assert ok
    total = float(W * sum(Fraction(float(x)) for x in rr.lat_weights(lat)))
    # the bins' bounds add up to bound * total; adding N + 1 of them in fp64 and rounding `total` cost (N + 2) u more
    assert np.all(np.abs(out.cpu().numpy().sum(-1) - total) <= (rr.bound(H, N) + (N + 2) * rr.U) * total)


@pytest.mark.parametrize("N", [15, 16, 31, 32])
def test_both_sides_of_the_row_group_thresholds(dev, N):
    """The launcher takes 8 rows per group up to N = 15, 4 up to 31, 2 above: H = 9 leaves a partial group in each."""
    shape = (1, N, 2, 9, 70)
    lat = rr.lat_of(9)
    pred, y = rr.make("ties", shape, seed=8)
    ok, worst = rr.within(_run(dev, pred, y, lat).cpu().numpy(), rr.reference(pred, y, rr.lat_weights(lat)), 9, N)
    print(f"ties {shape}: worst error / bound {worst:.3g}")
    assert ok
    pred, y = rr.make("gauss", shape, seed=9)
    counts = np.stack([((pred < y[:, None]).sum(1) == r).sum((-1, -2)) for r in range(N + 1)], -1).astype(np.float64)
    assert not np.any(pred == y[:, None]) and np.array_equal(_raw(dev, pred, y, np.ones(9)), counts)


@pytest.mark.parametrize("shape", rr.SHAPES, ids=IDS)
def test_a_constant_plane_fills_every_bin_alike(dev, shape):
    n, N, V, H, W = shape
    lat = rr.lat_of(H)
    pred, y = rr.make("const", shape)
    got = _run(dev, pred, y, lat).cpu().numpy()
    each = float(W * sum(Fraction(float(x)) for x in rr.lat_weights(lat)) / (N + 1))
    assert np.all(got == got[..., :1])
    assert np.all(np.abs(got - each) <= rr.bound(H, N) * each)


@pytest.mark.parametrize("shape", rr.SHAPES, ids=IDS)
def test_truth_outside_the_ensemble_fills_one_end_bin(dev, shape):
    n, N, V, H, W = shape
    lat = rr.lat_of(H)
    total = float(W * sum(Fraction(float(x)) for x in rr.lat_weights(lat)))
    for kind, full in (("below", 0), ("above", N)):
        pred, y = rr.make(kind, shape, seed=4)
        got = _run(dev, pred, y, lat).cpu().numpy()
        assert np.all(np.abs(got[..., full] - total) <= rr.bound(H, N) * total)
        assert np.all(np.delete(got, full, axis=-1) == 0.0)


@pytest.mark.parametrize("N,H,W", [(5, 6, 70), (40, 3, 300)], ids=["N5-6x70", "N40-3x300"])
def test_rows_do_not_depend_on_batch_or_slot(dev, N, H, W):
    """One plane's values alone and as plane (i = 2, v = 1) of a 3 x 2 batch: the same bits; a second call: the same bits again."""
    lat = rr.lat_of(H)
    p1, y1 = rr.make("ties", (1, N, 1, H, W), seed=11)
    pb, yb = rr.make("ties", (3, N, 2, H, W), seed=12)
    pb[2, :, 1], yb[2, 1] = p1[0, :, 0], y1[0, 0]
    alone, again = _run(dev, p1, y1, lat), _run(dev, p1, y1, lat)
    inside, inside_again = _run(dev, pb, yb, lat), _run(dev, pb, yb, lat)
    assert torch.equal(alone, again) and torch.equal(inside, inside_again)
    assert torch.equal(alone[0, 0], inside[2, 1])
    assert not torch.equal(alone[0, 0], inside[0, 0])  # (other planes do differ)


@pytest.mark.parametrize("shape", rr.SHAPES, ids=IDS)
def test_out_is_written_completely(dev, shape):
    n, N, V, H, W = shape
    pred, y = rr.make("ties", shape, seed=6)
    got = _raw(dev, pred, y, rr.lat_weights(rr.lat_of(H)))   # (the buffer was NaN before the call)
    assert np.all(np.isfinite(got))


def test_refusals_come_before_any_launch(dev):
    """Host-side checks: nothing is launched, so the bad pointers are never dereferenced."""
    from swift_amd import _lib
    L = _lib.lib()
    n, N, V, H, W = 2, 3, 2, 3, 8
    pred = torch.zeros(n, 65, V, H, W + 1, device=dev)     # (large enough for the N = 64 call below)
    y = torch.zeros(n, V, H, W + 1, device=dev)
    wl = torch.ones(H + 1, dtype=torch.float64, device=dev)
    out = torch.empty(n * V * 65 + 1, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()

    def call(pp=pred.data_ptr(), yp=y.data_ptr(), wp=wl.data_ptr(), op=out.data_ptr(), n_=n, m=N, v=V, h=H, w=W):
        return L.swiftk_rank_histogram(pp, yp, wp, op, n_, m, v, h, w, st)

    assert call() == 0 and call(m=64) == 0
    assert call(m=65) == -2                                                                     # SWIFTK_ESHAPE
    assert call(n_=1 << 20, v=1 << 12) == -2                                                    # n V beyond the grid
    assert call(pp=None) == call(yp=None) == call(wp=None) == call(op=None) == -1               # SWIFTK_EINVAL
    assert call(n_=0) == call(m=0) == call(v=-1) == call(h=0) == call(w=0) == -1
    assert call(pp=pred.data_ptr() + 2) == call(yp=y.data_ptr() + 2) == -3                      # SWIFTK_EALIGN
    assert call(wp=wl.data_ptr() + 4) == call(op=out.data_ptr() + 4) == -3
    torch.cuda.synchronize()


def test_the_python_function_refuses_what_the_kernel_cannot_take(dev):
    from swift_amd.eval.metrics import rank_histogram
    pred, y = rr.make("gauss", (1, 2, 1, 3, 8), seed=7)
    lat = rr.lat_of(3)
    with pytest.raises(ValueError, match="rank_histogram"):
        rank_histogram(torch.from_numpy(pred), torch.from_numpy(y), lat)                        # CPU tensors
    p, t = torch.from_numpy(pred).to(dev), torch.from_numpy(y).to(dev)
    with pytest.raises(ValueError, match="latitudes"):
        rank_histogram(p, t, rr.lat_of(4))
    with pytest.raises(ValueError, match="rank_histogram"):
        rank_histogram(p.double(), t, lat)
    with pytest.raises(ValueError, match="rank_histogram"):
        rank_histogram(p[0], t, lat)                                                            # wrong rank
