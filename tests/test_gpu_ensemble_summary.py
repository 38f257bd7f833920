"""-m gpu: ``swiftk_ensemble_summary`` / ``swift_amd.eval.metrics.ensemble_summary`` on the MI355X against the references of
tests/summary_reference.py: the quantile planes equal to the emulation of the definition in every element, mean and spread within
the bounds derived there of the exact (rational-arithmetic) values, identical members, ties and signed zeros, a complete write of
``out``, independence of batch and slot, refusals.  Shapes: two lead steps of two variables on 5 x 37 and 3 x 300 grids (odd, no
multiple of 4 or 64, more pixels in a row than a workgroup has threads), ensemble sizes on both sides of every padded size."""
import numpy as np
import pytest
import torch

import summary_reference as sr

pytestmark = pytest.mark.gpu
GRIDS = [(5, 37), (3, 300)]
MEMBERS = [2, 3, 4, 5, 12, 13, 33, 64]
QS = (0.0, 0.1, 0.25, 0.5, 0.9, 1.0)
n, V = 2, 2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def _run(dev, pred, qs=QS):
    from swift_amd.eval.metrics import ensemble_summary
    out = ensemble_summary(torch.from_numpy(pred).to(dev), qs)
    torch.cuda.synchronize()
    return out


def _table(N, qs=QS):
    from swift_amd.eval.metrics import quantile_table
    return quantile_table(qs, N)


def _raw(dev, pred, lo, frac):
    """The C entry with an explicit table into a NaN-filled buffer; ``lo`` / ``frac`` None: Q = 0 with null table pointers."""
    from swift_amd import _lib
    n_, N, V_, H, W = pred.shape
    Q = 0 if lo is None else len(lo)
    p = torch.from_numpy(pred).to(dev)
    tl = torch.from_numpy(np.asarray(lo, dtype=np.int32)).to(dev) if Q else None
    tf = torch.from_numpy(np.asarray(frac, dtype=np.float64)).to(dev) if Q else None
    out = torch.empty(n_, 2 + Q, V_, H, W, dtype=torch.float32, device=dev)
    out.fill_(float("nan"))
    _lib.check(_lib.lib().swiftk_ensemble_summary(p.data_ptr(), tl.data_ptr() if Q else None, tf.data_ptr() if Q else None,
                                                  out.data_ptr(), n_, N, V_, H, W, Q, torch.cuda.current_stream().cuda_stream),
               "swiftk_ensemble_summary")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("N", MEMBERS)
def test_quantiles_are_the_emulation_and_mean_and_spread_within_the_bounds(dev, N, grid):
    lo, frac = _table(N)
    for kind in ("normal", "t280", "mixed"):
        pred = sr.make(kind, (n, N, V, *grid), seed=3)
        out = _run(dev, pred)
        assert out.dtype == torch.float32 and tuple(out.shape) == (n, 2 + len(QS), V, *grid) and out.is_cuda
        got = out.cpu().numpy()
        assert np.array_equal(got[:, 2:], sr.quantiles_emulated(pred, lo, frac))
        assert np.array_equal(got[:, 2], pred.min(1)) and np.array_equal(got[:, 2 + len(QS) - 1], pred.max(1))
        mean, s, A = sr.reference_exact(pred)
        ok_m, w_m = sr.worst(got[:, 0], mean, sr.bound_mean(mean, A, N))
        ok_s, w_s = sr.worst(got[:, 1], s, sr.bound_spread(s, A, N))
        print(f"{kind} N={N} {grid}: worst error / bound: mean {w_m:.3g}, spread {w_s:.3g}")
        assert ok_m and ok_s


@pytest.mark.parametrize("N", [7, 8, 11, 15, 16, 19, 23, 27, 31, 32, 35, 39, 43, 47, 51, 55, 59, 63])
def test_every_kernel_of_the_family_sorts(dev, N):
    """One kernel per multiple of 4 members, each with its own sorting network: every one of them, one member short of full and
    full, on a tie-heavy and a tie-free plane."""
    lo, frac = _table(N)
    for pred in (sr.make("normal", (1, N, 1, 5, 37), seed=N),
                 np.random.default_rng(N).integers(-3, 4, size=(1, N, 1, 5, 37)).astype(np.float32)):
        got = _run(dev, pred).cpu().numpy()
        assert np.array_equal(got[:, 2:], sr.quantiles_emulated(pred, lo, frac))
        mean, s, A = sr.reference_exact(pred)
        assert sr.worst(got[:, 0], mean, sr.bound_mean(mean, A, N))[0] and sr.worst(got[:, 1], s, sr.bound_spread(s, A, N))[0]


@pytest.mark.parametrize("N", MEMBERS)
def test_identical_members_have_no_spread(dev, N):
    pred = sr.make("const", (n, N, V, 5, 37), seed=4)
    got = _run(dev, pred).cpu().numpy()
    assert np.all(got[:, 1] == 0.0) and not np.any(np.signbit(got[:, 1]))
    for k in [0] + list(range(2, 2 + len(QS))):
        assert np.array_equal(got[:, k], pred[:, 0])


@pytest.mark.parametrize("N", [3, 12, 33])
def test_ties_and_signed_zeros(dev, N):
    lo, frac = _table(N)
    r = np.random.default_rng(5)
    ties = r.integers(-2, 3, size=(n, N, V, 5, 37)).astype(np.float32)                       # five levels: ties everywhere
    zeros = np.where(r.random((n, N, V, 5, 37)) < 0.5, np.float32(-0.0), np.float32(0.0))     # -0 and +0 only
    mixed = np.where(r.random((n, N, V, 5, 37)) < 0.4, zeros, ties).astype(np.float32)
    for pred in (ties, zeros.astype(np.float32), mixed):
        got = _run(dev, np.ascontiguousarray(pred)).cpu().numpy()
        assert np.array_equal(got[:, 2:], sr.quantiles_emulated(pred, lo, frac))
        m64, s64 = sr.emulate64(pred)     # small integers: every sum is exact, the emulation is the exact answer rounded once
        assert np.array_equal(got[:, 0], m64)
        mean, s, A = sr.reference_exact(pred)
        assert sr.worst(got[:, 1], s, sr.bound_spread(s, A, N))[0]


@pytest.mark.parametrize("N", [2, 12, 64])
def test_out_is_written_completely_and_the_index_is_clamped(dev, N):
    pred = sr.make("normal", (n, N, V, 3, 300), seed=6)
    lo, frac = _table(N)
    got = _raw(dev, pred, lo, frac)                      # (the buffer was NaN before the call)
    assert np.all(np.isfinite(got)) and np.array_equal(got, _run(dev, pred).cpu().numpy())
    bare = _raw(dev, pred, None, None)                   # Q = 0: mean and spread only, null table pointers
    assert bare.shape == (n, 2, V, 3, 300) and np.array_equal(bare, got[:, :2])
    wild = _raw(dev, pred, [-7, 1000, N - 1], [0.0, 0.5, 0.75])   # indices outside [0, N - 1] are clamped, b stops at the maximum
    assert np.array_equal(wild[:, 2], pred.min(1)) and np.array_equal(wild[:, 3], pred.max(1))
    assert np.array_equal(wild[:, 4], pred.max(1))


@pytest.mark.parametrize("N,H,W", [(5, 5, 37), (40, 3, 300)], ids=["N5-5x37", "N40-3x300"])
def test_a_plane_does_not_depend_on_batch_or_slot(dev, N, H, W):
    """One plane's members alone and as plane (i = 1, v = 1) of the batch: the same bits; a second call: the same bits again."""
    p1 = sr.make("t280", (1, N, 1, H, W), seed=7)
    pb = sr.make("normal", (n, N, V, H, W), seed=8)
    pb[1, :, 1] = p1[0, :, 0]
    alone, again = _run(dev, p1), _run(dev, p1)
    inside, inside_again = _run(dev, pb), _run(dev, pb)
    assert torch.equal(alone, again) and torch.equal(inside, inside_again)
    assert torch.equal(alone[0, :, 0], inside[1, :, 1])
    assert not torch.equal(alone[0, :, 0], inside[0, :, 0])  # (other planes do differ)


def test_the_python_function_refuses_what_the_kernel_cannot_take(dev):
    from swift_amd.eval.metrics import ensemble_summary
    pred = sr.make("normal", (1, 3, 1, 3, 8), seed=9)
    with pytest.raises(ValueError, match="ensemble_summary"):
        ensemble_summary(torch.from_numpy(pred))                                                # CPU tensor
    p = torch.from_numpy(pred).to(dev)
    with pytest.raises(ValueError, match="ensemble_summary"):
        ensemble_summary(p.double())
    with pytest.raises(ValueError, match="ensemble_summary"):
        ensemble_summary(p[0])                                                                  # wrong rank
    with pytest.raises(ValueError, match="ensemble_summary"):
        ensemble_summary(p[:, :1])                                                              # one member has no spread
    with pytest.raises(ValueError, match="quantile"):
        ensemble_summary(p, (0.5, 1.5))
    with pytest.raises(ValueError, match="quantile"):
        ensemble_summary(p, [0.5] * 17)
    assert tuple(ensemble_summary(p, ()).shape) == (1, 2, 1, 3, 8)                              # no quantiles: legal
