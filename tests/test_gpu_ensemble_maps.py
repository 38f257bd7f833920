"""-m gpu: ``swiftk_ensemble_maps`` / ``swift_amd.eval.metrics.ensemble_maps`` on the MI355X against the references of
tests/maps_reference.py: every element of the fp64 buffer equal, bit for bit, to the numpy emulation of the documented order of
arithmetic, and within the derived bound of the exact (rational-arithmetic) terms; a complete write without ``accumulate``,
accumulation over three calls, independence of a plane's position, identical members, the wrapper.  Shapes (n, N, V, H, W): the
smallest that can go wrong -- one pixel, odd sizes, two lead steps and three variables at the job's 12 members, a row wider than
a workgroup (and than the 4 x 256 pixels a small ensemble's workgroup takes), ensemble sizes on both sides of the padded sizes
and in each of the kernel's pixels-per-thread forms (N <= 4, <= 8, beyond)."""
import functools

import numpy as np
import pytest
import torch

import maps_reference as mr

pytestmark = pytest.mark.gpu
SHAPES = [(1, 2, 1, 1, 1), (1, 3, 2, 3, 5), (2, 12, 3, 5, 67), (1, 13, 1, 2, 257), (1, 33, 1, 3, 9), (1, 64, 2, 2, 33)]
KINDS = ("normal", "t280", "z2e5")
_id = lambda s: "x".join(map(str, s))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@functools.lru_cache(maxsize=None)
def case(kind, shape, seed=3):
    """(pred, y, emulation) of a field, computed once and shared (treat as read-only)."""
    pred, y = mr.make(kind, shape, seed=seed)
    return pred, y, mr.emulate(pred, y)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _raw(dev, pred, y, acc=None):
    """The C entry: into a NaN-filled buffer with accumulate = 0, into ``acc`` (a device tensor, changed in place) with 1."""
    from swift_amd import _lib
    n, N, V, H, W = pred.shape
    p, t = torch.from_numpy(pred).to(dev), torch.from_numpy(y).to(dev)
    out = acc if acc is not None else torch.full((n, 4, V, H, W), float("nan"), dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().swiftk_ensemble_maps(p.data_ptr(), t.data_ptr(), out.data_ptr(), n, N, V, H, W, int(acc is not None),
                                               torch.cuda.current_stream().cuda_stream), "swiftk_ensemble_maps")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_the_kernel_is_the_emulation_bit_for_bit_and_within_the_bound_of_the_exact_terms(dev, shape):
    N = shape[1]
    for kind in KINDS:
        pred, y, emu = case(kind, shape)
        got = _raw(dev, pred, y).cpu().numpy()                # (the buffer was NaN before the call)
        assert not np.any(np.isnan(got))
        diff = got.view(np.int64) != emu.view(np.int64)
        print(f"{kind} {shape}: {int(diff.sum())} of {diff.size} elements differ from the emulation")
        assert bits_equal(got, emu)
        ref, bnd = mr.exact(pred, y), mr.bound(N, pred, y)
        for s, name in enumerate(mr.STATISTICS):
            ok, worst = mr.within(got[:, s], ref[:, s], bnd[:, s])
            print(f"{kind} {shape} {name}: worst error / bound {worst:.3g}")
            assert ok


@pytest.mark.parametrize("N", [4, 5, 8, 9, 16, 17, 20, 24, 28, 31, 36, 40, 44, 48, 52, 56, 60, 61])
def test_every_kernel_of_the_family(dev, N):
    """One kernel per multiple of 4 members: each of them on a ragged plane, full or one past the previous size."""
    pred, y, emu = case("t280", (1, N, 2, 3, 90), seed=N)
    assert bits_equal(_raw(dev, pred, y).cpu().numpy(), emu)


@pytest.mark.parametrize("shape", [(2, 3, 2, 3, 5), (2, 12, 3, 5, 67), (1, 64, 2, 2, 33)], ids=_id)
def test_three_accumulating_calls_are_the_emulation(dev, shape):
    fields = [mr.make(kind, shape, seed=20 + i) for i, kind in enumerate(("t280", "normal", "z2e5"))]
    acc, emu = None, None
    for pred, y in fields:
        acc = _raw(dev, pred, y, acc)
        emu = mr.emulate(pred, y, emu)
        assert bits_equal(acc.cpu().numpy(), emu)


@pytest.mark.parametrize("N,H,W", [(5, 5, 37), (12, 3, 300), (40, 2, 257)], ids=["N5-5x37", "N12-3x300", "N40-2x257"])
def test_a_plane_does_not_depend_on_its_position(dev, N, H, W):
    """One plane's members and truth alone, and as plane (i = 1, v = 2) of a batch: the same bits, also when accumulating."""
    p1, y1 = mr.make("t280", (1, N, 1, H, W), seed=7)
    pb, yb = mr.make("normal", (2, N, 3, H, W), seed=8)
    pb[1, :, 2], yb[1, 2] = p1[0, :, 0], y1[0, 0]
    alone, inside = _raw(dev, p1, y1), _raw(dev, pb, yb)
    assert torch.equal(alone[0, :, 0], inside[1, :, 2]) and torch.equal(alone, _raw(dev, p1, y1))
    assert not torch.equal(alone[0, :, 0], inside[0, :, 0])  # (other planes do differ)
    alone, inside = _raw(dev, p1, y1, alone), _raw(dev, pb, yb, inside)
    assert torch.equal(alone[0, :, 0], inside[1, :, 2])
    assert bits_equal(alone.cpu().numpy(), mr.emulate(p1, y1, mr.emulate(p1, y1)))


@pytest.mark.parametrize("N", [2, 3, 12, 13, 33, 64])
def test_identical_members_have_no_spread(dev, N):
    pred, y = mr.make("const", (2, N, 2, 5, 37), seed=4)
    got = _raw(dev, pred, y).cpu().numpy()
    d = pred[:, 0].astype(np.float64) - y
    assert np.all(got[:, 3] == 0.0) and not np.any(np.signbit(got[:, 3]))
    assert bits_equal(got[:, 0], d) and bits_equal(got[:, 1], d * d) and bits_equal(got[:, 2], np.abs(d))   # p = 0 exactly


def test_the_wrapper_is_the_raw_call(dev):
    from swift_amd.eval.metrics import ensemble_maps
    shape = (2, 12, 3, 5, 67)
    pred, y, emu = case("t280", shape)
    p, t = torch.from_numpy(pred).to(dev), torch.from_numpy(y).to(dev)
    out = ensemble_maps(p, t)
    assert out.dtype == torch.float64 and tuple(out.shape) == (2, 4, 3, 5, 67) and out.is_cuda and out.is_contiguous()
    assert torch.equal(out, _raw(dev, pred, y)) and bits_equal(out.cpu().numpy(), emu)
    pred2, y2 = mr.make("normal", shape, seed=5)
    back = ensemble_maps(torch.from_numpy(pred2).to(dev), torch.from_numpy(y2).to(dev), out)
    assert back is out                                                                           # accumulated in place
    assert torch.equal(out, _raw(dev, pred2, y2, _raw(dev, pred, y))) and bits_equal(out.cpu().numpy(), mr.emulate(pred2, y2, emu))
    # non-contiguous inputs are taken by value
    wide = torch.from_numpy(np.concatenate([pred, pred], axis=-1)).to(dev)
    assert torch.equal(ensemble_maps(wide[..., :67], t), _raw(dev, pred, y))
    for bad in (out.float(), out[:1], out.cpu(), out.transpose(-1, -2), out.cpu().numpy()):
        with pytest.raises(ValueError, match="ensemble_maps"):
            ensemble_maps(p, t, bad)
    for bp, bt in ((p, t[:1]), (p, t.double()), (p[:, :1], t), (p, t.cpu()), (p[0], t)):
        with pytest.raises(ValueError, match="ensemble_maps"):
            ensemble_maps(bp, bt)
