"""-m gpu: ``swiftk_zonal_power`` / ``swift_amd.eval.metrics.zonal_power`` on the MI355X against the numpy reference of
tests/spectrum_reference.py: every bin of every plane within the per-bin bound derived there (nothing in it is measured; an fp32
emulation of the same arithmetic misses it by six orders of magnitude, tests/test_spectrum_reference_cpu.py), Parseval on the
device output, independence of batch size and slot, refusals before any launch."""
import numpy as np
import pytest
import torch

import spectrum_reference as sp

pytestmark = pytest.mark.gpu
IDS = [f"{kind}-{'x'.join(map(str, shape))}" for kind, shape in sp.GPU_CASES]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def _run(dev, x, lat, group):
    from swift_amd.eval.metrics import zonal_power
    out = zonal_power(torch.from_numpy(x).to(dev), lat, group=group)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("kind,shape", sp.GPU_CASES, ids=IDS)
def test_every_bin_within_the_bound(dev, kind, shape):
    n, G, V, H, W = shape
    x, lat = sp.make(kind, shape, seed=3), sp.lat_of(H)
    ref = sp.reference(x, lat, group=G)
    bnd = sp.bound(ref, G, H, W)
    out = _run(dev, x, lat, G)
    assert out.dtype == torch.float64 and tuple(out.shape) == (n, V, W // 2 + 1) and out.is_cuda
    got = out.cpu().numpy()
    assert np.all(np.isfinite(got)) and np.all(got >= 0)
    err = np.abs(got - ref)
    print(f"{kind} {shape}: worst error / bound {np.max(err / bnd):.3g}")
    assert np.all(err <= bnd)
    # Parseval on the device output: the bins' bounds add up to at most eps (sqrt(K) + eps K) T (Cauchy-Schwarz over k)
    ms = sp.weighted_mean_square(x, lat, group=G)
    K, e = W // 2 + 1, sp.eps_of(G, H, W)
    print("  Parseval, worst relative difference", np.max(np.abs(got.sum(-1) - ms) / ms))
    assert np.all(np.abs(got.sum(-1) - ms) <= (e * (np.sqrt(K) + e * K) + 1e-13) * ms)
    if kind == "red":  # the bound is below 1e-5 of every bin k >= 1 (asserted on the CPU): so is the error
        print("  red, bins k >= 1: worst relative error", np.max(err[..., 1:] / ref[..., 1:]))
        assert np.all(err[..., 1:] <= 1e-5 * ref[..., 1:])
    if kind == "const":  # only bin 0, and it is c^2 mean(w_lat) = c^2
        c2 = float(x.flat[0]) ** 2
        assert np.all(np.abs(got[..., 0] - c2) <= bnd[..., 0]) and np.all(got[..., 1:] <= bnd[..., 1:])


def test_group_1_takes_four_dimensions(dev):
    x, lat = sp.make("rand", (2, 1, 2, 3, 8), seed=5), sp.lat_of(3)
    a, b = _run(dev, x, lat, 1), _run(dev, x[:, 0], lat, 1)
    assert b.dtype == torch.float64 and tuple(b.shape) == (2, 2, 5) and torch.equal(a, b)


@pytest.mark.parametrize("G,H,W", [(3, 5, 12), (1, 128, 256)], ids=["G3-5x12", "G1-128x256"])
def test_rows_do_not_depend_on_batch_or_slot(dev, G, H, W):
    """One plane's values at n = 0 of a batch of 1 and at n = 2, v = 1 of a batch of 3 x 2: the same bits; a second call on the
    same input: the same bits again."""
    lat = sp.lat_of(H)
    plane = sp.make("rand", (1, G, 1, H, W), seed=11)
    batch = sp.make("rand", (3, G, 2, H, W), seed=12)
    batch[2, :, 1] = plane[0, :, 0]
    alone, again = _run(dev, plane, lat, G), _run(dev, plane, lat, G)
    inside, inside_again = _run(dev, batch, lat, G), _run(dev, batch, lat, G)
    assert torch.equal(alone, again) and torch.equal(inside, inside_again)
    assert torch.equal(alone[0, 0], inside[2, 1])
    assert not torch.equal(alone[0, 0], inside[0, 0])  # (other planes do differ)


def test_refusals_come_before_any_launch(dev):
    """Host-side checks: nothing is launched, so the bad pointers are never dereferenced."""
    from swift_amd import _lib
    L = _lib.lib()
    n, G, V, H, W = 2, 1, 2, 3, 8
    x = torch.zeros(n, G, V, H, W + 1, device=dev)
    wl, tw, out = (torch.ones(m, dtype=torch.float64, device=dev) for m in (H + 1, 2 * W + 3, n * V * (W // 2 + 1) + 1))
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()

    def call(xp=x.data_ptr(), wp=wl.data_ptr(), tp=tw.data_ptr(), op=out.data_ptr(), n_=n, g=G, v=V, h=H, w=W):
        return L.swiftk_zonal_power(xp, wp, tp, op, n_, g, v, h, w, st)

    assert call() == 0
    assert call(w=7) == call(w=2) == call(w=2050) == -2                                        # SWIFTK_ESHAPE
    assert call(n_=1 << 20, v=1 << 12) == -2                                                    # n V beyond the grid
    assert call(op=None) == call(xp=None) == call(wp=None) == call(tp=None) == -1               # SWIFTK_EINVAL
    assert call(n_=0) == call(g=0) == call(v=-1) == call(h=0) == call(w=0) == -1
    assert call(xp=x.data_ptr() + 2) == -3                                                      # SWIFTK_EALIGN
    assert call(wp=wl.data_ptr() + 4) == call(tp=tw.data_ptr() + 4) == call(op=out.data_ptr() + 4) == -3
    torch.cuda.synchronize()
    with pytest.raises(_lib.SwiftkError, match="SWIFTK_ESHAPE"):
        _run(dev, np.zeros((1, 1, 1, 2, 6 + 1), np.float32), sp.lat_of(2), 1)
