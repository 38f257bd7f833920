"""-m gpu: ``swiftk_event_table`` through ``swift_amd.eval.metrics.event_table`` against tests/events_reference.py, bit for bit
(``np.array_equal`` on the fp64 values, zeros and all): the contract fixes integer counts and one order of fp64 arithmetic, so it
leaves no rounding freedom.  Every case is a few thousand pixels.

Shapes (N, H, W, E), always n = 2 leads and V = 3 channels with the events on channels 2, 0, 2, (1, 1) -- member and plane
strides, two events on one channel: N = 1, 2, 3 and the maximum 64, 12 and 16 (the workload's; the last N whose N + 1 bins are
asserted to be hit), 33 (2 (N + 1) = 68 cell threads: more than a wave); H = 1, 5, 9, 17: below, not a multiple of, one more than
and two groups plus one of the 8-row group; W = 1, 255, 257, 300: both sides of the 256-thread stride."""
import numpy as np
import pytest
import torch

import events_reference as er

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 1, 1), (2, 5, 255, 3), (3, 9, 257, 5), (12, 17, 300, 3), (16, 9, 300, 5), (33, 5, 257, 3), (64, 17, 255, 1),
          (12, 9, 1, 3), (64, 1, 300, 5), (2, 17, 257, 1)]
n, V = 2, 3
EV_VAR, EV_DIR = [2, 0, 2, 1, 1], [0, 1, 1, 0, 1]


def _events(N, E):
    """(ev_var, ev_dir) of a case: the one event of an E = 1 case takes its direction from N, so both directions occur."""
    return EV_VAR[:E], ([N % 2] if E == 1 else EV_DIR[:E])


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def _run(dev, pred, y, thr, ev_var, ev_dir, lat):
    from swift_amd.eval.metrics import event_table
    out = event_table(torch.from_numpy(pred).to(dev), torch.from_numpy(y).to(dev), lat, ev_var, ev_dir, thr)
    assert out.dtype == torch.float64 and tuple(out.shape) == (pred.shape[0], len(ev_var), pred.shape[1] + 1, 2)
    return out.cpu().numpy()


def _check(dev, kind, shape, seed):
    N, H, W, E = shape
    ev_var, ev_dir = _events(N, E)
    pred, y, thr = er.make(kind, (n, N, V, H, W), E, seed=seed)
    lat = er.lat_of(H)
    ref = er.reference(pred, y, thr, ev_var, ev_dir, er.lat_weights(lat))
    got = _run(dev, pred, y, thr, ev_var, ev_dir, lat)
    assert np.array_equal(got, ref), (kind, shape, np.max(np.abs(got - ref)))
    return pred, y, thr, ref, got


@pytest.mark.parametrize("shape", SHAPES)
def test_random_fields_around_the_threshold(dev, shape):
    N, H, W, E = shape
    _, _, _, ref, _ = _check(dev, "random", shape, seed=11)
    if N <= 16 and H * W >= 1000:   # not vacuous: every forecast bin of every plane is hit, and both outcomes
        assert np.all(ref.sum(-1) > 0) and np.all(ref.sum(-2) > 0)


@pytest.mark.parametrize("shape", SHAPES)
def test_values_on_the_threshold_are_no_event(dev, shape):
    """Members and truth exactly on the threshold, -0 and +0 against a 0 threshold: strict comparisons put every pixel into
    cell (0, 0)."""
    N, H, W, E = shape
    ev_var, ev_dir = _events(N, E)
    pred, y, thr = er.on_threshold((n, N, V, H, W), ev_var)
    assert np.signbit(pred).any() and np.signbit(y).any() and not np.signbit(thr).any()
    lat = er.lat_of(H)
    w = er.lat_weights(lat)
    got = _run(dev, pred, y, thr, ev_var, ev_dir, lat)
    assert np.array_equal(got, er.reference(pred, y, thr, ev_var, ev_dir, w))
    total = np.float64(0.0)
    for h in range(H):
        total = total + w[h] * np.float64(W)
    assert np.all(got[:, :, 0, 0] == total) and np.all(got.reshape(n, E, -1)[:, :, 1:] == 0.0)


@pytest.mark.parametrize("shape", SHAPES)
def test_identical_members_fill_only_the_two_end_bins(dev, shape):
    N = shape[0]
    _, _, _, ref, got = _check(dev, "identical", shape, seed=12)
    assert np.all(got[:, :, 1:N] == 0.0)
    if shape[1] * shape[2] >= 1000:
        assert np.all(got[:, :, 0].sum(-1) > 0) and np.all(got[:, :, N].sum(-1) > 0)


@pytest.mark.parametrize("shape", SHAPES)
def test_nan_thresholds_mask_pixels(dev, shape):
    """A NaN band of rows and scattered NaN pixels: the cells of a plane sum to sum_h w_lat[h] #{unmasked pixels of row h} --
    bit for bit against the reference, and against the direct weighted count within the (N + H) roundings of the two sums."""
    N, H, W, E = shape
    _, _, thr, ref, got = _check(dev, "masked", shape, seed=13)
    assert np.isnan(thr).any()
    w = er.lat_weights(er.lat_of(H))
    direct = ((~np.isnan(thr)).sum(-1) * w[None]).sum(-1)                                     # [E]
    assert np.array_equal(got.sum((-2, -1)), ref.sum((-2, -1)))
    np.testing.assert_allclose(got.sum((-2, -1)), np.broadcast_to(direct, (n, E)), rtol=(2 * N + 2 * H + 4) * 2.0 ** -53, atol=0)
    full = np.full((E, H, W), np.nan, dtype=np.float32)                                        # everything masked: a zero table
    pred, y, _ = er.make("masked", (n, N, V, H, W), E, seed=13)
    assert np.all(_run(dev, pred, y, full, *_events(N, E), er.lat_of(H)) == 0.0)


@pytest.mark.parametrize("shape", SHAPES)
def test_physical_magnitude(dev, shape):
    _check(dev, "t280", shape, seed=14)


def test_a_planes_table_does_not_depend_on_its_batch(dev):
    """The same plane -- channel 2 of lead 1 under event 2 of the batch -- alone in a batch of its own (n = V = E = 1): the same bits."""
    N, H, W, E = 12, 17, 300, 5
    ev_var, ev_dir = _events(N, E)
    pred, y, thr = er.make("masked", (n, N, V, H, W), E, seed=15)
    lat = er.lat_of(H)
    big = _run(dev, pred, y, thr, ev_var, ev_dir, lat)
    for e in range(E):
        v = ev_var[e]
        alone = _run(dev, np.ascontiguousarray(pred[1:, :, v:v + 1]), np.ascontiguousarray(y[1:, v:v + 1]),
                     np.ascontiguousarray(thr[e:e + 1]), [0], [ev_dir[e]], lat)
        assert alone.shape == (1, 1, N + 1, 2) and np.array_equal(alone[0, 0], big[1, e]), e
    # and in another position: events reversed, the leads swapped
    back = _run(dev, np.ascontiguousarray(pred[::-1]), np.ascontiguousarray(y[::-1]), np.ascontiguousarray(thr[::-1]),
                ev_var[::-1], ev_dir[::-1], lat)
    assert np.array_equal(back[::-1, ::-1], big)


def test_a_channel_out_of_range_on_the_device_is_clamped(dev):
    """Device tables are taken as they are (the host arrays of ``parse_events`` are validated); the kernel clamps the channel into
    [0, V - 1], so the read stays inside pred and y."""
    from swift_amd.eval.metrics import event_table
    N, H, W = 3, 9, 257
    pred, y, thr = er.make("random", (n, N, V, H, W), 3, seed=16)
    lat = er.lat_of(H)
    tables = (torch.tensor([7, -3, 1], dtype=torch.int32, device=dev), torch.tensor([0, 1, 9], dtype=torch.int32, device=dev),
              torch.from_numpy(thr).to(dev))
    got = event_table(torch.from_numpy(pred).to(dev), torch.from_numpy(y).to(dev), lat, *tables).cpu().numpy()
    assert np.array_equal(got, er.reference(pred, y, thr, [2, 0, 1], [0, 1, 1], er.lat_weights(lat)))
    with pytest.raises(ValueError, match="event_table"):
        event_table(torch.from_numpy(pred).to(dev), torch.from_numpy(y).to(dev), lat, [7, -3, 1], [0, 1, 1], thr)


def test_a_non_contiguous_truth_view(dev):
    from swift_amd.eval.metrics import event_table
    N, H, W, E = 12, 9, 300, 3
    ev_var, ev_dir = _events(N, E)
    pred, y, thr = er.make("random", (n, N, V, H, W), E, seed=17)
    lat = er.lat_of(H)
    p, yy = torch.from_numpy(pred).to(dev), torch.from_numpy(y).to(dev)
    wide = torch.zeros(n, V, H, 2 * W, device=dev)
    wide[..., ::2] = yy
    view = wide[..., ::2]
    assert not view.is_contiguous() and torch.equal(view, yy)
    a, b = event_table(p, view, lat, ev_var, ev_dir, thr), event_table(p, yy, lat, ev_var, ev_dir, thr)
    assert torch.equal(a, b) and np.array_equal(b.cpu().numpy(), er.reference(pred, y, thr, ev_var, ev_dir, er.lat_weights(lat)))
