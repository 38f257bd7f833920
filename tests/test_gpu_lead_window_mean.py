"""-m gpu: ``swiftk_lead_window_mean`` (swift_amd/csrc/lead_mean.hip) through ``swift_amd.eval.metrics.lead_window_mean`` and
through the raw C ABI, bit for bit against tests/windows_reference.py.

The definition leaves no rounding freedom (an fp64 running sum from the window's first row, rows ascending, one division, one
cast), so every comparison is of bits; tests/test_windows_reference_cpu.py shows that an fp32 running sum misses those bits on
more than half the columns of the physical design at counts 28 and 240, which this file's shapes include.

Shapes: M in {1, 3, 4, 255, 1025, 4100, 2^22 + 3} -- below one vector, no multiple of 4 (dword form only), one vector, below and
just above a 1024-column block, a multiple of 4 with a partly filled last block (the vector form's tail), and more than the
2048 x 1024 columns of one grid pass -- times n in {1, 2, 7, 240} (below, and no multiple of, the 8 rows in flight: the 4 / 2 / 1
remainders all occur) times nw in {1, 3, 8, 11} (every kernel instantiation; 11 is two launches).  Every case runs from a
16-byte-aligned base (the vector form where M allows it) and from a base one float further on (the dword form) on the same data.
At 2^22 + 3 columns the leads stay short (7 and 2) so the case takes about a second.

Measured on MI355X: no output differs from the reference in any case, from either base; the file runs in 2.9 s (the grid-stride
case 0.95 s, the 64-bit case 0.86 s).  On the parent commit every test here fails: the symbol and the function do not exist."""
import ctypes

import numpy as np
import pytest
import torch

import windows_reference as wr

pytestmark = pytest.mark.gpu
SENTINEL = float("nan")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def windows_for(n, nw):
    """nw windows over n rows: whole, single step, last step only, two overlapping, nested, two disjoint halves, first step only,
    and three more in another order (a later window may begin before an earlier one)."""
    h, t = max(n // 2, 1), max(n // 3, 1)
    cand = [(0, n), (n // 2, 1), (n - 1, 1), (0, max(2 * n // 3, 1)), (n // 3, n - n // 3), (min(1, n - 1), max(n - 2, 1)), (0, h),
            (n // 2, n - n // 2), (0, 1), (n - t, t), (min(2, n - 1), 1)]
    first, count = [c[0] for c in cand[:nw]], [c[1] for c in cand[:nw]]
    assert all(0 <= f and c >= 1 and f + c <= n for f, c in zip(first, count))
    return first, count


def offset_view(x, dev):
    """x on the device in a buffer whose base is one float past a 16-byte boundary: [n, M] contiguous, 4-byte aligned only."""
    buf = torch.empty(x.size + 4, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + x.size].view(x.shape)
    v.copy_(torch.from_numpy(x))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def raw_call(x, first, count, out=None):
    """The C ABI itself on at most 8 windows; ``out`` pre-filled with NaN so that equality with the reference shows every element written."""
    from swift_amd import _lib
    n, M = x.shape[0], x.numel() // x.shape[0]
    if out is None:
        out = torch.full((len(first), M), SENTINEL, dtype=torch.float32, device=x.device)
    f, c = (ctypes.c_int * len(first))(*first), (ctypes.c_int * len(count))(*count)
    rc = _lib.lib().swiftk_lead_window_mean(x.data_ptr(), out.data_ptr(), f, c, n, len(first), M, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out


def bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.uint32)


def check_case(dev, x, first, count, what):
    from swift_amd.eval.metrics import lead_window_mean
    ref = bits(wr.window_mean_ref(x, first, count))
    xa = torch.from_numpy(x).to(dev)
    assert xa.data_ptr() % 16 == 0
    got_a = lead_window_mean(xa, first, count)
    got_o = lead_window_mean(offset_view(x, dev), first, count)
    assert got_a.shape == (len(first),) + x.shape[1:] and got_a.dtype == torch.float32
    ba, bo = bits(got_a), bits(got_o)
    print(f"{what}: aligned base {int((ba != ref).sum())} and offset base {int((bo != ref).sum())} of {ref.size} outputs differ from the "
          f"reference in bits, {int((ba != bo).sum())} between the two forms (must all be 0)")
    assert np.array_equal(ba, ref) and np.array_equal(bo, ref), what
    if len(first) <= 8:
        rc, out = raw_call(xa, first, count)
        assert rc == 0 and np.array_equal(bits(out), ref.reshape(len(first), -1)), what       # the NaN pre-fill is gone everywhere
        # the output row one float off a 16-byte boundary as well
        buf = torch.full((len(first) * x.shape[1] + 4,), SENTINEL, dtype=torch.float32, device=dev)
        rc, _ = raw_call(xa, first, count, buf[1:])
        assert rc == 0 and np.array_equal(bits(buf[1:-3]), ref.reshape(-1)) and bool(buf[0].isnan()) and bool(buf[-3:].isnan().all()), what


@pytest.mark.parametrize("M", [1, 3, 4, 255, 1025, 4100])
def test_bits_equal_the_reference_at_every_small_shape(dev, M):
    for n in (1, 2, 7, 240):
        for design in ("integer", "physical"):
            x = (wr.integer_design if design == "integer" else wr.physical_design)(n, M, seed=n)
            for nw in (1, 3, 8, 11):
                first, count = windows_for(n, nw)
                check_case(dev, x, first, count, f"{design} M {M} n {n} nw {nw}")


def test_integer_design_counts_1_2_4_8_are_the_exact_means(dev):
    """Counts that are powers of two on multiples of 2^-3: the reference is the exact rational mean (CPU test), so the kernel is."""
    x = wr.integer_design(16, 4100)
    first, count = [5, 0, 3, 8, 12, 1, 15, 6], [1, 2, 4, 8, 4, 8, 1, 2]
    check_case(dev, x, first, count, "integer counts 1 2 4 8")
    want = np.stack([x[f:f + c].astype(np.float64).sum(0) / c for f, c in zip(first, count)])
    from swift_amd.eval.metrics import lead_window_mean
    assert np.array_equal(lead_window_mean(torch.from_numpy(x).to(dev), first, count).cpu().numpy().astype(np.float64), want)


def test_physical_design_at_counts_28_and_240(dev):
    """The counts at which the CPU test shows an fp32 running sum to miss the reference's bits on most columns."""
    x = wr.physical_design(240, 4100)
    check_case(dev, x, [0, 0, 28, 212, 100], [240, 28, 28, 28, 56], "physical counts 240 28 56")


def test_a_grid_stride_pass(dev):
    """2^22 + 3 columns: 4097 blocks of 1024 for a grid of 2048, the last block holding 3 columns; not a multiple of 4, so both
    bases take the dword form -- and 2^22 + 4 columns from an aligned base, the vector form through the same stride loop."""
    M = 2 ** 22 + 3
    x = wr.physical_design(7, M + 1)
    check_case(dev, np.ascontiguousarray(x[:, :M]), *windows_for(7, 3), what=f"physical M 2^22+3 n 7 nw 3")
    check_case(dev, x, [0, 5, 2], [7, 2, 3], what=f"physical M 2^22+4 n 7 nw 3")
    y = wr.integer_design(2, M)
    check_case(dev, y, *windows_for(2, 8), what=f"integer M 2^22+3 n 2 nw 8")


def test_a_count_of_one_returns_the_input_bits(dev):
    x = wr.physical_design(7, 1025)
    tiny = np.float32(1e-45)
    x[3, :8] = [-0.0, 0.0, tiny, -tiny, np.float32(1.1754942e-38), np.inf, -np.inf, np.float32(3.4028235e38)]
    x[3, 1020:1025] = [-0.0, tiny, -np.inf, 0.0, -0.0]
    first, count = [3, 0, 6, 3], [1, 1, 1, 1]
    check_case(dev, x, first, count, "count 1")
    from swift_amd.eval.metrics import lead_window_mean
    got = lead_window_mean(torch.from_numpy(x).to(dev), first, count).cpu().numpy()
    assert got[0].tobytes() == x[3].tobytes() and got[3].tobytes() == x[3].tobytes() and got[1].tobytes() == x[0].tobytes()
    assert np.signbit(got[0, 0]) and np.signbit(got[0, 1024]) and got[0, 2] == tiny
    # -0 survives only a window of one: -0 + -0 is -0, -0 + 0 is +0, as IEEE has it and the reference too
    z = np.zeros((2, 4), np.float32)
    z[:, :2] = -0.0
    z[1, 1] = 0.0
    check_case(dev, z, [0], [2], "signed zeros")


def test_nan_and_inf_show_up_only_in_the_windows_that_hold_their_lead(dev):
    from swift_amd.eval.metrics import lead_window_mean
    n, M = 7, 1025
    x = wr.physical_design(n, M)
    x[4, 10], x[4, 11], x[4, 12], x[4, 1024] = np.nan, np.inf, -np.inf, np.nan
    x[2, 12] = np.inf                                                     # +inf and -inf in one window: NaN
    first, count = [0, 4, 5, 0, 3, 2, 4, 6], [7, 1, 2, 4, 2, 2, 3, 1]
    holds4 = [f <= 4 < f + c for f, c in zip(first, count)]
    ref = wr.window_mean_ref(x, first, count)
    for xd in (torch.from_numpy(x).to(dev), offset_view(x, dev)):
        got = lead_window_mean(xd, first, count).cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(ref))               # positions, not payloads
        ok = ~np.isnan(ref)
        assert np.array_equal(got[ok].view(np.uint32), ref[ok].view(np.uint32))
        for w, h in enumerate(holds4):
            assert bool(np.isnan(got[w, 10])) == h and bool(np.isnan(got[w, 1024])) == h
            assert bool(np.isfinite(got[w, 11])) != h
        assert np.isnan(got[0, 12]) and got[1, 12] == -np.inf and np.isnan(got[5, 12]) == False and got[5, 12] == np.inf
        assert int(np.isnan(got).sum()) == 2 * sum(holds4) + 1            # nothing leaks into a neighbouring column


def test_rows_outside_every_window_are_never_used(dev):
    from swift_amd.eval.metrics import lead_window_mean
    n, M = 23, 4100
    x = wr.physical_design(n, M)
    first, count = [2, 9, 20, 3], [3, 4, 1, 1]                           # rows 0-1, 5-8, 13-19 and 21-22 lie in no window
    used = np.zeros(n, bool)
    for f, c in zip(first, count):
        used[f:f + c] = True
    x[~used] = np.nan
    assert (~used).sum() == 15
    check_case(dev, x, first, count, "NaN rows outside the windows")
    got = lead_window_mean(torch.from_numpy(x).to(dev), first, count)
    assert not bool(got.isnan().any())


def test_index_arithmetic_is_64_bit(dev):
    """n = 3, M = 2^30 + 5: row 1 crosses element 2^31 at column 2^30 - 5 and the out rows do too.  x is zeros with planted
    columns at both ends, around 2^31 / n and around that crossing; the planted columns against the reference, every other
    output zero (counted on the device)."""
    from swift_amd.eval.metrics import lead_window_mean
    free, _ = torch.cuda.mem_get_info(dev)
    if free < 40e9:
        pytest.skip(f"{free / 1e9:.0f} GB free on the device, 40 GB wanted")
    n, M = 3, 2 ** 30 + 5
    third, cross = 2 ** 31 // n, 2 ** 30 - 5
    cols = np.array([0, 1, 2, 3, 4, third - 1, third, third + 1, cross - 1, cross, cross + 1, M - 5, M - 4, M - 3, M - 2, M - 1], dtype=np.int64)
    vals = wr.physical_design(n, cols.size, seed=64)
    vals[vals == 0] = 1.0
    first, count = [0, 1, 2], [3, 2, 1]
    x = torch.zeros(n, M, dtype=torch.float32, device=dev)
    x[:, torch.from_numpy(cols).to(dev)] = torch.from_numpy(vals).to(dev)
    out = lead_window_mean(x, first, count)
    torch.cuda.synchronize()
    del x
    ref = wr.window_mean_ref(vals, first, count)
    got = out[:, torch.from_numpy(cols).to(dev)].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert int(np.count_nonzero(ref)) == ref.size
    assert sum(int(torch.count_nonzero(out[w])) for w in range(len(first))) == ref.size
    del out
    torch.cuda.empty_cache()


def test_refusals_return_their_codes_and_launch_nothing(dev):
    x = torch.from_numpy(wr.physical_design(4, 8)).to(dev)
    out = torch.full((8, 8), 7.0, dtype=torch.float32, device=dev)
    from swift_amd import _lib
    L = _lib.lib()
    ints = lambda *a: (ctypes.c_int * len(a))(*a)
    call = lambda xp, op, f, c, n, nw, M: L.swiftk_lead_window_mean(xp, op, f, c, n, nw, M, torch.cuda.current_stream().cuda_stream)
    xp, op = x.data_ptr(), out.data_ptr()
    assert call(None, op, ints(0), ints(1), 4, 1, 8) == -1 and call(xp, None, ints(0), ints(1), 4, 1, 8) == -1
    assert call(xp, op, None, ints(1), 4, 1, 8) == -1 and call(xp, op, ints(0), None, 4, 1, 8) == -1
    assert call(xp, op, ints(0), ints(1), 0, 1, 8) == -1 and call(xp, op, ints(0), ints(1), 4, 0, 8) == -1
    assert call(xp, op, ints(0), ints(1), 4, 1, 0) == -1 and call(xp, op, ints(0), ints(1), -4, 1, 8) == -1
    assert call(xp, op, ints(*[0] * 9), ints(*[1] * 9), 4, 9, 8) == -2
    assert call(xp, op, ints(-1), ints(1), 4, 1, 8) == -2 and call(xp, op, ints(0), ints(0), 4, 1, 8) == -2
    assert call(xp, op, ints(3), ints(2), 4, 1, 8) == -2 and call(xp, op, ints(0, 4), ints(4, 1), 4, 2, 8) == -2
    assert call(xp + 2, op, ints(0), ints(1), 4, 1, 4) == -3 and call(xp, op + 1, ints(0), ints(1), 4, 1, 4) == -3
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    from swift_amd.eval.metrics import lead_window_mean
    for bad in ((x, [0], [5]), (x, [-1], [1]), (x, [0], [0]), (x, [0, 1], [1]), (x, [], []), (x.double(), [0], [1]), (x.t(), [0], [1]),
                (x.cpu(), [0], [1]), (x, [0.5], [1])):
        with pytest.raises(ValueError, match="lead_window_mean"):
            lead_window_mean(*bad)
    assert lead_window_mean(x, [0], [4]).shape == (1, 8) and lead_window_mean(x.view(4, 2, 4), [1, 0], [2, 1]).shape == (2, 2, 4)
