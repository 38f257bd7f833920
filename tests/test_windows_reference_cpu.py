"""CPU checks of the lead-window yardstick (tests/windows_reference.py) and of the host side of ``generate --lead-windows``: the
reference returns a one-step window bit for bit, gives the exact rational mean on the integer design, and differs in bits from an
fp32-accumulating mean on most columns of the physical design -- so bit-equality with it on the GPU
(tests/test_gpu_lead_window_mean.py) rejects an fp32 kernel; ``parse_lead_windows`` and ``check_windows_args`` refuse what they
must, naming the spec."""
import argparse
from fractions import Fraction

import numpy as np
import pytest

import windows_reference as wr


def test_a_window_of_one_step_returns_its_input_bit_for_bit():
    x = wr.physical_design(5, 64)
    tiny = np.float32(1e-45)                                                # the smallest subnormal
    x[2, :8] = [-0.0, 0.0, tiny, -tiny, np.float32(1.1754942e-38), np.inf, -np.inf, np.float32(3.4028235e38)]
    out = wr.window_mean_ref(x, [2, 0, 4], [1, 1, 1])
    assert out.dtype == np.float32
    assert out[0].tobytes() == x[2].tobytes() and out[1].tobytes() == x[0].tobytes() and out[2].tobytes() == x[4].tobytes()
    assert np.signbit(out[0, 0]) and not np.signbit(out[0, 1]) and out[0, 2] == tiny and out[0, 2] != 0


def test_integer_design_gives_the_exact_rational_mean():
    x = wr.integer_design(8, 257)
    first, count = [0, 3, 2, 4, 0, 7], [1, 2, 4, 4, 8, 1]
    out = wr.window_mean_ref(x, first, count)
    for w, (f, c) in enumerate(zip(first, count)):
        for j in range(x.shape[1]):
            want = sum(Fraction(float(v)) for v in x[f:f + c, j]) / c
            assert Fraction(float(out[w, j])) == want, (w, j)


@pytest.mark.parametrize("count", [28, 240])
def test_an_fp32_running_sum_differs_in_bits_on_most_physical_columns(count):
    x = wr.physical_design(count, 4100)
    ref, f32 = wr.window_mean_ref(x, [0], [count])[0], wr.window_mean_fp32(x, [0], [count])[0]
    differ = ref.view(np.uint32) != f32.view(np.uint32)
    print(f"count {count}: fp32 running sum differs from the fp64 reference on {differ.mean():.3f} of the columns "
          f"(280 K columns {differ[0::2].mean():.3f}, 2e5 columns {differ[1::2].mean():.3f})")
    assert differ.mean() > 0.5
    # and the reference itself is the correctly rounded mean up to the fp64 sum's own error: far inside half an fp32 ulp
    exact = x.astype(np.float64).sum(0) / count
    assert np.all(np.abs(ref.astype(np.float64) - exact) <= 0.5000001 * np.spacing(np.abs(ref)).astype(np.float64))


def test_parse_lead_windows_accepts_and_names():
    from swift_amd.eval.metrics import parse_lead_windows
    names, first, count = parse_lead_windows(["6-6", "6-168", "12-24h"], 28, 6)
    assert names == ["6-6h", "6-168h", "12-24h"]
    assert first.dtype == count.dtype == np.int32 and first.tolist() == [0, 0, 1] and count.tolist() == [1, 28, 3]
    names, first, count = parse_lead_windows(["24-48"], 4, 12)
    assert names == ["24-48h"] and first.tolist() == [1] and count.tolist() == [3]


@pytest.mark.parametrize("specs, bad", [(["6-5"], "6-5"), (["0-6"], "0-6"), (["7-12"], "7-12"), (["6-30"], "6-30"), (["a-b"], "a-b"),
                                        (["6-12", "12-24", "6-12h"], "6-12h"), (["6-12", "6--12"], "6--12"), (["6-12", ""], "''")])
def test_parse_lead_windows_refuses_and_names_the_spec(specs, bad):
    from swift_amd.eval.metrics import parse_lead_windows
    with pytest.raises(ValueError) as e:
        parse_lead_windows(specs, 4, 6)
    assert bad in str(e.value), str(e.value)


def test_parse_lead_windows_refuses_off_interval_and_too_many():
    from swift_amd.eval.metrics import parse_lead_windows
    with pytest.raises(ValueError, match="6-12"):
        parse_lead_windows(["6-12"], 4, 12)
    many = [f"{6 * a}-{6 * b}" for a in range(1, 9) for b in range(a, 9)][:33]
    assert len(set(many)) == 33
    parse_lead_windows(many[:32], 8, 6)
    with pytest.raises(ValueError) as e:
        parse_lead_windows(many, 8, 6)
    assert "32" in str(e.value) and many[32] in str(e.value)
    with pytest.raises(ValueError):
        parse_lead_windows([], 8, 6)


def test_check_windows_args_runs_on_the_host():
    from swift_amd.generate import check_windows_args, parser
    ok = parser.parse_args(["--input", "x", "--members", "3", "--steps", "4", "--lead-windows", "6-24", "12-18"])
    assert ok.lead_windows == ["6-24", "12-18"]
    check_windows_args(ok)
    check_windows_args(argparse.Namespace(lead_windows=None, members=1, steps=4, interval=6))     # without the flag: nothing to check
    with pytest.raises(ValueError, match="--members 1"):
        check_windows_args(parser.parse_args(["--input", "x", "--members", "1", "--steps", "4", "--lead-windows", "6-24"]))
    with pytest.raises(ValueError, match="--members 65"):
        check_windows_args(parser.parse_args(["--input", "x", "--members", "65", "--steps", "4", "--lead-windows", "6-24"]))
    with pytest.raises(ValueError, match="6-30"):
        check_windows_args(parser.parse_args(["--input", "x", "--members", "3", "--steps", "4", "--lead-windows", "6-30"]))


def test_the_flag_implies_the_metric_sums_and_a_job_without_it_is_unchanged():
    from swift_amd.generating.products import LeadWindows, MetricSums, product_types
    ns = lambda **k: argparse.Namespace(**k)
    assert product_types(ns(lead_windows=["6-24"])) == [MetricSums, LeadWindows]
    assert product_types(ns(lead_windows=None)) == [] and product_types(ns()) == []
    assert product_types(ns(metrics=True, lead_windows=None)) == [MetricSums]


def test_lead_window_mean_validates_before_the_library_is_touched():
    import torch
    from swift_amd.eval.metrics import lead_window_mean
    with pytest.raises(ValueError, match="lead_window_mean"):
        lead_window_mean(torch.zeros(3, 4), [0], [1])                                       # not on the device
    with pytest.raises(ValueError, match="lead_window_mean"):
        lead_window_mean(np.zeros((3, 4), np.float32), [0], [1])


def test_the_c_abi_refuses_on_the_host():
    """The refusals of include/swiftk.h, which come before any launch and therefore need no GPU."""
    import ctypes
    from swift_amd import _lib
    L = _lib.lib()
    ints = lambda *a: (ctypes.c_int * len(a))(*a)
    call = lambda x, out, f, c, n, nw, M: L.swiftk_lead_window_mean(x, out, f, c, n, nw, M, None)
    assert call(None, 16, ints(0), ints(1), 1, 1, 4) == -1 and call(16, None, ints(0), ints(1), 1, 1, 4) == -1
    assert call(16, 16, None, ints(1), 1, 1, 4) == -1 and call(16, 16, ints(0), None, 1, 1, 4) == -1
    assert call(16, 16, ints(0), ints(1), 0, 1, 4) == -1 and call(16, 16, ints(0), ints(1), 1, 0, 4) == -1
    assert call(16, 16, ints(0), ints(1), 1, 1, 0) == -1
    assert call(16, 16, ints(*[0] * 9), ints(*[1] * 9), 1, 9, 4) == -2
    assert call(16, 16, ints(-1), ints(1), 2, 1, 4) == -2 and call(16, 16, ints(0), ints(0), 2, 1, 4) == -2
    assert call(16, 16, ints(1), ints(2), 2, 1, 4) == -2 and call(16, 16, ints(0, 2), ints(1, 1), 2, 2, 4) == -2
    assert call(18, 16, ints(0), ints(1), 1, 1, 4) == -3 and call(16, 17, ints(0), ints(1), 1, 1, 4) == -3
