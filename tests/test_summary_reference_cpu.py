"""The references and bounds of tests/summary_reference.py on the CPU, the host side of the quantiles, and the refusals of
``swiftk_ensemble_summary`` (which come before any launch, so they need no GPU): the fp64 order of arithmetic stays within the
derived bounds, the fp32 one does not (the reason the kernel works in fp64), the quantile table is numpy's ``linear`` method."""
import numpy as np
import pytest

import summary_reference as sr

SHAPE = (1, 1, 4, 50)   # n, V, H, W of the CPU checks: 200 pixels per ensemble size and kind


def _case(kind, N, seed=1):
    n, V, H, W = SHAPE
    pred = sr.make(kind, (n, N, V, H, W), seed=seed)
    return (pred,) + sr.reference_exact(pred)


@pytest.mark.parametrize("N", sr.MEMBERS)
def test_the_fp64_order_of_arithmetic_stays_within_both_bounds(N):
    for kind in sr.KINDS:
        pred, mean, s, A = _case(kind, N)
        m64, s64 = sr.emulate64(pred)
        ok_m, w_m = sr.worst(m64, mean, sr.bound_mean(mean, A, N))
        ok_s, w_s = sr.worst(s64, s, sr.bound_spread(s, A, N))
        print(f"{kind} N={N}: worst error / bound: mean {w_m:.3g}, spread {w_s:.3g}")
        assert ok_m and ok_s
        if kind == "const":   # identical members: N x is exact, so the mean is the member and the spread exactly zero
            assert np.array_equal(m64, pred[:, 0]) and np.all(s64 == 0.0) and np.all(s == 0.0)


@pytest.mark.parametrize("N", sr.MEMBERS)
def test_fp32_arithmetic_exceeds_the_spread_bound_at_280_kelvin(N):
    """The reason for fp64: 280 K under a spread of 1e-2 K in the same order of arithmetic, in fp32."""
    pred, mean, s, A = _case("t280", N)
    m32, s32 = sr.emulate32(pred)
    ok_s, w_s = sr.worst(s32, s, sr.bound_spread(s, A, N))
    ok_m, w_m = sr.worst(m32, mean, sr.bound_mean(mean, A, N))
    print(f"t280 N={N} in fp32: worst error / bound: mean {w_m:.3g}, spread {w_s:.3g}")
    assert not ok_s and w_s > 1.0
    if N >= 3:   # (two members: x_0 + x_1 is one rounding and the halving exact)
        assert not ok_m


def test_quantile_table_is_numpys_linear_method():
    from swift_amd.eval.metrics import quantile_table
    for N in (2, 3, 12, 13, 64):
        lo, frac = quantile_table([0.0, 1.0, 0.5, 0.1, 0.9], N)
        assert lo.dtype == np.int32 and frac.dtype == np.float64 and lo.shape == frac.shape == (5,)
        assert (lo[0], frac[0]) == (0, 0.0) and (lo[1], frac[1]) == (N - 1, 0.0)
        if N % 2:
            assert (lo[2], frac[2]) == ((N - 1) // 2, 0.0)   # the median of an odd ensemble is a member
        assert np.all((0 <= lo) & (lo <= N - 1)) and np.all((0.0 <= frac) & (frac < 1.0))
        assert np.array_equal(lo + frac, np.array([0.0, 1.0, 0.5, 0.1, 0.9]) * (N - 1))
    lo, frac = quantile_table([], 5)
    assert lo.shape == frac.shape == (0,)
    for bad in ([1.5], [-0.1], [float("nan")], [float("inf")], [0.5] * 17):
        with pytest.raises(ValueError, match="quantile"):
            quantile_table(bad, 12)
    with pytest.raises(ValueError, match="members"):
        quantile_table([0.5], 1)


@pytest.mark.parametrize("N", sr.MEMBERS)
def test_the_emulated_quantiles_are_numpys(N):
    """a + g (b - a) in three fp64 roundings against ``np.quantile(..., method="linear")`` on the fp64 members: within
    4 u max(|a|, |b|) (each of the three operations rounds a value of at most 2 max(|a|, |b|), numpy's lerp likewise)."""
    from swift_amd.eval.metrics import quantile_table
    qs = [0.0, 0.1, 0.25, 0.5, 0.9, 1.0]
    lo, frac = quantile_table(qs, N)
    for kind in sr.KINDS:
        pred = sr.make(kind, (1, N, 1, 4, 50), seed=2)
        x64 = pred.astype(np.float64)
        xs = np.sort(x64, axis=1)
        for j, q in enumerate(qs):
            a, b = xs[:, lo[j]], xs[:, min(lo[j] + 1, N - 1)]
            mine = a + frac[j] * (b - a)
            theirs = np.quantile(x64, q, axis=1, method="linear")
            assert np.all(np.abs(mine - theirs) <= 4 * sr.U * np.maximum(np.abs(a), np.abs(b)))
            assert np.array_equal(sr.quantiles_emulated(pred, lo[j:j + 1], frac[j:j + 1])[:, 0], mine.astype(np.float32))
        got = sr.quantiles_emulated(pred, lo, frac)
        assert got.shape == (1, len(qs), 1, 4, 50) and got.dtype == np.float32
        assert np.array_equal(got[:, 0], pred.min(1)) and np.array_equal(got[:, -1], pred.max(1))


def test_the_c_entry_refuses_bad_arguments_without_a_gpu():
    """Every refusal comes before the launch: no pointer here is ever dereferenced."""
    from swift_amd import _lib
    L = _lib.lib()

    def call(pred=64, lo=64, frac=64, out=64, n=2, N=3, V=2, H=3, W=8, Q=2):
        return L.swiftk_ensemble_summary(pred, lo, frac, out, n, N, V, H, W, Q, None)

    assert call(pred=None) == call(out=None) == -1                                            # SWIFTK_EINVAL
    assert call(n=0) == call(N=0) == call(V=-1) == call(H=0) == call(W=0) == -1
    assert call(lo=None) == call(frac=None) == -1                                             # the table is needed when Q > 0
    assert call(N=1) == call(N=65) == -2                                                      # SWIFTK_ESHAPE
    assert call(Q=-1) == call(Q=17) == -2
    assert call(n=1 << 20, V=1 << 12) == -2                                                   # n V beyond 2^31 - 1
    assert call(pred=66) == call(out=66) == call(lo=66) == -3                                 # SWIFTK_EALIGN
    assert call(frac=68) == -3
