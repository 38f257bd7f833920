"""The references and the bound of tests/maps_reference.py on the CPU, the host side of ``generate --maps`` and the refusals of
``swiftk_ensemble_maps`` (which come before any launch, so they need no GPU): the documented fp64 order of arithmetic stays within
the derived bound of the exact rational values, the fp32 one does not on physical-magnitude fields (the reason the kernel works
in fp64), accumulation over ICs costs one rounding per IC, and the regional reduction is what a hand computation gives."""
import argparse
import math

import numpy as np
import pytest

import maps_reference as mr

MEMBERS = (2, 3, 12, 13, 64)
GRID = (1, 2, 3, 11)   # n, V, H, W of the CPU checks: 66 pixels per ensemble size and kind


def _case(kind, N, seed=1):
    n, V, H, W = GRID
    pred, y = mr.make(kind, (n, N, V, H, W), seed=seed)
    return pred, y, mr.exact(pred, y), mr.bound(N, pred, y)


@pytest.mark.parametrize("N", MEMBERS)
def test_the_fp64_order_of_arithmetic_stays_within_the_bound(N):
    for kind in mr.KINDS:
        pred, y, ref, bnd = _case(kind, N)
        got = mr.emulate(pred, y)
        assert got.shape == ref.shape == bnd.shape == (GRID[0], 4) + GRID[1:] and got.dtype == np.float64
        for s, name in enumerate(mr.STATISTICS):
            ok, worst = mr.within(got[:, s], ref[:, s], bnd[:, s])
            print(f"{kind} N={N} {name}: worst error / bound {worst:.3g}")
            assert ok
        if kind == "const":   # identical members: no pair differs and N x is exact, so p and the variance are exactly zero
            assert np.all(got[:, 3] == 0.0) and np.all(ref[:, 3] == 0.0)
            a_n = np.abs(pred[:, 0].astype(np.float64) - y)          # a / N of N equal terms: N d is exact, so a / N = d
            assert np.array_equal(got[:, 2], a_n)


@pytest.mark.parametrize("kind", sorted(mr.PHYSICAL))
@pytest.mark.parametrize("N", MEMBERS)
def test_fp32_arithmetic_exceeds_the_bound_on_physical_fields(N, kind):
    """The reason for fp64: 280 K under a spread of 1e-2 K (2e5 under 0.1) in the same order of arithmetic, in fp32, loses the
    variance and the CRPS difference -- and the bound can fail."""
    pred, y, ref, bnd = _case(kind, N)
    got = mr.emulate_fp32(pred, y)
    for s, name in enumerate(mr.STATISTICS):
        ok, worst = mr.within(got[:, s], ref[:, s], bnd[:, s])
        print(f"{kind} N={N} {name} in fp32: worst error / bound {worst:.3g}")
        # (two members: the differences from the truth are exact by Sterbenz's lemma, small multiples of the field's ulp add up
        # exactly and halving is exact, so fp32 can hit bias, mse and crps; the variance it still misses through x_0 + x_1)
        if name == "variance" or N >= 3:
            assert not ok and worst > 1.0


def test_accumulating_three_ics_is_the_sum_of_their_terms():
    """acc = t_0; acc += t_1; acc += t_2: two rounded additions after the first write, so within n_ic u sum |t_i| of the correctly
    rounded sum (``math.fsum``) of the three per-IC terms."""
    N, shape = 5, (2, 5, 2, 3, 7)
    cases = [mr.make(kind, shape, seed=10 + i) for i, kind in enumerate(("t280", "normal", "t280"))]
    terms = [mr.emulate(p, y) for p, y in cases]
    acc = None
    for p, y in cases:
        acc = mr.emulate(p, y, acc)
    assert np.array_equal(acc, (terms[0] + terms[1]) + terms[2])
    fs = np.frompyfunc(lambda a, b, c: math.fsum((a, b, c)), 3, 1)(*terms).astype(np.float64)
    scale = sum(np.abs(t) for t in terms)
    assert np.all(np.abs(acc - fs) <= len(cases) * mr.U * scale)
    assert not np.shares_memory(acc, terms[0]) and np.array_equal(terms[0], mr.emulate(*cases[0]))   # emulate leaves acc alone


def test_the_c_entry_refuses_bad_arguments_without_a_gpu():
    """Every refusal comes before the launch: no pointer here is ever dereferenced."""
    from swift_amd import _lib
    L = _lib.lib()

    def call(pred=64, y=64, acc=64, n=2, N=3, V=2, H=3, W=8, accumulate=0):
        return L.swiftk_ensemble_maps(pred, y, acc, n, N, V, H, W, accumulate, None)

    assert call(pred=None) == call(y=None) == call(acc=None) == -1                            # SWIFTK_EINVAL
    assert call(n=0) == call(N=0) == call(V=-1) == call(H=0) == call(W=0) == call(n=-3) == -1
    assert call(accumulate=2) == call(accumulate=-1) == -1
    assert call(N=1) == call(N=65) == -2                                                      # SWIFTK_ESHAPE
    assert call(n=1 << 20, V=1 << 12) == -2                                                   # n V beyond 2^31 - 1
    assert call(pred=66) == call(y=66) == call(pred=65) == -3                                 # SWIFTK_EALIGN
    assert call(acc=68) == call(acc=66) == -3
    assert call(accumulate=1, acc=68) == -3


def test_check_maps_args_refuses_on_the_host():
    from swift_amd import generate
    for members in (2, 12, 64):
        generate.check_maps_args(argparse.Namespace(maps=True, members=members))
    for members in (1, 0, 65):
        with pytest.raises(ValueError, match="--maps"):
            generate.check_maps_args(argparse.Namespace(maps=True, members=members))
        generate.check_maps_args(argparse.Namespace(maps=False, members=members))             # without the flag: nothing to check
    a = generate.parser.parse_args(["--input", "x", "--maps"])
    assert a.maps is True and generate.parser.parse_args(["--input", "x"]).maps is False
    with pytest.raises(ValueError, match="--maps"):
        generate.main(a)                                                                      # --members 1: before anything is loaded


def test_ensemble_maps_refuses_what_the_kernel_cannot_take_without_a_gpu():
    import torch
    from swift_amd.eval.metrics import MAP_STATISTICS, ensemble_maps
    assert MAP_STATISTICS == mr.STATISTICS == ["bias", "mse", "crps", "variance"]
    pred, y = (torch.from_numpy(a) for a in mr.make("normal", (1, 3, 1, 3, 8), seed=9))
    for bad in ((pred, y), (pred.double(), y), (pred[0], y), (pred.numpy(), y)):               # CPU tensors, dtype, rank, type
        with pytest.raises(ValueError, match="ensemble_maps"):
            ensemble_maps(*bad)


def test_the_region_reduction_on_a_hand_made_grid():
    """Four rows at -60, -10, 10 and 45 degrees, two columns: the tropics are rows 1 and 2, the north row 3, the south row 0."""
    from swift_amd.eval.metrics import region_means
    lat = np.array([-60.0, -10.0, 10.0, 45.0])
    m = np.array([[1.0, 3.0], [10.0, 30.0], [-5.0, -7.0], [100.0, 300.0]])                    # row means 2, 20, -6, 200
    c = [math.cos(math.radians(v)) for v in lat]
    want = {"global": (2 * c[0] + 20 * c[1] - 6 * c[2] + 200 * c[3]) / sum(c), "tropics": (20 * c[1] - 6 * c[2]) / (c[1] + c[2]),
            "n_extratropics": 200.0, "s_extratropics": 2.0}
    for fn in (region_means, mr.regions):
        got = fn(m, lat)
        assert sorted(got) == sorted(want)
        for k in want:
            assert np.shape(got[k]) == () and abs(float(got[k]) - want[k]) <= 8 * mr.U * 600.0, (fn.__name__, k)
    stacked = np.stack([m, 2 * m])[None]                                                      # leading axes are kept: [1, 2, H, W]
    for fn in (region_means, mr.regions):
        got = fn(stacked, lat)
        assert got["tropics"].shape == (1, 2) and np.allclose(got["tropics"][0], [want["tropics"], 2 * want["tropics"]], rtol=1e-14)
    # a band that holds no row of the grid is left out (both edges of the tropics belong to it and to the extratropics)
    assert sorted(region_means(m[:2], lat[:2])) == sorted(mr.regions(m[:2], lat[:2])) == ["global", "s_extratropics", "tropics"]
    edge = region_means(np.ones((3, 2)), np.array([-20.0, 0.0, 20.0]))
    assert sorted(edge) == ["global", "n_extratropics", "s_extratropics", "tropics"] and all(abs(v - 1.0) < 1e-15 for v in edge.values())
    scores = mr.region_scores(np.stack([m, np.abs(m), m, 4 * np.abs(m)])[None, :, None], lat, ["t"], 6)   # [1, 4, 1, H, W]
    s = scores["n_extratropics"]
    assert sorted(s) == ["bias_t_6h", "crps_t_6h", "rmse_t_6h", "spread_t_6h", "ssr_t_6h"]
    assert s["bias_t_6h"] == 200.0 and s["rmse_t_6h"] == math.sqrt(200.0) and s["spread_t_6h"] == math.sqrt(800.0)
    assert abs(s["ssr_t_6h"] - 2.0) < 1e-15
