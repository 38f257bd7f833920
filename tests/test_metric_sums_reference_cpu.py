"""The conditions the bounds of tests/test_gpu_metric_sums.py rest on, on the CPU (tests/metric_sums_reference.py):
(a) the first-member form of the per-point arithmetic, in fp32 with the grid sums in fp64, is within 1e-6 of the fp64 truth on every
    builder and every ensemble size the device tests use -- a tenth of their bound, so the arithmetic alone leaves room for the
    device's accumulation;
(b) the exact builders are exact: fp32 summation of their term planes in shuffled orders and in the (lane, wave, block) order
    equals the fp64 sum bit for bit, and every output has its own value;
(c) teeth: the unshifted mean misses 1e-5 on the hostile builder at 12 and 64 members, and leaves a non-zero variance where all
    members agree, so the device tests can tell the two forms apart;
(d) offset / spread of each builder is what its name says."""
import pytest
import torch

import metric_sums_reference as mr

ALL_N = mr.MEMBERS + (12,)


@pytest.mark.parametrize("N", ALL_N)
def test_first_member_form_is_within_a_tenth_of_the_device_bound(N):
    for shape in mr.SHAPES:
        for kind in mr.BUILDERS:
            pred, y, w, ref = mr.case(kind, N, shape)
            e = mr.rel_err(mr.sums64(mr.ensemble_terms_fp32(pred, y, w, shifted=True)), ref).amax((0, 1))
            print(f"{kind} N={N} {shape[2]}x{shape[3]}: first-member form, worst relative error per sum {[f'{float(v):.1e}' for v in e]} "
                  f"(bound {mr.ARITH_TOL:.0e})")
            assert float(e.max()) <= mr.ARITH_TOL, (kind, shape)


@pytest.mark.parametrize("N", ALL_N)
def test_agreeing_members_give_exact_zeros_in_the_first_member_form_only(N):
    pred, y, w, ref = mr.case("planted", N)
    v = mr.PLANTED_AGREE_VAR
    assert bool((ref[:, v, 2:] == 0).all()) and bool((ref[:, v, :2] > 0).all())
    s = mr.sums64(mr.ensemble_terms_fp32(pred, y, w, shifted=True))
    assert bool((s[:, v, 2:] == 0).all())
    u = mr.sums64(mr.ensemble_terms_fp32(pred, y, w, shifted=False))
    assert bool((u[:, v, 2] == 0).all())
    if N in (9, 12, 17):   # x + ... + x (N times) / N is not x in fp32
        assert bool((u[:, v, 3] > 0).all())


def test_the_planted_points_are_where_the_builder_says():
    N, shape = 9, mr.SHAPE_PAST_CAP
    pred, y, w, ref = mr.case("planted", N, shape)
    B, V, H, W = shape
    one, every = mr.planted_one_member_points(shape)
    x, t = pred[:, :, mr.PLANTED_POINTS_VAR].reshape(B, N, -1), y[:, mr.PLANTED_POINTS_VAR].reshape(B, -1)
    hit = x == t[:, None]
    assert bool(hit[:, :, every].all()) and bool((hit[:, :, one].sum(1) >= 1).all())
    only_one = one[~torch.isin(one, every)]
    # (exactly one but for chance: 280 +- 0.3 in fp32 has some 1e4 values per spread, so a second member coincides now and then)
    assert only_one.numel() > 1000 and float((hit[:, :, only_one].sum(1) == 1).double().mean()) > 0.99
    far = (y[:, mr.PLANTED_FAR_VAR] - pred[:, :, mr.PLANTED_FAR_VAR].amax(1)).min()
    assert float(far) > 900 * mr.PHYSICAL[mr.PLANTED_FAR_VAR][1]
    assert bool(torch.isfinite(pred).all()) and bool(torch.isfinite(y).all())


@pytest.mark.parametrize("N", mr.MEMBERS)
def test_exact_ensemble_case_has_one_answer_in_any_order(N):
    for shape in mr.SHAPES:
        pred, y, w, ref = mr.case("exact", N, shape)
        B, V, H, W = shape
        assert bool((ref == ref.round()).all()) and float(ref.max()) < 2 ** 24 and float(ref.min()) > 0
        assert ref.unique().numel() == B * V * 4, "every output needs its own value"
        for shifted in (False, True):
            terms = mr.ensemble_terms_fp32(pred, y, w, shifted)
            assert bool((terms == terms.round()).all())
            assert torch.equal(mr.sums64(terms), ref)
            for b in range(B):
                for v in range(V):
                    for k in range(4):
                        got = [mr.device_order_sum(terms[k, b, v], mr.ENSEMBLE_BLOCK_CAP)] + [mr.shuffled_sum(terms[k, b, v], sd) for sd in (1, 2, 3)]
                        assert all(float(g) == float(ref[b, v, k]) for g in got), (shape, shifted, b, v, k)


def test_exact_ensemble_case_fills_what_it_can():
    """Every point carries the error and skill terms; the member spread sits on every s-th point and reaches the second trip."""
    for N in mr.MEMBERS:
        pred, y, w, ref = mr.case("exact", N)
        B, _, V, H, W = pred.shape
        assert bool(((pred.double().mean(1) - y.double()).abs().reshape(B, V, -1).sum(-1) > 0).all())
        spread = (pred.amax(1) > pred.amin(1)).reshape(B, V, -1)
        assert bool(spread[:, :, 8192:].any(-1).all()) and bool(spread[:, :, :256].any(-1).all())
        assert int(spread[0, 0].sum()) >= (H * W) // mr.exact_stride(N, mr.SHAPE_PAST_CAP)
    assert mr.exact_stride(9, mr.SHAPE_PAST_CAP) == 1 and mr.exact_stride(64, mr.SHAPE_BLOCKS) > 1


def test_exact_rmse_case_has_one_answer_in_any_order():
    y, T, w, ref = mr.rmse_case("exact")
    B, C, H, W = y.shape
    assert bool(torch.isnan(T[:, 0]).all()) and bool(torch.isnan(T[:, 2]).all())
    assert bool((ref == ref.round()).all()) and float(ref.max()) < 2 ** 24 and ref.unique().numel() == 1 + C
    terms = mr.rmse_terms_fp32(y, T[:, 1], w)
    assert float(terms[0].double().sum()) == float(ref[0])
    assert all(float(mr.shuffled_sum(terms[0], sd)) == float(ref[0]) for sd in (1, 2, 3))
    for c in range(C):
        plane = terms[1, :, c].contiguous()
        got = [mr.device_order_sum(plane, mr.RMSE_BLOCK_CAP)] + [mr.shuffled_sum(plane, sd) for sd in (1, 2, 3)]
        assert all(float(g) == float(ref[1 + c]) for g in got), c


def test_physical_rmse_case_arithmetic():
    """y - t is exact at 2e5 (neighbours within a factor of two); the term planes in fp32 are within 1e-6 of the truth."""
    y, T, w, ref = mr.rmse_case("physical")
    terms = mr.rmse_terms_fp32(y, T[:, 1], w)
    got = torch.cat([terms[0].double().sum().reshape(1), terms[1].double().sum((0, 2, 3))])
    e = mr.rel_err(got, ref)
    print(f"rmse physical: worst relative error of the fp32 terms {float(e.max()):.1e} (bound {mr.ARITH_TOL:.0e})")
    assert float(e.max()) <= mr.ARITH_TOL
    assert float(y[:, 0].abs().median() / (y[:, 0] - T[:, 1, 0]).std()) > 1e5


@pytest.mark.parametrize("N", [12, 64])
def test_teeth_the_unshifted_mean_misses_the_bound_on_the_hostile_field(N):
    pred, y, w, ref = mr.case("hostile", N)
    e = mr.rel_err(mr.sums64(mr.ensemble_terms_fp32(pred, y, w, shifted=False)), ref)
    worst = e.amax(0)   # [V, 4]
    print(f"hostile N={N}: unshifted mean, worst relative error per variable of sum 0 {[f'{float(v):.1e}' for v in worst[:, 0]]}, "
          f"sum 3 {[f'{float(v):.1e}' for v in worst[:, 3]]}, sums 1 and 2 {float(worst[:, 1:3].max()):.1e}")
    assert float(worst[:, 0].max()) > mr.F32_TOL and float(worst[:, 3].max()) > mr.F32_TOL
    assert bool((worst[2:, 0] > mr.F32_TOL).all()) and bool((worst[2:, 3] > mr.F32_TOL).all())   # both 2e5 families, each sum
    assert float(worst[:, 1:3].max()) <= mr.ARITH_TOL   # differences of neighbours: exact either way


def test_offset_over_spread_is_what_the_names_say():
    for fam, kind in ((mr.PHYSICAL, "physical"), (mr.HOSTILE, "hostile")):
        pred = mr.case(kind, 64)[0]
        ratio = mr.offset_over_spread(pred)
        print(f"{kind}: offset / spread per variable {[f'{float(r):.3g}' for r in ratio]}")
        for v, (off, sp) in enumerate(fam):
            if off == 0.0:
                assert float(ratio[v]) < 2.0
            else:
                assert 0.8 * off / sp <= float(ratio[v]) <= 1.25 * off / sp
    assert min(off / sp for off, sp in mr.HOSTILE) >= 2.5e4 and max(off / sp for off, sp in mr.PHYSICAL) <= 2e3


def test_latitudes_are_not_symmetric_and_weights_are_the_wrappers():
    import numpy as np
    H = 33
    w = mr.lat_weights(H)
    assert not torch.allclose(w, w.flip(0), rtol=1e-3)
    c = np.cos(np.deg2rad(mr.lats(H)))
    assert torch.equal(w, torch.from_numpy(c / c.mean()).float())   # eval/metrics.py:28-29
    e = mr.exact_weights(H)
    assert not torch.equal(e, e.flip(0)) and bool((e[1:] != e[:-1]).any()) and set(e.tolist()) == {1.0, 2.0}
