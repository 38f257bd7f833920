"""-m gpu: ``swiftk_ensemble_sums`` and ``swiftk_rmse_sums`` (swift_amd/csrc/train_kernels.hip) through the C ABI on fields of physical
magnitude, each output scored on its own against the fp64 truths of tests/backward_reference.py / tests/tangent_reference.py on the
fields of tests/metric_sums_reference.py (tests/test_metric_sums_reference_cpu.py pins the conditions the bounds rest on).  Every
case prints its worst error beside its bound.

Shapes.  ``ensemble_sums`` launches min(ceil(H W / 256), 32) workgroups per (sample, variable): 7 x 11 is one partly filled
workgroup, 19 x 67 five with a ragged last one, 33 x 257 = 8481 points wants 34, gets 32 and sends 289 threads on a ragged second
trip (W odd: the row index changes inside a wave); N = 2, 8, 9, 16, 17, 64 are both ends of the three instantiations.  ``rmse_sums``
launches min(ceil(B H W / 256), 64) per channel: (3, 2, 33, 257) is 25443 points against 16384, and the sample index changes inside
a workgroup.

Bounds.  Every term of every sum is non-negative, so the suite's "1e-5 x the sum of the absolute terms" is F32_TOL = 1e-5 relative
to each sum, for each (b, v) and each of the four sums separately; the per-point arithmetic alone stays within 1e-6 (CPU test).
The exact cases have one right answer in any order of summation and must come back bit for bit.  Where all members agree the
pair-spread and variance sums must be exactly 0.0.  Metric level, from the sums' bound and nothing measured: rmse = mean_b sqrt(s0 / hw)
halves a relative error (1e-5 stands); ssr is a quotient of two such roots (2e-5); crps = skill term - spread term is a difference, so
|got - ref| <= 1e-5 (skill term + spread term).

Measured on MI355X (worst relative error over (b, v) and the three shapes, sums in the order mean error^2, skill, pair spread,
variance; bound in brackets):
                N = 2                  8                      9                      16                     17                     64
  physical      1.4e-7 1.4e-7 2.1e-7 1.1e-7 | 8.6e-8 1.8e-7 2.0e-7 1.5e-7 | 1.1e-7 1.0e-7 8.6e-8 1.1e-7 | 1.1e-7 1.4e-7 1.9e-7 2.1e-7 |
                2.0e-7 1.1e-7 1.5e-7 1.0e-7 | 1.8e-7 1.8e-7 2.0e-7 2.2e-7   [1e-5]
  hostile       1.2e-7 2.7e-7 1.3e-7 1.8e-7 | 2.8e-7 1.6e-7 2.2e-7 1.4e-7 | 1.1e-7 1.5e-7 1.7e-7 2.3e-7 | 2.5e-7 1.5e-7 1.1e-7 2.0e-7 |
                1.1e-7 1.7e-7 2.0e-7 1.6e-7 | 1.3e-7 1.4e-7 1.3e-7 2.1e-7   [1e-5]
  planted       1.9e-7 1.5e-7 1.1e-7 1.8e-7 | 1.7e-7 1.2e-7 1.6e-7 2.1e-7 | 2.6e-7 1.9e-7 1.5e-7 1.8e-7 | 1.2e-7 1.6e-7 2.1e-7 1.4e-7 |
                9.4e-8 1.4e-7 1.2e-7 8.5e-8 | 2.1e-7 1.4e-7 1.5e-7 1.2e-7   [1e-5]; the sums of the agreeing members exactly 0.0 at every N
  exact         all 32 outputs bit-equal at every N and shape, also on a non-zero out (largest sum 8,604,792 < 2^24)
  on a non-zero out (N = 9)   physical 3.5e-7 2.1e-7 2.2e-7 2.2e-7, hostile 1.3e-7 2.2e-7 1.7e-7 1.5e-7 [1e-5]
  rmse_sums     exact bit-equal; physical 2.5e-7 (all), 3.7e-8 (2e5 channel), 1.0e-8 (280 channel) [1e-5]
  all_metrics (N = 12), worst variable: physical rmse 2.7e-8, ssr 4.4e-8, crps 4.7e-8; hostile 3.0e-8, 5.8e-8, 4.4e-8; planted 5.4e-8,
                7.7e-8, 7.3e-8 [1e-5, 2e-5, 1e-5]; ssr of the agreeing members 0.0
The parent commit's kernel took the mean of the members as they are (x_0 + ... + x_{N-1}) / N, and (mean - y)^2 and sum (x_n - mean)^2 from
it; its library on the same inputs (sums 1 and 2 are differences of neighbours and stood at <= 2.8e-7 throughout):
  hostile       sum 0: 1.4e-2  3.0e-2  1.5e-2  3.4e-2  3.2e-2  3.2e-1 for N = 2 .. 64;  sum 3: 7.1e-3  1.0e-2  1.3e-2  1.8e-2  1.9e-2  2.9e-1
                per variable at 33 x 257 (280 +- 0.01, 1e5 +- 3, 2e5 +- 1, 2e5 +- 0.1): N = 12 sum 0 7.4e-5 6.8e-5 7.2e-4 1.6e-2, sum 3 3.4e-6 4.6e-6
                1.6e-4 1.6e-2; N = 64 sum 0 7.2e-5 3.3e-5 1.0e-3 2.3e-1, sum 3 1.2e-5 1.6e-5 6.0e-4 2.5e-1 -- within a tenth of the figures of the
                fp32 restatement on the CPU (test_metric_sums_reference_cpu.py)
  physical      sum 0: 2.8e-5  2.9e-5  2.3e-5  3.0e-5  3.9e-5  1.0e-4, all at 7 x 11 (77 points average less of it away: <= 8.0e-6 at
                the two larger shapes) in the 280 +- 0.3 and 5e4 +- 30 variables; sum 3 <= 2.1e-7
  planted       sum 0: 2.6e-6  1.5e-5  1.2e-5  3.9e-5  2.1e-5  2.0e-4; the variance sum of the agreeing members is non-zero from N = 8 on
                (2 x is exact, 3 x is not), so ssr of that variable came out as 9.1e-5 instead of 0
  all_metrics (N = 12) hostile, per variable: rmse 6.0e-6 2.2e-5 2.4e-4 7.1e-3, ssr 4.4e-6 2.5e-5 1.6e-4 6.7e-4
On the parent commit test_ensemble_sums_each_sum_of_each_sample_and_variable fails for physical and hostile at every N and for
planted at N = 8 .. 64, test_ensemble_sums_adds_to_what_out_holds[hostile] and
test_all_metrics_per_variable_against_the_oracle_in_fp64[hostile] and [planted] fail; the exact cases, planted at N = 2, the physical
cases of the other two tests and both rmse_sums cases pass there: placement, the stride loop and the atomics were right, the arithmetic
about an unshifted mean was not.  ``swiftk_rmse_sums`` needed no change.
"""
import pytest
import torch

import metric_sums_reference as mr

pytestmark = pytest.mark.gpu

F32_TOL = mr.F32_TOL
SCORED = ("physical", "hostile", "planted")
METRIC_N = 12


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def s():
    return torch.cuda.current_stream().cuda_stream


def L():
    from swift_amd import _lib
    return _lib.lib()


def fmt(v):
    return "[" + ", ".join(f"{float(x):.1e}" for x in v) + "]"


def run_ensemble(dev, pred, y, w, out0=None):
    """out0 (or zeros) + the kernel's four sums, [B, V, 4] fp32 on the host."""
    B, N, V, H, W = pred.shape
    p, t, wd = pred.to(dev), y.to(dev), w.to(dev)
    out = torch.zeros(B, V, 4, device=dev) if out0 is None else out0.to(dev).clone()
    assert L().swiftk_ensemble_sums(p.data_ptr(), t.data_ptr(), wd.data_ptr(), out.data_ptr(), B, N, V, H, W, s()) == 0
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("N", mr.MEMBERS)
def test_ensemble_sums_exact_case_bit_for_bit(dev, N):
    """All B V 4 outputs of the integer design, each with a value of its own: placement by (b, v) and sum, the member stride, the
    grid-stride loop's second trip and its ragged end (a dropped or doubled point changes an integer), the cross-block atomics.
    At the largest shape also on top of a non-zero (integer) ``out``: the kernel adds."""
    for shape in mr.SHAPES:
        pred, y, w, ref = mr.case("exact", N, shape)
        out = run_ensemble(dev, pred, y, w).double()
        bad = int((out != ref).sum())
        print(f"ensemble_sums exact N {N} {shape[2]}x{shape[3]}: {bad} of {ref.numel()} outputs differ from the fp64 sums "
              f"(worst {float(mr.rel_err(out, ref).max()):.1e}; largest sum {float(ref.max()):.0f} < 2^24)")
        assert bad == 0, (shape, out, ref)
    out0 = (1.0 + torch.arange(ref.numel())).view_as(ref).float()
    out = run_ensemble(dev, pred, y, w, out0).double()
    assert torch.equal(out, ref + out0.double())


@pytest.mark.parametrize("N", mr.MEMBERS)
@pytest.mark.parametrize("kind", SCORED)
def test_ensemble_sums_each_sum_of_each_sample_and_variable(dev, kind, N):
    worst = torch.zeros(4, dtype=torch.float64)
    for shape in mr.SHAPES:
        pred, y, w, ref = mr.case(kind, N, shape)
        out = run_ensemble(dev, pred, y, w)
        e = mr.rel_err(out, ref)                       # [B, V, 4]
        hit = e.amax(-1).flatten().argmax()
        print(f"ensemble_sums {kind} N {N} {shape[2]}x{shape[3]}: worst relative error per sum {fmt(e.amax((0, 1)))} (bound {F32_TOL:.0e}), "
              f"the worst at (b, v) = ({int(hit) // shape[1]}, {int(hit) % shape[1]})")
        worst = torch.maximum(worst, e.amax((0, 1)))
        if kind == "planted":
            zeros = out[:, mr.PLANTED_AGREE_VAR, 2:]
            print(f"ensemble_sums {kind} N {N} {shape[2]}x{shape[3]}: pair-spread and variance sums where the members agree "
                  f"{zeros.flatten().tolist()} (must be exactly 0.0)")
            assert bool((zeros == 0.0).all()), shape
        assert float(e.max()) <= F32_TOL, shape
    print(f"ensemble_sums {kind} N {N}: worst over the shapes {fmt(worst)} (bound {F32_TOL:.0e})")


@pytest.mark.parametrize("kind", ["physical", "hostile"])
def test_ensemble_sums_adds_to_what_out_holds(dev, kind):
    """include/swiftk.h: the kernel adds into ``out``.  A quarter of each sum is there already (the 3e-6 family's sums are 1e-9:
    a common starting value would drown them); the increment is scored like the sum."""
    N = 9
    pred, y, w, ref = mr.case(kind, N)
    out0 = (0.25 * ref).float()
    out = run_ensemble(dev, pred, y, w, out0)
    e = mr.rel_err(out.double() - out0.double(), ref)
    print(f"ensemble_sums {kind} N {N} on a non-zero out: worst relative error of the increment per sum {fmt(e.amax((0, 1)))} (bound {F32_TOL:.0e})")
    assert float(e.max()) <= F32_TOL


@pytest.mark.parametrize("kind", ["exact", "physical"])
def test_rmse_sums_past_the_block_cap(dev, kind):
    """25443 points per channel (16384 before the grid-stride loop), the truth a [:, 1] slice of [B, days, C, H, W] whose other days
    are NaN, on top of a non-zero ``sq``; every entry of ``sq`` on its own.  exact: integers, bit for bit.  physical: 2e5 +- 50 with
    differences of order 1 and 280 +- 5 with differences of order 0.3, 1e-5 relative to the added sum."""
    yv, T, w, ref = mr.rmse_case(kind)
    B, C, H, W = yv.shape
    sq0 = (5.0 + 2.0 * torch.arange(1 + C)).float() if kind == "exact" else (0.25 * ref).float()
    yd, Td, wd, sq = yv.to(dev), T.to(dev), w.to(dev), sq0.to(dev).clone()
    tsl = Td[:, 1]
    assert Td.stride(0) == mr.RMSE_DAYS * C * H * W and tsl.data_ptr() != Td.data_ptr()
    assert L().swiftk_rmse_sums(yd.data_ptr(), tsl.data_ptr(), Td.stride(0), wd.data_ptr(), sq.data_ptr(), B, C, H, W, s()) == 0
    torch.cuda.synchronize()
    got = sq.cpu().double()
    e = mr.rel_err(got - sq0.double(), ref)
    print(f"rmse_sums {kind} {tuple(yv.shape)}: relative error of the added sums (all, then per channel) {fmt(e)} "
          f"(bound {'bit-equal' if kind == 'exact' else f'{F32_TOL:.0e}'})")
    if kind == "exact":
        assert torch.equal(got, sq0.double() + ref)
    else:
        assert float(e.max()) <= F32_TOL


@pytest.mark.parametrize("kind", SCORED)
def test_all_metrics_per_variable_against_the_oracle_in_fp64(dev, kind):
    """``all_metrics`` (what generate --metrics and the store CLI report) at 12 members on 33 x 257 against oracle/metrics.py on the
    same fp32 fields in fp64, variable by variable, with the bounds derived in this file's docstring."""
    from oracle import metrics as omet
    from swift_amd.eval.metrics import all_metrics
    N = METRIC_N
    pred, y, w, ref = mr.case(kind, N)
    B, _, V, H, W = pred.shape
    hw, lat = H * W, mr.lats(H)
    names = [f"v{i}" for i in range(V)]
    got = all_metrics(pred.to(dev), y.to(dev), names, lat, "t")
    torch.cuda.synchronize()
    g = lambda m: torch.stack([got[f"{m}_{nm}_t"] for nm in names]).cpu().double()
    p64, y64 = pred.double(), y.double()
    rmse, crps, ssr = omet.rmse(p64, y64, lat), omet.crps(p64, y64, lat), omet.spread_skill_ratio(p64, y64, lat)
    skill, spread = ref[..., 1].sum(0) / (B * N * hw), (ref[..., 2] / hw / (2 * N * (N - 1))).mean(0)
    assert float(mr.rel_err(skill - spread, crps).max()) < 1e-6   # (the two terms are the oracle's; its weights are fp64, the sums' fp32)
    e_rmse, e_ssr, e_crps = mr.rel_err(g("rmse"), rmse), mr.rel_err(g("ssr"), ssr), (g("crps") - crps).abs() / (skill + spread)
    print(f"all_metrics {kind} N {N}: per variable rmse {fmt(e_rmse)} (bound 1e-5), ssr {fmt(e_ssr)} (bound 2e-5), "
          f"crps {fmt(e_crps)} of skill + spread term (bound 1e-5)")
    if kind == "planted":
        assert float(ssr[mr.PLANTED_AGREE_VAR]) == 0.0 and float(g("ssr")[mr.PLANTED_AGREE_VAR]) == 0.0
    assert float(e_rmse.max()) <= F32_TOL and float(e_ssr.max()) <= 2 * F32_TOL and float(e_crps.max()) <= F32_TOL
