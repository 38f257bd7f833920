"""CPU: the reference, the fp32 yardstick and the hostile-row case of tests/test_gpu_modnorm_rows.py (tests/modnorm_reference.py):
the fp64 reference is the oracle's ModulatedNorm + residual, the yardstick and its pair quantisation stay inside the bars at every
row width the GPU module runs, and each deliberate mistake (``VARIANTS``) misses the bar at least 3 x on the rows built to catch it.

Seen on the cases below (seed CASE_SEED), max|err| / max|ref| per row against fp64, over the nine widths:
  fp32 yardstick        benign rows 1.6e-7 .. 2.4e-7; row E (63.5 + 0.25 Bernoulli) 5.2e-8 .. 4.3e-6, so its bar is 1e-5 .. 1.7e-5; every
                        other hostile row <= 1.8e-7 (all bars but row E's are the floor 1e-5)
  one_pass              row E 3.4e-4 .. 6.2e-3 at d >= 520: 23 .. 400 x its bar
  no_eps                row G 0.20 .. 0.35 (also gross on row C);  drop_last_slot row D 4.6 .. 2e5
  neighbour_sample      rows 31 / 32 0.29 .. 0.68;  neighbour_row_stats every placed hostile row >= 0.26
  padded_d              rows 0 / 6 >= 0.11 / 0.67 where d % 512 != 0
"""
import pytest
import torch

import modnorm_reference as mr
from conftest import rel_l2

F64 = torch.float64
SEED = mr.CASE_SEED
MARGIN = 3.0  # a variant must miss a row's bar by this factor


def rnd(shape, seed, std=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=dtype) * std


def _scored(d, bf16_y=True, **kw):
    c = mr.make_forward_case(d, SEED, bf16_y=bf16_y, **kw)
    a = mr.forward_args(c)
    ref = mr.modnorm_forward(**a)
    yard = mr.modnorm_forward(**a, dtype=torch.float32)
    assert ref.dtype == F64 and yard.dtype == torch.float32
    return c, a, ref, yard


def _row_of(c, kind):
    return next(r for r, k in c["hostile"].items() if k == kind)


@pytest.mark.parametrize("d", [1056, 104, 8])
def test_reference_equals_the_oracle(d):
    """fp64 modnorm_forward == x + oracle.swinv2.modulated_norm(y, latent) with the modulation a Linear of a latent, as in
    tests/test_gpu_kernels.py -- hostile rows included, each scored on its own."""
    from oracle.swinv2 import modulated_norm
    B, rps = 3, 32
    c = mr.make_forward_case(d, SEED)
    p = {"n.norm.weight": c["gamma"].double(), "n.norm.bias": c["beta"].double(),
         "n.modulation.weight": rnd((2 * d, d), 16, 0.02, F64), "n.modulation.bias": rnd((2 * d,), 17, 0.1, F64)}
    lat = rnd((B, d), 18, dtype=F64)
    mod = torch.nn.functional.linear(lat, p["n.modulation.weight"], p["n.modulation.bias"])
    want = c["x"].double() + modulated_norm(c["y"].double().view(B, rps, d), lat, p, "n.").reshape(B * rps, d)
    got = mr.modnorm_forward(c["y"], c["x"], c["gamma"], c["beta"], mod, rps)
    assert rel_l2(got, want) < 1e-12
    assert float(mr.row_errs(got, want).max()) < 1e-11
    # the variants are mistakes, none of them the oracle -- but one_pass, the same function in exact arithmetic (its mistake is fp32's)
    for v in mr.VARIANTS:
        e = rel_l2(mr.modnorm_forward(c["y"], c["x"], c["gamma"], c["beta"], mod, rps, variant=v), want)
        assert (e < 1e-9) if v == "one_pass" else (e > 1e-3), (v, e)


@pytest.mark.parametrize("bf16_y", [True, False], ids=["bf16y", "f32y"])
@pytest.mark.parametrize("d", mr.WIDTHS)
def test_case_builder_places_what_it_promises(d, bf16_y):
    c = mr.make_forward_case(d, SEED, bf16_y=bf16_y)
    y, x, hostile = c["y"], c["x"], c["hostile"]
    M = y.shape[0]
    assert M == 96 and c["mod"].shape == (3, 2 * d)
    assert sorted(hostile) == [1, 6, 11, 12, 31, 32, 95] and "".join(hostile[r] for r in sorted(hostile)) == "ABCDEFG"
    for r in hostile:  # bf16-representable, whatever the benign rows are
        assert torch.equal(y[r], mr.bf16_round(y[r])), r
    benign = [r for r in range(M) if r not in hostile]
    assert torch.equal(y[benign], mr.bf16_round(y[benign])) == bf16_y
    assert float(y[1, 0]) == 300.0 and float(y[12, d - 1]) == -500.0
    assert float(y[6].min()) == float(y[6].max()) == 40.0
    assert int((y[11] != 0).sum()) == 1 and 0.9e-3 < float(y[11, 5]) < 1.1e-3
    assert set(y[31].tolist()) <= {63.5, 63.75} and (d < 64 or len(set(y[31].tolist())) == 2)
    assert float(y[32].abs().max()) > 1e4 and float(y[95].abs().max()) < 5e-3 and float(y[95].abs().max()) > 0
    assert float(x[mr.ZERO_X_ROW].abs().max()) == 0.0 and mr.ZERO_X_ROW in benign
    # (a zero value as a pair: hi = 0, byte 128)
    _, hi, byte = mr.pair_quantise(x[mr.ZERO_X_ROW], parts=True)
    assert float(hi.float().abs().max()) == 0.0 and bool((byte == 128).all())


@pytest.mark.parametrize("d", mr.WIDTHS)
def test_yardstick_and_its_pair_quantisation_stay_inside_the_bars(d):
    """The condition that the reference alone does not use up the bar: on benign rows the fp32 yardstick errs far below the floor
    (so their bar is the fixed 1e-5, not a measured number), every row of it passes the fp32 bar and every element of its
    (bf16 hi, 8-bit lo) quantisation the pair bound -- also on what a pair holds for x, and with fp32 benign y rows."""
    for bf16_y in (True, False):
        c, a, ref, yard = _scored(d, bf16_y)
        errs, bar = mr.row_errs(yard, ref), mr.f32_row_bar(yard, ref)
        hostile = c["hostile"]
        benign = [r for r in range(ref.shape[0]) if r not in hostile]
        print(f"d {d} {'bf16' if bf16_y else 'fp32'} y: yardstick benign {float(errs[benign].max()):.1e}; " +
              ", ".join(f"{k}@{r} {float(errs[r]):.1e}" for r, k in sorted(hostile.items())))
        assert float(errs[benign].max()) <= mr.F32_TOL / mr.FACTOR / 4
        assert bool((errs <= bar).all()) and bool((bar >= mr.F32_TOL).all())
        q, hi, _ = mr.pair_quantise(yard, parts=True)
        assert float(mr.pair_excess(q, hi, yard, ref).max()) <= 1.0
    # the pair kernels start from what a pair holds for x
    c, a, _, _ = _scored(d)
    a["x"] = mr.pair_quantise(c["x"])
    ref, yard = mr.modnorm_forward(**a), mr.modnorm_forward(**a, dtype=torch.float32)
    q, hi, _ = mr.pair_quantise(yard, parts=True)
    assert float(mr.pair_excess(q, hi, yard, ref).max()) <= 1.0
    assert rel_l2(q, ref) < 1e-5


def _misses(d, variant, c, a, ref, yard):
    bar = mr.f32_row_bar(yard, ref)
    got = mr.modnorm_forward(**a, dtype=torch.float32, variant=variant)
    return mr.row_errs(got, ref) / bar, got


@pytest.mark.parametrize("d", mr.WIDTHS)
def test_every_variant_misses_the_bar_on_its_rows(d):
    """Sensitivity: evaluated in fp32 like a kernel, each mistake misses max(4 x yardstick, 1e-5) at least 3 x on the named rows --
    one_pass on row E (d >= 520), no_eps on row G, drop_last_slot on row D, neighbour_row_stats on every placed hostile row,
    neighbour_sample on the two rows at the sample boundary, padded_d (d % 512 != 0) on a benign row and the constant row -- and so
    does the pair value of each, element by element."""
    c, a, ref, yard = _scored(d)
    rows = {"one_pass": [_row_of(c, "E")] if d >= 520 else [],
            "no_eps": [_row_of(c, "G")],
            "drop_last_slot": [_row_of(c, "D")],
            "neighbour_row_stats": sorted(c["hostile"]),
            "neighbour_sample": [c["rows_per_sample"] - 1, c["rows_per_sample"]],
            "padded_d": [0, _row_of(c, "B")] if d % 512 else []}
    assert set(rows) == set(mr.VARIANTS)
    for v in mr.VARIANTS:
        ratio, got = _misses(d, v, c, a, ref, yard)
        q, hi, _ = mr.pair_quantise(got, parts=True)
        excess = mr.pair_excess(q, hi, yard, ref)
        print(f"d {d} {v}: " + ", ".join(f"row {r} {float(ratio[r]):.1f} x" for r in rows[v]))
        for r in rows[v]:
            assert float(ratio[r]) >= MARGIN, (v, r, float(ratio[r]))
            assert float(excess[r]) >= MARGIN, (v, r, float(excess[r]))


@pytest.mark.parametrize("rps,B", [(20, 4), (18, 4)])
@pytest.mark.parametrize("d", [64, 1544])
def test_sample_boundary_off_the_chunk_cases(d, rps, B):
    """The rows_per_sample = 20 and 18, B = 4 cases of the GPU module (sample boundaries inside a 16-row chunk; at 18 also inside a
    four-row workgroup of the row-per-wave kernel): a hostile row on each side of the first boundary, and taking the neighbour's
    modulation or the next row's statistics there is gross."""
    c, a, ref, yard = _scored(d, rows_per_sample=rps, B=B)
    assert ref.shape[0] == rps * B and c["hostile"][rps - 1] == "E" and c["hostile"][rps] == "F"
    ratio, _ = _misses(d, "neighbour_sample", c, a, ref, yard)
    assert float(ratio[rps - 1]) >= MARGIN and float(ratio[rps]) >= MARGIN
    ratio, _ = _misses(d, "neighbour_row_stats", c, a, ref, yard)
    assert all(float(ratio[r]) >= MARGIN for r in c["hostile"])
