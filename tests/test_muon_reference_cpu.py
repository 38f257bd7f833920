"""tests/muon_reference.py pinned on the CPU: the yardsticks test_gpu_muon.py scores the device against, and the proof that its
assertions bite.

* the bf16 restatement in the implementation's rounding order equals the scalar recurrence of the diagonal designs in VALUE, 0
  mismatches, at every design shape, wide and tall, steps 1 / 2 / 5, with native bf16 matmuls and with fp32 K-chunks of 64;
* ``ns_fp64`` is the singular-value map phi^k(s / |s|) on the singular vectors of the bf16-rounded input, to 1e-12;
* the oracle's bf16 iteration (reference order ``b A + (c A) A``) and the restatement (``c (A A)``) differ by no more than their
  two errors against fp64 add up to -- bf16 noise -- and the restatement is not the worse of the two;
* the yardstick's spread: native, K-chunk-64 and K-chunk-32 emulations agree in whole-matrix error against fp64 (measured: bit
  identical results at steps 1; 0.999 ... 1.012 at steps 5), and per tile-sized slice within ``SLICE_SPREAD`` (measured: 1.000 at
  steps 1, at most 1.347 at steps 5 -- 360 x 264 gauss);
* the four defects ``ns_bf16_impl_order(perturb=...)`` restates make ``check_diagonal`` / ``check_dense`` fail.  Observed, stack of
  three at 64 x 160 (diagonal, wrong values of 30,720 after 1 / 2 / 5 steps) and of three kinds at 264 x 360 (dense, worst member's
  whole-matrix error and worst slice error over the yardstick's, steps 1 / 5):
      a neighbour's XT       220 / 306 / 3760 wrong values (2 of 3 matrices);  dense 11x / 1e39x whole, 8x / 1e39x slice
      XT one iteration old   0 / 174 / 174 (the first iteration has no older XT);  dense 1x / 4e24x whole, 1x / 8e24x slice
      1.0 in a pad column    3712 / 3712 / 10240 (the matrix it is in);  dense 8.5e5x whole / not finite
      last K-chunk dropped   37 / 37 / 37 (all three);  dense 2.1x / 26x whole, 3.6x / 90x slice
"""
import itertools

import pytest
import torch

import muon_reference as R

DESIGN_CASES = [(m, n, tall) for (m, n) in R.DESIGN_COUNTS for tall in (False, True)]


@pytest.mark.parametrize("m,n,tall", DESIGN_CASES, ids=[f"{m}x{n}{'-tall' if t else ''}" for m, n, t in DESIGN_CASES])
def test_restatement_equals_scalar_recurrence(m, n, tall):
    G, *design = R.diagonal_design(m, n, R.DESIGN_COUNTS[(m, n)], 7, tall)
    assert tuple(G.shape) == ((n, m) if tall else (m, n))
    for steps in R.DESIGN_STEPS:
        for chunk in (None, 64):
            got = R.ns_bf16_impl_order(G, steps, chunk)
            R.check_diagonal(got, m, n, design, steps, tall, f"{m} x {n} tall {tall} steps {steps} chunk {chunk}")
    # steps 1 and 2 tell the three non-zero levels apart (after 5 two of them may coincide)
    perm, sigma, sign = design
    for steps in (1, 2):
        x = R.diagonal_recurrence(sigma, torch.ones_like(sigma), steps)
        assert len({float(x[sigma == v][0]) for v in R.LEVELS if bool((sigma == v).any())}) == sum(1 for k in R.DESIGN_COUNTS[(m, n)] if k)


def test_restatement_equals_scalar_recurrence_stacks():
    for (m, n, L) in ((64, 160, 12), (20, 36, 2), (1, 12, 12)):
        for tall in (False, True):
            G, designs = R.design_stack(m, n, L, 3, tall)
            assert len({tuple(d[0].tolist()) for d in designs}) >= (L if m > 1 else 6)  # every matrix its own perm (1 x 12: its own column or sigma)
            for steps in R.DESIGN_STEPS:
                got = R.ns_bf16_impl_order(G, steps)
                for l in range(L):
                    R.check_diagonal(got[l], m, n, designs[l], steps, tall, f"{L} x {m} x {n} matrix {l} steps {steps}")


def test_design_rejects_what_has_no_exact_answer():
    with pytest.raises(AssertionError):
        R.diagonal_design(64, 160, (10, 16, 33, 5), 0)      # sum sigma^2 = 16.0625
    with pytest.raises(AssertionError):
        R.diagonal_design(64, 160, (10, 16, 32, 6)[:3] + (0,), 0)
    with pytest.raises(AssertionError):
        R.diagonal_design(16, 160, (16, 0, 0, 0), 0)        # no zero row, one level
    with pytest.raises(AssertionError):
        R.diagonal_design(17, 160, (16, 0, 0, 1), 0)        # one level


@pytest.mark.parametrize("shape", [(264, 360), (360, 264)], ids=str)
@pytest.mark.parametrize("kind", R.DENSE_KINDS)
def test_fp64_iteration_is_the_singular_value_map(shape, kind):
    G, s = R.spectrum_case(shape[0], shape[1], kind, 5)
    assert float((torch.linalg.svdvals(G) - s.sort(descending=True).values).abs().max()) < 1e-12
    Gb = G.to(R.BF).double()
    U, sv, Vh = torch.linalg.svd(Gb, full_matrices=False)
    for steps in (1, 5):
        got = R.ns_fp64(G, steps)
        assert got.shape == G.shape
        want = (U * R.phi(sv / sv.norm(), steps)) @ Vh
        assert float((got - want).abs().max()) < 1e-12
        assert float((torch.linalg.svdvals(got).sort().values - R.phi(sv / sv.norm(), steps).sort().values).abs().max()) < 1e-12
    # a stack is its members
    st = torch.stack([G, 2 * G.flip(0)])
    assert float((R.ns_fp64(st, 2)[1] - R.ns_fp64(2 * G.flip(0), 2)).abs().max()) < 1e-13


@pytest.fixture(scope="module")
def dense():
    """shape, kind, steps -> (fp64 result, {emulation: result})"""
    out = {}
    for shape in R.DENSE_SHAPES:
        for kind in R.DENSE_KINDS:
            G = R.dense_input(shape, kind)
            for steps in R.DENSE_STEPS:
                out[shape, kind, steps] = (G, R.ns_fp64(G, steps), {c: R.ns_bf16_impl_order(G, steps, c) for c in (None, 64, 32)})
    return out


def test_oracle_order_is_bf16_noise_away(dense):
    """The reference multiplies ``(c A) A``, the implementation ``c (A A)``: as many roundings, at other places."""
    from oracle import muon as om
    for (shape, kind, steps), (G, ref, emu) in dense.items():
        o = om.newton_schulz5(G, steps)
        eo, ei = float(R.slice_errors(o, ref)[0]), float(R.slice_errors(emu[None], ref)[0])
        d = float(R.slice_errors(o.float(), emu[None].float())[0])
        print(f"{shape} {kind} steps {steps}: vs fp64 oracle {eo:.3e} restatement {ei:.3e} (ratio {ei / eo:.3f}); oracle vs restatement {d:.3e}")
        assert d <= eo + ei                 # no further apart than their own rounding errors put them
        assert ei <= 1.1 * eo               # measured 0.72 ... 1.005 at steps 5, 1.000 at steps 1


def test_yardstick_spread(dense):
    worst = {s: 1.0 for s in R.DENSE_STEPS}
    for (shape, kind, steps), (G, ref, emu) in dense.items():
        scores = {c: R.slice_errors(x, ref) for c, x in emu.items()}
        whole = [float(w[0]) for w, _ in scores.values()]
        spread = max(float((a[1] / b[1]).max()) for a, b in itertools.permutations(scores.values(), 2))
        worst[steps] = max(worst[steps], spread)
        print(f"{shape} {kind} steps {steps}: whole-matrix error vs fp64 native {whole[0]:.3e} chunk-64 {whole[1]:.3e} chunk-32 {whole[2]:.3e}; "
              f"worst slice ratio between two of them {spread:.3f}")
        assert max(whole) / min(whole) <= (1.01 if steps == 1 else 1 / 0.82)
        assert (2.0e-3 < min(whole) and max(whole) < 4.5e-3) if steps == 1 else (1.5e-2 < min(whole) and max(whole) < 2.2e-1)
    print(f"worst CPU-vs-CPU slice ratio: {worst}")
    for steps in R.DENSE_STEPS:
        assert worst[steps] <= R.SLICE_SPREAD[steps]


PERTURBATIONS = ("swap_xt", "stale_xt", "pad_one", "drop_chunk")


@pytest.mark.parametrize("perturb", PERTURBATIONS)
def test_assertions_fail_on_a_perturbed_restatement(perturb):
    """The tests of the tests: each defect of the composition, restated on the CPU, fails the assertions the device run gets."""
    m, n, L = 64, 160, 3
    G, designs = R.design_stack(m, n, L, 11)
    for steps in R.DESIGN_STEPS:
        got = R.ns_bf16_impl_order(G, steps, perturb=perturb)
        failing = 0
        for l in range(L):
            try:
                R.check_diagonal(got[l], m, n, designs[l], steps, False, perturb)
            except AssertionError:
                failing += 1
        want = torch.stack([R.diagonal_expected(m, n, *d, steps) for d in designs])
        print(f"{perturb} diagonal steps {steps}: {int((got.float() != want).sum())} wrong values, {failing} of {L} matrices fail")
        assert failing >= 1 or (perturb == "stale_xt" and steps == 1)
    G, _ = R.dense_stack_input((264, 360), 0)
    for steps in R.DENSE_STEPS:
        if perturb == "stale_xt" and steps == 1:
            continue
        with pytest.raises(AssertionError):
            R.check_dense(R.ns_bf16_impl_order(G, steps, perturb=perturb), G, steps, what=perturb)


def test_unperturbed_restatements_pass_the_dense_check():
    """... and the K-chunk-32 emulation, a correct run in another summation order, passes them."""
    for shape in ((264, 360), (128, 1024)):
        G, _ = R.dense_stack_input(shape, 1)
        for steps in R.DENSE_STEPS:
            R.check_dense(R.ns_bf16_impl_order(G, steps, chunk=32), G, steps, what=f"chunk-32 {shape}")
