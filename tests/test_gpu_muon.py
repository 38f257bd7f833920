"""-m gpu: Muon's Newton-Schulz orthogonaliser (swift_amd/training/optimizers/muon.py) bit for bit and slice by slice, against
tests/muon_reference.py.

(a) diagonal designs -- rows with disjoint supports, sigma in {1, 1/2, 1/4, 0}, sum sigma^2 a power of four: every product is a
    single-term sum and the whole iteration ONE right answer per entry.  All three entry points, value-equal after 1, 2 and 5
    steps, zero off the support, at the shapes where the host code branches (plain / split-K GEMM, k-splits that do not divide,
    two row and column tiles, the slab buffer reused and regrown, the stacked ``XT`` view, both branches of ``_fro_norm``).
(b) dense spectra against the fp64 iteration per matrix and per 256 x 352 slice, next to the bf16 restatement in the
    implementation's rounding order on the same input and slices; the bounds are margins over that yardstick.
(c) two steps of ``MuonWithAuxAdam.step`` on a mixed group, bit for bit against the same torch glue around the test's own calls of
    the orthogonalisers.
"""
import contextlib
import math

import pytest
import torch

import muon_reference as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def pm():
    from swift_amd.training.optimizers import muon
    return muon


@contextlib.contextmanager
def torch_gemms():
    """The library's GEMM launches of the orthogonaliser swapped for fp32 torch.matmul + a cast, on the device: tells a wrong
    launch of ours from a torch element-wise op that rounds otherwise than the recurrence assumes."""
    def gemm(a, w, out, n, k):
        out[..., :n] = (a[..., :k].float() @ w[..., :n, :k].float().mT).to(BF)
        return out
    m = pm()
    saved = m._gemm_bf16, m._gemm_stack
    m._gemm_bf16 = m._gemm_stack = gemm
    try:
        yield
    finally:
        m._gemm_bf16, m._gemm_stack = saved


def run_diagonal(fn, G, designs, m, n, steps, tall, what, dev):
    """fn(G on the device, steps) against the designs' right answers; a mismatch is re-run on torch matmuls and says which side
    it was on."""
    got = fn(G.to(dev), steps)
    torch.cuda.synchronize()
    assert got.dtype == BF and tuple(got.shape) == tuple(G.shape), f"{what}: {got.dtype} {tuple(got.shape)} for input {tuple(G.shape)}"
    got = got.float().cpu()
    try:
        for l, d in enumerate(designs):
            R.check_diagonal(got[l] if G.ndim == 3 else got, m, n, d, steps, tall, f"{what} matrix {l} steps {steps}")
    except AssertionError as e:
        with torch_gemms():
            again = fn(G.to(dev), steps).float().cpu()
        try:
            for l, d in enumerate(designs):
                R.check_diagonal(again[l] if G.ndim == 3 else again, m, n, d, steps, tall, what)
            verdict = "right with torch matmuls in place of the GEMM launches: one of the library's GEMM launches (or its operands' strides)"
        except AssertionError as e2:
            verdict = f"wrong with torch matmuls as well ({e2}): the transpose launch or a torch element-wise op"
        raise AssertionError(f"{e}\n -> {verdict}") from None


def single(G, steps):
    return pm().zeropower_via_newtonschulz5(G, steps)


def stack(G, steps):
    return pm().zeropower_stack(G, steps)


def small(G, steps):
    return pm().zeropower_stack_small(G, steps)


# ------------------------------------------------------------------------------------------------------- (a) diagonal designs
SINGLE = [(20, 36), (64, 160), (24, 260), (128, 1024), (264, 360), (8, 8), (18, 30)]


@pytest.mark.parametrize("tall", [False, True], ids=["wide", "tall"])
@pytest.mark.parametrize("m,n", SINGLE, ids=[f"{m}x{n}" for m, n in SINGLE])
def test_single_matrix_diagonal_designs(dev, m, n, tall):
    """``zeropower_via_newtonschulz5``: 20 x 36 every product on the plain GEMM (m % 8); 64 x 160 no k-split; 24 x 260 product 1 on
    two uneven k-ranges (5 chunks of 64), product 3 plain; 128 x 1024 eight k-ranges, then one; 264 x 360 two row and column
    tiles, k-splits 3 / 2 / 2; 8 x 8 and 18 x 30 the library-matmul branch.  measured on MI355X: 0 values differ."""
    G, *design = R.diagonal_design(m, n, R.DESIGN_COUNTS[(m, n)], 21 + m, tall)
    for steps in R.DESIGN_STEPS:
        run_diagonal(single, G, [design], m, n, steps, tall, f"single {m} x {n} {'tall' if tall else 'wide'}", dev)


def test_single_matrix_small_large_small_shares_the_slab_buffer(dev):
    """The split-K slabs live in ONE buffer per device that grows on demand: small, large, small again in one process, from an
    empty buffer (24 x 260 needs 2 x 24 x 24 floats, 128 x 1024 8 x 128 x 128, 264 x 360 3 x 264 x 264)."""
    pm()._SLABS.clear()
    sizes = []
    for i, (m, n) in enumerate([(24, 260), (128, 1024), (264, 360), (24, 260), (128, 1024), (64, 160), (264, 360)]):
        for tall in (False, True):
            G, *design = R.diagonal_design(m, n, R.DESIGN_COUNTS[(m, n)], 300 + 2 * i + tall, tall)
            run_diagonal(single, G, [design], m, n, 5, tall, f"visit {i}: single {m} x {n} {'tall' if tall else 'wide'}", dev)
        sizes.append(pm()._SLABS[dev].numel())
    assert sizes[0] < sizes[1] < sizes[2] == sizes[-1], sizes  # grown twice, then reused


STACKS = [(2, 64, 160), (3, 64, 160), (12, 64, 160), (3, 264, 360), (2, 20, 36)]


@pytest.mark.parametrize("tall", [False, True], ids=["wide", "tall"])
@pytest.mark.parametrize("L,m,n", STACKS, ids=[f"{L}x{m}x{n}" for L, m, n in STACKS])
def test_stack_diagonal_designs(dev, L, m, n, tall):
    """``zeropower_stack``: every matrix its own perm, signs and deal of levels, so a neighbour's operand (the ``XT`` view of
    ``XTall``: ldw = L km, stride km; the one-launch transpose of [L km, kn]) shows as values off the support.  64 x 160 takes
    the two-stage ``_fro_norm``, 264 x 360 and 20 x 36 its fallback.  measured on MI355X: 0 values differ."""
    G, designs = R.design_stack(m, n, L, 40 + L, tall)
    for steps in R.DESIGN_STEPS:
        run_diagonal(stack, G, designs, m, n, steps, tall, f"stack {L} x {m} x {n} {'tall' if tall else 'wide'}", dev)


SMALL = [(12, 1, 12), (12, 8, 8), (12, 18, 30)]


@pytest.mark.parametrize("tall", [False, True], ids=["wide", "tall"])
@pytest.mark.parametrize("L,m,n", SMALL, ids=[f"{L}x{m}x{n}" for L, m, n in SMALL])
def test_small_stack_diagonal_designs(dev, L, m, n, tall):
    """``zeropower_stack_small`` (batched library matmuls): twelve 1 x 12 logit scales with one non-zero entry each (sigma 2, 4 or
    8: the normalised entry is +-1), 8 x 8, 18 x 30.  measured on MI355X: 0 values differ."""
    G, designs = R.design_stack(m, n, L, 70 + m, tall)
    for steps in R.DESIGN_STEPS:
        run_diagonal(small, G, designs, m, n, steps, tall, f"small stack {L} x {m} x {n} {'tall' if tall else 'wide'}", dev)


# ---------------------------------------------------------------------------------------------------------- (b) dense spectra
@pytest.mark.parametrize("kind", R.DENSE_KINDS)
@pytest.mark.parametrize("shape", R.DENSE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_single_matrix_dense_spectra_vs_fp64(dev, shape, kind):
    """``zeropower_via_newtonschulz5`` against the fp64 iteration, whole matrix (relative L2) and per 256 x 352 slice (max error
    over max reference), steps 1 and 5; bounds 1.25 x / 1.5 x the restatement's whole-matrix error and, per slice, 1.5 x the
    larger of the native and K-chunk-64 restatements' times the CPU-vs-CPU slice spread (1.0 / 1.35).
    measured on MI355X: whole-matrix error 2.3e-3 ... 4.3e-3 at steps 1, 1.000 x the yardstick's in all 12 cases, worst slice at
    1.00 x the yardstick's; 1.8e-2 ... 2.0e-1 (halfrank) at steps 5, 0.996 ... 1.010 x the yardstick's, worst slice at most
    1.07 x.  Well inside the margins, which stay where the CPU emulations' own spread puts them."""
    G = R.dense_input(shape, kind)
    for steps in R.DENSE_STEPS:
        got = single(G.to(dev), steps).float().cpu()
        R.check_dense(got, G, steps, what=f"single {shape[0]} x {shape[1]} {kind}")


@pytest.mark.parametrize("first", [0, 2])
@pytest.mark.parametrize("shape", R.DENSE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stack_dense_spectra_vs_fp64(dev, shape, first):
    """``zeropower_stack`` on three members of different kinds (gauss, geo1e-3, flat / flat, halfrank, gauss), scored per member
    and per slice as above.  measured on MI355X: per member 2.3e-3 ... 4.3e-3 at steps 1 (1.000 x the yardstick's, worst slice
    1.00 x), 1.8e-2 ... 2.0e-1 at steps 5 (0.996 ... 1.010 x, worst slice at most 1.05 x): well inside the margins."""
    G, kinds = R.dense_stack_input(shape, first)
    for steps in R.DENSE_STEPS:
        got = stack(G.to(dev), steps).float().cpu()
        R.check_dense(got, G, steps, what=f"stack {shape[0]} x {shape[1]} {'/'.join(kinds)}")


# ---------------------------------------------------------------------------------------------------------- (c) the step's glue
def test_step_glue_bit_for_bit(dev):
    """Two steps of ``MuonWithAuxAdam.step`` (one rank, parameters on the device) on a group of three 64 x 160, two 160 x 64
    (tall: rescale sqrt 2.5), a lone 48 x 48, a 4-D [32, 5, 2, 2] and twelve [1, 12, 1, 1], handed over interleaved.  Expected:
    momentum and Nesterov blend with the same torch ops, the orthogonalisers called HERE on the stacked directions (no atomics
    in those launches: a repeat gives the same bits, asserted), then p (1 - lr wd) - lr scale ortho.  Parameters and momentum
    buffers equal bit for bit: neither the grouping by shape nor the size-sorted order permutes anything, and the tall rescale
    is applied once (also read off the update's norm)."""
    m = pm()
    lr, wd, beta = 0.02, 0.01, 0.95
    decay = 1.0 - lr * wd
    # shape -> (how the step must treat it, rows, cols, rescale)
    classes = {(64, 160): ("stack", 64, 160, 1.0), (160, 64): ("stack", 160, 64, math.sqrt(2.5)), (48, 48): ("lone", 48, 48, 1.0),
               (32, 5, 2, 2): ("lone", 32, 20, 1.0), (1, 12, 1, 1): ("small", 1, 12, 1.0)}
    shapes = [(1, 12, 1, 1), (64, 160), (160, 64), (1, 12, 1, 1), (48, 48), (64, 160), (1, 12, 1, 1), (32, 5, 2, 2), (160, 64),
              (64, 160)] + [(1, 12, 1, 1)] * 9
    g = torch.Generator().manual_seed(5)
    ps = [torch.nn.Parameter((torch.randn(sh, generator=g) * 0.05).to(dev)) for sh in shapes]
    opt = m.MuonWithAuxAdam([dict(params=list(ps), use_muon=True, lr=lr, weight_decay=wd)])
    exp_p = [p.detach().clone() for p in ps]
    exp_buf = [torch.zeros_like(p) for p in ps]

    G = torch.stack([torch.randn(64, 160, generator=g) for _ in range(3)]).to(dev)
    assert torch.equal(m.zeropower_stack(G), m.zeropower_stack(G))
    assert torch.equal(m.zeropower_via_newtonschulz5(G[0]), m.zeropower_via_newtonschulz5(G[0]))

    for step in range(2):
        grads = [torch.randn(sh, generator=g).to(dev) for sh in shapes]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()
        opt.step()
        for shape, (how, rows, cols, scale) in classes.items():
            idx = [i for i, sh in enumerate(shapes) if sh == shape]
            gs, bufs, qs = [grads[i].clone() for i in idx], [exp_buf[i] for i in idx], [exp_p[i] for i in idx]
            old = [q.clone() for q in qs]
            if how == "lone":
                (gr,), (buf,), (q,) = gs, bufs, qs
                buf.mul_(beta).add_(gr, alpha=1.0 - beta)
                direction = gr.mul_(1.0 - beta).add_(buf, alpha=beta)
                ortho = m.zeropower_via_newtonschulz5(direction.reshape(rows, cols))
                q.mul_(decay).add_((ortho * scale).reshape(shape).to(q.dtype), alpha=-lr)
                orthos = [ortho]
            else:
                torch._foreach_mul_(bufs, beta)
                torch._foreach_add_(bufs, gs, alpha=1.0 - beta)
                torch._foreach_mul_(gs, 1.0 - beta)
                torch._foreach_add_(gs, bufs, alpha=beta)
                st = torch.stack([x.reshape(rows, cols) for x in gs])
                ortho = m.zeropower_stack_small(st) if how == "small" else m.zeropower_stack(st)
                scaled = (ortho * scale).float()
                torch._foreach_mul_(qs, decay)
                torch._foreach_add_(qs, [u.reshape(shape) for u in scaled.unbind(0)], alpha=-lr)
                orthos = list(ortho.unbind(0))
            for i, q, o, ortho_i in zip(idx, qs, old, orthos):
                # the rescale, read off the update itself: |p_new - decay p_old| = lr scale |ortho| (bf16 rounding of the product)
                took = float((q.double() - decay * o.double()).norm() / (lr * ortho_i.double().norm()))
                assert abs(took / scale - 1.0) < 4e-3, (step, i, shape, took, scale)
        torch.cuda.synchronize()
        for i, p in enumerate(ps):
            buf = opt.state[p]["momentum_buffer"]
            assert p.shape == exp_p[i].shape and torch.equal(p.detach(), exp_p[i]), \
                f"step {step} parameter {i} {shapes[i]}: {int((p.detach() != exp_p[i]).sum())} of {p.numel()} values differ"
            assert torch.equal(buf, exp_buf[i]), f"step {step} momentum buffer {i} {shapes[i]}"
            if step == 0:  # buf = (1 - beta) g after the first step, whatever the launch that made it
                assert torch.allclose(buf, (1.0 - beta) * grads[i], rtol=1e-6, atol=0)
    # the step moved every parameter, and no two of one shape alike
    for shape in classes:
        idx = [i for i, sh in enumerate(shapes) if sh == shape]
        assert len({tuple(ps[i].detach().flatten()[:4].tolist()) for i in idx}) == len(idx)
