"""CPU references for Muon's Newton-Schulz orthogonaliser (swift_amd/training/optimizers/muon.py); no device code.

Three yardsticks and the scores built on them:

* ``ns_fp64``            the quintic iteration in fp64, started from the bf16-rounded input: what the bf16 iteration approximates.
* ``ns_bf16_impl_order`` the iteration in bf16 with every rounding where the implementation puts it (bf16 norm + 1e-7, the three
                         bf16 products on zero-padded operands, the in-place ``mul_`` / ``add_`` glue), with native bf16 matmuls
                         or fp32 accumulation over K-chunks.  Its error against ``ns_fp64`` is rounding noise that the summation
                         order barely moves, so it says how far a CORRECT bf16 run of this order sits from fp64.
* ``diagonal_design`` /  an input family with ONE right answer: rows with disjoint supports (row i holds a single +-sigma_i at
  ``diagonal_expected``  column perm[i]).  X X^T, A A and B X are then single-term sums, exact in any accumulator, and the iteration
                         is a scalar recurrence per row with the bf16 roundings of the code:
                             A = bf(x x); A2 = bf(A A); B = bf(bf(c A2) + bf(b A)); BX = bf(B x); x <- bf(bf(a x) + BX)
                         (scalars a, b, c in fp32, as torch multiplies a bf16 tensor by a Python number on host and device).
                         sigma in {1, 1/2, 1/4, 0} with sum sigma^2 in {4, 16, 64}: the Frobenius norm is a power of two and the
                         normalisation exact as well.  Compare VALUES (a -sigma with sigma = 0 is a signed zero).

``ns_bf16_impl_order(..., perturb=...)`` restates four defects of the composition around the GEMMs (a neighbour's ``XT``, a stale
``XT``, a non-zero pad column, a dropped K-chunk); tests/test_muon_reference_cpu.py shows that the assertions used on the device
(``check_diagonal``, ``check_dense``) fail on each of them.
"""
import torch

BF = torch.bfloat16
NS_COEFFS = (3.4445, -4.7750, 2.0315)
K_GRAN = 64                      # swiftk_gemm_k_pad granularity of bf16 operands
TILE = (256, 352)                # the GEMM's output tile: the slices of slice_errors
LEVELS = (1.0, 0.5, 0.25, 0.0)

# Worst ratio, over every slice of every dense case below, between the slice errors (vs fp64) of any two of the three CPU
# emulations (native bf16 matmul, fp32 accumulation in K-chunks of 64 and of 32); tests/test_muon_reference_cpu.py measures it
# and asserts it stays below these figures, tests/test_gpu_muon.py widens its per-slice bound by them.  Measured: 1.000 at steps 1
# (the three emulations give the same bits), 1.347 at steps 5 (360 x 264 gauss).
SLICE_SPREAD = {1: 1.0, 5: 1.35}

# ------------------------------------------------------------------------------------------------------------------ the cases
# (m, n) in the wide orientation -> rows at sigma = 1, 1/2, 1/4, 0; sum sigma^2 is 4, 16 or 64
DESIGN_COUNTS = {
    (20, 36): (2, 6, 8, 4),          # 4
    (64, 160): (10, 16, 32, 6),      # 16
    (24, 260): (2, 6, 8, 8),         # 4
    (128, 1024): (56, 24, 32, 16),   # 64
    (264, 360): (40, 64, 128, 32),   # 64
    (8, 8): (3, 4, 0, 1),            # 4
    (18, 30): (2, 6, 8, 2),          # 4
}
DESIGN_STEPS = (1, 2, 5)
DENSE_SHAPES = ((264, 360), (360, 264), (128, 1024))
DENSE_KINDS = ("gauss", "geo1e-3", "flat", "halfrank")
DENSE_STEPS = (1, 5)
WHOLE_MARGIN = {1: 1.25, 5: 1.5}  # device whole-matrix error <= margin x yardstick's (CPU emulations: < 1 % apart / 0.82 ... 1.02)
SLICE_MARGIN = 1.5


def k_pad(k):
    return (k + K_GRAN - 1) // K_GRAN * K_GRAN


def _bf(x):
    return x.to(BF).float()


# --------------------------------------------------------------------------------------------------------------------- fp64
def ns_fp64(G, steps=5):
    """The iteration in fp64 from ``G.bfloat16().double()``, normalised by the fp64 Frobenius norm; [.., rows, cols], tall
    matrices iterated in the wide orientation and returned in G's."""
    a, b, c = NS_COEFFS
    X = G.to(BF).double()
    tall = X.shape[-2] > X.shape[-1]
    if tall:
        X = X.mT
    X = X / X.norm(dim=(-2, -1), keepdim=True)
    for _ in range(steps):
        A = X @ X.mT
        X = a * X + (b * A + c * (A @ A)) @ X
    return X.mT if tall else X


def phi(x, steps=1):
    a, b, c = NS_COEFFS
    for _ in range(steps):
        x = a * x + b * x ** 3 + c * x ** 5
    return x


# ------------------------------------------------------------------------------------------------- bf16, implementation order
def _product(a, w, chunk, drop_last=False):
    """bf(a w^T) of bf16 [L, r, K] x [L, s, K]: native bf16 matmul, or fp32 accumulation over K-chunks of ``chunk``."""
    K = a.shape[-1]
    if chunk is None:
        if drop_last:
            a, w = a[..., :K - K_GRAN], w[..., :K - K_GRAN]
        return a @ w.mT
    acc = torch.zeros(a.shape[0], a.shape[1], w.shape[1], dtype=torch.float32)
    for k0 in range(0, K - (chunk if drop_last else 0), chunk):
        acc += a[..., k0:k0 + chunk].float() @ w[..., k0:k0 + chunk].float().mT
    return acc.to(BF)


def ns_bf16_impl_order(G, steps=5, chunk=None, perturb=None):
    """``zeropower_stack`` restated on the CPU, rounding for rounding ([rows, cols] or a stack [L, rows, cols]; returns bf16 of
    G's shape).  The single-matrix form rounds at the same places (its glue is out of place), so this is its yardstick too.

    ``perturb`` (tests of the tests): "swap_xt" -- matrices 0 and 1 of the stack read each other's ``XT``; "stale_xt" -- ``XT``
    is the one of the previous iteration (the first iteration's is right); "pad_one" -- 1.0 in the first pad column of X of
    matrix 0; "drop_chunk" -- product 1 leaves out its last 64 columns of K."""
    assert perturb in (None, "swap_xt", "stale_xt", "pad_one", "drop_chunk")
    a, b, c = NS_COEFFS
    single = G.ndim == 2
    X = (G[None] if single else G).to(BF)
    tall = X.shape[1] > X.shape[2]
    norm = X.float().square().sum(dim=(-2, -1), keepdim=True).sqrt().to(BF)  # fp32 sum, rounded once
    X = X / (norm + 1e-7)
    if tall:
        X = X.mT
    L, m, n = X.shape
    km, kn = k_pad(m), k_pad(n)
    Xb = torch.zeros(L, m, kn, dtype=BF)
    Xb[:, :, :n] = X
    if perturb == "pad_one":
        assert kn > n, "no pad column at this shape"
        Xb[0, :, n] = 1.0
    XT = None
    for _ in range(steps):
        A = torch.zeros(L, m, km, dtype=BF)
        A[:, :, :m] = _product(Xb, Xb, chunk, drop_last=perturb == "drop_chunk")[:, :, :m]     # A = X X^T over kn
        A2 = torch.zeros(L, m, km, dtype=BF)
        A2[:, :, :m] = _product(A, A, chunk)[:, :, :m]                                          # A A over km
        B = A2.mul_(c).add_(A.mul_(b))
        cur = torch.zeros(L, n, km, dtype=BF)
        cur[:, :, :m] = Xb[:, :, :n].mT                                                         # operand form of X for B X
        use = XT if perturb == "stale_xt" and XT is not None else cur
        XT = cur
        if perturb == "swap_xt":
            assert L >= 2
            use = use[[1, 0] + list(range(2, L))]
        BX = torch.zeros(L, m, kn, dtype=BF)
        BX[:, :, :n] = _product(B, use, chunk)                                                  # B X over km
        Xb.mul_(a).add_(BX)
    X = Xb[:, :, :n]
    X = X.mT if tall else X
    return X[0] if single else X


# ---------------------------------------------------------------------------------------------------------- diagonal designs
def diagonal_design(m, n, counts, seed, tall=False):
    """(G, perm, sigma, sign): G fp32, row i of the wide orientation [m, n] holds sign[i] sigma[i] at column perm[i] and nothing
    else; ``counts`` rows at each of LEVELS, dealt to rows at random.  G is [n, m] (transposed) when ``tall``.  For m >= 2 the
    design has sum sigma^2 in {4, 16, 64}, a zero row and two non-zero levels; a one-row matrix takes ``counts`` = (sigma,)
    with sigma in {2, 4, 8}."""
    g = torch.Generator().manual_seed(seed)
    if m == 1:
        (s,) = counts
        sigma = torch.tensor([float(s)])
    else:
        assert len(counts) == len(LEVELS) and sum(counts) == m and m <= n
        assert counts[3] >= 1, "needs a zero row"
        assert sum(1 for k in counts[:3] if k) >= 2, "needs two non-zero levels"
        sigma = torch.cat([torch.full((k,), v) for k, v in zip(counts, LEVELS)])[torch.randperm(m, generator=g)]
    total = float(sigma.double().square().sum())
    assert total in (4.0, 16.0, 64.0), f"sum sigma^2 = {total} is no power of four in [4, 64]"
    perm = torch.randperm(n, generator=g)[:m]
    sign = torch.randint(0, 2, (m,), generator=g).float() * 2 - 1
    G = torch.zeros(m, n)
    G[torch.arange(m), perm] = sign * sigma
    return (G.mT.contiguous() if tall else G), perm, sigma, sign


def diagonal_recurrence(sigma, sign, steps):
    """The scalar recurrence per row, in fp32 arithmetic with a bf16 rounding wherever the implementation stores bf16."""
    a, b, c = (torch.tensor(v, dtype=torch.float32) for v in NS_COEFFS)
    norm = _bf(sigma.double().square().sum().sqrt().float())     # a power of two: exact
    x = _bf(_bf(sign * sigma) / _bf(norm + 1e-7))
    for _ in range(steps):
        A = _bf(x * x)
        A2 = _bf(A * A)
        B = _bf(_bf(c * A2) + _bf(b * A))
        BX = _bf(B * x)
        x = _bf(_bf(a * x) + BX)
    return x


def diagonal_expected(m, n, perm, sigma, sign, steps, tall=False):
    """The one right answer for ``diagonal_design``'s G after ``steps`` iterations: fp32 values, of G's shape."""
    E = torch.zeros(m, n)
    E[torch.arange(m), perm] = diagonal_recurrence(sigma, sign, steps)
    return E.mT.contiguous() if tall else E


def design_stack(m, n, L, seed, tall=False):
    """L designs of one shape with their own perm, signs and deal of levels: ([L, ..] G, [(perm, sigma, sign)] * L)."""
    if m == 1:
        parts = [diagonal_design(1, n, ((2, 4, 8)[l % 3],), seed + 101 * l, tall) for l in range(L)]
    else:
        parts = [diagonal_design(m, n, DESIGN_COUNTS[(m, n)], seed + 101 * l, tall) for l in range(L)]
    return torch.stack([p[0] for p in parts]), [p[1:] for p in parts]


def check_diagonal(got, m, n, design, steps, tall=False, what=""):
    """``got`` (one matrix, any float type, on the CPU) against the one right answer: shape and orientation, zero outside perm,
    value-equal at perm.  Raises AssertionError naming the first wrong place."""
    perm, sigma, sign = design
    want = diagonal_expected(m, n, perm, sigma, sign, steps, tall)
    assert tuple(got.shape) == tuple(want.shape), f"{what}: shape {tuple(got.shape)}, want {tuple(want.shape)}"
    g = got.float()
    assert bool(torch.isfinite(g).all()), f"{what}: non-finite values"
    on = want != 0
    on_all = torch.zeros(m, n, dtype=torch.bool)
    on_all[torch.arange(m), perm] = True
    on_all = on_all.mT if tall else on_all
    stray = ((g != 0) & ~on_all).nonzero()
    assert len(stray) == 0, (f"{what}: {len(stray)} non-zero values off the design's support, first at {stray[0].tolist()}: "
                             f"{float(g[tuple(stray[0])]):g}")
    bad = (g != want).nonzero()
    assert len(bad) == 0, (f"{what}: {len(bad)} of {int(on.sum())} values differ after {steps} steps, first at {bad[0].tolist()}: "
                           f"got {float(g[tuple(bad[0])]):.8g}, want {float(want[tuple(bad[0])]):.8g}")


# -------------------------------------------------------------------------------------------------------------- dense spectra
def spectrum_case(m, n, kind, seed):
    """G = U diag(s) V^T in fp64 with U, V from QR of Gaussian matrices; (G, s).  gauss: the singular values of a Gaussian
    m x n matrix; geo1e-3: geometric 1 ... 1e-3; flat: all ones; halfrank: ones on half the rank, zeros on the rest."""
    g = torch.Generator().manual_seed(seed)
    r = min(m, n)
    U = torch.linalg.qr(torch.randn(m, r, dtype=torch.float64, generator=g))[0]
    V = torch.linalg.qr(torch.randn(n, r, dtype=torch.float64, generator=g))[0]
    if kind == "gauss":
        s = torch.linalg.svdvals(torch.randn(m, n, dtype=torch.float64, generator=g))
    elif kind == "geo1e-3":
        s = torch.logspace(0, -3, r, dtype=torch.float64)
    elif kind == "flat":
        s = torch.ones(r, dtype=torch.float64)
    elif kind == "halfrank":
        s = torch.cat([torch.ones(r // 2, dtype=torch.float64), torch.zeros(r - r // 2, dtype=torch.float64)])
    else:
        raise ValueError(kind)
    return (U * s) @ V.mT, s


def dense_seed(shape, kind):
    return 1000 + 37 * DENSE_SHAPES.index(tuple(shape)) + DENSE_KINDS.index(kind)


def dense_input(shape, kind):
    """The bf16-rounded input of a dense case, as fp32 (what the optimiser hands the orthogonaliser)."""
    return spectrum_case(shape[0], shape[1], kind, dense_seed(shape, kind))[0].to(BF).float()


def dense_stack_input(shape, first):
    """A stack of three members of DIFFERENT kinds, starting at kind number ``first``."""
    kinds = [DENSE_KINDS[(first + j) % len(DENSE_KINDS)] for j in range(3)]
    return torch.stack([dense_input(shape, k) for k in kinds]), kinds


def slice_errors(got, ref, bm=TILE[0], bn=TILE[1]):
    """(whole, slices) of a result against its reference, both [L, rows, cols] or [rows, cols] in the INPUT's orientation:
    whole[l] = |got - ref|_F / |ref|_F per matrix; slices[l, i, j] = max|err| / max|ref| over block (i, j) of the bm x bn tiling
    of the wide-orientation result -- every element falls in one block."""
    got, ref = got.double(), ref.double()
    if got.ndim == 2:
        got, ref = got[None], ref[None]
    assert got.shape == ref.shape
    if got.shape[1] > got.shape[2]:
        got, ref = got.mT, ref.mT
    L, m, n = got.shape
    err = (got - ref).abs()
    whole = (got - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)
    nbm, nbn = (m + bm - 1) // bm, (n + bn - 1) // bn
    slices = torch.empty(L, nbm, nbn, dtype=torch.float64)
    for i in range(nbm):
        for j in range(nbn):
            e = err[:, i * bm:(i + 1) * bm, j * bn:(j + 1) * bn].flatten(1)
            r = ref[:, i * bm:(i + 1) * bm, j * bn:(j + 1) * bn].abs().flatten(1)
            slices[:, i, j] = e.amax(dim=1) / r.amax(dim=1)
    return whole, slices


def check_dense(got, G, steps, yard=None, what=""):
    """Score ``got`` (the orthogonaliser's result for G, on the CPU) against ``ns_fp64`` per matrix and per tile-sized slice, next
    to ``ns_bf16_impl_order`` on the same input and slices.  ``yard`` = (native, chunk-64) restatement results if the caller
    has them.  Returns the printed report; raises AssertionError when a score exceeds its margin over the yardstick."""
    ref = ns_fp64(G, steps)
    nat, k64 = yard if yard is not None else (ns_bf16_impl_order(G, steps), ns_bf16_impl_order(G, steps, chunk=64))
    assert tuple(got.shape) == tuple(ref.shape), f"{what}: shape {tuple(got.shape)}, want {tuple(ref.shape)}"
    assert bool(torch.isfinite(got.float()).all()), f"{what}: non-finite values"
    wg, sg = slice_errors(got, ref)
    wn, sn = slice_errors(nat, ref)
    wk, sk = slice_errors(k64, ref)
    lines, fails = [], []
    for l in range(len(wg)):
        bound = WHOLE_MARGIN[steps] * float(wn[l])
        sb = SLICE_MARGIN * max(SLICE_SPREAD[steps], 1.0) * torch.maximum(sn[l], sk[l])
        ratio = sg[l] / sb
        i, j = divmod(int(ratio.argmax()), ratio.shape[1])
        lines.append(f"{what} matrix {l} steps {steps}: whole kernel {float(wg[l]):.3e} yardstick {float(wn[l]):.3e} (ratio "
                     f"{float(wg[l] / wn[l]):.3f}, bound {WHOLE_MARGIN[steps]}); worst slice ({i}, {j}) of {tuple(ratio.shape)}: kernel "
                     f"{float(sg[l, i, j]):.3e} yardstick native {float(sn[l, i, j]):.3e} / chunk-64 {float(sk[l, i, j]):.3e} "
                     f"(kernel / bound {float(ratio[i, j]):.3f})")
        if not float(wg[l]) <= bound:
            fails.append(f"matrix {l}: whole-matrix error {float(wg[l]):.3e} > {WHOLE_MARGIN[steps]} x {float(wn[l]):.3e}")
        if not bool((sg[l] <= sb).all()):
            fails.append(f"matrix {l}: slice ({i}, {j}) error {float(sg[l, i, j]):.3e} > bound {float(sb[i, j]):.3e}")
    report = "\n".join(lines)
    print(report)
    assert not fails, f"{what}: " + "; ".join(fails) + "\n" + report
    return report
