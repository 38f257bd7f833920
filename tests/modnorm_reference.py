"""TEST INFRASTRUCTURE: the forward ModulatedNorm + residual, x += LN(y) (1 + scale_b) + shift_b, as plain PyTorch-CPU code, the
hostile-row inputs of tests/test_gpu_modnorm_rows.py and the bars that module scores every row against.

  * ``modnorm_forward``    -- the operation in fp64 (the reference) or in fp32 in the kernels' order of operations (the yardstick:
                              mean, centred squares, rsqrt; P = gamma (1 + sc), Q = beta (1 + sc) + sh; x + ((c rstd) P + Q)), with a
                              keyword that commits one named mistake (``VARIANTS``) for the sensitivity checks
  * ``make_forward_case``  -- seeded inputs with seven hostile y rows (``KINDS``) placed where the kernels' row batches and register
                              sets change (``hostile_rows``) and one all-zero x row
  * ``row_errs``, ``f32_row_bar``, ``pair_bound`` -- the per-row / per-element bars

``pair_quantise``, ``row_err`` and ``bf16_round`` are those of tests/tangent_reference.py.  tests/test_modnorm_reference_cpu.py
pins the reference to the oracle and shows that every variant misses the bars on the rows built to catch it.
"""
from __future__ import annotations

import torch

from tangent_reference import bf16_round, pair_quantise, row_err

VARIANTS = ("one_pass", "no_eps", "neighbour_sample", "neighbour_row_stats", "drop_last_slot", "padded_d")
F32_TOL = 1e-5  # floor of a row's bar (tests/test_gpu_tangent_kernels.py: F32_TOL)
FACTOR = 4      # a kernel row may err FACTOR x as far as the fp32 yardstick's (the same file's hostile-row rule)
CHUNK = 16      # rows of a workgroup of the chunked kernels (elementwise.hip: MN_ROWS)
WIDTHS = (8, 64, 512, 520, 1056, 1280, 1536, 1544, 2048)  # every row width tests/test_gpu_modnorm_rows.py runs
CASE_SEED = 3    # the seed of the GPU module's cases.  How far a one-pass variance misses on ONE row E depends on where that row's few
                 # roundings fall (eight seeds x six widths: 0 .. 640 x the bar, a tenth of them under 3 x); on this seed it is
                 # >= 20 x at every width from 520 on (tests/test_modnorm_reference_cpu.py asserts 3 x)
ZERO_X_ROW = 13  # the all-zero x row (a benign y row; as a pair: hi = 0, byte 128)

# hostile y rows, all bf16-representable
KINDS = {
    "A": "element 0 = 300: an outlier in the first element",
    "B": "constant 40: variance 0, rstd = 1 / sqrt(eps)",
    "C": "zero but for one element 1e-3: a nearly empty row",
    "D": "element d - 1 = -500: an outlier in the last lane of the last live slot",
    "E": "63.5 + 0.25 Bernoulli(1/2): a large mean with a spread of one bf16 step (a one-pass variance)",
    "F": "3e4 randn: large magnitude",
    "G": "1e-3 randn: variance about eps",
}


def hostile_rows(rows_per_sample: int, M: int) -> dict:
    """row -> kind.  Rows 1, 6, 11, 12 are positions 1, 2, 3, 0 of the packed kernel's four-row batches in waves 0, 1, 2, 3 of chunk 0
    and, for the row-per-wave kernels (wave w: rows w, w + 4, ...), waves 1, 2, 3, 0 on trips 0, 1, 2, 3: both register sets.  Then
    the last row of sample 0, the first of sample 1 and the last row of all.  Neighbours are benign, but 11 | 12 and the two rows
    at the sample boundary, which are of different kinds."""
    assert rows_per_sample >= 14 and M >= 2 * rows_per_sample
    return {1: "A", 6: "B", 11: "C", 12: "D", rows_per_sample - 1: "E", rows_per_sample: "F", M - 1: "G"}


def _per_row(m: torch.Tensor, sample: torch.Tensor) -> torch.Tensor:
    return m.index_select(0, sample)


def modnorm_forward(y, x, gamma, beta, mod, rows_per_sample, eps=1e-6, dtype=torch.float64, variant=None):
    """x + LN(y) (1 + sc_b) + sh_b.  y, x [M, d]; mod = (sc | sh) [B, 2d]; sample b owns rows b rps .. (b + 1) rps - 1.
    ``variant`` (one of VARIANTS) commits one deliberate mistake:
      one_pass             the variance as E[y^2] - mean^2, unshifted
      no_eps               rstd without eps
      neighbour_sample     the 16-row chunk on either side of a sample boundary takes the other sample's modulation
      neighbour_row_stats  row r is normalised with the mean / rstd of row r + 1 (the last row: of row 0)
      drop_last_slot       the last 8 channels are left out of both sums (which are still divided by d)
      padded_d             the sums are divided by d rounded up to 512"""
    assert variant is None or variant in VARIANTS
    y, x, gamma, beta, mod = (v.to(dtype) for v in (y, x, gamma, beta, mod))
    M, d = y.shape
    B = mod.shape[0]
    rows = torch.arange(M)
    sample = rows // rows_per_sample
    if variant == "neighbour_sample":
        edge = min(CHUNK, rows_per_sample // 2)
        r = rows % rows_per_sample
        sample = torch.where((r >= rows_per_sample - edge) & (sample < B - 1), sample + 1,
                             torch.where((r < edge) & (sample > 0), sample - 1, sample))
    sc, sh = _per_row(mod[:, :d], sample), _per_row(mod[:, d:2 * d], sample)
    live = y[:, :d - 8] if variant == "drop_last_slot" else y
    n_div = float(-(-d // 512) * 512) if variant == "padded_d" else float(d)
    mu = live.sum(1, keepdim=True) / n_div
    if variant == "one_pass":
        var = ((live * live).sum(1, keepdim=True) / n_div - mu * mu).clamp_min(0.0)
    else:
        cl = live - mu
        var = (cl * cl).sum(1, keepdim=True) / n_div
    rstd = torch.rsqrt(var.clamp_min(1e-30) if variant == "no_eps" else var + eps)
    if variant == "neighbour_row_stats":
        mu, rstd = mu.roll(-1, 0), rstd.roll(-1, 0)
    P = gamma * (1.0 + sc)
    Q = beta * (1.0 + sc) + sh
    return x + (((y - mu) * rstd) * P + Q)


def make_forward_case(d: int, seed: int, bf16_y: bool = True, rows_per_sample: int = 32, B: int = 3) -> dict:
    """Inputs of the forward tests (fp32 CPU tensors): benign rows as in tangent_reference.make_norm_case -- y = 2 randn + 0.5 rounded
    to bf16 (``bf16_y`` False: they keep their fp32 values), x of std 1, gamma = 1 + 0.1 randn, beta = 0.1 randn, mod = 0.3 randn
    [B, 2d] (the wrong sample's modulation is a gross error) -- the hostile rows of ``hostile_rows`` and x[ZERO_X_ROW] = 0."""
    assert d >= 8 and d % 8 == 0
    g = torch.Generator().manual_seed(seed)
    rn = lambda *shape: torch.randn(*shape, generator=g)
    M = B * rows_per_sample
    y, x = 2.0 * rn(M, d) + 0.5, rn(M, d)
    gamma, beta, mod = 1.0 + 0.1 * rn(d), 0.1 * rn(d), 0.3 * rn(B, 2 * d)
    coin = (torch.rand(d, generator=g) < 0.5).float()
    big, small = bf16_round(3e4 * rn(d)), bf16_round(1e-3 * rn(d))
    if bf16_y:
        y = bf16_round(y)
    hostile = hostile_rows(rows_per_sample, M)
    for r, kind in hostile.items():
        if kind in "AD":
            y[r] = bf16_round(y[r])
            y[r, 0 if kind == "A" else d - 1] = 300.0 if kind == "A" else -500.0
        elif kind == "B":
            y[r] = 40.0
        elif kind == "C":
            y[r] = 0.0
            y[r, 5] = bf16_round(torch.tensor(1e-3))
        elif kind == "E":
            y[r] = 63.5 + 0.25 * coin
        elif kind == "F":
            y[r] = big
        elif kind == "G":
            y[r] = small
    assert ZERO_X_ROW not in hostile
    x[ZERO_X_ROW] = 0.0
    return dict(y=y, x=x, gamma=gamma, beta=beta, mod=mod, rows_per_sample=rows_per_sample, hostile=hostile)


def forward_args(c: dict) -> dict:
    """The keyword arguments of ``modnorm_forward`` held by a case."""
    return {k: c[k] for k in ("y", "x", "gamma", "beta", "mod", "rows_per_sample")}


# ---------------------------------------------------------------------------------------------------------------------- bars

def row_errs(a: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """``row_err`` of every row, fp64 [M] (a row holding a non-finite value scores inf)."""
    e = torch.tensor([row_err(a[r], ref[r]) for r in range(ref.shape[0])], dtype=torch.float64)
    return torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))


def f32_row_bar(yard: torch.Tensor, ref64: torch.Tensor) -> torch.Tensor:
    """fp32 outputs, per row: row_err(kernel, ref64) <= max(FACTOR row_err(yardstick, ref64), F32_TOL)."""
    return (FACTOR * row_errs(yard, ref64)).clamp_min(F32_TOL)


def biased_exponent(hi: torch.Tensor) -> torch.Tensor:
    return (hi.to(torch.bfloat16).contiguous().view(torch.int16).to(torch.int32) >> 7) & 0xFF


def pair_bound(hi: torch.Tensor, yard: torch.Tensor, ref64: torch.Tensor) -> torch.Tensor:
    """Pair outputs, per element: |value - ref64| <= 2^(E - 142) + max(FACTOR max_row |yardstick - ref64|, F32_TOL max|ref row|),
    E the larger biased exponent of ``hi`` (the hi part under test) and bf16(ref64).  The first term is one byte step of the 8-bit low
    part: its half-step rounding plus the saturated byte 255 that ``pair_quantise`` documents (loose by 2 x for a 16-bit low part)."""
    E = torch.maximum(biased_exponent(hi), biased_exponent(ref64.float()))
    step = torch.ldexp(torch.ones_like(ref64), E - 142)
    yard_worst = (yard.double() - ref64).abs().amax(1, keepdim=True)
    return step + torch.maximum(FACTOR * yard_worst, F32_TOL * ref64.abs().amax(1, keepdim=True))


def pair_excess(value: torch.Tensor, hi: torch.Tensor, yard: torch.Tensor, ref64: torch.Tensor) -> torch.Tensor:
    """Per row, the largest |value - ref64| / pair_bound of its elements (<= 1 passes; non-finite values score inf)."""
    q = (value.double() - ref64).abs() / pair_bound(hi, yard, ref64)
    q = torch.where(torch.isfinite(q), q, torch.full_like(q, float("inf")))
    return q.amax(1)
