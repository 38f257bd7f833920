"""Exactly summable operands for the GEMM family: inputs, fp64 references and the case table (no GPU in this module).

With small integer operands every product and every partial sum of a GEMM is an integer.  Below 2^24 the fp32 accumulators hold
each of them exactly, in any summation order, split, chunking or k-loop schedule, so the expected output is ONE bit pattern: the
GPU tests compare with torch.equal on the raw bits against a CPU fp64 product and no tolerance appears anywhere.

Input families (seeded, built on the CPU):
  wide     integers uniform in [-8, 8]: |sum| <= 64 K < 2^24 for every K used; an fp32 result is exact, a bf16 result is the RNE
           rounding of the exact integer (most outputs get rounded, many are exact ties: this pins the rounding mode of the store)
  ternary  entries in {-1, 0, 1}, each sign with probability 1/8: for the cells that store PARTIAL sums as bf16.  The running
           prefix of every output element at every 64-column boundary stays <= 128 in magnitude, so every sum over a run of whole
           k-tiles is an integer of magnitude <= 256, which bf16 holds exactly (tests/test_exact_gemm_cpu.py asserts it per case)

Sentinels: output buffers carry extra rows and (where the entry allows) ldc > N and are prefilled with a NaN bit pattern that must
come back untouched; operand columns the contract says are never read hold NaN; under the half-k-tile rule (include/swiftk.h,
swiftk_gemm: "pad columns must be finite; W's pad columns must be zero") A's pad holds finite non-zero integers, W's pad zeros.
"""
from __future__ import annotations

import zlib
from collections import namedtuple
from dataclasses import dataclass
from typing import Optional

import torch

GRID = 256                     # swiftk_get_tuning(2): workgroups of the persistent kernels (the GPU tests assert it)
SENT_F32 = 0x7FC12345          # quiet NaNs with a payload nothing computes
SENT_BF16 = 0x7FC1
ESHAPE = -2


@dataclass(frozen=True)
class Case:
    entry: str                 # gemm | chunked | splitk | splitk_bf16 | tail | batched | tn | swiglu_both | jvp | bias_pos_pair
    name: str
    M: int                     # tn: N1 (rows of the result); jvp: Mh (primal rows; A has 2 Mh)
    N: int                     # tn: N2
    K: int                     # tn: token count
    dt: str = "bf16"           # operand type: bf16 | f32
    out: str = "bf16"          # result type
    epi: str = "none"          # none | bias_pos | accum
    family: str = "wide"
    pad_a: int = 0             # lda = K + pad_a (tn: ldp = N1 + pad_a)
    pad_w: int = 0             # ldw = K + pad_w (tn: ldq = N2 + pad_w)
    pad_c: int = 0             # ldc = N + pad_c
    pos_rows: int = 0          # bias_pos: rows of pos (0: ep1 = NULL)
    ksplit: int = 1
    chunk_k: int = 0
    batch: int = 0
    gap: int = 0               # batched: elements between consecutive matrices of a stack
    rc: int = 0                # the return code the header's rules give
    cell: str = ""             # what the row is in the table for

    @property
    def lda(self):
        return (self.M if self.entry == "tn" else self.K) + self.pad_a

    @property
    def ldw(self):
        return (self.N if self.entry == "tn" else self.K) + self.pad_w

    @property
    def ldc(self):
        return self.N + self.pad_c

    @property
    def tile_k(self):
        return 64 if self.dt == "bf16" else 32

    @property
    def khalf(self):  # gemm.hip, gemm_impl: "K must fill whole 128-B k-tiles, or end exactly half-way into the last one provided ..."
        h = self.tile_k // 2
        return self.entry != "tn" and self.entry != "batched" and self.entry != "bias_pos_pair" and self.K % self.tile_k == h \
            and self.lda >= self.K + h and self.ldw >= self.K + h

    @property
    def nk(self):  # k-tiles of the contraction
        return (self.K + (self.tile_k // 2 if self.khalf else 0)) // self.tile_k

    @property
    def seed(self):
        return zlib.crc32(self.name.encode())

    @property
    def flops(self):
        rows = 2 * self.M if self.entry == "jvp" else self.M
        return 2 * rows * self.N * self.K * max(1, self.batch)


# ------------------------------------------------------------------------------------------------ inputs and references
def ints(shape, family, seed):
    g = torch.Generator().manual_seed(seed)
    if family == "wide":
        return torch.randint(-8, 9, shape, generator=g, dtype=torch.int8)
    r = torch.randint(0, 8, shape, generator=g, dtype=torch.int8)
    return (r == 0).to(torch.int8) - (r == 1).to(torch.int8)


def operand(rows, K, ld, family, seed, half_pad=None):
    """[rows, ld] fp32 holding integers in [:, :K] and NaN behind them; half_pad = (width, value) fills [K, K + width) instead
    (the half-k-tile rule: finite non-zero for A, zero for W)."""
    x = torch.full((rows, ld), float("nan"))
    x[:, :K] = ints((rows, K), family, seed).float()
    if half_pad:
        x[:, K:K + half_pad[0]] = half_pad[1]
    return x


def operands(c: Case):
    """(A, W) of a row-major NT case as fp32 CPU tensors [rows, ld]."""
    h = c.tile_k // 2
    rows_a = 2 * c.M if c.entry == "jvp" else c.M
    a = operand(rows_a, c.K, c.lda, c.family, c.seed, (h, 3.0) if c.khalf else None)
    w = operand(c.N, c.K, c.ldw, c.family, c.seed + 1, (h, 0.0) if c.khalf else None)
    return a, w


def rows_and_reference(c: Case):
    """(A, W, fp64 product) of a row.  TN form: (P [tokens, ldp], Q [tokens, ldq], P^T Q); batched: the matrices of a stack one under
    the other ([batch M, lda], [batch N, ldw]) and the products [batch, M, N]."""
    if c.entry == "tn":
        p = operand(c.K, c.M, c.lda, c.family, c.seed)
        q = operand(c.K, c.N, c.ldw, c.family, c.seed + 1)
        return p, q, p[:, :c.M].double().t() @ q[:, :c.N].double() + 0.0
    if c.entry == "batched":
        a = operand(c.batch * c.M, c.K, c.lda, c.family, c.seed)
        w = operand(c.batch * c.N, c.K, c.ldw, c.family, c.seed + 1)
        return a, w, torch.bmm(a[:, :c.K].double().view(c.batch, c.M, c.K), w[:, :c.K].double().view(c.batch, c.N, c.K).transpose(1, 2)) + 0.0
    a, w = operands(c)
    return a, w, product(a, w, 0, c.K)


def product(a, w, k0=0, k1=None):
    """fp64 product over the columns [k0, k1) (exact: every partial sum is an integer far below 2^53); + 0.0 folds -0 into +0."""
    return a[:, k0:k1].double() @ w[:, k0:k1].double().t() + 0.0


def k_range(c: Case, s, ksplit=None):
    """Columns of k-range s: k-tiles [s T / ksplit, (s + 1) T / ksplit) (include/swiftk.h, swiftk_gemm_splitk), clipped to K."""
    ks = ksplit or c.ksplit
    return min(c.K, s * c.nk // ks * c.tile_k), min(c.K, (s + 1) * c.nk // ks * c.tile_k)


def epilogue_terms(c: Case):
    """Integer bias [N], pos [pos_rows, N] (or None) and prefill C0 [M, N] of the BIAS_POS / ACCUM epilogues, fp32."""
    bias = ints((c.N,), "wide", c.seed + 2).float()
    pos = ints((c.pos_rows, c.N), "wide", c.seed + 3).float() if c.pos_rows else None
    c0 = ints((c.M, c.N), "wide", c.seed + 4).float()
    return bias, pos, c0


def bias_pos_sum(c: Case, ref, bias, pos):
    out = ref + bias.double()
    if pos is not None:
        out = out + pos.double()[torch.arange(c.M) % c.pos_rows]
    return out


def to_bits(x64, out):
    """The one bit pattern an exact result has: fp32 as is, bf16 as RNE of the exact value."""
    if out == "f32":
        return x64.float().contiguous().view(torch.int32)
    return x64.float().bfloat16().contiguous().view(torch.int16)


def prefix_max(a, w, K, tile=64, block=4096):
    """Largest |sum over columns [0, 64 t)| of any output element at any k-tile boundary t (and at K).  (k-tile-major contiguous
    copies and large row blocks: the 64-deep products are what this costs.)"""
    T, mx = K // tile, 0.0
    chunks = lambda x: x[:, :T * tile].float().reshape(x.shape[0], T, tile).permute(1, 0, 2).contiguous()  # [T, rows, 64]
    wt, w_rest = chunks(w), w[:, T * tile:K].float()
    for r0 in range(0, a.shape[0], block):
        at, a_rest = chunks(a[r0:r0 + block]), a[r0:r0 + block, T * tile:K].float()
        acc = torch.zeros(at.shape[1], w.shape[0])
        run, tmp = torch.zeros_like(acc), torch.empty_like(acc)
        for t in range(T + (K > T * tile)):
            acc.addmm_(at[t], wt[t].t()) if t < T else acc.addmm_(a_rest, w_rest.t())
            torch.maximum(run, torch.abs(acc, out=tmp), out=run)
        mx = max(mx, float(run.max()))
    return mx


# ------------------------------------------------------------------------------------------------ the dispatch, restated
Cell = namedtuple("Cell", "entry dt out epi kernel width kloop rounds nk khalf trigger")


def rounds_of(items, grid=GRID):
    if items < grid:
        return "below"
    if items == grid:
        return "equal"
    r = items % grid
    if r == 0:
        return "full"
    if r == 1:
        return "last_1"
    if r == grid - 1:
        return "last_all_but_one"
    return "last_half" if grid // 4 <= r <= 3 * grid // 4 else "last_other"


def expected_cell(c: Case, grid=GRID) -> Cell:
    """Which kernel a row runs.  Restates swift_amd/csrc/gemm.hip: gemm_impl (khalf rule, tile width `ni` from N, kchunk, the tail
    form: "K must fill whole 128-B k-tiles ..." down to the dispatch_epi calls), pp_ok, launch() (one-tile kernel when M % 8, N % 8
    or a bf16 store that cannot move 16-B row chunks; else the persistent kernel at ni = 10 / 11 / 12, ping-pong k-loop for bf16
    operands with >= 3 k-tiles per work item), launch_paired(), swiftk_gemm_jvp / _bias_pos_pair / _batched; and gemm_tn.hip:
    swiftk_gemm_tn_splitk (tile width, ping-pong always at the default of tuning key 22)."""
    cdiv = lambda a, b: -(-a // b)
    nkc = lambda n: str(n) if n <= 3 else "many"
    if c.entry == "tn":
        ni = 11
        if c.N % 352:
            ni = 12 if cdiv(c.N, 384) * 384 <= cdiv(c.N, 320) * 320 else 10
        items = cdiv(c.M, 256) * cdiv(c.N, 32 * ni) * c.ksplit
        return Cell("tn", "bf16", "f32", "none", "tn", 32 * ni, "pp", rounds_of(items, 256), nkc(c.K // 64 // c.ksplit), False, "")
    if c.entry == "batched":
        return Cell(c.entry, c.dt, c.out, "none", "one_tile", 352, "two_stage", "tile_per_wg", nkc(c.nk), False, "batched")
    ni = 11
    if c.entry == "bias_pos_pair":
        ni = 10 if c.N % 352 and c.N % 320 == 0 else 11
    elif c.dt == "bf16" and c.N % 352:
        ni = 12 if c.N % 384 == 0 else 10 if c.N % 320 == 0 else 11
    rows = 2 * c.M if c.entry == "jvp" else c.M
    paired = c.entry in ("jvp", "bias_pos_pair")
    trigger = ""
    if not paired and c.entry != "tail":
        wide_ok = c.out != "bf16" or (c.ldc % 8 == 0 and c.N % (16 if c.entry == "swiglu_both" else 8) == 0)
        trigger = "M%8" if c.M % 8 else "N%8" if c.N % 8 else "" if wide_ok else "ldc%8"
    if trigger:
        return Cell(c.entry, c.dt, c.out, c.epi, "one_tile", 352, "two_stage", "tile_per_wg", nkc(c.nk), c.khalf, trigger)
    tiles = cdiv(rows, 256) * cdiv(c.N, 32 * ni)
    if c.entry == "tail":
        return Cell(c.entry, c.dt, c.out, c.epi, "tail", 352, "pp", rounds_of(2 * tiles - (tiles - tiles % grid), grid), nkc(c.nk // 2),
                    c.khalf, "")
    kloop = "pp" if c.dt == "bf16" and c.nk // c.ksplit >= 3 else "one_barrier"
    if c.entry == "chunked":
        chains = max(1, c.nk // (c.chunk_k // 32))
        kloop += f"+chains{chains}" if chains > 1 else "+one_chain"
    return Cell(c.entry, c.dt, c.out, c.epi, "persistent", 32 * ni, kloop, rounds_of(tiles * c.ksplit, grid), nkc(c.nk // c.ksplit),
                c.khalf, "")


# ------------------------------------------------------------------------------------------------ the case table
TYPES = {"bb": ("bf16", "bf16"), "bf": ("bf16", "f32"), "ff": ("f32", "f32")}
CASES: list = []


def _add(entry, name, M, N, K, types="bb", **kw):
    for t in types.split(","):
        dt, out = TYPES[t]
        k = K[t] if isinstance(K, dict) else K
        CASES.append(Case(entry, f"{name}-{t}", M, N, k, dt, out, **kw))


ALL = "bb,bf,ff"
# ---- swiftk_gemm, EPI_NONE.  One-tile kernel through each of its three triggers
_add("gemm", "one_tile_M%8", 301, 704, 192, ALL, pad_c=8, cell="one-tile kernel: M % 8 != 0")
_add("gemm", "one_tile_N%8", 512, 276, {"bb": 1088, "bf": 1088, "ff": 544}, ALL, pad_c=4, cell="one-tile kernel: N % 8 == 4")
_add("gemm", "one_tile_ldc%8", 512, 704, 128, "bb", pad_c=4, cell="one-tile kernel: bf16 rows that are not whole 16-B chunks")
_add("gemm", "one_tile_khalf", 301, 704, {"bb": 1056, "ff": 1072}, "bb,ff", pad_a=32, pad_w=32, cell="one-tile kernel, half k-tile")
# persistent kernel: the three widths below the grid, ragged edges
_add("gemm", "p352_below", 2048, 3168, {"bb": 1088, "bf": 1088, "ff": 544}, ALL, pad_c=8, cell="persistent 352, 72 tiles")
_add("gemm", "p320_below", 1024, 2560, 192, "bb,bf", pad_c=8, cell="persistent 320 (N = 1280 k)")
_add("gemm", "p384_below", 1024, 3072, 192, "bb,bf", pad_c=8, cell="persistent 384 (N = 1536 k)")
_add("gemm", "p320_rounds", 8448, 2560, 192, "bb,bf", cell="persistent 320, 264 tiles")
_add("gemm", "p384_rounds", 8448, 3072, 192, "bb,bf", cell="persistent 384, 264 tiles")
_add("gemm", "ragged_cols_6832", 512, 6832, 1280, "bb,bf", pad_c=8, cell="ragged last column tile (468 M variant's w1 width)")
_add("gemm", "ragged_rows", 1000, 1056, {"bb": 576, "bf": 576, "ff": 288}, ALL, pad_c=8, cell="ragged last row tile, M % 8 == 0")
# tile counts against the grid of 256 workgroups
_add("gemm", "tiles_256", 16384, 1408, {"bb": 192, "bf": 192, "ff": 96}, ALL, cell="tiles == grid")
_add("gemm", "tiles_257", 65792, 352, {"bb": 192, "bf": 192, "ff": 96}, ALL, pad_c=8, cell="two rounds, 1 tile in the last")
_add("gemm", "tiles_384", 32768, 1056, {"bb": 192, "bf": 192, "ff": 96}, ALL, cell="two rounds, half of the last")
_add("gemm", "tiles_511", 18688, 2464, {"bb": 192, "bf": 192, "ff": 96}, ALL, cell="two rounds, all but one of the last")
# k-tile counts: one-barrier loop below three k-tiles, ping-pong from three (bf16 operands); several tiles per workgroup
for nk_ in (1, 2, 3):
    _add("gemm", f"ktiles_{nk_}", 8448, 3168, {"bb": 64 * nk_, "bf": 64 * nk_, "ff": 32 * nk_}, ALL, pad_a=64, pad_w=64,
         cell=f"{nk_} k-tile(s), 297 tiles, lda / ldw > K")
_add("gemm", "ktiles_many", 8448, 3168, {"bb": 1088, "ff": 352}, "bb,ff", cell="many k-tiles, 297 tiles")
_add("gemm", "ktiles_44", 1024, 1056, {"bb": 2816, "bf": 2816, "ff": 1408}, ALL, pad_a=64, pad_w=128, cell="44 k-tiles, lda != ldw")
# half k-tile
_add("gemm", "khalf_rounds", 8448, 3168, 1056, "bb", pad_a=32, pad_w=32, cell="K = 16.5 k-tiles, rows of 1088, 297 tiles")
_add("gemm", "khalf", 1024, 1056, {"bf": 1056, "ff": 1072}, "bf,ff", pad_a=32 + 64, pad_w=32, cell="half k-tile, rows extended")
# ---- SWIFTK_EPI_BIAS_POS
_add("gemm", "bias_pos_96", 1000, 1056, 576, "bf", epi="bias_pos", pos_rows=96, pad_c=8, cell="pos_rows not a power of two, not dividing M")
_add("gemm", "bias_pos_384", 1024, 1056, 288, "ff", epi="bias_pos", pos_rows=384, cell="pos_rows > 256, not dividing M")
_add("gemm", "bias_pos_100", 1000, 1280, 192, "bb", epi="bias_pos", pos_rows=100, pad_c=8, cell="bf16 store of the integer sum, 320 wide")
_add("gemm", "bias_pos_null", 1000, 1056, 192, "bf,ff", epi="bias_pos", pos_rows=0, cell="ep1 = NULL")
_add("gemm", "bias_pos_rounds", 8448, 3168, 192, "bf", epi="bias_pos", pos_rows=1000, cell="several rounds")
_add("gemm", "bias_pos_one_tile", 1004, 1056, {"bf": 192, "ff": 96}, "bf,ff", epi="bias_pos", pos_rows=96, pad_c=4, cell="one-tile kernel")
_add("gemm", "bias_pos_one_tile_384", 512, 276, 128, "bb", epi="bias_pos", pos_rows=384, pad_c=4, cell="one-tile kernel, bf16 out")
# ---- SWIFTK_EPI_ACCUM (called twice: C0 + ref, C0 + 2 ref)
_add("gemm", "accum_352", 8448, 3168, {"bf": 192, "ff": 96}, "bf,ff", epi="accum", pad_c=8, cell="several rounds")
_add("gemm", "accum_320", 8448, 2560, 192, "bf", epi="accum", cell="320 wide, several rounds")
_add("gemm", "accum_384", 8448, 3072, 192, "bf", epi="accum", cell="384 wide, several rounds")
_add("gemm", "accum_ragged", 1000, 1056, 1056, "bf", epi="accum", pad_a=32, pad_w=32, pad_c=4, cell="ragged rows, half k-tile")
# ---- every (epilogue, result type, tile width, k-loop) the dispatch has for bf16 operands: 2 k-tiles take the one-barrier loop,
# 3 the ping-pong loop; two tile rows, a ragged last row tile
for epi_ in ("none", "bias_pos", "accum"):
    for n_ in (1056, 1280, 1536):
        for k_ in (128, 192):
            _add("gemm", f"cross_{epi_}_N{n_}_K{k_}", 504, n_, k_, "bf" if epi_ == "accum" else "bb,bf", epi=epi_, pad_c=8,
                 pos_rows=96 if epi_ == "bias_pos" else 0, cell=f"{epi_}, {32 * (n_ // 96 if n_ % 352 else 11)} wide, {k_ // 64} k-tiles")
# ---- swiftk_gemm_chunked (fp32 operands; K = 1056 is 33 k-tiles: chains of 9, 9, 9, 6 at chunk_k = 256)
for ck in (32, 64, 256, 4096):
    _add("chunked", f"chunk{ck}_K1056", 1024, 1056, 1056, "ff", chunk_k=ck, pad_c=8, cell=f"chunk_k {ck}")
_add("chunked", "chunk256_K2816", 512, 704, 2816, "ff", chunk_k=256, cell="K = 2816")
_add("chunked", "chunk256_khalf", 1024, 1056, 1072, "ff", chunk_k=256, pad_a=16, pad_w=16, cell="half k-tile")
_add("chunked", "chunk64_rounds", 76840, 352, 192, "ff", chunk_k=64, cell="301 tiles: the parked slab is re-used tile after tile")
_add("chunked", "chunk256_bias_pos", 1000, 1056, 1056, "ff", chunk_k=256, epi="bias_pos", pos_rows=96, cell="BIAS_POS behind merged accumulators")
_add("chunked", "chunk256_accum", 1000, 1056, 1056, "ff", chunk_k=256, epi="accum", pad_c=8, cell="ACCUM behind merged accumulators")
# ---- swiftk_gemm_splitk (fp32 slabs); ksplit > k-tiles is rejected (no empty k-range)
for ks in (2, 3, 4, 16):
    _add("splitk", f"splitk{ks}", 2048, 1056, {"bf": 2816, "ff": 1056}, "bf,ff", ksplit=ks, pad_c=8, cell=f"ksplit {ks}")
_add("splitk", "splitk2_khalf", 8192, 1056, 1056, "bf", ksplit=2, pad_a=32, pad_w=32, cell="wo at one unit per step: 8 + 8.5 k-tiles")
_add("splitk", "splitk_more_than_ktiles", 512, 704, {"bf": 128, "ff": 64}, "bf,ff", ksplit=3, rc=ESHAPE, cell="ksplit > k-tiles")
# ---- swiftk_gemm_splitk_bf16 (bf16 slabs: ternary, every slab exact)
for ks in (2, 3, 4, 16):
    _add("splitk_bf16", f"splitk_bf16_{ks}", 2048, 1056, 2816, "bb", ksplit=ks, family="ternary", pad_c=8, cell=f"ksplit {ks}")
_add("splitk_bf16", "splitk_bf16_2_khalf", 8192, 1056, 1056, "bb", ksplit=2, family="ternary", pad_a=32, pad_w=32, cell="w2 / wo at one unit")
_add("splitk_bf16", "splitk_bf16_more_than_ktiles", 512, 704, 128, "bb", ksplit=3, family="ternary", rc=ESHAPE, cell="ksplit > k-tiles")
# ---- swiftk_gemm_tail_split_bf16: 3, 4 and 6 units of 8192 rows
_add("tail", "tail_3u_K1056", 3 * 8192, 1056, 1056, "bb", family="ternary", pad_a=32, pad_w=32, cell="288 tiles, 32 split, half k-tile")
_add("tail", "tail_4u_K2816", 4 * 8192, 1056, 2816, "bb", family="ternary", cell="384 tiles, 128 split")
_add("tail", "tail_6u_K1056", 6 * 8192, 1056, 1056, "bb", family="ternary", pad_a=32, pad_w=32, cell="576 tiles, 64 split, half k-tile")
# ---- swiftk_gemm_batched (the one-tile kernel, blockIdx.y = matrix)
_add("batched", "batch1", 320, 100, 64, "bb,bf", batch=1, pad_c=4, gap=64, cell="ragged row tile, N % 8 == 4, one k-tile")
_add("batched", "batch3", 320, 96, 1088, "bb,bf", batch=3, pad_a=64, pad_c=8, gap=128, cell="17 k-tiles, strides past the matrices")
_add("batched", "batch12", 264, 708, 1088, "bb,bf", batch=12, pad_c=4, gap=256, cell="twelve matrices, three column tiles")
# ---- swiftk_gemm_tn_splitk (M, N, K = N1, N2, tokens; pad = ldp - N1, ldq - N2): the table of test_tn_wgrad_equals_transposed_path
for i, (tok, n1, n2, ks, ldp, ldq) in enumerate([(1024, 1056, 704, 3, 1088, 704), (4096, 256, 352, 16, 320, 360), (2048, 3168, 1056, 1, 3200, 1088),
                                                 (640, 72, 1408, 2, 128, 1408), (1024, 1280, 1280, 2, 1280, 1280), (1024, 512, 1536, 1, 512, 1536),
                                                 (512, 1536, 3416, 1, 1536, 3456),
                                                 (448, 512, 704, 2, 512, 704)]):  # 7 k-tiles in 2 ranges: 3 + 4
    _add("tn", f"tn{i}_{n1}x{n2}_t{tok}_ks{ks}", n1, n2, tok, "bf", ksplit=ks, pad_a=ldp - n1, pad_w=ldq - n2, cell="weight gradient, TN form")
_add("tn", "tn_rows_end_inside_a_block", 1056, 1280, 256, "bf", rc=ESHAPE, cell="ldp = 1056 < 1088: P rows end inside a 64-column block")
# ---- linear outputs of the fused epilogues (ternary: the bf16 value IS the integer)
for H in (2816, 2560, 3072):
    _add("swiglu_both", f"swiglu_both_H{H}", 1000, 2 * H, 1056, "bb", family="ternary", pad_a=32, pad_w=32, cell="pre-activation of the training forward")
_add("jvp", "jvp_swiglu_1056", 256, 2 * 2816, 1056, "bb", family="ternary", pad_a=32, pad_w=32, cell="kept pre-activation, half k-tile")
_add("jvp", "jvp_swiglu_1280", 128, 2 * 3416, 1280, "bb", family="ternary", cell="kept pre-activation, ragged last column tile")
_add("jvp", "jvp_swiglu_1536", 384, 2 * 4096, 1536, "bb", family="ternary", cell="kept pre-activation, 352-wide tiles over 8192 columns")
_add("bias_pos_pair", "pair_1056", 2048, 1056, 576, "bb", family="ternary", pos_rows=512, pad_c=32, cell="hi = the integer, lo = 128")
_add("bias_pos_pair", "pair_1280", 1032, 1280, 192, "bb", family="ternary", pos_rows=0, pad_c=64, cell="pos = NULL, 320 wide")
_add("bias_pos_pair", "pair_1536", 512, 1536, 576, "bb", family="ternary", pos_rows=256, pad_c=64, cell="352-wide tiles over 1536 columns")
_add("bias_pos_pair", "pair_pos96", 1000, 1056, 192, "bb", family="ternary", pos_rows=96, pad_c=32, cell="pos_rows not a power of two")

assert len({c.name for c in CASES}) == len(CASES)


def cases(*entries):
    return [c for c in CASES if c.entry in entries]


# The dispatch cells the table must cover, as partial cells: each must be matched by at least one row (test_exact_gemm_cpu.py).
def _req():
    R = []
    for dt, out in TYPES.values():
        for trig in ("M%8", "N%8"):
            R.append(dict(entry="gemm", epi="none", dt=dt, out=out, kernel="one_tile", trigger=trig))
        R.append(dict(entry="gemm", epi="none", dt=dt, out=out, kernel="persistent", width=352))
        for rounds in ("below", "equal", "last_1", "last_half", "last_all_but_one"):
            R.append(dict(entry="gemm", epi="none", dt=dt, out=out, kernel="persistent", rounds=rounds))
        for nk in ("1", "2", "3", "many"):
            R.append(dict(entry="gemm", epi="none", dt=dt, out=out, kernel="persistent", nk=nk))
        R.append(dict(entry="gemm", epi="none", dt=dt, out=out, kernel="persistent", khalf=True))
    R.append(dict(entry="gemm", epi="none", dt="bf16", out="bf16", kernel="one_tile", trigger="ldc%8"))
    for out in ("bf16", "f32"):
        for width in (320, 384):
            R.append(dict(entry="gemm", epi="none", dt="bf16", out=out, kernel="persistent", width=width))
        R.append(dict(entry="gemm", epi="none", dt="bf16", out=out, kernel="persistent", kloop="pp"))
        R.append(dict(entry="gemm", epi="none", dt="bf16", out=out, kernel="persistent", kloop="one_barrier"))
    # the persistent kernel's instantiations for the linear epilogues with bf16 operands: <out, epilogue, width, ping-pong or not>
    for epi in ("none", "bias_pos", "accum"):
        for out in ("f32",) if epi == "accum" else ("bf16", "f32"):
            for width in (320, 352, 384):
                for kloop in ("pp", "one_barrier"):
                    R.append(dict(entry="gemm", epi=epi, dt="bf16", out=out, kernel="persistent", width=width, kloop=kloop))
    # fp32 operands: one instantiation per epilogue (352 wide, one barrier per k-tile); the one-tile kernel has no ACCUM
    for epi in ("none", "bias_pos", "accum"):
        R.append(dict(entry="gemm", epi=epi, dt="f32", out="f32", kernel="persistent", width=352, kloop="one_barrier"))
    for dt, out in TYPES.values():
        for epi in ("none", "bias_pos"):
            R.append(dict(entry="gemm", epi=epi, dt=dt, out=out, kernel="one_tile"))
    for width in (320, 352, 384):
        R.append(dict(entry="gemm", epi="accum", kernel="persistent", width=width, rounds="last_other"))
    R.append(dict(entry="chunked", kloop="one_barrier+one_chain"))
    R.append(dict(entry="chunked", kloop="one_barrier+chains4"))
    R.append(dict(entry="chunked", khalf=True))
    R.append(dict(entry="chunked", rounds="last_other"))
    R.append(dict(entry="chunked", epi="bias_pos"))
    R.append(dict(entry="chunked", epi="accum"))
    for dt in ("bf16", "f32"):
        R.append(dict(entry="splitk", dt=dt, kernel="persistent"))
    R.append(dict(entry="splitk", khalf=True))
    R.append(dict(entry="splitk_bf16", kloop="pp"))
    R.append(dict(entry="splitk_bf16", kloop="one_barrier"))
    R.append(dict(entry="tail", khalf=True))
    R.append(dict(entry="tail", khalf=False))
    for out in ("bf16", "f32"):
        R.append(dict(entry="batched", out=out))
    for width in (320, 352, 384):
        R.append(dict(entry="tn", width=width))
        R.append(dict(entry="swiglu_both", width=width))
    R.append(dict(entry="jvp", khalf=True))
    for width in (320, 352):
        R.append(dict(entry="bias_pos_pair", width=width))
    return R


REQUIRED = _req()
