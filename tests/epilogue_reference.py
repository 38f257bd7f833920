"""The non-linear epilogues of swiftk_gemm / swiftk_gemm_jvp on exactly summable operands: inputs, fp64 closed forms, their fp32
restatements, the bounds and the case table (no GPU in this module).

Operands.  A and W are exact_gemm.ints(..., "ternary", seed); row m of A is scaled by 2^-(m mod 4), so every product and partial sum
is an integer times 1/8 far below 2^24 quanta: the fp32 accumulators ENTERING an epilogue are known bit for bit in any k-loop, split
or schedule, and what a comparison measures is the epilogue's own arithmetic and one output rounding.  The gates land on multiples of
1, 1/2, 1/4, 1/8 in about [-15, 15]; QK-norm is invariant to the row scaling.  Planted primal rows of A: row ZERO_ROW = 5 is all zero
(its q and k vectors are zero: the max(|.|, 1e-12) clamp decides the output, 0, and rn, 1e12) and row sat_row = 4 ((M - 1) // 4) is multiplied
by 8 (gates of about +-100: saturated SiLU; rows 0, 2, 4, 6 of W are planted so that its gates 0 .. 3 are exactly +96, -96, -96, +96).  Logit scales per head lie below, at (4.605170185988092f, the kernel's own constant) and
above ln 100.  SWIGLU_BWD's saved pre-activation H is no GEMM output: backward_reference.swiglu_inputs rounded to bf16 (its last row
starts with the gates -100, -30, -1.2784645, 0, 30, 100).  Operand rows carry 8 NaN columns behind K (K fills whole k-tiles, so the
header's half-k-tile rule reads none of them); result buffers carry 8 extra rows and pad columns prefilled with exact_gemm's NaN
patterns; rn buffers reach past the last row TILE (a store without its row guard lands in the sentinel, not outside the buffer).

Bounds (tests/test_gpu_backward_kernels.py's, see score()): linear outputs bit-equal; bf16 non-linear outputs per element within one
bf16 ulp of the bf16-rounded fp64 value -- the ulp taken at the element's scale where its terms cancel -- and different from it on at
most 1e-3 of a case's elements; q / k (tangent) vectors 2^-8 (bf16) or 1e-5 (fp32) relative L2, zero vectors exactly zero; rn 1e-5 per
entry; fp32 SwiGLU per element 8 x the worst error of the torch-fp32 restatement on the same case, relative to the element's scale plus
TINY = 2^-102; SPLIT3 hi + lo within 2^-16 of the fp64 value (relative to it plus TINY: below fp32's normal range the device flushes).
"""
from __future__ import annotations

import math
import zlib
from collections import namedtuple
from dataclasses import dataclass

import torch

import backward_reference as br
import exact_gemm as X

F64, F32 = torch.float64, torch.float32
AT_LN100 = 4.605170185988092   # the kernels' constant
ZERO_ROW = 5
TINY = 2.0 ** -102
BF16_VEC_TOL, F32_TOL, RN_TOL, SHARE_CAP, SPLIT3_TOL = 2.0 ** -8, 1e-5, 1e-5, 1e-3, 2.0 ** -16
PAD_K = 8          # NaN columns behind K in both operands
EXTRA_ROWS = 8
PLANTED = 12       # non-zeros of W's planted rows
ESHAPE = X.ESHAPE
SCALE_BASE = (math.log(10.0), AT_LN100, math.log(200.0), math.log(3.0), math.log(50.0), math.log(30.0))


@dataclass(frozen=True)
class Case:
    epi: str            # swiglu | both | bwd | split3 | qknorm | qknorm_jvp | swiglu_jvp
    name: str
    M: int              # paired-row entries: Mh (A has 2 Mh rows)
    N: int              # as the entry point takes it (qk_only: 2 head_dim per head)
    K: int
    dt: str = "bf16"
    out: str = "bf16"
    hd: int = 0
    form: str = ""      # qknorm: "" | single | qk_only
    rn: bool = True     # qknorm, qknorm_jvp: rn given
    keep: bool = True   # swiglu_jvp: the primal pre-activations kept
    chunk_k: int = 0    # > 0: swiftk_gemm_chunked
    shift: int = 0      # rotation of SCALE_BASE
    key31: bool = False  # run at tuning key 31 = 0, 1, 2, 3
    rc: int = 0
    cell: str = ""

    @property
    def paired(self):
        return self.epi in ("qknorm_jvp", "swiglu_jvp")

    @property
    def rows_a(self):
        return 2 * self.M if self.paired else self.M

    @property
    def heads(self):
        if self.epi not in ("qknorm", "qknorm_jvp"):
            return 0
        return self.N // ((2 if self.form == "qk_only" else 3) * self.hd)

    @property
    def rows_w(self):
        return 3 * self.heads * self.hd if self.form == "qk_only" else self.N

    @property
    def lda(self):
        return self.K + PAD_K

    @property
    def sat_row(self):
        return (self.M - 1) // 4 * 4   # (a row the 2^-(m mod 4) scaling leaves at 1: gates on multiples of 8)

    @property
    def seed(self):
        return zlib.crc32(self.name.encode())

    @property
    def ncols(self):
        """Columns of the main result."""
        return {"swiglu": self.N // 2, "both": self.N, "bwd": 2 * self.N, "split3": self.N // 2, "swiglu_jvp": self.N,
                "qknorm_jvp": self.N}.get(self.epi, self.rows_w)

    @property
    def split3_block(self):
        return self.N // 2 + 32   # pos_rows: block width past the N / 2 live columns

    @property
    def ldc(self):
        if self.epi == "split3":
            return 2 * self.split3_block + self.N // 2 + 8
        return self.ncols + 8

    @property
    def ldc2(self):
        return self.N // 2 + 64

    @property
    def ldh(self):   # bwd: row stride of H
        return 2 * self.N + 8

    @property
    def rn_rows(self):
        return -(-self.M // 256) * 256 + EXTRA_ROWS


# ------------------------------------------------------------------------------------------------ inputs
def scales(c: Case):
    s = [SCALE_BASE[(i + c.shift) % len(SCALE_BASE)] for i in range(c.heads)]
    return torch.tensor(s, dtype=F32)


def head_classes(c: Case):
    s = scales(c)
    at = torch.tensor(AT_LN100, dtype=F32)
    return {"below" if v < at else "at" if v == at else "above" for v in s}


def inputs(c: Case):
    """dict: A [rows_a, lda], W [rows_w, lda] fp32 (NaN behind K), acc = the exact product fp64 [rows_a, columns the GEMM computes],
    scale [heads], H / (bwd) the saved pre-activation as bf16 values."""
    a = X.operand(c.rows_a, c.K, c.lda, "ternary", c.seed)
    w = X.operand(c.rows_w, c.K, c.lda, "ternary", c.seed + 1)
    a[:, :c.K] *= torch.ldexp(torch.ones(c.rows_a), -(torch.arange(c.rows_a) % 4))[:, None]
    a[ZERO_ROW, :c.K] = 0.0
    a[c.sat_row, :c.K] *= 8.0
    # rows 0, 2, 4, 6 of W (gates 0 .. 3; q columns of head 0) follow the signs of the saturating row's first PLANTED non-zeros: that
    # row's gates 0 .. 3 are 8 PLANTED x (+1, -1, -1, +1) = +96, -96, -96, +96 whatever the seed (exp(96) is no finite fp32 number) -- both
    # signs in both (gate, up) pairs a lane's accumulator quad holds
    nz = a[c.sat_row, :c.K].nonzero().flatten()[:PLANTED]
    for r, sign in ((0, 1.0), (2, -1.0), (4, -1.0), (6, 1.0)):
        w[r, :c.K] = 0.0
        w[r, nz] = sign * torch.sign(a[c.sat_row, nz])
    wl = w
    if c.form == "qk_only":   # the v rows of every [q | k | v] triple are skipped
        wl = w.view(c.heads, 3, c.hd, c.lda)[:, :2].reshape(-1, c.lda)
    out = dict(A=a, W=w, acc=X.product(a, wl, 0, c.K))
    if c.heads:
        out["scale"] = scales(c)
    if c.epi == "bwd":
        h, _ = br.swiglu_inputs(c.M, c.N, c.seed % 1000 + 7)
        out["H"] = h.bfloat16().float()
    return out


# ------------------------------------------------------------------------------------------------ closed forms (dtype F64) and
# their fp32 restatements (dtype F32: plain torch fp32 on the CPU, in the kernels' order of operations)
def swiglu_jvp(h, dh, dtype=F64):
    """(out, tangent, scale of the tangent): out = silu(g) u;  d out = (s + g s (1 - s)) dg u + g s du,  s = sigmoid(g)."""
    h, dh = h.to(dtype), dh.to(dtype)
    g, u, dg, du = h[:, 0::2], h[:, 1::2], dh[:, 0::2], dh[:, 1::2]
    s = 1.0 / (1.0 + torch.exp(-g))
    a = g * s
    t1, t2 = (s + a * (1.0 - s)) * dg * u, a * du
    return a * u, t1 + t2, t1.abs() + t2.abs()


def swiglu_f32(h):
    h = h.to(F32)
    g, u = h[:, 0::2], h[:, 1::2]
    return g / (1.0 + torch.exp(-g)) * u


def swiglu_fast_f32(h):
    """The bf16-output form: g * rcp(1 + exp(-g)) * u."""
    h = h.to(F32)
    g, u = h[:, 0::2], h[:, 1::2]
    return g * (1.0 / (1.0 + torch.exp(-g))) * u


def swiglu_bwd_f32(h, d):
    h, d = h.to(F32), d.to(F32)
    g, u = h[:, 0::2], h[:, 1::2]
    s = 1.0 / (1.0 + torch.exp(-g))
    return d * u * (s + g * s * (1.0 - s)), d * g * s


def split3_read(buf, n, block):
    """The [hi | lo | hi] reading of SWIGLU_SPLIT3's output rows: (block 0, block 1, block 2), n live columns each."""
    return buf[:, :n], buf[:, block:block + n], buf[:, 2 * block:2 * block + n]


def qknorm_jvp(raw, draw, scale, heads, hd, dtype=F64):
    """(qkvh, d qkvh, rn, scale of d qkvh): v-hat = tau v / n;  d v-hat = tau / n (dv - v (v . dv) / n^2),  n = max(|v|, 1e-12);  v and
    its tangent pass through.  The scale of a tangent element is |f dv| + |f c v| (f = tau / n, c = (v . dv) / n^2)."""
    M = raw.shape[0]
    v, dv = raw.to(dtype).view(M, heads, 3, hd), draw.to(dtype).view(M, heads, 3, hd)
    eps = torch.tensor(1e-12, dtype=dtype)
    rn = 1.0 / torch.maximum(torch.sqrt((v * v).sum(-1)), eps)
    rn[:, :, 2] = 1.0
    f = rn.clone()
    # (fp64: the true ln 100, as backward_reference.prenorm_fwd; fp32: the kernels' constant, which rounds 6.4e-8 above it)
    tau = torch.exp(torch.clamp(scale.to(dtype), max=br.LN100 if dtype == F64 else float(torch.tensor(AT_LN100, dtype=F32)))).view(1, heads)
    f[:, :, 0] = tau * rn[:, :, 0]
    fc = f * (v * dv).sum(-1) * rn * rn
    fc[:, :, 2] = 0.0
    t1, t2 = f[..., None] * dv, fc[..., None] * v
    return (f[..., None] * v).reshape(M, -1), (t1 - t2).reshape(M, -1), rn.reshape(M, -1), (t1.abs() + t2.abs()).reshape(M, -1)


def qknorm_fwd(raw, scale, heads, hd, dtype=F64):
    """(qkvh, rn): backward_reference.prenorm_fwd in fp64; in fp32 the kernel's order (tau / max(sqrt(sum), 1e-12), then the product)."""
    if dtype == F64:
        return br.prenorm_fwd(raw, scale, heads, hd)
    M = raw.shape[0]
    v = raw.to(F32).view(M, heads, 3, hd)
    n = torch.maximum(torch.sqrt((v * v).sum(-1)), torch.tensor(1e-12, dtype=F32))
    tau = torch.exp(torch.clamp(scale.to(F32), max=torch.tensor(AT_LN100, dtype=F32))).view(1, heads)
    f, rn = 1.0 / n, 1.0 / n
    f[:, :, 0] = tau / n[:, :, 0]
    f[:, :, 2], rn[:, :, 2] = 1.0, 1.0
    return (v * f[..., None]).reshape(M, -1), rn.reshape(M, -1)


def qk_cols(c: Case):
    """qk_only: the columns of C (laid out [q | k | v] per head) that the form writes, in the order the GEMM computes them."""
    h, k, e = torch.meshgrid(torch.arange(c.heads), torch.arange(2), torch.arange(c.hd), indexing="ij")
    return ((3 * h + k) * c.hd + e).reshape(-1)


def qk_view(c: Case, x):
    """[M, heads, kinds, hd] view of a QK-norm result in the columns the GEMM computes (qk_only: kinds = 2)."""
    return x.reshape(x.shape[0], c.heads, 2 if c.form == "qk_only" else 3, c.hd)


def qk_forms(c: Case, inp, dtype):
    """(out, rn) over the columns the GEMM computes."""
    acc, kinds = inp["acc"], 2 if c.form == "qk_only" else 3
    M = acc.shape[0]
    raw = acc
    if kinds == 2:   # place the pairs into triples with a dummy v
        raw = torch.ones(M, c.heads, 3, c.hd, dtype=F64)
        raw[:, :, :2] = acc.view(M, c.heads, 2, c.hd)
        raw = raw.reshape(M, -1)
    out, rn = qknorm_fwd(raw, inp["scale"], c.heads, c.hd, dtype)
    if kinds == 2:
        out = out.view(M, c.heads, 3, c.hd)[:, :, :2].reshape(M, -1)
        rn = rn.view(M, c.heads, 3)[:, :, :2].reshape(M, -1)
    return out, rn


# ------------------------------------------------------------------------------------------------ buffers
def sent(shape, out):
    return torch.full(shape, X.SENT_F32 if out == "f32" else X.SENT_BF16, dtype=torch.int32 if out == "f32" else torch.int16)


def values(bits):
    return (bits.view(torch.float32) if bits.dtype == torch.int32 else bits.view(torch.bfloat16)).double()


def to_bits(x, out):
    x = x.float()
    return x.contiguous().view(torch.int32) if out == "f32" else x.bfloat16().contiguous().view(torch.int16)


def prefill(c: Case):
    """The result buffers of a case as raw bits, sentinel everywhere: C, C2, rn (None where the case has none)."""
    rows = c.rows_a + EXTRA_ROWS
    b = dict(C=sent((rows, c.ldc), c.out), C2=None, rn=None)
    if c.epi == "qknorm" and c.form == "qk_only":
        b["C"] = sent((rows, 3 * c.heads * c.hd + 8), c.out)
    if c.epi == "both":
        b["C2"] = sent((rows, c.ldc2), "bf16")
    if c.epi == "swiglu_jvp":
        b["C"] = sent((c.M + EXTRA_ROWS, c.ldc), "bf16") if c.keep else None
        b["C2"] = sent((rows, c.ldc2), "bf16")
    if c.epi in ("qknorm", "qknorm_jvp") and c.rn:
        b["rn"] = sent((c.rn_rows, c.N // c.hd), "f32")
    return b


def restate(c: Case, inp):
    """What the entry point leaves in prefill(c)'s buffers if it computes the fp32 restatement of its epilogue on the exact
    accumulators and rounds where the kernel rounds."""
    b = prefill(c)
    if c.rc:
        return b
    acc, M, out = inp["acc"].float(), c.M, c.out
    if c.epi == "swiglu":
        b["C"][:M, :c.ncols] = to_bits(swiglu_f32(acc) if out == "f32" else swiglu_fast_f32(acc), out)
    elif c.epi == "both":
        b["C"][:M, :c.N] = to_bits(acc, "bf16")
        b["C2"][:M, :c.N // 2] = to_bits(swiglu_fast_f32(acc), "bf16")
    elif c.epi == "bwd":
        dg, du = swiglu_bwd_f32(inp["H"], acc)
        b["C"][:M, 0:2 * c.N:2], b["C"][:M, 1:2 * c.N:2] = to_bits(dg, "bf16"), to_bits(du, "bf16")
    elif c.epi == "split3":
        h = swiglu_f32(acc)
        hi = h.bfloat16()
        lo = (h - hi.float()).bfloat16()
        n, P = c.N // 2, c.split3_block
        for k, v in enumerate((hi, lo, hi)):
            b["C"][:M, k * P:k * P + n] = v.view(torch.int16)
    elif c.epi == "qknorm":
        o, rn = qk_forms(c, inp, F32)
        if c.form == "qk_only":
            b["C"][:M, qk_cols(c)] = to_bits(o, out)
        else:
            b["C"][:M, :c.N] = to_bits(o, out)
        if c.rn:
            b["rn"][:M] = to_bits(rn, "f32")
    elif c.epi == "qknorm_jvp":
        o, do, rn, _ = qknorm_jvp(acc[:M], acc[M:], inp["scale"], c.heads, c.hd, F32)
        b["C"][:M, :c.N], b["C"][M:2 * M, :c.N] = to_bits(o, "bf16"), to_bits(do, "bf16")
        if c.rn:
            b["rn"][:M] = to_bits(rn, "f32")
    elif c.epi == "swiglu_jvp":
        o, do, _ = swiglu_jvp(acc[:M], acc[M:], F32)
        if c.keep:
            b["C"][:M, :c.N] = to_bits(acc[:M], "bf16")
        b["C2"][:M, :c.N // 2], b["C2"][M:2 * M, :c.N // 2] = to_bits(o, "bf16"), to_bits(do, "bf16")
    return b


# ------------------------------------------------------------------------------------------------ scoring
class Report:
    def __init__(self, c):
        self.c, self.lines, self.failed = c, [], []

    def add(self, what, figure, bound, where="", ok=None):
        ok = figure <= bound if ok is None else ok
        self.lines.append(f"{self.c.epi} {self.c.name} {what}: {figure:.3g} [bound {bound:.3g}]{' at ' + where if where else ''}{'' if ok else '  <-- FAILS'}")
        if not ok:
            self.failed.append(self.lines[-1])

    def text(self):
        return "\n".join(self.lines)


def _where(c, idx, shape, cols_kind="col"):
    pos = [int(v) for v in torch.unravel_index(torch.as_tensor(idx), shape)]
    r, col = pos[0], pos[-1] if len(pos) == 2 else None
    if len(pos) == 2:
        if c.heads and c.hd:
            kinds = 2 if c.form == "qk_only" else 3
            v = col // c.hd
            return f"row {r}, head {v // kinds}, kind {'qkv'[v % kinds]}, column {col}"
        return f"row {r}, column {col}"
    return f"row {r}, head {pos[1]}, kind {'qkv'[pos[2]]}"


def _untouched(rep, name, got, want_prefill, live):
    """Every word outside `live` (a bool mask) is the prefill."""
    bad = (got != want_prefill) & ~live
    n = int(bad.sum())
    where = ""
    if n:
        r, col = [int(v) for v in bad.nonzero()[0]]
        where = f"(row {r}, column {col})"
    rep.add(f"{name}: words changed outside the written region", n, 0, where)


def _finite(rep, name, vals):
    n = int((~torch.isfinite(vals)).sum())
    where = _where(rep.c, int((~torch.isfinite(vals)).flatten().nonzero()[0]), vals.shape) if n else ""
    rep.add(f"{name}: non-finite results", n, 0, where)


def _bits_equal(rep, name, got_bits, ref64, out):
    want = to_bits(ref64, out)
    bad = got_bits != want
    n = int(bad.sum())
    where = _where(rep.c, int(bad.flatten().nonzero()[0]), bad.shape) if n else ""
    rep.add(f"{name}: elements not bit-equal to the exact value", n, 0, where)


def _bf16_elements(rep, name, got, ref64, scale64=None):
    want = ref64.float().bfloat16().double()
    # (the ulp is taken no lower than at TINY, the floor the fp32 rule has for the same reason: sigmoid(g) < 2^-126 is no normal fp32
    # number -- exp(-g) overflows from g = -88.8 and the reciprocal is subnormal from -87.4 --, so |g u| 2^-126 <= 2^-112 of absolute error
    # is what fp32 arithmetic itself leaves at the +-100 gates; literal ulps of a result in bf16's subnormal range would ask fp32 for more)
    at = want.abs().clamp_min(TINY) if scale64 is None else torch.maximum(want.abs(), scale64.float().bfloat16().double()).clamp_min(TINY)
    err = (got - want).abs() / br.bf16_ulp(at)
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    rep.add(f"{name}: worst element, bf16 ulp from the rounded fp64 value", float(err.max()), 1.0, _where(rep.c, int(err.argmax()), err.shape))
    rep.add(f"{name}: share of elements that differ from it", float((got != want).double().mean()), SHARE_CAP)


def _f32_elements(rep, name, got, yard, ref64, scale64):
    s = scale64 + TINY
    ek, ey = (got - ref64).abs() / s, (yard.double() - ref64).abs() / s
    ek = torch.where(torch.isfinite(ek), ek, torch.full_like(ek, float("inf")))
    rep.add(f"{name}: worst element error of its scale (8 x torch fp32's {float(ey.max()):.3g})", float(ek.max()), 8 * float(ey.max()),
            _where(rep.c, int(ek.argmax()), ek.shape))


def _vectors(rep, name, got4, ref4, tol):
    """q | k vectors [M, heads, kinds, hd] (kinds 0, 1): relative L2 per vector, zero vectors exactly zero."""
    e = br.row_rel_l2(got4[:, :, :2], ref4[:, :, :2])
    e = torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)
    rep.add(f"{name}: worst q / k vector, relative L2", float(e.max()), tol, _where(rep.c, int(e.argmax()), e.shape))


def score(c: Case, inp, b) -> Report:
    """Every bound of the module docstring on the buffers `b` (as prefill(c) lays them out) an entry point left."""
    rep = Report(c)
    p = prefill(c)
    if c.rc:   # refused: nothing written anywhere
        for k, v in b.items():
            if v is not None:
                rep.add(f"{k}: words changed by a refused call", int((v != p[k]).sum()), 0)
        return rep
    acc, M, bf = inp["acc"], c.M, c.out == "bf16"
    C = b["C"]
    live = lambda buf, rows, cols: _mask(buf, rows, cols)
    if c.epi in ("swiglu", "both", "split3", "swiglu_jvp"):
        prim = acc[:M]
        ref = br.swiglu_fwd(prim)
    if c.epi == "swiglu":
        _untouched(rep, "C", C, p["C"], live(C, M, c.ncols))
        got = values(C[:M, :c.ncols])
        _finite(rep, "C", got)
        if bf:
            _bf16_elements(rep, "silu(g) u", got, ref)
        else:
            _f32_elements(rep, "silu(g) u", got, swiglu_f32(acc), ref, ref.abs())
    elif c.epi == "both":
        _untouched(rep, "C", C, p["C"], live(C, M, c.N))
        _untouched(rep, "C2", b["C2"], p["C2"], live(b["C2"], M, c.N // 2))
        _bits_equal(rep, "pre-activation", C[:M, :c.N], acc, "bf16")
        got = values(b["C2"][:M, :c.N // 2])
        _finite(rep, "C2", got)
        _bf16_elements(rep, "silu(g) u", got, ref)
    elif c.epi == "bwd":
        _untouched(rep, "C", C, p["C"], live(C, M, 2 * c.N))
        got = values(C[:M, :2 * c.N])
        _finite(rep, "C", got)
        dg, du, sg, su = br.swiglu_bwd(inp["H"], acc)
        _bf16_elements(rep, "dgate", got[:, 0::2], dg, sg)
        _bf16_elements(rep, "dup", got[:, 1::2], du, su)
    elif c.epi == "split3":
        n, P = c.N // 2, c.split3_block
        m = live(C, M, n)
        m[:M, P:P + n] = True
        m[:M, 2 * P:2 * P + n] = True
        _untouched(rep, "C (the blocks' pad columns included)", C, p["C"], m)
        b0, b1, b2 = split3_read(C[:M], n, P)
        rep.add("block 2: elements not bit-equal to block 0", int((b0 != b2).sum()), 0)
        hi, lo = values(b0), values(b1)
        _finite(rep, "hi", hi)
        _finite(rep, "lo", lo)
        _bf16_elements(rep, "hi", hi, ref)
        e = (hi + lo - ref).abs() / (ref.abs() + TINY)
        e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
        rep.add("hi + lo: worst element, relative to the fp64 value", float(e.max()), SPLIT3_TOL, _where(c, int(e.argmax()), e.shape))
    elif c.epi == "qknorm":
        ref, rn = qk_forms(c, inp, F64)
        kinds = 2 if c.form == "qk_only" else 3
        if kinds == 2:
            m = torch.zeros_like(C, dtype=torch.bool)
            m[:M, qk_cols(c)] = True
            _untouched(rep, "C (the v columns included)", C, p["C"], m)
            got = values(C[:M][:, qk_cols(c)].contiguous())
        else:
            _untouched(rep, "C", C, p["C"], live(C, M, c.N))
            got = values(C[:M, :c.N])
            _bits_equal(rep, "v columns", qk_view(c, C[:M, :c.N])[:, :, 2], qk_view(c, acc)[:, :, 2], c.out)
        _finite(rep, "C", got)
        if bf:
            _bf16_elements(rep, "q-hat | k-hat | v", got, ref)
        _vectors(rep, "q-hat | k-hat", qk_view(c, got), qk_view(c, ref), BF16_VEC_TOL if bf else F32_TOL)
        if c.rn:
            _score_rn(rep, c, b["rn"], p["rn"], rn, kinds)
    elif c.epi == "qknorm_jvp":
        ref, dref, rn, sc = qknorm_jvp(acc[:M], acc[M:], inp["scale"], c.heads, c.hd)
        _untouched(rep, "C", C, p["C"], live(C, 2 * M, c.N))
        got, dgot = values(C[:M, :c.N]), values(C[M:2 * M, :c.N])
        _finite(rep, "C", values(C[:2 * M, :c.N]))
        _bits_equal(rep, "v columns", qk_view(c, C[:M, :c.N])[:, :, 2], qk_view(c, acc[:M])[:, :, 2], "bf16")
        _bits_equal(rep, "tangent v columns", qk_view(c, C[M:2 * M, :c.N])[:, :, 2], qk_view(c, acc[M:])[:, :, 2], "bf16")
        _bf16_elements(rep, "q-hat | k-hat | v", got, ref)
        _bf16_elements(rep, "tangent", dgot, dref, sc)
        _vectors(rep, "q-hat | k-hat", qk_view(c, got), qk_view(c, ref), BF16_VEC_TOL)
        _vectors(rep, "tangent of q-hat | k-hat", qk_view(c, dgot), qk_view(c, dref), BF16_VEC_TOL)
        if c.rn:
            _score_rn(rep, c, b["rn"], p["rn"], rn, 3)
    elif c.epi == "swiglu_jvp":
        o, do, sc = swiglu_jvp(acc[:M], acc[M:])
        C2 = b["C2"]
        _untouched(rep, "C2 (hm, its k-padding included)", C2, p["C2"], live(C2, 2 * M, c.N // 2))
        if c.keep:
            _untouched(rep, "C", C, p["C"], live(C, M, c.N))
            _bits_equal(rep, "kept pre-activation", C[:M, :c.N], acc[:M], "bf16")
        got, dgot = values(C2[:M, :c.N // 2]), values(C2[M:2 * M, :c.N // 2])
        _finite(rep, "C2", values(C2[:2 * M, :c.N // 2]))
        _bf16_elements(rep, "silu(g) u", got, o)
        _bf16_elements(rep, "tangent", dgot, do, sc)
    return rep


def _mask(buf, rows, cols):
    m = torch.zeros_like(buf, dtype=torch.bool)
    m[:rows, :cols] = True
    return m


def _score_rn(rep, c, got_bits, pre, rn64, kinds):
    M = c.M
    _untouched(rep, "rn", got_bits, pre, _mask(got_bits, M, c.N // c.hd))
    got = values(got_bits[:M]).view(M, c.heads, kinds)
    ref = rn64.view(M, c.heads, kinds)
    _finite(rep, "rn", got)
    e = ((got - ref).abs() / ref.abs())
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
    rep.add("rn: worst entry, relative", float(e.max()), RN_TOL, f"row {int(e.argmax()) // (c.heads * kinds)}, vector {int(e.argmax()) % (c.heads * kinds)}")
    if kinds == 3:
        rep.add("rn of v: entries that are not exactly 1", int((got[:, :, 2] != 1.0).sum()), 0)
    rep.add("rn of the zero row: worst |rn / 1e12 - 1|", float((got[ZERO_ROW, :, :2] / 1e12 - 1).abs().max()), RN_TOL)


# ------------------------------------------------------------------------------------------------ the dispatch, restated
Cell = namedtuple("Cell", "epi dt out kernel width kloop rounds hd form rn keep rc")


def expected_cell(c: Case, grid=X.GRID) -> Cell:
    """Which kernel a row runs and what a refused row returns.  Restates swift_amd/csrc/gemm.hip: gemm_impl (QKNORM: tile width
    4 head_dim, fp32 operands at head_dim 80 / 96 need M, N % 8 == 0; otherwise the width out of 384 / 320 that divides N where 352 does
    not, bf16 operands only), launch() (the one-tile kernel when M % 8, N % 8 or a bf16 store that cannot move 16-B row chunks: it has no
    SWIGLU_BOTH / SWIGLU_BWD and runs QKNORM at 352-wide tiles only), dispatch_epi (SPLIT3: persistent kernel only), pp_ok (ping-pong
    from three k-tiles, bf16 operands) and swiftk_gemm_jvp (128 primal + 128 tangent rows per tile)."""
    cdiv = lambda a, b: -(-a // b)
    tile_k = 64 if c.dt == "bf16" else 32
    if c.hd:
        ni = c.hd // 8
    elif c.dt == "bf16" and c.N % 352:
        ni = 12 if c.N % 384 == 0 else 10 if c.N % 320 == 0 else 11
    else:
        ni = 11
    one_tile = False
    if not c.paired:
        glu_n = 16 if c.epi in ("swiglu", "both") else 8
        wide_ok = c.out != "bf16" or (c.ldc % 8 == 0 and c.N % glu_n == 0)
        one_tile = bool(c.M % 8 or c.N % 8 or not wide_ok)
    rc = 0
    if one_tile and (c.epi in ("both", "bwd", "split3") or (c.epi == "qknorm" and ni != 11)):
        rc = ESHAPE
    kloop = "pp" if c.dt == "bf16" and c.K // tile_k >= 3 else "one_barrier"
    if c.chunk_k:
        kloop += "+chunked"
    if one_tile:
        return Cell(c.epi, c.dt, c.out, "one_tile", 352, "two_stage", "tile_per_wg", c.hd, c.form, c.rn, c.keep, rc)
    tiles = cdiv(c.rows_a, 256) * cdiv(c.N, 32 * ni)
    return Cell(c.epi, c.dt, c.out, "persistent", 32 * ni, kloop, X.rounds_of(tiles, grid), c.hd, c.form, c.rn, c.keep, rc)


# ------------------------------------------------------------------------------------------------ the case table
CASES: list = []
TYPES = X.TYPES
WIDTHS = {320: 1280, 352: 1408, 384: 1536}   # N = 2 tile columns of each width for the SwiGLU family
QK_N = {80: 960, 88: 1056, 96: 1152}         # 4 heads x 3 x head_dim: three tile columns
KB = {"one_barrier": 128, "pp": 192}         # bf16 operands: two k-tiles, three k-tiles
M_P, M_1, M_BIG = 264, 261, 256 * 90


def _add(epi, name, M, N, K, types="bb", **kw):
    dt, out = TYPES[types]
    CASES.append(Case(epi, f"{name}-{types}", M, N, K, dt, out, **kw))


# ---- SWIFTK_EPI_SWIGLU
for t_ in ("bb", "bf", "ff"):
    _add("swiglu", "one_tile", M_1, 1408, 96 if t_ == "ff" else 192, t_, cell="one-tile kernel, M % 8 != 0, ragged last row tile")
for w_, n_ in WIDTHS.items():
    for kl_, k_ in KB.items():
        _add("swiglu", f"p{w_}_{kl_}", M_P, n_, k_, "bb", key31=(w_ == 352 and kl_ == "pp"),
             cell=f"persistent {w_}, {kl_}" + (", tuning key 31 = 0 .. 3" if w_ == 352 and kl_ == "pp" else ""))
_add("swiglu", "p352_f32_operands", M_P, 1408, 96, "ff", cell="fp32 operands and output, 352 wide")
_add("swiglu", "p352_f32_out", M_P, 1408, 192, "bf", cell="bf16 operands, fp32 output (scattered store2)")
_add("swiglu", "chunked", M_P, 1408, 96, "ff", chunk_k=32, cell="swiftk_gemm_chunked: SwiGLU behind merged accumulators")
_add("swiglu", "rounds", M_BIG, 1056, 192, "bb", cell="270 tiles on 256 workgroups: a second epilogue behind a prefetched tile")
# ---- SWIGLU_BOTH, SWIGLU_BWD, SWIGLU_SPLIT3
for epi_ in ("both", "bwd", "split3"):
    for w_, n_ in WIDTHS.items():
        for kl_, k_ in KB.items():
            _add(epi_, f"p{w_}_{kl_}", M_P, n_, k_, "bb", cell=f"persistent {w_}, {kl_}")
    _add(epi_, "rounds", M_BIG, 1056, 192, "bb", cell="270 tiles on 256 workgroups")
    _add(epi_, "ragged_M_refused", M_1, 1408, 192, "bb", rc=ESHAPE, cell="M % 8 != 0: no one-tile form, SWIFTK_ESHAPE, nothing written")
# ---- SWIFTK_EPI_QKNORM
_add("qknorm", "one_tile_hd88", M_1, QK_N[88], 192, "bb", hd=88, cell="one-tile kernel, head_dim 88, rn's row guard on a ragged tile")
_add("qknorm", "one_tile_hd88", M_1, QK_N[88], 96, "ff", hd=88, cell="one-tile kernel, fp32")
_add("qknorm", "one_tile_hd88_no_rn", M_1, QK_N[88], 192, "bf", hd=88, rn=False, cell="one-tile kernel, rn = NULL, fp32 out")
for hd_ in (80, 96):
    _add("qknorm", f"one_tile_hd{hd_}_refused", M_1, QK_N[hd_], 192, "bb", hd=hd_, rc=ESHAPE, cell="one-tile kernel has 352-wide tiles only")
    _add("qknorm", f"one_tile_hd{hd_}_refused", M_1, QK_N[hd_], 96, "ff", hd=hd_, rc=ESHAPE, cell="fp32 operands: whole tiles only")
for hd_ in (80, 88, 96):
    for kl_, k_ in KB.items():
        _add("qknorm", f"p_hd{hd_}_{kl_}", M_P, QK_N[hd_], k_, "bb", hd=hd_, rn=(kl_ == "pp" or hd_ == 88), cell=f"persistent, head_dim {hd_}, {kl_}")
    for k_ in (64, 96):
        _add("qknorm", f"p_hd{hd_}_K{k_}", M_P, QK_N[hd_], k_, "ff", hd=hd_, rn=(k_ == 96), cell=f"persistent, fp32 operands, head_dim {hd_}")
    _add("qknorm", f"single_hd{hd_}", M_P, 3 * hd_, 96, "ff", hd=hd_, form="single", shift=(hd_ - 80) // 8,
         cell="one head: the tile's fourth vector is empty")
_add("qknorm", "p_hd88_f32_out", M_P, QK_N[88], 192, "bf", hd=88, cell="bf16 operands, fp32 output")
for pairs_, hd_ in ((1, 88), (2, 96), (3, 80)):
    _add("qknorm", f"qk_only_{pairs_}_pairs_hd{hd_}", M_P, 2 * pairs_ * 2 * hd_, 96, "ff", hd=hd_, form="qk_only", rn=False, shift=pairs_ % 2,
         cell=f"[q | k]-only form, {pairs_} head pair(s): the v columns of C untouched")
_add("qknorm", "rounds_hd80", M_BIG, QK_N[80], 192, "bb", hd=80, cell="270 tiles on 256 workgroups")
# ---- swiftk_gemm_jvp
for hd_ in (80, 88, 96):
    for kl_, k_ in KB.items():
        _add("qknorm_jvp", f"hd{hd_}_{kl_}", 128 if kl_ == "pp" else 256, QK_N[hd_], k_, "bb", hd=hd_, rn=((kl_ == "one_barrier") != (hd_ == 88)),
             cell=f"paired rows, head_dim {hd_}, {kl_}")
_add("qknorm_jvp", "rounds_hd88", 128 * 90, QK_N[88], 192, "bb", hd=88, cell="270 paired tiles on 256 workgroups")
for w_, n_ in WIDTHS.items():
    for kl_, k_ in KB.items():
        _add("swiglu_jvp", f"p{w_}_{kl_}", 256 if kl_ == "pp" else 128, n_, k_, "bb", keep=(kl_ == "pp" or w_ == 352),
             cell=f"paired rows, {w_} wide, {kl_}")
_add("swiglu_jvp", "rounds", 128 * 90, 1056, 192, "bb", cell="270 paired tiles on 256 workgroups")

assert len({(c.epi, c.name) for c in CASES}) == len(CASES)


def cases(*epis):
    return [c for c in CASES if c.epi in epis]


def ids(cs):
    return [c.name for c in cs]


def _req():
    """Partial cells the table must meet (tests/test_epilogue_reference_cpu.py)."""
    R = []
    for dt, out in TYPES.values():
        R.append(dict(epi="swiglu", dt=dt, out=out, kernel="one_tile", rc=0))
    for w in (320, 352, 384):
        for kl in ("one_barrier", "pp"):
            for epi in ("swiglu", "both", "bwd", "split3", "swiglu_jvp"):
                R.append(dict(epi=epi, dt="bf16", out="bf16", kernel="persistent", width=w, kloop=kl, rc=0))
    for keep in (True, False):
        R.append(dict(epi="swiglu_jvp", keep=keep))
    R.append(dict(epi="swiglu", dt="f32", kernel="persistent", width=352, kloop="one_barrier"))
    R.append(dict(epi="swiglu", dt="f32", kloop="one_barrier+chunked"))
    for epi in ("both", "bwd"):
        R.append(dict(epi=epi, kernel="one_tile", rc=ESHAPE))
    R.append(dict(epi="qknorm", kernel="one_tile", hd=88, rc=0, rn=True))
    for hd in (80, 96):
        R.append(dict(epi="qknorm", kernel="one_tile", hd=hd, rc=ESHAPE))
    for hd in (80, 88, 96):
        for kl in ("one_barrier", "pp"):
            R.append(dict(epi="qknorm", dt="bf16", out="bf16", kernel="persistent", hd=hd, width=4 * hd, kloop=kl))
            R.append(dict(epi="qknorm_jvp", kernel="persistent", hd=hd, width=4 * hd, kloop=kl))
        R.append(dict(epi="qknorm", dt="f32", kernel="persistent", hd=hd, width=4 * hd, form=""))
        for rn in (True, False):
            R.append(dict(epi="qknorm", kernel="persistent", hd=hd, rn=rn, form=""))
            R.append(dict(epi="qknorm_jvp", hd=hd, rn=rn))
    R.append(dict(epi="qknorm", form="single", dt="f32"))
    R.append(dict(epi="qknorm", form="qk_only", dt="f32"))
    for epi in ("swiglu", "both", "bwd", "split3", "qknorm", "qknorm_jvp", "swiglu_jvp"):
        R.append(dict(epi=epi, kernel="persistent", rounds="last_other", rc=0))   # more tiles than workgroups
    return R


REQUIRED = _req()
