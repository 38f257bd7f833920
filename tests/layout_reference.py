"""Index-formula and fp64 references for the layout kernels that sit between the matrix products (no GPU in this module).

Written from include/swiftk.h: patchify / un-patchify, the timestep embedding, the small-batch linear, the rollout update, axpby,
the fp32 -> bf16 conversions, the three column-sum gathers of the backward pass and the persistent GEMM's incremental tile walk.

Placement references are explicit index arithmetic on torch tensors (tests/test_layout_reference_cpu.py pins them to
oracle.swinv2).  Inputs come in four families:
  tagged    fp32, element value = 1 + flat index + per-source offset, all below 2^24: exact in fp32 and unique, so a wrong output
            element names the source element it was read from (decode_tag)
  normal    seeded N(0, 1), for the bf16 outputs
  edges     CONVERSION_TABLE: fp32 bit patterns with the bf16 bits round-to-nearest-even gives
  integer   integers in [-8, 8] times a power of two: every product and partial sum is exact below 2^24, one bit pattern expected
Error bounds are functions of the operands, u = 2^-24; every fp64 reference starts from the fp32 values the kernel receives.
"""
from __future__ import annotations

import math
from collections import namedtuple

import torch

U = 2.0 ** -24
SENT_F32 = 0x7FC12345   # quiet NaNs with a payload nothing computes
SENT_BF16 = 0x7FC1
CAP = 4096 * 256        # elementwise.hip, grid_for: the most work items one pass of a grid-stride kernel covers
EINVAL, ESHAPE, EALIGN = -1, -2, -3


# ------------------------------------------------------------------------------------------------------------ input makers
def tagged(shape, offset=0):
    """fp32 tensor whose element at flat index i holds 1 + i + offset."""
    n = math.prod(shape)
    assert 1 + n + offset < 2 ** 24
    return (torch.arange(n, dtype=torch.float64) + (1 + offset)).float().reshape(shape)


def decode_tag(value, shapes, offsets, scales=None):
    """The (source, coordinate) a tagged value came from, for every source that could have produced it ([] = none)."""
    hits = []
    for s, (shape, off) in enumerate(zip(shapes, offsets)):
        if shape is None:
            continue
        v = float(value) / (float(scales[s]) if scales else 1.0) - 1 - off
        if v == int(v) and 0 <= v < math.prod(shape):
            hits.append((s, tuple(int(c) for c in torch.unravel_index(torch.tensor(int(v)), shape))))
    return hits


def normal(shape, seed, std=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * std


def integers(shape, seed, pow2=0, lo=-8, hi=8):
    """Integers uniform in [lo, hi] times 2^pow2, fp32."""
    v = torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()
    return v * (2.0 ** pow2)


def f32_from_bits(bits):
    return torch.tensor([b - (1 << 32) if b >= 1 << 31 else b for b in bits], dtype=torch.int32).view(torch.float32)


def bf16_bits(x):
    """The 16 raw bits of a bf16 tensor as non-negative ints."""
    return x.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def f32_bits(x):
    return x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def rne_bf16_bits(x):
    """Round-to-nearest-even of fp32 (or fp64 holding fp32-representable values) to bf16, by integer arithmetic on the bits."""
    b = f32_bits(x.float())
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF
    nan = ((b & 0x7F800000) == 0x7F800000) & ((b & 0x007FFFFF) != 0)
    return torch.where(nan, (b >> 16) | 0x40, r).to(torch.int32)


Edge = namedtuple("Edge", "name f32 bf16")
CONVERSION_TABLE = [
    Edge("tie, even below: 1 + 2^-8 -> 1", 0x3F808000, 0x3F80),
    Edge("tie, even above: 1 + 3 2^-8 -> 1 + 2^-6", 0x3F818000, 0x3F82),
    Edge("one ulp above a tie", 0x3F808001, 0x3F81),
    Edge("one ulp below a tie", 0x3F807FFF, 0x3F80),
    Edge("negative tie, even above", 0xBF818000, 0xBF82),
    Edge("rounds up into the next binade: 2 - 2^-23 -> 2", 0x3FFFFFFF, 0x4000),
    Edge("tie that carries into the next binade", 0x3FFF8000, 0x4000),
    Edge("-0.0", 0x80000000, 0x8000),
    Edge("+0.0", 0x00000000, 0x0000),
    Edge("smallest fp32 subnormal -> 0", 0x00000001, 0x0000),
    Edge("subnormal tie, even below -> 0", 0x00008000, 0x0000),
    Edge("subnormal tie, even above", 0x00018000, 0x0002),
    Edge("negative subnormal tie, even above", 0x80018000, 0x8002),
    Edge("largest fp32 subnormal -> smallest normal", 0x007FFFFF, 0x0080),
    Edge("largest fp32 below the bf16 overflow point", 0x7F7F7FFF, 0x7F7F),
    Edge("the overflow point (a tie whose even neighbour is inf)", 0x7F7F8000, 0x7F80),
    Edge("FLT_MAX -> inf", 0x7F7FFFFF, 0x7F80),
    Edge("negative overflow", 0xFF7F8000, 0xFF80),
    Edge("one", 0x3F800000, 0x3F80),
]


def edge_values(n):
    """n fp32 values cycling through CONVERSION_TABLE, and the bf16 bits each must become."""
    k = len(CONVERSION_TABLE)
    f = f32_from_bits([CONVERSION_TABLE[i % k].f32 for i in range(n)])
    want = torch.tensor([CONVERSION_TABLE[i % k].bf16 for i in range(n)], dtype=torch.int32)
    return f, want


# ------------------------------------------------------------------------------------------------------------ patchify
def patchify_ref(srcs, scales, patch, lda, per_sample=None):
    """include/swiftk.h, swiftk_patchify(_scaled): A[b gh gw + gy gw + gx][(i1 p2 + i2) C + c] = scale_s src_s[b][c - c0_s][gy p1 + i1]
    [gx p2 + i2] (source 0 also times per_sample[b]); columns [F, lda) zero.  srcs: up to three [B, c_s, H, W] fp32 or None.
    Returns fp64 [B gh gw, lda] (products of the fp32 values, exact for power-of-two scales)."""
    p1, p2 = patch
    first = next(s for s in srcs if s is not None)
    B, _, H, W = first.shape
    gh, gw = H // p1, W // p2
    C = sum(s.shape[1] for s in srcs if s is not None)
    F = p1 * p2 * C
    out = torch.zeros(B, gh * gw, lda, dtype=torch.float64)
    tok = torch.arange(gh * gw)
    gy, gx = tok // gw, tok % gw
    f = torch.arange(F)
    c, pp = f % C, f // C
    i1, i2 = pp // p2, pp % p2
    yy = gy[:, None] * p1 + i1[None, :]            # [T, F]
    xx = gx[:, None] * p2 + i2[None, :]
    c0 = 0
    for s, src in enumerate(srcs):
        if src is None:
            continue
        cn = src.shape[1]
        mine = (c >= c0) & (c < c0 + cn)
        cols = f[mine]
        v = src.double()[:, (c[mine] - c0)[None, :], yy[:, mine], xx[:, mine]]     # [B, T, F_s]
        v = v * float(torch.tensor(scales[s], dtype=torch.float32))
        if s == 0 and per_sample is not None:
            v = v * per_sample.double().view(B, 1, 1)
        out[:, :, cols] = v
        c0 += cn
    return out.reshape(B * gh * gw, lda)


def patchify_source_of(row, col, chans, B, H, W, patch):
    """(source, b, channel in source, y, x) that output element (row, col) must read (None for a pad column)."""
    p1, p2 = patch
    gh, gw = H // p1, W // p2
    C = sum(chans)
    if col >= p1 * p2 * C:
        return None
    b, t = divmod(row, gh * gw)
    gy, gx = divmod(t, gw)
    pp, c = divmod(col, C)
    i1, i2 = divmod(pp, p2)
    s = 0
    while c >= chans[s]:
        c -= chans[s]
        s += 1
    return s, b, c, gy * p1 + i1, gx * p2 + i2


def patchify_path(chans, B, H, W, patch, lda, a_align=0, src_align=(0, 0, 0)):
    """elementwise.hip, swiftk_patchify_scaled: 'tiled' or 'element'.  *_align: byte address modulo 16 of the output / sources."""
    p1, p2 = patch
    C = sum(chans)
    gw = W // p2
    rs = 16 * p2 + 4
    tile_bytes = C * p1 * rs * 4
    aligned = gw % 16 == 0 and (16 * p2) % 4 == 0 and W % 4 == 0 and lda % 8 == 0 and a_align == 0 and tile_bytes <= 64 * 1024
    for s in range(3):  # (an absent source stands in as source 0)
        aligned = aligned and (src_align[s] if chans[s] else src_align[0]) == 0
    return "tiled" if aligned else "element"


# ------------------------------------------------------------------------------------------------------------ un-patchify
def unpatchify_gather(tok, C, H, W, patch):
    """f[b][c][y][x] = tok[b][gy gw + gx][(c p1 + i1) p2 + i2], gy = y / p1, i1 = y % p1, gx = x / p2, i2 = x % p2 (same dtype)."""
    p1, p2 = patch
    gw = W // p2
    y, x, c = torch.arange(H), torch.arange(W), torch.arange(C)
    t = (y // p1)[:, None] * gw + (x // p2)[None, :]                                         # [H, W]
    f = (c[:, None, None] * p1 + (y % p1)[None, :, None]) * p2 + (x % p2)[None, None, :]     # [C, H, W]
    return tok[:, t[None, :, :], f]                                                          # [B, C, H, W]


def unpatchify_ref(tok, C, H, W, patch, xt=None, alpha=None, beta=None):
    """out = alpha[b] xt + beta[b] f (alpha == NULL: 0, beta == NULL: 1; xt == NULL: alpha ignored) in fp64, and the bound:
    with xt 2u (|a x| + |b f|) (two products and a sum, fused or not); beta only u |b f| (one rounding); neither 0 (bit equal)."""
    B = tok.shape[0]
    f = unpatchify_gather(tok, C, H, W, patch).double()
    b = beta.double().view(B, 1, 1, 1) if beta is not None else 1.0
    bf = b * f
    if xt is None:
        return bf, (U * bf.abs() if beta is not None else torch.zeros_like(bf))
    a = alpha.double().view(B, 1, 1, 1) if alpha is not None else 0.0
    ax = a * xt.double()
    return ax + bf, 2 * U * (ax.abs() + bf.abs())


def unpatchify_source_of(b, c, y, x, W, patch):
    """(b, token, feature) of tok that output element (b, c, y, x) must read."""
    p1, p2 = patch
    return b, (y // p1) * (W // p2) + x // p2, (c * p1 + y % p1) * p2 + x % p2


def unpatchify_path(H, W, patch, ldt, tok_align=0, out_align=0, xt_align=0):
    """elementwise.hip, swiftk_unpatchify_affine: 'fast4' (unpatchify4_kernel) or 'generic'.  tok_align: address modulo 8; out_align,
    xt_align: modulo 16 (0 for an absent xt)."""
    fast = patch == (2, 2) and W % 4 == 0 and ldt % 2 == 0 and tok_align == 0 and out_align == 0 and xt_align == 0
    return "fast4" if fast else "generic"


# ------------------------------------------------------------------------------------------------------------ timestep embedding
def timestep_embed_ref(t, weight, freqs, d, aux=None, aux_w=None, aux_b=None):
    """emb[b] = [sin(arg) | cos(arg) | 0 if d is odd] + aux part, arg = (t_b w) f_i formed in fp32 as the kernel forms it, then fp64
    sin / cos of that fp32 argument.  Returns (fp64 reference, bound): 2^-22 on the sine / cosine part (2 ulp at magnitude 1,
    doubled) and, where aux is given, (aux_dim + 3) u (sum |aux s w| + |b| + 1) on top for the aux part and the final sum."""
    B, half = t.shape[0], d // 2
    w32 = torch.tensor(weight, dtype=torch.float32)
    arg = ((t.float() * w32)[:, None] * freqs.float()[None, :half]).double()
    ref = torch.zeros(B, d, dtype=torch.float64)
    ref[:, :half], ref[:, half:2 * half] = torch.sin(arg), torch.cos(arg)
    bound = torch.full((B, d), 2.0 ** -22, dtype=torch.float64)
    bound[:, 2 * half:] = 0.0
    if aux is not None and aux_w is not None:
        aux_dim = aux.shape[1]
        s = torch.sqrt(torch.tensor(float(aux_dim), dtype=torch.float32)).double()
        terms = (aux.double() * s)[:, None, :] * aux_w.double()[None, :, :]      # [B, d, aux_dim]
        ref += terms.sum(-1) + aux_b.double()[None, :]
        bound += (aux_dim + 3) * U * (terms.abs().sum(-1) + aux_b.double().abs()[None, :] + 1.0)
    return ref, bound


def default_freqs(d, max_period=10_000):
    half = d // 2
    return torch.exp(-math.log(max_period) * torch.arange(half, dtype=torch.float32) / max(half, 1))


# ------------------------------------------------------------------------------------------------------------ small-batch linear
def linear_small_path(B, N, K, ldx, ldw, x_align=0, w_align=0):
    """elementwise.hip, swiftk_linear_small: 'ealign', 'lds_prefetch' (K <= 1280), 'lds_walk' (1280 < K <= 1920) or 'wave'."""
    if x_align or w_align or ldx % 4 or ldw % 4:
        return "ealign"
    if K % 4 == 0 and 8 * K * 4 <= 60 * 1024 and N >= 4096:
        return "lds_prefetch" if K // 4 <= 5 * 64 else "lds_walk"
    return "wave"


def linear_small_ref(x, W, bias=None):
    """Exact fp64 pre-activation x W^T + bias ([B, K] x [N, K])."""
    z = x.double() @ W.double().t()
    return z + bias.double()[None, :] if bias is not None else z


def linear_small_max_partial(x, W, bias=None):
    """Largest magnitude any partial sum of any summation order can reach: sum |x w| + |bias|, in units of the operands' common
    power-of-two scale the caller divides out."""
    z = x.double().abs() @ W.double().abs().t()
    return float((z + (bias.double().abs()[None, :] if bias is not None else 0.0)).max())


def silu64(z):
    return z / (1.0 + torch.exp(-z))


def silu_allowance(z):
    """The act = 1 allowance: 4 x the largest relative error of torch CPU fp32 silu on the pre-activations z (fp64, exactly
    representable in fp32) against fp64 SiLU, never below 4u.  Returns (allowance, torch's figure)."""
    want = silu64(z)
    got = torch.nn.functional.silu(z.float()).double()
    nz = want != 0
    fig = float(((got - want).abs()[nz] / want.abs()[nz]).max()) if bool(nz.any()) else 0.0
    return max(4 * fig, 4 * U), fig


# ------------------------------------------------------------------------------------------------------------ rollout update, axpby
def rollout_ref(x, y, m, s, t):
    """Residual form in fp64 from the fp32 operands: phys = x s + m + y t, xstd = (phys - m) / s; [B, C, hw] with per-channel m, s, t.
    Returns (phys, xstd, phys bound 3u (|x s| + |m| + |y t|))."""
    v = lambda a: a.double().view(1, -1, 1)
    xs, yt = x.double() * v(s), y.double() * v(t)
    phys = xs + v(m) + yt
    return phys, (phys - v(m)) / v(s), 3 * U * (xs.abs() + v(m).abs() + yt.abs())


def rollout_xstd_from(p, m, s):
    """xstd against the kernel's OWN phys p: fp64 (p - m) / s and the bound 4u (|p| + |m|) / |s| (one subtraction, a division of at
    most 2.5 ulp)."""
    v = lambda a: a.double().view(1, -1, 1)
    return (p.double() - v(m)) / v(s), 4 * U * (p.double().abs() + v(m).abs()) / v(s).abs()


def axpby_ref(a, x, b, y):
    """fp64 a x + b y with a, b rounded to fp32 first, and the bound 2u (|a x| + |b y|)."""
    a32, b32 = float(torch.tensor(a, dtype=torch.float32)), float(torch.tensor(b, dtype=torch.float32))
    ax, by = a32 * x.double(), b32 * y.double()
    return ax + by, 2 * U * (ax.abs() + by.abs())


# ------------------------------------------------------------------------------------------------------------ column-sum gathers
def reduce_slabs_ref(slabs, ld_slab, slab_stride, nslabs, rows, cols, prefill=None):
    """out[r][c] (= | +=) sum_s slabs[s slab_stride + r ld_slab + c] on a flat fp32 buffer; fp64 [rows, cols]."""
    r, c = torch.arange(rows)[:, None], torch.arange(cols)[None, :]
    out = torch.zeros(rows, cols, dtype=torch.float64) if prefill is None else prefill.double().clone()
    for s in range(nslabs):
        out += slabs.double()[s * slab_stride + r * ld_slab + c]
    return out


def embed_bwd_sums_ref(src, cols, period):
    """src [rows = samples x period, lds]: bias[c] = sum_r src[r][c], pos[t][c] = sum_b src[b period + t][c] (fp64)."""
    nsamp = src.shape[0] // period
    b, t, c = torch.arange(nsamp)[:, None, None], torch.arange(period)[None, :, None], torch.arange(cols)[None, None, :]
    v = src.double()[b * period + t, c]                                                      # [samples, period, cols]
    return v.sum((0, 1)), v.sum(0)


def colsum_ref(src, cols, period):
    """period == 0: out[c] = sum_r src[r][c]; else out[r % period][c] += src[r][c] (fp64)."""
    rows = src.shape[0]
    r, c = torch.arange(rows), torch.arange(cols)
    v = src.double()[r[:, None], c[None, :]]
    if period == 0:
        return v.sum(0)
    out = torch.zeros(period, cols, dtype=torch.float64)
    return out.index_add_(0, r % period, v)


# ------------------------------------------------------------------------------------------------------------ the GEMM tile walk
def tile_coords(t, ntm, ntn, gm):
    """gemm.hip, TileIter::coords: tile number -> (tile row, tile column) by division; groups of gm tile rows, column-major inside
    a group, the last group ntm % gm rows high."""
    per = gm * ntn
    grp, r = divmod(t, per)
    rows = min(gm, ntm - grp * gm)
    tn = r // rows
    return grp * gm + (r - tn * rows), tn


def walk_digits(v, ntn, gm):
    """tile (or stride) v = (grp ntn + tn) gm + rr -> (grp, tn, rr)."""
    per = gm * ntn
    grp, r = divmod(v, per)
    tn, rr = divmod(r, gm)
    return grp, tn, rr


def walk_step(w, s, ntn, gm, first_carry_strict=False):
    """gemm.hip, walk_step: digits w advanced by the stride digits s with two carries.  Returns (new digits, carry 1, carry 2)."""
    (w_grp, w_tn, w_rr), (s_grp, s_tn, s_rr) = w, s
    w_rr += s_rr
    c1 = int(w_rr >= gm)
    w_rr -= gm if c1 else 0
    w_tn += s_tn + c1
    c2 = int(w_tn >= ntn)
    w_tn -= ntn if c2 else 0
    w_grp += s_grp + c2
    return (w_grp, w_tn, w_rr), c1, c2


def walk_coords(w, ntm, gm):
    """gemm.hip, walk_coords: a full group reads its coordinates off the digits; the short last group divides."""
    w_grp, w_tn, w_rr = w
    rows = ntm - w_grp * gm
    if rows < gm:
        r = w_tn * gm + w_rr
        tn = r // rows
        return w_grp * gm + (r - tn * rows), tn
    return w_grp * gm + w_rr, w_tn


Step = namedtuple("Step", "tile coords carry1 carry2 short")


def walk_trace(ntm, ntn, gm, stride, vid):
    """Every tile workgroup `vid` of `stride` visits: Step(tile, (tm, tn), carries of the step that led here, in the short group)."""
    ntiles = ntm * ntn
    if vid >= ntiles:
        return []
    w, s = walk_digits(vid, ntn, gm), walk_digits(stride, ntn, gm)
    tile, c1, c2, out = vid, 0, 0, []
    while True:
        out.append(Step(tile, walk_coords(w, ntm, gm), c1, c2, ntm - w[0] * gm < gm))
        if tile + stride >= ntiles:
            return out
        tile += stride
        w, c1, c2 = walk_step(w, s, ntn, gm)


def vid_of(bid, nwg):
    """gemm.hip: workgroups with equal blockIdx % 8 share an XCD and take a contiguous run of virtual ids."""
    q, r, xcd = nwg >> 3, nwg & 7, bid & 7
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + (bid >> 3)


WalkCase = namedtuple("WalkCase", "name epi M N gm wgs claims")
BM, BN = 256, 352   # K = 192: the 352-wide ping-pong kernel
# claims: 'digits' = the stride digits; 'c1_most' = the first carry on more than half the steps; 'both' = a step with both
# carries; 'short_carry' = a carrying step that lands in the short last group; 'short_rows' = height of that group;
# 'short_first' = every first tile lies in a short group; 'ntn' = column tiles
WALK_CASES = [
    WalkCase("first-carry", "none", 2048, 1056, 8, 5, dict(digits=(0, 0, 5), c1_most=True)),
    WalkCase("both-carries", "none", 3072, 704, 4, 13, dict(digits=(1, 1, 1), both=True)),
    WalkCase("carry-into-short-group", "none", 2560, 704, 4, 7, dict(short_carry=True, short_rows=2)),
    WalkCase("group-height-1", "none", 1024, 1056, 1, 5, dict(gm=1)),
    WalkCase("only-group-short", "none", 768, 704, 8, 4, dict(short_first=True, short_rows=3)),
    WalkCase("one-column-tile", "none", 2048, 352, 4, 3, dict(ntn=1)),
    WalkCase("both-carries-swiglu", "swiglu", 3072, 704, 4, 13, dict(digits=(1, 1, 1), both=True)),
]


# ------------------------------------------------------------------------------------------------------------ case tables
# Every row names the kernel it is meant to reach (`path`); tests/test_layout_reference_cpu.py checks that against the restated
# launcher conditions above.
PatchCase = namedtuple("PatchCase", "name path patch B H W chans lda scales per_sample misaligned_source misalign past_cap",
                       defaults=((0.5, 1.0, 2.0), False, -1, 0, False))
PATCHIFY_CASES = [
    PatchCase("tiled-1x1-three-sources", "tiled", (1, 1), 2, 32, 64, (5, 4, 3), 16),
    PatchCase("tiled-2x2-C11-chunks-straddle", "tiled", (2, 2), 2, 32, 64, (5, 4, 2), 48),
    PatchCase("tiled-3x2", "tiled", (3, 2), 2, 12, 64, (5, 4, 3), 72),
    PatchCase("tiled-2x3", "tiled", (2, 3), 2, 8, 48, (5, 4, 3), 72),
    PatchCase("tiled-one-source", "tiled", (2, 2), 2, 32, 64, (5, 0, 0), 24),
    PatchCase("tiled-source-1-absent", "tiled", (2, 2), 2, 32, 64, (5, 0, 3), 40),
    PatchCase("tiled-per-sample-B3", "tiled", (2, 2), 3, 32, 64, (5, 4, 3), 48, per_sample=True),
    PatchCase("element-7x7", "element", (7, 7), 2, 14, 21, (5, 4, 3), 592),
    PatchCase("element-2x3", "element", (2, 3), 2, 8, 48, (5, 4, 2), 67),
    PatchCase("element-1x1-gw24", "element", (1, 1), 2, 8, 24, (5, 4, 3), 16),
    PatchCase("element-misaligned-source", "element", (2, 2), 2, 32, 64, (5, 4, 3), 48, misaligned_source=1, misalign=1),
    PatchCase("element-per-sample-B3", "element", (2, 2), 3, 4, 12, (5, 4, 3), 50, per_sample=True),
    PatchCase("element-C228-tile-past-64 KiB", "element", (2, 2), 1, 4, 32, (100, 100, 28), 912),
    PatchCase("element-past-the-grid-cap", "element", (1, 1), 1, 128, 1028, (3, 2, 2), 8, past_cap=True),
]


def patchify_inputs(case, kind, seed=0):
    """The case's sources ([B, c, H, W] fp32 or None) and, for tagged inputs, their offsets.  kind: tagged | normal | edges."""
    srcs, offs, off = [], [], 0
    for s, c in enumerate(case.chans):
        if c == 0:
            srcs.append(None)
            offs.append(0)
            continue
        shape = (case.B, c, case.H, case.W)
        if kind == "tagged":
            srcs.append(tagged(shape, off))
        elif kind == "normal":
            srcs.append(normal(shape, 100 + 7 * seed + s))
        else:
            srcs.append(edge_values(math.prod(shape))[0].reshape(shape))
        offs.append(off)
        off += math.prod(shape)
    return srcs, offs


UnpatchCase = namedtuple("UnpatchCase", "name path patch B C H W ldt_extra wide xt_misalign past_cap", defaults=(0, 4, 0, False))
UNPATCHIFY_CASES = [
    UnpatchCase("fast4-2x2", "fast4", (2, 2), 3, 5, 32, 64),
    UnpatchCase("generic-1x1", "generic", (1, 1), 3, 5, 32, 64),
    UnpatchCase("generic-7x7", "generic", (7, 7), 3, 3, 14, 21),
    UnpatchCase("generic-2x3", "generic", (2, 3), 3, 4, 8, 48),
    UnpatchCase("generic-2x2-W6", "generic", (2, 2), 3, 5, 4, 6),
    UnpatchCase("generic-2x2-odd-ldt", "generic", (2, 2), 3, 5, 8, 16, ldt_extra=1, wide=2),
    UnpatchCase("generic-2x2-misaligned-xt", "generic", (2, 2), 3, 5, 8, 16, xt_misalign=1),
    UnpatchCase("generic-past-the-grid-cap", "generic", (1, 1), 3, 1, 1, 349528, wide=1, past_cap=True),
]

LinearCase = namedtuple("LinearCase", "name path B N K pad_x pad_w pad_o bias act px", defaults=(0, 0, 3, True, 0, 0))


def _lin(name, path, B, N, K, **kw):
    return LinearCase(name, path, B, N, K, **kw)


LINEAR_CASES = (
    [_lin(f"K{K}-N4100", path, 3, 4100, K) for K, path in ((4, "lds_prefetch"), (1056, "lds_prefetch"), (1280, "lds_prefetch"),
                                                           (1284, "lds_walk"), (1920, "lds_walk"), (1924, "wave"))]
    + [_lin(f"N{N}-K1056", path, 3, N, 1056) for N, path in ((1, "wave"), (13, "wave"), (4095, "wave"), (4096, "lds_prefetch"))]
    + [_lin(f"B{B}-{path}", path, B, N, K) for path, N, K in (("wave", 13, 1056), ("lds_prefetch", 4096, 64), ("lds_walk", 4096, 1284))
       for B in (1, 8, 9, 17)]
    + [_lin("K70-row-strides-72", "wave", 3, 13, 70, pad_x=2, pad_w=2)]
    + [_lin(f"wide-strides-{path}", path, 9, N, K, pad_x=8, pad_w=4, pad_o=5)
       for path, N, K in (("wave", 13, 1056), ("lds_prefetch", 4099, 64), ("lds_walk", 4099, 1284))]
    + [_lin(f"no-bias-{path}", path, 2, N, K, bias=False) for path, N, K in (("wave", 13, 64), ("lds_prefetch", 4096, 64), ("lds_walk", 4096, 1284))]
    + [_lin(f"silu-{path}", path, 5, N, K, act=1, px=-7)
       for path, N, K in (("wave", 4095, 1056), ("lds_prefetch", 4100, 1056), ("lds_walk", 4100, 1284))]
)
LinearCase.ldx = property(lambda c: c.K + c.pad_x)
LinearCase.ldw = property(lambda c: c.K + c.pad_w)
LinearCase.ldo = property(lambda c: c.N + c.pad_o)

_W_CACHE = {}


def linear_operands(case):
    """x [B, K] = integers in [-8, 8] times 2^px, W [N, K] integers in [-8, 8], bias [N] like x (or None), and px: every product
    and partial sum is an integer multiple of 2^px."""
    key = (case.N, case.K)
    if key not in _W_CACHE:
        _W_CACHE.clear()  # (one weight matrix alive at a time: the largest is 31 MB)
        _W_CACHE[key] = integers((case.N, case.K), 1000 + case.N + case.K)
    x = integers((case.B, case.K), 2000 + case.B + case.K, case.px)
    b = integers((case.N,), 3000 + case.N, case.px) if case.bias else None
    return x, _W_CACHE[key], b, case.px
