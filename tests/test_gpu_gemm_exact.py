"""-m gpu: the GEMM family, bit for bit, on exactly summable operands (tests/exact_gemm.py).

Every product and partial sum here is an integer the accumulators (fp32) and the stored type hold exactly, so each launch has ONE
right answer whatever the tile walk, the k-loop, the split or the chunking: torch.equal on the raw bits against a CPU fp64
product, over the whole output buffer including its NaN-patterned surroundings.  A failure names the first wrong element, the
tile it falls in and how many elements (and tiles) differ.  swiftk_unit_checksum gets the same treatment at the end.
"""
import ctypes

import pytest
import torch

import exact_gemm as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from swift_amd import _lib
    assert _lib.lib().swiftk_get_tuning(2) == X.GRID  # the table's tile counts are placed against this grid
    assert _lib.lib().swiftk_get_tuning(0) == 1 and _lib.lib().swiftk_get_tuning(20) == 1 and _lib.lib().swiftk_get_tuning(22) == 1
    return torch.device("cuda", 0)


def st():
    return torch.cuda.current_stream().cuda_stream


def L():
    from swift_amd import _lib
    return _lib.lib()


def tdt(name):
    return torch.bfloat16 if name == "bf16" else torch.float32


def code(name):
    from swift_amd import _lib
    return _lib.BF16 if name == "bf16" else _lib.F32


def sent(shape, out, device="cpu"):
    """A buffer of the result type, as its raw bits, prefilled with the NaN pattern."""
    if out == "f32":
        return torch.full(shape, X.SENT_F32, dtype=torch.int32, device=device)
    return torch.full(shape, X.SENT_BF16, dtype=torch.int16, device=device)


def check_bits(got, want, c, what, rows, cols, tile_rows=256):
    """got (device) and want (CPU): raw bits [R, ld]; [0, rows) x [0, cols) is the result, everything else sentinel."""
    torch.cuda.synchronize()
    g = got.cpu()
    if torch.equal(g, want):
        return
    cell = X.expected_cell(c)
    bad = (g != want).nonzero()
    r, col = bad[0].tolist()
    asf = (lambda t: t.view(torch.float32)) if g.dtype == torch.int32 else (lambda t: t.view(torch.bfloat16).float())
    inside = bad[(bad[:, 0] < rows) & (bad[:, 1] < cols)]
    tiles = sorted({(int(a) // tile_rows, int(b) // cell.width) for a, b in inside[:: max(1, len(inside) // 4096)].tolist()})
    where = (f"tile (row {r // tile_rows}, column {col // cell.width}) of the {tile_rows} x {cell.width} tiling" if r < rows and col < cols
             else "OUTSIDE the result: a sentinel was overwritten")
    pytest.fail(f"{c.name} [{c.cell}] {what}: {len(bad)} elements differ ({len(bad) - len(inside)} of them sentinels); first at (row {r}, "
                f"column {col}), {where}: got {float(asf(g[r, col])):g} (bits {int(g[r, col]) & 0xFFFFFFFF:#x}), want "
                f"{float(asf(want[r, col])):g}; tiles hit (sampled): {tiles[:12]}{' ...' if len(tiles) > 12 else ''}; {cell}")


def ids(cs):
    return [c.name for c in cs]


# ------------------------------------------------------------------------------------------------ swiftk_gemm, swiftk_gemm_chunked
@pytest.fixture(scope="module")
def scratch(dev):
    return torch.empty(L().swiftk_gemm_chunk_scratch_bytes(), dtype=torch.uint8, device=dev)


@pytest.mark.parametrize("c", X.cases("gemm", "chunked"), ids=ids(X.cases("gemm", "chunked")))
def test_gemm_exact(dev, scratch, c):
    """swiftk_gemm / swiftk_gemm_chunked with EPI_NONE, BIAS_POS and ACCUM: C = the integer product (+ integer bias and pos, + the
    integers C held), every bit; rows [M, M + 8) and columns [N, ldc) of the buffer untouched."""
    from swift_amd import _lib
    a, w, ref = X.rows_and_reference(c)
    bias, pos, c0 = X.epilogue_terms(c)
    ad, wd = a.to(dev).to(tdt(c.dt)), w.to(dev).to(tdt(c.dt))
    rows = c.M + 8
    want, buf = sent((rows, c.ldc), c.out), sent((rows, c.ldc), c.out, dev)
    epi, ep0, ep1 = _lib.EPI_NONE, None, None
    calls = 1
    if c.epi == "bias_pos":
        epi, bd, pd = _lib.EPI_BIAS_POS, bias.to(dev), None if pos is None else pos.to(dev)
        ep0, ep1 = bd.data_ptr(), None if pd is None else pd.data_ptr()
        ref = X.bias_pos_sum(c, ref, bias, pos)
    elif c.epi == "accum":
        epi, calls = _lib.EPI_ACCUM, 2
        buf[:c.M, :c.N] = X.to_bits(c0.double(), "f32").to(dev)
    for n in range(1, calls + 1):
        if c.entry == "chunked":
            rc = L().swiftk_gemm_chunked(ad.data_ptr(), c.lda, wd.data_ptr(), c.ldw, buf.data_ptr(), c.ldc, c.M, c.N, c.K, code(c.dt), code(c.out),
                                         epi, ep0, ep1, c.pos_rows, c.chunk_k, scratch.data_ptr(), scratch.numel(), st())
        else:
            rc = L().swiftk_gemm(ad.data_ptr(), c.lda, wd.data_ptr(), c.ldw, buf.data_ptr(), c.ldc, c.M, c.N, c.K, code(c.dt), code(c.out), epi,
                                 ep0, ep1, c.pos_rows, st())
        assert rc == c.rc
        want[:c.M, :c.N] = X.to_bits(c0.double() + n * ref if c.epi == "accum" else ref, c.out)
        check_bits(buf, want, c, f"call {n}", c.M, c.N)


# ------------------------------------------------------------------------------------------------ split-K
@pytest.mark.parametrize("c", X.cases("splitk", "splitk_bf16"), ids=ids(X.cases("splitk", "splitk_bf16")))
def test_gemm_splitk_exact(dev, c):
    """swiftk_gemm_splitk (fp32 slabs) and swiftk_gemm_splitk_bf16 (bf16 slabs, ternary operands): slab s = the product over k-tiles
    [s T / ksplit, (s + 1) T / ksplit), the slabs add up to the whole product, nothing else is written; ksplit > T is refused
    without a launch."""
    a, w, ref = X.rows_and_reference(c)
    ad, wd = a.to(dev).to(tdt(c.dt)), w.to(dev).to(tdt(c.dt))
    out = "bf16" if c.entry == "splitk_bf16" else "f32"
    rows = c.M + 8
    want, buf = sent((c.ksplit * rows, c.ldc), out), sent((c.ksplit * rows, c.ldc), out, dev)
    if c.entry == "splitk_bf16":
        rc = L().swiftk_gemm_splitk_bf16(ad.data_ptr(), c.lda, wd.data_ptr(), c.ldw, buf.data_ptr(), c.ldc, rows * c.ldc, c.M, c.N, c.K, c.ksplit, st())
    else:
        rc = L().swiftk_gemm_splitk(ad.data_ptr(), c.lda, wd.data_ptr(), c.ldw, buf.data_ptr(), c.ldc, rows * c.ldc, c.M, c.N, c.K, code(c.dt),
                                    c.ksplit, st())
    assert rc == c.rc
    if rc == 0:
        total = torch.zeros_like(ref)
        for s in range(c.ksplit):
            part = X.product(a, w, *X.k_range(c, s))
            total += part
            want[s * rows:s * rows + c.M, :c.N] = X.to_bits(part, out)
        assert torch.equal(total, ref)
    torch.cuda.synchronize()
    g = buf.cpu()
    for s in range(c.ksplit):
        check_bits(buf[s * rows:(s + 1) * rows], want[s * rows:(s + 1) * rows], c, f"slab {s} of {c.ksplit}", c.M, c.N)
    if rc == 0:
        vals = g.view(torch.float32 if out == "f32" else torch.bfloat16).view(c.ksplit, rows, c.ldc)[:, :c.M, :c.N].double().sum(0)
        assert torch.equal(vals, ref)


@pytest.mark.parametrize("c", X.cases("tail"), ids=ids(X.cases("tail")))
def test_gemm_tail_split_exact(dev, c):
    """swiftk_gemm_tail_split_bf16: slab 0 = the whole product under every tile of the full rounds (everywhere above tail[0] among
    others) and the first k-half under the split tiles of the last round, slab 1 = the second k-half under the split tiles and
    untouched everywhere else; the halves add up to the product."""
    a, w, ref = X.rows_and_reference(c)
    ad, wd = a.to(dev).to(torch.bfloat16), w.to(dev).to(torch.bfloat16)
    rows = c.M + 8
    buf = sent((2 * rows, c.ldc), "bf16", dev)
    tail = (ctypes.c_int64 * 3)(-1, -1, -1)
    rc = L().swiftk_gemm_tail_split_bf16(ad.data_ptr(), c.lda, wd.data_ptr(), c.ldw, buf.data_ptr(), c.ldc, rows * c.ldc, c.M, c.N, c.K, tail, st())
    assert rc == 0
    rows_from, tail_from, gm = tail[0], tail[1], tail[2]
    ntm, ntn = c.M // 256, c.N // 352
    tiles = ntm * ntn
    assert tail_from == tiles - tiles % X.GRID and gm >= 1 and rows_from == (tail_from // (gm * ntn)) * gm * 256 and 0 < rows_from < c.M
    # the walk's order (groups of gm tile rows, column-major inside a group): the tiles from tail_from on are split
    tm, tn = torch.meshgrid(torch.arange(ntm), torch.arange(ntn), indexing="ij")
    grp = tm // gm
    split = (grp * gm * ntn + tn * torch.clamp(ntm - grp * gm, max=gm) + (tm - grp * gm)) >= tail_from
    assert int(split.sum()) == tiles % X.GRID and not bool(split[: rows_from // 256].any())
    sel = split[:, None, :, None].expand(ntm, 256, ntn, 352).reshape(c.M, c.N)
    khalf_cols = (c.nk // 2) * 64
    first = X.product(a, w, 0, khalf_cols)
    second = X.product(a, w, khalf_cols, c.K)
    assert torch.equal(first + second, ref)
    want0, want1 = sent((rows, c.ldc), "bf16"), sent((rows, c.ldc), "bf16")
    want0[:c.M, :c.N] = torch.where(sel, X.to_bits(first, "bf16"), X.to_bits(ref, "bf16"))
    want1[:c.M, :c.N] = torch.where(sel, X.to_bits(second, "bf16"), want1[:c.M, :c.N])
    check_bits(buf[:rows], want0, c, f"slab 0 (tail {rows_from}, {tail_from}, {gm})", c.M, c.N)
    check_bits(buf[rows:], want1, c, f"slab 1 (tail {rows_from}, {tail_from}, {gm})", c.M, c.N)
    g = buf.cpu().view(torch.bfloat16).view(2, rows, c.ldc)[:, :c.M, :c.N].double()
    assert torch.equal(torch.where(sel, g[0] + g[1], g[0]), ref)


# ------------------------------------------------------------------------------------------------ batched, TN
@pytest.mark.parametrize("c", X.cases("batched"), ids=ids(X.cases("batched")))
def test_gemm_batched_exact(dev, c):
    """swiftk_gemm_batched: every matrix of the stack, strides larger than the matrices, NaN in the operands' gaps and the sentinel
    in the result's."""
    a, w, ref = X.rows_and_reference(c)
    sa, sw, sc = c.M * c.lda + c.gap, c.N * c.ldw + c.gap, (c.M + 2) * c.ldc + c.gap
    A = torch.full((c.batch, sa), float("nan"))
    W = torch.full((c.batch, sw), float("nan"))
    A[:, :c.M * c.lda] = a.view(c.batch, -1)
    W[:, :c.N * c.ldw] = w.view(c.batch, -1)
    ad, wd = A.to(dev).bfloat16(), W.to(dev).bfloat16()
    want, buf = sent((c.batch, sc), c.out), sent((c.batch, sc), c.out, dev)
    rc = L().swiftk_gemm_batched(ad.data_ptr(), c.lda, sa, wd.data_ptr(), c.ldw, sw, buf.data_ptr(), c.ldc, sc, c.batch, c.M, c.N, c.K, code(c.dt),
                                 code(c.out), st())
    assert rc == 0
    for b in range(c.batch):
        want[b, :(c.M + 2) * c.ldc].view(c.M + 2, c.ldc)[:c.M, :c.N] = X.to_bits(ref[b], c.out)
        check_bits(buf[b, :(c.M + 2) * c.ldc].view(c.M + 2, c.ldc), want[b, :(c.M + 2) * c.ldc].view(c.M + 2, c.ldc), c, f"matrix {b}", c.M, c.N)
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), want)  # (the gaps between the matrices too)


@pytest.mark.parametrize("c", X.cases("tn"), ids=ids(X.cases("tn")))
def test_gemm_tn_splitk_exact(dev, c):
    """swiftk_gemm_tn_splitk: slab s = P^T Q over the token rows of k-tiles [s T / ksplit, (s + 1) T / ksplit) against fp64, and
    their sum; what the header's shape rules refuse must come back as SWIFTK_ESHAPE."""
    p, q, ref = X.rows_and_reference(c)
    n1, n2, tok, ldp, ldq = c.M, c.N, c.K, c.lda, c.ldw
    ni = X.expected_cell(c).width // 32
    fits = tok % 64 == 0 and n1 % 8 == 0 and n2 % 4 == 0 and tok // 64 >= c.ksplit and ldp >= -(-n1 // 64) * 64 and \
        ldq >= (-(-n2 // 352) * 352 if ni == 11 else -(-n2 // 64) * 64)
    pd, qd = p.to(dev).bfloat16(), q.to(dev).bfloat16()
    rows = n1 + 8
    want, buf = sent((c.ksplit * rows, c.ldc), "f32"), sent((c.ksplit * rows, c.ldc), "f32", dev)
    rc = L().swiftk_gemm_tn_splitk(pd.data_ptr(), ldp, qd.data_ptr(), ldq, buf.data_ptr(), c.ldc, rows * c.ldc, n1, n2, tok, c.ksplit, st())
    assert fits == (c.rc == 0)  # the table says which rows the header refuses
    assert rc == c.rc
    total = torch.zeros_like(ref)
    for s in range(c.ksplit if fits else 0):
        r0, r1 = s * (tok // 64) // c.ksplit * 64, (s + 1) * (tok // 64) // c.ksplit * 64
        part = p[r0:r1, :n1].double().t() @ q[r0:r1, :n2].double() + 0.0
        total += part
        want[s * rows:s * rows + n1, :n2] = X.to_bits(part, "f32")
    assert not fits or torch.equal(total, ref)
    for s in range(c.ksplit):
        check_bits(buf[s * rows:(s + 1) * rows], want[s * rows:(s + 1) * rows], c, f"slab {s} of {c.ksplit}", n1, n2)


# ------------------------------------------------------------------------------------------------ linear outputs of fused epilogues
@pytest.mark.parametrize("c", X.cases("swiglu_both"), ids=ids(X.cases("swiglu_both")))
def test_swiglu_both_preactivation_exact(dev, c):
    from swift_amd import _lib
    a, w, ref = X.rows_and_reference(c)
    ad, wd = a.to(dev).bfloat16(), w.to(dev).bfloat16()
    H, rows = c.N // 2, c.M + 8
    want, buf = sent((rows, c.ldc), "bf16"), sent((rows, c.ldc), "bf16", dev)
    hm = sent((rows, H + 64), "bf16", dev)
    rc = L().swiftk_gemm(ad.data_ptr(), c.lda, wd.data_ptr(), c.ldw, buf.data_ptr(), c.ldc, c.M, c.N, c.K, _lib.BF16, _lib.BF16,
                         _lib.EPI_SWIGLU_BOTH, None, hm.data_ptr(), H + 64, st())
    assert rc == 0
    want[:c.M, :c.N] = X.to_bits(ref, "bf16")
    check_bits(buf, want, c, "pre-activation", c.M, c.N)
    assert not bool(hm[:c.M, :H].view(torch.bfloat16).isnan().any())
    assert bool((hm[:, H:] == X.SENT_BF16).all()) and bool((hm[c.M:] == X.SENT_BF16).all())


@pytest.mark.parametrize("c", X.cases("jvp"), ids=ids(X.cases("jvp")))
def test_gemm_jvp_kept_preactivation_exact(dev, c):
    from swift_amd import _lib
    a, w, ref = X.rows_and_reference(c)  # [2 Mh, N]: primal rows, then tangent rows
    ad, wd = a.to(dev).bfloat16(), w.to(dev).bfloat16()
    Mh, mlp = c.M, c.N // 2
    rows = Mh + 8
    want, buf = sent((rows, c.ldc), "bf16"), sent((rows, c.ldc), "bf16", dev)
    hm = sent((2 * Mh + 8, mlp + 64), "bf16", dev)
    rc = L().swiftk_gemm_jvp(ad.data_ptr(), c.lda, wd.data_ptr(), c.ldw, buf.data_ptr(), c.ldc, Mh, c.N, c.K, _lib.EPI_SWIGLU_JVP, None, None, 0,
                             hm.data_ptr(), mlp + 64, st())
    assert rc == 0
    want[:Mh, :c.N] = X.to_bits(ref[:Mh], "bf16")
    check_bits(buf, want, c, "kept pre-activation", Mh, c.N, tile_rows=128)
    assert not bool(hm[:2 * Mh, :mlp].view(torch.bfloat16).isnan().any())
    assert bool((hm[:, mlp:] == X.SENT_BF16).all()) and bool((hm[2 * Mh:] == X.SENT_BF16).all())


@pytest.mark.parametrize("c", X.cases("bias_pos_pair"), ids=ids(X.cases("bias_pos_pair")))
def test_gemm_bias_pos_pair_exact(dev, c):
    """swiftk_gemm_bias_pos_pair on integers: hi = the integer product + bias + pos itself, every low byte = 128 (no remainder)."""
    a, w, ref = X.rows_and_reference(c)
    bias, pos, _ = X.epilogue_terms(c)
    ad, wd, bd = a.to(dev).bfloat16(), w.to(dev).bfloat16(), bias.to(dev)
    pd = None if pos is None else pos.to(dev)
    rows = c.M + 8
    want, hi = sent((rows, c.ldc), "bf16"), sent((rows, c.ldc), "bf16", dev)
    lo = torch.full((rows, c.N), 7, dtype=torch.uint8, device=dev)
    rc = L().swiftk_gemm_bias_pos_pair(ad.data_ptr(), c.lda, wd.data_ptr(), c.ldw, hi.data_ptr(), c.ldc, lo.data_ptr(), c.N, c.M, c.N, c.K,
                                       bd.data_ptr(), None if pd is None else pd.data_ptr(), c.pos_rows, st())
    assert rc == 0
    x = X.bias_pos_sum(c, ref, bias, pos)
    assert float(x.abs().max()) <= 256
    want[:c.M, :c.N] = X.to_bits(x, "bf16")
    check_bits(hi, want, c, "hi", c.M, c.N)
    wlo = torch.full((rows, c.N), 7, dtype=torch.int16)
    wlo[:c.M] = 128
    check_bits(lo.to(torch.int16), wlo, c, "lo", c.M, c.N)


# ------------------------------------------------------------------------------------------------ tuning key 20 = 0, the tuning keys
ONE_BARRIER = ["p320_below-bb", "p320_below-bf", "p384_below-bb", "p384_below-bf", "p352_below-bb", "swiglu_both_H2816-bb", "accum_320-bf",
               "pair_1280-bb", "jvp_swiglu_1280-bb"]


@pytest.mark.parametrize("name", ONE_BARRIER)
def test_one_barrier_loop_exact(dev, scratch, name):
    """Tuning key 20 = 0: the same rows of the table through the one-barrier k-loop of the persistent kernel (the launcher's other
    arm at all three tile widths, plain, SwiGLU, ACCUM, pair-output and paired-row epilogues).  One right answer, so the same bits."""
    c, = [c for c in X.CASES if c.name == name]
    body = {"gemm": lambda: test_gemm_exact(dev, scratch, c), "swiglu_both": lambda: test_swiglu_both_preactivation_exact(dev, c),
            "jvp": lambda: test_gemm_jvp_kept_preactivation_exact(dev, c), "bias_pos_pair": lambda: test_gemm_bias_pos_pair_exact(dev, c)}[c.entry]
    assert X.expected_cell(c).kernel == "persistent" and L().swiftk_set_tuning(20, 0) == 0
    try:
        assert L().swiftk_get_tuning(20) == 0
        body()
    finally:
        L().swiftk_set_tuning(20, 1)


def test_tuning_keys_read_back(dev):
    """Every key include/swiftk.h documents (25 and 32 act on being set: left alone) takes the value it reports and reports it again;
    so does key 24 (the complete-row kernel's ablation bits); keys 10 and 99 do not exist."""
    for key in [*range(0, 10), *range(11, 25), *range(26, 32)]:
        v = L().swiftk_get_tuning(key)
        assert v >= 0, key
        assert L().swiftk_set_tuning(key, v) == 0 and L().swiftk_get_tuning(key) == v, key
    for key in (10, 99):
        assert L().swiftk_get_tuning(key) == -1 and L().swiftk_set_tuning(key, 1) == -1  # SWIFTK_EINVAL
        assert L().swiftk_get_tuning(key) == -1


# ------------------------------------------------------------------------------------------------ swiftk_unit_checksum
def checksum(x, B, n, ptr=None):
    out = torch.full((B,), float("nan"), dtype=torch.float64, device=x.device)
    scr = torch.empty(32 * B, dtype=torch.float64, device=x.device)
    rc = L().swiftk_unit_checksum(x.data_ptr() if ptr is None else ptr, out.data_ptr(), scr.data_ptr(), B, n, st())
    torch.cuda.synchronize()
    return rc, out.cpu()


@pytest.mark.parametrize("n", [4, 100, 132, 69 * 128 * 256])
def test_unit_checksum_exact(dev, n):
    """swiftk_unit_checksum (the only evidence the multi-GPU output collection has) on integer-valued fp32 inputs, where the fp64
    sum is exact in any order: all ones, a single one at both ends and on each side of every boundary of the 32 parts, and
    +/-1e8 around a run of ones (an fp32 accumulation loses the ones)."""
    rc, s = checksum(torch.ones(n, device=dev), 1, n)
    assert rc == 0 and s.tolist() == [float(n)]
    n4 = n // 4
    per = -(-n4 // 32)  # float4 elements per part (elementwise.hip, checksum_part_kernel)
    spots = {0, n - 1}
    for p in range(1, 32):
        if p * per < n4:
            spots |= {4 * p * per - 1, 4 * p * per}
    spots = sorted(spots)
    for i0 in range(0, len(spots), 8):  # (8 x 9 MB per launch at the largest n)
        at = spots[i0:i0 + 8]
        xb = torch.zeros(len(at), n, device=dev)
        xb[torch.arange(len(at), device=dev), torch.tensor(at, device=dev)] = 1.0
        rc, s = checksum(xb, len(at), n)
        assert rc == 0 and s.tolist() == [1.0] * len(at), (at, s.tolist())
    y = torch.ones(n)
    y[0], y[n - 1] = 1e8, -1e8
    rc, s = checksum(y.to(dev), 1, n)
    assert rc == 0 and s.tolist() == [float(n - 2)]
    if n >= 100:  # the pair inside one thread's float4 and across two parts
        y = torch.ones(n)
        y[1], y[2], y[4 * per - 1], y[4 * per] = 1e8, -1e8, -1e8, 1e8
        rc, s = checksum(y.to(dev), 1, n)
        assert rc == 0 and s.tolist() == [float(n - 4)]


@pytest.mark.parametrize("B", [1, 7, 96])
def test_unit_checksum_batch_slots(dev, B):
    """A unit's checksum is the same bits alone and in any slot of a batch, and equals the exact integer sum."""
    n = 4 * 1237
    g = torch.Generator().manual_seed(B)
    x = torch.randint(-1000, 1001, (B, n), generator=g).float()
    xd = x.to(dev)
    rc, s = checksum(xd, B, n)
    assert rc == 0 and torch.equal(s, x.double().sum(1))
    for b in sorted({0, B // 2, B - 1}):
        rc, one = checksum(xd[b].contiguous(), 1, n)
        assert rc == 0 and one.view(torch.int64).tolist() == s[b:b + 1].view(torch.int64).tolist()
    perm = torch.randperm(B, generator=g)
    rc, sp = checksum(xd[perm.to(dev)].contiguous(), B, n)
    assert rc == 0 and torch.equal(sp.view(torch.int64), s[perm].view(torch.int64))
    # non-integer values: still the same bits in every slot (the order of the additions is fixed)
    z = torch.randn(B, n, generator=g).to(dev)
    rc, sz = checksum(z, B, n)
    rc1, z0 = checksum(z[B - 1].contiguous(), 1, n)
    assert rc == 0 and rc1 == 0 and z0.view(torch.int64).tolist() == sz[B - 1:].view(torch.int64).tolist()


def test_unit_checksum_rejects(dev):
    x = torch.ones(64, device=dev)
    assert checksum(x, 1, 6)[0] == -2                         # n % 4 != 0: SWIFTK_ESHAPE
    assert checksum(x, 1, 8, ptr=x.data_ptr() + 4)[0] == -3   # misaligned pointer: SWIFTK_EALIGN
