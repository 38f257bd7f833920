"""CPU checks of tests/exact_gemm.py: the exactness the GPU tests of test_gpu_gemm_exact.py rest on holds for every row's actual
inputs, the fp64 reference is the integer product, bf16 rounding is RNE, and the case table reaches every dispatch cell it is
meant to reach (a dropped row fails here, not silently on the GPU)."""
import time

import pytest
import torch

import exact_gemm as X


def test_every_case_is_exactly_summable():
    """wide: 64 K (+ the epilogue's integers, twice the product for ACCUM's second call) < 2^24; ternary: the running prefix at every
    64-column boundary <= 128, so every sum over whole k-tiles fits bf16's 8 bits of integer; the references are integers inside
    those bounds (computed for every row, the largest included: the time of this test is the time the GPU file spends on the CPU)."""
    t0, flops, worst = time.time(), 0, {}
    for c in X.CASES:
        a, w, ref = X.rows_and_reference(c)
        flops += c.flops
        assert torch.equal(ref, ref.round()) and not torch.isnan(ref).any(), c.name
        peak = float(ref.abs().max())
        if c.family == "wide":
            assert float(a[:, :c.K if c.entry != "tn" else c.M].abs().max()) <= 8 and 2 * 64 * c.K + 3 * 8 < 2 ** 24, c.name
            assert peak <= 64 * c.K
        else:
            assert c.dt == "bf16" and c.entry != "tn" and c.entry != "batched"
            pm = X.prefix_max(a, w, c.K)
            worst[c.name] = pm
            assert pm <= 128, (c.name, pm)
            assert peak <= 128
        if c.khalf:  # the pad the half-k-tile rule speaks of: finite and non-zero in A, zero in W; NaN behind it
            h = c.tile_k // 2
            assert bool((a[:, c.K:c.K + h] == 3.0).all()) and bool((w[:, c.K:c.K + h] == 0.0).all())
            assert bool(a[:, c.K + h:].isnan().all()) and bool(w[:, c.K + h:].isnan().all())
        elif c.entry != "tn":
            assert bool(a[:, c.K:].isnan().all()) and bool(w[:, c.K:].isnan().all())
    dt = time.time() - t0
    print(f"{len(X.CASES)} cases, {flops / 1e9:.0f} GFLOP of fp64 references + prefix sums in {dt:.1f} s; largest ternary prefix "
          f"{max(worst.values()):.0f} ({max(worst, key=worst.get)})")


@pytest.mark.parametrize("M,N,K", [(37, 52, 64), (128, 100, 1056), (16, 352, 2816)])
def test_fp64_reference_is_the_integer_product(M, N, K):
    for fam in ("wide", "ternary"):
        a, w = X.ints((M, K), fam, 11), X.ints((N, K), fam, 12)
        exact = a.long() @ w.long().t()
        ref = X.product(a.float(), w.float())
        assert torch.equal(ref, exact.double())
        assert torch.equal(ref.float().long(), exact)                      # fp32 holds it
        if fam == "ternary":
            assert torch.equal(ref.float().bfloat16().float().long(), exact)  # and so does bf16


def test_ternary_family_has_the_stated_density():
    x = X.ints((4096, 1024), "ternary", 5)
    for v, p in ((-1, 0.125), (1, 0.125), (0, 0.75)):
        assert abs(float((x == v).float().mean()) - p) < 0.002
    y = X.ints((4096, 1024), "wide", 5)
    assert int(y.min()) == -8 and int(y.max()) == 8 and abs(float(y.float().mean())) < 0.02


def test_bf16_rounding_of_integers_is_rne():
    """bf16 keeps 8 significant bits: integers in [256, 512) round to even multiples of 2, ties to the even neighbour."""
    src = [255, 256, 257, 258, 259, 261, 263, 511, 513, 514, 515, 516, 518, 1026, 1028, 1030, 1032, 1036, -257, -259, -1028, 22527, 22528 + 64,
           22528 + 192, 180224 - 512]
    want = [255, 256, 256, 258, 260, 260, 264, 512, 512, 512, 516, 516, 520, 1024, 1024, 1032, 1032, 1040, -256, -260, -1024, 22528, 22528,
            22528 + 256, 180224]
    got = X.to_bits(torch.tensor(src, dtype=torch.float64), "bf16").view(torch.bfloat16).float().long().tolist()
    assert got == want
    # truncation would give something else on most of them
    trunc = (torch.tensor(src, dtype=torch.float32).view(torch.int32) & ~0xFFFF).view(torch.float32).long().tolist()
    assert sum(t != w for t, w in zip(trunc, want)) >= 10
    # the wide family at a forward-pass K: most results are rounded and a good part are exact ties
    a, w = X.ints((256, 2816), "wide", 1), X.ints((352, 2816), "wide", 2)
    ref = X.product(a.float(), w.float())
    back = X.to_bits(ref, "bf16").view(torch.bfloat16).double()
    ulp = 2.0 ** (torch.floor(torch.log2(ref.abs().clamp(min=1))) - 7)
    rounded, ties = float((back != ref).double().mean()), float(((ref - back).abs() * 2 == ulp).double().mean())
    print(f"wide family, K = 2816: {100 * rounded:.0f} % of the outputs are rounded by the bf16 store, {100 * ties:.0f} % are ties")
    assert rounded > 0.5 and ties > 0.1


def test_case_table_reaches_every_listed_cell():
    cells = {X.expected_cell(c) for c in X.CASES if c.rc == 0}
    for req in X.REQUIRED:
        assert any(all(getattr(cell, k) == v for k, v in req.items()) for cell in cells), f"no row of CASES reaches {req}"
    # rows the header's rules reject are in the table to assert the rejection
    assert {c.entry for c in X.CASES if c.rc != 0} == {"splitk", "splitk_bf16", "tn"}
    # the k-ranges of the split forms tile [0, K) without gap or overlap
    for c in X.cases("splitk", "splitk_bf16"):
        if c.rc == 0:
            edges = [X.k_range(c, s) for s in range(c.ksplit)]
            assert edges[0][0] == 0 and edges[-1][1] == c.K and all(a[1] == b[0] and a[0] < a[1] for a, b in zip(edges, edges[1:]))
    # the tail form's shapes leave a last round that is at most half full
    for c in X.cases("tail"):
        tiles = (c.M // 256) * 3
        assert tiles > X.GRID and 0 < tiles % X.GRID <= X.GRID // 2


def test_split_k_refuses_an_empty_k_range_before_any_launch():
    """ksplit > k-tiles would leave a k-range empty, and a work item of the persistent kernel ends on the LAST k-tile of its range:
    the host refuses it, as swiftk_gemm_tn_splitk does.  Argument validation only (placeholder addresses, no GPU), but it needs the
    built libswiftk.so, like tests/test_abi_and_layout.py."""
    from swift_amd import _lib
    L = _lib.lib()
    assert L.swiftk_gemm_splitk(16, 128, 16, 128, 16, 8, 64, 8, 8, 128, _lib.BF16, 3, None) == X.ESHAPE
    assert L.swiftk_gemm_splitk(16, 64, 16, 64, 16, 8, 64, 8, 8, 64, _lib.F32, 3, None) == X.ESHAPE
    assert L.swiftk_gemm_splitk_bf16(16, 128, 16, 128, 16, 8, 64, 8, 8, 128, 3, None) == X.ESHAPE
    assert L.swiftk_gemm_splitk_bf16(16, 96, 16, 96, 16, 8, 64, 8, 8, 32, 2, None) == X.ESHAPE  # half a k-tile + its pad: one k-tile
    assert L.swiftk_gemm_tn_splitk(16, 64, 16, 64, 16, 8, 64, 8, 8, 128, 3, None) == X.ESHAPE
