"""Persistent bf16 GEMM outside its k-loop (tuning key 31): the straight-line epilogue of interior tiles (bit 0) and the incremental
tile walk (bit 1) against the forms they replace (key 31 = 0), bit for bit, at the smallest shapes where each new path can go wrong:
several tiles per workgroup (the slab base's advance, the walk's successor across the grouped order, the counted store wait between
tiles, the ping-pong loop's minimum of three k-tiles, the half k-tile), edge tiles beside interior ones in one launch (the predicated
cold path), and a last row group shorter than the group height.  The output sits in a buffer wider than the product, pre-filled with a
sentinel that every arm must leave alone.

The walk cases (tests/layout_reference.py, WALK_CASES; K = 192, whole 256 x 352 tiles) set the group height (tuning key 1) and the
workgroup count (key 2) so that the mixed-radix successor takes what no default launch does: a non-zero row digit of the stride, the
first carry, both carries in one step, a carrying step into the short last group, a row digit of radix 1, a walk whose only group is
short, and a single column tile.  tests/test_layout_reference_cpu.py checks that each case takes the carries its name claims."""
import pytest
import torch

from layout_reference import WALK_CASES

pytestmark = pytest.mark.gpu

SENTINEL = -7.0  # exact in bf16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _operands(dev, M, N, K, ldk, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    a = torch.zeros(M, ldk, dtype=torch.bfloat16, device=dev)
    a[:, :K] = torch.randn(M, K, generator=g, device=dev).bfloat16()
    w = torch.zeros(N, ldk, dtype=torch.bfloat16, device=dev)
    w[:, :K] = (0.05 * torch.randn(N, K, generator=g, device=dev)).bfloat16()
    return a, w


# (epilogue, M, N, K, row stride of the operands, workgroups (tuning key 2) or None for the default grid, group height (tuning key 1))
CASES = [
    pytest.param("none", 1024, 1056, 192, 192, 8, 8, id="interior-plain-12-tiles-on-8"),
    pytest.param("swiglu", 1024, 1408, 1056, 1088, 8, 8, id="interior-swiglu-16-tiles-on-8-half-k-tile"),
    pytest.param("none", 304, 536, 192, 192, None, 8, id="edges-plain"),
    pytest.param("swiglu", 304, 528, 1056, 1088, None, 8, id="edges-swiglu"),
    pytest.param("none", 2304, 704, 192, 192, 8, 8, id="short-last-group-plain"),
    pytest.param("swiglu", 2304, 704, 1056, 1088, 8, 8, id="short-last-group-swiglu"),
] + [pytest.param(c.epi, c.M, c.N, 192, 192, c.wgs, c.gm, id="walk-" + c.name) for c in WALK_CASES]


@pytest.mark.parametrize("epi, M, N, K, ldk, wgs, gm", CASES)
def test_key31_arms_equal_old_forms(dev, epi, M, N, K, ldk, wgs, gm):
    from swift_amd import _lib
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    a, w = _operands(dev, M, N, K, ldk, M + N)
    code = _lib.EPI_SWIGLU if epi == "swiglu" else _lib.EPI_NONE
    ncol = N // 2 if epi == "swiglu" else N
    ldc = ncol + 24
    key31, key2, group_m = L.swiftk_get_tuning(31), L.swiftk_get_tuning(2), L.swiftk_get_tuning(1)
    assert group_m == 8  # the short last group of the 2304-row cases is a statement about this group height
    outs = {}
    try:
        if wgs is not None:
            _lib.check(L.swiftk_set_tuning(2, wgs), "swiftk_set_tuning")
        _lib.check(L.swiftk_set_tuning(1, gm), "swiftk_set_tuning")
        assert L.swiftk_get_tuning(1) == gm
        for arm in (0, 1, 2, 3):
            _lib.check(L.swiftk_set_tuning(31, arm), "swiftk_set_tuning")
            assert L.swiftk_get_tuning(31) == arm
            _lib.check(L.swiftk_set_tuning(32, 0), "swiftk_set_tuning")  # (key 32: which SL instantiations were launched since)
            c = torch.full((M + 16, ldc), SENTINEL, dtype=torch.bfloat16, device=dev)  # (16 rows the product must not reach)
            _lib.check(L.swiftk_gemm(a.data_ptr(), ldk, w.data_ptr(), ldk, c.data_ptr(), ldc, M, N, K, _lib.BF16, _lib.BF16, code,
                                     None, None, 0, st), "swiftk_gemm")
            outs[arm] = c
            # the launch took the instantiation the arm names and no other: an arm that fell back to the old forms would pass every
            # comparison below without running a line of the new code
            assert L.swiftk_get_tuning(32) == 1 << arm, f"key 31 = {arm} launched SL mask {L.swiftk_get_tuning(32):#x}"
        torch.cuda.synchronize()
    finally:
        L.swiftk_set_tuning(31, key31)
        L.swiftk_set_tuning(2, key2)
        L.swiftk_set_tuning(1, group_m)
    ref = outs[0]
    # the old arm is the reference; it is itself the product (fp32 accumulation of the bf16 operands, one rounding to bf16: half an
    # ulp = 2^-9 relative, doubled for the SwiGLU epilogue's exp / rcp at 1 ulp of fp32 each and its three products)
    acc = a[:, :K].float() @ w[:, :K].float().t()
    want = torch.nn.functional.silu(acc[:, 0::2]) * acc[:, 1::2] if epi == "swiglu" else acc
    got = ref[:M, :ncol].float()
    assert torch.isfinite(got).all()
    assert float((got - want).abs().max()) <= 2.0 ** -8 * float(want.abs().max())
    for arm in (0, 1, 2, 3):
        assert bool((outs[arm][:, ncol:] == SENTINEL).all()), f"key 31 = {arm} wrote past column {ncol}"
        assert bool((outs[arm][M:] == SENTINEL).all()), f"key 31 = {arm} wrote past row {M}"
    for arm in (1, 2, 3):
        if not torch.equal(outs[arm].view(torch.int16), ref.view(torch.int16)):
            bad = torch.nonzero(outs[arm].view(torch.int16) != ref.view(torch.int16))
            r, c = int(bad[0][0]), int(bad[0][1])
            msg = (f"key 31 = {arm} differs from key 31 = 0 in {bad.shape[0]} elements, first at (row, column) ({r}, {c}) = tile "
                   f"(row, column) ({r // 256}, {c // (176 if epi == 'swiglu' else 352)})")
            print(msg)
            raise AssertionError(msg)


def test_key31_is_a_two_bit_mask(dev):
    """The key holds a two-bit mask and reads back what was set."""
    from swift_amd import _lib
    L = _lib.lib()
    key31 = L.swiftk_get_tuning(31)
    try:
        assert 0 <= key31 <= 3
        for v, want in ((7, 3), (2, 2), (0, 0)):
            _lib.check(L.swiftk_set_tuning(31, v), "swiftk_set_tuning")
            assert L.swiftk_get_tuning(31) == want
    finally:
        L.swiftk_set_tuning(31, key31)
