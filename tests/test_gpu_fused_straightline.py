"""-m gpu: the straight-line hand-off and output stage of swiftk_qkv_attention_fused (tuning key 30) against the forms they
replace, which stay selectable as the yardstick: bit 0 = hand-off, bit 1 = output stage + item decode, 0 = the old arm.

The new forms do the same arithmetic in the same order (a multiply by 1.0f on the v lanes of the q|v block is exact), so the
outputs must be bit-equal -- torch.equal, no tolerance.  Correctness of the old arm itself is test_gpu_kernels.py's business
(test_fused_qkv_attention).  Operands follow that test's recipe: rnd, zeroed k-padding, a logit-scale vector that mixes heads
with bound <= 48 (max-free softmax) and > 48 (online form), output rows padded with a sentinel that must stay untouched.

Shapes: grid (16, 32) = two windows, the smallest that changes the window inside set_item; head_dim 88 (q|v and v|pad blocks,
half k-tile) with 12 heads, 80 and 96 (whole blocks; 96 with the LDS overlap) with 16; two walks -- B = 3 on the default grid
(72 / 96 items: at most one per workgroup) and B = 1 on 8 workgroups (tuning key 2; 3 / 4 items back to back per workgroup:
cross-item prefetch, output slabs reused, the incremental item decode carries).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

GRID = (16, 32)
SCALES = [10.0, 3.0, 30.0, 200.0, 1.0, 10.0, 50.0, 99.0, 101.0, 5.0, 20.0, 48.0, 2.0, 60.0, 47.0, 49.0]
KEY_GRID, KEY_SL = 2, 30
SENTINEL = 7.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def rnd(shape, seed, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * std


_operands = {}


def operands(dev, hd, B):
    """(a, w, scale, heads, d, ldo) for one head_dim and batch, made once and left unchanged."""
    if (hd, B) not in _operands:
        from swift_amd import ops
        heads = 12 if hd == 88 else 16
        n, d = GRID[0] * GRID[1], heads * hd
        K = ops.k_pad(torch.bfloat16, d)
        a, w = rnd((B * n, K), 60 + B), rnd((3 * heads * hd, K), 61, 0.03)
        a[:, d:] = 0
        w[:, d:] = 0
        scale = torch.log(torch.tensor(SCALES[:heads])).to(dev)
        ldo = K + (0 if hd == 88 else 64)  # padded rows, as in the engine (88: 1056 -> 1088)
        _operands[(hd, B)] = (a.to(dev).bfloat16(), w.to(dev).bfloat16(), scale, heads, d, ldo)
    return _operands[(hd, B)]


def run(dev, hd, B, shift, sl, fill=SENTINEL, wgs=None):
    """One call with tuning key 30 = sl (and key 2 = wgs) into a fresh buffer filled with `fill`; both keys restored."""
    from swift_amd import _lib, ops
    L = _lib.lib()
    a, w, scale, heads, d, ldo = operands(dev, hd, B)
    out = torch.full((B, GRID[0] * GRID[1], ldo), fill, dtype=torch.bfloat16, device=dev)
    sl0, wgs0 = L.swiftk_get_tuning(KEY_SL), L.swiftk_get_tuning(KEY_GRID)
    try:
        assert L.swiftk_set_tuning(KEY_SL, sl) == 0
        if wgs is not None:
            assert L.swiftk_set_tuning(KEY_GRID, wgs) == 0
        ops.qkv_attention_fused(a, w, scale, B, GRID, heads, shift, out=out[..., :d], k=d, head_dim=hd)
        torch.cuda.synchronize()
    finally:
        L.swiftk_set_tuning(KEY_SL, sl0)
        L.swiftk_set_tuning(KEY_GRID, wgs0)
    return out, d


WALKS = [(3, None), (1, 8)]  # (B, workgroups): one item per workgroup | 3-4 items per workgroup


def test_key_30_defaults_and_round_trip(dev):
    from swift_amd import _lib
    L = _lib.lib()
    v0 = L.swiftk_get_tuning(KEY_SL)
    assert 0 <= v0 <= 3
    try:
        for v in (0, 1, 2, 3):
            assert L.swiftk_set_tuning(KEY_SL, v) == 0 and L.swiftk_get_tuning(KEY_SL) == v
    finally:
        L.swiftk_set_tuning(KEY_SL, v0)


@pytest.mark.parametrize("walk", WALKS, ids=["B3-default-grid", "B1-8wgs"])
@pytest.mark.parametrize("shift", [(0, 0), (3, 5)])
@pytest.mark.parametrize("hd", [88, 80, 96])
def test_new_arms_bit_equal_to_old(dev, hd, shift, walk):
    B, wgs = walk
    old, d = run(dev, hd, B, shift, 0, wgs=wgs)
    assert torch.isfinite(old.float()).all() and (old[..., d:].float() == SENTINEL).all()
    assert (old[..., :d].float().abs().amax(-1) > 0).all()  # every token row carries a result
    for sl in (3, 1, 2):
        new, _ = run(dev, hd, B, shift, sl, wgs=wgs)
        assert (new[..., d:].float() == SENTINEL).all(), f"key 30 = {sl}: pad columns written"
        assert torch.equal(new[..., :d], old[..., :d]), f"key 30 = {sl} differs from the old arm"


@pytest.mark.parametrize("walk", WALKS, ids=["B3-default-grid", "B1-8wgs"])
@pytest.mark.parametrize("hd", [88, 80, 96])
def test_repeat_call_is_bit_identical(dev, hd, walk):
    """A second call into a buffer pre-filled with a different value: no dependence on what the output or the LDS held."""
    from swift_amd import _lib
    B, wgs = walk
    sl = _lib.lib().swiftk_get_tuning(KEY_SL)  # the shipped default
    first, d = run(dev, hd, B, (3, 5), sl, fill=SENTINEL, wgs=wgs)
    second, _ = run(dev, hd, B, (3, 5), sl, fill=-3.0, wgs=wgs)
    assert torch.equal(first[..., :d], second[..., :d])
    assert (second[..., d:].float() == -3.0).all()


def test_output_offset_guard(dev):
    """The kernel addresses a sample's output rows with 32-bit byte offsets: gh * gw * ldo * 2 >= 4 GiB is refused with
    SWIFTK_ESHAPE (-2) and nothing is launched (small real buffers, a large ldo: a launch would write far outside them)."""
    from swift_amd import _lib
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    a = torch.zeros(2 * 512, 1152, dtype=torch.bfloat16, device=dev)
    w = torch.zeros(3168, 1152, dtype=torch.bfloat16, device=dev)
    sc = torch.zeros(12, device=dev)
    out = torch.full((2 * 512, 1088), SENTINEL, dtype=torch.bfloat16, device=dev)
    call = lambda ldo: L.swiftk_qkv_attention_fused(a.data_ptr(), 1152, w.data_ptr(), 1152, sc.data_ptr(), out.data_ptr(), ldo,
                                                    1056, 2, 16, 32, 12, 88, 0, 0, st)
    sl0 = L.swiftk_get_tuning(KEY_SL)
    try:
        for sl in (0, 3):  # the guard belongs to the entry point, whichever arm is selected
            L.swiftk_set_tuning(KEY_SL, sl)
            assert call(1 << 22) == -2       # 512 tokens x 2^22 elements x 2 B = 4 GiB exactly
            assert call((1 << 22) + 8) == -2
            assert call(1 << 30) == -2
    finally:
        L.swiftk_set_tuning(KEY_SL, sl0)
    torch.cuda.synchronize()
    assert (out.float() == SENTINEL).all()
    assert call(1088) == 0                   # the same buffers run at their real row length
    torch.cuda.synchronize()
    assert not (out[:, :1056].float() == SENTINEL).any()
