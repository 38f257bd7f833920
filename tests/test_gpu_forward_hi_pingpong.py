"""-m gpu: the forward's two alternating hi buffers of the pair-form residual stream (tuning key 33, counted by key 34).

On the plain wo / w2 + ModulatedNorm path of the bf16 engine the norm writes the new hi to a second buffer
(swiftk_modnorm_residual_pair_to, which tests/test_gpu_modnorm_rows.py scores row by row) and the two buffers change roles.  The
arithmetic is that of the in-place call -- the same kernel with another store address -- so the check is bit for bit.
"""
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

KEY_SPLITK, KEY_PINGPONG, KEY_PINGPONG_SEEN = 14, 33, 34


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def test_forward_alternating_hi_is_bit_equal(dev):
    """swiftk_swinv2_forward at dim 1056, depth 2, a 32 x 32 grid, one and two samples, on the plain wo / w2 + norm path (tuning key
    14 = 0: this small grid would otherwise run split-K): key 33 = 1 exchanges the two buffers four times (key 34), key 33 = 0 never,
    and the outputs are the same bit for bit -- twice in a row, so a forward that left the buffers exchanged would show.  With
    split-K on (the shipped form at this size) nothing is exchanged."""
    import test_gpu_model as tm
    from swift_amd import _lib
    L = _lib.lib()
    g = load_golden("swinv2_smallb")
    net, _ = tm.build(tm.SMALLB, int(g["seed"]), dev)
    x = tm.det_normal((2, 141, 64, 64), int(g["seed"]), "x").to(dev)
    t, aux = torch.from_numpy(g["t"]).to(dev), torch.from_numpy(g["aux"]).to(dev)
    shipped = {k: L.swiftk_get_tuning(k) for k in (KEY_SPLITK, KEY_PINGPONG)}
    assert shipped[KEY_PINGPONG] == 1

    def run(B, splitk, pingpong):
        L.swiftk_set_tuning(KEY_SPLITK, splitk)
        L.swiftk_set_tuning(KEY_PINGPONG, pingpong)
        L.swiftk_set_tuning(KEY_PINGPONG_SEEN, 0)
        try:
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                y = net.model(x[:B], t[:B], auxiliary=aux[:B])
            torch.cuda.synchronize()
            return y.float().cpu(), L.swiftk_get_tuning(KEY_PINGPONG_SEEN)
        finally:
            for k, v in shipped.items():
                L.swiftk_set_tuning(k, v)

    for B in (1, 2):
        y0, n0 = run(B, 0, 0)
        y1, n1 = run(B, 0, 1)
        y1b, n1b = run(B, 0, 1)
        _, n_splitk = run(B, shipped[KEY_SPLITK], 1)
        assert (n0, n1, n1b, n_splitk) == (0, 4, 4, 0), (B, n0, n1, n1b, n_splitk)
        assert bool(torch.isfinite(y0).all())
        assert torch.equal(y0, y1) and torch.equal(y0, y1b), B
