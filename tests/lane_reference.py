"""The head-lane index map of SWIFTK_PAD_HEADS, restated in plain Python for the tests of ``swiftk_cast_pad_t_lanes`` /
``swiftk_lanes_grad_add`` and of the torch packers they replace (``engine.pack_*_lanes`` / ``unpack_*_lanes``).

Along the lane axis a parameter has ``blocks * hd`` entries (blocks = 3 * heads for to_qkv's rows: q, k and v of every head; heads
for wo's columns); on the device every block occupies ``hdp >= hd`` entries, the last ``hdp - hd`` of them zero."""
import torch

STRIDE = 4096  # tag(r, c) = r * STRIDE + c + 1: exact in fp32 below 2^24, never zero, and it names its own coordinate


def lane_src(p: int, hd: int, hdp: int) -> int:
    """Parameter index the lane-shaped index ``p`` reads; -1 on a pad lane."""
    b, j = divmod(p, hdp)
    return b * hd + j if j < hd else -1


def lane_dst(i: int, hd: int, hdp: int) -> int:
    """Lane-shaped index the parameter index ``i`` lands on."""
    b, j = divmod(i, hd)
    return b * hdp + j


def src_table(blocks: int, hd: int, hdp: int) -> torch.Tensor:
    return torch.tensor([lane_src(p, hd, hdp) for p in range(blocks * hdp)], dtype=torch.int64)


def dst_table(blocks: int, hd: int, hdp: int) -> torch.Tensor:
    return torch.tensor([lane_dst(i, hd, hdp) for i in range(blocks * hd)], dtype=torch.int64)


def tagged(rows: int, cols: int, dtype=torch.float64) -> torch.Tensor:
    assert rows * STRIDE + cols < 2 ** 24 and cols < STRIDE
    return (torch.arange(rows, dtype=torch.float64).view(-1, 1) * STRIDE + torch.arange(cols, dtype=torch.float64) + 1).to(dtype)


def untag(v: float):
    """(row, column) a tag names."""
    v = int(v) - 1
    return divmod(v, STRIDE)


def pack(w: torch.Tensor, axis: int, blocks: int, hd: int, hdp: int) -> torch.Tensor:
    """Lane-shaped copy of ``w`` by the table alone (gather + zero lanes)."""
    src = src_table(blocks, hd, hdp)
    g = w.index_select(axis, src.clamp_min(0))
    mask = (src >= 0).to(w.dtype)
    return g * (mask.view(-1, 1) if axis == 0 else mask.view(1, -1))


def unpack(g: torch.Tensor, axis: int, blocks: int, hd: int, hdp: int) -> torch.Tensor:
    """The parameter-shaped part of a lane-shaped ``g`` by the table alone."""
    return g.index_select(axis, dst_table(blocks, hd, hdp))
