"""sCM and distillation on zero-padded head lanes (SWIFTK_PAD_HEADS=2), the CPU side: the switch levels, the four 5.625-degree
experiments of the distillation family, and the lane index map that ``swiftk_cast_pad_t_lanes`` / ``swiftk_lanes_grad_add``
implement -- restated in tests/lane_reference.py and compared here with the torch packers those kernels replace."""
import os

import pytest
import torch

import lane_reference as lanes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "swift_amd", "configs")
BF = torch.bfloat16


@pytest.mark.parametrize("value,pad,tangent", [(None, False, False), ("0", False, False), ("1", True, False), ("2", True, True),
                                               (" 2 ", True, True), ("true", True, False)])
def test_switch_levels(monkeypatch, value, pad, tangent):
    from swift_amd.engine import pad_heads_enabled, pad_heads_tangent_enabled
    if value is None:
        monkeypatch.delenv("SWIFTK_PAD_HEADS", raising=False)
    else:
        monkeypatch.setenv("SWIFTK_PAD_HEADS", value)
    assert pad_heads_enabled() is pad and pad_heads_tangent_enabled() is tangent


def test_level_two_pads_like_level_one(monkeypatch):
    from swift_amd._lib import SwiftkError
    from swift_amd.engine import head_lanes
    monkeypatch.setenv("SWIFTK_PAD_HEADS", "2")
    assert head_lanes(768, 12, BF) == (64, 80)
    assert head_lanes(1056, 16, BF) == (66, 80) and head_lanes(1056, 12, BF) == (88, 88) and head_lanes(768, 8, BF) == (96, 96)
    monkeypatch.delenv("SWIFTK_PAD_HEADS")
    with pytest.raises(SwiftkError, match="head_dim.*66") as e:  # the refusal still names the width and the switch
        head_lanes(1056, 16, BF)
    assert "SWIFTK_PAD_HEADS" in str(e.value)


@pytest.mark.parametrize("name,loss,solver,depth,dim,heads", [
    ("era5-swinv2-5.6-trigflow", "TrigFlowLoss", "2s", 12, 1056, 12), ("era5-swinv2-5.6-distill", "SCMLoss", "scm", 12, 1056, 12),
    ("era5-swinv2-5.6-distill-sm", "SCMLoss", "scm", 8, 768, 8), ("era5-swinv2-5.6-distill-md", "SCMLoss", "scm", 12, 768, 12)])
def test_distillation_experiments_compose(name, loss, solver, depth, dim, heads):
    from swift_amd.config import compose
    from swift_amd.train import apply_distill_flag
    cfg = compose(CONFIGS, "train", [f"experiment={name}"])
    assert cfg.experiment_name == name and cfg.loss["_target_"].endswith("loss." + loss)
    assert (cfg.model["depth"], cfg.model["dim"], cfg.model["heads"]) == (depth, dim, heads)
    assert list(cfg.model["patch_size"]) == [1, 1] and list(cfg.model["window_size"]) == [16, 16] and list(cfg.model["shift_size"]) == [8, 8]
    assert cfg.precond["_target_"].endswith("PassPrecond") and cfg.optimizer["_target_"].endswith("AdamW")
    assert cfg.loss["noise"]["dist"] == "loguniform"
    assert cfg.data["batch_size"] == 120 and cfg.data["data_workers"] == 4 and cfg.data["val_local_batch_size"] == 8
    tr = cfg.trainer
    assert (tr["total_kimg"], tr["ema_halflife_kimg"], tr["lr_rampup_kimg"], tr["lr_min_factor"], tr["lr_cosine_anneal"]) == \
        (200000, 500, 2000, 0.0001, False)
    assert (tr["kimg_per_tick"], tr["checkpoint_ticks"], tr["val_ticks"], tr["val_target_interval"]) == (1, 500, 100, 8)
    scm = compose(CONFIGS, "train", ["experiment=era5-swinv2-5.6-scm"])
    assert dict(cfg.data["dataset"]) == dict(scm.data["dataset"])  # the same 5.625-degree data
    if loss == "SCMLoss":
        assert dict(cfg.solver) == dict(scm.solver)
        assert cfg.get("distill") is None and cfg.loss["tangent_warmup_kimg"] == 3000  # a teacher is named on the command line
        assert not apply_distill_flag(cfg).loss.get("distillation")
        given = apply_distill_flag(compose(CONFIGS, "train", [f"experiment={name}", "distill=/runs/teacher/000"]))
        assert given.distill == "/runs/teacher/000" and given.loss["distillation"] is True
    else:
        assert "num_steps" in cfg.solver and cfg.get("distill") is None
        assert "distillation" not in apply_distill_flag(compose(CONFIGS, "train", [f"experiment={name}", "distill=/runs/x"])).loss


LANE_CASES = [(9, 33, 80), (48, 66, 80), (18, 64, 80), (4, 80, 80), (5, 1, 3)]


@pytest.mark.parametrize("blocks,hd,hdp", LANE_CASES)
def test_lane_map_is_a_bijection_onto_the_valid_lanes(blocks, hd, hdp):
    src, dst = lanes.src_table(blocks, hd, hdp), lanes.dst_table(blocks, hd, hdp)
    assert src.shape == (blocks * hdp,) and dst.shape == (blocks * hd,)
    assert torch.equal(src[dst], torch.arange(blocks * hd))  # lane_src undoes lane_dst
    assert int((src >= 0).sum()) == blocks * hd and int((src < 0).sum()) == blocks * (hdp - hd)
    pad = torch.ones(blocks * hdp, dtype=torch.bool)
    pad[dst] = False
    assert torch.equal(pad, src < 0)  # every index lane_dst never reaches is a pad lane
    assert torch.equal(pad.view(blocks, hdp)[:, hd:], torch.ones(blocks, hdp - hd, dtype=torch.bool))  # ... the tail of its block


@pytest.mark.parametrize("blocks,hd,hdp", LANE_CASES)
def test_packers_follow_the_lane_map_on_tagged_inputs(blocks, hd, hdp):
    """to_qkv: blocks = 3 * heads on the rows; wo: blocks = heads on the columns.  Tagged entries name their own coordinate, so an
    element in the wrong place says where it came from."""
    from swift_amd.engine import pack_qkv_lanes, pack_wo_lanes, unpack_qkv_lanes, unpack_wo_lanes
    other = 7
    if blocks % 3 == 0:
        heads = blocks // 3
        w = lanes.tagged(blocks * hd, other)
        wp = pack_qkv_lanes(w, heads, hd, hdp)
        assert torch.equal(wp, lanes.pack(w, 0, blocks, hd, hdp))
        for p in range(blocks * hdp):
            s = lanes.lane_src(p, hd, hdp)
            assert (not wp[p].any()) if s < 0 else lanes.untag(wp[p, 3]) == (s, 3)
        g = lanes.tagged(blocks * hdp, other)
        gu = unpack_qkv_lanes(g, heads, hd, hdp)
        assert torch.equal(gu, lanes.unpack(g, 0, blocks, hd, hdp))
        assert all(lanes.untag(gu[i, 2]) == (lanes.lane_dst(i, hd, hdp), 2) for i in range(blocks * hd))
    w = lanes.tagged(other, blocks * hd)
    wp = pack_wo_lanes(w, blocks, hd, hdp)
    assert torch.equal(wp, lanes.pack(w, 1, blocks, hd, hdp))
    for p in range(blocks * hdp):
        s = lanes.lane_src(p, hd, hdp)
        assert (not wp[:, p].any()) if s < 0 else lanes.untag(wp[5, p]) == (5, s)
    g = lanes.tagged(other, blocks * hdp)
    gu = unpack_wo_lanes(g, blocks, hd, hdp)
    assert torch.equal(gu, lanes.unpack(g, 1, blocks, hd, hdp))
    assert all(lanes.untag(gu[4, i]) == (4, lanes.lane_dst(i, hd, hdp)) for i in range(blocks * hd))


def test_new_entry_points_are_declared_and_bound():
    from swift_amd import _lib
    text = open(os.path.join(ROOT, "include", "swiftk.h")).read()
    for name, nargs in (("swiftk_cast_pad_t_lanes", 13), ("swiftk_lanes_grad_add", 11)):
        assert name in _lib.EXPORTS and len(_lib._SIGS[name][0]) == nargs
        assert f"int {name}(" in text
        assert hasattr(_lib.lib(), name)
