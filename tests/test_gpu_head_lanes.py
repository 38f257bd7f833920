"""-m gpu: head widths no kernel runs natively (66; 64 and 32 on bf16) on zero-padded head lanes (SWIFTK_PAD_HEADS=1).

Every case is depth 2 on a 64x64 image with 2x2 patches (a 32x32 token grid: four windows, one layer shifted) at B = 2 -- the
shapes of the SMALLB tests -- and takes its inputs and its bars from the existing test of the same path on a native width."""
import json
import os

import pytest
import torch

from conftest import rel_l2
from swift_amd.utils.detinit import det_normal
from test_gpu_model import BF16_TOL, FP32_TOL, SMALLB, build

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _variant(dim, heads):
    return dict(SMALLB, dim=dim, heads=heads)


def _three_engines(net, x, t, cond, dev):
    with torch.no_grad():
        y = net(x.to(dev), t.to(dev), cond.to(dev), 0.6)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            yb = net(x.to(dev), t.to(dev), cond.to(dev), 0.6)
        net.model.fp32_engine = "bf16x3"
        y3 = net(x.to(dev), t.to(dev), cond.to(dev), 0.6)
        net.model.fp32_engine = None
    return y.cpu(), yb.cpu(), y3.cpu()


@pytest.mark.parametrize("dim,heads,hd", [(1056, 16, 66), (384, 6, 64), (320, 10, 32)])
def test_forward_on_padded_lanes_vs_oracle(dev, monkeypatch, dim, heads, hd):
    """Inputs and bars of test_gpu_model.py::test_forward_other_swift_variants_vs_oracle (the project's bars for depth-2 nets), at
    dims that test already runs with native heads."""
    from swift_amd._lib import SwiftkError
    monkeypatch.delenv("SWIFTK_PAD_HEADS", raising=False)
    net, onet = build(_variant(dim, heads), 12, dev)
    x, cond = det_normal((2, 69, 64, 64), 12, "x"), det_normal((2, 72, 64, 64), 12, "cond")
    t = torch.tensor([0.4, 1.3])
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16), pytest.raises(SwiftkError, match=f"head_dim.*{hd}"):
        net(x.to(dev), t.to(dev), cond.to(dev), 0.6)  # bf16 refuses each of the three widths without the switch
    monkeypatch.setenv("SWIFTK_PAD_HEADS", "1")
    y, yb, y3 = _three_engines(net, x, t, cond, dev)
    with torch.no_grad():
        yo = onet(x, t, cond, 0.6)
    e32, e16, e3 = rel_l2(y, yo), rel_l2(yb, yo), rel_l2(y3, yo)
    print(f"dim {dim}, {heads} heads of {hd}: fp32 rel-L2 {e32:.3e}, bf16x3 rel-L2 {e3:.3e}, bf16 rel-L2 {e16:.3e}")
    for key in (torch.bfloat16, torch.float32, "bf16x3"):
        eng = net.model._engines[key]
        want = 64 if (hd == 64 and key != torch.bfloat16) else 80  # (64 stays native on the exact-fp32 attention)
        assert (eng.hd, eng.hdp) == (hd, want)
        assert int(eng.model.head_dim) == (0 if want == hd else want)
    assert e32 < FP32_TOL and e3 < FP32_TOL
    assert e16 < BF16_TOL


def test_fused_kernel_leaves_exact_zeros_in_the_pad_lanes(dev):
    """The premise on the existing kernel: swiftk_qkv_attention_fused on a pack_qkv_lanes-packed weight (16 heads of 66 on 80
    lanes, K = 1056, one sample on a 16x32 grid, shifted windows) returns exact zeros in every pad lane -- v's pad lanes are
    x . 0, so P V adds zeros -- and in the real lanes the oracle's attention on the UNPACKED weight, within the bound
    test_gpu_kernels.py::test_fused_qkv_attention uses for that yardstick (1.2e-2)."""
    import torch.nn.functional as F
    from oracle.swinv2 import cosine_window_attention, window_token_index
    from swift_amd import ops
    from swift_amd.engine import pack_qkv_lanes
    heads, hd, hdp, d, B, grid, shift = 16, 66, 80, 1056, 1, (16, 32), (8, 8)
    n, K = grid[0] * grid[1], ops.k_pad(torch.bfloat16, d)
    a = det_normal((B * n, d), 90, "a").to(torch.bfloat16)
    w = det_normal((heads * 3 * hd, d), 90, "w", std=0.03).to(torch.bfloat16)
    scale = torch.log(torch.tensor([10.0, 3.0, 30.0, 200.0, 1.0, 10.0, 50.0, 99.0, 101.0, 5.0, 20.0, 48.0, 2.0, 60.0, 47.0, 49.0]))
    ad = F.pad(a, (0, K - d)).to(dev)
    wd = F.pad(pack_qkv_lanes(w, heads, hd, hdp), (0, K - d)).to(dev)
    assert wd.shape == (heads * 3 * hdp, K)
    out = ops.qkv_attention_fused(ad, wd, scale.to(dev), B, grid, heads, shift, k=d, head_dim=hdp)
    o = out.float().cpu().view(B, n, heads, hdp)
    assert torch.isfinite(o).all() and not o[..., hd:].any()
    idx = window_token_index(grid, (16, 16), shift)
    qkv = F.linear(a.float(), w.float()).view(B, n, -1)
    ow = cosine_window_attention(qkv[:, idx.reshape(-1)].reshape(B * idx.shape[0], 256, -1), scale.view(1, heads, 1, 1), heads, naive=True)
    ref = torch.empty(B, n, heads * hd)
    ref[:, idx.reshape(-1)] = ow.reshape(B, idx.numel(), -1)
    e = rel_l2(o[..., :hd].reshape(B, n, heads * hd), ref)
    print(f"fused to_qkv + attention, 16 heads of 66 on 80 lanes vs the oracle on the unpacked weight: rel-L2 {e:.3e}")
    assert e < 1.2e-2


def test_nothing_moves_for_native_widths(dev, monkeypatch):
    from swift_amd._lib import SwiftkError
    x, cond = det_normal((2, 69, 64, 64), 12, "x"), det_normal((2, 72, 64, 64), 12, "cond")
    t = torch.tensor([0.4, 1.3])
    net, _ = build(SMALLB, 12, dev)
    outs = {}
    for switch in (None, "1"):
        if switch is None:
            monkeypatch.delenv("SWIFTK_PAD_HEADS", raising=False)
        else:
            monkeypatch.setenv("SWIFTK_PAD_HEADS", switch)
        net.model._engines.clear()  # the switch is read when an engine is built
        outs[switch] = _three_engines(net, x, t, cond, dev)
        assert all(int(e.model.head_dim) == 0 and (e.hd, e.hdp) == (88, 88) for e in net.model._engines.values())
    for a, b in zip(outs[None], outs["1"]):
        assert torch.equal(a, b)
    monkeypatch.delenv("SWIFTK_PAD_HEADS", raising=False)
    net16, _ = build(_variant(1056, 16), 12, dev)
    for autocast in (False, True):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast), \
                pytest.raises(SwiftkError, match="head_dim.*66"):
            net16(x.to(dev), t.to(dev), cond.to(dev), 0.6)


def test_training_step_on_padded_lanes_vs_oracle(dev, monkeypatch):
    """Inputs and bars of test_gpu_train.py::test_larger_variants_training_step_and_tangent_vs_oracle (loss rel 1e-3, every
    gradient cosine above 0.99), at 16 heads of 66; the replay bounds are those of test_graph_replay_equals_eager (the fp32
    atomics of the loss mean and of the column sums are the only run-to-run noise)."""
    from oracle import loss as oloss
    from swift_amd._lib import SwiftkError
    from swift_amd.jvp_engine import SwinJvpEngine
    from swift_amd.training.loss import TrigFlowLoss
    from swift_amd.training.trainer import GradAllReduce
    from test_gpu_train import _build_pair, _dataset, _grad_report
    monkeypatch.setenv("SWIFTK_PAD_HEADS", "1")
    net, onet, st = _build_pair(dev, 61, logvar=True, dim=1056, heads=16)
    ds = _dataset(61)
    L = TrigFlowLoss(ds, dict(dist="loguniform", sigma_min=0.02, sigma_max=200.0), sigma_data=1.0).to(dev)
    B = 2
    x, cond, z = det_normal((B, 69, 64, 64), 61, "x"), det_normal((B, 72, 64, 64), 61, "c"), det_normal((B, 69, 64, 64), 61, "z")
    tau, aux = torch.tensor([0.3, 4.0]).view(B, 1, 1, 1), torch.tensor([0.6, 0.6])
    ddp = GradAllReduce(net)

    def step():
        ddp.zero_grad_flat()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = L(ddp, x.to(dev), condition=cond.to(dev), auxiliary=aux.to(dev), _tau=tau.to(dev), _z=z.to(dev))
        loss.backward()
        return float(loss), ddp.flatten_grads().clone()

    l1, g1 = step()  # eager
    ref = oloss.trigflow_loss(onet, x, tau, z, L.w_var.cpu(), L.w_lat.cpu(), 1.0, condition=cond, auxiliary=aux, return_logvar=True)
    ref.backward()
    print(f"16 heads of 66: trigflow loss {l1:.6f} vs oracle {float(ref):.6f}; worst grad cosine {_grad_report(net, st):.4f}")
    assert l1 == pytest.approx(float(ref), rel=1e-3)
    att = net.model.transformer.layers[0][0]
    assert att.to_qkv.weight.grad.shape == att.to_qkv.weight.shape == (3 * 1056, 1056)
    assert att.wo.weight.grad.shape == att.wo.weight.shape == (1056, 1056)
    eng = net.model._train_engine
    assert (eng.hd0, eng.hd, eng.inner, eng.katt) == (66, 80, 1280, 1280) and eng.L[0]["qkv"].shape[0] == 3 * 1280
    assert not eng.graphs._graphs
    l2, g2 = step()  # captured into HIP graphs, then replayed
    assert len(eng.graphs._graphs) == 2  # forward + backward
    l3, g3 = step()  # replayed
    assert l2 == pytest.approx(l1, rel=1e-5) and l3 == pytest.approx(l1, rel=1e-5)
    assert rel_l2(g2.cpu(), g1.cpu()) < 5e-5 and rel_l2(g3.cpu(), g1.cpu()) < 5e-5
    _grad_report(net, st)  # the replay's gradients against the oracle's, parameter by parameter
    with pytest.raises(SwiftkError, match="tangent kernels"):  # sCM stays out of scope: the reference ships 66 only with EDM
        SwinJvpEngine(net.model, torch.bfloat16)


def test_edm_experiment_as_shipped_trains_validates_generates(tmp_path):
    """The user story: experiment=era5-swinv2-1.4-edm with its 16 heads of 66 (the `small` overrides of
    test_gpu_edm.py::test_edm_train_validate_generate_cli, which pins the refusal without the switch), then a forecast from the
    16-head checkpoint it wrote."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from test_gpu_cli import run
    small = ["data=era5-synthetic-1.4", "data.dataset.img_resolution=[64,64]", "data.dataset.length=48", "data.data_workers=0",
             "model.depth=2", "trainer.total_kimg=0.008", "trainer.kimg_per_tick=0.004", "trainer.checkpoint_ticks=1",
             "trainer.lr_rampup_kimg=0", "trainer.val_ticks=1", "trainer.val_target_interval=4", "data.val_local_batch_size=2",
             "data.batch_size=2", "solver.num_steps=3"]
    env = {"SWIFTK_PAD_HEADS": "1"}
    out = run(["swift_amd.train", "experiment=era5-swinv2-1.4-edm"] + small, cwd=str(tmp_path), env=env)
    assert "in-training validation: solver edm" in out, out[-2000:]
    rdir = tmp_path / "results" / "era5-swinv2-1.4-edm" / "000"
    lines = [json.loads(l) for l in open(rdir / "stats.jsonl")]
    assert lines and all(torch.isfinite(torch.tensor(l["train/loss"])) for l in lines)
    val = [json.loads(l) for l in open(rdir / "val_stats.jsonl")]
    assert val and torch.isfinite(torch.tensor(val[0]["val/rmse"]))
    out = run(["swift_amd.generate", "--input", str(rdir), "--members", "2", "--steps", "2", "--samples", "2", "--batch", "4",
               "--num-steps", "3"], cwd=str(tmp_path), env=env)
    assert os.path.isdir(rdir / "output" / "latest"), out[-2000:]
    assert any(n.endswith(".zarr") for n in os.listdir(rdir / "output" / "latest"))
