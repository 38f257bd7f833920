"""-m gpu: EDM (EDMPrecond, edm_sampler, EDMLoss) on the MI355X against the CPU restatement of tests/edm_reference.py (which
tests/test_edm_cpu.py pins to the reference's own outputs), on a depth-2 dim-1056 / 12-head net at the SMALLB grid."""
import os

import pytest
import torch

import edm_reference as er
from conftest import rel_l2
from swift_amd.utils.detinit import det_normal, swinv2_state
from test_gpu_model import BF16_TOL, FP32_TOL, SMALLB
from test_gpu_train import _dataset, _grad_report

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SD = 0.5


def _build(seed, clamp_scale=False):
    from oracle.swinv2 import OracleNet, SwinCfg
    from swift_amd.models.precond import EDMPrecond
    c = SMALLB
    nv, nf = c["n_vars"], c["n_forc"]
    mcfg = dict(_target_="swift.models.swinv2.SwinV2", window_size=list(c["window"]), shift_size=list(c["shift"]),
                patch_size=list(c["patch"]), depth=c["depth"], dim=c["dim"], heads=c["heads"])
    net = EDMPrecond(mcfg, img_resolution=list(c["img"]), img_channels=nv, condition_channels=nv + nf, auxiliary_dim=1,
                     sigma_data=SD)
    state = swinv2_state(grid=(32, 32), in_channels=2 * nv + nf, out_channels=nv, patch_size=c["patch"], depth=c["depth"],
                         dim=c["dim"], heads=c["heads"], auxiliary_dim=1, seed=seed)
    if clamp_scale:  # (the training tests' nets: logit scales below e^3)
        for k in state:
            if k.endswith(".scale"):
                state[k] = state[k].clamp(max=3.0)
    net.load_state_dict(state, strict=True)
    st = {k: v.clone().requires_grad_(True) for k, v in state.items()}
    ocfg = SwinCfg(img_resolution=c["img"], in_channels=2 * nv + nf, out_channels=nv, window_size=c["window"],
                   shift_size=c["shift"], patch_size=c["patch"], depth=c["depth"], dim=c["dim"], heads=c["heads"], auxiliary_dim=1)
    return net.to("cuda").eval(), OracleNet(ocfg, st, nv, nv + nf, sigma_data=SD), st


@pytest.fixture(scope="module")
def nets():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _build(51)


def test_edm_precond_forward_vs_restatement(nets):
    net, onet, _ = nets
    B = 3
    x, cond = det_normal((B, 69, 64, 64), 51, "x"), det_normal((B, 72, 64, 64), 51, "c")
    sig, aux = torch.tensor([0.03, 1.0, 80.0]), torch.tensor([0.6, 0.6, 0.6])
    with torch.no_grad():
        ref = er.precond(onet, x, sig, cond, aux)
        xd, cd, sd_, ad = x.cuda(), cond.cuda(), sig.cuda(), aux.cuda()
        y32 = net(xd, sd_, cd, ad)
        net.model.fp32_engine = "bf16x3"
        y3 = net(xd, sd_, cd, ad)
        net.model.fp32_engine = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y16 = net(xd, sd_, cd, ad)
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")  # a device sigma: c_in / c_skip / c_out / c_noise never reach the host
            try:
                y16b = net(xd, sd_, cd, ad)
            finally:
                torch.cuda.set_sync_debug_mode(0)
        # a number sigma (host coefficients) and a [1] tensor give the same as the per-sample vector
        y1 = net(xd[1:2], 1.0, cd[1:2], ad[1:2])
        y1t = net(xd[1:2], torch.tensor([1.0], device="cuda"), cd[1:2], ad[1:2])
    e32, e3, e16 = rel_l2(y32.cpu(), ref), rel_l2(y3.cpu(), ref), rel_l2(y16.cpu(), ref)
    print(f"EDMPrecond vs restatement: fp32 {e32:.3e}  bf16x3 {e3:.3e}  bf16 {e16:.3e}")
    assert e32 < FP32_TOL and e3 < FP32_TOL and e16 < BF16_TOL
    for b in range(B):  # per sample: sigma 0.03 (D ~ x), 1, 80 (D ~ sd F)
        assert rel_l2(y32[b].cpu(), ref[b]) < FP32_TOL, b
    assert torch.equal(y16, y16b)
    assert rel_l2(y1.cpu(), y32[1:2].cpu()) < 1e-6 and rel_l2(y1t.cpu(), y32[1:2].cpu()) < 1e-6


@pytest.mark.parametrize("dtype,tol", [(torch.float32, FP32_TOL), (torch.bfloat16, BF16_TOL)])
def test_edm_sampler_vs_restatement(nets, dtype, tol, monkeypatch):
    from swift_amd.engine import SwinEngine
    from swift_amd.generating.factory import sampler_factory
    net, onet, _ = nets
    B, N = 2, 4
    cond, lat = det_normal((B, 72, 64, 64), 52, "cond"), det_normal((B, 69, 64, 64), 52, "lat")
    ren = [det_normal((B, 69, 64, 64), 52, f"ren{i}") for i in range(N)]
    kw = dict(num_steps=N, sigma_min=0.03, sigma_max=80.0, rho=7, S_churn=2.5, S_min=0.75, S_max=80, S_noise=1.05, auxiliary=0.6)
    calls = []
    fwd = SwinEngine.forward
    monkeypatch.setattr(SwinEngine, "forward", lambda self, *a, **k: calls.append(1) or fwd(self, *a, **k))
    it = iter(ren)
    smp = sampler_factory("edm", net, denoise_dtype=dtype, randn_like=lambda like: next(it).to(like), **kw)
    y = smp(cond.cuda(), latents=lat.cuda())
    assert len(calls) == 2 * N - 1
    it = iter(ren)
    ref = er.edm_sampler(onet, lat, cond, 0.6, randn_like=lambda like: next(it), grid_dtype=dtype,  # (bf16: the reference's bf16 grid)
                         **{k: v for k, v in kw.items() if k != "auxiliary"})
    e = rel_l2(y.cpu(), ref)
    print(f"edm_sampler N={N} churn 2.5 {dtype}: rel-L2 {e:.3e}")
    assert e < tol * 3


def test_edm_loss_and_grads_vs_restatement():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from swift_amd.training.loss import EDMLoss
    from swift_amd.training.trainer import GradAllReduce
    net, onet, st = _build(53, clamp_scale=True)
    net.train()
    ds = _dataset(53)
    L = EDMLoss(ds, dict(dist="lognormal", P_mean=-0.2, P_std=2.2), sigma_data=SD).to("cuda")
    B = 4
    x, cond, z = det_normal((B, 69, 64, 64), 53, "x"), det_normal((B, 72, 64, 64), 53, "c"), det_normal((B, 69, 64, 64), 53, "z")
    sigma, aux = torch.tensor([0.01, 0.3, 4.0, 60.0]).view(B, 1, 1, 1), torch.tensor([0.6] * B)
    ddp = GradAllReduce(net)
    ddp.zero_grad_flat()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = L(ddp, x.cuda(), condition=cond.cuda(), auxiliary=aux.cuda(), _sigma=sigma.cuda(), _z=z.cuda())
    loss.backward()
    ref = er.edm_loss(onet, x, sigma, z, L.w_var.cpu(), L.w_lat.cpu(), SD, condition=cond, auxiliary=aux)
    ref.backward()
    print(f"EDM loss {float(loss):.6f} vs restatement {float(ref):.6f}; worst grad cosine {_grad_report(net, st):.4f}")
    assert float(loss) == pytest.approx(float(ref.detach()), rel=1e-3)


def test_edm_forecast_unit_alone_vs_in_a_batch(nets):
    """Counter-stream churn: unit (member 0, IC 2)'s EDM forecast is the same alone and as row 2 of a batch of 4."""
    from swift_amd.data.era5 import SyntheticERA5Dataset
    from swift_amd.rollout import RolloutEngine, unit_seed
    net, _, _ = nets
    ds = SyntheticERA5Dataset([f"v{i}" for i in range(69)], ["f0", "f1", "f2"], img_resolution=(64, 64), length=16, seed=54)
    eng = RolloutEngine(net, ds, interval=6, solver="edm", denoise_dtype=torch.float32, num_steps=3, sigma_min=0.03,
                        sigma_max=80.0, rho=7, S_churn=2.5, S_min=0.75, S_max=80, S_noise=1.05)
    assert eng.renoises
    X0 = det_normal((4, 69, 64, 64), 54, "X0").cuda()
    forc = det_normal((2, 4, 3, 64, 64), 54, "f").cuda()
    seeds = [unit_seed(0, i) for i in range(4)]
    batch = eng.run(X0, forc, 2, seeds=seeds, keep_trajectory=False)
    alone = eng.run(X0[2:3].contiguous(), forc[:, 2:3].contiguous(), 2, seeds=seeds[2:3], keep_trajectory=False)
    e = rel_l2(alone.cpu(), batch[2:3].cpu())
    print(f"EDM forecast (fp32 engine), unit alone vs in a batch of 4: rel-L2 {e:.3e}")
    assert e < 1e-6  # the fp32 bound of test_bf16_engine_unit_alone_vs_in_a_batch
    other = eng.run(X0[2:3].contiguous(), forc[:, 2:3].contiguous(), 2, seeds=[unit_seed(1, 2)], keep_trajectory=False)
    assert rel_l2(other.cpu(), alone.cpu()) > 1e-3  # (another member's churn and latents: a different forecast)
    with pytest.raises(ValueError, match="one-step samplers"):
        eng.capture_step(X0, forc[0], torch.empty_like(X0), torch.empty_like(X0), seeds=torch.tensor(seeds, device="cuda"),
                         step=torch.zeros((), dtype=torch.int64, device="cuda"))


def test_edm_train_validate_generate_cli(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from test_gpu_cli import run
    small = ["data=era5-synthetic-1.4", "data.dataset.img_resolution=[64,64]", "data.dataset.length=48", "data.data_workers=0",
             "model.depth=2", "trainer.total_kimg=0.008", "trainer.kimg_per_tick=0.004", "trainer.checkpoint_ticks=1",
             "trainer.lr_rampup_kimg=0", "trainer.val_ticks=1", "trainer.val_target_interval=4", "data.val_local_batch_size=2",
             "data.batch_size=2", "solver.num_steps=3"]
    out = run(["swift_amd.train", "experiment=era5-swinv2-1.4-edm", "model.heads=12"] + small, cwd=str(tmp_path))
    assert "in-training validation: solver edm" in out, out[-2000:]
    import json
    rdir = tmp_path / "results" / "era5-swinv2-1.4-edm" / "000"
    lines = [json.loads(l) for l in open(rdir / "stats.jsonl")]
    assert lines and all(torch.isfinite(torch.tensor(l["train/loss"])) for l in lines)
    val = [json.loads(l) for l in open(rdir / "val_stats.jsonl")]
    assert val and torch.isfinite(torch.tensor(val[0]["val/rmse"]))
    out = run(["swift_amd.generate", "--input", str(rdir), "--members", "2", "--steps", "2", "--samples", "2", "--batch", "4",
               "--num-steps", "3"], cwd=str(tmp_path))
    assert os.path.isdir(rdir / "output" / "latest"), out[-2000:]
    assert any(n.endswith(".zarr") for n in os.listdir(rdir / "output" / "latest"))
    import subprocess
    import sys
    p = subprocess.run([sys.executable, "-m", "swift_amd.train", "experiment=era5-swinv2-1.4-edm"] + small, cwd=str(tmp_path),
                       env=dict(os.environ, PYTHONPATH=ROOT, HYDRA_RUN_ID="001"), capture_output=True, text=True, timeout=600)
    assert p.returncode != 0 and "head_dim" in p.stderr and "66" in p.stderr, p.stderr[-2000:]
