"""-m gpu: swiftk_mars_ema_step (two launches: per-chunk sums of squares of c_t, then moments / update / EMA / last_grad) driven
by FusedMarsEMA -- inside Trainer.train_step against the reference's own run (tests/golden/mars_tiny.npz), and on multi-chunk
tensors against the torch-op MARS class on the same device tensors and gradients.

Bars: rel-L2 < 3e-6 against the golden, the fused AdamW test's bar (fp32 device arithmetic with fused multiply-adds and
1 / norm as a factor against fp32 CPU ops).  The kernel's norm against a float64 norm of the same c_t: 1e-5 -- each thread adds
<= 64 squares serially, then 6 butterfly levels, 2 wave sums and <= 2 + 9 levels over the tensor's partials: fewer than 90
roundings of 6e-8 on a sum of non-negative terms bound the relative error by 5.4e-6, halved by the square root, plus two
roundings in c_t itself.
"""
import pytest
import torch

from conftest import rel_l2
from test_mars_cpu import CONFIGS, fixture, make_trainer, run_trainer_on_fixture, trainer_step, worst_vs_golden

pytestmark = pytest.mark.gpu
TOL = 3e-6
NORM_TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_trainer_step_fused_mars_vs_reference_golden(dev, cfg):
    from swift_amd.training.fused_optim import FusedMarsEMA
    g, names, _ = fixture()
    tr, worst = run_trainer_on_fixture(cfg, dev)
    print(f"{cfg}: fused MARS step vs reference golden: worst rel-L2 {worst:.3e}")
    assert isinstance(tr._fused, FusedMarsEMA)
    assert worst < TOL
    norms = tr._fused.norms.cpu()
    for i, n in enumerate(names):  # the last step's ||c_t|| per tensor, 0 where the AdamW-1d rule applied
        key = f"{cfg}_norm3_{n}"
        if key in g:
            assert float(norms[i]) == pytest.approx(float(g[key]), rel=NORM_TOL), n
        else:
            assert float(norms[i]) == 0.0, n
    sd = tr.optimizer.state_dict()
    assert len(sd["state"]) == len(names) and float(sd["state"][0]["step"]) == 4.0
    assert sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "last_grad", "step"]
    for p, n in zip(tr.net.parameters(), names):
        st = tr.optimizer.state[p]
        assert rel_l2(st["exp_avg"].cpu(), g[f"{cfg}_m4_{n}"]) < TOL, n
        if cfg == "adamw":
            assert rel_l2(st["exp_avg_sq"].cpu(), g[f"{cfg}_v4_{n}"]) < TOL, n
        assert torch.equal(st["last_grad"], p.grad) and st["last_grad"].data_ptr() != p.grad.data_ptr()


def test_multi_chunk_step_vs_torch_op_class_without_host_sync(dev):
    """363 chunks in one tensor (5632 x 1056), an element count that is a multiple of neither 4 nor 16384 (3413 x 1279: the last
    chunk ends in a dword tail), a small matrix behind it whose flat offset is off the 16-byte boundary (dword path) and a 1-D
    tensor (AdamW-1d rule).  Step 1 has ||c_t|| below 1 on the large tensors, step 2 above.  The fused step runs under
    set_sync_debug_mode("error"); two runs from equal state are bit-equal.  mars-adamw only: among 10 M random first moments some
    lie within a rounding error of zero, where mars-lion's sign is not determined (one flipped sign moves a parameter by 2 lr);
    the golden case above covers mars-lion on a fixture generated without such entries."""
    kind = "mars-adamw"
    from swift_amd.training.fused_optim import FusedMarsEMA
    from swift_amd.training.optimizers.mars import MARS
    shapes = [(5632, 1056), (1056,), (3413, 1279), (33, 7)]
    gen = torch.Generator(device=dev).manual_seed(5)
    rnd = lambda sh, std: torch.randn(sh, generator=gen, device=dev) * std
    P = [torch.nn.Parameter(rnd(sh, 0.05)) for sh in shapes]
    E = [p.detach().clone() + 0.01 for p in P]
    Pr = [torch.nn.Parameter(p.detach().clone()) for p in P]
    Er = [e.clone() for e in E]
    kw = dict(lr=2e-3, lr_1d=3e-3, weight_decay=0.05, mars_type=kind)
    opt, ref = MARS(P, **kw), MARS(Pr, **kw)
    flat = torch.zeros(sum(p.numel() for p in P), device=dev)
    o = 0
    for p in P:
        p.grad = flat[o:o + p.numel()].view_as(p)
        o += p.numel()
    fused = FusedMarsEMA(opt, P, E, flat)
    assert fused.n_chunks == 363 + 1 + 267 + 1 and fused.rules == [0, 1, 0, 0]
    k = 0.025 * (0.95 / 0.05)
    ema_beta = (0.3, 0.9)  # both sides of torch's two-sided lerp formula
    for step, std in enumerate((1e-4, 1e-2)):
        G = [rnd(sh, std) for sh in shapes]
        if step == 1:
            G[0].view(-1)[16384 * 200 + 5] = float("nan")
            G[2].view(-1)[-2] = float("inf")     # in the dword tail
            G[3].view(-1)[4] = float("-inf")
            G[1][7] = float("nan")
        for p, gk in zip(P, G):
            p.grad.copy_(gk)
        Gs = [torch.nan_to_num(gk, nan=0, posinf=1e5, neginf=-1e5) for gk in G]
        want_norm = [float((gs.double() + k * (gs.double() - opt.state[p]["last_grad"].double())).norm())
                     for gs, p in zip(Gs, P)]
        keep = [t.clone() for t in (flat, fused.m, fused.v, fused.last, *[p.detach() for p in P], *E)]
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            fused.step(ema_beta[step])
        finally:
            torch.cuda.set_sync_debug_mode("default")
        first = [t.clone() for t in (flat, fused.m, fused.v, fused.last, *[p.detach() for p in P], *E)]
        # the same step again from the same state: bit-equal (fixed summation order, no atomics)
        with torch.no_grad():
            for t, s in zip((flat, fused.m, fused.v, fused.last, *P, *E), keep):
                t.copy_(s)
        fused.step_t -= 1
        fused.step(ema_beta[step])
        for a, b in zip(first, (flat, fused.m, fused.v, fused.last, *P, *E)):
            assert torch.equal(a, b.detach())
        assert torch.equal(flat, torch.cat([gs.flatten() for gs in Gs]))  # sanitised in place
        norms = fused.norms.cpu()
        for i, sh in enumerate(shapes):
            if len(sh) == 2:
                print(f"{kind} step {step + 1} {sh}: ||c_t|| kernel {float(norms[i]):.7e}, float64 {want_norm[i]:.7e}")
                assert float(norms[i]) == pytest.approx(want_norm[i], rel=NORM_TOL)
        assert (want_norm[0] < 1.0 and want_norm[2] < 1.0) if step == 0 else (want_norm[0] > 1.0 and want_norm[2] > 1.0)
        # the torch-op class (the reference's sequence) on copies of the same tensors and the same gradients
        for p, gs in zip(Pr, Gs):
            p.grad = gs.clone()
        ref.step()
        with torch.no_grad():
            for e, p in zip(Er, Pr):
                e.copy_(p.detach().lerp(e, ema_beta[step]))
        for i, (p, pr, e, er) in enumerate(zip(P, Pr, E, Er)):
            errs = {"p": rel_l2(p.detach(), pr.detach()), "ema": rel_l2(e, er),
                    "exp_avg": rel_l2(opt.state[p]["exp_avg"], ref.state[pr]["exp_avg"])}
            if kind == "mars-adamw" or fused.rules[i]:
                errs["exp_avg_sq"] = rel_l2(opt.state[p]["exp_avg_sq"], ref.state[pr]["exp_avg_sq"])
            else:
                assert float(opt.state[p]["exp_avg_sq"].abs().max()) == 0.0  # lion leaves the second moment alone
            assert torch.equal(opt.state[p]["last_grad"], ref.state[pr]["last_grad"])
            print(f"{kind} step {step + 1} {shapes[i]}: " + ", ".join(f"{a} {b:.2e}" for a, b in errs.items()))
            assert max(errs.values()) < TOL, (step, shapes[i], errs)
        assert all(p._version > 0 for p in P)  # the engines' operand copies key on (data_ptr, _version)


def test_checkpoint_round_trip_continues_bit_equal(dev, tmp_path, monkeypatch):
    """Three steps, a checkpoint through Trainer._save_checkpoint, a fourth step; a second trainer resumed from that file
    (loaded moments and last_grad adopted into the flat buffers) takes the same fourth step."""
    import os
    from swift_amd.training.fused_optim import FusedMarsEMA
    cfg = "adamw"
    monkeypatch.chdir(tmp_path)
    tr, params, opt, cur = make_trainer(cfg, dev)
    for k in range(3):
        trainer_step(tr, cur, cfg, k)
    tr._save_checkpoint(3000)
    trainer_step(tr, cur, cfg, 3)
    tr2, params2, opt2, cur2 = make_trainer(cfg, dev, ckpt=os.path.join(str(tmp_path), "checkpoints", "checkpoint-000003.pt"))
    trainer_step(tr2, cur2, cfg, 3)
    assert isinstance(tr2._fused, FusedMarsEMA) and float(tr2._fused.step_t) == 4.0
    for a, b in zip(list(params) + list(tr.ema.parameters()), list(params2) + list(tr2.ema.parameters())):
        assert torch.equal(a.detach(), b.detach())
    for p, q in zip(params, params2):
        for key in ("exp_avg", "exp_avg_sq", "last_grad"):
            assert torch.equal(opt.state[p][key], opt2.state[q][key]), key
    assert worst_vs_golden(cfg, 3, params2, list(tr2.ema.parameters())) < TOL
