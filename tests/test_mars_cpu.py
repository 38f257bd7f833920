"""MARS (swift_amd/training/optimizers/mars.py) against the reference's own MARS inside its Trainer._backward_step
(tests/golden/mars_tiny.npz, tools/make_golden.py::fx_mars_tiny): four steps over warm-up, cosine and final learning rates,
NaN / +-inf gradients, ||c_t|| on both sides of 1, three configurations (mars-adamw, mars-lion, mars-adamw with optimize_1d),
two param groups.  Bar: rel-L2 < 2e-6 on parameters and EMA, the bar of the host-path trainer test -- fp32 CPU against fp32 CPU
with another op order stays near 3e-8 here, so a wrong formula (1e-3 and up) cannot hide and rounding cannot trip it.
"""
import ctypes
import io
import os

import pytest
import torch

from conftest import ROOT, load_golden, rel_l2

TOL = 2e-6
CONFIGS = {"adamw": dict(mars_type="mars-adamw"), "lion": dict(mars_type="mars-lion"),
           "adamw1d": dict(mars_type="mars-adamw", optimize_1d=True)}
_G = {}


def fixture():
    if not _G:
        g = load_golden("mars_tiny")
        _G.update(g=g, names=[str(n) for n in g["names"]], no_decay=set(int(i) for i in g["no_decay"]))
        assert [str(c) for c in g["configs"]] == list(CONFIGS)
    return _G["g"], _G["names"], _G["no_decay"]


def grads(cfg, k):
    g, names, _ = fixture()
    return [torch.from_numpy(g.get(f"{cfg}_g{k}_{n}", g[f"g{k}_{n}"])) for n in names]


def build(cfg, device):
    """Parameters, their EMA start and the optimizer, grouped as the fixture's generator groups them."""
    from swift_amd.training.optimizers.mars import MARS
    g, names, no_decay = fixture()
    net = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(g[f"p0_{n}"]).clone()) for n in names]).to(device)
    params = list(net.parameters())
    opt = MARS([{"params": [p for i, p in enumerate(params) if i not in no_decay], "weight_decay": 0.05},
                {"params": [params[i] for i in sorted(no_decay)], "weight_decay": 0.0, "lr": 1e-3}],
               lr=2e-3, lr_1d=3e-3, weight_decay_1d=0.1, **CONFIGS[cfg])
    return net, params, opt


def make_trainer(cfg, device, ckpt=None):
    from swift_amd.training.trainer import Trainer
    g, names, _ = fixture()
    net, params, opt = build(cfg, device)
    cur = {}
    loss_fn = lambda ddp, t, condition=None, auxiliary=None, **kw: sum((p * cur["G"][i].to(p.device)).sum() for i, p in enumerate(params))
    tr = Trainer(net, opt, loss_fn, total_kimg=0.02, ema_halflife_kimg=0.5, ema_rampup_ratio=0.05, lr_rampup_kimg=0.004,
                 lr_min_factor=0.01, lr_cosine_anneal=True, kimg_per_tick=1, checkpoint_ticks=None, device=device, ckpt=ckpt)
    tr.global_batch_size = 2
    if ckpt is None:
        with torch.no_grad():
            for e, n in zip(tr.ema.parameters(), names):
                e.copy_(torch.from_numpy(g[f"e0_{n}"]))
    return tr, params, opt, cur


def trainer_step(tr, cur, cfg, k):
    g = fixture()[0]
    cur["G"] = grads(cfg, k)
    tr.train_step(None, None, None, None, int(g["nimgs"][k]))


def worst_vs_golden(cfg, k, params, ema_params):
    """Largest rel-L2 of the parameters (and the EMA, where the fixture holds it) after step k (0-based)."""
    g, names, _ = fixture()
    worst = max(rel_l2(p.detach().cpu(), g[f"{cfg}_p{k + 1}_{n}"]) for p, n in zip(params, names))
    if f"{cfg}_e{k + 1}_{names[0]}" in g:
        worst = max(worst, max(rel_l2(e.detach().cpu(), g[f"{cfg}_e{k + 1}_{n}"]) for e, n in zip(ema_params, names)))
    return worst


def run_trainer_on_fixture(cfg, device):
    """swift_amd's Trainer.train_step driven with the fixture's gradients (a loss linear in the parameters)."""
    g = fixture()[0]
    tr, params, opt, cur = make_trainer(cfg, device)
    worst = 0.0
    for k in range(len(g["nimgs"])):
        trainer_step(tr, cur, cfg, k)
        assert [gr["lr"] for gr in opt.param_groups] == pytest.approx(list(g[f"{cfg}_lr_{k}"]), rel=1e-12)
        worst = max(worst, worst_vs_golden(cfg, k, params, list(tr.ema.parameters())))
    return tr, worst


def test_fixture_covers_both_norm_branches_away_from_one():
    g, names, _ = fixture()
    for cfg in CONFIGS:
        norms = [float(v) for k, v in g.items() if k.startswith(f"{cfg}_norm")]
        assert len(norms) == (28 if cfg == "adamw1d" else 16)  # 4 steps x (7 tensors | 4 matrices)
        assert any(v > 1.0 for v in norms) and any(v < 1.0 for v in norms)
        assert all(abs(v - 1.0) > 0.05 for v in norms)
    assert "adamw_norm0_model.pos_embed" not in g and "adamw1d_norm0_model.pos_embed" in g  # 3-D: the AdamW-1d rule


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_optimizer_class_vs_reference_golden(cfg):
    """The class driven directly: fresh gradient tensors every step, the fixture's learning rates written into the groups."""
    g, names, _ = fixture()
    net, params, opt = build(cfg, torch.device("cpu"))
    worst = 0.0
    for k in range(len(g["nimgs"])):
        for gr, lr in zip(opt.param_groups, g[f"{cfg}_lr_{k}"]):
            gr["lr"] = float(lr)
        for p, gk in zip(params, grads(cfg, k)):
            p.grad = torch.nan_to_num(gk, nan=0, posinf=1e5, neginf=-1e5)
        opt.step()
        worst = max(worst, max(rel_l2(p.detach(), g[f"{cfg}_p{k + 1}_{n}"]) for p, n in zip(params, names)))
    print(f"{cfg}: MARS class vs reference golden: worst rel-L2 {worst:.3e}")
    assert worst < TOL
    for p, n in zip(params, names):
        assert rel_l2(opt.state[p]["exp_avg"], g[f"{cfg}_m4_{n}"]) < TOL
        if cfg == "adamw":
            assert rel_l2(opt.state[p]["exp_avg_sq"], g[f"{cfg}_v4_{n}"]) < TOL
        assert torch.equal(opt.state[p]["last_grad"], p.grad) and opt.state[p]["last_grad"].data_ptr() != p.grad.data_ptr()
    assert opt.step_num == 4


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_trainer_flat_gradient_path_vs_reference_golden(cfg):
    """Trainer.train_step on CPU: every param.grad is a view of one flat buffer that is cleared in place and overwritten by
    the next backward pass.  A last_grad that aliased the gradient would equal the current gradient (c_t = g): this case is
    the one that catches it."""
    tr, worst = run_trainer_on_fixture(cfg, torch.device("cpu"))
    print(f"{cfg}: Trainer host path vs reference golden: worst rel-L2 {worst:.3e}")
    assert tr._fused is False and worst < TOL


def test_constructor_contract_and_validation():
    from swift_amd.training.optimizers.mars import MARS
    g = fixture()[0]
    p = [torch.nn.Parameter(torch.zeros(3, 2))]
    opt = MARS(p)
    grp = opt.param_groups[0]
    assert (grp["lr"], grp["betas"], grp["eps"], grp["weight_decay"], grp["amsgrad"], grp["gamma"], grp["mars_type"],
            grp["optimize_1d"], grp["weight_decay_1d"]) == (3e-3, (0.95, 0.99), 1e-8, 0.0, False, 0.025, "mars-adamw", False, 0.1)
    assert opt.is_approx is True and opt.betas_1d == (0.9, 0.95) and opt.lr_1d_factor == 1.0
    assert sorted(k for k in grp if k != "params") == [str(k) for k in g["adamw_group_keys"]]  # the keys the reference writes
    assert MARS(p, lr=1e-3, lr_1d=3e-3).lr_1d_factor == pytest.approx(3.0)
    for bad in (dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(1.0, 0.99)), dict(betas=(0.9, -0.1))):
        with pytest.raises(ValueError):
            MARS(p, **bad)
    with pytest.raises(AssertionError):
        MARS(p, mars_type="mars-sgd")


def test_state_dict_round_trip_with_the_reference_keys():
    """state_dict() carries the reference's per-parameter keys; loaded into a fresh optimizer (through a serialised file, as a
    checkpoint does) the next step equals the uninterrupted run bit for bit -- last_grad included, and a reference-style state
    whose step is a Python int and whose tensors are separate allocations loads the same way."""
    g, names, _ = fixture()
    cfg = "adamw"
    net, params, opt = build(cfg, torch.device("cpu"))

    def step(o, ps, k):
        for gr, lr in zip(o.param_groups, g[f"{cfg}_lr_{k}"]):
            gr["lr"] = float(lr)
        for p, gk in zip(ps, grads(cfg, k)):
            p.grad = torch.nan_to_num(gk, nan=0, posinf=1e5, neginf=-1e5)
        o.step()

    for k in range(3):
        step(opt, params, k)
    sd = opt.state_dict()
    assert sorted(sd["state"][0]) == [str(k) for k in g["adamw_state_keys"]] == ["exp_avg", "exp_avg_sq", "last_grad", "step"]
    assert sd["state"][0]["step"] == 3 and len(sd["state"]) == len(names)
    buf = io.BytesIO()
    torch.save({"optimizer": sd, "net": net.state_dict()}, buf)
    buf.seek(0)
    state = torch.load(buf, weights_only=True)
    net2, params2, opt2 = build(cfg, torch.device("cpu"))
    net2.load_state_dict(state["net"])
    opt2.load_state_dict(state["optimizer"])
    step(opt, params, 3)
    step(opt2, params2, 3)
    for p, q, n in zip(params, params2, names):
        assert torch.equal(p, q), n
        assert rel_l2(q.detach(), g[f"{cfg}_p4_{n}"]) < TOL
    # amsgrad adds max_exp_avg_sq, as the reference does
    from swift_amd.training.optimizers.mars import MARS
    w = torch.nn.Parameter(torch.ones(4, 3))
    o = MARS([w], amsgrad=True)
    w.grad = torch.full((4, 3), 0.01)
    o.step()
    assert sorted(o.state[w]) == ["exp_avg", "exp_avg_sq", "last_grad", "max_exp_avg_sq", "step"]


def test_exact_form_keeps_previous_grad_in_plain_torch():
    from swift_amd.training.optimizers.mars import MARS
    w = torch.nn.Parameter(torch.ones(4, 3))
    o = MARS([w], is_approx=False)
    w.grad = torch.full((4, 3), 0.25)
    o.update_previous_grad()
    w.grad = torch.full((4, 3), 0.5)
    o.step()
    assert float(o.state[w]["last_grad"].abs().max()) == 0.0  # the exact form does not take the step's own gradient
    o.update_last_grad()
    assert torch.equal(o.state[w]["last_grad"], torch.full((4, 3), 0.25))


def test_mars_shampoo_runs_in_plain_torch():
    from swift_amd.training.optimizers.mars import MARS
    torch.manual_seed(0)
    w, b = torch.nn.Parameter(torch.randn(12, 8) * 0.1), torch.nn.Parameter(torch.zeros(8))
    o = MARS([w, b], mars_type="mars-shampoo", lr=1e-2)
    w0 = w.detach().clone()
    w.grad, b.grad = torch.randn(12, 8), torch.randn(8)
    o.step()
    d = (w.detach() - w0) / -1e-2
    # a Newton-Schulz step direction: singular values near 1 (0.5 .. 1.5 after five quintic iterations), times sqrt(12 / 8)
    s = torch.linalg.svdvals(d.double()) / (12 / 8) ** 0.5
    assert 0.4 < float(s.min()) and float(s.max()) < 1.6
    assert torch.isfinite(b).all() and float(b.detach().abs().max()) > 0


def test_optimizer_mars_composes_and_instantiates():
    from swift_amd.config import compose, instantiate
    from swift_amd.training.optimizers.mars import MARS
    cfg = compose(os.path.join(ROOT, "swift_amd", "configs"), "train", ["optimizer=mars"])
    assert cfg.optimizer._target_ == "swift.training.optimizers.mars.MARS"
    assert (cfg.optimizer.mars_type, cfg.optimizer.lr, cfg.optimizer.lr_1d, cfg.optimizer.weight_decay) == ("mars-adamw", 1e-3, 1e-3, 0.1)
    net = torch.nn.Linear(4, 3)
    opt = instantiate(cfg.optimizer, net.parameters(), _convert_="object")  # what swift_amd/train.py does for this target
    assert type(opt) is MARS and len(opt.param_groups) == 1 and len(opt.param_groups[0]["params"]) == 2
    assert opt.param_groups[0]["weight_decay"] == 0.1 and opt.lr_1d_factor == 1.0


def test_fused_step_is_not_offered_off_device_or_for_uncovered_variants():
    from swift_amd.training import fused_optim
    from swift_amd.training.optimizers.mars import MARS
    p = [torch.nn.Parameter(torch.zeros(3, 2))]
    assert not fused_optim.supported(MARS(p))  # CPU parameters
    assert not fused_optim._mars_supported(MARS(p, mars_type="mars-shampoo"))
    assert not fused_optim._mars_supported(MARS(p, is_approx=False))


def test_mars_ema_step_argument_validation_needs_no_gpu():
    """Error conventions of the C ABI: SWIFTK_EINVAL (-1) before anything is launched."""
    from swift_amd import _lib
    L = _lib.lib()
    h = _lib.MarsHyper()
    h.mars_type, h.n_groups = _lib.MARS_ADAMW, 1
    ok = (16, 1, 16, 16, 16, 16, 16, None)  # table, n_chunks, grad, exp_avg, exp_avg_sq, last_grad, partials, tensor_norms
    call = lambda a, hh=h: L.swiftk_mars_ema_step(*a, ctypes.byref(hh), None)
    assert call((None,) + ok[1:]) == -1                     # null table
    assert call(ok[:1] + (0,) + ok[2:]) == -1               # n_chunks <= 0
    assert call(ok[:1] + (-3,) + ok[2:]) == -1
    for i in (2, 3, 4, 5, 6):                               # null flat buffer / scratch
        assert call(ok[:i] + (None,) + ok[i + 1:]) == -1
    assert L.swiftk_mars_ema_step(*ok, None, None) == -1    # null hyper
    for groups in (0, -1, _lib.OPT_MAX_GROUPS + 1):         # group count (hence every group index) out of range
        hb = _lib.MarsHyper()
        hb.mars_type, hb.n_groups = _lib.MARS_LION, groups
        assert call(ok, hb) == -1
    for kind in (-1, 2, 7):                                 # a mars type outside the two (mars-shampoo has no kernel)
        hb = _lib.MarsHyper()
        hb.mars_type, hb.n_groups = kind, 1
        assert call(ok, hb) == -1
    assert call(ok[:2] + (20,) + ok[3:]) == -3              # a flat buffer off the 16-byte boundary: SWIFTK_EALIGN
    assert ctypes.sizeof(_lib.MarsChunk) == 48 and ctypes.sizeof(_lib.MarsHyper) == 4 * (3 * _lib.OPT_MAX_GROUPS + 18)
