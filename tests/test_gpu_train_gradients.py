"""-m gpu: end-to-end training gradients, slice by slice against fp64 autograd of the CPU oracle (tests/gradient_reference.py).

What is scored is the COMPOSITION every kernel-level backward test leaves out: SwinTrainEngine.backward, the flat gradient
buffer of GradAllReduce, the tangent-then-backward path of SCMLoss, the recompute / resident walk of CRPSLoss and the padded
head lanes.  Each case runs the SMALLB net (64x64 image, 32x32 token grid, four 16x16 windows, one layer shifted, dim 1056,
depth 2) -- the smallest shape the kernels run -- and holds every natural slice of every parameter gradient (and of every
requested input gradient) to 2 x the worst slice of the oracle's own two bf16 emulations, all measured against fp64 in the
test.  The whole-tensor cosine checks of test_gpu_train.py stay as they are; tests/test_gradient_reference_cpu.py shows what
they cannot see."""
import pytest
import torch

import gradient_reference as gr

pytestmark = pytest.mark.gpu
NV, NF = gr.SMALLB["n_vars"], gr.SMALLB["n_forc"]
# Seeds: 21 is the issue's engine-level configuration; the loss cases take the seed of the test_gpu_train.py case on the same
# path (31, 42), or the next one at which the fp64 truth meets score()'s condition that at most one slice per slicing lies
# under the floor (CRPS 33, padded lanes 62: with every scale clamped to 0.5 the per-head scale gradients scatter around zero,
# and two of them under a tenth of the median is a property of the operands, decided on the CPU before any kernel runs).
_refs = {}   # oracle runs shared by the cases that differ only in how the engine walks (one-pass / two-pass, resident / recomputed)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _net(dev, kind, seed, logvar=True, heads=None):
    from swift_amd.models.precond import PassPrecond
    cfg, mcfg, state = gr.small_net(kind, seed, logvar=logvar, heads=heads)
    net = PassPrecond(mcfg, img_resolution=[64, 64], img_channels=NV, condition_channels=NV + NF, auxiliary_dim=1)
    net.load_state_dict(state)
    return net.to(dev), cfg, state


def _param_grads(net):
    torch.cuda.synchronize()
    return {k: p.grad.detach().float().cpu().clone() for k, p in net.named_parameters()}


def _hold(title, got, ref, cfg, smooth, unguarded=()):
    """Score, print, assert: every slicing's worst slice within its bound; on a smooth net every bound but the per-head
    scales' (and those of the ``unguarded`` (name suffix, slicing) pairs, which the caller has to justify) is itself under 3e-2,
    so a change to the oracle cannot quietly loosen the test."""
    truth, ya, yb = ref
    assert set(got) == set(truth), set(got) ^ set(truth)
    recs = gr.score_all(got, truth, ya, yb, cfg, title=title)
    if smooth:
        loose = [(r["name"], r["slicing"], r["bound"]) for r in recs if not r["name"].endswith(".scale") and not r["bound"] < 3e-2
                 and not any(r["name"].endswith(n) and r["slicing"] == sl for n, sl in unguarded)]
        assert not loose, loose
    bad = [(r["name"], r["slicing"], r["index"], f"{r['worst']:.3e} > {r['bound']:.3e}") for r in gr.over(recs)]
    assert not bad, bad
    return recs


# --------------------------------------------------------------------------- 1. the engine itself


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("kind", list(gr.NETS))
def test_engine_backward_slices_vs_fp64(dev, kind, B):
    """SwinTrainEngine.forward / .backward called directly (want_logvar, input gradients of x and of the condition's state
    channels), every sample with its own t and aux.  On the default net the heads beyond the ln 100 clamp have a scale
    gradient of exactly 0."""
    from swift_amd.train_engine import SwinTrainEngine
    net, cfg, state = _net(dev, kind, 21)
    ins, loss_fn = gr.engine_case(B)
    ref = gr.oracle_gradients(cfg, state, NV, NV + NF, loss_fn, ins, wrt=("x", "cond"))
    for g in ref:
        g[gr.INPUT + "cond"] = g[gr.INPUT + "cond"][:, :NV]   # the forcing channels' gradient is not requested
    x, cond = ins["x"].to(dev), ins["cond"].to(dev)
    eng = SwinTrainEngine(net.model)
    out, lv, ctx = eng.forward([x, cond[:, :NV].contiguous(), cond[:, NV:].contiguous()], [1.0, 1.0, 1.0], ins["t"].to(dev),
                               ins["aux"].to(dev), want_logvar=True)
    dins = eng.backward(ctx, ins["R"].to(dev), ins["rl"].to(dev), need_input_grad=(True, True, False))
    assert dins[2] is None
    got = _param_grads(net)
    got[gr.INPUT + "x"], got[gr.INPUT + "cond"] = dins[0].float().cpu(), dins[1].float().cpu()
    _hold(f"engine backward, {kind} net, B = {B}", got, ref, cfg, kind == "smooth")
    if kind == "default":
        for i in range(cfg.depth):
            k, h = f"model.transformer.layers.{i}.0.scale", (i + 1) % cfg.heads
            assert float(state[k].reshape(-1)[h]) > 4.61 and float(got[k].reshape(-1)[h]) == 0.0


# --------------------------------------------------------------------------- 2. TrigFlowLoss through the flat buffer


def _trigflow_case(seed, B=2):
    from swift_amd.utils.detinit import det_normal
    ins = dict(x=det_normal((B, NV, 64, 64), seed, "x"), cond=det_normal((B, NV + NF, 64, 64), seed, "c"),
               z=det_normal((B, NV, 64, 64), seed, "z"), tau=torch.tensor([0.3, 4.0]).view(B, 1, 1, 1), aux=torch.tensor([0.6, 1.2]))
    return ins


def _trigflow_ref(cfg, state, ins, L):
    from oracle import loss as oloss
    ins = dict(ins, w_var=L.w_var.cpu(), w_lat=L.w_lat.cpu())
    f = lambda onet, i: oloss.trigflow_loss(onet, i["x"], i["tau"], i["z"], i["w_var"], i["w_lat"], 1.0, condition=i["cond"],
                                            auxiliary=i["aux"], return_logvar=True)
    return gr.oracle_gradients(cfg, state, NV, NV + NF, f, ins)


def _trigflow_step(L, ddp, ins, dev):
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = L(ddp, ins["x"].to(dev), condition=ins["cond"].to(dev), auxiliary=ins["aux"].to(dev), _tau=ins["tau"].to(dev),
                 _z=ins["z"].to(dev))
    loss.backward()
    return float(loss)


def test_trigflow_through_flat_buffer_slices_and_accumulation(dev):
    """TrigFlowLoss -> GradAllReduce's flat buffer, smooth net; then a second forward + backward WITHOUT zero_grad_flat():
    the buffer must hold 2 x the first gradients to fp32 rounding (the backward accumulates, it does not overwrite)."""
    from swift_amd.training.loss import TrigFlowLoss
    from swift_amd.training.trainer import GradAllReduce
    from test_gpu_train import _dataset
    net, cfg, state = _net(dev, "smooth", 31)
    L = TrigFlowLoss(_dataset(31), dict(dist="loguniform", sigma_min=0.02, sigma_max=200.0), sigma_data=1.0).to(dev)
    ins = _trigflow_case(31)
    ref = _trigflow_ref(cfg, state, ins, L)
    ddp = GradAllReduce(net)
    ddp.zero_grad_flat()
    _trigflow_step(L, ddp, ins, dev)
    flat = ddp.flatten_grads()
    assert all(p.grad.data_ptr() >= flat.data_ptr() and p.grad.data_ptr() < flat.data_ptr() + 4 * flat.numel() for p in net.parameters())
    g1 = _param_grads(net)
    _hold("TrigFlowLoss through GradAllReduce, smooth net", g1, ref, cfg, True)
    _trigflow_step(L, ddp, ins, dev)   # no zero_grad_flat()
    g2 = _param_grads(net)
    errs = {}
    for k in g1:
        for sl, lab in gr.slicings(k, g1[k].shape, cfg).items():
            err, _ = gr.slice_errors(g2[k], 2 * g1[k].double(), lab)
            errs[k, sl, int(err.argmax())] = float(err.max())
    worst = max(errs, key=errs.get)
    print(f"second backward without zero_grad_flat(): worst slice of |g2 - 2 g1| / |2 g1| = {errs[worst]:.2e} at {worst}")
    assert errs[worst] <= 1e-5, (worst, errs[worst])


# --------------------------------------------------------------------------- 3. SCMLoss


@pytest.mark.parametrize("form", ["two-pass", "one-pass"])
def test_scm_slices_vs_fp64(dev, form):
    """SCMLoss on the smooth net: the two-pass form (fp32 tangent pass, then forward + backward) and the one-pass form (the
    bf16 tangent pass's primal rows are the saved activations of the backward)."""
    from oracle import loss as oloss
    from swift_amd.training.loss import SCMLoss
    from swift_amd.training.trainer import GradAllReduce
    from test_gpu_train import _dataset
    net, cfg, state = _net(dev, "smooth", 42)
    L = SCMLoss(_dataset(42), dict(dist="loguniform", sigma_min=0.02, sigma_max=200.0), sigma_data=1.0, tangent_warmup_kimg=3,
                jvp_dtype="f32" if form == "two-pass" else "bf16").to(dev)
    ins = _trigflow_case(42)
    if "scm" not in _refs:
        i64 = dict(ins, w_var=L.w_var.cpu(), w_lat=L.w_lat.cpu())
        f = lambda onet, i: oloss.scm_loss(onet, i["x"], i["tau"], i["z"], i["w_var"], i["w_lat"], step=1200, sigma_data=1.0,
                                           tangent_warmup_kimg=3, condition=i["cond"], auxiliary=i["aux"], return_logvar=True)
        _refs["scm"] = gr.oracle_gradients(cfg, state, NV, NV + NF, f, i64)
    ddp = GradAllReduce(net)
    ddp.zero_grad_flat()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = L(ddp, ins["x"].to(dev), 1200, condition=ins["cond"].to(dev), auxiliary=ins["aux"].to(dev), _tau=ins["tau"].to(dev),
                 _z=ins["z"].to(dev))
    loss.backward()
    assert L.last_one_pass == (form == "one-pass")
    _hold(f"SCMLoss, {form}, smooth net", _param_grads(net), _refs["scm"], cfg, True)


# --------------------------------------------------------------------------- 4. CRPSLoss


# The CRPS is a sum of absolute values, so its gradient with respect to a prediction is a sign: where a prediction sits within
# bf16 noise of the target or of the other member, ANY bf16 forward flips it.  On this case the oracle's own emulation flips
# 1e-5 ... 6e-5 of the elements, which moves d(loss)/d(prediction) by 7 ... 10 % in relative L2 (measured on the CPU, per
# network call).  The damage is local to a pixel, so it averages out of every gradient that sums over tokens (7e-3 like the other
# loss paths) and stays in the three slicings that are local in token or channel space: yardsticks 2.7e-2 (pos_embed per
# window), 5.0e-2 (per 16-token row) and 2.3e-2 (patch embedding per input channel).  They keep the 2 x yardstick rule -- the
# engine sits at 1.04 ... 1.09 of it -- but cannot meet the 3e-2 guard, which was derived from the smooth losses.
CRPS_PIXEL_LOCAL = (("pos_embed", "window"), ("pos_embed", "row16"), ("patch_embed.emb.weight", "channel"))


@pytest.mark.parametrize("keep", [None, "0"])
def test_crps_slices_vs_fp64(dev, keep, monkeypatch):
    """CRPSLoss, two members x two rollout steps (four network calls; three steps cost the fp64 oracle 15 s), smooth net: every
    call's activations resident (SWIFTK_CRPS_KEEP unset: the memory rule keeps all four of this small net) and every call
    recomputed ("0")."""
    from oracle import loss as oloss
    from oracle.rollout import Stats
    from swift_amd.training.loss import CRPSLoss
    from swift_amd.training.trainer import GradAllReduce
    from swift_amd.utils.detinit import det_normal
    from test_gpu_train import _dataset
    if keep is None:
        monkeypatch.delenv("SWIFTK_CRPS_KEEP", raising=False)
    else:
        monkeypatch.setenv("SWIFTK_CRPS_KEEP", keep)
    steps, B, seed = 2, 2, 33
    net, cfg, state = _net(dev, "smooth", seed, logvar=False)
    ds = _dataset(seed)
    L = CRPSLoss(ds, sigma_data=1.0, ensemble_size=2, alpha=0.95).to(dev)
    target, cond = det_normal((B, NV, 64, 64), seed, "t"), det_normal((B, NV + NF, 64, 64), seed, "c")
    aux, idx = torch.tensor([0.6, 0.6]), [0, 4]
    lat = [[det_normal((B, NV, 64, 64), seed, f"l{e}{i}") for i in range(steps)] for e in range(2)]
    if "crps" not in _refs:
        stats = Stats(ds.x_means, ds.x_stds, {6: ds.t_stds[6]}, n_vars=NV, n_forc=NF)
        ins = dict(target=target, cond=cond, aux=aux, w_var=L.w_var.cpu(), w_lat=L.w_lat.cpu())
        ins.update({f"l{e}{i}": lat[e][i] for e in range(2) for i in range(steps)})

        def f(onet, i):
            forc = lambda j: torch.stack([ds.get_forcings(q + j) for q in idx], 0).to(i["target"].dtype)
            ll = [[i[f"l{e}{j}"] for j in range(steps)] for e in range(2)]
            return oloss.crps_multistep_loss(onet, stats, i["target"], i["cond"], i["aux"], forc, ll, i["w_var"], i["w_lat"],
                                             steps=steps, alpha=0.95)
        _refs["crps"] = gr.oracle_gradients(cfg, state, NV, NV + NF, f, ins)
    ddp = GradAllReduce(net)
    ddp.zero_grad_flat()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = L(ddp, target.to(dev), condition=cond.to(dev), auxiliary=aux.to(dev), idx=idx, steps=steps, _latents=lat)
    loss.backward()
    assert L.last_n_keep == (2 * steps if keep is None else 0)
    _hold(f"CRPSLoss, steps = {steps}, SWIFTK_CRPS_KEEP = {keep}, smooth net", _param_grads(net), _refs["crps"], cfg, True,
          unguarded=CRPS_PIXEL_LOCAL)


# --------------------------------------------------------------------------- 5. padded head lanes


def test_padded_head_lanes_slices_vs_fp64(dev, monkeypatch):
    """SWIFTK_PAD_HEADS=1, 16 heads of 66 on 80 lanes, TrigFlowLoss, smooth clamp.  The gradients come back in the checkpoint's
    shapes and are sliced there (16 heads of 66 rows / columns): nothing of a pad lane may show up in any head's slice."""
    from swift_amd.training.loss import TrigFlowLoss
    from swift_amd.training.trainer import GradAllReduce
    from test_gpu_train import _dataset
    monkeypatch.setenv("SWIFTK_PAD_HEADS", "1")
    net, cfg, state = _net(dev, "smooth", 62, heads=16)
    assert (cfg.heads, cfg.head_dim) == (16, 66)
    L = TrigFlowLoss(_dataset(62), dict(dist="loguniform", sigma_min=0.02, sigma_max=200.0), sigma_data=1.0).to(dev)
    ins = _trigflow_case(62)
    ref = _trigflow_ref(cfg, state, ins, L)
    ddp = GradAllReduce(net)
    ddp.zero_grad_flat()
    _trigflow_step(L, ddp, ins, dev)
    eng = net.model._train_engine
    assert (eng.hd0, eng.hd) == (66, 80)
    got = _param_grads(net)
    assert all(got[k].shape == state[k].shape for k in state)
    _hold("TrigFlowLoss on padded head lanes (16 heads of 66), smooth net", got, ref, cfg, True)
