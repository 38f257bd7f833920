"""The closed forms of tests/backward_reference.py (the references of tests/test_gpu_backward_kernels.py) against autograd of what the
oracle already has -- F.silu(gate) * up, _prenorm, F.layer_norm with the modulation, oracle.loss.almost_fair_crps and trigflow_loss,
tests/edm_reference.py, oracle.metrics, torch.optim.Adam / AdamW + lerp -- all in fp64 to <= 1e-12, and the conditions the GPU
tolerances rest on: every dlogvar / dscale sum is well conditioned, torch's fp32 evaluation of SwiGLU rounds to the same bf16 value as
fp64 on all but <= 1e-4 of the elements, and the exact CRPS case really is exactly summable in fp32 in any order.
"""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import backward_reference as br
import edm_reference as er
from conftest import rel_l2
from oracle import loss as oloss
from oracle import metrics as omet

TOL = 1e-12
D = torch.float64


def rnd64(shape, seed, std=1.0):
    return br.rnd(shape, seed, std).double()


def test_swiglu_closed_form_vs_autograd():
    h, d = (v.double() for v in br.swiglu_inputs(7, 13, 1))
    hc = h.clone().requires_grad_(True)
    out = F.silu(hc[:, 0::2]) * hc[:, 1::2]
    out.backward(d)
    dg, du, sg, su = br.swiglu_bwd(h, d)
    assert rel_l2(br.swiglu_fwd(h), out.detach()) < TOL
    assert rel_l2(dg, hc.grad[:, 0::2]) < TOL and rel_l2(du, hc.grad[:, 1::2]) < TOL
    # the planted gates sit in the last row; at -1.2784645 the factor of dgate vanishes: the result is tiny against |d u|
    j = br.PLANTED_GATES.index(-1.2784645)
    assert float(h[-1, 2 * j]) == pytest.approx(-1.2784645, rel=1e-7)
    assert abs(float(dg[-1, j])) < 1e-6 * float(sg[-1, j])
    assert torch.equal(sg, (d * h[:, 1::2]).abs()) and rel_l2(su, du.abs()) < TOL


def test_swiglu_fp32_restatement_share_is_far_below_the_cap():
    """Condition of the bf16 scoring: torch's fp32 evaluation, rounded to bf16, differs from the rounded fp64 result on <= 1e-4 of
    the elements and never by more than one ulp -- the GPU test's cap of 1e-3 is >= 10 x what correct arithmetic needs."""
    h, d = br.swiglu_inputs(301, 3413, 40)
    h, d = h.bfloat16().float(), d.bfloat16().float()
    dg, du, _, _ = br.swiglu_bwd(h, d)
    dg32, du32, _, _ = br.swiglu_bwd(h, d, torch.float32)
    for name, got, ref in (("out", br.swiglu_fwd(h, torch.float32), br.swiglu_fwd(h)), ("dgate", dg32, dg), ("dup", du32, du)):
        ulps, share = br.bf16_score(got.bfloat16().float(), ref)
        print(f"swiglu {name}: fp32 restatement vs fp64, bf16-rounded: worst {ulps:.2f} ulp, mismatch share {share:.2e}")
        assert ulps <= 1.0 and share <= 1e-4


def test_bf16_ulp_and_score():
    v = torch.tensor([1.0, 1.5, 2.0, -3.0, 0.0078125, 100.0])
    assert torch.equal(br.bf16_ulp(v), torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -14, 2.0 ** -1], dtype=D))
    ref = torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=D)
    got = torch.tensor([1.0, 2.0 + 2.0 ** -6, 3.0, 4.0])
    ulps, share = br.bf16_score(got, ref)
    assert ulps == 1.0 and share == 0.25


def test_qknorm_closed_form_vs_autograd_of_prenorm():
    from test_gpu_train import _prenorm
    M, heads, hd = 6, 3, 8
    raw, dq = rnd64((M, 3 * heads * hd), 2), rnd64((M, 3 * heads * hd), 3)
    scale = torch.log(torch.tensor([10.0, 200.0, 3.0], dtype=D))  # (torch's clamp passes the gradient AT the bound, the kernel does not)
    rc, sc = raw.clone().requires_grad_(True), scale.clone().requires_grad_(True)
    ref = _prenorm(rc.view(1, M, -1), sc, heads, hd)[0]
    ref.backward(dq)
    qkvh, rn = br.prenorm_fwd(raw, scale, heads, hd)
    assert rel_l2(qkvh, ref.detach()) < TOL
    dqkv, dscale, ascale = br.qknorm_bwd(qkvh, dq, rn, scale, heads, hd)
    assert rel_l2(dqkv, rc.grad) < TOL
    assert rel_l2(dscale, sc.grad) < TOL and float(dscale[1]) == 0.0
    assert (ascale >= dscale.abs()).all()
    # the v vectors pass through
    assert torch.equal(dqkv.view(M, heads, 3, hd)[:, :, 2], dq.view(M, heads, 3, hd)[:, :, 2])
    at = torch.tensor([4.605170185988092], dtype=torch.float32)
    assert float(br.qknorm_bwd(qkvh[:, :3 * hd], dq[:, :3 * hd], rn[:, :3], at, 1, hd)[1]) == 0.0


@pytest.mark.parametrize("M,heads,hd,dt,seed", br.qknorm_cases())
def test_dscale_sums_are_well_conditioned(M, heads, hd, dt, seed):
    qkvh, dq, rn, scale = br.qknorm_inputs(M, heads, hd, seed, dt)
    _, dscale, ascale = br.qknorm_bwd(qkvh.float(), dq.float(), rn, scale, heads, hd)
    live = scale.double() < br.LN100
    assert live.any() and not live.all()
    assert float(scale[1]) == float(torch.tensor(4.605170185988092, dtype=torch.float32)) or (heads == 2 and seed % 2)
    cond = ascale[live] / dscale[live].abs()
    assert float(cond.max()) <= 10.0, cond


def test_modnorm_closed_form_vs_autograd():
    d, rps, B = 24, 8, 3
    y, g, gamma, beta, mod = (v.double() for v in br.modnorm_inputs(d, rps, B, 5, bf16=False, offset_row=True))
    yc, gc, bc, mc = (v.clone().requires_grad_(True) for v in (y, gamma, beta, mod))
    ln = F.layer_norm(yc.view(B, rps, d), (d,), gc, bc, 1e-6)
    out = ln * (1 + mc[:, None, :d]) + mc[:, None, d:]
    out.backward(g.view(B, rps, d))
    r = br.modnorm_bwd(y, g, gamma, beta, mod, rps)
    # (row 0 is constant: rstd = 1000 amplifies the fp64 rounding of autograd's own centring; the other rows to 1e-12)
    assert rel_l2(r["dy"][1:], yc.grad[1:]) < TOL and rel_l2(r["dy"][0], yc.grad[0]) < 1e-9
    assert rel_l2(r["dgamma"], gc.grad) < TOL and rel_l2(r["dbeta"], bc.grad) < TOL and rel_l2(r["dmod"], mc.grad) < TOL
    assert float(r["dy"][4].abs().max()) == 0.0   # the zero row of g
    for one_pass in (False, True):
        e = br.row_rel_l2(br.modnorm_bwd_fp32(y.float(), g.float(), gamma.float(), mod.float(), rps, one_pass=one_pass), r["dy"])
        assert float(e[br.MODNORM_HOSTILE + 1:].max()) < 1e-5, (one_pass, e)


def _weights4(w_var, w_lat):
    return w_var.double().view(1, -1, 1, 1), w_lat.double().view(1, 1, -1, 1)


@pytest.mark.parametrize("m", [2, 3, 8, 12])
@pytest.mark.parametrize("alpha", [0.95, 1.0])
def test_crps_closed_form_vs_autograd(m, alpha):
    B, C, H, W = br.SHAPE_SMALL
    preds, target = rnd64((m, B, C, H, W), 10 + m), rnd64((B, C, H, W), 11 + m)
    w_var, w_lat = br.loss_weights(C, H, 12)
    wv, wl = _weights4(w_var, w_lat)
    pc = preds.clone().requires_grad_(True)
    ref = (wv * wl * oloss.almost_fair_crps(pc, target, alpha)).sum(1).mean()
    (0.25 * ref).backward()
    loss, dp, scale = br.crps(preds, target, w_var, w_lat, alpha, 0.25)
    assert float(loss) == pytest.approx(float(ref.detach()), rel=TOL)
    assert rel_l2(dp, pc.grad) < TOL and scale.shape == target.shape


def test_crps_ties_have_sign_zero():
    B, C, H, W = br.SHAPE_SMALL
    preds, target = rnd64((3, B, C, H, W), 13), rnd64((B, C, H, W), 14)
    preds[0, 0, 0, 0, 0] = target[0, 0, 0, 0]           # a member equal to the target
    preds[1, 1, 2, 3, 4] = preds[2, 1, 2, 3, 4]         # two equal members
    w_var, w_lat = br.loss_weights(C, H, 12)
    wv, wl = _weights4(w_var, w_lat)
    pc = preds.clone().requires_grad_(True)
    (wv * wl * oloss.almost_fair_crps(pc, target, 0.95)).sum(1).mean().backward()
    _, dp, _ = br.crps(preds, target, w_var, w_lat, 0.95)
    assert rel_l2(dp, pc.grad) < TOL


def test_trigflow_closed_forms_vs_oracle():
    c = br.trigflow_inputs(br.SHAPE_SMALL, 20)
    B = br.SHAPE_SMALL[0]
    x, z, t, Fo, lv = (c[k].double() for k in ("x", "z", "t", "F", "lv"))
    wv, wl = _weights4(c["w_var"], c["w_lat"])
    Fc, lc = Fo.clone().requires_grad_(True), lv.clone().requires_grad_(True)
    seen = {}

    def net(xx, tt, cond, aux, return_logvar=False):
        seen["x"] = xx
        return Fc, lc

    tau = br.SD * torch.tan(t).view(B, 1, 1, 1)
    ref = oloss.trigflow_loss(net, x, tau, z, wv, wl, br.SD, return_logvar=True)
    (0.25 * ref).backward()
    xt, vt = br.trigflow_prep(x, z, t, br.SD)
    assert rel_l2(xt, seen["x"]) < TOL
    r = br.trigflow_loss(Fo, vt, lv, c["w_var"], c["w_lat"], br.SD, 0.25)
    assert float(r["loss"]) == pytest.approx(float(ref.detach()), rel=TOL)
    assert rel_l2(r["dF"], Fc.grad) < TOL and rel_l2(r["dlogvar"], lc.grad) < TOL
    # without logvar: lv = 0
    r0 = br.trigflow_loss(Fo, vt, None, c["w_var"], c["w_lat"], br.SD)
    ref0 = oloss.trigflow_loss(lambda *a, **k: Fo, x, tau, z, wv, wl, br.SD)
    assert float(r0["loss"]) == pytest.approx(float(ref0.detach()), rel=TOL)


@pytest.mark.parametrize("shape", [br.SHAPE_SMALL, br.SHAPE_PAST_CAP, br.SHAPE_WORKLOAD], ids=["small", "past-cap", "workload"])
def test_dlogvar_sums_are_well_conditioned(shape):
    c = br.trigflow_inputs(shape, 20)
    r = br.trigflow_loss(c["F"], c["vt"], c["lv"], c["w_var"], c["w_lat"], br.SD, 0.25)
    cond = br.condition(r["terms"], 1)
    print(f"dlogvar at {shape}: sum|term| / |sum term| = {[round(float(v), 3) for v in cond]}")
    assert float(cond.max()) <= 10.0


def test_edm_closed_forms_vs_edm_reference():
    B, C, H, W = br.SHAPE_SMALL
    x, z, Fo = rnd64((B, C, H, W), 30), rnd64((B, C, H, W), 31), rnd64((B, C, H, W), 32)
    sigma = torch.tensor([0.01, 0.7, 40.0], dtype=D)
    w_var, w_lat = br.loss_weights(C, H, 33)
    wv, wl = _weights4(w_var, w_lat)
    Fc = Fo.clone().requires_grad_(True)
    seen = {}

    def net(xx, cn, cond, aux):
        seen["x"] = xx
        return Fc

    ref = er.edm_loss(net, x, sigma, z, wv, wl, br.SD)
    (0.25 * ref).backward()
    assert rel_l2(br.edm_prep(x, z, sigma, br.SD), seen["x"]) < TOL
    loss, dF, scale = br.edm_loss(Fo, x, z, sigma, w_var, w_lat, br.SD, 0.25)
    # (D - x at sigma = 0.01 cancels 1e4-fold in the reference's form: compare at the conditioning of that difference)
    assert float(loss) == pytest.approx(float(ref.detach()), rel=1e-10)
    assert float((dF - Fc.grad).abs().max() / scale.max()) < TOL and (scale >= dF.abs() * (1 - 1e-12)).all()


@pytest.mark.parametrize("N", [2, 9, 17])
def test_ensemble_sums_vs_oracle_metrics(N):
    B, V, H, W = 2, 3, 7, 11
    pred, y = rnd64((B, N, V, H, W), 50 + N), rnd64((B, V, H, W), 51)
    lat = np.linspace(-80, 80, H)
    w = omet._w(lat, y)
    s = br.ensemble_sums(pred, y, w)
    hw = H * W
    rm = torch.sqrt(s[..., 0] / hw).mean(0)
    assert rel_l2(rm, omet.rmse(pred, y, lat)) < TOL
    cr = (s[..., 1] / (N * hw)).mean(0) - (s[..., 2] / (hw * 2 * N * (N - 1))).mean(0)
    assert rel_l2(cr, omet.crps(pred, y, lat)) < TOL
    assert rel_l2(torch.sqrt(s[..., 3] / hw).mean(0) / rm, omet.spread_skill_ratio(pred, y, lat)) < TOL


@pytest.mark.parametrize("cls", [torch.optim.AdamW, torch.optim.Adam])
def test_adam_ema_step_vs_torch(cls):
    p0, e0 = rnd64((33, 7), 60, 0.05), rnd64((33, 7), 61, 0.05)
    kw = dict(lr=2e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05)
    P = torch.nn.Parameter(p0.clone())
    opt = cls([P], **kw)
    p, m, v, e = p0, torch.zeros_like(p0), torch.zeros_like(p0), e0
    E = e0.clone()
    for t, beta in ((1, 0.3), (2, 0.9)):
        g = rnd64((33, 7), 62 + t, 1e-2)
        g[0, 0], g[1, 1], g[2, 2] = float("nan"), float("inf"), float("-inf")
        P.grad = torch.nan_to_num(g, nan=0.0, posinf=1e5, neginf=-1e5)
        opt.step()
        E = P.detach().lerp(E, beta)
        gs, p, m, v, e = br.adam_ema_step(p, g, m, v, e, kw["lr"], kw["weight_decay"], 0.9, 0.95, 1e-8, t, beta, cls is torch.optim.AdamW)
        assert torch.equal(gs, P.grad)
        assert rel_l2(p, P.detach()) < TOL and rel_l2(e, E) < TOL
        assert rel_l2(m, opt.state[P]["exp_avg"]) < TOL and rel_l2(v, opt.state[P]["exp_avg_sq"]) < 1e-11
    assert br.adam_ema_step(p, g, m, v, None, 1e-3, 0.0, 0.9, 0.95, 1e-8, 3, 0.5, True)[4] is None


def test_exact_crps_inputs_are_exactly_summable():
    """The loss terms and the gradient of the exact case in fp32 arithmetic: summed one by one in 8 random orders the terms give
    the fp64 loss bit for bit, and every gradient element is an fp32 number."""
    preds, target, w_var, w_lat = br.exact_crps_inputs()
    loss, dp, _ = br.crps(preds, target, w_var, w_lat, 1.0)
    m, B, C, H, W = preds.shape
    assert preds.numel() // m == 2 ** 21
    f = np.float32
    x, y = preds.numpy(), target.numpy()
    cs = f(1.0) / (f(2.0) * f(m) * f(m - 1))
    skill = np.abs(x - y[None]).sum(0, dtype=f)
    spread = f(2.0) * np.abs(x[0] - x[1])
    terms = (skill / f(m) - cs * spread).astype(f).reshape(-1)
    assert set(np.unique(terms * 4)) <= set(range(-2, 9))
    inv = f(1.0) / (f(B) * f(H) * f(W))
    rng = np.random.default_rng(0)
    for _ in range(8):
        total = np.cumsum(rng.permutation(terms), dtype=f)[-1] * inv
        assert total.dtype == f and float(total) == float(loss)
    assert float(loss) != 0.0
    assert torch.equal(dp.float().double(), dp) and float(dp.abs().max()) > 0
