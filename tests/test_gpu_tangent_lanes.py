"""-m gpu: sCM pre-training and distillation at head widths no tangent kernel runs natively (64, 66), on zero-padded head lanes
(SWIFTK_PAD_HEADS=2), and the two device kernels that put a weight onto those lanes and take its gradient back off them.

Every network case is the SMALLB geometry of test_gpu_train.py (64x64 image, 2x2 patches, four windows, depth 2, B = 2) with the
inputs and the bars of the existing test of the same path on a native width.  The lane kernels are pure data movement plus one
rounding (pack) or one fp32 addition (gradient), so they are held to the BITS of the torch sequences they replace."""
import os

import numpy as np
import pytest
import torch
import yaml

import lane_reference as lanes
import layout_reference as lr
from conftest import rel_l2
from swift_amd.utils.detinit import det_normal
from test_gpu_train import _build_pair, _dataset, _grad_report

pytestmark = pytest.mark.gpu
GUARD = 1024  # sentinel elements in front of and behind every output buffer
EINVAL, ESHAPE = -1, -2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


# ============================================================================================ 1. tangent against the oracle
@pytest.mark.parametrize("dim,heads,lanes_want", [(768, 12, (64, 80, 960)), (1056, 16, (66, 80, 1280))])
def test_network_tangent_on_padded_lanes_vs_oracle_jvp(dev, monkeypatch, dim, heads, lanes_want):
    """Inputs and bars of test_gpu_train.py::test_network_tangent_vs_oracle_jvp, at the shipped distill-md width (12 heads of 64)
    and at 16 heads of 66 (dim % 64 == 32: the GEMMs' half k-tile)."""
    from swift_amd.jvp_engine import SwinJvpEngine
    from swift_amd.models.precond import _process_auxiliary
    monkeypatch.setenv("SWIFTK_PAD_HEADS", "2")
    net, onet, _ = _build_pair(dev, 41, dim=dim, heads=heads)
    B = 2
    x, cond = det_normal((B, 69, 64, 64), 41, "x"), det_normal((B, 72, 64, 64), 41, "c")
    vx = det_normal((B, 69, 64, 64), 41, "vx")
    t, vt, aux = torch.tensor([0.4, 1.3]), torch.tensor([0.35, 0.2]), torch.tensor([0.6, 0.6])
    with torch.no_grad():
        f = lambda xx, tt: onet(xx, tt, cond, aux, jvp=True)
        Fref, dref = torch.func.jvp(f, (x, t), (vx, vt))
    auxd = _process_auxiliary(aux.to(dev), 1, B, dev)
    errs = {}
    for dt in (torch.float32, torch.bfloat16):
        eng = SwinJvpEngine(net.model, dt)
        assert (eng.hd0, eng.hd, eng.inner) == lanes_want
        dF = eng.jvp([x.to(dev), cond.to(dev)], vx.to(dev), t.to(dev), vt.to(dev), auxd)
        assert torch.isfinite(dF).all()
        errs[dt] = rel_l2(dF.cpu(), dref)
        assert eng.L[0]["qkv"].shape[0] == 3 * lanes_want[2] and eng.L[0]["wo"].shape[0] == dim
    print(f"dim {dim}, {heads} heads: network tangent vs oracle jvp: fp32 rel-L2 {errs[torch.float32]:.3e}, "
          f"bf16 rel-L2 {errs[torch.bfloat16]:.3e}")
    assert errs[torch.float32] < 1e-4
    assert errs[torch.bfloat16] < 8e-2


# ============================================================================================ 2. sCM loss
def test_scm_loss_and_grads_on_padded_lanes_vs_oracle(dev, monkeypatch):
    """The sequence and bars of test_gpu_train.py::test_scm_loss_and_grads_vs_oracle at 12 heads of 64; the bf16 pass must be the
    one-pass form (the tangent pass's primal rows, saved at the padded widths, are the backward's activations)."""
    from oracle import loss as oloss
    from swift_amd.training.loss import SCMLoss
    from swift_amd.training.trainer import GradAllReduce
    monkeypatch.setenv("SWIFTK_PAD_HEADS", "2")
    monkeypatch.delenv("SWIFTK_SCM_ONE_PASS", raising=False)
    net, onet, st = _build_pair(dev, 42, logvar=True, dim=768, heads=12)
    ds = _dataset(42)
    L = SCMLoss(ds, dict(dist="loguniform", sigma_min=0.02, sigma_max=200.0), sigma_data=1.0, tangent_warmup_kimg=3,
                jvp_dtype="f32").to(dev)
    B = 2
    x, cond, z = det_normal((B, 69, 64, 64), 42, "x"), det_normal((B, 72, 64, 64), 42, "c"), det_normal((B, 69, 64, 64), 42, "z")
    tau, aux = torch.tensor([0.3, 4.0]).view(B, 1, 1, 1), torch.tensor([0.6, 0.6])
    ddp = GradAllReduce(net)
    ddp.zero_grad_flat()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = L(ddp, x.to(dev), 1200, condition=cond.to(dev), auxiliary=aux.to(dev), _tau=tau.to(dev), _z=z.to(dev))
    loss.backward()
    assert not L.last_one_pass  # (fp32 tangent rows are no bf16 activations)
    ref = oloss.scm_loss(onet, x, tau, z, L.w_var.cpu(), L.w_lat.cpu(), step=1200, sigma_data=1.0, tangent_warmup_kimg=3,
                         condition=cond, auxiliary=aux, return_logvar=True)
    ref.backward()
    print(f"12 heads of 64: sCM loss {float(loss):.6f} vs oracle {float(ref):.6f}; worst grad cosine {_grad_report(net, st, 0.999):.4f}")
    assert float(loss) == pytest.approx(float(ref), rel=1e-3)
    att = net.model.transformer.layers[0][0]
    assert att.to_qkv.weight.grad.shape == att.to_qkv.weight.shape == (3 * 768, 768)
    assert att.wo.weight.grad.shape == att.wo.weight.shape == (768, 768)
    L.jvp_dtype = torch.bfloat16
    with torch.autocast("cuda", dtype=torch.bfloat16):
        lb = L(ddp, x.to(dev), 1200, condition=cond.to(dev), auxiliary=aux.to(dev), _tau=tau.to(dev), _z=z.to(dev))
    assert float(lb) == pytest.approx(float(ref), rel=5e-2)
    assert L.last_one_pass
    eng, jeng = net.model._train_engine, net.model._jvp_engine
    assert (jeng.hd0, jeng.hd, jeng.inner, jeng.katt) == (eng.hd0, eng.hd, eng.inner, eng.katt) == (64, 80, 960, 960)
    assert jeng._share and jeng.L[0]["qkv"] is eng.L[0]["qkv"]
    ddp.zero_grad_flat()
    lb.backward()
    print(f"12 heads of 64: sCM one-pass loss {float(lb):.6f}; worst grad cosine {_grad_report(net, st, 0.999):.4f}")
    assert att.to_qkv.weight.grad.shape == (3 * 768, 768) and att.wo.weight.grad.shape == (768, 768)


# ============================================================================================ 3. distillation
def test_scm_distillation_on_padded_lanes_vs_oracle(dev, monkeypatch):
    """The sequence and bars of test_gpu_train.py::test_scm_distillation_loss_and_grads_vs_oracle: a 12-heads-of-64 student and a
    native-width teacher (12 heads of 88), as era5-swinv2-5.6-distill-md pairs them."""
    from oracle import loss as oloss
    from swift_amd.training.loss import SCMLoss
    from swift_amd.training.trainer import GradAllReduce
    monkeypatch.setenv("SWIFTK_PAD_HEADS", "2")
    net, onet, st = _build_pair(dev, 43, logvar=True, dim=768, heads=12)
    teacher, oteacher, _ = _build_pair(dev, 53, logvar=False, dim=1056, heads=12)
    teacher.eval().requires_grad_(False)
    ds = _dataset(43)
    L = SCMLoss(ds, dict(dist="loguniform", sigma_min=0.02, sigma_max=200.0), sigma_data=1.0, tangent_warmup_kimg=3,
                distillation=True, jvp_dtype="f32").to(dev)
    B = 2
    x, cond, z = det_normal((B, 69, 64, 64), 43, "x"), det_normal((B, 72, 64, 64), 43, "c"), det_normal((B, 69, 64, 64), 43, "z")
    tau, aux = torch.tensor([0.3, 4.0]).view(B, 1, 1, 1), torch.tensor([0.6, 0.6])
    ddp = GradAllReduce(net)
    ddp.zero_grad_flat()
    loss = L(ddp, x.to(dev), 1200, condition=cond.to(dev), auxiliary=aux.to(dev), net_pretrained=teacher, _tau=tau.to(dev),
             _z=z.to(dev))
    loss.backward()
    kw = dict(step=1200, sigma_data=1.0, tangent_warmup_kimg=3, condition=cond, auxiliary=aux, return_logvar=True)
    ref = oloss.scm_loss(onet, x, tau, z, L.w_var.cpu(), L.w_lat.cpu(), teacher=oteacher, **kw)
    ref.backward()
    with torch.no_grad():
        plain = oloss.scm_loss(onet, x, tau, z, L.w_var.cpu(), L.w_lat.cpu(), **kw)
    print(f"12 heads of 64: sCM distillation loss {float(loss):.6f} vs oracle {float(ref):.6f} (without teacher {float(plain):.6f}); "
          f"worst grad cosine {_grad_report(net, st, 0.999):.4f}")
    assert float(loss) == pytest.approx(float(ref), rel=1e-3)
    assert abs(float(plain) - float(ref)) > 10 * abs(float(loss) - float(ref))  # the teacher is what is being tested
    assert all(p.grad is None for p in teacher.parameters())
    L.jvp_dtype = torch.bfloat16
    with torch.autocast("cuda", dtype=torch.bfloat16):
        lb = L(ddp, x.to(dev), 1200, condition=cond.to(dev), auxiliary=aux.to(dev), net_pretrained=teacher, _tau=tau.to(dev),
               _z=z.to(dev))
    assert float(lb) == pytest.approx(float(ref), rel=5e-2)


# ============================================================================================ 4. what must stay as it is
def test_refusals_and_native_widths_are_untouched(dev, monkeypatch):
    from swift_amd._lib import SwiftkError
    from swift_amd.jvp_engine import SwinJvpEngine
    from swift_amd.models.precond import _process_auxiliary
    net16, _, _ = _build_pair(dev, 61, dim=1056, heads=16)
    for level in (None, "0", "1"):
        if level is None:
            monkeypatch.delenv("SWIFTK_PAD_HEADS", raising=False)
        else:
            monkeypatch.setenv("SWIFTK_PAD_HEADS", level)
        for dt in (torch.bfloat16, torch.float32):
            with pytest.raises(SwiftkError, match="tangent kernels") as e:
                SwinJvpEngine(net16.model, dt)
            assert str(e.value) == "the tangent kernels are built for head_dim 80 / 88 / 96"
    net, _, _ = _build_pair(dev, 41)  # 12 heads of 88
    B = 2
    x, cond, vx = det_normal((B, 69, 64, 64), 41, "x"), det_normal((B, 72, 64, 64), 41, "c"), det_normal((B, 69, 64, 64), 41, "vx")
    t, vt = torch.tensor([0.4, 1.3]), torch.tensor([0.35, 0.2])
    auxd = _process_auxiliary(torch.tensor([0.6, 0.6]).to(dev), 1, B, dev)
    outs = {}
    for level in (None, "2"):
        if level is None:
            monkeypatch.delenv("SWIFTK_PAD_HEADS", raising=False)
        else:
            monkeypatch.setenv("SWIFTK_PAD_HEADS", level)
        for dt in (torch.float32, torch.bfloat16):
            eng = SwinJvpEngine(net.model, dt)
            outs[level, dt] = eng.jvp([x.to(dev), cond.to(dev)], vx.to(dev), t.to(dev), vt.to(dev), auxd).clone()
            assert (eng.hd0, eng.hd, eng.inner, eng.katt) == (88, 88, 1056, eng.kd)  # the same lane arguments and buffer widths
    for dt in (torch.float32, torch.bfloat16):
        assert torch.equal(outs[None, dt], outs["2", dt])


# ============================================================================================ 5. the lane kernels through the C ABI
LANE_CASES = [(9, 33, 80, 100), (48, 66, 80, 1056), (18, 64, 80, 384)]  # blocks x hd -> hdp, the other extent


@pytest.fixture(scope="module")
def L():
    from swift_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(n, dtype, dev):
    """n elements of ``dtype`` with GUARD sentinel elements on either side, all sentinel to begin with."""
    if dtype == torch.bfloat16:
        whole = torch.full((n + 2 * GUARD,), lr.SENT_BF16, dtype=torch.int16, device=dev).view(torch.bfloat16)
    else:
        whole = torch.full((n + 2 * GUARD,), lr.SENT_F32, dtype=torch.int32, device=dev).view(torch.float32)
    return whole, whole[GUARD:GUARD + n]


def _bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32).cpu()


def _guards_intact(whole, body_too=False):
    b = _bits(whole)
    sent = lr.SENT_BF16 if whole.dtype == torch.bfloat16 else lr.SENT_F32
    part = b if body_too else torch.cat([b[:GUARD], b[-GUARD:]])
    return bool((part == sent).all())


def _nan_rows(valid, ld, dev):
    buf = torch.full((valid.shape[0], ld), float("nan"), dtype=torch.float32)
    buf[:, :valid.shape[1]] = valid
    return buf.to(dev)


def _first_mismatch(name, got, want, source_of):
    bad = _bits(got) != _bits(want)
    if bool(bad.any()):
        idx = torch.nonzero(bad)
        at = tuple(int(v) for v in idx[0])
        msg = (f"{name}: {idx.shape[0]} wrong elements, first at {at}: got {float(got[at])!r}, want {float(want[at])!r}; "
               f"that element {source_of(at)}")
        print(msg)
        raise AssertionError(msg)


def _extents(axis, blocks, hd, hdp, other):
    """(rows, cols) of the parameter and (rl, cl) of its lane-shaped copy."""
    return ((blocks * hd, other), (blocks * hdp, other)) if axis == 0 else ((other, blocks * hd), (other, blocks * hdp))


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("blocks,hd,hdp,other", LANE_CASES)
def test_cast_pad_t_lanes_bit_exact(L, dev, axis, blocks, hd, hdp, other):
    from swift_amd import ops
    from swift_amd.engine import pack_qkv_lanes, pack_wo_lanes
    (rows, cols), (rl, cl) = _extents(axis, blocks, hd, hdp, other)
    w = det_normal((rows, cols), 500 + hd + axis, "w")
    ldw = cols + 5
    wd = _nan_rows(w, ldw, dev)  # NaN behind every row of the parameter: nothing past `cols` may be read
    ldo, ldt = ops.k_pad(torch.bfloat16, cl), ops.k_pad(torch.bfloat16, rl) + 8
    whole_o, out = _guarded(rl * ldo, torch.bfloat16, dev)
    whole_t, out_t = _guarded(cl * ldt, torch.bfloat16, dev)
    rc = L.swiftk_cast_pad_t_lanes(wd.data_ptr(), ldw, rows, cols, out.data_ptr(), ldo, out_t.data_ptr(), ldt, axis, blocks, hd, hdp,
                                   _stream())
    torch.cuda.synchronize()
    assert rc == 0
    # what the kernel replaces: the host-side packer, then the cast with zero row padding, of the weight and of its transpose
    heads = blocks // 3 if axis == 0 else blocks
    wp = (pack_qkv_lanes(w, heads, hd, hdp) if axis == 0 else pack_wo_lanes(w, heads, hd, hdp)).to(dev)
    assert wp.shape == (rl, cl)
    want, want_t = ops.pad_cols(wp, ldo, torch.bfloat16), ops.pad_cols(wp.t().contiguous(), ldt, torch.bfloat16)
    torch.cuda.synchronize()

    def source(at, transposed):
        r, c = (at[1], at[0]) if transposed else at
        if r >= rl or c >= cl:
            return "is row padding: it must be zero and reads nothing"
        s = lanes.lane_src(r if axis == 0 else c, hd, hdp)
        if s < 0:
            return f"is a pad lane (lane index {r if axis == 0 else c} = block {(r if axis == 0 else c) // hdp}, lane {(r if axis == 0 else c) % hdp}): it must be zero"
        return f"should have read W[{s if axis == 0 else r}][{c if axis == 0 else s}]"

    _first_mismatch(f"cast_pad_t_lanes axis {axis} out (r', c')", out.view(rl, ldo), want, lambda at: source(at, False))
    _first_mismatch(f"cast_pad_t_lanes axis {axis} out_t (c', r')", out_t.view(cl, ldt), want_t, lambda at: source(at, True))
    assert _guards_intact(whole_o) and _guards_intact(whole_t)
    assert not _bits(out.view(rl, ldo)[:, cl:]).any() and not _bits(out_t.view(cl, ldt)[:, rl:]).any()  # +0.0 in every padding


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("blocks,hd,hdp,other", LANE_CASES)
def test_lanes_grad_add_bit_exact(L, dev, axis, blocks, hd, hdp, other):
    from swift_amd.engine import unpack_qkv_lanes, unpack_wo_lanes
    (rows, cols), (rl, cl) = _extents(axis, blocks, hd, hdp, other)
    heads = blocks // 3 if axis == 0 else blocks
    G0 = det_normal((rows, cols), 600 + hd + axis, "G")
    g = det_normal((rl, cl), 600 + hd + axis, "g")
    gn = g.clone()  # NaN in every pad lane: the adjoint drops them unread
    pad = lanes.src_table(blocks, hd, hdp) < 0
    if axis == 0:
        gn[pad, :] = float("nan")
    else:
        gn[:, pad] = float("nan")
    want = (G0.to(dev) + (unpack_qkv_lanes(g.to(dev), heads, hd, hdp) if axis == 0 else unpack_wo_lanes(g.to(dev), heads, hd, hdp))).cpu()
    for pad_g, pad_l in ((0, 0), (4, 8), (3, 1)):  # contiguous (the engine's case), padded rows that keep the vector form, odd strides
        ldg, ldl = cols + pad_g, cl + pad_l
        whole, Gd = _guarded(rows * ldg, torch.float32, dev)
        Gd.view(rows, ldg)[:, :cols] = G0.to(dev)
        gd = _nan_rows(gn, ldl, dev)
        rc = L.swiftk_lanes_grad_add(Gd.data_ptr(), ldg, gd.data_ptr(), ldl, rows, cols, axis, blocks, hd, hdp, _stream())
        torch.cuda.synchronize()
        assert rc == 0

        def source(at):
            r, c = at
            return (f"should have read g[{lanes.lane_dst(r, hd, hdp)}][{c}]" if axis == 0 else
                    f"should have read g[{r}][{lanes.lane_dst(c, hd, hdp)}]")

        _first_mismatch(f"lanes_grad_add axis {axis} ldg {ldg} ldl {ldl} G (r, c)", Gd.view(rows, ldg)[:, :cols].cpu(), want, source)
        assert _guards_intact(whole)
        if pad_g:
            assert bool((_bits(Gd.view(rows, ldg)[:, cols:]) == lr.SENT_F32).all())  # the padding of G's rows is not written


def test_lane_kernels_refuse_before_launching(L, dev):
    """Every refusal the header lists, by return code, with the outputs (sentinel all over) untouched."""
    blocks, hd, hdp, other = 6, 33, 80, 40
    big = (1 << 30) + 64
    for axis in (0, 1):
        (rows, cols), (rl, cl) = _extents(axis, blocks, hd, hdp, other)
        w = torch.zeros(rows, cols, device=dev)
        whole_o, out = _guarded(rl * cl, torch.bfloat16, dev)
        whole_t, out_t = _guarded(cl * rl, torch.bfloat16, dev)
        good = dict(W=w.data_ptr(), ldw=cols, rows=rows, cols=cols, out=out.data_ptr(), ldo=cl, out_t=out_t.data_ptr(), ldt=rl, axis=axis,
                    blocks=blocks, hd=hd, hdp=hdp)
        lane, cross = ("rows", "cols") if axis == 0 else ("cols", "rows")
        cases = [(dict(W=None), EINVAL), (dict(out=None), EINVAL), (dict(out_t=None), EINVAL), (dict(rows=0), EINVAL),
                 (dict(cols=0), EINVAL), (dict(rows=-rows), EINVAL), (dict(blocks=0), EINVAL), (dict(hd=0), EINVAL),
                 (dict(hdp=hd - 1), EINVAL), (dict(ldw=cols - 1), EINVAL), (dict(axis=2), EINVAL), (dict(axis=-1), EINVAL),
                 (dict(ldo=cl - 1), EINVAL), (dict(ldt=rl - 1), EINVAL),
                 (dict(ldo=blocks * hd if axis == 1 else cl - 1), EINVAL), (dict(ldt=blocks * hd if axis == 0 else rl - 1), EINVAL),
                 (dict(blocks=blocks + 1), ESHAPE), (dict(hd=hd + 1, hdp=hdp), ESHAPE), ({lane: blocks * hd - 1}, ESHAPE),
                 ({cross: big, "ldw": big, "ldo": big, "ldt": big}, ESHAPE), (dict(ldo=big), ESHAPE), (dict(ldt=big), ESHAPE),
                 (dict(hdp=big), ESHAPE), ({cross: 65536 * 64, "ldw": 65536 * 64, "ldt": 65536 * 64}, ESHAPE) if axis == 1 else
                 (dict(ldt=65536 * 64), ESHAPE)]
        for change, want in cases:
            a = dict(good, **change)
            rc = L.swiftk_cast_pad_t_lanes(a["W"], a["ldw"], a["rows"], a["cols"], a["out"], a["ldo"], a["out_t"], a["ldt"], a["axis"],
                                           a["blocks"], a["hd"], a["hdp"], _stream())
            assert rc == want, (axis, change, rc)
        torch.cuda.synchronize()
        assert _guards_intact(whole_o, body_too=True) and _guards_intact(whole_t, body_too=True)
        whole_g, G = _guarded(rows * cols, torch.float32, dev)
        gl = torch.zeros(rl, cl, device=dev)
        good = dict(G=G.data_ptr(), ldg=cols, g=gl.data_ptr(), ldl=cl, rows=rows, cols=cols, axis=axis, blocks=blocks, hd=hd, hdp=hdp)
        cases = [(dict(G=None), EINVAL), (dict(g=None), EINVAL), (dict(rows=0), EINVAL), (dict(cols=0), EINVAL), (dict(blocks=-1), EINVAL),
                 (dict(hd=0), EINVAL), (dict(hdp=hd - 1), EINVAL), (dict(ldg=cols - 1), EINVAL), (dict(axis=2), EINVAL),
                 (dict(ldl=cl - 1), EINVAL), (dict(ldl=blocks * hd if axis == 1 else cl - 1), EINVAL),
                 (dict(blocks=blocks + 1), ESHAPE), ({lane: blocks * hd + 1, "ldg": big}, ESHAPE), ({cross: big, "ldg": big, "ldl": big}, ESHAPE),
                 (dict(hdp=big), ESHAPE)]
        for change, want in cases:
            a = dict(good, **change)
            rc = L.swiftk_lanes_grad_add(a["G"], a["ldg"], a["g"], a["ldl"], a["rows"], a["cols"], a["axis"], a["blocks"], a["hd"],
                                         a["hdp"], _stream())
            assert rc == want, (axis, change, rc)
        torch.cuda.synchronize()
        assert _guards_intact(whole_g, body_too=True)


def test_training_engine_operands_are_the_packed_casts(dev, monkeypatch):
    """The engine-level statement of bit identity at 16 heads of 66: after ``refresh()`` the four attention operands of a layer are,
    bit for bit, ``cast_pad_t`` of the host-side packers' output -- the sequence the kernel replaced."""
    from swift_amd import ops
    from swift_amd.engine import pack_qkv_lanes, pack_wo_lanes
    from swift_amd.train_engine import SwinTrainEngine
    monkeypatch.setenv("SWIFTK_PAD_HEADS", "1")
    net, _, _ = _build_pair(dev, 61, dim=1056, heads=16)
    eng = SwinTrainEngine(net.model)
    eng.refresh()
    att = net.model.transformer.layers[1][0]
    W = eng.L[1]
    for name, packed in (("qkv", pack_qkv_lanes(att.to_qkv.weight.detach(), 16, 66, 80)), ("wo", pack_wo_lanes(att.wo.weight.detach(), 16, 66, 80))):
        a, b = torch.empty_like(W[name]), torch.empty_like(W[name + "_t"])
        ops.cast_pad_t(packed.contiguous(), a, b)
        torch.cuda.synchronize()
        assert torch.equal(_bits(a), _bits(W[name])) and torch.equal(_bits(b), _bits(W[name + "_t"])), name


# ============================================================================================ 6. the command line, end to end
def test_distill_md_experiment_as_shipped_trains_and_generates(tmp_path):
    """The user story: a TrigFlow teacher run, then experiment=era5-swinv2-5.6-distill-md (12 heads of 64) distilling from it under
    SWIFTK_PAD_HEADS=2 with in-training validation, then a forecast from the student's checkpoint."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from test_gpu_cli import run
    small = ["data=era5-synthetic-5.6", "data.dataset.length=48", "data.data_workers=0", "model.depth=2", "trainer.total_kimg=0.008",
             "trainer.kimg_per_tick=0.004", "trainer.checkpoint_ticks=1", "trainer.lr_rampup_kimg=0", "data.batch_size=2"]
    run(["swift_amd.train", "experiment=era5-swinv2-5.6-trigflow", "trainer.val_ticks=null"] + small, cwd=str(tmp_path))
    teacher = tmp_path / "results" / "era5-swinv2-5.6-trigflow" / "000"
    assert sorted(os.listdir(teacher / "checkpoints"))
    env = {"SWIFTK_PAD_HEADS": "2", "HYDRA_RUN_ID": "001"}
    run(["swift_amd.train", "experiment=era5-swinv2-5.6-distill-md", f"distill={teacher}", "loss.tangent_warmup_kimg=1",
         "trainer.val_ticks=1", "trainer.val_target_interval=4", "data.val_local_batch_size=2"] + small, cwd=str(tmp_path), env=env)
    rdir = tmp_path / "results" / "era5-swinv2-5.6-distill-md" / "001"
    cfg = yaml.safe_load(open(rdir / ".hydra" / "config.yaml"))
    assert cfg["loss"]["_target_"].endswith("SCMLoss") and cfg["distill"] == str(teacher)  # distillation flag: apply_distill_flag
    assert (cfg["model"]["dim"], cfg["model"]["heads"]) == (768, 12)
    assert sorted(os.listdir(rdir / "checkpoints"))
    lines = [yaml.safe_load(l) for l in open(rdir / "stats.jsonl")]
    assert len(lines) >= 2 and all(np.isfinite(l["train/loss"]) for l in lines)
    val = [yaml.safe_load(l) for l in open(rdir / "val_stats.jsonl")]
    assert val and np.isfinite(val[0]["val/rmse"])
    run(["swift_amd.generate", "--input", str(rdir), "--members", "2", "--steps", "2", "--samples", "2", "--batch", "4",
         "--dump", "numpy"], cwd=str(tmp_path), env=env)
    a = np.load(rdir / "output" / "latest" / "output-2i-2s-2m-6h.npy")
    assert a.shape == (2, 2, 3, 69, 32, 64) and np.isfinite(a).all()
