"""-m gpu: the network tangent of SwinJvpEngine, branch by branch, slice by slice and direction by direction against
torch.func.jvp of the CPU oracle in fp64 (tests/network_tangent_reference.py).

Every tangent kernel is scored on its own elsewhere; what is scored here is their COMPOSITION in swift_amd/jvp_engine.py -- the
modulation slot each norm reads, tangent rows without bias and position embedding, the layers that shift, primal and tangent rows
in one buffer, and each of the fused / unfused, pair / fp32-stream, shared / per-layer-buffer, native / padded-lane forms.  The
engine's ``taps`` hand out the residual stream after the patch embedding and after every branch, and the latent chain; each is
cut into windows of the layer that wrote it, head-width column blocks and GEMM tiles (the output: channels, windows, shifted
windows), and every slice is held to

  bf16 operands   2 x the worst slice of the oracle's two bf16 emulations, measured against fp64 in the same test (and that
                  bound itself under 3e-2); emb / lat / mod and their tangents, fp32 on both sides, to 1e-5
  fp32 operands   1e-4 (the whole-output figure of test_gpu_train.py::test_network_tangent_vs_oracle_jvp, now per slice)
  zeros           exactly: a sample whose direction is zero has a zero tangent everywhere and leaves the other samples' bits
                  alone; the time direction does not reach tok0

in the direction the sCM loss uses (``both``) and in the time direction alone, which is 1 % of ``both`` in norm and all that
the dmod chain carries.  All at SMALLB (64x64 image, four windows, one shifted layer, dim 1056, depth 2), B = 3, smooth net."""
import pytest
import torch

import gradient_reference as gr
import network_tangent_reference as nt

pytestmark = pytest.mark.gpu
CHAIN = ["emb", "lat", "mod"]
SWITCHES = ("SWIFTK_JVP_UNFUSED", "SWIFTK_TRAIN_FP32_STREAM", "SWIFTK_PAD_HEADS")
FORMS = {   # operand type, environment, jvp() arguments, (dim, heads) of the net
    "bf16": (torch.bfloat16, {}, {}, (None, None)),
    "unfused": (torch.bfloat16, {"SWIFTK_JVP_UNFUSED": "1"}, {}, (None, None)),
    "fp32-stream": (torch.bfloat16, {"SWIFTK_TRAIN_FP32_STREAM": "1"}, {}, (None, None)),
    "save-ctx": (torch.bfloat16, {}, dict(save_ctx=True, want_logvar=True), (None, None)),
    "padded-lanes": (torch.bfloat16, {"SWIFTK_PAD_HEADS": "2"}, {}, (768, 12)),
    "fp32": (torch.float32, {}, {}, (None, None)),
}
_state = {}   # nets, engines and engine runs (device tensors) shared by the tests of this module


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield torch.device("cuda", 0)
    _state.clear()


def _net(dev, dim, heads):
    if ("net", dim, heads) not in _state:
        from swift_amd.models.precond import PassPrecond
        cfg, mcfg, state = nt.net(dim, heads)
        net = PassPrecond(mcfg, img_resolution=[64, 64], img_channels=nt.NV, condition_channels=nt.NV + nt.NF, auxiliary_dim=1)
        net.load_state_dict(state)
        _state["net", dim, heads] = net.to(dev)
    return _state["net", dim, heads]


def _switch(monkeypatch, form):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMS[form][1].items():
        monkeypatch.setenv(k, v)


def _engine(dev, form):
    """A fresh engine per form (the switches are read at construction or per pass; ``_switch`` has set them)."""
    if ("engine", form) not in _state:
        from swift_amd.jvp_engine import SwinJvpEngine
        dtype, _, _, (dim, heads) = FORMS[form]
        _state["engine", form] = SwinJvpEngine(_net(dev, dim, heads).model, dtype)
    return _state["engine", form]


def _call(eng, ins, dev, **kw):
    from swift_amd.models.precond import _process_auxiliary
    i = {k: v.to(dev) for k, v in ins.items()}
    return eng.jvp([i["x"], i["cond"]], i["vx"], i["t"], i["vt"], _process_auxiliary(i["aux"], 1, nt.B, dev), **kw)


def _run(dev, form, direction):
    """One tapped pass: {"out": dF, "tok0": ..., "mod": ..., ...} as ``tangent`` and ``primal`` (device tensors)."""
    key = ("run", form, direction)
    if key not in _state:
        eng = _engine(dev, form)
        taps = {}
        res = _call(eng, nt.case(nt.SEEDS[FORMS[form][3]], direction), dev, taps=taps, **FORMS[form][2])
        torch.cuda.synchronize()
        names = CHAIN + nt.stream_taps(len(eng.L))
        assert set(taps) == set(names) | {"d" + n for n in names}, sorted(taps)
        assert all(v.dtype == torch.float32 for v in taps.values())
        tangent, primal = {n: taps["d" + n] for n in names}, {n: taps[n] for n in CHAIN}
        if FORMS[form][2].get("save_ctx"):
            tangent["out"], primal["out"], primal["logvar"] = res[0].clone(), res[1].clone(), res[2].clone().view(-1, 1)
        else:
            tangent["out"] = res.clone()
        _state[key] = dict(tangent=tangent, primal=primal)
    return _state[key]


def _cpu(values, names):
    return {n: values[n].float().cpu() for n in names}


def _ratios(recs):
    worst = {}
    for r in recs:
        worst[r["name"]] = max(worst.get(r["name"], 0.0), r["worst"] / r["yardstick"])
    return ", ".join(f"{k[len(gr.FIELD):]} {v:.2f}" for k, v in worst.items())


def _hold_bf16(dev, form, direction):
    """A bf16-operand form in one direction: stream and output per slice against 2 x the emulations, the chain against 1e-5."""
    dim, heads = FORMS[form][3]
    cfg = nt.net(dim, heads)[0]
    ref = nt.truth_and_yardsticks(direction, dim, heads)
    got = _run(dev, form, direction)
    names = ["out"] + nt.stream_taps(cfg.depth)[1 if direction == "time" else 0:]
    recs, bad = nt.score_bf16(f"{form} engine, direction {direction}", _cpu(got["tangent"], names), ref, cfg, names)
    print(f"{form} / {direction}: worst slice as a ratio of its yardstick: {_ratios(recs)}")
    _, bad_c = nt.score_fp32(f"{form} engine, direction {direction}, chain tangents", _cpu(got["tangent"], CHAIN), ref[0].tangent, cfg,
                             CHAIN, nt.FP32_CHAIN)
    _, bad_p = nt.score_fp32(f"{form} engine, chain values", _cpu(got["primal"], CHAIN), ref[0].primal, cfg, CHAIN, nt.FP32_CHAIN)
    assert not (bad + bad_c + bad_p), (form, direction, bad + bad_c + bad_p)
    return ref, got, cfg


# --------------------------------------------------------------------------- 1. the tap changes nothing


@pytest.mark.parametrize("form", ["bf16", "fp32"])
def test_tap_is_inert(dev, monkeypatch, form):
    """Without taps, with taps, and replayed from the captured graph: the same bits; a tapped call leaves the graph cache alone."""
    from swift_amd import graphs
    from swift_amd.jvp_engine import SwinJvpEngine
    _switch(monkeypatch, form)
    eng = SwinJvpEngine(_net(dev, None, None).model, FORMS[form][0])
    ins = nt.case(nt.SEED, "both")
    outs = [_call(eng, ins, dev).clone()]                       # first sight of the signature: eager
    seen = dict(eng.graphs._seen)
    taps = {}
    outs.append(_call(eng, ins, dev, taps=taps).clone())
    assert len(taps) == 2 * (3 + 1 + 2 * len(eng.L)) and eng.graphs._seen == seen and not eng.graphs._graphs
    outs.append(_call(eng, ins, dev).clone())                   # captured and replayed
    outs.append(_call(eng, ins, dev).clone())                   # replayed
    if graphs.enabled():
        assert len(eng.graphs._graphs) == 1
    outs.append(_call(eng, ins, dev, taps={}).clone())          # eager again, beside the captured sequence
    outs.append(_call(eng, ins, dev).clone())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
    for k, o in enumerate(outs[1:], 1):
        assert torch.equal(o.view(torch.int32), outs[0].view(torch.int32)), f"call {k} differs from the first"
    # what a tap holds is a copy: the next pass does not move it
    kept = taps["dx0"].clone()
    _call(eng, nt.case(nt.SEED, "time"), dev, taps={})
    torch.cuda.synchronize()
    assert torch.equal(kept, taps["dx0"])


# --------------------------------------------------------------------------- 2. bf16 operands


@pytest.mark.parametrize("direction", ["both", "time"])
def test_bf16_engine_default_forms_slices_vs_fp64(dev, monkeypatch, direction):
    """Fused swiftk_gemm_jvp, pair stream, shared buffers: what the trainer runs."""
    _switch(monkeypatch, "bf16")
    _hold_bf16(dev, "bf16", direction)


@pytest.mark.parametrize("form", ["unfused", "fp32-stream", "save-ctx", "padded-lanes"])
def test_bf16_engine_other_forms_slices_vs_fp64(dev, monkeypatch, form):
    _switch(monkeypatch, form)
    eng = _engine(dev, form)
    if form == "padded-lanes":
        assert (eng.hd0, eng.hd, eng.inner) == (64, 80, 960)
    for direction in ("time", "both"):
        ref, got, cfg = _hold_bf16(dev, form, direction)
        if form == "save-ctx":
            # per-layer buffers hold what the shared set held: the same tangent bits; and the primal rows are a forward pass
            _switch(monkeypatch, "bf16")
            shared = _run(dev, "bf16", direction)
            _switch(monkeypatch, form)
            for n in shared["tangent"]:
                assert torch.equal(got["tangent"][n].view(torch.int32), shared["tangent"][n].view(torch.int32)), (direction, n)
            _, bad = nt.score_bf16(f"{form} engine, F", _cpu(got["primal"], ["out"]), ref, cfg, ["out"], kind="primal")
            _, bad_l = nt.score_fp32(f"{form} engine, logvar", _cpu(got["primal"], ["logvar"]),
                                     dict(logvar=ref[0].primal["logvar"].view(-1, 1)), cfg, ["logvar"], nt.FP32_CHAIN)
            assert not (bad + bad_l), bad + bad_l


# --------------------------------------------------------------------------- 3. fp32 operands


@pytest.mark.parametrize("direction", ["both", "time"])
def test_fp32_engine_slices_vs_fp64(dev, monkeypatch, direction):
    _switch(monkeypatch, "fp32")
    cfg = nt.net()[0]
    truth, f32 = nt.run(direction, "f64"), nt.run(direction, "f32")
    got = _run(dev, "fp32", direction)
    names = ["out"] + nt.stream_taps(cfg.depth)[1 if direction == "time" else 0:]
    ro, _ = nt.score_fp32(f"fp32 oracle, direction {direction}", f32.tangent, truth.tangent, cfg, names, nt.FP32_NETWORK, show=False)
    re, bad = nt.score_fp32(f"fp32 engine, direction {direction}", _cpu(got["tangent"], names), truth.tangent, cfg, names, nt.FP32_NETWORK,
                            show=False)
    print(f"fp32 engine, direction {direction}: worst slice against fp64 (beside the fp32 oracle's own)")
    for e, o in zip(re, ro):
        print(f"  {e['name']:14s} [{e['slicing']:15s}] engine {e['worst']:.3e} at {e['index']:3d} of {e['n']:3d}   oracle {o['worst']:.3e}")
    _, bad_c = nt.score_fp32("fp32 engine, chain tangents", _cpu(got["tangent"], CHAIN), truth.tangent, cfg, CHAIN, nt.FP32_CHAIN)
    _, bad_p = nt.score_fp32("fp32 engine, chain values", _cpu(got["primal"], CHAIN), truth.primal, cfg, CHAIN, nt.FP32_CHAIN)
    assert not (bad + bad_c + bad_p), bad + bad_c + bad_p


# --------------------------------------------------------------------------- 4. exact zeros


@pytest.mark.parametrize("form", list(FORMS))
def test_zero_direction_is_exactly_zero_and_samples_do_not_mix(dev, monkeypatch, form):
    """Every tangent rule is linear in the tangent operands, so these hold exactly; a failure means one sample read another's
    modulation row or tangent rows."""
    _switch(monkeypatch, form)
    silent, both, time = (_run(dev, form, d)["tangent"] for d in ("silent", "both", "time"))
    for n, v in silent.items():
        assert bool(torch.isfinite(v).all()), n
        nz = torch.nonzero(v[1])
        assert nz.numel() == 0, f"{form}: d{n} of the silent sample 1 is not zero at {tuple(int(q) for q in nz[0])} ({nz.shape[0]} places)"
        for b in (0, 2):
            diff = torch.nonzero(v[b].view(torch.int32) != both[n][b].view(torch.int32))
            assert diff.numel() == 0, (f"{form}: d{n} of sample {b} moved when sample 1 lost its tangent, first at "
                                       f"{tuple(int(q) for q in diff[0])} ({diff.shape[0]} places)")
    nz = torch.nonzero(time["tok0"])
    assert nz.numel() == 0, f"{form}: dtok0 in the time direction is not zero at {tuple(int(q) for q in nz[0])}"
    assert all(float(time[n].abs().max()) > 0 for n in time if n != "tok0")
