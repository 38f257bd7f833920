"""End-to-end training gradients scored slice by slice against fp64 autograd of the CPU oracle (TEST INFRASTRUCTURE, no GPU).

A cosine per whole parameter tensor is blind to size (a gradient twice too large has cosine 1) and to defects in a part of
a tensor (one head's rows of ``to_qkv.weight`` are 1/36 of it).  Here every gradient is cut into the units the kernels
produce it in -- heads, 256-wide GEMM tiles, windows, channels -- and each unit is held to

    ||got_s - truth_s|| / max(||truth_s||, median_s ||truth_s||)  <=  2 x yardstick,

where truth is the oracle in fp64 and the yardstick is the worst such slice error of the oracle's own two bf16 emulations
(``emulate_bf16=True`` and ``"offset0"``, whose cast pairs round the gradients as well): the distance from fp64 of a bf16
implementation nobody doubts, measured on the same operands in the same test, never stored.  The factor 2 is the
project's convention for bf16 yardsticks (DESIGN, "Exact tests of the two hot-path families").

A slice whose truth is exactly zero (a head beyond the ln 100 clamp) must come back exactly zero, and a slicing no bf16
rounding reaches is held to FP32_BOUND (see there).  Rounding points added to the emulations beyond the oracle's own: none
(measured on an MI355X the engine sits at 0.9 ... 1.45 of the yardsticks; the table is in DESIGN, section 2).
"""
import math

import torch

from oracle.swinv2 import OracleNet

FACTOR = 2.0          # bound = FACTOR x yardstick
FLOOR = 0.1           # a slice whose truth is below FLOOR x the median slice norm is "under the floor"
INPUT = "input:"      # key prefix of input gradients in a gradient dictionary
FIELD = "field:"      # key prefix of a value (or tangent) of the network pass: out, tok0, xmid{i}, x{i}, mod, emb, lat
# Where no bf16 rounding reaches a gradient (the logvar head: fp32 latent MLP, fp32 small-Linear backward) both emulations ARE
# the fp32 oracle, the yardstick is that one summation order's accident (6e-7; exactly 0 for the logvar bias, a sum of B
# numbers) and 2 x it would ask an atomically accumulated fp32 sum to be bit-exact.  Such a slicing is held to the bound the
# fp32 oracle itself is held to against fp64 (tests/test_gradient_reference_cpu.py): 1e-4 per slice, two orders under any
# bf16 yardstick, so it decides nothing where bf16 is involved.
FP32_BOUND = 1e-4


# --------------------------------------------------------------------------- oracle runs


def oracle_run(cfg, state, img_channels, condition_channels, loss_fn, inputs, wrt=(), dtype=torch.float64, emulate_bf16=False):
    """One autograd run of ``loss_fn(onet, inputs)`` over an ``OracleNet`` whose state dict and ``inputs`` (a dict of
    tensors) are cast to ``dtype``.  Returns ``{state key: gradient} | {"input:" + name: gradient for name in wrt}``."""
    def cast(v):
        return v.detach().to(dtype) if v.is_floating_point() else v

    st = {k: cast(v).clone().requires_grad_(True) for k, v in state.items()}
    ins = {k: (cast(v).clone() if torch.is_tensor(v) else v) for k, v in inputs.items()}
    for k in wrt:
        ins[k].requires_grad_(True)
    onet = OracleNet(cfg, st, img_channels, condition_channels)
    onet.emulate_bf16 = emulate_bf16
    loss_fn(onet, ins).backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in st.items()}
    grads.update({INPUT + k: ins[k].grad.detach() for k in wrt})
    return grads


def oracle_gradients(cfg, state, img_channels, condition_channels, loss_fn, inputs, wrt=()):
    """(truth, yard_a, yard_b): the oracle in fp64, and in fp32 with ``emulate_bf16=True`` / ``"offset0"``."""
    run = lambda dtype, emu: oracle_run(cfg, state, img_channels, condition_channels, loss_fn, inputs, wrt, dtype, emu)
    return run(torch.float64, False), run(torch.float32, True), run(torch.float32, "offset0")


# --------------------------------------------------------------------------- the nets and the engine-level case

SMALLB = dict(img=(64, 64), n_vars=69, n_forc=3, window=(16, 16), shift=(8, 8), patch=(2, 2), dim=1056, heads=12, depth=2)
NETS = {"smooth": 0.5, "hostile": 4.0, "default": None}   # clamp of every *.scale (ln 100 = 4.605; detinit puts one head per layer at 5.0)


def small_net(kind, seed, logvar=True, dim=None, heads=None):
    """(SwinCfg, PassPrecond model config, state dict) of the SMALLB net (32x32 token grid, four windows, one layer shifted,
    depth 2) with its logit scales clamped as ``NETS[kind]`` says."""
    from oracle.swinv2 import SwinCfg
    from swift_amd.utils.detinit import swinv2_state
    c = dict(SMALLB, dim=dim or SMALLB["dim"], heads=heads or SMALLB["heads"])
    nv, nf = c["n_vars"], c["n_forc"]
    state = swinv2_state(grid=(32, 32), in_channels=2 * nv + nf, out_channels=nv, patch_size=(2, 2), depth=c["depth"],
                         dim=c["dim"], heads=c["heads"], logvar=logvar, seed=seed)
    if NETS[kind] is not None:
        for k in state:
            if k.endswith(".scale"):
                state[k] = state[k].clamp(max=NETS[kind])
    cfg = SwinCfg(img_resolution=c["img"], in_channels=2 * nv + nf, out_channels=nv, window_size=c["window"], shift_size=c["shift"],
                  patch_size=c["patch"], depth=c["depth"], dim=c["dim"], heads=c["heads"], auxiliary_dim=1, logvar=logvar)
    mcfg = dict(_target_="swift.models.swinv2.SwinV2", window_size=list(c["window"]), shift_size=list(c["shift"]),
                patch_size=list(c["patch"]), depth=c["depth"], dim=c["dim"], heads=c["heads"], logvar=logvar)
    return cfg, mcfg, state


def engine_case(B=2, seed=21):
    """Operands of the engine-level case (those of test_gpu_train.py::test_train_engine_gradients_vs_oracle_autograd at
    B = 2; a third sample with its own t and aux at B = 3) and its loss closure sum(y R) + sum(logvar r)."""
    from swift_amd.utils.detinit import det_normal
    nv, nf = SMALLB["n_vars"], SMALLB["n_forc"]
    ins = dict(x=det_normal((B, nv, 64, 64), seed, "x"), cond=det_normal((B, nv + nf, 64, 64), seed, "cond"),
               t=torch.tensor([0.5, 1.4, 0.9][:B]), aux=torch.tensor([[0.6], [1.2], [0.3]][:B]),
               R=det_normal((B, nv, 64, 64), seed, "R"), rl=torch.tensor([0.7, -0.4, 0.25][:B]))

    def loss_fn(onet, i):
        y, lv = onet(i["x"], i["t"], i["cond"], i["aux"], return_logvar=True)
        return (y * i["R"]).sum() + (lv * i["rl"]).sum()

    return ins, loss_fn


# --------------------------------------------------------------------------- slicings


def _blocks(n, width):
    return torch.arange(n) // width


def slicings(name, shape, cfg):
    """The natural units of a gradient in the reference's (checkpoint) shapes: ``{slicing: int64 labels}``, the labels
    broadcastable to ``shape`` (size 1 along every axis a slice runs the whole length of)."""
    shape = tuple(shape)
    heads, hd, d, m = cfg.heads, cfg.head_dim, cfg.dim, cfg.mlp_dim
    col = lambda lab: lab.view(-1, 1)                   # one label per row of a matrix
    row = lambda lab: lab.view(1, -1)                   # one label per column
    out = {}
    if name.startswith(INPUT):                          # [B, C, H, W]: per (sample, channel)
        B, C = shape[:2]
        out["sample,channel"] = torch.arange(B * C).view(B, C, 1, 1)
    elif name.startswith(FIELD):                        # a value of the network pass itself (tests/network_tangent_reference.py)
        tap = name[len(FIELD):]
        B = shape[0]
        smp = torch.arange(B)
        gh, gw = cfg.grid
        wh, ww = cfg.window_size
        nwx = gw // ww
        nW = (gh // wh) * nwx

        def windows(sh):                                # window of every token under roll(-sh) + partition (oracle window_token_index)
            y, x = torch.arange(gh).view(-1, 1), torch.arange(gw).view(1, -1)
            return ((y - sh[0]) % gh // wh) * nwx + (x - sh[1]) % gw // ww

        if tap == "out":                                # [B, C, H, W]
            C = shape[1]
            p1, p2 = cfg.patch_size
            px = lambda w: w.repeat_interleave(p1, 0).repeat_interleave(p2, 1).view(1, 1, gh * p1, gw * p2)
            out["sample,channel"] = torch.arange(B * C).view(B, C, 1, 1)
            out["sample,window"] = smp.view(B, 1, 1, 1) * nW + px(windows((0, 0)))
            out["sample,shifted"] = smp.view(B, 1, 1, 1) * nW + px(windows(cfg.shift_size))
        elif tap == "mod":                              # [B, 2 depth, 2, d]: slot, scale | shift
            out["sample,slot,half"] = torch.arange(B * shape[1] * 2).view(B, shape[1], 2, 1)
        elif len(shape) == 2:                           # [B, d]: emb, lat
            out["sample"] = smp.view(B, 1)
        else:                                           # the residual stream [B, gh gw, d] after tok0 / xmid{i} / x{i}
            i = int(tap.lstrip("xmidtok"))
            sh = cfg.shift_size if (tap != "tok0" and any(cfg.shift_size) and i % 2) else (0, 0)   # the layer that wrote it
            n256, n352 = -(-B * gh * gw // 256), -(-d // 352)
            rows = (smp.view(B, 1) * (gh * gw) + torch.arange(gh * gw).view(1, -1)).view(B, -1, 1)
            out["sample,window"] = smp.view(B, 1, 1) * nW + windows(sh).reshape(1, -1, 1)
            out["sample,headblk"] = smp.view(B, 1, 1) * -(-d // hd) + _blocks(d, hd).view(1, 1, -1)
            out["tile256x352"] = rows // 256 * n352 + _blocks(d, 352).view(1, 1, -1)   # the GEMM's output tile over [B gh gw, d]
            assert int(out["tile256x352"].max()) + 1 == n256 * n352
    elif name.endswith("to_qkv.weight"):                # rows [head][q | k | v][hd] (oracle/swinv2.py cosine_window_attention)
        r = torch.arange(shape[0])
        out["third,head"] = col((r // hd) % 3 * heads + r // (3 * hd))
        out["col256"] = row(_blocks(shape[1], 256))
    elif name.endswith("wo.weight"):
        out["head"] = row(_blocks(shape[1], hd))
        out["row256"] = col(_blocks(shape[0], 256))
    elif name.endswith("w1.weight"):                    # rows [gate (m) | up (m)]
        r = torch.arange(shape[0])
        out["half,row256"] = col(r // m * -(-m // 256) + r % m // 256)
    elif name.endswith("w2.weight"):
        out["col256"] = row(_blocks(shape[1], 256))
    elif name.endswith(".scale"):                       # [1, heads, 1, 1]
        out["head"] = torch.arange(heads).view(shape)
    elif name.endswith("pos_embed"):                    # [1, gh gw, d], tokens row-major
        gh, gw = cfg.grid
        wh, ww = cfg.window_size
        y, x = torch.arange(gh).view(-1, 1), torch.arange(gw).view(1, -1)
        out["window"] = ((y // wh) * (gw // ww) + x // ww).reshape(1, -1, 1)
        out["row16"] = (y * -(-gw // 16) + x // 16).reshape(1, -1, 1)
    elif name.endswith("patch_embed.emb.weight"):       # column (i1 p2 + i2) C + c (oracle/swinv2.py patchify)
        out["channel"] = row(torch.arange(shape[1]) % cfg.in_channels)
    elif name.endswith("modulation.weight") or name.endswith("modulation.bias"):   # [scale half (d) | shift half (d)]
        r = torch.arange(shape[0])
        lab = r // d * -(-d // 96) + r % d // 96
        out["half,blk96"] = col(lab) if len(shape) == 2 else lab
    elif name.endswith("head.head.0.weight"):           # row (c p1 + i1) p2 + i2 (oracle/swinv2.py unpatchify)
        out["variable"] = col(_blocks(shape[0], cfg.patch_size[0] * cfg.patch_size[1]))
    elif len(shape) == 2 and shape[0] > 1:
        out["row96"] = col(_blocks(shape[0], 96))
    else:
        out["blk96"] = _blocks(shape[-1], 96).view((1,) * (len(shape) - 1) + (-1,))
    return out


# --------------------------------------------------------------------------- score


def _slice_sums(v, lab):
    """Sum of ``v`` per label: first along the axes a slice runs the whole length of, then by label."""
    dims = [i for i in range(v.dim()) if lab.shape[i] == 1 and v.shape[i] != 1]
    r = v.sum(dim=dims, keepdim=True) if dims else v
    return torch.bincount(lab.expand(r.shape).reshape(-1), weights=r.reshape(-1), minlength=int(lab.max()) + 1)


def _errors(d2, g2, t2, lab):
    d2, g2, t2 = _slice_sums(d2, lab), _slice_sums(g2, lab), _slice_sums(t2, lab)
    tn = t2.sqrt()
    err = d2.sqrt() / torch.maximum(tn, tn.median()).clamp_min(1e-300)
    zero = t2 == 0
    err[zero] = torch.where(g2[zero] == 0, 0.0, math.inf).to(err.dtype)
    return err, tn


def slice_errors(got, truth, labels):
    """Per slice: ||got_s - truth_s|| / max(||truth_s||, median_s ||truth_s||), and ||truth_s||.  A slice whose truth is
    exactly zero scores 0 if ``got`` is exactly zero there and inf otherwise."""
    g, t = got.detach().double(), truth.detach().double()
    return _errors((g - t) ** 2, g ** 2, t ** 2, labels)


def score(name, got, truth, yard_a, yard_b, cfg):
    """One record per slicing of ``name``: worst slice error of ``got`` and its index, the yardstick (the larger of the two
    emulations' worst slice errors), the bound, the whole-tensor relative L2 and the cosine the older checks look at.

    Conditions of the measurement, asserted here: at most one slice per slicing lies under the floor (a slice whose truth
    is exactly zero -- a head beyond the ln 100 clamp -- is not floored but scored exactly), and every tensor but the
    logvar head's has a nonzero truth."""
    assert tuple(got.shape) == tuple(truth.shape) == tuple(yard_a.shape) == tuple(yard_b.shape), (name, got.shape, truth.shape)
    g, t, a, b = (v.detach().double() for v in (got, truth, yard_a, yard_b))
    tnorm = float(t.norm())
    assert tnorm > 0 or "logvar" in name, f"{name}: the fp64 gradient is identically zero, nothing is scored"
    rel = float((g - t).norm()) / max(tnorm, 1e-300)
    cos = float((g * t).sum()) / max(float(g.norm()) * tnorm, 1e-300)
    t2 = t ** 2
    sq = [((v - t) ** 2, v ** 2) for v in (g, a, b)]
    recs = []
    for sl, lab in slicings(name, truth.shape, cfg).items():
        (err, tn), (ea, _), (eb, _) = (_errors(d2, v2, t2, lab) for d2, v2 in sq)
        under = int(((tn < FLOOR * tn.median()) & (tn > 0)).sum())
        assert under <= 1, f"{name} [{sl}]: {under} of {tn.numel()} slices under the floor"
        yard = max(float(ea.max()), float(eb.max()))
        i = int(err.argmax())
        recs.append(dict(name=name, slicing=sl, worst=float(err[i]), index=i, n=int(tn.numel()), yardstick=yard,
                         bound=max(FACTOR * yard, FP32_BOUND), rel_l2=rel, cos=cos, under=under))
    return recs


def score_all(got, truth, yard_a, yard_b, cfg, title=None, show=True):
    """``score`` over every key of ``got`` (all must be in ``truth``); prints one line per slicing."""
    recs = []
    if show and title:
        print(title)
    for k in got:
        for r in score(k, got[k], truth[k], yard_a[k], yard_b[k], cfg):
            recs.append(r)
            if show:
                ratio = r["worst"] / r["yardstick"] if r["yardstick"] > 0 else (0.0 if r["worst"] == 0 else math.inf)
                print(f"  {k:52s} rel-L2 {r['rel_l2']:.3e}  [{r['slicing']:14s}] worst {r['worst']:.3e} / yard "
                      f"{r['yardstick']:.3e} = {ratio:5.2f}  at {r['index']} of {r['n']}")
    return recs


def over(recs):
    """The records whose worst slice exceeds the bound, max(2 x yardstick, FP32_BOUND)."""
    return [r for r in recs if not r["worst"] <= r["bound"]]


def cosine_passes(recs, floor):
    """What the whole-tensor cosine check says of the same gradients."""
    return all(r["cos"] > floor for r in recs)
