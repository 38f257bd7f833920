"""The forward-mode tangent of the whole denoiser, branch by branch, from the CPU oracle (TEST INFRASTRUCTURE, no GPU).

``SwinJvpEngine.jvp`` composes a dozen tangent kernels, each scored on its own elsewhere.  What the host code decides -- which
modulation slot a norm reads, that the tangent rows skip the bias and the position embedding, which layers shift, how primal and
tangent rows share a buffer -- is scored here: ``torch.func.jvp`` of the ``OracleNet`` (``jvp=True``), with the oracle's taps
(``tok0``, ``xmid{i}``, ``x{i}``), the latent chain (``emb``, ``lat``) and the modulation of every norm (``mod`` [B, 2 depth, 2, d],
recomputed from ``lat`` with the modulation Linears) returned as further outputs, so every one of them comes back as primal and
tangent.  Truth is the oracle in fp64; the yardsticks are its two bf16 emulations, whose cast pairs round tangents as they round
values; slices, floor and factor are those of tests/gradient_reference.py (``FIELD`` names in ``gr.slicings``).

Directions, all on ``small_net("smooth", SEED)`` at B = 3, every sample with its own t and aux:

  both    vx random, vt non-zero                      the tangent the sCM loss asks for
  time    vx = 0                                      1 % of ``both`` in norm, and the whole of what the dmod chain carries
  space   vt = 0                                      (CPU only: linearity)
  silent  ``both`` with vx = 0 and vt = 0 in sample 1   every tangent of that sample is exactly zero

SEED: 41 (the seed of test_gpu_train.py::test_network_tangent_vs_oracle_jvp).  At it every slicing of every fp64 tangent has no
slice under the floor in ``both`` and in ``time`` (tests/test_network_tangent_reference_cpu.py prints the smallest slice of each)
and every 2 x yardstick bound is under BOUND_CAP.  The 12-heads-of-64 net of the padded-lane form takes the next seed, 42: at 41
the oracle's own emulations are 1.6e-2 from fp64 in one (sample, channel) slice of the time direction (sample 2, channel 52),
2 x which is over the cap -- a property of those operands, decided on the CPU before any kernel runs; seeds 42 ... 45 all meet it.
"""
import torch
import torch.nn.functional as F

import gradient_reference as gr
import oracle.swinv2 as osw

NV, NF = gr.SMALLB["n_vars"], gr.SMALLB["n_forc"]
SEED, B = 41, 3
SEEDS = {(None, None): SEED, (768, 12): 42}
FP32_CHAIN = 1e-5      # emb -> lat -> mod and their tangents: fp32 small Linears on both sides (test_gpu_tangent_kernels.py's figure)
FP32_NETWORK = 1e-4    # the fp32 engine against the oracle: test_gpu_train.py::test_network_tangent_vs_oracle_jvp's figure
BOUND_CAP = 3e-2       # every 2 x yardstick bound on the smooth net lies under it (test_gpu_train_gradients.py's guard)
PRECISIONS = {"f64": (torch.float64, False), "f32": (torch.float32, False), "a": (torch.float32, True), "b": (torch.float32, "offset0")}
_cache = {}


def stream_taps(depth):
    return ["tok0"] + [n for i in range(depth) for n in (f"xmid{i}", f"x{i}")]


def case(seed, direction):
    """Operands and tangent direction: x, cond, t, aux and (vx, vt)."""
    from swift_amd.utils.detinit import det_normal
    ins = dict(x=det_normal((B, NV, 64, 64), seed, "x"), cond=det_normal((B, NV + NF, 64, 64), seed, "c"),
               vx=det_normal((B, NV, 64, 64), seed, "vx"), t=torch.tensor([0.4, 1.3, 0.8]), vt=torch.tensor([0.35, 0.2, -0.5]),
               aux=torch.tensor([[0.6], [1.2], [0.3]]))
    if direction == "time":
        ins["vx"] = torch.zeros_like(ins["vx"])
    elif direction == "space":
        ins["vt"] = torch.zeros_like(ins["vt"])
    elif direction == "silent":
        ins["vx"][1] = 0
        ins["vt"][1] = 0
    else:
        assert direction == "both", direction
    return ins


class Tangent:
    """``primal`` / ``tangent``: {"out", "logvar", "emb", "lat", "mod", "tok0", "xmid0", "x0", ...} (the primal of the stream
    taps is not kept)."""

    def __init__(self, primal, tangent):
        self.primal, self.tangent = primal, tangent


def oracle_tangent(cfg, state, inputs, dtype=torch.float64, emulate_bf16=False, drop_dshift=None):
    """``torch.func.jvp`` of the OracleNet over ``state`` (cast to ``dtype``) in (x, t) along (vx, vt).

    ``drop_dshift=(slot, lat)``: the planted defect of the CPU tests -- norm ``slot`` (2 i: attention branch of layer i, 2 i + 1:
    its feed-forward branch) takes its shift from the constant ``lat`` (the primal latent), so the primal is unchanged and
    the tangent is the true one with that norm's ``dshift`` dropped and the loss propagated downstream."""
    cast = lambda v: v.detach().to(dtype) if v.is_floating_point() else v
    st = {k: cast(v) for k, v in state.items()}
    i = {k: cast(v) for k, v in inputs.items()}
    onet = osw.OracleNet(cfg, st, NV, NV + NF)
    onet.emulate_bf16 = emulate_bf16
    p, d = onet.p, cfg.dim
    names = stream_taps(cfg.depth)
    slots = [f"transformer.layers.{l}.{j}.norm.modulation." for l in range(cfg.depth) for j in (0, 1)]

    def f(x, t):
        taps = {}
        out, lv = onet(x, t, i["cond"], i["aux"], jvp=True, taps=taps, return_logvar=True)
        lat = taps["lat"]
        emb = osw.timestep_embedding(t * cfg.timestep_weight, d) + F.linear(i["aux"] * cfg.auxiliary_dim ** 0.5,
                                                                           p["auxiliary_embed.weight"], p["auxiliary_embed.bias"])
        mod = torch.stack([F.linear(lat, p[s + "weight"], p[s + "bias"]).view(-1, 2, d) for s in slots], 1)
        return (out, lv, emb, lat, mod) + tuple(taps[n] for n in names)

    orig = osw.modulated_norm
    if drop_dshift is not None:
        slot, lat0 = drop_dshift
        target = f"transformer.layers.{slot // 2}.{slot % 2}.norm."

        def planted(x, t_lat, pp, prefix, eps=1e-6):
            if prefix != target:
                return orig(x, t_lat, pp, prefix, eps)
            xn = F.layer_norm(x, (d,), pp[prefix + "norm.weight"], pp[prefix + "norm.bias"], eps)
            w, b = pp[prefix + "modulation.weight"], pp[prefix + "modulation.bias"]
            scale, shift = F.linear(t_lat, w, b)[:, :d], F.linear(lat0.to(dtype), w, b)[:, d:]
            return xn * (1 + scale[:, None, :]) + shift[:, None, :]
        osw.modulated_norm = planted
    try:
        with torch.no_grad():
            prim, tang = torch.func.jvp(f, (i["x"], i["t"]), (i["vx"], i["vt"]))
    finally:
        osw.modulated_norm = orig
    keys = ["out", "logvar", "emb", "lat", "mod"] + names
    return Tangent({k: v for k, v in zip(keys[:5], prim)}, dict(zip(keys, tang)))


def net(dim=None, heads=None):
    key = ("net", dim, heads)
    if key not in _cache:
        _cache[key] = gr.small_net("smooth", SEEDS[dim, heads], logvar=True, dim=dim, heads=heads)
    return _cache[key]


def run(direction, precision="f64", dim=None, heads=None):
    """One oracle run on the smooth net (at ``dim`` / ``heads`` if given), computed once per process."""
    key = (direction, precision, dim, heads)
    if key not in _cache:
        cfg, _, state = net(dim, heads)
        _cache[key] = oracle_tangent(cfg, state, case(SEEDS[dim, heads], direction), *PRECISIONS[precision])
    return _cache[key]


def truth_and_yardsticks(direction, dim=None, heads=None):
    """(fp64, emulate_bf16=True, emulate_bf16="offset0") as ``gradient_reference.oracle_gradients`` orders them."""
    return tuple(run(direction, p, dim, heads) for p in ("f64", "a", "b"))


# --------------------------------------------------------------------------- scoring


def fields(values, names):
    return {gr.FIELD + n: values[n] for n in names}


def place(sl, index, n, batch=B):
    """Slice ``index`` of the ``n`` of slicing ``sl`` in words: sample and unit for the per-sample slicings, tile row and column
    for the GEMM tiles."""
    if sl == "tile256x352":
        ncol = n // (batch * 4)
        return f"row tile {index // ncol}, column tile {index % ncol}"
    parts = sl.split(",")
    if len(parts) == 1:
        return f"sample {index}"
    per = n // batch
    rest = index % per
    if len(parts) == 3:
        return f"sample {index // per}, slot {rest // 2}, {'shift' if rest % 2 else 'scale'}"
    return f"sample {index // per}, {parts[1]} {rest}"


def score_bf16(title, got, ref, cfg, names, kind="tangent", show=True):
    """``gr.score`` of ``got[name]`` for every name against ``ref = (truth, a, b)`` (``Tangent``s; ``kind`` picks the side).
    Returns (records, failures): a failure names the tap, the slicing and the slice; a bound at or over BOUND_CAP is one."""
    t, a, b = (fields(getattr(r, kind), names) for r in ref)
    recs = gr.score_all(fields(got, names), t, a, b, cfg, title=f"{title} [{kind}]", show=show)
    bad = [f"{r['name']} [{r['slicing']}] {place(r['slicing'], r['index'], r['n'], got[names[0]].shape[0])}: "
           f"{r['worst']:.3e} > {r['bound']:.3e}" for r in gr.over(recs)]
    bad += [f"{r['name']} [{r['slicing']}]: bound {r['bound']:.3e} is not under {BOUND_CAP}" for r in recs if not r["bound"] < BOUND_CAP]
    return recs, bad


def score_fp32(title, got, truth, cfg, names, bound, show=True):
    """Every slice of ``got[name]`` within ``bound`` of ``truth[name]`` (the gradient tests' slice error, no yardstick).
    Returns (records, failures)."""
    recs, bad = [], []
    if show:
        print(f"{title} [bound {bound:.0e}]")
    for n in names:
        for sl, lab in gr.slicings(gr.FIELD + n, truth[n].shape, cfg).items():
            err, tn = gr.slice_errors(got[n], truth[n], lab)
            i = int(err.argmax())
            r = dict(name=gr.FIELD + n, slicing=sl, worst=float(err[i]), index=i, n=int(tn.numel()), bound=bound)
            recs.append(r)
            if show:
                print(f"  {r['name']:20s} [{sl:16s}] worst {r['worst']:.3e} at {i} of {r['n']}")
            if not r["worst"] <= bound:
                bad.append(f"{r['name']} [{sl}] {place(sl, i, r['n'], got[n].shape[0])}: {r['worst']:.3e} > {bound:.0e}")
    return recs, bad
