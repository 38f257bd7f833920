"""CPU checks of tests/gradient_reference.py: the per-slice rule is satisfiable (the two bf16 emulations of the oracle meet it
against each other), it flags every planted defect, and the whole-tensor cosine floors of the older end-to-end checks
(0.99 / 0.999) do not flag the size defects and the one-slice defect -- the gap tests/test_gpu_train_gradients.py closes.

Configuration: the SMALLB net of test_gpu_train.py (64x64 image, 16x16 windows, shift (8, 8), dim 1056, 12 heads, depth 2) at
B = 2 with the operands of test_train_engine_gradients_vs_oracle_autograd, on the three nets of gradient_reference.NETS."""
import math

import pytest
import torch

import gradient_reference as gr

WRT = ("x", "cond")
_cache = {}


def runs(kind):
    """(cfg, truth fp64, emulation a, emulation b, fp32 oracle) of the engine-level case on net ``kind``; computed once."""
    if kind not in _cache:
        cfg, _, state = gr.small_net(kind, 21)
        ins, loss_fn = gr.engine_case(2)
        nv, nf = gr.SMALLB["n_vars"], gr.SMALLB["n_forc"]
        t, a, b = gr.oracle_gradients(cfg, state, nv, nv + nf, loss_fn, ins, WRT)
        f32 = gr.oracle_run(cfg, state, nv, nv + nf, loss_fn, ins, WRT, torch.float32, False)
        _cache[kind] = (cfg, t, a, b, f32)
    return _cache[kind]


def _key(t, suffix):
    return next(k for k in t if k.endswith(suffix))


def _verdict(cfg, t, a, b, name, planted, what):
    """Score ``planted`` (a damaged copy of emulation a's ``name``): (flagged by the slice rule, passes cosine 0.99, 0.999)."""
    recs = gr.score(name, planted, t[name], a[name], b[name], cfg)
    flagged = bool(gr.over(recs))
    c99, c999 = gr.cosine_passes(recs, 0.99), gr.cosine_passes(recs, 0.999)
    worst = max(recs, key=lambda r: r["worst"] / max(r["bound"], 1e-300))
    print(f"{what:58s} slice rule {'FLAGS ' if flagged else 'passes'} (worst {worst['worst']:.3e} vs bound {worst['bound']:.3e} "
          f"[{worst['slicing']}] at {worst['index']}); cosine {recs[0]['cos']:.5f}: 0.99 {'passes' if c99 else 'FLAGS'}, "
          f"0.999 {'passes' if c999 else 'FLAGS'}")
    return flagged, c99, c999


@pytest.mark.parametrize("kind", list(gr.NETS))
def test_emulations_meet_the_rule_against_each_other_and_fp32_is_the_truth(kind):
    """Each emulation's worst slice is within 2 x the other's on every slicing (so 2 x the larger is a bound a correct bf16
    implementation meets and a 5 % defect does not); the fp32 oracle is within 1e-4 of fp64 on every slice, three orders
    under the bf16 yardsticks, so either may serve as truth.  (Asserted on the smooth and the hostile net.  On the default net,
    whose clamped heads run logits up to 100, fp32 is 1.2e-4 from fp64 on one pos_embed row segment: printed, and no test
    substitutes fp32 for the truth.)"""
    cfg, t, a, b, f32 = runs(kind)
    n_under, worst_f32 = 0, 0.0
    for k in t:
        ra, rb = gr.score(k, a[k], t[k], a[k], b[k], cfg), gr.score(k, b[k], t[k], a[k], b[k], cfg)
        for x, y, f in zip(ra, rb, gr.score(k, f32[k], t[k], a[k], b[k], cfg)):
            n_under += x["under"]
            assert x["worst"] <= 2 * y["worst"] and y["worst"] <= 2 * x["worst"], (k, x["slicing"], x["worst"], y["worst"])
            worst_f32 = max(worst_f32, f["worst"])
            if kind != "default":
                assert f["worst"] <= gr.FP32_BOUND, (k, f["slicing"], f["worst"])
            if kind == "smooth" and not k.endswith(".scale") and "logvar" not in k:
                assert x["bound"] < 3e-2, (k, x["slicing"], x["bound"])
    print(f"{kind}: {n_under} slices under the floor in total; fp32 oracle vs fp64, worst slice {worst_f32:.2e}")
    if kind == "smooth":
        assert n_under == 0


def test_every_slicing_partitions_its_tensor_into_the_units_it_names():
    cfg, t, *_ = runs("smooth")
    want = {"to_qkv.weight": {"third,head": 36, "col256": 5}, "wo.weight": {"head": 12, "row256": 5}, "w1.weight": {"half,row256": 22},
            "w2.weight": {"col256": 11}, ".0.scale": {"head": 12}, "pos_embed": {"window": 4, "row16": 64},
            "patch_embed.emb.weight": {"channel": 141}, "0.norm.modulation.weight": {"half,blk96": 22},
            "0.norm.modulation.bias": {"half,blk96": 22}, "head.head.0.weight": {"variable": 69}, "norm.norm.weight": {"blk96": 11},
            gr.INPUT + "x": {"sample,channel": 138}, gr.INPUT + "cond": {"sample,channel": 144}}
    for suffix, counts in want.items():
        k = _key(t, suffix)
        sl = gr.slicings(k, t[k].shape, cfg)
        assert {n: int(l.max()) + 1 for n, l in sl.items()} == counts, k
        for lab in sl.values():
            sizes = torch.bincount(lab.expand(t[k].shape).reshape(-1))
            assert int(sizes.min()) > 0 and int(sizes.sum()) == t[k].numel()
    # the row blocks are where the oracle reads them: head 1's k rows of to_qkv, the up half of w1, one variable's 4 head rows
    k = _key(t, "0.0.to_qkv.weight")
    lab = gr.slicings(k, t[k].shape, cfg)["third,head"].reshape(-1)
    assert lab[3 * 88 + 88] == 1 * 12 + 1 and lab[3 * 88 + 2 * 88 - 1] == 13 and lab[3 * 88 + 2 * 88] == 2 * 12 + 1
    k = _key(t, "0.1.w1.weight")
    lab = gr.slicings(k, t[k].shape, cfg)["half,row256"].reshape(-1)
    assert lab[2815] == 10 and lab[2816] == 11 and lab[2816 + 256] == 12
    k = _key(t, "patch_embed.emb.weight")
    lab = gr.slicings(k, t[k].shape, cfg)["channel"].reshape(-1)
    assert [int(i) for i in (lab == 69).nonzero().reshape(-1)] == [69, 141 + 69, 282 + 69, 423 + 69]   # first condition channel


def test_size_defects_are_flagged_and_the_cosine_floors_miss_them():
    for kind, factor in (("hostile", 2.0), ("smooth", 1.05)):
        cfg, t, a, b, _ = runs(kind)
        for k in t:
            if "logvar" in k or (factor < 2 and k.endswith(".scale")):   # (the per-head scale yardstick, 1.1e-1, is above 5 %)
                continue
            flagged, c99, c999 = _verdict(cfg, t, a, b, k, a[k] * factor, f"{kind}: {k[6:]} x {factor}")
            # (0.999 is the floor the suite uses on smooth nets only: at clamp 4.0 the undamaged emulation is already under it)
            assert flagged and c99 and (c999 or kind != "smooth"), k


def test_one_slice_five_percent_is_flagged_on_the_smooth_net_and_the_cosine_floors_miss_it():
    """The largest slice of every slicing x 1.05: 33 of 35 sliced tensors in the issue's count (all but the per-head scales)."""
    cfg, t, a, b, _ = runs("smooth")
    n = 0
    for k in t:
        if "logvar" in k or k.endswith(".scale"):
            continue
        for sl, lab in gr.slicings(k, t[k].shape, cfg).items():
            _, tn = gr.slice_errors(a[k], t[k], lab)
            planted = torch.where(lab.expand(t[k].shape) == int(tn.argmax()), a[k] * 1.05, a[k])
            flagged, c99, c999 = _verdict(cfg, t, a, b, k, planted, f"smooth: {k[6:]} [{sl}] largest slice x 1.05")
            assert flagged and c99 and c999, (k, sl)
            n += 1
    assert n >= 33


def test_layout_defects_are_flagged():
    cfg, t, a, b, _ = runs("hostile")
    seen = {}

    def plant(suffix, what, fn):
        k = _key(t, suffix)
        g = a[k].clone()
        fn(g)
        seen[what] = _verdict(cfg, t, a, b, k, g, f"hostile: {k[6:]}: {what}")
        assert seen[what][0], what

    def zero_tile(g):
        g[2816 + 512: 2816 + 768] = 0
    plant("1.1.w1.weight", "one 256-row tile zeroed", zero_tile)

    def swap_heads(g):
        g[:, 2 * 88: 3 * 88], g[:, 7 * 88: 8 * 88] = g[:, 7 * 88: 8 * 88].clone(), g[:, 2 * 88: 3 * 88].clone()
    plant("0.0.wo.weight", "heads 2 and 7 swapped", swap_heads)

    def swap_qkv_heads(g):
        g[2 * 264: 3 * 264], g[7 * 264: 8 * 264] = g[7 * 264: 8 * 264].clone(), g[2 * 264: 3 * 264].clone()
    plant("1.0.to_qkv.weight", "heads 2 and 7 swapped", swap_qkv_heads)

    def swap_halves(g):
        g[:2816], g[2816:] = g[2816:].clone(), g[:2816].clone()
    plant("0.1.w1.weight", "gate and up halves swapped", swap_halves)

    def drop_window(g):
        g.view(32, 32, -1)[16:, :16] = 0
    plant("pos_embed", "window 2 dropped", drop_window)

    def one_channel(g):
        g[:, 100::141] = 0
    plant("patch_embed.emb.weight", "one condition channel zeroed", one_channel)
    # one channel of 141 is the kind of defect the tensor cosine cannot see
    assert seen["one condition channel zeroed"][1]


def test_clamped_head_must_be_exactly_zero():
    cfg, t, a, b, _ = runs("default")
    for i in (0, 1):
        k = _key(t, f"{i}.0.scale")
        h = (i + 1) % 12   # detinit: one head per layer at 5.0 > ln 100
        assert float(t[k].reshape(-1)[h]) == 0.0 and float(a[k].reshape(-1)[h]) == 0.0
        assert not gr.over(gr.score(k, a[k], t[k], a[k], b[k], cfg))
        g = a[k].clone()
        g.reshape(-1)[h] = 1e-6 * float(t[k].abs().max())
        flagged, c99, c999 = _verdict(cfg, t, a, b, k, g, f"default: {k[6:]}: clamped head set to 1e-6 of the largest")
        assert flagged and c99   # (0.99: the floor the suite uses on nets with sharp heads)
        err, _ = gr.slice_errors(g, t[k], gr.slicings(k, t[k].shape, cfg)["head"])
        assert math.isinf(float(err[h]))
