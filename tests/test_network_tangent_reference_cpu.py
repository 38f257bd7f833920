"""CPU checks of tests/network_tangent_reference.py: the fp32 oracle's tangent is the fp64 one to 1e-5 per slice, the fp64
tangent is linear in its direction, a sample without a tangent stays exactly zero, every slicing meets the floor condition at
the chosen seed and every yardstick-derived bound is under 3e-2 -- and a dropped ``dshift`` of one norm, which the whole-output
bar of the older tests (8e-2) cannot see, fails the time-direction slice bounds and the dmod check that
tests/test_gpu_network_tangent.py applies to the engine."""
import pytest
import torch

import gradient_reference as gr
import network_tangent_reference as nt
from conftest import rel_l2
from oracle.swinv2 import window_token_index

CFG = nt.net()[0]
STREAM = nt.stream_taps(CFG.depth)
CHAIN = ["emb", "lat", "mod"]


def _names(direction):
    """What is scored: in the time direction tok0's tangent is identically zero (checked exactly, not scored)."""
    return ["out"] + (STREAM[1:] if direction == "time" else STREAM)


def test_field_slicings_partition_their_tensors_into_the_units_they_name():
    t = nt.run("time").tangent
    want = {"out": {"sample,channel": 207, "sample,window": 12, "sample,shifted": 12}, "mod": {"sample,slot,half": 24},
            "lat": {"sample": 3}, "emb": {"sample": 3}}
    want.update({n: {"sample,window": 12, "sample,headblk": 36, "tile256x352": 36} for n in STREAM})
    for n, counts in want.items():
        sl = gr.slicings(gr.FIELD + n, t[n].shape, CFG)
        assert {k: int(l.max()) + 1 for k, l in sl.items()} == counts, n
        for lab in sl.values():
            sizes = torch.bincount(lab.expand(t[n].shape).reshape(-1))
            assert int(sizes.min()) > 0 and int(sizes.sum()) == t[n].numel() and int(sizes.min()) == int(sizes.max())
    # the windows are the oracle's: layer 1 (shifted) wrote xmid1 / x1, layer 0 and the patch embedding are unshifted
    for n, shift in (("tok0", (0, 0)), ("x0", (0, 0)), ("xmid1", CFG.shift_size), ("x1", CFG.shift_size)):
        lab = gr.slicings(gr.FIELD + n, t[n].shape, CFG)["sample,window"]
        idx = window_token_index(CFG.grid, CFG.window_size, shift)
        for w in range(idx.shape[0]):
            assert bool((lab[1, idx[w], 0] == 4 + w).all()), (n, w)
    # ... and in pixels: token (y, x) covers pixels (2 y .. 2 y + 1, 2 x .. 2 x + 1)
    sl = gr.slicings(gr.FIELD + "out", t["out"].shape, CFG)
    for name, shift in (("sample,window", (0, 0)), ("sample,shifted", CFG.shift_size)):
        idx = window_token_index(CFG.grid, CFG.window_size, shift)
        for w in range(idx.shape[0]):
            y, x = idx[w] // 32, idx[w] % 32
            assert bool((sl[name][2, 0, 2 * y + 1, 2 * x] == 8 + w).all()) and bool((sl[name][0, 0, 2 * y, 2 * x + 1] == w).all())
    lab = gr.slicings(gr.FIELD + "x0", t["x0"].shape, CFG)
    assert int(lab["sample,headblk"][2, 0, 88 * 5 - 1]) == 24 + 4 and int(lab["tile256x352"][1, 255, 352]) == 4 * 3 + 1
    assert int(lab["tile256x352"][1, 256, 351]) == 5 * 3


@pytest.mark.parametrize("dim,heads", [(None, None), (768, 12)])
def test_fp32_oracle_is_the_truth_and_every_bound_is_tight(dim, heads):
    """fp32 against fp64: within 1e-5 on every slice.  The emulations: no slice under the floor, each within 2 x the other,
    2 x the larger under 3e-2.  Prints the table DESIGN quotes.  (768, 12): the net of the padded-lane form, 12 heads of 64."""
    CFG = nt.net(dim, heads)[0]
    for direction in ("both", "time"):
        ref = nt.truth_and_yardsticks(direction, dim, heads)
        f32 = nt.run(direction, "f32", dim, heads)
        names = _names(direction)
        print(f"direction {direction}: " + ", ".join(f"|d{n}| = {float(ref[0].tangent[n].norm()):.4g}" for n in ["out"] + STREAM))
        ra, bad = nt.score_bf16(f"{direction}: emulation a", ref[1].tangent, ref, CFG, names)
        assert not bad, bad
        rb, bad = nt.score_bf16(f"{direction}: emulation b", ref[2].tangent, ref, CFG, names, show=False)
        assert not bad, bad
        for x, y in zip(ra, rb):
            assert x["under"] == 0 and x["worst"] <= 2 * y["worst"] and y["worst"] <= 2 * x["worst"], (x["name"], x["slicing"])
        _, bad = nt.score_fp32(f"{direction}: fp32 oracle against fp64", f32.tangent, ref[0].tangent, CFG, names + CHAIN, nt.FP32_CHAIN)
        assert not bad, bad
        # the emulations leave the latent chain in fp32: their dmod IS the fp32 oracle's
        _, bad = nt.score_fp32(f"{direction}: emulation a's chain", ref[1].tangent, ref[0].tangent, CFG, CHAIN, nt.FP32_CHAIN, show=False)
        assert not bad, bad
        # smallest slice of every slicing against the median (the floor is 0.1)
        for n in names:
            for sl, lab in gr.slicings(gr.FIELD + n, ref[0].tangent[n].shape, CFG).items():
                _, tn = gr.slice_errors(ref[0].tangent[n], ref[0].tangent[n], lab)
                print(f"  {direction} {n:6s} [{sl:15s}] smallest slice {float(tn.min() / tn.median()):.2f} of the median")
                assert float(tn.min()) >= gr.FLOOR * float(tn.median())
    if dim is not None:
        return
    # the primal output (scored for the engine's save_ctx form)
    ref = nt.truth_and_yardsticks("both")
    _, bad = nt.score_bf16("primal F: emulation a", ref[1].primal, ref, CFG, ["out"], kind="primal")
    assert not bad, bad


def test_tangent_is_linear_and_zero_where_the_direction_is():
    both, time, space, silent = (nt.run(d).tangent for d in ("both", "time", "space", "silent"))
    for n in both:
        err = rel_l2(space[n] + time[n], both[n])
        assert err < 1e-10, (n, err)
    assert all(float(time[n].abs().max()) > 0 for n in time if n != "tok0")
    for prec in ("f64", "f32", "a", "b"):
        assert not bool(nt.run("time", prec).tangent["tok0"].any()), prec    # the patch embedding does not see t
    for n, v in silent.items():
        assert not bool(v[1].any()), n                                       # a sample without a tangent: exactly zero everywhere
        assert rel_l2(v[0], both[n][0]) < 1e-12 and rel_l2(v[2], both[n][2]) < 1e-12, n   # ... and no trace of it in the others
    for n in CHAIN:
        assert not bool(space[n].any()), n


def test_dropped_dshift_passes_the_whole_output_bar_and_fails_the_slices():
    """The second norm of layer 0 (slot 1) loses its ``dshift``: the fp64 tangent with that one term missing."""
    slot = 1
    ref_b, ref_t = nt.truth_and_yardsticks("both"), nt.truth_and_yardsticks("time")
    cfg, _, state = nt.net()
    planted = nt.oracle_tangent(cfg, state, nt.case(nt.SEED, "both"), drop_dshift=(slot, ref_b[0].primal["lat"])).tangent
    assert nt.osw.modulated_norm.__name__ == "modulated_norm"               # (the oracle is as it was)
    assert rel_l2(planted["xmid0"], ref_b[0].tangent["xmid0"]) < 1e-12       # nothing upstream of the norm moves
    lost = {n: ref_b[0].tangent[n] - planted[n] for n in planted}            # depends on vt alone: the same in both directions
    whole = rel_l2(planted["out"], ref_b[0].tangent["out"])
    print(f"dshift of slot {slot} dropped, direction both: whole-output rel-L2 {whole:.3e} (the older bar: 8e-2)")
    assert 0 < whole < 8e-2
    planted_t = {n: ref_t[0].tangent[n] - lost[n] for n in lost}
    names = ["out", "x0", "xmid1", "x1"]
    recs, bad = nt.score_bf16("dshift dropped, direction time", planted_t, ref_t, CFG, names)
    print("\n".join(bad))
    hit = {b.split(" ")[0] for b in bad}
    assert hit == {gr.FIELD + n for n in names}, hit
    worst = max(recs, key=lambda r: r["worst"] / r["bound"])
    print(f"direction time: worst slice {worst['worst']:.3e} against its bound {worst['bound']:.3e} ({worst['name']} [{worst['slicing']}])")
    # in the combined direction the loss is a fraction of a percent of every slice
    recs, bad_b = nt.score_bf16("dshift dropped, direction both", planted, ref_b, CFG, names, show=False)
    print(f"direction both: {len(bad_b)} of {len(recs)} slicings over their bound; worst ratio "
          f"{max(r['worst'] / r['bound'] for r in recs):.2f}")
    # the dmod-level check names the slot
    dmod = ref_b[0].tangent["mod"].clone()
    dmod[:, slot, 1] = 0
    _, bad = nt.score_fp32("dmod with slot 1's shift zeroed", dict(mod=dmod), ref_b[0].tangent, CFG, ["mod"], nt.FP32_CHAIN)
    assert len(bad) == 1 and "slot 1, shift" in bad[0], bad
