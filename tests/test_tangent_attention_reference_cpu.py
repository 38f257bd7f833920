"""CPU proof of tests/tangent_attention_reference.py: the restatements are the formula (fp64 through the same lines equals
torch.func.jvp), the tangent is linear in its three operands, the conditions the GPU bounds rest on hold for every case and variant,
the case table takes both block orders of the bf16 kernel, and three faults planted in ONE item of the 96-item problem of
test_gpu_train.py::test_window_attention_jvp_kernel pass that test's global bounds while the per-item rule catches each."""
import pytest
import torch

import exact_attention as X
import tangent_attention_reference as ta

IDS = [c.name for c in ta.CASES]


def test_case_table():
    assert [(c.B, c.grid, c.heads, c.hd, c.shift, c.items) for c in ta.CASES] == [
        (1, (16, 32), 3, 80, (3, 5), 6), (2, (32, 16), 4, 88, (8, 8), 16), (1, (16, 16), 8, 96, (0, 0), 8)]
    # attn_jvp_bf16_kernel remaps (item, query half) when its grid of 2 x items workgroups is a multiple of 16
    assert [(2 * c.items) % 16 == 0 for c in ta.CASES] == [False, True, True]
    assert {float(t) for c in ta.CASES for t in ta.taus(c)} == set(ta.TAUS)


@pytest.mark.parametrize("c", ta.CASES, ids=IDS)
def test_operands_are_what_the_builder_says(c):
    for f32 in (False, True):
        qkv, dqkv = ta.operands(c, f32)
        q, k, v, dq, dk, dv = ta.parts(c, qkv, dqkv)
        tol = 1e-6 if f32 else 2.0 ** -8
        assert float((q.norm(dim=-1) / ta.taus(c).view(1, 1, -1, 1).double() - 1).abs().max()) < tol
        assert float((k.norm(dim=-1) - 1).abs().max()) < tol
        assert abs(float(v.std()) - 1) < 0.02 and all(abs(float(t.std()) - 0.3) < 0.01 for t in (dq, dk, dv))
        assert torch.equal(qkv, ta.store(qkv, f32)) and torch.equal(dqkv, ta.store(dqkv, f32))
        for only in ("dq", "dk", "dv"):
            q1, d1 = ta.operands(c, f32, only)
            t1 = dict(zip(("dq", "dk", "dv"), X.thirds(c, d1)))
            assert torch.equal(q1, qkv) and torch.equal(t1[only].double(), {"dq": dq, "dk": dk, "dv": dv}[only])
            assert all(float(t.abs().max()) == 0 for n, t in t1.items() if n != only)


@pytest.mark.parametrize("c", ta.CASES, ids=IDS)
def test_restatements_are_the_formula_and_the_tangent_is_linear(c):
    qkv, dqkv = ta.operands(c, False)
    out, dout = ta.truth(c, qkv, dqkv)
    p64 = ta.parts(c, qkv, dqkv)
    same = lambda t: t
    forms = [ta.restate_bf16(*p64, rnd=same), ta.restate_autocast(*p64, rnd=same), ta.restate_fp32(*p64)]
    for o, d in forms:
        assert float(ta.item_rel_l2(o, out).max()) < 1e-12 and float(ta.item_rel_l2(d, dout).max()) < 1e-11
    total = sum(ta.truth(c, *ta.operands(c, False, only))[1] for only in ("dq", "dk", "dv"))
    assert float(ta.item_rel_l2(total, dout).max()) < 1e-12
    # the share of each term in an item's tangent: dv (and dq) fall to 1 % on the tau = 100 heads, where a fault in that term alone
    # would hide under the other two -- why every GPU case also runs with one tangent at a time
    for only in ("dq", "dk", "dv"):
        share = ta.truth(c, *ta.operands(c, False, only))[1].flatten(3).norm(dim=-1) / dout.flatten(3).norm(dim=-1)
        print(f"{c.name}: share of the {only} term in an item's tangent {float(share.min()):.2e} .. {float(share.max()):.2e}")
        assert float(share.min()) > 0


@pytest.mark.parametrize("only", ta.VARIANTS)
@pytest.mark.parametrize("c", ta.CASES, ids=IDS)
def test_conditions_of_the_gpu_bounds(c, only):
    """Every bf16 tangent yardstick <= 1.5e-2 and every fp32 one <= 5e-6, so that 2 x the yardstick (resp. F32_TOL) separates a
    right item from a wrong one; the primal yardsticks are printed beside them."""
    b, f = ta.reference(c, False, only), ta.reference(c, True, only)
    fmt = lambda t: "[" + ", ".join(f"{float(x):.2e}" for x in t) + "]"
    print(f"{c.name} {only}: per head (tau {[float(t) for t in ta.taus(c)]}) bf16 yardstick primal {fmt(b['yard_out'])} tangent "
          f"{fmt(b['yard_dout'])}; fp32 yardstick primal {fmt(f['yard_out'])} tangent {fmt(f['yard_dout'])}")
    assert float(b["yard_dout"].max()) <= ta.BF16_YARD_CAP and float(b["yard_dout"].min()) > 1e-4
    assert float(f["yard_dout"].max()) <= ta.F32_YARD_CAP
    assert float(b["yard_out"].max()) <= ta.BF16_YARD_CAP and float(f["yard_out"].max()) <= ta.F32_YARD_CAP
    assert ta.FACTOR * float(f["yard_dout"].max()) <= ta.F32_TOL      # F32_TOL is no tighter than the bf16 rule's margin


FAULTS = [("the correction term dropped on a tau = 1 head", dict(drop_correction=True), 4, None),
          ("dK taken from the other key half, one query half", dict(swap_dk_halves=True), 1, slice(128, 256)),
          ("dv ignored in one item", dict(ignore_dv=True), 7, None)]


@pytest.fixture(scope="module")
def problem96():
    c = ta.THE_96
    qkv, dqkv = ta.operands_96()
    out, dout = ta.truth(c, qkv, dqkv)
    p32 = ta.parts(c, qkv, dqkv, torch.float32)
    a = ta.restate_bf16(*p32)
    b = ta.restate_autocast(*p32)
    yard = [torch.maximum(ta.per_head_worst(ta.item_rel_l2(a[i], r)), ta.per_head_worst(ta.item_rel_l2(b[i], r))) for i, r in enumerate((out, dout))]
    return c, p32, out, dout, a, yard


def _global(got, ref):
    return float((got.double() - ref).norm() / ref.norm())


def test_yardstick_a_passes_both_rules_on_the_96_item_problem(problem96):
    c, p32, out, dout, a, yard = problem96
    assert c.items == 96
    assert _global(a[0], out) < 1e-2 and _global(a[1], dout) < 2e-2
    for got, ref, y in zip(a, (out, dout), yard):
        assert float((ta.item_rel_l2(got, ref) / y).max()) <= 1.0


@pytest.mark.parametrize("what,fault,head,rows", FAULTS, ids=[f[0] for f in FAULTS])
def test_a_fault_in_one_item_passes_the_global_bound_and_fails_the_per_item_rule(problem96, what, fault, head, rows):
    c, p32, out, dout, a, yard = problem96
    assert float(ta.SCALE_96[4]) == 1.0
    item = (1, 2, head)                                               # (sample, window, head)
    one = tuple(t[item][None] for t in p32)
    bad_o, bad_d = ta.restate_bf16(*one, **fault)
    got_o, got_d = a[0].clone(), a[1].clone()
    sl = rows if rows is not None else slice(0, 256)
    got_o[item][sl], got_d[item][sl] = bad_o[0][sl], bad_d[0][sl]
    assert torch.equal(got_o, a[0])                                   # the faults touch the tangent only
    g_o, g_d = _global(got_o, out), _global(got_d, dout)
    err = ta.item_rel_l2(got_d, dout)
    ratio = err / yard[1]
    print(f"{what}: global rel-L2 primal {g_o:.2e} (< 1e-2), tangent {g_d:.2e} (< 2e-2): passes; the item's own error {float(err[item]):.2e} = "
          f"{float(ratio[item]):.1f} x its head's yardstick {float(yard[1][head]):.2e} (rule: <= {ta.FACTOR})")
    assert g_o < 1e-2 and g_d < 2e-2
    assert float(ratio[item]) > ta.FACTOR
    ratio[item] = 0
    assert float(ratio.max()) <= 1.0                                  # and no other item is touched
