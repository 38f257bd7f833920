"""CPU proof of tests/exact_attention.py: on the ORACLE alone every row of the case table has the single answer the GPU tests of
test_gpu_attention_exact.py demand -- zero mismatching elements under oracle.swinv2.cosine_window_attention in its three modes (fp32
naive, emulate_bf16=True, emulate_bf16="offset0") -- the code sets respect the cos cap, the table reaches every branch of the
persistent kernels' item walk, and the plain bf16 restatement of the backward agrees with fp64 autograd."""
import math

import pytest
import torch
import torch.nn.functional as F

import exact_attention as X
from oracle.swinv2 import bf16_round, cosine_window_attention

IDS = [c.name for c in X.CASES]


def oracle_windows(c, qkv_tokens, scale, **mode):
    """token-order raw qkv [B, n, 3 dim] -> the oracle's attention per window, returned in window order [B, nW, H, 256, hd]."""
    idx = X.window_index(c).reshape(-1)
    ow = cosine_window_attention(qkv_tokens[:, idx].reshape(c.B * c.nW, 256, -1), scale.view(1, c.heads, 1, 1), c.heads, **mode)
    return ow.reshape(c.B, c.nW, 256, c.heads, c.hd).permute(0, 1, 3, 2, 4)


MODES = (dict(naive=True), dict(emulate_bf16=True), dict(emulate_bf16="offset0"))


@pytest.mark.parametrize("c", X.CASES, ids=IDS)
def test_selector_has_one_answer_on_the_oracle(c):
    s = X.selector(c)
    assert X.max_offdiag_cos(s["code"]) <= X.COS_CAP
    assert all(t >= 30 for t in c.taus()) and all(t >= 49 for t in c.taus(True))
    assert torch.equal(s["v"], bf16_round(s["v"])) and float(s["v"].abs().min()) >= 0.5
    # every item has its own permutation, and none is the identity
    assert len({tuple(p.tolist()) for p in s["pi"].reshape(-1, 256)[:64]}) == min(64, c.items)
    qkv = X.raw_qkv(c, "selector")
    assert torch.equal(qkv, bf16_round(qkv))                      # the raw operands are bf16 values: one tensor serves both types
    for mode in MODES:
        got = bf16_round(oracle_windows(c, qkv, c.scale(), **mode))
        assert int((got != s["out"]).sum()) == 0, mode
    got = oracle_windows(c, qkv, c.scale(True), naive=True)       # fp32 at tau >= 49: exact without any rounding
    assert int((got != s["out"]).sum()) == 0
    for bits in (16, 24):                                         # wider v for the fp32 kernels: still the gather, every bit
        v, out = X.selector_v(c, bits)
        assert int((v != bf16_round(v)).sum()) > v.numel() // 2
        hi = bf16_round(v)
        assert torch.equal(hi + bf16_round(v - hi), v) == (bits == 16)   # 16 bits: exactly what a (hi, lo) pair of bf16 holds
        got = oracle_windows(c, X.raw_qkv(c, "selector", bits), c.scale(True), naive=True)
        assert int((got != out).sum()) == 0
    # the token-order expectation is the scatter of the window-order one through the oracle's map
    back = X.expected_out(c, "selector").reshape(c.B, c.n, c.heads, c.hd)[:, X.window_index(c).reshape(-1)]
    assert torch.equal(back.reshape(c.B, c.nW, 256, c.heads, c.hd).permute(0, 1, 3, 2, 4), s["out"])


def test_selector_is_not_exact_at_a_low_scale():
    """The one-hot property is a property of the scale: at tau = 12 the wrong keys keep enough weight to move most bf16 results (with
    this module's v, bounded away from zero, mismatches start below tau = 16; the table's floor of 30 keeps a wide margin)."""
    c = X.BY_NAME["below8"]
    s = X.selector(c)
    got = bf16_round(oracle_windows(c, X.raw_qkv(c, "selector"), torch.full((c.heads,), math.log(12.0)), emulate_bf16=True))
    assert int((got != s["out"]).sum()) > 1000


@pytest.mark.parametrize("c", X.CASES, ids=IDS)
def test_uniform_has_one_answer_on_the_oracle(c):
    u = X.uniform(c)
    assert bool((u["k"] == u["k"][..., :1, :]).all()) and set(u["v"].unique().tolist()) == {-1.0, 0.0, 1.0}
    assert torch.equal(u["out"], bf16_round(u["out"]))
    qkv = X.raw_qkv(c, "uniform")
    for sc in (c.scale(), c.scale(True)):
        for mode in MODES:
            got = oracle_windows(c, qkv, sc, **mode)
            assert int((bf16_round(got) != u["out"]).sum()) == 0, mode
    # bf16-rounded operands (what the bf16 entries see) change nothing
    got = oracle_windows(c, bf16_round(qkv), c.scale(), emulate_bf16="offset0")
    assert int((bf16_round(got) != u["out"]).sum()) == 0


@pytest.mark.parametrize("c", [c for c in X.CASES if X.expected_rc(c, "fused") == 0], ids=lambda c: c.name)
@pytest.mark.parametrize("fam", ["selector", "uniform"])
def test_fused_operands_have_one_answer_on_the_oracle(c, fam):
    f = X.fused_operands(c, fam)
    x, w, K = f["x"], f["w"], f["K"]
    assert torch.equal(x, bf16_round(x)) and torch.equal(w, bf16_round(w))
    assert bool((x[:, :K].abs() == 1).all()) and bool((x[:, K:] == 3.0).all()) and bool((w[:, K:] == 0).all())
    if fam == "selector":
        assert X.max_offdiag_cos(f["base"]) <= X.COS_CAP
    qkv = F.linear(x[:, :K].double(), w[:, :K].double())          # exact: integers (halves of integers for the uniform v)
    assert torch.equal(qkv.float().double(), qkv)
    qkv = qkv.float().view(c.B, c.n, 3 * c.dim)
    for mode in MODES:
        got = bf16_round(oracle_windows(c, qkv, c.scale(), **mode))
        assert int((got != f["out"]).sum()) == 0, mode


@pytest.mark.parametrize("c", [c for c in X.CASES if X.expected_rc(c, "bwd") == 0], ids=lambda c: c.name)
def test_selector_backward_scatter_and_bounds_hold_in_fp64(c):
    """fp64 autograd of the attention core on the prenormalised bf16 operands: dv is the scatter of dO to within the wrong keys'
    weight (so its bf16 rounding IS the scatter), dq and dk are far inside the cancellation bounds, the tangent of v passes through
    the gather."""
    s, b = X.selector(c), X.selector_backward(c)
    q, k, v = (t.bfloat16().double().requires_grad_(True) for t in X.prenorm_parts(c, "selector"))
    p = (q @ k.transpose(-2, -1)).softmax(-1)
    o = p @ v
    assert torch.equal(o.float().bfloat16().float(), s["out"])
    o.backward(b["do"].double())
    assert torch.equal(v.grad.float().bfloat16().float(), b["dv"])
    assert bool((q.grad.abs() <= b["dq_bound"]).all()) and bool((k.grad.abs() <= b["dk_bound"]).all())
    assert float(b["dq_bound"].max()) < 1e-2 and float(b["dk_bound"].max()) < 1.0   # against |dO| ~ 1: the bounds say "nothing"
    dout = (p.detach() @ b["tv"].double()).float().bfloat16().float()
    assert torch.equal(dout, b["dout"])


@pytest.mark.parametrize("c", [c for c in X.CASES if X.expected_rc(c, "bwd") == 0], ids=lambda c: c.name)
def test_uniform_backward_is_the_column_mean(c):
    u, b = X.uniform(c), X.uniform_backward(c)
    q, k, v = (t.bfloat16().float() for t in X.prenorm_parts(c, "uniform"))
    _, _, dv = X.backward_bf16(q, k, v, u["out"], b["do"])
    assert torch.equal(dv.bfloat16().float(), b["dv"]) and torch.equal(b["dv"], bf16_round(b["dv"]))


@pytest.mark.parametrize("c", X.CASES, ids=IDS)
def test_flat_tangent_has_one_answer(c):
    """The flat family of the tangent entry: constant logit rows, W a bf16 value, every accumulation's sum of absolute terms below
    2^24 units of its last place (so any order is exact, and so is the kernels' fp32 closing sequence), the closed form equal to
    torch.func.jvp in fp64, every query row of an item with its own expected tangent row, and every one of dq, dk, dv visible in
    every item."""
    f, e = X.flat(c), X.flat_expected(c)
    q, k, v, dq, dk, dv = (f[n] for n in ("q", "k", "v", "dq", "dk", "dv"))
    for t in (q, k, v, dq, dk, dv):
        assert torch.equal(t, bf16_round(t)) and float(t.abs().max()) > 0
    assert bool(((q != 0).sum(-1) == 1).all()) and set(q.abs().amax(-1).unique().tolist()) == {1.0, 2.0, 4.0}      # rows s_i e_{a_i}
    assert bool((k.gather(-1, X.flat(c)["A"].unsqueeze(-2).expand(*k.shape[:-1], X.FLAT_A)) == 1).all())
    assert bool((dq.abs().sum(-1) == 4).all()) and bool((dk.abs().sum(-1) == 4).all())
    # W = 1 x dS is an integer with |dS| <= 4 + 4 (four +-1 of dq against |k| <= 1, s_i <= 4 against one +-1 of dk): every integer up
    # to 256 is a bf16 value, so bounding the maximum bounds them all
    assert e["ds_max"] <= 8
    assert e["budget"] < 2 ** 24
    print(f"{c.name}: max |dS| {e['ds_max']:.0f}, largest sum of absolute terms {e['budget']:.3g} (2^24 = {2 ** 24})")
    out, dout = e["out"], e["dout"]
    assert float(out.abs().max()) * 256 <= 256                                                  # colsum(v) / 256 is a bf16 value
    assert torch.equal(out.float().double(), out) and torch.equal(bf16_round(out.float()).double(), out)
    assert torch.equal(dout.float().double(), dout)                                             # an fp32 value
    # the kernels' closing sequence in fp32 on the exact sums reproduces it
    for b in range(c.B):
        qd, kd, vd, dqd, dkd, dvd = (f[n][b].double() for n in ("q", "k", "v", "dq", "dk", "dv"))
        logits = qd @ kd.transpose(-2, -1)
        assert torch.equal(logits, qd.sum(-1, keepdim=True).expand_as(logits))                  # every logit of row i is s_i
        ds = dqd @ kd.transpose(-2, -1) + qd @ dkd.transpose(-2, -1)
        u, tt, o = (ds @ vd).float(), dvd.sum(-2, keepdim=True).float(), vd.sum(-2, keepdim=True).float()
        rl = torch.tensor(1.0 / 256.0)
        rr = ds.sum(-1, keepdim=True).float() * rl
        assert torch.equal(((u + tt - rr * o) * rl).double(), dout[b])
        # fp64 forward-mode differentiation of softmax(q k^T) v
        fn = lambda q_, k_, v_: (q_ @ k_.transpose(-2, -1)).softmax(-1) @ v_
        ro, rd = torch.func.jvp(fn, (qd, kd, vd), (dqd, dkd, dvd))
        assert float((ro - out[b]).abs().max()) < 1e-13 and float((rd - dout[b]).abs().max()) < 1e-12
    # a misrouted row shows: the 256 expected tangent rows of an item are all different, also after the bf16 rounding
    rows = bf16_round(dout.float()).reshape(-1, 256, c.hd)
    assert all(len(r.unique(dim=0)) == 256 for r in rows)
    # each product is pinned: without dq, dk or dv the expected tangent changes in every item
    for name in ("dq", "dk", "dv"):
        other = bf16_round(X.flat_expected(c, zero=(name,))["dout"].float()).reshape(-1, 256, c.hd)
        assert bool((other != rows).flatten(1).any(1).all()), name


def test_case_table_reaches_every_branch_and_entry():
    seen = set()
    for c in X.CASES:
        seen |= X.walk(c.items)
    assert seen >= set(X.REQUIRED_WALK)
    for c, want in (("below8", {"below8"}), ("items12", {"shrunk_grid", "ragged_eighths"}), ("items20", {"shrunk_grid", "ragged_eighths"}),
                    ("items324", {"ragged_eighths", "several_rounds"}), ("items288", {"ragged_last_round", "several_rounds"}),
                    ("row528", {"ragged_last_round"}), ("items768", {"full_rounds", "several_rounds"})):
        assert want <= X.walk(X.BY_NAME[c].items), c
    # every entry runs on some row and (where the header has a rule to refuse by) is refused on some row
    for e in X.FWD_ENTRIES + X.BWD_ENTRIES:
        assert any(X.expected_rc(c, e) == 0 for c in X.CASES), e
    for e in ("tiled", "fused", "gemm_tiled", "bwd", "bwd_scaled", "bwd_qknorm", "jvp"):
        assert any(X.expected_rc(c, e) == X.ESHAPE for c in X.CASES), e
    assert {c.grid for c in X.CASES} >= {(16, 16), (16, 64), (64, 16), (32, 64), (32, 48)}
    assert {c.shift for c in X.CASES} >= {(0, 0), (8, 8), (0, 5), (5, 0), (15, 15), (1, 0)}
    assert {c.hd for c in X.CASES} == {64, 80, 88, 96} and max(c.B for c in X.CASES) <= 11
    # the fused entry sees K = dim with and without the half k-tile pad
    assert {c.dim % 64 for c in X.CASES if X.expected_rc(c, "fused") == 0} == {0, 32}


def test_backward_restatement_agrees_with_fp64_autograd():
    """X.backward_bf16 on random prenormalised inputs against fp64 autograd of softmax(q k^T) v, per third: the distance is the
    bf16 rounding of P and dS (a few 1e-3), and with the roundings switched off (fp64 operands through the same lines, bf16r made
    the identity) it is the formula itself, to 1e-12."""
    g = torch.Generator().manual_seed(5)
    hd, heads = 88, 6
    tau = torch.tensor([10.0, 3.0, 30.0, 60.0, 100.0, 48.0]).view(1, heads, 1, 1)
    q = F.normalize(torch.randn(2, heads, 256, hd, generator=g), dim=-1) * tau
    k = F.normalize(torch.randn(2, heads, 256, hd, generator=g), dim=-1)
    v, do = torch.randn(2, heads, 256, hd, generator=g), torch.randn(2, heads, 256, hd, generator=g)
    q, k, v, do = (bf16_round(t) for t in (q, k, v, do))
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    od = (qd @ kd.transpose(-2, -1)).softmax(-1) @ vd
    od.backward(do.double())
    got = X.backward_bf16(q, k, v, bf16_round(od.detach().float()), do)
    for name, a, b in zip("qkv", got, (qd.grad, kd.grad, vd.grad)):
        e = X.item_rel_l2(a[:, None], b[:, None])
        print(f"backward restatement d{name}: per-item rel-L2 {float(e.min()):.2e} .. {float(e.max()):.2e}")
        assert float(e.max()) < (2e-2 if name != "v" else 6e-3), name
    keep = X.bf16r
    X.bf16r = lambda t: t
    try:
        exact = X.backward_bf16(q.double(), k.double(), v.double(), od.detach(), do.double())
    finally:
        X.bf16r = keep
    for a, b in zip(exact, (qd.grad, kd.grad, vd.grad)):
        assert float(X.item_rel_l2(a[:, None], b[:, None]).max()) < 1e-12
