"""CPU: tests/epilogue_reference.py itself.  Its closed forms against autograd / torch.func.jvp of the oracle's own expressions
(oracle/swinv2.py: F.silu(gate) * up; q / q.norm().clamp_min(1e-12) * clamp(scale, max=ln 100).exp(), k likewise without tau) in fp64,
the preconditions every bound of tests/test_gpu_gemm_epilogues.py rests on, the case table against the dispatch cells it must reach,
and the fp32 restatement of every epilogue -- rounded where the kernel rounds -- against every bound on every case: the restatement
stays within the caps on its own, so a kernel that misses one is further from fp64 than plain fp32 arithmetic has to be."""
import math

import pytest
import torch
import torch.nn.functional as F

import backward_reference as br
import epilogue_reference as E

F64 = torch.float64


def _oracle_prenorm(raw, scale, heads, hd):
    """cosine_window_attention's prologue (oracle/swinv2.py) on raw [M, heads * 3 * hd], columns head-major then q | k | v."""
    M = raw.shape[0]
    x = raw.view(M, heads, 3 * hd)
    q, k, v = x[..., :hd], x[..., hd:2 * hd], x[..., 2 * hd:]
    tau = torch.clamp(scale, max=math.log(1.0 / 0.01)).exp().view(1, heads, 1)
    q = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12) * tau
    k = k / k.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return torch.cat([q, k, v], -1).reshape(M, -1)


@pytest.mark.parametrize("hd", [80, 88, 96])
def test_qknorm_tangent_vs_jvp_of_the_oracle(hd):
    heads, M = 4, 9
    raw, draw = br.rnd((M, 3 * heads * hd), hd).double(), br.rnd((M, 3 * heads * hd), hd + 1).double()
    raw[3] = 0.0   # the clamp decides: v-hat = 0, d v-hat = tau dv / 1e-12
    scale = torch.tensor([math.log(10.0), E.AT_LN100, math.log(200.0), math.log(3.0)], dtype=F64)
    want, dwant = torch.func.jvp(lambda r: _oracle_prenorm(r, scale, heads, hd), (raw,), (draw,))
    got, dgot, rn, sc = E.qknorm_jvp(raw, draw, scale, heads, hd)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    live = torch.ones(M, dtype=torch.bool)
    live[3] = False   # (autograd differentiates norm() at 0 as 0 / 0; the closed form's clamp branch is checked by hand below)
    assert float((dgot[live] - dwant[live]).abs().max()) <= 1e-12 * float(dwant[live].abs().max())
    v3 = dgot[3].view(heads, 3, hd)
    tau = scale.clamp(max=br.LN100).exp()
    d3 = draw[3].view(heads, 3, hd)
    assert torch.allclose(v3[:, 0], tau[:, None] * d3[:, 0] / 1e-12, rtol=1e-12) and torch.allclose(v3[:, 1], d3[:, 1] / 1e-12, rtol=1e-12)
    assert torch.equal(v3[:, 2], d3[:, 2])
    fwd, rn2 = E.qknorm_fwd(raw, scale, heads, hd)
    assert torch.equal(fwd, got) or float((fwd - got).abs().max()) <= 1e-12 * float(got.abs().max())
    assert float((rn - rn2).abs().max() / rn2.abs().max()) <= 1e-12
    assert bool((sc >= dgot.abs() * (1 - 1e-12)).all())   # the scale bounds the element


def test_swiglu_tangent_vs_jvp_of_the_oracle():
    h, dh = br.swiglu_inputs(7, 33, 5)
    h, dh2 = h.double(), br.rnd((7, 66), 6).double()
    f = lambda x: F.silu(x[:, 0::2]) * x[:, 1::2]
    want, dwant = torch.func.jvp(f, (h,), (dh2,))
    got, dgot, sc = E.swiglu_jvp(h, dh2)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert float((dgot - dwant).abs().max()) <= 1e-12 * float(dwant.abs().max())
    assert bool((sc >= dgot.abs() * (1 - 1e-12)).all())
    assert float((got - br.swiglu_fwd(h)).abs().max()) <= 1e-12 * float(want.abs().max())


def test_split3_reading():
    buf = torch.arange(2 * 40).view(2, 40)
    b0, b1, b2 = E.split3_read(buf, 5, 12)
    assert b0[1].tolist() == [40, 41, 42, 43, 44] and b1[0].tolist() == [12, 13, 14, 15, 16] and b2[0].tolist() == [24, 25, 26, 27, 28]


def test_table_meets_every_required_cell():
    cells = [E.expected_cell(c)._asdict() for c in E.CASES]
    for c, cell in zip(E.CASES, cells):
        assert cell["rc"] == c.rc, (c.name, cell)   # the table says which rows the header's rules refuse
    for req in E.REQUIRED:
        assert any(all(cell[k] == v for k, v in req.items()) for cell in cells), req
    assert sum(c.key31 for c in E.CASES) == 1
    key31, = [c for c in E.CASES if c.key31]
    cell = E.expected_cell(key31)
    assert (cell.epi, cell.width, cell.kloop, cell.kernel) == ("swiglu", 352, "pp", "persistent") and key31.M > 256   # an interior tile
    for c in E.CASES:   # the size limit: about 23,040 x 1,152 outputs
        assert c.rows_a * c.N <= 23040 * 1152


def test_head_classes_occur():
    every = {"below", "at", "above"}
    for c in E.cases("qknorm", "qknorm_jvp"):
        if c.heads >= 3:
            assert E.head_classes(c) == every, c.name
    for form in ("single", "qk_only"):
        seen = set().union(*(E.head_classes(c) for c in E.cases("qknorm") if c.form == form))
        assert seen == every, form


@pytest.fixture(scope="module", params=E.CASES, ids=[f"{c.epi}-{c.name}" for c in E.CASES])
def case(request):
    c = request.param
    return c, E.inputs(c)


def test_preconditions(case):
    c, inp = case
    a, acc = inp["A"], inp["acc"]
    # scaled-integer partial sums: every |a| is an integer times 1/8, |w| <= 1
    q = a[:, :c.K].double() * 8
    assert torch.equal(q, q.round()) and float(q.abs().sum(1).max()) < 2 ** 24
    assert bool(torch.isnan(a[:, c.K:]).all()) and bool(torch.isnan(inp["W"][:, c.K:]).all())
    # the planted rows are where the docstring says
    assert not bool(a[E.ZERO_ROW, :c.K].any()) and not bool(acc[E.ZERO_ROW].any())
    assert c.sat_row != E.ZERO_ROW and 0 <= c.sat_row < c.M
    ordinary = torch.ones(acc.shape[0], dtype=torch.bool)
    ordinary[c.sat_row] = False
    assert float(acc[ordinary].abs().max()) < 32.0
    if c.epi not in ("qknorm", "qknorm_jvp", "bwd"):
        gates = acc[c.sat_row, 0::2]
        assert gates[:4].tolist() == [96.0, -96.0, -96.0, 96.0] and float(gates.max()) <= 128.0 and float(gates.min()) >= -128.0   # saturated on both sides
        assert torch.isinf(torch.exp(torch.tensor(96.0)))
    if c.epi == "bwd":
        assert inp["H"][c.M - 1, 0:12:2].tolist() == torch.tensor(br.PLANTED_GATES).bfloat16().float().tolist()
    # what the GPU test compares by bits is representable in the stored type
    if c.out == "bf16":
        assert torch.equal(acc.float().bfloat16().double(), acc)
    assert torch.equal(acc.float().double(), acc)
    if c.epi == "qknorm_jvp":
        _, dref, _, sc = E.qknorm_jvp(acc[:c.M], acc[c.M:], inp["scale"], c.heads, c.hd)
        num, den = E.qk_view(c, sc).norm(dim=-1), E.qk_view(c, dref).norm(dim=-1)
        assert bool((den > 0).all()) and float((num / den).max()) < 16.0   # far below 2^8: a relative bound on the result is fair
    if c.epi == "swiglu_jvp":
        assert bool(acc[c.M:].abs().sum(1).min() > 0)   # no tangent row is empty


def test_restatement_meets_every_bound(case):
    c, inp = case
    rep = E.score(c, inp, E.restate(c, inp))
    print(rep.text())
    assert not rep.failed, "\n".join(rep.failed)
    if c.rc == 0:   # and the score is no rubber stamp: one wrong element, one touched pad word
        b = E.restate(c, inp)
        main = "C2" if c.epi == "swiglu_jvp" else "C"
        b[main][c.M - 1, 3] ^= 0x4000 if b[main].dtype == torch.int16 else 0x40000000
        assert E.score(c, inp, b).failed
        b = E.restate(c, inp)
        b[main][-1, -1] = 0
        assert E.score(c, inp, b).failed
