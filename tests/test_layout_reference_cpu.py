"""tests/layout_reference.py against the oracle and against its own claims (no GPU): the placement references equal
oracle.swinv2.patchify / unpatchify bit for bit on tagged inputs, the embedding and rollout references equal the oracle's in fp64,
every case of the GPU tables reaches the kernel it names, tagged and integer inputs stay exact, the conversion table is what torch's
own bf16 rounding gives, and the restated tile walk equals division of the tile number."""
import math

import pytest
import torch

import layout_reference as lr
from layout_reference import LINEAR_CASES, PATCHIFY_CASES, UNPATCHIFY_CASES, linear_operands, patchify_inputs

PATCHES = [(1, 1), (2, 2), (7, 7), (3, 2), (2, 3)]


@pytest.mark.parametrize("patch", PATCHES)
def test_patchify_reference_equals_oracle_on_tagged_sources(patch):
    from oracle.swinv2 import patchify
    p1, p2 = patch
    B, H, W = 2, 2 * p1, 3 * p2
    chans, scales = (3, 2, 4), (0.5, 1.0, 2.0)
    srcs, off = [], 0
    for c in chans:
        srcs.append(lr.tagged((B, c, H, W), off))
        off += srcs[-1].numel()
    F = p1 * p2 * sum(chans)
    got = lr.patchify_ref(srcs, scales, patch, F + 3)
    want = patchify(torch.cat([s.double() * k for s, k in zip(srcs, scales)], 1), patch).reshape(-1, F)
    assert torch.equal(got[:, :F], want) and bool((got[:, F:] == 0).all())
    # sources 0 and 2 with source 1 absent, and the per-sample factor
    ps = torch.tensor([2.0, 0.25])
    got = lr.patchify_ref([srcs[0], None, srcs[2]], scales, patch, p1 * p2 * 7, per_sample=ps)
    want = patchify(torch.cat([srcs[0].double() * 0.5 * ps.double().view(B, 1, 1, 1), srcs[2].double() * 2.0], 1), patch)
    assert torch.equal(got, want.reshape(got.shape))
    # the single-element restatement names the same source element
    for row, col in ((0, 0), (got.shape[0] - 1, got.shape[1] - 1), (3, 5 % got.shape[1])):
        s, b, c, y, x = lr.patchify_source_of(row, col, (3, 0, 4), B, H, W, patch)
        src = (srcs[0], None, srcs[2])[s]
        assert float(got[row, col]) == float(src[b, c, y, x]) * (0.5 * float(ps[b]) if s == 0 else 2.0)


@pytest.mark.parametrize("patch", PATCHES)
def test_unpatchify_reference_equals_oracle_on_tagged_tokens(patch):
    from oracle.swinv2 import unpatchify
    p1, p2 = patch
    B, C, gh, gw = 2, 3, 2, 4
    H, W = gh * p1, gw * p2
    tok = lr.tagged((B, gh * gw, C * p1 * p2))
    got = lr.unpatchify_gather(tok, C, H, W, patch)
    assert torch.equal(got, unpatchify(tok, patch, (gh, gw)))
    wide = torch.full((B, gh * gw, C * p1 * p2 + 5), float("nan"))
    wide[..., :C * p1 * p2] = tok
    assert torch.equal(lr.unpatchify_gather(wide, C, H, W, patch), got)
    b, t, f = lr.unpatchify_source_of(1, 2, H - 1, W - 1, W, patch)
    assert float(tok[b, t, f]) == float(got[1, 2, H - 1, W - 1])
    xt, al, be = lr.normal((B, C, H, W), 3), torch.tensor([0.3, -1.0]), torch.tensor([2.0, 0.5])
    ref, bound = lr.unpatchify_ref(tok, C, H, W, patch, xt, al, be)
    want = al.double().view(B, 1, 1, 1) * xt.double() + be.double().view(B, 1, 1, 1) * unpatchify(tok, patch, (gh, gw)).double()
    assert torch.equal(ref, want) and bool((bound > 0).all())
    ref, bound = lr.unpatchify_ref(tok, C, H, W, patch)
    assert torch.equal(ref, got.double()) and bool((bound == 0).all())
    ref, _ = lr.unpatchify_ref(tok, C, H, W, patch, xt, None, be)  # alpha == NULL means 0
    assert torch.equal(ref, be.double().view(B, 1, 1, 1) * got.double())


@pytest.mark.parametrize("d", [2, 98, 1056])
@pytest.mark.parametrize("aux_dim", [0, 1, 3])
def test_embedding_reference_equals_oracle_for_even_d(d, aux_dim):
    from oracle.swinv2 import timestep_embedding
    B, w = 4, 1000.0
    t = torch.tensor([0.0, -0.37, 1.0, 1.5])
    freqs = lr.default_freqs(d)
    aux = lr.normal((B, aux_dim), 5) if aux_dim else None
    aw, ab = (lr.normal((d, aux_dim), 6, 0.02), lr.normal((d,), 7, 0.02)) if aux_dim else (None, None)
    ref, bound = lr.timestep_embed_ref(t, w, freqs, d, aux, aw, ab)
    # the oracle in fp64 on the SAME fp32 argument: t w rounded to fp32, then times the fp32 frequency
    half = d // 2
    arg = ((t * torch.tensor(w))[:, None] * freqs[None, :]).double()
    want = torch.cat([torch.sin(arg), torch.cos(arg)], -1)
    # (oracle.timestep_embedding builds its own fp64 frequencies; it agrees to the frequencies' fp32 rounding times the argument)
    tw = (t * torch.tensor(w)).double()
    assert float((timestep_embedding(tw, d) - want).abs().max()) <= 2.0 ** -23 * float(tw.abs().max()) + 1e-12
    if aux_dim:
        want = want + torch.nn.functional.linear(aux.double() * math.sqrt(float(aux_dim)), aw.double(), ab.double())
    tol = 1e-12 if aux_dim != 3 else 1e-7  # (sqrt(3) reaches the kernel as fp32: 2^-25 relative on the aux term)
    assert float((ref - want).abs().max()) <= tol
    assert bool((bound >= 2.0 ** -22).all())


def test_embedding_reference_for_odd_d_is_sin_cos_zero():
    d, t = 7, torch.tensor([0.5, 2.0])
    freqs = lr.default_freqs(d)
    ref, bound = lr.timestep_embed_ref(t, 1.0, freqs, d)
    arg = (t[:, None] * freqs[None, :]).double()
    assert torch.equal(ref[:, :3], torch.sin(arg)) and torch.equal(ref[:, 3:6], torch.cos(arg))
    assert bool((ref[:, 6] == 0).all()) and bool((bound[:, 6] == 0).all())


def test_rollout_reference_equals_oracle_update():
    from oracle.rollout import Stats
    B, C, H, W = 2, 5, 4, 8
    x, y = lr.normal((B, C, H, W), 1).double(), lr.normal((B, C, H, W), 2).double()
    m, s, t = lr.normal((C,), 3, 3.0).double(), lr.normal((C,), 4).abs().double() + 0.5, lr.normal((C,), 5).abs().double() + 0.1
    st = Stats(m, s, {6: t}, C, 0)
    st.x_mean, st.x_std, st.t_std = m.view(-1, 1, 1), s.view(-1, 1, 1), {6: t.view(-1, 1, 1)}  # (Stats casts to fp32: keep fp64)
    phys = st.unstandardize_x(x) + st.unstandardize_t(y, 6)
    xstd = st.standardize_x(phys)
    p, q, bound = lr.rollout_ref(x.reshape(B, C, -1), y.reshape(B, C, -1), m, s, t)
    assert float((p - phys.reshape(B, C, -1)).abs().max()) <= 1e-12 and float((q - xstd.reshape(B, C, -1)).abs().max()) <= 1e-12
    q2, b2 = lr.rollout_xstd_from(p, m, s)
    assert torch.equal(q2, q) and bool((b2 > 0).all()) and bool((bound > 0).all())


@pytest.mark.parametrize("case", PATCHIFY_CASES, ids=lambda c: c.name)
def test_patchify_cases_reach_the_kernel_they_name(case):
    B, H, W = case.B, case.H, case.W
    for dt_bytes in (4, 2):
        src_align = tuple((4 * case.misalign) % 16 if s == case.misaligned_source else 0 for s in range(3))
        assert lr.patchify_path(case.chans, B, H, W, case.patch, case.lda, 0, src_align) == case.path
    F = case.patch[0] * case.patch[1] * sum(case.chans)
    assert case.lda >= F and H % case.patch[0] == 0 and W % case.patch[1] == 0
    if case.past_cap:
        gh, gw = H // case.patch[0], W // case.patch[1]
        assert lr.CAP < B * gh * gw * case.lda <= lr.CAP + 8192
    if "64 KiB" in case.name:
        assert sum(case.chans) * case.patch[0] * (16 * case.patch[1] + 4) * 4 > 64 * 1024
    # tagged inputs: below 2^24 and unique
    srcs, offs = patchify_inputs(case, "tagged")
    flat = torch.cat([s.reshape(-1) for s in srcs if s is not None])
    assert float(flat.max()) < 2 ** 24 and flat.unique().numel() == flat.numel()


@pytest.mark.parametrize("case", UNPATCHIFY_CASES, ids=lambda c: c.name)
def test_unpatchify_cases_reach_the_kernel_they_name(case):
    for wide in (0, case.wide):
        ldt = case.C * case.patch[0] * case.patch[1] + case.ldt_extra + wide
        xt_align = (4 * case.xt_misalign) % 16
        assert lr.unpatchify_path(case.H, case.W, case.patch, ldt, 0, 0, xt_align) == case.path, (ldt,)
        assert lr.unpatchify_path(case.H, case.W, case.patch, ldt, 0, 0, 0) == (case.path if not case.xt_misalign else "fast4")
    if case.past_cap:
        assert lr.CAP < case.B * case.C * case.H * case.W <= lr.CAP + 8192
    n = case.B * (case.H // case.patch[0]) * (case.W // case.patch[1]) * (case.C * case.patch[0] * case.patch[1] + case.ldt_extra + case.wide)
    assert 1 + n < 2 ** 24


@pytest.mark.parametrize("case", LINEAR_CASES, ids=lambda c: c.name)
def test_linear_small_cases_reach_the_kernel_they_name_and_sum_exactly(case):
    assert lr.linear_small_path(case.B, case.N, case.K, case.ldx, case.ldw) == case.path
    x, w, b, p2 = linear_operands(case)
    # in units of the operands' common power of two every partial sum of every order is an integer below 2^24
    scale = 2.0 ** p2
    assert lr.linear_small_max_partial(x, w, b) / scale < 2 ** 24
    assert torch.equal((x / 2.0 ** case.px), (x / 2.0 ** case.px).round()) and torch.equal(w, w.round())
    if case.act:
        z = lr.linear_small_ref(x, w, b)
        assert float(z.min()) < -15 and float(z.max()) > 15 and float(z.abs().max()) < 40


def test_conversion_table_is_what_torch_rounds_to():
    f, want = lr.edge_values(len(lr.CONVERSION_TABLE))
    got = lr.bf16_bits(f.bfloat16())
    for e, g, w in zip(lr.CONVERSION_TABLE, got.tolist(), want.tolist()):
        assert g == w == e.bf16, f"{e.name}: torch {g:#06x}, table {e.bf16:#06x}"
    assert torch.equal(lr.rne_bf16_bits(f), want)
    x = lr.normal((4096,), 9)
    assert torch.equal(lr.rne_bf16_bits(x), lr.bf16_bits(x.bfloat16()))
    names = " ".join(e.name for e in lr.CONVERSION_TABLE)
    for claim in ("even below", "even above", "next binade", "-0.0", "subnormal", "below the bf16 overflow", "overflow point"):
        assert claim in names


def test_sum_gathers_on_small_integers():
    src = lr.integers((6, 5), 1)
    src[:, 3:] = float("nan")  # behind the valid columns
    bias, pos = lr.embed_bwd_sums_ref(src, 3, 3)
    assert torch.equal(bias, src[:, :3].double().sum(0)) and torch.equal(pos, src[:3, :3].double() + src[3:, :3].double())
    assert torch.equal(lr.colsum_ref(src, 3, 0), bias) and torch.equal(lr.colsum_ref(src, 3, 3), pos)
    flat = lr.integers((2 * 40,), 2)
    got = lr.reduce_slabs_ref(flat, 5, 40, 2, 4, 3, prefill=torch.ones(4, 3))
    want = 1 + flat[:40].view(8, 5)[:4, :3].double() + flat[40:].view(8, 5)[:4, :3].double()
    assert torch.equal(got, want)


def test_walk_restatement_equals_division_of_the_tile_number():
    for ntm in range(1, 13):
        for ntn in range(1, 13):
            for gm in range(1, 10):
                want = [lr.tile_coords(t, ntm, ntn, gm) for t in range(ntm * ntn)]
                for stride in range(1, 41):
                    for vid in range(min(stride, ntm * ntn)):
                        for st in lr.walk_trace(ntm, ntn, gm, stride, vid):
                            assert st.coords == want[st.tile], (ntm, ntn, gm, stride, vid, st)


def test_walk_restatement_visits_every_tile_once():
    for ntm, ntn, gm, stride in ((10, 3, 4, 7), (12, 2, 4, 13), (3, 2, 8, 4), (8, 3, 8, 5)):
        seen = sorted(st.tile for vid in range(stride) for st in lr.walk_trace(ntm, ntn, gm, stride, vid))
        assert seen == list(range(ntm * ntn))


@pytest.mark.parametrize("case", lr.WALK_CASES, ids=lambda c: c.name)
def test_walk_cases_take_the_carries_they_claim(case):
    ntm, ntn = -(-case.M // lr.BM), -(-case.N // lr.BN)
    assert case.M % lr.BM == 0 and case.N % lr.BN == 0  # interior tiles only: the straight-line epilogue runs on every one
    claims = case.claims
    steps = [st for bid in range(case.wgs) for st in lr.walk_trace(ntm, ntn, case.gm, case.wgs, lr.vid_of(bid, case.wgs))]
    assert sorted(st.tile for st in steps) == list(range(ntm * ntn))
    assert ntm * ntn > case.wgs  # (at least one workgroup steps)
    moved = [st for bid in range(case.wgs) for st in lr.walk_trace(ntm, ntn, case.gm, case.wgs, lr.vid_of(bid, case.wgs))[1:]]
    if "digits" in claims:
        assert lr.walk_digits(case.wgs, ntn, case.gm) == claims["digits"]
    if claims.get("c1_most"):
        assert sum(st.carry1 for st in moved) * 2 > len(moved)
    if claims.get("both"):
        assert any(st.carry1 and st.carry2 for st in moved)
    if "short_rows" in claims:
        assert ntm % case.gm == claims["short_rows"]
    if claims.get("short_carry"):
        assert any((st.carry1 or st.carry2) and st.short for st in moved)
    if claims.get("short_first"):
        assert all(st.short for st in steps) and ntm < case.gm
    if "gm" in claims:
        # (the row digit has radix 1: it never moves, the first carry never fires and the column digit carries alone)
        assert case.gm == claims["gm"] == 1 and not any(st.carry1 for st in moved) and any(st.carry2 for st in moved)
    if "ntn" in claims:
        assert ntn == claims["ntn"] and any(st.carry2 for st in moved)
