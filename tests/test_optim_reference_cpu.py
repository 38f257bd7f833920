"""The yardsticks of tests/test_gpu_optim_steps.py checked on the CPU: the float64 closed forms against the optimizer classes
themselves in float64, the exact designs against their stated answers, the chunk lists, and the per-chunk score against
deliberately wrong restatements of the rule.  No GPU, no kernel: what is under test here is the test."""
import pytest
import torch

import optim_reference as R

FIELDS = ("P", "E", "M", "V", "L", "G")
EXACT = tuple(n for n in R.NAMES + R.BIG if n.startswith("exact-"))


def _rel(a, b):
    d = float((a.double() - b.double()).norm())
    return 0.0 if d == 0.0 else d / float(b.double().norm())


@pytest.mark.parametrize("name", R.NAMES)
def test_closed_form_equals_the_optimizer_classes_in_float64(name):
    """rule() in float64 against torch.optim.Adam / AdamW (foreach=False) and the MARS class run on float64 tensors, lerp after
    them: 1e-13 in every tensor of p, ema, both moments, last_grad and the sanitised gradient, non-finite gradients included."""
    c = R.case(name)
    r, y = R.rule(c), R.torch_ops(c, torch.float64)
    for f in FIELDS:
        if f == "L" and not c.mars:
            continue
        for ti, (a, b) in enumerate(zip(getattr(r, f), getattr(y, f))):
            if b is None:
                assert a is None
                continue
            assert torch.isfinite(a).all() and torch.isfinite(b).all()
            assert _rel(a, b) <= 1e-13, (name, f, ti, _rel(a, b))


@pytest.mark.parametrize("name", EXACT)
def test_exact_designs_are_exact(name):
    """Every value of the float64 form is an fp32 number, and the fp32 yardstick produces those bits."""
    c = R.case(name)
    assert c.exact
    r, y = R.rule(c), R.torch_ops(c)
    for f in FIELDS:
        if f == "L" and not c.mars:
            continue
        for ti, (a, b) in enumerate(zip(getattr(r, f), getattr(y, f))):
            if b is None:
                assert a is None
                continue
            assert torch.equal(a.float().double(), a), (name, f, ti)
            assert torch.equal(a.float(), b) and not torch.signbit(b[b == 0]).any(), (name, f, ti)
    for ti in range(len(c.shapes)):
        g, p = c.G[ti].double().flatten(), c.P[ti].double().flatten()
        if not c.mars:
            lr, wd = c.groups[c.group_of[ti]]
            assert torch.equal(r.M[ti], g / 2) and torch.equal(r.V[ti], g * g / 4)
            assert torch.equal(r.P[ti], p * (1 - lr * wd) - lr * torch.sign(g))
        else:
            assert r.norms[ti] == R.exact_norm(c, ti)
            if c.kind == "mars-lion" and c.mars_rule(ti):
                assert float(r.V[ti].abs().max()) == 0.0
    if c.mars:
        assert {R.exact_norm(c, 0)} <= {1.0, 2.0} and R.exact_norm(c, 1) == 0.0
        side = c.shapes[0][0]
        assert R.numel(c.shapes[0]) == side * side and len(R.chunk_table(c)) == side * side // R.CHUNK + 1


def test_exact_adam_design_covers_the_chunk_lengths_and_eight_groups():
    for kind in R.ADAM_KINDS:
        c = R.case(f"exact-{kind}")
        rows = R.chunk_table(c)
        assert {1, 3, 4, 5, 255, 256, 257, 16383, 16384} <= {r["n"] for r in rows}
        assert {r["group"] for r in rows} == set(range(8)) and len({g for g in c.groups}) == 8
        assert any(e is None for e in c.E) and any(e is not None for e in c.E)
        assert any(r["flat_off"] % 4 for r in rows) and any(r["flat_off"] % 4 == 0 for r in rows)


@pytest.mark.parametrize("name", ("mars-lion-s1", "mars-lion-s2"))
def test_lion_margin_holds(name):
    """|m| >= 1e-3 rms(m) on every element of the float64 first moment: every sign is determined, nothing is excluded."""
    c = R.case(name)
    assert R.lion_margin(c) >= 1e-3
    assert len(R.chunk_table(c)) >= 363 + 2


@pytest.mark.parametrize("name", R.NAMES + R.BIG[:1])
def test_chunk_list_tiles_the_tensors(name):
    c = R.case(name)
    rows, off = R.chunk_table(c), 0
    it = iter(rows)
    for ti, sh in enumerate(c.shapes):
        start, first = 0, None
        while start < R.numel(sh):
            r = next(it)
            first = rows.index(r) if first is None else first
            assert (r["tensor"], r["start"], r["flat_off"], r["group"]) == (ti, start, off + start, c.group_of[ti])
            assert 0 < r["n"] <= R.CHUNK and r["first"] == first and r["count"] == -(-R.numel(sh) // R.CHUNK)
            start += r["n"]
        assert start == R.numel(sh)
        off += start
    assert next(it, None) is None


def test_designs_cover_what_they_claim():
    c = R.case("mars-adamw-t1000")
    r = R.rule(c)
    assert len(R.chunk_table(c)) == 40
    assert r.norms[0] > 1.05 and r.norms[2] > 1.05 and 0 < r.norms[3] < 0.95 and 0 < r.norms[4] < 0.95 and r.norms[1] == 0.0
    offs = [row["flat_off"] for row in R.chunk_table(c) if row["start"] == 0]
    assert [o % 4 for o in offs] == [0, 0, 0, 3, 2]
    big = R.case("mars-adamw-large")
    assert len(R.chunk_table(big)) == 534 + 1 and abs(R.rule(big).norms[0] - 1.0) > 0.05
    g = torch.cat([x.flatten() for x in R.case("adamw-small-t1").G]).abs()
    assert 1e-13 <= float(g.min()) and float(g.max()) <= 1e-9
    nf = R.case("adamw-nonfinite")
    assert sum(int((~torch.isfinite(x)).sum()) for x in nf.G) == 9
    assert R.case("adamw-t2").groups != R.case("adamw-t1").groups      # the schedule moved the learning rates
    for k in ("adam", "adamw", "mars-adamw"):
        z = R.case(f"{k}-zero")
        assert all(float(x.abs().max()) == 0.0 for x in z.G + z.M + z.V) and float(z.P[1].abs().max()) == 0.0
    for name in R.NAMES:   # p stays within about 8 lr of zero wherever dp is scored
        c = R.case(name)
        for ti, p in enumerate(c.P):
            lr = c.groups[c.group_of[ti]][0] * (1.0 if c.mars_rule(ti) or not c.mars else max(1.0, c.lr_1d / c.lr0))
            assert float(p.abs().pow(2).mean().sqrt()) <= 8 * lr, (name, ti)


@pytest.mark.parametrize("name", R.NAMES)
def test_yardstick_passes_its_own_bounds_and_is_finite(name):
    c = R.case(name)
    r, y = R.references(name)
    for f in FIELDS:
        assert all(x is None or bool(torch.isfinite(x).all()) for x in getattr(y, f))
    fails, worst = R.judge(c, y, y, r)
    assert not fails and all(w[0] <= 1.0 for w in worst.values())


WRONG = [("eps_first", "adamw-small-t1"), ("eps_first", "adam-small-t2"), ("neighbour_group", "adamw-t1000"),
         ("neighbour_group", "mars-adamw-t1000"), ("omb2", "adamw-beta0.999-t1"), ("omb2", "adamw-beta0.999-t1000"),
         ("omb2", "mars-adamw-t1"), ("clip_always", "mars-adamw-t1000"), ("lerp_single", "adamw-ema1"),
         ("lerp_single", "mars-adamw-ema1")]


@pytest.mark.parametrize("wrong,name", WRONG)
def test_score_rejects_wrong_variants(wrong, name):
    """An fp32 restatement of the rule passes every per-chunk bound; the same restatement with one defect (eps joined before the
    bias division, a chunk on its neighbour's group, 1 - beta2 off by a relative 1e-4, the clip applied to every tensor, the
    single-sided lerp formula) misses at least one."""
    c = R.case(name)
    r, y = R.references(name)
    fails, worst = R.judge(c, R.rule(c, torch.float32), y, r)
    assert not fails, (R.describe(c, worst), fails[:3])
    fails, worst = R.judge(c, R.rule(c, torch.float32, wrong=wrong), y, r)
    print(f"{wrong}: {R.describe(c, worst)}; {len(fails)} chunk bounds missed")
    assert fails
    want = {"eps_first": {"dp"}, "neighbour_group": {"dp"}, "omb2": {"v"}, "clip_always": {"m", "v", "dp"},
            "lerp_single": {"de"}}[wrong]
    assert want & {f[0] for f in fails}
    if wrong == "neighbour_group":   # exactly the one chunk
        assert {(f[1], f[2]) for f in fails if f[0] == "dp"} == {(0, 1)}


def test_clip_at_greater_or_equal_is_the_same_function():
    """`norm >= 1` differs from `norm > 1` only at a norm of exactly 1, where the scale 1 / norm is 1: the two are one function,
    so no score can (or needs to) tell them apart.  The exact design with a norm of exactly 1.0 pins that: both give the same
    bits.  What the design does reject is a clip that fires below 1 (clip_always above) and a kernel whose norm of 4^8 values of
    2^-8 is not exactly 1.0 (tensor_norms is compared for equality on the GPU)."""
    for kind in R.MARS_KINDS:
        c = R.case(f"exact-{kind}-256-norm1")
        a, b = R.rule(c, torch.float32), R.rule(c, torch.float32, wrong="clip_ge")
        assert a.norms[0] == 1.0
        for f in ("P", "E", "M", "V"):
            assert all(torch.equal(x, y) for x, y in zip(getattr(a, f), getattr(b, f)))


def test_opt_hyper_layout_mirrors_the_header():
    """swiftk_opt_hyper carries 1 - beta1 and 1 - beta2 from the host (csrc/train_kernels.hip static_asserts the same sizes), and
    FusedAdamEMA's arithmetic gives them torch's bits: the double 1 - beta rounded once."""
    import ctypes
    import os
    import re
    from swift_amd import _lib
    assert ctypes.sizeof(_lib.OptChunk) == 32 and ctypes.sizeof(_lib.OptHyper) == 4 * (3 * _lib.OPT_MAX_GROUPS + 8)
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "swiftk.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} swiftk_opt_hyper;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip().split("[")[0] for decl in body.split(";") if decl.strip()
             for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in _lib.OptHyper._fields_]
    h = _lib.OptHyper()
    for beta in (0.9, 0.95, 0.99, 0.999):
        h.one_minus_beta2 = 1.0 - beta
        assert h.one_minus_beta2 == float(torch.tensor(1.0 - beta, dtype=torch.float32))
    h.beta2 = 0.999
    assert abs((1.0 - h.beta2) / (1.0 - 0.999) - 1.0) > 1e-5   # what forming it from the rounded beta costs
