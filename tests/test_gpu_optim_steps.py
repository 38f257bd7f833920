"""-m gpu: swiftk_adamw_ema_step and swiftk_mars_ema_step, the two kernels that write the parameters, scored chunk by chunk
against the float64 closed form of tests/optim_reference.py (designs, yardstick and score are described and checked there and in
tests/test_optim_reference_cpu.py).  Every design runs twice: through the raw C ABI with hand-built chunk tables and hyper
structs (so pointer alignment can be chosen), and through FusedAdamEMA / FusedMarsEMA (so the host's arithmetic, step_t and the
param_groups are under test).  A chunk passes when err_kernel <= 4 * max(err_yardstick, storage floor); the exact designs must
come out bit for bit.

Two defects these tests found, with the figures before and after (MI355X, worst chunk, err_kernel / bound's base):
  * adamw_ema_kernel formed 1.0f - beta1 and 1.0f - beta2 on the device from the fp32-rounded betas; torch rounds the double
    1 - beta.  At t = 1 (v = (1 - beta2) g^2, m = (1 - beta1) g) that was m 2.4e-07 at every beta1 = 0.9 design (4.08 x the
    floor 5.96e-08), v 2.4e-07 at beta2 0.95 (4.09 x), dp 7.6e-07 at (0.9, 0.99) (4.1 x) and dp 6.6e-06 at (0.9, 0.999)
    (35 x), v 6.5e-07 at t = 2 of the small-gradient design (10.8 x): 14 designs missed, by either route.  swiftk_opt_hyper now carries
    one_minus_beta1 / one_minus_beta2 from the host as swiftk_mars_hyper does: m 4.0e-08, v 6.3e-08, dp 1.8e-07 at (0.9, 0.999),
    every ratio <= 1.00.
  * mars_update_kernel gave an element different bits in its 16-byte and its dword loop (p of the unclipped AdamW-1d tensor
    differed between a chunk on a 16-byte boundary and the same chunk 4 bytes off it): the compiler contracted different
    multiply-add pairs in the two inlined copies of mars_elem.  The multiply-adds are now spelled out and contraction is off in
    mars_elem / ema_lerp; the two forms agree bit for bit wherever no clip is applied.
"""
import ctypes as C

import pytest
import torch

import optim_reference as R
from test_gpu_mars import NORM_TOL

pytestmark = pytest.mark.gpu
FIELDS = ("P", "E", "M", "V", "L")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _refs(name):
    if name in R.BIG:
        c = R.case(name)
        return c, R.rule(c), R.torch_ops(c)
    return (R.case(name),) + R.references(name)


# ------------------------------------------------------------------------------------------------------- the raw C ABI
def _hyper(c):
    """The hyper struct as include/swiftk.h documents its fields, from the case's Python doubles."""
    from swift_amd import _lib
    b1, b2 = c.betas
    t = c.t
    if not c.mars:
        h = _lib.OptHyper()
        for gi, (lr, wd) in enumerate(c.groups):
            h.lr[gi], h.weight_decay[gi], h.step_size[gi] = lr, wd, lr / (1.0 - b1 ** t)
        h.beta1, h.beta2, h.eps, h.bias2_sqrt, h.ema_beta = b1, b2, c.eps, (1.0 - b2 ** t) ** 0.5, c.ema_beta
        h.one_minus_beta1, h.one_minus_beta2 = 1.0 - b1, 1.0 - b2
        h.decoupled = int(c.kind == "adamw")
        return h
    h = _lib.MarsHyper()
    f = c.lr_1d / c.lr0
    for gi, (lr, wd) in enumerate(c.groups):
        h.neg_lr[gi], h.neg_lr_1d[gi], h.weight_decay[gi] = -lr, -lr * f, wd
    c1, c2 = c.betas_1d
    h.beta1, h.one_minus_beta1, h.beta2, h.one_minus_beta2 = b1, 1.0 - b1, b2, 1.0 - b2
    h.bias1, h.inv_bias2_sqrt = 1.0 - b1 ** t, 1.0 / (1.0 - b2 ** t) ** 0.5
    h.beta1_1d, h.one_minus_beta1_1d, h.beta2_1d, h.one_minus_beta2_1d = c1, 1.0 - c1, c2, 1.0 - c2
    h.bias1_1d, h.inv_bias2_sqrt_1d = 1.0 - c1 ** t, 1.0 / (1.0 - c2 ** t) ** 0.5
    h.weight_decay_1d, h.gamma_ratio, h.eps, h.ema_beta = c.weight_decay_1d, c.gamma * (b1 / (1.0 - b1)), c.eps, c.ema_beta
    h.mars_type = _lib.MARS_ADAMW if c.kind == "mars-adamw" else _lib.MARS_LION
    h.n_groups = len(c.groups)
    return h


class Raw:
    """Device buffers and a chunk table for one case.  p and ema are views of one arena each, every tensor starting on a
    16-byte boundary plus p_off / e_off elements; partials and tensor_norms are seeded with NaN."""

    def __init__(self, c, dev, p_off=0, e_off=0):
        from swift_amd import _lib
        self.c, self.lib = c, _lib.lib()
        cat = lambda xs: torch.cat([x.flatten() for x in xs]).to(dev)
        self.g, self.m, self.v = cat(c.G), cat(c.M), cat(c.V)
        self.last = cat(c.L) if c.mars else None
        ns = [R.numel(sh) for sh in c.shapes]
        starts, o = [], 0
        for n in ns:
            starts.append(o)
            o += -(-n // 4) * 4
        self.pa, self.ea = torch.zeros(o + 4, device=dev), torch.zeros(o + 4, device=dev)
        assert self.pa.data_ptr() % 16 == 0 and self.ea.data_ptr() % 16 == 0
        self.p = [self.pa[s + p_off:s + p_off + n] for s, n in zip(starts, ns)]
        self.e = [None if x is None else self.ea[s + e_off:s + e_off + n] for s, n, x in zip(starts, ns, c.E)]
        for dst, src in zip(self.p + self.e, c.P + c.E):
            if dst is not None:
                dst.copy_(src.flatten())
        rows = R.chunk_table(c)
        arr = ((_lib.MarsChunk if c.mars else _lib.OptChunk) * len(rows))()
        for a, r in zip(arr, rows):
            ti, s = r["tensor"], r["start"]
            a.p = self.p[ti].data_ptr() + 4 * s
            a.ema = None if self.e[ti] is None else self.e[ti].data_ptr() + 4 * s
            a.flat_off, a.n, a.group = r["flat_off"], r["n"], r["group"]
            if c.mars:
                a.tensor, a.first_chunk, a.tensor_chunks, a.rule = ti, r["first"], r["count"], r["rule"]
        self.rows = rows
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
        self.partials = torch.full((len(rows),), float("nan"), device=dev)
        self.norms = torch.full((len(ns),), float("nan"), device=dev)
        self.h = _hyper(c)

    def args(self):
        a = [self.table.data_ptr(), len(self.rows), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr()]
        if self.c.mars:
            a += [self.last.data_ptr(), self.partials.data_ptr(), self.norms.data_ptr()]
        return a

    def call(self, args=None, hyper="own"):
        fn = self.lib.swiftk_mars_ema_step if self.c.mars else self.lib.swiftk_adamw_ema_step
        h = self.h if hyper == "own" else hyper
        return fn(*(self.args() if args is None else args), None if h is None else C.byref(h),
                  torch.cuda.current_stream().cuda_stream)

    def buffers(self):
        return [t for t in (self.g, self.m, self.v, self.last, self.pa, self.ea, self.partials, self.norms) if t is not None]

    def result(self):
        torch.cuda.synchronize()
        c, out, o = self.c, R.Result(), 0
        for ti, sh in enumerate(c.shapes):
            n = R.numel(sh)
            sl = slice(o, o + n)
            out.P.append(self.p[ti].cpu()), out.E.append(None if self.e[ti] is None else self.e[ti].cpu())
            out.M.append(self.m[sl].cpu()), out.V.append(self.v[sl].cpu()), out.G.append(self.g[sl].cpu())
            out.L.append(self.last[sl].cpu() if c.mars else None)
            o += n
        out.norms = self.norms.cpu().tolist()
        return out


def run_raw(c, dev, p_off=0, e_off=0):
    raw = Raw(c, dev, p_off, e_off)
    assert raw.call() == 0
    got = raw.result()
    if c.mars:  # launch 1 writes every entry of partials (0 for AdamW-1d chunks), launch 2 every tensor's norm
        part = raw.partials.cpu()
        assert bool(torch.isfinite(part).all())
        assert all(float(part[i]) == 0.0 for i, r in enumerate(raw.rows) if r["rule"] == 1)
    return got


# --------------------------------------------------------------------------------------------------- the fused classes
class Fused:
    def __init__(self, c, dev):
        from swift_amd.training.fused_optim import FusedAdamEMA, FusedMarsEMA
        from swift_amd.training.optimizers.mars import MARS
        self.P = [torch.nn.Parameter(torch.zeros(sh, device=dev)) for sh in c.shapes]
        self.E = [None if e is None else torch.zeros(sh, device=dev) for e, sh in zip(c.E, c.shapes)]
        groups = [dict(params=[p for p, g in zip(self.P, c.group_of) if g == gi], lr=lr, weight_decay=wd)
                  for gi, (lr, wd) in enumerate(c.groups)]
        if c.mars:
            self.opt = MARS(groups, lr=c.lr0, betas=c.betas, eps=c.eps, gamma=c.gamma, mars_type=c.kind, lr_1d=c.lr_1d,
                            betas_1d=c.betas_1d, weight_decay_1d=c.weight_decay_1d)
        else:
            self.opt = (torch.optim.AdamW if c.kind == "adamw" else torch.optim.Adam)(groups, betas=c.betas, eps=c.eps)
        self.flat = torch.zeros(sum(p.numel() for p in self.P), device=dev)
        o = 0
        for p in self.P:
            p.grad = self.flat[o:o + p.numel()].view_as(p)
            o += p.numel()
        self.f = (FusedMarsEMA if c.mars else FusedAdamEMA)(self.opt, self.P, self.E, self.flat)
        assert self.f.n_chunks == len(R.chunk_table(c))

    def seat(self, c):
        """Put the case's state into the object: state through the optimizer's own state dict views, lr and weight decay
        through param_groups (as the schedule does), the count through step_t."""
        cat = lambda xs: torch.cat([x.flatten() for x in xs])
        with torch.no_grad():
            for p, e, cp, ce in zip(self.P, self.E, c.P, c.E):
                p.copy_(cp)
                if e is not None:
                    e.copy_(ce)
            self.flat.copy_(cat(c.G))
            self.f.m.copy_(cat(c.M)), self.f.v.copy_(cat(c.V))
            if c.mars:
                self.f.last.copy_(cat(c.L))
                self.f.norms.fill_(float("nan")), self.f.partials.fill_(float("nan"))
        for g, (lr, wd) in zip(self.opt.param_groups, c.groups):
            g["lr"], g["weight_decay"] = lr, wd
        self.f.step_t.fill_(float(c.t - 1))

    def step(self, c):
        self.seat(c)
        self.f.step(c.ema_beta)
        torch.cuda.synchronize()
        assert float(self.f.step_t) == float(c.t)
        out, o = R.Result(), 0
        for p, e in zip(self.P, self.E):
            n = p.numel()
            sl = slice(o, o + n)
            st = self.opt.state[p]
            out.P.append(p.detach().flatten().cpu()), out.E.append(None if e is None else e.flatten().cpu())
            out.M.append(st["exp_avg"].flatten().cpu()), out.V.append(st["exp_avg_sq"].flatten().cpu())
            out.L.append(st["last_grad"].flatten().cpu() if c.mars else None)
            out.G.append(self.flat[sl].cpu())
            o += n
        out.norms = self.f.norms.cpu().tolist() if c.mars else [0.0] * len(self.P)
        return out


# ------------------------------------------------------------------------------------------------------------ checking
def same(a, b):
    """Bit-equal results (None where a tensor has no EMA copy)."""
    return all((x is None and y is None) or torch.equal(x, y) for f in FIELDS + ("G",)
               for x, y in zip(getattr(a, f), getattr(b, f)))


def verify(c, got, ref, yard, route):
    for ti in range(len(c.shapes)):
        assert torch.equal(got.G[ti], yard.G[ti]), (c.name, ti, "gradient not left sanitised bit for bit")
        if c.mars:
            assert torch.equal(got.L[ti], yard.G[ti]), (c.name, ti, "last_grad")
            want = ref.norms[ti]
            if c.mars_rule(ti):
                assert got.norms[ti] == pytest.approx(want, rel=NORM_TOL), (c.name, ti)
            else:
                assert got.norms[ti] == 0.0, (c.name, ti)
        if not c.scores_v(ti):
            assert torch.equal(got.V[ti], c.V[ti].flatten()), (c.name, ti, "mars-lion touched exp_avg_sq")
        if got.E[ti] is not None and c.ema_beta == 0.0:
            assert torch.equal(got.E[ti], got.P[ti]), (c.name, ti)
        if got.E[ti] is not None and c.ema_beta == 1.0:
            assert torch.equal(got.E[ti], c.E[ti].flatten()), (c.name, ti)
        if c.name.endswith("-zero"):
            for x in (got.M[ti], got.V[ti]):
                assert float(x.abs().max()) == 0.0 and not bool(torch.signbit(x).any()), (c.name, ti)
            if float(c.P[ti].abs().max()) == 0.0:
                assert float(got.P[ti].abs().max()) == 0.0
            if c.kind == "adam":
                assert torch.equal(got.P[ti], c.P[ti].flatten())
        if c.exact:
            for f in FIELDS:
                a, b = getattr(got, f)[ti], getattr(ref, f)[ti]
                if a is not None:
                    assert torch.equal(a, b.float()) and torch.equal(a.double(), b), (c.name, f, ti)
            if c.mars:
                assert got.norms[ti] == R.exact_norm(c, ti), (c.name, ti, got.norms[ti])
    fails, worst = R.judge(c, got, yard, ref)
    print(f"[{route}] {R.describe(c, worst)}")
    assert not fails, (c.name, route, len(fails), fails[:4])


# --------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("name", R.NAMES + R.BIG)
def test_raw_abi_per_chunk_vs_fp64(dev, name):
    """Every design through swiftk_adamw_ema_step / swiftk_mars_ema_step themselves, p and ema on 16-byte boundaries; partials and
    tensor_norms start as NaN (AdamW-1d entries must read 0, the others the norm).
    measured on MI355X, worst chunk per design family as err_kernel / max(err_yardstick, floor), with the largest err_kernel:
    Adam / AdamW  steps t 1..100000: dp 0.44-0.98 (5.4e-07), m 0.49-0.68 (4.0e-08), v 0.45-1.00 (6.3e-08), de 0.49-0.68 (5.2e-07);
      betas x t 1 / 1000: dp <= 0.93, m <= 0.68, v <= 1.00 (7.8e-08), de <= 0.51; small gradients: dp <= 0.91 (2.3e-07),
      v <= 1.00; non-finite: m <= 0.98, v <= 0.82; ema_beta 0 .. 1: de <= 0.68 (5.9e-04 at the half-life beta, where the
      yardstick's own 1 - (float)beta carries the same error); zero gradient: m = v = +0, dp 0.53 (2.3e-04 of lr wd p, floor 4.3e-04).
    MARS  steps: dp <= 0.64 (4.9e-07), m <= 0.76, v <= 0.97 (6.6e-08), de <= 0.59; ema_beta: de <= 0.55; mars-lion on 363
      chunks: dp 0.57-0.60 (1.1e-07), m <= 0.61; 534-chunk tensor: dp 0.42, m 0.59, v 0.45, de 0.49; non-finite (c_t divided by a
      norm of about 2e5): m 1.45 (8.7e-08), v 1.37 (8.2e-08), the largest ratios of the file (1 / norm as a factor against a
      division).  Exact designs: every error 0, norms exactly 1.0 and 2.0 on 4 and on 1024 chunks."""
    c, ref, yard = _refs(name)
    verify(c, run_raw(c, dev), ref, yard, "raw")


FUSED = dict(R.SEQUENCES)
FUSED.update({n: (n,) for n in R.NAMES if not any(n in s for s in R.SEQUENCES.values())})


@pytest.mark.parametrize("key", list(FUSED))
def test_fused_classes_per_chunk_vs_fp64(dev, key):
    """The same designs through FusedAdamEMA / FusedMarsEMA: step_size, bias2_sqrt and friends come from the classes' host
    arithmetic at the step_t set here (1, 2, 1000, 100000).  A sequence's second step runs on the same object after
    param_groups[i]["lr"] has been changed, so a stale learning rate misses the dp bound; every step is taken twice from equal
    state and must repeat bit for bit, and must equal the raw-ABI run of the same case bit for bit (the test's own hyper struct
    against the classes').  measured on MI355X: the figures of test_raw_abi_per_chunk_vs_fp64, digit for digit.  The 4^12
    exact designs run through the raw ABI only (67 MB per buffer)."""
    fused = None
    for name in FUSED[key]:
        c, ref, yard = _refs(name)
        fused = fused or Fused(c, dev)
        got = fused.step(c)
        verify(c, got, ref, yard, "fused")
        assert same(got, fused.step(c)), (name, "a second run from equal state differs")
        assert same(got, run_raw(c, dev)), (name, "raw ABI and fused class differ")


ALIGN = ("mars-adamw-t2", "mars-adamw-nonfinite", "mars-adamw-ema0.5", "mars-lion-s2", "exact-mars-adamw-256-norm1",
         "exact-mars-adamw-256-norm2", "exact-mars-lion-256-norm1", "exact-mars-lion-256-norm2")


@pytest.mark.parametrize("name", ALIGN)
def test_mars_vector_and_dword_forms_agree(dev, name):
    """mars_chunk_vec4 picks 16-byte or dword accesses per chunk from flat_off, p and ema.  The same data with p, ema or both
    carved 4 bytes off the boundary: every run within the per-chunk bounds and NORM_TOL; tensors that are not clipped (the two
    forms differ only in the order of the sum of squares) bit-equal to the aligned run in p, m, v, e and last.
    measured on MI355X: clipped tensors move in the third digit between the forms (mars-adamw-t2 de 7.24e-08
    aligned, 7.18e-08 with p off the boundary; mars-lion-s2 dp 1.07e-07 / 1.10e-07), ratios 0.53-0.97 in every form; norms agree
    within NORM_TOL.  Before the fix in mars_elem the unclipped 1-D tensor's p differed between the forms in four designs."""
    c, ref, yard = _refs(name)
    base = run_raw(c, dev)
    verify(c, base, ref, yard, "raw 0/0")
    for p_off, e_off in ((1, 0), (0, 1), (1, 1)):
        got = run_raw(c, dev, p_off, e_off)
        verify(c, got, ref, yard, f"raw {p_off}/{e_off}")
        for ti in range(len(c.shapes)):
            if ref.norms[ti] <= 1.0:
                for f in FIELDS:
                    a, b = getattr(got, f)[ti], getattr(base, f)[ti]
                    assert a is None or torch.equal(a, b), (name, p_off, e_off, f, ti)


def _refused(raw, calls):
    """Every call returns its code before anything is launched: afterwards no buffer has changed."""
    keep = [t.clone() for t in raw.buffers()]
    for what, want, kw in calls:
        assert raw.call(**kw) == want, what
    torch.cuda.synchronize()
    for a, b in zip(keep, raw.buffers()):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "a refused call wrote to a buffer"


def test_mars_step_refusals_leave_every_buffer_unchanged(dev):
    from swift_amd import _lib
    c = R.case("exact-mars-adamw-256-norm1")
    raw = Raw(c, dev)
    ok = raw.args()
    sub = lambda i, v: dict(args=ok[:i] + [v] + ok[i + 1:])
    calls = [(f"NULL argument {i}", -1, sub(i, None)) for i in (0, 2, 3, 4, 5, 6)]
    calls += [("NULL hyper", -1, dict(hyper=None)), ("n_chunks 0", -1, sub(1, 0)), ("n_chunks -1", -1, sub(1, -1))]
    for groups in (0, _lib.OPT_MAX_GROUPS + 1):
        h = _hyper(c)
        h.n_groups = groups
        calls.append((f"n_groups {groups}", -1, dict(hyper=h)))
    for kind in (-1, 2):
        h = _hyper(c)
        h.mars_type = kind
        calls.append((f"mars_type {kind}", -1, dict(hyper=h)))
    calls += [(f"flat buffer {i} off the 16-byte boundary", -3, sub(i, ok[i] + 4)) for i in (2, 3, 4, 5)]
    _refused(raw, calls)
    assert raw.call(args=ok[:7] + [None]) == 0   # tensor_norms may be NULL
    torch.cuda.synchronize()
    assert bool(torch.isnan(raw.norms).all()) and bool(torch.isfinite(raw.partials).all())


def test_adamw_step_refusals_leave_every_buffer_unchanged(dev):
    c = R.case("exact-adamw")
    raw = Raw(c, dev)
    ok = raw.args()
    sub = lambda i, v: dict(args=ok[:i] + [v] + ok[i + 1:])
    calls = [(f"NULL argument {i}", -1, sub(i, None)) for i in (0, 2, 3, 4)]
    calls += [("NULL hyper", -1, dict(hyper=None)), ("n_chunks 0", -1, sub(1, 0)), ("n_chunks -1", -1, sub(1, -1))]
    _refused(raw, calls)
