"""Place-by-place checks of the layout kernels between the matrix products, each called through the C ABI (include/swiftk.h):
patchify, un-patchify + affine, timestep embedding, small-batch linear, rollout update, axpby, the fp32 -> bf16 conversions and the
three column-sum gathers.  References, inputs, bounds and the case tables are tests/layout_reference.py (pinned to the oracle by
tests/test_layout_reference_cpu.py).  Outputs sit in buffers longer (and where the entry has a row stride, wider) than needed,
prefilled with a NaN sentinel; inputs carry NaN behind their valid columns; every comparison is per element and a failure prints the
count of wrong elements, the first wrong coordinate and -- for tagged inputs -- the source coordinate the wrong value decodes to.

Measured on an MI355X with this module as committed (126 tests, 2.2 s in all; the slowest, the rollout update past the grid cap, 0.5 s):

SiLU of swiftk_linear_small (act = 1; pre-activations in about [-27, 28], 20 000 of them per kernel): torch CPU fp32 silu is at most
1.267e-07 relative from fp64 SiLU of the exact pre-activation, so the allowance is 4 x that = 5.07e-07; each of the three kernels
(wave per feature, LDS with prefetch, LDS general walk) came to 1.267e-07 as well, a quarter of the allowance.

Largest observed fraction of each bound (none is used to less than 1 %, so none was tightened after the first run -- except that the
un-patchify betas were first 2, 0.5 and -0.75, whose products with a tag are exact: the one-rounding bound u |beta f| went unused at
0.0000, and the betas became 0.3, -1.1 and 0.7):
  axpby                                   2u (|a x| + |b y|)               0.96
  unpatchify_affine, beta only            u |beta f|                       0.93 (both kernels)
  unpatchify_affine, xt + alpha + beta    2u (|a x| + |b f|)               0.96 generic, 0.90 2 x 2 kernel
  unpatchify_affine, xt + beta            the same with alpha = 0          0.47
  patchify_scaled, general factor         2u |v| fp32, + half an ulp bf16  0.82 fp32, 1.00 bf16 (the rounding itself)
  rollout_update phys                     3u (|x s| + |m| + |y t|)         0.65
  rollout_update xstd from its own phys   4u (|p| + |m|) / |s|             0.46
  rollout_update xstd, fp64 chain         the two above combined           0.35
  timestep_embed sine | cosine            2^-22 (+ the aux bound)          0.23 | 0.25 alone, 0.21 | 0.19 with aux
  linear_small SiLU                       measured allowance               0.25
Everything else in this module is compared bit for bit.

Conversions: every entry of layout_reference.CONVERSION_TABLE -- ties in both directions, the carry into the next binade, -0.0, fp32
subnormals (kept, not flushed), the largest value below the bf16 overflow point and the overflow to infinity at and above it -- came
out as round-to-nearest-even through swiftk_cast_pad, both outputs of swiftk_cast_pad_t (with and without the row interleave) and the
bf16 patchify in both of its kernels.  The shared f2bf needed no change.
"""
import math

import pytest
import torch

import layout_reference as lr
from layout_reference import LINEAR_CASES, PATCHIFY_CASES, UNPATCHIFY_CASES, U

pytestmark = pytest.mark.gpu

USE = {}  # kernel -> largest observed fraction of its bound (printed by every test that updates it)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def L():
    from swift_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sent_f32(n, dev):
    return torch.full((n,), lr.SENT_F32, dtype=torch.int32, device=dev).view(torch.float32)


def _sent_bf16(n, dev):
    return torch.full((n,), lr.SENT_BF16, dtype=torch.int16, device=dev).view(torch.bfloat16)


def _is_sent(x):
    if x.dtype == torch.float32:
        return bool((x.contiguous().view(torch.int32) == lr.SENT_F32).all())
    return bool((x.contiguous().view(torch.int16) == lr.SENT_BF16).all())


def _nan_padded(valid, ld, dev):
    """[rows, ld] fp32 on the device: `valid` in the leading columns, NaN behind."""
    buf = torch.full((valid.shape[0], ld), float("nan"), dtype=torch.float32)
    buf[:, :valid.shape[1]] = valid
    return buf.to(dev)


def _first_bad(bad):
    idx = torch.nonzero(bad)
    return int(idx.shape[0]), tuple(int(v) for v in idx[0])


def _use(name, err, bound):
    """Record and print the largest fraction of `bound` that `err` uses (where the bound is positive)."""
    pos = bound > 0
    frac = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    USE[name] = max(USE.get(name, 0.0), frac)
    print(f"[bound use] {name}: {frac:.4f} (largest so far {USE[name]:.4f})")
    return frac


def _check_bits(name, got_bits, want_bits, decode=None):
    bad = got_bits != want_bits
    if bool(bad.any()):
        n, at = _first_bad(bad)
        g, w = int(got_bits[at]), int(want_bits[at])
        msg = f"{name}: {n} wrong elements, first at {at}: got bits {g:#x}, want {w:#x}"
        if decode is not None:
            msg += f"; the wrong value decodes to {decode(at)}"
        print(msg)
        raise AssertionError(msg)


def _check_bound(name, got, ref, bound, use=None, decode=None):
    """|got - ref| <= bound per element (got fp32 on the CPU, ref / bound fp64); bound 0 means the exact fp32 value."""
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)  # (a NaN in got is wrong as well)
    if use:
        _use(use, torch.nan_to_num(err, nan=float("inf")), bound)
    if bool(bad.any()):
        n, at = _first_bad(bad)
        msg = (f"{name}: {n} wrong elements, first at {at}: got {float(got[at])!r}, want {float(ref[at])!r} "
               f"+- {float(bound[at]):.3e}")
        if decode is not None:
            msg += f"; the wrong value decodes to {decode(at)}"
        print(msg)
        raise AssertionError(msg)


# ================================================================================================================= patchify
def _run_patchify(L, dev, case, srcs, scales, per_sample, dt):
    """-> (valid rows [rows, lda], guard rows) on the CPU."""
    p1, p2 = case.patch
    rows = case.B * (case.H // p1) * (case.W // p2)
    guard = 3
    n = (rows + guard) * case.lda
    out = (_sent_f32(n, dev) if dt == torch.float32 else _sent_bf16(n, dev)).view(rows + guard, case.lda)
    dsrc, keep = [], []
    for s, src in enumerate(srcs):
        if src is None:
            dsrc.append(None)
            continue
        if s == case.misaligned_source:  # a slice whose base is not on a 16-byte boundary
            buf = torch.zeros(src.numel() + 4, dtype=torch.float32, device=dev)
            view = buf[case.misalign:case.misalign + src.numel()]
            view.copy_(src.reshape(-1))
            assert view.data_ptr() % 16 != 0
            keep.append(buf)
            dsrc.append(view)
        else:
            dsrc.append(src.to(dev).contiguous())
            assert dsrc[-1].data_ptr() % 16 == 0
    ptr = [d.data_ptr() if d is not None else None for d in dsrc]
    code = 0 if dt == torch.float32 else 1
    if per_sample is None:
        rc = L.swiftk_patchify(ptr[0], case.chans[0], scales[0], ptr[1], case.chans[1], scales[1], ptr[2], case.chans[2], scales[2],
                               out.data_ptr(), case.lda, case.B, case.H, case.W, p1, p2, code, _stream())
    else:
        ps = per_sample.to(dev)
        rc = L.swiftk_patchify_scaled(ptr[0], case.chans[0], scales[0], ps.data_ptr(), ptr[1], case.chans[1], scales[1], ptr[2],
                                      case.chans[2], scales[2], out.data_ptr(), case.lda, case.B, case.H, case.W, p1, p2, code,
                                      _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = out.cpu()
    return out[:rows], out[rows:]


@pytest.mark.parametrize("case", PATCHIFY_CASES, ids=lambda c: c.name)
def test_patchify_places_every_element(L, dev, case):
    p1, p2 = case.patch
    F = p1 * p2 * sum(case.chans)
    # fp32 placement: tagged sources, power-of-two scales (and per-sample factors): every product is exact, one bit pattern expected
    srcs, offs = lr.patchify_inputs(case, "tagged")
    ps = torch.tensor([2.0, 0.25, 4.0][:case.B]) if case.per_sample else None
    want = lr.patchify_ref(srcs, case.scales, case.patch, case.lda, ps).float()
    got, guard = _run_patchify(L, dev, case, srcs, case.scales, ps, torch.float32)
    shapes = [tuple(s.shape) if s is not None else None for s in srcs]

    def decode(at):
        need = lr.patchify_source_of(at[0], at[1], case.chans, case.B, case.H, case.W, case.patch)
        hits = []
        for b in range(case.B):  # (the per-sample factor of the sample the value may have come from)
            sc = [case.scales[0] * (float(ps[b]) if ps is not None else 1.0), case.scales[1], case.scales[2]]
            hits += [h for h in lr.decode_tag(float(got[at]), shapes, offs, sc) if h[0] != 0 or h[1][0] == b]
        return f"(source, (b, c, y, x)) {sorted(set(hits))}, where (source, b, c, y, x) {need} belongs"

    _check_bits(f"patchify fp32 {case.name}", lr.f32_bits(got), lr.f32_bits(want), decode)  # (pad columns: +0 bit for bit)
    assert bool((lr.f32_bits(got[:, F:]) == 0).all()) and _is_sent(guard)
    # bf16: random values, power-of-two scales: the output is RNE of the exact product
    srcs, _ = lr.patchify_inputs(case, "normal")
    want = lr.rne_bf16_bits(lr.patchify_ref(srcs, case.scales, case.patch, case.lda, ps).float())
    got, guard = _run_patchify(L, dev, case, srcs, case.scales, ps, torch.bfloat16)
    _check_bits(f"patchify bf16 {case.name}", lr.bf16_bits(got), want)
    assert bool((lr.bf16_bits(got[:, F:]) == 0).all()) and _is_sent(guard)
    if not case.per_sample:
        return
    # the general per-sample factor: two roundings at most (scale times factor, then times the value; or value times scale, then
    # times the factor): 2u |value| in fp32, half a bf16 ulp (2^-9 relative) on top for a bf16 output
    ps = torch.tensor([0.7310586, 1.9, 0.0123][:case.B])
    scales = (0.3, 1.0, 2.0)
    ref = lr.patchify_ref(srcs, scales, case.patch, case.lda, ps)
    got, guard = _run_patchify(L, dev, case, srcs, scales, ps, torch.float32)
    _check_bound(f"patchify fp32 general factor {case.name}", got, ref, 2 * U * ref.abs(), use=f"patchify_scaled fp32 ({case.path})")
    assert _is_sent(guard)
    got, guard = _run_patchify(L, dev, case, srcs, scales, ps, torch.bfloat16)
    half_ulp = torch.ldexp(torch.ones_like(ref), torch.frexp(ref)[1] - 9)  # |ref| in [2^(e-1), 2^e): bf16 ulp 2^(e-8)
    _check_bound(f"patchify bf16 general factor {case.name}", got.float(), ref, half_ulp + 2 * U * ref.abs(),
                 use=f"patchify_scaled bf16 ({case.path})")
    assert _is_sent(guard)


# ================================================================================================================= un-patchify
# (beta times a tag must round: with factors like 2 or 0.75 the product of a tag is exact and the one-rounding bound goes unused)
ALPHA, BETA = torch.tensor([0.3, -1.0, 1.7]), torch.tensor([0.3, -1.1, 0.7])
COMBOS = ("none", "beta", "xt+alpha+beta", "xt+beta")


def _run_unpatchify(L, dev, case, tok_dev, ldt, combo, xt):
    B, C, H, W = case.B, case.C, case.H, case.W
    n = B * C * H * W
    out = _sent_f32(n + 64, dev)
    al, be = ALPHA[:B].to(dev), BETA[:B].to(dev)
    xt_view = None
    if combo.startswith("xt"):
        buf = torch.zeros(n + 4, dtype=torch.float32, device=dev)
        xt_view = buf[case.xt_misalign:case.xt_misalign + n]
        xt_view.copy_(xt.reshape(-1))
        assert (xt_view.data_ptr() % 16 != 0) == bool(case.xt_misalign)
    rc = L.swiftk_unpatchify_affine(tok_dev.data_ptr(), ldt, xt_view.data_ptr() if xt_view is not None else None,
                                    al.data_ptr() if combo == "xt+alpha+beta" else None,
                                    be.data_ptr() if combo != "none" else None, out.data_ptr(), B, C, H, W, case.patch[0],
                                    case.patch[1], _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = out.cpu()
    assert _is_sent(out[n:]), "wrote past the output"
    return out[:n].view(B, C, H, W)


@pytest.mark.parametrize("case", UNPATCHIFY_CASES, ids=lambda c: c.name)
def test_unpatchify_affine_places_every_element(L, dev, case):
    B, C, H, W = case.B, case.C, case.H, case.W
    p1, p2 = case.patch
    T, feat = (H // p1) * (W // p2), C * p1 * p2
    tok = lr.tagged((B, T, feat))
    xt = lr.normal((B, C, H, W), 41) * 1000.0  # (of the tags' magnitude, so that neither term hides the other)
    for wide in (0, case.wide):
        ldt = feat + case.ldt_extra + wide
        tok_dev = _nan_padded(tok.view(B * T, feat), ldt, dev)
        assert tok_dev.data_ptr() % 16 == 0

        def decode(at, got):
            v = float(got[at]) - 1
            where = tuple(int(c) for c in torch.unravel_index(torch.tensor(int(v)), (B, T, feat))) if 0 <= v < tok.numel() and v == int(v) else None
            return f"tok (b, token, feature) {where}, where {lr.unpatchify_source_of(at[0], at[1], at[2], at[3], W, case.patch)} belongs"

        for combo in COMBOS:
            ref, bound = lr.unpatchify_ref(tok, C, H, W, case.patch, xt if combo.startswith("xt") else None,
                                           ALPHA[:B] if combo == "xt+alpha+beta" else None, BETA[:B] if combo != "none" else None)
            got = _run_unpatchify(L, dev, case, tok_dev, ldt, combo, xt)
            name = f"unpatchify {case.name} ldt {ldt} {combo}"
            if combo == "none":
                _check_bits(name, lr.f32_bits(got), lr.f32_bits(ref.float()), lambda at: decode(at, got))
            else:
                _check_bound(name, got, ref, bound, use=f"unpatchify_affine {combo} ({case.path})")
            if case.path == "fast4" and wide == 0:
                # the same case through the generic kernel (an odd row stride sends it there): bit equal
                other = case._replace(ldt_extra=1, path="generic")
                assert lr.unpatchify_path(H, W, case.patch, feat + 1) == "generic"
                got2 = _run_unpatchify(L, dev, other, _nan_padded(tok.view(B * T, feat), feat + 1, dev), feat + 1, combo, xt)
                _check_bits(name + ": generic kernel against the 2 x 2 kernel", lr.f32_bits(got2), lr.f32_bits(got))


# ================================================================================================================= timestep embedding
T_VALUES = [1.5, 0.0, -0.37, 1.0, math.pi / 2, 0.37, 0.999]


@pytest.mark.parametrize("aux_dim", [0, 1, 3])
@pytest.mark.parametrize("weight", [1.0, 1000.0])
@pytest.mark.parametrize("B, d", [(1, 2), (5, 1056), (3, 98), (7, 1280), (2, 7)])
def test_timestep_embed_every_element(L, dev, B, d, weight, aux_dim):
    t = torch.tensor(T_VALUES[:B])
    freqs = lr.default_freqs(d)
    aux = lr.normal((B, aux_dim), 50 + aux_dim) if aux_dim else None
    aw, ab = (lr.normal((d, aux_dim), 51, 0.02), lr.normal((d,), 52, 0.02)) if aux_dim else (None, None)
    ref, bound = lr.timestep_embed_ref(t, weight, freqs, d, aux, aw, ab)
    out = _sent_f32(B * d + 16, dev)
    dv = [v.to(dev) if v is not None else None for v in (t, aux, freqs, aw, ab)]
    ptr = [v.data_ptr() if v is not None else None for v in dv]
    rc = L.swiftk_timestep_embed(ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], out.data_ptr(), B, d, max(aux_dim, 1), weight, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = out.cpu()
    assert _is_sent(out[B * d:])
    got, half = out[:B * d].view(B, d), d // 2
    name = f"timestep_embed B {B} d {d} w {weight} aux {aux_dim}"
    kind = "with aux" if aux_dim else "alone"
    _check_bound(name + " sine half (b, i)", got[:, :half], ref[:, :half], bound[:, :half], use=f"timestep_embed sine {kind}")
    _check_bound(name + " cosine half (b, i - d/2)", got[:, half:2 * half], ref[:, half:2 * half], bound[:, half:2 * half],
                 use=f"timestep_embed cosine {kind}")
    if d % 2:  # the header: [sin | cos | 0]
        _check_bound(name + " odd last column", got[:, 2 * half:], ref[:, 2 * half:], bound[:, 2 * half:])


# ================================================================================================================= small-batch linear
@pytest.mark.parametrize("case", LINEAR_CASES, ids=lambda c: c.name)
def test_linear_small_exact(L, dev, case):
    x, w, b, _ = lr.linear_operands(case)
    xd, wd = _nan_padded(x, case.ldx, dev), _nan_padded(w, case.ldw, dev)
    bd = b.to(dev) if b is not None else None
    out = _sent_f32((case.B + 1) * case.ldo, dev).view(case.B + 1, case.ldo)
    rc = L.swiftk_linear_small(xd.data_ptr(), case.ldx, wd.data_ptr(), case.ldw, bd.data_ptr() if bd is not None else None,
                               out.data_ptr(), case.ldo, case.B, case.N, case.K, case.act, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = out.cpu()
    assert _is_sent(out[case.B:]) and _is_sent(out[:case.B, case.N:]), "wrote outside [B, N]"
    got = out[:case.B, :case.N]
    z = lr.linear_small_ref(x, w, b)
    name = f"linear_small {case.name} ({case.path}) (b, n)"
    if case.act == 0:
        _check_bits(name, lr.f32_bits(got), lr.f32_bits(z.float()))
        return
    want = lr.silu64(z)
    allow, torch_fig = lr.silu_allowance(z)
    rel = (got.double() - want).abs() / want.abs().clamp_min(1e-300)
    print(f"[silu] {case.name}: torch CPU fp32 silu {torch_fig:.3e} relative, kernel {float(rel.max()):.3e}, allowance {allow:.3e}; "
          f"pre-activations in [{float(z.min()):.1f}, {float(z.max()):.1f}]")
    _check_bound(name + " SiLU", got, want, allow * want.abs(), use=f"linear_small SiLU ({case.path})")


def test_linear_small_refusals(L, dev):
    x, w, out = torch.zeros(2 * 64 + 4, device=dev), torch.zeros(8 * 68, device=dev), torch.zeros(2 * 8, device=dev)
    args = lambda xp, ldw: (xp, 64, w.data_ptr(), ldw, None, out.data_ptr(), 8, 2, 8, 64, 0, _stream())
    assert L.swiftk_linear_small(*args(x.data_ptr(), 64)) == 0
    assert L.swiftk_linear_small(*args(x[1:].data_ptr(), 64)) == lr.EALIGN  # x off its 16-byte boundary
    assert L.swiftk_linear_small(*args(x.data_ptr(), 66)) == lr.EALIGN      # ldw % 4
    torch.cuda.synchronize()


# ================================================================================================================= rollout update
def _rollout_operands(B, C, hw, zero_channel):
    x, y = lr.normal((B, C, hw), 60), lr.normal((B, C, hw), 61)
    m, s, t = lr.normal((C,), 62, 3.0), lr.normal((C,), 63).abs() + 0.5, lr.normal((C,), 64).abs() + 0.1
    if zero_channel is not None:
        m[zero_channel], s[zero_channel] = 0.0, 0.0
    return x, y, m, s, t


ROLLOUT_SHAPES = {"7-channels-one-with-s-0": (2, 7, 64, 3), "C1-hw4": (1, 1, 4, None), "past-the-grid-cap": (1, 3, 4 * 349528, None)}
ROLLOUT_CASES = [(res, ph, name) for name in ("7-channels-one-with-s-0", "C1-hw4") for res in (True, False) for ph in (True, False)] \
    + [(True, True, "past-the-grid-cap")]  # (the stride step needs one run)


@pytest.mark.parametrize("residual, with_phys, shape", ROLLOUT_CASES,
                         ids=[f"{'residual' if r else 'state'}-{'phys' if p else 'no-phys'}-{n}" for r, p, n in ROLLOUT_CASES])
def test_rollout_update_every_element(L, dev, residual, with_phys, shape):
    B, C, hw, zero_channel = ROLLOUT_SHAPES[shape]
    assert shape != "past-the-grid-cap" or lr.CAP < B * C * hw // 4 <= lr.CAP + 8192
    x, y, m, s, t = _rollout_operands(B, C, hw, zero_channel)
    n = B * C * hw
    xd, pd = _sent_f32(n + 16, dev), _sent_f32(n + 16, dev)
    xd[:n] = x.reshape(-1).to(dev)
    yd, md, sd, td = (v.to(dev) for v in (y, m, s, t))
    rc = L.swiftk_rollout_update(xd.data_ptr(), yd.data_ptr(), pd.data_ptr() if with_phys else None, md.data_ptr(), sd.data_ptr(),
                                 td.data_ptr() if residual else None, B, C, hw, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    xo, po = xd.cpu(), pd.cpu()
    assert _is_sent(xo[n:]) and _is_sent(po[n:] if with_phys else po)
    xo, po = xo[:n].view(B, C, hw), po[:n].view(B, C, hw)
    v = lambda a: a.view(1, C, 1)
    if not residual:  # bit equal to the reference's two roundings (no fused multiply-add) and xstd = y
        _check_bits("rollout state form xstd (b, c, i)", lr.f32_bits(xo), lr.f32_bits(y))
        if with_phys:
            _check_bits("rollout state form phys (b, c, i)", lr.f32_bits(po), lr.f32_bits(y * v(s) + v(m)))
        return
    phys, xstd, pbound = lr.rollout_ref(x, y, m, s, t)
    live = [c for c in range(C) if c != zero_channel]
    if with_phys:
        _check_bound("rollout phys (b, c, i)", po[:, live], phys[:, live], pbound[:, live], use="rollout_update phys")
        q, qbound = lr.rollout_xstd_from(po, m, s)  # against the kernel's own phys
        _check_bound("rollout xstd from the kernel's phys (b, c, i)", xo[:, live], q[:, live], qbound[:, live],
                     use="rollout_update xstd | phys")
    # loosely against the fp64 chain: the error of phys divided by s, plus the subtraction and the division
    loose = (pbound + 4 * U * (phys.abs() + v(m).double().abs())) / v(s).double().abs()
    _check_bound("rollout xstd against the fp64 chain (b, c, i)", xo[:, live], xstd[:, live], loose[:, live], use="rollout_update xstd chain")
    if zero_channel is not None:  # s == 0: xstd exactly +0, phys == y t bit for bit
        zc = zero_channel
        assert bool((lr.f32_bits(xo[:, zc]) == 0).all()), "xstd of the s == 0 channel is not +0"
        if with_phys:
            _check_bits("rollout phys of the s == 0 channel (b, i)", lr.f32_bits(po[:, zc]), lr.f32_bits(y[:, zc] * t[zc]))


def test_rollout_update_refusals(L, dev):
    buf = [torch.zeros(2 * 3 * 8 + 4, device=dev) for _ in range(3)]
    ch = [torch.ones(3, device=dev) for _ in range(3)]
    call = lambda xp, hw: L.swiftk_rollout_update(xp, buf[1].data_ptr(), buf[2].data_ptr(), ch[0].data_ptr(), ch[1].data_ptr(),
                                                  ch[2].data_ptr(), 2, 3, hw, _stream())
    assert call(buf[0].data_ptr(), 8) == 0
    assert call(buf[0].data_ptr(), 6) == lr.ESHAPE        # hw % 4
    assert call(buf[0][1:].data_ptr(), 8) == lr.EALIGN    # a pointer off its 16-byte boundary
    torch.cuda.synchronize()


# ================================================================================================================= axpby
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4 * lr.CAP + 7])
def test_axpby_every_element_and_in_place(L, dev, n):
    a, b = 0.3, -1.7
    x, y = lr.normal((n,), 70), lr.normal((n,), 71)
    ref, bound = lr.axpby_ref(a, x, b, y)

    def run(alias):
        xd, yd, od = _sent_f32(n + 16, dev), _sent_f32(n + 16, dev), _sent_f32(n + 16, dev)
        xd[:n], yd[:n] = x.to(dev), y.to(dev)
        o = {"none": od, "x": xd, "y": yd}[alias]
        rc = L.swiftk_axpby(o.data_ptr(), a, xd.data_ptr(), b, yd.data_ptr(), n, _stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        for name, buf in (("out", od), ("x", xd), ("y", yd)):
            assert _is_sent(buf[n:].cpu()), f"wrote past n in {name}"
        if alias != "none":
            assert _is_sent(od.cpu())
        return o[:n].cpu()

    got = run("none")
    _check_bound(f"axpby n {n} (i)", got, ref, bound, use="axpby")
    for alias in ("x", "y"):
        _check_bits(f"axpby n {n} with out = {alias} against out of place (i)", lr.f32_bits(run(alias)), lr.f32_bits(got))


def test_axpby_refusal(L, dev):
    x, y, o = (torch.zeros(12, device=dev) for _ in range(3))
    assert L.swiftk_axpby(o.data_ptr(), 1.0, x.data_ptr(), 1.0, y.data_ptr(), 8, _stream()) == 0
    assert L.swiftk_axpby(o.data_ptr(), 1.0, x[1:].data_ptr(), 1.0, y.data_ptr(), 8, _stream()) == lr.EALIGN
    assert L.swiftk_axpby(o[1:].data_ptr(), 1.0, x.data_ptr(), 1.0, y.data_ptr(), 8, _stream()) == lr.EALIGN
    torch.cuda.synchronize()


# ================================================================================================================= conversions
def _edge_name(i):
    return lr.CONVERSION_TABLE[i % len(lr.CONVERSION_TABLE)].name


def test_conversion_edges_through_cast_pad(L, dev):
    rows, cols, lds, ldd = 5, 37, 41, 48
    f, want = lr.edge_values(rows * cols)
    src = _nan_padded(f.view(rows, cols), lds, dev)
    dst = _sent_bf16((rows + 1) * ldd, dev).view(rows + 1, ldd)
    assert L.swiftk_cast_pad(src.data_ptr(), lds, dst.data_ptr(), ldd, rows, cols, 1, _stream()) == 0
    torch.cuda.synchronize()
    out = dst.cpu()
    assert _is_sent(out[rows:]) and bool((lr.bf16_bits(out[:rows, cols:]) == 0).all())
    got = lr.bf16_bits(out[:rows, :cols])
    _check_bits("cast_pad bf16 (r, c)", got, want.view(rows, cols), lambda at: _edge_name(at[0] * cols + at[1]))


@pytest.mark.parametrize("inter", [0, 35])
def test_conversion_edges_through_cast_pad_t(L, dev, inter):
    rows, cols, ldw, ldo, ldt = 70, 130, 133, 136, 72
    f, want = lr.edge_values(rows * cols)
    src = _nan_padded(f.view(rows, cols), ldw, dev)
    out = _sent_bf16((rows + 1) * ldo, dev).view(rows + 1, ldo)
    out_t = _sent_bf16((cols + 1) * ldt, dev).view(cols + 1, ldt)
    assert L.swiftk_cast_pad_t(src.data_ptr(), ldw, rows, cols, out.data_ptr(), ldo, out_t.data_ptr(), ldt, inter, _stream()) == 0
    torch.cuda.synchronize()
    o, ot = out.cpu(), out_t.cpu()
    assert _is_sent(o[rows:]) and _is_sent(ot[cols:])
    assert bool((lr.bf16_bits(o[:rows, cols:]) == 0).all()) and bool((lr.bf16_bits(ot[:cols, rows:]) == 0).all())
    rp = torch.arange(rows)
    r = (rp & 1) * inter + (rp >> 1) if inter else rp  # output row r' takes input row r
    w = want.view(rows, cols)[r]
    name = lambda at: _edge_name(int(r[at[0]]) * cols + at[1])
    _check_bits(f"cast_pad_t out interleave {inter} (r', c)", lr.bf16_bits(o[:rows, :cols]), w, name)
    _check_bits(f"cast_pad_t out_t interleave {inter} (c, r')", lr.bf16_bits(ot[:cols, :rows]), w.t(),
                lambda at: _edge_name(int(r[at[1]]) * cols + at[0]))


@pytest.mark.parametrize("case", [c for c in PATCHIFY_CASES if c.name in ("tiled-2x2-C11-chunks-straddle", "element-2x3")],
                         ids=lambda c: c.name)
def test_conversion_edges_through_patchify(L, dev, case):
    srcs, _ = lr.patchify_inputs(case, "edges")
    ones = (1.0, 1.0, 1.0)
    want = lr.rne_bf16_bits(lr.patchify_ref(srcs, ones, case.patch, case.lda).float())
    got, guard = _run_patchify(L, dev, case, srcs, ones, None, torch.bfloat16)
    ref32 = lr.patchify_ref(srcs, ones, case.patch, case.lda).float()
    _check_bits(f"patchify bf16 edges {case.name} (row, col)", lr.bf16_bits(got), want,
                lambda at: f"fp32 bits {int(lr.f32_bits(ref32)[at]):#010x}")
    assert _is_sent(guard)


# ================================================================================================================= column sums
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("rows, cols, pad_slab, pad_out, nslabs", [(1025, 1024, 4, 6, 1), (37, 19, 5, 3, 5), (37, 19, 0, 0, 1)],
                         ids=["past-the-grid-cap", "five-slabs-wide-strides", "one-slab-dense"])
def test_reduce_slabs_exact(L, dev, rows, cols, pad_slab, pad_out, nslabs, accumulate):
    ld_slab, ld_out = cols + pad_slab, cols + pad_out
    stride = rows * ld_slab + 8
    flat = torch.full((nslabs * stride,), float("nan"))
    for s in range(nslabs):
        blk = flat[s * stride:s * stride + rows * ld_slab].view(rows, ld_slab)
        blk[:, :cols] = lr.integers((rows, cols), 80 + s)
    pre = lr.integers((rows, cols), 90)
    out = _sent_f32((rows + 1) * ld_out, dev).view(rows + 1, ld_out)
    if accumulate:
        out[:rows, :cols] = pre.to(dev)
    fd = flat.to(dev)
    rc = L.swiftk_reduce_slabs(fd.data_ptr(), ld_slab, stride, nslabs, out.data_ptr(), ld_out, rows, cols, accumulate, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    o = out.cpu()
    assert _is_sent(o[rows:]) and (pad_out == 0 or _is_sent(o[:rows, cols:]))
    want = lr.reduce_slabs_ref(flat, ld_slab, stride, nslabs, rows, cols, pre if accumulate else None)
    _check_bits(f"reduce_slabs accumulate {accumulate} (r, c)", lr.f32_bits(o[:rows, :cols]), lr.f32_bits(want.float()))


@pytest.mark.parametrize("period", [1, 7, 8, 9, 201])
def test_embed_bwd_sums_exact(L, dev, period):
    cols, lds, ldd = 300, 304, 320
    for nsamp in (1, 8, 9, 17):
        rows = nsamp * period
        src = lr.integers((rows, cols), 100 + nsamp)
        bias0, pos0 = lr.integers((cols,), 101), lr.integers((period, cols), 102)
        want_b, want_p = lr.embed_bwd_sums_ref(src, cols, period)
        for copy in (True, False):
            sd = _nan_padded(src, lds, dev)
            bd, pd = _sent_f32(cols + 8, dev), _sent_f32(period * cols + 8, dev)
            bd[:cols], pd[:period * cols] = bias0.to(dev), pos0.reshape(-1).to(dev)
            dst = _sent_bf16((rows + 1) * ldd, dev).view(rows + 1, ldd)
            rc = L.swiftk_embed_bwd_sums(sd.data_ptr(), lds, bd.data_ptr(), pd.data_ptr(), dst.data_ptr() if copy else None, ldd, rows,
                                         cols, period, _stream())
            assert rc == 0, rc
            torch.cuda.synchronize()
            b, p, d = bd.cpu(), pd.cpu(), dst.cpu()
            assert _is_sent(b[cols:]) and _is_sent(p[period * cols:])
            name = f"embed_bwd_sums period {period} samples {nsamp} copy {copy}"
            _check_bits(name + " pos (t, c)", lr.f32_bits(p[:period * cols].view(period, cols)), lr.f32_bits((pos0.double() + want_p).float()))
            _check_bits(name + " bias (c)", lr.f32_bits(b[:cols]), lr.f32_bits((bias0.double() + want_b).float()))
            if copy:
                assert _is_sent(d[rows:])
                _check_bits(name + " bf16 copy (r, c)", lr.bf16_bits(d[:rows, :cols]), lr.rne_bf16_bits(src))
                assert bool((lr.bf16_bits(d[:rows, cols:]) == 0).all()), name + ": pad columns of the copy are not +0"
            else:
                assert _is_sent(d)


@pytest.mark.parametrize("period", [0, 7])
@pytest.mark.parametrize("rows", [1, 64, 65, 200])
def test_colsum_exact(L, dev, rows, period):
    cols, lds = 300, 304
    src = lr.integers((rows, cols), 110 + rows)
    nout = max(period, 1) * cols
    pre = lr.integers((nout,), 111)
    od = _sent_f32(nout + 8, dev)
    od[:nout] = pre.to(dev)
    sd = _nan_padded(src, lds, dev)
    assert L.swiftk_colsum(sd.data_ptr(), lds, od.data_ptr(), rows, cols, period, _stream()) == 0
    torch.cuda.synchronize()
    o = od.cpu()
    assert _is_sent(o[nout:])
    want = pre.double().view(-1, cols) + lr.colsum_ref(src, cols, period).view(-1, cols)
    _check_bits(f"colsum rows {rows} period {period} (t, c)", lr.f32_bits(o[:nout].view(-1, cols)), lr.f32_bits(want.float()))
