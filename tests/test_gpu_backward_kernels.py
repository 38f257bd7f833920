"""-m gpu: the training backward and loss kernels of swift_amd/csrc/train_kernels.hip, each called through the C ABI and scored per
element, per row or per vector against the fp64 closed forms of tests/backward_reference.py on exactly the arrays the kernel is
given (tests/test_backward_reference_cpu.py pins those to autograd of the oracle and checks the conditions the bounds rest on).
Every case prints the kernel's worst error beside its bound.

Bounds.  bf16 results: one bf16 rounding of an fp32 value -- SwiGLU per element within one bf16 ulp of the rounded fp64 value and
different from it on <= 1e-3 of the elements (torch's own fp32 evaluation: <= 2e-5); vectors and rows 2^-8 relative L2 (twice the
2^-9 of one rounding).  fp32 results: F32_TOL = 1e-5 per row / vector; SwiGLU per element 8 x the worst error of torch's fp32 CPU
evaluation of the same formulas on the same inputs, both relative to |silu(g) u|, |d u| and |d g s| plus 2^-102 -- below its normal
range fp32 holds nothing to relative precision and the device flushes there (silu(-100) u = -3.7e-42 u comes back as 0), so an
absolute error of 2^-126 weighs as one fp32 epsilon --;
hostile ModulatedNorm rows 4 x the error of the fp32 restatement of the same arithmetic on that row, unless the row meets F32_TOL
anyway.  Sums: 1e-5 x the sum of the absolute terms; loss values 1e-5 and dlogvar 1e-4 relative (the sums are well conditioned);
elementwise loss gradients and prep outputs 1e-6 x the size of the element's own operands.

Measured on MI355X (worst over the cases of each kernel; bound in brackets):
  swiglu bf16          <= 1 bf16 ulp everywhere [1]; mismatch shares out 9.7e-6 / 1.7e-5, dgate 2.5e-5 / 1.8e-5, dup 1.3e-5 / 1.3e-5 at
                       (301, 3413) / (385, 2816) [1e-3]; torch's fp32 evaluation at (301, 3413): 6.8e-6, 1.8e-5, 0
  swiglu fp32          out 2.16e-7, dgate 6.07e-7, dup 2.13e-7 of the element's scale; torch's fp32 evaluation on the CPU 2.16e-7, 6.07e-7,
                       2.07e-7 [8 x: 1.7e-6, 4.9e-6, 1.7e-6].  With the hardware exp (__expf rounds g log2 e once: 4e-8 |g|) the forward stood
                       at 1.25e-6 .. 1.27e-6 and missed the bound at (1, 8), where the planted gate -30 decides both figures (6.3e-7): the
                       fp32 instantiation now takes expf and an IEEE division, the bf16 one is unchanged
  qknorm_bwd bf16      worst vector 1.7e-3 .. 2.4e-3 [3.9e-3]; dscale increment 1.7e-8 .. 1.5e-6 of sum|term| [1e-5]
  qknorm_bwd fp32      worst vector 1.2e-7 .. 2.2e-7 [1e-5]; dscale increment 1.2e-8 .. 9.4e-8 [1e-5]
  modnorm_bwd bf16     worst row 1.9e-3 .. 2.5e-3 [3.9e-3] at 256 / 128 / forced 256 rows per block; column sums 5.8e-9 .. 2.4e-6 [1e-5]
  modnorm_bwd fp32     ordinary rows 1.4e-6 (one-kernel form), 1.5e-7 (two-kernel form) [1e-5]; the row whose first element is
                       1000 x the rest's spread 9.9e-5 in the one-kernel form against 1.0e-4 of the fp32 restatement [4 x], every other
                       planted row <= 1.3e-7; column sums <= 1.0e-6 [1e-5].  The two-kernel form took its mean without a shift: the row
                       300 +- 0.02 stood at 2.4e-5 .. 3.3e-5 (on its restatement) and put 8.7e-6 (dgamma) and 1.5e-5 (dmod) of sum|term| into
                       the column sums at (1536, 200) -- over the bound; it now shifts by the row's first element like the one-kernel
                       form: 6.7e-8 and 1.1e-7
  crps                 loss 1.6e-8 .. 1.5e-7 small, 1.6e-6 past the grid cap [1e-5]; gradient elements <= 8.4e-8 [1e-6]; exact case bit-equal
  trigflow prep / loss prep 2.0e-7 [1e-6]; loss 5.3e-8 small, 4.7e-6 past the cap, 2.9e-6 at (2, 69, 128, 256) [1e-5]; dF 2.2e-7 [1e-6];
                       dlogvar 1.7e-7 small, 1.7e-6 past the cap, 3.4e-6 at (2, 69, 128, 256) [1e-4] -- with one atomic per element (the
                       parent commit's kernel on the same inputs) 2.4e-4 past the cap and 4.2e-3 at (2, 69, 128, 256)
  edm prep / loss      prep 1.6e-7 [1e-6]; loss 1.4e-7 [1e-5]; dF 3.4e-7 [1e-6]
  ensemble_sums        <= 2.0e-7 for N = 2 .. 64 [5e-5]
  fused Adam / AdamW   p 2.3e-8, ema 1.6e-8, exp_avg 3.1e-7, exp_avg_sq 3.3e-7 against the torch optimiser [3e-6]; bit-equal reruns
On the parent commit test_trigflow_past_the_grid_cap, test_trigflow_loss_dlogvar_at_the_workload_sample_size and
test_qknorm_bwd_refuses_what_it_cannot_run (fp32 head_dim 88 returned 0, the first refusal tried) fail, as do
test_swiglu_fwd_bwd_per_element[fp32-1-8] and test_modnorm_bwd_fp32[1536-200-two] for the reasons above.
"""
import functools

import numpy as np
import pytest
import torch

import backward_reference as br
from conftest import rel_l2

pytestmark = pytest.mark.gpu

F32_TOL = 1e-5
BF16_VEC_TOL = 2.0 ** -8
BF = torch.bfloat16
F32 = torch.float32
EINVAL, ESHAPE, EALIGN = -1, -2, -3
TINY = 2.0 ** -102   # an absolute error of 2^-126 (what flushing a subnormal result costs) weighs as one fp32 epsilon, 2^-24


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def s():
    return torch.cuda.current_stream().cuda_stream


def L():
    from swift_amd import _lib
    return _lib.lib()


def code(dt):
    from swift_amd import _lib
    return _lib.BF16 if dt == BF else _lib.F32


def bits(t):
    """The raw words of a tensor (compares NaN-poisoned buffers and signed zeros bit for bit)."""
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def padded(v, ld, dt, dev):
    """[rows, ld] of NaN in ``dt`` on the device with v in its first columns."""
    out = torch.full((v.shape[0], ld), float("nan"), dtype=dt, device=dev)
    out[:, :v.shape[1]] = v.to(dev).to(dt)
    return out


def dt_name(dt):
    return "bf16" if dt == BF else "fp32"


# ------------------------------------------------------------------------------------------ SwiGLU

@pytest.mark.parametrize("M,mlp", [(1, 8), (301, 3413), (385, 2816)])
@pytest.mark.parametrize("dt", [BF, F32], ids=dt_name)
def test_swiglu_fwd_bwd_per_element(dev, dt, M, mlp):
    """swiftk_swiglu_fwd / swiftk_swiglu_bwd with all three row strides larger than the widths and NaN in the pad columns.
    (385, 2816) is 1,084,160 items: the grid-stride loop's second trip with a ragged end.  The last row starts with the planted
    gates -100, -30, -1.2784645 (where dgate's factor s + g s (1 - s) vanishes), 0, 30, 100."""
    h32, d32 = br.swiglu_inputs(M, mlp, 40 + M)
    hv, dv = h32.to(dt).float(), d32.to(dt).float()   # the values the kernel reads
    ldh, ldo, lddh = 2 * mlp + 16, mlp + 8, 2 * mlp + 24
    h, d = padded(hv, ldh, dt, dev), padded(dv, ldo, dt, dev)
    o, dh = (torch.full((M, ld), float("nan"), dtype=dt, device=dev) for ld in (ldo, lddh))
    o0, dh0, h0, d0 = o.clone(), dh.clone(), h.clone(), d.clone()
    assert L().swiftk_swiglu_fwd(h.data_ptr(), ldh, o.data_ptr(), ldo, M, mlp, code(dt), s()) == 0
    assert L().swiftk_swiglu_bwd(h.data_ptr(), ldh, d.data_ptr(), ldo, dh.data_ptr(), lddh, M, mlp, code(dt), s()) == 0
    torch.cuda.synchronize()
    assert same_bits(o[:, mlp:], o0[:, mlp:]) and same_bits(dh[:, 2 * mlp:], dh0[:, 2 * mlp:])   # pad columns as they were
    assert same_bits(h, h0) and same_bits(d, d0)
    got = {"out": o[:, :mlp].float().cpu(), "dgate": dh[:, 0:2 * mlp:2].float().cpu(), "dup": dh[:, 1:2 * mlp:2].float().cpu()}
    assert all(torch.isfinite(v).all() for v in got.values())
    rdg, rdu, sdg, sdu = br.swiglu_bwd(hv, dv)
    ref = {"out": br.swiglu_fwd(hv), "dgate": rdg, "dup": rdu}
    tag = f"swiglu {dt_name(dt)} ({M}, {mlp})"
    if dt == BF:
        for k in got:
            ulps, share = br.bf16_score(got[k], ref[k])
            print(f"{tag} {k}: worst {ulps:.2f} bf16 ulp from the rounded fp64 value (bound 1), mismatch share {share:.2e} (cap 1e-3)")
            assert ulps <= 1.0 and share <= 1e-3, (k, ulps, share)
        return
    t32g, t32u, _, _ = br.swiglu_bwd(hv, dv, F32)
    yard = {"out": br.swiglu_fwd(hv, F32), "dgate": t32g, "dup": t32u}
    scale = {"out": ref["out"].abs() + TINY, "dgate": sdg + TINY, "dup": sdu + TINY}
    for k in got:
        ek = float(((got[k].double() - ref[k]).abs() / scale[k]).max())
        ey = float(((yard[k].double() - ref[k]).abs() / scale[k]).max())
        print(f"{tag} {k}: worst element error {ek:.2e} of its scale; torch fp32 on the CPU {ey:.2e}, bound 8 x = {8 * ey:.2e}")
        assert ek <= 8 * ey, (k, ek, ey)


# ------------------------------------------------------------------------------------------ QK-norm backward

@functools.lru_cache(maxsize=1)
def _qk_case(M, heads, hd, dt, seed):
    qkvh, dq, rn, scale = br.qknorm_inputs(M, heads, hd, seed, dt)
    ref, dscale, ascale = br.qknorm_bwd(qkvh.float(), dq.float(), rn, scale, heads, hd)
    return qkvh, dq, rn, scale, ref, dscale, ascale


@pytest.mark.parametrize("M,heads,hd,dt,seed", br.qknorm_cases(),
                         ids=[f"{dt_name(c[3])}-{c[1]}x{c[2]}-M{c[0]}" for c in br.qknorm_cases()])
def test_qknorm_bwd_per_vector(dev, M, heads, hd, dt, seed):
    """swiftk_qknorm_bwd out of place (ldo = k_pad(3 heads head_dim), or 64 more where that pads nothing; pad columns NaN) and in
    place (the gradient buffer at stride ldo > ld; v columns and pad bit-identical afterwards), on the same inputs.  Every q / k vector
    against the fp64 closed form on the stored values; dscale starts nonzero and heads at or above ln 100 keep their bits."""
    from swift_amd import ops
    qkvh, dq, rn, scale, ref, dscale_ref, ascale = _qk_case(M, heads, hd, dt, seed)
    width = 3 * heads * hd
    ldo = ops.k_pad(dt, width)
    if ldo == width:
        ldo += 64
    tol = BF16_VEC_TOL if dt == BF else F32_TOL
    a, rn_d, sc_d = qkvh.to(dev), rn.to(dev), scale.to(dev)
    ds0 = (0.25 + 0.01 * torch.arange(heads, dtype=F32)).to(dev)
    refv = ref.view(M, heads, 3, hd)
    for form in ("out of place", "in place"):
        dscale = ds0.clone()
        if form == "in place":
            out = padded(dq, ldo, dt, dev)
            before = out.clone()
            rc = L().swiftk_qknorm_bwd(a.data_ptr(), out.data_ptr(), width, rn_d.data_ptr(), out.data_ptr(), ldo, sc_d.data_ptr(),
                                       dscale.data_ptr(), M, heads, hd, code(dt), s())
        else:
            g = dq.to(dev)
            out = torch.full((M, ldo), float("nan"), dtype=dt, device=dev)
            before = padded(dq, ldo, dt, dev)   # (what the v columns and the pad must hold afterwards)
            rc = L().swiftk_qknorm_bwd(a.data_ptr(), g.data_ptr(), width, rn_d.data_ptr(), out.data_ptr(), ldo, sc_d.data_ptr(),
                                       dscale.data_ptr(), M, heads, hd, code(dt), s())
        assert rc == 0
        torch.cuda.synchronize()
        assert same_bits(out[:, width:], before[:, width:])
        gv, bv = out[:, :width].reshape(M, heads, 3, hd), before[:, :width].reshape(M, heads, 3, hd)
        assert same_bits(gv[:, :, 2], bv[:, :, 2])                                          # v passes through bit for bit
        e = br.row_rel_l2(gv[:, :, :2].float().cpu(), refv[:, :, :2])
        assert torch.isfinite(gv[:, :, :2].float()).all()
        inc = dscale.cpu().double() - ds0.cpu().double()
        live = scale.double() < br.LN100
        es = ((inc - dscale_ref).abs() / ascale)[live]
        print(f"qknorm_bwd {dt_name(dt)} heads {heads} head_dim {hd} M {M} {form}: worst vector {float(e.max()):.2e} (bound {tol:.2e}), "
              f"dscale increment {float(es.max()):.2e} of sum|term| (bound 1e-5)")
        assert float(e.max()) <= tol
        assert float(es.max()) <= 1e-5
        assert same_bits(dscale[~live.to(dev)], ds0[~live.to(dev)]) and int((~live).sum()) >= 1   # clamped heads: unchanged


def test_qknorm_bwd_refuses_what_it_cannot_run(dev):
    """Shapes whose head vectors are not <= 16 whole 16-byte chunks, more heads than LDS accumulators and rows off the 16-byte
    boundary return the documented code and write nothing."""
    M = 4
    a = torch.zeros(M, 4096, dtype=F32, device=dev)
    rn = torch.ones(M, 3 * 65, device=dev)
    scale = torch.zeros(128, device=dev)
    out = torch.full((M, 4096), float("nan"), dtype=F32, device=dev)
    g = torch.ones(M, 4096, dtype=F32, device=dev)
    dscale = torch.full((128,), 7.0, device=dev)
    out0 = out.clone()

    def call(heads, hd, dt, ld=None, ldo=None, off=0):
        w = 3 * heads * hd
        return L().swiftk_qknorm_bwd(a.data_ptr(), g.data_ptr() + off, ld or w, rn.data_ptr(), out.data_ptr(), ldo or w, scale.data_ptr(),
                                     dscale.data_ptr(), M, heads, hd, code(dt), s())

    def untouched():
        torch.cuda.synchronize()
        return same_bits(out, out0) and bool((dscale == 7.0).all())

    assert call(2, 88, F32) == ESHAPE and untouched()             # 22 chunks of four floats
    assert call(2, 12, BF) == ESHAPE and untouched()              # one and a half chunks
    assert call(2, 136, BF) == ESHAPE and untouched()             # 17 chunks
    assert call(65, 8, BF) == ESHAPE and untouched()              # more heads than accumulators
    assert call(2, 64, BF, ld=384 + 4) == EALIGN and untouched()  # rows of qkvh / dqkvh 8 bytes off
    assert call(2, 64, BF, ldo=384 + 4) == EALIGN and untouched() # rows of dqkv 8 bytes off
    assert call(2, 64, F32, off=4) == EALIGN and untouched()      # base pointer
    assert call(2, 64, BF, ld=380) == ESHAPE and untouched()      # rows shorter than the vectors
    assert call(2, 64, F32) == 0                                  # (and the same buffers are fine for what it can run)
    torch.cuda.synchronize()
    assert torch.isfinite(out.view(-1)[:M * 384]).all() and same_bits(out.view(-1)[M * 384:], out0.view(-1)[M * 384:])   # (rows at stride 384)


# ------------------------------------------------------------------------------------------ ModulatedNorm backward

def _modnorm_run(dev, dt, d, rps, B, key16, seed, ws0, ldy=None):
    """One call on fresh buffers.  Returns dict of CPU results and the inputs' fp64 reference."""
    from swift_amd import ops
    M = B * rps
    y, g, gamma, beta, mod = br.modnorm_inputs(d, rps, B, seed, bf16=dt == BF, offset_row=dt == F32)
    ldy = ldy or d
    lddy = ops.k_pad(dt, d) if dt == BF else d + 8
    if lddy == d:
        lddy += 32
    yd = padded(y, ldy, dt, dev)
    gd, gam, bet = g.to(dev), gamma.to(dev), beta.to(dev)
    wide = br.rnd((B, 6 * d), seed + 10).to(dev)
    wide[:, 2 * d:4 * d] = mod.to(dev)
    msl = wide[:, 2 * d:4 * d]
    dy = torch.full((M, lddy), float("nan"), dtype=dt, device=dev)
    dgam0, dbet0 = br.rnd((d,), seed + 11).to(dev), br.rnd((d,), seed + 12).to(dev)
    dmod0 = br.rnd((B, 6 * d), seed + 13).to(dev)
    dgam, dbet, dmod = dgam0.clone(), dbet0.clone(), dmod0.clone()
    dsl = dmod[:, 2 * d:4 * d]
    ws = torch.zeros(2 * B * d, device=dev) if ws0 else torch.full((2 * M,), float("nan"), device=dev)
    fn = L().swiftk_modnorm_bwd_ws0 if ws0 else L().swiftk_modnorm_bwd
    L().swiftk_set_tuning(16, key16)
    try:
        rc = fn(yd.data_ptr(), ldy, gd.data_ptr(), dy.data_ptr(), lddy, gam.data_ptr(), bet.data_ptr(), msl.data_ptr(), msl.stride(0),
                dgam.data_ptr(), dbet.data_ptr(), dsl.data_ptr(), dsl.stride(0), ws.data_ptr(), M, d, rps, 1e-6, code(dt), s())
    finally:
        L().swiftk_set_tuning(16, 1)
    torch.cuda.synchronize()
    res = dict(rc=rc, dy=dy[:, :d].float().cpu(), dy_pad_ok=bool(torch.isnan(dy[:, d:].float()).all()) and same_bits(dy[:, d:], torch.full_like(dy[:, d:], float("nan"))),
               dgamma=dgam.cpu().double() - dgam0.cpu().double(), dbeta=dbet.cpu().double() - dbet0.cpu().double(),
               dmod=dsl.cpu().double() - dmod0[:, 2 * d:4 * d].cpu().double(),
               others_ok=same_bits(dmod[:, :2 * d], dmod0[:, :2 * d]) and same_bits(dmod[:, 4 * d:], dmod0[:, 4 * d:]),
               ws_zero=bool(ws0 and not ws.view(torch.int32).any()), y_ok=same_bits(yd, padded(y, ldy, dt, dev)))
    return res, (y, g, gamma, beta, mod)


def _modnorm_check(res, inputs, ref, dt, rps, one_pass, tag):
    y, g, gamma, beta, mod = inputs
    assert res["rc"] == 0
    assert res["dy_pad_ok"] and res["others_ok"] and res["y_ok"]
    assert torch.isfinite(res["dy"]).all()
    e = br.row_rel_l2(res["dy"], ref["dy"])
    assert float(e[4]) == 0.0                                      # the zero row of g: dy exactly zero
    H = br.MODNORM_HOSTILE
    benign = e[H:]
    if dt == BF:
        print(f"{tag}: dy worst row {float(e.max()):.2e} (planted rows {[f'{float(v):.1e}' for v in e[:H]]}; bound {BF16_VEC_TOL:.2e})")
        assert float(e.max()) <= BF16_VEC_TOL
    else:
        y32 = br.modnorm_bwd_fp32(y[:H], g[:H], gamma, mod[:1], H, one_pass=one_pass)
        ey = br.row_rel_l2(y32, ref["dy"][:H])
        print(f"{tag}: dy worst ordinary row {float(benign.max()):.2e} (bound {F32_TOL:.0e}); planted rows kernel "
              f"{[f'{float(v):.1e}' for v in e[:H]]}, fp32 restatement {[f'{float(v):.1e}' for v in ey]} (bound 4 x, or {F32_TOL:.0e})")
        assert float(benign.max()) <= F32_TOL
        for r in range(H):
            assert float(e[r]) <= max(F32_TOL, 4 * float(ey[r])), (r, float(e[r]), float(ey[r]))
    worst = {}
    for k, a in (("dgamma", "agamma"), ("dbeta", "abeta"), ("dmod", "amod")):
        worst[k] = float(((res[k] - ref[k]).abs() / ref[a]).max())
    print(f"{tag}: column sums, worst error / sum|term|: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) + " (bound 1e-5)")
    assert max(worst.values()) <= 1e-5, worst


@pytest.mark.parametrize("d,rps,B,key16,rows", [(96, 256, 256, 1, 256), (96, 128, 256, 1, 128), (1056, 1280, 3, 4, 256)],
                         ids=["natural-256", "natural-128", "key16-4"])
def test_modnorm_bwd_bf16_rows_per_block(dev, d, rps, B, key16, rows):
    """The one-kernel form at the block sizes no other test reaches: M / 256 >= 256 picks 256 rows per block by itself (M = 65,536),
    M / 128 >= 256 with rows_per_sample = 128 picks 128, tuning key 16 = 4 forces 256.  Both entry points; accumulators start
    nonzero; planted rows: constant, first element 1000 x the spread of the rest, an outlier elsewhere, a zero row of g."""
    M = B * rps
    if key16 == 1:  # what the dispatcher computes (train_kernels.hip: modnorm_bwd_impl)
        rpbf = 256
        while rpbf > 64 and (rps % rpbf or M // rpbf < 256):
            rpbf >>= 1
        assert rpbf == rows
    ref = None
    first = None
    for ws0 in (False, True):
        res, inputs = _modnorm_run(dev, BF, d, rps, B, key16, 700 + d + rps, ws0)
        if ref is None:
            ref = br.modnorm_bwd(*inputs, rps)
        _modnorm_check(res, inputs, ref, BF, rps, True, f"modnorm_bwd{'_ws0' if ws0 else ''} bf16 d {d} rows/sample {rps} x {B}, {rows} rows per block")
        if ws0:
            assert res["ws_zero"]
            assert torch.equal(res["dy"], first["dy"])
        first = res


@pytest.mark.parametrize("d,rps,form", [(1056, 1088, "one"), (1056, 1088, "ws0"), (1056, 1088, "two"), (1536, 200, "two")])
def test_modnorm_bwd_fp32(dev, d, rps, form):
    """fp32 activations with ldy > d: the one-kernel form (both entry points) and the two-kernel form (tuning key 16 = 0, and
    rows_per_sample < d).  Planted rows as above plus a common offset of 300 with spread 0.02."""
    B = 2
    key16 = 0 if (form == "two" and rps >= d) else 1
    res, inputs = _modnorm_run(dev, F32, d, rps, B, key16, 800 + d + rps, form == "ws0", ldy=d + 8)
    ref = br.modnorm_bwd(*inputs, rps)
    _modnorm_check(res, inputs, ref, F32, rps, form != "two", f"modnorm_bwd fp32 d {d} rows/sample {rps}, {form}-kernel form")
    if form == "ws0":
        assert res["ws_zero"]


def test_modnorm_bwd_ws0_fp32_refuses_the_two_kernel_shape(dev):
    res, _ = _modnorm_run(dev, F32, 1536, 200, 2, 1, 801, True, ldy=1544)
    assert res["rc"] == ESHAPE and res["ws_zero"] and res["others_ok"]
    assert float(res["dgamma"].abs().max()) == 0.0 and float(res["dmod"].abs().max()) == 0.0 and bool(torch.isnan(res["dy"]).all())


# ------------------------------------------------------------------------------------------ losses

def _dev_weights(c, dev):
    return c["w_var"].to(dev), c["w_lat"].to(dev)


def _elem_err(got, ref, scale):
    return float(((got.cpu().double() - ref).abs() / scale).max())


def _crps_inputs(m, shape, seed):
    B, C, H, W = shape
    preds, target = br.rnd((m, *shape), seed), br.rnd(shape, seed + 1)
    preds[0, 0, 0, 0, 0] = target[0, 0, 0, 0]                       # a member equal to the target
    preds[1, B - 1, 2, 3, 4] = preds[0, B - 1, 2, 3, 4]             # two equal members
    w_var, w_lat = br.loss_weights(C, H, seed + 2)
    return preds, target, w_var, w_lat


def _crps_check(dev, m, shape, alpha, seed, with_grad=True):
    B, C, H, W = shape
    preds, target, w_var, w_lat = _crps_inputs(m, shape, seed)
    pd, td, wv, wl = (v.to(dev) for v in (preds, target, w_var, w_lat))
    loss0 = 0.125
    loss = torch.full((1,), loss0, device=dev)
    dp = torch.full_like(pd, float("nan")) if with_grad else None
    rc = L().swiftk_crps_loss(pd.data_ptr(), td.data_ptr(), wv.data_ptr(), wl.data_ptr(), loss.data_ptr(), dp.data_ptr() if with_grad else None,
                              m, B, C, H, W, alpha, 0.25, s())
    assert rc == 0
    torch.cuda.synchronize()
    rl, rdp, scale = br.crps(preds, target, w_var, w_lat, alpha, 0.25)
    el = abs((float(loss) - loss0) - float(rl)) / abs(float(rl))
    eg = _elem_err(dp, rdp, scale) if with_grad else 0.0
    print(f"crps m {m} alpha {alpha} {shape}{'' if with_grad else ' (no dpreds)'}: loss {el:.2e} (bound 1e-5), worst gradient element "
          f"{eg:.2e} of its scale (bound 1e-6)")
    assert el <= 1e-5 and eg <= 1e-6


@pytest.mark.parametrize("alpha", [0.95, 1.0])
@pytest.mark.parametrize("m", [2, 3, 8, 12])
def test_crps_small(dev, m, alpha):
    _crps_check(dev, m, br.SHAPE_SMALL, alpha, 900 + m)
    if m == 3:
        _crps_check(dev, m, br.SHAPE_SMALL, alpha, 900 + m, with_grad=False)


def test_crps_past_the_grid_cap(dev):
    _crps_check(dev, 3, br.SHAPE_PAST_CAP, 0.95, 950)


def test_crps_refuses_one_member(dev):
    B, C, H, W = br.SHAPE_SMALL
    pd, td = torch.zeros(1, B, C, H, W, device=dev), torch.zeros(B, C, H, W, device=dev)
    wv, wl = torch.ones(C, device=dev), torch.ones(H, device=dev)
    loss, dp = torch.full((1,), 3.0, device=dev), torch.full_like(pd, float("nan"))
    assert L().swiftk_crps_loss(pd.data_ptr(), td.data_ptr(), wv.data_ptr(), wl.data_ptr(), loss.data_ptr(), dp.data_ptr(), 1, B, C, H, W,
                                1.0, 1.0, s()) == EINVAL
    torch.cuda.synchronize()
    assert float(loss) == 3.0 and bool(torch.isnan(dp).all())


def test_crps_exact(dev):
    """m = 2, alpha = 1, n = 2^21, values in {-1, 0, 1}, unit weights: every partial sum in any order is exact in fp32
    (tests/test_backward_reference_cpu.py), so the loss and every gradient element equal the fp64 result bit for bit."""
    preds, target, w_var, w_lat = br.exact_crps_inputs()
    m, B, C, H, W = preds.shape
    pd, td, wv, wl = (v.to(dev) for v in (preds, target, w_var, w_lat))
    loss, dp = torch.zeros(1, device=dev), torch.full_like(pd, float("nan"))
    assert L().swiftk_crps_loss(pd.data_ptr(), td.data_ptr(), wv.data_ptr(), wl.data_ptr(), loss.data_ptr(), dp.data_ptr(), m, B, C, H, W,
                                1.0, 1.0, s()) == 0
    torch.cuda.synchronize()
    rl, rdp, _ = br.crps(preds, target, w_var, w_lat, 1.0)
    print(f"exact crps: loss {float(loss)!r} vs fp64 {float(rl)!r}; gradient elements that differ: {int((dp.cpu().double() != rdp).sum())}")
    assert float(loss) == float(rl)
    assert torch.equal(dp.cpu().double(), rdp)


def _trigflow_check(dev, shape, seed, prep=True, variants=("all",)):
    B, C, H, W = shape
    c = br.trigflow_inputs(shape, seed)
    wv, wl = _dev_weights(c, dev)
    if prep:
        xt, vt = (torch.full(shape, float("nan"), device=dev) for _ in range(2))
        assert L().swiftk_trigflow_prep(c["x"].to(dev).data_ptr(), c["z"].to(dev).data_ptr(), c["t"].to(dev).data_ptr(), xt.data_ptr(), vt.data_ptr(),
                                        br.SD, B, C * H * W, s()) == 0
        rxt, rvt = br.trigflow_prep(c["x"], c["z"], c["t"], br.SD)
        x, z = c["x"].double(), c["z"].double() * br.SD
        cs, sn = torch.cos(c["t"].double()).view(B, 1, 1, 1).abs(), torch.sin(c["t"].double()).view(B, 1, 1, 1).abs()
        e1 = _elem_err(xt, rxt, (cs * x.abs() + sn * z.abs()) / br.SD)
        e2 = _elem_err(vt, rvt, cs * z.abs() + sn * x.abs())
        print(f"trigflow_prep {shape}: worst element x_t/sd {e1:.2e}, v_t {e2:.2e} of |cos t x| + |sin t sd z| (bound 1e-6)")
        assert e1 <= 1e-6 and e2 <= 1e-6
    Fd, vd, lvd = c["F"].to(dev), c["vt"].to(dev), c["lv"].to(dev)
    out = {}
    for var in variants:
        use_lv, use_dF, use_dlv = var != "no logvar", var != "no dF", var != "no dlogvar"
        loss0 = 0.125
        loss = torch.full((1,), loss0, device=dev)
        dF = torch.full(shape, float("nan"), device=dev)
        dlv0 = torch.linspace(0.5, -0.25, B)
        dlv = dlv0.to(dev)
        rc = L().swiftk_trigflow_loss(Fd.data_ptr(), vd.data_ptr(), lvd.data_ptr() if use_lv else None, wv.data_ptr(), wl.data_ptr(), loss.data_ptr(),
                                      dF.data_ptr() if use_dF else None, dlv.data_ptr() if use_dlv else None, br.SD, B, C, H, W, 0.25, s())
        assert rc == 0
        torch.cuda.synchronize()
        r = br.trigflow_loss(c["F"], c["vt"], c["lv"] if use_lv else None, c["w_var"], c["w_lat"], br.SD, 0.25)
        el = abs((float(loss) - loss0) - float(r["loss"])) / abs(float(r["loss"]))
        eF = _elem_err(dF, r["dF"], r["wr"]) if use_dF else 0.0
        if use_dlv:
            ed = float(((dlv.cpu().double() - dlv0.double() - r["dlogvar"]).abs() / r["dlogvar"].abs()).max())
        else:
            ed = 0.0
            assert torch.equal(dlv.cpu(), dlv0)
        if not use_dF:
            assert bool(torch.isnan(dF).all())
        print(f"trigflow_loss {shape} [{var}]: loss {el:.2e} (bound 1e-5), worst dF element {eF:.2e} of its scale (bound 1e-6), "
              f"dlogvar {ed:.2e} (bound 1e-4)")
        out[var] = (el, eF, ed)
    for var, (el, eF, ed) in out.items():
        assert el <= 1e-5 and eF <= 1e-6 and ed <= 1e-4, (var, el, eF, ed)


def test_trigflow_small_with_each_optional_pointer_null(dev):
    _trigflow_check(dev, br.SHAPE_SMALL, 20, variants=("all", "no logvar", "no dF", "no dlogvar"))


def test_trigflow_past_the_grid_cap(dev):
    _trigflow_check(dev, br.SHAPE_PAST_CAP, 20)


def test_trigflow_loss_dlogvar_at_the_workload_sample_size(dev):
    """(2, 69, 128, 256): 2,260,992 terms per sample behind each dlogvar.  One atomic per element (the parent commit's kernel,
    measured on these inputs) left 4.2e-3 here against the bound of 1e-4; summed in the lane and the wave first: 3.4e-6."""
    _trigflow_check(dev, br.SHAPE_WORKLOAD, 20, prep=False)


def _edm_check(dev, shape, seed, with_grad=True):
    B, C, H, W = shape
    x, z, Fo = br.rnd(shape, seed), br.rnd(shape, seed + 1), br.rnd(shape, seed + 2)
    sigma = torch.tensor([0.01, 0.7, 40.0, 2.0])[:B]
    w_var, w_lat = br.loss_weights(C, H, seed + 3)
    xd, zd, Fd, sg, wv, wl = (v.to(dev) for v in (x, z, Fo, sigma, w_var, w_lat))
    net_in = torch.full(shape, float("nan"), device=dev)
    assert L().swiftk_edm_prep(xd.data_ptr(), zd.data_ptr(), sg.data_ptr(), net_in.data_ptr(), br.SD, B, C * H * W, s()) == 0
    sg4 = sigma.double().view(B, 1, 1, 1)
    ep = _elem_err(net_in, br.edm_prep(x, z, sigma, br.SD), (x.double().abs() + sg4 * z.double().abs()) / torch.sqrt(sg4 * sg4 + br.SD ** 2))
    loss0 = 0.125
    loss = torch.full((1,), loss0, device=dev)
    dF = torch.full(shape, float("nan"), device=dev)
    assert L().swiftk_edm_loss(Fd.data_ptr(), xd.data_ptr(), zd.data_ptr(), sg.data_ptr(), wv.data_ptr(), wl.data_ptr(), loss.data_ptr(),
                               dF.data_ptr() if with_grad else None, br.SD, B, C, H, W, 0.25, s()) == 0
    torch.cuda.synchronize()
    rl, rdF, scale = br.edm_loss(Fo, x, z, sigma, w_var, w_lat, br.SD, 0.25)
    el = abs((float(loss) - loss0) - float(rl)) / abs(float(rl))
    eF = _elem_err(dF, rdF, scale) if with_grad else 0.0
    print(f"edm {shape}{'' if with_grad else ' (no dF)'}: prep worst element {ep:.2e} (bound 1e-6), loss {el:.2e} (bound 1e-5), worst dF element "
          f"{eF:.2e} of its scale (bound 1e-6)")
    assert ep <= 1e-6 and el <= 1e-5 and eF <= 1e-6
    if not with_grad:
        assert bool(torch.isnan(dF).all())


def test_edm_small(dev):
    _edm_check(dev, br.SHAPE_SMALL, 30)
    _edm_check(dev, br.SHAPE_SMALL, 30, with_grad=False)


def test_edm_past_the_grid_cap(dev):
    _edm_check(dev, br.SHAPE_PAST_CAP, 30)


# ------------------------------------------------------------------------------------------ ensemble sums

@pytest.mark.parametrize("N", [2, 8, 9, 16, 17, 64])
def test_ensemble_sums(dev, N):
    """Both ends of each of the three instantiations (<= 8, <= 16, <= 64 members in registers)."""
    from oracle import metrics as omet
    B, V, H, W = 2, 3, 7, 11
    pred, y = br.rnd((B, N, V, H, W), 60 + N), br.rnd((B, V, H, W), 61)
    w = omet._w(np.linspace(-80, 80, H), y)
    out = torch.zeros(B * V * 4, device=dev)
    pd, yd, wd = pred.to(dev), y.to(dev), w.to(dev)   # (named: a temporary's block returns to the allocator once data_ptr() has been taken)
    assert L().swiftk_ensemble_sums(pd.data_ptr(), yd.data_ptr(), wd.data_ptr(), out.data_ptr(), B, N, V, H, W, s()) == 0
    torch.cuda.synchronize()
    ref = br.ensemble_sums(pred, y, w)
    e = ((out.cpu().double().view(B, V, 4) - ref).abs() / ref.abs()).amax((0, 1))
    print(f"ensemble_sums N {N}: worst relative error of (mean error^2, skill, spread, variance) sums {[f'{float(v):.1e}' for v in e]} (bound 5e-5)")
    assert float(e.max()) <= 5e-5


def test_ensemble_sums_refuses_65_members(dev):
    B, V, H, W = 1, 1, 7, 11
    pred, y, w = torch.zeros(B, 65, V, H, W, device=dev), torch.zeros(B, V, H, W, device=dev), torch.ones(H, device=dev)
    out = torch.full((4,), 5.0, device=dev)
    assert L().swiftk_ensemble_sums(pred.data_ptr(), y.data_ptr(), w.data_ptr(), out.data_ptr(), B, 65, V, H, W, s()) == ESHAPE
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())


# ------------------------------------------------------------------------------------------ fused Adam / AdamW + EMA

@pytest.mark.parametrize("kind,with_ema", [("adamw", True), ("adam", True), ("adamw", False)], ids=["adamw", "adam-l2", "adamw-no-ema"])
def test_fused_adam_multi_chunk_step_vs_torch_without_host_sync(dev, kind, with_ema):
    """FusedAdamEMA on 363 + 1 + 267 + 1 chunks in two parameter groups (different lr and weight decay) against the torch optimiser
    and lerp on copies, as tests/test_gpu_mars.py does for MARS: two steps (ema_beta 0.3, then 0.9: both sides of torch's lerp), NaN
    and +-inf planted in a late chunk, in a chunk's last element and in the ragged tail; the gradient buffer ends up sanitised, the
    step runs under set_sync_debug_mode("error"), and a second run from equal state is bit-equal."""
    from swift_amd.training.fused_optim import FusedAdamEMA
    from test_gpu_mars import TOL
    cls = torch.optim.AdamW if kind == "adamw" else torch.optim.Adam
    shapes = [(5632, 1056), (1056,), (3413, 1279), (33, 7)]
    gen = torch.Generator(device=dev).manual_seed(6)
    rnd = lambda sh, std: torch.randn(sh, generator=gen, device=dev) * std
    P = [torch.nn.Parameter(rnd(sh, 0.05)) for sh in shapes]
    E = [p.detach().clone() + 0.01 for p in P] if with_ema else None
    Pr = [torch.nn.Parameter(p.detach().clone()) for p in P]
    Er = [e.clone() for e in E] if with_ema else None
    groups = lambda ps: [dict(params=ps[:2], lr=2e-3, weight_decay=0.05), dict(params=ps[2:], lr=7e-4, weight_decay=0.2)]
    kw = dict(betas=(0.9, 0.95), eps=1e-8)
    opt, ref = cls(groups(P), **kw), cls(groups(Pr), **kw)
    flat = torch.zeros(sum(p.numel() for p in P), device=dev)
    o = 0
    for p in P:
        p.grad = flat[o:o + p.numel()].view_as(p)
        o += p.numel()
    fused = FusedAdamEMA(opt, P, E, flat)
    assert fused.n_chunks == 363 + 1 + 267 + 1 and fused.decoupled == (kind == "adamw")
    ema_beta = (0.3, 0.9)
    state = lambda: (flat, fused.m, fused.v, *[p.detach() for p in P], *(E or []))
    for step, std in enumerate((1e-4, 1e-2)):
        G = [rnd(sh, std) for sh in shapes]
        G[0].view(-1)[16384 * 200 + 5] = float("nan")       # a late chunk
        G[0].view(-1)[16384 * 300 - 1] = float("inf")       # a chunk's last element
        G[2].view(-1)[-2] = float("-inf")                   # the ragged tail
        G[1][7] = float("nan")
        G[3].view(-1)[4] = float("inf")
        for p, gk in zip(P, G):
            p.grad.copy_(gk)
        Gs = [torch.nan_to_num(gk, nan=0, posinf=1e5, neginf=-1e5) for gk in G]
        keep = [t.clone() for t in state()]
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            fused.step(ema_beta[step])
        finally:
            torch.cuda.set_sync_debug_mode("default")
        first = [t.clone() for t in state()]
        with torch.no_grad():
            for t, k in zip(state(), keep):
                t.copy_(k)
        fused.step_t -= 1
        fused.step(ema_beta[step])
        for a, b in zip(first, state()):
            assert torch.equal(a, b)
        assert torch.equal(flat, torch.cat([gs.flatten() for gs in Gs]))   # sanitised in place, bit for bit
        for p, gs in zip(Pr, Gs):
            p.grad = gs.clone()
        ref.step()
        if with_ema:
            with torch.no_grad():
                for e, p in zip(Er, Pr):
                    e.copy_(p.detach().lerp(e, ema_beta[step]))
        for i, (p, pr) in enumerate(zip(P, Pr)):
            errs = {"p": rel_l2(p.detach(), pr.detach()), "exp_avg": rel_l2(opt.state[p]["exp_avg"], ref.state[pr]["exp_avg"]),
                    "exp_avg_sq": rel_l2(opt.state[p]["exp_avg_sq"], ref.state[pr]["exp_avg_sq"])}
            if with_ema:
                errs["ema"] = rel_l2(E[i], Er[i])
            print(f"fused {kind} step {step + 1} {shapes[i]}: " + ", ".join(f"{a} {b:.2e}" for a, b in errs.items()) + f" (bound {TOL:.0e})")
            assert max(errs.values()) < TOL, (step, shapes[i], errs)
        assert all(p._version > 0 for p in P)
    assert float(opt.state[P[0]]["step"]) == 2.0
