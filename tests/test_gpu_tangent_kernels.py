"""-m gpu: the tangent-pass norm kernels and the training / loss glue entries, each called through the C ABI and compared with the
fp64 closed forms of tests/tangent_reference.py on the same inputs (tests/test_tangent_reference_cpu.py pins those to
torch.func.jvp / autograd of the oracle and shows that every term of the norm tangent is >= 2e-2 of the whole on these inputs).

Tolerances: F32_TOL = 1e-5 relative L2 for fp32 results (one or two fp32 operations per element); a pair result's floor is its
8-bit low part (6.5e-6), so 1e-5 for pair values and 1.5e-5 for the tangent increment; hostile rows are scored one by one against
4 x the error of the fp32 restatement of the same arithmetic on the same row (computed here, printed beside the kernel's).
swiftk_qknorm_jvp and swiftk_swiglu_jvp standing alone: per vector BF16_VEC_TOL = 2^-8 / F32_TOL, per element the bounds of
test_swiglu_fwd_bwd_per_element (tests/test_gpu_backward_kernels.py); figures in the tests' docstrings.
"""
import math

import pytest
import torch

import tangent_reference as tr
from conftest import rel_l2

pytestmark = pytest.mark.gpu

F32_TOL = 1e-5
BF = torch.bfloat16
EINVAL, ESHAPE, EALIGN = -1, -2, -3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def rnd(shape, seed, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * std


def s():
    return torch.cuda.current_stream().cuda_stream


def nan_like(shape, dev, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def bits(t):
    """The raw words of a tensor (compares NaN-poisoned buffers and signed zeros bit for bit)."""
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else (torch.int32 if t.element_size() == 4 else torch.uint8))


# ------------------------------------------------------------------------------------------ ModulatedNorm tangent, pair form

class _PairCase:
    """Device inputs of one swiftk_modnorm_jvp_pair case: y / dy bf16 [M, ldy], the (hi, lo) pairs of x and dx from
    swiftk_split_pair with 7.0 in hi's pad columns, mod / dmod as the [2d : 4d] column slice of [B, 6d] tensors."""

    def __init__(self, dev, d, rps, B, seed, ldy=None):
        from swift_amd import ops
        self.d, self.rps, self.B, self.M, self.dev = d, rps, B, B * rps, dev
        self.c = c = tr.make_norm_case(d, rps, B, seed)
        self.ld = ops.k_pad(BF, d)
        self.ldy = ldy or d
        self.y, self.dy = (torch.zeros(self.M, self.ldy, dtype=BF, device=dev) for _ in range(2))
        self.y[:, :d], self.dy[:, :d] = c["y"].to(dev).to(BF), c["dy"].to(dev).to(BF)
        self.hx, self.lx = ops.split_pair(c["x"].to(dev), self.ld, 8)
        self.hdx, self.ldx = ops.split_pair(c["dx"].to(dev), self.ld, 8)
        self.hx[:, d:] = 7.0
        self.hdx[:, d:] = 7.0
        self.gamma, self.beta = c["gamma"].to(dev), c["beta"].to(dev)
        wide, dwide = rnd((B, 6 * d), seed + 1).to(dev), rnd((B, 6 * d), seed + 2).to(dev)
        wide[:, 2 * d: 4 * d], dwide[:, 2 * d: 4 * d] = c["mod"].to(dev), c["dmod"].to(dev)
        self.msl, self.dsl = wide[:, 2 * d: 4 * d], dwide[:, 2 * d: 4 * d]
        # the reference starts from what the pairs actually hold
        self.x_in, self.dx_in = ops.pair_value(self.hx, self.lx, d).cpu(), ops.pair_value(self.hdx, self.ldx, d).cpu()
        self.ref_x, self.ref_dx = tr.modnorm_tangent(c["y"], c["dy"], self.x_in, self.dx_in, c["gamma"], c["beta"], c["mod"], c["dmod"], rps)

    def run(self, inplace, key17):
        """One call on fresh copies; returns (hi_x, lo_x, hi_dx, lo_dx, hi_x_in, hi_dx_in) -- the last two None when in place."""
        from swift_amd import _lib
        L = _lib.lib()
        d, ld, M = self.d, self.ld, self.M
        hx_in, hdx_in, lx, ldx = self.hx.clone(), self.hdx.clone(), self.lx.clone(), self.ldx.clone()
        if inplace:
            hx, hdx = hx_in, hdx_in
        else:
            hx, hdx = (torch.full((M, ld), 7.0, dtype=BF, device=self.dev) for _ in range(2))
            hx[:, :d] = float("nan")
            hdx[:, :d] = float("nan")
        L.swiftk_set_tuning(17, key17)
        try:
            rc = L.swiftk_modnorm_jvp_pair(self.y.data_ptr(), self.dy.data_ptr(), self.ldy, hx_in.data_ptr(), hdx_in.data_ptr(), hx.data_ptr(),
                                           hdx.data_ptr(), ld, lx.data_ptr(), ldx.data_ptr(), self.gamma.data_ptr(), self.beta.data_ptr(),
                                           self.msl.data_ptr(), self.dsl.data_ptr(), self.msl.stride(0), M, d, self.rps, 1e-6, s())
        finally:
            L.swiftk_set_tuning(17, 1)
        assert rc == 0
        torch.cuda.synchronize()
        return hx, lx, hdx, ldx, (None if inplace else hx_in), (None if inplace else hdx_in)

    def row_yardstick(self, one_pass, quantise=True):
        """Per hostile row (err_x, err_dx) of the fp32 restatement of the kernel's arithmetic, stored as the kernel stores."""
        c, n = self.c, tr.HOSTILE_ROWS
        x32, dx32 = tr.modnorm_tangent_fp32(c["y"][:n], c["dy"][:n], self.x_in[:n], self.dx_in[:n], c["gamma"], c["beta"], c["mod"][:1],
                                            c["dmod"][:1], n, one_pass=one_pass)
        if quantise:
            x32, dx32 = tr.pair_quantise(x32), tr.pair_quantise(dx32)
        return [(tr.row_err(x32[r], self.ref_x[r]), tr.row_err(dx32[r], self.ref_dx[r])) for r in range(n)]


def _check_pair_result(case, out, one_pass, tag):
    from swift_amd import ops
    d = case.d
    hx, lx, hdx, ldx, hx_in, hdx_in = out
    got_x, got_dx = ops.pair_value(hx, lx, d).cpu(), ops.pair_value(hdx, ldx, d).cpu()
    assert torch.isfinite(got_x).all() and torch.isfinite(got_dx).all()
    b = tr.benign
    ex, edx = rel_l2(b(got_x), b(case.ref_x)), rel_l2(b(got_dx), b(case.ref_dx))
    einc = rel_l2(b(got_dx.double() - case.dx_in.double()), b(case.ref_dx - case.dx_in.double()))
    print(f"{tag}: benign rows, pair value vs fp64: x {ex:.2e}, dx {edx:.2e}, increment {einc:.2e}")
    assert ex < 1e-5 and edx < 1e-5
    assert einc < 1.5e-5
    yard = case.row_yardstick(one_pass)
    for r in range(tr.HOSTILE_ROWS):
        kx, kdx = tr.row_err(got_x[r], case.ref_x[r]), tr.row_err(got_dx[r], case.ref_dx[r])
        print(f"{tag}: hostile row {r}: kernel x {kx:.2e} dx {kdx:.2e}; fp32 yardstick x {yard[r][0]:.2e} dx {yard[r][1]:.2e}")
        assert kx <= 4 * yard[r][0] and kdx <= 4 * yard[r][1], (r, kx, kdx, yard[r])
    # hi is the bf16 operand of the new value (re-rounding hi + lo differs only at ties: test_modnorm_residual_pair)
    assert float((hx[:, :d].cpu() != got_x.bfloat16()).float().mean()) < 3e-3
    assert float((hdx[:, :d].cpu() != got_dx.bfloat16()).float().mean()) < 3e-3
    assert (hx[:, d:].float() == 7.0).all() and (hdx[:, d:].float() == 7.0).all()   # pad columns untouched
    if hx_in is not None:  # out of place: the inputs' hi parts are left as they were
        assert torch.equal(bits(hx_in), bits(case.hx)) and torch.equal(bits(hdx_in), bits(case.hdx))
    return got_x, got_dx


@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "to"])
@pytest.mark.parametrize("rps", [64, 1024, 40, 200])
@pytest.mark.parametrize("d", [1056, 1280, 1536, 96])
def test_modnorm_jvp_pair(dev, d, rps, inplace):
    """swiftk_modnorm_jvp_pair against the fp64 tangent on what the pairs hold.  rows_per_sample % 32 == 0 takes the kernel that walks
    32 rows per block and forms the variance in one pass shifted by the row's first element (tuning key 17 = 1); key 17 = 0 and every
    other rows_per_sample take the row-per-wave kernel (two-pass).  d = 1056 / 1280 / 1536 fill one to three 8-channel register slots
    per lane, d = 96 a part of the first.  At the % 32 shapes both kernels run on the same inputs and must agree with each other, and
    where swiftk_modnorm_residual_pair accepts the shape (rows_per_sample % 16 == 0) the primal half must agree with that forward
    kernel: the one-pass sCM loss uses the tangent pass's primal rows as saved activations.
    measured on MI355X over the 32 cases (benign rows, relative L2; both kernels alike): pair value x 6.4e-6 .. 6.6e-6, dx 6.4e-6 .. 6.6e-6,
    increment 9.3e-6 .. 9.6e-6 -- the storage floor, as the fp32 restatement predicts.  Hostile rows, max|err| / max|ref|: row 0 on the
    32-rows-per-block kernel 4.7e-6 .. 1.35e-4 (worst at d = 1536) against a one-pass yardstick of 7.4e-6 .. 2.5e-4, ratio 0.34 .. 1.2; rows 1-3 on
    it, and all four rows on the row-per-wave kernel (row 0: 4.6e-6 .. 2.8e-5), sit ON their yardstick (ratio 1.00 .. 1.02).  The two
    kernels against each other 9.6e-7 .. 1.25e-6, hi mismatch share 5.5e-5 .. 9.1e-5; the primal against swiftk_modnorm_residual_pair
    7.8e-7 .. 1.14e-6, hi mismatch share 2.1e-5 .. 1.1e-4."""
    from swift_amd import ops
    B = 2 if rps == 1024 else 3
    case = _PairCase(dev, d, rps, B, seed=1000 + d + rps, ldy=None if inplace else ops.k_pad(BF, d))
    tag = f"jvp_pair d {d} rows/sample {rps} {'in place' if inplace else 'out of place'}"
    if rps % 32 == 0:
        out_rows = case.run(inplace, 1)
        vx, vdx = _check_pair_result(case, out_rows, True, tag + " [32 rows per block]")
    out_wave = case.run(inplace, 0)
    wx, wdx = _check_pair_result(case, out_wave, False, tag + " [row per wave]")
    b = tr.benign
    if rps % 32 == 0:
        # the two kernels on the same inputs (the bounds test_modnorm_residual_pair holds the forward pair of kernels to)
        e = max(rel_l2(b(vx), b(wx)), rel_l2(b(vdx), b(wdx)))
        mism = max(float((b(out_rows[0][:, :d]) != b(out_wave[0][:, :d])).float().mean()),
                   float((b(out_rows[2][:, :d]) != b(out_wave[2][:, :d])).float().mean()))
        print(f"{tag}: 32-rows-per-block vs row-per-wave kernel: pair values {e:.2e}, hi mismatch share {mism:.2e}")
        assert e < 2e-6 and mism < 1e-3
    if rps % 16 == 0:  # (the forward pair kernel refuses other rows_per_sample: SWIFTK_ESHAPE, include/swiftk.h)
        fh, fl = case.hx.clone(), case.lx.clone()
        ops.modnorm_residual_pair(case.y, fh, fl, case.gamma, case.beta, case.msl, rps, d)
        fx = ops.pair_value(fh, fl, d).cpu()
        for name, (hx, gx) in {"row per wave": (out_wave[0], wx), **({"32 rows per block": (out_rows[0], vx)} if rps % 32 == 0 else {})}.items():
            e, mism = rel_l2(b(gx), b(fx)), float((b(hx[:, :d]) != b(fh[:, :d])).float().mean())
            print(f"{tag}: primal of the {name} kernel vs swiftk_modnorm_residual_pair: {e:.2e}, hi mismatch share {mism:.2e}")
            assert e < 2e-6 and mism < 1e-3


def test_modnorm_jvp_pair_rejections(dev):
    """What the host function refuses before any launch returns the documented code and writes nothing."""
    from swift_amd import _lib
    L = _lib.lib()
    M, d, ld = 64, 1056, 1600   # (buffers wide enough for every d tried below)
    y, dy = (torch.zeros(M + 1, ld, dtype=BF, device=dev) for _ in range(2))
    hx, hdx = (torch.full((M, ld), 3.0, dtype=BF, device=dev) for _ in range(2))
    lx, ldx = (torch.full((M + 1, ld), 77, dtype=torch.uint8, device=dev) for _ in range(2))
    gamma, beta = torch.ones(ld, device=dev), torch.full((ld,), 0.5, device=dev)   # (y = 0: a valid call adds beta to x)
    mod, dmod = torch.zeros(2, 4 * ld, device=dev), torch.zeros(2, 4 * ld, device=dev)
    before = [t.clone() for t in (hx, hdx, lx, ldx)]

    def call(d_=d, M_=M, rps=64, ldmod=2 * d, y_off=0, lo_off=0, ldy=ld):
        return L.swiftk_modnorm_jvp_pair(y.data_ptr() + y_off, dy.data_ptr(), ldy, hx.data_ptr(), hdx.data_ptr(), hx.data_ptr(), hdx.data_ptr(), ld,
                                         lx.data_ptr() + lo_off, ldx.data_ptr(), gamma.data_ptr(), beta.data_ptr(), mod.data_ptr(),
                                         dmod.data_ptr(), ldmod, M_, d_, rps, 1e-6, s())

    assert call(d_=1544) == ESHAPE            # more than three 8-channel slots per lane
    assert call(d_=100) == ESHAPE             # not whole 8-channel chunks
    assert call(rps=48) == ESHAPE             # M % rows_per_sample
    assert call(ldmod=2 * d + 1) == ESHAPE    # ldmod % 4
    assert call(y_off=2) == EALIGN            # y not 16-byte aligned
    assert call(lo_off=4) == EALIGN           # x_lo not 8-byte aligned
    torch.cuda.synchronize()
    assert all(torch.equal(a, b_) for a, b_ in zip(before, (hx, hdx, lx, ldx)))
    assert call() == 0                        # and the same buffers are accepted when nothing is wrong
    torch.cuda.synchronize()
    assert not torch.equal(before[0][:, :d], hx[:, :d])


# ------------------------------------------------------------------------------------------ ModulatedNorm tangent, fp32 stream

def _run_stream(dev, dtype, d, rps, B, seed, ldy=None, odd_ldmod=False):
    """One swiftk_modnorm_jvp call; returns (case, x, dx, xT, dxT, ref_x, ref_dx, ldxT)."""
    from swift_amd import _lib, ops
    L = _lib.lib()
    M = B * rps
    c = tr.make_norm_case(d, rps, B, seed, bf16_rows=dtype == BF)   # (fp32: the benign rows keep every mantissa bit)
    ldy = ldy or d
    ldxT = ops.k_pad(dtype, d)
    y, dy = (torch.zeros(M, ldy, dtype=dtype, device=dev) for _ in range(2))
    y[:, :d], dy[:, :d] = c["y"].to(dev).to(dtype), c["dy"].to(dev).to(dtype)
    assert torch.equal(y[:, :d].float().cpu(), c["y"])   # the reference sees what the kernel sees
    x, dx = c["x"].to(dev).clone(), c["dx"].to(dev).clone()
    xT, dxT = (torch.full((M, ldxT), 7.0, dtype=dtype, device=dev) for _ in range(2))
    xT[:, :d] = float("nan")
    dxT[:, :d] = float("nan")
    wcols = 6 * d + (1 if odd_ldmod else 0)
    wide, dwide = rnd((B, wcols), seed + 1).to(dev), rnd((B, wcols), seed + 2).to(dev)
    wide[:, 2 * d: 4 * d], dwide[:, 2 * d: 4 * d] = c["mod"].to(dev), c["dmod"].to(dev)
    msl, dsl = wide[:, 2 * d: 4 * d], dwide[:, 2 * d: 4 * d]
    gamma, beta = c["gamma"].to(dev), c["beta"].to(dev)
    rc = L.swiftk_modnorm_jvp(y.data_ptr(), dy.data_ptr(), ldy, x.data_ptr(), dx.data_ptr(), xT.data_ptr(), dxT.data_ptr(), ldxT,
                              gamma.data_ptr(), beta.data_ptr(), msl.data_ptr(), dsl.data_ptr(), msl.stride(0), M, d, rps, 1e-6,
                              ops.dtype_code(dtype), s())
    assert rc == 0
    torch.cuda.synchronize()
    ref_x, ref_dx = tr.modnorm_tangent(**c)
    return c, x, dx, xT, dxT, ref_x, ref_dx, ldxT


STREAM_CASES = [pytest.param(1056, 64, None, False, id="vector-1056-64"), pytest.param(1056, 50, None, False, id="vector-1056-50"),
                pytest.param(1536, 64, None, False, id="vector-1536-64"), pytest.param(1536, 50, None, False, id="vector-1536-50"),
                pytest.param(100, 50, None, False, id="scalar-d100"), pytest.param(1056, 64, 1058, False, id="scalar-ldy1058"),
                pytest.param(1056, 64, None, True, id="scalar-ldmod-odd")]


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("d,rps,ldy,odd_ldmod", STREAM_CASES)
def test_modnorm_jvp_stream(dev, dtype, d, rps, ldy, odd_ldmod):
    """swiftk_modnorm_jvp (fp32 residual stream, operand copies in `dtype`): the 8-wide vector kernel, and the scalar kernel forced
    three ways -- d not a multiple of 8, a row stride of y that is not, an ldmod that is not a multiple of 4.  x, dx against fp64 at
    F32_TOL (the fp32 two-pass restatement measures 7e-8); the operand copies are the roundings of the kernel's own fp32 outputs.
    measured on MI355X (14 cases): benign rows x 5.9e-8 .. 6.5e-8, dx 6.0e-8 .. 6.6e-8, increment 8.7e-8 .. 9.8e-8; hostile rows 5.0e-8 .. 2.4e-7
    against yardsticks of 5.8e-8 .. 2.4e-7.  Before the scalar kernel took its means by division, its row 1 (the constant row at 40) had
    x off by 6.4e-4 (d = 1056) / 5.9e-4 (d = 100) of the row's maximum and dx by 9.4e-7: `sum * (1 / d)` was contracted into the
    subtraction y - mean, which exposed the rounding of 1 / d times 40 times rstd = 1e3 (csrc/jvp_kernels.hip)."""
    c, x, dx, xT, dxT, ref_x, ref_dx, ldxT = _run_stream(dev, dtype, d, rps, 3, 2000 + d + rps, ldy, odd_ldmod)
    b = tr.benign
    xc, dxc = x.cpu(), dx.cpu()
    assert torch.isfinite(xc).all() and torch.isfinite(dxc).all()
    ex, edx = rel_l2(b(xc), b(ref_x)), rel_l2(b(dxc), b(ref_dx))
    einc = rel_l2(b(dxc.double() - c["dx"].double()), b(ref_dx - c["dx"].double()))
    print(f"modnorm_jvp d {d} rows/sample {rps}: benign rows vs fp64: x {ex:.2e}, dx {edx:.2e}, increment {einc:.2e}")
    assert ex < F32_TOL and edx < F32_TOL and einc < F32_TOL
    n = tr.HOSTILE_ROWS
    x32, dx32 = tr.modnorm_tangent_fp32(c["y"][:n], c["dy"][:n], c["x"][:n], c["dx"][:n], c["gamma"], c["beta"], c["mod"][:1], c["dmod"][:1], n)
    for r in range(n):
        kx, kdx = tr.row_err(xc[r], ref_x[r]), tr.row_err(dxc[r], ref_dx[r])
        yx, ydx = tr.row_err(x32[r], ref_x[r]), tr.row_err(dx32[r], ref_dx[r])
        print(f"modnorm_jvp d {d} rows/sample {rps}: hostile row {r}: kernel x {kx:.2e} dx {kdx:.2e}; fp32 yardstick x {yx:.2e} dx {ydx:.2e}")
        assert kx <= max(4 * yx, F32_TOL) and kdx <= max(4 * ydx, F32_TOL), (r, kx, kdx, yx, ydx)
    assert torch.equal(bits(xT[:, :d]), bits(x.to(dtype))) and torch.equal(bits(dxT[:, :d]), bits(dx.to(dtype)))
    assert (xT[:, d:].float() == 7.0).all() and (dxT[:, d:].float() == 7.0).all()


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
def test_modnorm_jvp_stream_scalar_equals_vector(dev, dtype):
    """The scalar and the vector kernel on the same data (d = 1056: contiguous rows of y against a row stride of 1058).
    measured on MI355X: 6.8e-8 (fp32 and bf16 operands alike); 1.2e-3 on the constant row before the scalar kernel's fix."""
    _, xv, dxv, xTv, dxTv, _, _, _ = _run_stream(dev, dtype, 1056, 64, 3, 77)
    _, xs, dxs, xTs, dxTs, _, _, _ = _run_stream(dev, dtype, 1056, 64, 3, 77, ldy=1058)
    b = tr.benign
    e = max(rel_l2(b(xs.cpu()), b(xv.cpu())), rel_l2(b(dxs.cpu()), b(dxv.cpu())))
    print(f"modnorm_jvp scalar vs vector kernel ({dtype}): {e:.2e}")
    assert e < 2e-6
    for r in range(tr.HOSTILE_ROWS):  # (rows whose tangents are 1e3 times larger score on their own)
        assert rel_l2(xs[r].cpu(), xv[r].cpu()) < 2e-6 and rel_l2(dxs[r].cpu(), dxv[r].cpu()) < 2e-6, r


# ------------------------------------------------------------------------------------------ QK-norm and SwiGLU tangents, alone

def _dt_name(dt):
    return "bf16" if dt == BF else "fp32"


def _sent(shape, dt, dev):
    """A buffer of ``dt`` holding the NaN pattern of exact_attention.sent in every element."""
    import exact_attention as X
    return X.sent(shape, dt == torch.float32, dev).view(dt)


def _vec_rel_l2(got, ref):
    """[..., hd] x 2 -> relative L2 per vector (fp64); a zero reference vector scores 0 when met exactly, inf otherwise."""
    g, r = got.double(), ref.double()
    num, den = (g - r).norm(dim=-1), r.norm(dim=-1)
    return torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num > 0, torch.full_like(num, float("inf")), torch.zeros_like(num)))


@pytest.mark.parametrize("with_rn", [True, False], ids=["rn", "rn-null"])
@pytest.mark.parametrize("dt", [BF, torch.float32], ids=_dt_name)
@pytest.mark.parametrize("M,heads,hd", tr.QKNORM_JVP_CASES)
def test_qknorm_jvp_alone(dev, M, heads, hd, dt, with_rn):
    """swiftk_qknorm_jvp in place on rows padded with the NaN pattern of exact_attention.sent (ld = width + 24, one extra row) against the fp64 closed form on the stored values
    (tangent_reference.qknorm_tangent): every q / k vector, primal and tangent, within BF16_VEC_TOL = 2^-8 (bf16) / F32_TOL (fp32)
    relative L2; the v third, the dv third and the pad keep their bits; rn = 1 / |x| to 1e-6 and exactly 1 for v, no entry left
    unwritten, the row behind the last untouched.  18 and 3096 vectors: a ragged last block of 16; the last head's scale is ln 200
    (clamped); two all-zero primal vectors keep a zero primal and get the finite tangent tau dx 1e12.
    measured on MI355X (16 cases; bound in brackets): worst vector bf16 primal 2.0e-3 .. 2.4e-3, tangent 1.8e-3 .. 2.2e-3 [3.9e-3], medians
    1.6e-3 .. 1.7e-3; fp32 primal 9.9e-8 .. 1.7e-7, tangent 9.5e-8 .. 1.9e-7 [1e-5], medians 3.1e-8 .. 4.9e-8; rn 5.8e-8 .. 1.3e-7 [1e-6].
    Passes on the parent commit."""
    from swift_amd import _lib, ops
    L = _lib.lib()
    width = 3 * heads * hd
    ld = width + 24
    q32, dq32, scale = tr.qknorm_jvp_inputs(M, heads, hd, 500 + M + hd)
    qs, dqs = q32.to(dt).float(), dq32.to(dt).float()   # the values the kernel reads
    buf, dbuf = _sent((M + 1, ld), dt, dev), _sent((M + 1, ld), dt, dev)
    buf[:M, :width], dbuf[:M, :width] = qs.to(dev).to(dt), dqs.to(dev).to(dt)
    before, dbefore = buf.clone(), dbuf.clone()
    rn = _sent((M + 1, 3 * heads), torch.float32, dev)
    rc = L.swiftk_qknorm_jvp(buf.data_ptr(), dbuf.data_ptr(), ld, scale.to(dev).data_ptr(), rn.data_ptr() if with_rn else None, M, heads, hd,
                             ops.dtype_code(dt), s())
    assert rc == 0
    torch.cuda.synchronize()
    ref, dref, rn_ref = tr.qknorm_tangent(qs, dqs, scale, heads, hd)
    tol = 2.0 ** -8 if dt == BF else F32_TOL
    tag = f"qknorm_jvp {_dt_name(dt)} M {M} heads {heads} head_dim {hd}{'' if with_rn else ' rn NULL'}"
    for what, b_, b0, r_ in (("primal", buf, before, ref), ("tangent", dbuf, dbefore, dref)):
        assert torch.equal(bits(b_[:, width:]), bits(b0[:, width:])) and torch.equal(bits(b_[M]), bits(b0[M])), f"{tag} {what}: pad or extra row written"
        gv, bv = b_[:M, :width].reshape(M, heads, 3, hd), b0[:M, :width].reshape(M, heads, 3, hd)
        assert torch.equal(bits(gv[:, :, 2]), bits(bv[:, :, 2])), f"{tag} {what}: the v third changed"
        got = gv[:, :, :2].float().cpu()
        assert torch.isfinite(got).all()
        e = _vec_rel_l2(got, r_[:, :, :2])
        w = int(e.flatten().argmax())
        print(f"{tag} {what}: worst vector {float(e.max()):.2e} (row {w // (2 * heads)}, head {w // 2 % heads}, {'qk'[w % 2]}; bound {tol:.2e}), "
              f"median {float(e.median()):.2e}")
        assert float(e.max()) <= tol
    for z in tr.zero_vectors(M, heads):
        assert float(buf[z[0], (z[1] * 3 + z[2]) * hd:(z[1] * 3 + z[2] + 1) * hd].float().abs().max()) == 0.0   # the primal stays 0
    if with_rn:
        rg = rn.cpu()
        assert torch.equal(bits(rg[M]), bits(_sent((3 * heads,), torch.float32, "cpu"))) and torch.isfinite(rg[:M]).all()
        rg = rg[:M].view(M, heads, 3)
        assert bool((rg[:, :, 2] == 1.0).all())
        e = ((rg[:, :, :2].double() - rn_ref[:, :, :2]).abs() / rn_ref[:, :, :2]).max()
        print(f"{tag}: rn worst relative error {float(e):.2e} (bound 1e-6)")
        assert float(e) <= 1e-6


@pytest.mark.parametrize("dt", [BF, torch.float32], ids=_dt_name)
def test_qknorm_jvp_refusals(dev, dt):
    """Head width 64, a row stride under the width and NULL pointers return the header's codes and write nothing."""
    from swift_amd import _lib, ops
    L = _lib.lib()
    M, heads, hd = 3, 3, 88
    width = 3 * heads * hd
    buf, dbuf = (torch.full((M, width), 0.5, dtype=dt, device=dev) for _ in range(2))
    scale, rn = torch.zeros(heads, device=dev), nan_like((M, 3 * heads), dev)
    keep = [bits(t).clone() for t in (buf, dbuf, rn)]

    def call(q=buf.data_ptr(), dq=dbuf.data_ptr(), ld=width, sc=scale.data_ptr(), hd_=hd):
        return L.swiftk_qknorm_jvp(q, dq, ld, sc, rn.data_ptr(), M, heads, hd_, ops.dtype_code(dt), s())

    assert call(hd_=64) == ESHAPE            # (3 heads of 64 need less room than the buffers have)
    assert call(ld=width - 8) == ESHAPE
    assert call(q=None) == EINVAL and call(dq=None) == EINVAL and call(sc=None) == EINVAL
    torch.cuda.synchronize()
    assert all(torch.equal(bits(t), k) for t, k in zip((buf, dbuf, rn), keep))
    assert call() == 0
    torch.cuda.synchronize()
    assert not torch.equal(bits(buf), keep[0]) and torch.isfinite(rn).all()


@pytest.mark.parametrize("M,mlp", [(1, 8), (5, 37), (385, 2816)])
@pytest.mark.parametrize("dt", [BF, torch.float32], ids=_dt_name)
def test_swiglu_jvp_alone(dev, dt, M, mlp):
    """swiftk_swiglu_jvp with both row strides larger than the widths and the NaN pattern of exact_attention.sent in every pad column, on backward_reference.swiglu_inputs
    (the last row starts with the planted gates -100, -30, -1.2784645, 0, 30, 100) and a random tangent.  (385, 2816) is 1,084,160
    items: the grid-stride loop's second trip with a ragged end.  Bounds as test_swiglu_fwd_bwd_per_element: bf16 within 1 bf16 ulp of
    the rounded fp64 value and different from it on <= 1e-3 of the elements; fp32 within 8 x the error of torch's fp32 CPU evaluation
    of the same formulas, both relative to the element's scale (tangent_reference.swiglu_tangent) + 2^-102.  Inputs and pads keep
    their bits.
    measured on MI355X (bound in brackets): bf16 against the fp64 value rounded once: tangent 0.00 ulp and 0 mismatches in all three
    shapes, out (fp32 arithmetic) <= 1.00 ulp [1], mismatch share 1.2e-5 at (385, 2816) [1e-3]; against the fp64 value rounded through
    fp32, as test_swiglu_fwd_bwd_per_element scores (asserted too): out 1.00 ulp, 8.3e-6; tangent 1.00 ulp, 1.0e-5 -- those 11
    elements are the REFERENCE's second rounding: the exact value lies within 2^-24 of a bf16 tie (6.671874914 under 6.671875), its
    fp32 rounding is the tie, and ties-to-even then picks the farther neighbour; the kernel, converting fp64 to bf16 directly,
    returns the nearer one (tests/test_tangent_reference_cpu.py::test_bf16_round_once_rounds_once).  fp32 out 7.8e-8 .. 2.0e-7,
    tangent 1.1e-7 .. 3.8e-7 of the element's scale, torch's fp32 evaluation on the CPU the same to two digits [8 x: 6.3e-7 ..
    3.1e-6]; at the planted gate -30 out 6.7e-8 .. 1.3e-7, tangent 9.4e-9 .. 1.1e-7: the fp32 instantiation already took expf and a
    true division and needed no cure.
    [bf16-385-2816] fails on the parent commit: the tangent is a sum of two products, the two cancel to 2.5e-6 of their size at
    element (7, 187) (below 2^-15 at twenty elements), and the fp32 evaluation stood 2.00 bf16 ulp from the rounded fp64 value there
    (mismatch share 3.4e-5 through fp32) -- as does torch's own fp32 evaluation (2.00 ulp, 3.8e-5).  The bf16 instantiation now forms
    its tangent in fp64, sigmoid included, and converts it to bf16 in one rounding (csrc/jvp_kernels.hip, swiglu_tangent): 0.00 ulp.
    Its cost, printed by the (385, 2816) case: 141 us per call at (12288, 2816), 2.94 TB/s of the 12 bytes an element moves; the
    parent's fp32 form was not timed on the same machine, so what the fp64 sigmoid adds is not known."""
    import backward_reference as br
    from swift_amd import _lib, ops
    L = _lib.lib()
    h32, _ = br.swiglu_inputs(M, mlp, 40 + M)
    dh32 = rnd((M, 2 * mlp), 140 + M)
    hv, dhv = h32.to(dt).float(), dh32.to(dt).float()   # the values the kernel reads
    ldh, ldo = 2 * mlp + 16, mlp + 8
    h, dh = _sent((M, ldh), dt, dev), _sent((M, ldh), dt, dev)
    h[:, :2 * mlp], dh[:, :2 * mlp] = hv.to(dev).to(dt), dhv.to(dev).to(dt)
    o, do = _sent((M + 1, ldo), dt, dev), _sent((M + 1, ldo), dt, dev)   # (outputs: the NaN pattern everywhere, one extra row)
    h0, dh0, o0 = h.clone(), dh.clone(), o.clone()
    assert L.swiftk_swiglu_jvp(h.data_ptr(), dh.data_ptr(), ldh, o.data_ptr(), do.data_ptr(), ldo, M, mlp, ops.dtype_code(dt), s()) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(h), bits(h0)) and torch.equal(bits(dh), bits(dh0))                               # inputs and their pads
    assert torch.equal(bits(o[:, mlp:]), bits(o0[:, mlp:])) and torch.equal(bits(do[:, mlp:]), bits(o0[:, mlp:]))   # output pads
    assert torch.equal(bits(o[M]), bits(o0[M])) and torch.equal(bits(do[M]), bits(o0[M]))                          # and the extra row
    got = {"out": o[:M, :mlp].float().cpu(), "tangent": do[:M, :mlp].float().cpu()}
    assert all(torch.isfinite(v).all() for v in got.values())
    ro, rd, so, sd = tr.swiglu_tangent(hv, dhv)
    ref, scale = {"out": ro, "tangent": rd}, {"out": so + 2.0 ** -102, "tangent": sd + 2.0 ** -102}
    tag = f"swiglu_jvp {_dt_name(dt)} ({M}, {mlp})"
    if dt == BF:
        for k in got:
            ulps, share = tr.bf16_score_once(got[k], ref[k])       # the fp64 value rounded once
            ulps2, share2 = br.bf16_score(got[k], ref[k])          # ... and through fp32, as test_swiglu_fwd_bwd_per_element scores
            print(f"{tag} {k}: worst {ulps:.2f} bf16 ulp from the rounded fp64 value (bound 1), mismatch share {share:.2e} (cap 1e-3); "
                  f"from the fp64 value rounded through fp32 {ulps2:.2f} ulp, {share2:.2e}")
            assert ulps <= 1.0 and share <= 1e-3, (k, ulps, share)
            assert ulps2 <= 1.0 and share2 <= 1e-3, (k, ulps2, share2)
        if M == 385:   # what the fp64 sigmoid costs the bf16 instantiation (printed, nothing asserted)
            Mw = 12288
            hw, dhw = (torch.randn(Mw, 2 * mlp, device=dev).to(dt) for _ in range(2))
            ow, dow = (torch.empty(Mw, mlp, dtype=dt, device=dev) for _ in range(2))
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            for rep in range(3):
                if rep == 1:
                    ev[0].record()
                assert L.swiftk_swiglu_jvp(hw.data_ptr(), dhw.data_ptr(), 2 * mlp, ow.data_ptr(), dow.data_ptr(), mlp, Mw, mlp, ops.dtype_code(dt), s()) == 0
            ev[1].record()
            torch.cuda.synchronize()
            us = ev[0].elapsed_time(ev[1]) * 1e3 / 2
            print(f"swiglu_jvp bf16 ({Mw}, {mlp}): {us:.0f} us per call, {12 * Mw * mlp / us / 1e6:.2f} TB/s of its 12 bytes per element")
        return
    yo, yd, _, _ = tr.swiglu_tangent(hv, dhv, torch.float32)
    yard = {"out": yo, "tangent": yd}
    for k in got:
        ek = float(((got[k].double() - ref[k]).abs() / scale[k]).max())
        ey = float(((yard[k].double() - ref[k]).abs() / scale[k]).max())
        planted = ((got[k][M - 1, :min(6, mlp)].double() - ref[k][M - 1, :min(6, mlp)]).abs() / scale[k][M - 1, :min(6, mlp)]).tolist()
        print(f"{tag} {k}: worst element error {ek:.2e} of its scale; torch fp32 on the CPU {ey:.2e}, bound 8 x = {8 * ey:.2e}; planted gates "
              f"{[f'{v:.1e}' for v in planted]}")
        assert ek <= 8 * ey, (k, ek, ey)


# ------------------------------------------------------------------------------------------ SiLU, time embedding

def _silu_inputs(n, dev):
    z = rnd((n,), 41, 3.0)
    special = torch.tensor([0.0, 30.0, -30.0, 90.0, -90.0])[:n]   # expf(90) overflows in fp32: the limits must still come out
    z[: special.numel()] = special
    return z.to(dev), rnd((n,), 42).to(dev)


@pytest.mark.parametrize("n", [1, 255, 2 * 1056, 1_000_003])
def test_silu_jvp_and_bwd(dev, n):
    from swift_amd import _lib
    L = _lib.lib()
    z, dz = _silu_inputs(n, dev)
    ref_y, ref_dy = tr.silu_tangent(z.cpu(), dz.cpu())
    y, dy = nan_like((n,), dev), nan_like((n,), dev)
    assert L.swiftk_silu_jvp(z.data_ptr(), dz.data_ptr(), y.data_ptr(), dy.data_ptr(), n, s()) == 0
    assert torch.isfinite(y).all() and torch.isfinite(dy).all()
    assert rel_l2(y.cpu(), ref_y) < F32_TOL and rel_l2(dy.cpu(), ref_dy) < F32_TOL
    dy2 = nan_like((n,), dev)
    assert L.swiftk_silu_jvp(z.data_ptr(), dz.data_ptr(), None, dy2.data_ptr(), n, s()) == 0   # y = NULL
    assert torch.equal(dy2, dy)
    g = nan_like((n,), dev)
    assert L.swiftk_silu_bwd(z.data_ptr(), dz.data_ptr(), g.data_ptr(), n, s()) == 0
    assert torch.isfinite(g).all() and rel_l2(g.cpu(), tr.silu_grad(z.cpu()) * dz.cpu().double()) < F32_TOL
    if n >= 5:  # silu'(90) = 1, silu'(-90) = 0 (to fp32), silu'(0) = 1/2
        for out in (dy, g):
            o, dzc = out.cpu(), dz.cpu()
            assert abs(float(o[3] / dzc[3]) - 1.0) < 1e-6 and abs(float(o[4])) < 1e-30 and abs(float(o[0] / dzc[0]) - 0.5) < 1e-6


@pytest.mark.parametrize("w", [1.0, 1000.0])
@pytest.mark.parametrize("B,d", [(2, 1056), (5, 97), (1, 2)])
def test_timestep_embed_jvp(dev, B, d, w):
    """d/dt of the time embedding, [cos | -sin](t w f) w f dt; odd d leaves the last column zero.  At timestep_weight 1 (the shipped
    config) the arguments stay below 1.6 rad: 1e-5.  At weight 1000 the fp32 product t w f is itself rounded before cosf sees it (an
    argument of 1500 rad carries 6e-5 rad of rounding), so the bound is 4 x the error of the SAME expression evaluated in fp32 torch
    on the CPU against fp64: that error is 5.9e-6 .. 1.6e-5 over the three shapes, i.e. a bound of 2.4e-5 .. 6.5e-5 (printed).
    measured on MI355X: weight 1: 3.1e-8 .. 4.5e-8; weight 1000: 5.9e-6 .. 1.6e-5, the CPU evaluation's own error to two digits."""
    from swift_amd import _lib
    L = _lib.lib()
    half = d // 2
    freqs = torch.exp(-math.log(10_000) * torch.arange(half, dtype=torch.float32) / half)
    t, dt = torch.tensor([0.4, 1.5, 0.0, 0.4, 1.5])[:B], rnd((B,), 51)
    ref = tr.timestep_embed_tangent(t, dt, freqs, d, w)
    out = nan_like((B, d), dev)
    assert L.swiftk_timestep_embed_jvp(t.to(dev).data_ptr(), dt.to(dev).data_ptr(), freqs.to(dev).data_ptr(), out.data_ptr(), B, d, w, s()) == 0
    got = out.cpu()
    assert torch.isfinite(got).all()
    if d % 2:
        assert float(got[:, -1].abs().max()) == 0.0
    e = rel_l2(got, ref)
    if w == 1.0:
        bound = F32_TOL
    else:
        bound = 4 * rel_l2(tr.timestep_embed_tangent(t, dt, freqs, d, w, dtype=torch.float32), ref)
    print(f"timestep_embed_jvp B {B} d {d} weight {w}: kernel {e:.2e}, bound {bound:.2e}")
    assert e < bound
    for b_ in range(B):  # every sample on its own (dt differs by sample, so one sample cannot hide behind another)
        assert rel_l2(got[b_], ref[b_]) < 2 * bound or float(ref[b_].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ sCM target, per-sample / per-channel axpy

@pytest.mark.parametrize("r", [0.0, 0.4, 1.0])
@pytest.mark.parametrize("per", [69 * 64 * 64, 1000, 7])
@pytest.mark.parametrize("B", [1, 3])
def test_scm_target(dev, B, per, r):
    """target = F + g / (rms_b(g) + 0.1) against fp64, sample by sample.  At B = 3 the middle sample has dxt = sd F, x_t = 0, dF = 0
    with F held by bf16 and sd = 0.75, so that sd F is exact in fp32 and g is exactly zero: the + 0.1 keeps the division finite and
    the target is F bit for bit.  The scratch arrives full of NaN (the call clears it); the per-sample sum is atomic, so a second
    call may differ in the last bit only.
    measured on MI355X (36 samples): target <= 5.3e-7, the normalised g alone <= 4.7e-6 (t = 1.55, r = 0, where g is 4e-3 of F)."""
    from swift_amd import _lib
    L = _lib.lib()
    sd = 0.75
    F_, dxt, xos, dF = (rnd((B, per), 60 + i) for i in range(4))
    t = torch.tensor([0.8, 0.02, 1.55])[:B]
    if B == 3:
        F_[1] = tr.bf16_round(F_[1])
        dxt[1], xos[1], dF[1] = sd * F_[1], 0.0, 0.0
    ref, ref_g = tr.scm_target(F_, dxt, xos, dF, t, r, sd)
    dv = [v.to(dev) for v in (F_, dxt, xos, dF, t)]
    outs = []
    for _ in range(2):
        target, ss = nan_like((B, per), dev), nan_like((B,), dev)
        assert L.swiftk_scm_target(*(v.data_ptr() for v in dv), r, sd, target.data_ptr(), ss.data_ptr(), B, per, s()) == 0
        outs.append(target.cpu())
    got = outs[0]
    assert torch.isfinite(got).all()
    for b_ in range(B):
        e = rel_l2(got[b_], ref[b_])
        # the normalised g alone: the final fp32 add rounds at 2^-24 |target|, which the subtraction below brings back
        gn = ref[b_] - F_[b_].double()
        slack = 2.0 ** -23 * float(ref[b_].norm() / gn.norm().clamp_min(1e-300))
        eg = rel_l2(got[b_].double() - F_[b_].double(), gn) if float(gn.norm()) > 0 else 0.0
        print(f"scm_target B {B} per_sample {per} r {r} sample {b_} (t {float(t[b_]):.2f}): target {e:.2e}, normalised g {eg:.2e} (slack {slack:.1e})")
        assert e < F32_TOL and eg < F32_TOL + slack
    if B == 3:
        assert float(ref_g[1].abs().max()) == 0.0 and torch.equal(bits(got[1]), bits(F_[1]))
    assert rel_l2(outs[1], got) < 1e-6


def test_axpby_per_sample(dev):
    from swift_amd import _lib
    L = _lib.lib()
    B, per = 3, 69 * 64 * 5 + 3
    a, c = torch.tensor([0.3, -1.7, 2.5]), torch.tensor([1.1, 0.0, -0.6])
    x, y = rnd((B, per), 70), rnd((B, per), 71)
    ad, cd, xd, yd = (v.to(dev) for v in (a, c, x, y))
    out = nan_like((B, per), dev)
    assert L.swiftk_axpby_per_sample(out.data_ptr(), ad.data_ptr(), xd.data_ptr(), cd.data_ptr(), yd.data_ptr(), B, per, s()) == 0
    assert rel_l2(out.cpu(), a.double()[:, None] * x.double() + c.double()[:, None] * y.double()) < F32_TOL
    out = nan_like((B, per), dev)
    assert L.swiftk_axpby_per_sample(out.data_ptr(), ad.data_ptr(), xd.data_ptr(), None, None, B, per, s()) == 0   # without y
    assert torch.equal(out.cpu(), a[:, None] * x)
    assert L.swiftk_axpby_per_sample(out.data_ptr(), ad.data_ptr(), xd.data_ptr(), None, yd.data_ptr(), B, per, s()) == EINVAL  # y without c


@pytest.mark.parametrize("hw", [64 * 64, 5])
def test_channel_axpy(dev, hw):
    """out = x + coef[channel] y, with and without x (both forms of the CRPS loss's condition update), and out aliasing x."""
    from swift_amd import _lib
    L = _lib.lib()
    B, C = 2, 69
    x, y, coef = rnd((B, C, hw), 72), rnd((B, C, hw), 73), rnd((C,), 74)
    xd, yd, cd = x.to(dev), y.to(dev), coef.to(dev)
    ref = x.double() + coef.double()[None, :, None] * y.double()
    out = nan_like((B, C, hw), dev)
    assert L.swiftk_channel_axpy(out.data_ptr(), xd.data_ptr(), yd.data_ptr(), cd.data_ptr(), B, C, hw, s()) == 0
    assert rel_l2(out.cpu(), ref) < F32_TOL
    out2 = nan_like((B, C, hw), dev)
    assert L.swiftk_channel_axpy(out2.data_ptr(), None, yd.data_ptr(), cd.data_ptr(), B, C, hw, s()) == 0
    assert torch.equal(out2.cpu(), coef[None, :, None] * y)
    xa = xd.clone()
    assert L.swiftk_channel_axpy(xa.data_ptr(), xa.data_ptr(), yd.data_ptr(), cd.data_ptr(), B, C, hw, s()) == 0   # in place
    assert torch.equal(xa, out)


def test_edm_prep(dev):
    from swift_amd import _lib
    L = _lib.lib()
    B, per, sd = 3, 69 * 16 * 5 + 1, 0.7
    x, z, sigma = rnd((B, per), 75), rnd((B, per), 76), torch.tensor([0.002, 0.5, 80.0])
    out = nan_like((B, per), dev)
    assert L.swiftk_edm_prep(x.to(dev).data_ptr(), z.to(dev).data_ptr(), sigma.to(dev).data_ptr(), out.data_ptr(), sd, B, per, s()) == 0
    sg = sigma.double()[:, None]
    ref = (x.double() + sg * z.double()) / torch.sqrt(sg ** 2 + float(torch.tensor(sd)) ** 2)   # (sd as the fp32 the kernel receives)
    for b_ in range(B):
        assert rel_l2(out[b_].cpu(), ref[b_]) < F32_TOL, b_


# ------------------------------------------------------------------------------------------ sums and copies

@pytest.mark.parametrize("H,W", [(16, 32), (7, 3)])
def test_rmse_sums(dev, H, W):
    """sq[0] += sum (y - t)^2, sq[1 + c] += sum w_lat[h] (y - t)^2 with t a slice of [B, days, C, H, W] (batch stride != C H W), on
    top of a non-zero sq; fp64 reference, 1e-5 (sums of <= 1536 positive terms per atomic)."""
    from swift_amd import _lib
    L = _lib.lib()
    B, C, days = 3, 5, 3
    y, T = rnd((B, C, H, W), 80), rnd((B, days, C, H, W), 81)
    w_lat = torch.cos(torch.deg2rad(torch.linspace(-80, 80, H)))
    w_lat = w_lat / w_lat.mean()
    sq0 = rnd((1 + C,), 82).abs() + 0.5
    yd, Td, wd, sq = y.to(dev), T.to(dev), w_lat.to(dev), sq0.to(dev).clone()
    tsl = Td[:, 1]
    assert L.swiftk_rmse_sums(yd.data_ptr(), tsl.data_ptr(), Td.stride(0), wd.data_ptr(), sq.data_ptr(), B, C, H, W, s()) == 0
    ref = tr.rmse_sums(y, T[:, 1], w_lat)
    assert rel_l2(sq.cpu(), sq0.double() + ref) < F32_TOL
    assert rel_l2(sq.cpu().double() - sq0.double(), ref) < F32_TOL
    assert float(((sq.cpu().double() - sq0.double() - ref).abs() / ref).max()) < 4 * F32_TOL   # every channel's sum, not only the large ones


def test_colsum(dev):
    """out[c] += sum_r src[r][c] (period 0) and out[r % period][c] += src[r][c], accumulating on a non-zero out; a row count that
    is not a multiple of the kernel's 64 rows per block, and rows narrower than their stride."""
    from swift_amd import _lib
    L = _lib.lib()
    rows, cols, lds = 70, 130, 136
    src = rnd((rows, lds), 83).to(dev)
    out0 = rnd((cols,), 84).to(dev)
    out = out0.clone()
    assert L.swiftk_colsum(src.data_ptr(), lds, out.data_ptr(), rows, cols, 0, s()) == 0
    assert rel_l2(out.cpu(), out0.cpu().double() + src[:, :cols].cpu().double().sum(0)) < F32_TOL
    for rows_p in (21, 70):
        outp0 = rnd((7, cols), 85).to(dev)
        outp = outp0.clone()
        assert L.swiftk_colsum(src.data_ptr(), lds, outp.data_ptr(), rows_p, cols, 7, s()) == 0
        ref = outp0.cpu().double() + src[:rows_p, :cols].cpu().double().view(rows_p // 7, 7, cols).sum(0)
        assert rel_l2(outp.cpu(), ref) < F32_TOL, rows_p


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,cols,lds,ldd", [(70, 130, 136, 160), (2112, 1056, 1056, 1088)])
def test_cast_pad(dev, dtype, rows, cols, lds, ldd):
    from swift_amd import _lib, ops
    L = _lib.lib()
    src = rnd((rows, lds), 86).to(dev)
    dst = nan_like((rows, ldd), dev, dtype)
    assert L.swiftk_cast_pad(src.data_ptr(), lds, dst.data_ptr(), ldd, rows, cols, ops.dtype_code(dtype), s()) == 0
    assert torch.equal(bits(dst[:, :cols]), bits(src[:, :cols].to(dtype)))
    assert torch.equal(bits(dst[:, cols:]), torch.zeros_like(bits(dst[:, cols:])))   # pad columns are + 0


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,W", [pytest.param(64, 64, id="tiled"), pytest.param(8, 24, id="per-element")])
def test_patchify_scaled(dev, dtype, H, W):
    """swiftk_patchify_scaled: EDM's per-sample c_in on source 0.  The launcher takes patchify_tiled_kernel when the grid row is whole
    16-token runs with 16-byte aligned rows (gw % 16 == 0, W % 4 == 0, lda % 8 == 0, aligned pointers, tile <= 64 KB) -- 64 x 64 with
    2 x 2 patches, gw = 32 -- and patchify_kernel (an element per thread) otherwise -- 8 x 24, gw = 12.  The two apply the per-sample
    factor in different places (on the value, resp. folded into the channel scale)."""
    from oracle.swinv2 import patchify as opatchify
    from swift_amd import _lib, ops
    L = _lib.lib()
    B, c0, c1, p, s1 = 3, 5, 3, (2, 2), 1.5
    F_ = p[0] * p[1] * (c0 + c1)
    lda = ops.k_pad(dtype, F_)
    src0, src1 = rnd((B, c0, H, W), 87).to(dev), rnd((B, c1, H, W), 88).to(dev)
    ntok = B * (H // 2) * (W // 2)

    def scaled(s0, sps):
        A = torch.full((ntok, lda), 7.0, dtype=dtype, device=dev)
        rc = L.swiftk_patchify_scaled(src0.data_ptr(), c0, s0, None if sps is None else sps.data_ptr(), src1.data_ptr(), c1, s1, None, 0, 1.0,
                                      A.data_ptr(), lda, B, H, W, p[0], p[1], ops.dtype_code(dtype), s())
        assert rc == 0
        return A

    pow2 = torch.tensor([0.5, 2.0, -1.0], device=dev)   # powers of two: scaling commutes with every rounding
    for s0 in (1.0, 0.25):
        A = scaled(s0, pow2)
        ref = ops.patchify([src0 * (s0 * pow2)[:, None, None, None], src1], [1.0, s1], p, lda, dtype)
        assert torch.equal(bits(A), bits(ref)), s0   # source 1's columns and the zeroed pad columns included
        assert (A[:, F_:].float() == 0).all()
    assert torch.equal(bits(scaled(0.25, None)), bits(ops.patchify([src0, src1], [0.25, s1], p, lda, dtype)))   # NULL = swiftk_patchify
    gen = torch.tensor([0.3, 1.7, -0.9], device=dev)
    A = scaled(0.25, gen)
    full = torch.cat([src0.cpu().double() * (0.25 * gen.cpu().double())[:, None, None, None], src1.cpu().double() * s1], 1)
    ref = opatchify(full, p).reshape(ntok, F_)
    e = rel_l2(A[:, :F_].float().cpu(), ref)
    print(f"patchify_scaled {H}x{W} {dtype}: general per-sample scale vs fp64 {e:.2e}")
    assert e < (1e-6 if dtype == torch.float32 else 4e-3)
    for b_ in range(B):   # sample by sample: a factor taken from the wrong sample shows in that sample's rows
        rows = slice(b_ * ntok // B, (b_ + 1) * ntok // B)
        assert rel_l2(A[rows, :F_].float().cpu(), ref[rows]) < (1e-6 if dtype == torch.float32 else 4e-3), b_
