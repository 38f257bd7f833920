"""-m gpu: the forward ModulatedNorm + residual family, x += LN(y) (1 + scale_b) + shift_b, scored ROW BY ROW on hostile rows against
the fp64 reference of tests/modnorm_reference.py -- every entry point and every template instantiation behind it, called through the
C ABI, at B = 3 samples of 32 rows (two 16-row chunks each).  tests/test_modnorm_reference_cpu.py shows that a one-pass variance, a
missing eps, a neighbour's statistics or modulation, a dropped last slot or a padded divisor each miss these bars on the rows placed
here.

Bars (tests/modnorm_reference.py; none of them a new number):
  fp32 results   every row: row_err(kernel) <= max(4 x row_err(fp32 yardstick), 1e-5)       (test_gpu_tangent_kernels.py's rule)
  pair results   every element: |value - ref| <= 2^(E - 142) + max(4 x the yardstick's worst |error| of that row, 1e-5 max|ref row|),
                 and rel-L2 < 1e-5 over the tensor
  operand copies (xcopy, the split-3 blocks) bit-equal to the roundings of the kernel's own fp32 x

measured on MI355X, max|err| / max|ref| of a row, kernel | fp32 yardstick (for pairs: the yardstick stored as a (bf16, 8-bit) pair);
"on" = equal to two digits.  The 91 cases take 1.8 s.
  swiftk_modnorm_residual (chunked and row-per-wave, fp32 and bf16 y, nine widths; rows_per_sample 20 and 18)
      benign worst 1.3e-7 .. 2.4e-7 | 1.5e-7 .. 2.8e-7;  rows A B C D F G <= 1.8e-7 | <= 1.8e-7 (bar: the 1e-5 floor)
      row E 5.2e-8 .. 5.2e-6 | 5.2e-8 .. 5.2e-6, at most 1.29 x its yardstick (bar 1e-5 .. 2.1e-5)
  swiftk_modnorm_residual_split3 (d 520, 1544, 2048)
      benign worst 1.6e-7 .. 2.1e-7 | 1.6e-7 .. 2.0e-7;  row E 1.1e-7 .. 4.3e-6 | 8.6e-8 .. 4.3e-6;  the other rows <= 1.3e-7
  swiftk_modnorm_residual_pair
      row-per-wave kernel, 8-bit low part, seven widths, contiguous / strided / key 6 bit 2: every row on its yardstick -- benign worst
      1.3e-5 .. 2.3e-5, hostile rows 5.2e-7 .. 1.2e-5;  16-bit low part: benign worst 6.0e-6 .. 6.5e-6, hostile rows 5.2e-7 .. 6.6e-6
      packed kernel (d 1056 | 1280): on its yardstick (benign worst 2.1e-5 | 1.9e-5) but for row E, 1.7e-5 | 1.2e-5 against 8.1e-6 | 1.2e-5:
      2.04 x at d = 1056, where it forms the mean as sum x (1 / D) and the row-per-wave kernels and the yardstick as sum / D
  swiftk_modnorm_residual_pair_to (d 1056 | 1280)          the packed kernel's figures, row E included
  swiftk_modnorm_residual_pair_slabs, _pair_slabs_bf16 (d 520, 1056, 1544)
      8-bit: every row on its yardstick, benign worst 1.3e-5 .. 2.3e-5, hostile rows 8.5e-7 .. 1.3e-5;  16-bit: benign worst
      6.0e-6 .. 6.6e-6, hostile rows 9.0e-7 .. 6.6e-6 (0.3 .. 1.0 x the 8-bit yardstick)
  swiftk_modnorm_residual_pair_halves_bf16 (d 1056, 1280; tail NULL, rows_from 0 .. 96)
      on its yardstick (benign worst 1.7e-5 .. 2.1e-5, hostile rows 3.4e-6 .. 1.2e-5) but for row E: 8.8e-6 | 8.1e-6 (1.09 x) where the
      two-slab form takes it, 1.7e-5 | 8.1e-6 (2.04 x, d = 1056) where the one-y packed kernel does (rows_from > 31)
  swiftk_gemm_modnorm_residual_pair (32 | 64 rows per workgroup)
      every row on its yardstick: benign worst 1.9e-5 | 2.2e-5, zero rows 8.3e-6 .. 1.3e-5, x 2^7 rows 6.7e-6 .. 1.5e-5, x 2^-10 rows
      8.5e-6 .. 2.2e-5
No kernel misses a bar.
"""
import contextlib
import ctypes

import pytest
import torch

import modnorm_reference as mr
from conftest import rel_l2

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
EINVAL, ESHAPE = -1, -2
SENT = 7.0       # pad columns of 16- and 32-bit buffers
SENT8 = 77       # pad columns of a byte buffer
KEY = 6          # tuning key 6: bit 1 = chunked fp32-stream kernel, bit 2 = row-per-wave pair kernel instead of the packed one


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture
def key6():
    """``with key6(set_bits, clear_bits):`` launches under another value of tuning key 6 and puts the previous value back in a
    ``finally``.  Only launches go inside: every assertion runs after the key is restored, and the fixture checks on its way out that
    the key is what it was before the test."""
    from swift_amd import _lib
    L = _lib.lib()
    before = L.swiftk_get_tuning(KEY)

    @contextlib.contextmanager
    def changed(set_bits=0, clear_bits=0):
        prev = L.swiftk_get_tuning(KEY)
        L.swiftk_set_tuning(KEY, (prev | set_bits) & ~clear_bits)
        try:
            yield
        finally:
            L.swiftk_set_tuning(KEY, prev)

    yield changed
    assert L.swiftk_get_tuning(KEY) == before


def rnd(shape, seed, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * std


def s():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    """The raw words of a tensor (compares NaN-poisoned buffers and signed zeros bit for bit)."""
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else (torch.int32 if t.element_size() == 4 else torch.uint8))


def padded(t, ld, dev, dtype=None, fill=SENT):
    """[M, d] CPU tensor -> device [M, ld] of ``dtype`` with ``fill`` in the pad columns."""
    out = torch.full((t.shape[0], ld), fill, dtype=dtype or t.dtype, device=dev)
    out[:, :t.shape[1]] = t.to(dev).to(out.dtype)
    return out


# ------------------------------------------------------------------------------------------------- cases, references, scoring

_CASES, _REFS = {}, {}


def cpu_case(d, bf16_y=True, rps=32, B=3):
    k = (d, bf16_y, rps, B)
    if k not in _CASES:
        _CASES[k] = mr.make_forward_case(d, mr.CASE_SEED, bf16_y, rps, B)
    return _CASES[k]


def scored(key, c, x_in=None, y=None):
    """(fp64 reference, fp32 yardstick) of case ``c`` with x / y replaced by what the kernel really starts from; computed once per
    ``key`` and shared (never written to)."""
    a = mr.forward_args(c)
    if x_in is not None:
        a["x"] = x_in
    if y is not None:
        a["y"] = y
    if key not in _REFS:
        _REFS[key] = (mr.modnorm_forward(**a), mr.modnorm_forward(**a, dtype=torch.float32), a["x"].clone(), a["y"].clone())
    ref, yard, x0, y0 = _REFS[key]
    assert torch.equal(bits(x0), bits(a["x"])) and torch.equal(bits(y0), bits(a["y"])), key
    return ref, yard


def modulation(c, dev):
    """The case's mod as the [2d : 4d] column slice of a [B, 6d] tensor (a strided slice, like one layer of the concatenated
    modulation)."""
    B, d2 = c["mod"].shape
    wide = rnd((B, 3 * d2), 5).to(dev)
    wide[:, d2: 2 * d2] = c["mod"].to(dev)
    return wide[:, d2: 2 * d2]


def report(entry, tag, kern, yard, hostile):
    benign = [r for r in range(kern.shape[0]) if r not in hostile]
    print(f"{entry} | {tag} | benign worst | kernel {float(kern[benign].max()):.2e} | yardstick {float(yard[benign].max()):.2e}")
    for r, kind in sorted(hostile.items()):
        print(f"{entry} | {tag} | row {r} {kind} | kernel {float(kern[r]):.2e} | yardstick {float(yard[r]):.2e}")


def check_f32(entry, tag, got, ref, yard, hostile):
    """Every row of an fp32 result against max(4 x yardstick, 1e-5)."""
    got = got.cpu()
    errs, yerrs = mr.row_errs(got, ref), mr.row_errs(yard, ref)
    report(entry, tag, errs, yerrs, hostile)
    bar = mr.f32_row_bar(yard, ref)
    bad = [(r, hostile.get(r, "benign"), float(errs[r]), float(bar[r])) for r in range(ref.shape[0]) if not float(errs[r]) <= float(bar[r])]
    assert not bad, (entry, tag, bad)
    assert rel_l2(got, ref) < mr.F32_TOL


def check_pair(entry, tag, hi, lo, d, ref, yard, hostile):
    """Every element of a pair result against one byte step + max(4 x the yardstick's worst of the row, 1e-5 max|ref row|); printed
    beside the error of the yardstick stored as a (bf16, 8-bit) pair."""
    from swift_amd import ops
    value = ops.pair_value(hi, lo[:, :d], d).cpu()
    errs, yerrs = mr.row_errs(value, ref), mr.row_errs(mr.pair_quantise(yard), ref)
    report(entry, tag, errs, yerrs, hostile)
    excess = mr.pair_excess(value, hi[:, :d].cpu(), yard, ref)
    bad = [(r, hostile.get(r, "benign"), float(excess[r])) for r in range(ref.shape[0]) if not float(excess[r]) <= 1.0]
    assert not bad, (entry, tag, bad)
    assert rel_l2(value, ref) < 1e-5
    return value


def make_pair(dev, c, lo_bits, strided_lo=False):
    """The pair of the case's x from swiftk_split_pair: hi [M, k_pad(d) + 8] with SENT in the pad columns, lo [M, d] (``strided_lo``:
    [M, d + 8] with pad sentinels); and the fp32 value the pair holds (CPU), which is what the references start from."""
    from swift_amd import ops
    M, d = c["x"].shape
    ldh = ops.k_pad(BF, d) + 8
    hi, lo = ops.split_pair(c["x"].to(dev), ldh, lo_bits)
    hi[:, d:] = SENT
    x_in = ops.pair_value(hi, lo, d).cpu()
    assert torch.equal(x_in[mr.ZERO_X_ROW], torch.zeros(d))
    if lo_bits == 8:  # the kernel's split is the pair tests/tangent_reference.py describes
        assert torch.equal(x_in, mr.pair_quantise(c["x"]))
    if strided_lo:
        wide = torch.full((M, d + 8), SENT8 if lo_bits == 8 else SENT, dtype=lo.dtype, device=dev)
        wide[:, :d] = lo
        lo = wide
    return hi, lo, x_in, ldh


def pads_intact(t, d, fill=SENT):
    return bool((t[:, d:].float() == float(fill)).all())


# ------------------------------------------------------------------------------------------ (a) swiftk_modnorm_residual

def run_residual(dev, key6, c, ydt, chunked):
    from swift_amd import _lib
    L = _lib.lib()
    M, d = c["y"].shape
    y, x = c["y"].to(dev).to(ydt), c["x"].to(dev).clone()
    ldc = d + 8
    xc = torch.full((M, ldc), SENT, dtype=ydt, device=dev)
    g, b, msl = c["gamma"].to(dev), c["beta"].to(dev), modulation(c, dev)
    with key6(set_bits=2 if chunked else 0, clear_bits=0 if chunked else 2):
        rc = L.swiftk_modnorm_residual(y.data_ptr(), d, x.data_ptr(), xc.data_ptr(), ldc, g.data_ptr(), b.data_ptr(), msl.data_ptr(),
                                       msl.stride(0), M, d, c["rows_per_sample"], 1e-6, _lib.BF16 if ydt == BF else _lib.F32, s())
        torch.cuda.synchronize()
    return rc, x, xc


@pytest.mark.parametrize("kernel", ["chunked", "row_per_wave"])
@pytest.mark.parametrize("ydt", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("d", [8, 64, 512, 520, 1056, 1280, 1536, 1544, 2048])
def test_residual_rows(dev, key6, d, ydt, kernel):
    """swiftk_modnorm_residual: modnorm_chunk_kernel<T, 3 | 4> (tuning key 6 bit 1) and modnorm_kernel<T, 3 | 4>, T = float | bf16;
    d = 8 is one live lane, 512 exactly one slot, 520 one lane into the second, 1544 / 2048 the four-slot forms.  xcopy has
    ldc = d + 8 with sentinel pad columns, mod is a strided slice."""
    c = cpu_case(d, bf16_y=ydt == BF)
    rc, x, xc = run_residual(dev, key6, c, ydt, kernel == "chunked")
    assert rc == 0
    ref, yard = scored(("stream", d, ydt), c)
    check_f32("modnorm_residual", f"{kernel} {'bf16' if ydt == BF else 'f32'} d{d}", x, ref, yard, c["hostile"])
    assert torch.equal(bits(xc[:, :d]), bits(x.to(ydt)))   # the operand copy IS the rounding of the kernel's own x
    assert pads_intact(xc, d)


@pytest.mark.parametrize("ydt", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("d", [64, 1544])
@pytest.mark.parametrize("rps,B", [(20, 4), (18, 4)])
def test_residual_sample_boundary_off_the_chunk(dev, key6, rps, B, d, ydt):
    """rows_per_sample no multiple of the 16-row chunk: modnorm_kernel runs whatever key 6 bit 1 says.  20 x 4 (M = 80) puts the sample
    boundaries inside a 16-row chunk but on the row-per-wave kernel's four-row workgroups (20 = 5 x 4); 18 x 4 (M = 72) puts them
    inside those too (rows 16, 17 | 18, 19 share a workgroup).  A hostile row on each side of the first boundary."""
    c = cpu_case(d, bf16_y=ydt == BF, rps=rps, B=B)
    assert c["hostile"][rps - 1] == "E" and c["hostile"][rps] == "F"
    ref, yard = scored(("stream", rps, B, d, ydt), c)
    for chunked in (True, False):
        rc, x, xc = run_residual(dev, key6, c, ydt, chunked)
        assert rc == 0
        check_f32("modnorm_residual", f"rps{rps} key6.bit1={int(chunked)} {'bf16' if ydt == BF else 'f32'} d{d}", x, ref, yard, c["hostile"])
        assert torch.equal(bits(xc[:, :d]), bits(x.to(ydt))) and pads_intact(xc, d)


@pytest.mark.parametrize("d", [2056, 12])
def test_residual_refuses_widths_it_cannot_run(dev, d):
    """d > 2048 and d % 8 != 0: SWIFTK_ESHAPE, nothing written."""
    from swift_amd import _lib
    L = _lib.lib()
    M = 96
    y, x = rnd((M, d), 1).to(dev), rnd((M, d), 2).to(dev)
    xc = torch.full((M, d + 4), SENT, device=dev)
    x0 = x.clone()
    g, mod = torch.ones(d, device=dev), torch.zeros(3, 2 * d, device=dev)
    for dt, yy in ((_lib.F32, y), (_lib.BF16, y.to(BF))):
        rc = L.swiftk_modnorm_residual(yy.data_ptr(), d, x.data_ptr(), xc.data_ptr(), d + 4, g.data_ptr(), g.data_ptr(), mod.data_ptr(), 2 * d, M, d,
                                       32, 1e-6, dt, s())
        torch.cuda.synchronize()
        assert rc == ESHAPE
        assert torch.equal(bits(x), bits(x0)) and bool((xc == SENT).all())


# ----------------------------------------------------------------------------------- (b) swiftk_modnorm_residual_split3

@pytest.mark.parametrize("d", [520, 1544, 2048])
def test_residual_split3_rows(dev, key6, d):
    """swiftk_modnorm_residual_split3: modnorm_chunk_kernel<float, 3> (d = 520) and <float, 4> (1544, 2048) with the operand blocks.
    x against the bars; xcopy bit-equal to x; the blocks [hi | lo | hi] bit-equal to bf16(x), bf16(x - hi), bf16(x) of the kernel's
    own x with zeroed k-padding; and everything bit for bit what swiftk_modnorm_residual + swiftk_split3 give."""
    from swift_amd import _lib, ops
    L = _lib.lib()
    c = cpu_case(d, bf16_y=False)
    M = c["y"].shape[0]
    rps = c["rows_per_sample"]
    y = c["y"].to(dev)
    g, b, msl = c["gamma"].to(dev), c["beta"].to(dev), modulation(c, dev)
    ldc, ld3 = d + 8, ops.k_pad(BF, 3 * d)
    if ld3 == 3 * d:
        ld3 += 64
    xa, xb = c["x"].to(dev).clone(), c["x"].to(dev).clone()
    ca, cb = (torch.full((M, ldc), SENT, device=dev) for _ in range(2))
    a3, b3 = (torch.full((M, ld3), SENT, dtype=BF, device=dev) for _ in range(2))
    with key6(set_bits=2):
        rc = L.swiftk_modnorm_residual_split3(y.data_ptr(), d, xb.data_ptr(), cb.data_ptr(), ldc, b3.data_ptr(), ld3, g.data_ptr(), b.data_ptr(),
                                              msl.data_ptr(), msl.stride(0), M, d, rps, 1e-6, s())
        rc_a = L.swiftk_modnorm_residual(y.data_ptr(), d, xa.data_ptr(), ca.data_ptr(), ldc, g.data_ptr(), b.data_ptr(), msl.data_ptr(),
                                         msl.stride(0), M, d, rps, 1e-6, _lib.F32, s())
        torch.cuda.synchronize()
    assert rc == 0 and rc_a == 0
    rc_s = L.swiftk_split3(ca.data_ptr(), ldc, a3.data_ptr(), ld3, M, d, 0, s())
    torch.cuda.synchronize()
    assert rc_s == 0
    ref, yard = scored(("stream", d, torch.float32), c)
    check_f32("modnorm_residual_split3", f"d{d}", xb, ref, yard, c["hostile"])
    assert torch.equal(bits(cb[:, :d]), bits(xb)) and pads_intact(cb, d)
    hi = xb.to(BF)
    assert torch.equal(bits(b3[:, :d]), bits(hi)) and torch.equal(bits(b3[:, 2 * d: 3 * d]), bits(hi))
    assert torch.equal(bits(b3[:, d: 2 * d]), bits((xb - hi.float()).to(BF)))
    assert bool((b3[:, 3 * d:].float() == 0).all())
    # the two-kernel path
    assert torch.equal(bits(xa), bits(xb)) and torch.equal(bits(ca), bits(cb))
    assert torch.equal(bits(a3[:, :3 * d]), bits(b3[:, :3 * d]))


# -------------------------------------------------------------------------------------- (c) swiftk_modnorm_residual_pair

def run_pair(dev, key6, c, lo_bits, mode):
    """One swiftk_modnorm_residual_pair call.  mode "plain": contiguous y / lo (d = 1056 / 1280 with the 8-bit low part: the packed
    kernel); "key": the same with key 6 bit 2 (the row-per-wave kernel); "strided": ldy = ldl = d + 8, which the packed kernel does
    not take."""
    from swift_amd import _lib
    L = _lib.lib()
    M, d = c["y"].shape
    strided = mode == "strided"
    hi, lo, x_in, ldh = make_pair(dev, c, lo_bits, strided_lo=strided)
    y = padded(c["y"], d + 8 if strided else d, dev, BF)
    g, b, msl = c["gamma"].to(dev), c["beta"].to(dev), modulation(c, dev)
    with key6(set_bits=4 if mode == "key" else 0, clear_bits=0 if mode == "key" else 4):
        rc = L.swiftk_modnorm_residual_pair(y.data_ptr(), y.stride(0), hi.data_ptr(), ldh, lo.data_ptr(), lo.stride(0), lo_bits, g.data_ptr(),
                                            b.data_ptr(), msl.data_ptr(), msl.stride(0), M, d, c["rows_per_sample"], 1e-6, s())
        torch.cuda.synchronize()
    return rc, hi, lo, x_in, y


@pytest.mark.parametrize("lo_bits", [8, 16])
@pytest.mark.parametrize("d", [8, 520, 1056, 1280, 1536, 1544, 2048])
def test_pair_rows(dev, key6, d, lo_bits):
    """swiftk_modnorm_residual_pair: modnorm_pair_kernel<3 | 4, LO8, 0> (d <= 1536 | above) and, at d = 1056 / 1280 with the 8-bit low
    part, modnorm_pair_packed_kernel<132 | 160>.  There the packed kernel, the row-per-wave kernel behind key 6 bit 2 and the
    row-per-wave kernel reached by strides are each held to the bars on their own, then compared with each other; elsewhere the
    contiguous and the strided call are the same kernel and must agree bit for bit."""
    from swift_amd import ops
    c = cpu_case(d)
    packed = lo_bits == 8 and d in (1056, 1280)
    out = {}
    for mode in ("plain", "strided") + (("key",) if packed else ()):
        rc, hi, lo, x_in, y = run_pair(dev, key6, c, lo_bits, mode)
        assert rc == 0
        ref, yard = scored(("pair", d, lo_bits), c, x_in)
        kern = "packed" if packed and mode == "plain" else "row_per_wave"
        value = check_pair("modnorm_residual_pair", f"{kern} ({mode}) lo{lo_bits} d{d}", hi, lo, d, ref, yard, c["hostile"])
        assert pads_intact(hi, d) and pads_intact(y, d)
        if mode == "strided":
            assert pads_intact(lo, d, SENT8 if lo_bits == 8 else SENT)
        out[mode] = (hi[:, :d], lo[:, :d], value)
    same = ("key", "strided") if packed else ("plain", "strided")   # one kernel, one order of operations
    assert torch.equal(bits(out[same[0]][0]), bits(out[same[1]][0])) and torch.equal(bits(out[same[0]][1]), bits(out[same[1]][1]))
    if packed:
        # (same formulas; the row sums associate differently, so a few last bits of the statistics may differ: the figures of
        # tests/test_gpu_kernels.py::test_modnorm_residual_pair)
        # -- figures taken on benign rows, so compared on the benign rows here: the two kernels form the mean differently (sum x (1 / D)
        # against sum / D), which on row E is an ulp of 63.6 against a spread of 0.125; every hostile row is scored on its own above
        benign = [r for r in range(c["y"].shape[0]) if r not in c["hostile"]]
        assert float((out["plain"][0][benign] != out["key"][0][benign]).float().mean()) < 1e-3
        assert rel_l2(out["plain"][2][benign], out["key"][2][benign]) < 2e-6
    # against the fp32-stream kernel on the same x: not a bar (both are scored above), the existing cross-check
    xd = x_in.to(dev).clone()
    ops.modnorm_residual(c["y"].to(dev).to(BF), xd, c["gamma"].to(dev), c["beta"].to(dev), c["mod"].to(dev), c["rows_per_sample"])
    assert rel_l2(out["plain"][2], xd.cpu()) < 1e-5


# ----------------------------------------------------------------------------------- (d) swiftk_modnorm_residual_pair_to

@pytest.mark.parametrize("d", [1056, 1280])
def test_pair_to_rows(dev, key6, d):
    """swiftk_modnorm_residual_pair_to (modnorm_pair_packed_kernel<132 | 160> with xh_out != xh): the output against the bars -- not
    against the in-place call -- and the input hi unchanged."""
    from swift_amd import _lib
    L = _lib.lib()
    c = cpu_case(d)
    M = c["y"].shape[0]
    hi_in, lo, x_in, ldh = make_pair(dev, c, 8)
    keep = hi_in.clone()
    hi_out = torch.full((M, ldh), SENT, dtype=BF, device=dev)
    hi_out[:, :d] = float("nan")
    y = c["y"].to(dev).to(BF)
    g, b, msl = c["gamma"].to(dev), c["beta"].to(dev), modulation(c, dev)
    with key6(clear_bits=4):
        rc = L.swiftk_modnorm_residual_pair_to(y.data_ptr(), d, hi_in.data_ptr(), hi_out.data_ptr(), ldh, lo.data_ptr(), d, 8, g.data_ptr(),
                                               b.data_ptr(), msl.data_ptr(), msl.stride(0), M, d, c["rows_per_sample"], 1e-6, s())
        torch.cuda.synchronize()
    assert rc == 0
    ref, yard = scored(("pair", d, 8), c, x_in)
    check_pair("modnorm_residual_pair_to", f"packed d{d}", hi_out, lo, d, ref, yard, c["hostile"])
    assert torch.equal(bits(hi_in), bits(keep)) and pads_intact(hi_out, d)


# ------------------------------------------------------------- (e) swiftk_modnorm_residual_pair_slabs / _pair_slabs_bf16

def two_addends(y):
    """y as two addends of opposite sign and comparable size: s0 = y + t, s1 = -t, t = sign(y) 2^floor(log2 |y|) (1 where y = 0).
    For bf16-representable y the fp32 sum s0 + s1 is y again, exactly; a kernel that reads one slab twice sees 2 (y + t) or -2 t,
    neither of which normalises to anything like LN(y)."""
    t = torch.where(y == 0, torch.ones_like(y), torch.sign(y) * torch.exp2(torch.floor(torch.log2(y.abs().clamp_min(1e-30)))))
    return y + t, -t


@pytest.mark.parametrize("lo_bits", [8, 16])
@pytest.mark.parametrize("d", [520, 1056, 1544])
@pytest.mark.parametrize("form", ["f32", "bf16"])
def test_pair_slabs_rows(dev, key6, form, d, lo_bits):
    """swiftk_modnorm_residual_pair_slabs (modnorm_pair_kernel<3 | 4, LO8, 1>) and _pair_slabs_bf16 (<3 | 4, LO8, 2>) on hand-made
    slabs.  The reference is the fp64 reference on slab0.float() + slab1.float() formed in fp32, as the kernel forms it: for the fp32
    slabs that is the hostile y itself, for the bf16 slabs (addends rounded to bf16 first) y up to a last bit."""
    from swift_amd import _lib
    L = _lib.lib()
    c = cpu_case(d)
    M = c["y"].shape[0]
    s0, s1 = two_addends(c["y"])
    if form == "bf16":
        s0, s1 = mr.bf16_round(s0), mr.bf16_round(s1)
    ysum = s0 + s1   # (fp32)
    if form == "f32":
        assert torch.equal(ysum, c["y"])
    assert float((2 * s0 - c["y"]).abs().max() / c["y"].abs().max()) > 0.5   # one slab read twice is another y altogether
    slabs = torch.stack([s0, s1]).to(dev).to(BF if form == "bf16" else torch.float32).contiguous()
    hi, lo, x_in, ldh = make_pair(dev, c, lo_bits)
    g, b, msl = c["gamma"].to(dev), c["beta"].to(dev), modulation(c, dev)
    fn = L.swiftk_modnorm_residual_pair_slabs_bf16 if form == "bf16" else L.swiftk_modnorm_residual_pair_slabs
    rc = fn(slabs.data_ptr(), d, M * d, hi.data_ptr(), ldh, lo.data_ptr(), d, lo_bits, g.data_ptr(), b.data_ptr(), msl.data_ptr(), msl.stride(0),
            M, d, c["rows_per_sample"], 1e-6, s())
    torch.cuda.synchronize()
    assert rc == 0
    ref, yard = scored(("slabs", form, d, lo_bits), c, x_in, ysum)
    check_pair("modnorm_residual_pair_slabs" + ("_bf16" if form == "bf16" else ""), f"lo{lo_bits} d{d}", hi, lo, d, ref, yard, c["hostile"])
    assert pads_intact(hi, d)


# --------------------------------------------------------------------------- (f) swiftk_modnorm_residual_pair_halves_bf16

@pytest.mark.parametrize("rows_from", [None, 0, 16, 48, 64, 96], ids=lambda v: "null" if v is None else f"from{v}")
@pytest.mark.parametrize("d", [1056, 1280])
def test_pair_halves_rows(dev, d, rows_from):
    """swiftk_modnorm_residual_pair_halves_bf16: modnorm_pair_packed_kernel<132 | 160, true> from ``rows_from`` on and the one-y kernel
    below it.  tail = NULL and (rows_from, 0, 8) with rows_from a chunk boundary inside a sample (16, 48), a sample boundary (64)
    and the extremes (0: no one-y launch; 96: no two-slab launch).  Slab 1 is NaN below rows_from.  The reference is the fp64
    reference on bf16(slab 0 + slab 1) -- not another kernel."""
    from swift_amd import _lib
    L = _lib.lib()
    c = cpu_case(d)
    M = c["y"].shape[0]
    rf = 0 if rows_from is None else rows_from
    s0, s1 = two_addends(c["y"])
    s0, s1 = mr.bf16_round(s0), mr.bf16_round(s1)
    yref = mr.bf16_round(s0 + s1)
    s0[:rf], s1[:rf], yref[:rf] = c["y"][:rf], float("nan"), c["y"][:rf]
    slabs = torch.stack([s0, s1]).to(dev).to(BF).contiguous()
    hi, lo, x_in, ldh = make_pair(dev, c, 8)
    g, b, msl = c["gamma"].to(dev), c["beta"].to(dev), modulation(c, dev)
    tail = None if rows_from is None else (ctypes.c_int64 * 3)(rows_from, 0, 8)
    rc = L.swiftk_modnorm_residual_pair_halves_bf16(slabs.data_ptr(), M * d, tail, hi.data_ptr(), ldh, lo.data_ptr(), g.data_ptr(), b.data_ptr(),
                                                    msl.data_ptr(), msl.stride(0), M, d, c["rows_per_sample"], 1e-6, s())
    torch.cuda.synchronize()
    assert rc == 0
    ref, yard = scored(("halves", d, rf), c, x_in, yref)
    check_pair("modnorm_residual_pair_halves_bf16", f"{'tail null' if rows_from is None else f'rows_from {rows_from}'} d{d}", hi, lo, d, ref, yard,
               c["hostile"])
    assert pads_intact(hi, d)


# --------------------------------------------------------------------------------- (g) swiftk_gemm_modnorm_residual_pair

@pytest.mark.parametrize("rows", [32, 64])
def test_gemm_modnorm_rows(dev, rows):
    """swiftk_gemm_modnorm_residual_pair (gemm_rownorm_kernel<11, 2 | 4>), d = 1056, K = 64.  A has zero rows (their y is constant 0),
    rows scaled by 2^7 and rows scaled by 2^-10 (variance about eps) at the case builder's places; the reference is the fp64 reference
    on swiftk_gemm's bf16 y.  (The entry wants rows_per_sample to be a multiple of the rows of a workgroup: 32 rows per sample at 32,
    64 at 64 -- the places move with the sample boundary.)"""
    from swift_amd import ops
    d, K, B, rps = 1056, 64, 3, rows
    c = dict(cpu_case(d, rps=rps, B=B))
    M = B * rps
    a, w = rnd((M, K), 61), rnd((d, K), 62, 0.25)
    hostile = {}
    for i, r in enumerate(sorted(mr.hostile_rows(rps, M))):
        kind = ("zero", "x2^7", "x2^-10")[i % 3]
        a[r] *= {"zero": 0.0, "x2^7": 128.0, "x2^-10": 2.0 ** -10}[kind]
        hostile[r] = kind
    ad, wd = a.to(dev).to(BF), w.to(dev).to(BF)
    y = ops.gemm(ad, wd).float().cpu()
    assert y.shape == (M, d) and float(y[1].abs().max()) == 0.0 and float(y[6].abs().max()) > 100 and float(y[11].abs().max()) < 2e-2
    hi, lo, x_in, ldh = make_pair(dev, c, 8)
    ops.gemm_modnorm_residual_pair(ad, wd, hi, lo, c["gamma"].to(dev), c["beta"].to(dev), modulation(c, dev), rps, d, k=K, rows_per_workgroup=rows)
    torch.cuda.synchronize()
    ref, yard = scored(("rownorm", rows), c, x_in, y)
    check_pair("gemm_modnorm_residual_pair", f"{rows} rows per workgroup", hi, lo, d, ref, yard, hostile)
    assert pads_intact(hi, d)
