"""-m gpu: the non-linear epilogues fused into swiftk_gemm and swiftk_gemm_jvp (swift_amd/csrc/gemm.hip), called through the C ABI on
the exactly summable operands of tests/epilogue_reference.py and scored place by place: per element, per (row, head, q | k) vector
and per rn entry against fp64 closed forms on the EXACT accumulators, every word outside the written region against its prefill.
tests/test_epilogue_reference_cpu.py pins the closed forms to autograd / torch.func.jvp of the oracle's expressions, checks the
preconditions and that the table reaches every dispatch cell.  Every case prints each figure beside its bound; a failure names the
row, head, kind and column of the worst element.

A case whose k-loop is the ping-pong one runs a second time at tuning key 20 = 0 (one barrier per k-tile), the 352-wide ping-pong
SwiGLU case at tuning key 31 = 0, 1, 2, 3 with key 32 proving which instantiation ran: every run must leave the same bits as the first, which
is scored against fp64 (a run that differs is scored on its own and fails the comparison).

Measured on MI355X (worst over the cases of each entry; bound in brackets).  Everywhere: 0 words changed outside the written region
(pad columns, extra rows, rn past the last row, the v columns of the [q | k]-only form, the 32 pad columns of every SPLIT3 block, hm's
k-padding), 0 non-finite results, 0 linear elements off the exact bits (v columns and their tangents, SWIGLU_BOTH's C, the kept
pre-activation, rn == 1 for v), 0 words written by a refused call, every key-20 and key-31 rerun bit-equal to the first run.
  SWIGLU bf16          every element equal to the bf16-rounded fp64 value but the -96 gates' (fp64: a bf16 subnormal, the kernel: -0;
                       0.017 ulp at the 2^-102 floor) [1 ulp]; mismatch share <= 1.6e-5 [1e-3]
  SWIGLU fp32 out      1.13e-7 of the element's scale, the torch-fp32 restatement 1.13e-7 [8 x = 9.07e-7] (bf16 and fp32 operands, one-tile,
                       persistent and chunked alike)
  SWIGLU_BOTH C2       as SWIGLU bf16; share <= 1.5e-5 [1e-3]
  SWIGLU_BWD           dgate, dup <= 1.0 ulp at |d u|, |d g s| [1]; share 3.9e-5 / 5.6e-5 [1e-3]
  SWIGLU_SPLIT3        hi 5e-6 ulp, share 1.2e-5 [1, 1e-3]; hi + lo 7.3e-6 of the fp64 value [2^-16 = 1.53e-5]; block 2 = block 0
  QKNORM bf16          every element equal to the bf16-rounded fp64 value (0 ulp, share 0) [1, 1e-3]; worst q / k vector 3.2e-3 [2^-8 = 3.9e-3]
  QKNORM fp32          worst vector 1.9e-7 (fp32 operands), 1.7e-7 (bf16 operands, fp32 out) [1e-5]
  rn                   8.8e-8 per entry [1e-5]; the zero row 1e12 to 4.1e-9 [1e-5]
  QKNORM_JVP           primal rows as QKNORM bf16 (0 ulp, share 0; worst vector 3.1e-3); tangent <= 1.0 ulp at |f dv| + |f c v| [1], share
                       6.7e-5 [1e-3], worst tangent vector 2.8e-3 [3.9e-3]
  SWIGLU_JVP           silu(g) u as SWIGLU bf16 (share 2.4e-5); tangent 0.008 ulp at its scale [1], share 1.0e-4 [1e-3]
Every figure above is this module's measurement; the bounds are tests/test_gpu_backward_kernels.py's, with one addition that the
saturated gates force and tests/test_epilogue_reference_cpu.py demonstrates on the fp32 restatement: the bf16 ulp is taken no lower than at
2^-102 (the fp32 rule's TINY, for its reason).  At gate -96 with up = 16 the fp64 value is -3.1e-39, a non-zero bf16 subnormal, while
exp(96) is no finite fp32 number and any fp32 evaluation returns -0: 34 literal ulps for the restatement itself.
Nothing fails on the parent commit: no epilogue was found wrong and gemm.hip is unchanged.  What the tests notice was tried on mutated
copies of gemm.hip (not kept): tauB reading scale[vA / 3] (a head takes its neighbour's logit scale), the 16 j + 4 g4 < HD boundary moved by
one lane group, rn's row guard dropped, and SWIGLU_BOTH's silu returning NaN below gate -95 each fail tests here -- named by row, head,
kind and column; under the last two the earlier tests of the epilogue pass (test_gemm_qknorm_epilogue, test_qknorm_epilogue_rn_and_bwd;
test_gemm_swiglu_both_outputs, test_gemm_swiglu), the first two they notice too, at head_dim 88 only for the boundary.  (scale[vA / 3] -> scale[vB / 3] in tauA changes nothing: vA is even and a
multiple of 3 wherever tauA is read, so vB / 3 == vA / 3.)
"""
import pytest
import torch

import epilogue_reference as E
import exact_gemm as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from swift_amd import _lib
    assert _lib.lib().swiftk_get_tuning(2) == X.GRID   # the table's tile counts are placed against this grid
    assert _lib.lib().swiftk_get_tuning(0) == 1 and _lib.lib().swiftk_get_tuning(20) == 1
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def scratch(dev):
    return torch.empty(L().swiftk_gemm_chunk_scratch_bytes(), dtype=torch.uint8, device=dev)


def L():
    from swift_amd import _lib
    return _lib.lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def code(name):
    from swift_amd import _lib
    return _lib.BF16 if name == "bf16" else _lib.F32


def ptr(t):
    return None if t is None else t.data_ptr()


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def launch(c, inp, dev, scratch):
    """One call of the case's entry point on fresh sentinel-filled buffers: (return code, the buffers as raw bits on the CPU).  The
    operands must come back bit-identical."""
    from swift_amd import _lib
    tdt = torch.bfloat16 if c.dt == "bf16" else torch.float32
    a, w = inp["A"].to(dev).to(tdt), inp["W"].to(dev).to(tdt)
    a0, w0 = a.clone(), w.clone()
    b = {k: None if v is None else v.to(dev) for k, v in E.prefill(c).items()}
    C, C2, rn = b["C"], b["C2"], b["rn"]
    scale = inp["scale"].to(dev) if c.heads else None
    H = H0 = None
    common = (a.data_ptr(), c.lda, w.data_ptr(), c.lda)
    if c.paired:
        epi = _lib.EPI_QKNORM_JVP if c.epi == "qknorm_jvp" else _lib.EPI_SWIGLU_JVP
        rc = L().swiftk_gemm_jvp(*common, ptr(C), c.ldc, c.M, c.N, c.K, epi, ptr(scale), ptr(rn), c.hd, ptr(C2), c.ldc2, st())
    else:
        epi, ep0, ep1, pos_rows = {"swiglu": (_lib.EPI_SWIGLU, None, None, 0), "both": (_lib.EPI_SWIGLU_BOTH, None, ptr(C2), c.ldc2),
                                   "split3": (_lib.EPI_SWIGLU_SPLIT3, None, None, c.split3_block),
                                   "qknorm": (_lib.EPI_QKNORM, ptr(scale), ptr(rn), -c.hd if c.form == "qk_only" else c.hd),
                                   "bwd": (_lib.EPI_SWIGLU_BWD, None, None, c.ldh)}[c.epi]
        if c.epi == "bwd":
            H = torch.full((c.M, c.ldh), float("nan"), dtype=torch.bfloat16, device=dev)
            H[:, :2 * c.N] = inp["H"].to(dev).bfloat16()
            H0, ep1 = H.clone(), H.data_ptr()
        ldc = C.shape[1]
        args = (*common, C.data_ptr(), ldc, c.M, c.N, c.K, code(c.dt), code(c.out), epi, ep0, ep1, pos_rows)
        if c.chunk_k:
            rc = L().swiftk_gemm_chunked(*args, c.chunk_k, scratch.data_ptr(), scratch.numel(), st())
        else:
            rc = L().swiftk_gemm(*args, st())
    torch.cuda.synchronize()
    assert torch.equal(bits(a), bits(a0)) and torch.equal(bits(w), bits(w0)), "an operand changed"
    assert H is None or torch.equal(bits(H), bits(H0)), "the saved pre-activation changed"
    return rc, {k: None if v is None else v.cpu() for k, v in b.items()}


def same(b0, b1):
    return all((b0[k] is None and b1[k] is None) or torch.equal(b0[k], b1[k]) for k in b0)


def run_case(c, dev, scratch):
    """Every run of a case (see the module docstring): the first scored against fp64, the others bit-equal to it."""
    inp = E.inputs(c)
    cell = E.expected_cell(c)
    assert cell.rc == c.rc
    runs = [("", {})]
    if cell.kloop.startswith("pp"):
        runs.append(("key 20 = 0", {20: 0}))
    if c.key31:
        runs = [(f"key 31 = {arm}", {31: arm}) for arm in (0, 1, 2, 3)] + runs[1:]
    first, failed = None, []
    for tag, keys in runs:
        saved = {k: L().swiftk_get_tuning(k) for k in keys}
        try:
            for k, v in keys.items():
                assert L().swiftk_set_tuning(k, v) == 0 and L().swiftk_get_tuning(k) == v
            if c.key31:
                L().swiftk_set_tuning(32, 0)
            rc, b = launch(c, inp, dev, scratch)
            if c.key31 and 31 in keys:   # the instantiation the arm names ran, and no other
                assert L().swiftk_get_tuning(32) == 1 << keys[31], f"{tag} launched SL mask {L().swiftk_get_tuning(32):#x}"
        finally:
            for k, v in saved.items():
                L().swiftk_set_tuning(k, v)
        assert rc == c.rc, f"{c.epi} {c.name} [{c.cell}] {tag}: returned {rc}, the header's rules give {c.rc}; {cell}"
        print(f"--- {c.epi} {c.name} [{c.cell}] {tag} {cell.kernel} {cell.width} {cell.kloop} {cell.rounds}")
        if first is not None and same(first, b):   # (the same bits score the same)
            print("every buffer bit-equal to the first run's: the same figures")
            continue
        rep = E.score(c, inp, b)
        print(rep.text())
        failed += [f"{tag}: {line}" for line in rep.failed]
        if first is None:
            first = b
        else:
            failed.append(f"{tag}: the bits differ from the first run's")
    assert not failed, "\n".join(failed)


def cases(*epis):
    cs = E.cases(*epis)
    return pytest.mark.parametrize("c", cs, ids=E.ids(cs))


@cases("swiglu")
def test_swiglu_epilogue(dev, scratch, c):
    """SWIFTK_EPI_SWIGLU through the one-tile kernel (three type pairs), the persistent kernel at every width and k-loop, the four
    arms of tuning key 31, fp32 operands, swiftk_gemm_chunked, and a second epilogue per workgroup."""
    run_case(c, dev, scratch)


@cases("both")
def test_swiglu_both_epilogue(dev, scratch, c):
    """SWIFTK_EPI_SWIGLU_BOTH: the pre-activation bit for bit, silu(gate) * up per element; a ragged M is refused untouched."""
    run_case(c, dev, scratch)


@cases("bwd")
def test_swiglu_bwd_epilogue(dev, scratch, c):
    """SWIFTK_EPI_SWIGLU_BWD: both columns per element against the exact d(hidden) and the saved (gate, up), the ulp at |d u| and
    |d g s|; a ragged M is refused untouched."""
    run_case(c, dev, scratch)


@cases("split3")
def test_swiglu_split3_blocks(dev, scratch, c):
    """SWIFTK_EPI_SWIGLU_SPLIT3: [hi | lo | hi] with block 2 = block 0, hi per element, hi + lo within 2^-16, the pad columns of
    every block (32 behind the live ones) untouched."""
    run_case(c, dev, scratch)


@cases("qknorm")
def test_qknorm_epilogue(dev, scratch, c):
    """SWIFTK_EPI_QKNORM per element, per (row, head, q | k) vector and per rn entry: one-tile kernel (head_dim 88; 80 / 96 refused
    untouched), persistent kernel x head_dim x operand type x k-loop, rn given and NULL, the single-head and the [q | k]-only forms."""
    run_case(c, dev, scratch)


@cases("qknorm_jvp")
def test_qknorm_jvp_epilogue(dev, scratch, c):
    """SWIFTK_EPI_QKNORM_JVP: the primal rows as SWIFTK_EPI_QKNORM, the tangent rows per element (ulp at |f dv| + |f c v|) and per
    vector, v and its tangent bit for bit, rn given and NULL."""
    run_case(c, dev, scratch)


@cases("swiglu_jvp")
def test_swiglu_jvp_epilogue(dev, scratch, c):
    """SWIFTK_EPI_SWIGLU_JVP: silu(gate) * up and its tangent per element, the kept pre-activation bit for bit (on and off)."""
    run_case(c, dev, scratch)
