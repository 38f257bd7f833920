"""-m gpu: the window-attention tangent kernels on random operands, judged per (sample, window, head) item, in both storage types.

swiftk_window_attention_jvp is called through the C ABI on the operands of tests/tangent_attention_reference.py (q-hat of norm tau in
{1, 10, 47, 100} across the heads, unit k-hat, v ~ N(0, 1), tangents 0.3 N(0, 1); rows wider than their content, NaN in the operand
pad) over its three cases -- 6 items in the plain block order, 16 and 8 in the remapped one, head_dim 80 / 88 / 96 -- and four
variants each: all three tangents, then dq, dk, dv alone (the dv term is 1 % of the tangent on the tau = 100 heads and would hide a
fault there under the other two).  Both outputs arrive full of the NaN pattern of exact_attention.sent; pad columns and the extra
row must keep it, bit for bit.

Bounds.  bf16: every item within 2 x its head's yardstick = the larger worst-item error against fp64 of the plain restatement of the
kernel's documented arithmetic (A) and of the autocast form (B), computed here on the CPU before the launch.  fp32: every item within
F32_TOL = 1e-5; the ratio to the fp32 restatement (C) is printed.  Conditions asserted before any launch: bf16 tangent yardsticks
<= 1.5e-2, fp32 ones <= 5e-6.  tests/test_tangent_attention_reference_cpu.py shows three faults, each in one item of the 96-item
problem of test_window_attention_jvp_kernel, that pass that test's global 1e-2 / 2e-2 and fail this rule at 23 x .. 374 x.
Two invariants on the launches of the "all" variant, bit for bit: the primal output is the same with zero, random and 4 x tangents;
4 x the tangent operands gives 4 x the tangent output.

Measured on MI355X (worst over the 12 case-variants of a storage type; bound in brackets):
  bf16  yardsticks per head: primal 2.0e-3 .. 2.5e-3, tangent 2.0e-3 .. 7.1e-3 (tau 1 .. 100; 2.0e-3 .. 2.6e-3 with dv alone) [1.5e-2];
        worst item / yardstick: primal 0.945, tangent 1.001 [2]; medians primal 0.79 .. 0.91, tangent 0.80 .. 1.00 -- the kernel's items
        sit ON the restatement's worst item of their head
  fp32  worst item: primal 9.2e-7 .. 1.4e-6, tangent 9.3e-7 .. 3.5e-6 [1e-5]; restatement C per head 2.1e-7 .. 3.0e-6 [5e-6];
        worst item / restatement 1.24 .. 1.42, medians 1.04 .. 1.12 (printed, not asserted)
  both  the invariants hold bit for bit in all six (case, storage type) pairs; every refusal returns its code with both outputs
        untouched
No test of this module fails on the parent commit: neither attention tangent kernel showed a defect.
"""
import pytest
import torch

import exact_attention as X
import tangent_attention_reference as ta

pytestmark = pytest.mark.gpu

EINVAL, ESHAPE, EALIGN = -1, -2, -3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def st():
    return torch.cuda.current_stream().cuda_stream


def L():
    from swift_amd import _lib
    return _lib.lib()


def code(f32):
    from swift_amd import _lib
    return _lib.F32 if f32 else _lib.BF16


def tdt(f32):
    return torch.float32 if f32 else torch.bfloat16


def name(f32):
    return "fp32" if f32 else "bf16"


def strides(c):
    """(ldq, ldo): both larger than the widths, rows still on the kernels' 16-byte (operands) and 8-byte (bf16 outputs) boundaries."""
    return 3 * c.dim + 8, c.dim + 4


def padded_operand(c, x, f32, dev):
    rows, ldq = c.B * c.n, strides(c)[0]
    buf = torch.full((rows, ldq), float("nan"))
    buf[:, :3 * c.dim] = x.reshape(rows, -1)
    return buf.to(tdt(f32)).to(dev)


def launch(c, qkv, dqkv, f32, dev):
    """One call on sentinel-filled outputs; checks everything outside the result bit for bit and returns the window-order
    (out, dout) as fp32 CPU tensors together with the raw result bits [rows, dim] of both."""
    rows, (ldq, ldo) = c.B * c.n, strides(c)
    out, dout = X.sent((rows + 1, ldo), f32, dev), X.sent((rows + 1, ldo), f32, dev)
    rc = L().swiftk_window_attention_jvp(qkv.data_ptr(), dqkv.data_ptr(), ldq, out.data_ptr(), dout.data_ptr(), ldo, c.B, c.grid[0], c.grid[1],
                                         c.heads, c.hd, c.shift[0], c.shift[1], code(f32), st())
    assert rc == 0
    torch.cuda.synchronize()
    res = []
    for what, buf in (("primal", out), ("tangent", dout)):
        g = buf.cpu()
        want = X.sent((rows + 1, ldo), f32)
        want[:rows, :c.dim] = g[:rows, :c.dim]
        assert torch.equal(g, want), f"{c.name} {name(f32)} {what} output: a pad column or the extra row was written"
        inner = g[:rows, :c.dim].contiguous()
        val = inner.view(tdt(f32)).float()
        assert bool(torch.isfinite(val).all()), f"{c.name} {name(f32)} {what} output: a result element was not written (or is not finite)"
        res += [ta.windows(c, val.view(c.B, c.n, c.dim)), inner]
    return res[0], res[2], res[1], res[3]


def score(c, tag, what, got, ref, yard, f32):
    err = ta.item_rel_l2(got, ref)                                   # [B, nW, H]
    ratio = err / yard
    w = int(ratio.flatten().argmax())
    head = w % c.heads
    if f32:
        print(f"{tag} {what}: worst item {float(err.max()):.2e} (bound {ta.F32_TOL:.0e}); fp32 restatement per head {float(yard.min()):.2e} .. "
              f"{float(yard.max()):.2e}; worst item / restatement {float(ratio.max()):.2f}, median {float(ratio.median()):.2f}")
        assert float(err.max()) <= ta.F32_TOL, f"{tag} {what}: item {w} (sample, window, head; heads fastest) at {float(err.max()):.2e}"
    else:
        print(f"{tag} {what}: yardstick per head {float(yard.min()):.2e} .. {float(yard.max()):.2e}; item errors {float(err.min()):.2e} .. "
              f"{float(err.max()):.2e}; worst item / yardstick {float(ratio.max()):.3f} (item {w // c.heads}, head {head}, tau "
              f"{float(ta.taus(c)[head]):g}; bound {ta.FACTOR:g}), median {float(ratio.median()):.3f}")
        assert float(ratio.max()) <= ta.FACTOR, f"{tag} {what}: item {w} (sample, window, head; heads fastest) at {float(ratio.max()):.2f} x the yardstick"


RUNS = [(c, f32, only) for c in ta.CASES for f32 in (False, True) for only in ta.VARIANTS]


@pytest.mark.parametrize("c,f32,only", RUNS, ids=[f"{c.name}-{name(f32)}-{only}" for c, f32, only in RUNS])
def test_tangent_attention_per_item(dev, c, f32, only):
    """See the module docstring.  Measured on MI355X: there."""
    r = ta.reference(c, f32, only)
    # the conditions the bounds rest on, before any launch
    assert float(r["yard_dout"].max()) <= (ta.F32_YARD_CAP if f32 else ta.BF16_YARD_CAP)
    qkv, dqkv = padded_operand(c, r["qkv"], f32, dev), padded_operand(c, r["dqkv"], f32, dev)
    out, dout, out_bits, dout_bits = launch(c, qkv, dqkv, f32, dev)
    tag = f"attention tangent {name(f32)} {c.name} (head_dim {c.hd}, {c.items} items) [{only}]"
    score(c, tag, "primal", out, r["out"], r["yard_out"], f32)
    score(c, tag, "tangent", dout, r["dout"], r["yard_dout"], f32)
    if only != "all":
        return
    # the primal output does not see the tangent operands; a power of two passes every rounding of the tangent unchanged
    zero = padded_operand(c, torch.zeros_like(r["dqkv"]), f32, dev)
    _, dout0, out_bits0, _ = launch(c, qkv, zero, f32, dev)
    assert torch.equal(out_bits0, out_bits), f"{tag}: the primal output changed with the tangent operands (zero tangents)"
    assert float(dout0.abs().max()) == 0.0, f"{tag}: zero tangent operands gave a nonzero tangent"
    four = padded_operand(c, 4.0 * r["dqkv"], f32, dev)
    _, dout4, out_bits4, _ = launch(c, qkv, four, f32, dev)
    assert torch.equal(out_bits4, out_bits), f"{tag}: the primal output changed with the tangent operands (4 x tangents)"
    assert torch.equal(dout4, 4.0 * dout), f"{tag}: 4 x the tangent operands did not give 4 x the tangent, bit for bit"
    print(f"{tag}: primal bits equal under zero / random / 4 x tangents; 4 x tangents -> 4 x tangent output, bit for bit")


@pytest.mark.parametrize("f32", [False, True], ids=name)
def test_tangent_attention_refusals(dev, f32):
    """What swiftk_window_attention_jvp refuses returns the header's code and leaves both outputs at their sentinels."""
    c = ta.BY_NAME["plain6"]
    r = ta.reference(c, f32, "all")
    rows, (ldq, ldo) = c.B * c.n, strides(c)
    qkv, dqkv = padded_operand(c, r["qkv"], f32, dev), padded_operand(c, r["dqkv"], f32, dev)
    out, dout = X.sent((rows + 1, ldo), f32, dev), X.sent((rows + 1, ldo), f32, dev)
    es = 4 if f32 else 2

    def call(q=qkv.data_ptr(), dq=dqkv.data_ptr(), ldq_=ldq, o=out.data_ptr(), do=dout.data_ptr(), ldo_=ldo, gh=c.grid[0], gw=c.grid[1],
             heads=c.heads, hd=c.hd, sh=c.shift[0], sw=c.shift[1]):
        return L().swiftk_window_attention_jvp(q, dq, ldq_, o, do, ldo_, c.B, gh, gw, heads, hd, sh, sw, code(f32), st())

    # (head_dim 64 with 3 heads needs less room than the buffers have: a refusal that came too late would stay in bounds)
    assert call(hd=64) == ESHAPE
    assert call(gh=24) == ESHAPE and call(gw=8) == ESHAPE            # not whole 16 x 16 windows
    assert call(sh=c.grid[0]) == ESHAPE and call(sw=c.grid[1] + 3) == ESHAPE and call(sh=-1) == ESHAPE
    assert call(ldq_=3 * c.dim - 8) == ESHAPE and call(ldo_=c.dim - 4) == ESHAPE
    assert call(q=qkv.data_ptr() + es) == EALIGN and call(dq=dqkv.data_ptr() + 8) == EALIGN
    if not f32:
        assert call(ldo_=c.dim + 6) == EALIGN                        # bf16 results leave as 8-byte stores
    for nul in ("q", "dq", "o", "do"):
        assert call(**{nul: None}) == EINVAL
    torch.cuda.synchronize()
    blank = X.sent((rows + 1, ldo), f32)
    assert torch.equal(out.cpu(), blank) and torch.equal(dout.cpu(), blank)
    assert call() == 0                                               # and the same buffers are accepted when nothing is wrong
    torch.cuda.synchronize()
    assert not torch.equal(out.cpu(), blank) and not torch.equal(dout.cpu(), blank)
