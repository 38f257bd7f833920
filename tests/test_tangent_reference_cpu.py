"""CPU: the references of tests/test_gpu_tangent_kernels.py (tests/tangent_reference.py) against torch.func.jvp / autograd of the
oracle's own expressions, the sensitivity condition on the norm inputs, and the fp32 yardsticks the GPU tolerances derive from."""
import math

import pytest
import torch
import torch.nn.functional as F

import tangent_reference as tr
from conftest import rel_l2

F64 = torch.float64
# the cases the fp32 yardsticks were taken on: (d, rows_per_sample, B)
YARD_CASES = [(1056, 64, 3), (1280, 96, 2), (1536, 40, 2), (96, 32, 2)]


def rnd(shape, seed, std=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=dtype) * std


@pytest.mark.parametrize("d", [1056, 100])
def test_modnorm_tangent_equals_jvp_of_the_oracle(d):
    """modnorm_tangent == torch.func.jvp of x + oracle.swinv2.modulated_norm(y, mod) over (x, y, mod) in fp64 (the modulation
    Linear fed as an identity, so that ``mod`` itself is the latent), hostile rows included."""
    from oracle.swinv2 import modulated_norm
    B, rps = 2, 8
    c = {k: (v.double() if torch.is_tensor(v) else v) for k, v in tr.make_norm_case(d, rps, B, 11).items()}
    p = {"n.norm.weight": c["gamma"], "n.norm.bias": c["beta"], "n.modulation.weight": torch.eye(2 * d, dtype=F64),
         "n.modulation.bias": torch.zeros(2 * d, dtype=F64)}

    def f(x, y, mod):
        return x + modulated_norm(y.view(B, rps, d), mod, p, "n.").reshape(B * rps, d)

    ref_x, ref_dx = torch.func.jvp(f, (c["x"], c["y"], c["mod"]), (c["dx"], c["dy"], c["dmod"]))
    x_new, dx_new = tr.modnorm_tangent(**c)
    assert rel_l2(tr.benign(x_new), tr.benign(ref_x)) < 1e-12 and rel_l2(tr.benign(dx_new), tr.benign(ref_dx)) < 1e-12
    for r in range(tr.HOSTILE_ROWS):
        assert rel_l2(x_new[r], ref_x[r]) < 1e-12 and rel_l2(dx_new[r], ref_dx[r]) < 1e-12, r
    # the constant row really is one: variance 0, n = 0, and its tangent is dy - mean(dy) at rstd = 1 / sqrt(eps) = 1e3
    assert float(c["y"][1].std()) == 0.0 and float(c["y"][1, 0]) == 40.0
    # the fp32 restatement is the same function (two-pass and one-pass agree with fp64 far below any term's share)
    for one_pass in (False, True):
        x32, dx32 = tr.modnorm_tangent_fp32(**c, one_pass=one_pass)
        assert x32.dtype == torch.float32
        assert rel_l2(tr.benign(x32), tr.benign(x_new)) < 1e-5 and rel_l2(tr.benign(dx32), tr.benign(dx_new)) < 1e-6


@pytest.mark.parametrize("d", [1056, 1536, 96])
def test_every_term_of_the_tangent_is_visible_on_the_norm_inputs(d):
    """The sensitivity condition: over the benign rows of make_norm_case, leaving out any one named term moves the increment
    dx_new - dx by at least 1e-2 relative L2 -- a thousand times the GPU tolerances, so none of them can hide a missing term.
    (Seen at d = 1056 / 1536 / 96: mean_dy 0.34 / 0.34 / 0.35, n_mean_ndy 0.026 / 0.020 / 0.085, gamma_dn 0.79, dsc 0.44, dsh 0.43.)
    Not asserted on the hostile rows, which are there for the arithmetic only."""
    c = tr.make_norm_case(d, 64, 3, 100)
    _, dx_new = tr.modnorm_tangent(**c)
    inc = tr.benign(dx_new - c["dx"].double())
    for term in tr.TERMS:
        _, dx_drop = tr.modnorm_tangent(**c, drop=term)
        share = rel_l2(tr.benign(dx_drop - c["dx"].double()), inc)
        print(f"d {d}: without {term} the increment moves by {share:.3e}")
        assert share >= 1e-2, (term, share)
    # and the primal is untouched by the keyword
    assert torch.equal(tr.modnorm_tangent(**c, drop="dsc")[0], tr.modnorm_tangent(**c)[0])


def test_pair_quantise_is_the_8_bit_pair():
    """hi is the bf16 rounding, the byte stays in [0, 255] with |value - v| <= ulp(hi) / 512 (ulp(hi) / 256 where it saturates),
    values a pair holds exactly are fixed points (ties apart), zero stays zero, and ops.pair_value of the parts gives the same value."""
    from swift_amd import ops
    v = torch.cat([rnd((4096,), 1), rnd((4096,), 2, 1e-6), rnd((4096,), 3, 3e4), torch.tensor([0.0, 1.0, -1.0, 300.0, 2.0 ** -100])])
    q, hi, byte = tr.pair_quantise(v, parts=True)
    assert torch.equal(hi, v.bfloat16()) and byte.dtype == torch.uint8
    assert torch.isfinite(q).all() and float(q[-5]) == 0.0
    E = ((hi.view(torch.int16).to(torch.int32) >> 7) & 0xFF).double()
    err = (q.double() - v.double()).abs()
    # (byte 255 also stands for a remainder that rounds to 256 -- just under + ulp / 2 -- and is then a whole step off)
    assert bool((err <= 2.0 ** (E - 142)).all()) and bool((err <= 2.0 ** (E - 143))[byte < 255].all())
    nz = v != 0
    assert float(((q - v).abs() / v.abs())[nz].max()) <= 2.0 ** -15  # (a whole step of 2^-8 ulp(hi), ulp(hi) <= 2^-7 |hi|)
    keep = byte > 0  # (byte 0 is hi - ulp / 2: a tie that bf16 may round to the other neighbour, whose byte would be 256)
    assert torch.equal(tr.pair_quantise(q)[keep], q[keep])
    assert torch.equal(ops.pair_value(hi.view(1, -1), byte.view(1, -1), v.numel()).view(-1), q)


def _yardsticks(d, rps, B):
    c = tr.make_norm_case(d, rps, B, 100)
    c["x"], c["dx"] = tr.pair_quantise(c["x"]), tr.pair_quantise(c["dx"])  # what a pair can hold going in
    x64, dx64 = tr.modnorm_tangent(**c)
    inc64 = dx64 - c["dx"].double()
    out = {}
    for one_pass in (False, True):
        x32, dx32 = tr.modnorm_tangent_fp32(**c, one_pass=one_pass)
        qx, qdx = tr.pair_quantise(x32), tr.pair_quantise(dx32)
        b = tr.benign
        out[one_pass] = dict(
            raw_x=rel_l2(b(x32), b(x64)), raw_dx=rel_l2(b(dx32), b(dx64)), pair_x=rel_l2(b(qx), b(x64)), pair_dx=rel_l2(b(qdx), b(dx64)),
            pair_inc=rel_l2(b(qdx.double() - c["dx"].double()), b(inc64)),
            row_raw=[rel_l2(dx32[r], dx64[r]) for r in range(tr.HOSTILE_ROWS)],
            row_pair=[max(tr.row_err(qx[r], x64[r]), tr.row_err(qdx[r], dx64[r])) for r in range(tr.HOSTILE_ROWS)])
    return out


@pytest.mark.parametrize("d,rps,B", YARD_CASES)
def test_fp32_yardsticks_stay_where_the_tolerances_were_derived(d, rps, B):
    """The fp32 restatement against fp64 on the norm inputs.  The GPU thresholds (1e-5 for a pair value, 1.5e-5 for the increment,
    4 x the hostile row's own yardstick) are 1.5 x / 4 x what is measured HERE, so these brackets notice a change of the inputs
    that makes the case easier or harder.  Seen (benign rows, relative L2, over the four cases):
      before storage      two-pass x, dx 6.5e-8 .. 6.9e-8; one-pass x 7e-8 .. 1.2e-7, dx 6.6e-8 .. 1.0e-7
      pair value          6.5e-6 .. 6.6e-6 either way (the 8-bit low part: 2^-17 relative, uniformly distributed)
      increment           9.6e-6 .. 9.7e-6 (the low part's error scales with |dx_new|, 1.5 x the increment)
      row 0 tangent       two-pass 4e-8 .. 6e-8; one-pass 1.7e-6 (d 96) .. 3.3e-5 (d 1280): the outlier sits in the shift element
      rows 1-3 tangent    <= 1.1e-7 either way
      worst row after storage, max|err| / max|ref|   two-pass 1.0e-5 .. 1.9e-5, one-pass 2.4e-5 .. 6.6e-5 (row 0)"""
    y = _yardsticks(d, rps, B)
    for one_pass in (False, True):
        print(f"d {d} rows/sample {rps} one_pass {one_pass}: " + ", ".join(
            f"{k} {v:.2e}" if isinstance(v, float) else f"{k} [" + " ".join(f"{e:.1e}" for e in v) + "]" for k, v in y[one_pass].items()))
    two, one = y[False], y[True]
    assert 3e-8 < two["raw_x"] < 2e-7 and 3e-8 < two["raw_dx"] < 2e-7
    assert 3e-8 < one["raw_x"] < 1e-5 and 3e-8 < one["raw_dx"] < 2e-7
    for k in (two, one):
        assert 6e-6 < k["pair_x"] < 8.5e-6 and 6e-6 < k["pair_dx"] < 8.5e-6
        assert 9e-6 < k["pair_inc"] < 1.0e-5     # (1.5e-5, the GPU bound, is 1.5 x this)
        assert max(k["row_raw"][1:]) < 2e-7
    assert two["row_raw"][0] < 2e-7 and max(two["row_pair"]) < 4e-5
    assert one["row_raw"][0] < 1e-4 and max(one["row_pair"]) < 3e-4
    if d >= 1056:  # the shifted one-pass variance does feel the outlier in its shift element (else the row tests nothing)
        assert one["row_raw"][0] > 5 * two["row_raw"][0]


def test_silu_closed_forms():
    z = torch.cat([rnd((1000,), 4, 3.0, F64), torch.tensor([0.0, 30.0, -30.0, 90.0, -90.0], dtype=F64)])
    dz = rnd((1005,), 5, 1.0, F64)
    ry, rdy = torch.func.jvp(F.silu, (z,), (dz,))
    y, dy = tr.silu_tangent(z, dz)
    assert rel_l2(y, ry) < 1e-12 and rel_l2(dy, rdy) < 1e-12
    zz = z.clone().requires_grad_(True)
    F.silu(zz).backward(dz)
    assert rel_l2(tr.silu_grad(z) * dz, zz.grad) < 1e-12
    # the limits the kernels must reach although expf(90) overflows in fp32: silu'(+inf) = 1, silu'(-inf) = 0
    assert abs(float(tr.silu_grad(torch.tensor([90.0]))) - 1.0) < 1e-30 and abs(float(tr.silu_grad(torch.tensor([-90.0])))) < 1e-30


@pytest.mark.parametrize("M,heads,hd", tr.QKNORM_JVP_CASES)
def test_qknorm_tangent_equals_jvp_of_the_oracle_lines(M, heads, hd):
    """oracle/swinv2.py, cosine_window_attention: q = q / |q|.clamp_min(1e-12) * exp(min(scale, ln 100)), k = k / |k|.clamp_min(1e-12),
    differentiated by torch.func.jvp in fp64; the planted all-zero vectors keep a zero primal and get the finite tangent tau dx 1e12;
    the builder's shapes leave a ragged last block of 16 vectors and one head above the clamp."""
    qkv, dqkv, scale = tr.qknorm_jvp_inputs(M, heads, hd, 7)
    assert (M * heads * 2) % 16 != 0 and float(scale[-1]) > tr.LN100 and float(scale[:-1].max()) < tr.LN100
    x, dx = qkv.double().view(M, heads, 3, hd), dqkv.double().view(M, heads, 3, hd)
    tau = torch.clamp(scale.double(), max=math.log(1.0 / 0.01)).exp().view(1, heads, 1)

    def lines(t):
        q, k, v = t[:, :, 0], t[:, :, 1], t[:, :, 2]
        q = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12) * tau
        k = k / k.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        return torch.stack([q, k, v], dim=2)

    zeros = tr.zero_vectors(M, heads)
    live = torch.ones(M, heads, 3, dtype=torch.bool)
    for z in zeros:
        live[z] = False
        assert float(x[z].abs().max()) == 0 and float(dx[z].abs().max()) > 0
    ref, dref = torch.func.jvp(lines, (x,), (dx,))
    got, dgot, rn = tr.qknorm_tangent(qkv, dqkv, scale, heads, hd)
    assert rel_l2(got, ref) < 1e-14 and rel_l2(dgot[live], dref[live]) < 1e-13       # (autograd of norm() at 0 is a subgradient)
    assert torch.equal(got[:, :, 2], x[:, :, 2]) and torch.equal(dgot[:, :, 2], dx[:, :, 2]) and bool((rn[:, :, 2] == 1).all())
    assert rel_l2(rn[:, :, :2][live[:, :, :2]], 1.0 / x[:, :, :2].norm(dim=-1)[live[:, :, :2]]) < 1e-14
    for z in zeros:   # the kernel's formula at |x| = 0: c = 0 / 1e-24 = 0, x-hat = 0, d x-hat = tau dx / 1e-12
        t = float(tau[0, z[1], 0]) if z[2] == 0 else 1.0
        assert float(got[z].abs().max()) == 0 and rel_l2(dgot[z], t * dx[z] * 1e12) < 1e-14 and float(rn[z]) == 1e12
        assert bool(torch.isfinite(dgot[z].float().bfloat16()).all())
    # the tangent is orthogonal to the direction: the term v (v . dv) / n^2 is pinned
    assert float(((dgot[:, :, :2] * got[:, :, :2]).sum(-1)[live[:, :, :2]]).abs().max()) < 1e-10


def test_swiglu_tangent_equals_jvp_of_the_oracle_line():
    """oracle/swinv2.py: h = F.silu(h[..., :m]) * h[..., m:], on the interleaved columns, by torch.func.jvp in fp64 -- planted gates
    included; the scales bound the terms, and torch's fp32 evaluation stays within a few fp32 epsilon of them."""
    import backward_reference as br
    h, _ = br.swiglu_inputs(5, 37, 45)
    dh = rnd((5, 74), 46)
    assert h[4, 0:12:2].tolist() == [pytest.approx(g) for g in br.PLANTED_GATES]
    ref, dref = torch.func.jvp(lambda t: F.silu(t[:, 0::2]) * t[:, 1::2], (h.double(),), (dh.double(),))
    out, dout, so, sd = tr.swiglu_tangent(h, dh)
    assert float(((out - ref).abs() / (so + 1e-300)).max()) < 1e-14 and float(((dout - dref).abs() / (sd + 1e-300)).max()) < 1e-14
    assert bool((out.abs() <= so).all()) and bool((dout.abs() <= sd * (1 + 1e-15)).all())
    o32, d32, _, _ = tr.swiglu_tangent(h, dh, torch.float32)
    assert o32.dtype == torch.float32
    eo, ed = float(((o32.double() - out).abs() / (so + 2.0 ** -102)).max()), float(((d32.double() - dout).abs() / (sd + 2.0 ** -102)).max())
    print(f"swiglu tangent, torch fp32 on the CPU: out {eo:.2e}, tangent {ed:.2e} of the element's scale")
    assert eo < 2e-6 and ed < 2e-6


def test_bf16_round_once_rounds_once():
    """Equal to torch's fp32 -> bf16 rounding on fp32 values (powers of two, binade ends and ties included), and the nearer neighbour
    where fp64 -> fp32 -> bf16 rounds twice: 6.671874913737452 (an element of test_swiglu_jvp_alone) is below the tie 6.671875."""
    x = torch.cat([rnd((20000,), 9, 3.0), torch.tensor([1.0, 2.0, -0.5, 1.99609375, 1.998046875, 1.00390625, 1.01171875, 3e-5, -7e4])])
    assert torch.equal(tr.bf16_round_once(x.double()), x.bfloat16().double())
    v = torch.tensor([6.671874913737452, -0.001598358150361509], dtype=F64)
    assert tr.bf16_round_once(v).tolist() == [6.65625, -0.00159454345703125]
    assert v.float().bfloat16().double().tolist() == [6.6875, -0.0016021728515625]           # the twice-rounded route
    assert tr.bf16_score_once(torch.tensor([6.65625]), v[:1]) == (0.0, 0.0)


@pytest.mark.parametrize("B,d", [(3, 1056), (1, 2), (5, 97)])
@pytest.mark.parametrize("w", [1.0, 1000.0])
def test_timestep_embed_tangent(B, d, w):
    from oracle.swinv2 import timestep_embedding
    half = d // 2
    freqs = torch.exp(-math.log(10_000) * torch.arange(half, dtype=F64) / half)
    t, dt = torch.tensor([0.0, 0.4, 1.5, 0.77, 1.1], dtype=F64)[:B], rnd((B,), 6, 1.0, F64)
    got = tr.timestep_embed_tangent(t, dt, freqs, d, w)
    assert got.shape == (B, d)
    _, ref = torch.func.jvp(lambda tt: timestep_embedding(tt * w, 2 * half), (t,), (dt,))
    assert rel_l2(got[:, :2 * half], ref) < 1e-12
    if d % 2:
        assert float(got[:, -1].abs().max()) == 0.0
    # the fp32 evaluation of the same expression: what bounds a kernel at large arguments
    g32 = tr.timestep_embed_tangent(t, dt, freqs, d, w, dtype=torch.float32)
    assert g32.dtype == torch.float32 and rel_l2(g32, got) < (1e-6 if w == 1.0 else 1e-3)


@pytest.mark.parametrize("r", [0.0, 0.4, 1.0])
def test_scm_target_equals_the_lines_of_the_oracle_loss(r):
    """The `g` lines of oracle.loss.scm_loss (loss.py:236-247 of the reference), lifted out, on [B, C, H, W] tensors."""
    import numpy as np
    B, C, H, W, sd = 3, 5, 4, 6, 0.7
    Fx, dxt, x_t, dF = (rnd((B, C, H, W), 20 + i, 1.0, F64) for i in range(4))
    tt = torch.tensor([0.02, 0.8, 1.55], dtype=F64)
    t = tt.view(B, 1, 1, 1)
    c, s = torch.cos(t), torch.sin(t)
    g = -(c ** 2) * (sd * Fx - dxt) - r * ((c * s) * x_t + sd * dF)
    g_raw = g
    gn = torch.linalg.vector_norm(g, dim=(1, 2, 3), keepdim=True)
    gn = gn * np.sqrt(gn.numel() / g.numel())
    g = g / (gn + 0.1)
    target, g_got = tr.scm_target(Fx.view(B, -1), dxt.view(B, -1), (x_t / sd).view(B, -1), dF.view(B, -1), tt, r, sd)
    assert rel_l2(g_got, g_raw.view(B, -1)) < 1e-12
    assert rel_l2(target, (Fx + g).view(B, -1)) < 1e-12 and rel_l2(target - Fx.view(B, -1), g.view(B, -1)) < 1e-12
    # g = 0 exactly: the + 0.1 keeps the division finite and the target is F itself
    tz, gz = tr.scm_target(Fx.view(B, -1), (sd * Fx).view(B, -1), torch.zeros(B, C * H * W), torch.zeros(B, C * H * W), tt, r, sd)
    assert float(gz.abs().max()) == 0.0 and torch.equal(tz, Fx.view(B, -1))


def test_rmse_sums_equals_the_oracle_validation_sums():
    """oracle/validate.py: mean((Y - T)^2) and mean_{b,h,w}(w_lat (Y - T)^2) are these sums over their counts."""
    B, C, H, W = 3, 5, 7, 3
    y, t = rnd((B, C, H, W), 30, 1.0, F64), rnd((B, C, H, W), 31, 1.0, F64)
    w_lat = torch.cos(torch.deg2rad(torch.linspace(-80, 80, H, dtype=F64)))
    w_lat = w_lat / w_lat.mean()
    sq = tr.rmse_sums(y, t, w_lat)
    assert sq.shape == (1 + C,)
    assert abs(float(sq[0] / (B * C * H * W)) - float(torch.mean((y - t) ** 2))) < 1e-12
    assert rel_l2(sq[1:] / (B * H * W), torch.mean(w_lat[None, None, :, None] * ((y - t) ** 2), dim=(0, 2, 3))) < 1e-12


def test_make_norm_case_hostile_rows():
    c = tr.make_norm_case(1056, 40, 2, 5)
    y, dy = c["y"], c["dy"]
    assert y.shape == (80, 1056) and c["mod"].shape == (2, 2112) and c["dmod"].shape == (2, 2112)
    assert torch.equal(y, tr.bf16_round(y)) and torch.equal(dy, tr.bf16_round(dy))  # bf16 holds every element exactly
    assert float(y[0, 0]) == 300.0 and float(y[3, 7]) == -500.0
    assert float(y[1].min()) == float(y[1].max()) == 40.0
    assert int((y[2] != 0).sum()) == 1 and abs(float(y[2].sum()) - 1e-3) < 1e-5
    b = tr.benign(y)
    assert abs(float(b.mean()) - 0.5) < 0.05 and abs(float(b.std()) - 2.0) < 0.05
    assert abs(float(dy.mean()) - 0.3) < 0.05 and abs(float(dy.std()) - 0.7) < 0.05
    # the same seed gives the same case; fp32 benign rows on request, hostile rows rounded all the same
    assert all(torch.equal(v, tr.make_norm_case(1056, 40, 2, 5)[k]) for k, v in c.items() if torch.is_tensor(v))
    f = tr.make_norm_case(1056, 40, 2, 5, bf16_rows=False)
    assert torch.equal(f["y"][:4], y[:4]) and not torch.equal(f["y"][4:], y[4:]) and torch.equal(tr.bf16_round(f["y"][4:]), y[4:])
