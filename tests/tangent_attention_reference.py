"""TEST INFRASTRUCTURE: random operands, the fp64 truth and three plain restatements for the window-attention TANGENT kernels
(swiftk_window_attention_jvp: attn_jvp_bf16_kernel and attn_jvp_kernel<float, HD> of swift_amd/csrc/jvp_kernels.hip), judged per
(sample, window, head) item.  No GPU and nothing from the HIP library here.

  * ``operands``      q-hat rows of norm tau_h with tau in TAUS across the heads (as the QK-norm leaves them), k-hat rows of unit
                      norm, v ~ N(0, 1), tangents 0.3 N(0, 1); everything rounded to the storage type; ``only`` keeps one of the
                      three tangents and zeroes the other two (a missing or mis-signed term cannot then hide under the others)
  * ``truth``         torch.func.jvp in fp64 of softmax(q k^T) v on the windowed layout, token order in, through
                      oracle.swinv2.window_token_index
  * ``item_rel_l2``   relative L2 per item, [B, nW, H]
  * ``restate_bf16``  yardstick A: what the bf16 kernel documents -- fp32 S, dS, e = exp(S - max), W = e o dS, l = rowsum(e),
                      r = rowsum(W); e and W rounded to bf16 for the value products e V, W V, e dV (fp32 accumulation);
                      out = bf16((e V) / l), dout = bf16(((W V + e dV) - (r / l)(e V)) / l): one bf16 rounding at the store.
                      Three keyword faults for tests/test_tangent_attention_reference_cpu.py.
  * ``restate_autocast``  yardstick B: the autocast form -- P = softmax(S) and dP = P o (dS - rowsum(P o dS)) normalised in
                      fp32 and THEN rounded to bf16 for P V, dP V, P dV; bf16 store
  * ``restate_fp32``  yardstick C: the formula of A in fp32 throughout (the fp32 kernel's)

The bound of tests/test_gpu_tangent_attention.py: every item of the bf16 kernel within FACTOR = 2 x its head's yardstick, the larger
worst-item error of A and B against the truth (the rule and margin of test_random_inputs_per_item_against_the_oracle_yardstick: the
hardware exp and the matrix pipe's order are a third rounding of the same quantities); every item of the fp32 kernel within
F32_TOL.  Conditions, asserted on the CPU: every bf16 tangent yardstick <= BF16_YARD_CAP, every fp32 one <= F32_YARD_CAP.
"""
from __future__ import annotations

import math
from functools import lru_cache

import torch

import exact_attention as X
from oracle.swinv2 import window_token_index

TAUS = (1.0, 10.0, 47.0, 100.0)
FACTOR = 2.0
F32_TOL = 1e-5                 # tests/test_gpu_backward_kernels.py: fp32 vectors
BF16_YARD_CAP = 1.5e-2         # twice what yardstick A reaches (7.2e-3 at head_dim 88, tau 100)
F32_YARD_CAP = 5e-6            # four times what yardstick C reaches (1.3e-6)
VARIANTS = ("all", "dq", "dk", "dv")

#            name        B  grid      heads hd  shift    what the row is for
CASES = [
    X.Case("plain6",     1, (16, 32),  3, 80, (3, 5),  "6 items = 12 workgroups: the plain (item, query half) block order; odd shifts"),
    X.Case("remap16",    2, (32, 16),  4, 88, (8, 8),  "16 items = 32 workgroups: the remapped block order; two samples, head_dim 88"),
    X.Case("remap8",     1, (16, 16),  8, 96, (0, 0),  "8 items = 16 workgroups: remapped, head_dim 96, all four tau twice"),
]
BY_NAME = {c.name: c for c in CASES}
THE_96 = X.Case("jvp96", 2, (32, 32), 12, 88, (8, 8), "the 96-item problem of test_gpu_train.py::test_window_attention_jvp_kernel")
SCALE_96 = (10.0, 3.0, 30.0, 60.0, 1.0, 10.0, 50.0, 20.0, 15.0, 5.0, 20.0, 10.0)


def taus(c: X.Case):
    return torch.tensor([TAUS[h % len(TAUS)] for h in range(c.heads)])


def store(x, f32):
    """Rounded to the storage type, returned as fp32."""
    return x.float() if f32 else x.float().bfloat16().float()


@lru_cache(maxsize=None)   # 3 cases x 2 storage types x 4 variants, a few MB each
def operands(c: X.Case, f32: bool, only: str = "all"):
    """token-order (qkv, dqkv) [B, n, 3 dim] fp32 holding storage-type values."""
    g = torch.Generator().manual_seed(c.seed + 31)
    sh = (c.B, c.nW, c.heads, 256, c.hd)
    q, k, v, dq, dk, dv = (torch.randn(sh, generator=g) for _ in range(6))
    q = q / q.norm(dim=-1, keepdim=True) * taus(c).view(1, 1, c.heads, 1, 1)
    k = k / k.norm(dim=-1, keepdim=True)
    tan = {"dq": 0.3 * dq, "dk": 0.3 * dk, "dv": 0.3 * dv}
    if only != "all":
        tan = {n: (t if n == only else torch.zeros_like(t)) for n, t in tan.items()}
    return store(X.assemble(c, q, k, v), f32), store(X.assemble(c, tan["dq"], tan["dk"], tan["dv"]), f32)


def operands_96():
    """The operands of test_window_attention_jvp_kernel at (12, 88), shift (8, 8), as that test draws them (bf16 values)."""
    c = THE_96
    rnd = lambda shape, seed: torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
    raw = rnd((c.B, c.n, 3 * c.dim), 40).reshape(c.B, c.n, c.heads, 3, c.hd)
    tau = torch.clamp(torch.log(torch.tensor(SCALE_96)), max=math.log(100.0)).exp().view(1, 1, c.heads, 1)
    q = raw[:, :, :, 0] / raw[:, :, :, 0].norm(dim=-1, keepdim=True).clamp_min(1e-12) * tau
    k = raw[:, :, :, 1] / raw[:, :, :, 1].norm(dim=-1, keepdim=True).clamp_min(1e-12)
    pre = torch.stack([q, k, raw[:, :, :, 2]], dim=3).reshape(c.B, c.n, -1)
    return store(pre, False), store(0.3 * rnd((c.B, c.n, 3 * c.dim), 41), False)


def windows(c: X.Case, x):
    """token-order [B, n, heads * hd] -> window order [B, nW, H, 256, hd] through the oracle's index map."""
    idx = window_token_index(c.grid, (16, 16), c.shift).reshape(-1)
    return x.reshape(c.B, c.n, c.heads, c.hd)[:, idx].reshape(c.B, c.nW, 256, c.heads, c.hd).permute(0, 1, 3, 2, 4)


def parts(c: X.Case, qkv, dqkv, dtype=torch.float64):
    """token-order operands -> window-order (q, k, v, dq, dk, dv) in ``dtype``."""
    return tuple(t.to(dtype) for t in (*X.thirds(c, qkv), *X.thirds(c, dqkv)))


def _attn(q, k, v):
    return (q @ k.transpose(-2, -1)).softmax(-1) @ v


def truth(c: X.Case, qkv, dqkv):
    """(out, dout) [B, nW, H, 256, hd] fp64: torch.func.jvp of softmax(q k^T) v on the windowed layout."""
    q, k, v, dq, dk, dv = parts(c, qkv, dqkv)
    return torch.func.jvp(_attn, (q, k, v), (dq, dk, dv))


item_rel_l2 = X.item_rel_l2          # [B, nW, H, 256, hd] x 2 -> relative L2 per (sample, window, head) item, [B, nW, H] (fp64)


def per_head_worst(err):
    """[B, nW, H] -> the worst item of each head, [H]."""
    return err.amax(dim=(0, 1))


def _scores(q, k, dq, dk):
    s = q @ k.transpose(-2, -1)
    ds = dq @ k.transpose(-2, -1) + q @ dk.transpose(-2, -1)
    e = (s - s.amax(-1, keepdim=True)).exp()
    return e, e * ds


def restate_bf16(q, k, v, dq, dk, dv, drop_correction=False, swap_dk_halves=False, ignore_dv=False, rnd=X.bf16r):
    """Yardstick A on window-order fp32 tensors holding bf16 values; returns (out, dout) as bf16 values in fp32.
    The keyword faults: the correction -(r / l)(e V) left out; dK taken from the other key half (keys 0..127 <-> 128..255); dv
    taken as zero.  ``rnd``: the rounding of e, W and the stored results (the identity leaves the bare formula)."""
    if swap_dk_halves:
        dk = dk.roll(128, dims=-2)
    if ignore_dv:
        dv = torch.zeros_like(dv)
    e, w = _scores(q, k, dq, dk)
    l, r = e.sum(-1, keepdim=True), w.sum(-1, keepdim=True)
    eb, wb = rnd(e), rnd(w)
    o, u, tt = eb @ v, wb @ v, eb @ dv
    rl = 1.0 / l
    corr = torch.zeros_like(o) if drop_correction else (r * rl) * o
    return rnd(o * rl), rnd(((u + tt) - corr) * rl)


def restate_autocast(q, k, v, dq, dk, dv, rnd=X.bf16r):
    """Yardstick B: P and dP normalised in fp32, then rounded to bf16 for the value products; bf16 store."""
    s = q @ k.transpose(-2, -1)
    ds = dq @ k.transpose(-2, -1) + q @ dk.transpose(-2, -1)
    p = s.softmax(-1)
    dp = p * (ds - (p * ds).sum(-1, keepdim=True))
    pb = rnd(p)
    return rnd(pb @ v), rnd(rnd(dp) @ v + pb @ dv)


def restate_fp32(q, k, v, dq, dk, dv):
    """Yardstick C: the kernels' formula in fp32 throughout."""
    e, w = _scores(q, k, dq, dk)
    l, r = e.sum(-1, keepdim=True), w.sum(-1, keepdim=True)
    o, u, tt = e @ v, w @ v, e @ dv
    rl = 1.0 / l
    return o * rl, ((u + tt) - (r * rl) * o) * rl


@lru_cache(maxsize=None)   # 3 cases x 2 storage types x 4 variants, a few MB each
def reference(c: X.Case, f32: bool, only: str = "all"):
    """dict: qkv, dqkv (token order), out, dout (fp64 truth, window order), yard_out, yard_dout [H] (per head: the worst item of
    A and B in bf16, of C in fp32, against the truth)."""
    qkv, dqkv = operands(c, f32, only)
    out, dout = truth(c, qkv, dqkv)
    p32 = parts(c, qkv, dqkv, torch.float32)
    yo, yd = torch.zeros(c.heads, dtype=torch.float64), torch.zeros(c.heads, dtype=torch.float64)
    for fn in ((restate_fp32,) if f32 else (restate_bf16, restate_autocast)):
        o, d = fn(*p32)
        yo = torch.maximum(yo, per_head_worst(item_rel_l2(o, out)))
        yd = torch.maximum(yd, per_head_worst(item_rel_l2(d, dout)))
    return dict(qkv=qkv, dqkv=dqkv, out=out, dout=dout, yard_out=yo, yard_dout=yd)
