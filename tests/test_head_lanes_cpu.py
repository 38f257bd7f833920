"""Head widths no kernel runs (66, and 64 / 32 on bf16) on zero-padded head lanes (SWIFTK_PAD_HEADS): the decisions of
``engine.head_lanes``, the weight packers with their adjoints, and the descriptor field -- all on the CPU.

The premise the packers rest on, checked here in fp64 with the oracle's attention: a head whose q, k and v carry zero lanes
has the same L2 norms, hence the same cosine logits and softmax; P V is zero in the pad lanes and wo's zero columns ignore
them."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from conftest import rel_l2
from swift_amd.utils.detinit import det_normal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF, F32 = torch.bfloat16, torch.float32


def test_head_lanes_decisions_switch_unset(monkeypatch):
    from swift_amd._lib import SwiftkError
    from swift_amd.engine import head_lanes
    monkeypatch.delenv("SWIFTK_PAD_HEADS", raising=False)
    with pytest.raises(SwiftkError, match="head_dim.*66") as e:
        head_lanes(1056, 16, BF)
    assert "SWIFTK_PAD_HEADS" in str(e.value)
    assert head_lanes(1056, 12, BF) == (88, 88)
    assert head_lanes(256, 4, F32) == (64, 64)
    assert head_lanes(256, 4, "bf16x3") == (64, 64)
    with pytest.raises(SwiftkError, match="head_dim"):
        head_lanes(256, 4, BF)
    monkeypatch.setenv("SWIFTK_PAD_HEADS", "0")  # "0" is off, as for the other switches
    with pytest.raises(SwiftkError, match="head_dim.*66"):
        head_lanes(1056, 16, BF)


def test_head_lanes_decisions_switch_set(monkeypatch):
    from swift_amd._lib import SwiftkError
    from swift_amd.engine import head_lanes
    monkeypatch.setenv("SWIFTK_PAD_HEADS", "1")
    for dt in (BF, F32, "bf16x3"):
        assert head_lanes(1056, 16, dt) == (66, 80)
        with pytest.raises(SwiftkError, match="head_dim.*100"):
            head_lanes(400, 4, dt)
        assert head_lanes(1056, 12, dt) == (88, 88) and head_lanes(1280, 16, dt) == (80, 80) and head_lanes(1536, 16, dt) == (96, 96)
    assert head_lanes(768, 12, BF) == (64, 80)
    assert head_lanes(256, 8, BF) == (32, 80)
    assert head_lanes(1056, 12, BF) == (88, 88)
    assert head_lanes(256, 4, F32) == (64, 64) and head_lanes(256, 4, "bf16x3") == (64, 64)  # native there: not padded
    assert head_lanes(1008, 12, BF) == (84, 88) and head_lanes(1080, 12, BF) == (90, 96)  # the smallest width that holds it
    with pytest.raises(SwiftkError, match="head_dim"):
        head_lanes(1000, 12, BF)  # dim not divisible by heads


@pytest.mark.parametrize("heads,hd,hdp", [(16, 66, 80), (6, 64, 80), (10, 32, 80), (3, 33, 80)])
def test_packers_keep_the_attention_and_have_exact_adjoints(heads, hd, hdp):
    from oracle.swinv2 import cosine_window_attention
    from swift_amd.engine import pack_qkv_lanes, pack_wo_lanes, unpack_qkv_lanes, unpack_wo_lanes
    d = heads * hd
    seed = 100 + hd + heads
    x = det_normal((2, 256, d), seed, "x").double()
    W = det_normal((heads * 3 * hd, d), seed, "wqkv", std=d ** -0.5).double()
    Wo = det_normal((d, heads * hd), seed, "wo", std=d ** -0.5).double()
    scale = (math.log(10.0) + det_normal((1, heads, 1, 1), seed, "scale")).double()
    Wp, Wop = pack_qkv_lanes(W, heads, hd, hdp), pack_wo_lanes(Wo, heads, hd, hdp)
    assert Wp.shape == (heads * 3 * hdp, d) and Wop.shape == (d, heads * hdp)
    # head h's q block starts at row 3 hdp h; rows hd .. hdp of every block are zero
    Wp4, Wop3 = Wp.view(heads, 3, hdp, d), Wop.view(d, heads, hdp)
    assert torch.equal(Wp4[:, :, :hd], W.view(heads, 3, hd, d)) and not Wp4[:, :, hd:].any()
    assert torch.equal(Wop3[:, :, :hd], Wo.view(d, heads, hd)) and not Wop3[:, :, hd:].any()
    a = cosine_window_attention(x @ W.t(), scale, heads, naive=True)
    ap = cosine_window_attention(x @ Wp.t(), scale, heads, naive=True)
    ap3 = ap.view(2, 256, heads, hdp)
    assert not ap3[..., hd:].any()  # exactly zero, not merely small
    assert rel_l2(ap3[..., :hd].reshape(2, 256, d), a) <= 1e-12
    assert rel_l2(ap @ Wop.t(), a @ Wo.t()) <= 1e-12
    # adjoints: <pack(W), G> == <W, unpack(G)> for lane-shaped G
    G, Go = det_normal(tuple(Wp.shape), seed, "g").double(), det_normal(tuple(Wop.shape), seed, "go").double()
    gq, go = unpack_qkv_lanes(G, heads, hd, hdp), unpack_wo_lanes(Go, heads, hd, hdp)
    assert gq.shape == W.shape and go.shape == Wo.shape
    for lhs, rhs in (((Wp * G).sum(), (W * gq).sum()), ((Wop * Go).sum(), (Wo * go).sum())):
        assert abs(float(lhs) - float(rhs)) <= 1e-12 * max(1.0, abs(float(rhs)))
    # a native width passes through untouched
    assert pack_qkv_lanes(W, heads, hd, hd) is W and unpack_wo_lanes(Go, heads, hdp, hdp) is Go


def test_descriptor_carries_the_head_width_behind_layers_host():
    from swift_amd._lib import Layer, Model
    names = [f[0] for f in Model._fields_]
    assert names[-2:] == ["layers_host", "head_dim"]
    assert dict(Model._fields_)["head_dim"] is C.c_int32
    assert Model.head_dim.offset == Model.layers_host.offset + C.sizeof(C.POINTER(Layer))  # appended: no existing offset moved
    assert Model().head_dim == 0  # 0 = dim / heads
    text = open(os.path.join(ROOT, "include", "swiftk.h")).read()
    body = re.search(r"typedef struct swiftk_model \{(.*?)\} swiftk_model;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+)\s*;", body)
    assert fields[-2:] == ["layers_host", "head_dim"] and re.search(r"int32_t\s+head_dim\s*;", body)


def test_workspace_follows_the_attention_inner_width():
    """swiftk_workspace_bytes is host arithmetic: head_dim = 0 and head_dim = dim / heads size the same workspace, and padded lanes
    add exactly the wider q/k/v buffer (3 inner columns) and attention output (k_pad(inner) columns) -- nothing else depends on it
    in the bf16 and exact-fp32 engines; the split engine's operand buffer also holds wo's input (3 inner against 3 mlp: no growth here)."""
    from swift_amd import _lib
    L = _lib.lib()
    al = lambda v: (v + 255) & ~255

    def bytes_(dtype, heads, head_dim, B=2):
        mo = _lib.Model()
        mo.dtype, mo.H, mo.W, mo.p1, mo.p2, mo.in_ch, mo.out_ch = dtype, 64, 64, 2, 2, 141, 69
        mo.depth, mo.dim, mo.heads, mo.mlp, mo.wh, mo.ww, mo.sh, mo.sw = 2, 1056, heads, 2816, 16, 16, 8, 8
        code = _lib.BF16 if dtype == _lib.BF16 else _lib.F32
        mo.kd, mo.kmlp, mo.kpe = (int(L.swiftk_gemm_k_pad(code, k)) for k in (1056, 2816, 141 * 4))
        layers = (_lib.Layer * 2)()
        mo.layers_host = C.cast(layers, C.POINTER(_lib.Layer))
        mo.head_dim = head_dim
        return int(L.swiftk_workspace_bytes(C.byref(mo), B))

    M = 2 * 32 * 32
    for dtype, es in ((_lib.BF16, 2), (_lib.F32, 4), (_lib.BF16X3, 4)):
        code = _lib.BF16 if dtype == _lib.BF16 else _lib.F32
        base = bytes_(dtype, 12, 0)
        assert base > 0 and bytes_(dtype, 12, 88) == base and bytes_(dtype, 16, 0) == base
        kd, katt = int(L.swiftk_gemm_k_pad(code, 1056)), int(L.swiftk_gemm_k_pad(code, 1280))
        grow = al(M * 3 * 1280 * es) + al(M * katt * es) - al(M * 3 * 1056 * es) - al(M * kd * es)
        assert bytes_(dtype, 16, 80) == base + grow
    assert bytes_(_lib.BF16, 16, -1) == 0  # a negative width is no model
