"""SwinV2-style isotropic windowed denoiser -- host-side mirror of the reference module.

Same constructor kwargs, same ``forward`` signature and the same 166 state-dict
keys / shapes as reference ``src/swift/models/swinv2.py:254-330`` (so reference
checkpoints load unchanged, including the per-head ``[q|k|v]`` interleave of
``to_qkv``), but the modules below only *hold parameters*: the arithmetic runs in
the hand-written gfx950 kernels of ``csrc/`` through ``SwinEngine``.  There is no
ATen fallback -- CPU tensors raise.

Compute dtype follows the reference's mechanism: callers wrap the network call in
``torch.autocast(device, dtype=...)`` (diffusion.py:457, trainer.py:192); bf16
autocast selects the bf16-MFMA engine, anything else the exact-fp32 engine.
"""
from __future__ import annotations

import math
import os
from typing import Optional, Sequence, Union

import torch
import torch.nn as nn

from ..engine import SwinEngine
from .abstract import AbstractNetwork, Shape2D, _Shape2D


class _Holder(nn.Module):
    """Parameter container; never called."""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("parameter holder: the arithmetic lives in swift_amd/csrc")


class LatentEmbedding(_Holder):  # swinv2.py:67-74
    def __init__(self, dim):
        super().__init__()
        self.l1 = nn.Linear(dim, dim, bias=True)
        self.l2 = nn.Linear(dim, dim, bias=True)


class ModulatedNorm(_Holder):  # swinv2.py:77-86
    def __init__(self, dim: int, eps: float = 1e-6):
        super().__init__()
        self.norm = nn.LayerNorm(dim, eps)
        self.modulation = nn.Linear(dim, dim * 2, bias=True)


class FeedForward(_Holder):  # swinv2.py:89-102
    def __init__(self, dim, hidden_dim):
        super().__init__()
        self.norm = ModulatedNorm(dim)
        self.w1 = nn.Linear(dim, 2 * hidden_dim, bias=False)
        self.w2 = nn.Linear(hidden_dim, dim, bias=False)


class Attention(_Holder):  # swinv2.py:105-139
    def __init__(self, dim, heads, head_dim, flash=True):
        super().__init__()
        inner = head_dim * heads
        self.heads, self.flash = heads, flash
        self.norm = ModulatedNorm(dim)
        self.to_qkv = nn.Linear(dim, inner * 3, bias=False)
        self.wo = nn.Linear(inner, dim, bias=False)
        self.scale = nn.Parameter(torch.log(10 * torch.ones(1, heads, 1, 1)))


class SwinTransformer(_Holder):  # swinv2.py:142-214
    def __init__(self, depth, dim, heads, window_size, grid_size, shift_size, flash):
        super().__init__()
        self.window_size, self.grid_size, self.shift_size = window_size, grid_size, shift_size
        head_dim = dim // heads
        mlp_dim = int(8 / 3.0 * dim)
        self.layers = nn.Sequential(
            *[nn.ModuleList([Attention(dim, heads, head_dim, flash), FeedForward(dim, mlp_dim)]) for _ in range(depth)])


class PatchEmbedding(_Holder):  # swinv2.py:217-230
    def __init__(self, in_channels, patch_size, dim):
        super().__init__()
        self.patch_size = p1, p2 = patch_size
        self.emb = nn.Linear(in_channels * p1 * p2, dim)


class OutputHead(_Holder):  # swinv2.py:233-247 (index 1 of the Sequential is a parameter-free rearrange there)
    def __init__(self, dim, out_channels, patch_size, grid_size):
        super().__init__()
        p1, p2 = patch_size
        self.head = nn.Sequential(nn.Linear(dim, out_channels * p1 * p2, bias=False), nn.Identity())


class SwinV2(AbstractNetwork):
    def __init__(
        self,
        img_resolution: _Shape2D,
        in_channels: int,
        out_channels: int,
        window_size: _Shape2D,
        shift_size: _Shape2D,
        patch_size: _Shape2D,
        depth: int = 6,
        dim: int = 512,
        heads: int = 12,
        auxiliary_dim: int = 0,
        flash: bool = True,
        logvar: bool = False,
        timestep_weight: float = 1.0,
    ):
        super().__init__(img_resolution, in_channels, out_channels)
        self.image_size = Shape2D(img_resolution).shape
        self.patch_size = Shape2D(patch_size).shape
        self.window_size = Shape2D(window_size).shape
        self.shift_size = Shape2D(shift_size).shape
        gh, gw = self.image_size[0] // self.patch_size[0], self.image_size[1] // self.patch_size[1]
        self.grid_size = (gh, gw)
        self.depth, self.dim, self.heads = depth, dim, heads
        self.mlp_dim = int(8 / 3.0 * dim)
        self.auxiliary_dim = auxiliary_dim
        self.timestep_weight = timestep_weight

        self.pos_embed = nn.Parameter(torch.randn(1, gh * gw, dim) * 0.02)
        self.patch_embed = PatchEmbedding(in_channels, self.patch_size, dim)
        self.latent_embed = LatentEmbedding(dim)
        self.logvar_embed = nn.Linear(dim, 1) if logvar else None
        self.auxiliary_embed = nn.Linear(auxiliary_dim, dim) if auxiliary_dim else None
        self.transformer = SwinTransformer(depth, dim, heads, self.window_size, self.grid_size, self.shift_size, flash)
        self.head = OutputHead(dim, out_channels, self.patch_size, self.grid_size)
        self._init_weights()
        self._engines = {}

    def _init_weights(self):
        """trunc-normal(0.02) Linears, zero ``modulation``/``head`` and biases (swinv2.py:295-303)."""
        for name, m in self.named_modules():
            if isinstance(m, nn.Linear):
                if "modulation" in name or "head" in name:
                    nn.init.zeros_(m.weight)
                else:
                    nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def __deepcopy__(self, memo):
        """EMA copies (trainer.py:87) must not drag the device-side engines (ctypes descriptors) along."""
        import copy
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k not in ("_engines", "_train_engine"):
                new.__dict__[k] = copy.deepcopy(v, memo)
        new.__dict__["_engines"] = {}
        return new

    # ------------------------------------------------------------------ engine plumbing
    @staticmethod
    def compute_dtype(device_type: str = "cuda") -> torch.dtype:
        if torch.is_autocast_enabled(device_type) and torch.get_autocast_dtype(device_type) == torch.bfloat16:
            return torch.bfloat16
        return torch.float32

    def engine(self, dtype=None) -> SwinEngine:
        """The engine of a compute dtype: bf16 under bf16 autocast, else the exact-fp32 engine -- or, when
        ``SWIFTK_FP32_ENGINE=bf16x3`` (or ``module.fp32_engine = "bf16x3"``), the split-bf16 engine in its place: fp32
        activations, every GEMM as three bf16 MFMA products (about twice the exact engine's throughput; parity with the
        reference measured at a few 1e-5 instead of 1e-5, tests/test_gpu_model.py)."""
        dtype = dtype or self.compute_dtype()
        if dtype == torch.float32 and (getattr(self, "fp32_engine", None) or os.environ.get("SWIFTK_FP32_ENGINE", "exact")) == "bf16x3":
            dtype = "bf16x3"
        if dtype not in self._engines:
            self._engines[dtype] = SwinEngine(self, dtype)
        return self._engines[dtype]

    def _prep_t(self, t: torch.Tensor, B: int) -> torch.Tensor:
        if t.dim() == 0 or (t.dim() == 1 and t.size(0) == 1):  # swinv2.py:316-317
            t = t.reshape(1).repeat(B)
        return t

    def forward_sources(self, srcs: Sequence[torch.Tensor], scales: Sequence[float], t: torch.Tensor,
                        auxiliary: Optional[torch.Tensor] = None, return_logvar: bool = False, xt=None, alpha=None,
                        beta=None, dtype: Optional[torch.dtype] = None, src0_scale: Optional[torch.Tensor] = None):
        """Network on the channel-concatenation of ``srcs`` without materialising the concat (``src0_scale``: an extra
        per-sample [B] factor on ``srcs[0]``, applied in the patch gather)."""
        B = srcs[0].shape[0]
        t = self._prep_t(t, B)
        aux = None
        if self.auxiliary_embed is not None and auxiliary is not None:
            aux = auxiliary.to(torch.float32)
            if aux.shape[0] == 1 and B > 1:  # precond.py:25 hands a [1, aux_dim] zero row when auxiliary is None
                aux = aux.expand(B, -1)
        want_lv = bool(self.logvar_embed is not None and return_logvar)
        return self.engine(dtype).forward(srcs, scales, t, aux, xt=xt, alpha=alpha, beta=beta, want_logvar=want_lv,
                                          src0_scale=src0_scale)

    def forward(self, x: torch.Tensor, t: torch.Tensor, auxiliary: Optional[torch.Tensor] = None, jvp: bool = False,
                return_logvar: bool = False):
        """x [B, in_channels, H, W], t [B] (or scalar), auxiliary [B, aux_dim] -> [B, out_channels, H, W].

        ``jvp`` only selects between two mathematically identical attention code paths in the
        reference (swinv2.py:129-134); the fused kernel serves both.
        """
        return self.forward_sources([x], [1.0], t, auxiliary, return_logvar=return_logvar)
