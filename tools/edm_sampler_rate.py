#!/usr/bin/env python
"""EDM sampler rate against dpm_solver_2s at the Swift-B shape (12 heads of 88): N = 20 steps each, i.e. 39 network
evaluations per sample-step for both.  The two solvers alternate in one process, timed with device events after a warm-up,
at 1 and 8 units per batch, for the bf16 and the bf16x3 engines.  Prints one JSON line per cell and a summary line.

    python tools/edm_sampler_rate.py [--reps 3] [--units 1,8] [--dtypes bf16,bf16x3] [--heads 12]

``--heads 16`` is the reference's EDM model (16 heads of 66): it needs SWIFTK_PAD_HEADS=1 in the environment and runs each head
on 80 lanes; its rate against ``--heads 12`` at the same depth and units is what the padded lanes cost.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from swift_amd.generating.factory import sampler_factory  # noqa: E402
from swift_amd.models.precond import EDMPrecond, PassPrecond  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--units", default="1,8")
ap.add_argument("--dtypes", default="bf16,bf16x3")
ap.add_argument("--num-steps", type=int, default=20)
ap.add_argument("--heads", type=int, default=12)
a = ap.parse_args()

NV, NF, IMG = 69, 3, [128, 256]
mcfg = dict(_target_="swift.models.swinv2.SwinV2", window_size=[16, 16], shift_size=[8, 8], patch_size=[2, 2], depth=12,
            dim=1056, heads=a.heads)
torch.manual_seed(0)
edm = EDMPrecond(mcfg, IMG, NV, NV + NF, auxiliary_dim=1)
for p in edm.parameters():  # (the zero-initialised head would make F = 0: give every weight a value)
    with torch.no_grad():
        p.add_(torch.randn_like(p) * 0.02)
tf = PassPrecond(mcfg, IMG, NV, NV + NF, auxiliary_dim=1)
tf.load_state_dict(edm.state_dict())
edm, tf = edm.cuda().eval(), tf.cuda().eval()
dts = {"bf16": torch.bfloat16, "bf16x3": "bf16x3", "f32": torch.float32}
N = a.num_steps
rows = []
for dname in a.dtypes.split(","):
    dt = dts[dname]
    for B in (int(u) for u in a.units.split(",")):
        cond = torch.randn(B, NV + NF, *IMG, device="cuda")
        lat = torch.randn(B, NV, *IMG, device="cuda")
        samplers = {
            "edm": sampler_factory("edm", edm, denoise_dtype=dt, num_steps=N, sigma_min=0.03, sigma_max=80.0, rho=7, S_churn=2.5,
                                   S_min=0.75, S_max=80, S_noise=1.05, auxiliary=0.6),
            "2s": sampler_factory("2s", tf, denoise_dtype=dt, num_steps=N, sigma_min=0.02, sigma_max=200.0, auxiliary=0.6),
        }
        for s in samplers.values():  # warm-up: weight packing, workspaces
            s(cond, latents=lat)
        ms = {k: [] for k in samplers}
        for _ in range(a.reps):
            for k, s in samplers.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                s(cond, latents=lat)
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        rate = {k: B * 1000.0 / sorted(v)[len(v) // 2] for k, v in ms.items()}
        row = dict(dtype=dname, heads=a.heads, units=B, num_steps=N, evaluations=2 * N - 1, edm_rate=round(rate["edm"], 3),
                   dpm2s_rate=round(rate["2s"], 3), ratio=round(rate["edm"] / rate["2s"], 4), unit="sample-steps/s")
        rows.append(row)
        print(json.dumps(row), flush=True)
print(json.dumps(dict(summary="edm / dpm_solver_2s", worst_ratio=min(r["ratio"] for r in rows))))
