#!/usr/bin/env python
"""refresh() + one backward of SwinTrainEngine at 16 heads of 66, depth 12, on padded head lanes: HIP-event medians of 15 timed rounds
after 4 warm-up rounds (every round bumps the parameter versions, so refresh() rebuilds every operand; the backward is the replayed
HIP graph).  One JSON line per run; for an A/B of two trees run it alternately with PYTHONPATH on either:
    SWIFTK_PAD_HEADS=1 PYTHONPATH=<tree> python tools/lane_kernels_ab.py <tag>"""
import json, os, statistics, sys
if not os.environ.get("PYTHONPATH"):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import swift_amd
from swift_amd.models.precond import PassPrecond
from swift_amd.train_engine import SwinTrainEngine
from swift_amd.utils.detinit import swinv2_state

tag = sys.argv[1]
dev = torch.device("cuda", 0)
depth, dim, heads, img = 12, 1056, 16, (64, 64)
mcfg = dict(_target_="swift.models.swinv2.SwinV2", window_size=[16, 16], shift_size=[8, 8], patch_size=[2, 2], depth=depth, dim=dim, heads=heads)
net = PassPrecond(mcfg, img_resolution=list(img), img_channels=69, condition_channels=72, auxiliary_dim=1)
net.load_state_dict(swinv2_state(grid=(32, 32), in_channels=141, out_channels=69, patch_size=(2, 2), depth=depth, dim=dim, heads=heads, seed=3))
net = net.to(dev)
eng = SwinTrainEngine(net.model)
B = 2
g = torch.Generator(device=dev).manual_seed(0)
x = torch.randn(B, 69, *img, generator=g, device=dev); c = torch.randn(B, 72, *img, generator=g, device=dev)
t = torch.tensor([0.5, 1.2], device=dev); aux = torch.tensor([[0.6], [0.6]], device=dev)
R = torch.randn(B, 69, *img, generator=g, device=dev)
params = list(net.parameters())

def ev():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

def bump():
    with torch.no_grad():
        for p in params:
            p.add_(0.0)  # new parameter version: the next refresh() rebuilds every operand

def one(timed=True):
    bump()
    torch.cuda.synchronize()
    e0, e1 = ev(); e0.record(); eng.refresh(); e1.record()
    out, ctx = eng.forward([x, c], [1.0, 1.0], t, aux)
    torch.cuda.synchronize()
    b0, b1 = ev(); b0.record(); eng.backward(ctx, R); b1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), b0.elapsed_time(b1)

for _ in range(4):  # warm-up: allocator, graph capture, first replay
    one()
rs = [one() for _ in range(15)]
ref, bwd = [r[0] for r in rs], [r[1] for r in rs]
tot = [a + b for a, b in rs]
q = lambda v: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v))
gsum = float(sum(p.grad.double().abs().sum() for p in params if p.grad is not None))
print(json.dumps(dict(tree=tag, refresh=q(ref), backward=q(bwd), refresh_plus_backward=q(tot), hd=(eng.hd0, eng.hd), grad_abs_sum=gsum)), flush=True)
