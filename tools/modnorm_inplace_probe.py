#!/usr/bin/env python
"""The packed pair ModulatedNorm at the bench shape (units x 8192 rows x 1056) in place (swiftk_modnorm_residual_pair) against the
same kernel writing the new hi to another buffer (swiftk_modnorm_residual_pair_to), and a device copy of hi for scale; interleaved
rounds in one process, the order reversed every other round (profiles/r10a_modnorm_rowstats.txt, part B).
usage: modnorm_inplace_probe.py [units] [rounds]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from swift_amd import ops, _lib
dev = torch.device("cuda"); L = _lib.lib()
B = int(sys.argv[1]) if len(sys.argv) > 1 else 96
R = int(sys.argv[2]) if len(sys.argv) > 2 else 9
M, d, ld, rps = B * 8192, 1056, 1088, 8192
st = lambda: torch.cuda.current_stream().cuda_stream
torch.manual_seed(0)
y = torch.randn(M, d, device=dev).bfloat16()
gamma, beta = 1 + 0.1 * torch.randn(d, device=dev), 0.1 * torch.randn(d, device=dev)
mod = 0.3 * torch.randn(B, 48 * d, device=dev)[:, 4 * d:6 * d]
hi, lo = ops.split_pair(torch.randn(M, d, device=dev), ld, 8)
hi2 = torch.zeros_like(hi)
def inplace():
    assert L.swiftk_modnorm_residual_pair(y.data_ptr(), d, hi.data_ptr(), ld, lo.data_ptr(), d, 8, gamma.data_ptr(), beta.data_ptr(), mod.data_ptr(), mod.stride(0), M, d, rps, 1e-6, st()) == 0
def outofplace():
    assert L.swiftk_modnorm_residual_pair_to(y.data_ptr(), d, hi.data_ptr(), hi2.data_ptr(), ld, lo.data_ptr(), d, 8, gamma.data_ptr(), beta.data_ptr(), mod.data_ptr(), mod.stride(0), M, d, rps, 1e-6, st()) == 0
def copy():
    hi2.copy_(hi)
res = {"in place": [], "hi out of place": [], "torch copy of hi (2 x 1.7 GB)": []}
fns = dict(zip(res, (inplace, outofplace, copy)))
for rnd in range(R):
    order = list(res)
    for name in (order if rnd % 2 == 0 else order[::-1]):
        fn = fns[name]; fn(); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(4): fn()
        e1.record(); torch.cuda.synchronize(); res[name].append(e0.elapsed_time(e1) / 4)
for name, t in res.items():
    t = sorted(t); med = t[len(t) // 2]
    byt = M * d * 8.0 if "place" in name else 2.0 * M * ld * 2
    print(f"{name}: median {med*1e3:8.1f} us  min {t[0]*1e3:8.1f}  max {t[-1]*1e3:8.1f}  {byt/med/1e9:6.2f} TB/s", flush=True)
