#!/usr/bin/env python
"""Persistent bf16 GEMM outside its k-loop: A/B of tuning key 31 (bit 0 = straight-line epilogue of interior tiles, bit 1 =
incremental tile walk) on the four Swift-B GEMM shapes of tools/gemm_ab.py.  Key 31 = 0 is the old arm and the reference.  All arms
run interleaved in one process, the order reversed every other round; per shape and arm: median, min and max of the rounds, whether
the output equals arm 0's bit for bit, and the criterion "the slowest round of the arm beats the fastest round of the old arm".
(to_qkv's tiled QKNORM epilogue does not take the new forms: its rows are the control.)
usage: gemm_epilogue_probe.py [units] [rounds]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from swift_amd import _lib
dev = torch.device("cuda"); L = _lib.lib()
B = int(sys.argv[1]) if len(sys.argv) > 1 else 96
R = int(sys.argv[2]) if len(sys.argv) > 2 else 9
ARMS = (0, 1, 2, 3)
M = B * 8192
st = lambda: torch.cuda.current_stream().cuda_stream
torch.manual_seed(0)
scale = torch.full((12,), 2.3, device=dev)
shipped = L.swiftk_get_tuning(31)
shapes = [("qkv_tiled", 3168, 1088, 1056, "tiled"), ("wo", 1056, 1088, 1056, _lib.EPI_NONE),
          ("w1+swiglu", 5632, 1088, 1056, _lib.EPI_SWIGLU), ("w2", 1056, 2816, 2816, _lib.EPI_NONE)]
for sname, N, K, Kalg, epi in shapes:
    a = torch.randn(M, K, device=dev).bfloat16(); a[:, Kalg:] = 0
    w = (torch.randn(N, K, device=dev) * 0.03).bfloat16(); w[:, Kalg:] = 0
    ncol = N // 2 if epi == _lib.EPI_SWIGLU else N
    outs = {n: torch.zeros(M, ncol, dtype=torch.bfloat16, device=dev) for n in ARMS}

    def run(n):
        L.swiftk_set_tuning(31, n)
        try:
            if epi == "tiled":
                rc = L.swiftk_gemm_qkv_tiled(a.data_ptr(), K, w.data_ptr(), K, outs[n].data_ptr(), Kalg, scale.data_ptr(), B, 64, 128, 12, 88, 8, 8, st())
            else:
                rc = L.swiftk_gemm(a.data_ptr(), K, w.data_ptr(), K, outs[n].data_ptr(), ncol, M, N, Kalg, _lib.BF16, _lib.BF16, epi, None, None, 0, st())
        finally:
            L.swiftk_set_tuning(31, shipped)
        assert rc == 0, (n, sname, rc)

    res = {n: [] for n in ARMS}
    for rnd in range(R):
        for n in (ARMS if rnd % 2 == 0 else ARMS[::-1]):
            run(n); torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(6): run(n)
            e1.record(); torch.cuda.synchronize(); res[n].append(e0.elapsed_time(e1) / 6)
    flop = 2.0 * M * N * Kalg
    old = sorted(res[0])
    for n in ARMS:
        t = sorted(res[n]); med = t[len(t) // 2]
        same = bool(torch.equal(outs[n].view(torch.int16), outs[0].view(torch.int16)))
        print(f"{sname:10s} key 31 = {n}  median {med*1e3:8.1f} us  min {t[0]*1e3:8.1f} us  max {t[-1]*1e3:8.1f} us  {100*(med/old[len(old)//2]-1):+6.2f} %  "
              f"{flop/med/1e9:7.1f} TFLOP/s  equal to key 31 = 0: {same}  slowest < old arm's fastest: {t[-1] < old[0]}   ({B} units)", flush=True)
print(f"shipped default: key 31 = {shipped}")
