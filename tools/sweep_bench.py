"""Time ``swiftk_sweep_sse`` against the two-kernel route it replaces for the sampler sweep's scoring,
``swiftk_rollout_update`` (forecast in physical units) followed by ``swiftk_rmse_sums`` against a physical truth:

    python tools/sweep_bench.py [--batch 32] [--channels 69] [--rounds 9] [--iters 200] [--out FILE.json]

HIP events around ``--iters`` back-to-back calls per window, the two routes alternating window by window (``--rounds`` windows
each, after a warm-up window of each); medians and extremes are reported.  Bytes per element, counted from the shapes:
sweep_sse reads x, y, t = 12 B; the pair reads x, y and writes phys, x (16 B), then reads phys and the truth (8 B) = 24 B --
plus, once per batch and not timed here, 16 B to bring the truth into physical units, and the clear of its fp32 sums, which
is timed.  The fraction of the 6.29 TB/s copy rate is bytes / time / 6.29e12.  The pair's sums are fp32 atomics over the
whole batch (not reproducible, not per sample); the comparison is of time only.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from swift_amd import _lib, ops  # noqa: E402

COPY_RATE = 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--channels", type=int, default=69)
    ap.add_argument("--forcings", type=int, default=3)
    ap.add_argument("--grid", type=int, nargs=2, default=[128, 256])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sweep_bench.py measures on the GPU: none found")
    dev = torch.device("cuda")
    B, C, (H, W) = a.batch, a.channels, a.grid
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, C + a.forcings, H, W, device=dev, generator=g)
    y, t = (torch.randn(B, C, H, W, device=dev, generator=g) for _ in range(2))
    mx, sx, st = torch.randn(C, device=dev, generator=g), torch.rand(C, device=dev, generator=g) + 0.5, torch.rand(C, device=dev, generator=g) * 0.1 + 0.05
    w64 = torch.cos(torch.deg2rad(torch.linspace(-89.3, 89.3, H, dtype=torch.float64)))
    w64 = (w64 / w64.mean()).to(dev)
    w32 = w64.float()
    out = torch.empty(B, C, dtype=torch.float64, device=dev)
    xc = x[:, :C].contiguous()          # the pair updates its state in place: a contiguous [B, C, H, W] copy
    x0 = xc.clone()
    phys, truth = torch.empty_like(y), torch.randn(B, C, H, W, device=dev, generator=g)
    sq = torch.empty(1 + C, device=dev)
    L, s = _lib.lib(), torch.cuda.current_stream().cuda_stream

    def fused():
        ops.sweep_sse(x, y, t, mx, sx, st, w64, out=out)

    def pair():
        ops.rollout_update(xc, y, mx, sx, st, phys=phys)
        ops.zero_acc_(sq)
        _lib.check(L.swiftk_rmse_sums(phys.data_ptr(), truth.data_ptr(), truth.stride(0), w32.data_ptr(), sq.data_ptr(), B, C, H, W, s),
                   "swiftk_rmse_sums")

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters * 1e3  # microseconds per call

    times = {"sweep_sse": [], "update_plus_rmse_sums": []}
    window(fused), window(pair)  # warm-up: code objects, allocator
    for _ in range(a.rounds):
        times["sweep_sse"].append(window(fused))
        xc.copy_(x0)  # (the pair's state would otherwise drift: x <- x + y st / sx every call)
        times["update_plus_rmse_sums"].append(window(pair))
    n = B * C * H * W
    res = dict(shape=dict(B=B, C=C, H=H, W=W, x_channels=C + a.forcings), iters_per_window=a.iters, rounds=a.rounds,
               bytes_per_element=dict(sweep_sse=12, update_plus_rmse_sums=24), copy_rate_TBps=COPY_RATE / 1e12)
    for k, v in times.items():
        med = statistics.median(v)
        byts = n * res["bytes_per_element"][k]
        res[k] = dict(us_median=round(med, 2), us_min=round(min(v), 2), us_max=round(max(v), 2),
                      TBps_at_median=round(byts / (med * 1e-6) / 1e12, 3), fraction_of_copy_rate=round(byts / (med * 1e-6) / COPY_RATE, 3))
    res["time_ratio_pair_over_sweep_sse"] = round(res["update_plus_rmse_sums"]["us_median"] / res["sweep_sse"]["us_median"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
