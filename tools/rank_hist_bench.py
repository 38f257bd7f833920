"""Time the ``swiftk_rank_histogram`` call that ``swift_amd.generate --rank-hist`` adds, at the size of one lead step of the
flagship job (8 ICs x 12 members, 69 variables at 128 x 256), against the torch formulation of the same histogram:

    python tools/rank_hist_bench.py [--ics 8] [--members 12] [--channels 69] [--grid 128 256] [--reps 25] [--out FILE.json]

    kernel   rank_histogram(pred [ICs, members, V, H, W], y [ICs, V, H, W], lat)        one launch, [ICs, V, members + 1] fp64
    torch    b = (pred < y[:, None]).sum(1); one_hot(b, members + 1) in fp64; weighted sum over (H, W)   (ties ignored)

Both are timed with HIP events, ``--reps`` times after two warm-up calls, in the same process on the same Gaussian fields.  On
tie-free input they must give the same histogram (checked before timing); at the default size 2e8 fp32 normal draws hold a
handful of exact ties, which the torch formulation puts into bin b alone -- their count and the largest relative difference
between the two histograms are reported instead.  Reported: medians and extremes in milliseconds, the
bytes the kernel has to read ((members + 1) * 4 per pixel) and the rate that makes, the floor of those bytes at ``--copy-tbs``
(default 6.29 TB/s, the device's measured copy rate), the share of the forecast step ``--step-ms`` (default 251.5,
profiles/r05m_bench_b96.json) and the ratio torch / kernel.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from swift_amd.eval.metrics import rank_histogram  # noqa: E402


def torch_histogram(pred, y, w_lat):
    """The tie-free histogram in torch: comparison, one-hot, weighted sum.  [I, V, N + 1] fp64."""
    N = pred.shape[1]
    b = (pred < y[:, None]).sum(1)                                                   # [I, V, H, W] int64
    return torch.einsum("ivhwr,h->ivr", torch.nn.functional.one_hot(b, N + 1).to(torch.float64), w_lat)


def timed(fn, reps):
    fn(), fn()  # warm-up: code object, tables, allocator
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ics", type=int, default=8)
    ap.add_argument("--members", type=int, default=12)
    ap.add_argument("--channels", type=int, default=69)
    ap.add_argument("--grid", type=int, nargs=2, default=[128, 256])
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--step-ms", type=float, default=251.5)
    ap.add_argument("--copy-tbs", type=float, default=6.29)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps: at least 20 (the figure quoted is a median)")
    if not torch.cuda.is_available():
        raise SystemExit("rank_hist_bench.py measures on the GPU: none found")
    dev = torch.device("cuda")
    I, N, V, (H, W) = a.ics, a.members, a.channels, a.grid
    g = torch.Generator(device=dev).manual_seed(0)
    pred = torch.randn(I, N, V, H, W, device=dev, generator=g)
    truth = torch.randn(I, V, H, W, device=dev, generator=g)
    lat = -90.0 + (np.arange(H) + 0.5) * (180.0 / H)
    w = np.cos(np.deg2rad(lat))
    w_lat = torch.from_numpy(w / w.mean()).to(dev)
    ours, theirs = rank_histogram(pred, truth, lat), torch_histogram(pred, truth, w_lat)
    torch.cuda.synchronize()
    ties = int((pred == truth[:, None]).sum())
    rel = float(((ours - theirs).abs() / theirs.clamp_min(1e-300)).max())
    if ties == 0 and rel > 1e-12:
        raise SystemExit(f"kernel and torch formulation disagree on tie-free fields: {rel:.3e} relative")
    res = dict(shape=dict(ics=I, members=N, V=V, H=H, W=W, planes=I * V), reps=a.reps, device=torch.cuda.get_device_name(0),
               ties_in_input=ties, max_rel_difference_kernel_vs_torch=rel)
    k_med, k_min, k_max = timed(lambda: rank_histogram(pred, truth, lat), a.reps)
    t_med, t_min, t_max = timed(lambda: torch_histogram(pred, truth, w_lat), a.reps)
    nbytes = I * V * H * W * (N + 1) * 4
    res["kernel"] = dict(ms_median=round(k_med, 4), ms_min=round(k_min, 4), ms_max=round(k_max, 4), bytes_read=nbytes,
                         TB_per_s_at_median=round(nbytes / (k_med * 1e-3) / 1e12, 3),
                         byte_floor_ms=round(nbytes / (a.copy_tbs * 1e12) * 1e3, 4), copy_rate_TB_per_s=a.copy_tbs)
    res["torch"] = dict(ms_median=round(t_med, 4), ms_min=round(t_min, 4), ms_max=round(t_max, 4))
    res["torch_over_kernel"] = round(t_med / k_med, 2)
    res["forecast_step_ms"] = a.step_ms
    res["share_of_forecast_step"] = round(k_med / a.step_ms, 5)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
