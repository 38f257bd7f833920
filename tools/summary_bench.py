"""Time the ``swiftk_ensemble_summary`` call that ``swift_amd.generate --summary`` adds, at the size of one lead step of the
flagship job (8 ICs x 12 members, 69 variables at 128 x 256, 3 quantiles), against the torch formulation of the same statistics:

    python tools/summary_bench.py [--ics 8] [--members 12] [--channels 69] [--grid 128 256] [--quantiles 0.1 0.5 0.9] [--reps 25] [--out FILE.json]

    kernel   ensemble_summary(pred [ICs, members, V, H, W], quantiles)      one launch, [ICs, 2 + Q, V, H, W] fp32
    torch    pred.mean(1), pred.std(1), torch.quantile(pred, q, dim=1)      fp32 throughout

``torch.quantile`` refuses inputs above 16 M elements (the default size has 217 M); then its definition stands in for it -- one
``torch.sort`` over the members and a ``lerp`` between the two neighbours of each quantile -- and the result line says so.  Both
sides are timed with HIP events, ``--reps`` times after two warm-up calls, in the same process on the same fields: 280 + 1e-2 x
Gaussian noise, a temperature under a small spread, where the largest difference between the two spreads relative to the
kernel's is reported next to the times (the fp32 formulation loses the spread's digits there: DESIGN 8e).  Reported: medians and
extremes in milliseconds, the bytes the kernel moves (4 N read and 4 (2 + Q) written per pixel) and the rate that makes, the floor
of those bytes at ``--copy-tbs`` (default 6.29 TB/s, the device's measured copy rate), the share of the forecast step
``--step-ms`` (default 251.5, profiles/r05m_bench_b96.json) and the ratio torch / kernel.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from swift_amd.eval.metrics import ensemble_summary, quantile_table  # noqa: E402


def torch_summary(pred, quantiles, use_quantile):
    """The torch one-liners, fp32: [I, 2 + Q, V, H, W]."""
    N = pred.shape[1]
    parts = [pred.mean(1), pred.std(1)]
    if use_quantile:
        parts += list(torch.quantile(pred, torch.tensor(quantiles, device=pred.device), dim=1))
    elif quantiles:
        xs = torch.sort(pred, dim=1).values
        lo, frac = quantile_table(quantiles, N)
        parts += [torch.lerp(xs[:, int(l)], xs[:, min(int(l) + 1, N - 1)], float(g)) for l, g in zip(lo, frac)]
    return torch.stack(parts, 1)


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
    ap.add_argument("--quantiles", type=float, nargs="*", default=[0.1, 0.5, 0.9])
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--step-ms", type=float, default=251.5)
    ap.add_argument("--copy-tbs", type=float, default=6.29)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps: at least 20 (the figure quoted is a median)")
    if not torch.cuda.is_available():
        raise SystemExit("summary_bench.py measures on the GPU: none found")
    dev = torch.device("cuda")
    I, N, V, (H, W), qs = a.ics, a.members, a.channels, a.grid, tuple(a.quantiles)
    Q = len(qs)
    g = torch.Generator(device=dev).manual_seed(0)
    pred = 280.0 + 1e-2 * torch.randn(I, N, V, H, W, device=dev, generator=g)
    use_quantile = pred.numel() <= 16_000_000
    ours, theirs = ensemble_summary(pred, qs), torch_summary(pred, qs, use_quantile)
    torch.cuda.synchronize()
    rel = lambda k: float(((ours[:, k] - theirs[:, k]).abs() / ours[:, k].abs().clamp_min(1e-30)).max())
    res = dict(shape=dict(ics=I, members=N, V=V, H=H, W=W, quantiles=list(qs), pixels=I * V * H * W), reps=a.reps,
               device=torch.cuda.get_device_name(0), fields="280 + 1e-2 x normal",
               torch_quantiles="torch.quantile" if use_quantile else "torch.sort + lerp (torch.quantile refuses more than 16 M elements)",
               max_rel_difference_torch_vs_kernel=dict(mean=rel(0), spread=rel(1), quantiles=max([rel(2 + j) for j in range(Q)] or [0.0])))
    del theirs
    k_med, k_min, k_max = timed(lambda: ensemble_summary(pred, qs), a.reps)
    t_med, t_min, t_max = timed(lambda: torch_summary(pred, qs, use_quantile), a.reps)
    nbytes = I * V * H * W * (N + 2 + Q) * 4
    res["kernel"] = dict(ms_median=round(k_med, 4), ms_min=round(k_min, 4), ms_max=round(k_max, 4), bytes_moved=nbytes,
                         TB_per_s_at_median=round(nbytes / (k_med * 1e-3) / 1e12, 3),
                         byte_floor_ms=round(nbytes / (a.copy_tbs * 1e12) * 1e3, 4), copy_rate_TB_per_s=a.copy_tbs,
                         over_byte_floor=round(k_med / (nbytes / (a.copy_tbs * 1e12) * 1e3), 2))
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
