"""Time the ``swiftk_ensemble_maps`` call that ``swift_amd.generate --maps`` adds, at the size of one lead step of the flagship
job (8 ICs x 12 members, 69 variables at 128 x 256) and at 64 members, against the torch formulation of the same four maps:

    python tools/maps_bench.py [--ics 8] [--members 12 64] [--channels 69] [--grid 128 256] [--reps 25] [--out FILE.json]

    kernel   ensemble_maps(pred [ICs, members, V, H, W], y [ICs, V, H, W], acc)       one launch, acc [ICs, 4, V, H, W] fp64 += terms
    torch    x = pred.double(): mean(1) - y, its square, |x - y|.mean(1) - sum_m |x[m+1:] - x[m]|.sum(1) / (N (N - 1)), x.var(1),
             stacked and added to acc   (fp64 throughout, the pair sum member by member: the [N, N] difference tensor of the
             reference's CRPS would take 21 GB at 12 members and 593 GB at 64)

Both are timed with HIP events, ``--reps`` times after two warm-up calls, in the same process on the same fields: 280 + 1e-2 x
Gaussian noise around a per-pixel centre, a temperature under a small spread.  Before timing the two results are compared
(largest difference per statistic relative to the statistic's largest magnitude: re-associated fp64 sums).  The timed kernel
call accumulates, as every IC after a rank's first does; the first IC's call, which only writes acc, is timed beside it.
Reported per ensemble size: medians and extremes in milliseconds, the bytes the call has to move ((members + 1) * 4 read and 64
read and written per pixel; 32 without the read of acc) and the rate that makes, the floor of those bytes at ``--copy-tbs``
(default 6.29 TB/s, the device's measured copy rate), the share of the forecast step ``--step-ms`` (default 251.5,
profiles/r05m_bench_b96.json) and the ratio torch / kernel.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from swift_amd.eval.metrics import ensemble_maps  # noqa: E402


def torch_maps(pred, y, acc):
    """The four maps in torch fp64, added to acc [I, 4, V, H, W]."""
    N = pred.shape[1]
    x, t = pred.double(), y.double()
    e = x.mean(1) - t
    a = (x - t[:, None]).abs().mean(1)
    p = torch.zeros_like(t)
    for m in range(N - 1):
        p += (x[:, m + 1:] - x[:, m:m + 1]).abs().sum(1)
    return acc.add_(torch.stack([e, e * e, a - p / (N * (N - 1)), x.var(1)], 1))


def timed(fn, reps):
    fn(), fn()  # warm-up: code object, allocator
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ics", type=int, default=8)
    ap.add_argument("--members", type=int, nargs="+", default=[12, 64])
    ap.add_argument("--channels", type=int, default=69)
    ap.add_argument("--grid", type=int, nargs=2, default=[128, 256])
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--step-ms", type=float, default=251.5)
    ap.add_argument("--copy-tbs", type=float, default=6.29)
    ap.add_argument("--no-torch", action="store_true", help="time the kernel only (sweeps over the ensemble size)")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps: at least 20 (the figure quoted is a median)")
    if not torch.cuda.is_available():
        raise SystemExit("maps_bench.py measures on the GPU: none found")
    dev = torch.device("cuda")
    I, V, (H, W) = a.ics, a.channels, a.grid
    pixels = I * V * H * W
    res = dict(shape=dict(ics=I, V=V, H=H, W=W, pixels=pixels), reps=a.reps, device=torch.cuda.get_device_name(0),
               fields="280 + 1e-2 x normal about a per-pixel centre", forecast_step_ms=a.step_ms, copy_rate_TB_per_s=a.copy_tbs,
               members={})
    for N in a.members:
        g = torch.Generator(device=dev).manual_seed(N)
        centre = 280.0 + 1e-2 * torch.randn(I, V, H, W, device=dev, generator=g)
        pred = centre[:, None] + 1e-2 * torch.randn(I, N, V, H, W, device=dev, generator=g)
        y = centre + 1e-2 * torch.randn(I, V, H, W, device=dev, generator=g)
        del centre
        acc = ensemble_maps(pred, y)
        r = dict()
        if not a.no_torch:
            theirs = torch_maps(pred, y, torch.zeros_like(acc))
            torch.cuda.synchronize()
            r["max_difference_torch_vs_kernel_over_max_magnitude"] = {
                s: float((acc[:, k] - theirs[:, k]).abs().max() / acc[:, k].abs().max()) for k, s in enumerate(("bias", "mse", "crps", "variance"))}
            if max(r["max_difference_torch_vs_kernel_over_max_magnitude"].values()) > 1e-9:
                raise SystemExit(f"kernel and torch formulation disagree at {N} members: {r}")
            del theirs
        nbytes, nbytes_w = pixels * ((N + 1) * 4 + 64), pixels * ((N + 1) * 4 + 32)
        k = timed(lambda: ensemble_maps(pred, y, acc), a.reps)
        floor = nbytes / (a.copy_tbs * 1e12) * 1e3
        k.update(bytes_moved=nbytes, TB_per_s_at_median=round(nbytes / (k["ms_median"] * 1e-3) / 1e12, 3), byte_floor_ms=round(floor, 4),
                 over_byte_floor=round(k["ms_median"] / floor, 2))
        r["kernel"] = k
        w = timed(lambda: ensemble_maps(pred, y), a.reps)   # (allocates its result like the job's first call; the allocator is warm)
        floor_w = nbytes_w / (a.copy_tbs * 1e12) * 1e3
        w.update(bytes_moved=nbytes_w, byte_floor_ms=round(floor_w, 4), over_byte_floor=round(w["ms_median"] / floor_w, 2))
        r["kernel_first_ic"] = w
        r["share_of_forecast_step"] = round(k["ms_median"] / a.step_ms, 5)
        if not a.no_torch:
            r["torch"] = timed(lambda: torch_maps(pred, y, acc), a.reps)
            r["torch_over_kernel"] = round(r["torch"]["ms_median"] / k["ms_median"], 2)
        res["members"][str(N)] = r
        del pred, y, acc
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
