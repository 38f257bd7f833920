"""Time the three ``swiftk_zonal_power`` calls that ``swift_amd.generate --spectra`` adds per lead step, at the size of one
forecast step of the flagship job (96 units = 8 ICs x 12 members, 69 variables at 128 x 256):

    python tools/spectra_bench.py [--ics 8] [--members 12] [--channels 69] [--grid 128 256] [--reps 25] [--out FILE.json]

    member         n = ICs * members, G = 1        (the members' own spectra)
    ensemble_mean  n = ICs,           G = members  (the spectrum of the ensemble mean)
    truth          n = ICs,           G = 1        (the verifying fields)

Each call is timed on its own with HIP events, ``--reps`` times after two warm-up calls; medians and extremes are reported in
milliseconds, with the fp64 multiply-adds the direct transform needs (2 per (row, wavenumber below W/2, longitude), counted
from the shapes) and the rate that makes.  No share of a peak: the fp64 vector peak of the MI355X has not been measured here.
``--step-ms`` (default 251.5, profiles/r05m_bench_b96.json) is the forecast step the total is set against.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from swift_amd.eval.metrics import zonal_power  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ics", type=int, default=8)
    ap.add_argument("--members", type=int, default=12)
    ap.add_argument("--channels", type=int, default=69)
    ap.add_argument("--grid", type=int, nargs=2, default=[128, 256])
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--step-ms", type=float, default=251.5)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps: at least 20 (the figure quoted is a median)")
    if not torch.cuda.is_available():
        raise SystemExit("spectra_bench.py measures on the GPU: none found")
    dev = torch.device("cuda")
    I, N, V, (H, W) = a.ics, a.members, a.channels, a.grid
    g = torch.Generator(device=dev).manual_seed(0)
    pred = torch.randn(I, N, V, H, W, device=dev, generator=g)
    truth = torch.randn(I, V, H, W, device=dev, generator=g)
    lat = -90.0 + (np.arange(H) + 0.5) * (180.0 / H)
    calls = {"member": lambda: zonal_power(pred.view(I * N, V, H, W), lat),
             "ensemble_mean": lambda: zonal_power(pred, lat, group=N),
             "truth": lambda: zonal_power(truth, lat)}
    planes = {"member": I * N * V, "ensemble_mean": I * V, "truth": I * V}
    res = dict(shape=dict(ics=I, members=N, units=I * N, V=V, H=H, W=W), reps=a.reps, device=torch.cuda.get_device_name(0))
    total = 0.0
    for name, fn in calls.items():
        fn(), fn()  # warm-up: code object, tables, allocator
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        med = statistics.median(ms)
        fmas = planes[name] * H * (W // 2) * W * 2
        res[name] = dict(planes=planes[name], ms_median=round(med, 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4),
                         fp64_fma=fmas, fp64_Tfma_per_s_at_median=round(fmas / (med * 1e-3) / 1e12, 3))
        total += med
    res["total_ms"] = round(total, 4)
    res["forecast_step_ms"] = a.step_ms
    res["share_of_forecast_step"] = round(total / a.step_ms, 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
