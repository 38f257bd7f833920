"""Time the ``swiftk_lead_window_mean`` call that ``swift_amd.generate --lead-windows`` adds, at the size of one IC of the flagship
job (12 members, 60 lead steps, 69 variables at 128 x 256: x [60, 12 69 128 256], 6.5 GB), against the torch formulation:

    python tools/windows_bench.py [--steps 60] [--members 12] [--channels 69] [--grid 128 256] [--reps 20] [--out FILE.json]

    kernel   lead_window_mean(x [steps, M], first, count)            one launch per 8 windows, out [nw, M] fp32
    torch    x[a:b].double().sum(0).div(L).float() per window        an fp64 temporary of twice the window's bytes each

for three window sets: the whole 15 days (6-360), weeks 1 and 2 (6-168, 174-336), and eight overlapping windows (the four
weeks-of-the-fortnight, both weeks together, days 1-3, days 4-10, everything).  Both are timed with HIP events, ``--reps`` times
after two warm-up calls, in the same process on the same fields (280 + 1e-2 x normal, a temperature under a small variation);
before timing the two results are compared (the torch sum is a tree, the kernel's sequential: they may differ in the last bit).
Reported per set: medians and extremes in milliseconds, the byte floor -- 4 B x (rows in any window + nw) x M at ``--copy-tbs``
(default 6.29 TB/s, the device's measured copy rate) -- the call as a multiple of it, the achieved TB/s of those bytes, and the
ratio torch / kernel; and the commit and the device."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from swift_amd.eval.metrics import lead_window_mean, parse_lead_windows  # noqa: E402

SETS = {"15_days": ["6-360"], "weeks_1_2": ["6-168", "174-336"],
        "eight_overlapping": ["6-168", "174-336", "6-336", "6-72", "78-240", "90-258", "192-360", "6-360"]}


def torch_means(x, first, count):
    return torch.stack([x[f:f + c].double().sum(0).div(c).float() for f, c in zip(first, count)])


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
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--members", type=int, default=12)
    ap.add_argument("--channels", type=int, default=69)
    ap.add_argument("--grid", type=int, nargs=2, default=[128, 256])
    ap.add_argument("--interval", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--copy-tbs", type=float, default=6.29)
    ap.add_argument("--commit", type=str, default=None, help="the commit measured, where the tree is not a git checkout")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps: at least 20 (the figure quoted is a median)")
    if not torch.cuda.is_available():
        raise SystemExit("windows_bench.py measures on the GPU: none found")
    dev = torch.device("cuda")
    n, M = a.steps, a.members * a.channels * a.grid[0] * a.grid[1]
    try:
        commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    res = dict(shape=dict(steps=n, members=a.members, V=a.channels, H=a.grid[0], W=a.grid[1], M=M, x_bytes=4 * n * M), reps=a.reps,
               device=torch.cuda.get_device_name(0), commit=commit, fields="280 + 1e-2 x normal", copy_rate_TB_per_s=a.copy_tbs, sets={})
    g = torch.Generator(device=dev).manual_seed(n)
    x = torch.empty(n, M, device=dev)
    for r in range(n):  # row by row: no second buffer of x's size
        x[r] = 280.0 + 1e-2 * torch.randn(M, device=dev, generator=g)
    for name, specs in SETS.items():
        specs = [s for s in specs if int(s.split("-")[1]) <= n * a.interval]
        _, first, count = parse_lead_windows(specs, n, a.interval)
        used = torch.zeros(n, dtype=torch.bool)
        for f, c in zip(first, count):
            used[f:f + c] = True
        nbytes = 4 * (int(used.sum()) + len(specs)) * M
        ours, theirs = lead_window_mean(x, first, count), torch_means(x, first, count)
        torch.cuda.synchronize()
        diff = (ours.double() - theirs.double()).abs().max().item()
        if diff > 280.0 * 2.0 ** -23:     # one fp32 ulp at 280
            raise SystemExit(f"kernel and torch formulation disagree on {name}: {diff}")
        del ours, theirs
        k = timed(lambda: lead_window_mean(x, first, count), a.reps)
        floor = nbytes / (a.copy_tbs * 1e12) * 1e3
        k.update(byte_floor_ms=round(floor, 4), over_byte_floor=round(k["ms_median"] / floor, 2),
                 TB_per_s_at_median=round(nbytes / (k["ms_median"] * 1e-3) / 1e12, 3),
                 share_of_copy_rate=round(nbytes / (k["ms_median"] * 1e-3) / 1e12 / a.copy_tbs, 3))
        t = timed(lambda: torch_means(x, first, count), a.reps)
        res["sets"][name] = dict(windows=specs, rows_in_any_window=int(used.sum()), bytes_floor=nbytes, max_abs_difference_torch_vs_kernel=diff,
                                 kernel=k, torch=t, torch_over_kernel=round(t["ms_median"] / k["ms_median"], 2))
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
