"""Time the ``swiftk_event_table`` call that ``swift_amd.generate --events`` adds, at the size of one lead step of the flagship
job (8 ICs x 12 members, 69 variables at 128 x 256), for 1, 4 and 16 events (half of them sharing one variable), next to
``swiftk_rank_histogram`` in the same process and against the torch formulation of the same table:

    python tools/events_bench.py [--ics 8] [--members 12] [--channels 69] [--grid 128 256] [--events 1 4 16] [--reps 25] [--out FILE.json]

    kernel   event_table(pred [ICs, members, V, H, W], y [ICs, V, H, W], lat, ev_var, ev_dir, thr [E, H, W])   one launch
    torch    k = (pred[:, :, ev_var] > thr).sum(1); o = y[:, ev_var] > thr; one_hot(2 k + o) in fp64; weighted sum over (H, W)

All are timed with HIP events, ``--reps`` times after two warm-up calls, on the same Gaussian fields; before timing the kernel's
table must equal the torch formulation's within the reordering of its fp64 sums (1e-12 relative).  Reported per event count:
medians and extremes in milliseconds, the time per (IC, event) plane next to the rank histogram's time per (IC, variable) plane,
the bytes the kernel has to read ((members + 2) * 4 per pixel and event: members, truth, threshold), the floor of those bytes
at ``--copy-tbs`` (default 6.29 TB/s, the device's measured copy rate) and the ratio to it, and the ratio torch / kernel.  A call
has ICs x E workgroups, one per plane: below the device's 256 compute units a call's time is one workgroup's walk through its
plane, so the time per plane of a small E is that of an under-filled device, not a rate -- ``workgroups`` says which it is.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from swift_amd.eval.metrics import event_table, event_tables_to_device, rank_histogram  # noqa: E402


def torch_table(pred, y, w_lat, ev_var, ev_dir, thr):
    """The same table in torch: comparisons, one-hot of the cell index, weighted sum.  [I, E, N + 1, 2] fp64."""
    I, N = pred.shape[:2]
    x, yy, t = pred[:, :, ev_var.long()], y[:, ev_var.long()], thr[None]                 # [I, N, E, H, W], [I, E, H, W]
    lt = (ev_dir != 0)[None, :, None, None]
    k = torch.where(lt[:, None], x < t[:, None], x > t[:, None]).sum(1)
    o = torch.where(lt, yy < t, yy > t)
    cell = torch.nn.functional.one_hot(2 * k + o, 2 * (N + 1)).to(torch.float64) * (~torch.isnan(t))[..., None]
    return torch.einsum("iehwc,h->iec", cell, w_lat).view(I, -1, N + 1, 2)


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
    ap.add_argument("--events", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--copy-tbs", type=float, default=6.29)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("--reps: at least 20 (the figure quoted is a median)")
    if not torch.cuda.is_available():
        raise SystemExit("events_bench.py measures on the GPU: none found")
    dev = torch.device("cuda")
    I, N, V, (H, W) = a.ics, a.members, a.channels, a.grid
    g = torch.Generator(device=dev).manual_seed(0)
    pred = torch.randn(I, N, V, H, W, device=dev, generator=g)
    truth = torch.randn(I, V, H, W, device=dev, generator=g)
    lat = -90.0 + (np.arange(H) + 0.5) * (180.0 / H)
    w = np.cos(np.deg2rad(lat))
    w_lat = torch.from_numpy(w / w.mean()).to(dev)
    res = dict(shape=dict(ics=I, members=N, V=V, H=H, W=W), reps=a.reps, device=torch.cuda.get_device_name(0),
               compute_units=torch.cuda.get_device_properties(0).multi_processor_count, copy_rate_TB_per_s=a.copy_tbs)
    r_med, r_min, r_max = timed(lambda: rank_histogram(pred, truth, lat), a.reps)
    res["rank_histogram"] = dict(planes=I * V, ms_median=round(r_med, 4), ms_min=round(r_min, 4), ms_max=round(r_max, 4),
                                 us_per_plane=round(r_med * 1e3 / (I * V), 4), us_per_plane_min=round(r_min * 1e3 / (I * V), 4),
                                 us_per_plane_max=round(r_max * 1e3 / (I * V), 4))
    res["event_table"] = []
    rng = np.random.default_rng(0)
    for E in a.events:
        # half of the events on one variable, the others on variables of their own; thresholds around the median and in the tail
        ev_var = np.array([0 if e % 2 == 0 else (1 + 7 * e) % V for e in range(E)], dtype=np.int32)
        ev_dir = (np.arange(E) // 2 % 2).astype(np.int32)
        thr = np.broadcast_to(rng.uniform(-1.5, 1.5, (E, 1, 1)), (E, H, W)).astype(np.float32)
        tables = event_tables_to_device(ev_var, ev_dir, thr, V, dev)
        ours, theirs = event_table(pred, truth, lat, *tables), torch_table(pred, truth, w_lat, *tables)
        torch.cuda.synchronize()
        rel = float(((ours - theirs).abs() / theirs.clamp_min(1e-300)).max())
        if rel > 1e-12:
            raise SystemExit(f"kernel and torch formulation disagree at E = {E}: {rel:.3e} relative")
        k_med, k_min, k_max = timed(lambda: event_table(pred, truth, lat, *tables), a.reps)
        t_med, t_min, t_max = timed(lambda: torch_table(pred, truth, w_lat, *tables), a.reps)
        nbytes = I * E * H * W * (N + 2) * 4
        floor = nbytes / (a.copy_tbs * 1e12) * 1e3
        res["event_table"].append(dict(
            events=E, workgroups=I * E, max_rel_difference_kernel_vs_torch=rel, ms_median=round(k_med, 4), ms_min=round(k_min, 4),
            ms_max=round(k_max, 4), us_per_plane=round(k_med * 1e3 / (I * E), 4), bytes_read=nbytes,
            TB_per_s_at_median=round(nbytes / (k_med * 1e-3) / 1e12, 4), byte_floor_ms=round(floor, 5),
            over_byte_floor=round(k_med / floor, 2), per_plane_over_rank_histogram=round(k_med / (I * E) / (r_med / (I * V)), 2),
            torch_ms_median=round(t_med, 4), torch_ms_min=round(t_min, 4), torch_ms_max=round(t_max, 4),
            torch_over_kernel=round(t_med / k_med, 2)))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
