"""Ensemble autoregressive rollout driver -- ``python -m swift_amd.generate`` (mirrors reference
src/swift/generate.py: same flags, same run-directory layout, same npy output layout).

    python -m swift_amd.generate --input RUN --checkpoint NAME --members 12 --steps 60 --samples 64 --interval 6 --dump numpy

reads ``RUN/.hydra/config.yaml`` (the saved composed config, generate.py:161) and
``RUN/checkpoints/checkpoint-NNNNNN.pt`` (``state["ema"]``, generate.py:225-226) and writes
``RUN/output/<ckpt>/output-{n}i-{steps}s-{members}m-{interval}h.npy`` with shape
(samples, members, steps+1, C, H, W) float32 (utils/io.py:237-259).

MI355X-first differences: the flattened IC-major (IC, member) space is
sharded in contiguous blocks over ranks (the reference shards members only, generate.py:79-81,
which caps 12 members at 6x on 8 GPUs) -- an IC's members sit next to each other, so a batch
reads each IC's state and forcing files once; rank 0 loads the checkpoint and broadcasts the
weights over RCCL; each rank rolls its units on the device (``RolloutEngine``) and writes its
own slices of the shared store (npy memmap, or one zarr chunk file per unit and variable:
``utils/zarrlite.py``); a barrier closes the job.  What else a job makes of its rollout is a list of output products, one small
object per flag (``generating/products.py``): ``rollout_and_save`` hands each of them every IC's members once, in IC order, and
lets it finish with its collective and its files.  Additive flags: ``--solver`` (``edm`` is the default of an EDMPrecond run),
``--num-steps``, ``--dtype``, ``--synthetic`` (random-init weights + synthetic fields when no run directory exists), ``--metrics``
(ensemble RMSE / CRPS / spread-skill against the dataset's own fields, reduced per rank on the device and all-gathered:
eval/metrics.py:39-134 without the round trip through the store), ``--spectra`` (implies ``--metrics``; adds ``evaluation_spectra.npz``
beside evaluation_metrics.json: latitude-weighted zonal power spectra of the members, of the ensemble mean and of the verifying
fields per lead step and variable, ``swiftk_zonal_power`` in fp64 on the device -- whether the members stay as sharp as the truth,
which RMSE and CRPS cannot tell), ``--rank-hist`` (implies ``--metrics``; adds ``evaluation_rank_histogram.npz``: per lead step and variable
the latitude-weighted frequency with which the verifying value takes each rank 0 .. members among the members, ties spread evenly,
``swiftk_rank_histogram`` in exact integers and fp64 on the device -- flat is calibrated, U-shaped under-dispersive, dome-shaped
over-dispersive, sloped biased, which one spread-skill number per variable cannot tell), ``--summary [--quantiles q ...]``
(writes ``<output name>-summary.zarr`` beside the other outputs: per IC, lead step (lead 0 included), variable and grid point the
ensemble mean, the spread and the quantiles, default 0.1 0.5 0.9 -- the forecast store's structure with a ``statistic`` dimension
where ``number`` stands; ``swiftk_ensemble_summary`` in fp64 on the device, one call per IC on the members the device already
holds, so the raw trajectories never leave it on this flag's account: what a forecaster reads out of an ensemble, at
(2 + quantiles) / members of the raw store's size; it needs an IC's members in one batch, like the metrics, but does not imply
them and loads no verifying fields: ``--dump none --summary`` is a complete job), ``--maps`` (implies ``--metrics``; adds
``evaluation_maps.zarr`` and ``evaluation_regions.json``: per lead step, variable and grid point the bias, MSE, fair CRPS and
member variance, means over the ICs -- ``swiftk_ensemble_maps`` in fp64 on the device, accumulated per rank in one resident
buffer -- and their latitude-weighted means over the globe, the tropics and the two extratropics: where the forecast is good,
which no whole-grid average can tell), ``--events SPEC ... [--events-file FILE.npz]`` (either implies ``--metrics``; adds
``evaluation_reliability.npz`` and ``evaluation_brier.json``: for every threshold event -- ``2m_temperature:lt:273.15``, or a
per-grid-point threshold field from the file, NaN where a pixel is left out -- and lead step the latitude-weighted contingency
table of the number of members in the event against the outcome, ``swiftk_event_table`` in exact integers and fp64 on the device,
and from it the reliability diagram, the Brier score with its reliability / resolution / uncertainty decomposition, the fair
Brier score and the skill score against climatology: the probability of an event, which lives in the tails where a score of the
whole distribution looks least), ``--lead-windows SPEC ...`` (implies ``--metrics``; adds ``evaluation_windows.json``: for every
window of lead hours ``A-B``, both ends included -- ``6-168 174-336`` are weeks 1 and 2 of a 6-hourly job -- the RMSE, CRPS and
spread/skill ratio of the lead-time-MEAN fields, members and verifying fields averaged over the window by
``swiftk_lead_window_mean`` in fp64 on the device and scored by ``swiftk_ensemble_sums`` like an instantaneous field: what is
verified past day 10, where a forecast can have lost its skill at every single step and still have a useful weekly mean, and
where a drifting model shows first) and ``--gpus N`` (start the N ranks from a bare ``python -m`` call).
"""
from __future__ import annotations

import argparse
import json
import os
import time
from concurrent.futures import ThreadPoolExecutor
from glob import glob

import numpy as np
import torch
import torch.distributed as tdist

from . import dist
from .config import Cfg, instantiate, load_saved
from .eval.metrics import (BRIER_SCORES, MAP_STATISTICS, WINDOWS_FILE, brier_scores, parse_events, parse_lead_windows, quantile_table,
                           region_means, scores_from_sums, window_scores)
from .rollout import RolloutEngine, unit_seed
from .utils import zarrlite

# the flags every CLI that loads a run shares (eval/sampler.py builds its parser on them too)
common_parser = argparse.ArgumentParser(add_help=False)
common_parser.add_argument("--input", type=str, required=True, help="Input directory")
common_parser.add_argument("--checkpoint", type=str, default=None, help="Checkpoint name (default: latest)")
common_parser.add_argument("--samples", type=int, default=-1, help="Number of samples use")
common_parser.add_argument("--interval", type=int, default=6, choices=[6, 12, 24], help="Interval in hours")
# additive
common_parser.add_argument("--dtype", type=str, default="f32", choices=["f32", "bf16", "bf16x3"],
                           help="compute engine: f32 = exact fp32 MFMA (the reference's arithmetic, factory.py:11); bf16x3 = fp32-grade "
                                "(<= 1e-4 of the reference) from split-bf16 MFMA products, about twice as fast; bf16 = throughput engine")
common_parser.add_argument("--synthetic", action="store_true", help="random-init weights + synthetic data (no run dir needed)")
common_parser.add_argument("--gpus", type=int, default=None, help="start this many ranks (one per GPU) when not launched by torchrun/mpiexec")
DENOISE_DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32, "bf16x3": "bf16x3"}  # --dtype -> sampler_factory's denoise_dtype

parser = argparse.ArgumentParser(parents=[common_parser])
parser.add_argument("--members", type=int, default=1, help="Number of ensemble members")
parser.add_argument("--steps", type=int, default=8, help="Number of prediction steps")
parser.add_argument("--batch", type=int, default=32, help="(member, IC) units per device batch")
parser.add_argument("--dump", type=str, default=None, choices=["zarr", "numpy", "none"],
                    help="Output format (default: zarr, the reference's default, for a one-rank job; with more than one rank the "
                         "default is 'none' + --metrics -- the ensemble metrics, reduced on the devices, and no raw trajectories: one "
                         "rank streams 3.4 GB/s of fp32 fields (330 sample-steps/s x 9 MB + host page faults ~3 GB/s per process), "
                         "eight of them 27 GB/s into ONE filesystem.  Ask for zarr / numpy explicitly to get the raw store at any rank count)")
# additive
parser.add_argument("--solver", type=str, default=None, choices=["scm", "2s", "dpm", "edm"],
                    help="default: edm for an EDMPrecond run (settings from its saved solver config), else scm")
parser.add_argument("--num-steps", type=int, default=None, help="solver steps per forecast step (default: 1; an EDM run's "
                    "saved solver.num_steps)")
parser.add_argument("--metrics", action="store_true", help="ensemble metrics vs the dataset's fields -> evaluation_metrics.json")
parser.add_argument("--spectra", action="store_true", help="implies --metrics; zonal power spectra of the members, the ensemble "
                    "mean and the verifying fields per lead step and variable -> evaluation_spectra.npz")
parser.add_argument("--rank-hist", action="store_true", help="implies --metrics; rank (Talagrand) histogram of the verifying "
                    "fields among the members per lead step and variable -> evaluation_rank_histogram.npz")
parser.add_argument("--summary", action="store_true", help="per IC, lead step, variable and grid point the ensemble mean, spread "
                    "and quantiles -> <output name>-summary.zarr (does not imply --metrics)")
parser.add_argument("--maps", action="store_true", help="implies --metrics; per lead step, variable and grid point the bias, MSE, "
                    "fair CRPS and member variance, means over the ICs -> evaluation_maps.zarr, and their regional means "
                    "(global, tropics, extratropics) -> evaluation_regions.json")
parser.add_argument("--events", type=str, nargs="+", default=None, metavar="SPEC", help="implies --metrics; threshold events "
                    "<variable>:<gt|lt>:<value> (2m_temperature:lt:273.15): per lead step the contingency table of members in the "
                    "event against the outcome -> evaluation_reliability.npz, and the Brier score, its decomposition and the skill "
                    "score -> evaluation_brier.json")
parser.add_argument("--events-file", type=str, default=None, metavar="FILE.npz", help="implies --metrics; further events: keys "
                    "<variable>:<gt|lt>:<label>, values a scalar or an [H, W] threshold field, NaN where a pixel is left out")
parser.add_argument("--lead-windows", type=str, nargs="+", default=None, metavar="SPEC", help="implies --metrics; lead-time windows "
                    "A-B (lead hours, both ends included: 6-168 174-336 are weeks 1 and 2): RMSE, CRPS and spread/skill of the "
                    "fields averaged over each window -> evaluation_windows.json")
parser.add_argument("--quantiles", type=float, nargs="+", default=[0.1, 0.5, 0.9], help="quantiles of --summary, each in [0, 1], "
                    "at most 16 (default: 0.1 0.5 0.9)")


def get_ckpt_num(fpath: str) -> int:
    """utils/helpers.py:11-14."""
    return int(fpath.split(".pt")[-2].split("-")[-1])


def create_empty_numpy(ofile, dataset_len, n_channels, img_resolution, members, steps):
    """utils/io.py:237-259."""
    np.lib.format.open_memmap(ofile, dtype=np.float32, mode="w+",
                              shape=(dataset_len, members, steps + 1, n_channels, *img_resolution))


def synthetic_cfg() -> Cfg:
    from .config import compose
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")
    return compose(here, "train", ["data=era5-synthetic-1.4"])


def solver_setup(cfg, solver=None, num_steps=None, interval: int = 6):
    """(solver mode, solver kwargs) of a run: a PassPrecond (TrigFlow) run defaults to 1-step "scm" at sigma 0.02..200, an
    EDMPrecond run to "edm" with its saved ``solver`` config (reference keys: num_steps, sigma_min, sigma_max, rho, S_churn,
    S_min, S_max, S_noise); ``num_steps`` overrides only when given, the auxiliary input is the lead time of ``interval``.
    A solver of the other parametrisation is refused here, before any GPU work."""
    edm = str((cfg.get("precond") or {}).get("_target_", "")).rsplit(".", 1)[-1] == "EDMPrecond"
    solver = solver or ("edm" if edm else "scm")
    if edm != (solver == "edm"):
        raise ValueError(f"--solver {solver} does not match this run's precond ({'EDMPrecond' if edm else 'PassPrecond'}): "
                         f"{'an EDM net samples with --solver edm' if edm else '--solver edm needs an EDMPrecond run'}")
    if solver == "edm":
        kw = {k: v for k, v in dict(cfg.get("solver") or {}).items() if k != "auxiliary"}
        if num_steps is not None:
            kw["num_steps"] = int(num_steps)
    else:
        kw = dict(num_steps=1 if num_steps is None else int(num_steps), sigma_min=0.02, sigma_max=200.0)
    kw["auxiliary"] = interval / 10.0
    return solver, kw


def select_indices(n_dataset: int, samples: int, steps: int, interval: int):
    if samples == -1:
        return list(range(n_dataset))
    return np.linspace(0, n_dataset - 1 - (steps * interval // 6), num=samples, dtype=int).tolist()  # generate.py:179-184


def create_empty_zarr(ofile, dataset, indices, members, steps, interval):
    """utils/io.py:161-235 through the stdlib writer (no zarr / xarray in this image)."""
    lat, lon = dataset.get_lat_lon()
    times = np.array([dataset.get_time(int(i)) for i in indices], dtype="datetime64[ns]")
    zarrlite.create_forecast_store(ofile, list(dataset.variables), times, lat, lon, members, steps, interval=interval, batch=1)


def rollout_and_save(engine: RolloutEngine, dataset, indices, members: int, steps: int, ofile: str, device, args, products=None):
    """generate.py:48-154 with (member, IC) units instead of members as the sharded work item.  Batch by batch: inputs staged one
    batch ahead, the rollout, every product (``generating/products.py``; default: those of ``args``) fed each IC of the batch once
    in ascending IC order -- so that no product's sums depend on ``--batch`` -- and the trajectory handed to the raw store's writer;
    then every product finishes (its collective; on rank 0 its files).  Returns rank 0's metrics dict (``--metrics``), else None."""
    from .generating.products import StoreWriter, plan_units, products_from_args
    nv, interval, n_ic = len(dataset.variables), engine.interval, len(indices)
    on_gpu = torch.device(device).type == "cuda"   # (the host-logic tests drive this loop with a CPU stand-in engine)
    reader = ThreadPoolExecutor(max_workers=1)
    loaders = ThreadPoolExecutor(max_workers=8)
    stagers = ThreadPoolExecutor(max_workers=4)  # forcing slabs, step by step (their own pool: output writes must not queue behind them)
    products = products_from_args(args, dataset, members, steps, ofile, device, n_ic, interval, loaders) if products is None else products
    need_truth = any(p.needs_truth for p in products)
    batch, mine = plan_units(products, n_ic, members, int(args.batch), dist.get_rank(), dist.get_world_size())
    store = StoreWriter(getattr(args, "dump", "numpy") or "zarr", ofile, dataset, loaders, device)
    t_stage = 0.0  # seconds in input staging (host side)

    def stage(s):
        """Host-side inputs of the batch starting at unit s (pinned tensors; runs on the reader thread, one batch ahead)."""
        nonlocal t_stage
        t1 = time.time()
        # flattened unit id -> (member, position of its IC in ``indices``); IC-major, so an IC's members are adjacent
        units = [(u % members, u // members) for u in range(s, min(s + batch, mine.stop))]
        ics = [indices[ic] for _, ic in units]
        state = getattr(dataset, "get_state", None)  # one read per IC; dataset[j] would also read j's training target
        x0 = {int(j): (dataset.standardize_x(state(int(j))) if state else dataset[int(j)][0][0][:nv]) for j in set(ics)}
        X0 = torch.stack([x0[int(j)] for j in ics], 0)
        # GPU path: forcings are staged step by step behind the rollout's back (the first batch starts after step 0's slab, not
        # after all `steps` of them); the CPU stand-in of the host-logic tests takes the whole tensor
        forc = engine.stage_forcings_lazily(ics, steps, device, stagers) if on_gpu else engine.stage_forcings(ics, steps, "cpu")
        truth = None
        if need_truth:  # verifying fields of every lead step, physical units, one copy per IC of the batch
            uniq = sorted(set(ic for _, ic in units))
            get = state if state else (lambda j: dataset.unstandardize_x(dataset[j][0][0][:nv]))
            jobs = [int(indices[ic]) + (i + 1) * interval // 6 for ic in uniq for i in range(steps)]

            def load_truth():  # file reads / field synthesis in parallel (numpy and h5 release the GIL)
                fields = list(loaders.map(get, jobs))
                tt = torch.stack(fields, 0).view(len(uniq), steps, *fields[0].shape)
                return tt.pin_memory() if on_gpu else tt

            # needed only once the batch has been rolled out: on the GPU path it loads while the rollout runs
            truth = stagers.submit(load_truth) if on_gpu else load_truth()
        if on_gpu:
            X0 = X0.pin_memory()
        t_stage += time.time() - t1
        return units, X0, forc, truth

    starts = list(range(mine.start, mine.stop, batch))
    nxt = reader.submit(stage, starts[0]) if starts else None
    done = 0
    for bi, s in enumerate(starts):
        units, X0, forc, truth = nxt.result()
        nxt = reader.submit(stage, starts[bi + 1]) if bi + 1 < len(starts) else None
        X0 = X0.to(device, non_blocking=True)
        if not on_gpu:
            forc = forc.to(device, non_blocking=True)
        traj = engine.run(X0, forc, steps, seeds=[unit_seed(m, indices[ic]) for m, ic in units],  # [B, steps+1, ...] view
                          **({"after_step": store.after_step(units)} if on_gpu else {}))
        dev_buf = traj.transpose(0, 1)      # the contiguous step-major buffer behind it
        truth = truth.result() if hasattr(truth, "result") else truth
        # every IC's truth products before any IC's other products, the order of device calls this loop has always had: the summary
        # kernel of one IC never sits in front of the next IC's metric sums, whose copy to the host the loop waits for
        for with_truth in (True, False):
            feed = [p for p in products if p.needs_truth == with_truth]
            for k, ic in enumerate(sorted(set(ic for _, ic in units)) if feed else []):
                slots = [b for b, (_, i) in enumerate(units) if i == ic]
                assert len(slots) == members and slots == list(range(slots[0], slots[0] + members))
                ic_traj = dev_buf[:, slots[0]:slots[0] + members]                    # [steps + 1, members, nv, H, W]
                pred = ic_traj[1:].contiguous() if with_truth else None             # the one copy every truth product shares
                y = truth[k].to(pred.device, non_blocking=True) if with_truth else None
                for p in feed:
                    p.add_ic(ic, ic_traj, pred, y)
        if on_gpu:
            dev_buf.record_stream(store.copy_stream)  # its last slabs may still be on their way to the host
        else:
            store.submit_traj(units, dev_buf)
        done += len(units)
        dist.log0(f"rank 0: {done}/{len(mine)} units")
    store.close()
    reader.shutdown()
    stagers.shutdown()
    results = [p.finish() for p in products]   # (the summary's last files are still being written by the loaders)
    loaders.shutdown()
    dist.log0(f"host side: {t_stage:.2f} s staging inputs, "
              f"{store.seconds + sum(getattr(p, 'seconds', 0.0) for p in products):.2f} s writing outputs")
    return next((r for r in results if r is not None), None)  # (only the metric sums return something: rank 0's dict)


def summary_path(ofile: str) -> str:
    """``<output name>-summary.zarr`` beside the job's other outputs (``ofile``: the raw store's name, whatever ``--dump``)."""
    return os.path.splitext(ofile)[0] + "-summary.zarr"


def create_empty_summary(sfile, dataset, indices, members, steps, interval, quantiles):
    lat, lon = dataset.get_lat_lon()
    times = np.array([dataset.get_time(int(i)) for i in indices], dtype="datetime64[ns]")
    zarrlite.create_summary_store(sfile, list(dataset.variables), times, lat, lon, members, steps, quantiles, interval=interval)


def check_summary_args(args):
    """``--summary`` / ``--quantiles`` checked on the host (``ValueError``), before any rank is started or the GPU is touched."""
    if getattr(args, "summary", False):
        if not 2 <= args.members <= 64:
            raise ValueError(f"--summary takes the statistics over 2 .. 64 members, got --members {args.members}")
        quantile_table(args.quantiles, args.members)


def collect_metrics(metric_sums, n_ic, steps, nv, members, dataset, interval, device, odir):
    """Output collection over RCCL: every rank contributes the ensemble sums of its ICs ([n_ic, steps, nv, 4], zeros
    elsewhere), one all-gather, rank 0 turns them into the reference's metric names (eval/metrics.py:39-134)."""
    local = torch.zeros(n_ic, steps, nv, 4, dtype=torch.float64)
    for ic, v in metric_sums.items():
        local[ic] = v
    total = torch.stack(dist.all_gather_parts(local, device), 0).sum(0).cpu() if dist.collectives_active() else local
    if dist.get_rank() != 0:
        return None
    H, W = dataset.img_resolution
    res = {}
    for j in range(steps):
        rmse, crps, ssr = scores_from_sums(total[:, j], members, H * W)    # [n_ic, nv, 4] -> [nv] each
        for i, v in enumerate(dataset.variables):
            tag = f"{(j + 1) * interval}h"
            res[f"rmse_{v}_{tag}"], res[f"crps_{v}_{tag}"], res[f"ssr_{v}_{tag}"] = float(rmse[i]), float(crps[i]), float(ssr[i])
    path = os.path.join(odir, "evaluation_metrics.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    dist.log0(f"ensemble metrics of {n_ic} ICs x {members} members gathered from {dist.get_world_size()} rank(s): {path}")
    return res


SPECTRA_FILE = "evaluation_spectra.npz"


def collect_spectra(local, n_ic, members, variables, interval, odir):
    """``local`` [steps, nv, 3, K] fp64: this rank's sums over its ICs (the ``Spectra`` product's).  One all-gather of these arrays (not
    of per-IC rows: 64 ICs x 60 steps of them are 0.8 GB per rank), rank 0 adds them in rank order, divides by the number of
    terms and writes ``evaluation_spectra.npz`` (plain arrays, no pickles): wavenumber [K], lead_hours [steps], variables [nv],
    member / ensemble_mean / truth [steps, nv, K] (means over ICs and members / ICs / ICs), members, samples."""
    total = dist.sum_in_rank_order(local)
    if total is None:
        return None
    steps, nv, _, K = total.shape
    arrays = dict(wavenumber=np.arange(K, dtype=np.int64), lead_hours=(np.arange(steps, dtype=np.int64) + 1) * int(interval),
                  variables=np.array([str(v) for v in variables], dtype=np.str_),
                  member=total[:, :, 0] / (n_ic * members), ensemble_mean=total[:, :, 1] / n_ic, truth=total[:, :, 2] / n_ic,
                  members=np.int64(members), samples=np.int64(n_ic))
    path = os.path.join(odir, SPECTRA_FILE)
    np.savez(path, allow_pickle=False, **arrays)
    dist.log0(f"zonal power spectra (--spectra) of {n_ic} ICs x {members} members, {K} wavenumbers, gathered from "
              f"{dist.get_world_size()} rank(s): {path}")
    return arrays


RANK_HIST_FILE = "evaluation_rank_histogram.npz"


def collect_rank_histogram(local, n_ic, members, variables, interval, norm, odir):
    """``local`` [steps, nv, members + 1] fp64: this rank's sums over its ICs (the ``RankHistogram`` product's).  One all-gather of
    these arrays (never of per-IC rows), rank 0 adds them in rank order, divides by ``n_ic * norm`` (``norm`` = W sum(w_lat), what
    one plane's bins sum to) so that each (lead, variable) row sums to 1, and writes ``evaluation_rank_histogram.npz`` (plain
    arrays, no pickles): rank [members + 1], lead_hours [steps], variables [nv], frequency [steps, nv, members + 1], members,
    samples."""
    total = dist.sum_in_rank_order(local)
    if total is None:
        return None
    steps, nv, bins = total.shape
    assert bins == members + 1
    arrays = dict(rank=np.arange(bins, dtype=np.int64), lead_hours=(np.arange(steps, dtype=np.int64) + 1) * int(interval),
                  variables=np.array([str(v) for v in variables], dtype=np.str_), frequency=total / (n_ic * float(norm)),
                  members=np.int64(members), samples=np.int64(n_ic))
    path = os.path.join(odir, RANK_HIST_FILE)
    np.savez(path, allow_pickle=False, **arrays)
    dist.log0(f"rank histograms (--rank-hist) of {n_ic} ICs x {members} members, {bins} ranks, gathered from "
              f"{dist.get_world_size()} rank(s): {path}")
    return arrays


MAPS_FILE, REGIONS_FILE = "evaluation_maps.zarr", "evaluation_regions.json"


def check_maps_args(args):
    """``--maps`` checked on the host (``ValueError``), before any rank is started or the GPU is touched."""
    if getattr(args, "maps", False) and not 2 <= args.members <= 64:
        raise ValueError(f"--maps takes the CRPS and the variance over 2 .. 64 members, got --members {args.members}")


def collect_maps(local, steps, n_ic, members, variables, lat, lon, interval, odir, device="cpu"):
    """``local`` [steps, 4, nv, H, W] fp64: this rank's sums over its ICs of the ``ensemble_maps`` terms (None for a rank without
    ICs: it contributes zeros).  Lead step by lead step -- nothing larger than world x one [4, nv, H, W] slab is ever gathered --
    one all-gather of the step's slabs; rank 0 adds them in rank order, divides by ``n_ic`` and writes the slab's chunks of
    ``evaluation_maps.zarr`` (float32: ``zarrlite.create_maps_store``) and, from the fp64 means before that cast, the step's
    entries of ``evaluation_regions.json``: region -> ``bias_`` / ``rmse_`` / ``crps_`` / ``spread_`` / ``ssr_<var>_<lead>h``, the
    latitude-weighted regional means (``eval.metrics.region_means``) of the IC-mean maps, then rmse = sqrt(mean mse),
    spread = sqrt(mean variance), ssr = spread / rmse."""
    variables = [str(v) for v in variables]
    nv, H, W = len(variables), len(lat), len(lon)
    root = dist.get_rank() == 0
    path, rpath = os.path.join(odir, MAPS_FILE), os.path.join(odir, REGIONS_FILE)
    if root:
        channels = zarrlite.create_maps_store(path, variables, lat, lon, members, steps, MAP_STATISTICS, n_ic, interval=interval)
    regions = {}
    for j in range(steps):
        slab = local[j].contiguous() if local is not None else torch.zeros(4, nv, H, W, dtype=torch.float64, device=device)
        assert tuple(slab.shape) == (4, nv, H, W) and slab.dtype == torch.float64
        total = dist.sum_in_rank_order(slab)
        if not root:
            continue
        total /= float(n_ic)
        zarrlite.write_maps_step(path, channels, j, total.astype(np.float32))
        for region, m in region_means(total, lat).items():   # m [4, nv]
            with np.errstate(divide="ignore", invalid="ignore"):
                rmse, spread = np.sqrt(m[1]), np.sqrt(m[3])
                ssr = spread / rmse
            out = regions.setdefault(region, {})
            for i, v in enumerate(variables):
                tag = f"{v}_{(j + 1) * interval}h"
                out[f"bias_{tag}"], out[f"rmse_{tag}"], out[f"crps_{tag}"] = float(m[0, i]), float(rmse[i]), float(m[2, i])
                out[f"spread_{tag}"], out[f"ssr_{tag}"] = float(spread[i]), float(ssr[i])
    if not root:
        return None
    zarrlite.consolidate(path)
    with open(rpath, "w") as f:
        json.dump(regions, f, indent=1)
    dist.log0(f"verification maps (--maps) of {n_ic} ICs x {members} members, statistics {', '.join(MAP_STATISTICS)} at {steps} "
              f"lead steps, gathered from {dist.get_world_size()} rank(s): {path}; regional means ({', '.join(regions)}): {rpath}")
    return regions


RELIABILITY_FILE, BRIER_FILE = "evaluation_reliability.npz", "evaluation_brier.json"


def check_events_args(args, cfg=None):
    """``--events`` / ``--events-file`` checked on the host (``ValueError``), before any rank is started or the GPU is touched:
    2 .. 64 members, and ``parse_events`` against the variables (and, where it names one, the grid) of the run's saved config."""
    if getattr(args, "events", None) or getattr(args, "events_file", None):
        if not 2 <= args.members <= 64:
            raise ValueError(f"--events takes the event probability from 2 .. 64 members, got --members {args.members}")
        ds = (cfg if cfg is not None else load_cfg(args)).data.dataset
        parse_events(args.events, args.events_file, ds.variables, *(ds.get("img_resolution") or (None, None)))


def collect_events(local, n_ic, members, names, variables, interval, odir):
    """``local`` [steps, E, members + 1, 2] fp64: this rank's sums over its ICs of the ``event_table`` cells (the ``Events``
    product's).  One all-gather of these arrays (never of per-IC rows), rank 0 adds them in rank order and writes
    ``evaluation_reliability.npz`` (plain arrays, no pickles): events [E], variables [E] (each event's variable), lead_hours
    [steps], probability [members + 1] = k / members, forecast_frequency [steps, E, members + 1] = n_k / S (each row sums to 1),
    observed_frequency [steps, E, members + 1] = o_k / n_k (NaN in an empty bin), table [steps, E, members + 1, 2] the summed cells
    divided by ``n_ic``, members, samples -- and ``evaluation_brier.json``: ``brier_`` / ``fair_brier_`` / ``reliability_`` /
    ``resolution_`` / ``uncertainty_`` / ``bss_`` / ``base_rate_<event>_<lead>h`` (``eval.metrics.brier_scores`` of the table),
    NaN written as null."""
    total = dist.sum_in_rank_order(local)
    if total is None:
        return None
    steps, E, bins, _ = total.shape
    assert bins == members + 1 and E == len(names) == len(variables)
    table = total / float(n_ic)
    n_k = table[..., 0] + table[..., 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        arrays = dict(events=np.array([str(e) for e in names], dtype=np.str_),
                      variables=np.array([str(v) for v in variables], dtype=np.str_),
                      lead_hours=(np.arange(steps, dtype=np.int64) + 1) * int(interval),
                      probability=np.arange(bins, dtype=np.float64) / members,
                      forecast_frequency=n_k / n_k.sum(-1, keepdims=True), observed_frequency=table[..., 1] / n_k, table=table,
                      members=np.int64(members), samples=np.int64(n_ic))
    path, jpath = os.path.join(odir, RELIABILITY_FILE), os.path.join(odir, BRIER_FILE)
    np.savez(path, allow_pickle=False, **arrays)
    scores = brier_scores(table, members)                                 # {score: [steps, E]}
    flat = {f"{s}_{e}_{(j + 1) * interval}h": (float(scores[s][j, i]) if np.isfinite(scores[s][j, i]) else None)
            for j in range(steps) for i, e in enumerate(names) for s in BRIER_SCORES}
    with open(jpath, "w") as f:
        json.dump(flat, f, indent=1)
    dist.log0(f"threshold events (--events) of {n_ic} ICs x {members} members, {E} events at {steps} lead steps, gathered from "
              f"{dist.get_world_size()} rank(s): reliability diagrams {path}; Brier scores {jpath}")
    return arrays


def check_windows_args(args):
    """``--lead-windows`` checked on the host (``ValueError``), before any rank is started or the GPU is touched: 2 .. 64 members,
    and ``parse_lead_windows`` against the job's ``--steps`` and ``--interval``."""
    if getattr(args, "lead_windows", None):
        if not 2 <= args.members <= 64:
            raise ValueError(f"--lead-windows takes the CRPS and the spread over 2 .. 64 members, got --members {args.members}")
        parse_lead_windows(args.lead_windows, args.steps, args.interval)


def collect_windows(sums, n_ic, names, nv, members, dataset, device, odir):
    """Output collection of ``--lead-windows``, as ``collect_metrics``: every rank contributes the ensemble sums of the window-mean
    fields of its ICs ([n_ic, nw, nv, 4], zeros elsewhere: an IC's slot comes from one rank and is added to zeros, so the file
    does not depend on ``--gpus`` or ``--batch``), one all-gather, rank 0 applies ``scores_from_sums`` per window and writes
    ``evaluation_windows.json``: ``rmse_`` / ``crps_`` / ``ssr_<var>_<A>-<B>h``, the conventions of evaluation_metrics.json."""
    local = torch.zeros(n_ic, len(names), nv, 4, dtype=torch.float64)
    for ic, v in sums.items():
        local[ic] = v
    total = torch.stack(dist.all_gather_parts(local, device), 0).sum(0).cpu() if dist.collectives_active() else local
    if dist.get_rank() != 0:
        return None
    H, W = dataset.img_resolution
    res = window_scores(total, names, dataset.variables, members, H * W)
    path = os.path.join(odir, WINDOWS_FILE)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    dist.log0(f"lead-window scores (--lead-windows) of {n_ic} ICs x {members} members, windows {', '.join(names)}, gathered from "
              f"{dist.get_world_size()} rank(s): {path}")
    return res


def load_cfg(args) -> Cfg:
    """The run's saved composed config (generate.py:161), or the synthetic one when ``--synthetic`` names no run directory."""
    if args.synthetic and not os.path.exists(os.path.join(args.input, ".hydra", "config.yaml")):
        return synthetic_cfg()
    return load_saved(os.path.join(args.input, ".hydra", "config.yaml"))


def build_net(cfg, dataset, args, device):
    """(net on the device in eval mode, checkpoint basename): the run's precond + model with the checkpoint's ``"ema"`` weights
    (generate.py:200-226; ``--synthetic``: seeded random-init weights), loaded by rank 0 and broadcast to the others."""
    net = instantiate(cfg.precond, model_config=cfg.model, img_resolution=dataset.img_resolution,
                      img_channels=dataset.n_target_channels, condition_channels=dataset.n_condition_channels,
                      sigma_max=float("inf"), _recursive_=False, _convert_="object")
    ckpt_basename = "synthetic"
    if not args.synthetic:
        if args.checkpoint is not None:
            name = args.checkpoint if args.checkpoint.endswith(".pt") else args.checkpoint + ".pt"
            ckpt = os.path.join(args.input, "checkpoints", name)
            if not os.path.exists(ckpt):
                raise ValueError(f"Specified checkpoint {ckpt} does not exist")
            ckpt_basename = os.path.basename(name)[:-3]
        else:
            paths = sorted(glob(os.path.join(args.input, "checkpoints", "checkpoint*.pt")), key=get_ckpt_num)
            assert paths, FileNotFoundError(f"No checkpoints in {os.path.join(args.input, 'checkpoints')}")
            ckpt, ckpt_basename = paths[-1], "latest"
        if dist.get_rank() == 0:
            dist.log0(f"Loading checkpoint: {ckpt}")
            net.load_state_dict(torch.load(ckpt, map_location="cpu", weights_only=True)["ema"])
    elif dist.get_rank() == 0:
        from .utils.detinit import swinv2_state
        m = net.model
        net.load_state_dict(swinv2_state(grid=m.grid_size, in_channels=m.in_channels, out_channels=m.out_channels,
                                         patch_size=m.patch_size, depth=m.depth, dim=m.dim, heads=m.heads,
                                         auxiliary_dim=m.auxiliary_dim, logvar=m.logvar_embed is not None, seed=cfg.seed))
    net = net.to(device).eval()
    if dist.collectives_active():  # one-time weight broadcast over RCCL / xGMI
        for p in net.parameters():
            tdist.broadcast(p.data, src=0)
    return net, ckpt_basename


def main(args):
    check_summary_args(args)
    check_maps_args(args)
    cfg = load_cfg(args)
    check_events_args(args, cfg)
    check_windows_args(args)
    solver, solver_kwargs = solver_setup(cfg, args.solver, args.num_steps, args.interval)
    dist.setup_torch(backend=cfg.system.torch.backend)
    np.random.seed(cfg.seed % (1 << 31))
    torch.manual_seed(np.random.randint(1 << 31))
    device = dist.get_torch_device()

    dist.log0("Loading dataset...")
    dataset = instantiate(cfg.data.dataset, split="test", _convert_="object")
    indices = select_indices(len(dataset), args.samples, args.steps, args.interval)

    dist.log0("Constructing network...")
    net, ckpt_basename = build_net(cfg, dataset, args, device)

    from .generating.products import MetricSums, product_types
    args.metrics = MetricSums in product_types(args)  # (--spectra, --rank-hist, --maps, --events and --lead-windows imply the metric sums)
    if args.dump is None:  # (see --dump: the raw store is the one-rank default, metrics only the multi-rank one)
        args.dump = "zarr" if dist.get_world_size() == 1 else "none"
        if args.dump == "none":
            args.metrics = True
            dist.log0(f"{dist.get_world_size()} ranks and no --dump given: writing the ensemble metrics only (--dump none --metrics); raw "
                      "trajectories stream at 3.4 GB/s per rank -- pass --dump zarr / numpy to get them")
    if args.dump == "none" and not args.metrics and not args.summary:
        raise ValueError("--dump none writes nothing but the metrics: add --metrics")
    odir = os.path.join(args.input, "output", ckpt_basename)
    dist.run_on_rank0(os.makedirs, odir, exist_ok=True)
    filename = f"output-{len(indices)}i-{args.steps}s-{args.members}m-{args.interval}h"
    if args.dump == "numpy":
        ofile = os.path.join(odir, f"{filename}.npy")
        dist.run_on_rank0(create_empty_numpy, ofile, len(indices), dataset.n_target_channels, dataset.img_resolution,
                          args.members, args.steps)
    elif args.dump == "none":
        ofile = os.path.join(odir, f"{filename}.none")  # (never created: names the directory evaluation_metrics.json goes to)
    else:  # zarr (the reference's default, generate.py:41-43)
        ofile = os.path.join(odir, f"{filename}.zarr")
        dist.run_on_rank0(create_empty_zarr, ofile, dataset, indices, args.members, args.steps, args.interval)

    if args.summary:
        dist.run_on_rank0(create_empty_summary, summary_path(ofile), dataset, indices, args.members, args.steps, args.interval,
                          args.quantiles)

    engine = RolloutEngine(net, dataset, interval=args.interval, solver=solver,
                           denoise_dtype=DENOISE_DTYPES[args.dtype],
                           **solver_kwargs)
    dist.log0("Rolling out samples...")
    t0 = time.time()
    rollout_and_save(engine, dataset, indices, args.members, args.steps, ofile, device, args)
    torch.cuda.synchronize()
    dist.barrier()
    el = time.time() - t0
    n = len(indices) * args.members * args.steps
    dist.log0(f"Done! Took {el:.3f} seconds: {n} sample-steps, {n / el:.1f} sample-steps/s including forcing staging and output "
              f"streaming to {os.path.basename(ofile)}.")
    if args.dump == "zarr" and dist.get_rank() == 0:  # generate.py:281-285
        zarrlite.consolidate(ofile)
    if args.summary and dist.get_rank() == 0:  # (after the barrier: every rank's chunk files are in place)
        zarrlite.consolidate(summary_path(ofile))
        dist.log0(f"ensemble summary (--summary) of {len(indices)} ICs x {args.members} members, statistics "
                  f"{', '.join(zarrlite.statistic_names(args.quantiles))} at {args.steps + 1} lead steps: {summary_path(ofile)}")
    if tdist.is_initialized():
        tdist.destroy_process_group()
    dist.log0(f"Output saved to: "
              f"{ofile if args.dump != 'none' else os.path.join(odir, 'evaluation_metrics.json') if args.metrics else summary_path(ofile)}")
    return ofile


if __name__ == "__main__":
    _args = parser.parse_args()
    check_summary_args(_args)
    check_maps_args(_args)
    check_events_args(_args)
    check_windows_args(_args)
    dist.maybe_launch_ranks(_args.gpus, "swift_amd.generate")  # before anything touches the GPU; returns in the ranks
    main(_args)
