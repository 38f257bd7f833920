"""Sampler sweep -- ``python -m swift_amd.eval.sampler`` (reference src/swift/eval/sampler.py: same flags, same defaults,
same ``RUN/output/<ckpt>/sampler_results.csv``).

    python -m swift_amd.eval.sampler --input RUN --checkpoint checkpoint-015000 --num-steps 32 16 8 4 2 1 --sigma-max 80 200

scores every ``num_steps x sigma_min x sigma_max`` combination (``itertools.product`` order, sampler.py:63) of the ``scm``
solver on one-step forecasts of the test split: per variable the latitude-weighted RMSE in physical units and their mean,
``overall_error`` (sampler.py:105-114), one CSV row per combination (sampler.py:127-131).

Where this departs from the reference's script, and why.  The script no longer runs against its own dataset class, so this
module builds what it evidently means:
  * sampler.py:91 iterates ``for X, T in dataloader`` while ``ERA5Dataset.__getitem__`` returns ``((x, t), (idx, delta))``
    (data/era5.py:190-227): here sample n is dataset item ``(idx_n, 1, --interval)``, the condition is its full standardised
    ``x`` (variables + forcings), ``t`` its standardised target, and the lead time reaches the network as ``auxiliary =
    interval / 10`` the way generate.py:255-260 passes it (the script passes none);
  * sampler.py:102-103 adds the ``C + F``-channel ``X`` to the ``C``-channel ``Y`` / ``T``: the residual base is the first
    ``C`` channels of ``x``.  A non-residual dataset is refused (the script adds ``X`` unconditionally under its
    ``# if residual`` comment);
  * sampler.py:97-99 un-standardises with the default ``delta = 6`` whatever interval the sample has: here all three use the
    sample's interval (``dataset.rollout_stats(interval)``: one delta everywhere, SST zeroed unless it is 24);
  * sampler.py:97-105 copies ``X``, ``Y`` and ``T`` to the host every batch and reduces in numpy; here one
    ``swiftk_sweep_sse`` call per combination and batch leaves a ``[B, C]`` fp64 row block on the device -- the reference's
    fp32 arithmetic per element (data/era5.py:131: ``v * s + m``, two roundings), the weighted squares summed in fp64 in a
    fixed order -- and ONE device-to-host copy per batch moves ``n_combos x B x C`` doubles.  The latitude weights are formed
    in fp64 from the latitudes (the script's are fp32 because ``get_lat_lon`` returns fp32, data/era5.py:172-175);
  * sampler.py:76-91 re-reads the dataset once per combination; here a batch is loaded once and all combinations run on it;
  * sampler.py:147 shards with a ``DistributedSampler``, which pads the last ranks with duplicates that sampler.py:106 then
    counts: here the sample list is cut into contiguous blocks (``dist.shard_units``) and ``total`` is the true sample count;
  * sampler.py:108-111 all-reduces per-rank sums, whose value depends on the sharding.  Here the per-sample rows are
    all-gathered and rank 0 adds each combination's rows in dataset-index order in fp64, so the CSV is bit-identical for any
    world size and any ``--batch`` (given the engine's guarantee that a unit's network output does not depend on batching);
  * sampler.py:89 seeds one torch generator per combination and consumes it in batch order.  Noise here is counter-based
    (``ops.unit_noise``), keyed so that a sample's draws depend on neither rank nor batch slot:
        Philox key     = rollout.unit_seed(--seed, dataset index)   (--seed in the high word, the index in the low one)
        step counter   = combination index + (k << 40)
    with k = 0 for the initial latents and k = 1, 2, ... for the ``randn_like`` draws ``scm_solver`` makes between network
    evaluations (diffusion.py:452-455) -- the keying ``RolloutEngine._randn_like`` uses, with the combination index in the
    place of the lead step;
  * pandas is not needed: the CSV is written with the ``csv`` module, floats in their shortest round-trip form (what
    ``DataFrame.to_csv`` writes); ``--batch`` is the global batch as in the reference (each rank takes ``batch // world``).
Additive flags are those of ``swift_amd.generate``: ``--dtype``, ``--gpus``, ``--samples``, ``--interval``, ``--synthetic``.
Only ``scm`` is swept, as in the reference; an ``EDMPrecond`` run is refused by ``sampler_factory``.
"""
from __future__ import annotations

import argparse
import csv
import itertools
import os
import time
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, NamedTuple, Optional, Sequence

import numpy as np
import torch
import torch.distributed as tdist

from .. import dist, generate
from ..config import instantiate
from ..generating.factory import sampler_factory
from ..rollout import unit_seed
from . import metrics

parser = argparse.ArgumentParser(parents=[generate.common_parser])
parser.add_argument("--seed", type=int, default=0, help="Random seed")
parser.add_argument("--batch", type=int, default=60, help="Global batch size")
parser.add_argument("--num-steps", type=int, nargs="+", default=[32, 16, 8, 4, 2, 1], help="Number of steps for sampling")
parser.add_argument("--sigma-min", type=float, nargs="+", default=[0.02], help="Minimum sigma values")
parser.add_argument("--sigma-max", type=float, nargs="+", default=[200.0], help="Maximum sigma values")


class Samples(NamedTuple):
    """What ``sample_experiment`` takes as its ``dataloader``: the dataset and the dataset indices of the samples to score."""
    dataset: object
    indices: Sequence[int]


def combos(args):
    """sampler.py:63."""
    return list(itertools.product(args.num_steps, args.sigma_min, args.sigma_max))


def lat_weights(dataset) -> np.ndarray:
    """sampler.py:70-72 in fp64: cos(latitude), normalised to mean 1 -- [H]."""
    return metrics.lat_weights(dataset.get_lat_lon()[0])


def _unit_noise(out: torch.Tensor, seeds: torch.Tensor, step: int) -> torch.Tensor:
    from .. import ops
    return ops.unit_noise(out, seeds, step)


class KeyedNoise:
    """The sweep's counter-based draws (module docstring): ``batch(idxs)`` keys the samples of a batch, ``start(combo)``
    begins a combination, ``latents(shape)`` is draw 0 and every ``randn_like`` call after it draw 1, 2, ...
    ``draw_fn(out, seeds, step)`` fills ``out`` [B, ...] from (seeds [B] int64, step): ``ops.unit_noise`` unless a host-logic
    test substitutes its own."""

    def __init__(self, seed: int, device, draw_fn: Optional[Callable] = None):
        self.seed, self.device, self.draw_fn = int(seed), device, draw_fn or _unit_noise
        self.seeds = None
        self.combo = self.k = 0

    def batch(self, idxs: Sequence[int]) -> "KeyedNoise":
        self.seeds = torch.tensor([unit_seed(self.seed, int(i)) for i in idxs], dtype=torch.int64, device=self.device)
        return self

    def start(self, combo: int) -> "KeyedNoise":
        self.combo, self.k = int(combo), 0
        return self

    def _draw(self, out: torch.Tensor) -> torch.Tensor:
        z = self.draw_fn(out, self.seeds, self.combo + (self.k << 40))
        self.k += 1
        return z

    def latents(self, shape) -> torch.Tensor:
        assert self.k == 0, "start(combo) first: the latents are draw 0"
        return self._draw(torch.empty(*shape, dtype=torch.float32, device=self.device))

    def randn_like(self, like: torch.Tensor) -> torch.Tensor:
        return self._draw(torch.empty_like(like, dtype=torch.float32).contiguous())


def device_score(X, Y, T, mx, sx, st, w_lat, out) -> None:
    """``score_fn`` of the product path: ``swiftk_sweep_sse`` rows of the batch into ``out`` [B, C] fp64, all on the device."""
    from .. import ops
    ops.sweep_sse(X, Y, T, mx, sx, st, w_lat, out=out)


def combine_rows(parts, n: int, world: int) -> np.ndarray:
    """Per-rank [n_combos, n, C] blocks (each valid on its own ``dist.shard_units`` range) -> [n_combos, C] sums of squared
    errors: every combination's rows added one by one in sample order, in fp64 -- the same additions whatever the world size."""
    rows = np.concatenate([np.asarray(parts[r])[:, dist.shard_units(n, r, world).start:dist.shard_units(n, r, world).stop]
                           for r in range(world)], axis=1)
    assert rows.shape[1] == n and rows.dtype == np.float64
    sse = np.zeros((rows.shape[0], rows.shape[2]), dtype=np.float64)
    for j in range(n):
        sse += rows[:, j]
    return sse


def write_results(path: str, params, variables, errors: np.ndarray) -> None:
    """sampler.py:118-131: ``num_steps, sigma_min, sigma_max, <var>_error ..., overall_error``, one row per combination."""
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(["num_steps", "sigma_min", "sigma_max"] + [f"{v}_error" for v in variables] + ["overall_error"])
        for (num_steps, sigma_min, sigma_max), e in zip(params, errors):
            w.writerow([int(num_steps), repr(float(sigma_min)), repr(float(sigma_max))] + [repr(float(d)) for d in e]
                       + [repr(float(np.mean(e)))])


@torch.no_grad()
def sample_experiment(net, dataloader, odir, args, *, score_fn: Optional[Callable] = None, factory: Optional[Callable] = None,
                      draw_fn: Optional[Callable] = None, rank: Optional[int] = None, world: Optional[int] = None,
                      gather_fn: Optional[Callable] = None):
    """sampler.py:62-131.  ``dataloader``: a ``Samples`` (or anything with ``.dataset``; every item of the dataset is then
    scored).  ``args``: num_steps / sigma_min / sigma_max lists, batch, seed, interval, dtype.  Host-logic tests replace the
    device pieces: ``score_fn(X, Y, T, mx, sx, st, w_lat, out)`` (default ``device_score``), ``factory`` (default
    ``sampler_factory``), ``draw_fn`` (``KeyedNoise``), and the process layout: ``rank`` / ``world`` and
    ``gather_fn(local [n_combos, N, C]) -> list of every rank's block``.  Returns rank 0's [n_combos, C] errors (None elsewhere)."""
    params = combos(args)
    dist.log0(f"Running {len(params)} parameter combinations")
    rank = dist.get_rank() if rank is None else rank
    world = dist.get_world_size() if world is None else world
    dataset = dataloader.dataset
    indices = [int(i) for i in getattr(dataloader, "indices", range(len(dataset)))]
    interval = int(getattr(args, "interval", 6))
    if not getattr(dataset, "residual", False):
        raise ValueError("the sampler sweep scores residual forecasts (x + y against x + t, sampler.py:101-103): this dataset is not residual")
    p = next(iter(net.parameters()), None)
    device = p.device if p is not None else torch.device("cpu")
    on_gpu = device.type == "cuda"
    score_fn, factory = score_fn or device_score, factory or sampler_factory
    noise = KeyedNoise(getattr(args, "seed", 0), device, draw_fn)
    dtype = generate.DENOISE_DTYPES[getattr(args, "dtype", "f32")]
    # every sampler is built before anything is loaded or launched: a net of the other parametrisation is refused here
    samplers = [factory("scm", net, denoise_dtype=dtype, num_steps=num_steps, sigma_min=sigma_min, sigma_max=sigma_max,
                        auxiliary=interval / 10.0, randn_like=noise.randn_like) for num_steps, sigma_min, sigma_max in params]

    C, (H, W) = dataset.n_target_channels, dataset.img_resolution
    mx, sx, st = dataset.rollout_stats(interval, device)
    w_lat = torch.from_numpy(lat_weights(dataset)).to(device)
    n = len(indices)
    mine = dist.shard_units(n, rank, world)
    batch = max(1, int(args.batch) // world)  # --batch is the global batch (sampler.py:150)
    local = torch.zeros(len(params), n, C, dtype=torch.float64)

    def stage(s):
        """Host-side inputs of the batch starting at sample s: one dataset read per sample, shared by every combination."""
        idxs = indices[s:min(s + batch, mine.stop)]
        items = [dataset[(i, 1, interval)][0] for i in idxs]
        X, T = torch.stack([x for x, _ in items], 0).float(), torch.stack([t for _, t in items], 0).float()
        return idxs, (X.pin_memory() if on_gpu else X), (T.pin_memory() if on_gpu else T)

    starts = list(range(mine.start, mine.stop, batch))
    reader = ThreadPoolExecutor(max_workers=1)
    nxt = reader.submit(stage, starts[0]) if starts else None
    t0, done = time.time(), 0
    for bi, s in enumerate(starts):
        idxs, X, T = nxt.result()
        nxt = reader.submit(stage, starts[bi + 1]) if bi + 1 < len(starts) else None  # staged while this batch computes
        X, T = X.to(device, non_blocking=True), T.to(device, non_blocking=True)
        noise.batch(idxs)
        rows = torch.empty(len(params), len(idxs), C, dtype=torch.float64, device=device)
        for i, sampler in enumerate(samplers):
            Y = sampler(X, latents=noise.start(i).latents((len(idxs), C, H, W)))
            score_fn(X, Y.contiguous(), T, mx, sx, st, w_lat, rows[i])
        local[:, s:s + len(idxs)] = rows.cpu()  # the batch's only device-to-host copy: n_combos x B x C doubles
        done += len(idxs)
        dist.log0(f"rank 0: {done}/{len(mine)} samples")
    reader.shutdown()
    if on_gpu:
        torch.cuda.synchronize()
    el = time.time() - t0
    evals = sum(int(p_[0]) for p_ in params)
    if len(mine):
        dist.log0(f"rank 0: {len(mine)} samples x {len(params)} combinations ({evals} network evaluations per sample) in {el:.3f} s: "
                  f"{1e3 * el / len(mine):.1f} ms per sample, {1e3 * el / (len(mine) * evals):.2f} ms per evaluation including "
                  "staging and scoring")

    parts = gather_fn(local) if gather_fn is not None else [q.cpu() for q in dist.all_gather_parts(local, device)]
    if rank != 0:
        return None
    sse = combine_rows([q.numpy() if isinstance(q, torch.Tensor) else q for q in parts], n, world)
    errors = np.sqrt(sse / (float(n) * H * W))  # sampler.py:113
    for (num_steps, sigma_min, sigma_max), e in zip(params, errors):
        dist.log0(f"Testing: num_steps={num_steps}, sigma_min={sigma_min}, sigma_max={sigma_max}")
        dist.log0("Per channel error")
        for v, d in zip(dataset.variables, e):
            dist.log0(f"{v}: {d:.6f}")
        dist.log0(f"Overall error: {float(np.mean(e))}")
    path = os.path.join(odir, "sampler_results.csv")
    write_results(path, params, list(dataset.variables), errors)
    dist.log0(f"Results saved to: {path}")
    return errors


def main(args):
    cfg = generate.load_cfg(args)
    dist.setup_torch(backend=cfg.system.torch.backend)
    np.random.seed(args.seed % (1 << 31))
    torch.manual_seed(args.seed)
    device = dist.get_torch_device()

    dist.log0("Loading dataset...")
    dataset = instantiate(cfg.data.dataset, split="test", _convert_="object")
    indices = generate.select_indices(len(dataset), args.samples, 1, args.interval)

    dist.log0("Constructing network...")
    net, ckpt_basename = generate.build_net(cfg, dataset, args, device)

    dist.log0("Setting up output directory/file...")
    odir = os.path.join(args.input, "output", ckpt_basename)
    dist.run_on_rank0(os.makedirs, odir, exist_ok=True)

    dist.log0("Starting Experiment...")
    sample_experiment(net, Samples(dataset, indices), odir, args)
    dist.barrier()
    if tdist.is_initialized():
        tdist.destroy_process_group()
    return os.path.join(odir, "sampler_results.csv")


if __name__ == "__main__":
    _args = parser.parse_args()
    dist.maybe_launch_ranks(_args.gpus, "swift_amd.eval.sampler")  # before anything touches the GPU; returns in the ranks
    main(_args)
