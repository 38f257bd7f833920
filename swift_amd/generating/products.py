"""What ``swift_amd.generate`` makes of a rollout: the raw store's writer and one small object per output flag.  A product gets
``add_ic(ic, traj, pred, y)`` once per initial condition, in ascending IC order -- ``traj`` [steps + 1, members, nv, H, W] the
IC's device view (lead 0 included), ``pred`` the one contiguous copy of leads 1 .. steps, ``y`` [steps, nv, H, W] the verifying
fields on the device, both None for a product that has no ``needs_truth`` -- and ``finish()`` on every rank after the loop, ranks without
ICs included: the collective and, on rank 0, the files."""
from __future__ import annotations

import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .. import dist, generate
from ..eval import metrics
from ..utils import zarrlite

RING = 4


class StoreWriter:
    """The raw trajectories' way out (``dump``: "numpy" / "zarr"; "none" writes nothing).  The reference copies every step to the
    host synchronously (generate.py:129).  GPU path: the output leaves STEP BY STEP -- as soon as a lead step of the batch is
    enqueued (``after_step``) its [B, nv, H, W] slab is copied on the side stream into one of RING pinned slabs (RING x 0.87 GB at
    96 units, instead of two whole pinned trajectories: 2 x 52 GB for 60 steps) and written from there while the following steps
    compute; at the end of a batch only its last slabs are still on their way, so a job of ONE batch (12 members x 8 ICs on a GPU)
    overlaps its output as well.  The CPU stand-in engine of the host-logic tests hands over whole trajectories (``submit_traj``)."""

    def __init__(self, dump, ofile, dataset, loaders, device):
        self.dump, self.ofile, self.loaders, self.seconds = dump, ofile, loaders, 0.0
        if dump == "numpy":
            store = np.lib.format.open_memmap(ofile, mode="r+")  # shape / data offset of the .npy the launcher created
            self.fd, self.off, shape = os.open(ofile, os.O_WRONLY), int(store.offset), tuple(store.shape)
            del store
            self.members, self.slab = shape[1], int(np.prod(shape[3:])) * 4   # [samples, members, steps + 1, nv, H, W] float32
            self.per_unit = shape[2] * self.slab
        elif dump == "zarr":
            self.channels = zarrlite.variable_channels(list(dataset.variables))
        self.thread = ThreadPoolExecutor(max_workers=1)
        self.copy_stream = torch.cuda.Stream(device=device) if torch.device(device).type == "cuda" else None
        self.ring, self.busy, self.pos = None, [None] * RING, 0  # (the CPU stand-in's one trajectory in flight: busy[0])

    def write_step(self, units, j, h):
        """h [B, nv, H, W]: lead step j of the batch's (member, IC) units."""
        t1 = time.time()
        if self.dump == "numpy":
            # every (step, unit) slab is contiguous on both sides, so the store is filled by positional writes from the loader
            # threads (pwrite releases the GIL; assigning into a memory map of the file page-faults its way through fresh pages
            # at ~3 GB/s however many threads share the mapping -- less than one GPU produces: 330 sample-steps/s x 9 MB)
            put = lambda k, m, ic: os.pwrite(self.fd, memoryview(h[k]).cast("B"),
                                             self.off + (ic * self.members + m) * self.per_unit + j * self.slab)
        else:  # one chunk file per unit and variable: independent files, written by a few threads
            put = lambda k, m, ic: zarrlite.write_unit_step(self.ofile, self.channels, ic, m, j, h[k])
        list(self.loaders.map(lambda kmi: put(kmi[0], *kmi[1]), enumerate(units)))
        self.seconds += time.time() - t1

    def write_traj(self, units, h):
        """h [steps + 1, B, nv, H, W]: a batch's whole step-major trajectory, lead step by lead step."""
        for j in range(h.shape[0]):
            self.write_step(units, j, h[j])

    def after_step(self, units):
        """``after_step`` hook of ``RolloutEngine.run`` for one batch on the GPU (None: nothing to write)."""
        def hook(j, slab_dev):
            B = slab_dev.shape[0]
            if self.ring is None or self.ring.shape[1] < B:
                self.drain()
                self.ring = torch.empty(RING, B, *slab_dev.shape[1:], dtype=torch.float32, pin_memory=True)
            slot = self.pos % RING
            self.pos += 1
            if self.busy[slot] is not None:
                self.busy[slot].result()  # the writer is done with this slab (back-pressure when the store is slower than the GPU)
            host = self.ring[slot, :B]
            ready, ev = torch.cuda.Event(), torch.cuda.Event()
            ready.record()
            with torch.cuda.stream(self.copy_stream):
                self.copy_stream.wait_event(ready)
                host.copy_(slab_dev, non_blocking=True)
                ev.record(self.copy_stream)
            self.busy[slot] = self.thread.submit(lambda: (ev.synchronize(), self.write_step(units, j, host.numpy())))
        return hook if self.dump != "none" else None

    def submit_traj(self, units, dev_buf):
        """CPU stand-in engine: the whole trajectory goes to the writer thread at once, one in flight, under the next staging."""
        if self.dump != "none":
            host = dev_buf.contiguous()
            self.drain()
            self.busy[0] = self.thread.submit(self.write_traj, units, host.numpy())

    def drain(self):
        for f in self.busy:
            if f is not None:
                f.result()

    def close(self):
        self.drain()
        self.thread.shutdown()
        if self.dump == "numpy":
            os.close(self.fd)


class Product:
    needs_truth = True

    def __init__(self, dataset, members, steps, n_ic, interval, device, odir):
        self.dataset, self.members, self.steps, self.n_ic, self.interval = dataset, members, steps, n_ic, interval
        self.device, self.odir, self.sums = device, odir, {}  # sums: IC position -> [steps, nv, 4] float64 swiftk_ensemble_sums rows
        self.lat, self.variables, self.nv, self.total = dataset.get_lat_lon()[0], dataset.variables, len(dataset.variables), None

    def add(self, t):  # this rank's ICs added in IC order on the device
        self.total = t if self.total is None else self.total + t

    def local(self, *shape):  # a rank without ICs contributes zeros
        return self.total if self.total is not None else torch.zeros(*shape, dtype=torch.float64, device=self.device)


class MetricSums(Product):
    """--metrics: swiftk_ensemble_sums of the IC's members against the verifying fields at every lead step."""

    def add_ic(self, ic, traj, pred, y):
        self.sums[ic] = metrics.ensemble_sums(pred, y, self.lat).double().cpu()

    def finish(self):
        return generate.collect_metrics(self.sums, self.n_ic, self.steps, self.nv, self.members, self.dataset, self.interval,
                                        self.device, self.odir)


class Spectra(Product):
    """--spectra: an IC's zonal power spectra [steps, nv, 3, K] fp64 on the device -- the member spectra summed over the members,
    the spectrum of the ensemble mean, the spectrum of the verifying fields."""

    def add_ic(self, ic, traj, pred, y):
        steps, members, nv, H, W = pred.shape
        member = metrics.zonal_power(pred.view(steps * members, nv, H, W), self.lat).view(steps, members, nv, -1).sum(1)
        self.add(torch.stack([member, metrics.zonal_power(pred, self.lat, group=members),
                              metrics.zonal_power(y.contiguous(), self.lat)], 2))

    def finish(self):
        generate.collect_spectra(self.local(self.steps, self.nv, 3, self.dataset.img_resolution[1] // 2 + 1), self.n_ic, self.members,
                                 self.variables, self.interval, self.odir)


class RankHistogram(Product):
    """--rank-hist: an IC's rank histograms [steps, nv, members + 1] fp64 on the device, each row summing to W sum(w_lat)."""

    def add_ic(self, ic, traj, pred, y):
        self.add(metrics.rank_histogram(pred, y.contiguous(), self.lat))

    def finish(self):
        norm = float(self.dataset.img_resolution[1]) * float(metrics.lat_weights(self.lat).sum())  # one plane's bins: W sum(w_lat)
        generate.collect_rank_histogram(self.local(self.steps, self.nv, self.members + 1), self.n_ic, self.members, self.variables,
                                        self.interval, norm, self.odir)


class Maps(Product):
    """--maps: [steps, 4, nv, H, W] float64 resident on the device: the first IC writes it, later ICs add, per pixel and in IC
    order whatever the batch, so the buffer's bits do not depend on --batch."""

    def add_ic(self, ic, traj, pred, y):
        first = self.total is None
        self.total = metrics.ensemble_maps(pred, y, self.total)
        if first:
            dist.log0(f"--maps: {self.total.numel() * 8 / 1e9:.2f} GB of fp64 maps {list(self.total.shape)} stay on each "
                      "device until the job's end")

    def finish(self):
        generate.collect_maps(self.total, self.steps, self.n_ic, self.members, self.variables, *self.dataset.get_lat_lon(),
                              self.interval, self.odir, self.device)


class Events(Product):
    """--events / --events-file: an IC's contingency tables [steps, E, members + 1, 2] fp64 on the device, the cells of an
    (event, lead) table summing to the sum over the rows of w_lat[h] times the row's unmasked pixels.  The events are parsed on the host when the
    product is made; their tables go to the device with the first IC."""

    def __init__(self, *job, specs, file):
        super().__init__(*job)
        self.names, self.ev_var, self.ev_dir, self.thr = metrics.parse_events(specs, file, self.variables, *self.dataset.img_resolution)
        self.tables = None

    def add_ic(self, ic, traj, pred, y):
        if self.tables is None:
            self.tables = metrics.event_tables_to_device(self.ev_var, self.ev_dir, self.thr, self.nv, pred.device)
        self.add(metrics.event_table(pred, y.contiguous(), self.lat, *self.tables))

    def finish(self):
        generate.collect_events(self.local(self.steps, len(self.names), self.members + 1, 2), self.n_ic, self.members, self.names,
                                [str(self.variables[v]) for v in self.ev_var], self.interval, self.odir)


class LeadWindows(Product):
    """--lead-windows: per IC the members and the verifying fields averaged over every window of leads (swiftk_lead_window_mean)
    and the swiftk_ensemble_sums of those means, [nw, nv, 4] -- a window scored like one more lead step.  The windows are parsed
    on the host when the product is made."""

    def __init__(self, *job, specs):
        super().__init__(*job)
        self.names, self.first, self.count = metrics.parse_lead_windows(specs, self.steps, self.interval)
        self.logged = False

    def add_ic(self, ic, traj, pred, y):
        pm = metrics.lead_window_mean(pred, self.first, self.count)                 # [nw, members, nv, H, W]
        ym = metrics.lead_window_mean(y.contiguous(), self.first, self.count)       # [nw, nv, H, W]
        self.sums[ic] = metrics.ensemble_sums(pm, ym, self.lat).double().cpu()
        if not self.logged:
            self.logged = True
            dist.log0(f"--lead-windows: {pm.numel() * 4 / 1e9:.2f} GB of fp32 window means {list(pm.shape)} per IC, on the device "
                      "until the IC is scored")

    def finish(self):
        generate.collect_windows(self.sums, self.n_ic, self.names, self.nv, self.members, self.dataset, self.device, self.odir)


class Summary(Product):
    """--summary: swiftk_ensemble_summary of the IC's members at every lead step, lead 0 included.  The [steps + 1, 2 + Q, nv, H,
    W] result stays on the device until the summary thread has taken it -- through one pinned buffer on a stream of its own -- and
    written its 2 + Q chunk files per variable; the rollout loop never waits for a copy, only, one batch's worth of ICs
    (``ics_per_batch``) later, for the files (back-pressure when the store is slower than the GPU)."""
    needs_truth = False

    def __init__(self, *job, quantiles, ofile, loaders, ics_per_batch):
        super().__init__(*job)
        self.quantiles, self.file, self.loaders, self.ics_per_batch = quantiles, generate.summary_path(ofile), loaders, ics_per_batch
        self.channels, self.thread = zarrlite.variable_channels(list(self.variables)), ThreadPoolExecutor(max_workers=1)
        self.stream = torch.cuda.Stream(device=self.device) if torch.device(self.device).type == "cuda" else None
        self.host, self.pending, self.seconds = None, [], 0.0

    def _flush(self, out_dev, ready, ic):
        with torch.cuda.device(self.device):
            if self.host is None:
                self.host = torch.empty(out_dev.shape, dtype=torch.float32, pin_memory=True)
            with torch.cuda.stream(self.stream):
                self.stream.wait_event(ready)
                self.host.copy_(out_dev, non_blocking=True)
            self.stream.synchronize()
        del out_dev
        t1 = time.time()
        h = self.host.numpy()  # [steps + 1, 2 + Q, nv, H, W]
        list(self.loaders.map(lambda k: zarrlite.write_unit(self.file, self.channels, ic, k, h[:, k]), range(h.shape[1])))
        self.seconds += time.time() - t1

    def add_ic(self, ic, traj, pred, y):
        out = metrics.ensemble_summary(traj, self.quantiles)
        ready = torch.cuda.Event()
        ready.record()
        while len(self.pending) >= self.ics_per_batch:
            self.pending.pop(0).result()
        self.pending.append(self.thread.submit(self._flush, out, ready, ic))

    def finish(self):
        for f in self.pending:
            f.result()
        self.thread.shutdown()


def product_types(args) -> list:
    """The product classes of a command line, in feeding order: --spectra, --rank-hist, --maps, --events / --events-file and
    --lead-windows imply the metric sums."""
    implying = [c for c, flag in ((Spectra, "spectra"), (RankHistogram, "rank_hist"), (Maps, "maps")) if getattr(args, flag, False)]
    implying += [Events] if getattr(args, "events", None) or getattr(args, "events_file", None) else []
    implying += [LeadWindows] if getattr(args, "lead_windows", None) else []
    truth = [MetricSums] + implying if implying or getattr(args, "metrics", False) else []
    return truth + ([Summary] if getattr(args, "summary", False) else [])


def products_from_args(args, dataset, members, steps, ofile, device, n_ic=None, interval=6, loaders=None) -> list:
    job = (dataset, members, steps, n_ic, interval, device, os.path.dirname(ofile))  # what every product of a job knows
    summary = dict(quantiles=getattr(args, "quantiles", None), ofile=ofile, loaders=loaders, ics_per_batch=max(1, int(args.batch) // members))
    own = {Summary: summary, Events: dict(specs=getattr(args, "events", None), file=getattr(args, "events_file", None)),
           LeadWindows: dict(specs=getattr(args, "lead_windows", None))}
    return [c(*job, **own.get(c, {})) for c in product_types(args)]


def plan_units(products, n_ic, members, batch, rank, world):
    """(units per device batch, this rank's range of units u = ic * members + member): every product takes an IC's members
    together, so with any product a batch and a rank hold whole ICs; without, the (member, IC) units themselves are sharded."""
    if not products:
        return batch, dist.shard_units(members * n_ic, rank, world)
    ics = dist.shard_units(n_ic, rank, world)
    return max(members, batch // members * members), range(ics.start * members, ics.stop * members)
