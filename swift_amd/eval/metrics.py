"""Offline ensemble metrics on the device (mirrors reference src/swift/eval/metrics.py:39-134).

``lat_weighted_rmse`` / ``lat_weighted_crps`` / ``lat_weighted_spread_skill_ratio`` keep the reference's signatures and key
names (``rmse_<var>_<postfix>`` ...); all three come out of ONE pass over the ensemble (``swiftk_ensemble_sums``: the N member
values of a grid point are read once into registers; the reference materialises a [B, N, N, H, W] difference tensor per
variable).  ``python -m swift_amd.eval.metrics --truth T.zarr --pred P.zarr`` is the reference's CLI (eval/metrics.py:157-280: both
stores, the structured evaluation_metrics.json), walking the forecast store one initial condition at a time through the
standard-library zarr reader (zarr / xarray are not in this image); ``--pred output.npy --truth truth.npy --lat lat.npy`` evaluates
the ``--dump numpy`` output of ``swift_amd.generate``.
"""
from __future__ import annotations

import argparse
import json
import os
from typing import Dict, Sequence

import numpy as np
import torch

from .._lib import check, lib


def lat_weights(lat) -> np.ndarray:
    """cos(latitude), normalised to mean 1, in fp64 -- [H]: the weights of every whole-grid score here and in the sampler sweep."""
    w = np.cos(np.deg2rad(np.asarray(lat, dtype=np.float64)))
    return w / w.mean()


def ensemble_sums(pred: torch.Tensor, y: torch.Tensor, lat) -> torch.Tensor:
    """pred [B, N, V, H, W], y [B, V, H, W] (device, fp32) -> [B, V, 4] weighted grid sums (see include/swiftk.h)."""
    assert pred.is_cuda and y.is_cuda and pred.ndim == 5 and y.ndim == 4
    B, N, V, H, W = pred.shape
    w_lat = torch.from_numpy(lat_weights(lat)).float().to(pred.device).contiguous()
    pred, y = pred.contiguous().float(), y.contiguous().float()
    out = torch.zeros(B, V, 4, device=pred.device)
    check(lib().swiftk_ensemble_sums(pred.data_ptr(), y.data_ptr(), w_lat.data_ptr(), out.data_ptr(), B, N, V, H, W,
                                     torch.cuda.current_stream().cuda_stream), "swiftk_ensemble_sums")
    return out


_SPECTRUM_TABLES: dict = {}  # (W, latitudes, device) -> (w_lat [H], twiddle [W, 2]) fp64 on the device


def _spectrum_tables(W: int, lat, device):
    lat = np.ascontiguousarray(lat, dtype=np.float64)
    key = (W, lat.tobytes(), str(device))
    if key not in _SPECTRUM_TABLES:
        a = 2.0 * np.pi * np.arange(W, dtype=np.float64) / W
        _SPECTRUM_TABLES[key] = (torch.from_numpy(lat_weights(lat)).to(device),
                                 torch.from_numpy(np.stack([np.cos(a), np.sin(a)], 1)).to(device).contiguous())
    return _SPECTRUM_TABLES[key]


def zonal_power(fields: torch.Tensor, lat, group: int = 1) -> torch.Tensor:
    """Latitude-weighted one-sided zonal power spectra, wavenumbers 0 .. W/2 (definition: include/swiftk.h,
    ``swiftk_zonal_power``; summed over k a spectrum is the plane's latitude-weighted mean square).  fields [n, group, V, H, W]
    (or [n, V, H, W] when ``group == 1``), fp32 on the device -> [n, V, W/2 + 1] fp64 on the device; with ``group > 1`` the
    spectrum is that of the mean over the ``group`` consecutive planes (the members of an ensemble)."""
    if fields.ndim == 4 and group == 1:
        fields = fields.unsqueeze(1)
    if not (fields.is_cuda and fields.ndim == 5 and fields.dtype == torch.float32 and fields.shape[1] == group):
        raise ValueError(f"zonal_power: fp32 device fields [n, {group}, V, H, W] expected, got {fields.dtype} "
                         f"{tuple(fields.shape)} on {fields.device}")
    n, G, V, H, W = fields.shape
    fields = fields.contiguous()
    w_lat, twiddle = _spectrum_tables(W, lat, fields.device)
    if w_lat.numel() != H:
        raise ValueError(f"zonal_power: {w_lat.numel()} latitudes for {H} rows")
    out = torch.empty(n, V, W // 2 + 1, dtype=torch.float64, device=fields.device)  # written completely by every call
    check(lib().swiftk_zonal_power(fields.data_ptr(), w_lat.data_ptr(), twiddle.data_ptr(), out.data_ptr(), n, G, V, H, W,
                                   torch.cuda.current_stream().cuda_stream), "swiftk_zonal_power")
    return out


def rank_histogram(pred: torch.Tensor, y: torch.Tensor, lat) -> torch.Tensor:
    """Latitude-weighted rank (Talagrand) histograms (definition: include/swiftk.h, ``swiftk_rank_histogram``: a pixel with b
    members below the truth and e equal to it adds w_lat[h] / (e + 1) to the bins b .. b + e, so a row sums to W sum(w_lat)).
    pred [n, N, V, H, W], y [n, V, H, W], fp32 on the device -> [n, V, N + 1] fp64 on the device."""
    if not (pred.is_cuda and y.is_cuda and pred.ndim == 5 and y.ndim == 4 and pred.dtype == torch.float32
            and y.dtype == torch.float32 and y.device == pred.device
            and tuple(y.shape) == (pred.shape[0],) + tuple(pred.shape[2:])):
        raise ValueError(f"rank_histogram: fp32 device pred [n, N, V, H, W] and y [n, V, H, W] expected, got {pred.dtype} "
                         f"{tuple(pred.shape)} on {pred.device} and {y.dtype} {tuple(y.shape)} on {y.device}")
    n, N, V, H, W = pred.shape
    pred, y = pred.contiguous(), y.contiguous()
    w_lat, _ = _spectrum_tables(W, lat, pred.device)   # the fp64 weights of the spectra (the twiddle table rides along unused)
    if w_lat.numel() != H:
        raise ValueError(f"rank_histogram: {w_lat.numel()} latitudes for {H} rows")
    out = torch.empty(n, V, N + 1, dtype=torch.float64, device=pred.device)  # written completely by every call
    check(lib().swiftk_rank_histogram(pred.data_ptr(), y.data_ptr(), w_lat.data_ptr(), out.data_ptr(), n, N, V, H, W,
                                      torch.cuda.current_stream().cuda_stream), "swiftk_rank_histogram")
    return out


EVENT_OPERATORS = {"gt": 0, "lt": 1}  # the direction word of an event spec -> ev_dir of swiftk_event_table


def parse_events(specs, file, variables, H=None, W=None):
    """The threshold events of ``generate --events SPEC ... --events-file FILE.npz`` -> (names [E], ev_var int32 [E], ev_dir int32
    [E], thr float32 [E, H, W]), the tables of ``swiftk_event_table`` on the host.  A spec is ``<variable>:<gt|lt>:<value>``
    (``2m_temperature:lt:273.15``: the event is the variable strictly below 273.15); the file is an ``.npz`` (loaded with
    ``allow_pickle=False``) whose keys are ``<variable>:<gt|lt>:<label>`` and whose values are a scalar or an [H, W] float array,
    NaN where a pixel is to be left out (a climatological percentile field computed offline, a land mask).  The event's name is
    the spec as typed, or the key; specs come first, then the file's keys in the file's order.  ``ValueError`` -- pure host
    work, before any rank is started or the GPU is touched -- for an unknown variable, a bad operator, a non-finite scalar, a
    field of the wrong shape, a duplicate name, no events at all.  Without (H, W) the field shapes are not checked (any 2-d
    field passes) and ``thr`` is None: what the launcher can check before the dataset is open."""
    variables = [str(v) for v in variables]
    entries = [(str(s), None) for s in (specs or [])]
    if file:
        with np.load(file, allow_pickle=False) as f:
            entries += [(str(k), np.asarray(f[k])) for k in f.files]
    if not entries:
        raise ValueError("events: no events given (--events <variable>:<gt|lt>:<value> ... or a non-empty --events-file)")
    names, ev_var, ev_dir, fields = [], [], [], []
    for name, value in entries:
        parts = name.split(":", 2)
        if len(parts) != 3:
            raise ValueError(f"events: '{name}' is not <variable>:<gt|lt>:<{'label' if value is not None else 'value'}>")
        var, op, last = parts
        if var not in variables:
            raise ValueError(f"events: '{name}' names the variable '{var}', which this run does not have ({', '.join(variables)})")
        if op not in EVENT_OPERATORS:
            raise ValueError(f"events: '{name}' has the operator '{op}', expected one of {', '.join(EVENT_OPERATORS)}")
        if name in names:
            raise ValueError(f"events: '{name}' is given twice")
        if value is None:
            try:
                value = np.asarray(float(last))
            except ValueError:
                raise ValueError(f"events: '{name}' has the threshold '{last}', expected a number") from None
        if value.dtype.kind not in "fiu":
            raise ValueError(f"events: '{name}' holds {value.dtype} values, expected numbers")
        if value.ndim == 0:
            if not np.isfinite(value):
                raise ValueError(f"events: '{name}' has the threshold {float(value)}, expected a finite number")
        elif value.ndim != 2 or (H is not None and tuple(value.shape) != (int(H), int(W))):
            raise ValueError(f"events: '{name}' holds a field of shape {tuple(value.shape)}, expected a scalar or "
                             f"{[int(H), int(W)] if H is not None else '[H, W]'}")
        names.append(name), ev_var.append(variables.index(var)), ev_dir.append(EVENT_OPERATORS[op]), fields.append(value)
    thr = None
    if H is not None:
        thr = np.stack([np.broadcast_to(np.asarray(f, dtype=np.float32), (int(H), int(W))) for f in fields]).astype(np.float32)
    return names, np.asarray(ev_var, dtype=np.int32), np.asarray(ev_dir, dtype=np.int32), thr


def event_tables_to_device(ev_var, ev_dir, thr, V: int, device):
    """The host tables of ``parse_events`` checked against a V-channel ensemble (``ValueError``) and put on ``device``:
    (ev_var int32 [E], ev_dir int32 [E], thr fp32 [E, H, W]), what ``event_table`` takes call after call."""
    ev_var, ev_dir = np.asarray(ev_var), np.asarray(ev_dir)
    thr = np.ascontiguousarray(thr, dtype=np.float32)
    if not (ev_var.ndim == 1 and ev_var.size > 0 and ev_var.shape == ev_dir.shape and ev_var.dtype.kind in "iu"
            and ev_dir.dtype.kind in "iub" and thr.ndim == 3 and thr.shape[0] == ev_var.size):
        raise ValueError(f"event_table: ev_var [E] and ev_dir [E] integers and thr [E, H, W] expected, got {ev_var.dtype} "
                         f"{ev_var.shape}, {ev_dir.dtype} {ev_dir.shape} and {thr.shape}")
    if ev_var.min() < 0 or ev_var.max() >= V:
        raise ValueError(f"event_table: ev_var {ev_var.tolist()} outside the {V} channels")
    return (torch.from_numpy(ev_var.astype(np.int32)).to(device), torch.from_numpy((ev_dir != 0).astype(np.int32)).to(device),
            torch.from_numpy(thr).to(device))


def event_table(pred: torch.Tensor, y: torch.Tensor, lat, ev_var, ev_dir, thr) -> torch.Tensor:
    """Latitude-weighted contingency tables of threshold events (definition: include/swiftk.h, ``swiftk_event_table``: a pixel
    with k members in the event and outcome o adds w_lat[h] to cell (k, o); a NaN threshold leaves the pixel out).  pred [n, N,
    V, H, W], y [n, V, H, W], fp32 on the device -> [n, E, N + 1, 2] fp64 on the device.  ``ev_var`` / ``ev_dir`` [E] and ``thr``
    [E, H, W] as host arrays (``parse_events``) are checked against V here and uploaded; given as device tensors (int32, int32,
    fp32: ``event_tables_to_device``, once per job) they are taken as they are -- reading them back would stall the stream --
    and the kernel clamps a channel outside [0, V - 1]."""
    if not (isinstance(pred, torch.Tensor) and isinstance(y, torch.Tensor) and pred.is_cuda and y.is_cuda and pred.ndim == 5
            and y.ndim == 4 and pred.dtype == torch.float32 and y.dtype == torch.float32 and y.device == pred.device
            and tuple(y.shape) == (pred.shape[0],) + tuple(pred.shape[2:]) and 1 <= pred.shape[1] <= 64 and pred.numel() > 0):
        raise ValueError(f"event_table: fp32 device pred [n, N, V, H, W] with N <= 64 and y [n, V, H, W] expected, got "
                         f"{getattr(pred, 'dtype', type(pred))} {tuple(getattr(pred, 'shape', ()))} on {getattr(pred, 'device', None)} "
                         f"and {getattr(y, 'dtype', type(y))} {tuple(getattr(y, 'shape', ()))} on {getattr(y, 'device', None)}")
    n, N, V, H, W = pred.shape
    if not all(isinstance(t, torch.Tensor) for t in (ev_var, ev_dir, thr)):
        ev_var, ev_dir, thr = event_tables_to_device(ev_var, ev_dir, thr, V, pred.device)
    E = ev_var.numel()
    if not (ev_var.dtype == torch.int32 and ev_dir.dtype == torch.int32 and thr.dtype == torch.float32 and E > 0
            and ev_var.ndim == 1 and tuple(ev_dir.shape) == (E,) and tuple(thr.shape) == (E, H, W)
            and ev_var.device == ev_dir.device == thr.device == pred.device):
        raise ValueError(f"event_table: int32 ev_var [E], int32 ev_dir [E] and fp32 thr [E, {H}, {W}] on {pred.device} expected, got "
                         f"{ev_var.dtype} {tuple(ev_var.shape)}, {ev_dir.dtype} {tuple(ev_dir.shape)}, {thr.dtype} {tuple(thr.shape)} "
                         f"on {thr.device}")
    pred, y, ev_var, ev_dir, thr = pred.contiguous(), y.contiguous(), ev_var.contiguous(), ev_dir.contiguous(), thr.contiguous()
    w_lat, _ = _spectrum_tables(W, lat, pred.device)   # the fp64 weights of the spectra (the twiddle table rides along unused)
    if w_lat.numel() != H:
        raise ValueError(f"event_table: {w_lat.numel()} latitudes for {H} rows")
    out = torch.empty(n, E, N + 1, 2, dtype=torch.float64, device=pred.device)  # written completely by every call
    check(lib().swiftk_event_table(pred.data_ptr(), y.data_ptr(), thr.data_ptr(), ev_var.data_ptr(), ev_dir.data_ptr(),
                                   w_lat.data_ptr(), out.data_ptr(), n, N, V, H, W, E, torch.cuda.current_stream().cuda_stream),
          "swiftk_event_table")
    return out


BRIER_SCORES = ["brier", "fair_brier", "reliability", "resolution", "uncertainty", "bss", "base_rate"]


def brier_scores(table, members: int) -> Dict[str, np.ndarray]:
    """Brier score and its decomposition from contingency tables [..., E, N + 1, 2] (``event_table``, or any positive multiple of
    sums of them) -> {score: [..., E] fp64}, pure host code.  With n_k = T[k,0] + T[k,1], o_k = T[k,1], p_k = k / N, S = sum n_k:
    ``base_rate`` = sum o_k / S; ``brier`` = sum [o_k (1 - p_k)^2 + (n_k - o_k) p_k^2] / S; ``reliability`` = sum n_k (p_k -
    o_k / n_k)^2 / S and ``resolution`` = sum n_k (o_k / n_k - base_rate)^2 / S over the non-empty bins; ``uncertainty`` =
    base_rate (1 - base_rate); ``fair_brier`` = brier - sum n_k k (N - k) / (N^2 (N - 1)) / S (Ferro's ensemble-size correction:
    NaN for one member); ``bss`` = 1 - brier / uncertainty, NaN where the uncertainty is 0.  The forecast takes exactly the
    N + 1 values p_k, so brier = reliability - resolution + uncertainty holds exactly in real arithmetic.  A table without any
    pixel (an all-NaN threshold field) gives NaN everywhere, without a warning."""
    T = np.asarray(table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else table, dtype=np.float64)
    N = int(members)
    if N < 1 or T.ndim < 2 or T.shape[-2:] != (N + 1, 2):
        raise ValueError(f"brier_scores: tables [..., {N + 1}, 2] of {N} >= 1 members expected, got {T.shape}")
    n_k, o_k = T[..., 0] + T[..., 1], T[..., 1]
    k = np.arange(N + 1, dtype=np.float64)
    p, S = k / N, n_k.sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        base = o_k.sum(-1) / S
        brier = (o_k * (1.0 - p) ** 2 + (n_k - o_k) * p ** 2).sum(-1) / S
        obar = o_k / n_k
        full = n_k > 0
        rel = np.where(full, n_k * (p - obar) ** 2, 0.0).sum(-1) / S
        res = np.where(full, n_k * (obar - base[..., None]) ** 2, 0.0).sum(-1) / S
        unc = base * (1.0 - base)
        fair = brier - (n_k * k * (N - k)).sum(-1) / (float(N) ** 2 * (N - 1)) / S if N >= 2 else np.full(S.shape, np.nan)
        bss = np.where(unc > 0, 1.0 - brier / unc, np.nan)
    return dict(brier=brier, fair_brier=fair, reliability=rel, resolution=res, uncertainty=unc, bss=bss, base_rate=base)


MAX_QUANTILES = 16  # what swiftk_ensemble_summary takes in one call


def quantile_table(quantiles, N: int):
    """Host side of the quantiles of ``ensemble_summary``: for each q in [0, 1] the position p = q (N - 1) among the N sorted
    members, in fp64, as (lo int32 [Q], frac float64 [Q]) with lo = floor(p), frac = p - lo (numpy's default ``linear`` method);
    q = 1 gives (N - 1, 0.0).  ``ValueError`` for a q outside [0, 1] or not finite, for more than 16 quantiles, for N < 2."""
    q = np.asarray(list(quantiles), dtype=np.float64).reshape(-1)
    if int(N) < 2:
        raise ValueError(f"quantile_table: at least 2 members, got {N}")
    if q.size > MAX_QUANTILES:
        raise ValueError(f"quantile_table: at most {MAX_QUANTILES} quantiles, got {q.size}")
    if not np.all(np.isfinite(q)) or np.any(q < 0.0) or np.any(q > 1.0):
        raise ValueError(f"quantile_table: quantiles must be finite numbers in [0, 1], got {q.tolist()}")
    p = q * np.float64(int(N) - 1)
    lo = np.floor(p)
    return lo.astype(np.int32), p - lo


_QUANTILE_TABLES: dict = {}  # (quantiles, N, device) -> (lo int32 [Q], frac fp64 [Q]) on the device


def ensemble_summary(pred: torch.Tensor, quantiles=(0.1, 0.5, 0.9)) -> torch.Tensor:
    """Per-pixel mean, spread (unbiased standard deviation) and quantiles over the members (definition: include/swiftk.h,
    ``swiftk_ensemble_summary``: fp64 in member order, quantiles as selections plus one interpolation).  pred [n, N, V, H, W] fp32
    on the device -> [n, 2 + Q, V, H, W] fp32 on the device: statistic 0 the mean, 1 the spread, 2 + j quantile j."""
    if not (isinstance(pred, torch.Tensor) and pred.is_cuda and pred.ndim == 5 and pred.dtype == torch.float32
            and 2 <= pred.shape[1] <= 64 and pred.numel() > 0):
        raise ValueError(f"ensemble_summary: fp32 device pred [n, N, V, H, W] with 2 <= N <= 64 expected, got "
                         f"{getattr(pred, 'dtype', type(pred))} {tuple(getattr(pred, 'shape', ()))} on {getattr(pred, 'device', None)}")
    n, N, V, H, W = pred.shape
    key = (tuple(float(q) for q in quantiles), N, str(pred.device))
    if key not in _QUANTILE_TABLES:
        lo, frac = quantile_table(key[0], N)
        _QUANTILE_TABLES[key] = (torch.from_numpy(lo).to(pred.device), torch.from_numpy(frac).to(pred.device))
    lo, frac = _QUANTILE_TABLES[key]
    Q = len(key[0])
    pred = pred.contiguous()
    out = torch.empty(n, 2 + Q, V, H, W, dtype=torch.float32, device=pred.device)  # written completely by every call
    check(lib().swiftk_ensemble_summary(pred.data_ptr(), lo.data_ptr() if Q else None, frac.data_ptr() if Q else None,
                                        out.data_ptr(), n, N, V, H, W, Q, torch.cuda.current_stream().cuda_stream),
          "swiftk_ensemble_summary")
    return out


MAP_STATISTICS = ["bias", "mse", "crps", "variance"]  # the statistic axis of ensemble_maps, in order


def ensemble_maps(pred: torch.Tensor, y: torch.Tensor, acc: torch.Tensor = None) -> torch.Tensor:
    """Per-pixel bias, squared error, fair CRPS and member variance of an ensemble against the verifying fields (definition:
    include/swiftk.h, ``swiftk_ensemble_maps``: fp64 in member order, nothing fused).  pred [n, N, V, H, W] and y [n, V, H, W],
    fp32 on the device, 2 <= N <= 64 -> [n, 4, V, H, W] fp64 on the device, the statistics in the order of ``MAP_STATISTICS``.
    Without ``acc`` the result is a new buffer, written completely; with ``acc`` (such a buffer, contiguous) the terms are added
    to it in place, one rounded add each, and ``acc`` is returned: the sum over initial conditions that ``generate --maps`` keeps."""
    if not (isinstance(pred, torch.Tensor) and isinstance(y, torch.Tensor) and pred.is_cuda and y.is_cuda and pred.ndim == 5
            and y.ndim == 4 and pred.dtype == torch.float32 and y.dtype == torch.float32 and y.device == pred.device
            and tuple(y.shape) == (pred.shape[0],) + tuple(pred.shape[2:]) and 2 <= pred.shape[1] <= 64 and pred.numel() > 0):
        raise ValueError(f"ensemble_maps: fp32 device pred [n, N, V, H, W] with 2 <= N <= 64 and y [n, V, H, W] expected, got "
                         f"{getattr(pred, 'dtype', type(pred))} {tuple(getattr(pred, 'shape', ()))} on {getattr(pred, 'device', None)} "
                         f"and {getattr(y, 'dtype', type(y))} {tuple(getattr(y, 'shape', ()))} on {getattr(y, 'device', None)}")
    n, N, V, H, W = pred.shape
    if acc is not None and not (isinstance(acc, torch.Tensor) and acc.dtype == torch.float64 and acc.device == pred.device
                                and tuple(acc.shape) == (n, 4, V, H, W) and acc.is_contiguous()):
        raise ValueError(f"ensemble_maps: acc must be a contiguous fp64 [{n}, 4, {V}, {H}, {W}] buffer on {pred.device}, got "
                         f"{getattr(acc, 'dtype', type(acc))} {tuple(getattr(acc, 'shape', ()))} on {getattr(acc, 'device', None)}")
    pred, y = pred.contiguous(), y.contiguous()
    accumulate = int(acc is not None)
    if acc is None:
        acc = torch.empty(n, 4, V, H, W, dtype=torch.float64, device=pred.device)  # written completely by the call
    check(lib().swiftk_ensemble_maps(pred.data_ptr(), y.data_ptr(), acc.data_ptr(), n, N, V, H, W, accumulate,
                                     torch.cuda.current_stream().cuda_stream), "swiftk_ensemble_maps")
    return acc


MAX_LEAD_WINDOWS, LEAD_WINDOWS_PER_CALL = 32, 8  # what a job takes; what swiftk_lead_window_mean takes in one call
WINDOWS_FILE = "evaluation_windows.json"


def parse_lead_windows(specs, steps: int, interval: int):
    """The lead-time windows of ``generate --lead-windows SPEC ...`` -> (names [nw], first int32 [nw], count int32 [nw]), the host
    tables of ``lead_window_mean`` over the leads 1 .. ``steps`` of a rollout (row 0 is the lead ``interval`` hours).  A spec is
    ``A-B`` or ``A-Bh``: the lead hours A to B, both ends included (``6-168`` is week 1 of a 6-hourly job); its name is
    ``<A>-<B>h``.  ``ValueError`` naming the spec -- pure host work, before any rank is started or the GPU is touched -- for a
    malformed spec, A below ``interval`` (lead 0 is not a forecast), A > B, A or B not a multiple of ``interval``, B beyond
    ``steps * interval``, a window given twice, more than 32 windows, none at all."""
    import re
    steps, interval = int(steps), int(interval)
    specs = [str(s) for s in (specs or [])]
    if not specs:
        raise ValueError("lead windows: no windows given (--lead-windows <A>-<B> ..., lead hours, both ends included)")
    if len(specs) > MAX_LEAD_WINDOWS:
        raise ValueError(f"lead windows: at most {MAX_LEAD_WINDOWS} windows, got {len(specs)}: '{specs[MAX_LEAD_WINDOWS]}' is one too many")
    names, first, count = [], [], []
    for spec in specs:
        m = re.fullmatch(r"(\d+)-(\d+)h?", spec)
        if not m:
            raise ValueError(f"lead windows: '{spec}' is not <A>-<B> or <A>-<B>h (lead hours, both ends included)")
        a, b = int(m.group(1)), int(m.group(2))
        if a < interval:
            raise ValueError(f"lead windows: '{spec}' starts at {a} h, before the first forecast lead {interval} h (lead 0 is not a forecast)")
        if a > b:
            raise ValueError(f"lead windows: '{spec}' ends before it starts")
        if a % interval or b % interval:
            raise ValueError(f"lead windows: '{spec}' does not lie on the {interval}-hourly leads of this job")
        if b > steps * interval:
            raise ValueError(f"lead windows: '{spec}' ends after the last lead of this job, {steps * interval} h ({steps} steps of {interval} h)")
        name = f"{a}-{b}h"
        if name in names:
            raise ValueError(f"lead windows: '{spec}' is given twice")
        names.append(name), first.append(a // interval - 1), count.append((b - a) // interval + 1)
    return names, np.asarray(first, dtype=np.int32), np.asarray(count, dtype=np.int32)


def _window_tables(what: str, first, count, n: int):
    first, count = np.asarray(first), np.asarray(count)
    if not (first.ndim == 1 and first.size > 0 and first.shape == count.shape and first.dtype.kind in "iu" and count.dtype.kind in "iu"):
        raise ValueError(f"{what}: first [nw] and count [nw] integers expected, got {first.dtype} {first.shape} and {count.dtype} {count.shape}")
    first, count = first.astype(np.int64), count.astype(np.int64)
    if first.min() < 0 or count.min() < 1 or (first + count).max() > n:
        raise ValueError(f"{what}: windows first {first.tolist()} count {count.tolist()} do not lie inside the {n} lead rows")
    return first, count


def lead_window_mean(x: torch.Tensor, first, count) -> torch.Tensor:
    """Means over windows of the leading (lead-time) axis (definition: include/swiftk.h, ``swiftk_lead_window_mean``: an fp64
    running sum in lead order from the window's first element, one division, one cast).  x [n, ...] contiguous fp32 on the device,
    ``first`` / ``count`` [nw] host integers (``parse_lead_windows``): window w the rows first[w] .. first[w] + count[w] - 1 ->
    [nw, ...] fp32 on the device, written completely.  More than 8 windows go out as several launches of at most 8."""
    import ctypes
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.ndim >= 1 and x.dtype == torch.float32 and x.numel() > 0
            and x.is_contiguous()):
        raise ValueError(f"lead_window_mean: a contiguous fp32 device tensor [n, ...] expected, got "
                         f"{getattr(x, 'dtype', type(x))} {tuple(getattr(x, 'shape', ()))} on {getattr(x, 'device', None)}")
    n = x.shape[0]
    M = x.numel() // n
    first, count = _window_tables("lead_window_mean", first, count, n)
    nw = first.size
    out = torch.empty((nw,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)  # written completely by the calls
    for w0 in range(0, nw, LEAD_WINDOWS_PER_CALL):
        k = min(LEAD_WINDOWS_PER_CALL, nw - w0)
        f, c = (ctypes.c_int * k)(*first[w0:w0 + k].tolist()), (ctypes.c_int * k)(*count[w0:w0 + k].tolist())
        check(lib().swiftk_lead_window_mean(x.data_ptr(), out.data_ptr() + w0 * M * 4, f, c, n, k, M,
                                            torch.cuda.current_stream().cuda_stream), "swiftk_lead_window_mean")
    return out


def window_scores(sums, names, variables, members: int, hw) -> Dict[str, float]:
    """Per-IC ``ensemble_sums`` rows of window-mean fields, sums [n_ic, nw, nv, 4] fp64 -> the flat ``evaluation_windows.json``
    dict ``rmse_`` / ``crps_`` / ``ssr_<var>_<A>-<B>h``: ``scores_from_sums`` per window, the conventions of
    evaluation_metrics.json (the IC-mean of the per-IC RMSE, and so on)."""
    sums = sums if isinstance(sums, torch.Tensor) else torch.from_numpy(np.asarray(sums, dtype=np.float64))
    res = {}
    for w, name in enumerate(names):
        rmse, crps, ssr = scores_from_sums(sums[:, w], members, hw)    # [n_ic, nv, 4] -> [nv] each
        for i, v in enumerate(variables):
            res[f"rmse_{v}_{name}"], res[f"crps_{v}_{name}"], res[f"ssr_{v}_{name}"] = float(rmse[i]), float(crps[i]), float(ssr[i])
    return res


def region_means(maps: np.ndarray, lat) -> Dict[str, np.ndarray]:
    """Latitude-weighted regional means of maps [..., H, W] (fp64) -> {region: [...]}: weights cos(lat), normalised over the
    region's rows.  Regions (the WeatherBench2 bands): ``global``, ``tropics`` (|lat| <= 20), ``n_extratropics`` (lat >= 20),
    ``s_extratropics`` (lat <= -20); a region with no rows on the grid is left out."""
    lat = np.asarray(lat, dtype=np.float64)
    w = np.cos(np.deg2rad(lat))
    rows = {"global": np.ones(lat.shape, dtype=bool), "tropics": np.abs(lat) <= 20.0, "n_extratropics": lat >= 20.0,
            "s_extratropics": lat <= -20.0}
    maps = np.asarray(maps, dtype=np.float64)
    out = {}
    for name, sel in rows.items():
        if sel.any():
            ws = w[sel] / w[sel].sum()
            out[name] = np.tensordot(maps[..., sel, :].mean(-1), ws, axes=([-1], [0]))
    return out


def scores_from_sums(s: torch.Tensor, n_members: int, hw):
    """``ensemble_sums`` rows s [B, ..., 4] (fp64) on a grid of ``hw`` points -> (rmse, crps, ssr) [...] (eval/metrics.py:39-134)."""
    B, N = s.shape[0], n_members
    rmse = torch.sqrt(s[..., 0] / hw).mean(0)
    crps = s[..., 1].sum(0) / (B * N * hw) - (s[..., 2] / hw / (2 * N * (N - 1))).mean(0)
    ssr = torch.sqrt(s[..., 3] / hw).mean(0) / rmse
    return rmse, crps, ssr


def all_metrics(pred: torch.Tensor, y: torch.Tensor, vars: Sequence[str], lat, log_postfix: str) -> Dict[str, torch.Tensor]:
    B, N, V, H, W = pred.shape
    rmse, crps, ssr = scores_from_sums(ensemble_sums(pred, y, lat).double(), N, H * W)
    out = {}
    for i, v in enumerate(vars):
        out[f"rmse_{v}_{log_postfix}"], out[f"crps_{v}_{log_postfix}"], out[f"ssr_{v}_{log_postfix}"] = rmse[i], crps[i], ssr[i]
    return out


def _pick(prefix):
    def fn(pred, y, vars, lat, log_postfix):
        if pred.ndim == 4:  # reference: deterministic input -> plain RMSE
            pred = torch.stack([pred, pred], 1)
        return {k: v for k, v in all_metrics(pred, y, vars, lat, log_postfix).items() if k.startswith(prefix)}
    return fn


lat_weighted_rmse = _pick("rmse_")
lat_weighted_crps = _pick("crps_")
lat_weighted_spread_skill_ratio = _pick("ssr_")


# --------------------------------------------------------------------------------- store-to-store evaluation (eval/metrics.py:157-280)
# (the reference's schema: which store variables carry a level axis, and the level values its metric names use)
PRESSURE_LEVEL_VARS = ["geopotential", "u_component_of_wind", "v_component_of_wind", "vertical_velocity", "wind_speed", "temperature",
                       "relative_humidity", "specific_humidity", "vorticity", "potential_vorticity"]
DEFAULT_PRESSURE_LEVELS = [50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000]
_COORDS = {"time", "number", "prediction_timedelta", "level", "latitude", "longitude"}
_UNIT_NS = {"nanoseconds": 1, "microseconds": 10**3, "milliseconds": 10**6, "seconds": 10**9, "minutes": 60 * 10**9,
            "hours": 3600 * 10**9, "days": 86400 * 10**9}


def _unit_ns(word: str) -> int:
    w = word.strip().lower()
    w = w if w.endswith("s") else w + "s"
    if w not in _UNIT_NS:
        raise ValueError(f"unknown CF time unit {word!r}")
    return _UNIT_NS[w]


def _cf_times(root: str, name: str = "time") -> np.ndarray:
    """A CF-encoded time coordinate (``units: '<unit> since <date>'``, what xarray writes and ``xr.open_zarr`` decodes) -> datetime64[ns]."""
    from ..utils import zarrlite
    v = zarrlite.read_array(root, name)
    if v.dtype.kind == "M":
        return v.astype("datetime64[ns]")
    units = str(zarrlite.read_attrs(root, name).get("units", "nanoseconds since 1970-01-01"))
    unit, _, ref = units.partition(" since ")
    ref_ns = np.datetime64(ref.strip().replace(" ", "T").rstrip("Z") or "1970-01-01", "ns").astype(np.int64)
    ns = np.round(v.astype(np.float64) * _unit_ns(unit)).astype(np.int64) if v.dtype.kind == "f" else v.astype(np.int64) * _unit_ns(unit)
    return (ns + ref_ns).astype("datetime64[ns]")


def _cf_lead_hours(root: str, name: str = "prediction_timedelta") -> list:
    from ..utils import zarrlite
    v = zarrlite.read_array(root, name)
    if v.dtype.kind == "m":
        return [int(x) for x in v.astype("timedelta64[h]").astype(np.int64)]
    unit = str(zarrlite.read_attrs(root, name).get("units", "nanoseconds"))
    return [int(x) for x in (v.astype(np.float64) * _unit_ns(unit) / _UNIT_NS["hours"]).round().astype(np.int64)]


def evaluate_stores(truth: str, pred: str, device=None, sums_fn=None, log=print, windows=None, mean_fn=None):
    """The reference's ``python -m swift.eval.metrics --truth T.zarr --pred P.zarr`` (eval/metrics.py:157-222): for every lead time of
    the forecast store and every variable (pressure-level variables level by level), latitude-weighted ensemble-mean RMSE, CRPS
    and spread/skill ratio against the truth store's fields at ``init time + lead`` -- keys ``<metric>_<var>[_<level>]_<lead>h``.

    The reference loads both stores whole (``ds[v].values``: 100+ GB for the 15-day 12 x 128 job) and evaluates lead by lead; here
    the forecast store is walked one initial condition at a time (``zarrlite.read_region``: one unit = one chunk file per variable
    in the layout ``generate`` writes), the [lead, member, level, H, W] block of that IC goes to the device once and ONE
    ``swiftk_ensemble_sums`` launch per variable and IC yields the sums of every lead and level; the per-IC sums are combined at
    the end exactly as the reference's batch means are.  ``sums_fn(pred[T, N, V, H, W], y[T, V, H, W], lat) -> [T, V, 4]``
    replaces the device kernel in the host-logic tests.

    ``windows`` (the specs of ``--lead-windows``, checked by ``parse_lead_windows`` against the store's own lead times) adds the
    scores of the lead-time-mean fields: per IC and variable the block and its verifying fields are averaged over every window
    (``swiftk_lead_window_mean``) and the means go through the same sums -- and the call returns (flat, flat_windows), the second
    dict with the keys ``<metric>_<var>[_<level>]_<A>-<B>h`` of evaluation_windows.json.  ``mean_fn(x[T, ...], first, count) ->
    [nw, ...]`` replaces that kernel in the host-logic tests."""
    from ..utils import zarrlite
    if sums_fn is None or (windows and mean_fn is None):
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if sums_fn is None:
        sums_fn = lambda p, y, lat: ensemble_sums(torch.from_numpy(p).to(dev), torch.from_numpy(y).to(dev), lat).double().cpu().numpy()
    if windows and mean_fn is None:
        mean_fn = lambda x, first, count: lead_window_mean(torch.from_numpy(x).to(dev), first, count).cpu().numpy()
    lat = zarrlite.read_array(truth, "latitude").astype(np.float64)
    init_times, truth_times = _cf_times(pred), _cf_times(truth)
    where = {int(t): i for i, t in enumerate(truth_times.astype(np.int64))}
    try:
        init_idx = np.array([where[int(t)] for t in init_times.astype(np.int64)])
    except KeyError as e:
        raise ValueError(f"initial time {np.datetime64(int(e.args[0]), 'ns')} of the forecast store is not in the truth store") from None
    dt_truth = int((truth_times[1] - truth_times[0]).astype("timedelta64[h]").astype(np.int64))
    leads = _cf_lead_hours(pred)
    offs = [h // dt_truth for h in leads]
    if init_idx.max() + max(offs) >= len(truth_times):
        raise ValueError("the truth store ends before the forecasts' last verification time")
    if windows:
        lead0 = int(leads[0] == 0)  # (the stores of generate begin with the initial condition, lead 0: not a forecast)
        fl = leads[lead0:]
        if not fl or fl[0] <= 0 or fl != [(j + 1) * fl[0] for j in range(len(fl))]:
            raise ValueError(f"lead windows: the forecast store's lead times {leads} h are not the steps 1 .. n of one interval")
        wnames, wfirst, wcount = parse_lead_windows(windows, len(fl), fl[0])
    out: Dict[str, float] = {}
    wout: Dict[str, float] = {}
    for var in [v for v in zarrlite.list_arrays(pred) if v not in _COORDS]:
        shape, _dt, _dims = zarrlite.array_info(pred, var)
        levelled = var in PRESSURE_LEVEL_VARS
        if levelled != (len(shape) == 6):
            raise ValueError(f"{var}: {len(shape)}-d array, but the reference's schema says it has {'a' if levelled else 'no'} level axis")
        B, N, T = shape[:3]
        L = shape[3] if levelled else 1
        names = [f"{var}_{DEFAULT_PRESSURE_LEVELS[i]}" for i in range(L)] if levelled else [var]  # (by position, as the reference)
        sums = np.zeros((B, T, L, 4))
        wsums = np.zeros((B, len(wnames), L, 4)) if windows else None
        for b in range(B):
            p = np.asarray(zarrlite.read_region(pred, var, (b,)), dtype=np.float32)                 # [N, T, (L,) H, W]
            y = np.stack([np.asarray(zarrlite.read_region(truth, var, (int(init_idx[b] + o),)), dtype=np.float32) for o in offs], 0)
            if not levelled:
                p, y = p[:, :, None], y[:, None]
            p, y = np.ascontiguousarray(p.transpose(1, 0, 2, 3, 4)), np.ascontiguousarray(y)
            sums[b] = sums_fn(p, y, lat)
            if windows:
                wsums[b] = sums_fn(mean_fn(p[lead0:], wfirst, wcount), mean_fn(y[lead0:], wfirst, wcount), lat)
        hw = float(shape[-1] * shape[-2])
        for j, h in enumerate(leads):   # the batch statistics of eval/metrics.py:39-134 from the per-IC sums (as generate --metrics)
            rmse, crps, ssr = scores_from_sums(torch.from_numpy(sums[:, j]), N, hw)
            for i, nm in enumerate(names):
                out[f"crps_{nm}_{h}h"], out[f"rmse_{nm}_{h}h"], out[f"ssr_{nm}_{h}h"] = float(crps[i]), float(rmse[i]), float(ssr[i])
        if windows:
            wout.update(window_scores(wsums, wnames, names, N, hw))
        log(f"{var}: {B} initial conditions x {N} members x {T} lead times" + (f" x {L} levels" if levelled else "")
            + (f", {len(wnames)} lead windows" if windows else ""))
    return (out, wout) if windows else out


def structure(flat: Dict[str, float]) -> Dict[str, dict]:
    """metric type -> lead time (hours, as a string) -> variable name, as the reference's evaluation_metrics.json (eval/metrics.py:234-252)."""
    res: Dict[str, dict] = {}
    for key, value in flat.items():
        parts = key.split("_")
        res.setdefault(parts[0], {}).setdefault(parts[-1][:-1], {})["_".join(parts[1:-1])] = float(value)
    return res


def main(argv=None):
    """``--truth T.zarr --pred P.zarr``: the reference's CLI and output file (structured evaluation_metrics.json beside the forecast
    store).  ``--pred output.npy --truth truth.npy [--lat lat.npy]``: the ``--dump numpy`` form of ``swift_amd.generate`` (additive)."""
    import time
    ap = argparse.ArgumentParser()
    ap.add_argument("--truth", required=True, help="Path to ground-truth (zarr store; or npy (samples, steps+1, C, H, W) in physical units)")
    ap.add_argument("--pred", required=True, help="Path to prediction (zarr store of swift.generate; or its output-*.npy)")
    ap.add_argument("--lat", default=None, help="npy mode: latitudes (default: linspace(-90, 90, H))")
    ap.add_argument("--interval", type=int, default=6, help="npy mode: hours per step")
    ap.add_argument("--lead-windows", type=str, nargs="+", default=None, metavar="SPEC", help="zarr mode: also score the means over "
                    "the lead hours A to B (both included) of each SPEC A-B, as generate --lead-windows -> evaluation_windows.json")
    a = ap.parse_args(argv)
    if a.lead_windows and a.pred.rstrip("/").endswith(".npy"):
        raise SystemExit("--lead-windows scores a zarr forecast store (--pred P.zarr --truth T.zarr); the npy mode does not take it")
    if not a.pred.rstrip("/").endswith(".npy"):
        t0 = time.time()
        flat = evaluate_stores(a.truth, a.pred, windows=a.lead_windows)
        if a.lead_windows:
            flat, wflat = flat
            wpath = os.path.join(os.path.dirname(os.path.abspath(a.pred.rstrip("/"))), WINDOWS_FILE)
            with open(wpath, "w") as f:
                json.dump(wflat, f, indent=1)
            print(f"wrote {wpath} ({len(wflat)} metrics of {len(a.lead_windows)} lead windows)")
        path = os.path.join(os.path.dirname(os.path.abspath(a.pred.rstrip("/"))), "evaluation_metrics.json")
        with open(path, "w") as f:
            json.dump({"metadata": {"prediction_file": os.path.abspath(a.pred), "truth_file": os.path.abspath(a.truth),
                                    "time": time.strftime("%Y-%m-%d %H:%M:%S UTC", time.gmtime()), "timestamp": time.time()},
                       "metrics": structure(flat)}, f, indent=2)
        print(f"wrote {path} ({len(flat)} metrics, {time.time() - t0:.1f} s)")
        return flat
    dev = torch.device("cuda", 0)
    pred, truth = np.load(a.pred, mmap_mode="r"), np.load(a.truth, mmap_mode="r")
    S, N, T, C, H, W = pred.shape
    lat = np.load(a.lat) if a.lat else np.linspace(-90, 90, H)
    names = [f"var{i}" for i in range(C)]
    res = {}
    for j in range(1, T):
        p = torch.from_numpy(np.ascontiguousarray(pred[:, :, j])).to(dev)
        y = torch.from_numpy(np.ascontiguousarray(truth[:, j])).to(dev)
        res.update({k: float(v) for k, v in all_metrics(p, y, names, lat, f"{j * a.interval}h").items()})
    path = os.path.join(os.path.dirname(os.path.abspath(a.pred)), "evaluation_metrics.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {path} ({len(res)} metrics)")


if __name__ == "__main__":
    main()
