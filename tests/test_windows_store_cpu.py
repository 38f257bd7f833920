"""Host logic of ``python -m swift_amd.eval.metrics --truth T.zarr --pred P.zarr --lead-windows ...`` on the CPU:
``evaluate_stores(..., windows=, sums_fn=, mean_fn=)`` with numpy stand-ins for the two kernels on a tiny zarr pair written with
``zarrlite`` -- a surface variable and a two-level one, three ICs, the forecast store beginning with lead 0 as ``generate`` writes
it.  Keys and values against tests/windows_reference.py; without ``windows`` the call returns what it always did."""
import os

import numpy as np
import pytest

import windows_reference as wr

NAMES = ["2m_temperature", "geopotential_500", "geopotential_850"]
KEYS = ["2m_temperature", "geopotential_50", "geopotential_100"]        # (levels are named by position, as the reference does)
H, W, B, N, STEPS, INTERVAL = 4, 8, 3, 3, 4, 6
INIT = [2, 5, 9]
WINDOWS = ["6-24", "12-18h", "18-18"]


def _sums(p, y, lat):
    """The four sums of swiftk_ensemble_sums in numpy fp64: p [T, N, V, H, W], y [T, V, H, W] -> [T, V, 4]."""
    p, y = p.astype(np.float64), y.astype(np.float64)
    w = wr.lat_weights(lat).reshape(1, 1, -1, 1)
    s0 = (w * (p.mean(1) - y) ** 2).sum((-2, -1))
    s1 = (w[:, None] * np.abs(p - y[:, None])).sum((1, -2, -1))
    s2 = (w[:, None, None] * np.abs(p[:, :, None] - p[:, None])).sum((1, 2, -2, -1))
    s3 = (w * p.var(1, ddof=1)).sum((-2, -1))
    return np.stack([s0, s1, s2, s3], -1)


@pytest.fixture(scope="module")
def stores(tmp_path_factory):
    from swift_amd.utils import zarrlite
    base = tmp_path_factory.mktemp("windows_store")
    rng = np.random.default_rng(5)
    lat = np.linspace(-80, 80, H)
    t_all = np.datetime64("2020-01-01T00") + np.arange(20) * np.timedelta64(6, "h")
    pred = str(base / "run" / f"output-{B}i-{STEPS}s-{N}m-{INTERVAL}h.zarr")
    os.makedirs(os.path.dirname(pred))
    ch = zarrlite.create_forecast_store(pred, NAMES, t_all[INIT], lat, np.arange(W) * 45.0, members=N, steps=STEPS, interval=INTERVAL)
    traj = (280.0 + rng.standard_normal((B, N, STEPS + 1, 3, H, W))).astype(np.float32)
    for b in range(B):
        for n in range(N):
            zarrlite.write_unit(pred, ch, b, n, traj[b, n])
    truth = str(base / "truth.zarr")
    zarrlite.create_group(truth)
    zarrlite.write_full(truth, "time", (np.arange(20) * 6).astype(np.int64), ["time"],
                        {"units": "hours since 2020-01-01 00:00:00", "calendar": "proleptic_gregorian"})
    zarrlite.write_full(truth, "latitude", lat.astype(np.float32), ["latitude"])
    fields = (280.0 + rng.standard_normal((20, 3, H, W))).astype(np.float32)
    zarrlite.write_full(truth, "2m_temperature", fields[:, 0], ["time", "latitude", "longitude"])
    zarrlite.write_full(truth, "geopotential", fields[:, 1:], ["time", "level", "latitude", "longitude"])
    return dict(truth=truth, pred=pred, traj=traj, fields=fields, lat=lat)


def test_windows_of_a_store_against_the_reference(stores):
    from swift_amd.eval import metrics as em
    flat, wflat = em.evaluate_stores(stores["truth"], stores["pred"], sums_fn=_sums, mean_fn=wr.window_mean_ref, windows=WINDOWS,
                                     log=lambda *_: None)
    plain = em.evaluate_stores(stores["truth"], stores["pred"], sums_fn=_sums, log=lambda *_: None)
    assert isinstance(plain, dict) and plain == flat and len(flat) == 3 * (STEPS + 1) * 3   # without the flag: as before
    names = ["6-24h", "12-18h", "18-18h"]
    assert sorted(wflat) == sorted(f"{m}_{k}_{n}" for m in ("rmse", "crps", "ssr") for k in KEYS for n in names)
    first, count = [0, 1, 2], [4, 2, 1]
    p = np.ascontiguousarray(stores["traj"][:, :, 1:].transpose(0, 2, 1, 3, 4, 5))                 # [B, steps, N, 3, H, W]
    y = np.stack([stores["fields"][i + 1:i + 1 + STEPS] for i in INIT])                             # [B, steps, 3, H, W]
    ref = wr.window_scores_ref(p, y, stores["lat"], first, count, N)
    for w, n in enumerate(names):
        for i, k in enumerate(KEYS):
            assert wflat[f"rmse_{k}_{n}"] == pytest.approx(ref["rmse"][w, i], rel=1e-9)
            assert wflat[f"ssr_{k}_{n}"] == pytest.approx(ref["ssr"][w, i], rel=1e-9)
            assert abs(wflat[f"crps_{k}_{n}"] - ref["crps"][w, i]) <= 1e-9 * (ref["skill"][w, i] + ref["spread"][w, i])
    # a one-step window is that lead's instantaneous score
    for k in KEYS:
        for m in ("rmse", "crps", "ssr"):
            assert wflat[f"{m}_{k}_18-18h"] == pytest.approx(flat[f"{m}_{k}_18h"], rel=1e-9)
    assert set(em.structure(wflat)["crps"]) == {"6-24", "12-18", "18-18"}


def test_a_window_the_store_does_not_hold_is_refused(stores):
    from swift_amd.eval import metrics as em
    with pytest.raises(ValueError, match="6-30"):
        em.evaluate_stores(stores["truth"], stores["pred"], sums_fn=_sums, mean_fn=wr.window_mean_ref, windows=["6-30"], log=lambda *_: None)


def test_the_npy_mode_refuses_the_flag():
    from swift_amd.eval import metrics as em
    with pytest.raises(SystemExit) as e:
        em.main(["--truth", "truth.npy", "--pred", "output.npy", "--lead-windows", "6-12"])
    assert "--lead-windows" in str(e.value) and "zarr" in str(e.value)
