"""-m gpu: ``python -m swift_amd.generate --maps`` end to end.  The run directory holds nothing but ``.hydra/config.yaml`` (the
composed config of a depth-2 net on the 64 x 64 grid, saved as ``swift_amd.train`` saves it) and the jobs run with ``--synthetic``
weights, so no training precedes the test.  Job A (``--maps --batch 6``: both ICs in one batch) is recomputed with the emulation
of tests/maps_reference.py from the trajectories it wrote itself (``--dump numpy``) and from the dataset's verifying fields; job B
(``--batch 3``: one IC per batch) must write the same bytes; job C (one IC) ties the regional scores to evaluation_metrics.json,
whose RMSE convention coincides with the maps' for one IC; job D (no flag) writes neither file and the same trajectories."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import maps_reference as mr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMBERS, STEPS, SAMPLES = 3, 2, 2
JOB = ["--synthetic", "--members", str(MEMBERS), "--steps", str(STEPS), "--dump", "numpy"]
NPY = f"output-{SAMPLES}i-{STEPS}s-{MEMBERS}m-6h.npy"
NPY_ONE = f"output-1i-{STEPS}s-{MEMBERS}m-6h.npy"
STORE, REGIONS, METRICS = "evaluation_maps.zarr", "evaluation_regions.json", "evaluation_metrics.json"
F32_TOL = 1e-5   # tests/test_gpu_metric_sums.py: an fp32 metric sum lies within 1e-5 x the sum of its absolute terms


def _generate(rdir, extra):
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    e.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, "-m", "swift_amd.generate", "--input", str(rdir)] + JOB + extra, env=e, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return p.stdout


def _run_dir(path):
    from swift_amd.config import compose, to_yaml
    cfg = compose(os.path.join(ROOT, "swift_amd", "configs"), "train",
                  ["experiment=era5-swinv2-1.4-trigflow", "data=era5-synthetic-1.4", "data.dataset.img_resolution=[64,64]",
                   "data.dataset.length=48", "data.data_workers=0", "model.depth=2"])
    os.makedirs(path / ".hydra")
    with open(path / ".hydra" / "config.yaml", "w") as f:
        f.write(to_yaml({k: v for k, v in cfg.items() if k != "hydra"}))
    return path


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    """{job: output directory} and job A's log."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    base = tmp_path_factory.mktemp("maps")
    flags = dict(a=["--maps", "--samples", "2", "--batch", "6"], b=["--maps", "--samples", "2", "--batch", "3"],
                 c=["--maps", "--samples", "1", "--batch", "6"], d=["--samples", "2", "--batch", "6"])
    out, log = {}, None
    for k, extra in flags.items():
        text = _generate(_run_dir(base / k), extra)
        log = text if k == "a" else log
        out[k] = base / k / "output" / "synthetic"
    return out, log


@pytest.fixture(scope="module")
def dataset(jobs):
    """The dataset object of the runs, built from their config with the helpers ``generate`` itself uses."""
    from swift_amd import generate
    from swift_amd.config import instantiate
    rdir = jobs[0]["a"].parent.parent
    cfg = generate.load_cfg(argparse.Namespace(input=str(rdir), synthetic=True))
    return instantiate(cfg.data.dataset, split="test", _convert_="object")


def _store(d):
    from swift_amd.utils import zarrlite
    root = str(d / STORE)
    return {v: zarrlite.read_array(root, v) for v in zarrlite.list_arrays(root)}, zarrlite.read_attrs(root)


def _recompute(d, npy, ds, samples):
    """(IC-mean maps [steps, 4, nv, H, W] fp64, error term, spread term [steps, nv, H, W]) by the emulation over the job's own
    trajectories: accumulated in IC order, divided by the number of ICs."""
    from swift_amd import generate
    idx = generate.select_indices(len(ds), samples, STEPS, 6)
    a = np.load(d / npy)                                           # [samples, members, steps + 1, nv, H, W]
    assert a.shape == (samples, MEMBERS, STEPS + 1, len(ds.variables), *ds.img_resolution)
    acc, err, spr = None, 0.0, 0.0
    for ic, j in enumerate(idx):
        pred = np.ascontiguousarray(a[ic, :, 1:].transpose(1, 0, 2, 3, 4))                                  # [steps, members, nv, H, W]
        y = np.stack([np.asarray(ds.get_state(int(j) + i + 1), dtype=np.float32) for i in range(STEPS)])   # [steps, nv, H, W]
        acc = mr.emulate(pred, y, acc)
        x = pred.astype(np.float64)
        err = err + np.abs(x - y[:, None]).mean(1)
        spr = spr + sum(np.abs(x[:, m] - x[:, k]) for m in range(MEMBERS) for k in range(m + 1, MEMBERS)) / (MEMBERS * (MEMBERS - 1))
    return acc / samples, err / samples, spr / samples


@pytest.fixture(scope="module")
def recomputed(jobs, dataset):
    return _recompute(jobs[0]["a"], NPY, dataset, SAMPLES)


def test_the_flag_implies_the_metrics_and_is_logged(jobs, dataset):
    out, log = jobs
    assert len(json.load(open(out["a"] / METRICS))) == STEPS * 3 * len(dataset.variables)
    assert "--maps" in log and STORE in log and REGIONS in log     # the log line names the flag and both files
    assert sorted(os.listdir(out["a"])) == sorted([NPY, METRICS, STORE, REGIONS])


def test_layout_of_the_store(jobs, dataset):
    from swift_amd.utils import zarrlite
    ds = dataset
    (H, W), channels = ds.img_resolution, zarrlite.variable_channels(list(ds.variables))
    arrays, attrs = _store(jobs[0]["a"])
    assert attrs == {"statistics": ["bias", "mse", "crps", "variance"], "members": MEMBERS, "samples": SAMPLES}
    levels = zarrlite.compress_variables(list(ds.variables))
    coords = ["statistic", "prediction_timedelta", "latitude", "longitude"] + (["level"] if any(levels.values()) else [])
    assert sorted(arrays) == sorted(coords + list(channels))      # no time, no number
    assert arrays["statistic"].tolist() == [0, 1, 2, 3]
    assert arrays["prediction_timedelta"].tolist() == [(j + 1) * 6 * 3_600_000_000_000 for j in range(STEPS)]   # leads 1 .. steps
    lat, lon = ds.get_lat_lon()
    assert np.array_equal(arrays["latitude"], np.asarray(lat, np.float32)) and np.array_equal(arrays["longitude"], np.asarray(lon, np.float32))
    root = str(jobs[0]["a"] / STORE)
    for var, ch in channels.items():
        levelled = zarrlite.compress_variables(list(ds.variables))[var] != []
        shape, dt, dims = zarrlite.array_info(root, var)
        assert dt == np.float32 and shape == ((4, STEPS, len(ch), H, W) if levelled else (4, STEPS, H, W))
        assert dims == ["statistic", "prediction_timedelta"] + (["level"] if levelled else []) + ["latitude", "longitude"]
        meta = json.load(open(jobs[0]["a"] / STORE / var / ".zarray"))
        assert meta["chunks"] == [1, 1] + list(shape[2:]) and meta["compressor"] is None
        assert len([f for f in os.listdir(jobs[0]["a"] / STORE / var) if not f.startswith(".")]) == 4 * STEPS
        assert np.all(np.isfinite(arrays[var]))
    assert os.path.exists(jobs[0]["a"] / STORE / ".zmetadata")


def test_the_maps_are_the_emulation_over_the_written_trajectories(jobs, dataset, recomputed):
    """The written trajectories are the device buffer's values, so kernel and emulation see the same fp32 fields: the same bits."""
    from swift_amd.utils import zarrlite
    want = recomputed[0].astype(np.float32).transpose(1, 0, 2, 3, 4)                                       # [4, steps, nv, H, W]
    arrays, _ = _store(jobs[0]["a"])
    for var, ch in zarrlite.variable_channels(list(dataset.variables)).items():
        w = want[:, :, ch] if arrays[var].ndim == 5 else want[:, :, ch[0]]
        diff = arrays[var].view(np.int32) != np.ascontiguousarray(w).view(np.int32)
        print(f"{var}: {int(diff.sum())} of {diff.size} elements differ")
        assert not diff.any(), var
    assert np.all(want[1] >= 0) and np.all(want[3] >= 0) and np.any(want[0] < 0) and np.any(want[0] > 0)


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_the_result_does_not_depend_on_the_batch(jobs):
    a, b = jobs[0]["a"], jobs[0]["b"]
    assert open(a / REGIONS, "rb").read() == open(b / REGIONS, "rb").read()
    assert _files(a / STORE) == _files(b / STORE) and len(_files(a / STORE)) > 8
    for f in _files(a / STORE):
        assert open(a / STORE / f, "rb").read() == open(b / STORE / f, "rb").read(), f
    assert open(a / NPY, "rb").read() == open(b / NPY, "rb").read()


def _global_mean(field, lat):
    w = np.cos(np.deg2rad(np.asarray(lat, dtype=np.float64)))
    return np.tensordot(field.mean(-1), w / w.sum(), axes=([-1], [0]))


def test_the_global_crps_is_the_crps_of_the_metrics(jobs, dataset, recomputed):
    """evaluation_metrics.json's CRPS is the IC-mean of fp32 grid sums of the same two terms, each within 1e-5 of its sum."""
    lat = dataset.get_lat_lon()[0]
    reg, met = json.load(open(jobs[0]["a"] / REGIONS))["global"], json.load(open(jobs[0]["a"] / METRICS))
    err, spr = _global_mean(recomputed[1], lat), _global_mean(recomputed[2], lat)                           # [steps, nv]
    for j in range(STEPS):
        for i, v in enumerate(dataset.variables):
            k = f"crps_{v}_{(j + 1) * 6}h"
            print(k, reg[k], met[k], abs(reg[k] - met[k]) / (F32_TOL * (err[j, i] + spr[j, i])))
            assert abs(reg[k] - met[k]) <= F32_TOL * (err[j, i] + spr[j, i]), k


def test_for_one_ic_rmse_and_ssr_are_those_of_the_metrics(jobs, dataset):
    """One IC: sqrt(IC-mean MSE) is the IC-mean RMSE, and the two files must agree to the accuracy of the fp32 sums."""
    lat = dataset.get_lat_lon()[0]
    reg, met = json.load(open(jobs[0]["c"] / REGIONS))["global"], json.load(open(jobs[0]["c"] / METRICS))
    _, err, spr = _recompute(jobs[0]["c"], NPY_ONE, dataset, 1)
    err, spr = _global_mean(err, lat), _global_mean(spr, lat)
    for j in range(STEPS):
        for i, v in enumerate(dataset.variables):
            tag = f"{v}_{(j + 1) * 6}h"
            for stat in ("rmse", "ssr"):    # roots and ratios of sums of non-negative terms, each sum within 1e-5 of itself
                assert abs(reg[f"{stat}_{tag}"] - met[f"{stat}_{tag}"]) <= F32_TOL * abs(met[f"{stat}_{tag}"]), (stat, tag)
            assert abs(reg[f"crps_{tag}"] - met[f"crps_{tag}"]) <= F32_TOL * (err[j, i] + spr[j, i]), tag


@pytest.mark.parametrize("job", ["a", "c"])
def test_the_regions_are_the_reference_reduction_of_the_fp64_maps(jobs, dataset, recomputed, job):
    """H W = 4096 fp64 terms per regional mean: any order of adding them stays within H W u < 1e-12 of the sum of the absolute
    terms (bias and the fair CRPS are signed per pixel), the root and the ratio add two roundings."""
    lat = dataset.get_lat_lon()[0]
    mean = recomputed[0] if job == "a" else _recompute(jobs[0]["c"], NPY_ONE, dataset, 1)[0]
    got = json.load(open(jobs[0][job] / REGIONS))
    ref, scale = mr.region_scores(mean, lat, list(dataset.variables), 6), mr.region_abs(mean, lat)
    assert sorted(got) == sorted(ref) == ["global", "n_extratropics", "s_extratropics", "tropics"]
    nv = len(dataset.variables)
    for region in ref:
        assert sorted(got[region]) == sorted(ref[region]) and len(ref[region]) == 5 * nv * STEPS
        for j in range(STEPS):
            for i, v in enumerate(dataset.variables):
                tag = f"{v}_{(j + 1) * 6}h"
                assert abs(got[region][f"bias_{tag}"] - ref[region][f"bias_{tag}"]) <= 1e-12 * scale[region][j, 0, i], (region, tag)
                assert abs(got[region][f"crps_{tag}"] - ref[region][f"crps_{tag}"]) <= 1e-12 * scale[region][j, 2, i], (region, tag)
                for stat in ("rmse", "spread", "ssr"):
                    k = f"{stat}_{tag}"
                    assert abs(got[region][k] - ref[region][k]) <= 1e-12 * abs(ref[region][k]), (region, k)


def test_without_the_flag_no_file_and_the_same_trajectories(jobs):
    a, d = jobs[0]["a"], jobs[0]["d"]
    assert sorted(os.listdir(d)) == [NPY]
    assert open(a / NPY, "rb").read() == open(d / NPY, "rb").read()
