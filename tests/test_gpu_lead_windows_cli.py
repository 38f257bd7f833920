"""-m gpu: ``python -m swift_amd.generate --lead-windows ...`` end to end, and the store CLI on the same job.  The run directories
hold nothing but ``.hydra/config.yaml`` (the composed config of a depth-2 net on the 64 x 64 grid) and the jobs run with
``--synthetic`` weights.  Job A runs with ``--metrics`` only and writes its trajectories (``--dump numpy``); job B adds
``--lead-windows 6-24 12-18 18-18 6-6``: the same trajectories and metrics, and an evaluation_windows.json whose every value agrees
with tests/windows_reference.py applied to the dumped trajectories and the dataset's verifying fields; job C repeats B with one IC
per device batch; job D is ``python -m swift_amd.eval.metrics --lead-windows`` on a ``--dump zarr`` run of the same job and a
truth store written from the dataset's fields.

Bounds (tests/metric_sums_reference.py, imported, not restated): the window means are bit-exact, so what separates the job from the
fp64 reference is ``swiftk_ensemble_sums`` alone -- F32_TOL relative for rmse, twice that for ssr, F32_TOL x (skill + spread term)
for crps.  Jobs C and D are held to the same bounds against B.  A one-step window against evaluation_metrics.json compares two
sets of fp32-atomic sums of the same fields: twice the bounds.  evaluation_metrics.json of A and B: rel 1e-6, what
tests/test_gpu_cli.py holds two runs of one job to.

Measured on MI355X (worst over the 4 windows x 69 variables; rmse, ssr, crps of skill + spread term): B against the reference
7.1e-8 8.9e-8 1.6e-7; C against B 6.9e-8 8.9e-8 1.4e-7; D against B 1.2e-7 1.3e-7 1.6e-7, against the reference 5.8e-8 8.6e-8 1.2e-7
[1e-5, 2e-5, 1e-5].  On the parent commit every test here fails: the flag does not exist."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import metric_sums_reference as mr
import windows_reference as wr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMBERS, STEPS, SAMPLES = 3, 4, 2
JOB = ["--synthetic", "--members", str(MEMBERS), "--steps", str(STEPS), "--samples", str(SAMPLES)]
NAME = f"output-{SAMPLES}i-{STEPS}s-{MEMBERS}m-6h"
NPY, METRICS, FILE = NAME + ".npy", "evaluation_metrics.json", "evaluation_windows.json"
SPECS = ["6-24", "12-18", "18-18", "6-6"]
WINDOWS = ["6-24h", "12-18h", "18-18h", "6-6h"]
FIRST, COUNT = [0, 1, 2, 0], [4, 2, 1, 1]
F32_TOL = mr.F32_TOL


def _generate(rdir, extra, batch="6", dump="numpy", ok=True):
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    e.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, "-m", "swift_amd.generate", "--input", str(rdir), "--batch", batch, "--dump", dump] + JOB + extra,
                       env=e, capture_output=True, text=True, timeout=600)
    assert (p.returncode == 0) == ok, p.stdout[-3000:] + p.stderr[-3000:]
    return p.stdout + p.stderr


def _run_dir(path):
    from swift_amd.config import compose, to_yaml
    cfg = compose(os.path.join(ROOT, "swift_amd", "configs"), "train",
                  ["experiment=era5-swinv2-1.4-trigflow", "data=era5-synthetic-1.4", "data.dataset.img_resolution=[64,64]",
                   "data.dataset.length=48", "data.data_workers=0", "model.depth=2"])
    os.makedirs(path / ".hydra")
    with open(path / ".hydra" / "config.yaml", "w") as f:
        f.write(to_yaml({k: v for k, v in cfg.items() if k != "hydra"}))
    return path


def _truth_store(path, ds, n_times):
    """The dataset's own fields at time indices 0 .. n_times - 1 as a truth store: one array per store variable."""
    from swift_amd.eval.metrics import PRESSURE_LEVEL_VARS
    from swift_amd.utils import zarrlite
    lat, _ = ds.get_lat_lon()
    states = np.stack([np.asarray(ds.get_state(j), dtype=np.float32) for j in range(n_times)])          # [T, nv, H, W]
    times = np.array([ds.get_time(j) for j in range(n_times)], dtype="datetime64[ns]")
    zarrlite.create_group(str(path))
    zarrlite.write_full(str(path), "time", times.astype(np.int64), ["time"], {"units": "nanoseconds since 1970-01-01"})
    zarrlite.write_full(str(path), "latitude", np.asarray(lat, dtype=np.float32), ["latitude"])
    for var, ch in zarrlite.variable_channels(list(ds.variables)).items():
        if var in PRESSURE_LEVEL_VARS:
            zarrlite.write_full(str(path), var, np.ascontiguousarray(states[:, ch]), ["time", "level", "latitude", "longitude"])
        else:
            zarrlite.write_full(str(path), var, np.ascontiguousarray(states[:, ch[0]]), ["time", "latitude", "longitude"])


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from swift_amd import generate
    from swift_amd.config import instantiate
    from swift_amd.eval import metrics as em
    base = tmp_path_factory.mktemp("windows")
    a, b, c, d = (_run_dir(base / k) for k in "abcd")
    _generate(a, ["--metrics"])
    log = _generate(b, ["--lead-windows"] + SPECS)
    _generate(c, ["--lead-windows"] + SPECS, batch="3")
    _generate(d, [], dump="zarr")
    cfg = generate.load_cfg(argparse.Namespace(input=str(a), synthetic=True))
    ds = instantiate(cfg.data.dataset, split="test", _convert_="object")
    idx = generate.select_indices(len(ds), SAMPLES, STEPS, 6)
    out = lambda r: r / "output" / "synthetic"
    truth = base / "truth.zarr"
    _truth_store(truth, ds, int(max(idx)) + STEPS + 1)
    em.main(["--truth", str(truth), "--pred", str(out(d) / (NAME + ".zarr")), "--lead-windows"] + SPECS)
    return dict(a=out(a), b=out(b), c=out(c), d=out(d), log=log, ds=ds, idx=idx, base=base)


@pytest.fixture(scope="module")
def expected(jobs):
    """The reference scores from B's dumped trajectories and the dataset's verifying fields."""
    ds, store = jobs["ds"], np.load(jobs["b"] / NPY)
    pred = np.ascontiguousarray(store[:, :, 1:].transpose(0, 2, 1, 3, 4, 5))                          # [ICs, steps, members, nv, H, W]
    y = np.stack([np.stack([np.asarray(ds.get_state(int(j) + i + 1), dtype=np.float32) for i in range(STEPS)]) for j in jobs["idx"]])
    return wr.window_scores_ref(pred, y, ds.get_lat_lon()[0], FIRST, COUNT, MEMBERS)


def _compare(got, want, variables, margin, what, skill_spread):
    """got / want: flat dicts; the bounds of this file's docstring times ``margin``; prints the worst of each score before asserting."""
    worst = dict(rmse=0.0, ssr=0.0, crps=0.0)
    for w, n in enumerate(WINDOWS):
        for i, v in enumerate(variables):
            worst["rmse"] = max(worst["rmse"], abs(got[f"rmse_{v}_{n}"] - want[f"rmse_{v}_{n}"]) / abs(want[f"rmse_{v}_{n}"]))
            worst["ssr"] = max(worst["ssr"], abs(got[f"ssr_{v}_{n}"] - want[f"ssr_{v}_{n}"]) / abs(want[f"ssr_{v}_{n}"]))
            worst["crps"] = max(worst["crps"], abs(got[f"crps_{v}_{n}"] - want[f"crps_{v}_{n}"]) / skill_spread[w, i])
    print(f"{what}: worst rmse {worst['rmse']:.2e} (bound {margin * F32_TOL:.0e}), ssr {worst['ssr']:.2e} (bound {2 * margin * F32_TOL:.0e}), "
          f"crps {worst['crps']:.2e} of skill + spread term (bound {margin * F32_TOL:.0e})")
    assert worst["rmse"] <= margin * F32_TOL and worst["ssr"] <= 2 * margin * F32_TOL and worst["crps"] <= margin * F32_TOL


def _flat(ref, variables):
    return {f"{m}_{v}_{n}": float(ref[m][w, i]) for m in ("rmse", "crps", "ssr") for w, n in enumerate(WINDOWS) for i, v in enumerate(variables)}


def test_without_the_flag_no_file_and_the_same_trajectories_and_metrics(jobs):
    assert sorted(os.listdir(jobs["a"])) == sorted([NPY, METRICS])
    assert sorted(os.listdir(jobs["b"])) == sorted([NPY, METRICS, FILE])                  # the flag implies --metrics
    assert open(jobs["a"] / NPY, "rb").read() == open(jobs["b"] / NPY, "rb").read()
    ma, mb = json.load(open(jobs["a"] / METRICS)), json.load(open(jobs["b"] / METRICS))
    assert ma.keys() == mb.keys() and len(ma) == STEPS * 3 * len(jobs["ds"].variables)
    assert all(mb[k] == pytest.approx(ma[k], rel=1e-6) for k in ma)
    assert "--lead-windows" in jobs["log"] and FILE in jobs["log"] and "window means" in jobs["log"]


def test_every_value_agrees_with_the_reference_on_the_dumped_trajectories(jobs, expected):
    variables = [str(v) for v in jobs["ds"].variables]
    got = json.load(open(jobs["b"] / FILE))
    assert len(got) == len(WINDOWS) * len(variables) * 3
    assert sorted(got) == sorted(f"{m}_{v}_{n}" for m in ("rmse", "crps", "ssr") for v in variables for n in WINDOWS)
    assert all(isinstance(x, float) and np.isfinite(x) for x in got.values())
    _compare(got, _flat(expected, variables), variables, 1, "job B against the fp64 reference", expected["skill"] + expected["spread"])
    # a window mean is smoother than a step: the 6-24 h spread term lies below the mean of the four steps' (not a bound, a sanity print)
    print("crps 6-24h / 6-6h of the first variable:", got[f"crps_{variables[0]}_6-24h"], got[f"crps_{variables[0]}_6-6h"])


def test_one_step_windows_are_the_lead_steps_of_evaluation_metrics(jobs, expected):
    variables = [str(v) for v in jobs["ds"].variables]
    got, met = json.load(open(jobs["b"] / FILE)), json.load(open(jobs["b"] / METRICS))
    ss = expected["skill"] + expected["spread"]
    for w, (n, h) in ((2, ("18-18h", "18h")), (3, ("6-6h", "6h"))):
        for i, v in enumerate(variables):
            assert abs(got[f"rmse_{v}_{n}"] - met[f"rmse_{v}_{h}"]) <= 2 * F32_TOL * abs(met[f"rmse_{v}_{h}"]), (v, n)
            assert abs(got[f"ssr_{v}_{n}"] - met[f"ssr_{v}_{h}"]) <= 4 * F32_TOL * abs(met[f"ssr_{v}_{h}"]), (v, n)
            assert abs(got[f"crps_{v}_{n}"] - met[f"crps_{v}_{h}"]) <= 2 * F32_TOL * ss[w, i], (v, n)


def test_one_ic_per_batch_agrees(jobs, expected):
    variables = [str(v) for v in jobs["ds"].variables]
    b, c = json.load(open(jobs["b"] / FILE)), json.load(open(jobs["c"] / FILE))
    assert list(b) == list(c)
    assert open(jobs["b"] / NPY, "rb").read() == open(jobs["c"] / NPY, "rb").read()
    _compare(c, b, variables, 1, "job C (--batch 3) against job B", expected["skill"] + expected["spread"])


def test_the_store_cli_agrees(jobs, expected):
    """Job D: the same trajectories through ``--dump zarr`` and the store CLI; its keys name the levels by position."""
    from swift_amd.eval.metrics import DEFAULT_PRESSURE_LEVELS, PRESSURE_LEVEL_VARS
    from swift_amd.utils import zarrlite
    variables = [str(v) for v in jobs["ds"].variables]
    d = json.load(open(jobs["d"] / FILE))
    assert len(d) == len(WINDOWS) * len(variables) * 3
    renamed = {}
    for var, ch in zarrlite.variable_channels(variables).items():
        for i, cidx in enumerate(ch):
            key = f"{var}_{DEFAULT_PRESSURE_LEVELS[i]}" if var in PRESSURE_LEVEL_VARS else var
            for m in ("rmse", "crps", "ssr"):
                for n in WINDOWS:
                    renamed[f"{m}_{variables[cidx]}_{n}"] = d[f"{m}_{key}_{n}"]
    assert len(renamed) == len(d)
    ss = expected["skill"] + expected["spread"]
    _compare(renamed, json.load(open(jobs["b"] / FILE)), variables, 1, "job D (store CLI) against job B", ss)
    _compare(renamed, _flat(expected, variables), variables, 1, "job D (store CLI) against the fp64 reference", ss)
    assert os.path.exists(jobs["d"] / METRICS)                                              # the CLI's usual file is still written


def test_a_bad_spec_is_refused_before_any_gpu_work(jobs):
    e = _run_dir(jobs["base"] / "e")
    out = _generate(e, ["--lead-windows", "6-24", "6-30"], ok=False)
    assert "6-30" in out and "Loading dataset" not in out and not os.path.exists(e / "output")
