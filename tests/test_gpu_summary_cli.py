"""-m gpu: ``python -m swift_amd.generate --summary`` end to end, on the run directory of tests/test_gpu_rank_hist_cli.py (nothing
but ``.hydra/config.yaml`` of a depth-2 net on the 64 x 64 grid, ``--synthetic`` weights).  The summary store is read back with
the standard-library zarr reader and recomputed from the trajectories the same job wrote (``--dump numpy``), at every lead step
including lead 0; the same job carries ``--rank-hist``; a second job without the flag writes no store and the same trajectories;
a third, ``--dump none --summary``, writes the store and nothing else, byte for byte the first job's."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import summary_reference as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMBERS, STEPS, SAMPLES = 3, 2, 2
QS = [0.0, 0.5, 1.0]
JOB = ["--synthetic", "--members", str(MEMBERS), "--steps", str(STEPS), "--samples", str(SAMPLES), "--batch", "6"]
SUMMARY = ["--summary", "--quantiles", "0", "0.5", "1"]
NAME = f"output-{SAMPLES}i-{STEPS}s-{MEMBERS}m-6h"
NPY, STORE = NAME + ".npy", NAME + "-summary.zarr"


def _generate(rdir, extra, ok=True):
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    e.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, "-m", "swift_amd.generate", "--input", str(rdir)] + JOB + extra, env=e, capture_output=True,
                       text=True, timeout=600)
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


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    base = tmp_path_factory.mktemp("summary")
    a, b, c = _run_dir(base / "a"), _run_dir(base / "b"), _run_dir(base / "c")
    log = _generate(a, ["--dump", "numpy", "--rank-hist"] + SUMMARY)
    _generate(b, ["--dump", "numpy"])
    _generate(c, ["--dump", "none"] + SUMMARY)
    return tuple(d / "output" / "synthetic" for d in (a, b, c)) + (log,)


@pytest.fixture(scope="module")
def variables(jobs):
    import argparse
    from swift_amd import generate
    from swift_amd.config import instantiate
    cfg = generate.load_cfg(argparse.Namespace(input=str(jobs[0].parent.parent), synthetic=True))
    return list(instantiate(cfg.data.dataset, split="test", _convert_="object").variables)


@pytest.fixture(scope="module")
def store(jobs, variables):
    """The summary store of job A as one array [samples, statistics, steps + 1, nv, H, W], channels in the dataset's order."""
    from swift_amd.utils import zarrlite
    root = str(jobs[0] / STORE)
    out = np.empty((SAMPLES, 2 + len(QS), STEPS + 1, len(variables), 64, 64), dtype=np.float32)
    for var, ch in zarrlite.variable_channels(variables).items():
        a = zarrlite.read_array(root, var)
        assert a.dtype == np.float32
        out[:, :, :, ch] = a if a.ndim == 6 else a[:, :, :, None]
    return out


def test_structure_attributes_and_log(jobs, variables):
    from swift_amd.utils import zarrlite
    root = str(jobs[0] / STORE)
    attrs = zarrlite.read_attrs(root)
    assert attrs == {"statistics": ["mean", "spread", "q0", "q0.5", "q1"], "quantiles": QS, "members": MEMBERS}
    stat = zarrlite.read_array(root, "statistic")
    assert stat.dtype == np.int64 and stat.tolist() == list(range(2 + len(QS)))
    assert "number" not in zarrlite.list_arrays(root) and os.path.exists(os.path.join(root, ".zmetadata"))
    td = zarrlite.read_array(root, "prediction_timedelta")
    assert td.dtype == np.int64 and td.tolist() == [i * 6 * 3_600_000_000_000 for i in range(STEPS + 1)]   # lead 0 included
    assert zarrlite.read_array(root, "time").shape == (SAMPLES,)
    assert zarrlite.read_array(root, "latitude").shape == zarrlite.read_array(root, "longitude").shape == (64,)
    comp = zarrlite.compress_variables(variables)
    coords = {"time", "statistic", "prediction_timedelta", "latitude", "longitude", "level"}
    assert set(zarrlite.list_arrays(root)) - coords == set(comp)
    for var, levels in comp.items():
        shape, dt, dims = zarrlite.array_info(root, var)
        lev = (len(levels),) if levels else ()
        assert shape == (SAMPLES, 2 + len(QS), STEPS + 1) + lev + (64, 64) and dt == np.float32
        assert dims == ["time", "statistic", "prediction_timedelta"] + (["level"] if levels else []) + ["latitude", "longitude"]
        chunks = sorted(f for f in os.listdir(os.path.join(root, var)) if not f.startswith("."))
        assert len(chunks) == SAMPLES * (2 + len(QS))                                        # one chunk per (IC, statistic)
        assert all(os.path.getsize(os.path.join(root, var, f)) == 4 * (STEPS + 1) * max(len(levels), 1) * 64 * 64 for f in chunks)
    assert "--summary" in jobs[3] and STORE in jobs[3]                                       # the log names flag and store
    assert os.path.exists(jobs[0] / "evaluation_rank_histogram.npz")                         # --rank-hist rode along


def test_the_store_equals_a_recomputation_from_the_trajectories(jobs, store):
    """The written trajectories are the device buffer's values, so kernel and references see the same fp32 members."""
    from swift_amd.eval.metrics import quantile_table
    a = np.load(jobs[0] / NPY)                                   # [samples, members, steps + 1, nv, H, W]
    assert a.shape == (SAMPLES, MEMBERS) + store.shape[2:]
    lo, frac = quantile_table(QS, MEMBERS)
    for ic in range(SAMPLES):
        pred = np.ascontiguousarray(a[ic].transpose(1, 0, 2, 3, 4))                          # [steps + 1, members, nv, H, W]
        got = store[ic].transpose(1, 0, 2, 3, 4)                                             # [steps + 1, statistics, nv, H, W]
        assert np.array_equal(got[:, 2:], sr.quantiles_emulated(pred, lo, frac))
        assert np.array_equal(got[:, 2], pred.min(1)) and np.array_equal(got[:, 4], pred.max(1))
        mean, s, A = sr.reference_exact(pred)
        ok_m, w_m = sr.worst(got[:, 0], mean, sr.bound_mean(mean, A, MEMBERS))
        ok_s, w_s = sr.worst(got[:, 1], s, sr.bound_spread(s, A, MEMBERS))
        print(f"IC {ic}: worst error / bound: mean {w_m:.3g}, spread {w_s:.3g}")
        assert ok_m and ok_s
        # lead 0: the members are the initial condition
        assert np.all(got[0, 1] == 0.0)
        assert all(np.array_equal(got[0, k], pred[0, 0]) for k in (0, 2, 3, 4))
        assert np.any(got[1:, 1] > 0.0)


def test_without_the_flag_no_store_and_the_same_trajectories(jobs):
    assert sorted(os.listdir(jobs[1])) == [NPY]
    assert open(jobs[0] / NPY, "rb").read() == open(jobs[1] / NPY, "rb").read()


def test_dump_none_with_the_flag_writes_the_store_alone(jobs):
    assert sorted(os.listdir(jobs[2])) == [STORE]
    files = lambda root: sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)
    assert files(jobs[0] / STORE) == files(jobs[2] / STORE)
    for f in files(jobs[0] / STORE):
        assert open(jobs[0] / STORE / f, "rb").read() == open(jobs[2] / STORE / f, "rb").read(), f


def test_bad_quantiles_are_refused_before_any_gpu_work(tmp_path):
    out = _generate(_run_dir(tmp_path / "d"), ["--dump", "none", "--summary", "--quantiles", "1.5"], ok=False)
    assert "quantile" in out and not os.path.exists(tmp_path / "d" / "output")
