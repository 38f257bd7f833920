"""-m gpu: ``python -m swift_amd.generate --rank-hist`` end to end.  The run directory holds nothing but ``.hydra/config.yaml``
(the composed config of a depth-2 net on the 64 x 64 grid, saved as ``swift_amd.train`` saves it) and the job runs with
``--synthetic`` weights, so no training precedes the test.  evaluation_rank_histogram.npz is recomputed with the exact reference
of tests/rank_reference.py from the trajectories the same job wrote (``--dump numpy``) and from the dataset's verifying fields;
the same job carries ``--spectra`` and writes that file too; a second job without either flag writes neither file and the same
trajectories."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rank_reference as rr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMBERS, STEPS, SAMPLES = 3, 2, 2
JOB = ["--synthetic", "--members", str(MEMBERS), "--steps", str(STEPS), "--samples", str(SAMPLES), "--batch", "6", "--dump", "numpy"]
NPY = f"output-{SAMPLES}i-{STEPS}s-{MEMBERS}m-6h.npy"
FILE = "evaluation_rank_histogram.npz"


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
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    base = tmp_path_factory.mktemp("rank_hist")
    with_flag, without = _run_dir(base / "a"), _run_dir(base / "b")
    out = _generate(with_flag, ["--rank-hist", "--spectra"])
    _generate(without, [])
    return with_flag / "output" / "synthetic", without / "output" / "synthetic", out


@pytest.fixture(scope="module")
def dataset(jobs):
    """The dataset object of the run, built from its config with the helpers ``generate`` itself uses."""
    from swift_amd import generate
    from swift_amd.config import instantiate
    rdir = jobs[0].parent.parent
    cfg = generate.load_cfg(argparse.Namespace(input=str(rdir), synthetic=True))
    ds = instantiate(cfg.data.dataset, split="test", _convert_="object")
    return ds, generate.select_indices(len(ds), SAMPLES, STEPS, 6)


@pytest.fixture(scope="module")
def hist(jobs):
    with np.load(jobs[0] / FILE, allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def test_the_flag_implies_the_metrics_and_is_logged(jobs, dataset):
    nv = len(dataset[0].variables)
    met = json.load(open(jobs[0] / "evaluation_metrics.json"))
    assert len(met) == STEPS * 3 * nv
    assert "--rank-hist" in jobs[2] and FILE in jobs[2]  # the log line names flag and file
    assert os.path.exists(jobs[0] / "evaluation_spectra.npz")  # --spectra --rank-hist together write both files


def test_layout_of_the_file(hist, dataset):
    ds = dataset[0]
    nv = len(ds.variables)
    assert sorted(hist) == sorted(["rank", "lead_hours", "variables", "frequency", "members", "samples"])
    assert hist["rank"].dtype == np.int64 and hist["rank"].tolist() == list(range(MEMBERS + 1))
    assert hist["lead_hours"].tolist() == [6, 12]
    assert hist["variables"].dtype.kind == "U" and hist["variables"].tolist() == list(ds.variables)
    assert hist["members"].shape == hist["samples"].shape == () and hist["members"].dtype == hist["samples"].dtype == np.int64
    assert int(hist["members"]) == MEMBERS and int(hist["samples"]) == SAMPLES
    assert hist["frequency"].shape == (STEPS, nv, MEMBERS + 1) and hist["frequency"].dtype == np.float64
    assert np.all(np.isfinite(hist["frequency"])) and np.all(hist["frequency"] >= 0)


def test_frequency_equals_a_recomputation_from_the_trajectories(jobs, hist, dataset):
    """The written trajectories are the device buffer's values, so kernel and reference see the same fp32 fields: the mean over
    the ICs lies within the mean of the per-IC bounds; every row sums to 1 within N + 1 of them."""
    ds, idx = dataset
    lat = ds.get_lat_lon()[0]
    w = rr.lat_weights(lat)
    a = np.load(jobs[0] / NPY)                                   # [samples, members, steps + 1, nv, H, W]
    nv, (H, W) = len(ds.variables), ds.img_resolution
    assert a.shape == (SAMPLES, MEMBERS, STEPS + 1, nv, H, W)
    norm = float(W) * float(w.sum())
    tot, tot_b = np.zeros((STEPS, nv, MEMBERS + 1)), np.zeros((STEPS, nv, MEMBERS + 1))
    for ic, j in enumerate(idx):
        pred = np.ascontiguousarray(a[ic, :, 1:].transpose(1, 0, 2, 3, 4))                          # [steps, members, nv, H, W]
        y = np.stack([np.asarray(ds.get_state(int(j) + i + 1), dtype=np.float32) for i in range(STEPS)])   # [steps, nv, H, W]
        r = rr.reference(pred, y, w) / norm
        tot, tot_b = tot + r, tot_b + rr.bound(H, MEMBERS) * r
    ref, bnd = tot / SAMPLES, tot_b / SAMPLES
    e = np.abs(hist["frequency"] - ref)
    print("frequency: worst error / bound", np.max(e[bnd > 0] / bnd[bnd > 0]))
    assert np.all(e <= bnd)
    assert np.all(hist["frequency"][ref == 0.0] == 0.0)
    s = hist["frequency"].sum(-1)
    print("row sums: worst |sum - 1| / bound", np.max(np.abs(s - 1.0)) / rr.bound(H, MEMBERS))
    assert np.all(np.abs(s - 1.0) <= (MEMBERS + 1) * rr.bound(H, MEMBERS))


def test_without_the_flag_no_file_and_the_same_trajectories(jobs):
    assert os.path.exists(jobs[0] / FILE)
    assert sorted(os.listdir(jobs[1])) == [NPY]
    assert open(jobs[0] / NPY, "rb").read() == open(jobs[1] / NPY, "rb").read()
