"""-m gpu: ``python -m swift_amd.generate --spectra`` end to end.  The run directory holds nothing but ``.hydra/config.yaml``
(the composed config of a depth-2 net on the 64 x 64 grid, saved as ``swift_amd.train`` saves it) and the job runs with
``--synthetic`` weights, so no training precedes the test.  evaluation_spectra.npz is recomputed with the numpy reference of
tests/spectrum_reference.py from the trajectories the same job wrote (``--dump numpy``) and from the dataset's verifying fields;
a second job without the flag writes no such file and the same trajectories."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import spectrum_reference as sp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMBERS, STEPS, SAMPLES = 2, 2, 2
JOB = ["--synthetic", "--members", str(MEMBERS), "--steps", str(STEPS), "--samples", str(SAMPLES), "--batch", "4", "--dump", "numpy"]
NPY = f"output-{SAMPLES}i-{STEPS}s-{MEMBERS}m-6h.npy"


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
    base = tmp_path_factory.mktemp("spectra")
    with_flag, without = _run_dir(base / "a"), _run_dir(base / "b")
    out = _generate(with_flag, ["--spectra"])
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
def spectra(jobs):
    with np.load(jobs[0] / "evaluation_spectra.npz", allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def test_metrics_file_is_what_it_is_without_the_flag(jobs, dataset):
    nv = len(dataset[0].variables)
    met = json.load(open(jobs[0] / "evaluation_metrics.json"))
    assert len(met) == STEPS * 3 * nv and all(np.isfinite(v) for v in met.values())
    assert "--spectra" in jobs[2] and "evaluation_spectra.npz" in jobs[2]  # the log line names flag and file


def test_layout_of_the_spectra_file(spectra, dataset):
    ds = dataset[0]
    nv, K = len(ds.variables), 33
    assert sorted(spectra) == sorted(["wavenumber", "lead_hours", "variables", "member", "ensemble_mean", "truth", "members", "samples"])
    assert spectra["wavenumber"].tolist() == list(range(K)) and spectra["lead_hours"].tolist() == [6, 12]
    assert spectra["variables"].dtype.kind == "U" and spectra["variables"].tolist() == list(ds.variables)
    assert int(spectra["members"]) == MEMBERS and int(spectra["samples"]) == SAMPLES
    for k in ("member", "ensemble_mean", "truth"):
        assert spectra[k].shape == (STEPS, nv, K) and spectra[k].dtype == np.float64
        assert np.all(np.isfinite(spectra[k])) and np.all(spectra[k] >= 0)


def test_member_and_mean_spectra_equal_a_recomputation_from_the_trajectories(jobs, spectra, dataset):
    """The written trajectories are the device buffer's values, so kernel and reference see the same fp32 fields: each averaged
    spectrum lies within the average of its terms' bounds."""
    ds = dataset[0]
    lat = ds.get_lat_lon()[0]
    a = np.load(jobs[0] / NPY)                                   # [samples, members, steps + 1, nv, H, W]
    nv, (H, W) = len(ds.variables), ds.img_resolution
    assert a.shape == (SAMPLES, MEMBERS, STEPS + 1, nv, H, W)
    member, member_b = np.zeros((STEPS, nv, W // 2 + 1)), np.zeros((STEPS, nv, W // 2 + 1))
    mean, mean_b = np.zeros_like(member), np.zeros_like(member)
    for ic in range(SAMPLES):
        for m in range(MEMBERS):
            r = sp.reference(np.ascontiguousarray(a[ic, m, 1:]), lat)
            member, member_b = member + r, member_b + sp.bound(r, 1, H, W)
        r = sp.reference(np.ascontiguousarray(a[ic, :, 1:].transpose(1, 0, 2, 3, 4)), lat, group=MEMBERS)
        mean, mean_b = mean + r, mean_b + sp.bound(r, MEMBERS, H, W)
    n = SAMPLES * MEMBERS
    e = np.abs(spectra["member"] - member / n)
    print("member: worst error / bound", np.max(e / (member_b / n)))
    assert np.all(e <= member_b / n)
    e = np.abs(spectra["ensemble_mean"] - mean / SAMPLES)
    print("ensemble mean: worst error / bound", np.max(e / (mean_b / SAMPLES)))
    assert np.all(e <= mean_b / SAMPLES)
    # Jensen: the mean's power is at most the mean power of the members
    assert np.all(spectra["ensemble_mean"].sum(-1) <= spectra["member"].sum(-1))


def test_truth_spectrum_equals_a_recomputation_from_the_dataset(spectra, dataset):
    ds, idx = dataset
    lat = ds.get_lat_lon()[0]
    H, W = ds.img_resolution
    tot, tot_b = 0.0, 0.0
    for j in idx:
        y = np.stack([np.asarray(ds.get_state(int(j) + i + 1), dtype=np.float32) for i in range(STEPS)])   # [steps, nv, H, W]
        r = sp.reference(y, lat)
        tot, tot_b = tot + r, tot_b + sp.bound(r, 1, H, W)
    e = np.abs(spectra["truth"] - tot / len(idx))
    print("truth: worst error / bound", np.max(e / (tot_b / len(idx))))
    assert np.all(e <= tot_b / len(idx))


def test_without_the_flag_no_spectra_file_and_the_same_trajectories(jobs):
    assert os.path.exists(jobs[0] / "evaluation_spectra.npz")
    assert sorted(os.listdir(jobs[1])) == [NPY]
    assert open(jobs[0] / NPY, "rb").read() == open(jobs[1] / NPY, "rb").read()
