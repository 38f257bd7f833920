"""-m gpu: ``python -m swift_amd.generate --events ... --events-file ...`` end to end.  The run directories hold nothing but
``.hydra/config.yaml`` (the composed config of a depth-2 net on the 64 x 64 grid, saved as ``swift_amd.train`` saves it) and the
jobs run with ``--synthetic`` weights, so no training precedes the test.  Job A runs without the flags and writes its trajectories
(``--dump numpy``); from them and from the dataset's verifying fields the test picks the thresholds -- per scalar event the pooled
median of member and truth values, and for one variable the dataset's field at another time index with a band of NaN rows, through an
``.npz``.  Job B repeats the job with the events: same trajectories, and tables that equal tests/events_reference.py applied to
them, summed in IC order and divided by the number of ICs, bit for bit (one rank, IC-ordered adds: no rounding freedom).  Job C
repeats B with one IC per device batch: the same file."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import events_reference as er

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMBERS, STEPS, SAMPLES = 3, 2, 2
JOB = ["--synthetic", "--members", str(MEMBERS), "--steps", str(STEPS), "--samples", str(SAMPLES), "--dump", "numpy"]
NPY = f"output-{SAMPLES}i-{STEPS}s-{MEMBERS}m-6h.npy"
FILE, JSON = "evaluation_reliability.npz", "evaluation_brier.json"
SCALAR = [("2m_temperature", "lt"), ("geopotential_500", "gt"), ("2m_temperature", "gt")]     # two events on one variable
FIELD = ("u_component_of_wind_850", "gt", "another_day")
SCORES = ["brier", "fair_brier", "reliability", "resolution", "uncertainty", "bss", "base_rate"]


def _generate(rdir, extra, batch="6", ok=True):
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    e.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, "-m", "swift_amd.generate", "--input", str(rdir), "--batch", batch] + JOB + extra, env=e,
                       capture_output=True, text=True, timeout=600)
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


def _fields(ds, idx, store):
    """Per IC (pred [steps, members, nv, H, W], y [steps, nv, H, W]) fp32: the job's trajectories and the verifying fields."""
    out = []
    for ic, j in enumerate(idx):
        pred = np.ascontiguousarray(store[ic, :, 1:].transpose(1, 0, 2, 3, 4))
        y = np.stack([np.asarray(ds.get_state(int(j) + i + 1), dtype=np.float32) for i in range(STEPS)])
        out.append((pred, y))
    return out


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from swift_amd import generate
    from swift_amd.config import instantiate
    base = tmp_path_factory.mktemp("events")
    a, b, c = (_run_dir(base / k) for k in "abc")
    _generate(a, [])
    cfg = generate.load_cfg(argparse.Namespace(input=str(a), synthetic=True))
    ds = instantiate(cfg.data.dataset, split="test", _convert_="object")
    idx = generate.select_indices(len(ds), SAMPLES, STEPS, 6)
    variables, (H, W) = list(ds.variables), ds.img_resolution
    fields = _fields(ds, idx, np.load(a / "output" / "synthetic" / NPY))
    specs = []
    for var, op in SCALAR:   # the pooled median of member and truth values of the variable, as the fp32 number the spec spells
        v = variables.index(var)
        pooled = np.concatenate([np.concatenate([p[:, :, v].ravel(), y[:, v].ravel()]) for p, y in fields])
        specs.append(f"{var}:{op}:{float(np.float32(np.median(pooled)))!r}")
    field = np.asarray(ds.get_state(int(idx[0]) + 7), dtype=np.float32)[variables.index(FIELD[0])].copy()
    field[20:27] = np.nan
    npz = base / "events.npz"
    np.savez(npz, **{":".join(FIELD): field})
    flags = ["--events", *specs, "--events-file", str(npz)]
    log = _generate(b, flags)
    _generate(c, flags, batch="3")
    out = lambda r: r / "output" / "synthetic"
    return dict(a=out(a), b=out(b), c=out(c), log=log, ds=ds, idx=idx, specs=specs, field=field, npz=npz, base=base)


@pytest.fixture(scope="module")
def rel(jobs):
    with np.load(jobs["b"] / FILE, allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def expected(jobs):
    """The events as the test itself builds them, and the IC-mean table of the reference on B's trajectories."""
    ds = jobs["ds"]
    variables, (H, W) = list(ds.variables), ds.img_resolution
    names = jobs["specs"] + [":".join(FIELD)]
    ev_var = [variables.index(var) for var, _ in SCALAR] + [variables.index(FIELD[0])]
    ev_dir = [int(op == "lt") for _, op in SCALAR] + [int(FIELD[1] == "lt")]
    thr = np.stack([np.full((H, W), np.float32(float(s.rsplit(":", 1)[1])), dtype=np.float32) for s in jobs["specs"]] + [jobs["field"]])
    w = er.lat_weights(ds.get_lat_lon()[0])
    tot = None
    for pred, y in _fields(ds, jobs["idx"], np.load(jobs["b"] / NPY)):
        r = er.reference(pred, y, thr, ev_var, ev_dir, w)
        tot = r if tot is None else tot + r
    return dict(names=names, variables=[variables[v] for v in ev_var], table=tot / float(SAMPLES))


def test_without_the_flags_no_file_and_the_same_trajectories(jobs):
    assert sorted(os.listdir(jobs["a"])) == [NPY]
    assert sorted(os.listdir(jobs["b"])) == sorted([NPY, FILE, JSON, "evaluation_metrics.json"])
    assert open(jobs["a"] / NPY, "rb").read() == open(jobs["b"] / NPY, "rb").read()


def test_the_flags_imply_the_metrics_and_are_logged(jobs):
    met = json.load(open(jobs["b"] / "evaluation_metrics.json"))
    assert len(met) == STEPS * 3 * len(jobs["ds"].variables)
    assert "--events" in jobs["log"] and FILE in jobs["log"] and JSON in jobs["log"]     # one log line names flag and files


def test_layout_of_the_file(rel, expected):
    E, B = len(expected["names"]), MEMBERS + 1
    assert sorted(rel) == sorted(["events", "variables", "lead_hours", "probability", "forecast_frequency", "observed_frequency",
                                  "table", "members", "samples"])
    assert rel["events"].dtype.kind == "U" and rel["events"].tolist() == expected["names"]
    assert rel["variables"].dtype.kind == "U" and rel["variables"].tolist() == expected["variables"]
    assert rel["lead_hours"].tolist() == [6, 12] and np.array_equal(rel["probability"], np.arange(B) / MEMBERS)
    assert int(rel["members"]) == MEMBERS and int(rel["samples"]) == SAMPLES
    assert rel["table"].shape == (STEPS, E, B, 2) and rel["table"].dtype == np.float64
    assert rel["forecast_frequency"].shape == rel["observed_frequency"].shape == (STEPS, E, B)
    assert np.all(np.abs(rel["forecast_frequency"].sum(-1) - 1.0) <= 1e-12)


def test_tables_equal_a_recomputation_from_the_trajectories_bit_for_bit(jobs, rel, expected):
    assert np.array_equal(rel["table"], expected["table"])
    n_k = expected["table"].sum(-1)
    assert np.array_equal(rel["forecast_frequency"], n_k / n_k.sum(-1, keepdims=True))
    with np.errstate(divide="ignore", invalid="ignore"):
        assert np.array_equal(rel["observed_frequency"], expected["table"][..., 1] / n_k, equal_nan=True)
    # the masked band of the field event: its cells sum to the weights of the unmasked pixels only
    ds = jobs["ds"]
    w = er.lat_weights(ds.get_lat_lon()[0])
    valid = (~np.isnan(jobs["field"])).sum(-1)
    assert valid.min() == 0 and valid.max() == ds.img_resolution[1]
    np.testing.assert_allclose(rel["table"][:, -1].sum((-2, -1)), (w * valid).sum(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(rel["table"][:, 0].sum((-2, -1)), w.sum() * ds.img_resolution[1], rtol=1e-12, atol=0)


def test_scores_are_the_brier_scores_of_the_table(jobs, expected):
    from swift_amd.eval.metrics import brier_scores
    got = json.load(open(jobs["b"] / JSON))
    want = brier_scores(expected["table"], MEMBERS)
    assert sorted(got) == sorted(f"{s}_{e}_{h}h" for s in SCORES for e in expected["names"] for h in (6, 12))
    for s in SCORES:
        for i, e in enumerate(expected["names"]):
            for j, h in enumerate((6, 12)):
                g, w = got[f"{s}_{e}_{h}h"], want[s][j, i]
                assert (g is None and np.isnan(w)) or (isinstance(g, float) and abs(g - w) <= 1e-12), (s, e, h, g, w)


def test_the_scalar_events_are_not_degenerate(rel):
    """At the pooled median both outcomes occur and the members disagree somewhere: a test of tables with one cell would show little."""
    for i in range(len(SCALAR)):
        n_k = rel["table"][:, i].sum(-1)                                 # [steps, members + 1]
        base = rel["table"][:, i, :, 1].sum(-1) / n_k.sum(-1)
        print(rel["events"][i], "populated bins", (n_k > 0).sum(-1), "base rate", base)
        assert np.all((n_k > 0).sum(-1) >= 2) and np.all(base > 0) and np.all(base < 1)


def test_one_ic_per_batch_writes_the_same_arrays(jobs, rel):
    with np.load(jobs["c"] / FILE, allow_pickle=False) as f:
        c = {k: f[k] for k in f.files}
    assert sorted(c) == sorted(rel)
    for k in rel:
        assert c[k].dtype == rel[k].dtype and c[k].tobytes() == rel[k].tobytes(), k
    assert open(jobs["c"] / JSON).read() == open(jobs["b"] / JSON).read()


def test_an_unknown_variable_is_refused_before_any_gpu_work(jobs):
    d = _run_dir(jobs["base"] / "d")
    out = _generate(d, ["--events", "bogus:gt:1"], ok=False)
    assert "bogus" in out and "Loading dataset" not in out and not os.path.exists(d / "output")
