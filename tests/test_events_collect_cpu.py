"""The combine step of ``swift_amd.generate --events`` on the CPU (``collect_events``): every rank hands in ONE [steps, E,
members + 1, 2] fp64 array, the sum of the per-IC tables of its ICs in IC order; rank 0 adds the ranks' arrays in rank order and
writes evaluation_reliability.npz and evaluation_brier.json.  One process against two gloo ranks on fake per-IC tables: the two
sets of files differ by the reordering of at most n_ic positive fp64 terms per cell -- 1e-12 relative is 10^3 times that."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, N_IC, MEMBERS, INTERVAL = 3, 5, 6, 12
EVENTS = ["2m_temperature:lt:273.15", "geopotential_500:gt:p90", "2m_temperature:gt:303.15", "10m_wind:gt:masked"]
VARIABLES = ["2m_temperature", "geopotential_500", "2m_temperature", "10m_wind"]
SCORES = ["brier", "fair_brier", "reliability", "resolution", "uncertainty", "bss", "base_rate"]


def _tables():
    """Fake per-IC tables [n_ic, steps, E, members + 1, 2]: positive, uneven; event 2 never observed (its outcome column 1 is
    zero: no uncertainty, so no skill score) and with an empty forecast bin; event 3 fully masked (all zeros)."""
    t = np.random.default_rng(29).lognormal(0.0, 2.0, (N_IC, STEPS, len(EVENTS), MEMBERS + 1, 2))
    t[:, :, 2, :, 1] = 0.0
    t[:, :, 2, 4] = 0.0
    t[:, :, 3] = 0.0
    return t


WORKER = textwrap.dedent("""
    import sys
    import numpy as np, torch
    sys.path.insert(0, %(root)r)
    sys.path.insert(0, %(tests)r)
    from swift_amd import dist
    from swift_amd.generate import collect_events
    import test_events_collect_cpu as t
    dist.setup_torch(backend="gloo")
    tables = t._tables()
    mine = dist.shard_units(t.N_IC, dist.get_rank(), dist.get_world_size())
    local = torch.zeros(t.STEPS, len(t.EVENTS), t.MEMBERS + 1, 2, dtype=torch.float64)
    for ic in mine:                                                                  # IC order, as the product adds them
        local = local + torch.from_numpy(tables[ic])
    collect_events(local, t.N_IC, t.MEMBERS, t.EVENTS, t.VARIABLES, t.INTERVAL, sys.argv[1])
    dist.barrier()
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()
""")


def test_two_gloo_ranks_write_what_one_process_writes(tmp_path):
    from swift_amd.eval.metrics import brier_scores
    script = tmp_path / "worker.py"
    script.write_text(WORKER % {"root": ROOT, "tests": os.path.join(ROOT, "tests")})
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    one, two = tmp_path / "one", tmp_path / "two"
    os.makedirs(one), os.makedirs(two)
    subprocess.run([sys.executable, str(script), str(one)], check=True, env={**env, "WORLD_SIZE": "1", "RANK": "0"}, timeout=200)
    port = str(29600 + (os.getpid() + 163) % 300)
    procs = [subprocess.Popen([sys.executable, str(script), str(two)],
                              env={**env, "WORLD_SIZE": "2", "RANK": str(r), "LOCAL_RANK": str(r), "MASTER_PORT": port})
             for r in range(2)]
    assert [p.wait(timeout=200) for p in procs] == [0, 0]
    assert sorted(os.listdir(one)) == sorted(os.listdir(two)) == ["evaluation_brier.json", "evaluation_reliability.npz"]
    with np.load(one / "evaluation_reliability.npz", allow_pickle=False) as f:
        a = {k: f[k] for k in f.files}
    with np.load(two / "evaluation_reliability.npz", allow_pickle=False) as f:
        b = {k: f[k] for k in f.files}
    E, B = len(EVENTS), MEMBERS + 1
    # layout
    assert sorted(a) == sorted(b) == sorted(["events", "variables", "lead_hours", "probability", "forecast_frequency",
                                             "observed_frequency", "table", "members", "samples"])
    assert a["events"].dtype.kind == "U" and a["events"].tolist() == EVENTS
    assert a["variables"].dtype.kind == "U" and a["variables"].tolist() == VARIABLES
    assert a["lead_hours"].dtype == np.int64 and a["lead_hours"].tolist() == [12, 24, 36]
    assert a["members"].shape == a["samples"].shape == () and a["members"].dtype == a["samples"].dtype == np.int64
    assert int(a["members"]) == MEMBERS and int(a["samples"]) == N_IC
    assert a["probability"].dtype == np.float64 and np.array_equal(a["probability"], np.arange(B) / MEMBERS)
    assert a["table"].shape == (STEPS, E, B, 2) and a["table"].dtype == np.float64
    assert a["forecast_frequency"].shape == a["observed_frequency"].shape == (STEPS, E, B)
    # values: against the tables themselves
    mean = _tables().sum(0) / N_IC
    n_k = mean.sum(-1)
    np.testing.assert_allclose(a["table"], mean, rtol=1e-12, atol=0)
    live = [0, 1, 2]                                                     # (event 3 is fully masked: 0 / 0 everywhere)
    np.testing.assert_allclose(a["forecast_frequency"][:, live], n_k[:, live] / n_k[:, live].sum(-1, keepdims=True), rtol=1e-12, atol=0)
    assert np.all(np.abs(a["forecast_frequency"][:, live].sum(-1) - 1.0) <= 1e-12)
    full = n_k > 0
    np.testing.assert_allclose(a["observed_frequency"][full], (mean[..., 1] / np.where(full, n_k, 1.0))[full], rtol=1e-12, atol=0)
    assert np.all(np.isnan(a["observed_frequency"][~full])) and np.all(~full[:, 2, 4]) and np.all(~full[:, 3])
    assert np.all(np.isnan(a["forecast_frequency"][:, 3]))
    # two ranks against one: integer-valued arrays equal, float arrays to 1e-12
    for k in a:
        if a[k].dtype.kind == "f":
            np.testing.assert_allclose(b[k], a[k], rtol=1e-12, atol=0, equal_nan=True)
        else:
            assert np.array_equal(a[k], b[k])
    # the scores: brier_scores of the written table, NaN as null, floats otherwise
    ja, jb = json.load(open(one / "evaluation_brier.json")), json.load(open(two / "evaluation_brier.json"))
    assert sorted(ja) == sorted(jb) == sorted(f"{s}_{e}_{h}h" for s in SCORES for e in EVENTS for h in (12, 24, 36))
    assert "NaN" not in open(one / "evaluation_brier.json").read()
    want = brier_scores(a["table"], MEMBERS)
    for s in SCORES:
        for i, e in enumerate(EVENTS):
            for j, h in enumerate((12, 24, 36)):
                got, got2, w = ja[f"{s}_{e}_{h}h"], jb[f"{s}_{e}_{h}h"], want[s][j, i]
                if np.isnan(w):
                    assert got is None and got2 is None
                else:
                    assert isinstance(got, float) and abs(got - w) <= 1e-12 and abs(got2 - got) <= 1e-12
    assert ja[f"bss_{EVENTS[2]}_12h"] is None and ja[f"brier_{EVENTS[3]}_24h"] is None     # no uncertainty; no pixels
    assert ja[f"base_rate_{EVENTS[2]}_12h"] == 0.0 and 0.0 < ja[f"base_rate_{EVENTS[0]}_12h"] < 1.0
