"""The combine step of ``swift_amd.generate --rank-hist`` on the CPU (``collect_rank_histogram``): every rank hands in ONE
[steps, nv, members + 1] fp64 array, the sum of the per-IC rows of its ICs in IC order; rank 0 adds the ranks' arrays in rank
order, divides by n_ic * norm and writes evaluation_rank_histogram.npz.  One process against two gloo ranks on fake per-IC rows:
the two files differ by the reordering of at most n_ic positive fp64 terms per entry -- 1e-12 relative is 10^3 times that."""
import os
import subprocess
import sys
import textwrap

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, NV, N_IC, MEMBERS, INTERVAL, NORM = 3, 4, 5, 6, 12, 8192.0
VARIABLES = ["2m_temperature", "geopotential_500", "u_component_of_wind_850", "mean_sea_level_pressure"]


def _rows():
    """Fake per-IC histograms [n_ic, steps, nv, members + 1]: positive, uneven, every row summing to NORM."""
    r = np.random.default_rng(23).lognormal(0.0, 2.0, (N_IC, STEPS, NV, MEMBERS + 1))
    return r / r.sum(-1, keepdims=True) * NORM


WORKER = textwrap.dedent("""
    import sys
    import numpy as np, torch
    sys.path.insert(0, %(root)r)
    sys.path.insert(0, %(tests)r)
    from swift_amd import dist
    from swift_amd.generate import collect_rank_histogram
    import test_rank_hist_collect_cpu as t
    dist.setup_torch(backend="gloo")
    rows = t._rows()
    mine = dist.shard_units(t.N_IC, dist.get_rank(), dist.get_world_size())
    local = torch.zeros(t.STEPS, t.NV, t.MEMBERS + 1, dtype=torch.float64)
    for ic in mine:                                                                  # IC order, as batch_metrics adds them
        local = local + torch.from_numpy(rows[ic])
    collect_rank_histogram(local, t.N_IC, t.MEMBERS, t.VARIABLES, t.INTERVAL, t.NORM, sys.argv[1])
    dist.barrier()
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()
""")


def test_two_gloo_ranks_write_what_one_process_writes(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER % {"root": ROOT, "tests": os.path.join(ROOT, "tests")})
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    one, two = tmp_path / "one", tmp_path / "two"
    os.makedirs(one), os.makedirs(two)
    subprocess.run([sys.executable, str(script), str(one)], check=True, env={**env, "WORLD_SIZE": "1", "RANK": "0"}, timeout=200)
    port = str(29600 + (os.getpid() + 97) % 300)
    procs = [subprocess.Popen([sys.executable, str(script), str(two)],
                              env={**env, "WORLD_SIZE": "2", "RANK": str(r), "LOCAL_RANK": str(r), "MASTER_PORT": port})
             for r in range(2)]
    assert [p.wait(timeout=200) for p in procs] == [0, 0]
    assert os.listdir(one) == os.listdir(two) == ["evaluation_rank_histogram.npz"]
    with np.load(one / "evaluation_rank_histogram.npz", allow_pickle=False) as f:
        a = {k: f[k] for k in f.files}
    with np.load(two / "evaluation_rank_histogram.npz", allow_pickle=False) as f:
        b = {k: f[k] for k in f.files}
    # layout
    assert sorted(a) == sorted(b) == sorted(["rank", "lead_hours", "variables", "frequency", "members", "samples"])
    assert a["rank"].dtype == np.int64 and a["rank"].tolist() == list(range(MEMBERS + 1))
    assert a["lead_hours"].tolist() == [12, 24, 36]
    assert a["variables"].dtype.kind == "U" and a["variables"].tolist() == VARIABLES
    assert a["members"].shape == a["samples"].shape == () and a["members"].dtype == a["samples"].dtype == np.int64
    assert int(a["members"]) == MEMBERS and int(a["samples"]) == N_IC
    assert a["frequency"].shape == (STEPS, NV, MEMBERS + 1) and a["frequency"].dtype == np.float64
    # values: against the rows themselves (each row of the file sums to 1), and two ranks against one
    np.testing.assert_allclose(a["frequency"], _rows().sum(0) / (N_IC * NORM), rtol=1e-12, atol=0)
    np.testing.assert_allclose(a["frequency"].sum(-1), 1.0, rtol=1e-12, atol=0)
    for k in a:
        if a[k].dtype.kind == "f":
            np.testing.assert_allclose(b[k], a[k], rtol=1e-12, atol=0)
        else:
            assert np.array_equal(a[k], b[k])
