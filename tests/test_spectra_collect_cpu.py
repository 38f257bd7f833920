"""The combine step of ``swift_amd.generate --spectra`` on the CPU (``collect_spectra``): every rank hands in ONE
[steps, nv, 3, K] fp64 array, the sum of the per-IC rows of its ICs in IC order; rank 0 adds the ranks' arrays in rank order,
divides and writes evaluation_spectra.npz.  One process against two gloo ranks on fake per-IC rows: the two files differ by the
reordering of at most n_ic * members positive fp64 terms per entry -- 1e-12 relative is 10^3 times that."""
import os
import subprocess
import sys
import textwrap

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, NV, K, N_IC, MEMBERS, INTERVAL = 3, 4, 7, 5, 3, 12
VARIABLES = ["2m_temperature", "geopotential_500", "u_component_of_wind_850", "mean_sea_level_pressure"]

WORKER = textwrap.dedent("""
    import sys
    import numpy as np, torch
    sys.path.insert(0, %(root)r)
    from swift_amd import dist
    from swift_amd.generate import collect_spectra
    dist.setup_torch(backend="gloo")
    steps, nv, K, n_ic, members, interval = %(shape)r
    rows = np.random.default_rng(17).lognormal(0.0, 3.0, (n_ic, steps, nv, 3, K))   # positive, eight orders of magnitude apart
    mine = dist.shard_units(n_ic, dist.get_rank(), dist.get_world_size())
    local = torch.zeros(steps, nv, 3, K, dtype=torch.float64)
    for ic in mine:                                                                  # IC order, as batch_metrics adds them
        local = local + torch.from_numpy(rows[ic])
    collect_spectra(local, n_ic, members, %(variables)r, interval, sys.argv[1])
    dist.barrier()
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()
""")


def test_two_gloo_ranks_write_what_one_process_writes(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER % {"root": ROOT, "shape": (STEPS, NV, K, N_IC, MEMBERS, INTERVAL), "variables": VARIABLES})
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    one, two = tmp_path / "one", tmp_path / "two"
    os.makedirs(one), os.makedirs(two)
    subprocess.run([sys.executable, str(script), str(one)], check=True, env={**env, "WORLD_SIZE": "1", "RANK": "0"}, timeout=200)
    port = str(29600 + (os.getpid() + 11) % 300)
    procs = [subprocess.Popen([sys.executable, str(script), str(two)],
                              env={**env, "WORLD_SIZE": "2", "RANK": str(r), "LOCAL_RANK": str(r), "MASTER_PORT": port})
             for r in range(2)]
    assert [p.wait(timeout=200) for p in procs] == [0, 0]
    assert os.listdir(one) == os.listdir(two) == ["evaluation_spectra.npz"]
    with np.load(one / "evaluation_spectra.npz", allow_pickle=False) as f:
        a = {k: f[k] for k in f.files}
    with np.load(two / "evaluation_spectra.npz", allow_pickle=False) as f:
        b = {k: f[k] for k in f.files}
    # layout
    assert sorted(a) == sorted(b) == sorted(["wavenumber", "lead_hours", "variables", "member", "ensemble_mean", "truth", "members",
                                             "samples"])
    assert a["wavenumber"].tolist() == list(range(K)) and a["lead_hours"].tolist() == [12, 24, 36]
    assert a["variables"].dtype.kind == "U" and a["variables"].tolist() == VARIABLES
    assert a["members"].shape == a["samples"].shape == () and int(a["members"]) == MEMBERS and int(a["samples"]) == N_IC
    for k in ("member", "ensemble_mean", "truth"):
        assert a[k].shape == (STEPS, NV, K) and a[k].dtype == np.float64
    # values: against the rows themselves, and two ranks against one
    rows = np.random.default_rng(17).lognormal(0.0, 3.0, (N_IC, STEPS, NV, 3, K))
    np.testing.assert_allclose(a["member"], rows[:, :, :, 0].sum(0) / (N_IC * MEMBERS), rtol=1e-12, atol=0)
    np.testing.assert_allclose(a["ensemble_mean"], rows[:, :, :, 1].sum(0) / N_IC, rtol=1e-12, atol=0)
    np.testing.assert_allclose(a["truth"], rows[:, :, :, 2].sum(0) / N_IC, rtol=1e-12, atol=0)
    for k in a:
        if a[k].dtype.kind == "f":
            np.testing.assert_allclose(b[k], a[k], rtol=1e-12, atol=0)
        else:
            assert np.array_equal(a[k], b[k])
