"""The combine step of ``swift_amd.generate --lead-windows`` on the CPU (``collect_windows``): every rank fills the [nw, nv, 4]
slots of its own ICs in an [n_ic, nw, nv, 4] fp64 array of zeros, one all-gather, rank 0 adds the ranks' arrays -- each slot is one
rank's rows plus zeros, so nothing is re-associated -- applies ``scores_from_sums`` per window and writes evaluation_windows.json.
One process against two gloo ranks on fake per-IC sums: the two files must be the same bytes."""
import json
import os
import subprocess
import sys
import textwrap
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_IC, MEMBERS, H, W = 5, 6, 8, 16
NAMES = ["6-168h", "174-336h", "12-12h"]
VARIABLES = ["2m_temperature", "geopotential_500"]


def _sums():
    """Fake per-IC rows [n_ic, nw, nv, 4]: positive and uneven; the pair-spread sum kept small enough for a positive crps."""
    s = np.random.default_rng(31).lognormal(0.0, 1.0, (N_IC, len(NAMES), len(VARIABLES), 4))
    s[..., 1] *= 50.0
    return s


WORKER = textwrap.dedent("""
    import sys, types
    import numpy as np, torch
    sys.path.insert(0, %(root)r)
    sys.path.insert(0, %(tests)r)
    from swift_amd import dist
    from swift_amd.generate import collect_windows
    import test_windows_collect_cpu as t
    dist.setup_torch(backend="gloo")
    sums = t._sums()
    mine = {ic: torch.from_numpy(sums[ic]) for ic in dist.shard_units(t.N_IC, dist.get_rank(), dist.get_world_size())}
    ds = types.SimpleNamespace(img_resolution=(t.H, t.W), variables=t.VARIABLES)
    collect_windows(mine, t.N_IC, t.NAMES, len(t.VARIABLES), t.MEMBERS, ds, "cpu", sys.argv[1])
    dist.barrier()
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()
""")


def test_two_gloo_ranks_write_what_one_process_writes(tmp_path):
    from swift_amd.eval.metrics import scores_from_sums
    script = tmp_path / "worker.py"
    script.write_text(WORKER % {"root": ROOT, "tests": os.path.join(ROOT, "tests")})
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    one, two = tmp_path / "one", tmp_path / "two"
    os.makedirs(one), os.makedirs(two)
    subprocess.run([sys.executable, str(script), str(one)], check=True, env={**env, "WORLD_SIZE": "1", "RANK": "0"}, timeout=200)
    port = str(29600 + (os.getpid() + 211) % 300)
    procs = [subprocess.Popen([sys.executable, str(script), str(two)],
                              env={**env, "WORLD_SIZE": "2", "RANK": str(r), "LOCAL_RANK": str(r), "MASTER_PORT": port})
             for r in range(2)]
    assert [p.wait(timeout=200) for p in procs] == [0, 0]
    assert os.listdir(one) == os.listdir(two) == ["evaluation_windows.json"]
    a, b = open(one / "evaluation_windows.json", "rb").read(), open(two / "evaluation_windows.json", "rb").read()
    assert a == b
    got = json.loads(a)
    assert sorted(got) == sorted(f"{m}_{v}_{n}" for m in ("rmse", "crps", "ssr") for v in VARIABLES for n in NAMES)
    sums = torch.from_numpy(_sums())
    for w, n in enumerate(NAMES):
        rmse, crps, ssr = scores_from_sums(sums[:, w], MEMBERS, H * W)
        for i, v in enumerate(VARIABLES):
            assert got[f"rmse_{v}_{n}"] == float(rmse[i]) and got[f"crps_{v}_{n}"] == float(crps[i]) and got[f"ssr_{v}_{n}"] == float(ssr[i])
    # the keys parse like those of evaluation_metrics.json
    from swift_amd.eval.metrics import structure
    st = structure(got)
    assert set(st) == {"rmse", "crps", "ssr"} and set(st["rmse"]) == {"6-168", "174-336", "12-12"}
    assert set(st["ssr"]["174-336"]) == set(VARIABLES)
