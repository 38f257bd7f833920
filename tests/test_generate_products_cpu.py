"""The product loop of ``swift_amd.generate.rollout_and_save`` on the CPU: a recording product, handed in through ``products=``,
sees every initial condition once and in ascending order -- its members as the store holds them, the one contiguous copy of the
lead steps, the dataset's verifying fields -- whatever ``--batch`` and however many ranks share the job; and
``products_from_args`` names the products of a command line (which flags bring the metric sums, which need the truth)."""
import os
import subprocess
import sys
import textwrap
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMBERS, STEPS, N_IC, NV, H, W = 3, 2, 5, 3, 4, 8


def _dataset():
    from swift_amd.data.era5 import SyntheticERA5Dataset
    return SyntheticERA5Dataset(["t2m", "z_500", "z_850"], ["f0"], img_resolution=(H, W), length=40, seed=5)


class FakeEngine:   # stands in for RolloutEngine (as in tests/test_host_logic.py): a function of (X0, forcings, seed), CPU only
    interval = 6

    def __init__(self, ds):
        self.ds = ds

    def stage_forcings(self, ics, steps, device):
        return torch.stack([torch.stack([self.ds.get_forcings(j + i) for j in ics]) for i in range(steps)])

    def run(self, X0, forc, steps, seeds=None, **kw):
        out = [X0]
        for i in range(steps):
            z = torch.stack([torch.randn(X0.shape[1:], generator=torch.Generator().manual_seed(int(s) + i)) for s in seeds])
            out.append(0.9 * out[-1] + 0.1 * z + forc[i].mean(dim=1, keepdim=True))
        return torch.stack(out, 1)


class Recorder:
    needs_truth = True

    def __init__(self):
        self.calls, self.finished = [], 0

    def add_ic(self, ic, traj, pred, y):
        self.calls.append(dict(ic=ic, traj=traj.clone(), pred=pred.clone(), pred_contiguous=pred.is_contiguous(), y=y.clone()))

    def finish(self):
        self.finished += 1


def _run(ofile, batch):
    """One ``rollout_and_save`` job (``--dump numpy``) with a recording product -> (the recorder, the ICs' dataset indices)."""
    from swift_amd import dist
    from swift_amd.generate import create_empty_numpy, rollout_and_save, select_indices
    ds = _dataset()
    idx = select_indices(len(ds), N_IC, STEPS, 6)
    dist.run_on_rank0(create_empty_numpy, ofile, len(idx), NV, (H, W), MEMBERS, STEPS)
    rec = Recorder()
    out = rollout_and_save(FakeEngine(ds), ds, idx, MEMBERS, STEPS, ofile, torch.device("cpu"),
                           types.SimpleNamespace(dump="numpy", batch=batch), products=[rec])
    assert out is None and rec.finished == 1
    return rec, idx


def _same(a, b):
    return len(a) == len(b) and all(x["ic"] == y["ic"] and x["pred_contiguous"] == y["pred_contiguous"]
                                    and all(torch.equal(x[k], y[k]) for k in ("traj", "pred", "y")) for x, y in zip(a, b))


def test_every_ic_once_in_order_whatever_the_batch(tmp_path):
    ds, first = _dataset(), None
    for batch in (4, 7, 100):                      # one, two and all five ICs per device batch
        ofile = str(tmp_path / f"b{batch}.npy")
        rec, idx = _run(ofile, batch)
        store = np.load(ofile)                     # [samples, members, steps + 1, nv, H, W]
        assert store.shape == (N_IC, MEMBERS, STEPS + 1, NV, H, W) and np.abs(store).sum() > 0
        assert [c["ic"] for c in rec.calls] == list(range(N_IC))
        for c in rec.calls:
            assert tuple(c["traj"].shape) == (STEPS + 1, MEMBERS, NV, H, W)
            assert np.array_equal(c["traj"].numpy(), store[c["ic"]].transpose(1, 0, 2, 3, 4))    # its members, in member order
            assert c["pred_contiguous"] and torch.equal(c["pred"], c["traj"][1:])
            assert tuple(c["y"].shape) == (STEPS, NV, H, W)
            for i in range(STEPS):                 # physical fields, through the accessor the staging uses
                assert torch.equal(c["y"][i], ds.get_state(int(idx[c["ic"]]) + (i + 1) * FakeEngine.interval // 6))
        first = first or rec.calls
        assert _same(rec.calls, first), batch


WORKER = textwrap.dedent("""
    import sys, torch
    sys.path.insert(0, %(root)r)
    sys.path.insert(0, %(tests)r)
    from swift_amd import dist
    import test_generate_products_cpu as t
    dist.setup_torch(backend="gloo")
    rec, _ = t._run(sys.argv[1], 4)                # (asserts that finish() was called, once)
    assert [c["ic"] for c in rec.calls] == list(dist.shard_units(t.N_IC, dist.get_rank(), dist.get_world_size()))
    torch.save(rec.calls, sys.argv[1] + f".rank{dist.get_rank()}.pt")
    dist.barrier()
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()
""")


def test_two_gloo_ranks_see_their_shards_and_together_the_one_process_record(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER % {"root": ROOT, "tests": os.path.join(ROOT, "tests")})
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    out = str(tmp_path / "two.npy")
    port = str(29600 + (os.getpid() + 131) % 300)
    procs = [subprocess.Popen([sys.executable, str(script), out],
                              env={**env, "WORLD_SIZE": "2", "RANK": str(r), "LOCAL_RANK": str(r), "MASTER_PORT": port})
             for r in range(2)]
    assert [p.wait(timeout=200) for p in procs] == [0, 0]  # (each rank: exactly its dist.shard_units ICs, finish() called)
    two = [c for r in range(2) for c in torch.load(out + f".rank{r}.pt")]
    one, _ = _run(str(tmp_path / "one.npy"), 4)
    assert _same(two, one.calls)
    assert np.array_equal(np.load(out), np.load(tmp_path / "one.npy"))


def test_products_from_args_names_the_products_of_a_command_line():
    from swift_amd.generate import parser
    from swift_amd.generating.products import products_from_args
    ds = _dataset()

    def products(*flags):
        args = parser.parse_args(["--input", "run", "--members", str(MEMBERS), "--steps", str(STEPS), *flags])
        return products_from_args(args, ds, MEMBERS, STEPS, os.path.join("run", "output", "out.npy"), "cpu")

    names = lambda ps: [type(p).__name__ for p in ps]
    assert names(products()) == []
    assert names(products("--metrics")) == ["MetricSums"]
    for flag, name in (("--spectra", "Spectra"), ("--rank-hist", "RankHistogram"), ("--maps", "Maps")):
        assert names(products(flag)) == ["MetricSums", name], flag          # each of the three brings the metric sums with it
    alone = products("--summary")
    assert names(alone) == ["Summary"] and not any(p.needs_truth for p in alone)
    everything = products("--metrics", "--spectra", "--rank-hist", "--maps", "--summary")
    assert names(everything) == ["MetricSums", "Spectra", "RankHistogram", "Maps", "Summary"]
    assert [p.needs_truth for p in everything] == [True, True, True, True, False]
