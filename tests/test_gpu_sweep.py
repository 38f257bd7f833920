"""-m gpu: the sampler sweep on the MI355X -- ``swiftk_sweep_sse`` against the numpy restatement of tests/sweep_reference.py
(which tests/test_sweep_cpu.py pins to the reference's own lines), its independence of batch size and slot, its refusals, and
``python -m swift_amd.eval.sampler`` end to end on a depth-2 Swift-B at 5.625 degrees with seeded weights.

Tolerance of the value checks: every term w_lat[h] * (double)q is reproduced exactly (same fp32 roundings, one fp64 product),
so kernel and restatement differ in the ORDER of an fp64 sum of n = H W non-negative terms only: each is within
n 2^-53 of the true sum relative, 3.6e-12 at n = 32768 -- written as 1e-11.  Nothing in it is measured."""
import argparse
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sweep_reference as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-11


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def _score(dev, x, y, t, mx, sx, st, w):
    from swift_amd import ops
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = ops.sweep_sse(d(x), d(y), d(t), d(mx), d(sx), d(st), d(w))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("zero", [True, False])
@pytest.mark.parametrize("shape,extra", [((3, 5, 8, 12), 2),      # general case
                                         ((2, 1, 5, 4), 3),       # 5 float4s for 8 slices: three slices are empty
                                         ((1, 2, 128, 256), 1)])  # full-size plane: 1024 float4s per slice, 4 per lane
def test_kernel_against_the_restatement(dev, shape, extra, zero):
    """x carries ``extra`` channels more than y (the forcings of the condition): another batch stride per shape."""
    x, y, t, mx, sx, st, w = sr.random_case(5, *shape, extra=extra)
    if zero:
        sx[0] = 0.0
    ref = sr.sweep_rows(x, y, t, mx, sx, st, w)
    got = _score(dev, x, y, t, mx, sx, st, w)
    assert got.shape == shape[:2] and got.dtype == np.float64
    print("max relative difference", np.max(np.abs(got - ref) / ref))
    assert np.all(np.abs(got - ref) <= RTOL * ref)


def test_kernel_bit_for_bit_on_exactly_summable_values(dev):
    """Small integers and power-of-two weights and scales: every term and every partial sum is an integer multiple of 1/4 far
    below 2^53, so any order of the additions gives the same bits."""
    B, C, H, W = 2, 3, 16, 24
    rng = np.random.default_rng(7)
    x = rng.integers(-8, 9, (B, C + 2, H, W)).astype(np.float32)
    y, t = (rng.integers(-6, 7, (B, C, H, W)).astype(np.float32) for _ in range(2))
    mx, sx, st = np.array([3, -5, 16], np.float32), np.array([2, 0, 0.5], np.float32), np.array([1, 2, 0.5], np.float32)
    w = np.array([0.5, 1.0, 2.0, 4.0] * (H // 4))
    d = (y.astype(np.int64) - t.astype(np.int64)) * st.reshape(1, C, 1, 1).astype(np.float64)   # xp cancels exactly
    exact = (w.reshape(1, 1, H, 1) * d * d).sum(axis=(2, 3))
    assert np.array_equal(sr.sweep_rows(x, y, t, mx, sx, st, w), exact)
    assert np.array_equal(_score(dev, x, y, t, mx, sx, st, w), exact)


@pytest.mark.parametrize("shape", [(3, 5, 8, 12), (3, 2, 128, 256)])
def test_rows_do_not_depend_on_batch_or_slot(dev, shape):
    x, y, t, mx, sx, st, w = sr.random_case(9, *shape)
    pick = lambda order: _score(dev, x[order], y[order], t[order], mx, sx, st, w)
    a, b, c = 0, 1, 2
    first = pick([a, b, c])
    for _ in range(2):  # twice: the same bits again
        runs = {(a, b, c): pick([a, b, c]), (c, a): pick([c, a]), (b,): pick([b]), (a,): pick([a]), (c,): pick([c])}
        for order, rows in runs.items():
            for slot, s in enumerate(order):
                assert np.array_equal(rows[slot], first[s]), (order, slot)


def test_kernel_does_not_contract_the_multiply_add(dev):
    """Where mx is of the size of x sx, ONE rounding of x sx + mx (a fused multiply-add) differs from the reference's two:
    constructed and asserted on the CPU, then the kernel must side with the two-rounding form."""
    x, y, t, mx, sx, st, w = sr.random_case(13, 2, 4, 8, 12)
    two, one = sr.sweep_rows(x, y, t, mx, sx, st, w), sr.sweep_rows(x, y, t, mx, sx, st, w, fused_x=True)
    s4, m4 = sx.reshape(1, 4, 1, 1), mx.reshape(1, 4, 1, 1)
    two_roundings = ((x[:, :4] * s4).astype(np.float32) + m4).astype(np.float32)
    one_rounding = (x[:, :4].astype(np.float64) * s4.astype(np.float64) + m4.astype(np.float64)).astype(np.float32)  # exact product
    assert np.any(two_roundings[:, 1] != one_rounding[:, 1])  # element level
    # channels 1 and 3 have means of the product's size: there the two forms' rows lie more than two tolerances apart, so a
    # row within one tolerance of the two-rounding form cannot also be within one of the contracted form
    assert np.all(np.abs(one[:, 1::2] - two[:, 1::2]) > 2 * RTOL * two[:, 1::2])
    got = _score(dev, x, y, t, mx, sx, st, w)
    print("contracted - two roundings, relative", np.abs(one - two) / two, "kernel - two roundings", np.abs(got - two) / two)
    assert np.all(np.abs(got - two) <= RTOL * two)
    assert np.all(np.abs(got[:, 1::2] - one[:, 1::2]) > RTOL * two[:, 1::2])


def test_refusals_come_before_any_launch(dev):
    """Host-side checks: nothing is launched, so nothing can fault (the bad pointers are never dereferenced)."""
    from swift_amd import _lib
    L = _lib.lib()
    B, C, H, W = 2, 3, 4, 8
    f = lambda *s: torch.zeros(*s, device=dev)
    x, y, t, v = f(B, C + 1, H, W + 4), f(B, C, H, W + 4), f(B, C, H, W + 4), f(3, C)
    w, out, scr = (torch.zeros(n, dtype=torch.float64, device=dev) for n in (H, B * C + 1, B * C * _lib.SWEEP_SLICES + 1))
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()

    def call(xp=x.data_ptr(), stride=(C + 1) * H * W, yp=y.data_ptr(), tp=t.data_ptr(), wp=w.data_ptr(), op=out.data_ptr(),
             sp=scr.data_ptr(), b=B, c=C, h=H, w_=W):
        return L.swiftk_sweep_sse(xp, stride, yp, tp, v[0].data_ptr(), v[1].data_ptr(), v[2].data_ptr(), wp, op, sp, b, c, h, w_, st)

    assert call() == 0
    assert call(w_=6) == -2                                                       # W % 4 != 0: SWIFTK_ESHAPE
    assert call(xp=x.data_ptr() + 4) == call(yp=y.data_ptr() + 8) == call(tp=t.data_ptr() + 4) == -3   # SWIFTK_EALIGN
    assert call(stride=(C + 1) * H * W + 2) == -3                                 # a stride that breaks the 16-byte rows
    assert call(op=out.data_ptr() + 4) == call(sp=scr.data_ptr() + 4) == call(wp=w.data_ptr() + 4) == -3
    assert call(xp=None) == call(yp=None) == call(tp=None) == call(wp=None) == call(op=None) == call(sp=None) == -1
    assert call(b=0) == call(c=-1) == call(h=0) == call(w_=0) == -1
    assert call(stride=C * H * W - 4) == -1                                       # x cannot hold C channels per sample
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- the CLI end to end
SWEEP = ["--num-steps", "2", "1", "--sigma-max", "80", "200", "--samples", "6", "--batch", "4"]


@pytest.fixture(scope="module")
def run_dir(dev, tmp_path_factory):
    """A run directory without training: the composed config of a depth-2 Swift-B at 5.625 degrees on synthetic fields, and a
    checkpoint whose "ema" weights are the seeded ones ``--synthetic`` initialises -- so both forms of the CLI see one net."""
    from swift_amd import generate
    from swift_amd.config import compose, instantiate, to_yaml
    rdir = tmp_path_factory.mktemp("sweep") / "run"
    os.makedirs(rdir / ".hydra")
    os.makedirs(rdir / "checkpoints")
    cfg = compose(os.path.join(ROOT, "swift_amd", "configs"), "train",
                  ["experiment=era5-swinv2-5.6-scm", "data=era5-synthetic-5.6", "data.dataset.length=24", "model.depth=2"])
    with open(rdir / ".hydra" / "config.yaml", "w") as f:
        f.write(to_yaml(cfg))
    dataset = instantiate(cfg.data.dataset, split="test", _convert_="object")
    args = argparse.Namespace(input=str(rdir), synthetic=True, checkpoint=None)
    net, name = generate.build_net(generate.load_cfg(args), dataset, args, dev)
    assert name == "synthetic"
    torch.save({"ema": {k: v.cpu() for k, v in net.state_dict().items()}}, rdir / "checkpoints" / "checkpoint-000001.pt")
    return rdir, dataset, net


def _cli(rdir, extra, env=None):
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    e.pop("WORLD_SIZE", None)
    e.update(env or {})
    p = subprocess.run([sys.executable, "-m", "swift_amd.eval.sampler", "--input", str(rdir)] + SWEEP + extra, env=e,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return p.stdout


@pytest.fixture(scope="module")
def one_rank_csv(run_dir):
    rdir = run_dir[0]
    out = _cli(rdir, ["--synthetic"])
    path = rdir / "output" / "synthetic" / "sampler_results.csv"
    assert f"Results saved to: {path}" in out and "Overall error:" in out
    return open(path, "rb").read()


def test_cli_rows_equal_a_recomputation(run_dir, one_rank_csv, dev):
    """4 rows (2 x 1 x 2 combinations); each equals sampler_factory on the same keyed noise (the module's own ``KeyedNoise``)
    scored by the numpy restatement: both sides see the same network output, so only the order of the fp64 sums differs."""
    from swift_amd.eval.sampler import KeyedNoise, lat_weights
    from swift_amd.generate import select_indices
    from swift_amd.generating.factory import sampler_factory
    rdir, ds, net = run_dir
    rows = list(csv.reader(one_rank_csv.decode().splitlines()))
    assert rows[0] == ["num_steps", "sigma_min", "sigma_max"] + [f"{v}_error" for v in ds.variables] + ["overall_error"]
    assert [r[:3] for r in rows[1:]] == [["2", "0.02", "80.0"], ["2", "0.02", "200.0"], ["1", "0.02", "80.0"], ["1", "0.02", "200.0"]]
    idx = select_indices(len(ds), 6, 1, 6)
    C, (H, W) = ds.n_target_channels, ds.img_resolution
    items = [ds[(j, 1, 6)][0] for j in idx]
    X, T = torch.stack([x for x, _ in items]).to(dev), torch.stack([t for _, t in items])
    mx, sx, st = (v.numpy() for v in ds.rollout_stats(6, "cpu"))
    w = lat_weights(ds)
    noise = KeyedNoise(0, dev).batch(idx)
    for i, r in enumerate(rows[1:]):
        sampler = sampler_factory("scm", net, denoise_dtype=torch.float32, num_steps=int(r[0]), sigma_min=float(r[1]),
                                  sigma_max=float(r[2]), auxiliary=0.6, randn_like=noise.randn_like)
        Y = sampler(X, latents=noise.start(i).latents((len(idx), C, H, W)))
        per_sample = sr.sweep_rows(X.cpu().numpy(), Y.cpu().numpy(), T.numpy(), mx, sx, st, w)
        sse = np.zeros(C)
        for row in per_sample:
            sse += row
        want = np.sqrt(sse / (len(idx) * H * W))
        got = np.array([float(v) for v in r[3:3 + C]])
        print("combination", i, "max relative difference", np.max(np.abs(got - want) / want))
        assert np.all(np.isfinite(got)) and np.all(got > 0)
        np.testing.assert_allclose(got, want, rtol=1e-10, atol=0)
        assert float(r[-1]) == pytest.approx(float(np.mean(want)), rel=1e-10)
    assert rows[1][3:] != rows[2][3:] and rows[3][3:] != rows[4][3:]


def test_cli_two_ranks_from_a_checkpoint_write_the_same_bytes(run_dir, one_rank_csv):
    """The run-directory form (latest checkpoint, "ema" weights) as two ranks sharing this GPU, collectives over gloo: shards of
    3 + 3 samples in batches of 2 against one rank's 4 + 2 -- the file is the same, byte for byte."""
    rdir = run_dir[0]
    _cli(rdir, ["--gpus", "2"], env={"SWIFTK_DIST_BACKEND": "gloo", "SWIFTK_ALLOW_SHARED_GPU": "1"})
    assert open(rdir / "output" / "latest" / "sampler_results.csv", "rb").read() == one_rank_csv


def test_no_field_leaves_the_device_during_a_sweep(run_dir, one_rank_csv, dev, tmp_path, monkeypatch):
    """Counted form: every Tensor.cpu / numpy / tolist / item on a DEVICE tensor during an in-process sweep is recorded; the
    largest is the per-batch row block (n_combos x B x C doubles), one per batch, and ``score_fn`` sees device tensors only.
    The one-rank group (SWIFTK_SINGLE_RANK_GROUP) is not set here, so no gather copy is among them."""
    from swift_amd.eval import sampler as sw
    rdir, ds, net = run_dir
    args = sw.parser.parse_args(["--input", str(rdir), "--synthetic"] + SWEEP)
    moved = []
    for name in ("cpu", "numpy", "tolist", "item"):
        orig = getattr(torch.Tensor, name)

        def spy(self, *a, _orig=orig, _name=name, **k):
            if self.is_cuda:
                moved.append((_name, self.numel()))
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, spy)

    def score(X, Y, T, mx, sx, st, w_lat, out):
        assert all(v.is_cuda for v in (X, Y, T, mx, sx, st, w_lat, out))
        sw.device_score(X, Y, T, mx, sx, st, w_lat, out)

    from swift_amd.generate import select_indices
    sw.sample_experiment(net, sw.Samples(ds, select_indices(len(ds), 6, 1, 6)), str(tmp_path), args, score_fn=score)
    monkeypatch.undo()
    C = ds.n_target_channels
    assert max(n for _, n in moved) == 4 * 4 * C, moved   # nothing larger than a row block: n_combos x B x C (a field is B C H W)
    assert [(name, n) for name, n in moved if n >= 4 * 2 * C] == [("cpu", 4 * 4 * C), ("cpu", 4 * 2 * C)], moved  # one per batch
    assert open(tmp_path / "sampler_results.csv", "rb").read() == one_rank_csv  # and the same file as the child process wrote
