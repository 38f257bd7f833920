"""Sampler sweep, host side (no GPU): the scoring restatement against the reference's literal lines, and
``swift_amd.eval.sampler.sample_experiment`` end to end on the tiny ERA5 tree of tests/era5_fixture.py with a CPU stand-in
network, sampler, noise draw and ``score_fn`` -- combination order, CSV surface, reported errors, sharding over 1 / 2 / 3
ranks, the EDM refusal."""
import argparse
import csv
import itertools
import os
import sys

import numpy as np
import pytest
import torch

import sweep_reference as sr


@pytest.mark.parametrize("shape", [(3, 5, 8, 12), (2, 1, 5, 4), (1, 2, 32, 64)])
def test_restatement_agrees_with_the_reference_lines(shape):
    """Rounding by rounding the restatement IS the reference's expression: summed over the batch its rows agree with
    ``np.sum(w_lat * (Y - T) ** 2, axis=(0, 2, 3))`` to 1e-12 relative -- only the order of the fp64 additions differs."""
    x, y, t, mx, sx, st, w = sr.random_case(11, *shape)
    sx[0] = 0.0  # a zeroed channel: x * 0 + m = m in the reference's arithmetic too
    rows = sr.sweep_rows(x, y, t, mx, sx, st, w)
    lit = sr.reference_lines(x[:, :shape[1]], y, t, mx, sx, st, w)
    assert rows.shape == shape[:2] and rows.dtype == np.float64 and lit.dtype == np.float64
    np.testing.assert_allclose(rows.sum(0), lit, rtol=1e-12, atol=0)
    # ... and the contracted form of x * sx + mx is a different number: the check can tell the two apart
    fused = sr.sweep_rows(x, y, t, mx, sx, st, w, fused_x=True)
    assert np.all(fused[:, 0] == rows[:, 0]) and (shape[1] == 1 or np.all(fused[:, 1] != rows[:, 1]))


# ---------------------------------------------------------------------------------------------- sample_experiment, CPU stand-ins
class StandInNet(torch.nn.Module):
    """A per-sample function of (x_t, t, condition, auxiliary): no batch statistics, so batching cannot change a sample."""
    sigma_data = 1.0

    def __init__(self, C):
        super().__init__()
        self.w = torch.nn.Parameter(torch.linspace(0.2, 0.6, C).view(1, C, 1, 1), requires_grad=False)
        self.C = C

    def forward(self, x, t, cond, aux):
        return self.w * x * torch.cos(t) + 0.1 * cond[:, :self.C] + 0.05 * cond[:, self.C:].mean(1, keepdim=True) + 0.01 * aux


def stand_in_factory(mode, net, denoise_dtype=torch.float32, *, num_steps, sigma_min, sigma_max, auxiliary, randn_like):
    """``sampler_factory("scm", ...)`` in plain torch (diffusion.py:417-461) over the stand-in net."""
    from swift_amd.generating.diffusion import scm_time_steps
    assert mode == "scm"
    ts = scm_time_steps(num_steps, sigma_min, sigma_max, net.sigma_data)

    def sampler(X, generator=None, *, latents):
        x = latents
        for i in range(len(ts) - 1):
            if i > 0:
                x = torch.sin(ts[i]) * randn_like(x) + torch.cos(ts[i]) * x
            x = torch.cos(ts[i]) * x - torch.sin(ts[i]) * net(x, ts[i], X, auxiliary)
        return x
    return sampler


def stand_in_draw(out, seeds, step):
    """A pure function of (seed, step) per sample, like ``ops.unit_noise``."""
    for b, s in enumerate(seeds.tolist()):
        g = torch.Generator().manual_seed((int(s) * 1_000_003 + int(step) * 7919) % (1 << 62))
        out[b] = torch.randn(out[b].shape, generator=g)
    return out


def numpy_score(X, Y, T, mx, sx, st, w_lat, out):
    assert all(isinstance(v, torch.Tensor) for v in (X, Y, T, mx, sx, st, w_lat, out)) and w_lat.dtype == torch.float64
    out.copy_(torch.from_numpy(sr.sweep_rows(*(v.numpy() for v in (X, Y, T, mx, sx, st, w_lat)))))


ARGS = dict(num_steps=[4, 2, 1], sigma_min=[0.02], sigma_max=[80.0, 200.0], batch=4, seed=3, interval=12, dtype="f32")


@pytest.fixture()
def tiny(tmp_path, monkeypatch):
    import era5_fixture as fx
    monkeypatch.setitem(sys.modules, "h5py", fx.install_fake_h5py())
    from swift_amd.data.era5 import ERA5Dataset
    from swift_amd.eval.sampler import Samples
    from swift_amd.generate import select_indices
    ds = ERA5Dataset(fx.write_tree(str(tmp_path / "era5")), list(fx.VARS), list(fx.FORC), intervals=[6, 12, 24], split="train",
                     residual=True)
    idx = select_indices(len(ds), 7, 1, 12)  # 7 samples: 4 + 3 over two ranks, 3 + 2 + 2 over three
    assert len(set(idx)) == 7
    return Samples(ds, idx), StandInNet(len(fx.VARS)), tmp_path


def _run(samples, net, odir, world=1, **over):
    """The job as ``world`` ranks, one after the other in this process: ranks 1.. hand their blocks to rank 0's gather."""
    from swift_amd.eval.sampler import sample_experiment
    args = argparse.Namespace(**dict(ARGS, **over))
    os.makedirs(odir, exist_ok=True)
    blocks = {}
    kw = dict(score_fn=numpy_score, factory=stand_in_factory, draw_fn=stand_in_draw, world=world)
    for r in range(world - 1, -1, -1):  # rank 0 last: its gather returns every rank's block
        def gather(local, r=r):
            blocks[r] = local.clone()
            return [blocks[q] for q in range(world)] if r == 0 else None
        res = sample_experiment(net, samples, str(odir), args, rank=r, gather_fn=gather, **kw)
        assert (res is None) == (r != 0)
    return res, open(os.path.join(str(odir), "sampler_results.csv"), "rb").read()


def test_combos_csv_and_errors(tiny):
    from swift_amd.eval.sampler import KeyedNoise, combos, lat_weights, parser
    samples, net, tmp = tiny
    ds, idx = samples
    # the reference's flags and defaults (sampler.py:24-56)
    d = parser.parse_args(["--input", "RUN"])
    assert (d.checkpoint, d.seed, d.batch, d.num_steps, d.sigma_min, d.sigma_max) == (None, 0, 60, [32, 16, 8, 4, 2, 1], [0.02], [200.0])
    assert (d.dtype, d.gpus, d.samples, d.interval, d.synthetic) == ("f32", None, -1, 6, False)
    args = argparse.Namespace(**ARGS)
    params = combos(args)
    assert params == list(itertools.product([4, 2, 1], [0.02], [80.0, 200.0])) and params[1] == (4, 0.02, 200.0)

    errors, raw = _run(samples, net, tmp / "out")
    rows = list(csv.reader(raw.decode().splitlines()))
    assert rows[0] == ["num_steps", "sigma_min", "sigma_max"] + [f"{v}_error" for v in ds.variables] + ["overall_error"]
    assert len(rows) == 1 + len(params)  # every combination, the 1-step ones that ignore sigma included
    assert [(int(r[0]), float(r[1]), float(r[2])) for r in rows[1:]] == params and rows[1][:3] == ["4", "0.02", "80.0"]

    # a direct computation: one sample at a time, the reference's literal lines, rows added in sample order
    C, (H, W) = ds.n_target_channels, ds.img_resolution
    mx, sx, st = (v.numpy() for v in ds.rollout_stats(12, "cpu"))
    w = lat_weights(ds)
    noise = KeyedNoise(ARGS["seed"], torch.device("cpu"), stand_in_draw)
    for i, (num_steps, smin, smax) in enumerate(params):
        sampler = stand_in_factory("scm", net, num_steps=num_steps, sigma_min=smin, sigma_max=smax, auxiliary=1.2,
                                   randn_like=noise.randn_like)
        sse = np.zeros(C)
        for j in idx:
            (x, t), _ = ds[(j, 1, 12)]
            y = sampler(x[None], latents=noise.batch([j]).start(i).latents((1, C, H, W)))
            sse += sr.reference_lines(x[None, :C].numpy(), y.numpy(), t[None].numpy(), mx, sx, st, w)
        want = np.sqrt(sse / (len(idx) * H * W))
        got = np.array([float(v) for v in rows[1 + i][3:3 + C]])
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
        np.testing.assert_array_equal(got, errors[i])  # the CSV carries the doubles in round-trip form
        assert float(rows[1 + i][-1]) == float(np.mean(errors[i]))
    assert rows[1][3:] != rows[2][3:]  # 4 steps at sigma_max 80 / 200: two time grids
    assert rows[5][3:] != rows[6][3:]  # the 1-step grid ignores sigma, but the draws are keyed by the combination index


def test_sharding_and_batching_leave_the_csv_unchanged(tiny):
    samples, net, tmp = tiny
    _, one = _run(samples, net, tmp / "w1")
    for world in (2, 3):
        _, raw = _run(samples, net, tmp / f"w{world}", world=world)
        assert raw == one
    for batch in (1, 3, 60):
        _, raw = _run(samples, net, tmp / f"b{batch}", batch=batch)
        assert raw == one


def test_edm_net_is_refused(tiny):
    from swift_amd.eval.sampler import Samples, sample_experiment
    from swift_amd.models.precond import EDMPrecond
    samples, _, tmp = tiny
    mcfg = dict(_target_="swift.models.swinv2.SwinV2", window_size=[16, 16], shift_size=[8, 8], patch_size=[2, 2], depth=1,
                dim=96, heads=4)
    net = EDMPrecond(mcfg, [32, 32], 2, 3, auxiliary_dim=1)
    with pytest.raises(ValueError, match="this net is an EDMPrecond: use 'edm'"):
        sample_experiment(net, samples, str(tmp), argparse.Namespace(**ARGS), score_fn=numpy_score, draw_fn=stand_in_draw)
    assert not os.path.exists(tmp / "sampler_results.csv")
