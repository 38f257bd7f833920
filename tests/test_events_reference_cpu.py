"""The reference of tests/events_reference.py on the CPU, the host side of ``generate --events`` (``parse_events``,
``brier_scores``, the product list) and the refusals of ``swiftk_event_table`` (which come before any launch, so they need no
GPU).

Bound of the score checks: every score is a sum of at most 65 terms of magnitude at most 1, each a few ulps of fp64 off, so the
error is about 2e-14; 1e-12 absolute is 50 times that."""
import argparse
import warnings

import numpy as np
import pytest

import events_reference as er

TOL = 1e-12


def _case(N=5, seed=3, kind="random"):
    shape, ev_var, ev_dir = (2, N, 3, 6, 17), [2, 0, 2], [0, 1, 1]
    pred, y, thr = er.make(kind, shape, len(ev_var), seed=seed)
    return pred, y, thr, ev_var, ev_dir, er.lat_weights(er.lat_of(shape[3]))


def test_reference_cells_equal_a_per_pixel_loop():
    pred, y, thr, ev_var, ev_dir, w = _case(N=3, kind="masked")
    n, N, V, H, W = pred.shape
    want = np.zeros((n, len(ev_var), N + 1, 2))
    cnt = np.zeros((n, len(ev_var), H, N + 1, 2), dtype=np.int64)
    for i in range(n):
        for e, (v, d) in enumerate(zip(ev_var, ev_dir)):
            for h in range(H):
                for x in range(W):
                    t = thr[e, h, x]
                    if t != t:
                        continue
                    ev = (lambda a: bool(a < t)) if d else (lambda a: bool(a > t))
                    k = sum(ev(pred[i, m, v, h, x]) for m in range(N))
                    cnt[i, e, h, k, int(ev(y[i, v, h, x]))] += 1
            for h in range(H):                                   # the documented order, scalar by scalar
                want[i, e] = want[i, e] + w[h] * cnt[i, e, h].astype(np.float64)
    assert np.array_equal(er.counts(pred, y, thr, ev_var, ev_dir), cnt)
    got = er.reference(pred, y, thr, ev_var, ev_dir, w)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    assert np.isnan(thr).any() and cnt.sum() == n * (~np.isnan(thr)).sum()


@pytest.mark.parametrize("N", (1, 2, 5, 12, 64))
def test_brier_scores_of_the_table_agree_with_the_definition(N):
    from swift_amd.eval.metrics import BRIER_SCORES, brier_scores
    for kind in ("random", "masked", "t280"):
        pred, y, thr, ev_var, ev_dir, w = _case(N=N, kind=kind)
        T = er.reference(pred, y, thr, ev_var, ev_dir, w)
        s = brier_scores(T, N)
        assert sorted(s) == sorted(BRIER_SCORES) and all(v.shape == T.shape[:2] and v.dtype == np.float64 for v in s.values())
        direct = er.brier_direct(pred, y, thr, ev_var, ev_dir, w)
        print(f"{kind} N={N}: worst |brier - direct| {np.max(np.abs(s['brier'] - direct)):.3g}, worst decomposition residual "
              f"{np.max(np.abs(s['brier'] - (s['reliability'] - s['resolution'] + s['uncertainty']))):.3g}")
        assert np.all(np.abs(s["brier"] - direct) <= TOL)
        assert np.all(np.abs(s["brier"] - (s["reliability"] - s["resolution"] + s["uncertainty"])) <= TOL)
        assert np.all(np.abs(s["uncertainty"] - s["base_rate"] * (1 - s["base_rate"])) <= TOL)
        k, o, valid = er._events(pred, y, thr, ev_var, ev_dir)
        wt = w[None, None, :, None] * valid[None]
        assert np.all(np.abs(s["base_rate"] - (wt * o).sum((-2, -1)) / np.broadcast_to(wt, o.shape).sum((-2, -1))) <= TOL)
        ok = s["uncertainty"] > 0
        assert np.all(np.abs(s["bss"][ok] - (1 - s["brier"][ok] / s["uncertainty"][ok])) <= TOL) and np.all(np.isnan(s["bss"][~ok]))
        if N == 1:
            assert np.all(np.isnan(s["fair_brier"]))
        else:   # Ferro: the mean over pixels of k (N - k) / (N^2 (N - 1)) comes off
            corr = (wt * (k * (N - k) / (N * N * (N - 1.0)))).sum((-2, -1)) / np.broadcast_to(wt, k.shape).sum((-2, -1))
            assert np.all(np.abs(s["fair_brier"] - (direct - corr)) <= TOL)


def test_fair_brier_of_a_two_member_table_by_hand():
    """N = 2, cells (k, o): n = (4, 4, 2), o = (1, 2, 2) -> S = 10, base rate 1/2;
    brier = [3 * 0 + 1 * 1 + 2 * 1/4 + 2 * 1/4 + 0 + 2 * 0] / 10 = 0.2; Ferro's term: n_1 * 1 * 1 / (4 * 1) / 10 = 0.1."""
    from swift_amd.eval.metrics import brier_scores
    T = np.array([[3.0, 1.0], [2.0, 2.0], [0.0, 2.0]])[None]
    s = brier_scores(T, 2)
    assert s["brier"].shape == (1,)
    assert abs(s["brier"][0] - 0.2) <= TOL and abs(s["fair_brier"][0] - 0.1) <= TOL and abs(s["base_rate"][0] - 0.5) <= TOL
    assert abs(s["uncertainty"][0] - 0.25) <= TOL and abs(s["bss"][0] - 0.2) <= TOL
    # reliability: [4 (0 - 1/4)^2 + 4 (1/2 - 1/2)^2 + 2 (1 - 1)^2] / 10 = 0.025; resolution: [4 / 16 + 0 + 2 / 4] / 10 = 0.075
    assert abs(s["reliability"][0] - 0.025) <= TOL and abs(s["resolution"][0] - 0.075) <= TOL
    assert abs(brier_scores(7.0 * T, 2)["fair_brier"][0] - 0.1) <= TOL   # the scores do not depend on the table's scale
    with pytest.raises(ValueError, match="brier_scores"):
        brier_scores(T, 3)


def test_an_all_nan_threshold_gives_a_zero_table_and_nan_scores_without_a_warning():
    from swift_amd.eval.metrics import brier_scores
    pred, y, thr, ev_var, ev_dir, w = _case(N=4)
    thr[1] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        T = er.reference(pred, y, thr, ev_var, ev_dir, w)
        s = brier_scores(T, 4)
        d = er.brier_direct(pred, y, thr, ev_var, ev_dir, w)
    assert np.all(T[:, 1] == 0.0) and np.all(T[:, 0].sum((-2, -1)) > 0)
    for name, v in s.items():
        assert np.all(np.isnan(v[:, 1])), name
        assert np.all(np.isfinite(v[:, [0, 2]])), name
    assert np.all(np.isnan(d[:, 1]))


VARS = ["2m_temperature", "10m_wind", "geopotential_500"]


def test_parse_events_reads_specs_and_file(tmp_path):
    from swift_amd.eval.metrics import parse_events
    field = np.arange(12, dtype=np.float64).reshape(3, 4)
    field[1, 2] = np.nan
    f = tmp_path / "ev.npz"
    np.savez(f, **{"geopotential_500:gt:p90": field, "10m_wind:lt:calm": np.float32(1.5)})
    names, ev_var, ev_dir, thr = parse_events(["2m_temperature:lt:273.15", "10m_wind:gt:17"], str(f), VARS, 3, 4)
    assert names == ["2m_temperature:lt:273.15", "10m_wind:gt:17", "geopotential_500:gt:p90", "10m_wind:lt:calm"]
    assert ev_var.dtype == ev_dir.dtype == np.int32 and ev_var.tolist() == [0, 1, 2, 1] and ev_dir.tolist() == [1, 0, 0, 1]
    assert thr.dtype == np.float32 and thr.shape == (4, 3, 4) and thr.flags.c_contiguous
    assert np.all(thr[0] == np.float32(273.15)) and np.all(thr[1] == 17.0) and np.all(thr[3] == 1.5)
    assert np.array_equal(thr[2], field.astype(np.float32), equal_nan=True) and np.isnan(thr[2]).sum() == 1
    only = parse_events(None, str(f), VARS, 3, 4)
    assert only[0] == names[2:] and np.array_equal(only[3], thr[2:], equal_nan=True)
    early = parse_events(["10m_wind:gt:17"], str(f), VARS)          # before the grid is known: no thresholds yet
    assert early[0] == names[1:] and early[3] is None


def test_parse_events_refuses_on_the_host(tmp_path):
    from swift_amd.eval.metrics import parse_events

    def npz(**kw):
        p = tmp_path / f"f{len(list(tmp_path.iterdir()))}.npz"
        np.savez(p, **kw)
        return str(p)

    with pytest.raises(ValueError, match="bogus"):
        parse_events(["bogus:gt:1"], None, VARS, 3, 4)                                       # unknown variable
    with pytest.raises(ValueError, match="'ge'"):
        parse_events(["10m_wind:ge:1"], None, VARS, 3, 4)                                    # bad operator
    for bad in ("10m_wind:gt:nan", "10m_wind:gt:inf", "10m_wind:lt:-inf", "10m_wind:gt:fast", "10m_wind:gt", "10m_wind"):
        with pytest.raises(ValueError, match="events"):
            parse_events([bad], None, VARS, 3, 4)                                            # non-finite / unreadable / short
    with pytest.raises(ValueError, match="finite"):
        parse_events(None, npz(**{"10m_wind:gt:x": np.float64("nan")}), VARS, 3, 4)          # a NaN scalar masks everything
    for shape in ((4, 3), (3,), (1, 3, 4), (3, 5)):
        with pytest.raises(ValueError, match="shape"):
            parse_events(None, npz(**{"10m_wind:gt:x": np.zeros(shape)}), VARS, 3, 4)        # wrong field shape
    with pytest.raises(ValueError, match="shape"):
        parse_events(None, npz(**{"10m_wind:gt:x": np.zeros(3)}), VARS)                      # not 2-d, even without a grid
    with pytest.raises(ValueError, match="twice"):
        parse_events(["10m_wind:gt:17", "10m_wind:gt:17"], None, VARS, 3, 4)                 # duplicate name
    with pytest.raises(ValueError, match="twice"):
        parse_events(["10m_wind:gt:17"], npz(**{"10m_wind:gt:17": np.float64(3.0)}), VARS, 3, 4)
    with pytest.raises(ValueError, match="no events"):
        parse_events(None, None, VARS, 3, 4)
    with pytest.raises(ValueError, match="no events"):
        parse_events([], npz(), VARS, 3, 4)
    with pytest.raises(ValueError, match="bogus"):
        parse_events(None, npz(**{"bogus:lt:x": np.zeros((3, 4))}), VARS, 3, 4)
    with pytest.raises(ValueError):                                                          # an object array needs a pickle
        p = tmp_path / "pickled.npz"
        np.savez(p, **{"10m_wind:gt:x": np.array([{"a": 1}], dtype=object)})
        parse_events(None, str(p), VARS, 3, 4)


def test_check_events_args_refuses_on_the_host(tmp_path):
    from swift_amd import generate
    a = generate.parser.parse_args(["--input", str(tmp_path), "--synthetic", "--events", "2m_temperature:lt:273.15"])
    assert a.events == ["2m_temperature:lt:273.15"] and a.events_file is None
    plain = generate.parser.parse_args(["--input", "x"])
    assert plain.events is None and plain.events_file is None
    generate.check_events_args(plain)                                                         # without the flags: nothing to check
    with pytest.raises(ValueError, match="--events"):
        generate.check_events_args(a)                                                         # --members 1
    a.members = 65
    with pytest.raises(ValueError, match="--events"):
        generate.check_events_args(a)
    a.members = 2
    generate.check_events_args(a)                                                             # the synthetic run has the variable
    a.events = ["bogus:gt:1"]
    with pytest.raises(ValueError, match="bogus"):
        generate.check_events_args(a)
    with pytest.raises(ValueError, match="bogus"):
        generate.main(a)                                                                      # before anything is loaded
    f = tmp_path / "ev.npz"
    np.savez(f, **{"2m_temperature:gt:field": np.zeros((3, 4))})                              # the synthetic grid is 128 x 256
    b = argparse.Namespace(input=str(tmp_path), synthetic=True, members=4, events=None, events_file=str(f))
    with pytest.raises(ValueError, match="shape"):
        generate.check_events_args(b)


def test_the_c_entry_refuses_bad_arguments_without_a_gpu():
    """Every refusal comes before the launch: no pointer here is ever dereferenced."""
    from swift_amd import _lib
    L = _lib.lib()

    def call(pred=64, y=64, thr=64, ev_var=64, ev_dir=64, w_lat=64, out=64, n=2, N=3, V=2, H=3, W=8, E=2):
        return L.swiftk_event_table(pred, y, thr, ev_var, ev_dir, w_lat, out, n, N, V, H, W, E, None)

    for name in ("pred", "y", "thr", "ev_var", "ev_dir", "w_lat", "out"):
        assert call(**{name: None}) == -1, name                                               # SWIFTK_EINVAL
    for name in ("n", "N", "V", "H", "W", "E"):
        assert call(**{name: 0}) == call(**{name: -2}) == -1, name
    assert call(N=65) == -2                                                                   # SWIFTK_ESHAPE
    assert call(n=1 << 20, E=1 << 11) == -2                                                   # n E beyond 2^31 - 1
    for name in ("pred", "y", "thr", "ev_var", "ev_dir"):
        assert call(**{name: 66}) == call(**{name: 65}) == -3, name                           # SWIFTK_EALIGN
    for name in ("w_lat", "out"):
        assert call(**{name: 68}) == call(**{name: 66}) == -3, name
    assert call(N=0, pred=66) == -1 and call(N=65, out=68) == -2                              # in the order of the contract


def test_event_table_refuses_what_the_kernel_cannot_take_without_a_gpu():
    import torch
    from swift_amd.eval.metrics import event_table, event_tables_to_device
    pred, y, thr = (torch.from_numpy(a) for a in er.make("random", (1, 3, 2, 3, 8), 2, seed=9))
    for bad in ((pred, y), (pred.double(), y), (pred[0], y), (pred.numpy(), y)):               # CPU tensors, dtype, rank, type
        with pytest.raises(ValueError, match="event_table"):
            event_table(*bad, er.lat_of(3), [0, 1], [0, 1], thr.numpy())
    for ev_var in ([0, 2], [-1, 0], [0], [[0, 1]], [0.0, 1.0]):                                # outside V, wrong length, rank, type
        with pytest.raises(ValueError, match="event_table"):
            event_tables_to_device(ev_var, [0, 1], thr.numpy(), 2, "cpu")
    v, d, t = event_tables_to_device([1, 0], [0, 5], thr.numpy(), 2, "cpu")
    assert v.dtype == d.dtype == torch.int32 and v.tolist() == [1, 0] and d.tolist() == [0, 1] and t.dtype == torch.float32


def test_the_products_of_a_command_line_with_events():
    from swift_amd.generate import parser
    from swift_amd.generating.products import product_types
    names = lambda *flags: [c.__name__ for c in product_types(parser.parse_args(["--input", "run", *flags]))]
    assert names("--events", "2m_temperature:lt:273.15") == ["MetricSums", "Events"]
    assert names("--events-file", "f.npz") == ["MetricSums", "Events"]
    assert names("--metrics", "--spectra", "--rank-hist", "--maps", "--summary", "--events", "a:gt:1", "--events-file", "f.npz") == \
        ["MetricSums", "Spectra", "RankHistogram", "Maps", "Events", "Summary"]
    assert names("--metrics", "--spectra", "--rank-hist", "--maps", "--summary") == \
        ["MetricSums", "Spectra", "RankHistogram", "Maps", "Summary"]
    assert names() == [] and names("--summary") == ["Summary"]


def test_the_events_product_parses_on_the_host_and_waits_with_the_device(tmp_path):
    """``products_from_args`` with a CPU device (as tests/test_generate_products_cpu.py calls it) builds the product: nothing
    touches a device before the first IC."""
    from swift_amd.data.era5 import SyntheticERA5Dataset
    from swift_amd.generate import parser
    from swift_amd.generating.products import products_from_args
    ds = SyntheticERA5Dataset(VARS, ["f0"], img_resolution=(4, 8), length=40, seed=5)
    f = tmp_path / "ev.npz"
    np.savez(f, **{"geopotential_500:gt:p90": np.ones((4, 8))})
    args = parser.parse_args(["--input", "run", "--members", "3", "--steps", "2", "--events", "10m_wind:gt:17", "--events-file", str(f)])
    ps = products_from_args(args, ds, 3, 2, str(tmp_path / "out.npy"), "cpu")
    assert [type(p).__name__ for p in ps] == ["MetricSums", "Events"] and all(p.needs_truth for p in ps)
    ev = ps[1]
    assert ev.names == ["10m_wind:gt:17", "geopotential_500:gt:p90"] and ev.ev_var.tolist() == [1, 2] and ev.tables is None
    assert ev.thr.shape == (2, 4, 8)
    args.events = ["bogus:gt:1"]
    with pytest.raises(ValueError, match="bogus"):
        products_from_args(args, ds, 3, 2, str(tmp_path / "out.npy"), "cpu")
