"""The combine step of ``swift_amd.generate --maps`` on the CPU (``collect_maps``): every rank hands in ONE [steps, 4, nv, H, W]
fp64 array, the sum of the per-IC maps of its ICs in IC order (None when it has no IC); lead step by lead step rank 0 adds the
ranks' slabs in rank order, divides by n_ic and writes evaluation_maps.zarr (float32) and evaluation_regions.json (from the fp64
means).  One process against two gloo ranks on fake per-IC maps: the two results differ by the re-association of at most n_ic
fp64 terms per pixel, 1e-12 relative (the signed bias: of the sum of the absolute terms) is 10^3 times that; the float32 store
can differ by the one ulp a cast next to a rounding boundary gives."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np

import maps_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, N_IC, MEMBERS, INTERVAL, H, W = 2, 5, 6, 12, 6, 8
VARIABLES = ["2m_temperature", "geopotential_500", "geopotential_850", "mean_sea_level_pressure"]
NV = len(VARIABLES)
LAT, LON = np.linspace(-75.0, 75.0, H), np.arange(W) * (360.0 / W)
STORE, REGIONS = "evaluation_maps.zarr", "evaluation_regions.json"


def _rows():
    """Fake per-IC maps [n_ic, steps, 4, nv, H, W]: a signed bias, positive and uneven mse, crps and variance."""
    r = np.random.default_rng(29)
    m = r.lognormal(0.0, 2.0, (N_IC, STEPS, 4, NV, H, W))
    m[:, :, 0] *= r.choice([-1.0, 1.0], size=m[:, :, 0].shape)
    return m


WORKER = textwrap.dedent("""
    import sys
    import numpy as np, torch
    sys.path.insert(0, %(root)r)
    sys.path.insert(0, %(tests)r)
    from swift_amd import dist
    from swift_amd.generate import collect_maps
    import test_maps_collect_cpu as t
    dist.setup_torch(backend="gloo")
    rows = t._rows()
    mine = dist.shard_units(int(sys.argv[2]), dist.get_rank(), dist.get_world_size())
    local = None
    for ic in mine:                                                                  # IC order, as batch_metrics adds them
        local = torch.from_numpy(rows[ic]).clone() if local is None else local + torch.from_numpy(rows[ic])
    collect_maps(local, t.STEPS, int(sys.argv[2]), t.MEMBERS, t.VARIABLES, t.LAT, t.LON, t.INTERVAL, sys.argv[1])
    dist.barrier()
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()
""")


def _load(d):
    from swift_amd.utils import zarrlite
    store = {v: zarrlite.read_array(str(d / STORE), v) for v in zarrlite.list_arrays(str(d / STORE))}
    return store, zarrlite.read_attrs(str(d / STORE)), json.load(open(d / REGIONS))


def _run(tmp_path, n_ic):
    script = tmp_path / f"worker{n_ic}.py"
    script.write_text(WORKER % {"root": ROOT, "tests": os.path.join(ROOT, "tests")})
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    one, two = tmp_path / f"one{n_ic}", tmp_path / f"two{n_ic}"
    os.makedirs(one), os.makedirs(two)
    subprocess.run([sys.executable, str(script), str(one), str(n_ic)], check=True, env={**env, "WORLD_SIZE": "1", "RANK": "0"},
                   timeout=200)
    port = str(29600 + (os.getpid() + 131 + n_ic) % 300)
    procs = [subprocess.Popen([sys.executable, str(script), str(two), str(n_ic)],
                              env={**env, "WORLD_SIZE": "2", "RANK": str(r), "LOCAL_RANK": str(r), "MASTER_PORT": port})
             for r in range(2)]
    assert [p.wait(timeout=200) for p in procs] == [0, 0]
    assert sorted(os.listdir(one)) == sorted(os.listdir(two)) == sorted([REGIONS, STORE])
    return one, two


def _ulps_apart(a, b):
    """Distance of two float32 arrays in units in the last place (same sign, finite)."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def test_two_gloo_ranks_write_what_one_process_writes(tmp_path):
    from swift_amd.utils import zarrlite
    one, two = _run(tmp_path, N_IC)
    (a, attrs, ja), (b, attrs_b, jb) = _load(one), _load(two)
    rows = _rows()
    mean = rows.sum(0) / N_IC                                                               # [steps, 4, nv, H, W]
    # layout of the store
    assert sorted(a) == sorted(b) == sorted(["statistic", "prediction_timedelta", "level", "latitude", "longitude",
                                             "2m_temperature", "geopotential", "mean_sea_level_pressure"])
    assert attrs == attrs_b == {"statistics": ["bias", "mse", "crps", "variance"], "members": MEMBERS, "samples": N_IC}
    assert a["statistic"].dtype == np.int64 and a["statistic"].tolist() == [0, 1, 2, 3]
    assert a["prediction_timedelta"].dtype == np.int64
    assert a["prediction_timedelta"].tolist() == [(j + 1) * INTERVAL * 3_600_000_000_000 for j in range(STEPS)]   # no lead 0
    assert a["latitude"].dtype == a["longitude"].dtype == np.float32
    assert np.array_equal(a["latitude"], LAT.astype(np.float32)) and np.array_equal(a["longitude"], LON.astype(np.float32))
    assert a["level"].tolist() == [0, 1]
    root = str(one / STORE)
    assert zarrlite.array_info(root, "geopotential") == ((4, STEPS, 2, H, W), np.dtype(np.float32),
                                                         ["statistic", "prediction_timedelta", "level", "latitude", "longitude"])
    assert zarrlite.array_info(root, "2m_temperature") == ((4, STEPS, H, W), np.dtype(np.float32),
                                                           ["statistic", "prediction_timedelta", "latitude", "longitude"])
    meta = json.load(open(one / STORE / "geopotential" / ".zarray"))
    assert meta["chunks"] == [1, 1, 2, H, W] and meta["compressor"] is None
    assert sorted(f for f in os.listdir(one / STORE / "geopotential") if not f.startswith(".")) == \
        sorted(f"{s}.{j}.0.0.0" for s in range(4) for j in range(STEPS))                      # one chunk per (statistic, lead)
    assert json.load(open(one / STORE / "2m_temperature" / ".zarray"))["chunks"] == [1, 1, H, W]
    cons = json.load(open(one / STORE / ".zmetadata"))["metadata"]
    assert "geopotential/.zarray" in cons and ".zattrs" in cons and cons[".zattrs"] == attrs
    # values: against the fake rows (one process adds the ICs in order: the store is the fp32 cast of that very sum), ...
    seq = np.zeros_like(rows[0])
    for ic in range(N_IC):
        seq = rows[ic].copy() if ic == 0 else seq + rows[ic]
    want = (seq / N_IC).astype(np.float32).transpose(1, 0, 2, 3, 4)                           # [4, steps, nv, H, W]
    channels = zarrlite.variable_channels(VARIABLES)
    assert channels == {"2m_temperature": [0], "geopotential": [1, 2], "mean_sea_level_pressure": [3]}
    for var, ch in channels.items():
        w = want[:, :, ch] if var == "geopotential" else want[:, :, ch[0]]
        assert a[var].dtype == np.float32 and np.array_equal(a[var], w), var
        assert np.all(_ulps_apart(a[var], b[var]) <= 1), var                                  # ... and two ranks against one
    # the regions: against the reference reduction of the fp64 means, and two ranks against one
    ref, scale = mr.region_scores(mean, LAT, VARIABLES, INTERVAL), mr.region_abs(mean, LAT)
    assert sorted(ja) == sorted(jb) == sorted(ref) == ["global", "n_extratropics", "s_extratropics", "tropics"]
    for region in ref:
        assert sorted(ja[region]) == sorted(jb[region]) == sorted(ref[region]) and len(ref[region]) == 5 * NV * STEPS
        for key, val in ref[region].items():
            stat, rest = key.split("_", 1)
            i = [f"{v}_{(j + 1) * INTERVAL}h" for j in range(STEPS) for v in VARIABLES].index(rest)
            tol = 1e-12 * (scale[region][i // NV, 0, i % NV] if stat == "bias" else abs(val))
            assert abs(ja[region][key] - val) <= tol and abs(jb[region][key] - ja[region][key]) <= tol, (region, key)


def test_a_rank_without_ics_contributes_zeros(tmp_path):
    """One IC on two ranks: rank 1 holds none, hands in None and must neither hang the gather nor change the result."""
    one, two = _run(tmp_path, 1)
    (a, attrs, ja), (b, attrs_b, jb) = _load(one), _load(two)
    assert attrs == attrs_b and attrs["samples"] == 1
    for var in a:
        assert np.array_equal(a[var], b[var]), var
    assert ja == jb
    assert np.array_equal(a["mean_sea_level_pressure"], _rows()[0][:, :, 3].astype(np.float32).transpose(1, 0, 2, 3))
