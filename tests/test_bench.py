"""bench.py's own interface: a plain run prints the headline and nothing else, --steps sets the number of timed steps,
and --dump-outputs writes what the last timed step computed, at the wavenumbers bench.dump_indices() names."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cpu_ref as ref
from radtxfr_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
TOL_L, TOL_TAU = 1e-5, 2e-6


def test_bench_refuses_a_run_without_timed_steps():
    res = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "--steps" in res.stderr, res.stderr[-2000:]


@pytest.mark.gpu
def test_bench_plain_run_and_dump_outputs(tmp_path):
    """One plain run: the headline fields only, `steps` = --steps, value = points x steps / (steps x ms_per_step); the
    dumped tau / L-up / L-down are float32, within 64 MB, and equal the oracle on a 3000-point window of the grid."""
    import bench
    d = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    res = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)],
                         env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert out["higher_is_better"] is True and out["dtype"] == "f32" and out["unit"] == "wavenumber*layer points/s"
    pts = bench.N_WAVENUMBERS * bench.N_LAYERS
    assert abs(out["value"] * out["ms_per_step"] * 1e-3 / pts - 1.0) < 1e-9
    assert not {"roofline", "checksum", "cpu_baseline", "sharding"} & set(out), sorted(out)

    assert sorted(os.listdir(d)) == ["Ld.npy", "Lu.npy", "tau.npy"]
    assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64e6
    got = {k: np.load(d / f"{k}.npy") for k in ("tau", "Lu", "Ld")}
    idx = bench.dump_indices()
    assert idx.size == bench.DUMP_SAMPLES and np.all(np.diff(idx) > 0)
    for v in got.values():
        assert v.dtype == np.float32 and v.shape == idx.shape and np.isfinite(v).all()

    # the window test_full_c3_width_properties checks against the oracle, read through the dump's indices
    i0, n = 1234567, 3000
    full = synthetic.synth_line_table(synthetic.SEED_C3, bench.N_LINES, 475.0, 6025.0)
    a = synthetic.c3_atmosphere(bench.N_LAYERS)
    Xw = np.linspace(500.0, 6000.0, bench.N_WAVENUMBERS)[i0:i0 + n]
    sub = synthetic.subset_table(full, Xw[0] - 12.0, Xw[-1] + 12.0)
    ODr = np.stack([ref.layer_od(sub, Xw, a["Ts"][k], a["Ps"][k], a["PLs"][k], a["MFs_VAL"][k], a["MFs_ID"])
                    for k in range(bench.N_LAYERS)], 1)
    tr, ur, dr = ref.tud_from_od(Xw, ODr, a["Ts"], a["Zs"])
    sel = (idx >= i0) & (idx < i0 + n)
    j = idx[sel] - i0
    assert j.size > 1000
    assert np.max(np.abs(got["tau"][sel] - tr[j])) <= TOL_TAU
    for key, r in (("Lu", ur), ("Ld", dr)):  # relative error floored at 1e-3 of the window's largest value (conftest.rel_err)
        e = np.abs(got[key][sel] - r[j]) / np.maximum(np.abs(r[j]), 1e-3 * np.max(np.abs(r)))
        assert float(e.max()) <= TOL_L, (key, float(e.max()))
