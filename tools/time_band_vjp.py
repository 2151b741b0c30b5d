"""Time the sensor stage's adjoint (rtx_srf_radiance_vjp, sensor.band_radiance_srf_vjp) at the reference caller's size
(690-1410 cm^-1 at 0.0005, the 66-layer standard atmosphere, Sensor.mako's bands, emissivity knots 1 cm^-1 apart, one
surface temperature, nE = 1 and 2000) next to the forward pass it mirrors (rtx_srf_moments + rtx_band_mix: both read the
same three spectra), and the whole rt.compute_band_radiance_vjp next to rt.compute_TUD_vjp with a ready cotangent.
HIP events, medians, the routes interleaved.

    python tools/time_band_vjp.py [--reps 5] [--out profiles/band_vjp_time.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from radtxfr_amd import _lib, engine, sensor, synthetic  # noqa: E402
from radtxfr_amd import radiative_transfer as rt  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.load()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    lo, hi, dv, Ts_s = 690.0, 1410.0, 0.0005, 300.0
    full = synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)
    sub = synthetic.subset_table(full, lo - 12.0, hi + 12.0)
    sa = rt.StdAtmos
    a = dict(Zs=sa[:, 1], Ts=sa[:, 5].copy(), Ps=sa[:, 4], PLs=sa[:, 3], MFs_VAL=sa[:, 6:9] * 1e6, MFs_ID=np.array([1, 2, 3]))
    wrt = ("T", 1, 2, 3)
    kw = dict(DVOUT=dv, line_table=sub, Altitudes=np.array([8.0]), **a)
    X = rt._cached_axis(lo, hi, dv)
    grid = engine.Grid(lo, hi, X.size)
    s = sensor.Sensor.mako(X[0], X[-1])
    Xk = np.arange(lo, hi + 0.5, 1.0)
    nB, nk = len(s), Xk.size
    say("caller configuration: %d points, %d layers, 1 altitude, %d MAKO bands, %d emissivity knots, 1 surface temperature, wrt %s"
        % (grid.n, a["Ts"].size, nB, nk, wrt))
    say("device: %s" % torch.cuda.get_device_name(0))
    _, tau, La, Ld = rt.compute_TUD(lo, hi, **kw)
    t_d, a_d, d_d = (torch.as_tensor(np.asarray(v, dtype=np.float32).ravel(), device="cuda") for v in (tau, La, Ld))
    rng = np.random.default_rng(1)
    for nE in (1, 2000):
        E = rng.uniform(0.6, 1.0, (nk, nE)).astype(np.float32)
        g = rng.normal(size=(nB, nE)).astype(np.float32)
        E_d, g_d = torch.as_tensor(E, device="cuda"), torch.as_tensor(g, device="cuda")
        rows = sensor.band_radiance_srf_vjp(grid, t_d, a_d, d_d, Xk, E_d, Ts_s, s, g_d)
        cot = {"tau": rows["G_tau"], "La": rows["G_La"], "Ld": rows["G_Ld"]}
        routes = [
            ("forward: rtx_srf_moments + rtx_band_mix", lambda: sensor.band_radiance_srf_fused(grid, t_d, a_d, d_d, Xk, E_d, Ts_s, s)),
            ("sensor adjoint, all five outputs", lambda: sensor.band_radiance_srf_vjp(grid, t_d, a_d, d_d, Xk, E_d, Ts_s, s, g_d)),
            ("sensor adjoint, the three rows and dTs (no dE)",
             lambda: sensor.band_radiance_srf_vjp(grid, t_d, a_d, d_d, Xk, E_d, Ts_s, s, g_d, outputs=("G_tau", "G_La", "G_Ld", "Ts"))),
            ("sensor adjoint, dE alone", lambda: sensor.band_radiance_srf_vjp(grid, t_d, a_d, d_d, Xk, E_d, Ts_s, s, g_d, outputs=("emis",))),
            ("rt.compute_band_radiance_vjp, whole call", lambda: rt.compute_band_radiance_vjp(lo, hi, s, Xk, E_d, Ts_s, g, wrt=wrt, **kw)),
            ("rt.compute_TUD_vjp with a ready cotangent", lambda: rt.compute_TUD_vjp(lo, hi, cot, wrt=wrt, **kw)),
        ]
        for _, fn in routes:  # warm-up: workspaces, allocator, table caches
            fn()
        torch.cuda.synchronize()
        ts = {name: [] for name, _ in routes}
        for _ in range(args.reps):  # interleaved
            for name, fn in routes:
                ts[name].append(timed(fn)[0])
        say("nE = %d: medians over %d interleaved runs [ms] (runs):" % (nE, args.reps))
        for name, _ in routes:
            say("  %-50s %9.3f   (%s)" % (name, np.median(ts[name]), ", ".join("%.3f" % t for t in ts[name])))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
