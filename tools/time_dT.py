"""Time the analytic dOD/dT line-sum (rtx_line_prep_dt + rtx_voigt_sum_dt) against the route it replaces, at
the reference caller's configuration (690-1410 cm^-1 at 0.0005: 1.44 M points, the 66-layer standard atmosphere, T + 3
species: DESIGN 4.9).

  step "sums": (a) the central-difference route: two rtx_line_prep_window + rtx_voigt_sum (engine.voigt_sum_window at T -+ 0.5 K)
               (b) rtx_line_prep_dt + rtx_voigt_sum_dt (engine.voigt_sum_dT)
  step "vjp":  (c) engine.tud_vjp end to end (a cotangent on L-up, 1 vector) with dT_method "fd" and "analytic"

Within a step the routes are interleaved; HIP events after a warm-up; medians of --reps runs. Each step is a child
process under its own time limit (this process never opens the GPU); a step that fails ends the tool.

    python tools/time_dT.py [--reps 5] [--out profiles/dT_sum_time.txt]
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"sums": 240, "vjp": 420}  # seconds per step
ALTS = np.concatenate((np.array([200, 500, 1000, 2000, 5000, 10000, 20000, 50000]) * 0.3048 / 1e3, [100.0]))


def run_step(step, reps):
    import torch
    from radtxfr_amd import engine, synthetic
    from radtxfr_amd import radiative_transfer as rt

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    full = synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)
    sub = synthetic.subset_table(full, 690.0 - 12.0, 1410.0 + 12.0)
    sa = rt.StdAtmos
    a = dict(Zs=sa[:, 1], Ts=sa[:, 5].copy(), Ps=sa[:, 4], PLs=sa[:, 3], MFs_VAL=sa[:, 6:9] * 1e6, MFs_ID=np.array([1, 2, 3]))
    tbl = rt._resolve_table(sub)
    X = rt._cached_axis(690.0, 1410.0, 0.0005)
    grid = engine.Grid(690.0, 1410.0, X.size)
    nL = a["Ts"].size
    T = a["Ts"]
    print("%d points, %d layers, %d lines; device: %s" % (grid.n, nL, tbl.n, torch.cuda.get_device_name(0)), flush=True)
    if step == "sums":
        o1 = torch.empty((nL, grid.n), dtype=torch.float32, device="cuda")
        o2 = torch.empty_like(o1)

        def fd_route():
            for sgn, out in ((1.0, o1), (-1.0, o2)):
                Ts = T + sgn * 0.5
                w, p_atm = engine.layer_weights_od(tbl.species, Ts, a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"])
                engine.voigt_sum_window(tbl, grid, Ts, T, p_atm, w, out)

        def analytic_route():
            w, p_atm = engine.layer_weights_od(tbl.species, T, a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"])
            engine.voigt_sum_dT(tbl, grid, T, p_atm, w, o1)

        routes = [("(a) 2 x (rtx_line_prep_window + rtx_voigt_sum)", fd_route),
                  ("(b) rtx_line_prep_dt + rtx_voigt_sum_dt", analytic_route)]
    else:
        gen = torch.Generator(device="cuda").manual_seed(1)
        G = torch.randn((1, ALTS.size, grid.n), generator=gen, device="cuda", dtype=torch.float32)
        args = (tbl, grid, a["Zs"], T, a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"])
        kw = dict(G_Lu=G, Altitudes=ALTS, theta_r=0.0, N_angle=30, returnOD=True, wrt=("T", 1, 2, 3))
        routes = [("(c) engine.tud_vjp, L-up, 1 vector, dT_method=\"fd\"", lambda: engine.tud_vjp(*args, dT_method="fd", **kw)),
                  ("(c) engine.tud_vjp, L-up, 1 vector, dT_method=\"analytic\"", lambda: engine.tud_vjp(*args, dT_method="analytic", **kw))]
    for _, fn in routes:  # warm-up: allocations, scratch, the zero rows of the *_dod entry points
        fn()
    torch.cuda.synchronize()
    ts = {name: [] for name, _ in routes}
    for _ in range(reps):  # interleaved
        for name, fn in routes:
            ts[name].append(timed(fn))
    print("medians over %d interleaved runs [ms] (runs):" % reps)
    for name, _ in routes:
        print("  %-62s %8.2f   (%s)" % (name, np.median(ts[name]), ", ".join("%.2f" % t for t in ts[name])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=sorted(LIMITS), default=None, help="run one step in this process (used by the tool itself)")
    args = ap.parse_args()
    if args.step:
        run_step(args.step, args.reps)
        return 0
    lines = []
    rc = 0
    for step in ("sums", "vjp"):
        cmd = ["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
        print(r.stdout, end="", flush=True)
        lines.append("step %s:" % step)
        lines += ["  " + s for s in r.stdout.splitlines()]
        if r.returncode != 0:
            lines.append("step %s ended with status %d: stopping" % (step, r.returncode))
            print(lines[-1], flush=True)
            rc = r.returncode
            break
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
