"""Cross-section look-up against the line-sum on config C3 (32 layers, 500-6000 cm^-1 at 0.001 cm^-1, 100 000 synthetic
lines; bench.py's flagship), DESIGN 4.11.

    python tools/time_xs_lut.py [--reps 20] [--out profiles/xs_lut_time.txt]

runs the four measurements below one after the other, each in a child process of its own under `timeout` (a step that
faults or hangs ends the run: nothing further is started on the device). A child builds its own table: H2O and CO2 of the
line list on T = 220, 245, 270, 295 K x p = 0.25, 0.45, 0.75, 1.05 atm (the rectangle that holds the C3 atmosphere), with
afit_xs.cross_section_grid.

  kernel   rtx_xs_od alone (engine.xs_od into a preallocated block: the 2 KB copy of the terms + the kernel), `reps`
           back-to-back calls between two device events, median of 5; achieved bytes/s against the 32 x 5.5 M x 4 B =
           704 MB it must write (reads are extra: each node row once from HBM at least, 704 MB for this table)
  step     engine.TudRunner.run through the table (rtx_xs_od + rtx_tud) against the line-by-line runner (rtx_compute_tud:
           prologue + line-sum + TUD), the two alternating, each step between two events, medians; then rt.compute_TUD
           end to end (host clock, results on the host) for both
  step10x  the same pair with the line list replicated to ten times the lines (each copy shifted by a fraction of a
           line spacing, strengths / 10)
  build    cross_section_grid + XsLut.from_grids wall time and the table's device footprint
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T_NODES = np.array([220.0, 245.0, 270.0, 295.0])
P_NODES = np.array([0.25, 0.45, 0.75, 1.05])
XMIN, XMAX, DV, NL = 500.0, 6000.0, 0.001, 32
STEPS = (("build", 600), ("kernel", 600), ("step", 600), ("step10x", 900))


def line_list(times):
    from radtxfr_amd import synthetic
    tbl = synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)
    if times == 1:
        return tbl
    out = {k: np.concatenate([v] * times) for k, v in tbl.items()}
    out["nu"] = np.concatenate([tbl["nu"] + 0.0055 * j for j in range(times)])  # mean line spacing 0.055 cm^-1
    out["sw"] = out["sw"] / times
    order = np.argsort(out["nu"], kind="stable")
    return {k: v[order] for k, v in out.items()}


def build_table(tbl, report=None):
    import torch
    from radtxfr_amd import afit_xs, hapi
    from radtxfr_amd import radiative_transfer as rt
    X = rt.make_spectral_axis(XMIN, XMAX, DV)
    entries = []
    t0 = time.perf_counter()
    for m in (1, 2):
        sel = tbl["molec_id"] == m
        name = "time_xs_lut_m%d" % m
        hapi.LOCAL_TABLE_CACHE[name] = {"header": {"number_of_rows": int(sel.sum())}, "data": {k: v[sel] for k, v in tbl.items()}}
        entries.append(dict(ID=m, T=T_NODES, P_atm=P_NODES, X=X, xs=afit_xs.cross_section_grid(name, T_NODES, P_NODES, X)))
    t1 = time.perf_counter()
    lut = afit_xs.XsLut.from_grids(entries)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    if report is not None:
        report("table: %d molecules x %d x %d nodes x %d points, %d lines" % (len(entries), T_NODES.size, P_NODES.size, X.size, tbl["nu"].size))
        report("  cross_section_grid (line-sums of %d states + copy to the host)  %.2f s" % (2 * T_NODES.size * P_NODES.size, t1 - t0))
        report("  XsLut.from_grids (scale, round to fp32, upload)                  %.2f s" % (t2 - t1))
        report("  device footprint                                                %.1f MB (fp32 rows), host arrays %.1f MB (float64)"
               % (lut.nbytes / 1e6, sum(e["xs"].nbytes for e in entries) / 1e6))
    return lut


def child(step, reps):
    import torch
    from radtxfr_amd import _lib, engine, synthetic
    from radtxfr_amd import radiative_transfer as rt
    _lib.load()
    say = lambda s: print(s, flush=True)
    a = synthetic.c3_atmosphere(NL)
    assert T_NODES[0] <= a["Ts"].min() and a["Ts"].max() <= T_NODES[-1]
    assert P_NODES[0] <= a["Ps"].min() / 101325.0 and a["Ps"].max() / 101325.0 <= P_NODES[-1]
    tbl = line_list(10 if step == "step10x" else 1)
    lut = build_table(tbl, say if step in ("build", "step10x") else None)
    if step == "build":
        return
    grid = engine.Grid(XMIN, XMAX, int(np.ceil((XMAX - XMIN) / DV)))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    if step == "kernel":
        OD = torch.empty((NL, grid.n), dtype=torch.float32, device="cuda")
        fn = lambda: engine.xs_od(lut, grid, a["Ts"], a["Ps"] / 101325.0, a["PLs"], a["MFs_VAL"], a["MFs_ID"], out_f32=OD)
        ts = []
        for _ in range(6):  # the first round warms up
            fn()
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(reps):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]) / reps)
        t = float(np.median(ts[1:]))
        wr = 4.0 * NL * grid.n
        rows, w = lut.layer_terms(a["Ts"], a["Ps"] / 101325.0, a["PLs"], a["MFs_VAL"], a["MFs_ID"])
        n_rows = np.unique(rows[w != 0]).size
        terms = int((w != 0).sum())
        say("rtx_xs_od, %d layers x %d points, %d non-zero terms on %d distinct node rows" % (NL, grid.n, terms, n_rows))
        say("  %.4f ms per call (min %.4f, max %.4f of 5 medians over %d calls)" % (t, min(ts[1:]), max(ts[1:]), reps))
        say("  writes %.0f MB -> %.2f TB/s of written bytes; with each node row read once from HBM (%.0f MB) %.2f TB/s; "
            "row reads issued (cache or HBM) %.1f GB -> %.2f TB/s"
            % (wr / 1e6, wr / t / 1e9, 4.0 * n_rows * grid.n / 1e6, (wr + 4.0 * n_rows * grid.n) / t / 1e9, 4.0 * terms * grid.n / 1e9,
               4.0 * terms * grid.n / t / 1e9))
        return
    lines = engine.LineTable(tbl)
    runs = {"table (rtx_xs_od + rtx_tud)": engine.TudRunner(None, grid, a["Zs"], n_layers=NL, xs_lut=lut),
            "lines (rtx_compute_tud)": engine.TudRunner(lines, grid, a["Zs"], n_layers=NL)}
    ts = {k: [] for k in runs}
    for it in range(reps + 3):
        for k, run in runs.items():  # alternating
            torch.cuda.synchronize()
            ev[0].record()
            run.run(a["Ts"], a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"])
            ev[1].record()
            torch.cuda.synchronize()
            if it >= 3:
                ts[k].append(ev[0].elapsed_time(ev[1]))
    say("TudRunner.run, %d lines, device events around one step, %d steps each, alternating:" % (tbl["nu"].size, reps))
    for k, v in ts.items():
        say("  %-28s median %.3f ms (min %.3f, max %.3f)" % (k, float(np.median(v)), min(v), max(v)))
    tau = {k: r.tau.clone() for k, r in runs.items()}
    d = (tau["table (rtx_xs_od + rtx_tud)"] - tau["lines (rtx_compute_tud)"]).abs().max().item()
    say("  max |tau(table) - tau(lines)| = %.3g (interpolation between nodes %g K / factor %.2f in p apart, not rounding)"
        % (d, T_NODES[1] - T_NODES[0], P_NODES[1] / P_NODES[0]))
    kw = {"table": dict(xs_lut=lut), "lines": dict(line_table=lines)}
    te = {k: [] for k in kw}
    for it in range(reps // 2 + 2):
        for k, extra in kw.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rt.compute_TUD(XMIN, XMAX, DVOUT=DV, Altitudes=np.asarray([500]), **extra, **a)
            if it >= 2:
                te[k].append(1e3 * (time.perf_counter() - t0))
    say("rt.compute_TUD end to end (host clock; float64 results on the host, 132 MB over PCIe), %d calls each:" % (reps // 2))
    for k, v in te.items():
        say("  %-28s median %.2f ms (min %.2f, max %.2f)" % (k, float(np.median(v)), min(v), max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=[s for s, _ in STEPS])
    args = ap.parse_args()
    if args.step:
        child(args.step, args.reps)
        return
    import torch
    text = ["# python tools/time_xs_lut.py --reps %d" % args.reps,
            "# device: %s, torch %s" % (torch.cuda.get_device_name(0) if torch.cuda.is_available() else "none", torch.__version__)]
    print("\n".join(text), flush=True)
    for step, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--reps",
                            str(args.reps)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        block = "\n[%s]\n%s" % (step, r.stdout.rstrip())
        print(block, flush=True)
        text.append(block)
        if r.returncode != 0:
            text.append("step %s ended with status %d: stopping" % (step, r.returncode))
            print(text[-1], flush=True)
            break
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(text) + "\n")
    sys.exit(0 if r.returncode == 0 else 1)


if __name__ == "__main__":
    main()
