"""The continuum add on config C3 (32 layers, 500-6000 cm^-1 at 0.001 cm^-1, 100 000 synthetic lines; bench.py's flagship),
DESIGN 4.22, with continuum.synthetic() (made-up coefficients: the time does not depend on their values).

    python tools/time_continuum.py [--reps 20] [--out profiles/continuum_time.txt]

runs the two measurements below one after the other, each in a child process of its own under `timeout` (a step that
faults or hangs ends the run: nothing further is started on the device).

  kernel   rtx_continuum_add alone (engine._continuum_call on host tables made once: the copy of the tables + the kernel),
           `reps` back-to-back calls between two device events, median of 5 rounds; achieved bytes/s against the
           2 x 32 x 5.5 M x 4 B = 1408 MB it must move (the block read once and written once; the node rows, 72 KB, come
           from cache), next to the expectation of 0.35 ms at the TUD kernel's recorded 4.05 TB/s. One and four components.
  step     engine.TudRunner.run with continuum=synthetic() (rtx_line_prep + rtx_voigt_sum + rtx_continuum_add + rtx_tud)
           against the runner without (rtx_compute_tud), the two alternating, each step between two device events, medians;
           the host time of Continuum.layer_tables on its own
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

XMIN, XMAX, DV, NL = 500.0, 6000.0, 0.001, 32
EXPECT_TBS, EXPECT_MS = 4.05, 0.35
STEPS = (("kernel", 600), ("step", 600))


def child(step, reps):
    import torch
    from radtxfr_amd import _lib, continuum, engine, synthetic
    lib = _lib.load()
    say = lambda s: print(s, flush=True)
    a = synthetic.c3_atmosphere(NL)
    grid = engine.Grid(XMIN, XMAX, int(np.ceil((XMAX - XMIN) / DV)))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    T = np.ascontiguousarray(a["Ts"], dtype=np.float64)
    one = continuum.synthetic()
    if step == "kernel":
        OD = torch.zeros((NL, grid.n), dtype=torch.float32, device="cuda")
        four = one + continuum.synthetic(molecule=2, foreign=False) + continuum.synthetic(molecule=2, dv=5.0, n=1401) + continuum.synthetic(molecule=1, v0=400.0)
        for name, cont in (("1 component (H2O self + foreign)", one), ("4 components", four)):
            tables, axes = cont.layer_tables(T, a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"])
            fn = lambda: engine._continuum_call(lib, tables, axes, grid, T, OD, engine._stream_ptr())
            ts = []
            for _ in range(6):  # the first round warms up
                OD.zero_()
                fn()
                torch.cuda.synchronize()
                ev[0].record()
                for _ in range(reps):
                    fn()
                ev[1].record()
                torch.cuda.synchronize()
                ts.append(ev[0].elapsed_time(ev[1]) / reps)
            t = float(np.median(ts[1:]))
            moved = 2 * 4.0 * NL * grid.n
            say("rtx_continuum_add, %s, %d layers x %d points, node tables %.0f KB" % (name, NL, grid.n, tables.nbytes / 1e3))
            say("  %.4f ms per call (min %.4f, max %.4f of 5 medians over %d calls)" % (t, min(ts[1:]), max(ts[1:]), reps))
            say("  reads + writes %.0f MB -> %.2f TB/s achieved; expected %.2f ms at %.2f TB/s (an estimate, not a gate): %.2f x"
                % (moved / 1e6, moved / t / 1e9, EXPECT_MS, EXPECT_TBS, t / EXPECT_MS))
        return
    tbl = synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)
    lines = engine.LineTable(tbl)
    runs = {"with continuum (prep + sum + add + tud)": engine.TudRunner(lines, grid, a["Zs"], n_layers=NL, continuum=one),
            "without (rtx_compute_tud)": engine.TudRunner(lines, grid, a["Zs"], n_layers=NL)}
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
    say("TudRunner.run on C3, device events around one step, %d steps each, alternating:" % reps)
    for k, v in ts.items():
        say("  %-42s median %.3f ms (min %.3f, max %.3f)" % (k, float(np.median(v)), min(v), max(v)))
    med = {k: float(np.median(v)) for k, v in ts.items()}
    say("  difference of the medians %.3f ms" % (med["with continuum (prep + sum + add + tud)"] - med["without (rtx_compute_tud)"]))
    th = []
    for _ in range(reps):
        t0 = time.perf_counter()
        one.layer_tables(T, a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"])
        th.append(1e3 * (time.perf_counter() - t0))
    say("  Continuum.layer_tables on the host (float64 rows of %d layers x %d nodes, inside the step above): median %.3f ms"
        % (NL, one.components[0].n, float(np.median(th))))
    d = (runs["with continuum (prep + sum + add + tud)"].OD - runs["without (rtx_compute_tud)"].OD).max().item()
    say("  max OD(with) - OD(without) = %.3g (made-up coefficients: a check that the add ran, not a physical figure)" % d)


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
    text = ["# python tools/time_continuum.py --reps %d" % args.reps,
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
