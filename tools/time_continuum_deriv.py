"""The continuum's derivative kernel on config C3 (32 layers, 500-6000 cm^-1 at 0.001 cm^-1; bench.py's flagship), DESIGN
4.23, with continuum.synthetic() (made-up coefficients: the time does not depend on their values).

    python tools/time_continuum_deriv.py [--reps 20] [--out profiles/continuum_deriv_time.txt]

runs the measurement in a child process under `timeout` (a step that faults or hangs ends the run: nothing further is
started on the device).

  rtx_continuum_add_d alone (the copy of the three node tables + the kernel, host tables made once), one component: dOD/dT
  only, one species only, and both; and rtx_continuum_add on the same layers in the same process. The four alternate: each
  round times `reps` back-to-back calls of one of them between two device events, then the next; medians over 5 rounds
  after a warm-up round. Achieved bytes/s against what each must move: every destination block read once and written once
  (2 x 32 x 5.5 M x 4 B = 1408 MB per block; the node rows come from cache). Estimated from the code alone, before any
  measurement: both blocks at the add's recorded 4.2 TB/s, 0.67 ms.
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

XMIN, XMAX, DV, NL = 500.0, 6000.0, 0.001, 32
EXPECT_TBS = 4.2
LIMIT_S = 600


def child(reps):
    import ctypes as C
    import torch
    from radtxfr_amd import _lib, continuum, engine, synthetic
    lib = _lib.load()
    say = lambda s: print(s, flush=True)
    a = synthetic.c3_atmosphere(NL)
    grid = engine.Grid(XMIN, XMAX, int(np.ceil((XMAX - XMIN) / DV)))
    T = np.ascontiguousarray(a["Ts"], dtype=np.float64)
    cont = continuum.synthetic()
    A, A_T, A_x, axes = cont.layer_tables_d(T, a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"])
    tables, _ = cont.layer_tables(T, a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"])
    OD = torch.zeros((NL, grid.n), dtype=torch.float32, device="cuda")
    dOD = torch.zeros_like(OD)
    Kb = torch.zeros((1, NL, grid.n), dtype=torch.float32, device="cuda")
    vp = C.c_void_p
    h = lambda x: x.ctypes.data_as(vp)
    v0, dv = np.array([axes[0][0]]), np.array([axes[0][1]])
    nn, slot, none = np.array([axes[0][2]], dtype=np.int32), np.array([0], dtype=np.int32), np.array([-1], dtype=np.int32)

    def deriv(with_T, with_K):
        def fn():
            _lib.check(lib.rtx_continuum_add_d(grid.byref(), NL, h(T), 1, h(v0), h(dv), h(nn), h(A), h(A_T), h(A_x), A.shape[2],
                                               h(slot if with_K else none), 1, vp(dOD.data_ptr()) if with_T else None,
                                               vp(Kb.data_ptr()) if with_K else None, grid.n, engine._stream_ptr(), 0))
        return fn
    runs = [("rtx_continuum_add_d, dOD/dT only", deriv(True, False), 1), ("rtx_continuum_add_d, one species only", deriv(False, True), 1),
            ("rtx_continuum_add_d, dOD/dT and one species", deriv(True, True), 2),
            ("rtx_continuum_add", lambda: engine._continuum_call(lib, tables, axes, grid, T, OD, engine._stream_ptr()), 1)]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts = {name: [] for name, _, _ in runs}
    seen = {}
    for _ in range(6):  # the first round warms up; the four alternate within a round
        for name, fn, _ in runs:
            for t in (OD, dOD, Kb):
                t.zero_()
            fn()
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(reps):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            ts[name].append(ev[0].elapsed_time(ev[1]) / reps)
            seen[name] = (dOD.abs().max().item(), Kb.max().item())  # the blocks are zeroed before every round of every run
    say("one component (H2O self + foreign), %d layers x %d points, node tables %.0f KB each; %d calls per round, alternating"
        % (NL, grid.n, A.nbytes / 1e3, reps))
    for name, _, blocks in runs:
        t = float(np.median(ts[name][1:]))
        moved = blocks * 2 * 4.0 * NL * grid.n
        say("%s\n  %.4f ms per call (min %.4f, max %.4f of 5 rounds); reads + writes %.0f MB -> %.2f TB/s achieved"
            % (name, t, min(ts[name][1:]), max(ts[name][1:]), moved / 1e6, moved / t / 1e9))
    both, add = (float(np.median(ts[n][1:])) for n in (runs[2][0], runs[3][0]))
    say("dOD/dT and one species against the add of the same run: %.2f x; against the estimate of %.2f ms (both blocks at %.1f TB/s, "
        "made from the code alone, not a gate): %.2f x" % (both / add, 2 * 2 * 4.0 * NL * grid.n / EXPECT_TBS / 1e9, EXPECT_TBS,
                                                           both / (2 * 2 * 4.0 * NL * grid.n / EXPECT_TBS / 1e9)))
    say("after %d calls of the run with both: max |dOD/dT| = %.3g, max dOD/dMF = %.3g (made-up coefficients: a check that the "
        "kernel ran, not a physical figure)" % ((reps + 1,) + seen[runs[2][0]]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args.reps)
        return
    import torch
    text = ["# python tools/time_continuum_deriv.py --reps %d" % args.reps,
            "# device: %s, torch %s" % (torch.cuda.get_device_name(0) if torch.cuda.is_available() else "none", torch.__version__)]
    print("\n".join(text), flush=True)
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    text.append("\n" + r.stdout.rstrip())
    print(text[-1], flush=True)
    if r.returncode != 0:
        text.append("the measurement ended with status %d" % r.returncode)
        print(text[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(text) + "\n")
    sys.exit(0 if r.returncode == 0 else 1)


if __name__ == "__main__":
    main()
