"""Cost of per-layer diluent mixes in the prologue, and of a compute_TUD step with broadening="self", on config C3
(100 000-line table, 500-6000 cm^-1 at 0.001 cm^-1, 32 layers).

    python tools/time_broadening.py [--reps 20]

Prologue variants, each timed as `reps` back-to-back launches between two events (the records of every line and
layer; the line-sum is not run):
  air              rtx_line_prep            dil_air = 1 (the default path)
  mix air          rtx_line_prep_mix        {air: 1}
  mix self         rtx_line_prep_mix        {air: 1 - x, self: x} per species and layer (broadening="self")
  mix self+h2o     rtx_line_prep_mix        {air, self, h2o} (broadening=("self", "h2o"); the table gets gamma_h2o / n_h2o)
Whole step: TudRunner.run (prologue + line-sum + TUD) with broadening None (rtx_compute_tud) and "self", median of
`reps` steps, each between two events.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from radtxfr_amd import _lib, engine, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    lib = _lib.load()
    full = synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)
    rng = np.random.default_rng(1)
    full["gamma_h2o"] = np.round(rng.uniform(0.2, 0.5, full["nu"].size), 4)
    full["n_h2o"] = np.round(rng.uniform(0.5, 0.9, full["nu"].size), 2)
    a = synthetic.c3_atmosphere(32)
    lines = engine.LineTable(full)
    grid = engine.Grid(500.0, 6000.0, 5500000)
    nL = 32
    w, p_atm = engine.layer_weights_od(lines.species, a["Ts"], a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"])
    q, m = engine.species_factors(lines.species, a["Ts"], weight=w)
    plan = lines.plan(nL, grid.n)
    keep = [np.ascontiguousarray(x, dtype=np.float64) for x in (a["Ts"], p_atm, q, w, m)]
    env = [k.ctypes.data_as(C.c_void_p) for k in keep]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / reps

    def mix_call(dil):
        n_dil, idx, frac = engine.diluent_mix(lines, dil, nL)
        return lambda: _lib.check(lib.rtx_line_prep_mix(plan._h, lines._h, grid.byref(), nL, *env, n_dil, idx[1], frac[1], 0.0,
                                                        50.0, 0.0, 1.0, 0, st))

    variants = [
        ("air (rtx_line_prep)", lambda: _lib.check(lib.rtx_line_prep(plan._h, lines._h, grid.byref(), nL, *env, 1.0, 0.0, 0.0, 50.0,
                                                                     0.0, 1.0, st))),
        ("mix air", mix_call({"air": 1.0})),
        ("mix self", mix_call(engine.broadening_fractions(lines.species, a["MFs_VAL"], a["MFs_ID"], ()))),
        ("mix self+h2o", mix_call(engine.broadening_fractions(lines.species, a["MFs_VAL"], a["MFs_ID"], ("h2o",)))),
    ]
    print("device:", torch.cuda.get_device_name(0), "| C3: %d lines x %d layers, %d points" % (lines.n, nL, grid.n))
    base = None
    for name, fn in variants:
        ts = [timed(fn, args.reps) for _ in range(5)]
        t = float(np.median(ts))
        base = t if base is None else base
        print("prologue %-22s %.4f ms (min %.4f)  x%.2f of air" % (name, t, min(ts), t / base))

    Z = a["Zs"]
    for b in (None, "self"):
        run = engine.TudRunner(lines, grid, Z, n_layers=nL, broadening=b)
        ts = []
        for it in range(args.reps + 2):
            torch.cuda.synchronize()
            ev[0].record()
            run.run(a["Ts"], a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"])
            ev[1].record()
            torch.cuda.synchronize()
            if it >= 2:
                ts.append(ev[0].elapsed_time(ev[1]))
        print("compute_TUD step broadening=%-6s %.3f ms (min %.3f)" % (b, float(np.median(ts)), min(ts)))


if __name__ == "__main__":
    main()
