#!/usr/bin/env python3
"""The C3 step with the optical depths nobody reads left out (rtx_compute_tud_opts, RTX_CTUD_OD_SCRATCH), on
the C3 column and on thinned ones where nothing is hidden and the split only costs: a stream of atmospheres through
engine.TudPipelines as bench.py runs it, mixing ratios scaled by --scales, ms per atmosphere (median of --repeats timed
blocks of --steps). --keep-od passes keep_od=True (the plain order: one line-sum over all layers, one TUD launch), which is
also what RADTXFR_OD_SKIP=0 forces. --census fills the optical-depth buffer with NaN before one run and counts what was
left unwritten: line-sum tiles (16 rows of 64 points) and rows that the middle-layer launch passed over.

    python tools/time_od_skip.py [--scales 1,1e-1,1e-3] [--pipes 3] [--steps 60] [--repeats 5] [--keep-od] [--census]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from radtxfr_amd import engine, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scales", default="1,1e-1,1e-3")
ap.add_argument("--pipes", type=int, default=3)
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--keep-od", action="store_true")
ap.add_argument("--census", action="store_true")
args = ap.parse_args()
NL, N = 32, 5500000
full = synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)
a = synthetic.c3_atmosphere(NL)
grid = engine.Grid(500.0, 6000.0, N)
lines = engine.LineTable(full)
kw = dict(keep_od=True) if args.keep_od else {}
for scale in [float(s) for s in args.scales.split(",")]:
    mf = a["MFs_VAL"] * scale
    pipes = engine.TudPipelines(lines, grid, a["Zs"], n_layers=NL, n_pipes=args.pipes, **kw)

    def go(n):
        for _ in range(n):
            pipes.run(a["Ts"], a["Ps"], a["PLs"], mf, a["MFs_ID"])
    go(20)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        go(args.steps)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / args.steps * 1e3)
    print("mixing ratios x %-6g %s: %.4f ms per atmosphere (median of %d blocks of %d; range %.4f-%.4f)"
          % (scale, "keep_od=True" if args.keep_od else "OD scratch  ", float(np.median(ms)), args.repeats, args.steps, min(ms), max(ms)), flush=True)
    if args.census and not args.keep_od:
        run = pipes.runs[0]
        with torch.cuda.stream(pipes.streams[0]):
            run.OD.fill_(float("nan"))
            run.run(a["Ts"], a["Ps"], a["PLs"], mf, a["MFs_ID"])
            left = torch.isnan(run.OD[4])  # a layer of the middle launch
            assert not bool(torch.isnan(run.OD[:4]).any()) and not bool(torch.isnan(run.OD[20:]).any())
            pad = (-N) % 1024
            rows = torch.cat([left, left[-1:].expand((-N) % 64), left.new_ones(pad - (-N) % 64)]).view(-1, 16, 64)  # rows past the grid count as done
            assert bool((rows.all(2) == rows.any(2)).all()), "a row is left whole or not at all"
            rows = rows.all(2)
            n_tiles = rows.shape[0]
            print("  census: %d of %d rows done (%.1f %%); %d of %d tiles hidden whole (%.1f %%: the share of the middle launch's "
                  "workgroups that return at once); %d tiles partly hidden"
                  % (int(rows.flatten()[:(N + 63) // 64].sum()), (N + 63) // 64, 100.0 * int(left.sum()) / N, int(rows.all(1).sum()), n_tiles,
                     100.0 * int(rows.all(1).sum()) / n_tiles, int((rows.any(1) & ~rows.all(1)).sum())), flush=True)
        torch.cuda.synchronize()
    pipes.close()
lines.close()
