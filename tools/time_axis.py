#!/usr/bin/env python3
"""The line-sum on an explicit axis (engine.voigt_sum_axis: rtx_line_prep_axis + rtx_voigt_sum_axis), HIP-event times of
prologue + line-sum, median of 7 after 2 warm-up calls:
  (a) the two-density grid of tests/test_gpu_linesum_axis.py (a): 950-1050 cm^-1, 0.0005 within +-2 cm^-1 of the strongest
      line, 0.02 elsewhere; the G4 table (2000 lines), at (296 K, 1 atm) and (220 K, 0.02 atm)
  (b) config C2 (BASELINE): 700-1400 cm^-1 @ 0.01 (70 000 points), 20 000 lines, one layer at the surface state -- a uniform
      grid forced through the axis path, next to the same grid on the default nodal line-sum and on
      RADTXFR_VOIGT_KERNEL=scatter (measured in a child process: the kernel choice is read once per process)
  (c) the clustered band head of test (f) on its two-density grid (~3000 lines inside 0.5 cm^-1; axis tiles are never cut)
    python tools/time_axis.py"""
import argparse, json, math, os, subprocess, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from radtxfr_amd import engine, synthetic

ap = argparse.ArgumentParser()
ap.add_argument("--uniform-only", action="store_true", help="(child) time C2 on the grid path only and print JSON")
args = ap.parse_args()


def timed(fn, reps=7, warm=2):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts = []
    for r in range(warm + reps):
        torch.cuda.synchronize()
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        if r >= warm:
            ts.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(ts))


def setup(tbl, nL=1):
    lines = engine.LineTable(tbl)
    scale = 2.0 ** (-math.floor(math.log2(float(np.max(tbl["sw"])))))
    return lines, np.ones((len(lines.species), nL)), scale


def two_density(lo, hi, centre, half, fine, coarse):
    return np.concatenate([np.arange(lo, centre - half, coarse), np.arange(centre - half, centre + half, fine),
                           np.arange(centre + half, hi, coarse)])


c2 = synthetic.synth_line_table(synthetic.SEED_C2, 20000, 675.0, 1425.0)
T2, p2 = 287.87, 100697.30225 / 101325.0
if args.uniform_only:
    lines, w, scale = setup(c2)
    grid = engine.Grid(700.0, 1400.0, 70000)
    out = torch.empty((1, grid.n), dtype=torch.float64, device="cuda")
    ms = timed(lambda: engine.voigt_sum(lines, grid, [T2], [p2], w, out_f64=out, scale=scale))
    print(json.dumps({"ms": ms, "kernel": os.environ.get("RADTXFR_VOIGT_KERNEL", "nodal")}))
    sys.exit(0)

print(f"device: {torch.cuda.get_device_name(0)}; prologue + line-sum, HIP events, median of 7", flush=True)
# (a)
g4 = synthetic.synth_line_table(synthetic.SEED_C2, 2000, 675.0, 1425.0)
sel = (g4["nu"] > 952.0) & (g4["nu"] < 1048.0)
X = two_density(950.0, 1050.0, float(g4["nu"][sel][np.argmax(g4["sw"][sel])]), 2.0, 0.0005, 0.02)
lines, w, scale = setup(g4)
out = torch.empty((1, X.size), dtype=torch.float64, device="cuda")
for T, p in ((296.0, 1.0), (220.0, 0.02)):
    ms = timed(lambda: engine.voigt_sum_axis(lines, X, [T], [p], w, out_f64=out, scale=scale))
    print(f"(a) two-density grid, {X.size} points, {g4['nu'].size} lines, T={T} p={p}: axis path {ms:.3f} ms", flush=True)
lines.close()
# (b)
lines, w, scale = setup(c2)
Xc = np.linspace(700.0, 1400.0, 70000)
out = torch.empty((1, Xc.size), dtype=torch.float64, device="cuda")
ms_axis = timed(lambda: engine.voigt_sum_axis(lines, Xc, [T2], [p2], w, out_f64=out, scale=scale))
grid = engine.Grid(700.0, 1400.0, 70000)
ms_nodal = timed(lambda: engine.voigt_sum(lines, grid, [T2], [p2], w, out_f64=out, scale=scale))
lines.close()
env = dict(os.environ, RADTXFR_VOIGT_KERNEL="scatter")
res = subprocess.run([sys.executable, os.path.abspath(__file__), "--uniform-only"], env=env, capture_output=True, text=True,
                     timeout=300)
ms_scatter = json.loads(res.stdout.strip().splitlines()[-1])["ms"] if res.returncode == 0 else float("nan")
print(f"(b) C2, 70000 points @ 0.01, 20000 lines, 1 layer: axis path {ms_axis:.3f} ms | grid path, nodal (default) "
      f"{ms_nodal:.3f} ms | grid path, scatter {ms_scatter:.3f} ms", flush=True)
# (c)
clu = synthetic.synth_clustered_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)
h, edges = np.histogram(clu["nu"], bins=np.arange(475.0, 6026.0, 0.5))
head = float(edges[int(np.argmax(h))])
Xh = two_density(head - 1.0, head + 1.5, head + 0.25, 0.5, 0.0005, 0.002)
sub = synthetic.subset_table(clu, Xh[0] - 12.0, Xh[-1] + 12.0)
lines, w, scale = setup(sub)
out = torch.empty((1, Xh.size), dtype=torch.float64, device="cuda")
for T, p in ((287.9, 0.994), (220.0, 0.01)):
    ms = timed(lambda: engine.voigt_sum_axis(lines, Xh, [T], [p], w, out_f64=out, scale=scale))
    print(f"(c) clustered band head ({int(h.max())} lines in 0.5 cm^-1), two-density grid, {Xh.size} points, {sub['nu'].size} "
          f"lines, T={T} p={p}: axis path {ms:.3f} ms", flush=True)
lines.close()
