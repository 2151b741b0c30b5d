#!/usr/bin/env python3
"""Device time of the Hartmann-Tran line-sum (rtx_ht_prep + rtx_ht_sum) at the cross-section generator's settings
(misc/RT_gen_AbsXS_files.py:86-92: WavenumberStep = 0.0025, WavenumberWingHW = 350), next to the speed-dependent Voigt sum
(rtx_sdvoigt_sum: its point-by-point gather kernel and its default node-level kernel) on the same table, grid and state,
measured in the same call. Device events around enough repeats to fill half a second, three windows, after a warm-up of
every shape; profiler off.
    python tools/time_ht.py [--out profiles/ht_sum_time.txt] [--lines 2500]"""
import argparse, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from radtxfr_amd import engine, synthetic

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--lines", type=int, default=2500)
ap.add_argument("--min-seconds", type=float, default=0.5)
args = ap.parse_args()
engine.require_gpu()
rows = []


def say(s):
    print(s, flush=True)
    rows.append(s)


def timed(fn):
    """Median device time [s] of one call: warm-up, then windows of enough calls to fill --min-seconds, three times."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    fn()
    torch.cuda.synchronize()
    ev[0].record(); fn(); ev[1].record()
    torch.cuda.synchronize()
    reps = max(2, int(np.ceil(args.min_seconds / max(ev[0].elapsed_time(ev[1]) * 1e-3, 1e-6))))
    ts = []
    for _ in range(3):
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]) * 1e-3 / reps)
    return float(np.median(ts)), reps, (max(ts) - min(ts)) / float(np.median(ts))


HW, T, P = 350.0, 296.0, 1.0
X = np.linspace(800.0, 1000.0, 80001)  # step 0.0025
n = args.lines
rng = np.random.default_rng(2017)
tbl = dict(synthetic.synth_line_table(77, n, 760.0, 1040.0))
tbl["SD_air"] = np.round(rng.uniform(0.05, 0.2, n), 3)
ht = dict(tbl)
ht["gamma_HT_0_air_296"] = np.round(tbl["gamma_air"] * rng.uniform(0.8, 1.2, n), 4)
ht["n_HT_air_296"] = np.round(rng.uniform(0.4, 0.8, n), 2)
ht["gamma_HT_2_air_296"] = np.round(ht["gamma_HT_0_air_296"] * rng.uniform(0.05, 0.15, n), 5)
ht["delta_HT_2_air_296"] = np.round(rng.uniform(-5e-4, 5e-4, n), 6)
ht["nu_HT_air"] = np.round(rng.uniform(0.0, 0.02, n), 5)
ht["kappa_HT_air"] = np.round(rng.uniform(0.5, 1.0, n), 2)
ht["eta_HT_air"] = np.round(rng.uniform(0.0, 0.3, n), 3)
say("%s, %d lines (760-1040 cm^-1) on %d points (800-1000 cm^-1, step 0.0025), WavenumberWingHW = %g, T = %g K, p = %g atm, one state"
    % (torch.cuda.get_device_name(0), n, X.size, HW, T, P))
lib = engine._lib.load()
out = torch.empty((1, X.size), dtype=torch.float64, device="cuda")

lines = engine.LineTable(ht)
w = np.ones((len(lines.species), 1))
prm = engine.ht_line_params(lines, X, [T], [P], w, {"air": 1.0}, omega_wing_hw=HW)
pairs = int(np.sum(prm["window"][0][:, 1] - prm["window"][0][:, 0]))


def ht_both():
    engine.ht_sum(lines, X, [T], [P], w, {"air": 1.0}, out_f64=out, omega_wing_hw=HW)


def ht_sum_alone():  # the records of the last prologue stay in the plan
    engine._lib.check(lib.rtx_ht_sum(lines._ht_plan._h, 1, None, engine._ptr(out), X.size, engine._stream_ptr()))


ht_both()
rate = {}
for what, fn in (("line-sum kernel alone", ht_sum_alone), ("prologue + line-sum", ht_both)):
    t, reps, spread = timed(fn)
    rate[what] = pairs / t
    say("rtx_ht_sum (Hartmann-Tran columns: Bterm, common part)  %-22s %d (line, point) pairs, %8.3f ms  %.3e pairs/s  (%d launches per window, spread %.1f%%)"
        % (what + ",", pairs, t * 1e3, pairs / t, reps, spread * 100))

sd = engine.LineTable(tbl)
grid = engine.Grid.from_axis(X)
plan = sd.plan(1, grid.n)


def sd_both():
    engine.voigt_sum(sd, grid, np.array([T]), np.array([P]), w, out_f64=out, omega_wing_hw=HW, scale=1.0, profile=3)


def sd_sum_alone():
    engine._lib.check(lib.rtx_sdvoigt_sum(plan._h, grid.byref(), 1, None, engine._ptr(out), grid.n, engine._stream_ptr()))


for mode in ("gather", "tile"):
    if mode == "gather":
        os.environ["RADTXFR_SD_KERNEL"] = "gather"
    else:
        os.environ.pop("RADTXFR_SD_KERNEL", None)
    sd_both()
    for what, fn in (("line-sum kernel alone", sd_sum_alone), ("prologue + line-sum", sd_both)):
        t, reps, spread = timed(fn)
        rate[(mode, what)] = t
        say("rtx_sdvoigt_sum %-6s kernel (SD_air alone: Re Aterm)      %-22s %42.3f ms  (%d launches per window, spread %.1f%%)"
            % (mode, what + ",", t * 1e3, reps, spread * 100))
os.environ.pop("RADTXFR_SD_KERNEL", None)
say("rtx_ht_sum / rtx_sdvoigt_sum gather kernel, line-sum kernels alone: %.1f x the time; / the node-level kernel: %.1f x"
    % (pairs / rate["line-sum kernel alone"] / rate[("gather", "line-sum kernel alone")],
       pairs / rate["line-sum kernel alone"] / rate[("tile", "line-sum kernel alone")]))
say("For scale: rtx_profile_sum evaluates 3.8e10 (line, point) pairs/s with the same profile (profiles/profiles_time.txt).")
lines.close()
sd.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(rows) + "\n")
