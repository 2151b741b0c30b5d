#!/usr/bin/env python3
"""Throughput of the line-profile evaluator (rtx_profile_eval / rtx_profile_sum, the complete pcqsdhc in fp64, complex)
next to the existing point-by-point path of the speed-dependent Voigt line-sum (sdvoigt_kernel, RADTXFR_SD_KERNEL=gather:
Re(Aterm)/pi only, with its real-only shortcuts), re-measured in the same call. Device events around enough repeats to fill
half a second, after a warm-up of every shape; profiler off.
    python tools/time_profiles.py [--out profiles/profiles_time.txt] [--lines 1024] [--points 65536]"""
import argparse, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from radtxfr_amd import engine, hapi, synthetic

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--lines", type=int, default=1024)
ap.add_argument("--points", type=int, default=65536)
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


say("%s, %d lines x %d points = %.2e evaluations per launch" % (torch.cuda.get_device_name(0), args.lines, args.points, args.lines * args.points))
nL, n = args.lines, args.points
sg0 = np.linspace(1000.0, 1002.0, nL)
sg = torch.as_tensor(np.linspace(998.0, 1004.0, n), device="cuda")
midp = dict(GamD=0.0012, Gam0=0.005, Gam2=0.0006, Shift0=-0.0002, Shift2=0.00005, anuVC=0.001, eta=0.3)
sets = (("ht_midp parameters (Bterm, common part, complex)", midp),
        ("SDVoigt-only parameters (anuVC = eta = Shift2 = 0: no Bterm)", dict(midp, Shift2=0.0, anuVC=0.0, eta=0.0)))
w = torch.ones(nL, dtype=torch.float64, device="cuda")
rate = {}
for label, kw in sets:
    P = torch.as_tensor(hapi._line_params(sg0, kw["GamD"], kw["Gam0"], kw["Gam2"], kw["Shift0"], kw["Shift2"], kw["anuVC"], kw["eta"]), device="cuda")
    for what, fn in (("eval (re + im stored)", lambda: engine.profile_eval(engine.LS_PCQSDHC, P, sg)),
                     ("eval (re only stored)", lambda: engine.profile_eval(engine.LS_PCQSDHC, P, sg, imag=False)),
                     ("sum  (weights + mixing)", lambda: engine.profile_sum(P, w, w, sg))):
        t, reps, spread = timed(fn)
        rate[(label, what)] = nL * n / t
        say("%-62s %-24s %8.3f ms per launch  %.3e evaluations/s  (%d launches per window, spread %.1f%%)"
            % (label, what, t * 1e3, nL * n / t, reps, spread * 100))

# the existing point-by-point path: every point of every window through sdvoigt_profile. A fixed window of +-W cm^-1
# (OmegaWing = W, OmegaWingHW = 0) makes the number of (line, point) pairs a host-side count.
W, n_lines = 10.0, 2000
X = np.linspace(900.0, 1100.0, 200001)
tbl = dict(synthetic.synth_line_table(2016, n_lines, 900.0, 1100.0))
tbl["SD_air"] = np.round(np.random.default_rng(5).uniform(0.05, 0.2, n_lines), 3)
hapi.storage2cache_from_columns("tp", tbl)
lines = hapi._device_table(["tp"])
grid = engine.Grid.from_axis(X)
nu = np.asarray(tbl["nu"], dtype=np.float64)
pairs = int(np.sum(np.searchsorted(X, nu + W, "right") - np.searchsorted(X, nu - W, "left")))
wgt = np.ones((len(lines.species), 1))
out = torch.empty((1, grid.n), dtype=torch.float64, device="cuda")
lib = engine._lib.load()
plan = lines.plan(1, grid.n)


def prologue_and_sum():
    engine.voigt_sum(lines, grid, np.array([296.0]), np.array([1.0]), wgt, out_f64=out, omega_wing=W, omega_wing_hw=0.0, scale=1.0, profile=3)


def sum_alone():  # the records of the last prologue stay in the plan: the line-sum kernel on its own, like rtx_profile_eval
    engine._lib.check(lib.rtx_sdvoigt_sum(plan._h, grid.byref(), 1, None, engine._ptr(out), grid.n, engine._stream_ptr()))


for mode in ("gather", "tile"):
    if mode == "gather":
        os.environ["RADTXFR_SD_KERNEL"] = "gather"
    else:
        os.environ.pop("RADTXFR_SD_KERNEL", None)
    prologue_and_sum()
    assert lines.plan(1, grid.n) is plan
    for what, fn in (("line-sum kernel alone", sum_alone), ("prologue + line-sum", prologue_and_sum)):
        t, reps, spread = timed(fn)
        if fn is sum_alone:
            rate[mode] = pairs / t
        say("rtx_sdvoigt_sum %-6s kernel, %-21s %d lines x %d points, window +-%g cm^-1: %d (line, point) pairs, %8.3f ms  %.3e pairs/s"
            "  (%d launches per window, spread %.1f%%)" % (mode, what + ",", n_lines, grid.n, W, pairs, t * 1e3, pairs / t, reps, spread * 100))
os.environ.pop("RADTXFR_SD_KERNEL", None)
for label, _ in sets:
    say("gather line-sum kernel rate / rtx_profile_eval rate (kernel against kernel), %s: %.2f"
        % (label, rate["gather"] / rate[(label, "eval (re + im stored)")]))
say("What the two rates count. A pair of the gather kernel is Re(Aterm)/pi of one point: real parts only (the real two-term Weideman\n"
    "recurrence, half the operations of the complex Horner form), the closed-form far wing where both arguments are beyond\n"
    "|x| + y = 15, per-line reciprocals taken from the prologue's record, Newton reciprocals and square roots instead of the IEEE\n"
    "sequences, and one accumulated value per point, so nothing is stored per pair. An evaluation of rtx_profile_eval is the\n"
    "complex LS: both complex probability functions in full (24 complex Horner steps each), Bterm and the common part's complex\n"
    "division when eta != 0, library division / sqrt / hypot throughout, and 16 bytes stored per evaluation (re and im).")
say("CPU reference (misc/hapi.py pcqsdhc, one core): not measured in this call; the figure quoted for it is 1.6 ms per vector call of "
    "2001 points, 1.2e6 points/s")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(rows) + "\n")
