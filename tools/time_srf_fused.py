"""Fused band radiances under tabulated response functions (rtx_srf_moments + rtx_band_mix) on config C4's
input: 560 000 wavenumbers (750 - 1310 cm^-1 at 0.001 cm^-1), 2000 emissivities on synthetic.synth_emissivities' 791 knots.

    python tools/time_srf_fused.py [--reps 10] [--out profiles/srf_fused_time.txt]

runs the three measurements below one after the other, each in a child process of its own under `timeout` (a step that
faults or hangs ends the run: nothing further is started on the device). Each times sensor.band_radiance_srf_fused against
sensor.band_radiance_srf (rtx_interp_knots -> rtx_apparent_radiance -> rtx_srf_apply, which forms [nX][nE] twice: 4.48 GB
each) for one surface temperature and for the reference's 41 (Ts + arange(-10, 10.5, 0.5); the unfused path is called
once per temperature). A time is the median of 5 rounds, after a warm-up round, of back-to-back calls between two device
events, host side of the calls included. Also printed: the largest difference between the two results relative to each
band's largest radiance, and the bytes of tau / La / Ld (read once per launch group of 16 bands that reaches them).

  mako        Sensor.mako (128 three-knot triangles); also sensor.band_radiance_fused kind 0, the MAKO-only fused path
  radiometer  6 boxcar bands of 100 cm^-1
  gauss512    512 Gaussian bands, centres evenly spaced over the axis, FWHM = 2 band spacings, 65 knots each
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

XMIN, XMAX, NX, NE, TS0 = 750.0, 1310.0, 560000, 2000, 287.87
DT = np.arange(-10.0, 10.5, 0.5)  # Compute_LWIR_Apparent_Radiance.py:24-25
STEPS = (("mako", 300), ("radiometer", 300), ("gauss512", 300))


def timed(torch, fns, reps):
    """Median ms per call of each (function, calls per round): the functions alternate per round; the first round warms up."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts = {k: [] for k in fns}
    for _ in range(6):
        for k, (fn, n) in fns.items():
            fn()
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(n):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            ts[k].append(ev[0].elapsed_time(ev[1]) / n)
    return {k: (float(np.median(v[1:])), min(v[1:]), max(v[1:])) for k, v in ts.items()}


def child(step, reps):
    import torch
    from radtxfr_amd import _lib, engine, sensor, synthetic
    _lib.load()
    say = lambda s: print(s, flush=True)
    grid = engine.Grid(XMIN, XMAX, NX)
    X = grid.axis()
    f32 = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float32), device="cuda")
    tau, La, Ld = f32(0.5 + 0.45 * np.sin(X / 13.0)), f32(2.0 + np.cos(X / 29.0)), f32(4.0 + 2.0 * np.sin(X / 7.0))
    Xk, em = synthetic.synth_emissivities(n_emis=NE)
    E = f32(em)
    if step == "mako":
        s = sensor.Sensor.mako(XMIN, XMAX)
    elif step == "radiometer":
        s = sensor.Sensor.from_shape(XMIN + 80.0 * np.arange(1, 7), 100.0, "boxcar")
    else:
        c = np.linspace(XMIN, XMAX, 514)[1:-1]
        s = sensor.Sensor.from_shape(c, 2.0 * (c[1] - c[0]), "gaussian")
    Ts41 = TS0 + DT
    say("%d bands, %d response knots in all; %d points, %d emissivities on %d knots; tau + La + Ld = %.2f MB; [nX][nE] = %.2f GB"
        % (len(s), s.knot_start[-1], NX, NE, len(Xk), 12.0 * NX / 1e6, 4.0 * NX * NE / 1e9))
    fused = lambda Ts: sensor.band_radiance_srf_fused(grid, tau, La, Ld, Xk, E, Ts, s)[1]
    unfused = lambda Ts: sensor.band_radiance_srf(grid, tau, La, Ld, Xk, E, Ts, s)[1]

    def unfused41():
        for T in Ts41:
            unfused(float(T))

    few = max(1, reps // 5)
    fns = {"fused nT=1": (lambda: fused(TS0), reps), "unfused nT=1": (lambda: unfused(TS0), reps),
           "fused nT=41": (lambda: fused(Ts41), reps), "unfused nT=41": (unfused41, few)}
    if step == "mako":
        fns["band_radiance_fused kind 0"] = (lambda: sensor.band_radiance_fused(grid, tau, La, Ld, Xk, E, TS0, kind=0), reps)
    t = timed(torch, fns, reps)
    for k, (ms, lo, hi) in t.items():
        say("  %-28s %10.3f ms per call (min %.3f, max %.3f of 5 medians over %d calls)" % (k, ms, lo, hi, fns[k][1]))
    for n in (1, 41):
        say("  nT=%-2d unfused / fused = %.1f" % (n, t["unfused nT=%d" % n][0] / t["fused nT=%d" % n][0]))
    a, b = fused(TS0), unfused(TS0)
    torch.cuda.synchronize()
    ok = torch.isfinite(b).all(dim=1)
    d = ((a - b).abs() / b.abs().amax(dim=1, keepdim=True))[ok].max().item()
    say("  largest difference between the two at nT=1, relative to the band's largest radiance: %.3g (%d finite bands)" % (d, int(ok.sum())))
    a41 = fused(Ts41)
    say("  fused nT=41 slice 20 (Ts0) equals the nT=1 result bit for bit: %s" % bool(torch.equal(a41[20][ok], a[ok])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=[s for s, _ in STEPS])
    args = ap.parse_args()
    if args.step:
        child(args.step, args.reps)
        return
    import torch
    text = ["# python tools/time_srf_fused.py --reps %d" % args.reps,
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
