"""Band averages under tabulated response functions (rtx_srf_apply) on config C4's input: 560 000 wavenumbers
(750 - 1310 cm^-1 at 0.001 cm^-1) x 2000 columns of float32, 4.48 GB.

    python tools/time_srf.py [--reps 10] [--out profiles/srf_time.txt]

runs the three measurements below one after the other, each in a child process of its own under `timeout` (a step that
faults or hangs ends the run: nothing further is started on the device). Each times `reps` back-to-back calls between two
device events, median of 5 rounds after a warm-up round, and reports achieved bytes/s against the size of Y read ONCE.

  mako        Sensor.mako (128 three-knot triangles) through rtx_srf_apply, against rtx_ils kind 0 on the same data, the two
              alternating; also the largest difference between the two results over the bands wholly inside the axis
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

XMIN, XMAX, NX, NS = 750.0, 1310.0, 560000, 2000
STEPS = (("mako", 600), ("radiometer", 600), ("gauss512", 600))


def timed(torch, fns, reps):
    """Median ms per call of each function: rounds of `reps` back-to-back calls, the functions alternating per round."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts = {k: [] for k in fns}
    for _ in range(6):  # the first round warms up
        for k, fn in fns.items():
            fn()
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(reps):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            ts[k].append(ev[0].elapsed_time(ev[1]) / reps)
    return {k: (float(np.median(v[1:])), min(v[1:]), max(v[1:])) for k, v in ts.items()}


def child(step, reps):
    import torch
    from radtxfr_amd import _lib, engine, sensor
    _lib.load()
    say = lambda s: print(s, flush=True)
    grid = engine.Grid(XMIN, XMAX, NX)
    g = torch.Generator(device="cuda").manual_seed(1)
    Y = torch.rand((NX, NS), dtype=torch.float32, device="cuda", generator=g) + 0.5  # random data, not zeros
    nbytes = 4.0 * NX * NS
    if step == "mako":
        s = sensor.Sensor.mako(XMIN, XMAX)
        _, c, sg = sensor.mako_bands(XMIN, XMAX)
        c_d, s_d = torch.as_tensor(c, device="cuda"), torch.as_tensor(sg, device="cuda")
        fns = {"rtx_srf_apply": lambda: sensor.apply_srf(s, Y, grid=grid), "rtx_ils kind 0": lambda: engine.ils(0, Y, c_d, s_d, grid=grid)}
    elif step == "radiometer":
        s = sensor.Sensor.from_shape(XMIN + 80.0 * np.arange(1, 7), 100.0, "boxcar")
        fns = {"rtx_srf_apply": lambda: sensor.apply_srf(s, Y, grid=grid)}
    else:
        c = np.linspace(XMIN, XMAX, 514)[1:-1]
        s = sensor.Sensor.from_shape(c, 2.0 * (c[1] - c[0]), "gaussian")
        fns = {"rtx_srf_apply": lambda: sensor.apply_srf(s, Y, grid=grid)}
    say("%d bands, %d knots in all; Y %d x %d float32 = %.2f GB" % (len(s), s.knot_start[-1], NX, NS, nbytes / 1e9))
    for k, (t, lo, hi) in timed(torch, fns, reps).items():
        say("  %-16s %.3f ms per call (min %.3f, max %.3f of 5 medians over %d calls) -> %.2f TB/s of Y read once"
            % (k, t, lo, hi, reps, nbytes / t / 1e9))
    if step == "mako":
        a = fns["rtx_srf_apply"]()[1]
        b = fns["rtx_ils kind 0"]()
        inside = torch.as_tensor((c - sg >= XMIN) & (c + sg <= XMAX), device="cuda")
        d = ((a - b).abs() / b.abs())[inside].max().item()
        say("  largest relative difference between the two over the %d bands wholly inside the axis: %.3g" % (int(inside.sum()), d))


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
    text = ["# python tools/time_srf.py --reps %d" % args.reps,
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
