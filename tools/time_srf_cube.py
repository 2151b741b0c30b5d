"""The per-pixel HSI cube under tabulated response functions (sensor.hsi_cube_srf: srf_moments at the node temperatures ->
rtx_srf_cube_tables -> rtx_srf_pixel_cube) on config C5's input: synthetic.synth_scene's 256 x 256 pixels
(mixtures of 2 out of 6 endmembers on synthetic.synth_emissivities' knots, T = 287.87 + 3 N(0, 1) K) from tau / La / Ld
on the MAKO span of the C3 grid (570 000 wavenumbers, 755 - 1325 cm^-1).

    python tools/time_srf_cube.py [--reps 10] [--out profiles/srf_cube_time.txt]

runs the three measurements below one after the other, each in a child process of its own under `timeout` (a step that
faults or hangs ends the run: nothing further is started on the device). A time is the median of 5 rounds, after a warm-up
round, of `reps` back-to-back calls between two device events, host side of the calls included; functions timed together
alternate per round. Each step times hsi_cube_srf (8 nodes, explicit T_range: no synchronisation) and its three stages on
their own, and prints the pixel kernel's achieved bytes/s against the cube written once (it also reads kidx, frac and
Tpix: 20 bytes per pixel and block of 64 bands, not counted).

  mako        Sensor.mako(resFactor=2): 256 three-knot triangles; also sensor.hsi_cube (resFactor=2) on the same inputs,
              the MAKO-only path, whole and its rtx_pixel_cube stage alone, and the largest difference between the two cubes
  radiometer  6 boxcar bands of 100 cm^-1
  gauss512    512 Gaussian bands, centres evenly spaced over the axis, FWHM = 2 band spacings, 65 knots each
"""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q = 8
STEPS = (("mako", 300), ("radiometer", 300), ("gauss512", 300))


def timed(torch, fns):
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
    lib = _lib.load()
    say = lambda s: print(s, flush=True)
    full = engine.Grid(500.0, 6000.0, 5500000)
    i0, i1 = int((755.0 - 500.0) / full.step), int((1325.0 - 500.0) / full.step)
    grid = full.shard(i0, i1 - i0)
    X = grid.axis()
    f32 = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float32), device="cuda")
    tau, La, Ld = f32(0.5 + 0.45 * np.sin(X / 13.0)), f32(2.0 + np.cos(X / 29.0)), f32(4.0 + 2.0 * np.sin(X / 7.0))
    Xk, em = synthetic.synth_emissivities(n_emis=2000)
    sc = synthetic.synth_scene()
    E = f32(em[:, sc["end_idx"]]).contiguous()  # the column selection leaves NumPy strides of its own
    kidx, frac, T = torch.as_tensor(sc["kidx"], device="cuda"), f32(sc["frac"]), torch.as_tensor(sc["T"], device="cuda")
    T_range = (float(np.floor(sc["T"].min())), float(np.ceil(sc["T"].max())))
    if step == "mako":
        s = sensor.Sensor.mako(X[0], X[-1], resFactor=2)
    elif step == "radiometer":
        s = sensor.Sensor.from_shape(X[0] + 80.0 * np.arange(1, 7), 100.0, "boxcar")
    else:
        c = np.linspace(X[0], X[-1], 514)[1:-1]
        s = sensor.Sensor.from_shape(c, 2.0 * (c[1] - c[0]), "gaussian")
    nB, nk, nEnd, (nPix, nMix) = len(s), len(Xk), E.shape[1], kidx.shape
    say("%d bands, %d response knots in all; %d points; %d pixels, mixtures of %d out of %d endmembers on %d knots; %d nodes over [%g, %g] K, "
        "estimated interpolation error %.2g; cube %.1f MB" % (nB, s.knot_start[-1], grid.n, nPix, nMix, nEnd, nk, Q, T_range[0], T_range[1],
                                                           sensor.planck_node_error(X[-1], T_range[0], T_range[1], Q), 4e-6 * nB * nPix))
    whole = lambda: sensor.hsi_cube_srf(grid, tau, La, Ld, Xk, E, kidx, frac, T, s, n_nodes=Q, T_range=T_range)[1]
    # the three stages on their own, as hsi_cube_srf chains them
    nodes = sensor.srf_cube_nodes(T_range[0], T_range[1], Q)
    Xk_d = torch.as_tensor(np.asarray(Xk, dtype=np.float64), device="cuda")
    N, Cb, M, jr = sensor.srf_moments(grid, tau, La, Ld, Xk_d, nodes, s)
    tab = torch.empty((nEnd, Q, nB), dtype=torch.float32, device="cuda")
    cube = torch.empty((nB, nPix), dtype=torch.float32, device="cuda")
    T_host = np.ascontiguousarray(np.concatenate([nodes, T_range]))
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fns = {"hsi_cube_srf": (whole, reps),
           "  srf_moments (%d temperatures)" % Q: (lambda: sensor.srf_moments(grid, tau, La, Ld, Xk_d, nodes, s), reps),
           "  rtx_srf_cube_tables": (lambda: _lib.check(lib.rtx_srf_cube_tables(p(M), p(jr), nB, Q, nk, p(E), nEnd, p(tab), st)), reps),
           "  rtx_srf_pixel_cube": (lambda: _lib.check(lib.rtx_srf_pixel_cube(nB, Q, T_host.ctypes.data_as(C.c_void_p), p(N), p(Cb), p(tab), nEnd,
                                                                              nPix, nMix, p(kidx), p(frac), p(T), p(cube), st)), reps)}
    if step == "mako":
        fns["hsi_cube (MAKO only)"] = (lambda: sensor.hsi_cube(grid, tau, La, Ld, Xk, E, kidx, frac, T, resFactor=2)[1], reps)
        # its pixel stage alone, on the tables a whole call leaves behind
        plan = sensor._cube_plan(grid, Xk, 2, None, 4, None, tau.device)
        N4, C4 = (torch.empty(nB, dtype=torch.float32, device="cuda") for _ in range(2))
        M4 = torch.empty((5, nB, nk), dtype=torch.float32, device="cuda")
        jr4 = torch.empty((nB, 2), dtype=torch.int32, device="cuda")
        tab4 = torch.empty((nEnd, 5, nB), dtype=torch.float32, device="cuda")
        cube4 = torch.empty((nB, nPix), dtype=torch.float32, device="cuda")
        _lib.check(lib.rtx_band_basis_moments(0, grid.byref(), p(tau), p(La), p(Ld), p(plan["Xk_d"]), nk, nB, p(plan["c_d"]), p(plan["s_d"]), 4,
                                              plan["coef32"].ctypes.data_as(C.c_void_p), 1.0, p(N4), p(C4), p(M4[4]), p(M4), p(jr4), st))
        _lib.check(lib.rtx_band_mix_stacked(p(M4), p(jr4), nB, 5, nk, p(E), nEnd, p(tab4), st))
        fns["  rtx_pixel_cube (Q = 4)"] = (lambda: _lib.check(lib.rtx_pixel_cube(nB, 4, p(plan["c_d"]), p(plan["s_d"]), 1.0,
                                                                                 plan["sn32"].ctypes.data_as(C.c_void_p), p(N4), p(C4), p(tab4), nEnd,
                                                                                 nPix, nMix, p(kidx), p(frac), p(T), p(cube4), st)), reps)
    t = timed(torch, fns)
    for k, (ms, lo, hi) in t.items():
        say("  %-34s %10.4f ms per call (min %.4f, max %.4f of 5 medians over %d calls)" % (k, ms, lo, hi, fns[k][1]))
    ms = t["  rtx_srf_pixel_cube"][0]
    say("  rtx_srf_pixel_cube writes the cube once: %.1f MB in %.4f ms = %.2f TB/s" % (4e-6 * nB * nPix, ms, 4.0 * nB * nPix / (ms * 1e-3) / 1e12))
    a = whole()
    torch.cuda.synchronize()
    say("  finite bands %d of %d; the stages' cube equals hsi_cube_srf's bit for bit: %s"
        % (int(torch.isfinite(a).all(dim=1).sum()), nB, bool(torch.equal(torch.nan_to_num(a), torch.nan_to_num(cube)))))
    if step == "mako":
        b = sensor.hsi_cube(grid, tau, La, Ld, Xk, E, kidx, frac, T, resFactor=2)[1]
        torch.cuda.synchronize()
        _, cen, sig = sensor.mako_bands(X[0], X[-1], 2)
        inside = torch.as_tensor((cen - sig > X[0]) & (cen + sig < X[-1]), device="cuda")
        d = ((a - b).abs() / b.abs().amax(dim=1, keepdim=True))[inside].max().item()
        say("  largest difference from hsi_cube, relative to the band's largest radiance: %.3g (%d bands that reach neither end of the grid)"
            % (d, int(inside.sum())))


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
    text = ["# python tools/time_srf_cube.py --reps %d" % args.reps,
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
