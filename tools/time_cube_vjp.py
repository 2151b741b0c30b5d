"""The adjoint of the per-pixel HSI cube (sensor.hsi_cube_srf_vjp: srf_moments at the nodes -> rtx_srf_cube_tables ->
rtx_srf_pixel_cube_vjp -> band_radiance_srf_vjp at the nodes with [E | 0]) next to its forward, sensor.hsi_cube_srf,
on config C5's input: 256 x 256 pixels, Sensor.mako(resFactor=2)'s 256 bands, tau / La / Ld on the MAKO span of the C3 grid
(570 000 wavenumbers, 755 - 1325 cm^-1), 8 nodes.

    python tools/time_cube_vjp.py [--reps 10] [--out profiles/cube_vjp_time.txt]

runs the two scenes below one after the other, each in a child process of its own under `timeout` (a step that faults or
hangs ends the run: nothing further is started on the device). A time is the median of 5 rounds, after a warm-up round, of
`reps` back-to-back calls between two device events, host side of the calls included; the functions timed together
alternate per round, so the adjoint and the forward see the same machine. The new half is timed through its entry with one
group of outputs at a time: (dT, dfrac) is scv_pixel_kernel + scv_finish_kernel, (gL) is scv_gl_kernel + scv_sum_kernel; the
two small kernels ride with the large one they follow.

  small   synthetic.synth_scene: mixtures of 2 out of 6 endmembers (the pixel kernel's table in LDS, one slice of the reduction)
  end400  the same pixels' temperatures, mixtures of 3 out of 400 endmembers (table in global memory, 29 slices: g is read
          once per slice by the reduction, and once by the pixel kernel)
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
STEPS = (("small", 300), ("end400", 300))


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
    if step == "end400":
        r = np.random.default_rng(77)
        nPix = sc["T"].size
        fr = r.random((nPix, 3)) + 0.05
        sc = dict(end_idx=np.arange(400), kidx=r.integers(0, 400, (nPix, 3)).astype(np.int32), frac=fr / fr.sum(axis=1, keepdims=True), T=sc["T"])
    E = f32(em[:, sc["end_idx"]]).contiguous()
    kidx, frac, T = torch.as_tensor(sc["kidx"], device="cuda"), f32(sc["frac"]), torch.as_tensor(sc["T"], device="cuda")
    T_range = (float(np.floor(sc["T"].min())), float(np.ceil(sc["T"].max())))
    s = sensor.Sensor.mako(X[0], X[-1], resFactor=2)
    nB, nk, nEnd, (nPix, nMix) = len(s), len(Xk), E.shape[1], kidx.shape
    g = torch.as_tensor(np.random.default_rng(5).uniform(-1.0, 1.0, (nB, nPix)).astype(np.float32), device="cuda")
    eps = 112 // Q
    n_slices = (nEnd + eps - 1) // eps
    say("%d bands; %d points; %d pixels, mixtures of %d out of %d endmembers on %d knots; %d nodes over [%g, %g] K; cube and g %.1f MB each; "
        "table %d rows: %s in the pixel kernel, %d slice(s) of the reduction"
        % (nB, grid.n, nPix, nMix, nEnd, nk, Q, T_range[0], T_range[1], 4e-6 * nB * nPix, nEnd * Q,
           "LDS" if nEnd * Q <= 128 else "global memory", n_slices))
    args = (grid, tau, La, Ld, Xk, E, kidx, frac, T, s)
    fwd = lambda: sensor.hsi_cube_srf(*args, n_nodes=Q, T_range=T_range)[1]
    vjp = lambda outputs: (lambda: sensor.hsi_cube_srf_vjp(*args, g, n_nodes=Q, T_range=T_range, outputs=outputs))
    nodes = sensor.srf_cube_nodes(T_range[0], T_range[1], Q)
    Xk_d = torch.as_tensor(np.asarray(Xk, dtype=np.float64), device="cuda")
    N, Cb, M, jr = sensor.srf_moments(grid, tau, La, Ld, Xk_d, nodes, s)
    tab = torch.empty((nEnd, Q, nB), dtype=torch.float32, device="cuda")
    cube = torch.empty((nB, nPix), dtype=torch.float32, device="cuda")
    dT = torch.empty(nPix, dtype=torch.float64, device="cuda")
    dfrac = torch.empty((nPix, nMix), dtype=torch.float64, device="cuda")
    gL = torch.empty((Q, nB, nEnd + 1), dtype=torch.float32, device="cuda")
    E0 = torch.cat([E, torch.zeros((nk, 1), dtype=torch.float32, device="cuda")], dim=1)
    T_host = np.ascontiguousarray(np.concatenate([nodes, T_range]))
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.rtx_srf_cube_tables(p(M), p(jr), nB, Q, nk, p(E), nEnd, p(tab), st))
    new_half = lambda a, b, c: (lambda: _lib.check(lib.rtx_srf_pixel_cube_vjp(nB, Q, T_host.ctypes.data_as(C.c_void_p), p(N), p(tab), nEnd, nPix, nMix,
                                                                              p(kidx), p(frac), p(T), p(g), p(a), p(b), p(c), st, 0)))
    new_half(dT, dfrac, gL)()
    fns = {"hsi_cube_srf (forward)": (fwd, reps),
           "hsi_cube_srf_vjp, all six outputs": (vjp(("G_tau", "G_La", "G_Ld", "Tpix", "frac", "endmembers")), reps),
           "hsi_cube_srf_vjp, Tpix and frac only": (vjp(("Tpix", "frac")), reps),
           "  srf_moments (%d temperatures)" % Q: (lambda: sensor.srf_moments(grid, tau, La, Ld, Xk_d, nodes, s), reps),
           "  rtx_srf_pixel_cube (forward)": (lambda: _lib.check(lib.rtx_srf_pixel_cube(nB, Q, T_host.ctypes.data_as(C.c_void_p), p(N), p(Cb), p(tab),
                                                                                        nEnd, nPix, nMix, p(kidx), p(frac), p(T), p(cube), st)), reps),
           "  rtx_srf_pixel_cube_vjp, all": (new_half(dT, dfrac, gL), reps),
           "    dT, dfrac: pixel + finish kernels": (new_half(dT, dfrac, None), reps),
           "    gL: reduction + chunk-sum kernels": (new_half(None, None, gL), reps),
           "  band_radiance_srf_vjp (back half)": (lambda: sensor.band_radiance_srf_vjp(grid, tau, La, Ld, Xk, E0, nodes, s, gL), reps)}
    t = timed(torch, fns)
    for k, (ms, lo, hi) in t.items():
        say("  %-40s %10.4f ms per call (min %.4f, max %.4f of 5 medians over %d calls)" % (k, ms, lo, hi, fns[k][1]))
    say("  adjoint : forward, whole calls   %.2f   (all six outputs), %.2f (Tpix and frac only)"
        % (t["hsi_cube_srf_vjp, all six outputs"][0] / t["hsi_cube_srf (forward)"][0],
           t["hsi_cube_srf_vjp, Tpix and frac only"][0] / t["hsi_cube_srf (forward)"][0]))
    say("  adjoint : forward, pixel stage   %.2f   (rtx_srf_pixel_cube_vjp : rtx_srf_pixel_cube); g (%.1f MB) is read once by the pixel kernel "
        "and once per slice by the reduction: %d + %d times" % (t["  rtx_srf_pixel_cube_vjp, all"][0] / t["  rtx_srf_pixel_cube (forward)"][0],
                                                                4e-6 * nB * nPix, 1, n_slices))


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
    text = ["# python tools/time_cube_vjp.py --reps %d" % args.reps,
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
