"""The tangent of the per-pixel HSI cube (sensor.hsi_cube_srf_jvp: srf_moments at the nodes -> rtx_srf_cube_tables ->
rtx_srf_pixel_cube -> rtx_srf_radiance_jvp at the nodes with [E | 0] -> rtx_srf_pixel_cube_jvp) next to its forward,
sensor.hsi_cube_srf, and next to the two forward calls a difference quotient takes per direction, on config C5's input:
256 x 256 pixels, Sensor.mako(resFactor=2)'s 256 bands, tau / La / Ld on the MAKO span of the C3 grid (570 000 wavenumbers,
755 - 1325 cm^-1), 8 nodes.

    python tools/time_cube_jvp.py [--reps 10] [--out profiles/cube_jvp_time.txt]

runs the two scenes below one after the other, each in a child process of its own under `timeout` (a step that faults or
hangs ends the run: nothing further is started on the device). A time is the median of 5 rounds, after a warm-up round, of
`reps` back-to-back calls between two device events, host side of the calls included; the functions timed together
alternate per round, so the tangent and the forward see the same machine.

  small   synthetic.synth_scene: mixtures of 2 out of 6 endmembers (the pixel kernel's table in LDS)
  end400  the same pixels' temperatures, mixtures of 3 out of 400 endmembers (table in global memory)

Whole calls are timed with 1, rtx_srf_pixel_cube_jvp_max_vectors() and twice that many vectors (the band tangent behind dL,
rtx_srf_radiance_jvp, takes 4 per call), the new entry alone with 1 and the maximum, by group of tangents.
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
    NV = lib.rtx_srf_pixel_cube_jvp_max_vectors()
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
    nB, nk, nEnd, (nPix, nMix), nX = len(s), len(Xk), E.shape[1], kidx.shape, grid.n
    say("%d bands; %d points; %d pixels, mixtures of %d out of %d endmembers on %d knots; %d nodes over [%g, %g] K; cube and d_cube %.1f MB "
        "each (per vector); table %d rows: %s in the pixel kernel; %d vectors per library call"
        % (nB, nX, nPix, nMix, nEnd, nk, Q, T_range[0], T_range[1], 4e-6 * nB * nPix, nEnd * Q, "LDS" if nEnd * Q <= 128 else "global memory", NV))
    rng = np.random.default_rng(9)
    rel = lambda x, nv: x[..., None] * f32(rng.uniform(-0.5, 0.5, tuple(x.shape) + (nv,)))
    tang = {nv: dict(d_tau=rel(tau, nv), d_La=rel(La, nv), d_Ld=rel(Ld, nv), d_endmembers=rel(E, nv), d_frac=rel(frac, nv),
                     d_Tpix=torch.as_tensor(rng.uniform(-2.0, 2.0, (nPix, nv)), device="cuda")) for nv in (1, NV, 2 * NV)}
    args = (grid, tau, La, Ld, Xk, E, kidx, frac, T, s)
    fwd = lambda: sensor.hsi_cube_srf(*args, n_nodes=Q, T_range=T_range)[1]
    jvp = lambda nv, keys: (lambda: sensor.hsi_cube_srf_jvp(*args, n_nodes=Q, T_range=T_range, **{k: tang[nv][k] for k in keys}))
    ALL, PIX = ("d_tau", "d_La", "d_Ld", "d_endmembers", "d_frac", "d_Tpix"), ("d_frac", "d_Tpix")
    nodes = sensor.srf_cube_nodes(T_range[0], T_range[1], Q)
    Xk_d = torch.as_tensor(np.asarray(Xk, dtype=np.float64), device="cuda")
    N, Cb, M, jr = sensor.srf_moments(grid, tau, La, Ld, Xk_d, nodes, s)
    tab = torch.empty((nEnd, Q, nB), dtype=torch.float32, device="cuda")
    cube = torch.empty((nB, nPix), dtype=torch.float32, device="cuda")
    d_cube = torch.empty((NV, nB, nPix), dtype=torch.float32, device="cuda")
    dL = f32(rng.uniform(-1.0, 1.0, (NV, Q, nB, nEnd + 1)))
    dF = tang[NV]["d_frac"].movedim(-1, 0).contiguous()
    dT = tang[NV]["d_Tpix"].movedim(-1, 0).contiguous()
    E0 = torch.cat([E, torch.zeros((nk, 1), dtype=torch.float32, device="cuda")], dim=1)
    dE0 = torch.cat([tang[NV]["d_endmembers"], torch.zeros((nk, 1, NV), dtype=torch.float32, device="cuda")], dim=1)
    T_host = np.ascontiguousarray(np.concatenate([nodes, T_range]))
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.rtx_srf_cube_tables(p(M), p(jr), nB, Q, nk, p(E), nEnd, p(tab), st))
    new_half = lambda a, b, c, nv: (lambda: _lib.check(lib.rtx_srf_pixel_cube_jvp(nB, Q, T_host.ctypes.data_as(C.c_void_p), p(N), p(tab), nEnd, nPix,
                                                                                  nMix, p(kidx), p(frac), p(T), p(a), p(b), p(c), nv, p(d_cube), st, 0)))
    new_half(dF, dT, dL, NV)()
    rows = {k: tang[NV][k] for k in ("d_tau", "d_La", "d_Ld")}
    fns = {"hsi_cube_srf (forward)": (fwd, reps),
           "two hsi_cube_srf calls (a difference quotient)": (lambda: (fwd(), fwd()), reps),
           "hsi_cube_srf_jvp, all groups, 1 vector": (jvp(1, ALL), reps),
           "hsi_cube_srf_jvp, all groups, %d vectors" % NV: (jvp(NV, ALL), reps),
           "hsi_cube_srf_jvp, all groups, %d vectors" % (2 * NV): (jvp(2 * NV, ALL), reps),
           "hsi_cube_srf_jvp, d_frac and d_Tpix, 1 vector": (jvp(1, PIX), reps),
           "hsi_cube_srf_jvp, d_frac and d_Tpix, %d vectors" % NV: (jvp(NV, PIX), reps),
           "  srf_moments (%d temperatures)" % Q: (lambda: sensor.srf_moments(grid, tau, La, Ld, Xk_d, nodes, s), reps),
           "  rtx_srf_pixel_cube (forward)": (lambda: _lib.check(lib.rtx_srf_pixel_cube(nB, Q, T_host.ctypes.data_as(C.c_void_p), p(N), p(Cb), p(tab),
                                                                                        nEnd, nPix, nMix, p(kidx), p(frac), p(T), p(cube), st)), reps),
           "  rtx_srf_pixel_cube_jvp, all groups, 1 vector": (new_half(dF, dT, dL, 1), reps),
           "  rtx_srf_pixel_cube_jvp, all groups, %d vectors" % NV: (new_half(dF, dT, dL, NV), reps),
           "  rtx_srf_pixel_cube_jvp, d_frac and d_Tpix, %d vectors" % NV: (new_half(dF, dT, None, NV), reps),
           "  rtx_srf_pixel_cube_jvp, dL only, %d vectors" % NV: (new_half(None, None, dL, NV), reps),
           "  band_radiance_srf_jvp at the nodes with [E | 0], %d vectors" % NV: (lambda: sensor.band_radiance_srf_jvp(grid, tau, La, Ld, Xk, E0, nodes, s,
                                                                                                                       d_emis=dE0, **rows), reps)}
    t = timed(torch, fns)
    for k, (ms, lo, hi) in t.items():
        say("  %-62s %10.4f ms per call (min %.4f, max %.4f of 5 medians over %d calls)" % (k, ms, lo, hi, fns[k][1]))
    one, two = t["hsi_cube_srf (forward)"][0], t["two hsi_cube_srf calls (a difference quotient)"][0]
    whole = lambda k: t["hsi_cube_srf_jvp, " + k][0]
    per = lambda n: whole("all groups, %d vectors" % n) / n
    say("  tangent : forward, whole calls        all groups %.2f (1 vector), %.2f per vector (%d vectors), %.2f per vector (%d: two library calls "
        "of the pixel stage, one vector group of the band tangent); d_frac and d_Tpix %.2f, %.2f per vector"
        % (whole("all groups, 1 vector") / one, per(NV) / one, NV, per(2 * NV) / one, 2 * NV,
           whole("d_frac and d_Tpix, 1 vector") / one, whole("d_frac and d_Tpix, %d vectors" % NV) / NV / one))
    say("  tangent : two forward calls           all groups %.2f (1 vector), %.2f per vector (%d vectors), %.2f per vector (%d); the tangent also "
        "returns the cube" % (whole("all groups, 1 vector") / two, per(NV) / two, NV, per(2 * NV) / two, 2 * NV))
    k1, kn = t["  rtx_srf_pixel_cube_jvp, all groups, 1 vector"][0], t["  rtx_srf_pixel_cube_jvp, all groups, %d vectors" % NV][0]
    say("  tangent : forward, pixel stage        %.2f (1 vector), %.2f per vector (%d vectors); d_cube written at %.0f GB/s (1 vector), %.0f GB/s (%d)"
        % (k1 / t["  rtx_srf_pixel_cube (forward)"][0], kn / NV / t["  rtx_srf_pixel_cube (forward)"][0], NV,
           4e-6 * nB * nPix / k1, 4e-6 * nB * nPix * NV / kn, NV))


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
    text = ["# python tools/time_cube_jvp.py --reps %d" % args.reps,
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
