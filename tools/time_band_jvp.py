"""Time the sensor stage's tangent (rtx_srf_radiance_jvp, sensor.band_radiance_srf_jvp) at the size of DESIGN
4.17's caller: 1.44 M points (690 - 1410 cm^-1 at 0.0005), Sensor.mako's 128 bands, 721 emissivity knots 1 cm^-1 apart, one
surface temperature, nE = 1 and 2000. tau / La / Ld are smooth synthetic spectra (the kernels' time depends on the shapes,
not on the values); all five input groups move.

    python tools/time_band_jvp.py [--reps 5] [--out profiles/band_jvp_time.txt]

runs one measurement per nE, each in a child process of its own under `timeout` (a step that faults or hangs ends the run:
nothing further is started on the device). Routes, interleaved, medians of --reps runs between two HIP events after a
warm-up round, host side of the calls included:

  forward              sensor.band_radiance_srf_fused (rtx_srf_moments + rtx_band_mix)
  central difference   what one direction cost before: two forward passes
  jvp call, n vectors  sensor.band_radiance_srf_jvp: the forward pass (it supplies L, N, M and jrange) and the tangent
  tangent, n vectors   rtx_srf_radiance_jvp alone, on the moments of a forward pass made beforehand
"""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

XMIN, XMAX, DV, TS0 = 690.0, 1410.0, 0.0005, 300.0
STEPS = (("1", 300), ("2000", 300))


def child(nE, reps):
    import torch
    from radtxfr_amd import _lib, engine, sensor
    from radtxfr_amd import radiative_transfer as rt
    lib = _lib.load()
    say = lambda s: print(s, flush=True)
    X = rt._cached_axis(XMIN, XMAX, DV)
    grid = engine.Grid(XMIN, XMAX, X.size)
    s = sensor.Sensor.mako(X[0], X[-1])
    Xk = np.arange(XMIN, XMAX + 0.5, 1.0)
    nB, nk, nX, NV = len(s), Xk.size, grid.n, lib.rtx_srf_radiance_jvp_max_vectors()
    say("%d points, %d bands, %d emissivity knots, nE = %d, 1 surface temperature; vectors per call: up to %d" % (nX, nB, nk, nE, NV))
    f32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float32), device="cuda")
    tau, La, Ld = f32(0.5 + 0.45 * np.sin(X / 13.0)), f32(2.0 + np.cos(X / 29.0)), f32(4.0 + 2.0 * np.sin(X / 7.0))
    rng = np.random.default_rng(1)
    E = f32(rng.uniform(0.6, 1.0, (nk, nE)))
    rows = [f32(rng.normal(size=(NV, nX)) * 0.01) for _ in range(3)]  # [n_vec][nX], as rtx_tud_jvp writes them
    dTs = rng.normal(size=NV)
    dE = f32(rng.normal(size=(nk, nE, NV)) * 0.01)
    Xk_d = torch.as_tensor(Xk, device="cuda")
    N, _, M, jr = sensor.srf_moments(grid, tau, La, Ld, Xk_d, [TS0], s)
    kx, kr = s.on_device(tau.device)
    dE_v = dE.movedim(-1, 0).contiguous()
    out = torch.empty((NV, 1, nB, nE), dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    Ts_h = np.array([TS0])

    def raw(nv):
        _lib.check(lib.rtx_srf_radiance_jvp(grid.byref(), p(tau), p(Ld), p(rows[0]), p(rows[1]), p(rows[2]), nX, Ts_h.ctypes.data_as(C.c_void_p),
                                            np.ascontiguousarray(dTs[:nv]).ctypes.data_as(C.c_void_p), 1, p(Xk_d), nk, nB,
                                            s.knot_start.ctypes.data_as(C.c_void_p), p(kx), p(kr), p(N), p(M), p(jr), p(E), p(dE_v), nE, nv,
                                            p(out), C.c_void_p(torch.cuda.current_stream().cuda_stream)))

    fwd = lambda: sensor.band_radiance_srf_fused(grid, tau, La, Ld, Xk, E, TS0, s)
    jvp = lambda nv: sensor.band_radiance_srf_jvp(grid, tau, La, Ld, Xk, E, TS0, s, d_tau=rows[0][:nv].T, d_La=rows[1][:nv].T,
                                                  d_Ld=rows[2][:nv].T, d_Ts=dTs[:nv], d_emis=dE[..., :nv])
    routes = [("forward", fwd), ("central difference: two forward passes", lambda: (fwd(), fwd())),
              ("jvp call, 1 vector (forward included)", lambda: jvp(1)), ("jvp call, %d vectors (forward included)" % NV, lambda: jvp(NV)),
              ("tangent alone, 1 vector", lambda: raw(1)), ("tangent alone, %d vectors" % NV, lambda: raw(NV))]
    for _, fn in routes:  # warm-up: workspaces, allocator
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts = {name: [] for name, _ in routes}
    for _ in range(reps):  # interleaved
        for name, fn in routes:
            ev[0].record()
            fn()
            ev[1].record()
            ev[1].synchronize()
            ts[name].append(ev[0].elapsed_time(ev[1]))
    med = {name: float(np.median(v)) for name, v in ts.items()}
    for name, _ in routes:
        say("  %-44s %9.3f ms   (%s)" % (name, med[name], ", ".join("%.3f" % t for t in ts[name])))
    t1, tn, f = med["tangent alone, 1 vector"], med["tangent alone, %d vectors" % NV], med["forward"]
    say("  tangent alone / forward: %.2f (1 vector), %.2f (%d vectors); a further vector: %.3f ms" % (t1 / f, tn / f, NV, (tn - t1) / (NV - 1)))
    say("  jvp call / central difference: %.2f (1 vector), %.2f per vector at %d vectors"
        % (med["jvp call, 1 vector (forward included)"] / med["central difference: two forward passes"],
           med["jvp call, %d vectors (forward included)" % NV] / (NV * med["central difference: two forward passes"]), NV))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=[s for s, _ in STEPS])
    args = ap.parse_args()
    if args.step:
        child(int(args.step), args.reps)
        return
    import torch
    text = ["# python tools/time_band_jvp.py --reps %d" % args.reps,
            "# device: %s, torch %s" % (torch.cuda.get_device_name(0) if torch.cuda.is_available() else "none", torch.__version__)]
    print("\n".join(text), flush=True)
    for step, limit in STEPS:
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--reps",
                            str(args.reps)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        block = "\n[nE = %s]\n%s" % (step, r.stdout.rstrip())
        print(block, flush=True)
        text.append(block)
        if r.returncode != 0:
            text.append("step nE = %s ended with status %d: stopping" % (step, r.returncode))
            print(text[-1], flush=True)
            break
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(text) + "\n")
    sys.exit(0 if r.returncode == 0 else 1)


if __name__ == "__main__":
    main()
