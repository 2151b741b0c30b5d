"""The bound-constrained per-pixel fit (rtx_srf_pixel_cube_fit_box) next to the unconstrained fit
(rtx_srf_pixel_cube_fit) on the same data in the same process, interleaved: config C5's scene as
tools/time_srf_cube_fit.py sets it up (256 x 256 pixels, mixtures of 2 out of 6 endmembers made distinct, 8 nodes over
[273, 301] K, the MAKO bands), here with one fraction of every second pixel set to 0 (the row renormalised) and Gaussian
noise of 1e-3 of each band's largest radiance on the cube.

    python tools/time_srf_cube_fit_box.py [--reps 5] [--out profiles/cube_fit_box_time.txt]

Each line is the median over 5 rounds (after a warm-up round) of a round's mean time per call over `reps` calls, with the
smallest and largest of the 5 round means; a round times the four launches one after the other (fit scan, fit 30 trials,
fit_box scan, fit_box 30 trials), so both fits see the same clocks. Per trial = (the call with 30 trials - the scan alone) /
the largest trial count of a pixel, as tools/time_srf_cube_fit.py reports it."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q = 8
T_RANGE = (273.0, 301.0)
TRIALS = 30
NOISE = 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from radtxfr_amd import _lib, engine, sensor, synthetic
    lib = _lib.load()
    text = ["# python tools/time_srf_cube_fit_box.py --reps %d" % args.reps,
            "# device: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__)]

    def say(s):
        print(s, flush=True)
        text.append(s)
    full = engine.Grid(500.0, 6000.0, 5500000)
    i0, i1 = int((755.0 - 500.0) / full.step), int((1325.0 - 500.0) / full.step)
    grid = full.shard(i0, i1 - i0)
    X = grid.axis()
    f32 = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float32), device="cuda")
    tau, La, Ld = f32(0.5 + 0.45 * np.sin(X / 13.0)), f32(2.0 + np.cos(X / 29.0)), f32(4.0 + 2.0 * np.sin(X / 7.0))
    Xk, em = synthetic.synth_emissivities(n_emis=2000)
    sc = synthetic.synth_scene()
    k_h = np.array(sc["kidx"])
    k_h[:, 1] = np.where(k_h[:, 1] == k_h[:, 0], (k_h[:, 0] + 1) % 6, k_h[:, 1])
    f_h = np.array(sc["frac"], dtype=np.float64)
    rng = np.random.default_rng(11)
    drop = rng.random(f_h.shape[0]) < 0.5
    f_h[np.flatnonzero(drop), rng.integers(0, f_h.shape[1], f_h.shape[0])[drop]] = 0.0
    f_h = f_h / f_h.sum(axis=1, keepdims=True)
    E = f32(em[:, sc["end_idx"]]).contiguous()
    kidx, frac = torch.as_tensor(k_h, device="cuda"), f32(f_h)
    T = torch.as_tensor(np.clip(sc["T"], *T_RANGE), device="cuda")
    s = sensor.Sensor.mako(X[0], X[-1], resFactor=2)
    nB, nk, nEnd, (nPix, nMix) = len(s), len(Xk), E.shape[1], kidx.shape
    nU = 1 + nMix
    nodes = sensor.srf_cube_nodes(T_RANGE[0], T_RANGE[1], Q)
    N, Cb, M, jr = sensor.srf_moments(grid, tau, La, Ld, torch.as_tensor(np.asarray(Xk, dtype=np.float64), device="cuda"), nodes, s)
    tab = torch.empty((nEnd, Q, nB), dtype=torch.float32, device="cuda")
    clean = torch.empty((nB, nPix), dtype=torch.float32, device="cuda")
    T_host = np.ascontiguousarray(np.concatenate([nodes, T_RANGE]))
    Tp = T_host.ctypes.data_as(C.c_void_p)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.rtx_srf_cube_tables(p(M), p(jr), nB, Q, nk, p(E), nEnd, p(tab), st))
    front = (nB, Q, Tp, p(N), p(Cb), p(tab), nEnd, nPix, nMix, p(kidx))
    _lib.check(lib.rtx_srf_pixel_cube(*front, p(frac), p(T), p(clean), st))
    torch.cuda.synchronize()
    live = (N > 0)
    top = torch.where(live, torch.nan_to_num(clean.abs(), nan=0.0).amax(dim=1), torch.zeros_like(N))
    noise = torch.as_tensor(rng.standard_normal((nB, nPix)).astype(np.float32), device="cuda")
    meas = torch.where(live[:, None], clean + NOISE * top[:, None] * noise, clean).contiguous()
    say("%d bands (%d live); %d pixels, mixtures of %d out of %d endmembers, %d pixels with a fraction of 0; noise %g of a band's largest radiance; "
        "%d nodes over [%g, %g] K; table %d rows: %s" % (nB, int(live.sum()), nPix, nMix, nEnd, int(drop.sum()), NOISE, Q, T_RANGE[0], T_RANGE[1],
                                                         nEnd * Q, "LDS" if nEnd * Q <= 128 else "global memory"))
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
    out = {}
    for name in ("fit", "box"):
        out[name] = dict(f=torch.empty_like(frac), T=torch.empty_like(T), cost=f64(nPix), hess=f64(nPix, nU * (nU + 1) // 2), grad=f64(nPix, nU),
                         n_iter=torch.empty(nPix, dtype=torch.int32, device="cuda"), status=torch.empty(nPix, dtype=torch.int32, device="cuda"),
                         active=torch.empty(nPix, dtype=torch.int32, device="cuda"))

    def run(name, it):
        o = out[name]
        if name == "fit":
            _lib.check(lib.rtx_srf_pixel_cube_fit(*front, p(meas), None, p(o["f"]), p(o["T"]), it, 1e-3, 0.0, p(o["cost"]), p(o["n_iter"]),
                                                  p(o["status"]), p(o["hess"]), st, 0))
        else:
            _lib.check(lib.rtx_srf_pixel_cube_fit_box(*front, p(meas), None, p(o["f"]), p(o["T"]), it, 1e-3, 0.0, p(o["cost"]), p(o["n_iter"]),
                                                      p(o["status"]), p(o["hess"]), st, 0, 0.0, p(o["grad"]), p(o["active"])))
    cases = [("fit", 0), ("fit", TRIALS), ("box", 0), ("box", TRIALS)]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts = {c: [] for c in cases}
    for _ in range(6):
        for c in cases:  # interleaved: every round times the four launches one after the other
            run(*c)
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(args.reps):
                run(*c)
            ev[1].record()
            torch.cuda.synchronize()
            ts[c].append(ev[0].elapsed_time(ev[1]) / args.reps)
    med = {c: (float(np.median(v[1:])), min(v[1:]), max(v[1:])) for c, v in ts.items()}
    names = dict(fit="rtx_srf_pixel_cube_fit", box="rtx_srf_pixel_cube_fit_box")
    for name in ("fit", "box"):
        run(name, TRIALS)
        torch.cuda.synchronize()
        o = out[name]
        ni = o["n_iter"].cpu().numpy()
        t0, t30 = med[(name, 0)], med[(name, TRIALS)]
        fmt = "  %-52s %10.4f ms per call (median of 5 round means of %d calls each; smallest %.4f, largest %.4f)"
        say(fmt % (names[name] + ", the scan alone (%d evaluations)" % (2 * Q), t0[0], args.reps, t0[1], t0[2]))
        say(fmt % (names[name] + ", the scan and %d trials" % TRIALS, t30[0], args.reps, t30[1], t30[2]))
        say("    per trial (the scan taken off): %.4f ms; per evaluation of the scan: %.4f ms; trials per pixel %d .. %d (mean %.1f); statuses %s; "
            "pixels with a negative fraction %d, lowest fraction %.3g; mean cost %.6g"
            % ((t30[0] - t0[0]) / max(int(ni.max()), 1), t0[0] / (2 * Q), ni.min(), ni.max(), ni.mean(), np.bincount(o["status"].cpu().numpy()).tolist(),
               int((o["f"] < 0).any(dim=1).sum()), float(o["f"].min()), float(o["cost"].mean())))
    act = out["box"]["active"].cpu().numpy()
    say("  rtx_srf_pixel_cube_fit_box: pixels with an active fraction %d, with T active %d" % (int(((act >> 1) != 0).sum()), int((act & 1).sum())))
    per = lambda name: (med[(name, TRIALS)][0] - med[(name, 0)][0]) / max(int(out[name]["n_iter"].max()), 1)
    say("  per trial, box / unconstrained: %.3f; per evaluation of the scan, box / unconstrained: %.3f" % (per("box") / per("fit"), med[("box", 0)][0] / med[("fit", 0)][0]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
