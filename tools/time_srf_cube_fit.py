"""The per-pixel fit to a measured HSI cube (rtx_srf_pixel_cube_fit) next to a host loop over
rtx_srf_pixel_cube_normal and next to what the library offered per iteration before it, on config C5's scene: 256 x 256
pixels, mixtures of 2 out of 6 endmembers (made distinct per pixel: a repeated endmember has a singular H),
Sensor.mako(resFactor=2)'s bands, tau / La / Ld on the MAKO span of the C3 grid, 8 nodes over 273 - 301 K (temperatures
clipped into it). The measurement is rtx_srf_pixel_cube's own cube of the scene.

    python tools/time_srf_cube_fit.py [--reps 5] [--out profiles/cube_fit_time.txt]

runs the steps below one after the other, each in a child process of its own under `timeout` (a step that faults or hangs
ends the run: nothing further is started on the device). A time is the median of 5 rounds, after a warm-up round, of `reps`
back-to-back calls between two device events, host side of the calls included.

  fit      rtx_srf_pixel_cube_fit from the node scan, 30 trials (and the scan alone, max_iter = 0): ms per call, per trial
  normal   (i) a host loop over rtx_srf_pixel_cube_normal: per trial one call for the step at the current point, one for the
           trial point, and the accept rule in torch
  parent   (ii) what the parent commit offers per iteration: rtx_srf_pixel_cube, ceil((1 + nMix) / 2) calls of
           rtx_srf_pixel_cube_jvp (unit vectors in T and the fractions) and a torch contraction to H and grad
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
T_RANGE = (273.0, 301.0)
TRIALS = 30
STEPS = (("fit", 300), ("normal", 300), ("parent", 300))


def timed(torch, fn, n):
    """Median, min and max ms per call over 5 rounds of n calls, after a warm-up round."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts = []
    for _ in range(6):
        fn()
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(n):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]) / n)
    return float(np.median(ts[1:])), min(ts[1:]), max(ts[1:])


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
    k_h = np.array(sc["kidx"])
    k_h[:, 1] = np.where(k_h[:, 1] == k_h[:, 0], (k_h[:, 0] + 1) % 6, k_h[:, 1])
    E = f32(em[:, sc["end_idx"]]).contiguous()
    kidx, frac = torch.as_tensor(k_h, device="cuda"), f32(sc["frac"])
    T = torch.as_tensor(np.clip(sc["T"], *T_RANGE), device="cuda")
    s = sensor.Sensor.mako(X[0], X[-1], resFactor=2)
    nB, nk, nEnd, (nPix, nMix) = len(s), len(Xk), E.shape[1], kidx.shape
    nU = 1 + nMix
    nodes = sensor.srf_cube_nodes(T_RANGE[0], T_RANGE[1], Q)
    N, Cb, M, jr = sensor.srf_moments(grid, tau, La, Ld, torch.as_tensor(np.asarray(Xk, dtype=np.float64), device="cuda"), nodes, s)
    tab = torch.empty((nEnd, Q, nB), dtype=torch.float32, device="cuda")
    meas = torch.empty((nB, nPix), dtype=torch.float32, device="cuda")
    T_host = np.ascontiguousarray(np.concatenate([nodes, T_RANGE]))
    Tp = T_host.ctypes.data_as(C.c_void_p)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.rtx_srf_cube_tables(p(M), p(jr), nB, Q, nk, p(E), nEnd, p(tab), st))
    front = (nB, Q, Tp, p(N), p(Cb), p(tab), nEnd, nPix, nMix, p(kidx))
    _lib.check(lib.rtx_srf_pixel_cube(*front, p(frac), p(T), p(meas), st))
    say("%d bands (%d live); %d pixels, mixtures of %d out of %d endmembers; %d nodes over [%g, %g] K; table %d rows: %s"
        % (nB, int((N > 0).sum()), nPix, nMix, nEnd, Q, T_RANGE[0], T_RANGE[1], nEnd * Q, "LDS" if nEnd * Q <= 128 else "global memory"))
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
    cost, grad, hess, stp = f64(nPix), f64(nPix, nU), f64(nPix, nU * (nU + 1) // 2), f64(nPix, nU)
    line = lambda k, t, n: say("  %-64s %10.4f ms per call (min %.4f, max %.4f of 5 medians over %d calls)" % ((k,) + t + (n,)))
    if step == "fit":
        f_o, T_o = torch.empty_like(frac), torch.empty_like(T)
        n_iter, status = (torch.empty(nPix, dtype=torch.int32, device="cuda") for _ in range(2))
        run = lambda it: (lambda: _lib.check(lib.rtx_srf_pixel_cube_fit(*front, p(meas), None, p(f_o), p(T_o), it, 1e-3, 0.0, p(cost), p(n_iter),
                                                                       p(status), p(hess), st, 0)))
        t0, t30 = timed(torch, run(0), reps), timed(torch, run(TRIALS), reps)
        run(TRIALS)()
        torch.cuda.synchronize()
        ni = n_iter.cpu().numpy()
        line("rtx_srf_pixel_cube_fit, the scan alone (max_iter 0: %d evaluations)" % (2 * Q), t0, reps)
        line("rtx_srf_pixel_cube_fit, the scan and %d trials" % TRIALS, t30, reps)
        say("  per trial (the scan taken off): %.4f ms; per evaluation of the scan: %.4f ms; trials per pixel %d .. %d (mean %.1f); statuses %s; "
            "worst |T - truth| %.3g K, worst |f - truth| %.3g"
            % ((t30[0] - t0[0]) / max(int(ni.max()), 1), t0[0] / (2 * Q), ni.min(), ni.max(), ni.mean(), np.bincount(status.cpu().numpy()).tolist(),
               float((T_o - T).abs().max()), float((f_o - frac).abs().max())))
    elif step == "normal":
        T0 = torch.clamp(T + 2.0, max=T_RANGE[1])
        f0 = (frac * 0.8).contiguous()
        lam = torch.full((nPix,), 1e-3, dtype=torch.float64, device="cuda")
        nrm = lambda T_, f_, l_, g_, h_, s_: _lib.check(lib.rtx_srf_pixel_cube_normal(*front, p(f_), p(T_), p(meas), None, p(l_), p(cost), p(g_), p(h_),
                                                                                      p(s_), st, 0))
        line("rtx_srf_pixel_cube_normal, all outputs", timed(torch, lambda: nrm(T0, f0, lam, grad, hess, stp), reps), reps)
        line("rtx_srf_pixel_cube_normal, cost only", timed(torch, lambda: nrm(T0, f0, None, None, None, None), reps), reps)
        c_cur = f64(nPix)

        def trial(state):
            Tc, fc, lm = state
            nrm(Tc, fc, lm, None, None, stp)
            c_cur.copy_(cost)
            Tt = torch.clamp(Tc + stp[:, 0], min=T_RANGE[0], max=T_RANGE[1])
            ft = (fc.double() + stp[:, 1:]).float()
            nrm(Tt, ft, None, None, None, None)
            acc = cost < c_cur
            return (torch.where(acc, Tt, Tc), torch.where(acc[:, None], ft, fc),
                    torch.where(acc, torch.clamp(0.1 * lm, min=1e-12), torch.clamp(10.0 * lm, max=1e12)))

        def loop():
            state = (T0, f0, lam)
            for _ in range(TRIALS):
                state = trial(state)
        t = timed(torch, loop, max(reps // 2, 1))
        line("(i) host loop over rtx_srf_pixel_cube_normal, %d trials" % TRIALS, t, max(reps // 2, 1))
        say("  per trial: %.4f ms (two calls and the accept rule in torch)" % (t[0] / TRIALS))
    else:
        NV = lib.rtx_srf_pixel_cube_jvp_max_vectors()
        cube = torch.empty((nB, nPix), dtype=torch.float32, device="cuda")
        unit = torch.eye(nU, dtype=torch.float64, device="cuda")
        dT = unit[:, 0][:, None].expand(nU, nPix).contiguous()                                         # [nU][nPix]
        dF = unit[:, 1:].float()[:, None, :].expand(nU, nPix, nMix).contiguous()                       # [nU][nPix][nMix]
        J = torch.empty((nU, nB, nPix), dtype=torch.float32, device="cuda")
        live = (N > 0)

        def iteration():
            _lib.check(lib.rtx_srf_pixel_cube(*front, p(frac), p(T), p(cube), st))
            for v0 in range(0, nU, NV):
                v1 = min(v0 + NV, nU)
                _lib.check(lib.rtx_srf_pixel_cube_jvp(nB, Q, Tp, p(N), p(tab), nEnd, nPix, nMix, p(kidx), p(frac), p(T), p(dF[v0:v1]), p(dT[v0:v1]),
                                                      None, v1 - v0, p(J[v0:v1]), st, 0))
            Jl = J[:, live].double()
            r = (cube[live] - meas[live]).double()
            return torch.einsum("ibp,bp->pi", Jl, r), torch.einsum("ibp,jbp->pij", Jl, Jl), (r * r).sum(dim=0)
        calls = lambda: (_lib.check(lib.rtx_srf_pixel_cube(*front, p(frac), p(T), p(cube), st)),
                         [_lib.check(lib.rtx_srf_pixel_cube_jvp(nB, Q, Tp, p(N), p(tab), nEnd, nPix, nMix, p(kidx), p(frac), p(T), p(dF[v0:v0 + NV]),
                                                                p(dT[v0:v0 + NV]), None, min(NV, nU - v0), p(J[v0:v0 + NV]), st, 0)) for v0 in range(0, nU, NV)])
        t = timed(torch, iteration, reps)
        line("(ii) rtx_srf_pixel_cube + %d rtx_srf_pixel_cube_jvp + torch contraction" % ((nU + NV - 1) // NV), t, reps)
        line("  the library calls of (ii) alone", timed(torch, calls, reps), reps)
        say("  per iteration: %.4f ms, before any solve or accept rule" % t[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=[s for s, _ in STEPS])
    args = ap.parse_args()
    if args.step:
        child(args.step, args.reps)
        return
    import torch
    text = ["# python tools/time_srf_cube_fit.py --reps %d" % args.reps,
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
