"""Time the tangent-linear TUD (rtx_tud_jvp, engine.tud_jvp_from_od) at the reference caller's configuration (690-1410 cm^-1
at 0.0005, the 66-layer standard atmosphere, 9 sensor altitudes, returnOD, T + 3 species: DESIGN 4.9, the size
tools/time_vjp.py uses) against the route it replaces: the rtx_tud_jacobian launches over all layers plus a float64
contraction of each J block with the tangents on the device (the block widened to float64, then one matrix product).
Both work on the same device columns; the routes alternate, HIP events, medians.

Each timed step (all rows; rows = tau + L-up) runs in a child process of its own under a time limit; the parent never
opens the device and starts nothing more once a child fails or runs out of time.

    python tools/time_jvp.py [--reps 5] [--limit 240] [--out profiles/tud_jvp_time.txt]
"""
import argparse
import os
import subprocess
import sys

STEPS = (("all", "tau + L-up + Ld"), ("noLd", "tau + L-up"))


def child(step, reps):
    import numpy as np
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from radtxfr_amd import _lib, engine, synthetic
    from radtxfr_amd import radiative_transfer as rt

    alts = np.concatenate((np.array([200, 500, 1000, 2000, 5000, 10000, 20000, 50000]) * 0.3048 / 1e3, [100.0]))
    rows = ("tau", "La", "Ld") if step == "all" else ("tau", "La")

    def say(s):
        print(s, flush=True)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    lib = _lib.load()
    n_max = lib.rtx_tud_jvp_max_vectors()
    full = synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)
    sub = synthetic.subset_table(full, 690.0 - 12.0, 1410.0 + 12.0)
    sa = rt.StdAtmos
    a = dict(Zs=sa[:, 1], Ts=sa[:, 5].copy(), Ps=sa[:, 4], PLs=sa[:, 3], MFs_VAL=sa[:, 6:9] * 1e6, MFs_ID=np.array([1, 2, 3]))
    wrt = ("T", 1, 2, 3)
    tbl = rt._resolve_table(sub)
    X = rt._cached_axis(690.0, 1410.0, 0.0005)
    grid = engine.Grid(690.0, 1410.0, X.size)
    nZ, nL = alts.size, a["Ts"].size
    nrow = 2 * nZ + 1
    say("step %r: rows %s; %d points, %d layers, %d altitudes, returnOD, wrt %s" % (step, rows, grid.n, nL, nZ, wrt))
    say("device: %s; tangent vectors per rtx_tud_jvp call: up to %d" % (torch.cuda.get_device_name(0), n_max))
    # the shared stages, once: base state, T -+ h line-sums, species line-sums
    s = engine._jacobian_stages("time_jvp", tbl, grid, a["Zs"], a["Ts"], a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"], alts, 0.0,
                                30, True, wrt, None, 0.5, None)
    T, Z, layers, t_pos, tau, OD, ODp, ODm, K = s.T, s.Z, s.layers, s.t_pos, s.tau, s.OD, s.OD_plus, s.OD_minus, s.K
    rng = np.random.default_rng(1)
    V = rng.normal(size=(n_max, len(wrt), nL))
    V_dev = torch.as_tensor(V, device="cuda")
    common = dict(Altitudes=alts, theta_r=0.0, N_angle=30, returnOD=True, layers=layers, t_pos=t_pos)

    def jvp(n_vec):
        return engine.tud_jvp_from_od(OD, ODp, ODm, 0.5, K, tau, grid, T, Z, V[:n_vec], rows=rows, **common)

    def jacobian_kernels():
        engine.tud_jacobian_from_od(OD, ODp, ODm, 0.5, K, tau, grid, T, Z, on_block=lambda k0, k1, blk: None, **common)

    def jacobian_route(n_vec):
        out = torch.zeros((n_vec, nrow * grid.n), dtype=torch.float64, device="cuda")

        def on_block(k0, k1, blk):  # blk [n_wrt][k1 - k0][nrow][n]
            v = V_dev[:n_vec, :, k0:k1].reshape(n_vec, -1)
            out.addmm_(v, blk.reshape(len(wrt) * (k1 - k0), -1).double())

        engine.tud_jacobian_from_od(OD, ODp, ODm, 0.5, K, tau, grid, T, Z, on_block=on_block, **common)
        return out.view(n_vec, nrow, grid.n)

    routes = [
        ("tangent, 1 vector", lambda: jvp(1)),
        ("Jacobian launches + float64 contraction, 1 vector", lambda: jacobian_route(1)),
        ("tangent, %d vectors (one launch)" % n_max, lambda: jvp(n_max)),
        ("Jacobian launches + float64 contraction, %d vectors" % n_max, lambda: jacobian_route(n_max)),
        ("Jacobian kernel launches alone (J discarded)", jacobian_kernels),
    ]
    for _, fn in routes:  # warm-up: staging, allocator, code objects
        fn()
    torch.cuda.synchronize()
    ts = {name: [] for name, _ in routes}
    for _ in range(reps):  # alternating
        for name, fn in routes:
            ts[name].append(timed(fn)[0])
    say("medians over %d alternating runs [ms] (runs):" % reps)
    for name, _ in routes:
        say("  %-56s %8.2f   (%s)" % (name, np.median(ts[name]), ", ".join("%.2f" % t for t in ts[name])))
    # agreement of the two routes, in units of the bound the tests hold the tangent to against a stored J:
    # 2 TOL_L sum|v| max(|J|, 1e-3 rowmax, 1e-30) + 2^-24 |ref|
    got = jvp(1)
    want = jacobian_route(1)[0]
    S = torch.zeros((nrow, grid.n), dtype=torch.float64, device="cuda")

    def on_block(k0, k1, blk):
        b = blk.double().abs()
        den = torch.maximum(torch.maximum(b, 1e-3 * b.amax(dim=-1, keepdim=True)), torch.tensor(1e-30, device="cuda", dtype=torch.float64))
        S.add_(torch.einsum("wkrn,wk->rn", den, V_dev[0, :, k0:k1].abs()))

    engine.tud_jacobian_from_od(OD, ODp, ODm, 0.5, K, tau, grid, T, Z, on_block=on_block, block_bytes=1 << 29, **common)
    sl = {"tau": slice(0, nZ), "La": slice(nZ, 2 * nZ), "Ld": slice(2 * nZ, nrow)}
    for name in rows:
        g = got[name][0].double().reshape(-1, grid.n)
        bound = 2e-5 * S[sl[name]] + 2.0 ** -24 * want[sl[name]].abs()
        say("tangent %-3s against the contracted stored J: worst |difference| / bound = %.3g"
            % (name, ((g - want[sl[name]]).abs() / bound).max().item()))
    say("result: %.1f MB per vector; the stored J: %.1f GB"
        % (sum(nZ if r != "Ld" else 1 for r in rows) * grid.n * 4 / 1e6, len(wrt) * nL * nrow * grid.n * 4 / 1e9))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.reps)
        return 0
    text = []
    rc = 0
    for step, what in STEPS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", step, "--reps", str(args.reps)],
                               stdout=subprocess.PIPE, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired as e:
            print("step %r (%s): no result within %d s; stopping" % (step, what, args.limit))
            print(e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or ""))
            rc = 124
            break
        print(p.stdout, end="", flush=True)
        if p.returncode != 0:
            print("step %r (%s): exit status %d; stopping" % (step, what, p.returncode))
            rc = p.returncode
            break
        text.append(p.stdout)
    if args.out and rc == 0:
        with open(args.out, "w") as f:
            f.write("\n".join(t.rstrip("\n") for t in text) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
