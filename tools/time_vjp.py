"""Time the adjoint of the TUD Jacobian (rtx_tud_vjp, engine.tud_vjp_from_od) at the reference caller's configuration
(690-1410 cm^-1 at 0.0005, the 66-layer standard atmosphere, 9 sensor altitudes, returnOD, T + 3 species: DESIGN 4.9)
against the route it replaces: the rtx_tud_jacobian launches plus a float64 contraction of each J block with the cotangent
in torch (the block widened to float64, then one matrix-vector product). Both work on the same device columns; the
routes are interleaved, HIP events, medians.

    python tools/time_vjp.py [--reps 5] [--out profiles/tud_vjp_time.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from radtxfr_amd import _lib, engine, synthetic  # noqa: E402
from radtxfr_amd import radiative_transfer as rt  # noqa: E402

ALTS = np.concatenate((np.array([200, 500, 1000, 2000, 5000, 10000, 20000, 50000]) * 0.3048 / 1e3, [100.0]))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.load()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    full = synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)
    sub = synthetic.subset_table(full, 690.0 - 12.0, 1410.0 + 12.0)
    sa = rt.StdAtmos
    a = dict(Zs=sa[:, 1], Ts=sa[:, 5].copy(), Ps=sa[:, 4], PLs=sa[:, 3], MFs_VAL=sa[:, 6:9] * 1e6, MFs_ID=np.array([1, 2, 3]))
    wrt = ("T", 1, 2, 3)
    tbl = rt._resolve_table(sub)
    X = rt._cached_axis(690.0, 1410.0, 0.0005)
    grid = engine.Grid(690.0, 1410.0, X.size)
    nZ, nL = ALTS.size, a["Ts"].size
    say("caller configuration: %d points, %d layers, %d altitudes, returnOD, wrt %s" % (grid.n, nL, nZ, wrt))
    say("device: %s; cotangent vectors per rtx_tud_vjp call: up to %d" % (torch.cuda.get_device_name(0), lib.rtx_tud_vjp_max_vectors()))

    # the shared stages, once: base state, T -+ h line-sums, species line-sums
    s = engine._jacobian_stages("time_vjp", tbl, grid, a["Zs"], a["Ts"], a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"], ALTS, 0.0,
                                30, True, wrt, None, 0.5, None)
    T, Z, layers, t_pos, tau, OD, ODp, ODm, K = s.T, s.Z, s.layers, s.t_pos, s.tau, s.OD, s.OD_plus, s.OD_minus, s.K
    gen = torch.Generator(device="cuda").manual_seed(1)
    G = torch.randn((4, 2 * nZ + 1, grid.n), generator=gen, device="cuda", dtype=torch.float32)
    common = dict(Altitudes=ALTS, theta_r=0.0, N_angle=30, returnOD=True, layers=layers, t_pos=t_pos)

    def vjp(groups, n_vec=1):
        g = G[:n_vec]
        return engine.tud_vjp_from_od(OD, ODp, ODm, 0.5, K, tau, grid, T, Z, G_tau=g[:, :nZ] if groups[0] else None,
                                      G_Lu=g[:, nZ:2 * nZ] if groups[1] else None, G_Ld=g[:, 2 * nZ] if groups[2] else None,
                                      **common)

    G64 = G[0].double()

    def jacobian_kernels():
        engine.tud_jacobian_from_od(OD, ODp, ODm, 0.5, K, tau, grid, T, Z, on_block=lambda k0, k1, blk: None, **common)

    def jacobian_route():
        out = torch.empty((len(wrt), nL), dtype=torch.float64, device="cuda")

        def on_block(k0, k1, blk):
            out[:, k0:k1] = (blk.reshape(len(wrt) * (k1 - k0), -1).double() @ G64.reshape(-1)).view(len(wrt), k1 - k0)

        engine.tud_jacobian_from_od(OD, ODp, ODm, 0.5, K, tau, grid, T, Z, on_block=on_block, **common)
        return out

    routes = [
        ("adjoint (i)   tau + L-up + Ld, 1 vector", lambda: vjp((True, True, True))),
        ("adjoint (ii)  L-up only, 1 vector", lambda: vjp((False, True, False))),
        ("adjoint (iii) tau only, 1 vector", lambda: vjp((True, False, False))),
        ("adjoint       tau + L-up + Ld, 4 vectors", lambda: vjp((True, True, True), 4)),
        ("adjoint       L-up only, 4 vectors", lambda: vjp((False, True, False), 4)),
        ("Jacobian kernel launches alone (J discarded)", jacobian_kernels),
        ("Jacobian launches + float64 matrix-vector product per block", jacobian_route),
    ]
    for _, fn in routes:  # warm-up: scratch, allocator
        fn()
    torch.cuda.synchronize()
    ts = {name: [] for name, _ in routes}
    for _ in range(args.reps):  # interleaved
        for name, fn in routes:
            ts[name].append(timed(fn)[0])
    say("medians over %d interleaved runs [ms] (runs):" % args.reps)
    for name, _ in routes:
        say("  %-52s %8.2f   (%s)" % (name, np.median(ts[name]), ", ".join("%.2f" % t for t in ts[name])))
    # agreement of the two routes, in units of the bound the tests hold the adjoint to: 4 2^-24 sum|G J|
    got = vjp((True, True, True))[0]
    want = jacobian_route()
    scale = torch.zeros_like(want)

    def on_block(k0, k1, blk):
        scale[:, k0:k1] = (blk.reshape(len(wrt) * (k1 - k0), -1).double().abs() @ G64.abs().reshape(-1)).view(len(wrt), k1 - k0)

    engine.tud_jacobian_from_od(OD, ODp, ODm, 0.5, K, tau, grid, T, Z, on_block=on_block, **common)
    seen = scale > 0  # (an ozone column without lines in the table: J, and the adjoint, are exactly 0 there)
    ratio = ((got - want).abs()[seen] / (4.0 * 2.0 ** -24 * scale[seen])).max().item()
    say("adjoint (i) against the contracted stored J: worst |difference| / (4 2^-24 sum|G J|) = %.3g over %d of %d elements"
        " (the others: J = 0 throughout, adjoint %s)" % (ratio, int(seen.sum()), seen.numel(),
                                                          "0.0 too" if not got[~seen].any() else "not 0"))
    say("scratch of the adjoint: %.1f MB per vector (one float64 per 256-point workgroup and output element)"
        % ((grid.n + 255) // 256 * len(wrt) * nL * 8 / 1e6))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
