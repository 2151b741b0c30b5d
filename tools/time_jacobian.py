"""Time rt.compute_TUD_jacobian at the reference caller's configuration (Generate_LWIR_TUD.py: 690-1410 cm^-1 at 0.0005,
the 66-layer standard atmosphere, 9 sensor altitudes, returnOD, reduced to 0.25 cm^-1), split into its stages, against
compute_TUD_batch over the caller's 1 + 3 x 66 JacIn atmospheres with the same reduce.

    python tools/time_jacobian.py [--reps 3] [--out profiles/r4_time_jacobian.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from radtxfr_amd import _lib, engine, synthetic  # noqa: E402
from radtxfr_amd import radiative_transfer as rt  # noqa: E402

ALTS = np.concatenate((np.array([200, 500, 1000, 2000, 5000, 10000, 20000, 50000]) * 0.3048 / 1e3, [100.0]))


def jac_in(X, rel_step):
    """JacIn(X, relStep, rel=True) of the caller (Generate_LWIR_TUD.py:55-65), restated: row ii has X[ii] + relStep max|X|."""
    out = np.tile(X, (X.shape[-1], 1))
    out[np.arange(X.size), np.arange(X.size)] += rel_step * np.max(np.abs(out))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.load()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    full = synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)
    sub = synthetic.subset_table(full, 690.0 - 12.0, 1410.0 + 12.0)
    sa = rt.StdAtmos
    a = dict(Zs=sa[:, 1], Ts=sa[:, 5].copy(), Ps=sa[:, 4], PLs=sa[:, 3], MFs_VAL=sa[:, 6:9] * 1e6, MFs_ID=np.array([1, 2, 3]))
    kw = dict(DVOUT=0.0005, line_table=sub, Altitudes=ALTS, returnOD=True, **a)
    red = dict(dX=0.25)
    wrt = ("T", 1, 2, 3)
    tbl = rt._resolve_table(sub)
    X = rt._cached_axis(690.0, 1410.0, 0.0005)
    grid = engine.Grid(690.0, 1410.0, X.size)
    say("caller configuration: %d points, 66 layers, 9 altitudes, returnOD, wrt %s, reduce dX = 0.25 (N = 4, hanning)"
        % (grid.n, wrt))
    say("device: %s" % torch.cuda.get_device_name(0))

    # ---- stages, by events on the stream (engine.tud_jacobian's mark hook; the reduce of each block after its kernel) ----
    def staged():
        ev = [("start", torch.cuda.Event(enable_timing=True))]
        ev[0][1].record()

        def mark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev.append((name, e))

        def on_block(k0, k1, blk):
            engine.reduce_resolution_cached(blk.view(-1, grid.n), float(X[0]), grid.step, grid.n, 0.25)
            mark("reduce")

        out = engine.tud_jacobian(tbl, grid, a["Zs"], a["Ts"], a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"], Altitudes=ALTS,
                                  returnOD=True, wrt=wrt, on_block=on_block, mark=mark)
        rows = torch.cat([out[0], out[1], out[2][None, :]])
        engine.reduce_resolution_cached(rows, float(X[0]), grid.step, grid.n, 0.25)
        mark("reduce")
        torch.cuda.synchronize()
        acc = {}
        for (_, e0), (name, e1) in zip(ev, ev[1:]):
            acc[name] = acc.get(name, 0.0) + e0.elapsed_time(e1)
        return acc

    staged()  # warm-up: plans, reduce plan, allocator
    res = [staged() for _ in range(args.reps)]
    med = {k: float(np.median([r[k] for r in res])) for k in res[0]}
    n_wrt, nrow = len(wrt), 2 * ALTS.size + 1
    jbytes = n_wrt * 66 * nrow * grid.n * 4
    say("stage medians over %d runs [ms]:" % args.reps)
    say("  base line-sum + TUD         %8.2f" % med["base"])
    say("  T -+ h line-sums (2)        %8.2f" % med["T"])
    say("  species line-sums (%d)       %8.2f" % (3, med["species"]))
    # bytes the kernel loads, from its loop structure (rtx_tud_jac.hip: chunks of 8 requested layers per launch, each
    # sweeping the whole column bottom-up, then the stream groups of 8 top-down from n_down - 1 to the chunk's lowest layer)
    n_down = int((a["Zs"] <= ALTS[-1]).sum())
    n_groups = (30 - 1 + 7) // 8
    nb = max(1, min(66, engine.JAC_BLOCK_BYTES // (n_wrt * nrow * grid.n * 4)))
    loads = 0
    for b0 in range(0, 66, nb):
        blk = list(range(b0, min(b0 + nb, 66)))
        for c0 in range(0, len(blk), 8):
            ch = blk[c0:c0 + 8]
            loads += 66 + n_groups * (n_down - min(ch)) + len(ch) * (2 + (n_wrt - 1))  # sweep, streams, dOD (T: 2 loads)
    rbytes = loads * grid.n * 4
    tb = (jbytes + rbytes) / med["jacobian"] / 1e9
    say("  Jacobian kernel             %8.2f   (%.2f GB written + %.2f GB read: %.2f TB/s, %.0f %% of the 8 TB/s peak;"
        " written alone %.2f TB/s)" % (med["jacobian"], jbytes / 1e9, rbytes / 1e9, tb, 100.0 * tb / 8.0,
                                        jbytes / med["jacobian"] / 1e9))
    say("  reduce (%d + %d rows)      %8.2f" % (n_wrt * 66 * nrow, nrow, med["reduce"]))
    say("  device total                %8.2f" % sum(med.values()))

    # ---- the public call, end to end (host results included) ----
    ts = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rt.compute_TUD_jacobian(690.0, 1410.0, wrt=wrt, reduce=red, **kw)
        ts.append(1e3 * (time.perf_counter() - t0))
    say("rt.compute_TUD_jacobian end to end: median %.1f ms (runs %s)" % (np.median(ts), ", ".join("%.1f" % t for t in ts)))
    torch.cuda.reset_peak_memory_stats()
    rt.compute_TUD_jacobian(690.0, 1410.0, wrt=wrt, reduce=red, **kw)
    say("  peak torch-allocated device memory: %.2f GiB" % (torch.cuda.max_memory_allocated() / 2 ** 30))

    # ---- the caller's way: 199 atmospheres (mean profile, then T, H2O, O3 one layer at a time, relStep 0.001) ----
    T0, M0 = a["Ts"], a["MFs_VAL"]
    TJ = np.vstack([T0, jac_in(T0, 0.001), np.tile(T0, (132, 1))])
    HJ = np.vstack([M0[:, 0], np.tile(M0[:, 0], (66, 1)), jac_in(M0[:, 0], 0.001), np.tile(M0[:, 0], (66, 1))])
    OJ = np.vstack([M0[:, 2], np.tile(M0[:, 2], (132, 1)), jac_in(M0[:, 2], 0.001)])
    atms = [dict(Ts=TJ[j], MFs_VAL=np.column_stack([HJ[j], M0[:, 1], OJ[j]])) for j in range(TJ.shape[0])]
    assert len(atms) == 199
    ts = []
    for _ in range(max(1, args.reps - 1)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rt.compute_TUD_batch(690.0, 1410.0, atms, reduce=red, **kw)
        ts.append(1e3 * (time.perf_counter() - t0))
    say("rt.compute_TUD_batch over the 199 JacIn atmospheres, same reduce: median %.1f ms (runs %s)"
        % (np.median(ts), ", ".join("%.1f" % t for t in ts)))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
