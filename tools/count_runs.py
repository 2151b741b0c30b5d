#!/usr/bin/env python3
"""CPU-side census of the point-by-point entries that the nodal line-sum kernel drains on the C3 workload
(rtx_voigt_scatter.hip: nodal_tile, drain). Per layer, over every STRIDE-th tile, from cpu_ref.row_masks: the general
entries (64-byte, drained row by row) and the edge-only ones, and per general entry its near-zone rows and their runs of
consecutive rows, its window-edge rows, and its band rows -- wholly inside the window or cut by it, on the 6-term series
(y >= 6), on the per-row choice (1 <= y < 6) or of a y < 1 line. From those and the per-row / per-entry instruction counts
of the device assembly (PARENT and NEW below, counted in the listings that profiles/linesum_runs_isa.txt records) the
expected change of SQ_INSTS_SALU and SQ_INSTS_VALU per launch of voigt_nodal_kernel<false>. Pure NumPy; no GPU.

    python tools/count_runs.py [--stride 197] [--layers 0,8,16,24,31]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import cpu_ref
from radtxfr_amd import synthetic

ROWS, NEAR = cpu_ref.LS_ROWS, cpu_ref.LS_NEAR
TILE = 64 * ROWS
N = 5500000
# (SALU, VALU) wave-instructions of the drain, from the assembly of voigt_nodal_kernel<false> (s_waitcnt and s_nop not counted):
# per general entry (head: reads, v_readfirstlane, mask decode, loop guards), per entry with band rows on top of that (the
# flags, the run's bounds), and per row of each kind. A band row's body holds both the series and the Weideman path; the
# y >= 6 rows are counted with the series path alone, the 1 <= y < 6 rows with the whole body (an upper bound for both builds).
PARENT = dict(entry=(12, 5), band_entry=(3, 1), near=(6, 10), edge=(7, 13), band_in6=(25, 80), band_in=(36, 163), band_cut=(36, 163))
NEW = dict(entry=(13, 3), band_entry=(9, 2), near=(6, 10), edge=(7, 13), band_in6=(18, 74), band_in=(23, 155), band_cut=(40, 161))


def run_lengths(bits):
    """Lengths of the runs of consecutive set rows in a bool [rows] vector."""
    d = np.diff(np.r_[0, bits.astype(np.int8), 0])
    return np.nonzero(d == -1)[0] - np.nonzero(d == 1)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stride", type=int, default=197)
    ap.add_argument("--layers", default="all")
    args = ap.parse_args()
    layers = range(32) if args.layers == "all" else [int(v) for v in args.layers.split(",")]
    full = synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)
    atm = synthetic.c3_atmosphere(32)
    step = 5500.0 / (N - 1)
    nu = full["nu"]
    assert np.all(np.diff(nu) >= 0)
    keys = ("entries", "band_entries", "edge_only", "near_rows", "near_runs", "edge_rows", "band_in6", "band_in", "band_cut", "band_smally")
    tot = dict.fromkeys(keys, 0)
    hist = np.zeros(2 * NEAR + 2, dtype=np.int64)  # near-zone runs by length
    n_tl = 0
    for k in layers:
        T, p = atm["Ts"][k], atm["Ps"][k] / 101325.0
        P = cpu_ref.line_params(full, T, p)
        W = np.maximum(50 * P["Gamma0"], 50 * P["GammaD"])
        lo = np.clip(np.ceil((nu - W - 500.0) / step), 0, N).astype(np.int64)
        hi = np.clip(np.floor((nu + W - 500.0) / step) + 1, 0, N).astype(np.int64)
        i0 = np.rint((nu + P["Shift0"] - 500.0) / step).astype(np.int64)
        cte = np.sqrt(np.log(2)) / P["GammaD"]
        y = P["Gamma0"] * cte
        zw = np.where(y < 15, np.ceil((15 - y) / (step * cte)) + 2, 0).astype(np.int64)
        c = dict.fromkeys(keys, 0)
        nt = 0
        for t in range(100, (N + TILE - 1) // TILE, args.stride):
            ia, ib = t * TILE, min((t + 1) * TILE, N)
            r = np.nonzero((hi > ia) & (lo < ib))[0]
            if r.size == 0:
                continue
            idx = np.arange(r[0], r[-1] + 1)
            m = cpu_ref.row_masks(i0[idx], lo[idx], hi[idx], zw[idx], ia, ib - ia, rows=ROWS, near=NEAR)
            pp, ed, bd, inside = m["pp"], m["edge"], m["bd"], m["inside"]
            single = ~pp.any(1) & ~bd.any(1) & (ed.sum(1) == 1)
            re = np.argmax(ed, 1)
            left, right = m["part_l"] & (re == m["r_lo"]), m["part_r"] & (re == m["r_hi"] - 1)
            edge_only = single & (left != right)
            gen = (pp | ed | bd).any(1) & ~edge_only
            yy = y[idx]
            cut = bd & ~inside
            c["entries"] += int(gen.sum())
            c["band_entries"] += int((gen & bd.any(1)).sum())
            c["edge_only"] += int(edge_only.sum())
            c["near_rows"] += int(pp[gen].sum())
            c["edge_rows"] += int(ed[gen].sum())
            c["band_smally"] += int(bd[gen & (yy < 1)].sum())
            c["band_cut"] += int(cut[gen & (yy >= 1)].sum())
            c["band_in6"] += int((bd & ~cut)[gen & (yy >= 6)].sum())
            c["band_in"] += int((bd & ~cut)[gen & (yy >= 1) & (yy < 6)].sum())
            for row in pp[gen]:
                rl = run_lengths(row)
                c["near_runs"] += rl.size
                np.add.at(hist, np.minimum(rl, hist.size - 1), 1)
            nt += 1
        n_tl += nt
        for key in keys:
            tot[key] += c[key]
        print("layer %2d p = %.3f atm, per tile: entries %.1f (with band rows %.1f; edge-only %.1f)  near-zone rows %.1f in %.1f runs  "
              "edge rows %.1f  band rows inside y >= 6 %.1f, inside 1 <= y < 6 %.1f, cut %.1f, y < 1 %.1f" % (
                  k, p, c["entries"] / nt, c["band_entries"] / nt, c["edge_only"] / nt, c["near_rows"] / nt, c["near_runs"] / nt,
                  c["edge_rows"] / nt, c["band_in6"] / nt, c["band_in"] / nt, c["band_cut"] / nt, c["band_smally"] / nt), flush=True)
    per = {key: tot[key] / n_tl for key in keys}
    print("per (tile, layer): " + "  ".join("%s %.2f" % (key, per[key]) for key in keys))
    print("near-zone runs by length 1..%d+: %s" % (hist.size - 1, " ".join("%.1f %%" % (100.0 * h / max(hist.sum(), 1)) for h in hist[1:])))
    n_launch = ((N + TILE - 1) // TILE) * 32  # (tile, layer) pairs of one launch
    for name, j in (("SQ_INSTS_SALU", 0), ("SQ_INSTS_VALU", 1)):
        def total(tab):
            return (per["entries"] * tab["entry"][j] + per["band_entries"] * tab["band_entry"][j] + per["near_rows"] * tab["near"][j]
                    + per["edge_rows"] * tab["edge"][j] + per["band_in6"] * tab["band_in6"][j] + per["band_in"] * tab["band_in"][j]
                    + (per["band_cut"] + per["band_smally"]) * tab["band_cut"][j])
        a, b = total(PARENT), total(NEW)
        print("%s of the drain per (tile, layer): parent %.0f  new %.0f; expected change per launch %+.3g" % (name, a, b, (b - a) * n_launch))


if __name__ == "__main__":
    main()
