#!/usr/bin/env python3
"""CPU-side census of the nodal line-sum kernel's row-level groups on the C3 workload (rtx_voigt_scatter.hip: nodal_tile).
Per layer, over every STRIDE-th tile: the kernel's own deal of a tile's candidates (first to last line whose window
reaches it, table order; candidate c -> wave c % 2, round c // 128), the tile-level / full / partial members of each wave
and round (cpu_ref.row_masks), and the groups of 8 that serve them -- with the two classes always apart, and with the
kernel's rule: the full members go through the partial pass whenever ceil((nF + nP) / 8) < ceil(nF / 8) + ceil(nP / 8).
From the groups, the row-level wave-instructions: a full group 112 VALU, a partial (or merged) one 144; LDS per group = the
pulls (ds_bpermute), with and without the pull of ub that forming xb = ub a + c on the candidate lane saves, plus one
ds_permute per pass. Pure NumPy on the oracle's line parameters; no GPU.

    python tools/count_groups.py [--stride 197] [--layers 0,8,16,24,31]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import cpu_ref
from radtxfr_amd import synthetic

ROWS, NEAR, NW, TILE_DIST = cpu_ref.LS_ROWS, cpu_ref.LS_NEAR, cpu_ref.LS_NW, cpu_ref.LS_TILE_DIST
TILE = 64 * ROWS
N = 5500000
VALU_FULL, VALU_PART = 112, 144  # per group of 8: 16 rows x 7 (full) / x 9 (partial: + v_bfe_i32, v_and_b32)
PULL_TILE, PULL_FULL, PULL_PART = 8, 8, 9  # ds_bpermute per group with ub pulled: slot + a c b1 b0 Ay Ay0 ub (+ row mask)


def ceil8(n):
    return -(-n // 8)


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
    tot = dict(g_apart=0, g_rule=0, g_tile=0, valu_apart=0, valu_rule=0, lds_apart=0, lds_rule=0, lds_rule_xb=0, lds_tile=0,
               lds_tile_xb=0, rounds=0, merged_rounds=0)
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
        c = dict(T=0, F=0, P=0, g_tile=0, g_apart=0, g_rule=0, rounds=0, merged=0)
        nt = 0
        for t in range(100, (N + TILE - 1) // TILE, args.stride):
            ia, ib = t * TILE, min((t + 1) * TILE, N)
            r = np.nonzero((hi > ia) & (lo < ib))[0]
            if r.size == 0:
                continue
            idx = np.arange(r[0], r[-1] + 1)
            m = cpu_ref.row_masks(i0[idx], lo[idx], hi[idx], zw[idx], ia, ib - ia, rows=ROWS, near=NEAR)
            far = m["far"]
            is_full = far.all(1)
            is_t = is_full & ((ia - i0[idx] >= TILE_DIST) | (i0[idx] - (ia + TILE - 1) >= TILE_DIST)) if ib - ia == TILE else np.zeros_like(is_full)
            is_f, is_p = is_full & ~is_t, far.any(1) & ~is_full
            for w in range(NW):
                sel = np.arange(w, idx.size, NW)
                for b in range(0, sel.size, 64):
                    s = sel[b:b + 64]
                    nT, nF, nP = int(is_t[s].sum()), int(is_f[s].sum()), int(is_p[s].sum())
                    gT, gF, gP, gM = ceil8(nT), ceil8(nF), ceil8(nP), ceil8(nF + nP)
                    merged = gM < gF + gP
                    c["T"] += nT; c["F"] += nF; c["P"] += nP; c["rounds"] += 1; c["merged"] += merged
                    c["g_tile"] += gT; c["g_apart"] += gF + gP; c["g_rule"] += gM if merged else gF + gP
                    tot["valu_apart"] += gF * VALU_FULL + gP * VALU_PART
                    tot["lds_apart"] += gF * PULL_FULL + gP * PULL_PART + (gF > 0) + (gP > 0)
                    tot["lds_tile"] += gT * PULL_TILE + (gT > 0)
                    tot["lds_tile_xb"] += gT * (PULL_TILE - 1) + (gT > 0)
                    if merged:
                        tot["valu_rule"] += gM * VALU_PART
                        tot["lds_rule"] += gM * PULL_PART + 1
                        tot["lds_rule_xb"] += gM * (PULL_PART - 1) + 1
                    else:
                        tot["valu_rule"] += gF * VALU_FULL + gP * VALU_PART
                        tot["lds_rule"] += gF * PULL_FULL + gP * PULL_PART + (gF > 0) + (gP > 0)
                        tot["lds_rule_xb"] += gF * (PULL_FULL - 1) + gP * (PULL_PART - 1) + (gF > 0) + (gP > 0)
            nt += 1
        for a, b in (("g_apart", "g_apart"), ("g_rule", "g_rule"), ("g_tile", "g_tile"), ("rounds", "rounds"), ("merged_rounds", "merged")):
            tot[a] += c[b]
        print("layer %2d p = %.3f atm, per tile: wave rounds %.2f (merged %.2f)  members tile %.1f full %.1f partial %.1f | per wave round: "
              "full %.1f partial %.1f | groups per tile: tile level %.2f, row level apart %.2f, with the rule %.2f" % (
                  k, p, c["rounds"] / nt, c["merged"] / nt, c["T"] / nt, c["F"] / nt, c["P"] / nt, c["F"] / c["rounds"], c["P"] / c["rounds"],
                  c["g_tile"] / nt, c["g_apart"] / nt, c["g_rule"] / nt), flush=True)
    print("row-level groups, rule / apart: %.3f   (wave rounds that merge: %.1f %%)" % (tot["g_rule"] / tot["g_apart"], 100.0 * tot["merged_rounds"] / tot["rounds"]))
    print("row-level VALU, rule / apart: %.3f" % (tot["valu_rule"] / tot["valu_apart"]))
    print("row-level LDS (pulls + permutes), rule / apart: %.3f; rule and xb / apart: %.3f" % (tot["lds_rule"] / tot["lds_apart"], tot["lds_rule_xb"] / tot["lds_apart"]))
    print("tile-level LDS, xb / ub pulled: %.3f" % (tot["lds_tile_xb"] / max(tot["lds_tile"], 1)))


if __name__ == "__main__":
    main()
