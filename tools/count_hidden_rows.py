#!/usr/bin/env python3
"""CPU-side census of what the done rows of partly hidden tiles are worth to the line-sum of the middle layers
(rtx_voigt_scatter.hip: the instantiation for launches that carry done flags), on the C3 column.

Windows of whole line-sum tiles spread over the bench grid, as tools/count_tud_layers.py spreads its own: the oracle's
optical depths (cpu_ref.layer_od, float32) and count_tud_layers.census say which 64-point waves the early TUD launch
finishes (done = skips and loads no middle chunk); cpu_ref.linesum_records and cpu_ref.row_masks restate row_geom and
the classification of every candidate of a tile, per layer of the middle launch [4, k_top - 8). Printed:

  - the done-row patterns of the partly hidden tiles: share of rows done, runs, prefix / suffix, aligned blocks of 2 / 4 / 8;
  - the share of row-level evaluations (16 per member and group, whatever the member's mask) that a test per row, per pair,
    per block of four or a live hull [r_lo, r_hi) removes;
  - per (partly hidden tile, layer): general entries, edge-only entries and their rows, and the share that is dead (no live
    row: not stored), the near-zone and window-edge rows that leave the stored masks, and the band rows that trimming the run
    to its first and last live row removes (and those a row-by-row mask would remove on top).

Pure NumPy; no GPU.

    python tools/count_hidden_rows.py [--windows 20] [--tiles 4]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import count_tud_layers as ctl  # noqa: E402
from oracle import cpu_ref  # noqa: E402
from radtxfr_amd import synthetic  # noqa: E402

ROWS = cpu_ref.LS_ROWS
TILE = 64 * ROWS
N, NL = ctl.N, ctl.NL
STAGE, SCAN, BOTTOM = ctl.STAGE, 12, ctl.BOTTOM


def runs(bits):
    d = np.diff(np.r_[0, bits.astype(np.int8), 0])
    return np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]


def trim(bd, done):
    lv = bd & ~done[None, :]
    r = np.arange(ROWS)[None, :]
    first = np.where(lv.any(1), np.argmax(lv, 1), ROWS)[:, None]
    last = np.where(lv.any(1), ROWS - 1 - np.argmax(lv[:, ::-1], 1), -1)[:, None]
    return bd & (r >= first) & (r <= last)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--tiles", type=int, default=4)
    args = ap.parse_args()
    full = synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)
    atm = synthetic.c3_atmosphere(NL)
    cnt0 = int(np.sum(np.asarray(atm["Zs"]) <= 500))
    k_top = (cnt0 - 1) // STAGE * STAGE
    mid = range(BOTTOM, k_top - (SCAN - STAGE))  # the layers of launch B
    pts = args.tiles * TILE
    Xg = np.linspace(500.0, 6000.0, N)
    starts = (np.linspace(0, N - pts, args.windows).astype(np.int64) // TILE) * TILE
    pat = dict(tiles=0, whole=0, part=0, part_done=0, runs=0, by_runs={}, done_rows=0, ends=0, blk={2: 0, 4: 0, 8: 0}, hull=0)
    keys = ("entries", "dead_entries", "edges", "dead_edges", "pp_rows", "pp_dead", "ed_rows", "ed_dead", "bd_rows", "bd_trimmed", "bd_done",
            "members", "tile_layers")
    tot = dict.fromkeys(keys, 0)
    for i0 in starts:
        X = Xg[i0:i0 + pts]
        sub = synthetic.subset_table(full, X[0] - 12.0, X[-1] + 12.0)
        OD = np.stack([cpu_ref.layer_od(sub, X, atm["Ts"][k], atm["Ps"][k], atm["PLs"][k], atm["MFs_VAL"][k], atm["MFs_ID"])
                       for k in range(NL)], axis=1).astype(np.float32)
        B = cpu_ref.planckian(X, np.asarray(atm["Ts"], dtype=np.float64))
        c = ctl.census(OD, B, cnt0, cnt0, SCAN, BOTTOM)
        done_w = (c["skip"] & (c["summed"] == 0)).reshape(args.tiles, ROWS)
        part = []
        for t in range(args.tiles):
            d = done_w[t]
            pat["tiles"] += 1
            if d.all():
                pat["whole"] += 1
                continue
            if not d.any():
                continue
            part.append(t)
            a, b = runs(d)
            pat["part"] += 1
            pat["part_done"] += int(d.sum())
            pat["runs"] += a.size
            pat["by_runs"][a.size] = pat["by_runs"].get(a.size, 0) + 1
            pat["ends"] += int(sum(e - s for s, e in zip(a, b) if s == 0 or e == ROWS))
            for G in (2, 4, 8):
                pat["blk"][G] += G * int(d.reshape(-1, G).all(1).sum())
            lv = np.nonzero(~d)[0]
            pat["hull"] += int(lv[0] + (ROWS - 1 - lv[-1]))
        print("window %7.1f cm^-1: done rows per tile %s" % (X[0], [int(done_w[t].sum()) for t in range(args.tiles)]), flush=True)
        if not part:
            continue
        g = (500.0, 6000.0, N, int(i0), pts)
        for k in mid:
            R = cpu_ref.linesum_records(sub, g, float(atm["Ts"][k]), float(atm["Ps"][k]) / 101325.0)
            lo, hi = R["lo"], R["hi"]
            for t in part:
                ia, d = t * TILE, done_w[t]
                reach = np.nonzero((hi > lo) & (hi > ia) & (lo < ia + TILE))[0]
                if reach.size == 0:
                    continue
                sl = np.arange(reach[0], reach[-1] + 1)
                m = cpu_ref.row_masks(R["i0"][sl], lo[sl], hi[sl], R["zw"][sl], ia, TILE)
                pp, ed, bd, far = m["pp"], m["edge"], m["bd"], m["far"]
                single = ~pp.any(1) & ~bd.any(1) & (ed.sum(1) == 1)
                re = np.argmax(ed, 1)
                edge_only = single & ((m["part_l"] & (re == m["r_lo"])) != (m["part_r"] & (re == m["r_hi"] - 1)))
                gen = (pp | ed | bd).any(1) & ~edge_only
                live = ((pp | ed | bd) & ~d[None, :]).any(1)
                tot["tile_layers"] += 1
                tot["members"] += int((far.any(1) & ~far.all(1)).sum() + far.all(1).sum())
                tot["entries"] += int(gen.sum())
                tot["dead_entries"] += int((gen & ~live).sum())
                tot["edges"] += int(edge_only.sum())
                tot["dead_edges"] += int((edge_only & d[re]).sum())
                tot["pp_rows"] += int(pp[gen].sum())
                tot["pp_dead"] += int((pp[gen] & d[None, :]).sum())
                tot["ed_rows"] += int(ed[gen].sum())
                tot["ed_dead"] += int((ed[gen] & d[None, :]).sum())
                tot["bd_rows"] += int(bd[gen].sum())
                tot["bd_trimmed"] += int(bd[gen].sum() - trim(bd[gen], d).sum())
                tot["bd_done"] += int((bd[gen] & d[None, :]).sum())
    p = pat
    print("\n%d tiles in %d windows: %.1f %% wholly done, %.1f %% partly; of the partly done tiles' rows %.1f %% are done"
          % (p["tiles"], args.windows, 100.0 * p["whole"] / p["tiles"], 100.0 * p["part"] / p["tiles"],
             100.0 * p["part_done"] / max(ROWS * p["part"], 1)))
    if p["part"]:
        print("done rows of a partly done tile lie in %.2f runs on average (tiles by number of runs: %s); %.1f %% of the done rows are a "
              "prefix or a suffix of the tile" % (p["runs"] / p["part"], dict(sorted(p["by_runs"].items())), 100.0 * p["ends"] / p["part_done"]))
        print("share of the done rows in wholly done aligned blocks of 2 / 4 / 8 rows: %s"
              % " / ".join("%.1f %%" % (100.0 * p["blk"][G] / p["part_done"]) for G in (2, 4, 8)))
        allrows = ROWS * p["part"]
        print("row-level evaluations of the partly done tiles removed by a test per row %.1f %%, per pair %.1f %%, per block of four "
              "%.1f %%, per block of eight %.1f %%, by the live hull %.1f %%"
              % (100.0 * p["part_done"] / allrows, 100.0 * p["blk"][2] / allrows, 100.0 * p["blk"][4] / allrows, 100.0 * p["blk"][8] / allrows,
                 100.0 * p["hull"] / allrows))
    n = max(tot["tile_layers"], 1)
    pc = lambda a, b: 100.0 * tot[a] / max(tot[b], 1)
    print("per (partly done tile, layer of the middle launch), %d of them: row-level members %.1f; general entries %.1f, dead %.1f %%; "
          "edge-only entries %.1f, dead %.1f %%" % (tot["tile_layers"], tot["members"] / n, tot["entries"] / n, pc("dead_entries", "entries"),
                                                    tot["edges"] / n, pc("dead_edges", "edges")))
    print("rows of the general entries: near-zone %.1f, done %.1f %%; window-edge %.1f, done %.1f %%; band %.1f, removed by trimming the "
          "run %.1f %% (done, what a row-by-row mask would remove: %.1f %%)"
          % (tot["pp_rows"] / n, pc("pp_dead", "pp_rows"), tot["ed_rows"] / n, pc("ed_dead", "ed_rows"), tot["bd_rows"] / n,
             pc("bd_trimmed", "bd_rows"), pc("bd_done", "bd_rows")))


if __name__ == "__main__":
    main()
