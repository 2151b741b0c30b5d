"""Cases of the line-sum's done rows (rtx_voigt_sum_rows; rtx_voigt_scatter.hip: the instantiation for launches that carry
skip flags), and the NumPy restatement of what that instantiation does with them. Imported by tests/test_od_hide_host.py
(each case reaches what it names) and tests/test_gpu_od_hide.py (each case against rtx_voigt_sum's bits); no test in here.

Grids are two tiles and a ragged third, n = 2 * 1024 + 100 (rows 0 and 1 of the third tile, the second ragged). Two tables:

  base   33 lines, all but two 83 points apart at 1e-4 cm^-1 per point, seven widths, four layers (T, p below): layers 0-2 have no
         y < 1 line (the fp32 instantiation, the one that leaves done rows out), layer 3 has (the fp64 one, which only does
         not store them). Band runs of up to nine rows, near zones, window edges inside the tiles, partial, full and
         tile-level members.
  dense  a comb 0.01 cm^-1 apart at 1e-3 cm^-1 per point, two layers: under the hot-tile cut of 768 candidates, and both
         entry lists of a wave overflow.

A case: table, layers (how many of the table's), k_lo / k_hi, skip (bool per row of the grid or shard, padded to whole
tiles; None: a NULL pointer), shard (offset, n) or None."""
import functools

import numpy as np

import linesum_cases as LC
from oracle import cpu_ref

ROWS, TILE = cpu_ref.LS_ROWS, 64 * cpu_ref.LS_ROWS
N = 2 * TILE + 100
N_TILES = 3
GAMMAS = (0.04, 0.1, 0.15, 0.3, 0.52, 0.61, 1.6)


@functools.lru_cache(maxsize=None)
def table(name):
    """(HITRAN-format columns, grid tuple, T per layer, p per layer [atm])."""
    if name == "base":
        g = LC.grid(1000.0, 1e-4, N)
        gi = np.r_[-1200, -1100, np.arange(-200, N + 200, 83)]  # the first two reach tile 0 alone, and only in layer 0
        gam = np.array([GAMMAS[i % len(GAMMAS)] for i in range(gi.size)])
        return LC.table(LC.at(g, gi), gam), g, np.array([296.0, 290.0, 300.0, 296.0]), np.array([0.1, 0.05, 0.3, 0.01])
    assert name == "dense"
    g = LC.grid(1000.0, 1e-3, N)
    return LC.table(np.arange(997.0, 1005.2, 0.01) + 2.5e-4, 0.05), g, np.array([296.0, 296.0]), np.array([1.0, 0.1])


def rows_of(n):
    """Rows of a grid or shard of n points, padded to whole tiles."""
    return -(-n // TILE) * ROWS


def pattern(per_tile):
    """skip flags of the whole grid from one list of done rows per tile."""
    s = np.zeros(N_TILES * ROWS, dtype=bool)
    for t, rows in enumerate(per_tile):
        s[t * ROWS + np.asarray(list(rows), dtype=np.int64)] = True
    return s


def _but(r):
    return [q for q in range(ROWS) if q != r]


ALT = list(range(1, ROWS, 2))
CASES = {
    # no byte set, through the pointer (the instantiation with done rows, none done but the rows past the grid's end) and
    # without one (the plain instantiation): rtx_voigt_sum everywhere
    "none": dict(table="base", layers=4, skip=pattern([[], [], []])),
    "null": dict(table="base", layers=3, skip=None),
    "live_0": dict(table="base", layers=3, skip=pattern([_but(0)] * 3)),
    "live_7": dict(table="base", layers=3, skip=pattern([_but(7)] * 3)),
    "live_15": dict(table="base", layers=3, skip=pattern([_but(15)] * 3)),
    # no block of two or four wholly done; holes inside band runs and near zones
    "alt_rows": dict(table="base", layers=4, skip=pattern([ALT, [r - 1 for r in ALT], ALT])),
    "alt_blocks": dict(table="base", layers=2, skip=pattern([[4, 5, 6, 7, 12, 13, 14, 15], [0, 1, 2, 3, 8, 9, 10, 11], []])),
    # a done prefix and a done suffix that end inside a block of four, and inside a pair
    "prefix_suffix": dict(table="base", layers=3, skip=pattern([range(0, 6), range(9, 16), [0]])),
    "both_ends": dict(table="base", layers=1, skip=pattern([list(range(0, 3)) + list(range(13, 16)), range(0, 7), []])),
    "whole_tile": dict(table="base", layers=3, skip=pattern([range(16), [], range(16)])),
    # the ragged tile: its second (ragged) row done, the bytes of the rows past the grid's end set or not
    "ragged": dict(table="base", layers=2, skip=pattern([[], [3], [1, 5, 9]])),
    "ragged_live": dict(table="base", layers=2, skip=pattern([[2], [], [0, 2, 3]])),
    "layer_range": dict(table="base", layers=4, k_lo=1, k_hi=3, skip=pattern([ALT, range(0, 6), [1]])),
    "smally_alone": dict(table="base", layers=4, k_lo=3, k_hi=4, skip=pattern([range(0, 6), ALT, [0]])),
    # the second tile and the ragged third as a shard, with only the lines in reach of it
    "shard": dict(table="base", layers=2, shard=(TILE, N - TILE), skip=pattern([ALT, [1]])[:2 * ROWS]),
    # both lists of a wave overflow, dead entries before the overflow
    "dense": dict(table="dense", layers=2, skip=pattern([ALT, list(range(0, 5)) + [8, 9], [1]])),
}
for _c in CASES.values():
    _c.setdefault("k_lo", 0)
    _c.setdefault("k_hi", _c["layers"])
    _c.setdefault("shard", None)


def case_grid(c):
    """The grid tuple the case's call runs on."""
    _, g, _, _ = table(c["table"])
    if c["shard"] is None:
        return g
    return (g[0], g[1], g[2], c["shard"][0], c["shard"][1])


def case_table(c):
    """The line table of the call: a shard takes only the lines whose window reaches it in some layer."""
    tbl, g, T, p = table(c["table"])
    if c["shard"] is None:
        return tbl
    gs = case_grid(c)
    keep = np.zeros(np.asarray(tbl["nu"]).size, dtype=bool)
    for k in range(c["layers"]):
        R = cpu_ref.linesum_records(tbl, gs, float(T[k]), float(p[k]))
        keep[R["order"][R["hi"] > R["lo"]]] = True
    assert 0 < keep.sum() < keep.size, "the shard drops no line: the case proves nothing"
    return {key: np.asarray(v)[keep] for key, v in tbl.items()}


def done_mask(c):
    """bool [tiles][ROWS]: what the kernel treats as done -- the skip flags, and the rows past the grid's end."""
    n = case_grid(c)[4]
    nt = -(-n // TILE)
    skip = np.zeros(nt * ROWS, dtype=bool) if c["skip"] is None else np.asarray(c["skip"], dtype=bool).copy()
    assert skip.size == nt * ROWS
    skip[-(-n // 64):] = True
    return skip.reshape(nt, ROWS)


def live_points(c):
    """bool [n]: points of rows that are summed."""
    n = case_grid(c)[4]
    skip = np.zeros(rows_of(n), dtype=bool) if c["skip"] is None else np.asarray(c["skip"], dtype=bool)
    return ~np.repeat(skip, 64)[:n]


def _bits(M):
    return (M.astype(np.int64) << np.arange(ROWS)).sum(1)


def _trim(bd, done):
    """The band run trimmed to its first and last live row (bool [lines][ROWS])."""
    lv = bd & ~done[None, :]
    r = np.arange(ROWS)[None, :]
    first = np.where(lv.any(1), np.argmax(lv, 1), ROWS)[:, None]
    last = np.where(lv.any(1), ROWS - 1 - np.argmax(lv[:, ::-1], 1), -1)[:, None]
    return (r >= first) & (r <= last)


def restate(c):
    """What the kernels do with the case, per (layer of [k_lo, k_hi), tile with a live row): a list of dicts with
      layer, tile, smally, done (bool [ROWS]), far / pp / ed / bd (bool [candidates][ROWS], cpu_ref.row_masks), tile_level,
      full, partial, edge_only, entry (bool [candidates]), edge_row, and per wave w of LS_NW:
      lists[w] = {"edge": live, "entry": live}: one bool per candidate of the wave that emits into the list, in order, True
      where the entry is stored -- the fill level counts all of them, the drain walks the stored ones.
    Candidates are the canonical range of the tile (first to last line whose window meets it), candidate i of wave i % LS_NW."""
    tbl, _, T, p = table(c["table"])
    tbl = case_table(c)
    g = case_grid(c)
    n = g[4]
    D = done_mask(c)
    out = []
    for k in range(c["k_lo"], c["k_hi"]):
        R = cpu_ref.linesum_records(tbl, g, float(T[k]), float(p[k]))
        i0, lo, hi, zw = R["i0"], R["lo"], R["hi"], R["zw"]
        live = hi > lo
        smally = bool(np.any((zw > 0) & (R["y"] < 1.0)))
        for t, ia in enumerate(range(0, n, TILE)):
            nt = min(TILE, n - ia)
            done = D[t]
            reach = live & (hi > ia) & (lo < ia + nt)
            if done.all() or not reach.any():
                continue
            idx = np.nonzero(reach)[0]
            sl = np.arange(idx[0], idx[-1] + 1)
            assert sl.size <= cpu_ref.LS_SPLIT_MIN, "a hot tile: the subset launch refuses such tables"
            m = cpu_ref.row_masks(i0[sl], lo[sl], hi[sl], zw[sl], ia, nt)
            far, pp, ed, bd = m["far"], m["pp"], m["edge"], m["bd"]
            fb, pb, eb, bb = _bits(far), _bits(pp), _bits(ed), _bits(bd)
            allr = (1 << ROWS) - 1
            is_t = (fb == allr) & ((ia - i0[sl] >= cpu_ref.LS_TILE_DIST) | (i0[sl] - (ia + TILE - 1) >= cpu_ref.LS_TILE_DIST))
            single = (pb == 0) & (bb == 0) & (eb != 0) & ((eb & (eb - 1)) == 0)
            re = np.where(single, np.argmax(ed, 1), 0)
            left, right = m["part_l"] & (re == m["r_lo"]), m["part_r"] & (re == m["r_hi"] - 1)
            edge_only = single & (left != right)
            entry = ~edge_only & ((pb | eb | bb) != 0)
            live_edge = edge_only & ~done[re]
            live_entry = entry & ((pp | ed | bd) & ~done[None, :]).any(1)
            lists = []
            for w in range(cpu_ref.LS_NW):
                mine = np.arange(sl.size) % cpu_ref.LS_NW == w
                lists.append({"edge": live_edge[mine & edge_only], "entry": live_entry[mine & entry]})
            out.append(dict(layer=k, tile=t, smally=smally, done=done, far=far, pp=pp, ed=ed, bd=bd, bd_trim=_trim(bd, done) & bd,
                            inside=m["inside"], tile_level=is_t, full=(fb == allr) & ~is_t, partial=(fb != 0) & (fb != allr),
                            edge_only=edge_only, entry=entry, edge_row=re, lists=lists, y=R["y"][sl]))
    return out


def overflow(live, cap):
    """A list's life in one wave: (how often its counted fill level reaches the capacity, whether the stored fill level was
    below the counted one at the first of those drains)."""
    return live.size // cap, bool(live.size >= cap and not live[:cap].all())
