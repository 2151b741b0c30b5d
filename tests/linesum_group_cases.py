"""Line tables that put a chosen number of full and partial row-level members into ONE wave's round of the nodal line-sum
kernel (rtx_voigt_scatter.hip: nodal_tile), so that the rule that sends the full members through the partial pass is taken
both ways. Imported by the GPU test (tests/test_gpu_linesum_groups.py: every case against the fp64 oracle, shards, the
layout of the final sums) and by the host test (tests/test_linesum_groups_host.py: each case reaches the (nF, nP, merged)
it names, from cpu_ref.row_masks), so the two cannot drift apart.

The rule, per wave and round of 64 candidates: with nF full members that are not at tile level and nP partial members, the
full members are served by the partial pass (row mask ALL_ROWS) iff ceil((nF + nP) / 8) < ceil(nF / 8) + ceil(nP / 8).

Geometry (tests/linesum_cases.py: a_row_level): 9 x 1024 points at step 1e-3, the members act on tile 4. Air width 0.07
cm^-1/atm at 1 atm gives windows of 3500 points. A full member has its centre 300 points outside the tile (window over all
of it, near zone outside); a partial member 3000 points outside (its window edge cuts the tile: the rows before the cut are
far rows, the cut row an edge-only entry). The candidates of a tile are dealt to the kernel's two waves by parity, in
table order from the first line that reaches the tile: every member is followed, one point on, by a filler -- width 0.002
cm^-1/atm, a window of 100 points that ends short of the tile, y = 1.15 so that the layer stays on the plain
instantiation -- which puts all members on even candidates: wave 0 sees them, wave 1 sees fillers only. Two narrow lines
near tiles 0 and 8 are in no tile-4 range: a shard of tile 4 leaves them out of its table."""
import numpy as np

from oracle import cpu_ref

import linesum_cases as LC

TILE = 64 * cpu_ref.LS_ROWS
TARGET = 4                      # the tile the members act on
IA, IB = TARGET * TILE, (TARGET + 1) * TILE
GRID = LC.grid(1000.0, 1e-3, 9 * TILE)
G_MEMBER, G_FILLER, G_OMEGA = 0.07, 0.002, 0.02


def merge_rule(nF, nP):
    """The kernel's decision, restated: one pass over both classes iff it needs fewer groups of 8."""
    return -(-(nF + nP) // 8) < -(-nF // 8) + -(-nP // 8)


def _left(nF, nP):
    """Ascending centres (grid indices) left of the tile: partial members, then full members."""
    return sorted(IA - 3000 - 6 * k for k in range(nP)) + sorted(IA - 300 - 4 * k for k in range(nF))


def _right(nF, nP):
    """Ascending centres right of the tile: full members, then partial members."""
    return sorted(IB - 1 + 300 + 4 * k for k in range(nF)) + sorted(IB - 1 + 3000 + 6 * k for k in range(nP))


def _with_fillers(members, pad=()):
    """(centres, widths): every member followed by a filler one point on; `pad`: further filler centres."""
    gi = [v for m in members for v in (m, m + 1)] + list(pad)
    ga = [v for _ in members for v in (G_MEMBER, G_FILLER)] + [G_FILLER] * len(pad)
    gi += [300, 8 * TILE + 700]  # reach tiles 0 and 8 only
    ga += [G_FILLER, G_FILLER]
    o = np.argsort(gi, kind="stable")
    gi, ga = np.asarray(gi)[o], np.asarray(ga)[o]
    assert np.all(np.diff(gi) > 0)
    return gi, ga


def _case(gi, ga, expect, ow=0.0, tile_members=0):
    c = LC._case(LC.table(LC.at(GRID, gi), ga), GRID, 296.0, 1.0, ow=ow)
    c["expect"] = dict(expect)          # (wave, round) -> (nF, nP, merged) in tile TARGET; every other round: (0, 0, False)
    c["tile_members"] = tile_members    # tile-level members per wave and round named in expect
    return c


def _cases():
    C = {}
    # (1, 7) merged into one full group; (1, 8) not (two groups either way); (9, 7) merged into two groups; (7, 2) and (3, 6)
    # no saving, two groups either way, not merged; (3, 12) merged, 15 members: a ragged last group; one class alone
    for nF, nP in ((1, 7), (1, 8), (9, 7), (7, 2), (3, 6), (3, 12), (5, 0), (0, 5)):
        gi, ga = _with_fillers(_left(nF, nP))
        C["g_%d_%d" % (nF, nP)] = _case(gi, ga, {(0, 0): (nF, nP, merge_rule(nF, nP))})
    # two rounds: (2, 5) left of the tile, merged; fillers up to candidate 128; (1, 8) right of the tile, not merged
    left, right = _left(2, 5), _right(1, 8)
    pad = [IA - 290 + k for k in range(64 * cpu_ref.LS_NW - 2 * len(left))]
    gi, ga = _with_fillers(left + right, pad)
    C["g_two_rounds"] = _case(gi, ga, {(0, 0): (2, 5, True), (0, 1): (1, 8, False)})
    # tile-level members in the same round: OmegaWing 3 cm^-1 sets every window (3000 points; width 0.02: 50 Gamma0 = 1),
    # centres >= 512 points outside are tile level. Every line reaches the tile under this OmegaWing, so there is no
    # filler: each member has a twin of its class one point on, and BOTH waves see (nT, nF, nP) = (3, 1, 7), merged
    mem = sorted(IA - 2500 - 6 * k for k in range(7)) + sorted(IA - 600 - 8 * k for k in range(3)) + [IA - 300]
    gi = np.asarray([v for m in mem for v in (m, m + 1)])
    C["g_tile_level"] = _case(gi, np.full(gi.size, G_OMEGA), {(0, 0): (1, 7, True), (1, 0): (1, 7, True)}, ow=3.0, tile_members=3)
    return C


CASES = _cases()
NAMES = sorted(CASES)
SHARD_CASES = ("g_3_12", "g_7_2")  # one merged, one not


def round_census(case, tile=TARGET, layer=0):
    """{(wave, round): (nT, nF, nP, merged)} of `tile`: the classes of the kernel's candidates (first to last line that
    reaches the tile, table order; candidate c -> wave c % LS_NW, round c // (64 LS_NW)), from cpu_ref.row_masks."""
    g = case["grid"]
    R = cpu_ref.linesum_records(case["tbl"], g, float(case["T"][layer]), float(case["p"][layer]), case["ow"], case["hw"])
    i0, lo, hi, zw = R["i0"], R["lo"], R["hi"], R["zw"]
    ia = tile * TILE
    nt = min(TILE, g[4] - ia)
    idx = np.nonzero((hi > lo) & (hi > ia) & (lo < ia + nt))[0]
    first, last = int(idx[0]), int(idx[-1]) + 1
    assert last - first <= cpu_ref.LS_SPLIT_MIN, "a hot tile: cut into parts"
    sl = np.arange(first, last)
    m = cpu_ref.row_masks(i0[sl], lo[sl], hi[sl], zw[sl], ia, nt)
    far = m["far"]
    full = far.all(1)
    is_t = full & ((ia - i0[sl] >= cpu_ref.LS_TILE_DIST) | (i0[sl] - (ia + TILE - 1) >= cpu_ref.LS_TILE_DIST))
    is_f, is_p = full & ~is_t, far.any(1) & ~full
    c = np.arange(sl.size)
    wave, rnd = c % cpu_ref.LS_NW, c // (64 * cpu_ref.LS_NW)
    out = {}
    for w in range(cpu_ref.LS_NW):
        for r in range(int(rnd.max()) + 1):
            s = (wave == w) & (rnd == r)
            nT, nF, nP = int(is_t[s].sum()), int(is_f[s].sum()), int(is_p[s].sum())
            out[(w, r)] = (nT, nF, nP, bool(merge_rule(nF, nP)))
    return out


def smally(case, layer=0):
    """Does the layer hold a Doppler-dominated line (the other instantiation of the kernel)?"""
    R = cpu_ref.linesum_records(case["tbl"], case["grid"], float(case["T"][layer]), float(case["p"][layer]), case["ow"], case["hw"])
    return bool(np.any((R["zw"] > 0) & (R["y"] < 1.0)))


def shard_of(case, tile=TARGET):
    """(grid of the one-tile shard, table of the lines from the first to the last that reaches it): the contiguous subset
    of the table a rank that owns this tile alone would upload."""
    g = case["grid"]
    R = cpu_ref.linesum_records(case["tbl"], g, float(case["T"][0]), float(case["p"][0]), case["ow"], case["hw"])
    ia = tile * TILE
    idx = np.nonzero((R["hi"] > R["lo"]) & (R["hi"] > ia) & (R["lo"] < ia + TILE))[0]
    order = np.argsort(np.asarray(case["tbl"]["nu"], dtype=np.float64), kind="stable")  # linesum_records' order
    keep = np.sort(order[int(idx[0]):int(idx[-1]) + 1])
    return (g[0], g[1], g[2], ia, TILE), {k: np.asarray(v)[keep] for k, v in case["tbl"].items()}


# ---- the layout of the final sums: one line alone, each tile row a value of its own -------------------------------------
def _layout_cases():
    L = {}
    g = LC.grid(1000.0, 1e-3, 6 * TILE)
    ia = 2 * TILE
    L["full_alone"] = dict(LC._case(LC.table(LC.at(g, [ia - 300])), g, 296.0, 1.0), tile=2, classes=(0, 1, 0))
    L["tile_alone"] = dict(LC._case(LC.table(LC.at(g, [ia - 600]), G_OMEGA), g, 296.0, 1.0, ow=3.0), tile=2, classes=(1, 0, 0))
    hot = LC.CASES["d_hot"]  # 6 x 1024 points already; its pressure-broadened layer alone
    L["hot_parts"] = dict(hot, T=hot["T"][:1].copy(), p=hot["p"][:1].copy(), tile=None, classes=None)
    return L


LAYOUT_CASES = _layout_cases()
