"""The drain of the nodal line-sum kernel (rtx_voigt_scatter.hip: nodal_tile, drain) takes an entry's rows by kind: the
near-zone rows (at most two runs of consecutive rows, the near zone minus the band), the rows cut by a window edge, the
band rows wholly inside the window (one run: a loop for y >= 6 and one for 1 <= y < 6, no window mask) and the band rows
cut by a window edge or of a y < 1 line (band_row's full body). Each shape at the smallest size at which it exists, against
the fp64 oracle in the metric and at the bound of tests/test_gpu_linesum_paths.py (TOL = F = 1e-5, local floor), and run
twice: array_equal.

1. One line; its near zone wholly inside tile 1, clipped to rows 0-1 at the start of tile 1, clipped at the end of tile 1,
   and its band astride tiles 1 | 2. Per placement: y = 20 (no band: one run of five), y = 14 / 12 / 8 (a band of 1 / 2 / 3
   rows at the first placement: two near-zone runs of 2, 2 + 1 and 1 rows, one of them empty where a tile clips it), y = 3
   (Weideman rows inside, series rows outside). The last placement again on a grid of 2049 points (a one-point last tile).
2. A window of a few half-widths: (a) its edges in band rows (masked body beside the unmasked one), (b) its edges in
   near-zone rows of a line with one band row: an entry with near-zone, edge and band rows.
3. 40 lines centred in tile 1: 20 general entries per wave in one round, the list (16) drained in mid-round; 48 lines
   with nothing but one window-edge row in tile 1.
4. The 40 lines on a surface layer and one at 0.005 atm (y < 1: the other instantiation, every band row the full body).
5. Tile 1 of case 3 as a shard with the contiguous part of the table that reaches it: bit-identical to the full run.

Each case asserts on the CPU (cpu_ref.row_masks) that it has the rows it names. Shapes: 3 x 1024 points, 1-2 layers,
1-48 lines."""
import numpy as np
import pytest

from oracle import cpu_ref

import linesum_cases as LC
import linesum_group_cases as GC
from test_gpu_linesum_paths import oracle, pointwise_err, run

pytestmark = pytest.mark.gpu

TOL = 1e-5  # = F of pointwise_err: the bound of tests/test_gpu_linesum_paths.py
TILE = 64 * cpu_ref.LS_ROWS
STEP = 3e-4  # 0.17 of x per point at 1000 cm^-1: a band of y = 8 is 43 points either side, three rows
FINE = 1e-4  # y = 3: a band of 211 points either side, |z| >= 8 from 130 points on: Weideman rows inside series rows
G3 = LC.grid(1000.0, STEP, 3 * TILE)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    from radtxfr_amd import _lib, engine
    _lib.load()
    return engine


def gamma_for_y(y, T=296.0, p=1.0):
    """Air width (cm^-1/atm) that gives Gamma0 sqrt(ln 2) / GammaD = y at 1000 cm^-1 (n_air 0.7, reference 296 K)."""
    P = cpu_ref.line_params(LC.table([1000.5], 0.05), T, p)
    return float(y * 0.05 / (P["Gamma0"][0] * np.sqrt(np.log(2.0)) / P["GammaD"][0]))


def masks(case, tile, layer=0):
    """cpu_ref.row_masks of every line of the case in `tile`, plus the fp32 y of the records."""
    g = case["grid"]
    R = cpu_ref.linesum_records(case["tbl"], g, float(case["T"][layer]), float(case["p"][layer]), case["ow"], case["hw"])
    ia = tile * TILE
    m = cpu_ref.row_masks(R["i0"], R["lo"], R["hi"], R["zw"], ia, min(TILE, g[4] - ia))
    m["y"] = R["y"]
    return m


def runs_of(row_bits):
    """Lengths of the runs of consecutive set rows."""
    out, n = [], 0
    for b in list(row_bits) + [False]:
        if b:
            n += 1
        elif n:
            out.append(n)
            n = 0
    return out


def check(eng, name, case):
    want = oracle("runs_" + name, case)
    r32, r64 = run(eng, case)
    e32, e64 = pointwise_err(r32, want), pointwise_err(r64, want)
    print("linesum_runs %s: f32 %.3g f64 %.3g" % (name, e32, e64))
    assert e32 <= TOL and e64 <= TOL, (name, e32, e64)
    s32, s64 = run(eng, case)
    assert np.array_equal(s32, r32) and np.array_equal(s64, r64), name
    return r32, r64


# ------------------------------------------------------------------------------------------ 1. one line, four placements
PLACE = {"inside": TILE + 8 * 64 + 32, "tile_start": TILE - 32, "tile_end": TILE + 14 * 64 + 32, "astride": 2 * TILE - 1}
KIND = {"y20": (20.0, 0, STEP), "y14": (14.0, 0, STEP), "y12": (12.0, 16, STEP), "y8": (8.0, 0, STEP),
        "y3": (3.0, 0, FINE)}  # y, lanes the centre moves, grid step
# near-zone runs / band rows of the centre tile at the first placement
INSIDE = {"y20": ([5], 0), "y14": ([2, 2], 1), "y12": ([2, 1], 2), "y8": ([1, 1], 3)}


def one_line(place, kind, n=3 * TILE):
    y, shift, step = KIND[kind]
    g = LC.grid(1000.0, step, n)
    return LC._case(LC.table(LC.at(g, [PLACE[place] + shift]), gamma_for_y(y)), g, 296.0, 1.0)


def test_one_line_census():
    """The cases are what their names say (CPU only, but it belongs to the GPU cases below)."""
    for kind, (pp_runs, n_band) in INSIDE.items():
        m = masks(one_line("inside", kind), 1)
        assert runs_of(m["pp"][0]) == pp_runs and int(m["bd"][0].sum()) == n_band, (kind, runs_of(m["pp"][0]), int(m["bd"][0].sum()))
        assert not m["edge"][0].any() and np.array_equal(m["bd"][0], m["bd"][0] & m["inside"][0])
    c = one_line("inside", "y3")
    m = masks(c, 1)
    C = cpu_ref.linesum_census(c["tbl"], c["grid"], 296.0, 1.0, c["ow"], c["hw"])
    assert 1.0 <= m["y"][0] < 6.0 and m["bd"][0].sum() >= 6 and C["band_wei32"] > 0 and C["band_series"] > 0, C
    m = masks(one_line("tile_start", "y20"), 1)
    assert np.array_equal(np.nonzero(m["pp"][0])[0], [0, 1])
    m = masks(one_line("tile_start", "y14"), 1)
    assert runs_of(m["pp"][0]) == [2] and not m["bd"][0].any()  # the band row and the other run lie in tile 0
    m = masks(one_line("tile_end", "y20"), 1)
    assert np.array_equal(np.nonzero(m["pp"][0])[0], [12, 13, 14, 15])
    m1, m2 = masks(one_line("astride", "y8"), 1), masks(one_line("astride", "y8"), 2)
    assert m1["bd"][0, 15] and m2["bd"][0, 0] and m1["pp"][0].any() and m2["pp"][0].any()


@pytest.mark.parametrize("kind", sorted(KIND))
@pytest.mark.parametrize("place", sorted(PLACE))
def test_one_line(eng, place, kind):
    check(eng, "%s_%s" % (place, kind), one_line(place, kind))


@pytest.mark.parametrize("kind", sorted(KIND))
def test_one_line_ragged_grid(eng, kind):
    """2049 points: the near zone and the band reach into the last tile, which holds one point."""
    check(eng, "ragged_%s" % kind, one_line("astride", kind, 2 * TILE + 1))


# ------------------------------------------------------------------------------------------------- 2. narrow windows
def narrow(which):
    y, hw = {"edge_in_band": (8.0, 1.0), "edge_in_near": (14.0, 1.5)}[which]
    return LC._case(LC.table(LC.at(G3, [PLACE["inside"]]), gamma_for_y(y)), G3, 296.0, 1.0, hw=hw)


@pytest.mark.parametrize("which", ["edge_in_band", "edge_in_near"])
def test_narrow_window(eng, which):
    m = masks(narrow(which), 1)
    cut = m["bd"][0] & ~m["inside"][0]
    if which == "edge_in_band":
        assert cut.any() and (m["bd"][0] & m["inside"][0]).any(), "band rows cut by the window beside band rows inside it"
    else:
        assert m["pp"][0].any() and m["edge"][0].any() and m["bd"][0].any() and not cut.any(), "all three row kinds in one entry"
    check(eng, "narrow_" + which, narrow(which))


# ------------------------------------------------------------------------------------- 3. lists drained in mid-round
def crowd(p=1.0, T=296.0):
    """40 lines centred in tile 1, 20 points apart, y = 20 / 14 / 8 / 3 in turn: every one a general entry there."""
    gi = TILE + 100 + 20 * np.arange(40)
    ys = np.tile([20.0, 14.0, 8.0, 3.0], 10)
    return LC._case(LC.table(LC.at(G3, gi), [gamma_for_y(y) for y in ys]), G3, T, p)


def edge_crowd():
    """48 lines centred in tile 0 whose right window edge falls in tile 1, two points apart: in tile 1 each is far rows
    and ONE cut row, an edge-only entry (24 per wave; their centres, bands and near zones lie in tile 0)."""
    gi = 200 + 2 * np.arange(48)
    W = (TILE + 5 * 64 + 30 - 200) * STEP  # the first line's window ends in row 5 of tile 1
    return LC._case(LC.table(LC.at(G3, gi), W / 50.0), G3, 296.0, 1.0)


def test_entry_list_overflow(eng):
    case = crowd()
    m = masks(case, 1)
    general = (m["pp"] | m["bd"]).any(1)
    assert general.sum() == 40 and general[0::2].sum() > cpu_ref.LS_ENT_CAP, "more entries than the list holds, per wave"
    check(eng, "crowd", case)


def test_edge_only_lines(eng):
    case = edge_crowd()
    m = masks(case, 1)
    assert np.all(m["edge"].sum(1) == 1) and not m["pp"].any() and not m["bd"].any() and m["far"].any(1).all()
    check(eng, "edge_crowd", case)


# ------------------------------------------------------------------------------------------ 4. a y < 1 layer beside it
def test_smally_layer_beside_surface_layer(eng):
    case = crowd(p=(1.0, 0.005), T=(296.0, 250.0))
    m = masks(case, 1, layer=1)
    assert np.all(m["y"] < 1.0) and m["bd"].any(), "layer 1: the instantiation for Doppler-dominated lines"
    assert np.all(masks(case, 1, layer=0)["y"] >= 1.0)
    check(eng, "crowd_two_layers", case)


# -------------------------------------------------------------------------------------------------- 5. shard identity
def test_shard_of_crowd_is_bit_identical(eng):
    case = crowd()
    g, sub = GC.shard_of(case, tile=1)
    assert g[3] == TILE and g[4] == TILE
    f32, f64 = run(eng, case)
    s32, s64 = run(eng, dict(case, tbl=sub), g=g)
    cut = slice(g[3], g[3] + g[4])
    assert np.all(f64[:, cut] > 0.0)
    assert np.array_equal(s32, f32[:, cut]) and np.array_equal(s64, f64[:, cut])
