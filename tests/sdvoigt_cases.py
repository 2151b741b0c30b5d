"""Line tables, grids and states that put rtx_sdvoigt_sum's default kernel (sdvoigt_tile_kernel) on one path at a time.
Imported by the GPU test (tests/test_gpu_sdvoigt_paths.py: every case against the long-double oracle, on both kernels)
and by the host test (tests/test_sdvoigt_paths_host.py: each case reaches the paths it names in `expect`, by
cpu_ref.sd_census), so the two cannot drift apart.

A case is a dict: tbl (HITRAN-format columns with SD_air), grid (xmin, xmax, n_total, offset, n), T, p (per state,
atm), ow / hw (OmegaWing / OmegaWingHW), thresh (IntensityThreshold), expect (census labels that must be non-zero over the
case's states; "!label": must be zero). Centres sit a quarter step past a grid point and have no pressure shift, so a
centre's grid index is the one named here; the cases named *_switch put a regime switch on the grid on purpose and say
so. Windows are set exactly: by OmegaWing = (k + 1/2) step, a window of [c - k, c + k] around the centre index c, or per
line by gamma_air = (k + 1/2) step / OmegaWingHW at T = 296 K, p = 1 atm (Gamma0 = gamma_air there).

Numbers behind the choices, H2O near 1000 cm^-1 at 296 K: GammaD = 1.45e-3 cm^-1, cte = 574; with gamma_air = 0.07 and
SD = 0.1 at 1 atm Gamma2 = 0.007, csqrtY = 0.124 and the PART4 far switch (sd_zones: far4) lies 0.80 cm^-1 from the
centre; at 0.01 atm csqrtY = 12.4 and far4 = 0.025 cm^-1."""
import numpy as np

from oracle import cpu_ref
from linesum_cases import at, grid, table

T0 = 296.0


def sd_table(nu, gamma_air=0.07, sd=0.1, sw=1e-20):
    t = table(nu, gamma_air, sw)
    t["SD_air"] = np.broadcast_to(np.asarray(sd, dtype=np.float64), t["nu"].shape).copy()
    return t


def _case(tbl, g, T=T0, p=1.0, ow=0.0, hw=0.0, thresh=0.0, expect=(), shards=()):
    T, p = np.broadcast_arrays(np.atleast_1d(np.asarray(T, dtype=np.float64)), np.atleast_1d(np.asarray(p, dtype=np.float64)))
    return dict(tbl=tbl, grid=g, T=T.copy(), p=p.copy(), ow=float(ow), hw=float(hw), thresh=float(thresh),
                expect=tuple(expect), shards=tuple(shards))


def step_of(g):
    return (g[1] - g[0]) / (g[2] - 1)


def ow_of(g, k):
    """OmegaWing that gives a centre at index c + 1/4 the window [c - k, c + k]."""
    return (k + 0.5) * step_of(g)


def window_table(g, centres, ks, hw, sd=0.1, sw=1e-20):
    """Lines at indices `centres` whose windows are [c - k, c + k] at T = 296 K, p = 1 atm under OmegaWingHW = hw."""
    ks = np.asarray(ks, dtype=np.float64)
    return sd_table(at(g, centres), (ks + 0.5) * step_of(g) / hw, sd, sw)


def far4_of(gamma, sd, p, nu=1000.0, T=T0):
    """sd_zones' PART4 far switch (cm^-1 from the centre) of a line of the tables here."""
    P = cpu_ref.line_params(sd_table([nu], gamma, sd), T, p)
    return cpu_ref.sd_zones(P["Gamma0"][0], sd * p * gamma, np.sqrt(np.log(2.0)) / P["GammaD"][0], 1.0)[4]


def _cases():
    C = {}
    TILE = 1024
    # ---- levels -----------------------------------------------------------------------------------------------------
    # tile level: centres 255 / 256 / 257 points outside tile 1 on both sides (SD_TDIST = 256 is the cut), windows over
    # the whole grid. step 4e-3 puts far4 200 points from the centre, inside the 256
    g = grid(1000.0, 4e-3, 3 * TILE)
    gi = np.array([TILE - 255, TILE - 256, TILE - 257, 2 * TILE - 1 + 255, 2 * TILE - 1 + 256, 2 * TILE - 1 + 257])
    C["lv_tile_256"] = _case(sd_table(at(g, gi)), g, ow=ow_of(g, 4000),
                             expect=("tile_left_255", "tile_left_256", "tile_left_257", "tile_right_255", "tile_right_256",
                                     "tile_right_257", "tile_level_at_256", "tile_level_at_257", "row_list_at_255",
                                     "!tile_level_at_255", "!row_list_at_256", "!row_list_at_257", "tile_b", "covers_grid"))
    # window edges against tile 1: lo == ia / ia + 1 from a centre right of it, hi == ib / ib - 1 from one left of it
    g = grid(1000.0, 4e-3, 3 * TILE)
    C["lv_tile_edges"] = _case(window_table(g, [2400, 2400 + 8, 700, 700 - 8], [2400 - TILE, 2400 + 8 - TILE - 1, 2 * TILE - 700 - 1,
                                                                               2 * TILE - 1 - (700 - 8) - 1], hw=78.0),
                               g, hw=78.0, expect=("lo_eq_ia", "lo_eq_ia1", "hi_eq_ib", "hi_eq_ib1", "tile_b", "row_edge"))
    # a narrow low-pressure line (Gamma0 = 7e-5 << GammaD: the poles of 1/2 + t^2 sit on the real axis, 11 points either
    # side of the centre at this step) exactly 256 points outside tile 1: the worst case of the 32-node bound
    g = grid(1000.0, 1.1e-4, 3 * TILE)
    C["lv_tile_narrow_line"] = _case(sd_table(at(g, [TILE - 256, 2 * TILE - 1 + 256])), g, p=1e-3, ow=ow_of(g, 4000),
                                     expect=("tile_level_at_256", "tile_left_256", "tile_right_256"))
    # row level: centres on rows 0, 8 and 15 of tile 1, and 1 and 2 rows outside it (the near zone reaches in); at 0.05 atm
    # far4 lies 34 points out, so the third row from a centre row is nodal and the second is near. One centre sits on the
    # last point of row 5: row 7 starts 65 points from it, where 12 nodes would be off by ~1e-6 of the line
    g = grid(1000.0, 1e-3, 3 * TILE)
    gi = np.array([TILE + 10, TILE + 5 * 64 + 63, TILE + 8 * 64 + 33, TILE + 15 * 64 + 60, TILE - 20, TILE - 64 - 20, 2 * TILE + 20,
                   2 * TILE + 64 + 20])
    C["lv_rows"] = _case(sd_table(at(g, gi)), g, p=0.05, ow=ow_of(g, 4000),
                         expect=("centre_row_0", "centre_row_8", "centre_row_15", "rc_outside_-1", "rc_outside_-2", "rc_outside_16",
                                 "rc_outside_17", "row_near", "row_near_2_from_centre", "row_nodal_3_from_centre", "row_nodal_b",
                                 "p4_real_in_in", "p4_real_in_out", "p4_far"))
    # window edges against rows of tile 1: on a row boundary at either end, inside a row, both in one row (a window
    # narrower than a row), one window over the whole grid, and one that ends on the last point but one of a far row (row 8
    # from a centre on row 1: hi == pb, the row is an edge row and its last point lies outside the window)
    g = grid(1000.0, 4e-3, 3 * TILE)
    C["lv_row_edges"] = _case(window_table(g, [TILE + 476, TILE + 576, TILE + 64 * 5 + 30, TILE + 500, 300, TILE + 100],
                                           [220, 191, 10, 4000, 300 + 0, 474], hw=20.0), g, hw=20.0,
                              expect=("row_starts_window", "row_ends_window", "edge_inside_row", "both_edges_one_row", "narrow",
                                      "covers_grid", "row_edge", "window_ends_at_row_last_point"))

    # ---- zones ------------------------------------------------------------------------------------------------------
    # zn_far4_switch: the PART4 far switch (|x1| + y1 = 15) g - 1/2 points before the near end of tile 1 (step 2e-3: far4 is
    # 400 points out) and of a row of tile 1, g = 1, 2, 3, on both sides of the centre. The two-point margin decides: g = 3
    # is nodal, g = 1 and 2 are not. These centres are placed by the switch, not a quarter step past a grid point.
    g = grid(1000.0, 2e-3, 3 * TILE)
    h = step_of(g)
    X = lambda i: g[0] + i * h
    f4 = far4_of(0.07, 0.1, 1.0)
    nus = []
    for gap in (1, 2, 3):
        nus += [X(TILE) - f4 - (gap - 0.5) * h, X(2 * TILE - 1) + f4 + (gap - 0.5) * h,
                X(TILE + 64 * 10) - f4 - (gap - 0.5) * h, X(TILE + 64 * 4 + 63) + f4 + (gap - 0.5) * h]
    C["zn_far4_switch"] = _case(sd_table(nus), g, ow=ow_of(g, 4000),
                                expect=("tile_switch_gap_1_rows", "tile_switch_gap_2_rows", "tile_switch_gap_3_tile",
                                        "!tile_switch_gap_1_tile", "!tile_switch_gap_2_tile", "!tile_switch_gap_3_rows",
                                        "switch_gap_pointwise_1", "switch_gap_pointwise_2", "switch_gap_nodal_3", "row_switch"))
    # the same switch exactly on a grid point, right and left of a centre: the only case in which the float64 and the
    # long-double run may take different branches at a point (the metric drops such points, at most 2 per line)
    C["zn_switch_on_point"] = _case(sd_table([X(TILE + 300) - f4, X(TILE + 700) + f4]), g, ow=ow_of(g, 4000),
                                    expect=("row_switch", "p4_far", "p4_real_in_out"))
    # d <= 0 in sd_zones: at 10 atm with SD = 0.004 (y = 400) every point of PART4 is far, far4 = 0 and zone b starts at
    # the margin; only the near rows are point by point
    g = grid(1000.0, 4e-3, 3 * TILE)
    C["zn_all_far"] = _case(sd_table(at(g, [300, TILE + 500, 2 * TILE + 800]), sd=0.004), g, p=10.0, ow=ow_of(g, 4000),
                            expect=("zone_b_all_far", "tile_b", "row_nodal_b", "row_near", "p4_far", "!row_switch",
                                    "!p4_real_in_in", "!p4_real_in_out"))
    # zone a: SD = 1e-10 at 0.01 atm has csqrtY = 1.2e10 and PART2 out to 0.32 cm^-1, beyond the windows (0.3 cm^-1): Z1 is on
    # hum1_wei's asymptote from 0.0254 cm^-1 (254 points), Z2 has y2 ~ 2 csqrtY. Tile and row level through zone a
    g = grid(1000.0, 1e-4, 3 * TILE)
    C["zn_zone_a"] = _case(sd_table(at(g, [300, TILE + 500, 2 * TILE + 700]), sd=1e-10), g, p=0.01, ow=ow_of(g, 2900),
                           expect=("tile_a", "row_nodal_a", "p2_real", "!tile_b", "!row_nodal_b", "!p4_far", "!p4_real_in_in"))
    # a tiny speed dependence with csqrtY < 8: SD = 1e-8 on a microwave line (0.07 cm^-1: cte = 8.3e6) at 10 atm. PART2 needs
    # |X| <= 3e-8 Y, here 1e8 against 4e-8: there is no PART2 and so no zone a (for Gamma0 > 1.5 Gamma2, PART2 with
    # csqrtY < 8 would need SD within 8.5e-7 of 2/3 and a grid step of 1e-10 cm^-1: tools/sdvoigt_reference_error.py)
    g = grid(2.0, 1e-3, 2 * TILE)
    C["zn_tiny_sd_small_sy"] = _case(sd_table(at(g, [-1930]), 0.5, 1e-8), g, p=10.0, hw=50.0,
                                     expect=("zone_b_all_far", "tile_b", "!tile_a", "!row_nodal_a", "!p2_real"))
    # the PART2 boundary inside tile 1: SD = 7e-10 at 0.01 atm, |X| = 3e-8 Y 457 points from the centre (step 1e-4); rows
    # through zone a inside it, zone b outside it, the row that holds it point by point
    g = grid(1000.0, 1e-4, 3 * TILE)
    C["zn_part2_boundary"] = _case(sd_table(at(g, [TILE + 100, 2 * TILE - 90]), sd=7e-10), g, p=0.01, ow=ow_of(g, 2900),
                                   expect=("row_nodal_a", "row_nodal_b", "row_switch", "p2_real", "p4_far", "tile_b"))
    # SD = 0 lines beside one speed-dependent line: PART1, zone b from (15 - y) / cte, at 1 atm (y = 40: the asymptote
    # everywhere) and at 0.01 atm (Weideman within 25 points of the centre)
    g = grid(1000.0, 1e-3, 3 * TILE)
    C["zn_sd0"] = _case(sd_table(at(g, [200, TILE + 300, TILE + 900, 2 * TILE + 500]), sd=[0.0, 0.0, 0.1, 0.0]), g, p=(1.0, 0.01),
                        T=(296.0, 250.0), ow=ow_of(g, 4000), expect=("p1_w24", "p1_asym", "tile_b", "row_nodal_b"))
    # Gamma0 <= 1.5 Gamma2 (SD = 0.7 and 1.0): no zones, every row point by point, the complex Weideman form for Re Z < 0.
    # These two stay positive over 1e-4 ... 10 atm (tools/sdvoigt_reference_error.py); SD = 3 is negative beyond ~0.1 cm^-1 of the
    # centre from 0.01 atm up, so the sum changes sign (SIGN_CHANGE: the host test asserts it) and den != |want|
    g = grid(1000.0, 1e-3, 2 * TILE)
    C["zn_sd_large"] = _case(sd_table(at(g, [400, TILE + 200, TILE + 500, TILE + 800]), sd=[0.7, 1.0, 3.0, 0.7]), g, p=(1.0, 0.02),
                             ow=ow_of(g, 3000), expect=("row_nozones", "p4_cplx", "!tile_a", "!tile_b", "!row_nodal_a", "!row_nodal_b"))

    # ---- profile branches -------------------------------------------------------------------------------------------
    # the cpf3 shell (|Z| = 8 between the two arguments, 2 csqrtY <= 1): 1 atm, SD 0.08 ... 0.15, ~40 points per line
    g = grid(1000.0, 1e-3, TILE)
    C["pf_cpf3"] = _case(sd_table(at(g, [200, 500, 800]), sd=[0.08, 0.1, 0.15]), g, ow=ow_of(g, 1100),
                         expect=("p4_cpf3", "p4_real_in_in", "p4_real_in_out", "p4_far"))
    # PART3's near form: a microwave line (0.07 cm^-1) at 10 atm with SD 0.1; Y / |X| falls through 1e-15 53.2 cm^-1 from
    # the centre, inside the 350-half-width window (245 cm^-1): PART4's far wing below it, PART3 above, the switch in tile 1
    g = grid(0.07 + 51929.75e-3, 1e-3, 3 * TILE)
    C["pf_p3_near"] = _case(sd_table(at(g, [-51930])), g, p=10.0, hw=350.0,
                            expect=("p3_near", "p4_far", "row_switch", "tile_b", "row_nodal_b", "!p3_far"))
    # PART3's far form (|X| > 1.6e7, from 7616 cm^-1): the same line at 0.068 atm, where PART3 starts 7826 cm^-1 from the
    # centre, under OmegaWing = 9000; the switch from PART4's far wing lies in tile 0
    g = grid(0.07 + 77499.75 * 0.1, 0.1, 2 * TILE)
    C["pf_p3_far"] = _case(sd_table(at(g, [-77500])), g, p=0.068, ow=9000.0, expect=("p3_far", "p4_far", "row_switch", "!p3_near"))
    # PART2 with Re Z1 < 0 (p2_cplx): SD = 1.0 at 1e-6 atm, where |X| <= 3e-8 Y within 3e-7 cm^-1 of the centre
    g = grid(1000.0, 1e-7, TILE)
    C["pf_p2_cplx"] = _case(sd_table(at(g, [300, 700]), sd=[1.0, 0.8]), g, p=1e-6, ow=ow_of(g, 1100), expect=("p2_cplx", "p4_cplx"))

    # ---- lists ------------------------------------------------------------------------------------------------------
    # one tile with 257 candidates: 200 lines 300 ... 1300 points left of the grid (tile level) and 57 inside it; the second
    # chunk holds the last line alone and has no tile-level line
    g = grid(1000.0, 4e-3, TILE)
    gi = np.r_[np.arange(-1295, -295, 5), np.arange(10, 1007, 17.5).astype(int)[:57]]
    C["ls_257"] = _case(sd_table(at(g, gi)), g, ow=ow_of(g, 2400),
                        expect=("second_chunk", "chunk_no_tile_after_tile", "chunk_mixed", "tile_b", "row_list"))
    # 520 candidates left of a one-tile grid, every other one without zones (SD = 0.7: row list, every row point by point),
    # the rest tile level: three chunks that mix both classes
    gi = np.arange(-1300, -260, 2)
    C["ls_mixed_520"] = _case(sd_table(at(g, gi), sd=np.where(np.arange(gi.size) % 2 == 0, 0.1, 0.7)), g, ow=ow_of(g, 2400),
                              expect=("second_chunk", "chunk_mixed", "tile_b", "row_nozones"))
    # 1, 8 and 9 tile-level lines in the chunk (a ragged group of 8, a full one, one more), plus one line in the tile
    for k in (1, 8, 9):
        C["ls_nT_%d" % k] = _case(sd_table(at(g, np.r_[np.arange(-300 - 40 * k, -300, 40), 500])), g, ow=ow_of(g, 2400),
                                  expect=("nT_%d" % k, "row_list"))
    # candidates inside the range with an empty window (a window of +-0.29 steps between two grid points: OmegaWingHW = 10
    # times GammaD on a 0.05 cm^-1 grid, centres 0.45 steps past a point) and candidates under the IntensityThreshold
    # (WS = 0, window emptied)
    g = grid(1000.0, 0.05, TILE + 100)
    gi = np.array([100, 300, 500, 700, 900, 1100], dtype=np.float64)
    nus = at(g, gi) + np.array([0, 0.2, 0, 0.2, 0, 0]) * step_of(g)
    C["ls_empty_dropped"] = _case(sd_table(nus, [0.3, 1e-4, 0.3, 1e-4, 0.3, 0.3], 0.1, [1e-20, 1e-20, 1e-26, 1e-20, 1e-20, 1e-26]), g,
                                  hw=10.0, thresh=1e-23, expect=("cand_empty_window", "cand_dropped", "row_list"))

    # ---- shapes -----------------------------------------------------------------------------------------------------
    # n = 1 (a one-point shard of a two-point grid: the ABI takes no shorter grid) ... 2049: ragged last rows and tiles; a
    # tile-level member over a ragged last tile (its nodes lie beyond the grid's end) and a row-level member over a ragged
    # last row
    for n in (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049):
        g = grid(1000.0, 4e-3, max(n, 2), 0, n)
        gi = np.array([-300, -200, n // 3, n - 340, n - 100, n + 300])
        ex = ("ragged_tile" if n % TILE else "!ragged_tile", "ragged_row" if n % 64 else "!ragged_row")
        C["sh_n_%d" % n] = _case(sd_table(at(g, gi), sd=[0.1, 0.12, 0.0, 0.1, 0.7, 0.1]), g, ow=ow_of(g, 4000), expect=ex)
    # shards of lv_rows and lv_tile_256 off a tile boundary, the grid's last point alone (the oracle's X there is xmax), and a
    # tile-aligned shard (equal, bit for bit, to the same points of the full grid)
    C["lv_rows"]["shards"] = ((37, 1500), (TILE + 333, 2 * TILE - 333 - 17), (3 * TILE - 1, 1), (TILE, TILE))
    C["lv_tile_256"]["shards"] = ((700, 2000), (3 * TILE - 1, 1), (TILE, 2 * TILE))

    # ---- layers -----------------------------------------------------------------------------------------------------
    # three states in one call, 1 / 1e-2 / 1e-4 atm: windows of 50 half-widths, so maxhw differs (3500, 37 and 65 points) and
    # the same line is tile level, row level or point by point depending on the state; and the middle state alone
    g = grid(1000.0, 1e-3, 4 * TILE)
    gi = np.array([150, 700, 1100, 1500, 2047, 2048, 2500, 3000, 3300, 3900, 4300, -400])
    sd = [0.1, 0.0, 0.15, 1e-9, 0.7, 0.1, 0.05, 1e-5, 0.1, 0.0, 0.1, 0.1]
    tb = sd_table(at(g, gi), np.linspace(0.05, 0.09, gi.size), sd)
    C["ly_three"] = _case(tb, g, T=(296.0, 250.0, 220.0), p=(1.0, 1e-2, 1e-4), hw=50.0,
                          expect=("tile_b", "row_nodal_b", "row_near", "row_edge", "p1_w24", "p4_cplx", "p4_real_in_in"))
    C["ly_one"] = _case(tb, g, T=250.0, p=1e-2, hw=50.0, expect=("row_near", "!row_nodal_b", "!tile_b"))
    return C


CASES = _cases()
SIGN_CHANGE = ("zn_sd_large",)  # cases whose long-double sum takes both signs


# ---- the reference and the metric (shared by the host and the GPU test) ------------------------------------------------
BOUND = 1e-9     # of den: the contract of this path
OWN_FACTOR = 4   # on the reference's own fp64 loss
OWN_HALO = 64
PREDICATES = cpu_ref.SD_P1 | cpu_ref.SD_P2 | cpu_ref.SD_P3 | cpu_ref.SD_P4 | cpu_ref.SD_CPF3 | cpu_ref.SD_W24_1 | cpu_ref.SD_W24_2


def axis(g):
    """The shard's wavenumbers as the library forms them: index * step + xmin, the grid's last point pinned to xmax."""
    xmin, xmax, n_total, offset, n = g
    X = np.arange(offset, offset + n, dtype=np.float64) * ((xmax - xmin) / (n_total - 1)) + xmin
    if n and offset + n == n_total:
        X[-1] = xmax
    return X


def _halo_max(a, h=OWN_HALO):
    b = np.concatenate([np.zeros(h, a.dtype), a, np.zeros(h, a.dtype)])
    return np.lib.stride_tricks.sliding_window_view(b, 2 * h + 1).max(axis=1)


_ORACLE = {}


def oracle(name, g=None):
    """Per state of case `name` on its grid (or the shard g): want (long double sum), want64 (the float64 oracle), den
    (sum_l |WS_l profile_l|, long double), own (max over |j - i| <= 64 of |want64 - want|), skip (points at which a branch
    predicate of some line differs between the two precisions), skip_per_line (the most such points on one line) and
    pairs ((line, point) pairs inside windows). Lists over the states; cached."""
    case = CASES[name]
    g = g or case["grid"]
    if (name, g) not in _ORACLE:
        X = axis(g)
        out = dict(want=[], want64=[], den=[], own=[], skip=[], skip_per_line=[], pairs=[])
        for T, p in zip(case["T"], case["p"]):
            kw = dict(T=float(T), p=float(p), OmegaGrid=X, OmegaWing=case["ow"], OmegaWingHW=case["hw"],
                      IntensityThreshold=case["thresh"])
            lo = cpu_ref.sdvoigt_terms(case["tbl"], dtype=np.float64, **kw)
            hi = cpu_ref.sdvoigt_terms(case["tbl"], dtype=np.longdouble, **kw)
            skip = np.zeros(X.size, dtype=bool)
            worst, pairs = 0, 0
            for (r64, a64, b64, c64), (rl, al, bl, cl) in zip(lo["lines"], hi["lines"]):
                assert (r64, a64, b64) == (rl, al, bl)
                d = ((c64 ^ cl) & PREDICATES) != 0
                skip[a64:b64] |= d
                worst = max(worst, int(d.sum()))
                pairs += b64 - a64
            out["want"].append(hi["xs"])
            out["want64"].append(lo["xs"])
            out["den"].append(hi["den"])
            out["own"].append(_halo_max(np.abs(lo["xs"].astype(np.longdouble) - hi["xs"])))
            out["skip"].append(skip)
            out["skip_per_line"].append(worst)
            out["pairs"].append(pairs)
        _ORACLE[(name, g)] = out
    return _ORACLE[(name, g)]


def judge(got, ref_k, k):
    """The metric for state k of an oracle() result: (worst |got - want| / den, worst |got - want| / (BOUND den + OWN_FACTOR
    own), share of points where the own term exceeds the den term, structural zeros exact) over the points not skipped.
    got is one state's row."""
    L = np.longdouble
    want, den, own, skip = ref_k["want"][k], ref_k["den"][k], ref_k["own"][k], ref_k["skip"][k]
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    zero = den == 0
    zeros_exact = bool(np.all(got[zero] == 0.0))
    use = ~zero & ~skip
    if not use.any():
        return 0.0, 0.0, 0.0, zeros_exact
    if not np.isfinite(got).all():
        return float("inf"), float("inf"), 0.0, zeros_exact
    err = np.abs(got[use].astype(L) - want[use])
    allow = BOUND * den[use] + OWN_FACTOR * own[use]
    return (float(np.max(err / den[use])), float(np.max(err / allow)),
            float(np.mean(OWN_FACTOR * own[use] > BOUND * den[use])), zeros_exact)
