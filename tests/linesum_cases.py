"""Line tables, grids and layers that put rtx_voigt_sum's nodal kernel on one path at a time. Imported by the GPU test
(tests/test_gpu_linesum_paths.py: every case against the fp64 oracle) and by the host census (tests/test_host.py: each
case reaches the paths it names in `expect`, by cpu_ref.linesum_census), so the two cannot drift apart.

A case is a dict: tbl (HITRAN-format columns: synthetic.synth_line_table with its columns edited), grid (xmin, xmax,
n_total, offset, n), T, p (per layer, atm), ow / hw (OmegaWing / OmegaWingHW), expect (census labels that must be
non-zero; "!label": must be zero). Centres sit a quarter step past a grid point (no rounding tie in the nearest index) and have no pressure
shift, so a centre's grid index is the one named here."""
import numpy as np

from oracle import cpu_ref
from radtxfr_amd import synthetic


def grid(xmin, step, n_total, offset=0, n=None):
    return (xmin, xmin + (n_total - 1) * step, n_total, offset, n_total - offset if n is None else n)


def at(g, gi):
    """Wavenumber a quarter step past global grid index gi (array)."""
    return g[0] + (np.asarray(gi, dtype=np.float64) + 0.25) * (g[1] - g[0]) / (g[2] - 1)


def table(nu, gamma_air=0.07, sw=1e-20, seed=7):
    """synth_line_table's columns with every line edited: H2O main isotopologue, the given centres, air widths and
    strengths, n_air 0.7, no pressure shift."""
    nu = np.atleast_1d(np.asarray(nu, dtype=np.float64))
    t = synthetic.synth_line_table(seed, nu.size, 500.0, 600.0)
    full = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), nu.shape).copy()
    t.update(molec_id=np.ones(nu.size, np.int64), local_iso_id=np.ones(nu.size, np.int64), nu=nu.copy(), sw=full(sw),
             gamma_air=full(gamma_air), n_air=full(0.7), delta_air=np.zeros(nu.size), elower=full(100.0))
    return t


def _case(tbl, g, T, p, ow=0.0, hw=50.0, expect=()):
    T, p = np.broadcast_arrays(np.atleast_1d(np.asarray(T, dtype=np.float64)), np.atleast_1d(np.asarray(p, dtype=np.float64)))
    return dict(tbl=tbl, grid=g, T=T.copy(), p=p.copy(), ow=float(ow), hw=float(hw), expect=tuple(expect))


def _at_switch(g, gi, gamma, T, p, sign):
    """A centre that puts |x| + y = 15 (hum1_wei's switch) on grid point gi: the fp64 recheck lane."""
    P = cpu_ref.line_params(table([at(g, gi)], gamma), T, p)
    cte = np.sqrt(np.log(2.0)) / P["GammaD"][0]
    y = P["Gamma0"][0] * cte
    X = g[0] + gi * (g[1] - g[0]) / (g[2] - 1)
    return X - sign * (15.0 - y) / cte


def _cases():
    C = {}
    # a. one class at a time ------------------------------------------------------------------------------------------
    # tile level: full members 511 / 512 / 513 points outside tile 2 on both sides (RTX_SC_TILE_DIST = 512 is the cut),
    # plus members 130 points out, row level here, whose 16-node tile interpolation would be off by ~1e-4 (narrow
    # Lorentz, pole close to the tile); OmegaWing sets the windows (3 cm^-1 > 50 Gamma0) so that all of them cover tile 2
    g = grid(1000.0, 1e-3, 5 * 1024)
    gi = np.array([2048 - 511, 2048 - 512, 2048 - 513, 2048 - 130, 3071 + 511, 3071 + 512, 3071 + 513, 3071 + 130])
    C["a_tile_level"] = _case(table(at(g, gi), 0.02), g, 296.0, 1.0, ow=3.0,
                              expect=("tile_left_512", "tile_left_513", "full_left_511", "tile_right_512",
                                      "tile_right_513", "full_right_511", "tile", "full"))
    # row level: a full member (300 points outside tile 4, window over all of it) and partial members whose window edge
    # cuts tile 4 (centres 3000 points out, W = 3.5 cm^-1), on both sides; their cut rows are edge-only entries
    g = grid(1000.0, 1e-3, 9 * 1024)
    gi = np.array([4096 - 300, 4096 - 3000, 5119 + 3000, 5119 + 300])
    C["a_row_level"] = _case(table(at(g, gi)), g, 296.0, 1.0, expect=("full", "partial", "edge_only"))
    # near zone (+-2 rows, point by point) with the centre on the first, the middle and the last row of tile 2
    g = grid(1000.0, 1e-3, 6 * 1024)
    gi = np.array([2048 + 10, 2048 + 512 + 10, 2048 + 1013])
    C["a_near_zone"] = _case(table(at(g, gi)), g, 296.0, 1.0, expect=("centre_row_0", "centre_row_8", "centre_row_15", "near"))
    # |x| + y = 15 exactly on a lane, left and right of the centre, for y ~ 10 (series rows) and y ~ 3 (Weideman rows)
    g = grid(1000.0, 1e-4, 4 * 1024)
    nus = [_at_switch(g, 1500, 0.0174, 296.0, 1.0, +1), _at_switch(g, 2600, 0.0174, 296.0, 1.0, -1),
           _at_switch(g, 3500, 0.0052, 296.0, 1.0, +1)]
    C["a_switch"] = _case(table(nus, [0.0174, 0.0174, 0.0052]), g, 296.0, 1.0, expect=("band_recheck", "band_asym6"))
    # Weideman band rows. At p = 0.01 atm y = {0.115, 0.57, 0.86, 1.7, 3.0, 3.5, 9.2}: a SMALLY layer with fp64 Weideman
    # rows and fp32 asymK_re<12> outer rows (every lane |x| >= 5.5), the 1 <= y < 6 series / Weideman rows (y = 3.5: the
    # 6-term series would be off by ~3e-5 at |z| = y) and y >= 6; at 0.1 atm y = {1.15, 5.7, 8.6, 17, 30, 35, 92}: the
    # plain instantiation with the same three fp32 regimes
    gam = [0.02, 0.1, 0.15, 0.3, 0.52, 0.61, 1.6]
    for nu0, step, ps in ((1000.0, 1e-4, (0.01, 0.1)), (6000.0, 6e-4, (0.06, 0.6))):
        g = grid(nu0, step, 16 * 1024)
        gi = np.linspace(1500, 16 * 1024 - 1500, len(gam)).astype(int)
        C["a_band_%d" % int(nu0)] = _case(table(at(g, gi), gam), g, 296.0, ps,
                                          expect=("band_outer", "band_w64", "band_series", "band_wei32", "band_asym6",
                                                  "smally_layer", "plain_layer"))
    # the upper standard atmosphere: Doppler-dominated down to y ~ 1e-6 (the last rows of the table, then 2e-8 atm)
    A = synthetic.load_standard_atmosphere()
    rows = A[[40, 52, 60, 65]]
    g = grid(1000.0, 1e-4, 8 * 1024)
    C["a_upper_atmosphere"] = _case(table(at(g, [1800, 4100, 6300])), g, np.r_[rows[:, 5], 200.0],
                                    np.r_[rows[:, 4] / 101325.0, 2e-8], expect=("band_outer", "band_w64", "smally_layer"))

    # b. window geometry ----------------------------------------------------------------------------------------------
    # windows narrower than a row (OmegaWingHW = 0.2: 14 points at 1 atm, one point at 0.01 atm), both edges in one row
    # (centre mid-row) or astride a row boundary
    g = grid(1000.0, 1e-3, 3 * 1024)
    C["b_narrow"] = _case(table(at(g, [64 * 5 + 32, 64 * 20 + 2, 64 * 33 + 61])), g, 296.0, (1.0, 0.01), hw=0.2,
                          expect=("narrow", "one_row", "entry"))
    # window edges exactly on a row boundary (lo / hi a multiple of 64: no partial row); OmegaWing = 0.3 sets some
    # windows, OmegaWingHW * Gamma0 (gamma_air 0.5 cm^-1/atm) the others
    g = grid(1000.0, 1e-3, 4 * 1024)
    X = lambda i: g[0] + i * (g[1] - g[0]) / (g[2] - 1)
    nus = [X(64 * 10) + 0.3 - 0.5e-3, X(64 * 40) - 0.3 - 0.5e-3, X(64 * 30) + 0.5 + 0.25e-3]
    C["b_aligned"] = _case(table(nus, [0.07, 0.07, 0.5]), g, 296.0, 1.0, ow=0.3, hw=1.0,
                           expect=("lo_aligned", "hi_aligned", "W_omega", "W_hw"))
    # a window over the whole grid, centres left and right of the grid (windows reaching in)
    g = grid(1000.0, 1e-3, 3000)
    C["b_outside"] = _case(table([at(g, 1500), g[0] - 1.0, g[1] + 1.0]), g, 296.0, 1.0,
                           expect=("covers_grid", "centre_left", "centre_right"))
    # centres 0.9e8 and 1.2e8 points outside the grid, OmegaWing reaching in: the prologue clamps the local centre index
    # at 1e8 points outside
    g = grid(5000.0, 1e-5, 4096)
    C["b_far_centre"] = _case(table([5000.0 - 1200.0, 5000.0 - 900.0, 5000.0 + 900.0, 5000.0 + 1200.0]), g, 296.0, 1.0,
                              ow=1250.0, expect=("i0_clamped", "W_omega"))

    # c. list capacities and rounds: a comb 0.01 cm^-1 apart (10 points), windows 2.5 cm^-1: ~600 candidates per tile
    # (under RTX_SPLIT_MIN), > 32 edge-only lines and > 16 entries in one wave round, several rounds, > 8 tile-level,
    # full and partial members in a round with a ragged last group
    g = grid(1000.0, 1e-3, 8 * 1024)
    C["c_comb"] = _case(table(np.arange(997.0, 1011.2, 0.01) + 2.5e-4, 0.05), g, 296.0, 1.0,
                        expect=("edge_overflow", "entry_overflow", "rounds", "tile_ragged", "full_ragged",
                                "partial_ragged", "edge_only", "entry", "!hot_plain"))

    # d. hot tiles: a comb 0.005 cm^-1 apart under 4 cm^-1 windows (OmegaWing): ~1800 candidates per tile, cut into
    # parts, on a pressure-broadened layer and a SMALLY layer (y = 0.2) of the same call
    g = grid(1000.0, 1e-3, 6 * 1024)
    C["d_hot"] = _case(table(np.arange(996.5, 1009.7, 0.005) + 2.5e-4), g, 296.0, (1.0, 0.005), ow=4.0,
                       expect=("hot_plain", "hot_smally", "rounds", "tile", "full", "partial", "band_w64"))
    return C


CASES = _cases()
PATH_CASES = sorted(k for k in CASES if k[0] in "abcd")  # cases a-d: the ones the scatter cross-check repeats
