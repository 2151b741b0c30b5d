"""Shapes, alignments and band / knot lists that put the sensor stage (radtxfr_amd/csrc/rtx_radiance.hip) on one path at a
time. Imported by the GPU test (tests/test_gpu_sensor_paths.py: every case against an fp64 reference, element by element)
and by the host census (tests/test_sensor_host.py: each case reaches the paths it names in `expect`, by a restatement of
the drivers' dispatch rules whose constants are read from the source), so the two cannot drift apart.

NumPy only, fixed seeds. Alignment is part of a case: `off` gives, per pointer, the offset in floats of its first
element from a 16-byte boundary (0: aligned; 1: a contiguous view that starts one float into a larger flat buffer).
All inputs are strictly positive (emissivities in [0, 1]) so that no result is a cancelled difference."""
import numpy as np

# the values of the source constants the cases were laid out for (the census compares them with the source)
CONSTANTS = dict(ILS_CH=1024, ILS_SLOTS_TRI=12, ILS_SLOTS_GAUSS=24, ILS_MIN_WORK=3.0e7, RAD_LDS_MAX=150 * 1024,
                 RAD_LDS_ATTR=64 * 1024, CUBE_TAB_LDS=40 * 1024, CUBE_STAGE_MIX=4, BBM_SEGS=16, CUBE_PB=256)

# every path the census must find at least one case on
PATHS = (
    # rtx_apparent_radiance
    "rad_row", "rad_row_q0_second", "rad_row_wave_tail", "rad_row_grid_stride", "rad_row_Ls", "rad_general", "rad_fallback_nE",
    "rad_fallback_emis", "rad_fallback_L", "rad_general_dT", "rad_log2TA_0", "rad_log2TA_1", "rad_log2TA_7", "rad_log2TA_8",
    "rad_TA_gt_nAT_tail", "rad_multi_atm_step", "rad_general_grid_stride", "rad_chunks_of_one", "rad_chunks_ragged",
    "rad_lds_attr", "rad_lds_refused",
    # rtx_ils
    "ils_points4", "ils_points16", "ils_columns", "ils_columns4", "ils_rows", "ils_columns_misaligned", "ils_columns_ld_odd",
    "ils_columns4_strided", "ils_points_strided", "ils_one_point", "ils_no_point", "ils_rows_inside_chunk",
    "ils_rows_ends_on_boundary", "ils_rows_ends_after_boundary", "ils_rows_ends_before_boundary", "ils_rows_three_chunks",
    "ils_rows_row0", "ils_rows_last_chunk", "ils_rows_ragged_chunk", "ils_rows_overflow", "ils_rows_gauss",
    # rtx_interp_knots
    "interp_vector", "interp_scalar_nS", "interp_scalar_misaligned", "interp_second_block", "interp_grid_stride",
    "interp_explicit_X", "interp_ragged_group", "interp_outside_knots", "interp_on_knots", "interp_two_knots",
    # band moments
    "bbm_one_round", "bbm_two_rounds", "bbm_three_rounds", "bbm_empty_intervals", "bbm_left_end", "bbm_right_end",
    "bbm_knot_on_grid", "bbm_no_point",
    # rtx_pixel_cube
    "cube_lds_staged", "cube_lds_unstaged", "cube_global_staged", "cube_global_unstaged", "cube_two_groups",
    "cube_ragged_group", "cube_kidx_clamped", "cube_nan_T",
)


def grid_axis(xmin, xmax, n_total):
    """The wavenumbers of a uniform grid as the kernels form them (grid_x in rtx_common.h, engine.Grid.axis): index * step
    + xmin in two roundings, the last point pinned to xmax. A knot copied from here is a grid point to the last bit."""
    step = (float(xmax) - float(xmin)) / (n_total - 1)
    X = np.arange(n_total, dtype=np.float64) * step + float(xmin)
    X[-1] = xmax
    return X


# ------------------------------------------------------------------------------------------- rtx_apparent_radiance
def _rad(nX, nE, nA=1, nT=0, Ls=False, off=None, expect=()):
    """nT = 0: no dT axis. off: float offsets of emis, L and Ls from a 16-byte boundary."""
    o = dict(emis=0, L=0, Ls=0)
    o.update(off or {})
    return dict(nX=nX, nE=nE, nA=nA, nT=nT, Ls=Ls, off=o, expect=tuple(expect))


RAD_CASES = {
    # the row kernel: one atmosphere, no dT, nE % 4 == 0, 16-byte aligned emis / L / Ls
    "row_nE4_nX1": _rad(1, 4, expect=("rad_row", "rad_row_wave_tail")),
    "row_nE4_nX3_Ls": _rad(3, 4, Ls=True, expect=("rad_row", "rad_row_wave_tail", "rad_row_Ls")),
    "row_nE4_nX5": _rad(5, 4, expect=("rad_row", "rad_row_wave_tail")),
    "row_nE2048_nX5_Ls": _rad(5, 2048, Ls=True, expect=("rad_row", "!rad_row_q0_second", "rad_row_Ls")),
    "row_nE2052_nX3": _rad(3, 2052, expect=("rad_row", "rad_row_q0_second")),
    "row_nE2052_nX5_Ls": _rad(5, 2052, Ls=True, expect=("rad_row", "rad_row_q0_second", "rad_row_Ls")),
    "row_nX32771": _rad(32771, 4, expect=("rad_row", "rad_row_grid_stride", "rad_row_wave_tail")),
    # one atmosphere, no dT, but the row kernel cannot take it
    "fallback_nE6": _rad(5, 6, expect=("rad_general", "rad_fallback_nE", "rad_log2TA_0")),
    "fallback_emis": _rad(5, 8, off=dict(emis=1), expect=("rad_general", "rad_fallback_emis")),
    "fallback_L": _rad(5, 8, off=dict(L=1), expect=("rad_general", "rad_fallback_L")),
    "fallback_Ls": _rad(5, 8, Ls=True, off=dict(Ls=1), expect=("rad_general", "rad_fallback_L")),
    # the general kernel
    "gen_dT_nT1": _rad(5, 4, nA=1, nT=1, expect=("rad_general", "rad_general_dT", "rad_log2TA_0")),
    "gen_nAT3": _rad(5, 3, nA=3, Ls=True, expect=("rad_general", "rad_log2TA_1", "rad_TA_gt_nAT_tail")),
    "gen_nAT255": _rad(3, 5, nA=85, nT=3, expect=("rad_general", "rad_log2TA_7", "rad_multi_atm_step")),
    "gen_nAT256": _rad(3, 5, nA=16, nT=16, Ls=True, expect=("rad_general", "rad_log2TA_8", "!rad_multi_atm_step")),
    "gen_nAT257": _rad(3, 5, nA=1, nT=257, expect=("rad_general", "rad_log2TA_8")),
    "gen_TA256_walk": _rad(3, 5, nA=50, nT=7, Ls=True, expect=("rad_general", "rad_log2TA_8", "rad_multi_atm_step")),
    "gen_nX4100": _rad(4100, 2, nA=2, expect=("rad_general", "rad_general_grid_stride")),
    "gen_chunks_of_one": _rad(1, 5, nA=2, expect=("rad_general", "rad_chunks_of_one")),
    "gen_chunks_ragged": _rad(1, 2049, nA=2, expect=("rad_general", "rad_chunks_ragged")),
    "gen_lds_attr": _rad(2, 3, nA=130, nT=128, expect=("rad_general", "rad_lds_attr")),
    "gen_lds_refused": _rad(1, 1, nA=200, nT=200, expect=("rad_lds_refused",)),
}
RAD_ZERO_SIZES = ((0, 4, 1, None), (3, 0, 1, None), (3, 4, 0, None), (3, 4, 2, 0), (0, 0, 0, 0))  # (nX, nE, nA, nT); nT None: no dT, 0: a dT of length 0


def rad_inputs(case, seed=11):
    """fp64 X, Ts, dT and fp32 emis, tau, La, Ld of a case (C-contiguous; the test places them at the case's offsets)."""
    r = np.random.default_rng(seed)
    nX, nE, nA, nT = case["nX"], case["nE"], case["nA"], case["nT"]
    X = np.sort(r.uniform(800.0, 1250.0, nX))
    emis = r.uniform(0.0, 1.0, (nX, nE)).astype(np.float32)
    if emis.size:
        emis.flat[0], emis.flat[-1] = 0.0, 1.0
    Ts = r.uniform(270.0, 320.0, nA)
    tau = r.uniform(0.2, 0.95, (nX, nA)).astype(np.float32)
    La = r.uniform(0.5, 3.0, (nX, nA)).astype(np.float32)
    Ld = r.uniform(1.0, 6.0, (nX, nA)).astype(np.float32)
    dT = r.uniform(-5.0, 5.0, nT) if nT else None
    return dict(X=X, emis=emis, Ts=Ts, tau=tau, La=La, Ld=Ld, dT=dT)


# ------------------------------------------------------------------------------------------------------- rtx_ils
def ils_axis(axis, nx, seed=5):
    """axis "uniform": (grid tuple (xmin, xmax, n_total), X); "explicit": (None, X) with uneven ascending steps."""
    if axis == "uniform":
        xmin, step = 1000.0, 0.01
        if nx == 1:  # a grid needs two points: a one-point shard of a two-point grid
            return (xmin, xmin + step, 2, 0, 1), np.array([xmin])
        xmax = xmin + (nx - 1) * step
        return (xmin, xmax, nx, 0, nx), grid_axis(xmin, xmax, nx)
    r = np.random.default_rng(seed)
    return None, 1000.0 + np.cumsum(r.uniform(0.004, 0.016, nx))


def _gap(X, i):
    g = []
    if i > 0:
        g.append(X[i] - X[i - 1])
    if i + 1 < X.size:
        g.append(X[i + 1] - X[i])
    return min(g) if g else 0.01


def band_over_rows(X, lo, hi, kind):
    """(centre, sigma) of the band whose open support covers exactly rows lo..hi (inclusive) of X: its edges lie a
    quarter of the smallest neighbouring gap outside X[lo] and X[hi]. Triangle: R = sigma; Gaussian: R = 7 sigma."""
    R = 0.5 * (X[hi] - X[lo]) + 0.25 * min(_gap(X, lo), _gap(X, hi))
    return 0.5 * (X[lo] + X[hi]), (R if kind == 0 else R / 7.0)


def band_between(X, i):
    """A triangle that covers no point: centred between X[i] and X[i + 1], a quarter of the gap wide."""
    return 0.5 * (X[i] + X[i + 1]), 0.25 * (X[i + 1] - X[i])


def ils_reach(kind, sigma):
    return sigma if kind == 0 else 7.0 * sigma  # bands centred inside the grid only


def ils_support(X, c, R):
    """[lo, hi): the open interval |x - c| < R (the kernels' ils_bound pair)."""
    return int(np.searchsorted(X, c - R, side="right")), int(np.searchsorted(X, c + R, side="left"))


def ils_small_bands(X, kind):
    """Band list of the small-nS cases, by rows: the first and last rows, a single point, 700 rows (three blocks of 256
    rows for the column kernels), a handful; for the triangle also a band that covers no point (NaN in its row)."""
    nx = X.size
    if nx == 1:
        rows = [(0, 0)]
    elif nx == 2:
        rows = [(0, 0), (0, 1), (1, 1)]
    else:
        rows = [(0, 2), (5, 5), (10, 16), (100, 799), (300, 563), (nx - 9, nx - 1)]
    c, s = map(list, zip(*[band_over_rows(X, lo, hi, kind) for lo, hi in rows]))
    if kind == 0 and nx > 2:
        cc, ss = band_between(X, 40)
        c.insert(2, cc), s.insert(2, ss)
    return np.array(c), np.array(s)


def _ils(nS, axis="uniform", nx=3000, kind=0, ld_extra=0, off=0, expect=()):
    return dict(nS=nS, axis=axis, nx=nx, kind=kind, ldY=nS + ld_extra, off=dict(Y=off, out=0), expect=tuple(expect))


ILS_SMALL = {}
for _ax in ("uniform", "explicit"):
    for _nS, _k in ((1, "ils_points4"), (4, "ils_points4"), (5, "ils_points16"), (16, "ils_points16"), (17, "ils_columns"),
                    (20, "ils_columns4"), (64, "ils_columns4"), (68, "ils_columns4"), (130, "ils_columns")):
        ILS_SMALL["tri_%s_nS%d" % (_ax, _nS)] = _ils(_nS, _ax, expect=(_k, "ils_one_point", "ils_no_point"))
    ILS_SMALL["gauss_%s_nS20" % _ax] = _ils(20, _ax, kind=1, expect=("ils_columns4",))
    ILS_SMALL["gauss_%s_nS5" % _ax] = _ils(5, _ax, kind=1, expect=("ils_points16",))
    for _nx in (1, 2):
        ILS_SMALL["tri_%s_nx%d" % (_ax, _nx)] = _ils(20, _ax, nx=_nx, expect=("ils_columns4", "ils_one_point"))
        ILS_SMALL["tri_%s_nx%d_nS3" % (_ax, _nx)] = _ils(3, _ax, nx=_nx, expect=("ils_points4", "ils_one_point"))
# layouts of Y, nS = 20 (and the two point kernels): (case, the contiguous case whose kernel it shares or None)
for _kind, _kn in ((0, "tri"), (1, "gauss")):
    ILS_SMALL[_kn + "_ld_plus4"] = _ils(20, kind=_kind, ld_extra=4, expect=("ils_columns4", "ils_columns4_strided"))
    ILS_SMALL[_kn + "_ld_plus3"] = _ils(20, kind=_kind, ld_extra=3, expect=("ils_columns", "ils_columns_ld_odd"))
    ILS_SMALL[_kn + "_Y_misaligned"] = _ils(20, kind=_kind, off=1, expect=("ils_columns", "ils_columns_misaligned"))
    ILS_SMALL[_kn + "_explicit_ld_plus3"] = _ils(20, "explicit", kind=_kind, ld_extra=3, expect=("ils_columns", "ils_columns_ld_odd"))
ILS_SMALL["tri_points4_strided"] = _ils(4, ld_extra=3, expect=("ils_points4", "ils_points_strided"))
ILS_SMALL["tri_points16_strided"] = _ils(16, ld_extra=5, off=1, expect=("ils_points16", "ils_points_strided"))
# (strided case, contiguous case): same kernel, so the results are the same bits
ILS_SAME_BITS = (("tri_ld_plus4", "tri_uniform_nS20"), ("gauss_ld_plus4", "gauss_uniform_nS20"),
                 ("tri_ld_plus3", "tri_Y_misaligned"), ("gauss_ld_plus3", "gauss_Y_misaligned"),
                 ("tri_points4_strided", "tri_uniform_nS4"), ("tri_points16_strided", "tri_uniform_nS16"))
# (case, case): another kernel on the same data, within the tolerance of each other
ILS_SAME_DATA = (("tri_ld_plus3", "tri_uniform_nS20"), ("tri_Y_misaligned", "tri_uniform_nS20"))

# The one-pass form (ils_rows_kernel + ils_rows_reduce_kernel) at its smallest shape: nx * nS >= 3.0e7 with nS = 460.
# nx = 65536 is 64 full chunks of 1024 rows; nx = 65436 ends in a ragged chunk of 924 rows.
ILS_ROWS_NS = 460
ILS_ROWS_COLS = (0, 1, 3, 127, 255, 256, 258, 457, 459)  # 256.. lie in the second (last) 64-float4 block
ILS_ROWS_NX = (65536, 65436)


def ils_rows_axis(nx):
    xmin, step = 1000.0, 0.01
    xmax = xmin + (nx - 1) * step
    return (xmin, xmax, nx, 0, nx), grid_axis(xmin, xmax, nx)


def ils_rows_band_rows(nx):
    """(first row, last row, path) of the one-pass band list, in ascending order of the centres."""
    last = nx - 1
    return ((0, 299, "ils_rows_row0"),
            (1024 * 3 + 100, 1024 * 3 + 700, "ils_rows_inside_chunk"),
            (1024 * 8 + 500, 1024 * 10 - 1, "ils_rows_ends_on_boundary"),      # support [lo, hi) with hi = 1024 * 10
            (1024 * 14 + 200, 1024 * 15, "ils_rows_ends_after_boundary"),      # hi = 1024 * 15 + 1: one row of chunk 15
            (1024 * 20 + 300, 1024 * 21 - 2, "ils_rows_ends_before_boundary"),  # hi = 1024 * 21 - 1
            (1024 * 30 + 900, 1024 * 32 + 100, "ils_rows_three_chunks"),
            (last - 500, last, "ils_rows_last_chunk"))


def ils_rows_bands(X, kind):
    c, s = zip(*[band_over_rows(X, lo, hi, kind) for lo, hi, _ in ils_rows_band_rows(X.size)])
    return np.array(c), np.array(s)


def ils_rows_overflow_bands(X):
    """14 triangles stacked on chunk 5 (more than the 12 slots), each over its own rows."""
    c, s = zip(*[band_over_rows(X, 1024 * 5 + 10 + 40 * j, 1024 * 5 + 400 + 40 * j, 0) for j in range(14)])
    return np.array(c), np.array(s)


ILS_ROWS = {}
for _nx in ILS_ROWS_NX:
    for _kind, _kn in ((0, "tri"), (1, "gauss")):
        ILS_ROWS["%s_nx%d" % (_kn, _nx)] = dict(
            nx=_nx, nS=ILS_ROWS_NS, kind=_kind, bands="paths",
            expect=("ils_rows", "!ils_rows_overflow") + tuple(p for _, _, p in ils_rows_band_rows(_nx)) +
            (("ils_rows_ragged_chunk",) if _nx % 1024 else ("!ils_rows_ragged_chunk",)) + (("ils_rows_gauss",) if _kind else ()))
ILS_ROWS["tri_overflow"] = dict(nx=65536, nS=ILS_ROWS_NS, kind=0, bands="overflow", expect=("ils_rows", "ils_rows_overflow"))


# ------------------------------------------------------------------------------------------------- rtx_interp_knots
INTERP_GRID = (900.0, 900.0 + 0.01 * 299999, 300000)  # the shards below are cut from this axis


def interp_knots_axis(kind):
    xmin, xmax, n_total = INTERP_GRID
    X = grid_axis(xmin, xmax, n_total)
    if kind == "two":
        return np.array([X[1020] + 0.003, X[1050] + 0.004])
    if kind == "on_grid":  # every knot is a grid point: t = 0 or 1 exactly there
        return X[1000:1200:7].copy()
    if kind == "wide":     # covers the long shard
        return np.linspace(X[900], X[263000], 500) + 0.0031
    return X[1010] + np.cumsum(np.random.default_rng(3).uniform(0.05, 0.4, 9))  # "inner": points left and right of all knots


def _interp(nx, nS, knots="inner", offset=1000, offF=0, explicit=False, expect=()):
    return dict(nx=nx, nS=nS, knots=knots, offset=offset, off=dict(F=offF, out=0), explicit=explicit, expect=tuple(expect))


INTERP_CASES = {
    "nx1": _interp(1, 4, offset=1017, expect=("interp_vector", "interp_ragged_group")),
    "nx63": _interp(63, 4, expect=("interp_vector", "interp_ragged_group")),
    "nx64": _interp(64, 8, expect=("interp_vector", "!interp_ragged_group")),
    "nx65": _interp(65, 3, expect=("interp_scalar_nS", "interp_ragged_group")),
    "nx262209": _interp(262209, 1, knots="wide", offset=800, expect=("interp_scalar_nS", "interp_grid_stride", "interp_outside_knots")),
    "nS1": _interp(200, 1, expect=("interp_scalar_nS", "interp_outside_knots")),
    "nS4": _interp(200, 4, expect=("interp_vector", "interp_outside_knots")),
    "nS1024": _interp(67, 1024, expect=("interp_vector", "!interp_second_block")),
    "nS1028": _interp(67, 1028, expect=("interp_vector", "interp_second_block")),
    "nS1026": _interp(67, 1026, expect=("interp_scalar_nS",)),
    "F_misaligned": _interp(130, 8, offF=1, expect=("interp_scalar_misaligned",)),
    "explicit_X": _interp(150, 8, explicit=True, expect=("interp_vector", "interp_explicit_X", "interp_outside_knots")),
    "explicit_X_scalar": _interp(150, 5, explicit=True, expect=("interp_scalar_nS", "interp_explicit_X")),
    "two_knots": _interp(100, 4, knots="two", expect=("interp_vector", "interp_two_knots", "interp_outside_knots")),
    "on_knots": _interp(260, 4, knots="on_grid", offset=980, expect=("interp_vector", "interp_on_knots", "interp_outside_knots")),
}


def interp_axis(case):
    """(grid tuple, X) of a case; an explicit-X case gets uneven steps of its own."""
    xmin, xmax, n_total = INTERP_GRID
    X = grid_axis(xmin, xmax, n_total)[case["offset"]:case["offset"] + case["nx"]]
    if case["explicit"]:
        X = X[0] + np.cumsum(np.random.default_rng(8).uniform(0.004, 0.03, case["nx"]))
        return None, X
    return (xmin, xmax, n_total, case["offset"], case["nx"]), X


# --------------------------------------------------------------------------------------------------- band moments
BBM_GRID = (900.0, 900.0 + 0.01 * 8191, 8192)
BBM_TS = 301.5


def bbm_axis():
    return grid_axis(*BBM_GRID)


def bbm_knot_sets():
    """"on_grid": 0.25 cm^-1 apart, every knot a grid point, first knot 905, last 975: bands stick out on either side.
    "dense": 0.0037 cm^-1 apart (the grid step is 0.01): most knot intervals hold no grid point."""
    X = bbm_axis()
    return {"on_grid": X[500:7501:25].copy(), "dense": 940.0 + 0.0037 * np.arange(200) + 0.0011}


def bbm_bands(knots, kind):
    """(centre, sigma, paths per band). R = sigma (triangle) or 14 sigma (Gaussian): the same supports for both kinds."""
    X = bbm_axis()
    Xk = bbm_knot_sets()[knots]
    if knots == "on_grid":
        a = Xk[60]
        bands = [(a + 2.0, 1.999, ("bbm_one_round", "bbm_knot_on_grid")),       # 16 intervals
                 (a + 10.125, 2.12, ("bbm_two_rounds", "bbm_knot_on_grid")),    # 17
                 (a + 24.125, 4.12, ("bbm_three_rounds", "bbm_knot_on_grid")),  # 33
                 (Xk[0] - 0.4, 2.5, ("bbm_left_end",)),
                 (Xk[-1] + 0.3, 2.2, ("bbm_right_end",)),
                 (X[4000] + 0.005, 0.003, ("bbm_no_point",)),
                 (X[3000] + 0.002, 3.1, ())]                                    # the band of the shard-invariance test
    else:
        bands = [(940.37, 0.5, ("bbm_empty_intervals", "bbm_left_end", "bbm_right_end")),
                 (940.2, 0.1, ("bbm_empty_intervals",)),
                 (X[4100] + 0.005, 0.003, ("bbm_no_point",))]
    c = np.array([b[0] for b in bands])
    s = np.array([b[1] for b in bands]) / (1.0 if kind == 0 else 14.0)
    return c, s, [b[2] for b in bands]


BBM_INTERVALS = {("on_grid", 0): 16, ("on_grid", 1): 17, ("on_grid", 2): 33}  # (knots, band) -> knot intervals
BBM_SHARD_BAND = 6
BBM_SHARDS = ((2000, 2000), (1003, 5001))  # (offset, n): both hold all of band 6's support (rows 2691 .. 3309)
BBM_CASES = [(knots, kind) for knots in ("on_grid", "dense") for kind in (0, 1)]
BBM_Q = (1, 4, 6)


def bbm_inputs(seed=21):
    r = np.random.default_rng(seed)
    n = BBM_GRID[2]
    return dict(tau=r.uniform(0.3, 0.9, n).astype(np.float32), La=r.uniform(0.5, 1.5, n).astype(np.float32),
                Ld=r.uniform(1.0, 3.0, n).astype(np.float32))


MIX_NE = (1, 255, 256, 257)
MIX_NB, MIX_NK = 5, 40
MIX_JRANGE = np.array([[0, 0], [3, 20], [39, 39], [0, 39], [7, 6]], dtype=np.int32)  # the last: an empty range


# ------------------------------------------------------------------------------------------------- rtx_pixel_cube
def _cube(nPix, nEnd=8, nMix=3, Q=4, nB=70, bad_kidx=False, nan_pixel=None, expect=()):
    return dict(nPix=nPix, nEnd=nEnd, nMix=nMix, Q=Q, nB=nB, bad_kidx=bad_kidx, nan_pixel=nan_pixel, expect=tuple(expect))


CUBE_CASES = {
    "nPix1": _cube(1, expect=("cube_lds_staged", "cube_ragged_group")),
    "nPix64": _cube(64, expect=("cube_lds_staged", "!cube_ragged_group", "!cube_two_groups")),
    "nPix65": _cube(65, expect=("cube_lds_staged", "cube_ragged_group")),
    "nPix256": _cube(256, expect=("cube_lds_staged", "!cube_ragged_group", "!cube_two_groups")),
    "nPix257": _cube(257, expect=("cube_lds_staged", "cube_two_groups", "cube_ragged_group")),
    "unstaged": _cube(257, nMix=5, expect=("cube_lds_unstaged",)),
    "global_staged": _cube(65, nEnd=40, nMix=4, expect=("cube_global_staged",)),
    "global_unstaged": _cube(65, nEnd=40, nMix=5, Q=6, expect=("cube_global_unstaged",)),
    "lds_largest": _cube(65, nEnd=32, nMix=2, expect=("cube_lds_staged",)),
    "Q1": _cube(65, Q=1, nB=3, expect=("cube_lds_staged",)),
    "kidx_staged": _cube(257, bad_kidx=True, expect=("cube_lds_staged", "cube_kidx_clamped")),
    "kidx_unstaged": _cube(65, nEnd=40, nMix=5, bad_kidx=True, expect=("cube_global_unstaged", "cube_kidx_clamped")),
    "nan_T": _cube(600, nan_pixel=300, expect=("cube_lds_staged", "cube_nan_T")),
}


def cube_inputs(case, seed=31):
    """Tables as rtx_band_mix_stacked would leave them, but all positive: tab [nEnd][Q+1][nB], N, C [nB]; the scene."""
    r = np.random.default_rng(seed)
    nB, Q, nEnd, nPix, nMix = case["nB"], case["Q"], case["nEnd"], case["nPix"], case["nMix"]
    centre = np.linspace(780.0, 1300.0, nB) if nB > 1 else np.array([1000.0])
    sigma = r.uniform(2.0, 6.0, nB)
    s_node = np.cos((2 * np.arange(Q) + 1) * np.pi / (2 * Q)).astype(np.float32)
    tab = r.uniform(0.5, 1.5, (nEnd, Q + 1, nB)).astype(np.float32)
    tab[:, Q, :] *= 0.5  # the Ld table, subtracted: well below sum_q B tab_q (B ~ 3 .. 15)
    kidx = r.integers(0, nEnd, (nPix, nMix)).astype(np.int32)
    if case["bad_kidx"]:
        kidx[::3, 0] = -1
        kidx[1::4, nMix - 1] = nEnd
        kidx[nPix - 1, :] = nEnd + 5
    frac = r.uniform(0.1, 1.0, (nPix, nMix)).astype(np.float32)
    Tpix = r.uniform(270.0, 330.0, nPix)
    if case["nan_pixel"] is not None:
        Tpix[case["nan_pixel"]] = np.nan
    return dict(centre=centre, sigma=sigma, s_node=s_node, tab=tab, kidx=kidx, frac=frac, Tpix=Tpix,
                N=r.uniform(50.0, 150.0, nB).astype(np.float32), C=r.uniform(10.0, 50.0, nB).astype(np.float32))
