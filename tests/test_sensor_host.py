"""CPU census of tests/sensor_cases.py (the configurations of tests/test_gpu_sensor_paths.py): the dispatch rules of the
drivers in radtxfr_amd/csrc/rtx_radiance.hip restated in a few lines of Python each, with their constants read from the
source. Every case must reach the paths it names, and every path of sensor_cases.PATHS must have a case: a constant that
moves fails here, on a CPU, instead of silently taking a case off its path. No GPU."""
import os
import re

import numpy as np

import sensor_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "radtxfr_amd", "csrc", "rtx_radiance.hip")).read()


def constants(src=SRC):
    one = lambda pat: re.search(pat, src).group(1)
    define = lambda name: int(one(r"#define %s (\d+)" % name))
    return dict(ILS_CH=define("ILS_CH"), ILS_SLOTS_TRI=define("ILS_SLOTS_TRI"), ILS_SLOTS_GAUSS=define("ILS_SLOTS_GAUSS"),
                ILS_MIN_WORK=float(one(r"\(double\)nx \* \(double\)nS >= ([0-9.]+e[0-9]+)")),
                RAD_LDS_MAX=int(one(r"if \(lds > (\d+) \* 1024\) RTX_FAIL")) * 1024,
                RAD_LDS_ATTR=int(one(r"if \(lds > (\d+) \* 1024\)\s*\n\s*RTX_HIP\(hipFuncSetAttribute")) * 1024,
                CUBE_TAB_LDS=int(one(r"if \(tab_bytes <= (\d+) \* 1024\)")) * 1024,
                CUBE_STAGE_MIX=define("CUBE_STAGE_MIX"), BBM_SEGS=define("BBM_SEGS"), CUBE_PB=define("CUBE_PB"))


K = constants()

# the literal rules restated below without a named constant: the restatement is void if one of these lines changes
RULES = (
    "const bool aligned16 = (nE % 4 == 0) && (((uintptr_t)emis | (uintptr_t)L | (uintptr_t)Ls) % 16 == 0);",
    "if (nA == 1 && nT == 1 && dT == nullptr && aligned16) {",
    "const long long blocks = rows4 < 256 * 32 ? rows4 : 256 * 32;",
    "for (long long q0 = 0; q0 < nE4; q0 += 512) {",
    "const size_t lds = sizeof(float) * (size_t)(nAT + 3 * nA);",
    "while (log2TA < 8 && (2LL << log2TA) <= nAT) ++log2TA;",
    "long long bx = nX < 4096 ? nX : 4096;",
    "long long chunks = (2048 + bx - 1) / bx;",
    "if (nS <= 4) hipLaunchKernelGGL(ils_points_kernel<4>",
    "else if (nS <= 16) hipLaunchKernelGGL(ils_points_kernel<16>",
    "else if (nS % 4 == 0 && ldY % 4 == 0 && (((uintptr_t)Y | (uintptr_t)Y_out) % 16 == 0)) {",
    "if (one_pass && nx >= (long long)nB * 2 * ILS_CH && (double)nx * (double)nS >= 3.0e7 && n_chunks < (1 << 20)) {",
    "if (!dead && c + R > x_lo && c - R < x_hi) { atomicMin(&s_b0, b); atomicMax(&s_b1, b); }",
    "const bool vec = (a.nS % 4 == 0) && ((((uintptr_t)a.F | (uintptr_t)a.out) & 15) == 0);",
    "constexpr int R = 64;  // grid points per workgroup-iteration",
    "for (long long q0 = 0; q0 < nS4; q0 += 256) {",
    "const long long blocks = groups < 256 * 16 ? groups : 256 * 16;",
    "const size_t tab_bytes = (size_t)a.nEnd * (Q + 1) * 64 * sizeof(float);",
    "const bool staged = a.nMix <= CUBE_STAGE_MIX;",
    "const double R = KIND == 0 ? s : 14.0 * s;",
    "for (long long base = jj_first; base <= jj_last; base += BBM_SEGS) {",
)


# ------------------------------------------------------------------------------------------------ the restatements
def rad_dispatch(c, K=K):
    """rtx_apparent_radiance: kernel, launch geometry and the labels of sensor_cases.PATHS the call reaches."""
    nX, nE, nA, has_dT = c["nX"], c["nE"], c["nA"], c["nT"] > 0
    nT = c["nT"] if has_dT else 1
    off = c["off"]
    ptr_ok = off["emis"] % 4 == 0 and off["L"] % 4 == 0 and (not c["Ls"] or off["Ls"] % 4 == 0)
    aligned16 = nE % 4 == 0 and ptr_ok
    d, lab = {}, set()
    if nA == 1 and nT == 1 and not has_dT and aligned16:
        rows4 = (nX + 3) // 4
        d.update(kernel="row", blocks=min(rows4, 256 * 32))
        lab.add("rad_row")
        if nE // 4 > 512: lab.add("rad_row_q0_second")
        if nX % 4: lab.add("rad_row_wave_tail")
        if rows4 > d["blocks"]: lab.add("rad_row_grid_stride")
        if c["Ls"]: lab.add("rad_row_Ls")
        return d, lab
    nAT = nA * nT
    lds = 4 * (nAT + 3 * nA)
    d.update(kernel="general", lds=lds)
    if lds > K["RAD_LDS_MAX"]:
        d["kernel"] = "refused"
        return d, {"rad_lds_refused"}
    log2TA = 0
    while log2TA < 8 and (2 << log2TA) <= nAT:
        log2TA += 1
    bx = min(nX, 4096)
    chunks = max(1, min((2048 + bx - 1) // bx, nE))
    e_chunk = (nE + chunks - 1) // chunks
    chunks = (nE + e_chunk - 1) // e_chunk
    TA = 1 << log2TA
    d.update(log2TA=log2TA, bx=bx, chunks=chunks, e_chunk=e_chunk)
    lab |= {"rad_general", "rad_log2TA_%d" % log2TA}
    if nA == 1 and not has_dT:
        if nE % 4: lab.add("rad_fallback_nE")
        if off["emis"] % 4: lab.add("rad_fallback_emis")
        if off["L"] % 4 or (c["Ls"] and off["Ls"] % 4): lab.add("rad_fallback_L")
    if has_dT: lab.add("rad_general_dT")
    if nAT % TA: lab.add("rad_TA_gt_nAT_tail")                     # the last pass over the [nA][nT] slab is ragged
    if TA >= 2 * nT and nAT > TA: lab.add("rad_multi_atm_step")    # `while (it >= nT)` runs twice or more, and is used
    if nX > bx: lab.add("rad_general_grid_stride")
    if chunks > 1 and e_chunk == 1: lab.add("rad_chunks_of_one")
    if chunks > 1 and nE % e_chunk: lab.add("rad_chunks_ragged")
    if lds > K["RAD_LDS_ATTR"]: lab.add("rad_lds_attr")
    return d, lab


def ils_kernel(nx, nS, ldY, nB, offY, offOut, K=K):
    if nS <= 4: return "points4"
    if nS <= 16: return "points16"
    if nS % 4 == 0 and ldY % 4 == 0 and offY % 4 == 0 and offOut % 4 == 0:
        n_chunks = (nx + K["ILS_CH"] - 1) // K["ILS_CH"]
        if nx >= nB * 2 * K["ILS_CH"] and float(nx) * float(nS) >= K["ILS_MIN_WORK"] and n_chunks < (1 << 20):
            return "rows"
        return "columns4"
    return "columns"


def ils_small_labels(c, K=K):
    _, X = SC.ils_axis(c["axis"], c["nx"])
    centre, sigma = SC.ils_small_bands(X, c["kind"])
    k = ils_kernel(c["nx"], c["nS"], c["ldY"], centre.size, c["off"]["Y"], c["off"]["out"], K)
    lab = {"ils_" + k}
    n = [hi - lo for lo, hi in (SC.ils_support(X, cc, SC.ils_reach(c["kind"], ss)) for cc, ss in zip(centre, sigma))]
    if 1 in n: lab.add("ils_one_point")
    if 0 in n: lab.add("ils_no_point")
    fits4 = c["nS"] > 16 and c["nS"] % 4 == 0
    if k == "columns" and fits4 and c["ldY"] % 4 == 0: lab.add("ils_columns_misaligned")
    if k == "columns" and fits4 and c["ldY"] % 4: lab.add("ils_columns_ld_odd")
    if k == "columns4" and c["ldY"] > c["nS"]: lab.add("ils_columns4_strided")
    if k.startswith("points") and c["ldY"] > c["nS"]: lab.add("ils_points_strided")
    return lab


def ils_rows_census(c, K=K):
    """The one-pass form: kernel, chunks, the bands active per chunk (first .. last band that meets it) against the slots."""
    CH = K["ILS_CH"]
    _, X = SC.ils_rows_axis(c["nx"])
    centre, sigma = SC.ils_rows_bands(X, c["kind"]) if c["bands"] == "paths" else SC.ils_rows_overflow_bands(X)
    R = np.array([SC.ils_reach(c["kind"], s) for s in sigma])
    k = ils_kernel(c["nx"], c["nS"], c["nS"], centre.size, 0, 0, K)
    lab = {"ils_" + k}
    n_chunks = (c["nx"] + CH - 1) // CH
    slots = K["ILS_SLOTS_TRI"] if c["kind"] == 0 else K["ILS_SLOTS_GAUSS"]
    n_act = []
    for ch in range(n_chunks):
        x_lo, x_hi = X[ch * CH], X[min(ch * CH + CH, c["nx"]) - 1]
        act = np.nonzero((centre + R > x_lo) & (centre - R < x_hi))[0]
        n_act.append(int(act[-1] - act[0] + 1) if act.size else 0)
    if max(n_act) > slots: lab.add("ils_rows_overflow")
    if c["kind"] == 1: lab.add("ils_rows_gauss")
    for cc, rr in zip(centre, R):
        lo, hi = SC.ils_support(X, cc, rr)
        c0, c1 = lo // CH, (hi - 1) // CH
        if c0 == c1 and lo % CH and hi % CH: lab.add("ils_rows_inside_chunk")
        if hi % CH == 0 and hi < c["nx"]: lab.add("ils_rows_ends_on_boundary")
        if hi % CH == 1: lab.add("ils_rows_ends_after_boundary")
        if hi % CH == CH - 1: lab.add("ils_rows_ends_before_boundary")
        if c1 - c0 == 2: lab.add("ils_rows_three_chunks")
        if lo == 0: lab.add("ils_rows_row0")
        if hi == c["nx"]:
            lab.add("ils_rows_last_chunk")
            if c["nx"] % CH: lab.add("ils_rows_ragged_chunk")
    return dict(kernel=k, n_chunks=n_chunks, n_act=n_act, slots=slots), lab


def interp_labels(c):
    _, X = SC.interp_axis(c)
    Xk = SC.interp_knots_axis(c["knots"])
    vec = c["nS"] % 4 == 0 and c["off"]["F"] % 4 == 0 and c["off"]["out"] % 4 == 0
    lab = {"interp_vector"} if vec else {"interp_scalar_nS" if c["nS"] % 4 else "interp_scalar_misaligned"}
    if vec and c["nS"] // 4 > 256: lab.add("interp_second_block")
    if (c["nx"] + 63) // 64 > 256 * 16: lab.add("interp_grid_stride")
    if c["explicit"]: lab.add("interp_explicit_X")
    if c["nx"] % 64: lab.add("interp_ragged_group")
    if X[0] < Xk[0] and X[-1] > Xk[-1]: lab.add("interp_outside_knots")
    if np.isin(Xk, X).sum() >= 2: lab.add("interp_on_knots")
    if Xk.size == 2: lab.add("interp_two_knots")
    return lab


def bbm_census(knots, kind, K=K):
    """Per band: support [lo, hi), knot intervals jj_first .. jj_last (-1: left of the first knot, nk - 1: right of the
    last), rounds of BBM_SEGS intervals, intervals without a grid point; and the labels."""
    X, Xk = SC.bbm_axis(), SC.bbm_knot_sets()[knots]
    centre, sigma, _ = SC.bbm_bands(knots, kind)
    out = []
    for c, s in zip(centre, sigma):
        lo, hi = SC.ils_support(X, c, s if kind == 0 else 14.0 * s)
        d, lab = dict(lo=lo, hi=hi), set()
        if lo == hi:
            lab.add("bbm_no_point")
        else:
            jj = np.searchsorted(Xk, X[lo:hi], side="right") - 1
            n = int(jj[-1] - jj[0] + 1)
            d.update(jj_first=int(jj[0]), jj_last=int(jj[-1]), intervals=n, rounds=-(-n // K["BBM_SEGS"]), empty=n - np.unique(jj).size)
            if n == K["BBM_SEGS"]: lab.add("bbm_one_round")
            if n == K["BBM_SEGS"] + 1: lab.add("bbm_two_rounds")
            if n == 2 * K["BBM_SEGS"] + 1: lab.add("bbm_three_rounds")
            if d["empty"] and d["rounds"] > 1: lab.add("bbm_empty_intervals")
            if jj[0] == -1: lab.add("bbm_left_end")
            if jj[-1] == Xk.size - 1: lab.add("bbm_right_end")
            if np.isin(Xk, X[lo:hi]).any(): lab.add("bbm_knot_on_grid")
        out.append((d, lab))
    return out


def cube_labels(c, K=K):
    d = SC.cube_inputs(c)
    lds = c["nEnd"] * (c["Q"] + 1) * 64 * 4 <= K["CUBE_TAB_LDS"]
    staged = c["nMix"] <= K["CUBE_STAGE_MIX"]
    lab = {"cube_%s_%s" % ("lds" if lds else "global", "staged" if staged else "unstaged")}
    if c["nPix"] > K["CUBE_PB"]: lab.add("cube_two_groups")
    if c["nPix"] % 64: lab.add("cube_ragged_group")
    if (d["kidx"] < 0).any() and (d["kidx"] >= c["nEnd"]).any(): lab.add("cube_kidx_clamped")
    bad = np.nonzero(np.isnan(d["Tpix"]))[0]
    # one NaN pixel with neighbours in its own workgroup (the per-pixel path) and workgroups without one (the fast path)
    if bad.size == 1 and c["nPix"] > 2 * K["CUBE_PB"] and 0 < bad[0] % K["CUBE_PB"] < K["CUBE_PB"] - 1: lab.add("cube_nan_T")
    return lab


def census(K=K):
    """case -> (labels expected, labels reached) over every table of sensor_cases."""
    out = {}
    for n, c in SC.RAD_CASES.items():
        out["rad:" + n] = (c["expect"], rad_dispatch(c, K)[1])
    for n, c in SC.ILS_SMALL.items():
        out["ils:" + n] = (c["expect"], ils_small_labels(c, K))
    for n, c in SC.ILS_ROWS.items():
        out["ils_rows:" + n] = (c["expect"], ils_rows_census(c, K)[1])
    for n, c in SC.INTERP_CASES.items():
        out["interp:" + n] = (c["expect"], interp_labels(c))
    for knots, kind in SC.BBM_CASES:
        for b, ((_, lab), exp) in enumerate(zip(bbm_census(knots, kind, K), SC.bbm_bands(knots, kind)[2])):
            out["bbm:%s:%d:%d" % (knots, kind, b)] = (exp, lab)
    for n, c in SC.CUBE_CASES.items():
        out["cube:" + n] = (c["expect"], cube_labels(c, K))
    return out


def misses(cen):
    bad = []
    for name, (expect, got) in cen.items():
        bad += [(name, e) for e in expect if (e[1:] in got if e.startswith("!") else e not in got)]
    return bad


# ------------------------------------------------------------------------------------------------------------ tests
def test_constants_are_the_ones_the_cases_were_laid_out_for():
    assert K == SC.CONSTANTS
    for rule in RULES:
        assert rule in SRC, rule


def test_every_case_reaches_the_paths_it_names():
    assert misses(census()) == []


def test_every_path_has_a_case():
    cen = census()
    reached = set().union(*[set(e for e in expect if not e.startswith("!")) & got for expect, got in cen.values()])
    assert sorted(set(SC.PATHS) - reached) == []
    named = set(e.lstrip("!") for expect, _ in cen.values() for e in expect)
    assert sorted(named - set(SC.PATHS)) == [], "a case names a path that is not in PATHS"
    print("sensor census: %d cases, %d paths, all covered" % (len(cen), len(SC.PATHS)))


def test_a_moved_constant_takes_a_case_off_its_path():
    """Each constant read from the source, moved past the nearest case that leans on it (the moves listed: some in both
    directions, ILS_SLOTS_TRI, ILS_SLOTS_GAUSS, ILS_MIN_WORK and RAD_LDS_ATTR in one), leaves some case off the path it
    names. A smaller move keeps every case on its path and is caught by the equality with sensor_cases.CONSTANTS alone."""
    moves = dict(ILS_CH=(1023, 1025, 512, 2048), ILS_SLOTS_TRI=(14,), ILS_SLOTS_GAUSS=(0,), ILS_MIN_WORK=(3.02e7,),
                 RAD_LDS_MAX=(66 * 1024, 160 * 1024), RAD_LDS_ATTR=(67 * 1024,), CUBE_TAB_LDS=(40 * 1024 - 1, 52 * 1024),
                 CUBE_STAGE_MIX=(3, 5), BBM_SEGS=(15, 17), CUBE_PB=(128, 512))
    assert set(moves) == set(K)
    for name, values in moves.items():
        for v in values:
            assert misses(census(dict(K, **{name: v}))), (name, v)


def test_radiance_geometry_of_the_named_cases():
    """The numbers the issue names: five chunks of one emissivity, a ragged last chunk, LDS just over 64 KiB, the refusal."""
    d = lambda n: rad_dispatch(SC.RAD_CASES[n])[0]
    assert (d("gen_chunks_of_one")["chunks"], d("gen_chunks_of_one")["e_chunk"]) == (5, 1)
    assert (d("gen_chunks_ragged")["chunks"], d("gen_chunks_ragged")["e_chunk"]) == (1025, 2)
    assert K["RAD_LDS_ATTR"] < d("gen_lds_attr")["lds"] == 4 * (130 * 128 + 390) <= K["RAD_LDS_MAX"]
    assert d("gen_lds_refused")["lds"] > K["RAD_LDS_MAX"]
    assert d("gen_nX4100")["bx"] == 4096 and d("row_nX32771")["blocks"] == 8192
    assert [d(n)["log2TA"] for n in ("gen_dT_nT1", "gen_nAT3", "gen_nAT255", "gen_nAT256", "gen_nAT257", "gen_TA256_walk")] == [0, 1, 7, 8, 8, 8]
    for nX, nE, nA, nT in SC.RAD_ZERO_SIZES:
        assert nX * nE * nA * (1 if nT is None else nT) == 0


def test_ils_rows_chunks_and_slots():
    for name, c in SC.ILS_ROWS.items():
        d, _ = ils_rows_census(c)
        assert d["kernel"] == "rows" and d["n_chunks"] == -(-c["nx"] // 1024), name
        assert float(c["nx"]) * c["nS"] >= K["ILS_MIN_WORK"] > float(d["n_chunks"] - 1) * 1024 * c["nS"], name  # one chunk less: another kernel
        if c["bands"] == "overflow":
            assert max(d["n_act"]) == 14 > d["slots"] and d["n_act"].index(14) == 5, name
        else:
            assert 1 <= max(d["n_act"]) <= 2, (name, max(d["n_act"]))
    assert all(0 <= col < SC.ILS_ROWS_NS for col in SC.ILS_ROWS_COLS) and len(SC.ILS_ROWS_COLS) >= 8
    assert SC.ILS_ROWS_COLS[0] == 0 and SC.ILS_ROWS_COLS[-1] == SC.ILS_ROWS_NS - 1
    assert any(col // 4 >= 64 for col in SC.ILS_ROWS_COLS)  # a column of the last 64-float4 block


def test_band_moment_intervals_and_shards():
    for (knots, b), n in SC.BBM_INTERVALS.items():
        for kind in (0, 1):
            assert bbm_census(knots, kind)[b][0]["intervals"] == n, (knots, b, kind)
    for kind in (0, 1):
        cen = bbm_census("dense", kind)
        assert cen[0][0]["rounds"] >= 3 and cen[0][0]["empty"] > cen[0][0]["intervals"] // 2
        d = bbm_census("on_grid", kind)[SC.BBM_SHARD_BAND][0]
        for off, n in SC.BBM_SHARDS:
            assert off < d["lo"] and d["hi"] < off + n and off + n <= SC.BBM_GRID[2]
        assert len(set(off % 64 for off, _ in SC.BBM_SHARDS)) == len(SC.BBM_SHARDS)  # the shards start at different phases


def test_chebyshev_lagrange_for_every_Q():
    """The node tables of rtx_band_basis_moments / rtx_pixel_cube for Q = 1 .. 6 (CUBE_QMAX): l_q(s_r) = delta_qr. Q = 1
    (one node, the constant 1) used to raise: np.poly of no roots is a scalar."""
    from radtxfr_amd import sensor
    for Q in range(1, 7):
        s, coef = sensor.chebyshev_lagrange(Q)
        assert s.shape == (Q,) and coef.shape == (Q, Q)
        V = np.array([[np.polyval(coef[q][::-1], x) for x in s] for q in range(Q)])
        assert np.allclose(V, np.eye(Q), atol=1e-12), Q


def test_case_axes_are_the_kernels_grid():
    """sensor_cases.grid_axis is engine.Grid.axis (the kernels' grid_x), bit for bit, also on a shard: a knot copied from it
    is a grid point on the device too."""
    from radtxfr_amd import engine
    for xmin, xmax, n in (SC.INTERP_GRID, SC.BBM_GRID, SC.ils_rows_axis(65436)[0][:3], SC.ils_axis("uniform", 3000)[0][:3]):
        assert np.array_equal(SC.grid_axis(xmin, xmax, n), engine.Grid(xmin, xmax, n).axis())
    c = SC.INTERP_CASES["on_knots"]
    g, X = SC.interp_axis(c)
    assert np.array_equal(X, engine.Grid(*g).axis()) and np.isin(SC.interp_knots_axis("on_grid"), X).sum() >= 20
