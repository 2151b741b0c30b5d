"""CPU-only checks of tests/srf_axis_cases.py, the cases tests/test_gpu_srf_axis_paths.py runs the response-table sensor
kernels on: that they reach every path the kernels cut the spectral axis into (a census in integer NumPy of what
srf_rows_kernel, srfm_chunk_kernel, srfm_reduce_kernel and their adjoint and tangent twins would do), that the fp64 oracles
agree with each other on every one of them, and that a kernel wrong in one of six plausible ways would be caught there with
a margin of 4 over the GPU test's bound."""
import os

import numpy as np
import pytest

from oracle import cpu_ref as ref

import srf_fused_cases as FC
import sensor_vjp_cases as VC
import srf_axis_cases as AC
from test_gpu_srf import cells
from test_gpu_srf_fused import TOL as TOL_L
from test_gpu_sensor_vjp import K_DE, EPS

CH = AC.CH_HOST
SUB = AC.SUB
REL_NC = 1e-6   # N and C of the moments: test_gpu_srf_fused.py::test_moments
MARGIN = 4.0
CASES = AC.all_cases(CH)
ids = lambda cs: ["off%d-n%d-%s" % c[:3] for c in cs]


def test_chunk_constants_are_the_library_s():
    """CH_HOST, SUB and SLOTS are what the sources define (the GPU test takes CH from rtx_srf_chunk_points())."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = open(os.path.join(root, "radtxfr_amd", "csrc", "rtx_srf_common.h")).read()
    srf = open(os.path.join(root, "radtxfr_amd", "csrc", "rtx_srf.hip")).read()
    jvp = open(os.path.join(root, "radtxfr_amd", "csrc", "rtx_srf_jvp.hip")).read()
    assert "#define SRF_CH %d " % CH in common and "#define SRF_SLOTS %d " % AC.SLOTS in common
    assert "#define SRFM_SUB %d " % SUB in srf and "#define SRFJ_SUB %d " % SUB in jvp


# ---------------------------------------------------------------------------------------------------------- census
def census(c):
    """The classes of work one case gives the kernels, as strings, from integer arithmetic on the axis alone."""
    X, Xk, n, nk = c["X"], c["Xk"], c["X"].size, c["Xk"].size
    seen = set()
    chunks, subs = -(-n // CH), -(-n // SUB)
    seen |= {"chunks=%d" % chunks, "subs=%d" % subs, "ragged_sub" if n % SUB else "full_last_sub",
             "rows%4!=0" if n % 4 else "rows%4==0", "groups=%d" % -(-len(c["tables"]) // AC.SLOTS),
             "last_chunk=%s" % {1: "1", CH: "CH", CH - 1: "CH-1"}.get(n - (chunks - 1) * CH, "other")}
    cnt = np.searchsorted(Xk, X, side="right")
    j0 = np.maximum(cnt - 1, 0)
    first = SUB * np.arange(subs)
    last = np.minimum(first + SUB, n) - 1
    ja, jb = j0[first], np.minimum(j0[last] + 1, nk - 1)
    kn = jb - ja + 1
    assert np.all(kn >= 1) and np.all(jb[:-1] <= ja[1:] + 1)  # the workspace layout j + 2 s: no two sub-chunks share an element
    for k in kn:
        seen.add("sub_knots=%s" % ("1" if k == 1 else "2" if k == 2 else "3..255" if k < 256 else ">=256"))
    for b, (xk, _) in enumerate(c["tables"]):
        lo, hi = np.searchsorted(X, xk[0], side="left"), np.searchsorted(X, xk[-1], side="right")
        assert (hi <= lo) == bool(c["dead"][b])
        if hi <= lo:
            seen.add("dead_band")
            continue
        if b >= AC.SLOTS:
            seen.add("live_band_in_group_2")
        per = [max(0, min(hi, (ch + 1) * CH, n) - max(lo, ch * CH)) for ch in range(chunks)]
        reached = [r for r in per if r]
        if len(reached) < chunks:
            seen.add("band_skips_a_chunk")
        if reached == [1, 1]:
            seen.add("band_one_row_each_side_of_a_chunk_cut")
        if hi - lo == 2 and lo % SUB == SUB - 1:
            seen.add("band_one_row_each_side_of_a_sub_cut")
        for r in reached:
            seen.add("band_rows_in_chunk=%s" % ("1" if r == 1 else "2" if r == 2 else "CH" if r == CH else "some"))
        if hi - lo == 1:
            seen.add("one_row_band_at_%s" % {0: "row0", n - 1: "last_row"}.get(lo, "sub%d_row%d" % (min(lo // SUB, 2), lo % SUB)
                                                                               if lo % SUB in (0, SUB - 1) else "other"))
        if X[lo] == xk[0] and X[hi - 1] == xk[-1]:
            seen.add("band_end_knots_on_grid_points")
        # srfm_chunk_kernel's tasks: (sub-chunk the band reaches, knot it touches); rows of the task: lower knot jk - 1 or jk
        for s in range(lo // SUB, (hi - 1) // SUB + 1):
            b0, b1 = max(SUB * s, lo), min(SUB * (s + 1), hi)
            rows_j0 = j0[b0:b1]
            empty = sum(1 for jk in range(ja[s], jb[s] + 1) if not np.any((rows_j0 == jk) | (rows_j0 == jk - 1)))
            if empty:
                seen.add("task_without_rows")
            if empty >= 256:
                seen.add("sub_chunk_with_256_empty_tasks")
        jr = c["jrange"][b]
        # srfm_reduce_kernel's two cuts of a knot's sub-chunk range
        for jk in range(jr[0], jr[1] + 1):
            if jk >= 2 and np.searchsorted(X, Xk[jk - 1], side="left") // SUB > lo // SUB:
                seen.add("reduce_lower_cut_binds")
            if jk <= nk - 2:
                p = np.searchsorted(X, Xk[jk + 1], side="left")
                if p > 0 and (p - 1) // SUB < (hi - 1) // SUB:
                    seen.add("reduce_upper_cut_binds")
    if np.all(cnt == 0):
        seen.add("all_points_below_the_knots")
    if np.all(cnt == nk):
        seen.add("all_points_above_the_knots")
    if np.any(np.isin(X[[r for pair in AC.cuts(CH, n) for r in pair]], Xk)):
        seen.add("knot_on_a_cut_row")
    return seen


def test_path_census():
    """Every class of axis shape, band placement and knot placement the issue names occurs in the case set."""
    seen = set()
    for off, n, knots, _, _ in CASES:
        c = AC.case(CH, off, n, knots)
        s = census(c)
        seen |= s
        seen |= {"shard" if off else "whole_grid"}
        if knots == "cluster":
            assert "sub_knots=>=256" in s and "sub_chunk_with_256_empty_tasks" in s, (off, n)
        live = ~c["dead"]
        nk = c["Xk"].size
        if knots == "all_below":
            assert np.all(c["jrange"][live] == (nk - 1, nk - 1))
        if knots in ("all_above", "one_inside", "one_below"):
            assert np.all(c["jrange"][live] == (0, 0))
        assert np.all(c["jrange"][~live] == (0, -1))
    need = {"chunks=1", "chunks=2", "chunks=3", "subs=1", "subs=2", "subs=3", "subs=16", "subs=17", "subs=32", "subs=33",
            "ragged_sub", "full_last_sub", "rows%4!=0", "rows%4==0", "groups=1", "groups=2", "last_chunk=1", "last_chunk=CH",
            "last_chunk=CH-1", "last_chunk=other", "sub_knots=1", "sub_knots=2", "sub_knots=3..255", "sub_knots=>=256",
            "dead_band", "live_band_in_group_2", "band_skips_a_chunk", "band_one_row_each_side_of_a_chunk_cut",
            "band_one_row_each_side_of_a_sub_cut", "band_rows_in_chunk=1", "band_rows_in_chunk=2", "band_rows_in_chunk=CH",
            "band_rows_in_chunk=some", "one_row_band_at_row0", "one_row_band_at_last_row", "one_row_band_at_sub0_row63",
            "one_row_band_at_sub1_row0", "one_row_band_at_sub2_row63", "one_row_band_at_sub2_row0", "band_end_knots_on_grid_points",
            "task_without_rows", "sub_chunk_with_256_empty_tasks", "reduce_lower_cut_binds", "reduce_upper_cut_binds",
            "all_points_below_the_knots", "all_points_above_the_knots", "knot_on_a_cut_row", "shard", "whole_grid"}
    assert need <= seen, sorted(need - seen)
    assert sum(AC.many_bands(CH, off, n) for off, n, k, _, _ in CASES if k == "straddle") == 2
    assert {(off, n) for off, n, _, _, _ in CASES} == {(0, n) for n in AC.lengths(CH)} | set(AC.shards(CH))


# ------------------------------------------------------------------------------------------------ oracle consistency
@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_oracles_agree(case):
    """On every case, in fp64: the moment form against the direct form within 1e-12 of the band maximum; <g, dL> = <G, d>
    between sensor_vjp_cases.adjoint and sensor_jvp_cases.tangent within 1e-12 of the sum of the absolute terms; the dead
    bands are exactly the declared ones. MEASURED on the CPU: at most 3.1e-15 and 2.0e-16 over the set."""
    off, n, knots, nE, many = case
    c = AC.case(CH, off, n, knots)
    live = ~c["dead"]
    assert np.array_equal(c["N"] == 0.0, c["dead"]) and np.all(c["N"][live] > 0.0)
    L = FC.moment_form(c["N"], c["C"], c["M"], c["E"])
    assert np.array_equal(np.isnan(L), np.isnan(c["want"]))
    assert np.array_equal(np.isnan(c["want"][0, :, 0]), c["dead"])
    e = float(np.max((np.abs(L - c["want"]) / FC.band_max(c["want"]))[:, live]))
    assert np.all(c["Ma"] >= np.abs(c["M"]) * (1.0 - 1e-12)) and not c["Ma"][:, c["dead"]].any()
    g, o = AC.case_adjoint(CH, off, n, knots, nE, many)
    d, dL, scale = AC.case_tangent(CH, off, n, knots, nE, many)
    assert np.isnan(dL[:, c["dead"]]).all() and np.isfinite(dL[:, live]).all()
    gl = g[:, live].astype(np.float64)
    pairs = ((o["G_tau"], d["d_tau"]), (o["G_La"], d["d_La"]), (o["G_Ld"], d["d_Ld"]), (o["dTs"], d["d_Ts"]), (o["dE"], d["d_E"]))
    lhs = np.sum(gl * dL[:, live])
    rhs = sum(np.sum(G * np.asarray(v).astype(np.float64)) for G, v in pairs)
    terms = np.sum(np.abs(gl * dL[:, live])) + sum(np.sum(np.abs(G * np.asarray(v).astype(np.float64))) for G, v in pairs)
    print("srf axis oracles off=%d n=%d %s: moment vs direct %.3g of the band maximum, adjoint identity %.3g of the terms"
          % (off, n, knots, e, abs(lhs - rhs) / terms))
    assert e <= 1e-12
    assert abs(lhs - rhs) <= 1e-12 * terms


def test_moments_scale_leaves_the_adjoint_oracle_as_it_was():
    """srf_fused_cases.moments_scale is the loop sensor_vjp_cases.adjoint used to carry inline: the same bits, and with them
    the same scale of dE."""
    cases = [FC.case(CH, 1024, "coarse"), FC.case(CH, 1024, "dense"), AC.case(CH, 64, CH + 1, "on_cuts"), AC.case(CH, 0, 129, "cluster")]
    for c in cases:
        X, tables, Xk = c["X"], c["tables"], c["Xk"]
        Ts = np.array(FC.TS_LIST)
        tau, Ld = c["tau"].astype(np.float64), c["Ld"].astype(np.float64)
        w, N = VC.weights(X, tables)
        live = N > 0.0
        j0, j1, f = FC.knot_intervals(X, Xk)
        B = ref.planckian(X, Ts)
        Ma = np.zeros((3, len(tables), Xk.size))
        for t in range(3):  # the former inline loop, to the letter
            a = w * np.abs(tau) * (B[:, t] + np.abs(Ld))
            for b in np.flatnonzero(live):
                np.add.at(Ma[t, b], j0, a[b] * (1.0 - f))
                np.add.at(Ma[t, b], j1, a[b] * f)
        assert np.array_equal(FC.moments_scale(X, tables, c["tau"], c["Ld"], Xk, Ts), Ma)
        g = VC.cotangent(3, len(tables), 3, c["dead"])
        o = VC.adjoint(X, tables, c["tau"], c["La"], c["Ld"], Xk, c["E"][:, :3], Ts, g)
        gz = np.where(live[None, :, None], g.astype(np.float64), 0.0)
        invN = np.where(live, 1.0 / np.where(live, N, 1.0), 0.0)
        assert np.array_equal(o["scale"]["dE"], np.einsum("tbe,tbj,b->je", np.abs(gz), Ma, invN))


# ------------------------------------------------------------------------------------------------------------ teeth
def parts(c):
    """The oracle taken apart: W [nB][nX] the weights, G [nT][nX] = tau (B - Ld), Cc [nX] = tau Ld + La, Hat [nX][nk]."""
    X, Xk = c["X"], c["Xk"]
    tau, La, Ld = (c[k].astype(np.float64) for k in ("tau", "La", "Ld"))
    W, _ = VC.weights(X, c["tables"])
    G = (tau * (ref.planckian(X, np.array(FC.TS_LIST)).T - Ld))
    j0, j1, f = FC.knot_intervals(X, Xk)
    Hat = np.zeros((X.size, Xk.size))
    np.add.at(Hat, (np.arange(X.size), j0), 1.0 - f)
    np.add.at(Hat, (np.arange(X.size), j1), f)
    return W, G, tau * Ld + La, Hat


def put_together(W, G, Cc, Hat):
    """(N, C, M) from the parts; Hat may be one matrix or one per band."""
    per_band = Hat.ndim == 3
    M = np.stack([np.stack([(W[b] * G[t]) @ (Hat[b] if per_band else Hat) for b in range(W.shape[0])]) for t in range(G.shape[0])])
    return W.sum(axis=1), W @ Cc, M


def moved(c, N, Cb, M):
    """How far (N, C, M) lie from the case's own, in units of the GPU test's bound of each quantity: the largest over N and
    C (1e-6 relative), M element by element (K_DE 2^-24 of its scale) and L (1e-5 of the band maximum); a live band that
    comes out dead, or a value moved where the scale is 0, counts as infinitely far."""
    live = ~c["dead"]
    if np.any(N[live] <= 0.0):
        return np.inf
    out = [np.max(np.abs(N[live] / c["N"][live] - 1.0)) / REL_NC, np.max(np.abs(Cb[live] / c["C"][live] - 1.0)) / REL_NC]
    dM, Ma = np.abs(M - c["M"])[:, live], c["Ma"][:, live]
    if np.any(dM[Ma == 0.0] > 0.0):
        return np.inf
    out.append(np.max(dM[Ma > 0.0] / (K_DE * EPS * Ma[Ma > 0.0])))
    L = FC.moment_form(N, Cb, M, c["E"])
    out.append(np.max((np.abs(L - c["want"]) / FC.band_max(c["want"]))[:, live]) / TOL_L)
    return float(max(out))


def wrong_shard_cells(c, W, G, Cc, Hat):
    """(a) the parent grid's cells at a shard's ends instead of half cells"""
    if not c["off"]:
        return None
    X = c["X"]
    W = W * (np.full(X.size, AC.STEP) / cells(X))
    return W, G, Cc, Hat


def wrong_open_support(c, W, G, Cc, Hat):
    """(b) a band's support open at an end knot that is a grid point"""
    W = W.copy()
    for b, (xk, _) in enumerate(c["tables"]):
        W[b, (c["X"] == xk[0]) | (c["X"] == xk[-1])] = 0.0
    return W, G, Cc, Hat


def wrong_ragged_sub(c, W, G, Cc, Hat):
    """(c) the ragged last sub-chunk dropped"""
    n = c["X"].size
    if n % SUB == 0:
        return None
    W = W.copy()
    W[:, SUB * (n // SUB):] = 0.0
    return W, G, Cc, Hat


def wrong_chunk_first_row(c, W, G, Cc, Hat):
    """(d) the first row of every chunk after the first dropped"""
    if c["X"].size <= CH:
        return None
    W = W.copy()
    W[:, CH::CH] = 0.0
    return W, G, Cc, Hat


def wrong_low_end_not_held(c, W, G, Cc, Hat):
    """(e) rows below the first emissivity knot dropped from M (end value not held)"""
    Hat = Hat.copy()
    Hat[c["X"] < c["Xk"][0]] = 0.0
    return W, G, Cc, Hat


def wrong_reduce_upper_end(c, W, G, Cc, Hat):
    """(f) a knot's sum taken from one sub-chunk too few at the upper end"""
    n = c["X"].size
    sub = np.arange(n) // SUB
    per = np.empty((W.shape[0],) + Hat.shape)
    for b in range(W.shape[0]):
        touch = (W[b] != 0.0)[:, None] & (Hat != 0.0)
        last = np.where(touch, sub[:, None], -1).max(axis=0)  # the last sub-chunk that holds a term of knot j
        per[b] = np.where(sub[:, None] == last[None, :], 0.0, Hat)
    return W, G, Cc, per


WRONG = (wrong_shard_cells, wrong_open_support, wrong_ragged_sub, wrong_chunk_first_row, wrong_low_end_not_held, wrong_reduce_upper_end)


def test_the_parts_are_the_oracle():
    """parts() and put_together() restate srf_fused_cases.moments: the teeth below bite the oracle, not something else."""
    for off, n, knots, _, _ in CASES[::7]:
        c = AC.case(CH, off, n, knots)
        assert moved(c, *put_together(*parts(c))) <= 1e-6  # of the GPU bounds: 3e-11 relative for N and C, 2e-12 of M's scale


@pytest.mark.parametrize("wrong", WRONG, ids=[w.__name__ for w in WRONG])
def test_teeth(wrong):
    """Each deliberate error, applied to the oracle, moves a quantity the GPU test asserts (N, C, M element by element, L)
    by more than 4 times that quantity's GPU bound in at least one case: a kernel wrong in that way fails the GPU test.
    MEASURED on the CPU, cases that catch the error of the 152 / the largest finite margin: (a) 48 / 1e6, (b) 126, (c) 119,
    (d) 36 (b, c, d: a live band comes out dead), (e) 40 / 4.5e5, (f) 143 / 4.5e5."""
    best, hits = 0.0, 0
    for off, n, knots, _, _ in CASES:
        if hits >= 3 and knots == "cluster":
            continue  # the dense hat matrices of the cluster cases: not needed once the error is caught
        c = AC.case(CH, off, n, knots)
        w = wrong(c, *parts(c))
        if w is None:
            continue
        m = moved(c, *put_together(*w))
        if m > MARGIN:
            hits += 1
        best = max(best, m if np.isfinite(m) else 1e300)
    print("teeth %s: caught by %d cases, largest margin %.3g" % (wrong.__name__, hits, best))
    assert hits >= 1, wrong.__doc__
