"""CPU side of tests/test_gpu_sdvoigt_paths.py: the cases of tests/sdvoigt_cases.py reach the paths of sdvoigt_tile_kernel
they name (cpu_ref.sd_census restates sd_zones, the tile / row classification, the chunk lists and the branch of
sdvoigt_profile each point-by-point point takes), and the reference the GPU test uses is sound: the long-double and the
float64 run of the oracle agree to the metric, drop at most 2 points per line and 1e-3 of a case's points where their
branch predicates differ, and stay within 1e6 (line, point) pairs per case. The float64 path of the dtype switch is the
oracle as it was, bit for bit."""
import os
import re
from collections import Counter

import numpy as np
import pytest

from oracle import cpu_ref as ref

import sdvoigt_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _census(case):
    C = Counter()
    for T, p in zip(case["T"], case["p"]):
        C.update(ref.sd_census(case["tbl"], case["grid"], T, p, case["ow"], case["hw"], case["thresh"]))
    return C


def test_census_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "radtxfr_amd", "csrc", "rtx_sdvoigt.hip")).read()
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, src).group(1))
    assert (define("SD_TILE"), define("SD_ROWS"), define("SD_TDIST"), define("SD_NEAR"), define("SD_CHUNK")) == \
        (ref.SD_TILE, ref.SD_ROWS, ref.SD_TDIST, ref.SD_NEAR, ref.SD_CHUNK)
    for text in ("const double m = 2.0 * step;", "dP2 > 0.0 && sY >= 8.0", "r < rc - SD_NEAR || r > rc + SD_NEAR",
                 "lo <= ia && hi >= ib && (left || right)", "lo <= pa && hi > pb"):
        assert text in src, text


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_case_reaches_its_paths(name):
    case = SC.CASES[name]
    C = _census(case)
    missing = [e for e in case["expect"] if not e.startswith("!") and C[e] <= 0]
    present = [e[1:] for e in case["expect"] if e.startswith("!") and C[e[1:]] > 0]
    assert not missing and not present, (name, missing, present)
    assert case["grid"][4] <= 4 * ref.SD_TILE + 1


def test_every_branch_and_class_is_reached_by_some_case():
    """Every label of the census that names a class, a row kind or a branch of sdvoigt_profile is in some case's expect."""
    named = {e for c in SC.CASES.values() for e in c["expect"] if not e.startswith("!")}
    want = {"cand_empty_window", "cand_dropped", "tile_a", "tile_b", "row_list", "row_nodal_a", "row_nodal_b", "row_near", "row_edge",
            "row_switch", "row_nozones", "p1_w24", "p1_asym", "p2_real", "p2_cplx", "p3_near", "p3_far", "p4_far", "p4_cpf3",
            "p4_real_in_in", "p4_real_in_out", "p4_cplx", "second_chunk", "chunk_mixed", "chunk_no_tile_after_tile", "nT_1",
            "nT_8", "nT_9", "ragged_tile", "ragged_row", "tile_level_at_256", "row_list_at_255", "rc_outside_-2", "rc_outside_-1",
            "rc_outside_16", "rc_outside_17", "centre_row_0", "centre_row_8", "centre_row_15", "zone_b_all_far",
            "tile_switch_gap_2_rows", "tile_switch_gap_3_tile", "switch_gap_pointwise_2", "switch_gap_nodal_3"}
    assert want <= named, sorted(want - named)
    hi = ref.sdvoigt_terms(SC.CASES["pf_cpf3"]["tbl"], T=296.0, p=1.0, OmegaGrid=SC.axis(SC.CASES["pf_cpf3"]["grid"]),
                           OmegaWing=SC.CASES["pf_cpf3"]["ow"], OmegaWingHW=0.0)
    per_line = [int(np.sum((code & ref.SD_CPF3) != 0)) for _, _, _, code in hi["lines"]]
    assert len(per_line) == 3 and min(per_line) >= 8, per_line  # >= 8 points of every line in the cpf3 shell


def test_metric_fails_on_non_finite_output():
    """A NaN or an inf inside a window (an unwritten point: the GPU test prefills its outputs with NaN) is an infinite error."""
    o = SC.oracle("pf_p3_far")
    for bad in (np.nan, np.inf):
        got = o["want64"][0].copy()
        got[100] = bad
        e_den, e_allow, _, _ = SC.judge(got, o, 0)
        assert not (e_allow <= 1.0) and e_den == np.inf


def test_nodes_lie_inside_their_row_and_tile():
    """sd_zones' two-point margin is not what keeps a node level off a regime switch: the outermost Chebyshev node lies
    0.27 points inside a row (12 nodes on 64 points) and 0.62 inside a tile (32 on 1024), so a row or tile that starts on
    a switch is evaluated on one side of it. Holds for the kernel's SD_RN / SD_TN."""
    src = open(os.path.join(ROOT, "radtxfr_amd", "csrc", "rtx_sdvoigt.hip")).read()
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, src).group(1))
    inset = lambda N, L: (L - 1) / 2.0 * (1.0 - np.cos(np.pi / (2.0 * N)))
    assert 0.25 <= inset(define("SD_RN"), 64) <= 0.3 and 0.6 <= inset(define("SD_TN"), define("SD_TILE")) <= 0.65


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_reference_is_sound(name):
    """The oracle of the GPU test, from the reference alone: pair count, excluded-point caps, and the float64 run against
    the long-double one under the metric itself (own finite, ratio <= 1/4 by construction of own, zeros the same)."""
    case = SC.CASES[name]
    for g in (case["grid"],) + tuple(case["grid"][:3] + s for s in case["shards"]):
        o = SC.oracle(name, g)
        n_pts = sum(w.size for w in o["want"])
        assert sum(o["pairs"]) <= 1000000, (name, sum(o["pairs"]))
        assert max(o["skip_per_line"]) <= 2, (name, o["skip_per_line"])
        assert sum(int(s.sum()) for s in o["skip"]) <= 1e-3 * n_pts, name
        if "switch_on_point" not in name:
            assert not any(s.any() for s in o["skip"]), name
        for k in range(len(o["want"])):
            assert o["want"][k].dtype == np.longdouble and np.isfinite(o["own"][k].astype(np.float64)).all()
            assert np.array_equal(o["den"][k] == 0, o["want64"][k] == 0)
            e_den, e_allow, _, zeros = SC.judge(o["want64"][k], o, k)
            assert zeros and e_allow <= 1.0 / SC.OWN_FACTOR + 1e-12, (name, k, e_den, e_allow)
    if name in SC.SIGN_CHANGE:
        w = np.concatenate(SC.oracle(name)["want"])
        assert w.min() < 0 < w.max()


# ---- cpu_ref's hum1_wei, cpf3 and PROFILE_SDVOIGT as they were before the dtype switch, kept here word for word so that
# the float64 path of the switch is held to them bit for bit ---------------------------------------------------------------
def _before_hum1_wei(x, y):
    """misc/hapi.py:9833-9844: Weideman-24 where |x|+y<15, else the 1-term asymptote."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64) + np.zeros_like(x)
    t = y - 1.0j * x
    cerf = 1 / np.sqrt(np.pi) * t / (0.5 + t ** 2)
    mask = abs(x) + y < 15.0
    if np.any(mask):
        z = x[mask] + 1.0j * y[mask]
        Z = (ref._L24 + 1.0j * z) / (ref._L24 - 1.0j * z)
        p = np.polyval(ref._W24, Z)
        w = 2 * p / (ref._L24 - 1.0j * z) ** 2 + (1 / np.sqrt(np.pi)) / (ref._L24 - 1.0j * z)
        np.place(cerf, mask, w)
    return cerf.real, cerf.imag


def _before_cpf3(X, Y):
    """misc/hapi.py:9645-9670: 15-term asymptotic series of w(z), z = X + iY."""
    zm1 = 1.0 / (np.asarray(X, dtype=np.float64) + 1.0j * np.asarray(Y, dtype=np.float64))
    zm2 = zm1 ** 2
    zsum = np.ones_like(zm1)
    zterm = np.ones_like(zm1)
    for t in ref._CPF3_TT:
        zterm = zterm * zm2 * t
        zsum = zsum + zterm
    zsum = zsum * 1.0j * zm1 * 0.564189583547756
    return zsum.real, zsum.imag


def _before_profile_sdvoigt(sg0, GamD, Gam0, Gam2, Shift0, Shift2, sg):
    """misc/hapi.py:10117-10129 -> pcqsdhc (:9850-10024) with anuVC = eta = 0, for which the common part (:10022) is
    LS = Aterm/pi. Real part only (what absorptionCoefficient_SDVoigt uses, :10897). CPF = hum1_wei (:9846)."""
    sg = np.asarray(sg, dtype=np.float64)
    cte = np.sqrt(np.log(2.0)) / GamD
    rpi = np.sqrt(np.pi)
    c0 = complex(Gam0, Shift0)
    c2 = complex(Gam2, Shift2)
    c0t = c0 - 1.5 * c2
    c2t = c2
    cw = lambda x, y: (lambda r: r[0] + 1.0j * r[1])(_before_hum1_wei(x, y))
    if abs(c2t) == 0.0:  # PART1 (:9908-9915)
        Z1 = (1.0j * (sg0 - sg) + c0t) * cte
        A = rpi * cte * cw(-Z1.imag, Z1.real)
        return (A / np.pi).real
    X = (1.0j * (sg0 - sg) + c0t) / c2t
    Y = 1.0 / ((2.0 * cte * c2t)) ** 2
    csqrtY = (Gam2 - 1.0j * Shift2) / (2.0 * cte * (Gam2 ** 2 + Shift2 ** 2))
    p2 = np.abs(X) <= 3.0e-8 * abs(Y)
    p3 = (abs(Y) <= 1.0e-15 * np.abs(X)) & ~p2
    p4 = ~(p2 | p3)
    A = np.zeros(sg.size, dtype=np.complex128)
    if np.any(p4):  # PART4 (:9933-9971)
        Z1 = np.sqrt(X[p4] + Y) - csqrtY
        Z2 = Z1 + 2.0 * csqrtY
        x1, y1, x2, y2 = -Z1.imag, Z1.real, -Z2.imag, Z2.real
        S1, S2 = np.sqrt(x1 ** 2 + y1 ** 2), np.sqrt(x2 ** 2 + y2 ** 2)
        use3 = (np.abs(S1 - S2) <= 1.0) & (np.maximum(S1, S2) > 8.0) & (np.minimum(S1, S2) <= 8.0)
        W1 = np.zeros(Z1.size, dtype=np.complex128)
        W2 = np.zeros(Z1.size, dtype=np.complex128)
        if np.any(use3):
            r1, r2 = _before_cpf3(x1[use3], y1[use3]), _before_cpf3(x2[use3], y2[use3])
            W1[use3], W2[use3] = r1[0] + 1.0j * r1[1], r2[0] + 1.0j * r2[1]
        if np.any(~use3):
            W1[~use3], W2[~use3] = cw(x1[~use3], y1[~use3]), cw(x2[~use3], y2[~use3])
        A[p4] = rpi * cte * (W1 - W2)
    if np.any(p2):  # PART2 (:9974-9989)
        Z1 = (1.0j * (sg0 - sg[p2]) + c0t) * cte
        Z2 = np.sqrt(X[p2] + Y) + csqrtY
        A[p2] = rpi * cte * (cw(-Z1.imag, Z1.real) - cw(-Z2.imag, Z2.real))
    if np.any(p3):  # PART3 (:9992-10017; the reference indexes the full X at :10003, which only works when every point is PART3)
        Xt = X[p3]
        sq = np.sqrt(Xt)
        near = np.abs(sq) <= 4.0e3
        At = np.zeros(Xt.size, dtype=np.complex128)
        if np.any(near):
            At[near] = (2.0 * rpi / c2t) * (1.0 / rpi - sq[near] * cw(-sq[near].imag, sq[near].real))
        if np.any(~near):
            At[~near] = (1.0 / c2t) * (1.0 / Xt[~near] - 1.5 / (Xt[~near] ** 2))
        A[p3] = At
    return (A / np.pi).real


def test_float64_switch_is_the_oracle_unchanged(golden):
    """PROFILE_SDVOIGT, hum1_wei and cpf3 with dtype=float64 (and by default) against the functions as they were before the
    switch (above), array_equal, on the golden G11 lines at three states and on parameter sets that reach PART1, PART2,
    both PART3 forms, the cpf3 shell and Gamma0 < 1.5 Gamma2; sdvoigt_terms(float64) against
    absorptionCoefficient_SDVoigt, array_equal; the long-double path returns long double."""
    from radtxfr_amd import synthetic
    g = golden("g11_sdvoigt.npz")
    tbl = dict(synthetic.synth_line_table(int(g["seed"]), int(g["n_lines"]), float(g["nu_lo"]), float(g["nu_hi"])))
    tbl["SD_air"], tbl["SD_self"] = g["SD_air"], g["SD_self"]
    grid = np.linspace(float(g["g_lo"]), float(g["g_hi"]), int(g["g_n"]))
    seen = 0
    sets = []
    for T, p in ((250.0, 0.3), (220.0, 0.01), (296.0, 1.0)):
        _, xs = ref.absorptionCoefficient_SDVoigt(tbl, T=T, p=p, OmegaGrid=grid)
        t = ref.sdvoigt_terms(tbl, T=T, p=p, OmegaGrid=grid)
        assert np.array_equal(t["xs"], xs) and t["xs"].dtype == np.float64
        P = ref.line_params(tbl, T, p)
        for r in range(0, int(g["n_lines"]), 3):
            sets.append((tbl["nu"][r], P["GammaD"][r], P["Gamma0"][r], ref._gamma2(tbl, r, p), P["Shift0"][r], 0.0, grid[r % 7::7]))
    far = np.linspace(7750.0, 7950.0, 801)
    sets += [(1000.0, 1.45e-3, 0.07, 0.0, 1e-3, 0.0, grid), (1000.0, 1.45e-3, 7e-4, 7e-13, 0.0, 0.0, np.linspace(999.9, 1000.1, 2001)),
             (1000.0, 1.45e-3, 7e-4, 4.9e-13, -2e-4, 0.0, np.linspace(999.9, 1000.1, 2001)),
             (0.07, 1.016e-7, 0.7, 0.07, 0.0, 0.0, np.linspace(50.0, 56.0, 601)), (0.07, 1.016e-7, 4.76e-3, 4.76e-4, 0.0, 0.0, far),
             (1000.0, 1.45e-3, 0.07, 0.007, 0.0, 0.0, np.linspace(999.0, 1001.0, 2001)),
             (1000.0, 1.45e-3, 0.07, 0.07, 0.0, 0.0, np.linspace(999.0, 1001.0, 2001)),
             (1000.0, 1.45e-3, 7e-8, 7e-8, 0.0, 0.0, np.linspace(1000.0 - 1e-6, 1000.0 + 1e-6, 201)),
             (1000.0, 1.45e-3, 0.05, 0.004, 0.002, 1e-3, np.linspace(999.0, 1001.0, 501))]
    for args in sets:
        old = _before_profile_sdvoigt(*args)
        new, code = ref.PROFILE_SDVOIGT(*args, dtype=np.float64, branches=True)
        assert old.dtype == np.float64 and np.array_equal(old, new) and np.array_equal(old, ref.PROFILE_SDVOIGT(*args))
        assert ref.PROFILE_SDVOIGT(*args, dtype=np.longdouble).dtype == np.longdouble
        seen |= int(np.bitwise_or.reduce(code))
    assert seen & ref.SD_P1 and seen & ref.SD_P2 and seen & ref.SD_P3 and seen & ref.SD_P4 and seen & ref.SD_CPF3
    assert seen & ref.SD_P3NEAR and seen & ref.SD_NEG1 and seen & ref.SD_W24_1
    assert any(not ((c & ref.SD_P3NEAR) != 0)[(c & ref.SD_P3) != 0].all() for c in
               (ref.PROFILE_SDVOIGT(*sets[-5], branches=True)[1],))  # the far form of PART3
    x = np.arange(-320, 321) / 16.0  # binary fractions: |x| + y < 15 is the same predicate in both precisions
    for y in (0.0, 0.25, 5.0, 16.0):
        w, wo, wl = ref.hum1_wei(x, y), _before_hum1_wei(x, y), ref.hum1_wei(x, y, dtype=np.longdouble)
        assert np.array_equal(w[0], wo[0]) and np.array_equal(w[1], wo[1]) and wl[0].dtype == np.longdouble
        assert np.max(np.abs(w[0] - wl[0].astype(np.float64))) <= 2e-15
    xc = np.linspace(6.0, 9.0, 31)
    c, co, cl = ref.cpf3(xc, 2.0), _before_cpf3(xc, 2.0), ref.cpf3(xc, 2.0, dtype=np.longdouble)
    assert np.array_equal(c[0], co[0]) and np.array_equal(c[1], co[1])
    assert np.max(np.abs(c[0] - cl[0].astype(np.float64))) <= 1e-16
    with pytest.raises(ValueError):
        ref.hum1_wei(x, 1.0, dtype=np.float32)
