"""Every instantiation and every exit of the per-pixel cube's derivative kernels (radtxfr_amd/csrc/rtx_srf_cube_vjp.hip,
rtx_srf_cube_jvp.hip, rtx_srf_cube_fit.hip): the adjoint, the tangent, the normal equations and the fit at every node count
Q = 1 .. 8 with the table slice in LDS and in global memory, the two fit kernels at every (Q, nMix), band counts on both
sides of one and two blocks of 64, every way the fit can end, and the adjoint's reduction with its chunk doubled.

The cases are those of tests/srf_cube_path_cases.py (tests/test_srf_cube_paths_host.py shows on the CPU that each does what its
name says); the oracles, the helpers and the rounding counts are those of tests/test_gpu_srf_cube_vjp.py, _jvp.py and _fit.py:
|got - want| <= k 2^-24 scale element by element on the device's own float32 N, C and table, or bit identity, or the fit's
sensitivity bound. Nothing here has a bound of its own. Scenes are 65 pixels (one full wave of the fit and one pixel more; one
ragged round of the pixel kernels), pixels 0 and 1 on the ends of the range, T_range = (285, 315) for every Q.

MEASURED figures are in the docstrings and, with the run times, in profiles/srf_cube_paths.txt."""
import numpy as np
import pytest

import srf_cube_cases as CC
import srf_cube_fit_cases as FT
import srf_cube_jvp_cases as JC  # noqa: F401  (the tangent's oracle, reached through test_gpu_srf_cube_jvp.check_raw)
import srf_cube_path_cases as PC
import srf_cube_vjp_cases as VC
import test_gpu_srf_cube_fit as GF
import test_gpu_srf_cube_jvp as GJ
import test_gpu_srf_cube_vjp as GV
from test_gpu_sensor_vjp import within
from test_gpu_srf_cube_fit import env  # noqa: F401

pytestmark = pytest.mark.gpu

GROUPS = GJ.GROUPS


def tabs(env, Q, nEnd, nB=20):
    """The device tables of (Q, nEnd) on T_RANGE, with nB bands: the keys of all three sibling modules' helpers."""
    return GF.device_tables(env, PC.KNOTS, nEnd, (PC.T_RANGE, Q), nB=nB)


def mixed_scene(nEnd, nPix=PC.NPIX):
    """The siblings' scene of the table-size tests, mixtures of 3 out of all nEnd, with the table's first and last column in it."""
    sc = CC.scene(nPix, 3, nEnd, PC.T_RANGE, seed=11)
    sc["kidx"][2, 0], sc["kidx"][3, 1] = nEnd - 1, 0
    return sc


def distinct_scene(nMix, nEnd, seed=5):
    """FT.distinct_scene, with the table's last column in pixel 2 (its row stays without a repeat)."""
    sc = FT.distinct_scene(PC.NPIX, nMix, nEnd, PC.T_RANGE, seed=seed)
    if nEnd - 1 not in sc["kidx"][2]:
        sc["kidx"][2, 0] = nEnd - 1
    return sc


# ------------------------------------------------------------------------------ 1. node counts and table placements
@pytest.mark.parametrize("Q", PC.Q_LIST)
def test_adjoint_at_every_node_count(env, Q):
    """rtx_srf_pixel_cube_vjp at nEnd = 5, 128 // Q (the largest table in LDS) and 128 // Q + 1 (the smallest in global memory),
    mixtures of 3: dT, dfrac and gL against the oracle. One node: dT is 0.0 exactly.
    MEASURED on an MI355X, worst of the 24 tables, in units of 2^-24 scale: dT 0.29 (k = 3 .. 10), dfrac 0.94, gL 1.73 (k = 3; Q = 2,
    64 endmembers); by node count in profiles/srf_cube_paths.txt."""
    for nEnd in PC.nend_list(Q):
        t = tabs(env, Q, nEnd)
        sc = mixed_scene(nEnd)
        assert sc["kidx"].max() == nEnd - 1 and sc["kidx"].min() == 0
        g = VC.cotangent(20, PC.NPIX, t["dead"], seed=12)
        got, _ = GV.check_raw(env, t, sc, PC.T_RANGE, g, "paths vjp Q=%d nEnd=%d" % (Q, nEnd))
        if Q == 1:
            assert np.all(got["dT"] == 0.0) and np.any(got["dfrac"] != 0.0)


@pytest.mark.parametrize("Q", PC.Q_LIST)
def test_tangent_at_every_node_count(env, Q):
    """rtx_srf_pixel_cube_jvp at the same tables, two vectors: each group moving alone and all three together against the
    oracle; at nEnd = 128 // Q also the second vector alone (the NV = 1 instantiation), which has the bits it has beside the
    first. One node: a d_Tpix-only tangent is 0.0 exactly on the live bands.
    MEASURED on an MI355X, worst of the 24 tables, in units of 2^-24 scale: dL 3.16 (k = 11), d_frac 3.09 (k = 10), d_Tpix 1.15 (k = 6),
    all together 2.16 (k = 5, the largest share of a count: 0.43)."""
    for nEnd in PC.nend_list(Q):
        t = tabs(env, Q, nEnd)
        sc = mixed_scene(nEnd)
        d = GJ.directions(t, sc, 2, seed=12)
        got = GJ.check_raw(env, t, sc, PC.T_RANGE, d, "paths jvp Q=%d nEnd=%d" % (Q, nEnd), dead=t["dead"])
        if nEnd == PC.TAB_LDS // Q:
            alone = GJ.raw(env, t, sc, **{k: np.ascontiguousarray(d[k][1:2]) for k in GROUPS})
            assert alone.shape[0] == 1 and np.array_equal(alone[0], got[1], equal_nan=True)
        if Q == 1:
            only = GJ.raw(env, t, sc, d_Tpix=d["d_Tpix"])
            assert np.all(only[:, ~t["dead"]] == 0.0) and np.isnan(only[:, t["dead"]]).all()


@pytest.mark.parametrize("nEnd", PC.JVP_TILE_NEND)
def test_tangent_relayout_tile_edge(env, nEnd):
    """dL's nEnd + 1 columns fill one 64-column tile of the re-layout kernel exactly (63 endmembers) and spill one column into
    a second (64).
    MEASURED on an MI355X: at most 2.13 (dL, k = 5)."""
    t = tabs(env, 2, nEnd)
    sc = mixed_scene(nEnd)
    assert sc["kidx"].max() == nEnd - 1
    GJ.check_raw(env, t, sc, PC.T_RANGE, GJ.directions(t, sc, 2, seed=12), "paths jvp relayout nEnd=%d" % nEnd, dead=t["dead"])


# ------------------------------------------------------------------------------ 2. every (Q, nMix) of the fit kernels
def check_normal_any(env, t, st, meas, what, w=None):
    """GF.check_normal for Q >= 2. One node has l' = 0: cost, grad and hess against the oracle under the same counts, the
    T row of hess 0.0 exactly and, H_00 being no pivot, every entry of the step NaN."""
    if t["Q"] >= 2:
        return GF.check_normal(env, t, st, meas, what, w=w)
    nMix = st["kidx"].shape[1]
    lam = np.random.default_rng(31).uniform(0.0, 0.5, st["T"].size)
    got = GF.normal(env, t, st, meas, w=w, lam=lam)
    o = FT.evaluate(t["N_h"], t["C_h"], t["G_h"], t["nodes"], st["kidx"], st["frac"], st["T"], meas, w)
    within(got["cost"], o["cost"], o["scale"]["cost"], GF.K_COST(1, nMix), what + " cost")
    within(got["grad"], o["grad"], o["scale"]["grad"], GF.K_GRAD(1, nMix), what + " grad")
    within(got["hess"], o["hess"], o["scale"]["hess"], GF.K_H(1), what + " hess")
    T_row = [FT.tri(i, 0) for i in range(nMix + 1)]
    assert np.all(got["hess"][:, T_row] == 0.0) and np.all(got["grad"][:, 0] == 0.0) and np.all(got["hess"][:, FT.tri(1, 1)] > 0.0)
    assert np.isnan(got["step"]).all()
    return got


def fit_case(env, t, sc, what, w=None, k=3, scan=True):
    """One table and scene through both fit kernels: normal at a start away from the truth against the oracle; the fit from
    that start, k trials, against the host loop bit for bit; the scan alone. Returns what was computed, for bit comparisons."""
    meas = GF.forward(env, t, sc)
    st = GF.away(sc, PC.T_RANGE)
    out = dict(normal=check_normal_any(env, t, st, meas, what, w=w))
    start = (st["T"], st["frac"])
    out["fit"] = GF.fit(env, t, sc["kidx"], meas, w=w, start=start, max_iter=k)
    want, _, _ = GF.host_loop(env, t, sc["kidx"], meas, start, k, 1e-3, 0.0, w=w)
    GF.same(out["fit"], want)
    if t["Q"] == 1:
        assert np.all(out["fit"]["status"] == 3) and np.all(out["fit"]["n_iter"] == 0) and np.isnan(out["fit"]["T"]).all()
    else:
        assert np.all(out["fit"]["status"] <= 1) and out["fit"]["n_iter"].max() == k
    if scan:  # on a noisy cube: with one node the clean one is met exactly by some pixels (cost 0.0 is status 0, not 1)
        out["scan"] = s = GF.fit(env, t, sc["kidx"], PC.noisy(meas), w=w, max_iter=0)
        assert np.all(s["status"] == 1) and np.all(s["n_iter"] == 0) and np.all(np.isin(s["T"], t["nodes"]))
        assert np.all(np.isfinite(s["frac"])) and np.all(s["cost"] > 0.0) and np.all(np.isfinite(s["hess"]))
    return out


@pytest.mark.parametrize("Q,nMix", PC.QMIX)
def test_fit_kernels_at_every_node_count_and_mixture(env, Q, nMix):
    """scf_normal_kernel<Q, nMix> and scf_fit_kernel<Q, nMix> at nEnd = 5, 128 // Q and 128 // Q + 1 (5 Q runs through every
    residue mod 4 of the LDS stride): normal against the oracle, with the step's residual for Q >= 2 and the exact zeros and
    NaN of one node; the fit from a given start, 3 trials, against the host loop bit for bit; the scan alone ends with status 1
    on a node. The scene of nEnd = 128 // Q + 1 keeps to the first 128 // Q endmembers, and both placements give the same
    bits; a second scene there reaches the last column.
    MEASURED on an MI355X, worst of the 96 tables and the 32 further scenes, in units of 2^-24 scale: cost 0.063 (k = 11 .. 31), grad
    0.48 (k = 9 .. 26), hess 2.6 (k = 7 .. 21; at most 0.25 of its count); the step's residual at most 0.45 of the Cholesky
    residual bound."""
    small, edge, over = PC.nend_list(Q)
    res = {}
    for nEnd in (small, edge, over):
        t = tabs(env, Q, nEnd)
        sc = distinct_scene(nMix, min(nEnd, edge))
        assert PC.fit_stride(nEnd, Q) == (0 if nEnd == over else 4 * (((nEnd * Q + 3) // 4) | 1))
        res[nEnd] = fit_case(env, t, sc, "paths fit Q=%d nMix=%d nEnd=%d" % (Q, nMix, nEnd))
    assert np.array_equal(tabs(env, Q, over)["G_h"][:, :, :edge], tabs(env, Q, edge)["G_h"])
    for part in ("normal", "fit", "scan"):
        GF.same(res[edge][part], res[over][part])
    t = tabs(env, Q, over)
    sc = distinct_scene(nMix, over, seed=6)
    assert sc["kidx"].max() == over - 1 and all(len(set(row)) == nMix for row in sc["kidx"])
    check_normal_any(env, t, GF.away(sc, PC.T_RANGE), GF.forward(env, t, sc), "paths fit Q=%d nMix=%d nEnd=%d, every column" % (Q, nMix, over))


# ------------------------------------------------------------------------------ 3. band-block edges
BLOCK_FIT = (PC.BLOCK_TABLES[0] + (3,), PC.BLOCK_TABLES[1] + (4,), (PC.BLOCK_SCALAR[0], PC.BLOCK_TABLES[0][1], PC.BLOCK_SCALAR[1]))  # (Q, nEnd, nMix)


@pytest.mark.parametrize("nB", PC.NB_FIT)
@pytest.mark.parametrize("Q,nEnd,nMix", BLOCK_FIT)
def test_fit_band_blocks(env, Q, nEnd, nMix, nB):
    """1, 63, 64, 65, 128 and 129 bands (a block of 64 bands one short, exactly full, one over; two blocks and one band of a
    third), weights of which bands 63 and 64 are zero: normal against the oracle, the fit against the host loop. 8 nodes and 8
    endmembers (LDS, 16-byte row reads), 5 and 31 (global memory), 7 and 8 (LDS, the row read word by word).
    MEASURED on an MI355X, worst of the 18 cases, in units of 2^-24 scale: cost 0.14, grad 0.72, hess 4.5 (k = 15), all three at
    one band; the step's residual at most 0.24 of its bound."""
    t = tabs(env, Q, nEnd, nB=nB)
    assert t["N_h"].shape == (nB,) and np.array_equal(t["dead"], np.tile(t["case"]["dead"], 7)[:nB])
    sc = distinct_scene(nMix, nEnd)
    w = PC.block_weights(129)[:nB]
    fit_case(env, t, sc, "paths fit Q=%d nMix=%d nEnd=%d nB=%d" % (Q, nMix, nEnd, nB), w=w, scan=nB > 1)


@pytest.mark.parametrize("Q,nEnd,nMix", BLOCK_FIT)
def test_fit_band_subset(env, Q, nEnd, nMix):
    """Any subset of the bands, order kept: 129 bands with weight zero on bands 64 .. 128 give the bits of the first 64 bands
    alone, in normal, in the fit from a start and in the fit from the scan."""
    t129, t64 = tabs(env, Q, nEnd, nB=129), tabs(env, Q, nEnd, nB=64)
    assert np.array_equal(t129["G_h"][:, :64], t64["G_h"]) and np.array_equal(t129["N_h"][:64], t64["N_h"])
    sc = distinct_scene(nMix, nEnd)
    meas = GF.forward(env, t129, sc)
    m64 = np.ascontiguousarray(meas[:64])
    assert np.array_equal(m64, GF.forward(env, t64, sc), equal_nan=True)
    w = PC.block_weights(129)
    w[64:] = 0.0
    st = GF.away(sc, PC.T_RANGE)
    lam = np.random.default_rng(31).uniform(0.0, 0.5, PC.NPIX)
    GF.same(GF.normal(env, t129, st, meas, w=w, lam=lam), GF.normal(env, t64, st, m64, w=w[:64], lam=lam))
    start = (st["T"], st["frac"])
    GF.same(GF.fit(env, t129, sc["kidx"], meas, w=w, start=start, max_iter=6), GF.fit(env, t64, sc["kidx"], m64, w=w[:64], start=start, max_iter=6))
    a = GF.fit(env, t129, sc["kidx"], meas, w=w, max_iter=6)
    GF.same(a, GF.fit(env, t64, sc["kidx"], m64, w=w[:64], max_iter=6))
    assert np.all(a["status"] <= 1)


@pytest.mark.parametrize("Q,nEnd", PC.BLOCK_TABLES)
def test_adjoint_band_blocks(env, Q, nEnd):
    """63, 64, 65 and 129 bands against the oracle; gL's rows of the first 64 bands are the same bits in the 129-band run and
    in the 64-band run (dT and dfrac sum over the bands).
    MEASURED on an MI355X, worst of the 8 cases, in units of 2^-24 scale: dT 0.17, dfrac 0.37, gL 1.46 (k = 3)."""
    sc = mixed_scene(nEnd)
    g129 = VC.cotangent(129, PC.NPIX, tabs(env, Q, nEnd, nB=129)["dead"], seed=21)
    got = {}
    for nB in PC.NB_DERIV:
        t = tabs(env, Q, nEnd, nB=nB)
        got[nB], _ = GV.check_raw(env, t, sc, PC.T_RANGE, np.ascontiguousarray(g129[:nB]), "paths vjp Q=%d nEnd=%d nB=%d" % (Q, nEnd, nB))
    assert np.array_equal(got[129]["gL"][:, :64], got[64]["gL"]) and np.array_equal(got[65]["gL"][:, :63], got[63]["gL"])
    assert not np.array_equal(got[129]["dfrac"], got[64]["dfrac"])


@pytest.mark.parametrize("Q,nEnd", PC.BLOCK_TABLES)
def test_tangent_band_blocks(env, Q, nEnd):
    """63, 64, 65 and 129 bands against the oracle; the rows of the first 64 bands are the same bits in the 129-band run and in
    the 64-band run.
    MEASURED on an MI355X, worst of the 8 cases, in units of 2^-24 scale: dL 3.57, d_frac 2.66, all together 2.09 (k = 11), d_Tpix 0.87
    (k = 8)."""
    sc = mixed_scene(nEnd)
    d129 = GJ.directions(tabs(env, Q, nEnd, nB=129), sc, 2, seed=21)
    got = {}
    for nB in PC.NB_DERIV:
        t = tabs(env, Q, nEnd, nB=nB)
        d = dict(d129, dL=np.ascontiguousarray(d129["dL"][:, :, :nB]))
        got[nB] = GJ.check_raw(env, t, sc, PC.T_RANGE, d, "paths jvp Q=%d nEnd=%d nB=%d" % (Q, nEnd, nB), dead=t["dead"])
    assert np.array_equal(got[129][:, :64], got[64], equal_nan=True) and np.array_equal(got[65][:, :63], got[63], equal_nan=True)


# ------------------------------------------------------------------------------ 4. the exits of the fit
_EXIT = {}


def exit_case(env):
    """(device tables, the scene, the forward's cube at its truth, a start away from it) of the exit cases, made once."""
    if not _EXIT:
        t = tabs(env, PC.EXIT["Q"], PC.EXIT["nEnd"])
        sc = PC.exit_scene()
        _EXIT["v"] = (t, sc, GF.forward(env, t, sc), GF.away(sc, PC.T_RANGE))
    return _EXIT["v"]


def against_host_loop(env, t, kidx, meas, k=10, w=None, start=None, lambda0=1e-3, ftol=0.0):
    """The fit and the host loop of the same call, bit for bit -> (the fit's result, clamped trials, lanes stopped at the cap)."""
    got = GF.fit(env, t, kidx, meas, w=w, start=start, max_iter=k, lambda0=lambda0, ftol=ftol)
    want, clamped, capped = GF.host_loop(env, t, kidx, meas, start, k, lambda0, ftol, w=w)
    GF.same(got, want)
    return got, clamped, capped


def all_nan(r, sel):
    return all(np.isnan(r[k][sel]).all() for k in ("T", "frac", "cost", "hess"))


def test_exit_zero_weights(env):
    """wgt all zero: no node of the scan has a fraction block to solve, so every pixel ends with status 3, NaN outputs and no
    trial; from a given start the same call has cost 0.0 and status 0 where it stands."""
    t, sc, meas, st = exit_case(env)
    zero = np.zeros(20, dtype=np.float32)
    r, _, _ = against_host_loop(env, t, sc["kidx"], meas, w=zero)
    assert np.all(r["status"] == 3) and np.all(r["n_iter"] == 0) and all_nan(r, slice(None))
    r, _, _ = against_host_loop(env, t, sc["kidx"], meas, w=zero, start=(st["T"], st["frac"]))
    assert np.all(r["status"] == 0) and np.all(r["n_iter"] == 0) and np.all(r["cost"] == 0.0) and np.all(r["hess"] == 0.0)
    assert np.array_equal(r["T"], st["T"]) and np.array_equal(r["frac"], st["frac"])


def test_exit_nan_in_the_data(env):
    """One NaN in meas under a counting band of one pixel: status 3 for that pixel, from the scan and from a given start; its
    64 neighbours keep the bits of the clean run."""
    t, sc, meas, st = exit_case(env)
    m2, px = PC.nan_pixel(meas, int(np.flatnonzero(~t["dead"])[0]))
    others = np.arange(PC.NPIX) != px
    for start in (None, (st["T"], st["frac"])):
        clean, _, _ = against_host_loop(env, t, sc["kidx"], meas, start=start)
        r, _, _ = against_host_loop(env, t, sc["kidx"], m2, start=start)
        assert np.all(clean["status"] <= 1) and int(r["status"][px]) == 3 and int(r["n_iter"][px]) == 0 and all_nan(r, px)
        for key in r:
            assert np.array_equal(r[key][others], clean[key][others]), key


def test_exit_one_node(env):
    """One node: l' = 0, H_00 = 0 is no pivot, and a given start with wrong fractions is given up (status 3) after no trial."""
    _, sc, _, st = exit_case(env)
    t = tabs(env, 1, PC.EXIT["nEnd"])
    meas = GF.forward(env, t, sc)
    r, _, _ = against_host_loop(env, t, sc["kidx"], meas, start=(st["T"], st["frac"]))
    assert np.all(r["status"] == 3) and np.all(r["n_iter"] == 0) and all_nan(r, slice(None))


def _noisy_fit(env, t, sc, what):
    """meas = the forward's cube times (1 + 1e-3 N(0, 1)), ftol = 0, up to 200 trials from the scan, against the host loop."""
    mn = PC.noisy(GF.forward(env, t, sc))
    r, clamped, capped = against_host_loop(env, t, sc["kidx"], mn, k=200)
    print("%s: trials %d .. %d, statuses %s, %d trial temperatures clamped, %d lanes stopped at the cap of lambda, %d final T on an end"
          % (what, r["n_iter"].min(), r["n_iter"].max(), np.bincount(r["status"]).tolist(), clamped, capped,
             int(np.sum((r["T"] == PC.T_RANGE[0]) | (r["T"] == PC.T_RANGE[1])))))
    # at ftol = 0 a lane ends with status 0 only on a cost of 0.0 or at the cap of lambda
    assert np.all(r["status"] == 0) and np.all(r["cost"] > 0.0) and r["n_iter"].max() < 200 and capped == PC.NPIX
    return mn, r, clamped


def test_exit_lambda_cap(env):
    """The noisy scene: every pixel ends with status 0 and a cost above 0 before 200 trials, which at ftol = 0 only the cap of
    lambda does; T and the fractions agree with the fp64 restatement (fp32 roundings simulated) on the same meas and device
    tables within the sensitivity bound; a restart from the result at lambda0 = 1e11 stops after at most 2 trials where it is.
    MEASURED on an MI355X: 19 to 41 trials, 46 trial temperatures clamped, all 65 lanes stopped at the cap; |got - restatement| at
    most 0.968 of the sensitivity bound (the restatement takes 15 to 33 trials: the two stop at different points of a valley
    that is flat to fp32, and the bound is the width of that valley); the restart stops every lane after 1 trial."""
    t, sc, _, _ = exit_case(env)
    mn, r, _ = _noisy_fit(env, t, sc, "paths fit lambda cap")
    args = (t["N_h"], t["C_h"], t["G_h"], t["nodes"])
    with np.errstate(invalid="ignore"):
        want = FT.fit(*args, PC.T_RANGE, sc["kidx"], mn, max_iter=200, ftol=0.0, f32=True)
    u = lambda T, f: np.concatenate([np.asarray(T)[:, None], np.asarray(f).astype(np.float64)], axis=1)
    ratio = np.abs(u(r["T"], r["frac"]) - u(want["T"], want["frac"])) / FT.sensitivity_bound(*args, sc)
    print("paths fit lambda cap: worst |got - restatement| / bound = %.3g; the restatement's trials %d .. %d, statuses %s"
          % (ratio.max(), want["n_iter"].min(), want["n_iter"].max(), np.bincount(want["status"]).tolist()))
    assert np.all(ratio <= 1.0)
    again, _, capped = against_host_loop(env, t, sc["kidx"], mn, k=5, start=(r["T"], r["frac"]), lambda0=1e11)
    print("paths fit lambda cap: the restart at lambda0 = 1e11 takes %d .. %d trials" % (again["n_iter"].min(), again["n_iter"].max()))
    assert np.all(again["status"] == 0) and np.all(again["n_iter"] >= 1) and np.all(again["n_iter"] <= 2) and capped == PC.NPIX
    assert np.array_equal(again["T"], r["T"]) and np.array_equal(again["frac"], r["frac"]) and np.array_equal(again["cost"], r["cost"])


def test_exit_clamp(env):
    """The noisy scene with every true T on an end of the range: trial temperatures are clamped (the host loop counts them),
    and some final T is an end exactly.
    MEASURED on an MI355X: 19 to 51 trials, 851 trial temperatures clamped, 25 of the 65 final temperatures on an end."""
    t = exit_case(env)[0]
    se = PC.end_scene()
    _, r, clamped = _noisy_fit(env, t, se, "paths fit clamp")
    on_end = (r["T"] == PC.T_RANGE[0]) | (r["T"] == PC.T_RANGE[1])
    assert clamped > 0 and on_end.any() and np.all((r["T"] >= PC.T_RANGE[0]) & (r["T"] <= PC.T_RANGE[1]))


def test_exit_tie_in_the_scan(env):
    """Every node's rows equal to node 0's: every node of the scan has the same cost, and the first one wins, T == nodes[0] in
    every pixel; with the table as it is the scan picks other nodes too."""
    t, sc, meas, _ = exit_case(env)
    tab = PC.tie(t["tab"].cpu().numpy(), 1)
    assert np.array_equal(tab[:, 3], tab[:, 0]) and np.array_equal(tab[:, 0], t["tab"].cpu().numpy()[:, 0])
    tied = dict(t, tab=GF.dev(env, tab), G_h=tab.astype(np.float64).transpose(1, 2, 0))
    s = GF.fit(env, tied, sc["kidx"], meas, max_iter=0)
    assert np.all(s["status"] == 1) and np.all(s["T"] == t["nodes"][0])
    plain = GF.fit(env, t, sc["kidx"], meas, max_iter=0)
    assert np.all(plain["status"] == 1) and np.all(np.isin(plain["T"], t["nodes"])) and not np.all(plain["T"] == t["nodes"][0])
    against_host_loop(env, tied, sc["kidx"], meas)


# ------------------------------------------------------------------------------ 5. the adjoint's chunk doubling
@pytest.mark.parametrize("nPix", PC.CHUNK_NPIX)
def test_adjoint_chunk_doubles(env, nPix):
    """400 endmembers, 8 nodes, 80 bands, 8193 pixels: 33 chunks of 256 would take more than the workspace's 64 MiB, so the
    reduction runs 17 chunks of 512, the last of one pixel; 8449 pixels: 17 chunks too, the last of 257. All three outputs
    against the oracle; dT and dfrac of the first 257 pixels are the bits of the 257-pixel scene, which runs 2 chunks of 256.
    MEASURED on an MI355X, in units of 2^-24 scale: dT 0.24, dfrac 0.63 (k = 10), gL 1.24 (k = 3)."""
    c = dict(PC.CHUNK_CASE, nPix=nPix)
    assert PC.vjp_chunks(**c) == (512, 17) and PC.vjp_chunks(**dict(c, nPix=257)) == (256, 2)
    t = tabs(env, c["Q"], c["nEnd"], nB=c["nB"])
    sc = mixed_scene(c["nEnd"], c["nPix"])
    g = VC.cotangent(c["nB"], c["nPix"], t["dead"], seed=12)
    got, _ = GV.check_raw(env, t, sc, PC.T_RANGE, g, "paths vjp chunk doubled nPix=%d" % nPix)
    part = GV.raw(env, t, GV.cut(sc, slice(0, 257)), np.ascontiguousarray(g[:, :257]), outs=("dT", "dfrac"))
    assert np.array_equal(part["dT"], got["dT"][:257]) and np.array_equal(part["dfrac"], got["dfrac"][:257])
