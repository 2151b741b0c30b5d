"""Fused band radiances under tabulated response functions (radtxfr_amd/csrc/rtx_srf.hip: rtx_srf_moments; sensor.srf_moments,
sensor.band_radiance_srf_fused) against the fp64 NumPy of tests/srf_fused_cases.py on the float32 inputs the kernels receive.

Grid: 3 CH + 7 points at 0.01 cm^-1 from 900 cm^-1 (CH = rtx_srf_chunk_points()); 20 bands (two launch groups); emissivity
knots 1 cm^-1 apart over the middle of the grid ("coarse"), 0.003 cm^-1 apart ("dense", several knots per grid point) and on
grid points ("on_grid"). Bound of the parity cases: |got - want| <= 1e-5 of the band's largest |L| over the emissivities
(as test_gpu_srf.py::test_band_radiance_srf). MEASURED on an MI355X: in each test's docstring."""
import ctypes as C

import numpy as np
import pytest

import sensor_cases as SC
import srf_fused_cases as FC
from test_gpu_sensor_vjp import K_DE

pytestmark = pytest.mark.gpu

TOL = 1e-5


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    from radtxfr_amd import _lib, engine, sensor
    lib = _lib.load()
    return dict(torch=torch, lib=lib, engine=engine, sensor=sensor, CH=lib.rtx_srf_chunk_points(), K=lib.rtx_srf_max_knots(),
                MT=lib.rtx_srf_moments_max_temps())


def case(env, knots):
    return FC.case(env["CH"], env["K"], knots)


def dev_inputs(env, c):
    torch = env["torch"]
    return [torch.as_tensor(np.array(c[k]), device="cuda") for k in ("tau", "La", "Ld")]


def fused(env, c, nE, Ts, pick=None):
    """band_radiance_srf_fused on the device -> NumPy; pick: indices of the bands to take, in that order."""
    torch, sensor, engine = env["torch"], env["sensor"], env["engine"]
    tables = c["tables"] if pick is None else [c["tables"][b] for b in pick]
    s = sensor.Sensor.from_tables(tables)
    tau, La, Ld = dev_inputs(env, c)
    E = torch.as_tensor(np.ascontiguousarray(c["E"][:, :nE]), device="cuda")
    xo, L = sensor.band_radiance_srf_fused(engine.Grid(*FC.grid_tuple(env["CH"])), tau, La, Ld, c["Xk"], E, Ts, s)
    torch.cuda.synchronize()
    assert np.array_equal(xo, s.centres)
    return L.cpu().numpy()


def moments(env, c, Ts, pick=None):
    """sensor.srf_moments on the device -> (N, C, M, jrange) NumPy."""
    torch, sensor, engine = env["torch"], env["sensor"], env["engine"]
    tables = c["tables"] if pick is None else [c["tables"][b] for b in pick]
    s = sensor.Sensor.from_tables(tables)
    tau, La, Ld = dev_inputs(env, c)
    Xk_d = torch.as_tensor(np.array(c["Xk"]), device="cuda")
    out = sensor.srf_moments(engine.Grid(*FC.grid_tuple(env["CH"])), tau, La, Ld, Xk_d, Ts, s)
    torch.cuda.synchronize()
    return tuple(v.cpu().numpy() for v in out)


def worst(got, want, dead):
    """max over the live bands of |got - want| / the band's largest |want|; the NaN bands are NaN in exactly the same places."""
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.isnan(got), np.broadcast_to(dead[:, None], got.shape))
    live = ~dead
    return float(np.max((np.abs(got - want) / FC.band_max(want))[..., live, :]))


# ---------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("many", (False, True), ids=("Ts_scalar", "Ts_list"))
@pytest.mark.parametrize("nE", FC.NE_CASES)
@pytest.mark.parametrize("knots", FC.KNOT_SETS)
def test_parity(env, knots, nE, many):
    """Test 1: every finite band within 1e-5 of its largest |L| of the fp64 direct form, the NaN bands NaN in the same
    places. MEASURED: coarse 1.4e-7 (nE = 1, 3) to 2.9e-7 (nE = 260); on_grid 2.3e-7 to 4.7e-7; dense 1.8e-6 to 2.7e-6, the same
    for one and for three temperatures (dense: the band over the whole grid touches all 2000 knots, and rtx_band_mix adds
    them in one fp32 chain)."""
    c = case(env, knots)
    if many:
        got, want = fused(env, c, nE, list(FC.TS_LIST)), c["want"][:, :, :nE]
        assert got.shape == (3, 20, nE)
    else:
        got, want = fused(env, c, nE, FC.TS_SCALAR), c["want"][1, :, :nE]
        assert got.shape == (20, nE)
    e = worst(got, want, c["dead"])
    print("srf fused parity %s nE=%d nT=%d: max |got - want| / band max = %.3g" % (knots, nE, 3 if many else 1, e))
    assert e <= TOL


def test_against_unfused(env):
    """Test 2: band_radiance_srf (rtx_interp_knots -> rtx_apparent_radiance -> rtx_srf_apply) on the same inputs: the two
    within 2e-5 of the band maximum of each other, each within 1e-5 of the same fp64 value, NaN bands NaN in both.
    MEASURED: coarse fused 2.9e-7, unfused 1.09e-6, between them 1.07e-6; on_grid 4.7e-7, 1.20e-6, 1.19e-6."""
    torch, sensor, engine = env["torch"], env["sensor"], env["engine"]
    for knots in ("coarse", "on_grid"):
        c = case(env, knots)
        want = c["want"][1]
        got = fused(env, c, FC.NE_ALL, FC.TS_SCALAR)
        tau, La, Ld = dev_inputs(env, c)
        E = torch.as_tensor(np.array(c["E"]), device="cuda")
        _, un = sensor.band_radiance_srf(engine.Grid(*FC.grid_tuple(env["CH"])), tau, La, Ld, c["Xk"], E, FC.TS_SCALAR,
                                         sensor.Sensor.from_tables(c["tables"]))
        torch.cuda.synchronize()
        un = un.cpu().numpy()
        ef, eu = worst(got, want, c["dead"]), worst(un, want, c["dead"])
        live = ~c["dead"]
        d = float(np.max((np.abs(got - un) / FC.band_max(want))[live]))
        print("srf fused vs unfused %s: fused %.3g, unfused %.3g, between them %.3g of the band maximum" % (knots, ef, eu, d))
        assert ef <= TOL and eu <= TOL and d <= 2 * TOL


@pytest.mark.parametrize("knots", FC.KNOT_SETS)
def test_moments(env, knots):
    """Test 3: N against apply_srf(..., wsum=True)'s denominators (1e-6 relative, 0 for the NaN bands) and the fp64 N;
    jrange exactly the helper's first and last touched knot; C against the fp64 C (fp64 sums of fp32 terms: 1e-6); M is 0
    outside jrange and, element by element, within K_DE 2^-24 of its scale (srf_fused_cases.moments_scale: the same sum with
    every term's absolute value; K_DE = 32 is what tests/test_gpu_sensor_vjp.py allows dE = sum g M / N, which carries M's
    error and one rounding more). MEASURED on an MI355X, in units of 2^-24 scale: coarse 2.35, dense 3.9,
    on_grid 4.05 (62.6, 14.3 and 12.6 while the lower knot's weight was 1.0f - f of the rounded f: DESIGN.md 4.13)."""
    torch, sensor, engine = env["torch"], env["sensor"], env["engine"]
    c = case(env, knots)
    N, Cb, M, jr = moments(env, c, list(FC.TS_LIST))
    live = ~c["dead"]
    ones = torch.ones((c["X"].size, 1), dtype=torch.float32, device="cuda")
    _, _, den = sensor.apply_srf(sensor.Sensor.from_tables(c["tables"]), ones, grid=engine.Grid(*FC.grid_tuple(env["CH"])), wsum=True)
    den = den.cpu().numpy()
    assert N.shape == (20,) and M.shape == (3, 20, c["Xk"].size) and jr.dtype == np.int32
    assert np.all(N[c["dead"]] == 0.0) and np.all(Cb[c["dead"]] == 0.0) and np.all(den[c["dead"]] == 0.0)
    assert np.max(np.abs(N[live] / den[live] - 1.0)) <= 1e-6
    assert np.max(np.abs(N[live] / c["N"][live] - 1.0)) <= 1e-6
    assert np.array_equal(jr, c["jrange"])
    assert np.max(np.abs(Cb[live] / c["C"][live] - 1.0)) <= 1e-6
    assert np.any(M[:, live] != 0.0)
    for b in range(20):  # zeros outside the touched knots
        assert not M[:, b, :max(jr[b, 0], 0)].any() and not M[:, b, jr[b, 1] + 1:].any()
    e = FC.moments_error(M, c["M"], c["Ma"])
    print("srf fused moments %s: max |M - want| / (2^-24 scale) = %.3g (k = %d)" % (knots, e, K_DE))
    assert M.dtype == np.float32 and e <= K_DE


@pytest.mark.parametrize("knots", FC.KNOT_SETS)
def test_purity(env, knots):
    """Test 4: the same bits for the bands in reverse order and for a subset of three, for a subset of the temperatures in
    another order, and run to run."""
    c = case(env, knots)
    full = moments(env, c, list(FC.TS_LIST))
    again = moments(env, c, list(FC.TS_LIST))
    for a, b in zip(full, again):
        assert np.array_equal(a, b, equal_nan=True)
    order = list(range(19, -1, -1))
    rev = moments(env, c, list(FC.TS_LIST), pick=order)
    sub = moments(env, c, list(FC.TS_LIST), pick=list(FC.SUBSET))
    for (N, Cb, M, jr), pick in ((rev, order), (sub, list(FC.SUBSET))):
        assert np.array_equal(N, full[0][pick]) and np.array_equal(Cb, full[1][pick])
        assert np.array_equal(M, full[2][:, pick]) and np.array_equal(jr, full[3][pick])
    two = moments(env, c, [FC.TS_LIST[2], FC.TS_LIST[0]])
    assert np.array_equal(two[2][0], full[2][2]) and np.array_equal(two[2][1], full[2][0])
    assert np.array_equal(two[0], full[0]) and np.array_equal(two[1], full[1]) and np.array_equal(two[3], full[3])


def test_temperature_groups(env):
    """Test 5: one temperature more than a call of rtx_srf_moments takes: the grouped call equals the scalar calls, bit for bit."""
    c = case(env, "coarse")
    Ts = list(np.linspace(255.0, 335.0, env["MT"] + 1))
    pick = list(FC.SUBSET)
    got = fused(env, c, 1, Ts, pick=pick)
    assert got.shape == (env["MT"] + 1, 3, 1) and np.all(np.isfinite(got))
    for t, T in enumerate(Ts):
        assert np.array_equal(got[t], fused(env, c, 1, float(T), pick=pick)), t
    assert not np.array_equal(got[0], got[-1])


def test_tie_to_mako_fused(env):
    """Test 6: Sensor.mako against band_radiance_fused(kind=0) on BBM_GRID. Where a triangle reaches neither end point of a
    uniform grid the trapezoid cells are one constant and the two definitions coincide: within 2e-5 of the band maximum.
    Of the 21 MAKO bands inside BBM_GRID three reach an end point, where the cell is half as wide, and are left out: one at
    the low end and two at the high end (at most two at either end). MEASURED: 18 of 21 bands, 7.0e-7."""
    torch, sensor, engine = env["torch"], env["sensor"], env["engine"]
    X = SC.bbm_axis()
    d = SC.bbm_inputs()
    Xk = SC.bbm_knot_sets()["on_grid"]
    E = np.random.default_rng(17).uniform(0.55, 1.0, (Xk.size, 8)).astype(np.float32)
    grid = engine.Grid(*SC.BBM_GRID)
    f32 = lambda a: torch.as_tensor(a, device="cuda")
    s = sensor.Sensor.mako(X[0], X[-1])
    xo, mako = sensor.band_radiance_fused(grid, f32(d["tau"]), f32(d["La"]), f32(d["Ld"]), Xk, f32(E), SC.BBM_TS, kind=0)
    _, got = sensor.band_radiance_srf_fused(grid, f32(d["tau"]), f32(d["La"]), f32(d["Ld"]), Xk, f32(E), SC.BBM_TS, s)
    torch.cuda.synchronize()
    mako, got = mako.cpu().numpy(), got.cpu().numpy()
    _, cen, sig = sensor.mako_bands(X[0], X[-1])
    assert got.shape == mako.shape == (cen.size, 8) and np.allclose(xo, s.centres, rtol=1e-12)
    low, high = cen - sig <= X[0], cen + sig >= X[-1]
    inside = ~(low | high)
    print("srf fused vs MAKO fused: %d of %d bands, %d left out at the low end, %d at the high end" % (inside.sum(), cen.size, low.sum(), high.sum()))
    assert low.sum() <= 2 and high.sum() <= 2 and inside.sum() >= cen.size - 3
    e = float(np.max(np.abs(got[inside] - mako[inside]) / np.max(np.abs(mako[inside]), axis=1, keepdims=True)))
    print("srf fused vs MAKO fused: max difference / band maximum = %.3g" % e)
    assert np.all(np.isfinite(got)) and e <= 2 * TOL


def test_refusals_write_nothing(env):
    """Test 7: every refused call returns non-zero and leaves N, C, M and jrange alone; nB == 0 returns 0 and writes nothing;
    the same arguments, well formed, do write."""
    torch, lib, K, MT = env["torch"], env["lib"], env["K"], env["MT"]
    from radtxfr_amd import _lib
    nx, nk = 300, 6
    g = _lib.make_grid(1000.0, 1002.99, nx)
    tau, La, Ld = (torch.full((nx,), v, dtype=torch.float32, device="cuda") for v in (0.7, 1.0, 2.0))
    Xk = torch.as_tensor(np.linspace(1000.5, 1002.5, nk), device="cuda")
    kx = torch.as_tensor(np.concatenate([np.linspace(1000.1, 1002.5, K), [1000.2, 1000.6, 1001.0, 1001.4]]), device="cuda")
    kr = torch.ones(K + 4, dtype=torch.float32, device="cuda")
    N = torch.full((2,), 7.0, dtype=torch.float32, device="cuda")
    Cb = torch.full((2,), 7.0, dtype=torch.float32, device="cuda")
    M = torch.full((MT, 2, nk), 7.0, dtype=torch.float32, device="cuda")
    jr = torch.full((2, 2), 7, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    Ts_ok = np.linspace(280.0, 320.0, MT + 1)

    def call(start, nT=1, Ts=Ts_ok, nB=None, nk_=nk, tau_=tau, M_=M, grid=C.byref(g)):
        s = np.asarray(start, dtype=np.int32)
        return lib.rtx_srf_moments(grid, p(tau_), p(La), p(Ld), Ts.ctypes.data_as(C.c_void_p), nT, p(Xk), nk_, len(start) - 1 if nB is None else nB,
                                   s.ctypes.data_as(C.c_void_p), p(kx), p(kr), p(N), p(Cb), p(M_), p(jr), st)

    bad_grid = _lib.make_grid(1000.0, 1002.99, nx)
    bad_grid.n = nx + 5  # a shard that runs past its grid
    for start, kw in (([0, 3], dict(nT=0)), ([0, 3], dict(nT=MT + 1)), ([0, K + 1], {}), ([0, 3, 4], {}), ([0, 1], {}), ([0, 3, 1], {}),
                      ([3, 0, 3], {}), ([0, 3], dict(nk_=0)), ([0, 3], dict(tau_=None)), ([0, 3], dict(M_=None)),
                      ([0, 3], dict(Ts=np.array([300.0, -1.0]), nT=2)), ([0, 3], dict(nB=-1)), ([0, 3], dict(grid=C.byref(bad_grid)))):
        assert call(start, **kw) != 0, (start, kw)
        assert lib.rtx_last_error()
    assert call([0, 3], nB=0) == 0
    torch.cuda.synchronize()
    for v in (N, Cb, M):
        assert bool((v == 7.0).all())
    assert bool((jr == 7).all())
    assert call([0, K, K + 4], nT=MT) == 0  # and the same arguments, well formed, do write
    torch.cuda.synchronize()
    assert bool(torch.isfinite(N).all()) and bool((N != 7.0).all()) and bool((Cb != 7.0).all()) and bool((M != 7.0).all())
    assert bool((jr != 7).all())
