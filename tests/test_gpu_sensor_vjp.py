"""The sensor stage's adjoint (radtxfr_amd/csrc/rtx_srf_vjp.hip: rtx_srf_radiance_vjp; sensor.band_radiance_srf_vjp,
rt.compute_band_radiance_vjp) against the fp64 NumPy of tests/sensor_vjp_cases.py on the float32 inputs the kernels receive,
against the shipped forward kernels, and bit for bit against itself.

Shapes: the forward's own (tests/srf_fused_cases.py): 3 CH + 7 points, 20 bands (more than one forward launch group; a
chunk-boundary boxcar, a sub-grid-step triangle, three dead bands, half-off-grid bands, a 65-knot Gaussian, a K-knot table,
two identical bands, five overlapping triangles, a two-row band across a chunk boundary), the coarse / dense / on_grid
emissivity knots, nE in {1, 3, 260}. The cotangent is random of both signs and NaN on the dead bands throughout.

Bound of the oracle cases: |got - want| <= k 2^-24 scale, element by element, scale = the oracle's sum of the absolute
values of the same terms, k = the fp32 roundings along the kernel's chain (counted at K_* below; an operation good to one
ulp, v_exp_f32, v_rcp_f32 and the fp32 division, counts as two)."""
import numpy as np
import pytest

import srf_fused_cases as FC
import sensor_vjp_cases as VC

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
# B(nu, Ts) of planck_f32: the exponent's fraction (1), v_exp_f32 (2), e - 1 (1), v_rcp_f32 (2), (float)c1x3 (1), the product (1)
K_PLANCK = 8
# A_t: the weight w (1), N (1), H (1), the hats f and 1 - f (2); everything after that is fp64
K_A = 5
K_ROW = {"G_tau": K_A + K_PLANCK + 1,  # A_t (B_t - Ld) + S Ld, rounded once on the way out
         "G_La": 1 + 1 + 1,            # S: w, N, and the store
         "G_Ld": K_A + 1}              # tau (S - sum_t A_t) and the store
# dB/dT = B (float)uT (1 + B / (float)c1x3): B (8), uT (1), c1x3 (1), the division (2), 1 + . (1), two products (2)
K_DTS = K_A + K_PLANCK + 7
# dE = sum g M / N. M's terms: w (1), tau (B - Ld) (8 + 2), w . (1), the hat (2); then fp32 chains of up to 64 additions whose
# roundings are each relative to a partial sum: no count bounds their worst case, their expected growth is sqrt(64) = 8.
# 14 + 8 + M's and N's stores (2) = 24; held at the 32 the definition of this test allows at most.
K_DE = 32


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


def full_grid(env):
    return env["engine"].Grid(*FC.grid_tuple(env["CH"]))


def run(env, c, nE, Ts, g, pick=None, grid=None, rows=slice(None), outputs=None, **over):
    """sensor.band_radiance_srf_vjp on the device -> dict of NumPy. pick: the bands to take, in that order (g is then the
    picked bands' cotangent); grid / rows: a shard and the rows of tau, La, Ld that belong to it; over: inputs replaced."""
    torch, sensor = env["torch"], env["sensor"]
    tables = c["tables"] if pick is None else [c["tables"][b] for b in pick]
    s = sensor.Sensor.from_tables(tables)
    tau, La, Ld = (torch.as_tensor(np.array(over.get(k, c[k]), dtype=np.float32)[rows], device="cuda") for k in ("tau", "La", "Ld"))
    E = torch.as_tensor(np.array(c["E"][:, :nE]), device="cuda")
    kw = {} if outputs is None else dict(outputs=outputs)
    out = sensor.band_radiance_srf_vjp(full_grid(env) if grid is None else grid, tau, La, Ld, c["Xk"], E, Ts, s,
                                       torch.as_tensor(np.array(g), device="cuda"), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def forward(env, c, nE, Ts, **over):
    torch, sensor = env["torch"], env["sensor"]
    tau, La, Ld = (torch.as_tensor(np.array(over.get(k, c[k]), dtype=np.float32), device="cuda") for k in ("tau", "La", "Ld"))
    E = torch.as_tensor(np.array(c["E"][:, :nE]), device="cuda")
    _, L = sensor.band_radiance_srf_fused(full_grid(env), tau, La, Ld, c["Xk"], E, Ts, sensor.Sensor.from_tables(c["tables"]))
    torch.cuda.synchronize()
    return L.cpu().numpy()


def within(got, want, scale, k, what):
    """max over the elements of |got - want| / (2^-24 scale) against k; elements of scale 0 must be equal."""
    got, want, scale = (np.asarray(v, dtype=np.float64) for v in (got, want, scale))
    assert got.shape == want.shape and np.all(np.isfinite(got)), what
    zero = scale == 0.0
    assert np.array_equal(got[zero], want[zero]), what
    e = float(np.max(np.abs(got - want)[~zero] / (EPS * scale[~zero]))) if (~zero).any() else 0.0
    print("%s: max |got - want| / (2^-24 scale) = %.3g (k = %d)" % (what, e, k))
    assert e <= k, what


def check_against_oracle(got, o, what, extra=0):
    for key in ("G_tau", "G_La", "G_Ld"):
        assert got[key].dtype == np.float32
        within(got[key], o[key], o["scale"][key], K_ROW[key] + extra, what + " " + key)
    assert got["Ts"].dtype == np.float64 and got["emis"].dtype == np.float64
    within(np.atleast_1d(got["Ts"]), o["dTs"], o["scale"]["dTs"], K_DTS, what + " dTs")
    within(got["emis"], o["dE"], o["scale"]["dE"], K_DE, what + " dE")


# ---------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("many", (False, True), ids=("Ts_scalar", "Ts_list"))
@pytest.mark.parametrize("nE", FC.NE_CASES)
@pytest.mark.parametrize("knots", FC.KNOT_SETS)
def test_against_oracle(env, knots, nE, many):
    """Test 1: the three rows point by point, dTs and dE element by element, within k 2^-24 of the oracle's scale.
    MEASURED on an MI355X, worst over the 18 cases, in units of 2^-24 scale: G_tau 2.76 (k = 14), G_La 2.17 (k = 3),
    G_Ld 0.72 (k = 6), dTs 0.40 (k = 20), dE 3.24 (k = 32; on_grid knots, 3.03 dense, 1.63 coarse; 11.8 on the dense knots before
    the forward's M took both knot weights from srfm_hats)."""
    c = case(env, knots)
    g, o = VC.case_adjoint(env["CH"], env["K"], knots, nE, many)
    got = run(env, c, nE, list(FC.TS_LIST) if many else FC.TS_SCALAR, g if many else g[0])
    assert got["G_tau"].shape == (c["X"].size,) and got["emis"].shape == (c["Xk"].size, nE)
    assert got["Ts"].shape == ((3,) if many else ())
    check_against_oracle(got, o, "sensor vjp %s nE=%d nT=%d" % (knots, nE, 3 if many else 1))


def test_exact_zeros(env):
    """Test 2: points under no live band are == 0.0 in all three rows; NaN in g on the dead bands leaves every output
    finite; g == 0 gives zeros everywhere."""
    c = case(env, "coarse")
    pick = [0, 4, 5, 6, 13]  # rows 100 .. 400 and 700 .. 900 and the three dead bands
    g = VC.cotangent(1, 20, 3, c["dead"])[0][pick]
    assert np.isnan(g[1:4]).all()
    got = run(env, c, 3, FC.TS_SCALAR, g, pick=pick)
    X = c["X"]
    under = np.zeros(X.size, dtype=bool)
    for b in (0, 13):
        under |= (X >= c["tables"][b][0][0]) & (X <= c["tables"][b][0][-1])
    assert under.sum() == 301 + 201
    for k in ("G_tau", "G_La", "G_Ld"):
        assert np.all(np.isfinite(got[k])) and np.all(got[k][~under] == 0.0) and np.all(got[k][under] != 0.0), k
    assert np.isfinite(got["Ts"]) and got["Ts"] != 0.0 and np.all(np.isfinite(got["emis"])) and got["emis"].any()
    full = run(env, c, 3, list(FC.TS_LIST), VC.cotangent(3, 20, 3, c["dead"]))
    assert all(np.all(np.isfinite(v)) for v in full.values())
    g0 = np.zeros((20, 3), dtype=np.float32)
    g0[c["dead"]] = np.nan
    for k, v in run(env, c, 3, FC.TS_SCALAR, g0).items():
        assert not v.any(), k


@pytest.mark.parametrize("knots", FC.KNOT_SETS)
def test_inner_product_against_the_forward_kernels(env, knots):
    """Test 3, no oracle: L is linear in each of tau, La, Ld, so sum_i G . d = sum g . (L(x + d) - L(x)) with L from
    band_radiance_srf_fused, within twice the forward's own asserted 1e-5 of sum |g| band_max.
    MEASURED on an MI355X: |difference| at most 9.9e-6 against a bound of 5.4e-3."""
    nE = 3
    c = case(env, knots)
    live = ~c["dead"]
    g = VC.cotangent(1, 20, nE, c["dead"], seed=9)[0]
    got = run(env, c, nE, FC.TS_SCALAR, g)
    L1 = forward(env, c, nE, FC.TS_SCALAR)
    bound = 2 * 1e-5 * float(np.sum(np.abs(g[live].astype(np.float64)) * FC.band_max(L1[live].astype(np.float64))))
    for key, G, frac in (("tau", "G_tau", 0.3), ("La", "G_La", 0.2), ("Ld", "G_Ld", 0.2)):
        x2 = (c[key] * np.float32(1.0 + frac)).astype(np.float32)
        d = x2.astype(np.float64) - c[key].astype(np.float64)  # the step the forward kernel is really given
        L2 = forward(env, c, nE, FC.TS_SCALAR, **{key: x2})
        lhs = float(np.sum(got[G].astype(np.float64) * d))
        rhs = float(np.sum(g[live].astype(np.float64) * (L2[live].astype(np.float64) - L1[live].astype(np.float64))))
        print("sensor vjp inner product %s d%s: %.9g vs %.9g, |diff| = %.3g, bound %.3g" % (knots, key, lhs, rhs, abs(lhs - rhs), bound))
        assert abs(lhs - rhs) <= bound


@pytest.mark.parametrize("knots", FC.KNOT_SETS)
def test_bit_identity(env, knots):
    """Test 4: the same bits run to run; for SUBSET's bands alone at the points only they cover; for a shard that holds a
    band's full support, at that band's points; for each output asked for alone; and N equal to rtx_srf_moments' N."""
    torch, sensor, CH = env["torch"], env["sensor"], env["CH"]
    nE = 3
    c = case(env, knots)
    X = c["X"]
    g = VC.cotangent(3, 20, nE, c["dead"])
    Ts = list(FC.TS_LIST)
    full = run(env, c, nE, Ts, g)
    again = run(env, c, nE, Ts, g)
    for k in full:
        assert np.array_equal(full[k], again[k]), k
    cover = lambda b: (X >= c["tables"][b][0][0]) & (X <= c["tables"][b][0][-1])
    # the bands of SUBSET alone, at the points no other band covers
    pick = list(FC.SUBSET)
    others = np.zeros(X.size, dtype=bool)
    for b in range(20):
        if b not in pick:
            others |= cover(b)
    only = ~others
    assert only.sum() > 100 and (only & cover(16)).any()
    sub = run(env, c, nE, Ts, g[:, pick], pick=pick)
    for k in ("G_tau", "G_La", "G_Ld"):
        assert np.array_equal(sub[k][only], full[k][only]) and sub[k][only].any(), k
    # shards that hold the full support of band 3 (rows ~1498 .. 1502; with bands 1 and 14, which reach across the first
    # chunk boundary): the band's points get the bits of the whole grid. Offsets are multiples of the chunk.
    pick = [1, 3, 14]
    whole = run(env, c, nE, Ts, g[:, pick], pick=pick)
    at3 = np.flatnonzero(cover(3))
    assert at3.size >= 3 and not (cover(1) | cover(14))[at3].any()
    for off, n in ((0, 2 * CH), (CH, CH + 100)):
        part = run(env, c, nE, Ts, g[:, pick], pick=pick, grid=full_grid(env).shard(off, n), rows=slice(off, off + n))
        for k in ("G_tau", "G_La", "G_Ld"):
            assert part[k].shape == (n,)
            assert np.array_equal(part[k][at3 - off], whole[k][at3]) and whole[k][at3].all(), (k, off)
    # each output alone
    for k in ("G_tau", "G_La", "G_Ld", "Ts", "emis"):
        alone = run(env, c, nE, Ts, g, outputs=(k,))
        assert list(alone) == [k] and np.array_equal(alone[k], full[k]), k
    # N against the forward's
    s = sensor.Sensor.from_tables(c["tables"])
    tau, La, Ld = (torch.as_tensor(np.array(c[k]), device="cuda") for k in ("tau", "La", "Ld"))
    N_fwd = sensor.srf_moments(full_grid(env), tau, La, Ld, torch.as_tensor(np.array(c["Xk"]), device="cuda"), [FC.TS_SCALAR], s)[0]
    N = sensor.srf_norms(full_grid(env), s, dev=tau.device)
    torch.cuda.synchronize()
    N, N_fwd = N.cpu().numpy(), N_fwd.cpu().numpy()
    assert N.dtype == np.float32 and np.array_equal(N, N_fwd) and np.array_equal(N == 0.0, c["dead"])


def test_temperature_groups(env):
    """Test 5: one temperature more than a call of rtx_srf_radiance_vjp takes: against the oracle for the whole list, within
    test 1's bound (the rows: two more roundings, each group's float32 rows are added in float64 and rounded once).
    MEASURED on an MI355X, in units of 2^-24 scale: G_tau 0.79, G_La 0.64, G_Ld 0.14, dTs 0.13, dE 0.35."""
    c = case(env, "coarse")
    nE, MT = 3, env["MT"]
    Ts = list(np.linspace(255.0, 335.0, MT + 1))
    g = VC.cotangent(MT + 1, 20, nE, c["dead"], seed=13)
    o = VC.adjoint(c["X"], c["tables"], c["tau"], c["La"], c["Ld"], c["Xk"], c["E"][:, :nE], Ts, g)
    got = run(env, c, nE, Ts, g)
    assert got["Ts"].shape == (MT + 1,)
    check_against_oracle(got, o, "sensor vjp %d temperatures" % (MT + 1), extra=2)


def test_refusals_write_nothing(env):
    """A refused call returns non-zero and leaves every output alone; the same arguments, well formed, do write."""
    import ctypes as C
    from radtxfr_amd import _lib
    torch, lib, MT = env["torch"], env["lib"], env["MT"]
    nx, nk, nE = 300, 6, 2
    gr = _lib.make_grid(1000.0, 1002.99, nx)
    tau, La, Ld = (torch.full((nx,), v, dtype=torch.float32, device="cuda") for v in (0.7, 1.0, 2.0))
    Xk = torch.as_tensor(np.linspace(1000.5, 1002.5, nk), device="cuda")
    kx = torch.as_tensor(np.array([1000.2, 1000.6, 1001.0, 1001.4]), device="cuda")
    kr = torch.ones(4, dtype=torch.float32, device="cuda")
    E = torch.full((nk, nE), 0.9, dtype=torch.float32, device="cuda")
    g = torch.ones((MT, 1, nE), dtype=torch.float32, device="cuda")
    G = [torch.full((nx,), 7.0, dtype=torch.float32, device="cuda") for _ in range(3)]
    dTs = torch.full((MT,), 7.0, dtype=torch.float64, device="cuda")
    dE = torch.full((nk, nE), 7.0, dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    Ts = np.linspace(280.0, 320.0, MT + 1)

    def call(start=(0, 4), nT=1, Ts_=Ts, nk_=nk, nE_=nE, E_=E, g_=g, outs=True):
        s = np.asarray(start, dtype=np.int32)
        o = [p(v) for v in G + [dTs, dE]] if outs else [None] * 5
        return lib.rtx_srf_radiance_vjp(C.byref(gr), p(tau), p(La), p(Ld), Ts_.ctypes.data_as(C.c_void_p), nT, p(Xk), nk_, len(start) - 1,
                                        s.ctypes.data_as(C.c_void_p), p(kx), p(kr), p(E_), nE_, p(g_), *o, st)

    for kw in (dict(nT=0), dict(nT=MT + 1), dict(start=(0, 1)), dict(start=(0, 3, 1)), dict(nk_=0), dict(nE_=0), dict(E_=None),
               dict(g_=None), dict(Ts_=np.array([300.0, -1.0]), nT=2), dict(outs=False)):
        assert call(**kw) != 0, kw
        assert lib.rtx_last_error()
    torch.cuda.synchronize()
    for v in G + [dTs, dE]:
        assert bool((v == 7.0).all())
    assert call(nT=MT) == 0
    torch.cuda.synchronize()
    for v in G + [dTs, dE]:
        assert bool(torch.isfinite(v).all()) and bool((v != 7.0).any())
    assert bool((G[1][:15] == 0.0).all())  # below the band's first knot


@pytest.mark.parametrize("thin", (1.0, 1e-3), ids=("standard", "thinned"))
def test_compute_band_radiance_vjp_end_to_end(thin):
    """Test 6: rt.compute_band_radiance_vjp on 1000.0 .. 1000.5 cm^-1 at 0.0005 (make_spectral_axis: 1000 points, as
    test_gpu_tud_vjp.py::test_compute_tud_vjp_end_to_end's axis), the standard 66 layers and the
    12 cm^-1-padded subset of the seed-C3 table: L is band_radiance_srf_fused's on compute_TUD's outputs, bit for bit; the
    atmospheric gradients are compute_TUD_vjp's on the downloaded rows of band_radiance_srf_vjp; the surface gradients are
    that call's. The synthetic table is opaque at the standard mixing ratios (tau = 0: the surface is not seen and its
    gradients are exact zeros); the second case thins them a thousandfold, as smoke() does, so that every term is live."""
    import torch
    assert torch.cuda.is_available()
    from radtxfr_amd import engine, sensor, synthetic
    from radtxfr_amd import radiative_transfer as rt
    lo, hi, dv = 1000.0, 1000.5, 0.0005
    full = synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)
    sub = synthetic.subset_table(full, lo - 12.0, hi + 12.0)
    sa = rt.StdAtmos
    a = dict(Zs=sa[:, 1], Ts=sa[:, 5].copy(), Ps=sa[:, 4], PLs=sa[:, 3], MFs_VAL=sa[:, 6:9] * 1e6 * thin,
             MFs_ID=np.array([1, 2, 3]))
    wrt = ("T", 1, 3)
    kw = dict(DVOUT=dv, line_table=sub, Altitudes=np.array([8.0]), **a)
    # four triangles: two overlapping, one wholly off the axis (NaN in L, nothing in any gradient)
    s = sensor.Sensor.from_shape([1000.10, 1000.14, 1000.38, 1003.0], 0.06, "triangle")
    Xk = np.array([999.9, 1000.07, 1000.2, 1000.33, 1000.6])
    nB, nk, nE, n_vec, Ts_s = 4, 5, 3, 2, 296.0
    rng = np.random.default_rng(3)
    E = rng.uniform(0.6, 1.0, (nk, nE)).astype(np.float32)
    cot = rng.normal(size=(nB, nE, n_vec)).astype(np.float32)
    cot[3, :, 0] = np.nan
    X_out, L, grad = rt.compute_band_radiance_vjp(lo, hi, s, Xk, E, Ts_s, cot, wrt=wrt, **kw)
    assert np.array_equal(X_out, s.centres) and L.shape == (nB, nE) and L.dtype == np.float32
    assert set(grad) == set(wrt) | {"Ts_surface", "emis"}
    X, tau, La, Ld = rt.compute_TUD(lo, hi, **kw)
    nX, nL = X.size, a["Ts"].size
    assert nX == 1000 and nL == 66
    grid = engine.Grid(lo, hi, nX)
    dev32 = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float32).ravel(), device="cuda")
    t_d, a_d, d_d, E_d = dev32(tau), dev32(La), dev32(Ld), torch.as_tensor(E, device="cuda")
    L_want = sensor.band_radiance_srf_fused(grid, t_d, a_d, d_d, Xk, E_d, Ts_s, s)[1].cpu().numpy()
    assert np.array_equal(L, L_want, equal_nan=True) and np.isnan(L[3]).all() and np.isfinite(L[:3]).all()
    rows = [{k: v.cpu().numpy() for k, v in sensor.band_radiance_srf_vjp(grid, t_d, a_d, d_d, Xk, E_d, Ts_s, s, cot[..., v]).items()}
            for v in range(n_vec)]
    stack = lambda k: np.stack([r[k] for r in rows], axis=-1)
    _, _, _, _, want = rt.compute_TUD_vjp(lo, hi, {"tau": stack("G_tau"), "La": stack("G_La"), "Ld": stack("G_Ld")}, wrt=wrt, **kw)
    for w in wrt:
        assert grad[w].shape == (nL, n_vec) and grad[w].dtype == np.float64
        assert np.array_equal(grad[w], want[w]), w
    # species 3 has no lines in the table: exact zeros; the layers between the ground and the sensor carry a gradient
    assert np.all(grad[3] == 0.0) and np.count_nonzero(grad["T"]) >= 2 * n_vec and np.count_nonzero(grad[1]) >= 2 * n_vec
    assert grad["Ts_surface"].shape == (n_vec,) and grad["emis"].shape == (nk, nE, n_vec)
    assert np.array_equal(grad["Ts_surface"], stack("Ts")) and np.array_equal(grad["emis"], stack("emis"))
    assert np.all(np.isfinite(grad["emis"])) and np.all(np.isfinite(grad["Ts_surface"]))
    if thin < 1.0:
        assert tau.min() > 0.0 and np.all(grad["Ts_surface"] != 0.0) and np.count_nonzero(grad["emis"]) > nk * nE
    one = rt.compute_band_radiance_vjp(lo, hi, s, Xk, E, Ts_s, cot[..., 1], wrt=wrt, layers=[65, 3, 8], **kw)[2]
    for w in wrt:
        assert one[w].shape == (3,) and np.array_equal(one[w], grad[w][[65, 3, 8], 1])
    assert one["Ts_surface"].shape == () and one["Ts_surface"] == grad["Ts_surface"][1]
    assert np.array_equal(one["emis"], grad["emis"][..., 1])
