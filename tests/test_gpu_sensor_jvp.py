"""The sensor stage's tangent (radtxfr_amd/csrc/rtx_srf_jvp.hip: rtx_srf_radiance_jvp; sensor.band_radiance_srf_jvp,
rt.compute_band_radiance_jvp) against the fp64 NumPy of tests/sensor_jvp_cases.py on the float32 inputs the kernels receive,
against the shipped adjoint and forward kernels, and bit for bit against itself.

Shapes: the forward's own (tests/srf_fused_cases.py): 3 CH + 7 points, 20 bands (more than one launch group; a
chunk-boundary boxcar, a sub-grid-step triangle, three dead bands, a 65-knot Gaussian, a K-knot table), the coarse / dense /
on_grid emissivity knots, nE in {1, 3, 260}. The tangents are random of both signs (sensor_jvp_cases.tangents).

Bound of the oracle cases: |got - want| <= k 2^-24 scale, element by element, scale = the oracle's sum of the absolute
values of the same terms, k = the fp32 roundings along the kernel's chain for the input group that moves (K_TERM below; an
operation good to one ulp, v_exp_f32, v_rcp_f32 and the fp32 division, counts as two). c', m', every product with the
weight and a hat and every sum are fp64 in the kernels and add nothing to the count."""
import numpy as np
import pytest

import srf_fused_cases as FC
import sensor_vjp_cases as VC
import sensor_jvp_cases as JC
from test_gpu_sensor_vjp import K_ROW, K_DTS, K_DE, K_PLANCK

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
TOL_L = 1e-5          # the forward's asserted accuracy, of the band maximum (tests/test_gpu_srf_fused.py)
U32 = 2.0 ** -24
F32_TINY = 2.0 ** -126
F32_FLOOR = 1e-30     # tests/test_gpu_tud_jvp.py
# the roundings of a term of dL, by the input group that moves:
K_TERM = {
    "d_La": 1 + 1 + 1,                   # w d_La / N: the weight w, N, the store
    "d_tau": 1 + K_PLANCK + 2 + 1 + 1,   # w d_tau (B - Ld) hat E / N: w, B (8), the hats f and 1 - f, N, the store (w d_tau Ld / N: 3)
    "d_Ld": 1 + 2 + 1 + 1,               # w tau d_Ld (1 - hat E) / N: w, the hats, N, the store
    "d_Ts": 1 + (K_PLANCK + 7) + 2 + 1 + 1,  # w tau dB/dT d_Ts hat E / N: w, dB/dT (B and 7 more, K_DTS of the adjoint's test), hats, N, store
    # M d_E / N with the forward's fp32 M: w (1), tau (B - Ld) (8 + 2), w . (1), the hat (2), fp32 chains of up to 64 additions
    # (no count bounds them; expected growth sqrt(64) = 8), M's store, N, this store (3): 25, held at the 32 allowed at most
    "d_E": 32,
}
assert max(K_TERM.values()) <= 32
# the vectors of a many-vector case: which groups move in vector v (the others are zeros), v modulo 4
SUBSETS = (JC.GROUPS, ("d_tau", "d_La"), ("d_Ld", "d_Ts"), ("d_E",))
k_of = lambda only: max(K_TERM[g] for g in only)


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    from radtxfr_amd import _lib, engine, sensor
    lib = _lib.load()
    return dict(torch=torch, lib=lib, engine=engine, sensor=sensor, CH=lib.rtx_srf_chunk_points(), K=lib.rtx_srf_max_knots(),
                NV=lib.rtx_srf_radiance_jvp_max_vectors(), MT=lib.rtx_srf_radiance_jvp_max_temps())


def case(env, knots):
    return FC.case(env["CH"], env["K"], knots)


def full_grid(env):
    return env["engine"].Grid(*FC.grid_tuple(env["CH"]))


def stacked(ds):
    """A list of tangent dicts (one per vector) -> one dict with a trailing vector axis; a group that no vector carries
    stays None, one that some carry gets zeros in the others."""
    out = {}
    for key in JC.GROUPS:
        have = [d[key] for d in ds if d[key] is not None]
        out[key] = None if not have else np.stack([np.zeros_like(have[0]) if d[key] is None else d[key] for d in ds], axis=-1)
    return out


def run(env, c, nE, Ts, d, pick=None, **over):
    """sensor.band_radiance_srf_jvp on the device -> (L, dL) NumPy. d: a tangent dict (sensor_jvp_cases' keys), with or
    without a trailing vector axis; d_Ts is given for the temperatures of Ts. pick: the bands to take, in that order."""
    torch, sensor = env["torch"], env["sensor"]
    tables = c["tables"] if pick is None else [c["tables"][b] for b in pick]
    s = sensor.Sensor.from_tables(tables)
    dev = lambda v: None if v is None else torch.as_tensor(np.array(v, dtype=np.float32), device="cuda")
    tau, La, Ld = (dev(over.get(k, c[k])) for k in ("tau", "La", "Ld"))
    E = dev(over.get("E", c["E"][:, :nE]))
    d_Ts = d["d_Ts"]
    if d_Ts is not None and np.ndim(Ts) == 0:
        d_Ts = np.asarray(d_Ts)[0]  # a scalar Ts takes a tangent shaped like it (plus the vector axis)
    L, dL = sensor.band_radiance_srf_jvp(full_grid(env), tau, La, Ld, c["Xk"], E, Ts, s, d_tau=dev(d["d_tau"]), d_La=dev(d["d_La"]),
                                         d_Ld=dev(d["d_Ld"]), d_Ts=d_Ts, d_emis=dev(d["d_E"]))
    torch.cuda.synchronize()
    assert L.dtype == torch.float32 and dL.dtype == torch.float32
    return L.cpu().numpy(), dL.cpu().numpy()


def forward(env, c, nE, Ts, **over):
    torch, sensor = env["torch"], env["sensor"]
    tau, La, Ld = (torch.as_tensor(np.array(over.get(k, c[k]), dtype=np.float32), device="cuda") for k in ("tau", "La", "Ld"))
    E = torch.as_tensor(np.array(over.get("E", c["E"][:, :nE]), dtype=np.float32), device="cuda")
    _, L = sensor.band_radiance_srf_fused(full_grid(env), tau, La, Ld, c["Xk"], E, Ts, sensor.Sensor.from_tables(c["tables"]))
    torch.cuda.synchronize()
    return L.cpu().numpy()


def within(got, want, scale, k, dead, what):
    """Over the live bands (axis -2), max |got - want| / (2^-24 scale) against k, elements of scale 0 equal; the dead bands
    NaN. Returns the ratio."""
    got, want, scale = (np.asarray(v, dtype=np.float64) for v in (got, want, scale))
    assert got.shape == want.shape == scale.shape, what
    assert np.isnan(got[..., dead, :]).all(), what + ": a dead band is not NaN"
    got, want, scale = (v[..., ~dead, :] for v in (got, want, scale))
    assert np.all(np.isfinite(got)), what + ": a live band is not finite"
    zero = scale == 0.0
    assert np.array_equal(got[zero], want[zero]), what
    e = float(np.max(np.abs(got - want)[~zero] / (EPS * scale[~zero]))) if (~zero).any() else 0.0
    print("%s: max |got - want| / (2^-24 scale) = %.3g (k = %d)" % (what, e, k))
    assert e <= k, what
    return e


def ts_of(many):
    return list(FC.TS_LIST) if many else FC.TS_SCALAR


# ---------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("vectors", ("one", "max"))
@pytest.mark.parametrize("many", (False, True), ids=("Ts_scalar", "Ts_list"))
@pytest.mark.parametrize("nE", FC.NE_CASES)
@pytest.mark.parametrize("knots", FC.KNOT_SETS)
def test_against_oracle(env, knots, nE, many, vectors):
    """Test 1: dL element by element within k 2^-24 of the oracle's scale; one vector in which all five groups move, and
    the library's maximum of vectors per call, vector v moving SUBSETS[v % 4] (so every vector has its own k). Three
    temperatures are more than one call takes (rtx_srf_radiance_jvp_max_temps() = 2).
    MEASURED on an MI355X, worst over the 18 cases, in units of 2^-24 scale (test_terms_alone has the terms one by one): all
    groups 1.09 (k = 32), (d_tau, d_La) 1.05 (k = 13), (d_Ld, d_Ts) 0.37 (k = 20), d_E 3.15 (k = 32; on_grid knots; 2.25 coarse,
    2.06 dense; 10.0 on the coarse knots before the forward's M took both knot weights from srfm_hats)."""
    c = case(env, knots)
    nv = 1 if vectors == "one" else env["NV"]
    subsets = [SUBSETS[v % len(SUBSETS)] for v in range(nv)]
    per = [JC.case_tangent(env["CH"], env["K"], knots, nE, many, 51 + v, only) for v, only in enumerate(subsets)]
    d = per[0][0] if vectors == "one" else stacked([p[0] for p in per])
    L, dL = run(env, c, nE, ts_of(many), d)
    nT = 3 if many else 1
    assert dL.shape == ((nT,) if many else ()) + (20, nE) + ((nv,) if vectors == "max" else ())
    assert np.array_equal(L, forward(env, c, nE, ts_of(many)), equal_nan=True)
    for v, (only, (_, want, scale)) in enumerate(zip(subsets, per)):
        got = dL[..., v] if vectors == "max" else dL
        within(got.reshape(nT, 20, nE), want, scale, k_of(only), c["dead"],
               "sensor jvp %s nE=%d nT=%d vector %d/%d %s" % (knots, nE, nT, v, nv, "+".join(only)))


@pytest.mark.parametrize("knots", FC.KNOT_SETS)
def test_terms_alone(env, knots):
    """Test 1, term by term: each input group as the only one given (the others NULL: without d_tau and d_Ts no Planck
    evaluation, with d_E alone no pass over the points), against its own k.
    MEASURED on an MI355X, worst over the three knot sets, in units of 2^-24 scale: d_tau 1.19 (k = 13), d_La 0.74 (k = 3),
    d_Ld 0.28 (k = 5), d_Ts 2.31 (k = 20), d_E 1.72 (k = 32)."""
    c = case(env, knots)
    nE = 3
    for g in JC.GROUPS:
        d, want, scale = JC.case_tangent(env["CH"], env["K"], knots, nE, True, 71, (g,))
        assert sum(v is not None for v in d.values()) == 1
        _, dL = run(env, c, nE, ts_of(True), d)
        within(dL, want, scale, K_TERM[g], c["dead"], "sensor jvp %s %s alone" % (knots, g))


def test_exact_values(env):
    """Test 2: dead bands NaN and live bands finite (asserted by every `within`); an all-zero tangent gives exact zeros on
    the live bands; a NULL group gives the bits of that group passed as zeros; a tangent that is non-zero only at points
    under no live band gives exact zeros."""
    c = case(env, "coarse")
    nE, Ts, dead = 3, ts_of(True), c["dead"]
    d = JC.tangents(c, nE, 3, seed=83)
    zeros = {k: np.zeros_like(v) for k, v in d.items()}
    _, z = run(env, c, nE, Ts, zeros)
    assert np.isnan(z[:, dead]).all() and np.all(z[:, ~dead] == 0.0)
    _, full = run(env, c, nE, Ts, d)
    assert np.isnan(full[:, dead]).all() and np.all(np.isfinite(full[:, ~dead])) and np.all(full[:, ~dead] != 0.0)
    for g in JC.GROUPS:
        _, a = run(env, c, nE, Ts, dict(d, **{g: None}))
        _, b = run(env, c, nE, Ts, dict(d, **{g: zeros[g]}))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), g
        assert not np.array_equal(a, full, equal_nan=True), g
    for keep in (("d_E",), ("d_Ts",), ("d_La", "d_E")):  # the paths without a point pass / without Planck / without both Planck and d_tau
        _, a = run(env, c, nE, Ts, {k: (v if k in keep else None) for k, v in d.items()})
        _, b = run(env, c, nE, Ts, {k: (v if k in keep else zeros[k]) for k, v in d.items()})
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), keep
    # bands 0 and 13 cover rows 100 .. 400 and 700 .. 900; 4, 5, 6 are dead: rows that move elsewhere only
    pick = [0, 4, 5, 6, 13]
    X = c["X"]
    under = np.zeros(X.size, dtype=bool)
    for b in (0, 13):
        under |= (X >= c["tables"][b][0][0]) & (X <= c["tables"][b][0][-1])
    assert under.sum() == 301 + 201
    off = {k: (np.where(under, np.float32(0.0), d[k]) if k in ("d_tau", "d_La", "d_Ld") else None) for k in JC.GROUPS}
    assert all(np.count_nonzero(off[k]) > 2000 for k in ("d_tau", "d_La", "d_Ld"))
    _, o = run(env, c, nE, Ts, off, pick=pick)
    assert o.shape == (3, 5, nE) and np.isnan(o[:, 1:4]).all() and np.all(o[:, [0, 4]] == 0.0)


@pytest.mark.parametrize("knots", FC.KNOT_SETS)
def test_adjoint_identity_against_the_shipped_adjoint(env, knots):
    """Test 3: <g, dL> over the live bands against <G_tau, d_tau> + <G_La, d_La> + <G_Ld, d_Ld> + <dTs, d_Ts> + <dE, d_E> with
    the right-hand side from rtx_srf_radiance_vjp (sensor.band_radiance_srf_vjp), both sums in fp64 on the host. Bound: the
    two sides' own, sum |g| (32 2^-24 scale of test 1) + sum |tangent| (K 2^-24 scale of tests/test_gpu_sensor_vjp.py).
    MEASURED on an MI355X: |difference| at most 2.9e-7 against a bound of 1.2e-3."""
    torch, sensor = env["torch"], env["sensor"]
    nE, Ts = 3, ts_of(True)
    c = case(env, knots)
    live = ~c["dead"]
    g = VC.cotangent(3, 20, nE, c["dead"], seed=9)
    d, _, scale = JC.case_tangent(env["CH"], env["K"], knots, nE, True, 51, JC.GROUPS)
    _, dL = run(env, c, nE, Ts, d)
    dev = lambda v: torch.as_tensor(np.array(v, dtype=np.float32), device="cuda")
    adj = sensor.band_radiance_srf_vjp(full_grid(env), dev(c["tau"]), dev(c["La"]), dev(c["Ld"]), c["Xk"], dev(c["E"][:, :nE]), Ts,
                                       sensor.Sensor.from_tables(c["tables"]), dev(g))
    adj = {k: v.cpu().numpy().astype(np.float64) for k, v in adj.items()}
    o = VC.adjoint(c["X"], c["tables"], c["tau"], c["La"], c["Ld"], c["Xk"], c["E"][:, :nE], Ts, g)
    gl = g[:, live].astype(np.float64)
    f64 = lambda v: np.asarray(v).astype(np.float64)
    pairs = (("G_tau", "G_tau", "d_tau", K_ROW["G_tau"]), ("G_La", "G_La", "d_La", K_ROW["G_La"]), ("G_Ld", "G_Ld", "d_Ld", K_ROW["G_Ld"]),
             ("Ts", "dTs", "d_Ts", K_DTS), ("emis", "dE", "d_E", K_DE))
    lhs = float(np.sum(gl * dL[:, live].astype(np.float64)))
    rhs = float(sum(np.sum(adj[a] * f64(d[t])) for a, _, t, _ in pairs))
    bound = 32 * EPS * float(np.sum(np.abs(gl) * scale[:, live]))
    bound += float(sum(k * EPS * np.sum(o["scale"][s] * np.abs(f64(d[t]))) for _, s, t, k in pairs))
    print("sensor jvp adjoint identity %s: %.9g vs %.9g, |diff| = %.3g, bound %.3g" % (knots, lhs, rhs, abs(lhs - rhs), bound))
    assert lhs != 0.0 and abs(lhs - rhs) <= bound


@pytest.mark.parametrize("knots", FC.KNOT_SETS)
def test_linearity_against_the_forward_kernels(env, knots):
    """Test 4, no oracle: L is linear in each of tau, La, Ld and E, so the tangent along d equals L(x + d) - L(x) from
    band_radiance_srf_fused, within the forward's own asserted 1e-5 of the band maximum for each of the two. The step is the
    float32 difference of the two float32 inputs the forward is really given (exact: they lie within a factor 2).
    MEASURED on an MI355X: at most 0.095 of that bound (dense knots, d_E)."""
    nE, Ts = 3, FC.TS_SCALAR
    c = case(env, knots)
    live = ~c["dead"]
    L1 = forward(env, c, nE, Ts).astype(np.float64)
    x = dict(tau=c["tau"], La=c["La"], Ld=c["Ld"], E=c["E"][:, :nE])
    for key, dkey, frac in (("tau", "d_tau", 0.3), ("La", "d_La", 0.2), ("Ld", "d_Ld", 0.2), ("E", "d_E", -0.25)):
        x2 = (x[key] * np.float32(1.0 + frac)).astype(np.float32)
        step = x2 - x[key]
        assert step.dtype == np.float32 and np.array_equal(step.astype(np.float64), x2.astype(np.float64) - x[key].astype(np.float64))
        L2 = forward(env, c, nE, Ts, **{key: x2}).astype(np.float64)
        _, dL = run(env, c, nE, Ts, {k: (step if k == dkey else None) for k in JC.GROUPS})
        bound = TOL_L * (FC.band_max(L1[live]) + FC.band_max(L2[live]))
        err = np.abs(dL[live].astype(np.float64) - (L2[live] - L1[live]))
        print("sensor jvp linearity %s %s: max |dL - (L2 - L1)| / bound = %.3g" % (knots, dkey, np.max(err / bound)))
        assert np.isnan(dL[~live]).all() and np.all(err <= bound) and np.all(dL[live] != 0.0)


@pytest.mark.parametrize("knots", FC.KNOT_SETS)
def test_bit_identity(env, knots):
    """Test 5: the same bits run to run; for a vector alone and among NV + 1 (across the vector-group boundary); for a
    temperature alone, for the temperatures permuted and as a scalar (three temperatures: across the temperature-group
    boundary); for SUBSET's bands alone; and L equal to band_radiance_srf_fused's."""
    nE, NV = 3, env["NV"]
    c = case(env, knots)
    Ts = ts_of(True)
    ds = [JC.tangents(c, nE, 3, seed=90 + v) for v in range(NV + 1)]
    d = stacked(ds)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    L, full = run(env, c, nE, Ts, d)
    L2, again = run(env, c, nE, Ts, d)
    assert full.shape == (3, 20, nE, NV + 1)
    assert np.array_equal(bits(full), bits(again)) and np.array_equal(bits(L), bits(L2))
    assert np.array_equal(bits(L), bits(forward(env, c, nE, Ts)))
    for v in (0, NV - 1, NV):
        _, alone = run(env, c, nE, Ts, ds[v])
        assert alone.shape == (3, 20, nE) and np.array_equal(bits(alone), bits(full[..., v])), v
    sel = lambda dd, t: dict(dd, d_Ts=None if dd["d_Ts"] is None else np.asarray(dd["d_Ts"])[t])
    for t in range(3):
        L1, one = run(env, c, nE, [Ts[t]], sel(d, [t]))
        assert np.array_equal(bits(one[0]), bits(full[t])) and np.array_equal(bits(L1[0]), bits(L[t])), t
        L0, scal = run(env, c, nE, Ts[t], sel(d, [t]))
        assert scal.shape == (20, nE, NV + 1) and np.array_equal(bits(scal), bits(full[t])) and np.array_equal(bits(L0), bits(L[t])), t
    perm = [2, 0, 1]
    Lp, p = run(env, c, nE, [Ts[t] for t in perm], sel(d, perm))
    assert np.array_equal(bits(p), bits(full[perm])) and np.array_equal(bits(Lp), bits(L[perm]))
    pick = list(FC.SUBSET)
    Ls, sub = run(env, c, nE, Ts, d, pick=pick)
    assert np.array_equal(bits(sub), bits(full[:, pick])) and np.array_equal(bits(Ls), bits(L[:, pick]))
    assert np.all(np.isfinite(sub)) and np.all(sub != 0.0)


def test_tangents_that_disagree_are_refused(env):
    """sensor.band_radiance_srf_jvp raises ValueError for tangents that disagree on the vector axis, one of the wrong shape,
    and none at all."""
    c = case(env, "coarse")
    nE = 3
    d = JC.tangents(c, nE, 3, seed=5)
    two = stacked([d, d])
    for bad in (dict(two, d_La=d["d_La"]), dict(d, d_E=two["d_E"]), dict(d, d_Ts=two["d_Ts"]), dict(d, d_tau=d["d_tau"][:-1]),
                {k: None for k in JC.GROUPS}):
        with pytest.raises(ValueError, match="band_radiance_srf_jvp"):
            run(env, c, nE, ts_of(True), bad)


def test_refusals_write_nothing(env):
    """Test 6: a refused call returns non-zero with rtx_last_error set and leaves dL alone; the same arguments, well formed,
    do write."""
    import ctypes as C
    from radtxfr_amd import _lib
    torch, lib, sensor, NV, MT = env["torch"], env["lib"], env["sensor"], env["NV"], env["MT"]
    nx, nk, nE = 300, 6, 2
    grid = env["engine"].Grid(1000.0, 1002.99, nx)
    gr = _lib.make_grid(1000.0, 1002.99, nx)
    tau, La, Ld = (torch.full((nx,), v, dtype=torch.float32, device="cuda") for v in (0.7, 1.0, 2.0))
    rows = [torch.full((NV, nx), v, dtype=torch.float32, device="cuda") for v in (0.1, 0.2, 0.3)]
    Xk = torch.as_tensor(np.linspace(1000.5, 1002.5, nk), device="cuda")
    s = sensor.Sensor.from_tables([(np.array([1000.2, 1000.6, 1001.0, 1001.4]), np.ones(4))])
    kx, kr = s.on_device("cuda")
    Ts = np.linspace(280.0, 320.0, MT + 1)
    N, _, M, jr = sensor.srf_moments(grid, tau, La, Ld, Xk, Ts[:MT], s)
    E = torch.full((nk, nE), 0.9, dtype=torch.float32, device="cuda")
    dE = torch.full((NV, nk, nE), 0.01, dtype=torch.float32, device="cuda")
    dTs = np.ones((NV + 1) * (MT + 1))
    dL = torch.full((NV, MT, 1, nE), 7.0, dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    hp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(start=(0, 4), nT=1, nv=1, Ts_=Ts, dTs_=dTs, nk_=nk, nE_=nE, ld=nx, rows_=rows, tau_=tau, N_=N, M_=M, jr_=jr, E_=E, dE_=dE,
             dL_=dL):
        st_ = np.asarray(start, dtype=np.int32)
        r = [p(v) for v in rows_] if rows_ is not None else [None] * 3
        return lib.rtx_srf_radiance_jvp(C.byref(gr), p(tau_), p(Ld), *r, ld, hp(Ts_), hp(dTs_), nT, p(Xk), nk_, len(start) - 1,
                                        hp(st_), p(kx), p(kr), p(N_), p(M_), p(jr_), p(E_), p(dE_), nE_, nv, p(dL_), st)

    bad_dTs = dTs.copy()
    bad_dTs[0] = np.inf
    for kw in (dict(nT=0), dict(nT=MT + 1), dict(nv=0), dict(nv=NV + 1), dict(start=(0, 1)), dict(start=(0, 3, 1)), dict(nk_=0),
               dict(nE_=0), dict(ld=nx - 1), dict(tau_=None), dict(N_=None), dict(M_=None), dict(jr_=None), dict(E_=None),
               dict(Ts_=np.array([300.0, -1.0]), nT=2), dict(dTs_=bad_dTs), dict(rows_=None, dTs_=None, dE_=None)):
        assert call(**kw) != 0, kw
        assert lib.rtx_last_error()
    assert call(dL_=None) != 0 and lib.rtx_last_error()
    torch.cuda.synchronize()
    assert bool((dL == 7.0).all())
    assert call(nT=MT, nv=NV) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dL).all()) and bool((dL != 7.0).all())


@pytest.mark.parametrize("thin", (1.0, 1e-3), ids=("standard", "thinned"))
def test_compute_band_radiance_jvp_end_to_end(thin):
    """Test 7: rt.compute_band_radiance_jvp on test_compute_band_radiance_vjp_end_to_end's axis and atmosphere (1000 points,
    66 layers, four triangles with one off the axis, 5 knots, nE = 3; standard and x 1e-3 columns), keys ("T", 1, 3,
    "Ts_surface", "emis"), two vectors. dL is sensor.band_radiance_srf_jvp on compute_TUD_jvp's float32 rows, bit for bit; L is
    compute_band_radiance_vjp's; species 3 (no lines) moves nothing; layers= equals the dense call with zeros elsewhere; a
    surface-only call equals the full call with zero atmospheric tangents. <cot, dL> against <grad, tangents> from
    compute_band_radiance_vjp, per vector, within the sum of the two chains' bounds: the sensor tangent's (test 1) and the
    sensor adjoint's (tests/test_gpu_sensor_vjp.py) on the device rows, and, through the stored Jacobian, the TUD tangent's
    (tests/test_gpu_tud_jvp.py, end to end) under |G| and the TUD adjoint's (tests/test_gpu_tud_vjp.py, end to end) under |v|.
    MEASURED on an MI355X: |difference| at most 4.2e-9 against bounds of 4e-6 to 1.1e-5 (the standard columns are opaque, tau = 0:
    the surface is not seen and only the La rows move L)."""
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
    s = sensor.Sensor.from_shape([1000.10, 1000.14, 1000.38, 1003.0], 0.06, "triangle")
    Xk = np.array([999.9, 1000.07, 1000.2, 1000.33, 1000.6])
    nB, nk, nE, n_vec, Ts_s, nL = 4, 5, 3, 2, 296.0, 66
    rng = np.random.default_rng(7)
    E = rng.uniform(0.6, 1.0, (nk, nE)).astype(np.float32)
    atm = {"T": rng.normal(size=(nL, n_vec)), 1: rng.normal(size=(nL, n_vec)) * 30.0 * thin, 3: rng.normal(size=(nL, n_vec)) * 0.1}
    surf = {"Ts_surface": rng.normal(size=n_vec), "emis": (rng.normal(size=(nk, nE, n_vec)) * 0.05).astype(np.float32)}
    tang = dict(atm, **surf)
    X_out, L, dL = rt.compute_band_radiance_jvp(lo, hi, s, Xk, E, Ts_s, tang, **kw)
    assert np.array_equal(X_out, s.centres) and L.shape == (nB, nE) and L.dtype == np.float32
    assert dL.shape == (nB, nE, n_vec) and dL.dtype == np.float64
    assert np.isnan(L[3]).all() and np.isfinite(L[:3]).all() and np.isnan(dL[3]).all() and np.isfinite(dL[:3]).all()
    # the two stages on their own
    X, tau, La, Ld, rows = rt.compute_TUD_jvp(lo, hi, atm, **kw)
    nX = X.size
    assert nX == 1000 and a["Ts"].size == nL
    grid = engine.Grid(lo, hi, nX)
    dev32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float32), device="cuda")
    t_d, a_d, d_d, E_d = dev32(tau), dev32(La), dev32(Ld), dev32(E)
    r32 = {k: rows[k].astype(np.float32) for k in ("tau", "La", "Ld")}
    assert all(np.array_equal(r32[k].astype(np.float64), rows[k]) for k in r32)  # float32 rows, returned as float64
    L2, dL2 = sensor.band_radiance_srf_jvp(grid, t_d, a_d, d_d, Xk, E_d, Ts_s, s, d_tau=dev32(r32["tau"]), d_La=dev32(r32["La"]),
                                           d_Ld=dev32(r32["Ld"]), d_Ts=surf["Ts_surface"], d_emis=dev32(surf["emis"]))
    assert np.array_equal(dL, dL2.double().cpu().numpy(), equal_nan=True)
    # L, and the adjoint's gradients for the identity
    cot = rng.normal(size=(nB, nE, n_vec)).astype(np.float32)
    cot[3, :, 0] = np.nan
    _, L_v, grad = rt.compute_band_radiance_vjp(lo, hi, s, Xk, E, Ts_s, cot, wrt=wrt, **kw)
    assert np.array_equal(L, L_v, equal_nan=True) and np.array_equal(L, L2.cpu().numpy(), equal_nan=True)
    _, _, _, _, J = rt.compute_TUD_jacobian(lo, hi, wrt=wrt, **kw)  # {w: (dtau, dLa, dLd)}, each [nX][nL]
    tables = [(np.asarray(x), np.asarray(r)) for x, r in s.tables]
    live = np.array([True, True, True, False])
    names = ("tau", "La", "Ld")
    for v in range(n_vec):
        adj = {k: t.cpu().numpy().astype(np.float64) for k, t in
               sensor.band_radiance_srf_vjp(grid, t_d, a_d, d_d, Xk, E_d, Ts_s, s, cot[..., v]).items()}
        G = {"tau": adj["G_tau"], "La": adj["G_La"], "Ld": adj["G_Ld"]}
        c64 = cot[live, :, v].astype(np.float64)
        lhs = float(np.sum(c64 * dL[live, :, v]))
        rhs = float(sum(np.sum(grad[w][:, v] * atm[w][:, v]) for w in wrt) + grad["Ts_surface"][v] * surf["Ts_surface"][v]
                    + np.sum(grad["emis"][..., v] * surf["emis"][..., v].astype(np.float64)))
        # the sensor stage's two sides, on the rows the device holds
        d_s = dict(d_tau=r32["tau"][:, v], d_La=r32["La"][:, v], d_Ld=r32["Ld"][:, v], d_Ts=surf["Ts_surface"][v:v + 1],
                   d_E=surf["emis"][..., v])
        _, sc = JC.tangent(X, tables, tau.astype(np.float32), La.astype(np.float32), Ld.astype(np.float32), Xk, E, [Ts_s], **d_s)
        o = VC.adjoint(X, tables, tau.astype(np.float32), La.astype(np.float32), Ld.astype(np.float32), Xk, E, [Ts_s], cot[None, ..., v])
        bound = 32 * EPS * float(np.sum(np.abs(c64) * sc[0][live]))
        for key, skey, k in (("d_tau", "G_tau", K_ROW["G_tau"]), ("d_La", "G_La", K_ROW["G_La"]), ("d_Ld", "G_Ld", K_ROW["G_Ld"]),
                             ("d_Ts", "dTs", K_DTS), ("d_E", "dE", K_DE)):
            bound += k * EPS * float(np.sum(o["scale"][skey] * np.abs(np.asarray(d_s[key]).astype(np.float64))))
        # the TUD stage's two sides, through the stored Jacobian
        v_sum = sum(np.abs(atm[w][:, v]).sum() for w in wrt)
        for i_, name in enumerate(names):
            S_J, want = 0.0, 0.0
            for w in wrt:
                Jw = np.abs(J[w][i_])
                den = np.maximum(np.maximum(Jw, 1e-3 * np.max(Jw, axis=0, keepdims=True)), F32_FLOOR)
                S_J = S_J + den @ np.abs(atm[w][:, v])
                want = want + J[w][i_] @ atm[w][:, v]
            bound += float(np.sum(np.abs(G[name]) * (2.0 * TOL_L * S_J + F32_TINY * v_sum + U32 * np.abs(want))))
        g_sum = sum(np.abs(G[name]).sum() for name in names)
        for w in wrt:
            scale_w = sum(np.abs(G[name]) @ np.abs(J[w][i_]) for i_, name in enumerate(names))  # [nL]
            bound += float(np.sum(np.abs(atm[w][:, v]) * (4.0 * U32 * scale_w + F32_TINY * g_sum)))
        print("band jvp end to end, thin %g vector %d: %.9g vs %.9g, |diff| = %.3g, bound %.3g" % (thin, v, lhs, rhs, abs(lhs - rhs), bound))
        assert lhs != 0.0 and abs(lhs - rhs) <= bound
    if thin < 1.0:
        assert tau.min() > 0.0 and np.count_nonzero(rows["tau"]) > nX and np.all(dL[:3] != 0.0)
    # species 3 has no lines in the table: it moves nothing
    only3 = rt.compute_band_radiance_jvp(lo, hi, s, Xk, E, Ts_s, {3: atm[3]}, **kw)[2]
    assert only3.shape == (nB, nE, n_vec) and np.all(only3[:3] == 0.0) and np.isnan(only3[3]).all()
    # layers=: the layers named move, the others do not; a single vector drops the vector axis
    lay = [65, 3, 8]
    some = rt.compute_band_radiance_jvp(lo, hi, s, Xk, E, Ts_s, dict({w: t[lay, 1] for w, t in atm.items()}, Ts_surface=surf["Ts_surface"][1],
                                                                        emis=surf["emis"][..., 1]), layers=lay, **kw)[2]
    z = {w: np.zeros(nL) for w in wrt}
    for w in wrt:
        z[w][lay] = atm[w][lay, 1]
    dense = rt.compute_band_radiance_jvp(lo, hi, s, Xk, E, Ts_s, dict(z, Ts_surface=surf["Ts_surface"][1], emis=surf["emis"][..., 1]), **kw)[2]
    assert some.shape == (nB, nE) and np.array_equal(some, dense, equal_nan=True)
    # surface keys only: the base state alone, and the bits of the full call with zero atmospheric tangents
    _, L_s, only_s = rt.compute_band_radiance_jvp(lo, hi, s, Xk, E, Ts_s, surf, **kw)
    with_zero = rt.compute_band_radiance_jvp(lo, hi, s, Xk, E, Ts_s, dict({w: np.zeros((nL, n_vec)) for w in wrt}, **surf), **kw)[2]
    assert np.array_equal(L_s, L, equal_nan=True) and np.array_equal(only_s, with_zero, equal_nan=True)
    if thin < 1.0:
        assert np.all(only_s[:3] != 0.0)
