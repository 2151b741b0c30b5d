"""CPU-only checks of the sensor stage's tangent (rtx_srf_radiance_jvp, rt.compute_band_radiance_jvp): the fp64 oracle of
tests/sensor_jvp_cases.py against the oracle forward srf_fused_cases.direct_form and the oracle adjoint
sensor_vjp_cases.adjoint, the C ABI, and the argument checks that need no device."""
import os
import re

import numpy as np
import pytest

import srf_fused_cases as FC
import sensor_vjp_cases as VC
import sensor_jvp_cases as JC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH, K = 1024, 1024  # the issue's case(1024, K, knots); K: the library's rtx_srf_max_knots()
NE = 3
TS = FC.TS_LIST


def _lib_or_build():
    from radtxfr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib


def _inputs(c):
    return dict(tau=c["tau"].astype(np.float64), La=c["La"].astype(np.float64), Ld=c["Ld"].astype(np.float64),
                E=c["E"][:, :NE].astype(np.float64))


@pytest.mark.parametrize("knots", FC.KNOT_SETS)
def test_oracle_tangent_against_central_difference(knots):
    """dL against (L(x + h d) - L(x - h d)) / 2h of direct_form, all five groups moving at once, three temperatures.
    Bound, from the step: the tangents are at most r = 1/2 of the inputs they belong to, and L's highest term tau eps B is
    trilinear in (tau, E, B(Ts)), so |d^3 L / ds^3| <= 6 r^3 |L| (Planck's own third derivative along d_Ts <= 2 K is
    (2 u / T)^3 B < 1e-4 B and does not count); the central difference is off by h^2 / 6 of that, h^2 r^3 |L| = 1.25e-9 |L|
    at h = 1e-4, and by rounding 2^-52 |L| / h = 2.3e-12 |L|. Asserted: 2e-9 of the band's largest |L|.
    MEASURED on the CPU: coarse 5.3e-11, dense 6.8e-11, on_grid 2.8e-11 of the band's largest |L| (1.0e-10, 1.2e-10 and
    5.2e-11 of the largest |dL|)."""
    c = FC.case(CH, K, knots)
    X, tables, Xk, live = c["X"], c["tables"], c["Xk"], ~c["dead"]
    x = _inputs(c)
    d = {k: v.astype(np.float64) for k, v in JC.tangents(c, NE, len(TS), seed=31).items()}  # h d is formed in fp64
    dL, scale = JC.tangent(X, tables, x["tau"], x["La"], x["Ld"], Xk, x["E"], TS, **d)
    assert np.isnan(dL[:, c["dead"]]).all() and np.isfinite(dL[:, live]).all()
    assert np.all(scale[:, live] >= np.abs(dL[:, live]) * (1.0 - 1e-12))
    h = 1e-4
    fwd = lambda s: FC.direct_form(X, tables, x["tau"] + s * d["d_tau"], x["La"] + s * d["d_La"], x["Ld"] + s * d["d_Ld"], Xk,
                                   x["E"] + s * d["d_E"], np.array(TS) + s * d["d_Ts"])[:, live]
    Lp, Lm = fwd(h), fwd(-h)
    fd = (Lp - Lm) / (2.0 * h)
    err = np.max(np.abs(fd - dL[:, live]) / FC.band_max(0.5 * (Lp + Lm)))
    print("oracle tangent %s: max |fd - dL| / band max |L| = %.3g, / max |dL| = %.3g"
          % (knots, err, np.max(np.abs(fd - dL[:, live])) / np.max(np.abs(dL[:, live]))))
    assert err <= 2e-9


@pytest.mark.parametrize("knots", FC.KNOT_SETS)
def test_oracle_tangent_against_oracle_adjoint(knots):
    """<g, dL> over the live bands equals <G_tau, d_tau> + <G_La, d_La> + <G_Ld, d_Ld> + <dTs, d_Ts> + <dE, d_E> with the
    right-hand side from sensor_vjp_cases.adjoint, to 1e-12 of the two sides' absolute terms."""
    c = FC.case(CH, K, knots)
    X, tables, Xk, live = c["X"], c["tables"], c["Xk"], ~c["dead"]
    x = _inputs(c)
    g = VC.cotangent(len(TS), len(tables), NE, c["dead"], seed=11)
    o = VC.adjoint(X, tables, x["tau"], x["La"], x["Ld"], Xk, x["E"], TS, g)
    d = JC.tangents(c, NE, len(TS), seed=37)
    dL, _ = JC.tangent(X, tables, x["tau"], x["La"], x["Ld"], Xk, x["E"], TS, **d)
    gl = g[:, live].astype(np.float64)
    pairs = ((o["G_tau"], d["d_tau"]), (o["G_La"], d["d_La"]), (o["G_Ld"], d["d_Ld"]), (o["dTs"], d["d_Ts"]), (o["dE"], d["d_E"]))
    lhs = np.sum(gl * dL[:, live])
    rhs = sum(np.sum(G * v.astype(np.float64)) for G, v in pairs)
    scale = np.sum(np.abs(gl * dL[:, live])) + sum(np.sum(np.abs(G * v.astype(np.float64))) for G, v in pairs)
    print("oracle tangent/adjoint %s: %.17g vs %.17g, |diff| / scale = %.3g" % (knots, lhs, rhs, abs(lhs - rhs) / scale))
    assert abs(lhs - rhs) <= 1e-12 * scale


def test_abi():
    """rtx_srf_radiance_jvp and its two limit queries are in _lib.PROTOTYPES, declared in the header and exported by the
    built library, with the 25 arguments pinned."""
    _lib = _lib_or_build()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "radtxfr_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in (("rtx_srf_radiance_jvp", 25), ("rtx_srf_radiance_jvp_max_vectors", 0), ("rtx_srf_radiance_jvp_max_temps", 0)):
        assert name in _lib.PROTOTYPES
        assert len(_lib.PROTOTYPES[name][1]) == nargs
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name + " is not declared in include/radtxfr_hip.h"
        assert (len(m.group(1).split(",")) if nargs else m.group(1).strip() == "void")
        assert nargs == 0 or len(m.group(1).split(",")) == nargs
        assert getattr(lib, name) is not None
    assert 1 <= lib.rtx_srf_radiance_jvp_max_temps() <= lib.rtx_srf_moments_max_temps()
    assert lib.rtx_srf_radiance_jvp_max_vectors() >= 1


def test_refusals_need_no_device():
    """The library refuses a bad call before it touches a device: every pointer here is NULL or a host address."""
    import ctypes as C
    _lib = _lib_or_build()
    lib = _lib.load()
    g = _lib.make_grid(1000.0, 1002.99, 300)
    NV, MT = lib.rtx_srf_radiance_jvp_max_vectors(), lib.rtx_srf_radiance_jvp_max_temps()
    Ts = np.full(MT + 1, 300.0)
    dTs = np.ones((NV + 1) * (MT + 1))
    start = np.array([0, 3], dtype=np.int32)
    one = C.c_void_p(16)  # never dereferenced: the call is refused first
    hp = lambda v: v.ctypes.data_as(C.c_void_p)

    def call(grid=C.byref(g), tau=one, rows=(one, one, one), ld=300, Ts_=Ts, dTs_=dTs, nT=1, nk=4, nB=1, start_=start, N=one, M=one,
             jr=one, E=one, dE=one, nE=2, nv=1, dL=one):
        return lib.rtx_srf_radiance_jvp(grid, tau, one, *rows, ld, hp(Ts_), None if dTs_ is None else hp(dTs_), nT, one, nk, nB,
                                        hp(start_), one, one, N, M, jr, E, dE, nE, nv, dL, None)

    nan = dTs.copy()
    nan[1] = np.nan
    for kw, word in ((dict(grid=None), b"grid"), (dict(nT=0), b"nT"), (dict(nT=MT + 1), b"nT"), (dict(nv=0), b"n_vec"),
                     (dict(nv=NV + 1), b"n_vec"), (dict(nk=0), b"nk"), (dict(nE=0), b"nE"), (dict(nB=-1), b"negative"),
                     (dict(rows=(None, None, None), dTs_=None, dE=None), b"no tangent"), (dict(ld=299), b"ld_d"),
                     (dict(tau=None), b"NULL"), (dict(N=None), b"NULL"), (dict(M=None), b"NULL"), (dict(jr=None), b"NULL"),
                     (dict(E=None), b"NULL"), (dict(dL=None), b"NULL"), (dict(dTs_=nan, nv=2), b"finite"),
                     (dict(Ts_=np.array([-1.0])), b"temperature"), (dict(start_=np.array([0, 1], dtype=np.int32)), b"knots")):
        assert call(**kw) != 0, kw
        assert word in lib.rtx_last_error(), (kw, lib.rtx_last_error())
    assert call(nB=0) == 0  # no band: nothing to write


def test_argument_checks_of_compute_band_radiance_jvp():
    """Two altitudes, returnOD=True, xs_lut=, reduce=, two slant paths, broadening=, an unknown key and tangents of the wrong
    shape or with different vector axes are refused by name before any device work (this machine has no device to touch)."""
    from radtxfr_amd import radiative_transfer as rt
    from radtxfr_amd import sensor
    s = sensor.Sensor.from_shape([1000.1, 1000.3], 0.1, "triangle")
    Xk = np.linspace(1000.0, 1000.5, 5)
    E = np.full((5, 3), 0.9, dtype=np.float32)
    nL = np.asarray(rt.options["Ts"]).size
    good = {"T": np.ones(nL), "Ts_surface": 1.0, "emis": np.ones((5, 3))}
    kw = dict(DVOUT=0.0005, Altitudes=np.array([8.0]))
    call = lambda tan=good, Ts=300.0, **k: rt.compute_band_radiance_jvp(1000.0, 1000.5, s, Xk, E, Ts, tan, **dict(kw, **k))
    for exc, k in ((NotImplementedError, dict(Altitudes=np.array([0.5, 8.0]))), (NotImplementedError, dict(returnOD=True)),
                   (NotImplementedError, dict(xs_lut=object())), (NotImplementedError, dict(reduce=dict(dX=1.0))),
                   (NotImplementedError, dict(theta_r=np.array([0.0, 0.3]))), (NotImplementedError, dict(broadening="self")),
                   (ValueError, dict(tan={})), (ValueError, dict(tan=None)), (ValueError, dict(tan={"P": np.ones(nL)})),
                   (ValueError, dict(tan={99: np.ones(nL)})), (ValueError, dict(tan={"T": np.ones(nL + 1)})),
                   (ValueError, dict(tan={"T": np.ones(3)}, layers=[0, 1])), (ValueError, dict(tan={"T": np.ones(nL)}, dT_method="x")),
                   (ValueError, dict(tan={"T": np.ones(nL)}, fd_step_T=0.0)),
                   (ValueError, dict(tan={"Ts_surface": np.ones((2, 2))})), (ValueError, dict(tan={"Ts_surface": np.nan})),
                   (ValueError, dict(tan={"Ts_surface": 1.0}, Ts=[300.0, 310.0])),
                   (ValueError, dict(tan={"emis": np.ones((4, 3))})), (ValueError, dict(tan={"emis": np.ones((5, 3, 2, 2))})),
                   (ValueError, dict(tan={"T": np.ones((nL, 2)), "emis": np.ones((5, 3))})),
                   (ValueError, dict(tan={"Ts_surface": np.ones(3), "emis": np.ones((5, 3, 2))})),
                   (ValueError, dict(Ts=-1.0))):
        with pytest.raises(exc, match="compute_band_radiance_jvp"):
            call(**k)
    with pytest.raises(ValueError, match="compute_band_radiance_jvp"):
        rt.compute_band_radiance_jvp(1000.0, 1000.5, s, Xk, E[:4], 300.0, good, **kw)
