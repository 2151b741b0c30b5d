"""CPU-only checks of the sensor stage's adjoint (rtx_srf_radiance_vjp, rt.compute_band_radiance_vjp): the fp64 oracle of
tests/sensor_vjp_cases.py against the oracle forward srf_fused_cases.direct_form, the C ABI, and the argument checks that
need no device."""
import os
import re

import numpy as np
import pytest

import srf_fused_cases as FC
import sensor_vjp_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH, K = 1024, 1024  # the issue's case(1024, K, knots); K: the library's rtx_srf_max_knots()
NE = 3
TS = (250.0, 301.5)


def _lib_or_build():
    from radtxfr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib


@pytest.mark.parametrize("knots", FC.KNOT_SETS)
def test_oracle_adjoint_against_oracle_forward(knots):
    """tau, La, Ld and E enter L linearly: for a random direction d in each, sum G . d equals sum g . (L(x + d) - L(x))
    over the live bands to 1e-11 of the sums' absolute terms; for Ts, central differences at 1e-3 K agree with dTs to
    1e-6 relative. g is NaN on the dead bands and must not show. This pins the oracle; it needs no kernel."""
    c = FC.case(CH, K, knots)
    X, tables, Xk, live = c["X"], c["tables"], c["Xk"], ~c["dead"]
    x = dict(tau=c["tau"].astype(np.float64), La=c["La"].astype(np.float64), Ld=c["Ld"].astype(np.float64),
             E=c["E"][:, :NE].astype(np.float64))
    g = VC.cotangent(len(TS), len(tables), NE, c["dead"], seed=11)
    assert np.all(np.isnan(g[:, c["dead"]]))
    o = VC.adjoint(X, tables, x["tau"], x["La"], x["Ld"], Xk, x["E"], TS, g)
    for k in ("G_tau", "G_La", "G_Ld", "dTs", "dE"):
        assert np.all(np.isfinite(o[k])) and np.all(o["scale"][k] >= np.abs(o[k]) * (1.0 - 1e-12))
    assert np.array_equal(o["N"] > 0.0, live)
    gl = g[:, live].astype(np.float64)
    fwd = lambda v, Ts=TS: FC.direct_form(X, tables, v["tau"], v["La"], v["Ld"], Xk, v["E"], Ts)[:, live]
    L0 = fwd(x)
    rng = np.random.default_rng(23)
    for key, G in (("tau", o["G_tau"]), ("La", o["G_La"]), ("Ld", o["G_Ld"]), ("E", o["dE"])):
        d = x[key] * rng.uniform(-0.5, 0.5, x[key].shape)
        L1 = fwd(dict(x, **{key: x[key] + d}))
        lhs, rhs = np.sum(G * d), np.sum(gl * (L1 - L0))
        scale = np.sum(np.abs(G * d)) + np.sum(np.abs(gl) * (np.abs(L1) + np.abs(L0)))
        print("oracle adjoint %s d%s: %.17g vs %.17g, |diff| / scale = %.3g" % (knots, key, lhs, rhs, abs(lhs - rhs) / scale))
        assert abs(lhs - rhs) <= 1e-11 * scale
    h = 1e-3
    for t in range(len(TS)):
        Tp, Tm = np.array(TS), np.array(TS)
        Tp[t] += h
        Tm[t] -= h
        fd = np.sum(gl * (fwd(x, Tp) - fwd(x, Tm))) / (2.0 * h)
        print("oracle adjoint %s dTs[%d]: %.12g vs central difference %.12g" % (knots, t, o["dTs"][t], fd))
        assert abs(o["dTs"][t] - fd) <= 1e-6 * o["scale"]["dTs"][t]


def test_abi():
    """rtx_srf_radiance_vjp is in _lib.PROTOTYPES, declared in the header and exported by the built library, with its 21
    arguments pinned; rtx_srf_norms (the denominators alone) likewise."""
    _lib = _lib_or_build()
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "radtxfr_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in (("rtx_srf_radiance_vjp", 21), ("rtx_srf_norms", 7)):
        assert name in _lib.PROTOTYPES
        res, args = _lib.PROTOTYPES[name]
        assert len(args) == nargs
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name + " is not declared in include/radtxfr_hip.h"
        assert len(m.group(1).split(",")) == nargs
        assert getattr(lib, name) is not None


def test_refusals_need_no_device():
    """The library refuses a bad call before it touches a device: every pointer here is NULL or a host address."""
    import ctypes as C
    _lib = _lib_or_build()
    lib = _lib.load()
    g = _lib.make_grid(1000.0, 1002.99, 300)
    Ts = np.array([300.0])
    start = np.array([0, 3], dtype=np.int32)
    one = C.c_void_p(16)  # never dereferenced: the call is refused first
    tsp, sp = Ts.ctypes.data_as(C.c_void_p), start.ctypes.data_as(C.c_void_p)

    def call(grid=C.byref(g), nT=1, nk=4, nB=1, E=one, nE=2, gg=one, outs=(one, one, one, one, one), tau=one):
        return lib.rtx_srf_radiance_vjp(grid, tau, one, one, tsp, nT, one, nk, nB, sp, one, one, E, nE, gg, *outs, None)

    for kw, word in ((dict(grid=None), b"grid"), (dict(nT=0), b"nT"), (dict(nT=lib.rtx_srf_moments_max_temps() + 1), b"nT"),
                     (dict(nk=0), b"nk"), (dict(nE=0), b"nE"), (dict(E=None), b"NULL"), (dict(gg=None), b"NULL"),
                     (dict(tau=None), b"NULL"), (dict(nB=-1), b"negative"), (dict(outs=(None,) * 5), b"no output")):
        assert call(**kw) != 0, kw
        assert word in lib.rtx_last_error(), (kw, lib.rtx_last_error())
    bad = np.array([0, 1], dtype=np.int32)  # a one-knot band
    assert lib.rtx_srf_radiance_vjp(C.byref(g), one, one, one, tsp, 1, one, 4, 1, bad.ctypes.data_as(C.c_void_p), one, one, one, 2, one,
                                    one, one, one, one, one, None) != 0
    assert b"knots" in lib.rtx_last_error()


def test_argument_checks_of_compute_band_radiance_vjp():
    """Two altitudes, returnOD=True, xs_lut=, reduce= and a cotangent of the wrong shape are refused by name before any
    device work (this machine has no device to touch)."""
    from radtxfr_amd import radiative_transfer as rt
    from radtxfr_amd import sensor
    s = sensor.Sensor.from_shape([1000.1, 1000.3], 0.1, "triangle")
    Xk = np.linspace(1000.0, 1000.5, 5)
    E = np.full((5, 3), 0.9, dtype=np.float32)
    g = np.ones((2, 3), dtype=np.float32)
    kw = dict(DVOUT=0.0005, Altitudes=np.array([8.0]))
    call = lambda cot=g, Ts=300.0, **k: rt.compute_band_radiance_vjp(1000.0, 1000.5, s, Xk, E, Ts, cot, **dict(kw, **k))
    for exc, k in ((NotImplementedError, dict(Altitudes=np.array([0.5, 8.0]))), (NotImplementedError, dict(returnOD=True)),
                   (NotImplementedError, dict(xs_lut=object())), (NotImplementedError, dict(reduce=dict(dX=1.0))),
                   (NotImplementedError, dict(theta_r=np.array([0.0, 0.3]))), (NotImplementedError, dict(broadening="self")),
                   (ValueError, dict(wrt=("T", 99))), (ValueError, dict(cot=np.ones((3, 3), dtype=np.float32))),
                   (ValueError, dict(cot=np.ones((2, 2, 3), dtype=np.float32))),
                   (ValueError, dict(cot=np.ones((2, 3), dtype=np.float32), Ts=[300.0, 310.0])), (ValueError, dict(Ts=-1.0))):
        with pytest.raises(exc, match="compute_band_radiance_vjp"):
            call(**k)
    with pytest.raises(ValueError, match="compute_band_radiance_vjp"):
        rt.compute_band_radiance_vjp(1000.0, 1000.5, s, Xk, E[:4], 300.0, g, **kw)
