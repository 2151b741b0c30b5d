"""CPU-only checks of the per-pixel fit to a measured HSI cube (include/radtxfr_hip.h: rtx_srf_pixel_cube_normal,
rtx_srf_pixel_cube_fit; sensor.hsi_cube_srf_normal / hsi_cube_srf_fit, rt.compute_hsi_cube_fit): the fp64 oracle of
tests/srf_cube_fit_cases.py against central differences of srf_cube_cases.node_cube, the convergence of the fp64
restatement of the fit from the scan start to within the sensitivity bound, the new ABI entries with the refusals they make
before any launch, and the argument checks of the three Python entries that need no device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from radtxfr_amd import _lib, engine, sensor
from radtxfr_amd import radiative_transfer as rt

import srf_cube_cases as CC
import srf_cube_fit_cases as FT
import srf_fused_cases as FC

STEP = 1e-6   # step of the central differences, relative to max(|u_i|, 1)
AGREE = 1e-7  # of the oracle's own scale (the sum of the absolute values of the summands)


def _case(knots):
    lib = _lib.load()
    return FC.case(lib.rtx_srf_chunk_points(), lib.rtx_srf_max_knots(), knots)


def _setup(knots, sname, tname):
    """The fp64 moments of a case, its table G [Q][nB][nEnd], a scene with distinct endmembers and its node form."""
    c = _case(knots)
    nMix, nEnd = FT.SCENES[sname]
    T_range, Q = CC.T_CONFIGS[tname]
    End = CC.endmembers(c["Xk"].size, nEnd)
    sc = FT.distinct_scene(FT.NPIX, nMix, nEnd, T_range)
    Tq = CC.nodes(T_range, Q)
    N, Cb, M, _ = CC.node_moments(c, knots, tname)
    G = M @ End.astype(np.float64)
    return c, sc, Tq, T_range, N, Cb, M, End, G


def _away(sc, T_range, seed=19):
    """A start away from the truth: T moved by up to a quarter of the range (kept inside), the fractions by up to 0.2."""
    r = np.random.default_rng(seed)
    T = np.clip(sc["T"] + r.uniform(-0.25, 0.25, sc["T"].size) * (T_range[1] - T_range[0]), *T_range)
    f = (sc["frac"] + r.uniform(-0.2, 0.2, sc["frac"].shape)).astype(np.float32)
    return T, f


@pytest.mark.parametrize("tname", list(CC.T_CONFIGS))
@pytest.mark.parametrize("sname", ("mix3_of_8", "mix4_of_31"))
def test_oracle_against_central_differences(sname, tname):
    """grad against central differences of 1/2 cost built from CC.node_cube, H against J^T W J with J from central differences
    of node_cube, at a start away from the truth, with weights of which one is zero: within 1e-7 of the oracle's own scale.
    MEASURED (fp64 NumPy), worst of the 4 cases: grad 2.4e-11, H 2.5e-10 of the scale."""
    c, sc, Tq, T_range, N, Cb, M, End, G = _setup("coarse", sname, tname)
    cnt = ~c["dead"]
    w = np.random.default_rng(3).uniform(0.5, 2.0, N.size)
    w[4] = 0.0
    cnt = cnt & (w > 0.0)
    meas = CC.node_cube(N, Cb, M, End, sc, Tq).astype(np.float32)
    meas[c["dead"]] = np.nan
    T, f = _away(sc, T_range)
    o = FT.evaluate(N, Cb, G, Tq, sc["kidx"], f, T, meas, w)
    nU = f.shape[1] + 1
    u = np.concatenate([T[:, None], f.astype(np.float64)], axis=1)

    def cube(u_):
        return CC.node_cube(N, Cb, M, End, dict(kidx=sc["kidx"], frac=u_[:, 1:], T=u_[:, 0]), Tq)[cnt]

    def half_cost(u_):
        return 0.5 * np.sum(w[cnt][:, None] * (cube(u_) - meas[cnt].astype(np.float64)) ** 2, axis=0)
    e_g = 0.0
    Jfd = np.zeros((nU, int(cnt.sum()), T.size))
    for i in range(nU):
        h = np.zeros_like(u)
        h[:, i] = STEP * np.maximum(np.abs(u[:, i]), 1.0)  # a fraction near 0 still takes a step of 1e-6
        fd = (half_cost(u + h) - half_cost(u - h)) / (2 * h[:, i])
        e_g = max(e_g, float(np.max(np.abs(fd - o["grad"][:, i]) / o["scale"]["grad"][:, i])))
        Jfd[i] = (cube(u + h) - cube(u - h)) / (2 * h[:, i])[None, :]
    e_H = 0.0
    for i in range(nU):
        for j in range(i + 1):
            Hfd = np.sum(w[cnt][:, None] * Jfd[i] * Jfd[j], axis=0)
            e_H = max(e_H, float(np.max(np.abs(Hfd - o["hess"][:, FT.tri(i, j)]) / o["scale"]["hess"][:, FT.tri(i, j)])))
    cost = 2.0 * half_cost(u)
    print("srf cube fit oracle vs central differences %s %s: grad %.3g, H %.3g of the scale" % (sname, tname, e_g, e_H))
    assert np.allclose(cost, o["cost"], rtol=1e-12, atol=0.0) and np.all(np.isfinite(o["cost"]))
    assert max(e_g, e_H) <= AGREE


def test_solve_against_numpy():
    """The restated Cholesky step against np.linalg.solve on (H + lam diag H), and a matrix that is not positive definite."""
    c, sc, Tq, T_range, N, Cb, M, End, G = _setup("coarse", "mix3_of_8", "230-350_Q8")
    meas = CC.node_cube(N, Cb, M, End, sc, Tq).astype(np.float32)
    T, f = _away(sc, T_range)
    o = FT.evaluate(N, Cb, G, Tq, sc["kidx"], f, T, np.nan_to_num(meas))
    lam = np.random.default_rng(5).uniform(0.0, 1.0, T.size)
    d, ok = FT.solve(o["hess"], o["grad"], lam)
    A = FT.unpack(o["hess"])
    A = A + lam[:, None, None] * A * np.eye(A.shape[1])[None]
    want = np.linalg.solve(A, -o["grad"][:, :, None])[:, :, 0]
    err = np.max(np.abs(d - want) / np.max(np.abs(want), axis=1, keepdims=True))
    print("srf cube fit restated step vs np.linalg.solve: %.3g relative, condition up to %.3g" % (err, FT.jacobi_condition(o["hess"]).max()))
    assert ok.all() and err <= 1e-6  # both are backward stable: eps x the condition number (at most a few 1e6)
    Hbad = o["hess"].copy()
    Hbad[0, FT.tri(1, 1)] = -1.0
    d, ok = FT.solve(Hbad, o["grad"], 0.0)
    assert not ok[0] and np.isnan(d[0]).all() and ok[1:].all()


@pytest.mark.parametrize("tname", list(CC.T_CONFIGS))
@pytest.mark.parametrize("sname", list(FT.SCENES))
@pytest.mark.parametrize("knots", CC.KNOTS)
def test_restatement_converges_from_the_scan(knots, sname, tname):
    """257 pixels, the measurement = the node form rounded to float32, the scan start, 40 trials: |T - T_true| and
    |f - f_true| within the sensitivity bound for every pixel, in fp64 and with the kernel's fp32 roundings simulated; the
    cost never above the start's.
    MEASURED, worst of the 12 cases: 0.0040 of the bound in fp64, 0.0060 with fp32 simulated; worst |dT| 5.4e-4 K (the
    largest bound on T per case 0.035 .. 0.19 K); Jacobi-scaled condition numbers 9e3 .. 3.5e6."""
    c, sc, Tq, T_range, N, Cb, M, End, G = _setup(knots, sname, tname)
    meas = CC.node_cube(N, Cb, M, End, sc, Tq).astype(np.float32)
    assert np.isnan(meas[c["dead"]]).all()
    bound = FT.sensitivity_bound(N, Cb, G, Tq, sc)
    truth = np.concatenate([sc["T"][:, None], sc["frac"].astype(np.float64)], axis=1)
    for f32 in (False, True):
        r = FT.fit(N, Cb, G, Tq, T_range, sc["kidx"], meas, f32=f32)
        got = np.concatenate([r["T"][:, None], r["frac"].astype(np.float64)], axis=1)
        ratio = np.abs(got - truth) / bound
        print("srf cube fit restatement %s %s %s fp32=%d: worst ratio %.3g, worst |dT| %.3g K, bound on T %.3g .. %.3g K, cond %.3g, statuses %r"
              % (knots, sname, tname, f32, ratio.max(), np.abs(got[:, 0] - truth[:, 0]).max(), bound[:, 0].min(), bound[:, 0].max(),
                 FT.jacobi_condition(r["hess"]).max(), np.unique(r["status"]).tolist()))
        assert np.all(r["status"] <= 1) and np.all(r["n_iter"] <= FT.TRIALS)
        assert np.all(r["cost"] <= r["cost0"])
        assert np.all(ratio <= 1.0)


# ------------------------------------------------------------------------------------------ the entries' refusals
def _stub(fn, **kw):
    """hsi_cube_srf_normal / hsi_cube_srf_fit on host tensors: every check runs before any device work."""
    nk, nEnd, nPix, nMix = 5, 6, 4, 2
    z = torch.zeros(FC.axis(1024).size, dtype=torch.float32)
    args = dict(endmembers=torch.zeros((nk, nEnd), dtype=torch.float32), kidx=torch.zeros((nPix, nMix), dtype=torch.int32),
                frac=torch.zeros((nPix, nMix), dtype=torch.float32), Tpix=torch.full((nPix,), 300.0, dtype=torch.float64),
                meas=torch.zeros((2, nPix), dtype=torch.float32))
    opts = dict(n_nodes=8, T_range=(230.0, 350.0))
    for k, v in kw.items():
        (args if k in args else opts)[k] = v
    s = sensor.Sensor.from_shape([910.0, 920.0], 4.0, "boxcar")
    grid, Xk = engine.Grid(*FC.grid_tuple(1024)), np.linspace(905.0, 925.0, nk)
    if fn == "normal":
        return sensor.hsi_cube_srf_normal(grid, z, z, z, Xk, args["endmembers"], args["kidx"], args["frac"], args["Tpix"], s, args["meas"], **opts)
    T_range = opts.pop("T_range")
    return sensor.hsi_cube_srf_fit(grid, z, z, z, Xk, args["endmembers"], args["kidx"], args["meas"], s, T_range, **opts)


def test_argument_checks_of_hsi_cube_srf_normal():
    for kw, text in ((dict(outputs=("cost", "jac")), "outputs"), (dict(outputs=()), "outputs"), (dict(n_nodes=0), "n_nodes"),
                     (dict(T_range=(350.0, 230.0)), "T_range"), (dict(kidx=torch.zeros((4, 2), dtype=torch.int64)), "kidx"),
                     (dict(frac=torch.zeros((4, 3), dtype=torch.float32)), "frac"), (dict(Tpix=torch.zeros(4, dtype=torch.float32)), "Tpix"),
                     (dict(n_nodes=4), "narrow T_range"), (dict(T_range=None), "device tensors"), (dict(), "device tensors")):
        with pytest.raises(ValueError, match=text):
            _stub("normal", **kw)
    # the fit's own arguments are checked on a scene that passes the shared checks only on a device: kidx of 5 slots is refused first
    five = dict(kidx=torch.zeros((4, 5), dtype=torch.int32), frac=torch.zeros((4, 5), dtype=torch.float32))
    with pytest.raises(ValueError, match="device tensors"):
        _stub("normal", **five)


def test_argument_checks_of_hsi_cube_srf_fit():
    """T_range required, the start both or neither, max_iter / lambda0 / ftol, nMix against the library's, meas and weights:
    all before any device work (the stub tensors are host tensors, which is the last thing refused)."""
    f0, T0 = torch.zeros((4, 2), dtype=torch.float32), torch.full((4,), 300.0, dtype=torch.float64)
    for kw, text in ((dict(T_range=None), "T_range"), (dict(frac0=f0), "frac0 and T0"), (dict(T0=T0), "frac0 and T0"),
                     (dict(max_iter=-1), "max_iter"), (dict(max_iter=1001), "max_iter"), (dict(max_iter=2.5), "max_iter"),
                     (dict(lambda0=-1.0), "lambda0"), (dict(lambda0=np.inf), "lambda0"), (dict(ftol=np.nan), "ftol"), (dict(ftol=-1e-3), "ftol"),
                     (dict(n_nodes=9), "n_nodes"), (dict(n_nodes=4), "narrow T_range"), (dict(T_range=(350.0, 230.0)), "T_range"),
                     (dict(kidx=torch.zeros((4, 2), dtype=torch.int64)), "kidx"), (dict(kidx=torch.zeros((4, 5), dtype=torch.int32)), "nMix=5"),
                     (dict(frac0=torch.zeros((4, 3), dtype=torch.float32), T0=T0), "frac"),
                     (dict(frac0=f0, T0=torch.zeros(4, dtype=torch.float32)), "Tpix"),
                     (dict(meas=torch.zeros((3, 4), dtype=torch.float32)), "meas"), (dict(meas=torch.zeros((2, 4), dtype=torch.float64)), "meas"),
                     (dict(meas=np.zeros((2, 4), dtype=np.float32)), "meas"), (dict(weights=np.ones(3)), "weights"),
                     (dict(weights=torch.ones(2, dtype=torch.int32)), "weights"), (dict(), "device tensors"),
                     (dict(frac0=f0, T0=T0), "device tensors"), (dict(weights=np.ones(2)), "device tensors")):
        with pytest.raises(ValueError, match=text):
            _stub("fit", **kw)


def test_argument_checks_of_compute_hsi_cube_fit():
    """compute_TUD's restrictions for a single view, the scene, the measurement and the fit's own arguments: before any
    device work (this machine has no device to touch)."""
    s = sensor.Sensor.from_shape([1000.1, 1000.3], 0.1, "triangle")
    Xk = np.linspace(1000.0, 1000.5, 5)
    nPix, nMix = 6, 2
    base = dict(End=np.full((5, 3), 0.9, dtype=np.float32), kidx=np.zeros((nPix, nMix), dtype=np.int32), meas=np.ones((2, nPix), dtype=np.float32),
                T_range=(290.0, 310.0))
    kw = dict(DVOUT=0.0005, Altitudes=np.array([8.0]))

    def call(**k):
        a = dict(base)
        a.update({n: k.pop(n) for n in list(k) if n in a})
        return rt.compute_hsi_cube_fit(1000.0, 1000.5, s, Xk, a["End"], a["kidx"], a["meas"], a["T_range"], **dict(kw, **k))

    for k in (dict(Altitudes=np.array([0.5, 8.0])), dict(returnOD=True), dict(theta_r=np.array([0.0, 0.3]))):
        with pytest.raises(NotImplementedError, match="compute_hsi_cube_fit"):
            call(**k)
    for k, text in ((dict(T_range=None), "T_range"), (dict(frac0=np.zeros((nPix, nMix), dtype=np.float32)), "frac0 and T0"),
                    (dict(max_iter=1001), "max_iter"), (dict(lambda0=-1.0), "lambda0"), (dict(ftol=np.inf), "ftol"),
                    (dict(kidx=np.zeros((nPix, nMix))), "kidx has dtype"), (dict(kidx=np.zeros(nPix, dtype=np.int32)), "kidx"),
                    (dict(kidx=np.zeros((nPix, 5), dtype=np.int32)), "nMix=5"), (dict(End=np.full((4, 3), 0.9, dtype=np.float32)), "endmembers"),
                    (dict(meas=np.ones((3, nPix), dtype=np.float32)), "meas"), (dict(meas=np.ones((2, nPix + 1), dtype=np.float32)), "meas"),
                    (dict(frac0=np.zeros((nPix, 3), dtype=np.float32), T0=np.full(nPix, 300.0)), "frac"),
                    (dict(frac0=np.zeros((nPix, nMix), dtype=np.float32), T0=np.full(nPix + 1, 300.0)), "Tpix"),
                    (dict(weights=np.ones(3)), "weights"), (dict(n_nodes=9), "n_nodes"), (dict(n_nodes=2, T_range=(230.0, 350.0)), "narrow T_range"),
                    (dict(T_range=(310.0, 290.0)), "T_range")):
        with pytest.raises(ValueError, match=text):
            call(**k)


def test_abi_symbols_and_refusals():
    """The four new symbols are in PROTOTYPES, declared in the header and exported, with 21 and 23 arguments; max_mix >= 4,
    max_iter = 1000; what the two entries refuse, they refuse before anything touches a device (the pointers are host
    memory, never read there), and nB == 0 / nPix == 0 return 0."""
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "radtxfr_hip.h")).read()
    for name, n in (("rtx_srf_pixel_cube_normal", 21), ("rtx_srf_pixel_cube_fit", 23), ("rtx_srf_pixel_cube_fit_max_mix", 0),
                    ("rtx_srf_pixel_cube_fit_max_iter", 0)):
        assert name in _lib.PROTOTYPES and ("int %s(" % name) in header and hasattr(lib, name)
        decl = header.split("int %s(" % name)[1].split(");")[0]
        assert len(_lib.PROTOTYPES[name][1]) == (decl.count(",") + 1 if n else 0) == n
    assert "#define RTX_FIT_START_GIVEN 1u" in header and sensor.RTX_FIT_START_GIVEN == 1
    MM, IM = lib.rtx_srf_pixel_cube_fit_max_mix(), lib.rtx_srf_pixel_cube_fit_max_iter()
    assert MM >= 4 and IM == 1000
    assert hasattr(sensor, "hsi_cube_srf_normal") and hasattr(sensor, "hsi_cube_srf_fit") and hasattr(rt, "compute_hsi_cube_fit")
    QM = lib.rtx_srf_cube_max_nodes()
    buf = np.zeros(64)
    p = C.c_void_p(buf.ctypes.data)
    good = np.array([310.0, 290.0, 285.0, 315.0])  # two nodes, then the range
    th = lambda T: None if T is None else np.ascontiguousarray(T, dtype=np.float64)

    def normal(nB=2, Q=2, T=good, N=p, Cb=p, tab=p, nEnd=3, nPix=4, nMix=2, kidx=p, frac=p, Tpix=p, meas=p, cost=p, flags=0):
        T = th(T)
        return lib.rtx_srf_pixel_cube_normal(nB, Q, None if T is None else T.ctypes.data_as(C.c_void_p), N, Cb, tab, nEnd, nPix, nMix, kidx, frac,
                                             Tpix, meas, None, None, cost, p, p, p, None, flags)

    def fit(nB=2, Q=2, T=good, N=p, Cb=p, tab=p, nEnd=3, nPix=4, nMix=2, kidx=p, meas=p, frac=p, Tpix=p, max_iter=5, lambda0=1e-3, ftol=0.0,
            cost=p, n_iter=p, status=p, flags=0):
        T = th(T)
        return lib.rtx_srf_pixel_cube_fit(nB, Q, None if T is None else T.ctypes.data_as(C.c_void_p), N, Cb, tab, nEnd, nPix, nMix, kidx, meas, None,
                                          frac, Tpix, max_iter, lambda0, ftol, cost, n_iter, status, None, None, flags)

    shared = [("Q=", dict(Q=0)), ("Q=", dict(Q=QM + 1, T=np.linspace(300.0, 310.0, QM + 3))), ("negative", dict(nB=-1)), ("negative", dict(nPix=-1)),
              ("nEnd=", dict(nEnd=0)), ("nMix=", dict(nMix=0)), ("max_mix", dict(nMix=MM + 1)), ("NULL", dict(T=None)), ("NULL", dict(meas=None)),
              ("NULL", dict(cost=None)), ("NULL", dict(meas=None, nPix=0)), ("NULL", dict(N=None)), ("NULL", dict(Cb=None)), ("NULL", dict(tab=None)),
              ("NULL", dict(kidx=None)), ("NULL", dict(frac=None)), ("NULL", dict(Tpix=None)),
              ("node temperature", dict(T=[310.0, np.nan, 285.0, 315.0])), ("outside the range", dict(T=[310.0, 284.0, 285.0, 315.0])),
              ("not distinct", dict(T=[300.0, 300.0, 285.0, 315.0])), ("range", dict(T=[310.0, 290.0, 315.0, 285.0]))]
    for fn, extra in ((normal, [("flags", dict(flags=1))]),
                      (fit, [("flags", dict(flags=2)), ("flags", dict(flags=3)), ("max_iter", dict(max_iter=-1)), ("max_iter", dict(max_iter=IM + 1)),
                             ("lambda0", dict(lambda0=-1.0)), ("lambda0", dict(lambda0=np.inf)), ("lambda0", dict(lambda0=np.nan)),
                             ("ftol", dict(ftol=-1.0)), ("ftol", dict(ftol=np.nan)), ("NULL", dict(n_iter=None)), ("NULL", dict(status=None))])):
        for text, kw in shared + extra:
            assert fn(**kw) != 0 and text in lib.rtx_last_error().decode(), (fn.__name__, kw, lib.rtx_last_error())
        assert fn(nB=0) == 0 and fn(nPix=0) == 0
    assert not buf.any()
