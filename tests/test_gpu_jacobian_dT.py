"""dT_method="analytic" through rt.compute_TUD_jacobian, rt.compute_TUD_vjp and rt.compute_band_radiance_vjp on the GPU:
the T rows of tests/test_gpu_jacobian.py's case against the same fp64 fixed-window differences at h = 0.01, at the
species' tolerance and without the float32 line-sum floor that the central-difference route needs for the returnOD tau
slot; that route's own error in that slot as the yardstick (the analytic one at least 10 x smaller); the adjoint against
the contraction of the stored analytic J; and the default method's bits through the old entry point."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_err
from oracle import cpu_ref as ref

import dT_cases as D

pytestmark = pytest.mark.gpu

LO, HI, DV = D.LO, D.HI, D.DV
ALTS = np.concatenate((np.array([200, 500, 1000, 2000, 5000, 10000, 20000, 50000]) * 0.3048 / 1e3, [100.0]))  # test_gpu_jacobian.py
LAYERS = [0, 17, 65]
TOL_SPECIES = 2e-4  # test_gpu_jacobian.py
TOL_T = 2e-3        # test_gpu_jacobian.py
F32_FLOOR = 1e-30   # test_gpu_jacobian.py
U32 = 2.0 ** -24
F32_TINY = 2.0 ** -126
H = 0.01


@pytest.fixture(scope="module")
def rt():
    import torch
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    from radtxfr_amd import _lib
    _lib.load()
    from radtxfr_amd import radiative_transfer
    return radiative_transfer


def _rows(X, OD, T, Z, returnOD):
    tau, Lu, Ld = ref.tud_from_od(X, OD, T, Z, Altitudes=ALTS, theta_r=0.0, N_angle=30, returnOD=returnOD)
    return tau.T, Lu.T, Ld  # [9][nX], [9][nX], [nX]


@pytest.fixture(scope="module")
def case():
    """The column, the oracle's optical depths of all 66 layers and, per returnOD, the base rows and the fixed-window
    differences of the three layers at h = 0.01: computed once, read-only."""
    sub, X = D.jacobian_column()
    a = D.standard_atmosphere()
    nL = a["Ts"].size
    OD = np.zeros((X.size, nL))
    for l in range(nL):
        OD[:, l] = ref.layer_od(sub, X, a["Ts"][l], a["Ps"][l], a["PLs"][l], a["MFs_VAL"][l], a["MFs_ID"])
    col = {}
    for l in LAYERS:
        col[l] = [ref.od_fixed_window(sub, X, a["Ts"][l] + s * H, a["Ts"][l], a["Ps"][l], a["PLs"][l], a["MFs_VAL"][l], a["MFs_ID"])
                  for s in (1.0, -1.0)]
    fds, bases = {}, {}
    for returnOD in (False, True):
        bases[returnOD] = _rows(X, OD, a["Ts"], a["Zs"], returnOD)
        for l in LAYERS:
            rows = []
            for s, o in zip((1.0, -1.0), col[l]):
                T = a["Ts"].copy()
                T[l] += s * H
                O = OD.copy()
                O[:, l] = o
                rows.append(_rows(X, O, T, a["Zs"], returnOD))
            fds[(returnOD, l)] = [(p_ - m_) / (2 * H) for p_, m_ in zip(*rows)]
    OD.setflags(write=False)
    return sub, a, X, OD, bases, fds


def _cmp(got, fd, base, step, tol, what, eps_rel=1e2 * np.finfo(np.float64).eps):
    """test_gpu_jacobian.py's _cmp without its floor_abs argument: the only floor is the rounding noise of the fp64
    difference itself, 1e2 eps max|base| / (2 step)."""
    noise = max(eps_rel * float(np.max(np.abs(base))) / (2.0 * step), F32_FLOOR)
    mx = float(np.max(np.abs(fd)))
    if mx * tol <= 2.0 * noise:
        assert float(np.max(np.abs(got - fd))) <= 2.0 * noise / tol * 1e-3 + noise, what
        return 0.0
    ff = max(1e-3, 2.0 * noise / (tol * mx))
    e = rel_err(got, fd, floor_frac=ff)
    assert e <= tol, (what, e, ff, mx, noise)
    return e


@pytest.mark.parametrize("returnOD", [False, True])
def test_temperature_analytic_against_oracle(rt, case, returnOD):
    sub, a, X, OD, bases, fds = case
    kw = dict(wrt=("T",), layers=LAYERS, DVOUT=DV, line_table=sub, Altitudes=ALTS, returnOD=returnOD, **a)
    _, _, _, _, J = rt.compute_TUD_jacobian(LO, HI, dT_method="analytic", **kw)
    base = bases[returnOD]
    worst = 0.0
    for c, l in enumerate(LAYERS):
        fd = fds[(returnOD, l)]
        for a_ in range(ALTS.size):
            worst = max(worst, _cmp(J["T"][0][:, a_, c], fd[0][a_], base[0][a_], H, TOL_SPECIES, ("T", l, "tau", a_)))
            worst = max(worst, _cmp(J["T"][1][:, a_, c], fd[1][a_], base[1][a_], H, TOL_SPECIES, ("T", l, "Lu", a_)))
        worst = max(worst, _cmp(J["T"][2][..., c], fd[2], base[2], H, TOL_SPECIES, ("T", l, "Ld")))
    print("analytic T rows, returnOD=%s: worst rel_err %.3e (bound %.0e)" % (returnOD, worst, TOL_SPECIES))
    if returnOD:
        # the yardstick: the central-difference route in the slot that is mu sum dOD/dT itself (top altitude: every layer)
        _, _, _, _, Jf = rt.compute_TUD_jacobian(LO, HI, **kw)
        top = ALTS.size - 1
        for c, l in enumerate(LAYERS):
            want = fds[(True, l)][0][top]
            e_an = rel_err(J["T"][0][:, top, c], want, floor_frac=1e-3)
            e_fd = rel_err(Jf["T"][0][:, top, c], want, floor_frac=1e-3)
            print("returnOD tau slot, layer %d: fd %.3e analytic %.3e" % (l, e_fd, e_an))
            assert 10.0 * e_an <= e_fd, (l, e_an, e_fd)


def test_vjp_is_the_contraction_of_the_analytic_jacobian(rt, case):
    sub, a, X, OD, _, _ = case
    alts = np.array([0.5, 30.0, 8.0])
    wrt = ("T", 1)
    kw = dict(DVOUT=DV, line_table=sub, Altitudes=alts, dT_method="analytic", **a)
    nX, nZ, nL = X.size, alts.size, a["Ts"].size
    rng = np.random.default_rng(3)
    n_vec = 2
    g_tau = rng.normal(size=(nX, nZ, n_vec))
    g_La = rng.normal(size=(nX, nZ, n_vec))
    g_La[:, 1, 0] = 0.0
    g_Ld = rng.normal(size=(nX, n_vec))
    g_Ld[nX // 4:nX // 2] = 0.0
    _, _, _, _, grad = rt.compute_TUD_vjp(LO, HI, {"tau": g_tau, "La": g_La, "Ld": g_Ld}, wrt=wrt, layers=LAYERS, **kw)
    _, _, _, _, J = rt.compute_TUD_jacobian(LO, HI, wrt=wrt, layers=LAYERS, **kw)
    G32 = lambda g: g.astype(np.float32).astype(np.float64)  # the cotangent the device is given
    for w in wrt:
        dtau, dLa, dLd = J[w]
        terms = [("xav,xal->lv", G32(g_tau), dtau), ("xav,xal->lv", G32(g_La), dLa), ("xv,xl->lv", G32(g_Ld), dLd)]
        want = sum(np.einsum(s, g, j) for s, g, j in terms)
        scale = sum(np.einsum(s, np.abs(g), np.abs(j)) for s, g, j in terms)
        g_sum = np.abs(G32(g_tau)).sum(axis=(0, 1)) + np.abs(G32(g_La)).sum(axis=(0, 1)) + np.abs(G32(g_Ld)).sum(axis=0)
        bound = 4.0 * U32 * scale + F32_TINY * g_sum[None, :]  # test_gpu_tud_vjp.py's bound (_within)
        assert np.count_nonzero(want) > 0.5 * want.size
        err = np.abs(grad[w] - want)
        print("vjp vs stored analytic J, wrt %r: worst |got - ref| / bound = %.3g" % (w, float(np.max(err / bound))))
        assert np.all(err <= bound), (w, float(np.max(err / bound)))
    # the species entry does not depend on the method
    _, _, _, _, grad_fd = rt.compute_TUD_vjp(LO, HI, {"tau": g_tau, "La": g_La, "Ld": g_Ld}, wrt=wrt, layers=LAYERS,
                                             **dict(kw, dT_method="fd"))
    assert np.array_equal(grad[1], grad_fd[1]) and not np.array_equal(grad["T"], grad_fd["T"])


def test_band_radiance_vjp_matches_the_fd_route(rt):
    """rt.compute_band_radiance_vjp(dT_method="analytic") on test_gpu_sensor_vjp.py's thinned end-to-end case: everything but
    the "T" entry has the "fd" route's bits; the "T" entries differ by at most TOL_T sum|g J|, with g the native-grid
    cotangents of the sensor adjoint and J the stored analytic Jacobian."""
    import torch
    from radtxfr_amd import engine, sensor, synthetic
    lo, hi, dv = 1000.0, 1000.5, 0.0005
    full = synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)
    sub = synthetic.subset_table(full, lo - 12.0, hi + 12.0)
    a = D.standard_atmosphere()
    a["MFs_VAL"] = a["MFs_VAL"] * 1e-3
    wrt = ("T", 1)
    kw = dict(DVOUT=dv, line_table=sub, Altitudes=np.array([8.0]), **a)
    s = sensor.Sensor.from_shape([1000.10, 1000.14, 1000.38], 0.06, "triangle")
    Xk = np.array([999.9, 1000.07, 1000.2, 1000.33, 1000.6])
    nB, nk, nE, Ts_s = 3, 5, 3, 296.0
    rng = np.random.default_rng(3)
    E = rng.uniform(0.6, 1.0, (nk, nE)).astype(np.float32)
    cot = rng.normal(size=(nB, nE)).astype(np.float32)
    _, L_an, g_an = rt.compute_band_radiance_vjp(lo, hi, s, Xk, E, Ts_s, cot, wrt=wrt, dT_method="analytic", **kw)
    _, L_fd, g_fd = rt.compute_band_radiance_vjp(lo, hi, s, Xk, E, Ts_s, cot, wrt=wrt, **kw)
    assert np.array_equal(L_an, L_fd)
    for k in (1, "Ts_surface", "emis"):
        assert np.array_equal(g_an[k], g_fd[k]), k
    X, tau, La, Ld = rt.compute_TUD(lo, hi, **kw)
    grid = engine.Grid(lo, hi, X.size)
    dev32 = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float32).ravel(), device="cuda")
    rows = sensor.band_radiance_srf_vjp(grid, dev32(tau), dev32(La), dev32(Ld), Xk, torch.as_tensor(E, device="cuda"), Ts_s, s, cot)
    G = {k: rows[k].double().cpu().numpy() for k in ("G_tau", "G_La", "G_Ld")}
    _, _, _, _, J = rt.compute_TUD_jacobian(lo, hi, wrt=("T",), dT_method="analytic", **kw)
    dtau, dLa, dLd = J["T"]  # [nX][nL] each (one altitude)
    scale = np.abs(G["G_tau"]) @ np.abs(dtau) + np.abs(G["G_La"]) @ np.abs(dLa) + np.abs(G["G_Ld"]) @ np.abs(dLd)
    err = np.abs(g_an["T"] - g_fd["T"])
    print("band radiance vjp, T: worst |analytic - fd| / sum|g J| = %.3e (bound %.0e)" % (float(np.max(err / np.maximum(scale, 1e-300))), TOL_T))
    assert np.count_nonzero(g_an["T"]) >= 2 and np.all(np.isfinite(g_an["T"]))
    assert np.all(err <= TOL_T * scale)


def test_default_method_is_the_old_entry_point_bit_for_bit(rt, case):
    """engine.tud_jacobian with the default dT_method against rtx_tud_jacobian called directly on the same columns."""
    import torch
    from radtxfr_amd import _lib, engine
    lib = _lib.load()
    sub, a, X, OD, _, _ = case
    tbl = rt._resolve_table(sub)
    grid = engine.Grid(LO, HI, X.size)
    args = (tbl, grid, a["Zs"], a["Ts"], a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"])
    wrt = ("T", 1)
    J = engine.tud_jacobian(*args, Altitudes=ALTS, wrt=wrt, layers=LAYERS)[4]
    assert torch.equal(J, engine.tud_jacobian(*args, Altitudes=ALTS, wrt=wrt, layers=LAYERS, dT_method="fd")[4])
    s = engine._jacobian_stages("test", *args, ALTS, 0.0, 30, False, wrt, LAYERS, 0.5, None)
    T, Z, layers, t_pos, tau, od, ODp, ODm, K = s.T, s.Z, s.layers, s.t_pos, s.tau, s.OD, s.OD_plus, s.OD_minus, s.K
    assert ODp is not None and ODm is not None
    n, nL, nA = grid.n, T.size, ALTS.size
    mask = np.ascontiguousarray(np.stack([(Z <= zs) for zs in ALTS]).astype(np.uint8))
    out = torch.full((2, len(LAYERS), 2 * nA + 1, n), float("nan"), dtype=torch.float32, device="cuda")
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    T_h = np.ascontiguousarray(T)
    _lib.check(lib.rtx_tud_jacobian(engine._ptr(od), engine._ptr(ODp), engine._ptr(ODm), od.stride(0), 0.5, engine._ptr(K), 1,
                                    engine._ptr(tau), tau.stride(0), grid.byref(), nL, vp(T_h), nA, vp(mask), 1.0, int(mask[-1].sum()),
                                    30, 0, vp(layers), layers.size, t_pos, engine._ptr(out), n, engine._stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(out, J)
    # and the analytic route changes the T rows only
    Ja = engine.tud_jacobian(*args, Altitudes=ALTS, wrt=wrt, layers=LAYERS, dT_method="analytic")[4]
    assert torch.equal(Ja[1], J[1]) and not torch.equal(Ja[0], J[0])
