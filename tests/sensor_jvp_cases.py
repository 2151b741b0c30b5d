"""Tangent of the fused band radiances under response tables (rtx_srf_radiance_jvp, sensor.band_radiance_srf_jvp): the fp64
NumPy restatement of the definition, shared by tests/test_sensor_jvp_host.py (CPU: the oracle tangent against the oracle
forward srf_fused_cases.direct_form and against the oracle adjoint sensor_vjp_cases.adjoint) and
tests/test_gpu_sensor_jvp.py (the kernels against it). The inputs, bands and emissivity knots are srf_fused_cases' own;
nothing is added to them. NumPy only, fixed seeds.

With w_b,i = R_b(X_i) D_i, N_b = sum_i w, hat_j np.interp's hats on Xk (ends held), eps_e,i = sum_j hat_j(X_i) E[j][e] and
tangents d_tau, d_La, d_Ld [nX], d_Ts [nT], d_E [nk][nE]:

    c'_i   = d_tau_i Ld_i + tau_i d_Ld_i + d_La_i
    m'_t,i = d_tau_i (B(X_i, Ts_t) - Ld_i) + tau_i (dB/dT(X_i, Ts_t) d_Ts_t - d_Ld_i)
    C'_b = sum_i w c'_i,     M'[t][b][j] = sum_i w m'_t,i hat_j(X_i)
    dL[t][b][e] = (C'_b + sum_j M'[t][b][j] E[j][e] + sum_j M[t][b][j] d_E[j][e]) / N_b

Every value comes with its scale: the same sum with every term's absolute value. A band with N_b = 0 is NaN in both."""
import numpy as np

from oracle import cpu_ref as ref

import srf_fused_cases as FC
import sensor_vjp_cases as VC

GROUPS = ("d_tau", "d_La", "d_Ld", "d_Ts", "d_E")


def tangents(c, nE, nT, seed, only=GROUPS):
    """One random direction of both signs in the inputs of case c: the rows up to half the input they belong to (float32,
    what the kernels receive), d_Ts within -+2 K, d_E up to half of E (float32). Groups not in `only` are None."""
    r = np.random.default_rng(seed)
    rel = lambda x: (np.asarray(x, dtype=np.float64) * r.uniform(-0.5, 0.5, np.shape(x))).astype(np.float32)
    d = dict(d_tau=rel(c["tau"]), d_La=rel(c["La"]), d_Ld=rel(c["Ld"]), d_Ts=r.uniform(-2.0, 2.0, nT), d_E=rel(c["E"][:, :nE]))
    return {k: (v if k in only else None) for k, v in d.items()}


def tangent(X, tables, tau, La, Ld, Xk, E, Ts, d_tau=None, d_La=None, d_Ld=None, d_Ts=None, d_E=None):
    """fp64 (dL, scale), each [nT][nB][nE]; a group left None is zero. La is taken for the signature's sake: L is linear in
    it and its tangent does not depend on it."""
    X, Xk = np.asarray(X, dtype=np.float64), np.asarray(Xk, dtype=np.float64)
    tau, Ld = (np.asarray(v).astype(np.float64) for v in (tau, Ld))
    E = np.asarray(E).astype(np.float64)
    Ts = np.atleast_1d(np.asarray(Ts, dtype=np.float64))
    nX, nT, nB, nk = X.size, Ts.size, len(tables), Xk.size
    f64 = lambda v, shape: np.zeros(shape) if v is None else np.asarray(v).astype(np.float64).reshape(shape)
    dt, da, dd, dTs, dE = f64(d_tau, nX), f64(d_La, nX), f64(d_Ld, nX), f64(d_Ts, nT), f64(d_E, E.shape)
    w, N = VC.weights(X, tables)
    j0, j1, f = FC.knot_intervals(X, Xk)
    B, dB = ref.planckian(X, Ts), VC.planck_dT(X, Ts)  # [nX][nT]
    col = lambda v: v[:, None]

    def knot_moments(a):
        """[nT][nB][nk] = sum_i w a[i][t] hat_j(X_i)"""
        M = np.zeros((nT, nB, nk))
        for t in range(nT):
            for b in range(nB):
                wa = w[b] * a[:, t]
                M[t, b] = np.bincount(j0, weights=wa * (1.0 - f), minlength=nk) + np.bincount(j1, weights=wa * f, minlength=nk)
        return M

    C1 = w @ (dt * Ld + tau * dd + da)
    C1a = w @ (np.abs(dt * Ld) + np.abs(tau * dd) + np.abs(da))
    M1 = knot_moments(col(dt) * (B - col(Ld)) + col(tau) * (dB * dTs[None, :] - col(dd)))
    M1a = knot_moments(col(np.abs(dt)) * (B + col(np.abs(Ld))) + col(np.abs(tau)) * (dB * np.abs(dTs)[None, :] + col(np.abs(dd))))
    M = knot_moments(col(tau) * (B - col(Ld)))
    Ma = knot_moments(col(np.abs(tau)) * (B + col(np.abs(Ld))))
    num = C1[None, :, None] + M1 @ E + M @ dE
    numa = C1a[None, :, None] + M1a @ np.abs(E) + Ma @ np.abs(dE)
    with np.errstate(invalid="ignore", divide="ignore"):
        return num / N[None, :, None], np.where(N[None, :, None] > 0.0, numa / N[None, :, None], np.nan)


_CACHE = {}


def case_tangent(CH, K, knots, nE, many, seed, only=GROUPS):
    """tangent() of srf_fused_cases.case(CH, K, knots) with its first nE emissivity columns, for TS_LIST (many) or TS_SCALAR,
    along tangents(seed, only); made once and frozen. Returns (the tangents dict, dL, scale)."""
    key = (CH, K, knots, nE, bool(many), seed, tuple(only))
    if key not in _CACHE:
        c = FC.case(CH, K, knots)
        Ts = list(FC.TS_LIST) if many else [FC.TS_SCALAR]
        d = tangents(c, nE, len(Ts), seed, only)
        dL, scale = tangent(c["X"], c["tables"], c["tau"], c["La"], c["Ld"], c["Xk"], c["E"][:, :nE], Ts, **d)
        for v in list(d.values()) + [dL, scale]:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[key] = (d, dL, scale)
    return _CACHE[key]
