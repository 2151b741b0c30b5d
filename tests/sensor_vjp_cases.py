"""Adjoint of the fused band radiances under response tables (rtx_srf_radiance_vjp, sensor.band_radiance_srf_vjp): the fp64
NumPy restatement of the definition, shared by tests/test_sensor_vjp_host.py (CPU: the oracle adjoint against the oracle
forward srf_fused_cases.direct_form) and tests/test_gpu_sensor_vjp.py (the kernels against it). The inputs, bands and
emissivity knots are srf_fused_cases' own; nothing is added to them. NumPy only, fixed seeds.

With w_b,i = R_b(X_i) D_i, N_b = sum_i w, hat_j np.interp's hats on Xk (ends held), over the live bands (N_b > 0):

    H[t][b][j] = sum_e g[t][b][e] E[j][e]
    A_t,i = sum_b (w / N_b) sum_j hat_j(X_i) H[t][b][j],      S_i = sum_t sum_b (w / N_b) sum_e g[t][b][e]
    G_tau = sum_t A_t (B_t - Ld) + S Ld,   G_La = S,   G_Ld = tau (S - sum_t A_t)
    dTs[t] = sum_i A_t,i tau dB/dT(X_i, Ts_t),   dE[j][e] = sum_t sum_b g[t][b][e] M[t][b][j] / N_b

Every value comes with its scale: the same sum with every term's absolute value."""
import numpy as np

from oracle import cpu_ref as ref

import srf_fused_cases as FC
from test_gpu_srf import cells


def planck_dT(X, Ts):
    """[nX][nT] fp64 dB/dT = B (u / T) e^u / (e^u - 1), u = c2 100 X / T."""
    X = np.asarray(X, dtype=np.float64)[:, None]
    T = np.atleast_1d(np.asarray(Ts, dtype=np.float64))[None, :]
    u = ref.C2 * 100.0 * X / T
    return ref.planckian(X[:, 0], T[0]) * (u / T) / (-np.expm1(-u))


def weights(X, tables):
    """fp64 w [nB][nX] and N [nB] as srf_fused_cases.moments forms them."""
    X = np.asarray(X, dtype=np.float64)
    delta = cells(X)
    w = np.zeros((len(tables), X.size))
    for b, (xk, r) in enumerate(tables):
        xk, r = np.asarray(xk, dtype=np.float64), np.asarray(r, dtype=np.float32).astype(np.float64)
        w[b] = np.interp(X, xk, r, left=0.0, right=0.0) * delta
    return w, w.sum(axis=1)


def cotangent(nT, nB, nE, dead, seed=5):
    """A random g [nT][nB][nE] float32 of both signs, NaN on the dead bands."""
    g = np.random.default_rng(seed).uniform(-1.0, 1.0, (nT, nB, nE)).astype(np.float32)
    g[:, np.asarray(dead, dtype=bool), :] = np.nan
    return g


def adjoint(X, tables, tau, La, Ld, Xk, E, Ts, g):
    """fp64 dict: G_tau, G_La, G_Ld [nX], dTs [nT], dE [nk][nE], N [nB], and under "scale" the same keys with every
    term's absolute value. g [nT][nB][nE]; a band with N = 0 contributes nothing, whatever its g holds."""
    X, Xk = np.asarray(X, dtype=np.float64), np.asarray(Xk, dtype=np.float64)
    tau, La, Ld = (np.asarray(v).astype(np.float64) for v in (tau, La, Ld))
    E = np.asarray(E).astype(np.float64)
    Ts = np.atleast_1d(np.asarray(Ts, dtype=np.float64))
    g = np.asarray(g).astype(np.float64)
    nT, nB, nE = g.shape
    assert nT == Ts.size and nB == len(tables) and E.shape == (Xk.size, nE)
    w, N = weights(X, tables)
    live = N > 0.0
    g = np.where(live[None, :, None], g, 0.0)
    c = np.zeros_like(w)
    c[live] = w[live] / N[live, None]
    j0, j1, f = FC.knot_intervals(X, Xk)
    B, dB = ref.planckian(X, Ts), planck_dT(X, Ts)  # [nX][nT]

    def point_sums(gg, EE):
        H = gg @ EE.T                                            # [nT][nB][nk]
        Hh = (1.0 - f) * H[:, :, j0] + f * H[:, :, j1]          # [nT][nB][nX]
        return np.einsum("bi,tbi->ti", c, Hh), np.einsum("bi,b->i", c, gg.sum(axis=(0, 2)))

    A, S = point_sums(g, E)
    Aa, Sa = point_sums(np.abs(g), np.abs(E))
    out = dict(N=N, G_tau=np.sum(A * (B.T - Ld), axis=0) + S * Ld, G_La=S, G_Ld=tau * (S - A.sum(axis=0)),
               dTs=np.sum(A * tau * dB.T, axis=1))
    scale = dict(G_tau=np.sum(Aa * (B.T + np.abs(Ld)), axis=0) + Sa * np.abs(Ld), G_La=Sa, G_Ld=np.abs(tau) * (Sa + Aa.sum(axis=0)),
                 dTs=np.sum(Aa * np.abs(tau) * dB.T, axis=1))
    # dE through the forward's own moments M (srf_fused_cases.moments), and M's sum of absolute terms for the scale
    _, _, M, _ = FC.moments(X, tables, tau, La, Ld, Xk, Ts)
    Ma = FC.moments_scale(X, tables, tau, Ld, Xk, Ts)
    invN = np.where(live, 1.0 / np.where(live, N, 1.0), 0.0)
    out["dE"] = np.einsum("tbe,tbj,b->je", g, np.where(live[None, :, None], M, 0.0), invN)
    scale["dE"] = np.einsum("tbe,tbj,b->je", np.abs(g), Ma, invN)
    out["scale"] = scale
    return out


_CACHE = {}


def case_adjoint(CH, K, knots, nE, many):
    """adjoint() of srf_fused_cases.case(CH, K, knots) with its first nE emissivity columns, for TS_LIST (many) or
    TS_SCALAR, under cotangent(); made once and frozen. Returns (g, the adjoint dict)."""
    key = (CH, K, knots, nE, bool(many))
    if key not in _CACHE:
        c = FC.case(CH, K, knots)
        Ts = list(FC.TS_LIST) if many else [FC.TS_SCALAR]
        g = cotangent(len(Ts), len(c["tables"]), nE, c["dead"])
        o = adjoint(c["X"], c["tables"], c["tau"], c["La"], c["Ld"], c["Xk"], c["E"][:, :nE], Ts, g)
        g.setflags(write=False)
        for v in list(o.values()) + list(o["scale"].values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[key] = (g, o)
    return _CACHE[key]
