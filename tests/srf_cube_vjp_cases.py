"""The adjoint of the per-pixel HSI cube under response tables (rtx_srf_pixel_cube_vjp, sensor.hsi_cube_srf_vjp,
rt.compute_hsi_cube_vjp): the fp64 oracle that tests/test_srf_cube_vjp_host.py (CPU: the oracle against central differences
of srf_cube_cases.node_cube, and the identity behind the back half) and tests/test_gpu_srf_cube_vjp.py (the kernels against
it) share. NumPy only, fixed seeds. Grid, bands and knot sets are those of tests/srf_fused_cases.py, the scenes those of
tests/srf_cube_cases.py.

    cube[b][p] = sum_m f_pm sum_q l_q(T_p) L[q][b][k_pm] + (1 - sum_m f_pm) L0[b]
    L[q][b][e] = (C_b + G[q][b][e]) / N_b,   L0[b] = C_b / N_b,   G = M . End
so with u_bp = g[b][p] on a live band and an admitted pixel, 0 otherwise,
    dfrac[p][m] = sum_b (u_bp / N_b) sum_q l_q(T_p)  G[q][b][k_pm]
    dT[p]       = sum_b (u_bp / N_b) sum_m f_pm sum_q l'_q(T_p) G[q][b][k_pm]
    gL[q][b][e] = sum_p u_bp l_q(T_p) sum_{m: k_pm = e} f_pm,   gL[0][b][nEnd] = sum_p u_bp (1 - sum_m f_pm)
"""
import numpy as np

import srf_cube_cases as CC


def dlagrange(T, Tq):
    """[nPix][Q] fp64: l'_q(T_p) = sum_{s != q} prod_{r != q, s} (T - T_r) / prod_{r != q} (T_q - T_r)."""
    T, Tq = np.asarray(T, dtype=np.float64), np.asarray(Tq, dtype=np.float64)
    Q = Tq.size
    d = np.zeros((T.size, Q))
    for q in range(Q):
        den = np.prod([Tq[q] - Tq[r] for r in range(Q) if r != q]) if Q > 1 else 1.0
        for s in range(Q):
            if s == q:
                continue
            prod = np.ones(T.size)
            for r in range(Q):
                if r != q and r != s:
                    prod = prod * (T - Tq[r])
            d[:, q] += prod
        d[:, q] /= den
    return d


def cotangent(nB, nPix, dead, seed=7):
    """A random g [nB][nPix] float32 of both signs, NaN on the dead bands."""
    g = np.random.default_rng(seed).uniform(-1.0, 1.0, (nB, nPix)).astype(np.float32)
    g[np.asarray(dead, dtype=bool)] = np.nan
    return g


def admitted(T, T_range):
    T = np.asarray(T, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(T) & (T >= T_range[0]) & (T <= T_range[1])


def adjoint(N, G, sc, Tq, T_range, g):
    """The fp64 oracle. N [nB]; G [Q][nB][nEnd] (the table, laid out as M . End gives it); sc: a scene (kidx, frac, T); Tq the
    nodes; g [nB][nPix]. Returns a dict: dT [nPix], dfrac [nPix][nMix] (NaN for a pixel that is not admitted), gL [Q][nB][nEnd + 1],
    and under "scale" the same keys with every summand's absolute value."""
    N = np.asarray(N).astype(np.float64)
    G = np.asarray(G).astype(np.float64)
    Q, nB, nEnd = G.shape
    T = np.asarray(sc["T"], dtype=np.float64)
    ok = admitted(T, T_range)
    Ts = np.where(ok, T, 0.5 * (T_range[0] + T_range[1]))  # a stand-in where the pixel is refused: its terms are masked
    live = N > 0.0
    with np.errstate(invalid="ignore"):
        u = np.where(live[:, None] & ok[None, :], np.asarray(g).astype(np.float64), 0.0)
    x = u / np.where(live, N, 1.0)[:, None]
    w, wp = CC.lagrange(Ts, Tq), dlagrange(Ts, Tq)
    k = np.clip(sc["kidx"], 0, nEnd - 1)
    f = np.asarray(sc["frac"]).astype(np.float64)
    nPix, nMix = k.shape
    dfrac, s_dfrac = np.zeros((nPix, nMix)), np.zeros((nPix, nMix))
    dT, s_dT = np.zeros(nPix), np.zeros(nPix)
    F, Fa = np.zeros((nPix, nEnd + 1)), np.zeros((nPix, nEnd + 1))
    for m in range(nMix):
        Gm = G[:, :, k[:, m]]  # [Q][nB][nPix]
        dfrac[:, m] = np.sum(x * np.einsum("pq,qbp->bp", w, Gm), axis=0)
        s_dfrac[:, m] = np.sum(np.abs(x) * np.einsum("pq,qbp->bp", np.abs(w), np.abs(Gm)), axis=0)
        dT += f[:, m] * np.sum(x * np.einsum("pq,qbp->bp", wp, Gm), axis=0)
        s_dT += np.abs(f[:, m]) * np.sum(np.abs(x) * np.einsum("pq,qbp->bp", np.abs(wp), np.abs(Gm)), axis=0)
        np.add.at(F, (np.arange(nPix), k[:, m]), f[:, m])
        np.add.at(Fa, (np.arange(nPix), k[:, m]), np.abs(f[:, m]))
    # sum_p u_bp l_q(T_p) F_pe as one matrix product [Q nB][nPix] x [nPix][nEnd + 1], fp64 all the same: the three-operand einsum
    # it replaces took 7 s for each of the two on a scene of 8000 pixels
    rows = lambda a, b: (a[None] * b.T[:, None, :]).reshape(Q * nB, nPix)
    gL = (rows(u, w) @ F).reshape(Q, nB, nEnd + 1)
    s_gL = (rows(np.abs(u), np.abs(w)) @ Fa).reshape(Q, nB, nEnd + 1)
    rest = 1.0 - f.sum(axis=1)
    gL[:, :, nEnd], s_gL[:, :, nEnd] = 0.0, 0.0
    gL[0, :, nEnd] = u @ rest
    s_gL[0, :, nEnd] = np.abs(u) @ np.abs(rest)
    dT[~ok], dfrac[~ok] = np.nan, np.nan
    return dict(dT=dT, dfrac=dfrac, gL=gL, scale=dict(dT=s_dT, dfrac=s_dfrac, gL=s_gL))


def band_radiances(N, Cb, M, End):
    """L [Q][nB][nEnd + 1] fp64 = (C + M . [End | 0]) / N: the pure endmembers and the bare surface at the nodes; NaN where N = 0."""
    E0 = np.concatenate([np.asarray(End).astype(np.float64), np.zeros((M.shape[2], 1))], axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (Cb[None, :, None] + M @ E0[None]) / N[None, :, None]


def cube_from_radiances(L, sc, Tq):
    """[nB][nPix] fp64: the cube as the linear combination of the band radiances L [Q][nB][nEnd + 1] (the back half's identity)."""
    nEnd = L.shape[2] - 1
    w = CC.lagrange(sc["T"], Tq)
    f = np.asarray(sc["frac"]).astype(np.float64)
    k = np.clip(sc["kidx"], 0, nEnd - 1)
    out = (1.0 - f.sum(axis=1))[None, :] * L[0, :, nEnd][:, None]
    for m in range(k.shape[1]):
        out = out + f[:, m][None, :] * np.einsum("pq,qbp->bp", w, L[:, :, k[:, m]])
    return out
