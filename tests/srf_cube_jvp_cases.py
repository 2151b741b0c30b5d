"""The tangent of the per-pixel HSI cube under response tables (rtx_srf_pixel_cube_jvp, sensor.hsi_cube_srf_jvp,
rt.compute_hsi_cube_jvp): the fp64 oracle that tests/test_srf_cube_jvp_host.py (CPU: the oracle against central differences
of srf_cube_cases.node_cube, and against the adjoint's oracle) and tests/test_gpu_srf_cube_jvp.py (the kernels against it)
share. NumPy only, fixed seeds. Grid, bands and knot sets are those of tests/srf_fused_cases.py, the scenes those of
tests/srf_cube_cases.py.

    t_m  = sum_q l_q(T_p)  G[q][b][k_pm],   t'_m = sum_q l'_q(T_p) G[q][b][k_pm],   s_m = sum_q l_q(T_p) dL[v][q][b][k_pm]
    d_cube[v][b][p] = sum_m ( d_frac[v][p][m] t_m + d_Tpix[v][p] frac[p][m] t'_m ) / N_b
                    + sum_m frac[p][m] s_m + (1 - sum_m frac[p][m]) dL[v][0][b][nEnd]
"""
import numpy as np

import srf_cube_cases as CC
import srf_cube_vjp_cases as VC


def tangent(N, G, dL, sc, Tq, T_range, d_frac, d_Tpix):
    """The fp64 oracle. N [nB]; G [Q][nB][nEnd] (the table, laid out as M . End gives it); dL [n_vec][Q][nB][nEnd + 1]; sc: a
    scene (kidx, frac, T); Tq the nodes; d_frac [n_vec][nPix][nMix]; d_Tpix [n_vec][nPix]. dL, d_frac, d_Tpix: each may be
    None (an exact zero), not all three. Returns a dict: d_cube [n_vec][nB][nPix], NaN on a dead band (N = 0) and down the
    column of a pixel that is not admitted, and under "scale" the sum of the absolute values of the same summands."""
    N = np.asarray(N).astype(np.float64)
    G = np.asarray(G).astype(np.float64)
    Q, nB, nEnd = G.shape
    given = [x for x in (dL, d_frac, d_Tpix) if x is not None]
    assert given
    nV = np.shape(given[0])[0]
    T = np.asarray(sc["T"], dtype=np.float64)
    ok = VC.admitted(T, T_range)
    Ts = np.where(ok, T, 0.5 * (T_range[0] + T_range[1]))  # a stand-in where the pixel is refused: its column is masked
    live = N > 0.0
    Nl = np.where(live, N, 1.0)[:, None]
    w, wp = CC.lagrange(Ts, Tq), VC.dlagrange(Ts, Tq)
    k = np.clip(sc["kidx"], 0, nEnd - 1)
    f = np.asarray(sc["frac"]).astype(np.float64)
    nPix, nMix = k.shape
    out, scale = np.zeros((nV, nB, nPix)), np.zeros((nV, nB, nPix))
    for v in range(nV):
        for m in range(nMix):
            Gm = G[:, :, k[:, m]]  # [Q][nB][nPix]
            if d_frac is not None:
                df = np.asarray(d_frac[v]).astype(np.float64)[:, m][None, :]
                out[v] += df * np.einsum("pq,qbp->bp", w, Gm) / Nl
                scale[v] += np.abs(df) * np.einsum("pq,qbp->bp", np.abs(w), np.abs(Gm)) / Nl
            if d_Tpix is not None:
                dT = (np.asarray(d_Tpix[v], dtype=np.float64) * f[:, m])[None, :]
                out[v] += dT * np.einsum("pq,qbp->bp", wp, Gm) / Nl
                scale[v] += np.abs(dT) * np.einsum("pq,qbp->bp", np.abs(wp), np.abs(Gm)) / Nl
            if dL is not None:
                dm = np.asarray(dL[v]).astype(np.float64)[:, :, k[:, m]]
                out[v] += f[:, m][None, :] * np.einsum("pq,qbp->bp", w, dm)
                scale[v] += np.abs(f[:, m])[None, :] * np.einsum("pq,qbp->bp", np.abs(w), np.abs(dm))
        if dL is not None:
            rest = 1.0 - f.sum(axis=1)
            d0 = np.asarray(dL[v]).astype(np.float64)[0, :, nEnd]
            out[v] += rest[None, :] * d0[:, None]
            scale[v] += np.abs(rest)[None, :] * np.abs(d0)[:, None]
    bad = ~(live[:, None] & ok[None, :])
    out[:, bad] = np.nan
    scale[:, bad] = np.nan
    return dict(d_cube=out, scale=scale)


def radiance_tangent(N, M, End, dC=None, dM=None, dEnd=None):
    """dL [Q][nB][nEnd + 1] fp64 of L = (C + M . [End | 0]) / N along directions in C [nB], M [Q][nB][nk] and End [nk][nEnd], N
    held: (dC + dM . [End | 0] + M . [dEnd | 0]) / N; NaN where N = 0."""
    pad = lambda E: np.concatenate([np.asarray(E).astype(np.float64), np.zeros((M.shape[2], 1))], axis=1)
    num = np.zeros((M.shape[0], M.shape[1], np.shape(End)[1] + 1))
    if dC is not None:
        num = num + dC[None, :, None]
    if dM is not None:
        num = num + dM @ pad(End)[None]
    if dEnd is not None:
        num = num + M @ pad(dEnd)[None]
    with np.errstate(invalid="ignore", divide="ignore"):
        return num / N[None, :, None]


def directions(nV, nB, Q, nEnd, nPix, nMix, dead, seed=11):
    """Random tangents of both signs for the three groups of rtx_srf_pixel_cube_jvp: dL [nV][Q][nB][nEnd + 1] float32 whose
    column nEnd holds the same value at every node (as rtx_srf_radiance_jvp writes it) and whose dead bands are NaN, d_frac
    [nV][nPix][nMix] float32, d_Tpix [nV][nPix] float64."""
    r = np.random.default_rng(seed)
    dL = r.uniform(-1.0, 1.0, (nV, Q, nB, nEnd + 1)).astype(np.float32)
    dL[:, :, :, nEnd] = dL[:, :1, :, nEnd]
    dL[:, :, np.asarray(dead, dtype=bool)] = np.nan
    d_frac = r.uniform(-1.0, 1.0, (nV, nPix, nMix)).astype(np.float32)
    d_Tpix = r.uniform(-2.0, 2.0, (nV, nPix))
    return dL, d_frac, d_Tpix
