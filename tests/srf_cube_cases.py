"""The per-pixel HSI cube under tabulated response functions (rtx_srf_cube_tables, rtx_srf_pixel_cube, sensor.hsi_cube_srf):
the scenes, the fp64 oracle and the fp64 node form that tests/test_srf_cube_host.py (CPU: node form against direct form)
and tests/test_gpu_srf_cube.py (the kernels against both) share. NumPy only, fixed seeds. Grid, inputs, bands and knot
sets are those of tests/srf_fused_cases.py.

    direct form (the oracle), once per pixel:
        eps_p = sum_m frac[p][m] np.interp(X, Xk, End[:, kidx[p][m]])  ->  cpu_ref.compute_LWIR_apparent_radiance at T_p
        ->  the trapezoid-weighted band average of tests/test_gpu_srf.py::reference
    node form, what the kernels evaluate in fp32, here in fp64 from srf_fused_cases.moments at the node temperatures:
        G[q][b][e] = sum_j M[q][b][j] End[j][e],   l_q(T) = prod_{r != q} (T - T_r) / (T_q - T_r)
        cube[b][p] = (C_b + sum_m frac[p][m] sum_q l_q(T_p) G[q][b][kidx[p][m]]) / N_b
"""
import numpy as np

from oracle import cpu_ref as ref

import srf_fused_cases as FC
from test_gpu_srf import reference

NPIX = 257        # ends inside a workgroup of 256 pixels and inside a round of 64
NEND_ALL = 400    # the endmember set: a scene of nEnd endmembers takes its first nEnd columns
SCENES = {"mix3_of_8": (3, 8), "mix6_of_31": (6, 31)}  # name -> (nMix, nEnd)
T_CONFIGS = {"230-350_Q8": ((230.0, 350.0), 8), "285-315_Q5": ((285.0, 315.0), 5)}  # name -> (T_range, n_nodes)
KNOTS = ("coarse", "dense")


def nodes(T_range, Q):
    """The issue's nodes: T_q = (T_lo + T_hi) / 2 + (T_hi - T_lo) / 2 cos((2 q + 1) pi / (2 Q)), written out here."""
    lo, hi = T_range
    return 0.5 * (lo + hi) + 0.5 * (hi - lo) * np.cos((2 * np.arange(Q) + 1) * np.pi / (2 * Q))


def endmembers(nk, nEnd, seed=23):
    """[nk][nEnd] float32: the first nEnd columns of one [nk][400] draw, so that scenes of different nEnd share them."""
    return np.ascontiguousarray(np.random.default_rng(seed).uniform(0.55, 1.0, (nk, NEND_ALL)).astype(np.float32)[:, :nEnd])


def scene(nPix, nMix, nEnd, T_range, seed=5, k_below=None):
    """kidx [nPix][nMix] int32 in [0, k_below or nEnd), frac [nPix][nMix] float32 (rows sum to 1 before rounding), T [nPix]
    float64 uniform over T_range; the first two pixels (where there are that many) sit on the two ends of the range."""
    r = np.random.default_rng(seed)
    kidx = r.integers(0, nEnd if k_below is None else k_below, (nPix, nMix)).astype(np.int32)
    frac = r.random((nPix, nMix)) + 0.05
    frac = (frac / frac.sum(axis=1, keepdims=True)).astype(np.float32)
    T = r.uniform(T_range[0], T_range[1], nPix)
    T[:2] = np.asarray(T_range, dtype=np.float64)[:min(2, nPix)]
    return dict(kidx=kidx, frac=frac, T=T)


def direct_cube(c, End, sc):
    """[nB][nPix] fp64: the oracle, pixel by pixel. c: a case of srf_fused_cases (its float32 tau / La / Ld)."""
    X, Xk = c["X"], c["Xk"]
    used = np.unique(sc["kidx"])
    em = {k: np.interp(X, Xk, End[:, k].astype(np.float64)) for k in used}
    col = lambda v: np.asarray(v).astype(np.float64)[:, None]
    tau, La, Ld = col(c["tau"]), col(c["La"]), col(c["Ld"])
    nPix, nMix = sc["kidx"].shape
    L = np.empty((X.size, nPix))
    for p in range(nPix):
        eps = sum(float(sc["frac"][p, m]) * em[sc["kidx"][p, m]] for m in range(nMix))
        L[:, p] = ref.compute_LWIR_apparent_radiance(X, eps[:, None], np.array([sc["T"][p]]), tau, La, Ld)[:, 0, 0]
    return reference(X, c["tables"], L)[0]


def lagrange(T, Tq):
    """[nPix][Q] fp64: l_q(T_p) in the product form."""
    T, Tq = np.asarray(T, dtype=np.float64), np.asarray(Tq, dtype=np.float64)
    w = np.ones((T.size, Tq.size))
    for q in range(Tq.size):
        for r in range(Tq.size):
            if r != q:
                w[:, q] *= (T - Tq[r]) / (Tq[q] - Tq[r])
    return w


def node_cube(N, Cb, M, End, sc, Tq):
    """[nB][nPix] fp64 node form from moments (N [nB], C [nB], M [Q][nB][nk]) at the node temperatures Tq; N = 0 gives NaN."""
    G = M @ np.asarray(End).astype(np.float64)  # [Q][nB][nEnd]
    w = lagrange(sc["T"], Tq)                   # [nPix][Q]
    s = np.zeros((M.shape[1], sc["T"].size))
    for m in range(sc["kidx"].shape[1]):
        Gm = G[:, :, sc["kidx"][:, m]]          # [Q][nB][nPix]
        s += sc["frac"][:, m].astype(np.float64)[None, :] * np.einsum("pq,qbp->bp", w, Gm)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (Cb[:, None] + s) / N[:, None]


_CACHE = {}


def node_moments(c, knots, tname):
    """srf_fused_cases.moments of a case at the node temperatures of a T configuration, made once."""
    key = ("moments", knots, tname)
    if key not in _CACHE:
        T_range, Q = T_CONFIGS[tname]
        _CACHE[key] = FC.moments(c["X"], c["tables"], c["tau"], c["La"], c["Ld"], c["Xk"], nodes(T_range, Q))
    return _CACHE[key]


def case(c, knots, sname, tname):
    """One accuracy case, made once and frozen: the scene, its endmembers, the oracle `want` and the fp64 node form `node`."""
    key = (knots, sname, tname)
    if key not in _CACHE:
        nMix, nEnd = SCENES[sname]
        T_range, Q = T_CONFIGS[tname]
        End = endmembers(c["Xk"].size, nEnd)
        sc = scene(NPIX, nMix, nEnd, T_range)
        N, Cb, M, _ = node_moments(c, knots, tname)
        out = dict(End=End, T_range=T_range, Q=Q, want=direct_cube(c, End, sc), node=node_cube(N, Cb, M, End, sc, nodes(T_range, Q)), **sc)
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def worst(got, want, dead):
    """max over the live bands of |got - want| / the band's largest |want| over the scene; dead bands NaN in every pixel
    and nowhere else."""
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.broadcast_to(dead[:, None], got.shape))
    live = ~dead
    return float(np.max(np.abs(got[live] - want[live]) / np.max(np.abs(want[live]), axis=1, keepdims=True)))
