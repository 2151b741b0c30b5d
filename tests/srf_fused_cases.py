"""Fused band radiances under tabulated response functions (rtx_srf_moments, sensor.band_radiance_srf_fused): the fp64
NumPy restatement of the definition, in its direct and in its moment form, and the one set of inputs, bands and
emissivity knots that tests/test_srf_fused_host.py (CPU: the two forms against each other) and tests/test_gpu_srf_fused.py
(the kernels against them) share. NumPy only, fixed seeds.

    direct form:  eps_k = np.interp(X, Xk, E[:, k])  ->  cpu_ref.compute_LWIR_apparent_radiance  ->  the trapezoid-weighted
                  band average of tests/test_gpu_srf.py::reference
    moment form:  (C_b + sum_j M[t][b][j] E[j][k]) / N_b  with  w = R_b(X) D,  N = sum w,  C = sum w (tau Ld + La),
                  M[t][b][j] = sum w tau (B(X, Ts_t) - Ld) hat_j(X),  hat_j the hat functions of np.interp on Xk (ends held)
"""
import numpy as np

from oracle import cpu_ref as ref

import sensor_cases as SC
from test_gpu_srf import cells, over_rows, reference

TS_SCALAR = 301.5
TS_LIST = (250.0, 301.5, 340.0)
NE_ALL = 260
NE_CASES = (1, 3, 260)
KNOT_SETS = ("coarse", "dense", "on_grid")
SUBSET = (2, 9, 16)  # bands of the short tests: all three chunks, the Gaussian, a triangle of the second launch group


# ------------------------------------------------------------------------------------------------------ reference
def knot_intervals(X, Xk):
    """(j0, j1, f) per point: np.interp(X, Xk, F) = (1 - f) F[j0] + f F[j1]; outside the knots j0 = j1 = the end knot."""
    nk = Xk.size
    cnt = np.searchsorted(Xk, X, side="right")  # knots <= x
    j0, j1 = np.maximum(cnt - 1, 0), np.minimum(cnt, nk - 1)
    inner = (cnt > 0) & (cnt < nk)
    f = np.zeros(X.size)
    f[inner] = (X[inner] - Xk[j0[inner]]) / (Xk[j1[inner]] - Xk[j0[inner]])
    return j0, j1, f


def moments(X, tables, tau, La, Ld, Xk, Ts):
    """fp64 (N [nB], C [nB], M [nT][nB][nk], jrange [nB][2]); a band with no point in [x_first, x_last]: N = C = 0, (0, -1)."""
    X, Xk = np.asarray(X, dtype=np.float64), np.asarray(Xk, dtype=np.float64)
    tau, La, Ld = (np.asarray(v).astype(np.float64) for v in (tau, La, Ld))
    Ts = np.atleast_1d(np.asarray(Ts, dtype=np.float64))
    j0, j1, f = knot_intervals(X, Xk)
    B = ref.planckian(X, Ts)  # [nX][nT]
    delta = cells(X)
    nB, nk = len(tables), Xk.size
    N, Cb, M, jr = np.zeros(nB), np.zeros(nB), np.zeros((Ts.size, nB, nk)), np.zeros((nB, 2), dtype=np.int32)
    for b, (xk, r) in enumerate(tables):
        xk, r = np.asarray(xk, dtype=np.float64), np.asarray(r, dtype=np.float32).astype(np.float64)
        w = np.interp(X, xk, r, left=0.0, right=0.0) * delta
        sup = np.flatnonzero((X >= xk[0]) & (X <= xk[-1]))
        jr[b] = (j0[sup[0]], j1[sup[-1]]) if sup.size else (0, -1)
        N[b], Cb[b] = w.sum(), np.sum(w * (tau * Ld + La))
        for t in range(Ts.size):
            a = w * tau * (B[:, t] - Ld)
            np.add.at(M[t, b], j0, a * (1.0 - f))
            np.add.at(M[t, b], j1, a * f)
    return N, Cb, M, jr


def moments_scale(X, tables, tau, Ld, Xk, Ts):
    """fp64 [nT][nB][nk]: the scale of M, its sum with every term's absolute value, w |tau| (B + |Ld|) hat_j; 0 for a band
    with N = 0. What an error bound of M (and of dE = sum g M / N, sensor_vjp_cases.adjoint) is measured against."""
    X, Xk = np.asarray(X, dtype=np.float64), np.asarray(Xk, dtype=np.float64)
    tau, Ld = (np.asarray(v).astype(np.float64) for v in (tau, Ld))
    Ts = np.atleast_1d(np.asarray(Ts, dtype=np.float64))
    j0, j1, f = knot_intervals(X, Xk)
    B = ref.planckian(X, Ts)  # [nX][nT]
    delta = cells(X)
    w = np.zeros((len(tables), X.size))
    for b, (xk, r) in enumerate(tables):
        xk, r = np.asarray(xk, dtype=np.float64), np.asarray(r, dtype=np.float32).astype(np.float64)
        w[b] = np.interp(X, xk, r, left=0.0, right=0.0) * delta
    live = w.sum(axis=1) > 0.0
    Ma = np.zeros((Ts.size, len(tables), Xk.size))
    for t in range(Ts.size):
        a = w * np.abs(tau) * (B[:, t] + np.abs(Ld))            # [nB][nX]
        for b in np.flatnonzero(live):
            np.add.at(Ma[t, b], j0, a[b] * (1.0 - f))
            np.add.at(Ma[t, b], j1, a[b] * f)
    return Ma


def moments_error(got, want, scale):
    """max over the elements of |got - want| / (2^-24 scale); where the scale is 0 (a knot no point under the band touches)
    got must be exactly want, which is 0."""
    got, want, scale = (np.asarray(v, dtype=np.float64) for v in (got, want, scale))
    assert got.shape == want.shape == scale.shape and np.all(np.isfinite(got))
    zero = scale == 0.0
    assert np.array_equal(got[zero], want[zero]) and not want[zero].any()
    return float(np.max(np.abs(got - want)[~zero] / (2.0 ** -24 * scale[~zero]))) if (~zero).any() else 0.0


def moment_form(N, Cb, M, E):
    """[nT][nB][nE] fp64 = (C + M . E) / N; N = 0 gives NaN."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return (Cb[None, :, None] + M @ np.asarray(E).astype(np.float64)[None]) / N[None, :, None]


def direct_form(X, tables, tau, La, Ld, Xk, E, Ts):
    """[nT][nB][nE] fp64 through the monochromatic radiances [nX][nE]."""
    X = np.asarray(X, dtype=np.float64)
    E = np.asarray(E).astype(np.float64)
    em = np.stack([np.interp(X, Xk, E[:, k]) for k in range(E.shape[1])], axis=1)
    col = lambda v: np.asarray(v).astype(np.float64)[:, None]
    out = []
    for T in np.atleast_1d(np.asarray(Ts, dtype=np.float64)):
        L = ref.compute_LWIR_apparent_radiance(X, em, np.array([T]), col(tau), col(La), col(Ld))[:, :, 0]
        out.append(reference(X, tables, L)[0])
    return np.array(out)


# ---------------------------------------------------------------------------------------------------------- inputs
def grid_tuple(CH):
    n = 3 * CH + 7
    return (900.0, 900.0 + 0.01 * (n - 1), n)


def axis(CH):
    return SC.grid_axis(*grid_tuple(CH))


def inputs(X, seed=41):
    """Smooth, physically shaped fp64 tau in (0, 1), La = (1 - tau) B(X, ~275 K), Ld = (1 - tau) B(X, ~262 K) with ripples."""
    r = np.random.default_rng(seed)
    t = np.linspace(0.0, 1.0, X.size)
    wave = lambda: sum(a * np.sin(2 * np.pi * f * t + p) for a, f, p in zip(r.uniform(0.02, 0.08, 3), r.uniform(1.0, 40.0, 3), r.uniform(0.0, 6.28, 3)))
    tau = 0.6 + wave() + 0.1 * np.sin(2 * np.pi * 300.0 * t)  # within (0.26, 0.94)
    La = (1.0 - tau) * ref.planckian(X, np.array([275.0]))[:, 0] * (1.0 + wave())
    Ld = (1.0 - tau) * ref.planckian(X, np.array([262.0]))[:, 0] * (1.3 + wave())
    return dict(tau=tau, La=La, Ld=Ld)


def bands(X, CH, K):
    """The 20 response tables: more than one launch group of 16. dead: the bands that come out NaN."""
    g = X[1] - X[0]
    same = over_rows(X, 1500, 1900, (0.0, 0.3, 1.0, 0.8, 0.1))
    gs = 1.2 / (2.0 * np.sqrt(2.0 * np.log(2.0)))
    d = np.linspace(-4.8, 4.8, 65)
    span = X[-1] - X[0]
    t = [
        over_rows(X, 100, 400),                                            # 0 a boxcar inside one chunk
        over_rows(X, CH - 250, CH + 249),                                  # 1 a boxcar across a chunk boundary
        (np.array([X[0] - 0.1 * span, X[0] + 0.3 * span, X[0] + 0.8 * span, X[-1] + 0.2 * span]), np.array([0.1, 1.0, 0.5, 0.3])),  # 2 all three chunks
        (np.array([X[1500] + 0.003 - 0.018, X[1500] + 0.003, X[1500] + 0.003 + 0.018]), np.array([0.0, 1.0, 0.0])),  # 3 narrower than 4 grid steps
        (np.array([X[CH - 1] + 0.25 * g, X[CH - 1] + 0.5 * g, X[CH - 1] + 0.75 * g]), np.array([0.0, 1.0, 0.0])),      # 4 no point under it: NaN
        (np.array([X[-1] + 1e-9, X[-1] + 0.1 * span]), np.array([1.0, 1.0])),                                          # 5 above the grid: NaN
        (np.array([X[0] - 0.2 * span, X[0] - 0.1 * span, X[0] - 1e-9]), np.array([0.0, 1.0, 1.0])),                    # 6 below the grid: NaN
        (np.array([X[0] - 2.0, X[0], X[0] + 2.0]), np.array([0.0, 1.0, 0.0])),                                         # 7 half off the low end
        (np.array([X[-1] - 1.5, X[-1], X[-1] + 1.5]), np.array([0.0, 1.0, 0.0])),                                      # 8 half off the high end
        (915.0 + d, np.exp(-0.5 * (d / gs) ** 2)),                         # 9 a 65-knot Gaussian
        (np.linspace(X[200] + 0.3 * g, X[2 * CH - 40] + 0.3 * g, K), 1.0 + 0.9 * np.sin(np.arange(K) * 0.37)),  # 10 K knots
        same, (same[0].copy(), same[1].copy()),                            # 11, 12 two identical bands
        (np.array([X[700], X[900]]), np.array([1.0, 1.0])),                # 13 a boxcar whose end knots are grid points
        (np.array([X[CH - 1], X[CH]]), np.array([0.5, 1.0])),              # 14 two rows, one either side of a chunk boundary
    ]
    for i in range(5):                                                     # 15 .. 19 overlapping triangles, centres descending
        c = X[X.size - 200 - 500 * i]
        t.append((np.array([c - 0.04 * span, c + 0.01 * span, c + 0.05 * span]), np.array([0.0, 1.0, 0.0])))
    dead = np.zeros(len(t), dtype=bool)
    dead[[4, 5, 6]] = True
    return t, dead


def knot_set(X, kind):
    """"coarse": 1 cm^-1 apart (100 points per interval) over the middle of the grid only, so the end values are held on
    both sides; "dense": 0.003 cm^-1 apart, finer than the grid (several knots per point); "on_grid": every knot a grid point."""
    if kind == "coarse":
        return 908.0037 + 1.0 * np.arange(16)
    if kind == "dense":
        return 912.0011 + 0.003 * np.arange(2000)
    return X[300:2801:50].copy()


def emissivities(nk, seed=17):
    return np.random.default_rng(seed).uniform(0.55, 1.0, (nk, NE_ALL)).astype(np.float32)


_CACHE = {}


def case(CH, K, knots):
    """Everything of one knot set, made once and frozen: X, the fp32 inputs the kernels receive, the tables, Xk, E [nk][260]
    and, from those fp32 inputs in fp64, the moments, M's scale `Ma` (moments_scale) and the direct form's radiances `want`
    for TS_LIST ([3][nB][260]; TS_SCALAR is its middle entry)."""
    key = (CH, K, knots)
    if key not in _CACHE:
        X = axis(CH)
        d64 = inputs(X)
        d = {k: v.astype(np.float32) for k, v in d64.items()}
        tables, dead = bands(X, CH, K)
        Xk = knot_set(X, knots)
        E = emissivities(Xk.size)
        N, Cb, M, jr = moments(X, tables, d["tau"], d["La"], d["Ld"], Xk, TS_LIST)
        Ma = moments_scale(X, tables, d["tau"], d["Ld"], Xk, TS_LIST)
        want = direct_form(X, tables, d["tau"], d["La"], d["Ld"], Xk, E, TS_LIST)
        c = dict(X=X, d64=d64, tables=tables, dead=dead, Xk=Xk, E=E, N=N, C=Cb, M=M, Ma=Ma, jrange=jr, want=want, **d)
        for v in list(c.values()) + list(d64.values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[key] = c
    return _CACHE[key]


def band_max(want):
    """[..., nB, 1]: each band's largest |L| over the emissivities (NaN for a NaN band)."""
    return np.max(np.abs(want), axis=-1, keepdims=True)
