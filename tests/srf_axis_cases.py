"""The response-table sensor kernels (rtx_srf_apply, rtx_srf_moments + rtx_band_mix, rtx_srf_radiance_vjp,
rtx_srf_radiance_jvp) along the spectral axis they are cut on: every axis length around the cuts (chunks of CH points,
sub-chunks of 64, four rows per thread), grid shards, bands placed on the cuts and emissivity knots placed where the
sub-chunk ranges of the reduce kernels were reasoned about. The cases only: the fp64 oracles are srf_fused_cases',
sensor_vjp_cases', sensor_jvp_cases' and test_gpu_srf.reference, called on the axis a case passes. Shared by
tests/test_srf_axis_host.py (CPU: which paths the cases reach, the oracles against each other, and that a wrong kernel would
be caught) and tests/test_gpu_srf_axis_paths.py (the kernels). NumPy only, fixed seeds.

An axis is the slice [off, off + n) of one parent grid (srf_fused_cases.grid_tuple: 900 cm^-1 at 0.01 cm^-1, 3 CH + 7
points); the kernels cut it at multiples of CH and of 64 from ITS first point, and its trapezoid cells are its own (half
cells at the slice's ends), so every row index below is local to the slice."""
import numpy as np

import sensor_cases as SC
import srf_fused_cases as FC
import sensor_vjp_cases as VC
import sensor_jvp_cases as JC
from test_gpu_srf import over_rows, reference, smooth_Y

CH_HOST = 1024   # rtx_srf_chunk_points(), pinned by tests/test_srf_axis_host.py against the built library
SUB = 64         # SRFM_SUB = SRFJ_SUB
SLOTS = 16       # SRF_SLOTS: bands per launch group
STEP = 0.01
NE_MAX = 3
KNOTS_SHORT = ("one_inside", "one_below", "straddle", "all_below", "all_above", "on_cuts", "cluster")
KNOTS_SHARD = ("straddle", "on_cuts", "coarse")


def lengths(CH):
    return (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, CH - 1, CH, CH + 1, 2 * CH, 2 * CH + 1)


def shards(CH):
    return tuple((off, n) for off in (1, 63, 64, CH - 1, CH, CH + 1) for n in (1, 65, CH + 1))


def knot_kinds(off, n):
    """The knot sets an axis takes: cluster from 65 points on, on_cuts from 2; a shard takes the three of the issue."""
    if off:
        return tuple(k for k in KNOTS_SHARD if k != "on_cuts" or n >= 2)
    return tuple(k for k in KNOTS_SHORT if (k != "cluster" or n >= 65) and (k != "on_cuts" or n >= 2))


def many_bands(CH, off, n):
    """The two axes that carry more than SLOTS bands: a second launch group runs."""
    return n == CH + 1 and off in (0, 64)


def all_cases(CH):
    """[(off, n, knots, nE, many)]: every axis with every knot set it takes; nE in {1, 3} and scalar Ts / TS_LIST go round
    the list so that every axis sees both of each."""
    out = []
    for off, n in [(0, n) for n in lengths(CH)] + list(shards(CH)):
        for kind in knot_kinds(off, n):
            i = len(out)
            out.append((off, n, kind, (1, 3)[i % 2], bool((i // 2) % 2)))
    return out


def cuts(CH, n):
    """The rows either side of every sub-chunk-0 | 1 cut and chunk-0 | 1 cut the axis has, as (left, right) pairs."""
    return [(a, a + 1) for a in (SUB - 1, CH - 1) if a + 1 < n]


# ---------------------------------------------------------------------------------------------------------- inputs
def axis(CH, off, n):
    return SC.grid_axis(*FC.grid_tuple(CH))[off:off + n].copy()


def bands(X, CH, many=False):
    """(tables, dead, names) on the axis X; a band that needs rows the axis does not have is left out."""
    n = X.size
    span = X[-1] - X[0]
    t, names, dead = [], [], []

    def add(name, table, is_dead=False):
        names.append(name); t.append(table); dead.append(is_dead)

    if many:  # in front, so that the bands on the chunk cut and the dead bands fall into the second launch group
        for i in range(8):
            c = X[(n - 1) * (i + 1) // 9]
            add("tri%d" % i, (np.array([c - 0.04 * span, c + 0.01 * span, c + 0.05 * span]), np.array([0.0, 1.0, 0.0])))
    add("whole", (np.array([X[0] - 0.013, X[0] + 0.3 * span + 0.001, X[0] + 0.8 * span + 0.002, X[-1] + 0.017]),
                  np.array([0.1, 1.0, 0.5, 0.3])))
    if n >= 2:
        add("ends", (np.array([X[0], X[-1]]), np.array([0.25, 1.0])))
    rows = sorted({0, n - 1} | {r for pair in cuts(CH, n) for r in pair})
    for r in rows:
        add("row%d" % r, over_rows(X, r, r))
    for a, b in cuts(CH, n):
        add("rows%d_%d" % (a, b), over_rows(X, a, b, (0.5, 1.0)))
    if n >= 2:
        i = SUB - 1 if n > SUB else 0
        g = X[i + 1] - X[i]
        add("dead_between", (np.array([X[i] + 0.25 * g, X[i] + 0.5 * g, X[i] + 0.75 * g]), np.array([0.0, 1.0, 0.0])), True)
    add("dead_below", (np.array([X[0] - 2.0, X[0] - 1.0, X[0] - 1e-9]), np.array([0.0, 1.0, 1.0])), True)
    add("dead_above", (np.array([X[-1] + 1e-9, X[-1] + 1.0]), np.array([1.0, 1.0])), True)
    return t, np.array(dead), names


def knot_set(X, CH, kind):
    n = X.size
    if kind == "coarse":
        return FC.knot_set(X, "coarse")
    if kind == "one_inside":
        return np.array([X[(n - 1) // 2] + 0.3 * STEP]) if n >= 2 else X[:1].copy()
    if kind == "one_below":
        return np.array([X[0] - 0.5])
    if kind == "straddle":
        return np.array([X[0] - 0.5, X[-1] + 0.5])
    if kind == "all_below":
        return X[0] - np.array([1.5, 1.0, 0.5])
    if kind == "all_above":
        return X[-1] + np.array([0.5, 1.0, 1.5])
    if kind == "on_cuts":
        assert n >= 2
        return X[sorted({0, n - 1} | {r for pair in cuts(CH, n) for r in pair})].copy()
    assert kind == "cluster" and n >= 65
    i = cluster_row(n)
    inner = X[i] + (X[i + 1] - X[i]) * (np.arange(300) + 1.0) / 301.0
    assert X[i] < inner[0] and inner[-1] < X[i + 1] and np.all(np.diff(inner) > 0.0)
    return np.concatenate([[X[0] - 5.0], inner, [X[-1] + 5.0]])


def cluster_row(n):
    """The cluster lies between this row and the next: the middle of the middle full sub-chunk."""
    return SUB * ((n // SUB) // 2) + SUB // 2 - 1


def _freeze(*dicts):
    for d in dicts:
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)


_CACHE = {}


def case(CH, off, n, knots):
    """Everything of one (axis, knot set), made once and frozen, as srf_fused_cases.case: X, the fp32 rows the kernels
    receive (slices of FC.inputs on the parent axis), the tables, Xk, E [nk][3] and, from the fp32 rows in fp64 for TS_LIST,
    N, C, M, jrange, M's scale Ma and the direct form's radiances `want` [3][nB][3]; TS_SCALAR is TS_LIST's middle entry."""
    key = (CH, off, n, knots)
    if key not in _CACHE:
        parent = SC.grid_axis(*FC.grid_tuple(CH))
        X = parent[off:off + n].copy()
        d = {k: v[off:off + n].astype(np.float32) for k, v in FC.inputs(parent).items()}
        tables, dead, names = bands(X, CH, many_bands(CH, off, n))
        Xk = knot_set(X, CH, knots)
        E = np.ascontiguousarray(FC.emissivities(Xk.size)[:, :NE_MAX])
        N, Cb, M, jr = FC.moments(X, tables, d["tau"], d["La"], d["Ld"], Xk, FC.TS_LIST)
        Ma = FC.moments_scale(X, tables, d["tau"], d["Ld"], Xk, FC.TS_LIST)
        want = FC.direct_form(X, tables, d["tau"], d["La"], d["Ld"], Xk, E, FC.TS_LIST)
        c = dict(X=X, off=off, tables=tables, dead=dead, names=names, Xk=Xk, E=E, N=N, C=Cb, M=M, Ma=Ma, jrange=jr, want=want, **d)
        _freeze(c)
        _CACHE[key] = c
    return _CACHE[key]


def ts_of(many):
    return list(FC.TS_LIST) if many else [FC.TS_SCALAR]


def sel(many):
    """The rows of a case's TS_LIST arrays that ts_of(many) asks for."""
    return slice(None) if many else slice(1, 2)


_ADJ, _TAN, _APPLY = {}, {}, {}


def case_adjoint(CH, off, n, knots, nE, many):
    """(g, sensor_vjp_cases.adjoint's dict) of case() under sensor_vjp_cases.cotangent (NaN on the dead bands)."""
    key = (CH, off, n, knots, nE, bool(many))
    if key not in _ADJ:
        c = case(CH, off, n, knots)
        Ts = ts_of(many)
        g = VC.cotangent(len(Ts), len(c["tables"]), nE, c["dead"])
        o = VC.adjoint(c["X"], c["tables"], c["tau"], c["La"], c["Ld"], c["Xk"], c["E"][:, :nE], Ts, g)
        g.setflags(write=False)
        _freeze(o, o["scale"])
        _ADJ[key] = (g, o)
    return _ADJ[key]


def case_tangent(CH, off, n, knots, nE, many, seed=51):
    """(tangents, dL, scale) of case() along sensor_jvp_cases.tangents(seed), all five groups moving."""
    key = (CH, off, n, knots, nE, bool(many), seed)
    if key not in _TAN:
        c = case(CH, off, n, knots)
        Ts = ts_of(many)
        d = JC.tangents(c, nE, len(Ts), seed)
        dL, scale = JC.tangent(c["X"], c["tables"], c["tau"], c["La"], c["Ld"], c["Xk"], c["E"][:, :nE], Ts, **d)
        _freeze(d, dict(dL=dL, scale=scale))
        _TAN[key] = (d, dL, scale)
    return _TAN[key]


def case_apply(CH, off, n, nS=8):
    """rtx_srf_apply's case on the axis: (X, tables, dead, Y [n][nS] float32, want [nB][nS], denominators, support)."""
    key = (CH, off, n, nS)
    if key not in _APPLY:
        X = axis(CH, off, n)
        tables, dead, _ = bands(X, CH, many_bands(CH, off, n))
        Y = np.ascontiguousarray(smooth_Y(FC.grid_tuple(CH)[2], nS)[off:off + n])
        want, den, sup = reference(X, tables, Y)
        for a in (X, Y, want, den, sup, dead):
            a.setflags(write=False)
        _APPLY[key] = (X, tables, dead, Y, want, den, sup)
    return _APPLY[key]
