"""Tangent vectors and fp64 reference products for the tests of the tangent-linear TUD (rtx_tud_jvp); no test in here.

The columns are those of tests/tud_vjp_cases.py (CASES, make); this module adds, per case, the tangents v on the case's
`layers` list, their scatter into the dense all-layer array the library takes, and the reference J v formed from the fp64
oracle Jacobian of ALL layers (tud_vjp_cases.oracle_jacobian). Everything is NumPy."""
import numpy as np

import tud_vjp_cases as vjp_cases

CASES = vjp_cases.CASES
make = vjp_cases.make
oracle_jacobian = vjp_cases.oracle_jacobian
H_T = vjp_cases.H_T
F32_FLOOR = 1e-30


def tangents(c, seed=20261019):
    """V [n_vec][n_wrt][len(layers)] float64: normal * 10^U(-2, 2) per (vector, wrt); one whole entry of the layers list
    exactly 0 when the list has more than two; with more than one vector, vector 1 entirely 0."""
    rng = np.random.default_rng(seed + 1000 + c["nL"] * 7 + c["n"])
    n_vec, n_wrt, n_lay = c["n_vec"], len(c["wrt"]), len(c["layers"])
    V = rng.normal(size=(n_vec, n_wrt, n_lay)) * 10.0 ** rng.uniform(-2.0, 2.0, (n_vec, n_wrt, 1))
    if n_lay > 2:
        V[:, :, rng.integers(0, n_lay)] = 0.0
    if n_vec > 1:
        V[1] = 0.0
    return V


def scatter(V, layers, nL):
    """The dense [n_vec][n_wrt][nL] array: entries of a repeated layer index add, in the order given."""
    V = np.asarray(V, dtype=np.float64)
    dense = np.zeros(V.shape[:2] + (nL,))
    for k, l in enumerate(layers):
        dense[:, :, l] += V[:, :, k]
    return dense


def oracle_all_layers(c, X, ref):
    """J_oracle [n_wrt][nL][rows][n] over all layers, and the element-wise denominator of tests/test_gpu_tud_paths.py,
    max(|J|, 1e-3 rowmax, 1e-30)."""
    Jo = oracle_jacobian(dict(c, layers=list(range(c["nL"]))), X, ref)
    with np.errstate(invalid="ignore"):
        rowmax = np.max(np.abs(Jo), axis=-1, keepdims=True)
        den = np.maximum(np.maximum(np.abs(Jo), 1e-3 * rowmax), F32_FLOOR)
    return Jo, den


def contract(J, den, dense):
    """(ref, S) [n_vec][rows][n] in fp64: ref = sum_{w,l} J v, S = sum_{w,l} |v| den, v the dense [n_vec][n_wrt][nL]."""
    with np.errstate(invalid="ignore"):
        return np.einsum("wlrn,vwl->vrn", J, dense), np.einsum("wlrn,vwl->vrn", den, np.abs(dense))


def reference(c, X, ref, V):
    """ref and S of `contract` for the case's tangents V (on its layers list), plus the dense vectors."""
    Jo, den = oracle_all_layers(c, X, ref)
    dense = scatter(V, c["layers"], c["nL"])
    r, S = contract(Jo, den, dense)
    return r, S, dense
