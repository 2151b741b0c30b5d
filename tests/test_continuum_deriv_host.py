"""CPU: the derivatives of the continuum definition (radtxfr_amd/continuum.py). dod_host against central
differences of od_host in float64 on the layers and both grids of tests/continuum_cases.py, the exact properties of the
piecewise definition, the node tables, the ABI symbol, and the drop-in refusals that need no device."""
import ctypes as C
import os

import numpy as np
import pytest

import continuum_cases as K
import continuum_deriv_cases as D
from radtxfr_amd import continuum as ct

H_T = 1e-3    # K: truncation ~ (h / T)^2 ~ 1e-11, round-off ~ 1e-16 T / h ~ 3e-11 of the derivative
TOL_T = 1e-7
H_MF = 1.0    # ppmv: OD is quadratic in MF between kinks, the central difference is exact up to round-off
TOL_MF = 1e-9


def _axis(name):
    g = K.GRIDS[name]
    return g["xmin"] + g["step"] * np.arange(K.N_AXIS)


def _args(lay, T=None, MF=None):
    return (lay["T"] if T is None else T, lay["P"], lay["PL"], lay["MF"] if MF is None else MF, lay["ID"])


def _sign_changes(cont, X, args_a, args_b):
    """Points [nL][nX] where some component's stencil sum changes sign between two argument sets."""
    bad = np.zeros((len(args_a[0]), X.size), dtype=bool)
    for (Sa, _, _), (Sb, _, _) in zip(D.stencil_sums(cont, X, *args_a), D.stencil_sums(cont, X, *args_b)):
        bad |= (Sa > 0.0) != (Sb > 0.0)
    return bad


def _rel_err(got, want, keep):
    scale = np.max(np.abs(want), axis=1, keepdims=True)
    assert np.all(scale > 0.0)
    return float(np.max(np.where(keep, np.abs(got - want), 0.0) / scale))


@pytest.mark.parametrize("n_comp", [1, 2])
@pytest.mark.parametrize("name", ["fine", "coarse"])
def test_dod_host_against_central_differences(name, n_comp):
    lay, X = K.layers(3), _axis(name)
    cont = K.continuum(ct, name, n_comp)
    dT, dMF = cont.dod_host(X, *_args(lay))
    assert dT.shape == (3, X.size) and dT.dtype == np.float64
    assert sorted(dMF) == sorted({c.molecule for c in cont.components})
    inside = np.zeros(X.size, dtype=bool)
    for _, _, m in D.stencil_sums(cont, X, *_args(lay)):
        inside |= m
    # temperature
    a_p, a_m = _args(lay, T=lay["T"] + H_T), _args(lay, T=lay["T"] - H_T)
    bad = _sign_changes(cont, X, a_p, a_m)
    assert bad[:, inside].mean() <= 0.01
    fd = (cont.od_host(X, *a_p) - cont.od_host(X, *a_m)) / (2.0 * H_T)
    err = _rel_err(dT, fd, ~bad)
    print("%s, %d component(s): dOD/dT against central differences %.2e (%d points left out)" % (name, n_comp, err, bad.sum()))
    assert err <= TOL_T
    # each molecule's mixing ratio
    for mol, d in dMF.items():
        col = list(lay["ID"]).index(mol)
        step = np.zeros_like(lay["MF"])
        step[:, col] = H_MF
        a_p, a_m = _args(lay, MF=lay["MF"] + step), _args(lay, MF=lay["MF"] - step)
        bad = _sign_changes(cont, X, a_p, a_m)
        assert bad[:, inside].mean() <= 0.01
        fd = (cont.od_host(X, *a_p) - cont.od_host(X, *a_m)) / (2.0 * H_MF)
        err = _rel_err(d, fd, ~bad)
        print("%s, %d component(s): dOD/dMF[%d] against central differences %.2e (%d points left out)" % (name, n_comp, mol, err, bad.sum()))
        assert err <= TOL_MF


def test_zero_wherever_the_optical_depth_is_zero():
    """The "steps" component on the coarse grid: max(0, .) cuts the cubic's undershoot on part of its axis, and most of the
    grid lies outside the axis; the derivatives are exactly 0.0 on both."""
    lay, X = K.layers(3), _axis("coarse")
    m, v0, dv, n, kind = K.GRIDS["coarse"]["comps"][1]
    cont = K.component(ct, m, v0, dv, n, seed=4, kind=kind)
    c = cont.components[0]
    od = cont.od_host(X, *_args(lay))
    dT, dMF = cont.dod_host(X, *_args(lay))
    inside = (X >= c.v0) & (X <= c.vend)
    clamped = inside[None, :] & (od == 0.0)
    assert 0 < inside.sum() < X.size and clamped.any() and (od[:, inside] > 0.0).any()
    assert np.all(od[:, ~inside] == 0.0)
    for d in (dT, dMF[m]):
        assert np.all(d[od == 0.0] == 0.0) and not np.any(np.signbit(d[od == 0.0]))
        assert np.all(d[od > 0.0] != 0.0)


def test_a_mixing_ratio_of_zero_gives_finite_derivatives():
    """dA/dMF is formed without a division by x: at MF = 0 it is N g Cf 1e-6, finite and positive. The optical depth and its
    stencil sum are 0 there, so dOD/dMF takes the value the definition gives the kink, 0."""
    lay, X = K.layers(3), _axis("fine")
    cont = K.continuum(ct, "fine", 1)
    MF = lay["MF"].copy()
    MF[1, 0] = 0.0
    A, A_T, A_x = cont.components[0].layer_rows_d(*_args(lay, MF=MF))
    assert np.all(A[1] == 0.0) and np.all(A_T[1] == 0.0)
    assert np.all(np.isfinite(A_x)) and np.all(A_x[1] > 0.0)
    c = cont.components[0]
    N = (lay["P"][1] / K.P0 / 9.869233e-7) / (1.380648813e-16 * lay["T"][1]) * lay["PL"][1] * 1e5  # n(p, T) PL 1e5
    want = 1e-6 * N * (lay["P"][1] / K.P0) * (296.0 / lay["T"][1]) * c.Cf
    assert np.allclose(A_x[1], want, rtol=1e-14, atol=0.0)
    dT, dMF = cont.dod_host(X, *_args(lay, MF=MF))
    assert np.all(np.isfinite(dT)) and np.all(np.isfinite(dMF[1]))
    assert np.all(dT[1] == 0.0) and np.all(dMF[1][1] == 0.0) and np.all(dMF[1][0] > 0.0)


def test_components_of_one_molecule_share_an_entry():
    lay, X = K.layers(3), _axis("coarse")
    (m1, v1, d1, n1, k1), (_, v2, d2, n2, k2) = K.GRIDS["coarse"]["comps"]
    a = K.component(ct, m1, v1, d1, n1, seed=3, kind=k1)
    b = K.component(ct, m1, v2, d2, n2, seed=4, kind=k2)  # the second axis, on the first one's molecule
    other = K.component(ct, 2, v2, d2, n2, seed=5, kind="foreign")
    dT, dMF = (a + other + b).dod_host(X, *_args(lay))
    assert sorted(dMF) == [1, 2]
    dT_a, dMF_a = a.dod_host(X, *_args(lay))
    dT_b, dMF_b = b.dod_host(X, *_args(lay))
    dT_o, dMF_o = other.dod_host(X, *_args(lay))
    assert np.array_equal(dMF[1], dMF_a[1] + dMF_b[1]) and np.array_equal(dMF[2], dMF_o[2])
    assert np.array_equal(dT, (dT_a + dT_o) + dT_b)  # list order
    assert np.any(dMF_b[1] != 0.0) and np.any(dMF_o[2] != 0.0)


@pytest.mark.parametrize("name", ["fine", "coarse"])
def test_layer_tables_d_keeps_the_bits_of_layer_tables(name):
    lay = K.layers(3)
    cont = K.continuum(ct, name, 2)
    tab, axes = cont.layer_tables(*_args(lay))
    A, A_T, A_x, axes_d = cont.layer_tables_d(*_args(lay))
    assert axes_d == axes
    for t in (A, A_T, A_x):
        assert t.dtype == np.float32 and t.shape == tab.shape and np.all(np.isfinite(t))
    assert np.array_equal(A.view(np.uint32), tab.view(np.uint32))
    rows = cont.layer_rows_d(*_args(lay))
    for i, (r, r_T, r_x) in enumerate(rows):  # each rounded once from float64; the columns past a component's n are 0
        n = r.shape[1]
        assert np.array_equal(A_T[i, :, :n], r_T.astype(np.float32)) and np.array_equal(A_x[i, :, :n], r_x.astype(np.float32))
        assert np.all(A_T[i, :, n:] == 0.0) and np.all(A_x[i, :, n:] == 0.0)
        assert np.array_equal(r, cont.components[i].layer_rows(*_args(lay)))
    with pytest.raises(ValueError, match="molecule 7 is not in MF_ID"):
        ct.Continuum.from_arrays(7, 100.0, 1.0, Cf=np.ones(6)).layer_tables_d(*_args(lay))
    with pytest.raises(ValueError, match="molecule 7 is not in MF_ID"):
        ct.Continuum.from_arrays(7, 100.0, 1.0, Cf=np.ones(6)).dod_host([101.0], *_args(lay))


def test_abi_symbol_is_in_the_built_library():
    from radtxfr_amd import _lib
    assert "rtx_continuum_add_d" in _lib.PROTOTYPES
    res, args = _lib.PROTOTYPES["rtx_continuum_add_d"]
    assert res is C.c_int32 and args[-2] is C.c_void_p and args[-1] is C.c_uint and len(args) == 18
    assert _lib.load().rtx_continuum_add_d is not None
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "radtxfr_hip.h")) as f:
        assert "int rtx_continuum_add_d(const rtx_grid* grid, int n_layers, const double* T_h, int n_comp" in f.read()


def test_drop_in_option_is_checked_before_any_device_work():
    """continuum_derivatives=True: a continuum whose molecule MFs_ID lacks is compute_TUD's ValueError in each of the five
    derivative functions, on a machine without a GPU too; with the default False the refusal stands."""
    from radtxfr_amd import radiative_transfer as rt
    c9, s = ct.synthetic(molecule=9), ct.synthetic()
    calls = [(rt.compute_TUD_jacobian, ()), (rt.compute_TUD_vjp, (None,)), (rt.compute_TUD_jvp, (None,)),
             (rt.compute_band_radiance_vjp, (None, None, None, 296.0, None)),
             (rt.compute_band_radiance_jvp, (None, None, None, 296.0, None))]
    with pytest.raises(ValueError, match=r"molecule\(s\) \[9\]") as want:
        rt.compute_TUD(1000.0, 1001.0, continuum=c9)
    for fn, rest in calls:
        with pytest.raises(ValueError, match=r"molecule\(s\) \[9\]") as got:
            fn(1000.0, 1001.0, *rest, continuum=c9, continuum_derivatives=True)
        assert str(got.value).split(":", 1)[1] == str(want.value).split(":", 1)[1]
        for kw in (dict(), dict(continuum_derivatives=False)):
            with pytest.raises(NotImplementedError, match=fn.__name__ + ": continuum is not supported"):
                fn(1000.0, 1001.0, *rest, continuum=s, **kw)
    assert "continuum_derivatives" not in rt.options
