"""CPU: the continuum definition (radtxfr_amd/continuum.py). od_host against the definition written out with
scalar loops (tests/continuum_cases.py: direct_od) at the points where it can go wrong, the save / load round trip, every
ValueError, and the ABI symbol in the built library."""
import ctypes as C
import os

import numpy as np
import pytest

import continuum_cases as K
from radtxfr_amd import continuum as ct

V0, DV, N = 700.0, 10.0, 12  # nodes 700 .. 810
LAST = V0 + (N - 1) * DV


def _full():
    return K.component(ct, 1, V0, DV, N, seed=1)


def _check(cont, X, lay, rtol=1e-12):
    got = cont.od_host(X, lay["T"], lay["P"], lay["PL"], lay["MF"], lay["ID"])
    assert got.shape == (lay["T"].size, len(X)) and got.dtype == np.float64
    want = np.array([[K.direct_od(K.as_dicts(cont), float(x), float(lay["T"][l]), float(lay["P"][l]), float(lay["PL"][l]), lay["MF"][l], lay["ID"])
                      for x in X] for l in range(lay["T"].size)])
    assert np.all(got[want == 0.0] == 0.0)
    assert np.allclose(got, want, rtol=rtol, atol=0.0), np.max(np.abs(got - want) / np.maximum(want, 1e-300))
    return got


def test_on_nodes_and_in_every_kind_of_cell():
    lay = K.layers(3)
    X = [V0, V0 + 3 * DV, LAST,                 # exactly on the first, an inner and the last node
         V0 + 0.3 * DV, V0 + 0.999 * DV,        # first cell: j0 clamped to 0, t in [0, 1)
         V0 + 1.0 * DV + 1e-9, V0 + 5.5 * DV,   # inner cells: t in [1, 2)
         LAST - 0.6 * DV, LAST - 1e-9]          # last cell: j0 clamped to n - 4, t in [2, 3]
    got = _check(_full(), X, lay)
    assert np.all(got > 0.0)


def test_on_a_node_the_result_is_that_nodes_value():
    lay, cont = K.layers(3), _full()
    A = cont.layer_rows(lay["T"], lay["P"], lay["PL"], lay["MF"], lay["ID"])[0]
    for j in (0, 1, 5, N - 2, N - 1):
        nu = V0 + j * DV
        got = cont.od_host([nu], lay["T"], lay["P"], lay["PL"], lay["MF"], lay["ID"])[:, 0]
        want = nu * np.tanh(K.C2 * nu / (2.0 * lay["T"])) * A[:, j]
        assert np.allclose(got, want, rtol=1e-13, atol=0.0)


def test_just_outside_both_ends_is_exactly_zero():
    lay = K.layers(3)
    X = [np.nextafter(V0, -np.inf), V0 - 1e-6, V0 - 5.0, np.nextafter(LAST, np.inf), LAST + 1e-6, LAST + 123.0]
    got = _full().od_host(X, lay["T"], lay["P"], lay["PL"], lay["MF"], lay["ID"])
    assert np.all(got == 0.0)
    _check(_full(), X + [V0, LAST], lay)  # and the two end points themselves are inside


def test_at_T_a_and_T_b_the_stored_sets_come_back():
    c = _full().components[0]
    assert np.array_equal(c.self_coefficients(c.T_a), c.Cs_a)
    assert np.allclose(c.self_coefficients(c.T_b), c.Cs_b, rtol=4e-16, atol=0.0)
    lay = K.layers(2)  # layer 0 at T_a = 296, layer 1 at T_b = 260
    for l, Cs in ((0, c.Cs_a), (1, c.Cs_b)):
        one = ct.Continuum.from_arrays(1, V0, DV, Cs_a=Cs, Cf=c.Cf)  # no temperature dependence: the stored set as it is
        a = _full().od_host([733.0, 781.2], lay["T"][l], lay["P"][l], lay["PL"][l], lay["MF"][l:l + 1], lay["ID"])
        b = one.od_host([733.0, 781.2], lay["T"][l], lay["P"][l], lay["PL"][l], lay["MF"][l:l + 1], lay["ID"])
        assert np.allclose(a, b, rtol=1e-14, atol=0.0)
    # between and beyond the two temperatures: the power law of the definition
    assert np.allclose(c.self_coefficients(278.0), c.Cs_a * (c.Cs_b / c.Cs_a) ** 0.5, rtol=1e-15)
    assert np.allclose(c.self_coefficients(332.0), c.Cs_a * (c.Cs_b / c.Cs_a) ** -1.0, rtol=1e-15)


@pytest.mark.parametrize("kind", ["self", "foreign", "steps"])
def test_self_only_foreign_only_and_zero_nodes(kind):
    lay = K.layers(3)
    cont = K.component(ct, 2, V0, DV, N, seed=2, kind=kind)
    X = [V0 + 0.5 * DV, V0 + 2.2 * DV, V0 + 3.5 * DV, V0 + 6.9 * DV, LAST - 0.2 * DV]
    got = _check(cont, X, lay)
    if kind == "steps":  # the cubic undershoots beside a run of zeros: max(0, .) cut it somewhere
        A = cont.layer_rows(lay["T"], lay["P"], lay["PL"], lay["MF"], lay["ID"])[0]
        Xs = np.linspace(V0, LAST, 2001)
        assert np.any(cont.od_host(Xs, lay["T"], lay["P"], lay["PL"], lay["MF"], lay["ID"]) == 0.0) and A.min() == 0.0 and got.max() > 0.0


def test_x_zero_leaves_nothing_and_two_components_add_in_list_order():
    lay = K.layers(3)
    lay["MF"][:, 0] = 0.0  # the column amount W carries x: no absorber, no continuum (self or foreign)
    assert np.all(_full().od_host([733.0, 801.0], lay["T"], lay["P"], lay["PL"], lay["MF"], lay["ID"]) == 0.0)
    lay = K.layers(3)
    a, b = _full(), K.component(ct, 2, 733.3, 7.0, 5, seed=4, kind="foreign")  # 733.3 .. 761.3: part of a's range
    X = [720.0, 733.3, 740.0, 761.3, 761.4, 805.0]
    both = _check(a + b, X, lay)
    args = (X, lay["T"], lay["P"], lay["PL"], lay["MF"], lay["ID"])
    assert np.array_equal(both, a.od_host(*args) + b.od_host(*args)) and len(a + b) == 2


def test_layer_tables_are_the_float64_rows_rounded_once():
    lay = K.layers(3)
    cont = _full() + K.component(ct, 2, 733.3, 7.0, 5, seed=4, kind="foreign")
    tab, axes = cont.layer_tables(lay["T"], lay["P"], lay["PL"], lay["MF"], lay["ID"])
    rows = cont.layer_rows(lay["T"], lay["P"], lay["PL"], lay["MF"], lay["ID"])
    assert tab.dtype == np.float32 and tab.shape == (2, 3, N) and axes == [(V0, DV, N), (733.3, 7.0, 5)]
    assert np.array_equal(tab[0], rows[0].astype(np.float32)) and np.array_equal(tab[1, :, :5], rows[1].astype(np.float32))
    assert np.all(tab[1, :, 5:] == 0.0)
    # W is engine.layer_weights_od's weight of the molecule
    from radtxfr_amd import engine
    W, p = engine.layer_weights_od([(2, 1)], lay["T"], lay["P"], lay["PL"], lay["MF"], lay["ID"])
    c = cont.components[1]
    want = W[0][:, None] * p[:, None] * (296.0 / lay["T"])[:, None] * ((1.0 - lay["MF"][:, 1] * 1e-6)[:, None] * c.Cf[None, :])
    assert np.allclose(rows[1], want, rtol=1e-15, atol=0.0)


def test_save_load_round_trip_bit_for_bit(tmp_path):
    cont = _full() + K.component(ct, 2, 733.3, 7.0, 5, seed=4, kind="foreign") + K.component(ct, 7, 10.0, 0.25, 4, seed=5, kind="self")
    path = os.path.join(str(tmp_path), "cont.npz")
    cont.save(path)
    with np.load(path, allow_pickle=False) as z:  # arrays and scalars only
        assert all(z[k].dtype.kind in "fi" for k in z.files)
    back = ct.Continuum.load(path)
    assert len(back) == 3
    for a, b in zip(cont.components, back.components):
        for k in ("molecule", "v0", "dv", "n", "T_a", "T_b", "T_ref", "p_ref_atm"):
            assert getattr(a, k) == getattr(b, k) and type(getattr(a, k)) is type(getattr(b, k)), k
        for k in ("Cs_a", "Cs_b", "Cf"):
            x, y = getattr(a, k), getattr(b, k)
            assert (x is None and y is None) or (x.dtype == y.dtype and np.array_equal(x.view(np.int64), y.view(np.int64))), k
    lay = K.layers(3)
    lay["MF"] = np.concatenate([lay["MF"], [[2.09e5], [2.09e5], [2.09e5]]], axis=1)
    lay["ID"] = np.array([1, 2, 7])
    X = np.linspace(5.0, 820.0, 400)
    args = (X, lay["T"], lay["P"], lay["PL"], lay["MF"], lay["ID"])
    assert np.array_equal(cont.od_host(*args), back.od_host(*args))


def test_value_errors():
    a = np.full(6, 1e-24)
    ok = dict(molecule=1, v0=100.0, dv=1.0)
    bad = [
        dict(ok),                                                            # neither Cs_a nor Cf
        dict(ok, Cs_a=a[:3]),                                                # n < 4
        dict(ok, Cs_a=a, dv=0.0), dict(ok, Cs_a=a, dv=-1.0), dict(ok, Cs_a=a, dv=np.nan), dict(ok, Cs_a=a, v0=np.inf),
        dict(ok, Cs_a=np.where(np.arange(6) == 2, -1e-30, a)),               # negative
        dict(ok, Cf=np.where(np.arange(6) == 2, np.nan, a)),                 # not finite
        dict(ok, Cs_a=a, Cf=np.where(np.arange(6) == 5, np.inf, a)),
        dict(ok, Cs_a=a, Cs_b=a, T_b=296.0),                                 # T_b == T_a
        dict(ok, Cs_a=a, Cs_b=a),                                            # Cs_b without T_b
        dict(ok, Cf=a, Cs_b=a, T_b=260.0),                                   # Cs_b without Cs_a
        dict(ok, Cs_a=a, Cs_b=np.where(np.arange(6) == 1, 0.0, a), T_b=260.0),   # zero patterns differ
        dict(ok, Cs_a=np.where(np.arange(6) == 1, 0.0, a), Cs_b=a, T_b=260.0),
        dict(ok, Cs_a=a, Cf=a[:5]),                                          # lengths differ
        dict(ok, Cs_a=a, T_b=260.0),                                         # T_b without Cs_b
        dict(ok, Cs_a=a.reshape(2, 3)),
    ]
    for kw in bad:
        with pytest.raises(ValueError, match="continuum"):
            ct.Continuum.from_arrays(**kw)
    both_zero = np.where(np.arange(6) == 1, 0.0, a)
    ct.Continuum.from_arrays(**dict(ok, Cs_a=both_zero, Cs_b=both_zero * 0.5, T_b=260.0))  # zero on the same node: allowed
    with pytest.raises(ValueError):
        ct.Continuum([])
    lay = K.layers(3)
    c7 = ct.Continuum.from_arrays(7, 100.0, 1.0, Cf=a)
    for fn in (c7.od_host, ):
        with pytest.raises(ValueError, match="molecule 7 is not in MF_ID"):
            fn([101.0], lay["T"], lay["P"], lay["PL"], lay["MF"], lay["ID"])
    with pytest.raises(ValueError, match="molecule 7 is not in MF_ID"):
        c7.layer_tables(lay["T"], lay["P"], lay["PL"], lay["MF"], lay["ID"])


def test_synthetic_says_what_it_is():
    s = ct.synthetic()
    assert "NOT PHYSICAL" in ct.synthetic.__doc__ and len(s) == 1 and s.components[0].molecule == 1
    c = s.components[0]
    assert c.n >= 4 and c.Cs_b is not None and c.Cf is not None and c.v0 <= 475.0 and c.vend >= 6025.0
    assert np.all(c.Cs_b < c.Cs_a)  # the weaker T_b set
    assert ct.synthetic(molecule=2, foreign=False).components[0].Cf is None


def test_drop_in_refusals_come_before_any_device_work():
    """The derivative entry points and devices= refuse a continuum on a machine without a GPU too: nothing before the
    refusal touches a table or a device."""
    from radtxfr_amd import radiative_transfer as rt
    s = ct.synthetic()
    with pytest.raises(NotImplementedError, match="compute_TUD_jacobian: continuum"):
        rt.compute_TUD_jacobian(1000.0, 1001.0, continuum=s)
    with pytest.raises(NotImplementedError, match="compute_TUD_vjp: continuum"):
        rt.compute_TUD_vjp(1000.0, 1001.0, None, continuum=s)
    with pytest.raises(NotImplementedError, match="compute_TUD_jvp: continuum"):
        rt.compute_TUD_jvp(1000.0, 1001.0, None, continuum=s)
    with pytest.raises(NotImplementedError, match="compute_band_radiance_vjp: continuum"):
        rt.compute_band_radiance_vjp(1000.0, 1001.0, None, None, None, 296.0, None, continuum=s)
    with pytest.raises(NotImplementedError, match="compute_band_radiance_jvp: continuum"):
        rt.compute_band_radiance_jvp(1000.0, 1001.0, None, None, None, 296.0, None, continuum=s)
    with pytest.raises(NotImplementedError, match="continuum with devices"):
        rt.compute_TUD_batch(1000.0, 1001.0, [{}], devices=[0], continuum=s)
    with pytest.raises(ValueError, match=r"molecule\(s\) \[9\]"):
        rt.compute_TUD(1000.0, 1001.0, continuum=ct.synthetic(molecule=9))
    assert "continuum" not in rt.options


def test_abi_symbol_is_in_the_built_library():
    from radtxfr_amd import _lib
    assert "rtx_continuum_add" in _lib.PROTOTYPES and _lib.PROTOTYPES["rtx_continuum_add"][1][-2] is C.c_void_p
    lib = _lib.load()
    assert lib.rtx_continuum_add is not None and lib.rtx_continuum_tile_points() == 1024
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "radtxfr_hip.h")) as f:
        assert "int rtx_continuum_add(const rtx_grid* grid, int n_layers, const double* T_h, int n_comp" in f.read()
