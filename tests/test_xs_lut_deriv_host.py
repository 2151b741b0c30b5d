"""CPU: the host side of the derivatives through cross-section tables: afit_xs.layer_terms_d and the float64
definition built on it (afit_xs.dod_from_terms, what XsLut.dod_host evaluates on the stored rows) against central
differences of the float64 forward formula, the rule for a layer on a T node, single-node axes, the range check of a wrt
species, the C prototype, and the opt-in of the five derivative drop-ins."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import xs_deriv_cases as XC
from radtxfr_amd import afit_xs

H = 1e-2                      # K, the step of the central difference
EPS = np.finfo(np.float64).eps
# Each forward value is a sum of 12 non-negative products whose weights went through about 8 float64 operations: its
# relative error stays under 20 eps. The difference of two such values over the step carries at most 2 x 20 eps |OD| / (2 h);
# the margin below is that figure with a factor 1.6 for the derivative's own rounding and the products T OD of the bound.
ROUND = 32.0


@pytest.fixture(scope="module")
def table():
    ents = XC.entries()
    tabs, xs_rows = XC.tables(ents)
    return dict(tabs=tabs, xs_rows=xs_rows)


def _dod(t, lay, species):
    rows, w_T, w_K, idx = afit_xs.layer_terms_d(t["tabs"], *XC.largs(lay), species)
    dT, dK = afit_xs.dod_from_terms(t["xs_rows"], rows, w_T, w_K, idx)
    return rows, w_T, w_K, idx, dT, dK


def test_rows_and_species_weights_are_layer_terms_own(table):
    lay = XC.layers(3)
    for species in XC.SPECIES_LISTS + ((6, 1),):
        rows, w_T, w_K, idx = afit_xs.layer_terms_d(table["tabs"], *XC.largs(lay), species)
        rows0, _ = afit_xs.layer_terms(table["tabs"], *XC.largs(lay))
        assert rows.dtype == np.int32 and np.array_equal(rows, rows0)
        assert w_T.shape == (3, 3, 4) and w_K.shape == (len(species), 3, 4) and len(idx) == len(species)
        for s, m in enumerate(species):
            unit = np.zeros((3, 3))
            unit[:, list(XC.IDS).index(m)] = 1.0  # that molecule alone at 1 ppmv
            _, w1 = afit_xs.layer_terms(table["tabs"], lay["T"], lay["P"], lay["PL"], unit, lay["ID"])
            assert table["tabs"][idx[s]][0] == m
            for e in (0, 63, 77):  # whatever power of two the table carries: the fp32 weights are the same bits
                assert np.array_equal((w_K[s] * 2.0 ** -e).astype(np.float32), (w1[:, idx[s], :] * 2.0 ** -e).astype(np.float32))
            assert np.array_equal(w_K[s], w1[:, idx[s], :])
            others = [k for k in range(3) if k != idx[s]]
            assert not np.any(w1[:, others, :])


def _check_against_differences(t, lay, inside):
    """dod_from_terms against central differences of the forward formula for the layers `inside` (at least H inside a T
    cell). In a cell OD(T) = (A + B T) / T: the central difference of A / T is off by exactly |A| / T^2 * h^2 / (T^2 - h^2),
    that of B by nothing; the round-off of the difference is ROUND eps |OD| / h."""
    ids = [int(v) for v in lay["ID"]]
    _, _, _, _, dT, dK = _dod(t, lay, ids)
    T = lay["T"]
    Tp, Tm = T + H, T - H
    step = Tp - Tm  # exact in float64
    args = lambda Tx, MF=lay["MF"]: (t["tabs"], t["xs_rows"], Tx, lay["P"], lay["PL"], MF, lay["ID"])
    OD, ODp, ODm = XC.forward_od(*args(T)), XC.forward_od(*args(Tp)), XC.forward_od(*args(Tm))
    fd = (ODp - ODm) / step[:, None]
    g_slope = (Tp[:, None] * ODp - Tm[:, None] * ODm) / step[:, None]  # T OD is linear in T inside a cell
    A = T[:, None] * OD - T[:, None] * g_slope
    trunc = np.abs(A) / T[:, None] ** 2 * (H * H / (T[:, None] ** 2 - H * H))
    bound = trunc + ROUND * EPS * np.abs(OD) / H
    err = np.abs(dT - fd)
    worst = float(np.max(err[inside] / bound[inside]))
    print("dOD/dT against the central difference at h = %g K: worst |err| / (truncation + round-off) = %.3g" % (H, worst))
    assert np.all(np.abs(dT[inside]) > 0) and worst <= 1.0
    # the truncation term is a real part of the bound: the difference is not the derivative to round-off alone
    assert np.max(trunc[inside] / (ROUND * EPS * np.abs(OD[inside]) / H)) > 1.0
    d = 1.0  # ppmv; OD is linear in MF: exact up to round-off
    for s, m in enumerate(ids):
        up, dn = lay["MF"].copy(), lay["MF"].copy()
        up[:, s] += d
        dn[:, s] -= d
        fdm = (XC.forward_od(*args(T, up)) - XC.forward_od(*args(T, dn))) / (2.0 * d)
        bound_m = ROUND * EPS * np.abs(OD) / d
        worst = float(np.max(np.abs(dK[s] - fdm) / bound_m))
        print("dOD/dMF of molecule %d against the difference in MF: worst |err| / round-off bound = %.3g" % (m, worst))
        assert np.all(dK[s] > 0) and worst <= 1.0


def test_dod_against_central_differences(table):
    lay = XC.layers(3)
    inside = np.array([True, False, True])  # layer 1 sits on a node: its rule has a test of its own
    for Tl, ok in zip(lay["T"], inside):
        assert (min(abs(Tl - n) for n in XC.T_NODES) >= H) == ok
    _check_against_differences(table, lay, inside)


def test_on_node_rule(table):
    """A layer exactly on a T node takes the cell bracket() returns: the right one (fT exactly 0), on the last node the left
    one (fT exactly 1); its slope is that cell's, i.e. the limit from inside that cell, and not the other cell's."""
    tabs = table["tabs"]
    nP = XC.P_NODES.size
    base = XC.layers(1)
    for T_node, iT, fT, inward in ((260.0, 1, 0.0, np.inf), (300.0, 1, 1.0, -np.inf), (230.0, 0, 0.0, np.inf)):
        lay = dict(base, T=np.array([T_node]))
        i, f = afit_xs.bracket(XC.T_NODES, lay["T"])
        assert int(i[0]) == iT and float(f[0]) == fT
        rows, w_T, w_K, idx = afit_xs.layer_terms_d(tabs, *XC.largs(lay), (1, 2))
        for m in (0, 1):
            assert np.array_equal(rows[0, m] - tabs[m][3], [iT * nP, iT * nP + 1, (iT + 1) * nP, (iT + 1) * nP + 1])
        dead = (2, 3) if fT == 0.0 else (0, 1)
        assert not np.any(w_K[:, 0, dead]) and np.all(w_K[:, 0, [c for c in range(4) if c not in dead]] > 0)
        assert np.all(w_T[0, :2, :] != 0)  # the slope reaches all four corners of the cell
        near = dict(lay, T=np.nextafter(lay["T"], inward))
        _, w_in, _, _ = afit_xs.layer_terms_d(tabs, *XC.largs(near), (1, 2))
        assert np.allclose(w_T, w_in, rtol=1e-12, atol=0.0)
        if T_node == 260.0:  # an inner node: the other cell has other rows and another slope
            other = dict(lay, T=np.nextafter(lay["T"], -np.inf))
            rows_o, w_o, _, _ = afit_xs.layer_terms_d(tabs, *XC.largs(other), (1, 2))
            assert not np.array_equal(rows_o, rows)
            _, _, _, _, d_here, _ = _dod(table, lay, (1, 2))
            _, _, _, _, d_other, _ = _dod(table, other, (1, 2))
            assert np.median(np.abs(d_here - d_other) / np.abs(d_here)) > 1e-3


def test_single_node_axes(table):
    """Molecule 6 has one T node: dw/dT is 0, the derivative is -OD_6 / T, and corners 2 and 3 carry nothing. A table with
    one p node differentiates like any other."""
    lay = XC.layers(3)
    rows, w_T, w_K, idx = afit_xs.layer_terms_d(table["tabs"], *XC.largs(lay), (6,))
    _, w = afit_xs.layer_terms(table["tabs"], *XC.largs(lay))
    assert idx == [2]
    assert np.allclose(w_T[:, 2, :], -w[:, 2, :] / lay["T"][:, None], rtol=4 * EPS, atol=0.0)
    assert not np.any(w_T[:, 2, 2:]) and not np.any(w_K[0][:, 2:]) and np.all(w_T[:, 2, :2] < 0)
    rng = np.random.default_rng(3)
    ents = [dict(ID=7, T=XC.T_NODES, P_atm=np.array([0.5]), X=np.linspace(2000.0, 2000.4, 41), xs=10.0 ** rng.uniform(-24.0, -19.0, (3, 1, 41)))]
    tabs = [(7, XC.T_NODES, np.array([0.5]), 0)]
    t1 = dict(tabs=tabs, xs_rows=ents[0]["xs"].reshape(3, 41))
    lay1 = dict(T=np.array([281.3, 244.9]), P=np.array([0.9, 0.1]), PL=np.array([1.0, 2.0]), MF=np.array([[300.0], [2e3]]), ID=np.array([7]))
    rows1, w_T1, w_K1, _ = afit_xs.layer_terms_d(tabs, *XC.largs(lay1), (7,))
    assert not np.any(w_T1[:, 0, [1, 3]]) and not np.any(w_K1[0][:, [1, 3]])  # fP = 0 on the single p node, any p accepted
    _check_against_differences(t1, lay1, np.array([True, True]))


def test_range_check_of_a_wrt_species_at_zero_mixing_ratio(table):
    lay = XC.layers(3)
    lay = dict(lay, T=np.array([281.3, 310.0, 244.9]), MF=lay["MF"].copy())
    lay["MF"][1, :2] = 0.0  # the layer outside the tables of molecules 1 and 2 uses neither: the forward rule accepts it
    afit_xs.layer_terms(table["tabs"], *XC.largs(lay))
    rows, w_T, w_K, idx = afit_xs.layer_terms_d(table["tabs"], *XC.largs(lay), (6,))
    assert np.all(np.isfinite(w_T)) and not np.any(w_T[1, :2])
    with pytest.raises(ValueError, match=r"xs_lut: layer 1 \(T = 310 K\) lies outside molecule 2's table range \[230, 300\] K; there is no extrapolation"):
        afit_xs.layer_terms_d(table["tabs"], *XC.largs(lay), (6, 2))
    with pytest.raises(ValueError, match="layer 1 .*molecule 1"):
        afit_xs.layer_terms_d(table["tabs"], *XC.largs(lay), (1,))
    with pytest.raises(ValueError, match="distinct"):
        afit_xs.layer_terms_d(table["tabs"], *XC.largs(XC.layers(3)), (1, 1))
    with pytest.raises(ValueError, match="distinct molecule ids of MF_ID"):
        afit_xs.layer_terms_d(table["tabs"], *XC.largs(XC.layers(3)), (9,))


def test_prototype_header_and_symbol():
    from radtxfr_amd import _lib
    import stream_cases as S
    res, args = _lib.PROTOTYPES["rtx_xs_od_d"]
    assert res is C.c_int32 or res is C.c_int
    assert len(args) == 14 and args[-1] is C.c_uint and args[-2] is C.c_void_p
    code = re.sub(r"/\*.*?\*/", " ", S.header_text(), flags=re.S)
    m = re.search(r"\bint\s+rtx_xs_od_d\s*\(([^;{}()]*)\)\s*;", code)
    assert m, "include/radtxfr_hip.h does not declare rtx_xs_od_d"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 14 and re.fullmatch(r"void\s*\*\s*stream", params[-2]) and params[-1] == "unsigned flags"
    assert "rtx_xs_od_d" not in S.stream_entries()  # the stream is not the last parameter: rtx_continuum_add_d's form
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    assert getattr(_lib.load(), "rtx_xs_od_d") is not None


# ---- the five derivative drop-ins: refused by default, opt-in with xs_derivatives=True ---------------------------------------
class _Reached(Exception):
    pass


class _Table:
    """Stands in for an XsLut: the first thing a call does with its table is to align its axis."""
    def align(self, grid):
        raise _Reached("align(%d points)" % grid.n_total)


def _drop_ins():
    from radtxfr_amd import radiative_transfer as rt
    from radtxfr_amd import sensor
    s = sensor.Sensor.from_shape([1000.1, 1000.3], 0.1, "triangle")
    Xk = np.linspace(1000.0, 1000.5, 5)
    E = np.full((5, 3), 0.9, dtype=np.float32)
    nX, nL = 1000, np.asarray(rt.options["Ts"]).size
    kw = dict(DVOUT=0.0005, Altitudes=np.array([8.0]), line_table="no-such-table-the-checks-come-first")
    return [("compute_TUD_jacobian", lambda **k: rt.compute_TUD_jacobian(1000.0, 1000.5, **dict(kw, **k))),
            ("compute_TUD_vjp", lambda **k: rt.compute_TUD_vjp(1000.0, 1000.5, {"La": np.zeros(nX)}, **dict(kw, **k))),
            ("compute_TUD_jvp", lambda **k: rt.compute_TUD_jvp(1000.0, 1000.5, {"T": np.ones(nL)}, **dict(kw, **k))),
            ("compute_band_radiance_vjp", lambda **k: rt.compute_band_radiance_vjp(1000.0, 1000.5, s, Xk, E, 300.0, np.ones((2, 3), dtype=np.float32),
                                                                                   **dict(kw, **k))),
            ("compute_band_radiance_jvp", lambda **k: rt.compute_band_radiance_jvp(1000.0, 1000.5, s, Xk, E, 300.0, {"T": np.ones(nL)},
                                                                                   **dict(kw, **k)))]


@pytest.mark.parametrize("which", range(5))
def test_drop_ins_refuse_by_default_and_opt_in(which):
    name, call = _drop_ins()[which]
    for more in (dict(), dict(xs_derivatives=False)):
        with pytest.raises(NotImplementedError, match=name + ": xs_lut is not supported") as e:
            call(xs_lut=_Table(), **more)  # refused before the table is touched
        assert "xs_derivatives=True" in str(e.value)
        assert name == "compute_TUD_jacobian" or "compute_TUD_jacobian" not in str(e.value)
    with pytest.raises(_Reached):
        call(xs_lut=_Table(), xs_derivatives=True)
    with pytest.raises(Exception, match="no-such-table"):  # without a table the option is the plain call
        call(xs_derivatives=True)
    # what stays refused with the option on
    with pytest.raises(NotImplementedError, match="broadening"):
        call(xs_lut=_Table(), xs_derivatives=True, broadening="self")
    with pytest.raises(NotImplementedError, match="theta_r"):
        call(xs_lut=_Table(), xs_derivatives=True, theta_r=np.array([0.0, 0.3]))
