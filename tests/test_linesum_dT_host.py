"""The analytic dOD/dT without a GPU: the fp64 definition (tests/dT_cases.py) against finite differences of the oracle,
tips.partition_sums_dT against differences of partition_sums, and the C ABI of the four new entry points with their
refusals (no device is touched)."""
import ctypes as C
import os

import numpy as np
import pytest

import dT_cases as D
from oracle import cpu_ref as ref
from radtxfr_amd import _lib, tips

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------- 1. the definition against the oracle
@pytest.mark.parametrize("layer", [0, 17, 65])
def test_definition_against_fixed_window_differences(layer):
    """dod_dT against central differences of cpu_ref.od_fixed_window at h = 1e-3 K on the 1000-1004 cm^-1 column: max abs
    error <= 1e-7 of the row's max |dOD/dT|. Measured: 3.9e-11 (layer 0), 6.3e-11 (17), 2.4e-9 (65: the difference's own
    crossings of the |x| + y = 15 switch)."""
    tbl, X = D.jacobian_column()
    a = D.standard_atmosphere()
    args = (a["Ps"][layer], a["PLs"][layer], a["MFs_VAL"][layer], a["MFs_ID"])
    T = a["Ts"][layer]
    an = D.dod_dT(tbl, X, T, *args)
    h = 1e-3
    fd = (ref.od_fixed_window(tbl, X, T + h, T, *args) - ref.od_fixed_window(tbl, X, T - h, T, *args)) / (2 * h)
    mx = np.max(np.abs(fd))
    err = np.max(np.abs(an - fd)) / mx
    print("layer %d: max abs error / row max = %.3g" % (layer, err))
    assert mx > 0.0 and err <= 1e-7, err


@pytest.mark.parametrize("layer", [0, 17, 40])
def test_definition_with_shift_and_self_broadening(layer):
    """A table with deltap_air, gamma_self / n_self (a zero n_self falling back to n_air) at dil_air = 0.7, dil_self = 0.3:
    Shift0' and the self term of Gamma0'. The reference is the central difference of the fixed-window sum built from
    cpu_ref.line_params (with that mix) and PROFILE_VOIGT. With a moving centre the difference carries the rounding of
    nu0 + Shift0 (1e-13 cm^-1, times cte, over 2h), so its own error is estimated from halving the step:
    |analytic - fd(h)| <= 2 max|fd(h) - fd(h/2)| covers a truncation-dominated difference (fd(h) - fd(h/2) = 3/4 of the
    h^2 term) and a rounding-dominated one (the difference of two noisy values is no smaller than either's noise).
    That the bound has teeth -- at most 1e-5 of the row's maximum, where dropping Shift0' or the self term is an error of
    1e-2 or more -- is asserted as well."""
    tbl, _ = D.shifted_self_table()
    a = D.standard_atmosphere()
    T, p = a["Ts"][layer], a["Ps"][layer] / 101325.0
    g = (D.LO, D.LO + 4095 * D.DV, 4096, 0, 4096)
    kw = dict(dil_air=0.7, dil_self=0.3)
    an, _, _ = D.linesum_dT(tbl, g, T, p, 1.0, 0.0, **kw)
    fd = {}
    for h in (2e-2, 1e-2):
        fd[h] = (D.sum_fixed_window(tbl, g, T + h, T, p, **kw) - D.sum_fixed_window(tbl, g, T - h, T, p, **kw)) / (2 * h)
    mx = np.max(np.abs(fd[2e-2]))
    bound = 2.0 * np.max(np.abs(fd[2e-2] - fd[1e-2]))
    err = np.max(np.abs(an - fd[2e-2]))
    print("layer %d: error %.3g, bound %.3g of the row max" % (layer, err / mx, bound / mx))
    assert err <= bound, (err / mx, bound / mx)
    assert bound <= 1e-5 * mx, bound / mx
    # teeth: the two terms this table adds are far above the bound
    plain, _, _ = D.linesum_dT({k: v for k, v in tbl.items() if k != "deltap_air"}, g, T, p, 1.0, 0.0, **kw)
    air, _, _ = D.linesum_dT(tbl, g, T, p, 1.0, 0.0, dil_air=1.0, dil_self=0.0)
    assert np.max(np.abs(plain - an)) > 100 * bound and np.max(np.abs(air - an)) > 100 * bound


# ------------------------------------------------------------------------------------------ 2. tips.partition_sums_dT
SPECIES = [(1, 1), (2, 1), (3, 1), (6, 1)]


def test_partition_sums_dT_against_differences():
    """Temperatures at least 1 K from every node of 60:25:3010, in the 3-point ranges at both ends and the 4-point range
    between: rel <= 1e-8 against central differences of partition_sums at h = 1e-3."""
    T = np.array([71.5, 83.9, 86.1, 100.0, 216.65, 288.15, 296.0, 301.3, 333.9, 1000.5, 2961.0, 2984.0, 2990.0, 2999.0])
    assert np.min(np.abs(T[:, None] - D.TIPS_NODES[None, :])) >= 1.0
    h = 1e-3
    fd = (tips.partition_sums(SPECIES, T + h) - tips.partition_sums(SPECIES, T - h)) / (2 * h)
    an = tips.partition_sums_dT(SPECIES, T)
    rel = np.max(np.abs(an / fd - 1.0))
    print("partition_sums_dT: max rel error %.3g" % rel)
    assert rel <= 1e-8, rel


def test_partition_sums_dT_at_a_node_is_the_stencil_partition_sum_uses():
    """At a table node T = A[j] partition_sum takes I1 = the first node >= T, i.e. the stencil whose third node is T
    (nodes j-2 .. j+1; at the table's second node the 3-point stencil of its first three). Its derivative there, by
    numpy's own polynomial through those nodes."""
    t = tips._tab()
    A = t["tdat"]
    for j in (1, 2, 9, 10, A.size - 2):
        for key in SPECIES:
            B = t["q"][key]
            idx = [0, 1, 2] if j < 2 else [j - 2, j - 1, j, j + 1]
            c = np.polyfit(A[idx] - A[j], B[idx], len(idx) - 1)  # centred: well conditioned
            want = np.polyval(np.polyder(c), 0.0)
            got = tips.partition_sums_dT([key], [A[j]])[0, 0]
            assert abs(got - want) <= 1e-9 * abs(want), (j, key, got, want)
            # and Q itself is the node's value there: the same stencil
            assert abs(tips.partition_sum(key[0], key[1], A[j]) - B[j]) <= 1e-12 * B[j]


def test_partition_sums_dT_refuses_what_partition_sums_refuses():
    with pytest.raises(Exception, match="between 70K and 3000K"):
        tips.partition_sums_dT(SPECIES, [69.0])
    with pytest.raises(Exception, match="no data"):
        tips.partition_sums_dT([(99, 1)], [296.0])


# ------------------------------------------------------------------------------------------------------- 3. the C ABI
NEW = {"rtx_line_prep_dt": 17, "rtx_voigt_sum_dt": 7, "rtx_tud_jacobian_dod": 22, "rtx_tud_vjp_dod": 26}


def test_abi_symbols():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "radtxfr_hip.h")).read()
    for name, n_args in NEW.items():
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
        assert len(_lib.PROTOTYPES[name][1]) == n_args, name
        decl = header[header.index("int %s(" % name):]
        assert decl[:decl.index(");")].count(",") == n_args - 1, name
    # the *_dod forms are the old ones with dOD_dT in place of OD_plus, OD_minus (and no fd_step)
    for old, new in (("rtx_tud_jacobian", "rtx_tud_jacobian_dod"), ("rtx_tud_vjp", "rtx_tud_vjp_dod")):
        o, n = _lib.PROTOTYPES[old][1], _lib.PROTOTYPES[new][1]
        assert n == o[:2] + o[3:4] + o[5:], new
    assert len(_lib.PROTOTYPES["rtx_tud_jacobian"][1]) == 24 and len(_lib.PROTOTYPES["rtx_tud_vjp"][1]) == 28
    # rtx_line_prep_profile's arguments minus profile, plus dlnsw_h after mass_h
    prof = _lib.PROTOTYPES["rtx_line_prep_profile"][1]
    assert _lib.PROTOTYPES["rtx_line_prep_dt"][1] == prof[:9] + [C.c_void_p] + prof[9:15] + prof[16:]


def _tud_call(lib, name, **over):
    """A *_dod or an old entry point with valid host-side arguments (device pointers are never read before the
    refusals), overridden."""
    buf = np.zeros(64)
    p = C.c_void_p(buf.ctypes.data)
    nL, n_alt = 4, 2
    a = dict(OD=p, OD_plus=p, OD_minus=p, dOD_dT=p, ld=101, fd_step=0.5, K=p, n_spec=2, tau=p, ld_tau=101,
             grid=_lib.make_grid(900.0, 1000.0, 101), n_layers=nL, T=np.linspace(290.0, 220.0, nL),
             n_alt=n_alt, mask=np.ones((n_alt, nL), dtype=np.uint8), mu=1.0, n_down=nL, n_angle=9, return_od=0,
             layers=np.arange(nL, dtype=np.int32), n_lay=nL, t_pos=0, G_tau=p, G_Lu=p, G_Ld=p, ld_G=101, n_vec=1, out=p, J=p,
             ld_J=101)
    a.update(over)
    vp = lambda x: x if x is None or isinstance(x, C.c_void_p) else x.ctypes.data_as(C.c_void_p)
    head = (a["OD"], a["dOD_dT"], a["ld"]) if name.endswith("_dod") else (a["OD"], a["OD_plus"], a["OD_minus"], a["ld"], a["fd_step"])
    mid = (a["K"], a["n_spec"], a["tau"], a["ld_tau"], C.byref(a["grid"]), a["n_layers"], vp(a["T"]), a["n_alt"], vp(a["mask"]),
           a["mu"], a["n_down"], a["n_angle"], a["return_od"], vp(a["layers"]), a["n_lay"], a["t_pos"])
    tail = (a["J"], a["ld_J"], None) if "jacobian" in name else (a["G_tau"], a["G_Lu"], a["G_Ld"], a["ld_G"], a["n_vec"], a["out"], None)
    return getattr(lib, name)(*head, *mid, *tail)


def test_refusals_without_a_device():
    lib = _lib.load()

    def refused(rc, text):
        assert rc != 0 and text in lib.rtx_last_error().decode(), (text, lib.rtx_last_error())

    for name in ("rtx_tud_jacobian_dod", "rtx_tud_vjp_dod"):
        refused(_tud_call(lib, name, dOD_dT=None), "dOD_dT is NULL")
        # everything the old entry points refuse, through the same checks
        refused(_tud_call(lib, name, OD=None), "NULL")
        refused(_tud_call(lib, name, n_spec=17), "n_spec")
        refused(_tud_call(lib, name, K=None), "K is NULL")
        refused(_tud_call(lib, name, t_pos=3), "t_pos")
        refused(_tud_call(lib, name, ld=100), "leading dimension")
        refused(_tud_call(lib, name, n_layers=129), "n_layers")
    # the old entry points refuse what they refused
    for name in ("rtx_tud_jacobian", "rtx_tud_vjp"):
        refused(_tud_call(lib, name, OD_minus=None), "OD_plus and OD_minus are given together")
        refused(_tud_call(lib, name, OD_plus=None), "OD_plus and OD_minus are given together")
        refused(_tud_call(lib, name, fd_step=0.0), "fd_step")
    # rtx_line_prep_dt: a NULL dlnsw_h is refused before anything else is looked at
    buf = np.zeros(8)
    p = C.c_void_p(buf.ctypes.data)
    g = _lib.make_grid(900.0, 1000.0, 101)
    refused(lib.rtx_line_prep_dt(None, None, C.byref(g), 1, p, p, p, p, p, None, 1.0, 0.0, 0.0, 50.0, 0.0, 1.0, None), "dlnsw_h is NULL")
    refused(lib.rtx_line_prep_dt(None, None, C.byref(g), 1, p, p, p, p, p, p, 1.0, 0.0, 0.0, 50.0, 0.0, 1.0, None), "prep/lines is NULL")
    # rtx_voigt_sum_dt on a prep object whose last prologue was not rtx_line_prep_dt. A prep object cannot be made without a
    # device; the refusal reads one flag of it, clear after every other prologue and in a new object, so a block of
    # zeros (far larger than the object) stands in for "no rtx_line_prep_dt has run"
    blank = np.zeros(1 << 14, dtype=np.uint8)
    refused(lib.rtx_voigt_sum_dt(C.c_void_p(blank.ctypes.data), C.byref(g), 1, p, None, 101, None), "not rtx_line_prep_dt")
    refused(lib.rtx_voigt_sum_dt(None, C.byref(g), 1, p, None, 101, None), "prep is NULL")


# ------------------------------------------------------------------------------------------------ dT_method is checked
def _kw(**over):
    from radtxfr_amd import radiative_transfer as rt
    kw = dict(DVOUT=0.0005, Zs=rt.StdAtmos[:, 1], Ts=rt.StdAtmos[:, 5], Ps=rt.StdAtmos[:, 4], PLs=rt.StdAtmos[:, 3],
              MFs_VAL=rt.StdAtmos[:, 6:9] * 1e6, MFs_ID=np.array([1, 2, 3]), line_table="no-such-table-the-checks-come-first")
    kw.update(over)
    return kw


def test_unknown_dT_method_raises_before_the_device():
    from radtxfr_amd import engine, radiative_transfer as rt
    nX = 1000
    with pytest.raises(ValueError, match="dT_method"):
        rt.compute_TUD_jacobian(1000.0, 1000.5, dT_method="spline", **_kw())
    with pytest.raises(ValueError, match="dT_method"):
        rt.compute_TUD_vjp(1000.0, 1000.5, {"La": np.zeros(nX)}, dT_method="spline", **_kw())
    with pytest.raises(ValueError, match="dT_method"):
        rt.compute_band_radiance_vjp(1000.0, 1000.5, None, None, None, 300.0, None, dT_method="spline", **_kw())
    a = _kw()
    args = (None, None, a["Zs"], a["Ts"], a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"])
    with pytest.raises(ValueError, match="dT_method"):
        engine.tud_jacobian(*args, dT_method="spline")
    with pytest.raises(ValueError, match="dT_method"):
        engine.tud_vjp(*args, G_Ld=np.zeros(nX), dT_method="spline")


@pytest.mark.parametrize("method", ["fd", "analytic"])
def test_known_dT_methods_reach_the_table(method):
    from radtxfr_amd import radiative_transfer as rt
    with pytest.raises(Exception, match="no-such-table"):
        rt.compute_TUD_jacobian(1000.0, 1000.5, dT_method=method, **_kw())
    # "analytic" has no step to check
    with pytest.raises(Exception, match="no-such-table"):
        rt.compute_TUD_jacobian(1000.0, 1000.5, dT_method="analytic", fd_step_T=0.0, **_kw())
    with pytest.raises(ValueError, match="fd_step_T"):
        rt.compute_TUD_jacobian(1000.0, 1000.5, dT_method="fd", fd_step_T=0.0, **_kw())
