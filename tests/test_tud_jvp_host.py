"""The tangent-linear TUD without a GPU: the C ABI of rtx_tud_jvp and its refusals (no device is touched), the argument
checks of rt.compute_TUD_jvp, and a NumPy check that pins the reference the GPU tests use (tud_jvp_cases.reference: the
oracle Jacobian of all layers contracted with the tangents) to the directional derivative it stands for, a central
difference of cpu_ref.tud_from_od along the direction."""
import ctypes as C
import os

import numpy as np
import pytest

import tud_jvp_cases as cases
from oracle import cpu_ref
from radtxfr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the C ABI
def _call(lib, **over):
    """rtx_tud_jvp with valid host-side arguments (device pointers are never read before the refusals), overridden."""
    buf = np.zeros(64)
    p = C.c_void_p(buf.ctypes.data)
    nL, n_alt = 4, 2
    a = dict(OD=p, OD_plus=p, OD_minus=p, ld=101, fd_step=0.5, K=p, n_spec=2, tau=p, ld_tau=101,
             grid=_lib.make_grid(900.0, 1000.0, 101), n_layers=nL, T=np.linspace(290.0, 220.0, nL),
             n_alt=n_alt, mask=np.ones((n_alt, nL), dtype=np.uint8), mu=1.0, n_down=nL, n_angle=9, return_od=0,
             t_pos=0, V=np.ones((1, 3, nL)), n_vec=1, d_tau=p, d_Lu=p, d_Ld=p, ld_out=101)
    a.update(over)
    vp = lambda x: x if x is None or isinstance(x, C.c_void_p) else x.ctypes.data_as(C.c_void_p)
    return lib.rtx_tud_jvp(a["OD"], a["OD_plus"], a["OD_minus"], a["ld"], a["fd_step"], a["K"], a["n_spec"], a["tau"], a["ld_tau"],
                           C.byref(a["grid"]), a["n_layers"], vp(a["T"]), a["n_alt"], vp(a["mask"]), a["mu"], a["n_down"],
                           a["n_angle"], a["return_od"], a["t_pos"], vp(a["V"]), a["n_vec"], a["d_tau"], a["d_Lu"], a["d_Ld"],
                           a["ld_out"], None)


def test_jvp_abi_symbol_and_refusals():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "radtxfr_hip.h")).read()
    for name in ("rtx_tud_jvp", "rtx_tud_jvp_dod", "rtx_tud_jvp_max_vectors"):
        assert name in _lib.PROTOTYPES and "int %s(" % name in header and hasattr(lib, name)
    proto = _lib.PROTOTYPES["rtx_tud_jvp"][1]
    assert len(proto) == 26  # rtx_tud_jacobian's first 18, t_pos, V_h, n_vec, d_tau, d_Lu, d_Ld, ld_out, stream
    assert proto[:18] == _lib.PROTOTYPES["rtx_tud_jacobian"][1][:18]
    assert _lib.PROTOTYPES["rtx_tud_jvp_dod"][1][:16] == _lib.PROTOTYPES["rtx_tud_vjp_dod"][1][:16]
    decl = header[header.index("int rtx_tud_jvp("):]
    assert decl[:decl.index(");")].count(",") == 25
    n_max = lib.rtx_tud_jvp_max_vectors()
    assert 1 <= n_max <= 16

    def refused(text, **over):
        rc = _call(lib, **over)
        assert rc != 0 and text in lib.rtx_last_error().decode(), (over.keys(), lib.rtx_last_error())

    # the tangent's own
    refused("all NULL", d_tau=None, d_Lu=None, d_Ld=None)
    refused("n_vec", n_vec=0)
    refused("n_vec", n_vec=n_max + 1)
    refused("ld_out", ld_out=100)
    refused("V_h is NULL", V=None)
    bad = np.ones((1, 3, 4))
    bad[0, 2, 1] = np.inf
    refused("not finite", V=bad)
    bad[0, 2, 1] = np.nan
    refused("not finite", V=bad)
    refused("tau is NULL", tau=None)  # with d_tau and without return_od
    # inherited from rtx_tud_jacobian
    refused("NULL", OD=None)
    refused("NULL", T=None)
    refused("together", OD_minus=None)
    refused("fd_step", fd_step=0.0)
    refused("n_spec", n_spec=17)
    refused("K is NULL", K=None)
    refused("nothing to differentiate", OD_plus=None, OD_minus=None, n_spec=0)
    refused("n_layers", n_layers=129)
    refused("n_alt", n_alt=17)
    refused("n_angle", n_angle=97)
    refused("n_angle", n_angle=0)
    refused("n_down", n_down=5)
    refused("mu=", mu=0.5)
    refused("t_pos", t_pos=3)
    refused("leading dimension", ld=100)
    refused("leading dimension", ld_tau=100)
    refused("temperature", T=np.array([290.0, 0.0, 250.0, 220.0]))
    g_bad = _lib.make_grid(900.0, 1000.0, 101)
    g_bad.n = 200
    assert _call(lib, grid=g_bad) != 0
    # the dod entry point refuses a NULL derivative
    p = C.c_void_p(np.zeros(8).ctypes.data)
    assert lib.rtx_tud_jvp_dod(p, None, 101, p, 2, p, 101, C.byref(_lib.make_grid(900.0, 1000.0, 101)), 4, p, 2, p, 1.0, 4, 9, 0, 0,
                               p, 1, p, p, p, 101, None) != 0
    assert "dOD_dT is NULL" in lib.rtx_last_error().decode()
    # an empty shard: nothing to do, nothing written (the outputs here are not device memory)
    g0 = _lib.make_grid(900.0, 1000.0, 101)
    g0.n = 0
    assert _call(lib, grid=g0) == 0


# ------------------------------------------------------------------------------- rt.compute_TUD_jvp's argument checks
def _kw(**over):
    from radtxfr_amd import radiative_transfer as rt
    kw = dict(DVOUT=0.0005, Zs=rt.StdAtmos[:, 1], Ts=rt.StdAtmos[:, 5], Ps=rt.StdAtmos[:, 4], PLs=rt.StdAtmos[:, 3],
              MFs_VAL=rt.StdAtmos[:, 6:9] * 1e6, MFs_ID=np.array([1, 2, 3]), line_table="no-such-table-the-checks-come-first")
    kw.update(over)
    return kw


NL = 66  # the standard atmosphere's layers
_NAN = np.zeros(NL)
_NAN[5] = np.nan


@pytest.mark.parametrize("over, tan, exc, text", [
    (dict(reduce=dict(dX=0.1)), None, NotImplementedError, "reduce"),
    (dict(xs_lut=object()), None, NotImplementedError, "xs_lut"),
    (dict(broadening="self"), None, NotImplementedError, "broadening"),
    (dict(theta_r=np.array([0.0, 0.5])), None, NotImplementedError, "theta_r"),
    (dict(save=True), None, ValueError, "save"),
    (dict(), {}, ValueError, "non-empty"),
    (dict(), {"Tz": np.zeros(NL)}, ValueError, "unknown tangent key"),
    (dict(), {7: np.zeros(NL)}, ValueError, "MFs_ID"),
    (dict(), {"T": np.zeros(NL + 1)}, ValueError, "shape"),
    (dict(layers=[0, 5, 9]), {"T": np.zeros(NL)}, ValueError, "shape"),
    (dict(), {"T": np.zeros((NL, 2)), 1: np.zeros((NL, 3))}, ValueError, "vector axis"),
    (dict(), {"T": np.zeros((NL, 2)), 1: np.zeros(NL)}, ValueError, "vector axis"),
    (dict(), {"T": _NAN}, ValueError, "non-finite"),
    (dict(), {1: np.full((NL, 2), np.inf)}, ValueError, "non-finite"),
    (dict(rows=("tau", "Lu")), None, ValueError, "rows"),
    (dict(rows=()), None, ValueError, "rows"),
    (dict(layers=[0, 66]), {"T": np.zeros(2)}, ValueError, "layer"),
    (dict(fd_step_T=0.0), None, ValueError, "fd_step_T"),
    (dict(dT_method="exact"), None, ValueError, "dT_method"),
])
def test_compute_tud_jvp_checks_raise_before_the_device(over, tan, exc, text):
    from radtxfr_amd import radiative_transfer as rt
    args = {k: over.pop(k) for k in ("layers", "rows", "fd_step_T", "dT_method") if k in over}
    with pytest.raises(exc, match=text) as e:
        rt.compute_TUD_jvp(1000.0, 1000.5, {"T": np.zeros(NL)} if tan is None else tan, **args, **_kw(**over))
    assert "compute_TUD_jacobian" not in str(e.value) and "compute_TUD_vjp" not in str(e.value)


def test_compute_tud_jvp_valid_arguments_reach_the_table():
    from radtxfr_amd import radiative_transfer as rt
    with pytest.raises(Exception, match="no-such-table"):
        rt.compute_TUD_jvp(1000.0, 1000.5, {"T": np.zeros((NL, 3)), 1: np.ones((NL, 3))}, rows=("tau", "La"), **_kw())
    with pytest.raises(Exception, match="no-such-table"):
        rt.compute_TUD_jvp(1000.0, 1000.5, {3: np.zeros(3)}, layers=[4, 4, 60], dT_method="analytic", **_kw())


# -------------------------------------------------------------- the reference contraction is the directional derivative
def test_scatter_adds_repeated_layers_in_order():
    V = np.arange(2 * 3 * 5, dtype=np.float64).reshape(2, 3, 5) + 1.0
    dense = cases.scatter(V, [6, 0, 3, 3, 5], 7)
    assert dense.shape == (2, 3, 7)
    assert np.array_equal(dense[:, :, 3], V[:, :, 2] + V[:, :, 3]) and np.array_equal(dense[:, :, 6], V[:, :, 0])
    assert not dense[:, :, [1, 2, 4]].any()


@pytest.mark.parametrize("returnOD", [False, True])
@pytest.mark.parametrize("theta_r", [0.0, cases.vjp_cases.DEG40])
def test_reference_contraction_is_the_directional_derivative(returnOD, theta_r):
    """rows(s) = tud_from_od(OD + s dOD, T + s v_T), dOD_l = (dOD/dT)_l v_T[l] + sum_s K_s,l v_s[l]. Its derivative at s = 0
    is sum J_oracle v, the reference of the GPU tests (tud_jvp_cases.reference). It is compared, element by element, with
    the central difference at step e:
      |ref - fd(e)| <= 2 noise + truncation,
    noise = 1e2 eps |rows| / (2 e), the rounding of the difference of two values of that size (the floor
    tests/test_gpu_jacobian.py's _cmp uses), and truncation = 4/3 |fd(e) - fd(e/2)|, the leading e^2 term of fd(e)
    estimated from halving the step: the construction of tests/test_tud_vjp_host.py. Nothing in the bound is chosen by
    hand; that it is a meaningful one (small against the derivative's row) is asserted separately."""
    rng = np.random.default_rng(12)
    nL, nX, nA = 5, 16, 5
    X = np.linspace(700.0, 1400.0, nX)
    OD = np.exp(rng.uniform(np.log(1e-4), np.log(3.0), (nL, nX)))
    T = np.linspace(290.0, 215.0, nL) + rng.uniform(-3, 3, nL)
    Z = np.arange(nL, dtype=np.float64)
    alts = np.array([10.0, 2.5])  # the last inside the column: n_down = 3
    mu = 1.0 / np.cos(theta_r)
    wrt = (1, "T", 2)
    layers = [4, 0, 2, 2, 3]  # a repeated layer, layer 1 left out
    r = rng.uniform(-0.02, 0.02, (nL, nX))
    K = OD[None] * rng.uniform(0.0, 1.0, (2, nL, nX))
    tau = np.stack([np.exp(-mu * OD[Z <= zs].sum(axis=0)) for zs in alts])
    # float64 everywhere: the oracle takes these numbers as they are (the GPU cases hand it float32 columns)
    c = dict(nL=nL, n=nX, theta=theta_r, nA=nA, alts=alts, wrt=wrt, layers=layers, returnOD=returnOD, Z=Z, T=T, OD=OD,
             ODp=OD * (1.0 + r * cases.H_T), ODm=OD * (1.0 - r * cases.H_T), K=K, tau32=tau, mu=mu, n_vec=3)
    V = cases.tangents(c)
    V[:, 0] *= 0.3 / np.max(np.abs(V[:, 0]))  # ppmv-like steps that keep OD + s dOD positive, a few K for T
    V[:, 2] *= 0.3 / np.max(np.abs(V[:, 2]))
    V[:, 1] *= 3.0 / np.max(np.abs(V[:, 1]))
    assert not V[1].any()
    ref, S, dense = cases.reference(c, X, cpu_ref, V)
    assert ref.shape == S.shape == (3, 2 * alts.size + 1, nX)
    d_T = OD * r  # (ODp - ODm) / (2 H_T)

    def rows(vec, s):
        dOD = d_T * dense[vec, 1][:, None] + K[0] * dense[vec, 0][:, None] + K[1] * dense[vec, 2][:, None]
        O = OD + s * dOD
        assert (O > 0).all()
        tau_, Lu_, Ld_ = cpu_ref.tud_from_od(X, O.T, T + s * dense[vec, 1], Z, Altitudes=alts, theta_r=theta_r, N_angle=nA,
                                             returnOD=returnOD)
        return np.concatenate([tau_.T, Lu_.T, Ld_[None, :]])

    e = 1e-3
    for vec in range(3):
        fd = lambda step: (rows(vec, step) - rows(vec, -step)) / (2.0 * step)
        f1, f2 = fd(e), fd(0.5 * e)
        noise = 1e2 * np.finfo(np.float64).eps * np.abs(rows(vec, 0.0)) / (2.0 * e)
        bound = 2.0 * noise + 4.0 / 3.0 * np.abs(f1 - f2)
        err = np.abs(ref[vec] - f1)
        print("vector %d: worst |ref - fd| / bound = %.3g" % (vec, np.max(err / np.where(bound > 0, bound, 1.0))))
        assert np.all(err <= bound), (vec, np.argwhere(err > bound)[:5])
        if vec == 1:
            assert not ref[vec].any() and not f1.any()  # the all-zero vector
        else:
            assert np.count_nonzero(ref[vec]) > 0.9 * ref[vec].size
            # the check has teeth: a wrong contraction is O(1) of the row off
            assert np.all(bound <= 1e-4 * np.max(np.abs(f1), axis=1, keepdims=True)), vec
