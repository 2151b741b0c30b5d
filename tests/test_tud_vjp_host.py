"""The TUD adjoint without a GPU: the C ABI of rtx_tud_vjp and its refusals (no device is touched), the argument checks of
rt.compute_TUD_vjp, and a NumPy check that pins the contraction the GPU tests use as their oracle (tud_vjp_cases.contract
of cpu_ref.jacobian_from_od) to a finite difference of the scalar cost it is the gradient of."""
import ctypes as C
import os

import numpy as np
import pytest

import tud_vjp_cases as cases
from oracle import cpu_ref
from radtxfr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the C ABI
def _call(lib, **over):
    """rtx_tud_vjp with valid host-side arguments (device pointers are never read before the refusals), overridden."""
    buf = np.zeros(64)
    p = C.c_void_p(buf.ctypes.data)
    nL, n_alt = 4, 2
    a = dict(OD=p, OD_plus=p, OD_minus=p, ld=101, fd_step=0.5, K=p, n_spec=2, tau=p, ld_tau=101,
             grid=_lib.make_grid(900.0, 1000.0, 101), n_layers=nL, T=np.linspace(290.0, 220.0, nL),
             n_alt=n_alt, mask=np.ones((n_alt, nL), dtype=np.uint8), mu=1.0, n_down=nL, n_angle=9, return_od=0,
             layers=np.arange(nL, dtype=np.int32), n_lay=nL, t_pos=0, G_tau=p, G_Lu=p, G_Ld=p, ld_G=101, n_vec=1, out=p)
    a.update(over)
    vp = lambda x: x if x is None or isinstance(x, C.c_void_p) else x.ctypes.data_as(C.c_void_p)
    return lib.rtx_tud_vjp(a["OD"], a["OD_plus"], a["OD_minus"], a["ld"], a["fd_step"], a["K"], a["n_spec"], a["tau"], a["ld_tau"],
                           C.byref(a["grid"]), a["n_layers"], vp(a["T"]), a["n_alt"], vp(a["mask"]), a["mu"], a["n_down"],
                           a["n_angle"], a["return_od"], vp(a["layers"]), a["n_lay"], a["t_pos"], a["G_tau"], a["G_Lu"],
                           a["G_Ld"], a["ld_G"], a["n_vec"], a["out"], None)


def test_vjp_abi_symbol_and_refusals():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "radtxfr_hip.h")).read()
    assert "rtx_tud_vjp" in _lib.PROTOTYPES and "int rtx_tud_vjp(" in header and hasattr(lib, "rtx_tud_vjp")
    assert len(_lib.PROTOTYPES["rtx_tud_vjp"][1]) == 28  # rtx_tud_jacobian's first 21, G_tau, G_Lu, G_Ld, ld_G, n_vec, out, stream
    assert _lib.PROTOTYPES["rtx_tud_vjp"][1][:21] == _lib.PROTOTYPES["rtx_tud_jacobian"][1][:21]
    decl = header[header.index("int rtx_tud_vjp("):]
    assert decl[:decl.index(");")].count(",") == 27
    n_max = lib.rtx_tud_vjp_max_vectors()
    assert 1 <= n_max <= 16 and "int rtx_tud_vjp_max_vectors(" in header

    def refused(text, **over):
        rc = _call(lib, **over)
        assert rc != 0 and text in lib.rtx_last_error().decode(), (over.keys(), lib.rtx_last_error())

    # the adjoint's own
    refused("all NULL", G_tau=None, G_Lu=None, G_Ld=None)
    refused("n_vec", n_vec=0)
    refused("n_vec", n_vec=n_max + 1)
    refused("ld_G", ld_G=100)
    refused("out", out=None)
    refused("tau is NULL", tau=None)  # with G_tau and without return_od
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
    refused("n_lay", n_lay=0)
    refused("mu=", mu=0.5)
    refused("t_pos", t_pos=3)
    refused("leading dimension", ld=100)
    refused("leading dimension", ld_tau=100)
    refused("layer index", layers=np.array([0, 1, 2, 4], dtype=np.int32))
    refused("temperature", T=np.array([290.0, 0.0, 250.0, 220.0]))
    g_bad = _lib.make_grid(900.0, 1000.0, 101)
    g_bad.n = 200
    assert _call(lib, grid=g_bad) != 0


# ------------------------------------------------------------------------------- rt.compute_TUD_vjp's argument checks
def _kw(**over):
    from radtxfr_amd import radiative_transfer as rt
    kw = dict(DVOUT=0.0005, Zs=rt.StdAtmos[:, 1], Ts=rt.StdAtmos[:, 5], Ps=rt.StdAtmos[:, 4], PLs=rt.StdAtmos[:, 3],
              MFs_VAL=rt.StdAtmos[:, 6:9] * 1e6, MFs_ID=np.array([1, 2, 3]), line_table="no-such-table-the-checks-come-first")
    kw.update(over)
    return kw


NX = 1000  # 1000.0 .. 1000.5 at 0.0005


@pytest.mark.parametrize("over, cot, exc, text", [
    (dict(reduce=dict(dX=0.1)), None, NotImplementedError, "reduce"),
    (dict(xs_lut=object()), None, NotImplementedError, "xs_lut"),
    (dict(broadening="self"), None, NotImplementedError, "broadening"),
    (dict(theta_r=np.array([0.0, 0.5])), None, NotImplementedError, "theta_r"),
    (dict(), {"Lu": np.zeros(NX)}, ValueError, "unknown cotangent key"),
    (dict(), {}, ValueError, "non-empty"),
    (dict(), {"La": np.zeros(NX + 1)}, ValueError, "shape"),
    (dict(), {"La": np.zeros((NX, 2)), "Ld": np.zeros((NX, 3))}, ValueError, "vector axis"),
    (dict(wrt=(7,)), None, ValueError, "MFs_ID"),
    (dict(layers=[0, 66]), None, ValueError, "layer"),
    (dict(fd_step_T=0.0), None, ValueError, "fd_step_T"),
])
def test_compute_tud_vjp_checks_raise_before_the_device(over, cot, exc, text):
    from radtxfr_amd import radiative_transfer as rt
    args = {k: over.pop(k) for k in ("wrt", "layers", "fd_step_T") if k in over}
    with pytest.raises(exc, match=text) as e:
        rt.compute_TUD_vjp(1000.0, 1000.5, {"La": np.zeros(NX)} if cot is None else cot, **args, **_kw(**over))
    assert "compute_TUD_jacobian" not in str(e.value)


def test_compute_tud_vjp_valid_arguments_reach_the_table():
    from radtxfr_amd import radiative_transfer as rt
    with pytest.raises(Exception, match="no-such-table"):
        rt.compute_TUD_vjp(1000.0, 1000.5, {"La": np.zeros((NX, 3)), "Ld": np.zeros((NX, 3))}, wrt=("T", 1), **_kw())


# -------------------------------------------------------------- the oracle contraction is the gradient of a scalar cost
@pytest.mark.parametrize("returnOD", [False, True])
@pytest.mark.parametrize("theta_r", [0.0, cases.DEG40])
def test_contracted_closed_form_is_the_gradient_of_the_cost(returnOD, theta_r):
    """cost(OD) = sum G . rows(tud_from_od(OD)). Along OD_l -> OD_l + s dOD its derivative is contract(G, g_l dOD), the
    contraction the GPU tests take as their oracle. It is compared with the central difference of the cost at step e:
      |contract - fd(e)| <= 2 noise + truncation,
    noise = 1e2 eps sum|G . rows| / (2 e), the rounding of the difference of two sums of that size (the floor
    tests/test_gpu_jacobian.py's _cmp uses, here for the summed cost), and truncation = 4/3 |fd(e) - fd(e/2)|, the leading
    e^2 term of fd(e) estimated from halving the step. Nothing in the bound is chosen by hand; that it is a meaningful one
    (small against the gradient itself) is asserted separately."""
    rng = np.random.default_rng(11)
    nX, nL = 40, 12
    X = np.linspace(700.0, 1400.0, nX)
    OD = np.exp(rng.uniform(np.log(1e-4), np.log(3.0), (nX, nL)))
    T = np.linspace(290.0, 215.0, nL) + rng.uniform(-3, 3, nL)
    Z = np.arange(nL, dtype=np.float64)
    Z[3], Z[4] = Z[4], Z[3]
    alts = np.array([11.0, -1.0, 6.0])  # the last inside the column: n_down = 7
    nZ = alts.size
    layers = np.array([0, 3, 4, 6, 7, 11])
    G = rng.normal(size=(2, 2 * nZ + 1, nX))
    G[0, 1] = 0.0
    G[:, :, 10:15] = 0.0

    def rows(O):
        tau, Lu, Ld = cpu_ref.tud_from_od(X, O, T, Z, Altitudes=alts, theta_r=theta_r, N_angle=9, returnOD=returnOD)
        return np.concatenate([tau.reshape(nX, -1).T, Lu.reshape(nX, -1).T, Ld[None, :]])

    cost = lambda O: np.einsum("vrn,rn->v", G, rows(O))
    g, _ = cpu_ref.jacobian_from_od(X, OD, T, Z, alts, theta_r=theta_r, N_angle=9, returnOD=returnOD, layers=layers)
    size = np.einsum("vrn,rn->v", np.abs(G), np.abs(rows(OD)))
    e = 1e-3
    for k, l in enumerate(layers):
        dOD = rng.uniform(0.2, 1.0, nX) * OD[:, l]  # a relative perturbation: OD stays positive

        def fd(step):
            Op, Om = OD.copy(), OD.copy()
            Op[:, l] += step * dOD
            Om[:, l] -= step * dOD
            return (cost(Op) - cost(Om)) / (2.0 * step)

        J = (g[:, :, k] * dOD[None, :])[None, None]  # [1 wrt][1 layer][rows][nX]
        got, _ = cases.contract(G, J)
        got = got[:, 0, 0]
        f1, f2 = fd(e), fd(0.5 * e)
        noise = 1e2 * np.finfo(np.float64).eps * size / (2.0 * e)
        bound = 2.0 * noise + 4.0 / 3.0 * np.abs(f1 - f2)
        assert np.all(np.abs(got - f1) <= bound), (l, got, f1, bound)
        assert np.all(bound <= 1e-4 * np.abs(f1)), (l, bound, f1)  # the check has teeth: a wrong contraction is O(1) off
