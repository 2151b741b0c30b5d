"""compute_TUD_jacobian without a GPU: its argument checks, and a NumPy restatement of the sensitivity formulas it
evaluates (include/radtxfr_hip.h: rtx_tud_jacobian) against fp64 finite differences of the oracle's TUD body."""
import numpy as np
import pytest

from conftest import rel_err
from oracle import cpu_ref


# ---------------------------------------------------------------------------------------------- argument checks
def _kw(**over):
    from radtxfr_amd import radiative_transfer as rt
    kw = dict(DVOUT=0.0005, Zs=rt.StdAtmos[:, 1], Ts=rt.StdAtmos[:, 5], Ps=rt.StdAtmos[:, 4], PLs=rt.StdAtmos[:, 3],
              MFs_VAL=rt.StdAtmos[:, 6:9] * 1e6, MFs_ID=np.array([1, 2, 3]), line_table="no-such-table-the-checks-come-first")
    kw.update(over)
    return kw


@pytest.mark.parametrize("over, exc, text", [
    (dict(theta_r=np.array([0.0, 0.5])), NotImplementedError, "theta_r"),
    (dict(save=True), ValueError, "save"),
    (dict(wrt=(7,)), ValueError, "MFs_ID"),
    (dict(wrt=("T", "H2O")), ValueError, "wrt"),
    (dict(wrt=("T", "T")), ValueError, "twice"),
    (dict(layers=[0, 66]), ValueError, "layer"),
    (dict(layers=[-1]), ValueError, "layer"),
    (dict(fd_step_T=0.0), ValueError, "fd_step_T"),
    (dict(fd_step_T=-0.5), ValueError, "fd_step_T"),
    (dict(N_angle=97), ValueError, "N_angle"),
    (dict(Altitudes=np.linspace(1.0, 50.0, 17)), ValueError, "altitudes"),
])
def test_argument_checks_raise_before_the_device(over, exc, text):
    from radtxfr_amd import radiative_transfer as rt
    kw = _kw()
    args = {k: over.pop(k) for k in ("wrt", "layers", "fd_step_T") if k in over}
    kw.update(over)
    with pytest.raises(exc, match=text):
        rt.compute_TUD_jacobian(1000.0, 1004.0, **args, **kw)


def test_full_resolution_host_result_is_bounded():
    from radtxfr_amd import radiative_transfer as rt
    # the caller's grid, 9 altitudes, T and 3 species over 66 layers: ~200 GB of float64 without reduce=
    alts = np.concatenate((np.array([200, 500, 1000, 2000, 5000, 10000, 20000, 50000]) * 0.3048 / 1e3, [100.0]))
    with pytest.raises(ValueError, match="reduce=") as e:
        rt.compute_TUD_jacobian(690.0, 1410.0, wrt=("T", 1, 2, 3), Altitudes=alts, **_kw())
    assert "layers=" in str(e.value)
    # a modest request passes the checks and only then needs the table (which does not exist here)
    with pytest.raises(Exception, match="no-such-table"):
        rt.compute_TUD_jacobian(1000.0, 1001.0, wrt=("T",), layers=[0], **_kw())


# ------------------------------------------------------------------ the formulas, restated in NumPy (fp64)
def _planck_dT(X, T):
    """B(nu, T) [nX][nL] of the oracle and dB/dT analytic: dB/dT = B (u/T) e^u/(e^u - 1), u = c2 nu / T."""
    B = cpu_ref.planckian(X, T)
    u = cpu_ref.C2 * (np.asarray(X)[:, None] * 100.0) / np.asarray(T)[None, :]
    return B, B * (u / np.asarray(T)[None, :]) * (-1.0 / np.expm1(-u))


def jacobian_from_od(X, OD, T, Z, Altitudes, theta_r=0.0, N_angle=30, returnOD=False, layers=None):
    """g[row][nX][layer] = d row / d OD_l and h[row][nX][layer] = d row / d T_l at fixed OD, rows = tau per altitude,
    L-up per altitude, Ld: the closed forms rtx_tud_jacobian evaluates, with prefix sums for every transmittance product."""
    OD = np.asarray(OD, dtype=np.float64)  # [nX][nL]
    nX, nL = OD.shape
    layers = np.arange(nL) if layers is None else np.asarray(layers)
    Z_s = np.array([Altitudes]).ravel()
    nZ = Z_s.size
    mu = 1.0 / np.cos(theta_r)
    B, dB = _planck_dT(X, T)
    S = np.concatenate([np.zeros((nX, 1)), np.cumsum(OD, axis=1)], axis=1)  # S[:, j] = sum_{i<j} OD_i
    t = np.exp(-mu * OD)
    Lr = np.zeros((nX, nL + 1))  # Lr[:, l] = L^(l-1)
    for k in range(nL):
        Lr[:, k + 1] = t[:, k] * Lr[:, k] + (1 - t[:, k]) * B[:, k]
    masks = [Z <= zs for zs in Z_s]
    n_down = int(masks[-1].sum())
    g = np.zeros((2 * nZ + 1, nX, layers.size))
    h = np.zeros_like(g)
    for a, m in enumerate(masks):
        cnt = int(m.sum())
        tau_a = np.exp(-mu * np.sum(OD[:, m], axis=1))
        for c, l in enumerate(layers):
            if m[l]:
                g[a, :, c] = mu if returnOD else -mu * tau_a
            if l < cnt:
                Q = np.exp(-mu * (S[:, cnt] - S[:, l + 1]))
                g[nZ + a, :, c] = mu * t[:, l] * Q * (B[:, l] - Lr[:, l])
                h[nZ + a, :, c] = (1 - t[:, l]) * Q * dB[:, l]
    angles = np.linspace(0, np.pi / 2.0, N_angle, endpoint=False)
    w = np.cos(angles) * np.sin(angles)
    w = w / w.sum()
    for q in range(1, N_angle):
        cq = np.cos(angles[q])
        tq = np.exp(-OD / cq)
        R = np.zeros((nX, nL + 1))  # R[:, l] = radiance arriving at the top of layer l - 1 from above (R_l)
        for k in range(n_down - 1, -1, -1):
            R[:, k] = tq[:, k] * R[:, k + 1] + (1 - tq[:, k]) * B[:, k]
        for c, l in enumerate(layers):
            if l < n_down:
                g[2 * nZ, :, c] += (w[q] / cq) * np.exp(-S[:, l + 1] / cq) * (B[:, l] - R[:, l + 1])
                h[2 * nZ, :, c] += w[q] * (1 - tq[:, l]) * np.exp(-S[:, l] / cq) * dB[:, l]
    return g, h


def _rows(X, OD, T, Z, alts, returnOD):
    tau, Lu, Ld = cpu_ref.tud_from_od(X, OD, T, Z, Altitudes=alts, theta_r=0.0, N_angle=30, returnOD=returnOD)
    return np.concatenate([tau.reshape(X.size, -1).T, Lu.reshape(X.size, -1).T, Ld[None, :]])


def _richardson(d, e):
    """Central difference with one Richardson step: truncation O(e^4)."""
    return (4.0 * d(0.5 * e) - d(e)) / 3.0


@pytest.mark.parametrize("returnOD", [False, True])
def test_sensitivity_formulas_match_oracle_finite_differences(returnOD):
    rng = np.random.default_rng(7)
    nX, nL = 6, 12
    X = np.linspace(700.0, 1400.0, nX)
    # thin, moderate and opaque layers; a non-monotonic height so that a tau mask is not a prefix
    OD = np.exp(rng.uniform(np.log(1e-4), np.log(3.0), (nX, nL)))
    T = np.linspace(290.0, 215.0, nL) + rng.uniform(-3, 3, nL)
    Z = np.arange(nL, dtype=np.float64)
    Z[3], Z[4] = Z[4], Z[3]
    alts = np.array([3.5, 6.0, 11.0])
    layers = np.array([0, 1, 3, 4, 7, 11])
    g, h = jacobian_from_od(X, OD, T, Z, alts, returnOD=returnOD, layers=layers)
    for c, l in enumerate(layers):
        def d_od(e):
            Op, Om = OD.copy(), OD.copy()
            Op[:, l] += e
            Om[:, l] -= e
            return (_rows(X, Op, T, Z, alts, returnOD) - _rows(X, Om, T, Z, alts, returnOD)) / (2 * e)

        # at fixed OD the rows are linear in B_l: their change over a wide temperature step divided by B's change is
        # d row / d B_l up to rounding alone; times dB/dT from a (Richardson) difference of the oracle's planckian
        Tp, Tm = T.copy(), T.copy()
        Tp[l] += 20.0
        Tm[l] -= 20.0
        dB = cpu_ref.planckian(X, Tp[l]) - cpu_ref.planckian(X, Tm[l])
        d_row_dB = (_rows(X, OD, Tp, Z, alts, returnOD) - _rows(X, OD, Tm, Z, alts, returnOD)) / dB[None, :]
        dBdT = _richardson(lambda e: (cpu_ref.planckian(X, T[l] + e) - cpu_ref.planckian(X, T[l] - e)) / (2 * e), 0.2)
        fdT = d_row_dB * dBdT[None, :]
        fd = _richardson(d_od, 2e-3)  # steps large enough that rounding stays below 1e-8 of the smallest row
        for r in range(fd.shape[0]):
            assert rel_err(g[r, :, c], fd[r]) <= 1e-8, ("OD", l, r)
            assert rel_err(h[r, :, c], fdT[r]) <= 1e-8, ("T", l, r)
    # structural zeros: L-up of the lowest altitude (count 4) above its count, Ld above the last altitude's count
    assert np.all(g[3, :, 4:] == 0) and np.all(h[3, :, 4:] == 0)
