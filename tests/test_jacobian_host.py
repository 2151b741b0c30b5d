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
jacobian_from_od = cpu_ref.jacobian_from_od  # the closed forms rtx_tud_jacobian evaluates


def _rows(X, OD, T, Z, alts, returnOD, theta_r=0.0, N_angle=30):
    tau, Lu, Ld = cpu_ref.tud_from_od(X, OD, T, Z, Altitudes=alts, theta_r=theta_r, N_angle=N_angle, returnOD=returnOD)
    return np.concatenate([tau.reshape(X.size, -1).T, Lu.reshape(X.size, -1).T, Ld[None, :]])


def _richardson(d, e):
    """Central difference with one Richardson step: truncation O(e^4)."""
    return (4.0 * d(0.5 * e) - d(e)) / 3.0


def _column():
    rng = np.random.default_rng(7)
    nX, nL = 6, 12
    X = np.linspace(700.0, 1400.0, nX)
    # thin, moderate and opaque layers; a non-monotonic height so that a tau mask is not a prefix
    OD = np.exp(rng.uniform(np.log(1e-4), np.log(3.0), (nX, nL)))
    T = np.linspace(290.0, 215.0, nL) + rng.uniform(-3, 3, nL)
    T[6:10] = 221.5  # an isothermal run: B_l - B_l+1 = 0 exactly, where the differences the kernel carries would cancel
    Z = np.arange(nL, dtype=np.float64)
    Z[3], Z[4] = Z[4], Z[3]
    return X, OD, T, Z


# altitude sets: the last one at the top of the column (n_down = nL); the last one inside it (n_down = 7) with one below
# the surface (count 0) before it; the last one below the surface (n_down = 0: no downwelling at all)
ALT_SETS = {"top": np.array([3.5, 6.0, 11.0]), "inside": np.array([11.0, -1.0, 6.0]), "below": np.array([3.5, -0.5])}


@pytest.mark.parametrize("alts", list(ALT_SETS))
@pytest.mark.parametrize("N_angle", [2, 9, 30])
@pytest.mark.parametrize("theta_r", [0.0, 0.7])
@pytest.mark.parametrize("returnOD", [False, True])
def test_sensitivity_formulas_match_oracle_finite_differences(returnOD, theta_r, N_angle, alts):
    X, OD, T, Z = _column()
    alts = ALT_SETS[alts]
    nZ = alts.size
    layers = np.array([0, 1, 3, 4, 7, 8, 11])
    g, h = jacobian_from_od(X, OD, T, Z, alts, theta_r=theta_r, N_angle=N_angle, returnOD=returnOD, layers=layers)
    rows = lambda O, T_: _rows(X, O, T_, Z, alts, returnOD, theta_r, N_angle)
    for c, l in enumerate(layers):
        def d_od(e):
            Op, Om = OD.copy(), OD.copy()
            Op[:, l] += e
            Om[:, l] -= e
            return (rows(Op, T) - rows(Om, T)) / (2 * e)

        # at fixed OD the rows are linear in B_l: their change over a wide temperature step divided by B's change is
        # d row / d B_l up to rounding alone; times dB/dT from a (Richardson) difference of the oracle's planckian
        Tp, Tm = T.copy(), T.copy()
        Tp[l] += 20.0
        Tm[l] -= 20.0
        dB = cpu_ref.planckian(X, Tp[l]) - cpu_ref.planckian(X, Tm[l])
        d_row_dB = (rows(OD, Tp) - rows(OD, Tm)) / dB[None, :]
        dBdT = _richardson(lambda e: (cpu_ref.planckian(X, T[l] + e) - cpu_ref.planckian(X, T[l] - e)) / (2 * e), 0.2)
        fdT = d_row_dB * dBdT[None, :]
        fd = _richardson(d_od, 2e-3)  # steps large enough that rounding stays below 1e-8 of the smallest row
        for r in range(fd.shape[0]):
            assert rel_err(g[r, :, c], fd[r]) <= 1e-8, ("OD", l, r)
            assert rel_err(h[r, :, c], fdT[r]) <= 1e-8, ("T", l, r)
    # structural zeros: tau outside an altitude's mask, L-up at or above its count, Ld at or above the last one's count
    counts = [int((Z <= zs).sum()) for zs in alts]
    for c, l in enumerate(layers):
        for a, zs in enumerate(alts):
            if not Z[l] <= zs:
                assert np.all(g[a, :, c] == 0) and np.all(h[a, :, c] == 0)
            if l >= counts[a]:
                assert np.all(g[nZ + a, :, c] == 0) and np.all(h[nZ + a, :, c] == 0)
        if l >= counts[-1]:
            assert np.all(g[2 * nZ, :, c] == 0) and np.all(h[2 * nZ, :, c] == 0)
    if nZ == 3 and counts[0] == 4:  # L-up of the lowest altitude (count 4) above its count
        assert np.all(g[3, :, 4:] == 0) and np.all(h[3, :, 4:] == 0)


@pytest.mark.parametrize("theta_r", [0.0, 0.7])
def test_single_angle_downwelling_derivatives_are_nan(theta_r):
    """N_angle = 1: the oracle's Ld is 0/0 (theta = 0 carries weight 0), and so is any difference of it: the closed form's
    Ld rows are NaN too, every other row is unaffected."""
    X, OD, T, Z = _column()
    alts = ALT_SETS["inside"]
    nZ = alts.size
    layers = np.array([0, 5, 11])
    with np.errstate(invalid="ignore"):
        g, h = jacobian_from_od(X, OD, T, Z, alts, theta_r=theta_r, N_angle=1, layers=layers)
        g30, h30 = jacobian_from_od(X, OD, T, Z, alts, theta_r=theta_r, N_angle=30, layers=layers)
        for l in layers:
            Op, Om = OD.copy(), OD.copy()
            Op[:, l] += 1e-3
            Om[:, l] -= 1e-3
            fd = (_rows(X, Op, T, Z, alts, False, theta_r, 1) - _rows(X, Om, T, Z, alts, False, theta_r, 1)) / 2e-3
            assert np.isnan(fd[2 * nZ]).all() and not np.isnan(fd[:2 * nZ]).any()
    assert np.isnan(g[2 * nZ]).all() and np.isnan(h[2 * nZ]).all()
    assert np.array_equal(g[:2 * nZ], g30[:2 * nZ]) and np.array_equal(h[:2 * nZ], h30[:2 * nZ])
