"""Every TUD and TUD-Jacobian kernel path against the fp64 oracle, at the shapes and edges the other GPU tests leave out.

a. rtx_tud_jacobian (engine.tud_jacobian_from_od) on synthetic float32 columns against the oracle's closed form
   (cpu_ref.jacobian_from_od, pinned to finite differences by tests/test_jacobian_host.py) evaluated in fp64 on the same
   float32 inputs: no line-sum noise, so every row is held to TOL_L. Slant paths, 1..95 streams around the 8-stream
   groups, 1..128 layers and requested layers across the 8-layer chunks, 1..16 altitudes (below the surface, last one
   inside the column, non-ascending heights), returnOD, T first / in the middle / absent, optical depths from 1e-9 to 1e4
   per column with zeros, slightly negative values, isothermal runs and inversions, padded leading dimensions.
b. rt.compute_TUD_jacobian end to end from line tables, against the closed form driven by oracle line-sums.
c. The angle-summed TUD kernels without Planck nodes (grids coarser than rtx_tud's node criterion), and the coarsest grid
   that still uses them.
d. The stream kernel (per_angle / save) at every register width, column in LDS (<= 36 layers) and chunked.
e. rtx_tud at its limits: 128 layers x 16 altitudes x 8 slants.

Values below F32_FLOOR are outside what fp32 products of the kernels' factors represent and are compared absolutely.
Four configurations of (a) do not meet TOL_L; each is bounded at about 3x its measured worst error, never above 1e-4
(JAC_CASES). The source: the kernel carries D_l = B_l - L^(l-1) and E_l,q = B_l - R_l+1,q as fp32 recurrences driven by
fp64 differences of B. Their rounding is ~6e-8 of B. Where the radiance arriving at a layer nearly equals its Planck
value, D or E is 1e-3 of B or less, and that rounding becomes 1e-5 to 1e-4 of the value. The oracle forms the same
differences in fp64. Measured worst: 9.6e-5 (37 layers, 16 altitudes), 2.7e-5 (66 layers), 8.6e-5 (128 layers, 16
altitudes), 1.2e-5 (128 layers, one stream). Each sits at a wavenumber whose value is 1e-4 to 4e-3 of the row's
largest, and the same error shows in every altitude's L-up row of that layer (one D_l)."""
import numpy as np
import pytest

from oracle import cpu_ref as ref
from radtxfr_amd import synthetic

pytestmark = pytest.mark.gpu

TOL_L = 1e-5
TOL_TAU = 2e-6
F32_FLOOR = 1e-30  # |J| values under this are fp32 products of flushed / denormal factors: compared absolutely
TOL_SPECIES, TOL_T, LINESUM_REL = 2e-4, 2e-3, 2e-6  # end to end (b): as tests/test_gpu_jacobian.py
H_T = 0.5  # engine default fd_step_T [K]


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    from radtxfr_amd import _lib, engine
    _lib.load()
    return engine


def _rel(got, want, floor_abs=F32_FLOOR):
    """rel_err (max |got - want| / max(|want|, 1e-3 max|want|)) with an absolute floor."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    mx = float(np.max(np.abs(want))) if want.size else 0.0
    den = np.maximum(np.maximum(np.abs(want), 1e-3 * mx), floor_abs)
    return float(np.max(np.abs(got - want) / den))


def _planck_nodes(grid, T):
    """rtx_tud.hip's choice of the Planck-node (parabola) instantiations: (4/nu_lo + 100 c2 / T_min) 63 step <= 7e-3."""
    return grid.xmin > 0.0 and (4.0 / grid.xmin + ref.C2 * 100.0 / float(np.min(T))) * 63.0 * grid.step <= 7e-3


def _columns(rng, nL, n, lo_exp=-9.0, hi_exp=4.0):
    """OD [nL][n] float32: column totals 10^U(lo_exp, hi_exp) spread very unevenly over the layers, exact zeros in a few
    columns and one layer, slightly negative depths (a caller's rounding noise) in one column."""
    tot = 10.0 ** rng.uniform(lo_exp, hi_exp, n)
    prof = rng.dirichlet(np.full(nL, 0.3), size=n).T
    OD = np.ascontiguousarray(tot[None, :] * prof, dtype=np.float32)
    if n > 4:
        OD[:, rng.integers(0, n, max(1, n // 50))] = 0.0
        OD[:, 1] = (-1e-7 * rng.uniform(0, 1, nL)).astype(np.float32)
    if nL > 3:
        OD[nL // 2] = 0.0
    return OD


def _temperatures(rng, nL):
    """Decreasing with height, an inversion and an isothermal run (B differences exactly 0)."""
    T = np.linspace(295.0, 200.0, nL) + rng.uniform(-2.0, 2.0, nL)
    if nL >= 8:
        T[nL // 4:nL // 4 + 3] = np.linspace(240.0, 262.0, 3)  # inversion
        T[nL // 2:nL // 2 + max(2, nL // 5)] = 216.65  # isothermal
    return T


# ------------------------------------------------------------------------------------------------ a. the kernel itself
def _jac_trial(eng, rng, nL, n, theta, nA, alts, Z, wrt, layers, returnOD, lo=700.0, pad=0, nan_at=None, tol=TOL_L):
    import torch
    T = _temperatures(rng, nL)
    grid = eng.Grid(lo, lo + 1.5, n) if n > 1 else eng.Grid(lo, lo + 1.5, 64).shard(37, 1)  # a one-point shard
    X = grid.axis()
    OD = _columns(rng, nL, n)
    if nan_at is not None:
        OD[nan_at] = np.nan
    # dOD/dT: OD+ and OD- within a factor 2 of each other, so their fp32 difference is exact; 2 h = 1 K -> 1/(2h) = 1
    r = rng.uniform(0.0, 0.02, (nL, n)).astype(np.float32)
    ODp = OD * (1.0 + r)
    ODm = OD * (1.0 - r)
    n_spec = sum(1 for w in wrt if w != "T")
    K = (10.0 ** rng.uniform(-3.0, 1.0, (n_spec, nL, 1)) * rng.uniform(0.0, 1.0, (n_spec, nL, n))).astype(np.float32)
    alts = np.atleast_1d(np.asarray(alts, dtype=np.float64))
    mu = 1.0 / np.cos(theta)
    with np.errstate(invalid="ignore", over="ignore"):
        tau64 = np.stack([np.exp(-mu * OD.astype(np.float64)[Z <= zs].sum(axis=0)) for zs in alts])
    tau32 = tau64.astype(np.float32)
    ld = n + pad

    def dev(a):  # padded leading dimension, padding NaN: must not leak
        a = np.asarray(a, dtype=np.float32)
        b = np.full(a.shape[:-1] + (ld,), np.nan, dtype=np.float32)
        b[..., :n] = a
        return torch.as_tensor(b, device="cuda")[..., :n]

    with_T = "T" in wrt
    t_pos = wrt.index("T") if with_T else 0
    J = eng.tud_jacobian_from_od(dev(OD), dev(ODp) if with_T else None, dev(ODm) if with_T else None, H_T,
                                 dev(K) if n_spec else None, None if returnOD else dev(tau32), grid, T, Z, Altitudes=alts,
                                 theta_r=theta, N_angle=nA, returnOD=returnOD, layers=layers, t_pos=t_pos)
    J = J.double().cpu().numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        g, h = ref.jacobian_from_od(X, OD.astype(np.float64).T, T, Z, alts, theta_r=theta, N_angle=nA, returnOD=returnOD,
                                    layers=np.asarray(layers))
    if nan_at is not None:
        return J
    nZ = alts.size
    counts = [int((Z <= zs).sum()) for zs in alts]
    if not returnOD:  # the tau slot's factor -mu tau takes the tau the kernel is given (float32 of the same value)
        for a_, zs in enumerate(alts):
            for c, l in enumerate(layers):
                if Z[l] <= zs:
                    g[a_, :, c] = -mu * tau32[a_].astype(np.float64)
    d_T = (ODp.astype(np.float64) - ODm.astype(np.float64)) / (2.0 * H_T)
    K64 = K.astype(np.float64)
    worst = 0.0
    s = 0
    for w, name in enumerate(wrt):
        for c, l in enumerate(layers):
            d = d_T[l] if name == "T" else K64[s, l]
            want = g[:, :, c] * d[None, :] + (h[:, :, c] if name == "T" else 0.0)
            got = J[w, c]
            tag = (nL, n, theta, nA, nZ, returnOD, wrt, name, int(l))
            # structural zeros are exact: tau outside the mask, L-up at or above the count, Ld at or above n_down
            for a_, zs in enumerate(alts):
                if not Z[l] <= zs:
                    assert np.all(got[a_] == 0.0), tag + ("tau", a_)
                if l >= counts[a_]:
                    assert np.all(got[nZ + a_] == 0.0), tag + ("Lu", a_)
            if nA == 1:
                assert np.isnan(got[2 * nZ]).all(), tag
                rows = range(2 * nZ)
            else:
                if l >= counts[-1]:
                    assert np.all(got[2 * nZ] == 0.0), tag
                rows = range(2 * nZ + 1)
            for r_ in rows:
                e = _rel(got[r_], want[r_])
                worst = max(worst, e)
                assert e <= tol, (r_, e) + tag
        if name != "T":
            s += 1
    return worst


JAC_CASES = [
    # nL, n, theta, N_angle, altitudes, Z kind, wrt, layers, returnOD, pad, tolerance (see the module docstring)
    (1, 1, 0.0, 2, [0.5], "asc", ("T",), [0], False, 0, TOL_L),
    (8, 63, 0.3, 8, [-1.0, 3.5], "asc", (1, "T", 2), [7, 0, 3, 3], True, 0, TOL_L),
    (9, 257, 1.1, 9, [2.5, 8.0, 4.0], "asc", (1, 2), [8, 7, 6, 5, 4, 3, 2, 1, 0], False, 0, TOL_L),
    (37, 3000, 0.0, 10, "16", "shuffled", ("T", 1), list(range(0, 37, 4)) + [17], False, 0, 1e-4),
    (66, 257, 0.3, 17, [5.0, 30.0, 12.0, -2.0, 50.0], "asc", (1, "T"), [0, 3, 7, 8, 9, 15, 16, 40, 65, 16], True, 37, 8e-5),
    (128, 1024, 1.1, 30, "16", "asc", ("T",), list(range(0, 128, 3)) + [127], False, 0, 1e-4),
    (37, 63, 0.3, 96, [7.0, 20.0], "shuffled", (3, "T"), [36, 0, 9, 8, 18], False, 5, TOL_L),
    (12, 257, 0.0, 1, [3.0, 7.5], "shuffled", ("T", 1), [0, 5, 11], False, 0, TOL_L),
    (128, 63, 0.0, 2, [200.0], "asc", (1,), [127, 0, 64, 8, 7], True, 0, 3.5e-5),
]


@pytest.mark.parametrize("case", range(len(JAC_CASES)))
def test_tud_jacobian_kernel_vs_closed_form(eng, case):
    nL, n, theta, nA, alts, zkind, wrt, layers, returnOD, pad, tol = JAC_CASES[case]
    rng = np.random.default_rng(20261016 + case)
    Z = np.sort(rng.uniform(0.0, 60.0, nL)) if nL > 1 else np.array([0.2])
    if zkind == "shuffled":
        Z = rng.permutation(Z)
    if alts == "16":  # 16 altitudes: below the surface, inside, above the top, not in order
        alts = rng.permutation(np.concatenate([[-1.0], rng.uniform(0.0, 60.0, 14), [70.0]]))
    worst = _jac_trial(eng, rng, nL, n, theta, nA, alts, Z, wrt, layers, returnOD, pad=pad, tol=tol)
    print("jacobian case %d: worst rel_err %.3g" % (case, worst))


def test_tud_jacobian_nan_stays_in_its_column(eng):
    rng = np.random.default_rng(5)
    nL, n = 20, 257
    Z = np.sort(rng.uniform(0.0, 30.0, nL))
    col = 100
    J = _jac_trial(eng, rng, nL, n, 0.3, 9, [10.0, 40.0], Z, ("T", 1), list(range(nL)), False, nan_at=(7, col))
    assert np.isnan(J[..., col]).any()
    assert not np.isnan(np.delete(J, col, axis=-1)).any()


# ------------------------------------------------------------------------------------- b. compute_TUD_jacobian end to end
def _std_layers():
    A = synthetic.load_standard_atmosphere()
    rows = np.array([0, 2, 5, 9, 14, 20, 28, 36, 45, 55, 65])  # up to 100 km: Doppler-dominated layers at the top
    return dict(Zs=A[rows, 1], Ts=A[rows, 5].copy(), Ps=A[rows, 4], PLs=A[rows, 3], MFs_VAL=A[rows, 6:9] * 1e6 * 1e-2,
                MFs_ID=np.array([1, 2, 3]))


E2E_CASES = [
    # lo, hi, DVOUT, theta, N_angle, altitudes, returnOD, wrt
    (1000.0, 1001.0, 0.001, 0.6, 9, [0.5, 30.0], False, ("T", 1, 2)),
    (700.0, 702.0, 0.004, 0.0, 17, [1.0, 100.0], True, (2, "T")),
    (500.0, 502.0, 0.01, 1.0, 30, [12.0], False, ("T", 1)),
]


@pytest.mark.parametrize("case", range(len(E2E_CASES)))
def test_compute_tud_jacobian_vs_oracle_line_sums(case):
    import torch
    assert torch.cuda.is_available()
    from radtxfr_amd import radiative_transfer as rt
    lo, hi, dv, theta, nA, alts, returnOD, wrt = E2E_CASES[case]
    full = synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)
    sub = synthetic.subset_table(full, lo - 12.0, hi + 12.0)
    a = _std_layers()
    alts = np.asarray(alts)
    X, tau, Lu, Ld, J = rt.compute_TUD_jacobian(lo, hi, wrt=wrt, DVOUT=dv, line_table=sub, Altitudes=alts, theta_r=theta,
                                                N_angle=nA, returnOD=returnOD, **a)
    Xr = ref.make_spectral_axis(lo, hi, dv)
    assert np.array_equal(X, Xr)
    nL = a["Ts"].size
    OD = np.stack([ref.layer_od(sub, X, a["Ts"][l], a["Ps"][l], a["PLs"][l], a["MFs_VAL"][l], a["MFs_ID"]) for l in range(nL)], 1)
    g, h = ref.jacobian_from_od(X, OD, a["Ts"], a["Zs"], alts, theta_r=theta, N_angle=nA, returnOD=returnOD)
    nZ = alts.size
    for w in wrt:
        dJ = np.concatenate([J[w][0].reshape(X.size, nZ, nL), J[w][1].reshape(X.size, nZ, nL), J[w][2][:, None, :]], 1)
        for l in range(nL):
            if w == "T":
                d = np.zeros(X.size)
                for sgn in (1.0, -1.0):
                    d += sgn * ref.od_fixed_window(sub, X, a["Ts"][l] + sgn * H_T, a["Ts"][l], a["Ps"][l], a["PLs"][l],
                                                   a["MFs_VAL"][l], a["MFs_ID"]) / (2.0 * H_T)
                # the engine's dOD/dT is a difference of two float32 line-sums: LINESUM_REL of the layer's largest OD over
                # 2 h, times the row's factor g, is the floor of what it resolves
                noise = LINESUM_REL * float(np.max(OD[:, l])) / (2.0 * H_T)
                tol = TOL_T
            else:
                unit = np.zeros(3)
                unit[list(a["MFs_ID"]).index(w)] = 1.0
                d = ref.layer_od(sub, X, a["Ts"][l], a["Ps"][l], a["PLs"][l], unit, a["MFs_ID"])
                noise, tol = 0.0, TOL_SPECIES
            want = g[:, :, l] * d[None, :] + (h[:, :, l] if w == "T" else 0.0)
            for r_ in range(2 * nZ + 1):
                floor = max(F32_FLOOR, 2.0 * noise * float(np.max(np.abs(g[r_, :, l]))) / tol)
                e = _rel(dJ[:, r_, l], want[r_], floor_abs=floor)
                assert e <= tol, (case, w, l, r_, e)


# ------------------------------------------------------------------------------- c. TUD without Planck nodes (PN = false)
def _tud_vs_oracle(eng, OD, grid, T, Z, alts, theta, nA=30, returnOD=False, per_angle=False):
    import torch
    X = grid.axis()
    res = eng.tud(torch.as_tensor(OD, device="cuda"), grid, T, Z, Altitudes=alts, theta_r=theta, N_angle=nA,
                  returnOD=returnOD, per_angle=per_angle)
    tau, Lu, Ld, (nZ, nMu) = res[:4]
    tr, ur, dr = ref.tud_from_od(X, OD.astype(np.float64).T, T, Z, Altitudes=alts, theta_r=theta, N_angle=nA,
                                 returnOD=returnOD)
    tau_h = tau.double().cpu().numpy().reshape(nZ, nMu, -1).transpose(2, 0, 1).reshape(np.shape(tr))
    Lu_h = Lu.double().cpu().numpy().reshape(nZ, nMu, -1).transpose(2, 0, 1).reshape(np.shape(ur))
    tag = (grid.n, T.size, np.size(alts), np.size(theta), nA, returnOD, per_angle)
    if returnOD:
        assert _rel(tau_h, tr) <= TOL_L, tag
    else:
        assert np.max(np.abs(tau_h - tr)) <= TOL_TAU, tag
    assert _rel(Lu_h, ur) <= TOL_L, tag
    assert _rel(Ld.double().cpu().numpy(), dr) <= TOL_L, tag
    return res


PN_CONFIGS = ["one", "ascending", "slants", "shuffled"]


def _pn_case(rng, kind, nL=24):
    Z = np.sort(rng.uniform(0.0, 40.0, nL))
    alts, theta = [500.0], 0.0
    if kind != "one":
        alts = np.sort(rng.uniform(2.0, 45.0, 4))
    if kind == "slants":
        theta = np.array([0.0, 0.4, 0.9])
    if kind == "shuffled":
        Z = rng.permutation(Z)
    return Z, np.asarray(alts), theta


@pytest.mark.parametrize("kind", PN_CONFIGS)
def test_tud_without_planck_nodes_vs_oracle(eng, kind):
    """Steps of 0.01..0.05 cm^-1 from 500 cm^-1 select the kernels that evaluate B per wavenumber (PN = false); the coarsest
    step that still selects the parabola through three nodes per wave (its worst case) is held to the same tolerances."""
    rng = np.random.default_rng(11 + PN_CONFIGS.index(kind))
    nL = 24
    T = _temperatures(rng, nL)
    T[3] = 190.0  # T_min: the criterion's worst temperature
    Z, alts, theta = _pn_case(rng, kind, nL)
    lo = 500.0
    coarsest = 7e-3 / (63.0 * (4.0 / lo + ref.C2 * 100.0 / 190.0))
    for step, nodes in ((0.01, False), (0.05, False), (coarsest * (1.0 - 1e-6), True)):
        n = 300
        grid = eng.Grid(lo, lo + step * (n - 1), n)
        assert _planck_nodes(grid, T) == nodes, (step, grid.step)
        OD = _columns(rng, nL, n, -4.0, 1.5)
        _tud_vs_oracle(eng, OD, grid, T, Z, alts, theta)


def test_compute_tud_coarse_grid_vs_oracle():
    import torch
    assert torch.cuda.is_available()
    from radtxfr_amd import engine
    from radtxfr_amd import radiative_transfer as rt
    full = synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)
    lo, hi = 500.0, 504.0
    sub = synthetic.subset_table(full, lo - 12.0, hi + 12.0)
    a = synthetic.c3_atmosphere(16)
    a["MFs_VAL"] = a["MFs_VAL"] * 1e-3
    X, tau, Lu, Ld = rt.compute_TUD(lo, hi, DVOUT=0.01, line_table=sub, **a)
    assert not _planck_nodes(engine.Grid(lo, hi, X.size), a["Ts"])
    Xr, tau_r, Lu_r, Ld_r = ref.compute_TUD(sub, lo, hi, 0.01, a["Zs"], a["Ts"], a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"])
    assert np.array_equal(X, Xr)
    assert tau_r.max() - tau_r.min() > 0.3
    assert np.max(np.abs(tau - tau_r)) <= TOL_TAU and _rel(Lu, Lu_r) <= TOL_L and _rel(Ld, Ld_r) <= TOL_L


# ------------------------------------------------------------------------------------- d. the stream kernel at every width
@pytest.mark.parametrize("nL", [36, 37])
def test_stream_kernel_every_width_vs_oracle(eng, nL):
    """per_angle=True runs the stream kernel with N_angle streams (theta = 0 included): widths 4, 8, 16, 24, 29 and blocks
    of 32, each at both ends of its range; 36 layers keep the column in LDS, 37 stream it in chunks."""
    rng = np.random.default_rng(40 + nL)
    n = 256
    grid = eng.Grid(900.0, 901.0, n)
    X = grid.axis()
    T = _temperatures(rng, nL)
    Z = np.sort(rng.uniform(0.0, 50.0, nL))
    B = ref.planckian(X, T)
    for i, nA in enumerate((3, 4, 5, 8, 9, 16, 17, 24, 25, 29, 30, 31, 96)):
        OD = _columns(rng, nL, n, -6.0, 2.5)
        alts = np.array([Z[nL // 3], Z[-5]]) if i % 2 else np.array([70.0])
        theta = 0.5 if i % 3 == 1 else 0.0
        res = _tud_vs_oracle(eng, OD, grid, T, Z, alts, theta, nA=nA, returnOD=bool(i % 4 == 3), per_angle=True)
        Ld_ang = res[4].double().cpu().numpy()
        assert Ld_ang.shape == (nA, n)
        nd = int((Z <= alts[-1]).sum())
        for q in range(nA):
            sec = 1.0 / np.cos(q * (np.pi / 2) / nA)
            Lq = np.zeros(n)
            for j in range(nd - 1, -1, -1):
                t = np.exp(-OD[j].astype(np.float64) * sec)
                Lq = t * Lq + (1.0 - t) * B[:, j]
            assert _rel(Ld_ang[q], Lq) <= TOL_L, (nL, nA, q)


def test_compute_tud_save_20_angles_vs_oracle(tmp_path, monkeypatch):
    import torch
    assert torch.cuda.is_available()
    from radtxfr_amd import radiative_transfer as rt
    full = synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)
    lo, hi = 1000.0, 1001.0
    sub = synthetic.subset_table(full, lo - 12.0, hi + 12.0)
    a = synthetic.c3_atmosphere(12)
    a["MFs_VAL"] = a["MFs_VAL"] * 1e-3
    monkeypatch.chdir(tmp_path)
    alts = np.array([0.5, 3.0])
    X, tau, Lu, Ld = rt.compute_TUD(lo, hi, DVOUT=0.001, line_table=sub, save=True, N_angle=20, Altitudes=alts, **a)
    d = np.load(tmp_path / "ComputeTUD.npz")
    Xr, tau_r, Lu_r, Ld_r, OD = ref.compute_TUD(sub, lo, hi, 0.001, a["Zs"], a["Ts"], a["Ps"], a["PLs"], a["MFs_VAL"],
                                                a["MFs_ID"], Altitudes=alts, N_angle=20, return_layers=True)
    assert np.max(np.abs(tau - tau_r)) <= TOL_TAU and _rel(Lu, Lu_r) <= TOL_L and _rel(Ld, Ld_r) <= TOL_L
    assert d["Ld"].shape == (X.size, 20)
    B = ref.planckian(X, a["Ts"])
    nd = int((a["Zs"] <= alts[-1]).sum())
    for q in range(20):
        sec = 1.0 / np.cos(q * (np.pi / 2) / 20)
        Lq = np.zeros(X.size)
        for j in range(nd - 1, -1, -1):
            t = np.exp(-OD[:, j] * sec)
            Lq = t * Lq + (1.0 - t) * B[:, j]
        assert _rel(d["Ld"][:, q], Lq) <= TOL_L, q


# ------------------------------------------------------------------------------------------------------------ e. limits
@pytest.mark.parametrize("kind", ["ascending_8_slants", "shuffled_8_slants", "ascending_1_slant"])
def test_tud_at_its_limits_vs_oracle(eng, kind):
    """128 layers x 16 altitudes x 8 slants (128 altitude-slant pairs): snapshots of one recurrence per slant (ascending
    heights), pairs in blocks (shuffled), and the single-slant snapshot form."""
    rng = np.random.default_rng(128 + len(kind))
    nL, n = 128, 384
    grid = eng.Grid(1100.0, 1100.5, n)
    assert _planck_nodes(grid, np.full(nL, 190.0))
    T = _temperatures(rng, nL)
    Z = np.sort(rng.uniform(0.0, 100.0, nL))
    if kind.startswith("shuffled"):
        Z = rng.permutation(Z)
    alts = np.concatenate([[-1.0], np.sort(rng.uniform(0.0, 100.0, 14)), [120.0]])
    theta = np.linspace(0.0, 1.2, 8) if kind.endswith("8_slants") else 0.4
    OD = _columns(rng, nL, n, -7.0, 2.0)
    _tud_vs_oracle(eng, OD, grid, T, Z, alts, theta, nA=30, returnOD=False)
