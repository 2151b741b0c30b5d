"""Inputs and fp64 reference contractions for the tests of the TUD adjoint (rtx_tud_vjp); no test in here.

The synthetic float32 columns are those of tests/test_gpu_tud_paths.py (its _columns and _temperatures generators, copied:
test files are not imported from). Everything is NumPy; the GPU tests upload what `make` returns."""
import numpy as np

H_T = 0.5  # fd_step_T [K]: 2 h = 1 K, so (OD+ - OD-) / 2h is exact in fp32
DEG40 = np.deg2rad(40.0)


def columns(rng, nL, n, lo_exp=-9.0, hi_exp=4.0):
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


def temperatures(rng, nL):
    """Decreasing with height, an inversion and an isothermal run (B differences exactly 0)."""
    T = np.linspace(295.0, 200.0, nL) + rng.uniform(-2.0, 2.0, nL)
    if nL >= 8:
        T[nL // 4:nL // 4 + 3] = np.linspace(240.0, 262.0, 3)  # inversion
        T[nL // 2:nL // 2 + max(2, nL // 5)] = 216.65  # isothermal
    return T


def altitudes(rng, Z, n_alt):
    """n_alt sensor altitudes, not in order, one below the surface and one above the top when there is room; the LAST one
    inside the column (between two layers), so that n_down < nL wherever the column has more than one layer."""
    nL = Z.size
    Zs = np.sort(Z)
    last = 0.5 * (Zs[(2 * nL) // 3 - 1] + Zs[(2 * nL) // 3]) if nL > 1 else Zs[0] + 0.3
    if n_alt == 1:
        return np.array([last])
    rest = rng.uniform(Zs[0], Zs[-1] + 1.0, n_alt - 1)
    rest[0] = Zs[-1] + 10.0
    if n_alt > 2:
        rest[1] = Zs[0] - 1.0
    return np.concatenate([rng.permutation(rest), [last]])


# nL, n, theta, N_angle, n_alt, wrt, layers, returnOD, pad, n_vec, vs_oracle
# n: wave (64) and workgroup (256) edges, several partials, a one-point shard; layers: scrambled, repeated, across the
# 8-layer chunk; n_vec: 1, 3 and one more than a launch takes (4); T first, in the middle, absent.
# vs_oracle: the configurations on which the stored Jacobian itself is within TOL_L of the fp64 oracle (asserted by the
# test that uses the flag): not the 37-layer, 16-altitude kind tests/test_gpu_tud_paths.py documents as an exception, and
# not the last one, whose stored J is 9e-5 off at one wavenumber (the same fp32 D_l recurrence that test file describes).
CASES = [
    (1, 1, 0.0, 2, 1, ("T",), [0], False, 0, 1, True),
    (7, 63, DEG40, 9, 3, (1, "T", 2), [6, 0, 3, 3, 5], True, 0, 3, True),
    (8, 64, 0.0, 30, 1, (1, 2), [7, 6, 5, 4, 3, 2, 1, 0], False, 5, 5, True),
    (9, 65, DEG40, 2, 16, ("T", 1), [8, 0, 7, 1, 6, 2, 5, 3, 4], False, 0, 1, True),
    (37, 255, 0.0, 9, 3, ("T",), [36, 0, 9, 8, 18, 7, 30, 1, 24, 23, 2, 17], True, 37, 3, True),
    (37, 257, DEG40, 30, 16, (3, "T"), [5, 36, 8, 7, 22, 0, 9, 16, 31, 12], False, 0, 5, False),
    (9, 1000, 0.0, 9, 3, (1, "T", 2), [4, 8, 0, 7, 1, 3, 2, 6, 5], False, 24, 3, False),
]


def make(case, seed=20261019):
    """Everything one configuration needs, as NumPy arrays (float32 where the device takes float32)."""
    nL, n, theta, nA, n_alt, wrt, layers, returnOD, pad, n_vec, vs_oracle = CASES[case] if isinstance(case, int) else case
    rng = np.random.default_rng(seed + (case if isinstance(case, int) else 0))
    Z = np.sort(rng.uniform(0.0, 60.0, nL)) if nL > 1 else np.array([0.2])
    alts = altitudes(rng, Z, n_alt)
    T = temperatures(rng, nL)
    OD = columns(rng, nL, n)
    r = rng.uniform(0.0, 0.02, (nL, n)).astype(np.float32)
    ODp, ODm = OD * (1.0 + r), OD * (1.0 - r)  # within a factor 2 of each other: their fp32 difference is exact
    n_spec = sum(1 for w in wrt if w != "T")
    K = (10.0 ** rng.uniform(-3.0, 1.0, (n_spec, nL, 1)) * rng.uniform(0.0, 1.0, (n_spec, nL, n))).astype(np.float32)
    mu = 1.0 / np.cos(theta)
    with np.errstate(over="ignore"):
        tau32 = np.stack([np.exp(-mu * OD.astype(np.float64)[Z <= zs].sum(axis=0)) for zs in alts]).astype(np.float32)
    # cotangents of mixed sign and very different sizes per row; whole rows and whole wavenumber ranges exactly zero
    G = (rng.normal(size=(n_vec, 2 * n_alt + 1, n)) * 10.0 ** rng.uniform(-2.0, 2.0, (n_vec, 2 * n_alt + 1, 1))).astype(np.float32)
    G[:, rng.integers(0, 2 * n_alt + 1)] = 0.0
    if n_vec > 1:
        G[1, :n_alt] = 0.0  # a vector without any tau cotangent
    if n > 8:
        G[..., n // 3:n // 2] = 0.0
    return dict(nL=nL, n=n, theta=theta, nA=nA, alts=alts, wrt=wrt, layers=list(layers), returnOD=returnOD, pad=pad,
                n_vec=n_vec, vs_oracle=vs_oracle, Z=Z, T=T, OD=OD, ODp=ODp, ODm=ODm, K=K, tau32=tau32, G=G, mu=mu,
                with_T="T" in wrt, t_pos=wrt.index("T") if "T" in wrt else 0, n_spec=n_spec)


def contract(G, J):
    """(sum G J, sum |G J|) over rows and wavenumbers in fp64: G [n_vec][rows][n], J [n_wrt][n_lay][rows][n] ->
    [n_vec][n_wrt][n_lay] each. The second is what the bound of a float32-stored J is stated in."""
    G = np.asarray(G, dtype=np.float64)
    J = np.asarray(J, dtype=np.float64)
    return np.einsum("vrn,wkrn->vwk", G, J), np.einsum("vrn,wkrn->vwk", np.abs(G), np.abs(J))


def oracle_jacobian(c, X, ref):
    """J [n_wrt][n_lay][rows][n] in fp64 from the oracle's closed form (cpu_ref.jacobian_from_od) on the same float32
    inputs, as tests/test_gpu_tud_paths.py forms it: the tau slot's factor takes the float32 tau the kernel is given."""
    layers = np.asarray(c["layers"])
    with np.errstate(invalid="ignore", over="ignore"):
        g, h = ref.jacobian_from_od(X, c["OD"].astype(np.float64).T, c["T"], c["Z"], c["alts"], theta_r=c["theta"],
                                    N_angle=c["nA"], returnOD=c["returnOD"], layers=layers)
    if not c["returnOD"]:
        for a_, zs in enumerate(c["alts"]):
            for k, l in enumerate(layers):
                if c["Z"][l] <= zs:
                    g[a_, :, k] = -c["mu"] * c["tau32"][a_].astype(np.float64)
    d_T = (c["ODp"].astype(np.float64) - c["ODm"].astype(np.float64)) / (2.0 * H_T)
    K64 = c["K"].astype(np.float64)
    J = np.zeros((len(c["wrt"]), layers.size, g.shape[0], X.size))
    s = 0
    for w, name in enumerate(c["wrt"]):
        for k, l in enumerate(layers):
            d = d_T[l] if name == "T" else K64[s, l]
            J[w, k] = g[:, :, k] * d[None, :] + (h[:, :, k] if name == "T" else 0.0)
        if name != "T":
            s += 1
    return J
