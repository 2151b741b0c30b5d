"""The fp64 NumPy definition of the analytic temperature derivative of the Voigt line-sum and the cases
the tests of rtx_line_prep_dt / rtx_voigt_sum_dt share. No tests here. Written against the oracle's own pieces --
cpu_ref.line_params, cpu_ref.hum1_wei, cpu_ref.PYTIPS, cpu_ref.linesum_records -- and nothing of the package's.

Per line and point, with the line's window taken at T and not differentiated, g = A K(x, y), A = w S(T) cte / sqrt(pi),
cte = sqrt(ln 2) / GammaD, x = (nu - nu0 - Shift0) cte, y = Gamma0 cte, K + iL = hum1_wei(x, y):

  dg/dT = A [alpha K + K_x x' + K_y y'],  x' = -Shift0' cte - x / (2T),  y' = Gamma0' cte - y / (2T)  (GammaD ~ sqrt T),
  alpha = dln(qratio w)/dT + c2 E"/T^2 - (u/T) e^-u / (1 - e^-u) - 1/(2T),  u = c2 nu0 / T,
  Gamma0' = -sum_d f_d gamma_d p (Tref/T)^n_d n_d / T,  Shift0' = sum_d f_d deltap_d p,
  |x| + y < 15:  K_x = -2 (x K - y L),  K_y = 2 (x L + y K) - 2/sqrt(pi)            (w' = -2 z w + 2i/sqrt(pi))
  elsewhere, t = y - ix:  K_y + i K_x = (1/2 - t^2) / (sqrt(pi) (1/2 + t^2)^2)      (d/dt of hum1_wei's far form)."""
import bisect

import numpy as np

from oracle import cpu_ref as ref
from radtxfr_amd import synthetic

import linesum_cases as LC

TIPS_NODES = np.arange(60.0, 3011.0, 25.0)
DQ_STEP = 1e-3


def dlnq_dT(M, I, T):
    """d ln(Q(Tref)/Q(T)) / dT = -Q'/Q by a central difference of the oracle's PYTIPS: T must keep clear of the table's
    nodes (the interpolant changes stencil there and the difference would straddle two polynomials)."""
    assert np.min(np.abs(TIPS_NODES - T)) > 2 * DQ_STEP, T
    return -(np.log(ref.PYTIPS(M, I, T + DQ_STEP)) - np.log(ref.PYTIPS(M, I, T - DQ_STEP))) / (2 * DQ_STEP)


def w_and_dw(x, y):
    """K, L = hum1_wei(x, y) and K_x, K_y: every point differentiates the branch it is on."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64) + np.zeros_like(x)
    K, L = ref.hum1_wei(x, y)
    near = np.abs(x) + y < 15.0
    z = x + 1j * y
    dw = -2 * z * (K + 1j * L) + 2j / np.sqrt(np.pi)
    t = y - 1j * x
    dwdt = (0.5 - t * t) / (np.sqrt(np.pi) * (0.5 + t * t) ** 2)
    Kx = np.where(near, dw.real, dwdt.imag)
    Ky = np.where(near, -dw.imag, dwdt.real)
    return K, L, Kx, Ky


def _col(tbl, name, n, default=None):
    if name in tbl:
        return np.asarray(tbl[name], dtype=np.float64)
    return np.zeros(n) if default is None else np.asarray(tbl[default], dtype=np.float64)


def line_terms(sub, T, p, dil_air=1.0, dil_self=0.0):
    """Per line of `sub` at (T, p): line_params' dict plus cte, y, alpha0 (alpha without dln(qratio w)/dT), dG0 = Gamma0',
    dS0 = Shift0'."""
    dil = {}
    if dil_air != 0.0:
        dil["air"] = dil_air
    if dil_self != 0.0:
        dil["self"] = dil_self
    P = dict(ref.line_params(sub, T, p, Diluent=dil))
    nu = np.asarray(sub["nu"], dtype=np.float64)
    n = nu.size
    el = np.asarray(sub["elower"], dtype=np.float64)
    n_air = np.asarray(sub["n_air"], dtype=np.float64)
    dG0, dS0 = np.zeros(n), np.zeros(n)
    for sp, f in dil.items():
        g = _col(sub, "gamma_" + sp, n)
        npow = _col(sub, "n_" + sp, n, default="n_air").copy()
        if sp == "self":
            npow[npow == 0.0] = n_air[npow == 0.0]
        dG0 += -f * (g * p * (ref.TREF / T) ** npow) * npow / T
        dS0 += f * _col(sub, "deltap_" + sp, n) * p
    u = ref.HAPI_C2 * nu / T
    P["alpha0"] = ref.HAPI_C2 * el / T ** 2 - (u / T) * np.exp(-u) / (1.0 - np.exp(-u)) - 0.5 / T
    P["dG0"], P["dS0"] = dG0, dS0
    P["cte"] = np.sqrt(np.log(2.0)) / P["GammaD"]
    P["y"] = P["Gamma0"] * P["cte"]
    return P


def line_dT(P, r, Xw, T, A, dlnsw):
    """(dg/dT, g) of line r of line_terms' dict on the points Xw, with strength prefactor A = w S cte / sqrt(pi)."""
    cte, y = P["cte"][r], P["y"][r]
    x = (Xw - (np.asarray(P["nu0"])[r] + P["Shift0"][r])) * cte
    K, L, Kx, Ky = w_and_dw(x, y)
    xp = -P["dS0"][r] * cte - x / (2 * T)
    yp = P["dG0"][r] * cte - y / (2 * T)
    alpha = dlnsw + P["alpha0"][r]
    return A * (alpha * K + Kx * xp + Ky * yp), A * K


def shard_axis(g):
    """The shard's wavenumbers as the device forms them: (offset + i) step + xmin, the grid's last point pinned to xmax."""
    xmin, xmax, n_total, offset, n = g
    step = (xmax - xmin) / (n_total - 1)
    X = np.arange(offset, offset + n, dtype=np.float64) * step + xmin
    if n and offset + n == n_total:
        X[-1] = xmax
    return X


def by_species(v, key):
    return float(v[key]) if isinstance(v, dict) else float(v)


def linesum_dT(tbl, g, T, p, weight=1.0, dlnw_dT=0.0, ow=0.0, hw=50.0, dil_air=1.0, dil_self=0.0):
    """What rtx_line_prep_dt + rtx_voigt_sum_dt define for one layer on the shard g = (xmin, xmax, n_total, offset, n):
    (d sum / dT, sum, R). Windows are the device's (cpu_ref.linesum_records). weight, dlnw_dT: a scalar or {(M, I): value};
    dln(qratio)/dT comes from dlnq_dT. R is linesum_records' dict, with "y64" added."""
    dil = {k: v for k, v in (("air", dil_air), ("self", dil_self)) if v != 0.0}
    R = ref.linesum_records(tbl, g, T, p, omega_wing=ow, omega_wing_hw=hw, Diluent=dil)
    sub = {k: np.asarray(v)[R["order"]] for k, v in tbl.items()}
    P = line_terms(sub, T, p, dil_air, dil_self)
    P["nu0"] = np.asarray(sub["nu"], dtype=np.float64)
    X = shard_axis(g)
    d, s = np.zeros(X.size), np.zeros(X.size)
    dq = {}
    for r in range(P["nu0"].size):
        lo, hi = int(R["lo"][r]), int(R["hi"][r])
        key = (int(P["M"][r]), int(P["I"][r]))
        w = by_species(weight, key)
        if hi <= lo or w == 0.0:
            continue
        if key not in dq:
            dq[key] = dlnq_dT(key[0], key[1], T)
        A = w * P["S"][r] * P["cte"][r] / np.sqrt(np.pi)
        dg, gg = line_dT(P, r, X[lo:hi], T, A, dq[key] + by_species(dlnw_dT, key))
        d[lo:hi] += dg
        s[lo:hi] += gg
    R["y64"] = P["y"]
    return d, s, R


def sum_fixed_window(tbl, g, T, T_win, p, weight=1.0, ow=0.0, hw=50.0, dil_air=1.0, dil_self=0.0):
    """The line-sum at (T, p) with every line's window taken at T_win: what linesum_dT differentiates (weight: a scalar or
    {(M, I): value}, held fixed). The oracle's own pieces: line_params with the diluent mix, PROFILE_VOIGT."""
    dil = {k: v for k, v in (("air", dil_air), ("self", dil_self)) if v != 0.0}
    R = ref.linesum_records(tbl, g, T_win, p, omega_wing=ow, omega_wing_hw=hw, Diluent=dil)
    sub = {k: np.asarray(v)[R["order"]] for k, v in tbl.items()}
    P = ref.line_params(sub, T, p, Diluent=dil)
    nu = np.asarray(sub["nu"], dtype=np.float64)
    X = shard_axis(g)
    s = np.zeros(X.size)
    for r in range(nu.size):
        lo, hi = int(R["lo"][r]), int(R["hi"][r])
        w = by_species(weight, (int(P["M"][r]), int(P["I"][r])))
        if hi > lo and w != 0.0:
            s[lo:hi] += w * P["S"][r] * ref.PROFILE_VOIGT(nu[r] + P["Shift0"][r], P["GammaD"][r], P["Gamma0"][r], X[lo:hi])[0]
    return s


def dod_dT(tbl, X, T, P_pa, PL_km, MF_VAL, MF_ID):
    """d/dT of cpu_ref.od_fixed_window(tbl, X, T', T, ...) at T' = T: the layer's optical depth with every line's window
    [bisect(X, nu - W), bisect(X, nu + W)) taken at T and held. The weight volumeConcentration(p, T) ppmv PL ~ 1/T."""
    p = float(P_pa) / 101325.0
    X = np.asarray(X, dtype=np.float64)
    glist = X.tolist()
    out = np.zeros(X.size)
    Mall = np.asarray(tbl["molec_id"]).astype(int)
    for m, ppmv in zip(np.asarray(MF_ID).tolist(), np.asarray(MF_VAL).tolist()):
        keep = Mall == m
        if not keep.any():
            continue
        sub = {k: np.asarray(v)[keep] for k, v in tbl.items()}
        P = line_terms(sub, T, p)
        P["nu0"] = np.asarray(sub["nu"], dtype=np.float64)
        dq = {mi: dlnq_dT(mi[0], mi[1], T) for mi in set(zip(P["M"].tolist(), P["I"].tolist()))}
        w = ref.volumeConcentration(p, T) * (ppmv * 1e-6) * PL_km * 1e5
        for r in range(P["nu0"].size):
            W = max(0.0, 50.0 * P["Gamma0"][r], 50.0 * P["GammaD"][r])
            lo, hi = bisect.bisect(glist, P["nu0"][r] - W), bisect.bisect(glist, P["nu0"][r] + W)
            if hi <= lo:
                continue
            A = w * P["S"][r] * P["cte"][r] / np.sqrt(np.pi)
            out[lo:hi] += line_dT(P, r, X[lo:hi], T, A, dq[(int(P["M"][r]), int(P["I"][r]))] - 1.0 / T)[0]
    return out


# ---- the column of tests/test_gpu_jacobian.py ------------------------------------------------------------------------
LO, HI, DV = 1000.0, 1004.0, 0.0005


def jacobian_column():
    """(line table, spectral axis) of test_gpu_jacobian.py's case: 1000-1004 cm^-1 at 0.0005, the C3 table's 494 lines."""
    full = synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)
    return synthetic.subset_table(full, LO - 12.0, HI + 12.0), ref.make_spectral_axis(LO, HI, DV)


def standard_atmosphere():
    sa = synthetic.load_standard_atmosphere()
    return dict(Zs=sa[:, 1], Ts=sa[:, 5].copy(), Ps=sa[:, 4], PLs=sa[:, 3], MFs_VAL=sa[:, 6:9] * 1e6, MFs_ID=np.array([1, 2, 3]))


def shifted_self_table():
    """The column's table with a temperature-dependent shift, a self width with its own exponent (and a zero exponent
    that falls back to n_air) on every line: Shift0' and the self term of Gamma0' are exercised."""
    tbl, X = jacobian_column()
    tbl = {k: np.array(v, copy=True) for k, v in tbl.items()}
    n = np.asarray(tbl["nu"]).size
    rng = np.random.default_rng(5)
    tbl["deltap_air"] = rng.uniform(-2e-5, 2e-5, n)
    tbl["gamma_self"] = rng.uniform(0.1, 0.5, n)
    ns = rng.uniform(0.3, 0.9, n)
    ns[::7] = 0.0
    tbl["n_self"] = ns
    return tbl, X


# ---- kernel cases (tests/test_gpu_linesum_dT.py) ----------------------------------------------------------------------
def _two_species(tbl, second):
    """Lines `second` (indices) become CO2 (2, 1)."""
    tbl = dict(tbl)
    M = np.array(tbl["molec_id"], copy=True)
    M[np.asarray(second)] = 2
    tbl["molec_id"] = M
    return tbl


def kernel_case(n_total, n_layers):
    """A table and layers for a shard of n_total points (step 1e-3 from 1000 cm^-1; one point: the first of a two-point
    grid) that put every regime of voigt_dT_kernel on it; regimes() counts them. Layers: 1 atm / 296.3 K (gamma_air 0.02:
    y ~ 11, 0.009: y ~ 5, 0.0035: y ~ 2, 0.07: no band), 0.02 atm / 220.4 K (y < 1, windows of ~65 points inside the
    grid), 0.3 atm / 251.7 K. Lines: seven centres spread over the grid; one 0.9 cm^-1 left of the grid and one as far
    right of it (windows of 1.5 cm^-1 at 1 atm that reach ~600 points in and end mid-row); one 200 cm^-1 away (empty
    window); a second species, with a weight and a dlnw of its own, on every third line; a third species with weight 0."""
    step = 1e-3
    n_tot = max(n_total, 2)
    g = (1000.0, 1000.0 + (n_tot - 1) * step, n_tot, 0, n_total)
    span = (n_tot - 1) * step
    inside = 1000.0 + span * np.array([0.07, 0.21, 0.38, 0.52, 0.66, 0.81, 0.93]) + 0.25 * step
    nus = np.concatenate([inside, [1000.0 - 0.9, 1000.0 + span + 0.9, 1200.0]])
    gam = np.array([0.02, 0.009, 0.0035, 0.07, 0.009, 0.02, 0.03, 0.03, 0.03, 0.07])
    tbl = LC.table(nus, gam, sw=1e-20)
    n = nus.size
    rng = np.random.default_rng(3)
    tbl["elower"] = rng.uniform(50.0, 2500.0, n)
    tbl["n_air"] = rng.uniform(0.4, 0.8, n)
    tbl["deltap_air"] = rng.uniform(-2e-5, 2e-5, n)
    tbl["delta_air"] = rng.uniform(-5e-3, 5e-3, n)
    tbl = _two_species(tbl, np.arange(1, n, 3))
    M = np.array(tbl["molec_id"], copy=True)
    M[6] = 6  # CH4: weight 0
    tbl["molec_id"] = M
    T = np.array([296.3, 220.4, 251.7])[:n_layers]
    p = np.array([1.0, 0.02, 0.3])[:n_layers]
    weight = {(1, 1): 1.0, (2, 1): 0.37, (6, 1): 0.0}
    dlnw = {(1, 1): -1.0 / 250.0, (2, 1): 2.5e-3, (6, 1): 0.0}
    return dict(tbl=tbl, grid=g, T=T, p=p, weight=weight, dlnw=dlnw)


def regimes(R, g, weight_of_line):
    """Counts, from one layer's records, of what voigt_dT_kernel meets: lines (with weight) by y class that have band
    points on the shard, lanes at the |x| + y = 15 switch inside a band row, windows cut by the shard's first / last
    tile from outside, windows ending mid-row, empty windows."""
    n = g[4]
    live = (R["hi"] > R["lo"]) & (weight_of_line != 0.0)
    y = R["y64"]
    band_on = live & (R["zw"] > 0) & (R["i0"] + R["zw"] >= 0) & (R["i0"] - R["zw"] < n)
    out = {"y_ge_6": int(np.sum(band_on & (y >= 6.0))), "y_1_6": int(np.sum(band_on & (y >= 1.0) & (y < 6.0))),
           "y_lt_1": int(np.sum(band_on & (y < 1.0))), "empty": int(np.sum(R["hi"] <= R["lo"])),
           "centre_left": int(np.sum(live & (R["gi0"] < 0))), "centre_right": int(np.sum(live & (R["gi0"] >= g[2]))),
           "ends_mid_row": int(np.sum(live & (R["hi"] < n) & (R["hi"] % 64 != 0))), "switch_in_row": 0}
    X = shard_axis(g)
    for r in np.nonzero(band_on)[0]:
        lo, hi = int(R["lo"][r]), int(R["hi"][r])
        s = np.abs((X[lo:hi] - R["sg0"][r]) * R["cte"][r]) + y[r] < 15.0
        flips = np.nonzero(s[1:] != s[:-1])[0] + lo + 1  # first index of the new branch
        out["switch_in_row"] += int(np.sum(flips % 64 != 0))
    return out
