"""CPU oracle: fp64 NumPy restatement of the reference's LWIR hot path.

*** TEST INFRASTRUCTURE -- NOT PRODUCT CODE. ***
Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this
module, and only as the checker. The product path (radtxfr_amd/) never imports it and
fails loudly when the HIP library is missing.

Parity pin: the reference has no tests or golden vectors of its own, so this
restatement is pinned by golden vectors captured from the imported reference
(oracle/make_golden.py -> tests/golden/*.npz; checked by tests/test_oracle_golden.py to
~1e-13 relative).

All citations are file:line under the upstream reference checkout.
"""
import bisect as _bisect
import os

import numpy as np

# ---------------------------------------------------------------------------------------
# radiative_transfer.py constants (:71-72)
C1 = 1.19104295315e-16  # [J m^2 / s]
C2 = 1.43877736830e-02  # [m K]

# misc/hapi.py constants (:84-92, :10171, :11085)
CBOLTS = 1.380648813e-16  # erg/K
CC = 2.99792458e10  # cm/s
CMASSMOL = 1.66053873e-27
HAPI_C2 = 1.4388028496642257  # cm K   (EnvironmentDependency_Intensity)
TREF = 296.0
PREF = 1.0

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "radtxfr_amd", "data")
_tips = None


def _tables():
    global _tips
    if _tips is None:
        d = np.load(os.path.join(_DATA, "tips2011.npz"))
        _tips = {
            "tdat": d["tdat"].astype(np.float64),
            "q": {tuple(k): d["q"][r] for r, k in enumerate(d["mi"].tolist())},  # float32 rows
            "abun": {tuple(k): float(v) for k, v in zip(d["iso_mi"].tolist(), d["iso_abun"])},
            "mass": {tuple(k): float(v) for k, v in zip(d["iso_mi"].tolist(), d["iso_mass"])},
        }
    return _tips


# ---------------------------------------------------------------------------------------
# Planck / spectral axis                      radiative_transfer.py:251-271, 792-848
def make_spectral_axis(Xmin, Xmax, DVOUT):
    """:269-270 with the float->int crash fixed: spacing is (Xmax-Xmin)/(nX-1)."""
    nX = int(np.ceil((Xmax - Xmin) / DVOUT))
    return np.linspace(Xmin, Xmax, nX)


def planckian(X_in, T_in, wavelength=False):
    """radiative_transfer.py:792-848.  Output (X.size, *T.shape), uW/(cm^2 sr cm^-1)."""
    X = np.asarray(np.copy(X_in), dtype=np.float64).flatten()
    T = np.asarray(np.copy(T_in), dtype=np.float64)
    X = X[:, np.newaxis]
    dimsT = T.shape
    T = T.flatten()[np.newaxis, :]
    if wavelength or np.mean(X) < 50:
        X = X * 1e-6
        L = C1 / (X ** 5 * (np.exp(C2 / (X * T)) - 1))
        L *= 1e-4
    else:
        X = X * 100
        L = C1 * X ** 3 / (np.exp(C2 * X / T) - 1)
        L *= 1e4
    return np.reshape(L, (X.size, *dimsT))


def brightnessTemperature(X_in, L_in, wavelength=False, bad_value=np.nan, spectral_dim=0):
    """radiative_transfer.py:851-933 (section 8f 'next' row 1)."""
    X = np.asarray(np.copy(X_in), dtype=np.float64).flatten()
    L = np.asarray(np.copy(L_in), dtype=np.float64)
    if spectral_dim != 0:
        L = np.swapaxes(L, 0, spectral_dim)
    X = X[:, np.newaxis]
    if L.ndim == 1:
        L = L[:, np.newaxis]
        dimsL = L.shape
    else:
        dimsL = L.shape
        L = L.reshape((dimsL[0], int(np.prod(dimsL[1:]))))
    with np.errstate(all="ignore"):
        if wavelength or np.mean(X) < 50:
            X = X * 1e-6
            L = L * 1e4
            T = C2 / (X * np.log(1 + C1 / (X ** 5 * L)))
        else:
            X = X * 100
            L = L * 1e-4
            T = C2 * X / np.log(C1 * X ** 3 / L + 1)
    ixBad = ~np.isfinite(L) | (L <= 0)
    T[ixBad] = bad_value
    if [*dimsL[1:]] != [1]:
        T = np.reshape(T, (X.size, *dimsL[1:]))
    if spectral_dim != 0:
        T = np.swapaxes(T, 0, spectral_dim)
    return T


def BT2L(X_in, T_in, wavelength=False, bad_value=np.nan, spectral_dim=0):
    """radiative_transfer.py:936-1014 (section 8f 'next' row 1)."""
    X = np.asarray(np.copy(X_in), dtype=np.float64).flatten()
    T = np.asarray(np.copy(T_in), dtype=np.float64)
    if spectral_dim != 0:
        T = np.swapaxes(T, 0, spectral_dim)
    X = X[:, np.newaxis]
    if T.ndim == 1:
        T = T[:, np.newaxis]
        dimsT = T.shape
    else:
        dimsT = T.shape
        T = T.reshape((dimsT[0], int(np.prod(dimsT[1:]))))
    with np.errstate(all="ignore"):
        if wavelength or np.mean(X) < 50:
            X = X * 1e-6
            L = C1 / (X ** 5 * (np.exp(C2 / (X * T)) - 1))
            L *= 1e-4
        else:
            X = X * 100
            L = C1 * X ** 3 / (np.exp(C2 * X / T) - 1)
            L *= 1e4
    ixBad = ~np.isfinite(L) | (T <= 0)
    L[ixBad] = bad_value
    L = np.reshape(L, (X.size, *dimsT[1:]))
    if spectral_dim != 0:
        L = np.swapaxes(L, 0, spectral_dim)
    return L


# ---------------------------------------------------------------------------------------
# TUD integration                                   radiative_transfer.py:340-392
def tud_from_od(X, OD, T, Z, Altitudes=(500,), theta_r=0.0, N_angle=30, returnOD=False):
    """Body of compute_TUD after the per-layer OD loop (:340-392), quirks 3-6 reproduced:
    nL is overwritten by the LAST altitude's layer count and reused by the downwelling loop;
    tau uses the Z<=zs mask, L-up uses the first count(mask) layers; theta=0 carries weight 0."""
    X = np.asarray(X, dtype=np.float64)
    OD = np.asarray(OD, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    Z = np.asarray(Z, dtype=np.float64)
    nL = T.size
    nA = int(N_angle)
    f = lambda x: np.array([x]).ravel()
    Z_s = f(Altitudes)
    mu_s = f(1.0 / np.cos(theta_r))
    Lu_ = np.zeros((X.size, Z_s.size, mu_s.size))
    Ld_ = np.zeros((X.size, nA))
    tau_ = Lu_.copy()
    B = planckian(X, T)
    for ii, zs in enumerate(Z_s):
        for jj, mu in enumerate(mu_s):
            ix = Z <= zs
            if returnOD:
                tau_[:, ii, jj] = np.sum(OD[:, ix] * mu, axis=1)
            else:
                tau_[:, ii, jj] = np.exp(-1.0 * np.sum(OD[:, ix] * mu, axis=1))
            nL = int(np.sum(ix))
            for kk in range(nL):
                t = np.exp(-OD[:, kk] * mu)
                Lu_[:, ii, jj] = t * Lu_[:, ii, jj] + (1 - t) * B[:, kk]
    if (len(Z_s) == 1) and (len(mu_s) == 1):
        tau_ = tau_[:, 0, 0]
        Lu_ = Lu_[:, 0, 0]
    if (len(Z_s) == 1) and not (len(mu_s) == 1):
        tau_ = tau_[:, 0, :]
        Lu_ = Lu_[:, 0, :]
    if not (len(Z_s) == 1) and (len(mu_s) == 1):
        tau_ = tau_[:, :, 0]
        Lu_ = Lu_[:, :, 0]
    angles = np.linspace(0, np.pi / 2.0, nA, endpoint=False)
    for ii, th in enumerate(angles):
        for jj in np.arange(nL)[::-1]:
            t = np.exp(-OD[:, jj] / np.cos(th))
            Ld_[:, ii] = t * Ld_[:, ii] + (1 - t) * B[:, jj]
    cos_dOmega = np.cos(angles) * np.sin(angles)
    Ld_ = np.sum(Ld_ * cos_dOmega, axis=1) / np.sum(cos_dOmega)
    return tau_, Lu_, Ld_.flatten()


def compute_LWIR_apparent_radiance(X, emis, Ts, tau, La, Ld, dT=None, return_Ls=False):
    """radiative_transfer.py:1017-1069. Dtype-agnostic like the reference (callers feed fp32)."""
    if dT is not None:
        T_ = Ts.flatten()[:, np.newaxis] + np.asarray(dT).flatten()[np.newaxis, :]
        B_ = planckian(X, T_)[:, np.newaxis, :, :]
        tau_ = tau[:, np.newaxis, :, np.newaxis]
        La_ = La[:, np.newaxis, :, np.newaxis]
        Ld_ = Ld[:, np.newaxis, :, np.newaxis]
        em_ = emis[:, :, np.newaxis, np.newaxis]
    else:
        T_ = Ts.flatten()
        B_ = planckian(X, T_)[:, np.newaxis, :]
        tau_ = tau[:, np.newaxis, :]
        La_ = La[:, np.newaxis, :]
        Ld_ = Ld[:, np.newaxis, :]
        em_ = emis[:, :, np.newaxis]
    if return_Ls:
        Ls = em_ * B_ + (1 - em_) * Ld_
        L = tau_ * Ls + La_
        return L, Ls
    return tau_ * (em_ * B_ + (1 - em_) * Ld_) + La_


# ---------------------------------------------------------------------------------------
# MAKO instrument line shape         radiative_transfer.py:1072-1263, ILS_MAKO.py:2-35
# 128 MAKO band centres [um] (instrument constants; :1092-1223)
MAKO_UM = np.array([
    7.5711, 7.6158, 7.6606, 7.7053, 7.7500, 7.7947, 7.8394, 7.8841, 7.9288, 7.9734, 8.0181, 8.0627,
    8.1073, 8.1519, 8.1965, 8.2411, 8.2857, 8.3303, 8.3748, 8.4194, 8.4639, 8.5084, 8.5529, 8.5974,
    8.6419, 8.6863, 8.7308, 8.7752, 8.8197, 8.8641, 8.9085, 8.9529, 8.9973, 9.0417, 9.0860, 9.1304,
    9.1747, 9.2190, 9.2633, 9.3076, 9.3519, 9.3962, 9.4405, 9.4847, 9.5290, 9.5732, 9.6174, 9.6616,
    9.7058, 9.7500, 9.7942, 9.8383, 9.8825, 9.9266, 9.9707, 10.0148, 10.0589, 10.1030, 10.1471,
    10.1912, 10.2352, 10.2792, 10.3233, 10.3673, 10.4113, 10.4553, 10.4993, 10.5432, 10.5872,
    10.6311, 10.6751, 10.7190, 10.7629, 10.8068, 10.8507, 10.8945, 10.9384, 10.9822, 11.0261,
    11.0699, 11.1137, 11.1575, 11.2013, 11.2451, 11.2888, 11.3326, 11.3763, 11.4201, 11.4638,
    11.5075, 11.5512, 11.5948, 11.6385, 11.6822, 11.7258, 11.7694, 11.8131, 11.8567, 11.9003,
    11.9439, 11.9874, 12.0310, 12.0745, 12.1181, 12.1616, 12.2051, 12.2486, 12.2921, 12.3356,
    12.3791, 12.4225, 12.4660, 12.5094, 12.5528, 12.5962, 12.6396, 12.6830, 12.7264, 12.7697,
    12.8131, 12.8564, 12.8997, 12.9430, 12.9863, 13.0296, 13.0729, 13.1162, 13.1594])


def mako_band_axis(X, resFactor=None, clip=True):
    """Band centres in cm^-1: :1226-1233 (triangle variant clips to the open (X.min, X.max))."""
    X_out = MAKO_UM.copy()
    if resFactor is not None:
        _x0 = np.linspace(0, 1, len(X_out))
        _x1 = np.linspace(0, 1, int(len(X_out) * resFactor))
        X_out = np.interp(_x1, _x0, X_out)
    X_out = np.sort(10000.0 / X_out)
    if clip:
        X_out = X_out[(X_out > X.min()) & (X_out < X.max())]
    return X_out


def ILS_MAKO(X, Y, resFactor=None, returnX=True, fwhm_sf=1.0, shift=0.0, scale=1.0):
    """Triangle ILS, radiative_transfer.py:1072-1263. Banded evaluation (the reference's dense
    (nS,nX,nB) temporary is avoided; the sums are the same sums over the non-zero support)."""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y)
    X_out = mako_band_axis(X, resFactor, clip=True)
    sigma_out = fwhm_sf * np.abs(np.gradient(X_out)) * 1.6
    ctr = scale * X_out + shift
    Y2 = Y[:, None] if Y.ndim == 1 else Y
    Y_out = np.zeros((X_out.size, Y2.shape[1]))
    for b in range(X_out.size):
        # X ascending: support is the open interval |x-c| < s
        lo = np.searchsorted(X, ctr[b] - sigma_out[b], side="right")
        hi = np.searchsorted(X, ctr[b] + sigma_out[b], side="left")
        w = 1.0 - np.abs(X[lo:hi] - ctr[b]) / sigma_out[b]
        w[w < 0] = 0
        with np.errstate(all="ignore"):
            Y_out[b] = (w[:, None] * Y2[lo:hi]).sum(axis=0) / w.sum()
    if Y.ndim == 1:
        Y_out = Y_out[:, 0]
    if returnX:
        return X_out, Y_out
    return Y_out


def ILS_MAKO_gauss(X, Y):
    """Gaussian ILS, ILS_MAKO.py:2-35: sigma=|grad X_out| (no 1.6), no clipping, dense weights."""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y)
    X_out = mako_band_axis(X, None, clip=False)
    sigma_out = np.abs(np.gradient(X_out))
    Y2 = Y[:, None] if Y.ndim == 1 else Y
    Y_out = np.zeros((X_out.size, Y2.shape[1]))
    for b in range(X_out.size):
        g = np.exp(-0.5 * ((X - X_out[b]) / sigma_out[b]) ** 2) / (sigma_out[b] * np.sqrt(2.0 * np.pi))
        Y_out[b] = (g[:, None] * Y2).sum(axis=0) / g.sum()
    if Y.ndim == 1:
        Y_out = Y_out[:, 0]
    return X_out, Y_out


# ---------------------------------------------------------------------------------------
# hapi line-by-line chain
def AtoB(aa, A, B, npt):
    """Lagrange 3-/4-point interpolation, misc/hapi.py:5311-5388 (TIPS-2011 scheme)."""
    for I in range(2, npt + 1):
        if A[I - 1] >= aa:
            if I < 3 or I == npt:
                J = 3 if I < 3 else npt
                J -= 1
                a0, a1, a2 = A[J - 2], A[J - 1], A[J]
                A0 = (aa - a1) * (aa - a2) / ((a0 - a1) * (a0 - a2))
                A1 = (aa - a0) * (aa - a2) / ((a1 - a0) * (a1 - a2))
                A2 = (aa - a0) * (aa - a1) / ((a2 - a0) * (a2 - a1))
                return A0 * B[J - 2] + A1 * B[J - 1] + A2 * B[J]
            J = I - 1
            a0, a1, a2, a3 = A[J - 2], A[J - 1], A[J], A[J + 1]
            A0 = (aa - a1) * (aa - a2) * (aa - a3)
            A0 = A0 / ((a0 - a1) * (a0 - a2) * (a0 - a3))
            A1 = (aa - a0) * (aa - a2) * (aa - a3)
            A1 = A1 / ((a1 - a0) * (a1 - a2) * (a1 - a3))
            A2 = (aa - a0) * (aa - a1) * (aa - a3)
            A2 = A2 / ((a2 - a0) * (a2 - a1) * (a2 - a3))
            A3 = (aa - a0) * (aa - a1) * (aa - a2)
            A3 = A3 / ((a3 - a0) * (a3 - a1) * (a3 - a2))
            return A0 * B[J - 2] + A1 * B[J - 1] + A2 * B[J] + A3 * B[J + 1]
    raise ValueError("AtoB: aa above the last node")


def PYTIPS(M, I, T):
    """BD_TIPS_2011_PYTHON(M,I,T)[1], misc/hapi.py:9568-9582,10030."""
    if T < 70.0 or T > 3000.0:
        raise Exception("TIPS: T must be between 70K and 3000K.")
    t = _tables()
    try:
        q = t["q"][(int(M), int(I))]
    except KeyError:
        raise Exception("TIPS: no data for M,I = %d,%d." % (M, I))
    return AtoB(T, t["tdat"], q, t["tdat"].size)


def EnvironmentDependency_Intensity(S, T, Tref, SigmaT, SigmaTref, Elower, nu):
    """misc/hapi.py:10169-10175."""
    ch = np.exp(-HAPI_C2 * Elower / T) * (1 - np.exp(-HAPI_C2 * nu / T))
    zn = np.exp(-HAPI_C2 * Elower / Tref) * (1 - np.exp(-HAPI_C2 * nu / Tref))
    return S * SigmaTref / SigmaT * ch / zn


def volumeConcentration(p, T):
    """misc/hapi.py:10163-10164 (CGS, molecules/cm^3)."""
    return (p / 9.869233e-7) / (CBOLTS * T)


def weideman_coeffs(N=24):
    """Coefficients of Weideman's rational expansion (SIAM J. Numer. Anal. 31, 1994), as rebuilt
    per call by misc/hapi.py:9812-9824. polyval order (highest power first)."""
    M = 2 * N
    M2 = 2 * M
    k = np.arange(-M + 1, M)
    L = np.sqrt(N / np.sqrt(2))
    theta = k * np.pi / M
    t = L * np.tan(theta / 2)
    f = np.zeros(len(t) + 1)
    f[1:] = np.exp(-t ** 2) * (L ** 2 + t ** 2)
    a = np.real(np.fft.fft(np.fft.fftshift(f))) / M2
    return np.flipud(a[1:N + 1]), L


_W24, _L24 = weideman_coeffs(24)


def _wide(dtype):
    """(real type, complex type, pi, sqrt(ln 2)) of a dtype switch: float64 (the constants this module has always used) or
    longdouble (the same formulas in extended precision; every table value is the float64 one, widened)."""
    if np.dtype(dtype) == np.float64:
        return np.float64, np.complex128, np.pi, np.sqrt(np.log(2.0))
    if np.dtype(dtype) != np.dtype(np.longdouble):
        raise ValueError("dtype must be np.float64 or np.longdouble")
    L = np.longdouble
    return L, np.clongdouble, 4 * np.arctan(L(1)), np.sqrt(np.log(L(2)))


def hum1_wei(x, y, dtype=np.float64):
    """misc/hapi.py:9833-9844: Weideman-24 where |x|+y<15, else the 1-term asymptote."""
    F, _, pi, _ = _wide(dtype)
    x = np.asarray(x, dtype=F)
    y = np.asarray(y, dtype=F) + np.zeros_like(x)
    t = y - 1.0j * x
    cerf = 1 / np.sqrt(pi) * t / (0.5 + t ** 2)
    mask = abs(x) + y < 15.0
    if np.any(mask):
        z = x[mask] + 1.0j * y[mask]
        Z = (_L24 + 1.0j * z) / (_L24 - 1.0j * z)
        p = np.polyval(_W24 if F is np.float64 else _W24.astype(F), Z)
        w = 2 * p / (_L24 - 1.0j * z) ** 2 + (1 / np.sqrt(pi)) / (_L24 - 1.0j * z)
        np.place(cerf, mask, w)
    return cerf.real, cerf.imag


def PROFILE_VOIGT(sg0, GamD, Gam0, sg):
    """misc/hapi.py:10131-10140 -> pcqsdhc PART1 (:9900-9915) + common part (:10022):
    LS = (1/pi) * sqrt(pi)*cte*w(x+iy),  x=(sg-sg0)*cte, y=Gam0*cte, cte=sqrt(ln2)/GamD."""
    sg = np.asarray(sg, dtype=np.float64)
    cte = np.sqrt(np.log(2.0)) / GamD
    rpi = np.sqrt(np.pi)
    Z1 = (1.0j * (sg0 - sg) + complex(Gam0)) * cte
    WR1, WI1 = hum1_wei(-Z1.imag, Z1.real)
    A = rpi * cte * (WR1 + 1.0j * WI1)
    LS = (1.0 / np.pi) * (A / (1.0 - 0.0 * A))
    return LS.real, LS.imag


def line_params(tbl, T, p, Diluent=None, GammaL="gamma_air"):
    """Per-line environment dependences, misc/hapi.py:11068-11131 (vectorised over lines).
    Returns dict of arrays: S(T) (without abundance factors), GammaD, Gamma0, Shift0."""
    t = _tables()
    nu = np.asarray(tbl["nu"], dtype=np.float64)
    M = np.asarray(tbl["molec_id"]).astype(int)
    I = np.asarray(tbl["local_iso_id"]).astype(int)
    n = nu.size
    qT = {}
    qR = {}
    mass = np.zeros(n)
    SigmaT = np.zeros(n)
    SigmaR = np.zeros(n)
    for mi in sorted(set(zip(M.tolist(), I.tolist()))):
        qT[mi] = PYTIPS(mi[0], mi[1], T)
        qR[mi] = PYTIPS(mi[0], mi[1], TREF)
        sel = (M == mi[0]) & (I == mi[1])
        SigmaT[sel] = qT[mi]
        SigmaR[sel] = qR[mi]
        mass[sel] = t["mass"][mi]
    S = EnvironmentDependency_Intensity(np.asarray(tbl["sw"], dtype=np.float64), T, TREF, SigmaT, SigmaR,
                                        np.asarray(tbl["elower"], dtype=np.float64), nu)
    m = mass * CMASSMOL * 1000
    GammaD = np.sqrt(2 * CBOLTS * T * np.log(2) / m / CC ** 2) * nu
    if not Diluent:
        Diluent = {"air": 1.0} if GammaL.lower() == "gamma_air" else {"self": 1.0}
    Gamma0 = np.zeros(n)
    Shift0 = np.zeros(n)
    for species, abun in Diluent.items():
        sp = species.lower()
        g = np.asarray(tbl.get("gamma_" + sp, np.zeros(n)), dtype=np.float64)
        if "n_" + sp in tbl:
            npow = np.asarray(tbl["n_" + sp], dtype=np.float64).copy()
            if sp == "self":
                z = npow == 0.0
                npow[z] = np.asarray(tbl["n_air"], dtype=np.float64)[z]
        else:
            npow = np.asarray(tbl["n_air"], dtype=np.float64)
        Gamma0 = Gamma0 + abun * (g * p / PREF * (TREF / T) ** npow)
        d = np.asarray(tbl.get("delta_" + sp, np.zeros(n)), dtype=np.float64)
        dp = np.asarray(tbl.get("deltap_" + sp, np.zeros(n)), dtype=np.float64)
        Shift0 = Shift0 + abun * ((d + dp * (T - TREF)) * p / PREF)
    return {"S": S, "GammaD": GammaD, "Gamma0": Gamma0, "Shift0": Shift0, "M": M, "I": I}


def PROFILE_LORENTZ(sg0, Gam0, sg):
    """misc/hapi.py:10142-10150."""
    return Gam0 / (np.pi * (Gam0 ** 2 + (sg - sg0) ** 2))


def PROFILE_DOPPLER(sg0, GamD, sg):
    """misc/hapi.py:10152-10160 (cSqrtLn2divSqrtPi = sqrt(ln2/pi), cLn2 = ln2)."""
    return 0.469718639319144059835 * np.exp(-0.6931471805599 * ((sg - sg0) / GamD) ** 2) / GamD


def absorptionCoefficient_Lorentz(tbl, **kw):
    """misc/hapi.py:11144-11375: the Voigt loop with PROFILE_LORENTZ and OmegaWingF = max(OmegaWing, HW*Gamma0)."""
    return absorptionCoefficient_Voigt(tbl, _profile="lorentz", **kw)


def absorptionCoefficient_Doppler(tbl, LineShift=True, **kw):
    """misc/hapi.py:11384-11559: PROFILE_DOPPLER, GammaD from the function's own SI constants (:11534-11538),
    OmegaWingF = max(OmegaWing, HW*GammaD), Shift0 = delta_air*p/pref when LineShift (:11510-11513, 11543)."""
    return absorptionCoefficient_Voigt(tbl, _profile="doppler", _lineshift=LineShift, **kw)


def absorptionCoefficient_Voigt(tbl, Components=None, T=296.0, p=1.0, OmegaGrid=None, OmegaWing=0.0,
                                OmegaWingHW=50.0, HITRAN_units=True, GammaL="gamma_air", Diluent=None,
                                IntensityThreshold=0.0, _profile="voigt", _lineshift=True):
    """misc/hapi.py:10906-11141 on an explicit grid. `tbl` is the column dict of the line table
    (LOCAL_TABLE_CACHE[name]['data'], :438-463). Components: list of (M,I[,abundance]); None = every
    (M,I) in the table at natural abundance (:10237-10251). Returns (Omegas, Xsect)."""
    t = _tables()
    Omegas = np.sort(np.asarray(OmegaGrid, dtype=np.float64))
    Xsect = np.zeros(Omegas.size)
    Mcol = np.asarray(tbl["molec_id"]).astype(int)
    Icol = np.asarray(tbl["local_iso_id"]).astype(int)
    if Components is None:
        Components = sorted(set(zip(Mcol.tolist(), Icol.tolist())))
    ABUN, NAT = {}, {}
    for c in Components:
        mi = (int(c[0]), int(c[1]))
        if mi not in t["abun"]:
            raise Exception("cannot find component M,I = %d,%d." % mi)
        ABUN[mi] = c[2] if len(c) >= 3 else t["abun"][mi]
        NAT[mi] = t["abun"][mi]
    factor = 1.0 if HITRAN_units else volumeConcentration(p, T)
    keep = np.array([(m, i) in ABUN for m, i in zip(Mcol.tolist(), Icol.tolist())], dtype=bool)
    sub = {k: np.asarray(v)[keep] for k, v in tbl.items()}
    if sub["nu"].size == 0:
        return Omegas, Xsect
    P = line_params(sub, T, p, Diluent=Diluent, GammaL=GammaL)
    nu = np.asarray(sub["nu"], dtype=np.float64)
    glist = Omegas.tolist()
    for r in range(nu.size):
        S = P["S"][r]
        if S < IntensityThreshold:
            continue
        GammaD, Gamma0, Shift0 = P["GammaD"][r], P["Gamma0"][r], P["Shift0"][r]
        if _profile == "doppler":
            mass = t["mass"][(int(P["M"][r]), int(P["I"][r]))]
            GammaD = (1.1774100225 / 2.99792458e8) * np.sqrt(1.3806503e-23 / 1.66053873e-27) * np.sqrt(T) * nu[r] / np.sqrt(mass)
            Shift0 = (float(sub["delta_air"][r]) if _lineshift else 0.0) * p / PREF
            W = max(OmegaWing, OmegaWingHW * GammaD)
        elif _profile == "lorentz":
            W = max(OmegaWing, OmegaWingHW * Gamma0)
        else:
            W = max(OmegaWing, OmegaWingHW * Gamma0, OmegaWingHW * GammaD)
        lo = _bisect.bisect(glist, nu[r] - W)
        hi = _bisect.bisect(glist, nu[r] + W)
        if hi <= lo:
            continue
        if _profile == "sdvoigt":
            dil = Diluent if Diluent else ({"air": 1.0} if GammaL.lower() == "gamma_air" else {"self": 1.0})
            Gamma2 = 0.0
            for species, abun in dil.items():
                sp = species.lower()
                sd = float(sub["SD_" + sp][r]) if ("SD_" + sp) in sub else 0.0
                g0db = float(sub["gamma_" + sp][r]) if ("gamma_" + sp) in sub else 0.0
                Gamma2 += abun * (sd * p / PREF) * g0db
            ls = PROFILE_SDVOIGT(nu[r], GammaD, Gamma0, Gamma2, Shift0, 0.0, Omegas[lo:hi])
        elif _profile == "doppler":
            ls = PROFILE_DOPPLER(nu[r] + Shift0, GammaD, Omegas[lo:hi])
        elif _profile == "lorentz":
            ls = PROFILE_LORENTZ(nu[r] + Shift0, Gamma0, Omegas[lo:hi])
        else:
            ls = PROFILE_VOIGT(nu[r] + Shift0, GammaD, Gamma0, Omegas[lo:hi])[0]
        mi = (int(P["M"][r]), int(P["I"][r]))
        Xsect[lo:hi] += factor / NAT[mi] * ABUN[mi] * S * ls
    return Omegas, Xsect


def layer_od(tbl, X, T, P_pa, PL_km, MF_VAL, MF_ID):
    """Optical depth of one homogeneous layer -- the build-defined meaning of compute_OD
    (radiative_transfer.py:395-456 cannot run: LBLRTM is an LFS stub):
    OD = sum_m  k_m(nu; T, p) [cm^-1, HITRAN_units=False] * x_m * PL * 1e5 cm."""
    X = np.asarray(X, dtype=np.float64)
    od = np.zeros(X.size)
    Mcol = np.asarray(tbl["molec_id"]).astype(int)
    Icol = np.asarray(tbl["local_iso_id"]).astype(int)
    pairs = sorted(set(zip(Mcol.tolist(), Icol.tolist())))
    for m, ppmv in zip(np.asarray(MF_ID).tolist(), np.asarray(MF_VAL).tolist()):
        comps = [(mm, ii) for (mm, ii) in pairs if mm == m]
        if not comps:
            continue
        _, xs = absorptionCoefficient_Voigt(tbl, Components=comps, T=float(T), p=float(P_pa) / 101325.0,
                                            OmegaGrid=X, HITRAN_units=False)
        od += xs * (ppmv * 1e-6) * PL_km * 1e5
    return od


def compute_TUD(tbl, Xmin, Xmax, DVOUT, Zs, Ts, Ps, PLs, MFs_VAL, MFs_ID, Altitudes=(500,), theta_r=0.0,
                N_angle=30, returnOD=False, return_layers=False):
    """radiative_transfer.py:274-392 with compute_OD := layer_od (see above)."""
    X = make_spectral_axis(Xmin, Xmax, DVOUT)
    nL = np.asarray(Ts).size
    OD = np.zeros((X.size, nL))
    for ii in range(nL):
        OD[:, ii] = layer_od(tbl, X, Ts[ii], Ps[ii], PLs[ii], np.asarray(MFs_VAL)[ii, :], MFs_ID)
    tau, Lu, Ld = tud_from_od(X, OD, Ts, Zs, Altitudes, theta_r, N_angle, returnOD)
    if return_layers:
        return X, tau, Lu, Ld, OD
    return X, tau, Lu, Ld


# ---- TUD Jacobian (the definitions rtx_line_prep_window and rtx_tud_jacobian implement) --------------------------------
def od_fixed_window(tbl, X, T, T_win, P_pa, PL_km, MF_VAL, MF_ID):
    """layer_od with absorptionCoefficient_Voigt's loop restated: every line's window from the base temperature T_win,
    everything else at T (the definition rtx_line_prep_window implements)."""
    p = float(P_pa) / 101325.0
    t = _tables()
    X = np.asarray(X, dtype=np.float64)
    glist = X.tolist()
    od = np.zeros(X.size)
    M = np.asarray(tbl["molec_id"]).astype(int)
    for m, ppmv in zip(np.asarray(MF_ID).tolist(), np.asarray(MF_VAL).tolist()):
        keep = M == m
        if not keep.any():
            continue
        sub = {k: np.asarray(v)[keep] for k, v in tbl.items()}
        P = line_params(sub, T, p)
        Pw = line_params(sub, T_win, p)
        nu = np.asarray(sub["nu"], dtype=np.float64)
        xs = np.zeros(X.size)
        for r in range(nu.size):
            W = max(0.0, 50.0 * Pw["Gamma0"][r], 50.0 * Pw["GammaD"][r])
            lo, hi = _bisect.bisect(glist, nu[r] - W), _bisect.bisect(glist, nu[r] + W)
            if hi <= lo:
                continue
            ls = PROFILE_VOIGT(nu[r] + P["Shift0"][r], P["GammaD"][r], P["Gamma0"][r], X[lo:hi])[0]
            mi = (int(P["M"][r]), int(P["I"][r]))
            xs[lo:hi] += volumeConcentration(p, T) * P["S"][r] * ls * (t["abun"][mi] / t["abun"][mi])
        od += xs * (ppmv * 1e-6) * PL_km * 1e5
    return od


def planck_dT(X, T):
    """B(nu, T) [nX][nL] of planckian and dB/dT analytic: dB/dT = B (u/T) e^u/(e^u - 1), u = c2 nu / T."""
    B = planckian(X, T)
    u = C2 * (np.asarray(X)[:, None] * 100.0) / np.asarray(T)[None, :]
    return B, B * (u / np.asarray(T)[None, :]) * (-1.0 / np.expm1(-u))


def jacobian_from_od(X, OD, T, Z, Altitudes, theta_r=0.0, N_angle=30, returnOD=False, layers=None):
    """g[row][nX][layer] = d row / d OD_l and h[row][nX][layer] = d row / d T_l at fixed OD, rows = tau per altitude,
    L-up per altitude, Ld: the closed forms rtx_tud_jacobian evaluates, with prefix sums for every transmittance product.
    With N_angle = 1 tud_from_od's Ld is 0/0 (theta = 0 carries weight 0), so are its derivatives: the Ld rows are NaN."""
    OD = np.asarray(OD, dtype=np.float64)  # [nX][nL]
    nX, nL = OD.shape
    layers = np.arange(nL) if layers is None else np.asarray(layers)
    Z_s = np.array([Altitudes]).ravel()
    nZ = Z_s.size
    mu = 1.0 / np.cos(theta_r)
    B, dB = planck_dT(X, T)
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
    if int(N_angle) == 1:
        g[2 * nZ] = h[2 * nZ] = np.nan
        return g, h
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


# ---- the nodal line-sum's classification (rtx_voigt_scatter.hip: row_geom, nodal_tile) -------------------------------
# Restated so that host tests can show which path a configuration reaches. Not an oracle of values: the line-sum's
# results are checked against absorptionCoefficient_Voigt; this only says which code evaluates which (line, tile).
LS_ROWS, LS_NEAR, LS_TILE_DIST, LS_NW = 16, 2, 512, 2  # RTX_SC_ROWS, RTX_SC_NEAR, RTX_SC_TILE_DIST, SC_NW
LS_EDGE_CAP, LS_ENT_CAP, LS_SPLIT_MIN, LS_SPLIT_PART = 32, 16, 768, 256  # SC_EDGE_CAP, SC_ENT_CAP, RTX_SPLIT_*


def _row_bits(lo, hi, rows=LS_ROWS):
    r = np.arange(rows)[None, :]
    return (r >= np.asarray(lo)[:, None]) & (r < np.asarray(hi)[:, None])


def row_masks(i0, lo, hi, zw, ia, nt, rows=LS_ROWS, near=LS_NEAR):
    """row_geom and the row masks of voigt_nodal_kernel for lines (local i0, window [lo, hi), band half-width zw; int
    arrays) in the tile [ia, ia + nt): bool [lines][rows] masks reach, inside (m_in), near, band, far, pp, edge, bd, and
    the per-line r_lo, r_hi, part_l, part_r, rc (centre row, floor)."""
    i0, lo, hi, zw = (np.asarray(v, dtype=np.int64) for v in (i0, lo, hi, zw))
    dlo, dhi = lo - ia, hi - ia
    lo_t, hi_t = np.maximum(dlo, 0), np.minimum(dhi, nt)
    r_lo, r_hi = lo_t >> 6, (hi_t + 63) >> 6
    c0 = (lo_t + 63) >> 6
    c1 = np.where(dhi < nt, hi_t >> 6, r_hi)  # a ragged last row of the grid is not an edge
    zl, zh = i0 - np.maximum(zw, 0) - ia, i0 + np.maximum(zw, 0) - ia
    has_z = (zw > 0) & (zh >= 0) & (zl < 64 * rows)
    z0 = np.where(has_z, np.where(zl > 0, zl >> 6, 0), rows)
    z1 = np.where(has_z, np.minimum(zh >> 6, rows - 1), -1)
    rc = (i0 - ia) >> 6
    n0, n1 = np.minimum(rc - near, zl >> 6), np.maximum(rc + near, zh >> 6)
    reach = ((hi > ia) & (lo < ia + nt))[:, None]
    m = {"reach": reach & _row_bits(r_lo, r_hi, rows), "inside": reach & _row_bits(c0, c1, rows),
         "near": _row_bits(np.maximum(n0, 0), np.minimum(n1, rows - 1) + 1, rows), "band": _row_bits(z0, z1 + 1, rows)}
    m["far"] = m["inside"] & ~m["near"]
    m["pp"] = m["inside"] & m["near"] & ~m["band"]
    m["edge"] = m["reach"] & ~m["inside"] & ~m["band"]
    m["bd"] = m["reach"] & m["band"]
    m.update(r_lo=r_lo, r_hi=r_hi, part_l=c0 != r_lo, part_r=c1 != r_hi, rc=rc)
    return m


def linesum_records(tbl, grid, T, p, omega_wing=0.0, omega_wing_hw=50.0, Diluent=None):
    """line_prep_kernel's geometry for one layer, per line of `tbl` in ascending-nu (stable) order -- the order of the
    device table: local i0 (nearest index to the shifted centre, clamped), window [lo, hi) (local, bisect_right of
    nu -+ W on the global axis, clamped to the shard; empty = 0, 0), zw, fp32 y, cte, sg0, the global gi0 before the
    local clamp and whether W came from OmegaWing; for sd_census also W, the unclamped global window glo / ghi, the sort
    order and line_params' dict P of the sorted table. grid = (xmin, xmax, n_total, offset, n)."""
    xmin, xmax, n_total, offset, n = grid
    step = (xmax - xmin) / (n_total - 1)
    order = np.argsort(np.asarray(tbl["nu"], dtype=np.float64), kind="stable")
    sub = {k: np.asarray(v)[order] for k, v in tbl.items()}
    P = line_params(sub, T, p, Diluent=Diluent)
    nu = np.asarray(sub["nu"], dtype=np.float64)
    Whw = omega_wing_hw * np.maximum(P["Gamma0"], P["GammaD"])
    W = np.maximum(omega_wing, Whw)

    def gx(ig):
        return np.where(ig == n_total - 1, xmax, ig.astype(np.float64) * step + xmin)

    def bisect_right(v):
        t = (v - xmin) / step
        k = np.where(~(t > -1.0), 0, np.where(t >= n_total, n_total, np.floor(np.clip(t, -2.0, n_total)) + 1)).astype(np.int64)
        k = np.clip(k, 0, n_total)
        for _ in range(4):
            k = np.where((k < n_total) & (gx(np.minimum(k, n_total - 1)) <= v), k + 1, k)
            k = np.where((k > 0) & (gx(np.maximum(k - 1, 0)) > v), k - 1, k)
        return k

    lo = np.clip(bisect_right(nu - W) - offset, 0, n)
    hi = np.clip(bisect_right(nu + W) - offset, 0, n)
    live = hi > lo
    lo, hi = np.where(live, lo, 0), np.where(live, hi, 0)
    sg0 = nu + P["Shift0"]
    cte = np.sqrt(np.log(2.0)) / P["GammaD"]
    y = P["Gamma0"] * cte
    gi0 = np.clip(np.rint((sg0 - xmin) / step), -1e9, 1e9).astype(np.int64)
    i0 = np.clip(gi0 - offset, -100000000, n + 100000000)
    zw = np.where((y < 15.0) & live, np.minimum(np.ceil((15.0 - y) / (step * cte)) + 2.0, 4e7), 0).astype(np.int64)
    return {"i0": i0, "lo": lo, "hi": hi, "zw": zw, "y": y.astype(np.float32), "cte": cte, "sg0": sg0, "gi0": gi0,
            "W_omega": omega_wing > Whw, "nu": nu, "step": step, "W": W, "glo": bisect_right(nu - W), "ghi": bisect_right(nu + W),
            "order": order, "P": P}


def _band_row_labels(R, l, r, ia, grid, smally):
    """The band_row branch a (line, row) takes: lanes' x in fp64 (the kernel's fp32 x differs by ~1e-7 of |x|)."""
    xmin, xmax, n_total, offset, n = grid
    i = offset + ia + 64 * r + np.arange(64)
    X = np.where(i == n_total - 1, xmax, i * R["step"] + xmin)
    x = (X - R["sg0"][l]) * R["cte"][l]
    y = float(R["y"][l])
    out = set()
    if smally and y < 1.0:
        if np.all(np.abs(x) >= 5.5):
            out.add("band_outer")  # asymK_re<12> in fp32
        else:
            return {"band_w64"}  # fp64 Weideman on every lane
    if np.any(np.abs(np.abs(x) + y - 15.0) < 2e-3):
        out.add("band_recheck")  # the |x| + y < 15 switch repeated in fp64
    if y >= 1.0:
        wz = np.abs(x) + y < 15.0
        if y >= 6.0:
            out.add("band_asym6")
        elif not np.any(wz & (x * x + y * y < 64.0)):
            out.add("band_series")  # 1 <= y < 6, every Weideman lane at |z| >= 8
        else:
            out.add("band_wei32")
    return out


def linesum_census(tbl, grid, T, p, omega_wing=0.0, omega_wing_hw=50.0, Diluent=None):
    """Which paths of rtx_voigt_sum's nodal kernel a call reaches: a Counter of labels over every layer, (line, tile or
    hot-tile part) and wave round. T, p: per-layer sequences. Candidates are the canonical range of each tile (first to
    last line whose window meets it, tile_ranges_kernel), cut into parts of LS_SPLIT_PART when longer than LS_SPLIT_MIN;
    candidate c of a part goes to wave c % LS_NW, round c // (64 LS_NW)."""
    from collections import Counter
    xmin, xmax, n_total, offset, n = grid
    tile = 64 * LS_ROWS
    full_rows = (1 << LS_ROWS) - 1
    C = Counter()
    for T_k, p_k in zip(np.atleast_1d(T), np.atleast_1d(p)):
        R = linesum_records(tbl, grid, float(T_k), float(p_k), omega_wing, omega_wing_hw, Diluent)
        i0, lo, hi, zw = R["i0"], R["lo"], R["hi"], R["zw"]
        smally = bool(np.any((zw > 0) & (R["y"] < 1.0)))
        C["smally_layer" if smally else "plain_layer"] += 1
        live = hi > lo
        C["W_omega"] += int(np.sum(live & R["W_omega"]))
        C["W_hw"] += int(np.sum(live & ~R["W_omega"]))
        C["i0_clamped"] += int(np.sum(live & (i0 != R["gi0"] - offset)))
        C["centre_left"] += int(np.sum(live & (i0 < 0)))
        C["centre_right"] += int(np.sum(live & (i0 >= n)))
        C["covers_grid"] += int(np.sum(live & (lo == 0) & (hi == n) & (i0 > 0) & (i0 < n - 1)))
        C["narrow"] += int(np.sum(live & (hi - lo < 64) & (lo > 0) & (hi < n)))
        for ia in range(0, n, tile):
            nt = min(tile, n - ia)
            reach = live & (hi > ia) & (lo < ia + nt)
            if not reach.any():
                continue
            idx = np.nonzero(reach)[0]
            first, last = int(idx[0]), int(idx[-1]) + 1
            cnt = last - first
            parts = [(first, min(first + LS_SPLIT_PART, last))] if cnt > LS_SPLIT_MIN else [(first, last)]
            if cnt > LS_SPLIT_MIN:
                C["hot_smally" if smally else "hot_plain"] += 1
                for q in range(1, (cnt - 1) // LS_SPLIT_PART + 1):
                    parts.append((first + q * LS_SPLIT_PART, min(first + (q + 1) * LS_SPLIT_PART, last)))
            for a, b in parts:
                sl = np.arange(a, b)
                if b - a > 64 * LS_NW:
                    C["rounds"] += 1
                m = row_masks(i0[sl], lo[sl], hi[sl], zw[sl], ia, nt)
                bitsum = lambda M: (M.astype(np.int64) << np.arange(LS_ROWS)).sum(1)
                far, pp, ed, bd = bitsum(m["far"]), bitsum(m["pp"]), bitsum(m["edge"]), bitsum(m["bd"])
                is_t = (far == full_rows) & ((ia - i0[sl] >= LS_TILE_DIST) | (i0[sl] - (ia + tile - 1) >= LS_TILE_DIST))
                full = (far == full_rows) & ~is_t
                part = (far != 0) & (far != full_rows)
                single = (pp == 0) & (bd == 0) & (ed != 0) & ((ed & (ed - 1)) == 0)
                re = np.where(single, np.log2(np.maximum(ed, 1)).astype(np.int64), 0)
                left, right = m["part_l"] & (re == m["r_lo"]), m["part_r"] & (re == m["r_hi"] - 1)
                edge_only = single & (left != right)
                entry = ~edge_only & ((pp | ed | bd) != 0)
                for name, sel in (("tile", is_t), ("full", full), ("partial", part), ("edge_only", edge_only),
                                  ("entry", entry), ("near", pp != 0), ("band", bd != 0)):
                    C[name] += int(sel.sum())
                    if name in ("tile", "full", "partial", "edge_only", "entry"):
                        c = np.arange(b - a)
                        key = (c % LS_NW) + LS_NW * (c // (64 * LS_NW))
                        per = np.bincount(key[sel], minlength=1)
                        if name == "edge_only" and per.max() > LS_EDGE_CAP:
                            C["edge_overflow"] += 1  # a wave round emits more than the list holds: drained mid-round
                        if name == "entry" and per.max() > LS_ENT_CAP:
                            C["entry_overflow"] += 1
                        if name in ("tile", "full", "partial") and np.any((per > 8) & (per % 8 != 0)):
                            C[name + "_ragged"] += 1  # several groups of 8 members in a round, the last one ragged
                for d in (511, 512, 513):
                    C["tile_left_%d" % d] += int(np.sum(is_t & (ia - i0[sl] == d)))
                    C["tile_right_%d" % d] += int(np.sum(is_t & (i0[sl] - (ia + tile - 1) == d)))
                    C["full_left_%d" % d] += int(np.sum(full & (ia - i0[sl] == d)))
                    C["full_right_%d" % d] += int(np.sum(full & (i0[sl] - (ia + tile - 1) == d)))
                inside = (i0[sl] >= ia) & (i0[sl] < ia + nt) & (pp != 0)
                for rc in (0, LS_ROWS // 2, LS_ROWS - 1):
                    C["centre_row_%d" % rc] += int(np.sum(inside & (m["rc"] == rc)))
                C["one_row"] += int(np.sum((m["r_hi"] - m["r_lo"] == 1) & m["part_l"] & m["part_r"] & (m["reach"].any(1))))
                dlo, dhi = lo[sl] - ia, hi[sl] - ia
                C["lo_aligned"] += int(np.sum((dlo > 0) & (dlo < nt) & (dlo % 64 == 0)))
                C["hi_aligned"] += int(np.sum((dhi > 0) & (dhi < nt) & (dhi % 64 == 0)))
                for j in np.nonzero(bd != 0)[0]:
                    for r in np.nonzero(m["bd"][j])[0]:
                        for lab in _band_row_labels(R, a + j, int(r), ia, grid, smally):
                            C[lab] += 1
    return C


# ---- the explicit-axis line-sum's prologue and decisions (line_prep_axis_kernel, rtx_voigt_axis.hip) --------------------
# As above: which code evaluates which (line, tile, row), not an oracle of values.
AX_TILE = 1024  # AX_TILE; rows of 64 points are counted from the tile's first point


def axis_records(tbl, X, T, p, omega_wing=0.0, omega_wing_hw=50.0, Diluent=None, profile=0, lineshift=True):
    """line_prep_axis_kernel for one layer, per line of `tbl` in ascending-nu (stable) order: window [lo, hi) =
    bisect_right(X, nu -+ W) (empty: 0, 0; lo_raw / hi_raw before that), ic = bisect_right(X, nu), the band range
    [zlo, zhi) = [bisect_left(X, sg0 - wz), bisect_right(X, sg0 + wz)) with wz = (15 - y + 0.01)/cte, clamped to the window
    (zlo_raw / zhi_raw before the clamp), y (fp64; y32 as the record holds it), cte, sg0, W and maxhw = max over live lines
    of max(ic - lo, hi - ic) + 1. profile 0 Voigt, 1 Lorentz (y = 15, cte = 1/Gamma0: no band), 2 Doppler (y = 0, the
    function's own GammaD, Shift0 = delta_air p when lineshift)."""
    X = np.asarray(X, dtype=np.float64)
    nx = X.size
    order = np.argsort(np.asarray(tbl["nu"], dtype=np.float64), kind="stable")
    sub = {k: np.asarray(v)[order] for k, v in tbl.items()}
    P = line_params(sub, T, p, Diluent=Diluent)
    nu = np.asarray(sub["nu"], dtype=np.float64)
    GammaD, Gamma0, Shift0 = P["GammaD"], P["Gamma0"], P["Shift0"]
    if profile == 2:
        t = _tables()
        mass = np.array([t["mass"][(int(m), int(i))] for m, i in zip(P["M"], P["I"])])
        GammaD = (1.1774100225 / 2.99792458e8) * np.sqrt(1.3806503e-23 / 1.66053873e-27) * np.sqrt(T) * nu / np.sqrt(mass)
        Gamma0 = np.zeros(nu.size)
        Shift0 = (np.asarray(sub["delta_air"], dtype=np.float64) if lineshift else np.zeros(nu.size)) * p / PREF
        W = np.maximum(omega_wing, omega_wing_hw * GammaD)
    elif profile == 1:
        W = np.maximum(omega_wing, omega_wing_hw * Gamma0)
    else:
        W = np.maximum(omega_wing, np.maximum(omega_wing_hw * Gamma0, omega_wing_hw * GammaD))
    lo_raw = np.searchsorted(X, nu - W, side="right")
    hi_raw = np.searchsorted(X, nu + W, side="right")
    live = hi_raw > lo_raw
    lo, hi = np.where(live, lo_raw, 0), np.where(live, hi_raw, 0)
    ic = np.searchsorted(X, nu, side="right")
    sg0 = nu + Shift0
    if profile == 1:
        cte, y = 1.0 / Gamma0, np.full(nu.size, 15.0)
    else:
        cte = np.sqrt(np.log(2.0)) / GammaD
        y = Gamma0 * cte
    wz = (15.0 - y + 0.01) / cte
    zlo_raw = np.searchsorted(X, sg0 - wz, side="left")
    zhi_raw = np.searchsorted(X, sg0 + wz, side="right")
    has = (y < 15.0) & live
    zlo = np.where(has, np.maximum(zlo_raw, lo), 0)
    zhi = np.maximum(np.where(has, np.minimum(zhi_raw, hi), 0), zlo)
    hw = np.where(live, np.maximum(ic - lo, hi - ic) + 1, 0)
    return {"lo": lo, "hi": hi, "lo_raw": lo_raw, "hi_raw": hi_raw, "live": live, "ic": ic, "zlo": zlo, "zhi": zhi,
            "zlo_raw": zlo_raw, "zhi_raw": zhi_raw, "has_band": has, "y": y, "y32": y.astype(np.float32), "cte": cte, "sg0": sg0,
            "nu": nu, "W": W, "wz": wz, "maxhw": int(hw.max()) if nu.size else 0, "order": order, "nx": nx}


def axis_abscissa_f32(X, ia, sg0, cte, form="split"):
    """axis_line's fp32 abscissa x_i = (X[i] - sg0) cte on the tile that starts at index ia, in np.float32 arithmetic.
    form="split": the kernel's seven operations, (dh kh + ch) + (err(dh kh) + cl + dh kl + dl kh) on d_i = X[i] - X[ia],
    c = (X[ia] - sg0) cte and cte as two floats each; form="fma": the one-FMA form fmaf((float)d_i, (float)cte, (float)c)
    DESIGN 4.8 rejects. fmaf is the exact float64 product (two fp32 factors: 48 bits) plus the addend, rounded once to fp32."""
    f32, f64 = np.float32, np.float64
    X = np.asarray(X, dtype=f64)
    dd = X[ia:ia + AX_TILE] - X[ia]
    c64 = (X[ia] - f64(sg0)) * f64(cte)
    fma = lambda a, b, c: (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)
    if form == "fma":
        return fma(dd.astype(f32), f32(cte), f32(c64))
    if form != "split":
        raise ValueError(form)
    dh = dd.astype(f32)
    dl = (dd - dh.astype(f64)).astype(f32)
    ch = f32(c64)
    cl = f32(c64 - f64(ch))
    kh = f32(cte)
    kl = f32(f64(cte) - f64(kh))
    p = dh * kh
    low = fma(dh, kl, fma(dl, kh, cl + fma(dh, kh, -p)))
    return (p + ch) + low


def axis_census(tbl, X, T, p, omega_wing=0.0, omega_wing_hw=50.0, Diluent=None, profile=0, lineshift=True):
    """Which windows, candidate ranges and profile branches a rtx_line_prep_axis + rtx_voigt_sum_axis call reaches: a
    Counter of labels over every layer, (line, tile) and 64-point row of the tile. T, p: per-layer sequences; Diluent:
    {name: scalar or per-layer fractions}. The switch |x| + y < 15, its 2e-3 collar and the |z| < 8 ballot are evaluated in
    fp64 on x = -((sg0 - X[i]) cte) (the kernel's fp32 x differs by ~1e-7 of |x|); y < 1 and y >= 6 on the record's fp32 y.

    Windows (per line and layer): lo_row_aligned / lo_tile_aligned / hi_row_aligned / hi_tile_aligned (an edge inside the
    axis on a multiple of 64 / 1024), one_row (both edges inside one row, neither on its boundary), one_point,
    empty_between_points (nu -+ W fall between two neighbouring points: no record, no maxhw), edge_point_excluded (an axis
    point exactly at nu - W), edge_point_included (one exactly at nu + W), covers_axis, centre_left / centre_right (ic = 0 /
    nx with a window reaching in), centre_on_point, same_nu, band_empty (zlo == zhi before the clamp, window not empty),
    band_clamped_lo / _hi (the window cuts the band), band_cut_by_axis_end, maxhw_layers_differ.
    Candidates (per tile and layer): cand_0 ... cand_5, cand_not_mult4, cand_ge_256, idle_waves (1 to 3 candidates),
    tile_zero_between (no candidate, neighbours on both sides with some), left_reaches_tile1 (ic = 0, window into tile 1),
    outside_bracket (a line whose window meets the tile but whose ic lies outside [ia - maxhw, ib - 1 + maxhw]: must be 0)
    and outside_bracket_without_margin (the same with maxhw - 1).
    Rows (per line, tile, row that meets the window): band_w64 (y < 1: fp64 Weideman lanes), band_wei32, band_series_y6,
    band_series_ballot (1 <= y < 6, no Weideman lane at |z| < 8), ballot_and_wei32_same_line, far_rational (some in-window
    lane takes the rational), lorentz_rows, doppler_w64, doppler_dropped (in-window lanes of a Doppler record beyond the
    band: 0); lanes: recheck_in / recheck_out (inside the collar, fp64 decides < 15 / >= 15), switch_fp32 (band lanes
    within 0.01 of the switch but outside the collar: the fp32 comparison stands)."""
    from collections import Counter
    X = np.asarray(X, dtype=np.float64)
    nx = X.size
    T, p = np.atleast_1d(T), np.atleast_1d(p)
    nL = T.size
    C = Counter()
    n_tiles = (nx + AX_TILE - 1) // AX_TILE
    hws = []
    for k in range(nL):
        dil = None if Diluent is None else {n: float(np.broadcast_to(np.asarray(v, dtype=np.float64), (nL,))[k]) for n, v in Diluent.items()}
        R = axis_records(tbl, X, float(T[k]), float(p[k]), omega_wing, omega_wing_hw, dil, profile, lineshift)
        if k == 0:
            ic = R["ic"]  # written from layer 0 (the same in every layer: it depends on nu and X alone)
        assert np.array_equal(ic, R["ic"])
        hws.append(R["maxhw"])
        lo, hi, live, nu, W = R["lo"], R["hi"], R["live"], R["nu"], R["W"]
        inside = live & (lo > 0)
        C["lo_row_aligned"] += int(np.sum(inside & (lo % 64 == 0)))
        C["lo_tile_aligned"] += int(np.sum(inside & (lo % AX_TILE == 0)))
        C["hi_row_aligned"] += int(np.sum(live & (hi < nx) & (hi % 64 == 0)))
        C["hi_tile_aligned"] += int(np.sum(live & (hi < nx) & (hi % AX_TILE == 0)))
        C["one_row"] += int(np.sum(live & (lo // 64 == (hi - 1) // 64) & (lo % 64 != 0) & (hi % 64 != 0)))
        C["one_point"] += int(np.sum(live & (hi - lo == 1)))
        C["empty_between_points"] += int(np.sum(~live & (R["lo_raw"] > 0) & (R["lo_raw"] < nx)))
        C["edge_point_excluded"] += int(np.sum(inside & (X[np.maximum(lo, 1) - 1] == nu - W)))
        C["edge_point_included"] += int(np.sum(live & (X[np.maximum(hi, 1) - 1] == nu + W)))
        C["covers_axis"] += int(np.sum(live & (lo == 0) & (hi == nx) & (ic > 0) & (ic < nx)))
        C["centre_left"] += int(np.sum(live & (ic == 0)))
        C["centre_right"] += int(np.sum(live & (ic == nx)))
        C["centre_on_point"] += int(np.sum(live & (ic > 0) & (X[np.maximum(ic, 1) - 1] == nu)))
        C["same_nu"] += int(np.sum(live[1:] & live[:-1] & (nu[1:] == nu[:-1])))
        has = R["has_band"]
        C["band_empty"] += int(np.sum(has & (R["zlo_raw"] == R["zhi_raw"])))
        C["band_clamped_lo"] += int(np.sum(has & (R["zlo_raw"] < lo) & (R["zhi"] > R["zlo"])))
        C["band_clamped_hi"] += int(np.sum(has & (R["zhi_raw"] > hi) & (R["zhi"] > R["zlo"])))
        if nx:
            C["band_cut_by_axis_end"] += int(np.sum(has & (R["zhi"] > R["zlo"]) &
                                                    ((R["sg0"] - R["wz"] < X[0]) | (R["sg0"] + R["wz"] > X[-1]))))
        counts = []
        ballot_lines, wei_lines = set(), set()
        for t in range(n_tiles):
            ia, ib = t * AX_TILE, min((t + 1) * AX_TILE, nx)
            reach = np.nonzero(live & (hi > ia) & (lo < ib))[0]
            if reach.size == 0:
                counts.append(0)
                C["cand_0"] += 1
                continue
            first, last = int(reach[0]), int(reach[-1]) + 1
            for margin, lab in ((0, "outside_bracket"), (1, "outside_bracket_without_margin")):
                h = R["maxhw"] - margin
                l0, l1 = np.searchsorted(ic, ia - h, side="left"), np.searchsorted(ic, ib - 1 + h, side="right")
                C[lab] += int(first < l0) + int(last > l1)
            cnt = last - first
            counts.append(cnt)
            if cnt <= 5:
                C["cand_%d" % cnt] += 1
            C["cand_not_mult4"] += int(cnt % 4 != 0)
            C["cand_ge_256"] += int(cnt >= 256)
            C["idle_waves"] += int(cnt < 4)
            C["left_reaches_tile1"] += int(np.sum(ic[reach] == 0)) if t == 1 else 0
            for l in reach:
                t_lo, t_hi = max(int(lo[l]) - ia, 0), min(int(hi[l]), ib) - ia
                rows = np.arange(t_lo >> 6, (t_hi + 63) >> 6)
                if profile == 1:
                    C["lorentz_rows"] += rows.size
                    continue
                zlo, zhi = int(R["zlo"][l]), int(R["zhi"][l])
                row0 = ia + 64 * rows
                is_band = (row0 + 64 > zlo) & (row0 < zhi)
                far_lab = "doppler_dropped" if profile == 2 else "far_rational"
                C[far_lab] += int(np.sum(~is_band))
                y, y32 = float(R["y"][l]), float(R["y32"][l])
                for r in rows[is_band]:
                    i = ia + 64 * r + np.arange(64)
                    i = i[i < ib]
                    win = (i >= lo[l]) & (i < hi[l])
                    in_band = (i >= zlo) & (i < zhi)
                    x = -((R["sg0"][l] - X[i]) * R["cte"][l])
                    s = np.abs(x) + y
                    wz = in_band & (s < 15.0)
                    if y32 < 1.0:
                        if wz.any():
                            C["doppler_w64" if profile == 2 else "band_w64"] += 1
                    else:
                        near = in_band & (np.abs(s - 15.0) < 2e-3)
                        C["recheck_in"] += int(np.sum(near & (s < 15.0)))
                        C["recheck_out"] += int(np.sum(near & ~(s < 15.0)))
                        C["switch_fp32"] += int(np.sum(in_band & ~near & (np.abs(s - 15.0) < 0.01)))
                        if wz.any():
                            if y32 >= 6.0:
                                C["band_series_y6"] += 1
                            elif not np.any(wz & (x * x + y * y < 64.0)):
                                C["band_series_ballot"] += 1
                                ballot_lines.add(int(l))
                            else:
                                C["band_wei32"] += 1
                                wei_lines.add(int(l))
                    if np.any(win & ~wz):
                        C[far_lab] += 1
        C["ballot_and_wei32_same_line"] += len(ballot_lines & wei_lines)
        c = np.asarray(counts)
        if c.size >= 3:
            some_before = np.maximum.accumulate(c)[:-2] > 0
            some_after = np.maximum.accumulate(c[::-1])[::-1][2:] > 0
            C["tile_zero_between"] += int(np.sum((c[1:-1] == 0) & some_before & some_after))
    C["maxhw_layers_differ"] += int(len(set(hws)) > 1)
    return C


# ---- post-processing of TUD products ----------------------------------------
def smooth(x, window_len=11, window="hanning"):
    """radiative_transfer.py:1266-1324: reflect-pad by window_len-1 samples, convolve with the normalised
    window ('valid'), cut back to len(x). For an even window_len the result is half a sample off centre."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 1 or x.size < window_len or window_len < 3:
        return x
    if window not in ("flat", "hanning", "hamming", "bartlett", "blackman"):
        return x
    s = np.r_[x[window_len - 1:0:-1], x, x[-2:-window_len - 1:-1]]  # :1314
    w = np.ones(window_len, "d") if window == "flat" else getattr(np, window)(window_len)
    y = np.convolve(w / w.sum(), s, mode="valid")
    ix0 = int(np.ceil(window_len / 2 - 1))
    ix1 = -int(np.floor(window_len / 2))
    return y[ix0:ix1]


def smooth_sym(y, window_len, window="hanning"):
    """The symmetrised smoother of reduceResolution (:1331): mean of smoothing y and smoothing y reversed."""
    return 0.5 * (smooth(y, window_len, window) + smooth(y[::-1], window_len, window)[::-1])


def reduceResolution(X, Y, dX, N=4, window="hanning", X_out=None):
    """radiative_transfer.py:1327-1350 (np.int -> int): symmetric window smoothing over round(dX/dX_in) samples,
    then scipy's cubic interp1d (a not-a-knot cubic spline through ALL smoothed samples) evaluated on
    X_out = linspace(X_[smFactor], X_[-smFactor-1], ceil(N*span/dX)+1)."""
    import scipy.interpolate

    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    dX_in = np.mean(np.diff(X))
    smFactor = int(np.round(dX / dX_in))
    sm = lambda y: smooth_sym(y, smFactor, window)
    interp = lambda x, y, x0: scipy.interpolate.interp1d(x, y, kind="cubic", bounds_error=False, fill_value="extrapolate")(x0)
    X_ = sm(X)
    nPts = int(np.ceil(N * (X_[-smFactor - 1] - X_[smFactor]) / dX)) + 1
    ret_x = X_out is None
    if ret_x:
        X_out = np.linspace(X_[smFactor], X_[-smFactor - 1], nPts)
    if Y.ndim > 1:
        Y_out = np.zeros((X_out.size, Y.shape[-1]))
        for ii in range(Y.shape[-1]):
            Y_out[:, ii] = interp(X_, sm(Y[:, ii]), X_out)
    else:
        Y_out = interp(X_, sm(Y), X_out)
    return (X_out, Y_out) if ret_x else Y_out


# ---- speed-dependent Voigt: pcqsdhc with anuVC = eta = 0 -------------------------------
_CPF3_TT = np.array([0.5, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5, 7.5, 8.5, 9.5, 10.5, 11.5, 12.5, 13.5, 14.5])


def cpf3(X, Y, dtype=np.float64):
    """misc/hapi.py:9645-9670: 15-term asymptotic series of w(z), z = X + iY."""
    F = _wide(dtype)[0]
    zm1 = 1.0 / (np.asarray(X, dtype=F) + 1.0j * np.asarray(Y, dtype=F))
    zm2 = zm1 ** 2
    zsum = np.ones_like(zm1)
    zterm = np.ones_like(zm1)
    for t in _CPF3_TT:
        zterm = zterm * zm2 * t
        zsum = zsum + zterm
    zsum = zsum * 1.0j * zm1 * 0.564189583547756
    return zsum.real, zsum.imag


# branch bits of PROFILE_SDVOIGT(..., branches=True): the predicates of pcqsdhc, per point
SD_P1, SD_P2, SD_P3, SD_P4, SD_CPF3, SD_W24_1, SD_W24_2, SD_P3NEAR, SD_NEG1, SD_NEG2 = (1 << b for b in range(10))


def PROFILE_SDVOIGT(sg0, GamD, Gam0, Gam2, Shift0, Shift2, sg, dtype=np.float64, branches=False):
    """misc/hapi.py:10117-10129 -> pcqsdhc (:9850-10024) with anuVC = eta = 0, for which the common part (:10022) is
    LS = Aterm/pi. Real part only (what absorptionCoefficient_SDVoigt uses, :10897). CPF = hum1_wei (:9846).
    dtype np.longdouble: the same formulas, predicates and Weideman coefficients in extended precision (the parameters
    and the grid are the float64 values). branches: also the int array of SD_* bits (PART, cpf3 shell, |x| + y < 15 of
    the first / second argument, PART3's near form, a negative real part of the first / second argument)."""
    F, CT, pi, sln2 = _wide(dtype)
    sg = np.asarray(sg, dtype=F)
    cte = sln2 / GamD
    rpi = np.sqrt(pi)
    if F is np.float64:
        c0 = complex(Gam0, Shift0)
        c2 = complex(Gam2, Shift2)
    else:
        c0 = CT(F(Gam0) + 1.0j * F(Shift0))
        c2 = CT(F(Gam2) + 1.0j * F(Shift2))
        Gam2, Shift2 = F(Gam2), F(Shift2)
    c0t = c0 - 1.5 * c2
    c2t = c2
    cw = lambda x, y: (lambda r: r[0] + 1.0j * r[1])(hum1_wei(x, y, dtype))
    code = np.zeros(sg.size, dtype=np.int64)
    w24 = lambda Z: (np.abs(Z.imag) + Z.real < 15.0)
    if abs(c2t) == 0.0:  # PART1 (:9908-9915)
        Z1 = (1.0j * (sg0 - sg) + c0t) * cte
        A = rpi * cte * cw(-Z1.imag, Z1.real)
        code[:] = SD_P1 + SD_W24_1 * w24(Z1) + SD_NEG1 * (Z1.real < 0)
        return ((A / pi).real, code) if branches else (A / pi).real
    X = (1.0j * (sg0 - sg) + c0t) / c2t
    Y = 1.0 / ((2.0 * cte * c2t)) ** 2
    csqrtY = (Gam2 - 1.0j * Shift2) / (2.0 * cte * (Gam2 ** 2 + Shift2 ** 2))
    p2 = np.abs(X) <= 3.0e-8 * abs(Y)
    p3 = (abs(Y) <= 1.0e-15 * np.abs(X)) & ~p2
    p4 = ~(p2 | p3)
    A = np.zeros(sg.size, dtype=CT)
    if np.any(p4):  # PART4 (:9933-9971)
        Z1 = np.sqrt(X[p4] + Y) - csqrtY
        Z2 = Z1 + 2.0 * csqrtY
        x1, y1, x2, y2 = -Z1.imag, Z1.real, -Z2.imag, Z2.real
        S1, S2 = np.sqrt(x1 ** 2 + y1 ** 2), np.sqrt(x2 ** 2 + y2 ** 2)
        use3 = (np.abs(S1 - S2) <= 1.0) & (np.maximum(S1, S2) > 8.0) & (np.minimum(S1, S2) <= 8.0)
        W1 = np.zeros(Z1.size, dtype=CT)
        W2 = np.zeros(Z1.size, dtype=CT)
        if np.any(use3):
            r1, r2 = cpf3(x1[use3], y1[use3], dtype), cpf3(x2[use3], y2[use3], dtype)
            W1[use3], W2[use3] = r1[0] + 1.0j * r1[1], r2[0] + 1.0j * r2[1]
        if np.any(~use3):
            W1[~use3], W2[~use3] = cw(x1[~use3], y1[~use3]), cw(x2[~use3], y2[~use3])
        A[p4] = rpi * cte * (W1 - W2)
        code[p4] = SD_P4 + SD_CPF3 * use3 + SD_W24_1 * w24(Z1) + SD_W24_2 * w24(Z2) + SD_NEG1 * (y1 < 0) + SD_NEG2 * (y2 < 0)
    if np.any(p2):  # PART2 (:9974-9989)
        Z1 = (1.0j * (sg0 - sg[p2]) + c0t) * cte
        Z2 = np.sqrt(X[p2] + Y) + csqrtY
        A[p2] = rpi * cte * (cw(-Z1.imag, Z1.real) - cw(-Z2.imag, Z2.real))
        code[p2] = SD_P2 + SD_W24_1 * w24(Z1) + SD_W24_2 * w24(Z2) + SD_NEG1 * (Z1.real < 0) + SD_NEG2 * (Z2.real < 0)
    if np.any(p3):  # PART3 (:9992-10017; the reference indexes the full X at :10003, which only works when every point is PART3)
        Xt = X[p3]
        sq = np.sqrt(Xt)
        near = np.abs(sq) <= 4.0e3
        At = np.zeros(Xt.size, dtype=CT)
        if np.any(near):
            At[near] = (2.0 * rpi / c2t) * (1.0 / rpi - sq[near] * cw(-sq[near].imag, sq[near].real))
        if np.any(~near):
            At[~near] = (1.0 / c2t) * (1.0 / Xt[~near] - 1.5 / (Xt[~near] ** 2))
        A[p3] = At
        code[p3] = SD_P3 + SD_P3NEAR * near + SD_W24_1 * (near & w24(sq))
    return ((A / pi).real, code) if branches else (A / pi).real


def _gamma2(sub, r, p, Diluent=None, GammaL="gamma_air"):
    """Gamma2 = sum_species abun * SD_species * p/pref * gamma_species(296 K) of row r (misc/hapi.py:10884-10890)."""
    dil = Diluent if Diluent else ({"air": 1.0} if GammaL.lower() == "gamma_air" else {"self": 1.0})
    Gamma2 = 0.0
    for species, abun in dil.items():
        sp = species.lower()
        sd = float(sub["SD_" + sp][r]) if ("SD_" + sp) in sub else 0.0
        g0db = float(sub["gamma_" + sp][r]) if ("gamma_" + sp) in sub else 0.0
        Gamma2 += abun * (sd * p / PREF) * g0db
    return Gamma2


def sdvoigt_terms(tbl, T=296.0, p=1.0, OmegaGrid=None, OmegaWing=0.0, OmegaWingHW=50.0, IntensityThreshold=0.0,
                  Diluent=None, dtype=np.float64):
    """The line loop of absorptionCoefficient_SDVoigt (HITRAN units, every component at natural abundance) over the
    (line, point) pairs inside the windows, in `dtype` (np.float64: the values of absorptionCoefficient_SDVoigt, bit for
    bit; np.longdouble: the same loop in extended precision). Returns {"xs": the sum, "den": sum_l |S_l profile_l|,
    "lines": [(table row, lo, hi, branch bits of PROFILE_SDVOIGT on Omegas[lo:hi])]}."""
    F = _wide(dtype)[0]
    Omegas = np.sort(np.asarray(OmegaGrid, dtype=np.float64))
    xs, den = np.zeros(Omegas.size, dtype=F), np.zeros(Omegas.size, dtype=F)
    P = line_params(tbl, T, p, Diluent=Diluent)
    nu = np.asarray(tbl["nu"], dtype=np.float64)
    abun = _tables()["abun"]
    glist = Omegas.tolist()
    sg = Omegas.astype(F)
    lines = []
    for r in range(nu.size):
        S = P["S"][r]
        if S < IntensityThreshold:
            continue
        GammaD, Gamma0, Shift0 = P["GammaD"][r], P["Gamma0"][r], P["Shift0"][r]
        W = max(OmegaWing, OmegaWingHW * Gamma0, OmegaWingHW * GammaD)
        lo = _bisect.bisect(glist, nu[r] - W)
        hi = _bisect.bisect(glist, nu[r] + W)
        if hi <= lo:
            continue
        ls, code = PROFILE_SDVOIGT(nu[r], GammaD, Gamma0, _gamma2(tbl, r, p, Diluent), Shift0, 0.0, sg[lo:hi], dtype=dtype,
                                   branches=True)
        nat = abun[(int(P["M"][r]), int(P["I"][r]))]
        term = 1.0 / nat * nat * S * ls  # factor / NAT * ABUN * S * ls, as the float64 loop rounds it
        xs[lo:hi] += term
        den[lo:hi] += np.abs(term)
        lines.append((r, lo, hi, code))
    return {"xs": xs, "den": den, "lines": lines}


def absorptionCoefficient_SDVoigt(tbl, **kw):
    """misc/hapi.py:10657-10904: the Voigt loop with PROFILE_SDVOIGT(nu, GammaD, Gamma0, Gamma2, Shift0, 0, grid) and
    Gamma2 = sum_species abun * SD_species * p/pref * gamma_species(296 K) (:10884-10890)."""
    return absorptionCoefficient_Voigt(tbl, _profile="sdvoigt", **kw)


# ---- the speed-dependent line-sum's classification (rtx_sdvoigt.hip: sd_zones, sdvoigt_tile_kernel) -------------------
# Restated so that host tests can show which path a configuration reaches; not an oracle of values.
SD_TILE, SD_ROWS, SD_TDIST, SD_NEAR, SD_CHUNK = 1024, 16, 256, 2, 256


def sd_zones(Gam0, Gam2, cte, step):
    """sd_zones of rtx_sdvoigt.hip for one record: (a_lo, a_hi, b_lo, b_hi, far4) in cm^-1 from the shifted centre; empty
    zones have lo = +inf. far4 (the PART4 far switch, 0 where d <= 0) is returned for the census, the kernel keeps it local."""
    INF = np.inf
    z = [INF, -INF, INF, -INF, 0.0]
    m = 2.0 * step
    if Gam2 == 0.0:
        if not cte > 0.0:
            return tuple(z)
        z[2] = max(0.0, (15.0 - Gam0 * cte) / cte) + m
        z[3] = INF
        return tuple(z)
    a, c2 = Gam0 - 1.5 * Gam2, Gam2
    inv = 1.0 / Gam2
    sY = 1.0 / (2.0 * cte * Gam2)
    if not (c2 > 0.0) or not (a > 0.0) or not (sY > 0.0) or not (cte > 0.0):
        return tuple(z)
    Y = sY * sY
    K = 15.0 + sY
    K2 = K * K
    R = a * inv + Y
    d = 225.0 + 30.0 * sY - a * inv
    far4 = c2 * ((d * (K2 + R)) / (2.0 * K2)) if d > 0.0 else 0.0
    z[4] = far4
    t2 = 3.0e-8 * Y * c2
    dP2 = np.sqrt(t2 * t2 - a * a) if t2 > a else -1.0
    t3 = 1.0e15 * Y * c2
    if not t3 > a:
        return tuple(z)
    dP3 = np.sqrt(t3 * t3 - a * a)
    z[2] = max(far4, dP2) + m
    z[3] = dP3 - m
    if dP2 > 0.0 and sY >= 8.0:
        z[0] = max(0.0, (15.0 - a * cte) / cte) + m
        z[1] = dP2 - m
    return tuple(z)


def _sd_branch_labels(code):
    """sdvoigt_profile's branch per point from PROFILE_SDVOIGT's branch bits."""
    w1, w2 = (code & SD_W24_1) != 0, (code & SD_W24_2) != 0
    neg = (code & (SD_NEG1 | SD_NEG2)) != 0
    p1, p2, p3, p4 = ((code & b) != 0 for b in (SD_P1, SD_P2, SD_P3, SD_P4))
    cp = (code & SD_CPF3) != 0
    near = (code & SD_P3NEAR) != 0
    far = p4 & ~w1 & ~w2
    rest = p4 & ~far & ~cp
    return {"p1_w24": p1 & w1, "p1_asym": p1 & ~w1, "p2_real": p2 & ~neg, "p2_cplx": p2 & neg, "p3_near": p3 & near,
            "p3_far": p3 & ~near, "p4_far": far, "p4_cpf3": p4 & cp & ~far, "p4_real_in_in": rest & ~neg & w1 & w2,
            "p4_real_in_out": rest & ~neg & (w1 != w2), "p4_cplx": rest & neg}


def sd_census(tbl, grid, T, p, omega_wing=0.0, omega_wing_hw=50.0, intensity_threshold=0.0, Diluent=None):
    """Which paths of sdvoigt_tile_kernel one state reaches: a Counter of labels over (tile, candidate), (line, row) and
    point-by-point (line, point). Candidates of a tile are the lines whose unshifted centre index lies within maxhw of
    it; chunk c holds candidates [256 c, 256 c + 256) of that range. Built on linesum_records."""
    from collections import Counter
    xmin, xmax, n_total, offset, n = grid
    C = Counter()
    R = linesum_records(tbl, grid, float(T), float(p), omega_wing, omega_wing_hw, Diluent)
    P, nu, step, order = R["P"], R["nu"], R["step"], R["order"]
    sub = {k: np.asarray(v)[order] for k, v in tbl.items()}
    nl = nu.size
    Gam2 = np.array([_gamma2(sub, r, float(p), Diluent) for r in range(nl)])
    dropped = P["S"] < intensity_threshold
    lo, hi = np.where(dropped, 0, R["lo"]), np.where(dropped, 0, R["hi"])
    i0 = R["i0"]
    C["dropped"] = int(dropped.sum())
    gic = np.clip(np.rint((nu - xmin) / step), -1e9, 1e9).astype(np.int64)
    ic = np.clip(gic - offset, -100000000, n + 100000000)
    hw_l = np.where(~dropped & (R["ghi"] > R["glo"]), np.minimum(np.ceil(R["W"] / step) + 2.0, 1e9), 0).astype(np.int64)
    maxhw = int(hw_l.max()) if nl else 0
    C["maxhw"] = maxhw

    def gx(i):
        return xmax if i == n_total - 1 else float(i) * step + xmin

    zones = [sd_zones(P["Gamma0"][l], Gam2[l], R["cte"][l], step) for l in range(nl)]
    delta = lambda l, pt: abs((nu[l] - gx(offset + pt)) + P["Shift0"][l])

    def in_zone(z, d0, d1):
        dmin, dmax = min(d0, d1), max(d0, d1)
        if dmin >= z[0] and dmax <= z[1]:
            return "a"
        if dmin >= z[2] and dmax <= z[3]:
            return "b"
        return ""

    X = np.array([gx(offset + i) for i in range(n)])
    codes = {}

    def line_codes(l):
        if l not in codes:
            codes[l] = PROFILE_SDVOIGT(nu[l], P["GammaD"][l], P["Gamma0"][l], Gam2[l], P["Shift0"][l], 0.0, X[lo[l]:hi[l]],
                                       branches=True)[1]
        return codes[l]

    live = hi > lo
    C["covers_grid"] = int(np.sum(live & (lo == 0) & (hi == n)))
    C["narrow"] = int(np.sum(live & (hi - lo < 64) & (lo > 0) & (hi < n)))
    for ia in range(0, n, SD_TILE):
        ib = min(ia + SD_TILE, n)
        first = int(np.searchsorted(ic, ia - maxhw, side="left"))
        last = int(np.searchsorted(ic, ib - 1 + maxhw, side="right"))
        nchunk = (last - first + SD_CHUNK - 1) // SD_CHUNK
        C["chunks_max"] = max(C["chunks_max"], nchunk)
        if nchunk >= 2:
            C["second_chunk"] += 1
        nT, nR = np.zeros(max(nchunk, 1), np.int64), np.zeros(max(nchunk, 1), np.int64)
        for l in range(first, last):
            ch = (l - first) // SD_CHUNK
            if not (hi[l] > ia and lo[l] < ib):
                C["cand_not_reached"] += 1
                if hi[l] == lo[l]:
                    C["cand_dropped" if dropped[l] else "cand_empty_window"] += 1
                continue
            z = zones[l]
            nozones = z[0] == np.inf and z[2] == np.inf
            covers = lo[l] <= ia and hi[l] >= ib
            dl, dr = ia - i0[l], i0[l] - (ia + SD_TILE - 1)
            if covers:
                for d in (255, 256, 257):
                    for side, dist in (("left", dl), ("right", dr)):
                        if dist == d:
                            C["tile_%s_%d" % (side, d)] += 1
            for lab, ok in (("lo_eq_ia", lo[l] == ia and ia > 0), ("lo_eq_ia1", lo[l] == ia + 1), ("hi_eq_ib", hi[l] == ib and ib < n),
                            ("hi_eq_ib1", hi[l] == ib - 1)):
                if ok:
                    C[lab] += 1
            cls = ""
            if covers and (dl >= SD_TDIST or dr >= SD_TDIST):
                cls = in_zone(z, delta(l, ia), delta(l, ia + SD_TILE - 1))
            if covers and (dl >= SD_TDIST or dr >= SD_TDIST) and z[4] > 0.0:
                gap = int(np.ceil((min(delta(l, ia), delta(l, ia + SD_TILE - 1)) - z[4]) / step))
                if gap in (1, 2, 3):  # points from the PART4 far switch to the tile's near end
                    C["tile_switch_gap_%d_%s" % (gap, "tile" if cls else "rows")] += 1
            if not nozones and z[4] == 0.0 and Gam2[l] != 0.0:
                C["zone_b_all_far"] += 1
            if cls:
                C["tile_" + cls] += 1
                nT[ch] += 1
                if ib - ia < SD_TILE:
                    C["ragged_tile"] += 1
                for d in (255, 256, 257):
                    if dl == d or dr == d:
                        C["tile_level_at_%d" % d] += 1
                continue
            C["row_list"] += 1
            nR[ch] += 1
            if covers:
                for d in (255, 256, 257):
                    if dl == d or dr == d:
                        C["row_list_at_%d" % d] += 1
                if (dl >= SD_TDIST or dr >= SD_TDIST) and not nozones:
                    C["row_list_switch_in_tile"] += 1
            rc = (int(i0[l]) - ia) >> 6
            if ia <= i0[l] < ib:
                C["centre_row_%d" % rc] += 1
            elif rc in (-2, -1, 16, 17):
                C["rc_outside"] += 1
                C["rc_outside_%d" % rc] += 1
            for r in range(SD_ROWS):
                pa = ia + 64 * r
                if pa >= ib:
                    break
                pb = min(pa + 63, ib - 1)
                if not (hi[l] > pa and lo[l] <= pb):
                    continue
                full = lo[l] <= pa and hi[l] > pb
                near = abs(r - rc) <= SD_NEAR
                if full and lo[l] == pa and pa > 0:
                    C["row_starts_window"] += 1
                if full and hi[l] == pb + 1 and hi[l] < n:
                    C["row_ends_window"] += 1
                if lo[l] <= pa and hi[l] == pb and not near:
                    C["window_ends_at_row_last_point"] += 1  # hi > pb fails by one: an edge row, its last point outside
                zc = ""
                if full and not near:
                    zc = in_zone(z, delta(l, pa), delta(l, pa + 63))
                if zc:
                    C["row_nodal_" + zc] += 1
                    if abs(r - rc) == SD_NEAR + 1:
                        C["row_nodal_3_from_centre"] += 1
                    if pb < pa + 63:
                        C["ragged_row"] += 1
                    # distance (points, rounded up) from the PART4 far switch to the near end of a nodal row
                    if zc == "b" and z[4] > 0.0:
                        gap = int(np.ceil((min(delta(l, pa), delta(l, pa + 63)) - z[4]) / step))
                        if gap in (2, 3):
                            C["switch_gap_nodal_%d" % gap] += 1
                    continue
                if near:
                    C["row_near"] += 1
                    if abs(r - rc) == SD_NEAR:
                        C["row_near_2_from_centre"] += 1
                elif not full:
                    C["row_edge"] += 1
                elif nozones:
                    C["row_nozones"] += 1
                else:
                    C["row_switch"] += 1
                    if z[4] > 0.0:
                        gap = int(np.ceil((min(delta(l, pa), delta(l, pa + 63)) - z[4]) / step))
                        if gap in (1, 2):
                            C["switch_gap_pointwise_%d" % gap] += 1
                if not full:
                    wl, wh = max(lo[l], pa), min(hi[l], pb + 1)
                    if lo[l] > pa and hi[l] <= pb:
                        C["both_edges_one_row"] += 1
                    elif lo[l] > pa or hi[l] <= pb:
                        C["edge_inside_row"] += 1
                else:
                    wl, wh = pa, pb + 1
                cd = line_codes(l)[wl - lo[l]:wh - lo[l]]
                for lab, sel in _sd_branch_labels(cd).items():
                    if sel.any():
                        C[lab] += int(sel.sum())
        for c in range(nchunk):
            if nT[c] > 0:
                C["nT_%d" % nT[c]] += 1
                C["nT_mod8_%d" % (nT[c] % 8)] += 1
            if nT[c] > 0 and nR[c] > 0:
                C["chunk_mixed"] += 1
            if c > 0 and nT[c] == 0 and nT[:c].any():
                C["chunk_no_tile_after_tile"] += 1
        C["nT_max"] = max(C["nT_max"], int(nT.max()))
        C["nR_max"] = max(C["nR_max"], int(nR.max()))
    return C
