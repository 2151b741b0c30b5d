"""Tabulated continuum absorption: the definition, on the host in float64.

LBLRTM, which gave the reference its optical depths, adds the collision-induced continua (H2O self and foreign, CO2, N2,
O2: the MT_CKD model) to its line sum; `write_tape5` switches them on (radiative_transfer.py:591-601). The coefficient
data are not part of this package: the USER supplies the tables, as for afit_xs.XsLut, and this module defines what is
computed from them. The form is MT_CKD's, so its coefficient files load with a change of units at most.

A Continuum is a list of components and holds no device state. A component has a molecule (HITRAN id of the absorber), a
uniform node axis nu_j = v0 + j dv (j < n, n >= 4, dv > 0) and on it, in cm^2 molecule^-1 (cm^-1)^-1 at the reference
density (T_ref = 296 K, p_ref = 1 atm):
    Cs_a[n]   self coefficients at T_a,
    Cs_b[n]   optional, self coefficients at T_b != T_a,
    Cf[n]     optional, foreign coefficients;
at least one of Cs_a and Cf. For layer l with T, p = P / 101325 and x = MF_VAL[l][m] 1e-6 the component's optical depth is

    Cs(nu_j; T) = Cs_a[j] (Cs_b[j] / Cs_a[j]) ** ((T - T_a) / (T_b - T_a))      (Cs_a[j] without Cs_b, or where both are 0)
    A_l[j]      = W_l (p / p_ref) (T_ref / T) (x Cs(nu_j; T) + (1 - x) Cf[j])
    R(nu, T)    = nu tanh(c2 nu / (2 T))
    OD_l(nu)    = max(0, R(nu, T_l) sum_{k<4} L_k(t) A_l[j0 + k])               for v0 <= nu <= v0 + (n - 1) dv, else 0
    j0 = clamp(floor((nu - v0) / dv) - 1, 0, n - 4),  t = (nu - nu_j0) / dv,  L_k the cubic Lagrange basis on nodes 0..3

with W_l = n(p, T) x PL 1e5 the weight engine.layer_weights_od gives the molecule and c2 = rt.c2 in cm K. The total is the
sum over the components in list order. A component whose molecule MF_ID lacks raises ValueError: a silent zero would hide
a misconfigured call.

Continuum.layer_tables makes the float32 rows A the device kernel reads (rtx_continuum_add, engine.continuum_add);
Continuum.od_host evaluates the definition in NumPy from the float64 A and is what the tests hold the device to.

Derivatives. With S the stencil sum above, g = (p / p_ref) (T_ref / T) and N = n(p, T) PL 1e5:
    dA_l[j]/dT  = -2 A_l[j] / T + W_l g x Cs(nu_j; T) ln(Cs_b[j] / Cs_a[j]) / (T_b - T_a)     (second term 0 without Cs_b)
    dA_l[j]/dMF = 1e-6 N g (2 x Cs(nu_j; T) + (1 - 2 x) Cf[j])                                 per ppmv, finite at MF = 0
    dOD/dT = m (R_T S + R S_T),   dOD/dMF = m R S_x,   m = [S > 0],   R_T = -nu (c2 nu / (2 T^2)) sech^2(c2 nu / (2 T))
with S_T and S_x the same stencil and weights on dA/dT and dA/dMF. Where S <= 0, and outside the axis, both are exactly 0:
the kink of max(0, .) at S = 0 is given the value 0. A component differentiates only with respect to its own molecule's
mixing ratio. Continuum.layer_tables_d makes the three float32 tables rtx_continuum_add_d reads (engine.continuum_add_d);
Continuum.dod_host is the definition in NumPy float64 and the oracle of the derivative tests.
"""
import numpy as np

from . import engine

C2_CM_K = 1.43877736830  # rt.c2 (radiative_transfer.py:72, m K) in cm K
T_REF = 296.0
P_REF_ATM = 1.0

_ARRAYS = ("Cs_a", "Cs_b", "Cf")
_SCALARS = ("molecule", "v0", "dv", "n", "T_a", "T_b", "T_ref", "p_ref_atm")


class Component:
    """One absorber's coefficient set on one node axis; validated on construction (ValueError), then read-only."""

    def __init__(self, molecule, v0, dv, Cs_a=None, T_a=T_REF, Cs_b=None, T_b=None, Cf=None, T_ref=T_REF, p_ref_atm=P_REF_ATM):
        self.molecule = int(molecule)
        self.v0, self.dv = float(v0), float(dv)
        self.T_a, self.T_ref, self.p_ref_atm = float(T_a), float(T_ref), float(p_ref_atm)
        self.T_b = None if T_b is None else float(T_b)
        arr = {}
        for name, a in (("Cs_a", Cs_a), ("Cs_b", Cs_b), ("Cf", Cf)):
            if a is not None:
                a = np.array(a, dtype=np.float64)
                if a.ndim != 1:
                    raise ValueError("continuum: %s must be one-dimensional, got shape %r" % (name, a.shape))
                a.setflags(write=False)
            arr[name] = a
        self.Cs_a, self.Cs_b, self.Cf = arr["Cs_a"], arr["Cs_b"], arr["Cf"]
        if self.Cs_a is None and self.Cf is None:
            raise ValueError("continuum: molecule %d: at least one of Cs_a and Cf must be given" % self.molecule)
        given = [a for a in (self.Cs_a, self.Cs_b, self.Cf) if a is not None]
        self.n = int(given[0].size)
        if any(a.size != self.n for a in given):
            raise ValueError("continuum: molecule %d: Cs_a, Cs_b and Cf must have one length, got %r" % (self.molecule, [a.size for a in given]))
        if self.n < 4:
            raise ValueError("continuum: molecule %d: the node axis needs n >= 4 nodes (a cubic stencil), got %d" % (self.molecule, self.n))
        if not (np.isfinite(self.v0) and np.isfinite(self.dv) and self.dv > 0.0):
            raise ValueError("continuum: molecule %d: v0=%r must be finite and dv=%r > 0" % (self.molecule, self.v0, self.dv))
        for name, a in arr.items():
            if a is not None and not (np.all(np.isfinite(a)) and a.min() >= 0.0):
                raise ValueError("continuum: molecule %d: %s must be finite and >= 0" % (self.molecule, name))
        if not (np.isfinite(self.T_ref) and self.T_ref > 0.0 and np.isfinite(self.p_ref_atm) and self.p_ref_atm > 0.0):
            raise ValueError("continuum: molecule %d: T_ref=%r and p_ref_atm=%r must be > 0" % (self.molecule, self.T_ref, self.p_ref_atm))
        if self.Cs_b is not None:
            if self.Cs_a is None:
                raise ValueError("continuum: molecule %d: Cs_b needs Cs_a" % self.molecule)
            if self.T_b is None or not (np.isfinite(self.T_b) and np.isfinite(self.T_a)) or self.T_b == self.T_a:
                raise ValueError("continuum: molecule %d: Cs_b needs T_b != T_a, got T_a=%r T_b=%r" % (self.molecule, self.T_a, self.T_b))
            if np.any((self.Cs_a > 0.0) != (self.Cs_b > 0.0)):
                j = int(np.flatnonzero((self.Cs_a > 0.0) != (self.Cs_b > 0.0))[0])
                raise ValueError("continuum: molecule %d: Cs_a[j] > 0 must hold exactly where Cs_b[j] > 0 (node %d: %r, %r)"
                                 % (self.molecule, j, self.Cs_a[j], self.Cs_b[j]))
        elif self.T_b is not None:
            raise ValueError("continuum: molecule %d: T_b=%r without Cs_b" % (self.molecule, self.T_b))

    @property
    def vend(self):
        """The last wavenumber inside: v0 + (n - 1) dv, product then sum (what the kernel's host side forms)."""
        return self.v0 + float(self.n - 1) * self.dv

    def self_coefficients(self, T):
        """Cs(nu_j; T) float64 [n] (zeros without Cs_a)."""
        if self.Cs_a is None:
            return np.zeros(self.n)
        if self.Cs_b is None:
            return self.Cs_a.copy()
        pos = self.Cs_a > 0.0
        ratio = np.where(pos, self.Cs_b, 1.0) / np.where(pos, self.Cs_a, 1.0)
        return self.Cs_a * ratio ** ((float(T) - self.T_a) / (self.T_b - self.T_a))

    def layer_rows(self, T, P_pa, PL_km, MF_VAL, MF_ID):
        """A float64 [nL][n] of the definition."""
        T = np.atleast_1d(np.asarray(T, dtype=np.float64))
        ids = [int(v) for v in np.asarray(MF_ID).ravel()]
        if self.molecule not in ids:
            raise ValueError("continuum: component molecule %d is not in MF_ID %r" % (self.molecule, ids))
        MF = np.asarray(MF_VAL, dtype=np.float64).reshape(T.size, -1)
        W, p_atm = engine.layer_weights_od([(self.molecule, 1)], T, np.atleast_1d(P_pa), np.atleast_1d(PL_km), MF, ids)
        x = MF[:, ids.index(self.molecule)] * 1e-6
        Cf = self.Cf if self.Cf is not None else np.zeros(self.n)
        A = np.empty((T.size, self.n))
        for l in range(T.size):
            A[l] = W[0, l] * (p_atm[l] / self.p_ref_atm) * (self.T_ref / T[l]) * (x[l] * self.self_coefficients(T[l]) + (1.0 - x[l]) * Cf)
        return A

    def od_rows(self, X, T, A):
        """The component's optical depths float64 [nL][nX] from its float64 rows A."""
        X = np.asarray(X, dtype=np.float64).ravel()
        T = np.atleast_1d(np.asarray(T, dtype=np.float64))
        inside = (X >= self.v0) & (X <= self.vend)
        j0 = np.clip(np.floor((X - self.v0) / self.dv).astype(np.int64) - 1, 0, self.n - 4)
        j0[~inside] = 0
        t = (X - (self.v0 + j0 * self.dv)) / self.dv
        Lk = (-(t - 1.0) * (t - 2.0) * (t - 3.0) / 6.0, t * (t - 2.0) * (t - 3.0) / 2.0, -t * (t - 1.0) * (t - 3.0) / 2.0,
              t * (t - 1.0) * (t - 2.0) / 6.0)
        out = np.zeros((T.size, X.size))
        for l in range(T.size):
            S = sum(Lk[k] * A[l, j0 + k] for k in range(4))
            R = X * np.tanh(C2_CM_K * X / (2.0 * T[l]))
            out[l] = np.where(inside, np.maximum(0.0, R * S), 0.0)
        return out

    def self_coefficients_dT(self, T):
        """d Cs(nu_j; T) / dT float64 [n]: Cs(T) ln(Cs_b / Cs_a) / (T_b - T_a); 0 without Cs_b and where both are 0."""
        if self.Cs_a is None or self.Cs_b is None:
            return np.zeros(self.n)
        pos = self.Cs_a > 0.0
        ratio = np.where(pos, self.Cs_b, 1.0) / np.where(pos, self.Cs_a, 1.0)
        return self.self_coefficients(T) * (np.log(ratio) / (self.T_b - self.T_a))

    def layer_rows_d(self, T, P_pa, PL_km, MF_VAL, MF_ID):
        """(A, A_T, A_x) float64 [nL][n]: layer_rows' A (the same operations: the same bits), dA/dT per K and dA/dMF per ppmv
        of the component's own molecule. With g = (p / p_ref) (T_ref / T) and N = n(p, T) PL 1e5 (so W = N x, n ~ 1/T):
            A_T = -2 A / T + W g x dCs/dT,        A_x = 1e-6 N g (2 x Cs(T) + (1 - 2 x) Cf),
        the second formed without a division by x: MF = 0 gives its finite value N g Cf 1e-6."""
        T = np.atleast_1d(np.asarray(T, dtype=np.float64))
        ids = [int(v) for v in np.asarray(MF_ID).ravel()]
        if self.molecule not in ids:
            raise ValueError("continuum: component molecule %d is not in MF_ID %r" % (self.molecule, ids))
        MF = np.asarray(MF_VAL, dtype=np.float64).reshape(T.size, -1)
        P_pa, PL_km = np.atleast_1d(P_pa), np.atleast_1d(PL_km)
        W, p_atm = engine.layer_weights_od([(self.molecule, 1)], T, P_pa, PL_km, MF, ids)
        N = engine.volumeConcentration(p_atm, T) * np.asarray(PL_km, dtype=np.float64) * 1e5
        x = MF[:, ids.index(self.molecule)] * 1e-6
        Cf = self.Cf if self.Cf is not None else np.zeros(self.n)
        A, A_T, A_x = (np.empty((T.size, self.n)) for _ in range(3))
        for l in range(T.size):
            g = (p_atm[l] / self.p_ref_atm) * (self.T_ref / T[l])
            Cs = self.self_coefficients(T[l])
            A[l] = W[0, l] * (p_atm[l] / self.p_ref_atm) * (self.T_ref / T[l]) * (x[l] * Cs + (1.0 - x[l]) * Cf)
            A_T[l] = -2.0 / T[l] * A[l] + W[0, l] * g * (x[l] * self.self_coefficients_dT(T[l]))
            A_x[l] = 1e-6 * N[l] * g * (2.0 * x[l] * Cs + (1.0 - 2.0 * x[l]) * Cf)
        return A, A_T, A_x

    def stencil(self, X):
        """(inside [nX] bool, j0 [nX], (L_0 .. L_3) each [nX]) of the definition at the wavenumbers X, float64."""
        X = np.asarray(X, dtype=np.float64).ravel()
        inside = (X >= self.v0) & (X <= self.vend)
        j0 = np.clip(np.floor((X - self.v0) / self.dv).astype(np.int64) - 1, 0, self.n - 4)
        j0[~inside] = 0
        t = (X - (self.v0 + j0 * self.dv)) / self.dv
        Lk = (-(t - 1.0) * (t - 2.0) * (t - 3.0) / 6.0, t * (t - 2.0) * (t - 3.0) / 2.0, -t * (t - 1.0) * (t - 3.0) / 2.0,
              t * (t - 1.0) * (t - 2.0) / 6.0)
        return inside, j0, Lk

    def dod_rows(self, X, T, A, A_T, A_x):
        """(dOD/dT, dOD/dMF) float64 [nL][nX] of the component from its float64 rows (layer_rows_d): with S the stencil sum
        of od_rows, S_T and S_x the same stencil and weights on A_T and A_x, R_T = dR/dT = -nu (c2 nu / (2 T^2)) sech^2(c2 nu /
        (2 T)) and m = [S > 0] inside the axis (decided as od_rows decides it, on R S),
            dOD/dT = m (R_T S + R S_T),        dOD/dMF = m R S_x.
        Where S <= 0 (max(0, .) cut the cubic's undershoot) and outside the axis both are exactly 0: the kink at S = 0 is
        given the value 0."""
        X = np.asarray(X, dtype=np.float64).ravel()
        T = np.atleast_1d(np.asarray(T, dtype=np.float64))
        inside, j0, Lk = self.stencil(X)
        dT, dx = np.zeros((T.size, X.size)), np.zeros((T.size, X.size))
        for l in range(T.size):
            S, S_T, S_x = (sum(Lk[k] * a[l, j0 + k] for k in range(4)) for a in (A, A_T, A_x))
            h = C2_CM_K * X / (2.0 * T[l])
            R = X * np.tanh(h)
            R_T = -X * (h / T[l]) / np.cosh(h) ** 2
            m = inside & (R * S > 0.0)
            dT[l] = np.where(m, R_T * S + R * S_T, 0.0)
            dx[l] = np.where(m, R * S_x, 0.0)
        return dT, dx


class Continuum:
    """A list of Components, evaluated in list order. Continuum.from_arrays(...) makes one component; `a + b` joins lists."""

    def __init__(self, components):
        self.components = tuple(components)
        if not self.components or not all(isinstance(c, Component) for c in self.components):
            raise ValueError("Continuum: a non-empty sequence of continuum.Component")

    @classmethod
    def from_arrays(cls, molecule, v0, dv, Cs_a=None, T_a=T_REF, Cs_b=None, T_b=None, Cf=None, T_ref=T_REF, p_ref_atm=P_REF_ATM):
        """One component from its arrays (module docstring); ValueError for anything the definition excludes."""
        return cls([Component(molecule, v0, dv, Cs_a=Cs_a, T_a=T_a, Cs_b=Cs_b, T_b=T_b, Cf=Cf, T_ref=T_ref, p_ref_atm=p_ref_atm)])

    def __add__(self, other):
        if not isinstance(other, Continuum):
            return NotImplemented
        return Continuum(self.components + other.components)

    def __len__(self):
        return len(self.components)

    def save(self, path):
        """One .npz of arrays and scalars (no pickled objects): n_components and, per component i, c<i>_<field>."""
        out = {"n_components": np.int64(len(self.components))}
        for i, c in enumerate(self.components):
            for k in _SCALARS:
                v = getattr(c, k)
                if v is not None:
                    out["c%d_%s" % (i, k)] = np.int64(v) if k in ("molecule", "n") else np.float64(v)
            for k in _ARRAYS:
                if getattr(c, k) is not None:
                    out["c%d_%s" % (i, k)] = getattr(c, k)
        with open(path, "wb") as f:
            np.savez(f, **out)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            comps = []
            for i in range(int(z["n_components"])):
                def get(k, i=i):
                    return z["c%d_%s" % (i, k)] if "c%d_%s" % (i, k) in z.files else None
                T_b = get("T_b")
                comps.append(Component(int(get("molecule")), float(get("v0")), float(get("dv")), Cs_a=get("Cs_a"), T_a=float(get("T_a")),
                                       Cs_b=get("Cs_b"), T_b=None if T_b is None else float(T_b), Cf=get("Cf"),
                                       T_ref=float(get("T_ref")), p_ref_atm=float(get("p_ref_atm"))))
        return cls(comps)

    def axes(self):
        """[(v0, dv, n)] per component."""
        return [(c.v0, c.dv, c.n) for c in self.components]

    def layer_rows(self, T, P_pa, PL_km, MF_VAL, MF_ID):
        """The float64 A of every component: a list of [nL][n_c]."""
        return [c.layer_rows(T, P_pa, PL_km, MF_VAL, MF_ID) for c in self.components]

    def layer_tables(self, T, P_pa, PL_km, MF_VAL, MF_ID):
        """(float32 [nC][nL][n_max], [(v0, dv, n)]): A formed in float64 and rounded once; the columns past a component's n
        are 0 and read by nobody."""
        rows = self.layer_rows(T, P_pa, PL_km, MF_VAL, MF_ID)
        tab = np.zeros((len(rows), rows[0].shape[0], max(r.shape[1] for r in rows)), dtype=np.float32)
        for i, r in enumerate(rows):
            tab[i, :, :r.shape[1]] = r
        return tab, self.axes()

    def od_host(self, X, T, P_pa, PL_km, MF_VAL, MF_ID):
        """The definition in NumPy: float64 [nL][nX], evaluated from the float64 A, components summed in list order."""
        X = np.asarray(X, dtype=np.float64).ravel()
        T = np.atleast_1d(np.asarray(T, dtype=np.float64))
        out = np.zeros((T.size, X.size))
        for c, A in zip(self.components, self.layer_rows(T, P_pa, PL_km, MF_VAL, MF_ID)):
            out += c.od_rows(X, T, A)
        return out

    def layer_rows_d(self, T, P_pa, PL_km, MF_VAL, MF_ID):
        """The float64 (A, A_T, A_x) of every component: a list of triples of [nL][n_c] (Component.layer_rows_d)."""
        return [c.layer_rows_d(T, P_pa, PL_km, MF_VAL, MF_ID) for c in self.components]

    def layer_tables_d(self, T, P_pa, PL_km, MF_VAL, MF_ID):
        """(A, A_T, A_x, [(v0, dv, n)]): three float32 [nC][nL][n_max] arrays laid out as layer_tables lays out its one, each
        formed in float64 and rounded once; A is layer_tables' A bit for bit. What rtx_continuum_add_d reads
        (engine.continuum_add_d)."""
        rows = self.layer_rows_d(T, P_pa, PL_km, MF_VAL, MF_ID)
        shape = (len(rows), rows[0][0].shape[0], max(r[0].shape[1] for r in rows))
        tabs = tuple(np.zeros(shape, dtype=np.float32) for _ in range(3))
        for i, r in enumerate(rows):
            for tab, a in zip(tabs, r):
                tab[i, :, :a.shape[1]] = a
        return tabs + (self.axes(),)

    def dod_host(self, X, T, P_pa, PL_km, MF_VAL, MF_ID):
        """The derivatives of od_host in NumPy, float64: (dOD_dT [nL][nX] per K, {molecule: dOD_dMF [nL][nX] per ppmv}), of
        each layer's optical depth with respect to that layer's temperature and to its mixing ratio of each molecule that
        has a component (a component differentiates only with respect to its own molecule; several components of one
        molecule are summed into that molecule's entry). Components are summed in list order. Piecewise: where a
        component's stencil sum is <= 0, and outside its axis, its derivatives are exactly 0 (Component.dod_rows: the kink
        of max(0, .) is given the value 0)."""
        X = np.asarray(X, dtype=np.float64).ravel()
        T = np.atleast_1d(np.asarray(T, dtype=np.float64))
        dT = np.zeros((T.size, X.size))
        dMF = {}
        for c, (A, A_T, A_x) in zip(self.components, self.layer_rows_d(T, P_pa, PL_km, MF_VAL, MF_ID)):
            d_T, d_x = c.dod_rows(X, T, A, A_T, A_x)
            dT += d_T
            if c.molecule in dMF:
                dMF[c.molecule] += d_x
            else:
                dMF[c.molecule] = d_x
        return dT, dMF


def synthetic(molecule=1, v0=0.0, dv=10.0, n=701, foreign=True):
    """A smooth, MADE-UP coefficient set for tests and timing: an exponential roll-off in nu with a slow ripple, a weaker
    set at T_b = 260 K and (foreign=True) a foreign set two orders below. It is NOT PHYSICAL: the numbers come from no
    measurement or model, and nothing computed with it says anything about an atmosphere. Real work loads MT_CKD-style
    tables through Continuum.from_arrays."""
    nu = float(v0) + np.arange(int(n), dtype=np.float64) * float(dv)
    Cs_a = 2.0e-22 * np.exp(-nu / 250.0) * (1.0 + 0.3 * np.sin(nu / 170.0))
    Cs_b = Cs_a * (0.55 + 0.1 * np.cos(nu / 410.0))
    Cf = 2.0e-24 * np.exp(-nu / 300.0) * (1.0 + 0.5 * np.cos(nu / 90.0)) if foreign else None
    return Continuum.from_arrays(molecule, v0, dv, Cs_a=Cs_a, T_a=296.0, Cs_b=Cs_b, T_b=260.0, Cf=Cf)
