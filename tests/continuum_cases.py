"""Shared inputs of the continuum tests (tests/test_continuum_host.py on the CPU, tests/test_gpu_continuum.py on the device);
no test in here.

The coefficient sets are smooth made-up functions (NOT physical, like continuum.synthetic): what the tests hold the code
to is radtxfr_amd/continuum.py's definition, evaluated in float64 -- by od_host for whole spectra and, to check od_host
itself, by direct_od below: the definition written out with scalar loops and nothing shared with the module."""
import math

import numpy as np

C2 = 1.43877736830  # cm K
P0 = 101325.0
TOL_PIN = 1e-5  # README: "asserted <= 1e-5": relative to the layer's largest continuum value

# three layers; the first sits on T_a and the second on T_b of the sets below
LAYERS = dict(T=np.array([296.0, 260.0, 231.7]), P=np.array([101325.0, 70000.0, 30000.0]), PL=np.array([1.0, 0.5, 2.0]),
              MF=np.array([[1.5e4, 400.0], [8.0e3, 390.0], [100.0, 380.0]]), ID=np.array([1, 2]))


def layers(nL):
    return {k: (v[:nL].copy() if k != "ID" else v.copy()) for k, v in LAYERS.items()}


def shapes(v0, dv, n, seed):
    """Smooth positive node values of three coefficient sets on an axis: an exponential roll-off with a ripple a few
    nodes long (so that the cubic has something to interpolate), a weaker second self set, a foreign set."""
    nu = v0 + dv * np.arange(n)
    k = np.arange(n)
    ph = 0.37 * seed
    Cs_a = 3.0e-22 * np.exp(-(nu - v0) / (40.0 * dv)) * (1.0 + 0.3 * np.sin(k / 2.3 + ph))
    Cs_b = Cs_a * (0.55 + 0.1 * np.cos(k / 3.1 + ph))
    Cf = 4.0e-24 * np.exp(-(nu - v0) / (55.0 * dv)) * (1.0 + 0.4 * np.cos(k / 1.9 + ph))
    return Cs_a, Cs_b, Cf


def component(cont_mod, molecule, v0, dv, n, seed, kind="full"):
    """kind: full (Cs_a, Cs_b, Cf), self (Cs_a only), foreign (Cf only), steps (Cf with runs of exact zeros: the cubic
    undershoots next to them and max(0, .) cuts it; Cs_a / Cs_b zero on the same nodes)."""
    Cs_a, Cs_b, Cf = shapes(v0, dv, n, seed)
    if kind == "self":
        return cont_mod.Continuum.from_arrays(molecule, v0, dv, Cs_a=Cs_a, T_a=296.0)
    if kind == "foreign":
        return cont_mod.Continuum.from_arrays(molecule, v0, dv, Cf=Cf)
    if kind == "steps":
        z = (np.arange(n) // 3) % 2 == 1
        Cs_a, Cs_b, Cf = (np.where(z, 0.0, a) for a in (Cs_a, Cs_b, 60.0 * Cf))
    return cont_mod.Continuum.from_arrays(molecule, v0, dv, Cs_a=Cs_a, T_a=296.0, Cs_b=Cs_b, T_b=260.0, Cf=Cf)


# ---- the grids of the device tests: (xmin, step, points of the whole axis) and the components that go with them -----------
N_AXIS = 2051  # two tiles of 1024 points and three more
GRIDS = {
    # the fp32 abscissa: nu near 6000 with a step of 0.001, 500 points per node cell
    "fine": dict(xmin=5990.0, step=0.001,
                 comps=[(1, 5985.0, 0.5, 40, "full"),        # covers the axis
                        (2, 5990.7003, 0.3, 4, "steps")]),   # four nodes, 5990.7003 .. 5991.6003: part of the axis
    # a step of 1.0014 across many nodes: neighbouring lanes sit on different stencils
    "coarse": dict(xmin=5000.0, step=1.0014,
                   comps=[(1, 4990.0, 10.0, 215, "full"),    # covers the axis
                          (2, 5500.5, 7.3, 100, "steps")]),  # 5500.5 .. 6223.2: part of the axis
}


def grid_args(name):
    g = GRIDS[name]
    return g["xmin"], g["xmin"] + g["step"] * (N_AXIS - 1), N_AXIS


def continuum(cont_mod, name, n_comp):
    cs = [component(cont_mod, m, v0, dv, n, seed=3 + i, kind=kind) for i, (m, v0, dv, n, kind) in enumerate(GRIDS[name]["comps"][:n_comp])]
    return cs[0] if n_comp == 1 else cs[0] + cs[1]


# ---- the definition, written out ---------------------------------------------------------------------------------------------
def direct_od(comps, nu, T, P_pa, PL_km, mf_row, ids):
    """OD of ONE layer at ONE wavenumber: comps is a list of dicts(molecule, v0, dv, Cs_a, T_a, Cs_b, T_b, Cf) with None for
    what is absent; T_ref = 296, p_ref = 1 atm. Plain Python floats."""
    total = 0.0
    p = P_pa / P0
    for c in comps:
        n = len(c["Cs_a"] if c["Cs_a"] is not None else c["Cf"])
        v0, dv = c["v0"], c["dv"]
        if not (v0 <= nu <= v0 + (n - 1) * dv):
            continue
        x = mf_row[list(ids).index(c["molecule"])] * 1e-6
        W = (p / 9.869233e-7) / (1.380648813e-16 * T) * x * PL_km * 1e5
        A = []
        for j in range(n):
            cs = 0.0
            if c["Cs_a"] is not None:
                cs = c["Cs_a"][j]
                if c["Cs_b"] is not None and c["Cs_a"][j] > 0.0 and c["Cs_b"][j] > 0.0:
                    cs = c["Cs_a"][j] * (c["Cs_b"][j] / c["Cs_a"][j]) ** ((T - c["T_a"]) / (c["T_b"] - c["T_a"]))
            cf = c["Cf"][j] if c["Cf"] is not None else 0.0
            A.append(W * (p / 1.0) * (296.0 / T) * (x * cs + (1.0 - x) * cf))
        j0 = min(max(int(math.floor((nu - v0) / dv)) - 1, 0), n - 4)
        t = (nu - (v0 + j0 * dv)) / dv
        L = [-(t - 1) * (t - 2) * (t - 3) / 6.0, t * (t - 2) * (t - 3) / 2.0, -t * (t - 1) * (t - 3) / 2.0, t * (t - 1) * (t - 2) / 6.0]
        R = nu * math.tanh(C2 * nu / (2.0 * T))
        total += max(0.0, R * sum(L[k] * A[j0 + k] for k in range(4)))
    return total


def as_dicts(cont):
    return [dict(molecule=c.molecule, v0=c.v0, dv=c.dv, Cs_a=c.Cs_a, T_a=c.T_a, Cs_b=c.Cs_b, T_b=c.T_b, Cf=c.Cf) for c in cont.components]
