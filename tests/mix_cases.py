"""Line tables, layers and diluent mixes that put the mixed prologue (rtx_lines.hip: line_phys<MIX = true>, dil_cols, dil_sd;
rtx_lines_set_broadeners; rtx_line_prep_mix / _axis_mix; engine.diluent_mix; LineTable.broadener_sets) on one thing at a
time with FOREIGN broadener column sets (set index >= 2), and the fp64 definition of what each case must give. Imported
by the host test (tests/test_mix_host.py: each case reaches what it names and can tell every defect of MUTATIONS from the
definition) and by the GPU test (tests/test_gpu_mix_paths.py), so the two cannot drift apart. No torch import.

A case is a dict: tbl (linesum_cases.table-style columns plus broadener columns), grid (xmin, xmax, n_total, offset, n) or
X (explicit axis), T[nL], p[nL] (atm), profile (0 Voigt, 1 Lorentz, 3 speed-dependent Voigt), ow / hw (OmegaWing /
OmegaWingHW), diluent (ordered dict name -> [nS][nL] fractions, species in sorted (molec_id, local_iso_id) order: the
order of engine.LineTable.species) and expect (labels of `reach` that must be non-zero). Centres sit a quarter step past a
grid point (linesum_cases.at). 12 - 40 lines, 3 species of two molecules (two Doppler factors) except m_device_tables
(7), 1 - 4 layers (m_device_tables: 40), at most 2100 points per run except m_shard, whose full grid is the two tiles +
577 points its name needs (the shard itself has 1601).

definition(case, mutate=None): per layer and species the reference's absorptionCoefficient_Voigt / _Lorentz with
Components = [species] and Diluent = {name: fraction of (species, layer)}, summed over species (every species at weight 1:
natural abundance in HITRAN units); for profile 3 the float64 run of cpu_ref.sdvoigt_terms (sd_reference gives the dict
sdvoigt_cases.judge takes, with the long-double run). `mutate` names one defect of MUTATIONS, applied to the inputs -- the
fraction blocks or the table's columns -- before the oracle runs; the oracle itself is untouched."""
from collections import OrderedDict

import numpy as np

from oracle import cpu_ref

import linesum_cases as LC
import sdvoigt_cases as SC

TILE = 1024
SPECIES3 = [(1, 1), (1, 2), (2, 1)]
SPECIES7 = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (5, 1), (6, 1)]  # test_gpu_prep_consts.SPECIES7
FIELDS = ("gamma_", "n_", "delta_", "deltap_", "SD_")
# value ranges of a foreign set's columns: apart from set to set, so that a set taken for its neighbour shows
_RANGES = {"h2": (0.03, 0.06, 0.30, 0.45), "he": (0.012, 0.03, 0.15, 0.30), "co2": (0.08, 0.13, 0.60, 0.80),
           "n2": (0.05, 0.09, 0.70, 0.85), "o2": (0.02, 0.05, 0.45, 0.60)}


def species_of(tbl):
    """Sorted distinct (molec_id, local_iso_id): engine.LineTable.species."""
    return sorted(set(zip(np.asarray(tbl["molec_id"]).tolist(), np.asarray(tbl["local_iso_id"]).tolist())))


def mix_table(nu, seed, species=SPECIES3, foreign=(), shifts=False, sw=1e-20):
    """linesum_cases.table on the centres `nu`, species dealt round-robin, per-line gamma_air / gamma_self / n_air /
    n_self, and gamma_<sp> / n_<sp> (with `shifts`: delta_<sp> / deltap_<sp> too, and delta_self, deltap_air, deltap_self)
    for every sp of `foreign`."""
    nu = np.atleast_1d(np.asarray(nu, dtype=np.float64))
    n = nu.size
    rng = np.random.default_rng(seed)
    t = LC.table(nu, np.round(rng.uniform(0.04, 0.08, n), 4), sw)
    t["molec_id"] = np.array([species[i % len(species)][0] for i in range(n)], dtype=np.int64)
    t["local_iso_id"] = np.array([species[i % len(species)][1] for i in range(n)], dtype=np.int64)
    t["gamma_self"] = np.round(rng.uniform(0.10, 0.16, n), 3)
    t["n_air"] = np.round(rng.uniform(0.55, 0.75, n), 2)
    t["n_self"] = np.round(rng.uniform(0.35, 0.50, n), 2)
    for sp in foreign:
        g0, g1, n0, n1 = _RANGES[sp]
        t["gamma_" + sp] = np.round(rng.uniform(g0, g1, n), 4)
        t["n_" + sp] = np.round(rng.uniform(n0, n1, n), 2)
    if shifts:
        for sp in ("self",) + tuple(foreign):
            t["delta_" + sp] = np.round(rng.uniform(-0.008, 0.004, n), 6)
        for sp in ("air", "self") + tuple(foreign):
            t["deltap_" + sp] = np.round(rng.uniform(2e-5, 9e-5, n) * rng.choice([-1.0, 1.0], n), 7)
    return t


def fractions(names, nS, nL, seed, total=1.0):
    """Ordered dict name -> [nS][nL], every entry of the whole block distinct, each (species, layer) summing to ~total."""
    rng = np.random.default_rng(seed)
    raw = rng.uniform(0.4, 2.0, (len(names), nS, nL))
    f = np.round(total * raw / raw.sum(axis=0), 6)
    assert np.unique(f).size == f.size
    return OrderedDict((nm, f[d].copy()) for d, nm in enumerate(names))


def _case(tbl, T, p, diluent, grid=None, X=None, profile=0, ow=0.0, hw=4.0, expect=()):
    T, p = np.broadcast_arrays(np.atleast_1d(np.asarray(T, dtype=np.float64)), np.atleast_1d(np.asarray(p, dtype=np.float64)))
    nS, nL = len(species_of(tbl)), T.size
    dil = OrderedDict((nm, np.broadcast_to(np.asarray(v, dtype=np.float64), (nS, nL)).copy()) for nm, v in diluent.items())
    c = dict(tbl=tbl, T=T.copy(), p=p.copy(), profile=int(profile), ow=float(ow), hw=float(hw), diluent=dil, expect=tuple(expect))
    if X is not None:
        c["X"] = np.ascontiguousarray(X, dtype=np.float64)
    else:
        c["grid"] = grid
    return c


def case_axis(case, g=None):
    """The wavenumbers the case (or the shard g of its grid) is evaluated on: X, or the library's grid formula."""
    if "X" in case and g is None:
        return case["X"]
    return SC.axis(g or case["grid"])


def frac_block(case):
    """[n_dil][nS][nL] in the dict's order."""
    return np.stack([case["diluent"][nm] for nm in case["diluent"]])


def layer_params(case, k, s=None, tbl=None, diluent=None):
    """cpu_ref.line_params of layer k for the lines of species index s (None: per species, concatenated in species order
    -> dict of arrays plus "species" = species index per row and "row" = table row)."""
    tbl = case["tbl"] if tbl is None else tbl
    dil = case["diluent"] if diluent is None else diluent
    sp = species_of(tbl)
    out = {}
    for j in (range(len(sp)) if s is None else [s]):
        rows = np.flatnonzero((np.asarray(tbl["molec_id"]) == sp[j][0]) & (np.asarray(tbl["local_iso_id"]) == sp[j][1]))
        sub = {key: np.asarray(v)[rows] for key, v in tbl.items()}
        P = cpu_ref.line_params(sub, float(case["T"][k]), float(case["p"][k]), Diluent={nm: float(v[j, k]) for nm, v in dil.items()})
        P = dict(P, species=np.full(rows.size, j), row=rows, nu=np.asarray(sub["nu"], dtype=np.float64))
        for key, v in P.items():
            out.setdefault(key, []).append(np.asarray(v))
    return {key: np.concatenate(v) for key, v in out.items()}


def _wide_case(nu_idx, seed, names, foreign, T, p, n_total=2100, shifts=False, hw=4.0, profile=0, expect=(), fseed=None):
    g = LC.grid(1000.0, 1e-3, n_total)
    tbl = mix_table(LC.at(g, nu_idx), seed, foreign=foreign, shifts=shifts)
    dil = fractions(names, 3, np.size(T), seed + 100 if fseed is None else fseed)
    return _case(tbl, T, p, dil, grid=g, profile=profile, hw=hw, expect=expect)


T3, P3 = (296.0, 250.0, 220.0), (1.0, 0.06, 0.008)
T4, P4 = (296.0, 270.0, 245.0, 220.0), (1.0, 0.3, 0.05, 0.008)
_IDX18 = np.array([812, 845, 871, 902, 930, 968, 1001, 1037, 1060, 1093, 1122, 1150, 1184, 1210, 1243, 1270, 1301, 1333])


def _cases():
    C = OrderedDict()
    # the position d in the dict never equals the column set: co2 (set 4) first, air (0), he (3), self (1), h2 (2)
    C["m_sets_order"] = _wide_case(_IDX18, 21, ("co2", "air", "he", "self", "h2"), ("h2", "he", "co2"), T3, P3, shifts=True,
                                   expect=("y_ge_1", "y_lt_1", "foreign_sets_3", "position_ne_set", "structural_zeros"))
    C["m_sets_order"]["sets"] = ("h2", "he", "co2")  # the table holds them in this order (sets 2, 3, 4) before the call
    # nS = 3 != nL = 4, every (d, s, k) distinct, a few exact zeros for one diluent
    c = _wide_case(_IDX18, 22, ("air", "h2", "self", "he"), ("h2", "he"), T4, P4,
                   expect=("y_ge_1", "y_lt_1", "foreign_sets_2", "zero_fraction", "structural_zeros"))
    c["diluent"]["h2"][0, 1] = 0.0
    c["diluent"]["h2"][2, 3] = 0.0
    c["diluent"]["he"][1, 0] = 0.0
    C["m_frac_strides"] = c
    # the reference's fallbacks, at temperatures far from 296 K
    g = LC.grid(1000.0, 1e-3, 2100)
    tbl = mix_table(LC.at(g, _IDX18), 23, foreign=("he",), shifts=False)
    rng = np.random.default_rng(230)
    n = _IDX18.size
    tbl["n_he"][::3] = 0.0                                        # a foreign n of 0 stays 0
    tbl["n_self"][1::4] = 0.0                                     # a self n of 0 falls back to n_air
    tbl["gamma_h2"] = np.round(rng.uniform(0.03, 0.06, n), 4)     # gamma only: n -> n_air
    tbl["delta_co2"] = np.round(rng.uniform(-0.02, 0.01, n), 6)   # shifts only: gamma = 0, no width
    tbl["deltap_co2"] = np.round(rng.uniform(4e-5, 9e-5, n) * rng.choice([-1.0, 1.0], n), 7)
    tbl["deltap_air"] = np.round(rng.uniform(4e-5, 9e-5, n) * rng.choice([-1.0, 1.0], n), 7)
    tbl["deltap_self"] = np.round(rng.uniform(4e-5, 9e-5, n) * rng.choice([-1.0, 1.0], n), 7)
    tbl["delta_self"] = np.round(rng.uniform(-0.008, 0.004, n), 6)
    tbl["delta_air"] = np.round(rng.uniform(-0.008, 0.002, n), 6)
    C["m_fallbacks"] = _case(tbl, (340.0, 200.0, 250.0), (1.0, 0.3, 0.05), fractions(("air", "h2", "self", "co2", "he"), 3, 3, 123),
                             grid=g, expect=("y_ge_1", "n_missing", "foreign_n_zero", "self_n_zero", "shift_only_set", "deltap",
                                             "structural_zeros"))
    # n_dil = 8: repeated keys in other letter case are diluents of their own; gamma_o2 is on the table for the ninth key
    g = LC.grid(1000.0, 1e-3, 2100)
    tbl = mix_table(LC.at(g, _IDX18), 24, foreign=("h2", "he", "co2", "n2", "o2"), shifts=True)
    C["m_eight"] = _case(tbl, T3, P3, fractions(("air", "h2", "AIR", "he", "self", "co2", "SELF", "n2"), 3, 3, 124), grid=g,
                         expect=("y_ge_1", "y_lt_1", "n_dil_8", "repeated_keys", "structural_zeros"))
    # no column at all: n_dil = 0, Gamma0 = 0 and y = 0 exactly; the reference's windows are 50 GammaD
    g = LC.grid(1000.0, 1e-3, 2100)
    C["m_none"] = _case(mix_table(LC.at(g, _IDX18[::1]), 25), (296.0, 220.0), (1.0, 0.05), OrderedDict(xe=1.0), grid=g, hw=50.0,
                        expect=("y_eq_0", "n_dil_0", "structural_zeros"))
    # species 1 has every fraction 0 in layer 1 only (y = 0 there) beside lines with 0 < y < 1 (smally) in the same layer
    g = LC.grid(1000.0, 1e-3, 2100)
    dil = fractions(("h2", "air", "self"), 3, 3, 126)
    for v in dil.values():
        v[1, 1] = 0.0
    C["m_zero_layer"] = _case(mix_table(LC.at(g, _IDX18), 26, foreign=("h2",)), (296.0, 240.0, 260.0), (0.1, 0.01, 0.03), dil, grid=g,
                              hw=30.0, expect=("y_ge_1", "y_lt_1", "y_eq_0", "smally_beside_zero", "zero_fraction", "structural_zeros"))
    # Lorentz: windows from the mixed Gamma0; species 1 (alone on the right of the grid) has Gamma0 = 0 in layer 2: dropped
    g = LC.grid(1000.0, 1e-3, 2100)
    idx = np.array([612, 1640, 655, 690, 1700, 731, 770, 1760, 802, 845, 1810, 880, 921, 1850, 950, 990, 1905, 1020])
    dil = fractions(("he", "air", "self", "h2"), 3, 3, 127)
    for v in dil.values():
        v[1, 2] = 0.0
    C["m_lorentz"] = _case(mix_table(LC.at(g, idx), 27, foreign=("h2", "he")), T3, (1.0, 0.2, 0.03), dil, grid=g, profile=1,
                           expect=("lorentz_drop", "zero_fraction", "structural_zeros"))
    # speed-dependent Voigt: Gamma2 over four diluents, one without an SD column, SD_h2 with zeros; some lines with every
    # SD zero (Gamma2 = 0: PART1); fractions per layer and diluent, equal over the species (one oracle call per layer)
    g = LC.grid(1000.0, 1e-3, 2100)
    idx = _IDX18[:15]
    tbl = mix_table(LC.at(g, idx), 28, foreign=("h2", "he"))
    rng = np.random.default_rng(280)
    for sp, lo_, hi_ in (("air", 0.05, 0.12), ("self", 0.08, 0.15), ("h2", 0.02, 0.07)):
        tbl["SD_" + sp] = np.round(rng.uniform(lo_, hi_, idx.size), 3)
    tbl["SD_h2"][::2] = 0.0
    for sp in ("air", "self", "h2"):
        tbl["SD_" + sp][[4, 11]] = 0.0
    f = fractions(("self", "h2", "air", "he"), 1, 3, 128)
    C["m_sdvoigt"] = _case(tbl, T3, (1.0, 0.1, 0.01), OrderedDict((nm, np.tile(v, (3, 1))) for nm, v in f.items()), grid=g, profile=3,
                           expect=("gamma2_zero", "gamma2_nonzero", "sd_column_absent", "structural_zeros"))
    # m_frac_strides on a non-uniform axis with repeated points, Voigt and Lorentz
    base = C["m_frac_strides"]
    i = np.arange(2047)
    X = 1000.0 + np.concatenate([[0.0], np.cumsum(1e-3 * (1.0 + 0.5 * np.sin(0.7 * i)))])
    X = np.sort(np.concatenate([X, X[[300, 301, 1023, 1023, 1500]]]))
    for name, prof in (("m_axis", 0), ("m_axis_lorentz", 1)):
        C[name] = dict(base, X=X, profile=prof, expect=("y_ge_1", "foreign_sets_2", "zero_fraction", "repeated_points", "structural_zeros"))
        del C[name]["grid"]
    # 7 species x 40 layers: the per-layer tables leave the kernel-argument block (ENV_ARGS = false); fractions a function
    # of (d, s, k), no two equal
    g = LC.grid(1000.0, 1e-3, 1100)
    tbl = mix_table(LC.at(g, np.linspace(470, 640, 14).astype(int)), 29, species=SPECIES7, foreign=("h2", "he"))
    k = np.arange(40)
    d_, s_, k_ = np.meshgrid(np.arange(4), np.arange(7), k, indexing="ij")
    f = 0.05 + 0.4 * ((d_ * 7 + s_) * 40 + k_) / (4 * 7 * 40 - 1.0)
    C["m_device_tables"] = _case(tbl, 200.0 + 100.0 * ((k * 7) % 40) / 39.0, 10.0 ** np.linspace(0.0, -3.0, 40),
                                 OrderedDict((nm, f[d]) for d, nm in enumerate(("he", "air", "h2", "self"))), grid=g, hw=3.0,
                                 expect=("device_tables", "y_ge_1", "y_lt_1", "foreign_sets_2", "structural_zeros"))
    # m_sets_order on two tiles + 577 points, run on the shard [TILE, end): lines of tile 0 whose windows end more than a
    # grid step before the shard (the skip branch), and lines whose windows just reach in in their widest layer
    base = C["m_sets_order"]
    g = LC.grid(1000.0, 1e-3, 2 * TILE + 577)
    idx = np.r_[np.array([40, 150, 260, 380, 470, 560]), np.array([700, 760, 820]), _IDX18 + 500]
    tbl = mix_table(LC.at(g, idx), 21, foreign=("h2", "he", "co2"), shifts=True)
    c = _case(tbl, T3, P3, base["diluent"], grid=g,
              expect=("position_ne_set", "skip_branch", "reaches_in", "y_ge_1", "y_lt_1", "structural_zeros"))
    step = 1e-3
    for r in (6, 7, 8):  # moved so that nu + W ends 2.25 points inside the shard in the widest layer of the line
        W = max(max(c["ow"], c["hw"] * max(P["Gamma0"][P["row"] == r][0], P["GammaD"][P["row"] == r][0]))
                for P in (layer_params(c, kk) for kk in range(3)))
        tbl["nu"][r] = LC.at(g, TILE + 2 - int(np.floor(W / step)))
    c["shard"] = (TILE, g[2] - TILE)
    c["sets"] = base["sets"]
    C["m_shard"] = c
    return C


CASES = _cases()
GRID_CASES = [n for n, c in CASES.items() if "grid" in c and c["profile"] != 3 and n != "m_shard"]
AXIS_CASES = [n for n, c in CASES.items() if "X" in c]


# ---- the deliberate defects: each one a change of the INPUTS that gives what a kernel with that defect would compute -----
def _foreign(case):
    """Foreign broadeners of the case in column-set order: case["sets"] (registered on the table before the call) if given,
    then first appearance in the diluent dict (LineTable.broadener_sets appends on demand)."""
    out = []
    for nm in tuple(case.get("sets", ())) + tuple(case["diluent"]):
        sp = nm.lower()
        if sp not in ("air", "self") and sp not in out and any(f + sp in case["tbl"] for f in FIELDS):
            out.append(sp)
    return out


def _map_blocks(case, fn):
    return OrderedDict((nm, fn(v)) for nm, v in case["diluent"].items())


def _mutate(case, m):
    """(tbl, diluent) of the case under defect m."""
    tbl = {k: np.array(v, copy=True) for k, v in case["tbl"].items()}
    dil = OrderedDict((nm, v.copy()) for nm, v in case["diluent"].items())
    names = list(dil)
    nS, nL = next(iter(dil.values())).shape
    fs = _foreign(case)
    n = tbl["nu"].size
    if m == "frac_species_layer_swapped":   # frac[(d*nS + sp)*nL + k] read as frac[(d*nL + k)*nS + sp]
        dil = _map_blocks(case, lambda v: v.reshape(nL, nS).T.copy())
    elif m == "frac_diluents_rotated":      # diluent d takes the block of d + 1
        dil = OrderedDict((nm, case["diluent"][names[(d + 1) % len(names)]].copy()) for d, nm in enumerate(names))
    elif m == "sets_rotated":               # (c - 2)*n_lines + l off by a set: set j + 1 reads set j's columns
        for j, sp in enumerate(fs):
            src = fs[j - 1]
            for f in FIELDS:
                tbl.pop(f + sp, None)
                if f + src in case["tbl"]:
                    tbl[f + sp] = np.array(case["tbl"][f + src], copy=True)
    elif m == "foreign_n_zero_to_n_air":    # the self fallback applied to a foreign set
        for sp in fs:
            if "n_" + sp in tbl:
                z = tbl["n_" + sp] == 0.0
                tbl["n_" + sp][z] = tbl["n_air"][z]
    elif m == "missing_n_is_zero":          # an absent n column filled with 0, not with n_air
        for sp in fs:
            if "n_" + sp not in tbl:
                tbl["n_" + sp] = np.zeros(n)
    elif m == "self_n_zero_kept":           # a self n of 0 kept (1e-300: (Tref/T)^n = 1 exactly, and the oracle does not replace it)
        if "n_self" in tbl:
            tbl["n_self"][tbl["n_self"] == 0.0] = 1e-300
    elif m == "deltap_dropped":
        for k in [k for k in tbl if k.startswith("deltap_")]:
            del tbl[k]
    elif m == "zero_fraction_not_skipped":  # an exact 0 not honoured: the entry read as the diluent's largest fraction
        dil = _map_blocks(case, lambda v: np.where(v == 0.0, v.max(), v))
    elif m == "gamma2_from_other_set":      # dil_sd(c) of another c: each SD column handed to the next broadener that has one
        have = [sp for sp in ["air", "self"] + fs if "SD_" + sp in case["tbl"]]
        for j, sp in enumerate(have):
            tbl["SD_" + sp] = np.array(case["tbl"]["SD_" + have[j - 1]], copy=True)
    elif m == "gamma2_without_gamma":       # Gamma2 = f SD p, the gamma factor left out
        for sp in ["air", "self"] + fs:
            if "SD_" + sp in tbl and "gamma_" + sp in tbl:
                tbl["SD_" + sp] = tbl["SD_" + sp] / tbl["gamma_" + sp]
    elif m == "layer_fractions_shifted_by_one":  # stale fractions: layer k reads layer k + 1
        dil = _map_blocks(case, lambda v: np.roll(v, -1, axis=1))
    else:
        raise KeyError(m)
    return tbl, dil


MUTATIONS = ["frac_species_layer_swapped", "frac_diluents_rotated", "sets_rotated", "foreign_n_zero_to_n_air", "missing_n_is_zero",
             "self_n_zero_kept", "deltap_dropped", "zero_fraction_not_skipped", "gamma2_from_other_set", "gamma2_without_gamma",
             "layer_fractions_shifted_by_one"]


# ---- the definition ----------------------------------------------------------------------------------------------------
def _sd_layer(case, tbl, dil, X, k, dtype):
    return cpu_ref.sdvoigt_terms(tbl, T=float(case["T"][k]), p=float(case["p"][k]), OmegaGrid=X, OmegaWing=case["ow"],
                                 OmegaWingHW=case["hw"], Diluent={nm: float(v[0, k]) for nm, v in dil.items()}, dtype=dtype)


def definition(case, mutate=None, g=None, layers=None, diluent=None):
    """[layers][points] in float64 on the case's axis (or the shard g of its grid), for the layers `layers` (default all)
    and the diluent dict `diluent` (default the case's)."""
    if diluent is not None:
        nS, nL = len(species_of(case["tbl"])), case["T"].size
        case = dict(case, diluent=OrderedDict((nm, np.broadcast_to(np.asarray(v, dtype=np.float64), (nS, nL)).copy())
                                              for nm, v in diluent.items()))
    tbl, dil = (case["tbl"], case["diluent"]) if mutate is None else _mutate(case, mutate)
    X = case_axis(case, g)
    sp = species_of(tbl)
    out = []
    for k in (range(case["T"].size) if layers is None else layers):
        if case["profile"] == 3:
            if all(np.all(v == v[:1]) for v in dil.values()):  # the case itself: one call per layer serves
                out.append(np.asarray(_sd_layer(case, tbl, dil, X, k, np.float64)["xs"], dtype=np.float64))
            else:  # (a defect that tells the species apart: each species' lines with its own fractions)
                row = np.zeros(X.size)
                for s, mi in enumerate(sp):
                    rows = (np.asarray(tbl["molec_id"]) == mi[0]) & (np.asarray(tbl["local_iso_id"]) == mi[1])
                    sub = {key: np.asarray(v)[rows] for key, v in tbl.items()}
                    row += _sd_layer(case, sub, OrderedDict((nm, v[s:s + 1]) for nm, v in dil.items()), X, k, np.float64)["xs"]
                out.append(row)
            continue
        fn = cpu_ref.absorptionCoefficient_Lorentz if case["profile"] == 1 else cpu_ref.absorptionCoefficient_Voigt
        row = np.zeros(X.size)
        for s, mi in enumerate(sp):
            row += fn(tbl, Components=[mi], T=float(case["T"][k]), p=float(case["p"][k]), OmegaGrid=X, OmegaWing=case["ow"],
                      OmegaWingHW=case["hw"], Diluent=OrderedDict((nm, float(v[s, k])) for nm, v in dil.items()))[1]
        out.append(row)
    return np.stack(out)


def sd_reference(case, g=None):
    """The dict sdvoigt_cases.judge takes (lists over the layers): want (long double), want64, den, own, skip, skip_per_line,
    pairs -- sdvoigt_cases.oracle's assembly, with the case's Diluent."""
    X = case_axis(case, g)
    out = dict(want=[], want64=[], den=[], own=[], skip=[], skip_per_line=[], pairs=[])
    for k in range(case["T"].size):
        lo = _sd_layer(case, case["tbl"], case["diluent"], X, k, np.float64)
        hi = _sd_layer(case, case["tbl"], case["diluent"], X, k, np.longdouble)
        skip = np.zeros(X.size, dtype=bool)
        worst, pairs = 0, 0
        for (r64, a64, b64, c64), (rl, al, bl, cl) in zip(lo["lines"], hi["lines"]):
            assert (r64, a64, b64) == (rl, al, bl)
            d = ((c64 ^ cl) & SC.PREDICATES) != 0
            skip[a64:b64] |= d
            worst = max(worst, int(d.sum()))
            pairs += b64 - a64
        out["want"].append(hi["xs"])
        out["want64"].append(lo["xs"])
        out["den"].append(hi["den"])
        out["own"].append(SC._halo_max(np.abs(lo["xs"].astype(np.longdouble) - hi["xs"])))
        out["skip"].append(skip)
        out["skip_per_line"].append(worst)
        out["pairs"].append(pairs)
    return out


# ---- what a case reaches, from cpu_ref.line_params / linesum_records on its inputs ----------------------------------------
def reach(case):
    """Counter-like dict of labels over every (line, layer) of the case."""
    R = {}

    def add(label, v=1):
        R[label] = R.get(label, 0) + int(v)

    tbl, dil = case["tbl"], case["diluent"]
    sp = species_of(tbl)
    nS, nL = len(sp), case["T"].size
    fs = _foreign(case)
    sets = {"air": 0, "self": 1, **{f: 2 + j for j, f in enumerate(fs)}}
    live = [nm for nm in dil if nm.lower() in sets]
    add("foreign_sets_%d" % len(fs))
    add("n_dil_%d" % len(live))
    add("position_ne_set", len(live) > 0 and all(sets[nm.lower()] != d for d, nm in enumerate(live)))
    add("repeated_keys", len({nm.lower() for nm in dil}) < len(dil))
    add("zero_fraction", sum(int(np.sum(dil[nm] == 0.0)) for nm in live))
    add("device_tables", 2 * nL + 2 * nS * nL + nS > 416)  # RTX_ENV_MAX of rtx_lines.hip
    for f in fs:
        add("n_missing", "gamma_" + f in tbl and "n_" + f not in tbl)
        add("foreign_n_zero", "n_" + f in tbl and np.any(tbl["n_" + f] == 0.0))
        add("shift_only_set", "gamma_" + f not in tbl and ("delta_" + f in tbl or "deltap_" + f in tbl))
        add("sd_column_absent", case["profile"] == 3 and "SD_" + f not in tbl)
    add("self_n_zero", "n_self" in tbl and np.any(tbl["n_self"] == 0.0))
    add("deltap", all("deltap_" + s_ in tbl for s_ in ("air", "self")) and any("deltap_" + f in tbl for f in fs))
    X = case_axis(case)
    add("repeated_points", np.sum(X[1:] == X[:-1]))
    shard = case.get("shard")
    want_zero = []
    for k in range(nL):
        P = layer_params(case, k)
        cte = np.sqrt(np.log(2.0)) / P["GammaD"]
        y = P["Gamma0"] * cte
        W = np.maximum(case["ow"], case["hw"] * (P["Gamma0"] if case["profile"] == 1 else np.maximum(P["Gamma0"], P["GammaD"])))
        lo, hi = np.searchsorted(X, P["nu"] - W, side="right"), np.searchsorted(X, P["nu"] + W, side="right")
        add("y_ge_1", np.sum((y >= 1.0) & (y < 15.0)))
        add("y_lt_1", np.sum((y < 1.0) & (y > 0.0)))
        add("y_eq_0", np.sum(y == 0.0))
        if case["profile"] == 1:
            add("lorentz_drop", np.sum(P["Gamma0"] == 0.0))
        zero_sp = [s for s in range(nS) if np.all(y[P["species"] == s] == 0.0)]
        add("smally_beside_zero", bool(zero_sp) and len(zero_sp) < nS and np.any((y > 0.0) & (y < 1.0)))
        if case["profile"] == 3:
            g2 = np.array([cpu_ref._gamma2(tbl, int(r), float(case["p"][k]), {nm: float(v[0, k]) for nm, v in dil.items()})
                           for r in P["row"]])
            add("gamma2_zero", np.sum(g2 == 0.0))
            add("gamma2_nonzero", np.sum(g2 != 0.0))
        cover = np.zeros(X.size, dtype=bool)
        for a, b in zip(lo, hi):
            cover[a:b] = True
        want_zero.append(int(np.sum(~cover)))
        if shard:
            step = (case["grid"][1] - case["grid"][0]) / (case["grid"][2] - 1)
            x0 = X[shard[0]]
            add("skip_branch", np.sum(P["nu"] + W < x0 - step))
            add("reaches_in", np.sum((P["nu"] < x0) & (hi > shard[0]) & (hi <= shard[0] + 8)))
    add("structural_zeros", min(want_zero) > 0)
    return R
