"""Drop-in for the hot-path part of the reference's vendored HITRAN API (misc/hapi.py).

Only the functions on the north-star path are provided, with the reference's names, argument
meaning and error behaviour:

    absorptionCoefficient_Voigt   misc/hapi.py:10906-11141   -> HIP prologue + line-sum kernels
    LOCAL_TABLE_CACHE             misc/hapi.py:438-463       (same dict layout)
    PYTIPS / partitionSum pieces  misc/hapi.py:9568-9582, 10030
    abundance, molecularMass      misc/hapi.py:5088-5124
    volumeConcentration           misc/hapi.py:10163-10164
    transmittanceSpectrum, absorptionSpectrum, radianceSpectrum   misc/hapi.py:11582-11680   -> rtx_hapi_spectrum
    SLIT_* (host NumPy), convolveSpectrum, convolveSpectrumSame, convolveSpectrumFull
                                  misc/hapi.py:11742-11900   -> rtx_fir_same (fp64 direct FIR)
    absorptionCoefficient_HT      misc/hapi.py:10302-10653   -> rtx_ht_prep + rtx_ht_sum on tables with *_HT_* columns
                                  (opt-in: VARIABLES["HT_COLUMNS"]; otherwise the SDVoigt path)
    pcqsdhc, PROFILE_HT(P), PROFILE_SDRAUTIAN, PROFILE_RAUTIAN, PROFILE_SDVOIGT, PROFILE_VOIGT, PROFILE_LORENTZ,
    PROFILE_DOPPLER, hum1_wei, cpf3   misc/hapi.py:9645-10160   -> rtx_profile_eval / rtx_cpf_eval (fp64, complex)
    profile_lines                 (not in the reference) many lines at once, or their weighted sum -> rtx_profile_sum

The database client (fetch/select/...) and the Galatry profile are out of scope (SURVEY.md
section 2, rows 12-13). There is no CPU fallback: without the HIP library and a GPU,
absorptionCoefficient_Voigt, the spectrum / convolution functions and the profile functions raise.
"""
import math

import numpy as np
import torch

from . import engine
from .tips import PYTIPS, abundance, molecularMass, known_isotopologues  # noqa: F401  (re-exported API)

volumeConcentration = engine.volumeConcentration

DefaultIntensityThreshold = 0.0  # misc/hapi.py:10214
DefaultOmegaWingHW = 50.0        # misc/hapi.py:10218

# name -> {'header': {'number_of_rows': n, ...}, 'data': {column: list-or-array}}
LOCAL_TABLE_CACHE = {}
_DEVICE_TABLES = {}   # tuple(table names) -> (signature, engine.LineTable); least recently used entries are closed
_DEVICE_TABLES_MAX = 8


def storage2cache_from_columns(TableName, columns):
    """Convenience: register a column dict as a table (what db_begin()/fetch() leave in the cache)."""
    n = len(columns["nu"])
    # numeric columns are kept as ndarrays (as hitran_par.storage2cache does): the reference's Python lists would cost a
    # list -> array conversion of every column on every call (~50 ms for 100 000 rows, ten times the device time)
    def keep(v):
        a = np.asarray(v)
        return a.copy() if a.dtype.kind in "fiub" else list(v)
    LOCAL_TABLE_CACHE[TableName] = {"header": {"number_of_rows": n, "table_name": TableName},
                                    "data": {k: keep(v) for k, v in columns.items()}}


_USED_COLS = ("molec_id", "local_iso_id", "nu", "sw", "elower", "gamma_air", "gamma_self", "n_air", "delta_air",
              "n_self", "deltap_air", "delta_self", "deltap_self", "SD_air", "SD_self")
_SIG_WEIGHTS = {}


def _column_signature(v, nrow):
    """Content fingerprint of one column (list or array): length + a dot product with fixed pseudo-random weights, so
    that any in-place edit (a rescaled sw, a tweaked gamma_air, two rows swapped) changes it. ~30 us per 100 000-row
    ndarray column; list columns (the reference's layout) pay the list -> array conversion."""
    a = np.asarray(v)[:nrow]
    if a.dtype.kind not in "fiub":
        a = a.astype(np.float64)
    w = _SIG_WEIGHTS.get(a.size)
    if w is None:
        if len(_SIG_WEIGHTS) > 16:
            _SIG_WEIGHTS.clear()
        w = _SIG_WEIGHTS[a.size] = np.random.default_rng(12345).uniform(0.5, 1.5, a.size)
    if not a.size:
        return (0, 0.0)
    # (np.einsum, not np.dot: the BLAS dot product is multi-threaded -- 64 OpenBLAS threads on a box whose share is 16 CPUs --
    # and every few calls one of the 15 products stalled for 70-80 ms waking them: the sporadic slow drop-in calls of
    # profiles/r3_time_dropin.txt with a table name / column dict, and every other afit_xs.cross_section_grid call)
    if a.dtype != np.float64:
        a = a.astype(np.float64)
    d = float(np.einsum("i,i->", a, w))
    if d != d:
        # a NaN in the column (e.g. a blank field of a .par record): NaN never compares equal, which would rebuild the
        # device table on every call. Fingerprint the finite part and the positions of the NaNs instead.
        bad = np.isnan(a.astype(np.float64, copy=False))
        return (a.size, float(np.einsum("i,i->", np.where(bad, 0.0, a), w)), float(np.einsum("i,i->", bad.astype(np.float64), w)))
    return (a.size, d)


def _broadener_signatures(names, species):
    """{sp: fingerprint of the broadener columns gamma_<sp>, n_<sp>, ... of every table in `names`} (empty tuple: none)."""
    sigs = {}
    for sp in species:
        sig = []
        for n in names:
            d, nrow = LOCAL_TABLE_CACHE[n]["data"], LOCAL_TABLE_CACHE[n]["header"]["number_of_rows"]
            sig.extend((n, f + sp, _column_signature(d[f + sp], nrow)) for f in engine.BROADENER_FIELDS if f + sp in d)
        sigs[sp] = tuple(sig)
    return sigs


def _broadener_columns(names, species):
    """The broadener columns of `species` concatenated over the tables, each table's absent ones by the reference's
    fallbacks (gamma / delta / deltap / SD 0, n = that table's n_air): {<field><sp>: array}."""
    cols = {}
    for sp in species:
        for f in engine.BROADENER_FIELDS:
            if not any(f + sp in LOCAL_TABLE_CACHE[n]["data"] for n in names):
                continue
            parts = []
            for n in names:
                d, nrow = LOCAL_TABLE_CACHE[n]["data"], LOCAL_TABLE_CACHE[n]["header"]["number_of_rows"]
                if f + sp in d:
                    parts.append(np.asarray(d[f + sp], dtype=np.float64)[:nrow])
                elif f == "n_":
                    parts.append(np.asarray(d["n_air"], dtype=np.float64)[:nrow])
                else:
                    parts.append(np.zeros(nrow))
            cols[f + sp] = np.concatenate(parts)
    return cols


def _device_table(names, diluents=()):
    """Device LineTable for one or several cached tables (concatenated). The reference re-reads LOCAL_TABLE_CACHE on
    every call (misc/hapi.py:11044-11125); here the device copy is reused only while a content fingerprint of EVERY
    uploaded column is unchanged, so in-place edits of a cached table are seen (tests/test_gpu_parity.py).
    diluents: broadener names (lower case) other than air / self whose columns the call reads: they are fingerprinted too
    and (re-)uploaded to the table when new or edited (LineTable.broadener_sets)."""
    tbl = _device_table_base(names)
    extra = [sp for sp in dict.fromkeys(diluents) if sp not in ("air", "self")]
    if extra:
        sigs = _broadener_signatures(names, extra)
        stale = tbl.broadeners_stale(sigs)
        if stale:
            tbl.broadener_sets(stale, columns=_broadener_columns(names, stale), sigs=sigs)
    return tbl


def _tref_ht(T):
    """TrefHT of absorptionCoefficient_HT for temperature T (misc/hapi.py:10394-10398): 50 / 150 / 296 / 700 K for T in
    [0, 100) / [100, 200) / [200, 400) / [400, inf); the reference's loop leaves its last value, 700, for any other T."""
    TrefHT = None
    for TRange, TrefHT in zip(((0, 100), (100, 200), (200, 400), (400, float("inf"))), (50., 150., 296., 700.)):
        if T >= TRange[0] and T < TRange[1]:
            break
    return TrefHT


def _ht_columns_read(species, T):
    """The *_HT_* columns absorptionCoefficient_HT reads for the lower-cased Diluent keys `species` at temperature T: the
    six of the TrefHT bucket and nu_HT / kappa_HT / eta_HT of each (misc/hapi.py:10505-10637)."""
    b = (50., 150., 296., 700.).index(_tref_ht(T))
    read = []
    for sp in dict.fromkeys(species):
        names = engine.ht_column_names(sp)
        read += names[6 * b:6 * b + 6] + names[24:]
    return read


def _device_table_ht(tbl, names, species):
    """The Hartmann-Tran columns of `species` (lower case) on the device table, fingerprinted like the broadener columns:
    a changed column is uploaded again. A table that lacks a column another one has contributes zeros (= absent)."""
    species = list(dict.fromkeys(species))
    sigs = {}
    for sp in species:
        sig = []
        for n in names:
            d, nrow = LOCAL_TABLE_CACHE[n]["data"], LOCAL_TABLE_CACHE[n]["header"]["number_of_rows"]
            sig.extend((n, c, _column_signature(d[c], nrow)) for c in engine.ht_column_names(sp) if c in d)
        sigs[sp] = tuple(sig)
    stale = tbl.ht_stale(sigs)
    cols = {}
    for sp in stale:
        for c in engine.ht_column_names(sp):
            if any(c in LOCAL_TABLE_CACHE[n]["data"] for n in names):
                cols[c] = np.concatenate([
                    np.asarray(LOCAL_TABLE_CACHE[n]["data"][c], dtype=np.float64)[:LOCAL_TABLE_CACHE[n]["header"]["number_of_rows"]]
                    if c in LOCAL_TABLE_CACHE[n]["data"] else np.zeros(LOCAL_TABLE_CACHE[n]["header"]["number_of_rows"])
                    for n in names])
    tbl.ht_sets(species, columns=cols, sigs=sigs)
    return tbl


def _device_table_base(names):
    key = tuple(names)
    sig = []
    for n in names:
        d, nrow = LOCAL_TABLE_CACHE[n]["data"], LOCAL_TABLE_CACHE[n]["header"]["number_of_rows"]
        sig.append((nrow,) + tuple((k, _column_signature(d[k], nrow)) for k in _USED_COLS if k in d))
    sig = tuple(sig)
    hit = _DEVICE_TABLES.get(key)
    if hit is not None and hit[0] == sig:
        _DEVICE_TABLES[key] = _DEVICE_TABLES.pop(key)  # mark most recently used
        return hit[1]
    cols = {}
    keys = None
    for n in names:
        d = LOCAL_TABLE_CACHE[n]["data"]
        nrow = LOCAL_TABLE_CACHE[n]["header"]["number_of_rows"]
        keys = set(d.keys()) if keys is None else keys & set(d.keys())
        for k, v in d.items():
            cols.setdefault(k, []).append(np.asarray(v)[:nrow])
    use = [k for k in _USED_COLS if k in keys]
    for req in ("molec_id", "local_iso_id", "nu", "sw", "elower", "gamma_air", "n_air", "delta_air"):
        if req not in use:
            raise Exception("table(s) %s lack the column %s" % (names, req))
    merged = {k: np.concatenate(cols[k]) for k in use}
    if "gamma_self" not in merged:
        merged["gamma_self"] = np.zeros(merged["nu"].size)  # hapi: missing gamma_<species> -> 0 (:11097-11100)
    if hit is not None:
        hit[1].close()
    tbl = engine.LineTable(merged)
    _DEVICE_TABLES.pop(key, None)
    _DEVICE_TABLES[key] = (sig, tbl)
    while len(_DEVICE_TABLES) > _DEVICE_TABLES_MAX:  # bound the device memory held for callers' tables
        old_key = next(iter(_DEVICE_TABLES))
        _DEVICE_TABLES.pop(old_key)[1].close()
        for n in old_key:
            if n.startswith("__dict_"):
                LOCAL_TABLE_CACHE.pop(n, None)
    return tbl


def listOfTuples(a):
    """misc/hapi.py:10221-10228."""
    if type(a) not in set([list, tuple]):
        a = [a]
    return a


def arange_(lower, upper, step):
    """misc/hapi.py:133-139 with the float-`num` crash fixed (npnt cast to int)."""
    npnt = math.floor((upper - lower) / step) + 1
    upper_new = lower + step * (npnt - 1)
    if abs((upper - upper_new) - step) < 1e-10:
        upper_new += step
        npnt += 1
    return np.linspace(lower, upper_new, int(npnt))


def _absorption_coefficient(profile, Components, SourceTables, partitionFunction, Environment, OmegaRange, OmegaStep, OmegaWing,
                            IntensityThreshold, OmegaWingHW, GammaL, HITRAN_units, LineShift, File, Format, OmegaGrid,
                            WavenumberRange, WavenumberStep, WavenumberWing, WavenumberWingHW, WavenumberGrid, Diluent,
                            EnvDependences):
    """Common body of absorptionCoefficient_Voigt / _Lorentz / _Doppler (they share getDefaultValuesForXsect, the
    abundance bookkeeping and the per-line prologue; misc/hapi.py:10906-11141, 11144-11375, 11384-11559)."""
    if WavenumberRange is not None: OmegaRange = WavenumberRange
    if WavenumberStep: OmegaStep = WavenumberStep
    if WavenumberWing: OmegaWing = WavenumberWing
    if WavenumberWingHW: OmegaWingHW = WavenumberWingHW
    if WavenumberGrid is not None: OmegaGrid = WavenumberGrid
    if EnvDependences:
        raise NotImplementedError("EnvDependences hooks are not supported by the HIP line-sum")
    Components = listOfTuples(Components)
    SourceTables = listOfTuples(SourceTables)
    # getDefaultValuesForXsect, misc/hapi.py:10231-10281
    if SourceTables[0] is None:
        SourceTables = ["__BUFFER__"]
    for TableName in SourceTables:
        if TableName not in LOCAL_TABLE_CACHE:
            raise Exception("%s: no such table. Check tableList() for more info." % TableName)
    if Environment is None:
        Environment = {"T": 296.0, "p": 1.0}
    tbl = _device_table(SourceTables)
    if Components == [None]:
        Components = [p for p in tbl.species if p != (0, 0)]
    if OmegaRange is None:
        nu = tbl.cols["nu"]
        OmegaRange = (float(nu.min()), float(nu.max())) if nu.size else (0.0, 0.0)
    if OmegaStep is None:
        OmegaStep = 0.01
    if OmegaWing is None:
        OmegaWing = 0.0
    if not Format:
        Format = "%.12f %e"
    if OmegaStep > (0.005 if profile == 2 else 0.1):  # :11027 / :11452
        print("WARNING: Big wavenumber step: possible accuracy decline")
    if OmegaGrid is not None:
        Omegas = np.sort(np.asarray(OmegaGrid, dtype=np.float64))
    else:
        Omegas = arange_(OmegaRange[0], OmegaRange[1], OmegaStep)
    T = Environment["T"]
    p = Environment["p"]
    # abundances, misc/hapi.py:10996-11009
    ABUNDANCES, NATURAL = {}, {}
    for Component in Components:
        M, I = int(Component[0]), int(Component[1])
        nat = abundance(M, I)
        ABUNDANCES[(M, I)] = Component[2] if len(Component) >= 3 else nat
        NATURAL[(M, I)] = nat
    factor = 1.0 if HITRAN_units else volumeConcentration(p, T)
    GammaL = GammaL.lower()
    if profile == 2:
        Diluent = {"air": 1.0 if LineShift else 0.0}  # Doppler: Shift0 = delta_air*p, or none (misc/hapi.py:11510-11513)
    if not Diluent:
        if GammaL == "gamma_air":
            Diluent = {"air": 1.0}
        elif GammaL == "gamma_self":
            Diluent = {"self": 1.0}
        else:
            raise Exception("Unknown GammaL value: %s" % GammaL)
    # the reference sums over the Diluent keys in their order, each lower-cased (misc/hapi.py:11090-11092; "AIR" and "air"
    # are two terms). Air / self alone, each once, keep the call-wide dil_air / dil_self prologue; anything else takes the
    # per-diluent one (rtx_line_prep_mix), which reads the table's gamma_<sp>, n_<sp>, ... columns of every other key
    keys = [k.lower() for k in Diluent]
    mix = None
    if set(keys) - {"air", "self"} or len(set(keys)) != len(keys):
        mix = {k: float(v) for k, v in Diluent.items()}
        tbl = _device_table(SourceTables, keys)
    if profile == 4:  # Hartmann-Tran columns: every key's Voigt-style and HT columns, always on the explicit axis
        mix = {k: float(v) for k, v in Diluent.items()}
        tbl = _device_table_ht(_device_table(SourceTables, keys), SourceTables, keys)
    dil = {k.lower(): float(v) for k, v in Diluent.items()}
    # a uniform grid (what Grid.from_axis recognises) takes the grid line-sum; any other sorted grid -- non-uniform,
    # repeated points, fewer than 2 points -- the explicit-axis one (rtx_line_prep_axis + rtx_voigt_sum_axis)
    grid = None
    if Omegas.size >= 2 and profile != 4:
        try:
            grid = engine.Grid.from_axis(Omegas)
        except NotImplementedError:
            grid = None
    if grid is None and profile == 3 and Omegas.size:
        raise NotImplementedError("speed-dependent Voigt (non-zero SD_air / SD_self) needs a uniform wavenumber grid: this "
                                  "OmegaGrid / WavenumberGrid is not an np.linspace")
    # per-species weight = factor / natural * abundance (misc/hapi.py:11136-11137); 0 filters the species out (:11066)
    w = np.zeros((len(tbl.species), 1))
    for s, mi in enumerate(tbl.species):
        if mi in ABUNDANCES:
            w[s, 0] = factor / NATURAL[mi] * ABUNDANCES[mi]
    # fold a power of two into the fp32 strengths so HITRAN-unit intensities (~1e-19..1e-30) stay normal
    smax = float(np.max(tbl.cols["sw"])) * float(np.max(w)) if tbl.n and np.max(w) > 0 else 1.0
    scale = 2.0 ** (-math.floor(math.log2(smax))) if smax > 0 and math.isfinite(smax) else 1.0
    if tbl.n == 0 or Omegas.size == 0:
        Xsect = np.zeros(Omegas.size)
    elif profile == 4:
        out = torch.empty((1, Omegas.size), dtype=torch.float64, device=engine.device())
        engine.ht_sum(tbl, Omegas, [T], [p], w, mix, out_f64=out, omega_wing=OmegaWing, omega_wing_hw=OmegaWingHW,
                      intensity_threshold=IntensityThreshold, scale=scale, partitionFunction=partitionFunction)
        Xsect = out[0].cpu().numpy()
    elif grid is not None:
        out = torch.empty((1, grid.n), dtype=torch.float64, device=engine.device())
        engine.voigt_sum(tbl, grid, [T], [p], w, out_f64=out, dil_air=dil.get("air", 0.0), dil_self=dil.get("self", 0.0),
                         omega_wing=OmegaWing, omega_wing_hw=OmegaWingHW, intensity_threshold=IntensityThreshold,
                         scale=scale, partitionFunction=partitionFunction, profile=profile, diluent=mix)
        Xsect = out[0].cpu().numpy()
    else:
        out = torch.empty((1, Omegas.size), dtype=torch.float64, device=engine.device())
        engine.voigt_sum_axis(tbl, Omegas, [T], [p], w, out_f64=out, dil_air=dil.get("air", 0.0), dil_self=dil.get("self", 0.0),
                              omega_wing=OmegaWing, omega_wing_hw=OmegaWingHW, intensity_threshold=IntensityThreshold,
                              scale=scale, partitionFunction=partitionFunction, profile=profile, diluent=mix)
        Xsect = out[0].cpu().numpy()
    if File:
        with open(File, "w") as f:
            for o, x in zip(Omegas, Xsect):
                f.write((Format % (o, x)) + "\n")
    return Omegas, Xsect


def absorptionCoefficient_Voigt(Components=None, SourceTables=None, partitionFunction=PYTIPS, Environment=None,
                                OmegaRange=None, OmegaStep=None, OmegaWing=None,
                                IntensityThreshold=DefaultIntensityThreshold, OmegaWingHW=DefaultOmegaWingHW,
                                GammaL="gamma_air", HITRAN_units=True, LineShift=True, File=None, Format=None,
                                OmegaGrid=None, WavenumberRange=None, WavenumberStep=None, WavenumberWing=None,
                                WavenumberWingHW=None, WavenumberGrid=None, Diluent={}, EnvDependences=None):
    """Absorption coefficient with the Voigt profile; same inputs/outputs as misc/hapi.py:10906-11141.

    Returns (Omegas, Xsect) as float64 NumPy arrays. The sum over lines runs on the GPU
    (rtx_line_prep + rtx_voigt_sum on a uniform grid; rtx_line_prep_axis + rtx_voigt_sum_axis on any other sorted
    OmegaGrid -- non-uniform, repeated points, a single point); line strengths are carried in fp32 with a power-of-two
    scale, so Xsect agrees with the reference to ~1e-6 relative, not bit for bit.
    Diluent: any keys, as the reference (misc/hapi.py:11090-11128): a key other than air / self reads the table's
    gamma_<key>, n_<key>, delta_<key>, deltap_<key> columns (absent ones: 0, n_air). Fractions are not validated.
    Not supported (raises): EnvDependences hooks.
    """
    return _absorption_coefficient(0, Components, SourceTables, partitionFunction, Environment, OmegaRange, OmegaStep, OmegaWing,
                                   IntensityThreshold, OmegaWingHW, GammaL, HITRAN_units, LineShift, File, Format, OmegaGrid,
                                   WavenumberRange, WavenumberStep, WavenumberWing, WavenumberWingHW, WavenumberGrid, Diluent,
                                   EnvDependences)


def absorptionCoefficient_Lorentz(Components=None, SourceTables=None, partitionFunction=PYTIPS, Environment=None,
                                  OmegaRange=None, OmegaStep=None, OmegaWing=None,
                                  IntensityThreshold=DefaultIntensityThreshold, OmegaWingHW=DefaultOmegaWingHW,
                                  GammaL="gamma_air", HITRAN_units=True, LineShift=True, File=None, Format=None,
                                  OmegaGrid=None, WavenumberRange=None, WavenumberStep=None, WavenumberWing=None,
                                  WavenumberWingHW=None, WavenumberGrid=None, Diluent={}, EnvDependences=None):
    """Absorption coefficient with the Lorentz profile; same inputs/outputs as misc/hapi.py:11144-11375
    (PROFILE_LORENTZ :10150, wing max(OmegaWing, OmegaWingHW*Gamma0) :11364). GPU path and limits as for Voigt."""
    return _absorption_coefficient(1, Components, SourceTables, partitionFunction, Environment, OmegaRange, OmegaStep, OmegaWing,
                                   IntensityThreshold, OmegaWingHW, GammaL, HITRAN_units, LineShift, File, Format, OmegaGrid,
                                   WavenumberRange, WavenumberStep, WavenumberWing, WavenumberWingHW, WavenumberGrid, Diluent,
                                   EnvDependences)


def absorptionCoefficient_Doppler(Components=None, SourceTables=None, partitionFunction=PYTIPS, Environment=None,
                                  OmegaRange=None, OmegaStep=None, OmegaWing=None,
                                  IntensityThreshold=DefaultIntensityThreshold, OmegaWingHW=DefaultOmegaWingHW,
                                  ParameterBindings=None, EnvironmentDependencyBindings=None,
                                  GammaL="dummy", HITRAN_units=True, LineShift=True, File=None, Format=None,
                                  OmegaGrid=None, WavenumberRange=None, WavenumberStep=None, WavenumberWing=None,
                                  WavenumberWingHW=None, WavenumberGrid=None):
    """Absorption coefficient with the Doppler (Gauss) profile; same inputs/outputs as misc/hapi.py:11384-11559
    (PROFILE_DOPPLER :10160, its own GammaD constants :11534-11538, wing max(OmegaWing, OmegaWingHW*GammaD) :11540,
    shift delta_air*p only when LineShift). ParameterBindings / EnvironmentDependencyBindings are accepted and ignored,
    as in the reference. Values below exp(-225) of a line's peak (|nu - nu0| > 18 GammaD) come out 0."""
    return _absorption_coefficient(2, Components, SourceTables, partitionFunction, Environment, OmegaRange, OmegaStep, OmegaWing,
                                   IntensityThreshold, OmegaWingHW, "gamma_air", HITRAN_units, LineShift, File, Format, OmegaGrid,
                                   WavenumberRange, WavenumberStep, WavenumberWing, WavenumberWingHW, WavenumberGrid, {}, None)


absorptionCoefficient_Gauss = absorptionCoefficient_Doppler  # misc/hapi.py:11561


def absorptionCoefficient_SDVoigt(Components=None, SourceTables=None, partitionFunction=PYTIPS, Environment=None,
                                  OmegaRange=None, OmegaStep=None, OmegaWing=None,
                                  IntensityThreshold=DefaultIntensityThreshold, OmegaWingHW=DefaultOmegaWingHW,
                                  GammaL="gamma_air", HITRAN_units=True, LineShift=True, File=None, Format=None,
                                  OmegaGrid=None, WavenumberRange=None, WavenumberStep=None, WavenumberWing=None,
                                  WavenumberWingHW=None, WavenumberGrid=None, Diluent={}, EnvDependences=None):
    """Speed-dependent Voigt, signature of misc/hapi.py:10657-10904.

    Tables without speed-dependence columns (the 160-character HITRAN .par format has none) give Gamma2 = 0, for which
    pcqsdhc takes its PART1 branch (:9908-9915), i.e. the Voigt profile: those go through the fp32 Voigt line-sum.
    Tables with non-zero SD_air / SD_self (or SD_<key> of another Diluent key) (:10884-10890) go through rtx_sdvoigt_sum: pcqsdhc PART2-4 in fp64, far wings at
    Chebyshev nodes (the path of the reference's cross-section generator, misc/RT_gen_AbsXS_files.py:90); those need a uniform
    grid (a non-uniform OmegaGrid raises NotImplementedError)."""
    sd = False
    sd_cols = ["SD_air", "SD_self"] + ["SD_" + k.lower() for k in (Diluent or {}) if k.lower() not in ("air", "self")]
    for name in listOfTuples(SourceTables):
        if name is None or name not in LOCAL_TABLE_CACHE:
            continue
        data = LOCAL_TABLE_CACHE[name]["data"]
        for col in sd_cols:
            if col in data and np.any(np.asarray(data[col], dtype=np.float64) != 0.0):
                sd = True
    return _absorption_coefficient(3 if sd else 0, Components, SourceTables, partitionFunction, Environment, OmegaRange, OmegaStep,
                                   OmegaWing, IntensityThreshold, OmegaWingHW, GammaL, HITRAN_units, LineShift, File, Format,
                                   OmegaGrid, WavenumberRange, WavenumberStep, WavenumberWing, WavenumberWingHW, WavenumberGrid,
                                   Diluent, EnvDependences)


_HT_PREFIXES = ("gamma_HT_", "n_HT_", "delta_HT_", "deltap_HT_", "nu_HT_", "kappa_HT_", "eta_HT_")


def absorptionCoefficient_HT(Components=None, SourceTables=None, partitionFunction=PYTIPS, Environment=None,
                             OmegaRange=None, OmegaStep=None, OmegaWing=None,
                             IntensityThreshold=DefaultIntensityThreshold, OmegaWingHW=DefaultOmegaWingHW,
                             GammaL="gamma_air", HITRAN_units=True, LineShift=True, File=None, Format=None,
                             OmegaGrid=None, WavenumberRange=None, WavenumberStep=None, WavenumberWing=None,
                             WavenumberWingHW=None, WavenumberGrid=None, Diluent={}, EnvDependences=None):
    """Hartmann-Tran profile, signature of misc/hapi.py:10302-10653 -- by default for tables WITHOUT Hartmann-Tran columns.

    The reference looks each parameter up under its HT name first (gamma_HT_0_<species>_<Tref>, n_HT_..., delta_HT_...,
    nu_HT_..., eta_HT_..., :10505-10640) and falls back to the Voigt-style columns; a table that has none of the HT
    names gives nuVC = eta = 0, Gamma2 from SD_<species> (:10590-10599), i.e. exactly absorptionCoefficient_SDVoigt
    (checked against the reference in the build container: 6e-16). That case is evaluated here; by default non-zero HT
    columns raise NotImplementedError.

    VARIABLES["HT_COLUMNS"] = True: a call that would read a non-zero *_HT_* column (one of its lower-cased Diluent keys,
    in the TrefHT bucket of its temperature) takes the Hartmann-Tran line-sum -- the reference's lookups and fallbacks per
    line, PROFILE_HT on each window, fp64, on any sorted grid (rtx_ht_prep + rtx_ht_sum). S(T) and
    Q(Tref) are always taken from 296 K, which is what the reference computes for a one-row table; its whole-table call
    agrees with that only for T in [200, 400). Any other call goes to the SDVoigt path as before."""
    if VARIABLES.get("HT_COLUMNS"):
        # the columns this call would read: the *_HT_* ones of its lower-cased Diluent keys in its TrefHT bucket. One of them
        # non-zero: the Hartmann-Tran sum (rtx_ht_prep + rtx_ht_sum); none: the reference's own result is the SDVoigt one
        keys = [k.lower() for k in Diluent] if Diluent else [{"gamma_air": "air", "gamma_self": "self"}.get(GammaL.lower())]
        T = (Environment or {"T": 296.0})["T"]
        read = _ht_columns_read([k for k in keys if k], T)
        ht = False
        for name in listOfTuples(SourceTables if SourceTables is not None else "__BUFFER__"):
            data = LOCAL_TABLE_CACHE.get(name, {}).get("data", {})
            ht = ht or any(c in data and np.any(np.asarray(data[c], dtype=np.float64) != 0.0) for c in read)
        if not ht:
            return absorptionCoefficient_SDVoigt(Components, SourceTables, partitionFunction, Environment, OmegaRange, OmegaStep,
                                                 OmegaWing, IntensityThreshold, OmegaWingHW, GammaL, HITRAN_units, LineShift, File,
                                                 Format, OmegaGrid, WavenumberRange, WavenumberStep, WavenumberWing,
                                                 WavenumberWingHW, WavenumberGrid, Diluent, EnvDependences)
        return _absorption_coefficient(4, Components, SourceTables, partitionFunction, Environment, OmegaRange, OmegaStep, OmegaWing,
                                       IntensityThreshold, OmegaWingHW, GammaL, HITRAN_units, LineShift, File, Format, OmegaGrid,
                                       WavenumberRange, WavenumberStep, WavenumberWing, WavenumberWingHW, WavenumberGrid, Diluent,
                                       EnvDependences)
    for name in listOfTuples(SourceTables):
        if name is None or name not in LOCAL_TABLE_CACHE:
            continue
        for col, vals in LOCAL_TABLE_CACHE[name]["data"].items():
            if col.startswith(_HT_PREFIXES) and np.any(np.asarray(vals, dtype=np.float64) != 0.0):
                raise NotImplementedError("absorptionCoefficient_HT: table %r has the Hartmann-Tran column %s; only the "
                                          "Voigt / speed-dependent Voigt limits are implemented" % (name, col))
    return absorptionCoefficient_SDVoigt(Components, SourceTables, partitionFunction, Environment, OmegaRange, OmegaStep, OmegaWing,
                                         IntensityThreshold, OmegaWingHW, GammaL, HITRAN_units, LineShift, File, Format, OmegaGrid,
                                         WavenumberRange, WavenumberStep, WavenumberWing, WavenumberWingHW, WavenumberGrid, Diluent,
                                         EnvDependences)


absorptionCoefficient = absorptionCoefficient_HT  # the reference's profile selector alias, misc/hapi.py:11377


# ---- loading line files: what the reference's scripts do before the line-sum ---------------------------------------
# (misc/RT_gen_AbsXS_files.py:12: db_begin(folder)). hapi's SQL-like layer (select / sort / group, misc/hapi.py:433-3216)
# is out of scope; rows are filtered with NumPy on LOCAL_TABLE_CACHE[name]['data'] instead.
# HT_COLUMNS (not in the reference): absorptionCoefficient_HT on tables with non-zero Hartmann-Tran columns. False: such a
# table raises NotImplementedError; True: it takes the Hartmann-Tran line-sum
VARIABLES = {"BACKEND_DATABASE_NAME": "data", "HT_COLUMNS": False}


def db_begin(db=None):
    """Load the tables of folder `db` (default 'data') into LOCAL_TABLE_CACHE as misc/hapi.py:5205-5221 /
    loadCache :1718-1730 does: every `<name>.header` names a table whose rows are in `<name>.data` (else `<name>.par`);
    a `.par` file without a header is read with the default 160-character HITRAN layout. Parsing follows the
    reference's storage2cache row by row (radtxfr_amd/hitran_par.py). Returns the list of table names loaded."""
    import os

    from . import hitran_par

    folder = "data" if db is None else db
    os.makedirs(folder, exist_ok=True)
    VARIABLES["BACKEND_DATABASE_NAME"] = folder
    files = sorted(os.listdir(folder))
    names = [f[:-len(".header")] for f in files if f.endswith(".header")]
    names += [f[:-len(".par")] for f in files if f.endswith(".par") and f[:-len(".par")] not in names]
    for name in names:
        path = os.path.join(folder, name + ".data")
        if not os.path.isfile(path):
            path = os.path.join(folder, name + ".par")
            if not os.path.isfile(path):
                raise Exception('Lonely header "%s"' % path)
        hitran_par.storage2cache(name, path)
    return names


def tableList():
    """Names of the cached tables (misc/hapi.py:5168)."""
    return list(LOCAL_TABLE_CACHE.keys())


# ---- spectra from an absorption coefficient, and their convolution with a slit function --------------------------------
# (misc/hapi.py:11582-11680, 11742-11900: steps 2 and 3 of the usual hapi workflow after absorptionCoefficient_*)
cBolts = engine.CBOLTS   # erg/K  (misc/hapi.py:84)
cc = 2.99792458e10       # cm/s   (:85)
hh = 6.626196e-27        # erg s  (:86)


def _spectral_rows(A, n):
    """A spectrum (n,) or a batch (n, nS), spectral axis first; NumPy or torch (float32 / float64) -> (rows, back):
    rows [nS][n] device tensor with contiguous rows, back(out [nS][m]) -> (m,) or (m, nS) of the caller's kind: NumPy
    float64 for NumPy in, a torch tensor on the input's device for torch in."""
    as_torch = isinstance(A, torch.Tensor)
    dev = engine.device()
    if as_torch:
        src_dev = A.device
        t = A if A.dtype in (torch.float32, torch.float64) else A.to(torch.float64)
        t = t.to(dev if not A.is_cuda else A.device)
    else:
        src_dev = None
        t = torch.as_tensor(np.ascontiguousarray(A, dtype=np.float64), device=dev)
    if t.dim() not in (1, 2) or t.shape[0] != n:
        raise ValueError("spectrum of shape %s on a wavenumber grid of %d points (spectral axis first)" % (tuple(t.shape), n))
    one = t.dim() == 1
    rows = t[None].contiguous() if one else t.t().contiguous()

    def back(out):
        out = out[0] if one else out.t().contiguous()
        if as_torch:
            return out.to(src_dev)
        return out.cpu().numpy()

    return rows, back


def _save_to_file(File, Format, Omegas, Xsect):
    """misc/hapi.py:10286-10293."""
    O = Omegas.detach().cpu().numpy() if isinstance(Omegas, torch.Tensor) else np.asarray(Omegas)
    Y = Xsect.detach().cpu().numpy() if isinstance(Xsect, torch.Tensor) else np.asarray(Xsect)
    with open(File, "w") as f:
        for i in range(len(O)):
            f.write((Format + "\n") % (O[i], Y[i]))


def _spectrum(kind, Omegas, AbsorptionCoefficient, Environment, File, Format, Wavenumber):
    if Wavenumber is not None: Omegas = Wavenumber
    l = Environment["l"]
    T = Environment["T"] if kind == 2 else 0.0
    rows, back = _spectral_rows(AbsorptionCoefficient, len(Omegas))
    X = None
    if kind == 2:
        X = (Omegas.to(device=rows.device, dtype=torch.float64) if isinstance(Omegas, torch.Tensor)
             else torch.as_tensor(np.ascontiguousarray(Omegas, dtype=np.float64), device=rows.device)).contiguous()
    Xsect = back(engine.hapi_spectrum(kind, rows, l, T, X))
    if File: _save_to_file(File, Format, Omegas, Xsect)
    return Omegas, Xsect


def transmittanceSpectrum(Omegas, AbsorptionCoefficient, Environment={"l": 100.}, File=None, Format="%e %e", Wavenumber=None):
    """exp(-AbsorptionCoefficient * l), l = Environment['l'] in cm; same inputs / outputs as misc/hapi.py:11582-11611.
    AbsorptionCoefficient: (n,) or (n, nS) (a batch, spectral axis first), NumPy -> NumPy float64, torch -> torch on its device."""
    return _spectrum(0, Omegas, AbsorptionCoefficient, Environment, File, Format, Wavenumber)


def absorptionSpectrum(Omegas, AbsorptionCoefficient, Environment={"l": 100.}, File=None, Format="%e %e", Wavenumber=None):
    """1 - exp(-AbsorptionCoefficient * l); misc/hapi.py:11613-11642. Types as transmittanceSpectrum."""
    return _spectrum(1, Omegas, AbsorptionCoefficient, Environment, File, Format, Wavenumber)


def radianceSpectrum(Omegas, AbsorptionCoefficient, Environment={"l": 100., "T": 296.}, File=None, Format="%e %e", Wavenumber=None):
    """(1 - exp(-AbsorptionCoefficient * l)) * Planck(Omegas, T) in W/sr/cm^2/cm^-1 with hapi's own hh, cc, cBolts and its
    1.0E-7 factor (misc/hapi.py:11644-11680), not radiative_transfer's c1 / c2. Types as transmittanceSpectrum."""
    return _spectrum(2, Omegas, AbsorptionCoefficient, Environment, File, Format, Wavenumber)


# Slit functions (x, g) -> y on the host: the slit has 1e2-1e5 points. Written from the formulas of misc/hapi.py:11742-11823
# with the reference's quirks kept: the Gaussian and dispersion slits take g as the FULL width (they halve it), the cosine
# slit is not clipped outside one period, the diffraction and Michelson slits return 1 -- not the limit -- at exactly x == 0.
def SLIT_RECTANGULAR(x, g):
    """1/g for |x| <= g/2, else 0."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.abs(x) <= g / 2, 1 / g, 0.0)


def SLIT_TRIANGULAR(x, g):
    """(1 - |x|/g)/g for |x| <= g, else 0."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.abs(x) <= g, 1 / g * (1 - np.abs(x) / g), 0.0)


def SLIT_GAUSSIAN(x, g):
    """sqrt(ln2/pi)/h * exp(-ln2 (x/h)^2), h = g/2 the half-width at half-maximum."""
    h = g / 2
    return np.sqrt(np.log(2)) / (np.sqrt(np.pi) * h) * np.exp(-np.log(2) * (np.asarray(x, dtype=np.float64) / h) ** 2)


def SLIT_DISPERSION(x, g):
    """h/pi/(x^2 + h^2), h = g/2 the Lorentzian half-width at half-maximum."""
    h = g / 2
    return h / np.pi / (np.asarray(x, dtype=np.float64) ** 2 + h ** 2)


def SLIT_COSINUS(x, g):
    """(cos(pi x/g) + 1)/(2g), every period of it."""
    return (np.cos(np.pi / g * np.asarray(x, dtype=np.float64)) + 1) / (2 * g)


def SLIT_DIFFRACTION(x, g):
    """sin^2(pi x/g)/(pi x/g)^2/g; 1 at x == 0."""
    x = np.asarray(x, dtype=np.float64)
    y = np.ones(len(x))
    nz = x != 0
    a = np.pi / g * x[nz]
    y[nz] = np.sin(a) ** 2 / a ** 2 / g
    return y


def SLIT_MICHELSON(x, g):
    """2/g sin(2 pi x/g)/(2 pi x/g), the ideal Michelson interferometer with maximum path difference 1/g; 1 at x == 0."""
    x = np.asarray(x, dtype=np.float64)
    y = np.ones(len(x))
    nz = x != 0
    a = 2 * np.pi / g * x[nz]
    y[nz] = 2 / g * np.sin(a) / a
    return y


def _fir(CrossSection, n, taps, scale, first, n_out):
    """scale * (points [first, first + n_out) of the zero-padded convolution of CrossSection (n,) / (n, nS) with taps), on the
    GPU (rtx_fir_same); the only device step of convolveSpectrum*."""
    rows, back = _spectral_rows(CrossSection, n)
    return back(engine.fir_same(rows, taps, scale, first, n_out))


def _convolve(Omega, CrossSection, Resolution, AF_wing, SlitFunction, full):
    """The body the three convolveSpectrum* share: slit on x = [-AF_wing, AF_wing] at the grid's step, then the window of
    the zero-padded convolution that numpy.convolve returns ('same' cut to len(Omega) points, or 'full'), times step."""
    step = Omega[1] - Omega[0]
    step = float(step.item() if isinstance(step, torch.Tensor) else step)
    if full:
        x = np.arange(-AF_wing, AF_wing + step, step)  # plain arange, as the reference (:11891)
    else:
        if step >= Resolution: raise Exception("step must be less than resolution")
        x = arange_(-AF_wing, AF_wing + step, step)
    slit = np.asarray(SlitFunction(x, Resolution), dtype=np.float64)
    if not full:
        slit = slit / (sum(slit) * step)  # simple normalization (:11861; the reference's sum is Python's, left to right)
    n, m = len(Omega), len(slit)
    # numpy.convolve(..., 'same') has max(n, m) points; the reference keeps the first n of them (:11865, :11884)
    first, n_out = (0, n + m - 1) if full else (engine.same_window(n, m)[0], n)
    return _fir(CrossSection, n, slit, step, first, n_out), slit


def convolveSpectrum(Omega, CrossSection, Resolution=0.1, AF_wing=10., SlitFunction=SLIT_RECTANGULAR, Wavenumber=None):
    """Convolution with an instrument (slit) function, cut to the part the slit covers fully; misc/hapi.py:11826-11865.
    Returns (Omega[l:r], Y[l:r], l, r, slit), l = len(slit)//2, r = len(Omega) - len(slit)//2 (the reference computes
    len(slit)/2, a float on Python 3, and raises TypeError at the slice: DESIGN.md section 1). SlitFunction: a SLIT_*
    or any callable (x, g) -> y. CrossSection: (n,) or (n, nS), NumPy -> NumPy float64, torch -> torch on its device.
    The sum runs on the GPU in fp64, directly (rtx_fir_same; no FFT)."""
    if Wavenumber is not None: Omega = Wavenumber
    Y, slit = _convolve(Omega, CrossSection, Resolution, AF_wing, SlitFunction, False)
    left_bnd = len(slit) // 2
    right_bnd = len(Omega) - len(slit) // 2
    return Omega[left_bnd:right_bnd], Y[left_bnd:right_bnd], left_bnd, right_bnd, slit


def convolveSpectrumSame(Omega, CrossSection, Resolution=0.1, AF_wing=10., SlitFunction=SLIT_RECTANGULAR, Wavenumber=None):
    """convolveSpectrum on the whole of Omega (zero-padded ends); misc/hapi.py:11868-11884. Returns
    (Omega, Y, 0, len(Omega), slit). With a slit longer than the spectrum Y is what the reference returns: the first
    len(Omega) points of numpy's max(n, m)-point 'same' result."""
    if Wavenumber is not None: Omega = Wavenumber
    Y, slit = _convolve(Omega, CrossSection, Resolution, AF_wing, SlitFunction, False)
    return Omega[0:len(Omega)], Y, 0, len(Omega), slit


def convolveSpectrumFull(Omega, CrossSection, Resolution=0.1, AF_wing=10., SlitFunction=SLIT_RECTANGULAR):
    """The full convolution (len(Omega) + len(slit) - 1 points) with the un-normalised slit; misc/hapi.py:11886-11900
    without its debug prints. Returns (Omega, Y, None, None)."""
    Y, _ = _convolve(Omega, CrossSection, Resolution, AF_wing, SlitFunction, True)
    return Omega, Y, None, None


# ---- the line-shape functions themselves, with explicit per-line parameters ---------------------------------------------
# (misc/hapi.py:9645-10160: what people who fit spectra call directly, and the only place where hapi returns the imaginary,
# dispersion, part that first-order line mixing needs.) Evaluated on the GPU in fp64 by the complete pcqsdhc of
# csrc/rtx_pcqsdhc.h: every PART, Aterm and Bterm, the common part, complex eta. Each point is what the reference returns
# when that point is passed ALONE (its vector call assigns PART1's Bterm whole-array and raises when the points of a call
# split between PART3 and PART4). Types as for the spectrum functions: NumPy, list, tuple or scalar sg
# -> NumPy float64; a torch tensor sg -> torch tensors on its device. The parameters are scalars and are not validated.
cZero = 0.0  # misc/hapi.py:81


def _points(sg):
    """sg (scalar, list, tuple, NumPy, torch; at most one dimension) -> (fp64 device vector, back): a scalar gives one
    point, shape (1,), as misc/hapi.py:9893-9894 does; back(t) returns a device result in the caller's kind."""
    if isinstance(sg, torch.Tensor):
        if sg.dim() > 1:
            raise ValueError("sg of shape %s: the profile functions take a vector of wavenumbers" % (tuple(sg.shape),))
        src = sg.device
        t = sg.detach().to(device=sg.device if sg.is_cuda else engine.device(), dtype=torch.float64).reshape(-1).contiguous()
        return t, lambda o: o.to(src)
    a = np.asarray(sg, dtype=np.float64)
    if a.ndim > 1:
        raise ValueError("sg of shape %s: the profile functions take a vector of wavenumbers" % (a.shape,))
    return torch.as_tensor(np.ascontiguousarray(a.reshape(-1)), device=engine.device()), lambda o: o.cpu().numpy()


def _host(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def _line_params(sg0, GamD, Gam0, Gam2, Shift0, Shift2, anuVC, eta):
    """The per-line arguments (scalars, or arrays of one length; scalars broadcast) -> [nL][10] fp64 in rtx_profile_eval's
    layout: sg0, GamD, Gam0, Gam2, Shift0, Shift2, anuVC, Re eta, Im eta, pad."""
    eta = _host(eta).astype(np.complex128)
    cols = [np.asarray(_host(v), dtype=np.float64) for v in (sg0, GamD, Gam0, Gam2, Shift0, Shift2, anuVC)] + [eta.real, eta.imag]
    if any(c.ndim > 1 for c in cols):
        raise ValueError("per-line parameters are scalars or vectors of one length")
    cols = np.broadcast_arrays(*[np.atleast_1d(c) for c in cols])  # ValueError for lengths that do not match
    P = np.zeros((cols[0].size, engine.PROFILE_NPAR))
    for j, c in enumerate(cols):
        P[:, j] = c
    return P


def _profile(kind, sg, *line):
    t, back = _points(sg)
    P = torch.as_tensor(_line_params(*line), device=t.device)
    re, im = engine.profile_eval(kind, P, t, imag=kind == engine.LS_PCQSDHC)
    return (back(re[0]), back(im[0])) if im is not None else back(re[0])


def pcqsdhc(sg0, GamD, Gam0, Gam2, Shift0, Shift2, anuVC, eta, sg):
    """The partially-correlated quadratic-speed-dependent hard-collision (Hartmann-Tran) profile, misc/hapi.py:9850-10023:
    (real, imag) of the normalised complex line shape at the wavenumbers sg. eta may be complex (absorptionCoefficient_HT
    passes a complex Eta, :10641). A scalar sg gives shape (1,)."""
    return _profile(engine.LS_PCQSDHC, sg, sg0, GamD, Gam0, Gam2, Shift0, Shift2, anuVC, eta)


def PROFILE_HT(sg0, GamD, Gam0, Gam2, Shift0, Shift2, anuVC, eta, sg):
    """Hartmann-Tran profile, misc/hapi.py:10034-10085: pcqsdhc."""
    return pcqsdhc(sg0, GamD, Gam0, Gam2, Shift0, Shift2, anuVC, eta, sg)


PROFILE_HTP = PROFILE_HT  # misc/hapi.py:10087


def PROFILE_SDRAUTIAN(sg0, GamD, Gam0, Gam2, Shift0, Shift2, anuVC, sg):
    """Speed-dependent Rautian profile, misc/hapi.py:10089-10102: pcqsdhc with eta = 0."""
    return pcqsdhc(sg0, GamD, Gam0, Gam2, Shift0, Shift2, anuVC, cZero, sg)


def PROFILE_RAUTIAN(sg0, GamD, Gam0, Shift0, anuVC, eta, sg):
    """Rautian profile, misc/hapi.py:10104-10115: pcqsdhc with Gam2 = Shift2 = 0 -- and eta = 0: the reference ignores its
    eta argument (:10115), and so does this."""
    return pcqsdhc(sg0, GamD, Gam0, cZero, Shift0, cZero, anuVC, cZero, sg)


def PROFILE_SDVOIGT(sg0, GamD, Gam0, Gam2, Shift0, Shift2, sg):
    """Speed-dependent Voigt profile, misc/hapi.py:10117-10129: pcqsdhc with anuVC = eta = 0."""
    return pcqsdhc(sg0, GamD, Gam0, Gam2, Shift0, Shift2, cZero, cZero, sg)


def PROFILE_VOIGT(sg0, GamD, Gam0, sg):
    """Voigt profile, misc/hapi.py:10131-10140: pcqsdhc with everything but sg0, GamD and Gam0 zero."""
    return PROFILE_HTP(sg0, GamD, Gam0, cZero, cZero, cZero, cZero, cZero, sg)


def PROFILE_LORENTZ(sg0, Gam0, sg):
    """Gam0 / (pi (Gam0^2 + (sg - sg0)^2)), misc/hapi.py:10142-10150. One array."""
    return _profile(engine.LS_LORENTZ, sg, sg0, 1.0, Gam0, 0.0, 0.0, 0.0, 0.0, 0.0)


def PROFILE_DOPPLER(sg0, GamD, sg):
    """cSqrtLn2divSqrtPi exp(-cLn2 ((sg - sg0) / GamD)^2) / GamD with hapi's rounded constants, misc/hapi.py:10152-10160.
    One array."""
    return _profile(engine.LS_DOPPLER, sg, sg0, GamD, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def _cpf(kind, x, y):
    as_torch = isinstance(x, torch.Tensor)
    if as_torch:
        src = x.device
        dev = x.device if x.is_cuda else engine.device()
        tx, ty = torch.broadcast_tensors(x.detach().to(device=dev, dtype=torch.float64), torch.as_tensor(y, dtype=torch.float64).to(dev))
    else:
        ax, ay = np.broadcast_arrays(np.atleast_1d(np.asarray(x, dtype=np.float64)), np.atleast_1d(np.asarray(_host(y), dtype=np.float64)))
        dev = engine.device()
        tx, ty = torch.as_tensor(np.ascontiguousarray(ax), device=dev), torch.as_tensor(np.ascontiguousarray(ay), device=dev)
    shape = tuple(tx.shape)
    re, im = engine.cpf_eval(kind, tx.reshape(-1).contiguous(), ty.reshape(-1).contiguous())
    re, im = re.reshape(shape), im.reshape(shape)
    return (re.to(src), im.to(src)) if as_torch else (re.cpu().numpy(), im.cpu().numpy())


def hum1_wei(x, y, n=24):
    """w(x + iy) as VARIABLES['CPF'] of the reference computes it, misc/hapi.py:9833-9844: Weideman's 24-term rational
    expansion where |x| + y < 15, the one-term asymptote elsewhere; y may be negative. (real, imag). Only n = 24 exists on
    the GPU (its coefficients are compile-time constants)."""
    if n != 24:
        raise ValueError("hum1_wei: n=%r; only the 24-term expansion is implemented" % (n,))
    return _cpf(engine.CPF_HUM1_WEI, x, y)


def cpf3(X, Y):
    """The 15-term asymptotic series of w(X + iY) that pcqsdhc uses around |z| = 8, misc/hapi.py:9645-9670. (real, imag)."""
    return _cpf(engine.CPF_CPF3, X, Y)


def profile_lines(sg, sg0, GamD=None, Gam0=0., Gam2=0., Shift0=0., Shift2=0., anuVC=0., eta=0., profile="HT", weights=None,
                  mixing=None):
    """Many lines in one call (not in the reference, which takes one line per call). The per-line arguments are arrays of one
    length nL; scalars broadcast. profile: "HT" (pcqsdhc, eta may be complex), "LORENTZ" (reads sg0, Gam0) or "DOPPLER"
    (reads sg0, GamD). No windows: every line reaches every point of sg.
      weights=None   (real, imag), each [nL][n]: line l at point i, bit-identical to the one-line functions above
                     (imag is zero for LORENTZ and DOPPLER).
      weights [nL]   the spectrum  sum_l weights_l (Re LS_l + mixing_l Im LS_l)  of shape [n] (profile "HT" only): strengths
                     on the absorption part and first-order line-mixing coefficients on the dispersion part; mixing=None
                     means zeros. Summed on the GPU in line order (rtx_profile_sum): bit-reproducible."""
    kinds = {"HT": engine.LS_PCQSDHC, "LORENTZ": engine.LS_LORENTZ, "DOPPLER": engine.LS_DOPPLER}
    if profile not in kinds:
        raise ValueError("profile=%r; one of 'HT', 'LORENTZ', 'DOPPLER'" % (profile,))
    if GamD is None:
        if profile != "LORENTZ":
            raise ValueError("profile %r needs GamD" % profile)
        GamD = 1.0  # not read
    P = _line_params(sg0, GamD, Gam0, Gam2, Shift0, Shift2, anuVC, eta)
    nL = P.shape[0]
    w = m = None
    if weights is not None:
        if profile != "HT":
            raise ValueError("weights: the weighted sum is implemented for profile 'HT' (it contains the Voigt family as limits)")
        w = np.array(np.broadcast_to(np.asarray(_host(weights), dtype=np.float64), (nL,)))  # a writable copy
        if mixing is not None:
            m = np.ascontiguousarray(w * np.broadcast_to(np.asarray(_host(mixing), dtype=np.float64), (nL,)))
    elif mixing is not None:
        raise ValueError("mixing without weights")
    t, back = _points(sg)
    Pd = torch.as_tensor(P, device=t.device)
    if w is None:
        re, im = engine.profile_eval(kinds[profile], Pd, t)
        return back(re), back(im)
    return back(engine.profile_sum(Pd, torch.as_tensor(w, device=t.device), None if m is None else torch.as_tensor(m, device=t.device), t))
