"""Host-side engine: PyTorch-ROCm owns device memory and streams, libradtxfr_hip.so does the work.

This is plumbing between the reference-shaped shims (radiative_transfer.py, hapi.py, ILS_MAKO.py in
this package) and the C ABI (include/radtxfr_hip.h). Every compute call goes through the HIP
library; nothing here falls back to NumPy or to the oracle.
"""
import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib, tips

TUD_MAX_MU = 8  # slant paths per rtx_tud launch (include/radtxfr_hip.h)
TUD_OD_NONNEG = 1  # RTX_TUD_OD_NONNEG
CTUD_OD_SCRATCH = 1  # RTX_CTUD_OD_SCRATCH

# hapi constants used for per-species / per-layer host factors (misc/hapi.py:84-92, 10163-10164)
CBOLTS = 1.380648813e-16
TREF = 296.0


def volumeConcentration(p, T):
    """Molecules/cm^3 at p [atm], T [K] (misc/hapi.py:10163-10164)."""
    return (p / 9.869233e-7) / (CBOLTS * T)


class trace_range:
    """roctx range around a stage (tracing hook), visible in `rocprofv3 --marker-trace`: enabled with
    RADTXFR_ROCTX=1, otherwise a no-op that costs one attribute test. torch.cuda.nvtx maps to roctx on ROCm."""
    enabled = bool(int(__import__("os").environ.get("RADTXFR_ROCTX", "0") or 0))

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if trace_range.enabled:
            torch.cuda.nvtx.range_push(self.name)

    def __exit__(self, *exc):
        if trace_range.enabled:
            torch.cuda.nvtx.range_pop()
        return False


def require_gpu():
    if not torch.cuda.is_available():
        raise _lib.RtxError("no HIP device visible: radtxfr_amd has no CPU fallback (torch.cuda.is_available() is False)")


def device(dev=None):
    require_gpu()
    if dev is None:
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device(dev)


def _stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _h(a):
    """contiguous float64 host array + its pointer (kept alive by the caller holding the array)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(C.c_void_p)


class Grid:
    """np.linspace(xmin, xmax, n_total) (radiative_transfer.py:269-270), optionally one shard of it."""

    def __init__(self, xmin, xmax, n_total, offset=0, n=None):
        self.c = _lib.make_grid(xmin, xmax, n_total, offset, n)

    xmin = property(lambda s: s.c.xmin)
    xmax = property(lambda s: s.c.xmax)
    step = property(lambda s: s.c.step)
    n_total = property(lambda s: s.c.n_total)
    offset = property(lambda s: s.c.offset)
    n = property(lambda s: s.c.n)

    def shard(self, offset, n):
        return Grid(self.xmin, self.xmax, self.n_total, offset, n)

    def axis(self):
        """Materialise this shard's wavenumbers (host fp64), bit-identical to np.linspace."""
        ig = np.arange(self.offset, self.offset + self.n, dtype=np.float64)
        X = ig * self.step + self.xmin  # arange*step + start: the two roundings np.linspace makes
        if self.n and self.offset + self.n == self.n_total:
            X[-1] = self.xmax
        return X

    def x_at(self, i):
        """Wavenumber of local index i (same bits as axis()[i])."""
        ig = self.offset + int(i)
        return self.xmax if ig == self.n_total - 1 else float(np.float64(ig) * self.step + self.xmin)

    @staticmethod
    def from_axis(X, rtol=1e-9):
        """Recognise a uniform ascending axis; raises if X is not np.linspace-like."""
        X = np.asarray(X, dtype=np.float64).ravel()
        if X.size < 2:
            raise ValueError("spectral axis needs at least 2 points")
        g = Grid(X[0], X[-1], X.size)
        dev = np.max(np.abs(X - np.linspace(X[0], X[-1], X.size)))
        if not (g.step > 0) or dev > rtol * abs(g.step):
            raise NotImplementedError("the HIP line-sum needs a uniform ascending wavenumber grid "
                                      f"(max deviation from np.linspace = {dev:g}, step = {g.step:g})")
        return g

    def byref(self):
        return C.byref(self.c)


_COLS = ("nu", "sw", "elower", "gamma_air", "gamma_self", "n_air", "delta_air")
_OPT_COLS = ("n_self", "deltap_air", "delta_self")
# the columns of one broadener <sp> (misc/hapi.py:11090-11128, SD :10860-10890): <field><sp>, sp in lower case
BROADENER_FIELDS = ("gamma_", "n_", "delta_", "deltap_", "SD_")
MAX_DILUENTS = 8  # per prologue (include/radtxfr_hip.h: RTX_MAX_DILUENTS)


def _is_broadener_column(k):
    return isinstance(k, str) and any(k.startswith(f) and k[len(f):] not in ("", "air", "self") for f in BROADENER_FIELDS)


# Hartmann-Tran columns (misc/hapi.py:10505-10637): per broadener <sp> and TrefHT, then the three without a temperature
HT_TREFS = (50, 150, 296, 700)
HT_FIELDS = ("gamma_HT_0_", "n_HT_", "gamma_HT_2_", "delta_HT_0_", "deltap_HT_", "delta_HT_2_")
HT_PREFIXES = ("gamma_HT_", "n_HT_", "delta_HT_", "deltap_HT_", "nu_HT_", "kappa_HT_", "eta_HT_")


def ht_column_names(sp):
    """The 27 Hartmann-Tran column names of broadener `sp` (lower-cased, as the reference builds them) in the slot order
    of rtx_lines_set_ht (include/radtxfr_hip.h)."""
    sp = str(sp).lower()
    names = ["%s%s_%d" % (f, sp, t) for t in HT_TREFS for f in HT_FIELDS]
    return names + ["nu_HT_" + sp, "kappa_HT_" + sp, "eta_HT_" + sp]


class LineTable:
    """Device-resident HITRAN-format line table, sorted by nu (include/radtxfr_hip.h: rtx_lines).
    `columns` is the column dict of the reference's table type: LOCAL_TABLE_CACHE[name]['data']
    (misc/hapi.py:438-463)."""

    def __init__(self, columns):
        require_gpu()
        lib = _lib.load()
        self.device = torch.cuda.current_device()  # the table lives on the device that is current at creation
        nu = np.asarray(columns["nu"], dtype=np.float64)
        order = np.argsort(nu, kind="stable")
        self.n = int(nu.size)
        self.cols = {k: np.ascontiguousarray(np.asarray(columns[k], dtype=np.float64)[order]) for k in _COLS}
        for k in _OPT_COLS:
            if k in columns:
                self.cols[k] = np.ascontiguousarray(np.asarray(columns[k], dtype=np.float64)[order])
        M = np.asarray(columns["molec_id"]).astype(np.int64)[order]
        I = np.asarray(columns["local_iso_id"]).astype(np.int64)[order]
        self.molec_id, self.local_iso_id = M, I
        # distinct (molec_id, local_iso_id) pairs in sorted order and each row's index into them, vectorised: 100 000 Python
        # tuples per table were enough to tip the interpreter into a full garbage collection (40 ms with torch loaded)
        code = M * 1000003 + I  # ascending code = ascending (molec_id, local_iso_id) for the non-negative ids HITRAN uses
        uniq, inv = np.unique(code, return_inverse=True)
        pairs = [(int(u // 1000003), int(u % 1000003)) for u in uniq]
        self.species = pairs if pairs else [(0, 0)]
        sp = np.ascontiguousarray(inv, dtype=np.int32)
        self._h = C.c_void_p(0)
        ptr = lambda k: self.cols[k].ctypes.data_as(C.c_void_p) if k in self.cols else C.c_void_p(0)
        _lib.check(lib.rtx_lines_create(
            self.n, len(self.species), ptr("nu"), ptr("sw"), ptr("elower"), ptr("gamma_air"), ptr("gamma_self"),
            ptr("n_air"), ptr("n_self"), ptr("delta_air"), ptr("deltap_air"), ptr("delta_self"),
            sp.ctypes.data_as(C.c_void_p), C.byref(self._h)))
        # optional speed-dependence columns (absorptionCoefficient_SDVoigt, misc/hapi.py:10884-10887)
        self.has_sd = False
        sd = {}
        for k in ("SD_air", "SD_self"):
            if k in columns:
                sd[k] = np.ascontiguousarray(np.asarray(columns[k], dtype=np.float64)[order])
                self.has_sd = self.has_sd or bool(np.any(sd[k] != 0.0))
        self._sd = sd
        if self.has_sd:
            sp_ = lambda k: sd[k].ctypes.data_as(C.c_void_p) if k in sd else C.c_void_p(0)
            _lib.check(lib.rtx_lines_set_sd(self._h, sp_("SD_air"), sp_("SD_self")))
        if "deltap_self" in columns:  # misc/hapi.py:11120-11124
            dps = np.ascontiguousarray(np.asarray(columns["deltap_self"], dtype=np.float64)[order])
            if np.any(dps != 0.0):
                self.cols["deltap_self"] = dps
                _lib.check(lib.rtx_lines_set_deltap_self(self._h, dps.ctypes.data_as(C.c_void_p)))
        self._plans = {}
        # extra broadener column sets (rtx_lines_set_broadeners), uploaded on demand by broadener_sets(): the source columns
        # (caller's row order), the uploaded sets {sp: {field: sorted column}} in set order and their fingerprints
        self._order = order
        self._xsrc = {k: v for k, v in columns.items() if _is_broadener_column(k)}
        self._xcols, self._xsig = {}, {}
        # Hartmann-Tran columns (rtx_lines_set_ht), uploaded on demand by ht_sets(): the source columns (caller's row order)
        # and the uploaded ones {sp: {slot: sorted column}} with their fingerprints
        self._htsrc = {k: v for k, v in columns.items() if isinstance(k, str) and k.startswith(HT_PREFIXES)}
        self._htcols, self._htsig = {}, {}

    def ht_stale(self, sigs):
        """The broadeners of {sp: fingerprint of its HT columns} (empty: it has none) that this table holds differently."""
        return [sp for sp, sig in sigs.items() if (sp in self._htcols) != bool(sig) or (sig and self._htsig.get(sp) != sig)]

    def ht_sets(self, names, columns=None, sigs=None):
        """broadener_sets(names) for the Hartmann-Tran sum (rtx_ht_prep), with the HT columns of every name on the device
        (rtx_lines_set_ht). A broadener that has HT columns but no Voigt-style one gets a column set of its own (gamma = 0,
        n = n_air), so that its HT columns have a set to belong to. `columns` / `sigs`: as for broadener_sets, for the HT
        columns."""
        src = self._htsrc if columns is None else columns
        names = [str(n).lower() for n in names]
        changed = False
        for sp in dict.fromkeys(names):
            sig = None if sigs is None else sigs.get(sp)
            if sp in self._htcols and (sigs is None or self._htsig.get(sp) == sig):
                continue
            cols = {j: np.ascontiguousarray(np.asarray(src[c], dtype=np.float64)[:self._order.size][self._order])
                    for j, c in enumerate(ht_column_names(sp)) if c in src}
            if cols:
                self._htcols[sp], self._htsig[sp] = cols, sig
                changed = True
            elif sp in self._htcols:
                del self._htcols[sp]
                self._htsig.pop(sp, None)
                changed = True
        before = list(self._xcols)
        sets = self.broadener_sets(names)
        if changed and list(self._xcols) == before:  # (a new extra set has uploaded them already: _upload_broadeners)
            self._upload_ht()
        return sets

    def _upload_ht(self):
        order = list(self._xcols)
        sps = [sp for sp in self._htcols if sp in ("air", "self") or sp in order]
        set_h = np.ascontiguousarray([0 if sp == "air" else 1 if sp == "self" else 2 + order.index(sp) for sp in sps], dtype=np.int32)
        ptrs = (C.c_void_p * max(27 * len(sps), 1))()
        for s_, sp in enumerate(sps):
            for j, col in self._htcols[sp].items():
                ptrs[27 * s_ + j] = col.ctypes.data
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().rtx_lines_set_ht(self._h, len(sps), set_h.ctypes.data_as(C.c_void_p), ptrs))

    def broadeners_stale(self, sigs):
        """The broadeners of {sp: fingerprint} whose columns this table does not hold, or holds with another fingerprint."""
        return [sp for sp, sig in sigs.items() if sp not in self._xcols or self._xsig.get(sp) != sig]

    def broadener_sets(self, names, columns=None, sigs=None):
        """Column set of each diluent name for rtx_line_prep_mix: 0 air, 1 self, 2 + j the j-th uploaded extra set, None for
        a broadener without any column (gamma = delta = 0: it contributes nothing). Names are matched in lower case, as the
        reference builds gamma_<sp> (misc/hapi.py:11092). The columns of a broadener not yet on the device -- or whose
        fingerprint in `sigs` differs from the uploaded one -- are taken from `columns` (caller's row order; default: the
        columns given at creation) and the whole extra set is uploaded again; the sets stay on the device between calls."""
        src = self._xsrc if columns is None else columns
        names = [str(n).lower() for n in names]
        changed = False
        for sp in dict.fromkeys(names):
            if sp in ("air", "self"):
                continue
            sig = None if sigs is None else sigs.get(sp)
            if sp in self._xcols and (sigs is None or self._xsig.get(sp) == sig):
                continue
            cols = {f: src[f + sp] for f in BROADENER_FIELDS if f + sp in src}
            if cols or sp in self._htcols:  # (HT columns alone: a set of fallbacks to hold them)
                self._xcols[sp] = {f: np.ascontiguousarray(np.asarray(v, dtype=np.float64)[:self._order.size][self._order])
                                   for f, v in cols.items()}
                self._xsig[sp] = sig
                changed = True
            elif sp in self._xcols:
                del self._xcols[sp]
                self._xsig.pop(sp, None)
                changed = True
        if changed:
            self._upload_broadeners()
        order = list(self._xcols)
        return [0 if sp == "air" else 1 if sp == "self" else (2 + order.index(sp) if sp in self._xcols else None) for sp in names]

    def extra_has_sd(self, names):
        """True where a speed-dependence column SD_<sp> of an uploaded extra broadener among `names` is non-zero."""
        return any(np.any(self._xcols[sp]["SD_"] != 0.0) for sp in (str(n).lower() for n in names)
                   if sp in self._xcols and "SD_" in self._xcols[sp])

    def _upload_broadeners(self):
        n_x = len(self._xcols)
        if n_x > 64:
            raise ValueError("more than 64 extra broadeners on one line table")
        arr = []
        for f in BROADENER_FIELDS:
            a = (C.c_void_p * max(n_x, 1))()
            for j, cols in enumerate(self._xcols.values()):
                a[j] = cols[f].ctypes.data if f in cols else None
            arr.append(a)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().rtx_lines_set_broadeners(self._h, n_x, *arr))
        if self._htcols:  # the HT sets go by column-set index: attach them again
            self._upload_ht()

    def host_columns(self):
        """The uploaded columns as a host column dict (sorted by nu): what another device's copy is built from."""
        cols = dict(self.cols)
        cols.update(self._sd)
        for sp, c in self._xcols.items():
            cols.update({f + sp: v for f, v in c.items()})
        for sp, c in self._htcols.items():
            names = ht_column_names(sp)
            cols.update({names[j]: v for j, v in c.items()})
        cols["molec_id"], cols["local_iso_id"] = self.molec_id, self.local_iso_id
        return cols

    def on_device(self, dev):
        """This table on device index `dev`: itself, or a cached copy uploaded there (closed with this table)."""
        dev = int(dev)
        if dev == self.device:
            return self
        peers = self.__dict__.setdefault("_peers", {})
        if dev not in peers:
            with torch.cuda.device(dev):
                peers[dev] = LineTable(self.host_columns())
        peer = peers[dev]
        if list(peer._xcols) != list(self._xcols) or peer._xsig != self._xsig:  # extra broadeners uploaded here since
            peer._xcols, peer._xsig = dict(self._xcols), dict(self._xsig)
            peer._upload_broadeners()
        return peer

    def plan(self, n_layers, n_points):
        """A prep object big enough for (n_layers, n_points); cached, grown on demand."""
        best = None
        for (L, Np), p in self._plans.items():
            if L >= n_layers and Np >= n_points:
                best = p
        if best is None:
            best = VoigtPlan(self, n_layers, n_points)
            self._plans = {k: v for k, v in self._plans.items() if not (k[0] <= n_layers and k[1] <= n_points)}
            self._plans[(n_layers, n_points)] = best
        return best

    def close(self):
        for t in self.__dict__.pop("_peers", {}).values():
            t.close()
        for p in self._plans.values():
            p.close()
        self._plans = {}
        hp = self.__dict__.pop("_ht_plan", None)
        if hp is not None:
            hp.close()
        if self._h:
            with torch.cuda.device(self.device):
                _lib.load().rtx_lines_free(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VoigtPlan:
    """Per-(line, layer) record storage (rtx_prep)."""

    def __init__(self, lines, max_layers, max_points):
        self.lines = lines
        self._h = C.c_void_p(0)
        _lib.check(_lib.load().rtx_prep_create(lines._h, int(max_layers), int(max_points), C.byref(self._h)))

    def close(self):
        if self._h:
            _lib.load().rtx_prep_free(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _live_species(species, weight):
    """Indices of the species a prologue looks partition sums up for: those with an isotopologue and, given weight[nS][nL],
    a non-zero weight in some layer -- the reference skips the others before any look-up (`continue`, misc/hapi.py:11066)."""
    if weight is None:
        return [s for s, mi in enumerate(species) if mi != (0, 0)]
    live = np.asarray(weight).reshape(len(species), -1).any(axis=1)
    return [s for s, mi in enumerate(species) if mi != (0, 0) and live[s]]


def species_factors(species, T_layers, partitionFunction=None, weight=None):
    """qratio[nS][nL] = Q(Tref)/Q(T_k) (misc/hapi.py:11069-11070) and mass[nS] (:11086).
    A species whose weight[s][:] is all zero is filtered out by the reference BEFORE its partition sums and mass are
    looked up (`continue`, misc/hapi.py:11066): it keeps q = mass = 1 here, so an unselected isotopologue without TIPS
    data, or outside the 70-3000 K range, does not raise."""
    nS, nL = len(species), len(T_layers)
    q = np.ones((nS, nL))
    mass = np.ones(nS)
    use = _live_species(species, weight)
    if not use:
        return q, mass
    if partitionFunction is None or partitionFunction is tips.PYTIPS:
        # default TIPS-2011: all (species, layer) pairs in one vectorised pass, plus Q(Tref) as an extra column
        key = tuple(species[s] for s in use)
        plan = _TIPS_PLANS.get(key)
        if plan is None:
            if len(_TIPS_PLANS) > 32:
                _TIPS_PLANS.clear()
            plan = _TIPS_PLANS[key] = (tips.PartitionPlan(key), np.array([tips.molecularMass(*mi) for mi in key]))
        Tq = np.empty(nL + 1)
        Tq[:nL] = T_layers
        Tq[nL] = TREF
        Q = plan[0](Tq)
        q[use] = Q[:, -1:] / Q[:, :-1]
        mass[use] = plan[1]
    else:
        for s in use:
            m, i = species[s]
            mass[s] = tips.molecularMass(m, i)
            qref = partitionFunction(m, i, TREF)
            for k, T in enumerate(T_layers):
                q[s, k] = qref / partitionFunction(m, i, float(T))
    return q, mass


_TIPS_PLANS = {}


def _prologue_inputs(lines, T, p_atm, weight, partitionFunction, qratio, mass):
    """Host inputs of a prologue (rtx_line_prep_profile / rtx_line_prep_axis): n_layers and the (array, pointer) pairs of
    T, p, qratio[nS][nL], weight[nS][nL] and mass[nS]; the arrays stay alive as long as the caller holds the tuple."""
    T = np.atleast_1d(np.asarray(T, dtype=np.float64))
    p_atm = np.atleast_1d(np.asarray(p_atm, dtype=np.float64))
    nL = T.size
    if qratio is None:
        qratio, mass = species_factors(lines.species, T, partitionFunction, weight=weight)
    return nL, (_h(T), _h(p_atm), _h(qratio), _h(np.broadcast_to(weight, (len(lines.species), nL))), _h(mass))


def diluent_mix(lines, diluent, nL):
    """rtx_line_prep_mix's diluent arguments for `diluent` = {name: fraction}, a fraction a scalar or [nS][nL]: (n_dil,
    (set indices int32, pointer), (fractions [n_dil][nS][nL], pointer)), in the dict's order. Names are case-insensitive and
    each key is its own diluent, so "AIR" and "air" are both summed (the reference's loop over Diluent, misc/hapi.py:11090).
    A broadener without any column on the table is left out: its contribution is 0, as the reference's fallbacks make it."""
    names = list(diluent)
    sets = lines.broadener_sets(names)
    nS = len(lines.species)
    idx, fr = [], []
    for k, c in zip(names, sets):
        if c is not None:
            idx.append(c)
            fr.append(np.broadcast_to(np.asarray(diluent[k], dtype=np.float64), (nS, nL)))
    if len(idx) > MAX_DILUENTS:
        raise ValueError("diluent: %d broadeners with columns, at most %d per call" % (len(idx), MAX_DILUENTS))
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    frac = np.ascontiguousarray(np.stack(fr) if fr else np.zeros((0, nS, nL)), dtype=np.float64)
    return len(idx), (idx, idx.ctypes.data_as(C.c_void_p)), (frac, frac.ctypes.data_as(C.c_void_p))


def _host_axis(fn, X):
    """An explicit spectral axis as the prologues take it: contiguous float64 on the host, finite and non-decreasing, as
    the reference's bisect on the axis itself assumes (misc/hapi.py:11133-11134). ValueError in `fn`'s name otherwise."""
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float64).ravel())
    if not np.all(np.isfinite(X)):
        raise ValueError("%s: the axis has non-finite points" % fn)
    if X.size > 1 and np.any(X[1:] < X[:-1]):
        raise ValueError("%s: the axis must be non-decreasing (np.sort it)" % fn)
    return X


def _line_prep(plain, mix, head, lines, nL, diluent, dil_air, dil_self, omega_wing, omega_wing_hw, intensity_threshold, scale,
               profile, st):
    """One prologue call after its leading arguments `head` (everything up to mass): entry point `plain` with the call-wide
    dil_air / dil_self or, with a `diluent` dict, entry point `mix` with diluent_mix's arguments (the loop over Diluent,
    misc/hapi.py:11090), then the scalar tail the two share (include/radtxfr_hip.h)."""
    tail = (float(omega_wing), float(omega_wing_hw), float(intensity_threshold), float(scale), int(profile), st)
    if diluent is None:
        _lib.check(plain(*head, float(dil_air), float(dil_self), *tail))
    else:
        n_dil, idx, frac = diluent_mix(lines, diluent, nL)
        _lib.check(mix(*head, n_dil, idx[1], frac[1], *tail))


def _check_outputs(nL, ld, out_f32, out_f64):
    for o, dt in ((out_f32, torch.float32), (out_f64, torch.float64)):
        if o is not None:
            assert o.dtype == dt and o.is_cuda and o.is_contiguous() and o.shape == (nL, ld), (o.dtype, o.shape)


def voigt_sum(lines, grid, T, p_atm, weight, out_f32=None, out_f64=None, dil_air=1.0, dil_self=0.0, omega_wing=0.0,
              omega_wing_hw=50.0, intensity_threshold=0.0, scale=1.0, partitionFunction=None, qratio=None, mass=None,
              profile=0, diluent=None):
    """Prologue + line-sum for n_layers homogeneous states on `grid` (rtx_line_prep_profile + rtx_voigt_sum);
    profile 0 Voigt, 1 Lorentz, 2 Doppler, 3 speed-dependent Voigt (include/radtxfr_hip.h; 3 needs SD columns in `lines`
    and runs rtx_sdvoigt_sum).
    weight[nS][nL] multiplies S(T) per species and layer. Outputs are [nL][grid.n] device tensors.
    diluent: {broadener: fraction} replacing dil_air / dil_self (rtx_line_prep_mix; profiles 0, 1, 3): a fraction is a
    scalar or [nS][nL] (per species and layer); names other than air / self use the table's gamma_<sp>, n_<sp>, delta_<sp>,
    deltap_<sp>, SD_<sp> columns (LineTable.broadener_sets)."""
    lib = _lib.load()
    nL, env = _prologue_inputs(lines, T, p_atm, weight, partitionFunction, qratio, mass)
    plan = lines.plan(nL, grid.n)
    st = _stream_ptr()
    _line_prep(lib.rtx_line_prep_profile, lib.rtx_line_prep_mix, (plan._h, lines._h, grid.byref(), nL, *(e[1] for e in env)),
               lines, nL, diluent, dil_air, dil_self, omega_wing, omega_wing_hw, intensity_threshold, scale, profile, st)
    ld = grid.n
    _check_outputs(nL, ld, out_f32, out_f64)
    if int(profile) == 3:  # speed-dependent Voigt: its own fp64 line-sum
        _lib.check(lib.rtx_sdvoigt_sum(plan._h, grid.byref(), nL, _ptr(out_f32), _ptr(out_f64), ld, st))
    else:
        _lib.check(lib.rtx_voigt_sum(plan._h, grid.byref(), nL, _ptr(out_f32), _ptr(out_f64), ld, st))
    return out_f32, out_f64


def voigt_sum_rows(lines, grid, n_layers, out_f32, k_lo=0, k_hi=None, skip_rows=None):
    """The sum alone, for a part of the column (rtx_voigt_sum_rows), on the records of the last grid prologue that ran on
    lines.plan(n_layers, grid.n) -- voigt_sum's, say: layers [k_lo, k_hi) into out_f32 [n_layers][grid.n], without the
    64-point rows whose byte in skip_rows is set (a uint8 device tensor, 16 rows per tile of rtx_voigt_tile_points() points,
    padded to whole tiles; None: nothing is skipped). What is written is voigt_sum's, bit for bit; everything else in
    out_f32 keeps its value."""
    lib = _lib.load()
    nL = int(n_layers)
    k_hi = nL if k_hi is None else int(k_hi)
    _check_outputs(nL, grid.n, out_f32, None)
    if skip_rows is not None:
        tile = lib.rtx_voigt_tile_points()
        need = -(-grid.n // tile) * (tile // 64)
        assert skip_rows.dtype == torch.uint8 and skip_rows.is_cuda and skip_rows.is_contiguous() and skip_rows.numel() >= need, \
            (skip_rows.dtype, skip_rows.shape, need)
    _lib.check(lib.rtx_voigt_sum_rows(lines.plan(nL, grid.n)._h, grid.byref(), nL, _ptr(out_f32), grid.n, int(k_lo), k_hi,
                                      _ptr(skip_rows), _stream_ptr(), 0))
    return out_f32


def voigt_sum_axis(lines, X, T, p_atm, weight, out_f32=None, out_f64=None, dil_air=1.0, dil_self=0.0, omega_wing=0.0,
                   omega_wing_hw=50.0, intensity_threshold=0.0, scale=1.0, partitionFunction=None, qratio=None, mass=None,
                   profile=0, diluent=None):
    """voigt_sum on an explicit axis X (host, finite, non-decreasing; need not be uniform) instead of a Grid:
    rtx_line_prep_axis + rtx_voigt_sum_axis. Windows are bisect_right on X itself, as the reference's (misc/hapi.py:
    11133-11134). profile 0 Voigt, 1 Lorentz, 2 Doppler (the speed-dependent sum needs a uniform grid).
    diluent: as for voigt_sum (rtx_line_prep_axis_mix; profiles 0, 1). Outputs are [nL][X.size] device tensors."""
    lib = _lib.load()
    X = _host_axis("voigt_sum_axis", X)
    if int(profile) not in (0, 1, 2):
        raise NotImplementedError("voigt_sum_axis: profile %d; an explicit axis takes Voigt (0), Lorentz (1) or Doppler (2)"
                                  % int(profile))
    nL, env = _prologue_inputs(lines, T, p_atm, weight, partitionFunction, qratio, mass)
    nx = X.size
    plan = lines.plan(nL, max(nx, 1))
    st = _stream_ptr()
    _line_prep(lib.rtx_line_prep_axis, lib.rtx_line_prep_axis_mix,
               (plan._h, lines._h, X.ctypes.data_as(C.c_void_p), nx, nL, *(e[1] for e in env)),
               lines, nL, diluent, dil_air, dil_self, omega_wing, omega_wing_hw, intensity_threshold, scale, profile, st)
    _check_outputs(nL, nx, out_f32, out_f64)
    _lib.check(lib.rtx_voigt_sum_axis(plan._h, nL, _ptr(out_f32), _ptr(out_f64), nx, st))
    return out_f32, out_f64


class HtPlan:
    """Per-(line, state) records and the axis of the Hartmann-Tran sum (rtx_ht)."""

    def __init__(self, lines, max_states, max_points):
        self.max_states, self.max_points = int(max_states), int(max_points)
        self._h = C.c_void_p(0)
        _lib.check(_lib.load().rtx_ht_create(lines.n, self.max_states, self.max_points, C.byref(self._h)))

    def close(self):
        if self._h:
            _lib.load().rtx_ht_free(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _ht_prologue(lines, X, T, p_atm, weight, diluent, omega_wing, omega_wing_hw, intensity_threshold, scale, partitionFunction,
                 qratio, mass):
    """rtx_ht_prep on the table's cached HtPlan (grown on demand): (plan, n_states, nx)."""
    lib = _lib.load()
    X = _host_axis("ht_sum", X)
    nL, env = _prologue_inputs(lines, T, p_atm, weight, partitionFunction, qratio, mass)
    lines.ht_sets(list(diluent))  # the HT columns of every diluent on the device, before the set indices are taken
    n_dil, idx, frac = diluent_mix(lines, diluent, nL)
    plan = lines.__dict__.get("_ht_plan")
    if plan is None or plan.max_states < nL or plan.max_points < X.size:
        if plan is not None:
            plan.close()
        plan = lines.__dict__["_ht_plan"] = HtPlan(lines, max(nL, plan.max_states if plan else 1),
                                                   max(X.size, plan.max_points if plan else 1))
    _lib.check(lib.rtx_ht_prep(plan._h, lines._h, X.ctypes.data_as(C.c_void_p), X.size, nL, *(e[1] for e in env), n_dil, idx[1],
                               frac[1], float(omega_wing), float(omega_wing_hw), float(intensity_threshold), float(scale),
                               _stream_ptr()))
    return plan, nL, X.size


def ht_sum(lines, X, T, p_atm, weight, diluent, out_f32=None, out_f64=None, omega_wing=0.0, omega_wing_hw=50.0,
           intensity_threshold=0.0, scale=1.0, partitionFunction=None, qratio=None, mass=None):
    """Hartmann-Tran line-sum for n_states homogeneous states (T, p_atm: lists) on the explicit axis X (host, finite,
    non-decreasing; any spacing, repeats, a single point): rtx_ht_prep + rtx_ht_sum, the per-line block and the sum of
    absorptionCoefficient_HT (misc/hapi.py:10474-10651) in fp64. diluent = {broadener: fraction}, a fraction a scalar or
    [nS][nL], in the caller's order; each name reads its HT columns of the state's TrefHT bucket (the states of one call may
    fall into different buckets) and falls back to its Voigt-style columns. weight[nS][nL] multiplies S(T).
    Outputs are [nL][X.size] device tensors; without any, a float64 one is made. Returns (out_f32, out_f64)."""
    plan, nL, nx = _ht_prologue(lines, X, T, p_atm, weight, diluent, omega_wing, omega_wing_hw, intensity_threshold, scale,
                                partitionFunction, qratio, mass)
    if out_f32 is None and out_f64 is None:
        out_f64 = torch.zeros((nL, nx), dtype=torch.float64, device=device())
    _check_outputs(nL, nx, out_f32, out_f64)
    if nx == 0:  # an empty tensor has no pointer to pass
        return out_f32, out_f64
    _lib.check(_lib.load().rtx_ht_sum(plan._h, nL, _ptr(out_f32), _ptr(out_f64), nx, _stream_ptr()))
    return out_f32, out_f64


def ht_line_params(lines, X, T, p_atm, weight, diluent, omega_wing=0.0, omega_wing_hw=50.0, intensity_threshold=0.0,
                   partitionFunction=None, qratio=None, mass=None):
    """What ht_sum's prologue makes of every line, without the sum (rtx_ht_prep + rtx_ht_params): a dict of
    params [nL][n_lines][10] (device, fp64, rtx_profile_eval's layout: sg0, GamD, Gam0, Gam2, Shift0, Shift2, anuVC, Re eta,
    Im eta, 0), strength [nL][n_lines] (host; weight * S(T), 0 for a dropped line) and window [nL][n_lines][2] (host, int32:
    the axis indices [lo, hi) the line is summed over)."""
    plan, nL, nx = _ht_prologue(lines, X, T, p_atm, weight, diluent, omega_wing, omega_wing_hw, intensity_threshold, 1.0,
                                partitionFunction, qratio, mass)
    dev = device()
    params = torch.zeros((nL, lines.n, 10), dtype=torch.float64, device=dev)
    strength = torch.zeros((nL, lines.n), dtype=torch.float64, device=dev)
    window = torch.zeros((nL, lines.n, 2), dtype=torch.int32, device=dev)
    for k in range(nL):
        _lib.check(_lib.load().rtx_ht_params(plan._h, k, _ptr(params[k]), _ptr(strength[k]), _ptr(window[k]), _stream_ptr()))
    return {"params": params, "strength": strength.cpu().numpy(), "window": window.cpu().numpy()}


_MF_COLUMNS = {}


def layer_weights_od(species, T, P_pa, PL_km, MF_VAL, MF_ID):
    """weight[nS][nL] for optical depth: n(p,T) * x_m * PL*1e5 for the line's molecule.
    `xs * (ppmv*1e-6) * PL * 1e5` with xs carrying factor = volumeConcentration (HITRAN_units=False); the same operations in
    the same order for every species (one [nS][nL] pass: the species -> mixing-ratio column map is cached)."""
    T = np.asarray(T, dtype=np.float64)
    p_atm = np.asarray(P_pa, dtype=np.float64) / 101325.0
    PL = np.asarray(PL_km, dtype=np.float64)
    MF_VAL = np.asarray(MF_VAL, dtype=np.float64).reshape(T.size, -1)
    ids = tuple(int(v) for v in np.asarray(MF_ID).ravel())
    key = (tuple(species), ids)
    m = _MF_COLUMNS.get(key)
    if m is None:
        if len(_MF_COLUMNS) > 64:
            _MF_COLUMNS.clear()
        col = np.array([ids.index(mm) if mm in ids else 0 for mm, _ in species], dtype=np.int64)
        live = np.array([mm in ids for mm, _ in species], dtype=bool)
        m = _MF_COLUMNS[key] = (col, live, bool(live.all()))
    col, live, all_live = m
    nvol = volumeConcentration(p_atm, T)
    w = nvol * (MF_VAL.T[col] * 1e-6) * PL * 1e5 if len(species) else np.zeros((0, T.size))
    if not all_live:
        w[~live] = 0.0
    return w, p_atm


# HITRAN molecule ids of the gases of StdAtmos (radiative_transfer.options["MFs_ID"]) by formula: the foreign broadeners
# broadening= may name (their columns are gamma_<formula>, n_<formula>, ...)
HITRAN_FORMULA_IDS = {"h2o": 1, "co2": 2, "o3": 3, "n2o": 4, "co": 5, "ch4": 6, "o2": 7, "n2": 22}


def broadening_gases(broadening):
    """The foreign gases of a broadening= option: None for None (air at the layer pressure, the default path), () for
    "self", the formulas after "self" for a tuple such as ("self", "h2o"). Raises ValueError for anything else."""
    if broadening is None:
        return None
    b = (broadening,) if isinstance(broadening, str) else tuple(broadening)
    b = tuple(str(g).lower() for g in b)
    foreign = tuple(g for g in b if g != "self")
    if b.count("self") != 1 or len(set(foreign)) != len(foreign) or any(g not in HITRAN_FORMULA_IDS for g in foreign):
        raise ValueError("broadening=%r: None, \"self\", or a tuple of \"self\" and distinct foreign gases among %s"
                         % (broadening, sorted(HITRAN_FORMULA_IDS)))
    return foreign


def broadening_fractions(species, MF_VAL, MF_ID, foreign=()):
    """The per-layer diluent mix of broadening= (LBLRTM broadens each absorber by its own partial pressure): {"air": [nS][nL],
    "self": [nS][nL], gas: [nS][nL] for each foreign gas}. Species s of molecule m has self fraction x_m (MF_VAL * 1e-6 of
    m's first column in MF_ID, 0 for a molecule not in MF_ID), foreign fraction x_g for every listed gas g != m (0 for a line
    of g itself: it takes self), and air the remainder 1 - (x_m + sum_g x_g)."""
    MF_VAL = np.asarray(MF_VAL, dtype=np.float64)
    ids = [int(v) for v in np.asarray(MF_ID).ravel()]
    nL = MF_VAL.shape[0]
    MF_VAL = MF_VAL.reshape(nL, -1)

    def x_of(m):
        return MF_VAL[:, ids.index(m)] * 1e-6 if m in ids else np.zeros(nL)

    x_self = np.array([x_of(int(m)) for m, _ in species]).reshape(len(species), nL)
    out = {"air": None, "self": x_self}
    total = x_self.copy()
    for g in foreign:
        gid = HITRAN_FORMULA_IDS[g]
        f = np.array([np.zeros(nL) if int(m) == gid else x_of(gid) for m, _ in species]).reshape(len(species), nL)
        out[g] = f
        total = total + f
    out["air"] = 1.0 - total
    return out


def optical_depths(lines, grid, T, P_pa, PL_km, MF_VAL, MF_ID, out=None, broadening=None):
    """OD[nL][grid.n] float32 on the device (layer-major, wavenumber-contiguous).
    broadening: None (every line broadened by air at the layer pressure), "self" or ("self", gas, ...): each species
    broadened by the per-layer mix of broadening_fractions (rtx_line_prep_mix)."""
    T = np.atleast_1d(np.asarray(T, dtype=np.float64))
    w, p_atm = layer_weights_od(lines.species, T, np.atleast_1d(P_pa), np.atleast_1d(PL_km), MF_VAL, MF_ID)
    foreign = broadening_gases(broadening)
    dil = None if foreign is None else broadening_fractions(lines.species, np.asarray(MF_VAL).reshape(T.size, -1), MF_ID, foreign)
    if out is None:
        out = torch.empty((T.size, grid.n), dtype=torch.float32, device=device())
    voigt_sum(lines, grid, T, p_atm, w, out_f32=out, diluent=dil)
    return out


def xs_od(lut, grid_or_offset, T, P_atm, PL, MF, ID, out_f32=None):
    """OD[nL][n] float32 on the device from a cross-section table (afit_xs.XsLut; rtx_xs_od): the layout optical_depths
    returns, so tud() and everything after it take it unchanged. grid_or_offset: a Grid whose axis coincides with a run of
    the table's (ValueError otherwise; a shard of it gives that shard), or the index of the first point on the table's
    axis, n then taken from out_f32. T [K], P_atm [atm], PL [km] per layer, MF[nL][nM] ppmv, ID[nM] HITRAN molecule
    numbers. The node rows and weights are made on the host in float64 (afit_xs.layer_terms: linear in T and in ln p,
    ValueError outside the table or for a molecule it lacks). Bit-identical for every cut of the axis."""
    T = np.atleast_1d(np.asarray(T, dtype=np.float64))
    rows, w = lut.layer_terms(T, P_atm, PL, MF, ID)
    if isinstance(grid_or_offset, Grid):
        off, n = lut.align(grid_or_offset) + grid_or_offset.offset, grid_or_offset.n
    else:
        off, n = int(grid_or_offset), None if out_f32 is None else out_f32.shape[1]
        if n is None:
            raise ValueError("engine.xs_od: an offset needs out_f32 (its row length is the number of points)")
    if out_f32 is None:
        out_f32 = torch.empty((T.size, (n + 3) // 4 * 4), dtype=torch.float32, device=device())[:, :n]  # rows 16 bytes apart
    assert out_f32.dtype == torch.float32 and out_f32.is_cuda and out_f32.dim() == 2 and out_f32.shape[0] == T.size
    assert out_f32.shape[1] >= n and out_f32.stride(1) == 1
    _lib.check(_lib.load().rtx_xs_od(lut._handle(), off, n, T.size, rows.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p),
                                     _ptr(out_f32), out_f32.stride(0) if T.size > 1 else max(out_f32.shape[1], n), _stream_ptr()))
    return out_f32


def xs_od_d(lut, grid_or_offset, T, P_atm, PL, MF, ID, dOD_dT=None, K=None, species=()):
    """The derivative columns of a cross-section table (afit_xs.XsLut; rtx_xs_od_d) WRITTEN to
    float32 device columns in one pass over the table rows: dOD_dT[nL][>= n] = d(OD)/dT per K at fixed p, and K[s][nL][>= n]
    = d(OD)/dMF per ppmv of molecule species[s] (distinct ids of ID, at most 16). Either output may be None, not both; with
    both, they share one row stride. grid_or_offset, T, P_atm, PL, MF, ID as xs_od (n from the outputs with an offset). The
    weights are made on the host in float64 (afit_xs.layer_terms_d): a layer exactly on a T node takes the slope of the cell
    afit_xs.bracket returns for it (the cell to its right; to its left on the last node); a species is range-checked in every
    layer, also where its mixing ratio is 0. Bit-identical for every cut of the axis. Returns (dOD_dT, K)."""
    T = np.atleast_1d(np.asarray(T, dtype=np.float64))
    species = [int(m) for m in species]
    if dOD_dT is None and K is None:
        raise ValueError("xs_od_d: dOD_dT and K are both None")
    if K is not None and len(species) != K.shape[0]:
        raise ValueError("xs_od_d: species %r must name K's %d slots, each once" % (species, K.shape[0]))
    rows, w_T, w_K, idx = lut.layer_terms_d(T, P_atm, PL, MF, ID, species if K is not None else ())
    nL = T.size
    if isinstance(grid_or_offset, Grid):
        off, n = lut.align(grid_or_offset) + grid_or_offset.offset, grid_or_offset.n
    else:
        off, n = int(grid_or_offset), int((dOD_dT if dOD_dT is not None else K).shape[-1])
    lds = []  # the row strides the blocks fix; a single row fixes none
    if dOD_dT is not None:
        assert dOD_dT.dtype == torch.float32 and dOD_dT.is_cuda and dOD_dT.dim() == 2 and dOD_dT.shape[0] == nL
        assert dOD_dT.shape[1] >= n and dOD_dT.stride(1) == 1
        if nL > 1:
            lds.append(dOD_dT.stride(0))
    if K is not None:
        assert K.dtype == torch.float32 and K.is_cuda and K.dim() == 3 and K.shape[1] == nL and K.shape[2] >= n
        assert K.stride(2) == 1
        if nL > 1:
            assert K.shape[0] <= 1 or K.stride(0) == nL * K.stride(1)
            lds.append(K.stride(1))
        elif K.shape[0] > 1:
            lds.append(K.stride(0))
    if len(set(lds)) > 1:
        raise ValueError("xs_od_d: dOD_dT and K must share one row stride, got %r" % (lds,))
    ld = lds[0] if lds else n
    n_spec = len(species) if K is not None else 0
    vp = C.c_void_p
    _lib.check(_lib.load().rtx_xs_od_d(lut._handle(), off, n, nL, rows.ctypes.data_as(vp), w_T.ctypes.data_as(vp), n_spec,
                                       idx.ctypes.data_as(vp), w_K.ctypes.data_as(vp), _ptr(dOD_dT), _ptr(K) if n_spec else None, ld,
                                       _stream_ptr(), 0))
    return dOD_dT, K


def _continuum_call(lib, tables, axes, grid, T, OD, st):
    """rtx_continuum_add on host tables [nC][nL][n_max] float32 with axes [(v0, dv, n)]: OD[nL][>= grid.n] += continuum."""
    v0 = np.array([a[0] for a in axes], dtype=np.float64)
    dv = np.array([a[1] for a in axes], dtype=np.float64)
    nn = np.array([a[2] for a in axes], dtype=np.int32)
    vp = C.c_void_p
    _lib.check(lib.rtx_continuum_add(grid.byref(), T.size, T.ctypes.data_as(vp), len(axes), v0.ctypes.data_as(vp), dv.ctypes.data_as(vp),
                                     nn.ctypes.data_as(vp), tables.ctypes.data_as(vp), tables.shape[2], vp(OD.data_ptr()),
                                     OD.stride(0) if T.size > 1 else max(OD.shape[1], grid.n), st, 0))


def continuum_add(cont, grid, T, P_pa, PL_km, MF_VAL, MF_ID, OD):
    """OD[nL][>= grid.n] float32 on the device += the tabulated continuum `cont` (a continuum.Continuum; DESIGN.md section
    4.22) of the layers T [K], P_pa [Pa], PL_km [km], MF_VAL[nL][nM] ppmv, MF_ID[nM], in place (rtx_continuum_add); returns
    OD. The node rows are made on the host in float64 (Continuum.layer_tables; ValueError for a component whose molecule
    MF_ID lacks). A shard of `grid` gives the bits the whole axis gives."""
    T = np.ascontiguousarray(np.atleast_1d(T), dtype=np.float64)
    tables, axes = cont.layer_tables(T, P_pa, PL_km, MF_VAL, MF_ID)
    assert OD.dtype == torch.float32 and OD.is_cuda and OD.dim() == 2 and OD.shape[0] == T.size
    assert OD.shape[1] >= grid.n and OD.stride(1) == 1
    _continuum_call(_lib.load(), tables, axes, grid, T, OD, _stream_ptr())
    return OD


def continuum_add_d(cont, grid, T, P_pa, PL_km, MF_VAL, MF_ID, dOD_dT=None, K=None, species=()):
    """The derivatives of the tabulated continuum `cont` added in place to float32 device columns
    (rtx_continuum_add_d): dOD_dT[nL][>= grid.n] += d(continuum OD)/dT per K, and K[s][nL][>= grid.n] += d(continuum
    OD)/dMF per ppmv of molecule species[s], for the layers continuum_add takes. species: the molecule ids of K's slots; a
    component whose molecule is not among them adds nothing to K, several components of one molecule add to its slot.
    Either output may be None, not both; with both, they share one row stride. The node rows are made on the host in
    float64 (Continuum.layer_tables_d; ValueError for a component whose molecule MF_ID lacks). Where a component's stencil
    sum is <= 0 its derivatives are 0 (the kink of max(0, .) is given the value 0). A shard of `grid` gives the bits the
    whole axis gives. Returns (dOD_dT, K)."""
    T = np.ascontiguousarray(np.atleast_1d(T), dtype=np.float64)
    species = [int(m) for m in species]
    if dOD_dT is None and K is None:
        raise ValueError("continuum_add_d: dOD_dT and K are both None")
    if K is not None and (len(set(species)) != len(species) or len(species) != K.shape[0]):
        raise ValueError("continuum_add_d: species %r must name K's %d slots, each once" % (species, K.shape[0]))
    A, A_T, A_x, axes = cont.layer_tables_d(T, P_pa, PL_km, MF_VAL, MF_ID)
    nL, n = T.size, grid.n
    lds = []  # the row strides the blocks fix; a single row fixes none
    if dOD_dT is not None:
        assert dOD_dT.dtype == torch.float32 and dOD_dT.is_cuda and dOD_dT.dim() == 2 and dOD_dT.shape[0] == nL
        assert dOD_dT.shape[1] >= n and dOD_dT.stride(1) == 1
        if nL > 1:
            lds.append(dOD_dT.stride(0))
    if K is not None:
        assert K.dtype == torch.float32 and K.is_cuda and K.dim() == 3 and K.shape[1] == nL and K.shape[2] >= n
        assert K.stride(2) == 1
        if nL > 1:
            assert K.shape[0] == 1 or K.stride(0) == nL * K.stride(1)
            lds.append(K.stride(1))
        elif K.shape[0] > 1:
            lds.append(K.stride(0))
    if len(set(lds)) > 1:
        raise ValueError("continuum_add_d: dOD_dT and K must share one row stride, got %r" % (lds,))
    lds = lds or [n]
    slots = np.array([species.index(c.molecule) if K is not None and c.molecule in species else -1 for c in cont.components],
                     dtype=np.int32)
    v0 = np.array([a[0] for a in axes], dtype=np.float64)
    dv = np.array([a[1] for a in axes], dtype=np.float64)
    nn = np.array([a[2] for a in axes], dtype=np.int32)
    vp = C.c_void_p
    _lib.check(_lib.load().rtx_continuum_add_d(grid.byref(), nL, T.ctypes.data_as(vp), len(axes), v0.ctypes.data_as(vp),
                                               dv.ctypes.data_as(vp), nn.ctypes.data_as(vp), A.ctypes.data_as(vp),
                                               A_T.ctypes.data_as(vp), A_x.ctypes.data_as(vp), A.shape[2], slots.ctypes.data_as(vp),
                                               len(species) if K is not None else 0, _ptr(dOD_dT), _ptr(K), lds[0], _stream_ptr(), 0))
    return dOD_dT, K


class TudGeometry(NamedTuple):
    """What tud_geometry returns."""
    Z_s: np.ndarray   # sensor altitudes [nAlt]
    mu: np.ndarray    # slant factors 1 / cos(theta_r) [nMu]
    mask: np.ndarray  # uint8 [nAlt][nL]: layer k lies below sensor altitude a (Z <= zs)
    n_down: int       # layers the downwelling sweeps run over


def tud_geometry(Z, Altitudes, theta_r):
    """The sensor geometry of a TUD call as rtx_tud and its derivatives take it (radiative_transfer.py:346-370): a
    TudGeometry of Z_s and mu (contiguous float64), the contiguous Z <= zs masks and n_down."""
    Z = np.atleast_1d(np.asarray(Z, dtype=np.float64))
    Z_s = np.array([Altitudes], dtype=np.float64).ravel()
    mu = np.ascontiguousarray(np.array([1.0 / np.cos(np.asarray(theta_r, dtype=np.float64))], dtype=np.float64).ravel())
    mask = np.ascontiguousarray(np.stack([(Z <= zs) for zs in Z_s]).astype(np.uint8))
    n_down = int(mask[-1].sum())  # quirk 3: nL is overwritten by the LAST altitude's count (:353, :370)
    return TudGeometry(Z_s, mu, mask, n_down)


def _check_tud_outputs(tau, Lu, Ld, nrow, n):
    """Assert that (tau, Lu, Ld) are float32 device tensors rtx_tud can write nrow rows of n points into -- tau / Lu
    [nrow][>= n] with unit stride along the wavenumbers and a common row stride, Ld [>= n] -- and return that row stride,
    the library's ld_out (include/radtxfr_hip.h)."""
    for t in (tau, Lu):
        assert t.dtype == torch.float32 and t.is_cuda and t.dim() == 2 and t.shape[0] == nrow
        assert t.shape[1] >= n and t.stride(1) == 1 and t.stride(0) == tau.stride(0)
    assert Ld.dtype == torch.float32 and Ld.is_cuda and Ld.numel() >= n and Ld.stride(0) == 1
    return tau.stride(0) if tau.shape[0] > 1 else max(tau.shape[1], n)  # the stride of a size-1 dimension is arbitrary


def tud(OD, grid, T, Z, Altitudes=(500,), theta_r=0.0, N_angle=30, returnOD=False, per_angle=False, out=None,
        od_nonneg=False):
    """tau[nAlt*nMu][n], Lu[nAlt*nMu][n], Ld[n] float32 device tensors from OD[nL][n] (rtx_tud).
    out=(tau, Lu, Ld): write into caller-owned tensors (tau/Lu [nAlt*nMu][>=n] with a common row stride),
    e.g. the rows of the packed block a wavenumber shard all-gathers.
    od_nonneg=True: the caller vouches that every OD value is finite and >= 0 (RTX_TUD_OD_NONNEG, include/radtxfr_hip.h):
    a single (altitude, slant) pair may then pass over the layers an opaque column hides from every output."""
    lib = _lib.load()
    T = np.atleast_1d(np.asarray(T, dtype=np.float64))
    Z_s, mu_s, mask, n_down = tud_geometry(Z, Altitudes, theta_r)
    nL = T.size
    assert OD.dtype == torch.float32 and OD.is_cuda and OD.dim() == 2 and OD.shape[0] == nL and OD.shape[1] >= grid.n
    assert OD.stride(1) == 1
    if mu_s.size > TUD_MAX_MU:
        # more slant paths than one launch takes (radiative_transfer.py:346-356 loops over any number): blocks of
        # TUD_MAX_MU, each a launch of its own; the downwelling (independent of mu) is simply recomputed
        if out is not None:
            raise ValueError("engine.tud: out= is limited to %d slant paths per call" % TUD_MAX_MU)
        th = np.asarray(theta_r, dtype=np.float64).ravel()
        tau = torch.empty((Z_s.size, mu_s.size, grid.n), dtype=torch.float32, device=OD.device)
        Lu = torch.empty_like(tau)
        Ld_ang = None
        for m0 in range(0, mu_s.size, TUD_MAX_MU):
            m1 = min(m0 + TUD_MAX_MU, mu_s.size)
            # the per-stream downwelling radiances do not depend on the slant paths: taken from the first block
            res = tud(OD, grid, T, Z, Altitudes=Altitudes, theta_r=th[m0:m1], N_angle=N_angle, returnOD=returnOD,
                      per_angle=per_angle and m0 == 0, od_nonneg=od_nonneg)
            t_c, l_c, Ld_c = res[:3]
            if m0 == 0:
                Ld = Ld_c
                Ld_ang = res[4] if per_angle else None
            tau[:, m0:m1] = t_c.view(Z_s.size, m1 - m0, grid.n)
            Lu[:, m0:m1] = l_c.view(Z_s.size, m1 - m0, grid.n)
        if per_angle:
            return tau.view(-1, grid.n), Lu.view(-1, grid.n), Ld, (Z_s.size, mu_s.size), Ld_ang
        return tau.view(-1, grid.n), Lu.view(-1, grid.n), Ld, (Z_s.size, mu_s.size)
    dev = OD.device
    if out is None:
        tau = torch.empty((Z_s.size * mu_s.size, grid.n), dtype=torch.float32, device=dev)
        Lu = torch.empty_like(tau)
        Ld = torch.empty((grid.n,), dtype=torch.float32, device=dev)
    else:
        tau, Lu, Ld = out
    ld_out = _check_tud_outputs(tau, Lu, Ld, Z_s.size * mu_s.size, grid.n)
    # rows of the per-stream output use the same leading dimension as tau / Lu (include/radtxfr_hip.h: [n_angle][ld_out])
    Ld_ang = torch.empty((int(N_angle), ld_out), dtype=torch.float32, device=dev) if per_angle else None
    T_h, T_p = _h(T)
    mu_h, mu_p = _h(mu_s)
    _lib.check(lib.rtx_tud_opts(_ptr(OD), OD.stride(0), grid.byref(), nL, T_p, Z_s.size, mask.ctypes.data_as(C.c_void_p),
                                mu_s.size, mu_p, n_down, int(N_angle), int(bool(returnOD)), _ptr(tau), _ptr(Lu), _ptr(Ld),
                                _ptr(Ld_ang), ld_out, _stream_ptr(), TUD_OD_NONNEG if od_nonneg else 0))
    if per_angle:
        return tau, Lu, Ld, (Z_s.size, mu_s.size), Ld_ang[:, :grid.n]
    return tau, Lu, Ld, (Z_s.size, mu_s.size)


class TudRunner:
    """compute_TUD for a stream of atmospheres on one spectral grid / line table / altitude grid (the reference's outer
    loop, Generate_LWIR_TUD.py:117-150): everything that does not depend on the atmosphere -- grid, prep object, sensor
    altitude masks, slant factors, device buffers, the ctypes argument objects -- is set up once; run() does the
    per-atmosphere host factors (TIPS ratios, column weights) and ONE call into the library (rtx_compute_tud: prologue +
    line-sum + TUD enqueued back to back). Outputs are float32 device tensors owned by the runner (or `out`), overwritten
    by the next run(): tau, Lu [nAlt*nMu][n], Ld [n], OD [nL][n].
    broadening: None (the fused rtx_compute_tud), "self" or ("self", gas, ...): each species broadened by its per-layer
    mix (broadening_fractions), run as rtx_line_prep_mix + rtx_voigt_sum + rtx_tud -- the same line-sum and TUD kernels.
    xs_lut: an afit_xs.XsLut instead of `lines` (None then): the optical depths come from the table (rtx_xs_od + rtx_tud);
    `grid` must coincide with a run of the table's axis. Not with broadening (fixed when the table was made).
    continuum: a continuum.Continuum added to the optical depths of whichever branch made them,
    between them and rtx_tud (rtx_continuum_add); the default branch then runs rtx_line_prep + rtx_voigt_sum +
    rtx_continuum_add + rtx_tud as separate calls. None: every branch is what it is without the option.
    keep_od: whether self.OD must be complete after run(). None, the default: a buffer the runner allocated itself is
    scratch, a buffer the caller gave (OD=, or assigned to the attribute later) is kept complete; True / False override.
    Scratch matters only to the fused call (rtx_compute_tud_opts, RTX_CTUD_OD_SCRATCH) on an opaque column with one
    altitude and one slant path: tau, Lu and Ld are the same bits, but OD[k][i] is then UNSPECIFIED (stale, never
    written) for the middle layers k in [4, k_top - 8), k_top = (layers below the sensor - 1) & ~3, of every block of 64
    points, counted from the grid shard's first, that the TUD pass could finish without them. Whoever reads run.OD
    afterwards passes keep_od=True (the derivative front half does)."""

    def __init__(self, lines, grid, Z, n_layers=None, Altitudes=(500,), theta_r=0.0, N_angle=30, returnOD=False, out=None,
                 OD=None, plan=None, broadening=None, xs_lut=None, continuum=None, keep_od=None):
        self.lib = _lib.load()
        self.lines, self.grid = lines, grid
        self.continuum = continuum
        self.foreign = broadening_gases(broadening)
        self.xs_lut = xs_lut
        if xs_lut is not None:
            if broadening is not None:
                raise NotImplementedError("xs_lut with broadening=%r: a table's broadening was fixed when it was made" % (broadening,))
            self._xs_off = xs_lut.align(grid) + grid.offset
        Z = np.atleast_1d(np.asarray(Z, dtype=np.float64))
        self.nL = int(Z.size if n_layers is None else n_layers)
        Z_s, self.mu, self.mask, self.n_down = tud_geometry(Z, Altitudes, theta_r)
        if self.mu.size > TUD_MAX_MU:
            raise ValueError("TudRunner takes at most %d slant paths" % TUD_MAX_MU)
        self.shape = (Z_s.size, self.mu.size)
        self.N_angle, self.returnOD = int(N_angle), int(bool(returnOD))
        dev = device()
        nrow = Z_s.size * self.mu.size
        self.OD = OD if OD is not None else torch.empty((self.nL, grid.n), dtype=torch.float32, device=dev)
        self.keep_od = keep_od
        self._own_od = None if OD is not None else self.OD  # the buffer that is scratch unless told otherwise
        if out is None:
            self.tau = torch.empty((nrow, grid.n), dtype=torch.float32, device=dev)
            self.Lu = torch.empty_like(self.tau)
            self.Ld = torch.empty((grid.n,), dtype=torch.float32, device=dev)
        else:
            self.tau, self.Lu, self.Ld = out
        self.set_outputs(self.tau, self.Lu, self.Ld)
        # plan: a VoigtPlan of the caller's (two pipelines on one device must not share per-(line, layer) records);
        # default = the table's cached plan, shared by everything that runs on the device's current stream
        if xs_lut is not None:
            self.plan = None
            if OD is None:  # rows 16 bytes apart whatever n: rtx_xs_od's vector stores
                self.OD = torch.empty((self.nL, (grid.n + 3) // 4 * 4), dtype=torch.float32, device=dev)[:, :grid.n]
            return
        self.plan = plan if plan is not None else lines.plan(self.nL, grid.n)
        self._env = np.empty(2 * self.nL + 2 * len(lines.species) * self.nL + len(lines.species), dtype=np.float64)

    def set_outputs(self, tau, Lu, Ld):
        """Point the next run() at other output tensors (e.g. the other half of a double-buffered packed block)."""
        self._ld_out = _check_tud_outputs(tau, Lu, Ld, self.shape[0] * self.shape[1], self.grid.n)
        self.tau, self.Lu, self.Ld = tau, Lu, Ld
        self._ptrs = (C.c_void_p(tau.data_ptr()), C.c_void_p(Lu.data_ptr()), C.c_void_p(Ld.data_ptr()))

    def _add_continuum(self, T, P_pa, PL_km, MF_VAL, MF_ID, st):
        tables, axes = self.continuum.layer_tables(T, P_pa, PL_km, MF_VAL, MF_ID)
        _continuum_call(self.lib, tables, axes, self.grid, T, self.OD, st)

    def run(self, T, P_pa, PL_km, MF_VAL, MF_ID, partitionFunction=None):
        nL, lines = self.nL, self.lines
        T = np.ascontiguousarray(T, dtype=np.float64)
        assert T.size == nL
        if self.xs_lut is not None:
            vp, st = C.c_void_p, _stream_ptr()
            rows, wx = self.xs_lut.layer_terms(T, np.asarray(P_pa, dtype=np.float64) / 101325.0, PL_km, MF_VAL, MF_ID)
            with trace_range("rtx_xs_od + rtx_tud"):
                _lib.check(self.lib.rtx_xs_od(self.xs_lut._handle(), self._xs_off, self.grid.n, nL, rows.ctypes.data_as(vp),
                                              wx.ctypes.data_as(vp), vp(self.OD.data_ptr()), self.OD.stride(0), st))
                if self.continuum is not None:
                    self._add_continuum(T, P_pa, PL_km, MF_VAL, MF_ID, st)
                _lib.check(self.lib.rtx_tud(
                    vp(self.OD.data_ptr()), self.OD.stride(0), self.grid.byref(), nL, T.ctypes.data_as(vp), self.shape[0],
                    self.mask.ctypes.data_as(vp), self.shape[1], self.mu.ctypes.data_as(vp), self.n_down, self.N_angle, self.returnOD,
                    self._ptrs[0], self._ptrs[1], self._ptrs[2], None, self._ld_out, st))
            return self.tau, self.Lu, self.Ld
        w, p_atm = layer_weights_od(lines.species, T, P_pa, PL_km, MF_VAL, MF_ID)
        qratio, mass = species_factors(lines.species, T, partitionFunction, weight=w)
        nS = len(lines.species)
        env = self._env  # T | p | qratio | weight | mass, one contiguous host block
        env[0:nL] = T
        env[nL:2 * nL] = p_atm
        env[2 * nL:2 * nL + nS * nL] = qratio.ravel()
        env[2 * nL + nS * nL:2 * nL + 2 * nS * nL] = w.ravel()
        env[2 * nL + 2 * nS * nL:] = mass
        base = env.ctypes.data
        vp = C.c_void_p
        if self.foreign is not None:
            dil = broadening_fractions(lines.species, np.asarray(MF_VAL, dtype=np.float64).reshape(nL, -1), MF_ID, self.foreign)
            st = _stream_ptr()
            with trace_range("rtx_line_prep_mix + rtx_voigt_sum + rtx_tud"):
                _line_prep(None, self.lib.rtx_line_prep_mix,
                           (self.plan._h, lines._h, self.grid.byref(), nL, vp(base), vp(base + 8 * nL), vp(base + 16 * nL),
                            vp(base + 8 * (2 * nL + nS * nL)), vp(base + 8 * (2 * nL + 2 * nS * nL))),
                           lines, nL, dil, None, None, 0.0, 50.0, 0.0, 1.0, 0, st)
                _lib.check(self.lib.rtx_voigt_sum(self.plan._h, self.grid.byref(), nL, vp(self.OD.data_ptr()), None,
                                                  self.OD.stride(0), st))
                if self.continuum is not None:
                    self._add_continuum(T, P_pa, PL_km, MF_VAL, MF_ID, st)
                _lib.check(self.lib.rtx_tud(
                    vp(self.OD.data_ptr()), self.OD.stride(0), self.grid.byref(), nL, vp(base), self.shape[0],
                    self.mask.ctypes.data_as(vp), self.shape[1], self.mu.ctypes.data_as(vp), self.n_down, self.N_angle, self.returnOD,
                    self._ptrs[0], self._ptrs[1], self._ptrs[2], None, self._ld_out, st))
            return self.tau, self.Lu, self.Ld
        if self.continuum is not None:
            st = _stream_ptr()
            # what rtx_compute_tud hands its TUD step (include/radtxfr_hip.h): the continuum adds only values >= 0
            nonneg = TUD_OD_NONNEG if bool(np.all(np.isfinite(env)) and env.min() >= 0.0) else 0
            with trace_range("rtx_line_prep + rtx_voigt_sum + rtx_continuum_add + rtx_tud"):
                _lib.check(self.lib.rtx_line_prep(
                    self.plan._h, lines._h, self.grid.byref(), nL, vp(base), vp(base + 8 * nL), vp(base + 16 * nL),
                    vp(base + 8 * (2 * nL + nS * nL)), vp(base + 8 * (2 * nL + 2 * nS * nL)), 1.0, 0.0, 0.0, 50.0, 0.0, 1.0, st))
                _lib.check(self.lib.rtx_voigt_sum(self.plan._h, self.grid.byref(), nL, vp(self.OD.data_ptr()), None,
                                                  self.OD.stride(0), st))
                self._add_continuum(T, P_pa, PL_km, MF_VAL, MF_ID, st)
                _lib.check(self.lib.rtx_tud_opts(
                    vp(self.OD.data_ptr()), self.OD.stride(0), self.grid.byref(), nL, vp(base), self.shape[0],
                    self.mask.ctypes.data_as(vp), self.shape[1], self.mu.ctypes.data_as(vp), self.n_down, self.N_angle, self.returnOD,
                    self._ptrs[0], self._ptrs[1], self._ptrs[2], None, self._ld_out, st, nonneg))
            return self.tau, self.Lu, self.Ld
        scratch = (self.OD is self._own_od) if self.keep_od is None else not self.keep_od
        with trace_range("rtx_compute_tud"):
            _lib.check(self.lib.rtx_compute_tud_opts(
                self.plan._h, lines._h, self.grid.byref(), nL, vp(base), vp(base + 8 * nL), vp(base + 16 * nL),
                vp(base + 8 * (2 * nL + nS * nL)), vp(base + 8 * (2 * nL + 2 * nS * nL)), 1.0, 0.0, 0.0, 50.0, 0.0,
                self.shape[0], self.mask.ctypes.data_as(vp), self.shape[1], self.mu.ctypes.data_as(vp), self.n_down, self.N_angle,
                self.returnOD, vp(self.OD.data_ptr()), self.OD.stride(0), self._ptrs[0], self._ptrs[1], self._ptrs[2], self._ld_out,
                _stream_ptr(), CTUD_OD_SCRATCH if scratch else 0))
        return self.tau, self.Lu, self.Ld


class TudPipelines:
    """P independent TudRunners for a stream of atmospheres on one grid / table: each has its own HIP stream, per-(line,
    layer) records (VoigtPlan), optical-depth buffer and outputs, and atmosphere k runs on pipeline k mod P. Within a
    pipeline the four kernels of a step run back to back; across pipelines the fp64 prologue and the HBM-bound TUD pass of
    one atmosphere share the chip with the VALU-bound line-sum of the next (C3 on MI355X, bench.py: 1.97 / 1.90 / 1.90 /
    1.91 ms per atmosphere with 1 / 2 / 3 / 4 pipelines; profiles/r3_time_pipeline.txt). Results are the single-runner results bit for bit.
    outs: optional list of P (tau, Lu, Ld) output triples (e.g. rows of packed blocks that are all-gathered).
    kw: TudRunner's keywords (Altitudes, theta_r, N_angle, returnOD, broadening, continuum, keep_od: each pipeline's
    optical-depth buffer is the runner's own, hence scratch unless keep_od=True)."""

    def __init__(self, lines, grid, Z, n_layers=None, n_pipes=2, outs=None, **kw):
        self.streams = [torch.cuda.Stream() for _ in range(int(n_pipes))]
        self.runs = []
        nL = int(np.atleast_1d(Z).size if n_layers is None else n_layers)
        for p, s in enumerate(self.streams):
            with torch.cuda.stream(s):
                self.runs.append(TudRunner(lines, grid, Z, n_layers=nL, plan=VoigtPlan(lines, nL, grid.n),
                                           out=None if outs is None else outs[p], **kw))
        self.k = 0

    def run(self, T, P_pa, PL_km, MF_VAL, MF_ID):
        """Enqueue one atmosphere on the next pipeline; returns (pipeline index, (tau, Lu, Ld) of that pipeline)."""
        p = self.k % len(self.runs)
        self.k += 1
        with torch.cuda.stream(self.streams[p]):
            out = self.runs[p].run(T, P_pa, PL_km, MF_VAL, MF_ID)
        return p, out

    def close(self):
        torch.cuda.synchronize()
        for r in self.runs:
            r.plan.close()
        self.runs = []


def planck(X, T, wavelength=False, grid=None):
    """out[nx][nT] float64 device tensor (rtx_planck). X: device fp64 tensor, or None with a Grid."""
    lib = _lib.load()
    nx = grid.n if X is None else X.numel()
    out = torch.empty((nx, T.numel()), dtype=torch.float64, device=T.device)
    _lib.check(lib.rtx_planck(grid.byref() if grid is not None else None, _ptr(X), nx, _ptr(T), T.numel(),
                              int(bool(wavelength)), _ptr(out), _stream_ptr()))
    return out


def apparent_radiance(X, emis, Ts, tau, La, Ld, dT=None, return_Ls=False):
    """Device tensors in, L[nX][nE][nA][nT or 1] float32 out (rtx_apparent_radiance)."""
    lib = _lib.load()
    nX, nE = emis.shape
    nA = Ts.numel()
    nT = dT.numel() if dT is not None else 1
    L = torch.empty((nX, nE, nA, nT), dtype=torch.float32, device=emis.device)
    Ls = torch.empty_like(L) if return_Ls else None
    if L.numel() == 0:  # an empty dT has no pointer: the library would take it for "no dT axis" and ask for L
        return L, Ls
    _lib.check(lib.rtx_apparent_radiance(_ptr(X), nX, _ptr(emis), nE, _ptr(Ts), nA, _ptr(tau), _ptr(La), _ptr(Ld),
                                         _ptr(dT), nT if dT is not None else 0, _ptr(L), _ptr(Ls), _stream_ptr()))
    return L, Ls


def ils(kind, Y, centre, sigma, X=None, grid=None):
    """Y[nx][nS] float32 device -> Y_out[nB][nS] float32 (rtx_ils). kind 0 triangle, 1 Gaussian."""
    lib = _lib.load()
    assert Y.dtype == torch.float32 and Y.is_cuda and Y.dim() == 2 and Y.stride(1) == 1
    nx, nS = Y.shape
    nB = centre.numel()
    out = torch.empty((nB, nS), dtype=torch.float32, device=Y.device)
    _lib.check(lib.rtx_ils(int(kind), grid.byref() if grid is not None else None, _ptr(X), nx, _ptr(Y), nS, Y.stride(0),
                           nB, _ptr(centre), _ptr(sigma), _ptr(out), _stream_ptr()))
    return out


def max_wing_cm(columns, T_layers, p_atm_layers, omega_wing=0.0, omega_wing_hw=50.0):
    """Upper bound [cm^-1] of OmegaWingF (misc/hapi.py:11131) over all lines and layers, plus the largest
    pressure shift: how far outside a wavenumber shard a line centre can sit and still contribute.
    Used to give each GPU only the lines that can reach its shard."""
    T = np.asarray(T_layers, dtype=np.float64)
    p = np.asarray(p_atm_layers, dtype=np.float64)
    nu = np.asarray(columns["nu"], dtype=np.float64)
    if nu.size == 0:
        return float(omega_wing)
    g = float(np.max(columns["gamma_air"]))
    n_hi, n_lo = float(np.max(columns["n_air"])), float(np.min(columns["n_air"]))
    tr = TREF / T
    g0 = g * np.max(p * np.maximum(tr ** n_hi, tr ** n_lo))
    gd = 3.6e-7 * float(np.max(nu)) * np.sqrt(float(np.max(T)) / 1.0)  # mass >= 1 g/mol: generous
    shift = float(np.max(np.abs(columns["delta_air"]))) * float(np.max(p))
    return max(float(omega_wing), omega_wing_hw * g0, omega_wing_hw * min(gd, 10.0 * g0 + 1.0)) + shift


# Relative cost of one line-sum tile, fitted (non-negative least squares) to the step time of 32 contiguous chunks of the
# C3 grid on MI355X (tools/shard_balance.py, profiles/r3_shard_balance.txt): per line whose window reaches the tile
# (classification + row-level evaluations) and per Weideman band row; the line centres' near-zone rows come out
# collinear with the reach count (0), and the per-(tile, layer) constant (zeroing, interpolation, stores, the TUD pass)
# cannot be told from the per-launch constant on equal chunks -- a small value keeps empty spans from costing nothing.
TILE_COST = {"tile": 100.0, "reach": 30.0, "centre": 0.0, "band_row": 24.0}


def tile_costs(columns, xmin, step, n_total, T_layers, p_atm_layers, tile, omega_wing=0.0, omega_wing_hw=50.0, coef=None):
    """Estimated line-sum + TUD cost of every `tile`-point tile of the axis xmin + i*step, i < n_total, summed over the
    layers: cost[n_tiles]. Host arithmetic on the table's columns only (windows W = max(OmegaWing, HW*gamma0, HW*gammaD),
    misc/hapi.py:11131; band half-width (15 - y)/cte where y < 15, :9840) -- the same on every rank. Used to cut
    wavenumber shards of equal COST rather than equal length (dist.tile_aligned_bounds)."""
    c = dict(TILE_COST)
    if coef:
        c.update(coef)
    T = np.atleast_1d(np.asarray(T_layers, dtype=np.float64))
    p = np.atleast_1d(np.asarray(p_atm_layers, dtype=np.float64))
    n_tiles = (int(n_total) + int(tile) - 1) // int(tile)
    cost = np.full(n_tiles, c["tile"] * T.size)
    nu = np.asarray(columns["nu"], dtype=np.float64)
    if nu.size == 0:
        return cost
    ga = np.asarray(columns["gamma_air"], dtype=np.float64)
    na = np.asarray(columns["n_air"], dtype=np.float64)
    M = np.asarray(columns["molec_id"]).astype(np.int64)
    I = np.asarray(columns["local_iso_id"]).astype(np.int64)
    mass = np.ones(nu.size)
    code = M * 1000003 + I
    for u in np.unique(code):
        try:
            mass[code == u] = tips.molecularMass(int(u // 1000003), int(u % 1000003))
        except Exception:
            pass  # unknown isotopologue: the default only skews the estimate
    span = float(step) * int(tile)
    tc = np.floor((nu - xmin) / span).astype(np.int64)  # tile of the line centre
    inside = (tc >= 0) & (tc < n_tiles)
    sqln2 = np.sqrt(np.log(2.0))
    for k in range(T.size):
        g0 = ga * p[k] * (TREF / T[k]) ** na
        gd = np.sqrt(2.0 * CBOLTS * T[k] * np.log(2.0) / (mass * 1.66053873e-27 * 1000.0) / 2.99792458e10 ** 2) * nu
        W = np.maximum(omega_wing, np.maximum(omega_wing_hw * g0, omega_wing_hw * gd))
        t_lo = np.clip(np.floor((nu - W - xmin) / span), 0, n_tiles).astype(np.int64)
        t_hi = np.clip(np.floor((nu + W - xmin) / span) + 1, 0, n_tiles).astype(np.int64)
        d = np.bincount(t_lo, minlength=n_tiles + 1)[:n_tiles + 1] - np.bincount(t_hi, minlength=n_tiles + 1)[:n_tiles + 1]
        cost += c["reach"] * np.cumsum(d)[:n_tiles]
        y = g0 * sqln2 / gd
        rows = np.where(y < 15.0, 2.0 * (15.0 - y) * gd / sqln2 / (64.0 * step) + 1.0, 0.0)
        cost += np.bincount(tc[inside], weights=(c["centre"] + c["band_row"] * rows)[inside], minlength=n_tiles)[:n_tiles]
    return cost


# ---- post-processing: smooth / reduceResolution (rtx_fir_reflect, rtx_cubic_resample) ------------
_WINDOWS = ("flat", "hanning", "hamming", "bartlett", "blackman")


def window_taps(window_len, window="hanning", symmetric=False):
    """FIR taps and centre of radiative_transfer.smooth (:1314-1324) in the convention of rtx_fir_reflect:
    out[i] = sum_k taps[k] * x[R(i + k - centre)]. symmetric=True gives reduceResolution's symmetrised smoother
    (:1331), the mean of smoothing x and smoothing x reversed."""
    wl = int(window_len)
    w = np.ones(wl, "d") if window == "flat" else getattr(np, window)(wl)
    w = w / w.sum()
    ix0 = int(np.ceil(wl / 2 - 1))
    c = wl - 1 - ix0  # out[i] = sum_q w[wl-1-q] * s[i + ix0 + q],  s[k] = x[R(k - (wl - 1))]
    fwd = w[::-1].copy()
    if not symmetric:
        return fwd, c
    # the reversed pass uses offsets -(k - c): offsets d in [-(wl-1-c), c]
    m = max(c, wl - 1 - c)
    taps = np.zeros(2 * m + 1)
    for k in range(wl):
        taps[m + (k - c)] += 0.5 * fwd[k]
        taps[m - (k - c)] += 0.5 * fwd[k]
    return taps, m


def fir_reflect(Y, taps, centre):
    """Y [rows][n] float32/float64 device tensor -> [rows][n] float64 (rtx_fir_reflect)."""
    lib = _lib.load()
    assert Y.is_cuda and Y.dim() == 2 and Y.stride(1) == 1 and Y.dtype in (torch.float32, torch.float64)
    rows, n = Y.shape
    taps = np.ascontiguousarray(taps, dtype=np.float64)
    out = torch.empty((rows, n), dtype=torch.float64, device=Y.device)
    ld = Y.stride(0) if rows > 1 else n  # the stride of a size-1 dimension is arbitrary
    _lib.check(lib.rtx_fir_reflect(_ptr(Y), int(Y.dtype == torch.float64), ld, rows, n, taps.ctypes.data, taps.size,
                                   int(centre), _ptr(out), out.stride(0), _stream_ptr()))
    return out


def same_window(n, m):
    """(first, n_out) of numpy.convolve(a[n], v[m], mode='same') inside the full convolution: max(n, m) points from
    (min(n, m) - 1) // 2 (NumPy swaps the operands when v is the longer one; checked against NumPy, tests/test_spectra_host.py)."""
    return (min(n, m) - 1) // 2, max(n, m)


def fir_same(Y, taps, out_scale, first, n_out):
    """Y [rows][n] float32/float64 device tensor -> [rows][n_out] float64: out_scale times the points [first, first + n_out)
    of the zero-padded linear convolution of every row with `taps` (host fp64) (rtx_fir_same)."""
    lib = _lib.load()
    assert Y.is_cuda and Y.dim() == 2 and Y.stride(1) == 1 and Y.dtype in (torch.float32, torch.float64)
    rows, n = Y.shape
    taps = np.ascontiguousarray(taps, dtype=np.float64)
    out = torch.empty((rows, int(n_out)), dtype=torch.float64, device=Y.device)
    ld = Y.stride(0) if rows > 1 else n  # the stride of a size-1 dimension is arbitrary
    with torch.cuda.device(Y.device):
        _lib.check(lib.rtx_fir_same(_ptr(Y), int(Y.dtype == torch.float64), ld, rows, n, taps.ctypes.data, taps.size,
                                    float(out_scale), int(first), int(n_out), _ptr(out), max(int(n_out), 1), _stream_ptr()))
    return out


def hapi_spectrum(kind, K, l, T=0.0, X=None):
    """K [rows][n] float32/float64 device tensor of absorption coefficients -> [rows][n] float64 (rtx_hapi_spectrum):
    kind 0 transmittance, 1 absorption, 2 radiance (X: [n] fp64 device wavenumbers, T in K)."""
    lib = _lib.load()
    assert K.is_cuda and K.dim() == 2 and K.stride(1) == 1 and K.dtype in (torch.float32, torch.float64)
    rows, n = K.shape
    if X is not None:
        assert X.is_cuda and X.dtype == torch.float64 and X.dim() == 1 and X.is_contiguous() and X.numel() == n
    out = torch.empty((rows, n), dtype=torch.float64, device=K.device)
    with torch.cuda.device(K.device):
        _lib.check(lib.rtx_hapi_spectrum(int(kind), None, _ptr(X), _ptr(K), int(K.dtype == torch.float64), rows, n,
                                         K.stride(0) if rows > 1 else n, float(l), float(T), _ptr(out), max(n, 1), _stream_ptr()))
    return out


# ---- line-profile functions with explicit per-line parameters (rtx_profile_eval / _sum, rtx_cpf_eval) -----------------
LS_PCQSDHC, LS_LORENTZ, LS_DOPPLER = 0, 1, 2
CPF_HUM1_WEI, CPF_CPF3 = 0, 1
PROFILE_NPAR = 10  # sg0, GamD, Gam0, Gam2, Shift0, Shift2, anuVC, Re eta, Im eta, pad


def _f64_vector(t, what):
    assert t.is_cuda and t.dtype == torch.float64 and t.dim() == 1 and t.is_contiguous(), what


def profile_eval(kind, params, sg, imag=True):
    """params [nL][10] and sg [n], fp64 device tensors -> (re, im) [nL][n] fp64 (im None when imag=False): every line at
    every point (rtx_profile_eval); kind LS_PCQSDHC / LS_LORENTZ / LS_DOPPLER."""
    lib = _lib.load()
    assert params.is_cuda and params.dtype == torch.float64 and params.dim() == 2 and params.shape[1] == PROFILE_NPAR and params.is_contiguous()
    _f64_vector(sg, "sg")
    nL, n = params.shape[0], sg.numel()
    re = torch.empty((nL, n), dtype=torch.float64, device=sg.device)
    im = torch.empty((nL, n), dtype=torch.float64, device=sg.device) if imag else None
    if nL == 0 or n == 0:  # an empty tensor has no pointer to pass
        return re, im
    with torch.cuda.device(sg.device):
        _lib.check(lib.rtx_profile_eval(int(kind), nL, _ptr(params), _ptr(sg), n, _ptr(re), _ptr(im), n, _stream_ptr()))
    return re, im


def profile_sum(params, w_re, w_im, sg):
    """out[i] = sum_l w_re[l] Re LS_l(sg[i]) + w_im[l] Im LS_l(sg[i]) of the pcqsdhc profile, [n] fp64 (rtx_profile_sum);
    w_im None = zeros. Lines in index order, bit-reproducible."""
    lib = _lib.load()
    assert params.is_cuda and params.dtype == torch.float64 and params.dim() == 2 and params.shape[1] == PROFILE_NPAR and params.is_contiguous()
    _f64_vector(sg, "sg")
    _f64_vector(w_re, "w_re")
    nL, n = params.shape[0], sg.numel()
    assert w_re.numel() == nL
    if w_im is not None:
        _f64_vector(w_im, "w_im")
        assert w_im.numel() == nL
    if nL == 0 or n == 0:  # the empty sum; an empty tensor has no pointer to pass
        return torch.zeros(n, dtype=torch.float64, device=sg.device)
    out = torch.empty(n, dtype=torch.float64, device=sg.device)
    with torch.cuda.device(sg.device):
        _lib.check(lib.rtx_profile_sum(nL, _ptr(params), _ptr(w_re), _ptr(w_im), _ptr(sg), n, _ptr(out), _stream_ptr()))
    return out


def cpf_eval(kind, x, y):
    """hum1_wei (CPF_HUM1_WEI) or cpf3 (CPF_CPF3) of x + iy elementwise, [n] fp64 device tensors -> (re, im) (rtx_cpf_eval)."""
    lib = _lib.load()
    _f64_vector(x, "x")
    _f64_vector(y, "y")
    assert x.numel() == y.numel() and x.device == y.device
    re, im = torch.empty_like(x), torch.empty_like(x)
    if x.numel() == 0:
        return re, im
    with torch.cuda.device(x.device):
        _lib.check(lib.rtx_cpf_eval(int(kind), _ptr(x), _ptr(y), x.numel(), _ptr(re), _ptr(im), _stream_ptr()))
    return re, im


def cubic_resample(Ysm, x0, h, x_out, checked=True):
    """Cubic spline through every sample of the uniform axis x0 + i*h, at x_out (device fp64): [rows][n_out] fp64.
    checked=False: the caller has verified the range of x_out on the host; no device read-back, no synchronisation."""
    lib = _lib.load()
    assert Ysm.is_cuda and Ysm.dtype == torch.float64 and Ysm.dim() == 2 and Ysm.stride(1) == 1
    assert x_out.is_cuda and x_out.dtype == torch.float64 and x_out.dim() == 1 and x_out.is_contiguous()
    rows, n = Ysm.shape
    out = torch.empty((rows, x_out.numel()), dtype=torch.float64, device=Ysm.device)
    fn = lib.rtx_cubic_resample if checked else lib.rtx_cubic_resample_unchecked
    _lib.check(fn(_ptr(Ysm), Ysm.stride(0) if rows > 1 else n, rows, n, float(x0), float(h), _ptr(x_out), x_out.numel(),
                  _ptr(out), out.stride(0), _stream_ptr()))
    return out


SPL_END_GUARD = 24   # knots between the last output of an end region and the cut of its local spline (0.268^24 = 2e-14)
SPL_END_MAX = 768    # local knots rtx_cubic_end takes


def _smoothed_axis_ends(x0, h, n, taps, c, m):
    """The first and last m values of the reference's smoothed axis X_ = sm(X) (radiative_transfer.py:1331-1334): the
    symmetrised window applied to X = x0 + i*h with smooth()'s reflection padding. Host arithmetic on the axis only.
    Both reflections at both ends: on a short axis (m == n, or a window that reaches from the first m samples past the
    last one) a knot's window crosses the far end as well."""
    k = np.arange(taps.size)
    i = np.arange(m)

    def sm(first):
        j = (first + i)[:, None] + k[None, :] - c
        j = np.where(j < 0, -j, j)
        j = np.where(j >= n, 2 * (n - 1) - j, j)
        return (taps[None, :] * (x0 + h * j)).sum(axis=1)

    return sm(0), sm(n - m)


def _reduce_plan(x0, h, n, dX, N, window, x_out, device):
    """Everything of reduceResolution that does not depend on the spectra: output axis, window taps, the split of the
    outputs into a low-end region, the interior and a high-end region, and the true knots of the two end regions."""
    sm_factor = int(np.round(dX / h))
    if sm_factor < 3:
        raise ValueError(f"reduceResolution: dX/dX_in rounds to {sm_factor}; the window needs at least 3 samples")
    if window not in _WINDOWS:
        raise ValueError(f"window must be one of {_WINDOWS}")
    taps, c = window_taps(sm_factor, window, symmetric=True)
    if x_out is None:
        # the reference's default axis runs from X_[smFactor] to X_[-smFactor-1] (:1336-1338); a window length inside, the
        # smoothed axis is the axis itself
        xa, xb = x0 + sm_factor * h, x0 + (n - sm_factor - 1) * h
        v = N * (xb - xa) / dX
        x_out = np.linspace(xa, xb, int(np.ceil(v - 1e-9 * max(1.0, abs(v)))) + 1)  # see the shim's docstring: rounding-proof ceil
    x_out = np.ascontiguousarray(x_out, dtype=np.float64)
    # The interior evaluation (uniform knots, cardinal spline) is offered where the reflection padding of smooth() and the
    # not-a-knot end condition have faded below 1e-11: `margin` samples inside. Outputs nearer an end go through the local
    # not-a-knot spline on the true knots (rtx_cubic_end).
    margin = max((sm_factor + 1) // 2 + 20, 27)  # (27: what rtx_cubic_resample itself asks of its abscissae)
    x_lo, x_hi = x0 + margin * h, x0 + (n - 1 - margin) * h
    n_lo = n_hi = 0
    ends = None
    m = min(n, margin + SPL_END_GUARD + 2 + (sm_factor + 1) // 2)
    # a short axis (m == n <= 2 margin + 6): the local spline is the spline on all knots; with the not-a-knot condition at
    # both ends it is the reference's own, so one launch takes every output and nothing is cut
    whole = m == n
    if x_out.size and (whole or x_out.min() < x_lo or x_out.max() > x_hi):
        if m > SPL_END_MAX:
            raise NotImplementedError(
                f"reduceResolution: output points within {margin} samples of an end of the input axis need a local spline of {m} "
                f"knots (window {sm_factor}); supported up to {SPL_END_MAX}")
        if whole:
            n_lo = x_out.size
        else:  # n > 2 margin + 6: the two end regions do not meet
            if np.any(np.diff(x_out) < 0):
                raise NotImplementedError("reduceResolution: X_out must be ascending when it reaches into the end regions of the axis")
            n_lo = int(np.searchsorted(x_out, x_lo, side="left"))
            n_hi = int(x_out.size - np.searchsorted(x_out, x_hi, side="right"))
        k_lo, k_hi = _smoothed_axis_ends(x0, h, n, taps, c, m)
        # the knots here and the reference's sm(X) differ in the last bit (1e-13 at 900 cm^-1), so an X_out that starts or
        # ends on the reference's own first or last knot may overshoot ours by that: accepted up to the guard figure of the
        # point count above, and evaluated by the first or last interval's cubic
        tol = 1e-9 * h
        if (n_lo and x_out.min() < k_lo[0] - tol) or ((n_hi or whole) and x_out.max() > k_hi[-1] + tol):
            raise NotImplementedError("reduceResolution: X_out outside the smoothed axis (extrapolation is not supported)")
        if not whole and ((n_lo and x_out[n_lo - 1] > k_lo[m - 1 - SPL_END_GUARD]) or (n_hi and x_out[x_out.size - n_hi] < k_hi[SPL_END_GUARD])):
            raise NotImplementedError("reduceResolution: the axis is too short for its end regions to be treated separately")
        ends = (m, torch.as_tensor(k_lo, device=device), torch.as_tensor(k_hi, device=device), whole)
    return x_out, torch.as_tensor(x_out, device=device), taps, c, n_lo, n_hi, ends


def _reduce_apply(Y, x0, h, n, plan, checked):
    x_out, x_dev, taps, c, n_lo, n_hi, ends = plan
    Ysm = fir_reflect(Y, taps, c)
    n_out = x_out.size
    n_mid = n_out - n_lo - n_hi
    if not (n_lo or n_hi):
        return x_out, cubic_resample(Ysm, x0, h, x_dev, checked=checked)
    lib = _lib.load()
    rows = Ysm.shape[0]
    out = torch.empty((rows, n_out), dtype=torch.float64, device=Y.device)
    ld = Ysm.stride(0) if rows > 1 else n
    m, k_lo, k_hi, whole = ends
    if n_lo:
        _lib.check(lib.rtx_cubic_end(_ptr(Ysm), ld, rows, 0, m, 0, int(whole), _ptr(k_lo), C.c_void_p(x_dev.data_ptr()), n_lo,
                                     C.c_void_p(out.data_ptr()), out.stride(0), _stream_ptr()))
    if n_mid:
        out[:, n_lo:n_lo + n_mid] = cubic_resample(Ysm, x0, h, x_dev[n_lo:n_lo + n_mid], checked=checked)
    if n_hi:
        _lib.check(lib.rtx_cubic_end(_ptr(Ysm), ld, rows, n - m, m, 1, 0, _ptr(k_hi), C.c_void_p(x_dev.data_ptr() + 8 * (n_out - n_hi)), n_hi,
                                     C.c_void_p(out.data_ptr() + 8 * (n_out - n_hi)), out.stride(0), _stream_ptr()))
    return x_out, out


def reduce_resolution(Y, x0, h, n, dX, N=4, window="hanning", x_out=None):
    """Device-resident reduceResolution: Y [rows][n] (float32 as rtx_tud writes it, or float64) on the uniform axis
    x0 + i*h -> (x_out host fp64, Y_out [rows][n_out] fp64 device). See radiative_transfer.reduceResolution."""
    return _reduce_apply(Y, x0, h, n, _reduce_plan(x0, h, n, dX, N, window, x_out, Y.device), checked=True)


_REDUCE_PLANS = {}


def reduce_resolution_cached(Y, x0, h, n, dX, N=4, window="hanning"):
    """reduce_resolution on its default output axis, for a stream of spectra on one grid (compute_TUD_batch: every
    atmosphere of a batch is reduced the same way): the output axis (host and device copies), the symmetrised window taps
    (a Python loop over the window), the end-region knots and the range checks are made once per (axis, dX, N, window,
    device) instead of per spectrum -- together they cost more host time than the device needs for the whole atmosphere --
    and the resampling runs without its device read-back."""
    key = (float(x0), float(h), int(n), float(dX), int(N), window, Y.device.index)
    plan = _REDUCE_PLANS.get(key)
    if plan is None:
        if len(_REDUCE_PLANS) > 8:
            _REDUCE_PLANS.clear()
        plan = _REDUCE_PLANS[key] = _reduce_plan(x0, h, n, dX, N, window, None, Y.device)
    return _reduce_apply(Y, x0, h, n, plan, checked=False)


# ---- TUD Jacobian (rtx_line_prep_window + rtx_voigt_sum for dOD/dx, rtx_tud_jacobian) -------------------------------
JAC_BLOCK_BYTES = 2 << 30  # J block per rtx_tud_jacobian launch (float32 [n_wrt][layers][rows][n])
# rtx_tud_jacobian's limits (include/radtxfr_hip.h), checked here before any device work
JAC_MAX_LAYERS, JAC_MAX_ALT, JAC_MAX_ANGLES, JAC_MAX_SPEC = 128, 16, 96, 16


def jacobian_limits(n_layers, n_alt, n_angle, n_spec):
    """Raise ValueError where rtx_tud_jacobian would refuse the shape (host-only check)."""
    if not 1 <= int(n_layers) <= JAC_MAX_LAYERS:
        raise ValueError("Jacobian: %d layers, supported 1..%d" % (n_layers, JAC_MAX_LAYERS))
    if not 1 <= int(n_alt) <= JAC_MAX_ALT:
        raise ValueError("Jacobian: %d sensor altitudes, supported 1..%d" % (n_alt, JAC_MAX_ALT))
    if not 1 <= int(n_angle) <= JAC_MAX_ANGLES:
        raise ValueError("Jacobian: N_angle=%d, supported 1..%d" % (n_angle, JAC_MAX_ANGLES))
    if int(n_spec) > JAC_MAX_SPEC:
        raise ValueError("Jacobian: %d species in wrt, supported up to %d" % (n_spec, JAC_MAX_SPEC))


def voigt_sum_window(lines, grid, T, T_win, p_atm, weight, out_f32, qratio=None, mass=None, partitionFunction=None):
    """voigt_sum with every line's window taken at the layer temperatures T_win instead of T (rtx_line_prep_window +
    rtx_voigt_sum): strengths, partition sums and widths at T, supports at T_win. Output [nL][grid.n] float32."""
    lib = _lib.load()
    nL, env = _prologue_inputs(lines, T, p_atm, weight, partitionFunction, qratio, mass)
    T_win, T_win_p = _h(np.atleast_1d(T_win))
    assert T_win.size == nL
    plan = lines.plan(nL, grid.n)
    st = _stream_ptr()
    T_e, p_e, q_e, w_e, m_e = (e[1] for e in env)
    _lib.check(lib.rtx_line_prep_window(plan._h, lines._h, grid.byref(), nL, T_e, T_win_p, p_e, q_e, w_e, m_e, 1.0, 0.0,
                                        0.0, 50.0, 0.0, 1.0, 0, st))
    _check_outputs(nL, grid.n, out_f32, None)
    _lib.check(lib.rtx_voigt_sum(plan._h, grid.byref(), nL, _ptr(out_f32), None, grid.n, st))
    return out_f32


DT_METHODS = ("fd", "analytic")


def check_dT_method(dT_method):
    """Raise ValueError unless dT_method names a way to form dOD/dT (host-only check)."""
    if dT_method not in DT_METHODS:
        raise ValueError("dT_method: %r, expected one of %r" % (dT_method, DT_METHODS))


def species_dlnq_dT(species, T_layers, weight=None):
    """d ln(qratio) / dT [nS][nL] = -Q'(T_k) / Q(T_k) from TIPS-2011 (tips.partition_sums_dT: analytic). A species that
    species_factors leaves at q = 1 (no isotopologue, or weight all zero) has derivative 0."""
    nS, nL = len(species), len(T_layers)
    out = np.zeros((nS, nL))
    use = _live_species(species, weight)
    if use:
        key = [species[s] for s in use]
        out[use] = -tips.partition_sums_dT(key, T_layers) / tips.partition_sums(key, T_layers)
    return out


def voigt_sum_dT(lines, grid, T, p_atm, weight, out_f32=None, dlnw_dT=None, out_f64=None, dil_air=1.0, dil_self=0.0,
                 omega_wing=0.0, omega_wing_hw=50.0, intensity_threshold=0.0, scale=1.0, qratio=None, mass=None, dlnq_dT=None):
    """Analytic temperature derivative of voigt_sum's Voigt line-sum (rtx_line_prep_dt + rtx_voigt_sum_dt): per layer,
    d/dT of the sum at (T, p) with every line's window held fixed. dlnw_dT [nS][nL] (or broadcastable): d ln(weight) / dT,
    default -1/T, the optical-depth weights of layer_weights_od. dlnq_dT: d ln(qratio) / dT, default TIPS-2011's own
    derivative (required with a qratio of the caller's). Uniform grids (a Grid), the Voigt profile and the call-wide
    dil_air / dil_self only. Outputs [nL][grid.n] device tensors; after the call the plan also holds voigt_sum's records."""
    lib = _lib.load()
    if not isinstance(grid, Grid):
        raise TypeError("voigt_sum_dT: a uniform Grid is required (explicit axes are not supported)")
    if qratio is not None and dlnq_dT is None:
        raise ValueError("voigt_sum_dT: a caller's qratio needs its dlnq_dT")
    nL, env = _prologue_inputs(lines, T, p_atm, weight, None, qratio, mass)
    T_a = env[0][0]
    nS = len(lines.species)
    if dlnq_dT is None:
        dlnq_dT = species_dlnq_dT(lines.species, T_a, weight=weight)
    if dlnw_dT is None:
        dlnw_dT = -1.0 / T_a
    dlnsw = np.ascontiguousarray(np.broadcast_to(np.asarray(dlnq_dT, dtype=np.float64), (nS, nL))
                                 + np.broadcast_to(np.asarray(dlnw_dT, dtype=np.float64), (nS, nL)))
    plan = lines.plan(nL, grid.n)
    st = _stream_ptr()
    _lib.check(lib.rtx_line_prep_dt(plan._h, lines._h, grid.byref(), nL, *(e[1] for e in env), dlnsw.ctypes.data_as(C.c_void_p),
                                    float(dil_air), float(dil_self), float(omega_wing), float(omega_wing_hw),
                                    float(intensity_threshold), float(scale), st))
    _check_outputs(nL, grid.n, out_f32, out_f64)
    _lib.check(lib.rtx_voigt_sum_dt(plan._h, grid.byref(), nL, _ptr(out_f32), _ptr(out_f64), grid.n, st))
    return out_f32, out_f64


def jacobian_species_columns(MF_ID, wrt):
    """Column of MFs_VAL each species entry of `wrt` differentiates (its first occurrence in MF_ID, as layer_weights_od maps
    a line's molecule to a column). Raises ValueError for an id not in MF_ID."""
    ids = [int(v) for v in np.asarray(MF_ID).ravel()]
    cols = []
    for w in wrt:
        if isinstance(w, str):
            continue
        if int(w) not in ids:
            raise ValueError("wrt: molecule id %r is not in MFs_ID %r" % (w, ids))
        cols.append(ids.index(int(w)))
    return cols


class JacobianStages(NamedTuple):
    """What _jacobian_stages returns: the device columns tud_jacobian_from_od and tud_vjp_from_od take."""
    T: np.ndarray        # layer temperatures, contiguous float64 [nL]
    Z: np.ndarray        # layer altitudes, float64 [nL]
    layers: np.ndarray   # int32 layer indices, in output order
    t_pos: int           # position of "T" on the wrt axis
    tau: torch.Tensor    # base state, float32: tau / Lu [nAlt][n], Ld [n], OD [nL][n]
    Lu: torch.Tensor
    Ld: torch.Tensor
    OD: torch.Tensor
    OD_plus: Optional[torch.Tensor]   # [nL][n] at T + fd_step_T, windows at T ("fd" with "T" in wrt, else None)
    OD_minus: Optional[torch.Tensor]  # [nL][n] at T - fd_step_T, likewise
    dOD_dT: Optional[torch.Tensor]    # [nL][n] the derivative itself ("analytic" with "T" in wrt, else None)
    K: Optional[torch.Tensor]         # [n_spec][nL][n] OD per ppmv of each species of wrt, or None


def _jacobian_stages(what, lines, grid, Z, T, P_pa, PL_km, MF_VAL, MF_ID, Altitudes, theta_r, N_angle, returnOD, wrt, layers,
                     fd_step_T, mark, dT_method="fd", continuum=None, xs_lut=None):
    """The stages tud_jacobian and tud_vjp share: argument checks, the base state (exactly what compute_TUD runs), the
    line-sums at T -+ fd_step_T with every line's window at T (skipped without "T" in wrt; dT_method "analytic": one
    voigt_sum_dT instead, fd_step_T ignored) and the line-sum of each species of wrt at 1 ppmv (what the reference's
    caller gets from perturbed atmospheres, Generate_LWIR_TUD.py:55-71). Returns a JacobianStages.
    continuum: a continuum.Continuum in the base state (what compute_TUD(continuum=) runs) and in
    every column: "fd" adds the continuum at T -+ fd_step_T to the two line-sums (continuum_add: the full definition at
    that temperature), "analytic" its dOD/dT to the line-sum's, and each species column gets its dOD/dMF at the state
    (the self term is quadratic in the mixing ratio) -- the last two in one continuum_add_d. None: nothing changes.
    xs_lut: an afit_xs.XsLut instead of `lines` (None then): the base state is what
    compute_TUD(xs_lut=) runs, "analytic" takes dOD/dT and every species column from ONE rtx_xs_od_d, "fd" takes the forward
    rule (xs_od) at T -+ fd_step_T -- a layer the step pushes out of the table raises the forward's ValueError -- and the
    species columns from rtx_xs_od_d. A layer exactly on a T node takes the slope of the cell afit_xs.bracket returns for it
    (the cell to its right; to its left on the last node). A continuum composes unchanged after either."""
    check_dT_method(dT_method)
    T = np.ascontiguousarray(np.atleast_1d(np.asarray(T, dtype=np.float64)))
    Z = np.atleast_1d(np.asarray(Z, dtype=np.float64))
    nL = T.size
    P_pa = np.atleast_1d(np.asarray(P_pa, dtype=np.float64))
    PL_km = np.atleast_1d(np.asarray(PL_km, dtype=np.float64))
    MF_VAL = np.asarray(MF_VAL, dtype=np.float64).reshape(nL, -1)
    wrt = tuple(wrt)
    if len(set(wrt)) != len(wrt) or any(isinstance(w_, str) and w_ != "T" for w_ in wrt):
        raise ValueError("wrt: distinct entries, each \"T\" or a molecule id of MFs_ID (got %r)" % (wrt,))
    with_T = "T" in wrt
    spec_cols = jacobian_species_columns(MF_ID, wrt)
    layers = np.arange(nL, dtype=np.int32) if layers is None else np.ascontiguousarray(np.asarray(layers, dtype=np.int32).ravel())
    if layers.size == 0 or layers.min() < 0 or layers.max() >= nL:
        raise ValueError("layers: indices must lie in [0, %d)" % nL)
    if with_T and dT_method == "fd" and not (fd_step_T > 0.0):
        raise ValueError("fd_step_T must be > 0")
    th = np.asarray(theta_r, dtype=np.float64).ravel()
    if th.size != 1:
        raise NotImplementedError("%s: one slant path (theta_r) per call" % what)
    jacobian_limits(nL, np.array([Altitudes]).size, N_angle, len(spec_cols))
    dev = device()
    # base state: exactly what compute_TUD runs
    run = TudRunner(lines, grid, Z, n_layers=nL, Altitudes=Altitudes, theta_r=theta_r, N_angle=N_angle, returnOD=returnOD,
                    continuum=continuum, xs_lut=xs_lut, keep_od=True)  # the derivatives read every layer of OD
    tau, Lu, Ld = run.run(T, P_pa, PL_km, MF_VAL, MF_ID)
    OD = run.OD
    if mark:
        mark("base")
    n = grid.n
    ODp = ODm = dOD = None
    if xs_lut is not None:
        return _xs_jacobian_columns(xs_lut, grid, Z, T, P_pa, PL_km, MF_VAL, MF_ID, wrt, layers, fd_step_T, mark, dT_method, continuum,
                                    tau, Lu, Ld, OD)
    if with_T and dT_method == "analytic":
        dOD = torch.empty((nL, n), dtype=torch.float32, device=dev)
        w, p_atm = layer_weights_od(lines.species, T, P_pa, PL_km, MF_VAL, MF_ID)
        voigt_sum_dT(lines, grid, T, p_atm, w, dOD)
    elif with_T:
        ODp = torch.empty((nL, n), dtype=torch.float32, device=dev)
        ODm = torch.empty_like(ODp)
        for sgn, out in ((1.0, ODp), (-1.0, ODm)):
            Ts = T + sgn * float(fd_step_T)
            w, p_atm = layer_weights_od(lines.species, Ts, P_pa, PL_km, MF_VAL, MF_ID)
            voigt_sum_window(lines, grid, Ts, T, p_atm, w, out)
            if continuum is not None:
                continuum_add(continuum, grid, Ts, P_pa, PL_km, MF_VAL, MF_ID, out)
    if mark:
        mark("T")
    K = None
    if spec_cols:
        K = torch.empty((len(spec_cols), nL, n), dtype=torch.float32, device=dev)
        for s, c in enumerate(spec_cols):
            unit = np.zeros_like(MF_VAL)
            unit[:, c] = 1.0
            w, p_atm = layer_weights_od(lines.species, T, P_pa, PL_km, unit, MF_ID)
            voigt_sum(lines, grid, T, p_atm, w, out_f32=K[s])
    if continuum is not None and (dOD is not None or K is not None):
        continuum_add_d(continuum, grid, T, P_pa, PL_km, MF_VAL, MF_ID, dOD_dT=dOD, K=K,
                        species=[w_ for w_ in wrt if not isinstance(w_, str)])
    if mark:
        mark("species")
    # the wrt axis of the result follows `wrt`: T at t_pos and the species (K's order = their order in wrt) around it
    t_pos = wrt.index("T") if with_T else 0
    return JacobianStages(T, Z, layers, t_pos, tau, Lu, Ld, OD, ODp, ODm, dOD, K)


def _xs_jacobian_columns(lut, grid, Z, T, P_pa, PL_km, MF_VAL, MF_ID, wrt, layers, fd_step_T, mark, dT_method, continuum, tau, Lu, Ld, OD):
    """_jacobian_stages' columns from a cross-section table, after its checks and base state: every
    column has the row stride of the runner's OD (rows 16 bytes apart)."""
    nL, n, ld, dev = T.size, grid.n, OD.stride(0), OD.device
    with_T = "T" in wrt
    species = [w_ for w_ in wrt if not isinstance(w_, str)]
    P_atm = P_pa / 101325.0
    column = lambda: torch.empty((nL, ld), dtype=torch.float32, device=dev)[:, :n]
    ODp = ODm = dOD = K = None
    if with_T and dT_method == "analytic":
        dOD = column()
    elif with_T:
        ODp, ODm = column(), column()
        for sgn, out in ((1.0, ODp), (-1.0, ODm)):
            Ts = T + sgn * float(fd_step_T)
            xs_od(lut, grid, Ts, P_atm, PL_km, MF_VAL, MF_ID, out_f32=out)  # the forward rule at that temperature
            if continuum is not None:
                continuum_add(continuum, grid, Ts, P_pa, PL_km, MF_VAL, MF_ID, out)
    if species:
        K = torch.empty((len(species), nL, ld), dtype=torch.float32, device=dev)[:, :, :n]
    if dOD is not None or K is not None:
        xs_od_d(lut, grid, T, P_atm, PL_km, MF_VAL, MF_ID, dOD_dT=dOD, K=K, species=species)
    if mark:
        mark("T")
    if continuum is not None and (dOD is not None or K is not None):
        continuum_add_d(continuum, grid, T, P_pa, PL_km, MF_VAL, MF_ID, dOD_dT=dOD, K=K, species=species)
    if mark:
        mark("species")
    return JacobianStages(T, Z, layers, wrt.index("T") if with_T else 0, tau, Lu, Ld, OD, ODp, ODm, dOD, K)


def tud_jacobian(lines, grid, Z, T, P_pa, PL_km, MF_VAL, MF_ID, Altitudes=(500,), theta_r=0.0, N_angle=30, returnOD=False,
                 wrt=("T",), layers=None, fd_step_T=0.5, block_bytes=JAC_BLOCK_BYTES, on_block=None, mark=None, dT_method="fd",
                 continuum=None, xs_lut=None):
    """compute_TUD's outputs and their Jacobian with respect to layer temperatures and mixing ratios, on the device.

    wrt: "T" and/or molecule ids of MF_ID (T, when present, is computed first whatever its position: J's wrt axis follows
    `wrt`). layers: layer indices (default all), in output order. Returns (tau, Lu, Ld, OD, J): float32 device tensors,
    tau / Lu [nAlt][n], Ld [n], OD [nL][n] bit-identical to TudRunner / compute_TUD, J [n_wrt][n_layers][2 nAlt + 1][n]
    (rows: tau per altitude, L-up per altitude, Ld). With on_block(k0, k1, J_block) J is not kept: each block of layers
    (at most block_bytes of float32) is handed to the callback as soon as it is written, and None is returned for J.
    mark(name): called after each stage is enqueued ("base", "T", "species", "jacobian"), for timing.

    dOD/dT is the central difference of two line-sums at T -+ fd_step_T with every line's window at T (voigt_sum_window),
    or with dT_method="analytic" the closed-form derivative of the line-sum with the same fixed windows (voigt_sum_dT: one
    sum instead of two, fd_step_T ignored); any other dT_method raises ValueError before device work.
    dOD/dMF of a species is the line-sum of that species alone at 1 ppmv (OD is linear in each mixing ratio).
    continuum: a continuum.Continuum carried through the base state and every derivative (_jacobian_stages; DESIGN.md
    section 4.23). OD is then no longer linear in a mixing ratio: a species entry of J is the local derivative at the
    state, per ppmv; where a component's stencil sum is <= 0 its derivatives are 0 (the kink of max(0, .) is given 0).
    xs_lut: an afit_xs.XsLut instead of `lines` (None then): every column comes from the table (_jacobian_stages; DESIGN.md
    section 4.24). OD is piecewise in T there: a layer exactly on a T node takes the slope of the cell afit_xs.bracket
    returns for it, the cell to its right (to its left on the last node)."""
    s = _jacobian_stages("tud_jacobian", lines, grid, Z, T, P_pa, PL_km, MF_VAL, MF_ID, Altitudes, theta_r, N_angle, returnOD, wrt,
                         layers, fd_step_T, mark, dT_method, continuum, xs_lut)
    J = tud_jacobian_from_od(s.OD, s.OD_plus, s.OD_minus, fd_step_T, s.K, s.tau, grid, s.T, s.Z, Altitudes=Altitudes,
                             theta_r=theta_r, N_angle=N_angle, returnOD=returnOD, layers=s.layers, t_pos=s.t_pos,
                             block_bytes=block_bytes, on_block=on_block, mark=mark, dOD_dT=s.dOD_dT)
    return s.tau, s.Lu, s.Ld, s.OD, J


class _JacobianFront(NamedTuple):
    """What _jacobian_front returns."""
    entry: object       # the library entry point the columns select
    lead: tuple         # its arguments up to return_od
    layers: np.ndarray  # int32 layer indices, contiguous
    n_alt: int
    n_wrt: int
    keep: tuple         # host arrays `lead` points into


def _jacobian_front(what, fd_entry, dod_entry, OD, OD_plus, OD_minus, fd_step_T, K, tau, grid, T, Z, Altitudes, theta_r, N_angle,
                    returnOD, layers, dOD_dT):
    """What rtx_tud_jacobian and rtx_tud_vjp share ahead of their own arguments (include/radtxfr_hip.h: the first 18 of
    either), for `what`_from_od: host conversions, the rule that dOD_dT stands in for OD_plus / OD_minus / fd_step_T, the
    layout checks of the device columns, the sensor geometry (tud_geometry; one slant path) and n_wrt. Returns a
    _JacobianFront whose entry is fd_entry, or dod_entry with a dOD_dT."""
    T = np.ascontiguousarray(np.atleast_1d(np.asarray(T, dtype=np.float64)))
    nL = T.size
    layers = np.arange(nL, dtype=np.int32) if layers is None else np.ascontiguousarray(np.asarray(layers, dtype=np.int32).ravel())
    geo = tud_geometry(Z, Altitudes, theta_r)
    if geo.mu.size != 1:
        raise NotImplementedError("%s: one slant path (theta_r) per call" % what)
    if dOD_dT is not None and (OD_plus is not None or OD_minus is not None):
        raise ValueError("%s_from_od: dOD_dT replaces OD_plus / OD_minus / fd_step_T" % what)
    with_T = OD_plus is not None or dOD_dT is not None
    n_spec = 0 if K is None else int(K.shape[0])
    n, n_alt = grid.n, geo.Z_s.size
    ld = OD.stride(0)
    assert OD.dtype == torch.float32 and OD.is_cuda and OD.dim() == 2 and OD.shape[0] == nL and OD.shape[1] >= n
    assert OD.stride(1) == 1
    for t in (OD_plus, OD_minus, dOD_dT):
        assert t is None or (t.dtype == torch.float32 and t.shape == OD.shape and t.stride() == OD.stride())
    if K is not None:
        assert K.dtype == torch.float32 and K.dim() == 3 and K.shape[1] == nL and K.shape[2] >= n
        assert K.stride(2) == 1 and K.stride(1) == ld and K.stride(0) == nL * ld
    if tau is not None:
        assert tau.dtype == torch.float32 and tau.dim() == 2 and tau.shape[0] == n_alt and tau.shape[1] >= n
        assert tau.stride(1) == 1
    if dOD_dT is not None:
        entry, head = dod_entry, (_ptr(OD), _ptr(dOD_dT), ld)
    else:
        entry, head = fd_entry, (_ptr(OD), _ptr(OD_plus), _ptr(OD_minus), ld, float(fd_step_T))
    lead = head + (_ptr(K), n_spec, _ptr(tau), tau.stride(0) if tau is not None else 0, grid.byref(), nL,
                   T.ctypes.data_as(C.c_void_p), n_alt, geo.mask.ctypes.data_as(C.c_void_p), float(geo.mu[0]), geo.n_down,
                   int(N_angle), int(bool(returnOD)))
    return _JacobianFront(entry, lead, layers, n_alt, int(with_T) + n_spec, (T, geo.mask))


def tud_jacobian_from_od(OD, OD_plus, OD_minus, fd_step_T, K, tau, grid, T, Z, Altitudes=(500,), theta_r=0.0, N_angle=30,
                         returnOD=False, layers=None, t_pos=0, block_bytes=JAC_BLOCK_BYTES, on_block=None, mark=None,
                         dOD_dT=None):
    """rtx_tud_jacobian on given float32 device columns: OD [nL][>=n] (the base state), OD_plus / OD_minus at T -+ fd_step_T
    (or both None: no T rows; or dOD_dT [nL][.] instead of the three, the derivative itself: rtx_tud_jacobian_dod),
    K [n_spec][nL][.] OD per ppmv (or None), all with OD's row stride; tau [nAlt][>=n] the base
    transmittances (None allowed with returnOD). Altitude masks and n_down are formed as TudRunner forms them. Returns J
    [n_wrt][n_layers][2 nAlt + 1][n], T's rows at t_pos and the species in K's order around them, or None with on_block
    (see tud_jacobian)."""
    lib = _lib.load()
    f = _jacobian_front("tud_jacobian", lib.rtx_tud_jacobian, lib.rtx_tud_jacobian_dod, OD, OD_plus, OD_minus, fd_step_T, K, tau,
                        grid, T, Z, Altitudes, theta_r, N_angle, returnOD, layers, dOD_dT)
    layers, n_wrt, n = f.layers, f.n_wrt, grid.n
    nrow = 2 * f.n_alt + 1
    per_layer = n_wrt * nrow * n * 4
    nb = int(max(1, min(layers.size, int(block_bytes) // max(per_layer, 1))))
    dev = OD.device
    J = None if on_block is not None else torch.empty((n_wrt, layers.size, nrow, n), dtype=torch.float32, device=dev)
    st = _stream_ptr()
    for k0 in range(0, layers.size, nb):
        k1 = min(k0 + nb, layers.size)
        blk = torch.empty((n_wrt, k1 - k0, nrow, n), dtype=torch.float32, device=dev)
        lay = np.ascontiguousarray(layers[k0:k1])
        _lib.check(f.entry(*f.lead, lay.ctypes.data_as(C.c_void_p), lay.size, t_pos, _ptr(blk), n, st))
        if mark:
            mark("jacobian")
        if on_block is not None:
            on_block(k0, k1, blk)
        else:
            J[:, k0:k1] = blk
    return J


# ---- adjoint of the TUD Jacobian (rtx_tud_vjp): J^T g for cotangents g on the output rows, J never stored ----------------
VJP_VEC_GROUP = None  # cotangent vectors per rtx_tud_vjp call; None: the library's maximum (rtx_tud_vjp_max_vectors)


def _cotangent(G, lead, n, what):
    """A cotangent as float32 device rows [n_vec] + lead + [>= n] with unit stride along the wavenumbers, or None."""
    if G is None:
        return None
    if not torch.is_tensor(G):
        G = torch.as_tensor(np.asarray(G, dtype=np.float32))
    G = G.to(device=device(), dtype=torch.float32)
    if G.dim() == len(lead) + 1:
        G = G[None]
    if G.dim() != len(lead) + 2 or tuple(G.shape[1:-1]) != tuple(lead) or G.shape[-1] < n or G.shape[0] < 1:
        raise ValueError("%s: shape %r, expected [n_vec]%r[>= %d] (the vector axis may be left out)"
                         % (what, tuple(G.shape), list(lead), n))
    if G.stride(-1) != 1:
        G = G.contiguous()
    return G


def tud_vjp_from_od(OD, OD_plus, OD_minus, fd_step_T, K, tau, grid, T, Z, G_tau=None, G_Lu=None, G_Ld=None, Altitudes=(500,),
                    theta_r=0.0, N_angle=30, returnOD=False, layers=None, t_pos=0, dOD_dT=None):
    """rtx_tud_vjp on given float32 device columns (as tud_jacobian_from_od takes them, dOD_dT included): the adjoint of that
    Jacobian, grad[v][w][k] = sum over wavenumbers and rows of G[v][row] J[w][k][row], float64 on the device, [n_vec][n_wrt][n_layers],
    without J being stored. G_tau, G_Lu: [n_vec][nAlt][>= n], G_Ld: [n_vec][>= n], float32 (NumPy or torch), the vector
    axis optional; a group left None is not evaluated (no G_Ld: no downwelling sweeps; no G_tau: tau may be None). The
    vectors go to the library VJP_VEC_GROUP at a time; the grouping, like the choice and order of layers, changes no bit."""
    lib = _lib.load()
    f = _jacobian_front("tud_vjp", lib.rtx_tud_vjp, lib.rtx_tud_vjp_dod, OD, OD_plus, OD_minus, fd_step_T, K, tau, grid, T, Z,
                        Altitudes, theta_r, N_angle, returnOD, layers, dOD_dT)
    layers, nA, n = f.layers, f.n_alt, grid.n
    G_tau = _cotangent(G_tau, (nA,), n, "G_tau")
    G_Lu = _cotangent(G_Lu, (nA,), n, "G_Lu")
    G_Ld = _cotangent(G_Ld, (), n, "G_Ld")
    given = [g for g in (G_tau, G_Lu, G_Ld) if g is not None]
    if not given:
        raise ValueError("tud_vjp: no cotangent (G_tau, G_Lu and G_Ld are all None)")
    n_vec = int(given[0].shape[0])
    if any(int(g.shape[0]) != n_vec for g in given):
        raise ValueError("tud_vjp: the cotangents disagree on the number of vectors: %r" % [int(g.shape[0]) for g in given])
    # the library takes one leading dimension for the three groups: rows that already share one (padded or not) go as
    # they are, anything else is packed to ld_G = n

    def row_ld(g):
        ld_g = g.stride(-2) if g.shape[-2] > 1 else max(n, g.shape[-1])
        dense = ld_g >= n and g.stride(-1) == 1 and (g.dim() == 2 or g.shape[1] == 1 or g.stride(1) == ld_g)
        outer = ld_g * (g.shape[1] if g.dim() == 3 else 1)
        return ld_g if dense and (g.shape[0] == 1 or g.stride(0) == outer) else None

    lds = set(row_ld(g) for g in given)
    if len(lds) == 1 and None not in lds:
        ld_G = lds.pop()
    else:
        ld_G = n
        G_tau, G_Lu, G_Ld = (None if g is None else g[..., :n].contiguous() for g in (G_tau, G_Lu, G_Ld))
    vstride = {id(g): ld_G * (g.shape[1] if g.dim() == 3 else 1) for g in (G_tau, G_Lu, G_Ld) if g is not None}
    out = torch.empty((n_vec, f.n_wrt, layers.size), dtype=torch.float64, device=OD.device)
    group = int(VJP_VEC_GROUP or lib.rtx_tud_vjp_max_vectors())
    st = _stream_ptr()
    for v0 in range(0, n_vec, group):
        v1 = min(v0 + group, n_vec)
        part = lambda g: None if g is None else C.c_void_p(g.data_ptr() + 4 * v0 * vstride[id(g)])
        _lib.check(f.entry(*f.lead, layers.ctypes.data_as(C.c_void_p), layers.size, t_pos, part(G_tau), part(G_Lu), part(G_Ld),
                           ld_G, v1 - v0, _ptr(out[v0:v1]), st))
    return out


def tud_vjp(lines, grid, Z, T, P_pa, PL_km, MF_VAL, MF_ID, G_tau=None, G_Lu=None, G_Ld=None, Altitudes=(500,), theta_r=0.0,
            N_angle=30, returnOD=False, wrt=("T",), layers=None, fd_step_T=0.5, mark=None, cotangents=None, dT_method="fd",
            continuum=None, xs_lut=None):
    """compute_TUD's outputs and the gradient of a scalar cost with respect to layer temperatures and mixing ratios, given
    the cost's cotangents on the outputs: tud_jacobian's stages (the same base state, T -+ fd_step_T line-sums and species
    line-sums) followed by rtx_tud_vjp instead of rtx_tud_jacobian. wrt, layers, fd_step_T, dT_method as tud_jacobian; G_* as
    tud_vjp_from_od. Returns (tau, Lu, Ld, OD, grad), grad float64 [n_vec][n_wrt][n_layers] on the device, its wrt axis
    following `wrt`. mark(name): after each stage ("base", "T", "species", "vjp").
    cotangents: instead of G_tau / G_Lu / G_Ld, a function (tau, Lu, Ld) -> (G_tau, G_Lu, G_Ld) called once the base state
    exists, for a cost whose cotangents depend on the outputs themselves (rt.compute_band_radiance_vjp: the sensor stage's
    adjoint reads tau, Lu and Ld). The optical depths are computed once either way. continuum, xs_lut: as tud_jacobian."""
    if cotangents is not None and (G_tau is not None or G_Lu is not None or G_Ld is not None):
        raise ValueError("tud_vjp: cotangents= and G_tau / G_Lu / G_Ld exclude each other")
    check_dT_method(dT_method)
    s = _jacobian_stages("tud_vjp", lines, grid, Z, T, P_pa, PL_km, MF_VAL, MF_ID, Altitudes, theta_r, N_angle, returnOD, wrt,
                         layers, fd_step_T, mark, dT_method, continuum, xs_lut)
    if cotangents is not None:
        G_tau, G_Lu, G_Ld = cotangents(s.tau, s.Lu, s.Ld)
    grad = tud_vjp_from_od(s.OD, s.OD_plus, s.OD_minus, fd_step_T, s.K, s.tau, grid, s.T, s.Z, G_tau=G_tau, G_Lu=G_Lu, G_Ld=G_Ld,
                           Altitudes=Altitudes, theta_r=theta_r, N_angle=N_angle, returnOD=returnOD, layers=s.layers,
                           t_pos=s.t_pos, dOD_dT=s.dOD_dT)
    if mark:
        mark("vjp")
    return s.tau, s.Lu, s.Ld, s.OD, grad


# ---- tangent-linear TUD (rtx_tud_jvp): J v for tangents v on (layer T, mixing ratios), J never stored ---------------------
JVP_VEC_GROUP = None  # tangent vectors per rtx_tud_jvp call; None: the library's maximum (rtx_tud_jvp_max_vectors)
JVP_ROWS = ("tau", "La", "Ld")


def tud_jvp_from_od(OD, OD_plus, OD_minus, fd_step_T, K, tau, grid, T, Z, V, Altitudes=(500,), theta_r=0.0, N_angle=30,
                    returnOD=False, layers=None, t_pos=0, rows=JVP_ROWS, dOD_dT=None):
    """rtx_tud_jvp on given float32 device columns (as tud_jacobian_from_od takes them, dOD_dT included): the product of that
    Jacobian with tangent vectors, out[v][row] = sum over wrt slots w and layers k of J[w][k][row] V[v][w][k], without J being
    stored. V: [n_vec][n_wrt][len(layers)] (the vector axis optional), host numbers, taken as float64; wrt slots as J's
    (T at t_pos). It is scattered into the dense all-layer array the library takes: layers not named have tangent 0, the
    entries of a layer index named twice add (in float64, in the order given). rows: which of "tau", "La", "Ld" are
    evaluated (no "Ld": no downwelling sweeps; no "tau": tau may be None). Returns {row name: float32 device tensor},
    "tau" / "La" [n_vec][nAlt][n], "Ld" [n_vec][n]. The vectors go to the library JVP_VEC_GROUP at a time; the grouping
    changes no bit."""
    lib = _lib.load()
    f = _jacobian_front("tud_jvp", lib.rtx_tud_jvp, lib.rtx_tud_jvp_dod, OD, OD_plus, OD_minus, fd_step_T, K, tau, grid, T, Z,
                        Altitudes, theta_r, N_angle, returnOD, layers, dOD_dT)
    layers, nA, n, n_wrt = f.layers, f.n_alt, grid.n, f.n_wrt
    nL = int(OD.shape[0])
    rows = tuple(rows)
    if not rows or any(r not in JVP_ROWS for r in rows) or len(set(rows)) != len(rows):
        raise ValueError("tud_jvp: rows %r, expected distinct names among %r" % (rows, JVP_ROWS))
    if layers.size == 0 or layers.min() < 0 or layers.max() >= nL:
        raise ValueError("tud_jvp: layers: indices must lie in [0, %d)" % nL)
    V = np.asarray(V.detach().cpu().numpy() if torch.is_tensor(V) else V, dtype=np.float64)
    if V.ndim == 2:
        V = V[None]
    if V.ndim != 3 or V.shape[0] < 1 or V.shape[1:] != (n_wrt, layers.size):
        raise ValueError("tud_jvp: V has shape %r, expected [n_vec][%d][%d] (the vector axis may be left out)"
                         % (tuple(V.shape), n_wrt, layers.size))
    if not np.isfinite(V).all():
        raise ValueError("tud_jvp: V has non-finite entries")
    n_vec = V.shape[0]
    dense = np.zeros((n_vec, n_wrt, nL))
    for k, l in enumerate(layers):  # one at a time: a repeated index adds in the order given
        dense[:, :, l] += V[:, :, k]
    dev = OD.device
    out = {}
    if "tau" in rows:
        out["tau"] = torch.empty((n_vec, nA, n), dtype=torch.float32, device=dev)
    if "La" in rows:
        out["La"] = torch.empty((n_vec, nA, n), dtype=torch.float32, device=dev)
    if "Ld" in rows:
        out["Ld"] = torch.empty((n_vec, n), dtype=torch.float32, device=dev)
    group = int(JVP_VEC_GROUP or lib.rtx_tud_jvp_max_vectors())
    st = _stream_ptr()
    for v0 in range(0, n_vec, group):
        v1 = min(v0 + group, n_vec)
        part = lambda name: _ptr(out[name][v0:v1]) if name in out else None
        Vg = np.ascontiguousarray(dense[v0:v1])
        _lib.check(f.entry(*f.lead, t_pos, Vg.ctypes.data_as(C.c_void_p), v1 - v0, part("tau"), part("La"), part("Ld"), n, st))
    return out


def tud_jvp(lines, grid, Z, T, P_pa, PL_km, MF_VAL, MF_ID, V, Altitudes=(500,), theta_r=0.0, N_angle=30, returnOD=False,
            wrt=("T",), layers=None, fd_step_T=0.5, mark=None, rows=JVP_ROWS, dT_method="fd", continuum=None,
            xs_lut=None):
    """compute_TUD's outputs and their change along tangent directions in (layer temperatures, mixing ratios):
    tud_jacobian's stages (the same base state, T -+ fd_step_T line-sums and species line-sums) followed by rtx_tud_jvp
    instead of rtx_tud_jacobian. wrt, layers, fd_step_T, dT_method as tud_jacobian; V [n_vec][n_wrt][len(layers)] and rows as
    tud_jvp_from_od, V's wrt axis following `wrt`. Returns (tau, Lu, Ld, OD, d) with d as tud_jvp_from_od returns it.
    mark(name): after each stage ("base", "T", "species", "jvp"). continuum, xs_lut: as tud_jacobian."""
    check_dT_method(dT_method)
    s = _jacobian_stages("tud_jvp", lines, grid, Z, T, P_pa, PL_km, MF_VAL, MF_ID, Altitudes, theta_r, N_angle, returnOD, wrt,
                         layers, fd_step_T, mark, dT_method, continuum, xs_lut)
    d = tud_jvp_from_od(s.OD, s.OD_plus, s.OD_minus, fd_step_T, s.K, s.tau, grid, s.T, s.Z, V, Altitudes=Altitudes,
                        theta_r=theta_r, N_angle=N_angle, returnOD=returnOD, layers=s.layers, t_pos=s.t_pos, rows=rows,
                        dOD_dT=s.dOD_dT)
    if mark:
        mark("jvp")
    return s.tau, s.Lu, s.Ld, s.OD, d
