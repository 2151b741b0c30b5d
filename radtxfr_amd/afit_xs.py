"""AFIT_XS cross-section files: the binary format written by the reference's cross-section generator
(misc/RT_gen_AbsXS_files.py:45-83) and a batched generator for its temperature x pressure loop (:86-92).

File layout (little endian), as the reference's `AFIT_XS_write` produces it (its comments quote other sizes):
    2 bytes   b"v1"
    48 bytes  six float64: X.min(), X.max(), X.size, molecule ID, T [K], P [Pa]
    128 bytes database description, NUL padded
    8*n bytes the cross section as float64
Default file name: XS-{ID:02d}-{T:04d}K-{P:06d}Pa.bin (:73).

The reference computes one (T, p) state per hapi call; here all states of the grid go through ONE prologue + line-sum
launch as "layers" (rtx_line_prep + rtx_voigt_sum), 128 states at a time.

XsLut is the consumer the reference lacks: the files (or cross_section_grid's arrays) as one device-resident table from
which rt.compute_OD / compute_TUD / compute_TUD_batch(xs_lut=...) look optical depths up per layer instead of summing
lines, and through which the derivative functions differentiate when asked (layer_terms_d,
XsLut.dod_host)."""
import ctypes as C
import os
import struct

import numpy as np
import torch

from . import _hostio, _lib, engine
from . import hapi as _hapi

def _touch_pages(a):
    """Write one element per 4 KiB page of a fresh float64 slice (the values are overwritten by the copy that follows)."""
    a[::512] = 0.0
    a[-1:] = 0.0


_STAGE = {}  # one reusable pinned staging block for cross_section_grid (grow-only)
_HEADER = struct.Struct("<2s6d128s")


def AFIT_XS_write(X, Y, T, P, ID, fnDB, File=[]):
    """Save a cross section in the AFIT_XS format; same arguments and return value as RT_gen_AbsXS_files.py:45-83."""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y)
    if len(File) == 0:
        File = "XS-{0:02d}-{1:04d}K-{2:06d}Pa.bin".format(int(ID), int(T), int(P))
    db = str(fnDB).encode()[:128]
    with open(File, "wb") as f:
        f.write(_HEADER.pack(b"v1", float(X.min()), float(X.max()), float(X.size), float(ID), float(T), float(P), db))
        f.write(Y.astype("<f8").tobytes())
    return File


def AFIT_XS_read(File):
    """Inverse of AFIT_XS_write: dict(version, Xmin, Xmax, n, ID, T, P, db, X, Y)."""
    with open(File, "rb") as f:
        raw = f.read()
    ver, xmin, xmax, n, mid, T, P, db = _HEADER.unpack_from(raw, 0)
    n = int(n)
    Y = np.frombuffer(raw, dtype="<f8", count=n, offset=_HEADER.size).copy()
    return {"version": ver.decode(), "Xmin": xmin, "Xmax": xmax, "n": n, "ID": int(mid), "T": T, "P": P,
            "db": db.rstrip(b"\0").decode(), "X": np.linspace(xmin, xmax, n), "Y": Y}


def cross_section_grid(SourceTables, T, P_atm, X, WavenumberWingHW=50.0, WavenumberWing=0.0, IntensityThreshold=0.0,
                       GammaL="gamma_air", Components=None, Diluent=None):
    """HITRAN-unit Voigt cross sections [cm^2/molecule] of one table for every (T, p) pair of the grids: the body of the
    reference's double loop (RT_gen_AbsXS_files.py:88-90: absorptionCoefficient_SDVoigt, i.e. the Voigt line-sum for tables
    without speed-dependence columns and rtx_sdvoigt_sum for tables with them) as one batched launch per 128 states. X must be uniform. Returns xs[nT][nP][nX] float64 (host).
    Diluent: {broadener: fraction} as absorptionCoefficient_SDVoigt takes it (any keys, misc/hapi.py:10860-10890); None keeps
    GammaL (gamma_air: air, gamma_self: self)."""
    T = np.atleast_1d(np.asarray(T, dtype=np.float64))
    P = np.atleast_1d(np.asarray(P_atm, dtype=np.float64))
    X = np.asarray(X, dtype=np.float64)
    engine.require_gpu()
    names = _hapi.listOfTuples(SourceTables)
    tbl = _hapi._device_table(names, [k.lower() for k in Diluent] if Diluent else ())
    grid = engine.Grid.from_axis(X)
    comps = [p for p in tbl.species if p != (0, 0)] if Components is None else [(int(c[0]), int(c[1])) + tuple(c[2:3]) for c in Components]
    w = np.zeros(len(tbl.species))
    for s, mi in enumerate(tbl.species):
        for c in comps:
            if (c[0], c[1]) == mi:
                nat = _hapi.abundance(*mi)
                w[s] = (c[2] if len(c) >= 3 else nat) / nat
    states = [(t, p) for t in T for p in P]
    smax = float(np.max(tbl.cols["sw"])) * float(np.max(w)) if tbl.n and np.max(w) > 0 else 1.0
    scale = 2.0 ** (-np.floor(np.log2(smax))) if smax > 0 and np.isfinite(smax) else 1.0
    dil = {"air": 1.0} if GammaL.lower() == "gamma_air" else {"self": 1.0}
    mix = {k: float(v) for k, v in Diluent.items()} if Diluent else None
    has_sd = tbl.has_sd or (mix is not None and tbl.extra_has_sd(mix))
    out = np.empty((len(states), X.size))
    # states per launch: the per-(line, state) records (80-128 B each) and, with the caller's 350-half-width wings, the
    # partial tiles of the line-sum's part list (every tile then has > 256 candidate lines) must fit comfortably
    per = max(1, min(128, int(2.0e9 / (128.0 * max(tbl.n, 1)))))
    s0 = 0
    while s0 < len(states):
        chunk = states[s0:s0 + per]
        Tk = np.array([c[0] for c in chunk])
        pk = np.array([c[1] for c in chunk])
        if tbl.n:
            dev = torch.empty((len(chunk), grid.n), dtype=torch.float64, device=engine.device())
            try:
                engine.voigt_sum(tbl, grid, Tk, pk, np.tile(w[:, None], (1, len(chunk))), out_f64=dev, dil_air=dil.get("air", 0.0),
                                 dil_self=dil.get("self", 0.0), omega_wing=WavenumberWing, omega_wing_hw=WavenumberWingHW,
                                 intensity_threshold=IntensityThreshold, scale=scale, profile=3 if has_sd else 0, diluent=mix)
            except _lib.RtxError as e:
                if "work list" in str(e) and per > 1:  # too many partial tiles for one launch: fewer states at a time
                    per = max(1, per // 4)
                    continue
                raise
            # while the kernels run: the host thread pool touches one word per page of this chunk's rows of `out` -- fresh
            # memory whose page faults (8-90 ms for 86 MB, box and moment dependent) would otherwise sit behind the copy
            rows = out[s0:s0 + len(chunk)]
            touch = [_hostio._threads().submit(_touch_pages, rows[r, c0:c0 + _hostio._CHUNK])
                     for r in range(len(chunk)) for c0 in range(0, grid.n, _hostio._CHUNK)]
            # device -> one reusable pinned block (a pageable hipMemcpy runs at a few GB/s) -> the result rows, copied by
            # the host thread pool
            need = len(chunk) * grid.n
            pinned = _STAGE.get("buf")
            if pinned is None or pinned.numel() < need:  # kept between calls: page-locking a block of this size costs ~70 ms
                pinned = _STAGE["buf"] = torch.empty((need,), dtype=torch.float64, pin_memory=True)
            pinned = pinned[:need].view(len(chunk), grid.n)
            pinned[:len(chunk)].copy_(dev, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            src = pinned.numpy()
            for f in touch:
                f.result()
            futs = [_hostio._threads().submit(np.copyto, out[s0 + r, c0:c0 + _hostio._CHUNK], src[r, c0:c0 + _hostio._CHUNK])
                    for r in range(len(chunk)) for c0 in range(0, grid.n, _hostio._CHUNK)]
            for f in futs:
                f.result()
        else:
            out[s0:s0 + len(chunk)] = 0.0
        s0 += len(chunk)
    return out.reshape(T.size, P.size, X.size)


def generate_xs_files(SourceTables, ID, T, P_atm, X, descr, WavenumberWingHW=50.0, directory=".", Diluent=None):
    """The reference's generator loop (RT_gen_AbsXS_files.py:86-92) for one molecule table: one AFIT_XS file per (T, p);
    returns the file names in the reference's order (T outer, p inner). P is written in Pa (101325*p, :91). Diluent: as for
    cross_section_grid (None: air)."""
    import os

    T = np.atleast_1d(np.asarray(T, dtype=np.float64))
    P = np.atleast_1d(np.asarray(P_atm, dtype=np.float64))
    xs = cross_section_grid(SourceTables, T, P, X, WavenumberWingHW=WavenumberWingHW, Diluent=Diluent)
    names = []
    for it, t in enumerate(T):
        for ip, p in enumerate(P):
            fn = "XS-{0:02d}-{1:04d}K-{2:06d}Pa.bin".format(int(ID), int(t), int(101325 * p))
            names.append(AFIT_XS_write(X, xs[it, ip], t, 101325 * p, ID, descr, File=os.path.join(directory, fn)))
    return names


# ---- the table as a look-up: XsLut ---------------------------------------------------------
def group_xs_files(paths):
    """from_files' parsing step, host only: AFIT_XS files -> from_grids entries, one per molecule in ascending ID, T and
    P_atm (header Pa / 101325) ascending, xs[iT][iP] the file of that node. ValueError: a file whose n does not match its
    length, files on different axes, a molecule whose files do not form a full T x P rectangle."""
    by_id, axis = {}, None
    for fn in paths:
        with open(fn, "rb") as f:
            head = f.read(_HEADER.size)
        if len(head) < _HEADER.size or head[:2] != b"v1":
            raise ValueError("%s is not an AFIT_XS v1 file" % fn)
        n = _HEADER.unpack(head)[3]
        if n != int(n) or n < 2 or os.path.getsize(fn) != _HEADER.size + 8 * int(n):
            raise ValueError("%s: the header says n = %r points, the file holds %g" % (fn, n, (os.path.getsize(fn) - _HEADER.size) / 8.0))
        d = AFIT_XS_read(fn)
        ax = (d["Xmin"], d["Xmax"], d["n"])
        if axis is None:
            axis = (ax, fn)
        elif ax != axis[0]:
            raise ValueError("AFIT_XS files on different axes: %s has (Xmin, Xmax, n) = %r, %s has %r" % (axis[1], axis[0], fn, ax))
        by_id.setdefault(d["ID"], []).append((float(d["T"]), float(d["P"]) / 101325.0, d["Y"], fn))
    entries = []
    for mid in sorted(by_id):
        files = by_id[mid]
        Ts = sorted({f[0] for f in files})
        Ps = sorted({f[1] for f in files})
        cells = {(f[0], f[1]): f for f in files}
        if len(files) != len(Ts) * len(Ps) or len(cells) != len(files):
            missing = [(t, p) for t in Ts for p in Ps if (t, p) not in cells]
            raise ValueError("molecule %d: %d files do not form a full T x P rectangle of %d x %d nodes (missing (T [K], p [atm]): %r)"
                             % (mid, len(files), len(Ts), len(Ps), missing[:4]))
        xs = np.stack([np.stack([cells[(t, p)][2] for p in Ps]) for t in Ts])
        entries.append({"ID": mid, "T": np.array(Ts), "P_atm": np.array(Ps), "X": np.linspace(*axis[0][:2], axis[0][2]), "xs": xs})
    if not entries:
        raise ValueError("XsLut.from_files: no files")
    return entries


def check_xs_entries(entries):
    """Validate from_grids entries (host only): [(ID, T[nT], P_atm[nP], xs[nT][nP][nX])] and the common engine.Grid."""
    out, grid, X0 = [], None, None
    for e in entries:
        mid = int(e["ID"])
        T = np.atleast_1d(np.asarray(e["T"], dtype=np.float64))
        P = np.atleast_1d(np.asarray(e["P_atm"], dtype=np.float64))
        X = np.asarray(e["X"], dtype=np.float64).ravel()
        xs = np.asarray(e["xs"], dtype=np.float64)
        if T.ndim != 1 or T.size < 1 or np.any(np.diff(T) <= 0) or not np.all(np.isfinite(T)):
            raise ValueError("XsLut: molecule %d: T must be strictly ascending, got %r" % (mid, T))
        if P.ndim != 1 or P.size < 1 or np.any(np.diff(P) <= 0) or not np.all(np.isfinite(P)) or P[0] <= 0:
            raise ValueError("XsLut: molecule %d: P_atm must be strictly ascending and > 0, got %r" % (mid, P))
        if grid is None:
            try:
                grid, X0 = engine.Grid.from_axis(X), X
            except NotImplementedError as err:
                raise ValueError("XsLut: X must be a uniform ascending axis (%s)" % err)
        elif X.size != X0.size or np.max(np.abs(X - X0)) > 1e-9 * grid.step:
            raise ValueError("XsLut: molecule %d is on another axis (%d points from %.9g to %.9g) than molecule %d (%d points from "
                             "%.9g to %.9g)" % (mid, X.size, X[0], X[-1], out[0][0], X0.size, X0[0], X0[-1]))
        if xs.shape != (T.size, P.size, X.size):
            raise ValueError("XsLut: molecule %d: xs has shape %r, expected [nT][nP][nX] = %r" % (mid, xs.shape, (T.size, P.size, X.size)))
        if not np.all(np.isfinite(xs)) or xs.min() < 0:
            raise ValueError("XsLut: molecule %d: cross sections must be finite and >= 0" % mid)
        if any(mid == o[0] for o in out):
            raise ValueError("XsLut: molecule %d is given twice" % mid)
        out.append((mid, T, P, xs))
    if not out:
        raise ValueError("XsLut: no entries")
    return out, grid


def bracket(nodes, v, log=False):
    """The interpolation rule on one axis, host float64: (i, f) with nodes[i] <= v <= nodes[i+1] and f the fraction of the
    way from node i to node i + 1, linear in v (log=False: T) or in ln v (log=True: p). v on a node gives f exactly 0 (1 on
    the last node). An axis with one node is not interpolated: (0, 0) for every v. No range check here."""
    nodes = np.asarray(nodes, dtype=np.float64)
    v = np.atleast_1d(np.asarray(v, dtype=np.float64))
    if nodes.size == 1:
        return np.zeros(v.size, dtype=np.int64), np.zeros(v.size)
    i = np.clip(np.searchsorted(nodes, v, side="right") - 1, 0, nodes.size - 2)
    a, b = nodes[i], nodes[i + 1]
    if log:
        a, b, v = np.log(a), np.log(b), np.log(v)
    return i, (v - a) / (b - a)


def layer_terms(tables, T, P_atm, PL_km, MF_VAL, MF_ID):
    """Node rows and weights of every (layer, molecule), host float64.
    tables: [(ID, T_nodes, P_nodes, row0)] in table order, row0 the table row of node (0, 0) (rows iT * nP + iP follow).
    Returns rows int32 [L][M][4] and w float64 [L][M][4] for the corners (iT, iP), (iT, iP+1), (iT+1, iP), (iT+1, iP+1):
        w = N * [(1-fT)(1-fP), (1-fT) fP, fT (1-fP), fT fP],   N = MF_VAL * 1e-6 * volumeConcentration(p, T) * PL * 1e5
    with (iT, fT) linear in T and (iP, fP) linear in ln p (bracket). A molecule of the table that MF_ID lacks, or whose
    MF_VAL is 0 in a layer, has weight 0 there (and is not range-checked). ValueError: a molecule of MF_ID the table lacks; a
    layer outside the node range of a molecule it uses (no extrapolation, no clamping)."""
    T = np.atleast_1d(np.asarray(T, dtype=np.float64))
    p = np.atleast_1d(np.asarray(P_atm, dtype=np.float64))
    PL = np.atleast_1d(np.asarray(PL_km, dtype=np.float64))
    nL = T.size
    MF = np.asarray(MF_VAL, dtype=np.float64).reshape(nL, -1)
    ids = [int(v) for v in np.asarray(MF_ID).ravel()]
    have = [t[0] for t in tables]
    lacking = [m for m in ids if m not in have]
    if lacking:
        raise ValueError("xs_lut: MF_ID names molecule(s) %r, the table holds %r" % (lacking, have))
    nvol = engine.volumeConcentration(p, T)
    rows = np.zeros((nL, len(tables), 4), dtype=np.int32)
    w = np.zeros((nL, len(tables), 4))
    for m, (mid, Tn, Pn, row0) in enumerate(tables):
        rows[:, m, :] = row0
        if mid not in ids:
            continue
        N = nvol * (MF[:, ids.index(mid)] * 1e-6) * PL * 1e5  # layer_weights_od's operations, in its order
        for name, unit, nodes, v in (("T", "K", Tn, T), ("p", "atm", Pn, p)):
            bad = (N != 0) & ((v < nodes[0]) | (v > nodes[-1])) if nodes.size > 1 else np.zeros(nL, dtype=bool)
            if bad.any():
                l = int(np.flatnonzero(bad)[0])
                raise ValueError("xs_lut: layer %d (%s = %.9g %s) lies outside molecule %d's table range [%.9g, %.9g] %s; there is "
                                 "no extrapolation" % (l, name, v[l], unit, mid, nodes[0], nodes[-1], unit))
        iT, fT = bracket(Tn, T)
        iP, fP = bracket(Pn, p, log=True)
        iT1, iP1 = np.minimum(iT + 1, Tn.size - 1), np.minimum(iP + 1, Pn.size - 1)
        rows[:, m, :] = row0 + np.stack([iT * Pn.size + iP, iT * Pn.size + iP1, iT1 * Pn.size + iP, iT1 * Pn.size + iP1], axis=1)
        w[:, m, :] = N[:, None] * np.stack([(1 - fT) * (1 - fP), (1 - fT) * fP, fT * (1 - fP), fT * fP], axis=1)
    return rows, w


def layer_terms_d(tables, T, P_atm, PL_km, MF_VAL, MF_ID, species):
    """layer_terms' derivative weights at fixed p, host float64. tables, T, P_atm, PL_km, MF_VAL,
    MF_ID as layer_terms; species: distinct molecule ids of MF_ID whose mixing-ratio derivative is wanted. Returns
        rows  int32   [L][M][4]   what layer_terms returns
        w_T   float64 [L][M][4]   dOD_l/dT_l = sum_m sum_c w_T[l][m][c] xs_m[corner c]:  N (-w_c / T + dw_c/dT), with w_c the
                                  bilinear factor of layer_terms, N ~ 1/T the column amount and
                                  dw/dT = [-(1-fP), -fP, (1-fP), fP] / (T_{i+1} - T_i), all 0 on an axis with one T node
        w_K   float64 [S][L][4]   dOD_l/dMF_s,l per ppmv = sum_c w_K[s][l][c] xs_s[corner c]: N(MF = 1) w_c, formed by
                                  layer_terms' own operations in its order (the weights it gives that molecule alone at
                                  1 ppmv, bit for bit); exact and finite at MF = 0, OD being linear in MF
        idx   list [S]            the table index of each species' molecule.
    OD is piecewise linear-over-T in T, so dOD/dT jumps at a T node: A LAYER EXACTLY ON A NODE TAKES THE SLOPE OF THE CELL
    bracket() RETURNS FOR IT, the cell to its right, except on the last node, where it is the cell to its left -- the cell
    whose weights the forward run used. ValueError: what layer_terms raises; a species named twice or not in MF_ID; and a
    species is range-checked in EVERY layer, also where its MF_VAL is 0 (its derivative is not 0 there), with the forward's
    text."""
    T = np.atleast_1d(np.asarray(T, dtype=np.float64))
    p = np.atleast_1d(np.asarray(P_atm, dtype=np.float64))
    PL = np.atleast_1d(np.asarray(PL_km, dtype=np.float64))
    nL = T.size
    MF = np.asarray(MF_VAL, dtype=np.float64).reshape(nL, -1)
    ids = [int(v) for v in np.asarray(MF_ID).ravel()]
    species = [int(s) for s in species]
    rows, _ = layer_terms(tables, T, p, PL, MF, ids)  # the forward's rows and its checks
    if len(set(species)) != len(species) or any(s not in ids for s in species):
        raise ValueError("xs_lut: species %r must be distinct molecule ids of MF_ID %r" % (species, ids))
    nvol = engine.volumeConcentration(p, T)
    w_T = np.zeros((nL, len(tables), 4))
    w_K = np.zeros((len(species), nL, 4))
    idx = [0] * len(species)
    for m, (mid, Tn, Pn, row0) in enumerate(tables):
        if mid not in ids:
            continue
        if mid in species:
            for name, unit, nodes, v in (("T", "K", Tn, T), ("p", "atm", Pn, p)):
                bad = (v < nodes[0]) | (v > nodes[-1]) if nodes.size > 1 else np.zeros(nL, dtype=bool)
                if bad.any():
                    l = int(np.flatnonzero(bad)[0])
                    raise ValueError("xs_lut: layer %d (%s = %.9g %s) lies outside molecule %d's table range [%.9g, %.9g] %s; there is "
                                     "no extrapolation" % (l, name, v[l], unit, mid, nodes[0], nodes[-1], unit))
        N = nvol * (MF[:, ids.index(mid)] * 1e-6) * PL * 1e5
        iT, fT = bracket(Tn, T)
        iP, fP = bracket(Pn, p, log=True)
        corners = np.stack([(1 - fT) * (1 - fP), (1 - fT) * fP, fT * (1 - fP), fT * fP], axis=1)
        slope = np.zeros((nL, 4))
        if Tn.size > 1:
            slope = np.stack([-(1 - fP), -fP, (1 - fP), fP], axis=1) / (Tn[iT + 1] - Tn[iT])[:, None]
        w_T[:, m, :] = N[:, None] * (-corners / T[:, None] + slope)
        if mid in species:
            s = species.index(mid)
            idx[s] = m
            N1 = nvol * (np.ones(nL) * 1e-6) * PL * 1e5  # layer_terms' N at 1 ppmv
            w_K[s] = N1[:, None] * corners
    return rows, w_T, w_K, idx


def dod_from_terms(xs_rows, rows, w_T, w_K, idx):
    """The derivative columns of layer_terms_d's terms on table rows xs_rows [n_rows][nX], float64 on the host:
    (dOD_dT [L][nX], dOD_dMF [S][L][nX])."""
    xs_rows = np.asarray(xs_rows, dtype=np.float64)
    nL = rows.shape[0]
    dT = np.zeros((nL, xs_rows.shape[1]))
    dK = np.zeros((w_K.shape[0], nL, xs_rows.shape[1]))
    for l in range(nL):
        for m in range(rows.shape[1]):
            for c in range(4):
                if w_T[l, m, c] != 0.0:
                    dT[l] += w_T[l, m, c] * xs_rows[rows[l, m, c]]
        for s, m in enumerate(idx):
            for c in range(4):
                if w_K[s, l, c] != 0.0:
                    dK[s, l] += w_K[s, l, c] * xs_rows[rows[l, m, c]]
    return dT, dK


def align_axis(table_grid, grid):
    """Index of grid's first point (of the whole axis, shard offset not counted) on table_grid when `grid` coincides with a
    contiguous run of it -- same spacing, every point within 1e-9 of a step of a table point -- else ValueError naming both
    axes. There is no spectral interpolation."""
    tg, n = table_grid, grid.n_total
    k = int(round((grid.xmin - tg.xmin) / tg.step))
    ok = 0 <= k and k + n <= tg.n_total
    if ok:  # both ends within the bound: the points between are linear in the index on both axes
        tol = 1e-9 * tg.step + 4 * np.spacing(max(abs(tg.xmin), abs(tg.xmax)))  # plus the rounding of the axis values themselves
        ok = abs(grid.xmin - tg.x_at(k - tg.offset)) <= tol and abs(grid.xmax - tg.x_at(k + n - 1 - tg.offset)) <= tol
    if not ok:
        raise ValueError("xs_lut: the requested axis (%d points from %.9g to %.9g, step %.9g) is not a contiguous run of the table's "
                         "axis (%d points from %.9g to %.9g, step %.9g); there is no spectral interpolation"
                         % (n, grid.xmin, grid.xmax, grid.step, tg.n_total, tg.xmin, tg.xmax, tg.step))
    return k


_UPLOAD = {}  # one reusable pinned staging block for XsLut uploads (grow-only, like _STAGE for the way out)
_UPLOAD_BYTES = 64 << 20


class XsLut:
    """Cross-section tables of several molecules, resident on the current device as fp32 rows [molecule][iT][iP][x] (x
    fastest) behind an rtx_xs_lut handle (include/radtxfr_hip.h). Each molecule's rows are multiplied by its own power of
    two, 2**exponent(ID), so that its largest value lands in [1, 2) (1e-19 ... 1e-30 cm^2 is not fp32 material; the line
    strengths use the same device); the weights of a look-up carry 2**-exponent.

        lut = XsLut.from_grids([dict(ID=1, T=T, P_atm=P, X=X, xs=cross_section_grid(tbl, T, P, X, Components=...)), ...])
        lut = XsLut.from_files(generate_xs_files(...) + ...)
        rt.compute_TUD(Xmin, Xmax, xs_lut=lut, ...)

    Public: molecules (IDs in table order), grid (engine.Grid of the axis), nodes(ID) -> (T, P_atm), exponent(ID),
    rows(ID) (the device rows read back, float32 [nT][nP][nX]), nbytes, device; free() or del releases the device memory.
    Interpolation rule and summation order: layer_terms, DESIGN.md section 4.11. Derivatives with respect to layer
    temperature and mixing ratios (layer_terms_d, dod_host; xs_derivatives=True of the derivative functions of
    radiative_transfer): DESIGN.md section 4.24."""

    def __init__(self, entries):
        tabs, self.grid = check_xs_entries(entries)
        engine.require_gpu()
        self._lib = _lib.load()
        self.device = engine.device()
        self.molecules = tuple(t[0] for t in tabs)
        self._tables, self._exp, row0 = [], {}, 0
        for mid, T, P, xs in tabs:
            self._tables.append((mid, T, P, row0))
            mx = float(xs.max())
            self._exp[mid] = 1 - int(np.frexp(mx)[1]) if mx > 0 else 0  # mx * 2**e in [1, 2)
            row0 += T.size * P.size
        self.n_rows = row0
        self._scale = np.array([2.0 ** -self._exp[m] for m in self.molecules])  # folded into the fp32 weights
        h = C.c_void_p()
        _lib.check(self._lib.rtx_xs_lut_create(len(tabs), self.n_rows, self.grid.n_total, C.byref(h)))
        self._h = h
        nx = self.grid.n_total
        per = max(1, min(self.n_rows, _UPLOAD_BYTES // (4 * nx)))
        pinned = _UPLOAD.get("buf")
        if pinned is None or pinned.numel() < per * nx:
            pinned = _UPLOAD["buf"] = torch.empty((per * nx,), dtype=torch.float32, pin_memory=True)
        stage = pinned[:per * nx].view(per, nx).numpy()
        st = torch.cuda.current_stream()
        for (mid, T, P, r0), (_, _, _, xs) in zip(self._tables, tabs):
            flat = xs.reshape(-1, nx)
            for a in range(0, flat.shape[0], per):
                k = min(per, flat.shape[0] - a)
                np.ldexp(flat[a:a + k], self._exp[mid], out=stage[:k], casting="same_kind")  # exact scaling, one rounding to fp32
                _lib.check(self._lib.rtx_xs_lut_set_rows(self._h, r0 + a, k, stage.ctypes.data_as(C.c_void_p), C.c_void_p(st.cuda_stream)))
                st.synchronize()  # the block is refilled next

    @classmethod
    def from_grids(cls, entries):
        """entries: one dict per molecule with ID, T[nT] (K, strictly ascending), P_atm[nP] (strictly ascending, > 0), X[nX]
        (uniform, the same for all) and xs[nT][nP][nX] float64 cm^2/molecule (finite, >= 0): what cross_section_grid
        returns. nT == 1 or nP == 1 is allowed; that axis is then not interpolated (any layer value is accepted on it)."""
        return cls(list(entries))

    @classmethod
    def from_files(cls, paths):
        """The same table from AFIT_XS files (group_xs_files: grouped by ID, T and P from the headers)."""
        return cls(group_xs_files(list(paths)))

    def _table(self, ID):
        for t in self._tables:
            if t[0] == int(ID):
                return t
        raise KeyError("XsLut holds molecules %r, not %r" % (self.molecules, ID))

    def nodes(self, ID):
        _, T, P, _ = self._table(ID)
        return T.copy(), P.copy()

    def exponent(self, ID):
        return self._exp[self._table(ID)[0]]

    @property
    def nbytes(self):
        return int(self._lib.rtx_xs_lut_bytes(self._handle()))

    def _handle(self):
        if self._h is None:
            raise ValueError("this XsLut has been freed")
        return self._h

    def rows(self, ID):
        mid, T, P, r0 = self._table(ID)
        out = np.empty((T.size * P.size, self.grid.n_total), dtype=np.float32)
        _lib.check(self._lib.rtx_xs_lut_get_rows(self._handle(), r0, out.shape[0], out.ctypes.data_as(C.c_void_p),
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return out.reshape(T.size, P.size, -1)

    def align(self, grid):
        return align_axis(self.grid, grid)

    def layer_terms(self, T, P_atm, PL_km, MF_VAL, MF_ID):
        """rtx_xs_od's host inputs for one atmosphere: rows int32 [L][M][4], weights float32 [L][M][4] (layer_terms' float64
        weights times the molecule's 2**-exponent, rounded once)."""
        rows, w = layer_terms(self._tables, T, P_atm, PL_km, MF_VAL, MF_ID)
        return np.ascontiguousarray(rows), np.ascontiguousarray((w * self._scale[None, :, None]).astype(np.float32))

    def layer_terms_d(self, T, P_atm, PL_km, MF_VAL, MF_ID, species):
        """rtx_xs_od_d's host inputs for one atmosphere: rows int32 [L][M][4], w_T float32 [L][M][4],
        w_K float32 [S][L][4] (the module's layer_terms_d float64 weights times the molecule's 2**-exponent, rounded once) and
        the table index of each species, int32 [S]. A layer exactly on a T node takes the slope of the cell bracket() returns
        for it: the cell to its right, the cell to its left on the last node -- the cell the forward run used."""
        rows, w_T, w_K, idx = layer_terms_d(self._tables, T, P_atm, PL_km, MF_VAL, MF_ID, species)
        sK = self._scale[np.asarray(idx, dtype=np.int64)] if len(idx) else np.zeros(0)
        return (np.ascontiguousarray(rows), np.ascontiguousarray((w_T * self._scale[None, :, None]).astype(np.float32)),
                np.ascontiguousarray((w_K * sK[:, None, None]).astype(np.float32)), np.asarray(idx, dtype=np.int32))

    def dod_host(self, T, P_atm, PL_km, MF_VAL, MF_ID, species=None):
        """The definition of the table's derivatives, float64 on the host (the oracle of the device tests): (dOD_dT [nL][nX]
        per K, {molecule: dOD_dMF [nL][nX] per ppmv}) on the table's whole axis, from the module's layer_terms_d weights in
        float64 and the float32 rows as stored (rows(ID)) times 2**-exponent. species: the molecules differentiated, default
        every id of MF_ID once. A layer exactly on a T node takes the slope of the cell bracket() returns for it (the cell to
        its right; to its left on the last node)."""
        if species is None:
            species = list(dict.fromkeys(int(v) for v in np.asarray(MF_ID).ravel()))
        species = [int(s) for s in species]
        rows, w_T, w_K, idx = layer_terms_d(self._tables, T, P_atm, PL_km, MF_VAL, MF_ID, species)
        xs_rows = np.concatenate([np.ldexp(self.rows(m).astype(np.float64), -self._exp[m]).reshape(-1, self.grid.n_total)
                                  for m in self.molecules])
        dT, dK = dod_from_terms(xs_rows, rows, w_T, w_K, idx)
        return dT, {m: dK[s] for s, m in enumerate(species)}

    def free(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            self._lib.rtx_xs_lut_free(h)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
