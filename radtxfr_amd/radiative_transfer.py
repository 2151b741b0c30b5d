"""Drop-in for the hot-path functions of the reference's radiative_transfer.py.

Same names, positional order, keyword names and return shapes (spectral axis first) as the
reference (radiative_transfer.py:22-25, signatures listed in SURVEY.md section 8b):

    planckian                         :792-848
    make_spectral_axis                :251-271
    compute_OD                        :395-456    (LBLRTM replaced, see below)
    compute_TUD                       :274-392
    compute_LWIR_apparent_radiance    :1017-1069
    ILS_MAKO                          :1072-1263
    options, StdAtmos                 :75-183

NumPy in -> NumPy out (float64, like the reference); torch CUDA tensors in -> torch out where the
function is elementwise. All arithmetic runs in libradtxfr_hip.so on the GPU; there is no CPU path.

Conscious divergences from the reference:
  * compute_OD: the reference shells out to the LBLRTM Fortran binary with the AER line file; both
    are git-LFS stubs. Here OD(nu) = sum_m k_m(nu; T, p) x_m PL from the Voigt line-sum over the line
    table named by opts["line_table"] (a table in radtxfr_amd.hapi.LOCAL_TABLE_CACHE, or a column
    dict). The continuum LBLRTM adds is added only from tables the caller supplies (continuum=, radtxfr_amd/continuum.py);
    none is built in. Chunking / TAPE5 / TAPE12 plumbing does not exist.
  * options are copied per call: kwargs no longer leak into the module-level default (quirk 2).
  * make_spectral_axis casts the point count to int (quirk 1: the reference crashes on NumPy>=1.18).
  * spectra are computed in float32 on the device and returned as float64.
"""
import functools
import os
import threading
import time

import numpy as np
import torch

from . import _hostio, engine
from . import hapi as _hapi

# Module constants (radiative_transfer.py:71-72)
c1 = 1.19104295315e-16  # [J m^2 / s]
c2 = 1.43877736830e-02  # [m K]

# 66-layer 1976 US standard atmosphere. The reference embeds a rounded copy (:77-144) of its
# StandardAtmosphere.csv (2 decimals for Z/PL/P/T, %.3E for the mixing ratios); this package ships
# the CSV (input fixture) and applies the same rounding, which reproduces the embedded table exactly
# (tests/test_host.py checks it against a fixture captured from the reference).
_CSV = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "StandardAtmosphere.csv")
StdAtmosCSV = np.loadtxt(_CSV, delimiter=",", skiprows=1)
StdAtmos = StdAtmosCSV.copy()
StdAtmos[:, 1:6] = np.round(StdAtmosCSV[:, 1:6], 2)
StdAtmos[:, 6:] = np.vectorize(lambda v: float("%.3E" % v))(StdAtmosCSV[:, 6:])

options = {
    "DVOUT": 0.0005,  # [cm^{-1}]
    "T": 296.0, "P": 101325.0, "PL": 1.0,
    "MF_ID": np.array([]), "MF_VAL": np.array([]),
    "line_table": None,  # replaces "LBLRTM"/"TAPE3": name in hapi.LOCAL_TABLE_CACHE or column dict
    "copy_axis": False,  # True: compute_TUD returns a fresh writable X (the reference's behaviour) instead of a cached read-only one
    "chunks": None,      # compute_TUD: wavenumber chunks whose device-to-host copies overlap the next chunk's kernels (None: automatic)
    # options for compute_TUD (:172-182)
    "Zs": StdAtmos[:, 1], "Ts": StdAtmos[:, 5], "Ps": StdAtmos[:, 4], "PLs": StdAtmos[:, 3],
    "MFs_VAL": StdAtmos[:, 6:14] * 1e6, "MFs_ID": np.array([1, 2, 3, 4, 5, 6, 7, 22]),
    "theta_r": 0, "N_angle": 30, "Altitudes": np.asarray([500]), "save": False, "returnOD": False,
}


def _is_torch(x):
    return isinstance(x, torch.Tensor)


def _dev_f64(x, dev):
    if _is_torch(x):
        return x.to(device=dev, dtype=torch.float64).contiguous()
    a = np.asarray(x, dtype=np.float64)
    return torch.as_tensor(a if a.flags.writeable else a.copy(), device=dev).contiguous()  # read-only views (broadcast_to)


def _dev_f32(x, dev):
    if _is_torch(x):
        return x.to(device=dev, dtype=torch.float32).contiguous()
    return torch.as_tensor(np.asarray(x, dtype=np.float32), device=dev).contiguous()


def make_spectral_axis(Xmin, Xmax, DVOUT):
    """:251-271. Spacing is (Xmax-Xmin)/(nX-1), not DVOUT, exactly like the reference."""
    nX = int(np.ceil((Xmax - Xmin) / DVOUT))
    return np.linspace(Xmin, Xmax, nX)


def planckian(X_in, T_in, wavelength=False):
    """Planck spectral radiance, :792-848. Output shape (X.size, *T.shape);
    [uW/(cm^2 sr cm^-1)] or, for wavelength input in um, [uW/(cm^2 sr um)]."""
    as_torch = _is_torch(X_in) or _is_torch(T_in)
    dev = engine.device()
    X = _dev_f64(X_in, dev).flatten()
    T = _dev_f64(T_in, dev)
    dimsT = tuple(T.shape)
    if wavelength or float(X.mean()) < 50:
        if not wavelength:
            print("Assumes X given in µm; returning L in µF")
        wavelength = True
    L = engine.planck(X, T.flatten(), wavelength=wavelength).reshape((X.numel(), *dimsT))
    return L if as_torch else L.cpu().numpy()


def _planck_family(fn_name, X_in, V_in, wavelength, bad_value, spectral_dim, notice):
    """Shared body of brightnessTemperature / BT2L: the reference's reshaping rules (:890-907, :925-931)
    around one elementwise fp64 kernel."""
    import ctypes as C
    from . import _lib
    as_torch = _is_torch(X_in) or _is_torch(V_in)
    dev = engine.device()
    X = _dev_f64(X_in, dev).flatten()
    V = _dev_f64(V_in, dev)
    if spectral_dim != 0:
        V = V.swapaxes(0, spectral_dim)
    if V.dim() == 1:
        V = V[:, None]
    dims = tuple(V.shape)
    V2 = V.reshape(dims[0], -1).contiguous()
    if V2.shape[0] != X.numel():
        raise ValueError("operands could not be broadcast together with shapes (%d,1) (%d,%d)" % (X.numel(), *V2.shape))
    if wavelength or float(X.mean()) < 50:
        if not wavelength:
            print(notice)
        wavelength = True
    out = torch.empty_like(V2)
    lib = _lib.load()
    _lib.check(getattr(lib, fn_name)(C.c_void_p(X.data_ptr()), X.numel(), C.c_void_p(V2.data_ptr()), V2.shape[1],
                                     int(bool(wavelength)), float(bad_value), C.c_void_p(out.data_ptr()),
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    out = out.reshape((X.numel(), *dims[1:]))  # a 1-D input comes back (nX, 1), as in the reference
    if spectral_dim != 0:
        out = out.swapaxes(0, spectral_dim)
    return out if as_torch else out.cpu().numpy()


def brightnessTemperature(X_in, L_in, wavelength=False, bad_value=np.nan, spectral_dim=0):
    """Brightness temperature [K] of spectral radiance L, signature of :851-933. X (nX,), L with the
    spectral axis at `spectral_dim`; unphysical radiances (non-finite or <= 0) give `bad_value` (:922-923)."""
    return _planck_family("rtx_brightness_temperature", X_in, L_in, wavelength, bad_value, spectral_dim,
                          "Assumes X given in µm and L given in µF")


def BT2L(X_in, T_in, wavelength=False, bad_value=np.nan, spectral_dim=0):
    """Spectral radiance of a brightness-temperature spectrum, signature of :936-1014."""
    return _planck_family("rtx_bt2l", X_in, T_in, wavelength, bad_value, spectral_dim,
                          "Assumes X given in µm and L given in µF")


def _resolve_table(spec, diluents=()):
    if spec is None:
        raise Exception("compute_OD: set opts['line_table'] to a table in radtxfr_amd.hapi.LOCAL_TABLE_CACHE "
                        "(the reference's LBLRTM binary and AER TAPE3 are git-LFS stubs; there is no built-in line file)")
    if isinstance(spec, engine.LineTable):
        return spec
    if isinstance(spec, str):
        if spec not in _hapi.LOCAL_TABLE_CACHE:
            raise Exception("%s: no such table. Check tableList() for more info." % spec)
        return _hapi._device_table([spec], diluents)
    if isinstance(spec, dict):
        key = "__dict_%d" % id(spec)
        if key not in _hapi.LOCAL_TABLE_CACHE or _hapi.LOCAL_TABLE_CACHE[key].get("_src") is not spec:
            _hapi.LOCAL_TABLE_CACHE[key] = {"header": {"number_of_rows": len(spec["nu"])}, "data": spec, "_src": spec}
        return _hapi._device_table([key], diluents)
    raise TypeError("opts['line_table'] must be a table name, a column dict or an engine.LineTable")


def _xs_lut_option(fn, o):
    """The per-call xs_lut= option (an afit_xs.XsLut, or None): optical depths looked up in a cross-section table instead of
    summed over lines. Never stored in `options`. A table's broadening was fixed when it was made: NotImplementedError
    with any broadening=."""
    lut = o.get("xs_lut")
    if lut is not None and o.get("broadening") is not None:
        raise NotImplementedError("%s: xs_lut with broadening=%r is not supported: a table's broadening was fixed when it was made "
                                  "(afit_xs.cross_section_grid's GammaL / Diluent); use broadening=None" % (fn, o.get("broadening")))
    return lut


def _continuum_option(fn, o, ids):
    """The per-call continuum= option (a continuum.Continuum, or None): tabulated continuum absorption added to the optical
    depths. Never stored in `options`. ValueError, before any device work, for a component whose
    molecule the call's mixing ratios (`ids`) lack: a silent zero would hide a misconfigured call."""
    cont = o.get("continuum")
    if cont is not None:
        have = [int(v) for v in np.asarray(ids).ravel()]
        lacking = [c.molecule for c in cont.components if c.molecule not in have]
        if lacking:
            raise ValueError("%s: continuum component molecule(s) %r are not in the mixing-ratio ids %r" % (fn, lacking, have))
    return cont


def compute_OD(Xmin_in, Xmax_in, opts=options, **kwargs):
    """Monochromatic optical depth of one homogeneous layer, signature of :395-456.
    kwargs honoured: T [K], P [Pa], PL [km], MF_VAL [ppmv], MF_ID (HITRAN ids), DVOUT, line_table, xs_lut, continuum.
    continuum (per call, a continuum.Continuum): its tabulated continuum absorption is added to the optical depth, whichever
    way that was made. ValueError: a component whose molecule MF_ID lacks.
    xs_lut (per call, an afit_xs.XsLut): look the optical depth up in a cross-section table (bilinear in T and ln p between
    its nodes) instead of summing lines; line_table is then neither needed nor touched. ValueError: the axis is
    not a run of the table's, (T, P) outside the table, a molecule of MF_ID the table lacks.
    Returns (X_out, OD_out)."""
    o = dict(opts)
    o.update(kwargs)
    DVOUT = o.get("DVOUT", 0.025)
    X = make_spectral_axis(Xmin_in, Xmax_in, DVOUT)
    lut = _xs_lut_option("compute_OD", o)
    cont = _continuum_option("compute_OD", o, o["MF_ID"])
    grid = engine.Grid(Xmin_in, Xmax_in, X.size)
    MF = np.asarray(o["MF_VAL"], dtype=np.float64)[None, :]
    if lut is not None:
        OD = engine.xs_od(lut, grid, [o["T"]], [o["P"] / 101325.0], [o["PL"]], MF, o["MF_ID"])
    else:
        tbl = _resolve_table(o.get("line_table"))
        OD = engine.optical_depths(tbl, grid, [o["T"]], [o["P"]], [o["PL"]], MF, o["MF_ID"])
    if cont is not None:
        engine.continuum_add(cont, grid, [o["T"]], [o["P"]], [o["PL"]], MF, o["MF_ID"], OD)
    return X, OD[0].double().cpu().numpy()


_AXIS_CACHE = {}


def _cached_axis(Xmin, Xmax, DVOUT):
    """make_spectral_axis with a two-entry cache: np.linspace of the 5.5 M-point C3 axis costs ~12 ms of host time per call,
    more than the whole device computation. The cached array is returned READ-ONLY (every call on the same grid hands out the
    same object); callers that want to modify it copy it."""
    key = (float(Xmin), float(Xmax), float(DVOUT))
    X = _AXIS_CACHE.get(key)
    if X is None:
        X = make_spectral_axis(Xmin, Xmax, DVOUT)
        X.setflags(write=False)
        if len(_AXIS_CACHE) >= 2:
            _AXIS_CACHE.pop(next(iter(_AXIS_CACHE)))
        _AXIS_CACHE[key] = X
    return X


class _Call:
    """One call of the compute_TUD family, parsed: `opts` overlaid with `kwargs` in a copy (quirk 2) as `o`, and what the
    reference derives from it at the top of compute_TUD (:304-314, :346-349) -- the profile Z, T, P, PL, MF as float64
    arrays and ID, the sensor altitudes Z_s, theta (float64), N_angle, returnOD and the broadening= option. What can
    raise or costs time is made on first use, so that a caller's own argument checks come first: lut (the xs_lut option,
    _xs_lut_option in `fn`'s name), continuum (the continuum option, _continuum_option), foreign (broadening's foreign
    gases), X (the cached axis) and grid; table() looks the line table up (None with an xs_lut), and nothing before it
    touches a table or a device."""

    def __init__(self, fn, Xmin, Xmax, opts, kwargs):
        self.fn, self.Xmin, self.Xmax = fn, Xmin, Xmax
        self.o = o = dict(opts)
        o.update(kwargs)
        self.Z, self.T, self.P, self.PL, self.MF = (np.asarray(o[k], dtype=np.float64) for k in ("Zs", "Ts", "Ps", "PLs", "MFs_VAL"))
        self.ID = np.asarray(o["MFs_ID"])
        self.Z_s = np.array([o["Altitudes"]]).ravel()
        self.theta = np.asarray(o["theta_r"], dtype=np.float64)
        self.N_angle, self.returnOD = int(o["N_angle"]), bool(o["returnOD"])
        self.broadening = o.get("broadening")

    lut = functools.cached_property(lambda self: _xs_lut_option(self.fn, self.o))
    continuum = functools.cached_property(lambda self: _continuum_option(self.fn, self.o, self.ID))
    foreign = functools.cached_property(lambda self: engine.broadening_gases(self.broadening))
    X = functools.cached_property(lambda self: _cached_axis(self.Xmin, self.Xmax, self.o["DVOUT"]))
    grid = functools.cached_property(lambda self: engine.Grid(self.Xmin, self.Xmax, self.X.size))

    def table(self):
        return _resolve_table(self.o.get("line_table"), self.foreign or ()) if self.lut is None else None


_STAGING = {}
_TRACE = float(os.environ.get("RADTXFR_TRACE", "0") or 0)  # developer aid: print the phases of slow compute_TUD calls


def _rows_to_host_f64(rows, stream=None):
    """float32 device rows [(k_i, n)] -> float64 NumPy arrays (see _hostio): zero-copy views of a pinned block while the
    pinned bytes lent out stay under _hostio.PINNED_RESULT_CAP, else fresh pageable arrays filled from a reusable pinned
    staging ring by the host thread pool. Returns (arrays, event): the arrays are valid once `event` has completed
    (event.synchronize()); on the pageable path they are complete on return."""
    got = _hostio.rows_to_pinned_f64(rows, stream)
    if got is not None:
        return got
    key = (rows[0].device.index, threading.get_ident())
    st = _STAGING.get(key)
    if st is None:
        st = _STAGING[key] = _hostio.Staging(depth=1)
    ticket = st.stage(rows, stream)
    return st.collect(ticket), ticket[3]


def _tud_shapes(tau2, Lu2, nZ, nMu):
    """The reference's squeeze rules (:357-365) on [nZ*nMu][nX] host rows."""
    tau_ = tau2.reshape(nZ, nMu, -1).transpose(2, 0, 1)
    Lu_ = Lu2.reshape(nZ, nMu, -1).transpose(2, 0, 1)
    if nZ == 1 and nMu == 1:
        return tau_[:, 0, 0], Lu_[:, 0, 0]
    if nZ == 1:
        return np.ascontiguousarray(tau_[:, 0, :]), np.ascontiguousarray(Lu_[:, 0, :])
    if nMu == 1:
        return np.ascontiguousarray(tau_[:, :, 0]), np.ascontiguousarray(Lu_[:, :, 0])
    return np.ascontiguousarray(tau_), np.ascontiguousarray(Lu_)


_SIDE_STREAMS = {}


def _compute_tud_chunked(tbl, grid, Z, T, P, PL, MF, ID, Z_s, theta, nA, returnOD, n_chunks, broadening=None, xs_lut=None,
                         continuum=None):
    """compute_TUD's device work in n_chunks tile-aligned wavenumber chunks, each chunk's widening and device-to-host copy
    (side stream) under the next chunk's kernels: a single call is PCIe-bound (132 MB of float64 at C3 size: 2.7 ms against
    1.9 ms of kernels), and chunks cut on line-sum tile boundaries give the unchunked bits. Returns (tau_h, Lu_h, Ld_h,
    (nZ, nMu)) as float64 NumPy views of one pinned block, or None when no pinned block can be lent (the caller then takes
    the plain path)."""
    from . import _lib, dist as _dist
    n = grid.n
    tile = int(_lib.load().rtx_voigt_tile_points())
    offs = _dist.tile_aligned_bounds(n, n_chunks, tile)
    nL = T.size
    nZ, nMu = Z_s.size, np.atleast_1d(theta).size
    nrow = nZ * nMu
    lent = _hostio.lend_block((2 * nrow + 1, n))
    if lent is None:
        return None
    host, arr = lent
    dev = engine.device()
    tau = torch.empty((nrow, n), dtype=torch.float32, device=dev)
    Lu = torch.empty_like(tau)
    Ld = torch.empty((n,), dtype=torch.float32, device=dev)
    max_len = int(np.diff(offs).max())
    OD = torch.empty((nL, max_len), dtype=torch.float32, device=dev)
    plan = tbl.plan(nL, n) if xs_lut is None else None
    side = _SIDE_STREAMS.get(dev.index)
    if side is None:
        side = _SIDE_STREAMS[dev.index] = torch.cuda.Stream()
    done = None
    for c in range(n_chunks):
        off, ln = int(offs[c]), int(offs[c + 1] - offs[c])
        if ln == 0:
            continue
        sl = slice(off, off + ln)
        run = engine.TudRunner(tbl, grid.shard(grid.offset + off, ln), Z, n_layers=nL, Altitudes=Z_s, theta_r=theta, N_angle=nA,
                               returnOD=returnOD, out=(tau[:, sl], Lu[:, sl], Ld[sl]), OD=OD[:, :ln], plan=plan,
                               broadening=broadening, xs_lut=xs_lut, continuum=continuum, keep_od=False)  # OD: this function's scratch
        run.run(T, P, PL, MF, ID)
        ready = torch.cuda.Event()
        ready.record()
        with torch.cuda.stream(side):
            side.wait_event(ready)
            blk = torch.empty((2 * nrow + 1, ln), dtype=torch.float64, device=dev)  # widened on the device
            blk[:nrow].copy_(tau[:, sl])
            blk[nrow:2 * nrow].copy_(Lu[:, sl])
            blk[2 * nrow].copy_(Ld[sl])
            for r in range(2 * nrow + 1):
                host[r, sl].copy_(blk[r], non_blocking=True)  # contiguous row segments
            done = torch.cuda.Event()
            done.record(side)
    for t in (tau, Lu, Ld, OD):
        t.record_stream(side)
    if done is not None:
        done.synchronize()
    return arr[:nrow], arr[nrow:2 * nrow], arr[2 * nrow:], (nZ, nMu)


def compute_TUD(Xmin, Xmax, opts=options, **kwargs):
    """Monochromatic transmittance, upwelling and downwelling radiance, signature of :274-392.

    kwargs honoured (:304-314): DVOUT, Zs, Ts, Ps, PLs, MFs_VAL, MFs_ID, theta_r, N_angle, Altitudes,
    save, returnOD, plus line_table and broadening. Returns (X, tau, Lu, Ld); tau/Lu are (nX,), (nX,nMu), (nX,nZ) or
    (nX,nZ,nMu) by the reference's squeeze rules (:357-365); Ld is (nX,).
    Quirks 3-6 of SURVEY.md section 9 are reproduced (downwelling uses the layer count of the last
    sensor altitude; tau uses the Z<=zs mask, L-up the first count layers; returnOD; theta=0 weight 0).
    X is a cached read-only array (see _cached_axis; copy_axis=True gives the reference's fresh writable one); the
    spectra are fresh float64 arrays -- views of page-locked memory while less than _hostio.PINNED_RESULT_CAP is lent
    out to live results, ordinary pageable arrays beyond that.
    broadening (keyword only, not in `options`): None, the default, broadens every line by air at the layer pressure.
    "self" broadens each species by the per-layer mix {air: 1 - x, self: x}, x its molecule's mixing ratio in that layer
    (MFs_VAL * 1e-6; 0 for a molecule not in MFs_ID) -- LBLRTM, behind the reference's compute_OD, broadens each absorber by
    its own partial pressure. ("self", "h2o", ...) adds foreign broadeners by HITRAN formula, each at its layer mixing
    ratio, read from the table's gamma_<formula>, n_<formula>, ... columns; a line of that gas takes self, air the remainder
    (engine.broadening_fractions).
    xs_lut (keyword only, not in `options`): an afit_xs.XsLut. The optical depths are then looked up in the cross-section
    table -- bilinear in T and ln p between its nodes, DESIGN 4.11 -- instead of summed over lines; line_table is neither
    needed nor touched, and everything after the optical depths is the same code. ValueError: the axis is not a contiguous
    run of the table's, a layer outside the table's (T, p) range, a molecule of MFs_ID the table lacks.
    NotImplementedError: xs_lut together with any broadening= (fixed when the table was made).
    continuum (keyword only, not in `options`): a continuum.Continuum. Its tabulated continuum absorption (the
    user's MT_CKD-style tables) is added to the optical depths of whichever branch made them, before the TUD sweep;
    returnOD=True therefore carries it. ValueError: a component whose molecule MFs_ID lacks.
    """
    trace = [time.perf_counter()] if _TRACE else None
    c = _Call("compute_TUD", Xmin, Xmax, opts, kwargs)
    o, lut, broadening, cont = c.o, c.lut, c.broadening, c.continuum
    Z, T, P, PL, MF, ID, Z_s, nA = c.Z, c.T, c.P, c.PL, c.MF, c.ID, c.Z_s, c.N_angle
    X_, grid = c.X, c.grid
    if trace:
        trace.append(time.perf_counter())
    tbl = c.table()
    if trace:
        trace.append(time.perf_counter())
    if o.get("copy_axis"):
        X_ = _hostio.copy_threaded(X_)
    chunks = o.get("chunks")
    if chunks is None:  # automatic: worth it once the copy of the result outweighs a chunk's fixed costs
        chunks = 4 if grid.n >= 2000000 else 2 if grid.n >= 500000 else 1
    if chunks > 1 and c.theta.size <= engine.TUD_MAX_MU and not o["save"]:
        got = _compute_tud_chunked(tbl, grid, Z, T, P, PL, MF, ID, Z_s, c.theta, nA, c.returnOD, int(chunks), broadening=broadening,
                                   xs_lut=lut, continuum=cont)
        if got is not None:
            tau_h, Lu_h, Ld_h, (nZ, nMu) = got
            if trace:
                trace.append(time.perf_counter())
                if trace[-1] - trace[0] > _TRACE * 1e-3:
                    print("compute_TUD %.1f ms (chunked x%d): options+axis %.2f  table %.2f  kernels + copies %.2f"
                          % tuple([1e3 * (trace[-1] - trace[0]), chunks] + [1e3 * (b - a) for a, b in zip(trace, trace[1:])]), flush=True)
            tau_, Lu_ = _tud_shapes(tau_h, Lu_h, nZ, nMu)
            return X_, tau_, Lu_, Ld_h[0]
    if c.theta.size <= engine.TUD_MAX_MU and not o["save"]:
        # the common case: one call into the library (rtx_compute_tud)
        run = engine.TudRunner(tbl, grid, Z, n_layers=T.size, Altitudes=Z_s, theta_r=c.theta, N_angle=nA, returnOD=c.returnOD,
                               broadening=broadening, xs_lut=lut, continuum=cont)
        tau, Lu, Ld = run.run(T, P, PL, MF, ID)
        nZ, nMu = run.shape
        OD = run.OD
    else:
        if lut is not None:
            OD = engine.xs_od(lut, grid, T, P / 101325.0, PL, MF, ID)
        else:
            OD = engine.optical_depths(tbl, grid, T, P, PL, MF, ID, broadening=broadening)  # [nL][nX] float32 on the device
        if cont is not None:
            engine.continuum_add(cont, grid, T, P, PL, MF, ID, OD)
        res = engine.tud(OD, grid, T, Z, Altitudes=Z_s, theta_r=c.theta, N_angle=nA, returnOD=c.returnOD, per_angle=bool(o["save"]))
        tau, Lu, Ld, (nZ, nMu) = res[:4]
    if trace:
        trace.append(time.perf_counter())
    (tau_h, Lu_h, Ld_h), done = _rows_to_host_f64([tau, Lu, Ld[None, :]])
    if trace:
        trace.append(time.perf_counter())
    done.synchronize()
    if trace:
        trace.append(time.perf_counter())
        if trace[-1] - trace[0] > _TRACE * 1e-3:  # RADTXFR_TRACE=<ms>: phases of every call slower than that
            print("compute_TUD %.1f ms: options+axis %.2f  table %.2f  enqueue kernels %.2f  enqueue copies %.2f  wait %.2f"
                  % tuple(1e3 * v for v in [trace[-1] - trace[0]] + [b - a for a, b in zip(trace, trace[1:])]), flush=True)
    tau_, Lu_ = _tud_shapes(tau_h, Lu_h, nZ, nMu)
    Ld_ = Ld_h[0]
    if o["save"]:
        angles = np.linspace(0, np.pi / 2.0, nA, endpoint=False)
        t3 = tau_h.reshape(nZ, nMu, -1).transpose(2, 0, 1)
        u3 = Lu_h.reshape(nZ, nMu, -1).transpose(2, 0, 1)
        np.savez("ComputeTUD.npz", OD=OD.double().cpu().numpy().T, B=planckian(X_, T), tau=t3, Ld=res[4].double().cpu().numpy().T,
                 Lu=u3, X=X_, angles=angles, Z_s=Z_s, mu_s=np.array([1.0 / np.cos(o["theta_r"])]).ravel())
    return X_, tau_, Lu_, Ld_


class _TudPipeline:
    """One device's share of compute_TUD_batch: the line table's copy on that device, two runners (two sets of device
    outputs: the copy of one is in flight while the other is being computed), each on a compute stream of its own, a
    side stream for the device-to-host copies, a pinned staging ring."""

    def __init__(self, dev, tbl, grid, Z, nL, Z_s, theta_r, N_angle, returnOD, broadening=None, xs_lut=None, continuum=None):
        self.dev = int(dev)
        with torch.cuda.device(self.dev):
            self.lines = tbl.on_device(self.dev) if xs_lut is None else None
            self.side = torch.cuda.Stream()
            # two runners, each with a stream, per-(line, layer) records and an optical-depth buffer of its own (another
            # pipeline may share the device and the table's cached plan): the prologue and TUD pass of one atmosphere overlap
            # the line-sum of the next (engine.TudPipelines)
            self.computes = [torch.cuda.Stream(), torch.cuda.Stream()]
            # (a cross-section table needs no records: its per-atmosphere terms are kept per stream, rtx_xs_od)
            self.plans = [engine.VoigtPlan(self.lines, nL, grid.n) if xs_lut is None else None for _ in range(2)]
            self.runs = []
            for st, pl in zip(self.computes, self.plans):
                with torch.cuda.stream(st):
                    self.runs.append(engine.TudRunner(self.lines, grid, Z, n_layers=nL, Altitudes=Z_s, theta_r=theta_r, N_angle=N_angle,
                                                      returnOD=returnOD, plan=pl, broadening=broadening, xs_lut=xs_lut,
                                                      continuum=continuum))
        self.busy = [None, None]  # copy-done event of each runner's outputs
        self.staging = _hostio.Staging(depth=2)
        self.k = 0

    def enqueue(self, a, ID, grid, x0, reduce, full_dtype):
        """Kernels + device-to-host copy of one atmosphere, all asynchronous. Returns a ticket for finish()."""
        j = self.k & 1
        self.k += 1
        run = self.runs[j]
        with torch.cuda.device(self.dev), torch.cuda.stream(self.computes[j]):
            if self.busy[j] is not None:
                self.computes[j].wait_event(self.busy[j])  # its previous outputs have left the device
            tau, Lu, Ld = run.run(np.asarray(a["Ts"], dtype=np.float64), np.asarray(a["Ps"], dtype=np.float64),
                                  np.asarray(a["PLs"], dtype=np.float64), np.asarray(a["MFs_VAL"], dtype=np.float64), ID)
            Xr = None
            if reduce is not None:
                rows = torch.cat([tau, Lu, Ld[None, :]])
                Xr, red = engine.reduce_resolution_cached(rows, x0, grid.step, grid.n, float(reduce["dX"]), N=reduce.get("N", 4),
                                                          window=reduce.get("window", "hanning"))
                nr = tau.shape[0]
                t = self.staging.stage([red[:nr], red[nr:2 * nr], red[2 * nr:]], stream=self.side)
            else:
                # full float64 spectra: zero-copy pinned blocks while the module's cap allows (a short batch then costs no host
                # work at all), the pinned staging ring + threaded widening into pageable arrays beyond it
                got = _hostio.rows_to_pinned_f64([tau, Lu, Ld[None, :]], stream=self.side) if full_dtype == np.float64 else None
                if got is not None:
                    self.busy[j] = got[1]
                    return ("pinned", got[0], got[1]), Xr
                t = self.staging.stage([tau, Lu, Ld[None, :]], stream=self.side)
            self.busy[j] = t[3]
        return t, Xr

    def finish(self, ticket, dtype):
        if ticket[0] == "pinned":
            ticket[2].synchronize()
            return ticket[1]
        with torch.cuda.device(self.dev):
            return self.staging.collect(ticket, dtype)

    def close(self):
        with torch.cuda.device(self.dev):
            torch.cuda.synchronize()
            for pl in self.plans:
                if pl is not None:
                    pl.close()


def compute_TUD_batch(Xmin, Xmax, atmospheres, opts=options, reduce=None, devices=None, out_dtype=np.float64, **kwargs):
    """compute_TUD for MANY atmospheres on one spectral grid -- the reference's outer loop
    (Generate_LWIR_TUD.py:117-150: 199 atmospheres x `rt.compute_TUD(..., MFs_VAL=, Ts=, ...)`, fanned out over a
    multiprocessing.Pool(6) there) as device pipelines driven by ONE host process: atmosphere k's device-to-host copy
    runs on a side stream while the next atmosphere's kernels run on the compute stream.

    atmospheres: sequence of dicts with any of Ts, Ps, PLs, MFs_VAL (the per-atmosphere kwargs of the reference's caller);
    everything else (Zs, MFs_ID, DVOUT, Altitudes, theta_r, N_angle, returnOD, line_table, broadening) comes from opts /
    kwargs and is common to the batch (broadening as for compute_TUD: the mix follows each atmosphere's MFs_VAL). reduce = dict(dX=..., N=4, window="hanning") applies reduceResolution (:1327-1350) to tau, Lu and
    Ld on the device, as the reference's caller does right after each compute_TUD (Generate_LWIR_TUD.py:124-126): only the
    reduced spectra cross PCIe then.
    devices: GPU indices to spread the atmospheres over (the reference's Pool axis without a launcher): atmosphere k goes
    to devices[k % len(devices)]; the line table is uploaded once per distinct device; an index may repeat (independent
    pipelines sharing a device). None = the current device. Results come back in input order and are bit-identical to
    per-call compute_TUD whatever the devices.
    out_dtype: float64 (the reference's) or float32 (half the host work when full spectra are kept).
    Returns a list of (X, tau, Lu, Ld) with the shapes compute_TUD gives (X_out instead of X when reduce is set). Full
    float64 spectra are views of page-locked blocks while fewer than _hostio.PINNED_RESULT_CAP bytes are lent out (1 GiB:
    the first eight C3-sized results), ordinary pageable arrays beyond that and for every other output (float32 crosses
    PCIe into a reusable pinned ring, a host thread pool widens: host-memory bound, ~10 ms per 132 MB result).
    xs_lut (keyword only): as for compute_TUD -- every atmosphere's optical depths come from the cross-section table, the line
    table is not touched, results equal per-call compute_TUD(xs_lut=) bit for bit. NotImplementedError: xs_lut with any
    broadening=, or with devices= naming more than one device (a table lives on one device).
    continuum (keyword only): as for compute_TUD, the same Continuum for every atmosphere; results equal per-call
    compute_TUD(continuum=) bit for bit. NotImplementedError: continuum with devices=."""
    c = _Call("compute_TUD_batch", Xmin, Xmax, opts, kwargs)
    o, lut, cont = c.o, c.lut, c.continuum
    if cont is not None and devices is not None:
        raise NotImplementedError("compute_TUD_batch: continuum with devices=%r is not supported; run on the current device "
                                  "(devices=None)" % (devices,))
    if lut is not None and devices is not None and len({int(d) for d in devices}) > 1:
        raise NotImplementedError("compute_TUD_batch: xs_lut with devices=%r is not supported: a cross-section table lives on one "
                                  "device" % (devices,))
    if o["save"]:
        raise ValueError("compute_TUD_batch: save is a single-call option")
    if np.dtype(out_dtype) not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError("compute_TUD_batch: out_dtype must be float64 or float32")
    if c.theta.size > engine.TUD_MAX_MU:
        raise ValueError("compute_TUD_batch takes at most %d slant paths" % engine.TUD_MAX_MU)
    c.foreign  # a broadening= that names no mix: refused before the device is asked for
    engine.require_gpu()
    devs = [torch.cuda.current_device()] if devices is None else [int(d) for d in devices]
    if not devs or any(d < 0 or d >= torch.cuda.device_count() for d in devs):
        raise ValueError("compute_TUD_batch: devices=%r, visible GPUs: %d" % (devices, torch.cuda.device_count()))
    X_, grid = c.X, c.grid
    if lut is not None and lut.device.index != devs[0]:
        raise ValueError("compute_TUD_batch: xs_lut lives on device %d, devices=%r" % (lut.device.index, devices))
    with torch.cuda.device(devs[0]):
        tbl = c.table()
    pipes = [_TudPipeline(d, tbl, grid, c.Z, c.T.size, c.Z_s, c.theta, c.N_angle, c.returnOD, broadening=c.broadening, xs_lut=lut,
                          continuum=cont)
             for d in devs]
    nZ, nMu = pipes[0].runs[0].shape
    pending = []  # (pipeline, ticket, X of the result) in input order
    results = []

    def finish(item):
        pipe, ticket, Xr = item
        tau_h, Lu_h, Ld_h = pipe.finish(ticket, np.dtype(out_dtype))
        tau_, Lu_ = _tud_shapes(tau_h, Lu_h, nZ, nMu)
        results.append((Xr, tau_, Lu_, Ld_h[0]))

    try:
        for k, atm in enumerate(atmospheres):
            a = dict(o)
            a.update(atm)
            pipe = pipes[k % len(pipes)]
            ticket, Xr = pipe.enqueue(a, c.ID, grid, float(X_[0]), reduce, np.dtype(out_dtype))
            pending.append((pipe, ticket, X_ if Xr is None else Xr))
            # a pipeline's staging ring has two slots: the atmosphere staged two rounds ago on it must be collected first
            while len(pending) > len(pipes):
                finish(pending.pop(0))
        while pending:
            finish(pending.pop(0))
    finally:
        for p_ in pipes:
            p_.close()
    return results


JACOBIAN_HOST_LIMIT = 4 << 30  # bytes of full-resolution float64 results compute_TUD_jacobian returns without reduce=


def _jacobian_args(fn, Xmin, Xmax, o, wrt, layers, reduce, fd_step_T, host_result=True, dT_method="fd"):
    """compute_TUD_jacobian's argument checks, all on the host (no device is touched), raised in the name of the calling
    function `fn`: (wrt, layers, nX). host_result=False: the caller returns no J (compute_TUD_vjp), so the size of a
    full-resolution J on the host is not a concern."""
    if dT_method not in engine.DT_METHODS:
        raise ValueError(fn + ": dT_method=%r, expected one of %r" % (dT_method, engine.DT_METHODS))
    if o.get("broadening") is not None:
        raise NotImplementedError(fn + ": broadening=%r is not supported (with self-broadening dOD/dMF is no "
                                  "longer OD per ppmv); use broadening=None" % (o.get("broadening"),))
    if np.asarray(o["theta_r"]).size != 1:
        raise NotImplementedError(fn + ": one slant path (a single theta_r) per call")
    if o["save"]:
        raise ValueError(fn + ": save=True is a compute_TUD option (the per-stream dump) and is not offered here")
    if isinstance(wrt, (str, int, np.integer)):
        wrt = (wrt,)
    wrt = tuple(w if isinstance(w, str) else int(w) for w in wrt)
    if not wrt:
        raise ValueError(fn + ": wrt is empty")
    ids = [int(v) for v in np.asarray(o["MFs_ID"]).ravel()]
    for w in wrt:
        if isinstance(w, str):
            if w != "T":
                raise ValueError(fn + ": wrt entry %r: \"T\" or a molecule id of MFs_ID %r" % (w, ids))
        elif w not in ids:
            raise ValueError(fn + ": wrt molecule id %d is not in MFs_ID %r" % (w, ids))
    if len(set(wrt)) != len(wrt):
        raise ValueError(fn + ": wrt %r names an entry twice" % (wrt,))
    nL = np.asarray(o["Ts"]).size
    lay = np.arange(nL) if layers is None else np.asarray(layers).ravel()
    if lay.size == 0 or not np.issubdtype(lay.dtype, np.integer):
        raise ValueError(fn + ": layers must be a non-empty sequence of layer indices")
    if lay.min() < 0 or lay.max() >= nL:
        raise ValueError(fn + ": layer index outside [0, %d)" % nL)
    if "T" in wrt and dT_method == "fd" and not (float(fd_step_T) > 0.0):
        raise ValueError(fn + ": fd_step_T=%r must be > 0" % (fd_step_T,))
    nX = int(np.ceil((Xmax - Xmin) / o["DVOUT"]))  # make_spectral_axis's count
    nZ = np.array([o["Altitudes"]]).size
    engine.jacobian_limits(nL, nZ, int(o["N_angle"]), sum(1 for w in wrt if not isinstance(w, str)))
    if not host_result:
        pass
    elif reduce is None:
        nbytes = 8 * nX * ((2 * nZ + 1) * (1 + len(wrt) * lay.size))
        if nbytes > JACOBIAN_HOST_LIMIT:
            raise ValueError(fn + ": the full-resolution result would take %.1f GiB of host memory (limit %.0f GiB): "
                             "pass reduce=dict(dX=...) or fewer layers= / wrt=" % (nbytes / 2.0 ** 30, JACOBIAN_HOST_LIMIT / 2.0 ** 30))
    elif "dX" not in reduce:
        raise ValueError(fn + ": reduce needs dX")
    return wrt, np.ascontiguousarray(lay, dtype=np.int32), nX


def _no_xs_lut(c, xs_derivatives=False):
    """The cross-section table a derivative function differentiates call `c` through: None without xs_lut=; the call's
    XsLut with xs_derivatives=True (_xs_lut_option's refusal of broadening= applies);
    NotImplementedError in the function's name with the default False, before the table is touched: by default the
    derivatives are built on the line-sum, and OD from a table is piecewise in T (a layer on a T node takes one cell's slope)."""
    if c.o.get("xs_lut") is None:
        return None
    if not xs_derivatives:
        raise NotImplementedError(c.fn + ": xs_lut is not supported by default (dOD/dT is a difference of line-sums with fixed "
                                  "windows); use line_table=, or pass xs_derivatives=True to differentiate through the table")
    return c.lut


def _xs_axis(c, lut):
    """With a table to differentiate through: ValueError, before any device work, unless the call's axis is a run of the
    table's (XsLut.align; there is no spectral interpolation)."""
    if lut is not None:
        lut.align(c.grid)


def _derivative_continuum(c, continuum_derivatives):
    """The continuum a derivative function differentiates call `c` through: None without continuum=; the call's Continuum
    with continuum_derivatives=True (checked as _continuum_option checks it: ValueError for a component whose molecule
    MFs_ID lacks, before any device work); NotImplementedError in the function's name with the default False, which keeps
    a forward model with a continuum from being paired with a Jacobian that silently lacks it."""
    if c.o.get("continuum") is None:
        return None
    if not continuum_derivatives:
        raise NotImplementedError(c.fn + ": continuum is not supported by default (its self term is quadratic in the mixing "
                                  "ratio: a species derivative is then local to the state); pass continuum_derivatives=True "
                                  "to differentiate through it, or continuum=None")
    return c.continuum


def _vector_axis(g, base):
    """An array or tensor laid out as `base` plus an optional trailing vector axis: (g with that axis, its length -- None
    where g came without one), or None when g's shape is neither."""
    shape = tuple(g.shape)
    if shape == base:
        return g[..., None], None
    if len(shape) == len(base) + 1 and shape[:-1] == base and shape[-1] >= 1:
        return g, shape[-1]
    return None


def _grad_dict(grad_h, wrt, n_vec):
    """{wrt entry: float64 [n_layers], or [n_layers][n_vec] with a vector axis} from engine.tud_vjp's grad on the host,
    [n_vec][n_wrt][n_layers]."""
    return {w: np.ascontiguousarray(grad_h[:, w_i, :].T) if n_vec is not None else grad_h[0, w_i, :].copy()
            for w_i, w in enumerate(wrt)}


def compute_TUD_jacobian(Xmin, Xmax, opts=options, wrt=("T",), layers=None, reduce=None, fd_step_T=0.5, dT_method="fd",
                         continuum_derivatives=False, xs_derivatives=False, **kwargs):
    """compute_TUD and the derivatives of its outputs with respect to layer temperatures and mixing ratios in one call:
    what the reference's caller builds from 1 + 3 x 66 perturbed atmospheres (Generate_LWIR_TUD.py:55-71, JacIn, one
    layer and one quantity at a time, relStep 0.001) -- here closed-form chain rule through the TUD recurrences.

    kwargs as compute_TUD (DVOUT, Zs, Ts, Ps, PLs, MFs_VAL, MFs_ID, Altitudes, theta_r, N_angle, returnOD, line_table); one
    theta_r; save is not offered. wrt: "T" and / or molecule ids of MFs_ID. layers: layer indices (default all), in
    output order. Returns (X, tau, Lu, Ld, J):
      X, tau, Lu, Ld  bit-identical to compute_TUD with the same kwargs (reduced as compute_TUD_batch(reduce=) reduces them
                      when `reduce` is given, X then the reduced axis);
      J               {wrt entry: (dtau, dLu, dLd)}, each float64 with the shape compute_TUD gives that output plus a
                      trailing axis over `layers`, in units per K ("T") and per ppmv (a molecule id, the unit of MFs_VAL).
    Definition: for layer l and x in {T_l, MF_s,l}, d/dx of the same outputs compute_TUD returns -- the tau slot (tau, or
    sum(OD) mu under returnOD), L-up per sensor altitude and Ld, with every quirk of the reference's TUD body (the
    Z <= zs mask for tau, the first count(mask) layers for L-up, the last altitude's count for Ld, weight 0 at theta = 0).
    With N_angle = 1 that Ld is 0/0 (NaN), and so is every dLd.
    OD_l is linear in MF_s,l (without a continuum): dOD_l/dMF_s,l is the line-sum of species s alone at 1 ppmv (exact; MF = 0
    is fine).
    dOD_l/dT_l is the central difference of line-sums at T -+ fd_step_T [K] with every line's window held at the base T:
    the derivative of the truncated line-sum with each line's support fixed (the reference's cut-off OmegaWingHW x width
    moves with T; a finite difference of it carries those steps). Everything else is analytic.
    dT_method="analytic": dOD_l/dT_l is the closed-form derivative of the Voigt line-sum with the same fixed windows instead
    (engine.voigt_sum_dT): one line-sum in place of the two, no step to choose (fd_step_T is ignored). The
    default "fd" returns what it always did; any other value raises ValueError.
    reduce = dict(dX=..., N=4, window="hanning"): reduceResolution of the base outputs and of every J row on the device
    (engine.reduce_resolution_cached). Without it, full-resolution results above 4 GiB are refused (ValueError): pass
    reduce= or fewer layers=. Arguments are checked before any device work.
    xs_lut= (as compute_TUD takes it) is refused (NotImplementedError, before the table is touched) unless
    xs_derivatives=True; then the call is differentiated through the cross-section table: the base outputs
    are compute_TUD(xs_lut=)'s bit for bit, "analytic" takes dOD/dT and every species column from the table in one pass
    (rtx_xs_od_d), "fd" the table's forward rule at T -+ fd_step_T (ValueError where the step leaves the table). The table
    is piecewise in T: a layer exactly on a T node takes the slope of the cell the forward run used, the cell to its right
    (to its left on the last node). A species of wrt must lie inside its table in every layer, also where its mixing
    ratio is 0. xs_derivatives=True without an xs_lut is the plain call, bit for bit.
    continuum= (as compute_TUD takes it) is refused (NotImplementedError) unless continuum_derivatives=True; then the
    call is differentiated through the continuum: the base outputs are compute_TUD(continuum=)'s bit for
    bit, "fd" takes the continuum at T -+ fd_step_T with the line-sums, "analytic" its closed-form dOD/dT. With a
    continuum OD is no longer linear in a mixing ratio (the self term is quadratic in it): J's species entries are the
    local derivative at the state, per ppmv, and a component differentiates only with respect to its own molecule. The
    continuum is piecewise, OD_c = max(0, R S_c): where a component's interpolated sum S_c is <= 0 its derivatives are
    exactly 0 -- the kink at S_c = 0 is given the value 0 (continuum.Continuum.dod_host is the definition).
    continuum_derivatives=True without a continuum is the plain call, bit for bit. ValueError, before any device work,
    for a component whose molecule MFs_ID lacks."""
    c = _Call("compute_TUD_jacobian", Xmin, Xmax, opts, kwargs)
    lut = _no_xs_lut(c, xs_derivatives)
    cont = _derivative_continuum(c, continuum_derivatives)
    wrt, lay, _ = _jacobian_args(c.fn, Xmin, Xmax, c.o, wrt, layers, reduce, fd_step_T, dT_method=dT_method)
    _xs_axis(c, lut)
    X_, grid = c.X, c.grid
    tbl = c.table()
    nZ = c.Z_s.size
    nrow = 2 * nZ + 1
    n_lay = lay.size
    red = None
    if reduce is not None:
        red = dict(dX=float(reduce["dX"]), N=reduce.get("N", 4), window=reduce.get("window", "hanning"))
    x0 = float(X_[0])
    host = {}  # wrt entry -> float64 [nX_out][nrow][n_lay]

    def on_block(k0, k1, blk):
        rows = blk.view(-1, grid.n)
        if red is not None:
            _, out = engine.reduce_resolution_cached(rows, x0, grid.step, grid.n, red["dX"], N=red["N"], window=red["window"])
        else:
            out = rows
        out = out.view(len(wrt), k1 - k0, nrow, -1)
        for w_i, w in enumerate(wrt):
            h = out[w_i].permute(2, 1, 0).to(torch.float64).cpu().numpy()  # [n_out][nrow][k1-k0]
            if w not in host:
                host[w] = np.empty((h.shape[0], nrow, n_lay))
            host[w][:, :, k0:k1] = h

    tau, Lu, Ld, _, _ = engine.tud_jacobian(tbl, grid, c.Z, c.T, c.P, c.PL, c.MF, c.ID, Altitudes=c.Z_s, theta_r=c.theta,
                                             N_angle=c.N_angle, returnOD=c.returnOD, wrt=wrt, layers=lay,
                                             fd_step_T=float(fd_step_T), on_block=on_block, dT_method=dT_method,
                                             continuum=cont, xs_lut=lut)
    if red is not None:
        rows = torch.cat([tau, Lu, Ld[None, :]])
        X_out, r = engine.reduce_resolution_cached(rows, x0, grid.step, grid.n, red["dX"], N=red["N"], window=red["window"])
        r = r.cpu().numpy()
        tau_, Lu_ = _tud_shapes(r[:nZ], r[nZ:2 * nZ], nZ, 1)
        Ld_ = r[2 * nZ]
    else:
        (tau_h, Lu_h, Ld_h), done = _rows_to_host_f64([tau, Lu, Ld[None, :]])
        done.synchronize()
        tau_, Lu_ = _tud_shapes(tau_h, Lu_h, nZ, 1)
        Ld_ = Ld_h[0]
        X_out = X_
    J = {}
    for w in wrt:
        h = host[w]
        if nZ == 1:
            J[w] = (np.ascontiguousarray(h[:, 0, :]), np.ascontiguousarray(h[:, 1, :]), np.ascontiguousarray(h[:, 2, :]))
        else:
            J[w] = (np.ascontiguousarray(h[:, :nZ, :]), np.ascontiguousarray(h[:, nZ:2 * nZ, :]), np.ascontiguousarray(h[:, 2 * nZ, :]))
    return X_out, tau_, Lu_, Ld_, J


_COTANGENT_KEYS = ("tau", "La", "Ld")


def _vjp_cotangents(cotangents, nX, nZ):
    """compute_TUD_vjp's cotangents, checked on the host: ({key: array or tensor [n_vec][nZ][nX] / [n_vec][nX]}, n_vec or
    None without a vector axis). Each entry is laid out like the compute_TUD output it belongs to, [nX][nZ] (or [nX] with
    one altitude) and [nX], with an optional trailing vector axis."""
    if not isinstance(cotangents, dict) or not cotangents:
        raise ValueError("compute_TUD_vjp: cotangents must be a non-empty dict with keys among %r" % (_COTANGENT_KEYS,))
    out, n_vecs = {}, set()
    for key, g in cotangents.items():
        if key not in _COTANGENT_KEYS:
            raise ValueError("compute_TUD_vjp: unknown cotangent key %r (expected keys among %r)" % (key, _COTANGENT_KEYS))
        if g is None:
            continue
        if not _is_torch(g):
            g = np.asarray(g)
        base = (nX,) if key == "Ld" else (nX, nZ)
        shape = tuple(g.shape)
        if key != "Ld" and nZ == 1 and shape[:2] != base and shape[:1] == (nX,) and len(shape) <= 2:
            g = g[:, None]  # one altitude: compute_TUD squeezes the altitude axis
        got = _vector_axis(g, base)
        if got is None:
            raise ValueError("compute_TUD_vjp: cotangent %r has shape %r, expected %r plus an optional trailing vector axis"
                             % (key, tuple(g.shape), base))
        g, nv = got
        n_vecs.add(nv)
        # [nX]([nZ])[n_vec] -> [n_vec]([nZ])[nX]
        out[key] = g.permute(*range(g.dim() - 1, -1, -1)) if _is_torch(g) else np.transpose(g)
    if not out:
        raise ValueError("compute_TUD_vjp: every cotangent is None")
    if len(n_vecs) != 1:
        raise ValueError("compute_TUD_vjp: the cotangents disagree on the vector axis: %r" % sorted(n_vecs, key=str))
    return out, n_vecs.pop()


def compute_TUD_vjp(Xmin, Xmax, cotangents, opts=options, wrt=("T",), layers=None, fd_step_T=0.5, dT_method="fd",
                    continuum_derivatives=False, xs_derivatives=False, **kwargs):
    """compute_TUD and the gradient of a scalar cost of its outputs with respect to layer temperatures and mixing ratios:
    the transpose of compute_TUD_jacobian's J applied to the cost's cotangents, without J ever being stored (reverse mode;
    DESIGN 4.16).

    cotangents: dict with any of "tau", "La", "Ld": d cost / d output, each laid out like the compute_TUD output of that
    name ([nX][nAlt] -- [nX] with one altitude -- and [nX]), NumPy arrays or torch tensors (a device tensor is used where
    it is). An optional trailing axis of length n_vec carries several cotangent vectors at once (they share all the work
    up to the contraction). A key left out is a row group that is not evaluated: without "Ld" the downwelling stream
    sweeps, the expensive part of the Jacobian, are not run.
    kwargs, wrt, layers, fd_step_T, dT_method: as compute_TUD_jacobian, with the same definition of every derivative. Returns
    (X, tau, La, Ld, grad): X, tau, La, Ld bit-identical to compute_TUD with the same kwargs; grad {wrt entry: float64
    [n_layers]}, or [n_layers][n_vec] when a vector axis is given:
      grad[w][k(, v)] = sum over X and over the outputs with a cotangent of cotangent[(X, row, v)] * J[w][row][X, k],
    in units of cost per K ("T") and per ppmv (a molecule id). Products with the cotangents and all sums are float64 in a
    fixed order: the same call gives the same bits, whatever other layers or vectors it carries.
    There is no reduce=: a cost defined on a reduced axis, Y = R X_native with R linear (reduceResolution, a slit
    function), has the native-grid cotangent R^T (d cost / d Y), which is passed here. For a cost defined on at-sensor
    band radiances under a sensor's response tables, compute_band_radiance_vjp runs the whole chain, sensor adjoint
    included, and also returns the gradients of the surface temperature and the emissivity knots.
    continuum=, continuum_derivatives: as compute_TUD_jacobian (refused unless continuum_derivatives=True; then OD is not
    linear in a mixing ratio, a species entry is the local derivative at the state per ppmv, and where a continuum
    component's interpolated sum is <= 0 its derivatives are 0: the kink of max(0, .) is given the value 0).
    xs_lut=, xs_derivatives: as compute_TUD_jacobian (refused unless xs_derivatives=True; then every column comes from the
    cross-section table, DESIGN 4.24, and a layer exactly on a T node takes the slope of the cell to its right, to its left
    on the last node).
    Arguments are checked before any device work. NotImplementedError: more than one theta_r, broadening=, xs_lut= by default."""
    c = _Call("compute_TUD_vjp", Xmin, Xmax, opts, kwargs)
    if "reduce" in c.o:
        raise NotImplementedError("compute_TUD_vjp: reduce= is not offered: map the cotangent to the native grid with the "
                                  "transpose of the reduction and pass that")
    lut = _no_xs_lut(c, xs_derivatives)
    cont = _derivative_continuum(c, continuum_derivatives)
    wrt, lay, nX = _jacobian_args(c.fn, Xmin, Xmax, c.o, wrt, layers, None, fd_step_T, host_result=False, dT_method=dT_method)
    _xs_axis(c, lut)
    nZ = c.Z_s.size
    G, n_vec = _vjp_cotangents(cotangents, nX, nZ)
    X_, grid = c.X, c.grid
    assert X_.size == nX
    tbl = c.table()
    tau, Lu, Ld, _, grad = engine.tud_vjp(tbl, grid, c.Z, c.T, c.P, c.PL, c.MF, c.ID, G_tau=G.get("tau"), G_Lu=G.get("La"),
                                          G_Ld=G.get("Ld"), Altitudes=c.Z_s, theta_r=c.theta, N_angle=c.N_angle,
                                          returnOD=c.returnOD, wrt=wrt, layers=lay, fd_step_T=float(fd_step_T), dT_method=dT_method,
                                          continuum=cont, xs_lut=lut)
    (tau_h, Lu_h, Ld_h), done = _rows_to_host_f64([tau, Lu, Ld[None, :]])
    grad_h = grad.cpu().numpy()  # [n_vec][n_wrt][n_layers]
    done.synchronize()
    tau_, Lu_ = _tud_shapes(tau_h, Lu_h, nZ, 1)
    return X_, tau_, Lu_, Ld_h[0], _grad_dict(grad_h, wrt, n_vec)


def _jvp_tangents(tangents, n_lay, fn="compute_TUD_jvp"):
    """compute_TUD_jvp's tangents (a dict whose keys are checked already), checked on the host: (V float64
    [n_vec][n_wrt][n_lay], n_vec or None without a vector axis). Each entry is [n_lay] or [n_lay][n_vec]; the wrt axis
    follows the dict's order. Errors are raised in the name of the calling function `fn`."""
    cols, n_vecs = [], set()
    for key, v in tangents.items():
        v = np.asarray(v.detach().cpu().numpy() if _is_torch(v) else v, dtype=np.float64)
        got = _vector_axis(v, (n_lay,))
        if got is None:
            raise ValueError(fn + ": tangent %r has shape %r, expected %r (one entry per layer of layers=) plus an optional "
                             "trailing vector axis" % (key, tuple(v.shape), (n_lay,)))
        v, nv = got
        if not np.isfinite(v).all():
            raise ValueError(fn + ": tangent %r has non-finite entries" % (key,))
        n_vecs.add(nv)
        cols.append(v.T)  # [n_vec][n_lay]
    if len(n_vecs) != 1:
        raise ValueError(fn + ": the tangents disagree on the vector axis: %r" % sorted(n_vecs, key=str))
    return np.ascontiguousarray(np.stack(cols, axis=1)), n_vecs.pop()


def compute_TUD_jvp(Xmin, Xmax, tangents, opts=options, layers=None, rows=("tau", "La", "Ld"), fd_step_T=0.5, dT_method="fd",
                    continuum_derivatives=False, xs_derivatives=False, **kwargs):
    """compute_TUD and the change of its outputs along directions in (layer temperatures, mixing ratios): compute_TUD_jacobian's
    J applied to tangent vectors, without J ever being stored (forward mode). The result is spectra, 2 nAlt + 1
    rows per vector: it fits where J does not.

    tangents: dict {"T" or a molecule id of MFs_ID: array [n_layers], or [n_layers][n_vec] for several directions at once},
    in K ("T") and ppmv (a molecule id) per layer of `layers` (default all; layers not named do not move; a layer named
    twice moves by the sum of its entries). The keys are the wrt of compute_TUD_jacobian. rows: which of "tau", "La", "Ld"
    are evaluated: without "Ld" the downwelling stream sweeps, the expensive part, are not run.
    kwargs, layers, fd_step_T, dT_method: as compute_TUD_jacobian, with the same definition of every derivative. Returns
    (X, tau, La, Ld, d): X, tau, La, Ld bit-identical to compute_TUD with the same kwargs; d {"tau", "La", "Ld"} restricted
    to `rows`, each float64 and shaped like the output of that name, plus a trailing [n_vec] axis when the tangents have one:
      d[row][X(, alt)(, v)] = sum over the keys w and the layers k of J[w][row][X(, alt), k] * tangents[w][k(, v)].
    The tangents are carried through the TUD recurrences in float64 and each result is rounded to float32 once; a point's
    value does not depend on the other vectors of the call. There is no reduce=: the results are spectra, and
    reduceResolution takes them as it takes any spectrum.
    continuum=, continuum_derivatives: as compute_TUD_jacobian (refused unless continuum_derivatives=True; then OD is not
    linear in a mixing ratio, a species entry is the local derivative at the state per ppmv, and where a continuum
    component's interpolated sum is <= 0 its derivatives are 0: the kink of max(0, .) is given the value 0).
    xs_lut=, xs_derivatives: as compute_TUD_jacobian (refused unless xs_derivatives=True; then every column comes from the
    cross-section table, DESIGN 4.24, and a layer exactly on a T node takes the slope of the cell to its right, to its left
    on the last node).
    Arguments are checked before any device work. NotImplementedError: more than one theta_r, broadening=, xs_lut= by default."""
    c = _Call("compute_TUD_jvp", Xmin, Xmax, opts, kwargs)
    if "reduce" in c.o:
        raise NotImplementedError("compute_TUD_jvp: reduce= is not offered: the results are spectra, pass them to reduceResolution")
    lut = _no_xs_lut(c, xs_derivatives)
    cont = _derivative_continuum(c, continuum_derivatives)
    if isinstance(tangents, dict) and tangents:
        wrt = tuple(tangents.keys())
        bad = [k for k in wrt if k != "T" and (isinstance(k, bool) or not isinstance(k, (int, np.integer)))]
        if bad:
            raise ValueError("compute_TUD_jvp: unknown tangent key %r (expected \"T\" or a molecule id of MFs_ID)" % (bad[0],))
    else:
        raise ValueError("compute_TUD_jvp: tangents must be a non-empty dict {\"T\" or a molecule id of MFs_ID: array}")
    wrt, lay, nX = _jacobian_args(c.fn, Xmin, Xmax, c.o, wrt, layers, None, fd_step_T, host_result=False, dT_method=dT_method)
    _xs_axis(c, lut)
    if isinstance(rows, str):
        rows = (rows,)
    rows = tuple(rows)
    if not rows or any(r not in engine.JVP_ROWS for r in rows) or len(set(rows)) != len(rows):
        raise ValueError("compute_TUD_jvp: rows %r, expected distinct names among %r" % (rows, engine.JVP_ROWS))
    V, n_vec = _jvp_tangents(tangents, lay.size)
    nZ = c.Z_s.size
    X_, grid = c.X, c.grid
    assert X_.size == nX
    tbl = c.table()
    tau, Lu, Ld, _, d = engine.tud_jvp(tbl, grid, c.Z, c.T, c.P, c.PL, c.MF, c.ID, V, Altitudes=c.Z_s, theta_r=c.theta,
                                       N_angle=c.N_angle, returnOD=c.returnOD, wrt=wrt, layers=lay, fd_step_T=float(fd_step_T),
                                       rows=rows, dT_method=dT_method, continuum=cont, xs_lut=lut)
    (tau_h, Lu_h, Ld_h), done = _rows_to_host_f64([tau, Lu, Ld[None, :]])
    d_h = {name: t.to(torch.float64).cpu().numpy() for name, t in d.items()}  # [n_vec]([nZ])[nX]
    done.synchronize()
    tau_, Lu_ = _tud_shapes(tau_h, Lu_h, nZ, 1)
    out = {}
    for name in engine.JVP_ROWS:
        if name not in d_h:
            continue
        a = np.transpose(d_h[name])  # [nX]([nZ])[n_vec]
        if name != "Ld" and nZ == 1:
            a = a[:, 0]  # one altitude: compute_TUD squeezes the altitude axis
        out[name] = np.ascontiguousarray(a if n_vec is not None else a[..., 0])
    return X_, tau_, Lu_, Ld_h[0], out


def compute_band_radiance_vjp(Xmin, Xmax, sensor, Xk, emis_knots, Ts_surface, cotangent, opts=options, wrt=("T",), layers=None,
                              fd_step_T=0.5, dT_method="fd", continuum_derivatives=False, xs_derivatives=False, **kwargs):
    """At-sensor band radiances over a surface and the gradient of a scalar cost defined on them, in one call: the
    line-sums (base, T -+ fd_step_T, each species of wrt), compute_TUD's tau / La / Ld, the band radiances of
    sensor.band_radiance_srf_fused under the sensor's response tables, their adjoint (sensor.band_radiance_srf_vjp) and
    compute_TUD_vjp's adjoint on the native-grid cotangents that gives, which stay on the device. The optical depths are
    computed once; no Jacobian and nothing of size nX x nE is stored.

    sensor: a sensor.Sensor; Xk [nk] the emissivity knots [cm^-1], emis_knots [nk][nE] (float32; NumPy or a torch tensor);
    Ts_surface: a scalar or a 1-D sequence of surface temperatures [K]. cotangent = d cost / d L, laid out like L:
    [nB][nE] for a scalar Ts_surface, [nT][nB][nE] for a sequence, with an optional trailing axis of n_vec cotangent
    vectors (they share everything up to the sensor adjoint). kwargs, wrt, layers, fd_step_T, dT_method as compute_TUD_vjp, with
    exactly one sensor altitude and returnOD=False. Returns (X_out, L, grad):
      X_out  sensor.centres;
      L      float32 NumPy, bit-identical to band_radiance_srf_fused on compute_TUD's outputs (NaN for a band with no
             grid point under it; such a band contributes nothing to any gradient, whatever its cotangent holds);
      grad   {wrt entry: float64 [n_layers]} as compute_TUD_vjp returns them, plus "Ts_surface" (float64, Ts_surface's
             shape) and "emis" (float64 [nk][nE]); every entry with a trailing [n_vec] axis when the cotangent has one.
    continuum=, continuum_derivatives: as compute_TUD_jacobian (refused unless continuum_derivatives=True; then OD is not
    linear in a mixing ratio, a species entry is the local derivative at the state per ppmv, and where a continuum
    component's interpolated sum is <= 0 its derivatives are 0: the kink of max(0, .) is given the value 0).
    xs_lut=, xs_derivatives: as compute_TUD_jacobian (refused unless xs_derivatives=True; then every column comes from the
    cross-section table, DESIGN 4.24, and a layer exactly on a T node takes the slope of the cell to its right, to its left
    on the last node).
    Arguments are checked before any device work. NotImplementedError: more than one altitude or theta_r, returnOD=True,
    broadening=, xs_lut= by default, reduce=."""
    name = "compute_band_radiance_vjp"
    c = _Call(name, Xmin, Xmax, opts, kwargs)
    if "reduce" in c.o:
        raise NotImplementedError(name + ": reduce= is not offered: the cost is defined on the sensor's bands")
    lut = _no_xs_lut(c, xs_derivatives)
    cont = _derivative_continuum(c, continuum_derivatives)
    if c.returnOD:
        raise NotImplementedError(name + ": returnOD=True is not supported (the sensor stage takes transmittances)")
    if c.Z_s.size != 1:
        raise NotImplementedError(name + ": exactly one sensor altitude per call (got %d)" % c.Z_s.size)
    wrt, lay, nX = _jacobian_args(name, Xmin, Xmax, c.o, wrt, layers, None, fd_step_T, host_result=False, dT_method=dT_method)
    _xs_axis(c, lut)
    Xk = np.ascontiguousarray(np.asarray(Xk, dtype=np.float64).ravel())
    scalar = np.ndim(Ts_surface) == 0
    Ts_s = np.atleast_1d(np.asarray(Ts_surface, dtype=np.float64))
    if Ts_s.ndim != 1 or Ts_s.size == 0 or not np.all(Ts_s > 0.0):
        raise ValueError(name + ": Ts_surface must be a positive scalar or a non-empty 1-D sequence of positive temperatures")
    if not _is_torch(emis_knots):
        emis_knots = np.asarray(emis_knots)
    if tuple(emis_knots.shape[:1]) != (Xk.size,) or len(emis_knots.shape) != 2 or emis_knots.shape[1] < 1:
        raise ValueError(name + ": emis_knots has shape %r, expected [%d][nE]" % (tuple(emis_knots.shape), Xk.size))
    nB, nE, nT = len(sensor), int(emis_knots.shape[1]), Ts_s.size
    base = (nB, nE) if scalar else (nT, nB, nE)
    g = cotangent if _is_torch(cotangent) else np.asarray(cotangent)
    got = _vector_axis(g, base)
    if got is None:
        raise ValueError(name + ": cotangent has shape %r, expected %r (L's shape) plus an optional trailing vector axis"
                         % (tuple(g.shape), base))
    g, n_vec = got
    from . import sensor as _sensor  # sensor.py imports this module
    grid = c.grid
    assert c.X.size == nX
    tbl = c.table()
    dev = engine.device()
    E_d = _dev_f32(emis_knots, dev).contiguous()
    g_d = _dev_f32(g, dev)
    Ts_arg = float(Ts_s[0]) if scalar else Ts_s
    nv = g_d.shape[-1]
    kept = {}

    def sensor_stage(tau, Lu, Ld):
        t_, u_, d_ = tau[0, :nX].contiguous(), Lu[0, :nX].contiguous(), Ld[:nX].contiguous()
        _, kept["L"] = _sensor.band_radiance_srf_fused(grid, t_, u_, d_, Xk, E_d, Ts_arg, sensor)
        G = [torch.empty((nv, 1, nX), dtype=torch.float32, device=dev), torch.empty((nv, 1, nX), dtype=torch.float32, device=dev),
             torch.empty((nv, nX), dtype=torch.float32, device=dev)]
        kept["Ts"], kept["emis"] = [], []
        for v in range(nv):
            r = _sensor.band_radiance_srf_vjp(grid, t_, u_, d_, Xk, E_d, Ts_arg, sensor, g_d[..., v])
            G[0][v, 0], G[1][v, 0], G[2][v] = r["G_tau"], r["G_La"], r["G_Ld"]
            kept["Ts"].append(r["Ts"])
            kept["emis"].append(r["emis"])
        return G

    _, _, _, _, grad = engine.tud_vjp(tbl, grid, c.Z, c.T, c.P, c.PL, c.MF, c.ID, Altitudes=c.Z_s, theta_r=c.theta,
                                      N_angle=c.N_angle, returnOD=False, wrt=wrt, layers=lay, fd_step_T=float(fd_step_T),
                                      cotangents=sensor_stage, dT_method=dT_method, continuum=cont, xs_lut=lut)
    L_h = kept["L"].cpu().numpy()
    dTs_h = torch.stack(kept["Ts"], dim=-1).cpu().numpy()    # Ts_surface's shape + [n_vec]
    dE_h = torch.stack(kept["emis"], dim=-1).cpu().numpy()   # [nk][nE][n_vec]
    out = _grad_dict(grad.cpu().numpy(), wrt, n_vec)
    out["Ts_surface"] = np.ascontiguousarray(dTs_h) if n_vec is not None else dTs_h[..., 0].copy()
    out["emis"] = np.ascontiguousarray(dE_h) if n_vec is not None else dE_h[..., 0].copy()
    return np.array(sensor.centres), L_h, out


def compute_hsi_cube_vjp(Xmin, Xmax, sensor, Xk, endmembers, kidx, frac, Tpix, cotangent, opts=options, wrt=("T",), layers=None,
                         fd_step_T=0.5, dT_method="fd", continuum_derivatives=False, xs_derivatives=False, n_nodes=8, T_range=None,
                         interp_tol=1e-6, **kwargs):
    """The per-pixel HSI cube of a scene under any sensor and the gradient of a scalar cost defined on it, in one call:
    the line-sums, compute_TUD's tau / La / Ld, sensor.hsi_cube_srf's cube, its adjoint (sensor.hsi_cube_srf_vjp) and
    compute_TUD_vjp's adjoint on the native-grid cotangents that gives, which stay on the device. No Jacobian and nothing
    of size nPix x nX is stored.

    sensor: a sensor.Sensor; Xk [nk] the emissivity knots [cm^-1]; endmembers [nk][nEnd] (float32), kidx [nPix][nMix]
    (integers), frac [nPix][nMix] (float32), Tpix [nPix] (float64): the scene, NumPy or torch tensors, as hsi_cube_srf takes
    it; n_nodes, T_range, interp_tol as there (T_range=None: the smallest and largest finite Tpix). cotangent = d cost /
    d cube, [nB][nPix]: one vector per call. kwargs, wrt, layers, fd_step_T, dT_method as compute_TUD_vjp, with exactly one
    sensor altitude and returnOD=False. Returns (X_out, cube, grad):
      X_out  sensor.centres;
      cube   float32 NumPy [nB][nPix], bit-identical to hsi_cube_srf on compute_TUD's outputs;
      grad   {wrt entry: float64 [n_layers]} as compute_TUD_vjp returns them, plus "Tpix" [nPix], "frac" [nPix][nMix] and
             "endmembers" [nk][nEnd], float64.
    continuum=, continuum_derivatives, xs_lut=, xs_derivatives: as compute_band_radiance_vjp.
    Arguments are checked before any device work. NotImplementedError: more than one altitude or theta_r, returnOD=True,
    broadening=, xs_lut= or continuum= without their derivative flags, reduce=. ValueError: a cotangent that is not
    [nB][nPix] (a trailing vector axis is not offered)."""
    name = "compute_hsi_cube_vjp"
    c = _Call(name, Xmin, Xmax, opts, kwargs)
    if "reduce" in c.o:
        raise NotImplementedError(name + ": reduce= is not offered: the cost is defined on the sensor's bands")
    lut = _no_xs_lut(c, xs_derivatives)
    cont = _derivative_continuum(c, continuum_derivatives)
    if c.returnOD:
        raise NotImplementedError(name + ": returnOD=True is not supported (the sensor stage takes transmittances)")
    if c.Z_s.size != 1:
        raise NotImplementedError(name + ": exactly one sensor altitude per call (got %d)" % c.Z_s.size)
    wrt, lay, nX = _jacobian_args(name, Xmin, Xmax, c.o, wrt, layers, None, fd_step_T, host_result=False, dT_method=dT_method)
    _xs_axis(c, lut)
    from . import sensor as _sensor  # sensor.py imports this module

    def host(v, what, kinds, dtype):
        a = v.detach().cpu().numpy() if _is_torch(v) else np.asarray(v)
        if a.dtype.kind not in kinds:
            raise ValueError(name + ": %s has dtype %s" % (what, a.dtype))
        return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype))

    Xk = np.ascontiguousarray(np.asarray(Xk, dtype=np.float64).ravel())
    E_h, k_h = host(endmembers, "endmembers", "f", np.float32), host(kidx, "kidx", "iu", np.int32)
    f_h, T_h = host(frac, "frac", "f", np.float32), host(Tpix, "Tpix", "f", np.float64)
    g_h = host(cotangent, "cotangent", "f", np.float32)
    if k_h.dim() == 2 and g_h.dim() == 3 and tuple(g_h.shape[:2]) == (len(sensor), k_h.shape[0]):
        raise ValueError(name + ": one cotangent vector per call: cotangent has shape %r, expected %r"
                         % (tuple(g_h.shape), (len(sensor), k_h.shape[0])))
    z = torch.zeros(nX, dtype=torch.float32)  # stands for tau, La, Ld in the checks
    grid = c.grid
    assert c.X.size == nX
    front = _sensor._srf_cube_front(name, grid, z, z, z, Xk, E_h, k_h, f_h, T_h, sensor, n_nodes, T_range, interp_tol, g=g_h,
                                    need_device=False)
    T_range = (front["T_lo"], front["T_hi"])  # explicit from here on: no read from the device
    tbl = c.table()
    dev = engine.device()
    E_d, k_d, f_d, T_d, g_d = (v.to(dev) for v in (E_h, k_h, f_h, T_h, g_h))
    kept = {}

    def sensor_stage(tau, Lu, Ld):
        t_, u_, d_ = tau[0, :nX].contiguous(), Lu[0, :nX].contiguous(), Ld[:nX].contiguous()
        _, kept["cube"] = _sensor.hsi_cube_srf(grid, t_, u_, d_, Xk, E_d, k_d, f_d, T_d, sensor, n_nodes=n_nodes, T_range=T_range,
                                               interp_tol=interp_tol)
        r = _sensor.hsi_cube_srf_vjp(grid, t_, u_, d_, Xk, E_d, k_d, f_d, T_d, sensor, g_d, n_nodes=n_nodes, T_range=T_range,
                                     interp_tol=interp_tol)
        kept.update({k: r[k] for k in ("Tpix", "frac", "endmembers")})
        return [r["G_tau"].reshape(1, 1, nX), r["G_La"].reshape(1, 1, nX), r["G_Ld"].reshape(1, nX)]

    _, _, _, _, grad = engine.tud_vjp(tbl, grid, c.Z, c.T, c.P, c.PL, c.MF, c.ID, Altitudes=c.Z_s, theta_r=c.theta,
                                      N_angle=c.N_angle, returnOD=False, wrt=wrt, layers=lay, fd_step_T=float(fd_step_T),
                                      cotangents=sensor_stage, dT_method=dT_method, continuum=cont, xs_lut=lut)
    out = _grad_dict(grad.cpu().numpy(), wrt, None)
    for k in ("Tpix", "frac", "endmembers"):
        out[k] = kept[k].cpu().numpy()
    return np.array(sensor.centres), kept["cube"].cpu().numpy(), out


def compute_hsi_cube_fit(Xmin, Xmax, sensor, Xk, endmembers, kidx, meas, T_range, frac0=None, T0=None, weights=None, max_iter=50,
                         lambda0=1e-3, ftol=0.0, opts=options, n_nodes=8, interp_tol=1e-6, nonneg=False, sum_weight=0.0, **kwargs):
    """Fit every pixel's surface temperature and fractions to a measured HSI cube under a known atmosphere, in one call: the
    line-sums and compute_TUD's tau / La / Ld, which stay on the device, then sensor.hsi_cube_srf_fit.

    sensor, Xk, endmembers [nk][nEnd] (float32), kidx [nPix][nMix] (integers): as compute_hsi_cube_vjp; meas [nB][nPix]
    (float32): the measured cube, laid out as hsi_cube_srf returns it; T_range = (T_lo, T_hi), required. frac0 [nPix][nMix]
    and T0 [nPix] (both or neither), weights [nB], max_iter, lambda0, ftol, n_nodes, interp_tol: as hsi_cube_srf_fit. NumPy
    arrays or torch tensors. kwargs as compute_TUD, with exactly one sensor altitude and one theta_r and returnOD=False.
    Returns (X_out, fit): sensor.centres and hsi_cube_srf_fit's dict as NumPy arrays ("Tpix", "frac", "cost", "n_iter",
    "status", "hess"). Arguments are checked before any device work. NotImplementedError: more than one altitude or theta_r,
    returnOD=True, save=True.
    nonneg=True, sum_weight: the fit inside the box T_range x frac >= 0 with an optional soft sum-to-one, as hsi_cube_srf_fit
    (DESIGN 4.28); the dict gains "grad" and "active". sum_weight > 0 without nonneg is a ValueError."""
    name = "compute_hsi_cube_fit"
    c = _Call(name, Xmin, Xmax, opts, kwargs)
    if c.returnOD:
        raise NotImplementedError(name + ": returnOD=True is not supported (the sensor stage takes transmittances)")
    if c.Z_s.size != 1 or c.theta.size != 1:
        raise NotImplementedError(name + ": exactly one sensor altitude and one theta_r per call (got %d, %d)" % (c.Z_s.size, c.theta.size))
    if c.o["save"]:
        raise NotImplementedError(name + ": save=True is not supported")
    from . import _lib, sensor as _sensor  # sensor.py imports this module

    def host(v, what, kinds, dtype):
        a = v.detach().cpu().numpy() if _is_torch(v) else np.asarray(v)
        if a.dtype.kind not in kinds:
            raise ValueError(name + ": %s has dtype %s" % (what, a.dtype))
        return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype))

    if T_range is None:
        raise ValueError(name + ": T_range=(T_lo, T_hi) is required (there is no Tpix to read it from)")
    if (frac0 is None) != (T0 is None):
        raise ValueError(name + ": frac0 and T0 come together (a start) or not at all (the node scan)")
    it_max = _lib.load().rtx_srf_pixel_cube_fit_max_iter()
    if int(max_iter) != max_iter or not 0 <= max_iter <= it_max:
        raise ValueError(name + ": max_iter=%r: an integer from 0 to %d" % (max_iter, it_max))
    for what, v in (("lambda0", lambda0), ("ftol", ftol)):
        if not (np.isfinite(v) and v >= 0.0):
            raise ValueError(name + ": %s=%r: finite and not negative" % (what, v))
    Xk = np.ascontiguousarray(np.asarray(Xk, dtype=np.float64).ravel())
    E_h, k_h, m_h = host(endmembers, "endmembers", "f", np.float32), host(kidx, "kidx", "iu", np.int32), host(meas, "meas", "f", np.float32)
    if k_h.dim() != 2:
        raise ValueError(name + ": kidx: integers [nPix][nMix >= 1], got shape %r" % (tuple(k_h.shape),))
    given = frac0 is not None
    f_h = host(frac0, "frac0", "f", np.float32) if given else torch.empty(tuple(k_h.shape), dtype=torch.float32)
    T_h = host(T0, "T0", "f", np.float64) if given else torch.empty((k_h.shape[0],), dtype=torch.float64)
    grid, nX = c.grid, c.X.size
    z = torch.zeros(nX, dtype=torch.float32)  # stands for tau, La, Ld in the checks
    _sensor._srf_cube_front(name, grid, z, z, z, Xk, E_h, k_h, f_h, T_h, sensor, n_nodes, T_range, interp_tol, need_device=False)
    w_h = _sensor._cube_fit_args(name, sensor, k_h, m_h, weights)
    nonneg, sum_weight = _sensor._cube_box_args(name, nonneg, sum_weight, k_h)
    tbl = c.table()
    dev = engine.device()
    run = engine.TudRunner(tbl, grid, c.Z, n_layers=c.T.size, Altitudes=c.Z_s, theta_r=c.theta, N_angle=c.N_angle, returnOD=False,
                           broadening=c.broadening, xs_lut=c.lut, continuum=c.continuum)
    tau, Lu, Ld = run.run(c.T, c.P, c.PL, c.MF, c.ID)
    t_, u_, d_ = tau[0, :nX].contiguous(), Lu[0, :nX].contiguous(), Ld[:nX].contiguous()
    r = _sensor.hsi_cube_srf_fit(grid, t_, u_, d_, Xk, E_h.to(dev), k_h.to(dev), m_h.to(dev), sensor, T_range,
                                 frac0=f_h.to(dev) if given else None, T0=T_h.to(dev) if given else None, weights=w_h, max_iter=int(max_iter),
                                 lambda0=float(lambda0), ftol=float(ftol), n_nodes=n_nodes, interp_tol=interp_tol, nonneg=nonneg,
                                 sum_weight=sum_weight)
    return np.array(sensor.centres), {k: v.cpu().numpy() for k, v in r.items()}


_SURFACE_TANGENTS = ("Ts_surface", "emis")


def compute_band_radiance_jvp(Xmin, Xmax, sensor, Xk, emis_knots, Ts_surface, tangents, opts=options, layers=None, fd_step_T=0.5,
                              dT_method="fd", continuum_derivatives=False, xs_derivatives=False, **kwargs):
    """At-sensor band radiances over a surface and their change along directions in the unknowns of a retrieval, in one
    call: compute_TUD_jvp's tangent rows of tau / La / Ld (engine.tud_jvp), which stay on the device as float32, fed to the
    sensor stage's tangent (sensor.band_radiance_srf_jvp), which adds the surface temperature and the emissivity knots. No
    Jacobian and nothing of size nX x nE is stored. With compute_band_radiance_vjp, J^T (J v) at the bands.

    sensor, Xk, emis_knots, Ts_surface as compute_band_radiance_vjp. tangents: a non-empty dict with keys among
      "T", a molecule id of MFs_ID   [n_layers] per layer of `layers` (default all), as compute_TUD_jvp takes them;
      "Ts_surface"                   shaped like Ts_surface [K];
      "emis"                         [nk][nE];
    each with an optional trailing axis of n_vec directions (they share everything up to the contraction; all entries must
    agree on it). A key left out does not move. With only surface keys no rtx_tud_jvp launch and no T -+ fd_step_T or
    species line-sum is made: the base state alone. kwargs, layers, fd_step_T, dT_method as compute_TUD_jvp, with exactly
    one sensor altitude and returnOD=False. Returns (X_out, L, dL):
      X_out  sensor.centres;
      L      float32 NumPy, bit-identical to compute_band_radiance_vjp's L;
      dL     float64 NumPy shaped like L, plus a trailing [n_vec] axis when the tangents have one; NaN where L is NaN.
    continuum=, continuum_derivatives: as compute_TUD_jacobian (refused unless continuum_derivatives=True; then OD is not
    linear in a mixing ratio, a species entry is the local derivative at the state per ppmv, and where a continuum
    component's interpolated sum is <= 0 its derivatives are 0: the kink of max(0, .) is given the value 0).
    xs_lut=, xs_derivatives: as compute_TUD_jacobian (refused unless xs_derivatives=True; then every column comes from the
    cross-section table, DESIGN 4.24, and a layer exactly on a T node takes the slope of the cell to its right, to its left
    on the last node).
    Arguments are checked before any device work. NotImplementedError: more than one altitude or theta_r, returnOD=True,
    broadening=, xs_lut= by default, reduce=."""
    name = "compute_band_radiance_jvp"
    c = _Call(name, Xmin, Xmax, opts, kwargs)
    if "reduce" in c.o:
        raise NotImplementedError(name + ": reduce= is not offered: the tangent is defined on the sensor's bands")
    lut = _no_xs_lut(c, xs_derivatives)
    cont = _derivative_continuum(c, continuum_derivatives)
    if c.returnOD:
        raise NotImplementedError(name + ": returnOD=True is not supported (the sensor stage takes transmittances)")
    if c.Z_s.size != 1:
        raise NotImplementedError(name + ": exactly one sensor altitude per call (got %d)" % c.Z_s.size)
    if not isinstance(tangents, dict) or not tangents:
        raise ValueError(name + ": tangents must be a non-empty dict with keys among \"T\", a molecule id of MFs_ID, %r"
                         % (_SURFACE_TANGENTS,))
    atm = {k: v for k, v in tangents.items() if not (isinstance(k, str) and k in _SURFACE_TANGENTS)}
    bad = [k for k in atm if k != "T" and (isinstance(k, bool) or not isinstance(k, (int, np.integer)))]
    if bad:
        raise ValueError(name + ": unknown tangent key %r (expected \"T\", a molecule id of MFs_ID, \"Ts_surface\" or \"emis\")" % (bad[0],))
    wrt = tuple(atm.keys())
    # a surface-only call has no wrt entry: the checks that do not concern wrt are run with a stand-in
    wrt_, lay, nX = _jacobian_args(name, Xmin, Xmax, c.o, wrt if wrt else ("T",), layers, None, fd_step_T if wrt else 1.0,
                                   host_result=False, dT_method=dT_method)
    wrt = wrt_ if wrt else ()
    _xs_axis(c, lut)
    Xk = np.ascontiguousarray(np.asarray(Xk, dtype=np.float64).ravel())
    scalar = np.ndim(Ts_surface) == 0
    Ts_s = np.atleast_1d(np.asarray(Ts_surface, dtype=np.float64))
    if Ts_s.ndim != 1 or Ts_s.size == 0 or not np.all(Ts_s > 0.0):
        raise ValueError(name + ": Ts_surface must be a positive scalar or a non-empty 1-D sequence of positive temperatures")
    if not _is_torch(emis_knots):
        emis_knots = np.asarray(emis_knots)
    if tuple(emis_knots.shape[:1]) != (Xk.size,) or len(emis_knots.shape) != 2 or emis_knots.shape[1] < 1:
        raise ValueError(name + ": emis_knots has shape %r, expected [%d][nE]" % (tuple(emis_knots.shape), Xk.size))
    nk, nE, nT = Xk.size, int(emis_knots.shape[1]), Ts_s.size
    n_vecs = set()
    V = None
    if atm:
        V, nv = _jvp_tangents(atm, lay.size, fn=name)
        n_vecs.add(nv)
    d_Ts = d_emis = None
    if "Ts_surface" in tangents:
        d_Ts = tangents["Ts_surface"]
        d_Ts = np.asarray(d_Ts.detach().cpu().numpy() if _is_torch(d_Ts) else d_Ts, dtype=np.float64)
        base = () if scalar else (nT,)
        got = _vector_axis(d_Ts, base)
        if got is None:
            raise ValueError(name + ": tangent \"Ts_surface\" has shape %r, expected %r (Ts_surface's shape) plus an optional "
                             "trailing vector axis" % (tuple(d_Ts.shape), base))
        if not np.isfinite(d_Ts).all():
            raise ValueError(name + ": tangent \"Ts_surface\" has non-finite entries")
        n_vecs.add(got[1])
    if "emis" in tangents:
        d_emis = tangents["emis"]
        if not _is_torch(d_emis):
            d_emis = np.asarray(d_emis)
        got = _vector_axis(d_emis, (nk, nE))
        if got is None:
            raise ValueError(name + ": tangent \"emis\" has shape %r, expected %r (emis_knots' shape) plus an optional trailing "
                             "vector axis" % (tuple(d_emis.shape), (nk, nE)))
        n_vecs.add(got[1])
    if len(n_vecs) != 1:
        raise ValueError(name + ": the tangents disagree on the vector axis: %r" % sorted(n_vecs, key=str))
    n_vec = n_vecs.pop()
    from . import sensor as _sensor  # sensor.py imports this module
    grid = c.grid
    assert c.X.size == nX
    tbl = c.table()
    dev = engine.device()
    E_d = _dev_f32(emis_knots, dev).contiguous()
    rows = {}
    if atm:
        tau, Lu, Ld, _, d = engine.tud_jvp(tbl, grid, c.Z, c.T, c.P, c.PL, c.MF, c.ID, V, Altitudes=c.Z_s, theta_r=c.theta,
                                           N_angle=c.N_angle, returnOD=False, wrt=wrt, layers=lay, fd_step_T=float(fd_step_T),
                                           dT_method=dT_method, continuum=cont, xs_lut=lut)
        # [n_vec][nX] float32 where rtx_tud_jvp wrote them, seen as [nX][n_vec]: no copy, no host round trip
        rows = dict(d_tau=d["tau"][:, 0, :nX].T, d_La=d["La"][:, 0, :nX].T, d_Ld=d["Ld"][:, :nX].T)
        if n_vec is None:
            rows = {k: v[:, 0] for k, v in rows.items()}
    else:  # the base state alone, exactly what compute_TUD runs
        T = np.ascontiguousarray(np.atleast_1d(c.T))
        run = engine.TudRunner(tbl, grid, np.atleast_1d(c.Z), n_layers=T.size, Altitudes=c.Z_s, theta_r=c.theta, N_angle=c.N_angle,
                               returnOD=False, continuum=cont, xs_lut=lut)
        tau, Lu, Ld = run.run(T, np.atleast_1d(c.P), np.atleast_1d(c.PL), c.MF.reshape(T.size, -1), c.ID)
    t_, u_, d_ = tau[0, :nX].contiguous(), Lu[0, :nX].contiguous(), Ld[:nX].contiguous()
    L, dL = _sensor.band_radiance_srf_jvp(grid, t_, u_, d_, Xk, E_d, float(Ts_s[0]) if scalar else Ts_s, sensor, d_Ts=d_Ts,
                                          d_emis=None if d_emis is None else _dev_f32(d_emis, dev), **rows)
    L_h = L.cpu().numpy()
    dL_h = np.ascontiguousarray(dL.to(torch.float64).cpu().numpy())
    return np.array(sensor.centres), L_h, dL_h


_CUBE_TANGENTS = ("Tpix", "frac", "endmembers")


def compute_hsi_cube_jvp(Xmin, Xmax, sensor, Xk, endmembers, kidx, frac, Tpix, tangents, opts=options, layers=None, fd_step_T=0.5,
                         dT_method="fd", continuum_derivatives=False, xs_derivatives=False, n_nodes=8, T_range=None, interp_tol=1e-6,
                         **kwargs):
    """The per-pixel HSI cube of a scene under any sensor and its change along directions in the unknowns of a retrieval,
    in one call: compute_TUD_jvp's tangent rows of tau / La / Ld (engine.tud_jvp), which stay on the device as float32, fed
    to the cube's tangent (sensor.hsi_cube_srf_jvp), which adds the pixels' temperatures and fractions and the endmember
    knots. No Jacobian and nothing of size nPix x nX is stored. With compute_hsi_cube_vjp, J^T (J v) on the cube.

    sensor, Xk, endmembers, kidx, frac, Tpix, n_nodes, T_range, interp_tol as compute_hsi_cube_vjp. tangents: a non-empty
    dict with keys among
      "T", a molecule id of MFs_ID   [n_layers] per layer of `layers` (default all), as compute_TUD_jvp takes them;
      "Tpix"                         [nPix] [K];
      "frac"                         [nPix][nMix];
      "endmembers"                   [nk][nEnd];
    each with an optional trailing axis of n_vec directions (all entries must agree on it). A key left out does not move.
    With only "Tpix" / "frac" / "endmembers" no rtx_tud_jvp launch and no T -+ fd_step_T or species line-sum is made: the
    base state alone. kwargs, layers, fd_step_T, dT_method as compute_TUD_jvp, with exactly one sensor altitude and
    returnOD=False. Returns (X_out, cube, d_cube):
      X_out   sensor.centres;
      cube    float32 NumPy [nB][nPix], bit-identical to compute_hsi_cube_vjp's cube;
      d_cube  float32 NumPy shaped like cube, plus a trailing [n_vec] axis when the tangents have one; NaN where cube is NaN.
    continuum=, continuum_derivatives, xs_lut=, xs_derivatives: as compute_band_radiance_vjp.
    Arguments are checked before any device work. NotImplementedError: more than one altitude or theta_r, returnOD=True,
    broadening=, xs_lut= or continuum= without their derivative flags, reduce=."""
    name = "compute_hsi_cube_jvp"
    c = _Call(name, Xmin, Xmax, opts, kwargs)
    if "reduce" in c.o:
        raise NotImplementedError(name + ": reduce= is not offered: the tangent is defined on the sensor's bands")
    lut = _no_xs_lut(c, xs_derivatives)
    cont = _derivative_continuum(c, continuum_derivatives)
    if c.returnOD:
        raise NotImplementedError(name + ": returnOD=True is not supported (the sensor stage takes transmittances)")
    if c.Z_s.size != 1:
        raise NotImplementedError(name + ": exactly one sensor altitude per call (got %d)" % c.Z_s.size)
    if not isinstance(tangents, dict) or not tangents:
        raise ValueError(name + ": tangents must be a non-empty dict with keys among \"T\", a molecule id of MFs_ID, %r" % (_CUBE_TANGENTS,))
    atm = {k: v for k, v in tangents.items() if not (isinstance(k, str) and k in _CUBE_TANGENTS)}
    bad = [k for k in atm if k != "T" and (isinstance(k, bool) or not isinstance(k, (int, np.integer)))]
    if bad:
        raise ValueError(name + ": unknown tangent key %r (expected \"T\", a molecule id of MFs_ID, \"Tpix\", \"frac\" or \"endmembers\")"
                         % (bad[0],))
    wrt = tuple(atm.keys())
    # a call without an atmospheric key has no wrt entry: the checks that do not concern wrt are run with a stand-in
    wrt_, lay, nX = _jacobian_args(name, Xmin, Xmax, c.o, wrt if wrt else ("T",), layers, None, fd_step_T if wrt else 1.0,
                                   host_result=False, dT_method=dT_method)
    wrt = wrt_ if wrt else ()
    _xs_axis(c, lut)
    from . import sensor as _sensor  # sensor.py imports this module

    def host(v, what, kinds, dtype):
        a = v.detach().cpu().numpy() if _is_torch(v) else np.asarray(v)
        if a.dtype.kind not in kinds:
            raise ValueError(name + ": %s has dtype %s" % (what, a.dtype))
        return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype))

    Xk = np.ascontiguousarray(np.asarray(Xk, dtype=np.float64).ravel())
    E_h, k_h = host(endmembers, "endmembers", "f", np.float32), host(kidx, "kidx", "iu", np.int32)
    f_h, T_h = host(frac, "frac", "f", np.float32), host(Tpix, "Tpix", "f", np.float64)
    z = torch.zeros(nX, dtype=torch.float32)  # stands for tau, La, Ld in the checks
    grid = c.grid
    assert c.X.size == nX
    front = _sensor._srf_cube_front(name, grid, z, z, z, Xk, E_h, k_h, f_h, T_h, sensor, n_nodes, T_range, interp_tol, need_device=False)
    T_range = (front["T_lo"], front["T_hi"])  # explicit from here on: no read from the device
    n_vecs = set()
    V = None
    if atm:
        V, nv = _jvp_tangents(atm, lay.size, fn=name)
        n_vecs.add(nv)
    own = {"Tpix": ("d_Tpix", T_h, np.float64), "frac": ("d_frac", f_h, np.float32), "endmembers": ("d_endmembers", E_h, np.float32)}
    d_own = {}
    for key, (arg, like, dtype) in own.items():
        if key not in tangents:
            continue
        d = host(tangents[key], "tangent \"%s\"" % key, "fiu", dtype)
        if _vector_axis(d, tuple(like.shape)) is None:
            raise ValueError(name + ": tangent \"%s\" has shape %r, expected %r plus an optional trailing vector axis"
                             % (key, tuple(d.shape), tuple(like.shape)))
        n_vecs.add(_vector_axis(d, tuple(like.shape))[1])
        d_own[arg] = d
    if len(n_vecs) != 1:
        raise ValueError(name + ": the tangents disagree on the vector axis: %r" % sorted(n_vecs, key=str))
    n_vec = n_vecs.pop()
    tbl = c.table()
    dev = engine.device()
    E_d, k_d, f_d, T_d = (v.to(dev) for v in (E_h, k_h, f_h, T_h))
    d_own = {k: v.to(dev) for k, v in d_own.items()}
    rows = {}
    if atm:
        tau, Lu, Ld, _, d = engine.tud_jvp(tbl, grid, c.Z, c.T, c.P, c.PL, c.MF, c.ID, V, Altitudes=c.Z_s, theta_r=c.theta,
                                           N_angle=c.N_angle, returnOD=False, wrt=wrt, layers=lay, fd_step_T=float(fd_step_T),
                                           dT_method=dT_method, continuum=cont, xs_lut=lut)
        # [n_vec][nX] float32 where rtx_tud_jvp wrote them, seen as [nX][n_vec]: no copy, no host round trip
        rows = dict(d_tau=d["tau"][:, 0, :nX].T, d_La=d["La"][:, 0, :nX].T, d_Ld=d["Ld"][:, :nX].T)
        if n_vec is None:
            rows = {k: v[:, 0] for k, v in rows.items()}
    else:  # the base state alone, exactly what compute_TUD runs
        T = np.ascontiguousarray(np.atleast_1d(c.T))
        run = engine.TudRunner(tbl, grid, np.atleast_1d(c.Z), n_layers=T.size, Altitudes=c.Z_s, theta_r=c.theta, N_angle=c.N_angle,
                               returnOD=False, continuum=cont, xs_lut=lut)
        tau, Lu, Ld = run.run(T, np.atleast_1d(c.P), np.atleast_1d(c.PL), c.MF.reshape(T.size, -1), c.ID)
    t_, u_, d_ = tau[0, :nX].contiguous(), Lu[0, :nX].contiguous(), Ld[:nX].contiguous()
    _, cube, d_cube = _sensor.hsi_cube_srf_jvp(grid, t_, u_, d_, Xk, E_d, k_d, f_d, T_d, sensor, n_nodes=n_nodes, T_range=T_range,
                                               interp_tol=interp_tol, **rows, **d_own)
    return np.array(sensor.centres), cube.cpu().numpy(), np.ascontiguousarray(d_cube.cpu().numpy())


def compute_LWIR_apparent_radiance(X, emis, Ts, tau, La, Ld, dT=None, return_Ls=False):
    r"""L = tau [emis B(Ts + dT) + (1 - emis) Ld] + La for every combination, signature of :1017-1069.

    X (nX,), emis (nX,nE), Ts (nA,), tau/La/Ld (nX,nA), dT (nT,) optional ->
    L (nX,nE,nA) or (nX,nE,nA,nT) [, Ls]. Computed in float32 (the reference's own caller casts its
    inputs to float32 first, Compute_LWIR_Apparent_Radiance.py:9-20); NumPy in -> same dtype as `emis` out.
    """
    as_torch = any(_is_torch(v) for v in (X, emis, Ts, tau, La, Ld))
    dev = engine.device()
    Xd = _dev_f64(X, dev).flatten()
    em = _dev_f32(emis, dev)
    Tsd = _dev_f64(Ts, dev).flatten()
    nX, nA = Xd.numel(), Tsd.numel()
    td, Lad, Ldd = (_dev_f32(v, dev).reshape(nX, nA) for v in (tau, La, Ld))
    dTd = _dev_f64(np.asarray(dT).flatten() if not _is_torch(dT) else dT.flatten(), dev) if dT is not None else None
    L, Ls = engine.apparent_radiance(Xd, em.reshape(nX, -1), Tsd, td, Lad, Ldd, dTd, return_Ls)
    if dT is None:
        L = L[..., 0]
        Ls = Ls[..., 0] if Ls is not None else None
    if not as_torch:
        odt = np.asarray(emis).dtype if np.asarray(emis).dtype in (np.float32, np.float64) else np.float64
        L = L.cpu().numpy().astype(odt, copy=False)
        Ls = Ls.cpu().numpy().astype(odt, copy=False) if Ls is not None else None
    return (L, Ls) if return_Ls else L


# 128 MAKO band centres [um] -- instrument constants listed at :1092-1223
_MAKO_UM = np.array([
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


def _ils_apply(kind, X, Y, centre, sigma):
    """Shared device path of both ILS variants: Y (nX,) or (nX,nS) -> (nB,) or (nB,nS)."""
    as_torch = _is_torch(Y)
    dev = engine.device()
    Yd = _dev_f32(Y, dev)
    one_d = Yd.dim() == 1
    if one_d:
        Yd = Yd[:, None].contiguous()
    Xh = X.detach().cpu().numpy() if _is_torch(X) else np.asarray(X, dtype=np.float64)
    try:
        grid, Xd = engine.Grid.from_axis(Xh), None
    except NotImplementedError:
        grid, Xd = None, _dev_f64(Xh, dev)  # explicit (non-uniform) ascending axis
    out = engine.ils(kind, Yd, _dev_f64(centre, dev), _dev_f64(sigma, dev), X=Xd, grid=grid)
    if one_d:
        out = out[:, 0]
    if as_torch:
        return out
    odt = np.asarray(Y).dtype if np.asarray(Y).dtype in (np.float32, np.float64) else np.float64
    return out.cpu().numpy().astype(odt)


def ILS_MAKO(X, Y, resFactor=None, returnX=True, fwhm_sf=1.0, shift=0.0, scale=1.0):
    """MAKO instrument line shape (triangle), signature of :1072-1263.

    X (nX,) ascending wavenumbers, Y (nX,) or (nX,nS) -> X_out (nB,), Y_out (nB,) or (nB,nS);
    nB = 128 (or int(128*resFactor)) minus the bands outside the open interval (X.min, X.max) (:1233).
    A band whose triangle covers no grid point comes out NaN, as in the reference (quirk 13)."""
    Xh = X.detach().cpu().numpy() if _is_torch(X) else np.asarray(X, dtype=np.float64)
    X_out = _MAKO_UM.copy()
    if resFactor is not None:
        _x0 = np.linspace(0, 1, len(X_out))
        _x1 = np.linspace(0, 1, int(len(X_out) * resFactor))
        X_out = np.interp(_x1, _x0, X_out)
    X_out = np.sort(10000.0 / X_out)
    X_out = X_out[(X_out > Xh.min()) & (X_out < Xh.max())]
    sigma_out = fwhm_sf * np.abs(np.gradient(X_out)) * 1.6
    Y_out = _ils_apply(0, Xh, Y, scale * X_out + shift, sigma_out)
    if returnX:
        return X_out, Y_out
    return Y_out


def apply_sensor(X, Y, sensor, returnX=True):
    """Band averages under a sensor's tabulated spectral response functions (sensor.Sensor), with ILS_MAKO's conventions:
    X (nX,) ascending wavenumbers, Y (nX,) or (nX,nS), NumPy or torch -> X_out (nB,) NumPy = sensor.centres and Y_out (nB,) or
    (nB,nS) of Y's kind (NumPy: Y's float dtype; torch: a float32 device tensor). A uniform axis goes to the library as a grid,
    any other ascending axis as it is. A band with no point of X under it comes out NaN."""
    from . import sensor as _sensor  # sensor.py imports this module
    as_torch = _is_torch(Y)
    dev = engine.device()
    Yd = _dev_f32(Y, dev)
    one_d = Yd.dim() == 1
    if one_d:
        Yd = Yd[:, None].contiguous()
    Xh = np.asarray(X.detach().cpu().numpy() if _is_torch(X) else X, dtype=np.float64).ravel()
    try:
        grid, Xd = engine.Grid.from_axis(Xh), None
    except (NotImplementedError, ValueError):
        grid, Xd = None, _dev_f64(Xh, dev)  # explicit axis: non-uniform, or a single point
    X_out, out = _sensor.apply_srf(sensor, Yd, grid=grid, X=Xd)
    if one_d:
        out = out[:, 0]
    if not as_torch:
        odt = np.asarray(Y).dtype if np.asarray(Y).dtype in (np.float32, np.float64) else np.float64
        out = out.cpu().numpy().astype(odt)
    return (X_out, out) if returnX else out


# ---- post-processing of TUD products ----------------------------------------
def _uniform_axis(X, what):
    Xh = X.detach().cpu().numpy() if _is_torch(X) else np.asarray(X, dtype=np.float64)
    Xh = np.asarray(Xh, dtype=np.float64).ravel()
    if Xh.size < 2:
        raise ValueError(f"{what}: X needs at least two points")
    h = (Xh[-1] - Xh[0]) / (Xh.size - 1)
    if not np.allclose(np.diff(Xh), h, rtol=0, atol=1e-6 * abs(h)):
        raise NotImplementedError(f"{what}: only uniform spectral axes are supported")
    return Xh, float(h)


def smooth(x, window_len=11, window="hanning"):
    """Window smoothing, signature and early returns of :1266-1324 (1-D input only; reflect-padded, output of the
    same length; an even window_len leaves the result half a sample off centre, as in the reference)."""
    x = np.asarray(x)
    if x.ndim != 1:
        print("smooth only accepts 1 dimension arrays.")
        return x
    if x.size < window_len:
        print("Input vector needs to be bigger than window size.")
        return x
    if window_len < 3:
        return x
    if window not in engine._WINDOWS:
        print("Window is on of 'flat', 'hanning', 'hamming', 'bartlett', 'blackman'")
        return x
    engine.require_gpu()
    taps, c = engine.window_taps(window_len, window)
    Y = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)[None, :], device="cuda")
    return engine.fir_reflect(Y, taps, c)[0].cpu().numpy()


def reduceResolution(X, Y, dX, N=4, window="hanning", X_out=None):
    """Smooth to resolution dX and resample, signature of :1327-1350: X (nX,) uniform, Y (nX,) or (nX, nC)
    -> (X_out, Y_out) when X_out is None, else Y_out; Y_out (nOut,) or (nOut, nC), float64.

    The reference smooths with window length round(dX / mean(diff(X))) (forward and reversed, averaged), then puts
    scipy's cubic interp1d through all smoothed samples. Here: one fp64 FIR kernel and one cardinal-spline kernel.
    Conscious divergences: (1) nPts = ceil(N*span/dX)+1 is evaluated with a 1e-9 guard, because N*span/dX is normally
    an exact integer and the reference's value flips between two counts with the rounding of its convolution;
    (2) np.int (:1329,1336) is int; (3) X_out must be ascending when it reaches within ceil(window/2) + 20 samples of an
    end of the axis, and must not leave the smoothed axis (interp1d's extrapolation is not reproduced). Output points near
    the ends -- where the reference's knots are the SMOOTHED, no longer uniform axis and its not-a-knot end condition acts --
    are evaluated by a local not-a-knot spline on those knots (rtx_cubic_end), so short windows work with the default X_out.
    An axis so short that this local spline covers all of it (n <= 2 ceil(window/2) + 46 samples) is one spline with the
    not-a-knot condition at both ends, the reference's own, for every output point. X_out may overshoot the first or last
    smoothed knot by 1e-9 of a sample spacing: the knots computed here and the reference's sm(X) differ in the last bit, so
    an X_out that starts or ends on the reference's own end knots is accepted."""
    Xh, h = _uniform_axis(X, "reduceResolution")
    engine.require_gpu()
    Yt = Y if _is_torch(Y) else torch.as_tensor(np.asarray(Y, dtype=np.float64))
    one_d = Yt.dim() == 1
    Y2 = (Yt[None, :] if one_d else Yt.transpose(0, 1)).to("cuda").contiguous()
    if Y2.shape[1] != Xh.size:
        raise ValueError("reduceResolution: Y's first axis must match X")
    if Y2.dtype not in (torch.float32, torch.float64):
        Y2 = Y2.to(torch.float64)
    x_out, out = engine.reduce_resolution(Y2, float(Xh[0]), h, Xh.size, float(dX), N=N, window=window,
                                          x_out=None if X_out is None else np.asarray(X_out, dtype=np.float64).ravel())
    Y_out = out[0].cpu().numpy() if one_d else out.transpose(0, 1).contiguous().cpu().numpy()
    if X_out is None:
        return x_out, Y_out
    return Y_out


# ---- small host helpers of the reference module, kept for drop-in completeness -------------------------
def rs1D(y):
    """(flattened copy, original shape), as radiative_transfer.py:186-203."""
    y = np.array(y)
    return y.flatten(), y.shape


def rs2D(y):
    """(2-D view with the 2nd..Nth axes flattened, original shape); a scalar or 1-D input becomes one row
    (radiative_transfer.py:206-228)."""
    y = np.array(y)
    if y.ndim < 2:
        y = np.array([y]).flatten()[np.newaxis, :]
        return y, y.shape
    dims = y.shape
    return y.reshape((dims[0], int(np.prod(dims[1:])))), dims


def rsND(y, dims):
    """Back to the N-D shape (radiative_transfer.py:231-248)."""
    return y.reshape(dims)


def _no_lblrtm(name):
    def stub(*args, **kwargs):
        raise NotImplementedError(
            f"{name}: the LBLRTM plumbing of the reference (TAPE5 writer, binary runner, TAPE12 reader; "
            "radiative_transfer.py:395-789) is not part of this engine -- the LBLRTM executable and the AER line file are "
            "git-LFS stubs in the reference checkout. compute_OD / compute_TUD take a HITRAN-format line table instead "
            "(line_table=..., INTEGRATION.md section 2).")
    stub.__name__ = name
    return stub


write_tape5 = _no_lblrtm("write_tape5")
run_LBLRTM = _no_lblrtm("run_LBLRTM")
read_tape12 = _no_lblrtm("read_tape12")
