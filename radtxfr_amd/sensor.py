"""At-sensor band radiances on device tensors: the C4 pipeline of SURVEY.md 8d
(emissivity knots -> monochromatic grid -> compute_LWIR_apparent_radiance -> ILS_MAKO) without ever
leaving the GPU. The reference runs these steps as separate scripts on band-averaged TUDs
(Compute_LWIR_Apparent_Radiance.py:25 on the output of Generate_LWIR_TUD_MAKO.py:34-36) because its
ILS needs an (nS,nX,nB) temporary (1.4 TB at 2000 spectra); here the monochromatic arrays fit in HBM
(560 k wavenumbers x 2000 spectra x 4 B = 4.5 GB) and the order "radiance first, ILS second" is exact.
"""
import ctypes as C
import functools
import threading

import numpy as np
import torch

from . import _lib, engine
from .radiative_transfer import _MAKO_UM, c1 as _C1, c2 as _C2


def interp_knots(grid, Xk, F):
    """np.interp(grid, Xk, F[:, s]) for every column: F [nk][nS] float32 device -> [grid.n][nS] float32."""
    lib = _lib.load()
    assert F.dtype == torch.float32 and F.is_cuda and F.dim() == 2
    F = F.contiguous()
    Xk_d = torch.as_tensor(np.asarray(Xk, dtype=np.float64), device=F.device).contiguous()
    out = torch.empty((grid.n, F.shape[1]), dtype=torch.float32, device=F.device)
    _lib.check(lib.rtx_interp_knots(grid.byref(), None, grid.n, C.c_void_p(Xk_d.data_ptr()), Xk_d.numel(),
                                    C.c_void_p(F.data_ptr()), F.shape[1], C.c_void_p(out.data_ptr()),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def mako_bands(x_min, x_max, resFactor=None, fwhm_sf=1.0, shift=0.0, scale=1.0):
    """Band axis, centres and triangle widths of rt.ILS_MAKO (radiative_transfer.py:1226-1241)."""
    X_out = _MAKO_UM.copy()
    if resFactor is not None:
        X_out = np.interp(np.linspace(0, 1, int(len(X_out) * resFactor)), np.linspace(0, 1, len(X_out)), X_out)
    X_out = np.sort(10000.0 / X_out)
    X_out = X_out[(X_out > x_min) & (X_out < x_max)]
    sigma = fwhm_sf * np.abs(np.gradient(X_out)) * 1.6
    return X_out, scale * X_out + shift, sigma


_CUBE_PLANS = {}  # spectra-independent set-up of hsi_cube (band list, knots and node tables on the device), a few entries
_CUBE_PLANS_MAX = 8
_CUBE_PLANS_LOCK = threading.Lock()
_FUSED_PLANS = {}  # band list and knot axis of band_radiance_fused on the device (a few entries, see _cube_plan)


MAX_KNOTS = 1024  # per response table: rtx_srf_max_knots() of the library (tests/test_srf_host.py compares the two)


def trapezoid_cells(X):
    """The trapezoid cell of every point of the axis X, as rtx_srf_apply weighs it: (X[i+1] - X[i-1]) / 2 inside, half the
    distance to its one neighbour at either end, 1 for a one-point axis."""
    X = np.asarray(X, dtype=np.float64).ravel()
    if X.size == 1:
        return np.ones(1)
    d = np.empty(X.size)
    d[1:-1] = 0.5 * (X[2:] - X[:-2])
    d[0], d[-1] = 0.5 * (X[1] - X[0]), 0.5 * (X[-1] - X[-2])
    return d


def _table_centre(x, r):
    """Response-weighted mean wavenumber of a piecewise-linear table: int x R dx / int R dx, exact."""
    h, r0, r1 = np.diff(x), r[:-1], r[1:]
    den = np.sum(h * (r0 + r1)) / 2.0
    num = np.sum(h * (x[:-1] * (2.0 * r0 + r1) + x[1:] * (r0 + 2.0 * r1))) / 6.0
    return num / den


class Sensor:
    """An immutable set of bands, each a tabulated relative spectral response function: knots (x_j, r_j) on a wavenumber
    axis [cm^-1], x strictly ascending, r finite and >= 0. Between the knots the response is linear, outside them 0 (both end
    knots included: two knots of value 1 are a boxcar); include/radtxfr_hip.h, rtx_srf_apply, has the band average.

    tables: tuple of (x, r) read-only arrays (float64, float32). centres [nB]: what apply_srf returns as X_out, by default
    each table's response-weighted mean wavenumber. The concatenated knots go to a device once, on first use there."""

    def __init__(self, tables, centres):
        self.tables = tuple(tables)
        self.centres = centres
        self.knot_start = np.zeros(len(self.tables) + 1, dtype=np.int32)
        self.knot_start[1:] = np.cumsum([x.size for x, _ in self.tables])
        for a in (self.centres, self.knot_start):
            a.setflags(write=False)
        self._dev = {}
        self._lock = threading.Lock()

    def __len__(self):
        return len(self.tables)

    @classmethod
    def from_tables(cls, tables, centres=None):
        """tables: a list of (x_knots, response) pairs, one per band. Raises ValueError, naming the band, for knots that do
        not ascend strictly, a negative or non-finite response, a response that is zero everywhere, and fewer than 2 or
        more than MAX_KNOTS knots."""
        out = []
        for b, (x, r) in enumerate(tables):
            x = np.array(x, dtype=np.float64).ravel()
            r = np.array(r, dtype=np.float64).ravel()
            if x.size != r.size:
                raise ValueError(f"band {b}: {x.size} knots but {r.size} responses")
            if x.size < 2 or x.size > MAX_KNOTS:
                raise ValueError(f"band {b}: {x.size} knots, a response table needs 2 to {MAX_KNOTS}")
            if not np.all(np.isfinite(x)) or not np.all(np.diff(x) > 0):
                raise ValueError(f"band {b}: the knots must be finite and strictly ascending")
            if not np.all(np.isfinite(r)) or np.any(r < 0):
                raise ValueError(f"band {b}: the response must be finite and >= 0")
            r32 = r.astype(np.float32)
            if not np.any(r32 > 0):
                raise ValueError(f"band {b}: the response is zero everywhere")
            x.setflags(write=False), r32.setflags(write=False)
            out.append((x, r32))
        if centres is None:
            centres = np.array([_table_centre(x, r.astype(np.float64)) for x, r in out], dtype=np.float64)
        else:
            centres = np.array(centres, dtype=np.float64).ravel()
            if centres.size != len(out):
                raise ValueError(f"{centres.size} centres for {len(out)} bands")
        return cls(out, centres)

    @classmethod
    def from_shape(cls, centres, fwhm, shape, knots=65):
        """Bands of one analytic shape, tabulated on the host: "triangle" (3 knots, exact: base centre -+ fwhm), "boxcar"
        (2 knots, exact: centre -+ fwhm / 2) or "gaussian" (`knots` points out to -+ 4 fwhm; an odd count puts one on the
        peak). fwhm: one width or one per band."""
        c = np.atleast_1d(np.asarray(centres, dtype=np.float64)).ravel()
        f = np.broadcast_to(np.asarray(fwhm, dtype=np.float64), c.shape)
        if np.any(~(f > 0)):
            raise ValueError("fwhm must be positive")
        if shape == "triangle":
            tables = [(np.array([ci - fi, ci, ci + fi]), np.array([0.0, 1.0, 0.0])) for ci, fi in zip(c, f)]
        elif shape == "boxcar":
            tables = [(np.array([ci - 0.5 * fi, ci + 0.5 * fi]), np.array([1.0, 1.0])) for ci, fi in zip(c, f)]
        elif shape == "gaussian":
            tables = []
            for ci, fi in zip(c, f):
                d = np.linspace(-4.0 * fi, 4.0 * fi, int(knots))
                tables.append((ci + d, np.exp(-4.0 * np.log(2.0) * (d / fi) ** 2)))
        else:
            raise ValueError(f"shape {shape!r}: triangle, gaussian or boxcar")
        return cls.from_tables(tables, centres=c)

    @classmethod
    def mako(cls, x_min, x_max, resFactor=None, fwhm_sf=1.0, shift=0.0, scale=1.0):
        """mako_bands()'s triangles as 3-knot tables (c - sigma, 0), (c, 1), (c + sigma, 0), c = scale * X_out + shift."""
        _, c, s = mako_bands(x_min, x_max, resFactor, fwhm_sf, shift, scale)
        return cls.from_tables([(np.array([ci - si, ci, ci + si]), np.array([0.0, 1.0, 0.0])) for ci, si in zip(c, s)])

    @classmethod
    def in_wavelength(cls, tables_um, centres=None):
        """Tables given on a wavelength axis [um], in either order: the knots become wavenumbers 1e4 / um in ascending
        order. The response values are kept as they are, per unit wavenumber: NO Jacobian factor is applied, so a
        response measured per unit wavelength has to be converted by the caller. centres, if given, are wavenumbers."""
        out = []
        for lam, r in tables_um:
            x = 1.0e4 / np.asarray(lam, dtype=np.float64).ravel()
            order = np.argsort(x, kind="stable")
            out.append((x[order], np.asarray(r, dtype=np.float64).ravel()[order]))
        return cls.from_tables(out, centres=centres)

    def on_device(self, dev):
        """(knot_x fp64, knot_r fp32): all bands' knots concatenated, as device tensors cached per device."""
        key = str(torch.device(dev))
        with self._lock:
            hit = self._dev.get(key)
            if hit is None:
                kx = np.concatenate([x for x, _ in self.tables]) if self.tables else np.zeros(0)
                kr = np.concatenate([r for _, r in self.tables]) if self.tables else np.zeros(0, dtype=np.float32)
                hit = self._dev[key] = (torch.as_tensor(kx, device=dev), torch.as_tensor(kr, device=dev))
        return hit


def apply_srf(sensor, Y, grid=None, X=None, wsum=False):
    """Band averages of Y [nx][nS] float32 (device, rows contiguous) under the sensor's response tables (rtx_srf_apply):
    grid = the uniform engine.Grid of the axis, or X = an explicit ascending fp64 device axis. Returns (X_out [nB] NumPy =
    sensor.centres, Y_out [nB][nS] float32 device); with wsum=True also the denominators [nB] float32 device. A band with
    no axis point under it comes out NaN."""
    lib = _lib.load()
    assert Y.dtype == torch.float32 and Y.is_cuda and Y.dim() == 2 and (Y.stride(1) == 1 or Y.shape[1] <= 1)
    if (grid is None) == (X is None):
        raise ValueError("apply_srf needs the axis either as grid= or as X=")
    nx, nS = Y.shape
    if nx != (grid.n if X is None else X.numel()):
        raise ValueError(f"Y has {nx} rows, the axis {grid.n if X is None else X.numel()} points")
    if X is not None:
        assert X.dtype == torch.float64 and X.device == Y.device and X.is_contiguous()
    nB = len(sensor)
    kx, kr = sensor.on_device(Y.device)
    out = torch.empty((nB, nS), dtype=torch.float32, device=Y.device)
    den = torch.empty(nB, dtype=torch.float32, device=Y.device) if wsum else None
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    _lib.check(lib.rtx_srf_apply(grid.byref() if X is None else None, p(X), nx, p(Y), nS, Y.stride(0) if nx > 1 else max(nS, 1), nB,
                                 sensor.knot_start.ctypes.data_as(C.c_void_p), p(kx), p(kr), p(out), p(den),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    X_out = np.array(sensor.centres)
    return (X_out, out, den) if wsum else (X_out, out)


def band_radiance_srf(grid, tau, La, Ld, Xk, emis_knots, Ts, sensor, keep_hires=False):
    """band_radiance() for any sensor: L_b,k = SRF_b( tau*(eps_k*B(Ts) + (1-eps_k)*Ld) + La ) for every emissivity column k,
    the band average under the sensor's tabulated responses instead of the MAKO triangle. Same arguments as band_radiance()
    with a Sensor in place of resFactor. Returns (X_out [nB] NumPy, L [nB][nE] float32 device). Three streaming kernels:
    rtx_interp_knots -> rtx_apparent_radiance -> rtx_srf_apply."""
    dev = tau.device
    em = interp_knots(grid, Xk, emis_knots)  # [nX][nE]
    X_d = torch.as_tensor(grid.axis(), device=dev)
    Ts_d = torch.as_tensor(np.atleast_1d(np.asarray(Ts, dtype=np.float64)), device=dev)
    col = lambda v: v.reshape(-1, 1).contiguous()
    L, _ = engine.apparent_radiance(X_d, em, Ts_d, col(tau), col(La), col(Ld))
    L = L.reshape(grid.n, -1)  # [nX][nE] (nA = nT = 1)
    X_out, out = apply_srf(sensor, L, grid=grid)
    return (X_out, out, L) if keep_hires else (X_out, out)


def _fused_plan(grid, Xk, resFactor, kind, dev):
    Xk = np.ascontiguousarray(Xk, dtype=np.float64)
    key = (grid.x_at(0), grid.step, grid.n, resFactor, int(kind), str(dev), Xk.tobytes())
    with _CUBE_PLANS_LOCK:
        plan = _FUSED_PLANS.get(key)
    if plan is None:
        if kind == 0:
            X_out, centre, sigma = mako_bands(grid.x_at(0), grid.x_at(grid.n - 1), resFactor)
        else:  # Gaussian variant: no clipping, sigma = |gradient| (ILS_MAKO.py:19-21)
            X_out = np.sort(10000.0 / _MAKO_UM)
            centre, sigma = X_out, np.abs(np.gradient(X_out))
        plan = {"X_out": np.array(X_out, dtype=np.float64), "Xk_d": torch.as_tensor(Xk, device=dev),
                "c_d": torch.as_tensor(np.ascontiguousarray(centre, dtype=np.float64), device=dev),
                "s_d": torch.as_tensor(np.ascontiguousarray(sigma, dtype=np.float64), device=dev)}
        with _CUBE_PLANS_LOCK:
            if len(_FUSED_PLANS) >= _CUBE_PLANS_MAX:
                _FUSED_PLANS.pop(next(iter(_FUSED_PLANS)))
            _FUSED_PLANS[key] = plan
    return plan


def band_radiance_fused(grid, tau, La, Ld, Xk, emis_knots, Ts, resFactor=None, kind=0):
    """Same result as band_radiance() without any [nX][nE] array: one monochromatic pass
    (rtx_band_moments) + a [nB x nk] x [nk x nE] contraction over each band's ~10-30 knots (rtx_band_mix).
    Returns (X_out [nB] NumPy, L [nB][nE] float32 device)."""
    lib = _lib.load()
    dev = tau.device
    plan = _fused_plan(grid, Xk, resFactor, kind, dev)
    X_out = plan["X_out"].copy()
    nB, nk, nE = X_out.size, len(Xk), emis_knots.shape[1]
    assert emis_knots.dtype == torch.float32 and emis_knots.shape[0] == nk
    emis_knots = emis_knots.contiguous()
    N = torch.empty(nB, dtype=torch.float32, device=dev)
    Cb = torch.empty(nB, dtype=torch.float32, device=dev)
    M = torch.empty((nB, nk), dtype=torch.float32, device=dev)
    jr = torch.empty((nB, 2), dtype=torch.int32, device=dev)
    out = torch.empty((nB, nE), dtype=torch.float32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.rtx_band_moments(int(kind), grid.byref(), p(tau), p(La), p(Ld), float(Ts), p(plan["Xk_d"]), nk, nB, p(plan["c_d"]),
                                    p(plan["s_d"]), p(N), p(Cb), p(M), p(jr), st))
    _lib.check(lib.rtx_band_mix(p(N), p(Cb), p(M), p(jr), nB, nk, p(emis_knots), nE, p(out), st))
    return X_out, out


_SRF_FUSED_PLANS = {}  # (Xk bytes, device) -> the knot axis on the device, for band_radiance_srf_fused (see _fused_plan)


def _srf_fused_plan(Xk, dev):
    Xk = np.array(Xk, dtype=np.float64).ravel()  # a copy: the caller's array may be read-only
    key = (str(dev), Xk.tobytes())
    with _CUBE_PLANS_LOCK:
        plan = _SRF_FUSED_PLANS.get(key)
    if plan is None:
        plan = {"Xk_d": torch.as_tensor(Xk, device=dev)}
        with _CUBE_PLANS_LOCK:
            if len(_SRF_FUSED_PLANS) >= _CUBE_PLANS_MAX:
                _SRF_FUSED_PLANS.pop(next(iter(_SRF_FUSED_PLANS)))
            _SRF_FUSED_PLANS[key] = plan
    return plan


def srf_moments(grid, tau, La, Ld, Xk_d, Ts, sensor):
    """rtx_srf_moments for up to rtx_srf_moments_max_temps() temperatures Ts (a sequence): (N [nB], C [nB], M [nT][nB][nk]
    float32, jrange [nB][2] int32) on tau's device, what rtx_band_mix takes. Xk_d: the fp64 knot axis on that device."""
    lib = _lib.load()
    dev = tau.device
    for v in (tau, La, Ld):
        assert v.dtype == torch.float32 and v.is_cuda and v.is_contiguous() and v.numel() == grid.n
    Ts = np.ascontiguousarray(np.atleast_1d(np.asarray(Ts, dtype=np.float64)))
    nB, nk, nT = len(sensor), Xk_d.numel(), Ts.size
    kx, kr = sensor.on_device(dev)
    N = torch.empty(nB, dtype=torch.float32, device=dev)
    Cb = torch.empty(nB, dtype=torch.float32, device=dev)
    M = torch.empty((nT, nB, nk), dtype=torch.float32, device=dev)
    jr = torch.empty((nB, 2), dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(lib.rtx_srf_moments(grid.byref(), p(tau), p(La), p(Ld), Ts.ctypes.data_as(C.c_void_p), nT, p(Xk_d), nk, nB,
                                   sensor.knot_start.ctypes.data_as(C.c_void_p), p(kx), p(kr), p(N), p(Cb), p(M), p(jr),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return N, Cb, M, jr


def band_radiance_srf_fused(grid, tau, La, Ld, Xk, emis_knots, Ts, sensor):
    """band_radiance_srf() without any [nX][nE] array, for one surface temperature or many: one pass over tau / La / Ld
    per group of 16 bands (rtx_srf_moments; Planck evaluated at every point for every temperature) and one contraction
    over each band's emissivity knots per temperature (rtx_band_mix). Same arguments as band_radiance_srf(); Ts may be a
    sequence (the reference's Ts + dT: Ts=Ts0 + np.asarray(dT)), taken rtx_srf_moments_max_temps() at a time.
    Returns (X_out [nB] NumPy = sensor.centres, L float32 device: [nB][nE] for a scalar Ts, [nT][nB][nE] for a 1-D Ts).
    Allocated besides L: the moments M [nT][nB][nk] float32 (N, C [nB], jrange [nB][2]), nothing of size nX."""
    lib = _lib.load()
    dev = tau.device
    scalar = np.ndim(Ts) == 0
    Ts = np.atleast_1d(np.asarray(Ts, dtype=np.float64))
    if Ts.ndim != 1 or Ts.size == 0:
        raise ValueError("Ts: a scalar or a non-empty 1-D sequence")
    plan = _srf_fused_plan(Xk, dev)
    nB, nk, nE, nT = len(sensor), plan["Xk_d"].numel(), emis_knots.shape[1], Ts.size
    assert emis_knots.dtype == torch.float32 and emis_knots.is_cuda and emis_knots.shape[0] == nk
    emis_knots = emis_knots.contiguous()
    out = torch.empty((nT, nB, nE), dtype=torch.float32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    step = lib.rtx_srf_moments_max_temps()
    for t0 in range(0, nT, step):
        N, Cb, M, jr = srf_moments(grid, tau, La, Ld, plan["Xk_d"], Ts[t0:t0 + step], sensor)
        for t in range(M.shape[0]):
            _lib.check(lib.rtx_band_mix(p(N), p(Cb), p(M[t]), p(jr), nB, nk, p(emis_knots), nE, p(out[t0 + t]), st))
    X_out = np.array(sensor.centres)
    return X_out, (out[0] if scalar else out)


def srf_norms(grid, sensor, dev=None):
    """The denominators N [nB] float32 (device) of the sensor's bands on `grid`, as rtx_srf_radiance_vjp forms them
    (rtx_srf_norms): bit for bit rtx_srf_moments' N."""
    lib = _lib.load()
    dev = engine.device() if dev is None else dev
    kx, kr = sensor.on_device(dev)
    N = torch.empty(len(sensor), dtype=torch.float32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(lib.rtx_srf_norms(grid.byref(), len(sensor), sensor.knot_start.ctypes.data_as(C.c_void_p), p(kx), p(kr), p(N),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return N


_VJP_OUTPUTS = ("G_tau", "G_La", "G_Ld", "Ts", "emis")


def band_radiance_srf_vjp(grid, tau, La, Ld, Xk, emis_knots, Ts, sensor, g, outputs=_VJP_OUTPUTS):
    """The adjoint of band_radiance_srf_fused (rtx_srf_radiance_vjp): from g = d cost / d L, laid out like the L that call
    returns ([nB][nE] for a scalar Ts, [nT][nB][nE] for a 1-D Ts; float32, device or NumPy), to a dict with
      "G_tau", "G_La", "G_Ld"  d cost / d tau, La, Ld on the native grid, float32 [nX] on tau's device: the cotangents
                               engine.tud_vjp_from_od takes;
      "Ts"                     d cost / d Ts, float64 device, [nT] (0-d for a scalar Ts);
      "emis"                   d cost / d emis_knots, float64 [nk][nE] device.
    Same arguments as band_radiance_srf_fused otherwise. A band that comes out NaN there (no grid point under it)
    contributes nothing, whatever its g holds; a point under no live band gets exact zeros. Nothing of size nX x nE is
    formed. outputs: the keys wanted (default all); one left out is not computed. A Ts sequence longer than
    rtx_srf_moments_max_temps() is taken in groups: the groups' rows (and "emis") are added in float64 in group order
    and the rows rounded to float32 once."""
    lib = _lib.load()
    dev = tau.device
    scalar = np.ndim(Ts) == 0
    Ts = np.ascontiguousarray(np.atleast_1d(np.asarray(Ts, dtype=np.float64)))
    if Ts.ndim != 1 or Ts.size == 0:
        raise ValueError("Ts: a scalar or a non-empty 1-D sequence")
    outputs = tuple(outputs)
    if not outputs or any(k not in _VJP_OUTPUTS for k in outputs):
        raise ValueError("outputs: a non-empty selection of %r (got %r)" % (_VJP_OUTPUTS, outputs))
    for v in (tau, La, Ld):
        assert v.dtype == torch.float32 and v.is_cuda and v.is_contiguous() and v.numel() == grid.n
    plan = _srf_fused_plan(Xk, dev)
    nB, nk, nE, nT, nX = len(sensor), plan["Xk_d"].numel(), emis_knots.shape[1], Ts.size, grid.n
    assert emis_knots.dtype == torch.float32 and emis_knots.is_cuda and emis_knots.shape[0] == nk
    emis_knots = emis_knots.contiguous()
    if not torch.is_tensor(g):
        g = torch.as_tensor(np.ascontiguousarray(g, dtype=np.float32))
    g = g.to(device=dev, dtype=torch.float32)
    if tuple(g.shape) != ((nB, nE) if scalar else (nT, nB, nE)):
        raise ValueError("g has shape %r, expected %r (the shape of band_radiance_srf_fused's L)"
                         % (tuple(g.shape), (nB, nE) if scalar else (nT, nB, nE)))
    g = g.reshape(nT, nB, nE).contiguous()
    kx, kr = sensor.on_device(dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    step = lib.rtx_srf_moments_max_temps()
    rows = [k for k in ("G_tau", "G_La", "G_Ld") if k in outputs]
    dTs = torch.empty(nT, dtype=torch.float64, device=dev) if "Ts" in outputs else None
    total = {}  # the float64 sums over the groups of Ts, when there is more than one
    out = {}
    for t0 in range(0, nT, step):
        t1 = min(t0 + step, nT)
        G = {k: torch.empty(nX, dtype=torch.float32, device=dev) for k in rows}
        dE = torch.empty((nk, nE), dtype=torch.float64, device=dev) if "emis" in outputs else None
        _lib.check(lib.rtx_srf_radiance_vjp(grid.byref(), p(tau), p(La), p(Ld), Ts[t0:t1].ctypes.data_as(C.c_void_p), t1 - t0,
                                            p(plan["Xk_d"]), nk, nB, sensor.knot_start.ctypes.data_as(C.c_void_p), p(kx), p(kr),
                                            p(emis_knots), nE, p(g[t0:t1]), p(G.get("G_tau")), p(G.get("G_La")), p(G.get("G_Ld")),
                                            p(dTs[t0:t1]) if dTs is not None else None, p(dE), st))
        if dE is not None:
            G["emis"] = dE
        if nT <= step:
            out.update(G)
        else:
            for k, v in G.items():
                total[k] = v.to(torch.float64) if k not in total else total[k] + v.to(torch.float64)
    for k, v in total.items():
        out[k] = v if k == "emis" else v.to(torch.float32)
    if dTs is not None:
        out["Ts"] = dTs[0] if scalar else dTs
    return out


def _jvp_tangent(x, base, what, dev=None, fn="band_radiance_srf_jvp"):
    """A tangent laid out as `base` plus an optional trailing vector axis: (x with the vector axis FIRST -- a view where it
    can be --, its length or None where x came without one); None passes through. dev: the device of a float32 tensor to
    return, or None for float64 NumPy. fn: the caller named in the error."""
    if x is None:
        return None, None
    if dev is None:
        x = np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float64)
    else:
        if not torch.is_tensor(x):
            x = torch.as_tensor(np.asarray(x, dtype=np.float32))
        x = x.to(device=dev, dtype=torch.float32)
    shape = tuple(x.shape)
    if shape == tuple(base):
        return x[None], None
    if len(shape) == len(base) + 1 and shape[:-1] == tuple(base) and shape[-1] >= 1:
        return (np.moveaxis(x, -1, 0) if dev is None else x.movedim(-1, 0)), shape[-1]
    raise ValueError("%s: %s has shape %r, expected %r plus an optional trailing vector axis" % (fn, what, shape, tuple(base)))


def _jvp_pack_rows(rows, nV, nX):
    """The tangent rows {name: [n_vec][nX] float32 device} as rtx_srf_radiance_jvp takes them, and their leading dimension:
    the library takes one leading dimension for the three rows: rows that share one go as they are, else they are packed."""
    lds = set(x.stride(0) for x in rows.values()) if nV > 1 else {nX}
    if all(x.stride(1) == 1 for x in rows.values()) and len(lds) == 1 and min(lds) >= nX:
        return rows, lds.pop()
    return {k: x.contiguous() for k, x in rows.items()}, nX


def _srf_radiance_jvp_groups(grid, tau, Ld, plan, sensor, emis_knots, N, M, jr, Ts, m0, rows, ld_d, dTs, dE, dL):
    """rtx_srf_radiance_jvp on the moments N, M [nM][nB][nk], jr that srf_moments gave at Ts[m0:m0 + nM], into
    dL[:, m0:m0 + nM] ([n_vec][nT][nB][nE]): the temperatures and the vectors rtx_srf_radiance_jvp_max_temps() /
    _max_vectors() at a time. rows, ld_d from _jvp_pack_rows; dTs [n_vec][nT] host or None; dE [n_vec][nk][nE] or None."""
    lib = _lib.load()
    dev = tau.device
    nV, nB, nE, nk = dL.shape[0], dL.shape[2], dL.shape[3], plan["Xk_d"].numel()
    kx, kr = sensor.on_device(dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    step_t, step_v = lib.rtx_srf_radiance_jvp_max_temps(), lib.rtx_srf_radiance_jvp_max_vectors()
    for t0 in range(m0, m0 + M.shape[0], step_t):
        t1 = min(t0 + step_t, m0 + M.shape[0])
        Ts_g = np.ascontiguousarray(Ts[t0:t1])
        for v0 in range(0, nV, step_v):
            v1 = min(v0 + step_v, nV)
            dst = dL[v0:v1, t0:t1]
            out = dst if dst.is_contiguous() else torch.empty((v1 - v0, t1 - t0, nB, nE), dtype=torch.float32, device=dev)
            dTs_g = None if dTs is None else np.ascontiguousarray(dTs[v0:v1, t0:t1])
            row = lambda k: C.c_void_p(rows[k].data_ptr() + 4 * v0 * ld_d) if k in rows else None
            _lib.check(lib.rtx_srf_radiance_jvp(grid.byref(), p(tau), p(Ld), row("d_tau"), row("d_La"), row("d_Ld"), ld_d,
                                                Ts_g.ctypes.data_as(C.c_void_p),
                                                None if dTs_g is None else dTs_g.ctypes.data_as(C.c_void_p), t1 - t0,
                                                p(plan["Xk_d"]), nk, nB, sensor.knot_start.ctypes.data_as(C.c_void_p), p(kx), p(kr),
                                                p(N), p(M[t0 - m0:t1 - m0]), p(jr), p(emis_knots),
                                                None if dE is None else p(dE[v0:v1]), nE, v1 - v0, p(out), st))
            if out is not dst:
                dst.copy_(out)


def band_radiance_srf_jvp(grid, tau, La, Ld, Xk, emis_knots, Ts, sensor, d_tau=None, d_La=None, d_Ld=None, d_Ts=None, d_emis=None):
    """band_radiance_srf_fused and its tangent (rtx_srf_radiance_jvp): the change dL of the band radiances L along
    directions in the inputs, without a Jacobian and without anything of size nX x nE.
      d_tau, d_La, d_Ld  tangents of tau, La, Ld on the native grid, [nX] (float32; device or NumPy): the rows
                         engine.tud_jvp returns are taken where they are;
      d_Ts               tangent of Ts, shaped like Ts (host numbers, taken as float64);
      d_emis             tangent of emis_knots, [nk][nE] (float32).
    Each may carry a trailing axis of n_vec directions (all that are given must agree on it: ValueError otherwise); one left
    None is an exact zero and nothing is evaluated for it; not all five may be None. Same arguments as
    band_radiance_srf_fused otherwise. Returns (L, dL) on tau's device: L that call's, bit for bit (it comes from the
    srf_moments + rtx_band_mix run that supplies the tangent's N, M and jrange); dL float32 laid out like L, with a
    trailing [n_vec] axis when the tangents carry one. A band that is NaN in L is NaN in dL. The temperatures and the
    vectors go to the library rtx_srf_radiance_jvp_max_temps() / _max_vectors() at a time; the grouping changes no bit."""
    lib = _lib.load()
    dev = tau.device
    scalar = np.ndim(Ts) == 0
    Ts = np.ascontiguousarray(np.atleast_1d(np.asarray(Ts, dtype=np.float64)))
    if Ts.ndim != 1 or Ts.size == 0:
        raise ValueError("Ts: a scalar or a non-empty 1-D sequence")
    for v in (tau, La, Ld):
        assert v.dtype == torch.float32 and v.is_cuda and v.is_contiguous() and v.numel() == grid.n
    plan = _srf_fused_plan(Xk, dev)
    nB, nk, nE, nT, nX = len(sensor), plan["Xk_d"].numel(), emis_knots.shape[1], Ts.size, grid.n
    assert emis_knots.dtype == torch.float32 and emis_knots.is_cuda and emis_knots.shape[0] == nk
    emis_knots = emis_knots.contiguous()
    rows, n_vecs = {}, set()
    for key, x in (("d_tau", d_tau), ("d_La", d_La), ("d_Ld", d_Ld)):
        x, nv = _jvp_tangent(x, (nX,), key, dev)
        if x is not None:
            rows[key] = x
            n_vecs.add(nv)
    dTs, nv = _jvp_tangent(d_Ts, () if scalar else (nT,), "d_Ts")
    if dTs is not None:
        n_vecs.add(nv)
        dTs = dTs.reshape(-1, nT)
        if not np.isfinite(dTs).all():
            raise ValueError("band_radiance_srf_jvp: d_Ts has non-finite entries")
    dE, nv = _jvp_tangent(d_emis, (nk, nE), "d_emis", dev)
    if dE is not None:
        n_vecs.add(nv)
        dE = dE.contiguous()  # [n_vec][nk][nE]
    if not n_vecs:
        raise ValueError("band_radiance_srf_jvp: no tangent (d_tau, d_La, d_Ld, d_Ts and d_emis are all None)")
    if len(n_vecs) != 1:
        raise ValueError("band_radiance_srf_jvp: the tangents disagree on the vector axis: %r" % sorted(n_vecs, key=str))
    n_vec = n_vecs.pop()
    nV = 1 if n_vec is None else n_vec
    rows, ld_d = _jvp_pack_rows(rows, nV, nX)
    L = torch.empty((nT, nB, nE), dtype=torch.float32, device=dev)
    dL = torch.empty((nV, nT, nB, nE), dtype=torch.float32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    step_m = lib.rtx_srf_moments_max_temps()
    for m0 in range(0, nT, step_m):
        N, Cb, M, jr = srf_moments(grid, tau, La, Ld, plan["Xk_d"], Ts[m0:m0 + step_m], sensor)
        for t in range(M.shape[0]):
            _lib.check(lib.rtx_band_mix(p(N), p(Cb), p(M[t]), p(jr), nB, nk, p(emis_knots), nE, p(L[m0 + t]), st))
        _srf_radiance_jvp_groups(grid, tau, Ld, plan, sensor, emis_knots, N, M, jr, Ts, m0, rows, ld_d, dTs, dE, dL)
    if scalar:
        L, dL = L[0], dL[:, 0]
    dL = dL.movedim(0, -1) if n_vec is not None else dL[0]
    return L, dL


def chebyshev_lagrange(Q):
    """Chebyshev nodes s_q on (-1,1) and the monomial coefficients coef[q][d] of their Lagrange basis."""
    s = np.cos((2 * np.arange(Q) + 1) * np.pi / (2 * Q))
    coef = np.zeros((Q, Q))
    for q in range(Q):
        others = np.delete(s, q)
        poly = np.atleast_1d(np.poly(others)) / np.prod(s[q] - others)  # highest power first (Q = 1: np.poly gives a scalar)
        coef[q] = poly[::-1]
    return s, coef




def _cube_plan(grid, Xk, resFactor, band_slice, Q, bands, dev):
    """Everything hsi_cube needs that does not depend on the spectra or the scene: the band list of rt.ILS_MAKO, its centres
    and widths and the knot axis as device tensors, the Chebyshev nodes and Lagrange coefficients. A scene generator calls
    hsi_cube once per atmosphere / scene with the same axis, knots and bands; building these took as long as the kernels."""
    Xk = np.ascontiguousarray(Xk, dtype=np.float64)
    key = (grid.x_at(0), grid.step, grid.n, resFactor, band_slice, Q, str(dev), Xk.tobytes(),
           None if bands is None else tuple(np.ascontiguousarray(v, dtype=np.float64).tobytes() for v in bands))
    with _CUBE_PLANS_LOCK:
        plan = _CUBE_PLANS.get(key)
    if plan is None:
        X_out, centre, sigma = bands if bands is not None else mako_bands(grid.x_at(0), grid.x_at(grid.n - 1), resFactor)
        if band_slice is not None:
            X_out, centre, sigma = (v[band_slice[0]:band_slice[1]] for v in (X_out, centre, sigma))
        s_nodes, coef = chebyshev_lagrange(Q)
        plan = {"X_out": np.array(X_out, dtype=np.float64), "coef32": np.ascontiguousarray(coef, dtype=np.float32),
                "sn32": np.ascontiguousarray(s_nodes, dtype=np.float32), "Xk_d": torch.as_tensor(Xk, device=dev),
                "c_d": torch.as_tensor(np.ascontiguousarray(centre, dtype=np.float64), device=dev),
                "s_d": torch.as_tensor(np.ascontiguousarray(sigma, dtype=np.float64), device=dev)}
        with _CUBE_PLANS_LOCK:
            if len(_CUBE_PLANS) >= _CUBE_PLANS_MAX:
                _CUBE_PLANS.pop(next(iter(_CUBE_PLANS)))
            _CUBE_PLANS[key] = plan
    return plan


def hsi_cube(grid, tau, La, Ld, Xk, endmembers, kidx, frac, Tpix, resFactor=2, band_slice=None, Q=4, bands=None):
    """Config C5: band radiances of an HSI cube whose pixels each have an emissivity mixture and a surface
    temperature of their own (LWIR_HSI_Generator.py:151-167), from monochromatic tau/La/Ld through the
    triangle ILS (rt.ILS_MAKO with resFactor).

    endmembers [nk][nEnd] float32 device (knot spectra), kidx [nPix][nMix] int32, frac [nPix][nMix] float32,
    Tpix [nPix] float64 -- device tensors. band_slice: (b0, b1) to compute only a band-aligned shard.
    bands = (X_out, centre, sigma): explicit band list (mako_bands() of the FULL spectral axis) when `grid` is only the
    wavenumber shard under those bands (dist.hsi_cube_from_atmosphere); default: the bands inside `grid`.
    Returns (X_out [nB] NumPy, cube [nB][nPix] float32 device). Three launches: rtx_band_basis_moments (the one pass over
    the monochromatic arrays), rtx_band_mix_stacked (its Q + 1 moment arrays x the endmember knots), rtx_pixel_cube."""
    lib = _lib.load()
    dev = tau.device
    plan = _cube_plan(grid, Xk, resFactor, None if band_slice is None else (int(band_slice[0]), int(band_slice[1])), int(Q), bands, dev)
    X_out = plan["X_out"].copy()
    nB, nk, nEnd = X_out.size, len(Xk), endmembers.shape[1]
    nPix, nMix = kidx.shape
    assert endmembers.dtype == torch.float32 and endmembers.shape[0] == nk
    endmembers = endmembers.contiguous()
    assert kidx.dtype == torch.int32 and frac.dtype == torch.float32 and Tpix.dtype == torch.float64
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    cube = f32(nB, nPix)
    if nB == 0:
        return X_out, cube
    N, Cb, M = f32(nB), f32(nB), f32(Q + 1, nB, nk)  # M[0..Q-1]: the Planck-node basis moments, M[Q]: the Ld moment
    jr = torch.empty((nB, 2), dtype=torch.int32, device=dev)
    tab = f32(nEnd, Q + 1, nB)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.rtx_band_basis_moments(0, grid.byref(), p(tau), p(La), p(Ld), p(plan["Xk_d"]), nk, nB, p(plan["c_d"]), p(plan["s_d"]), Q,
                                          plan["coef32"].ctypes.data_as(C.c_void_p), 1.0, p(N), p(Cb), p(M[Q]), p(M), p(jr), st))
    _lib.check(lib.rtx_band_mix_stacked(p(M), p(jr), nB, Q + 1, nk, p(endmembers), nEnd, p(tab), st))
    _lib.check(lib.rtx_pixel_cube(nB, Q, p(plan["c_d"]), p(plan["s_d"]), 1.0, plan["sn32"].ctypes.data_as(C.c_void_p), p(N), p(Cb), p(tab),
                                  nEnd, nPix, nMix, p(kidx.contiguous()), p(frac.contiguous()), p(Tpix.contiguous()), p(cube), st))
    return X_out, cube


def srf_cube_nodes(T_lo, T_hi, n_nodes):
    """The n_nodes Chebyshev nodes of [T_lo, T_hi], descending: T_q = (T_lo + T_hi) / 2 + (T_hi - T_lo) / 2 * cos((2 q + 1) pi /
    (2 n_nodes)): chebyshev_lagrange's nodes mapped to the range."""
    Q = int(n_nodes)
    s = np.cos((2 * np.arange(Q) + 1) * np.pi / (2 * Q))  # chebyshev_lagrange(Q)[0], without its basis polynomials
    return 0.5 * (T_lo + T_hi) + 0.5 * (T_hi - T_lo) * s


def _planck_host(x, T):
    """B(nu, T) [uW/(cm^2 sr cm^-1)] in fp64 NumPy, rtx_planck's constants."""
    x100 = 100.0 * np.asarray(x, dtype=np.float64)
    return _C1 * x100 ** 3 * 1e4 / np.expm1(_C2 * x100 / np.asarray(T, dtype=np.float64))


@functools.lru_cache(maxsize=64)  # a scene generator asks for one (axis, range, node count) again and again
def planck_node_error(x_hi, T_lo, T_hi, n_nodes, samples=2001):
    """What interpolating the Planck function in temperature through srf_cube_nodes(T_lo, T_hi, n_nodes) costs at
    wavenumber x_hi [cm^-1]: the largest |interpolant - B| over `samples` temperatures evenly spaced over [T_lo, T_hi],
    relative to the largest B there. Host NumPy, fp64. The error grows with the wavenumber, so a grid's highest is its worst."""
    Tq = srf_cube_nodes(T_lo, T_hi, n_nodes)
    T = np.linspace(T_lo, T_hi, int(samples))
    B = _planck_host(x_hi, T)
    Bq = _planck_host(x_hi, Tq)
    interp = np.zeros_like(T)
    for q in range(Tq.size):
        others = np.delete(Tq, q)
        interp += Bq[q] * np.prod((T[:, None] - others[None, :]) / (Tq[q] - others)[None, :], axis=1)
    return float(np.max(np.abs(interp - B)) / np.max(B))


def _srf_cube_front(fn, grid, tau, La, Ld, Xk, endmembers, kidx, frac, Tpix, sensor, n_nodes, T_range, interp_tol, g=None,
                    need_device=True):
    """The front half hsi_cube_srf and hsi_cube_srf_vjp share: the argument checks, the temperature range (T_range=None:
    one read from the device), the interpolation estimate and the nodes. Everything up to the estimate runs before any
    device work. g: the cotangent of the adjoint, checked against the cube's shape [nB][nPix]. need_device=False: host
    tensors pass (a caller that validates before it has device arrays). Returns a dict: Q, Xk, T_lo, T_hi, nodes, and
    endmembers, kidx, frac, Tpix contiguous."""
    lib = _lib.load()
    Q = int(n_nodes)
    Q_max = lib.rtx_srf_cube_max_nodes()
    if Q != n_nodes or Q < 1 or Q > Q_max:
        raise ValueError(f"n_nodes={n_nodes!r}: an integer from 1 to {Q_max}")
    Xk = np.asarray(Xk, dtype=np.float64).ravel()
    if endmembers.dim() != 2 or endmembers.shape[0] != Xk.size or endmembers.shape[1] < 1 or endmembers.dtype != torch.float32:
        raise ValueError(f"endmembers: float32 [nk = {Xk.size}][nEnd >= 1], got {endmembers.dtype} {tuple(endmembers.shape)}")
    if kidx.dim() != 2 or kidx.shape[1] < 1 or kidx.dtype != torch.int32:
        raise ValueError(f"kidx: int32 [nPix][nMix >= 1], got {kidx.dtype} {tuple(kidx.shape)}")
    if frac.shape != kidx.shape or frac.dtype != torch.float32:
        raise ValueError(f"frac: float32 {tuple(kidx.shape)} like kidx, got {frac.dtype} {tuple(frac.shape)}")
    nPix, nMix = kidx.shape
    if Tpix.dim() != 1 or Tpix.shape[0] != nPix or Tpix.dtype != torch.float64:
        raise ValueError(f"Tpix: float64 [nPix = {nPix}], got {Tpix.dtype} {tuple(Tpix.shape)}")
    for name, v in (("tau", tau), ("La", La), ("Ld", Ld)):
        if v.dtype != torch.float32 or v.numel() != grid.n:
            raise ValueError(f"{name}: float32 [grid.n = {grid.n}], got {v.dtype} {tuple(v.shape)}")
    if g is not None and (tuple(g.shape) != (len(sensor), nPix) or g.dtype != torch.float32):
        raise ValueError(f"g: float32 [nB = {len(sensor)}][nPix = {nPix}] like the cube, got {g.dtype} {tuple(g.shape)}")
    if T_range is None:
        if need_device and not Tpix.is_cuda:
            raise ValueError(f"{fn} takes device tensors (Tpix is not on a GPU)")
        fin = torch.isfinite(Tpix)
        inf = torch.full_like(Tpix, float("inf"))
        ends = torch.stack([torch.where(fin, Tpix, inf).min(), torch.where(fin, Tpix, -inf).max()]).cpu().numpy() if nPix else None
        if ends is None or not np.all(np.isfinite(ends)):
            raise ValueError("T_range=None needs at least one finite Tpix")
        T_lo, T_hi = float(ends[0]), float(ends[1])
    else:
        T_lo, T_hi = (float(v) for v in T_range)
    if not (np.isfinite(T_lo) and np.isfinite(T_hi) and 0.0 < T_lo <= T_hi):
        raise ValueError(f"T_range=({T_lo!r}, {T_hi!r}): finite, positive and ascending")
    if T_hi - T_lo < 1.0:
        mid = 0.5 * (T_lo + T_hi)
        T_lo, T_hi = mid - 0.5, mid + 0.5
    est = planck_node_error(float(grid.x_at(grid.n - 1)), T_lo, T_hi, Q)
    if not est <= interp_tol:
        raise ValueError(f"{fn}: interpolating Planck through {Q} nodes over [{T_lo:g}, {T_hi:g}] K is off by an estimated "
                         f"{est:.3g} of the largest B at {grid.x_at(grid.n - 1):g} cm^-1, above interp_tol={interp_tol:g}: narrow "
                         "T_range, raise n_nodes or split the scene by temperature")
    if need_device:
        for name, v in (("tau", tau), ("endmembers", endmembers), ("kidx", kidx), ("frac", frac), ("Tpix", Tpix)):
            if not v.is_cuda:
                raise ValueError(f"{fn} takes device tensors ({name} is not on a GPU)")
    endmembers, kidx, frac, Tpix = (v.contiguous() for v in (endmembers, kidx, frac, Tpix))
    return dict(Q=Q, Xk=Xk, T_lo=T_lo, T_hi=T_hi, nodes=srf_cube_nodes(T_lo, T_hi, Q), endmembers=endmembers, kidx=kidx, frac=frac,
                Tpix=Tpix)


def _srf_cube_tables(grid, tau, La, Ld, f, sensor, keep_moments=False):
    """Stages 1 and 2 of hsi_cube_srf on the front half's dict f: (N, C, tab [nEnd][Q][nB], T_host = the nodes, then the range);
    keep_moments: followed by srf_moments' M [Q][nB][nk] and jrange at the nodes, which the cube's tangent uses again."""
    lib = _lib.load()
    dev = tau.device
    Q, Xk, endmembers = f["Q"], f["Xk"], f["endmembers"]
    nB, nk, nEnd = len(sensor), Xk.size, endmembers.shape[1]
    plan = _srf_fused_plan(Xk, dev)
    N, Cb, M, jr = srf_moments(grid, tau, La, Ld, plan["Xk_d"], f["nodes"], sensor)
    tab = torch.empty((nEnd, Q, nB), dtype=torch.float32, device=dev)
    T_host = np.ascontiguousarray(np.concatenate([f["nodes"], [f["T_lo"], f["T_hi"]]]))  # the nodes, then the range
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.rtx_srf_cube_tables(p(M), p(jr), nB, Q, nk, p(endmembers), nEnd, p(tab), st))
    return (N, Cb, tab, T_host, M, jr) if keep_moments else (N, Cb, tab, T_host)


def hsi_cube_srf(grid, tau, La, Ld, Xk, endmembers, kidx, frac, Tpix, sensor, n_nodes=8, T_range=None, interp_tol=1e-6):
    """hsi_cube() for any sensor: band radiances of an HSI cube whose pixels each have an emissivity mixture and a surface
    temperature of their own, under the sensor's tabulated responses, whatever their width. The Planck function is
    interpolated in TEMPERATURE through n_nodes Chebyshev nodes of T_range (hsi_cube interpolates in wavenumber across a
    band, which holds for MAKO-narrow bands only). Arguments as hsi_cube(), with a Sensor in place of resFactor.

    T_range = (T_lo, T_hi) [K]: the range the nodes span. None: the smallest and largest finite Tpix, read from the device
    -- ONE synchronisation; an explicit range avoids it. A range narrower than 1 K is widened symmetrically to 1 K (the
    nodes of a one-temperature scene stay distinct). A pixel whose temperature is not finite or lies outside the range is
    NaN in every band: there is no extrapolation and no check on the device's side.
    interp_tol: the call raises ValueError, before any device work, when planck_node_error(grid's highest wavenumber,
    T_lo, T_hi, n_nodes) exceeds it (8 nodes over 230-350 K at 1400 cm^-1: 5.5e-8; 4 nodes: 3.9e-4).

    Returns (X_out [nB] NumPy = sensor.centres, cube [nB][nPix] float32 device); a band with no grid point under it is NaN.
    Three stages: srf_moments at the node temperatures (the one pass over tau / La / Ld per group of 16 bands),
    rtx_srf_cube_tables (its n_nodes moment arrays x the endmember knots), rtx_srf_pixel_cube."""
    lib = _lib.load()
    f = _srf_cube_front("hsi_cube_srf", grid, tau, La, Ld, Xk, endmembers, kidx, frac, Tpix, sensor, n_nodes, T_range, interp_tol)
    dev = tau.device
    endmembers, kidx, frac, Tpix, Q = f["endmembers"], f["kidx"], f["frac"], f["Tpix"], f["Q"]
    nPix, nMix = kidx.shape
    X_out = np.array(sensor.centres)
    nB, nEnd = len(sensor), endmembers.shape[1]
    cube = torch.empty((nB, nPix), dtype=torch.float32, device=dev)
    if nB == 0 or nPix == 0:
        return X_out, cube
    N, Cb, tab, T_host = _srf_cube_tables(grid, tau, La, Ld, f, sensor)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.rtx_srf_pixel_cube(nB, Q, T_host.ctypes.data_as(C.c_void_p), p(N), p(Cb), p(tab), nEnd, nPix, nMix, p(kidx), p(frac),
                                      p(Tpix), p(cube), st))
    return X_out, cube


_CUBE_VJP_OUTPUTS = ("G_tau", "G_La", "G_Ld", "Tpix", "frac", "endmembers")


def hsi_cube_srf_vjp(grid, tau, La, Ld, Xk, endmembers, kidx, frac, Tpix, sensor, g, n_nodes=8, T_range=None, interp_tol=1e-6,
                     outputs=_CUBE_VJP_OUTPUTS):
    """The adjoint of hsi_cube_srf: from g = d cost / d cube, [nB][nPix] float32 (device or NumPy), to a dict with
      "Tpix"                   d cost / d Tpix, float64 [nPix] device;
      "frac"                   d cost / d frac, float64 [nPix][nMix] device;
      "endmembers"             d cost / d endmembers, float64 [nk][nEnd] device;
      "G_tau", "G_La", "G_Ld"  d cost / d tau, La, Ld on the native grid, float32 [nX] on tau's device: the cotangents
                               engine.tud_vjp_from_od takes.
    Same arguments, checks and nodes as hsi_cube_srf. No Jacobian is stored and nothing of size nPix x nX or nPix x nk is
    formed: the cube is a linear combination of the band radiances of the pure endmembers (and of a surface of emissivity
    0) at the node temperatures, so rtx_srf_pixel_cube_vjp gives the pixels' own gradients and the cotangent gL [Q][nB][nEnd + 1]
    of those radiances, and band_radiance_srf_vjp at Ts = the nodes, E' = [E | 0] takes gL to the rows and the knots.
    A band that is NaN in the cube contributes nothing, whatever its g holds; a pixel whose temperature is not finite or
    lies outside the range is NaN in its own "Tpix" and "frac" entries and contributes nothing elsewhere. The gradient
    with respect to Tpix is that of the interpolant hsi_cube_srf evaluates. outputs: the keys wanted (default all); one
    left out is not computed, and with "Tpix" and "frac" alone band_radiance_srf_vjp does not run."""
    lib = _lib.load()
    outputs = tuple(outputs)
    if not outputs or any(k not in _CUBE_VJP_OUTPUTS for k in outputs):
        raise ValueError("outputs: a non-empty selection of %r (got %r)" % (_CUBE_VJP_OUTPUTS, outputs))
    if not torch.is_tensor(g):
        g = np.asarray(g)
        if g.dtype != np.float32:
            raise ValueError(f"g: float32 like the cube, got {g.dtype} {tuple(g.shape)}")
        g = torch.as_tensor(np.ascontiguousarray(g))
    f = _srf_cube_front("hsi_cube_srf_vjp", grid, tau, La, Ld, Xk, endmembers, kidx, frac, Tpix, sensor, n_nodes, T_range, interp_tol, g=g)
    dev = tau.device
    endmembers, kidx, frac, Tpix, Q = f["endmembers"], f["kidx"], f["frac"], f["Tpix"], f["Q"]
    nPix, nMix = kidx.shape
    nB, nk, nEnd, nX = len(sensor), f["Xk"].size, endmembers.shape[1], grid.n
    back = {"G_tau": "G_tau", "G_La": "G_La", "G_Ld": "G_Ld", "endmembers": "emis"}
    want_back = tuple(back[k] for k in outputs if k in back)
    if nB == 0 or nPix == 0:  # the gradient of nothing
        zero = {"Tpix": ((nPix,), torch.float64), "frac": ((nPix, nMix), torch.float64), "endmembers": ((nk, nEnd), torch.float64),
                "G_tau": ((nX,), torch.float32), "G_La": ((nX,), torch.float32), "G_Ld": ((nX,), torch.float32)}
        return {k: torch.zeros(zero[k][0], dtype=zero[k][1], device=dev) for k in outputs}
    g = g.to(device=dev).contiguous()
    N, _, tab, T_host = _srf_cube_tables(grid, tau, La, Ld, f, sensor)
    dT = torch.empty(nPix, dtype=torch.float64, device=dev) if "Tpix" in outputs else None
    dfrac = torch.empty((nPix, nMix), dtype=torch.float64, device=dev) if "frac" in outputs else None
    gL = torch.empty((Q, nB, nEnd + 1), dtype=torch.float32, device=dev) if want_back else None
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.rtx_srf_pixel_cube_vjp(nB, Q, T_host.ctypes.data_as(C.c_void_p), p(N), p(tab), nEnd, nPix, nMix, p(kidx), p(frac),
                                          p(Tpix), p(g), p(dT), p(dfrac), p(gL), st, 0))
    out = {}
    if dT is not None:
        out["Tpix"] = dT
    if dfrac is not None:
        out["frac"] = dfrac
    if want_back:
        E0 = torch.cat([endmembers, torch.zeros((nk, 1), dtype=torch.float32, device=dev)], dim=1)  # [E | 0]
        r = band_radiance_srf_vjp(grid, tau.contiguous(), La.contiguous(), Ld.contiguous(), f["Xk"], E0, f["nodes"], sensor, gL,
                                  outputs=want_back)
        for k in outputs:
            if k in back:
                out[k] = r["emis"][:, :nEnd].contiguous() if k == "endmembers" else r[k]
    return {k: out[k] for k in outputs}


def _cube_jvp_axis(fn, tangents, bases):
    """The vector axis of a cube tangent's groups, from their shapes alone (nothing is moved or converted): tangents
    {name: array, tensor or None}, bases {name: the shape of the input it moves}. Returns n_vec, or None where the tangents
    come without a trailing axis. ValueError: a shape that is neither, all None, or groups that disagree."""
    n_vecs = set()
    for key, x in tangents.items():
        if x is None:
            continue
        shape, base = tuple(np.shape(x) if not torch.is_tensor(x) else x.shape), tuple(bases[key])
        if shape == base:
            n_vecs.add(None)
        elif len(shape) == len(base) + 1 and shape[:-1] == base and shape[-1] >= 1:
            n_vecs.add(shape[-1])
        else:
            raise ValueError("%s: %s has shape %r, expected %r plus an optional trailing vector axis" % (fn, key, shape, base))
    if not n_vecs:
        raise ValueError("%s: no tangent (%s are all None)" % (fn, ", ".join(tangents)))
    if len(n_vecs) != 1:
        raise ValueError("%s: the tangents disagree on the vector axis: %r" % (fn, sorted(n_vecs, key=str)))
    return n_vecs.pop()


def hsi_cube_srf_jvp(grid, tau, La, Ld, Xk, endmembers, kidx, frac, Tpix, sensor, d_tau=None, d_La=None, d_Ld=None,
                     d_endmembers=None, d_frac=None, d_Tpix=None, n_nodes=8, T_range=None, interp_tol=1e-6):
    """hsi_cube_srf and its tangent: the change d_cube of the cube along directions in its inputs, without a
    Jacobian and without anything of size nPix x nX or nPix x nk.
      d_tau, d_La, d_Ld  tangents of tau, La, Ld on the native grid, [nX] (float32; device or NumPy): the rows
                         engine.tud_jvp returns are taken where they are;
      d_endmembers       tangent of endmembers, [nk][nEnd] (float32);
      d_frac             tangent of frac, [nPix][nMix] (float32);
      d_Tpix             tangent of Tpix, [nPix] (float64).
    Each may carry a trailing axis of n_vec directions (all that are given must agree on it: ValueError otherwise); one left
    None is an exact zero and nothing is evaluated for it; not all six may be None. Same arguments, checks and nodes as
    hsi_cube_srf otherwise. Returns (X_out, cube, d_cube) on tau's device: cube that call's, bit for bit; d_cube float32 laid
    out like cube, with a trailing [n_vec] axis when the tangents carry one. The cube is a linear combination of the band
    radiances of the pure endmembers (and of a surface of emissivity 0) at the node temperatures: when any of the first four
    tangents is given, rtx_srf_radiance_jvp at Ts = the nodes, E' = [E | 0] supplies their tangent dL, on the node moments
    the cube itself is made from (one srf_moments pass for both), and rtx_srf_pixel_cube_jvp takes dL, d_frac and d_Tpix to
    d_cube; with d_frac / d_Tpix alone the band tangent does not run. A band that is NaN in the cube is NaN in d_cube, and so
    is the column of a pixel whose temperature is not finite or lies outside the range. The tangent along d_Tpix is that of
    the interpolant hsi_cube_srf evaluates. The vectors go to the library rtx_srf_pixel_cube_jvp_max_vectors() at a time;
    the grouping changes no bit."""
    lib = _lib.load()
    fn = "hsi_cube_srf_jvp"
    f = _srf_cube_front(fn, grid, tau, La, Ld, Xk, endmembers, kidx, frac, Tpix, sensor, n_nodes, T_range, interp_tol,
                        need_device=False)
    endmembers, kidx, frac, Tpix, Q = f["endmembers"], f["kidx"], f["frac"], f["Tpix"], f["Q"]
    nPix, nMix = kidx.shape
    nB, nk, nEnd, nX = len(sensor), f["Xk"].size, endmembers.shape[1], grid.n
    given = dict(d_tau=d_tau, d_La=d_La, d_Ld=d_Ld, d_endmembers=d_endmembers, d_frac=d_frac, d_Tpix=d_Tpix)
    bases = dict(d_tau=(nX,), d_La=(nX,), d_Ld=(nX,), d_endmembers=(nk, nEnd), d_frac=(nPix, nMix), d_Tpix=(nPix,))
    n_vec = _cube_jvp_axis(fn, given, bases)
    nV = 1 if n_vec is None else n_vec
    for name, v in (("tau", tau), ("endmembers", endmembers), ("kidx", kidx), ("frac", frac), ("Tpix", Tpix)):
        if not v.is_cuda:
            raise ValueError(f"{fn} takes device tensors ({name} is not on a GPU)")
    dev = tau.device
    X_out = np.array(sensor.centres)
    cube = torch.empty((nB, nPix), dtype=torch.float32, device=dev)
    d_cube = torch.empty((nV, nB, nPix), dtype=torch.float32, device=dev)
    shaped = lambda d: d.movedim(0, -1) if n_vec is not None else d[0]
    if nB == 0 or nPix == 0:
        return X_out, cube, shaped(d_cube)
    rows = {}
    for key in ("d_tau", "d_La", "d_Ld"):
        x, _ = _jvp_tangent(given[key], (nX,), key, dev, fn=fn)
        if x is not None:
            rows[key] = x
    dE, _ = _jvp_tangent(d_endmembers, (nk, nEnd), "d_endmembers", dev, fn=fn)
    dF, _ = _jvp_tangent(d_frac, (nPix, nMix), "d_frac", dev, fn=fn)
    dF = None if dF is None else dF.contiguous()  # [n_vec][nPix][nMix]
    dT = None
    if d_Tpix is not None:
        dT = d_Tpix if torch.is_tensor(d_Tpix) else torch.as_tensor(np.asarray(d_Tpix, dtype=np.float64))
        dT = dT.to(device=dev, dtype=torch.float64)
        dT = (dT.movedim(-1, 0) if n_vec is not None else dT[None]).contiguous()  # [n_vec][nPix]
    tau, La, Ld = tau.contiguous(), La.contiguous(), Ld.contiguous()
    N, Cb, tab, T_host, M, jr = _srf_cube_tables(grid, tau, La, Ld, f, sensor, keep_moments=True)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    T_p = T_host.ctypes.data_as(C.c_void_p)
    _lib.check(lib.rtx_srf_pixel_cube(nB, Q, T_p, p(N), p(Cb), p(tab), nEnd, nPix, nMix, p(kidx), p(frac), p(Tpix), p(cube), st))
    dL = None
    if rows or dE is not None:  # the tangent of the pure endmembers' band radiances at the nodes, column nEnd: emissivity 0
        pad = lambda x: torch.cat([x, torch.zeros(tuple(x.shape[:-1]) + (1,), dtype=torch.float32, device=dev)], dim=-1)
        dL = torch.empty((nV, Q, nB, nEnd + 1), dtype=torch.float32, device=dev)
        rows, ld_d = _jvp_pack_rows(rows, nV, nX)
        _srf_radiance_jvp_groups(grid, tau, Ld, _srf_fused_plan(f["Xk"], dev), sensor, pad(endmembers), N, M, jr, f["nodes"], 0, rows, ld_d,
                                 None, None if dE is None else pad(dE.contiguous()), dL)
    step = lib.rtx_srf_pixel_cube_jvp_max_vectors()
    for v0 in range(0, nV, step):
        v1 = min(v0 + step, nV)
        part = lambda t: p(t[v0:v1]) if t is not None else None
        _lib.check(lib.rtx_srf_pixel_cube_jvp(nB, Q, T_p, p(N), p(tab), nEnd, nPix, nMix, p(kidx), p(frac), p(Tpix), part(dF), part(dT),
                                              part(dL), v1 - v0, p(d_cube[v0:v1]), st, 0))
    return X_out, cube, shaped(d_cube)


RTX_FIT_START_GIVEN = 1  # include/radtxfr_hip.h
_CUBE_NORMAL_OUTPUTS = ("cost", "grad", "hess", "step")


def _cube_fit_args(fn, sensor, kidx, meas, weights):
    """What hsi_cube_srf_normal and hsi_cube_srf_fit check beside _srf_cube_front, before any device work: the mixture
    length against the library's, meas [nB][nPix] float32, weights [nB] (anything np.asarray takes, or a tensor) or None.
    Returns weights as a float32 host or device tensor, or None."""
    nMix_max = _lib.load().rtx_srf_pixel_cube_fit_max_mix()
    if kidx.dim() == 2 and kidx.shape[1] > nMix_max:
        raise ValueError(f"{fn}: nMix={kidx.shape[1]} above the {nMix_max} unknown fractions a pixel's fit holds")
    nB, nPix = len(sensor), kidx.shape[0]
    if not torch.is_tensor(meas) or tuple(meas.shape) != (nB, nPix) or meas.dtype != torch.float32:
        raise ValueError(f"{fn}: meas: a float32 tensor [nB = {nB}][nPix = {nPix}] like the cube, got "
                         f"{getattr(meas, 'dtype', type(meas))} {tuple(getattr(meas, 'shape', ()))}")
    if weights is None:
        return None
    w = weights if torch.is_tensor(weights) else torch.as_tensor(np.ascontiguousarray(np.asarray(weights, dtype=np.float32)))
    if tuple(w.shape) != (nB,) or not w.dtype.is_floating_point:
        raise ValueError(f"{fn}: weights: [nB = {nB}] floating point, got {w.dtype} {tuple(w.shape)}")
    return w.to(torch.float32)


def _cube_box_args(fn, nonneg, sum_weight, kidx):
    """The checks of the bound-constrained variants, before any device work. Returns (nonneg, sum_weight)."""
    nonneg = bool(nonneg)
    try:
        sw = float(sum_weight)
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: sum_weight={sum_weight!r}: a finite number that is not negative") from None
    if not (np.isfinite(sw) and sw >= 0.0):
        raise ValueError(f"{fn}: sum_weight={sum_weight!r}: a finite number that is not negative")
    if sw > 0.0 and not nonneg:
        raise ValueError(f"{fn}: sum_weight={sw!r} needs nonneg=True (the soft sum-to-one belongs to the constrained fit)")
    if nonneg and torch.is_tensor(kidx) and kidx.dim() == 2:
        nMix_max = _lib.load().rtx_srf_pixel_cube_fit_box_max_mix()
        if kidx.shape[1] > nMix_max:
            raise ValueError(f"{fn}: nMix={kidx.shape[1]} above the {nMix_max} unknown fractions a pixel's constrained fit holds")
    return nonneg, sw


def hsi_cube_srf_normal(grid, tau, La, Ld, Xk, endmembers, kidx, frac, Tpix, sensor, meas, weights=None, damping=None,
                        outputs=_CUBE_NORMAL_OUTPUTS, n_nodes=8, T_range=None, interp_tol=1e-6, nonneg=False, sum_weight=0.0):
    """The per-pixel normal equations of fitting (Tpix, frac) to a measured cube under hsi_cube_srf's model, the atmosphere
    and kidx fixed: with r = cube(Tpix, frac) - meas on the bands that count (live, weight > 0),
      "cost"  sum_b w_b r_b^2, float64 [nPix] device;
      "grad"  J^T W r, float64 [nPix][1 + nMix], the unknowns in the order T, then the fractions;
      "hess"  J^T W J, float64 [nPix][(1 + nMix)(2 + nMix) / 2], the lower triangle by rows;
      "step"  the solution of (H + damping diag H) step = -grad, NaN where that matrix is not positive definite.
    meas: float32 [nB][nPix] device tensor; weights: [nB] or None (all 1); damping: float64 [nPix] device tensor, a number, or
    None (0). outputs: the keys wanted ("cost" is always computed). Other arguments, checks and nodes as hsi_cube_srf. A pixel
    whose temperature is not finite or lies outside the range is NaN in all its outputs. One kernel: rtx_srf_pixel_cube_normal.
    nonneg=True (rtx_srf_pixel_cube_normal_box): "step" is the box step of the fit inside T_range and frac >= 0
    (unknowns on a bound whose gradient points outward stay, a step that would leave the box is cut there and the rest
    re-solved), and the dict gains "active", int32 [nPix]: bit i set where unknown i (0: T, m: fraction m) ended on a bound.
    sum_weight > 0 (needs nonneg=True) adds the soft sum-to-one term sum_weight (sum_m frac_m - 1)^2 to cost, grad and hess;
    its unit is radiance^2: (band noise / tolerated deviation of the sum)^2. The term rides on the band loop: a sensor with no
    band (nB == 0) evaluates nothing, the term included, as the library entry does (cost, grad, hess 0, step NaN, active 0).
    With the defaults nothing changes."""
    lib = _lib.load()
    fn = "hsi_cube_srf_normal"
    outputs = tuple(outputs)
    if not outputs or any(k not in _CUBE_NORMAL_OUTPUTS for k in outputs):
        raise ValueError("outputs: a non-empty selection of %r (got %r)" % (_CUBE_NORMAL_OUTPUTS, outputs))
    nonneg, sum_weight = _cube_box_args(fn, nonneg, sum_weight, kidx)
    f = _srf_cube_front(fn, grid, tau, La, Ld, Xk, endmembers, kidx, frac, Tpix, sensor, n_nodes, T_range, interp_tol)
    w = _cube_fit_args(fn, sensor, f["kidx"], meas, weights)
    endmembers, kidx, frac, Tpix, Q = f["endmembers"], f["kidx"], f["frac"], f["Tpix"], f["Q"]
    nPix, nMix = kidx.shape
    nU, nB, nEnd = 1 + nMix, len(sensor), endmembers.shape[1]
    if damping is not None and torch.is_tensor(damping) and (tuple(damping.shape) != (nPix,) or damping.dtype != torch.float64):
        raise ValueError(f"{fn}: damping: float64 [nPix = {nPix}] or a number, got {damping.dtype} {tuple(damping.shape)}")
    if not meas.is_cuda:
        raise ValueError(f"{fn} takes device tensors (meas is not on a GPU)")
    dev = tau.device
    shapes = dict(cost=(nPix,), grad=(nPix, nU), hess=(nPix, nU * (nU + 1) // 2), step=(nPix, nU))
    out = {k: torch.empty(shapes[k], dtype=torch.float64, device=dev) for k in set(outputs) | {"cost"}}
    if nonneg:
        return _cube_normal_box(lib, f, sensor, grid, tau, La, Ld, meas, w, damping, outputs, out, sum_weight)
    if nPix == 0:
        return {k: out[k] for k in outputs}
    if nB == 0:
        return {k: out[k].zero_() if k != "step" else out[k].fill_(float("nan")) for k in outputs}
    lam = None
    if damping is not None:
        lam = damping.to(dev).contiguous() if torch.is_tensor(damping) else torch.full((nPix,), float(damping), dtype=torch.float64, device=dev)
    w = None if w is None else w.to(dev).contiguous()
    N, Cb, tab, T_host = _srf_cube_tables(grid, tau, La, Ld, f, sensor)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.rtx_srf_pixel_cube_normal(nB, Q, T_host.ctypes.data_as(C.c_void_p), p(N), p(Cb), p(tab), nEnd, nPix, nMix, p(kidx), p(frac),
                                             p(Tpix), p(meas.contiguous()), p(w), p(lam), p(out["cost"]), p(out.get("grad")), p(out.get("hess")),
                                             p(out.get("step")), st, 0))
    return {k: out[k] for k in outputs}


def _cube_normal_box(lib, f, sensor, grid, tau, La, Ld, meas, w, damping, outputs, out, sum_weight):
    """hsi_cube_srf_normal's device part under nonneg=True: rtx_srf_pixel_cube_normal_box on the same tables."""
    kidx, frac, Tpix, Q = f["kidx"], f["frac"], f["Tpix"], f["Q"]
    nPix, nMix = kidx.shape
    nB, nEnd, dev = len(sensor), f["endmembers"].shape[1], tau.device
    active = torch.zeros(nPix, dtype=torch.int32, device=dev)
    res = lambda: dict({k: out[k] for k in outputs}, active=active)
    if nPix == 0:
        return res()
    if nB == 0:  # no band: the library entry evaluates nothing, the pseudo-band included (documented above)
        for k in outputs:
            out[k].zero_() if k != "step" else out[k].fill_(float("nan"))
        return res()
    lam = None
    if damping is not None:
        lam = damping.to(dev).contiguous() if torch.is_tensor(damping) else torch.full((nPix,), float(damping), dtype=torch.float64, device=dev)
    w = None if w is None else w.to(dev).contiguous()
    N, Cb, tab, T_host = _srf_cube_tables(grid, tau, La, Ld, f, sensor)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.rtx_srf_pixel_cube_normal_box(nB, Q, T_host.ctypes.data_as(C.c_void_p), p(N), p(Cb), p(tab), nEnd, nPix, nMix, p(kidx),
                                                 p(frac), p(Tpix), p(meas.contiguous()), p(w), p(lam), p(out["cost"]), p(out.get("grad")),
                                                 p(out.get("hess")), p(out.get("step")), st, 0, sum_weight, p(active)))
    return res()


def hsi_cube_srf_fit(grid, tau, La, Ld, Xk, endmembers, kidx, meas, sensor, T_range, frac0=None, T0=None, weights=None, max_iter=50,
                     lambda0=1e-3, ftol=0.0, n_nodes=8, interp_tol=1e-6, nonneg=False, sum_weight=0.0):
    """Fit every pixel's surface temperature and fractions to a measured cube under hsi_cube_srf's model, the atmosphere
    (tau, La, Ld) and the pixel's endmember indices kidx fixed: an unconstrained Levenberg-Marquardt loop per
    pixel in 1 + nMix unknowns, the whole loop in one kernel (rtx_srf_pixel_cube_fit; include/radtxfr_hip.h has the
    algorithm step by step). meas: float32 [nB][nPix] device tensor; weights [nB] or None (all 1): a band counts when it is
    live and its weight is > 0, and what meas holds under any other band is never read.
    T_range = (T_lo, T_hi) is required: the nodes span it and T never leaves it. frac0 [nPix][nMix] float32 and T0 [nPix]
    float64 (both or neither): the start; without them every pixel starts from the best of the n_nodes node temperatures
    with the fractions that minimise the cost there. max_iter trials at most (0 .. the library's 1000), lambda0 the first
    damping, ftol the relative decrease of the cost below which an accepted step is the last (0: never).
    Returns a dict of device tensors: "Tpix" float64 [nPix], "frac" float32 [nPix][nMix], "cost" float64 [nPix] (sum of
    w r^2), "n_iter" int32 [nPix] trials, "status" int32 [nPix] (0 converged or stalled, 1 iteration cap, 2 the start is
    outside T_range or not finite, 3 singular; under 2 and 3 the pixel's results are NaN), "hess" float64
    [nPix][(1 + nMix)(2 + nMix) / 2] = J^T W J at the result, lower triangle by rows: with nU = 1 + nMix unknowns and n
    counting bands, inv(hess) cost / (n - nU) estimates the covariance of (T, frac). All checks run before any device work.
    nonneg=True (rtx_srf_pixel_cube_fit_box) fits inside the box T_range x frac >= 0: every trial is the box step
    (see hsi_cube_srf_normal), a given start's fractions are raised to 0 first, and a pixel whose step no longer moves it
    stops with status 0. sum_weight > 0 (needs nonneg=True) adds sum_weight (sum_m frac_m - 1)^2 to the cost, a soft
    sum-to-one; its unit is radiance^2, so a sensible value is (band noise / tolerated deviation of the sum)^2, times the
    band weights' scale when weights are given. The dict gains "grad" float64 [nPix][1 + nMix], the gradient at the result,
    and "active" int32 [nPix]: bit i set where unknown i (0: T, m: fraction m) sits on a bound with the gradient pointing
    out of the box (the KKT active set). The covariance estimate then holds for the free unknowns only: invert hess with
    the rows and columns of the active unknowns removed, and count nU as the number of free ones. With the defaults the
    unconstrained entry is called and nothing changes."""
    lib = _lib.load()
    fn = "hsi_cube_srf_fit"
    nonneg, sum_weight = _cube_box_args(fn, nonneg, sum_weight, kidx)
    if T_range is None:
        raise ValueError(f"{fn}: T_range=(T_lo, T_hi) is required (there is no Tpix to read it from)")
    if (frac0 is None) != (T0 is None):
        raise ValueError(f"{fn}: frac0 and T0 come together (a start) or not at all (the node scan)")
    it_max = lib.rtx_srf_pixel_cube_fit_max_iter()
    if int(max_iter) != max_iter or not 0 <= max_iter <= it_max:
        raise ValueError(f"{fn}: max_iter={max_iter!r}: an integer from 0 to {it_max}")
    for name, v in (("lambda0", lambda0), ("ftol", ftol)):
        if not (np.isfinite(v) and v >= 0.0):
            raise ValueError(f"{fn}: {name}={v!r}: finite and not negative")
    given = frac0 is not None
    if not torch.is_tensor(kidx) or kidx.dim() != 2:
        raise ValueError(f"{fn}: kidx: int32 [nPix][nMix >= 1] tensor")
    # the start stands in for frac / Tpix in the shared checks; without one, host placeholders of the right shape do
    fr = frac0 if given else torch.empty(tuple(kidx.shape), dtype=torch.float32)
    Tp = T0 if given else torch.empty((kidx.shape[0],), dtype=torch.float64)
    f = _srf_cube_front(fn, grid, tau, La, Ld, Xk, endmembers, kidx, fr, Tp, sensor, n_nodes, T_range, interp_tol, need_device=False)
    w = _cube_fit_args(fn, sensor, f["kidx"], meas, weights)
    for name, v in (("tau", tau), ("endmembers", endmembers), ("kidx", kidx), ("meas", meas)) + ((("frac0", frac0), ("T0", T0)) if given else ()):
        if not v.is_cuda:
            raise ValueError(f"{fn} takes device tensors ({name} is not on a GPU)")
    endmembers, kidx, Q = f["endmembers"], f["kidx"], f["Q"]
    nPix, nMix = kidx.shape
    nU, nB, nEnd = 1 + nMix, len(sensor), endmembers.shape[1]
    dev = tau.device
    frac = f["frac"].clone() if given else torch.empty((nPix, nMix), dtype=torch.float32, device=dev)
    Tpix = f["Tpix"].clone() if given else torch.empty(nPix, dtype=torch.float64, device=dev)
    out = dict(Tpix=Tpix, frac=frac, cost=torch.empty(nPix, dtype=torch.float64, device=dev),
               n_iter=torch.zeros(nPix, dtype=torch.int32, device=dev), status=torch.zeros(nPix, dtype=torch.int32, device=dev),
               hess=torch.empty((nPix, nU * (nU + 1) // 2), dtype=torch.float64, device=dev))
    if nonneg:
        out["grad"] = torch.empty((nPix, nU), dtype=torch.float64, device=dev)
        out["active"] = torch.zeros(nPix, dtype=torch.int32, device=dev)
    if nPix == 0:
        return out
    if nB == 0:  # nothing to fit to
        for k in ("Tpix", "frac", "cost", "hess") + (("grad",) if nonneg else ()):
            out[k].fill_(float("nan"))
        out["status"].fill_(3)
        return out
    w = None if w is None else w.to(dev).contiguous()
    N, Cb, tab, T_host = _srf_cube_tables(grid, tau, La, Ld, f, sensor)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if nonneg:
        _lib.check(lib.rtx_srf_pixel_cube_fit_box(nB, Q, T_host.ctypes.data_as(C.c_void_p), p(N), p(Cb), p(tab), nEnd, nPix, nMix, p(kidx),
                                                  p(meas.contiguous()), p(w), p(frac), p(Tpix), int(max_iter), float(lambda0), float(ftol),
                                                  p(out["cost"]), p(out["n_iter"]), p(out["status"]), p(out["hess"]), st,
                                                  RTX_FIT_START_GIVEN if given else 0, sum_weight, p(out["grad"]), p(out["active"])))
        return out
    _lib.check(lib.rtx_srf_pixel_cube_fit(nB, Q, T_host.ctypes.data_as(C.c_void_p), p(N), p(Cb), p(tab), nEnd, nPix, nMix, p(kidx),
                                          p(meas.contiguous()), p(w), p(frac), p(Tpix), int(max_iter), float(lambda0), float(ftol), p(out["cost"]),
                                          p(out["n_iter"]), p(out["status"]), p(out["hess"]), st, RTX_FIT_START_GIVEN if given else 0))
    return out


def band_radiance(grid, tau, La, Ld, Xk, emis_knots, Ts, resFactor=None, keep_hires=False):
    """C4: L_b,k = ILS_MAKO( tau*(eps_k*B(Ts) + (1-eps_k)*Ld) + La ) for every emissivity column k.

    grid: engine.Grid of the monochromatic axis (e.g. the MAKO span of the C3 grid);
    tau, La, Ld: [grid.n] float32 device tensors; Xk [nk], emis_knots [nk][nE] float32 device; Ts scalar [K].
    Returns (X_out [nB] NumPy, L [nB][nE] float32 device). Three streaming kernels:
    rtx_interp_knots -> rtx_apparent_radiance -> rtx_ils."""
    dev = tau.device
    em = interp_knots(grid, Xk, emis_knots)  # [nX][nE]
    X_d = torch.as_tensor(grid.axis(), device=dev)
    Ts_d = torch.as_tensor(np.atleast_1d(np.asarray(Ts, dtype=np.float64)), device=dev)
    col = lambda v: v.reshape(-1, 1).contiguous()
    L, _ = engine.apparent_radiance(X_d, em, Ts_d, col(tau), col(La), col(Ld))
    L = L.reshape(grid.n, -1)  # [nX][nE] (nA = nT = 1)
    X_out, centre, sigma = mako_bands(grid.axis()[0], grid.axis()[-1], resFactor)
    out = engine.ils(0, L, torch.as_tensor(centre, device=dev), torch.as_tensor(sigma, device=dev), grid=grid)
    return (X_out, out, L) if keep_hires else (X_out, out)
