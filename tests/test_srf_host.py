"""Host side of the tabulated spectral response functions (radtxfr_amd/sensor.py: Sensor, trapezoid_cells; include/
radtxfr_hip.h: rtx_srf_apply): table validation, the analytic shapes' tables, the MAKO tables against mako_bands, the
wavelength convenience, the trapezoid cells, and the new ABI entries with the refusals they make before any launch."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from radtxfr_amd import _lib, sensor
from radtxfr_amd.sensor import Sensor


def _tri(c=1000.0, s=5.0):
    return np.array([c - s, c, c + s]), np.array([0.0, 1.0, 0.0])


@pytest.mark.parametrize("x, r, text", [
    ([1.0, 1.0, 2.0], [0.0, 1.0, 0.0], "ascending"),
    ([1.0, 3.0, 2.0], [0.0, 1.0, 0.0], "ascending"),
    ([3.0, 2.0, 1.0], [0.0, 1.0, 0.0], "ascending"),
    ([1.0, np.nan, 3.0], [0.0, 1.0, 0.0], "ascending"),
    ([1.0, 2.0, 3.0], [0.0, -1e-3, 1.0], "response"),
    ([1.0, 2.0, 3.0], [0.0, np.nan, 1.0], "response"),
    ([1.0, 2.0, 3.0], [0.0, np.inf, 1.0], "response"),
    ([1.0, 2.0, 3.0], [0.0, 0.0, 0.0], "zero everywhere"),
    ([1.0], [1.0], "knots"),
    ([], [], "knots"),
    (np.arange(sensor.MAX_KNOTS + 1.0), np.ones(sensor.MAX_KNOTS + 1), "knots"),
    ([1.0, 2.0, 3.0], [1.0, 1.0], "responses"),
])
def test_from_tables_refuses(x, r, text):
    """Every refusal names the band (the second of two here)."""
    with pytest.raises(ValueError) as e:
        Sensor.from_tables([_tri(), (x, r)])
    assert "band 1" in str(e.value) and text in str(e.value)


def test_from_tables_accepts_and_freezes():
    x = np.arange(float(sensor.MAX_KNOTS))
    s = Sensor.from_tables([_tri(), (x, np.ones(x.size)), ([900.0, 910.0], [1, 1])])
    assert len(s) == 3 and list(s.knot_start) == [0, 3, 3 + sensor.MAX_KNOTS, 5 + sensor.MAX_KNOTS] and s.knot_start.dtype == np.int32
    assert s.tables[0][0].dtype == np.float64 and s.tables[0][1].dtype == np.float32
    # centres: the response-weighted mean wavenumber, exact for a piecewise-linear table
    assert np.allclose(s.centres, [1000.0, 0.5 * (sensor.MAX_KNOTS - 1), 905.0], rtol=1e-14)
    skew = Sensor.from_tables([([0.0, 1.0, 4.0], [0.0, 1.0, 0.0])])  # a skew triangle's centroid: the mean of its corners
    assert np.isclose(skew.centres[0], 5.0 / 3.0, rtol=1e-14)
    for a in (s.centres, s.knot_start, s.tables[0][0], s.tables[0][1]):
        with pytest.raises(ValueError):
            a[0] = 1
    given = Sensor.from_tables([_tri()], centres=[1001.0])
    assert given.centres[0] == 1001.0
    with pytest.raises(ValueError):
        Sensor.from_tables([_tri()], centres=[1.0, 2.0])


def test_from_shape_tables():
    c, f = np.array([900.0, 1000.0, 1234.5]), np.array([4.0, 10.0, 100.0])
    t = Sensor.from_shape(c, f, "triangle")
    b = Sensor.from_shape(c, f, "boxcar")
    for i in range(3):
        assert np.array_equal(t.tables[i][0], [c[i] - f[i], c[i], c[i] + f[i]]) and np.array_equal(t.tables[i][1], [0, 1, 0])
        assert np.array_equal(b.tables[i][0], [c[i] - 0.5 * f[i], c[i] + 0.5 * f[i]]) and np.array_equal(b.tables[i][1], [1, 1])
    assert np.array_equal(t.centres, c) and np.array_equal(b.centres, c)
    one = Sensor.from_shape(1000.0, 10.0, "boxcar")  # scalars: one band
    assert len(one) == 1
    for knots in (65, 33, 129):
        g = Sensor.from_shape(c, f, "gaussian", knots=knots)
        for i in range(3):
            x, r = g.tables[i]
            assert x.size == knots and x[0] == c[i] - 4 * f[i] and x[-1] == c[i] + 4 * f[i]
            assert np.array_equal(r, r[::-1]) and np.allclose(x - c[i], -(x - c[i])[::-1], rtol=0, atol=1e-9)  # symmetric
            assert r[knots // 2] == 1.0 and x[knots // 2] == c[i] and r.max() == 1.0             # peaks at 1 at the centre
            h = x[1] - x[0]
            above = x[r >= 0.5]                                                                 # half maximum at +- fwhm / 2
            assert abs(above[0] - (c[i] - 0.5 * f[i])) <= h and abs(above[-1] - (c[i] + 0.5 * f[i])) <= h
    with pytest.raises(ValueError):
        Sensor.from_shape(c, f, "lorentzian")
    with pytest.raises(ValueError):
        Sensor.from_shape(c, -1.0, "boxcar")


@pytest.mark.parametrize("kw", [{}, dict(resFactor=2), dict(fwhm_sf=1.3, shift=0.4, scale=1.0005)])
def test_mako_tables(kw):
    X_out, centre, sigma = sensor.mako_bands(760.0, 1340.0, **kw)
    s = Sensor.mako(760.0, 1340.0, **kw)
    assert len(s) == X_out.size > 100
    for b in range(len(s)):
        assert np.array_equal(s.tables[b][0], [centre[b] - sigma[b], centre[b], centre[b] + sigma[b]])
        assert np.array_equal(s.tables[b][1], [0.0, 1.0, 0.0])
    assert np.allclose(s.centres, centre, rtol=1e-12, atol=0)  # a symmetric triangle's weighted mean is its centre


def test_in_wavelength():
    lam = np.array([8.0, 8.5, 9.0, 10.0])      # ascending wavelength = descending wavenumber
    r = np.array([0.1, 0.7, 1.0, 0.2])
    for order in (slice(None), slice(None, None, -1)):
        s = Sensor.in_wavelength([(lam[order], r[order])])
        x, rr = s.tables[0]
        assert np.array_equal(x, (1.0e4 / lam)[::-1]) and np.all(np.diff(x) > 0)
        assert np.array_equal(rr, r[::-1].astype(np.float32))  # the values as given: no Jacobian factor
    assert "Jacobian" in Sensor.in_wavelength.__doc__


def test_trapezoid_cells():
    X = np.linspace(900.0, 901.0, 11)
    d = sensor.trapezoid_cells(X)
    assert np.allclose(d, np.gradient(X) * np.r_[0.5, np.ones(9), 0.5], rtol=1e-12) and np.allclose(d[1:-1], 0.1, rtol=1e-12) and np.allclose(d[[0, -1]], 0.05, rtol=1e-12)
    assert np.isclose(d.sum(), X[-1] - X[0], rtol=1e-14)  # the trapezoid rule's weights
    X = np.array([1.0, 2.0, 4.0, 4.5, 7.0])
    d = sensor.trapezoid_cells(X)
    assert np.array_equal(d, [0.5, 1.5, 1.25, 1.5, 1.25])
    Y = np.random.default_rng(0).uniform(1.0, 2.0, X.size)
    assert np.isclose(d @ Y, np.sum(0.5 * (Y[1:] + Y[:-1]) * np.diff(X)), rtol=1e-14)
    assert np.array_equal(sensor.trapezoid_cells([5.0]), [1.0])
    assert np.array_equal(sensor.trapezoid_cells([5.0, 5.5]), [0.25, 0.25])


def test_srf_abi_symbols_and_refusals():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "radtxfr_hip.h")).read()
    for name in ("rtx_srf_apply", "rtx_srf_chunk_points", "rtx_srf_max_knots"):
        assert name in _lib.PROTOTYPES and ("int %s(" % name) in header and hasattr(lib, name)
    assert lib.rtx_srf_max_knots() == sensor.MAX_KNOTS >= 1024
    assert lib.rtx_srf_chunk_points() >= 64
    # refused before anything touches a device (the pointers are never read on the device)
    K = lib.rtx_srf_max_knots()
    buf = np.zeros(8)
    p = C.c_void_p(buf.ctypes.data)
    g = _lib.make_grid(900.0, 1000.0, 101)

    def refused(start, text, nx=101, nS=4, ldY=4, nB=None, Y=p, grid=C.byref(g)):
        st = np.asarray(start, dtype=np.int32)
        rc = lib.rtx_srf_apply(grid, None, nx, Y, nS, ldY, len(start) - 1 if nB is None else nB, st.ctypes.data_as(C.c_void_p), p, p, p, None, None)
        assert rc != 0 and text in lib.rtx_last_error().decode(), lib.rtx_last_error()

    refused([0, 1], "at least 2")
    refused([0, 3, 3 + K + 1], "at most")
    refused([0, 3, 2], "ascending")
    refused([0, 3], "ldY", ldY=3)
    refused([0, 3], "negative", nS=-1)
    refused([0, 3], "negative", nB=-1)
    refused([0, 3], "NULL", Y=None)
    refused([0, 3], "nx=", nx=100)
    refused([0, 3], "grid", grid=None)
    st = np.array([0, 3], dtype=np.int32)
    assert lib.rtx_srf_apply(C.byref(g), None, 101, p, 0, 0, 1, st.ctypes.data_as(C.c_void_p), p, p, p, None, None) == 0  # nS == 0
    assert lib.rtx_srf_apply(C.byref(g), None, 101, p, 4, 4, 0, None, None, None, None, None, None) == 0               # nB == 0
