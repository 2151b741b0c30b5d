"""Host side of the fused band radiances under response tables (include/radtxfr_hip.h: rtx_srf_moments; sensor.
band_radiance_srf_fused): the fp64 yardstick of tests/srf_fused_cases.py against itself (direct form = moment form), the
inputs of the GPU parity test against their own float32 rounding, and the new ABI entries with the refusals they make
before any launch."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from radtxfr_amd import _lib, sensor

import sensor_cases as SC
import srf_fused_cases as FC


def test_direct_form_equals_moment_form_small():
    """A 40-point grid, 5 knots inside it (the end values are held on both sides), 3 emissivities, 2 temperatures; a band
    that reaches below the first knot and off the grid, one above the last knot, one between two knots, one with no point."""
    X = SC.grid_axis(1000.0, 1003.9, 40)
    r = np.random.default_rng(5)
    tau, La, Ld = r.uniform(0.3, 0.9, 40), r.uniform(0.5, 1.5, 40), r.uniform(1.0, 3.0, 40)
    Xk = np.array([1001.03, 1001.5, 1001.9, 1002.44, 1002.8])
    E = r.uniform(0.5, 1.0, (5, 3))
    tables = [(np.array([999.0, 1000.7, 1001.7]), np.array([0.2, 1.0, 0.0])),
              (np.array([1002.9, 1003.2, 1003.85]), np.array([1.0, 0.5, 1.0])),
              (np.array([1001.55, 1001.85]), np.array([1.0, 1.0])),
              (np.array([1000.0, 1002.0, 1004.5]), np.array([0.0, 1.0, 0.3])),
              (np.array([1000.11, 1000.19]), np.array([1.0, 1.0]))]
    Ts = [280.0, 320.0]
    N, Cb, M, jr = FC.moments(X, tables, tau, La, Ld, Xk, Ts)
    a, b = FC.direct_form(X, tables, tau, La, Ld, Xk, E, Ts), FC.moment_form(N, Cb, M, E)
    assert a.shape == b.shape == (2, 5, 3)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.all(np.isnan(a[:, 4])) and np.all(np.isfinite(a[:, :4]))
    assert np.max(np.abs(a[:, :4] / b[:, :4] - 1.0)) <= 1e-12
    assert jr.tolist() == [[0, 2], [4, 4], [1, 2], [0, 4], [0, -1]]
    assert N[4] == 0.0 and Cb[4] == 0.0 and not M[:, 4].any()
    for b_ in range(4):  # nothing outside the touched knots
        assert not M[:, b_, :jr[b_, 0]].any() and not M[:, b_, jr[b_, 1] + 1:].any()
    one = FC.moments(X, tables, tau, La, Ld, Xk[:1], Ts)  # one knot: the emissivity is a constant
    assert np.max(np.abs(FC.moment_form(one[0], one[1], one[2], E[:1])[:, :4] /
                         FC.direct_form(X, tables, tau, La, Ld, np.array([Xk[0], Xk[0] + 1.0]), E[[0, 0]], Ts)[:, :4] - 1.0)) <= 1e-12


@pytest.mark.parametrize("knots", FC.KNOT_SETS)
def test_gpu_case_yardstick(knots):
    """The inputs of the GPU parity test, checked here: the two forms agree to 1e-12 on them; the direct form on the
    float32-rounded tau / La / Ld stays within 1e-6 of the band maximum of itself on the fp64 ones, so input rounding takes
    at most a tenth of the 1e-5 parity bound; the NaN bands are the three meant to be."""
    lib = _lib.load()
    c = FC.case(lib.rtx_srf_chunk_points(), lib.rtx_srf_max_knots(), knots)
    assert len(c["tables"]) == 20 and c["X"].size == 3 * lib.rtx_srf_chunk_points() + 7
    assert 0.0 < c["tau"].min() and c["tau"].max() < 1.0 and c["La"].min() > 0.0 and c["Ld"].min() > 0.0
    assert c["Xk"][0] > c["X"][0] and c["Xk"][-1] < c["X"][-1]  # held ends on both sides
    live = ~c["dead"]
    assert np.array_equal(np.isnan(c["want"]), np.broadcast_to(c["dead"][None, :, None], c["want"].shape))
    mom = FC.moment_form(c["N"], c["C"], c["M"], c["E"])
    assert np.max(np.abs(mom[:, live] / c["want"][:, live] - 1.0)) <= 1e-12
    d64 = c["d64"]
    exact = FC.direct_form(c["X"], c["tables"], d64["tau"], d64["La"], d64["Ld"], c["Xk"], c["E"], FC.TS_LIST)
    e = float(np.max((np.abs(c["want"] - exact) / FC.band_max(exact))[:, live]))
    print("srf fused %s: float32 inputs move the fp64 result by %.3g of the band maximum" % (knots, e))
    assert e <= 1e-6
    assert np.all(c["jrange"][c["dead"]] == (0, -1)) and np.all(c["jrange"][live, 1] >= c["jrange"][live, 0])


def test_srf_moments_abi_symbols_and_refusals():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "radtxfr_hip.h")).read()
    for name in ("rtx_srf_moments", "rtx_srf_moments_max_temps"):
        assert name in _lib.PROTOTYPES and ("int %s(" % name) in header and hasattr(lib, name)
    assert hasattr(sensor, "band_radiance_srf_fused")
    MT = lib.rtx_srf_moments_max_temps()
    assert MT >= 1
    # refused before anything touches a device (the pointers are never read on the device)
    K = lib.rtx_srf_max_knots()
    buf = np.zeros(8)
    p = C.c_void_p(buf.ctypes.data)
    g = _lib.make_grid(900.0, 1000.0, 101)
    Ts = np.full(MT + 1, 300.0)

    def refused(text, start=(0, 3), nT=1, nk=5, nB=None, tau=p, out=p, Xk=p, Ts=Ts, grid=C.byref(g)):
        st = np.asarray(start, dtype=np.int32)
        rc = lib.rtx_srf_moments(grid, tau, p, p, Ts.ctypes.data_as(C.c_void_p) if Ts is not None else None, nT, Xk, nk,
                                 len(start) - 1 if nB is None else nB, st.ctypes.data_as(C.c_void_p), p, p, p, p, out, p, None)
        assert rc != 0 and text in lib.rtx_last_error().decode(), lib.rtx_last_error()

    refused("nT=", nT=0)
    refused("nT=", nT=MT + 1)
    refused("nT=", nT=-1)
    refused("ascending", start=(0, 3, 2))
    refused("ascending", start=(3, 0, 3))
    refused("at least 2", start=(0, 1))
    refused("at most", start=(0, 3, 3 + K + 1))
    refused("NULL", tau=None)
    refused("NULL", out=None)
    refused("NULL", Xk=None)
    refused("NULL", Ts=None)
    refused("nk=", nk=0)
    refused("nk=", nk=-3)
    refused("negative", nB=-1)
    refused("grid", grid=None)
    refused("temperature", Ts=np.array([300.0, 0.0]), nT=2)
    refused("temperature", Ts=np.array([np.nan]))
    assert lib.rtx_srf_moments(C.byref(g), None, None, None, None, 1, None, 5, 0, None, None, None, None, None, None, None, None) == 0  # nB == 0
