"""Host side of the per-pixel HSI cube under response tables (include/radtxfr_hip.h: rtx_srf_cube_tables, rtx_srf_pixel_cube;
sensor.hsi_cube_srf): the fp64 node form of tests/srf_cube_cases.py against the fp64 direct form on the GPU tests' scenes
(this pins the interpolation error, so that the GPU bound measures arithmetic only), sensor.planck_node_error and the
refusal it drives, and the new ABI entries with the refusals they make before any launch."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from radtxfr_amd import _lib, engine, sensor

import srf_cube_cases as CC
import srf_fused_cases as FC


def _case(knots):
    lib = _lib.load()
    return FC.case(lib.rtx_srf_chunk_points(), lib.rtx_srf_max_knots(), knots)


@pytest.mark.parametrize("tname", list(CC.T_CONFIGS))
@pytest.mark.parametrize("sname", list(CC.SCENES))
@pytest.mark.parametrize("knots", CC.KNOTS)
def test_node_form_against_direct_form(knots, sname, tname):
    """Interpolating Planck in temperature through 8 nodes over 230-350 K, or 5 over 285-315 K, moves no band radiance of
    the GPU tests' scenes by more than 1e-6 of the band's largest |L| (predicted at 930 cm^-1: <= 1e-7). Dead bands are
    NaN in both forms. MEASURED (fp64 NumPy): 230-350_Q8 1.9e-8 to 2.0e-8, 285-315_Q5 2.2e-8 to 2.3e-8."""
    c = _case(knots)
    s = CC.case(c, knots, sname, tname)
    assert s["want"].shape == s["node"].shape == (20, CC.NPIX)
    assert s["T"].min() == s["T_range"][0] and s["T"].max() == s["T_range"][1]  # both ends of the range are in the scene
    assert np.array_equal(np.isnan(s["want"]), np.broadcast_to(c["dead"][:, None], s["want"].shape))
    e = CC.worst(s["node"], s["want"], c["dead"])
    print("srf cube node form vs direct form %s %s %s: %.3g of the band maximum" % (knots, sname, tname, e))
    assert e <= 1e-6


def test_nodes_and_weights():
    """sensor.srf_cube_nodes gives the issue's nodes; the product-form weights sum to 1 and are 1 / 0 at a node."""
    for (T_range, Q) in CC.T_CONFIGS.values():
        Tq = sensor.srf_cube_nodes(T_range[0], T_range[1], Q)
        assert np.array_equal(Tq, CC.nodes(T_range, Q)) and np.all(np.diff(Tq) < 0)
        assert T_range[0] < Tq.min() and Tq.max() < T_range[1]  # Chebyshev nodes lie inside their range
        w = CC.lagrange(np.linspace(T_range[0], T_range[1], 101), Tq)
        assert np.max(np.abs(w.sum(axis=1) - 1.0)) <= 1e-12
        assert np.array_equal(CC.lagrange(Tq, Tq), np.eye(Q))


def test_planck_node_error_table():
    """The 230-350 K, 1400 cm^-1 entries of the issue's table (Q = 6: 5.1e-6, Q = 8: 5.5e-8) within a factor 2, and the
    ordering the table shows: worse for wider ranges, for higher wavenumbers and for fewer nodes."""
    e6, e8 = sensor.planck_node_error(1400.0, 230.0, 350.0, 6), sensor.planck_node_error(1400.0, 230.0, 350.0, 8)
    print("planck_node_error 230-350 K at 1400 cm^-1: Q=6 %.3g, Q=8 %.3g" % (e6, e8))
    assert 5.1e-6 / 2 <= e6 <= 5.1e-6 * 2 and 5.5e-8 / 2 <= e8 <= 5.5e-8 * 2
    assert sensor.planck_node_error(1400.0, 285.0, 315.0, 6) < e6 < sensor.planck_node_error(3000.0, 230.0, 350.0, 6)
    assert sensor.planck_node_error(1400.0, 230.0, 350.0, 4) > e6


def _stub_call(**kw):
    """hsi_cube_srf on host tensors: every check up to the interpolation estimate runs before any device work."""
    X = FC.axis(1024)
    nk, nEnd, nPix, nMix = 5, 3, 4, 2
    z = torch.zeros(X.size, dtype=torch.float32)
    args = dict(endmembers=torch.zeros((nk, nEnd), dtype=torch.float32), kidx=torch.zeros((nPix, nMix), dtype=torch.int32),
                frac=torch.zeros((nPix, nMix), dtype=torch.float32), Tpix=torch.full((nPix,), 300.0, dtype=torch.float64))
    opts = dict(n_nodes=8, T_range=(230.0, 350.0))
    for k, v in kw.items():
        (args if k in args else opts)[k] = v
    s = sensor.Sensor.from_shape([910.0, 920.0], 4.0, "boxcar")
    return sensor.hsi_cube_srf(engine.Grid(*FC.grid_tuple(1024)), z, z, z, np.linspace(905.0, 925.0, nk), args["endmembers"], args["kidx"],
                               args["frac"], args["Tpix"], s, **opts)


def test_refusal_by_interpolation_estimate():
    """(230, 350) K with 4 nodes is refused at the default interp_tol, with the estimate and the three ways out in the
    message; with 8 nodes the estimate passes and the stub tensors are refused for not being on a device instead."""
    with pytest.raises(ValueError) as ei:
        _stub_call(n_nodes=4)
    msg = str(ei.value)
    est = sensor.planck_node_error(FC.axis(1024)[-1], 230.0, 350.0, 4)
    assert est > 1e-6 and ("%.3g" % est) in msg
    assert "narrow T_range" in msg and "raise n_nodes" in msg and "split the scene" in msg
    with pytest.raises(ValueError, match="device tensors"):
        _stub_call(n_nodes=8)
    with pytest.raises(ValueError, match="device tensors"):
        _stub_call(n_nodes=4, interp_tol=1e-3)
    with pytest.raises(ValueError, match="device tensors"):
        _stub_call(n_nodes=4, T_range=(299.9, 300.0))  # narrower than 1 K: widened to 1 K, where 4 nodes pass


def test_argument_checks_come_first():
    lib = _lib.load()
    for kw, text in ((dict(n_nodes=0), "n_nodes"), (dict(n_nodes=lib.rtx_srf_cube_max_nodes() + 1), "n_nodes"), (dict(n_nodes=2.5), "n_nodes"),
                     (dict(T_range=(350.0, 230.0)), "T_range"), (dict(T_range=(0.0, 300.0)), "T_range"),
                     (dict(T_range=(230.0, float("nan"))), "T_range"),
                     (dict(kidx=torch.zeros((4, 2), dtype=torch.int64)), "kidx"), (dict(frac=torch.zeros((4, 3), dtype=torch.float32)), "frac"),
                     (dict(Tpix=torch.zeros(4, dtype=torch.float32)), "Tpix"), (dict(Tpix=torch.zeros(5, dtype=torch.float64)), "Tpix"),
                     (dict(endmembers=torch.zeros((4, 3), dtype=torch.float32)), "endmembers"),
                     (dict(T_range=None), "device tensors")):
        with pytest.raises(ValueError, match=text):
            _stub_call(**kw)


def test_abi_symbols_and_refusals():
    """The three names are in PROTOTYPES, declared in the header and exported with their argument counts; what the two
    entries refuse, they refuse before anything touches a device (the pointers are host memory, never read there)."""
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "radtxfr_hip.h")).read()
    for name, n_args in (("rtx_srf_cube_max_nodes", 0), ("rtx_srf_cube_tables", 9), ("rtx_srf_pixel_cube", 14)):
        assert name in _lib.PROTOTYPES and ("int %s(" % name) in header and hasattr(lib, name)
        assert len(_lib.PROTOTYPES[name][1]) == n_args
        decl = header.split("int %s(" % name)[1].split(");")[0]
        assert (decl.count(",") + 1 if decl.strip() != "void" else 0) == n_args
    assert hasattr(sensor, "hsi_cube_srf") and hasattr(sensor, "planck_node_error")
    QM = lib.rtx_srf_cube_max_nodes()
    assert QM == 8 == lib.rtx_srf_moments_max_temps()
    buf = np.zeros(64)
    p = C.c_void_p(buf.ctypes.data)

    def tables(text, M=p, jr=p, nB=2, Q=2, nk=5, E=p, nEnd=3, tab=p):
        rc = lib.rtx_srf_cube_tables(M, jr, nB, Q, nk, E, nEnd, tab, None)
        assert rc != 0 and text in lib.rtx_last_error().decode(), lib.rtx_last_error()

    tables("Q=", Q=0)
    tables("Q=", Q=QM + 1)
    tables("nk=", nk=0)
    tables("negative", nB=-1)
    tables("negative", nEnd=-1)
    for k in ("M", "jr", "E", "tab"):
        tables("NULL", **{k: None})
    assert lib.rtx_srf_cube_tables(None, None, 0, 2, 5, None, 3, None, None) == 0
    assert lib.rtx_srf_cube_tables(None, None, 2, 2, 5, None, 0, None, None) == 0

    good = np.array([310.0, 290.0, 285.0, 315.0])  # two nodes, then the range

    def pixels(text, nB=2, Q=2, T=good, N=p, Cb=p, tab=p, nEnd=3, nPix=4, nMix=2, kidx=p, frac=p, Tpix=p, cube=p):
        T = None if T is None else np.ascontiguousarray(T, dtype=np.float64)
        rc = lib.rtx_srf_pixel_cube(nB, Q, None if T is None else T.ctypes.data_as(C.c_void_p), N, Cb, tab, nEnd, nPix, nMix, kidx, frac,
                                    Tpix, cube, None)
        assert rc != 0 and text in lib.rtx_last_error().decode(), lib.rtx_last_error()

    pixels("Q=", Q=0)
    pixels("Q=", Q=QM + 1, T=np.linspace(300.0, 310.0, QM + 3))
    pixels("negative", nB=-1)
    pixels("negative", nPix=-1)
    pixels("nEnd=", nEnd=0)
    pixels("nMix=", nMix=0)
    pixels("NULL", T=None)
    for k in ("N", "Cb", "tab", "kidx", "frac", "Tpix", "cube"):
        pixels("NULL", **{k: None})
    pixels("node temperature", T=[310.0, np.nan, 285.0, 315.0])
    pixels("node temperature", T=[310.0, np.inf, 285.0, 315.0])
    pixels("node temperature", T=[310.0, -290.0, 285.0, 315.0])
    pixels("node temperature", T=[310.0, 0.0, 285.0, 315.0])
    pixels("outside the range", T=[310.0, 284.0, 285.0, 315.0])
    pixels("not distinct", T=[300.0, 300.0, 285.0, 315.0])
    pixels("not distinct", Q=3, T=[310.0, 290.0, 310.0, 285.0, 315.0])
    pixels("range", T=[310.0, 290.0, 315.0, 285.0])
    pixels("range", T=[310.0, 290.0, np.nan, 315.0])
    pixels("range", T=[310.0, 290.0, 285.0, np.inf])
    T = np.ascontiguousarray(good)
    assert lib.rtx_srf_pixel_cube(0, 2, T.ctypes.data_as(C.c_void_p), None, None, None, 3, 4, 2, None, None, None, None, None) == 0
    assert lib.rtx_srf_pixel_cube(2, 2, T.ctypes.data_as(C.c_void_p), None, None, None, 3, 0, 2, None, None, None, None, None) == 0
