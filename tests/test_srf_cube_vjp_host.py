"""CPU-only checks of the adjoint of the per-pixel HSI cube (include/radtxfr_hip.h: rtx_srf_pixel_cube_vjp;
sensor.hsi_cube_srf_vjp, rt.compute_hsi_cube_vjp): the fp64 oracle of tests/srf_cube_vjp_cases.py against central differences
of srf_cube_cases.node_cube itself, the identity the back half rests on (the cube is a linear combination of the band
radiances of [E | 0] at the nodes), the new ABI entry with the refusals it makes before any launch, and the argument checks
of the two Python entries that need no device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from radtxfr_amd import _lib, engine, sensor
from radtxfr_amd import radiative_transfer as rt

import srf_cube_cases as CC
import srf_cube_vjp_cases as VC
import srf_fused_cases as FC

STEP = 1e-6   # relative step of the central differences
AGREE = 1e-7  # of sum |g| band_max


def _case(knots):
    lib = _lib.load()
    return FC.case(lib.rtx_srf_chunk_points(), lib.rtx_srf_max_knots(), knots)


def _setup(knots, sname, tname):
    c = _case(knots)
    s = CC.case(c, knots, sname, tname)
    Tq = CC.nodes(s["T_range"], s["Q"])
    N, Cb, M, _ = CC.node_moments(c, knots, tname)
    sc = dict(kidx=np.array(s["kidx"]), frac=np.array(s["frac"]), T=np.array(s["T"]))
    g = VC.cotangent(20, CC.NPIX, c["dead"])
    return c, s, sc, Tq, N, Cb, M, g


def _costs(N, Cb, M, End, sc, Tq, g, live):
    """The per-pixel costs sum_b g[b][p] cube[b][p] over the live bands, fp64."""
    cube = CC.node_cube(N, Cb, M, End, sc, Tq)
    return np.sum(g[live].astype(np.float64) * cube[live], axis=0)


@pytest.mark.parametrize("tname", list(CC.T_CONFIGS))
@pytest.mark.parametrize("sname", list(CC.SCENES))
@pytest.mark.parametrize("knots", CC.KNOTS)
def test_oracle_against_central_differences(knots, sname, tname):
    """The analytic adjoint against central differences of node_cube in fp64, relative steps of 1e-6: x d cost / d x agrees
    to 1e-7 of sum |g| band_max for every pixel's T and every slot's fraction (per pixel: a pixel's column is its own), and,
    through gL contracted with d L / d End and d L / d C, for the endmember knots and the path term along random directions.
    MEASURED (fp64 NumPy), worst of the 8 cases, in units of sum |g| band_max: T 3.2e-10, frac 1.6e-10, End 4.2e-12,
    C 3.2e-12: a margin of 300."""
    c, s, sc, Tq, N, Cb, M, g = _setup(knots, sname, tname)
    live = ~c["dead"]
    End = np.array(s["End"]).astype(np.float64)
    nEnd = End.shape[1]
    G = M @ End
    o = VC.adjoint(N, G, sc, Tq, s["T_range"], g)
    bmax = np.max(np.abs(s["node"][live]), axis=1)
    S_p = np.sum(np.abs(g[live].astype(np.float64)) * bmax[:, None], axis=0)  # [nPix]
    S = float(S_p.sum())
    cost = lambda End_=End, sc_=sc, Cb_=Cb: _costs(N, Cb_, M, End_, sc_, Tq, g, live)
    # T: node_cube is a polynomial in T and knows no range, so the two pixels at the ends of the range step across them too
    T = sc["T"]
    h = STEP * T
    fd = (cost(sc_=dict(sc, T=T + h)) - cost(sc_=dict(sc, T=T - h))) / (2 * STEP)
    e_T = float(np.max(np.abs(fd - o["dT"] * T) / S_p))
    # frac: one slot at a time, all pixels at once
    e_f = 0.0
    for m in range(sc["frac"].shape[1]):
        f64 = sc["frac"].astype(np.float64)
        d = np.zeros_like(f64)
        d[:, m] = STEP * f64[:, m]
        fd = (cost(sc_=dict(sc, frac=f64 + d)) - cost(sc_=dict(sc, frac=f64 - d))) / (2 * STEP)
        e_f = max(e_f, float(np.max(np.abs(fd - o["dfrac"][:, m] * f64[:, m]) / S_p)))
    # the endmember knots and the path term, through gL: d cost = sum gL . dL, L = (C + M . [End | 0]) / N
    r = np.random.default_rng(31)
    gl = o["gL"][:, live]
    e_E = e_C = 0.0
    for _ in range(3):
        d = STEP * End * r.choice([-1.0, 1.0], End.shape)
        fd = float(np.sum(cost(End_=End + d) - cost(End_=End - d))) / (2 * STEP)
        an = float(np.sum(gl[:, :, :nEnd] * ((M[:, live] @ d) / N[live][None, :, None]))) / STEP
        e_E = max(e_E, abs(fd - an) / S)
        dC = STEP * Cb * r.choice([-1.0, 1.0], Cb.shape)
        fd = float(np.sum(cost(Cb_=Cb + dC) - cost(Cb_=Cb - dC))) / (2 * STEP)
        an = float(np.sum(gl * (dC[live] / N[live])[None, :, None])) / STEP
        e_C = max(e_C, abs(fd - an) / S)
    print("srf cube vjp oracle vs central differences %s %s %s: T %.3g, frac %.3g, End %.3g, C %.3g of sum |g| band_max"
          % (knots, sname, tname, e_T, e_f, e_E, e_C))
    assert max(e_T, e_f, e_E, e_C) <= AGREE
    assert np.all(o["gL"][:, c["dead"]] == 0.0) and np.all(o["gL"][1:, :, nEnd] == 0.0)


@pytest.mark.parametrize("tname", list(CC.T_CONFIGS))
def test_back_half_identity(tname):
    """What lets band_radiance_srf_vjp serve as the back half: with L = (C + M . [End | 0]) / N at the nodes (moment_form of
    srf_fused_cases.moments), sum_m f sum_q l_q L[q][b][k] + (1 - sum_m f) L[0][b][nEnd] is node_cube, to fp64 rounding; and
    the oracle's gL is the transpose of that combination: <gL, dL> = <g, d cube> for a random dL.
    MEASURED: the forward identity 5.3e-16 of the band maximum, the transpose 1.4e-15 relative."""
    c, s, sc, Tq, N, Cb, M, g = _setup("coarse", "mix3_of_8", tname)
    live = ~c["dead"]
    L = VC.band_radiances(N, Cb, M, s["End"])
    assert np.array_equal(L[:, :, :-1], FC.moment_form(N, Cb, M, s["End"]), equal_nan=True)
    assert np.array_equal(L[:, live, -1], np.broadcast_to(Cb[live] / N[live], (Tq.size, live.sum())))
    cube = VC.cube_from_radiances(L, sc, Tq)
    e = float(np.max(np.abs(cube[live] - s["node"][live]) / np.max(np.abs(s["node"][live]), axis=1, keepdims=True)))
    assert np.all(np.isnan(cube[c["dead"]]))
    o = VC.adjoint(N, M @ np.array(s["End"]).astype(np.float64), sc, Tq, s["T_range"], g)
    dL = np.random.default_rng(37).normal(size=L.shape)
    dcube = VC.cube_from_radiances(dL, sc, Tq)
    lhs, rhs = float(np.sum(o["gL"][:, live] * dL[:, live])), float(np.sum(g[live].astype(np.float64) * dcube[live]))
    print("srf cube vjp back half %s: forward identity %.3g of the band maximum, transpose %.3g relative" % (tname, e, abs(lhs - rhs) / abs(rhs)))
    assert e <= 1e-13 and abs(lhs - rhs) <= 1e-12 * abs(rhs)


def test_masks_of_the_oracle():
    """A NaN or out-of-range pixel is NaN in its own dT / dfrac and absent from gL; NaN in g on a dead band changes nothing."""
    c, s, sc, Tq, N, Cb, M, g = _setup("coarse", "mix3_of_8", "230-350_Q8")
    G = M @ np.array(s["End"]).astype(np.float64)
    sc["T"][3], sc["T"][70] = np.nan, np.nextafter(s["T_range"][1], np.inf)
    o = VC.adjoint(N, G, sc, Tq, s["T_range"], g)
    bad = np.zeros(CC.NPIX, dtype=bool)
    bad[[3, 70]] = True
    assert np.array_equal(np.isnan(o["dT"]), bad) and np.array_equal(np.isnan(o["dfrac"]).all(axis=1), bad)
    keep = {k: v[~bad] for k, v in sc.items()}
    o2 = VC.adjoint(N, G, keep, Tq, s["T_range"], g[:, ~bad])
    assert np.allclose(o["gL"], o2["gL"], rtol=1e-13, atol=0.0) and np.all(np.isfinite(o["gL"]))
    g0 = np.where(np.isnan(g), np.float32(1e30), g)
    assert np.array_equal(VC.adjoint(N, G, sc, Tq, s["T_range"], g0)["gL"], o["gL"])


# ------------------------------------------------------------------------------------------ the entries' refusals
def _stub_call(**kw):
    """hsi_cube_srf_vjp on host tensors: every check up to the interpolation estimate runs before any device work."""
    nk, nEnd, nPix, nMix = 5, 3, 4, 2
    z = torch.zeros(FC.axis(1024).size, dtype=torch.float32)
    args = dict(endmembers=torch.zeros((nk, nEnd), dtype=torch.float32), kidx=torch.zeros((nPix, nMix), dtype=torch.int32),
                frac=torch.zeros((nPix, nMix), dtype=torch.float32), Tpix=torch.full((nPix,), 300.0, dtype=torch.float64),
                g=torch.zeros((2, nPix), dtype=torch.float32))
    opts = dict(n_nodes=8, T_range=(230.0, 350.0))
    for k, v in kw.items():
        (args if k in args else opts)[k] = v
    s = sensor.Sensor.from_shape([910.0, 920.0], 4.0, "boxcar")
    return sensor.hsi_cube_srf_vjp(engine.Grid(*FC.grid_tuple(1024)), z, z, z, np.linspace(905.0, 925.0, nk), args["endmembers"], args["kidx"],
                                   args["frac"], args["Tpix"], s, args["g"], **opts)


def test_argument_checks_of_hsi_cube_srf_vjp():
    """hsi_cube_srf's checks, in its order, plus the cotangent's shape and dtype and the output keys: all before any device
    work (the stub tensors are host tensors, which is the last thing refused)."""
    for kw, text in ((dict(outputs=("Tpix", "emis")), "outputs"), (dict(outputs=()), "outputs"), (dict(n_nodes=0), "n_nodes"),
                     (dict(n_nodes=2.5), "n_nodes"), (dict(T_range=(350.0, 230.0)), "T_range"),
                     (dict(kidx=torch.zeros((4, 2), dtype=torch.int64)), "kidx"), (dict(frac=torch.zeros((4, 3), dtype=torch.float32)), "frac"),
                     (dict(Tpix=torch.zeros(4, dtype=torch.float32)), "Tpix"), (dict(endmembers=torch.zeros((4, 3), dtype=torch.float32)), "endmembers"),
                     (dict(g=torch.zeros((2, 5), dtype=torch.float32)), "g: float32"), (dict(g=torch.zeros((3, 4), dtype=torch.float32)), "g: float32"),
                     (dict(g=torch.zeros((2, 4), dtype=torch.float64)), "g: float32"), (dict(g=np.zeros((2, 4))), "g: float32"),
                     (dict(g=np.zeros((4, 2), dtype=np.float32)), "g: float32"), (dict(n_nodes=4), "narrow T_range"),
                     (dict(T_range=None), "device tensors"), (dict(), "device tensors"), (dict(outputs=("Tpix",)), "device tensors")):
        with pytest.raises(ValueError, match=text):
            _stub_call(**kw)


def test_argument_checks_of_compute_hsi_cube_vjp():
    """The refusals of compute_band_radiance_vjp, a scene or a cotangent of the wrong shape or dtype, a trailing vector axis,
    and hsi_cube_srf's interpolation estimate: before any device work (this machine has no device to touch)."""
    s = sensor.Sensor.from_shape([1000.1, 1000.3], 0.1, "triangle")
    Xk = np.linspace(1000.0, 1000.5, 5)
    nPix, nMix = 6, 2
    base = dict(End=np.full((5, 3), 0.9, dtype=np.float32), kidx=np.zeros((nPix, nMix), dtype=np.int32),
                frac=np.full((nPix, nMix), 0.5, dtype=np.float32), T=np.linspace(290.0, 310.0, nPix), g=np.ones((2, nPix), dtype=np.float32))
    kw = dict(DVOUT=0.0005, Altitudes=np.array([8.0]))

    def call(**k):
        a = dict(base)
        a.update({n: k.pop(n) for n in list(k) if n in a})
        return rt.compute_hsi_cube_vjp(1000.0, 1000.5, s, Xk, a["End"], a["kidx"], a["frac"], a["T"], a["g"], **dict(kw, **k))

    for exc, k in ((NotImplementedError, dict(Altitudes=np.array([0.5, 8.0]))), (NotImplementedError, dict(returnOD=True)),
                   (NotImplementedError, dict(xs_lut=object())), (NotImplementedError, dict(reduce=dict(dX=1.0))),
                   (NotImplementedError, dict(theta_r=np.array([0.0, 0.3]))), (NotImplementedError, dict(broadening="self")),
                   (ValueError, dict(wrt=("T", 99)))):
        with pytest.raises(exc, match="compute_hsi_cube_vjp"):
            call(**k)
    for k, text in ((dict(g=np.ones((3, nPix), dtype=np.float32)), "g: float32"), (dict(g=np.ones((2, nPix, 2), dtype=np.float32)), "one cotangent vector"),
                    (dict(g=np.ones((2, nPix + 1), dtype=np.float32)), "g: float32"), (dict(kidx=np.zeros((nPix, nMix))), "kidx has dtype"),
                    (dict(kidx=np.zeros(nPix, dtype=np.int32)), "kidx"), (dict(frac=np.zeros((nPix, 3), dtype=np.float32)), "frac"),
                    (dict(T=np.full(nPix + 1, 300.0)), "Tpix"), (dict(End=np.full((4, 3), 0.9, dtype=np.float32)), "endmembers"),
                    (dict(T=np.full(nPix, np.nan)), "finite Tpix"), (dict(n_nodes=9), "n_nodes"),
                    (dict(n_nodes=2, T_range=(230.0, 350.0)), "narrow T_range"), (dict(T_range=(310.0, 290.0)), "T_range")):
        with pytest.raises(ValueError, match=text):
            call(**k)


def test_abi_symbol_and_refusals():
    """rtx_srf_pixel_cube_vjp is in PROTOTYPES, declared in the header and exported with its 17 arguments (the stream, then flags); what it refuses, it
    refuses before anything touches a device (the pointers are host memory, never read there)."""
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "radtxfr_hip.h")).read()
    name = "rtx_srf_pixel_cube_vjp"
    assert name in _lib.PROTOTYPES and ("int %s(" % name) in header and hasattr(lib, name)
    decl = header.split("int %s(" % name)[1].split(");")[0]
    assert len(_lib.PROTOTYPES[name][1]) == decl.count(",") + 1 == 17
    assert hasattr(sensor, "hsi_cube_srf_vjp") and hasattr(rt, "compute_hsi_cube_vjp")
    QM = lib.rtx_srf_cube_max_nodes()
    buf = np.zeros(64)
    p = C.c_void_p(buf.ctypes.data)
    good = np.array([310.0, 290.0, 285.0, 315.0])  # two nodes, then the range

    def call(text, nB=2, Q=2, T=good, N=p, tab=p, nEnd=3, nPix=4, nMix=2, kidx=p, frac=p, Tpix=p, g=p, outs=(p, p, p), flags=0):
        T = None if T is None else np.ascontiguousarray(T, dtype=np.float64)
        rc = lib.rtx_srf_pixel_cube_vjp(nB, Q, None if T is None else T.ctypes.data_as(C.c_void_p), N, tab, nEnd, nPix, nMix, kidx, frac, Tpix,
                                        g, *outs, None, flags)
        assert rc != 0 and text in lib.rtx_last_error().decode(), lib.rtx_last_error()

    call("Q=", Q=0)
    call("Q=", Q=QM + 1, T=np.linspace(300.0, 310.0, QM + 3))
    call("negative", nB=-1)
    call("negative", nPix=-1)
    call("nEnd=", nEnd=0)
    call("nMix=", nMix=0)
    call("NULL", T=None)
    for k in ("N", "tab", "kidx", "frac", "Tpix", "g"):
        call("NULL", **{k: None})
    call("no output", outs=(None, None, None))
    call("no output", outs=(None, None, None), nPix=0)
    call("flags", flags=1)
    call("node temperature", T=[310.0, np.nan, 285.0, 315.0])
    call("outside the range", T=[310.0, 284.0, 285.0, 315.0])
    call("not distinct", T=[300.0, 300.0, 285.0, 315.0])
    call("range", T=[310.0, 290.0, 315.0, 285.0])
