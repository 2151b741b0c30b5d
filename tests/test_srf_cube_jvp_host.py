"""CPU-only checks of the tangent of the per-pixel HSI cube (include/radtxfr_hip.h: rtx_srf_pixel_cube_jvp;
sensor.hsi_cube_srf_jvp, rt.compute_hsi_cube_jvp): the fp64 oracle of tests/srf_cube_jvp_cases.py against central differences
of srf_cube_cases.node_cube itself and against the adjoint's oracle (the transpose identity), the new ABI entry with the
refusals it makes before any launch, and the argument checks of the two Python entries that need no device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from radtxfr_amd import _lib, engine, sensor
from radtxfr_amd import radiative_transfer as rt

import srf_cube_cases as CC
import srf_cube_jvp_cases as JC
import srf_cube_vjp_cases as VC
import srf_fused_cases as FC

STEP = 1e-6   # relative step of the central differences
AGREE = 1e-7  # of the band maximum: DESIGN 4.25's figure for the same differences


def _case(knots):
    lib = _lib.load()
    return FC.case(lib.rtx_srf_chunk_points(), lib.rtx_srf_max_knots(), knots)


def _setup(knots, sname, tname):
    c = _case(knots)
    s = CC.case(c, knots, sname, tname)
    Tq = CC.nodes(s["T_range"], s["Q"])
    N, Cb, M, _ = CC.node_moments(c, knots, tname)
    sc = dict(kidx=np.array(s["kidx"]), frac=np.array(s["frac"]), T=np.array(s["T"]))
    return c, s, sc, Tq, N, Cb, M


@pytest.mark.parametrize("tname", list(CC.T_CONFIGS))
@pytest.mark.parametrize("sname", list(CC.SCENES))
@pytest.mark.parametrize("knots", CC.KNOTS)
def test_oracle_against_central_differences(knots, sname, tname):
    """The analytic tangent against central differences of node_cube in fp64, a relative step of 1e-6 along directions
    x * (+-1) that hold N: C, M and End (through dL = (dC + dM . [End | 0] + M . [dEnd | 0]) / N), frac and T, each alone and
    all together. Element by element, the difference is at most 1e-7 of the band's largest radiance (the directions are
    relative, so the tangent is of the cube's own size).
    MEASURED (fp64 NumPy), worst of the 8 cases, of the band maximum: C 1.9e-10, M 8.7e-10, End 1.3e-9, frac 2.1e-10, T 4.6e-10,
    all five together 9.6e-9: a margin of 10."""
    c, s, sc, Tq, N, Cb, M = _setup(knots, sname, tname)
    live = ~c["dead"]
    End = np.array(s["End"]).astype(np.float64)
    f64, T = sc["frac"].astype(np.float64), sc["T"]
    r = np.random.default_rng(41)
    sign = lambda x: x * r.choice([-1.0, 1.0], np.shape(x))
    d = dict(C=sign(Cb), M=sign(M), End=sign(End), frac=sign(f64), T=sign(T))
    bmax = np.max(np.abs(s["node"][live]), axis=1, keepdims=True)

    def cube(h, keys):
        mv = lambda x, k: x + h * d[k] if k in keys else x
        return CC.node_cube(N, mv(Cb, "C"), mv(M, "M"), mv(End, "End"), dict(sc, frac=mv(f64, "frac"), T=mv(T, "T")), Tq)[live]

    worst = {}
    for name, keys in [(k, (k,)) for k in d] + [("all", tuple(d))]:
        fd = (cube(STEP, keys) - cube(-STEP, keys)) / (2 * STEP)
        back = {k: d[k] for k in ("C", "M", "End") if k in keys}
        dL = JC.radiance_tangent(N, M, End, back.get("C"), back.get("M"), back.get("End"))[None] if back else None
        # node_cube is a polynomial in T and knows no range: the oracle is given a range the stepped pixels stay inside
        o = JC.tangent(N, M @ End, dL, sc, Tq, (1.0, 1e4), d["frac"][None] if "frac" in keys else None, d["T"][None] if "T" in keys else None)
        assert np.all(np.isnan(o["d_cube"][0][c["dead"]]))
        worst[name] = float(np.max(np.abs(fd - o["d_cube"][0][live]) / bmax))
    print("srf cube jvp oracle vs central differences %s %s %s: %s of the band maximum"
          % (knots, sname, tname, ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert max(worst.values()) <= AGREE


@pytest.mark.parametrize("tname", list(CC.T_CONFIGS))
@pytest.mark.parametrize("sname", list(CC.SCENES))
def test_transpose_of_the_adjoint_oracle(sname, tname):
    """<g, d_cube> = <dT, d_Tpix> + <dfrac, d_frac> + <gL, dL> with srf_cube_vjp_cases.adjoint, over the live bands and the
    admitted pixels, with three dead bands, a NaN pixel and a pixel just outside the range in the scene, g and dL NaN under
    the dead bands, two vectors. MEASURED: at most 3.9e-17 of the sum of the absolute values of the terms (asserted 1e-13)."""
    c, s, sc, Tq, N, Cb, M = _setup("coarse", sname, tname)
    sc["T"][3], sc["T"][70] = np.nan, np.nextafter(s["T_range"][1], np.inf)
    ok = VC.admitted(sc["T"], s["T_range"])
    assert (~ok).sum() == 2 and c["dead"].sum() == 3
    live = ~c["dead"]
    G = M @ np.array(s["End"]).astype(np.float64)
    nMix, nEnd = CC.SCENES[sname]
    g = VC.cotangent(20, CC.NPIX, c["dead"])
    dL, d_frac, d_Tpix = JC.directions(2, 20, Tq.size, nEnd, CC.NPIX, nMix, c["dead"])
    a = VC.adjoint(N, G, sc, Tq, s["T_range"], g)
    o = JC.tangent(N, G, dL, sc, Tq, s["T_range"], d_frac, d_Tpix)
    assert np.array_equal(np.isnan(o["d_cube"]), np.broadcast_to(~(live[:, None] & ok[None, :]), o["d_cube"].shape))
    for v in range(2):
        lhs = float(np.sum(g[live][:, ok].astype(np.float64) * o["d_cube"][v][live][:, ok]))
        terms = [a["dT"][ok] * d_Tpix[v][ok], a["dfrac"][ok] * d_frac[v][ok].astype(np.float64), a["gL"][:, live] * dL[v][:, live].astype(np.float64)]
        rhs = float(sum(np.sum(t) for t in terms))
        size = float(sum(np.sum(np.abs(t)) for t in terms))
        print("srf cube jvp transpose %s %s vector %d: |lhs - rhs| = %.3g of sum |terms|" % (sname, tname, v, abs(lhs - rhs) / size))
        assert abs(lhs - rhs) <= 1e-13 * size


# ------------------------------------------------------------------------------------------ the entries' refusals
def _stub_call(**kw):
    """hsi_cube_srf_jvp on host tensors: every check runs before any device work."""
    nk, nEnd, nPix, nMix = 5, 3, 4, 2
    nX = FC.axis(1024).size
    z = torch.zeros(nX, dtype=torch.float32)
    args = dict(endmembers=torch.zeros((nk, nEnd), dtype=torch.float32), kidx=torch.zeros((nPix, nMix), dtype=torch.int32),
                frac=torch.zeros((nPix, nMix), dtype=torch.float32), Tpix=torch.full((nPix,), 300.0, dtype=torch.float64))
    opts = dict(n_nodes=8, T_range=(230.0, 350.0), d_Tpix=np.zeros(nPix))
    for k, v in kw.items():
        (args if k in args else opts)[k] = v
    s = sensor.Sensor.from_shape([910.0, 920.0], 4.0, "boxcar")
    return sensor.hsi_cube_srf_jvp(engine.Grid(*FC.grid_tuple(1024)), z, z, z, np.linspace(905.0, 925.0, nk), args["endmembers"], args["kidx"],
                                   args["frac"], args["Tpix"], s, **opts)


def test_argument_checks_of_hsi_cube_srf_jvp():
    """hsi_cube_srf's checks, in its order, then the tangents' shapes and their vector axis: all before any device work
    (the stub tensors are host tensors, which is the last thing refused)."""
    nX = FC.axis(1024).size
    for kw, text in ((dict(n_nodes=0), "n_nodes"), (dict(n_nodes=2.5), "n_nodes"), (dict(T_range=(350.0, 230.0)), "T_range"),
                     (dict(kidx=torch.zeros((4, 2), dtype=torch.int64)), "kidx"), (dict(frac=torch.zeros((4, 3), dtype=torch.float32)), "frac"),
                     (dict(Tpix=torch.zeros(4, dtype=torch.float32)), "Tpix"), (dict(endmembers=torch.zeros((4, 3), dtype=torch.float32)), "endmembers"),
                     (dict(n_nodes=4), "narrow T_range"),
                     (dict(d_Tpix=None), "no tangent"), (dict(d_Tpix=np.zeros(5)), "d_Tpix has shape"),
                     (dict(d_frac=np.zeros((4, 3), dtype=np.float32)), "d_frac has shape"),
                     (dict(d_endmembers=np.zeros((5, 3, 0), dtype=np.float32)), "d_endmembers has shape"),
                     (dict(d_tau=np.zeros(nX + 1, dtype=np.float32)), "d_tau has shape"),
                     (dict(d_La=torch.zeros((2, nX))), "d_La has shape"), (dict(d_Ld=np.zeros((nX, 2, 2))), "d_Ld has shape"),
                     (dict(d_frac=np.zeros((4, 2, 3), dtype=np.float32)), "disagree on the vector axis"),
                     (dict(d_Tpix=np.zeros((4, 2)), d_tau=np.zeros((nX, 3), dtype=np.float32)), "disagree on the vector axis"),
                     (dict(T_range=None), "device tensors"), (dict(), "device tensors"),
                     (dict(d_Tpix=np.zeros((4, 3)), d_frac=np.zeros((4, 2, 3), dtype=np.float32)), "device tensors")):
        with pytest.raises(ValueError, match=text):
            _stub_call(**kw)


def test_argument_checks_of_compute_hsi_cube_jvp():
    """The refusals of compute_hsi_cube_vjp, a scene or a tangent of the wrong shape or dtype, an unknown key, tangents
    that disagree on the vector axis, and hsi_cube_srf's interpolation estimate: before any device work (this machine has
    no device to touch)."""
    s = sensor.Sensor.from_shape([1000.1, 1000.3], 0.1, "triangle")
    Xk = np.linspace(1000.0, 1000.5, 5)
    nPix, nMix = 6, 2
    base = dict(End=np.full((5, 3), 0.9, dtype=np.float32), kidx=np.zeros((nPix, nMix), dtype=np.int32),
                frac=np.full((nPix, nMix), 0.5, dtype=np.float32), T=np.linspace(290.0, 310.0, nPix), tangents={"Tpix": np.ones(nPix)})
    kw = dict(DVOUT=0.0005, Altitudes=np.array([8.0]))

    def call(**k):
        a = dict(base)
        a.update({n: k.pop(n) for n in list(k) if n in a})
        return rt.compute_hsi_cube_jvp(1000.0, 1000.5, s, Xk, a["End"], a["kidx"], a["frac"], a["T"], a["tangents"], **dict(kw, **k))

    for exc, k in ((NotImplementedError, dict(Altitudes=np.array([0.5, 8.0]))), (NotImplementedError, dict(returnOD=True)),
                   (NotImplementedError, dict(xs_lut=object())), (NotImplementedError, dict(reduce=dict(dX=1.0))),
                   (NotImplementedError, dict(theta_r=np.array([0.0, 0.3]))), (NotImplementedError, dict(broadening="self")),
                   (ValueError, dict(tangents={})), (ValueError, dict(tangents=None)), (ValueError, dict(tangents={"emis": np.ones(3)})),
                   (ValueError, dict(tangents={"T": np.ones(3), 99: np.ones(3)}))):
        with pytest.raises(exc, match="compute_hsi_cube_jvp"):
            call(**k)
    for k, text in ((dict(tangents={"Tpix": np.ones(nPix + 1)}), "tangent \"Tpix\" has shape"),
                    (dict(tangents={"frac": np.ones((nPix, 3))}), "tangent \"frac\" has shape"),
                    (dict(tangents={"endmembers": np.ones((5, 3), dtype=complex)}), "has dtype"),
                    (dict(tangents={"endmembers": np.ones((5, 4))}), "tangent \"endmembers\" has shape"),
                    (dict(tangents={"Tpix": np.ones((nPix, 2)), "frac": np.ones((nPix, nMix, 3))}), "disagree on the vector axis"),
                    (dict(tangents={"Tpix": np.ones(nPix), "frac": np.ones((nPix, nMix, 1))}), "disagree on the vector axis"),
                    (dict(kidx=np.zeros((nPix, nMix))), "kidx has dtype"),
                    (dict(kidx=np.zeros(nPix, dtype=np.int32)), "kidx"), (dict(frac=np.zeros((nPix, 3), dtype=np.float32)), "frac"),
                    (dict(T=np.full(nPix + 1, 300.0)), "Tpix"), (dict(End=np.full((4, 3), 0.9, dtype=np.float32)), "endmembers"),
                    (dict(T=np.full(nPix, np.nan)), "finite Tpix"), (dict(n_nodes=9), "n_nodes"),
                    (dict(n_nodes=2, T_range=(230.0, 350.0)), "narrow T_range"), (dict(T_range=(310.0, 290.0)), "T_range")):
        with pytest.raises(ValueError, match=text):
            call(**k)


def test_abi_symbol_and_refusals():
    """rtx_srf_pixel_cube_jvp is in PROTOTYPES, declared in the header and exported with its 18 arguments (the stream, then
    flags), next to rtx_srf_pixel_cube_jvp_max_vectors; what it refuses, it refuses before anything touches a device (the
    pointers are host memory, never read there)."""
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "radtxfr_hip.h")).read()
    name = "rtx_srf_pixel_cube_jvp"
    assert name in _lib.PROTOTYPES and ("int %s(" % name) in header and hasattr(lib, name)
    assert name + "_max_vectors" in _lib.PROTOTYPES and ("int %s_max_vectors(void);" % name) in header
    decl = header.split("int %s(" % name)[1].split(");")[0]
    assert len(_lib.PROTOTYPES[name][1]) == decl.count(",") + 1 == 18
    assert decl.rstrip().endswith("void* stream, unsigned flags")
    assert hasattr(sensor, "hsi_cube_srf_jvp") and hasattr(rt, "compute_hsi_cube_jvp")
    NV = lib.rtx_srf_pixel_cube_jvp_max_vectors()
    assert NV >= 1
    QM = lib.rtx_srf_cube_max_nodes()
    buf = np.zeros(64)
    p = C.c_void_p(buf.ctypes.data)
    good = np.array([310.0, 290.0, 285.0, 315.0])  # two nodes, then the range

    def call(text, nB=2, Q=2, T=good, N=p, tab=p, nEnd=3, nPix=4, nMix=2, kidx=p, frac=p, Tpix=p, tans=(p, p, p), n_vec=1, d_cube=p, flags=0):
        T = None if T is None else np.ascontiguousarray(T, dtype=np.float64)
        rc = lib.rtx_srf_pixel_cube_jvp(nB, Q, None if T is None else T.ctypes.data_as(C.c_void_p), N, tab, nEnd, nPix, nMix, kidx, frac, Tpix,
                                        *tans, n_vec, d_cube, None, flags)
        assert rc != 0 and text in lib.rtx_last_error().decode(), lib.rtx_last_error()

    call("Q=", Q=0)
    call("Q=", Q=QM + 1, T=np.linspace(300.0, 310.0, QM + 3))
    call("negative", nB=-1)
    call("negative", nPix=-1)
    call("nEnd=", nEnd=0)
    call("nMix=", nMix=0)
    call("NULL", T=None)
    for k in ("N", "tab", "kidx", "frac", "Tpix", "d_cube"):
        call("NULL", **{k: None})
    call("no tangent", tans=(None, None, None))
    call("no tangent", tans=(None, None, None), nPix=0)
    call("n_vec=", n_vec=0)
    call("n_vec=", n_vec=NV + 1)
    call("flags", flags=1)
    call("node temperature", T=[310.0, np.nan, 285.0, 315.0])
    call("outside the range", T=[310.0, 284.0, 285.0, 315.0])
    call("not distinct", T=[300.0, 300.0, 285.0, 315.0])
    call("range", T=[310.0, 290.0, 315.0, 285.0])
    assert np.all(buf == 0.0)
