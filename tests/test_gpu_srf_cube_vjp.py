"""The adjoint of the per-pixel HSI cube (radtxfr_amd/csrc/rtx_srf_cube_vjp.hip: rtx_srf_pixel_cube_vjp; sensor.hsi_cube_srf_vjp,
rt.compute_hsi_cube_vjp) against the fp64 NumPy of tests/srf_cube_vjp_cases.py evaluated on the device's own float32 N and
table, against the shipped forward kernels, bit for bit against rtx_srf_radiance_vjp and against itself.

Grid, inputs, the 20 bands (three dead) and the knot sets are those of tests/srf_fused_cases.py, the scenes those of
tests/srf_cube_cases.py (257 pixels: ends inside a workgroup of 256, inside a round of 64 and one pixel into a second
chunk of 256). The cotangent is random of both signs and NaN on the dead bands throughout.

Bound of the oracle cases: |got - want| <= k 2^-24 scale, element by element, scale = the oracle's sum of the absolute
values of the same summands, k = the fp32 roundings along the kernel's chain (K_* below; everything not counted is fp64)."""
import ctypes as C

import numpy as np
import pytest

import sensor_vjp_cases as SV
import srf_cube_cases as CC
import srf_cube_vjp_cases as VC
import srf_fused_cases as FC
from test_gpu_sensor_vjp import K_DE, K_ROW, within

pytestmark = pytest.mark.gpu

# dfrac = sum_b x sum_q l_q G: the rounding of l_q to fp32 (1), the fmaf chain over the Q <= 8 nodes (one rounding per link,
# each relative to a partial sum the scale bounds: Q); x = u / N, the product and the sum over the bands are fp64 (1 for all)
K_DFRAC = lambda Q: Q + 2
# dT = sum_b x sum_m f sum_q l'_q G: the rounding of l'_q (1), the chain (Q), the rest fp64 (1)
K_DT = lambda Q: Q + 2
# gL = sum_p u l_q f: the rounding of l_q (1), the store (1), the fp64 products and sums (1 for all)
K_GL = 3
FIRST = ("coarse", "mix3_of_8", "230-350_Q8")
FWD_TOL = 1e-5  # tests/test_gpu_srf_cube.py: the forward's own asserted bound


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    from radtxfr_amd import _lib, engine, sensor
    lib = _lib.load()
    return dict(torch=torch, lib=lib, _lib=_lib, engine=engine, sensor=sensor, CH=lib.rtx_srf_chunk_points(), K=lib.rtx_srf_max_knots())


def fused_case(env, knots):
    return FC.case(env["CH"], env["K"], knots)


def dev(env, a):
    return env["torch"].as_tensor(np.array(a), device="cuda")  # a copy: the shared inputs are read-only


def grid_of(env):
    return env["engine"].Grid(*FC.grid_tuple(env["CH"]))


_TABLES = {}


def device_tables(env, c, knots, End, T_range, Q, times=1):
    """The device's own N [nB] and table [nEnd][Q][nB] (float32, device) at the nodes, with host copies: N and G [Q][nB][nEnd]
    float64, what the oracle is evaluated on. times: the case's 20 bands repeated that often."""
    key = (knots, End.shape[1], T_range, Q, times)
    if key not in _TABLES:
        torch, sensor, lib = env["torch"], env["sensor"], env["lib"]
        s = sensor.Sensor.from_tables(list(c["tables"]) * times)
        nodes = sensor.srf_cube_nodes(T_range[0], T_range[1], Q)
        N, Cb, M, jr = sensor.srf_moments(grid_of(env), dev(env, c["tau"]), dev(env, c["La"]), dev(env, c["Ld"]), dev(env, c["Xk"]), nodes, s)
        nB, nk, nEnd = len(s), c["Xk"].size, End.shape[1]
        tab = torch.empty((nEnd, Q, nB), dtype=torch.float32, device="cuda")
        p = lambda t: C.c_void_p(t.data_ptr())
        env["_lib"].check(lib.rtx_srf_cube_tables(p(M), p(jr), nB, Q, nk, p(dev(env, End)), nEnd, p(tab), None))
        torch.cuda.synchronize()
        T_host = np.ascontiguousarray(np.concatenate([nodes, list(T_range)]))
        _TABLES[key] = dict(N=N, tab=tab, T_host=T_host, nodes=nodes, N_h=N.cpu().numpy().astype(np.float64),
                            G_h=tab.cpu().numpy().astype(np.float64).transpose(1, 2, 0))
    return _TABLES[key]


def raw(env, t, sc, g, outs=("dT", "dfrac", "gL")):
    """rtx_srf_pixel_cube_vjp itself on the device tables t -> dict of NumPy."""
    torch, lib = env["torch"], env["lib"]
    nEnd, Q, nB = t["tab"].shape
    nPix, nMix = sc["kidx"].shape
    kidx, frac, T, g_d = dev(env, sc["kidx"]), dev(env, sc["frac"]), dev(env, sc["T"]), dev(env, g)
    assert g_d.dtype == torch.float32 and tuple(g_d.shape) == (nB, nPix)
    o = dict(dT=torch.empty(nPix, dtype=torch.float64, device="cuda"), dfrac=torch.empty((nPix, nMix), dtype=torch.float64, device="cuda"),
             gL=torch.empty((Q, nB, nEnd + 1), dtype=torch.float32, device="cuda"))
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    env["_lib"].check(lib.rtx_srf_pixel_cube_vjp(nB, Q, t["T_host"].ctypes.data_as(C.c_void_p), p(t["N"]), p(t["tab"]), nEnd, nPix, nMix, p(kidx),
                                                 p(frac), p(T), p(g_d), *[p(o[k]) if k in outs else None for k in ("dT", "dfrac", "gL")], st, 0))
    torch.cuda.synchronize()
    return {k: o[k].cpu().numpy() for k in outs}


def full(env, c, End, sc, g, Q, T_range, outputs=None, **over):
    """sensor.hsi_cube_srf_vjp on the device -> dict of NumPy. over: tau / La / Ld replaced."""
    torch, sensor = env["torch"], env["sensor"]
    s = sensor.Sensor.from_tables(c["tables"])
    kw = {} if outputs is None else dict(outputs=outputs)
    tau, La, Ld = (dev(env, over.get(k, c[k])) for k in ("tau", "La", "Ld"))
    out = sensor.hsi_cube_srf_vjp(grid_of(env), tau, La, Ld, c["Xk"], dev(env, End), dev(env, sc["kidx"]), dev(env, sc["frac"]), dev(env, sc["T"]),
                                  s, dev(env, g), n_nodes=Q, T_range=T_range, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def forward(env, c, End, sc, Q, T_range, **over):
    torch, sensor = env["torch"], env["sensor"]
    tau, La, Ld = (dev(env, over.get(k, c[k])) for k in ("tau", "La", "Ld"))
    _, cube = sensor.hsi_cube_srf(grid_of(env), tau, La, Ld, c["Xk"], dev(env, End), dev(env, sc["kidx"]), dev(env, sc["frac"]), dev(env, sc["T"]),
                                  sensor.Sensor.from_tables(c["tables"]), n_nodes=Q, T_range=T_range)
    torch.cuda.synchronize()
    return cube.cpu().numpy()


def cut(sc, sel):
    return dict(kidx=np.ascontiguousarray(sc["kidx"][sel]), frac=np.ascontiguousarray(sc["frac"][sel]), T=np.ascontiguousarray(sc["T"][sel]))


def check_raw(env, t, sc, T_range, g, what):
    """The three outputs of the entry against the oracle on the device's N and table."""
    Q = t["tab"].shape[1]
    got = raw(env, t, sc, g)
    o = VC.adjoint(t["N_h"], t["G_h"], sc, t["nodes"], T_range, g)
    assert got["dT"].dtype == got["dfrac"].dtype == np.float64 and got["gL"].dtype == np.float32
    within(got["dT"], o["dT"], o["scale"]["dT"], K_DT(Q), what + " dT")
    within(got["dfrac"], o["dfrac"], o["scale"]["dfrac"], K_DFRAC(Q), what + " dfrac")
    within(got["gL"], o["gL"], o["scale"]["gL"], K_GL, what + " gL")
    return got, o


_FIRST = {}


def first_case(env):
    """(fused case, cube case, device tables, g, the entry's outputs) of FIRST, run once."""
    if not _FIRST:
        c = fused_case(env, FIRST[0])
        s = CC.case(c, *FIRST)
        t = device_tables(env, c, FIRST[0], s["End"], s["T_range"], s["Q"])
        g = VC.cotangent(20, CC.NPIX, c["dead"])
        _FIRST["v"] = (c, s, t, g, raw(env, t, s, g))
    return _FIRST["v"]


# ---------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("tname", list(CC.T_CONFIGS))
@pytest.mark.parametrize("sname", list(CC.SCENES))
@pytest.mark.parametrize("knots", CC.KNOTS)
def test_against_oracle(env, knots, sname, tname):
    """Test 1: 257 pixels; mixtures of 3 out of 8 endmembers (the pixel kernel's table in LDS, one slice of the reduction) and
    of 6 out of 31 (table in global memory, 3 or 2 slices, two passes over the mixture); 8 nodes and 5. dT, dfrac and gL of the
    entry element by element, then the rows and the endmember gradient of sensor.hsi_cube_srf_vjp against
    sensor_vjp_cases.adjoint at the nodes with [E | 0] and the oracle's gL: the back half's K_ROW / K_DE plus K_GL, on the
    scale the same adjoint gives for the scale of gL.
    MEASURED on an MI355X, worst of the 8 cases, in units of 2^-24 scale: dT 0.42 (k = 10 / 7), dfrac 0.98, gL 0.99 (k = 3),
    G_tau 0.29 (k = 17), G_La 0.26 (k = 6), G_Ld 0.059 (k = 9), endmembers 0.65 (k = 35)."""
    c = fused_case(env, knots)
    s = CC.case(c, knots, sname, tname)
    t = device_tables(env, c, knots, s["End"], s["T_range"], s["Q"])
    g = VC.cotangent(20, CC.NPIX, c["dead"])
    what = "srf cube vjp %s %s %s" % (knots, sname, tname)
    got, o = check_raw(env, t, s, s["T_range"], g, what)
    out = full(env, c, s["End"], s, g, s["Q"], s["T_range"])
    assert set(out) == {"G_tau", "G_La", "G_Ld", "Tpix", "frac", "endmembers"}
    assert np.array_equal(out["Tpix"], got["dT"]) and np.array_equal(out["frac"], got["dfrac"])
    nk, nEnd = s["End"].shape
    E0 = np.concatenate([s["End"], np.zeros((nk, 1), dtype=np.float32)], axis=1)
    args = (c["X"], c["tables"], c["tau"], c["La"], c["Ld"], c["Xk"], E0, t["nodes"])
    b, bs = SV.adjoint(*args, o["gL"]), SV.adjoint(*args, o["scale"]["gL"])
    for key in ("G_tau", "G_La", "G_Ld"):
        assert out[key].dtype == np.float32 and out[key].shape == (c["X"].size,)
        within(out[key], b[key], bs["scale"][key], K_ROW[key] + K_GL, what + " " + key)
    assert out["endmembers"].dtype == np.float64 and out["endmembers"].shape == (nk, nEnd)
    within(out["endmembers"], b["dE"][:, :nEnd], bs["scale"]["dE"][:, :nEnd], K_DE + K_GL, what + " endmembers")


@pytest.mark.parametrize("nEnd,tname", ((16, "230-350_Q8"), (26, "285-315_Q5"), (14, "230-350_Q8"), (15, "230-350_Q8"), (22, "285-315_Q5"),
                                        (23, "285-315_Q5"), (400, "230-350_Q8")))
def test_table_sizes(env, nEnd, tname):
    """Test 1: nEnd x Q = 128 (the pixel kernel's largest table in LDS) and just above it (26 x 5); 14 / 15 endmembers of 8
    nodes and 22 / 23 of 5, where the reduction goes from one slice of at most 112 rows to two; the 400-endmember set: 29
    slices, and with 257 pixels two chunks. The scene mixes all nEnd endmembers.
    MEASURED: dT at most 0.42, dfrac 1.37, gL 1.83 (the 400-endmember set; the others at most 1.43)."""
    c = fused_case(env, "coarse")
    T_range, Q = CC.T_CONFIGS[tname]
    End = CC.endmembers(c["Xk"].size, nEnd)
    t = device_tables(env, c, "coarse", End, T_range, Q)
    sc = CC.scene(CC.NPIX if nEnd == 400 else 65, 3, nEnd, T_range, seed=11)
    assert sc["kidx"].max() >= min(nEnd - 1, 13)
    g = VC.cotangent(20, sc["T"].size, c["dead"], seed=12)
    check_raw(env, t, sc, T_range, g, "srf cube vjp nEnd=%d Q=%d" % (nEnd, Q))


def test_more_than_one_band_block(env):
    """Beyond the issue's list: 80 bands (the 20 bands four times) are two blocks of 64, the second one 16 bands wide: dT and
    dfrac add the blocks' sums, the reduction runs a second row of waves. Against the oracle, and gL's rows of a repeated
    band equal bit for bit where g's rows are equal.
    MEASURED: dT 0.21, dfrac 0.55, gL 0.82."""
    c, s, _, g, _ = first_case(env)
    t = device_tables(env, c, FIRST[0], s["End"], s["T_range"], s["Q"], times=4)
    assert t["N_h"].shape == (80,) and np.array_equal(t["N_h"][:20], t["N_h"][60:])
    g4 = np.concatenate([g, VC.cotangent(40, CC.NPIX, np.tile(c["dead"], 2), seed=21), g])
    got, _ = check_raw(env, t, s, s["T_range"], g4, "srf cube vjp 80 bands")
    assert np.array_equal(got["gL"][:, :20], got["gL"][:, 60:]) and not np.array_equal(got["gL"][:, :20], got["gL"][:, 20:40])


@pytest.mark.parametrize("nPix", (1, 63, 255, 256))
def test_pixel_counts(env, nPix):
    """Test 1: one pixel, and scenes that end one short of a round of 64, one short of a chunk of 256 and on it (257, one
    past it, is the scene of the other tests): the bound, and for dT / dfrac the bits of the 257-pixel scene's first nPix."""
    c, s, t, g, whole = first_case(env)
    sc = cut(s, slice(0, nPix))
    got, _ = check_raw(env, t, sc, s["T_range"], np.ascontiguousarray(g[:, :nPix]), "srf cube vjp nPix=%d" % nPix)
    assert np.array_equal(got["dT"], whole["dT"][:nPix]) and np.array_equal(got["dfrac"], whole["dfrac"][:nPix])


@pytest.mark.parametrize("nMix,nEnd", ((1, 8), (5, 8), (9, 31)))
def test_mixture_lengths(env, nMix, nEnd):
    """Test 1: nMix = 1, 5 (two passes of the pixel kernel's 4 slots) and 9 (three, and two of the reduction's 8)."""
    c, s, _, _, _ = first_case(env)
    End = CC.endmembers(c["Xk"].size, nEnd)
    t = device_tables(env, c, "coarse", End, s["T_range"], s["Q"])
    sc = CC.scene(70, nMix, nEnd, s["T_range"], seed=13)
    check_raw(env, t, sc, s["T_range"], VC.cotangent(20, 70, c["dead"], seed=14), "srf cube vjp nMix=%d nEnd=%d" % (nMix, nEnd))


@pytest.mark.parametrize("knots", CC.KNOTS)
def test_inner_product_against_the_forward_kernels(env, knots):
    """Test 2, no oracle: the cube is linear in frac, in the endmembers and in La, so <g, cube(x + d) - cube(x)> = <grad_x, d>
    with the cube from hsi_cube_srf, within twice the forward's own asserted 1e-5 of sum |g| band_max.
    MEASURED: |difference| at most 4.9e-5 against a bound of 0.60."""
    c = fused_case(env, knots)
    s = CC.case(c, knots, "mix3_of_8", "230-350_Q8")
    live = ~c["dead"]
    g = VC.cotangent(20, CC.NPIX, c["dead"], seed=9)
    g64 = g[live].astype(np.float64)
    Q, T_range = s["Q"], s["T_range"]
    got = full(env, c, s["End"], s, g, Q, T_range)
    cube1 = forward(env, c, s["End"], s, Q, T_range)
    bound = 2 * FWD_TOL * float(np.sum(np.abs(g64) * np.max(np.abs(cube1[live].astype(np.float64)), axis=1, keepdims=True)))
    diff = lambda cube2: float(np.sum(g64 * (cube2[live].astype(np.float64) - cube1[live].astype(np.float64))))
    step = lambda x, fr: (x * np.float32(1.0 + fr)).astype(np.float32)
    frac2, End2, La2 = step(s["frac"], 0.3), step(s["End"], -0.2), step(c["La"], 0.2)
    d64 = lambda x2, x: x2.astype(np.float64) - np.asarray(x).astype(np.float64)  # the step the forward is really given
    for what, lhs, rhs in (("frac", np.sum(got["frac"] * d64(frac2, s["frac"])), diff(forward(env, c, s["End"], dict(s, frac=frac2), Q, T_range))),
                           ("endmembers", np.sum(got["endmembers"] * d64(End2, s["End"])), diff(forward(env, c, End2, s, Q, T_range))),
                           ("La", np.sum(got["G_La"].astype(np.float64) * d64(La2, c["La"])), diff(forward(env, c, s["End"], s, Q, T_range, La=La2)))):
        print("srf cube vjp inner product %s d %s: %.9g vs %.9g, |diff| = %.3g, bound %.3g" % (knots, what, lhs, rhs, abs(lhs - rhs), bound))
        assert abs(lhs - rhs) <= bound


@pytest.mark.parametrize("tname", list(CC.T_CONFIGS))
def test_bit_identity_with_the_band_adjoint(env, tname):
    """Test 3: nEnd x Q pixels, pixel (e, q) pure endmember e (frac 1.0 in the middle slot, 0.0 with any index in the two
    others) exactly on node q: gL[q][b][e] is g[b][p(e, q)] bit for bit on the live bands and 0.0 on the dead ones, the pad
    column exactly 0.0, and the rows are band_radiance_srf_vjp's at Ts = the nodes for g rearranged to [Q][nB][nEnd]."""
    torch, sensor = env["torch"], env["sensor"]
    c = fused_case(env, "coarse")
    T_range, Q = CC.T_CONFIGS[tname]
    nEnd = 8
    End = CC.endmembers(c["Xk"].size, nEnd)
    t = device_tables(env, c, "coarse", End, T_range, Q)
    r = np.random.default_rng(41)
    e_of, q_of = np.repeat(np.arange(nEnd), Q), np.tile(np.arange(Q), nEnd)
    nPix = nEnd * Q
    kidx = r.integers(0, nEnd, (nPix, 3)).astype(np.int32)
    kidx[:, 1] = e_of
    frac = np.zeros((nPix, 3), dtype=np.float32)
    frac[:, 1] = 1.0
    sc = dict(kidx=kidx, frac=frac, T=t["nodes"][q_of].copy())
    g = VC.cotangent(20, nPix, c["dead"], seed=43)
    gL = raw(env, t, sc, g, outs=("gL",))["gL"]
    want = np.where(c["dead"][:, None], np.float32(0.0), g).reshape(20, nEnd, Q).transpose(2, 0, 1)  # [Q][nB][nEnd]
    assert np.array_equal(gL[:, :, :nEnd], want) and np.all(gL[:, :, nEnd] == 0.0)
    out = full(env, c, End, sc, g, Q, T_range, outputs=("G_tau", "G_La", "G_Ld"))
    g_re = np.ascontiguousarray(g.reshape(20, nEnd, Q).transpose(2, 0, 1))  # NaN on the dead bands, as the band adjoint takes it
    ref = sensor.band_radiance_srf_vjp(grid_of(env), dev(env, c["tau"]), dev(env, c["La"]), dev(env, c["Ld"]), c["Xk"], dev(env, End), t["nodes"],
                                       sensor.Sensor.from_tables(c["tables"]), dev(env, g_re), outputs=("G_tau", "G_La", "G_Ld"))
    torch.cuda.synchronize()
    for k in ("G_tau", "G_La", "G_Ld"):
        assert np.array_equal(out[k], ref[k].cpu().numpy()) and out[k].any(), k


def test_determinism(env):
    """Test 4: the same bits run to run; dT / dfrac of a pixel unchanged when the scene is permuted, cut to a prefix or a
    middle part, or when other outputs are dropped; every output alone has its bits among the others; and the same bits with
    the pixel kernel's table in LDS (8 endmembers) and in global memory (the same 8 followed by 9 unused columns: 17 x 8 > 128)."""
    c, s, t, g, whole = first_case(env)
    again = raw(env, t, s, g)
    for k in whole:
        assert np.array_equal(again[k], whole[k]), k
    perm = np.random.default_rng(3).permutation(CC.NPIX)
    moved = raw(env, t, cut(s, perm), np.ascontiguousarray(g[:, perm]), outs=("dT", "dfrac"))
    assert np.array_equal(moved["dT"], whole["dT"][perm]) and np.array_equal(moved["dfrac"], whole["dfrac"][perm])
    part = raw(env, t, cut(s, slice(60, 190)), np.ascontiguousarray(g[:, 60:190]), outs=("dT", "dfrac"))
    assert np.array_equal(part["dT"], whole["dT"][60:190]) and np.array_equal(part["dfrac"], whole["dfrac"][60:190])
    for k in ("dT", "dfrac", "gL"):
        alone = raw(env, t, s, g, outs=(k,))
        assert list(alone) == [k] and np.array_equal(alone[k], whole[k]), k
    End17 = CC.endmembers(c["Xk"].size, 17)
    assert np.array_equal(End17[:, :8], s["End"])
    t17 = device_tables(env, c, FIRST[0], End17, s["T_range"], s["Q"])
    assert np.array_equal(t17["G_h"][:, :, :8], t["G_h"])
    wide = raw(env, t17, s, g)
    assert np.array_equal(wide["dT"], whole["dT"]) and np.array_equal(wide["dfrac"], whole["dfrac"])
    assert np.array_equal(wide["gL"][:, :, :8], whole["gL"][:, :, :8]) and np.array_equal(wide["gL"][:, :, 17], whole["gL"][:, :, 8])
    assert np.all(wide["gL"][:, :, 8:17] == 0.0)
    for k in ("Tpix", "frac", "endmembers", "G_Ld"):  # the Python entry: a key alone has the bits it has among the others
        both = full(env, c, s["End"], s, g, s["Q"], s["T_range"], outputs=(k, "G_tau"))
        alone = full(env, c, s["End"], s, g, s["Q"], s["T_range"], outputs=(k,))
        assert list(alone) == [k] and np.array_equal(alone[k], both[k]), k


def test_masks(env):
    """Test 5: NaN or 1e30 in g under the dead bands changes no output and leaves all finite; a NaN pixel, pixels just outside
    the range and an infinite one (one of them with NaN in its column of g) are NaN in their own dT / dfrac, every other
    pixel keeps its bits, and gL is the gL of the scene without them; kidx out of range gives the bits of the clamped indices."""
    c, s, t, g, whole = first_case(env)
    assert c["dead"].sum() == 3 and np.isnan(g[c["dead"]]).all()
    for k, v in whole.items():
        assert np.all(np.isfinite(v)), k
    g30 = np.where(c["dead"][:, None], np.float32(1e30), g)
    other = raw(env, t, s, g30)
    for k in whole:
        assert np.array_equal(other[k], whole[k]), k
    sc = {k: np.array(v) for k, v in cut(s, slice(0, CC.NPIX)).items()}
    sc["T"][3] = np.nan
    sc["T"][70] = np.nextafter(s["T_range"][1], np.inf)
    sc["T"][200] = np.nextafter(s["T_range"][0], -np.inf)
    sc["T"][201] = np.inf
    bad = np.zeros(CC.NPIX, dtype=bool)
    bad[[3, 70, 200, 201]] = True
    g_bad = np.array(g)
    g_bad[:, 3] = np.nan  # what a cost built on a NaN column hands back
    got = raw(env, t, sc, g_bad)
    assert np.array_equal(np.isnan(got["dT"]), bad) and np.array_equal(np.isnan(got["dfrac"]), np.repeat(bad[:, None], 3, axis=1))
    assert np.array_equal(got["dT"][~bad], whole["dT"][~bad]) and np.array_equal(got["dfrac"][~bad], whole["dfrac"][~bad])
    # gL is the gL of the scene without the four: here bit for bit, because the 253 pixels left are one chunk, the refused
    # pixels are passed over inside their chunk, and pixel 256, a chunk of its own in the full scene, is added last either way
    without = raw(env, t, cut(s, ~bad), np.ascontiguousarray(g[:, ~bad]), outs=("gL",))["gL"]
    assert np.array_equal(got["gL"], without) and not np.array_equal(got["gL"], whole["gL"])
    sc = {k: np.array(v) for k, v in cut(s, slice(0, CC.NPIX)).items()}
    lo, hi = sc["kidx"] == 0, sc["kidx"] == 7
    assert lo.any() and hi.any()
    sc["kidx"][lo], sc["kidx"][hi] = -1, 8
    sc["kidx"][5, 0], sc["kidx"][6, 1] = -2**31, 2**31 - 1
    ref_k = np.array(s["kidx"])
    ref_k[5, 0], ref_k[6, 1] = 0, 7
    a, b = raw(env, t, sc, g), raw(env, t, dict(sc, kidx=ref_k), g)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_refusals_write_nothing(env):
    """Test 5: every refusal returns non-zero with a message and leaves the canary-filled outputs alone; nB == 0 and nPix == 0
    return 0; the same arguments, well formed, do write."""
    torch, lib = env["torch"], env["lib"]
    QM = lib.rtx_srf_cube_max_nodes()
    nB, Q, nEnd, nPix, nMix = 3, 2, 4, 70, 2
    f32 = lambda *shape: torch.rand(shape, dtype=torch.float32, device="cuda") + 0.5
    N, tab, g, frac = f32(nB), f32(nEnd, Q, nB), f32(nB, nPix), f32(nPix, nMix)
    kidx = torch.randint(0, nEnd, (nPix, nMix), dtype=torch.int32, device="cuda")
    Tpix = torch.full((nPix,), 300.0, dtype=torch.float64, device="cuda")
    dT = torch.full((nPix,), 7.0, dtype=torch.float64, device="cuda")
    dfrac = torch.full((nPix, nMix), 7.0, dtype=torch.float64, device="cuda")
    gL = torch.full((Q, nB, nEnd + 1), 7.0, dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = [310.0, 290.0, 285.0, 315.0]  # two nodes, then the range

    def call(nB_=nB, Q_=Q, T=good, N_=N, tab_=tab, nEnd_=nEnd, nPix_=nPix, nMix_=nMix, kidx_=kidx, frac_=frac, Tpix_=Tpix, g_=g, outs=True, flags=0):
        T = None if T is None else np.ascontiguousarray(T, dtype=np.float64)
        o = [p(dT), p(dfrac), p(gL)] if outs else [None] * 3
        return lib.rtx_srf_pixel_cube_vjp(nB_, Q_, None if T is None else T.ctypes.data_as(C.c_void_p), p(N_), p(tab_), nEnd_, nPix_, nMix_,
                                          p(kidx_), p(frac_), p(Tpix_), p(g_), *o, st, flags)

    for kw in (dict(Q_=0), dict(Q_=QM + 1, T=list(np.linspace(290.0, 310.0, QM + 1)) + [285.0, 315.0]), dict(nB_=-1), dict(nPix_=-1),
               dict(nEnd_=0), dict(nMix_=0), dict(T=None), dict(N_=None), dict(tab_=None), dict(kidx_=None), dict(frac_=None), dict(Tpix_=None),
               dict(g_=None), dict(outs=False), dict(flags=1), dict(T=[310.0, np.nan, 285.0, 315.0]), dict(T=[300.0, 300.0, 285.0, 315.0]),
               dict(T=[310.0, 290.0, 291.0, 315.0]), dict(T=[310.0, 290.0, 285.0, np.inf])):
        assert call(**kw) != 0 and lib.rtx_last_error(), kw
    torch.cuda.synchronize()
    for v in (dT, dfrac, gL):
        assert bool((v == 7.0).all())
    assert call(nPix_=0) == 0
    torch.cuda.synchronize()
    assert bool((gL == 0.0).all()) and bool((dT == 7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dT).all()) and bool((dT != 7.0).all()) and bool((dfrac != 7.0).all())
    assert bool((gL[:, :, :nEnd] != 7.0).all()) and bool((gL[1:, :, nEnd] == 0.0).all())
    assert call(nB_=0) == 0


def test_stream_contract(env):
    """Test 6: the call runs on the current stream. Behind a delay on a side stream, with every device input NaN until the
    stream has passed the delay, it gives the default-stream bits; a second scene on the same stream (whose workspace then
    holds the other call's partial sums) does too; the warmed call returns while the delay is pending."""
    import stream_cases as S
    torch, lib = env["torch"], env["lib"]
    c, s, t, g, whole = first_case(env)

    def make(sc, gg):
        nEnd, Q, nB = t["tab"].shape
        nPix, nMix = sc["kidx"].shape
        kidx = dev(env, sc["kidx"])
        T_host = t["T_host"]

        def call(d, h):
            env["_lib"].check(lib.rtx_srf_pixel_cube_vjp(nB, Q, S.hp(h["T_node"]), S.vp(d["N"]), S.vp(d["tab"]), nEnd, nPix, nMix, S.vp(kidx),
                                                         S.vp(d["frac"]), S.vp(d["T"]), S.vp(d["g"]), S.vp(d["dT"]), S.vp(d["dfrac"]), S.vp(d["gL"]),
                                                         C.c_void_p(torch.cuda.current_stream().cuda_stream), 0))
            return [d["dT"], d["dfrac"], d["gL"]]
        return S.Case(call, inputs=dict(N=t["N"], tab=t["tab"], frac=dev(env, sc["frac"]), T=dev(env, sc["T"]), g=dev(env, gg)),
                      outputs=dict(dT=((nPix,), torch.float64), dfrac=((nPix, nMix), torch.float64), gL=((Q, nB, nEnd + 1), torch.float32)),
                      host=dict(T_node=np.array(T_host)), scribble=dict(T_node=np.array(T_host)), keep=(kidx,))

    case = make(s, g)
    other = make(cut(s, slice(0, 65)), np.ascontiguousarray(g[:, 10:75]))
    ref, _ = S.run_plain(case)
    assert np.array_equal(S.as_float(ref[0]), whole["dT"]) and np.array_equal(S.as_float(ref[2]), whole["gL"])
    ref_o, _ = S.run_plain(other)
    s1, delay = torch.cuda.Stream(), S.Delay()
    S.run_plain(case, s1)  # grows the workspace of s1
    _, host_ms = S.run_plain(case, s1)
    Dms = delay.ms_for(host_ms, "rtx_srf_pixel_cube_vjp")
    out, pend, _ = S.run_delayed([case, other, case], s1, delay, Dms)
    torch.cuda.synchronize()
    assert S.same_bits(out[0], ref), S.describe(out[0], ref)
    assert S.same_bits(out[1], ref_o), S.describe(out[1], ref_o)
    assert S.same_bits(out[2], ref), S.describe(out[2], ref)
    assert all(pend), "the call returned only after %.0f ms of device work ahead of it on its stream had finished" % Dms


@pytest.mark.parametrize("thin", (1.0, 1e-3), ids=("standard", "thinned"))
def test_compute_hsi_cube_vjp_end_to_end(thin):
    """Test 7: rt.compute_hsi_cube_vjp at the atmosphere and span of test_gpu_sensor_vjp.py's end-to-end test, a 257-pixel
    scene of 3 out of 8 endmembers: the cube is hsi_cube_srf's on compute_TUD's outputs bit for bit; the layer gradients are
    rt.compute_TUD_jacobian's rows contracted with hsi_cube_srf_vjp's G_tau / G_La / G_Ld on those outputs, within
    test_gpu_tud_vjp.py's end-to-end bound; "Tpix", "frac" and "endmembers" are that call's, and agree with the fp64 oracle
    on the device's N and table.
    MEASURED: the layer gradients at most 0.023 of the bound; thinned, in units of 2^-24 scale: Tpix 0.79, frac 3.1 (k = 10),
    endmembers 0.10 (k = 35); standard (tau = 0: the surface is not seen) exact zeros."""
    import torch
    assert torch.cuda.is_available()
    from radtxfr_amd import _lib, engine, sensor, synthetic
    from radtxfr_amd import radiative_transfer as rt
    from test_gpu_tud_vjp import F32_TINY, U32
    lo, hi, dv = 1000.0, 1000.5, 0.0005
    sub = synthetic.subset_table(synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0), lo - 12.0, hi + 12.0)
    sa = rt.StdAtmos
    a = dict(Zs=sa[:, 1], Ts=sa[:, 5].copy(), Ps=sa[:, 4], PLs=sa[:, 3], MFs_VAL=sa[:, 6:9] * 1e6 * thin, MFs_ID=np.array([1, 2, 3]))
    wrt = ("T", 1, 3)
    kw = dict(DVOUT=dv, line_table=sub, Altitudes=np.array([8.0]), **a)
    s = sensor.Sensor.from_shape([1000.10, 1000.14, 1000.38, 1003.0], 0.06, "triangle")  # the last one off the axis: a dead band
    Xk = np.array([999.9, 1000.07, 1000.2, 1000.33, 1000.6])
    nB, nk, nEnd, Q, T_range = 4, 5, 8, 8, (230.0, 350.0)
    End = CC.endmembers(nk, nEnd)
    sc = CC.scene(CC.NPIX, 3, nEnd, T_range)
    dead = np.array([False, False, False, True])
    cot = VC.cotangent(nB, CC.NPIX, dead, seed=3)
    X_out, cube, grad = rt.compute_hsi_cube_vjp(lo, hi, s, Xk, End, sc["kidx"], sc["frac"], sc["T"], cot, wrt=wrt, n_nodes=Q, **kw)
    assert np.array_equal(X_out, s.centres) and cube.shape == (nB, CC.NPIX) and cube.dtype == np.float32
    assert set(grad) == set(wrt) | {"Tpix", "frac", "endmembers"}
    X, tau, La, Ld = rt.compute_TUD(lo, hi, **kw)
    nX, nL = X.size, a["Ts"].size
    grid = engine.Grid(lo, hi, nX)
    d32 = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float32).ravel(), device="cuda")
    dv_ = lambda v: torch.as_tensor(np.array(v), device="cuda")
    scene = (Xk, dv_(End), dv_(sc["kidx"]), dv_(sc["frac"]), dv_(sc["T"]), s)
    t_d, a_d, d_d = d32(tau), d32(La), d32(Ld)
    want_cube = sensor.hsi_cube_srf(grid, t_d, a_d, d_d, *scene, n_nodes=Q)[1].cpu().numpy()  # T_range from the scene: both ends are in it
    assert np.array_equal(cube, want_cube, equal_nan=True) and np.isnan(cube[3]).all() and np.isfinite(cube[:3]).all()
    r = {k: v.cpu().numpy() for k, v in sensor.hsi_cube_srf_vjp(grid, t_d, a_d, d_d, *scene, dv_(cot), n_nodes=Q).items()}
    for k in ("Tpix", "frac", "endmembers"):
        assert grad[k].dtype == np.float64 and np.array_equal(grad[k], r[k]), k
    _, _, _, _, J = rt.compute_TUD_jacobian(lo, hi, wrt=wrt, **kw)
    G = {k: r[k].astype(np.float64) for k in ("G_tau", "G_La", "G_Ld")}
    g_sum = sum(np.abs(v).sum() for v in G.values())
    for w in wrt:
        assert grad[w].shape == (nL,) and grad[w].dtype == np.float64
        rows = [np.asarray(J[w][i], dtype=np.float64).reshape(nX, nL) for i in range(3)]
        want = sum(np.einsum("x,xl->l", G[k], rows[i]) for i, k in enumerate(("G_tau", "G_La", "G_Ld")))
        scale = sum(np.einsum("x,xl->l", np.abs(G[k]), np.abs(rows[i])) for i, k in enumerate(("G_tau", "G_La", "G_Ld")))
        bound = 4.0 * U32 * scale + F32_TINY * g_sum
        err = np.abs(grad[w] - want)
        print("compute_hsi_cube_vjp end to end, wrt %r: worst |got - ref| / bound = %.3g" % (w, float(np.max(err / np.where(bound > 0, bound, 1.0)))))
        assert np.all(err <= bound), w
    assert np.all(grad[3] == 0.0) and np.count_nonzero(grad["T"]) >= 2 and np.count_nonzero(grad[1]) >= 2
    # the surface side against the fp64 oracle on the device's own N and table
    lib = _lib.load()
    nodes = sensor.srf_cube_nodes(T_range[0], T_range[1], Q)
    N, Cb, M, jr = sensor.srf_moments(grid, t_d, a_d, d_d, dv_(Xk), nodes, s)
    tab = torch.empty((nEnd, Q, nB), dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(lib.rtx_srf_cube_tables(p(M), p(jr), nB, Q, nk, p(dv_(End)), nEnd, p(tab), None))
    torch.cuda.synchronize()
    o = VC.adjoint(N.cpu().numpy(), tab.cpu().numpy().astype(np.float64).transpose(1, 2, 0), sc, nodes, T_range, cot)
    assert np.array_equal(N.cpu().numpy() == 0.0, dead)
    within(grad["Tpix"], o["dT"], o["scale"]["dT"], K_DT(Q), "end to end Tpix")
    within(grad["frac"], o["dfrac"], o["scale"]["dfrac"], K_DFRAC(Q), "end to end frac")
    E0 = np.concatenate([End, np.zeros((nk, 1), dtype=np.float32)], axis=1)
    args = (X, s.tables, tau.ravel().astype(np.float32), La.ravel().astype(np.float32), Ld.ravel().astype(np.float32), Xk, E0, nodes)
    b, bs = SV.adjoint(*args, o["gL"]), SV.adjoint(*args, o["scale"]["gL"])
    within(grad["endmembers"], b["dE"][:, :nEnd], bs["scale"]["dE"][:, :nEnd], K_DE + K_GL, "end to end endmembers")
    assert np.all(np.isfinite(grad["endmembers"]))
    if thin < 1.0:
        assert tau.min() > 0.0 and np.all(grad["Tpix"] != 0.0) and np.count_nonzero(grad["endmembers"]) > nk * nEnd // 2
