"""CPU-only checks of the bound-constrained per-pixel fit (include/radtxfr_hip.h: rtx_srf_pixel_cube_normal_box,
rtx_srf_pixel_cube_fit_box; the nonneg / sum_weight keywords of sensor.hsi_cube_srf_normal / hsi_cube_srf_fit and
rt.compute_hsi_cube_fit): the fp64 restatement of tests/srf_cube_fit_box_cases.py against a brute-force optimum
on noisy scenes with absent endmembers, the unconstrained restatement as the control that those scenes need the constraint,
the KKT conditions at the result, the new ABI entries with what they refuse before any launch, and the argument checks of
the three Python entries that need no device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from radtxfr_amd import _lib, sensor
from radtxfr_amd import radiative_transfer as rt

import srf_cube_cases as CC
import srf_cube_fit_box_cases as BX
import srf_cube_fit_cases as FT
import test_srf_cube_fit_host as TH

KKT_FREE = 1e-6  # |g_i| <= KKT_FREE sqrt(H_ii cost) on the free unknowns of the fp64 restatement

_SCENE = {}


def _noisy(knots, sname, tname):
    """The fp64 moments of a case, the noisy scene and its measurement (the node form plus noise, float32), made once."""
    key = (knots, sname, tname)
    if key not in _SCENE:
        c, _, Tq, T_range, N, Cb, M, End, G = TH._setup(knots, sname, tname)
        nMix, nEnd = FT.SCENES[sname]
        sc = BX.noisy_scene(FT.NPIX, nMix, nEnd, T_range)
        meas = BX.add_noise(CC.node_cube(N, Cb, M, End, sc, Tq))
        assert np.isnan(meas[c["dead"]]).all() and np.isfinite(meas[~c["dead"]]).all()
        _SCENE[key] = (sc, Tq, T_range, N, Cb, G, meas)
    return _SCENE[key]


@pytest.mark.parametrize("delta", BX.DELTAS)
@pytest.mark.parametrize("tname", list(CC.T_CONFIGS))
@pytest.mark.parametrize("sname", list(FT.SCENES))
@pytest.mark.parametrize("knots", CC.KNOTS)
def test_restatement_reaches_the_brute_optimum(knots, sname, tname, delta):
    """257 pixels, noise 1e-3, half the pixels with an absent endmember, the scan start, 40 trials. In fp64 the cost at the
    restatement's result exceeds the brute-force optimum (a grid of 400 in T refined 3 times, non-negative least squares by
    subset enumeration) by at most 1e-7 relative; with the kernel's fp32 roundings simulated the fp64 cost at the result is
    within 2 sum_b w_b |r_b| e_b of it, the GPU recovery test's bound. No fraction negative, T in range, the cost never above
    the start's.
    MEASURED (fp64 NumPy), worst of the 24 cases: fp64 relative excess 1.8e-9 (negative down to -2.5e-10 where the restatement
    beats the search's resolution in T); with fp32 simulated 0.011 of the bound (relative excess 1.8e-4); 0 to 13 pixels per
    scene end with T on an end of the range, 57 to 105 with a fraction at 0 (none in the one-endmember scenes)."""
    sc, Tq, T_range, N, Cb, G, meas = _noisy(knots, sname, tname)
    best = BX.brute(N, Cb, G, Tq, T_range, sc["kidx"], meas, delta=delta)
    for f32 in (False, True):
        r = BX.fit(N, Cb, G, Tq, T_range, sc["kidx"], meas, delta=delta, f32=f32)
        c64 = BX.cost_at(N, Cb, G, Tq, sc["kidx"], r["frac"], r["T"], meas, delta=delta)
        excess = c64 - best["cost"]
        slack = BX.cost_slack(N, Cb, G, Tq, sc["kidx"], r["frac"], r["T"], meas)
        print("srf cube box restatement %s %s %s delta=%g fp32=%d: relative excess %.3g .. %.3g, excess / bound %.3g, T on an end %d, a fraction at 0 %d, "
              "statuses %r" % (knots, sname, tname, delta, f32, (excess / best["cost"]).min(), (excess / best["cost"]).max(), (excess / slack).max(),
                               ((r["T"] == T_range[0]) | (r["T"] == T_range[1])).sum(), (r["frac"] == 0).any(axis=1).sum(),
                               np.unique(r["status"]).tolist()))
        assert np.all(r["status"] <= 1) and np.all(r["n_iter"] <= FT.TRIALS) and np.all(r["cost"] <= r["cost0"])
        assert np.all(r["frac"] >= 0.0) and np.all(r["T"] >= T_range[0]) and np.all(r["T"] <= T_range[1])
        if f32:
            assert np.all(excess <= slack)
        else:
            assert np.all(excess <= 1e-7 * best["cost"])


@pytest.mark.parametrize("tname", list(CC.T_CONFIGS))
@pytest.mark.parametrize("sname", [s for s in FT.SCENES if FT.SCENES[s][0] > 1])
@pytest.mark.parametrize("knots", CC.KNOTS)
def test_unconstrained_fit_goes_negative(knots, sname, tname):
    """The control: on the same scenes the unconstrained restatement (FT.fit) ends with a negative fraction in at least one
    pixel, so these scenes exercise the constraint.
    MEASURED (fp64 NumPy), the 8 scenes: 57 to 104 of the 257 pixels; the lowest fraction -0.03 .. -0.85 on the narrow range,
    -1.2 .. -7.5 on the wide one."""
    sc, Tq, T_range, N, Cb, G, meas = _noisy(knots, sname, tname)
    r = FT.fit(N, Cb, G, Tq, T_range, sc["kidx"], meas)
    neg = (r["frac"] < 0.0).any(axis=1)
    print("srf cube unconstrained control %s %s %s: %d pixels with a negative fraction, lowest %.3g" % (knots, sname, tname, neg.sum(), np.nanmin(r["frac"])))
    assert neg.sum() >= 1


@pytest.mark.parametrize("case", (("coarse", "mix3_of_8", "230-350_Q8", 0.0), ("dense", "mix4_of_31", "285-315_Q5", 1e-2),
                                  ("coarse", "mix1_of_8", "285-315_Q5", 1e-2)), ids=("mix3", "mix4", "mix1"))
def test_kkt_at_the_result(case):
    """At the restatement's result after 40 trials from the scan: the active set (step 1's set) holds only unknowns on a bound,
    with g_i > 0 on a lower bound and g_i < 0 on an upper one; an unknown on a bound that is not active has the opposite sign
    or 0; and on the free unknowns the gradient is as small as the number format of the unknowns lets it be. Two assertions:
      the iteration as the entry runs it, the fractions rounded to float32 after every trial. A free fraction then lives on the
      float32 grid and can be brought no nearer to its stationary value than the grid allows; with every free fraction within
      one spacing s_j = spacing((float)f_j) of it (T is fp64 and has no grid), the quadratic model leaves, element by element,
          |g_i| <= sum_{j free, j >= 1} |H_ij| s_j.                                           ASSERTED; measured 0.99 of it at worst
      the same iteration with the fractions kept in fp64 (frac_dtype=np.float64), which shows that the floor above is the grid
      and not the step: there |g_i| <= 1e-6 sqrt(H_ii cost).                                  ASSERTED; measured 3.3e-8 at worst
    MEASURED (fp64 NumPy), the three cases, |g_i| / sqrt(H_ii cost) on free unknowns: fractions in fp64 3.3e-8, 2.3e-9, 4.0e-9;
    rounded to float32 1.5e-5, 1.5e-5, 4.2e-5 (the same after 200 trials, when every pixel has stopped by itself), which is
    0.99, 0.29, 0.49 of the grid bound; over all 24 scenes of the optimum test the worst is that 0.99, the next 0.68."""
    knots, sname, tname, delta = case
    sc, Tq, T_range, N, Cb, G, meas = _noisy(knots, sname, tname)
    nU = sc["kidx"].shape[1] + 1
    lo, hi = BX.bounds(nU, T_range)
    worst, grid = {}, None
    for fd in (np.float64, np.float32):
        r = BX.fit(N, Cb, G, Tq, T_range, sc["kidx"], meas, delta=delta, frac_dtype=fd)
        e = BX.evaluate(N, Cb, G, Tq, sc["kidx"], r["frac"], r["T"], meas, delta=delta)
        assert np.array_equal(e["grad"], r["grad"]) and np.all(r["status"] <= 1) and r["frac"].dtype == fd
        B = BX.unbits(r["active"], nU)
        u = np.concatenate([r["T"][:, None], r["frac"].astype(np.float64)], axis=1)
        g = r["grad"]
        assert np.all((u == lo)[B] | (u == hi)[B])
        assert np.all(g[B & (u == lo)] > 0.0) and np.all(g[B & (u == hi)] < 0.0)
        assert np.all(g[~B & (u == lo)] <= 0.0) and np.all(g[~B & (u == hi)] >= 0.0)
        Hd = np.stack([e["hess"][:, FT.tri(i, i)] for i in range(nU)], axis=1)
        free = ~B & (u > lo) & (u < hi)
        worst[fd] = np.where(free, np.abs(g) / np.sqrt(Hd * e["cost"][:, None]), 0.0).max()
        assert B.any() and free.any()
        if fd is np.float32:
            s_j = np.concatenate([np.zeros((FT.NPIX, 1)), np.spacing(r["frac"]).astype(np.float64)], axis=1)
            lim = np.einsum("pij,pj->pi", np.abs(FT.unpack(e["hess"])), np.where(free, s_j, 0.0))
            grid = np.where(free, np.abs(g) / np.where(lim > 0.0, lim, 1.0), 0.0).max()
            assert np.all(np.abs(g)[free] <= lim[free])
    print("srf cube box KKT %s %s %s delta=%g: worst |g_i| / sqrt(H_ii cost) on free unknowns: fractions in fp64 %.3g, rounded to float32 %.3g "
          "(%.3g of the float32 grid's bound)" % (knots, sname, tname, delta, worst[np.float64], worst[np.float32], grid))
    assert worst[np.float64] <= KKT_FREE


def test_box_step_by_hand():
    """The restated box step on a 3-unknown system worked by hand: an unknown on its bound with an outward gradient stays (step
    1); a free one that the solve would carry across 0 is cut there and the third re-solved with the cut step in its
    right-hand side; with everything free and inside it is FT.solve's step."""
    H = np.array([[4.0, 0.0, 1.0, 1.0, 0.5, 2.0]])  # rows: H_00; H_10 H_11; H_20 H_21 H_22
    T_range = (250.0, 350.0)
    T, f = np.array([300.0]), np.array([[0.5, 0.5]], dtype=np.float32)
    g = np.array([[0.4, 0.1, -0.2]])
    d, ok, B = BX.box_step(H, g, 0.0, T, f, T_range)
    want, _ = FT.solve(H, g, 0.0)
    assert ok.all() and not B.any() and np.array_equal(d, want)
    f0 = np.array([[0.0, 0.5]], dtype=np.float32)
    d, ok, B = BX.box_step(H, g, 0.0, T, f0, T_range)  # f_1 = 0 with g_1 > 0: held; the rest is the 2 x 2 system of T and f_2
    assert B.tolist() == [[False, True, False]] and d[0, 1] == 0.0
    assert np.allclose(d[0, [0, 2]], np.linalg.solve(np.array([[4.0, 1.0], [1.0, 2.0]]), -g[0, [0, 2]]), rtol=1e-14)
    g2 = np.array([[0.0, 1.0, 0.0]])
    f2 = np.array([[0.25, 0.5]], dtype=np.float32)     # the free solve gives d_1 = -1.14..: across 0, so d_1 = -0.25 and a re-solve
    d, ok, B = BX.box_step(H, g2, 0.0, T, f2, T_range)
    assert B.tolist() == [[False, True, False]] and d[0, 1] == -0.25
    rhs = -(g2[0, [0, 2]] + np.array([0.0, 0.5]) * -0.25)
    assert np.allclose(d[0, [0, 2]], np.linalg.solve(np.array([[4.0, 1.0], [1.0, 2.0]]), rhs), rtol=1e-14)
    Tt, ft = BX.trial_point(T, f2, d, T_range)
    assert ft[0, 0] == 0.0 and ft[0, 1] > 0.5 and T_range[0] <= Tt[0] <= T_range[1]
    d, ok, B = BX.box_step(H, g, 0.0, np.array([350.0]), f, T_range)  # T on the upper end with g_0 > 0: it may move down
    assert not B[0, 0] and d[0, 0] < 0.0
    d, ok, B = BX.box_step(H, -g, 0.0, np.array([350.0]), f, T_range)  # g_0 < 0 there: held
    assert B[0, 0] and d[0, 0] == 0.0
    Hbad = H.copy()
    Hbad[0, FT.tri(2, 2)] = -1.0
    d, ok, B = BX.box_step(Hbad, g, 0.0, T, f, T_range)
    assert not ok[0] and np.isnan(d).all()


def test_pseudo_band():
    """BX.evaluate with delta against FT.evaluate plus the pseudo-band's terms written out, and delta = 0 is FT.evaluate."""
    sc, Tq, T_range, N, Cb, G, meas = _noisy("coarse", "mix3_of_8", "230-350_Q8")
    a = FT.evaluate(N, Cb, G, Tq, sc["kidx"], sc["frac"], sc["T"], meas)
    z = BX.evaluate(N, Cb, G, Tq, sc["kidx"], sc["frac"], sc["T"], meas, delta=0.0)
    b = BX.evaluate(N, Cb, G, Tq, sc["kidx"], sc["frac"], sc["T"], meas, delta=0.25)
    for k in ("cost", "grad", "hess"):
        assert np.array_equal(a[k], z[k])
    r = sc["frac"].astype(np.float64).sum(axis=1) - 1.0
    assert np.allclose(b["cost"], a["cost"] + 0.25 * r * r, rtol=1e-15) and np.array_equal(b["grad"][:, 0], a["grad"][:, 0])
    assert np.allclose(b["grad"][:, 1:], a["grad"][:, 1:] + 0.25 * r[:, None], rtol=1e-15, atol=0.0)
    J = np.array([0.0, 1.0, 1.0, 1.0])
    for i in range(4):
        for j in range(i + 1):
            assert np.allclose(b["hess"][:, FT.tri(i, j)], a["hess"][:, FT.tri(i, j)] + 0.25 * J[i] * J[j], rtol=1e-15, atol=0.0)


# ------------------------------------------------------------------------------------------ the entries' refusals
def test_argument_checks_of_the_python_entries():
    """nonneg / sum_weight of the three entries: sum_weight must be finite and not negative, and > 0 needs nonneg=True; with
    them well formed the next refusal is the one the unconstrained call makes (host tensors; here there is no device). All
    before any device work."""
    f0, T0 = torch.zeros((4, 2), dtype=torch.float32), torch.full((4,), 300.0, dtype=torch.float64)
    for fn in ("normal", "fit"):
        for kw, text in ((dict(sum_weight=1e-2), "needs nonneg=True"), (dict(nonneg=True, sum_weight=-1.0), "sum_weight"),
                         (dict(nonneg=True, sum_weight=np.nan), "sum_weight"), (dict(nonneg=True, sum_weight=np.inf), "sum_weight"),
                         (dict(nonneg=True, sum_weight="x"), "sum_weight"), (dict(nonneg=True, sum_weight=1e-2), "device tensors"),
                         (dict(nonneg=True), "device tensors"), (dict(nonneg=False, sum_weight=0.0), "device tensors")):
            with pytest.raises(ValueError, match=text):
                TH._stub(fn, **kw)
    with pytest.raises(ValueError, match="nMix=5"):
        TH._stub("fit", nonneg=True, kidx=torch.zeros((4, 5), dtype=torch.int32))
    with pytest.raises(ValueError, match="device tensors"):
        TH._stub("fit", nonneg=True, sum_weight=1e-2, frac0=f0, T0=T0)
    s = sensor.Sensor.from_shape([1000.1, 1000.3], 0.1, "triangle")
    Xk = np.linspace(1000.0, 1000.5, 5)
    call = lambda **k: rt.compute_hsi_cube_fit(1000.0, 1000.5, s, Xk, np.full((5, 3), 0.9, dtype=np.float32), np.zeros((6, 2), dtype=np.int32),
                                               np.ones((2, 6), dtype=np.float32), (290.0, 310.0), DVOUT=0.0005, Altitudes=np.array([8.0]), **k)
    for kw, text in ((dict(sum_weight=1e-2), "needs nonneg=True"), (dict(nonneg=True, sum_weight=-1.0), "sum_weight"),
                     (dict(nonneg=True, sum_weight=np.nan), "sum_weight"), (dict(nonneg=True, max_iter=1001), "max_iter")):
        with pytest.raises(ValueError, match=text):
            call(**kw)


def test_abi_symbols_and_refusals():
    """The three new symbols are in PROTOTYPES, declared in the header and exported, with 23 and 26 arguments; box_max_mix is 4
    (3 would have to be said in DESIGN 4.28); what the two entries refuse, they refuse before anything touches a device (the
    pointers are host memory, never read there), and nB == 0 / nPix == 0 return 0. The unconstrained fit still refuses flag
    bits 2 and 3."""
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "radtxfr_hip.h")).read()
    for name, n in (("rtx_srf_pixel_cube_normal_box", 23), ("rtx_srf_pixel_cube_fit_box", 26), ("rtx_srf_pixel_cube_fit_box_max_mix", 0)):
        assert name in _lib.PROTOTYPES and ("int %s(" % name) in header and hasattr(lib, name)
        decl = header.split("int %s(" % name)[1].split(");")[0]
        assert len(_lib.PROTOTYPES[name][1]) == (decl.count(",") + 1 if n else 0) == n
    for name, base in (("rtx_srf_pixel_cube_normal_box", "rtx_srf_pixel_cube_normal"), ("rtx_srf_pixel_cube_fit_box", "rtx_srf_pixel_cube_fit")):
        assert _lib.PROTOTYPES[name][1][:len(_lib.PROTOTYPES[base][1])] == _lib.PROTOTYPES[base][1]  # the parent's arguments first
    MM, IM = lib.rtx_srf_pixel_cube_fit_box_max_mix(), lib.rtx_srf_pixel_cube_fit_max_iter()
    assert MM == 4 and MM <= lib.rtx_srf_pixel_cube_fit_max_mix()
    QM = lib.rtx_srf_cube_max_nodes()
    buf = np.zeros(64)
    p = C.c_void_p(buf.ctypes.data)
    good = np.array([310.0, 290.0, 285.0, 315.0])  # two nodes, then the range
    th = lambda T: None if T is None else np.ascontiguousarray(T, dtype=np.float64)

    def normal(nB=2, Q=2, T=good, N=p, Cb=p, tab=p, nEnd=3, nPix=4, nMix=2, kidx=p, frac=p, Tpix=p, meas=p, cost=p, flags=0, sw=1e-2, active=p):
        T = th(T)
        return lib.rtx_srf_pixel_cube_normal_box(nB, Q, None if T is None else T.ctypes.data_as(C.c_void_p), N, Cb, tab, nEnd, nPix, nMix, kidx, frac,
                                                 Tpix, meas, None, None, cost, p, p, p, None, flags, sw, active)

    def fit(nB=2, Q=2, T=good, N=p, Cb=p, tab=p, nEnd=3, nPix=4, nMix=2, kidx=p, meas=p, frac=p, Tpix=p, max_iter=5, lambda0=1e-3, ftol=0.0,
            cost=p, n_iter=p, status=p, flags=0, sw=1e-2, active=p):
        T = th(T)
        return lib.rtx_srf_pixel_cube_fit_box(nB, Q, None if T is None else T.ctypes.data_as(C.c_void_p), N, Cb, tab, nEnd, nPix, nMix, kidx, meas,
                                              None, frac, Tpix, max_iter, lambda0, ftol, cost, n_iter, status, None, None, flags, sw, None, active)

    shared = [("Q=", dict(Q=0)), ("Q=", dict(Q=QM + 1, T=np.linspace(300.0, 310.0, QM + 3))), ("negative", dict(nB=-1)), ("negative", dict(nPix=-1)),
              ("nEnd=", dict(nEnd=0)), ("nMix=", dict(nMix=0)), ("max_mix", dict(nMix=MM + 1)), ("NULL", dict(T=None)), ("NULL", dict(meas=None)),
              ("NULL", dict(cost=None)), ("NULL", dict(meas=None, nPix=0)), ("NULL", dict(N=None)), ("NULL", dict(Cb=None)), ("NULL", dict(tab=None)),
              ("NULL", dict(kidx=None)), ("NULL", dict(frac=None)), ("NULL", dict(Tpix=None)),
              ("node temperature", dict(T=[310.0, np.nan, 285.0, 315.0])), ("outside the range", dict(T=[310.0, 284.0, 285.0, 315.0])),
              ("not distinct", dict(T=[300.0, 300.0, 285.0, 315.0])), ("range", dict(T=[310.0, 290.0, 315.0, 285.0])),
              ("sum_weight", dict(sw=-1e-300)), ("sum_weight", dict(sw=np.nan)), ("sum_weight", dict(sw=np.inf)),
              ("sum_weight", dict(sw=np.nan, nPix=0))]
    for fn, extra in ((normal, [("flags", dict(flags=1))]),
                      (fit, [("flags", dict(flags=2)), ("flags", dict(flags=3)), ("max_iter", dict(max_iter=-1)), ("max_iter", dict(max_iter=IM + 1)),
                             ("lambda0", dict(lambda0=-1.0)), ("lambda0", dict(lambda0=np.inf)), ("lambda0", dict(lambda0=np.nan)),
                             ("ftol", dict(ftol=-1.0)), ("ftol", dict(ftol=np.nan)), ("NULL", dict(n_iter=None)), ("NULL", dict(status=None))])):
        for text, kw in shared + extra:
            assert fn(**kw) != 0 and text in lib.rtx_last_error().decode(), (fn.__name__, kw, lib.rtx_last_error())
        assert fn(nB=0) == 0 and fn(nPix=0) == 0 and fn(nB=0, sw=0.0, active=None) == 0
    assert not buf.any()
    for flags in (2, 3):
        assert lib.rtx_srf_pixel_cube_fit(2, 2, good.ctypes.data_as(C.c_void_p), p, p, p, 3, 4, 2, p, p, None, p, p, 5, 1e-3, 0.0, p, p, p, None, None,
                                          flags) != 0


def test_the_shared_header_and_the_makefile():
    """The device functions both families share live in rtx_srf_cube_fit_common.h, once; the new source is in the Makefile's
    SRCS and the header in its dependencies; SCF_PB and SCF_TAB_LDS are defined in rtx_srf_cube_fit.hip alone, the header holds
    the same values as defaults for the box source and checks them."""
    csrc = os.path.join(ROOT, "radtxfr_amd", "csrc")
    src = {f: open(os.path.join(csrc, f)).read() for f in ("rtx_srf_cube_fit.hip", "rtx_srf_cube_fit_box.hip", "rtx_srf_cube_fit_common.h", "Makefile")}
    for fn in ("void scf_eval(", "bool scf_solve(", "void scf_trial(", "int scf_front("):
        assert src["rtx_srf_cube_fit_common.h"].count(fn) == 1 and fn not in src["rtx_srf_cube_fit.hip"] and fn not in src["rtx_srf_cube_fit_box.hip"]
    for f in ("rtx_srf_cube_fit.hip", "rtx_srf_cube_fit_box.hip"):
        assert '#include "rtx_srf_cube_fit_common.h"' in src[f]
    assert "#define SCF_PB 64 " in src["rtx_srf_cube_fit.hip"] and "#define SCF_TAB_LDS 128 " in src["rtx_srf_cube_fit.hip"]
    assert "#define SCF_PB" not in src["rtx_srf_cube_fit_box.hip"] and "#define SCF_TAB_LDS" not in src["rtx_srf_cube_fit_box.hip"]
    assert "static_assert(SCF_PB == 64" in src["rtx_srf_cube_fit_common.h"]
    srcs = [l for l in src["Makefile"].splitlines() if l.startswith("SRCS")][0]
    assert "rtx_srf_cube_fit_box.hip" in srcs.split() and "rtx_srf_cube_fit_common.h" in src["Makefile"]
