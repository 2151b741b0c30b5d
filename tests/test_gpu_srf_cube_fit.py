"""The per-pixel fit to a measured HSI cube (radtxfr_amd/csrc/rtx_srf_cube_fit.hip: rtx_srf_pixel_cube_normal,
rtx_srf_pixel_cube_fit; sensor.hsi_cube_srf_normal / hsi_cube_srf_fit, rt.compute_hsi_cube_fit) against the fp64 NumPy of
tests/srf_cube_fit_cases.py evaluated on the device's own float32 N, C and table, against the shipped forward kernel bit for
bit, and against itself.

Grid, inputs, the 20 bands (three dead) and the knot sets are those of tests/srf_fused_cases.py; the scenes are
srf_cube_fit_cases.distinct_scene's (257 pixels: four workgroups of 64 and one pixel of a fifth).

Bound of the oracle cases: |got - want| <= k 2^-24 scale, element by element, scale = the oracle's sum of the absolute
values of the same summands (|r| taken as |y| + |meas|), k = the fp32 roundings along the kernel's chain (K_* below;
everything not counted is fp64)."""
import ctypes as C

import numpy as np
import pytest

import srf_cube_cases as CC
import srf_cube_fit_cases as FT
import srf_cube_vjp_cases as VC
import srf_fused_cases as FC
from test_gpu_sensor_vjp import within

pytestmark = pytest.mark.gpu

# a J entry: the rounding of l_q or l'_q to fp32 (1), the fmaf chain over the Q nodes (Q), the rest fp64 (1)
K_J = lambda Q: Q + 2
# r = y - meas: the rounding of l_q (1), the chain (Q), the fmaf over the nMix slots (nMix), the sum with C_b (1), the division (1)
K_R = lambda Q, nMix: Q + nMix + 3
K_H = lambda Q: 2 * K_J(Q) + 1                     # a product of two J entries, the fp64 sums (1 for all)
K_GRAD = lambda Q, nMix: K_J(Q) + K_R(Q, nMix) + 1  # J r
K_COST = lambda Q, nMix: 2 * K_R(Q, nMix) + 1       # r r
FIRST = ("coarse", "mix3_of_8", "230-350_Q8")
GIVEN = 1  # RTX_FIT_START_GIVEN
E2E_THIN = 1e-3  # the end-to-end test's mixing ratios: the standard atmosphere's times this (tau up to 0.8: the surface is seen, and Ld
                 # is large enough to tell T from the fractions; at 1e-2 tau stays below 0.11 and 40 trials do not reach the bound)


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    from radtxfr_amd import _lib, engine, sensor
    lib = _lib.load()
    return dict(torch=torch, lib=lib, _lib=_lib, engine=engine, sensor=sensor, CH=lib.rtx_srf_chunk_points(), K=lib.rtx_srf_max_knots())


def dev(env, a):
    return env["torch"].as_tensor(np.array(a), device="cuda")  # a copy: the shared inputs are read-only


_TABLES = {}


def device_tables(env, knots, nEnd, tname, times=1, nB=None):
    """The device's own N, C [nB] and table [nEnd][Q][nB] (float32, device) at the nodes, with fp64 host copies N_h, C_h and
    G_h [Q][nB][nEnd], what the oracle is evaluated on. tname: a name of CC.T_CONFIGS, or (T_range, Q) itself. The bands are
    the case's 20 repeated `times` over, or repeated and cut to nB (the 3 dead bands recur every 20)."""
    nB = 20 * times if nB is None else nB
    key = (knots, nEnd, tname, nB)
    if key not in _TABLES:
        torch, sensor, lib = env["torch"], env["sensor"], env["lib"]
        c = FC.case(env["CH"], env["K"], knots)
        T_range, Q = CC.T_CONFIGS[tname] if isinstance(tname, str) else tname
        End = CC.endmembers(c["Xk"].size, nEnd)
        assert len(c["tables"]) == 20
        reps = -(-nB // 20)
        s = sensor.Sensor.from_tables((list(c["tables"]) * reps)[:nB])
        nodes = sensor.srf_cube_nodes(T_range[0], T_range[1], Q)
        grid = env["engine"].Grid(*FC.grid_tuple(env["CH"]))
        N, Cb, M, jr = sensor.srf_moments(grid, dev(env, c["tau"]), dev(env, c["La"]), dev(env, c["Ld"]), dev(env, c["Xk"]), nodes, s)
        assert len(s) == nB
        nk = c["Xk"].size
        tab = torch.empty((nEnd, Q, nB), dtype=torch.float32, device="cuda")
        p = lambda t: C.c_void_p(t.data_ptr())
        env["_lib"].check(lib.rtx_srf_cube_tables(p(M), p(jr), nB, Q, nk, p(dev(env, End)), nEnd, p(tab), None))
        torch.cuda.synchronize()
        _TABLES[key] = dict(N=N, C=Cb, tab=tab, T_host=np.ascontiguousarray(np.concatenate([nodes, list(T_range)])), nodes=nodes, T_range=T_range,
                            Q=Q, End=End, dead=np.tile(c["dead"], reps)[:nB], case=c, N_h=N.cpu().numpy().astype(np.float64),
                            C_h=Cb.cpu().numpy().astype(np.float64), G_h=tab.cpu().numpy().astype(np.float64).transpose(1, 2, 0))
    return _TABLES[key]


def band_subset(env, t, keep):
    """The tables of t with only the bands `keep` (a boolean mask), order kept."""
    torch = env["torch"]
    kd = torch.as_tensor(np.flatnonzero(keep), device="cuda")
    return dict(t, N=t["N"][kd].contiguous(), C=t["C"][kd].contiguous(), tab=t["tab"][:, :, kd].contiguous(), dead=t["dead"][keep],
                N_h=t["N_h"][keep], C_h=t["C_h"][keep], G_h=t["G_h"][:, keep])


def _ptr(x):
    return C.c_void_p(x.data_ptr()) if x is not None else None


def _front(env, t):
    nEnd, Q, nB = t["tab"].shape
    return nB, Q, t["T_host"].ctypes.data_as(C.c_void_p), _ptr(t["N"]), _ptr(t["C"]), _ptr(t["tab"]), nEnd


def forward(env, t, sc):
    """rtx_srf_pixel_cube itself -> float32 [nB][nPix] NumPy."""
    torch = env["torch"]
    nPix, nMix = sc["kidx"].shape
    cube = torch.empty((t["tab"].shape[2], nPix), dtype=torch.float32, device="cuda")
    k_d, f_d, T_d = dev(env, sc["kidx"]), dev(env, sc["frac"]), dev(env, sc["T"])  # held until the call has run
    env["_lib"].check(env["lib"].rtx_srf_pixel_cube(*_front(env, t), nPix, nMix, _ptr(k_d), _ptr(f_d), _ptr(T_d), _ptr(cube),
                                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return cube.cpu().numpy()


OUTS = ("cost", "grad", "hess", "step")


def normal(env, t, sc, meas, w=None, lam=None, outs=OUTS):
    """rtx_srf_pixel_cube_normal itself at (sc["T"], sc["frac"]) -> dict of NumPy; "cost" always."""
    torch = env["torch"]
    nPix, nMix = sc["kidx"].shape
    nU = nMix + 1
    shapes = dict(cost=(nPix,), grad=(nPix, nU), hess=(nPix, nU * (nU + 1) // 2), step=(nPix, nU))
    o = {k: torch.full(shapes[k], 7.0, dtype=torch.float64, device="cuda") for k in set(outs) | {"cost"}}
    meas_d = dev(env, meas)
    assert meas_d.dtype == torch.float32 and tuple(meas_d.shape) == (t["tab"].shape[2], nPix)
    w_d = None if w is None else dev(env, np.asarray(w, dtype=np.float32))
    lam_d = None if lam is None else dev(env, np.broadcast_to(np.asarray(lam, dtype=np.float64), (nPix,)))
    k_d, f_d, T_d = dev(env, sc["kidx"]), dev(env, sc["frac"]), dev(env, sc["T"])  # held until the call has run
    assert k_d.dtype == torch.int32 and f_d.dtype == torch.float32 and T_d.dtype == torch.float64
    env["_lib"].check(env["lib"].rtx_srf_pixel_cube_normal(*_front(env, t), nPix, nMix, _ptr(k_d), _ptr(f_d), _ptr(T_d), _ptr(meas_d), _ptr(w_d),
                                                           _ptr(lam_d), _ptr(o["cost"]),
                                                           _ptr(o.get("grad")), _ptr(o.get("hess")), _ptr(o.get("step")),
                                                           C.c_void_p(torch.cuda.current_stream().cuda_stream), 0))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def fit(env, t, kidx, meas, w=None, start=None, max_iter=FT.TRIALS, lambda0=1e-3, ftol=0.0):
    """rtx_srf_pixel_cube_fit itself -> dict of NumPy (T, frac, cost, n_iter, status, hess). start: (T, frac) or None (the scan)."""
    torch = env["torch"]
    nPix, nMix = kidx.shape
    nU = nMix + 1
    T_d = dev(env, start[0]) if start is not None else torch.full((nPix,), 7.0, dtype=torch.float64, device="cuda")
    f_d = dev(env, start[1]) if start is not None else torch.full((nPix, nMix), 7.0, dtype=torch.float32, device="cuda")
    assert T_d.dtype == torch.float64 and f_d.dtype == torch.float32
    cost = torch.full((nPix,), 7.0, dtype=torch.float64, device="cuda")
    hess = torch.full((nPix, nU * (nU + 1) // 2), 7.0, dtype=torch.float64, device="cuda")
    n_iter, status = (torch.full((nPix,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    w_d = None if w is None else dev(env, np.asarray(w, dtype=np.float32))
    k_d, meas_d = dev(env, kidx), dev(env, meas)  # held until the call has run
    assert k_d.dtype == torch.int32 and meas_d.dtype == torch.float32 and tuple(meas_d.shape) == (t["tab"].shape[2], nPix)
    env["_lib"].check(env["lib"].rtx_srf_pixel_cube_fit(*_front(env, t), nPix, nMix, _ptr(k_d), _ptr(meas_d), _ptr(w_d), _ptr(f_d),
                                                        _ptr(T_d), int(max_iter), float(lambda0), float(ftol), _ptr(cost), _ptr(n_iter), _ptr(status),
                                                        _ptr(hess), C.c_void_p(torch.cuda.current_stream().cuda_stream), GIVEN if start is not None else 0))
    torch.cuda.synchronize()
    return dict(T=T_d.cpu().numpy(), frac=f_d.cpu().numpy(), cost=cost.cpu().numpy(), n_iter=n_iter.cpu().numpy(), status=status.cpu().numpy(),
                hess=hess.cpu().numpy())


def cut(sc, sel):
    return dict(kidx=np.ascontiguousarray(sc["kidx"][sel]), frac=np.ascontiguousarray(sc["frac"][sel]), T=np.ascontiguousarray(sc["T"][sel]))


def away(sc, T_range, seed=19):
    """A start away from the truth: T moved by up to a quarter of the range (kept inside), the fractions by up to 0.2."""
    r = np.random.default_rng(seed)
    T = np.clip(sc["T"] + r.uniform(-0.25, 0.25, sc["T"].size) * (T_range[1] - T_range[0]), *T_range)
    return dict(kidx=sc["kidx"], frac=(sc["frac"] + r.uniform(-0.2, 0.2, sc["frac"].shape)).astype(np.float32), T=T)


def same(a, b, keys=None):
    for k in (keys or a):
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=True), k


def scene_of(t, sname, nPix=FT.NPIX, seed=5):
    nMix, nEnd = FT.SCENES[sname]
    return FT.distinct_scene(nPix, nMix, nEnd, t["T_range"], seed=seed)


_FIRST = {}


def first_case(env):
    """(device tables, the scene, meas = the forward's cube at the truth, a start away from it, normal's outputs there with a
    random damping) of FIRST, run once."""
    if not _FIRST:
        knots, sname, tname = FIRST
        t = device_tables(env, knots, FT.SCENES[sname][1], tname)
        sc = scene_of(t, sname)
        meas = forward(env, t, sc)
        st = away(sc, t["T_range"])
        lam = np.random.default_rng(29).uniform(0.0, 0.5, FT.NPIX)
        _FIRST["v"] = (t, sc, meas, st, lam, normal(env, t, st, meas, lam=lam))
    return _FIRST["v"]


def host_loop(env, t, kidx, meas, start, k, lambda0, ftol, w=None):
    """k host-driven trials built from rtx_srf_pixel_cube_normal, with the trial point and the accept rule in torch fp64: what
    rtx_srf_pixel_cube_fit(max_iter = k) computes, as NumPy under fit()'s keys. start: (T, frac) of RTX_FIT_START_GIVEN, or
    None: the start is the device's own scan (the fit with max_iter = 0), and a pixel the scan gives up (status 3) stays given
    up. Returns (the dict, the number of trial temperatures that were clamped at an end of the range, the number of lanes
    that stopped because lambda reached its cap)."""
    torch = env["torch"]
    nPix, nMix = kidx.shape
    T_lo, T_hi = t["T_range"]
    tt = lambda a: torch.as_tensor(np.array(a), device="cuda")
    status = torch.full((nPix,), -1, dtype=torch.int32, device="cuda")
    if start is None:
        s0 = fit(env, t, kidx, meas, w=w, max_iter=0)
        assert np.all((s0["status"] == 1) | (s0["status"] == 3)) and np.all(s0["n_iter"] == 0)
        lost = s0["status"] == 3
        status[tt(lost)] = 3
        T0, f0 = np.where(lost, 0.5 * (T_lo + T_hi), s0["T"]), np.where(lost[:, None], np.float32(0.0), s0["frac"])
    else:
        T0, f0 = np.array(start[0], dtype=np.float64), np.array(start[1], dtype=np.float32)
        bad = ~(VC.admitted(T0, t["T_range"]) & np.all(np.isfinite(f0), axis=1))
        status[tt(bad)] = 2
        T0[bad], f0[bad] = T_lo, 0.0
    T, f = tt(T0), tt(f0)
    call = lambda T_, f_, lam_, outs: {key: tt(v) for key, v in normal(env, t, dict(kidx=kidx, frac=f_.cpu().numpy(), T=T_.cpu().numpy()), meas, w=w,
                                                                         lam=lam_.cpu().numpy(), outs=outs).items()}
    lam = torch.full((nPix,), lambda0, dtype=torch.float64, device="cuda")
    cur = call(T, f, lam, ("cost", "hess"))
    status[(status < 0) & ~torch.isfinite(cur["cost"])] = 3  # no finite cost to start from
    n_iter = torch.zeros(nPix, dtype=torch.int32, device="cuda")
    clamped, capped = 0, 0
    for _ in range(k + 1):
        status[(status < 0) & (cur["cost"] == 0.0)] = 0
        status[(status < 0) & (n_iter >= k)] = 1
        run = status < 0
        if not bool(run.any()):
            break
        step = call(T, f, lam, ("step",))["step"]
        sing = run & torch.isnan(step).any(dim=1)
        status[sing] = 3
        run = status < 0
        step = torch.where(run[:, None], step, torch.zeros_like(step))
        raw_T = T + step[:, 0]
        Tt = torch.clamp(raw_T, min=T_lo, max=T_hi)
        clamped += int((run & (Tt != raw_T)).sum())
        ft = (f.double() + step[:, 1:]).float()
        tr = call(Tt, ft, lam, ("cost", "hess"))
        n_iter[run] += 1
        acc = run & (tr["cost"] < cur["cost"])
        rej = run & ~acc
        small = acc & (cur["cost"] - tr["cost"] < ftol * cur["cost"])
        T, f = torch.where(acc, Tt, T), torch.where(acc[:, None], ft, f)
        cur = {key: torch.where(acc.reshape((-1,) + (1,) * (cur[key].dim() - 1)), tr[key], cur[key]) for key in cur}
        lam = torch.where(acc, torch.clamp(0.1 * lam, min=FT.LAM_MIN), torch.where(rej, torch.clamp(10.0 * lam, max=FT.LAM_MAX), lam))
        status[small] = 0
        cap = rej & (lam >= FT.LAM_MAX)
        capped += int(cap.sum())
        status[cap] = 0
    gone = (status >= 2).cpu().numpy()  # a pixel that is refused or given up: NaN in every floating output
    out = dict(T=T, frac=f, cost=cur["cost"], hess=cur["hess"], n_iter=n_iter, status=status)
    out = {key: v.cpu().numpy() for key, v in out.items()}
    for key in ("T", "frac", "cost", "hess"):
        out[key][gone] = np.nan
    return out, clamped, capped


def check_normal(env, t, st, meas, what, w=None):
    """normal's cost, grad and hess against the oracle on the device's tables; its step against ITS OWN hess, grad and
    damping in fp64, so that no condition number enters: with A = H + lam diag H, n = 1 + nMix and u = 2^-53, a Cholesky solve
    leaves |A step + grad|_i <= gamma_(3n+1) sqrt(a_ii) sum_j sqrt(a_jj) |step_j| (Higham, Accuracy and Stability of Numerical
    Algorithms, th. 10.4 with |R^T||R|_ij <= sqrt(a_ii a_jj)). Asserted: twice that, plus (n + 1) u (|A||step| + |grad|)_i for
    this function's own evaluation of the residual."""
    Q = t["Q"]
    nMix = st["kidx"].shape[1]
    lam = np.random.default_rng(31).uniform(0.0, 0.5, st["T"].size)
    got = normal(env, t, st, meas, w=w, lam=lam)
    o = FT.evaluate(t["N_h"], t["C_h"], t["G_h"], t["nodes"], st["kidx"], st["frac"], st["T"], meas, w)
    within(got["cost"], o["cost"], o["scale"]["cost"], K_COST(Q, nMix), what + " cost")
    within(got["grad"], o["grad"], o["scale"]["grad"], K_GRAD(Q, nMix), what + " grad")
    within(got["hess"], o["hess"], o["scale"]["hess"], K_H(Q), what + " hess")
    A = FT.unpack(got["hess"])
    n = A.shape[1]
    A = A + lam[:, None, None] * A * np.eye(n)[None]
    u = 2.0 ** -53
    sd = np.sqrt(np.einsum("pii->pi", A))
    res = np.abs(np.einsum("pij,pj->pi", A, got["step"]) + got["grad"])
    lim = (3 * n + 1) * u * sd * np.sum(sd * np.abs(got["step"]), axis=1, keepdims=True)
    own = (n + 1) * u * (np.einsum("pij,pj->pi", np.abs(A), np.abs(got["step"])) + np.abs(got["grad"]))
    print("%s step: worst residual of the device's own system / the Cholesky residual bound = %.3g" % (what, float(np.max(res / lim))))
    assert np.all(np.isfinite(got["step"])) and np.all(res <= 2.0 * lim + own)
    return got


# ---------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("tname", list(CC.T_CONFIGS))
@pytest.mark.parametrize("sname", list(FT.SCENES))
@pytest.mark.parametrize("knots", CC.KNOTS)
def test_normal_against_oracle(env, knots, sname, tname):
    """257 pixels at a start away from the truth, meas the forward's cube at the truth: mixtures of 1 and 3 out of 8 (the table
    slice in LDS) and of 4 out of 31 (31 x 8 and 31 x 5 > 128: the table read from global memory); 8 nodes and 5.
    MEASURED on an MI355X, worst of the 12 cases, in units of 2^-24 scale: cost 0.11 (k = 19 .. 31), grad 0.56 (k = 17 .. 26),
    hess 2.9 (k = 15 / 21); the step's residual at most 0.48 of the Cholesky residual bound."""
    t = device_tables(env, knots, FT.SCENES[sname][1], tname)
    sc = scene_of(t, sname)
    meas = forward(env, t, sc)
    check_normal(env, t, away(sc, t["T_range"]), meas, "srf cube normal %s %s %s" % (knots, sname, tname))


def test_more_than_one_band_block(env):
    """80 bands (the 20 bands four times) are two blocks of 64, the second one 16 bands wide, with weights of which two are
    zero: against the oracle; the cost is the 20-band cost's sum over the repeats when the weights repeat (fp64 sums of the
    same terms in another order: to 1e-12).
    MEASURED: cost 0.091, grad 0.38, hess 1.9; the step's residual 0.25 of its bound."""
    t, sc, meas, st, _, _ = first_case(env)
    t4 = device_tables(env, FIRST[0], FT.SCENES[FIRST[1]][1], FIRST[2], times=4)
    assert t4["N_h"].shape == (80,) and np.array_equal(t4["N_h"][:20], t4["N_h"][60:])
    meas4 = np.ascontiguousarray(np.tile(meas, (4, 1)))
    w = np.random.default_rng(33).uniform(0.5, 2.0, 80).astype(np.float32)
    w[[7, 70]] = 0.0
    check_normal(env, t4, st, meas4, "srf cube normal 80 bands", w=w)
    one = normal(env, t, st, meas, outs=("cost",))["cost"]
    four = normal(env, t4, st, meas4, outs=("cost",))["cost"]
    assert np.allclose(four, 4.0 * one, rtol=1e-12, atol=0.0)


def test_the_forward_bits(env):
    """y has the forward's bits: with meas = rtx_srf_pixel_cube's own output at (T, f), cost == 0.0 and grad == 0.0 exactly,
    and the fit from that start returns n_iter 0, status 0, T and frac unchanged bit for bit -- with the table in LDS and in
    global memory, 8 nodes and 5."""
    for knots, sname, tname in (FIRST, ("dense", "mix4_of_31", "285-315_Q5"), ("coarse", "mix1_of_8", "285-315_Q5")):
        t = device_tables(env, knots, FT.SCENES[sname][1], tname)
        sc = scene_of(t, sname)
        meas = forward(env, t, sc)
        got = normal(env, t, sc, meas)
        assert np.all(got["cost"] == 0.0) and np.all(got["grad"] == 0.0) and np.all(got["step"] == 0.0) and np.all(got["hess"][:, 0] > 0.0)
        r = fit(env, t, sc["kidx"], meas, start=(sc["T"], sc["frac"]))
        assert np.all(r["n_iter"] == 0) and np.all(r["status"] == 0) and np.all(r["cost"] == 0.0)
        assert np.array_equal(r["T"], sc["T"]) and np.array_equal(r["frac"], sc["frac"]) and np.array_equal(r["hess"], got["hess"])


def test_masks(env):
    """A NaN in meas under a dead band or under a band of weight zero changes no bit; a pixel that is not admitted (NaN, just
    outside the range, infinite) is NaN in its own outputs only -- status 2 in the fit, with a NaN fraction too -- and its
    neighbours keep their bits; kidx out of range gives the bits of the clamped indices."""
    t, sc, meas, st, lam, whole = first_case(env)
    dead = t["dead"]
    assert dead.sum() == 3 and np.isnan(meas[dead]).all()
    for v in whole.values():
        assert np.all(np.isfinite(v))
    w = np.ones(20, dtype=np.float32)
    w[[2, 9]] = 0.0
    base_w = normal(env, t, st, meas, w=w, lam=lam)
    m2 = np.where(dead[:, None], np.float32(1e30), meas)
    m2[[2, 9]] = np.nan
    same(normal(env, t, st, m2, w=w, lam=lam), base_w)
    assert not np.array_equal(base_w["cost"], whole["cost"])
    fit_w = fit(env, t, sc["kidx"], meas, w=w, start=(st["T"], st["frac"]), max_iter=6)
    same(fit(env, t, sc["kidx"], m2, w=w, start=(st["T"], st["frac"]), max_iter=6), fit_w)
    bad_T = {3: np.nan, 70: np.nextafter(t["T_range"][1], np.inf), 200: np.nextafter(t["T_range"][0], -np.inf), 201: np.inf}
    s2 = {k: np.array(v) for k, v in st.items()}
    for i, v in bad_T.items():
        s2["T"][i] = v
    bad = np.zeros(FT.NPIX, dtype=bool)
    bad[list(bad_T)] = True
    got = normal(env, t, s2, meas, lam=lam)
    for k in OUTS:
        nan = np.isnan(got[k]).reshape(FT.NPIX, -1)
        assert np.array_equal(nan, np.repeat(bad[:, None], nan.shape[1], axis=1)), k
        assert np.array_equal(got[k][~bad], whole[k][~bad]), k
    s2["frac"][100, 1] = np.nan
    bad[100] = True
    plain = fit(env, t, sc["kidx"], meas, start=(st["T"], st["frac"]), max_iter=6)
    r = fit(env, t, sc["kidx"], meas, start=(s2["T"], s2["frac"]), max_iter=6)
    assert np.array_equal(r["status"] == 2, bad) and np.all(r["n_iter"][bad] == 0) and np.all(plain["status"] <= 1)
    for k in ("T", "frac", "cost", "hess"):
        nan = np.isnan(r[k]).reshape(FT.NPIX, -1)
        assert np.array_equal(nan, np.repeat(bad[:, None], nan.shape[1], axis=1)), k
    for k in r:
        assert np.array_equal(r[k][~bad], plain[k][~bad]), k
    s3 = {k: np.array(v) for k, v in st.items()}
    lo, hi = s3["kidx"] == 0, s3["kidx"] == 7
    assert lo.any() and hi.any()
    s3["kidx"][lo], s3["kidx"][hi] = -1, 8
    s3["kidx"][5, 0] = -2**31 if st["kidx"][5, 0] == 0 else s3["kidx"][5, 0]
    same(normal(env, t, s3, meas, lam=lam), whole)
    same(fit(env, t, s3["kidx"], meas, start=(st["T"], st["frac"]), max_iter=6), plain)


@pytest.mark.parametrize("k", (1, 3, 8))
def test_fit_equals_a_host_loop_over_normal(env, k):
    """fit(START_GIVEN, max_iter = k) equals, bit for bit, k host-driven trials built from rtx_srf_pixel_cube_normal with the
    trial point and the accept rule in torch fp64: T, frac, cost, hess, n_iter and status. One pixel starts on the truth
    (cost 0: it stops before any trial). An ftol of 0.3 stops pixels early: with k = 8, 121 of the 257 end with status 0 after
    1 to 8 trials, the rest at the cap."""
    t, sc, meas, st, _, _ = first_case(env)
    lambda0, ftol = 1e-3, 0.3
    T0, f0 = np.array(st["T"]), np.array(st["frac"])
    T0[9], f0[9] = sc["T"][9], sc["frac"][9]
    got = fit(env, t, sc["kidx"], meas, start=(T0, f0), max_iter=k, lambda0=lambda0, ftol=ftol)
    want, _, _ = host_loop(env, t, sc["kidx"], meas, (T0, f0), k, lambda0, ftol)
    assert int(got["n_iter"][9]) == 0 and int(got["status"][9]) == 0
    print("srf cube fit vs host loop k=%d: trials %s, statuses %s" % (k, np.bincount(got["n_iter"]).tolist(), np.bincount(got["status"]).tolist()))
    assert got["n_iter"].max() == k and (got["status"] == 1).any()
    for key, v in want.items():
        assert np.array_equal(got[key], v), key


def test_purity(env):
    """The same bits run to run; for the 257-pixel scene's first n pixels, n = 1, 63, 64, 65, 256; for a permuted scene; in
    normal whichever optional outputs are asked for; and with the table slice in LDS (8 endmembers) against global memory (the
    same 8 followed by 9 unused columns: 17 x 8 > 128). normal at a start, and the fit from the scan with 12 trials."""
    t, sc, meas, st, lam, whole = first_case(env)
    fit_whole = fit(env, t, sc["kidx"], meas, max_iter=12)
    same(normal(env, t, st, meas, lam=lam), whole)
    same(fit(env, t, sc["kidx"], meas, max_iter=12), fit_whole)
    for n in (1, 63, 64, 65, 256):
        part = normal(env, t, cut(st, slice(0, n)), np.ascontiguousarray(meas[:, :n]), lam=lam[:n])
        same(part, {k: v[:n] for k, v in whole.items()})
        same(fit(env, t, sc["kidx"][:n], np.ascontiguousarray(meas[:, :n]), max_iter=12), {k: v[:n] for k, v in fit_whole.items()})
    perm = np.random.default_rng(3).permutation(FT.NPIX)
    same(normal(env, t, cut(st, perm), np.ascontiguousarray(meas[:, perm]), lam=lam[perm]), {k: v[perm] for k, v in whole.items()})
    same(fit(env, t, sc["kidx"][perm], np.ascontiguousarray(meas[:, perm]), max_iter=12), {k: v[perm] for k, v in fit_whole.items()})
    for outs in (("cost",), ("grad",), ("hess",), ("step",), ("grad", "step")):
        alone = normal(env, t, st, meas, lam=lam, outs=outs)
        assert set(alone) == set(outs) | {"cost"}
        same(alone, whole, keys=alone)
    t17 = device_tables(env, FIRST[0], 17, FIRST[2])
    assert np.array_equal(t17["G_h"][:, :, :8], t["G_h"]) and t17["tab"].shape[0] * t17["Q"] > 128
    same(normal(env, t17, st, meas, lam=lam), whole)
    same(fit(env, t17, sc["kidx"], meas, max_iter=12), fit_whole)


@pytest.mark.parametrize("tname", list(CC.T_CONFIGS))
@pytest.mark.parametrize("sname", list(FT.SCENES))
@pytest.mark.parametrize("knots", CC.KNOTS)
def test_recovery_from_the_scan(env, knots, sname, tname):
    """The scan start, 40 trials, meas = the device's forward at the truth: T and the fractions within the sensitivity bound
    of the truth AND of the fp64 restatement run on the same meas and device tables; the cost never above the start's (the
    scan alone, max_iter = 0); statuses 0 or 1.
    MEASURED on an MI355X, worst of the 12 cases: |got - truth| 0.0078 of the bound, |got - restatement| 0.0063 of the bound,
    worst |dT| 4.4e-4 K; 2 to 40 trials per pixel."""
    t = device_tables(env, knots, FT.SCENES[sname][1], tname)
    sc = scene_of(t, sname)
    meas = forward(env, t, sc)
    args = (t["N_h"], t["C_h"], t["G_h"], t["nodes"])
    bound = FT.sensitivity_bound(*args, sc)
    got = fit(env, t, sc["kidx"], meas)
    want = FT.fit(*args, t["T_range"], sc["kidx"], meas)
    u = lambda T, f: np.concatenate([np.asarray(T)[:, None], np.asarray(f).astype(np.float64)], axis=1)
    r_true = np.abs(u(got["T"], got["frac"]) - u(sc["T"], sc["frac"])) / bound
    r_rest = np.abs(u(got["T"], got["frac"]) - u(want["T"], want["frac"])) / bound
    print("srf cube fit recovery %s %s %s: worst |got - truth| / bound = %.3g, worst |got - restatement| / bound = %.3g, worst |dT| = %.3g K, "
          "trials %d .. %d, statuses %r" % (knots, sname, tname, r_true.max(), r_rest.max(), np.abs(got["T"] - sc["T"]).max(), got["n_iter"].min(),
                                            got["n_iter"].max(), np.unique(got["status"]).tolist()))
    assert np.all(got["status"] <= 1) and np.all(got["n_iter"] <= FT.TRIALS) and np.all(np.isfinite(got["hess"]))
    start = fit(env, t, sc["kidx"], meas, max_iter=0)  # the scan alone: the start's cost
    assert np.all(start["status"] == 1) and np.all(start["n_iter"] == 0) and np.all(got["cost"] <= start["cost"])
    assert np.all(r_true <= 1.0) and np.all(r_rest <= 1.0)


def test_zero_weights_remove_bands(env):
    """wgt of 0 on two bands equals the fit (and normal) on the scene with those bands removed, bit for bit."""
    t, sc, meas, st, lam, _ = first_case(env)
    w = np.ones(20, dtype=np.float32)
    w[[1, 16]] = 0.0
    keep = w > 0.0
    ts = band_subset(env, t, keep)
    ms = np.ascontiguousarray(meas[keep])
    same(normal(env, t, st, meas, w=w, lam=lam), normal(env, ts, st, ms, lam=lam))
    same(normal(env, t, st, meas, w=w, lam=lam), normal(env, ts, st, ms, w=w[keep], lam=lam))
    a, b = fit(env, t, sc["kidx"], meas, w=w, max_iter=12), fit(env, ts, sc["kidx"], ms, max_iter=12)
    same(a, b)
    assert np.all(a["status"] <= 1) and not np.array_equal(a["cost"], fit(env, t, sc["kidx"], meas, max_iter=12)["cost"])


def test_python_entries(env):
    """sensor.hsi_cube_srf_normal and hsi_cube_srf_fit are the raw entries on hsi_cube_srf's own tables, bit for bit."""
    torch, sensor = env["torch"], env["sensor"]
    t, sc, meas, st, lam, whole = first_case(env)
    c = t["case"]
    s = sensor.Sensor.from_tables(c["tables"])
    grid = env["engine"].Grid(*FC.grid_tuple(env["CH"]))
    base = (grid, dev(env, c["tau"]), dev(env, c["La"]), dev(env, c["Ld"]), c["Xk"], dev(env, t["End"]), dev(env, sc["kidx"]))
    out = sensor.hsi_cube_srf_normal(*base, dev(env, st["frac"]), dev(env, st["T"]), s, dev(env, meas), damping=dev(env, lam), n_nodes=t["Q"],
                                     T_range=t["T_range"])
    same({k: v.cpu().numpy() for k, v in out.items()}, whole)
    r = sensor.hsi_cube_srf_fit(*base, dev(env, meas), s, t["T_range"], max_iter=12, n_nodes=t["Q"])
    want = fit(env, t, sc["kidx"], meas, max_iter=12)
    assert set(r) == {"Tpix", "frac", "cost", "n_iter", "status", "hess"}
    same({("T" if k == "Tpix" else k): v.cpu().numpy() for k, v in r.items()}, want)
    r = sensor.hsi_cube_srf_fit(*base, dev(env, meas), s, t["T_range"], frac0=dev(env, st["frac"]), T0=dev(env, st["T"]), weights=np.ones(20),
                                max_iter=6, lambda0=1e-2, ftol=1e-3, n_nodes=t["Q"])
    want = fit(env, t, sc["kidx"], meas, w=np.ones(20), start=(st["T"], st["frac"]), max_iter=6, lambda0=1e-2, ftol=1e-3)
    same({("T" if k == "Tpix" else k): v.cpu().numpy() for k, v in r.items()}, want)


def test_refusals_write_nothing(env):
    """Every refusal returns non-zero and leaves the canary-filled outputs alone; nB == 0 and nPix == 0 return 0 and write
    nothing; the same arguments, well formed, do write."""
    torch, lib = env["torch"], env["lib"]
    nB, Q, nEnd, nPix, nMix = 3, 2, 4, 70, 2
    f32 = lambda *shape: torch.rand(shape, dtype=torch.float32, device="cuda") + 0.5
    N, Cb, tab, meas = f32(nB), f32(nB), f32(nEnd, Q, nB), f32(nB, nPix)
    kidx = torch.stack([torch.randperm(nEnd)[:nMix] for _ in range(nPix)]).to(dtype=torch.int32, device="cuda")
    frac = torch.full((nPix, nMix), 0.4, dtype=torch.float32, device="cuda")
    Tpix = torch.full((nPix,), 300.0, dtype=torch.float64, device="cuda")
    cost, grad, hess, step = (torch.full(s, 7.0, dtype=torch.float64, device="cuda") for s in ((nPix,), (nPix, 3), (nPix, 6), (nPix, 3)))
    n_iter, status = (torch.full((nPix,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = np.array([310.0, 290.0, 285.0, 315.0])
    Tp = lambda T: np.ascontiguousarray(T, dtype=np.float64).ctypes.data_as(C.c_void_p)
    MM, IM = lib.rtx_srf_pixel_cube_fit_max_mix(), lib.rtx_srf_pixel_cube_fit_max_iter()

    def nrm(nB_=nB, Q_=Q, T=good, nPix_=nPix, nMix_=nMix, meas_=meas, cost_=cost, flags=0):
        return lib.rtx_srf_pixel_cube_normal(nB_, Q_, Tp(T), _ptr(N), _ptr(Cb), _ptr(tab), nEnd, nPix_, nMix_, _ptr(kidx), _ptr(frac), _ptr(Tpix),
                                             _ptr(meas_), None, None, _ptr(cost_), _ptr(grad), _ptr(hess), _ptr(step), st, flags)

    def ft(nB_=nB, Q_=Q, T=good, nPix_=nPix, nMix_=nMix, meas_=meas, cost_=cost, max_iter=5, lambda0=1e-3, ftol=0.0, flags=GIVEN):
        return lib.rtx_srf_pixel_cube_fit(nB_, Q_, Tp(T), _ptr(N), _ptr(Cb), _ptr(tab), nEnd, nPix_, nMix_, _ptr(kidx), _ptr(meas_), None, _ptr(frac),
                                          _ptr(Tpix), max_iter, lambda0, ftol, _ptr(cost_), _ptr(n_iter), _ptr(status), _ptr(hess), st, flags)

    shared = (dict(Q_=0), dict(nB_=-1), dict(nPix_=-1), dict(nMix_=0), dict(nMix_=MM + 1), dict(meas_=None), dict(cost_=None),
              dict(T=[310.0, np.nan, 285.0, 315.0]), dict(T=[300.0, 300.0, 285.0, 315.0]), dict(T=[310.0, 290.0, 291.0, 315.0]))
    for kw in shared + (dict(flags=1),):
        assert nrm(**kw) != 0 and lib.rtx_last_error(), kw
    for kw in shared + (dict(flags=2), dict(max_iter=-1), dict(max_iter=IM + 1), dict(lambda0=-1.0), dict(lambda0=float("nan")), dict(ftol=float("inf"))):
        assert ft(**kw) != 0 and lib.rtx_last_error(), kw
    assert nrm(nPix_=0) == 0 and nrm(nB_=0) == 0 and ft(nPix_=0) == 0 and ft(nB_=0) == 0
    torch.cuda.synchronize()
    for v in (cost, grad, hess, step):
        assert bool((v == 7.0).all())
    assert bool((n_iter == -7).all()) and bool((status == -7).all()) and bool((frac == 0.4).all()) and bool((Tpix == 300.0).all())
    assert nrm() == 0
    torch.cuda.synchronize()
    for v in (cost, grad, hess):
        assert bool(torch.isfinite(v).all()) and bool((v != 7.0).all())
    assert bool((step != 7.0).all())
    assert ft() == 0
    torch.cuda.synchronize()
    assert bool((n_iter >= 0).all()) and bool((n_iter <= 5).all()) and bool((status >= 0).all()) and bool((status <= 3).all())


def test_compute_hsi_cube_fit_end_to_end():
    """rt.compute_hsi_cube_fit on a small line-table scene (a thinned standard atmosphere, 2 cm^-1, eight triangular bands and
    one off the axis, 65 pixels of 2 out of 8 endmembers): meas is hsi_cube_srf's cube on compute_TUD's outputs, and the fit from
    the scan recovers the scene within the sensitivity bound evaluated on the device's own tables.
    MEASURED: worst |got - truth| 0.0063 of the bound (bounds on T 0.003 .. 0.03 K), at most 29 trials, every status 0."""
    import torch
    assert torch.cuda.is_available()
    from radtxfr_amd import _lib, engine, sensor, synthetic
    from radtxfr_amd import radiative_transfer as rt
    lo, hi, dv = 1000.0, 1002.0, 0.0005
    sub = synthetic.subset_table(synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0), lo - 12.0, hi + 12.0)
    sa = rt.StdAtmos
    a = dict(Zs=sa[:, 1], Ts=sa[:, 5].copy(), Ps=sa[:, 4], PLs=sa[:, 3], MFs_VAL=sa[:, 6:9] * 1e6 * E2E_THIN, MFs_ID=np.array([1, 2, 3]))
    kw = dict(DVOUT=dv, line_table=sub, Altitudes=np.array([8.0]), **a)
    s = sensor.Sensor.from_shape(list(np.linspace(1000.15, 1001.85, 8)) + [1004.5], 0.2, "triangle")  # the last one off the axis: a dead band
    Xk = np.array([999.9, 1000.4, 1000.9, 1001.4, 1002.1])
    nB, nk, nEnd, Q, T_range, nPix = 9, 5, 8, 8, (230.0, 350.0), 65
    End = CC.endmembers(nk, nEnd)
    sc = FT.distinct_scene(nPix, 2, nEnd, T_range)
    X, tau, La, Ld = rt.compute_TUD(lo, hi, **kw)
    grid = engine.Grid(lo, hi, X.size)
    d32 = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float32).ravel(), device="cuda")
    dv_ = lambda v: torch.as_tensor(np.array(v), device="cuda")
    t_d, a_d, d_d = d32(tau), d32(La), d32(Ld)
    meas = sensor.hsi_cube_srf(grid, t_d, a_d, d_d, Xk, dv_(End), dv_(sc["kidx"]), dv_(sc["frac"]), dv_(sc["T"]), s, n_nodes=Q, T_range=T_range)[1]
    meas = meas.cpu().numpy()
    assert np.isnan(meas[8]).all() and np.isfinite(meas[:8]).all()
    X_out, r = rt.compute_hsi_cube_fit(lo, hi, s, Xk, End, sc["kidx"], meas, T_range, max_iter=FT.TRIALS, n_nodes=Q, **kw)
    assert np.array_equal(X_out, s.centres) and set(r) == {"Tpix", "frac", "cost", "n_iter", "status", "hess"}
    assert r["Tpix"].shape == (nPix,) and r["frac"].shape == (nPix, 2) and r["frac"].dtype == np.float32 and r["hess"].shape == (nPix, 6)
    lib = _lib.load()
    nodes = sensor.srf_cube_nodes(T_range[0], T_range[1], Q)
    N, Cb, M, jr = sensor.srf_moments(grid, t_d, a_d, d_d, dv_(Xk), nodes, s)
    tab = torch.empty((nEnd, Q, nB), dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(lib.rtx_srf_cube_tables(p(M), p(jr), nB, Q, nk, p(dv_(End)), nEnd, p(tab), None))
    torch.cuda.synchronize()
    bound = FT.sensitivity_bound(N.cpu().numpy(), Cb.cpu().numpy(), tab.cpu().numpy().astype(np.float64).transpose(1, 2, 0), nodes, sc)
    got = np.concatenate([r["Tpix"][:, None], r["frac"].astype(np.float64)], axis=1)
    truth = np.concatenate([sc["T"][:, None], sc["frac"].astype(np.float64)], axis=1)
    ratio = np.abs(got - truth) / bound
    print("compute_hsi_cube_fit end to end: worst |got - truth| / bound = %.3g, bound on T %.3g .. %.3g K, tau %.3g .. %.3g, trials up to %d, statuses %r"
          % (ratio.max(), bound[:, 0].min(), bound[:, 0].max(), tau.min(), tau.max(), r["n_iter"].max(), np.unique(r["status"]).tolist()))
    assert np.all(r["status"] <= 1) and np.all(ratio <= 1.0)
