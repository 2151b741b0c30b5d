"""The bound-constrained per-pixel fit to a measured HSI cube (radtxfr_amd/csrc/rtx_srf_cube_fit_box.hip:
rtx_srf_pixel_cube_normal_box, rtx_srf_pixel_cube_fit_box; the nonneg / sum_weight keywords of sensor.hsi_cube_srf_normal /
hsi_cube_srf_fit and rt.compute_hsi_cube_fit) against the unconstrained kernels bit for bit where the box is not
felt, against the fp64 NumPy of tests/srf_cube_fit_box_cases.py evaluated on the device's own float32 N, C and table, against
a brute-force optimum, and against itself.

Shapes, scenes and helpers are tests/test_gpu_srf_cube_fit.py's (257 pixels: four workgroups of 64 and one pixel of a fifth);
the noisy scenes (noise 1e-3 of a band's largest radiance, half the pixels with one absent endmember) are
srf_cube_fit_box_cases.noisy_scene / add_noise on the forward kernel's own cube."""
import ctypes as C

import numpy as np
import pytest

import srf_cube_cases as CC
import srf_cube_fit_box_cases as BX
import srf_cube_fit_cases as FT
import srf_fused_cases as FC
import test_gpu_srf_cube_fit as GF
from test_gpu_sensor_vjp import within
from test_gpu_srf_cube_fit import env  # noqa: F401

pytestmark = pytest.mark.gpu

FIRST = GF.FIRST
MIX4 = ("dense", "mix4_of_31", "230-350_Q8")  # 31 x 8 > 128: the table read from global memory
GIVEN = GF.GIVEN
_ptr, dev = GF._ptr, GF.dev


def normal_box(env, t, sc, meas, w=None, lam=None, delta=0.0, outs=GF.OUTS, active=True):
    """rtx_srf_pixel_cube_normal_box itself at (sc["T"], sc["frac"]) -> dict of NumPy; "cost" always, "active" unless not asked."""
    torch = env["torch"]
    nPix, nMix = sc["kidx"].shape
    nU = nMix + 1
    shapes = dict(cost=(nPix,), grad=(nPix, nU), hess=(nPix, nU * (nU + 1) // 2), step=(nPix, nU))
    o = {k: torch.full(shapes[k], 7.0, dtype=torch.float64, device="cuda") for k in set(outs) | {"cost"}}
    if active:
        o["active"] = torch.full((nPix,), -7, dtype=torch.int32, device="cuda")
    meas_d = dev(env, meas)
    assert meas_d.dtype == torch.float32 and tuple(meas_d.shape) == (t["tab"].shape[2], nPix)
    w_d = None if w is None else dev(env, np.asarray(w, dtype=np.float32))
    lam_d = None if lam is None else dev(env, np.broadcast_to(np.asarray(lam, dtype=np.float64), (nPix,)))
    k_d, f_d, T_d = dev(env, sc["kidx"]), dev(env, np.asarray(sc["frac"], dtype=np.float32)), dev(env, sc["T"])  # held until the call has run
    env["_lib"].check(env["lib"].rtx_srf_pixel_cube_normal_box(*GF._front(env, t), nPix, nMix, _ptr(k_d), _ptr(f_d), _ptr(T_d), _ptr(meas_d),
                                                               _ptr(w_d), _ptr(lam_d), _ptr(o["cost"]), _ptr(o.get("grad")), _ptr(o.get("hess")),
                                                               _ptr(o.get("step")), C.c_void_p(torch.cuda.current_stream().cuda_stream), 0,
                                                               float(delta), _ptr(o.get("active"))))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def fit_box(env, t, kidx, meas, w=None, start=None, max_iter=FT.TRIALS, lambda0=1e-3, ftol=0.0, delta=0.0):
    """rtx_srf_pixel_cube_fit_box itself -> dict of NumPy (T, frac, cost, n_iter, status, hess, grad, active)."""
    torch = env["torch"]
    nPix, nMix = kidx.shape
    nU = nMix + 1
    T_d = dev(env, start[0]) if start is not None else torch.full((nPix,), 7.0, dtype=torch.float64, device="cuda")
    f_d = dev(env, start[1]) if start is not None else torch.full((nPix, nMix), 7.0, dtype=torch.float32, device="cuda")
    assert T_d.dtype == torch.float64 and f_d.dtype == torch.float32
    cost = torch.full((nPix,), 7.0, dtype=torch.float64, device="cuda")
    hess = torch.full((nPix, nU * (nU + 1) // 2), 7.0, dtype=torch.float64, device="cuda")
    grad = torch.full((nPix, nU), 7.0, dtype=torch.float64, device="cuda")
    n_iter, status, active = (torch.full((nPix,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    w_d = None if w is None else dev(env, np.asarray(w, dtype=np.float32))
    k_d, meas_d = dev(env, kidx), dev(env, meas)  # held until the call has run
    assert k_d.dtype == torch.int32 and meas_d.dtype == torch.float32 and tuple(meas_d.shape) == (t["tab"].shape[2], nPix)
    env["_lib"].check(env["lib"].rtx_srf_pixel_cube_fit_box(*GF._front(env, t), nPix, nMix, _ptr(k_d), _ptr(meas_d), _ptr(w_d), _ptr(f_d), _ptr(T_d),
                                                            int(max_iter), float(lambda0), float(ftol), _ptr(cost), _ptr(n_iter), _ptr(status),
                                                            _ptr(hess), C.c_void_p(torch.cuda.current_stream().cuda_stream),
                                                            GIVEN if start is not None else 0, float(delta), _ptr(grad), _ptr(active)))
    torch.cuda.synchronize()
    return dict(T=T_d.cpu().numpy(), frac=f_d.cpu().numpy(), cost=cost.cpu().numpy(), n_iter=n_iter.cpu().numpy(), status=status.cpu().numpy(),
                hess=hess.cpu().numpy(), grad=grad.cpu().numpy(), active=active.cpu().numpy())


_NOISY = {}


def noisy_case(env, knots, sname, tname, times=1):
    """(device tables, the noisy scene, meas = the forward's cube at its truth plus noise), made once per case."""
    key = (knots, sname, tname, times)
    if key not in _NOISY:
        nMix, nEnd = FT.SCENES[sname]
        t = GF.device_tables(env, knots, nEnd, tname, times=times)
        sc = BX.noisy_scene(FT.NPIX, nMix, nEnd, t["T_range"])
        _NOISY[key] = (t, sc, BX.add_noise(GF.forward(env, t, sc)))
    return _NOISY[key]


def rough_start(sc, T_range, seed=23):
    """A start with fractions at 0 and temperatures on the ends: the truth moved by up to 0.4 of the range in T (clipped
    into it) and by up to 0.2 in every fraction, then raised to 0."""
    r = np.random.default_rng(seed)
    T = np.clip(sc["T"] + r.uniform(-0.4, 0.4, sc["T"].size) * (T_range[1] - T_range[0]), *T_range)
    return dict(kidx=sc["kidx"], frac=BX.project(sc["frac"] + r.uniform(-0.2, 0.2, sc["frac"].shape).astype(np.float32)), T=T)


def host_loop(env, t, kidx, meas, start, k, lambda0, ftol, delta):
    """k host-driven trials built from rtx_srf_pixel_cube_normal_box, with the projected start, the trial point, the stop at a
    trial point that is the current point and the accept rule in NumPy fp64: what rtx_srf_pixel_cube_fit_box(START_GIVEN,
    max_iter = k) computes, under fit_box()'s keys. Also returns how many lanes the new stop ended."""
    nPix, nMix = kidx.shape
    T_range = t["T_range"]
    T, f = np.array(start[0], dtype=np.float64), np.array(start[1], dtype=np.float32)
    status = np.full(nPix, -1, dtype=np.int32)
    bad = ~(GF.VC.admitted(T, T_range) & np.all(np.isfinite(f), axis=1))
    status[bad] = 2
    T[bad], f[bad] = T_range[0], 0.0
    f = BX.project(f)
    call = lambda T_, f_, lam_, outs: normal_box(env, t, dict(kidx=kidx, frac=f_, T=T_), meas, lam=lam_, delta=delta, outs=outs, active=False)
    lam = np.full(nPix, float(lambda0))
    cur = call(T, f, lam, ("cost", "grad", "hess"))
    status[(status < 0) & ~np.isfinite(cur["cost"])] = 3
    n_iter = np.zeros(nPix, dtype=np.int32)
    still = 0
    for _ in range(k + 1):
        status[(status < 0) & (cur["cost"] == 0.0)] = 0
        status[(status < 0) & (n_iter >= k)] = 1
        run = status < 0
        if not run.any():
            break
        step = call(T, f, lam, ("step",))["step"]
        status[run & np.isnan(step).any(axis=1)] = 3
        run = status < 0
        Tt, ft = BX.trial_point(T, f, np.where(run[:, None], step, 0.0), T_range)
        same_pt = run & (Tt == T) & np.all(ft == f, axis=1)
        still += int(same_pt.sum())
        status[same_pt] = 0
        run = status < 0
        tr = call(Tt, ft, lam, ("cost", "grad", "hess"))
        n_iter[run] += 1
        with np.errstate(invalid="ignore"):
            acc = run & (tr["cost"] < cur["cost"])
        rej = run & ~acc
        small = acc & (cur["cost"] - tr["cost"] < ftol * cur["cost"])
        T, f = np.where(acc, Tt, T), np.where(acc[:, None], ft, f)
        cur = {key: np.where(acc.reshape((-1,) + (1,) * (cur[key].ndim - 1)), tr[key], cur[key]) for key in cur}
        lam = np.where(acc, np.maximum(0.1 * lam, FT.LAM_MIN), np.where(rej, np.minimum(10.0 * lam, FT.LAM_MAX), lam))
        status[small] = 0
        status[rej & (lam >= FT.LAM_MAX)] = 0
    gone = status >= 2
    active = np.where(gone, 0, BX.bits(BX.kkt_set(cur["grad"], T, f, T_range))).astype(np.int32)
    out = dict(T=T, frac=f.astype(np.float32), cost=cur["cost"], hess=cur["hess"], grad=cur["grad"], n_iter=n_iter, status=status, active=active)
    for key in ("T", "frac", "cost", "hess", "grad"):
        out[key] = np.array(out[key])
        out[key][gone] = np.nan
    return out, still


# ---------------------------------------------------------------------------------------------------------- tests
def test_bits_of_the_unconstrained_normal(env):
    """sum_weight = 0, the start strictly inside the box (the scene's own fractions, all > 0.01; T moved by up to 1 K), a random
    damping: wherever rtx_srf_pixel_cube_normal's own step stays inside the box, normal_box's cost, grad, hess and step are its
    bits and nothing is active. Cost, grad and hess are its bits for every pixel.
    MEASURED on an MI355X: 254 of the 257 pixels qualify (not the two on the ends of the range and one whose step leaves the box)."""
    t, sc, _, _, lam, _ = GF.first_case(env)
    T_lo, T_hi = t["T_range"]
    meas = BX.add_noise(GF.forward(env, t, sc))
    st = dict(kidx=sc["kidx"], frac=sc["frac"], T=np.clip(sc["T"] + np.random.default_rng(7).uniform(-1.0, 1.0, FT.NPIX), T_lo, T_hi))
    want = GF.normal(env, t, st, meas, lam=lam)
    got = normal_box(env, t, st, meas, lam=lam)
    u = np.concatenate([st["T"][:, None], st["frac"].astype(np.float64)], axis=1)
    x = u + want["step"]
    q = (st["T"] > T_lo) & (st["T"] < T_hi) & np.all(st["frac"] > 0, axis=1) & (x[:, 0] >= T_lo) & (x[:, 0] <= T_hi) & np.all(x[:, 1:] >= 0.0, axis=1)
    print("srf cube normal_box, bits of normal: %d of %d pixels strictly inside with the step inside" % (q.sum(), q.size))
    assert q.sum() >= 0.9 * q.size
    for k in ("cost", "grad", "hess"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["step"][q], want["step"][q]) and np.all(got["active"][q] == 0)


@pytest.mark.parametrize("tname", list(CC.T_CONFIGS))
@pytest.mark.parametrize("sname", list(FT.SCENES))
@pytest.mark.parametrize("knots", CC.KNOTS)
def test_normal_box_against_oracle(env, knots, sname, tname):
    """cost, grad and hess with sum_weight = 1e-2 against the fp64 oracle with the pseudo-band, at a start away from the truth
    (negative fractions among it): |got - want| <= k 2^-24 scale with the unconstrained test's k and the pseudo-band's summands
    in the scale.
    MEASURED on an MI355X, worst of the 12 cases, in units of 2^-24 scale: cost 0.11 (k = 19 .. 31), grad 0.56 (k = 17 .. 26),
    hess 2.9 (k = 15 / 21)."""
    t, sc, meas = noisy_case(env, knots, sname, tname)
    st = GF.away(sc, t["T_range"])
    Q, nMix = t["Q"], sc["kidx"].shape[1]
    got = normal_box(env, t, st, meas, delta=1e-2)
    o = BX.evaluate(t["N_h"], t["C_h"], t["G_h"], t["nodes"], st["kidx"], st["frac"], st["T"], meas, delta=1e-2)
    what = "srf cube normal_box %s %s %s" % (knots, sname, tname)
    within(got["cost"], o["cost"], o["scale"]["cost"], GF.K_COST(Q, nMix), what + " cost")
    within(got["grad"], o["grad"], o["scale"]["grad"], GF.K_GRAD(Q, nMix), what + " grad")
    within(got["hess"], o["hess"], o["scale"]["hess"], GF.K_H(Q), what + " hess")
    plain = normal_box(env, t, st, meas, delta=0.0, outs=("cost", "hess"))
    assert np.all(got["hess"][:, FT.tri(1, 1)] > plain["hess"][:, FT.tri(1, 1)]) and np.array_equal(got["hess"][:, 0], plain["hess"][:, 0])


@pytest.mark.parametrize("case", (FIRST, MIX4), ids=("mix3", "mix4"))
def test_properties_of_the_box_step(env, case):
    """At a start with fractions at 0 and temperatures on the ends (rough_start), sum_weight 1e-2, a random damping:
    on the reported active set step_i is exactly 0, lo_i - u_i or hi_i - u_i; step 1's set is in it; the free unknowns' system
    (A_FF d_F = -(g_F + H_FB s_B), A = H + lambda diag H of the device's own outputs) is solved to the unconstrained test's
    componentwise Cholesky residual bound; and wherever fewer than 1 + nMix unknowns are active every free u_i + step_i is
    inside the box (the same fp64 sum the kernel tests; an active one lands on its bound by the first property).
    MEASURED on an MI355X (mix3 / mix4): pixels with an active unknown 99 / 118, with an unknown that joined in a pass 41 / 51,
    with T active 6 / 6, with all unknowns active 0 / 0; the free residual at most 0.19 / 0.22 of the bound."""
    t, sc, meas = noisy_case(env, *case)
    st = rough_start(sc, t["T_range"])
    nU = sc["kidx"].shape[1] + 1
    lam = np.random.default_rng(31).uniform(0.0, 0.5, FT.NPIX)
    got = normal_box(env, t, st, meas, lam=lam, delta=1e-2)
    assert np.all(np.isfinite(got["step"])) and np.all(got["active"] >= 0) and np.all(got["active"] < 2 ** nU)
    B = BX.unbits(got["active"], nU)
    u = np.concatenate([st["T"][:, None], st["frac"].astype(np.float64)], axis=1)
    lo, hi = BX.bounds(nU, t["T_range"])
    d = got["step"]
    with np.errstate(invalid="ignore"):
        on = (d == 0.0) | (d == lo - u) | (d == hi - u)
    assert np.all(on[B])
    B1 = BX.kkt_set(got["grad"], st["T"], st["frac"], t["T_range"])
    assert np.all(B[B1])
    A = FT.unpack(got["hess"])
    A = A + lam[:, None, None] * A * np.eye(nU)[None]
    eps = 2.0 ** -53
    sd = np.sqrt(np.einsum("pii->pi", A))
    res = np.abs(np.einsum("pij,pj->pi", A, d) + got["grad"])
    lim = (3 * nU + 1) * eps * sd * np.sum(np.where(B, 0.0, sd * np.abs(d)), axis=1, keepdims=True)
    own = (nU + 1) * eps * (np.einsum("pij,pj->pi", np.abs(A), np.abs(d)) + np.abs(got["grad"]))
    free = ~B
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(free & (lim > 0.0), res / lim, 0.0)
    few = B.sum(axis=1) < nU
    x = u + d
    print("srf cube box step %s: active pixels %d, joined in a pass %d, T active %d, all active %d; free residual / bound = %.3g"
          % (case[1], B.any(axis=1).sum(), (B & ~B1).any(axis=1).sum(), B[:, 0].sum(), (~few).sum(), ratio.max()))
    assert np.all(res[free] <= (2.0 * lim + own)[free])
    assert np.all((x >= lo)[free & few[:, None]]) and np.all((x <= hi)[free & few[:, None]])
    assert (B & ~B1).any() and B[:, 0].any() and B[:, 1:].any()  # the passes, the T bound and the fraction bounds were all at work
    want, ok, Bw = BX.box_step(got["hess"], got["grad"], lam, st["T"], st["frac"], t["T_range"])
    agree = np.all(Bw == B, axis=1)
    assert ok.all() and agree.mean() >= 0.95  # the fp64 restatement on the device's own sums: the same sets but for ties in the last bit
    assert np.allclose(d[agree], want[agree], rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("k", (1, 3, 8))
def test_fit_box_equals_a_host_loop_over_normal_box(env, k):
    """fit_box(START_GIVEN, max_iter = k, sum_weight = 1e-2) equals, bit for bit, k host-driven trials built from
    rtx_srf_pixel_cube_normal_box with rule 3 and the new stop in NumPy fp64: T, frac, cost, hess, grad, active, n_iter and
    status. The start has negative fractions (projected first), fractions at 0 and temperatures on the ends; a pixel whose
    fractions all start at 0 with T free has H_00 = 0 and is given up as singular (status 3, NaN results) by both; pixels 0, 1
    and 9 start on the point a long fit (200 trials) ends on; an ftol of 0.3 stops pixels early. (The new stop has a test of
    its own below.)"""
    t, sc, meas = noisy_case(env, *FIRST)
    lambda0, ftol, delta = 1e-3, 0.3, 1e-2
    st = rough_start(sc, t["T_range"])
    T0, f0 = np.array(st["T"]), np.array(st["frac"])
    neg = np.random.default_rng(3).random(f0.shape) < 0.1
    f0[neg] = -0.05
    conv = fit_box(env, t, sc["kidx"], meas, max_iter=200, delta=delta)
    for i in (0, 1, 9):
        T0[i], f0[i] = conv["T"][i], conv["frac"][i]
    got = fit_box(env, t, sc["kidx"], meas, start=(T0, f0), max_iter=k, lambda0=lambda0, ftol=ftol, delta=delta)
    want, still = host_loop(env, t, sc["kidx"], meas, (T0, f0), k, lambda0, ftol, delta)
    print("srf cube fit_box vs host loop k=%d: trials %s, statuses %s, stopped by a trial point equal to the current one %d, pixels 0, 1, 9: n_iter %s status %s"
          % (k, np.bincount(got["n_iter"]).tolist(), np.bincount(got["status"]).tolist(), still, got["n_iter"][[0, 1, 9]].tolist(),
             got["status"][[0, 1, 9]].tolist()))
    assert got["n_iter"].max() == k and (got["status"] == 1).any() and np.all(got["frac"][got["status"] <= 1] >= 0.0)
    assert np.all(np.isnan(got["frac"][got["status"] >= 2])) and np.all(got["status"] != 2)
    for key, v in want.items():
        assert np.array_equal(got[key], v, equal_nan=True), key


def test_the_stop_at_a_trial_point_that_does_not_move(env):
    """From the point a long fit ends on, with lambda0 = 1e11: the damped step is then some 1e-11 of the undamped one, too small
    to move a float32 fraction or the fp64 temperature of most pixels, so their trial point is the current point: status 0,
    n_iter 0, T and frac returned bit for bit -- and the whole call still equals the host loop over normal_box bit for bit.
    MEASURED on an MI355X: all 257 pixels stop this way. (In the host-loop test above, at lambda0 = 1e-3, none does.)"""
    t, sc, meas = noisy_case(env, *FIRST)
    conv = fit_box(env, t, sc["kidx"], meas, max_iter=200, delta=1e-2)
    assert np.all(conv["status"] <= 1)
    start = (conv["T"], conv["frac"])
    got = fit_box(env, t, sc["kidx"], meas, start=start, max_iter=2, lambda0=1e11, delta=1e-2)
    want, still = host_loop(env, t, sc["kidx"], meas, start, 2, 1e11, 0.0, 1e-2)
    stopped = (got["status"] == 0) & (got["n_iter"] == 0)
    print("srf cube fit_box, the stop at a trial point that does not move: %d of %d pixels (the host loop: %d)" % (stopped.sum(), stopped.size, still))
    assert still > 0 and stopped.sum() == still
    assert np.array_equal(got["T"][stopped], conv["T"][stopped]) and np.array_equal(got["frac"][stopped], conv["frac"][stopped])
    for key, v in want.items():
        assert np.array_equal(got[key], v, equal_nan=True), key


RECOVERY = [(kn, sn, tn, 0.0) for kn in CC.KNOTS for sn in FT.SCENES for tn in CC.T_CONFIGS] + [FIRST + (1e-2,), MIX4 + (1e-2,)]


@pytest.mark.parametrize("knots,sname,tname,delta", RECOVERY)
def test_recovery_from_the_scan(env, knots, sname, tname, delta):
    """The scan start, 40 trials, on the noisy scene: statuses <= 1; no fraction negative, T inside the range; the cost never
    above the start's (the scan alone, max_iter = 0); the active set holds only unknowns on a bound with the gradient pointing
    out; and the fp64 cost at the device's result exceeds the brute-force optimum (BX.brute on the device's own tables) by at
    most 2 sum_b w_b |r_b| e_b, e_b = FT.FWD_TOL x the band's largest radiance: the first-order change of the cost that the
    forward's own asserted error allows. Zero patterns are not compared.
    MEASURED on an MI355X, worst of the 14 cases: excess / bound 0.0068 (relative excess of the cost 1.0e-4; the fp32-simulated
    restatement on the CPU: 0.011); 0 to 13 pixels per scene end with T on an end, 57 to 105 with a fraction at 0; 3 to 40 trials."""
    t, sc, meas = noisy_case(env, knots, sname, tname)
    args = (t["N_h"], t["C_h"], t["G_h"], t["nodes"])
    T_lo, T_hi = t["T_range"]
    got = fit_box(env, t, sc["kidx"], meas, delta=delta)
    start = fit_box(env, t, sc["kidx"], meas, max_iter=0, delta=delta)
    best = BX.brute(*args, t["T_range"], sc["kidx"], meas, delta=delta)
    c64 = BX.cost_at(*args, sc["kidx"], got["frac"], got["T"], meas, delta=delta)
    slack = BX.cost_slack(*args, sc["kidx"], got["frac"], got["T"], meas)
    excess = c64 - best["cost"]
    print("srf cube fit_box recovery %s %s %s delta=%g: worst excess / bound = %.3g, worst relative excess %.3g, T on an end %d, a fraction at 0 %d, "
          "trials %d .. %d, statuses %r" % (knots, sname, tname, delta, (excess / slack).max(), (excess / best["cost"]).max(),
                                            ((got["T"] == T_lo) | (got["T"] == T_hi)).sum(), (got["frac"] == 0).any(axis=1).sum(),
                                            got["n_iter"].min(), got["n_iter"].max(), np.unique(got["status"]).tolist()))
    assert np.all(got["status"] <= 1) and np.all(got["n_iter"] <= FT.TRIALS) and np.all(np.isfinite(got["hess"])) and np.all(np.isfinite(got["grad"]))
    assert np.all(got["frac"] >= 0.0) and np.all(got["T"] >= T_lo) and np.all(got["T"] <= T_hi)
    assert np.all(start["status"] == 1) and np.all(start["n_iter"] == 0) and np.all(start["frac"] >= 0.0) and np.all(got["cost"] <= start["cost"])
    B = BX.unbits(got["active"], sc["kidx"].shape[1] + 1)
    assert np.array_equal(B, BX.kkt_set(got["grad"], got["T"], got["frac"], t["T_range"]))
    g = got["grad"]
    assert np.all(g[:, 1:][B[:, 1:]] > 0.0) and np.all(got["frac"][B[:, 1:]] == 0.0)
    assert np.all(np.where(got["T"] == T_lo, g[:, 0] > 0.0, g[:, 0] < 0.0)[B[:, 0]])
    assert np.all(excess <= slack)


def test_purity_and_placement(env):
    """The same bits run to run and for a pixel alone or inside the scene (the first n = 1, 64, 65 pixels of the 257), normal_box
    and fit_box (from the scan, 12 trials, sum_weight 1e-2): with the table slice in LDS (8 endmembers x 8 nodes), in global
    memory (the same 8 endmembers followed by 9 unused ones, 17 x 8 > 128: the LDS case's bits; and mix4_of_31 with 8 nodes),
    and with more than one block of bands (80)."""
    for case, times in ((FIRST, 1), (MIX4, 1), (FIRST, 4)):
        t, sc, meas = noisy_case(env, *case, times=times)
        assert (t["tab"].shape[0] * t["Q"] <= 128) == (case is FIRST) and t["tab"].shape[2] == 20 * times
        st = rough_start(sc, t["T_range"])
        lam = np.random.default_rng(29).uniform(0.0, 0.5, FT.NPIX)
        whole = normal_box(env, t, st, meas, lam=lam, delta=1e-2)
        fit_whole = fit_box(env, t, sc["kidx"], meas, max_iter=12, delta=1e-2)
        GF.same(normal_box(env, t, st, meas, lam=lam, delta=1e-2), whole)
        GF.same(fit_box(env, t, sc["kidx"], meas, max_iter=12, delta=1e-2), fit_whole)
        for n in (1, 64, 65):
            m = np.ascontiguousarray(meas[:, :n])
            GF.same(normal_box(env, t, GF.cut(st, slice(0, n)), m, lam=lam[:n], delta=1e-2), {k: v[:n] for k, v in whole.items()})
            GF.same(fit_box(env, t, sc["kidx"][:n], m, max_iter=12, delta=1e-2), {k: v[:n] for k, v in fit_whole.items()})
        alone = normal_box(env, t, st, meas, lam=lam, delta=1e-2, outs=("step",), active=False)
        GF.same(alone, whole, keys=alone)
        if case is FIRST and times == 1:
            t17 = GF.device_tables(env, FIRST[0], 17, FIRST[2])
            assert np.array_equal(t17["G_h"][:, :, :8], t["G_h"]) and t17["tab"].shape[0] * t17["Q"] > 128
            GF.same(normal_box(env, t17, st, meas, lam=lam, delta=1e-2), whole)
            GF.same(fit_box(env, t17, sc["kidx"], meas, max_iter=12, delta=1e-2), fit_whole)


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
    n_iter, status, active = (torch.full((nPix,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = np.array([310.0, 290.0, 285.0, 315.0])
    Tp = lambda T: np.ascontiguousarray(T, dtype=np.float64).ctypes.data_as(C.c_void_p)
    MM, IM = lib.rtx_srf_pixel_cube_fit_box_max_mix(), lib.rtx_srf_pixel_cube_fit_max_iter()

    def nrm(nB_=nB, Q_=Q, T=good, nPix_=nPix, nMix_=nMix, meas_=meas, cost_=cost, flags=0, sw=1e-2):
        return lib.rtx_srf_pixel_cube_normal_box(nB_, Q_, Tp(T), _ptr(N), _ptr(Cb), _ptr(tab), nEnd, nPix_, nMix_, _ptr(kidx), _ptr(frac), _ptr(Tpix),
                                                 _ptr(meas_), None, None, _ptr(cost_), _ptr(grad), _ptr(hess), _ptr(step), st, flags, sw, _ptr(active))

    def ft(nB_=nB, Q_=Q, T=good, nPix_=nPix, nMix_=nMix, meas_=meas, cost_=cost, max_iter=5, lambda0=1e-3, ftol=0.0, flags=GIVEN, sw=1e-2):
        return lib.rtx_srf_pixel_cube_fit_box(nB_, Q_, Tp(T), _ptr(N), _ptr(Cb), _ptr(tab), nEnd, nPix_, nMix_, _ptr(kidx), _ptr(meas_), None,
                                              _ptr(frac), _ptr(Tpix), max_iter, lambda0, ftol, _ptr(cost_), _ptr(n_iter), _ptr(status), _ptr(hess),
                                              st, flags, sw, _ptr(grad), _ptr(active))

    shared = (dict(Q_=0), dict(nB_=-1), dict(nPix_=-1), dict(nMix_=0), dict(nMix_=MM + 1), dict(meas_=None), dict(cost_=None),
              dict(T=[310.0, np.nan, 285.0, 315.0]), dict(T=[300.0, 300.0, 285.0, 315.0]), dict(T=[310.0, 290.0, 291.0, 315.0]),
              dict(sw=-1e-3), dict(sw=float("nan")), dict(sw=float("inf")))
    for kw in shared + (dict(flags=1),):
        assert nrm(**kw) != 0 and lib.rtx_last_error(), kw
    for kw in shared + (dict(flags=2), dict(max_iter=-1), dict(max_iter=IM + 1), dict(lambda0=-1.0), dict(lambda0=float("nan")), dict(ftol=float("inf"))):
        assert ft(**kw) != 0 and lib.rtx_last_error(), kw
    assert nrm(nPix_=0) == 0 and nrm(nB_=0) == 0 and ft(nPix_=0) == 0 and ft(nB_=0) == 0
    torch.cuda.synchronize()
    for v in (cost, grad, hess, step):
        assert bool((v == 7.0).all())
    for v in (n_iter, status, active):
        assert bool((v == -7).all())
    assert bool((frac == 0.4).all()) and bool((Tpix == 300.0).all())
    assert nrm() == 0
    torch.cuda.synchronize()
    for v in (cost, grad, hess):
        assert bool(torch.isfinite(v).all()) and bool((v != 7.0).all())
    assert bool((step != 7.0).all()) and bool((active >= 0).all())
    active.fill_(-7)
    assert ft() == 0
    torch.cuda.synchronize()
    assert bool((n_iter >= 0).all()) and bool((n_iter <= 5).all()) and bool((status >= 0).all()) and bool((status <= 3).all())
    assert bool((active >= 0).all()) and bool((grad != 7.0).all())


def test_python_entries(env):
    """nonneg=False is the unconstrained entries' bits and keys; nonneg=True is the raw box entries on hsi_cube_srf's own tables,
    bit for bit, plus "active" (both) and "grad" (the fit)."""
    sensor = env["sensor"]
    t, sc, meas = noisy_case(env, *FIRST)
    st = rough_start(sc, t["T_range"])
    lam = np.random.default_rng(29).uniform(0.0, 0.5, FT.NPIX)
    c = t["case"]
    s = sensor.Sensor.from_tables(c["tables"])
    grid = env["engine"].Grid(*FC.grid_tuple(env["CH"]))
    base = (grid, dev(env, c["tau"]), dev(env, c["La"]), dev(env, c["Ld"]), c["Xk"], dev(env, t["End"]), dev(env, sc["kidx"]))
    num = lambda r: {("T" if k == "Tpix" else k): v.cpu().numpy() for k, v in r.items()}
    kw = dict(damping=dev(env, lam), n_nodes=t["Q"], T_range=t["T_range"])
    out = sensor.hsi_cube_srf_normal(*base, dev(env, st["frac"]), dev(env, st["T"]), s, dev(env, meas), nonneg=False, **kw)
    assert set(out) == set(GF.OUTS)
    GF.same(num(out), GF.normal(env, t, st, meas, lam=lam))
    out = sensor.hsi_cube_srf_normal(*base, dev(env, st["frac"]), dev(env, st["T"]), s, dev(env, meas), nonneg=True, sum_weight=1e-2, **kw)
    assert set(out) == set(GF.OUTS) | {"active"}
    GF.same(num(out), normal_box(env, t, st, meas, lam=lam, delta=1e-2))
    r = sensor.hsi_cube_srf_fit(*base, dev(env, meas), s, t["T_range"], max_iter=12, n_nodes=t["Q"], nonneg=False, sum_weight=0.0)
    assert set(r) == {"Tpix", "frac", "cost", "n_iter", "status", "hess"}
    GF.same(num(r), GF.fit(env, t, sc["kidx"], meas, max_iter=12))
    r = sensor.hsi_cube_srf_fit(*base, dev(env, meas), s, t["T_range"], max_iter=12, n_nodes=t["Q"], nonneg=True, sum_weight=1e-2)
    assert set(r) == {"Tpix", "frac", "cost", "n_iter", "status", "hess", "grad", "active"}
    GF.same(num(r), fit_box(env, t, sc["kidx"], meas, max_iter=12, delta=1e-2))
    r = sensor.hsi_cube_srf_fit(*base, dev(env, meas), s, t["T_range"], frac0=dev(env, st["frac"]), T0=dev(env, st["T"]), weights=np.ones(20),
                                max_iter=6, lambda0=1e-2, ftol=1e-3, n_nodes=t["Q"], nonneg=True)
    GF.same(num(r), fit_box(env, t, sc["kidx"], meas, w=np.ones(20), start=(st["T"], st["frac"]), max_iter=6, lambda0=1e-2, ftol=1e-3))


def test_compute_hsi_cube_fit_nonneg_end_to_end():
    """rt.compute_hsi_cube_fit(nonneg=True) on the unconstrained end-to-end test's scene (a thinned standard atmosphere, 2 cm^-1,
    eight triangular bands and one off the axis, 65 pixels of 2 out of 8 endmembers), here with an absent endmember in half the
    pixels and noise on the cube: no negative fraction, T in range, statuses <= 1, and the fp64 cost at the result within the
    recovery test's bound of the brute-force optimum on the device's own tables.
    MEASURED on an MI355X: excess / bound 0.0013, 12 of the 65 pixels with a fraction at 0, at most 26 trials, every status 0."""
    import torch
    assert torch.cuda.is_available()
    from radtxfr_amd import _lib, engine, sensor, synthetic
    from radtxfr_amd import radiative_transfer as rt
    lo, hi, dv = 1000.0, 1002.0, 0.0005
    sub = synthetic.subset_table(synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0), lo - 12.0, hi + 12.0)
    sa = rt.StdAtmos
    a = dict(Zs=sa[:, 1], Ts=sa[:, 5].copy(), Ps=sa[:, 4], PLs=sa[:, 3], MFs_VAL=sa[:, 6:9] * 1e6 * GF.E2E_THIN, MFs_ID=np.array([1, 2, 3]))
    kw = dict(DVOUT=dv, line_table=sub, Altitudes=np.array([8.0]), **a)
    s = sensor.Sensor.from_shape(list(np.linspace(1000.15, 1001.85, 8)) + [1004.5], 0.2, "triangle")  # the last one off the axis: a dead band
    Xk = np.array([999.9, 1000.4, 1000.9, 1001.4, 1002.1])
    nB, nk, nEnd, Q, T_range, nPix = 9, 5, 8, 8, (230.0, 350.0), 65
    End = CC.endmembers(nk, nEnd)
    sc = BX.noisy_scene(nPix, 2, nEnd, T_range)
    X, tau, La, Ld = rt.compute_TUD(lo, hi, **kw)
    grid = engine.Grid(lo, hi, X.size)
    d32 = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float32).ravel(), device="cuda")
    dv_ = lambda v: torch.as_tensor(np.array(v), device="cuda")
    t_d, a_d, d_d = d32(tau), d32(La), d32(Ld)
    cube = sensor.hsi_cube_srf(grid, t_d, a_d, d_d, Xk, dv_(End), dv_(sc["kidx"]), dv_(sc["frac"]), dv_(sc["T"]), s, n_nodes=Q, T_range=T_range)[1]
    meas = BX.add_noise(cube.cpu().numpy())
    assert np.isnan(meas[8]).all() and np.isfinite(meas[:8]).all()
    X_out, r = rt.compute_hsi_cube_fit(lo, hi, s, Xk, End, sc["kidx"], meas, T_range, max_iter=FT.TRIALS, n_nodes=Q, nonneg=True, **kw)
    assert np.array_equal(X_out, s.centres) and set(r) == {"Tpix", "frac", "cost", "n_iter", "status", "hess", "grad", "active"}
    assert r["grad"].shape == (nPix, 3) and r["active"].shape == (nPix,) and r["active"].dtype == np.int32
    assert np.all(r["status"] <= 1) and np.all(r["frac"] >= 0.0) and np.all(r["Tpix"] >= T_range[0]) and np.all(r["Tpix"] <= T_range[1])
    lib = _lib.load()
    nodes = sensor.srf_cube_nodes(T_range[0], T_range[1], Q)
    N, Cb, M, jr = sensor.srf_moments(grid, t_d, a_d, d_d, dv_(Xk), nodes, s)
    tab = torch.empty((nEnd, Q, nB), dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(lib.rtx_srf_cube_tables(p(M), p(jr), nB, Q, nk, p(dv_(End)), nEnd, p(tab), None))
    torch.cuda.synchronize()
    args = (N.cpu().numpy().astype(np.float64), Cb.cpu().numpy().astype(np.float64), tab.cpu().numpy().astype(np.float64).transpose(1, 2, 0), nodes)
    best = BX.brute(*args, T_range, sc["kidx"], meas)
    c64 = BX.cost_at(*args, sc["kidx"], r["frac"], r["Tpix"], meas)
    slack = BX.cost_slack(*args, sc["kidx"], r["frac"], r["Tpix"], meas)
    print("compute_hsi_cube_fit nonneg end to end: worst excess / bound = %.3g, a fraction at 0 in %d of %d pixels, trials up to %d, statuses %r"
          % (((c64 - best["cost"]) / slack).max(), (r["frac"] == 0).any(axis=1).sum(), nPix, r["n_iter"].max(), np.unique(r["status"]).tolist()))
    assert np.all(c64 - best["cost"] <= slack)
