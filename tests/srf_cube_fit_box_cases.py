"""The bound-constrained per-pixel fit to a measured HSI cube (rtx_srf_pixel_cube_normal_box, rtx_srf_pixel_cube_fit_box,
the nonneg / sum_weight keywords of sensor.hsi_cube_srf_normal / hsi_cube_srf_fit and rt.compute_hsi_cube_fit):
the pseudo-band, the fp64 restatement of the box step and of the box fit built on srf_cube_fit_cases.evaluate / solve, the
noisy scenes with absent endmembers, and the brute-force oracle (a dense search in T of non-negative least squares by subset
enumeration) that tests/test_srf_cube_fit_box_host.py (CPU) and tests/test_gpu_srf_cube_fit_box.py (the kernels) share.
NumPy only, fixed seeds. Shapes, scenes, knot sets and temperature configurations are srf_cube_fit_cases'."""
import itertools

import numpy as np

import srf_cube_cases as CC
import srf_cube_fit_cases as FT

NOISE = 1e-3        # sigma_b of the noise, of band b's largest radiance over the scene
DELTAS = (0.0, 1e-2)
GRID, REFINE = 400, 3  # the brute oracle's grid in T and the number of times it is refined around the best point
tri = FT.tri


# ------------------------------------------------------------------------------------------------------ the scenes
def noisy_scene(nPix, nMix, nEnd, T_range, seed=5):
    """FT.distinct_scene; then with probability 1/2 one fraction of a pixel (nMix > 1) is set to 0 and the row renormalised:
    an endmember of kidx that is absent from the pixel. The first two pixels stay on the ends of the range."""
    sc = FT.distinct_scene(nPix, nMix, nEnd, T_range, seed=seed)
    r = np.random.default_rng(seed + 100)
    drop = r.random(nPix) < 0.5
    which = r.integers(0, nMix, nPix)
    f = sc["frac"].astype(np.float64)
    if nMix > 1:
        f[np.flatnonzero(drop), which[drop]] = 0.0
        f = f / f.sum(axis=1, keepdims=True)
    return dict(kidx=sc["kidx"], frac=f.astype(np.float32), T=sc["T"])


def add_noise(cube, noise=NOISE, seed=41):
    """cube [nB][nPix] plus Gaussian noise of sigma_b = noise x band b's largest finite |radiance|, as float32; a band that is
    NaN (dead) stays NaN."""
    c = np.asarray(cube).astype(np.float64)
    with np.errstate(invalid="ignore"):
        top = np.nanmax(np.where(np.isfinite(c), np.abs(c), np.nan), axis=1, initial=0.0)
    top = np.where(np.isfinite(top), top, 0.0)
    g = np.random.default_rng(seed).standard_normal(c.shape)
    return (c + noise * top[:, None] * g).astype(np.float32)


# --------------------------------------------------------------------------------------- one evaluation in the box
def evaluate(N, Cb, G, Tq, kidx, frac, T, meas, w=None, delta=0.0, f32=False):
    """FT.evaluate plus the pseudo-band of weight delta: r_s = sum_m f_m - 1, j_0 = 0, j_m = 1, added to cost, grad, hess and
    to their scales (the absolute values of the same summands, |r_s| taken as sum |f_m| + 1). delta == 0: FT.evaluate."""
    e = FT.evaluate(N, Cb, G, Tq, kidx, frac, T, meas, w, f32=f32)
    if not delta > 0.0:
        return e
    f = np.asarray(frac).astype(np.float64)
    nMix = f.shape[1]
    r, ra = f.sum(axis=1) - 1.0, np.abs(f).sum(axis=1) + 1.0
    e["cost"] = e["cost"] + delta * r * r
    e["scale"]["cost"] = e["scale"]["cost"] + delta * ra * ra
    e["grad"], e["hess"] = e["grad"].copy(), e["hess"].copy()
    e["scale"]["grad"], e["scale"]["hess"] = e["scale"]["grad"].copy(), e["scale"]["hess"].copy()
    for i in range(1, nMix + 1):
        e["grad"][:, i] += delta * r
        e["scale"]["grad"][:, i] += delta * ra
        for j in range(1, i + 1):
            e["hess"][:, tri(i, j)] += delta
            e["scale"]["hess"][:, tri(i, j)] += delta
    return e


def project(f, dtype=np.float32):
    """max(0f, x) of the header: x > 0 ? x : 0, as float32 (dtype: see fit)."""
    f = np.asarray(f, dtype=dtype)
    with np.errstate(invalid="ignore"):
        return np.where(f > 0, f, dtype(0.0)).astype(dtype)


def bounds(nU, T_range):
    lo, hi = np.zeros(nU), np.full(nU, np.inf)
    lo[0], hi[0] = T_range
    return lo, hi


def kkt_set(g, T, f, T_range):
    """Step 1's set, bool [nPix][nU]: the unknowns on a bound whose gradient points out of the box."""
    u = np.concatenate([np.asarray(T, dtype=np.float64)[:, None], np.asarray(f).astype(np.float64)], axis=1)
    lo, hi = bounds(u.shape[1], T_range)
    with np.errstate(invalid="ignore"):
        return ((u <= lo) & (g > 0.0)) | ((u >= hi) & (g < 0.0))


def bits(B):
    """bool [nPix][nU] -> int32 [nPix], bit i = unknown i."""
    return (B.astype(np.int64) << np.arange(B.shape[1])).sum(axis=1).astype(np.int32)


def unbits(a, nU):
    return ((np.asarray(a)[:, None] >> np.arange(nU)) & 1).astype(bool)


def box_step(H, g, lam, T, f, T_range, hold_T=False):
    """The box step of the header, all pixels at once, on FT.solve: returns (d [nPix][nU], ok [nPix], B bool [nPix][nU])."""
    H, g = np.asarray(H, dtype=np.float64), np.asarray(g, dtype=np.float64)
    nPix, nU = g.shape
    u = np.concatenate([np.asarray(T, dtype=np.float64)[:, None], np.asarray(f).astype(np.float64)], axis=1)
    lo, hi = bounds(nU, T_range)
    B = kkt_set(g, T, f, T_range)
    if hold_T:
        B[:, 0] = True
    s = np.zeros((nPix, nU))
    A = FT.unpack(H)
    d, ok = np.zeros((nPix, nU)), np.ones(nPix, dtype=bool)
    for _ in range(nU):
        Hm, gm = H.copy(), np.zeros((nPix, nU))
        for i in range(nU):
            for j in range(i + 1):
                Hm[:, tri(i, j)] = np.where(B[:, i] | B[:, j], 1.0 if i == j else 0.0, H[:, tri(i, j)])
        with np.errstate(invalid="ignore", over="ignore"):
            for j in range(nU):
                r = g[:, j].copy()
                for i in range(nU):
                    if i != j:
                        r = np.where(B[:, i], r + A[:, j, i] * s[:, i], r)
                gm[:, j] = np.where(B[:, j], 0.0, r)
            d, ok = FT.solve(Hm, gm, lam)  # a row of B: pivot 1 + lam, every off-diagonal 0; its d is overwritten
            d = np.where(ok[:, None], np.where(B, s, d), np.nan)
            x = u + d
            jl, jh = ~B & (x < lo), ~B & (x > hi)
        s = np.where(jl, lo - u, np.where(jh, hi - u, s))
        B = B | jl | jh
        if not (jl | jh).any():
            break
    d = np.where(ok[:, None] & B, s, d)
    return d, ok, B


def trial_point(T, f, d, T_range, dtype=np.float32):
    """(T', f') of a box step d from (T, f float32): T clamped into the range, the fractions rounded to float32 once and
    projected (dtype: see fit)."""
    Tt = np.minimum(np.maximum(T + d[:, 0], T_range[0]), T_range[1])
    return Tt, project((np.asarray(f).astype(np.float64) + d[:, 1:]).astype(dtype), dtype)


def fit(N, Cb, G, Tq, T_range, kidx, meas, w=None, start=None, max_iter=FT.TRIALS, lambda0=1e-3, ftol=0.0, delta=0.0, f32=False,
        frac_dtype=np.float32):
    """The fp64 restatement of rtx_srf_pixel_cube_fit_box, all pixels at once: FT.fit with the box step, the projected start,
    the scan's box solve and the stop at a trial point that is the current point. Returns FT.fit's dict plus grad and active
    (step 1's set at the result, int32 bits). frac_dtype=np.float64 keeps the fractions in fp64 between trials instead of
    rounding them to float32 as the entry does: the same iteration without the float32 grid the entry's fractions live on."""
    fd = frac_dtype
    from srf_cube_vjp_cases import admitted
    nPix, nMix = kidx.shape
    nU = nMix + 1
    ev = lambda T, f: evaluate(N, Cb, G, Tq, kidx, f, T, meas, w, delta=delta, f32=f32)
    status = np.full(nPix, -1)
    mid = 0.5 * (T_range[0] + T_range[1])
    if start is not None:
        T, f = np.array(start[0], dtype=np.float64), np.array(start[1], dtype=fd)
        bad = ~(admitted(T, T_range) & np.all(np.isfinite(f), axis=1))
        status[bad] = 2
        T[bad], f[bad] = mid, 0.0
        f = project(f, fd)
        cur = ev(T, f)
    else:
        T, f = np.full(nPix, mid), np.zeros((nPix, nMix), dtype=fd)
        cur = dict(cost=np.full(nPix, np.inf), grad=np.zeros((nPix, nU)), hess=np.zeros((nPix, nU * (nU + 1) // 2)))
        zero = np.zeros((nPix, nMix), dtype=fd)
        for q in range(len(Tq)):
            Tt = np.full(nPix, float(Tq[q]))
            e0 = ev(Tt, zero)
            d, ok, _ = box_step(e0["hess"], e0["grad"], 0.0, Tt, zero, T_range, hold_T=True)
            ft = trial_point(Tt, zero, np.where(ok[:, None], d, 0.0), T_range, fd)[1]
            e1 = ev(Tt, ft)
            with np.errstate(invalid="ignore"):
                better = ok & (e1["cost"] < cur["cost"])  # strictly: the first node wins a tie
            for key in ("cost", "grad", "hess"):
                cur[key] = np.where(better.reshape((-1,) + (1,) * (cur[key].ndim - 1)), e1[key], cur[key])
            T, f = np.where(better, Tt, T), np.where(better[:, None], ft, f)
    cur = {key: np.array(cur[key]) for key in ("cost", "grad", "hess")}
    status[(status < 0) & ~np.isfinite(cur["cost"])] = 3
    cost0 = cur["cost"].copy()
    lam = np.full(nPix, float(lambda0))
    n_iter = np.zeros(nPix, dtype=np.int32)
    while True:
        run = status < 0
        status[run & (cur["cost"] == 0.0)] = 0
        run = status < 0
        status[run & (n_iter >= max_iter)] = 1
        run = status < 0
        if not run.any():
            break
        d, ok, _ = box_step(cur["hess"], cur["grad"], lam, T, f, T_range)
        status[run & ~ok] = 3
        run = status < 0
        Tt, ft = trial_point(T, f, np.where(run[:, None], d, 0.0), T_range, fd)
        status[run & (Tt == T) & np.all(ft == f, axis=1)] = 0  # the trial point is the current point
        run = status < 0
        if not run.any():
            break
        tr = ev(Tt, ft)
        n_iter[run] += 1
        with np.errstate(invalid="ignore"):
            acc = run & (tr["cost"] < cur["cost"])
        rej = run & ~acc
        small = acc & (cur["cost"] - tr["cost"] < ftol * cur["cost"])
        for key in ("cost", "grad", "hess"):
            cur[key] = np.where(acc.reshape((-1,) + (1,) * (cur[key].ndim - 1)), tr[key], cur[key])
        T, f = np.where(acc, Tt, T), np.where(acc[:, None], ft, f)
        lam = np.where(acc, np.maximum(0.1 * lam, FT.LAM_MIN), np.where(rej, np.minimum(10.0 * lam, FT.LAM_MAX), lam))
        status[small] = 0
        status[rej & (lam >= FT.LAM_MAX)] = 0
    dead = status >= 2
    active = np.where(dead, 0, bits(kkt_set(cur["grad"], T, f, T_range))).astype(np.int32)
    T, f = np.where(dead, np.nan, T), np.where(dead[:, None], fd(np.nan), f).astype(fd)
    return dict(T=T, frac=f, cost=np.where(dead, np.nan, cur["cost"]), n_iter=n_iter, status=status.astype(np.int32),
                hess=np.where(dead[:, None], np.nan, cur["hess"]), grad=np.where(dead[:, None], np.nan, cur["grad"]), active=active, cost0=cost0)


# -------------------------------------------------------------------------------------------- the brute-force oracle
def _solve_small(M, v):
    """M x = v for symmetric positive definite M [n][k][k], v [n][k], k <= 4: Cholesky written out over the n systems."""
    k = v.shape[1]
    L = np.zeros_like(M)
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(k):
            p = M[:, j, j] - np.sum(L[:, j, :j] ** 2, axis=1)
            L[:, j, j] = np.sqrt(np.where(p > 0.0, p, np.nan))
            for i in range(j + 1, k):
                L[:, i, j] = (M[:, i, j] - np.sum(L[:, i, :j] * L[:, j, :j], axis=1)) / L[:, j, j]
        z = np.zeros_like(v)
        for i in range(k):
            z[:, i] = (v[:, i] - np.sum(L[:, i, :i] * z[:, :i], axis=1)) / L[:, i, i]
        x = np.zeros_like(v)
        for i in range(k - 1, -1, -1):
            x[:, i] = (z[:, i] - np.sum(L[:, i + 1:, i] * x[:, i + 1:], axis=1)) / L[:, i, i]
    return x


def brute(N, Cb, G, Tq, T_range, kidx, meas, w=None, delta=0.0):
    """The optimum of the constrained problem by search, fp64, with no step of the fit in it: for every pixel a grid of GRID
    temperatures over the range (both ends on it), refined REFINE times around the best one (the new grid spans the two
    neighbours of the best point); at a fixed T the model is linear in f, and the non-negative least-squares optimum is the
    best of the unconstrained optima of all 2^nMix supports that are themselves >= 0. Returns dict(T, frac (float64), cost):
    cost is evaluate()'s at the point found, so it is the cost of a real point of the box and an upper bound of the optimum."""
    N, Cb, G = (np.asarray(v).astype(np.float64) for v in (N, Cb, G))
    nPix, nMix = kidx.shape
    k = np.clip(kidx, 0, G.shape[2] - 1)
    cnt = FT.counting(N, w)
    wv = np.ones(N.size) if w is None else np.asarray(w, dtype=np.float64)
    sw = np.sqrt(wv[cnt])
    Gm = [G[:, cnt][:, :, k[:, m]] for m in range(nMix)]                       # [Q][nb][nPix] each
    rhs = (np.asarray(meas).astype(np.float64)[cnt] - (Cb[cnt] / N[cnt])[:, None]) * sw[:, None]  # [nb][nPix]
    if delta > 0.0:
        rhs = np.concatenate([rhs, np.full((1, nPix), np.sqrt(delta))], axis=0)
    rhs = rhs.T                                                                # [nPix][nb']
    subsets = [s for n in range(1, nMix + 1) for s in itertools.combinations(range(nMix), n)]
    lo, hi = np.full(nPix, float(T_range[0])), np.full(nPix, float(T_range[1]))
    best = dict(cost=np.full(nPix, np.inf), T=np.full(nPix, np.nan), f=np.zeros((nPix, nMix)))
    pix = np.arange(nPix)
    for _ in range(REFINE + 1):
        Tg = lo[None, :] + (hi - lo)[None, :] * np.linspace(0.0, 1.0, GRID)[:, None]  # [GRID][nPix]
        Tg[-1] = hi
        for t0 in range(0, GRID, 100):
            Tc = Tg[t0:t0 + 100]
            nT = Tc.shape[0]
            l = CC.lagrange(Tc.ravel(), Tq).reshape(nT, nPix, -1)
            A = np.stack([np.einsum("tpq,qbp->tpb", l, Gm[m]) * (sw / N[cnt])[None, None, :] for m in range(nMix)], axis=3)
            if delta > 0.0:
                A = np.concatenate([A, np.full((nT, nPix, 1, nMix), np.sqrt(delta))], axis=2)
            A = A.reshape(nT * nPix, -1, nMix)
            b = np.broadcast_to(rhs[None], (nT, nPix, rhs.shape[1])).reshape(nT * nPix, -1)
            AtA, Atb, btb = np.einsum("nbi,nbj->nij", A, A), np.einsum("nbi,nb->ni", A, b), np.einsum("nb,nb->n", b, b)
            cost, f = btb.copy(), np.zeros((nT * nPix, nMix))                  # the empty support
            for s in subsets:
                ix = list(s)
                x = _solve_small(AtA[:, ix][:, :, ix], Atb[:, ix])
                c = btb - 2.0 * np.einsum("ni,ni->n", x, Atb[:, ix]) + np.einsum("ni,nij,nj->n", x, AtA[:, ix][:, :, ix], x)
                with np.errstate(invalid="ignore"):
                    good = np.all(x >= 0.0, axis=1) & (c < cost)
                cost = np.where(good, c, cost)
                full = np.zeros_like(f)
                full[:, ix] = x
                f = np.where(good[:, None], full, f)
            cost, f = cost.reshape(nT, nPix), f.reshape(nT, nPix, nMix)
            it = np.argmin(cost, axis=0)
            c = cost[it, pix]
            better = c < best["cost"]
            best["cost"] = np.where(better, c, best["cost"])
            best["T"] = np.where(better, Tc[it, pix], best["T"])
            best["f"] = np.where(better[:, None], f[it, pix], best["f"])
        h = (hi - lo) / (GRID - 1)
        lo, hi = np.maximum(best["T"] - h, T_range[0]), np.minimum(best["T"] + h, T_range[1])
    e = cost_at(N, Cb, G, Tq, kidx, best["f"], best["T"], meas, w, delta)
    return dict(T=best["T"], frac=best["f"], cost=e)


def cost_at(N, Cb, G, Tq, kidx, frac, T, meas, w=None, delta=0.0):
    """The fp64 cost at (T, frac), frac taken as float64 (FT.evaluate keeps what it is given)."""
    return evaluate(N, Cb, G, Tq, kidx, np.asarray(frac, dtype=np.float64), T, meas, w, delta=delta)["cost"]


def cost_slack(N, Cb, G, Tq, kidx, frac, T, meas, w=None):
    """2 sum_b w_b |r_b| e_b at (T, frac), e_b = FT.FWD_TOL x band b's largest |y| over the scene: the first-order change of the
    cost that an error of the forward's own asserted size in every band allows."""
    e = FT.evaluate(N, Cb, G, Tq, kidx, np.asarray(frac, dtype=np.float64), T, meas, w)
    cnt = FT.counting(N, w)
    wv = np.ones(np.asarray(N).size) if w is None else np.asarray(w, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        r = np.where(cnt[:, None], e["y"] - np.where(cnt[:, None], np.asarray(meas).astype(np.float64), 0.0), 0.0)
    e_b = FT.FWD_TOL * np.max(np.abs(e["y"]), axis=1)
    return 2.0 * np.sum((wv * cnt * e_b)[:, None] * np.abs(r), axis=0)
