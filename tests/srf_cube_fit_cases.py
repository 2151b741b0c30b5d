"""The per-pixel fit of temperature and fractions to a measured HSI cube (rtx_srf_pixel_cube_normal, rtx_srf_pixel_cube_fit,
sensor.hsi_cube_srf_normal / hsi_cube_srf_fit, rt.compute_hsi_cube_fit): the scenes, the fp64 oracle of one
evaluation, the fp64 restatement of the damped step and of the whole fit, and the sensitivity bound that
tests/test_srf_cube_fit_host.py (CPU) and tests/test_gpu_srf_cube_fit.py (the kernels) share. NumPy only, fixed seeds. Grid,
bands and knot sets are those of tests/srf_fused_cases.py, the temperature configurations those of tests/srf_cube_cases.py.

    y_b(u) = (C_b + sum_m f_m t_m) / N_b,  t_m = sum_q l_q(T) G[q][b][k_m],  t'_m = sum_q l'_q(T) G[q][b][k_m],  u = (T, f_1 ..)
    r = y - meas on the bands that count (N_b > 0 and w_b > 0),  J_b0 = sum_m f_m t'_m / N_b,  J_bm = t_m / N_b
    cost = sum w r^2,  grad = J^T W r,  H = J^T W J, the lower triangle by rows (H_00, H_10, H_11, H_20, ..)
"""
import numpy as np

import srf_cube_cases as CC
import srf_cube_vjp_cases as VC

NPIX = CC.NPIX
SCENES = {"mix1_of_8": (1, 8), "mix3_of_8": (3, 8), "mix4_of_31": (4, 31)}  # name -> (nMix, nEnd)
FWD_TOL = 1e-5  # tests/test_gpu_srf_cube.py: the forward's own asserted bound, of the band's largest radiance
TRIALS = 40     # of the recovery tests (the issue: 20 are not enough on the wide range)
LAM_MIN, LAM_MAX = 1e-12, 1e12


def tri(i, j):
    return i * (i + 1) // 2 + j


def distinct_scene(nPix, nMix, nEnd, T_range, seed=5):
    """CC.scene with the rows of kidx drawn WITHOUT replacement (a repeated endmember makes H singular): kidx [nPix][nMix]
    int32, frac [nPix][nMix] float32 as CC.scene draws it, T [nPix] float64 uniform over T_range with the first two pixels on
    its ends."""
    r = np.random.default_rng(seed)
    kidx = np.stack([r.permutation(nEnd)[:nMix] for _ in range(nPix)]).astype(np.int32)
    frac = r.random((nPix, nMix)) + 0.05
    frac = (frac / frac.sum(axis=1, keepdims=True)).astype(np.float32)
    T = r.uniform(T_range[0], T_range[1], nPix)
    T[:2] = np.asarray(T_range, dtype=np.float64)[:min(2, nPix)]
    return dict(kidx=kidx, frac=frac, T=T)


def counting(N, w=None):
    N = np.asarray(N, dtype=np.float64)
    return (N > 0.0) if w is None else (N > 0.0) & (np.asarray(w, dtype=np.float64) > 0.0)


def _r32(x):
    return np.asarray(x).astype(np.float32).astype(np.float64)


def evaluate(N, Cb, G, Tq, kidx, frac, T, meas, w=None, f32=False):
    """The oracle of one evaluation, all pixels at once, fp64. N, Cb [nB]; G [Q][nB][nEnd]; Tq the nodes; kidx, frac
    [nPix][nMix]; T [nPix]; meas [nB][nPix]; w [nB] or None. f32: the kernel's fp32 roundings simulated (the weights, every
    link of the chains, y). Returns a dict: cost [nPix], grad [nPix][nU], hess [nPix][nU (nU + 1) / 2], y and J
    ([nB][nPix], [nU][nB][nPix], zero on the bands that do not count), and under "scale" cost / grad / hess / r of the absolute
    values of the same summands, |r| taken as |y| + |meas| (r [nB][nPix])."""
    N, Cb, G = (np.asarray(v).astype(np.float64) for v in (N, Cb, G))
    Q, nB, nEnd = G.shape
    T = np.asarray(T, dtype=np.float64)
    f = np.asarray(frac).astype(np.float64)
    k = np.clip(kidx, 0, nEnd - 1)
    nPix, nMix = k.shape
    nU = nMix + 1
    cnt = counting(N, w)
    wv = np.where(cnt, 1.0 if w is None else np.asarray(w, dtype=np.float64), 0.0)[:, None]
    Ns = np.where(cnt, N, 1.0)[:, None]
    l, dl = CC.lagrange(T, Tq), VC.dlagrange(T, Tq)
    rnd = _r32 if f32 else (lambda x: x)
    l, dl = rnd(l), rnd(dl)

    def chain(wq, Gm, absolute=False):  # sum_q wq[p][q] Gm[q][b][p], q ascending
        t = np.zeros((nB, nPix))
        for q in range(Q):
            a, b = wq[:, q][None, :], Gm[q]
            t = t + np.abs(a * b) if absolute else rnd(t + a * b)
        return t
    J, Ja = np.zeros((nU, nB, nPix)), np.zeros((nU, nB, nPix))
    s, sa = np.zeros((nB, nPix)), np.zeros((nB, nPix))
    for m in range(nMix):
        Gm = G[:, :, k[:, m]]
        t, tp = chain(l, Gm), chain(dl, Gm)
        ta, tpa = chain(l, Gm, True), chain(dl, Gm, True)
        s, sa = rnd(s + f[:, m][None, :] * t), sa + np.abs(f[:, m])[None, :] * ta
        J[0] += f[:, m][None, :] * tp
        Ja[0] += np.abs(f[:, m])[None, :] * tpa
        J[m + 1], Ja[m + 1] = t, ta
    J, Ja = J / Ns[None], Ja / Ns[None]
    y, ya = rnd((Cb[:, None] + s) / Ns), (np.abs(Cb)[:, None] + sa) / Ns
    cm = np.broadcast_to(cnt[:, None], (nB, nPix))
    with np.errstate(invalid="ignore"):
        ms = np.where(cm, np.asarray(meas).astype(np.float64), 0.0)  # a select: what a band that does not count holds is not used
    y, ya = np.where(cm, y, 0.0), np.where(cm, ya, 0.0)
    J, Ja = np.where(cm[None], J, 0.0), np.where(cm[None], Ja, 0.0)
    r, ra = y - ms, ya + np.abs(ms)
    nH = nU * (nU + 1) // 2
    H, Ha = np.zeros((nPix, nH)), np.zeros((nPix, nH))
    for i in range(nU):
        for j in range(i + 1):
            H[:, tri(i, j)] = np.sum(wv * J[i] * J[j], axis=0)
            Ha[:, tri(i, j)] = np.sum(wv * Ja[i] * Ja[j], axis=0)
    return dict(cost=np.sum(wv * r * r, axis=0), grad=np.sum(wv[None] * J * r[None], axis=1).T, hess=H, y=y, J=J,
                scale=dict(cost=np.sum(wv * ra * ra, axis=0), grad=np.sum(wv[None] * Ja * ra[None], axis=1).T, hess=Ha, r=ra))


def unpack(H, n=None, off=0):
    """[nPix][n][n] symmetric from the packed lower triangle [nPix][nH]; off, n: the block of unknowns off .. off + n - 1."""
    nH = H.shape[1]
    nU = int(round((np.sqrt(8 * nH + 1) - 1) / 2))
    n = nU - off if n is None else n
    A = np.empty((H.shape[0], n, n))
    for i in range(n):
        for j in range(i + 1):
            A[:, i, j] = A[:, j, i] = H[:, tri(i + off, j + off)]
    return A


def solve(H, g, lam, off=0):
    """The damped step of the header, all pixels at once: (A + lam diag A) d = -g for the block of unknowns off .. of the packed
    H, by Cholesky, columns ascending, the inner sums k ascending. Returns (d [nPix][n], ok [nPix]); a pivot that is not
    finite or not positive: ok False and d NaN."""
    g = np.asarray(g, dtype=np.float64)[:, off:]
    A = unpack(np.asarray(H, dtype=np.float64), off=off)
    nPix, n, _ = A.shape
    lam = np.broadcast_to(np.asarray(lam, dtype=np.float64), (nPix,))
    L = np.zeros((nPix, n, n))
    ok = np.ones(nPix, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j in range(n):
            piv = lam * A[:, j, j] + A[:, j, j]
            for k in range(j):
                piv = piv - L[:, j, k] * L[:, j, k]
            ok &= np.isfinite(piv) & (piv > 0.0)
            L[:, j, j] = np.sqrt(np.where(piv > 0.0, piv, np.nan))
            for i in range(j + 1, n):
                v = A[:, i, j].copy()
                for k in range(j):
                    v = v - L[:, i, k] * L[:, j, k]
                L[:, i, j] = v / L[:, j, j]
        z = np.zeros((nPix, n))
        for i in range(n):
            v = -g[:, i]
            for k in range(i):
                v = v - L[:, i, k] * z[:, k]
            z[:, i] = v / L[:, i, i]
        d = np.zeros((nPix, n))
        for i in range(n - 1, -1, -1):
            v = z[:, i].copy()
            for k in range(n - 1, i, -1):
                v = v - L[:, k, i] * d[:, k]
            d[:, i] = v / L[:, i, i]
    d[~ok] = np.nan
    return d, ok


def trial_point(T, f, d, T_range):
    """(T', f') of a step d from (T, f float32): T clamped into the range, the fractions rounded to float32 once."""
    Tt = np.minimum(np.maximum(T + d[:, 0], T_range[0]), T_range[1])
    return Tt, (np.asarray(f).astype(np.float64) + d[:, 1:]).astype(np.float32)


def fit(N, Cb, G, Tq, T_range, kidx, meas, w=None, start=None, max_iter=TRIALS, lambda0=1e-3, ftol=0.0, f32=False):
    """The fp64 restatement of rtx_srf_pixel_cube_fit (include/radtxfr_hip.h has the steps), all pixels at once. start: (T
    [nPix], frac [nPix][nMix] float32) for RTX_FIT_START_GIVEN, None for the node scan. Returns a dict: T, frac (float32), cost,
    n_iter, status, hess, and cost0 = the cost of the start."""
    nPix, nMix = kidx.shape
    nU = nMix + 1
    ev = lambda T, f: evaluate(N, Cb, G, Tq, kidx, f, T, meas, w, f32=f32)
    status = np.full(nPix, -1)
    mid = 0.5 * (T_range[0] + T_range[1])
    if start is not None:
        T, f = np.array(start[0], dtype=np.float64), np.array(start[1], dtype=np.float32)
        bad = ~(VC.admitted(T, T_range) & np.all(np.isfinite(f), axis=1))
        status[bad] = 2
        T[bad], f[bad] = mid, 0.0
        cur = ev(T, f)
    else:
        T, f = np.full(nPix, mid), np.zeros((nPix, nMix), dtype=np.float32)
        cur = dict(cost=np.full(nPix, np.inf), grad=np.zeros((nPix, nU)), hess=np.zeros((nPix, nU * (nU + 1) // 2)))
        for q in range(len(Tq)):
            Tt = np.full(nPix, float(Tq[q]))
            e0 = ev(Tt, np.zeros((nPix, nMix), dtype=np.float32))
            d, ok = solve(e0["hess"], e0["grad"], 0.0, off=1)
            ft = np.where(ok[:, None], d, 0.0).astype(np.float32)
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
        d, ok = solve(cur["hess"], cur["grad"], lam)
        status[run & ~ok] = 3
        run = status < 0
        Tt, ft = trial_point(T, f, np.where(run[:, None], d, 0.0), T_range)
        tr = ev(Tt, ft)
        n_iter[run] += 1
        with np.errstate(invalid="ignore"):
            acc = run & (tr["cost"] < cur["cost"])
        rej = run & ~acc
        small = acc & (cur["cost"] - tr["cost"] < ftol * cur["cost"])
        for key in ("cost", "grad", "hess"):
            cur[key] = np.where(acc.reshape((-1,) + (1,) * (cur[key].ndim - 1)), tr[key], cur[key])
        T, f = np.where(acc, Tt, T), np.where(acc[:, None], ft, f)
        lam = np.where(acc, np.maximum(0.1 * lam, LAM_MIN), np.where(rej, np.minimum(10.0 * lam, LAM_MAX), lam))
        status[small] = 0
        status[rej & (lam >= LAM_MAX)] = 0
    dead = status >= 2
    T, f = np.where(dead, np.nan, T), np.where(dead[:, None], np.float32(np.nan), f).astype(np.float32)
    return dict(T=T, frac=f, cost=np.where(dead, np.nan, cur["cost"]), n_iter=n_iter, status=status.astype(np.int32),
                hess=np.where(dead[:, None], np.nan, cur["hess"]), cost0=cost0)


def sensitivity_bound(N, Cb, G, Tq, sc, w=None):
    """bound [nPix][nU]: sum_b |P_ib| e_b with P = (J^T W J)^-1 J^T W at the truth (fp64) and e_b = FWD_TOL x band b's largest
    |L| over the scene: how far an error of the forward's own asserted size in every band can move the unknowns."""
    nPix = sc["T"].size
    e = evaluate(N, Cb, G, Tq, sc["kidx"], sc["frac"], sc["T"], np.zeros((np.asarray(N).size, nPix)), w)
    cnt = counting(N, w)
    wv = 1.0 if w is None else np.asarray(w, dtype=np.float64)[cnt][None, :, None]
    J = e["J"][:, cnt].transpose(2, 1, 0)  # [nPix][nb][nU]
    e_b = FWD_TOL * np.max(np.abs(e["y"][cnt]), axis=1)
    JW = J * wv
    P = np.linalg.solve(np.einsum("pbi,pbj->pij", JW, J), JW.transpose(0, 2, 1))  # [nPix][nU][nb]
    return np.einsum("pib,b->pi", np.abs(P), e_b)


def jacobi_condition(H):
    """Condition numbers [nPix] of the packed H scaled to unit diagonal."""
    A = unpack(H)
    s = 1.0 / np.sqrt(np.einsum("pii->pi", A))
    return np.linalg.cond(A * s[:, :, None] * s[:, None, :])
