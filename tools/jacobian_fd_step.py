"""Error of rt.compute_TUD_jacobian's temperature rows against the fp64 fixed-window central difference at +-0.01 K, for
fd_step_T = 0.25, 0.5 and 1 K. 66-layer standard atmosphere (H2O, CO2, O3), seeded 100 k synthetic table,
1000-1004 cm^-1 at 0.0005, the caller's nine altitudes, layers 0, 17 and 65.

    python tools/jacobian_fd_step.py [--out FILE]
"""
import argparse
import bisect
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import rel_err  # noqa: E402
from oracle import cpu_ref as ref  # noqa: E402
from radtxfr_amd import _lib, synthetic  # noqa: E402
from radtxfr_amd import radiative_transfer as rt  # noqa: E402

LO, HI, DV = 1000.0, 1004.0, 0.0005
ALTS = np.concatenate((np.array([200, 500, 1000, 2000, 5000, 10000, 20000, 50000]) * 0.3048 / 1e3, [100.0]))


def od_fixed_window(tbl, X, T, T_win, P_pa, PL_km, MF_VAL, MF_ID):
    """cpu_ref.layer_od with the windows of every line from T_win (rtx_line_prep_window's definition)."""
    p = float(P_pa) / 101325.0
    glist = X.tolist()
    od = np.zeros(X.size)
    M = np.asarray(tbl["molec_id"]).astype(int)
    for m, ppmv in zip(np.asarray(MF_ID).tolist(), np.asarray(MF_VAL).tolist()):
        keep = M == m
        if not keep.any():
            continue
        sub = {k: np.asarray(v)[keep] for k, v in tbl.items()}
        P, Pw = ref.line_params(sub, T, p), ref.line_params(sub, T_win, p)
        nu = np.asarray(sub["nu"], dtype=np.float64)
        xs = np.zeros(X.size)
        for r in range(nu.size):
            W = max(0.0, 50.0 * Pw["Gamma0"][r], 50.0 * Pw["GammaD"][r])
            lo, hi = bisect.bisect(glist, nu[r] - W), bisect.bisect(glist, nu[r] + W)
            if hi > lo:
                xs[lo:hi] += ref.volumeConcentration(p, T) * P["S"][r] * ref.PROFILE_VOIGT(nu[r] + P["Shift0"][r], P["GammaD"][r],
                                                                                        P["Gamma0"][r], X[lo:hi])[0]
        od += xs * (ppmv * 1e-6) * PL_km * 1e5
    return od


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.load()
    full = synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)
    sub = synthetic.subset_table(full, LO - 12.0, HI + 12.0)
    sa = rt.StdAtmos
    a = dict(Zs=sa[:, 1], Ts=sa[:, 5].copy(), Ps=sa[:, 4], PLs=sa[:, 3], MFs_VAL=sa[:, 6:9] * 1e6, MFs_ID=np.array([1, 2, 3]))
    X = ref.make_spectral_axis(LO, HI, DV)
    OD = np.stack([ref.layer_od(sub, X, a["Ts"][l], a["Ps"][l], a["PLs"][l], a["MFs_VAL"][l], a["MFs_ID"])
                   for l in range(66)], axis=1)
    layers = [0, 17, 65]
    out = ["fd_step_T study: max rel_err (floor 1e-3 max) of the T rows against the fp64 fixed-window difference at +-0.01 K",
           "layers %s, 9 altitudes, 1000-1004 cm^-1 @ 0.0005; rows whose reference is below 1e-6 of the base row's maximum or "
           "below 1e-30 (outside float32) skipped"
           % layers]
    for returnOD in (False, True):
        fds = []
        for l in layers:
            rows = []
            for sgn in (1.0, -1.0):
                T = a["Ts"].copy()
                T[l] += sgn * 0.01
                O = OD.copy()
                O[:, l] = od_fixed_window(sub, X, T[l], a["Ts"][l], a["Ps"][l], a["PLs"][l], a["MFs_VAL"][l], a["MFs_ID"])
                t_, u_, d_ = ref.tud_from_od(X, O, T, a["Zs"], Altitudes=ALTS, returnOD=returnOD)
                rows.append(np.concatenate([t_.T, u_.T, d_[None, :]]))
            fds.append((rows[0] - rows[1]) / 0.02)
        t0, u0, d0 = ref.tud_from_od(X, OD, a["Ts"], a["Zs"], Altitudes=ALTS, returnOD=returnOD)
        base = np.concatenate([t0.T, u0.T, d0[None, :]])
        for h in (0.25, 0.5, 1.0):
            _, _, _, _, J = rt.compute_TUD_jacobian(LO, HI, wrt=("T",), layers=layers, fd_step_T=h, DVOUT=DV, line_table=sub,
                                                    Altitudes=ALTS, returnOD=returnOD, **a)
            g = np.concatenate([J["T"][0].transpose(1, 0, 2), J["T"][1].transpose(1, 0, 2), J["T"][2][None]])  # [row][nX][layer]
            errs = {"tau slot": [], "L-up": [], "Ld": []}
            for c in range(len(layers)):
                for r in range(g.shape[0]):
                    kind = "tau slot" if r < 9 else "L-up" if r < 18 else "Ld"
                    mx = np.max(np.abs(fds[c][r]))
                    # skip rows below what the difference resolves, or below float32's range (an opaque path's tau)
                    if mx > 1e-6 * np.max(np.abs(base[r])) and mx > 1e-30:
                        errs[kind].append(rel_err(g[r, :, c], fds[c][r]))
            out.append("returnOD=%-5s h = %.2f K: max rel_err  " % (returnOD, h) + "  ".join(
                "%s %.2e (%d rows)" % (k, max(v) if v else 0.0, len(v)) for k, v in errs.items()))
            print(out[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
