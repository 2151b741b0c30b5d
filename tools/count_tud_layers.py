#!/usr/bin/env python3
"""CPU-side census of the layers tud_g_kernel visits per 64-point wave on the C3 column (rtx_tud.hip: the hidden layers of
an opaque column), and on the same column with every mixing ratio scaled by 1e-1, 1e-2 and 1e-3. Optical depths from the
oracle (cpu_ref.layer_od, rounded to float32 as the kernel reads them; they are linear in the mixing ratios, so one
line-sum serves every scale) on windows spread over the bench grid; the decisions are the kernel's own:

  b      where the downwelling stops looking: every lane has G(S) <= G(0) 2^-min(opaque_y, 120), rounded up to the end of
         its chunk of TUD_STAGE layers (the wave decides between chunks);
  look   only a wave whose downwelling is done within TUD_SKIP_BOTTOM layers looks at the top at all;
  k_res  the highest chunk boundary above which every lane has sum OD |c0| >= opaque_y + TUD_SKIP_MARGIN, looked for over
         at most TUD_SKIP_SCAN layers from the top and only above b + TUD_STAGE;
  tau    the chunks in [b, k_res) are summed, one at a time, until (s0 + s_top) |c0| >= TUD_SKIP_TAU0 in every lane.

Per column: the share of waves that skip, the layers that run the full step (Planck, up_step, tau sum), the layers that are
only summed, the layers the scan reads (twice where the wave resumes there), and for comparison the same census at layer
granularity (b and k_up not rounded to chunks, no scan limit). Pure NumPy; no GPU.

    python tools/count_tud_layers.py [--windows 12] [--points 6400] [--scan 12] [--bottom 4]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import cpu_ref
from radtxfr_amd import synthetic

N, NL, N_ANGLE = 5500000, 32, 30
STAGE, MARGIN, TAU0, OPAQUE_Y = 4, 8.0, 151.0, 26.0  # TUD_STAGE, TUD_SKIP_MARGIN, TUD_SKIP_TAU0, TUD_OPAQUE_Y
BOTTOM = STAGE  # TUD_SKIP_BOTTOM: a wave looks only if its downwelling is done within this many layers
LOG2E = 1.0 / np.log(2.0)


def g_of(S):
    """The angle-summed transmission function of rtx_tud (theta = 0 has weight 0), S clamped at TUDG_SMAX = 48."""
    th = np.linspace(0.0, np.pi / 2.0, N_ANGLE, endpoint=False)[1:]
    w = np.cos(th) * np.sin(th)
    return np.exp(-np.minimum(S, 48.0)[..., None] / np.cos(th)) @ w, w.sum()


def census(OD, B, cnt0, nd, scan_max, bottom=BOTTOM):
    """OD [n][nL] float32, B [n][nL]; n a multiple of 64. Returns per-wave arrays."""
    n = OD.shape[0]
    nw = n // 64
    c0 = LOG2E  # nadir
    y_opq = OPAQUE_Y + 1.0 + np.maximum(np.log2(B.max(1) / B.min(1)), 0.0)
    S = np.cumsum(OD[:, :nd].astype(np.float64), axis=1)
    g, g0 = g_of(S)
    alive = g > (g0 * 2.0 ** -np.minimum(y_opq, 120.0))[:, None]           # after layer k the lane still looks
    wave_alive = alive.reshape(nw, 64, nd).any(1)                            # [nw][nd]
    dead_at = np.where(wave_alive.all(1), nd, np.argmin(wave_alive, axis=1) + 1)  # layers stepped before live goes false
    top = np.cumsum(OD[:, cnt0 - 1::-1].astype(np.float32), axis=1, dtype=np.float32)[:, ::-1]  # top[:, k] = sum_{j >= k}
    opaque_from = (top * np.float32(c0) >= (y_opq + MARGIN)[:, None]).reshape(nw, 64, cnt0).all(1)  # [nw][cnt0]
    bot = np.cumsum(OD[:, :cnt0].astype(np.float32), axis=1, dtype=np.float32)  # bot[:, k] = sum_{j <= k}
    k_top = (cnt0 - 1) // STAGE * STAGE
    out = dict(skip=np.zeros(nw, bool), full=np.full(nw, float(cnt0)), summed=np.zeros(nw), scanned=np.zeros(nw),
               fine=np.full(nw, float(cnt0)), fine_skip=np.zeros(nw, bool))
    for w in range(nw):
        # layer granularity, no scan limit (the design figure)
        b = int(dead_at[w])
        ks = np.nonzero(opaque_from[w])[0]
        if b < nd or nd < cnt0:
            if ks.size and ks[-1] >= b + 2:
                out["fine"][w], out["fine_skip"][w] = b + cnt0 - ks[-1], True
        # the kernel: chunks
        never = wave_alive[w].all() and nd >= cnt0
        k_hi = min(-(-b // STAGE) * STAGE, NL) if not never else NL
        if never or k_hi > bottom or k_hi + STAGE > k_top:
            continue
        k_scan = max(k_top - (scan_max - STAGE), k_hi + STAGE)
        k_res = -1
        for k in range(k_top, k_scan - 1, -STAGE):
            out["scanned"][w] += min(STAGE, cnt0 - k)
            if opaque_from[w, k]:
                k_res = k
                break
        if k_res < 0:
            continue
        lanes = slice(64 * w, 64 * w + 64)
        summed = 0
        for km in range(k_hi, k_res, STAGE):
            s0 = bot[lanes, km - 1] if km > 0 else 0.0
            if np.all((s0 + top[lanes, k_res]) * np.float32(c0) >= TAU0):
                break
            summed += STAGE
        out["skip"][w], out["full"][w], out["summed"][w] = True, k_hi + cnt0 - k_res, summed
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=12)
    ap.add_argument("--points", type=int, default=6400)
    ap.add_argument("--scan", type=int, default=12, help="TUD_SKIP_SCAN")
    ap.add_argument("--bottom", type=int, default=BOTTOM, help="TUD_SKIP_BOTTOM (32: every wave whose downwelling dies looks)")
    args = ap.parse_args()
    assert args.points % 64 == 0 and args.scan % STAGE == 0
    full = synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)
    atm = synthetic.c3_atmosphere(NL)
    cnt0 = nd = int(np.sum(np.asarray(atm["Zs"]) <= 500))
    Xg = np.linspace(500.0, 6000.0, N)
    starts = (np.linspace(0, N - args.points, args.windows).astype(np.int64) // 64) * 64
    ODs, Bs = [], []
    for i0 in starts:
        X = Xg[i0:i0 + args.points]
        sub = synthetic.subset_table(full, X[0] - 12.0, X[-1] + 12.0)
        ODs.append(np.stack([cpu_ref.layer_od(sub, X, atm["Ts"][k], atm["Ps"][k], atm["PLs"][k], atm["MFs_VAL"][k], atm["MFs_ID"])
                             for k in range(NL)], axis=1))
        Bs.append(cpu_ref.planckian(X, np.asarray(atm["Ts"], dtype=np.float64)))
        d = ODs[-1].sum(1)
        print("window %7.1f cm^-1: column depth median %.3g, min %.3g" % (X[0], np.median(d), d.min()), flush=True)
    OD, B = np.concatenate(ODs), np.concatenate(Bs)
    print("%d layers, count %d, n_down %d, TUD_STAGE %d, TUD_SKIP_SCAN %d, %d waves" % (NL, cnt0, nd, STAGE, args.scan, OD.shape[0] // 64))
    for scale in (1.0, 1e-1, 1e-2, 1e-3):
        c = census((OD * scale).astype(np.float32), B, cnt0, nd, args.scan, args.bottom)
        sk = c["skip"]
        print("mixing ratios x %-5g: waves that skip %5.1f %%; per wave: full layers %5.2f, summed only %4.2f, scan reads %4.2f "
              "(waves that scan and fail: %4.1f %%) | skipping waves alone: full %5.2f | layer granularity, no scan limit: "
              "%5.1f %% skip, %5.2f layers" % (
                  scale, 100.0 * sk.mean(), c["full"].mean(), c["summed"].mean(), c["scanned"].mean(),
                  100.0 * ((c["scanned"] > 0) & ~sk).mean(), c["full"][sk].mean() if sk.any() else float("nan"),
                  100.0 * c["fine_skip"].mean(), c["fine"][c["fine_skip"]].mean() if c["fine_skip"].any() else float("nan")))
        # what rtx_compute_tud_opts leaves out of the line-sum (RTX_CTUD_OD_SCRATCH): a wave that skips and loads no middle chunk is
        # done; a line-sum tile is 16 consecutive waves (counted from each window's start, which is a wave but not a tile boundary
        # of the bench grid: the same statistics, not the same tiles)
        done = sk & (c["summed"] == 0)
        if args.points % 1024 == 0:
            t = done.reshape(-1, 16)
            print("    done waves (skip, no middle chunk loaded) %5.1f %%; tiles with every wave done %5.1f %%, with some %5.1f %%"
                  % (100.0 * done.mean(), 100.0 * t.all(1).mean(), 100.0 * (t.any(1) & ~t.all(1)).mean()))
        else:
            print("    done waves (skip, no middle chunk loaded) %5.1f %%" % (100.0 * done.mean()))


if __name__ == "__main__":
    main()
