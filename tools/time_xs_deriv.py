"""The fused derivative look-up (rtx_xs_od_d) against 1 + S separate rtx_xs_od calls on the same fp32 weights, on the C3
shape of tools/time_xs_lut.py (32 layers, 500-6000 cm^-1 at 0.001 cm^-1; H2O and CO2 on 4 x 4 (T, p) nodes), DESIGN 4.24.

    python tools/time_xs_deriv.py [--reps 20] [--out profiles/xs_deriv_time.txt]

runs the measurement in a child process of its own under `timeout` (a child that faults or hangs ends the run). The table's
rows are synthetic (one random row per molecule, scaled per node): the kernels are bandwidth-bound and read every row the
weights name whatever it holds, so the line-sums that a real table costs to build are left out. Outputs: dOD/dT and the
columns of both species, three blocks of 32 x 5.5 M x 4 B = 704 MB. The two forms alternate in one process, each between two
device events; the separate form is checked to give the fused form's bits."""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T_NODES = np.array([220.0, 245.0, 270.0, 295.0])
P_NODES = np.array([0.25, 0.45, 0.75, 1.05])
XMIN, XMAX, DV, NL = 500.0, 6000.0, 0.001, 32
SPECIES = (1, 2)
LIMIT = 600


def child(reps):
    import torch
    from radtxfr_amd import _lib, afit_xs, engine, synthetic
    from radtxfr_amd import radiative_transfer as rt
    lib = _lib.load()
    say = lambda s: print(s, flush=True)
    say("# device: %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    a = synthetic.c3_atmosphere(NL)
    X = rt.make_spectral_axis(XMIN, XMAX, DV)
    rng = np.random.default_rng(24)
    entries = []
    for m in SPECIES:
        base = 10.0 ** rng.uniform(-24.0, -19.0, X.size)
        xs = np.stack([np.stack([base * (1.0 + 0.1 * i + 0.03 * j) for j in range(P_NODES.size)]) for i in range(T_NODES.size)])
        entries.append(dict(ID=m, T=T_NODES, P_atm=P_NODES, X=X, xs=xs))
    lut = afit_xs.XsLut.from_grids(entries)
    del entries
    n = lut.grid.n_total
    p_atm = a["Ps"] / 101325.0
    rows, w_T, w_K, idx = lut.layer_terms_d(a["Ts"], p_atm, a["PLs"], a["MFs_VAL"], a["MFs_ID"], SPECIES)
    nS = len(SPECIES)
    ld = (n + 3) // 4 * 4
    block = lambda *lead: torch.empty(lead + (ld,), dtype=torch.float32, device="cuda")
    dT, K = block(NL), block(nS, NL)
    dT2, K2 = block(NL), block(nS, NL)
    w_one = []
    for s in range(nS):
        w = np.zeros_like(w_T)
        w[:, idx[s], :] = w_K[s]
        w_one.append(w)
    hp = lambda x: x.ctypes.data_as(C.c_void_p)
    dp = lambda t: C.c_void_p(t.data_ptr())
    st = engine._stream_ptr

    def fused():
        _lib.check(lib.rtx_xs_od_d(lut._handle(), 0, n, NL, hp(rows), hp(w_T), nS, hp(idx), hp(w_K), dp(dT), dp(K), ld, st(), 0))

    def separate():
        _lib.check(lib.rtx_xs_od(lut._handle(), 0, n, NL, hp(rows), hp(w_T), dp(dT2), ld, st()))
        for s in range(nS):
            _lib.check(lib.rtx_xs_od(lut._handle(), 0, n, NL, hp(rows), hp(w_one[s]), dp(K2[s]), ld, st()))
    forms = {"fused (one rtx_xs_od_d)": fused, "separate (%d rtx_xs_od)" % (1 + nS): separate}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts = {k: [] for k in forms}
    for it in range(reps + 3):  # the first three rounds warm up
        for k, fn in forms.items():  # alternating
            torch.cuda.synchronize()
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            if it >= 3:
                ts[k].append(ev[0].elapsed_time(ev[1]))
    same = bool(torch.equal(dT[:, :n], dT2[:, :n]) and torch.equal(K[:, :, :n], K2[:, :, :n]))
    wr = 4.0 * (1 + nS) * NL * n
    say("%d layers x %d points, dOD/dT + %d species columns: %.0f MB written; %d non-zero temperature terms, %d per species column"
        % (NL, n, nS, wr / 1e6, int((w_T != 0).sum()), int((w_K[0] != 0).sum())))
    say("device events around one call sequence, %d each, alternating:" % reps)
    for k, v in ts.items():
        t = float(np.median(v))
        say("  %-28s median %.3f ms (min %.3f, max %.3f) -> %.2f TB/s of written bytes" % (k, t, min(v), max(v), wr / t / 1e9))
    say("the separate calls give the fused call's bits: %s" % same)
    if not same:
        sys.exit(2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args.reps)
        return
    text = ["# python tools/time_xs_deriv.py --reps %d" % args.reps]
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    text.append(r.stdout.rstrip())
    if r.returncode != 0:
        text.append("the measurement ended with status %d" % r.returncode)
    print("\n".join(text), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(text) + "\n")
    sys.exit(0 if r.returncode == 0 else 1)


if __name__ == "__main__":
    main()
