#!/usr/bin/env python3
"""Host-only figures behind DESIGN 4.7's notes on tests/test_gpu_sdvoigt_paths.py (no GPU; needs mpmath):
1. PART4's far wing against 50-digit arithmetic on two cases of tests/sdvoigt_cases.py: the kernel's closed form
   f(t1) - f(t2) = (t1 - t2)(1/2 - t1 t2) / ((1/2 + t1^2)(1/2 + t2^2)) restated in float64 with Z1 = sqrt(X + Y) - csqrtY
   and with Z1 = X / (sqrt(X + Y) + csqrtY), the long-double oracle and the float64 oracle (relative errors).
2. The sign of PROFILE_SDVOIGT (long double) for SD = 0.7 ... 10 between 1e-4 and 10 atm.
3. Where PART2 can meet csqrtY < 8 (zone a's `sY >= 8`).
    python tools/sdvoigt_reference_error.py"""
import os, sys
import numpy as np
import mpmath as mp
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from oracle import cpu_ref as ref
import sdvoigt_cases as SC

mp.mp.dps = 50


def closed_form(nu, GD, G0, G2, sg, stable):
    cte = np.sqrt(np.log(2.0)) / GD
    X = ((G0 - 1.5 * G2) + 1j * (nu - sg)) * (1.0 / G2)
    sY = 1.0 / (2 * cte * G2)
    S = np.sqrt(X + sY * sY)
    t1 = X / (S + sY) if stable else S - sY
    t2 = t1 + 2 * sY
    return (((0.5 - t1 * t2) * (-2 * sY)) / ((t1 * t1 + 0.5) * (t2 * t2 + 0.5)) * cte).real / np.pi


def exact(nu, GD, G0, G2, s):
    cte = mp.sqrt(mp.log(2)) / mp.mpf(GD)
    X = mp.mpc(mp.mpf(G0) - mp.mpf(1.5) * mp.mpf(G2), mp.mpf(nu) - mp.mpf(s)) / mp.mpf(G2)
    sY = 1 / (2 * cte * mp.mpf(G2))
    Z1 = mp.sqrt(X + sY * sY) - sY
    f = lambda t: t / (mp.mpf(0.5) + t * t) / mp.sqrt(mp.pi)
    return (mp.sqrt(mp.pi) * cte * (f(Z1) - f(Z1 + 2 * sY)) / mp.pi).real


print("1. PART4 far wing (both arguments on hum1_wei's one-term asymptote), worst relative error at 64 sampled points against"
      " 50 digits")
for name, p in (("pf_p3_far", 0.068), ("zn_part2_boundary", 0.01)):
    c = SC.CASES[name]
    X = SC.axis(c["grid"])
    P = ref.line_params(c["tbl"], 296.0, p)
    a = (c["tbl"]["nu"][0], P["GammaD"][0], P["Gamma0"][0], c["tbl"]["SD_air"][0] * p * c["tbl"]["gamma_air"][0])
    ld, code = ref.PROFILE_SDVOIGT(*a, 0.0, 0.0, X, dtype=np.longdouble, branches=True)
    f64 = ref.PROFILE_SDVOIGT(*a, 0.0, 0.0, X)
    far = np.nonzero(code == ref.SD_P4)[0]
    idx = far[:: max(1, far.size // 64)]
    m = [exact(*a, X[i]) for i in idx]
    rel = lambda v: max(abs(float((mp.mpf(float(v[i])) + mp.mpf(float(v[i] - type(v[i])(float(v[i])))) - t) / t)) for i, t in zip(idx, m))
    print("   %-18s closed form, Z1 = sqrt(X+Y) - csqrtY %.1e; Z1 = X / (sqrt(X+Y) + csqrtY) %.1e; long-double oracle %.1e; "
          "float64 oracle %.1e; |X| / Y = %.1e ... %.1e" % (name, rel(closed_form(*a, X, False)), rel(closed_form(*a, X, True)), rel(ld),
                                                         rel(f64), *[abs(complex(a[2] - 1.5 * a[3], a[0] - x) / a[3]) * (2 * np.sqrt(np.log(2.0)) / a[1] * a[3]) ** 2
                                                                     for x in (X[far[0]], X[far[-1]])]))

print("2. sign of the profile, nu = 1000 cm^-1, GammaD = 1.45e-3, Gamma0 = 0.07 p, +-5 cm^-1 in 40001 points (long double)")
sg = np.linspace(995.0, 1005.0, 40001)
for sd in (0.7, 1.0, 1.5, 3.0, 10.0):
    neg = [int((ref.PROFILE_SDVOIGT(1000.0, 1.45e-3, 0.07 * p, sd * 0.07 * p, 0.0, 0.0, sg, dtype=np.longdouble) < 0).sum())
           for p in (1e-4, 1e-3, 1e-2, 0.1, 1.0, 10.0)]
    print("   SD = %-4g negative points at 1e-4, 1e-3, 1e-2, 0.1, 1, 10 atm: %s" % (sd, neg))

print("3. PART2 (|X| <= 3e-8 Y somewhere) needs 3e-8 csqrtY^2 Gamma2 > Gamma0 - 1.5 Gamma2 > 0; with csqrtY < 8 that is\n"
      "   (1 - 1.5 SD) / SD < 1.92e-6, i.e. 2/3 - SD < %.1e, and PART2 then reaches sqrt(t2^2 - a^2) <= t2 = 3e-8 csqrtY^2 Gamma2\n"
      "   from the centre: for cte = 574 and csqrtY = 7.5 (Gamma2 = 1.2e-4 cm^-1) %.1e cm^-1" % (1.92e-6 * (2 / 3) ** 2, 3e-8 * 7.5 ** 2 / (2 * 574 * 7.5)))
