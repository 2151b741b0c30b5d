"""Generate tests/golden/g16_profiles.npz by RUNNING THE IMPORTED REFERENCE (build container only).

    python tests/make_golden_profiles.py

G16: hapi's line-profile functions (misc/hapi.py:9850-10160: pcqsdhc, PROFILE_HT and its limits, PROFILE_LORENTZ,
PROFILE_DOPPLER) and the complex probability functions under them (hum1_wei :9833, cpf3 :9645). For every case the npz holds
the parameters (JSON), the points `sg_<tag>`, the reference's values `ref_<tag>` taken ONE POINT PER CALL (the reference's
vector call only works when every point of the call lands in the same PART), `truth_<tag>`: the same
formulas evaluated by the code below in np.longdouble / np.clongdouble (with the fp64 Weideman coefficients of
oracle/cpu_ref.weideman_coeffs and the fp64 value of cte, so that it is the same function as the reference), and
`eref_<tag>` = max_i |ref_i - truth_i| / |truth_i| on complex moduli: the reference's own rounding and cancellation error,
from which tests/test_gpu_profiles.py takes its bounds. Read by tests/test_profiles_host.py and tests/test_gpu_profiles.py.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

LD, CLD = np.longdouble, np.clongdouble
PARAMS = ("sg0", "GamD", "Gam0", "Gam2", "Shift0", "Shift2", "anuVC", "eta_re", "eta_im")
N_POINTS = 401
HT_1ATM = dict(sg0=1000.0, GamD=0.0012, Gam0=0.05, Gam2=0.006, Shift0=-0.002, Shift2=0.0005, anuVC=0.01, eta_re=0.2, eta_im=0.0)
# the cases that sit on a regime threshold or beside one and carry the reference's own cancellation
NOT_ORDINARY = ("p2p4_switch", "small_g2_1e-10", "small_g2_1e-08", "p3_near", "p3_far")


def _case(tag, pts, fn="pcqsdhc", **kw):
    p = dict(HT_1ATM)
    p.update(kw)
    return dict(tag=tag, fn=fn, params=p, points=pts, ordinary=tag not in NOT_ORDINARY)


def _two_ranges():
    """Line core and near wing (Weideman inside |x| + y < 15) with the far wing (one-term asymptote): 201 + 200 points."""
    return np.concatenate([np.linspace(999.0, 1001.0, 201), np.linspace(1000.0, 1012.0, 200)])


def wide_points():
    """1000 +- 100 in 1201 points spaced as sinh: 1e-3 apart at the centre, 1.3 at the ends."""
    return 1000.0 + 100.0 * np.sinh(8.0 * np.linspace(-1.0, 1.0, 1201)) / np.sinh(8.0)


def make_cases(rng):
    lin = lambda a, b: np.linspace(a, b, N_POINTS)  # noqa: E731
    midp = dict(Gam0=0.005, Gam2=0.0006, Shift0=-0.0002, Shift2=0.00005, anuVC=0.001, eta_re=0.3)
    p1 = dict(Gam0=0.005, Gam2=0.0, Shift0=-0.0002, Shift2=0.0, anuVC=0.002)
    p2 = dict(Gam0=0.05, Gam2=1e-16, Shift0=-0.002, Shift2=0.0, anuVC=0.01, eta_re=0.2)
    cases = [
        _case("ht_1atm", _two_ranges()),
        # the tail shape: 900 ... 1100 for the integral of the real part (0.99966 by the trapezoid rule), dense at the centre
        _case("ht_1atm_wide", wide_points()),
        _case("ht_cplx", _two_ranges(), eta_im=0.05),
        _case("ht_midp", _two_ranges(), **midp),
        _case("cpf3_shell", lin(999.98, 1000.02), Gam0=0.0005, Gam2=0.00006, Shift0=-0.00002, Shift2=0.000005, anuVC=0.0001),
        _case("rautian", lin(999.98, 1000.02), eta_re=0.0, **p1),
        _case("part1_eta", lin(999.98, 1000.02), eta_re=0.4, **p1),
        _case("p1_4000", lin(1000.0, 1012.0), Gam2=0.0, Shift2=0.0),
        _case("neg_re", lin(999.0, 1001.0), Gam0=0.005, Gam2=0.004, Shift0=-0.0002, Shift2=0.0, anuVC=0.0, eta_re=0.0),
        _case("p2_all", lin(999.9, 1000.1), **p2),
        _case("p2p4_switch", lin(997.0, 1003.0), **dict(p2, Gam2=1e-14)),
        _case("small_g2_1e-10", lin(999.0, 1001.0), **dict(p2, Gam2=1e-10)),
        _case("small_g2_1e-08", lin(999.0, 1001.0), **dict(p2, Gam2=1e-8)),
        _case("small_g2_1e-06", lin(999.0, 1001.0), **dict(p2, Gam2=1e-6)),
        _case("p3_near", lin(999.9, 1000.1), GamD=1e-9),
        # PART3's far form: the reference reads WR1, WI1 of another PART there and raises; truth only
        _case("p3_far", np.array([4990.0, 4999.0, 4999.9, 5000.0, 5000.5, 5003.0, 5010.0]) + 0.0, GamD=1e-12, Gam0=5e-5, Gam2=6e-6,
              Shift0=0.0, Shift2=0.0, anuVC=0.0, eta_re=0.0),
        # the limit profiles on ht_1atm's numbers, each through the reference's own function
        _case("lim_sdrautian", lin(999.0, 1001.0), fn="PROFILE_SDRAUTIAN"),
        _case("lim_rautian", lin(999.0, 1001.0), fn="PROFILE_RAUTIAN"),  # eta = 0.2 is passed and ignored (:10115)
        _case("lim_sdvoigt", lin(999.0, 1001.0), fn="PROFILE_SDVOIGT"),
        _case("lim_voigt", lin(999.0, 1001.0), fn="PROFILE_VOIGT"),
        _case("lim_lorentz", lin(999.0, 1001.0), fn="PROFILE_LORENTZ"),
        _case("lim_doppler", lin(999.99, 1000.01), fn="PROFILE_DOPPLER"),
    ]
    # breadth: log-uniform widths, all in PART4 away from its thresholds. GamD / Gam2 stays within 0.3 ... 30: below that
    # the two arguments of PART4 differ by 2 csqrtY << |Z| and the reference's W1 - W2 loses digits (1e-12 at a ratio of
    # 1e-3), above it sqrt(X + Y) - csqrtY does (the small_g2 cases) -- both belong to the threshold cases, not to E_ord
    for k in range(20):
        sg0 = float(np.round(rng.uniform(600.0, 4000.0), 3))
        GamD = float(10.0 ** rng.uniform(-4.0, -2.0))
        Gam2 = GamD * float(10.0 ** rng.uniform(-1.5, 0.5))
        Gam0 = Gam2 / float(rng.uniform(0.05, 0.2))
        w = 30.0 * max(GamD, Gam0)
        cases.append(_case("rand%02d" % k, lin(sg0 - w, sg0 + 1.5 * w), sg0=sg0, GamD=GamD, Gam0=Gam0, Gam2=Gam2,
                           Shift0=-Gam0 * float(rng.uniform(0.0, 0.1)), Shift2=Gam2 * float(rng.uniform(-0.2, 0.2)),
                           anuVC=Gam0 * float(rng.uniform(0.0, 0.5)), eta_re=float(rng.uniform(0.0, 0.5)),
                           eta_im=float(rng.uniform(-0.1, 0.1)) if k % 3 == 0 else 0.0))
    return cases


def effective_params(case):
    """The pcqsdhc arguments a case's function passes on (misc/hapi.py:10085-10140), as (sg0, GamD, Gam0, Gam2, Shift0,
    Shift2, anuVC, eta)."""
    p = case["params"]
    eta = complex(p["eta_re"], p["eta_im"]) if p["eta_im"] != 0.0 else p["eta_re"]
    full = [p["sg0"], p["GamD"], p["Gam0"], p["Gam2"], p["Shift0"], p["Shift2"], p["anuVC"], eta]
    keep = {"pcqsdhc": "11111111", "PROFILE_HT": "11111111", "PROFILE_SDRAUTIAN": "11111110", "PROFILE_RAUTIAN": "11101010",
            "PROFILE_SDVOIGT": "11111100", "PROFILE_VOIGT": "11100000"}[case["fn"]]
    return [v if k == "1" else 0.0 for v, k in zip(full, keep)]


def reference_args(case, sg):
    """Positional arguments of the reference's function of this case."""
    p = case["params"]
    eta = complex(p["eta_re"], p["eta_im"]) if p["eta_im"] != 0.0 else p["eta_re"]
    a = {"pcqsdhc": (p["sg0"], p["GamD"], p["Gam0"], p["Gam2"], p["Shift0"], p["Shift2"], p["anuVC"], eta),
         "PROFILE_SDRAUTIAN": (p["sg0"], p["GamD"], p["Gam0"], p["Gam2"], p["Shift0"], p["Shift2"], p["anuVC"]),
         "PROFILE_RAUTIAN": (p["sg0"], p["GamD"], p["Gam0"], p["Shift0"], p["anuVC"], eta),
         "PROFILE_SDVOIGT": (p["sg0"], p["GamD"], p["Gam0"], p["Gam2"], p["Shift0"], p["Shift2"]),
         "PROFILE_VOIGT": (p["sg0"], p["GamD"], p["Gam0"]),
         "PROFILE_LORENTZ": (p["sg0"], p["Gam0"]),
         "PROFILE_DOPPLER": (p["sg0"], p["GamD"])}[case["fn"]]
    return a + (sg,)


# ---- the same formulas in extended precision, one point at a time ----------------------------------------------------
_W24 = _L24 = None
RPI, PI, ISP = LD(np.sqrt(np.pi)), LD(np.pi), LD(1 / np.sqrt(np.pi))  # the reference's fp64 constants


def _c(re, im=0.0):
    return CLD(LD(re) + 1j * LD(im))


def hum1_wei_ld(x, y):
    """misc/hapi.py:9833-9844 for one (x, y) in long double; the Weideman coefficients and L are the fp64 values."""
    global _W24, _L24
    if _W24 is None:
        from cpu_ref import weideman_coeffs
        _W24, _L24 = weideman_coeffs(24)
    if abs(x) + y < 15.0:
        z = _c(x, y)
        L = LD(_L24)
        d = L - 1j * z
        Z = (L + 1j * z) / d
        p = _c(0.0)
        for a in _W24:
            p = p * Z + LD(a)
        return 2 * p / d ** 2 + ISP / d
    t = _c(y, -x)
    return ISP * t / (LD(0.5) + t ** 2)


def cpf3_ld(x, y):
    """misc/hapi.py:9645-9670 in long double."""
    zm1 = 1 / _c(x, y)
    zm2 = zm1 ** 2
    zsum = zterm = _c(1.0)
    for k in range(15):
        zterm = zterm * (zm2 * LD(0.5 + k))
        zsum = zsum + zterm
    return zsum * (1j * zm1 * LD(0.564189583547756))


def pcqsdhc_ld(sg0, GamD, Gam0, Gam2, Shift0, Shift2, anuVC, eta, s):
    """misc/hapi.py:9850-10023 for ONE point s, every quantity after cte in long double. PART3's far form takes PART3's own
    W (the reference reads an unbound WR1 there)."""
    cw = lambda Z: hum1_wei_ld(-Z.imag, Z.real)  # noqa: E731
    cte = LD(np.sqrt(np.log(2.0)) / GamD)
    eta = _c(complex(eta).real, complex(eta).imag)
    c0, c2 = _c(Gam0, Shift0), _c(Gam2, Shift2)
    c0t = (1 - eta) * (c0 - LD(1.5) * c2) + LD(anuVC)
    c2t = (1 - eta) * c2
    num = 1j * (LD(sg0) - LD(s)) + c0t
    if abs(c2t) == 0:
        Z1 = num * cte
        W = cw(Z1)
        A = RPI * cte * W
        B = RPI * cte * ((1 - Z1 ** 2) * W + Z1 / RPI) if abs(Z1) <= 4.0e3 else cte * (RPI * W + LD(0.5) / Z1 - LD(0.75) / Z1 ** 3)
    else:
        X = num / c2t
        Y = 1 / (2 * cte * c2t) ** 2
        csqrtY = (LD(Gam2) - 1j * LD(Shift2)) / (2 * cte * (1 - eta) * (LD(Gam2) ** 2 + LD(Shift2) ** 2))
        k = RPI / (2 * csqrtY)
        if abs(X) <= LD(3.0e-8) * abs(Y):
            Z1, Z2 = num * cte, np.sqrt(X + Y) + csqrtY
            W1, W2 = cw(Z1), cw(Z2)
        elif abs(Y) <= LD(1.0e-15) * abs(X):
            Z1 = None
        else:
            Z1 = np.sqrt(X + Y) - csqrtY
            Z2 = Z1 + 2 * csqrtY
            S1, S2 = abs(Z1), abs(Z2)
            f = cpf3_ld if (abs(S1 - S2) <= 1 and max(S1, S2) > 8 and min(S1, S2) <= 8) else hum1_wei_ld
            W1, W2 = f(-Z1.imag, Z1.real), f(-Z2.imag, Z2.real)
        if Z1 is not None:
            A = RPI * cte * (W1 - W2)
            B = (-1 + k * (1 - Z1 ** 2) * W1 - k * (1 - Z2 ** 2) * W2) / c2t
        else:
            sXY, sX = np.sqrt(X + Y), np.sqrt(X)
            W3 = cw(sXY)
            if abs(sX) <= 4.0e3:
                g = 1 / RPI - sX * cw(sX)
                A = (2 * RPI / c2t) * g
                B = (1 / c2t) * (-1 + 2 * RPI * (1 - X - 2 * Y) * g + 2 * RPI * sXY * W3)
            else:
                g = 1 / X - LD(1.5) / X ** 2
                A = (1 / c2t) * g
                B = (1 / c2t) * (-1 + (1 - X - 2 * Y) * g + 2 * RPI * sXY * W3)
    return (1 / PI) * (A / (1 - (LD(anuVC) - eta * (c0 - LD(1.5) * c2)) * A + eta * c2 * B))


def truth_of(case, sg):
    p = case["params"]
    if case["fn"] == "PROFILE_LORENTZ":
        return np.array([LD(p["Gam0"]) / (PI * (LD(p["Gam0"]) ** 2 + (LD(s) - LD(p["sg0"])) ** 2)) for s in sg], dtype=LD)
    if case["fn"] == "PROFILE_DOPPLER":  # hapi's cSqrtLn2divSqrtPi and cLn2 (misc/hapi.py:89-90)
        return np.array([LD(0.469718639319144059835) * np.exp(-LD(0.6931471805599) * ((LD(s) - LD(p["sg0"])) / LD(p["GamD"])) ** 2)
                         / LD(p["GamD"]) for s in sg], dtype=LD)
    a = effective_params(case)
    return np.array([pcqsdhc_ld(*a, s) for s in sg], dtype=CLD)


CPF_XY = None


def cpf_points():
    """(x, y) for hum1_wei (crossing |x| + y = 15, y < 0 included) and for cpf3 (around |z| = 8)."""
    x = np.concatenate([np.linspace(-16.0, 16.0, 33), np.linspace(-16.0, 16.0, 33), np.linspace(-14.0, 18.0, 33), np.linspace(0.0, 6.0, 25),
                        np.linspace(-20.0, 20.0, 21)])
    y = np.concatenate([np.full(33, 0.5), np.full(33, 1e-4), np.linspace(0.0, 14.9, 33), np.linspace(-0.5, -0.01, 25), np.full(21, -2.0)])
    t = np.linspace(0.05, np.pi - 0.05, 60)
    r = np.tile(np.array([7.2, 8.0, 9.5]), 20)
    return x, y, r * np.cos(t), r * np.sin(t)


def main():
    from _refimport import load
    _, hapi, _ = load()
    rng = np.random.default_rng(20261018)
    cases = make_cases(rng)
    out, meta = {}, []
    for c in cases:
        sg = np.asarray(c.pop("points"), dtype=np.float64)
        tag, fn = c["tag"], getattr(hapi, c["fn"])
        truth = truth_of(c, sg)
        real_only = c["fn"] in ("PROFILE_LORENTZ", "PROFILE_DOPPLER")
        ref = None
        if tag != "p3_far":
            vals = [fn(*reference_args(c, np.array([s]))) for s in sg]
            ref = np.array([v[0] for v in vals]) if real_only else np.array([complex(v[0][0], v[1][0]) for v in vals])
            e = float(np.max(np.abs(ref - truth) / np.abs(truth)))
            out["ref_" + tag] = ref
            out["eref_" + tag] = np.array(e)
        c["has_ref"] = ref is not None
        out["sg_" + tag] = sg
        out["truth_" + tag] = truth.astype(np.float64 if real_only else np.complex128)
        meta.append(c)
        print("%-16s %-18s n=%3d ordinary=%d  e_ref=%s" % (tag, c["fn"], sg.size, c["ordinary"],
                                                         "%.2e" % float(out["eref_" + tag]) if ref is not None else "(reference cannot run)"))
    x, y, x3, y3 = cpf_points()
    hw = np.array([complex(*[v[0] for v in hapi.hum1_wei(np.array([a]), np.array([b]))]) for a, b in zip(x, y)])
    hw_t = np.array([hum1_wei_ld(a, b) for a, b in zip(x, y)], dtype=CLD)
    c3 = np.array([complex(*[v[0] for v in hapi.cpf3(np.array([a]), np.array([b]))]) for a, b in zip(x3, y3)])
    c3_t = np.array([cpf3_ld(a, b) for a, b in zip(x3, y3)], dtype=CLD)
    out.update(cpf_x=x, cpf_y=y, cpf_ref=hw, cpf_truth=hw_t.astype(np.complex128), eref_cpf=np.array(float(np.max(np.abs(hw - hw_t) / np.abs(hw_t)))),
               cpf3_x=x3, cpf3_y=y3, cpf3_ref=c3, cpf3_truth=c3_t.astype(np.complex128),
               eref_cpf3=np.array(float(np.max(np.abs(c3 - c3_t) / np.abs(c3_t)))))
    print("hum1_wei e_ref %.2e   cpf3 e_ref %.2e" % (float(out["eref_cpf"]), float(out["eref_cpf3"])))
    print("E_ord = %.2e" % max(float(out["eref_" + c["tag"]]) for c in meta if c["ordinary"]))
    p = os.path.join(HERE, "golden", "g16_profiles.npz")
    np.savez_compressed(p, cases=np.array(json.dumps(meta)), **out)
    print("%-28s %8.1f KB" % (os.path.basename(p), os.path.getsize(p) / 1024))


if __name__ == "__main__":
    main()
