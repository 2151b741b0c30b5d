"""Host side of the explicit-axis line-sum path suite (tests/test_gpu_linesum_axis_paths.py): the cases of
tests/linesum_axis_cases.py reach the paths they name (cpu_ref.axis_census, whose constants and branch expressions are the
kernels'), the census's windows are bisect.bisect_right's and the oracle's supports, the kernel's two-float abscissa is the
fp64 one to an fp32 ulp where the one-FMA form is not, and the metric's floor covers no path a case is named for."""
import bisect
import os
import re

import numpy as np
import pytest

from oracle import cpu_ref

import linesum_axis_cases as AC
from linesum_metric import TOL, on_floor, pointwise_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = dict(AC.CASES, **{"e_" + k: v for k, v in AC.UNIFORM_CASES.items()})


def _records(c, k):
    return cpu_ref.axis_records(c["tbl"], c["X"], float(c["T"][k]), float(c["p"][k]), c["ow"], c["hw"], AC.layer_diluent(c, k),
                                c["profile"], c["lineshift"])


_WANT = {}


def _want(name):
    if name not in _WANT:
        _WANT[name] = AC.oracle(AC.CASES[name])
    return _WANT[name]


def test_axis_kernel_constants_and_branches():
    """What cpu_ref.axis_census restates is what the kernels say: a kernel edit breaks this, not the coverage."""
    src = open(os.path.join(ROOT, "radtxfr_amd", "csrc", "rtx_voigt_axis.hip")).read()
    assert int(re.search(r"#define AX_TILE (\d+)", src).group(1)) == cpu_ref.AX_TILE
    for branch in ("s32 < 15.0f", "fabsf(s32 - 15.0f) < 2e-3f", "q.y >= 6.0f", "fmaf(x, x, q.y * q.y) < 64.0f", "q.y < 1.0f",
                   "fabs(x64) + Q.y < 15.0", "-((Q.sg0 - a.X[i]) * Q.cte)", "row0 + 64 > zlo && row0 < zhi",
                   "i >= zlo && i < zhi", "i >= lo && i < hi", "slot += 4",
                   "(p + ch) + fmaf(d.x, kl, fmaf(d.y, kh, cl + fmaf(d.x, kh, -p)))"):
        assert branch in src, branch
    prep = open(os.path.join(ROOT, "radtxfr_amd", "csrc", "rtx_lines.hip")).read()
    prep = prep[prep.index("void line_prep_axis_kernel(PrepArgs a)"):]
    prep = prep[:prep.index("\n}\n")]
    for stmt in ("axis_bisect<true>(a.X, a.nx, nu - ph.W), hi = axis_bisect<true>(a.X, a.nx, nu + ph.W)",
                 "ic = axis_bisect<true>(a.X, a.nx, nu)", "if (k == 0) a.ic[l] = (int)ic", "(15.0 - r64.y + 0.01) / r64.cte",
                 "axis_bisect<false>(a.X, a.nx, sg0 - wz)", "axis_bisect<true>(a.X, a.nx, sg0 + wz)", "r64.y < 15.0 && hi > lo",
                 "zlo = zlo < lo ? lo : zlo", "zhi = zhi > hi ? hi : zhi", "(ic - lo > hi - ic ? ic - lo : hi - ic) + 1"):
        assert stmt in prep, stmt


@pytest.mark.parametrize("name", sorted(ALL))
def test_case_census(name):
    """Every case reaches the labels it names, no line that reaches a tile lies outside the tile's bracket of centre
    indices, and the bracket would hold them without maxhw's + 1 too (the margin cannot change a result)."""
    c = ALL[name]
    if not c["uniform"]:
        dev = np.max(np.abs(c["X"] - np.linspace(c["X"][0], c["X"][-1], c["X"].size)))
        step = (c["X"][-1] - c["X"][0]) / (c["X"].size - 1)
        assert not (step > 0 and dev <= 1e-9 * step), "Grid.from_axis would take this axis"  # engine.Grid.from_axis's test
    assert c["X"].size <= 6 * 1024 or c["uniform"]
    C = cpu_ref.axis_census(c["tbl"], c["X"], c["T"], c["p"], c["ow"], c["hw"], c["diluent"], c["profile"], c["lineshift"])
    missing = [e for e in c["expect"] if not e.startswith("!") and C[e] <= 0]
    present = [e[1:] for e in c["expect"] if e.startswith("!") and C[e[1:]] > 0]
    print("axis_census %s: %s" % (name, {k: v for k, v in sorted(C.items()) if v}))
    assert not missing and not present, (name, missing, present)
    assert C["outside_bracket_without_margin"] == 0


@pytest.mark.parametrize("name", sorted(ALL))
def test_windows_are_bisect_right_and_the_oracle_support(name):
    """lo / hi / ic of the census are bisect.bisect_right on the axis; for cases a-d every line's window is the support of
    the oracle's single-line result (Doppler: the support lies inside it -- exp(-ln2 (50)^2) underflows to 0)."""
    c = ALL[name]
    glist = c["X"].tolist()
    for k in range(c["T"].size):
        R = _records(c, k)
        lo = np.array([bisect.bisect_right(glist, v) for v in (R["nu"] - R["W"]).tolist()])
        hi = np.array([bisect.bisect_right(glist, v) for v in (R["nu"] + R["W"]).tolist()])
        assert np.array_equal(lo, R["lo_raw"]) and np.array_equal(hi, R["hi_raw"])
        assert np.array_equal(R["ic"], [bisect.bisect_right(glist, v) for v in R["nu"].tolist()])
        assert np.array_equal(R["zlo_raw"], [bisect.bisect_left(glist, v) for v in (R["sg0"] - R["wz"]).tolist()])
        assert np.array_equal(R["zhi_raw"], [bisect.bisect_right(glist, v) for v in (R["sg0"] + R["wz"]).tolist()])
        b = R["has_band"]  # lines without a band (y >= 15, empty window) carry zlo = zhi = 0
        assert np.all((R["zlo"] >= R["lo"])[b] & (R["zhi"] <= R["hi"])[b]) and np.all(R["zlo"] <= R["zhi"])
        assert not np.any(R["zhi"][~b])
        if c["uniform"]:
            continue
        for j, l in enumerate(R["order"]):
            one = {key: np.asarray(v)[l:l + 1] for key, v in c["tbl"].items()}
            v = AC.oracle(c, tbl=one, layers=[k])[0]
            sup = np.zeros(c["X"].size, bool)
            sup[R["lo"][j]:R["hi"][j]] = True
            if c["profile"] == 2:
                assert not np.any((v != 0) & ~sup) and (v != 0).any() == sup.any(), (name, k, j)
            else:
                assert np.array_equal(v != 0, sup), (name, k, j)


def _w_re(x, y):
    return cpu_ref.hum1_wei(np.asarray(x, dtype=np.float64), y)[0]


def test_abscissa_split_holds_an_ulp_and_one_fma_does_not():
    """b_span: the seven-operation abscissa is within 1 ulp(fp32) of the fp64 x at every in-window point of every tile; the
    one-FMA form DESIGN 4.8 rejects, pushed through the fp64 profile, breaks the GPU test's bound on the wide tiles (and
    the split form, pushed through it, stays a decade under it: an ulp of x ~ 3 is 2.4e-7 and |d ln w / dx| <= 2 |x|): the
    case can tell the two apart."""
    c = AC.CASES["b_span"]
    X = c["X"]
    worst_fma = {}
    for k in range(c["T"].size):
        R = _records(c, k)
        got = {f: np.zeros(X.size) for f in ("split", "fma")}
        want = np.zeros(X.size)
        for l in range(R["nu"].size):
            lo, hi = int(R["lo"][l]), int(R["hi"][l])
            assert hi > lo
            for ia in range(lo // 1024 * 1024, hi, 1024):
                i = np.arange(max(lo, ia), min(hi, ia + 1024))
                x64 = -((R["sg0"][l] - X[i]) * R["cte"][l])
                want[i] += _w_re(x64, R["y"][l])
                for form in got:
                    x32 = cpu_ref.axis_abscissa_f32(X, ia, R["sg0"][l], R["cte"][l], form)[i - ia]
                    assert x32.dtype == np.float32
                    if form == "split":
                        ulp = np.spacing(np.abs(x64).astype(np.float32)).astype(np.float64)
                        assert np.all(np.abs(x32.astype(np.float64) - x64) <= ulp), (k, l, ia)
                    got[form][i] += _w_re(x32.astype(np.float64), R["y"][l])
        for t in range(X.size // 1024):
            s = slice(t * 1024, (t + 1) * 1024)
            span = X[s][-1] - X[s][0]
            e_split, e_fma = pointwise_err(got["split"][s], want[s]), pointwise_err(got["fma"][s], want[s])
            print("b_span layer %d tile %d span %.4g cm^-1: split %.3g one-FMA %.3g" % (k, t, span, e_split, e_fma))
            assert e_split <= 0.1 * TOL, (k, t, e_split)
            worst_fma[t] = max(worst_fma.get(t, 0.0), e_fma)
    assert max(worst_fma.values()) > TOL
    assert all(worst_fma[t] > TOL for t in (3, 4)), worst_fma  # the 2000 cm^-1 tiles


def test_weideman24_against_exp_at_y0():
    """What the Doppler cases and the axis-vs-grid bound of a_upper_atmosphere rest on, in fp64 on the CPU: the reference's
    Weideman-24 (the kernel's fp64 band lanes) against Re w(x) = exp(-x^2) at y = 0: at most 8.0e-11 of w(0) over |x| < 15,
    7.2e-11 over 3 <= |x| < 5.5 and 4.1e-11 over 5.5 <= |x| < 10 -- under the metric's floor of 1e-5 of the local peak that is
    8.0e-6, 7.2e-6 and 4.1e-6, below TOL."""
    x = np.linspace(0.0, 15.0, 300001)[:-1]
    d = np.abs(_w_re(x, 0.0) - np.exp(-x * x))
    zone = lambda a, b: float(d[(x >= a) & (x < b)].max())
    print("weideman24 - exp(-x^2) at y = 0: all %.3g, [3, 5.5) %.3g, [5.5, 10) %.3g" % (d.max(), zone(3, 5.5), zone(5.5, 10)))
    assert 7e-11 < d.max() < 8.5e-11 and 6.5e-11 < zone(3, 5.5) < 7.5e-11 and 3.8e-11 < zone(5.5, 10) < 4.3e-11


@pytest.mark.parametrize("name", sorted(AC.CASES))
def test_floor_share(name):
    """Share of in-window points per layer that the metric judges by its floor, not by their own value: 0 in every layer
    whose lines all have y >= 0.1; in Doppler-dominated layers no point within |x| < 3 of its nearest line is on the floor.
    The Doppler profile's values under F32_FLOOR (beyond |x| ~ 9) are compared absolutely by design."""
    c = AC.CASES[name]
    want = _want(name)
    fl = on_floor(want)
    for k in range(c["T"].size):
        R = _records(c, k)
        n_in = int(np.sum(want[k] != 0))
        share = float(fl[k].sum()) / max(n_in, 1)
        print("floor_share %s layer %d (y %.3g ... %.3g): %.4f of %d points" % (name, k, R["y"].min(), R["y"].max(), share, n_in))
        if R["y"].min() >= 0.1:
            assert share == 0.0, (name, k, share)
        else:
            x = np.min(np.abs((c["X"][None, :] - R["sg0"][:, None]) * R["cte"][:, None]), axis=0)
            core = (x < 3.0) & (want[k] != 0)
            assert core.any() and not np.any(fl[k] & core), (name, k)
