"""Host side of the mixed-prologue suite (tests/test_gpu_mix_paths.py): the cases of tests/mix_cases.py are well-formed and
reach what they name (cpu_ref.line_params on the case's inputs), their definition is finite and positive somewhere in every
layer, every deliberate defect of mix_cases.MUTATIONS moves the definition of every case it applies to by at least
100 x the GPU test's bound (the condition that lets the GPU suite fail), the metric's floor covers no point the cases
are about, and engine.broadening_fractions gives the TUD route's mix."""
from collections import OrderedDict

import numpy as np
import pytest

import mix_cases as MC
import sdvoigt_cases as SC
from linesum_metric import TOL, on_floor, pointwise_err

SENSITIVITY = 100.0
REF_ERR_Y0 = 8.0e-11  # of w(0): the reference's Weideman-24 against exp(-x^2) at y = 0 (test_reference_error_on_y0_lines)
X_CORE = 3.39  # < sqrt(ln(1 / linesum_metric.F)) = 3.393: test_floor_share

_DEF = {}


def _definition(name):
    if name not in _DEF:
        _DEF[name] = MC.definition(MC.CASES[name])
        _DEF[name].setflags(write=False)
    return _DEF[name]


_SDREF = {}


def _sd_reference():
    if "r" not in _SDREF:
        _SDREF["r"] = MC.sd_reference(MC.CASES["m_sdvoigt"])
    return _SDREF["r"]


@pytest.mark.parametrize("name", list(MC.CASES))
def test_case_is_well_formed_and_reaches_its_name(name):
    c = MC.CASES[name]
    tbl = c["tbl"]
    n = tbl["nu"].size
    sp = MC.species_of(tbl)
    nS, nL = len(sp), c["T"].size
    assert 12 <= n <= 40 and all(np.asarray(v).shape == (n,) for v in tbl.values())
    assert (nS, nL <= 4) == (3, True) or name == "m_device_tables" and (nS, nL) == (7, 40)
    assert len({m for m, _ in sp}) >= 2  # two Doppler factors
    X = MC.case_axis(c)
    assert X.size <= 2100 or (name == "m_shard" and c["shard"][1] <= 2100)
    assert isinstance(c["diluent"], OrderedDict) and all(v.shape == (nS, nL) for v in c["diluent"].values())
    assert c["profile"] in (0, 1, 3) and ("grid" in c) != ("X" in c)
    if "grid" in c:  # the x.xxx25 centres: none on a grid point (the lines m_shard places by their window edge too)
        step = (c["grid"][1] - c["grid"][0]) / (c["grid"][2] - 1)
        u = (tbl["nu"] - c["grid"][0]) / step
        assert np.all(np.abs(u - np.rint(u) - 0.25) < 1e-6), name
    R = MC.reach(c)
    print("mix reach %s: %s" % (name, {k: v for k, v in R.items() if v}))
    missing = [e for e in c["expect"] if R.get(e, 0) <= 0]
    assert not missing, (name, missing)
    if name in ("m_sets_order", "m_frac_strides", "m_device_tables"):  # every fraction of the block distinct
        f = MC.frac_block(c)
        f = f[f != 0.0]
        assert np.unique(f).size == f.size


@pytest.mark.parametrize("name", list(MC.CASES))
def test_definition_finite_and_positive_in_every_layer(name):
    want = _definition(name)
    c = MC.CASES[name]
    assert want.shape == (c["T"].size, MC.case_axis(c).size)
    assert np.all(np.isfinite(want)) and np.all(want.max(axis=1) > 0.0), name
    assert np.all(np.any(want == 0.0, axis=1)), name  # structural zeros in every layer


def test_lorentz_drop_gives_exact_zeros():
    """m_lorentz: species 1 stands alone right of index 1500; in layer 2 its Gamma0 is 0, the reference's window is empty and
    the definition is exactly 0 there, while the other layers are not."""
    want = _definition("m_lorentz")
    assert np.all(want[2, 1500:] == 0.0) and np.all(want[:2, 1600:1900].max(axis=1) > 0.0) and want[2, :1400].max() > 0.0


def test_shard_lines_skip_and_reach_in():
    """m_shard: the definition on the shard's axis is the same slice of the full-grid one wherever both exist; the lines
    placed by their window edge put non-zero values on the shard's first points only in their widest layer."""
    c = MC.CASES["m_shard"]
    off, n = c["shard"]
    full = _definition("m_shard")
    part = MC.definition(c, g=c["grid"][:3] + (off, n))
    assert np.array_equal(part, full[:, off:off + n])


def test_reference_error_on_y0_lines():
    """m_none against the Doppler profile in closed form (the Voigt profile at y = 0), line by line in the reference's
    windows: the definition -- the reference's Weideman-24 -- is off it by REF_ERR_Y0 = 8.0e-11 of the line's peak (the figure
    tests/test_linesum_axis_host.py finds for hum1_wei itself), and from |x| ~ 4.8 outwards that error is larger than the
    profile: there the definition's value says nothing about the line. The GPU test asserts a non-zero result only above
    4 x REF_ERR_Y0 of the local peak."""
    c = MC.CASES["m_none"]
    X = MC.case_axis(c)
    want = _definition("m_none")
    worst, noise = 0.0, 0
    for k in range(c["T"].size):
        P = MC.layer_params(c, k)
        true, peak = np.zeros(X.size), np.zeros(X.size)
        for nu, S, gd in zip(P["nu"], P["S"], P["GammaD"]):
            lo, hi = np.searchsorted(X, nu - c["hw"] * gd, side="right"), np.searchsorted(X, nu + c["hw"] * gd, side="right")
            a = S * np.sqrt(np.log(2.0) / np.pi) / gd
            true[lo:hi] += a * np.exp(-np.log(2.0) * ((X[lo:hi] - nu) / gd) ** 2)
            peak[lo:hi] = np.maximum(peak[lo:hi], a)
        inw = peak > 0
        assert np.array_equal(inw, want[k] != 0.0) or np.all(want[k][~inw] == 0.0)
        err = np.abs(want[k][inw] - true[inw]) / peak[inw]
        worst = max(worst, float(err.max()))
        noise += int(np.sum(np.abs(want[k][inw] - true[inw]) > true[inw]))
    print("mix reference error on y = 0 lines: %.3g of the peak; %d in-window points where it exceeds the profile" % (worst, noise))
    assert 0.5 * REF_ERR_Y0 < worst <= 1.06 * REF_ERR_Y0 and noise > 0


def _applies(case, m):
    tbl, dil = MC._mutate(case, m)
    same_tbl = set(tbl) == set(case["tbl"]) and all(np.array_equal(tbl[k], case["tbl"][k]) for k in tbl)
    same_dil = all(np.array_equal(dil[k], case["diluent"][k]) for k in dil)
    return not (same_tbl and same_dil)


_CAUGHT = {}


@pytest.mark.parametrize("name", list(MC.CASES))
def test_every_defect_that_applies_moves_the_definition(name):
    """pointwise_err(definition(case, mutate=m), definition(case)) >= 100 TOL for every m that changes the definition at all
    (m_sdvoigt: sdvoigt_cases.judge's ratio >= 100). A defect is not applicable where it leaves the inputs, or every value
    of the definition, as they were (no zero fraction, no deltap column, one layer, a Gamma2 defect on a Voigt case ...)."""
    c = MC.CASES[name]
    want = _definition(name)
    for m in MC.MUTATIONS:
        if not _applies(c, m):
            print("mix sensitivity %-16s %-32s n/a (inputs unchanged)" % (name, m))
            continue
        got = MC.definition(c, mutate=m)
        if np.array_equal(got, want):
            print("mix sensitivity %-16s %-32s n/a (definition unchanged)" % (name, m))
            continue
        if c["profile"] == 3:
            ref = _sd_reference()
            r = max(SC.judge(got[k], ref, k)[1] for k in range(c["T"].size))
            bound = SENSITIVITY
        else:
            r = pointwise_err(got, want)
            bound = SENSITIVITY * TOL
        print("mix sensitivity %-16s %-32s %.3g (needs %.3g)" % (name, m, r, bound))
        assert r >= bound, (name, m, r)
        _CAUGHT.setdefault(m, []).append(name)


def test_every_defect_is_caught_by_some_case():
    if len(_CAUGHT) < len(MC.MUTATIONS):  # run alone: fill it
        for name in MC.CASES:
            test_every_defect_that_applies_moves_the_definition(name)
    assert sorted(_CAUGHT) == sorted(MC.MUTATIONS), sorted(set(MC.MUTATIONS) - set(_CAUGHT))


@pytest.mark.parametrize("name", [n for n, c in MC.CASES.items() if c["profile"] != 3])
def test_floor_share(name):
    """tests/test_linesum_axis_host.py's cap: no in-window point on the metric's floor in a layer whose lines all have
    y >= 0.1, and none within |x| < 3 of its nearest line elsewhere. m_none and m_zero_layer hold y = 0 lines, whose wings
    fall under the floor by design: there every point within |x| < X_CORE of EVERY line is off the floor. X_CORE = 3.39 is
    the most a y = 0 line can meet: its profile is exp(-x^2) of its own peak, the floor is F = 1e-5 of the largest value
    within 1024 points -- at least that peak -- and exp(-x^2) > 1e-5 only for |x| < sqrt(ln 1e5) = 3.393 (at |x| = 4 it is
    1.1e-7)."""
    c = MC.CASES[name]
    want = _definition(name)
    fl = on_floor(want)
    X = MC.case_axis(c)
    for k in range(c["T"].size):
        P = MC.layer_params(c, k)
        cte = np.sqrt(np.log(2.0)) / P["GammaD"]
        y = P["Gamma0"] * cte
        live = np.ones(y.size, bool) if c["profile"] != 1 else P["Gamma0"] > 0.0
        sg0 = P["nu"] + P["Shift0"]
        n_in = int(np.sum(want[k] != 0))
        share = float(fl[k].sum()) / max(n_in, 1)
        print("mix floor_share %s layer %d (y %.3g ... %.3g): %.4f of %d points" % (name, k, y.min(), y.max(), share, n_in))
        xabs = np.abs((X[None, :] - sg0[live, None]) * cte[live, None])
        if name in ("m_none", "m_zero_layer"):
            for l in range(xabs.shape[0]):
                core = (xabs[l] < X_CORE) & (want[k] != 0)
                assert core.any() and not np.any(fl[k] & core), (name, k, l)
        elif y[live].min() >= 0.1:
            assert share == 0.0, (name, k, share)
        else:
            core = (xabs.min(axis=0) < 3.0) & (want[k] != 0)
            assert core.any() and not np.any(fl[k] & core), (name, k)


def test_sdvoigt_dropped_points_within_the_cap():
    """The points judge() drops for predicate flips between the two precisions: tests/test_sdvoigt_paths_host.py's caps (at
    most 2 per line, at most 1e-3 of the (line, point) pairs); the float64 definition meets the metric it is judged by."""
    c = MC.CASES["m_sdvoigt"]
    ref = _sd_reference()
    n_pts = sum(ref["pairs"])
    assert n_pts > 0 and max(ref["skip_per_line"]) <= 2
    assert sum(int(s.sum()) for s in ref["skip"]) <= 1e-3 * n_pts
    want = _definition("m_sdvoigt")
    for k in range(c["T"].size):
        e_den, e_allow, _, zeros = SC.judge(want[k], ref, k)
        assert zeros and e_allow <= 1.0, (k, e_den, e_allow)


# ---- engine.broadening_fractions for ("self", "h2o", "co2") -----------------------------------------------------------
TUD_SPECIES = [(1, 1), (2, 1), (3, 1)]


def tud_mixing_ratios():
    """Four layers, H2O, CO2 (and O3) between 5 and 30 % in every one: (MF_VAL [4][3] in ppmv, MF_ID)."""
    return np.array([[0.30, 0.06, 0.07], [0.12, 0.22, 0.06], [0.07, 0.30, 0.08], [0.06, 0.09, 0.07]]) * 1e6, np.array([1, 2, 3])


def test_broadening_fractions_self_h2o_co2():
    """A line of a listed gas gets 0 from its own column (its self set carries that), air is the remainder, and no fraction
    is below 0.05 apart from those zeros: an error in any of them shows in every layer."""
    from radtxfr_amd import engine
    MF, ID = tud_mixing_ratios()
    dil = engine.broadening_fractions(TUD_SPECIES, MF, ID, ("h2o", "co2"))
    assert list(dil) == ["air", "self", "h2o", "co2"]
    x = MF.T * 1e-6  # [gas][layer]
    for v in dil.values():
        assert np.asarray(v).shape == (3, 4)
    assert np.array_equal(dil["h2o"][0], np.zeros(4)) and np.array_equal(dil["co2"][1], np.zeros(4))
    assert np.allclose(dil["h2o"][1], x[0], rtol=1e-15) and np.allclose(dil["h2o"][2], x[0], rtol=1e-15)
    assert np.allclose(dil["co2"][0], x[1], rtol=1e-15) and np.allclose(dil["co2"][2], x[1], rtol=1e-15)
    assert np.allclose(dil["self"], x, rtol=1e-15)
    assert np.allclose(dil["air"] + dil["self"] + dil["h2o"] + dil["co2"], 1.0, rtol=0, atol=1e-15)
    own = {("h2o", 0), ("co2", 1)}
    small = [(nm, s, k) for nm, v in dil.items() for s in range(3) for k in range(4) if v[s, k] < 0.05 and (nm, s) not in own]
    assert not small, small
