"""GPU: the Hartmann-Tran line-sum (csrc/rtx_ht.hip: rtx_ht_prep + rtx_ht_sum) --
hapi.absorptionCoefficient_HT with VARIABLES["HT_COLUMNS"] on against the reference's row-by-row sums of
tests/golden/g17_ht_sum.npz, the sum against rtx_profile_eval of the same parameters (section 4.14) summed on the host, the
window and block edges, determinism, the SDVoigt limit and the switch.

Measured on an MI355X (profiles/ht_sum_accuracy.txt): golden parity rel_err <= 2.6e-13 and point by point <= 3.1e-13 over
the six cases, exact zeros where the reference has them; against rtx_profile_eval the sums are BIT-IDENTICAL (both states,
the tiny-Gamma2 table at both pressures and the 128 / 129 / 140-candidate blocks); the SDVoigt limit 1.1e-13."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_err
from make_golden_ht_sum import HEAD, N_LINES, SPECIES, case_kwargs, g17_axis, g17_table, ht_column_names
from radtxfr_amd import _lib, engine
from radtxfr_amd import hapi as H

pytestmark = pytest.mark.gpu

G17 = np.load(os.path.join(GOLDEN, "g17_ht_sum.npz"), allow_pickle=False)
CASES = json.loads(str(G17["cases"]))
X_FULL = np.linspace(899.5, 906.5, 2401)
STATES = dict(T=[90.0, 150.0, 296.0, 500.0], p=[0.05, 0.1, 1.0, 0.7])
DIL = {"air": 0.5, "self": 0.3, "H2": 0.2}


@pytest.fixture(scope="module")
def table():
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    _lib.load()
    tbl = g17_table(G17)
    H.storage2cache_from_columns("g17", tbl)
    return tbl


@pytest.fixture(scope="module")
def lines(table):
    t = engine.LineTable(table)
    yield t
    t.close()


@pytest.fixture
def switch_on():
    old = H.VARIABLES["HT_COLUMNS"]
    H.VARIABLES["HT_COLUMNS"] = True
    yield
    H.VARIABLES["HT_COLUMNS"] = old


def ones(t):
    return np.ones((len(t.species), 1))


def host_sum(t, X, prm, k):
    """sum_l strength_l Re PROFILE_HT_l on [lo_l, hi_l): rtx_profile_eval of the prologue's parameters, every line masked to
    its window and added on the host in line order with the kernel's association (acc = acc + WS * Re)."""
    re, _ = engine.profile_eval(engine.LS_PCQSDHC, prm["params"][k].contiguous(), torch.from_numpy(X).cuda(), imag=False)
    re = re.cpu().numpy()
    acc = np.zeros(X.size)
    for l in range(t.n):
        lo, hi = prm["window"][k, l]
        if hi > lo:
            acc[lo:hi] = acc[lo:hi] + prm["strength"][k, l] * re[l, lo:hi]
    return acc


def difference(out, ref):
    """max |out - ref| / ref where the host sum is positive; where it is 0 (no window reaches the point) out must be 0."""
    assert np.all(ref >= 0) and ref.max() > 0 and not out[ref == 0].any()
    pos = ref > 0
    return float(np.max(np.abs(out[pos] - ref[pos]) / ref[pos]))


def regime_ratio(X, prm, k):
    """min and max of |X| / |Y| over the windows of the live lines of state k with c2t != 0, and the number of PART1 lines."""
    lo_r, hi_r, part1 = np.inf, 0.0, 0
    P = prm["params"][k].cpu().numpy()
    for l in range(P.shape[0]):
        lo, hi = prm["window"][k, l]
        if hi <= lo:
            continue
        sg0, GamD, Gam0, Gam2, Shift0, Shift2, anuVC, er, ei, _ = P[l]
        eta, cte = complex(er, ei), np.sqrt(np.log(2.0)) / GamD
        c2t = (1 - eta) * complex(Gam2, Shift2)
        if abs(c2t) == 0:
            part1 += 1
            continue
        c0t = (1 - eta) * (complex(Gam0, Shift0) - 1.5 * complex(Gam2, Shift2)) + anuVC
        r = np.abs((1j * (sg0 - X[lo:hi]) + c0t) / c2t) / abs(1.0 / (2.0 * cte * c2t) ** 2)
        lo_r, hi_r = min(lo_r, float(r.min())), max(hi_r, float(r.max()))
    return lo_r, hi_r, part1


def test_golden_parity_every_case_through_the_drop_in(table, switch_on):
    """1e-9: the metric and bound of test_g11_sdvoigt_golden for this fp64 family, and point by point wherever the reference
    is positive; exactly 0 wherever it is 0. Precondition (from the prologue's own parameters): every line with c2t != 0
    keeps 3e-6 < |X| / |Y| < 1e13 on its window -- a factor 100 inside PART4 -- and the reference's arguments to PROFILE_HT
    are the prologue's (1e-12 of each column's largest entry: libm differences of pow / exp / log only)."""
    worst = []
    for c in CASES:
        X, ref = g17_axis(c), G17["xs_" + c["tag"]]
        kw = case_kwargs(c)
        om, xs = H.absorptionCoefficient_HT(SourceTables="g17", OmegaGrid=X, **kw)
        if c is CASES[0]:  # the alias is the same function
            assert H.absorptionCoefficient is H.absorptionCoefficient_HT
        # the prologue's parameters, through the engine, with the drop-in's weights
        tbl = H._device_table_ht(H._device_table(["g17"], [k.lower() for k in c["Diluent"]]), ["g17"], [k.lower() for k in c["Diluent"]])
        comps = {(int(q[0]), int(q[1])): (q[2] if len(q) > 2 else H.abundance(int(q[0]), int(q[1]))) for q in kw["Components"]}
        factor = 1.0 if c.get("HITRAN_units", True) else H.volumeConcentration(c["p"], c["T"])
        w = np.array([[factor / H.abundance(*mi) * comps[mi] if mi in comps else 0.0] for mi in tbl.species])
        prm = engine.ht_line_params(tbl, X, [c["T"]], [c["p"]], w, c["Diluent"], omega_wing=c.get("OmegaWing", 0.0),
                                    omega_wing_hw=c.get("OmegaWingHW", 50.0), intensity_threshold=c.get("IntensityThreshold", 0.0))
        r_lo, r_hi, part1 = regime_ratio(X, prm, 0)
        par = G17["par_" + c["tag"]]
        live = np.flatnonzero(prm["strength"][0] != 0.0)
        assert np.array_equal(live, par[:, 10].astype(np.int64)), c["tag"]
        P = prm["params"][0].cpu().numpy()[live]
        # (eta as one complex column: with a single diluent its imaginary part is rounding noise of either side's division)
        Pc = np.concatenate([P[:, :7], (P[:, 7] + 1j * P[:, 8])[:, None]], axis=1)
        Rc = np.concatenate([par[:, :7], (par[:, 7] + 1j * par[:, 8])[:, None]], axis=1)
        dpar = float(np.max(np.max(np.abs(Pc - Rc), axis=0) / np.max(np.abs(Rc), axis=0)))
        win = prm["window"][0][live]
        assert np.array_equal(win[:, 1] - win[:, 0], par[:, 9].astype(np.int64)), c["tag"]
        pos = ref > 0
        e_rel = rel_err(xs, ref)
        e_pt = float(np.max(np.abs(xs[pos] - ref[pos]) / ref[pos]))
        n_zero_bad = int(np.sum(xs[~pos] != 0.0))
        print("ht_sum golden %-18s rel_err %.3e  point-by-point %.3e  zeros %d (wrong %d)  params %.2e  |X|/|Y| in [%.3g, %.3g]  PART1 lines %d"
              % (c["tag"], e_rel, e_pt, int(np.sum(~pos)), n_zero_bad, dpar, r_lo, r_hi, part1))
        assert 3e-6 < r_lo and r_hi < 1e13 and part1 > 0, c["tag"]
        assert dpar <= 1e-12, (c["tag"], dpar)
        if not (np.array_equal(om, X) and e_rel <= 1e-9 and e_pt <= 1e-9 and n_zero_bad == 0 and int(np.sum(~pos)) == c["n_zero"]):
            worst.append((c["tag"], e_rel, e_pt, n_zero_bad))
    assert not worst, worst


def test_sum_equals_profile_eval_summed_on_the_host(lines, table):
    """DESIGN section 4.14's check: the same parameters through rtx_profile_eval, masked to the windows and added in line
    order. The terms and their order are the same and every sum is positive: bit-identity is expected, 1e-14 is the bound."""
    T, p = [150.0, 296.0], [0.1, 1.0]
    w = ones(lines)
    prm = engine.ht_line_params(lines, X_FULL, T, p, w, DIL, omega_wing_hw=15.0)
    _, out = engine.ht_sum(lines, X_FULL, T, p, w, DIL, omega_wing_hw=15.0)
    out = out.cpu().numpy()
    for k in range(2):
        ref = host_sum(lines, X_FULL, prm, k)
        d = difference(out[k], ref)
        print("ht_sum vs profile_eval, T = %g K: max relative difference %.3e, bit-identical %s" % (T[k], d, np.array_equal(out[k], ref)))
        assert d <= 1e-14
    # a table whose Gamma2 is tiny (gamma_HT_2 = 1e-9 gamma); the reference loses digits there and is not the yardstick. At
    # 1 atm its lines stay in PART4; at 2e-5 atm with windows of 0.1 cm^-1 every point is in PART2 (|X| <= 3e-8 |Y|)
    tiny = dict(table)
    for sp in SPECIES:
        names = ht_column_names(sp)
        for b in range(4):
            tiny[names[6 * b + 2]] = 1e-9 * np.where(tiny[names[6 * b]] != 0.0, tiny[names[6 * b]], 0.05)
            tiny[names[6 * b + 5]] = np.zeros(N_LINES)
        tiny["SD_" + sp] = np.zeros(N_LINES)
    t2 = engine.LineTable(tiny)
    try:
        for tag, pk, kw in (("1 atm", 1.0, dict(omega_wing_hw=15.0)), ("2e-5 atm", 2e-5, dict(omega_wing=0.1, omega_wing_hw=0.0))):
            prm = engine.ht_line_params(t2, X_FULL, [296.0], [pk], ones(t2), DIL, **kw)
            r_lo, r_hi, part1 = regime_ratio(X_FULL, prm, 0)
            assert part1 == 0
            if pk < 1.0:
                assert r_hi <= 3e-8, r_hi  # every point of every line in PART2
            out = engine.ht_sum(t2, X_FULL, [296.0], [pk], ones(t2), DIL, **kw)[1][0].cpu().numpy()
            ref = host_sum(t2, X_FULL, prm, 0)
            d = difference(out, ref)
            print("ht_sum vs profile_eval, tiny Gamma2 at %s (|X|/|Y| in [%.3g, %.3g]): max relative difference %.3e, bit-identical %s"
                  % (tag, r_lo, r_hi, d, np.array_equal(out, ref)))
            assert d <= 1e-14
    finally:
        t2.close()


def test_window_edges_of_a_one_line_table(table):
    """(nu0 - W, nu0 + W]: bisect_right on both bounds (misc/hapi.py:10646-10647), with points placed exactly on nu0 -+ W."""
    one = {k: np.asarray(v)[100:101].copy() for k, v in table.items()}
    one["nu"] = np.array([903.5])
    t = engine.LineTable(one)
    try:
        X = np.array([903.0, 903.25, np.nextafter(903.25, 1e9), 903.5, 903.75, np.nextafter(903.75, 1e9), 904.0])
        kw = dict(omega_wing=0.25, omega_wing_hw=0.0)
        prm = engine.ht_line_params(t, X, [296.0], [1.0], ones(t), DIL, **kw)
        assert prm["window"][0, 0].tolist() == [2, 5]
        out = engine.ht_sum(t, X, [296.0], [1.0], ones(t), DIL, **kw)[1][0].cpu().numpy()
        assert np.all(out[2:5] > 0) and np.all(out[[0, 1, 5, 6]] == 0.0)
        assert np.array_equal(out, host_sum(t, X, prm, 0))
    finally:
        t.close()


def test_axis_lengths_around_a_block_and_a_table_outside_the_axis(lines):
    """Whether a point lies in a window is a property of the point (nu0 - W < x <= nu0 + W), so a shorter axis gives the
    same bits at the points it keeps: lengths 1, 255, 256, 257 (one block, its edge, a second block of one point)."""
    w = ones(lines)
    full = engine.ht_sum(lines, X_FULL, [250.0], [0.5], w, DIL)[1][0].cpu().numpy()
    for n in (1, 255, 256, 257):
        for off in (0, 1100):  # the second start puts the band head in the axis
            got = engine.ht_sum(lines, X_FULL[off:off + n], [250.0], [0.5], w, DIL)[1].cpu().numpy()
            assert got.shape == (1, n) and np.array_equal(got[0], full[off:off + n]), (n, off)
    # a line list entirely outside the axis: zeros, exactly
    far = np.linspace(950.0, 951.0, 300)
    out32 = torch.full((1, 300), 7.0, dtype=torch.float32, device="cuda")
    out64 = torch.full((1, 300), 7.0, dtype=torch.float64, device="cuda")
    engine.ht_sum(lines, far, [250.0], [0.5], w, DIL, out_f32=out32, out_f64=out64)
    assert not out64.cpu().numpy().any() and not out32.cpu().numpy().any()
    # no points, and no lines: success without a launch
    assert engine.ht_sum(lines, np.zeros(0), [250.0], [0.5], w, DIL)[1].shape == (1, 0)
    empty = engine.LineTable({k: np.asarray(v)[:0] for k, v in lines.host_columns().items()})
    try:
        z = engine.ht_sum(empty, far, [250.0], [0.5], np.ones((1, 1)), {"air": 1.0})[1]
        assert z.shape == (1, 300) and not z.cpu().numpy().any()
    finally:
        empty.close()


@pytest.mark.parametrize("n_cand", [128, 129, 140])
def test_blocks_with_a_full_chunk_one_more_and_the_band_head(table, n_cand):
    """The sum kernel stages 128 records at a time: a block with exactly one chunk, one record more, and the whole band
    head. The counts are asserted from the prologue's windows; the values against rtx_profile_eval summed on the host."""
    a = HEAD[0]
    sub = {k: np.asarray(v)[a:a + n_cand].copy() for k, v in table.items()}
    t = engine.LineTable(sub)
    try:
        X = np.linspace(903.0, 903.4, 256)
        w = ones(t)
        kw = dict(omega_wing_hw=15.0)
        prm = engine.ht_line_params(t, X, [296.0], [1.0], w, DIL, **kw)
        win = prm["window"][0]
        assert int(np.sum((win[:, 1] > 0) & (win[:, 0] < 256))) == n_cand == t.n
        out = engine.ht_sum(t, X, [296.0], [1.0], w, DIL, **kw)[1][0].cpu().numpy()
        ref = host_sum(t, X, prm, 0)
        d = difference(out, ref)
        print("ht_sum %d candidates: max relative difference to the host sum %.3e, bit-identical %s" % (n_cand, d, np.array_equal(out, ref)))
        assert d <= 1e-14
    finally:
        t.close()


def test_determinism_slices_and_states(lines):
    w = ones(lines)
    T, p = STATES["T"], STATES["p"]
    kw = dict(omega_wing=0.3, omega_wing_hw=15.0)
    a = engine.ht_sum(lines, X_FULL, T, p, w, DIL, **kw)[1].cpu().numpy()
    b = engine.ht_sum(lines, X_FULL, T, p, w, DIL, **kw)[1].cpu().numpy()
    assert a.shape == (4, X_FULL.size) and np.array_equal(a, b) and np.all(np.isfinite(a)) and np.all(a.max(axis=1) > 0)
    s = engine.ht_sum(lines, X_FULL[300:1300], T, p, w, DIL, **kw)[1].cpu().numpy()
    assert np.array_equal(s, a[:, 300:1300])
    for k in range(4):  # the states of one call fall into four TrefHT buckets
        one = engine.ht_sum(lines, X_FULL, [T[k]], [p[k]], w, DIL, **kw)[1].cpu().numpy()
        assert np.array_equal(one[0], a[k]), T[k]
    # the scaled fp32 output next to the fp64 one
    o32 = torch.empty((4, X_FULL.size), dtype=torch.float32, device="cuda")
    o64 = torch.empty((4, X_FULL.size), dtype=torch.float64, device="cuda")
    engine.ht_sum(lines, X_FULL, T, p, w, DIL, out_f32=o32, out_f64=o64, scale=2.0 ** 70, **kw)
    assert np.array_equal(o64.cpu().numpy(), a) and np.array_equal(o32.cpu().numpy(), (a * 2.0 ** 70).astype(np.float32))


def test_sdvoigt_limit_against_the_gather_kernel(table, monkeypatch):
    """A table whose only speed-dependence columns are SD_air / SD_self: nuVC = eta = Shift2 = 0 and Gamma2 = SD gamma, the
    speed-dependent Voigt sum. engine.ht_sum against absorptionCoefficient_SDVoigt's point-by-point kernel, 1e-9."""
    sd = {k: v for k, v in table.items() if "_HT_" not in k and not k.endswith("_h2")}
    H.storage2cache_from_columns("g17sd", sd)
    monkeypatch.setenv("RADTXFR_SD_KERNEL", "gather")
    kw = dict(Environment={"T": 296.0, "p": 1.0}, Diluent={"air": 0.7, "self": 0.3}, OmegaWingHW=15.0)
    assert not H.VARIABLES["HT_COLUMNS"]
    _, xs = H.absorptionCoefficient_SDVoigt(SourceTables="g17sd", OmegaGrid=X_FULL, **kw)
    t = engine.LineTable(sd)
    try:
        assert t.has_sd
        out = engine.ht_sum(t, X_FULL, [296.0], [1.0], ones(t), {"air": 0.7, "self": 0.3}, omega_wing_hw=15.0)[1][0].cpu().numpy()
    finally:
        t.close()
    e = rel_err(out, xs)
    print("ht_sum vs SDVoigt gather kernel: rel_err %.3e" % e)
    assert xs.max() > 0 and e <= 1e-9


def test_the_switch(table, monkeypatch):
    kw = dict(Environment={"T": 296.0, "p": 1.0}, OmegaWingHW=15.0)
    H.VARIABLES["HT_COLUMNS"] = False
    with pytest.raises(NotImplementedError, match="Hartmann-Tran column"):
        H.absorptionCoefficient_HT(SourceTables="g17", OmegaGrid=X_FULL, **kw)
    # HT columns only for a species that is not in Diluent: the call reads none of them, and is the SDVoigt one
    h2 = {k: v for k, v in table.items() if "_HT_" not in k or k in ht_column_names("h2")}
    H.storage2cache_from_columns("g17h2", h2)
    _, sd = H.absorptionCoefficient_SDVoigt(SourceTables="g17h2", OmegaGrid=X_FULL, Diluent={"air": 0.6, "self": 0.4}, **kw)
    with pytest.raises(NotImplementedError):
        H.absorptionCoefficient_HT(SourceTables="g17h2", OmegaGrid=X_FULL, Diluent={"air": 0.6, "self": 0.4}, **kw)
    monkeypatch.setitem(H.VARIABLES, "HT_COLUMNS", True)
    _, on = H.absorptionCoefficient_HT(SourceTables="g17h2", OmegaGrid=X_FULL, Diluent={"air": 0.6, "self": 0.4}, **kw)
    assert np.array_equal(on, sd) and sd.max() > 0
    # ... and with h2 among the diluents it takes the Hartmann-Tran sum: another result, and an edited column is seen
    _, ht = H.absorptionCoefficient_HT(SourceTables="g17h2", OmegaGrid=X_FULL, Diluent={"air": 0.6, "h2": 0.4}, **kw)
    assert not np.array_equal(ht, sd)
    H.LOCAL_TABLE_CACHE["g17h2"]["data"]["eta_HT_h2"] = H.LOCAL_TABLE_CACHE["g17h2"]["data"]["eta_HT_h2"] * 0.5
    _, ht2 = H.absorptionCoefficient_HT(SourceTables="g17h2", OmegaGrid=X_FULL, Diluent={"air": 0.6, "h2": 0.4}, **kw)
    assert not np.array_equal(ht2, ht) and rel_err(ht2, ht) < 0.5
    # a broadener with HT columns and no Voigt-style column at all takes the fallbacks (gamma = delta = deltap = SD = 0,
    # n = n_air): the same bits as a table that spells them out
    d = H.LOCAL_TABLE_CACHE["g17h2"]["data"]
    bare = {k: v for k, v in d.items() if not (k.endswith("_h2") and "_HT_" not in k)}
    spelt = dict(bare, gamma_h2=np.zeros(N_LINES), delta_h2=np.zeros(N_LINES), deltap_h2=np.zeros(N_LINES), SD_h2=np.zeros(N_LINES),
                 n_h2=np.asarray(d["n_air"]).copy())
    H.storage2cache_from_columns("g17h2_bare", bare)
    H.storage2cache_from_columns("g17h2_spelt", spelt)
    for _ in range(2):  # (the second call finds the table and its column sets cached)
        _, xb = H.absorptionCoefficient_HT(SourceTables="g17h2_bare", OmegaGrid=X_FULL, Diluent={"air": 0.6, "h2": 0.4}, **kw)
        _, xp = H.absorptionCoefficient_HT(SourceTables="g17h2_spelt", OmegaGrid=X_FULL, Diluent={"air": 0.6, "h2": 0.4}, **kw)
        assert np.array_equal(xb, xp) and xb.max() > 0 and not np.array_equal(xb, ht2)
    with pytest.raises(NotImplementedError, match="EnvDependences"):
        H.absorptionCoefficient_HT(SourceTables="g17h2", OmegaGrid=X_FULL, Diluent={"h2": 1.0}, EnvDependences=lambda e, l: {}, **kw)


def test_refusals_that_need_a_table_on_the_device(lines):
    """A column set that does not exist and ld < n, refused with text and without a launch."""
    lib = _lib.load()
    h = C.c_void_p(0)
    assert lib.rtx_ht_create(lines.n, 1, 64, C.byref(h)) == 0
    try:
        X = np.linspace(903.0, 903.2, 64)
        one, q, w, m = np.array([296.0]), np.ones(len(lines.species)), np.ones(len(lines.species)), np.full(len(lines.species), 18.0)
        idx, fr = np.array([60], dtype=np.int32), np.ones(len(lines.species))
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = lib.rtx_ht_prep(h, lines._h, ptr(X), 64, 1, ptr(one), ptr(one), ptr(q), ptr(w), ptr(m), 1, ptr(idx), ptr(fr), 0.0, 50.0, 0.0, 1.0, None)
        assert rc != 0 and "column set 60" in lib.rtx_last_error().decode()
        sets = (C.c_int32 * 1)(60)
        cols = (C.c_void_p * 27)()
        assert lib.rtx_lines_set_ht(lines._h, 1, sets, cols) != 0 and "column set 60" in lib.rtx_last_error().decode()
        idx[0] = 0
        assert lib.rtx_ht_prep(h, lines._h, ptr(X), 64, 1, ptr(one), ptr(one), ptr(q), ptr(w), ptr(m), 1, ptr(idx), ptr(fr), 0.0, 50.0, 0.0, 1.0, None) == 0
        out = torch.zeros((1, 64), dtype=torch.float64, device="cuda")
        rc = lib.rtx_ht_sum(h, 1, None, C.c_void_p(out.data_ptr()), 63, None)
        assert rc != 0 and "ld=63" in lib.rtx_last_error().decode()
        assert lib.rtx_ht_sum(h, 2, None, C.c_void_p(out.data_ptr()), 64, None) != 0
        assert lib.rtx_ht_params(h, 1, None, None, None, None) != 0
        torch.cuda.synchronize()
        assert not out.cpu().numpy().any()
    finally:
        lib.rtx_ht_free(h)
