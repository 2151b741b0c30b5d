"""GPU: line broadening by any diluent (hapi shims, engine diluent=) and per-layer self-broadening on the TUD path
(compute_TUD / compute_TUD_batch broadening=), against the reference's own cross sections (tests/golden/g14_diluents.npz)
and the fp64 oracle.

Tolerances as tests/test_gpu_parity.py: cross sections / OD / radiances max |x-ref| / max(|ref|, 1e-3 max|ref|) <= 1e-5
(fp32 line-sum), |dtau| <= 2e-6; the speed-dependent sum is fp64 (1e-9).
"""
import json

import numpy as np
import pytest

from conftest import rel_err
from make_golden_diluents import g14_axis, g14_table
from oracle import cpu_ref as ref
from radtxfr_amd import synthetic

pytestmark = pytest.mark.gpu

TOL_L = 1e-5
TOL_TAU = 2e-6
TOL_SD = 1e-9


@pytest.fixture(scope="module")
def rt():
    import torch
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    from radtxfr_amd import _lib
    _lib.load()
    from radtxfr_amd import radiative_transfer
    return radiative_transfer


@pytest.fixture(scope="module")
def hapi(rt):
    from radtxfr_amd import hapi as h
    return h


def test_g14_hapi_shims_any_diluent(hapi, golden):
    """Every g14 case through the drop-in absorptionCoefficient_*: Diluent keys other than air / self (lower and upper
    case, a key without columns, repeated keys), Voigt / Lorentz / SDVoigt / HT, HITRAN_units=False, a non-uniform grid."""
    g = golden("g14_diluents.npz")
    tbl = g14_table(g)
    hapi.storage2cache_from_columns("g14", tbl)
    try:
        for c in json.loads(str(g["cases"])):
            kw = dict(SourceTables="g14", Environment={"T": c["T"], "p": c["p"]}, OmegaGrid=g14_axis(c), Diluent=c["Diluent"])
            if "HITRAN_units" in c:
                kw["HITRAN_units"] = c["HITRAN_units"]
            _, xs = getattr(hapi, "absorptionCoefficient_" + c["fn"])(**kw)
            r = g["xs_" + c["tag"]]
            tol = TOL_SD if c["fn"] in ("SDVoigt", "HT") else TOL_L
            assert rel_err(xs, r) <= tol, (c["tag"], rel_err(xs, r))
            assert np.array_equal(xs != 0, r != 0), c["tag"]
    finally:
        hapi.LOCAL_TABLE_CACHE.pop("g14", None)


def test_broadener_columns_fingerprinted(hapi):
    """An in-place edit of gamma_h2 in the cached table is seen by the next call (no stale device copy)."""
    tbl = synthetic.synth_line_table(12, 300, 995.0, 1005.0)
    rng = np.random.default_rng(5)
    tbl["gamma_h2"] = np.round(rng.uniform(0.05, 0.15, 300), 4)
    hapi.storage2cache_from_columns("edit_h2", tbl)
    grid = np.linspace(998.0, 1002.0, 4001)
    kw = dict(SourceTables="edit_h2", Environment={"T": 280.0, "p": 0.8}, OmegaGrid=grid, Diluent={"air": 0.4, "h2": 0.6})
    try:
        _, x0 = hapi.absorptionCoefficient_Voigt(**kw)
        _, r0 = ref.absorptionCoefficient_Voigt(tbl, T=280.0, p=0.8, OmegaGrid=grid, Diluent={"air": 0.4, "h2": 0.6})
        assert rel_err(x0, r0) <= TOL_L
        hapi.LOCAL_TABLE_CACHE["edit_h2"]["data"]["gamma_h2"] *= 3.0  # same array object, same row count
        _, x1 = hapi.absorptionCoefficient_Voigt(**kw)
        t1 = dict(tbl, gamma_h2=tbl["gamma_h2"] * 3.0)
        _, r1 = ref.absorptionCoefficient_Voigt(t1, T=280.0, p=0.8, OmegaGrid=grid, Diluent={"air": 0.4, "h2": 0.6})
        assert rel_err(x1, r1) <= TOL_L and rel_err(x1, x0) > 1e-2
        # a new broadener column appearing in the cached table is picked up too
        hapi.LOCAL_TABLE_CACHE["edit_h2"]["data"]["n_h2"] = np.full(300, 0.3)
        _, x2 = hapi.absorptionCoefficient_Voigt(**kw)
        _, r2 = ref.absorptionCoefficient_Voigt(dict(t1, n_h2=np.full(300, 0.3)), T=280.0, p=0.8, OmegaGrid=grid,
                                                Diluent={"air": 0.4, "h2": 0.6})
        assert rel_err(x2, r2) <= TOL_L and rel_err(x2, x1) > 1e-3
        # air-only calls on the same table are unaffected
        _, xa = hapi.absorptionCoefficient_Voigt(SourceTables="edit_h2", Environment={"T": 280.0, "p": 0.8}, OmegaGrid=grid)
        _, ra = ref.absorptionCoefficient_Voigt(tbl, T=280.0, p=0.8, OmegaGrid=grid)
        assert rel_err(xa, ra) <= TOL_L
    finally:
        hapi.LOCAL_TABLE_CACHE.pop("edit_h2", None)


def _self_table():
    tbl = synthetic.synth_line_table(13, 500, 995.0, 1005.0)
    rng = np.random.default_rng(6)
    tbl["n_self"] = np.round(rng.uniform(0.5, 0.9, 500), 2)
    tbl["n_self"][::4] = 0.0
    tbl["delta_self"] = np.round(rng.uniform(-0.02, 0.01, 500), 6)
    tbl["deltap_self"] = np.round(rng.uniform(-1e-4, 1e-4, 500), 7)
    tbl["deltap_air"] = np.round(rng.uniform(-1e-4, 1e-4, 500), 7)
    tbl["SD_air"] = np.round(rng.uniform(0.05, 0.2, 500), 4)
    tbl["SD_self"] = np.round(rng.uniform(0.0, 0.1, 500), 4)
    return tbl


def test_mix_prologue_equals_scalar_prologue(rt):
    """diluent={"air": 0.7, "self": 0.3} through rtx_line_prep_mix gives the records, hence the line-sum, of dil_air=0.7,
    dil_self=0.3 through rtx_line_prep_profile / _axis, bit for bit: grid (Voigt, Lorentz, SDVoigt) and axis (Voigt, Lorentz)."""
    import torch
    from radtxfr_amd import engine
    lt = engine.LineTable(_self_table())
    nS = len(lt.species)
    T, p = np.array([296.0, 250.0, 220.0]), np.array([1.0, 0.5, 0.1])
    w = np.ones((nS, 3))
    grid = engine.Grid(998.0, 1002.0, 8001)
    dev = engine.device()
    for profile in (0, 1, 3):
        outs = []
        for kw in (dict(dil_air=0.7, dil_self=0.3), dict(diluent={"air": 0.7, "self": 0.3})):
            o32 = torch.empty((3, grid.n), dtype=torch.float32, device=dev) if profile != 3 else None
            o64 = torch.empty((3, grid.n), dtype=torch.float64, device=dev)
            engine.voigt_sum(lt, grid, T, p, w, out_f32=o32, out_f64=o64, scale=2.0 ** 70, profile=profile, **kw)
            outs.append([o.cpu().numpy() for o in (o32, o64) if o is not None])
        for a, b in zip(*outs):
            assert np.array_equal(a, b), profile
        assert np.max(outs[0][-1]) > 0
    X = np.sort(np.concatenate([np.linspace(998.0, 1002.0, 3000), np.random.default_rng(7).uniform(999.0, 1001.0, 1000)]))
    for profile in (0, 1):
        outs = []
        for kw in (dict(dil_air=0.7, dil_self=0.3), dict(diluent={"air": 0.7, "self": 0.3})):
            o32 = torch.empty((3, X.size), dtype=torch.float32, device=dev)
            o64 = torch.empty((3, X.size), dtype=torch.float64, device=dev)
            engine.voigt_sum_axis(lt, X, T, p, w, out_f32=o32, out_f64=o64, scale=2.0 ** 70, profile=profile, **kw)
            outs.append([o32.cpu().numpy(), o64.cpu().numpy()])
        for a, b in zip(*outs):
            assert np.array_equal(a, b), profile
    # per-layer fractions: each layer's row is the single-layer call with that layer's scalars
    fa, fs = np.array([0.9, 0.6, 0.2]), np.array([0.1, 0.4, 0.8])
    o = torch.empty((3, grid.n), dtype=torch.float32, device=dev)
    engine.voigt_sum(lt, grid, T, p, w, out_f32=o, scale=2.0 ** 70,
                     diluent={"air": np.tile(fa, (nS, 1)), "self": np.tile(fs, (nS, 1))})
    for k in range(3):
        o1 = torch.empty((1, grid.n), dtype=torch.float32, device=dev)
        engine.voigt_sum(lt, grid, T[k:k + 1], p[k:k + 1], w[:, k:k + 1], out_f32=o1, scale=2.0 ** 70, dil_air=fa[k], dil_self=fs[k])
        assert np.array_equal(o[k].cpu().numpy(), o1[0].cpu().numpy()), k
    lt.close()


def test_mix_split_bound_covers_wide_foreign_gamma(rt):
    """The hot-tile bound of the mixed prologue takes the foreign sets' gamma / n extremes: on a dense table whose h2
    widths are ten times the air widths it covers the true work list (which the air-only bound does not), and the
    cut tiles still sum to the oracle."""
    import torch
    from radtxfr_amd import _lib, engine
    lib = _lib.load()
    n = 6000
    tbl = synthetic.synth_line_table(14, n, 980.0, 1020.0)
    rng = np.random.default_rng(8)
    tbl["gamma_h2"] = np.round(rng.uniform(0.5, 1.0, n), 4)
    tbl["n_h2"] = np.round(rng.uniform(0.2, 0.4, n), 2)
    comps = [(1, 1)]
    keep = (tbl["molec_id"] == 1) & (tbl["local_iso_id"] == 1)
    tbl = {k: v[keep] for k, v in tbl.items()}
    lt = engine.LineTable(tbl)
    nS = len(lt.species)
    w = np.zeros((nS, 2))
    w[lt.species.index((1, 1))] = 1.0
    X = np.linspace(999.0, 1001.0, 8001)
    grid = engine.Grid.from_axis(X)
    T, p = np.array([296.0, 240.0]), np.array([1.0, 0.6])
    dil = {"air": 0.5, "h2": 0.5}
    out = torch.empty((2, grid.n), dtype=torch.float64, device=engine.device())
    # air first: a prologue keeps a cached bound that covers it, so the narrower call must come before the wider one
    engine.voigt_sum(lt, grid, T, p, w, out_f64=torch.empty_like(out), dil_air=0.5, scale=2.0 ** 70)
    bound_air = int(lib.rtx_prep_split_bound(lt.plan(2, grid.n)._h))
    engine.voigt_sum(lt, grid, T, p, w, out_f64=out, diluent=dil, scale=2.0 ** 70)
    bound_mix = int(lib.rtx_prep_split_bound(lt.plan(2, grid.n)._h))
    tile = int(lib.rtx_voigt_tile_points())
    true_extra = 0
    nu = lt.cols["nu"]
    for k in range(2):
        P = ref.line_params(tbl, T[k], p[k], Diluent=dil)
        order = np.argsort(tbl["nu"], kind="stable")
        W = np.maximum(50.0 * P["Gamma0"], 50.0 * P["GammaD"])[order]
        lo, hi = np.searchsorted(X, nu - W, side="right"), np.searchsorted(X, nu + W, side="right")
        for ia in range(0, grid.n, tile):
            ib = min(ia + tile, grid.n)
            reach = np.nonzero((hi > ia) & (lo < ib) & (hi > lo))[0]
            if reach.size:
                cnt = int(reach[-1] + 1 - reach[0])
                if cnt > 768:
                    true_extra += (cnt - 1) // 256
    assert true_extra > 0 and bound_mix >= true_extra and bound_air < true_extra, (bound_mix, bound_air, true_extra)
    xs = out.cpu().numpy()
    for k in range(2):
        _, xr = ref.absorptionCoefficient_Voigt(tbl, Components=comps, T=T[k], p=p[k], OmegaGrid=X, Diluent=dil)
        assert rel_err(xs[k], xr) <= TOL_L, (k, rel_err(xs[k], xr))
    lt.close()


# ---- per-layer self-broadening on the TUD path ----------------------------------------------------------------------
LO, HI, DV = 1000.0, 1010.0, 0.002


def _h2o_window(extra_cols=False):
    """H2O (+ CO2 with extra_cols) lines of the C3 table around the window, strengths thinned so tau spans (0, 1) at full
    mixing ratios (the mixing ratios set the self-broadening; the strengths do not)."""
    full = synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)
    sub = synthetic.subset_table(full, LO - 12.0, HI + 12.0)
    if not extra_cols:
        sub = {k: v[sub["molec_id"] == 1] for k, v in sub.items()}
    sub["sw"] = sub["sw"] * 1e-3
    if extra_cols:
        rng = np.random.default_rng(9)
        sub["gamma_h2o"] = np.round(rng.uniform(0.2, 0.5, sub["nu"].size), 4)
        sub["n_h2o"] = np.round(rng.uniform(0.5, 0.9, sub["nu"].size), 2)
    return sub


def _oracle_od(tbl, X, a, layers, foreign=()):
    """Per layer and molecule: the reference's Voigt with Diluent {air: 1 - sum, self: x_m, gas: x_g (g != m)}, x PL 1e5."""
    ids = [int(v) for v in a["MFs_ID"]]
    pairs = sorted(set(zip(tbl["molec_id"].tolist(), tbl["local_iso_id"].tolist())))
    gid = {"h2o": 1, "co2": 2}
    OD = np.zeros((len(layers), X.size))
    for j, k in enumerate(layers):
        for m in sorted(set(tbl["molec_id"].tolist())):
            x = a["MFs_VAL"][k, ids.index(m)] * 1e-6
            dil = {"air": None, "self": x}
            tot = x
            for g in foreign:
                xg = 0.0 if gid[g] == m else a["MFs_VAL"][k, ids.index(gid[g])] * 1e-6
                dil[g] = xg
                tot = tot + xg
            dil["air"] = 1.0 - tot
            _, xs = ref.absorptionCoefficient_Voigt(tbl, Components=[c for c in pairs if c[0] == m], T=float(a["Ts"][k]),
                                                    p=float(a["Ps"][k]) / 101325.0, OmegaGrid=X, HITRAN_units=False, Diluent=dil)
            OD[j] += xs * (a["MFs_VAL"][k, ids.index(m)] * 1e-6) * a["PLs"][k] * 1e5
    return OD


def test_compute_tud_self_broadening_vs_oracle(rt):
    from radtxfr_amd import engine
    sub = _h2o_window()
    a = synthetic.c3_atmosphere(32)
    X, tau, Lu, Ld = rt.compute_TUD(LO, HI, DVOUT=DV, line_table=sub, Altitudes=np.asarray([500]), broadening="self", **a)
    ODr = _oracle_od(sub, X, a, range(32))
    tau_r, Lu_r, Ld_r = ref.tud_from_od(X, ODr.T, a["Ts"], a["Zs"], Altitudes=(500,))
    assert np.max(np.abs(tau - tau_r)) <= TOL_TAU
    assert rel_err(Lu, Lu_r) <= TOL_L and rel_err(Ld, Ld_r) <= TOL_L
    tbl = rt._resolve_table(sub)
    grid = engine.Grid(LO, HI, X.size)
    od_self = engine.optical_depths(tbl, grid, a["Ts"], a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"], broadening="self").double().cpu().numpy()
    od_air = engine.optical_depths(tbl, grid, a["Ts"], a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"]).double().cpu().numpy()
    for k in range(32):
        assert rel_err(od_self[k], ODr[k]) <= TOL_L, (k, rel_err(od_self[k], ODr[k]))
    # the option is visibly on: the lowest layer's H2O lines are several percent wider
    assert rel_err(od_self[0], od_air[0]) > 100 * TOL_L
    # broadening=None is today's path: the same bits as a call without the keyword
    base = rt.compute_TUD(LO, HI, DVOUT=DV, line_table=sub, Altitudes=np.asarray([500]), **a)
    none = rt.compute_TUD(LO, HI, DVOUT=DV, line_table=sub, Altitudes=np.asarray([500]), broadening=None, **a)
    for b, c in zip(base[1:], none[1:]):
        assert np.array_equal(b, c)
    assert rel_err(base[2], Lu) > 10 * TOL_L


def test_foreign_broadening_od_vs_oracle(rt):
    """("self", "h2o"): H2O lines take self, CO2 lines self + the table's gamma_h2o column at the H2O mixing ratio."""
    from radtxfr_amd import engine
    sub = _h2o_window(extra_cols=True)
    a = synthetic.c3_atmosphere(32)
    X = rt.make_spectral_axis(LO, HI, DV)
    layers = [0, 9, 31]
    ODr = _oracle_od(sub, X, a, layers, foreign=("h2o",))
    tbl = rt._resolve_table(sub, ("h2o",))
    grid = engine.Grid(LO, HI, X.size)
    od = engine.optical_depths(tbl, grid, a["Ts"], a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"],
                               broadening=("self", "h2o")).double().cpu().numpy()
    od_s = engine.optical_depths(tbl, grid, a["Ts"], a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"],
                                 broadening="self").double().cpu().numpy()
    for j, k in enumerate(layers):
        assert rel_err(od[k], ODr[j]) <= TOL_L, (k, rel_err(od[k], ODr[j]))
    assert rel_err(od[0], od_s[0]) > 10 * TOL_L
    X2, tau, Lu, Ld = rt.compute_TUD(LO, HI, DVOUT=DV, line_table=sub, Altitudes=np.asarray([500]), broadening=("self", "h2o"), **a)
    assert np.all(np.isfinite(Lu)) and np.all(np.isfinite(Ld))


def test_compute_tud_batch_self_broadening_equals_per_call(rt):
    sub = _h2o_window()
    a = synthetic.c3_atmosphere(32)
    common = {k: a[k] for k in ("Zs", "Ts", "Ps", "PLs", "MFs_ID")}  # the batch takes its layer count from Ts
    atms = [dict(Ts=a["Ts"], MFs_VAL=a["MFs_VAL"]), dict(Ts=a["Ts"] + 5.0, MFs_VAL=a["MFs_VAL"] * 1.5),
            dict(Ts=a["Ts"] - 3.0, MFs_VAL=a["MFs_VAL"] * 0.5)]
    res = rt.compute_TUD_batch(LO, HI, atms, DVOUT=DV, line_table=sub, Altitudes=np.asarray([500]), broadening="self", **common)
    for atm, r in zip(atms, res):
        one = rt.compute_TUD(LO, HI, DVOUT=DV, line_table=sub, Altitudes=np.asarray([500]), broadening="self", **dict(common, **atm))
        for x, y in zip(r[1:], one[1:]):
            assert np.array_equal(x, y)
    with pytest.raises(NotImplementedError, match="broadening"):
        rt.compute_TUD_jacobian(LO, HI, DVOUT=DV, line_table=sub, broadening="self", **a)


def test_tud_pipelines_broadening(rt):
    """engine.TudPipelines(broadening=) gives the single runner's bits."""
    import torch
    from radtxfr_amd import engine
    sub = _h2o_window()
    a = synthetic.c3_atmosphere(32)
    tbl = rt._resolve_table(sub)
    X = rt.make_spectral_axis(LO, HI, DV)
    grid = engine.Grid(LO, HI, X.size)
    run = engine.TudRunner(tbl, grid, a["Zs"], broadening="self")
    ref_out = [t.cpu().numpy().copy() for t in run.run(a["Ts"], a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"])]
    pipes = engine.TudPipelines(tbl, grid, a["Zs"], n_pipes=2, broadening="self")
    try:
        for _ in range(2):
            pi, out = pipes.run(a["Ts"], a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"])
            torch.cuda.synchronize()
            for x, y in zip(out, ref_out):
                assert np.array_equal(x.cpu().numpy(), y)
    finally:
        pipes.close()


def test_cross_section_grid_diluent(hapi, golden):
    """afit_xs.cross_section_grid(Diluent=) is the reference generator's absorptionCoefficient_SDVoigt with that Diluent: the
    g14 SDVoigt case, and a three-diluent mix against the oracle (SD_h2 makes it speed-dependent)."""
    from radtxfr_amd import afit_xs
    g = golden("g14_diluents.npz")
    tbl = g14_table(g)
    hapi.storage2cache_from_columns("g14x", tbl)
    try:
        for c in json.loads(str(g["cases"])):
            if c["tag"] not in ("voigt_air_h2_he", "sdvoigt_h2"):
                continue
            X = g14_axis(c)
            xs = afit_xs.cross_section_grid("g14x", [c["T"]], [c["p"]], X, Diluent=c["Diluent"])[0, 0]
            if c["fn"] == "SDVoigt":
                r = g["xs_" + c["tag"]]
            else:
                _, r = ref.absorptionCoefficient_SDVoigt(tbl, T=c["T"], p=c["p"], OmegaGrid=X, Diluent=c["Diluent"])
            assert rel_err(xs, r) <= TOL_SD, (c["tag"], rel_err(xs, r))
    finally:
        hapi.LOCAL_TABLE_CACHE.pop("g14x", None)
