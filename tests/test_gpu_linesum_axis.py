"""The line-sum on explicit, non-uniform wavenumber axes (rtx_line_prep_axis + rtx_voigt_sum_axis): what the hapi shims
compute for an OmegaGrid / WavenumberGrid that is not an np.linspace -- the reference sorts whatever grid it is given and
bisects it (misc/hapi.py:10979-10983, 11133-11134) -- against the CPU oracle, which does the same.

Tolerance: the suite's, max |x-ref| / max(|ref|, 1e-3 max|ref|) <= 1e-5; where a line's window ends inside the grid, the
support (non-zero set) must be the oracle's point for point (Voigt and Lorentz; the Doppler profile is dropped beyond
|x| = 15, where the reference's exp(-x^2) is below 1e-98)."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import rel_err
from oracle import cpu_ref as ref
from radtxfr_amd import synthetic

pytestmark = pytest.mark.gpu

TOL_L = 1e-5


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


def _g4_table():
    return synthetic.synth_line_table(synthetic.SEED_C2, 2000, 675.0, 1425.0)  # the G4 golden's table


def _two_density(lo, hi, centre, half, fine, coarse):
    """fine steps within +-half of centre, coarse steps elsewhere: a grid no Grid.from_axis accepts"""
    return np.concatenate([np.arange(lo, centre - half, coarse), np.arange(centre - half, centre + half, fine),
                           np.arange(centre + half, hi, coarse)])


def _not_uniform(grid):
    from radtxfr_amd import engine
    with pytest.raises(NotImplementedError):
        engine.Grid.from_axis(grid)


def _support_equal(xs, xr):
    return np.array_equal(xs != 0, xr != 0)


def test_a_two_density_grid_vs_oracle(hapi):
    tbl = _g4_table()
    hapi.storage2cache_from_columns("ax_g4", tbl)
    nu, sw = tbl["nu"], tbl["sw"]
    sel = (nu > 952.0) & (nu < 1048.0)
    strongest = float(nu[sel][np.argmax(sw[sel])])
    grid = _two_density(950.0, 1050.0, strongest, 2.0, 0.0005, 0.02)
    _not_uniform(grid)
    for T, p in ((296.0, 1.0), (220.0, 0.02)):
        om, xs = hapi.absorptionCoefficient_Voigt(SourceTables="ax_g4", Environment={"T": T, "p": p}, OmegaGrid=grid)
        _, xr = ref.absorptionCoefficient_Voigt(tbl, T=T, p=p, OmegaGrid=grid)
        assert np.array_equal(om, grid) and xs.dtype == np.float64 and xs.shape == grid.shape
        assert rel_err(xs, xr) <= TOL_L, (T, p, rel_err(xs, xr))
        assert _support_equal(xs, xr)
        if p < 0.1:  # at low pressure the windows end inside the grid: the support test means something
            assert (xr == 0).sum() > 100


def test_b_wavelength_uniform_grid_vs_oracle(hapi):
    tbl = _g4_table()
    hapi.storage2cache_from_columns("ax_g4", tbl)
    grid = np.sort(1e4 / np.linspace(7.5, 13.5, 200_000))
    _not_uniform(grid)
    for T, p in ((296.0, 1.0), (230.0, 0.05)):
        om, xs = hapi.absorptionCoefficient_Voigt(SourceTables="ax_g4", Environment={"T": T, "p": p}, OmegaGrid=grid)
        _, xr = ref.absorptionCoefficient_Voigt(tbl, T=T, p=p, OmegaGrid=grid)
        assert np.array_equal(om, grid)
        assert rel_err(xs, xr) <= TOL_L, (T, p, rel_err(xs, xr))
        assert _support_equal(xs, xr)


def test_c_unsorted_input_with_repeated_points(hapi):
    tbl = _g4_table()
    hapi.storage2cache_from_columns("ax_g4", tbl)
    rng = np.random.default_rng(7)
    base = np.linspace(995.0, 1005.0, 4001)
    raw = np.concatenate([base, base[::7], base[::13], rng.uniform(995.0, 1005.0, 3000)])
    raw = raw[rng.permutation(raw.size)]
    om, xs = hapi.absorptionCoefficient_Voigt(SourceTables="ax_g4", Environment={"T": 250.0, "p": 0.1}, OmegaGrid=raw)
    _, xr = ref.absorptionCoefficient_Voigt(tbl, T=250.0, p=0.1, OmegaGrid=raw)
    assert np.array_equal(om, np.sort(raw))
    same = np.flatnonzero(om[1:] == om[:-1])
    assert same.size > 500
    # equal points get equal values: the same bits inside one line-sum tile (same lines, same order, same abscissa), the
    # fp32 rounding of a regrouped sum across a tile boundary
    tp = 1024
    inside = same[(same // tp) == ((same + 1) // tp)]
    assert np.array_equal(xs[inside], xs[inside + 1])
    assert rel_err(xs[same], xs[same + 1]) <= 1e-6
    assert rel_err(xs, xr) <= TOL_L and _support_equal(xs, xr)


def test_d_doppler_regime_vs_oracle(hapi):
    """Low pressure at 5000 cm^-1: y << 1, the band lanes take fp64 Weideman on the fp64 abscissa."""
    tbl = synthetic.synth_line_table(5, 300, 4990.0, 5010.0)
    hapi.storage2cache_from_columns("ax_dop", tbl)
    rng = np.random.default_rng(11)
    grid = np.sort(np.concatenate([rng.uniform(4995.0, 5005.0, 40000), np.linspace(4995.0, 5005.0, 3001)]))
    _not_uniform(grid)
    for T, p in ((250.0, 0.005), (296.0, 0.01)):
        _, xs = hapi.absorptionCoefficient_Voigt(SourceTables="ax_dop", Environment={"T": T, "p": p}, OmegaGrid=grid)
        _, xr = ref.absorptionCoefficient_Voigt(tbl, T=T, p=p, OmegaGrid=grid)
        assert rel_err(xs, xr) <= TOL_L, (T, p, rel_err(xs, xr))
        assert _support_equal(xs, xr)
        _, xs = hapi.absorptionCoefficient_Doppler(SourceTables="ax_dop", Environment={"T": T, "p": p}, OmegaGrid=grid)
        _, xr = ref.absorptionCoefficient_Doppler(tbl, T=T, p=p, OmegaGrid=grid)
        assert rel_err(xs, xr) <= TOL_L, ("doppler", T, p, rel_err(xs, xr))


def test_e_lorentz_doppler_and_options_vs_oracle(hapi):
    tbl = _g4_table()
    hapi.storage2cache_from_columns("ax_g4", tbl)
    grid = np.sort(1e4 / np.linspace(9.6, 10.4, 40000))
    _not_uniform(grid)
    env = {"T": 250.0, "p": 0.4}
    opt = dict(Components=[(1, 1), (2, 1, 0.5)], HITRAN_units=False, OmegaWing=1.0, OmegaWingHW=20.0)
    opt_ref = dict(Components=[(1, 1), (2, 1, 0.5)], HITRAN_units=False, OmegaWing=1.0, OmegaWingHW=20.0)
    cases = [  # (shim function, oracle function, shim options, oracle options, support test)
        (hapi.absorptionCoefficient_Lorentz, ref.absorptionCoefficient_Lorentz, {}, {}, True),
        (hapi.absorptionCoefficient_Lorentz, ref.absorptionCoefficient_Lorentz, dict(opt, Diluent={"air": 0.7, "self": 0.3}),
         dict(opt_ref, Diluent={"air": 0.7, "self": 0.3}), True),
        (hapi.absorptionCoefficient_Lorentz, ref.absorptionCoefficient_Lorentz, dict(GammaL="gamma_self", IntensityThreshold=1e-23),
         dict(GammaL="gamma_self", IntensityThreshold=1e-23), True),
        (hapi.absorptionCoefficient_Voigt, ref.absorptionCoefficient_Voigt, dict(opt, GammaL="gamma_self"),
         dict(opt_ref, GammaL="gamma_self"), True),
        (hapi.absorptionCoefficient_Voigt, ref.absorptionCoefficient_Voigt, dict(Diluent={"air": 0.7, "self": 0.3},
         IntensityThreshold=1e-23), dict(Diluent={"air": 0.7, "self": 0.3}, IntensityThreshold=1e-23), True),
        (hapi.absorptionCoefficient_Doppler, ref.absorptionCoefficient_Doppler, {}, {}, False),
        (hapi.absorptionCoefficient_Doppler, ref.absorptionCoefficient_Doppler, dict(LineShift=False, HITRAN_units=False, OmegaWing=0.05),
         dict(LineShift=False, HITRAN_units=False, OmegaWing=0.05), False),
        (hapi.absorptionCoefficient_Doppler, ref.absorptionCoefficient_Doppler, dict(Components=[(2, 1, 0.5)], OmegaWingHW=20.0),
         dict(Components=[(2, 1, 0.5)], OmegaWingHW=20.0), False),
    ]
    for fn, fr, kw, kwr, support in cases:
        om, xs = fn(SourceTables="ax_g4", Environment=env, OmegaGrid=grid, **kw)
        _, xr = fr(tbl, T=env["T"], p=env["p"], OmegaGrid=grid, **kwr)
        assert np.array_equal(om, grid) and np.any(xr != 0)
        assert rel_err(xs, xr) <= TOL_L, (fn.__name__, kw, rel_err(xs, xr))
        if support:
            assert _support_equal(xs, xr), (fn.__name__, kw)
    # the threshold really drops lines
    _, xall = ref.absorptionCoefficient_Lorentz(tbl, T=env["T"], p=env["p"], OmegaGrid=grid, GammaL="gamma_self")
    _, xthr = ref.absorptionCoefficient_Lorentz(tbl, T=env["T"], p=env["p"], OmegaGrid=grid, GammaL="gamma_self", IntensityThreshold=1e-23)
    assert np.any(xall != xthr)


def _clustered_head():
    tbl = synthetic.synth_clustered_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)
    h, edges = np.histogram(tbl["nu"], bins=np.arange(475.0, 6026.0, 0.5))
    return tbl, float(edges[int(np.argmax(h))]), int(h.max())


def test_f_clustered_band_head_vs_oracle(hapi):
    """A band head with ~3000 lines inside 0.5 cm^-1 on a two-density grid across it: thousands of candidates on one tile
    (tiles of the axis path are never cut), many repeated centres, strengths spanning eleven decades."""
    tbl, head, n_head = _clustered_head()
    assert n_head >= 2500
    grid = _two_density(head - 1.0, head + 1.5, head + 0.25, 0.5, 0.0005, 0.002)
    _not_uniform(grid)
    sub = synthetic.subset_table(tbl, grid[0] - 12.0, grid[-1] + 12.0)
    assert sub["nu"].size > 3000
    hapi.storage2cache_from_columns("ax_clu", sub)
    for T, p in ((287.9, 0.994), (220.0, 0.01)):
        _, xs = hapi.absorptionCoefficient_Voigt(SourceTables="ax_clu", Environment={"T": T, "p": p}, OmegaGrid=grid)
        _, xr = ref.absorptionCoefficient_Voigt(sub, T=T, p=p, OmegaGrid=grid)
        assert rel_err(xs, xr) <= TOL_L, (T, p, rel_err(xs, xr))
        assert _support_equal(xs, xr)
    hapi.LOCAL_TABLE_CACHE.pop("ax_clu")


def test_g_tiny_grids_empty_grids_alias_and_file(hapi, tmp_path):
    tbl = _g4_table()
    hapi.storage2cache_from_columns("ax_g4", tbl)
    # one point (the grid path needs two): on a line's wing, and exactly on a line centre
    nu0 = float(tbl["nu"][1000])
    for pts in ([1000.0], [nu0], [nu0, nu0], [nu0, nu0 + 0.01, nu0 + 0.01]):
        om, xs = hapi.absorptionCoefficient_Voigt(SourceTables="ax_g4", OmegaGrid=np.array(pts))
        _, xr = ref.absorptionCoefficient_Voigt(tbl, OmegaGrid=np.array(pts))
        assert om.shape == (len(pts),) and rel_err(xs, xr) <= TOL_L, pts
        assert np.all(xs > 0) or nu0 not in pts
    # no points: two empty arrays, as the reference returns
    om, xs = hapi.absorptionCoefficient_Voigt(SourceTables="ax_g4", OmegaGrid=np.array([]))
    assert om.shape == (0,) and xs.shape == (0,)
    # beyond every line: exact zeros
    far = np.sort(1e4 / np.linspace(3.30, 3.31, 5000))
    _not_uniform(far)
    om, xs = hapi.absorptionCoefficient_Lorentz(SourceTables="ax_g4", OmegaGrid=far)
    assert xs.shape == far.shape and np.all(xs == 0)
    # WavenumberGrid= is OmegaGrid=; File= writes the same rows
    grid = np.sort(1e4 / np.linspace(9.9, 10.1, 7000))
    f = tmp_path / "xs.txt"
    om1, xs1 = hapi.absorptionCoefficient_Voigt(SourceTables="ax_g4", OmegaGrid=grid, File=str(f))
    om2, xs2 = hapi.absorptionCoefficient_Voigt(SourceTables="ax_g4", WavenumberGrid=grid)
    assert np.array_equal(om1, om2) and np.array_equal(xs1, xs2)
    rows = np.loadtxt(f)
    assert rows.shape == (grid.size, 2) and np.allclose(rows[:, 0], grid, rtol=0, atol=1e-11)
    assert np.allclose(rows[:, 1], xs1, rtol=1e-6, atol=0)
    _, xr = ref.absorptionCoefficient_Voigt(tbl, OmegaGrid=grid)
    assert rel_err(xs1, xr) <= TOL_L


def test_h_uniform_axis_matches_grid_path_and_is_deterministic(rt):
    import torch
    from radtxfr_amd import engine
    tbl = _g4_table()
    lines = engine.LineTable(tbl)
    T, p = np.array([296.0, 250.0, 220.0]), np.array([1.0, 0.3, 0.01])
    w = np.ones((len(lines.species), 3))
    scale = 2.0 ** (-math.floor(math.log2(float(np.max(tbl["sw"])))))
    grid = engine.Grid(900.0, 1100.0, 200001)
    a = torch.empty((3, grid.n), dtype=torch.float64, device=engine.device())
    b = torch.empty_like(a)
    engine.voigt_sum(lines, grid, T, p, w, out_f64=a, scale=scale)
    engine.voigt_sum_axis(lines, grid.axis(), T, p, w, out_f64=b, scale=scale)
    for k in range(3):
        assert rel_err(b[k].cpu().numpy(), a[k].cpu().numpy()) <= 1e-6, (k, rel_err(b[k].cpu().numpy(), a[k].cpu().numpy()))
    # the fp32 output of the same call, and two calls on a non-uniform axis: identical bits
    X = _two_density(900.0, 1100.0, 1000.0, 5.0, 0.0005, 0.01)
    o1 = torch.empty((3, X.size), dtype=torch.float32, device=engine.device())
    o2 = torch.empty_like(o1)
    d1 = torch.empty((3, X.size), dtype=torch.float64, device=engine.device())
    engine.voigt_sum_axis(lines, X, T, p, w, out_f32=o1, out_f64=d1, scale=scale)
    engine.voigt_sum_axis(lines, X, T, p, w, out_f32=o2, scale=scale)
    torch.cuda.synchronize()
    assert torch.equal(o1, o2), "two axis-path calls differ"
    assert torch.equal((o1.double() / scale), d1)
    with pytest.raises(ValueError):
        engine.voigt_sum_axis(lines, X[::-1], T, p, w, out_f32=o1, scale=scale)
    lines.close()


def test_h_c_abi_argument_errors(rt):
    """Bad input comes back as a non-zero return with rtx_last_error set."""
    import torch
    from radtxfr_amd import _lib, engine
    lib = _lib.load()
    lines = engine.LineTable(_g4_table())
    plan = lines.plan(1, 4096)
    nS = len(lines.species)
    env = [np.array([296.0]), np.array([1.0]), np.ones(nS), np.ones(nS), np.full(nS, 18.0)]
    ptrs = [e.ctypes.data_as(C.c_void_p) for e in env]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def prep(X, nx=None, profile=0):
        X = np.ascontiguousarray(X, dtype=np.float64)
        return lib.rtx_line_prep_axis(plan._h, lines._h, X.ctypes.data_as(C.c_void_p), X.size if nx is None else nx, 1, *ptrs,
                                      1.0, 0.0, 0.0, 50.0, 0.0, 1.0, profile, st)

    X = np.linspace(1000.0, 1001.0, 1000)
    for bad, msg in ((X[::-1], b"non-decreasing"), (np.where(np.arange(X.size) == 5, np.nan, X), b"not finite"),
                     (np.linspace(1000.0, 1001.0, 5000), b"capacity")):
        assert prep(bad) != 0 and msg in lib.rtx_last_error(), lib.rtx_last_error()
    assert prep(X, profile=3) != 0 and b"profile" in lib.rtx_last_error()
    out = torch.empty((1, X.size), dtype=torch.float32, device=engine.device())
    grid = engine.Grid(1000.0, 1001.0, X.size)
    assert prep(X) == 0
    assert lib.rtx_voigt_sum(plan._h, grid.byref(), 1, C.c_void_p(out.data_ptr()), None, X.size, st) != 0
    assert b"rtx_voigt_sum_axis" in lib.rtx_last_error()
    assert lib.rtx_voigt_sum_axis(plan._h, 1, C.c_void_p(out.data_ptr()), None, X.size - 1, st) != 0  # ld < nx
    assert lib.rtx_voigt_sum_axis(plan._h, 1, C.c_void_p(out.data_ptr()), None, X.size, st) == 0
    engine.voigt_sum(lines, grid, [296.0], [1.0], np.ones((nS, 1)), out_f32=out)  # a grid prologue ...
    assert lib.rtx_voigt_sum_axis(plan._h, 1, C.c_void_p(out.data_ptr()), None, X.size, st) != 0  # ... is not summed on an axis
    torch.cuda.synchronize()
    lines.close()


def test_i_speed_dependent_table_on_non_uniform_grid_raises(hapi):
    tbl = dict(_g4_table())
    tbl["SD_air"] = np.full(tbl["nu"].size, 0.1)
    hapi.storage2cache_from_columns("ax_sd", tbl)
    grid = np.sort(1e4 / np.linspace(9.9, 10.1, 3000))
    with pytest.raises(NotImplementedError, match="grid"):
        hapi.absorptionCoefficient_SDVoigt(SourceTables="ax_sd", OmegaGrid=grid)
    with pytest.raises(NotImplementedError, match="grid"):
        hapi.absorptionCoefficient_SDVoigt(SourceTables="ax_sd", OmegaGrid=np.array([1000.0]))
    hapi.LOCAL_TABLE_CACHE.pop("ax_sd")
