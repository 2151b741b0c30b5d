"""GPU: the grow-only scratch buffers and the table caches behind the C ABI ("Device memory"), reached on
purpose: every case runs a sequence of calls on ONE long-lived object -- a line table with its plan, a cross-section
table, the process-wide tap caches and ILS workspaces -- that makes a buffer grow, be reused at a smaller size, or be
evicted, and every result must be bit-identical to the same call on a fresh object. No case provokes an error on the
device; the failure paths are tests/test_devmem_host.py's.

Shapes: ~300 lines over 10 cm^-1, 2 layers, grids and axes of at most 3 line-sum tiles (1024 points each)."""
import numpy as np
import pytest
import torch

import linesum_cases

pytestmark = pytest.mark.gpu

SCALE = 2.0 ** 70  # cross sections of 1e-20 as fp32 normals
T2, P2 = np.array([296.0, 240.0]), np.array([1.0, 0.4])


@pytest.fixture(scope="module")
def mods():
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    from radtxfr_amd import _lib, afit_xs, engine, synthetic
    lib = _lib.load()
    assert int(lib.rtx_voigt_tile_points()) == 1024
    return dict(lib=lib, afit_xs=afit_xs, engine=engine, synthetic=synthetic)


def _columns(mods):
    """~300 lines over 10 cm^-1 with every optional column a case needs: self, h2 and speed-dependence sets."""
    n = 300
    tbl = mods["synthetic"].synth_line_table(31, n, 995.0, 1005.0)
    rng = np.random.default_rng(32)
    tbl["n_self"] = np.round(rng.uniform(0.5, 0.9, n), 2)
    tbl["delta_self"] = np.round(rng.uniform(-0.02, 0.01, n), 6)
    tbl["gamma_h2"] = np.round(rng.uniform(0.05, 0.3, n), 4)
    tbl["n_h2"] = np.round(rng.uniform(0.2, 0.6, n), 2)
    tbl["SD_air"] = np.round(rng.uniform(0.05, 0.2, n), 4)
    tbl["SD_self"] = np.round(rng.uniform(0.0, 0.1, n), 4)
    return tbl


def _run_sequence(mods, columns, calls, plan=None):
    """calls: functions (engine, table) -> device tensor. All of them in order on one table (its plan made first, for
    `plan` = (n_layers, n_points)), and each of them alone on a table of its own: the pairs (reused, fresh) on the host."""
    engine = mods["engine"]
    lt = engine.LineTable(columns)
    if plan:
        held = lt.plan(*plan)
    reused = [c(engine, lt).cpu() for c in calls]
    if plan:
        assert lt.plan(*plan) is held  # one prep object took the whole sequence
    lt.close()
    fresh = []
    for c in calls:
        lt1 = engine.LineTable(columns)
        fresh.append(c(engine, lt1).cpu())
        lt1.close()
    return list(zip(reused, fresh))


def _assert_same(pairs):
    for i, (a, b) in enumerate(pairs):
        assert a.shape == b.shape and torch.equal(a, b), "call %d of the sequence differs from a fresh object's" % i
        assert torch.isfinite(a).all() and float(a.max()) > 0.0, i


def test_axis_scratch(mods):
    """The device copy of an explicit axis: 300, then 3000, then 300 points on one plan."""
    rng = np.random.default_rng(33)
    X_long = np.sort(np.concatenate([np.linspace(998.0, 1002.0, 2200), rng.uniform(999.0, 1001.0, 800)]))
    X_short = np.sort(rng.uniform(999.5, 1000.5, 300))

    def call(X):
        def f(engine, lt):
            w = np.ones((len(lt.species), 2))
            out = torch.empty((2, X.size), dtype=torch.float32, device=engine.device())
            engine.voigt_sum_axis(lt, X, T2, P2, w, out_f32=out, scale=SCALE)
            return out
        return f

    _assert_same(_run_sequence(mods, _columns(mods), [call(X_short), call(X_long), call(X_short)], plan=(2, 3000)))


def test_mix_scratch(mods):
    """The diluent fractions: one diluent, three with per-layer fractions, one again."""
    grid_args = (998.0, 1002.0, 3000)

    def call(diluent):
        def f(engine, lt):
            nS = len(lt.species)
            grid = engine.Grid(*grid_args)
            out = torch.empty((2, grid.n), dtype=torch.float32, device=engine.device())
            dil = {k: np.tile(np.asarray(v, dtype=np.float64), (nS, 1)) if np.ndim(v) else v for k, v in diluent.items()}
            engine.voigt_sum(lt, grid, T2, P2, np.ones((nS, 2)), out_f32=out, scale=SCALE, diluent=dil)
            return out
        return f

    one = {"air": 1.0}
    three = {"air": [0.6, 0.2], "self": [0.1, 0.5], "h2": [0.3, 0.3]}
    _assert_same(_run_sequence(mods, _columns(mods), [call(one), call(three), call(one)], plan=(2, 3000)))


def test_window_scratch(mods):
    """The window temperatures: rtx_line_prep_window before and after an ordinary prologue on the same plan."""
    grid_args = (998.0, 1002.0, 3000)
    T_win = np.array([310.0, 225.0])

    def window(engine, lt):
        grid = engine.Grid(*grid_args)
        out = torch.empty((2, grid.n), dtype=torch.float32, device=engine.device())
        return engine.voigt_sum_window(lt, grid, T2, T_win, P2, np.ones((len(lt.species), 2)), out)

    def plain(engine, lt):
        grid = engine.Grid(*grid_args)
        out = torch.empty((2, grid.n), dtype=torch.float32, device=engine.device())
        engine.voigt_sum(lt, grid, T2, P2, np.ones((len(lt.species), 2)), out_f32=out)
        return out

    pairs = _run_sequence(mods, _columns(mods), [window, plain, window], plan=(2, 3000))
    for a, b in pairs:  # unscaled cross sections: tiny but non-zero fp32
        assert torch.equal(a, b) and float(a.max()) > 0.0
    assert not torch.equal(pairs[0][0], pairs[1][0])  # T_win != T moved some window edge


def test_lazy_sd_records(mods):
    """The speed-dependent records, allocated by the first profile-3 prologue: profile 3, 0, 3 on one plan."""
    grid_args = (999.0, 1001.0, 2500)

    def call(profile):
        def f(engine, lt):
            grid = engine.Grid(*grid_args)
            out = torch.empty((2, grid.n), dtype=torch.float64, device=engine.device())
            engine.voigt_sum(lt, grid, T2, P2, np.ones((len(lt.species), 2)), out_f64=out, scale=SCALE, profile=profile,
                             dil_air=0.8, dil_self=0.2)
            return out
        return f

    pairs = _run_sequence(mods, _columns(mods), [call(3), call(0), call(3)], plan=(2, 2500))
    _assert_same(pairs)
    assert not torch.equal(pairs[0][0], pairs[1][0])


def test_hot_tile_work_list(mods):
    """The work list of hot-tile parts: 1000 lines inside 0.5 cm^-1 (over RTX_SPLIT_MIN = 768 candidates in a tile) under
    windows of 0.3 cm^-1. On a 1e-3 grid the cluster lies in the middle tile of three and only that tile is cut; on a
    4e-4 grid it spans the first two tiles and both are cut, so the list grows; then the first grid again."""
    lib = mods["lib"]
    tbl = linesum_cases.table(1001.2 + 0.5 * (np.arange(1000) + 0.37) / 1000.0)
    T, p = np.array([296.0, 250.0]), np.array([0.05, 0.02])
    coarse, fine = (1000.0, 1000.0 + 3071 * 1e-3, 3072), (1001.0, 1001.0 + 3071 * 4e-4, 3072)
    assert 1000.0 + 1024e-3 < 1001.2 and 1001.7 < 1000.0 + 2048e-3          # coarse: all of it inside tile 1
    assert 1001.2 < 1001.0 + 1024 * 4e-4 < 1001.7 < 1001.0 + 2048 * 4e-4    # fine: astride tiles 0 and 1
    bounds = []

    def call(g, record):
        def f(engine, lt):
            grid = engine.Grid(*g)
            out = torch.empty((2, grid.n), dtype=torch.float32, device=engine.device())
            engine.voigt_sum(lt, grid, T, p, np.ones((len(lt.species), 2)), out_f32=out, omega_wing=0.3, scale=SCALE)
            if record:
                bounds.append(int(lib.rtx_prep_split_bound(lt.plan(2, grid.n)._h)))
            return out
        return f

    engine = mods["engine"]
    lt = engine.LineTable(tbl)
    reused = [call(g, True)(engine, lt).cpu() for g in (coarse, fine, coarse)]
    lt.close()
    print("split bounds on the coarse, fine, coarse grid:", bounds)
    assert all(b > 0 for b in bounds) and bounds[1] > bounds[0] and bounds[2] == bounds[0]
    fresh = []
    for g in (coarse, fine):
        lt1 = engine.LineTable(tbl)
        fresh.append(call(g, False)(engine, lt1).cpu())
        lt1.close()
    _assert_same(list(zip(reused, fresh + fresh[:1])))


def test_tap_caches(mods):
    """More distinct filters than a cache holds -- 17 slits through rtx_fir_same's 16 entries, 65 windows through
    rtx_fir_reflect's 64 -- then the first again, by now evicted and uploaded anew: the same result."""
    engine = mods["engine"]
    rng = np.random.default_rng(34)
    row = torch.as_tensor(rng.uniform(0.5, 2.0, (1, 256)), device=engine.device())
    slits = rng.uniform(0.1, 1.0, (17, 5))
    first, n_out = engine.same_window(256, 5)
    outs = [engine.fir_same(row, s, 0.5, first, n_out).cpu() for s in slits]
    assert torch.equal(engine.fir_same(row, slits[0], 0.5, first, n_out).cpu(), outs[0])
    assert torch.equal(engine.fir_same(row, slits[16], 0.5, first, n_out).cpu(), outs[16])  # a hit
    assert not torch.equal(outs[0], outs[1])
    want = np.convolve(row.cpu().numpy()[0], slits[0], mode="same") * 0.5
    assert np.allclose(outs[0].numpy()[0], want, rtol=1e-13, atol=0.0)

    row = torch.as_tensor(rng.uniform(0.5, 2.0, (1, 64)), device=engine.device())
    wins = rng.uniform(0.1, 1.0, (65, 3))
    outs = [engine.fir_reflect(row, w, 1).cpu() for w in wins]
    assert torch.equal(engine.fir_reflect(row, wins[0], 1).cpu(), outs[0])
    assert torch.equal(engine.fir_reflect(row, wins[64], 1).cpu(), outs[64])
    assert not torch.equal(outs[0], outs[1])
    x = row.cpu().numpy()[0]
    assert np.allclose(outs[0].numpy()[0, 1:-1], wins[0, 0] * x[:-2] + wins[0, 1] * x[1:-1] + wins[0, 2] * x[2:], rtol=1e-13, atol=0.0)


def test_ils_workspace(mods):
    """The one-pass ILS keeps a workspace per (device, stream): a call on each of two streams, then a larger one on the
    first, each equal to the same call on the current stream alone."""
    engine = mods["engine"]
    dev = engine.device()
    nS, nB = 256, 32  # nx * nS >= 3e7 and nx >= 2048 nB take the one-pass rows form

    def inputs(nx, seed):
        gen = torch.Generator(device=dev).manual_seed(seed)
        Y = torch.rand((nx, nS), dtype=torch.float32, device=dev, generator=gen) + 0.5
        grid = engine.Grid(700.0, 1400.0, nx)
        centre = torch.linspace(720.0, 1380.0, nB, dtype=torch.float64, device=dev)
        sigma = torch.full((nB,), 1.6 * 660.0 / (nB - 1), dtype=torch.float64, device=dev)
        return Y, grid, centre, sigma

    def ils(args):
        Y, grid, centre, sigma = args
        return engine.ils(0, Y, centre, sigma, grid=grid)

    small, large = inputs(120000, 1), inputs(150000, 2)
    ref_small, ref_large = ils(small), ils(large)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        a = ils(small)
    with torch.cuda.stream(s2):
        b = ils(small)
    with torch.cuda.stream(s1):
        c = ils(large)
    torch.cuda.synchronize()
    assert torch.equal(a, ref_small) and torch.equal(b, ref_small) and torch.equal(c, ref_large)
    assert torch.isfinite(ref_small).all() and float(ref_small.min()) > 0.5 and not torch.equal(ref_small, ref_large[:, :nS])


def test_xs_od_terms(mods):
    """The per-stream terms of rtx_xs_od: 1 layer, 3 layers, 1 layer on one table and one stream."""
    engine, afit_xs = mods["engine"], mods["afit_xs"]
    nX = 1024
    rng = np.random.default_rng(35)
    X = np.linspace(2000.0, 2000.0 + 0.01 * (nX - 1), nX)
    entries = [dict(ID=ID, T=np.array([250.0, 300.0]), P_atm=np.array([0.5]), X=X, xs=10.0 ** rng.uniform(-24.0, -19.0, (2, 1, nX)))
               for ID in (1, 2)]  # 2 molecules, 4 rows
    T3, p3, PL3 = np.array([260.0, 281.3, 299.0]), np.array([0.5, 0.5, 0.5]), np.array([1.0, 0.5, 2.0])
    MF3, ID = rng.uniform(1.0, 2e4, (3, 2)), np.array([1, 2])

    def od(lut, k):
        return engine.xs_od(lut, 0, T3[:k], p3[:k], PL3[:k], MF3[:k], ID, out_f32=torch.empty((k, nX), dtype=torch.float32, device="cuda")).cpu()

    lut = afit_xs.XsLut.from_grids(entries)
    reused = [od(lut, k) for k in (1, 3, 1)]
    lut.free()
    fresh = []
    for k in (1, 3):
        lut1 = afit_xs.XsLut.from_grids(entries)
        fresh.append(od(lut1, k))
        lut1.free()
    _assert_same(list(zip(reused, fresh + fresh[:1])))
