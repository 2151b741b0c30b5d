"""What the prologue (rtx_lines.hip) takes from the layer, or from the species and the layer, alone -- log(Tref/T), the
Doppler factor, the same at the window temperatures -- what it clears before it starts (maxhw / smally / n_items) and
where grid_bisect_right puts a window edge, through every entry that launches a prologue: optical depths against the fp64
oracle point by point, in the metric and at the bound of tests/test_gpu_linesum_paths.py (pointwise_err, TOL), and bit for
bit where two routes must agree. These are the shapes at which a prologue that forms such values once per call instead of
once per (line, layer) can go wrong (profiles/prep_consts_time.txt: measured, not kept); they hold for the present one.

a. n_species * n_layers above one block's 256 threads (7 x 40, 5 x 90: both beyond the kernel-argument block, so the
   per-layer tables are the device copy), and the kernel-argument path: 4 x 32 (the flagship's shape) and one line of one
   species in one layer.
b. rtx_line_prep_window with T_win = T +- 30 K in alternate layers: strengths, widths and shifts follow T, supports T_win.
c. rtx_line_prep_mix / _axis_mix with {air: 0.7, self: 0.3} against dil_air = 0.7, dil_self = 0.3 through the plain
   entries, bit for bit (tests/test_gpu_broadening.py's contract), and against the oracle's Diluent.
d. Lorentz and Doppler (rtx_line_prep_profile; Doppler has constants of its own) on 200 points, at golden G10's bound
   (tests/test_gpu_parity.py: conftest.rel_err <= 1e-5).
e. One prep object with 32 layers, then 3, then 32, other temperatures each time: the third result is a fresh object's.
f. Two pipelines (engine.TudPipelines) fed two atmospheres so that each pipeline sees both: every step's tau, Lu, Ld are
   the single runner's for that atmosphere, bit for bit.
g. Window edges: nu +- W exactly on a grid point, lines below xmin and above the last point (reaching in, just reaching
   the end point, and not reaching), on a grid whose step is a power of two and on a tile-aligned shard (offset > 0) of a
   grid whose step is not representable: the optical depth is non-zero exactly where the oracle's bisect() puts it
   (tests/test_gpu_parity.py: test_voigt_window_edges_exact)."""
import numpy as np
import pytest

from conftest import rel_err
from oracle import cpu_ref as ref
from radtxfr_amd import synthetic

import linesum_cases as LC
import test_gpu_linesum_paths as LP

pytestmark = pytest.mark.gpu

TOL = LP.TOL
TOL_G10 = 1e-5


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    from radtxfr_amd import _lib, engine
    _lib.load()
    return engine


def _axis(g):
    """The shard's wavenumbers as the library's grid formula gives them (LP.oracle's)."""
    from radtxfr_amd import _lib
    gr = _lib.make_grid(*g)
    X = np.arange(gr.offset, gr.offset + gr.n, dtype=np.float64) * gr.step + gr.xmin
    if gr.n and gr.offset + gr.n == gr.n_total:
        X[-1] = gr.xmax
    return X


def _run(eng, lines, case):
    """LP.run for a table of several species: weight 1 for each (the oracle's natural abundances)."""
    import torch
    grid = eng.Grid(*case["grid"])
    nL = case["T"].size
    o32 = torch.full((nL, grid.n), float("nan"), dtype=torch.float32, device="cuda")
    o64 = torch.full((nL, grid.n), float("nan"), dtype=torch.float64, device="cuda")
    eng.voigt_sum(lines, grid, case["T"], case["p"], np.ones((len(lines.species), nL)), out_f32=o32, out_f64=o64,
                  omega_wing=case["ow"], omega_wing_hw=case["hw"])
    torch.cuda.synchronize()
    return o32.double().cpu().numpy(), o64.cpu().numpy()


def _with_species(tbl, species):
    n = tbl["nu"].size
    tbl["molec_id"] = np.array([species[i % len(species)][0] for i in range(n)], dtype=np.int64)
    tbl["local_iso_id"] = np.array([species[i % len(species)][1] for i in range(n)], dtype=np.int64)
    return tbl


# ------------------------------------------------------------------------------------ a. species x layers, both table paths
SPECIES7 = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (5, 1), (6, 1)]
SHAPES = {"7x40": (SPECIES7, 40, 14), "5x90": (SPECIES7[:5], 90, 10), "4x32": (SPECIES7[:4], 32, 8), "1x1": (SPECIES7[:1], 1, 1)}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_layer_constants_vs_oracle(eng, shape):
    """Every (species, layer) pair has a line on the grid: a per-(species, layer) value missed, or taken from another
    pair's slot, shows in that layer's row. Temperatures and pressures differ from layer to layer (200 ... 300 K, 1 ... 1e-3 atm:
    plain and y < 1 layers)."""
    species, nL, n_lines = SHAPES[shape]
    g = LC.grid(1000.0, 1e-3, 1100)
    nu = np.linspace(999.8, 1001.3, n_lines) + 2.5e-4 if n_lines > 1 else np.array([1000.40025])
    tbl = _with_species(LC.table(nu, np.linspace(0.03, 0.11, n_lines)), species)
    k = np.arange(nL)
    T = 200.0 + 100.0 * ((k * 7) % nL) / max(nL - 1, 1) if nL > 1 else np.array([251.0])
    p = 10.0 ** np.linspace(0.0, -3.0, nL) if nL > 1 else np.array([0.3])
    case = LC._case(tbl, g, T, p)
    lines = eng.LineTable(tbl)
    assert len(lines.species) == len(species)
    nS = len(species)
    assert (2 * nL + 2 * nS * nL + nS <= 416) == (shape in ("4x32", "1x1"))  # RTX_ENV_MAX: which table path the case takes
    want = LP.oracle("prep_consts_" + shape, case)
    r32, r64 = _run(eng, lines, case)
    lines.close()
    e32, e64 = LP.pointwise_err(r32, want), LP.pointwise_err(r64, want)
    print("prep_consts %s: f32 %.3g f64 %.3g" % (shape, e32, e64))
    assert want.max(axis=1).min() > 0.0
    assert e32 <= TOL and e64 <= TOL, (shape, e32, e64)


# ------------------------------------------------------------------------------------------------- b. the window prologue
def test_window_prologue_strengths_at_T_windows_at_Twin(eng):
    """Expected, line by line: the oracle's cross section at T with the wing cutoff lifted (OmegaWing = 5 cm^-1, wider than
    any window here), kept on the support of the oracle's cross section at T_win. H2O and CO2 lines (two Doppler
    factors); T_win = T - 30 K widens a pressure-broadened window ((Tref/T)^n), T + 30 K narrows it."""
    import torch
    g = LC.grid(1000.0, 1e-3, 3000)
    nu = np.array([1000.30025, 1000.90025, 1001.50025, 1002.10025, 1002.60025])
    tbl = _with_species(LC.table(nu, [0.011, 0.009, 0.012, 0.008, 0.010]), [(1, 1), (2, 1)])
    T = np.array([296.0, 260.0, 230.0, 285.0, 215.0, 250.0])
    T_win = T + 30.0 * np.where(np.arange(T.size) % 2 == 0, 1.0, -1.0)
    p = np.array([1.0, 0.8, 0.6, 0.9, 0.5, 0.7])
    X = _axis(g)
    want = np.zeros((T.size, X.size))
    moved = 0
    for r in range(nu.size):
        one = {k: v[r:r + 1] for k, v in tbl.items()}
        for k in range(T.size):
            full = ref.absorptionCoefficient_Voigt(one, T=float(T[k]), p=float(p[k]), OmegaGrid=X, OmegaWing=5.0)[1]
            at_T = ref.absorptionCoefficient_Voigt(one, T=float(T[k]), p=float(p[k]), OmegaGrid=X)[1] != 0
            at_win = ref.absorptionCoefficient_Voigt(one, T=float(T_win[k]), p=float(p[k]), OmegaGrid=X)[1] != 0
            moved += int(np.count_nonzero(at_T != at_win) > 0)
            want[k] += np.where(at_win, full, 0.0)
    assert moved == nu.size * T.size  # every window differs from the one at T
    lines = eng.LineTable(tbl)
    grid = eng.Grid(*g)
    out = torch.full((T.size, grid.n), float("nan"), dtype=torch.float32, device="cuda")
    eng.voigt_sum_window(lines, grid, T, T_win, p, np.ones((len(lines.species), T.size)), out)
    torch.cuda.synchronize()
    got = out.double().cpu().numpy()
    lines.close()
    e = LP.pointwise_err(got, want)
    print("prep_consts window: %.3g" % e)
    assert e <= TOL, e


# -------------------------------------------------------------------------------------------------- c. the mixed prologue
def _mix_table():
    tbl = synthetic.synth_line_table(13, 60, 999.5, 1001.5)
    rng = np.random.default_rng(6)
    tbl["n_self"] = np.round(rng.uniform(0.5, 0.9, 60), 2)
    tbl["n_self"][::4] = 0.0
    tbl["delta_self"] = np.round(rng.uniform(-0.02, 0.01, 60), 6)
    return tbl


def test_mix_prologue_equals_plain_prologue(eng):
    import torch
    tbl = _mix_table()
    lines = eng.LineTable(tbl)
    nS = len(lines.species)
    T, p = np.array([296.0, 250.0, 220.0]), np.array([1.0, 0.5, 0.02])
    w = np.ones((nS, 3))
    dil = {"air": 0.7, "self": 0.3}
    g = LC.grid(1000.0, 1e-3, 1100)
    grid = eng.Grid(*g)
    X_uniform = _axis(g)
    X_axis = np.sort(np.concatenate([np.linspace(1000.0, 1001.1, 700), np.random.default_rng(7).uniform(1000.2, 1000.9, 300)]))
    outs = {}
    for route, kw in (("plain", dict(dil_air=0.7, dil_self=0.3)), ("mix", dict(diluent=dil))):
        o32 = torch.full((3, grid.n), float("nan"), dtype=torch.float32, device="cuda")
        o64 = torch.full((3, grid.n), float("nan"), dtype=torch.float64, device="cuda")
        eng.voigt_sum(lines, grid, T, p, w, out_f32=o32, out_f64=o64, **kw)
        a32 = torch.full((3, X_axis.size), float("nan"), dtype=torch.float32, device="cuda")
        a64 = torch.full((3, X_axis.size), float("nan"), dtype=torch.float64, device="cuda")
        eng.voigt_sum_axis(lines, X_axis, T, p, w, out_f32=a32, out_f64=a64, **kw)
        torch.cuda.synchronize()
        outs[route] = [t.cpu().numpy() for t in (o32, o64, a32, a64)]
    lines.close()
    for a, b in zip(outs["plain"], outs["mix"]):
        assert np.array_equal(a, b)
    for got, X in ((outs["mix"][1], X_uniform), (outs["mix"][3], X_axis)):
        want = np.stack([ref.absorptionCoefficient_Voigt(tbl, T=float(Tk), p=float(pk), OmegaGrid=X, Diluent=dil)[1]
                         for Tk, pk in zip(T, p)])
        e = LP.pointwise_err(got, want)
        print("prep_consts mix: %.3g" % e)
        assert want.max() > 0.0 and e <= TOL, e


# ------------------------------------------------------------------------------------------------------------ d. profiles
def test_lorentz_and_doppler_profiles(eng):
    import torch
    tbl = synthetic.synth_line_table(21, 30, 999.9, 1000.3)
    lines = eng.LineTable(tbl)
    nS = len(lines.species)
    assert nS >= 3  # several masses: the Doppler profile's sqrt(mass) per species
    T, p = np.array([296.0, 220.0]), np.array([1.0, 0.05])
    for profile, fn, (lo, hi) in ((1, ref.absorptionCoefficient_Lorentz, (999.9, 1000.3)),
                                  (2, ref.absorptionCoefficient_Doppler, (1000.0, 1000.04))):
        g = LC.grid(lo, (hi - lo) / 199, 200)
        grid = eng.Grid(*g)
        X = _axis(g)
        o64 = torch.full((2, grid.n), float("nan"), dtype=torch.float64, device="cuda")
        eng.voigt_sum(lines, grid, T, p, np.ones((nS, 2)), out_f64=o64, profile=profile)
        torch.cuda.synchronize()
        got = o64.cpu().numpy()
        for k in range(2):
            want = fn(tbl, T=float(T[k]), p=float(p[k]), OmegaGrid=X)[1]
            e = rel_err(got[k], want)
            print("prep_consts profile %d layer %d: %.3g" % (profile, k, e))
            assert want.max() > 0.0 and e <= TOL_G10, (profile, k, e)
    lines.close()


# ----------------------------------------------------------------------------------- e. stale state and cleared flags
def test_prep_object_reused_across_layer_counts(eng):
    """32 layers (the first of them with y < 1 lines: smally set), then 3 plain layers, then 32 again, on one prep object;
    the second and third calls must not see the first's per-layer values, maxima or flags."""
    import torch
    g = LC.grid(1000.0, 1e-3, 2100)
    tbl = _with_species(LC.table(np.linspace(999.7, 1002.3, 12) + 2.5e-4, np.linspace(0.03, 0.11, 12)), [(1, 1), (2, 1), (2, 2)])
    k = np.arange(32)
    calls = [(210.0 + 2.5 * k, 10.0 ** np.linspace(-3.5, 0.0, 32)),
             (np.array([300.0, 280.0, 296.0]), np.array([1.0, 0.7, 0.4])),
             (290.0 - 2.0 * k, 10.0 ** np.linspace(0.0, -3.0, 32))]

    def sums(lines, which):
        res = []
        grid = eng.Grid(*g)
        for i in which:
            T, p = calls[i]
            o = torch.full((T.size, grid.n), float("nan"), dtype=torch.float32, device="cuda")
            eng.voigt_sum(lines, grid, T, p, np.ones((len(lines.species), T.size)), out_f32=o)
            res.append(o)
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in res]

    lines = eng.LineTable(tbl)
    plan = lines.plan(32, g[4])
    reused = sums(lines, (0, 1, 2))
    assert lines.plan(3, g[4]) is plan  # one prep object throughout
    lines.close()
    for i in (1, 2):
        fresh_lines = eng.LineTable(tbl)
        fresh = sums(fresh_lines, (i,))[0]
        fresh_lines.close()
        assert fresh.max() > 0.0 and np.array_equal(reused[i], fresh), i
    case = LC._case(tbl, g, *calls[2])
    assert LP.pointwise_err(reused[2], LP.oracle("prep_consts_reuse", case)) <= TOL


# ------------------------------------------------------------------------------------------------------- f. pipelines
def test_two_pipelines_two_atmospheres(eng):
    """Steps A B B A A B on two pipelines: pipeline 0 runs A B A, pipeline 1 runs B A B, nothing waits in between (each
    step's outputs are copied on its own stream). Each pipeline's prep object holds its own per-call state."""
    import torch
    full = synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)
    lo, hi = 1000.0, 1004.0
    sub = synthetic.subset_table(full, lo - 12.0, hi + 12.0)
    a = synthetic.c3_atmosphere(32)
    a["MFs_VAL"] = a["MFs_VAL"] * 1e-3
    b = dict(a, Ts=a["Ts"] + 7.0, MFs_VAL=a["MFs_VAL"] * 1.5)
    lines = eng.LineTable(sub)
    grid = eng.Grid(lo, hi, 4001)
    args = lambda m: (m["Ts"], m["Ps"], m["PLs"], m["MFs_VAL"], m["MFs_ID"])
    single = {}
    for tag, m in (("a", a), ("b", b)):
        runner = eng.TudRunner(lines, grid, a["Zs"], plan=eng.VoigtPlan(lines, 32, grid.n))
        single[tag] = [t.cpu().numpy().copy() for t in runner.run(*args(m))]
        runner.plan.close()
    assert not np.array_equal(single["a"][0], single["b"][0])
    pipes = eng.TudPipelines(lines, grid, a["Zs"], n_pipes=2)
    order = "abbaab"
    got = []
    try:
        for tag in order:
            pi, out = pipes.run(*args(a if tag == "a" else b))
            with torch.cuda.stream(pipes.streams[pi]):
                got.append([t.clone() for t in out])
        torch.cuda.synchronize()
        for step, (tag, res) in enumerate(zip(order, got)):
            for x, y in zip(res, single[tag]):
                assert np.array_equal(x.cpu().numpy(), y), (step, tag)
    finally:
        pipes.close()
        lines.close()


# ---------------------------------------------------------------------------------------------------- g. window edges
def _edge_lines(X, step, n_total, xmin, W):
    """Centres whose nu -+ W is a grid point (as fp64 forms it), one ulp to either side of it, and centres outside the
    grid: reaching in, reaching exactly the first / last point, and not reaching."""
    xs = []
    for i in (X.size // 3, X.size // 2, X.size - 5):
        for d in (0.0, 1.0, -1.0):
            xs.append(np.nextafter(X[i] + W, X[i] + W + d))  # lower edge on X[i]
            xs.append(np.nextafter(X[i] - W, X[i] - W + d))  # upper edge on X[i]
    x_first, x_last = xmin, xmin + (n_total - 1) * step
    xs += [x_first - 0.5 * W, x_first - W, np.nextafter(x_first - W, 0.0), x_first - W - 3.25 * step, x_first - 2.0 * W]
    xs += [x_last + 0.5 * W, x_last + W, np.nextafter(x_last + W, 1e9), x_last + W + 3.25 * step, x_last + 2.0 * W]
    xs += [X[0] - W, X[0] + W, X[-1] - W, X[-1] + W]  # the shard's own end points
    return np.array(xs)


@pytest.mark.parametrize("which", ["pow2_step", "shard_inexact_step"])
def test_window_edges_on_grid_points(eng, which):
    """OmegaWing = 0.25 cm^-1 sets every window (OmegaWingHW = 1, Gamma0 = 0.07). One line at a time, so that a support is
    one line's window."""
    from radtxfr_amd import _lib
    tp = int(_lib.load().rtx_voigt_tile_points())
    W = 0.25
    if which == "pow2_step":
        step, n_total = 2.0 ** -10, 2049
        g = LC.grid(1000.0, step, n_total)
    else:
        step, n_total = 1e-3, 2 * tp + 601
        g = LC.grid(1000.0, step, n_total, offset=tp, n=tp + 577)
    X = _axis(g)
    nus = _edge_lines(X, (g[1] - g[0]) / (g[2] - 1), n_total, g[0], W)
    worst, n_empty = 0.0, 0
    for r, nu in enumerate(nus):
        case = LC._case(LC.table([nu]), g, 296.0, 1.0, ow=W, hw=1.0)
        want = LP.oracle("prep_consts_edge_%s_%d" % (which, r), case)
        r32, r64 = LP.run(eng, case)
        assert np.array_equal(r64 != 0, want != 0), (which, r, nu)
        assert np.array_equal(r32 != 0, want != 0), (which, r, nu)
        worst = max(worst, LP.pointwise_err(r64, want))
        n_empty += int(not want.any())
    print("prep_consts edges %s: %.3g, %d of %d lines outside" % (which, worst, n_empty, nus.size))
    assert 0 < n_empty < nus.size  # both kinds are present
    assert worst <= TOL
