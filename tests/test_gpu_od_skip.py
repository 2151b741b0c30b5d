"""rtx_compute_tud_opts(RTX_CTUD_OD_SCRATCH): the optical depths the TUD pass never reads are not summed (rtx_tud.hip,
rtx_voigt_scatter.hip; engine.TudRunner's keep_od).

The pass runs as line-sum A (layers [0, 4) and [k_top - 8, nL)) -> TUD early -> line-sum B (the layers in between, without the
rows of the 64-point waves that early finished) -> TUD late. What must hold: tau, L-up and L-down are the bits of the plain
order (keep_od=True); an optical depth is left unwritten exactly where a wave was done, in the layers of B; a wave that
skips but has to sum middle chunks still finds them; nothing stale is ever read; and every call that is not eligible leaves
OD complete.

Which waves are done does not show in the outputs, so every case first restates the kernel's decisions in NumPy
(tools/count_tud_layers.census, on the complete float32 optical depths of the keep_od=True run) and checks that the case
shows what it is there for: the "opaque" column (the CO2 15 um band core, 667 cm^-1, full mixing ratios) has a line-sum tile
whose 16 rows are all done, the "mixed" one (1000 cm^-1: the done waves end inside a tile) a tile with some but not all
rows done, the "thin" one (mixing ratios x 1e-3) none. Grids of two tiles and a ragged third: n = 2 * 1024 + 100, the last
wave ragged too. The windows were chosen with the same census on the oracle's optical depths."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cpu_ref as ref
from radtxfr_amd import synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import count_tud_layers as ctl  # noqa: E402

TILE, ROWS = 1024, 16
N = 2 * TILE + 100
STEP = 0.001
STAGE, SCAN, BOTTOM = 4, 12, 4  # TUD_STAGE, TUD_SKIP_SCAN, TUD_SKIP_BOTTOM
COLUMNS = {"opaque": (667.0, 1.0), "mixed": (1000.0, 1.0), "thin": (667.0, 1e-3)}  # window start [cm^-1], mixing-ratio scale


@functools.lru_cache(maxsize=None)
def _full_table():
    return synthetic.synth_line_table(synthetic.SEED_C3, 100000, 475.0, 6025.0)


def _table(lo):
    return synthetic.subset_table(_full_table(), lo - 12.0, lo + STEP * (N - 1) + 12.0)


def _atmosphere(nL, scale=1.0, mid=1.0):
    a = synthetic.c3_atmosphere(nL)
    mf = a["MFs_VAL"] * scale
    mf[BOTTOM:_mid_hi(nL)] *= mid
    return dict(T=a["Ts"], P=a["Ps"], PL=a["PLs"], MF=mf, ID=a["MFs_ID"], Z=a["Zs"])


def _mid_hi(cnt0):
    """Layers [BOTTOM, _mid_hi) are launch B's: below the lowest layer the look at the top can read."""
    return ((cnt0 - 1) // STAGE) * STAGE - (SCAN - STAGE)


def _census(OD, X, T):
    """The kernel's decisions per 64-point wave on OD [nL][n] float32 (ragged last wave: dead lanes shadow the last point):
    done = the wave skips and sums no middle chunk."""
    nL, n = OD.shape
    pad = (-n) % 64
    od = np.concatenate([OD.T, np.repeat(OD.T[-1:], pad, axis=0)])
    B = ref.planckian(X, np.asarray(T, dtype=np.float64))
    B = np.concatenate([B, np.repeat(B[-1:], pad, axis=0)])
    ctl.NL = nL
    c = ctl.census(np.ascontiguousarray(od), B, nL, nL, SCAN, BOTTOM)
    return dict(done=c["skip"] & (c["summed"] == 0), skip=c["skip"], summed=c["summed"])


def _tiles(done):
    """Done rows per tile and rows the tile has on the grid."""
    return [(int(done[i:i + ROWS].sum()), int(done[i:i + ROWS].size)) for i in range(0, done.size, ROWS)]


def _runner_pair(engine, lines, grid, a, nL, **kw):
    """(complete, scratch): the keep_od=True run (the plain order) and the run of a runner-owned, NaN-poisoned OD buffer."""
    import torch
    out = []
    for keep in (True, None):
        run = engine.TudRunner(lines, grid, a["Z"], n_layers=nL, keep_od=keep, **kw)
        run.OD.fill_(float("nan"))
        tau, Lu, Ld = run.run(a["T"], a["P"], a["PL"], a["MF"], a["ID"])
        torch.cuda.synchronize()
        out.append(dict(tau=tau.clone(), Lu=Lu.clone(), Ld=Ld.clone(), OD=run.OD.clone()))
    return out


@functools.lru_cache(maxsize=None)
def _case(column, nL, mid=1.0):
    import torch
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    from radtxfr_amd import engine
    lo, scale = COLUMNS[column]
    a = _atmosphere(nL, scale, mid)
    lines = engine.LineTable(_table(lo))
    grid = engine.Grid(lo, lo + STEP * (N - 1), N)
    full, scr = _runner_pair(engine, lines, grid, a, nL)
    lines.close()
    c = _census(full["OD"].cpu().numpy(), grid.axis(), a["T"])
    return dict(full=full, scr=scr, census=c, a=a, grid=grid)


def _assert_shows(column, c):
    t = _tiles(c["done"])
    if column == "opaque":
        assert any(d == ROWS for d, _ in t), t
    elif column == "mixed":
        assert any(0 < d < r for d, r in t), t
    else:
        assert not c["done"].any() and not c["skip"].any(), t


@pytest.mark.parametrize("column", list(COLUMNS))
@pytest.mark.parametrize("nL", [24, 28, 32, 33])
def test_outputs_keep_their_bits(nL, column):
    """1: tau, L-up, L-down of the scratch-OD runner equal those of keep_od=True bit for bit."""
    import torch
    k = _case(column, nL)
    _assert_shows(column, k["census"])
    assert bool(torch.isfinite(k["full"]["OD"]).all()), "keep_od=True left optical depths unwritten"
    for name in ("tau", "Lu", "Ld"):
        assert torch.equal(k["scr"][name], k["full"][name]), name


@pytest.mark.parametrize("column", list(COLUMNS))
@pytest.mark.parametrize("nL", [24, 28, 32, 33])
def test_never_read_never_written(nL, column):
    """2: on a NaN-filled buffer the outputs are finite, every optical depth that was written is the complete run's, and the
    entries left alone are exactly {done rows} x {layers of launch B}."""
    import torch
    k = _case(column, nL)
    _assert_shows(column, k["census"])
    for name in ("tau", "Lu", "Ld"):
        assert bool(torch.isfinite(k["scr"][name]).all()), name
    od, want = k["scr"]["OD"].cpu().numpy(), k["full"]["OD"].cpu().numpy()
    nan = np.isnan(od)
    assert np.array_equal(od[~nan].view(np.uint32), want[~nan].view(np.uint32))
    expect = np.zeros_like(nan)
    rows = np.repeat(k["census"]["done"], 64)[:N]
    expect[BOTTOM:_mid_hi(nL), :] = rows[None, :]
    print("%s, %d layers: done rows per tile %s, %d of %d entries unwritten" % (column, nL, _tiles(k["census"]["done"]), nan.sum(), nan.size))
    assert np.array_equal(nan, expect), "unwritten: %d, expected %d, differing %d" % (nan.sum(), expect.sum(), (nan != expect).sum())


def test_skip_that_sums_middle_chunks_finds_them():
    """3: bottom + top stay below TUD_SKIP_TAU0 while the top is opaque (only the middle layers' mixing ratios are scaled, which
    no decision of the early launch sees): such waves skip, sum middle chunks, are not done, and their OD is complete."""
    import torch
    k = _case("mixed", 32, mid=5.0)
    c = k["census"]
    summing = c["skip"] & (c["summed"] > 0)
    assert summing.sum() >= 4 and not (summing & c["done"]).any(), (summing.sum(), c["done"].sum())
    plain = _case("mixed", 32)["census"]
    assert np.array_equal(c["done"], plain["done"]), "the middle layers changed a decision of the early launch"
    lanes = np.repeat(summing, 64)[:N]
    od, want = k["scr"]["OD"].cpu().numpy(), k["full"]["OD"].cpu().numpy()
    assert np.array_equal(od[:, lanes].view(np.uint32), want[:, lanes].view(np.uint32))
    for name in ("tau", "Lu", "Ld"):
        assert torch.equal(k["scr"][name], k["full"][name]), name


def test_stale_flags_and_depths_are_not_reused():
    """4: one runner alternates opaque and thin atmospheres (its done flags and its OD buffer go stale in between), and two
    pipelines sharing nothing do the same: every result equals a fresh runner's."""
    import torch
    from radtxfr_amd import engine
    lo = COLUMNS["opaque"][0]
    lines = engine.LineTable(_table(lo))
    grid = engine.Grid(lo, lo + STEP * (N - 1), N)
    atms = [_atmosphere(32, s) for s in (1.0, 1e-3, 0.3, 1e-3, 1.0)]
    want = []
    for a in atms:
        run = engine.TudRunner(lines, grid, a["Z"], n_layers=32, keep_od=True)
        want.append([t.clone() for t in run.run(a["T"], a["P"], a["PL"], a["MF"], a["ID"])])
    torch.cuda.synchronize()
    one = engine.TudRunner(lines, grid, atms[0]["Z"], n_layers=32)
    for a, w in zip(atms, want):
        got = one.run(a["T"], a["P"], a["PL"], a["MF"], a["ID"])
        torch.cuda.synchronize()
        for g, x in zip(got, w):
            assert torch.equal(g, x)
    pipes = engine.TudPipelines(lines, grid, atms[0]["Z"], n_layers=32, n_pipes=2)
    got = []
    for a in atms:
        p, out = pipes.run(a["T"], a["P"], a["PL"], a["MF"], a["ID"])
        with torch.cuda.stream(pipes.streams[p]):
            got.append([t.clone() for t in out])
    torch.cuda.synchronize()
    for g3, w3 in zip(got, want):
        for g, x in zip(g3, w3):
            assert torch.equal(g, x)
    pipes.close()
    lines.close()


def test_tile_aligned_shard_reproduces_the_full_grid():
    """5: the second tile and the ragged third as a shard, with only the lines in reach of it."""
    import torch
    from radtxfr_amd import dist, engine
    for column in ("opaque", "mixed"):
        k = _case(column, 32)
        a, grid = k["a"], k["grid"]
        lo = COLUMNS[column][0]
        tbl = _table(lo)
        reach = engine.max_wing_cm(tbl, a["T"], np.asarray(a["P"]) / 101325.0) + STEP
        X = grid.axis()
        sub = dist.subset_lines(tbl, X[TILE], X[-1], reach)
        lines = engine.LineTable(sub)
        shard = grid.shard(TILE, N - TILE)
        run = engine.TudRunner(lines, shard, a["Z"], n_layers=32)
        run.OD.fill_(float("nan"))
        tau, Lu, Ld = run.run(a["T"], a["P"], a["PL"], a["MF"], a["ID"])
        torch.cuda.synchronize()
        assert bool(torch.isnan(run.OD).any()), "the shard hid nothing: the case proves nothing"
        assert torch.equal(tau, k["full"]["tau"][:, TILE:]) and torch.equal(Lu, k["full"]["Lu"][:, TILE:])
        assert torch.equal(Ld, k["full"]["Ld"][TILE:])
        lines.close()


def _ineligible(engine, lines, grid, a, nL, own=True, **kw):
    """Run with the scratch flag on a NaN-filled buffer; the optical depths afterwards."""
    import torch
    if own:
        run = engine.TudRunner(lines, grid, a["Z"], n_layers=nL, keep_od=False, **kw)
    else:  # a caller's buffer: kept complete without a word
        run = engine.TudRunner(lines, grid, a["Z"], n_layers=nL, OD=torch.empty((nL, grid.n), dtype=torch.float32, device="cuda"), **kw)
    run.OD.fill_(float("nan"))
    run.run(a["T"], a["P"], a["PL"], a["MF"], a["ID"])
    torch.cuda.synchronize()
    return run.OD


@pytest.mark.parametrize("what", ["two altitudes", "returnOD", "caller's OD", "too few layers", "hot tiles"])
def test_ineligible_calls_keep_od_complete(what):
    """6: OD complete and equal to engine.optical_depths."""
    import torch
    from radtxfr_amd import _lib, engine
    lo = COLUMNS["opaque"][0]
    nL = 16 if what == "too few layers" else 32  # 16: k_top - 8 = 4, no layer between the bottom chunk and the look
    a = _atmosphere(nL)
    tbl = _table(lo)
    if what == "hot tiles":  # every line six times, a hair apart: more candidates per tile than a workgroup takes whole
        tbl = {k: np.repeat(v, 6) for k, v in tbl.items()}
        tbl["nu"] = tbl["nu"] + np.tile(np.arange(6) * 1e-6, tbl["nu"].size // 6)
        tbl["sw"] = tbl["sw"] / 6.0
        order = np.argsort(tbl["nu"], kind="stable")
        tbl = {k: v[order] for k, v in tbl.items()}
    lines = engine.LineTable(tbl)
    grid = engine.Grid(lo, lo + STEP * (N - 1), N)
    kw = {"two altitudes": dict(Altitudes=[3.0, 500.0]), "returnOD": dict(returnOD=True)}.get(what, {})
    OD = _ineligible(engine, lines, grid, a, nL, own=what != "caller's OD", **kw)
    if what == "hot tiles":
        assert _lib.load().rtx_prep_split_bound(lines.plan(nL, grid.n)._h) > 0
    want = engine.optical_depths(lines, grid, a["T"], a["P"], a["PL"], a["MF"], a["ID"])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(OD).all()) and torch.equal(OD, want)
    lines.close()


_CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import torch
import test_gpu_od_skip as t
from radtxfr_amd import engine
lo = t.COLUMNS["opaque"][0]
a = t._atmosphere(32)
lines = engine.LineTable(t._table(lo))
grid = engine.Grid(lo, lo + t.STEP * (t.N - 1), t.N)
OD = t._ineligible(engine, lines, grid, a, 32)
want = engine.optical_depths(lines, grid, a["T"], a["P"], a["PL"], a["MF"], a["ID"])
torch.cuda.synchronize()
np.savez(sys.argv[2], complete=bool(torch.isfinite(OD).all()), equal=bool(torch.equal(OD, want)))
"""


@pytest.mark.parametrize("switch", ["RADTXFR_TUD_SKIP", "RADTXFR_OD_SKIP"])
def test_switches_keep_od_complete(tmp_path, switch):
    """6, the environment switches (read once per process: a child): the same opaque call, flag set, OD complete."""
    assert os.environ.get(switch) != "0"
    path = str(tmp_path / "od.npz")
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, path], check=True, env=dict(os.environ, **{switch: "0"}), timeout=300)
    r = np.load(path)
    assert bool(r["complete"]) and bool(r["equal"])


def test_jacobian_returns_a_complete_od(monkeypatch):
    """7: tud_jacobian (compute_TUD_jacobian's engine) on the opaque column returns a complete OD. Every float tensor the call
    allocates with torch.empty -- its base runner's OD buffer among them -- comes NaN-filled, so an entry the call does not
    write shows."""
    import torch
    from radtxfr_amd import engine
    lo = COLUMNS["opaque"][0]
    k = _case("opaque", 32)
    a, grid = k["a"], k["grid"]
    lines = engine.LineTable(_table(lo))
    real_empty = torch.empty

    def nan_empty(*args, **kw):
        t = real_empty(*args, **kw)
        return t.fill_(float("nan")) if t.is_floating_point() else t
    monkeypatch.setattr(torch, "empty", nan_empty)
    res = engine.tud_jacobian(lines, grid, a["Z"], a["T"], a["P"], a["PL"], a["MF"], a["ID"], wrt=(2,), layers=[0, 31])
    torch.cuda.synchronize()
    OD = res[3]
    assert bool(torch.isfinite(OD).all()) and torch.equal(OD, k["full"]["OD"])
    for got, name in zip(res[:3], ("tau", "Lu", "Ld")):
        assert torch.equal(got, k["full"][name]), name
    lines.close()
