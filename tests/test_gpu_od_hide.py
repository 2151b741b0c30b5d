"""GPU: the line-sum without the rows nobody reads (rtx_voigt_sum_rows, engine.voigt_sum_rows; rtx_voigt_scatter.hip: the
instantiation for launches that carry skip flags passes done rows over in the row level, keeps dead entries out of its two
lists and drains them where the full lists would have been drained).

For every case of tests/od_hide_cases.py (tests/test_od_hide_host.py shows by a NumPy restatement that each reaches what it
names): on a NaN-filled buffer every point of a live row of the layers [k_lo, k_hi) has the bits of rtx_voigt_sum on the same
prologue, and every other entry -- skipped rows, other layers -- is still NaN. Then the entry's refusals and its stream
contract, as tests/test_gpu_continuum_deriv.py holds rtx_continuum_add_d's."""
import ctypes as C
import functools

import numpy as np
import pytest

import od_hide_cases as H

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _mods():
    import torch
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    from radtxfr_amd import _lib, engine
    lib = _lib.load()
    assert int(lib.rtx_voigt_tile_points()) == H.TILE
    return torch, _lib, lib, engine


_LINES = {}


def _lines(c):
    """One LineTable per (table, shard): its prep object holds the last prologue."""
    _, _, _, eng = _mods()
    key = (c["table"], c["shard"], c["layers"] if c["shard"] else 0)
    if key not in _LINES:
        _LINES[key] = eng.LineTable(H.case_table(c))
    return _LINES[key]


@functools.lru_cache(maxsize=None)
def _want(tname, layers):
    """rtx_voigt_sum on the whole grid with the whole table: [layers][N] float32 on the host. Made once per (table, layers)."""
    torch, _, _, eng = _mods()
    c = dict(table=tname, shard=None, layers=layers)
    _, g, T, p = H.table(tname)
    out = torch.full((layers, g[4]), float("nan"), dtype=torch.float32, device="cuda")
    eng.voigt_sum(_lines(c), eng.Grid(*g), T[:layers], p[:layers], 1.0, out_f32=out)
    torch.cuda.synchronize()
    w = out.cpu().numpy()
    assert np.isfinite(w).all() and np.count_nonzero(w) == w.size
    w.setflags(write=False)
    return w


def _prologue(c):
    """The prologue of the case on its own grid and table (the sum that comes with it goes to a scratch buffer)."""
    torch, _, _, eng = _mods()
    _, _, T, p = H.table(c["table"])
    grid = eng.Grid(*H.case_grid(c))
    nL = c["layers"]
    eng.voigt_sum(_lines(c), grid, T[:nL], p[:nL], 1.0, out_f32=torch.empty((nL, grid.n), dtype=torch.float32, device="cuda"))
    return grid, nL


def _skip_tensor(c):
    torch = _mods()[0]
    return None if c["skip"] is None else torch.as_tensor(np.asarray(c["skip"], dtype=np.uint8), device="cuda")


@pytest.mark.parametrize("name", list(H.CASES))
def test_live_rows_keep_their_bits_and_skipped_rows_are_not_written(name):
    torch, _, _, eng = _mods()
    c = H.CASES[name]
    want = _want(c["table"], c["layers"])
    if c["shard"]:
        want = want[:, c["shard"][0]:c["shard"][0] + c["shard"][1]]
    grid, nL = _prologue(c)
    out = torch.full((nL, grid.n), float("nan"), dtype=torch.float32, device="cuda")
    skip = _skip_tensor(c)
    assert skip is None or (skip.data_ptr() % 16 == 0 and skip.numel() == H.rows_of(grid.n))
    eng.voigt_sum_rows(_lines(c), grid, nL, out, c["k_lo"], c["k_hi"], skip)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    live = np.zeros((nL, grid.n), dtype=bool)
    live[c["k_lo"]:c["k_hi"]] = H.live_points(c)[None, :]
    print("%s: %d of %d entries live" % (name, live.sum(), live.size))
    assert live.any()
    assert np.isnan(got[~live]).all(), "%d entries written that should have been left alone" % int((~np.isnan(got[~live])).sum())
    bad = got[live].view(np.uint32) != want[live].view(np.uint32)
    assert not bad.any(), "%d of %d live points differ from rtx_voigt_sum, first at (layer, point) %s" \
        % (int(bad.sum()), bad.size, np.argwhere(live)[np.nonzero(bad)[0][0]].tolist())


def test_full_range_without_flags_is_rtx_voigt_sum():
    """k_lo = 0, k_hi = n_layers, NULL: the plain sum's bits in every entry, the fp64 layer included; an empty range writes nothing."""
    torch, _, _, eng = _mods()
    c = dict(H.CASES["none"], skip=None)
    grid, nL = _prologue(c)
    out = torch.full((nL, grid.n), float("nan"), dtype=torch.float32, device="cuda")
    eng.voigt_sum_rows(_lines(c), grid, nL, out, 2, 2)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    eng.voigt_sum_rows(_lines(c), grid, nL, out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), _want("base", 4).view(np.uint32))


def test_entry_refusals():
    """Refusals come back as text and enqueue nothing."""
    torch, _lib, lib, eng = _mods()
    c = H.CASES["alt_rows"]
    grid, nL = _prologue(c)
    lines = _lines(c)
    plan = lines.plan(nL, grid.n)
    out = torch.full((nL, grid.n), float("nan"), dtype=torch.float32, device="cuda")
    skip = _skip_tensor(c)
    big = torch.zeros(H.rows_of(grid.n) + 16, dtype=torch.uint8, device="cuda")
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(plan=plan, nL=nL, out=out, ld=grid.n, k=(0, nL), skip=vp(skip), flags=0):
        return lib.rtx_voigt_sum_rows(plan._h if plan is not None else None, grid.byref(), nL, vp(out), ld, k[0], k[1], skip,
                                      eng._stream_ptr(), flags)
    refused = [call(flags=1), call(flags=0x80000000), call(k=(-1, 2)), call(k=(0, nL + 1)), call(k=(3, 2)), call(k=(nL + 1, nL + 1)),
               call(nL=nL - 1), call(ld=grid.n - 1), call(out=None), call(plan=None), call(skip=C.c_void_p(big.data_ptr() + 4))]
    assert all(rc != 0 for rc in refused), refused
    for kw, text in ((dict(flags=1), "flags"), (dict(k=(0, nL + 1)), "layers"), (dict(skip=C.c_void_p(big.data_ptr() + 8)), "aligned")):
        with pytest.raises(_lib.RtxError, match=text):
            _lib.check(call(**kw))
    # an axis prologue on the same prep object
    _, _, T, p = H.table("base")
    X = grid.axis()
    eng.voigt_sum_axis(lines, X, T[:nL], p[:nL], 1.0, out_f32=torch.empty((nL, X.size), dtype=torch.float32, device="cuda"))
    with pytest.raises(_lib.RtxError, match="axis"):
        _lib.check(call(plan=lines.plan(nL, grid.n)))
    # a table with a hot-tile bound: every line of the dense table three times, a hair apart
    tbl = {k: np.repeat(np.asarray(v), 3) for k, v in H.table("dense")[0].items()}
    tbl["nu"] = tbl["nu"] + np.tile(np.arange(3) * 1e-6, tbl["nu"].size // 3)
    hot = eng.LineTable(tbl)
    _, gd, Td, pd = H.table("dense")
    gdev = eng.Grid(*gd)
    eng.voigt_sum(hot, gdev, Td, pd, 1.0, out_f32=torch.empty((2, gdev.n), dtype=torch.float32, device="cuda"))
    assert lib.rtx_prep_split_bound(hot.plan(2, gdev.n)._h) > 0
    o2 = torch.full((2, gdev.n), float("nan"), dtype=torch.float32, device="cuda")
    rc = lib.rtx_voigt_sum_rows(hot.plan(2, gdev.n)._h, gdev.byref(), 2, vp(o2), gdev.n, 0, 2, None, eng._stream_ptr(), 0)
    with pytest.raises(_lib.RtxError, match="hot-tile"):
        _lib.check(rc)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(o2).all())  # a refused call enqueues nothing
    hot.close()
    # what is allowed: an empty shard, an empty layer range
    _prologue(c)
    assert lib.rtx_voigt_sum_rows(plan._h, grid.shard(0, 0).byref(), nL, vp(out), grid.n, 0, nL, vp(skip), eng._stream_ptr(), 0) == 0
    assert call(k=(nL, nL)) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


_CHILD = r"""
import ctypes as C, sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import torch
import test_gpu_od_hide as t
torch_, _lib, lib, eng = t._mods()
c = t.H.CASES["alt_rows"]
grid, nL = t._prologue(c)
out = torch.full((nL, grid.n), float("nan"), dtype=torch.float32, device="cuda")
rc = lib.rtx_voigt_sum_rows(t._lines(c).plan(nL, grid.n)._h, grid.byref(), nL, C.c_void_p(out.data_ptr()), grid.n, 0, nL, None,
                            eng._stream_ptr(), 0)
torch.cuda.synchronize()
msg = lib.rtx_last_error().decode()
print("RC", rc, "UNTOUCHED", bool(torch.isnan(out).all()), "MSG", msg)
"""


def test_point_by_point_kernel_choice_is_refused():
    """RADTXFR_VOIGT_KERNEL=scatter is read once per process: a child."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHILD, root], check=True, env=dict(os.environ, RADTXFR_VOIGT_KERNEL="scatter"), timeout=300,
                       capture_output=True, text=True)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RC ")][-1]
    assert line.startswith("RC 1 UNTOUCHED True") and "point-by-point" in line, line


# ---- the stream contract of rtx_voigt_sum_rows (include/radtxfr_hip.h): on a side stream that is busy when the call is made ----
def _stream_case(v):
    """Variants 0, 1, 2: other tables or layers, skip patterns and layer ranges, each on a LineTable (a prep object) of its own
    whose prologue ran when the case was built. The output is the payload: NaN-filled on the stream after the delay, so what a
    kernel that ran early wrote is gone. The skip flags are structural: any byte pattern is safe to read."""
    import stream_cases as S
    torch, _lib, lib, eng = _mods()
    name = ("alt_rows", "dense", "layer_range")[v]
    c = H.CASES[name]
    _, _, T, p = H.table(c["table"])
    lines = eng.LineTable(H.case_table(c))
    grid = eng.Grid(*H.case_grid(c))
    nL = c["layers"]
    eng.voigt_sum(lines, grid, T[:nL], p[:nL], 1.0, out_f32=torch.empty((nL, grid.n), dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    plan, skip = lines.plan(nL, grid.n), _skip_tensor(c)

    def call(d, h):
        _lib.check(lib.rtx_voigt_sum_rows(plan._h, grid.byref(), nL, S.vp(d["out"]), grid.n, c["k_lo"], c["k_hi"], S.vp(skip),
                                          eng._stream_ptr(), 0))
        return d["out"]
    return S.Case(call, outputs={"out": ((nL, grid.n), torch.float32)}, keep=(lines, skip)), c


@pytest.fixture(scope="module")
def stream_env():
    import stream_cases as S
    torch = _mods()[0]
    cases = [_stream_case(v) for v in range(3)]
    e = dict(S=S, s1=torch.cuda.Stream(), s2=torch.cuda.Stream(), delay=S.Delay(), cases=[k for k, _ in cases], specs=[c for _, c in cases])
    yield e
    torch.cuda.synchronize()
    for k in e["cases"]:
        k.keep[0].close()


def test_stream_order_and_asynchrony(stream_env):
    """Behind a delay on s1, with the output NaN-filled after the delay, the call gives the default-stream bits, and it
    returns while the delay is pending. The default-stream result is the case's: live rows rtx_voigt_sum's, the rest NaN."""
    torch = _mods()[0]
    S, s1, delay = stream_env["S"], stream_env["s1"], stream_env["delay"]
    case, c = stream_env["cases"][0], stream_env["specs"][0]
    ref, _ = S.run_plain(case)
    got = S.as_float(ref[0])
    live = np.zeros(got.shape, dtype=bool)
    live[c["k_lo"]:c["k_hi"]] = H.live_points(c)[None, :]
    assert np.isnan(got[~live]).all() and np.array_equal(got[live].view(np.uint32), _want(c["table"], c["layers"])[live].view(np.uint32))
    warm, _ = S.run_plain(case, s1)
    warm2, host_ms = S.run_plain(case, s1)
    Dms = delay.ms_for(host_ms, "rtx_voigt_sum_rows")
    out, pend, _ = S.run_delayed([case], s1, delay, Dms)
    torch.cuda.synchronize()
    print("rtx_voigt_sum_rows: returned before the delay had passed %s, warmed host time %.3f ms, D %.0f ms" % (pend[0], host_ms, Dms))
    for what, r in (("warm-up on s1", warm), ("warmed call on s1", warm2), ("behind the delay", out[0])):
        assert S.same_bits(r, ref), "%s: %s" % (what, S.describe(r, ref))
    assert pend[0], "the call returned only after %.0f ms of device work ahead of it on its stream had finished" % Dms


def test_two_calls_behind_one_delay_and_two_streams(stream_env):
    """Delay, call A, call B on s1: each equals its solo reference. Then delay and A on s1, B at once on s2, C on s1."""
    torch = _mods()[0]
    S, s1, s2, delay, cases = (stream_env[k] for k in ("S", "s1", "s2", "delay", "cases"))
    refs_ = [S.run_plain(k)[0] for k in cases]
    assert not S.same_bits(refs_[0], refs_[2])
    host_ms = 0.0
    for st in (s1, s2):
        host_ms = sum(S.run_plain(k, st)[1] for k in cases)
    Dms = delay.ms_for(host_ms, "rtx_voigt_sum_rows")
    out, _, _ = S.run_delayed(cases[:2], s1, delay, Dms)
    torch.cuda.synchronize()
    assert S.same_bits(out[0], refs_[0]), "A: " + S.describe(out[0], refs_[0])
    assert S.same_bits(out[1], refs_[1]), "B: " + S.describe(out[1], refs_[1])
    work = [S.fresh(k) for k in cases]
    torch.cuda.synchronize()
    res = [None, None, None]
    with torch.cuda.stream(s1):
        delay.enqueue(Dms)
        for i in (0, 2):
            S.fill(cases[i], work[i][0])
        res[0] = [x.clone() for x in S.flatten(S.issue(cases[0], *work[0])[0])]
    with torch.cuda.stream(s2):
        S.fill(cases[1], work[1][0])
        res[1] = [x.clone() for x in S.flatten(S.issue(cases[1], *work[1])[0])]
    with torch.cuda.stream(s1):
        res[2] = [x.clone() for x in S.flatten(S.issue(cases[2], *work[2])[0])]
    torch.cuda.synchronize()
    got = [S.finish(k, r) for k, r in zip(cases, res)]
    for nm, g, w in zip("ABC", got, refs_):
        assert S.same_bits(g, w), "%s: %s" % (nm, S.describe(g, w))


def teardown_module(module):
    for t in _LINES.values():
        t.close()
    _LINES.clear()
