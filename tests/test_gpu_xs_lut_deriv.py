"""GPU: derivatives through cross-section tables (rtx_xs_od_d, engine.xs_od_d, xs_derivatives=True of the five derivative
drop-ins). The fused kernel bit for bit against rtx_xs_od run on the same fp32 weights, point by point against
the float64 definition (XsLut.dod_host) at a derived bound, its cuts, its refusals and its stream contract, and the drop-ins
end to end: J against the oracle's closed-form chain rule fed dod_host, the adjoint and the tangent against that J, the band
radiances' adjoint identity, and one case composed with the continuum's derivatives.

With RADTXFR_XS_DERIV_PROFILE=<file> the module writes the worst ratio of every point-by-point case to that file
(profiles/xs_deriv_accuracy.txt is such a file); the bound is asserted either way."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import xs_deriv_cases as XC
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL_SPECIES = 2e-4   # tests/test_gpu_continuum_deriv.py, end to end
TOL_T = 2e-3         # tests/test_gpu_continuum_deriv.py, end to end
TOL_L = 1e-5         # tests/test_gpu_xs_lut.py (the table path against the line path), tests/test_gpu_tud_jvp.py
U32 = 2.0 ** -24
F32_TINY = 2.0 ** -126
F32_FLOOR = 1e-30    # tests/test_gpu_tud_jvp.py
_ROWS = []


@pytest.fixture(scope="module")
def mods():
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    from radtxfr_amd import _lib, afit_xs, continuum, engine, hapi, sensor, synthetic
    from radtxfr_amd import radiative_transfer as rt
    m = dict(lib=_lib.load(), _lib=_lib, afit_xs=afit_xs, ct=continuum, engine=engine, hapi=hapi, sensor=sensor, synthetic=synthetic, rt=rt)
    assert int(m["lib"].rtx_xs_tile_points()) == XC.TILE
    yield m
    path = os.environ.get("RADTXFR_XS_DERIV_PROFILE")
    if path and _ROWS:
        with open(path, "w") as f:
            f.write("# tests/test_gpu_xs_lut_deriv.py::test_kernel_point_by_point, written by the module itself with\n"
                    "# RADTXFR_XS_DERIV_PROFILE=<this file> (%s, torch %s).\n"
                    "# worst |device - dod_host| / ((n_terms + 2) 2^-24 sum_t |W_t| |row_t|) over every point of a case, n_terms = 12 for\n"
                    "# dOD/dT (3 molecules x 4 corners) and 4 for dOD/dMF; asserted <= 1\n"
                    "# layers | species | offset | n | ld | dOD/dT | dOD/dMF\n" % (torch.cuda.get_device_name(0), torch.__version__))
            for r in _ROWS:
                f.write(r + "\n")
            f.write("# worst of all cases: dOD/dT %.3g, dOD/dMF %.3g\n"
                    % (max(float(r.split("|")[5]) for r in _ROWS), max(float(r.split("|")[6]) for r in _ROWS)))


@pytest.fixture(scope="module")
def table(mods):
    """The random table on the device and, per number of layers, made once and read-only: the layers, the float64
    definition on the whole axis for species (1, 2) and the sum of magnitudes sum_t |W_t| |row_t| of each output."""
    afit_xs = mods["afit_xs"]
    lut = afit_xs.XsLut.from_grids(XC.entries())
    xs_rows = np.concatenate([np.ldexp(lut.rows(m).astype(np.float64), -lut.exponent(m)).reshape(-1, XC.N_AXIS) for m in lut.molecules])
    ref = {}
    for nL in (1, 3):
        lay = XC.layers(nL)
        dT, dMF = lut.dod_host(*XC.largs(lay), species=(1, 2))
        rows, w_T, w_K, idx = afit_xs.layer_terms_d(lut._tables, *XC.largs(lay), (1, 2))
        mag_T, mag_K = afit_xs.dod_from_terms(xs_rows, rows, np.abs(w_T), np.abs(w_K), idx)
        dK = np.stack([dMF[1], dMF[2]])
        for a in (dT, dK, mag_T, mag_K):
            a.setflags(write=False)
        ref[nL] = dict(lay=lay, dT=dT, dK=dK, mag_T=mag_T, mag_K=mag_K)
    yield dict(lut=lut, ref=ref)
    lut.free()


def _blocks(nL, nS, n, aligned):
    """Float32 views dOD_dT [nL][n] and K [nS][nL][n] with one row stride, filled with NaN: aligned -- rows 16 bytes apart from
    16-byte aligned bases; not aligned -- an odd leading dimension from bases one float past such an address."""
    ld = (n + 3) // 4 * 4 if aligned else (n + 4) // 4 * 4 + 1
    pad = 0 if aligned else 1
    bT = torch.full((nL * ld + 4,), float("nan"), dtype=torch.float32, device="cuda")
    bK = torch.full((max(nS, 1) * nL * ld + 4,), float("nan"), dtype=torch.float32, device="cuda")
    dT = bT[pad:][:nL * ld].view(nL, ld)[:, :n]
    Kb = bK[pad:][:nS * nL * ld].view(nS, nL, ld)[:, :, :n]
    assert (dT.data_ptr() % 16 == 0) == aligned and (ld % 4 == 0) == aligned
    return dT, Kb, ld, (bT, bK)


def _hp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _fused(mods, lut, off, n, terms, dT, Kb, ld, flags=0):
    """rtx_xs_od_d on host terms (rows, w_T, w_K, idx) as XsLut.layer_terms_d returns them; returns the status."""
    rows, w_T, w_K, idx = terms
    nS = 0 if Kb is None else len(idx)
    return mods["lib"].rtx_xs_od_d(lut._handle(), off, n, rows.shape[0], _hp(rows), _hp(w_T), nS, _hp(idx) if nS else None,
                                   _hp(w_K) if nS else None, _dp(dT), _dp(Kb) if nS else None, ld, mods["engine"]._stream_ptr(), flags)


def _separate(mods, lut, off, n, terms, aligned):
    """The oracle of the bits: 1 + S calls of rtx_xs_od on the same fp32 weights -- w_T for the temperature row, one
    molecule's slots and zeros elsewhere for each K[s]."""
    rows, w_T, w_K, idx = terms
    nL, nS = rows.shape[0], len(idx)
    dT, Kb, ld, keep = _blocks(nL, nS, n, aligned)
    check = mods["_lib"].check
    check(mods["lib"].rtx_xs_od(lut._handle(), off, n, nL, _hp(rows), _hp(w_T), _dp(dT), ld, mods["engine"]._stream_ptr()))
    for s in range(nS):
        w = np.zeros_like(w_T)
        w[:, idx[s], :] = w_K[s]
        check(mods["lib"].rtx_xs_od(lut._handle(), off, n, nL, _hp(rows), _hp(w), _dp(Kb[s]), ld, mods["engine"]._stream_ptr()))
    return dT, Kb, keep


@pytest.mark.parametrize("aligned", [True, False], ids=["ld4", "ld_odd"])
@pytest.mark.parametrize("off", XC.OFFSETS)
@pytest.mark.parametrize("n", XC.N_POINTS)
@pytest.mark.parametrize("nL", [1, 3])
def test_kernel_bits_are_rtx_xs_ods(mods, table, nL, n, off, aligned):
    """Every output of the fused entry equals, bit for bit, rtx_xs_od run on the same fp32 weights; for every species list,
    with both outputs and with either left out; nothing is written past n. The single layer, and the second of three, sits
    exactly on a T node."""
    lut, lay = table["lut"], table["ref"][nL]["lay"]
    assert off + n <= XC.N_AXIS
    for species in XC.SPECIES_LISTS:
        terms = lut.layer_terms_d(*XC.largs(lay), species)
        want_T, want_K, _ = _separate(mods, lut, off, n, terms, aligned)
        nS = len(species)
        variants = [(True, True), (True, False), (False, True)] if nS else [(True, False)]
        for with_T, with_K in variants:
            dT, Kb, ld, (bT, bK) = _blocks(nL, nS, n, aligned)
            assert _fused(mods, lut, off, n, terms, dT if with_T else None, Kb if with_K else None, ld) == 0, mods["lib"].rtx_last_error()
            what = (nL, n, off, aligned, species, with_T, with_K)
            pad = 0 if aligned else 1
            if with_T:
                assert np.array_equal(dT.cpu().numpy().view(np.uint32), want_T.cpu().numpy().view(np.uint32)), what
                assert bool(torch.isfinite(dT).all()) and float(dT.abs().max()) > 0.0
                gaps = bT.clone()
                gaps[pad:][:nL * ld].view(nL, ld)[:, :n] = float("nan")
                assert bool(torch.isnan(gaps).all()), what  # the NaN fill outside [nL][n] is untouched
            else:
                assert bool(torch.isnan(bT).all()), what
            if with_K:
                assert np.array_equal(Kb.cpu().numpy().view(np.uint32), want_K.cpu().numpy().view(np.uint32)), what
                assert bool(torch.isfinite(Kb).all()) and float(Kb.min()) > 0.0
                gaps = bK.clone()
                gaps[pad:][:nS * nL * ld].view(nS, nL, ld)[:, :, :n] = float("nan")
                assert bool(torch.isnan(gaps).all()), what
            else:
                assert bool(torch.isnan(bK).all()), what


@pytest.mark.parametrize("aligned", [True, False], ids=["ld4", "ld_odd"])
@pytest.mark.parametrize("off,n", [(0, XC.N_AXIS), (5, 2051), (4, 1027), (5, 3)])
@pytest.mark.parametrize("species", [(1, 2), (2, 1)])
@pytest.mark.parametrize("nL", [1, 3])
def test_kernel_point_by_point(mods, table, nL, species, off, n, aligned):
    """engine.xs_od_d against XsLut.dod_host at every point. The bound is derived: the device rounds each weight to fp32
    once (the rows are the stored fp32 rows in both) and runs one fmaf chain of n_terms terms, so
        |got - ref| <= (n_terms + 2) 2^-24 sum_t |W_t| |row_t|,
    against the sum of magnitudes because the terms of the temperature chain cancel."""
    lut, r = table["lut"], table["ref"][nL]
    dT, Kb, ld, _ = _blocks(nL, 2, n, aligned)
    mods["engine"].xs_od_d(lut, off, *XC.largs(r["lay"]), dOD_dT=dT, K=Kb, species=species)
    sl = slice(off, off + n)
    order = [s - 1 for s in species]
    e_T = np.abs(dT.double().cpu().numpy() - r["dT"][:, sl]) / ((12 + 2) * U32 * r["mag_T"][:, sl])
    e_K = np.abs(Kb.double().cpu().numpy() - r["dK"][order][:, :, sl]) / ((4 + 2) * U32 * r["mag_K"][order][:, :, sl])
    print("nL=%d species %r off=%d n=%d ld=%d: worst |got - ref| / bound dOD/dT %.3g, dOD/dMF %.3g" % (nL, species, off, n, ld, e_T.max(), e_K.max()))
    _ROWS.append("%d | %-6r | %d | %4d | %4d | %.3g | %.3g" % (nL, species, off, n, ld, e_T.max(), e_K.max()))
    assert np.all(r["mag_T"] > 0) and np.all(r["mag_K"] > 0)
    assert e_T.max() <= 1.0 and e_K.max() <= 1.0
    # the temperature chain has terms of both signs: the bound is stated against more than the result
    assert np.all(r["mag_T"] >= np.abs(r["dT"])) and np.any(r["mag_T"] > 1.01 * np.abs(r["dT"]))


def test_cuts_are_bit_identical(mods, table):
    """Halves at an offset not divisible by 4, and single points, give the bits of the uncut call; so does a Grid shard."""
    lut, lay = table["lut"], table["ref"][3]["lay"]
    eng = mods["engine"]

    def run(off, n, aligned=True):
        dT, Kb, _, _ = _blocks(3, 2, n, aligned)
        eng.xs_od_d(lut, off, *XC.largs(lay), dOD_dT=dT, K=Kb, species=(2, 1))
        return dT, Kb
    nX = XC.N_AXIS
    full_T, full_K = run(0, nX)
    h = nX // 2 + 1
    assert h % 4 != 0
    for a, b, aligned in ((0, h, True), (h, nX, True), (h, nX, False), (0, 1, True), (7, 8, True), (1023, 1025, False), (nX - 1, nX, True)):
        dT, Kb = run(a, b - a, aligned)
        assert torch.equal(dT, full_T[:, a:b]) and torch.equal(Kb, full_K[:, :, a:b]), (a, b)
    g = eng.Grid(lut.grid.xmin, lut.grid.xmax, nX)
    dT, Kb, _, _ = _blocks(3, 2, 100, True)
    eng.xs_od_d(lut, g.shard(h, 100), *XC.largs(lay), dOD_dT=dT, K=Kb, species=(2, 1))
    assert torch.equal(dT, full_T[:, h:h + 100]) and torch.equal(Kb, full_K[:, :, h:h + 100])
    # rtx_xs_od's own results are what they were: the forward call before and after a derivative call
    od = lambda: eng.xs_od(lut, 0, *XC.largs(lay), out_f32=torch.empty((3, nX), dtype=torch.float32, device="cuda"))
    before = od()
    run(0, nX)
    assert torch.equal(before, od())


def test_argument_errors_come_back_as_text(mods, table):
    lut, lay = table["lut"], table["ref"][3]["lay"]
    lib, _lib, eng = mods["lib"], mods["_lib"], mods["engine"]
    rows, w_T, w_K, idx = lut.layer_terms_d(*XC.largs(lay), (1, 2))
    n = 8
    dT, Kb, ld, (bT, bK) = _blocks(3, 2, n, True)

    def call(rows=rows, w_T=w_T, w_K=w_K, idx=idx, n_spec=2, out=(dT, Kb), off=0, n=n, ld=ld, flags=0, nL=3, lut_h=lut._handle()):
        return lib.rtx_xs_od_d(lut_h, off, n, nL, _hp(rows), _hp(w_T), n_spec, _hp(idx), _hp(w_K), _dp(out[0]), _dp(out[1]), ld,
                               eng._stream_ptr(), flags)

    def bad(a, at, value):
        b = a.copy()
        b.reshape(-1)[at] = value
        return b
    many = np.arange(17, dtype=np.int32)
    cases = {"both NULL": call(out=(None, None)), "flags": call(flags=1), "n_layers": call(nL=0),
             "outside the table's axis": call(off=XC.N_AXIS - 4), "smaller than n": call(ld=n - 1),
             "outside the table's 3 molecules": call(idx=np.array([1, 3], dtype=np.int32)),
             "outside the table's 3 molecules ": call(idx=np.array([-1, 0], dtype=np.int32)),
             "distinct": call(idx=np.array([1, 1], dtype=np.int32)), "n_spec=17": call(idx=many, n_spec=17),
             "n_spec=-1": call(n_spec=-1), "weight_dT_h[5] is not finite": call(w_T=bad(w_T, 5, np.nan)),
             "weight_K_h[13] is not finite": call(w_K=bad(w_K, 13, np.inf)),
             "rows_h[2]=14": call(rows=bad(rows, 2, 14)), "rows_h[0]=-1": call(rows=bad(rows, 0, -1)),
             "K is NULL": call(out=(dT, None)), "needs weight_dT_h": call(w_T=None),
             "needs spec_mol_h": call(idx=None), "pointer is NULL": call(rows=None), "pointer is NULL ": call(lut_h=None)}
    for text, rc in cases.items():
        assert rc != 0, text
    for text, kw in (("both NULL", dict(out=(None, None))), ("distinct", dict(idx=np.array([1, 1], dtype=np.int32))),
                     ("not finite", dict(w_K=bad(w_K, 13, np.inf))), ("n_spec=17", dict(idx=many, n_spec=17)), ("flags=1", dict(flags=1))):
        with pytest.raises(_lib.RtxError, match=text):
            _lib.check(call(**kw))
    with pytest.raises(ValueError, match="both None"):
        eng.xs_od_d(lut, 0, *XC.largs(lay))
    with pytest.raises(ValueError, match="species"):
        eng.xs_od_d(lut, 0, *XC.largs(lay), K=Kb, species=(1,))
    with pytest.raises(ValueError, match="distinct"):
        eng.xs_od_d(lut, 0, *XC.largs(lay), K=Kb, species=(1, 1))
    with pytest.raises(ValueError, match="layer 0 .*molecule 1"):
        eng.xs_od_d(lut, 0, lay["T"] + 30.0, *XC.largs(lay)[1:], K=Kb, species=(1, 2))
    torch.cuda.synchronize()
    assert bool(torch.isnan(bT).all()) and bool(torch.isnan(bK).all())  # a refused call enqueues nothing
    # what is allowed: n = 0 writes nothing; K = NULL with n_spec = 0; dOD_dT = NULL without its weights
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(bT).all()) and bool(torch.isnan(bK).all())
    assert call(n_spec=0, out=(dT, None), idx=None, w_K=None) == 0 and call(out=(None, Kb), w_T=None) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dT).all()) and bool(torch.isfinite(Kb).all())


# ---- the stream contract of rtx_xs_od_d (include/radtxfr_hip.h), as tests/test_gpu_continuum_deriv.py holds rtx_continuum_add_d
# ---- to it: on a side stream that is busy when the call is made ----------------------------------------------------------------
def _stream_case(mods, lut, v):
    """Variants 0, 1, 2: other layers, species lists, axis cuts and sizes. The call reads no device payload of the
    caller's: the order test rests on its two outputs, poisoned on the stream after the delay like any caller-owned output
    (a kernel that ran early would be overwritten). rows, the two weight arrays and the species' table indices are the host
    arrays; overwritten, the rows become row 0 and the indices 0, valid values, the weights NaN."""
    import stream_cases as S
    lib, _lib, eng = mods["lib"], mods["_lib"], mods["engine"]
    nL, species, off, n = ((3, (1, 2), 0, 2051), (1, (2,), 5, 700), (2, (2, 1), 4, 333))[v]
    lay = XC.layers(3)
    lay = {k: (a[:nL] if k != "ID" else a) for k, a in lay.items()}
    lay["T"] = lay["T"] + 1.5 * v
    rows, w_T, w_K, idx = lut.layer_terms_d(*XC.largs(lay), species)
    nS = len(species)

    def call(d, h):
        _lib.check(lib.rtx_xs_od_d(lut._handle(), off, n, nL, S.hp(h["rows"]), S.hp(h["w_T"]), nS, S.hp(h["idx"]), S.hp(h["w_K"]),
                                   S.vp(d["dT"]), S.vp(d["K"]), n, eng._stream_ptr(), 0))
        return [d["dT"], d["K"]]
    outs = {"dT": ((nL, n), torch.float32), "K": ((nS, nL, n), torch.float32)}
    return S.Case(call, outputs=outs, host=dict(rows=rows, w_T=w_T, w_K=w_K, idx=idx), keep=lut), (lay, species, off, n)


@pytest.fixture(scope="module")
def stream_env(mods):
    import stream_cases as S
    e = dict(S=S, s1=torch.cuda.Stream(), s2=torch.cuda.Stream(), delay=S.Delay())
    yield e
    torch.cuda.synchronize()


def test_stream_order_asynchrony_and_staging(mods, table, stream_env):
    """Behind a delay on s1 the call gives the default-stream bits; the warmed call returns while the delay is pending; the
    host arrays may be overwritten as soon as it has returned. The default-stream result is engine.xs_od_d's."""
    S, s1, delay = stream_env["S"], stream_env["s1"], stream_env["delay"]
    lut = table["lut"]
    case, (lay, species, off, n) = _stream_case(mods, lut, 0)
    other, _ = _stream_case(mods, lut, 1)
    ref, _ = S.run_plain(case)
    dT, Kb, _, _ = _blocks(3, 2, n, True)
    mods["engine"].xs_od_d(lut, off, *XC.largs(lay), dOD_dT=dT, K=Kb, species=species)
    assert np.array_equal(S.as_float(ref[0]), dT.cpu().numpy()) and np.array_equal(S.as_float(ref[1]), Kb.cpu().numpy())
    warm, _ = S.run_plain(case, s1)   # grows the terms of s1
    warm2, host_ms = S.run_plain(case, s1)
    Dms = delay.ms_for(host_ms, "rtx_xs_od_d")
    S.run_plain(other, s1)            # the terms of s1 are now another call's
    out, pend, _ = S.run_delayed([case], s1, delay, Dms)
    S.run_plain(other, s1)
    out_s, pend_s, _ = S.run_delayed([case], s1, delay, Dms, scribble=True)
    torch.cuda.synchronize()
    print("rtx_xs_od_d: returned before the delay had passed %s / %s, warmed host time %.3f ms, D %.0f ms" % (pend[0], pend_s[0], host_ms, Dms))
    for what, r in (("warm-up on s1", warm), ("warmed call on s1", warm2), ("behind the delay", out[0]), ("host arrays overwritten", out_s[0])):
        assert S.same_bits(r, ref), "%s: %s" % (what, S.describe(r, ref))
    assert pend[0] and pend_s[0], "the call returned only after %.0f ms of device work ahead of it on its stream had finished" % Dms


def test_two_calls_behind_one_delay_and_two_streams(mods, table, stream_env):
    """Delay, call A, call B (other terms, another size) on s1: each equals its solo reference, so B's terms did not reach
    A's kernel. Then delay and A on s1, B at once on s2, C on s1: two streams run against one table, each with terms of
    its own; rtx_xs_od's terms on the same stream are another array still."""
    S, s1, s2, delay = stream_env["S"], stream_env["s1"], stream_env["s2"], stream_env["delay"]
    lut = table["lut"]
    cases = [_stream_case(mods, lut, v)[0] for v in range(3)]
    refs_ = [S.run_plain(c)[0] for c in cases]
    host_ms = 0.0
    for st in (s1, s2):
        for c in cases:
            S.run_plain(c, st)
        host_ms = sum(S.run_plain(c, st)[1] for c in cases)
    Dms = delay.ms_for(host_ms, "rtx_xs_od_d")
    out, _, _ = S.run_delayed(cases[:2], s1, delay, Dms)
    torch.cuda.synchronize()
    assert S.same_bits(out[0], refs_[0]), "A: " + S.describe(out[0], refs_[0])
    assert S.same_bits(out[1], refs_[1]), "B: " + S.describe(out[1], refs_[1])
    work = [S.fresh(c) for c in cases]
    torch.cuda.synchronize()
    res = [None, None, None]
    lay = XC.layers(3)
    fwd = torch.empty((3, 64), dtype=torch.float32, device="cuda")
    with torch.cuda.stream(s1):
        delay.enqueue(Dms)
        for i in (0, 2):
            S.fill(cases[i], work[i][0])
        res[0] = [x.clone() for x in S.flatten(S.issue(cases[0], *work[0])[0])]
        mods["engine"].xs_od(lut, 0, *XC.largs(lay), out_f32=fwd)  # the forward entry between the two: terms of its own
    with torch.cuda.stream(s2):
        S.fill(cases[1], work[1][0])
        res[1] = [x.clone() for x in S.flatten(S.issue(cases[1], *work[1])[0])]
    with torch.cuda.stream(s1):
        res[2] = [x.clone() for x in S.flatten(S.issue(cases[2], *work[2])[0])]
    torch.cuda.synchronize()
    got = [S.finish(c, r) for c, r in zip(cases, res)]
    for nm, g, w in zip("ABC", got, refs_):
        assert S.same_bits(g, w), "%s: %s" % (nm, S.describe(g, w))
    assert torch.equal(fwd, mods["engine"].xs_od(lut, 0, *XC.largs(lay), out_f32=torch.empty_like(fwd)))


# ---- end to end: the drop-ins with xs_derivatives=True -------------------------------------------------------------------------
XMIN, XMAX, DV = 1000.0, 1002.0, 0.01
T_NODES = np.array([250.0, 296.0])
P_PA = np.array([0.3 * 101325.0, 101325.0])
WRT = ("T", 1, 2)
ALTS = np.array([1.2, 500.0])  # between the layers and above them all
FD_STEP = 0.5                  # the default fd_step_T of the drop-ins


@pytest.fixture(scope="module")
def e2e(mods):
    """tests/test_gpu_xs_lut.py's kind of fixture on 200 points: 400 synthetic lines, molecules 1 and 2, tables from
    cross_section_grid on 2 x 2 nodes, a four-layer off-node column (every layer at least FD_STEP from a T node) and an
    on-node one. The oracle in float64, made once: the table's optical depth by the rule of DESIGN 4.11 on the float64
    tables, dod_host, and J = g dOD + h from cpu_ref.jacobian_from_od; J_fd the same with dOD/dT the central difference of
    that optical depth at +- FD_STEP, which is what dT_method="fd" is defined to compute, in exact arithmetic."""
    from oracle import cpu_ref
    rt, afit_xs, hapi = mods["rt"], mods["afit_xs"], mods["hapi"]
    tbl = mods["synthetic"].synth_line_table(20261019, 400, XMIN - 5.0, XMAX + 5.0)
    X = rt.make_spectral_axis(XMIN, XMAX, DV)
    P_atm = P_PA / 101325.0
    entries, names = [], {}
    for m in (1, 2):
        sel = tbl["molec_id"] == m
        names[m] = "xs_deriv_test_m%d" % m
        hapi.LOCAL_TABLE_CACHE[names[m]] = {"header": {"number_of_rows": int(sel.sum())}, "data": {k: v[sel] for k, v in tbl.items()}}
        xs = afit_xs.cross_section_grid(names[m], T_NODES, P_atm, X, WavenumberWingHW=50.0, WavenumberWing=0.0, IntensityThreshold=0.0)
        entries.append(dict(ID=m, T=T_NODES, P_atm=P_atm, X=X, xs=xs))
    lut = afit_xs.XsLut.from_grids(entries)
    common = dict(DVOUT=DV, Zs=np.array([0.5, 1.5, 2.5, 3.5]), PLs=np.array([1.0, 1.0, 1.0, 1.0]),
                  MFs_VAL=np.array([[8.0, 0.4], [5.0, 0.4], [2.0, 0.39], [1.0, 0.38]]), MFs_ID=np.array([1, 2]), Altitudes=ALTS)
    a = dict(common, Ts=np.array([290.0, 277.7, 263.1, 251.0]), Ps=np.array([95000.0, 70000.0, 50000.0, 31000.0]))
    on_node = dict(common, Ts=np.array([296.0, 296.0, 250.0, 250.0]), Ps=np.array([P_PA[1], P_PA[0], P_PA[1], P_PA[0]]))
    assert np.all(np.abs(a["Ts"][:, None] - T_NODES[None, :]) >= FD_STEP)
    tabs, xs_rows = [(1, T_NODES, P_atm, 0), (2, T_NODES, P_atm, 4)], np.concatenate([e["xs"].reshape(4, -1) for e in entries])
    lay = (a["Ts"], a["Ps"] / 101325.0, a["PLs"], a["MFs_VAL"], a["MFs_ID"])
    od = XC.forward_od(tabs, xs_rows, *lay)
    d_T, d_MF = lut.dod_host(*lay)
    od_fd = (XC.forward_od(tabs, xs_rows, lay[0] + FD_STEP, *lay[1:]) - XC.forward_od(tabs, xs_rows, lay[0] - FD_STEP, *lay[1:])) / (2.0 * FD_STEP)
    yield dict(tbl=tbl, lut=lut, X=X, a=a, on_node=on_node, nL=4, od=od, d_T=d_T, d_MF=d_MF, od_fd=od_fd, cpu_ref=cpu_ref, lay=lay)
    lut.free()
    for n in names.values():
        hapi.LOCAL_TABLE_CACHE.pop(n, None)


def _oracle_J(e, od, dOD, returnOD):
    """{w: [2 nZ + 1][nX][nL]} from the closed-form chain rule on optical depths od [nL][nX] and their derivatives."""
    g, h = e["cpu_ref"].jacobian_from_od(e["X"], od.T, e["a"]["Ts"], e["a"]["Zs"], ALTS, returnOD=returnOD)
    return {w: g * dOD[w].T[None] + (h if w == "T" else 0.0) for w in dOD}


def _worst_rows(got_rows, want, nL):
    """Worst rel_err (floor 1e-3 of the row's maximum) over rows [2 nZ + 1] and layers; a (row, layer) the oracle has all
    zero (a layer above the sensor) must be all zero."""
    errs = []
    for row, got in enumerate(got_rows):
        for l in range(nL):
            if not np.any(want[row][:, l]):
                assert not np.any(got[:, l]), (row, l)
                continue
            errs.append(rel_err(got[:, l], want[row][:, l], floor_frac=1e-3))
    return max(errs)


def _jacobian_rows(Jw, nZ):
    return [Jw[0][:, z, :] for z in range(nZ)] + [Jw[1][:, z, :] for z in range(nZ)] + [Jw[2]]


def _kw(e, **more):
    return dict(dict(xs_lut=e["lut"], xs_derivatives=True, **e["a"]), **more)


@pytest.mark.parametrize("method,returnOD", [("analytic", False), ("analytic", True), ("fd", False)], ids=["analytic", "analytic-returnOD", "fd"])
def test_jacobian_against_the_oracle(mods, e2e, method, returnOD):
    """J of compute_TUD_jacobian(xs_lut=, xs_derivatives=True) against the oracle fed dod_host, at TOL_T for "T" and
    TOL_SPECIES for a species, row by row and layer by layer; the base outputs are compute_TUD(xs_lut=)'s bits. For "fd"
    the oracle's own central difference at +- 0.5 K is first held, in float64, to a quarter of TOL_T against its
    derivative (inside a cell OD = (A + B T) / T, and the difference is off by h^2 / T^2 of the A part alone): the column
    needs no scaling.

    MEASURED on an MI355X: "analytic" T 1.7e-5, species 1.6e-5 and 3.2e-5, the same under returnOD; "fd" T 7.3e-4 with the
    oracle's own difference at 1.6e-4."""
    rt, e = mods["rt"], e2e
    nZ = ALTS.size
    dOD = {"T": e["d_T"], 1: e["d_MF"][1], 2: e["d_MF"][2]}
    want = _oracle_J(e, e["od"], dOD, returnOD)
    if method == "fd":
        J_fd = _oracle_J(e, e["od"], {"T": e["od_fd"]}, returnOD)["T"]
        own = _worst_rows(J_fd, want["T"], e["nL"])
        print("the 0.5 K central difference of the oracle against its derivative, float64: %.3e" % own)
        assert own <= 0.25 * TOL_T
    Xj, tau, Lu, Ld, J = rt.compute_TUD_jacobian(XMIN, XMAX, wrt=WRT, dT_method=method, **_kw(e, returnOD=returnOD))
    base = rt.compute_TUD(XMIN, XMAX, xs_lut=e["lut"], returnOD=returnOD, **e["a"])
    for x, y in zip((Xj, tau, Lu, Ld), base):
        assert np.array_equal(x, y)
    for w in WRT:
        tol = TOL_T if w == "T" else TOL_SPECIES
        worst = _worst_rows(_jacobian_rows(J[w], nZ), want[w], e["nL"])
        print("%s, returnOD=%s, wrt %r: worst rel_err against the oracle %.3e (bound %.0e)" % (method, returnOD, w, worst, tol))
        assert worst <= tol


def test_on_node_species_entries_equal_the_line_paths(mods, e2e):
    """On the on-node column the table is the line path's cross section: the species entries of J within TOL_L of
    compute_TUD_jacobian(line_table=)'s. (The "T" entries differ by definition: a cell's slope against the line-sum's.)"""
    rt, e = mods["rt"], e2e
    _, _, _, _, J = rt.compute_TUD_jacobian(XMIN, XMAX, wrt=(1, 2), xs_lut=e["lut"], xs_derivatives=True, **e["on_node"])
    _, _, _, _, J_l = rt.compute_TUD_jacobian(XMIN, XMAX, wrt=(1, 2), line_table=e["tbl"], **e["on_node"])
    for w in (1, 2):
        for got, want in zip(_jacobian_rows(J[w], ALTS.size), _jacobian_rows(J_l[w], ALTS.size)):
            for l in range(e["nL"]):
                if not np.any(want[:, l]):
                    assert not np.any(got[:, l])
                    continue
                err = rel_err(got[:, l], want[:, l], floor_frac=1e-3)
                assert err <= TOL_L, (w, l, err)


def test_fd_step_out_of_the_table_raises_the_forwards_error(mods, e2e):
    rt, e = mods["rt"], e2e
    with pytest.raises(ValueError, match="layer 3 .*lies outside molecule 1's table range"):
        rt.compute_TUD_jacobian(XMIN, XMAX, wrt=("T",), fd_step_T=2.0, **_kw(e))
    rt.compute_TUD_jacobian(XMIN, XMAX, wrt=("T",), fd_step_T=2.0, dT_method="analytic", layers=[3], **_kw(e))


def test_vjp_and_jvp_are_the_contractions_of_that_jacobian(mods, e2e):
    """compute_TUD_vjp and compute_TUD_jvp through the table against the stored J, at the bounds of tests/test_gpu_tud_vjp.py
    and tests/test_gpu_tud_jvp.py as tests/test_gpu_continuum_deriv.py states them end to end."""
    rt, e = mods["rt"], e2e
    kw = _kw(e, dT_method="analytic")
    X, nL, nZ = e["X"], e["nL"], ALTS.size
    nX = X.size
    _, tau, La, Ld, J = rt.compute_TUD_jacobian(XMIN, XMAX, wrt=WRT, **kw)
    rng = np.random.default_rng(5)
    n_vec = 2
    g_tau, g_La, g_Ld = rng.normal(size=(nX, nZ, n_vec)), rng.normal(size=(nX, nZ, n_vec)), rng.normal(size=(nX, n_vec))
    Xv, tau_v, La_v, Ld_v, grad = rt.compute_TUD_vjp(XMIN, XMAX, {"tau": g_tau, "La": g_La, "Ld": g_Ld}, wrt=WRT, **kw)
    for x, y in zip((Xv, tau_v, La_v, Ld_v), (X, tau, La, Ld)):
        assert np.array_equal(x, y)
    G32 = lambda g: g.astype(np.float32).astype(np.float64)  # the cotangent the device is given
    for w in WRT:
        dtau, dLa, dLd = J[w]
        terms = [("xav,xal->lv", G32(g_tau), dtau), ("xav,xal->lv", G32(g_La), dLa), ("xv,xl->lv", G32(g_Ld), dLd)]
        want = sum(np.einsum(s, g, j) for s, g, j in terms)
        scale = sum(np.einsum(s, np.abs(g), np.abs(j)) for s, g, j in terms)
        g_sum = np.abs(G32(g_tau)).sum(axis=(0, 1)) + np.abs(G32(g_La)).sum(axis=(0, 1)) + np.abs(G32(g_Ld)).sum(axis=0)
        bound = 4.0 * U32 * scale + F32_TINY * g_sum[None, :]  # tests/test_gpu_tud_vjp.py's bound
        err = np.abs(grad[w] - want)
        print("vjp vs stored J, wrt %r: worst |got - ref| / bound = %.3g" % (w, float(np.max(err / bound))))
        assert np.count_nonzero(want) == want.size and np.all(err <= bound), w
    tang = {"T": rng.normal(size=(nL, n_vec)), 1: rng.normal(size=(nL, n_vec)) * 0.5, 2: rng.normal(size=(nL, n_vec)) * 0.05}
    Xv, tau_v, La_v, Ld_v, d = rt.compute_TUD_jvp(XMIN, XMAX, tang, **kw)
    for x, y in zip((Xv, tau_v, La_v, Ld_v), (X, tau, La, Ld)):
        assert np.array_equal(x, y)
    for i_, name in enumerate(("tau", "La", "Ld")):
        sub_x = "xal,lv->xav" if name != "Ld" else "xl,lv->xv"
        want = sum(np.einsum(sub_x, J[w][i_], tang[w]) for w in WRT)
        S_J = 0.0
        for w in WRT:
            Jw = np.abs(J[w][i_])
            den = np.maximum(np.maximum(Jw, 1e-3 * np.max(Jw, axis=0, keepdims=True)), F32_FLOOR)
            S_J = S_J + np.einsum(sub_x, den, np.abs(tang[w]))
        v_sum = sum(np.abs(tang[w]).sum(axis=0) for w in WRT)
        bound = 2.0 * TOL_L * S_J + F32_TINY * v_sum + U32 * np.abs(want)  # tests/test_gpu_tud_jvp.py, end to end
        err = np.abs(d[name] - want)
        print("jvp vs stored J, %s: worst |got - ref| / bound = %.3g" % (name, float(np.max(err / bound))))
        assert np.count_nonzero(want) > 0.5 * want.size and np.all(err <= bound), name


def test_band_radiance_adjoint_identity(mods, e2e):
    """<g, J v> = <J^T g, v> at the band radiances through compute_band_radiance_jvp and compute_band_radiance_vjp with
    xs_derivatives=True, within the sum of the two chains' bounds as tests/test_gpu_continuum_deriv.py forms it: the sensor
    tangent's and the sensor adjoint's on the device rows, and through the stored Jacobian the TUD tangent's under |G| and
    the TUD adjoint's under |v|."""
    import sensor_jvp_cases as JC
    import sensor_vjp_cases as VC
    from test_gpu_sensor_vjp import K_DE, K_DTS, K_ROW
    rt, eng, sensor, e = mods["rt"], mods["engine"], mods["sensor"], e2e
    s = sensor.Sensor.from_shape([1000.40, 1000.95, 1001.50], 0.3, "triangle")
    Xk = np.array([999.9, 1000.5, 1001.0, 1001.5, 1002.1])
    rng = np.random.default_rng(9)
    E = rng.uniform(0.6, 1.0, (5, 3)).astype(np.float32)
    Ts_s = 296.0
    one = np.array([500.0])
    kw = _kw(e, dT_method="analytic", Altitudes=one)
    nL, nB, nk, nE, n_vec = e["nL"], 3, 5, 3, 2
    atm = {"T": rng.normal(size=(nL, n_vec)), 1: rng.normal(size=(nL, n_vec)) * 0.5, 2: rng.normal(size=(nL, n_vec)) * 0.05}
    surf = {"Ts_surface": rng.normal(size=n_vec), "emis": (rng.normal(size=(nk, nE, n_vec)) * 0.05).astype(np.float32)}
    X_out, L, dL = rt.compute_band_radiance_jvp(XMIN, XMAX, s, Xk, E, Ts_s, dict(atm, **surf), **kw)
    assert L.shape == (nB, nE) and dL.shape == (nB, nE, n_vec) and np.all(np.isfinite(L)) and np.all(np.isfinite(dL))
    cot = rng.normal(size=(nB, nE, n_vec)).astype(np.float32)
    _, L_v, grad = rt.compute_band_radiance_vjp(XMIN, XMAX, s, Xk, E, Ts_s, cot, wrt=WRT, **kw)
    assert np.array_equal(L, L_v)
    # a surface-only tangent runs the base state alone, from the table
    _, L_s, _ = rt.compute_band_radiance_jvp(XMIN, XMAX, s, Xk, E, Ts_s, {"Ts_surface": 1.0}, **kw)
    assert np.array_equal(L, L_s)
    X, tau, La, Ld = rt.compute_TUD(XMIN, XMAX, xs_lut=e["lut"], **dict(e["a"], Altitudes=one))
    nX = X.size
    grid = eng.Grid(XMIN, XMAX, nX)
    dev32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float32), device="cuda")
    t_d, a_d, d_d, E_d = dev32(tau), dev32(La), dev32(Ld), dev32(E)
    _, L_f = sensor.band_radiance_srf_fused(grid, t_d, a_d, d_d, Xk, E_d, Ts_s, s)
    assert np.array_equal(L, L_f.cpu().numpy())
    _, _, _, _, rows = rt.compute_TUD_jvp(XMIN, XMAX, atm, **kw)
    r32 = {k: rows[k].astype(np.float32) for k in ("tau", "La", "Ld")}
    _, _, _, _, J = rt.compute_TUD_jacobian(XMIN, XMAX, wrt=WRT, **kw)  # {w: (dtau, dLa, dLd)}, each [nX][nL]
    tables = [(np.asarray(x), np.asarray(r)) for x, r in s.tables]
    names = ("tau", "La", "Ld")
    EPS = U32
    for v in range(n_vec):
        adj = {k: t.cpu().numpy().astype(np.float64) for k, t in
               sensor.band_radiance_srf_vjp(grid, t_d, a_d, d_d, Xk, E_d, Ts_s, s, cot[..., v]).items()}
        G = {"tau": adj["G_tau"], "La": adj["G_La"], "Ld": adj["G_Ld"]}
        c64 = cot[:, :, v].astype(np.float64)
        lhs = float(np.sum(c64 * dL[:, :, v]))
        rhs = float(sum(np.sum(grad[w][:, v] * atm[w][:, v]) for w in WRT) + grad["Ts_surface"][v] * surf["Ts_surface"][v]
                    + np.sum(grad["emis"][..., v] * surf["emis"][..., v].astype(np.float64)))
        d_s = dict(d_tau=r32["tau"][:, v], d_La=r32["La"][:, v], d_Ld=r32["Ld"][:, v], d_Ts=surf["Ts_surface"][v:v + 1],
                   d_E=surf["emis"][..., v])
        _, sc = JC.tangent(X, tables, tau.astype(np.float32), La.astype(np.float32), Ld.astype(np.float32), Xk, E, [Ts_s], **d_s)
        o = VC.adjoint(X, tables, tau.astype(np.float32), La.astype(np.float32), Ld.astype(np.float32), Xk, E, [Ts_s], cot[None, ..., v])
        bound = 32 * EPS * float(np.sum(np.abs(c64) * sc[0]))
        for key, skey, k in (("d_tau", "G_tau", K_ROW["G_tau"]), ("d_La", "G_La", K_ROW["G_La"]), ("d_Ld", "G_Ld", K_ROW["G_Ld"]),
                             ("d_Ts", "dTs", K_DTS), ("d_E", "dE", K_DE)):
            bound += k * EPS * float(np.sum(o["scale"][skey] * np.abs(np.asarray(d_s[key]).astype(np.float64))))
        v_sum = sum(np.abs(atm[w][:, v]).sum() for w in WRT)
        for i_, name in enumerate(names):
            S_J, want = 0.0, 0.0
            for w in WRT:
                Jw = np.abs(J[w][i_])
                den = np.maximum(np.maximum(Jw, 1e-3 * np.max(Jw, axis=0, keepdims=True)), F32_FLOOR)
                S_J = S_J + den @ np.abs(atm[w][:, v])
                want = want + J[w][i_] @ atm[w][:, v]
            bound += float(np.sum(np.abs(G[name]) * (2.0 * TOL_L * S_J + F32_TINY * v_sum + U32 * np.abs(want))))
        g_sum = sum(np.abs(G[name]).sum() for name in names)
        for w in WRT:
            scale_w = sum(np.abs(G[name]) @ np.abs(J[w][i_]) for i_, name in enumerate(names))  # [nL]
            bound += float(np.sum(np.abs(atm[w][:, v]) * (4.0 * U32 * scale_w + F32_TINY * g_sum)))
        print("band adjoint identity, vector %d: %.9g vs %.9g, |diff| = %.3g, bound %.3g" % (v, lhs, rhs, abs(lhs - rhs), bound))
        assert lhs != 0.0 and abs(lhs - rhs) <= bound


def test_with_the_continuums_derivatives(mods, e2e):
    """continuum= with continuum_derivatives=True composes after the table: J against the oracle fed both dod_hosts (the
    table's and continuum.Continuum.dod_host) on the optical depth of both; the base outputs are
    compute_TUD(xs_lut=, continuum=)'s bits."""
    import continuum_cases as K
    rt, ct, e = mods["rt"], mods["ct"], e2e
    X, lay = e["X"], e["lay"]
    lay_pa = (e["a"]["Ts"], e["a"]["Ps"], e["a"]["PLs"], e["a"]["MFs_VAL"], e["a"]["MFs_ID"])
    comps = []
    for unit in (K.component(ct, 1, 950.0, 10.0, 12, seed=6), K.component(ct, 2, 1000.303, 0.25, 9, seed=7, kind="steps")):
        sc = 0.25 / unit.od_host(X, *lay_pa).sum(axis=0).max()  # the definition is linear in the coefficients
        c = unit.components[0]
        comps.append(ct.Component(c.molecule, c.v0, c.dv, Cs_a=sc * c.Cs_a, T_a=c.T_a, Cs_b=sc * c.Cs_b, T_b=c.T_b, Cf=sc * c.Cf))
    cont = ct.Continuum(comps)
    c_T, c_MF = cont.dod_host(X, *lay_pa)
    od = e["od"] + cont.od_host(X, *lay_pa)
    dOD = {"T": e["d_T"] + c_T, 1: e["d_MF"][1] + c_MF[1], 2: e["d_MF"][2] + c_MF[2]}
    want = _oracle_J(e, od, dOD, False)
    kw = _kw(e, continuum=cont, continuum_derivatives=True, dT_method="analytic")
    Xj, tau, Lu, Ld, J = rt.compute_TUD_jacobian(XMIN, XMAX, wrt=WRT, **kw)
    base = rt.compute_TUD(XMIN, XMAX, xs_lut=e["lut"], continuum=cont, **e["a"])
    for x, y in zip((Xj, tau, Lu, Ld), base):
        assert np.array_equal(x, y)
    plain = rt.compute_TUD_jacobian(XMIN, XMAX, wrt=WRT, dT_method="analytic", **_kw(e))[4]
    nZ = ALTS.size
    for w in WRT:
        tol = TOL_T if w == "T" else TOL_SPECIES
        worst = _worst_rows(_jacobian_rows(J[w], nZ), want[w], e["nL"])
        print("table + continuum, wrt %r: worst rel_err against the oracle %.3e (bound %.0e)" % (w, worst, tol))
        assert worst <= tol
        # the continuum must matter: without it the same entry misses the oracle
        assert rel_err(plain[w][1][:, nZ - 1, 0], want[w][2 * nZ - 1][:, 0], floor_frac=1e-3) > 10.0 * tol, w
    with pytest.raises(NotImplementedError, match="continuum is not supported"):
        rt.compute_TUD_jacobian(XMIN, XMAX, wrt=WRT, **_kw(e, continuum=cont))


def test_the_default_still_refuses_and_the_option_alone_changes_no_bit(mods, e2e):
    rt, e = mods["rt"], e2e
    for fn, rest in ((rt.compute_TUD_jacobian, ()), (rt.compute_TUD_vjp, ({"tau": np.ones((e["X"].size, ALTS.size))},)),
                     (rt.compute_TUD_jvp, ({"T": np.ones(4)},))):
        with pytest.raises(NotImplementedError, match=fn.__name__ + ": xs_lut is not supported"):
            fn(XMIN, XMAX, *rest, xs_lut=e["lut"], **e["a"])
    a = rt.compute_TUD_jacobian(XMIN, XMAX, wrt=WRT, line_table=e["tbl"], **e["a"])
    b = rt.compute_TUD_jacobian(XMIN, XMAX, wrt=WRT, line_table=e["tbl"], xs_derivatives=True, **e["a"])
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x, y)
    for w in WRT:
        for x, y in zip(a[4][w], b[4][w]):
            assert np.array_equal(x, y, equal_nan=True)
    with pytest.raises(ValueError, match="requested axis"):
        rt.compute_TUD_jacobian(XMIN, XMAX - 1.0, xs_lut=e["lut"], xs_derivatives=True, **e["a"])
