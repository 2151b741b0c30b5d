"""GPU: tabulated continuum absorption (radtxfr_amd/continuum.py, rtx_continuum_add). The kernel point by point
against the float64 definition (continuum.od_host) at the project's pin of 1e-5 of the layer's largest value, the in-place
add, bit-identity under cuts of the axis, the drop-ins end to end against the oracle's TUD sweep fed line-sum + continuum,
the refusals, and the stream contract of the new entry point on a busy side stream.

With RADTXFR_CONTINUUM_PROFILE=<file> the module writes the worst error of every kernel case to that file
(profiles/continuum_accuracy.txt is such a file); the bound is asserted either way."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import continuum_cases as K
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL_L = 1e-5     # tests/test_gpu_parity.py: compute_TUD against the oracle
TOL_TAU = 2e-6
_ROWS = []


@pytest.fixture(scope="module")
def mods():
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    from radtxfr_amd import _lib, afit_xs, continuum, engine, hapi, synthetic
    from radtxfr_amd import radiative_transfer as rt
    m = dict(lib=_lib.load(), _lib=_lib, afit_xs=afit_xs, ct=continuum, engine=engine, hapi=hapi, synthetic=synthetic, rt=rt)
    assert int(m["lib"].rtx_continuum_tile_points()) == 1024  # N_AXIS = two tiles + 3, the n below sit around one tile
    yield m
    path = os.environ.get("RADTXFR_CONTINUUM_PROFILE")
    if path and _ROWS:
        with open(path, "w") as f:
            f.write("# tests/test_gpu_continuum.py::test_pure_continuum_point_by_point, written by the module itself with\n"
                    "# RADTXFR_CONTINUUM_PROFILE=<this file> (%s, torch %s).\n"
                    "# worst |device - od_host| / max(od_host of the layer) over the layers of a case; asserted <= %.0e\n"
                    "# grid | layers | components | n | ld | worst error\n"
                    % (torch.cuda.get_device_name(0), torch.__version__, K.TOL_PIN))
            for r in _ROWS:
                f.write(r + "\n")
            f.write("# worst of all cases: %.3g\n" % max(float(r.split("|")[5]) for r in _ROWS))


@pytest.fixture(scope="module")
def refs(mods):
    """od_host of the whole axis of every (grid, layers, components): made once, read-only."""
    out = {}
    for name in K.GRIDS:
        X = mods["engine"].Grid(*K.grid_args(name)).axis()
        for nL in (1, 3):
            lay = K.layers(nL)
            for nC in (1, 2):
                cont = K.continuum(mods["ct"], name, nC)
                ref = cont.od_host(X, lay["T"], lay["P"], lay["PL"], lay["MF"], lay["ID"])
                ref.setflags(write=False)
                out[(name, nL, nC)] = (cont, lay, ref)
    return out


def _block(nL, n, aligned, fill=None, rng=None):
    """A float32 [nL][n] view for the kernel: aligned -- rows 16 bytes apart from a 16-byte aligned base; not aligned -- an odd
    leading dimension from a base one float past such an address."""
    ld = (n + 3) // 4 * 4 if aligned else (n + 4) // 4 * 4 + 1
    buf = torch.zeros(nL * ld + 1, dtype=torch.float32, device="cuda")
    od = buf[0 if aligned else 1:][:nL * ld].view(nL, ld)[:, :n]
    assert (od.data_ptr() % 16 == 0) == aligned and (nL == 1 or (od.stride(0) % 4 == 0) == aligned)
    if fill is not None:
        od.copy_(torch.as_tensor(fill, device="cuda"))
    return od


def _add(mods, cont, lay, grid, od):
    return mods["engine"].continuum_add(cont, grid, lay["T"], lay["P"], lay["PL"], lay["MF"], lay["ID"], od)


@pytest.mark.parametrize("aligned", [True, False], ids=["ld4", "ld_odd"])
@pytest.mark.parametrize("n", [1, 3, 1024, 1027, 2051])
@pytest.mark.parametrize("nC", [1, 2])
@pytest.mark.parametrize("nL", [1, 3])
@pytest.mark.parametrize("name", sorted(K.GRIDS))
def test_pure_continuum_point_by_point(mods, refs, name, nL, nC, n, aligned):
    """From OD = 0 the device result against od_host at every point: at most 1e-5 of the layer's largest continuum value.
    fine: 5990 + 0.001 i with nodes 0.5 apart (the fp32 abscissa; whole waves on one stencil) and a four-node axis over part
    of the grid; coarse: step 1.0014 over nodes 10 and 7.3 apart (neighbouring lanes on different stencils)."""
    cont, lay, ref = refs[(name, nL, nC)]
    grid = mods["engine"].Grid(*K.grid_args(name))
    off = 0 if n == K.N_AXIS else 5  # a run that does not start on a multiple of 4 of the axis
    od = _block(nL, n, aligned)
    _add(mods, cont, lay, grid.shard(off, n), od)
    got = od.double().cpu().numpy()
    want = ref[:, off:off + n]
    scale = ref.max(axis=1, keepdims=True)  # the layer's largest value on the whole axis
    assert np.all(scale > 0) and np.all(np.isfinite(got))
    err = float(np.max(np.abs(got - want) / scale))
    print("%s nL=%d nC=%d n=%d %s: worst error %.3g of the layer maximum (bound %.0e)"
          % (name, nL, nC, n, "ld % 4 == 0" if aligned else "odd ld", err, K.TOL_PIN))
    _ROWS.append("%-6s | %d | %d | %4d | %4d | %.3g" % (name, nL, nC, n, od.stride(0) if nL > 1 else n, err))
    assert err <= K.TOL_PIN and np.all(got > 0)  # the first component covers the axis


def test_partial_axes_alone(mods):
    """A component that covers part of the grid, on its own: exactly 0 outside its axis, the pin inside. First a four-node
    axis (the one stencil there is: j0 = 0 for every point, t from 0 to 3), then the axis with runs of zero nodes, beside
    which the cubic undershoots and max(0, .) cuts it."""
    ct, eng = mods["ct"], mods["engine"]
    lay = K.layers(3)
    cont = K.component(ct, 1, 5990.2501, 0.4, 4, seed=9)  # 5990.2501 .. 5991.4501
    grid = eng.Grid(*K.grid_args("fine"))
    ref = cont.od_host(grid.axis(), lay["T"], lay["P"], lay["PL"], lay["MF"], lay["ID"])
    od = _add(mods, cont, lay, grid, _block(3, K.N_AXIS, True)).double().cpu().numpy()
    err = float(np.max(np.abs(od - ref) / ref.max(axis=1, keepdims=True)))
    print("four-node axis: worst error %.3g of the layer maximum" % err)
    inside = (grid.axis() >= 5990.2501) & (grid.axis() <= cont.components[0].vend)
    assert err <= K.TOL_PIN and inside.sum() == 1200 and np.all(od[:, ~inside] == 0) and np.all(od[:, inside] > 0)
    _ROWS.append("%-6s | %d | %d | %4d | %4d | %.3g" % ("fine, four nodes alone", 3, 1, K.N_AXIS, K.N_AXIS + 1, err))
    m, v0, dv, n, kind = K.GRIDS["coarse"]["comps"][1]
    cont = K.component(ct, m, v0, dv, n, seed=4, kind=kind)
    grid = eng.Grid(*K.grid_args("coarse"))
    X = grid.axis()
    ref = cont.od_host(X, lay["T"], lay["P"], lay["PL"], lay["MF"], lay["ID"])
    od = _add(mods, cont, lay, grid, _block(3, K.N_AXIS, False)).double().cpu().numpy()
    err = float(np.max(np.abs(od - ref) / ref.max(axis=1, keepdims=True)))
    inside = (X >= v0) & (X <= cont.components[0].vend)
    cut = int((ref[:, inside] == 0).sum())
    print("axis with zero runs: worst error %.3g of the layer maximum, max(0, .) cut %d of %d points" % (err, cut, 3 * inside.sum()))
    assert err <= K.TOL_PIN and cut > 0 and 600 < inside.sum() < 800 and np.all(od[:, ~inside] == 0) and np.all(od >= 0)
    _ROWS.append("%-6s | %d | %d | %4d | %4d | %.3g" % ("coarse, zero runs alone", 3, 1, K.N_AXIS, K.N_AXIS + 2, err))


@pytest.mark.parametrize("aligned", [True, False], ids=["ld4", "ld_odd"])
@pytest.mark.parametrize("name", sorted(K.GRIDS))
def test_in_place_add(mods, refs, name, aligned):
    """On a random non-zero block the result is OD + (the pure continuum the kernel gives from 0), rounded once."""
    cont, lay, _ = refs[(name, 3, 2)]
    grid = mods["engine"].Grid(*K.grid_args(name))
    n = K.N_AXIS
    pure = _add(mods, cont, lay, grid, _block(3, n, aligned)).double().cpu().numpy()
    od0 = (np.random.default_rng(11).uniform(0.05, 3.0, (3, n)) * pure.max(axis=1, keepdims=True) / 3.0).astype(np.float32)  # of the continuum's size
    got =_add(mods, cont, lay, grid, _block(3, n, aligned, fill=od0)).double().cpu().numpy()
    exact = od0.astype(np.float64) + pure
    assert pure.max() > 0.01 * od0.min(), "the continuum must be visible beside the block"
    err = np.abs(got - exact) / exact
    print("in place: worst |got - (OD + pure)| / (OD + pure) = %.3g (one rounding: %.3g)" % (err.max(), 2.0 ** -24))
    assert err.max() <= 2.0 ** -24


@pytest.mark.parametrize("aligned", [True, False], ids=["ld4", "ld_odd"])
@pytest.mark.parametrize("name", sorted(K.GRIDS))
def test_cuts_are_bit_identical(mods, refs, name, aligned):
    """Three ragged shards of the axis, none starting on a multiple of 4, give the bits of the uncut call."""
    cont, lay, _ = refs[(name, 3, 2)]
    grid = mods["engine"].Grid(*K.grid_args(name))
    full = _add(mods, cont, lay, grid, _block(3, K.N_AXIS, True))
    assert float(full.max()) > 0
    cuts = (0, 1021, 1538, K.N_AXIS)
    assert all(c % 4 for c in cuts[1:])
    for a, b in zip(cuts, cuts[1:]):
        part = _add(mods, cont, lay, grid.shard(a, b - a), _block(3, b - a, aligned))
        assert torch.equal(part, full[:, a:b]), (a, b, int((part != full[:, a:b]).sum()))
    one = _add(mods, cont, lay, grid.shard(1023, 1), _block(3, 1, aligned))
    assert torch.equal(one, full[:, 1023:1024])


def test_kernel_argument_errors(mods):
    eng, lib, RtxError = mods["engine"], mods["lib"], mods["_lib"].RtxError
    lay = K.layers(3)
    cont = K.continuum(mods["ct"], "fine", 1)
    grid = eng.Grid(*K.grid_args("fine"))
    with pytest.raises(ValueError, match="molecule 1 is not in MF_ID"):
        eng.continuum_add(cont, grid, lay["T"], lay["P"], lay["PL"], lay["MF"], np.array([3, 2]), _block(3, K.N_AXIS, True))
    od = _block(1, 8, True)
    T, v0, dv, tab = np.array([280.0]), np.array([5989.0]), np.array([0.5]), np.ones((1, 1, 8), dtype=np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(nn, T=T, dv=dv, tab=tab, flags=0):
        nn = np.array([nn], dtype=np.int32)
        return lib.rtx_continuum_add(grid.shard(0, 8).byref(), 1, vp(T), 1, vp(v0), vp(dv), vp(nn), vp(tab), 8, C.c_void_p(od.data_ptr()), 8,
                                     eng._stream_ptr(), flags)
    assert call(3) != 0 and call(9) != 0 and call(8, dv=np.array([0.0])) != 0 and call(8, T=np.array([0.0])) != 0 and call(8, flags=1) != 0
    bad = tab.copy()
    bad[0, 0, 5] = np.inf
    assert call(8, tab=bad) != 0 and call(6, tab=bad) != 0  # node 5 is read with 6 nodes or more
    with pytest.raises(RtxError, match="not finite"):
        mods["_lib"].check(call(8, tab=bad))
    torch.cuda.synchronize()
    assert float(od.abs().max()) == 0.0  # a refused call enqueues nothing
    assert call(8) == 0 and call(5, tab=bad) == 0  # with 5 nodes the columns from 5 on are read by nobody
    torch.cuda.synchronize()
    assert float(od.min()) > 0.0 and bool(torch.isfinite(od).all())


# ---- end to end: the drop-ins ------------------------------------------------------------------------------------------------
XMIN, XMAX, DV = 1000.0, 1004.0, 0.001


@pytest.fixture(scope="module")
def e2e(mods):
    """The small synthetic line table and four-layer column of tests/test_gpu_xs_lut.py on 4000 points, a two-component
    continuum scaled so that its column optical depth is about 0.5, and the oracle's line-sum and continuum, made once."""
    from oracle import cpu_ref
    rt, ct = mods["rt"], mods["ct"]
    tbl = mods["synthetic"].synth_line_table(20261019, 400, XMIN - 5.0, XMAX + 5.0)
    a = dict(DVOUT=DV, Zs=np.array([0.5, 1.5, 2.5, 3.5]), PLs=np.array([1.0, 1.0, 1.0, 1.0]),
             MFs_VAL=np.array([[8.0, 0.4], [5.0, 0.4], [2.0, 0.39], [1.0, 0.38]]), MFs_ID=np.array([1, 2]), Altitudes=np.asarray([500]),
             Ts=np.array([290.0, 277.7, 263.1, 251.0]), Ps=np.array([95000.0, 70000.0, 50000.0, 31000.0]))
    X = rt.make_spectral_axis(XMIN, XMAX, DV)
    unit = K.component(ct, 1, 950.0, 10.0, 12, seed=6) + K.component(ct, 2, 1001.3, 0.5, 9, seed=7, kind="foreign")
    col = unit.od_host(X, a["Ts"], a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"]).sum(axis=0).max()
    s = 0.5 / col  # the definition is linear in the coefficients
    cont = ct.Continuum([ct.Component(c.molecule, c.v0, c.dv, Cs_a=None if c.Cs_a is None else s * c.Cs_a, T_a=c.T_a,
                                      Cs_b=None if c.Cs_b is None else s * c.Cs_b, T_b=c.T_b, Cf=None if c.Cf is None else s * c.Cf)
                         for c in unit.components])
    od_c = cont.od_host(X, a["Ts"], a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"])  # [nL][nX]
    od_l = np.stack([cpu_ref.layer_od(tbl, X, a["Ts"][k], a["Ps"][k], a["PLs"][k], a["MFs_VAL"][k], a["MFs_ID"]) for k in range(4)])
    for r in (od_c, od_l):
        r.setflags(write=False)
    return dict(tbl=tbl, a=a, X=X, cont=cont, od_c=od_c, od_l=od_l, cpu_ref=cpu_ref)


def _against(e, got, od_lines, **kw):
    X, tau, Lu, Ld = got
    tr, ur, dr = e["cpu_ref"].tud_from_od(e["X"], (od_lines + e["od_c"]).T, e["a"]["Ts"], e["a"]["Zs"], **kw)
    err = dict(tau=float(np.max(np.abs(tau - tr))), Lu=rel_err(Lu, ur), Ld=rel_err(Ld, dr))
    print("against tud_from_od(line-sum + od_host):", err)
    assert np.array_equal(X, e["X"]) and tau.shape == np.shape(tr)
    return err


def test_compute_tud_with_continuum_vs_oracle(mods, e2e):
    rt, e = mods["rt"], e2e
    got = rt.compute_TUD(XMIN, XMAX, line_table=e["tbl"], continuum=e["cont"], **e["a"])
    err = _against(e, got, e["od_l"])
    assert err["tau"] <= TOL_TAU and err["Lu"] <= TOL_L and err["Ld"] <= TOL_L
    plain = rt.compute_TUD(XMIN, XMAX, line_table=e["tbl"], **e["a"])
    assert np.max(plain[1] - got[1]) > 0.1, "the continuum must matter in this case"
    assert "continuum" not in rt.options
    # the chunked copy-out cuts the axis: the same bits
    cut = rt.compute_TUD(XMIN, XMAX, line_table=e["tbl"], continuum=e["cont"], chunks=3, **e["a"])
    for x, y in zip(got, cut):
        assert np.array_equal(x, y)
    # more slant paths than one launch takes: the branch that makes the optical depths on their own
    th = np.linspace(0.0, 0.9, 9)
    err = _against(e, rt.compute_TUD(XMIN, XMAX, line_table=e["tbl"], continuum=e["cont"], theta_r=th, **e["a"]), e["od_l"], theta_r=th)
    assert err["tau"] <= TOL_TAU and err["Lu"] <= TOL_L and err["Ld"] <= TOL_L


def test_return_od_carries_the_continuum(mods, e2e):
    rt, e = mods["rt"], e2e
    got = rt.compute_TUD(XMIN, XMAX, line_table=e["tbl"], continuum=e["cont"], returnOD=True, **e["a"])
    X, od, Lu, Ld = got
    tr, ur, dr = e["cpu_ref"].tud_from_od(e["X"], (e["od_l"] + e["od_c"]).T, e["a"]["Ts"], e["a"]["Zs"], returnOD=True)
    print("returnOD: OD %.3g, Lu %.3g" % (rel_err(od, tr), rel_err(Lu, ur)))
    assert rel_err(od, tr) <= TOL_L and rel_err(Lu, ur) <= TOL_L
    bare = rt.compute_TUD(XMIN, XMAX, line_table=e["tbl"], returnOD=True, **e["a"])[1]
    assert np.max(od - bare) > 0.4  # the column's 0.5 is in it
    # one layer through compute_OD: line-sum + continuum
    a = e["a"]
    kw = dict(DVOUT=DV, T=a["Ts"][1], P=a["Ps"][1], PL=a["PLs"][1], MF_VAL=a["MFs_VAL"][1], MF_ID=a["MFs_ID"], line_table=e["tbl"])
    X1, od1 = rt.compute_OD(XMIN, XMAX, continuum=e["cont"], **kw)
    X0, od0 = rt.compute_OD(XMIN, XMAX, **kw)
    assert np.array_equal(X1, e["X"]) and rel_err(od1, e["od_l"][1] + e["od_c"][1]) <= TOL_L
    assert rel_err(od1 - od0, e["od_c"][1]) <= 1e-4  # a difference of two fp32 spectra


def test_explicit_none_is_the_call_without_the_keyword(mods, e2e):
    rt, e = mods["rt"], e2e
    for kw in (dict(), dict(broadening="self"), dict(returnOD=True)):
        a = rt.compute_TUD(XMIN, XMAX, line_table=e["tbl"], **dict(e["a"], **kw))
        b = rt.compute_TUD(XMIN, XMAX, line_table=e["tbl"], continuum=None, **dict(e["a"], **kw))
        for x, y in zip(a, b):
            assert np.array_equal(x, y), kw
    atm = [dict(Ts=e["a"]["Ts"] - 1.0)]
    a = rt.compute_TUD_batch(XMIN, XMAX, atm, line_table=e["tbl"], **e["a"])
    b = rt.compute_TUD_batch(XMIN, XMAX, atm, line_table=e["tbl"], continuum=None, **e["a"])
    assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))


def test_self_broadening_branch(mods, e2e):
    """broadening="self": the branch's own optical depths (engine.optical_depths) plus od_host, through the oracle's sweep."""
    rt, eng, e = mods["rt"], mods["engine"], e2e
    a = e["a"]
    tbl = rt._resolve_table(e["tbl"])
    grid = eng.Grid(XMIN, XMAX, e["X"].size)
    od_self = eng.optical_depths(tbl, grid, a["Ts"], a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"], broadening="self").double().cpu().numpy()
    got = rt.compute_TUD(XMIN, XMAX, line_table=e["tbl"], broadening="self", continuum=e["cont"], **a)
    err = _against(e, got, od_self)
    assert err["tau"] <= TOL_TAU and err["Lu"] <= TOL_L and err["Ld"] <= TOL_L
    # and the runner's block is that branch's block with the add applied in place: the same bits
    run = eng.TudRunner(tbl, grid, a["Zs"], broadening="self", continuum=e["cont"])
    run.run(a["Ts"], a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"])
    want = eng.optical_depths(tbl, grid, a["Ts"], a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"], broadening="self")
    eng.continuum_add(e["cont"], grid, a["Ts"], a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"], want)
    assert torch.equal(run.OD, want)


def test_xs_lut_branch(mods, e2e):
    """xs_lut=: the table's optical depths (engine.xs_od) plus od_host, through the oracle's sweep."""
    rt, eng, afit_xs, hapi, e = mods["rt"], mods["engine"], mods["afit_xs"], mods["hapi"], e2e
    a = e["a"]
    T_nodes, P_atm = np.array([250.0, 296.0]), np.array([0.3, 1.0])
    entries, names = [], []
    for m in (1, 2):
        sel = e["tbl"]["molec_id"] == m
        names.append("continuum_test_m%d" % m)
        hapi.LOCAL_TABLE_CACHE[names[-1]] = {"header": {"number_of_rows": int(sel.sum())}, "data": {k: v[sel] for k, v in e["tbl"].items()}}
        xs = afit_xs.cross_section_grid(names[-1], T_nodes, P_atm, e["X"], WavenumberWingHW=50.0, WavenumberWing=0.0, IntensityThreshold=0.0)
        entries.append(dict(ID=m, T=T_nodes, P_atm=P_atm, X=e["X"], xs=xs))
    lut = afit_xs.XsLut.from_grids(entries)
    try:
        grid = eng.Grid(XMIN, XMAX, e["X"].size)
        od_xs = eng.xs_od(lut, grid, a["Ts"], a["Ps"] / 101325.0, a["PLs"], a["MFs_VAL"], a["MFs_ID"]).double().cpu().numpy()
        got = rt.compute_TUD(XMIN, XMAX, xs_lut=lut, continuum=e["cont"], **a)
        err = _against(e, got, od_xs)
        assert err["tau"] <= TOL_TAU and err["Lu"] <= TOL_L and err["Ld"] <= TOL_L
        kw = dict(DVOUT=DV, T=a["Ts"][2], P=a["Ps"][2], PL=a["PLs"][2], MF_VAL=a["MFs_VAL"][2], MF_ID=a["MFs_ID"], xs_lut=lut)
        _, od1 = rt.compute_OD(XMIN, XMAX, continuum=e["cont"], **kw)
        assert rel_err(od1, od_xs[2] + e["od_c"][2]) <= TOL_L
        res = rt.compute_TUD_batch(XMIN, XMAX, [{}], xs_lut=lut, continuum=e["cont"], **a)
        assert all(np.array_equal(x, y) for x, y in zip(res[0], got))
    finally:
        lut.free()
        for n in names:
            hapi.LOCAL_TABLE_CACHE.pop(n, None)


def test_batch_equals_single_calls(mods, e2e):
    rt, e = mods["rt"], e2e
    base = e["a"]
    atms = [dict(Ts=base["Ts"] - 0.4 * k, Ps=base["Ps"] * (1 + 0.01 * k), MFs_VAL=base["MFs_VAL"] * (1 + 0.3 * k)) for k in range(3)]
    res = rt.compute_TUD_batch(XMIN, XMAX, atms, line_table=e["tbl"], continuum=e["cont"], **base)
    assert len(res) == 3
    for atm, (X, tau, Lu, Ld) in zip(atms, res):
        X1, tau1, Lu1, Ld1 = rt.compute_TUD(XMIN, XMAX, line_table=e["tbl"], continuum=e["cont"], **dict(base, **atm))
        assert np.array_equal(X, X1) and np.array_equal(tau, tau1) and np.array_equal(Lu, Lu1) and np.array_equal(Ld, Ld1)
    assert not np.array_equal(res[0][1], res[1][1])
    bare = rt.compute_TUD_batch(XMIN, XMAX, atms[:1], line_table=e["tbl"], **base)
    assert np.max(bare[0][1] - res[0][1]) > 0.1
    # engine.TudPipelines passes the option on
    eng = mods["engine"]
    tbl = rt._resolve_table(e["tbl"])
    grid = eng.Grid(XMIN, XMAX, e["X"].size)
    pipes = eng.TudPipelines(tbl, grid, base["Zs"], n_pipes=2, continuum=e["cont"])
    try:
        outs = []
        for atm in atms:
            p, (tau, Lu, Ld) = pipes.run(atm["Ts"], atm["Ps"], base["PLs"], atm["MFs_VAL"], base["MFs_ID"])
            pipes.streams[p].synchronize()
            outs.append(tau[0].double().cpu().numpy())
    finally:
        pipes.close()
    for (X, tau, Lu, Ld), t in zip(res, outs):
        assert np.array_equal(tau, t)


def test_refusals(mods, e2e):
    rt, e = mods["rt"], e2e
    kw = dict(line_table=e["tbl"], continuum=e["cont"], **e["a"])
    with pytest.raises(NotImplementedError, match="compute_TUD_jacobian: continuum"):
        rt.compute_TUD_jacobian(XMIN, XMAX, **kw)
    with pytest.raises(NotImplementedError, match="compute_TUD_vjp: continuum"):
        rt.compute_TUD_vjp(XMIN, XMAX, {"tau": np.ones(e["X"].size)}, **kw)
    with pytest.raises(NotImplementedError, match="compute_TUD_jvp: continuum"):
        rt.compute_TUD_jvp(XMIN, XMAX, {"T": np.ones(4)}, **kw)
    with pytest.raises(NotImplementedError, match="compute_band_radiance_vjp: continuum"):
        rt.compute_band_radiance_vjp(XMIN, XMAX, None, None, None, 296.0, None, **kw)
    with pytest.raises(NotImplementedError, match="compute_band_radiance_jvp: continuum"):
        rt.compute_band_radiance_jvp(XMIN, XMAX, None, None, None, 296.0, None, **kw)
    with pytest.raises(NotImplementedError, match="continuum with devices"):
        rt.compute_TUD_batch(XMIN, XMAX, [{}], devices=[0], **kw)
    c9 = K.component(mods["ct"], 9, 950.0, 10.0, 12, seed=6)
    for fn in (rt.compute_TUD, lambda *p, **k: rt.compute_TUD_batch(*p, [{}], **k)):
        with pytest.raises(ValueError, match=r"molecule\(s\) \[9\]"):
            fn(XMIN, XMAX, **dict(kw, continuum=c9))
    a = e["a"]
    with pytest.raises(ValueError, match=r"molecule\(s\) \[9\]"):
        rt.compute_OD(XMIN, XMAX, DVOUT=DV, T=a["Ts"][1], P=a["Ps"][1], PL=a["PLs"][1], MF_VAL=a["MFs_VAL"][1], MF_ID=a["MFs_ID"],
                      line_table=e["tbl"], continuum=c9)


# ---- the stream contract of rtx_continuum_add (include/radtxfr_hip.h), as tests/test_gpu_stream_contract.py holds the other
# ---- entry points to it: on a side stream that is busy when the call is made ------------------------------------------------
def _stream_case(mods, v):
    """Variants 0, 1, 2: other layers, components, axis cuts and sizes. The optical-depth block is the payload (NaN until the
    stream has passed the delay, so a kernel that runs early adds to NaN); T, the axes and the tables are the host arrays."""
    import stream_cases as S
    eng, lib, _lib = mods["engine"], mods["lib"], mods["_lib"]
    name, nL, nC, off, n = (("fine", 3, 2, 0, K.N_AXIS), ("coarse", 1, 1, 5, 700), ("coarse", 2, 2, 1021, 333))[v]
    lay = K.layers(nL)
    lay["T"] = lay["T"] + 1.5 * v
    cont = K.continuum(mods["ct"], name, nC)
    tab, axes = cont.layer_tables(lay["T"], lay["P"], lay["PL"], lay["MF"], lay["ID"])
    grid = eng.Grid(*K.grid_args(name)).shard(off, n)
    host = dict(T=np.ascontiguousarray(lay["T"]), v0=np.array([x[0] for x in axes]), dv=np.array([x[1] for x in axes]),
                nn=np.array([x[2] for x in axes], dtype=np.int32), tab=np.ascontiguousarray(tab))
    od0 = S.dev(np.random.default_rng(70 + v).uniform(0.05, 3.0, (nL, n)).astype(np.float32))

    def call(d, h):
        _lib.check(lib.rtx_continuum_add(grid.byref(), nL, S.hp(h["T"]), nC, S.hp(h["v0"]), S.hp(h["dv"]), S.hp(h["nn"]), S.hp(h["tab"]),
                                         tab.shape[2], S.vp(d["od"]), n, eng._stream_ptr(), 0))
        return d["od"]
    # what the staging run writes into the host arrays once the call has returned: other finite values, so that a copy read
    # late would change the bits without handing the kernel a stencil outside its row
    scribble = dict(T=host["T"] + 40.0, v0=host["v0"] + 1.0, dv=host["dv"] * 1.5, nn=np.full(nC, 4, dtype=np.int32), tab=tab * 3.0 + 1.0)
    return S.Case(call, inputs={"od": od0}, host=host, scribble=scribble), od0, (cont, lay, grid)


@pytest.fixture(scope="module")
def stream_env(mods):
    import stream_cases as S
    e = dict(S=S, s1=torch.cuda.Stream(), s2=torch.cuda.Stream(), delay=S.Delay())
    yield e
    torch.cuda.synchronize()


def test_stream_order_asynchrony_and_staging(mods, stream_env):
    """1-3 of the stream contract. Behind a delay on s1, with the block NaN until s1 has passed the delay, the call gives the
    default-stream bits; the warmed call returns while the delay is pending; the host arrays may be overwritten as soon as
    it has returned. The default-stream result is OD + od_host within the pin."""
    S, s1, delay = stream_env["S"], stream_env["s1"], stream_env["delay"]
    case, od0, (cont, lay, grid) = _stream_case(mods, 0)
    other, _, _ = _stream_case(mods, 1)
    ref, _ = S.run_plain(case)
    got = S.as_float(ref[0]).astype(np.float64) - od0.double().cpu().numpy()
    want = cont.od_host(grid.axis(), lay["T"], lay["P"], lay["PL"], lay["MF"], lay["ID"])
    bound = K.TOL_PIN * want.max(axis=1, keepdims=True) + 2.0 ** -24 * (od0.double().cpu().numpy() + want)  # the pin and the sum's rounding
    assert np.all(np.abs(got - want) <= bound)
    warm, _ = S.run_plain(case, s1)   # grows the scratch of s1
    warm2, host_ms = S.run_plain(case, s1)
    D = delay.ms_for(host_ms, "rtx_continuum_add")
    S.run_plain(other, s1)            # the scratch of s1 now holds another call's tables
    out, pend, _ = S.run_delayed([case], s1, delay, D)
    S.run_plain(other, s1)
    out_s, pend_s, _ = S.run_delayed([case], s1, delay, D, scribble=True)
    torch.cuda.synchronize()
    print("rtx_continuum_add: returned before the delay had passed %s / %s, warmed host time %.3f ms, D %.0f ms" % (pend[0], pend_s[0], host_ms, D))
    for what, r in (("warm-up on s1", warm), ("warmed call on s1", warm2), ("behind the delay", out[0]), ("host arrays overwritten", out_s[0])):
        assert S.same_bits(r, ref), "%s: %s" % (what, S.describe(r, ref))
    assert pend[0] and pend_s[0], "the call returned only after %.0f ms of device work ahead of it on its stream had finished" % D


def test_two_calls_behind_one_delay_and_two_streams(mods, stream_env):
    """4 and 5. Delay, call A, call B (other tables, another size) on s1: each equals its solo reference, so B's tables did
    not reach A's kernel. Then delay and A on s1, B at once on s2, C on s1: the scratch is owned per (device, stream)."""
    S, s1, s2, delay = stream_env["S"], stream_env["s1"], stream_env["s2"], stream_env["delay"]
    cases = [_stream_case(mods, v)[0] for v in range(3)]
    refs = [S.run_plain(c)[0] for c in cases]
    assert not S.same_bits(refs[0], refs[1])
    host_ms = 0.0
    for st in (s1, s2):
        for c in cases:
            S.run_plain(c, st)
        host_ms = sum(S.run_plain(c, st)[1] for c in cases)
    D = delay.ms_for(host_ms, "rtx_continuum_add")
    out, _, _ = S.run_delayed(cases[:2], s1, delay, D)
    torch.cuda.synchronize()
    assert S.same_bits(out[0], refs[0]), "A: " + S.describe(out[0], refs[0])
    assert S.same_bits(out[1], refs[1]), "B: " + S.describe(out[1], refs[1])
    work = [S.fresh(c) for c in cases]
    torch.cuda.synchronize()
    res = [None, None, None]
    with torch.cuda.stream(s1):
        delay.enqueue(D)
        for i in (0, 2):
            S.fill(cases[i], work[i][0])
        res[0] = [x.clone() for x in S.flatten(S.issue(cases[0], *work[0])[0])]
    with torch.cuda.stream(s2):
        S.fill(cases[1], work[1][0])
        res[1] = [x.clone() for x in S.flatten(S.issue(cases[1], *work[1])[0])]
    with torch.cuda.stream(s1):
        res[2] = [x.clone() for x in S.flatten(S.issue(cases[2], *work[2])[0])]
    torch.cuda.synchronize()
    got = [S.finish(c, r) for c, r in zip(cases, res)]
    for name, g, w in zip("ABC", got, refs):
        assert S.same_bits(g, w), "%s: %s" % (name, S.describe(g, w))
