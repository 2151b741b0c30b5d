"""rtx_line_prep_dt + rtx_voigt_sum_dt (voigt_dT_kernel) on the GPU against the fp64 definition of tests/dT_cases.py,
point by point, at the smallest shapes where the kernel can go wrong, and its exact properties.

Metric, per layer: |got - ref| / max(|ref|, 1e-3 max|ref|); where the definition is exactly 0 (outside every window) the
result must be exactly 0.

Shapes: shards of 1, 63, 64, 65, 1023, 1024, 1025 and 2049 points (one row short / exact / one over, one tile short /
exact / one over, three tiles with a ragged last row), 1 and 3 layers at different (T, p), through the C ABI with
ld = n + 5 (the padding must stay NaN). Regimes (dT_cases.kernel_case; counted from the records by dT_cases.regimes and
asserted to occur): band lines with y >= 6, 1 <= y < 6 and y < 1, the |x| + y = 15 switch inside a row, centres left and
right of the grid whose windows cut in, windows that end mid-row, an empty window, a species with weight 0, two species
with different dln(weight)/dT.

TOL: 4 x the worst ratio measured over these cases on the first run on an MI355X (7.12e-6 at n = 65 with 3 layers; every
figure in profiles/dT_sum_accuracy.txt), the margin because the pattern of fp32 roundings moves with the inputs. The cap
set for this kernel is 2e-4, a tenth of test_gpu_jacobian.py's TOL_T; above it the answer is fp64 where the error arises,
not a wider bound."""
import ctypes as C

import numpy as np
import pytest

import dT_cases as D

pytestmark = pytest.mark.gpu

TOL = 2.85e-5  # 4 x 7.12e-6, the worst ratio of the first run (n = 65, 3 layers); the cap is 2e-4
FLOOR = 1e-3
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 2049]
PAD = 5


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    from radtxfr_amd import _lib, engine
    _lib.load()
    return engine


_REF = {}


def reference(n, nL):
    """(case, [nL][n] definition, per-layer records); computed once per shape and left unchanged."""
    if (n, nL) not in _REF:
        c = D.kernel_case(n, nL)
        rows, recs = [], []
        for k in range(nL):
            d, _, R = D.linesum_dT(c["tbl"], c["grid"], c["T"][k], c["p"][k], c["weight"], c["dlnw"])
            d.setflags(write=False)
            rows.append(d)
            recs.append(R)
        _REF[(n, nL)] = (c, np.stack(rows), recs)
    return _REF[(n, nL)]


def _species_rows(eng, lines, c, nL):
    w = np.array([[c["weight"][s]] * nL for s in lines.species], dtype=np.float64)
    dw = np.array([[c["dlnw"][s]] * nL for s in lines.species], dtype=np.float64)
    return w, dw


def run_abi(eng, c, g=None, pad=PAD, also_base=False):
    """The two entry points through the C ABI on shard g (default the case's), out_f32 [nL][n + pad] filled with NaN.
    Returns the [nL][n + pad] float32 array (and, with also_base, rtx_voigt_sum's output on the same records)."""
    import torch
    from radtxfr_amd import _lib
    lib = _lib.load()
    lines = eng.LineTable(c["tbl"])
    try:
        xmin, xmax, n_total, offset, n = g or c["grid"]
        grid = eng.Grid(xmin, xmax, n_total, offset, n)
        nL = c["T"].size
        w, dw = _species_rows(eng, lines, c, nL)
        nL_, env = eng._prologue_inputs(lines, c["T"], c["p"], w, None, None, None)
        dlnsw = np.ascontiguousarray(eng.species_dlnq_dT(lines.species, c["T"], weight=w) + dw)
        plan = lines.plan(nL, grid.n)
        st = eng._stream_ptr()
        _lib.check(lib.rtx_line_prep_dt(plan._h, lines._h, grid.byref(), nL, *(e[1] for e in env),
                                        dlnsw.ctypes.data_as(C.c_void_p), 1.0, 0.0, 0.0, 50.0, 0.0, 1.0, st))
        ld = grid.n + pad
        out = torch.full((nL, ld), float("nan"), dtype=torch.float32, device="cuda")
        _lib.check(lib.rtx_voigt_sum_dt(plan._h, grid.byref(), nL, eng._ptr(out), None, ld, st))
        base = None
        if also_base:
            base = torch.full((nL, ld), float("nan"), dtype=torch.float32, device="cuda")
            _lib.check(lib.rtx_voigt_sum(plan._h, grid.byref(), nL, eng._ptr(base), None, ld, st))
        torch.cuda.synchronize()
        return (out.cpu().numpy(), base.cpu().numpy()) if also_base else out.cpu().numpy()
    finally:
        lines.close()


def ratio(got, want):
    """The module's metric over [layers][points]; inf if a structural zero of the definition is not exactly 0."""
    got = np.asarray(got, dtype=np.float64)
    zero = want == 0.0
    if np.any(got[zero] != 0.0):
        return float("inf")
    mx = np.max(np.abs(want), axis=1, keepdims=True)
    den = np.maximum(np.abs(want), FLOOR * mx)
    e = np.where(zero, 0.0, np.abs(got - want) / np.where(den > 0.0, den, 1.0))
    return float(np.max(e))


@pytest.mark.parametrize("nL", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_against_definition(eng, n, nL):
    c, want, _ = reference(n, nL)
    got = run_abi(eng, c)
    assert got.shape == (nL, n + PAD) and np.all(np.isnan(got[:, n:])), "padding written"
    assert np.all(np.isfinite(got[:, :n]))
    r = ratio(got[:, :n], want)
    print("dT_sum n=%d layers=%d worst ratio %.3e" % (n, nL, r))
    assert r <= TOL, r


def test_regimes_occur():
    c, want, recs = reference(2049, 3)
    tot = {}
    for R in recs:
        w = np.array([c["weight"][(int(m), int(i))] for m, i in zip(R["P"]["M"], R["P"]["I"])])
        for k, v in D.regimes(R, c["grid"], w).items():
            tot[k] = tot.get(k, 0) + v
    for k in ("y_ge_6", "y_1_6", "y_lt_1", "switch_in_row", "centre_left", "centre_right", "ends_mid_row", "empty"):
        assert tot[k] > 0, (k, tot)
    assert 0.0 in c["weight"].values() and len(set(c["dlnw"].values())) == 3
    assert np.any(want[1] == 0.0) and np.any(want[1] != 0.0)  # the thin layer's windows leave points outside every window
    # the one-point and one-row shards still hold band lanes and the switch
    for n in (1, 64):
        c1, _, recs1 = reference(n, 3)
        w = np.array([c1["weight"][(int(m), int(i))] for m, i in zip(recs1[0]["P"]["M"], recs1[0]["P"]["I"])])
        r = [D.regimes(R, c1["grid"], w) for R in recs1]
        assert sum(v["y_ge_6"] + v["y_1_6"] + v["y_lt_1"] for v in r) > 0, (n, r)


def test_exact_properties(eng):
    """Two calls give identical bits; a tile-aligned shard equals the same slice of the full run bit for bit; exact 0.0
    outside every window; the base records after rtx_line_prep_dt are rtx_line_prep_profile's (rtx_voigt_sum's outputs
    compared bitwise)."""
    import torch
    from radtxfr_amd import _lib, dist
    lib = _lib.load()
    c, want, _ = reference(2049, 3)
    n = 2049
    a, base_dT = run_abi(eng, c, also_base=True)
    b = run_abi(eng, c)
    assert np.array_equal(a[:, :n].view(np.uint32), b[:, :n].view(np.uint32))
    assert np.all(a[:, :n][want == 0.0] == 0.0) and np.any(want == 0.0)
    tile = lib.rtx_voigt_tile_points()
    offs = dist.tile_aligned_bounds(n, 2, tile)
    assert 0 < offs[1] < n and offs[1] % tile == 0
    for r in range(2):
        o, m = int(offs[r]), int(offs[r + 1] - offs[r])
        g = (c["grid"][0], c["grid"][1], n, o, m)
        s = run_abi(eng, c, g=g)
        assert np.array_equal(s[:, :m].view(np.uint32), a[:, o:o + m].view(np.uint32)), r
    # the base records: rtx_voigt_sum after rtx_line_prep_profile
    lines = eng.LineTable(c["tbl"])
    try:
        w, _ = _species_rows(eng, lines, c, 3)
        ref32 = torch.full((3, n), float("nan"), dtype=torch.float32, device="cuda")
        eng.voigt_sum(lines, eng.Grid(*c["grid"]), c["T"], c["p"], w, out_f32=ref32)
        torch.cuda.synchronize()
        assert np.array_equal(ref32.cpu().numpy().view(np.uint32), base_dT[:, :n].view(np.uint32))
    finally:
        lines.close()


def test_engine_entry_and_refusals(eng):
    """engine.voigt_sum_dT gives the bits of the C ABI route; its default dlnw_dT is -1/T; rtx_voigt_sum_dt after another
    prologue on the same plan is refused, and so are an explicit axis and a qratio without its derivative."""
    import torch
    from radtxfr_amd import _lib
    lib = _lib.load()
    c, want, _ = reference(1025, 3)
    n = 1025
    via_abi = run_abi(eng, c)[:, :n]
    lines = eng.LineTable(c["tbl"])
    try:
        grid = eng.Grid(*c["grid"])
        w, dw = _species_rows(eng, lines, c, 3)
        out = torch.empty((3, n), dtype=torch.float32, device="cuda")
        eng.voigt_sum_dT(lines, grid, c["T"], c["p"], w, out, dlnw_dT=dw)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), via_abi.view(np.uint32))
        # default dlnw_dT = -1/T: the optical-depth weights
        d1 = torch.empty_like(out)
        d2 = torch.empty_like(out)
        eng.voigt_sum_dT(lines, grid, c["T"], c["p"], w, d1)
        eng.voigt_sum_dT(lines, grid, c["T"], c["p"], w, d2, dlnw_dT=np.broadcast_to(-1.0 / c["T"], (len(lines.species), 3)))
        torch.cuda.synchronize()
        assert torch.equal(d1, d2)
        # another prologue on the plan, then the dT sum
        base = torch.empty_like(out)
        eng.voigt_sum(lines, grid, c["T"], c["p"], w, out_f32=base)
        plan = lines.plan(3, n)
        rc = lib.rtx_voigt_sum_dt(plan._h, grid.byref(), 3, eng._ptr(out), None, n, eng._stream_ptr())
        assert rc != 0 and "not rtx_line_prep_dt" in lib.rtx_last_error().decode()
        with pytest.raises(TypeError, match="uniform Grid"):
            eng.voigt_sum_dT(lines, np.linspace(1000.0, 1001.0, n), c["T"], c["p"], w, out)
        with pytest.raises(ValueError, match="dlnq_dT"):
            eng.voigt_sum_dT(lines, grid, c["T"], c["p"], w, out, qratio=np.ones((len(lines.species), 3)), mass=np.ones(len(lines.species)))
    finally:
        lines.close()
