"""The response-table sensor kernels along the axis they are cut on (radtxfr_amd/csrc/rtx_srf.hip, rtx_srf_vjp.hip,
rtx_srf_jvp.hip): sensor.apply_srf, sensor.srf_moments, sensor.band_radiance_srf_fused, sensor.band_radiance_srf_vjp and
sensor.band_radiance_srf_jvp on the cases of tests/srf_axis_cases.py -- every axis length around the chunk (CH), sub-chunk
(64) and four-row cuts, grid shards, bands on the cuts, emissivity knots outside, on and between the rows of the cuts --
against the fp64 oracles the older tests of these units use, on the float32 inputs the kernels receive.
tests/test_srf_axis_host.py shows on the CPU which kernel paths these cases reach and that a kernel wrong in one of six
ways would miss the bounds here by a factor of 4 at least.

Bounds: the older tests' own, imported from them. apply_srf 1e-5 of max|Y| over the band's support (test_gpu_srf.TOL), its
denominators and N, C of the moments 1e-6 relative (test_gpu_srf_fused.py::test_moments); jrange exact; M exactly 0 outside
jrange and element by element within K_DE 2^-24 of its scale (srf_fused_cases.moments_scale; K_DE = 32 is what
test_gpu_sensor_vjp.py allows dE = sum g M / N, M's error and one rounding more); L 1e-5 of the band maximum
(test_gpu_srf_fused.worst); the adjoint by test_gpu_sensor_vjp.check_against_oracle; the tangent by
test_gpu_sensor_jvp.within at that module's k for all five groups moving.

The axis of a case is engine.Grid(parent).shard(off, n), also at off = 0: the points are then the parent's to the last bit
and a knot copied from the oracle's axis is a grid point for the kernels too. Every row the kernels read lies in a buffer
whose other floats are NaN (before the rows, behind them and in the padding columns of Y): a read outside the rows turns a
finite output NaN. MEASURED on an MI355X (profiles/srf_axis_paths.txt): in each test's docstring."""
import ctypes as C

import numpy as np
import pytest

import srf_fused_cases as FC
import sensor_jvp_cases as JC
import srf_axis_cases as AC
from test_gpu_srf import TOL as TOL_APPLY
from test_gpu_srf_fused import TOL as TOL_L, worst as worst_L
from test_gpu_sensor_vjp import K_DE, check_against_oracle
from test_gpu_sensor_jvp import within as within_jvp, k_of

pytestmark = pytest.mark.gpu

REL_NC = 1e-6  # test_gpu_srf_fused.py::test_moments, test_gpu_srf.py::test_parity_uniform
assert TOL_APPLY == 1e-5 and TOL_L == 1e-5


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    from radtxfr_amd import _lib, engine, sensor
    lib = _lib.load()
    return dict(torch=torch, lib=lib, engine=engine, sensor=sensor, CH=lib.rtx_srf_chunk_points())


def grid_of(env, off, n):
    return env["engine"].Grid(*FC.grid_tuple(env["CH"])).shard(off, n)


def guarded(env, a, lead=4):
    """A device view of the 1-D float32 array a that starts `lead` floats into a buffer of NaN (lead = 4: 16-byte aligned,
    as a fresh tensor is; 1, 2, 3: not) with NaN behind it as well."""
    torch = env["torch"]
    a = np.array(a, dtype=np.float32)  # a copy: the shared cases are read-only
    buf = torch.full((lead + a.size + 9,), float("nan"), dtype=torch.float32, device="cuda")
    buf[lead:lead + a.size] = torch.as_tensor(a, device="cuda")
    v = buf[lead:lead + a.size]
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 * lead) % 16
    return v


def guarded_Y(env, Y, col=4, pad=4):
    """A device view of Y [n][nS] float32 as columns col .. col + nS of a NaN buffer with nS + col + pad columns."""
    torch = env["torch"]
    n, nS = Y.shape
    buf = torch.full((n + 2, nS + col + pad), float("nan"), dtype=torch.float32, device="cuda")
    buf[1:n + 1, col:col + nS] = torch.as_tensor(np.array(Y, order="C"), device="cuda")
    return buf[1:n + 1, col:col + nS]


def rows_of(env, c, leads=(4, 4, 4)):
    return [guarded(env, c[k], lead) for k, lead in zip(("tau", "La", "Ld"), leads)]


def sensor_of(env, tables):
    return env["sensor"].Sensor.from_tables(tables)


# ------------------------------------------------------------------------------------------------------- the four units
def run_apply(env, off, n, tables, Y, by="grid", col=4, pad=4, packed=False):
    """apply_srf(wsum=True) -> (out, denominators) NumPy; by: the axis as grid= (the shard) or as X= (its points)."""
    torch, sensor = env["torch"], env["sensor"]
    Yd = torch.as_tensor(np.array(Y, order="C"), device="cuda") if packed else guarded_Y(env, Y, col, pad)
    kw = dict(grid=grid_of(env, off, n)) if by == "grid" else dict(X=torch.as_tensor(AC.axis(env["CH"], off, n), device="cuda"))
    _, out, den = sensor.apply_srf(sensor_of(env, tables), Yd, wsum=True, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), den.cpu().numpy()


def run_moments(env, off, n, c, tables=None, leads=(4, 4, 4)):
    torch, sensor = env["torch"], env["sensor"]
    tau, La, Ld = rows_of(env, c, leads)
    out = sensor.srf_moments(grid_of(env, off, n), tau, La, Ld, torch.as_tensor(np.array(c["Xk"]), device="cuda"), list(FC.TS_LIST),
                             sensor_of(env, c["tables"] if tables is None else tables))
    torch.cuda.synchronize()
    return tuple(v.cpu().numpy() for v in out)


def run_fused(env, off, n, c, nE, many, tables=None, leads=(4, 4, 4)):
    torch, sensor = env["torch"], env["sensor"]
    tau, La, Ld = rows_of(env, c, leads)
    E = torch.as_tensor(np.array(c["E"][:, :nE], order="C"), device="cuda")
    _, L = sensor.band_radiance_srf_fused(grid_of(env, off, n), tau, La, Ld, c["Xk"], E, AC.ts_of(many) if many else FC.TS_SCALAR,
                                          sensor_of(env, c["tables"] if tables is None else tables))
    torch.cuda.synchronize()
    return L.cpu().numpy()


def run_vjp(env, off, n, c, nE, many, g, leads=(4, 4, 4)):
    torch, sensor = env["torch"], env["sensor"]
    tau, La, Ld = rows_of(env, c, leads)
    E = torch.as_tensor(np.array(c["E"][:, :nE], order="C"), device="cuda")
    out = sensor.band_radiance_srf_vjp(grid_of(env, off, n), tau, La, Ld, c["Xk"], E, AC.ts_of(many) if many else FC.TS_SCALAR,
                                       sensor_of(env, c["tables"]), torch.as_tensor(np.array(g if many else g[0]), device="cuda"))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def run_jvp(env, off, n, c, nE, many, d, tables=None, leads=(4, 4, 4), d_leads=(4, 4, 4)):
    torch, sensor = env["torch"], env["sensor"]
    tau, La, Ld = rows_of(env, c, leads)
    E = torch.as_tensor(np.array(c["E"][:, :nE], order="C"), device="cuda")
    dt, da, dd = (guarded(env, d[k], lead) for k, lead in zip(("d_tau", "d_La", "d_Ld"), d_leads))
    d_Ts = d["d_Ts"] if many else np.asarray(d["d_Ts"])[0]
    L, dL = sensor.band_radiance_srf_jvp(grid_of(env, off, n), tau, La, Ld, c["Xk"], E, AC.ts_of(many) if many else FC.TS_SCALAR,
                                         sensor_of(env, c["tables"] if tables is None else tables), d_tau=dt, d_La=da, d_Ld=dd,
                                         d_Ts=d_Ts, d_emis=torch.as_tensor(np.array(d["d_E"]), device="cuda"))
    torch.cuda.synchronize()
    return L.cpu().numpy(), dL.cpu().numpy()


def report(unit, off, n, knots, value, bound):
    print("srf axis paths | %s | off=%d n=%d %s | %.3g | of a bound of %g" % (unit, off, n, knots, value, bound))


def check_apply(env, off, n):
    """Both load widths of srf_rows_kernel: eight columns (16-byte loads) and the first five of them (point by point)."""
    X, tables, dead, Y, want, den, sup = AC.case_apply(env["CH"], off, n)
    live = ~dead
    for nS in (8, 5):
        got, d = run_apply(env, off, n, tables, Y[:, :nS])
        assert got.shape == (len(tables), nS) and got.dtype == np.float32
        assert np.array_equal(np.isnan(got), np.repeat(dead[:, None], nS, axis=1))
        assert np.all(d[dead] == 0.0) and np.max(np.abs(d[live] / den[live] - 1.0)) <= REL_NC
        e = max(float(np.max(np.abs(got[b] - want[b, :nS])) / np.max(np.abs(Y[sup[b], :nS]))) for b in np.flatnonzero(live))
        report("apply_srf nS=%d" % nS, off, n, "-", e, TOL_APPLY)
        assert e <= TOL_APPLY


def check_moments(env, off, n, knots, c):
    N, Cb, M, jr = run_moments(env, off, n, c)
    live, nB, nk = ~c["dead"], len(c["tables"]), c["Xk"].size
    assert N.shape == (nB,) and M.shape == (3, nB, nk) and M.dtype == np.float32 and jr.dtype == np.int32
    assert np.all(N[c["dead"]] == 0.0) and np.all(Cb[c["dead"]] == 0.0)
    assert np.max(np.abs(N[live] / c["N"][live] - 1.0)) <= REL_NC
    assert np.max(np.abs(Cb[live] / c["C"][live] - 1.0)) <= REL_NC
    assert np.array_equal(jr, c["jrange"])
    for b in range(nB):
        assert not M[:, b, :max(jr[b, 0], 0)].any() and not M[:, b, jr[b, 1] + 1:].any()
    e = FC.moments_error(M, c["M"], c["Ma"])
    report("moments M", off, n, knots, e, K_DE)
    assert e <= K_DE
    return N


def check_case(env, off, n, knots, nE, many):
    """The moments, the fused radiances, the adjoint and the tangent of one case against their oracles."""
    CH = env["CH"]
    c = AC.case(CH, off, n, knots)
    what = "off=%d n=%d %s nE=%d nT=%d" % (off, n, knots, nE, 3 if many else 1)
    check_moments(env, off, n, knots, c)
    L = run_fused(env, off, n, c, nE, many)
    want = c["want"][:, :, :nE] if many else c["want"][1, :, :nE]
    e = worst_L(L, want, c["dead"])
    report("fused L", off, n, knots, e, TOL_L)
    assert e <= TOL_L
    g, o = AC.case_adjoint(CH, off, n, knots, nE, many)
    got = run_vjp(env, off, n, c, nE, many, g)
    assert got["G_tau"].shape == (n,) and got["emis"].shape == (c["Xk"].size, nE) and got["Ts"].shape == ((3,) if many else ())
    check_against_oracle(got, o, "srf axis paths | vjp | " + what)
    d, dL_want, scale = AC.case_tangent(CH, off, n, knots, nE, many)
    L2, dL = run_jvp(env, off, n, c, nE, many, d)
    assert np.array_equal(L2, L, equal_nan=True)
    within_jvp(dL.reshape(dL_want.shape), dL_want, scale, k_of(JC.GROUPS), c["dead"], "srf axis paths | jvp | " + what)


# ---------------------------------------------------------------------------------------------------------- tests
def cases_of(off, n):
    return [c for c in AC.all_cases(AC.CH_HOST) if c[:2] == (off, n)]


@pytest.mark.parametrize("n", AC.lengths(AC.CH_HOST))
def test_axis_lengths(env, n):
    """Each length at offset 0 with every knot set it takes (one knot inside / below, two knots that straddle the axis, all
    knots below / above, knots on the rows of the cuts, 300 knots between two adjacent rows), all four units.
    MEASURED on an MI355X, worst over the lengths: apply_srf 9.0e-7 (n = CH) and L 2.0e-7 of their 1e-5; in units of 2^-24 scale
    M 5.25 (n = 128, knots on the cut rows; k = 32), G_tau 2.44 (14), G_La 1.79 (3), G_Ld 0.61 (6), dTs 1.14 (20), dE 1.69 (32),
    dL 1.47 (32)."""
    assert env["CH"] == AC.CH_HOST, "the cases are cut for rtx_srf_chunk_points() = %d" % AC.CH_HOST
    check_apply(env, 0, n)
    for off, n_, knots, nE, many in cases_of(0, n):
        check_case(env, off, n_, knots, nE, many)


@pytest.mark.parametrize("off,n", AC.shards(AC.CH_HOST))
def test_shards(env, off, n):
    """Each shard (offsets 1, 63, 64, CH - 1, CH, CH + 1; 1, 65 and CH + 1 points) with the straddling knots, the knots on
    the cut rows and the 16 coarse knots, all four units, against the oracle on the sliced axis (half cells at the shard's
    own ends). MEASURED on an MI355X, worst over the shards: apply_srf 7.0e-7 and L 2.3e-7 of their 1e-5; in units of 2^-24
    scale M 3.74 (k = 32), G_tau 2.40 (14), G_La 1.46 (3), G_Ld 0.52 (6), dTs 1.80 (20), dE 1.42 (32), dL 1.62 (32)."""
    assert env["CH"] == AC.CH_HOST
    check_apply(env, off, n)
    for off_, n_, knots, nE, many in cases_of(off, n):
        check_case(env, off_, n_, knots, nE, many)


@pytest.mark.parametrize("off,n", AC.shards(AC.CH_HOST))
def test_shard_against_explicit_axis(env, off, n):
    """apply_srf with grid= the shard and with X= the shard's points: the same bits (grid_x is np.linspace's arithmetic, and
    the cells of both are the slice's own)."""
    X, tables, dead, Y, _, _, _ = AC.case_apply(env["CH"], off, n)
    for nS in (8, 5):
        a, da = run_apply(env, off, n, tables, Y[:, :nS], by="grid")
        b, db = run_apply(env, off, n, tables, Y[:, :nS], by="X")
        assert np.array_equal(a, b, equal_nan=True) and np.array_equal(da, db)
        assert np.all(np.isfinite(a[~dead]))


@pytest.mark.parametrize("n", (5, 65, AC.CH_HOST + 1))
def test_misaligned_rows_and_a_leading_dimension(env, n):
    """tau, La, Ld (and d_tau, d_La, d_Ld) as views 1, 2 and 3 floats into larger buffers: srfm_chunk_kernel's
    point-by-point loads; Y as the column view buf[:, 1 : 1 + nS] of a buffer with nS + 3 columns, nS in {4, 8}:
    srf_rows_kernel<false> with nS a multiple of 4 and ldY > nS; and (beyond the issue's list) Y at column 4 of nS + 8
    columns: srf_rows_kernel<true> with ldY > nS. Bit for bit the results of the same values in aligned, packed tensors;
    everything around the views is NaN."""
    CH, off = env["CH"], 0
    knots = "on_cuts"
    c = AC.case(CH, off, n, knots)
    nE, many = 3, True
    odd = (1, 2, 3)
    for a, b in zip(run_moments(env, off, n, c), run_moments(env, off, n, c, leads=odd)):
        assert np.array_equal(a, b)
    check_moments(env, off, n, knots, c)
    L = run_fused(env, off, n, c, nE, many)
    assert np.array_equal(L, run_fused(env, off, n, c, nE, many, leads=odd), equal_nan=True)
    g, _ = AC.case_adjoint(CH, off, n, knots, nE, many)
    v0, v1 = run_vjp(env, off, n, c, nE, many, g), run_vjp(env, off, n, c, nE, many, g, leads=odd)
    for k in v0:
        assert np.array_equal(v0[k], v1[k]) and np.all(np.isfinite(v1[k])), k
    d, _, _ = AC.case_tangent(CH, off, n, knots, nE, many)
    (L0, j0), (L1, j1) = run_jvp(env, off, n, c, nE, many, d), run_jvp(env, off, n, c, nE, many, d, leads=odd, d_leads=(3, 1, 2))
    assert np.array_equal(j0, j1, equal_nan=True) and np.array_equal(L0, L1, equal_nan=True) and np.array_equal(L0, L, equal_nan=True)
    assert np.all(np.isfinite(j1[:, ~c["dead"]]))
    X, tables, dead, Y, want, den, sup = AC.case_apply(CH, off, n)
    for nS in (4, 8):
        packed, dp = run_apply(env, off, n, tables, Y[:, :nS], packed=True)
        for col, pad in ((1, 2), (4, 4)):
            got, dg = run_apply(env, off, n, tables, Y[:, :nS], col=col, pad=pad)
            assert np.array_equal(got, packed, equal_nan=True) and np.array_equal(dg, dp), (nS, col)
        assert np.all(np.isfinite(packed[~dead])) and np.isnan(packed[dead]).all()


@pytest.mark.parametrize("off,n,knots", ((0, 5, "straddle"), (63, 65, "on_cuts")))
def test_everything_is_written(env, off, n, knots):
    """rtx_srf_moments through the C ABI into N, C, M and jrange filled with a sentinel: every element is overwritten, M is
    finite everywhere and exactly 0 outside jrange."""
    torch, lib, CH = env["torch"], env["lib"], env["CH"]
    c = AC.case(CH, off, n, knots)
    s = sensor_of(env, c["tables"])
    kx, kr = s.on_device("cuda")
    nB, nk, nT = len(s), c["Xk"].size, 3
    tau, La, Ld = rows_of(env, c)
    Xk = torch.as_tensor(np.array(c["Xk"]), device="cuda")
    N = torch.full((nB,), 7.0, dtype=torch.float32, device="cuda")
    Cb = torch.full((nB,), 7.0, dtype=torch.float32, device="cuda")
    M = torch.full((nT, nB, nk), 7.0, dtype=torch.float32, device="cuda")
    jr = torch.full((nB, 2), -77, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    Ts = np.array(FC.TS_LIST, dtype=np.float64)
    rc = lib.rtx_srf_moments(grid_of(env, off, n).byref(), p(tau), p(La), p(Ld), Ts.ctypes.data_as(C.c_void_p), nT, p(Xk), nk, nB,
                             s.knot_start.ctypes.data_as(C.c_void_p), p(kx), p(kr), p(N), p(Cb), p(M), p(jr),
                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0, lib.rtx_last_error()
    N, Cb, M, jr = (v.cpu().numpy() for v in (N, Cb, M, jr))
    assert np.all(N != 7.0) and np.all(Cb != 7.0) and np.all(M != 7.0) and np.all(jr != -77)
    assert np.all(np.isfinite(M)) and np.array_equal(jr, c["jrange"])
    for b in range(nB):
        assert not M[:, b, :max(jr[b, 0], 0)].any() and not M[:, b, jr[b, 1] + 1:].any()
    assert FC.moments_error(M, c["M"], c["Ma"]) <= K_DE


@pytest.mark.parametrize("off,n", ((0, 1), (0, 65), (0, AC.CH_HOST + 1), (64, AC.CH_HOST + 1)))
def test_purity(env, off, n):
    """On the new shapes: the same bits run to run for every unit; each band computed alone gives the bits it has among
    the others (N, C, M, jrange, L, dL and apply_srf's output; on the two CH + 1 axes across the launch-group boundary of 20
    bands); and the adjoint's N (sensor.srf_norms) is rtx_srf_moments' N bit for bit."""
    torch, sensor, CH = env["torch"], env["sensor"], env["CH"]
    knots = "on_cuts" if n >= 2 else "straddle"
    c = AC.case(CH, off, n, knots)
    nE, many = 3, True
    nB = len(c["tables"])
    assert (nB > AC.SLOTS) == (n == CH + 1)
    eq = lambda a, b: np.array_equal(a, b, equal_nan=True)
    mom = run_moments(env, off, n, c)
    assert all(eq(a, b) for a, b in zip(mom, run_moments(env, off, n, c)))
    L = run_fused(env, off, n, c, nE, many)
    assert eq(L, run_fused(env, off, n, c, nE, many))
    g, _ = AC.case_adjoint(CH, off, n, knots, nE, many)
    v0, v1 = run_vjp(env, off, n, c, nE, many, g), run_vjp(env, off, n, c, nE, many, g)
    assert all(eq(v0[k], v1[k]) for k in v0)
    d, _, _ = AC.case_tangent(CH, off, n, knots, nE, many)
    _, dL = run_jvp(env, off, n, c, nE, many, d)
    assert eq(dL, run_jvp(env, off, n, c, nE, many, d)[1])
    X, tables, dead, Y, _, _, _ = AC.case_apply(CH, off, n)
    out, den = run_apply(env, off, n, tables, Y)
    assert all(eq(a, b) for a, b in zip((out, den), run_apply(env, off, n, tables, Y)))
    for b in range(nB):
        one = [c["tables"][b]]
        Nb, Cb, Mb, jb = run_moments(env, off, n, c, tables=one)
        assert eq(Nb[0], mom[0][b]) and eq(Cb[0], mom[1][b]) and eq(Mb[:, 0], mom[2][:, b]) and eq(jb[0], mom[3][b]), b
        assert eq(run_fused(env, off, n, c, nE, many, tables=one)[:, 0], L[:, b]), b
        assert eq(run_jvp(env, off, n, c, nE, many, d, tables=one)[1][:, 0], dL[:, b]), b
        ob, db = run_apply(env, off, n, one, Y)
        assert eq(ob[0], out[b]) and eq(db[0], den[b]), b
    Nv = sensor.srf_norms(grid_of(env, off, n), sensor_of(env, c["tables"]), dev=torch.device("cuda"))
    torch.cuda.synchronize()
    Nv = Nv.cpu().numpy()
    assert Nv.dtype == np.float32 and np.array_equal(Nv, mom[0]) and np.array_equal(Nv == 0.0, c["dead"])
