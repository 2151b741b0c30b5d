"""Every path of the sensor stage (radtxfr_amd/csrc/rtx_radiance.hip: rtx_apparent_radiance, rtx_ils, rtx_interp_knots,
rtx_band_moments, rtx_band_basis_moments, rtx_band_mix, rtx_pixel_cube) against fp64 NumPy, element by element.

The cases are the tables of tests/sensor_cases.py; tests/test_sensor_host.py proves on the CPU that each case reaches the
kernel, the block, the tail and the fallback it names. The references are written here from the formulas quoted in the
kernel comments (dense weights over the kernel's stated support, np.interp, direct sums) or taken from oracle/cpu_ref.py,
and are evaluated on the fp32-rounded inputs the kernel receives. Every input is strictly positive (emissivities in
[0, 1]); errors are relative at each element, never to the array maximum, except for the moment rows (TOL_L of the row's
largest entry: Lagrange basis values change sign). Outputs are pre-filled with NaN, so an element a kernel does not write
fails. Misaligned pointers are contiguous views that start one float into a larger buffer; strided Y is buf[:, :nS].

Bounds and the largest errors measured on an MI355X:
  radiance, general kernel   8 * 2^-24 = 4.8e-7 (seven fp32 roundings on non-negative terms, B rounded once from fp64)
  radiance, row kernel       TOL_L = 1e-5 (rtx_common.h states no bound for planck_f32)
  ILS, all forms             TOL_L at every (band, column)
  interp_knots               4 * 2^-24 * max(|f0|, |f1|)
  N, C, moment rows          TOL_L (rows: of the row's largest entry), exact zeros outside jrange, jrange exact
  band_mix                   (knots of the band + 2) * 2^-24 (one fp32 rounding per FMA, C and the division)
  pixel cube                 TOL_L
The largest error measured for each is in the docstring of its test."""
import ctypes as C

import numpy as np
import pytest

from oracle import cpu_ref as ref

import sensor_cases as SC

pytestmark = pytest.mark.gpu

TOL_L = 1e-5
EPS = 2.0 ** -24
TOL_RAD_GENERAL = 8 * EPS
TOL_INTERP = 4 * EPS


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    from radtxfr_amd import _lib, engine
    _lib.load()
    return engine


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f64(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def _nan32(shape, off=0, ld=None):
    """NaN-filled fp32 [rows][cols] whose first element lies `off` floats past a 16-byte boundary; ld: row stride."""
    import torch
    shape = tuple(shape)
    rows = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
    cols = shape[-1] if shape else 1
    ld = cols if ld is None else ld
    buf = torch.full((off + rows * ld + 4,), float("nan"), dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + rows * ld]
    if ld != cols:
        return v.view(rows, ld)[:, :cols]
    return v.view(shape)


def _dev32(a, off=0, ld=None):
    import torch
    a = np.ascontiguousarray(a, dtype=np.float32)
    t = _nan32(a.shape, off, ld)
    t.copy_(torch.as_tensor(a, device="cuda"))
    assert t.data_ptr() % 16 == 4 * (off % 4)
    return t


def _poison(*numels):
    """Leave NaN in the blocks the caching allocator hands out next (outputs the engine allocates with torch.empty)."""
    import torch
    ts = [torch.full((max(n, 1),), float("nan"), dtype=torch.float32, device="cuda") for n in numels]
    torch.cuda.synchronize()
    del ts


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.double().cpu().numpy()


def rel_each(got, want):
    """max over the elements of |got - want| / |want|; inf on a shape mismatch, a NaN or a non-positive reference."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not got.size:
        return 0.0
    if not (np.all(np.isfinite(got)) and np.all(want > 0.0)):
        return float("inf")
    return float(np.max(np.abs(got - want) / want))


def _report(group, name, err):
    print("SENSOR_ERR %s %s %.3e" % (group, name, err))


# ------------------------------------------------------------------------------------------- rtx_apparent_radiance
def _rad_run(eng, c):
    """(L, Ls or None) as float64 host arrays [nX][nE][nA][nT or 1]; through the engine unless an output is misaligned."""
    from radtxfr_amd import _lib
    d = SC.rad_inputs(c)
    nX, nE, nA, nT = c["nX"], c["nE"], c["nA"], c["nT"]
    X, Ts = _f64(d["X"]), _f64(d["Ts"])
    dT = _f64(d["dT"]) if nT else None
    emis = _dev32(d["emis"], c["off"]["emis"])
    tau, La, Ld = _dev32(d["tau"]), _dev32(d["La"]), _dev32(d["Ld"])
    shape = (nX, nE, nA, max(nT, 1))
    n = int(np.prod(shape))
    if c["off"]["L"] == 0 and c["off"]["Ls"] == 0:
        _poison(n, n)
        L, Ls = eng.apparent_radiance(X, emis, Ts, tau, La, Ld, dT=dT, return_Ls=c["Ls"])
    else:
        L = _nan32(shape, c["off"]["L"])
        Ls = _nan32(shape, c["off"]["Ls"]) if c["Ls"] else None
        _lib.check(_lib.load().rtx_apparent_radiance(_p(X), nX, _p(emis), nE, _p(Ts), nA, _p(tau), _p(La), _p(Ld), _p(dT), nT,
                                                     _p(L), _p(Ls), _stream()))
    assert tuple(L.shape) == shape
    return _host(L), (_host(Ls) if c["Ls"] else None)


def _rad_ref(c):
    d = SC.rad_inputs(c)
    f = lambda k: d[k].astype(np.float64)
    L, Ls = ref.compute_LWIR_apparent_radiance(d["X"], f("emis"), d["Ts"], f("tau"), f("La"), f("Ld"), dT=d["dT"], return_Ls=True)
    shape = (c["nX"], c["nE"], c["nA"], max(c["nT"], 1))
    return np.broadcast_to(L.reshape(L.shape + (1,) * (4 - L.ndim)), shape), np.broadcast_to(Ls.reshape(Ls.shape + (1,) * (4 - Ls.ndim)), shape)


@pytest.mark.parametrize("name", [n for n in SC.RAD_CASES if n != "gen_lds_refused"])
def test_apparent_radiance_paths(eng, name):
    """Row kernel (second q0 block, wave tail, grid stride, Ls on / off), the fallbacks on nE % 4 and on a misaligned
    emis / L / Ls, and the general kernel (dT with nT = 1, nA * nT around 256, TA = 256 walking several atmospheres per
    step, grid stride, chunks of one emissivity, a ragged last chunk, LDS over 64 KiB) against
    cpu_ref.compute_LWIR_apparent_radiance at every element.
    MEASURED: general kernel 1.8e-7 (gen_chunks_ragged; bound 4.8e-7); row kernel 2.5e-7 (row_nX32771; bound 1e-5)."""
    c = SC.RAD_CASES[name]
    L, Ls = _rad_run(eng, c)
    wL, wLs = _rad_ref(c)
    row = "rad_row" in c["expect"]
    tol = TOL_L if row else TOL_RAD_GENERAL
    e = rel_each(L, wL)
    eLs = rel_each(Ls, wLs) if c["Ls"] else 0.0
    _report("rad_row" if row else "rad_general", name, max(e, eLs))
    assert e <= tol and eLs <= tol, (name, e, eLs)


def test_apparent_radiance_refusal_and_zero_sizes(eng):
    """nA = nT = 200 does not fit the LDS staging: an error that says so, and the next small call is correct. Every zero
    size returns an empty result without an error."""
    import torch
    from radtxfr_amd import _lib
    with pytest.raises(_lib.RtxError, match="does not fit"):
        _rad_run(eng, SC.RAD_CASES["gen_lds_refused"])
    torch.cuda.synchronize()
    for name in ("gen_nAT3", "row_nE4_nX5"):
        c = SC.RAD_CASES[name]
        L, _ = _rad_run(eng, c)
        assert rel_each(L, _rad_ref(c)[0]) <= (TOL_L if name.startswith("row") else TOL_RAD_GENERAL), name
    e32 = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
    e64 = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")
    for nX, nE, nA, nT in SC.RAD_ZERO_SIZES:
        L, Ls = eng.apparent_radiance(e64(nX), e32(nX, nE), e64(nA), e32(nX, nA), e32(nX, nA), e32(nX, nA),
                                      dT=None if nT is None else e64(nT), return_Ls=True)
        torch.cuda.synchronize()
        assert L.numel() == 0 and Ls.numel() == 0 and L.shape[:3] == (nX, nE, nA)
        q = _p(e64(4))  # the library itself, with pointers that are not NULL: nothing to do, no error
        _lib.check(_lib.load().rtx_apparent_radiance(q, nX, q, nE, q, nA, q, q, q, None if nT is None else q, nT or 0, q, q, _stream()))
    c = SC.RAD_CASES["gen_nAT255"]
    assert rel_each(_rad_run(eng, c)[0], _rad_ref(c)[0]) <= TOL_RAD_GENERAL


# ------------------------------------------------------------------------------------------------------- rtx_ils
def ils_reference(X, Y, centre, sigma, kind):
    """Dense fp64 weights over the open support |x - c| < R (R = sigma; Gaussian, centred inside the grid: 7 sigma):
    tri() of radiative_transfer.py:1236-1239 or g() of ILS_MAKO.py:24, normalised. No point: 0/0 = NaN."""
    out = np.full((centre.size, Y.shape[1]), np.nan)
    for b, (c, s) in enumerate(zip(centre, sigma)):
        lo, hi = SC.ils_support(X, c, SC.ils_reach(kind, s))
        if hi > lo:
            z = (X[lo:hi] - c) / s
            w = 1.0 - np.abs(z) if kind == 0 else np.exp(-0.5 * z * z)
            out[b] = w @ Y[lo:hi] / w.sum()
    return out


def ils_err(got, want):
    """Relative error at every (band, column); inf unless NaN sits in exactly the rows where the reference has it."""
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return float("inf")
    ok = ~np.isnan(want)
    return rel_each(got[ok], want[ok])


_ILS_RUNS = {}


def _ils_small(eng, name):
    """(got, want) of a small-nS case, computed once per module: the layout tests compare cases with each other."""
    if name not in _ILS_RUNS:
        c = SC.ILS_SMALL[name]
        g, X = SC.ils_axis(c["axis"], c["nx"])
        centre, sigma = SC.ils_small_bands(X, c["kind"])
        Y = np.random.default_rng(17).uniform(0.5, 1.5, (c["nx"], c["nS"])).astype(np.float32)
        Yd = _dev32(Y, c["off"]["Y"], c["ldY"])
        assert Yd.stride(0) == c["ldY"] or c["nx"] == 1
        _poison(centre.size * c["nS"])
        out = eng.ils(c["kind"], Yd, _f64(centre), _f64(sigma), X=None if g else _f64(X), grid=eng.Grid(*g) if g else None)
        _ILS_RUNS[name] = (_host(out), ils_reference(X, Y.astype(np.float64), centre, sigma, c["kind"]))
    return _ILS_RUNS[name]


@pytest.mark.parametrize("name", list(SC.ILS_SMALL))
def test_ils_small_and_layouts(eng, name):
    """nS in {1, 4, 5, 16, 17, 20, 64, 68, 130} on a uniform grid and on an explicit uneven X (both point kernels, the
    column kernel, the float4 column kernel), nx in {1, 2}, a strided / odd-strided / misaligned Y, a triangle over one
    point, a triangle over none (NaN in its row only), the Gaussian on the strided and explicit-X cases.
    MEASURED: 3.4e-7 (tri_uniform_nS64; Gaussian 2.1e-7; bound 1e-5)."""
    got, want = _ils_small(eng, name)
    e = ils_err(got, want)
    _report("ils_small", name, e)
    if "ils_no_point" in SC.ILS_SMALL[name]["expect"]:
        assert np.isnan(want).all(axis=1).sum() == 1
    assert e <= TOL_L, (name, e)


def test_ils_layouts_agree(eng):
    """The same kernel on a strided and on a contiguous Y gives the same bits; another kernel on the same data stays
    within the tolerance."""
    for a, b in SC.ILS_SAME_BITS:
        ga, gb = _ils_small(eng, a)[0], _ils_small(eng, b)[0]
        assert np.array_equal(ga, gb, equal_nan=True), (a, b)
    for a, b in SC.ILS_SAME_DATA:
        assert ils_err(_ils_small(eng, a)[0], _ils_small(eng, b)[0]) <= TOL_L, (a, b)


def _rows_Y(nx):
    import torch
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234 + nx)
    Y = torch.rand((nx, SC.ILS_ROWS_NS), generator=gen, dtype=torch.float32, device="cuda") + 0.5
    cols = torch.as_tensor(SC.ILS_ROWS_COLS, device="cuda")
    return Y, _host(Y[:, cols])


def _rows_check(eng, Y, Ycols, X, g, centre, sigma, kind):
    """(error on the sampled columns, the whole result). The output block is left full of NaN before the call, so a column
    outside the sample that the kernels do not write fails too."""
    _poison(centre.size * SC.ILS_ROWS_NS)
    out = eng.ils(kind, Y, _f64(centre), _f64(sigma), grid=eng.Grid(*g))
    got = _host(out)
    assert np.all(np.isfinite(got))
    return ils_err(got[:, list(SC.ILS_ROWS_COLS)], ils_reference(X, Ycols, centre, sigma, kind)), got


@pytest.mark.parametrize("name", [n for n, c in SC.ILS_ROWS.items() if c["bands"] == "paths"])
def test_ils_one_pass(eng, name):
    """ils_rows_kernel + ils_rows_reduce_kernel at their smallest shape (nS = 460; nx = 65536: 64 full chunks; 65436: a
    ragged last chunk), triangle and Gaussian, with a custom band list: a band inside one chunk, supports that end on a
    chunk boundary, one row after and one row before it, a band over three chunks, one from row 0, one to the last row.
    Nine sampled columns (first, last, second float4 block) against dense fp64 weights.
    MEASURED: triangle 2.9e-7, Gaussian 4.7e-7 (gauss_nx65436; bound 1e-5)."""
    c = SC.ILS_ROWS[name]
    g, X = SC.ils_rows_axis(c["nx"])
    centre, sigma = SC.ils_rows_bands(X, c["kind"])
    Y, Ycols = _rows_Y(c["nx"])
    e, _ = _rows_check(eng, Y, Ycols, X, g, centre, sigma, c["kind"])
    _report("ils_rows", name, e)
    assert e <= TOL_L, (name, e)


def test_ils_one_pass_overflow_then_clean(eng):
    """14 triangles stacked on one chunk overflow the 12 slots: every band is redone per band. The flag is reset: the same
    call without overflow, made before and after the overflowing one on the same stream, gives the same bits (the
    one-pass form adds a band's chunks in a fixed order; redone per band, the rows are summed in another order, and the
    result would differ in the last bits).
    MEASURED: overflow 2.9e-7, next call 2.9e-7 (bound 1e-5)."""
    c = SC.ILS_ROWS["tri_overflow"]
    g, X = SC.ils_rows_axis(c["nx"])
    Y, Ycols = _rows_Y(c["nx"])
    e0, before = _rows_check(eng, Y, Ycols, X, g, *SC.ils_rows_bands(X, 0), 0)
    e1, redone = _rows_check(eng, Y, Ycols, X, g, *SC.ils_rows_overflow_bands(X), 0)
    e2, after = _rows_check(eng, Y, Ycols, X, g, *SC.ils_rows_bands(X, 0), 0)
    assert e0 <= TOL_L and np.array_equal(before, after)
    # the comparison can tell the two forms apart: the overflowing list redone per band is not the one-pass bits
    c14, s14 = SC.ils_rows_overflow_bands(X)
    _, one_pass = _rows_check(eng, Y, Ycols, X, g, c14[:12], s14[:12], 0)
    assert not np.array_equal(one_pass, redone[:12])
    _report("ils_rows", "tri_overflow", e1)
    _report("ils_rows", "tri_after_overflow", e2)
    assert e1 <= TOL_L and e2 <= TOL_L, (e1, e2)


# ------------------------------------------------------------------------------------------------- rtx_interp_knots
@pytest.mark.parametrize("name", list(SC.INTERP_CASES))
def test_interp_knots_paths(eng, name):
    """nx in {1, 63, 64, 65, 262209}, nS in {1, 4, 1024, 1028, 1026} (vector form with its second 256-float4 block, scalar
    form), a misaligned F, an explicit X through the C ABI, two knots, points left and right of all knots, grid points
    exactly on knots; against np.interp in fp64 (every column, or 16 sampled ones with the first and the last).
    MEASURED: 9.7e-8 of max(|f0|, |f1|) (nx262209; bound 2.4e-7)."""
    from radtxfr_amd import _lib, sensor
    c = SC.INTERP_CASES[name]
    g, X = SC.interp_axis(c)
    Xk = SC.interp_knots_axis(c["knots"])
    nk, nS = Xk.size, c["nS"]
    F = np.random.default_rng(23).uniform(0.2, 1.0, (nk, nS)).astype(np.float32)
    Fd = _dev32(F, c["off"]["F"])
    if g:
        _poison(c["nx"] * nS)
        out = sensor.interp_knots(eng.Grid(*g), Xk, Fd)
    else:
        out, Xd, Xkd = _nan32((c["nx"], nS)), _f64(X), _f64(Xk)
        _lib.check(_lib.load().rtx_interp_knots(None, _p(Xd), c["nx"], _p(Xkd), nk, _p(Fd), nS, _p(out), _stream()))
    got = _host(out)
    assert np.all(np.isfinite(got))
    cols = np.arange(nS) if nS <= 16 else np.unique(np.r_[0, nS - 1, nS - 2, 1023 % nS, np.linspace(0, nS - 1, 14).astype(int)])
    F64 = F.astype(np.float64)
    j = np.clip(np.searchsorted(Xk, X, side="right") - 1, 0, nk - 2)
    worst = 0.0
    for s in cols:
        want = np.interp(X, Xk, F64[:, s])
        bound = TOL_INTERP * np.maximum(F64[j, s], F64[j + 1, s])
        worst = max(worst, float(np.max(np.abs(got[:, s] - want) / bound)))
    _report("interp", name, worst * TOL_INTERP)
    assert worst <= 1.0, (name, worst)


# --------------------------------------------------------------------------------------------------- band moments
def _hat_matrix(x, Xk):
    """H[i][j]: np.interp's weight of knot j at x_i (end values held outside the knots); and the interval of x_i."""
    nk = Xk.size
    jj = np.searchsorted(Xk, x, side="right") - 1
    j0 = np.clip(jj, 0, nk - 2)
    f = np.clip((x - Xk[j0]) / (Xk[j0 + 1] - Xk[j0]), 0.0, 1.0)
    H = np.zeros((x.size, nk))
    H[np.arange(x.size), j0] += 1.0 - f
    H[np.arange(x.size), j0 + 1] += f
    return H, jj


def moments_reference(X, d, Xk, centre, sigma, kind, coef=None, node_span=1.0, Ts=None):
    """N_b = sum w, C_b = sum w (tau Ld + La), rows [nB][nk] = sum_i w tau g_i hat_j(nu_i) with g = B(nu, Ts) - Ld (Ts
    given: rtx_band_moments) or g = l_q((nu - c) / (node_span sigma)), q < Q, and g = Ld (rtx_band_basis_moments);
    jrange = first and last knot touched by a knot interval that holds a point of the band, (0, -1) without one."""
    tau, La, Ld = (d[k].astype(np.float64) for k in ("tau", "La", "Ld"))
    nB, nk = centre.size, Xk.size
    n_rows = 1 if Ts is not None else coef.shape[0] + 1
    N, Cc, rows, jr = np.zeros(nB), np.zeros(nB), np.zeros((n_rows, nB, nk)), np.zeros((nB, 2), dtype=np.int64)
    for b, (c, s) in enumerate(zip(centre, sigma)):
        lo, hi = SC.ils_support(X, c, s if kind == 0 else 14.0 * s)
        if hi == lo:
            jr[b] = (0, -1)
            continue
        x = X[lo:hi]
        z = (x - c) / s
        w = np.maximum(1.0 - np.abs(z), 0.0) if kind == 0 else np.exp(-0.5 * z * z) / (s * np.sqrt(2.0 * np.pi))
        H, jj = _hat_matrix(x, Xk)
        N[b], Cc[b] = w.sum(), (w * (tau[lo:hi] * Ld[lo:hi] + La[lo:hi])).sum()
        wt = w * tau[lo:hi]
        if Ts is not None:
            rows[0, b] = (wt * (ref.planckian(x, np.array([Ts]))[:, 0] - Ld[lo:hi])) @ H
        else:
            sn = (x - c) / (node_span * s)
            for q in range(coef.shape[0]):
                rows[q, b] = (wt * np.polyval(coef[q][::-1].astype(np.float64), sn)) @ H
            rows[-1, b] = (wt * Ld[lo:hi]) @ H
        jr[b] = (np.clip(jj.min(), 0, nk - 1), np.clip(jj.max() + 1, 0, nk - 1))
    return N, Cc, rows, jr


def _moments_run(eng, g, d, Xk, centre, sigma, kind, Q=None, node_span=1.0, Ts=None):
    """(N, C, rows [n_rows][nB][nk], jrange) of rtx_band_moments (Ts given) or rtx_band_basis_moments on a grid shard."""
    import torch
    from radtxfr_amd import _lib, sensor
    lib = _lib.load()
    grid = eng.Grid(*g)
    sl = slice(grid.offset, grid.offset + grid.n)
    tau, La, Ld = (_dev32(d[k][sl]) for k in ("tau", "La", "Ld"))
    nB, nk = centre.size, Xk.size
    n_rows = 1 if Ts is not None else Q + 1
    N, Cb, M = _nan32((nB,)), _nan32((nB,)), _nan32((n_rows, nB, nk))
    jr = torch.full((nB, 2), -77, dtype=torch.int32, device="cuda")
    Xkd, cd, sd = _f64(Xk), _f64(centre), _f64(sigma)
    if Ts is not None:
        _lib.check(lib.rtx_band_moments(kind, grid.byref(), _p(tau), _p(La), _p(Ld), float(Ts), _p(Xkd), nk, nB, _p(cd), _p(sd),
                                        _p(N), _p(Cb), _p(M), _p(jr), _stream()))
        coef = None
    else:
        coef = np.ascontiguousarray(sensor.chebyshev_lagrange(Q)[1], dtype=np.float32)
        _lib.check(lib.rtx_band_basis_moments(kind, grid.byref(), _p(tau), _p(La), _p(Ld), _p(Xkd), nk, nB, _p(cd), _p(sd), Q,
                                              coef.ctypes.data_as(C.c_void_p), float(node_span), _p(N), _p(Cb), _p(M[Q]), _p(M),
                                              _p(jr), _stream()))
    torch.cuda.synchronize()
    return _host(N), _host(Cb), _host(M), jr.cpu().numpy().astype(np.int64), coef


def _moments_err(got, want):
    """(error of N and C at every band, error of the rows in units of each row's largest entry); inf on a wrong jrange,
    a NaN or a non-zero outside jrange."""
    N, Cb, M, jr = got[:4]
    wN, wC, wM, wjr = want
    if not (np.array_equal(jr, wjr) and np.all(np.isfinite(N)) and np.all(np.isfinite(Cb)) and np.all(np.isfinite(M))):
        return float("inf"), float("inf")
    live = wN > 0
    if np.any(N[~live] != 0.0) or np.any(Cb[~live] != 0.0):
        return float("inf"), float("inf")
    e_nc = max(rel_each(N[live], wN[live]), rel_each(Cb[live], wC[live]))
    e_row = 0.0
    for b in range(N.size):
        outside = np.ones(M.shape[2], dtype=bool)
        outside[wjr[b, 0]:wjr[b, 1] + 1] = False
        if np.any(M[:, b, outside] != 0.0):
            return e_nc, float("inf")
        for r in range(M.shape[0]):
            mx = np.max(np.abs(wM[r, b]))
            if mx > 0.0:
                e_row = max(e_row, float(np.max(np.abs(M[r, b] - wM[r, b])) / mx))
    return e_nc, e_row


@pytest.mark.parametrize("knots,kind", SC.BBM_CASES)
def test_band_moments_paths(eng, knots, kind):
    """rtx_band_moments and rtx_band_basis_moments (Q in {1, 4, 6}), triangle and Gaussian, on 8192 grid points with
    custom bands: exactly 16, 17 and 33 knot intervals (one, two and three rounds: the knot shared by two rounds), knots
    denser than the grid (empty intervals), bands that stick out left of the first and right of the last knot, knots on
    grid points, a band without a grid point. N, C, every row of M / MB / MLd and jrange against direct fp64 sums. The
    Chebyshev nodes span the support (node_span 1 for the triangle, 14 for the Gaussian).
    MEASURED: N, C 1.7e-7 (dense knots, triangle); rows 6.5e-7 of the row's largest entry (knots on grid points, triangle);
    bound 1e-5."""
    X, Xk, d = SC.bbm_axis(), SC.bbm_knot_sets()[knots], SC.bbm_inputs()
    centre, sigma, _ = SC.bbm_bands(knots, kind)
    span = 1.0 if kind == 0 else 14.0
    got = _moments_run(eng, SC.BBM_GRID, d, Xk, centre, sigma, kind, Ts=SC.BBM_TS)
    errs = [_moments_err(got, moments_reference(X, d, Xk, centre, sigma, kind, Ts=SC.BBM_TS))]
    for Q in SC.BBM_Q:
        got = _moments_run(eng, SC.BBM_GRID, d, Xk, centre, sigma, kind, Q=Q, node_span=span)
        errs.append(_moments_err(got, moments_reference(X, d, Xk, centre, sigma, kind, coef=got[4], node_span=span)))
    _report("bbm_NC", "%s_kind%d" % (knots, kind), max(e[0] for e in errs))
    _report("bbm_rows", "%s_kind%d" % (knots, kind), max(e[1] for e in errs))
    assert max(e[0] for e in errs) <= TOL_L and max(e[1] for e in errs) <= TOL_L, errs


def test_band_moments_do_not_depend_on_the_shard(eng):
    """The kernel's header: a band's bits do not depend on where the grid shard starts. Two Grid.shard cuts that both hold
    all of a band (with the matching tau / La / Ld slices) and the whole grid give that band the same N, C, rows and
    jrange, bit for bit."""
    Xk, d = SC.bbm_knot_sets()["on_grid"], SC.bbm_inputs()
    b = SC.BBM_SHARD_BAND
    xmin, xmax, n_total = SC.BBM_GRID
    for kind in (0, 1):
        centre, sigma, _ = SC.bbm_bands("on_grid", kind)
        for kw in (dict(Ts=SC.BBM_TS), dict(Q=4, node_span=1.0 if kind == 0 else 14.0)):
            full = _moments_run(eng, SC.BBM_GRID, d, Xk, centre, sigma, kind, **kw)
            assert full[0][b] > 0
            for off, n in SC.BBM_SHARDS:
                part = _moments_run(eng, (xmin, xmax, n_total, off, n), d, Xk, centre, sigma, kind, **kw)
                assert part[0][b] == full[0][b] and part[1][b] == full[1][b], (kind, kw, off)
                assert np.array_equal(part[2][:, b], full[2][:, b]) and np.array_equal(part[3][b], full[3][b]), (kind, kw, off)


@pytest.mark.parametrize("nE", SC.MIX_NE)
def test_band_mix(eng, nE):
    """rtx_band_mix, nE in {1, 255, 256, 257}, with N and C and as the plain contraction (N = C = NULL); ranges of one knot,
    all knots and none. Every term is positive: one fp32 rounding per FMA, for C and for the division."""
    import torch
    from radtxfr_amd import _lib
    r = np.random.default_rng(41 + nE)
    nB, nk, jr = SC.MIX_NB, SC.MIX_NK, SC.MIX_JRANGE
    M, E = r.uniform(0.1, 1.0, (nB, nk)).astype(np.float32), r.uniform(0.1, 1.0, (nk, nE)).astype(np.float32)
    N, Cb = r.uniform(50.0, 150.0, nB).astype(np.float32), r.uniform(1.0, 5.0, nB).astype(np.float32)
    Md, Ed, Nd, Cd, jrd = _dev32(M), _dev32(E), _dev32(N), _dev32(Cb), torch.as_tensor(jr, device="cuda")
    for with_nc in (True, False):
        out = _nan32((nB, nE))
        _lib.check(_lib.load().rtx_band_mix(_p(Nd) if with_nc else None, _p(Cd) if with_nc else None, _p(Md), _p(jrd), nB, nk,
                                            _p(Ed), nE, _p(out), _stream()))
        got = _host(out)
        for b in range(nB):
            sl = slice(jr[b, 0], jr[b, 1] + 1)
            want = M[b, sl].astype(np.float64) @ E[sl].astype(np.float64)
            if with_nc:
                want = (want + float(Cb[b])) / float(N[b])
            if np.all(want == 0.0):
                assert np.all(got[b] == 0.0), (nE, b)
                continue
            e = rel_each(got[b], want)
            assert e <= (jr[b, 1] - jr[b, 0] + 3) * EPS, (nE, with_nc, b, e)


# ------------------------------------------------------------------------------------------------- rtx_pixel_cube
def cube_reference(c, d, kidx):
    """cube[b][p] = (C_b + sum_m f_pm (sum_q B(c_b + sigma_b s_q, T_p) tab[k_pm][q][b] - tab[k_pm][Q][b])) / N_b."""
    Q = c["Q"]
    f = lambda k: d[k].astype(np.float64)
    nu = d["centre"][:, None] + d["sigma"][:, None] * f("s_node")[None, :]  # [nB][Q], node_span 1
    with np.errstate(all="ignore"):
        B = ref.planckian(nu.ravel(), d["Tpix"]).reshape(c["nB"], Q, c["nPix"])
        tk = f("tab")[np.clip(kidx, 0, c["nEnd"] - 1)]  # [nPix][nMix][Q+1][nB]
        t = np.einsum("pmqb,bqp->pmb", tk[:, :, :Q, :], B) - tk[:, :, Q, :]
        acc = f("C")[None, :] + np.einsum("pm,pmb->pb", f("frac"), t)
        return (acc / f("N")[None, :]).T


def _cube_run(c, d, kidx):
    import torch
    from radtxfr_amd import _lib
    cube = _nan32((c["nB"], c["nPix"]))
    cd, sd, Td = _f64(d["centre"]), _f64(d["sigma"]), _f64(d["Tpix"])
    N, Cb, tab, frac = (_dev32(d[k]) for k in ("N", "C", "tab", "frac"))
    kd = torch.as_tensor(np.ascontiguousarray(kidx, dtype=np.int32), device="cuda")
    _lib.check(_lib.load().rtx_pixel_cube(c["nB"], c["Q"], _p(cd), _p(sd), 1.0, d["s_node"].ctypes.data_as(C.c_void_p), _p(N), _p(Cb),
                                          _p(tab), c["nEnd"], c["nPix"], c["nMix"], _p(kd), _p(frac), _p(Td), _p(cube), _stream()))
    return _host(cube)


@pytest.mark.parametrize("name", list(SC.CUBE_CASES))
def test_pixel_cube_paths(eng, name):
    """rtx_pixel_cube on tables built in NumPy: nPix in {1, 64, 65, 256, 257}, tables in LDS and in global memory, mixtures
    staged in the lanes and not; kidx with -1 and nEnd gives the bits of the clamped indices; one NaN temperature gives NaN
    in that pixel's column only while its workgroup takes the per-pixel path.
    MEASURED: 2.7e-7 (unstaged; bound 1e-5)."""
    c = SC.CUBE_CASES[name]
    d = SC.cube_inputs(c)
    got = _cube_run(c, d, d["kidx"])
    want = cube_reference(c, d, d["kidx"])
    if c["bad_kidx"]:
        assert (d["kidx"] == -1).any() and (d["kidx"] == c["nEnd"]).any()
        assert np.array_equal(got, _cube_run(c, d, np.clip(d["kidx"], 0, c["nEnd"] - 1)))
    ok = np.ones(c["nPix"], dtype=bool)
    if c["nan_pixel"] is not None:
        ok[c["nan_pixel"]] = False
        assert np.isnan(got[:, ~ok]).all() and np.isnan(want[:, ~ok]).all()
    e = rel_each(got[:, ok], want[:, ok])
    _report("cube", name, e)
    assert e <= TOL_L, (name, e)
