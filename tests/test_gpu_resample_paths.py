"""Every path of smooth / reduceResolution's three kernels (radtxfr_amd/csrc/rtx_resample.hip: fir_reflect_kernel<float|double>,
cubic_resample_kernel checked and unchecked, cubic_end_kernel) through the C ABI, point by point against the long-double
references of tests/resample_cases.py, and the engine and the shim against the oracle (oracle/cpu_ref.py).

tests/test_resample_host.py proves on the CPU that each case reaches the tile, chunk, tap-group, reflection, admission and
split it names. Outputs are pre-filled with NaN and have a leading dimension larger than the row: an element a kernel does
not write fails, and every padding element must still be NaN. Inputs are padded with NaN too: a read outside the row or
outside the local window of the end spline fails. Every element is checked unless the case says sampled.

Bounds (u = 2^-53), and the largest error / bound measured on an MI355X (profiles/resample_paths_accuracy.txt):
  fir_reflect     (n_taps + 1) u sum_k |taps[k]| |x[R(.)]|   one fma per tap in tap order, and the store        MEASURED 0.47
  cubic_resample  K u A(q), K = 129 (see CR_BOUND_K below)                                                       MEASURED 0.026
  cubic_end       C u max|y| over the local window, C = 4 x the largest fp64-restatement / long-double ratio of
                  the case table (resample_cases.ce_C, 18.4)                                                      MEASURED 0.25
  engine, shim    |got - want| <= 1e-9 |want| at every point against the oracle's reduceResolution               MEASURED 0.019
  rt.smooth       2 gamma_M sum |w| |x| against the oracle's smooth (two fp64 sums of M terms)                   MEASURED 0.021
"""
import ctypes as C

import numpy as np
import pytest

from oracle import cpu_ref as ref

import resample_cases as RC

pytestmark = pytest.mark.gpu

LD, U = RC.LD, RC.U
# K of cubic_resample's bound K u A(q), A(q) = (1/6) sum_j b_j(f) sum_k |pre_|k| y|. A coefficient c_j is a chain of
# 2 SPL_K + 1 = 81 fmas, one rounding each: 81 u of its absolute sum. pre[k] is sqrt(3) z^k by k multiplications from two
# rounded literals: at most (2k + 1) u relative, on a term of weight |z|^k; for any y within a factor 4 of each other (the
# table's uniform [0.5, 2]) the weighted mean of 2k + 1 is below 9, and SPL_K = 40 is allowed. 1 - f, the two basis
# polynomials (two fmas and a product each), the cubes, four products, three sums and the factor 1/6: 8.
CR_BOUND_K = RC.CR_K
assert CR_BOUND_K == 129


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    from radtxfr_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def rt():
    from radtxfr_amd import radiative_transfer
    return radiative_transfer


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _padded(a, ld, dtype=None):
    """Device [rows][ld] holding a [rows][n] in its first n columns and NaN in the padding."""
    import torch
    a = np.asarray(a)
    t = torch.full((a.shape[0], ld), float("nan"), dtype=dtype or torch.float64, device="cuda")
    t[:, :a.shape[1]] = torch.as_tensor(a, device="cuda").to(t.dtype)
    return t


def _nan(rows, ld):
    import torch
    return torch.full((rows, ld), float("nan"), dtype=torch.float64, device="cuda")


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def _report(kernel, name, ratio):
    print("RESAMPLE_RATIO %s %s %.3e" % (kernel, name, ratio))


def _ok(lib, rc):
    assert rc == 0, lib.rtx_last_error().decode()


# ------------------------------------------------------------------------------------------------------ fir_reflect
@pytest.mark.parametrize("name", list(RC.FIR_CASES))
def test_fir_reflect_paths(lib, name):
    """Tile edges (n = FIR_TILE - 1, FIR_TILE, FIR_TILE + 1, 2 FIR_TILE + 1), the register group of FIR_PER_THREAD taps and
    its tail loop (1 .. 8 taps), one to four chunks of FIR_CHUNK taps with the window centred at its first, middle and last
    tap, n = n_taps - 1 (both reflections in one staged span; -n -> n - 2 and 2n - 1 -> 1), n = 1, FIR_MAX_TAPS taps (64
    sampled outputs), float and double rows, three rows with ld_in = n + 5 and ld_out = n + 3. Signed taps and samples.
    Row r of the three-row call has the bits of a one-row contiguous call.
    MEASURED: largest error / bound 0.47 (tail_taps1: one product, half an ulp of a bound of two); 0.0053 or less from 511 taps up."""
    import torch
    c = RC.FIR_CASES[name]
    n, rows = c["n"], c["rows"]
    x, taps = RC.fir_inputs(name)
    dt = torch.float64 if c["dtype"] == "f64" else torch.float32
    xd, out = _padded(x, c["ld_in"], dt), _nan(rows, c["ld_out"])
    _ok(lib, lib.rtx_fir_reflect(_p(xd), int(c["dtype"] == "f64"), c["ld_in"], rows, n, taps.ctypes.data, taps.size, c["centre"], _p(out),
                                 c["ld_out"], _stream()))
    got = _host(out)
    assert np.isnan(got[:, n:]).all() and np.isfinite(got[:, :n]).all(), name
    o = RC.fir_outputs(name)
    worst = 0.0
    for r in range(rows):
        want, ab = RC.fir_reference(x[r], taps, c["centre"], o)
        worst = max(worst, float(np.max(np.abs(got[r, o].astype(LD) - want) / ((c["n_taps"] + 1) * U * ab))))
    _report("fir_reflect", name, worst)
    assert worst <= 1.0, (name, worst)
    if rows > 1:
        for r in range(rows):
            one, o1 = torch.as_tensor(x[r:r + 1], device="cuda").to(dt).contiguous(), _nan(1, n)
            _ok(lib, lib.rtx_fir_reflect(_p(one), int(c["dtype"] == "f64"), n, 1, n, taps.ctypes.data, taps.size, c["centre"], _p(o1), n, _stream()))
            assert np.array_equal(_host(o1)[0], got[r, :n]), (name, r)


# ---------------------------------------------------------------------------------------------------- cubic_resample
@pytest.mark.parametrize("name", list(RC.CR_CASES))
def test_cubic_resample_paths(lib, name):
    """n = 2 SPL_EDGE + 8 (only i = 25 .. 29 admitted), + 9 and 300; n_out = 1, 255, 256, 257; one and three rows with
    ld = n + 3, ld_out = n_out + 3; t exactly integer at the first and last admitted knot, just below the upper limit, points
    whose out-of-row samples are dropped at either end, interior points, unsorted; outside: just below the lower limit, on
    the upper limit, NaN, far outside. Unchecked form: NaN at exactly the outside elements, K u A(q) everywhere else. Checked
    form: an error with a message for the same abscissae, none without the outside ones, and then the same bits.
    MEASURED: largest error / bound 0.026 (cr_n300; 3.4 u A)."""
    c = RC.CR_CASES[name]
    n, rows, n_out = c["n"], c["rows"], c["n_out"]
    y, x = RC.cr_inputs(name)
    yd, xd, out = _padded(y, c["ld"]), _dev(x), _nan(rows, c["ld_out"])
    args = lambda xx, oo, ld_out: (_p(yd), c["ld"], rows, n, c["x0"], c["h"], _p(xx), xx.numel(), _p(oo), ld_out, _stream())  # noqa: E731
    _ok(lib, lib.rtx_cubic_resample_unchecked(*args(xd, out, c["ld_out"])))
    got = _host(out)
    assert np.isnan(got[:, n_out:]).all(), name
    worst = 0.0
    inside = None
    for r in range(rows):
        want, A, inside, _ = RC.cubic_resample_reference(y[r], c["x0"], c["h"], x)
        assert np.array_equal(np.isnan(got[r, :n_out]), ~inside), (name, r)
        worst = max(worst, float(np.max(np.abs(got[r, :n_out][inside].astype(LD) - want[inside]) / (CR_BOUND_K * U * A[inside]))))
    _report("cubic_resample", name, worst)
    assert worst <= 1.0, (name, worst)
    assert bool((~inside).any()) == c["outside"]
    if c["outside"]:
        chk = _nan(rows, c["ld_out"])
        assert lib.rtx_cubic_resample(*args(xd, chk, c["ld_out"])) != 0
        assert "an output abscissa lies within %d samples" % (RC.SPL_EDGE + 2) in lib.rtx_last_error().decode()
    xin = _dev(x[inside])
    chk = _nan(rows, xin.numel() + 3)
    _ok(lib, lib.rtx_cubic_resample(*args(xin, chk, xin.numel() + 3)))
    chk = _host(chk)
    assert np.isnan(chk[:, xin.numel():]).all() and np.array_equal(chk[:, :xin.numel()], got[:, :n_out][:, inside]), name


# --------------------------------------------------------------------------------------------------------- cubic_end
@pytest.mark.parametrize("name", list(RC.CE_CASES))
def test_cubic_end_paths(lib, name):
    """m = 4, 5, 64 and SPL_END_MAX local knots, low and high end (mirrored window), the window at the start and at the end
    of a longer row, n_out = 1, 255, 256, 257, 600, three rows with leading dimensions; knots from the engine's smoothed
    axis (bent first or last knots) and random non-uniform ones; abscissae exactly on the first, an interior and the last
    knot and between knots; the whole-axis form (not-a-knot at both ends) at m = 4, 5, 48. Samples outside the local window
    are NaN. Bound C u max|y|, C from the reference side alone (resample_cases.ce_C).
    MEASURED: largest error / bound 0.25 (ce_m768_rand_hi): the kernel has the bits of the fp64 restatement."""
    c = RC.CE_CASES[name]
    m, rows, n_out = c["m"], c["rows"], c["n_out"]
    y, k, x = RC.ce_inputs(name)
    w = slice(c["i_first"], c["i_first"] + m)
    ynan = np.full_like(y, np.nan)
    ynan[:, w] = y[:, w]
    yd, kd, xd, out = _padded(ynan, c["ld"]), _dev(k), _dev(x), _nan(rows, c["ld_out"])
    _ok(lib, lib.rtx_cubic_end(_p(yd), c["ld"], rows, c["i_first"], m, c["high_end"], c["whole_axis"], _p(kd), _p(xd), n_out, _p(out),
                               c["ld_out"], _stream()))
    got = _host(out)
    assert np.isnan(got[:, n_out:]).all() and np.isfinite(got[:, :n_out]).all(), name
    want = RC.ce_reference(name)
    bound = RC.ce_C() * U * np.max(np.abs(y[:, w]), axis=1)[:, None]
    worst = float(np.max(np.abs(got[:, :n_out].astype(LD) - want) / bound))
    _report("cubic_end", name, worst)
    assert worst <= 1.0, (name, worst)


# ----------------------------------------------------------------------------------- engine and shim against the oracle
def _rel_each(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.all(np.isfinite(got)) and np.all(want > 0.0)
    return float(np.max(np.abs(got - want) / want))


@pytest.mark.parametrize("window,wl", RC.SMOOTH_CASES)
def test_smooth_vs_oracle(rt, window, wl):
    """rt.smooth at n = 1600 with windows of 3, 4, FIR_CHUNK, FIR_CHUNK + 1, 2 FIR_CHUNK + 1 and n taps, odd and even, all
    five window kinds, against the oracle's smooth at every point.
    MEASURED: largest error / bound 0.021 (hamming, 512 taps); hanning(3) is the identity and gives 0."""
    from radtxfr_amd import engine
    x = RC.spectrum(RC.SMOOTH_N)
    got, want = rt.smooth(x, wl, window), ref.smooth(x, wl, window)
    taps, c = engine.window_taps(wl, window)
    assert taps.size == wl and got.shape == want.shape == x.shape
    ab = RC.fir_reference(x, taps, c)[1]
    worst = float(np.max(np.abs(got - want) / (2 * (wl * U / (1 - wl * U)) * ab).astype(np.float64)))
    _report("smooth", "%s_%d" % (window, wl), worst)
    assert worst <= 1.0, (window, wl, worst)


@pytest.mark.parametrize("n,window", RC.REDUCE_SPLITS + RC.REDUCE_SHORT + RC.REDUCE_LONG)
def test_reduce_resolution_vs_oracle(rt, n, window):
    """rt.reduceResolution and engine.reduce_resolution against the oracle, |got - want| <= 1e-9 |want| at every point: the
    splits (56, 3) 33/1/33, (80, 3) 33/33/33, (48, 3) whole axis, (64, 9), (100, 21); the short axes (20, 3), (30, 3), (40, 3),
    where the whole axis is one spline with the reference's not-a-knot condition at both ends; (4000, 721) with 721 taps and
    768 local knots and (1600, 512) with 513 taps, on an X_out from the oracle's own first smoothed knot to its last. On
    the default axis, on the explicit axis of every knot and midpoint, with a 2-D Y, on float32 device rows; the cached,
    unchecked form has the same bits.
    MEASURED: largest error 1.9e-11 ((48, 3)); (20, 3) 1.1e-11, (30, 3) 4e-16, (40, 3) 9e-12; long windows 1e-13. (The shim's
    h = (X[-1] - X[0]) / (n - 1) carries the rounding of X's end points, 1e-13 in a knot spacing of 0.002: with the exact h
    the CPU model of tests/test_resample_host.py gives 3e-16 on the short axes.)"""
    import torch
    from radtxfr_amd import engine
    X, Y = RC.axis(n), RC.spectrum(n, cols=3)
    dX = window * RC.H
    worst = 0.0
    if (n, window) in RC.REDUCE_LONG:
        axes = [RC.long_x_out(n, window)]
    else:
        xo_ref = ref.reduceResolution(X, Y[:, 0], dX)[0]
        xo, yo = rt.reduceResolution(X, Y, dX)
        if xo.size == xo_ref.size:  # (the reference's point count can flip by one with the rounding of its own convolution)
            assert np.max(np.abs(xo - xo_ref)) <= 1e-9 * RC.H
            worst = _rel_each(yo, ref.reduceResolution(X, Y, dX, X_out=xo))
        axes = [xo_ref, RC.full_x_out(n, window)]
    for xq in axes:
        want = ref.reduceResolution(X, Y, dX, X_out=xq)
        worst = max(worst, _rel_each(rt.reduceResolution(X, Y, dX, X_out=xq), want))
        worst = max(worst, _rel_each(rt.reduceResolution(X, Y[:, 1], dX, X_out=xq), want[:, 1]))
    # float32 device rows, as rtx_tud writes them
    Y32 = Y.astype(np.float32)
    rows = torch.as_tensor(Y32.T.copy(), device="cuda")
    h = float((X[-1] - X[0]) / (n - 1))
    xq = axes[-1]
    _, out = engine.reduce_resolution(rows, float(X[0]), h, n, dX, x_out=xq)
    worst = max(worst, _rel_each(_host(out).T, ref.reduceResolution(X, Y32.astype(np.float64), dX, X_out=xq)))
    xa, a = engine.reduce_resolution(rows, float(X[0]), h, n, dX)
    xb, b = engine.reduce_resolution_cached(rows, float(X[0]), h, n, dX)
    torch.cuda.synchronize()
    assert np.array_equal(xa, xb) and torch.equal(a, b) and bool(torch.isfinite(a).all())
    worst = max(worst, _rel_each(_host(a).T, ref.reduceResolution(X, Y32.astype(np.float64), dX, X_out=xa)))
    _report("reduce", "n%d_w%d" % (n, window), worst / 1e-9)
    assert worst <= 1e-9, (n, window, worst)


def test_reduce_resolution_refusals(rt):
    """One window past the largest whose end spline fits SPL_END_MAX knots, with X_out in an end region: NotImplementedError
    naming the knot count; the largest one works there. Extrapolation below the first smoothed knot still raises."""
    n = 4000
    X, Y = RC.axis(n), RC.spectrum(n)
    w = RC.largest_window()
    xq = X[300:360]
    assert _rel_each(rt.reduceResolution(X, Y, w * RC.H, X_out=xq), ref.reduceResolution(X, Y, w * RC.H, X_out=xq)) <= 1e-9
    with pytest.raises(NotImplementedError, match=r"local spline of %d knots .*supported up to %d" % (RC.SPL_END_MAX + 2, RC.SPL_END_MAX)):
        rt.reduceResolution(X, Y, (w + 1) * RC.H, X_out=xq)
    with pytest.raises(NotImplementedError, match="extrapolation"):
        rt.reduceResolution(X, Y, 10 * RC.H, X_out=np.array([X[0] - 1.0, X[50]]))
