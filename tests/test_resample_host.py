"""CPU census of tests/resample_cases.py (the configurations of tests/test_gpu_resample_paths.py). Every case must reach the
path its name claims, computed from the kernels' index arithmetic restated here; the long-double references must agree
with independent ones (numpy.convolve through the oracle's smooth, scipy's CubicSpline, the oracle's reduceResolution)
to a design figure stated as a condition; the slips the case table claims to catch are injected into a restatement of
fir_reflect_kernel's loops and must each fail a case; the C ABI must refuse what it documents before it touches a device;
and the two defects of engine._reduce_plan (short axes, end knots off by one bit) are pinned at plan level. No GPU."""
import os

import numpy as np
import pytest

from oracle import cpu_ref as ref
from radtxfr_amd import _lib, engine

import resample_cases as RC

LD, U = RC.LD, RC.U


# ------------------------------------------------------------------------------------------------------ fir_reflect
def test_constants_are_the_sources():
    assert engine.SPL_END_MAX == RC.SPL_END_MAX and RC.FIR_TILE == RC.FIR_BLOCK * RC.FIR_PER_THREAD
    assert engine.SPL_END_GUARD == RC.SPL_EDGE  # the two 0.268^24 figures
    for line in ("if (jdx < 0) jdx = -jdx;", "if (jdx >= n) jdx = 2 * (n - 1) - jdx;", "for (int k0 = 0; k0 < n_taps; k0 += FIR_CHUNK) {",
                 "for (; k + FIR_PER_THREAD <= kc; k += FIR_PER_THREAD) {", "for (; k < kc; ++k) {",
                 "if (!(i - 1 - SPL_EDGE >= 0 && i + 2 + SPL_EDGE <= n - 1)) {", "const int jj = high_end ? m - 1 - j : j;"):
        assert line in RC.SRC, line  # the rules restated below: void if one of these lines changes


def test_fir_cases_reach_their_paths():
    reached = set()
    for name, c in RC.FIR_CASES.items():
        p = RC.fir_paths(c["n"], c["n_taps"], c["centre"])
        assert c["expect"] <= p, (name, c["expect"] - p)
        assert c["n_taps"] - 1 <= c["n"] and 0 <= c["centre"] < c["n_taps"] and c["n_taps"] <= RC.FIR_MAX_TAPS, name
        reached |= p
    assert reached == RC.FIR_PATHS, (RC.FIR_PATHS - reached, reached - RC.FIR_PATHS)
    for name in ("max_n%d" % (RC.FIR_MAX_TAPS - 1), "max_n%d" % RC.FIR_MAX_TAPS):
        o = RC.fir_outputs(name)
        n = RC.FIR_CASES[name]["n"]
        assert o.size == 64 and np.unique(o).size == 64 and set(range(8)) <= set(o) and set(range(n - 8, n)) <= set(o)
        assert all(e - 1 in o and e in o for e in range(RC.FIR_TILE, n, RC.FIR_TILE))


def fir_kernel_model(x, taps, centre, outputs, slip=None):
    """fir_reflect_kernel's loops in fp64 NumPy: tiles of FIR_TILE outputs, chunks of FIR_CHUNK taps, the span of a chunk
    staged with the reflection applied, taps taken in groups of FIR_PER_THREAD and then one by one. (An fma rounds once, a
    product and a sum twice: within the bound.) slip: "reflect", "chunk_base" or "tail", one off-by-one each."""
    n, n_taps = x.size, taps.size
    out = np.zeros(n)
    T, Ck, P = RC.FIR_TILE, RC.FIR_CHUNK, RC.FIR_PER_THREAD
    for i0 in range(0, n, T):
        if not np.any((outputs >= i0) & (outputs < i0 + T)):
            continue
        acc = np.zeros(T)
        for k0 in range(0, n_taps, Ck):
            kc = min(Ck, n_taps - k0)
            j = i0 + k0 - centre + np.arange(T + kc - 1) + (1 if slip == "chunk_base" and k0 else 0)
            j = np.where(j < 0, -j, j)
            j = np.where(j >= n, 2 * (n - 1) - j + (1 if slip == "reflect" else 0), j)
            j = np.where(j < 0, -j, j)
            s_x = x[np.clip(j, 0, n - 1)]
            k = 0
            while k + P <= kc:
                for u in range(P):
                    acc += taps[k0 + k + u] * s_x[k + u:k + u + T]
                k += P
            for k in range(k, kc - (1 if slip == "tail" else 0)):
                acc += taps[k0 + k] * s_x[k:k + T]
        out[i0:min(i0 + T, n)] = acc[:min(T, n - i0)]
    return out[outputs]


@pytest.fixture(scope="module")
def fir_refs():
    """(outputs, reference, absolute sum) of row 0 of every FIR case, computed once."""
    r = {}
    for name, c in RC.FIR_CASES.items():
        x, taps = RC.fir_inputs(name)
        o = RC.fir_outputs(name)
        r[name] = (o,) + RC.fir_reference(x[0], taps, c["centre"], o)
    return r


def _fir_model_fails(name, fir_refs, slip):
    c = RC.FIR_CASES[name]
    x, taps = RC.fir_inputs(name)
    o, want, ab = fir_refs[name]
    got = fir_kernel_model(x[0], taps, c["centre"], o, slip)
    return bool(np.any(np.abs(got.astype(LD) - want) > 2 * (c["n_taps"] + 1) * U * ab))


def test_fir_kernel_restated_is_the_reference_and_slips_fail(fir_refs):
    """The kernel's tile / chunk / group / tail arithmetic gives the reflect-padded convolution on every case (two roundings
    per tap here: 2 (n_taps + 1) u sum |t| |x|), and each off-by-one of the case table's header fails the cases named there."""
    small = [n for n in RC.FIR_CASES if not n.startswith("max_")]
    for name in RC.FIR_CASES:
        assert not _fir_model_fails(name, fir_refs, None), name
    caught = {s: {n for n in small if _fir_model_fails(n, fir_refs, s)} for s in ("reflect", "chunk_base", "tail")}
    paths = {n: RC.fir_paths(*[RC.FIR_CASES[n][k] for k in ("n", "n_taps", "centre")]) for n in small}
    high = {n for n in small if paths[n] & {"high", "double_low"} and RC.FIR_CASES[n]["n"] > 1}  # (-n -> n takes the high rule too)
    assert caught["reflect"] == high and any(n.startswith("tile_") for n in high)
    multi = {n for n in small if RC.FIR_CASES[n]["n_taps"] > RC.FIR_CHUNK}
    assert caught["chunk_base"] == multi and len(multi) >= 12
    tails = {n for n in small if RC.FIR_CASES[n]["n_taps"] % RC.FIR_CHUNK % RC.FIR_PER_THREAD}
    assert caught["tail"] == tails and {"tail_taps1", "tail_taps7", "chunk_%d_mid" % (RC.FIR_CHUNK + 1)} <= tails


def test_fir_reference_vs_oracle_smooth():
    """The long-double reference with engine.window_taps is the oracle's smooth (numpy.convolve on the reflect-padded row),
    plain and symmetrised, within the bound of two fp64 sums of M terms, 2 gamma_M sum |w| |x|."""
    x = RC.spectrum(700)
    for win, wl in (("hanning", 3), ("flat", 4), ("hamming", 11), ("bartlett", 120), ("blackman", 513), ("hanning", 700)):
        for sym in (False, True):
            taps, c = engine.window_taps(wl, win, symmetric=sym)
            got, ab = RC.fir_reference(x, taps, c)
            want = ref.smooth_sym(x, wl, win) if sym else ref.smooth(x, wl, win)
            M = taps.size
            assert want.shape == got.shape
            assert np.all(np.abs(got - want.astype(LD)) <= 2 * (M * U / (1 - M * U)) * ab * (2 if sym else 1)), (win, wl, sym)


# ---------------------------------------------------------------------------------------------------- cubic_resample
def test_cubic_resample_cases_reach_their_paths():
    for name, want in RC.CR_EXPECT.items():
        p = RC.cr_paths(name)
        assert want <= p, (name, want - p)
        c = RC.CR_CASES[name]
        y, x = RC.cr_inputs(name)
        assert x.size == c["n_out"] and y.shape == (c["rows"], c["n"]) and c["n"] >= 2 * RC.SPL_EDGE + 8
    n = RC.CR_CASES["cr_n56"]["n"]
    y, x = RC.cr_inputs("cr_n56")
    _, _, inside, i = RC.cubic_resample_reference(y[0], RC.CR_X0, RC.CR_H, x)
    assert n == 2 * RC.SPL_EDGE + 8 and set(i[inside]) <= set(range(25, 30)) and {25, 29} <= set(i[inside])
    assert set(RC.CR_CASES[k]["n_out"] for k in RC.CR_CASES) == {1, 255, 256, 257}


def test_cubic_resample_admission_slips_fail():
    """Either admission limit moved by one knot in either direction changes the set of outside points of cr_n56, cr_n57 and
    cr_n300: the unchecked form's NaN pattern (compared exactly on the GPU) would differ."""
    for name in ("cr_n56", "cr_n57", "cr_n300"):
        c = RC.CR_CASES[name]
        y, x = RC.cr_inputs(name)
        inside = RC.cubic_resample_reference(y[0], c["x0"], c["h"], x)[2]
        with np.errstate(invalid="ignore"):
            i = np.floor((x - c["x0"]) * (1.0 / c["h"]))
            for dlo, dhi in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                slipped = (i - 1 - RC.SPL_EDGE >= dlo) & (i + 2 + RC.SPL_EDGE <= c["n"] - 1 + dhi)
                assert not np.array_equal(slipped, inside), (name, dlo, dhi)


def test_truncated_cardinal_spline_vs_scipy():
    """25 or more knots inside, the truncated cardinal spline is scipy's not-a-knot spline through the whole row to
    0.268^24 max|y| (the figure of the kernel comment)."""
    from scipy.interpolate import CubicSpline
    n = 300
    rng = np.random.default_rng(3)
    y = rng.uniform(0.5, 2.0, n)
    t = np.r_[25.0, n - 27.0, rng.uniform(25.0, n - 26.0, 500)]
    x = RC.CR_X0 + t * RC.CR_H
    v, A, inside, _ = RC.cubic_resample_reference(y, RC.CR_X0, RC.CR_H, x)
    assert inside.all() and np.all(A >= np.abs(v))
    want = CubicSpline(RC.CR_X0 + RC.CR_H * np.arange(n), y)(x)
    assert np.max(np.abs(v - want.astype(LD))) <= 0.268 ** 24 * np.max(np.abs(y))


# --------------------------------------------------------------------------------------------------------- cubic_end
def test_cubic_end_cases_and_bound_constant():
    ms = {c["m"] for c in RC.CE_CASES.values()}
    assert {4, 5, 64, RC.SPL_END_MAX} <= ms and {c["n_out"] for c in RC.CE_CASES.values()} >= {1, 255, 256, 257, 600}
    for name, c in RC.CE_CASES.items():
        y, k, x = RC.ce_inputs(name)
        assert 0 <= c["i_first"] and c["i_first"] + c["m"] <= c["n"] < c["ld"] and x.size == c["n_out"] < c["ld_out"]
        assert k[0] in x and (c["n_out"] == 1 or (k[-1] in x and k[c["m"] // 2] in x)) and np.all((x >= k[0]) & (x <= k[-1]))
        lo = RC.cubic_end_reference(y[0, c["i_first"]:c["i_first"] + c["m"]], k, x, c["high_end"], c["whole_axis"])[1]
        assert c["n_out"] == 1 or (lo.min() == 0 and lo.max() == c["m"] - 2)  # the first and the last interval are evaluated
    bent = RC.ce_inputs("ce_m64_9_lo")[1]
    assert abs((bent[1] - bent[0]) / RC.H - 1.0) > 0.1 and abs((bent[-1] - bent[-2]) / RC.H - 1.0) < 1e-9  # bent first knots
    assert {c["i_first"] for c in RC.CE_CASES.values() if c["high_end"] == 0} > {0}
    assert 0 in {c["i_first"] for c in RC.CE_CASES.values() if c["high_end"] == 1}
    ratios = {name: RC.ce_ratio(name) for name in RC.CE_CASES}
    print("CE_RATIO max %.2f (%s), C = %.1f" % (max(ratios.values()), max(ratios, key=ratios.get), RC.ce_C()))
    assert 4.0 <= RC.ce_C() <= 64.0  # a handful of roundings of max|y|: the table has no ill-conditioned knot set


def test_cubic_end_mirror_slip_fails():
    """high_end read with the window one sample off (m-1-j -> m-j or m-2-j) leaves the bound at every ce_*_hi case."""
    for name, c in RC.CE_CASES.items():
        if not c["high_end"]:
            continue
        y, k, x = RC.ce_inputs(name)
        want = RC.ce_reference(name)[0]
        for d in (-1, 1):
            if not 0 <= c["i_first"] + d <= c["n"] - c["m"]:
                continue
            w = slice(c["i_first"] + d, c["i_first"] + d + c["m"])
            got = RC.cubic_end_reference(y[0, w], k, x, 1, c["whole_axis"])[0]
            assert np.max(np.abs(got - want)) > 1e6 * RC.ce_C() * U * 2.0, (name, d)


def test_end_spline_vs_scipy():
    """The restated system is scipy's CubicSpline with the same end conditions, to the bound the GPU test uses."""
    from scipy.interpolate import CubicSpline
    for name in ("ce_m5_rand_lo", "ce_m64_9_lo", "ce_m64_rand_hi", "ce_m%d_721_lo" % RC.SPL_END_MAX, "ce_m%d_rand_hi" % RC.SPL_END_MAX,
                 "ce_whole_m4", "ce_whole_m5", "ce_whole_m48", "ce_whole_m5_hi"):
        c = RC.CE_CASES[name]
        y, k, x = RC.ce_inputs(name)
        yw = y[0, c["i_first"]:c["i_first"] + c["m"]]
        bc = ("not-a-knot", "not-a-knot") if c["whole_axis"] else (("natural", "not-a-knot") if c["high_end"] else ("not-a-knot", "natural"))
        want = CubicSpline(k, yw, bc_type=bc)(x)
        got = RC.ce_reference(name)[0]
        assert np.max(np.abs(got - want.astype(LD))) <= RC.ce_C() * U * np.max(np.abs(yw)), name


# ----------------------------------------------------------------------------------------------- the engine's plan
def _plan_split(n, window, x_out=None):
    p = engine._reduce_plan(RC.X0, RC.H, n, window * RC.H, 4, "hanning", x_out, "cpu")
    return p[4], p[0].size - p[4] - p[5], p[5], (p[6][0] if p[6] else 0), p


def test_reduce_plan_splits():
    for (n, w), want in RC.REDUCE_EXPECT.items():
        assert _plan_split(n, w)[:4] == want, (n, w)
    for n, w in RC.REDUCE_SHORT + ((48, 3),):  # m == n: one launch, the whole-axis end condition, knots reflected at both ends
        p = _plan_split(n, w)[4]
        m, k_lo, k_hi, whole = p[6]
        assert whole and m == n and np.array_equal(k_lo.numpy(), k_hi.numpy())
        assert np.max(np.abs(k_lo.numpy() - ref.smooth_sym(RC.axis(n), w))) <= 4 * U * RC.X0
    assert not _plan_split(56, 3)[4][6][3] and not _plan_split(64, 9)[4][6][3]
    (n, w), (n2, w2) = RC.REDUCE_LONG
    for nn, ww, taps, m in ((n, w, 721, RC.SPL_END_MAX), (n2, w2, 513, 558)):
        n_lo, n_mid, n_hi, mm, p = _plan_split(nn, ww, RC.long_x_out(nn, ww))
        assert (n_lo, n_mid, n_hi, mm) == (201, 11, 201, m) and p[2].size == taps
    for case in RC.REDUCE_SPLITS:  # the explicit axis from the first to the last knot uses all three kernels too
        if case != (48, 3):
            n_lo, n_mid, n_hi, _, _ = _plan_split(*case, RC.full_x_out(*case))
            assert n_lo and n_mid and n_hi, case


def test_reduce_plan_end_knot_tolerance_and_refusals():
    """The oracle's own first and last smoothed knot are accepted although they lie a rounding outside the engine's;
    extrapolation and a window whose end spline does not fit are refused."""
    worst = 0.0
    for n, w in RC.REDUCE_LONG:
        xq = RC.long_x_out(n, w)
        p = _plan_split(n, w, xq)[4]
        k_lo, k_hi = p[6][1].numpy(), p[6][2].numpy()
        worst = max(worst, k_lo[0] - xq[0], xq[-1] - k_hi[-1])
        assert abs(k_lo[0] - xq[0]) <= 1e-9 * RC.H and abs(k_hi[-1] - xq[-1]) <= 1e-9 * RC.H
    assert worst > 0.0  # at least one end of these two cases is outside without the tolerance: the defect is exercised
    X = RC.axis(4000)
    for bad in (np.array([X[0] - 1.0, X[50]]), np.array([X[50], X[-1] + 1.0]), np.array([X[0] - 1e-6 * RC.H, X[50]])):
        with pytest.raises(NotImplementedError, match="extrapolation"):
            _plan_split(4000, 10, bad)
    w = RC.largest_window()
    assert _plan_split(4000, w, X[300:360])[3] <= RC.SPL_END_MAX
    with pytest.raises(NotImplementedError, match=r"local spline of \d+ knots") as e:
        _plan_split(4000, w + 1, X[300:360])
    assert "of %d knots" % (_plan_split(4000, w, X[300:360])[3] + 2) in str(e.value) and "supported up to %d" % RC.SPL_END_MAX in str(e.value)
    assert _plan_split(4000, w + 1)[4][6] is None  # the default axis stays in the interior: no end spline, no refusal


@pytest.mark.parametrize("n,window", RC.REDUCE_SPLITS + RC.REDUCE_SHORT + RC.REDUCE_LONG)
def test_engine_plan_with_long_double_kernels_vs_oracle(n, window):
    """The engine's plan with the three kernels replaced by their long-double references is the oracle's reduceResolution to
    1e-9 at every point: the default axis, and the explicit axis from the oracle's first to its last smoothed knot. The
    margin the GPU test has: the largest error here is 4e-12."""
    X, Y = RC.axis(n), RC.spectrum(n)
    dX = window * RC.H
    axes = [RC.long_x_out(n, window)] if (n, window) in RC.REDUCE_LONG else [ref.reduceResolution(X, Y, dX)[0], RC.full_x_out(n, window)]
    for xq in axes:
        want = ref.reduceResolution(X, Y, dX, X_out=xq)
        got = RC.model_reduce(Y[None, :], n, window, x_out=xq)[1][0]
        e = float(np.max(np.abs(got - want) / np.abs(want)))
        print("MODEL_ERR n%d w%d %.2e" % (n, window, e))
        assert e <= 1e-9, (n, window, e)


# ---------------------------------------------------------------------------------------------------------- the ABI
def test_abi_refusals_need_no_device():
    lib = _lib.load()
    header = open(os.path.join(RC.ROOT, "include", "radtxfr_hip.h")).read()
    for name, nargs in (("rtx_fir_reflect", 11), ("rtx_cubic_resample", 11), ("rtx_cubic_resample_unchecked", 11), ("rtx_cubic_end", 13)):
        assert name in _lib.PROTOTYPES and ("int %s(" % name) in header and hasattr(lib, name)
        assert len(_lib.PROTOTYPES[name][1]) == nargs
        assert header.split("int %s(" % name)[1].split(");")[0].count(",") == nargs - 1, name
    buf = np.zeros(16)
    p = buf.ctypes.data

    def refused(rc, text):
        assert rc != 0
        assert text in lib.rtx_last_error().decode(), lib.rtx_last_error()

    def fir(n=8, nt=3, c=1, ld_in=8, ld_out=8, rows=1, a=p, t=p, o=p):
        return lib.rtx_fir_reflect(a, 1, ld_in, rows, n, t, nt, c, o, ld_out, None)

    refused(fir(nt=0), "n_taps=0 outside [1,%d]" % RC.FIR_MAX_TAPS)
    refused(fir(n=10000, ld_in=10000, ld_out=10000, nt=RC.FIR_MAX_TAPS + 1), "n_taps=%d outside" % (RC.FIR_MAX_TAPS + 1))
    refused(fir(n=8, nt=10, c=0), "window of 10 taps is longer than the 8 samples")
    refused(fir(c=-1), "centre=-1 outside the 3 taps")
    refused(fir(c=3), "centre=3 outside the 3 taps")
    refused(fir(ld_in=7), "leading dimension smaller than the row")
    refused(fir(ld_out=7), "leading dimension smaller than the row")
    refused(fir(rows=65536), "n_rows=65536 too large")
    refused(fir(rows=0), "n_rows=0")
    refused(fir(n=0), "n=0")
    for kw in (dict(a=None), dict(t=None), dict(o=None)):
        refused(fir(**kw), "a required pointer is NULL")
    for fn in (lib.rtx_cubic_resample, lib.rtx_cubic_resample_unchecked):
        def cr(n=60, h=0.5, ld=60, ld_out=4, rows=1, y=p, x=p, o=p, fn=fn):
            return fn(y, ld, rows, n, 0.0, h, x, 4, o, ld_out, None)

        refused(cr(n=2 * RC.SPL_EDGE + 7), "the spline needs at least %d samples" % (2 * RC.SPL_EDGE + 8))
        refused(cr(h=0.0), "h=0")
        refused(cr(h=-1.0), "h=-1")
        refused(cr(h=float("nan")), "h=nan")
        refused(cr(ld=59), "leading dimension smaller than the row")
        refused(cr(ld_out=3), "leading dimension smaller than the row")
        refused(cr(rows=65536), "n_rows=65536")
        for kw in (dict(y=None), dict(x=None), dict(o=None)):
            refused(cr(**kw), "a required pointer is NULL")

    def ce(m=8, i_first=0, ld=16, ld_out=4, rows=1, y=p, k=p, x=p, o=p):
        return lib.rtx_cubic_end(y, ld, rows, i_first, m, 0, 0, k, x, 4, o, ld_out, None)

    refused(ce(m=3), "m=3 local knots outside [4,%d]" % RC.SPL_END_MAX)
    refused(ce(m=RC.SPL_END_MAX + 1, ld=1000), "m=%d local knots outside" % (RC.SPL_END_MAX + 1))
    refused(ce(i_first=-1), "outside the row")
    refused(ce(i_first=9), "local window [9, +8) outside the row")
    refused(ce(ld_out=3), "leading dimension smaller than the row")
    refused(ce(rows=65536), "n_rows=65536")
    for kw in (dict(y=None), dict(k=None), dict(x=None), dict(o=None)):
        refused(ce(**kw), "a required pointer is NULL")
