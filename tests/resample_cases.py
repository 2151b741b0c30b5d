"""Case tables and long-double references for the three kernels of radtxfr_amd/csrc/rtx_resample.hip (fir_reflect_kernel,
cubic_resample_kernel, cubic_end_kernel) and for the engine's reduceResolution plan. NumPy only: tests/test_resample_host.py
proves on the CPU that every case reaches the path it names and that the references agree with independent ones;
tests/test_gpu_resample_paths.py runs the cases on the device. The kernels' constants are read from the source.

Which case catches which slip (tests/test_resample_host.py injects each into a CPU restatement and sees these cases fail):
  reflection off by one (2(n-1)-j -> 2n-1-j)                   every FIR case with a "high" label: tile_*, tail_taps2.., chunk_*_mid
  chunk base off by one (k0 -> k0 + 1 in the staged span)       chunk_* with two or more chunks (second pass reads a shifted span)
  tail-tap loop off by one (k < kc -> k < kc - 1)               tail_taps1/2/3/5/7 (kc % FIR_PER_THREAD != 0), chunk_513_*, chunk_1025_*
  admission limits of cubic_resample off by one                 cr_n56 / cr_n57 / cr_n300: t exactly 25, just below 25, just below
                                                                n - 26 and exactly n - 26 sit on both sides of both limits
  high_end mirror off by one (m-1-j -> m-j or m-2-j)            every ce_*_hi case (non-uniform knots: a shifted window moves every value)
"""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "radtxfr_amd", "csrc", "rtx_resample.hip")).read()


def _define(name):
    return int(re.search(r"#define %s (\d+)\b" % name, SRC).group(1))


FIR_MAX_TAPS, FIR_BLOCK, FIR_PER_THREAD, FIR_CHUNK = (_define(k) for k in ("FIR_MAX_TAPS", "FIR_BLOCK", "FIR_PER_THREAD", "FIR_CHUNK"))
assert "#define FIR_TILE (FIR_BLOCK * FIR_PER_THREAD)" in SRC
FIR_TILE = FIR_BLOCK * FIR_PER_THREAD
SPL_K, SPL_EDGE, SPL_END_MAX = (_define(k) for k in ("SPL_K", "SPL_EDGE", "SPL_END_MAX"))

LD = np.longdouble
U = 2.0 ** -53
X0, H = 900.0, 0.002  # the axis of the engine cases and of the end-spline knots


def _rng(name):
    return np.random.default_rng(int.from_bytes(name.encode(), "little") % (2 ** 32))


def signed(rng, shape):
    """uniform(0.5, 2) times a random sign: sums cancel, the bounds are on absolute sums."""
    return rng.uniform(0.5, 2.0, shape) * rng.choice([-1.0, 1.0], shape)


# ------------------------------------------------------------------------------------------------------ fir_reflect
def reflect_index(j, n):
    """R(j): numpy.pad(mode="reflect") about the first and last sample, period 2(n-1); n == 1: always sample 0."""
    j = np.asarray(j, dtype=np.int64)
    if n == 1:
        return np.zeros_like(j)
    p = 2 * (n - 1)
    j = np.mod(j, p)
    return np.where(j > n - 1, p - j, j)


def fir_reference(x, taps, centre, outputs=None):
    """(out, absum) in long double at the given output indices (default: all): out[i] = sum_k taps[k] x[R(i + k - centre)]
    and absum[i] = sum_k |taps[k]| |x[R(.)]|. x holds the values the kernel reads (fp32-rounded for a float row)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    i = np.arange(n) if outputs is None else np.asarray(outputs, dtype=np.int64)
    out, ab = np.zeros(i.size, dtype=LD), np.zeros(i.size, dtype=LD)
    xl, tl = x.astype(LD), np.asarray(taps, dtype=np.float64).astype(LD)
    for k0 in range(0, tl.size, 256):  # blocks of taps: bounded memory, the sum is long double either way
        k = np.arange(k0, min(k0 + 256, tl.size))
        p = tl[k][None, :] * xl[reflect_index(i[:, None] + k[None, :] - centre, n)]
        out += p.sum(axis=1)
        ab += np.abs(p).sum(axis=1)
    return out, ab


def fir_paths(n, n_taps, centre):
    """The kernel's index arithmetic restated: which loops and which reflections a case runs."""
    chunks = -(-n_taps // FIR_CHUNK)
    kcs = [min(FIR_CHUNK, n_taps - c * FIR_CHUNK) for c in range(chunks)]
    p = {"tiles%d" % min(-(-n // FIR_TILE), 3), "chunks%d" % min(chunks, 4)}
    if n % FIR_TILE:
        p.add("ragged_tile")
    if any(kc >= FIR_PER_THREAD for kc in kcs):
        p.add("group")
    p.add("tail%d" % (kcs[-1] % FIR_PER_THREAD))
    if chunks > 1 and kcs[-1] < FIR_PER_THREAD:
        p.add("last_chunk_tail_only")
    j_lo, j_hi = -centre, n - 1 + n_taps - 1 - centre  # first tap of output 0, last tap of output n-1
    if j_lo < 0:
        p.add("low")
    if j_hi >= n:
        p.add("high")
    # the window of n_taps = n + 1 taps of one output never crosses both ends; the span that a workgroup stages for one
    # chunk does, and only then does one staging pass apply both reflections
    for i0 in range(0, n, FIR_TILE):
        for ci, kc in enumerate(kcs):
            first, last = i0 + ci * FIR_CHUNK - centre, min(i0 + FIR_TILE, n) - 1 + ci * FIR_CHUNK + kc - 1 - centre
            if first < 0 and last >= n:
                p.add("both_in_one_span")
    if -j_lo >= n and n > 1:
        p.add("double_low")  # -n -> n -> n - 2
    if j_hi > 2 * (n - 1) and n > 1:
        p.add("double_high")  # 2n - 1 -> -1 -> 1
    if n == 1:
        p.add("n1")
    return p


def _fir_case(n, n_taps, centre, dtype="f64", rows=3, expect=(), sampled=False):
    return dict(n=n, n_taps=n_taps, centre=centre, dtype=dtype, rows=rows, ld_in=n + 5, ld_out=n + 3, expect=set(expect), sampled=sampled)


def _build_fir_cases():
    T, Ck, P = FIR_TILE, FIR_CHUNK, FIR_PER_THREAD
    c = {}
    for n, tiles in ((T - 1, 1), (T, 1), (T + 1, 2), (2 * T + 1, 3)):  # tile edges, 7 taps
        for dt in ("f64", "f32"):
            c["tile_n%d_%s" % (n, dt)] = _fir_case(n, 7, 3, dt, expect={"tiles%d" % tiles, "low", "high", "tail%d" % (7 % P)})
    for nt in (1, 2, 3, 4, 5, 7, 8):  # the register group of FIR_PER_THREAD taps and the tail loop
        exp = {"tail%d" % (nt % P)} | ({"group"} if nt >= P else set())
        c["tail_taps%d" % nt] = _fir_case(300, nt, nt // 2, "f32" if nt in (3, 5) else "f64", expect=exp)
    for nt in (Ck - 1, Ck, Ck + 1, 2 * Ck, 2 * Ck + 1, 3 * Ck + 1):  # the chunk loop, second and later passes
        for cname, centre in (("c0", 0), ("mid", nt // 2), ("last", nt - 1)):
            chunks = -(-nt // Ck)
            exp = {"chunks%d" % min(chunks, 4), "tiles2", "tail%d" % ((nt - (chunks - 1) * Ck) % P)}
            exp |= {"mid": {"low", "high"}, "c0": {"high"}, "last": {"low"}}[cname]
            c["chunk_%d_%s" % (nt, cname)] = _fir_case(1600, nt, centre, expect=exp)
    for nt in (Ck + 1, 2 * Ck + 1):
        c["chunk_%d_mid_f32" % nt] = _fir_case(1600, nt, nt // 2, "f32", expect={"low", "high"})
    for nt in (3, 8, Ck + 1):  # n == n_taps - 1: both reflections in one staged span, and the double reflections
        c["both_%d_last" % nt] = _fir_case(nt - 1, nt, nt - 1, expect={"double_low", "low"})
        c["both_%d_c0" % nt] = _fir_case(nt - 1, nt, 0, expect={"double_high", "high"})
        c["both_%d_mid" % nt] = _fir_case(nt - 1, nt, nt // 2, expect={"both_in_one_span"})
    for nt, centre in ((1, 0), (2, 0), (2, 1)):
        for dt in ("f64", "f32"):
            c["n1_taps%d_c%d_%s" % (nt, centre, dt)] = _fir_case(1, nt, centre, dt, expect={"n1"})
    for n in (FIR_MAX_TAPS - 1, FIR_MAX_TAPS):  # the longest window the ABI takes; 64 sampled outputs
        c["max_n%d" % n] = _fir_case(n, FIR_MAX_TAPS, FIR_MAX_TAPS // 2, rows=1, sampled=True,
                                     expect={"chunks4", "tiles3", "low", "high"})
    return c


FIR_CASES = _build_fir_cases()
FIR_PATHS = {"tiles1", "tiles2", "tiles3", "ragged_tile", "chunks1", "chunks2", "chunks3", "chunks4", "group", "tail0", "tail1", "tail2",
             "tail3", "last_chunk_tail_only", "low", "high", "both_in_one_span", "double_low", "double_high", "n1"}


def fir_inputs(name):
    """(x [rows][n] float64 holding the values the kernel reads, taps [n_taps]) of a case; signed."""
    c = FIR_CASES[name]
    rng = _rng(name)
    x = signed(rng, (c["rows"], c["n"]))
    if c["dtype"] == "f32":
        x = x.astype(np.float32).astype(np.float64)
    return x, signed(rng, c["n_taps"])


def fir_outputs(name):
    """The output indices a case checks: all, or (sampled) the first and last 8, both sides of every tile edge, random ones."""
    c = FIR_CASES[name]
    n = c["n"]
    if not c["sampled"]:
        return np.arange(n)
    edges = [e + d for e in range(FIR_TILE, n, FIR_TILE) for d in (-1, 0)]
    fixed = np.unique(np.r_[np.arange(8), np.arange(n - 8, n), edges])
    rest = np.setdiff1d(np.arange(n), fixed)
    return np.sort(np.r_[fixed, _rng(name + "o").choice(rest, 64 - fixed.size, replace=False)])


# ---------------------------------------------------------------------------------------------------- cubic_resample
def cubic_resample_reference(y, x0, h, x):
    """(value, A, inside, i) in long double: the formula of the kernel comment, literally. t = fl(fl(x - x0) fl(1/h)) in fp64
    (the kernel's own abscissa), i = floor(t), f = t - i (exact); admitted when i - 1 - SPL_EDGE >= 0 and
    i + 2 + SPL_EDGE <= n - 1; c_j = sum_{|k| <= SPL_K} sqrt(3) z^|k| y[i - 1 + j + k], samples outside the row dropped;
    value = (1/6) sum_j b_j(f) c_j with the cubic B-spline basis; A = (1/6) sum_j b_j(f) sum_k |pre_|k| y|."""
    y = np.asarray(y, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    n = y.size
    with np.errstate(invalid="ignore"):
        t = (x - x0) * (1.0 / h)
        fl = np.floor(t)
        inside = np.isfinite(t) & (fl - 1 - SPL_EDGE >= 0) & (fl + 2 + SPL_EDGE <= n - 1)
    i = np.where(inside, fl, SPL_EDGE + 1).astype(np.int64)
    f = (np.where(inside, t, SPL_EDGE + 1) - i).astype(LD)
    s3 = np.sqrt(LD(3))
    pre1 = s3 * np.cumprod(np.r_[LD(1), np.full(SPL_K, s3 - 2, dtype=LD)])  # sqrt(3) z^k, k = 0 .. K
    k = np.arange(-SPL_K, SPL_K + 1)
    pre = pre1[np.abs(k)]
    yl = y.astype(LD)
    g = 1 - f
    b = [g ** 3, 3 * f ** 3 - 6 * f ** 2 + 4, 3 * g ** 3 - 6 * g ** 2 + 4, f ** 3]
    val, A = np.zeros(x.size, dtype=LD), np.zeros(x.size, dtype=LD)
    for j in range(4):
        a = i[:, None] - 1 + j + k[None, :]
        ok = (a >= 0) & (a < n)
        p = pre[None, :] * np.where(ok, yl[np.clip(a, 0, n - 1)], LD(0))
        val += b[j] * p.sum(axis=1)
        A += b[j] * np.abs(p).sum(axis=1)
    return val / 6, A / 6, inside, np.where(inside, i, -1)


CR_X0, CR_H = 900.0, 2.0 ** -9  # x0 + t h, x - x0 and (x - x0) / h are exact for the designed abscissae


def _cr_case(n, n_out, rows, h=CR_H, outside=True):
    return dict(n=n, n_out=n_out, rows=rows, ld=n + 3, ld_out=n_out + 3, x0=CR_X0, h=h, outside=outside)


CR_CASES = {
    "cr_n56": _cr_case(2 * SPL_EDGE + 8, 257, 3),  # only i = 25 .. 29 are admitted
    "cr_n57": _cr_case(2 * SPL_EDGE + 9, 257, 3),
    "cr_n300": _cr_case(300, 257, 3),
    "cr_n300_out1": _cr_case(300, 1, 1, outside=False),
    "cr_n300_out255": _cr_case(300, 255, 1),
    "cr_n300_out256": _cr_case(300, 256, 1),
    "cr_n300_h002": _cr_case(300, 257, 3, h=0.002),  # an h whose reciprocal rounds: t is what the kernel computes, not x / h
}


def cr_inputs(name):
    """(y [rows][n], x_out [n_out]). Designed abscissae first (t exactly SPL_EDGE + 1 and exactly n - SPL_EDGE - 3, t just
    below n - SPL_EDGE - 2, points where samples are dropped at either end, interior points; with `outside`: t just below
    SPL_EDGE + 1, t = n - SPL_EDGE - 2, NaN), the rest random over the admitted range, then shuffled (unsorted)."""
    c = CR_CASES[name]
    rng = _rng(name)
    n, x0, h = c["n"], c["x0"], c["h"]
    lo, hi = SPL_EDGE + 1, n - SPL_EDGE - 2  # admitted: lo <= t < hi
    at = lambda t: x0 + t * h
    pts = [at(lo)]
    if c["n_out"] > 1:
        pts += [at(hi - 1), np.nextafter(at(hi), -np.inf), at(lo + 0.5), at(hi - 0.25), at(0.5 * (lo + hi)), at(0.5 * (lo + hi) + 0.125),
                at(min(lo + 3, hi - 1) + 0.75)]
        if c["outside"]:
            pts += [np.nextafter(at(lo), -np.inf), at(hi), np.nan, at(0.0), at(n - 1.0), at(-3.0), at(n + 5.0)]
    pts = np.array(pts)
    x = np.r_[pts, at(rng.uniform(lo, hi - 1e-6, c["n_out"] - pts.size))]
    if c["n_out"] > 1:
        x = x[rng.permutation(x.size)]
    return rng.uniform(0.5, 2.0, (c["rows"], n)), x


def cr_paths(name):
    """What the abscissae of a case reach, from the reference's own t."""
    c = CR_CASES[name]
    y, x = cr_inputs(name)
    _, _, inside, i = cubic_resample_reference(y[0], c["x0"], c["h"], x)
    n = c["n"]
    with np.errstate(invalid="ignore"):
        t = (x - c["x0"]) * (1.0 / c["h"])
    p = set()
    ii, tt = i[inside], t[inside]
    for lab, cond in (("t_int_first", (ii == SPL_EDGE + 1) & (tt == ii)), ("t_int_last", (ii == n - SPL_EDGE - 3) & (tt == ii)),
                      ("just_below_end", (ii == n - SPL_EDGE - 3) & (tt > n - SPL_EDGE - 2 - 1e-9)),
                      ("drop_low", ii - 1 - SPL_K < 0), ("drop_high", ii + 2 + SPL_K > n - 1),
                      ("interior", (ii - 1 - SPL_K >= 0) & (ii + 2 + SPL_K <= n - 1))):
        if np.any(cond):
            p.add(lab)
    to = t[~inside]
    for lab, cond in (("out_just_below", (to < SPL_EDGE + 1) & (to > SPL_EDGE + 1 - 1e-9)), ("out_at_end", to == n - SPL_EDGE - 2),
                      ("out_nan", np.isnan(to))):
        if np.any(cond):
            p.add(lab)
    if np.any(np.diff(x[np.isfinite(x)]) < 0):
        p.add("unsorted")
    return p


CR_EXPECT = {
    "cr_n56": {"t_int_first", "t_int_last", "just_below_end", "drop_low", "drop_high", "out_just_below", "out_at_end", "out_nan", "unsorted"},
    "cr_n57": {"t_int_first", "t_int_last", "just_below_end", "drop_low", "drop_high", "out_just_below", "out_at_end", "out_nan", "unsorted"},
    "cr_n300": {"t_int_first", "t_int_last", "just_below_end", "drop_low", "drop_high", "interior", "out_just_below", "out_at_end", "out_nan",
                "unsorted"},
    "cr_n300_out1": {"t_int_first", "drop_low"},
    "cr_n300_out255": {"interior", "out_nan"},
    "cr_n300_out256": {"interior", "out_nan"},
    "cr_n300_h002": {"interior", "drop_low", "drop_high", "out_nan", "unsorted"},
}
# K of the bound K u A(q): 2 SPL_K + 1 = 81 fmas in the chain of a coefficient; SPL_K = 40 multiplications behind the last
# power of z; 8 for 1 - f, the basis polynomials, the four products, three sums and the factor 1/6
CR_K = (2 * SPL_K + 1) + SPL_K + 8


# --------------------------------------------------------------------------------------------------------- cubic_end
def cubic_end_reference(y_win, knots, x, high_end, whole_axis=0, dtype=LD):
    """cubic_end_kernel restated in `dtype` arithmetic (np.longdouble: the reference; np.float64: the same operations in
    the kernel's order and precision). Second-derivative form on the given knots; not-a-knot at local index 0 (M_0
    eliminated into row 1), natural at index m-1 (M_{m-1} = 0) or, whole_axis, not-a-knot there too; Thomas sweep; the
    interval by bisection (largest lo <= m-2 with knot[lo] <= x); the cubic of that interval. high_end mirrors the
    window and the abscissae (index m-1-j, sign flipped) so that the true end is index 0."""
    F = dtype
    m = len(knots)
    jj = np.arange(m)[::-1] if high_end else np.arange(m)
    sx = (-np.asarray(knots, dtype=np.float64)[jj] if high_end else np.asarray(knots, dtype=np.float64)[jj]).astype(F)
    sy = np.asarray(y_win, dtype=np.float64)[jj].astype(F)
    M, sc, sd = np.zeros(m, dtype=F), np.zeros(m, dtype=F), np.zeros(m, dtype=F)
    h0, h1 = sx[1] - sx[0], sx[2] - sx[1]
    hz, hy = sx[m - 1] - sx[m - 2], sx[m - 2] - sx[m - 3]
    dprev = (sy[1] - sy[0]) / h0
    cp, dp = F(0), F(0)
    two, six, one = F(2), F(6), F(1)
    for i in range(1, m - 1):
        hl, hr = sx[i] - sx[i - 1], sx[i + 1] - sx[i]
        dcur = (sy[i + 1] - sy[i]) / hr
        a, b, c = hl, two * (hl + hr), hr
        r = six * (dcur - dprev)
        if i == 1:
            b = b + h0 * (one + h0 / h1)
            c = c - h0 * h0 / h1
            a = F(0)
        if i == m - 2:
            if whole_axis:
                b = b + hz * (one + hz / hy)
                a = a - hz * hz / hy
            c = F(0)
        den = b - a * cp
        cp = c / den
        dp = (r - a * dp) / den
        sc[i], sd[i] = cp, dp
        dprev = dcur
    mn = F(0)
    for i in range(m - 2, 0, -1):
        mn = sd[i] - sc[i] * mn
        M[i] = mn
    M[0] = (one + h0 / h1) * M[1] - (h0 / h1) * M[2]
    if whole_axis:
        M[m - 1] = (one + hz / hy) * M[m - 2] - (hz / hy) * M[m - 3]
    xx = (-np.asarray(x, dtype=np.float64) if high_end else np.asarray(x, dtype=np.float64)).astype(F)
    lo, hi = np.zeros(xx.size, dtype=np.int64), np.full(xx.size, m - 1, dtype=np.int64)
    while np.any(hi - lo > 1):
        mid = (lo + hi) >> 1
        act = hi - lo > 1
        le = sx[mid] <= xx
        lo = np.where(act & le, mid, lo)
        hi = np.where(act & ~le, mid, hi)
    h, A, B = sx[lo + 1] - sx[lo], sx[lo + 1] - xx, xx - sx[lo]
    v = (M[lo] * A * A * A + M[lo + 1] * B * B * B) / (six * h) + (sy[lo] / h - M[lo] * h / six) * A + (sy[lo + 1] / h - M[lo + 1] * h / six) * B
    return v, lo


def _end_knots(source, m, high_end):
    """m knots: `source` = window length: engine._smoothed_axis_ends for that window on the axis X0 + i H (bent first or last
    knots); "rand": a random strictly ascending non-uniform set."""
    if source == "rand":
        return X0 + np.cumsum(_rng("knots%d%d" % (m, high_end)).uniform(0.25, 1.75, m)) * H
    from radtxfr_amd import engine
    taps, c = engine.window_taps(source, "hanning", symmetric=True)
    return engine._smoothed_axis_ends(X0, H, 4000, taps, c, m)[high_end]


def _ce_case(m, high_end, source, n_out, first_at_zero=None, whole_axis=0):
    n = m + 7  # the row is longer than the window
    i_first = (n - m if high_end else 0) if first_at_zero is None else (0 if first_at_zero else n - m)
    return dict(m=m, high_end=high_end, source=source, n_out=n_out, n=n, ld=n + 3, ld_out=n_out + 3, i_first=i_first, rows=3,
                whole_axis=whole_axis)


def _build_ce_cases():
    c = {}
    for m, src, n_out in ((4, 3, 255), (4, "rand", 1), (5, 3, 256), (5, "rand", 257), (64, 9, 600), (64, "rand", 257),
                          (SPL_END_MAX, 721, 600), (SPL_END_MAX, "rand", 257)):
        for he in (0, 1):
            c["ce_m%d_%s_%s" % (m, src, "hi" if he else "lo")] = _ce_case(m, he, src, n_out)
    c["ce_m5_rand_lo_shifted"] = _ce_case(5, 0, "rand", 255, first_at_zero=False)  # i_first and high_end are independent
    c["ce_m5_rand_hi_at0"] = _ce_case(5, 1, "rand", 255, first_at_zero=True)
    for m in (4, 5, 48):  # the whole axis: not-a-knot at both ends
        c["ce_whole_m%d" % m] = _ce_case(m, 0, "rand" if m != 48 else 3, 257, first_at_zero=True, whole_axis=1)
    c["ce_whole_m5_hi"] = _ce_case(5, 1, "rand", 257, whole_axis=1)
    return c


CE_CASES = _build_ce_cases()


def ce_inputs(name):
    """(y [rows][n] uniform in [0.5, 2], knots [m], x_out): abscissae exactly on the first, an interior and the last knot,
    the rest between knots; one point: the first knot."""
    c = CE_CASES[name]
    rng = _rng(name)
    k = _end_knots(c["source"], c["m"], c["high_end"])
    assert np.all(np.diff(k) > 0)
    on = np.array([k[0], k[c["m"] // 2], k[-1], k[1], k[-2]])[:min(5, c["n_out"])]
    x = np.r_[on, rng.uniform(k[0], k[-1], c["n_out"] - on.size)]
    return rng.uniform(0.5, 2.0, (c["rows"], c["n"])), k, x


def ce_reference(name, dtype=LD):
    """[rows][n_out] values of a case in `dtype` arithmetic."""
    c = CE_CASES[name]
    y, k, x = ce_inputs(name)
    w = slice(c["i_first"], c["i_first"] + c["m"])
    return np.stack([cubic_end_reference(y[r, w], k, x, c["high_end"], c["whole_axis"], dtype)[0] for r in range(c["rows"])])


@functools.lru_cache(maxsize=None)
def ce_ratio(name):
    """max |fp64 restatement - long double| / (u max|y| over the local window) of a case."""
    c = CE_CASES[name]
    y = ce_inputs(name)[0][:, c["i_first"]:c["i_first"] + c["m"]]
    d = np.abs(ce_reference(name, np.float64).astype(LD) - ce_reference(name, LD))
    return float(np.max(d / (U * np.max(np.abs(y), axis=1)[:, None])))


@functools.lru_cache(maxsize=None)
def ce_C():
    """C of the bound C u max|y|: 4 times the largest ce_ratio of the table (4: what hipcc may reassociate or contract)."""
    return 4.0 * max(ce_ratio(n) for n in CE_CASES)


# ------------------------------------------------------------------------------------ engine and shim against the oracle
def axis(n):
    return X0 + H * np.arange(n)


def spectrum(n, cols=None, seed=0):
    """1.2 + 0.5 sin + 0.1 uniform(-1, 1): positive, so pointwise relative error means something."""
    rng = np.random.default_rng(1000 + n + seed)
    i = np.arange(n)
    one = lambda ph: 1.2 + 0.5 * np.sin(0.05 * i + ph) + 0.1 * rng.uniform(-1.0, 1.0, n)  # noqa: E731
    return one(0.3) if cols is None else np.stack([one(0.3 + j) for j in range(cols)], axis=1)


# (window kind, window length) at n = 1600: odd and even lengths, all five kinds, one to four chunks, window == n
SMOOTH_N = 1600
SMOOTH_CASES = (("hanning", 3), ("flat", 4), ("hamming", FIR_CHUNK), ("bartlett", FIR_CHUNK + 1), ("blackman", 2 * FIR_CHUNK + 1),
                ("hanning", SMOOTH_N), ("flat", FIR_CHUNK + 1))

# (n, window): the splits named in the comments are proved by tests/test_resample_host.py
REDUCE_SPLITS = ((56, 3), (80, 3), (48, 3), (64, 9), (100, 21))
REDUCE_SHORT = ((20, 3), (30, 3), (40, 3))      # the whole axis is one end spline: not-a-knot at both ends
REDUCE_LONG = ((4000, 721), (1600, 512))        # 721 and 513 taps; X_out from the oracle's own first to its last smoothed knot
REDUCE_EXPECT = {(56, 3): (33, 1, 33, 55), (80, 3): (33, 33, 33, 55), (48, 3): (56, 0, 0, 48), (20, 3): (19, 0, 0, 20),
                 (30, 3): (32, 0, 0, 30), (40, 3): (45, 0, 0, 40)}  # (n_lo, n_mid, n_hi, m) on the default axis


def long_x_out(n, window):
    """The oracle's smoothed knots Xs[0..200], 11 mid-axis points, Xs[-201..-1]."""
    from oracle import cpu_ref as ref
    X = axis(n)
    Xs = ref.smooth_sym(X, window)
    return np.r_[Xs[:201], np.linspace(X[n // 2 - 5], X[n // 2 + 5], 11) + 0.3 * H, Xs[-201:]]


def full_x_out(n, window):
    """Every smoothed knot of the oracle and every midpoint between two: first knot to last knot."""
    from oracle import cpu_ref as ref
    Xs = ref.smooth_sym(axis(n), window)
    return np.sort(np.r_[Xs, 0.5 * (Xs[1:] + Xs[:-1])])


def largest_window():
    """The largest window whose end spline fits SPL_END_MAX knots: m = 2 ceil(w / 2) + 2 SPL_EDGE-guard figures, from the plan."""
    from radtxfr_amd import engine
    w = 3
    while max((w + 2) // 2 + 20, 27) + engine.SPL_END_GUARD + 2 + (w + 2) // 2 <= SPL_END_MAX:
        w += 1
    return w


def model_reduce(Y, n, window, x_out=None, N=4, win="hanning"):
    """The engine's reduceResolution with its plan (engine._reduce_plan on the CPU) and the long-double references above in
    place of the three kernels: Y [rows][n] -> (x_out, [rows][n_out] float64, (n_lo, n_mid, n_hi, m))."""
    from radtxfr_amd import engine
    x_out, _, taps, c, n_lo, n_hi, ends = engine._reduce_plan(X0, H, n, window * H, N, win, x_out, "cpu")
    n_mid = x_out.size - n_lo - n_hi
    out = np.zeros((Y.shape[0], x_out.size))
    for r in range(Y.shape[0]):
        ysm = fir_reference(Y[r], taps, c)[0].astype(np.float64)
        if n_mid:
            v, _, inside, _ = cubic_resample_reference(ysm, X0, H, x_out[n_lo:n_lo + n_mid])
            assert inside.all()
            out[r, n_lo:n_lo + n_mid] = v
        if n_lo:
            m, k_lo, k_hi, whole = ends
            out[r, :n_lo] = cubic_end_reference(ysm[:m], k_lo.numpy(), x_out[:n_lo], 0, int(whole))[0]
        if n_hi:
            out[r, x_out.size - n_hi:] = cubic_end_reference(ysm[n - m:], k_hi.numpy(), x_out[x_out.size - n_hi:], 1, 0)[0]
    return x_out, out, (n_lo, n_mid, n_hi, ends[0] if ends else 0)
