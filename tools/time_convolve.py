#!/usr/bin/env python3
"""Slit-function convolution (hapi.convolveSpectrumSame -> rtx_fir_same) per call:
  (a) the C3 axis (5.5 M points at 0.001 cm^-1) under the default AF_wing = 10 (20 001 or 20 002 taps), Resolution 0.1,
      for 1 spectrum and for a batch of 8;
  (b) the sizes of the golden cases (tests/make_golden_spectra.py: 12 000 points x 2002 taps; 500 points x 2002 taps).
Kernel time by HIP events, the call through the shim by a host clock around a device synchronise, achieved fp64 FLOP/s
(2 n_out m per row: the multiply-adds of the direct sum, zero-padded ends included) against the vector FMA peak, a sampled
check of the timed result against host dot products, and numpy.convolve on the CPU for the same call at a reduced size.
    python tools/time_convolve.py [--points 5500000] [--cpu-points 131072]"""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from radtxfr_amd import engine, hapi

# MI355X vector FMA peak: 256 CUs x 4 SIMDs x 2.4 GHz x 64 FLOP/clk/SIMD = 157.3 TFLOP/s in fp32; v_fma_f64 issues at half
# that rate (AMD's published fp64 vector figure for the part, 78.6 TFLOP/s)
PEAK_F32_VECTOR, PEAK_F64_VECTOR = 157.3e12, 78.6e12

ap = argparse.ArgumentParser()
ap.add_argument("--points", type=int, default=5500000)
ap.add_argument("--cpu-points", type=int, default=131072)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
assert torch.cuda.is_available(), "needs a GPU"
rng = np.random.default_rng(3)


def spectrum(n, rows):
    y = rng.uniform(0.0, 1.0, (n, rows)) * np.exp(rng.normal(size=(n, rows)))
    return y[:, 0].copy() if rows == 1 else y


def sampled_check(a, taps, scale, first, y, n_samples=64):
    """y[i] against the plain dot product on the host, under 2 gamma_M scale sum |a| |taps| (tests/test_gpu_spectra.py)."""
    n, m = a.size, taps.size
    g = m * 2.0 ** -53 / (1 - m * 2.0 ** -53)
    worst = 0.0
    for i in np.unique(np.concatenate([[0, y.size - 1], rng.integers(0, y.size, n_samples - 2)])):
        q = i + first
        k = np.arange(max(0, q - n + 1), min(m, q + 1))
        ref = np.dot(taps[k], a[q - k]) * scale
        rhs = 2 * g * scale * np.dot(np.abs(taps[k]), np.abs(a[q - k]))
        worst = max(worst, abs(y[i] - ref) / rhs)
    assert worst <= 1.0, worst
    return worst


def run(label, n, rows, wing):
    Om = 600.0 + 0.001 * np.arange(n)
    cs = spectrum(n, rows)
    kw = dict(Resolution=0.1, AF_wing=wing, SlitFunction=hapi.SLIT_GAUSSIAN)
    d = torch.as_tensor(cs, device="cuda")
    for _ in range(2):  # warm up: code object, the slit's device copy
        _, Y, _, _, slit = hapi.convolveSpectrumSame(Om, d, **kw)
    torch.cuda.synchronize()
    t_call = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        _, Y, _, _, slit = hapi.convolveSpectrumSame(Om, d, **kw)
        torch.cuda.synchronize()
        t_call.append(time.perf_counter() - t0)
    m = slit.size
    step = float(Om[1] - Om[0])
    first = engine.same_window(n, m)[0]
    rows_dev = (d[None] if rows == 1 else d.t()).contiguous()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t_k = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        ev[0].record()
        out = engine.fir_same(rows_dev, slit, step, first, n)
        ev[1].record()
        torch.cuda.synchronize()
        t_k.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    col = cs if rows == 1 else cs[:, rows - 1].copy()
    got = (Y if rows == 1 else Y[:, rows - 1]).cpu().numpy()
    assert np.array_equal(got, out[rows - 1].cpu().numpy())
    worst = sampled_check(col, slit, step, first, got)
    flop = 2.0 * n * m * rows
    tk, tc = float(np.median(t_k)), float(np.median(t_call))
    print(f"{label}: {n} points x {m} taps x {rows} row(s): kernel {tk * 1e3:.3f} ms (HIP events, median of {args.reps}; min {min(t_k) * 1e3:.3f}) = "
          f"{flop / tk / 1e12:.2f} TFLOP/s fp64 = {100 * flop / tk / PEAK_F64_VECTOR:.1f} % of the 78.6 TFLOP/s fp64 vector peak "
          f"({100 * flop / tk / PEAK_F32_VECTOR:.1f} % of the 157.3 TFLOP/s vector FMA rate); hapi.convolveSpectrumSame on a device tensor "
          f"{tc * 1e3:.3f} ms per call incl. the host-side slit; sampled check: max err/bound {worst:.4f}", flush=True)
    return slit


slit = run("(a) C3 axis, AF_wing 10", args.points, 1, 10.0)
run("(a) C3 axis, AF_wing 10", args.points, 8, 10.0)
run("(b) golden size, AF_wing 1", 12000, 1, 1.0)
run("(b) golden size, slit longer than the spectrum", 500, 1, 1.0)
# the reference's own sum on one CPU core, same slit, at a size that finishes
nc = args.cpu_points
a = spectrum(nc, 1)
t0 = time.perf_counter()
ref = np.convolve(a, slit, mode="same") * 0.001
dt = time.perf_counter() - t0
print(f"CPU: numpy.convolve(mode='same') of {nc} points x {slit.size} taps: {dt:.2f} s = {2.0 * nc * slit.size / dt / 1e9:.2f} GFLOP/s; "
      f"scaled by points to the {args.points}-point axis: {dt * args.points / nc:.0f} s per spectrum", flush=True)
