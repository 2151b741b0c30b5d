"""GPU: hapi's spectrum functions and slit-function convolution (radtxfr_amd/hapi.py -> rtx_hapi_spectrum, rtx_fir_same)
against the reference's own outputs (tests/golden/g15_spectra.npz, tests/make_golden_spectra.py) and numpy.convolve.

Bounds:
    spectrum functions : rel_err <= 1e-12, the project's figure for its fp64 elementwise Planck path
    convolution        : pointwise, the a-priori bound of two differently ordered fp64 dot products of M = len(slit) terms,
                             |y_gpu[i] - y_ref[i]| <= 2 gamma_M step sum_k |in[i-k]| |slit[k]|,  gamma_M = M u / (1 - M u), u = 2^-53,
                         the right-hand side from numpy.convolve of the absolute values; no point is left out.
"""
import json

import numpy as np
import pytest

from conftest import rel_err
from make_golden_spectra import (ENVIRONMENTS, FULL_CASE, N_CONV, N_SPEC, RESOLUTION, g15_axis, g15_coefficient,
                                 g15_cross_section, g15_thin)

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


@pytest.fixture(scope="module")
def hapi():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from radtxfr_amd import _lib, hapi
    _lib.load()
    return hapi


@pytest.fixture(scope="module")
def engine(hapi):
    from radtxfr_amd import engine
    return engine


def gamma(M):
    return M * U / (1.0 - M * U)


def assert_within_bound(y, y_ref, a, taps, scale, first, what):
    """Every point of y against y_ref = scale * full(a, taps)[first : first + len(y)] under the dot-product bound."""
    y, y_ref = np.asarray(y), np.asarray(y_ref)
    assert y.shape == y_ref.shape and y.dtype == np.float64, (what, y.shape, y_ref.shape, y.dtype)
    rhs = 2.0 * gamma(len(taps)) * abs(scale) * np.convolve(np.abs(a), np.abs(taps), "full")[first:first + y.size]
    err = np.abs(y - y_ref)
    worst = int(np.argmax(err - rhs))
    print("%s: max |err| %.3e, max err/bound %.3f" % (what, err.max(), float(np.max(err / np.maximum(rhs, 1e-300)))))
    assert np.all(err <= rhs), (what, worst, err[worst], rhs[worst])


def fir(engine, a, taps, scale, first, n_out):
    import torch
    rows = torch.as_tensor(np.atleast_2d(a), device="cuda")
    out = engine.fir_same(rows, taps, scale, first, n_out).cpu().numpy()
    return out[0] if np.ndim(a) == 1 else out


# ------------------------------------------------------------------------------------------- spectrum functions
def test_spectrum_functions_vs_golden(hapi, golden):
    g = golden("g15_spectra.npz")
    X, k = g15_coefficient()
    thin = g15_thin(N_SPEC)
    for e, env in enumerate(ENVIRONMENTS):
        for fn in ("transmittanceSpectrum", "absorptionSpectrum", "radianceSpectrum"):
            Xo, Y = getattr(hapi, fn)(X, k, Environment=dict(env))
            assert Xo is X and Y.shape == (N_SPEC,) and Y.dtype == np.float64
            err = rel_err(Y[thin], g["%s_%d" % (fn, e)])
            print(fn, env, "rel_err %.3e" % err)
            assert err <= 1e-12, (fn, env, err)
    # hapi's constants, not radiative_transfer's c1 / c2: the closed form at one point
    _, R = hapi.radianceSpectrum(X, k, Environment={"l": 100.0, "T": 296.0})
    i = 1234
    want = (1 - np.exp(-k[i] * 100.0)) * (2 * hapi.hh * hapi.cc ** 2 * X[i] ** 3 / (np.exp(hapi.hh * hapi.cc * X[i] / (hapi.cBolts * 296.0)) - 1) * 1.0e-7)
    assert abs(R[i] - want) <= 1e-13 * want
    # the defaults of the reference's signatures, Wavenumber=, and positional order
    assert np.array_equal(hapi.transmittanceSpectrum(X, k)[1], hapi.transmittanceSpectrum(None, k, {"l": 100.}, Wavenumber=X)[1])
    assert np.array_equal(hapi.radianceSpectrum(X, k)[1], R)


def test_spectrum_functions_types_batches_and_file(hapi, tmp_path):
    import torch
    X, k = g15_coefficient()
    env = {"l": 2500.0, "T": 250.0}
    for fn in (hapi.transmittanceSpectrum, hapi.absorptionSpectrum, hapi.radianceSpectrum):
        _, Y = fn(X, k, Environment=env)
        # torch in -> torch out on the device, same bits
        kt = torch.as_tensor(k, device="cuda")
        Xo, Yt = fn(X, kt, Environment=env)
        assert isinstance(Yt, torch.Tensor) and Yt.is_cuda and Yt.dtype == torch.float64 and Xo is X
        assert np.array_equal(Yt.cpu().numpy(), Y)
        _, Ytt = fn(torch.as_tensor(X, device="cuda"), kt, Environment=env)
        assert np.array_equal(Ytt.cpu().numpy(), Y)
        # float32 in == the same values widened on the host
        k32 = k.astype(np.float32)
        _, Y32 = fn(X, torch.as_tensor(k32, device="cuda"), Environment=env)
        assert np.array_equal(Y32.cpu().numpy(), fn(X, k32.astype(np.float64), Environment=env)[1])
        # a batch (n, nS), spectral axis first == column by column
        k2 = np.stack([k, 0.5 * k, 3.0 * k], axis=1)
        _, Y2 = fn(X, k2, Environment=env)
        assert Y2.shape == (N_SPEC, 3) and Y2.dtype == np.float64
        for j in range(3):
            assert np.array_equal(Y2[:, j], fn(X, k2[:, j].copy(), Environment=env)[1])
    # File= in the reference's format (save_to_file, misc/hapi.py:10286-10293)
    p = tmp_path / "t.txt"
    _, Y = hapi.transmittanceSpectrum(X, k, File=str(p))
    lines = p.read_text().splitlines()
    assert len(lines) == N_SPEC and lines[7] == "%e %e" % (X[7], Y[7])


# --------------------------------------------------------------------------------------------------- convolution
def test_convolve_golden_cases(hapi, golden):
    """Every golden case, NumPy in: the stored points of the reference's result and, since the reference's sum IS
    numpy.convolve, every point of it recomputed here -- all under the dot-product bound."""
    g = golden("g15_spectra.npz")
    Om, cs = g15_axis(), g15_cross_section()
    step = Om[1] - Om[0]
    for c in json.loads(str(g["cases"])):
        n = c["n"]
        O, Y, l, r, slit = hapi.convolveSpectrumSame(Om[:n], cs[:n], Resolution=RESOLUTION, AF_wing=c["AF_wing"],
                                                     SlitFunction=getattr(hapi, "SLIT_" + c["slit"]))
        assert (l, r) == (0, n) and np.array_equal(O, Om[:n]) and slit.size == c["n_slit"] and isinstance(Y, np.ndarray)
        assert np.all(np.abs(slit[::16] - g["slit_" + c["tag"]]) <= 1e-14 * np.abs(g["slit_" + c["tag"]]))
        first = (min(n, slit.size) - 1) // 2
        assert_within_bound(Y, np.convolve(cs[:n], slit, "same")[:n] * step, cs[:n], slit, step, first, c["tag"] + " (all points)")
        thin = g15_thin(n)
        rhs = 2.0 * gamma(slit.size) * step * np.convolve(np.abs(cs[:n]), np.abs(slit), "full")[first:first + n]
        err = np.abs(Y[thin] - g["same_" + c["tag"]])
        print(c["tag"], "golden points: max err/bound %.3f" % float(np.max(err / rhs[thin])))
        assert np.all(err <= rhs[thin]), (c["tag"], float(np.max(err / rhs[thin])))
    O, Y, l, r = hapi.convolveSpectrumFull(Om, cs, Resolution=RESOLUTION, AF_wing=FULL_CASE[1],
                                           SlitFunction=getattr(hapi, "SLIT_" + FULL_CASE[0]))
    assert l is None and r is None and O is Om and Y.size == int(g["full_n"][0])
    slit = getattr(hapi, "SLIT_" + FULL_CASE[0])(np.arange(-FULL_CASE[1], FULL_CASE[1] + step, step), RESOLUTION)
    assert Y.size == N_CONV + slit.size - 1
    assert_within_bound(Y, np.convolve(cs, slit, "full") * step, cs, slit, step, 0, "full (all points)")
    thin = g15_thin(Y.size)
    rhs = 2.0 * gamma(slit.size) * step * np.convolve(np.abs(cs), np.abs(slit), "full")
    assert np.all(np.abs(Y[thin] - g["full"]) <= rhs[thin])


def test_convolve_spectrum_cut_equals_same(hapi):
    Om, cs = g15_axis(), g15_cross_section()
    for wing, slitf in ((1.0, hapi.SLIT_MICHELSON), (0.7505, hapi.SLIT_GAUSSIAN), (0.2, lambda x, g: np.exp(-np.abs(x) / g))):
        O, Y, l, r, slit = hapi.convolveSpectrum(Om, cs, Resolution=RESOLUTION, AF_wing=wing, SlitFunction=slitf)
        _, Ys, _, _, slits = hapi.convolveSpectrumSame(Om, cs, Resolution=RESOLUTION, AF_wing=wing, SlitFunction=slitf)
        assert l == len(slit) // 2 and r == N_CONV - len(slit) // 2 and np.array_equal(O, Om[l:r])
        assert np.array_equal(slit, slits) and np.array_equal(Y, Ys[l:r])


def test_convolve_types_batches_and_repeats(hapi):
    import torch
    Om, cs = g15_axis(), g15_cross_section()
    kw = dict(Resolution=RESOLUTION, AF_wing=1.0, SlitFunction=hapi.SLIT_DIFFRACTION)
    _, Y, _, _, slit = hapi.convolveSpectrumSame(Om, cs, **kw)
    # two repeated calls are bit-identical
    assert np.array_equal(hapi.convolveSpectrumSame(Om, cs, **kw)[1], Y)
    # torch in -> torch out on the device (float64 and float32), no host copy of the spectrum
    ct = torch.as_tensor(cs, device="cuda")
    Ot, Yt, l, r, st = hapi.convolveSpectrumSame(Om, ct, **kw)
    assert isinstance(Yt, torch.Tensor) and Yt.is_cuda and Yt.dtype == torch.float64 and Yt.shape == (N_CONV,)
    assert np.array_equal(Yt.cpu().numpy(), Y) and np.array_equal(st, slit)
    Oc, Yc, lc, rc, _ = hapi.convolveSpectrum(torch.as_tensor(Om, device="cuda"), ct, **kw)
    assert Yc.is_cuda and Oc.is_cuda and np.array_equal(Yc.cpu().numpy(), Y[lc:rc]) and np.array_equal(Oc.cpu().numpy(), Om[lc:rc])
    Yf = hapi.convolveSpectrumFull(Om, ct, **kw)[1]
    assert Yf.is_cuda and np.array_equal(Yf.cpu().numpy(), hapi.convolveSpectrumFull(Om, cs, **kw)[1])
    # float32 in == the same values widened to float64 on the host, bit for bit
    c32 = cs.astype(np.float32)
    Y32 = hapi.convolveSpectrumSame(Om, torch.as_tensor(c32, device="cuda"), **kw)[1]
    assert Y32.dtype == torch.float64
    assert np.array_equal(Y32.cpu().numpy(), hapi.convolveSpectrumSame(Om, c32.astype(np.float64), **kw)[1])
    # a batch (n, nS) under one slit == row by row, bit for bit (NumPy and torch, float64 and float32)
    rng = np.random.default_rng(7)
    cs2 = np.stack([cs, rng.uniform(0.0, 1.0, N_CONV), 2.0 * cs + 1.0, cs[::-1], -cs], axis=1)
    Y2 = hapi.convolveSpectrumSame(Om, cs2, **kw)[1]
    assert Y2.shape == (N_CONV, 5) and Y2.dtype == np.float64
    for j in range(5):
        assert np.array_equal(Y2[:, j], hapi.convolveSpectrumSame(Om, cs2[:, j].copy(), **kw)[1]), j
    assert np.array_equal(Y2[:, 0], Y)
    Y2t = hapi.convolveSpectrumSame(Om, torch.as_tensor(cs2, device="cuda"), **kw)[1]
    assert Y2t.is_cuda and Y2t.shape == (N_CONV, 5) and np.array_equal(Y2t.cpu().numpy(), Y2)
    Y2f = hapi.convolveSpectrumSame(Om, torch.as_tensor(cs2.astype(np.float32), device="cuda"), **kw)[1]
    assert np.array_equal(Y2f.cpu().numpy(), hapi.convolveSpectrumSame(Om, cs2.astype(np.float32).astype(np.float64), **kw)[1])
    O3, Y3, l3, r3, _ = hapi.convolveSpectrum(Om, cs2, **kw)
    assert Y3.shape == (r3 - l3, 5) and np.array_equal(Y3, Y2[l3:r3])


def test_fir_tile_and_chunk_edges(engine):
    """Lengths tile-1, tile, tile+1 and tap counts 1, 2, the 8-tap group's edges, and longer than one staged chunk: the
    full convolution against numpy.convolve under the bound, and any window of it equal to that slice bit for bit."""
    from radtxfr_amd import _lib
    lib = _lib.load()
    tile, chunk = lib.rtx_fir_tile_points(), lib.rtx_fir_chunk_taps()
    rng = np.random.default_rng(11)
    for n in (1, 5, tile - 1, tile, tile + 1, 2 * tile + 3):
        for m in (1, 2, 7, 8, 9, chunk - 1, chunk, chunk + 1, 2 * chunk + 5):
            a, taps = rng.normal(size=n), rng.normal(size=m)
            full = fir(engine, a, taps, 0.37, 0, n + m - 1)
            assert_within_bound(full, np.convolve(a, taps, "full") * 0.37, a, taps, 0.37, 0, "n=%d m=%d" % (n, m))
            first, n_out = engine.same_window(n, m)
            assert np.array_equal(fir(engine, a, taps, 0.37, first, n_out), full[first:first + n_out]), (n, m)
            if n + m - 1 > 3:
                assert np.array_equal(fir(engine, a, taps, 0.37, n + m - 4, 3), full[n + m - 4:n + m - 1]), (n, m)
    # one tap: a plain scaling, exactly
    a = rng.normal(size=tile + 1)
    assert np.array_equal(fir(engine, a, np.array([1.5]), 2.0, 0, a.size), a * 1.5 * 2.0)
    # the result of a row does not depend on how many rows the call has
    A = rng.normal(size=(7, tile + 9))
    taps = rng.normal(size=chunk + 3)
    out = fir(engine, A, taps, 1.0, 100, tile + 500)
    for j in range(7):
        assert np.array_equal(out[j], fir(engine, A[j], taps, 1.0, 100, tile + 500)), j


def test_fir_at_scale_sampled(engine):
    """2^20 points x 20 001 taps (the default AF_wing = 10 at 0.001 cm^-1): 64 sampled outputs of the 'same' window, each
    checked as a plain dot product on the host under the same bound."""
    import torch
    n, m = 1 << 20, 20001
    rng = np.random.default_rng(13)
    a = rng.uniform(0.0, 1.0, n) * np.exp(rng.normal(size=n))
    x = (np.arange(m) - m // 2) * 0.001
    taps = np.exp(-np.log(2) * (x / 0.05) ** 2) * (1.0 + 0.1 * rng.normal(size=m))
    step = 0.001
    first, n_out = engine.same_window(n, m)
    d = torch.as_tensor(a[None], device="cuda")
    y = engine.fir_same(d, taps, step, first, n)
    y2 = engine.fir_same(d, taps, step, first, n)
    assert torch.equal(y, y2)
    y = y[0].cpu().numpy()
    idx = np.unique(np.concatenate([[0, 1, m // 2, n - 1, n - 2, n - m // 2], rng.integers(0, n, 58)]))
    worst = 0.0
    for i in idx:
        q = i + first                       # index in the full convolution: sum_k taps[k] a[q - k]
        k = np.arange(max(0, q - n + 1), min(m, q + 1))
        ref = np.dot(taps[k], a[q - k]) * step
        rhs = 2.0 * gamma(m) * step * np.dot(np.abs(taps[k]), np.abs(a[q - k]))
        worst = max(worst, abs(y[i] - ref) / rhs)
        assert abs(y[i] - ref) <= rhs, (int(i), y[i], ref, rhs)
    print("scale: %d sampled outputs, max err/bound %.4f" % (idx.size, worst))
