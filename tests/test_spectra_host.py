"""CPU: the host side of hapi's spectrum / slit-function / convolution shims (radtxfr_amd/hapi.py) -- the SLIT_* functions
against the reference's own values (tests/golden/g15_spectra.npz, tests/make_golden_spectra.py), the window of the full
convolution that numpy.convolve(..., 'same') returns, the index arithmetic and exception texts of convolveSpectrum*, and
the new C ABI symbols with their refusals. The convolution itself runs on the GPU (tests/test_gpu_spectra.py); here the
one device step (hapi._fir) is replaced by numpy.convolve, which is what the reference runs."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from make_golden_spectra import (EXTRA_SAME, FULL_CASE, N_CONV, RESOLUTION, SLITS, g15_axis, g15_cross_section, g15_thin)
from radtxfr_amd import _lib, engine, hapi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def numpy_fir(monkeypatch):
    """hapi._fir by numpy.convolve: scale * full[first : first + n_out], per column for a batch."""
    def fir(cs, n, taps, scale, first, n_out):
        cs = np.asarray(cs, dtype=np.float64)
        assert cs.shape[0] == n
        one = lambda v: np.convolve(v, taps, "full")[first:first + n_out] * scale  # noqa: E731
        return one(cs) if cs.ndim == 1 else np.stack([one(cs[:, j]) for j in range(cs.shape[1])], axis=1)
    monkeypatch.setattr(hapi, "_fir", fir)


def _close(a, b, rtol):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape
    assert np.all(np.abs(a - b) <= rtol * np.abs(b)), float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def test_slit_functions_vs_golden(golden):
    g = golden("g15_spectra.npz")
    Om = g15_axis()
    step = Om[1] - Om[0]
    x = hapi.arange_(-1.0, 1.0 + step, step)
    assert x.size == 2002  # an even-length slit: the usual case
    for name in SLITS:
        _close(getattr(hapi, "SLIT_" + name)(x, RESOLUTION)[::8], g["fn_" + name.lower()], 1e-14)


def test_slit_function_quirks():
    x = np.array([-0.3, -0.05, 0.0, 0.05, 0.3])
    g = 0.1
    assert hapi.SLIT_DIFFRACTION(x, g)[2] == 1.0 and hapi.SLIT_MICHELSON(x, g)[2] == 1.0  # not the limits 1/g and 2/g
    assert abs(hapi.SLIT_DIFFRACTION(np.array([1e-9]), g)[0] - 1 / g) < 1e-6
    assert abs(hapi.SLIT_MICHELSON(np.array([1e-9]), g)[0] - 2 / g) < 1e-6
    # the cosine slit is not clipped outside one period
    np.testing.assert_allclose(hapi.SLIT_COSINUS(np.array([0.3]), g), (np.cos(np.pi / g * 0.3) + 1) / (2 * g), rtol=1e-15)
    assert hapi.SLIT_COSINUS(np.array([0.2]), g)[0] > 9.9
    # the Gaussian and dispersion slits halve g: g is the full width at half maximum
    for f in (hapi.SLIT_GAUSSIAN, hapi.SLIT_DISPERSION):
        y = f(np.array([0.0, g / 2]), g)
        assert abs(y[1] / y[0] - 0.5) < 1e-12
    assert np.array_equal(hapi.SLIT_RECTANGULAR(x, g), [0.0, 10.0, 10.0, 10.0, 0.0])
    np.testing.assert_allclose(hapi.SLIT_TRIANGULAR(x, g), [0.0, 5.0, 10.0, 5.0, 0.0], rtol=1e-15)
    assert hapi.SLIT_RECTANGULAR(x, g).dtype == np.float64


def test_same_window_is_numpys():
    """engine.same_window(n, m) is where numpy.convolve(a, v, 'same') sits in the full convolution, also for m > n."""
    rng = np.random.default_rng(5)
    for n in range(1, 40):
        for m in range(1, 40):
            a, v = rng.normal(size=n), rng.normal(size=m)
            first, n_out = engine.same_window(n, m)
            assert n_out == max(n, m)
            assert np.array_equal(np.convolve(a, v, "same"), np.convolve(a, v, "full")[first:first + n_out]), (n, m)


def test_convolve_same_vs_golden_with_numpy_fir(golden, numpy_fir):
    """Slit formation (arange_, the slit function, the normalisation) and the window, against the reference's outputs."""
    g = golden("g15_spectra.npz")
    Om, cs = g15_axis(), g15_cross_section()
    cases = json.loads(str(g["cases"]))
    assert {c["tag"] for c in cases} == {s.lower() for s in SLITS} | {t[0] for t in EXTRA_SAME}
    for c in cases:
        n = c["n"]
        O, Y, l, r, slit = hapi.convolveSpectrumSame(Om[:n], cs[:n], Resolution=RESOLUTION, AF_wing=c["AF_wing"],
                                                     SlitFunction=getattr(hapi, "SLIT_" + c["slit"]))
        assert (l, r) == (0, n) and O.shape == (n,) and Y.shape == (n,) and slit.size == c["n_slit"]
        _close(slit[::16], g["slit_" + c["tag"]], 1e-14)
        _close([slit.sum(), np.abs(slit).sum(), slit[0], slit[slit.size // 2], slit[-1]], g["slitsum_" + c["tag"]], 1e-13)
        step = Om[1] - Om[0]
        assert np.array_equal(Y, np.convolve(cs[:n], slit, "same")[:n] * step)
        want = g["same_" + c["tag"]]
        assert np.max(np.abs(Y[g15_thin(n)] - want)) <= 1e-12 * np.max(np.abs(want))
    O, Y, l, r = hapi.convolveSpectrumFull(Om, cs, Resolution=RESOLUTION, AF_wing=FULL_CASE[1],
                                           SlitFunction=getattr(hapi, "SLIT_" + FULL_CASE[0]))
    assert l is None and r is None and O is Om and Y.size == int(g["full_n"][0])
    assert np.max(np.abs(Y[g15_thin(Y.size)] - g["full"])) <= 1e-12 * np.max(np.abs(g["full"]))


def test_convolve_spectrum_index_arithmetic(numpy_fir):
    Om, cs = g15_axis(), g15_cross_section()
    for wing, slitf in ((1.0, hapi.SLIT_GAUSSIAN), (0.7505, hapi.SLIT_TRIANGULAR), (0.25, lambda x, g: np.exp(-np.abs(x) / g))):
        O, Y, l, r, slit = hapi.convolveSpectrum(Om, cs, Resolution=RESOLUTION, AF_wing=wing, SlitFunction=slitf)
        Os, Ys, ls, rs, slits = hapi.convolveSpectrumSame(Om, cs, Resolution=RESOLUTION, AF_wing=wing, SlitFunction=slitf)
        assert isinstance(l, int) and l == len(slit) // 2 and r == N_CONV - len(slit) // 2 and (ls, rs) == (0, N_CONV)
        assert np.array_equal(slit, slits) and np.array_equal(O, Om[l:r]) and np.array_equal(Y, Ys[l:r]) and Os.size == N_CONV
        assert abs(slit.sum() * (Om[1] - Om[0]) - 1.0) < 1e-12
    # Wavenumber= replaces Omega, as in the reference
    O, Y, l, r, slit = hapi.convolveSpectrum(None, cs, AF_wing=0.5, Wavenumber=Om)
    assert np.array_equal(O, Om[l:r])
    # a batch (n, nS) under one slit: column by column
    cs2 = np.stack([cs, 2.0 * cs + 1.0], axis=1)
    O2, Y2, l2, r2, _ = hapi.convolveSpectrum(Om, cs2, AF_wing=0.5)
    assert Y2.shape == (r2 - l2, 2) and np.array_equal(Y2[:, 0], Y)


def test_exception_texts(numpy_fir):
    Om, cs = g15_axis(200), g15_cross_section(200)
    for fn in (hapi.convolveSpectrum, hapi.convolveSpectrumSame):
        for res in (0.001 * 0.5, float(Om[1] - Om[0])):  # step > Resolution and step == Resolution
            with pytest.raises(Exception, match="^step must be less than resolution$"):
                fn(Om, cs, Resolution=res)
    hapi.convolveSpectrumFull(Om, cs, Resolution=0.0005, AF_wing=0.01)  # no such check there (:11886-11900)


def test_new_abi_symbols_and_refusals():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "radtxfr_hip.h")).read()
    for name in ("rtx_hapi_spectrum", "rtx_fir_same", "rtx_fir_tile_points", "rtx_fir_chunk_taps"):
        assert name in _lib.PROTOTYPES and ("int %s(" % name) in header and hasattr(lib, name)
    assert lib.rtx_fir_tile_points() == 2048 and lib.rtx_fir_chunk_taps() == 1024
    # refused before anything touches a device (the pointers are never read): m < 1, n < 1, a window outside the full convolution
    buf = np.zeros(8)
    p = buf.ctypes.data

    def refused(n, m, first, n_out, text):
        assert lib.rtx_fir_same(p, 1, max(n, 1), 1, n, p, m, 1.0, first, n_out, p, max(n_out, 1), None) != 0
        assert text in lib.rtx_last_error().decode(), lib.rtx_last_error()

    refused(8, 0, 0, 8, "m=0")
    refused(0, 3, 0, 2, "n=0")
    refused(8, 3, 0, 11, "outside the 10 points of the full convolution")
    refused(8, 3, 3, 8, "outside the 10 points of the full convolution")
    refused(8, 3, -1, 4, "outside the 10 points of the full convolution")
    assert lib.rtx_fir_same(None, 1, 8, 1, 8, p, 3, 1.0, 0, 8, p, 8, None) != 0
    assert lib.rtx_hapi_spectrum(3, None, None, p, 1, 1, 8, 8, 1.0, 296.0, p, 8, None) != 0
    assert "kind=3" in lib.rtx_last_error().decode()
    assert C.sizeof(C.c_double) == 8


def test_new_names_do_not_import_the_oracle():
    code = ("import sys; from radtxfr_amd import hapi; "
            "names = ['transmittanceSpectrum', 'absorptionSpectrum', 'radianceSpectrum', 'convolveSpectrum', "
            "'convolveSpectrumSame', 'convolveSpectrumFull'] + ['SLIT_' + s for s in %r]; "
            "assert all(callable(getattr(hapi, n)) for n in names); "
            "import numpy as np; hapi.SLIT_MICHELSON(np.linspace(-1, 1, 9), 0.1); "
            "bad = [m for m in sys.modules if m == 'oracle' or m.startswith('oracle.') or m in ('_refimport', 'cpu_ref')]; "
            "assert not bad, bad") % (list(SLITS),)
    subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code], check=True, cwd=ROOT)
