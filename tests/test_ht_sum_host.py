"""CPU: the host side of the Hartmann-Tran line-sum (csrc/rtx_ht.hip) -- the new C ABI entry points with
their refusals before any device work, the switch hapi.VARIABLES["HT_COLUMNS"] and its default, hapi._tref_ht, the 27-slot
column naming, and the fixture tests/golden/g17_ht_sum.npz (tests/make_golden_ht_sum.py). The values are checked on the GPU
(tests/test_gpu_ht_sum.py)."""
import ctypes as C
import json
import os

import numpy as np

from make_golden_ht_sum import ALL_COMPONENTS, HEAD, N_LINES, SPECIES, VOIGT_STYLE, g17_axis, g17_table, ht_column_names
from radtxfr_amd import _lib, engine, hapi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rtx_lines_set_ht", "rtx_ht_create", "rtx_ht_free", "rtx_ht_prep", "rtx_ht_sum", "rtx_ht_params")


def test_new_names_in_header_and_prototypes():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "radtxfr_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.PROTOTYPES and ("int %s(" % name) in header and hasattr(lib, name)
    assert "#define RTX_HT_COLS 27" in header
    assert "rtx_ht.hip" in open(os.path.join(ROOT, "radtxfr_amd", "csrc", "Makefile")).read()


def test_entry_points_refuse_bad_arguments_with_text():
    """Refused before anything touches a device: this runs without a GPU, and the pointers are host memory. (The refusals
    that need a table on the device -- a column set that does not exist, ld < n -- are in tests/test_gpu_ht_sum.py.)"""
    lib = _lib.load()
    buf = np.zeros(64)
    p = buf.ctypes.data

    def refused(rc, text):
        assert rc != 0
        assert text in lib.rtx_last_error().decode(), lib.rtx_last_error()

    refused(lib.rtx_lines_set_ht(None, 1, p, p), "NULL")
    h = C.c_void_p(0)
    refused(lib.rtx_ht_create(10, 2, 100, None), "NULL")
    refused(lib.rtx_ht_create(-1, 2, 100, C.byref(h)), "n_lines=-1")
    refused(lib.rtx_ht_create(10, 0, 100, C.byref(h)), "max_states=0")
    refused(lib.rtx_ht_create(10, 2, 0, C.byref(h)), "max_points=0")
    assert lib.rtx_ht_create(10, 2, 100, C.byref(h)) == 0 and h.value  # no device memory yet
    try:
        # rtx_ht_prep(ht, lines, X_h, nx, n_states, T_h, p_h, q_h, w_h, mass_h, n_dil, dil_h, frac_h, wing, wing_hw, thr, scale, stream)
        tail = (0.0, 50.0, 0.0, 1.0, None)
        refused(lib.rtx_ht_prep(None, p, p, 4, 1, p, p, p, p, p, 1, p, p, *tail), "NULL")
        refused(lib.rtx_ht_prep(h, p, p, -4, 1, p, p, p, p, p, 1, p, p, *tail), "nx=-4")
        refused(lib.rtx_ht_prep(h, p, p, 101, 1, p, p, p, p, p, 1, p, p, *tail), "nx=101")
        refused(lib.rtx_ht_prep(h, p, p, 4, 3, p, p, p, p, p, 1, p, p, *tail), "n_states=3")
        refused(lib.rtx_ht_prep(h, p, p, 4, 0, p, p, p, p, p, 1, p, p, *tail), "n_states=0")
        refused(lib.rtx_ht_prep(h, p, p, 4, 1, p, p, p, p, p, -1, p, p, *tail), "n_dil=-1")
        refused(lib.rtx_ht_prep(h, p, p, 4, 1, p, p, p, p, p, 9, p, p, *tail), "n_dil=9")
        for args in ((h, None, p, 4, 1, p, p, p, p, p, 1, p, p), (h, p, None, 4, 1, p, p, p, p, p, 1, p, p),
                     (h, p, p, 4, 1, None, p, p, p, p, 1, p, p), (h, p, p, 4, 1, p, None, p, p, p, 1, p, p),
                     (h, p, p, 4, 1, p, p, None, p, p, 1, p, p), (h, p, p, 4, 1, p, p, p, None, p, 1, p, p),
                     (h, p, p, 4, 1, p, p, p, p, None, 1, p, p), (h, p, p, 4, 1, p, p, p, p, p, 1, None, p),
                     (h, p, p, 4, 1, p, p, p, p, p, 1, p, None)):
            refused(lib.rtx_ht_prep(*args, *tail), "NULL")
        # rtx_ht_sum(ht, n_states, out_f32, out_f64, ld, stream); rtx_ht_params(ht, state, params, strength, window, stream)
        refused(lib.rtx_ht_sum(None, 1, None, p, 4, None), "NULL")
        refused(lib.rtx_ht_sum(h, 1, None, None, 4, None), "NULL")
        refused(lib.rtx_ht_sum(h, 1, None, p, 4, None), "rtx_ht_prep has not been run")
        refused(lib.rtx_ht_params(None, 0, p, p, p, None), "NULL")
        refused(lib.rtx_ht_params(h, 0, p, p, p, None), "rtx_ht_prep has not been run")
    finally:
        assert lib.rtx_ht_free(h) == 0
    assert lib.rtx_ht_free(None) == 0
    assert np.all(buf == 0.0)


def test_switch_is_off_by_default_and_tref_ht_edges():
    assert not hapi.VARIABLES["HT_COLUMNS"]
    got = [hapi._tref_ht(T) for T in (99.999, 100, 199.999, 200, 399.999, 400)]
    assert got == [50.0, 150.0, 150.0, 296.0, 296.0, 700.0]
    assert hapi._tref_ht(0.0) == 50.0 and hapi._tref_ht(3000.0) == 700.0


def test_column_naming_27_slots_mixed_case():
    names = engine.ht_column_names("He2O")
    assert len(names) == 27 == len(set(names)) and names == ht_column_names("he2o")
    assert names[:6] == ["gamma_HT_0_he2o_50", "n_HT_he2o_50", "gamma_HT_2_he2o_50", "delta_HT_0_he2o_50", "deltap_HT_he2o_50",
                         "delta_HT_2_he2o_50"]
    assert names[6] == "gamma_HT_0_he2o_150" and names[12] == "gamma_HT_0_he2o_296" and names[23] == "delta_HT_2_he2o_700"
    assert names[24:] == ["nu_HT_he2o", "kappa_HT_he2o", "eta_HT_he2o"]
    assert all(n.startswith(engine.HT_PREFIXES) for n in names)
    # what a call reads: the six of its bucket and the three without a temperature, per key, duplicates once
    read = hapi._ht_columns_read(["h2", "air", "h2"], 150.0)
    assert read == engine.ht_column_names("h2")[6:12] + engine.ht_column_names("h2")[24:] + engine.ht_column_names("air")[6:12] + \
        engine.ht_column_names("air")[24:]


def test_golden_loads_cases_parse_and_zeros_are_where_stated(golden):
    g = golden("g17_ht_sum.npz")
    cases = json.loads(str(g["cases"]))
    tags = [c["tag"] for c in cases]
    assert len(set(tags)) == len(tags) >= 6
    assert sorted({c["T"] for c in cases}) == [90.0, 150.0, 250.0, 280.0, 296.0, 500.0]
    assert any(k != k.lower() for c in cases for k in c["Diluent"]) and any(len(c["Diluent"]) == 3 for c in cases)
    assert any(c.get("HITRAN_units") is False for c in cases) and any("Components" in c and len(c["Components"][0]) == 3 for c in cases)
    assert any("OmegaWing" in c and "OmegaWingHW" in c and "IntensityThreshold" in c for c in cases)
    tbl = g17_table(g)
    assert tbl["nu"].size == N_LINES and np.all(np.diff(tbl["nu"]) >= 0)
    a, b, lo, hi = HEAD
    assert np.all((tbl["nu"][a:b] >= lo) & (tbl["nu"][a:b] <= hi)) and b - a == 140
    for sp in SPECIES:
        for c in ht_column_names(sp):
            assert tbl[c].shape == (N_LINES,) and np.any(tbl[c] == 0.0) and np.any(tbl[c] != 0.0), c
    for k in VOIGT_STYLE:
        assert tbl[k].shape == (N_LINES,)
    # every ninth row has no speed dependence at all
    for k in tbl:
        if k.startswith(("gamma_HT_2_", "delta_HT_2_", "SD_")):
            assert np.all(tbl[k][::9] == 0.0), k
    for c in cases:
        X, xs, par = g17_axis(c), g["xs_" + c["tag"]], g["par_" + c["tag"]]
        assert X.shape == xs.shape and np.all(np.diff(X) >= 0) and np.all(np.isfinite(xs)) and np.all(xs >= 0.0)
        assert int(np.sum(xs == 0.0)) == c["n_zero"]
        assert par.shape == (c["n_evaluated"], 11) and c["n_evaluated"] <= N_LINES
        if c["T"] in (90.0, 150.0):
            assert c["n_zero"] > 500  # points outside every window
        if "grid" in c:
            assert np.any(np.diff(X) == 0.0) and np.ptp(np.diff(X)) > 1e-3  # repeated points, non-uniform
    assert len(ALL_COMPONENTS) == 4
