"""CPU: the host side of hapi's line-profile functions (radtxfr_amd/hapi.py: pcqsdhc, PROFILE_*, hum1_wei, cpf3,
profile_lines) -- the fixture tests/golden/g16_profiles.npz (tests/make_golden_profiles.py) and the error of the reference
itself that the GPU bounds are taken from, the three C ABI entry points with their refusals and their empty-input no-ops,
the reference's signatures, and the exceptions raised before any device work. The values are checked on the GPU
(tests/test_gpu_profiles.py)."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest

from make_golden_profiles import NOT_ORDINARY, effective_params
from radtxfr_amd import _lib, hapi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rtx_profile_eval", "rtx_profile_sum", "rtx_cpf_eval")


def trapezoid(y, x):
    return float(np.sum(0.5 * np.diff(x) * (y[1:] + y[:-1])))


def test_golden_loads_and_reference_error_of_ordinary_cases(golden):
    g = golden("g16_profiles.npz")
    cases = json.loads(str(g["cases"]))
    tags = [c["tag"] for c in cases]
    assert len(tags) == len(set(tags)) and len([t for t in tags if t.startswith("rand")]) == 20
    for t in ("ht_1atm", "ht_cplx", "ht_midp", "cpf3_shell", "rautian", "part1_eta", "p1_4000", "neg_re", "p2_all", "p2p4_switch",
              "small_g2_1e-10", "small_g2_1e-08", "small_g2_1e-06", "p3_near", "p3_far", "lim_sdrautian", "lim_rautian", "lim_sdvoigt",
              "lim_voigt", "lim_lorentz", "lim_doppler", "ht_1atm_wide"):
        assert t in tags, t
    for c in cases:
        tag = c["tag"]
        sg, truth = g["sg_" + tag], g["truth_" + tag]
        assert sg.shape == truth.shape and np.all(np.isfinite(sg)) and np.all(np.isfinite(truth)) and np.all(np.abs(truth) > 0)
        assert c["ordinary"] == (tag not in NOT_ORDINARY)
        assert c["has_ref"] == (tag != "p3_far")  # the reference raises in PART3's far form
        if not c["has_ref"]:
            continue
        ref, e = g["ref_" + tag], float(g["eref_" + tag])
        assert ref.shape == sg.shape and np.all(np.isfinite(ref))
        # e_ref was formed against the long-double truth; the stored truth is that rounded to fp64 (<= 2^-53 relative)
        assert abs(e - float(np.max(np.abs(ref - truth) / np.abs(truth)))) <= 2.3e-16
        if c["ordinary"]:
            assert e <= 1e-12, (tag, e)  # the reference agrees with an extended-precision evaluation of its own formulas
    assert float(g["eref_cpf"]) <= 1e-12 and float(g["eref_cpf3"]) <= 1e-12
    assert np.any(g["cpf_y"] < 0) and np.any(np.abs(g["cpf_x"]) + g["cpf_y"] >= 15) and np.any(np.abs(g["cpf_x"]) + g["cpf_y"] < 15)
    # the regimes the cases are there for, by the reference's own tests on the parameters (misc/hapi.py:9910, :9930-9932)
    def parts(tag):
        c = next(c for c in cases if c["tag"] == tag)
        sg0, GamD, Gam0, Gam2, Shift0, Shift2, anuVC, eta = effective_params(c)
        cte = np.sqrt(np.log(2.0)) / GamD
        c0t = (1 - eta) * (complex(Gam0, Shift0) - 1.5 * complex(Gam2, Shift2)) + anuVC
        c2t = (1 - eta) * complex(Gam2, Shift2)
        if abs(c2t) == 0:
            return {"part1_far": int(np.sum(np.abs((1j * (sg0 - g["sg_" + tag]) + c0t) * cte) > 4.0e3)), "n": g["sg_" + tag].size}
        X = (1j * (sg0 - g["sg_" + tag]) + c0t) / c2t
        Y = abs(1.0 / (2.0 * cte * c2t) ** 2)
        p2 = np.abs(X) <= 3.0e-8 * Y
        p3 = (Y <= 1.0e-15 * np.abs(X)) & ~p2
        return {"p2": int(p2.sum()), "p3": int(p3.sum()), "p3_far": int(np.sum(p3 & (np.abs(np.sqrt(X)) > 4.0e3))), "n": X.size}
    assert parts("p1_4000")["part1_far"] == 208
    assert parts("p2_all")["p2"] == 401
    assert parts("p2p4_switch")["p2"] == 259
    assert parts("p3_near")["p3"] == 155 and parts("p3_near")["p3_far"] == 0
    assert parts("p3_far")["p3_far"] == parts("p3_far")["n"]
    assert parts("ht_1atm") == {"p2": 0, "p3": 0, "p3_far": 0, "n": 401}
    # physics: the real part integrates to 1 less the two Lorentzian tails beyond +-100 cm^-1 (the reference's value by the
    # trapezoid rule is 0.99966 ... 0.99969, depending on the grid)
    I = trapezoid(g["ref_ht_1atm_wide"].real, g["sg_ht_1atm_wide"])
    assert abs(I - 0.99966) < 5e-5, I


def test_new_names_in_header_and_prototypes():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "radtxfr_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.PROTOTYPES and ("int %s(" % name) in header and hasattr(lib, name)
    for macro in ("RTX_LS_PCQSDHC 0", "RTX_LS_LORENTZ 1", "RTX_LS_DOPPLER 2", "RTX_CPF_HUM1_WEI 0", "RTX_CPF_CPF3 1"):
        assert "#define " + macro in header


def test_entry_points_refuse_bad_arguments_with_text():
    """Refused before anything touches a device: the pointers are host memory that a kernel could not read."""
    lib = _lib.load()
    buf = np.zeros(64)
    p = buf.ctypes.data

    def refused(rc, text):
        assert rc != 0
        assert text in lib.rtx_last_error().decode(), lib.rtx_last_error()

    # rtx_profile_eval(kind, n_lines, params, sg, n, out_re, out_im, ld, stream)
    for args in ((0, 1, None, p, 4, p, p, 4, None), (0, 1, p, None, 4, p, p, 4, None), (0, 1, p, p, 4, None, p, 4, None)):
        refused(lib.rtx_profile_eval(*args), "NULL")
    refused(lib.rtx_profile_eval(0, -1, p, p, 4, p, p, 4, None), "n_lines=-1")
    refused(lib.rtx_profile_eval(0, 1, p, p, -4, p, p, 4, None), "n=-4")
    refused(lib.rtx_profile_eval(0, 1, p, p, 4, p, p, 3, None), "ld=3")
    refused(lib.rtx_profile_eval(3, 1, p, p, 4, p, p, 4, None), "kind=3")
    refused(lib.rtx_profile_eval(-1, 1, p, p, 4, p, None, 4, None), "kind=-1")
    # rtx_profile_sum(n_lines, params, w_re, w_im, sg, n, out, stream)
    for args in ((1, None, p, p, p, 4, p, None), (1, p, None, p, p, 4, p, None), (1, p, p, p, None, 4, p, None), (1, p, p, None, p, 4, None, None)):
        refused(lib.rtx_profile_sum(*args), "NULL")
    refused(lib.rtx_profile_sum(-2, p, p, None, p, 4, p, None), "n_lines=-2")
    refused(lib.rtx_profile_sum(2, p, p, None, p, -1, p, None), "n=-1")
    # rtx_cpf_eval(kind, x, y, n, out_re, out_im, stream)
    for args in ((0, None, p, 4, p, p, None), (0, p, None, 4, p, p, None), (1, p, p, 4, None, p, None)):
        refused(lib.rtx_cpf_eval(*args), "NULL")
    refused(lib.rtx_cpf_eval(2, p, p, 4, p, p, None), "kind=2")
    refused(lib.rtx_cpf_eval(0, p, p, -4, p, None, None), "n=-4")


def test_entry_points_accept_empty_input_without_a_launch():
    """n = 0 or n_lines = 0: success, nothing launched (this runs without a GPU) and nothing written."""
    lib = _lib.load()
    buf = np.full(64, 7.0)
    p = buf.ctypes.data
    for kind in (0, 1, 2):
        assert lib.rtx_profile_eval(kind, 0, p, p, 4, p, p, 4, None) == 0
        assert lib.rtx_profile_eval(kind, 3, p, p, 0, p, None, 0, None) == 0
    assert lib.rtx_profile_sum(0, p, p, p, p, 4, p, None) == 0
    assert lib.rtx_profile_sum(3, p, p, None, p, 0, p, None) == 0
    assert lib.rtx_cpf_eval(0, p, p, 0, p, p, None) == 0
    assert lib.rtx_cpf_eval(1, p, p, 0, p, None, None) == 0
    assert np.all(buf == 7.0)
    assert C.sizeof(C.c_double) == 8


def test_signatures_are_the_references():
    want = {
        "pcqsdhc": "sg0 GamD Gam0 Gam2 Shift0 Shift2 anuVC eta sg",
        "PROFILE_HT": "sg0 GamD Gam0 Gam2 Shift0 Shift2 anuVC eta sg",
        "PROFILE_HTP": "sg0 GamD Gam0 Gam2 Shift0 Shift2 anuVC eta sg",
        "PROFILE_SDRAUTIAN": "sg0 GamD Gam0 Gam2 Shift0 Shift2 anuVC sg",
        "PROFILE_RAUTIAN": "sg0 GamD Gam0 Shift0 anuVC eta sg",
        "PROFILE_SDVOIGT": "sg0 GamD Gam0 Gam2 Shift0 Shift2 sg",
        "PROFILE_VOIGT": "sg0 GamD Gam0 sg",
        "PROFILE_LORENTZ": "sg0 Gam0 sg",
        "PROFILE_DOPPLER": "sg0 GamD sg",
        "hum1_wei": "x y n",
        "cpf3": "X Y",
        "profile_lines": "sg sg0 GamD Gam0 Gam2 Shift0 Shift2 anuVC eta profile weights mixing",
    }
    for name, names in want.items():
        assert list(inspect.signature(getattr(hapi, name)).parameters) == names.split(), name
    assert hapi.PROFILE_HTP is hapi.PROFILE_HT
    assert inspect.signature(hapi.hum1_wei).parameters["n"].default == 24
    d = {k: v.default for k, v in inspect.signature(hapi.profile_lines).parameters.items()}
    assert d["GamD"] is None and d["profile"] == "HT" and d["weights"] is None and d["mixing"] is None
    assert all(d[k] == 0.0 for k in ("Gam0", "Gam2", "Shift0", "Shift2", "anuVC", "eta"))


def test_value_errors_come_before_any_device_work():
    sg2 = np.zeros((2, 3)) + 1000.0
    a = (1000.0, 0.0012, 0.05, 0.006, -0.002, 0.0005, 0.01, 0.2)
    for call in (lambda: hapi.pcqsdhc(*a, sg2), lambda: hapi.PROFILE_HT(*a, sg2), lambda: hapi.PROFILE_SDRAUTIAN(*a[:7], sg2),
                 lambda: hapi.PROFILE_RAUTIAN(1000.0, 0.0012, 0.05, -0.002, 0.01, 0.2, sg2),
                 lambda: hapi.PROFILE_SDVOIGT(*a[:6], sg2), lambda: hapi.PROFILE_VOIGT(1000.0, 0.0012, 0.05, sg2),
                 lambda: hapi.PROFILE_LORENTZ(1000.0, 0.05, sg2), lambda: hapi.PROFILE_DOPPLER(1000.0, 0.0012, sg2),
                 lambda: hapi.profile_lines(sg2, [1000.0, 1001.0], 0.0012, 0.05),
                 lambda: hapi.pcqsdhc(*a, [[1000.0], [1001.0]])):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match="n=12"):
        hapi.hum1_wei(np.array([0.5]), np.array([0.5]), n=12)
    with pytest.raises(ValueError):
        hapi.profile_lines([1000.0], [1000.0, 1001.0], 0.0012, 0.05, profile="GALATRY")
    with pytest.raises(ValueError):
        hapi.profile_lines([1000.0], [1000.0, 1001.0], None, 0.05)  # HT needs GamD
    with pytest.raises(ValueError):
        hapi.profile_lines([1000.0], [1000.0, 1001.0], [0.001, 0.002, 0.003], 0.05)  # lengths that do not match
    with pytest.raises(ValueError):
        hapi.profile_lines([1000.0], [1000.0, 1001.0], 0.0012, 0.05, mixing=[0.1, 0.2])  # mixing without weights


def test_profile_functions_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    sg = np.linspace(999.0, 1001.0, 5)
    for call in (lambda: hapi.pcqsdhc(1000.0, 0.0012, 0.05, 0.006, -0.002, 0.0005, 0.01, 0.2, sg),
                 lambda: hapi.PROFILE_VOIGT(1000.0, 0.0012, 0.05, sg), lambda: hapi.PROFILE_LORENTZ(1000.0, 0.05, 1000.0),
                 lambda: hapi.PROFILE_DOPPLER(1000.0, 0.0012, sg), lambda: hapi.hum1_wei(np.array([0.5]), np.array([0.5])),
                 lambda: hapi.cpf3(np.array([6.0]), np.array([6.0])),
                 lambda: hapi.profile_lines(sg, [1000.0, 1000.5], 0.0012, 0.05, weights=[1.0, 2.0])):
        with pytest.raises(_lib.RtxError):
            call()


def test_device_arithmetic_on_the_host_vs_golden(golden, tmp_path):
    """csrc/rtx_pcqsdhc.h compiled for the host (tests/pcqsdhc_host_main.cpp): every golden case, hum1_wei and cpf3 under the
    bounds of tests/test_gpu_profiles.py -- 16 * max(e_ref of the case, E_ord) on complex moduli point by point and on the
    real part against max |ref|; p3_far against `truth` under p3_near's bound. The GPU's v_rcp_f64 / v_rsq_f64 seeds are the
    one thing this cannot run; everything else, every PART and both forms of each, is the code the kernels run."""
    import subprocess
    from test_devmem_host import _host_cxx
    csrc = os.path.join(ROOT, "radtxfr_amd", "csrc")
    exe = str(tmp_path / "pcqsdhc_host")
    build = subprocess.run([_host_cxx(), "-std=c++17", "-O2", "-ffp-contract=off", "-I", csrc,
                            os.path.join(ROOT, "tests", "pcqsdhc_host_main.cpp"), "-o", exe, "-lm"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    g = golden("g16_profiles.npz")
    cases = [c for c in json.loads(str(g["cases"])) if c["fn"] not in ("PROFILE_LORENTZ", "PROFILE_DOPPLER")]
    E_ord = max(float(g["eref_" + c["tag"]]) for c in json.loads(str(g["cases"])) if c["ordinary"])
    recs = []
    for c in cases:
        a = effective_params(c)
        eta = complex(a[7])
        sg = g["sg_" + c["tag"]]
        recs.append(" ".join(["0"] + [repr(float(v)) for v in a[:7]] + [repr(eta.real), repr(eta.imag), "0", str(sg.size)] + [repr(float(s)) for s in sg]))
    for mode, name in ((1, "cpf"), (2, "cpf3")):
        recs.append(" ".join([str(mode), str(g[name + "_x"].size)] + ["%r %r" % (float(a), float(b)) for a, b in zip(g[name + "_x"], g[name + "_y"])]))
    run = subprocess.run([exe], input="\n".join(recs) + "\n", capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    vals = np.array([[float(t) for t in l.split()] for l in run.stdout.splitlines()])
    vals = vals[:, 0] + 1j * vals[:, 1]
    k, bad = 0, []
    for c in cases:
        tag = c["tag"]
        ref = g["ref_" + tag] if c["has_ref"] else g["truth_" + tag]
        bound = 16.0 * max(float(g["eref_" + (tag if c["has_ref"] else "p3_near")]), E_ord)
        v = vals[k:k + ref.size]
        k += ref.size
        err = float(np.max(np.abs(v - ref) / np.abs(ref)))
        err_re = float(np.max(np.abs(v.real - ref.real)) / np.max(np.abs(ref)))
        if not (err <= bound and err_re <= bound):
            bad.append((tag, err, err_re, bound))
    assert not bad, bad
    for name in ("cpf", "cpf3"):
        ref = g[name + "_ref"]
        v = vals[k:k + ref.size]
        k += ref.size
        assert float(np.max(np.abs(v - ref) / np.abs(ref))) <= 16.0 * max(float(g["eref_" + name]), E_ord), name
    assert k == vals.size
