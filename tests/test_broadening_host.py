"""CPU: line broadening by any diluent and per-layer self-broadening, host side.

  * the oracle's arbitrary-Diluent path (oracle/cpu_ref.line_params) against the reference's own absorptionCoefficient_*
    on every case of tests/golden/g14_diluents.npz (tests/make_golden_diluents.py);
  * the diluent mixes broadening="self" / ("self", "h2o") hand to the prologue (engine.broadening_fractions);
  * the option checks that refuse broadening= where it is not implemented (before any device work).
"""
import json

import numpy as np
import pytest

from make_golden_diluents import g14_axis, g14_table
from oracle import cpu_ref as ref
from radtxfr_amd import engine
from radtxfr_amd import radiative_transfer as rt

ORACLE = {"Voigt": ref.absorptionCoefficient_Voigt, "Lorentz": ref.absorptionCoefficient_Lorentz,
          "SDVoigt": ref.absorptionCoefficient_SDVoigt, "HT": ref.absorptionCoefficient_SDVoigt}  # HT without HT columns = SDVoigt


def g14_cases(g):
    return json.loads(str(g["cases"]))


def test_g14_oracle_reproduces_reference(golden):
    g = golden("g14_diluents.npz")
    tbl = g14_table(g)
    cases = g14_cases(g)
    assert len(cases) >= 8
    for c in cases:
        kw = {"HITRAN_units": c["HITRAN_units"]} if "HITRAN_units" in c else {}
        _, xs = ORACLE[c["fn"]](tbl, T=c["T"], p=c["p"], OmegaGrid=g14_axis(c), Diluent=c["Diluent"], **kw)
        r = g["xs_" + c["tag"]]
        assert np.max(np.abs(xs - r)) <= 1e-10 * np.max(np.abs(r)), c["tag"]


def test_g14_cases_exercise_the_foreign_columns(golden):
    """The fixture is not air in disguise: each foreign-broadener case differs from the air-only cross section."""
    g = golden("g14_diluents.npz")
    tbl = g14_table(g)
    for c in g14_cases(g):
        if c["tag"] == "voigt_no_columns":
            continue
        fn = ref.absorptionCoefficient_Lorentz if c["fn"] == "Lorentz" else ref.absorptionCoefficient_Voigt
        kw = {"HITRAN_units": c["HITRAN_units"]} if "HITRAN_units" in c else {}
        _, xa = fn(tbl, T=c["T"], p=c["p"], OmegaGrid=g14_axis(c), **kw)
        r = g["xs_" + c["tag"]]
        assert np.max(np.abs(xa - r)) > 1e-3 * np.max(np.abs(r)), c["tag"]


def test_g14_no_columns_and_fallbacks(golden):
    """A diluent without any column adds nothing; a foreign n of 0 stays 0 while a self n of 0 falls back to n_air."""
    g = golden("g14_diluents.npz")
    tbl = g14_table(g)
    nc = [c for c in g14_cases(g) if c["tag"] == "voigt_no_columns"][0]
    P = ref.line_params(tbl, nc["T"], nc["p"], Diluent=nc["Diluent"])
    Pa = ref.line_params(tbl, nc["T"], nc["p"], Diluent={"air": nc["Diluent"]["air"]})
    assert np.array_equal(P["Gamma0"], Pa["Gamma0"]) and np.array_equal(P["Shift0"], Pa["Shift0"])
    z = tbl["n_co2"] == 0.0
    assert z.any()
    T, p = 250.0, 1.0
    P = ref.line_params(tbl, T, p, Diluent={"co2": 1.0})
    np.testing.assert_allclose(P["Gamma0"][z], tbl["gamma_co2"][z] * p, rtol=1e-15)
    zs = tbl["n_self"] == 0.0
    P = ref.line_params(tbl, T, p, Diluent={"self": 1.0})
    np.testing.assert_allclose(P["Gamma0"][zs], tbl["gamma_self"][zs] * p * (296.0 / T) ** tbl["n_air"][zs], rtol=1e-15)


def _stdatmos():
    o = rt.options
    return np.asarray(o["MFs_VAL"], dtype=np.float64), np.asarray(o["MFs_ID"])


def test_broadening_self_fractions():
    MF, ID = _stdatmos()
    species = [(1, 1), (1, 2), (2, 1), (6, 1), (99, 1)]  # molecule 99 is not in MFs_ID
    f = engine.broadening_fractions(species, MF, ID, engine.broadening_gases("self"))
    assert list(f) == ["air", "self"]
    nL = MF.shape[0]
    x = np.stack([MF[:, 0], MF[:, 0], MF[:, 1], MF[:, 5], np.zeros(nL)]) * 1e-6
    assert np.array_equal(f["self"], x)
    assert np.array_equal(f["air"], 1.0 - x)
    assert f["air"].shape == (len(species), nL) and np.all(f["air"][4] == 1.0)
    assert 0.005 < x[0, 0] < 0.05  # H2O near the surface: the percent level the option is about


def test_broadening_foreign_fractions():
    MF, ID = _stdatmos()
    species = [(1, 1), (2, 1), (3, 1)]
    f = engine.broadening_fractions(species, MF, ID, engine.broadening_gases(("self", "H2O")))
    assert list(f) == ["air", "self", "h2o"]
    xh = MF[:, 0] * 1e-6
    assert np.all(f["h2o"][0] == 0.0)  # an H2O line takes self, not its own foreign column
    assert np.array_equal(f["h2o"][1], xh) and np.array_equal(f["h2o"][2], xh)
    assert np.array_equal(f["self"][0], xh)
    total = f["self"] + f["h2o"]
    assert np.array_equal(f["air"], 1.0 - total)
    np.testing.assert_allclose(f["air"] + f["self"] + f["h2o"], 1.0, rtol=0, atol=1e-15)


def test_broadening_option_values():
    assert engine.broadening_gases(None) is None
    assert engine.broadening_gases("self") == ()
    assert engine.broadening_gases(["self", "CO2", "h2o"]) == ("co2", "h2o")
    for bad in ("air", ("h2o",), ("self", "self"), ("self", "h2o", "H2O"), ("self", "xe")):
        with pytest.raises(ValueError):
            engine.broadening_gases(bad)


def test_broadening_not_in_module_options():
    assert "broadening" not in rt.options


def test_jacobian_refuses_broadening():
    with pytest.raises(NotImplementedError, match="broadening"):
        rt.compute_TUD_jacobian(1000.0, 1001.0, DVOUT=0.01, line_table={"nu": np.zeros(0)}, broadening="self")


def test_sharded_drivers_refuse_broadening():
    from radtxfr_amd import dist
    with pytest.raises(NotImplementedError, match="broadening"):
        dist.compute_TUD_sharded(1000.0, 1001.0, 0.01, None, [0.0], [296.0], [101325.0], [1.0], [[1.0]], [1],
                                 broadening="self")
    with pytest.raises(NotImplementedError, match="broadening"):
        dist.LocalShardedTud([0], 1000.0, 1001.0, 0.01, None, [0.0], [296.0], [101325.0], broadening="self")
    with pytest.raises(NotImplementedError, match="broadening"):
        dist.hsi_cube_from_atmosphere(1000.0, 1001.0, 0.01, None, [0.0], [296.0], [101325.0], [1.0], [[1.0]], [1], None, None,
                                      None, None, None, broadening="self")
