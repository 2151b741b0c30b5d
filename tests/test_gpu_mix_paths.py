"""The mixed prologue with FOREIGN broadener column sets (rtx_lines.hip: line_phys<MIX = true>, dil_cols, dil_sd;
rtx_lines_set_broadeners; rtx_line_prep_mix / _axis_mix; engine.diluent_mix; LineTable.broadener_sets) on the GPU, point by
point against the fp64 definition of tests/mix_cases.py, at the smallest shapes at which each thing can go wrong.
tests/test_mix_host.py proves on the CPU that each case reaches what it names and that every defect of
mix_cases.MUTATIONS -- a fraction stride, dil_idx[d] taken for d, a column set off by one, a fallback on the wrong kind of
set, deltap dropped, Gamma2 from the wrong column, stale fractions -- moves the definition by at least 100 x the bound here.

Bounds (none of them new; every measured figure: profiles/mix_paths_accuracy.txt):
  * Voigt / Lorentz, grid and axis, fp32 and fp64 outputs: linesum_metric.pointwise_err <= TOL = 1e-5, the bound the same
    line-sum kernels hold against this oracle; structural zeros exact. The mix changes fp64 prologue values only. CASE_TOL
    is empty; worst measured WORST_VOIGT below.
  * speed-dependent Voigt, both kernels: sdvoigt_cases.judge's ratio <= 1 (1e-9 of den + 4 own).
  * TUD route: TOL on the optical depths, TOL_TAU = 2e-6 and TOL_L = 1e-5 (tests/test_gpu_broadening.py) on tau, Lu, Ld.
Exact contracts (bit for bit): the C ABI route against the engine route; a tile-aligned shard against the full grid through
the MIX skip branch; one layer of a many-layer call against its own call; a reused prep object, a reused LineTable and a
table whose sets were dropped and uploaded again against fresh ones; compute_TUD(returnOD=True) against
engine.optical_depths. Another key order, and repeated keys against their merged fractions, regroup the fp64 sums of the
prologue: held to TOL, not to bits (which of them came out bit-identical is in the profile file).
Refusals return a status before any launch.

Non-zero where the definition is above fp32's normal range: asserted where the definition also exceeds NONZERO_ABOVE =
4 x 8.0e-11 of the largest value within the metric's halo. 8.0e-11 of w(0) is what the reference's own Weideman-24 is off
exp(-x^2) at y = 0 (tests/test_mix_host.py measures it on m_none: the definition against the Doppler profile in closed
form), so under it a value of the definition is that error, not the line. Without the second condition the check cannot
hold on a y = 0 line: the nodal kernel's outer band rows (every lane |x| >= 5.5) take the asymptotic series, which is
proportional to y and so exactly 0 there, where the true profile is exp(-x^2) <= 7.3e-14 of the peak and the definition
is +-5e-11 of it with either sign. First run: m_none is 0 at 10 points where the definition is above fp32's normal range,
all at or under 1.29e-11 of the local peak; no other case has such a point.

m_none's 2.65e-06 is the reference's own error too, as a_upper_atmosphere's 3.2e-6 in tests/test_gpu_linesum_paths.py: 8e-11
of w(0) against the metric's floor of 1e-5 of the local peak leaves up to 8e-6."""
import ctypes as C
import os
from collections import OrderedDict

import numpy as np
import pytest

import mix_cases as MC
import sdvoigt_cases as SC
from linesum_metric import TOL, _local_max, pointwise_err
from test_gpu_broadening import TOL_L, TOL_TAU, _oracle_od
from test_gpu_sdvoigt_paths import ENV as SD_ENV
from test_mix_host import REF_ERR_Y0, TUD_SPECIES, tud_mixing_ratios

pytestmark = pytest.mark.gpu

CASE_TOL = {}  # case -> bound looser than TOL, from the reference's own error (none needed)
WORST_VOIGT = "2.65e-06 (m_none, both outputs), then 5.41e-07 (m_frac_strides)"  # first run on an MI355X: profiles/mix_paths_accuracy.txt
NONZERO_ABOVE = 4 * REF_ERR_Y0  # of the local peak: under it the definition's value is the reference's own Weideman-24 error
PAD = 5
F32_MIN = 1.1754944e-38


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    from radtxfr_amd import _lib, engine
    _lib.load()
    return engine


_WANT = {}


def want_of(name, g=None):
    """The definition of case `name` (on the shard g); computed once, shared, read-only."""
    if (name, g) not in _WANT:
        _WANT[(name, g)] = MC.definition(MC.CASES[name], g=g)
        _WANT[(name, g)].setflags(write=False)
    return _WANT[(name, g)]


def table_of(eng, case, register=True):
    """A fresh LineTable of the case; with case["sets"] those broadeners are on the device first, in that order."""
    lines = eng.LineTable(case["tbl"])
    if register and case.get("sets"):
        assert lines.broadener_sets(list(case["sets"])) == [2 + j for j in range(len(case["sets"]))]
    return lines


def run(eng, case, g=None, lines=None, layers=None, diluent=None, gather=False, out32=True, **kw):
    """engine.voigt_sum / voigt_sum_axis of the case with diluent=case["diluent"] (or `diluent`), weight 1 for each species,
    on the shard g / for the layers `layers`; outputs filled with NaN first. Returns (out_f32 as float64 or None, out_f64)."""
    import torch
    own = lines is None
    lines = lines or table_of(eng, case)
    sel = slice(None) if layers is None else layers
    T, p = case["T"][sel], case["p"][sel]
    dil = case["diluent"] if diluent is None else diluent
    if layers is not None:
        dil = OrderedDict((nm, np.ascontiguousarray(np.asarray(v)[:, sel]) if np.ndim(v) == 2 else v) for nm, v in dil.items())
    nS, nL = len(lines.species), T.size
    sd = case["profile"] == 3
    axis = "X" in case
    n = case["X"].size if axis else (g or case["grid"])[4]
    o32 = torch.full((nL, n), float("nan"), dtype=torch.float32, device="cuda") if out32 and not sd else None
    o64 = torch.full((nL, n), float("nan"), dtype=torch.float64, device="cuda")
    args = dict(out_f32=o32, out_f64=o64, omega_wing=case["ow"], omega_wing_hw=case["hw"], profile=case["profile"], diluent=dil)
    args.update(kw)
    old = os.environ.get(SD_ENV)
    try:
        if gather:
            os.environ[SD_ENV] = "gather"
        else:
            os.environ.pop(SD_ENV, None)
        if axis:
            eng.voigt_sum_axis(lines, case["X"], T, p, np.ones((nS, nL)), **args)
        else:
            eng.voigt_sum(lines, eng.Grid(*(g or case["grid"])), T, p, np.ones((nS, nL)), **args)
        torch.cuda.synchronize()
    finally:
        if old is None:
            os.environ.pop(SD_ENV, None)
        else:
            os.environ[SD_ENV] = old
        if own:
            lines.close()
    return (o32.double().cpu().numpy() if o32 is not None else None), o64.cpu().numpy()


# ---- the C ABI, without engine.diluent_mix and LineTable.broadener_sets ---------------------------------------------------
def upload_sets(eng, lines, tbl, sps, n_extra=None):
    """rtx_lines_set_broadeners with the columns of `sps` from `tbl` (caller's row order), set j = sps[j]; returns the status."""
    from radtxfr_amd import _lib
    keep, arr = [], []
    for f in MC.FIELDS:
        a = (C.c_void_p * max(len(sps), 1))()
        for j, sp in enumerate(sps):
            if f + sp in tbl:
                col = np.ascontiguousarray(np.asarray(tbl[f + sp], dtype=np.float64)[lines._order])
                keep.append(col)
                a[j] = col.ctypes.data
        arr.append(a)
    return _lib.load().rtx_lines_set_broadeners(lines._h, len(sps) if n_extra is None else n_extra, *arr)


def mix_args(case, sps, names=None, layers=None):
    """(n_dil, set indices int32, fractions [n_dil][nS][nL] contiguous) of the case's diluents `names` (default all, in the
    dict's order) for the column sets 0 air, 1 self, 2 + j sps[j]; a name without a set is left out."""
    sets = {"air": 0, "self": 1, **{sp: 2 + j for j, sp in enumerate(sps)}}
    sel = slice(None) if layers is None else layers
    use = [nm for nm in (names or case["diluent"]) if nm.lower() in sets]
    idx = np.ascontiguousarray([sets[nm.lower()] for nm in use], dtype=np.int32)
    frac = np.ascontiguousarray(np.stack([case["diluent"][nm][:, sel] for nm in use]), dtype=np.float64)
    return len(use), idx, frac


def abi_prep(eng, plan, lines, case, n_dil, idx, frac, layers=None, g=None, profile=None, plain=None):
    """rtx_line_prep_mix / _axis_mix (plain = (dil_air, dil_self): rtx_line_prep_profile / _axis) on prep object `plan`;
    returns the status. idx / frac may be None (NULL)."""
    from radtxfr_amd import _lib
    lib = _lib.load()
    sel = slice(None) if layers is None else layers
    T, p = case["T"][sel], case["p"][sel]
    nL, env = eng._prologue_inputs(lines, T, p, np.ones((len(lines.species), T.size)), None, None, None)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    prof = case["profile"] if profile is None else profile
    tail = (float(case["ow"]), float(case["hw"]), 0.0, 1.0, int(prof), eng._stream_ptr())
    if "X" in case:
        head = (plan._h, lines._h, case["X"].ctypes.data_as(C.c_void_p), case["X"].size, nL, *(e[1] for e in env))
        if plain is not None:
            return lib.rtx_line_prep_axis(*head, float(plain[0]), float(plain[1]), *tail)
        return lib.rtx_line_prep_axis_mix(*head, int(n_dil), ptr(idx), ptr(frac), *tail)
    head = (plan._h, lines._h, eng.Grid(*(g or case["grid"])).byref(), nL, *(e[1] for e in env))
    if plain is not None:
        return lib.rtx_line_prep_profile(*head, float(plain[0]), float(plain[1]), *tail)
    return lib.rtx_line_prep_mix(*head, int(n_dil), ptr(idx), ptr(frac), *tail)


def abi_sum(eng, plan, case, nL, g=None, pad=PAD):
    """rtx_voigt_sum / _axis on the prep object with ld = n + pad into NaN-filled outputs: ([nL][n + pad] fp32 as float64, fp64)."""
    import torch
    from radtxfr_amd import _lib
    lib = _lib.load()
    axis = "X" in case
    n = case["X"].size if axis else (g or case["grid"])[4]
    ld = n + pad
    o32 = torch.full((nL, ld), float("nan"), dtype=torch.float32, device="cuda")
    o64 = torch.full((nL, ld), float("nan"), dtype=torch.float64, device="cuda")
    st = eng._stream_ptr()
    if axis:
        _lib.check(lib.rtx_voigt_sum_axis(plan._h, nL, eng._ptr(o32), eng._ptr(o64), ld, st))
    else:
        _lib.check(lib.rtx_voigt_sum(plan._h, eng.Grid(*(g or case["grid"])).byref(), nL, eng._ptr(o32), eng._ptr(o64), ld, st))
    torch.cuda.synchronize()
    return o32.double().cpu().numpy(), o64.cpu().numpy()


def run_abi(eng, case, g=None, pad=PAD):
    """The case through rtx_lines_set_broadeners + rtx_line_prep_mix / _axis_mix + rtx_voigt_sum / _axis alone."""
    from radtxfr_amd import _lib
    lines = eng.LineTable(case["tbl"])
    try:
        sps = MC._foreign(case)
        _lib.check(upload_sets(eng, lines, case["tbl"], sps))
        n_dil, idx, frac = mix_args(case, sps)
        nL = case["T"].size
        plan = lines.plan(nL, case["X"].size if "X" in case else (g or case["grid"])[4])
        _lib.check(abi_prep(eng, plan, lines, case, n_dil, idx, frac, g=g))
        return abi_sum(eng, plan, case, nL, g=g, pad=pad)
    finally:
        lines.close()


def last_error():
    from radtxfr_amd import _lib
    return (_lib.load().rtx_last_error() or b"").decode()


def check_voigt(tag, name, r32, r64, want):
    e32 = pointwise_err(r32, want) if r32 is not None else 0.0
    e64 = pointwise_err(r64, want)
    per_layer = [pointwise_err(r64[k], want[k]) for k in range(want.shape[0])]
    print("mix_paths %-14s %-18s f32 %.3g f64 %.3g (worst layer %d)" % (tag, name, e32, e64, int(np.argmax(per_layer))))
    tol = CASE_TOL.get(name, TOL)
    assert e32 <= tol and e64 <= tol, (tag, name, e32, e64)
    # not flushed: non-zero wherever the definition is above fp32's normal range AND above the reference's own error
    # (NONZERO_ABOVE of the largest value within the metric's halo; module docstring). The count without the second
    # condition is printed.
    live = (want > F32_MIN) & (want > NONZERO_ABOVE * _local_max(want))
    for r in (r32, r64):
        if r is not None:
            assert np.all(np.isfinite(r)) and np.all(r[want == 0.0] == 0.0), (tag, name)
            lost = (want > F32_MIN) & (r == 0.0)
            if lost.any():
                print("mix_paths %-14s %-18s %d points are 0 where the definition is above fp32's normal range, all at or under "
                      "%.3g of the largest value within 1024 points"
                      % (tag, name, int(lost.sum()), float(np.max((want / _local_max(want))[lost]))))
            assert np.all(r[live] != 0.0), (tag, name)
    return max(e32, e64)


_GOT = {}


def got_of(eng, name):
    if name not in _GOT:
        _GOT[name] = run(eng, MC.CASES[name])
    return _GOT[name]


# ------------------------------------------------------------------------------------------------------------ 1. accuracy
@pytest.mark.parametrize("name", MC.GRID_CASES + MC.AXIS_CASES)
def test_case_vs_definition(eng, name):
    """Every Voigt / Lorentz case, grid and axis, both outputs. (3: m_device_tables is among them.)"""
    r32, r64 = got_of(eng, name)
    check_voigt("engine", name, r32, r64, want_of(name))


def test_lorentz_drop_is_exact_zero(eng):
    """m_lorentz: where only the species with Gamma0 = 0 has lines, layer 2 is exactly 0 and the other layers are not."""
    r32, r64 = got_of(eng, "m_lorentz")
    for r in (r32, r64):
        assert np.all(r[2, 1500:] == 0.0) and np.all(r[:2, 1600:1900].max(axis=1) > 0.0)


def test_m_none_is_the_doppler_core(eng):
    """m_none: n_dil = 0, y = 0 exactly: every line's core (|x| < 3) is there in both layers."""
    c = MC.CASES["m_none"]
    r32, _ = got_of(eng, "m_none")
    X = MC.case_axis(c)
    for k in range(2):
        P = MC.layer_params(c, k)
        assert np.all(P["Gamma0"] == 0.0)
        x = np.abs((X[None, :] - P["nu"][:, None]) * (np.sqrt(np.log(2.0)) / P["GammaD"])[:, None])
        assert np.all(r32[k][(x < 3.0).any(axis=0)] > 0.0)


def test_ninth_key(eng):
    """m_eight plus a ninth key: without columns it is left out and the call gives m_eight's bits; with columns (gamma_o2 is
    on the table) the call is refused, naming the limit."""
    c = MC.CASES["m_eight"]
    nine = OrderedDict(c["diluent"])
    nine["xe"] = np.full((3, 3), 0.25)
    _, r64 = run(eng, c, diluent=nine)
    assert np.array_equal(r64, got_of(eng, "m_eight")[1])
    nine = OrderedDict(c["diluent"])
    nine["o2"] = np.full((3, 3), 0.25)
    with pytest.raises(ValueError, match="at most 8"):
        run(eng, c, diluent=nine)


# ------------------------------------------------------------------------------------------- 2. speed-dependent Voigt
_SDREF = {}


def _sd_reference():
    if "r" not in _SDREF:
        _SDREF["r"] = MC.sd_reference(MC.CASES["m_sdvoigt"])
    return _SDREF["r"]


@pytest.mark.parametrize("kernel", ["tile", "gather"])
def test_sdvoigt_vs_long_double(eng, kernel):
    """m_sdvoigt: Gamma2 summed over four diluents (SD_air, SD_self, SD_h2 with zeros, SD_he absent), on both SD kernels."""
    c = MC.CASES["m_sdvoigt"]
    ref = _sd_reference()
    _, got = run(eng, c, gather=kernel == "gather")
    worst = (0.0, 0.0)
    for k in range(c["T"].size):
        e_den, e_allow, share, zeros = SC.judge(got[k], ref, k)
        assert zeros and np.isfinite(got[k]).all() and e_allow <= 1.0, (kernel, k, e_den, e_allow)
        worst = (max(worst[0], e_den), max(worst[1], e_allow))
    print("mix_paths sdvoigt %-6s err/den %.3e err/bound %.3e" % ((kernel,) + worst))


# ------------------------------------------------------------------------------------------------- 3, 5. the shard
def test_shard_through_the_skip_branch(eng):
    """m_shard on the tile-aligned shard [tile, end): against the definition on the shard's axis, and the same bits as that
    slice of the full-grid run (lines of tile 0 take the MIX prologue's skip branch on the shard, three just reach in)."""
    from radtxfr_amd import _lib
    c = MC.CASES["m_shard"]
    off, n = c["shard"]
    assert off == _lib.load().rtx_voigt_tile_points() == MC.TILE
    g = c["grid"][:3] + (off, n)
    f32, f64 = run(eng, c)
    check_voigt("full", "m_shard", f32, f64, want_of("m_shard"))
    s32, s64 = run(eng, c, g=g)
    check_voigt("shard", "m_shard", s32, s64, want_of("m_shard", g))
    assert np.array_equal(s32, f32[:, off:off + n]) and np.array_equal(s64, f64[:, off:off + n])


# ------------------------------------------------------------------------------------- 4 - 8. routes with the same bits
@pytest.mark.parametrize("name", ["m_sets_order", "m_axis"])
def test_c_abi_equals_engine(eng, name):
    c = MC.CASES[name]
    n = MC.case_axis(c).size
    a32, a64 = run_abi(eng, c)
    assert a32.shape == (c["T"].size, n + PAD) and np.isnan(a32[:, n:]).all() and np.isnan(a64[:, n:]).all(), "padding written"
    r32, r64 = got_of(eng, name)
    assert np.array_equal(a32[:, :n], r32) and np.array_equal(a64[:, :n], r64), name


def test_other_key_order(eng):
    """m_sets_order with the dict reversed, on a fresh table that appends the sets as they come (h2 = 2, he = 3, co2 = 4
    becomes h2 = 2, self, he = 3, air, co2 = 4): other dil_idx, other summation order; the same definition within TOL."""
    c = MC.CASES["m_sets_order"]
    rev = OrderedDict(reversed(list(c["diluent"].items())))
    lines = table_of(eng, c, register=False)
    r32, r64 = run(eng, c, lines=lines, diluent=rev)
    assert lines.broadener_sets(list(rev)) == [2, 1, 3, 0, 4]
    lines.close()
    check_voigt("reversed keys", "m_sets_order", r32, r64, want_of("m_sets_order"))
    print("mix_paths reversed keys bit-identical to the case's order: %s" % np.array_equal(r64, got_of(eng, "m_sets_order")[1]))


def test_repeated_keys_against_merged(eng):
    """m_eight's {"air": a, "AIR": b, "self": c, "SELF": d, ...} against {"air": a + b, "self": c + d, ...}: the same
    physics, other summation order: both within TOL of the definition with the repeated keys."""
    c = MC.CASES["m_eight"]
    d = c["diluent"]
    merged = OrderedDict([("air", d["air"] + d["AIR"]), ("h2", d["h2"]), ("he", d["he"]), ("self", d["self"] + d["SELF"]),
                          ("co2", d["co2"]), ("n2", d["n2"])])
    r32, r64 = run(eng, c, diluent=merged)
    check_voigt("merged keys", "m_eight", r32, r64, want_of("m_eight"))
    print("mix_paths merged keys bit-identical to the repeated ones: %s" % np.array_equal(r64, got_of(eng, "m_eight")[1]))


def test_one_layer_of_many(eng):
    """Each layer of the 4-layer m_frac_strides call equals the 1-layer call with that layer's fractions, bit for bit."""
    c = MC.CASES["m_frac_strides"]
    r32, r64 = got_of(eng, "m_frac_strides")
    lines = table_of(eng, c)
    for k in range(c["T"].size):
        a32, a64 = run(eng, c, lines=lines, layers=slice(k, k + 1))
        assert np.array_equal(a32[0], r32[k]) and np.array_equal(a64[0], r64[k]), k
    lines.close()


# ----------------------------------------------------------------------------------------------------- 9 - 11. stale state
def test_reused_prep_object(eng):
    """One prep object (18-line tables all): m_eight (8 diluents, 3 layers), m_frac_strides with 2 diluents and 2 layers, a
    plain dil_air = 0.7 / dil_self = 0.3 call, m_frac_strides whole. Each equals a fresh LineTable's result, bit for bit."""
    from radtxfr_amd import _lib
    e, f = MC.CASES["m_eight"], MC.CASES["m_frac_strides"]
    le, lf = eng.LineTable(e["tbl"]), eng.LineTable(f["tbl"])
    sp_e, sp_f = MC._foreign(e), MC._foreign(f)
    _lib.check(upload_sets(eng, le, e["tbl"], sp_e))
    _lib.check(upload_sets(eng, lf, f["tbl"], sp_f))
    plan = eng.VoigtPlan(le, 4, 2100)
    two = OrderedDict((nm, f["diluent"][nm]) for nm in ("h2", "self"))
    stages = [("m_eight", e, le, mix_args(e, sp_e), None, None, dict()),
              ("2 diluents, 2 layers", f, lf, mix_args(f, sp_f, names=("h2", "self"), layers=slice(1, 3)), slice(1, 3), None,
               dict(diluent=two, layers=slice(1, 3))),
              ("plain", f, lf, (0, None, None), None, (0.7, 0.3), dict(diluent=OrderedDict(air=0.7, self=0.3))),
              ("m_frac_strides", f, lf, mix_args(f, sp_f), None, None, dict())]
    try:
        for tag, case, lines, (n_dil, idx, frac), layers, plain, fresh_kw in stages:
            _lib.check(abi_prep(eng, plan, lines, case, n_dil, idx, frac, layers=layers, plain=plain))
            nL = case["T"][layers if layers is not None else slice(None)].size
            a32, a64 = abi_sum(eng, plan, case, nL, pad=0)
            if plain is not None:  # the fresh result through the plain entry too
                import torch
                fl = eng.LineTable(case["tbl"])
                o32 = torch.full((nL, 2100), float("nan"), dtype=torch.float32, device="cuda")
                eng.voigt_sum(fl, eng.Grid(*case["grid"]), case["T"], case["p"], np.ones((3, nL)), out_f32=o32, dil_air=0.7, dil_self=0.3,
                              omega_wing=case["ow"], omega_wing_hw=case["hw"])
                torch.cuda.synchronize()
                assert np.array_equal(a32, o32.double().cpu().numpy()), tag
                fl.close()
            r32, r64 = run(eng, case, **fresh_kw)
            assert np.array_equal(a32, r32) and np.array_equal(a64, r64), tag
    finally:
        plan.close()
        le.close()
        lf.close()


def test_reused_line_table_bookkeeping(eng):
    """One LineTable through {"air", "h2"}, {"he", "air", "h2"} (he appended as set 3), {"co2", "h2", "self"} (co2 as set 4),
    then broadener_sets(names, columns, sigs) with another fingerprint and other values for h2 and no he column any more
    (its set deleted, co2 moves down to 3). After every stage the line-sum equals a fresh table's on the same columns."""
    c = MC.CASES["m_eight"]
    tbl = c["tbl"]
    lines = eng.LineTable(tbl)
    mixes = [OrderedDict(air=0.6, h2=0.4), OrderedDict(he=0.2, air=0.5, h2=0.3), OrderedDict(co2=0.3, h2=0.3, self=0.4)]
    held = [[0, 2], [3, 0, 2], [4, 2, 1]]
    try:
        for dil, sets in zip(mixes, held):
            got = run(eng, c, lines=lines, diluent=dil)
            assert lines.broadener_sets(list(dil)) == sets
            fresh = run(eng, c, diluent=dil)
            assert np.array_equal(got[0], fresh[0]) and np.array_equal(got[1], fresh[1]), list(dil)
        tbl2 = {k: v for k, v in tbl.items() if not k.endswith("_he")}
        tbl2["gamma_h2"] = np.round(tbl["gamma_h2"] * 1.5, 4)
        cols = {k: v for k, v in tbl2.items() if k.endswith(("_h2", "_he", "_co2"))}
        ret = lines.broadener_sets(["h2", "he", "co2"], columns=cols, sigs={"h2": ("edited",), "he": (), "co2": None})
        assert ret == [2, None, 3]
        got = run(eng, c, lines=lines, diluent=mixes[2])
        fresh = run(eng, dict(c, tbl=tbl2), diluent=mixes[2])
        assert np.array_equal(got[0], fresh[0]) and np.array_equal(got[1], fresh[1])
        assert pointwise_err(got[1], MC.definition(dict(c, tbl=tbl2), diluent=mixes[2])) <= TOL
        assert pointwise_err(got[1], MC.definition(c, diluent=mixes[2])) > 100 * TOL  # the edit is visible
    finally:
        lines.close()


def test_refused_call_leaves_no_state(eng):
    """A refused rtx_line_prep_mix (n_dil = 9) on a prep object that holds a good prologue; the next valid mix call equals a
    fresh object's, bit for bit."""
    from radtxfr_amd import _lib
    c = MC.CASES["m_sets_order"]
    lines = eng.LineTable(c["tbl"])
    try:
        sps = MC._foreign(c)
        _lib.check(upload_sets(eng, lines, c["tbl"], sps))
        n_dil, idx, frac = mix_args(c, sps)
        plan = lines.plan(3, 2100)
        _lib.check(abi_prep(eng, plan, lines, c, n_dil, idx, frac))
        idx9 = np.zeros(9, dtype=np.int32)
        frac9 = np.full((9, 3, 3), 0.5)
        assert abi_prep(eng, plan, lines, c, 9, idx9, frac9) != 0 and "n_dil=" in last_error()
        _lib.check(abi_prep(eng, plan, lines, c, n_dil, idx, frac))
        a32, a64 = abi_sum(eng, plan, c, 3, pad=0)
    finally:
        lines.close()
    r32, r64 = got_of(eng, "m_sets_order")
    assert np.array_equal(a32, r32) and np.array_equal(a64, r64)


# -------------------------------------------------------------------------------------------------- 12 - 14. refusals
@pytest.mark.parametrize("name", ["m_sets_order", "m_axis"])
def test_prep_mix_refusals(eng, name):
    """rtx_line_prep_mix / _axis_mix: each refusal is a non-zero status with its text, before any launch."""
    from radtxfr_amd import _lib
    c = MC.CASES[name]
    lines = eng.LineTable(c["tbl"])
    try:
        sps = MC._foreign(c)
        _lib.check(upload_sets(eng, lines, c["tbl"], sps))
        n_dil, idx, frac = mix_args(c, sps)
        plan = lines.plan(c["T"].size, MC.case_axis(c).size)

        def refused(text, n=n_dil, i=idx, f=frac, **kw):
            assert abi_prep(eng, plan, lines, c, n, i, f, **kw) != 0, text
            assert text in last_error(), (text, last_error())

        refused("n_dil=", n=-1)
        refused("n_dil=", n=9, i=np.zeros(9, np.int32), f=np.zeros((9,) + frac.shape[1:]))
        bad = idx.copy()
        bad[1] = 2 + len(sps)
        refused("column set", i=bad)
        bad[1] = -1
        refused("column set", i=bad)
        refused("NULL", i=None)
        refused("NULL", f=None)
        refused("takes no diluent", profile=2)
        if "X" in c:
            refused("profile=3", profile=3)
        assert abi_prep(eng, plan, lines, c, n_dil, idx, frac) == 0  # and the good call still goes through
    finally:
        lines.close()


def test_set_broadeners_refusals_and_reupload(eng):
    """rtx_lines_set_broadeners: n_extra = 65 is refused; n_extra = 0 drops the sets (a mix call with set 2 is then refused);
    two sets uploaded again give the bits of a fresh table."""
    from radtxfr_amd import _lib
    c = MC.CASES["m_frac_strides"]
    lines = eng.LineTable(c["tbl"])
    try:
        sps = MC._foreign(c)
        assert len(sps) == 2
        _lib.check(upload_sets(eng, lines, c["tbl"], sps))
        assert upload_sets(eng, lines, c["tbl"], sps * 33, n_extra=65) != 0 and "n_extra=65" in last_error()
        _lib.check(upload_sets(eng, lines, c["tbl"], sps))
        _lib.check(upload_sets(eng, lines, c["tbl"], [], n_extra=0))
        n_dil, idx, frac = mix_args(c, sps)
        plan = lines.plan(4, 2100)
        assert abi_prep(eng, plan, lines, c, n_dil, idx, frac) != 0 and "column set" in last_error()
        _lib.check(upload_sets(eng, lines, c["tbl"], sps))
        _lib.check(abi_prep(eng, plan, lines, c, n_dil, idx, frac))
        a32, a64 = abi_sum(eng, plan, c, 4, pad=0)
    finally:
        lines.close()
    r32, r64 = got_of(eng, "m_frac_strides")
    assert np.array_equal(a32, r32) and np.array_equal(a64, r64)


def test_engine_refusals(eng):
    """engine.voigt_sum(profile=2, diluent=) is refused by the C layer with its text; voigt_sum_window and voigt_sum_dT take
    no diluent at all (the call-wide dil_air / dil_self only): the keyword is refused by name."""
    import torch
    from radtxfr_amd import _lib
    c = MC.CASES["m_frac_strides"]
    lines = table_of(eng, c)
    grid = eng.Grid(*c["grid"])
    out = torch.zeros((4, grid.n), dtype=torch.float32, device="cuda")
    w = np.ones((3, 4))
    try:
        with pytest.raises(_lib.RtxError, match="takes no diluent"):
            eng.voigt_sum(lines, grid, c["T"], c["p"], w, out_f32=out, profile=2, diluent=c["diluent"])
        with pytest.raises(_lib.RtxError, match="takes no diluent"):
            eng.voigt_sum_axis(lines, grid.axis(), c["T"], c["p"], w, out_f32=out, profile=2, diluent=c["diluent"])
        with pytest.raises(TypeError, match="diluent"):
            eng.voigt_sum_window(lines, grid, c["T"], c["T"], c["p"], w, out, diluent=c["diluent"])
        with pytest.raises(TypeError, match="diluent"):
            eng.voigt_sum_dT(lines, grid, c["T"], c["p"], w, out, diluent=c["diluent"])
        torch.cuda.synchronize()
        assert not out.any()  # nothing was launched into it
    finally:
        lines.close()


# --------------------------------------------------------------------------------------------------- 15. the TUD route
def _tud_inputs():
    """<= 40 H2O + CO2 + O3 lines with gamma_h2o, n_h2o, gamma_co2, delta_co2 on 2000 points; four layers, 1 ... 0.1 atm,
    296 ... 220 K, H2O and CO2 (and O3) at 5 - 30 % in every layer (tests/test_mix_host.py: tud_mixing_ratios)."""
    lo, hi, dv = 1000.0, 1004.0, 0.002
    rng = np.random.default_rng(31)
    nu = np.round(np.sort(rng.uniform(lo - 1.0, hi + 1.0, 36)), 4) + 2.5e-4
    tbl = MC.mix_table(nu, 31, species=TUD_SPECIES, sw=np.round(10.0 ** rng.uniform(-26.5, -25.3, 36), 29))
    tbl["delta_air"] = np.round(rng.uniform(-0.008, 0.002, 36), 6)
    tbl["gamma_h2o"] = np.round(rng.uniform(0.15, 0.4, 36), 4)
    tbl["n_h2o"] = np.round(rng.uniform(0.5, 0.9, 36), 2)
    tbl["gamma_co2"] = np.round(rng.uniform(0.06, 0.12, 36), 4)
    tbl["delta_co2"] = np.round(rng.uniform(-0.01, 0.004, 36), 6)
    MF, ID = tud_mixing_ratios()
    a = dict(Zs=np.array([0.5, 2.0, 6.0, 14.0]), Ts=np.array([296.0, 275.0, 245.0, 220.0]),
             Ps=np.array([1.0, 0.7, 0.35, 0.1]) * 101325.0, PLs=np.array([1.0, 2.0, 4.0, 8.0]), MFs_VAL=MF, MFs_ID=ID)
    return lo, hi, dv, tbl, a


def test_tud_route_with_foreign_sets(eng):
    from radtxfr_amd import radiative_transfer as rt
    from oracle import cpu_ref
    lo, hi, dv, sub, a = _tud_inputs()
    B = ("self", "h2o", "co2")
    X = rt.make_spectral_axis(lo, hi, dv)
    assert X.size <= 2001 and sub["nu"].size <= 40
    ODr = _oracle_od(sub, X, a, range(4), foreign=("h2o", "co2"))
    tbl = rt._resolve_table(sub, ("h2o", "co2"))
    assert tbl.species == TUD_SPECIES
    grid = eng.Grid(lo, hi, X.size)
    od32 = eng.optical_depths(tbl, grid, a["Ts"], a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"], broadening=B).cpu().numpy()
    od = od32.astype(np.float64)
    for k in range(4):
        e = pointwise_err(od[k], ODr[k])
        print("mix_paths tud optical depth layer %d: %.3g (max OD %.3g)" % (k, e, ODr[k].max()))
        assert e <= TOL, (k, e)
    od_self = eng.optical_depths(tbl, grid, a["Ts"], a["Ps"], a["PLs"], a["MFs_VAL"], a["MFs_ID"], broadening="self").double().cpu().numpy()
    assert min(pointwise_err(od_self[k], ODr[k]) for k in range(4)) > 100 * TOL  # the foreign sets matter in every layer
    # compute_TUD(returnOD=True) with layer k alone below the sensor: its tau slot is that layer's optical depth
    for k in range(4):
        Zs = np.full(4, 5.0)
        Zs[k] = 0.1
        _, tau, _, _ = rt.compute_TUD(lo, hi, DVOUT=dv, line_table=sub, Altitudes=np.asarray([1.0]), broadening=B, returnOD=True,
                                      **dict(a, Zs=Zs))
        assert np.array_equal(np.asarray(tau), od[k]), k
    _, tau, Lu, Ld = rt.compute_TUD(lo, hi, DVOUT=dv, line_table=sub, Altitudes=np.asarray([500]), broadening=B, **a)
    tau_r, Lu_r, Ld_r = cpu_ref.tud_from_od(X, ODr.T, a["Ts"], a["Zs"], Altitudes=(500,))
    from conftest import rel_err
    e_tau, e_lu, e_ld = float(np.max(np.abs(tau - tau_r))), rel_err(Lu, Lu_r), rel_err(Ld, Ld_r)
    print("mix_paths tud tau %.3g Lu %.3g Ld %.3g (tau from %.3g to %.3g)" % (e_tau, e_lu, e_ld, tau_r.min(), tau_r.max()))
    assert 0.0 < tau_r.min() < 0.5 < tau_r.max() < 1.0
    assert e_tau <= TOL_TAU and e_lu <= TOL_L and e_ld <= TOL_L


# ------------------------------------------------------------------------------------------------------------ 16. hapi
@pytest.mark.parametrize("fn", ["Voigt", "Lorentz"])
def test_hapi_dropins_pointwise(eng, fn):
    """absorptionCoefficient_Voigt / _Lorentz with Diluent = {"xe": 1} (no columns) and with m_eight's eight keys on a cached
    table, against the definition in the pointwise metric (the g14 goldens hold these calls under conftest.rel_err only)."""
    from radtxfr_amd import hapi
    c = MC.CASES["m_eight"]
    X = MC.case_axis(c)
    name = "mix_paths_" + fn
    hapi.storage2cache_from_columns(name, c["tbl"])
    prof = 1 if fn == "Lorentz" else 0
    try:
        for tag, T, p, dil, hw in (("xe", 250.0, 0.05, OrderedDict(xe=1.0), 50.0),
                                   ("eight", 250.0, 0.4, OrderedDict((nm, float(v[1, 2])) for nm, v in c["diluent"].items()), 4.0)):
            one = dict(c, T=np.array([T]), p=np.array([p]), profile=prof, hw=hw)
            want = MC.definition(one, diluent=dil)
            _, xs = getattr(hapi, "absorptionCoefficient_" + fn)(SourceTables=name, Environment={"T": T, "p": p}, OmegaGrid=X,
                                                                 OmegaWingHW=hw, Diluent=dil)
            if fn == "Lorentz" and tag == "xe":  # Gamma0 = 0: every window is empty
                assert not want.any() and not np.asarray(xs).any()
                continue
            assert want.max() > 0.0
            e = pointwise_err(xs, want[0])
            print("mix_paths hapi %-7s %-5s %.3g" % (fn, tag, e))
            assert e <= TOL, (fn, tag, e)
            assert np.all(xs[want[0] == 0.0] == 0.0)
    finally:
        hapi.LOCAL_TABLE_CACHE.pop(name, None)
