"""Every path of the speed-dependent Voigt line-sum (rtx_sdvoigt_sum: sdvoigt_tile_kernel, and the point-by-point
sdvoigt_kernel under RADTXFR_SD_KERNEL=gather) against the oracle's own formula in long double, point by point and
state by state, on the cases of tests/sdvoigt_cases.py. tests/test_sdvoigt_paths_host.py proves on the CPU that each
case reaches the paths it names and that the reference is sound.

Metric (sdvoigt_cases.judge), per state and point i, with want the long-double sum, want64 the float64 oracle:
    den_i = sum_l |WS_l profile_l(i)|           (long double; |want_i| where every term is positive)
    own_i = max_{|j - i| <= 64} |want64_j - want_j|   (what the reference's own fp64 arithmetic loses there)
    |got_i - want_i| <= 1e-9 den_i + 4 own_i,    and got_i == 0 exactly where den_i == 0.
1e-9 is this path's contract; the 4 covers a second fp64 evaluation of the same ill-conditioned expressions
(PART4's W1 - W2, sqrt(X + Y) - csqrtY for a tiny Gamma2) in another order. Points at which a branch predicate differs
between the two precisions are dropped (none in these cases but zn_switch_on_point; the host test caps them).

Measured figures, per case and kernel: profiles/sdvoigt_paths_accuracy.txt; what they mean: DESIGN 4.7."""
import ctypes as C
import os

import numpy as np
import pytest

import sdvoigt_cases as SC

pytestmark = pytest.mark.gpu

ENV = "RADTXFR_SD_KERNEL"
VS_GATHER = 1e-9  # of den: the bound of test_sdvoigt_node_levels_equal_point_by_point (header: 6e-11 tile + 1e-10 row level)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    from radtxfr_amd import _lib, engine
    _lib.load()
    return engine


def run(eng, case, g=None, out32=False, out64=True, scale=1.0, lines=None, gather=False):
    """engine.voigt_sum(profile=3) on the case's grid (or the shard g); ([states][points] fp32 as float64 or None, fp64 or None)."""
    import torch
    own = lines is None
    lines = lines or eng.LineTable(case["tbl"])
    grid = eng.Grid(*(g or case["grid"]))
    nL = case["T"].size
    o32 = torch.full((nL, grid.n), float("nan"), dtype=torch.float32, device="cuda") if out32 else None
    o64 = torch.full((nL, grid.n), float("nan"), dtype=torch.float64, device="cuda") if out64 else None
    old = os.environ.get(ENV)
    try:
        if gather:
            os.environ[ENV] = "gather"
        else:
            os.environ.pop(ENV, None)
        eng.voigt_sum(lines, grid, case["T"], case["p"], 1.0, out_f32=o32, out_f64=o64, omega_wing=case["ow"],
                      omega_wing_hw=case["hw"], intensity_threshold=case["thresh"], scale=scale, profile=3)
        torch.cuda.synchronize()
    finally:
        if old is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = old
        if own:
            lines.close()
    return (o32.cpu().numpy() if out32 else None), (o64.cpu().numpy() if out64 else None)


def check(tag, name, got, ref):
    """Every state of `got` under the metric; prints the three recorded figures and returns the worst ratio to the bound."""
    worst = (0.0, 0.0, 0.0)
    for k in range(len(ref["want"])):
        e_den, e_allow, share, zeros = SC.judge(got[k], ref, k)
        assert zeros, (tag, name, k, "a point outside every window is not exactly 0")
        assert np.isfinite(got[k]).all() and e_allow <= 1.0, (tag, name, k, e_den, e_allow)  # (a NaN ratio fails here too)
        worst = (max(worst[0], e_den), max(worst[1], e_allow), max(worst[2], share))
    print("sdvoigt_paths %-7s %-22s err/den %.3e  err/bound %.3e  own-dominated %.3f" % ((tag, name) + worst))
    assert worst[1] <= 1.0, (tag, name, worst)
    return worst


_GOT = {}


def _result(eng, name, gather):
    if (name, gather) not in _GOT:
        _GOT[(name, gather)] = run(eng, SC.CASES[name], gather=gather)[1]
    return _GOT[(name, gather)]


# ------------------------------------------------------------------------------------------------ every case, both kernels
@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_default_kernel_vs_long_double_oracle(eng, name):
    check("tile", name, _result(eng, name, False), SC.oracle(name))


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_gather_kernel_vs_long_double_oracle(eng, name):
    """sdvoigt_profile at every point of every window, no interpolation in between."""
    check("gather", name, _result(eng, name, True), SC.oracle(name))


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_default_vs_gather(eng, name):
    """The node levels against the point-by-point sum of the same profile function: 1e-9 of den (the kernel header's
    interpolation bounds are 6e-11 at the tile level and 1e-10 at the row level, of a line's own contribution)."""
    ref = SC.oracle(name)
    a, b = _result(eng, name, False), _result(eng, name, True)
    assert np.isfinite(a).all() and np.isfinite(b).all(), name
    worst = 0.0
    for k in range(len(ref["den"])):
        den = ref["den"][k]
        nz = den != 0
        assert np.array_equal(a[k][~nz], b[k][~nz])
        if nz.any():
            e = float(np.max(np.abs(a[k][nz] - b[k][nz]).astype(np.longdouble) / den[nz]))
            assert e <= VS_GATHER, (name, k, e)
            worst = max(worst, e)
    print("sdvoigt_paths tile-vs-gather %-22s %.3e of den" % (name, worst))
    assert worst <= VS_GATHER, (name, worst)


# ------------------------------------------------------------------------------------------------------------- shards
@pytest.mark.parametrize("name", sorted(n for n, c in SC.CASES.items() if c["shards"]))
def test_shards(eng, name):
    """Shards off a tile boundary, a one-point shard on the grid's last point (X = xmax) and a tile-aligned shard, on both
    kernels under the metric; the tile-aligned shard equals the same points of the full-grid call bit for bit (candidate
    ranges from the full-axis maxhw, node positions from the global index)."""
    case = SC.CASES[name]
    full = _result(eng, name, False)
    lines = eng.LineTable(case["tbl"])
    for off, n in case["shards"]:
        g = case["grid"][:3] + (off, n)
        ref = SC.oracle(name, g)
        for gather in (False, True):
            got = run(eng, case, g=g, lines=lines, gather=gather)[1]
            check("gather" if gather else "tile", "%s[%d:+%d]" % (name, off, n), got, ref)
            if not gather and off % 1024 == 0:
                assert np.array_equal(got, full[:, off:off + n]), (name, off, n)
    lines.close()


# ------------------------------------------------------------------------------------------------------------ outputs
@pytest.mark.parametrize("scale", [1.0, 2.0 ** 70])
def test_outputs_and_scale(eng, scale):
    """out_f32 only, out_f64 only and both: the same values each time, out_f64 unscaled, out_f32 = float32(out_f64 * scale)."""
    name = "ly_three"
    case, ref = SC.CASES[name], SC.oracle(name)
    lines = eng.LineTable(case["tbl"])
    for gather in (False, True):
        b32, b64 = run(eng, case, out32=True, scale=scale, lines=lines, gather=gather)
        o32, _ = run(eng, case, out32=True, out64=False, scale=scale, lines=lines, gather=gather)
        _, o64 = run(eng, case, scale=scale, lines=lines, gather=gather)
        assert np.array_equal(o32, b32) and np.array_equal(o64, b64)
        assert b32.dtype == np.float32 and np.array_equal(b32, (b64 * scale).astype(np.float32))
        assert np.array_equal(b64, _result(eng, name, gather))  # out_f64 does not depend on scale
        check("gather" if gather else "tile", "%s*%g" % (name, scale), b64, ref)
        assert np.any(b32 != 0.0)
    lines.close()


def test_leading_dimension_and_fewer_layers_through_the_c_abi(eng):
    """rtx_sdvoigt_sum with ld > n: rows correct, the padding still NaN; a second sum with fewer n_layers after the same
    prologue writes those states only."""
    import torch
    from radtxfr_amd import _lib
    lib = _lib.load()
    name = "ly_three"
    case = SC.CASES[name]
    lines = eng.LineTable(case["tbl"])
    grid = eng.Grid(*case["grid"])
    nL, n = case["T"].size, grid.n
    for gather in (False, True):
        r32, r64 = run(eng, case, out32=True, scale=2.0 ** 70, lines=lines, gather=gather)  # the prologue and the reference rows
        ld = n + 77
        old = os.environ.get(ENV)
        try:
            if gather:
                os.environ[ENV] = "gather"
            else:
                os.environ.pop(ENV, None)
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            o32 = torch.full((nL, ld), float("nan"), dtype=torch.float32, device="cuda")
            o64 = torch.full((nL, ld), float("nan"), dtype=torch.float64, device="cuda")
            _lib.check(lib.rtx_sdvoigt_sum(lines.plan(nL, n)._h, grid.byref(), nL, C.c_void_p(o32.data_ptr()),
                                           C.c_void_p(o64.data_ptr()), ld, st))
            f64 = torch.full((nL, n), float("nan"), dtype=torch.float64, device="cuda")
            _lib.check(lib.rtx_sdvoigt_sum(lines.plan(nL, n)._h, grid.byref(), nL - 1, C.c_void_p(0), C.c_void_p(f64.data_ptr()), n, st))
            torch.cuda.synchronize()
        finally:
            if old is None:
                os.environ.pop(ENV, None)
            else:
                os.environ[ENV] = old
        p32, p64, few = o32.cpu().numpy(), o64.cpu().numpy(), f64.cpu().numpy()
        assert np.isnan(p32[:, n:]).all() and np.isnan(p64[:, n:]).all()
        assert np.array_equal(p32[:, :n], r32) and np.array_equal(p64[:, :n], r64)
        assert np.array_equal(few[:nL - 1], r64[:nL - 1]) and np.isnan(few[nL - 1]).all()
    lines.close()


# ---------------------------------------------------------------------------------------------------- reproducibility
def test_same_call_twice_is_bit_equal(eng):
    for name in ("ls_mixed_520", "ly_three", "sh_n_2049"):
        for gather in (False, True):
            again = run(eng, SC.CASES[name], gather=gather)[1]
            assert np.array_equal(again, _result(eng, name, gather)), (name, gather)
