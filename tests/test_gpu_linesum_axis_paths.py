"""Every path of the explicit-axis line-sum (rtx_line_prep_axis / _axis_mix: line_prep_axis_kernel; rtx_voigt_sum_axis:
tile_ranges_kernel on index-space inputs, voigt_axis_kernel) against the fp64 oracle, point by point and layer by layer.

a-d. The cases of tests/linesum_axis_cases.py on non-uniform axes, one path at a time: band rows of y < 1 (fp64 Weideman),
     1 <= y < 6 on both sides of the |z| < 8 ballot and y >= 6 at 1000 and 6000 cm^-1; |x| + y = 15 exactly on axis points
     with their nextafter neighbours and points inside and outside the 2e-3 collar; the upper atmosphere down to
     y ~ 1e-6; Lorentz and Doppler records with and without the line shift; a per-layer diluent mix; tiles spanning 0,
     0.5, 20 and 2000 cm^-1 with a narrow line at their far end (the two-float abscissa); repeated points; window edges
     on row and tile boundaries, on axis points, between two points, outside the axis; bands that are empty, clamped to
     the window, cut by the axis end; two-density axes, tiles with 0, 1, 2, 3, 5 and ~600 candidates, 1 atm and 1e-4 atm
     in one call. tests/test_linesum_axis_host.py proves on the CPU that each case reaches the paths it names
     (cpu_ref.axis_census), that the abscissa case can tell the one-FMA form from the kernel's, and that the metric's floor
     covers no path a case is named for.
e.   The uniform cases of tests/linesum_cases.py (a-d) with their grids as explicit axes: against the oracle, and against
     rtx_voigt_sum of the same case at the bounds tests/test_gpu_linesum_paths.py holds its two kernels to.
f.   X[:n] for n in {1, 2, 63, 64, 65, 1023, 1024, 1025, 2049} (prefix bit-identity: the trimmed ranges are canonical),
     ld > nx through the C ABI, a second sum after one prologue, 1 and 64 layers against their one-layer calls, layers
     alternating between 1 atm and 1e-4 atm.

Metric: tests/linesum_metric.py -- err_i = |got_i - want_i| / max(|want_i|, F max_{|j - i| <= 1024} |want_j|, F32_FLOOR) per
layer, at most TOL = 1e-5; points where the oracle is exactly 0 must be exactly 0. The Doppler oracle's values beyond
|x| = 15 (<= 1e-98 of the peak; the kernel returns 0 there) lie under F32_FLOOR and are compared absolutely.

No case needs a bound looser than TOL against the oracle (CASE_TOL is empty); measured figures:
profiles/linesum_axis_paths_accuracy.txt. Worst: the Doppler cases at 6.8e-6 -- a Doppler record's band lanes take fp64
Weideman-24 at y = 0, which is up to 8.0e-11 of w(0) off the oracle's exp(-x^2) (7.2e-11 at 3 <= |x| < 5.5, where the
profile has fallen under the floor of 1e-5 of the local peak): tests/test_linesum_axis_host.py evaluates that on the CPU.
Against rtx_voigt_sum one case is held to AXIS_VS_GRID_CASE_TOL, the bound test_gpu_linesum_paths.py already uses between
its own two kernels, for the same cause: a_upper_atmosphere -- the axis kernel evaluates every band lane of a y < 1 line in
fp64 Weideman-24, as the reference does, while the nodal kernel's outer rows (every lane |x| >= 5.5) take asymK_re<12>,
which follows the true function; Weideman-24 is 4.1e-11 of w(0) off it there (the same host test), 4.1e-6 of the floor.
The axis path is the side nearer the oracle (4.1e-7 against the nodal kernel's 3.2e-6)."""
import ctypes as C
import math

import numpy as np
import pytest

import linesum_axis_cases as AC
import linesum_cases as LC
from linesum_metric import TOL, pointwise_err

pytestmark = pytest.mark.gpu

CASE_TOL = {}  # case -> bound looser than TOL against the oracle (none needed)
AXIS_VS_GRID = 2e-6  # test_gpu_linesum_paths.SCATTER_VS_NODAL: two fp32 implementations of one sum
AXIS_VS_GRID_CASE_TOL = {"a_upper_atmosphere": 1e-5}  # test_gpu_linesum_paths.SCATTER_CASE_TOL (module docstring)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    from radtxfr_amd import _lib, engine
    _lib.load()
    return engine


_ORACLE = {}


def oracle(name, case):
    if name not in _ORACLE:
        _ORACLE[name] = AC.oracle(case)
        _ORACLE[name].setflags(write=False)
    return _ORACLE[name]


def _scale(case):
    return 2.0 ** (-math.floor(math.log2(float(np.max(case["tbl"]["sw"])))))


def _kw(case, scale):
    kw = dict(omega_wing=case["ow"], omega_wing_hw=case["hw"], scale=scale, profile=case["profile"])
    if case["diluent"] is not None:
        kw["diluent"] = case["diluent"]
    elif case["profile"] == 2:
        kw["dil_air"] = 1.0 if case["lineshift"] else 0.0  # Doppler: Shift0 = delta_air p, or none
    return kw


def run(eng, case, X=None, out32=True, out64=True, scale=None, lines=None, layers=None):
    """engine.voigt_sum_axis of the case (on X, for the layers `layers`): (out_f32 as float64 / scale, out_f64)."""
    import torch
    own = lines is None
    lines = lines or eng.LineTable(case["tbl"])
    X = case["X"] if X is None else X
    scale = _scale(case) if scale is None else scale
    sel = slice(None) if layers is None else layers
    T, p = case["T"][sel], case["p"][sel]
    kw = _kw(case, scale)
    if layers is not None and "diluent" in kw:
        kw["diluent"] = {n: np.broadcast_to(v, case["T"].shape)[sel] for n, v in kw["diluent"].items()}
    o32 = torch.full((T.size, X.size), float("nan"), dtype=torch.float32, device="cuda") if out32 else None
    o64 = torch.full((T.size, X.size), float("nan"), dtype=torch.float64, device="cuda") if out64 else None
    eng.voigt_sum_axis(lines, X, T, p, 1.0, out_f32=o32, out_f64=o64, **kw)
    torch.cuda.synchronize()
    r32 = o32.double().cpu().numpy() / scale if out32 else None
    r64 = o64.cpu().numpy() if out64 else None
    if own:
        lines.close()
    return r32, r64


_GOT = {}


# ---------------------------------------------------------------------------------------------- a-d. one path at a time
@pytest.mark.parametrize("name", AC.PATH_CASES)
def test_path_vs_oracle(eng, name):
    case = AC.CASES[name]
    want = oracle(name, case)
    r32, r64 = run(eng, case)
    e = pointwise_err(r64, want)
    per_layer = [pointwise_err(r64[k], want[k]) for k in range(want.shape[0])]
    print("linesum_axis_paths %s: %.3g (per layer %s)" % (name, e, " ".join("%.3g" % v for v in per_layer)))
    assert e <= CASE_TOL.get(name, TOL), (name, e)
    # out_f64 is the fp32 sum widened and divided by the power-of-two scale: the same bits
    assert np.array_equal(r64, r32), name
    _GOT[name] = r64


def test_sparse_tiles_are_exact_zeros(eng):
    """d_sparse: the tiles no window reaches are exact zeros between tiles that are not."""
    name = "d_sparse"
    got = _GOT[name] if name in _GOT else run(eng, AC.CASES[name])[1]
    per_tile = [np.any(got[0, t * 1024:(t + 1) * 1024] != 0) for t in range(6)]
    assert per_tile == [True, False, True, True, False, True], per_tile


def test_repeated_points(eng):
    """b_repeats: equal abscissae inside one tile give equal bits; across a tile boundary both meet the oracle (the sums
    regroup: other candidate ranges)."""
    name = "b_repeats"
    case = AC.CASES[name]
    got = _GOT[name] if name in _GOT else run(eng, case)[1]
    X = case["X"]
    same = np.flatnonzero(X[1:] == X[:-1])
    inside = same[same // 1024 == (same + 1) // 1024]
    across = same[same // 1024 != (same + 1) // 1024]
    assert inside.size >= 5 and across.size >= 2 and np.any(inside % 64 == 63)  # one pair astride a row boundary
    assert np.array_equal(got[:, inside], got[:, inside + 1])
    want = oracle(name, case)
    assert np.array_equal(want[:, across], want[:, across + 1])
    assert pointwise_err(got, want) <= TOL


# ------------------------------------------------------------------------------------------------- e. the uniform cases
@pytest.mark.parametrize("name", sorted(AC.UNIFORM_CASES))
def test_uniform_cases_through_the_axis_path(eng, name):
    import torch
    case = AC.UNIFORM_CASES[name]
    base = LC.CASES[name]
    want = oracle("e_" + name, case)
    lines = eng.LineTable(case["tbl"])
    scale = _scale(case)
    _, got = run(eng, case, out32=False, lines=lines)
    grid = eng.Grid(*base["grid"])
    assert np.array_equal(grid.axis(), case["X"])
    o64 = torch.full((case["T"].size, grid.n), float("nan"), dtype=torch.float64, device="cuda")
    eng.voigt_sum(lines, grid, case["T"], case["p"], 1.0, out_f64=o64, omega_wing=case["ow"], omega_wing_hw=case["hw"], scale=scale)
    torch.cuda.synchronize()
    nodal = o64.cpu().numpy()
    lines.close()
    e_axis, e_grid, e_pair = pointwise_err(got, want), pointwise_err(nodal, want), pointwise_err(got, nodal)
    print("linesum_axis_paths uniform %s: axis-vs-oracle %.3g grid-vs-oracle %.3g axis-vs-grid %.3g" % (name, e_axis, e_grid, e_pair))
    assert e_axis <= CASE_TOL.get(name, TOL), (name, e_axis)
    assert e_pair <= AXIS_VS_GRID_CASE_TOL.get(name, AXIS_VS_GRID), (name, e_pair, "axis-vs-oracle %.3g" % e_axis,
                                                                     "grid-vs-oracle %.3g" % e_grid)


# -------------------------------------------------------------------------------------------------------------- f. shapes
_FULL = {}


def _full(eng):
    if "r" not in _FULL:
        _FULL["r"] = run(eng, AC.CASES[AC.SHAPES_CASE])[1]
    return _FULL["r"]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_axis_prefixes(eng, n):
    """X[:n] of b_repeats (ragged last rows and tiles, a one-point axis): against the oracle, and bit-identical to the first n
    points of the full-axis result. DESIGN 4.8: a tile's candidate range is trimmed to the first and last line whose window
    meets the tile, and a candidate's wave is its position in that range. Cutting the axis leaves every whole tile its
    range; in the cut tile the lines that only met dropped points contribute to no kept point, but they could move the
    start of the range, hence the waves, and a regrouped fp32 sum may round differently. On this case every n gives the
    full axis's bits (measured: profiles/linesum_axis_paths_accuracy.txt), so it is asserted."""
    case = AC.CASES[AC.SHAPES_CASE]
    X = case["X"][:n]
    want = AC.oracle(case, X=X)
    r32, r64 = run(eng, case, X=X)
    e = pointwise_err(r64, want)
    same = np.array_equal(r64, _full(eng)[:, :n])
    print("linesum_axis_paths prefix n=%d: %.3g, bit-identical to the full axis: %s" % (n, e, same))
    assert e <= TOL and np.array_equal(r64, r32), (n, e)
    assert same, n


def test_leading_dimension_and_second_sum_through_the_c_abi(eng):
    """rtx_voigt_sum_axis with ld > nx: rows correct and the NaN padding still NaN, for out_f32 only, out_f64 only and both;
    a second sum after the same prologue repeats the bits."""
    import torch
    from radtxfr_amd import _lib
    lib = _lib.load()
    name = "a_band_1000"
    case = AC.CASES[name]
    lines = eng.LineTable(case["tbl"])
    scale = _scale(case)
    r32, r64 = run(eng, case, lines=lines)  # the prologue, and the reference rows
    assert pointwise_err(r64, oracle(name, case)) <= TOL
    nL, nx = case["T"].size, case["X"].size
    ld = nx + 77
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    plan = lines.plan(nL, nx)
    for use32, use64 in ((True, False), (False, True), (True, True), (True, True)):  # the last: a further sum, same bits
        o32 = torch.full((nL, ld), float("nan"), dtype=torch.float32, device="cuda")
        o64 = torch.full((nL, ld), float("nan"), dtype=torch.float64, device="cuda")
        _lib.check(lib.rtx_voigt_sum_axis(plan._h, nL, C.c_void_p(o32.data_ptr() if use32 else 0),
                                          C.c_void_p(o64.data_ptr() if use64 else 0), ld, st))
        torch.cuda.synchronize()
        p32, p64 = o32.double().cpu().numpy(), o64.cpu().numpy()
        assert np.isnan(p32[:, nx:]).all() and np.isnan(p64[:, nx:]).all(), (use32, use64)
        assert np.array_equal(p32[:, :nx] / scale, r32) if use32 else np.isnan(p32).all(), (use32, use64)
        assert np.array_equal(p64[:, :nx], r64) if use64 else np.isnan(p64).all(), (use32, use64)
    lines.close()


def test_layers_one_many_and_alternating(eng):
    """A 2-tile axis with 1 layer, with 64 layers (p from 1e-4 to 1 atm, T from 200 to 300 K, interleaved) and with layers
    alternating between 1 atm and 1e-4 atm: against the oracle, and every layer of the many-layer calls equal to its own
    one-layer call bit for bit (maxhw is per layer; a layer's candidate ranges do not depend on its neighbours)."""
    base = AC.CASES[AC.SHAPES_CASE]
    X = base["X"][:2048]
    k = np.arange(64)
    configs = {
        "one": (np.array([296.0]), np.array([1.0])),
        "alternating": (np.array([296.0, 250.0, 280.0, 220.0, 260.0, 210.0]), np.array([1.0, 1e-4, 1.0, 1e-4, 1.0, 1e-4])),
        "64": (200.0 + 100.0 * ((k * 37) % 64) / 64, np.where(k % 2 == 0, 10.0 ** np.linspace(-2.0, 0.0, 64), 10.0 ** np.linspace(-4.0, -2.5, 64))),
    }
    lines = eng.LineTable(base["tbl"])
    for tag, (T, p) in configs.items():
        case = dict(base, T=T, p=p)
        want = AC.oracle(case, X=X)
        _, got = run(eng, case, X=X, out32=False, lines=lines)
        e = pointwise_err(got, want)
        print("linesum_axis_paths layers %s: %.3g" % (tag, e))
        assert e <= TOL, (tag, e)
        for j in range(T.size):
            _, alone = run(eng, case, X=X, out32=False, lines=lines, layers=slice(j, j + 1))
            assert np.array_equal(alone[0], got[j]), (tag, j)
    lines.close()
