"""Every path of the Voigt line-sum (rtx_voigt_sum: voigt_nodal_kernel<false|true>, voigt_nodal_parts_kernel<false|true>,
split_combine_kernel, and the point-by-point cross-check voigt_scatter_kernel<false|true>) against the fp64 oracle, point
by point and layer by layer.

a-d. The cases of tests/linesum_cases.py, one path at a time: tile-level members 511 / 512 / 513 points outside a tile,
     full and partial row members, the near zone on the first / middle / last row, |x| + y = 15 on a lane (the fp64
     recheck), band rows with y >= 6, 1 <= y < 6 on both sides of |z| = 8, y < 1 on inner (fp64 Weideman) and outer
     (fp32 asymK_re<12>) rows at 1000 and 6000 cm^-1, the upper standard atmosphere down to y ~ 1e-6; windows narrower
     than a row, both edges in one row, edges on a row boundary, a window over the whole grid, centres left / right /
     1e8 points outside the grid, OmegaWing and OmegaWingHW each setting windows; a dense comb that overflows the
     edge-only and entry lists within one wave round; hot tiles cut into parts on a plain and a SMALLY layer of one call.
     tests/test_host.py's census proves on the CPU that each case reaches the paths it names.
d.   Hot tiles with out_f32 only, out_f64 only and both, scale != 1, and a second rtx_voigt_sum after one prologue.
e.   Layers alternating between having y < 1 lines and not (each instantiation returns at once on the other's layers),
     one layer, and the 4096 layers the plan allows on a small grid.
f.   n in {2, 63, 64, 65, 1023, 1024, 1025, 2049} and a one-point shard (ragged last row and tile), a shard that does not
     start on a tile boundary, and rtx_voigt_sum through the C ABI with ld > n (the NaN padding must stay NaN).
g.   Cases a-d again with RADTXFR_VOIGT_KERNEL=scatter in one child process (the choice is cached per process): against
     the oracle at the same bounds and against the nodal results at SCATTER_VS_NODAL.

Metric, per layer: err_i = |got_i - want_i| / max(|want_i|, F max_{|j - i| <= 1024} |want_j|, F32_FLOOR), at most TOL.
The floor is local, not global: a far wing, a weak band or a thin layer is held to 1e-5 of its own neighbourhood, not
of the strongest layer's peak (conftest.rel_err). It is not zero either: the reference's Weideman-24 is not the Faddeeva
function in far Doppler wings (y = 1e-7, |x| = 5.5 ... 10: 1.2-3.3e-11 of w(0), 0.5-2 % of the value there), and the
kernel's outer-row series follows the true function; F = 1e-5 holds that with a margin of 3x. Points where the oracle is
exactly 0 (outside every window) must be exactly 0. F32_FLOOR: values fp32 cannot hold are compared absolutely.

No case needs a bound looser than TOL against the oracle (CASE_TOL is empty). Worst measured: 3.2e-6 (a_upper_atmosphere),
which is the reference's own error -- its Weideman-24 is 4.1e-11 of w(0) off the Faddeeva function at |x| = 5.5 ... 10,
y ~ 1e-6, against the floor of 1e-5 of the local peak -- then 6.7e-7 (a_row_level). One bound of the scatter-vs-nodal
comparison is looser than SCATTER_VS_NODAL: a_upper_atmosphere at 1e-5 (SCATTER_CASE_TOL, measured 3.2e-6), for the same
cause: the scatter kernel evaluates every band lane of a y < 1 line in fp64 Weideman-24, as the reference does (it meets
the oracle there to 4.0e-7), while the nodal kernel's outer rows (every lane |x| >= 5.5) take the asymptotic series
asymK_re<12>, which follows the true function."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from oracle import cpu_ref as ref

import linesum_cases as LC
from linesum_metric import F, F32_FLOOR, HALO, TOL, _local_max, pointwise_err  # noqa: F401 (the metric of the module docstring)

pytestmark = pytest.mark.gpu

CASE_TOL = {}  # case -> bound looser than TOL (none needed)
SCATTER_VS_NODAL = 2e-6
SCATTER_CASE_TOL = {"a_upper_atmosphere": 1e-5}  # the reference's Weideman-24 in far Doppler wings (module docstring)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    from radtxfr_amd import _lib, engine
    _lib.load()
    return engine


def _engine_grid(eng, g):
    xmin, xmax, n_total, offset, n = g
    return eng.Grid(xmin, xmax, n_total, offset, n)


_ORACLE = {}


def oracle(name, case, g=None):
    """[layers][points] of absorptionCoefficient_Voigt on the case's (or g's) shard axis; cached per case."""
    g = g or case["grid"]
    key = (name, g)
    if key not in _ORACLE:
        from radtxfr_amd import _lib
        gr = _lib.make_grid(g[0], g[1], g[2], g[3], g[4])
        ig = np.arange(gr.offset, gr.offset + gr.n, dtype=np.float64)
        X = ig * gr.step + gr.xmin
        if gr.n and gr.offset + gr.n == gr.n_total:
            X[-1] = gr.xmax
        _ORACLE[key] = np.stack([ref.absorptionCoefficient_Voigt(case["tbl"], T=float(T), p=float(p), OmegaGrid=X,
                                                                 OmegaWing=case["ow"], OmegaWingHW=case["hw"])[1]
                                 for T, p in zip(case["T"], case["p"])])
    return _ORACLE[key]


def run(eng, case, g=None, out32=True, out64=True, scale=1.0, lines=None):
    import torch
    own = lines is None
    lines = lines or eng.LineTable(case["tbl"])
    grid = _engine_grid(eng, g or case["grid"])
    nL = case["T"].size
    o32 = torch.full((nL, grid.n), float("nan"), dtype=torch.float32, device="cuda") if out32 else None
    o64 = torch.full((nL, grid.n), float("nan"), dtype=torch.float64, device="cuda") if out64 else None
    eng.voigt_sum(lines, grid, case["T"], case["p"], 1.0, out_f32=o32, out_f64=o64, omega_wing=case["ow"],
                  omega_wing_hw=case["hw"], scale=scale)
    torch.cuda.synchronize()
    r32 = o32.double().cpu().numpy() if out32 else None
    r64 = o64.cpu().numpy() if out64 else None
    if own:
        lines.close()
    return r32, r64


# ---------------------------------------------------------------------------------------------- a-d. one path at a time
_NODAL = {}


@pytest.mark.parametrize("name", LC.PATH_CASES)
def test_path_vs_oracle(eng, name):
    case = LC.CASES[name]
    want = oracle(name, case)
    r32, r64 = run(eng, case)
    tol = CASE_TOL.get(name, TOL)
    e32, e64 = pointwise_err(r32, want), pointwise_err(r64, want)
    print("linesum_paths %s: f32 %.3g f64 %.3g" % (name, e32, e64))
    assert e32 <= tol and e64 <= tol, (name, e32, e64)
    # out_f64 is the fp32 sum widened (scale 1): the same values, except on hot tiles, whose parts split_combine_kernel
    # adds in fp64 there (d: test_hot_tile_outputs_scale_and_second_sum)
    if name != "d_hot":
        assert np.array_equal(r64.astype(np.float32), r32.astype(np.float32)), name
    _NODAL[name] = r64


def test_far_centre_clamp_keeps_x(eng):
    """Regression: a centre more than 1e8 points outside the grid (the prologue clamps its local index there) with a window
    reaching in. The record's x offset c now belongs to the clamped index, so x = u a + c is the line's own; it was that
    of a line at the clamp (a wing 1.2e8 points out 44 % too large). Each of the far lines alone against the oracle."""
    base = LC.CASES["b_far_centre"]
    for r in range(base["tbl"]["nu"].size):
        case = dict(base, tbl={k: v[r:r + 1] for k, v in base["tbl"].items()})
        want = oracle("b_far_centre_%d" % r, case)
        r32, r64 = run(eng, case)
        assert want.min() > 0.0
        assert pointwise_err(r64, want) <= TOL, (r, pointwise_err(r64, want))


# ------------------------------------------------------------------------------------------------------- d. hot tiles
def test_hot_tile_outputs_scale_and_second_sum(eng):
    """Hot tiles (plain and SMALLY layer) with out_f32 only, out_f64 only, both, scale != 1, and a second rtx_voigt_sum
    after one prologue: split_combine_kernel writes what was asked, in part order, every time."""
    import torch
    from radtxfr_amd import _lib
    lib = _lib.load()
    case = LC.CASES["d_hot"]
    want = oracle("d_hot", case)
    lines = eng.LineTable(case["tbl"])
    grid = _engine_grid(eng, case["grid"])
    both32, both64 = run(eng, case, lines=lines)
    assert lib.rtx_prep_split_bound(lines.plan(case["T"].size, grid.n)._h) > 0
    only32, _ = run(eng, case, out64=False, lines=lines)
    _, only64 = run(eng, case, out32=False, lines=lines)
    assert np.array_equal(only32, both32) and np.array_equal(only64, both64)
    assert pointwise_err(only64, want) <= TOL and pointwise_err(only32, want) <= TOL
    S = 2.5e3
    s32, s64 = run(eng, case, scale=S, lines=lines)
    assert pointwise_err(s32 / S, want) <= TOL and pointwise_err(s64, want) <= TOL
    # out_f64 = out_f32 / scale up to fp32 rounding (the parts are added in fp64 there, in fp32 in out_f32)
    assert np.all(np.abs(s64 - s32 / S) <= 4e-7 * np.abs(s64)), float(np.max(np.abs(s64 - s32 / S) / np.abs(s64)))
    assert np.all(np.abs(both64 - both32) <= 4e-7 * np.abs(both64))
    # a second sum after the same prologue (the last run: scale S): the work list is rebuilt, the bits repeat
    nL = case["T"].size
    o32 = torch.full((nL, grid.n), float("nan"), dtype=torch.float32, device="cuda")
    o64 = torch.full((nL, grid.n), float("nan"), dtype=torch.float64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.rtx_voigt_sum(lines.plan(nL, grid.n)._h, grid.byref(), nL, C.c_void_p(o32.data_ptr()),
                                 C.c_void_p(o64.data_ptr()), grid.n, st))
    torch.cuda.synchronize()
    assert np.array_equal(o32.double().cpu().numpy(), s32) and np.array_equal(o64.cpu().numpy(), s64)
    lines.close()


# ---------------------------------------------------------------------------------------------------------- e. layers
def _few_lines():
    return LC.table([999.5, 1000.02, 1000.4, 1001.0, 1002.1], [0.07, 0.03, 0.11, 0.05, 0.08])


def test_layers_alternating_one_and_many(eng):
    """Plain and SMALLY layers alternating in one call (y < 1 at p <= 0.01 atm), a single layer of each kind, and the
    4096 layers the plan allows on a 300-point grid (p from 1e-6 to 1 atm, T from 200 to 300 K, interleaved)."""
    g = LC.grid(1000.0, 1e-3, 1100)
    tbl = _few_lines()
    configs = {
        "alternating": (np.array([296.0, 250.0, 280.0, 220.0, 260.0, 210.0]), np.array([1.0, 0.003, 0.3, 0.001, 0.05, 5e-4])),
        "one_plain": (np.array([296.0]), np.array([1.0])),
        "one_smally": (np.array([230.0]), np.array([0.002])),
    }
    for tag, (T, p) in configs.items():
        case = LC._case(tbl, g, T, p)
        want = oracle("e_" + tag, case)
        r32, r64 = run(eng, case)
        e = pointwise_err(r64, want)
        print("linesum_paths e_%s: %.3g" % (tag, e))
        assert e <= TOL and pointwise_err(r32, want) <= TOL, (tag, e)
    nL = 4096
    k = np.arange(nL)
    p = np.where(k % 2 == 0, 10.0 ** np.linspace(-2.0, 0.0, nL), 10.0 ** np.linspace(-6.0, -2.5, nL))
    T = 200.0 + 100.0 * ((k * 37) % nL) / nL
    case = LC._case(tbl, LC.grid(1000.3, 1e-3, 300), T, p)
    want = oracle("e_4096", case)
    r32, r64 = run(eng, case)
    e = pointwise_err(r64, want)
    print("linesum_paths e_4096: %.3g" % e)
    assert e <= TOL, e


# ------------------------------------------------------------------------------------------------------ f. grid shapes
@pytest.mark.parametrize("n", [2, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_grid_sizes(eng, n):
    """Ragged last rows and tiles, down to the 2-point grid the ABI accepts."""
    case = LC._case(_few_lines(), LC.grid(1000.0, 2e-3 if n > 1000 else 1e-2, n), (296.0, 230.0), (1.0, 0.002))
    want = oracle("f_%d" % n, case)
    r32, r64 = run(eng, case)
    assert pointwise_err(r64, want) <= TOL and pointwise_err(r32, want) <= TOL, n


def test_one_point_and_unaligned_shards(eng):
    """A one-point shard; shards that start off a tile boundary (the sums regroup: against the oracle, at TOL)."""
    from radtxfr_amd import _lib
    tp = int(_lib.load().rtx_voigt_tile_points())
    for name in ("a_row_level", "c_comb", "d_hot"):
        case = LC.CASES[name]
        xmin, xmax, n_total = case["grid"][:3]
        for off, n in ((37, 1), (tp // 2 + 5, 3000), (tp + 333, n_total - tp - 333 - 17)):
            g = (xmin, xmax, n_total, off, n)
            want = oracle(name, case, g)
            r32, r64 = run(eng, case, g=g)
            e = pointwise_err(r64, want)
            assert e <= CASE_TOL.get(name, TOL) and pointwise_err(r32, want) <= CASE_TOL.get(name, TOL), (name, off, n, e)


def test_leading_dimension_through_the_c_abi(eng):
    """rtx_voigt_sum with ld > n (plain and SMALLY layers, hot tiles included): rows correct, padding still NaN."""
    import torch
    from radtxfr_amd import _lib
    lib = _lib.load()
    for name in ("a_band_1000", "d_hot"):
        case = LC.CASES[name]
        want = oracle(name, case)
        lines = eng.LineTable(case["tbl"])
        grid = _engine_grid(eng, case["grid"])
        r32, r64 = run(eng, case, lines=lines)  # the prologue (and the reference rows)
        nL, n = case["T"].size, grid.n
        ld = n + 77
        o32 = torch.full((nL, ld), float("nan"), dtype=torch.float32, device="cuda")
        o64 = torch.full((nL, ld), float("nan"), dtype=torch.float64, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.rtx_voigt_sum(lines.plan(nL, n)._h, grid.byref(), nL, C.c_void_p(o32.data_ptr()),
                                     C.c_void_p(o64.data_ptr()), ld, st))
        torch.cuda.synchronize()
        p32, p64 = o32.double().cpu().numpy(), o64.cpu().numpy()
        assert np.isnan(p32[:, n:]).all() and np.isnan(p64[:, n:]).all(), name
        assert np.array_equal(p32[:, :n], r32) and np.array_equal(p64[:, :n], r64), name
        assert pointwise_err(p64[:, :n], want) <= TOL, name
        lines.close()


# ------------------------------------------------------------------------------------------- g. the cross-check kernel
_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import linesum_cases as LC
from radtxfr_amd import _lib, engine
_lib.load()
res = {}
for name in LC.PATH_CASES:
    c = LC.CASES[name]
    g = engine.Grid(*c['grid'])
    nL = c['T'].size
    o64 = torch.full((nL, g.n), float('nan'), dtype=torch.float64, device='cuda')
    lines = engine.LineTable(c['tbl'])
    engine.voigt_sum(lines, g, c['T'], c['p'], 1.0, out_f64=o64, omega_wing=c['ow'], omega_wing_hw=c['hw'])
    torch.cuda.synchronize()
    res[name] = o64.cpu().numpy()
    lines.close()
np.savez(sys.argv[2], **res)
"""


def test_scatter_cross_check(eng):
    """Cases a-d with RADTXFR_VOIGT_KERNEL=scatter (every row point by point, the separate fp64 pass for y < 1): against
    the oracle at the same bounds, and against the nodal kernel at SCATTER_VS_NODAL."""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "scatter.npz")
        env = dict(os.environ, RADTXFR_VOIGT_KERNEL="scatter")
        subprocess.run([sys.executable, "-c", _CHILD, ROOT, out], check=True, env=env, timeout=600)
        got = dict(np.load(out))
    for name in LC.PATH_CASES:
        case = LC.CASES[name]
        want = oracle(name, case)
        e = pointwise_err(got[name], want)
        print("linesum_paths scatter %s: %.3g" % (name, e))
        assert e <= CASE_TOL.get(name, TOL), (name, e)
        nodal = _NODAL.get(name)
        if nodal is None:
            nodal = run(eng, case, out32=False)[1]
        e = pointwise_err(got[name], nodal)
        print("linesum_paths scatter-vs-nodal %s: %.3g" % (name, e))
        assert e <= SCATTER_CASE_TOL.get(name, SCATTER_VS_NODAL), (name, e)
