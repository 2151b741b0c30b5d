"""The row-level groups of the nodal line-sum kernel (rtx_voigt_scatter.hip: nodal_tile) and its final sum over the member
slots, against the fp64 oracle.

1. The cases of tests/linesum_group_cases.py: a chosen (nF, nP) of full and partial members in one wave's round, so that
   the rule that serves the full members through the partial pass is taken both ways -- one full group, two groups, a
   ragged last group, one class alone, two rounds that decide differently, tile-level members beside them. Every point
   within TOL of the oracle in the metric of tests/test_gpu_linesum_paths.py. tests/test_linesum_groups_host.py proves on
   the CPU that each case reaches the decision it names.
2. Shard identity: a merged and an unmerged case on the full grid with the full table, and again as the one-tile shard
   with the contiguous part of the table that reaches it: array_equal (the decision depends on the wave's own candidates
   of the round alone).
3. The layout of the final sums: one line alone as a full member, one alone as a tile-level member -- each tile row has a
   value of its own, so a row sum that lands in another row's slot shows -- row by row against the oracle; and the
   hot-tile parts path on one layer.

Measured on an MI355X (each test prints its figure): the g_nF_nP cases 1.1e-6 each, merged or not, g_two_rounds 9.0e-7,
g_tile_level 4.3e-7; full_alone 4.4e-7 on its worst row (row 10), tile_alone 4.4e-7 (row 9), hot_parts 2.2e-7. The kernel
before the merged pass and the register sums gives the same figures to three digits on every case."""
import numpy as np
import pytest

import linesum_group_cases as GC
import test_gpu_linesum_paths as LP

pytestmark = pytest.mark.gpu

TOL = LP.TOL  # 1e-5, the bar of tests/test_gpu_linesum_paths.py


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    from radtxfr_amd import _lib, engine
    _lib.load()
    return engine


_FULL = {}  # case name -> (r32, r64) on the full grid with the full table, computed once


def _full_run(eng, name):
    if name not in _FULL:
        _FULL[name] = LP.run(eng, GC.CASES[name])
    return _FULL[name]


@pytest.mark.parametrize("name", GC.NAMES)
def test_group_case_vs_oracle(eng, name):
    case = GC.CASES[name]
    want = LP.oracle("groups_" + name, case)
    r32, r64 = _full_run(eng, name)
    e32, e64 = LP.pointwise_err(r32, want), LP.pointwise_err(r64, want)
    print("linesum_groups %s %s: f32 %.3g f64 %.3g" % (name, case["expect"], e32, e64))
    assert e32 <= TOL and e64 <= TOL, (name, e32, e64)
    assert np.array_equal(r64.astype(np.float32), r32.astype(np.float32)), name


@pytest.mark.parametrize("name", GC.SHARD_CASES)
def test_shard_with_table_subset_is_bit_identical(eng, name):
    case = GC.CASES[name]
    g, sub = GC.shard_of(case)
    f32, f64 = _full_run(eng, name)
    s32, s64 = LP.run(eng, dict(case, tbl=sub), g=g)
    cut = slice(g[3], g[3] + g[4])
    assert s64.shape == f64[:, cut].shape and np.all(f64[:, cut] > 0.0)
    assert np.array_equal(s32, f32[:, cut]) and np.array_equal(s64, f64[:, cut]), (name, float(np.max(np.abs(s64 - f64[:, cut]) / f64[:, cut])))


def _err_rows(got, want, tile):
    """The metric of LP.pointwise_err, kept per point, as [rows of the tile][64]."""
    want = np.asarray(want, dtype=np.float64)
    den = np.maximum(np.maximum(np.abs(want), LP.F * LP._local_max(want)), LP.F32_FLOOR)
    e = np.abs(np.asarray(got, dtype=np.float64) - want) / den
    return e[0, tile * GC.TILE:(tile + 1) * GC.TILE].reshape(-1, 64)


@pytest.mark.parametrize("name", ["full_alone", "tile_alone"])
def test_one_member_row_by_row(eng, name):
    case = GC.LAYOUT_CASES[name]
    want = LP.oracle("groups_layout_" + name, case)
    r32, r64 = LP.run(eng, case)
    rows = _err_rows(r64, want, case["tile"]).max(1)
    print("linesum_groups %s: worst row %d: %.3g; whole grid %.3g" % (name, int(np.argmax(rows)), rows.max(), LP.pointwise_err(r64, want)))
    assert np.all(want[0, case["tile"] * GC.TILE:(case["tile"] + 1) * GC.TILE] > 0.0)
    for r, e in enumerate(rows):
        assert e <= TOL, (name, "row", r, e)
    assert LP.pointwise_err(r64, want) <= TOL and LP.pointwise_err(r32, want) <= TOL, name


def test_hot_tile_parts_one_layer(eng):
    case = GC.LAYOUT_CASES["hot_parts"]
    want = LP.oracle("groups_layout_hot_parts", case)
    r32, r64 = LP.run(eng, case)
    e32, e64 = LP.pointwise_err(r32, want), LP.pointwise_err(r64, want)
    print("linesum_groups hot_parts: f32 %.3g f64 %.3g" % (e32, e64))
    assert e32 <= TOL and e64 <= TOL, (e32, e64)
