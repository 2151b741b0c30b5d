"""CPU: every case of tests/od_hide_cases.py reaches what it names, by the NumPy restatement of the kernel's row masks
(cpu_ref.row_masks) and of what the done-row instantiation does with them (od_hide_cases.restate); the new entry point is
declared, bound and kept out of the table of entries whose last parameter is a stream."""
import os

import numpy as np
import pytest

import od_hide_cases as H
from oracle import cpu_ref

ROWS = H.ROWS


@pytest.fixture(scope="module")
def R():
    return {name: H.restate(c) for name, c in H.CASES.items()}


def _tiles(rs, layer=None):
    return sorted({r["tile"] for r in rs if layer is None or r["layer"] == layer})


def _hole(mask, done):
    """Lines of a bool [lines][ROWS] mask that have a done row between two live rows of theirs."""
    lv = mask & ~done[None, :]
    first = np.where(lv.any(1), np.argmax(lv, 1), ROWS)[:, None]
    last = np.where(lv.any(1), ROWS - 1 - np.argmax(lv[:, ::-1], 1), -1)[:, None]
    r = np.arange(ROWS)[None, :]
    return (mask & done[None, :] & (r > first) & (r < last)).any(1)


def test_tables_are_what_the_cases_say(R):
    """base: layers 0-2 go to the fp32 instantiation, layer 3 to the fp64 one; every kind of work is there; no hot tile."""
    rs = R["none"]
    assert {r["layer"]: r["smally"] for r in rs} == {0: False, 1: False, 2: False, 3: True}
    assert _tiles(rs) == [0, 1, 2]
    for k in (0, 1, 2):
        mine = [r for r in rs if r["layer"] == k]
        for what in ("tile_level", "full", "partial", "entry"):
            assert any(r[what].any() for r in mine), (k, what)
    assert any(r["edge_only"].any() for r in rs if not r["smally"])
    long_band = max(int(r["bd"].sum(1).max()) for r in rs if not r["smally"])
    assert long_band >= 7, long_band
    ys = np.concatenate([r["y"][r["bd"].any(1)] for r in rs if not r["smally"]])
    assert np.any(ys >= 6.0) and np.any((ys >= 1.0) & (ys < 6.0))  # both loops of the band run
    assert not H.done_mask(H.CASES["none"])[:2].any() and H.done_mask(H.CASES["none"])[2].tolist() == [False, False] + [True] * 14
    assert H.CASES["null"]["skip"] is None


@pytest.mark.parametrize("row", [0, 7, 15])
def test_one_live_row(R, row):
    """Row-level members of both passes add into the live row while every other row of its block is done; entries with no
    live row are dropped, others lose rows."""
    rs = [r for r in R["live_%d" % row] if r["tile"] < 2]
    assert _tiles(rs) == [0, 1]
    for r in rs:
        assert r["done"].sum() == ROWS - 1 and not r["done"][row]
    for k in (0, 1, 2):
        mine = [r for r in rs if r["layer"] == k]
        assert any((r["full"] & r["far"][:, row]).any() for r in mine), k
        assert any((r["partial"] & r["far"][:, row]).any() for r in mine), k
        assert any(r["tile_level"].any() for r in mine), k
    dropped = sum(int((~l["entry"]).sum()) + int((~l["edge"]).sum()) for r in rs for l in r["lists"])
    kept = sum(int(l["entry"].sum()) + int(l["edge"].sum()) for r in rs for l in r["lists"])
    assert dropped > 0 and kept > 0, (dropped, kept)
    # the ragged tile has rows 0 and 1 only: wholly done unless the live row is 0
    assert (2 in _tiles(R["live_%d" % row])) == (row == 0)


def test_alternating_rows(R):
    c, rs = H.CASES["alt_rows"], [r for r in R["alt_rows"] if not r["smally"]]
    D = H.done_mask(c)
    for t in (0, 1):
        assert not (D[t].reshape(-1, 2).all(1)).any() and D[t].sum() == ROWS // 2  # no pair, hence no block of four, wholly done
    assert any(_hole(r["bd"], r["done"])[r["entry"]].any() for r in rs), "no band run with a done row inside"
    assert any(_hole(r["pp"], r["done"])[r["entry"]].any() for r in rs), "no near zone with a done row inside"
    assert any((r["bd_trim"].sum(1) < r["bd"].sum(1))[r["entry"]].any() for r in rs), "no band run trimmed"
    assert any(r["smally"] for r in R["alt_rows"]), "the fp64 instantiation is not reached"
    assert any((r["edge_only"] & r["done"][r["edge_row"]]).any() for r in rs) and any((r["edge_only"] & ~r["done"][r["edge_row"]]).any() for r in rs)


def test_alternating_blocks(R):
    c, rs = H.CASES["alt_blocks"], R["alt_blocks"]
    D = H.done_mask(c)
    for t in (0, 1):
        b = D[t].reshape(-1, 4)
        assert np.array_equal(b.all(1), b.any(1)) and b.all(1).sum() == 2
    assert any((r["bd"] & r["done"][None, :]).any(1)[r["entry"] & (r["bd"] & ~r["done"][None, :]).any(1)].any() for r in rs)


def test_prefix_and_suffix_end_inside_a_block(R):
    for name in ("prefix_suffix", "both_ends"):
        c, rs = H.CASES[name], R[name]
        D = H.done_mask(c)
        for t in (0, 1):
            d = np.nonzero(D[t])[0]
            assert d.size and (d[0] == 0 or d[-1] == ROWS - 1)
            edges = np.nonzero(np.diff(D[t].astype(int)))[0] + 1
            assert all(e % 4 != 0 for e in edges), edges
    rs = R["prefix_suffix"]
    lo_trim = any((r["bd"] & ~r["bd_trim"] & (np.arange(ROWS)[None, :] < 6)).any() for r in rs if r["tile"] == 0)
    hi_trim = any((r["bd"] & ~r["bd_trim"] & (np.arange(ROWS)[None, :] >= 9)).any() for r in rs if r["tile"] == 1)
    assert lo_trim and hi_trim
    assert any(e % 2 for t in (0, 1) for e in np.nonzero(np.diff(H.done_mask(H.CASES["prefix_suffix"])[t].astype(int)))[0] + 1)


def test_whole_tile_beside_a_live_one(R):
    assert _tiles(R["whole_tile"]) == [1]
    assert H.done_mask(H.CASES["whole_tile"])[[0, 2]].all()


def test_ragged_tile(R):
    for name, live_rows in (("ragged", [0]), ("ragged_live", [1])):
        c, rs = H.CASES[name], [r for r in R[name] if r["tile"] == 2]
        assert rs and all(np.nonzero(~r["done"])[0].tolist() == live_rows for r in rs)
        for r in rs:
            work = r["far"] | r["pp"] | r["ed"] | r["bd"]
            assert work[:, live_rows[0]].any() and not work[:, 2:].any()  # nothing reaches the rows past the grid's end
    # the flags past the end: set in one case, clear in the other
    assert H.CASES["ragged"]["skip"][2 * ROWS + 5] and not H.CASES["ragged_live"]["skip"][2 * ROWS + 5]


def test_layer_range_and_shard(R):
    c = H.CASES["layer_range"]
    assert (c["k_lo"], c["k_hi"], c["layers"]) == (1, 3, 4) and sorted({r["layer"] for r in R["layer_range"]}) == [1, 2]
    c = H.CASES["smally_alone"]
    assert all(r["smally"] for r in R["smally_alone"]) and R["smally_alone"]
    c = H.CASES["shard"]
    assert c["shard"] == (H.TILE, H.N - H.TILE) and c["shard"][0] % H.TILE == 0
    assert np.asarray(H.case_table(c)["nu"]).size < np.asarray(H.table("base")[0]["nu"]).size
    assert _tiles(R["shard"]) == [0, 1] and any(r["done"][:2].tolist() == [False, True] for r in R["shard"] if r["tile"] == 1)


def test_dense_table_overflows_both_lists_with_dead_entries_first(R):
    """In one wave both lists reach their capacity at least once, and at the first time each does, it holds fewer entries
    than it counts. The candidates stay under the hot-tile cut (asserted by restate)."""
    hits = []
    for r in R["dense"]:
        for w, l in enumerate(r["lists"]):
            e, g = H.overflow(l["edge"], cpu_ref.LS_EDGE_CAP), H.overflow(l["entry"], cpu_ref.LS_ENT_CAP)
            if e[0] >= 1 and g[0] >= 1 and e[1] and g[1]:
                hits.append((r["layer"], r["tile"], w, e[0], g[0]))
    print("dense: (layer, tile, wave, edge-list drains at capacity, entry-list drains at capacity):", hits)
    assert hits
    assert any(not r["smally"] for r in R["dense"])
    # the base table never fills a list: there the two counts cannot be told apart
    for r in R["alt_rows"]:
        for l in r["lists"]:
            assert l["edge"].size < cpu_ref.LS_EDGE_CAP and l["entry"].size < cpu_ref.LS_ENT_CAP


def test_entry_is_declared_and_bound():
    import stream_cases as S
    from radtxfr_amd import _lib
    assert "rtx_voigt_sum_rows" in _lib.PROTOTYPES
    res, args = _lib.PROTOTYPES["rtx_voigt_sum_rows"]
    assert len(args) == 10 and args[-1] is __import__("ctypes").c_uint
    text = S.header_text()
    assert "int rtx_voigt_sum_rows(const rtx_prep* prep, const rtx_grid* grid, int n_layers, float* out_f32, int64_t ld, int k_lo," in text
    assert "rtx_voigt_sum_rows" not in S.stream_entries()  # flags come after the stream: rtx_continuum_add_d's form
    with open(os.path.join(S.ROOT, "INTEGRATION.md")) as f:
        assert "rtx_voigt_sum_rows" in f.read()
