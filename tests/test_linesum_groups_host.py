"""Host side of tests/test_gpu_linesum_groups.py: every case of tests/linesum_group_cases.py reaches the decision it names.
cpu_ref.row_masks restates the kernel's classification and linesum_group_cases.merge_rule its rule; no GPU."""
import numpy as np
import pytest

from oracle import cpu_ref

import linesum_group_cases as GC


def test_merge_rule_is_the_group_count_comparison():
    """ceil((nF + nP) / 8) < ceil(nF / 8) + ceil(nP / 8), spelled out over every pair a round of 64 can hold."""
    for nF in range(65):
        for nP in range(65 - nF):
            apart = (nF + 7) // 8 + (nP + 7) // 8
            together = (nF + nP + 7) // 8
            assert GC.merge_rule(nF, nP) == (together < apart), (nF, nP)
            assert together <= apart
    # (3, 6): 9 members make two groups together and two apart, so the rule leaves them apart; (3, 12) is the merged case
    # with a ragged last group (15 members in two groups instead of three)
    named = {(1, 7): True, (1, 8): False, (9, 7): True, (7, 2): False, (3, 6): False, (3, 12): True, (5, 0): False, (0, 5): False}
    for (nF, nP), want in named.items():
        assert GC.merge_rule(nF, nP) == want, (nF, nP)
    assert -(-(9 + 7) // 8) == 2 and -(-(1 + 7) // 8) == 1 and (3 + 12) % 8 != 0  # two groups / one full group / ragged


@pytest.mark.parametrize("name", GC.NAMES)
def test_case_reaches_its_decision(name):
    case = GC.CASES[name]
    got = GC.round_census(case)
    assert set(case["expect"]) <= set(got), (name, sorted(got))
    for key, (nT, nF, nP, merged) in got.items():
        if key in case["expect"]:
            assert (nF, nP, merged) == case["expect"][key], (name, key, (nT, nF, nP, merged))
            assert nT == case["tile_members"], (name, key, nT)
        else:
            assert (nT, nF, nP) == (0, 0, 0), (name, key, (nT, nF, nP))
    assert not GC.smally(case), name  # the plain instantiation, the one the benchmark runs


def test_cases_cover_the_named_decisions():
    triples = {v for c in GC.CASES.values() for v in c["expect"].values()}
    for nF, nP in ((1, 7), (1, 8), (9, 7), (7, 2), (3, 6), (3, 12), (5, 0), (0, 5)):
        assert (nF, nP, GC.merge_rule(nF, nP)) in triples
    two = GC.CASES["g_two_rounds"]["expect"]
    assert two[(0, 0)][2] and not two[(0, 1)][2]
    assert GC.CASES["g_tile_level"]["tile_members"] > 0 and GC.CASES["g_tile_level"]["ow"] == 3.0
    merged = [GC.CASES[n]["expect"][(0, 0)][2] for n in GC.SHARD_CASES]
    assert sorted(merged) == [False, True]


@pytest.mark.parametrize("name", GC.SHARD_CASES)
def test_shard_table_is_a_proper_subset_with_the_same_candidates(name):
    """The one-tile shard's table drops lines, and the tile's candidates on it are those of the full run, in the same order
    (same waves, same rounds, same decision)."""
    case = GC.CASES[name]
    g, sub = GC.shard_of(case)
    assert 0 < sub["nu"].size < case["tbl"]["nu"].size
    assert g[3] == GC.IA and g[3] % GC.TILE == 0 and g[4] == GC.TILE
    got = GC.round_census(dict(case, tbl=sub, grid=g), tile=0)
    assert got == GC.round_census(case), (got, GC.round_census(case))


def test_layout_cases_reach_their_class():
    for name, case in GC.LAYOUT_CASES.items():
        if case["classes"] is None:
            C = cpu_ref.linesum_census(case["tbl"], case["grid"], case["T"], case["p"], case["ow"], case["hw"])
            assert C["hot_plain"] > 0 and C["hot_smally"] == 0 and C["plain_layer"] == 1, (name, C)
            assert case["T"].size == 1 and case["grid"][4] == 6 * GC.TILE
            continue
        got = GC.round_census(case, case["tile"])
        assert got == {(0, 0): case["classes"] + (False,), (1, 0): (0, 0, 0, False)}, (name, got)
        # every far row of the line in that tile, and a value of its own on each: the oracle's row means differ
        want = cpu_ref.absorptionCoefficient_Voigt(case["tbl"], T=296.0, p=1.0, OmegaGrid=np.linspace(*case["grid"][:3]),
                                                   OmegaWing=case["ow"], OmegaWingHW=case["hw"])[1]
        rows = want[case["tile"] * GC.TILE:(case["tile"] + 1) * GC.TILE].reshape(cpu_ref.LS_ROWS, 64).mean(1)
        assert np.all(np.abs(np.diff(rows)) > 0.02 * rows[1:]), (name, rows)
