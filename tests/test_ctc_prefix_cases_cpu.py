"""What the fp64 reference says about the candidate lists of tests/ctc_prefix_ref.py, on the CPU: the share of unclear utterances of every
case the GPU tests of the recursion kernel run (tests/test_hip_ctc_prefix_kernel.py), the merges, and the re-entry events -- so that a
change of a generator cannot silently empty those tests.  The figures are the ones the lists were chosen by."""
import pytest

import ctc_beam_ref as br
import ctc_prefix_ref as pr

UNCLEAR = {"peaky_T130_V12_k8_beam16": 0, "peaky_T130_V40_k8_beam8": 0, "peaky_T70_V12_k8_beam16": 0, "peaky_T130_V12_k3_beam2": 0,
           "flat_T48_V40_k8_beam8": 3, "flat_T48_V40_k8_beam1": 0, "flat_T48_V40_k1_beam8": 1, "flat_T48_V6_k3_beam4": 1}


def _events(c):
    ev = [pr.reentry_events(*br.candidates_of(c["ids"][b], c["lp"][b], n), c["beam"]) for b, n in enumerate(c["lengths"])]
    return sum(e[0] for e in ev), sum(e[1] for e in ev)


@pytest.mark.parametrize("name", list(UNCLEAR))
def test_share_of_unclear_utterances(name):
    c = pr.case(name)
    assert sum(c["unclear"]) == UNCLEAR[name] and sum(c["unclear"]) <= 0.1 * len(c["unclear"])
    merges, _ = _events(c)
    if name == "peaky_T130_V12_k8_beam16":
        assert merges >= 600                                              # about 640
        assert all(len(hyps[0][0]) == 130 for hyps, _ in c["ref"])        # the best prefix is the labels themselves: past one wave
    if name == "flat_T48_V6_k3_beam4":
        assert merges >= 200


@pytest.mark.parametrize("V,beam,spread,seed", pr.REENTRY)
def test_reentry_lists_hold_a_reentry_and_are_clear(V, beam, spread, seed):
    c = pr.case(f"reentry_V{V}_beam{beam}_seed{seed}")
    assert c["unclear"] == [False]
    merges, back = _events(c)
    assert back >= 1 and merges > back


def test_grid_and_ragged_lists_are_clear_enough():
    for beam in pr.GRID_BEAMS:
        for k in pr.GRID_KS:
            c = pr.grid_case(beam, k)
            assert sum(c["unclear"]) <= 0.1 * len(c["unclear"]), (beam, k)
            assert max(len(h) for h, _ in c["ref"]) == (beam if k else 1)
    c = pr.ragged_case()
    assert c["lengths"][:5] == [70, 0, 1, 17, 69] and sum(c["unclear"]) <= 0.1 * len(c["unclear"])


def test_a_merge_with_the_parent_always_present_is_no_reentry():
    """beam 2 over labels a = 1, b = 2: "ab" and then "abb" take extensions of parents that never left the beam"""
    import math
    lg = math.log
    ids = [[0, 1, 2]] * 5
    lp = [[lg(0.05), lg(0.9), lg(0.05)], [lg(0.02), lg(0.01), lg(0.97)], [lg(0.98), lg(0.01), lg(0.01)], [lg(0.3), lg(0.3), lg(0.4)],
          [lg(0.3), lg(0.3), lg(0.4)]]
    assert pr.reentry_events(ids, lp, 2) == (2, 0)
    assert br.prefix_beam_ref(ids, lp, beam=2)[0][0][0] == (1, 2, 2)
