"""The fp64 prefix beam search of tests/ctc_beam_ref.py against brute force over every path: V = 4, Te = 6, beam 64, k = 3 (every label
is a candidate).  Its best prefix is the labeling of the largest total probability and its score that probability; no score exceeds
the exact log-likelihood of its labeling (a pruned search can only lose alignments); topk64 keeps its total order.  No GPU."""
import math

import pytest
import torch

import ctc_beam_ref as br


def _frames(seed, T=6, V=4, spread=2.0):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(T, V, generator=g, dtype=torch.float64) * spread, dim=1).tolist()


@pytest.mark.parametrize("seed", range(8))
def test_reference_equals_brute_force(seed):
    lp = _frames(seed)
    cands = [br.full_candidates(row) for row in lp]
    hyps, _ = br.prefix_beam_ref([c[0] for c in cands], [c[1] for c in cands], beam=64, nbest=4)
    exact = br.brute_force(lp)
    assert abs(br.lae(*([br.NEG] + [0.0])) - 0.0) < 1e-15
    total = -math.inf
    for s in exact.values():
        total = br.lae(total, s)
    assert abs(total) < 1e-9                                   # the labelings partition the paths
    best = max(exact, key=lambda l: exact[l])
    assert hyps[0][0] == best and abs(hyps[0][1] - exact[best]) < 1e-9, (hyps[0], best, exact[best])
    assert len({l for l, _ in hyps}) == len(hyps)
    for (l, s), (_, s2) in zip(hyps, hyps[1:]):
        assert s >= s2
    for l, s in hyps:
        assert s <= exact[l] + 1e-9, (l, s, exact[l])


def test_reference_with_pruned_candidates_stays_below_the_exact_likelihood():
    lp = _frames(11)
    cands = [br.full_candidates(row) for row in lp]
    ids, lps = [c[0][:3] for c in cands], [c[1][:3] for c in cands]      # the blank and the best two labels of each frame
    hyps, _ = br.prefix_beam_ref(ids, lps, beam=4, nbest=4)
    exact = br.brute_force(lp)
    assert 1 <= len(hyps) <= 4
    for l, s in hyps:
        assert s <= exact[l] + 1e-9


def test_missing_candidates_and_no_frames():
    hyps, margin = br.prefix_beam_ref([], [], beam=4)
    assert hyps == [((), 0.0)] and margin == math.inf
    # one label only, then a frame with no candidate but the blank
    hyps, _ = br.prefix_beam_ref([[0, 2, -1], [0, -1, -1]], [[math.log(0.25), math.log(0.75), br.NEG], [0.0, br.NEG, br.NEG]], beam=4)
    assert [l for l, _ in hyps] == [(2,), ()] and abs(hyps[0][1] - math.log(0.75)) < 1e-12


def test_topk64_total_order_and_fill():
    z = torch.tensor([[1.0, 3.0, 3.0, 0.5, 3.0], [0.0, 0.0, 0.0, 0.0, 0.0]], dtype=torch.float64)
    ids, lprob, lse, vals = br.topk64(z, 3)
    assert ids.tolist() == [[1, 2, 4], [0, 1, 2]]
    ids, lprob, _, _ = br.topk64(z, 8, keep=1)
    assert ids[0].tolist() == [1, 2, 4, 0, 3, -1, -1, -1, -1] and lprob[0, 5:].tolist() == [br.NEG] * 4
    assert torch.allclose(lprob[0, 0], z[0, 1] - lse[0])
    assert br.unclear_rows(z, 2, None, 1e-4).tolist() == [True, True]
    z2 = torch.tensor([[5.0, 1.0, 3.0, 2.0]], dtype=torch.float64)
    assert br.unclear_rows(z2, 2, None, 1e-4).tolist() == [False]
    ok = br.check_topk(z2, torch.tensor([[0, 2]]), torch.tensor([[5.0, 3.0]]) - torch.logsumexp(z2, 1), torch.logsumexp(z2, 1), 2, None, 1e-6)
    assert ok.tolist() == [False]
    with pytest.raises(AssertionError):
        br.check_topk(z2, torch.tensor([[2, 0]]), torch.tensor([[3.0, 5.0]]) - torch.logsumexp(z2, 1), torch.logsumexp(z2, 1), 2, None, 1e-6)


def test_topk_seeds_leave_at_most_one_percent_of_rows_unclear():
    """the cap of tests/test_hip_ctc_topk.py, checked before any GPU run with e taken as 1e-4 (the measured e is smaller)"""
    for M, K, N in br.TOPK_SHAPES + br.TOPK_SPLIT_SHAPES:
        for dtype in (torch.float32, torch.bfloat16):
            for with_bias in (False, True):
                if (M, K, N) in br.TOPK_SPLIT_SHAPES and not (dtype == torch.bfloat16 and with_bias):
                    continue
                z = br.topk_operands(M, K, N, dtype, with_bias)[3]
                for k in (1, 8):
                    for keep in (None, 0, N - 1):
                        u = int(br.unclear_rows(z, k, keep, 1e-4).sum())
                        assert u <= 0.01 * M, (M, K, N, dtype, with_bias, k, keep, u)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_beam_cases_leave_at_most_ten_percent_of_utterances_unclear(dtype):
    """the cap of tests/test_hip_ctc_beam.py from fp64 log-probabilities and the reference alone: an utterance whose smallest
    selection-boundary / final-ranking margin is <= twice the score bound is unclear"""
    _, _, L, lp = br.beam_operands(dtype)
    unclear = 0
    for b, n in enumerate(L.tolist()):
        ids, val, _, _ = br.topk64(lp[b, :n], 8, keep=0)
        hyps, margin = br.prefix_beam_ref(ids.tolist(), val.tolist(), beam=8, nbest=4)
        unclear += margin <= 2 * br.beam_bound(n, hyps[0][1])
    print(f"{dtype}: {unclear} of {len(L)} utterances unclear")
    assert unclear <= 0.1 * len(L)
