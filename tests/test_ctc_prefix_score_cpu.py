"""CTC prefix scores inside the attention beam, on the CPU: the fp64 restatement (tests/ctc_prefix_score_ref.py) against the definition
by enumeration, the torch form of ctc.ctc_prefix_score / ctc_prefix_commit / CTCPrefixScorer against the restatement, and the rules of
DESIGN.md "Beam search", "CTC prefix scores inside the beam" (floor, -inf, weight 0)."""
import math

import pytest
import torch

import ctc_beam_ref as br
import ctc_prefix_score_ref as ps

NEG = float("-inf")


def _lp(T, V, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(T, V, generator=g, dtype=torch.float64) * 1.5, dim=-1).tolist()


PREFIXES = [(), (1,), (2,), (1, 2), (2, 1), (1, 1), (2, 2), (1, 2, 1), (1, 1, 2), (2, 1, 1), (2, 2, 2)]


@pytest.mark.parametrize("T", [0, 1, 2, 3, 4, 5])
def test_restatement_is_the_enumeration(T):
    """V = 3 (blank, 1, 2): psi of every prefix up to 3 labels, repeats included, is the summed probability of the labellings whose
    collapsed string starts with it; gn[T-1] (+) gb[T-1] is the probability of the string itself"""
    x = _lp(T, 3, 100 + T)
    whole = br.brute_force(x) if T else {(): 0.0}
    for h in PREFIXES:
        st = ps.string_state(x, T, h)
        want = ps.brute_psi(x, T, h)
        if want == NEG:
            assert st[2] == NEG, (h, st[2])
        else:
            assert abs(st[2] - want) <= 1e-12 * max(1.0, abs(want)), (h, st[2], want)
        end, w_end = ps.psi_end(T, st, not h), whole.get(tuple(h), NEG)
        assert (end == w_end) if w_end == NEG else abs(end - w_end) <= 1e-12 * max(1.0, abs(w_end)), (h, end, w_end)


def test_psi_of_the_ended_string_is_the_ctc_loss():
    g = torch.Generator().manual_seed(7)
    T, V = 11, 9
    lp = torch.log_softmax(torch.randn(T, V, generator=g, dtype=torch.float64), dim=-1)
    for labels in ([], [4], [4, 4], [3, 5, 5, 8], [6, 6, 6, 6, 6, 6]):
        st = ps.string_state(lp.tolist(), T, labels)
        nll = torch.nn.functional.ctc_loss(lp.unsqueeze(1), torch.tensor([labels], dtype=torch.int64).view(1, -1), torch.tensor([T]),
                                           torch.tensor([len(labels)]), blank=0, reduction="none", zero_infinity=False)
        assert abs(ps.psi_end(T, st, not labels) + float(nll)) <= 1e-10, labels
    st = ps.string_state(lp.tolist(), 3, [4, 4])                  # "aa" needs three frames ...
    assert ps.psi_end(3, st, False) > NEG
    st = ps.string_state(lp.tolist(), 2, [4, 4])                  # ... and does not fit into two
    assert ps.psi_end(2, st, False) == NEG and st[2] == NEG


CASES = [  # seed, Bs, G, K, V, S, lens, lam, first_only, finished
    (1, 3, 2, 4, 9, 8, [7, 5, 0], 0.3, False, ()),
    (2, 2, 5, 10, 16, 7, [6, 1], 0.5, False, (1,)),
    (3, 3, 3, 6, 12, 6, [2, 5, 3], 1.0, True, ()),
    (4, 2, 1, 1, 9, 5, [4, 0], 0.3, False, ()),
    (5, 2, 2, 8, 14, 6, [5, 5], 0.0, False, ()),
]


@pytest.mark.parametrize("seed,Bs,G,K,V,S,lens,lam,first_only,finished", CASES)
def test_composed_form_against_the_restatement(seed, Bs, G, K, V, S, lens, lam, first_only, finished):
    case = ps.make_case(seed, Bs, G, K, V, S, lens, lam, first_only=first_only, finished=finished)
    out = ps.run_case(case, None, "cpu")
    assert ps.check_case(case, out) >= 1


def test_floor_and_minus_infinity_rules():
    """an extension no alignment spells, blank / pad / negative candidates: FLOOR, finite; an attention -inf stays -inf at any weight;
    T = 0: only the empty hypothesis' EOS has an alignment; no NaN anywhere"""
    from simulst_amd import ctc
    assert ctc.SCORE_FLOOR == ps.FLOOR == -1.0e4
    S, K, G, V = 4, 6, 1, 8
    x = torch.log_softmax(torch.randn(3, S, V, generator=torch.Generator().manual_seed(3)), dim=-1)
    # row 0: hypothesis (5, 5) over 3 frames, extended by 5 again -- "555" needs five frames; row 1: T = 0, empty; row 2: T = 0, one label
    lens = [3, 0, 0]
    st0 = ps.string_state(x[0].double().tolist(), 3, [5, 5])
    state = torch.full((3, S, 2), float("nan"))
    for t in range(3):
        state[0, t, 0], state[0, t, 1] = st0[0][t], st0[1][t]
    psi = torch.tensor([st0[2], 0.0, NEG])
    last, plen = torch.tensor([5, -1, 4]), torch.tensor([2, 0, 1])
    toks = torch.tensor([[5, 0, 1, -1, 2, 6]] * 3, dtype=torch.int32)
    lp = torch.tensor([[-1.0, -2.0, -3.0, -4.0, -5.0, NEG]] * 3)
    xc = x.gather(2, toks.view(3, 1, K).long().clamp(0, V - 1).expand(3, S, K)).contiguous()
    for lam in (0.3, 1.0):
        cand_lp, cand_tok = lp.clone(), toks.clone()
        slot, cst, cpsi = torch.zeros(3, K, dtype=torch.int32), torch.zeros(3, S, K, 2), torch.zeros(3, K)
        ctc.ctc_prefix_score(None, xc, x[:, :, 0].contiguous(), state, psi, last, plen, torch.tensor(lens), None, cand_lp, cand_tok, slot,
                             cst, cpsi, G=G, blank=0, eos=2, pad=1, weight=lam)
        assert not bool(torch.isnan(cand_lp).any()) and not bool(torch.isnan(cpsi).any())
        assert cpsi[0].tolist()[:4] == [NEG] * 4 and cpsi[0, 4] > NEG                    # 555, blank, pad, -1: no alignment; EOS has
        assert cpsi[1].tolist() == [NEG, NEG, NEG, NEG, 0.0, NEG]                        # T = 0, empty: EOS alone, probability 1
        assert cpsi[2].tolist() == [NEG] * 6                                             # T = 0, a label: nothing
        for r in range(3):
            by_tok = {int(t): float(v) for t, v in zip(cand_tok[r], cand_lp[r])}
            assert by_tok[6] == NEG                                                      # the attention's -inf is kept
            for c, a in ((5, -1.0), (0, -2.0), (1, -3.0), (-1, -4.0)):
                assert by_tok[c] == pytest.approx((1 - lam) * a + lam * ps.FLOOR, abs=1e-2) and math.isfinite(by_tok[c])
        assert float(cand_lp[1, 0]) == pytest.approx((1 - lam) * -5.0, abs=1e-6) and int(cand_tok[1, 0]) == 2


def test_weight_zero_returns_the_lists_bit_for_bit():
    case = ps.make_case(11, 2, 3, 6, 12, 6, [6, 4], 0.0, att_inf=False)
    order = torch.sort(case["cand_lp"], dim=1, descending=True, stable=True).indices          # candidate order, as the top-k leaves it
    case["cand_lp"], case["cand_tok"] = case["cand_lp"].gather(1, order), case["cand_tok"].gather(1, order)
    out = ps.run_case(case, None, "cpu")
    assert torch.equal(out["cand_lp"], case["cand_lp"]) and torch.equal(out["cand_tok"], case["cand_tok"])
    assert torch.equal(out["cand_slot"], torch.arange(6, dtype=torch.int32).expand(6, 6))


def test_order_on_equal_scores_and_commit():
    """equal combined scores go to the lower token; commit takes the chosen candidate's state, counts a token that is not there"""
    from simulst_amd import ctc
    S, K, G, V = 5, 4, 2, 9
    R = 2 * G
    x = torch.log_softmax(torch.randn(2, S, V, generator=torch.Generator().manual_seed(5)), dim=-1)
    sc = ctc.CTCPrefixScorer(None, None, None, torch.tensor([5, 3]), beam=G, weight=1.0, pad=1, eos=2, log_probs=x)
    assert sc.composed and sc.K == K

    class BS:                                                    # what the scorer reads of a BeamSearch
        cand_tok = torch.tensor([[7, 1, 0, 3]] * R, dtype=torch.int32)
        cand_lp = torch.tensor([[-1.0, -2.0, -3.0, -4.0]] * R)
        finished = torch.zeros(2, dtype=torch.int32)
        next_tok = torch.tensor([3, 7, 7, 8])
        reorder = torch.tensor([0, 0, 2, 2], dtype=torch.int32)
        result = torch.zeros(4, dtype=torch.int32)

    bs = BS()
    sc.rescore(0, bs)
    # weight 1: blank 0 and pad 1 both score FLOOR exactly -> the lower token first; rows j > 0 untouched at step 0
    assert bs.cand_tok[0].tolist()[2:] == [0, 1] and bs.cand_lp[0, 2] == bs.cand_lp[0, 3] == ps.FLOOR
    assert bs.cand_tok[1].tolist() == [7, 1, 0, 3] and bs.cand_tok[2].tolist()[2:] == [0, 1]
    sc.commit(0, bs)
    assert int(bs.result[3]) == 1                                # row 3 asked for 8, which its parent's list does not hold
    assert sc.cur == 1 and sc.last[1].tolist()[:3] == [3, 7, 7] and sc.plen[1].tolist()[:3] == [1, 1, 1]
    for r, (s, c) in enumerate(((0, 3), (0, 7), (1, 7))):
        T = [5, 3][s]
        ref = ps.string_state(x[s].double().tolist(), T, [c])
        assert abs(float(sc.psi[1][r]) - ref[2]) <= br.beam_bound(T, ref[2])
        for t in range(T):
            for i in (0, 1):
                v, w = float(sc.state[1][r, t, i]), ref[i][t]
                assert (v == w) if w == NEG else abs(v - w) <= br.beam_bound(t + 1, w), (r, t, i, v, w)


def test_surface_refusals():
    from simulst_amd import ctc
    x = torch.zeros(1, 2, 5)
    for w in (-0.1, 1.5):
        with pytest.raises(ValueError):
            ctc.CTCPrefixScorer(None, None, None, torch.tensor([2]), beam=2, weight=w, pad=1, eos=2, log_probs=x)
    with pytest.raises(ValueError):
        ctc.CTCPrefixScorer(None, None, None, torch.tensor([2]), beam=17, weight=0.3, pad=1, eos=2, log_probs=x)
    import inspect

    from simulst_amd.beam import BeamSearch
    from simulst_amd.decoder import MMADecoder
    from simulst_amd.model import SimulSTModel
    assert inspect.signature(BeamSearch.run).parameters["rescore"].default is None
    assert inspect.signature(MMADecoder.beam_offline).parameters["ctc"].default is None
    p = inspect.signature(SimulSTModel.generate).parameters
    assert p["ctc_weight"].default == 0.0 and p["blank"].default == 0
