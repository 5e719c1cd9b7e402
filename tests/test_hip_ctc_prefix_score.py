"""The scoring and commit launches of csrc/ctc_prefix_score.hip (ctc.ctc_prefix_score / ctc_prefix_commit) against the fp64
restatement of tests/ctc_prefix_score_ref.py, within ctc_beam_ref.beam_bound.  GPU only.

Every case holds empty, one-label and longer hypotheses (repeats included) and, where K allows, the candidates c == e, EOS, blank, pad,
a negative id and an attention -inf; every input is NaN at and past a sentence's frame count T, with S > T."""
import pytest
import torch

import ctc_beam_ref as br
import ctc_prefix_score_ref as ps

pytestmark = pytest.mark.gpu

NEG = float("-inf")
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from simulst_amd.ops import Ops
    return Ops()


# the frame counts around the staging block (32 frames) and its double, T = 0, 1, 2; S > T everywhere
LENS = [0, 1, 2, 63, 64, 65]


@pytest.mark.parametrize("K,G,V,lam", [(1, 1, 9, 0.3), (2, 5, 9, 0.5), (10, 5, 16, 0.3), (32, 16, 40, 1.0), (10, 16, 16, 1.0), (32, 1, 40, 0.3)])
def test_kernel_against_the_restatement(ops, K, G, V, lam):
    case = ps.make_case(100 + K + G, len(LENS), G, K, V, 67, LENS, lam)
    out = ps.run_case(case, ops, DEV)
    assert ps.check_case(case, out) == len(LENS) * G


def test_first_only_and_finished_rows_stay_untouched(ops):
    """step 0 scores row j = 0 alone; a finished sentence's rows are not touched: sentinel-filled buffers, bit for bit"""
    case = ps.make_case(7, 4, 5, 10, 16, 40, [33, 40, 5, 17], 0.3, first_only=True, finished=(2,))
    assert ps.check_case(case, ps.run_case(case, ops, DEV)) == 3
    case = ps.make_case(8, 4, 5, 10, 16, 40, [33, 40, 5, 17], 0.3, finished=(0, 3))
    assert ps.check_case(case, ps.run_case(case, ops, DEV)) == 10


def test_slot_and_row_independence_bit_for_bit(ops):
    """one (hypothesis, candidate) pair gives the same bits in every slot, in every row, and beside any other candidates"""
    G, K, V, S, T = 5, 10, 16, 70, 65
    base = ps.make_case(21, 2, G, K, V, S, [T, T], 0.3, att_inf=False)
    out0 = ps.run_case(base, ops, DEV)
    # the same hypotheses in other rows (the sentence's rows reversed) with every list rotated by three slots and two candidates changed
    case = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in base.items()}
    R = 2 * G
    src = torch.tensor([s * G + (G - 1 - j) for s in range(2) for j in range(G)])
    for name in ("state", "psi", "last", "plen"):
        case[name] = base[name][src]
    rot = (torch.arange(K) + 3) % K
    tok = base["cand_tok"][src][:, rot].clone()
    lp = base["cand_lp"][src][:, rot].clone()
    keep = torch.ones(R, K, dtype=torch.bool)
    keep[:, 0] = keep[:, 5] = False                               # these two slots hold other candidates now
    tok[:, 0], tok[:, 5] = 0, -1
    case["cand_tok"], case["cand_lp"] = tok, lp
    case["x"] = base["x"].view(2, S, G, K)[:, :, torch.arange(G - 1, -1, -1)][:, :, :, rot].reshape(2, S, G * K).contiguous()
    out1 = ps.run_case(case, ops, DEV)
    for r in range(R):
        for k in range(K):
            if not keep[r, k]:
                continue
            k0 = int(rot[k])
            assert torch.equal(out1["cand_psi"][r, k], out0["cand_psi"][src[r], k0]), (r, k)
            assert torch.equal(out1["cand_state"][r, :T, k], out0["cand_state"][src[r], :T, k0]), (r, k)
            p1 = out1["cand_slot"][r].tolist().index(k)
            p0 = out0["cand_slot"][src[r]].tolist().index(k0)
            assert torch.equal(out1["cand_lp"][r, p1], out0["cand_lp"][src[r], p0]), (r, k)


def test_equal_scores_go_to_the_lower_token(ops):
    """weight 1: blank, pad and a negative id all score FLOOR exactly, whatever their attention scores -- ordered by token"""
    from simulst_amd import ctc
    S, K, G, V, T = 8, 6, 1, 9, 5
    x = torch.log_softmax(torch.randn(1, S, V, generator=torch.Generator().manual_seed(2)), dim=-1)
    st = ps.empty_state(x[0].double().tolist(), T)
    state = torch.full((1, S, 2), float("nan"))
    state[0, :T, 0], state[0, :T, 1] = NEG, torch.tensor(st[1])
    toks = torch.tensor([[1, 5, 0, -1, 7, 2]], dtype=torch.int32)
    lp = torch.tensor([[-0.5, -1.0, -9.0, -2.0, -3.0, -4.0]])
    xc = x.gather(2, toks.view(1, 1, K).long().clamp(0, V - 1).expand(1, S, K)).contiguous()
    t = [v.to(DEV) for v in (xc, x[:, :, 0].contiguous(), state, torch.zeros(1), torch.tensor([-1]), torch.tensor([0]), torch.tensor([T]),
                             lp, toks, torch.zeros(1, K, dtype=torch.int32), torch.zeros(1, S, K, 2), torch.zeros(1, K))]
    ctc.ctc_prefix_score(ops, t[0], t[1], t[2], t[3], t[4], t[5], t[6], None, t[7], t[8], t[9], t[10], t[11], G=G, blank=0, eos=2, pad=1,
                         weight=1.0)
    assert t[8][0, 3:].tolist() == [-1, 0, 1] and t[7][0, 3:].tolist() == [ps.FLOOR] * 3
    assert t[9][0, 3:].tolist() == [3, 2, 0]


def _chain(ops, composed=False):
    """score + commit along a fixed string of 6 labels in every row of 3 sentences x 2 rows, the parents swapped at every step"""
    from simulst_amd import ctc
    Bs, G, K, V, S = 3, 2, 4, 9, 70
    lens = [65, 33, 12]
    labels = [4, 4, 7, 3, 3, 5]
    g = torch.Generator().manual_seed(17)
    x = torch.log_softmax(torch.randn(Bs, S, V, generator=g, dtype=torch.float64) * 1.5, dim=-1).float()
    xd = x.clone()
    for s in range(Bs):
        xd[s, lens[s]:] = float("nan")
    sc = ctc.CTCPrefixScorer(ops, None, None, torch.tensor(lens), beam=G, weight=0.3, pad=1, eos=2, log_probs=xd.to(DEV), composed=composed)
    R = Bs * G

    class BS:
        cand_tok = torch.zeros(R, K, dtype=torch.int32, device=DEV)
        cand_lp = torch.zeros(R, K, device=DEV)
        finished = torch.zeros(Bs, dtype=torch.int32, device=DEV)
        next_tok = torch.zeros(R, dtype=torch.int64, device=DEV)
        reorder = torch.zeros(R, dtype=torch.int32, device=DEV)
        result = torch.zeros(4, dtype=torch.int32, device=DEV)

    bs = BS()
    for step, c in enumerate(labels):
        others = [v for v in (3, 4, 5, 6, 7, 8) if v != c]
        for r in range(R):
            row = [others[(r + step) % 5], 2, others[(r + step + 1) % 5]]
            row.insert((r + step) % K, c)                          # the string's label in a slot that moves
            bs.cand_tok[r] = torch.tensor(row, dtype=torch.int32)
        bs.cand_lp.copy_(-torch.rand(R, K, generator=g) * 3)
        bs.next_tok.fill_(c)
        bs.reorder.copy_(torch.tensor([s * G + (0 if step == 0 else (j + 1) % G) for s in range(Bs) for j in range(G)], dtype=torch.int32))
        sc.rescore(step, bs)
        sc.commit(step, bs)
    return sc, bs, x, lens, labels


def test_score_and_commit_chained_along_a_string(ops):
    from simulst_amd import ctc_align
    sc, bs, x, lens, labels = _chain(ops)
    torch.cuda.synchronize()
    assert int(bs.result[3]) == 0
    c = sc.cur
    state, psi = sc.state[c].cpu(), sc.psi[c].cpu()
    assert sc.last[c].tolist() == [labels[-1]] * 6 and sc.plen[c].tolist() == [len(labels)] * 6
    ends = []
    for r in range(6):
        s, T = r // 2, lens[r // 2]
        ref = ps.string_state(x[s].double().tolist(), T, labels)
        assert abs(float(psi[r]) - ref[2]) <= br.beam_bound(T, ref[2]), (r, float(psi[r]), ref[2])
        for t in range(T):
            for i in (0, 1):
                v, w = float(state[r, t, i]), ref[i][t]
                assert (v == w) if w == NEG else abs(v - w) <= br.beam_bound(t + 1, w), (r, t, i, v, w)
        ends.append(ps.psi_end(T, ref, False))
    # psi(g . eos) of the chain's final state against the sum over alignments of g (ctc_align.ctc_nll)
    bs.cand_tok.copy_(torch.tensor([[2, 3, 4, 5]] * 6, dtype=torch.int32))
    sc.rescore(len(labels), bs)
    got = sc.cand_psi[:, 0].cpu()
    lp_sbv = x.to(DEV).transpose(0, 1).repeat_interleave(2, 1)
    tg = torch.tensor([labels] * 6, device=DEV)
    nll = ctc_align.ctc_nll(lp_sbv, tg, torch.tensor(lens, device=DEV).repeat_interleave(2), torch.full((6,), len(labels), device=DEV),
                            blank=0, ops=ops).cpu()
    for r in range(6):
        T = lens[r // 2]
        assert abs(float(got[r]) - ends[r]) <= br.beam_bound(T, ends[r]), (r, float(got[r]), ends[r])
        assert abs(float(got[r]) + float(nll[r])) <= br.beam_bound(T, ends[r]), (r, float(got[r]), float(nll[r]))


def test_kernel_and_composed_chain_agree_within_the_bound(ops):
    a, _, x, lens, labels = _chain(ops)
    b, _, _, _, _ = _chain(ops, composed=True)
    pa, pb = a.psi[a.cur].cpu(), b.psi[b.cur].cpu()
    for r in range(6):
        assert abs(float(pa[r]) - float(pb[r])) <= 2 * br.beam_bound(lens[r // 2], float(pa[r])), r


def test_commit_counts_a_token_that_is_not_there(ops):
    from simulst_amd import ctc
    G, K, S, R = 2, 4, 6, 4
    i32, f32 = dict(dtype=torch.int32, device=DEV), dict(dtype=torch.float32, device=DEV)
    cand_state = torch.arange(R * S * K * 2, **f32).view(R, S, K, 2)
    cand_psi = -torch.arange(R * K, **f32).view(R, K)
    cand_tok = torch.tensor([[5, 6, 7, 8]] * R, **i32)
    cand_slot = torch.tensor([[2, 0, 3, 1]] * R, **i32)
    next_tok = torch.tensor([7, 9, 6, 5], device=DEV)            # row 1 asks for 9: not among its parent's candidates
    reorder = torch.tensor([1, 0, 0, 3], **i32)                  # row 2 asks for a parent of the other sentence
    finished = torch.zeros(2, **i32)
    plen, in_len = torch.tensor([2, 3, 1, 4], device=DEV), torch.tensor([6, 6, 4, 4], device=DEV)
    last = torch.zeros(R, dtype=torch.int64, device=DEV)
    state_out, psi_out = torch.full((R, S, 2), -7.0, **f32), torch.full((R,), -7.0, **f32)
    last_out, len_out = torch.full((R,), -7, device=DEV), torch.full((R,), -7, device=DEV)
    result = torch.zeros(1, **i32)
    ctc.ctc_prefix_commit(ops, cand_state, cand_psi, cand_tok, cand_slot, next_tok, reorder, finished, last, plen, in_len, state_out,
                          psi_out, last_out, len_out, result, G=G)
    assert int(result[0]) == 2
    assert last_out.tolist() == [7, -7, -7, 5] and len_out.tolist() == [4, -7, -7, 5]
    assert torch.equal(state_out[0], cand_state[1, :, 3]) and float(psi_out[0]) == float(cand_psi[1, 3])          # token 7: position 2, slot 3
    assert torch.equal(state_out[3, :4], cand_state[3, :4, 2]) and bool((state_out[3, 4:] == -7).all())          # token 5: slot 2, 4 frames
    assert bool((state_out[1:3] == -7).all()) and psi_out[1:3].tolist() == [-7.0, -7.0]
    # a finished sentence's rows are left alone, and not counted
    finished[0] = 1
    state_out.fill_(-7.0)
    result.zero_()
    ctc.ctc_prefix_commit(ops, cand_state, cand_psi, cand_tok, cand_slot, next_tok, reorder, finished, last, plen, in_len, state_out,
                          psi_out, last_out, len_out, result, G=G)
    assert int(result[0]) == 1 and bool((state_out[:2] == -7).all())
