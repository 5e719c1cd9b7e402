"""CTC prefix beam search over the head's candidate lists (simulst_amd/ctc.py: ctc_topk, ctc_prefix_beam_search; the model-level
transcribe_ctc_nbest) on the MI355X against the fp64 dict-of-tuples reference of tests/ctc_beam_ref.py run on the DEVICE'S OWN candidate
lists, brute force over every path, the greedy path and the exact CTC likelihood (ctc.ctc_score).  GPU only.

Score bound of an utterance of Te_b frames: (Te_b + 1) 2^-22 max(1, |score_ref|), the form tests/test_hip_ctc_nll.py uses.  An utterance
whose smallest selection-boundary / final-ranking margin (reported by the reference) is <= twice that bound is UNCLEAR: its n-best
identity is not compared, the bound against the exact likelihood still is; at most 10 % of a case may be unclear."""
import pytest
import torch

import ctc_beam_ref as br

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16]
BEAM, CAND, NBEST = 8, 8, 4


@pytest.fixture(scope="module")
def ops():
    from simulst_amd.ops import Ops
    return Ops()


_CASES = {}


def _case(ops, dtype):
    """rows, head, lengths on the device; the device's candidate lists; one search over all rows -- made once and shared"""
    if dtype not in _CASES:
        from simulst_amd import ctc
        enc, W, L, _ = br.beam_operands(dtype)
        encd, Wd, Ld = enc.to(DEV), W.to(DEV), L.to(DEV)
        cand = ctc.ctc_topk(ops, Wd, encd, Ld, k=CAND)
        got = ctc.ctc_prefix_beam_search(ops, Wd, encd, Ld, beam=BEAM, candidates=CAND, nbest=NBEST)
        torch.cuda.synchronize()
        _CASES[dtype] = (encd, Wd, Ld, {k: v.cpu() for k, v in cand.items()}, {k: v.cpu() for k, v in got.items()})
    return _CASES[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_candidates_past_the_length(ops, dtype):
    _, _, L, cand, _ = _case(ops, dtype)
    ids, lp = cand["ids"], cand["lprob"]
    assert ids.shape == lp.shape == (len(br.BEAM_LENGTHS), max(br.BEAM_LENGTHS), CAND + 1) and ids.dtype == torch.int32
    for b, n in enumerate(br.BEAM_LENGTHS):
        assert bool((ids[b, n:, 0] == 0).all()) and bool((ids[b, n:, 1:] == -1).all())
        assert bool((lp[b, n:, 0] == 0).all()) and bool((lp[b, n:, 1:] == float("-inf")).all())
        assert bool((ids[b, :n] >= 0).all()) and bool(torch.isfinite(lp[b, :n]).all())
        assert bool((lp[b, :n, 1:-1] >= lp[b, :n, 2:]).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_search_against_the_reference_on_the_devices_candidates(ops, dtype):
    _, _, _, cand, got = _case(ops, dtype)
    B = len(br.BEAM_LENGTHS)
    assert got["tokens"].shape[:2] == got["n"].shape == got["score"].shape == (B, NBEST) and got["tokens"].dtype == torch.int64
    unclear = 0
    for b, n in enumerate(br.BEAM_LENGTHS):
        ids, lp = br.candidates_of(cand["ids"][b], cand["lprob"][b], n)
        hyps, margin = br.prefix_beam_ref(ids, lp, beam=BEAM, nbest=NBEST)
        bound = br.beam_bound(n, hyps[0][1])
        if margin <= 2 * bound:
            unclear += 1
            continue
        for j in range(NBEST):
            k = int(got["n"][b, j])
            if j >= len(hyps):
                assert k == 0 and float(got["score"][b, j]) == float("-inf")
                continue
            assert tuple(got["tokens"][b, j, :k].tolist()) == hyps[j][0], (b, j, got["tokens"][b, j, :k].tolist(), hyps[j])
            assert bool((got["tokens"][b, j, k:] == 1).all())
            d = abs(float(got["score"][b, j]) - hyps[j][1])
            print(f"{dtype} utterance {b} hypothesis {j}: |score - ref| {d:.3e}  bound {br.beam_bound(n, hyps[j][1]):.3e}  margin {margin:.3e}")
            assert d <= br.beam_bound(n, hyps[j][1])
    print(f"{dtype}: {unclear} of {B} utterances unclear")
    assert unclear <= 0.1 * B


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_score_exceeds_the_exact_likelihood(ops, dtype):
    from simulst_amd import ctc
    enc, W, L, _, got = _case(ops, dtype)
    B = enc.size(0)
    tgt = got["tokens"].reshape(B * NBEST, -1).to(DEV)
    tl = got["n"].reshape(-1).to(DEV)
    s = ctc.ctc_score(ops, W, enc.repeat_interleave(NBEST, 0), L.repeat_interleave(NBEST), tgt, tl)
    nll = s["nll"].cpu().view(B, NBEST)
    for b, n in enumerate(br.BEAM_LENGTHS):
        for j in range(NBEST):
            sc = float(got["score"][b, j])
            if sc == float("-inf"):
                continue
            assert sc <= -float(nll[b, j]) + br.beam_bound(n, sc), (b, j, sc, -float(nll[b, j]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_peaky_frames_give_the_greedy_transcript(ops, dtype):
    """every frame points along one label's weight row (that label's logit about 12 above the rest): the best prefix is the collapsed
    best path"""
    from simulst_amd import ctc
    g = torch.Generator().manual_seed(12)
    D, V, B, Te = 64, 40, 6, 40
    W = (torch.randn(V, D, generator=g) * 4 / D ** 0.5)
    lab = torch.randint(0, V, (B, Te), generator=g)
    lab[:, 1::3] = lab[:, 0::3][:, :lab[:, 1::3].size(1)]                      # runs of two
    lab[:, 5::7] = 0
    enc = W[lab] * (12.0 / W.pow(2).sum(1))[lab].unsqueeze(-1) + 0.05 * torch.randn(B, Te, D, generator=g)
    L = torch.tensor([40, 0, 1, 17, 33, 40])
    encd, Wd = enc.to(dtype).to(DEV), W.to(dtype).to(DEV)
    greedy = ctc.ctc_greedy(ops, Wd, encd, L.to(DEV))
    got = ctc.ctc_prefix_beam_search(ops, Wd, encd, L.to(DEV), beam=BEAM, candidates=CAND, nbest=1)
    for b in range(B):
        k = int(greedy["n"][b])
        assert int(got["n"][b, 0]) == k and got["tokens"][b, 0, :k].tolist() == greedy["tokens"][b, :k].tolist()
        assert float(got["score"][b, 0]) >= float(greedy["score"][b]) - 1e-4
    assert int(greedy["n"].max()) > 10


def test_small_vocabulary_against_every_path(ops):
    """V = 4, Te = 6, beam 16, k = 3 (every label a candidate): the best prefix is the labeling with the largest summed probability
    over all 4^6 paths of the device's own log-probabilities"""
    from simulst_amd import ctc
    g = torch.Generator().manual_seed(5)
    B, Te, D, V = 8, 6, 32, 4
    enc = torch.randn(B, Te, D, generator=g).to(DEV)
    W = (torch.randn(V, D, generator=g) * 3 / D ** 0.5).to(DEV)
    L = torch.full((B,), Te, device=DEV)
    cand = ctc.ctc_topk(ops, W, enc, L, k=3)
    got = ctc.ctc_prefix_beam_search(ops, W, enc, L, beam=16, candidates=3, nbest=2)
    ids, lp = cand["ids"].cpu(), cand["lprob"].cpu().double()
    checked = 0
    for b in range(B):
        full = torch.empty(Te, V, dtype=torch.float64)
        full.scatter_(1, ids[b].to(torch.int64), lp[b])
        exact = br.brute_force(full.tolist())
        ranked = sorted(exact.items(), key=lambda kv: -kv[1])
        bound = br.beam_bound(Te, ranked[0][1])
        k = int(got["n"][b, 0])
        assert float(got["score"][b, 0]) <= exact[tuple(got["tokens"][b, 0, :k].tolist())] + bound
        if ranked[0][1] - ranked[1][1] <= 2 * bound:
            continue
        checked += 1
        assert tuple(got["tokens"][b, 0, :k].tolist()) == ranked[0][0], (b, got["tokens"][b, 0, :k].tolist(), ranked[:2])
        # (beam 16 keeps fewer than the 1093 prefixes: the score may miss pruned alignments, so it is only bounded from above)
    assert checked >= B - 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_chunks_of_16_rows_with_state_equal_one_call(ops, dtype):
    from simulst_amd import ctc
    enc, W, L, _, got = _case(ops, dtype)
    state = None
    for c in range(0, enc.size(1), 16):
        r = ctc.ctc_prefix_beam_search(ops, W, enc[:, c:c + 16], (L - c).clamp(0, 16), beam=BEAM, candidates=CAND, nbest=NBEST,
                                       state=state, return_state=True)
        state = r["state"]
    assert torch.equal(r["tokens"].cpu(), got["tokens"]) and torch.equal(r["n"].cpu(), got["n"])
    assert torch.equal(r["score"].cpu(), got["score"])                    # the same bits
    with pytest.raises(ValueError, match="state"):
        ctc.ctc_prefix_beam_search(ops, W, enc[:2], L[:2], beam=BEAM, state=state)
    with pytest.raises(ValueError, match="nbest"):
        ctc.ctc_prefix_beam_search(ops, W, enc, L, beam=4, nbest=5)
    with pytest.raises(ValueError, match="beam"):
        ctc.ctc_prefix_beam_search(ops, W, enc, L, beam=17)


@pytest.mark.parametrize("dtype", DTYPES)
def test_padded_frames_change_nothing(ops, dtype):
    from simulst_amd import ctc
    enc, W, L, _, got = _case(ops, dtype)
    g = torch.Generator().manual_seed(1)
    more = torch.cat([enc, (torch.randn(enc.size(0), 9, enc.size(2), generator=g) * 3).to(enc.dtype).to(DEV)], dim=1)
    r = ctc.ctc_prefix_beam_search(ops, W, more, L, beam=BEAM, candidates=CAND, nbest=NBEST)
    assert torch.equal(r["tokens"].cpu(), got["tokens"]) and torch.equal(r["n"].cpu(), got["n"]) and torch.equal(r["score"].cpu(), got["score"])
    # the candidate lists of padded frames alone, as ctc_topk writes them, leave a state as it is: lengths say "all 57 frames"
    cand = ctc.ctc_topk(ops, W, more, L, k=CAND)
    st = ctc.ctc_prefix_beam_advance(cand["ids"], cand["lprob"], torch.full_like(L, more.size(1)), ctc.ctc_prefix_beam_init(enc.size(0), BEAM, DEV))
    score = ctc._lae(st[2], st[3])[:, :NBEST].cpu()
    assert torch.equal(score, got["score"]) and torch.equal(st[1][:, :NBEST].cpu(), got["n"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_model_level_nbest(dtype):
    from simulst_amd.config import tiny
    from simulst_amd.model import S2TEmformerModel, SimulSTModel
    from simulst_amd.weights import init_model
    cfg = tiny(model="s2t_emformer", simul_attn_type="full", mass_preservation=False, ctc_layer=True)
    model = S2TEmformerModel(cfg, init_model(cfg, seed=32), device=DEV, dtype=dtype)
    lengths = [333, 40, 200, 97]
    g = torch.Generator().manual_seed(77)
    fb = torch.randn(len(lengths), max(lengths), 80, generator=g)
    for b, n in enumerate(lengths):
        fb[b, n:] = 0
    L = torch.tensor(lengths)
    out = model.transcribe_ctc_nbest(fb.to(DEV), L, beam=8, nbest=4)
    assert len(out) == len(lengths)
    enc = model.encoder.forward(fb.to(DEV), L)
    step_ms = model.encoder.conv_layer_stride() * 10
    for b, hyps in enumerate(out):
        assert 1 <= len(hyps) <= 4
        nll = [h["nll"] for h in hyps]
        assert nll == sorted(nll)
        n_rows = int(enc["encoder_lengths"][b])
        for h in hyps:
            assert h["beam_score"] <= -h["nll"] + br.beam_bound(n_rows, h["beam_score"])
        assert len({tuple(h["tokens"]) for h in hyps}) == len(hyps)
        best = hyps[0]
        assert len(best["frames"]) == len(best["tokens"]) and best["frames_ms"] == [f * step_ms for f in best["frames"]]
        if best["tokens"]:
            tgt = torch.tensor([best["tokens"]], device=DEV)
            s = model.encoder.ctc_score(enc["encoder_out_btd"][b:b + 1], enc["encoder_lengths"][b:b + 1], tgt,
                                        torch.tensor([len(best["tokens"])], device=DEV), align=True)
            al = s["alignment"][0, :n_rows].cpu().tolist()
            starts = [t for t in range(n_rows) if al[t] != 0 and (t == 0 or al[t] != al[t - 1])]
            assert best["frames"] == starts and [al[t] for t in starts] == best["tokens"]
            assert best["frames"] == sorted(best["frames"]) and best["frames"][-1] < n_rows
    plain = model.transcribe_ctc_nbest(fb.to(DEV), L, beam=8, nbest=4, rescore=False)
    for hyps in plain:
        assert all(set(h) == {"tokens", "beam_score"} for h in hyps)
        assert [h["beam_score"] for h in hyps] == sorted((h["beam_score"] for h in hyps), reverse=True)
    cfg0 = tiny(waitk_lagging=3)
    m0 = SimulSTModel(cfg0, init_model(cfg0, seed=3), device=DEV, dtype=torch.float32)
    with pytest.raises(ValueError, match="no CTC head"):
        m0.transcribe_ctc_nbest(fb[:2].to(DEV), L[:2])
