"""The CTC head's scoring surface on the MI355X: CTCTranscriber.score_ctc, S2TEmformerEncoder.ctc_score and ctc.ctc_rescore on the tiny
CTC-headed models of tests/test_hip_ctc_decode.py, against fp64 F.ctc_loss over fp64 logits computed from the encoder rows the device
produced (tests/ctc_ref.logits64) and the head's weights.  GPU only.

Bound of utterance b: Te_b (2e + N 2^-24 + 2^-20) -- every frame of an alignment adds one gathered log-probability, each within the
bound of tests/test_hip_ctc_gather.py, e = 2 x the largest |fp32 - fp64| of the logits simulst_linear writes with
SIMULST_EPI_BIAS_F32OUT for the same rows -- plus the recursion's (Te_b + 1) 2^-22 max(1, max |alpha_ref|) of tests/test_hip_ctc_nll.py."""
import math

import pytest
import torch
import torch.nn.functional as F

import ctc_ref as cr
import ctc_score_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENGTHS = [333, 40, 200, 97]
BLANK = 0


def _build(kind, dtype, head=True):
    from simulst_amd.config import tiny
    from simulst_amd.weights import init_model
    if kind == "cif":
        from simulst_amd.cif import CIFTransformerModel
        cfg = tiny(model="cif_transformer", ctc_layer=head, simul_attn_type="none")
        return CIFTransformerModel(cfg, init_model(cfg, seed=31), device=DEV, dtype=dtype)
    from simulst_amd.model import S2TEmformerModel
    cfg = tiny(model="s2t_emformer", simul_attn_type="full", mass_preservation=False, ctc_layer=head)
    return S2TEmformerModel(cfg, init_model(cfg, seed=32), device=DEV, dtype=dtype)


_MODELS = {}


@pytest.fixture(params=[("cif", torch.float32), ("s2t", torch.bfloat16)], ids=["cif-fp32", "s2t-bf16"])
def model(request):
    if request.param not in _MODELS:
        _MODELS[request.param] = _build(*request.param)
    return _MODELS[request.param]


def _fbank():
    g = torch.Generator().manual_seed(77)
    fb = torch.randn(len(LENGTHS), max(LENGTHS), 80, generator=g)
    for b, n in enumerate(LENGTHS):
        fb[b, n:] = 0
    return fb, torch.tensor(LENGTHS)


def _reference(model, rows, target):
    """rows [n, D] (device, model dtype), target list -> (fp64 nll of the head over them, the bound, its recursion part alone)"""
    from simulst_amd._lib import EPI_BIAS_F32OUT
    rows = rows.contiguous()
    W = model.encoder.w.ctc
    z = cr.logits64(rows, W)
    e = 2 * float((model.ops.linear(rows, W, epilogue=EPI_BIAS_F32OUT).cpu().double() - z).abs().max())
    lp = z.log_softmax(-1)
    n = rows.size(0)
    ref = float(F.ctc_loss(lp.unsqueeze(1), torch.tensor([list(target) + [1]]), torch.tensor([n]), torch.tensor([len(target)]),
                           blank=BLANK, reduction="none"))
    nll, big = sr.alpha64(lp, list(target), BLANK)
    assert (nll == ref) if math.isinf(ref) else abs(nll - ref) <= 1e-9 * max(1.0, abs(ref))
    return ref, n * (2 * e + W.size(0) * 2.0 ** -24 + 2.0 ** -20) + sr.nll_bound(n, big), sr.nll_bound(n, big)


def _targets(V, enc_len):
    """a transcript per utterance: random labels (no blank, no pad) with a repeated pair; one that fills its rows exactly
    (L + repeats == rows); none; a short one"""
    g = torch.Generator().manual_seed(5)
    out = []
    for b, n in enumerate(enc_len):
        if b % 4 == 1:
            out.append([2, 2] + [3 + i % 2 for i in range(n - 3)])
            continue
        k = [12, 0, 0, 5][b % 4]
        t = torch.randint(2, V, (k,), generator=g).tolist()
        if k >= 4:
            t[2] = t[1]
        out.append(t)
    return out


def test_score_ctc_against_fp64_ctc_loss(model):
    fb, L = _fbank()
    enc = model.encoder.forward(fb.to(DEV), L)
    rows, enc_len = enc["encoder_out_btd"], [int(v) for v in enc["encoder_lengths"]]
    targets = _targets(model.encoder.w.ctc.size(0), enc_len)
    got = model.score_ctc(fb.to(DEV), L, targets)
    assert len(got) == len(LENGTHS)
    for b, (t, rec) in enumerate(zip(targets, got)):
        ref, bound, _ = _reference(model, rows[b, :enc_len[b]], t)
        print(f"utterance {b}: rows {enc_len[b]} labels {len(t)}  nll {rec['nll']:.6f}  fp64 {ref:.6f}  bound {bound:.3e}")
        assert math.isfinite(ref) and abs(rec["nll"] - ref) <= bound
        assert rec["score"] == -rec["nll"] / max(len(t), 1)
    # the padded-tensor form of the targets, and the encoder-level call with the forced alignment
    pad = model.encoder.cfg.padding_idx
    tt = torch.full((len(targets), max(len(t) for t in targets)), pad, dtype=torch.int64)
    for b, t in enumerate(targets):
        tt[b, :len(t)] = torch.tensor(t, dtype=torch.int64)
    assert [r["nll"] for r in model.score_ctc(fb.to(DEV), L, tt)] == [r["nll"] for r in got]
    s = model.encoder.ctc_score(rows, enc["encoder_lengths"], tt, torch.tensor([len(t) for t in targets]), align=True)
    assert tuple(s["lprobs"].shape) == (len(targets), rows.size(1), tt.size(1) + 1) and s["lprobs"].dtype == torch.float32
    assert s["nll"].cpu().tolist() == [r["nll"] for r in got]
    ali = s["alignment"].cpu()
    for b, t in enumerate(targets):
        toks, _ = cr.collapse_loop(ali[b].tolist(), enc_len[b], BLANK)
        assert toks == t and bool((ali[b, enc_len[b]:] == BLANK).all())
        assert float(s["nll"][b]) <= float(s["best_nll"][b]) + _reference(model, rows[b, :enc_len[b]], t)[1]


def test_greedy_transcript_scores_at_least_its_best_path(model):
    """the sum over alignments of the greedy transcript contains the greedy path itself"""
    fb, L = _fbank()
    enc = model.encoder.forward(fb.to(DEV), L)
    rows, enc_len = enc["encoder_out_btd"], enc["encoder_lengths"]
    g = model.encoder.ctc_greedy(rows, enc_len, blank=BLANK)
    s = model.encoder.ctc_score(rows, enc_len, g["tokens"], g["n"], blank=BLANK)
    for b in range(rows.size(0)):
        n = int(enc_len[b])
        _, bound, _ = _reference(model, rows[b, :n], g["tokens"][b, :int(g["n"][b])].tolist())
        print(f"utterance {b}: nll {float(s['nll'][b]):.6f}  greedy path {-float(g['score'][b]):.6f}  bound {bound:.3e}")
        assert float(s["nll"][b]) <= -float(g["score"][b]) + bound


def test_rescore_three_hypotheses_of_two_utterances(model):
    from simulst_amd import ctc
    fb, L = _fbank()
    enc = model.encoder.forward(fb.to(DEV)[:2], L[:2])
    rows, enc_len = enc["encoder_out_btd"], enc["encoder_lengths"]
    V = model.encoder.w.ctc.size(0)
    g = torch.Generator().manual_seed(9)
    nbest = []
    for b in range(2):
        hyps = []
        for k, (n, score) in enumerate(zip((6, 3, 8), (-2.0, -1.0, -3.0))):
            t = torch.randint(2, V, (n,), generator=g).tolist()
            if k == 2:
                t[4] = t[3]
            hyps.append((t, score - 0.25 * b))
        nbest.append(hyps)
    W = model.encoder.w.ctc
    for weight in (0.0, 0.3, 1.0):
        ranked = ctc.ctc_rescore(model.ops, W, rows, enc_len, nbest, weight=weight)
        assert len(ranked) == 2 and all(len(r) == 3 for r in ranked)
        for b in range(2):
            for rec in ranked[b]:
                k = [t for t, _ in nbest[b]].index(rec["tokens"])
                assert rec["score"] == nbest[b][k][1]
                # the same hypothesis scored alone: another gather layout (and another column split of the logsumexp): within the
                # recursion's bound
                alone = ctc.ctc_score(model.ops, W, rows[b:b + 1], enc_len[b:b + 1], torch.tensor([rec["tokens"]]),
                                      torch.tensor([len(rec["tokens"])]))
                _, _, bound = _reference(model, rows[b, :int(enc_len[b])], rec["tokens"])
                assert abs(rec["nll"] - float(alone["nll"][0])) <= bound, (rec, float(alone["nll"][0]))
                assert rec["combined"] == pytest.approx((1 - weight) * rec["score"] + weight * -rec["nll"], rel=1e-12, abs=1e-12)
            order = [r["tokens"] for r in ranked[b]]
            if weight == 0.0:
                assert order == [t for t, _ in sorted(nbest[b], key=lambda h: -h[1])]
            if weight == 1.0:
                assert order == [r["tokens"] for r in sorted(ranked[b], key=lambda r: r["nll"])]
    # lists of different lengths: the missing slot is scored as nothing and not returned
    ragged = ctc.ctc_rescore(model.ops, W, rows, enc_len, [nbest[0], nbest[1][:2]], weight=1.0)
    full = ctc.ctc_rescore(model.ops, W, rows, enc_len, nbest, weight=1.0)
    assert ragged[0] == full[0] and len(ragged[1]) == 2
    assert ragged[1] == [r for r in full[1] if r["tokens"] != nbest[1][2][0]]
    with pytest.raises(ValueError, match="nbest"):
        ctc.ctc_rescore(model.ops, W, rows, enc_len, [nbest[0], []], weight=0.5)


def test_model_without_a_head_raises():
    m = _build("s2t", torch.float32, head=False)
    fb, L = _fbank()
    with pytest.raises(ValueError, match="no CTC head"):
        m.score_ctc(fb.to(DEV)[:1], L[:1], [[3, 4]])
    with pytest.raises(ValueError, match="no CTC head"):
        m.encoder.ctc_score(torch.zeros(1, 4, 32, device=DEV), torch.tensor([4]), torch.tensor([[3]]), torch.tensor([1]))
