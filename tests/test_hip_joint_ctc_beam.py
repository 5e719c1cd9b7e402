"""Joint CTC / attention beam search (ctc.CTCPrefixScorer inside beam.BeamSearch, MMADecoder.beam_offline(ctc=...),
SimulSTModel.generate(ctc_weight=...)) against the CPU restatement of tests/joint_ctc_beam_ref.py.  GPU only.

No sentence is excused from the comparison: the inputs are chosen (on the CPU, from the restatement alone) so that every decision of
every sentence has a gap of at least 1e-3, and each test asserts that first."""
import os
import sys

import pytest
import torch

import ctc_beam_ref as br
import joint_ctc_beam_ref as jr

pytestmark = pytest.mark.gpu

NEG = -float("inf")
MIN_GAP = 1e-3


# ---------------------------------------------------------------------------------------------------- scripted logits
V, TE, BEAM, EOS, PAD = 12, 9, 4, 2, 1
ENC_LEN = [9, 7, 8, 6]
CAPS = [4, 3, 4, 3]                      # ragged; a string of n labels needs at most 2 n - 1 frames: every hypothesis has an alignment
SCRIPT_SEED = {(0.3, 1.0): 2, (0.3, 0.6): 2, (1.0, 1.0): 2, (1.0, 0.6): 2}      # chosen on the CPU: the gap assertion below holds
DIFFERENT_BEST_SEED = 2                  # lam 0.3 against lam 0: the two searches end on different best hypotheses for some sentence


class Script:
    """row r at step t: A[last token of r] + c[t], and the CTC head's log-probabilities x [4, TE, V] (NaN past a sentence's frames)"""

    def __init__(self, seed):
        g = torch.Generator().manual_seed(seed)
        self.A = torch.randn(V, V, generator=g) * 2.0
        self.c = torch.randn(max(CAPS) + 1, V, generator=g)
        self.c[:, EOS] += 1.0
        self.x = torch.log_softmax(torch.randn(len(CAPS), TE, V, generator=g, dtype=torch.float64) * 2.0, dim=-1).float()
        self.dev = None

    def cpu(self, t, toks):
        return self.A[toks] + self.c[t]

    def gpu(self, t, toks):
        if self.dev is None:
            self.dev = (self.A.cuda(), self.c.cuda())
        return (self.dev[0][toks] + self.dev[1][t]).contiguous()

    def ref(self, lam, lenpen, nbest=BEAM):
        return jr.joint_beam(self.cpu, jr.rows_of(self.x, ENC_LEN), CAPS, BEAM, V, EOS, PAD, lenpen, nbest, lam)

    def device(self, lam, lenpen, nbest=BEAM):
        from simulst_amd.beam import BeamSearch
        from simulst_amd.ctc import CTCPrefixScorer
        from simulst_amd.ops import Ops
        ops = Ops()
        xd = self.x.clone()
        for s, n in enumerate(ENC_LEN):
            xd[s, n:] = float("nan")
        bs = BeamSearch(ops, CAPS, beam=BEAM, V=V, eos=EOS, pad=PAD, lenpen=lenpen, nbest=nbest)
        if not lam:
            return _device_lists(*bs.run(self.gpu, chunk=2))
        sc = CTCPrefixScorer(ops, None, None, torch.tensor(ENC_LEN), beam=BEAM, weight=lam, pad=PAD, eos=EOS, log_probs=xd.cuda())
        return _device_lists(*bs.run(self.gpu, lambda t: sc.commit(t, bs), chunk=2, rescore=lambda t: sc.rescore(t, bs)))


def _device_lists(tokens, lengths, scores, pos):
    tokens, lengths, scores, pos = tokens.cpu(), lengths.cpu(), scores.cpu(), pos.cpu()
    out = []
    for s in range(tokens.size(0)):
        out.append([(tokens[s, k, :int(lengths[s, k])].tolist(), float(scores[s, k]), pos[s, k, :int(lengths[s, k])])
                    for k in range(tokens.size(1)) if int(lengths[s, k])])
    return out


def _assert_same(got, ref, tol):
    assert len(got) == len(ref)
    for s, (g, r) in enumerate(zip(got, ref)):
        assert [h[0] for h in g] == [h[0] for h in r], (s, g, r)
        for (gt, gs, gp), (rt, rs, rp, _) in zip(g, r):
            assert abs(gs - rs) <= tol, (s, gs, rs)
            torch.testing.assert_close(gp.double(), rp.double(), atol=tol, rtol=0)


@pytest.mark.parametrize("lam,lenpen", sorted(SCRIPT_SEED))
def test_scripted_logits_match_the_restatement(lam, lenpen):
    sc = Script(SCRIPT_SEED[(lam, lenpen)])
    ref, gaps = sc.ref(lam, lenpen)
    for s in range(len(CAPS)):                                    # on the CPU, before anything runs: no decision is a near-tie
        assert min(gaps[s]) >= MIN_GAP, (s, min(gaps[s]))
        assert not any(h[3] for h in ref[s]), s                   # and the floor applied to no returned hypothesis
    _assert_same(sc.device(lam, lenpen), ref, 1e-4)


def test_ctc_term_changes_the_best_hypothesis():
    """a case, picked on the CPU from the restatement, in which the CTC term acts: the joint and the plain search end on different best
    hypotheses, and the device returns both as restated"""
    sc = Script(DIFFERENT_BEST_SEED)
    plain, gp = sc.ref(0.0, 1.0, 1)
    joint, gj = sc.ref(0.3, 1.0, 1)
    for s in range(len(CAPS)):
        assert min(gp[s]) >= MIN_GAP and min(gj[s]) >= MIN_GAP, s
    differ = [s for s in range(len(CAPS)) if plain[s][0][0] != joint[s][0][0]]
    assert differ
    _assert_same(sc.device(0.0, 1.0, 1), plain, 1e-4)
    _assert_same(sc.device(0.3, 1.0, 1), joint, 1e-4)


# ---------------------------------------------------------------------------------------------------- the full model
MODEL_SEED = 31
FRAMES = [150, 96, 56]
MAX_LEN_B = 6                            # caps of 6 tokens: at most 11 frames of the shortest sentence's 14 encoder rows


def _model(dtype=torch.float32, rounded=False):
    from simulst_amd.config import tiny
    from simulst_amd.model import S2TEmformerModel
    from simulst_amd.weights import init_model
    cfg = tiny(model="s2t_emformer", simul_attn_type="full", ctc_layer=True, mass_preservation=False)
    w = init_model(cfg, seed=MODEL_SEED)
    g = torch.Generator().manual_seed(MODEL_SEED + 1)
    W = torch.randn(cfg.vocab, cfg.embed_dim, generator=g) * cfg.embed_dim ** -0.5
    W[cfg.eos] *= 3.0
    w["decoder.output_projection.weight"] = W                     # untied (a tied random embedding repeats one token), EOS reachable
    w["encoder.ctc_layer.weight"] = torch.randn(cfg.vocab, cfg.embed_dim, generator=g) * 4.0 * cfg.embed_dim ** -0.5
    if rounded:
        w = {k: v.to(torch.bfloat16).float() for k, v in w.items()}
    fb = torch.randn(len(FRAMES), max(FRAMES), 80, generator=torch.Generator().manual_seed(MODEL_SEED + 2))
    if rounded:
        fb = fb.to(torch.bfloat16).float()
    T = torch.tensor(FRAMES)
    for b in range(len(FRAMES)):
        fb[b, FRAMES[b]:] = 0
    return cfg, w, S2TEmformerModel(cfg, w, device="cuda:0", dtype=dtype), fb, T


def _model_restatement(cfg, w, model, fb, T, beam, lenpen, lam, nbest):
    """fp64 decoder logits (tests/test_hip_s2t_decoder.py ref_logits) over the device encoder's rows, the oracle encoder's ctc_logits"""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from oracle import emformer as oem
    from oracle.configs import from_model_config
    from test_hip_s2t_decoder import ref_logits
    enc = model.encoder.forward(fb.to("cuda:0"), T)
    e, el = enc["encoder_out_btd"].float().cpu(), enc["encoder_lengths"].cpu()
    ecfg, _ = from_model_config(cfg)
    with torch.no_grad():
        ctc_logits = oem.encoder_forward(w, "encoder", ecfg, fb, T)["ctc_logits"][0]          # [B, Te, V]
    assert ctc_logits.shape[:2] == e.shape[:2]
    ctc_lp = torch.log_softmax(ctc_logits.double(), dim=-1)
    caps = [model.target_cap(int(t), 0.0, MAX_LEN_B) for t in T.tolist()]
    R = len(caps) * beam
    er, lr = e.repeat_interleave(beam, 0), el.repeat_interleave(beam)
    state = {"prefix": torch.full((R, 1), cfg.eos, dtype=torch.int64)}

    def logits_fn(t, toks):
        if t > 0:
            state["prefix"] = torch.cat([state["prefix"], toks.view(R, 1)], 1)
        return ref_logits(w, cfg, er, lr, state["prefix"]).float()

    def on_select(t, reorder):
        state["prefix"] = state["prefix"][reorder]

    ref, gaps = jr.joint_beam(logits_fn, jr.rows_of(ctc_lp, el), caps, beam, cfg.vocab, cfg.eos, cfg.padding_idx, lenpen, nbest, lam,
                              on_select=on_select)
    return ref, gaps, int(el.max())


@pytest.mark.parametrize("lenpen", [1.0, 0.6])
def test_full_model_against_the_restatement_fp32(lenpen):
    cfg, w, model, fb, T = _model()
    beam, lam = 4, 0.3
    ref, gaps, _ = _model_restatement(cfg, w, model, fb, T, beam, lenpen, lam, beam)
    for s in range(len(FRAMES)):
        assert min(gaps[s]) >= MIN_GAP, (s, min(gaps[s]))
        assert not any(h[3] for h in ref[s]), s                   # the floor applied to no returned hypothesis: scores of the size of 1
    got = model.generate(fb.to("cuda:0"), T, beam=beam, lenpen=lenpen, nbest=beam, max_len_a=0.0, max_len_b=MAX_LEN_B, ctc_weight=lam)
    for s in range(len(FRAMES)):
        assert [h["tokens"].tolist() for h in got[s]] == [h[0] for h in ref[s]], s
        for h, (rt, rs, rp, _) in zip(got[s], ref[s]):
            print(f"lenpen {lenpen} sentence {s}: score {float(h['score']):.6f} restated {rs:.6f}")
            assert abs(float(h["score"]) - rs) <= 1e-4, (s, float(h["score"]), rs)
            torch.testing.assert_close(h["positional_scores"].double(), rp, atol=1e-4, rtol=0)


def test_weight_zero_is_the_plain_search_bit_for_bit():
    cfg, w, model, fb, T = _model()
    a = model.generate(fb.to("cuda:0"), T, beam=4, nbest=4, max_len_a=0.0, max_len_b=MAX_LEN_B)
    b = model.generate(fb.to("cuda:0"), T, beam=4, nbest=4, max_len_a=0.0, max_len_b=MAX_LEN_B, ctc_weight=0.0)
    for ha, hb in zip(a, b):
        assert len(ha) == len(hb)
        for x, y in zip(ha, hb):
            assert torch.equal(x["tokens"], y["tokens"]) and torch.equal(x["score"], y["score"])
            assert torch.equal(x["positional_scores"], y["positional_scores"])
    with pytest.raises(ValueError):
        model.generate(fb.to("cuda:0"), T, beam=4, ctc_weight=1.5)
    from simulst_amd.config import tiny
    from simulst_amd.model import S2TEmformerModel
    from simulst_amd.weights import init_model
    bare = tiny(model="s2t_emformer", simul_attn_type="full", mass_preservation=False)
    with pytest.raises(ValueError, match="no CTC head"):
        S2TEmformerModel(bare, init_model(bare, seed=1), device="cuda:0").generate(fb.to("cuda:0"), T, beam=4, ctc_weight=0.3)


def test_score_is_the_weighted_sum_of_both_models():
    """score x len^lenpen = (1 - lam) x the decoder's log-probability of the hypothesis (score_reference) + lam x the head's CTC
    log-likelihood of it (score_ctc): the prefix-score ratios telescope.  Hypotheses on which the floor applied are skipped."""
    cfg, w, model, fb, T = _model()
    lam, lenpen, beam = 0.3, 1.0, 4
    ref, _, Te = _model_restatement(cfg, w, model, fb, T, beam, lenpen, lam, beam)
    got = model.generate(fb.to("cuda:0"), T, beam=beam, lenpen=lenpen, nbest=beam, max_len_a=0.0, max_len_b=MAX_LEN_B, ctc_weight=lam)
    skipped = 0
    for s in range(len(FRAMES)):
        for h, r in zip(got[s], ref[s]):
            if r[3]:
                skipped += 1
                continue
            toks = h["tokens"].tolist()
            n = len(toks)
            one = slice(s, s + 1)
            att = model.score_reference(fb[one].to("cuda:0"), T[one], [toks])[0]["positional_scores"].double().sum()
            nll = model.score_ctc(fb[one].to("cuda:0"), T[one], [toks[:-1]])[0]["nll"]
            want = (1 - lam) * float(att) + lam * -nll
            tol = n * 1e-4 + lam * (n + 1) * br.beam_bound(Te, nll)
            assert abs(float(h["score"]) * n ** lenpen - want) <= tol, (s, toks, float(h["score"]) * n ** lenpen, want, tol)
    assert skipped <= 1, skipped


def test_bf16_best_hypothesis_agreement():
    """bf16 path against the fp32 restatement on bf16-rounded weights: reported; asserted as loosely as the plain beam's bf16 test"""
    cfg, w, model, fb, T = _model(torch.bfloat16, rounded=True)
    f32 = _model(rounded=True)[2]
    ref, _, _ = _model_restatement(cfg, w, f32, fb, T, 4, 1.0, 0.3, 1)
    got = model.generate(fb.to("cuda:0"), T, beam=4, nbest=1, max_len_a=0.0, max_len_b=MAX_LEN_B, ctc_weight=0.3)
    n = len(FRAMES)
    first = sum(int(g[0]["tokens"][0]) == r[0][0][0] for g, r in zip(got, ref)) / n
    same = sum(g[0]["tokens"].tolist() == r[0][0] for g, r in zip(got, ref)) / n
    print(f"bf16 joint beam 4 best hypothesis: first token {first:.2f}, whole hypothesis {same:.2f}")
    assert first >= 0.5
