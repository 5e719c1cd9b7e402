"""The CTC head's surface on the MI355X: S2TEmformerEncoder.ctc_greedy, transcribe_ctc, ctc_report on the device's path, and the
streaming agents of simulst_amd/ctc_agent.py, against the fp64 pick (tests/ctc_ref.py) and the Python collapse over the encoder's OWN
output rows and head weights.  Tiny cif_transformer and s2t_emformer models with the head, fp32 and bf16.  GPU only.

The pick rule is that of test_hip_ctc_pick.py: e = 2 x the largest |fp32 - fp64| of the logits simulst_linear writes with
SIMULST_EPI_BIAS_F32OUT for the same rows; a frame whose fp64 top-2 margin is <= 2e is unclear, and an utterance is compared token by
token up to its first unclear frame."""
import pytest
import torch

import ctc_ref as cr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENGTHS = [333, 40, 200, 97]
BLANK = 0
FWD_KEYS = {"encoder_out", "encoder_padding_mask", "encoder_embedding", "encoder_states", "src_tokens", "src_lengths", "ctc_logits",
            "encoder_out_btd", "encoder_lengths"}
CIF_KEYS = {"cif_out", "cif_out_btd", "cif_lengths", "alpha", "delays", "alpha_sum", "tail_weights"}


def _build(kind, dtype):
    from simulst_amd.config import tiny
    from simulst_amd.weights import init_model
    if kind == "cif":
        from simulst_amd.cif import CIFTransformerModel
        cfg = tiny(model="cif_transformer", ctc_layer=True, simul_attn_type="none")
        return CIFTransformerModel(cfg, init_model(cfg, seed=31), device=DEV, dtype=dtype)
    from simulst_amd.model import S2TEmformerModel
    cfg = tiny(model="s2t_emformer", simul_attn_type="full", mass_preservation=False, ctc_layer=True)
    return S2TEmformerModel(cfg, init_model(cfg, seed=32), device=DEV, dtype=dtype)


_MODELS = {}


def _get(kind, dtype):
    if (kind, dtype) not in _MODELS:
        _MODELS[(kind, dtype)] = _build(kind, dtype)
    return _MODELS[(kind, dtype)]


@pytest.fixture(params=[("cif", torch.float32), ("cif", torch.bfloat16), ("s2t", torch.float32), ("s2t", torch.bfloat16)],
                ids=["cif-fp32", "cif-bf16", "s2t-fp32", "s2t-bf16"])
def model(request):
    return _get(*request.param)


def _fbank():
    g = torch.Generator().manual_seed(77)
    fb = torch.randn(len(LENGTHS), max(LENGTHS), 80, generator=g)
    for b, n in enumerate(LENGTHS):
        fb[b, n:] = 0
    return fb, torch.tensor(LENGTHS)


def _reference(model, rows):
    """rows [n, D] (device, model dtype) -> (fp64 logits of the head over them, the measured bound e)"""
    from simulst_amd._lib import EPI_BIAS_F32OUT
    rows = rows.contiguous()
    z = cr.logits64(rows, model.encoder.w.ctc)
    e = 2 * float((model.ops.linear(rows, model.encoder.w.ctc, epilogue=EPI_BIAS_F32OUT).cpu().double() - z).abs().max())
    return z, e


def _first_unclear(z, e):
    _, _, _, margin = cr.pick64(z)
    bad = (margin <= 2 * e).nonzero()
    return int(bad[0]) if bad.numel() else z.size(0)


def _upto(tokens, frames, limit):
    return [(t, f) for t, f in zip(tokens, frames) if f < limit]


def test_ctc_greedy_against_fp64_and_python_collapse(model):
    fb, L = _fbank()
    enc = model.encoder.forward(fb.to(DEV), L)
    rows, enc_len = enc["encoder_out_btd"], enc["encoder_lengths"]
    g = model.encoder.ctc_greedy(rows, enc_len, blank=BLANK)
    torch.cuda.synchronize()
    B, Te = rows.shape[:2]
    assert g["path"].shape == g["lprob"].shape == (B, Te) and g["path"].dtype == torch.int32 and g["lprob"].dtype == torch.float32
    assert g["score"].shape == g["n"].shape == (B,) and g["tokens"].shape == g["frames"].shape
    path, lprob, tokens, frames = g["path"].cpu(), g["lprob"].cpu().double(), g["tokens"].cpu(), g["frames"].cpu()
    compared = 0
    for b in range(B):
        n = int(enc_len[b])
        assert bool((path[b, n:] == BLANK).all()) and bool((lprob[b, n:] == 0).all())          # rows past the length: blank, in no count
        z, e = _reference(model, rows[b, :n])
        cr.check_pick(z, path[b, :n], e, f"utterance {b}")
        ref, zmax64, lse64, _ = cr.pick64(z)
        lp64 = z.gather(1, path[b, :n].long().unsqueeze(1)).squeeze(1) - lse64
        assert float(((lprob[b, :n] - lp64).abs() - 1e-6 * lse64.abs()).max()) <= 2 * e
        assert abs(float(g["score"][b]) - float(lprob[b, :n].sum())) <= 1e-5 * max(1.0, abs(float(lprob[b, :n].sum())))
        u = _first_unclear(z, e)
        want = _upto(*cr.collapse_loop(ref.tolist(), n, BLANK), u)
        k = int(g["n"][b])
        got = _upto(tokens[b, :k].tolist(), frames[b, :k].tolist(), u)
        assert got == want and len(want) > 0, b
        assert bool((tokens[b, k:] == model.cfg.padding_idx).all())
        # the device's own path collapses to what ctc_greedy returned, whole
        assert cr.collapse_loop(path[b].tolist(), n, BLANK) == (tokens[b, :k].tolist(), frames[b, :k].tolist())
        compared += len(want)
    assert compared >= 50


def test_forward_is_unchanged_and_transcribe_agrees(model):
    fb, L = _fbank()
    enc = model.encoder.forward(fb.to(DEV), L)
    assert set(enc) == (FWD_KEYS | CIF_KEYS if model.cfg.model == "cif_transformer" else FWD_KEYS) and len(enc["ctc_logits"]) == 1
    rows = enc["encoder_out_btd"]
    B, Te, D = rows.shape
    # what forward() has always launched for the head, on the same rows: bit for bit
    again = model.ops.linear(rows.reshape(B * Te, D), model.encoder.w.ctc).view(B, Te, -1)
    assert enc["ctc_logits"][0].dtype == model.dtype and torch.equal(enc["ctc_logits"][0], again)
    g = model.encoder.ctc_greedy(rows, enc["encoder_lengths"])
    hyps = model.transcribe_ctc(fb.to(DEV), L)
    stride = model.encoder.conv_layer_stride()
    assert len(hyps) == B
    for b, h in enumerate(hyps):
        k = int(g["n"][b])
        assert set(h) == {"tokens", "score", "frames", "frames_ms"}
        assert h["tokens"] == g["tokens"][b, :k].tolist() and h["frames"] == g["frames"][b, :k].tolist()
        assert h["frames_ms"] == [f * stride * 10 for f in h["frames"]] and h["score"] == float(g["score"][b])


def test_report_equals_the_composition_in_fp32():
    """ctc_report on the kernel's path against the same report on ctc_logits.argmax(-1) (the reference's y_pred), frames with an unclear
    margin blanked on both sides"""
    from simulst_amd.ctc import ctc_report
    model = _get("cif", torch.float32)
    fb, L = _fbank()
    enc = model.encoder.forward(fb.to(DEV), L)
    rows, enc_len = enc["encoder_out_btd"], enc["encoder_lengths"]
    g = model.encoder.ctc_greedy(rows, enc_len)
    composed = enc["ctc_logits"][0].argmax(-1)
    B, Te = composed.shape
    z, e = _reference(model, rows.reshape(B * Te, -1))
    _, _, _, margin = cr.pick64(z)
    clear = (margin > 2 * e).view(B, Te).to(DEV)
    assert float(clear.float().mean()) > 0.99
    a = torch.where(clear, g["path"].long(), torch.zeros_like(composed))
    c = torch.where(clear, composed, torch.zeros_like(composed))
    target = torch.randint(2, model.cfg.vocab, (B, 9), generator=torch.Generator().manual_seed(5))
    target[1, 4:] = model.cfg.padding_idx
    ra, rc = ctc_report(a, enc_len, target, BLANK, model.cfg.padding_idx), ctc_report(c, enc_len, target, BLANK, model.cfg.padding_idx)
    assert all(float(ra[k]) == float(rc[k]) for k in ("recall", "precision", "blank_rate")) and float(ra["recall"]) > 0
    assert torch.equal(torch.where(clear & (torch.arange(Te, device=DEV).unsqueeze(0) < enc_len.to(DEV).unsqueeze(1)), composed, a), a)


def test_a_model_without_the_head_raises():
    from simulst_amd.config import tiny
    from simulst_amd.ctc_agent import BatchedCTCStreamingAgent, CTCAgent
    from simulst_amd.model import SimulSTModel
    from simulst_amd.weights import init_model
    cfg = tiny(waitk_lagging=3)
    assert not cfg.ctc_layer
    m = SimulSTModel(cfg, init_model(cfg, seed=3), device=DEV, dtype=torch.float32)
    fb, L = _fbank()
    enc = m.encoder.forward(fb[:2].to(DEV), L[:2])
    assert enc["ctc_logits"] == []
    with pytest.raises(ValueError, match="no CTC head"):
        m.encoder.ctc_greedy(enc["encoder_out_btd"], enc["encoder_lengths"])
    with pytest.raises(ValueError, match="no CTC head"):
        m.transcribe_ctc(fb[:2].to(DEV), L[:2])
    for cls in (CTCAgent, BatchedCTCStreamingAgent):
        with pytest.raises(ValueError, match="no CTC head"):
            cls(m)


def _check_stream_record(model, agent, rec, states, T):
    """tokens / frames = the collapse over ALL rows the head saw; delays = the READ that released each token's first row"""
    n = states.size(0)
    z, e = _reference(model, states)
    ref, _, _, _ = cr.pick64(z)
    u = _first_unclear(z, e)
    want = _upto(*cr.collapse_loop(ref.tolist(), n, BLANK), u)
    assert rec["tokens"][-1] == model.cfg.eos and rec["frames"][-1] == n and len(rec["tokens"]) == len(rec["frames"]) == len(rec["delays_ms"])
    assert _upto(rec["tokens"][:-1], rec["frames"][:-1], u) == want and len(want) > 0
    positions = agent._chunk_positions(T)
    released = model.encoder.stream_row_schedule(positions)
    assert released[-1] == n
    elapsed = [p * 10 + 15 for p in positions]
    for f, d in zip(rec["frames"][:-1], rec["delays_ms"][:-1]):
        assert d == elapsed[next(i for i, r in enumerate(released) if r > f)]
    assert rec["delays_ms"][-1] == elapsed[-1]
    writes = [sum(1 for f in rec["frames"][:-1] if (released[i - 1] if i else 0) <= f < released[i]) for i in range(len(positions))]
    writes[-1] += 1                                                                   # EOS, when the source ends
    assert rec["actions"] == "".join("R" + "W" * w for w in writes)
    from simulst_amd.latency import average_lagging
    assert rec["AL"] == average_lagging(rec["delays_ms"], T * 10 + 15)
    return ref, u, released


def test_streaming_agent_equals_the_collapse_over_the_rows_it_saw(model):
    from simulst_amd.ctc_agent import CTCAgent
    fb, _ = _fbank()
    T = 333
    utt = fb[0, :T].to(DEV)
    agent = CTCAgent(model, blank=BLANK)
    rec, states = agent.run_utterance(utt, return_states=True)
    ref, u, released = _check_stream_record(model, agent, rec, states, T)
    assert len(released) >= 4 and rec["actions"].count("R") == len(released)
    plain = agent.run_utterance(utt)
    assert plain == rec
    # a run that crosses a chunk boundary: the winner of the last row of the first chunk is made to win the next chunk's first row too,
    # by adding a multiple of that row to the winner's head weights
    t0 = released[0] - 1
    assert t0 + 1 < u, "the boundary rows are clear"
    head = model.encoder.w.ctc
    keep = head.clone()
    try:
        z = cr.logits64(states, head)
        c = int(ref[t0]) if int(ref[t0]) != BLANK else int(z[t0, 1:].argmax()) + 1
        for _ in range(8):                                                            # (both rows: a lift of one moves the other a little)
            z = cr.logits64(states, head)
            need = [t for t in (t0, t0 + 1) if int(z[t].argmax()) != c or float(z[t].topk(2).values[0] - z[t].topk(2).values[1]) < 1.0]
            if not need:
                break
            y = states[need[0]].float()
            lift = float(z[need[0]].max() - z[need[0], c]) + 3.0
            head[c] = (head[c].float() + lift * y / float(y.double().dot(y.double()))).to(head.dtype)
        rec2, states2 = agent.run_utterance(utt, return_states=True)
        assert torch.equal(states2, states)
        ref2, u2, _ = _check_stream_record(model, agent, rec2, states2, T)
        assert t0 + 1 < u2 and int(ref2[t0]) == int(ref2[t0 + 1]) == c != BLANK
        assert (c, t0 + 1) not in zip(rec2["tokens"], rec2["frames"])                # written once, at the run's first row
        first = t0
        while first > 0 and int(ref2[first - 1]) == c:
            first -= 1
        assert (c, first) in zip(rec2["tokens"], rec2["frames"])
    finally:
        head.copy_(keep)


def test_batched_agent_rows_equal_the_single_stream_in_fp32():
    from simulst_amd.ctc_agent import BatchedCTCStreamingAgent, CTCAgent
    model = _get("s2t", torch.float32)
    g = torch.Generator().manual_seed(78)
    fb = torch.randn(3, 230, 80, generator=g).to(DEV)
    batched = BatchedCTCStreamingAgent(model)
    recs, states = batched.run_batch(fb, lengths=[230, 230, 230], return_states=True)
    single = CTCAgent(model)
    for b in range(3):
        rec, st = single.run_utterance(fb[b], return_states=True)
        assert recs[b] == rec, b
        assert torch.equal(states[b], st)
    with pytest.raises(ValueError, match="equal length"):
        batched.run_batch(fb, lengths=[230, 200, 230])
