"""The layers above simulst_emformer_attention at a segment geometry of more than 128 keys per segment: the quality end of the
latency sweep, --segment-length 256 --segment-left-context 256 --segment-right-context 32 --max-memory-size 5, that is
S = 64, Lc = 64, R = 8, M = 5 encoder rows: 141 keys and 73 queries per segment (the blocked kernels of emformer_attn_tiled.hip).

fp32, tiny dims (embed 32, 2 heads, 2 layers): encoder.forward and encoder.infer against the oracle, streaming == offline, the
stream row schedule, and one policy model per attention type through config_from_args -> generate_offline, the B = 1 agent and
BatchedStreamingAgent.run_batch.  Tolerances are those of the existing fp32 comparisons: forward vs oracle atol 2e-4 / rtol 1e-3
(test_hip_kernels.py::test_encoder_forward_full_size_vs_oracle), infer vs oracle atol 1e-4 / rtol 1e-3
(test_hip_streaming.py::test_g11_streaming_encoder_golden), streaming vs offline atol = rtol = 1e-3
(test_hip_properties.py::test_full_size_streaming_equals_offline_fp32).

bf16, model dims (D 256, 4 heads of 64, 4 layers: the tiled MFMA form in every layer): offline forward and lockstep streaming
against the fp64 oracle on bf16-rounded weights under the four bars of test_hip_encoder_oracle.py, with that module's bf16
emulation and its rule (a missed bar is a bug or a rounding the emulation must gain, never a larger factor).  Both batches hold
more than 2 000 valid frames; at that count the emulation's own max / mean and worst-utterance ratios, measured on the CPU, are
1.29 and 1.30 offline (2 091 frames) and 1.32 and 1.32 streaming (2 200 frames): a few percent under the 1.35 and 1.36 that
module's docstring gives for ~10^4 frames (the maximum of fewer frames is smaller), which makes bars (b) and (c) slightly
tighter here, not looser.
"""
import contextlib
import math
from dataclasses import replace

import pytest
import torch

from oracle import emformer as oem
from test_hip_encoder_oracle import (assert_bars, bar_stats, bf16_emulation, oracle_forward, read_schedule, _fbank, _w64,
                                     BIAS_FACTOR, LOC_FACTOR, MAX_FACTOR, MEAN_FACTOR)

GEOMETRY = dict(segment_length=256, segment_left_context=256, segment_right_context=32, max_memory_size=5)
TINY = dict(conv_channels=64, encoder_embed_dim=32, encoder_ffn_embed_dim=64, encoder_attention_heads=2, encoder_layers=2,
            decoder_layers=2, conv_pos=16, conv_pos_groups=4, fixed_pre_decision_ratio=2, max_target_positions=24)
FBANK_LENGTHS = [1100, 1030, 515, 260, 17]
FWD_TOL = dict(atol=2e-4, rtol=1e-3)
INFER_TOL = dict(atol=1e-4, rtol=1e-3)
STREAM_TOL = dict(atol=1e-3, rtol=1e-3)
# bf16 batches: more than 2 000 valid encoder frames each
BF16_LENGTHS = [1100, 1030, 1003, 999, 900, 800, 777, 640, 515, 311, 260, 17]
BF16_STREAM_T, BF16_STREAMS = 1100, 8

assert (MEAN_FACTOR, MAX_FACTOR, LOC_FACTOR, BIAS_FACTOR) == (1.5, 2.0, 2.5, 6.0)


def tiny_cfg(**kw):
    """The tiny model through the checkpoint's argument surface: the four geometry flags are plain model args."""
    from simulst_amd.checkpoint import config_from_args
    cfg = config_from_args({"arch": "mma_model_s", **TINY, **GEOMETRY, **kw})
    return replace(cfg, vocab=64)


def test_geometry_is_beyond_the_all_keys_kernels():
    cfg = tiny_cfg()
    assert (cfg.S, cfg.Lc, cfg.R, cfg.M) == (64, 64, 8, 5)
    assert cfg.M + cfg.R + cfg.Lc + cfg.S == 141 > 128
    c192 = tiny_cfg(segment_left_context=192)
    assert c192.M + c192.R + c192.Lc + c192.S == 125 <= 128


def _chunks(cfg, T):
    return read_schedule(T, first=(cfg.S + cfg.R) * cfg.stride, nxt=cfg.S * cfg.stride)


def _hip_stream(enc, fb):
    """encoder.infer over the agent's READ schedule -> concatenated rows [B, T_e, D] and the row count after every call."""
    inc, outs, counts, total = {}, [], [], 0
    B = fb.size(0)
    for pos, fin in _chunks(enc.cfg, fb.size(1)):
        o = enc.infer(fb[:, :pos], torch.full((B,), pos), inc, finish=fin)["encoder_out_btd"]
        outs.append(o)
        total += o.size(1)
        counts.append(total)
    torch.cuda.synchronize()
    return torch.cat(outs, 1), counts


def _oracle_stream(w, ecfg, cfg, fb_1t, dtype=torch.float32, emulate=None):
    """oracle.encoder_infer over one utterance [1, T, 80] on the same schedule -> [T_e, D]."""
    ctx = bf16_emulation(emulate) if emulate is not None else contextlib.nullcontext()
    dt = torch.get_default_dtype()
    st, outs = oem.new_encoder_state(), []
    torch.set_default_dtype(dtype)                    # init_layer_state's zero states
    try:
        with torch.no_grad(), ctx:
            for pos, fin in _chunks(cfg, fb_1t.size(1)):
                o = oem.encoder_infer(w, "encoder", ecfg, fb_1t[:, :pos].to(dtype), torch.tensor([pos]), st, fin)
                outs.append(o["encoder_out"][0][:, 0])
    finally:
        torch.set_default_dtype(dt)
    return torch.cat(outs, 0)


@pytest.fixture(scope="module")
def ops():
    from simulst_amd.ops import Ops
    return Ops()


# ------------------------------------------------------------------ fp32, tiny dims: the encoder
@pytest.fixture(scope="module")
def tiny_enc():
    """cfg, weights, oracle cfg, the ragged fbank batch and the oracle's offline forward over it."""
    from oracle.configs import from_model_config
    from simulst_amd.weights import init_model
    cfg = tiny_cfg()
    w = init_model(cfg, seed=999)
    ecfg, _ = from_model_config(cfg)
    fb = torch.randn(len(FBANK_LENGTHS), max(FBANK_LENGTHS), 80, generator=torch.Generator().manual_seed(1100))
    for b, n in enumerate(FBANK_LENGTHS):
        fb[b, n:] = 0
    L = torch.tensor(FBANK_LENGTHS)
    with torch.no_grad():
        ref = oem.encoder_forward(w, "encoder", ecfg, fb, L)
    return dict(cfg=cfg, w=w, ecfg=ecfg, fb=fb, L=L, ref=ref)


@pytest.mark.gpu
def test_encoder_forward_vs_oracle_fp32(ops, tiny_enc):
    from simulst_amd.encoder import S2TEmformerEncoder
    t = tiny_enc
    enc = S2TEmformerEncoder(t["cfg"], t["w"], dtype=torch.float32, ops=ops)
    out = enc.forward(t["fb"].cuda(), t["L"])
    ref = t["ref"]["encoder_out"][0]
    assert torch.equal(out["encoder_padding_mask"][0].cpu(), t["ref"]["encoder_padding_mask"][0])
    y = out["encoder_out"][0].cpu()
    assert y.shape == ref.shape and y.size(0) == 275                      # 5 segments of 64 rows: 4 memory rows at the last
    for b in range(len(FBANK_LENGTHS)):
        n = int(out["encoder_lengths"][b])
        assert n == -(-FBANK_LENGTHS[b] // 4)
        torch.testing.assert_close(y[:n, b], ref[:n, b], **FWD_TOL)


@pytest.mark.gpu
def test_encoder_infer_vs_oracle_and_offline_fp32(ops, tiny_enc):
    """Chunk by chunk against oracle.encoder_infer, each utterance alone (first chunk 288 frames = 72 rows, then 256 = 64 rows,
    then the flush); the streamed rows equal the offline forward's; stream_row_schedule predicts every call's row count."""
    from simulst_amd.encoder import S2TEmformerEncoder
    t = tiny_enc
    enc = S2TEmformerEncoder(t["cfg"], t["w"], dtype=torch.float32, ops=ops)
    off = enc.forward(t["fb"].cuda(), t["L"])["encoder_out_btd"]
    for b, n in enumerate(FBANK_LENGTHS):
        fb = t["fb"][b:b + 1, :n]
        ref = _oracle_stream(t["w"], t["ecfg"], t["cfg"], fb)
        got, counts = _hip_stream(enc, fb.cuda())
        assert got.shape[1:] == ref.shape, (n, got.shape, ref.shape)
        torch.testing.assert_close(got[0].cpu(), ref, **INFER_TOL)
        torch.testing.assert_close(got[0], off[b, :got.size(1)], **STREAM_TOL)
        assert counts == enc.stream_row_schedule([pos for pos, _ in _chunks(t["cfg"], n)]), n
        assert counts[-1] == -(-n // 4)


@pytest.mark.gpu
def test_streaming_batch_in_lockstep_equals_offline_fp32(ops, tiny_enc):
    """T = 1100 as test_full_size_streaming_equals_offline_fp32 does it, two streams in lockstep."""
    from simulst_amd.encoder import S2TEmformerEncoder
    t = tiny_enc
    enc = S2TEmformerEncoder(t["cfg"], t["w"], dtype=torch.float32, ops=ops)
    fb = torch.randn(2, 1100, 80, generator=torch.Generator().manual_seed(999)).cuda()
    off = enc.forward(fb, torch.tensor([1100, 1100]))["encoder_out_btd"]
    st, _ = _hip_stream(enc, fb)
    assert st.shape == off.shape == (2, 275, 32)
    torch.testing.assert_close(st, off, **STREAM_TOL)


@pytest.mark.gpu
def test_more_left_context_is_attended_not_clamped(ops, tiny_enc):
    """segment_left_context 192 (125 keys: the all-keys VALU kernel) against 256 (141 keys: the blocked kernel), same weights and
    input: the outputs differ as the oracle's do.  Rows of the first segment have no left context in either."""
    from oracle.configs import from_model_config
    from simulst_amd.encoder import S2TEmformerEncoder
    t = tiny_enc
    c192 = tiny_cfg(segment_left_context=192)
    with torch.no_grad():
        ref192 = oem.encoder_forward(t["w"], "encoder", from_model_config(c192)[0], t["fb"], t["L"])["encoder_out"][0]
    ref256 = t["ref"]["encoder_out"][0]
    y = {}
    for name, cfg in (("192", c192), ("256", t["cfg"])):
        enc = S2TEmformerEncoder(cfg, t["w"], dtype=torch.float32, ops=ops)
        y[name] = enc.forward(t["fb"].cuda(), t["L"])["encoder_out"][0].cpu()
    n = 275                                                                   # utterance 0 is whole
    d_ref, d_hip = (ref256 - ref192)[:n, 0], (y["256"] - y["192"])[:n, 0]
    # segments 0 .. 2 (rows < 192) see the same keys under both settings up to the memory they carry; from row 192 on Lc = 48
    # drops keys that Lc = 64 attends
    assert float(d_ref[192:].abs().max()) > 100 * FWD_TOL["atol"]
    assert float(d_hip[192:].abs().max()) > 100 * FWD_TOL["atol"]
    torch.testing.assert_close(d_hip, d_ref, atol=2 * FWD_TOL["atol"], rtol=FWD_TOL["rtol"])


# ------------------------------------------------------------------ fp32, tiny dims: policy models
@pytest.mark.gpu
@pytest.mark.parametrize("attn,kw", [("waitk_fixed_pre_decision", dict(waitk_lagging=3)), ("hard_aligned_fixed_pre_decision", {})])
def test_policy_model_offline_and_agents_identical_to_oracle(ops, attn, kw):
    """config_from_args with the four geometry flags -> model -> generate_offline, the B = 1 agent and the batched agent, with no
    further argument: tokens, READ / WRITE actions and delays identical to the oracle's (the pattern of
    test_hip_streaming.py::test_agent_actions_tokens_al_identical_to_oracle)."""
    from oracle import agent as oag
    from oracle.configs import from_model_config
    from simulst_amd.agent import BatchedStreamingAgent, FairseqSimulSTAgent
    from simulst_amd.model import SimulSTModel
    from simulst_amd.weights import init_model
    cfg = tiny_cfg(simul_attn_type=attn, **kw)
    w = init_model(cfg, seed=999)
    # an untied output projection: with the tied random embedding a tiny model repeats one token (as in the smoke run)
    w["decoder.output_projection.weight"] = torch.randn(cfg.vocab, cfg.embed_dim,
                                                        generator=torch.Generator().manual_seed(5)) * cfg.embed_dim ** -0.5
    if "waitk" not in attn:
        for l in range(cfg.decoder_layers):
            w[f"decoder.layers.{l}.encoder_attn.q_proj.weight"] = w[f"decoder.layers.{l}.encoder_attn.q_proj.weight"] * 8
    ecfg, dcfg = from_model_config(cfg)
    model = SimulSTModel(cfg, w, dtype=torch.float32, ops=ops)
    lengths = [1100, 777, 515]
    fb = torch.randn(3, 1100, 80, generator=torch.Generator().manual_seed(1999))
    for b, n in enumerate(lengths):
        fb[b, n:] = 0
    L = torch.tensor(lengths)
    ref_toks, _, _ = oag.greedy_offline(w, ecfg, dcfg, fb, L, n_steps=10, mask_eos=True)
    toks, _ = model.generate_offline(fb.cuda(), L, n_steps=10, mask_eos=True)
    assert torch.equal(toks.cpu(), ref_toks), (attn, toks.cpu(), ref_toks)
    assert len(set(ref_toks.flatten().tolist())) >= 4, "degenerate hypothesis"
    agent = FairseqSimulSTAgent(model)
    singles = []
    for b, n in enumerate(lengths):
        ref = oag.simulate_mma(w, ecfg, dcfg, fb[b, :n])
        got = agent.run_utterance(fb[b, :n].cuda())
        for k in ("actions", "tokens", "delays_ms", "AL", "n_enc"):
            assert got[k] == ref[k], (attn, n, k)
        assert "R" in ref["actions"] and "W" in ref["actions"]
        singles.append(got)
    batch = BatchedStreamingAgent(model).run_batch(fb[:, :777])
    for b in range(3):
        one = singles[b] if lengths[b] == 777 else agent.run_utterance(fb[b, :777].cuda())
        for k in ("actions", "tokens", "delays_ms", "AL"):
            assert batch[b][k] == one[k], (attn, b, k)


# ------------------------------------------------------------------ bf16, model dims
def bf16_model():
    from oracle.configs import from_model_config
    from simulst_amd.checkpoint import config_from_args
    from simulst_amd.weights import init_model
    cfg = config_from_args({"arch": "mma_model_s", "encoder_layers": 4, **GEOMETRY})
    assert (cfg.embed_dim, cfg.num_heads, cfg.head_dim) == (256, 4, 64)
    w = {k: v.to(torch.bfloat16).float() for k, v in init_model(cfg, seed=999).items() if k.startswith("encoder.")}
    return cfg, w, from_model_config(cfg)[0]


def bf16_offline_case(cfg, w, ecfg):
    fb = _fbank(BF16_LENGTHS, seed=2560)
    ref, pad = oracle_forward(w, ecfg, fb, BF16_LENGTHS)
    # below fuse_ffn_min_rows the feed-forward is two launches: fc2 adds its residual in fp32 and rounds once
    emu, _ = oracle_forward(w, ecfg, fb, BF16_LENGTHS, emulate=False)
    enc_len = (~pad).sum(1)
    return dict(fb=fb, ref=ref, pad=pad, enc_len=enc_len, emu=bar_stats(emu, ref, enc_len))


def bf16_stream_case(cfg, w, ecfg):
    fb = _fbank([BF16_STREAM_T] * BF16_STREAMS, seed=2561)
    w64 = _w64(w)
    ref = torch.stack([_oracle_stream(w64, ecfg, cfg, fb[i:i + 1], torch.float64) for i in range(BF16_STREAMS)])
    emu = torch.stack([_oracle_stream(w64, ecfg, cfg, fb[i:i + 1], torch.float64, emulate=False) for i in range(BF16_STREAMS)])
    lens = [ref.size(1)] * BF16_STREAMS
    return dict(fb=fb, ref=ref, lens=lens, emu=bar_stats(emu, ref, lens))


@pytest.fixture(scope="module")
def model_bf16():
    return bf16_model()


@pytest.mark.gpu
def test_offline_bf16_model_dims_vs_fp64_oracle(ops, model_bf16):
    from simulst_amd.encoder import S2TEmformerEncoder
    cfg, w, ecfg = model_bf16
    case = bf16_offline_case(cfg, w, ecfg)
    assert int(case["enc_len"].sum()) >= 2000
    Te = case["pad"].size(1)
    enc = S2TEmformerEncoder(cfg, w, dtype=torch.bfloat16, ops=ops)
    assert len(BF16_LENGTHS) * (math.ceil(Te / cfg.S) * cfg.R + Te) < enc.fuse_ffn_min_rows       # the two-launch feed-forward
    out = enc.forward(case["fb"].to(torch.bfloat16).cuda(), torch.as_tensor(BF16_LENGTHS).cuda())
    torch.cuda.synchronize()
    assert torch.equal(out["encoder_padding_mask"][0].cpu(), case["pad"])
    assert torch.equal(out["encoder_lengths"].cpu(), case["enc_len"])
    y = out["encoder_out_btd"]
    assert torch.isfinite(y).all()
    assert_bars(bar_stats(y, case["ref"], case["enc_len"]), case["emu"], "offline 12 utterances, 141 keys per segment")


@pytest.mark.gpu
def test_streaming_lockstep_bf16_model_dims_vs_fp64_oracle(ops, model_bf16):
    from simulst_amd.encoder import S2TEmformerEncoder
    cfg, w, ecfg = model_bf16
    case = bf16_stream_case(cfg, w, ecfg)
    assert sum(case["lens"]) >= 2000
    enc = S2TEmformerEncoder(cfg, w, dtype=torch.bfloat16, ops=ops)
    y, _ = _hip_stream(enc, case["fb"].to(torch.bfloat16).cuda())
    assert y.shape == case["ref"].shape
    assert_bars(bar_stats(y, case["ref"], case["lens"]), case["emu"], f"streaming {BF16_STREAMS} lockstep, 141 keys per segment")
