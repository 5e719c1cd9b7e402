"""The s2t_emformer model's decoder (fairseq's plain TransformerDecoder: cross-attention over every valid encoder row,
SIMULST_ATTN_FULL) on the MI355X, against the reference's own decoder (g23, tests/golden/gen_golden_s2t_emformer.py) and an fp64
restatement of the TransformerDecoder, on every path: per-op step, the device decode loop in its three row classes, the EOS-retiring
loop, beam search and a checkpoint file loaded through checkpoint.load.  GPU only."""
import argparse
import math
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G23 = os.path.join(ROOT, "tests", "golden", "g23_s2t_emformer.npz")
DEV = "cuda:0"


# ---------------------------------------------------------------------------------------------------------------- fp64 restatement
def ref_logits(w, cfg, enc, enc_len, prefix):
    """fairseq TransformerDecoder (pre-norm, GELU, sinusoidal positions, final LayerNorm) over the whole prefix [B, u] in fp64;
    logits of its last position.  enc [B, S, D] (rows >= enc_len[b] masked out of the cross-attention)."""
    from simulst_amd.decoder import sinusoidal_table
    g = lambda n: w[n].double().cpu()       # noqa: E731
    B, u = prefix.shape
    D, H = cfg.embed_dim, cfg.num_heads
    d = D // H
    enc = enc.double().cpu()
    S = enc.shape[1]
    tab = sinusoidal_table(cfg.padding_idx + u + 2, D, cfg.padding_idx).double()
    x = math.sqrt(D) * g("decoder.embed_tokens.weight")[prefix] + tab[cfg.padding_idx + 1 + torch.arange(u)].unsqueeze(0)

    def lin(n, t):
        b = w.get(n + ".bias")
        return t @ g(n + ".weight").t() + (0 if b is None else b.double().cpu())

    def ln(n, t):
        return torch.nn.functional.layer_norm(t, (D,), g(n + ".weight"), g(n + ".bias"), 1e-5)

    def heads(t):
        return t.view(B, -1, H, d).transpose(1, 2)

    causal = torch.triu(torch.full((u, u), -math.inf, dtype=torch.float64), 1)
    kmask = torch.where(torch.arange(S).unsqueeze(0) < torch.as_tensor(enc_len).cpu().view(B, 1), 0.0, -math.inf).double()
    for l in range(cfg.decoder_layers):
        p = f"decoder.layers.{l}"
        h = ln(p + ".self_attn_layer_norm", x)
        q, k, v = (heads(lin(f"{p}.self_attn.{n}_proj", h)) for n in "qkv")
        a = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d) + causal, -1) @ v
        x = x + lin(p + ".self_attn.out_proj", a.transpose(1, 2).reshape(B, u, D))
        h = ln(p + ".encoder_attn_layer_norm", x)
        q = heads(lin(p + ".encoder_attn.q_proj", h))
        k, v = heads(lin(p + ".encoder_attn.k_proj", enc)), heads(lin(p + ".encoder_attn.v_proj", enc))
        a = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d) + kmask.view(B, 1, 1, S), -1) @ v
        x = x + lin(p + ".encoder_attn.out_proj", a.transpose(1, 2).reshape(B, u, D))
        h = ln(p + ".final_layer_norm", x)
        x = x + lin(p + ".fc2", torch.nn.functional.gelu(lin(p + ".fc1", h)))
    x = ln("decoder.layer_norm", x)
    return x[:, -1] @ g("decoder.output_projection.weight").t()


def ref_greedy(w, cfg, enc, enc_len, n):
    """greedy over the fp64 restatement: pad never, EOS masked at the first step (SequenceGenerator min_len 1)"""
    B = enc.shape[0]
    prefix = torch.full((B, 1), cfg.eos, dtype=torch.int64)
    for t in range(n):
        lg = ref_logits(w, cfg, enc, enc_len, prefix)
        lg[:, cfg.padding_idx] = -math.inf
        if t == 0:
            lg[:, cfg.eos] = -math.inf
        prefix = torch.cat([prefix, lg.argmax(-1, keepdim=True)], 1)
    return prefix[:, 1:]


# ---------------------------------------------------------------------------------------------------------------- models / inputs
def g23():
    g = np.load(G23)
    args = {k[5:]: g[k].item() for k in g.files if k.startswith("args.")}
    w = {k[2:]: torch.from_numpy(g[k]).float() for k in g.files if k.startswith("w:")}
    from simulst_amd.checkpoint import config_from_args
    cfg = replace(config_from_args(dict(args, arch="s2t_emformer_s")), vocab=w["decoder.embed_tokens.weight"].shape[0])
    return g, args, cfg, w


def full_weights(cfg, seed=999, eos_scale=None):
    """random-init weights with an untied output projection (a tied random embedding repeats one token); eos_scale scales its EOS row"""
    from simulst_amd.weights import init_model
    w = init_model(cfg, seed=seed)
    W = torch.randn(cfg.vocab, cfg.embed_dim, generator=torch.Generator().manual_seed(seed + 1)) * cfg.embed_dim ** -0.5
    if eos_scale is not None:
        W[cfg.eos] *= eos_scale
    w["decoder.output_projection.weight"] = W
    return w


def ragged_enc(B, S, D, seed, one_row=True):
    """encoder states [B, S, D] with ragged lengths (the last row: a single encoder row)"""
    gen = torch.Generator().manual_seed(seed)
    enc = torch.randn(B, S, D, generator=gen)
    L = torch.randint(max(2, S // 3), S + 1, (B,), generator=gen)
    L[0] = S
    if one_row:
        L[-1] = 1
    for b in range(B):
        enc[b, int(L[b]):] = 0
    return enc, L.to(torch.int32)


def decoder(cfg, w, dtype=torch.float32):
    from simulst_amd.decoder import MMADecoder
    return MMADecoder(cfg, w, device=DEV, dtype=dtype)


def perop_logits(dec, enc, L, forced):
    """teacher-forced per-op steps: logits [n, B, V] of prefixes [eos] + forced[:, :t]"""
    B, n = forced.shape
    st = dec.new_state(B, cap=n + 8, S_cap=enc.shape[1])
    dec.append_encoder_out(st, enc.to(DEV, dec.dtype), L.to(DEV))
    toks = torch.full((B,), dec.cfg.eos, device=DEV, dtype=torch.int64)
    out = []
    for t in range(n):
        lg, act = dec.step(st, toks)
        assert act == 1
        out.append(lg.float().cpu())
        dec.commit(st)
        toks = forced[:, t].to(DEV)
    return torch.stack(out)


# ---------------------------------------------------------------------------------------------------------------- 1. per-op logits
def test_step_logits_g23():
    g, _, cfg, w = g23()
    dec = decoder(cfg, w)
    enc = torch.from_numpy(g["enc_out"]).transpose(0, 1).contiguous()
    L = torch.from_numpy(g["enc_len"]).to(torch.int32)
    forced = torch.from_numpy(g["forced"]).long()
    got = perop_logits(dec, enc, L, forced)
    want = torch.from_numpy(g["step_logits"])
    assert (got - want).abs().max().item() <= 1e-4
    for t in range(forced.shape[1]):
        prefix = torch.cat([torch.full((forced.shape[0], 1), cfg.eos), forced[:, :t]], 1)
        assert (got[t].double() - ref_logits(w, cfg, enc, L, prefix)).abs().max().item() <= 1e-4, t


@pytest.mark.parametrize("S", [200, 700])
def test_step_logits_full_dims(S):
    """s2t_emformer_s dims, ragged enc_len with a 1-row source, sources of <= 256 and > 256 keys"""
    from simulst_amd.config import s2t_emformer_s
    cfg = s2t_emformer_s()
    w = full_weights(cfg)
    enc, L = ragged_enc(4, S, cfg.embed_dim, seed=S)
    forced = torch.randint(4, cfg.vocab, (4, 4), generator=torch.Generator().manual_seed(7))
    got = perop_logits(decoder(cfg, w), enc, L, forced)
    for t in range(forced.shape[1]):
        prefix = torch.cat([torch.full((4, 1), cfg.eos), forced[:, :t]], 1)
        assert (got[t].double() - ref_logits(w, cfg, enc, L, prefix)).abs().max().item() <= 1e-4, t


# ---------------------------------------------------------------------------------------------------------------- 2. fused loop
@pytest.mark.parametrize("B,S", [(64, 120), (64, 300), (448, 250), (448, 300), (1100, 120)])
def test_fused_equals_perop_fp32(B, S):
    from simulst_amd.config import s2t_emformer_s
    cfg = s2t_emformer_s()
    w = full_weights(cfg)
    enc, L = ragged_enc(B, S, cfg.embed_dim, seed=B + S)
    dec = decoder(cfg, w)
    a, _ = dec.greedy_offline(enc.to(DEV), L.to(DEV), 6, mask_eos=False, fused=True)
    a = a.cpu()
    b, _ = dec.greedy_offline(enc.to(DEV), L.to(DEV), 6, mask_eos=False, fused=False)
    assert torch.equal(a, b.cpu())


def test_fused_vs_perop_bf16_agreement():
    """bf16: the fused loop and the per-op steps round in different places; measured agreement is asserted against a bound"""
    from simulst_amd.config import s2t_emformer_s
    cfg = s2t_emformer_s()
    w = full_weights(cfg)
    agree = []
    for B, S in ((64, 250), (448, 300)):
        enc, L = ragged_enc(B, S, cfg.embed_dim, seed=3 * B + S)
        dec = decoder(cfg, w, torch.bfloat16)
        a, _ = dec.greedy_offline(enc.to(DEV, torch.bfloat16), L.to(DEV), 8, mask_eos=False, fused=True)
        a = a.cpu()
        b, _ = dec.greedy_offline(enc.to(DEV, torch.bfloat16), L.to(DEV), 8, mask_eos=False, fused=False)
        agree.append((a[:, :4] == b.cpu()[:, :4]).all(1).float().mean().item())
    print("bf16 fused vs per-op: rows with the first 4 tokens identical", agree)
    assert min(agree) >= 0.9, agree


# ---------------------------------------------------------------------------------------------------------------- 3. wait-k anchor
def test_anchor_waitk_beyond_source():
    """wait-k with lagging >= S, no pre-decision, no mass preservation attends to every key of a >= 2-row source: FULL must match it"""
    from simulst_amd.config import s2t_emformer_s
    from simulst_amd.model import SimulSTModel
    cfg = s2t_emformer_s(decoder_layers=3)
    w = full_weights(cfg, seed=11)
    for B, S in ((8, 40), (8, 300), (200, 100)):
        enc, L = ragged_enc(B, S, cfg.embed_dim, seed=B * S, one_row=False)
        cw = replace(cfg, model="mma_model", simul_attn_type="waitk", waitk_lagging=S + 8, mass_preservation=False)
        full, wk = decoder(cfg, w), decoder(cw, w)
        forced = torch.randint(4, cfg.vocab, (B, 3), generator=torch.Generator().manual_seed(B))
        a, b = perop_logits(full, enc, L, forced), perop_logits(wk, enc, L, forced)
        assert (a - b).abs().max().item() <= 1e-5
        ta, _ = full.greedy_offline(enc.to(DEV), L.to(DEV), 6, mask_eos=False)
        ta = ta.cpu()
        tb, _ = wk.greedy_offline(enc.to(DEV), L.to(DEV), 6, mask_eos=False)
        assert torch.equal(ta, tb.cpu()), (B, S)
    # beam: the two models over the same encoder output
    enc, L = ragged_enc(4, 60, cfg.embed_dim, seed=5, one_row=False)
    ms = [SimulSTModel(c, w, device=DEV) for c in (cfg, replace(cfg, model="mma_model", simul_attn_type="waitk", waitk_lagging=80,
                                                                  mass_preservation=False))]
    outs = [m.decoder.beam_offline(enc.to(DEV), L.to(DEV), 8, beam=4, nbest=2)[0].cpu() for m in ms]
    assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------------------------- 4. EOS retiring
def test_generate_offline_stop_at_eos():
    from simulst_amd.config import s2t_emformer_s
    cfg = s2t_emformer_s()
    w = full_weights(cfg, seed=21, eos_scale=6.0)
    B, S = 160, 200
    enc, L = ragged_enc(B, S, cfg.embed_dim, seed=22)
    caps = [int(x) for x in torch.randint(8, 20, (B,), generator=torch.Generator().manual_seed(23))]
    for dtype in (torch.float32, torch.bfloat16):
        dec = decoder(cfg, w, dtype)
        full, _ = dec.greedy_offline(enc.to(DEV, dtype), L.to(DEV), max(caps), mask_eos=False)
        full = full.cpu()
        hyp, lengths, _ = dec.generate_offline(enc.to(DEV, dtype), L.to(DEV), caps, stop_at_eos=True)
        hyp, lengths = hyp.cpu(), lengths.cpu()
        ended = 0
        for b in range(B):
            row = full[b, :caps[b]].tolist()
            n = row.index(cfg.eos) + 1 if cfg.eos in row else caps[b]
            ended += n < caps[b] or cfg.eos in row
            assert hyp[b, :n].tolist() == row[:n] and int(lengths[b]) == n, b
            assert (hyp[b, n:] == cfg.padding_idx).all(), b
        assert ended >= B // 8, ended                    # the EOS path is exercised


# ---------------------------------------------------------------------------------------------------------------- 5. beam search
def test_beam_vs_cpu_restatement():
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_hip_beam import cpu_beam
    from simulst_amd.config import tiny
    from simulst_amd.model import S2TEmformerModel
    cfg = tiny(model="s2t_emformer", simul_attn_type="full", mass_preservation=False)
    w = full_weights(cfg, seed=31, eos_scale=3.0)
    model = S2TEmformerModel(cfg, w, device=DEV)
    fb = torch.randn(3, 150, 80, generator=torch.Generator().manual_seed(32))
    T = torch.tensor([150, 96, 40])
    for b in range(3):
        fb[b, int(T[b]):] = 0
    enc = model.encoder.forward(fb.to(DEV), T)
    e, el = enc["encoder_out_btd"].float().cpu(), enc["encoder_lengths"].cpu()
    caps = [min(int(0.1 * t + 10), cfg.max_target_positions - 1) for t in T.tolist()]
    beam = 5
    R = 3 * beam
    er, lr = e.repeat_interleave(beam, 0), el.repeat_interleave(beam)
    state = {"prefix": torch.full((R, 1), cfg.eos, dtype=torch.int64)}

    def logits_fn(t, toks):
        if t > 0:
            state["prefix"] = torch.cat([state["prefix"], toks.view(R, 1)], 1)
        return ref_logits(w, cfg, er, lr, state["prefix"]).float()

    def on_select(t, reorder):
        state["prefix"] = state["prefix"][reorder]

    ref, gaps = cpu_beam(logits_fn, caps, beam, cfg.vocab, cfg.eos, cfg.padding_idx, 1.0, 1, on_select)
    got = model.generate(fb.to(DEV), T, beam=beam, lenpen=1.0, nbest=1, max_len_a=0.1, max_len_b=10)
    checked = 0
    for s in range(3):
        if min(gaps[s]) < 1e-4:                          # a near-tie fp32 may resolve the other way
            continue
        checked += 1
        assert got[s][0]["tokens"].cpu().tolist() == ref[s][0][0], s
        assert abs(float(got[s][0]["score"]) - ref[s][0][1]) <= 1e-4
    assert checked >= 2
    # beam 1 = greedy with EOS appended
    g1 = model.generate(fb.to(DEV), T, beam=1, nbest=1)
    hyp, lengths, _ = model.decoder.generate_offline(enc["encoder_out_btd"], enc["encoder_lengths"], caps, stop_at_eos=True)
    for s in range(3):
        h = hyp[s, :int(lengths[s])].cpu().tolist()
        if h[-1] != cfg.eos:
            h.append(cfg.eos)
        assert g1[s][0]["tokens"].cpu().tolist() == h, s


# ---------------------------------------------------------------------------------------------------------------- 6. checkpoint file
def test_checkpoint_load_decodes_full_attention(tmp_path):
    """an s2t_emformer_s checkpoint through checkpoint.load decodes with full attention (before this model had its own attention
    type it resolved onto mma_model_s and decoded as wait-k 3 over windows of 8 encoder rows)"""
    from simulst_amd import checkpoint
    from simulst_amd.weights import init_model
    g, args, cfg, wd = g23()
    sd = init_model(cfg, seed=5)
    sd.update(wd)
    p = str(tmp_path / "checkpoint_asr.pt")
    checkpoint.save_fairseq_layout(p, dict(args, arch="s2t_emformer_s"), sd)
    model = checkpoint.load(p, device=DEV)
    assert type(model).__name__ == "S2TEmformerModel" and model.cfg.attn_type == "full"
    enc = torch.from_numpy(g["enc_out"]).transpose(0, 1).contiguous()
    L = torch.from_numpy(g["enc_len"]).to(torch.int32)
    want = torch.from_numpy(g["greedy"]).long()
    n = want.shape[1]
    toks, _ = model.decoder.greedy_offline(enc.to(DEV), L.to(DEV), n, mask_eos=False)
    assert torch.equal(toks.cpu(), want)
    toks, _ = model.decoder.greedy_offline(enc.to(DEV), L.to(DEV), n, mask_eos=False, fused=False)
    assert torch.equal(toks.cpu(), want)
    assert torch.equal(ref_greedy(sd, cfg, enc, L, n), want)
    # the whole model: encoder + generate_offline / generate against the fp64 decoder over the device encoder's output
    fb = torch.randn(2, 160, 80, generator=torch.Generator().manual_seed(40))
    T = torch.tensor([160, 70])
    fb[1, 70:] = 0
    e = model.encoder.forward(fb.to(DEV), T)
    eo, el = e["encoder_out_btd"].float().cpu(), e["encoder_lengths"].cpu()
    n = int(0.1 * 160 + 10)
    toks, _ = model.generate_offline(fb.to(DEV), T, n_steps=n, mask_eos=False)
    ref = ref_greedy(sd, cfg, eo, el, n)
    assert torch.equal(toks.cpu(), ref)
    hyps = model.generate(fb.to(DEV), T, beam=1)
    for s in range(2):
        r = ref[s].tolist()
        cap = int(0.1 * int(T[s]) + 10)
        r = r[:r.index(cfg.eos) + 1] if cfg.eos in r[:cap] else r[:cap] + [cfg.eos]
        assert hyps[s][0]["tokens"].cpu().tolist() == r, s


# ---------------------------------------------------------------------------------------------------------------- 7. refusals
def test_agents_refuse_offline_model():
    from simulst_amd.agent import BatchedStreamingAgent, FairseqSimulSTAgent
    from simulst_amd.config import tiny
    from simulst_amd.model import S2TEmformerModel
    from simulst_amd.simuleval_agent import FairseqSimulSTAgent as SimulEvalAgent
    cfg = tiny(model="s2t_emformer", simul_attn_type="full", mass_preservation=False)
    model = S2TEmformerModel(cfg, full_weights(cfg), device=DEV)
    torch.cuda.synchronize()
    for make in (lambda: FairseqSimulSTAgent(model), lambda: BatchedStreamingAgent(model),
                 lambda: SimulEvalAgent(argparse.Namespace(), model=model)):
        with pytest.raises(ValueError, match="full attention"):
            make()
