"""The whole-target (teacher-forced) decoder pass on the GPU: MMADecoder.forward without an incremental_state against the reference's
own outputs (g24), against the step path fed the same tokens (wait-k, full attention; fp32 and bf16), the three kernels alone against
torch, SimulSTModel.score_reference, and the link to the latency loss.  The CPU restatement and its cases live in
tests/test_teacher_forced_oracle.py."""
import math
from types import SimpleNamespace

import pytest
import torch

from oracle import monotonic as mono
from oracle.configs import from_model_config
from test_teacher_forced_oracle import (BF16_ATOL, BF16_RTOL, FULL_CASES, G24_VARIANTS, WAITK_CASES, g24_case, make_case,
                                        safe_margin_mask, whole_target_forward)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from simulst_amd.ops import Ops
    return Ops()


def _encoder_out(enc, pad):
    return {"encoder_out": [enc.cuda()], "encoder_padding_mask": [pad.cuda()]}


# ------------------------------------------------------------------ the forward against the reference's own outputs
@pytest.mark.parametrize("name,extra", G24_VARIANTS)
def test_forward_equals_reference_fp32(ops, name, extra):
    from simulst_amd.decoder import MMADecoder
    a, tag, cfg, w, tokens, enc, enc_len, pad = g24_case(name, extra)
    dec = MMADecoder(cfg, w, dtype=torch.float32, ops=ops)
    logits, extra_out = dec.forward(tokens.cuda(), _encoder_out(enc, pad))
    assert extra_out["action"] == 1 and extra_out["attn"] == [None] and len(extra_out["attn_list"]) == cfg.decoder_layers
    assert logits.dtype == torch.float32 and tuple(logits.shape) == (3, 9, cfg.vocab)
    print(f"{tag}: max |logits - g24| = {(logits.cpu() - a[f'{tag}.logits']).abs().max().item():.3e}")
    for i, at in enumerate(extra_out["attn_list"]):
        for k in ("p_choose", "alpha", "beta"):
            got, want = at[k].cpu(), a[f"{tag}.l{i}.{k}"]
            assert got.dtype == torch.float32 and got.shape == want.shape
            for b in range(3):                       # keys beyond the row's source length are excluded
                n = int(enc_len[b])
                print(f"{tag} layer {i} {k} row {b}: max diff {(got[b, :, :, :n] - want[b, :, :, :n]).abs().max().item():.3e}")
                torch.testing.assert_close(got[b, :, :, :n], want[b, :, :, :n], atol=1e-5, rtol=1e-4)
                if k == "alpha" and cfg.mass_preservation:
                    # mass preservation adds 1 - clamp(sum, 0, 1): a row the recurrence left ABOVE one stays there.  Every source
                    # position multiplies the running product by (1 - p + eps), so a row can exceed one by n * eps (the
                    # reference's own rows of this fixture do, by 1.2e-5); the elementwise bound covers the fp32 summation
                    torch.testing.assert_close(got[b, :, :, :n].sum(-1), torch.ones(cfg.num_heads, 9),
                                               atol=1e-5 + n * cfg.attention_eps, rtol=0)
    torch.testing.assert_close(logits.cpu(), a[f"{tag}.logits"], atol=2e-4, rtol=1e-3)
    feats, _ = dec.forward(tokens.cuda(), _encoder_out(enc, pad), features_only=True)
    assert tuple(feats.shape) == (3, 9, cfg.embed_dim)


# ------------------------------------------------------------------ the forward against the step path on the same tokens
STEP_CASES = list(WAITK_CASES) + list(FULL_CASES)


def _step_logits(dec, tokens, enc, enc_len):
    """decoder.step + decoder.commit fed the reference tokens, 'online' unset -> logits [B, U, V]"""
    B, U = tokens.shape
    st = dec.new_state(B, cap=U + 2, S_cap=enc.size(0))
    dec.append_encoder_out(st, enc.to(device=dec.device, dtype=dec.dtype).transpose(0, 1).contiguous(), enc_len)
    toks = tokens.cuda()
    rows = []
    for u in range(U):
        logits, action = dec.step(st, toks[:, u].contiguous())
        assert action == 1
        rows.append(logits.clone())
        dec.commit(st)
    return torch.stack(rows, 1)


@pytest.mark.parametrize("case", STEP_CASES, ids=lambda c: f"{c[0]}-r{c[2]}-S{c[3]}")
def test_forward_equals_step_path_fp32(ops, case):
    from simulst_amd.decoder import MMADecoder
    cfg, w, tokens, enc, enc_len, pad = make_case(case)
    dec = MMADecoder(cfg, w, dtype=torch.float32, ops=ops)
    whole, extra = dec.forward(tokens.cuda(), _encoder_out(enc, pad))
    steps = _step_logits(dec, tokens, enc, enc_len)
    print(f"{case[0]} S={case[3]} fp32: max |whole - step| = {(whole - steps).abs().max().item():.3e}")
    torch.testing.assert_close(whole, steps, atol=1e-4, rtol=1e-4)
    if case[0] == "full":
        assert extra["attn_list"] == [None] * cfg.decoder_layers
    # and the CPU restatement, alignments included
    ref, ref_attn = whole_target_forward(w, from_model_config(cfg)[1], tokens, enc, pad)
    torch.testing.assert_close(whole.cpu(), ref, atol=2e-4, rtol=1e-3)
    if case[0] != "full":
        for b, n in enumerate(case[4]):
            for k in ("p_choose", "alpha", "beta"):
                torch.testing.assert_close(extra["attn_list"][0][k][b, :, :, :n].cpu(), ref_attn[0][k][b, :, :, :n].float(),
                                           atol=1e-5, rtol=1e-4)


@pytest.mark.parametrize("case", STEP_CASES, ids=lambda c: f"{c[0]}-r{c[2]}-S{c[3]}")
def test_forward_equals_step_path_bf16(ops, case):
    """bf16: the project's bound between two bf16 forms of a step, and the same argmax wherever the fp32 top-2 margin exceeds what
    that bound lets two logits move (at least 90 % of the positions: tests/test_teacher_forced_oracle.py checks the seeds on the CPU
    restatement, the fp32 reference of the margin)."""
    from simulst_amd.decoder import MMADecoder
    cfg, w, tokens, enc, enc_len, pad = make_case(case)
    dec = MMADecoder(cfg, w, dtype=torch.bfloat16, ops=ops)
    whole, _ = dec.forward(tokens.cuda(), _encoder_out(enc, pad))
    steps = _step_logits(dec, tokens, enc, enc_len)
    assert whole.dtype == torch.float32
    print(f"{case[0]} S={case[3]} bf16: max |whole - step| = {(whole - steps).abs().max().item():.3e}")
    torch.testing.assert_close(whole, steps, atol=BF16_ATOL, rtol=BF16_RTOL)
    ref, _ = whole_target_forward(w, from_model_config(cfg)[1], tokens, enc, pad)
    safe = safe_margin_mask(ref)
    print(f"{case[0]} S={case[3]} bf16: {100 * safe.float().mean().item():.1f} % decisive positions")
    assert safe.float().mean().item() >= 0.9
    assert torch.equal(whole.cpu().argmax(-1)[safe], ref.argmax(-1)[safe])
    assert torch.equal(steps.cpu().argmax(-1)[safe], ref.argmax(-1)[safe])


# ------------------------------------------------------------------ the three kernels alone against torch
# fp32: products on the fp32 matrix-core path, sums of <= 64 (scores) or S (context) terms of magnitude ~1: a few 1e-6.
# bf16: operands are exact in the reference (it reads the bf16 values); what differs is P / beta / pooled keys rounded to bf16 before
# the second product (2^-9 relative each) and the bf16 store (2^-9 relative): 0.02 absolute + 2^-7 relative covers |values| <= 4.
TOL = {torch.float32: dict(atol=2e-5, rtol=2e-5), torch.bfloat16: dict(atol=0.02, rtol=2 ** -7)}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("U,d", [(1, 64), (7, 64), (64, 64), (65, 64), (300, 64), (1024, 64), (65, 16)])
def test_causal_self_attention_kernel(ops, U, d, dtype):
    B, H = 2, 2
    D = H * d
    g = torch.Generator().manual_seed(U + d)
    qkv = torch.randn(B, U, 3 * D, generator=g).to(dtype)
    got = ops.decoder_self_attention_causal(qkv.cuda(), H=H).float().cpu()
    q, k, v = [t.double().view(B, U, H, d).transpose(1, 2) for t in qkv.split(D, dim=-1)]
    s = q @ k.transpose(-1, -2) * d ** -0.5 + torch.triu(torch.full((U, U), float("-inf"), dtype=torch.float64), 1)
    want = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, U, D).float()
    print(f"causal U={U} d={d} {dtype}: max diff {(got - want).abs().max().item():.3e}")
    torch.testing.assert_close(got, want, **TOL[dtype])


S_SET = (3, 8, 9, 17, 250, 750)


def _kv(B, H, S, d, dtype, seed):
    """a head-major cache with S_cap > S rows, the rows behind S poisoned (never read)"""
    g = torch.Generator().manual_seed(seed)
    K = torch.full((B, H, S + 5, d), float("nan"))
    K[:, :, :S] = torch.randn(B, H, S, d, generator=g)
    return K.to(dtype)


# ratio < 0: 'last' pooling with ratio |ratio| (the entry point rejects it for S < |ratio|)
ENERGY_CASES = [(S, r) for r in (1, 8, 4) for S in S_SET] + [(S, -4) for S in (8, 9, 17)] + [(17, 2)]
# head dim of a case (default 64).  24: head_dim^-0.5 is no power of two, so a query scaled BEFORE it is rounded to bf16 for the
# product would carry a second rounding; the kernel scales the fp32 energies instead (csrc/teacher_forced.hip)
ENERGY_HEAD_DIM = {(17, 2): 24}


def _pool(x, ratio):
    """x [N, S, C] pooled over S as the padded batch is in a training-mode forward: oracle.monotonic's own pooling"""
    if abs(ratio) == 1:
        return x
    cfg = SimpleNamespace(pre_decision_ratio=abs(ratio), pre_decision_type="average" if ratio > 0 else "last")
    return mono.pool_keys(x.transpose(0, 1), cfg).transpose(0, 1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("S,ratio", ENERGY_CASES)
def test_energy_kernel(ops, S, ratio, dtype):
    from simulst_amd import _lib
    B, H, d, U = 2, 2, ENERGY_HEAD_DIM.get((S, ratio), 64), 70
    D = H * d
    g = torch.Generator().manual_seed(S * 10 + ratio)
    q = torch.randn(B, U, D, generator=g).to(dtype)
    K = _kv(B, H, S, d, dtype, S)
    key_len = torch.tensor([S, max(1, (2 * S) // 3)], dtype=torch.int32)
    qh = q.double().view(B, U, H, d).transpose(1, 2).reshape(B * H, U, d) * d ** -0.5
    Kh = K[:, :, :S].double().reshape(B * H, S, d)
    # soft: raw energies of all keys, padded ones included
    got = ops.mma_energy(q.cuda(), K.cuda(), mode=_lib.ENERGY_SOFT, S=S, key_len=key_len.cuda()).cpu()
    want = (qh @ Kh.transpose(1, 2)).float()
    print(f"soft energy S={S} {dtype}: max diff {(got - want).abs().max().item():.3e}")
    torch.testing.assert_close(got, want, atol=TOL[dtype]["atol"] * 2, rtol=TOL[dtype]["rtol"])
    if d != 64 and dtype == torch.bfloat16:
        # the soft energies carry NO bf16 rounding: the operands are exact in the reference and the products accumulate in fp32, each of
        # the d additions erring by <= 2^-24 of a partial sum <= sum |q_i k_i| ~ d, i.e. <= d^2 2^-24 d^-0.5 ~ 7e-6 after the scale.  A
        # query rounded after scaling would err by ~2^-9 |energy| ~ 2e-3: 1e-4 lies a decade from both.
        torch.testing.assert_close(got, want, atol=1e-4, rtol=0)
    # monotonic: pooled keys (ceil, no trim), bias, pooled padding mask (0.3, first column never), sigmoid, zero insertion + tail
    bias = -0.5
    pooled = _pool(Kh, ratio)
    pad = (torch.arange(S).unsqueeze(0) >= key_len.unsqueeze(1)).float()
    mp = _pool(pad.unsqueeze(-1), ratio).squeeze(-1) > 0.3
    mp[:, 0] = False
    e = qh @ pooled.transpose(1, 2) + bias
    e = e.masked_fill(mp.repeat_interleave(H, 0).unsqueeze(1), -1e8)
    pp = torch.sigmoid(e)
    want = mono.insert_zeros(pp, abs(ratio))[:, :, :S].clone()
    want[:, :, -1] = pp[:, :, -1]
    got = ops.mma_energy(q.cuda(), K.cuda(), mode=_lib.ENERGY_MONOTONIC, S=S, key_len=key_len.cuda(), ratio=ratio, energy_bias=bias).cpu()
    print(f"monotonic p_choose S={S} ratio={ratio} {dtype}: max diff {(got - want.float()).abs().max().item():.3e}")
    torch.testing.assert_close(got, want.float(), **TOL[dtype])
    # wait-k's diagonal over the same pooled mask
    k = 3
    got = ops.mma_energy(None, K.cuda(), mode=_lib.ENERGY_WAITK, S=S, B=B, U=U, key_len=key_len.cuda(), ratio=ratio, waitk_k=k).cpu()
    P = pp.size(-1)
    last = (~mp).sum(1) - 1
    step = torch.minimum(torch.arange(U).unsqueeze(0) + k - 1, last.unsqueeze(1))                       # [B, U]
    onehot = (torch.arange(P).view(1, 1, P) == step.unsqueeze(-1)).double().repeat_interleave(H, 0)
    want = mono.insert_zeros(onehot, abs(ratio))[:, :, :S].clone()
    want[:, :, -1] = onehot[:, :, -1]
    assert torch.equal(got, want.float())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("S", S_SET)
def test_context_kernel(ops, S, dtype):
    B, H, d, U = 2, 2, 64, 70
    g = torch.Generator().manual_seed(S)
    beta = torch.softmax(torch.randn(B * H, U, S, generator=g) * 2, -1)
    V = _kv(B, H, S, d, dtype, S + 1)
    got = ops.mma_context(beta.cuda(), V.cuda()).float().cpu()
    want = (beta.to(dtype).double() @ V[:, :, :S].double().reshape(B * H, S, d)).view(B, H, U, d).transpose(1, 2).reshape(B, U, H * d)
    print(f"context S={S} {dtype}: max diff {(got - want.float()).abs().max().item():.3e}")
    torch.testing.assert_close(got, want.float(), **TOL[dtype])


def test_softmax_kernel(ops):
    B, H, U, S = 2, 2, 5, 300
    e = torch.randn(B * H, U, S, generator=torch.Generator().manual_seed(3)) * 3
    key_len = torch.tensor([300, 77], dtype=torch.int32)
    got = ops.mma_softmax(e.clone().cuda(), key_len.cuda(), H=H).cpu()
    pad = (torch.arange(S).unsqueeze(0) >= key_len.unsqueeze(1)).repeat_interleave(H, 0).unsqueeze(1)
    want = torch.softmax(e.masked_fill(pad, float("-inf")), -1)
    torch.testing.assert_close(got, want, atol=1e-6, rtol=1e-5)


# ------------------------------------------------------------------ score_reference
@pytest.fixture(scope="module")
def scoring_model():
    from simulst_amd.config import tiny
    from simulst_amd.model import SimulSTModel
    from simulst_amd.weights import init_model
    cfg = tiny(waitk_lagging=3)
    w = init_model(cfg, seed=999)
    w["decoder.output_projection.weight"] = torch.randn(cfg.vocab, cfg.embed_dim,
                                                        generator=torch.Generator().manual_seed(5)) * cfg.embed_dim ** -0.5
    return cfg, SimulSTModel(cfg, w, device="cuda:0", dtype=torch.float32)


def test_score_reference_scores_are_the_forward_log_probs(scoring_model):
    cfg, model = scoring_model
    fb = torch.randn(2, 200, 80, generator=torch.Generator().manual_seed(999))
    L = torch.tensor([200, 200])
    g = torch.Generator().manual_seed(6)
    targets = [torch.randint(4, cfg.vocab, (8,), generator=g).tolist() + [cfg.eos], torch.randint(4, cfg.vocab, (4,), generator=g).tolist() + [cfg.eos]]
    hyps = model.score_reference(fb.cuda(), L, targets, return_alignments=True)
    enc = model.encoder.forward(fb.cuda(), L)
    prev = torch.full((2, 9), cfg.padding_idx)
    for b, t in enumerate(targets):
        prev[b, :len(t)] = torch.tensor([cfg.eos] + t[:-1])
    logits, extra = model.decoder.forward(prev.cuda(), enc)
    lp = torch.log_softmax(logits, -1).cpu()
    for b, t in enumerate(targets):
        h = hyps[b]
        assert set(h) == {"tokens", "score", "positional_scores", "alignment", "attention", "alpha"}
        assert h["tokens"].tolist() == t and h["alignment"] is None and h["attention"] is None
        want = lp[b, torch.arange(len(t)), torch.tensor(t)]
        torch.testing.assert_close(h["positional_scores"], want, atol=1e-6, rtol=1e-6)
        torch.testing.assert_close(h["score"], h["positional_scores"].mean(), atol=1e-6, rtol=1e-6)
        n_src = int(enc["encoder_lengths"][b])
        assert len(h["alpha"]) == cfg.decoder_layers and tuple(h["alpha"][0].shape) == (cfg.num_heads, len(t), n_src)
        torch.testing.assert_close(h["alpha"][1], extra["attn_list"][1]["alpha"][b, :, :len(t), :n_src].cpu())
        # ragged targets in one batch: each sentence gets the result it gets alone
        alone = model.score_reference(fb[b:b + 1].cuda(), L[b:b + 1], [t])[0]
        assert "alpha" not in alone
        torch.testing.assert_close(h["positional_scores"], alone["positional_scores"], atol=1e-4, rtol=0)
        torch.testing.assert_close(h["score"], alone["score"], atol=1e-4, rtol=0)


def test_score_reference_reproduces_greedy_choices(scoring_model):
    """the tokens generate_offline(stop_at_eos=True) produced for a wait-k model, scored in one pass: at every position the scored
    token is the argmax greedy took (its log-probability is the position's maximum over the vocabulary, padding excluded)"""
    cfg, model = scoring_model
    fb = torch.randn(2, 200, 80, generator=torch.Generator().manual_seed(999))
    L = torch.tensor([200, 137])
    fb[1, 137:] = 0
    enc = model.encoder.forward(fb.cuda(), L)
    toks, lengths, _ = model.decoder.generate_offline(enc["encoder_out_btd"], enc["encoder_lengths"], [10, 10], stop_at_eos=True)
    toks, lengths = toks.cpu(), lengths.cpu()
    targets = []
    for b in range(2):
        t = toks[b, :int(lengths[b])].tolist()
        targets.append(t if t[-1] == cfg.eos else t + [cfg.eos])
    assert len(set(toks.flatten().tolist())) >= 4, "degenerate hypothesis"
    hyps = model.score_reference(fb.cuda(), L, targets)
    prev = torch.full((2, max(len(t) for t in targets)), cfg.padding_idx)
    for b, t in enumerate(targets):
        prev[b, :len(t)] = torch.tensor([cfg.eos] + t[:-1])
    logits, _ = model.decoder.forward(prev.cuda(), enc)
    lp = torch.log_softmax(logits.cpu(), -1)
    lp[:, :, cfg.padding_idx] = -math.inf           # greedy never picks padding, and no EOS at the first position
    lp[:, 0, cfg.eos] = -math.inf
    for b in range(2):
        n = int(lengths[b])
        assert lp[b, :n].argmax(-1).tolist() == toks[b, :n].tolist()
        torch.testing.assert_close(hyps[b]["positional_scores"][:n], lp[b, :n].max(-1).values, atol=1e-6, rtol=1e-6)


# ------------------------------------------------------------------ link to the losses
def test_latency_loss_on_the_forward_alignments(ops):
    from simulst_amd.decoder import MMADecoder
    from simulst_amd.losses import mma_latency_loss
    name, extra = "infinite_lookback_fixed_pre_decision", {}
    a, tag, cfg, w, tokens, enc, enc_len, pad = g24_case(name, extra)
    dec = MMADecoder(cfg, w, dtype=torch.float32, ops=ops)
    _, out = dec.forward(tokens.cuda(), _encoder_out(enc, pad))
    _, ref_attn = whole_target_forward(w, from_model_config(cfg)[1], tokens, enc, pad)
    tpm = torch.zeros(3, 9, dtype=torch.bool).cuda()
    kw = dict(latency_avg_weight=0.1, latency_var_weight=0.1)
    got = mma_latency_loss([x["alpha"] for x in out["attn_list"]], tpm, pad.cuda(), enc_len.cuda() * 4, **kw)
    want = mma_latency_loss([x["alpha"].float().cuda().contiguous() for x in ref_attn], tpm, pad.cuda(), enc_len.cuda() * 4, **kw)
    for g_, w_ in zip(got, want):
        print(f"latency loss term: {float(g_):.6f} vs {float(w_):.6f}")
        torch.testing.assert_close(g_, w_, rtol=1e-4, atol=0)
