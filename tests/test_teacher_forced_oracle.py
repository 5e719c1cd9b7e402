"""The yardstick of the whole-target (teacher-forced) decoder pass, on the CPU: a restatement of MMADecoder.forward without an
incremental_state (models/mma_model.py:156-220), composed from oracle.monotonic.attention_forward(state=None) and oracle.decoder's
_lin / _ln / sinusoidal_table plus a causal self-attention and the layer plumbing.  It equals the reference's own outputs
(tests/golden/g24_mma_teacher_forced.npz) for the learned policies, and for wait-k -- which the reference cannot run this way -- the
step path of oracle.decoder.mma_decoder_step run position by position.  tests/test_hip_teacher_forced_forward.py holds the HIP path
to this restatement."""
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, split_weights
from oracle import decoder as odec
from oracle import monotonic as mono
from oracle.configs import from_model_config

G24_VARIANTS = (("hard_aligned_fixed_pre_decision", {}),
                ("infinite_lookback_fixed_pre_decision", {}),
                ("hard_aligned", {"mass_preservation": False}),
                ("chunkwise", {"mocha_chunk_size": 3}),
                ("infinite_lookback", {}))


def tag_of(name, extra):
    return name + ("" if not extra else "." + ".".join(f"{k}={v}" for k, v in extra.items()))


def _causal_self_attn(w, p, cfg, x):
    """fairseq MultiheadAttention over the whole target with buffered_future_mask: softmax in fp32, no key padding mask."""
    U, B, D = x.shape
    H, hd = cfg.num_heads, D // cfg.num_heads
    q = (odec._lin(w, p + ".q_proj", x) * hd ** -0.5).contiguous().view(U, B * H, hd).transpose(0, 1)
    k = odec._lin(w, p + ".k_proj", x).contiguous().view(U, B * H, hd).transpose(0, 1)
    v = odec._lin(w, p + ".v_proj", x).contiguous().view(U, B * H, hd).transpose(0, 1)
    s = torch.bmm(q, k.transpose(1, 2)) + torch.triu(torch.full((U, U), float("-inf")), 1)
    a = torch.softmax(s.float(), dim=-1).type_as(q)
    o = torch.bmm(a, v).transpose(0, 1).contiguous().view(U, B, D)
    return odec._lin(w, p + ".out_proj", o)


def _full_cross_attn(w, p, cfg, x, enc, enc_pad):
    """fairseq MultiheadAttention as encoder-decoder attention (the s2t_emformer decoder): softmax over the valid keys in fp32"""
    U, B, D = x.shape
    S, H, hd = enc.size(0), cfg.num_heads, D // cfg.num_heads
    q = (odec._lin(w, p + ".q_proj", x) * hd ** -0.5).contiguous().view(U, B * H, hd).transpose(0, 1)
    k = odec._lin(w, p + ".k_proj", enc).contiguous().view(S, B * H, hd).transpose(0, 1)
    v = odec._lin(w, p + ".v_proj", enc).contiguous().view(S, B * H, hd).transpose(0, 1)
    s = torch.bmm(q, k.transpose(1, 2))
    if enc_pad is not None:
        s = s.masked_fill(enc_pad.repeat_interleave(H, 0).unsqueeze(1), float("-inf"))
    o = torch.bmm(torch.softmax(s.float(), dim=-1).type_as(q), v).transpose(0, 1).contiguous().view(U, B, D)
    return odec._lin(w, p + ".out_proj", o), None


def whole_target_forward(w, cfg, tokens, enc, enc_pad, p="decoder"):
    """tokens [B, U] ([eos] + target[:-1]), enc [S, B, D], enc_pad [B, S] bool or None -> (logits [B, U, V], attn_list)."""
    B, U = tokens.shape
    table = odec.sinusoidal_table(cfg.padding_idx + 1 + U + 1, cfg.embed_dim, cfg.padding_idx)
    pos = table[cfg.padding_idx + 1:cfg.padding_idx + 1 + U]
    x = cfg.embed_scale * F.embedding(tokens, w[p + ".embed_tokens.weight"], cfg.padding_idx) + pos.unsqueeze(0)
    x = x.transpose(0, 1)
    attn_list = []
    for i in range(cfg.num_layers):
        lp = f"{p}.layers.{i}"
        x = x + _causal_self_attn(w, lp + ".self_attn", cfg, odec._ln(w, lp + ".self_attn_layer_norm", x))
        y = odec._ln(w, lp + ".encoder_attn_layer_norm", x)
        if cfg.attn.attn_type == "full":
            h, attn = _full_cross_attn(w, lp + ".encoder_attn", cfg, y, enc, enc_pad)
        else:
            h, attn = mono.attention_forward(w, lp + ".encoder_attn", cfg.attn, y, enc, enc, enc_pad, None)
        x = x + h
        h = odec._ln(w, lp + ".final_layer_norm", x)
        x = x + odec._lin(w, lp + ".fc2", F.gelu(odec._lin(w, lp + ".fc1", h)))
        attn_list.append(attn)
    x = odec._ln(w, p + ".layer_norm", x).transpose(0, 1)
    return F.linear(x, w[p + ".output_projection.weight"]), attn_list


def step_by_step_logits(w, cfg, tokens, enc, enc_pad, p="decoder"):
    """the same tokens through oracle.decoder.mma_decoder_step position by position, 'online' unset -> logits [B, U, V]"""
    st = odec.new_decoder_state(cfg)
    eo = {"encoder_out": [enc], "encoder_padding_mask": [enc_pad] if enc_pad is not None else []}
    rows = []
    for u in range(1, tokens.size(1) + 1):
        x, extra = odec.mma_decoder_step(w, p, cfg, tokens[:, :u], eo, st)
        assert extra["action"] == 1
        rows.append(x[:, -1])
    return torch.stack(rows, 1)


def g24_case(name, extra):
    from simulst_amd.config import tiny
    a, _ = load_golden("g24_mma_teacher_forced")
    tag = tag_of(name, extra)
    cfg = tiny(simul_attn_type=name, mass_preservation=extra.get("mass_preservation", True),
               mocha_chunk_size=extra.get("mocha_chunk_size", 0))
    enc_len = a[f"{tag}.enc_len"].long()
    enc = a[f"{tag}.enc"]
    pad = torch.arange(enc.size(0)).unsqueeze(0) >= enc_len.unsqueeze(1)
    return a, tag, cfg, split_weights(a, tag), a[f"{tag}.tokens"].long(), enc, enc_len, pad


# wait-k cases: (simul_attn_type, waitk_lagging, ratio, S, source lengths, U).  With fixed pre-decision the source lengths are whole
# multiples of the ratio: train mode pools with ceil over the padded batch, the step path with floor over each row's own length,
# and the two see the same pooled positions exactly there (a partial last window is a pooled position in train mode only).
# The last element is the seed of the weights, tokens and source: chosen per case so that at least 90 % of the positions have a
# decisive top-2 margin (test_step_cases_have_decisive_margins), which the bf16 comparison of the HIP test relies on.
WAITK_CASES = (("waitk", 3, 1, 21, (21, 16, 9), 12, 10),
               ("waitk_fixed_pre_decision", 3, 2, 20, (20, 16, 10), 12, 5),
               ("waitk_fixed_pre_decision", 2, 4, 300, (300, 172, 64), 14, 11))


def spread_output_projection(cfg, g, max_norm=2.0, decay=0.8):
    """an UNTIED output projection whose row norms fall geometrically from max_norm (rows in random order): a few tokens dominate a
    position, as in a trained vocabulary -- Gaussian rows of equal norm put the top two of 64 logits within the bf16 bound of each
    other at a quarter of the positions -- while no row is long enough to lift the bf16 noise of the features (|w| |y| 2^-9, |y| =
    sqrt(D)) over that bound"""
    W = torch.randn(cfg.vocab, cfg.embed_dim, generator=g)
    W = W / W.norm(dim=1, keepdim=True)
    norms = max_norm * decay ** torch.arange(cfg.vocab, dtype=torch.float)
    return W * norms[torch.randperm(cfg.vocab, generator=g)].unsqueeze(1)


def waitk_case(name, k, ratio, S, lens, U, seed=7):
    """random tiny wait-k model with an UNTIED, spread output projection (a tied random embedding gives near-flat logits, which
    would make the bf16 argmax comparison of the HIP test vacuous), tokens and a right-padded source"""
    from simulst_amd.config import tiny
    from simulst_amd.weights import init_model
    cfg = tiny(simul_attn_type=name, waitk_lagging=k, fixed_pre_decision_ratio=ratio)
    w = init_model(cfg, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    w["decoder.output_projection.weight"] = spread_output_projection(cfg, g)
    B = len(lens)
    enc_len = torch.tensor(lens)
    pad = torch.arange(S).unsqueeze(0) >= enc_len.unsqueeze(1)
    enc = torch.randn(S, B, cfg.embed_dim, generator=g).masked_fill(pad.t().unsqueeze(-1), 0.0)
    tokens = torch.cat([torch.full((B, 1), cfg.eos), torch.randint(4, cfg.vocab, (B, U - 1), generator=g)], 1)
    return cfg, w, tokens, enc, enc_len, pad


FULL_CASES = (("full", 0, 1, 21, (21, 16, 9), 12, 3), ("full", 0, 1, 300, (300, 172, 64), 14, 3))


def full_case(name, k, ratio, S, lens, U, seed=3):
    """the same for the s2t_emformer decoder (plain encoder-decoder attention)"""
    from simulst_amd.config import tiny
    from simulst_amd.weights import init_model
    cfg = tiny(model="s2t_emformer", simul_attn_type="full", mass_preservation=False)
    w = init_model(cfg, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    w["decoder.output_projection.weight"] = spread_output_projection(cfg, g)
    enc_len = torch.tensor(lens)
    pad = torch.arange(S).unsqueeze(0) >= enc_len.unsqueeze(1)
    enc = torch.randn(S, len(lens), cfg.embed_dim, generator=g).masked_fill(pad.t().unsqueeze(-1), 0.0)
    tokens = torch.cat([torch.full((len(lens), 1), cfg.eos), torch.randint(4, cfg.vocab, (len(lens), U - 1), generator=g)], 1)
    return cfg, w, tokens, enc, enc_len, pad


def make_case(c):
    return full_case(*c) if c[0] == "full" else waitk_case(*c)


BF16_ATOL = BF16_RTOL = 0.05        # the project's bound between two bf16 forms of a step (tests/test_hip_decoder.py)


def safe_margin_mask(logits):
    """positions whose fp32 top-2 margin exceeds the bf16 bound at the top logit"""
    top = logits.float().topk(2, dim=-1).values
    return (top[..., 0] - top[..., 1]) > BF16_ATOL + BF16_RTOL * top[..., 0].abs()


@pytest.mark.parametrize("name,extra", G24_VARIANTS)
def test_restatement_equals_reference(name, extra):
    a, tag, cfg, w, tokens, enc, enc_len, pad = g24_case(name, extra)
    _, dcfg = from_model_config(cfg)
    with torch.no_grad():
        logits, attn_list = whole_target_forward(w, dcfg, tokens, enc, pad)
    for i, at in enumerate(attn_list):
        for k in ("p_choose", "alpha", "beta"):
            torch.testing.assert_close(at[k].float(), a[f"{tag}.l{i}.{k}"], atol=1e-5, rtol=0, msg=lambda m: f"{tag} layer {i} {k}: {m}")
    torch.testing.assert_close(logits, a[f"{tag}.logits"], atol=1e-4, rtol=0)


@pytest.mark.parametrize("case", WAITK_CASES, ids=lambda c: f"{c[0]}-k{c[1]}-r{c[2]}-S{c[3]}")
def test_waitk_restatement_equals_step_path(case):
    cfg, w, tokens, enc, enc_len, pad = waitk_case(*case)
    _, dcfg = from_model_config(cfg)
    with torch.no_grad():
        whole, attn_list = whole_target_forward(w, dcfg, tokens, enc, pad)
        steps = step_by_step_logits(w, dcfg, tokens, enc, pad)
    diff = (whole - steps).abs().max().item()
    print(f"{case[0]} S={case[3]}: max |whole - step| = {diff:.3e}")
    torch.testing.assert_close(whole, steps, atol=1e-4, rtol=0)
    # the diagonal: target u reads up to pooled position u + k - 1, clipped to the row's last one
    k, ratio = case[1], case[2]
    alpha = attn_list[0]["alpha"]
    for b, n in enumerate(case[4]):
        for u in range(tokens.size(1)):
            want = (min(u + k - 1, n // ratio - 1) + 1) * ratio - 1
            assert int(alpha[b, 0, u].argmax()) == want and float(alpha[b, 0, u, want]) == pytest.approx(1.0, abs=1e-5)


@pytest.mark.parametrize("case", WAITK_CASES + FULL_CASES, ids=lambda c: f"{c[0]}-k{c[1]}-r{c[2]}-S{c[3]}")
def test_step_cases_have_decisive_margins(case):
    """the bf16 HIP comparison asserts equal argmax wherever the fp32 top-2 margin exceeds the bf16 bound, and that at least 90 % of
    the positions have such a margin: the chosen seed must provide them"""
    cfg, w, tokens, enc, enc_len, pad = make_case(case)
    _, dcfg = from_model_config(cfg)
    with torch.no_grad():
        whole, _ = whole_target_forward(w, dcfg, tokens, enc, pad)
    frac = safe_margin_mask(whole).float().mean().item()
    print(f"{case[0]} S={case[3]}: {100 * frac:.1f} % of positions have a decisive margin")
    assert frac >= 0.9
