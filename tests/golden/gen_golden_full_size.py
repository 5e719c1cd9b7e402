#!/usr/bin/env python3
"""g21_full_size.npz: the reference's own encoder and decoder at FULL model size (s2t_emformer_s encoder, mma_model_s decoder,
wait-k 5, pre-decision ratio 8), recorded in the build container so that tests/test_oracle_vs_reference_live.py pins the oracle
at the dimensions every GPU parity test and the bench use without the reference tree.

The reference modules are built as tools/time_reference_cpu.py builds them (models/s2t_emformer.py, models/mma_model.py over
tests/golden/fairseq_standin.py), then loaded with simulst_amd.weights.init_model(mma_model_s(waitk_lagging=5), seed=999) --
with an untied output projection (randn seed 5, scaled by embed_dim ** -0.5) -- weights the test regenerates bit for bit, so
the fixture holds outputs only:

  lengths         [B]          of the B x T-frame N(0,1) fbank, utterance i drawn with seed 999 + i (not stored)
  encoder_out     [T', B, D]   the reference encoder's offline pass
  tokens          [B, steps]   110-step-style forced greedy decode (pad and EOS masked), `steps` steps
  seed            init_model seed

    python tests/golden/gen_golden_full_size.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import gen_golden as gg  # noqa: E402

B, T, STEPS, SEED = 2, 400, 16, 999


@torch.no_grad()
def main():
    from simulst_amd.config import mma_model_s
    from simulst_amd.weights import init_model
    gg.load_reference()
    s2e = sys.modules["codebase.models.s2t_emformer"]
    mmam = sys.modules["codebase.models.mma_model"]
    standin = gg.standin
    cfg = mma_model_s(waitk_lagging=5)
    a = gg.tiny_model_args(
        encoder_embed_dim=256, encoder_ffn_embed_dim=2048, encoder_attention_heads=4, encoder_layers=12,
        decoder_embed_dim=256, decoder_ffn_embed_dim=2048, decoder_attention_heads=4, decoder_layers=6,
        conv_channels=cfg.conv_channels, conv_pos=cfg.conv_pos, conv_pos_groups=cfg.conv_pos_groups, segment_length=64,
        segment_left_context=128, segment_right_context=32, max_memory_size=5, simul_attn_type="waitk_fixed_pre_decision",
        fixed_pre_decision_ratio=8, waitk_lagging=5, mass_preservation=False, share_decoder_input_output_embed=False)
    D = standin.Dictionary(cfg.vocab - 4)
    torch.manual_seed(SEED)
    enc = s2e.S2TEmformerEncoder(a, D).eval()
    emb = standin.Embedding(len(D), 256, D.pad())
    dec = mmam.MMADecoder(a, D, emb).eval()
    w = init_model(cfg, seed=SEED)
    # an UNTIED output projection (as smoke() does): with the tied random embedding the greedy decode repeats one token
    w["decoder.output_projection.weight"] = torch.randn(cfg.vocab, cfg.embed_dim,
                                                        generator=torch.Generator().manual_seed(5)) * cfg.embed_dim ** -0.5
    for pre, mod in (("encoder.", enc), ("decoder.", dec)):
        sd = {k[len(pre):]: v for k, v in w.items() if k.startswith(pre)}
        missing, unexpected = mod.load_state_dict(sd, strict=False)
        params = {k for k, _ in mod.named_parameters()}
        assert not unexpected, unexpected
        assert not (set(missing) & params), sorted(set(missing) & params)
    fb = torch.stack([torch.randn(T, 80, generator=torch.Generator().manual_seed(999 + i)) for i in range(B)])
    L = torch.full((B,), T)
    eo = enc(fb, L)
    inc = {}
    toks = torch.full((B, 1), D.eos(), dtype=torch.long)
    for _ in range(STEPS):
        inc["online"] = False
        x, _ = dec(prev_output_tokens=toks, encoder_out=eo, incremental_state=inc)
        lp = torch.log_softmax(x[:, -1].float(), dim=-1)
        lp[:, D.pad()] = -float("inf")
        lp[:, D.eos()] = -float("inf")
        toks = torch.cat([toks, lp.argmax(-1, keepdim=True)], dim=1)
    toks = toks[:, 1:]
    assert len(set(toks.flatten().tolist())) >= 4, "degenerate fixture: the greedy decode repeats a token"
    out = {"lengths": L.numpy(), "encoder_out": eo["encoder_out"][0].numpy(), "tokens": toks.numpy(),
           "seed": np.array(SEED)}
    np.savez_compressed(os.path.join(HERE, "g21_full_size.npz"), **out)
    print("g21_full_size.npz:", {k: v.shape for k, v in out.items()}, "tokens", toks.tolist())


if __name__ == "__main__":
    main()
