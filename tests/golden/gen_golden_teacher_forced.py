#!/usr/bin/env python3
"""g24_mma_teacher_forced.npz: the reference's MMADecoder (models/mma_model.py:156-220) called WITHOUT an incremental_state -- the
whole-target path through buffered_future_mask and monotonic_attention_process_train
(modules/monotonic_multihead_attention.py:301-352) -- at the tiny dims of g12, on top of tests/golden/fairseq_standin.py (tier 2).

B = 3 targets of U = 9 tokens over S = 21 encoder rows with source lengths 21 / 16 / 9 (encoder_padding_mask, right padding).
Per variant <tag>:
  <tag>.w:decoder.*        the decoder weights (monotonic energies spread as in g12)
  <tag>.enc [S, B, D], <tag>.enc_len [B], <tag>.tokens [B, U] (prev_output_tokens: eos first)
  <tag>.logits [B, U, V]
  <tag>.l<i>.p_choose / .alpha / .beta [B, H, U, S]    of every layer

wait-k cannot be recorded this way (waitk_p_choose dereferences incremental_state unconditionally,
utils/p_choose_strategy.py:35); tests/test_teacher_forced_oracle.py pins it against the step path instead.

    python tests/golden/gen_golden_teacher_forced.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402
import fairseq_standin as standin  # noqa: E402

VARIANTS = (("hard_aligned_fixed_pre_decision", {}),
            ("infinite_lookback_fixed_pre_decision", {}),
            ("hard_aligned", {"mass_preservation": False}),
            ("chunkwise", {"mocha_chunk_size": 3}),
            ("infinite_lookback", {}))


def tag_of(name, extra):
    return name + ("" if not extra else "." + ".".join(f"{k}={v}" for k, v in extra.items()))


@torch.no_grad()
def main():
    gg.load_reference()
    mmam = sys.modules["codebase.models.mma_model"]
    D = standin.Dictionary(60)   # vocab 64
    S, B, U = 21, 3, 9
    enc_len = torch.tensor([21, 16, 9])
    out = {}
    for name, extra in VARIANTS:
        torch.manual_seed(240 + len(name))
        a = gg.tiny_model_args(simul_attn_type=name, **extra)
        emb = standin.Embedding(len(D), 32, D.pad())
        dec = mmam.MMADecoder(a, D, emb).eval()
        gg.jitter_layernorms(dec, 241)
        # spread the monotonic energies so p_choose straddles 0.5 (as g12 does)
        for layer in dec.layers:
            layer.encoder_attn.q_proj.weight.data.mul_(4.0)
            layer.encoder_attn.k_proj.weight.data.mul_(4.0)
        tag = tag_of(name, extra)
        out.update({f"{tag}.{k}": v for k, v in gg.sd(dec, "decoder.").items()})
        g = torch.Generator().manual_seed(242)
        enc = torch.randn(S, B, 32, generator=g)
        pad = torch.arange(S).unsqueeze(0) >= enc_len.unsqueeze(1)
        enc = enc.masked_fill(pad.t().unsqueeze(-1), 0.0)
        tokens = torch.cat([torch.full((B, 1), D.eos()), torch.randint(4, len(D), (B, U - 1), generator=g)], 1)
        x, extra_out = dec(prev_output_tokens=tokens, encoder_out={"encoder_out": [enc], "encoder_padding_mask": [pad]})
        assert extra_out["action"] == 1 and len(extra_out["attn_list"]) == len(dec.layers)
        out[f"{tag}.enc"], out[f"{tag}.enc_len"], out[f"{tag}.tokens"] = enc.numpy(), enc_len.numpy(), tokens.numpy()
        out[f"{tag}.logits"] = x.numpy()
        for i, at in enumerate(extra_out["attn_list"]):
            for k in ("p_choose", "alpha", "beta"):
                out[f"{tag}.l{i}.{k}"] = at[k].float().numpy()
        print(f"g24 {tag}: logits {tuple(x.shape)}, alpha row sums layer 0 {at['alpha'][:, 0, -1].sum(-1).tolist()}")
    path = os.path.join(HERE, "g24_mma_teacher_forced.npz")
    np.savez_compressed(path, standin_tier=np.array(2), **out)
    print(f"  g24_mma_teacher_forced.npz  {os.path.getsize(path) / 1024:.1f} KB  ({len(out) + 1} arrays)")


if __name__ == "__main__":
    main()
