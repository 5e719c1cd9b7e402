#!/usr/bin/env python3
"""g23_s2t_emformer.npz: the reference's offline ASR model (models/s2t_emformer.py:297-413, S2TEmformerModel over fairseq's plain
TransformerDecoder) at tiny dims, built through its own ``build_model`` and arch function on top of tests/golden/fairseq_standin.py
(tier 2: decoder base).

The stand-in has no ``S2TTransformerModel.build_decoder`` and no ``TransformerDecoder.extract_features``; both are restated below
following fairseq's dataflow (the one models/mma_model.py:79-220 witnesses for its own decoder: sinusoidal positions of the whole
prefix with only the newest row kept under an incremental state, embed_scale * embedding + positions, the layers with the encoder
padding mask, the final LayerNorm).

  args.<name>           the arch-resolved model args (scalars; conv_kernel_sizes as a string)
  keys / shapes         the decoder state-dict key names and shapes (order of model.state_dict())
  w:<name>              the decoder weights (untied output projection, EOS row scaled down so hypotheses run long)
  enc_out [S, B, D]     encoder states of a ragged batch; enc_len [B] (one row with a single encoder row)
  step_logits [n, B, V] the incremental logits of teacher-forced steps over `forced` [B, n] (prefix [eos] + forced[:, :t])
  greedy [B, n_greedy]  greedy tokens (EOS masked at the first step, as SequenceGenerator's min_len 1), incremental

    python tests/golden/gen_golden_s2t_emformer.py
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402
import fairseq_standin as standin  # noqa: E402


def _extract_features(self, prev_output_tokens, encoder_out=None, incremental_state=None, full_context_alignment=False,
                      alignment_layer=None, alignment_heads=None):
    """fairseq TransformerDecoder.extract_features (decoder_normalize_before, no layernorm_embedding / project_in_dim)."""
    positions = self.embed_positions(prev_output_tokens, incremental_state=incremental_state)
    if incremental_state is not None:
        prev_output_tokens = prev_output_tokens[:, -1:]
        positions = positions[:, -1:]
    x = self.embed_scale * self.embed_tokens(prev_output_tokens)
    x = x + positions
    x = self.dropout_module(x)
    x = x.transpose(0, 1)
    enc = encoder_out["encoder_out"][0] if encoder_out is not None and len(encoder_out["encoder_out"]) > 0 else None
    pad = (encoder_out["encoder_padding_mask"][0]
           if encoder_out is not None and len(encoder_out.get("encoder_padding_mask", [])) > 0 else None)
    for layer in self.layers:
        self_attn_mask = self.buffered_future_mask(x) if incremental_state is None else None
        x, _, _ = layer(x, enc, pad, incremental_state, self_attn_mask=self_attn_mask, need_attn=False)
    if self.layer_norm is not None:
        x = self.layer_norm(x)
    return x.transpose(0, 1), {"attn": [None], "inner_states": None}


def _build_decoder(cls, args, task, embed_tokens):
    """S2TTransformerModel.build_decoder: a plain TransformerDecoder over the target dictionary."""
    return standin.TransformerDecoder(args, task.target_dictionary, embed_tokens)


@torch.no_grad()
def main():
    gg.load_reference()
    s2e = sys.modules["codebase.models.s2t_emformer"]
    standin.S2TTransformerModel.build_decoder = classmethod(_build_decoder)
    standin.TransformerDecoder.extract_features = _extract_features
    Dct = standin.Dictionary(60)                    # vocab 64
    task = argparse.Namespace(source_dictionary=None, target_dictionary=Dct)
    # the tiny dims of the other tier-2 fixtures; no policy flags (a plain TransformerDecoder reads none)
    a = argparse.Namespace(
        input_feat_per_channel=80, input_channels=1, conv_channels=64, conv_kernel_sizes="5,5",
        encoder_embed_dim=32, encoder_ffn_embed_dim=64, encoder_attention_heads=2, encoder_layers=2,
        decoder_embed_dim=32, decoder_ffn_embed_dim=64, decoder_attention_heads=2, decoder_layers=2,
        dropout=0.0, attention_dropout=0.0, activation_dropout=0.0,
        conv_pos=16, conv_pos_groups=4, segment_length=16, segment_left_context=32, segment_right_context=8,
        max_memory_size=2, share_decoder_input_output_embed=False)
    torch.manual_seed(23)
    model = s2e.S2TEmformerModel.build_model(a, task).eval()
    dec = model.decoder
    gg.jitter_layernorms(dec, 230)
    dec.output_projection.weight.data[Dct.eos()] *= 0.25
    out = {}
    for k, v in sorted(vars(a).items()):
        if isinstance(v, (bool, int, float, str)):
            out[f"args.{k}"] = np.array(v)
    sdict = dec.state_dict()
    out["keys"] = np.array(["decoder." + k for k in sdict])
    out["shapes"] = np.array([list(v.shape) + [0] * (2 - v.dim()) for v in sdict.values()])
    out.update({f"w:decoder.{k}": v.numpy() for k, v in sdict.items()})
    # ragged batch of encoder states: 9, 4 and 1 valid rows
    S, B = 9, 3
    enc_len = torch.tensor([9, 4, 1])
    enc = torch.randn(S, B, 32, generator=torch.Generator().manual_seed(231))
    pad = torch.arange(S).unsqueeze(0) >= enc_len.unsqueeze(1)
    enc = enc.masked_fill(pad.t().unsqueeze(-1), 0.0)
    eo = {"encoder_out": [enc], "encoder_padding_mask": [pad]}
    out["enc_out"], out["enc_len"] = enc.numpy(), enc_len.numpy()
    # teacher-forced incremental steps
    n = 6
    forced = torch.randint(4, len(Dct), (B, n), generator=torch.Generator().manual_seed(232))
    inc, logits = {}, []
    for t in range(n):
        prev = torch.cat([torch.full((B, 1), Dct.eos()), forced[:, :t]], 1)
        x, _ = dec(prev, encoder_out=eo, incremental_state=inc)
        logits.append(x[:, -1])
    out["forced"] = forced.numpy()
    out["step_logits"] = torch.stack(logits).numpy()
    # greedy, incremental (EOS masked at step 0 only; pad never)
    n_greedy = 8
    inc, hyp = {}, torch.full((B, 1), Dct.eos())
    for t in range(n_greedy):
        x, _ = dec(hyp, encoder_out=eo, incremental_state=inc)
        lp = torch.log_softmax(x[:, -1].float(), -1)
        lp[:, Dct.pad()] = -float("inf")
        if t == 0:
            lp[:, Dct.eos()] = -float("inf")
        hyp = torch.cat([hyp, lp.argmax(-1, keepdim=True)], 1)
    out["greedy"] = hyp[:, 1:].numpy()
    print("greedy:", out["greedy"].tolist())
    path = os.path.join(HERE, "g23_s2t_emformer.npz")
    np.savez_compressed(path, standin_tier=np.array(2), **out)
    print(f"  g23_s2t_emformer.npz  {os.path.getsize(path) / 1024:.1f} KB  ({len(out) + 1} arrays)")


if __name__ == "__main__":
    main()
