#!/usr/bin/env python3
"""g25_transducer.npz: the reference's transducer (models/transducer_model.py:28-212: AvgPool1dTBCPad, TransducerDecoder over
fairseq's TransformerDecoder with no_encoder_attn, SimpleJoiner) at tiny dims, built through its own ``build_model`` and arch
function on top of tests/golden/fairseq_standin.py.  The stand-in's TransformerDecoder gets the ``extract_features`` of
gen_golden_s2t_emformer.py and the decoder class the stand-in's incremental-state mixin (fairseq's TransformerDecoder carries it).

  args.<name>              the arch-resolved model args (scalars; conv_kernel_sizes as a string)
  keys / shapes            the decoder state-dict key names and shapes (order of model.state_dict())
  w:<name>                 the decoder weights (untied output projection; its blank row and the target projection scaled up so that
                           the blank wins often enough for the emit position to move -- with plain random weights it never does)
  enc_out [T, B, D]        encoder states of a ragged batch, enc_len [B] = 39, 38, 21, 3 with T = 39 and downsample 4:
                           len == T with T % k != 0 | the k / r rescale inside the batch's clipped last window | a partial window
                           inside a full-size one | S' = 1 (every step forced at position 0)
  pooled [S', B, D], pooled_len [B]   the downsample op's output
  forced [B, n], step_logits [n, B, V], step_emit [n, B]   teacher-forced incremental steps (prefix [bos] + forced[:, :t])
  greedy [B, m], greedy_emit [B, m]   greedy tokens (EOS masked at the first step, pad never) and their emit positions

The script searches a small grid (blank scale, target-projection scale, token seed) for the first setting whose trajectories meet
the assertions at the bottom, so that the fixture exercises advancing, staying and forced emissions with clear margins.

    python tests/golden/gen_golden_transducer.py
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
from gen_golden_s2t_emformer import _extract_features  # noqa: E402

LENS = [39, 38, 21, 3]
K = 4
N_FORCED, N_GREEDY = 14, 12
MARGIN = 1e-3


def run(dec, eo, Dct, tokens_fn, n, captured):
    """n incremental steps; tokens_fn(t, row logits [B, V]) -> the tokens written at step t.  Returns logits [n, B, V], emits [n, B],
    the written tokens [B, n] and the smallest decision margin."""
    B = eo["encoder_out"][0].shape[1]
    src_last = (~eo["encoder_padding_mask"][0][:, ::K]).sum(1) - 1
    inc, hyp, logits, emits, margin = {}, torch.full((B, 1), Dct.eos()), [], [], float("inf")
    prev_emit = torch.zeros(B, dtype=torch.long)
    for t in range(n):
        x, _ = dec(hyp.clone(), encoder_out=eo, incremental_state=inc)
        ne = dec._get_input_buffer(inc)["prev_emit"].clone()
        full = captured[-1].squeeze(2).double()                       # [B, S, V] before the blank / past-position edits
        for b in range(B):
            for s in range(int(prev_emit[b]), int(ne[b]) + 1):
                row = full[b, s].clone()
                if s == int(src_last[b]):
                    row[Dct.bos()] = -1e4
                margin = min(margin, float((row[1:].max() - row[0]).abs()))
        toks, m = tokens_fn(t, x[:, -1])
        margin = min(margin, m)
        hyp = torch.cat([hyp, toks.view(B, 1)], 1)
        logits.append(x[:, -1].clone()), emits.append(ne)
        prev_emit = ne
    return torch.stack(logits), torch.stack(emits), hyp[:, 1:], margin


def good_trajectory(emits, last):
    """per long row: >= 2 steps that advance by >= 2 positions, >= 2 that stay, >= 2 tokens at the row's last position"""
    for b in range(3):
        e = [0] + [int(v) for v in emits[:, b]]
        adv = sum(1 for i in range(1, len(e)) if e[i] - e[i - 1] >= 2)
        stay = sum(1 for i in range(2, len(e)) if e[i] == e[i - 1])
        at_end = sum(1 for v in e[1:] if v == int(last[b]))
        if adv < 2 or stay < 2 or at_end < 2:
            return False
    return True


@torch.no_grad()
def main():
    gg.load_reference()
    tm = gg._load("codebase.models.transducer_model", f"{gg.REF}/models/transducer_model.py")
    standin.TransformerDecoder.extract_features = _extract_features
    standin.with_incremental_state(tm.TransducerDecoder)
    Dct = standin.Dictionary(60)                    # vocab 64
    task = argparse.Namespace(source_dictionary=None, target_dictionary=Dct)
    a = argparse.Namespace(
        input_feat_per_channel=80, input_channels=1, conv_channels=64, conv_kernel_sizes="5,5",
        encoder_embed_dim=32, encoder_ffn_embed_dim=64, encoder_attention_heads=2, encoder_layers=2,
        decoder_embed_dim=32, decoder_ffn_embed_dim=64, decoder_attention_heads=2, decoder_layers=2,
        dropout=0.0, attention_dropout=0.0, activation_dropout=0.0,
        conv_pos=16, conv_pos_groups=4, segment_length=16, segment_left_context=32, segment_right_context=8,
        max_memory_size=2, share_decoder_input_output_embed=False, downsample=K)
    tm.transducer_model_s(a)
    torch.manual_seed(25)
    model = tm.TransducerModel.build_model(a, task).eval()
    dec = model.decoder
    dec.init_incremental_state()
    gg.jitter_layernorms(dec, 250)
    captured = []
    joiner_forward = dec.joiner.forward
    dec.joiner.forward = lambda s, t: (captured.append(joiner_forward(s, t).clone()), captured[-1])[1]
    T, B = max(LENS), len(LENS)
    enc_len = torch.tensor(LENS)
    enc = torch.randn(T, B, 32, generator=torch.Generator().manual_seed(251))
    pad = torch.arange(T).unsqueeze(0) >= enc_len.unsqueeze(1)
    enc = enc.masked_fill(pad.t().unsqueeze(-1), 0.0)
    pooled, pooled_pad = dec.downsample_op(enc.clone(), pad)
    pooled_len = (~pooled_pad).sum(1)
    last = pooled_len - 1
    w_out0 = dec.output_projection.weight.data.clone()
    w_tgt0 = dec.joiner.target_projection.weight.data.clone()

    def greedy_tokens(t, row):
        lp = torch.log_softmax(row.float(), -1)
        lp[:, Dct.pad()] = -float("inf")
        if t == 0:
            lp[:, Dct.eos()] = -float("inf")
        top = lp.topk(2, -1).values
        return lp.argmax(-1), float((top[:, 0] - top[:, 1]).min())

    found = None
    for tgt_scale in (1.0, 3.0, 6.0):
        for blank_scale in (2.0, 3.0, 4.0, 6.0, 8.0):
            dec.output_projection.weight.data.copy_(w_out0)
            dec.output_projection.weight.data[Dct.bos()] *= blank_scale
            dec.joiner.target_projection.weight.data.copy_(w_tgt0 * tgt_scale)
            for seed in range(24):
                forced = torch.randint(4, len(Dct), (B, N_FORCED), generator=torch.Generator().manual_seed(2520 + seed))
                eo = {"encoder_out": [enc.clone()], "encoder_padding_mask": [pad]}

                def forced_tokens(t, row, forced=forced):
                    top = row.topk(2, -1).values
                    return forced[:, t], float((top[:, 0] - top[:, 1]).min())
                fl, fe, _, fm = run(dec, eo, Dct, forced_tokens, N_FORCED, captured)
                if not good_trajectory(fe, last) or fm < MARGIN:
                    continue
                gl, ge, gt, gm = run(dec, eo, Dct, greedy_tokens, N_GREEDY, captured)
                if gm < MARGIN or any(len(set(gt[b].tolist())) < 4 for b in range(B)):
                    continue
                found = (tgt_scale, blank_scale, seed, forced, fl, fe, fm, gt, ge, gm)
                break
            if found:
                break
        if found:
            break
    assert found is not None, "no setting of the search grid gives a non-degenerate trajectory"
    tgt_scale, blank_scale, seed, forced, fl, fe, fm, gt, ge, gm = found
    # the three assertions of the fixture
    assert good_trajectory(fe, last)
    assert min(fm, gm) >= MARGIN
    assert all(len(set(gt[b].tolist())) >= 4 for b in range(B))
    assert bool((fe[:, 3] == 0).all()) and bool((ge[:, 3] == 0).all())          # the S' = 1 row: every step at position 0
    print(f"target-projection scale {tgt_scale}, blank scale {blank_scale}, token seed {seed}; margins forced {fm:.2e} greedy {gm:.2e}")
    print("forced emits:", fe.t().tolist())
    print("greedy:", gt.tolist(), "emits:", ge.t().tolist())

    out = {}
    for k, v in sorted(vars(a).items()):
        if isinstance(v, (bool, int, float, str)):
            out[f"args.{k}"] = np.array(v)
    sdict = dec.state_dict()
    out["keys"] = np.array(["decoder." + k for k in sdict])
    out["shapes"] = np.array([list(v.shape) + [0] * (2 - v.dim()) for v in sdict.values()])
    out.update({f"w:decoder.{k}": v.numpy() for k, v in sdict.items()})
    out["enc_out"], out["enc_len"] = enc.numpy(), enc_len.numpy()
    out["pooled"], out["pooled_len"] = pooled.numpy(), pooled_len.numpy()
    out["forced"], out["step_logits"], out["step_emit"] = forced.numpy(), fl.numpy(), fe.numpy()
    out["greedy"], out["greedy_emit"] = gt.numpy(), ge.t().contiguous().numpy()
    out["search"] = np.array([tgt_scale, blank_scale, seed])
    path = os.path.join(HERE, "g25_transducer.npz")
    np.savez_compressed(path, standin_tier=np.array(2), **out)
    print(f"  g25_transducer.npz  {os.path.getsize(path) / 1024:.1f} KB  ({len(out) + 1} arrays)")


if __name__ == "__main__":
    main()
