#!/usr/bin/env python3
"""g27_transducer_lattice.npz: the reference's TransducerDecoder.forward WITHOUT an incremental state (models/transducer_model.py
:124-163, the training lattice) on fixture g25's model and encoder states.  g25's arch-resolved args build the reference's model
through its own ``build_model`` on top of tests/golden/fairseq_standin.py, g25's decoder weights go in with ``load_state_dict``.

  targets [B, U], target_lengths [B]   EOS-terminated targets of lengths 6, 4, 1, 3 (EOS counted; random tokens >= 4, then EOS, pads)
  prev_output_tokens [B, U]            the targets with their EOS moved to the front (what the criterion's sample carries)
  pooled_len [B]                       valid pooled source positions (10, 10, 6, 1)
  lattice_logits [B, S', U + 1, V]     the reference's output, fp32 [4, 10, 7, 64]

The reference edits its inputs in place (the bos column, the zeroed padded frames), so it is given clones.

    python tests/golden/gen_golden_transducer_lattice.py [--out PATH]
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

TARGET_LENS = [6, 4, 1, 3]


def build_reference_decoder(g):
    """the reference's TransducerDecoder carrying g25's weights, and its dictionary"""
    gg.load_reference()
    tm = gg._load("codebase.models.transducer_model", f"{gg.REF}/models/transducer_model.py")
    standin.TransformerDecoder.extract_features = _extract_features
    standin.with_incremental_state(tm.TransducerDecoder)
    V = g["w:decoder.embed_tokens.weight"].shape[0]
    Dct = standin.Dictionary(V - 4)
    a = argparse.Namespace(**{k[5:]: g[k].item() for k in g.files if k.startswith("args.")})
    task = argparse.Namespace(source_dictionary=None, target_dictionary=Dct)
    model = tm.TransducerModel.build_model(a, task).eval()
    dec = model.decoder
    dec.load_state_dict({k[len("w:decoder."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w:decoder.")})
    return dec, Dct


def make_targets(Dct, V):
    gen = torch.Generator().manual_seed(2700)
    B, U = len(TARGET_LENS), max(TARGET_LENS)
    targets = torch.full((B, U), Dct.pad(), dtype=torch.int64)
    prev = torch.full((B, U), Dct.pad(), dtype=torch.int64)
    for b, n in enumerate(TARGET_LENS):
        y = torch.randint(4, V, (n - 1,), generator=gen)
        targets[b, :n] = torch.cat([y, torch.tensor([Dct.eos()])])
        prev[b, :n] = torch.cat([torch.tensor([Dct.eos()]), y])
    return targets, prev


@torch.no_grad()
def reference_lattice(dec, enc_tbd, enc_len, prev):
    T = enc_tbd.shape[0]
    pad = torch.arange(T).unsqueeze(0) >= enc_len.unsqueeze(1)
    eo = {"encoder_out": [enc_tbd.clone()], "encoder_padding_mask": [pad.clone()]}
    logits, extra = dec(prev.clone(), encoder_out=eo, incremental_state=None)
    return logits.float(), (~extra["padding_mask"]).sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "g27_transducer_lattice.npz"))
    path = ap.parse_args().out
    g = np.load(os.path.join(HERE, "g25_transducer.npz"))
    dec, Dct = build_reference_decoder(g)
    V = g["w:decoder.embed_tokens.weight"].shape[0]
    targets, prev = make_targets(Dct, V)
    logits, pooled_len = reference_lattice(dec, torch.from_numpy(g["enc_out"]), torch.from_numpy(g["enc_len"]), prev)
    assert tuple(logits.shape) == (4, 10, 7, V), logits.shape
    assert pooled_len.tolist() == g["pooled_len"].tolist()
    np.savez_compressed(path, standin_tier=np.array(2), targets=targets.numpy(), target_lengths=np.array(TARGET_LENS),
                        prev_output_tokens=prev.numpy(), pooled_len=pooled_len.numpy(), lattice_logits=logits.numpy())
    print(f"  {os.path.basename(path)}  {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
