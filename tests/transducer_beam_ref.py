"""fp64 restatement of beam search over the transducer: ``TransducerRef.step`` (tests/transducer_ref.py) on per-row hypotheses under
the ``cpu_beam`` loop of tests/test_hip_beam.py (fairseq's SequenceGenerator with search.BeamSearch).  Row s * beam + j carries its
own hypothesis and its own prev_emit; the blank (bos) is an ordinary candidate wherever the step did not force it out.

``beam_model`` is the small model the GPU tests decode (the recipe of test_hip_transducer._big_model at a small vocabulary), and
``ref_beam`` also returns, per sentence and step it ran, the smallest decision margin of the reference: the candidate gap cpu_beam
reports and the scan margins (|blank - best non-blank| at every position a row of the sentence looked at)."""
import math

import torch

import transducer_ref as tr
from test_hip_beam import cpu_beam


def beam_model(seed, V=192, lens=(96, 75, 33, 9), out_scale=2.0):
    """-> (cfg, weights, enc [4, 96, 256], lens): 2 prediction-network layers, V tokens, the blank row scaled so that it wins at
    times, the joiner's projections scaled so that tanh saturates and the rows are confident"""
    from simulst_amd.config import transducer_model_s
    from simulst_amd.weights import init_model
    cfg = transducer_model_s(encoder_layers=1, decoder_layers=2, vocab=V)
    w = dict(init_model(cfg, seed=seed))
    g = torch.Generator().manual_seed(seed + 2)
    out = torch.randn(V, cfg.embed_dim, generator=g) * cfg.embed_dim ** -0.5 * out_scale
    out[0] *= 3.0
    w["decoder.output_projection.weight"] = w["decoder.joiner.output_projection.weight"] = out
    w["decoder.joiner.target_projection.weight"] = w["decoder.joiner.target_projection.weight"] * 3.0
    w["decoder.joiner.source_projection.weight"] = w["decoder.joiner.source_projection.weight"] * 4.0
    lens = list(lens)
    enc = torch.randn(len(lens), max(lens), cfg.embed_dim, generator=torch.Generator().manual_seed(seed + 1))
    enc = enc.masked_fill((torch.arange(max(lens)).view(1, -1) >= torch.tensor(lens).view(-1, 1)).unsqueeze(-1), 0.0)
    return cfg, w, enc, lens


def ref_beam(w, cfg, enc, lens, caps, beam, lenpen, nbest, round_to=None):
    """-> (per sentence the nbest list of (tokens, score, positional scores, emit positions), per sentence the margins of the steps
    it ran, src_len' [Bs]).  round_to: the dtype the weights and the encoder states are rounded to first (a bf16 model's reference)"""
    ref = tr.TransducerRef(w, heads=cfg.num_heads, downsample=cfg.downsample, pad=cfg.padding_idx, eos=cfg.eos, round_to=round_to)
    ref.set_source(enc if round_to is None else enc.to(round_to), lens)
    Bs = len(lens)
    R = Bs * beam
    src_len = ref.src_len.clone()
    ref.P = ref.P.repeat_interleave(beam, 0)
    ref.src_len = ref.src_len.repeat_interleave(beam, 0)
    ref.prev_emit = torch.zeros(R, dtype=torch.int64)
    st = {"paths": [[] for _ in range(R)], "emits": [[] for _ in range(R)], "cur": None}
    emit_of = {}                 # (sentence, tokens written by a row) -> emit positions of those tokens and of the row's next one
    scan = []                    # [step][row]: the row's smallest scan margin

    def logits_fn(t, toks):
        if t > 0:
            for r in range(R):
                st["paths"][r].append(int(toks[r]))
        hyp = torch.tensor(st["paths"], dtype=torch.int64).view(R, -1)
        rows, new_emit, margins = ref.step(hyp)
        st["cur"] = new_emit.tolist()
        for r in range(R):
            emit_of.setdefault((r // beam, tuple(st["paths"][r])), st["emits"][r] + [st["cur"][r]])
        scan.append([min(m) for m in margins])
        return rows

    def on_select(t, reorder):
        order = reorder.tolist()
        st["paths"] = [list(st["paths"][p]) for p in order]
        st["emits"] = [st["emits"][p] + [st["cur"][p]] for p in order]
        ref.prev_emit = ref.prev_emit[reorder]

    hyps, gaps = cpu_beam(logits_fn, caps, beam, cfg.vocab, cfg.eos, cfg.padding_idx, lenpen, nbest, on_select)
    out, margins = [], []
    for s in range(Bs):
        out.append([(toks, score, pos, emit_of[(s, tuple(toks[:-1]))]) for toks, score, pos in hyps[s]])
        # step 0 decides from the sentence's first row alone; later steps from all of its rows
        margins.append([min([gaps[s][t]] + scan[t][s * beam:s * beam + (1 if t == 0 else beam)]) for t in range(len(gaps[s]))])
    return out, margins, src_len


def smallest_margin(margins):
    return min((m for sent in margins for m in sent), default=math.inf)
