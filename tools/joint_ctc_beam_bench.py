#!/usr/bin/env python3
"""Joint CTC / attention beam search (SimulSTModel.generate(ctc_weight=...): ctc.CTCPrefixScorer inside the beam loop) against the
plain beam search and against two-pass rescoring, and what one beam step of it costs.

Shape: 64 utterances x 1000 frames (250 encoder rows), s2t_emformer_s dims with a CTC head, bf16, beam 5 (K = 10 candidates a row,
320 rows); the encoder runs once and is not timed.  Three decodes of the same encoder output:
  plain      decoder.beam_offline(beam=5)
  joint      the same with ctc=CTCPrefixScorer(weight=0.3) (the scorer's construction -- the blank's column, the empty prefix -- included)
  two_pass   decoder.beam_offline(beam=5, nbest=5), the lists read back, ctc.ctc_rescore(weight=0.3)
and, on a scorer ten steps into a search, the device time of the three things a step adds: the gather of the candidates'
log-probabilities (Ops.linear_gather over cand_tok viewed as [64][50]), the scoring launch (against its composed torch form) and the
commit launch.

Method: warm-up, then 7 passes that ALTERNATE the forms; each pass times `inner` back-to-back calls of one form under a pair of HIP
events and reports the per-call time; the figure of a form is the median of its 7 passes (min / max beside it).

Prints ONE JSON line and writes it to --out.  Run under a time limit:
    timeout -k 10 600 python tools/joint_ctc_beam_bench.py --out profiles/joint_ctc_beam_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, FRAMES, BEAM, LAM = 64, 1000, 5, 0.3


def time_calls(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def stats(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def alternate(forms, passes=7):
    """forms: {name: (fn, inner)} -> {name: stats of the per-call ms}"""
    for fn, _ in forms.values():
        fn()
    ts = {n: [] for n in forms}
    for _ in range(passes):
        for n, (fn, inner) in forms.items():
            ts[n].append(time_calls(fn, inner))
    return {n: stats(v) for n, v in ts.items()}


class StepBuffers:
    """what a CTCPrefixScorer reads of a BeamSearch, with distinct random candidates a row"""

    def __init__(self, R, Bs, K, V, dev, gen):
        self.cand_tok = torch.stack([torch.randperm(V - 3, generator=gen)[:K] + 3 for _ in range(R)]).to(torch.int32).to(dev)
        self.cand_lp = -torch.sort(torch.rand(R, K, generator=gen) * 8, dim=1).values.to(dev)
        self.finished = torch.zeros(Bs, dtype=torch.int32, device=dev)
        self.next_tok = torch.zeros(R, dtype=torch.int64, device=dev)
        self.reorder = torch.arange(R, dtype=torch.int32, device=dev)
        self.result = torch.zeros(4, dtype=torch.int32, device=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--passes", type=int, default=7)
    args = ap.parse_args()
    from simulst_amd import ctc
    from simulst_amd.config import s2t_emformer_s
    from simulst_amd.model import S2TEmformerModel
    from simulst_amd.weights import init_model
    dev = "cuda:0"
    cfg = s2t_emformer_s(ctc_layer=True)
    model = S2TEmformerModel(cfg, init_model(cfg, seed=999), device=dev, dtype=torch.bfloat16)
    gen = torch.Generator().manual_seed(1)
    fb = torch.randn(B, FRAMES, 80, generator=gen).to(dev)
    L = torch.full((B,), FRAMES)
    caps = [model.target_cap(FRAMES)] * B
    dec, head, ops = model.decoder, model.encoder.w.ctc, model.ops
    with torch.no_grad():
        enc = model.encoder.forward(fb, L)
        rows, lens = enc["encoder_out_btd"], enc["encoder_lengths"]
        info = {}

        def plain():
            info["plain_steps"] = dec.beam_offline(rows, lens, caps, beam=BEAM)[4]["steps"]

        def joint():
            info["joint_steps"] = dec.beam_offline(rows, lens, caps, beam=BEAM, ctc=model.ctc_scorer(enc, beam=BEAM, ctc_weight=LAM))[4]["steps"]

        def two_pass():
            toks, n, scores, _, _ = dec.beam_offline(rows, lens, caps, beam=BEAM, nbest=BEAM)
            toks, n, scores = toks.cpu(), n.cpu(), scores.cpu()
            nbest = [[(toks[s, k, :int(n[s, k]) - 1].tolist(), float(scores[s, k])) for k in range(BEAM) if int(n[s, k])] for s in range(B)]
            ctc.ctc_rescore(ops, head, rows, lens, nbest, weight=LAM)

        decode = alternate({"plain": (plain, 1), "joint": (joint, 1), "two_pass": (two_pass, 1)}, args.passes)
        # ---- one step's additions, on a scorer ten steps into a search
        sc = model.ctc_scorer(enc, beam=BEAM, ctc_weight=LAM)
        bs = StepBuffers(sc.R, B, sc.K, cfg.vocab, dev, gen)
        keep_lp, keep_tok = bs.cand_lp.clone(), bs.cand_tok.clone()

        def step(t):
            bs.cand_lp.copy_(keep_lp)
            bs.cand_tok.copy_(keep_tok)
            sc.rescore(t, bs)
            own = torch.arange(sc.R, device=dev)
            par = own // BEAM * BEAM if t == 0 else own           # step 0 scores row 0 of a sentence alone: every row's parent
            bs.reorder.copy_(par.to(torch.int32))
            bs.next_tok.copy_(bs.cand_tok[par, 0])
            sc.commit(t, bs)

        for t in range(10):
            step(t)
        labels = bs.cand_tok.view(B, BEAM * sc.K)

        def score(composed=False):
            c = sc.cur
            ctc.ctc_prefix_score(ops, sc.xc, sc.xb, sc.state[c], sc.psi[c], sc.last[c], sc.plen[c], sc.in_len, bs.finished, bs.cand_lp,
                                 bs.cand_tok, sc.cand_slot, sc.cand_state, sc.cand_psi, G=BEAM, blank=0, eos=cfg.eos, pad=cfg.padding_idx,
                                 weight=LAM, composed=composed)

        def commit():
            c = sc.cur
            ctc.ctc_prefix_commit(ops, sc.cand_state, sc.cand_psi, bs.cand_tok, sc.cand_slot, bs.next_tok, bs.reorder, bs.finished,
                                  sc.last[c], sc.plen[c], sc.in_len, sc.state[1 - c], sc.psi[1 - c], sc.last[1 - c], sc.plen[1 - c],
                                  bs.result[3:4], G=BEAM)

        sc.gather(labels, out=sc.xc)
        score()
        bs.next_tok.copy_(bs.cand_tok[:, 0])
        parts = alternate({"gather": (lambda: sc.gather(labels, out=sc.xc), 20), "score": (score, 20), "commit": (commit, 20)}, args.passes)
        parts["score_composed"] = alternate({"c": (lambda: score(True), 1)}, 3)["c"]
        torch.cuda.synchronize()
        assert int(bs.result[3]) == 0
    steps = max(info["joint_steps"], 1)
    added = parts["gather"]["median"] + parts["score"]["median"] + parts["commit"]["median"]
    rec = {"bench": "joint_ctc_beam", "shape": f"{B} x {FRAMES} frames, {int(lens.max())} encoder rows, beam {BEAM}, K {sc.K}, rows {sc.R}",
           "dtype": "bf16", "model": "s2t_emformer_s + ctc_layer, random init", "ctc_weight": LAM, "decode_ms": decode, "steps": info,
           "joint_over_plain": decode["joint"]["median"] / decode["plain"]["median"],
           "two_pass_over_plain": decode["two_pass"]["median"] / decode["plain"]["median"],
           "per_step_ms": parts, "per_step_added_ms": added, "gather_share_of_added": parts["gather"]["median"] / added,
           "added_ms_per_decode_from_parts": added * steps,
           "score_composed_over_kernel": parts["score_composed"]["median"] / parts["score"]["median"]}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
