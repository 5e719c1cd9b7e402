#!/usr/bin/env python3
"""Error rates of the ASR paths, and what the metric costs: the batched edit distance of simulst_amd/edit_distance.py (ONE launch,
csrc/edit_distance.hip) against its composed form -- the hypotheses brought to the host and the same dynamic program as torch tensor
operations there, which is what a caller without the kernel does.

(a) Rates.  The tiny s2t_emformer model with a CTC head and random weights decodes 8 utterances five ways; the references are the
model's own output with a scripted corruption (every 7th label dropped, every 5th changed, one inserted behind every 11th), so a rate is
neither 0 nor 100 %.  A random model's CTC head and attention decoder say unrelated things, so each family is scored against ITS OWN
corrupted output: greedy and prefix beam 8 against the corrupted greedy transcript, attention beam 5 / joint ctc_weight 0.3 / the
16-best list's oracle / its minimum-Bayes-risk pick against the corrupted beam-5 hypothesis.  The numbers say that the plumbing
works (sums on the device, pairs by index), nothing about quality.

(b) Timings, synthetic label strings over 4096 labels, every hypothesis its reference with 15 % of the labels dropped / changed /
doubled:
  nbest_64x16     64 references x 16-best, 30-110 labels: 1 024 pairs, the reference read through its index
  mbr_64x16x16    the same lists against themselves: 16 384 pairs, one buffer on both sides
  ctc_1280x250    1 280 x 250-label strings: the best path of the large encoder batch, pairs by position
  nbest_64x16 with the alignment (back-pointers + device back-track) against counts only
Method (tools/ctc_beam_bench.py's): warm-up, then 7 passes that ALTERNATE the forms.  The kernel's figure is the per-call time of
`inner` back-to-back launches between two HIP events (allocation of the outputs included: it is Ops.edit_distance as a caller has it);
the composed form's is wall-clock from the device tensors to its result on the host (one call: it synchronises by itself).  Median of
the 7 passes, min / max beside it.

Prints ONE JSON line and writes it to --out.  Run under a time limit:
    timeout -k 10 600 python tools/error_rate_bench.py --out profiles/edit_distance_bench.json
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"
FRAMES = [400, 330, 260, 200, 150, 96, 80, 64]
DECODE_MS = 68.9                 # profiles/joint_ctc_beam_bench.json: the beam-5 decode of 64 utterances that the metric scores


def stats(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def corrupt(tokens, vocab, avoid):
    out = []
    for q, t in enumerate(tokens):
        if q % 7 == 6:
            continue
        if q % 5 == 4:
            t = (t + 3) % vocab
            while t in avoid:
                t = (t + 1) % vocab
        out.append(t)
        if q % 11 == 10:
            out.append(5)
    return out


def pack(strings, pad, width=None):
    width = max([len(s) for s in strings] + [1]) if width is None else width
    t = torch.full((len(strings), width), pad, dtype=torch.int64)
    for n, s in enumerate(strings):
        t[n, :len(s)] = torch.tensor(list(s), dtype=torch.int64)
    return t.to(DEV), torch.tensor([len(s) for s in strings], dtype=torch.int64, device=DEV)


def strip_eos(tokens, n, eos):
    """[..., L] hypotheses with lengths n that count a closing EOS -> lengths without it (device ops)"""
    n = n.to(torch.int64)
    last = tokens.gather(-1, (n - 1).clamp(min=0).unsqueeze(-1)).squeeze(-1)
    return n - ((n > 0) & (last == eos)).to(torch.int64)


def rates(ops):
    from simulst_amd.config import tiny
    from simulst_amd.ctc import token_error_report
    from simulst_amd.edit_distance import error_rate, error_sums, mbr_select, oracle_error
    from simulst_amd.model import S2TEmformerModel
    from simulst_amd.weights import init_model
    cfg = tiny(model="s2t_emformer", simul_attn_type="full", ctc_layer=True, mass_preservation=False)
    w = init_model(cfg, seed=31)
    g = torch.Generator().manual_seed(32)
    W = torch.randn(cfg.vocab, cfg.embed_dim, generator=g) * cfg.embed_dim ** -0.5
    W[cfg.eos] *= 3.0
    w["decoder.output_projection.weight"] = W
    w["encoder.ctc_layer.weight"] = torch.randn(cfg.vocab, cfg.embed_dim, generator=g) * 4.0 * cfg.embed_dim ** -0.5
    fb = torch.randn(len(FRAMES), max(FRAMES), 80, generator=torch.Generator().manual_seed(33))
    for b, f in enumerate(FRAMES):
        fb[b, f:] = 0
    T = torch.tensor(FRAMES)
    model = S2TEmformerModel(cfg, w, device=DEV, ops=ops)
    enc = model.encoder.forward(fb.to(DEV), T)
    rows, lens = enc["encoder_out_btd"], enc["encoder_lengths"]
    pad, eos = cfg.padding_idx, cfg.eos
    avoid = (pad, eos, 0)
    B = len(FRAMES)

    def rate(tokens, n, ref, ref_len):
        r = token_error_report(tokens, n, ref, ref_len, ops=ops)
        s = [int(r[k]) for k in ("errors", "sub", "del", "ins", "ref_labels")]
        return {"rate_pct": error_rate(s), "errors": s[0], "sub": s[1], "del": s[2], "ins": s[3], "ref_labels": s[4]}

    out = {}
    # ---- the CTC family against the corrupted greedy transcript
    gr = model.encoder.ctc_greedy(rows, lens)
    g_tok, g_n = gr["tokens"].cpu(), gr["n"].cpu()
    ref_ctc, ref_ctc_len = pack([corrupt(g_tok[b, :int(g_n[b])].tolist(), cfg.vocab, avoid) for b in range(B)], pad)
    out["greedy"] = rate(gr["tokens"], gr["n"], ref_ctc, ref_ctc_len)
    pb = model.encoder.ctc_prefix_beam_search(rows, lens, beam=8, candidates=8, nbest=1, pad=pad)
    out["prefix_beam_8"] = rate(pb["tokens"][:, 0], pb["n"][:, 0], ref_ctc, ref_ctc_len)
    # ---- the attention family against the corrupted beam-5 hypothesis
    max_len = [model.target_cap(int(t)) for t in FRAMES]

    def beam(width, nbest, lam=0.0):
        toks, n, scores, _, _ = model.decoder.beam_offline(rows, lens, max_len, beam=width, nbest=nbest,
                                                           ctc=model.ctc_scorer(enc, beam=width, ctc_weight=lam))
        return toks, strip_eos(toks, n, eos), scores, n
    a_tok, a_n, _, _ = beam(5, 1)
    a_c, a_nc = a_tok.cpu(), a_n.cpu()
    ref_att, ref_att_len = pack([corrupt(a_c[b, 0, :int(a_nc[b, 0])].tolist(), cfg.vocab, avoid) for b in range(B)], pad)
    out["attention_beam_5"] = rate(a_tok[:, 0], a_n[:, 0], ref_att, ref_att_len)
    j_tok, j_n, _, _ = beam(5, 1, 0.3)
    out["joint_ctc_weight_0.3"] = rate(j_tok[:, 0], j_n[:, 0], ref_att, ref_att_len)
    n_tok, n_n, n_scores, n_raw = beam(16, 16)
    present = n_raw > 0
    # a list may hold fewer than 16 finished hypotheses: an absent entry (length 0) may win neither choice
    _, _, allc = oracle_error(ref_att, ref_att_len, n_tok, n_n, ops=ops)
    dist = torch.where(present, allc[:, :, 0].to(torch.int64), 1 << 20)
    idx = (dist * 16 + torch.arange(16, device=dist.device)).argmin(1)          # the minimum, then the lower index
    best = allc[torch.arange(B, device=idx.device), idx]
    s = [int(x) for x in error_sums(best, ref_att_len)]
    out["oracle_of_16_best"] = {"rate_pct": error_rate(s), "errors": s[0], "ref_labels": s[4], "picked": idx.tolist(),
                                "entries_present": present.sum(1).tolist()}
    pick, _ = mbr_select(n_tok, n_n, torch.where(present, n_scores.float(), float("-inf")), ops=ops)
    m_tok = n_tok[torch.arange(B, device=pick.device), pick]
    m_n = n_n[torch.arange(B, device=pick.device), pick]
    out["mbr_pick_of_16_best"] = dict(rate(m_tok, m_n, ref_att, ref_att_len), picked=pick.tolist())
    out["first_of_16_best"] = rate(n_tok[:, 0], n_n[:, 0], ref_att, ref_att_len)
    return out


def noisy(rng, ref, vocab):
    h = []
    for t in ref:
        u = rng.random()
        if u < 0.05:
            continue
        h.append(rng.randrange(vocab) if u < 0.10 else t)
        if u > 0.95:
            h.append(t)
    return h[:1023]


def time_forms(kernel, composed, passes, inner):
    def kernel_ms():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            kernel()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / inner

    def composed_ms():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        composed()
        return (time.perf_counter() - t0) * 1e3
    kernel_ms()
    composed_ms()
    tk, tc = [], []
    for _ in range(passes):
        tk.append(kernel_ms())
        tc.append(composed_ms())
    k, c = stats(tk), stats(tc)
    return {"kernel_ms": k, "composed_ms": c, "composed_over_kernel": c["median"] / k["median"]}


def timings(ops, passes, inner):
    from simulst_amd.edit_distance import edit_distance
    rng = random.Random(41)
    V = 4096
    refs = [[rng.randrange(V) for _ in range(rng.randrange(30, 111))] for _ in range(64)]
    lists = [[noisy(rng, r, V) for _ in range(16)] for r in refs]
    ref, ref_len = pack(refs, 1)
    W = max(len(h) for hs in lists for h in hs)
    flat, flat_len = pack([h for hs in lists for h in hs], 1, W)
    ri = torch.arange(64, device=DEV, dtype=torch.int32).repeat_interleave(16)
    base = (torch.arange(64, device=DEV, dtype=torch.int32) * 16)[:, None, None]
    k16 = torch.arange(16, device=DEV, dtype=torch.int32)
    mi = (base + k16[None, :, None]).expand(64, 16, 16).reshape(-1).contiguous()
    mj = (base + k16[None, None, :]).expand(64, 16, 16).reshape(-1).contiguous()
    long_ref = [[rng.randrange(V) for _ in range(250)] for _ in range(1280)]
    lr, lrl = pack(long_ref, 1)
    lh, lhl = pack([noisy(rng, r, V)[:250] for r in long_ref], 1, 250)
    out = {}

    def both(name, pairs, **kw):
        def run(composed):
            return lambda: edit_distance(ops, *kw["args"], ref_idx=kw.get("ri"), hyp_idx=kw.get("hi"), path=kw.get("path", False),
                                         composed=composed)
        a, b = run(False)(), run(True)()
        a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
        same = all(torch.equal(x, y) for x, y in zip(a, b))
        out[name] = dict(time_forms(run(False), run(True), passes, inner), pairs=pairs, same_integers=same)
        if not same:
            raise SystemExit(f"{name}: the kernel and the composed form disagree")
    both("nbest_64x16_counts", 1024, args=(ref, ref_len, flat, flat_len), ri=ri)
    both("mbr_64x16x16_counts", 16384, args=(flat, flat_len, flat, flat_len), ri=mi, hi=mj)
    both("ctc_1280x250_counts", 1280, args=(lr, lrl, lh, lhl))
    both("nbest_64x16_path", 1024, args=(ref, ref_len, flat, flat_len), ri=ri, path=True)
    out["path_over_counts_kernel"] = out["nbest_64x16_path"]["kernel_ms"]["median"] / out["nbest_64x16_counts"]["kernel_ms"]["median"]
    out["label_lengths"] = {"nbest_reference": [min(len(r) for r in refs), max(len(r) for r in refs)], "nbest_hypothesis_width": W,
                            "ctc": 250}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    from simulst_amd.ops import Ops
    ops = Ops()
    res = {"bench": "edit_distance", "device": torch.cuda.get_device_name(0), "passes": args.passes, "inner": args.inner,
           "rates": rates(ops), "timings": timings(ops, args.passes, args.inner)}
    t = res["timings"]
    res["beside_the_decode"] = {"beam5_decode_ms_64_utterances": DECODE_MS, "source": "profiles/joint_ctc_beam_bench.json",
                                "nbest_64x16_counts_share_pct": 100.0 * t["nbest_64x16_counts"]["kernel_ms"]["median"] / DECODE_MS}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
