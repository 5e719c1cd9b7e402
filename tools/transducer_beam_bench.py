"""Beam search over the transducer (TransducerDecoder.beam_offline) at the bench shape of tools/transducer_bench.py, encoder
excluded: 64 utterances of 1000 frames (250 encoder rows -> 32 pooled positions with --downsample 8), bf16, transducer_model_s
dims, V = 4096, cap int(0.1 T + 10) = 110 tokens, random-init weights whose blank row is scaled up so that the emit positions move.

Reports
  * tokens/s of decoder.greedy_offline (110 steps of 64 rows) and of beam 1 / 4 / 5, the best hypothesis of each sentence counted
    (EOS included), as tools/beam_bench.py counts them,
  * per beam width the device time of a step, split with HIP events on the handle's stream into the prediction network, the joiner
    (target projection + scan + emit), the vocabulary row + top-k + select, and commit + reorder,
  * the same beam widths through the COMPOSITION of the earlier entry points -- P and src_len repeat_interleave'd to one copy per
    row, simulst_joiner_scan / simulst_joiner_emit over all rows (finished sentences included), K/V and prev_emit reordered with
    index_select -- with the same split.  It exists in this tool only and is the baseline the grouped entry points
    (simulst_joiner_scan_beam / simulst_joiner_emit_beam / simulst_transducer_beam_reorder) are measured against.
Every figure is the median of --reps passes after one warm-up pass (minimum and maximum beside the wall times); the two forms
alternate within each pass.  Writes one JSON object to --out.

    python tools/transducer_beam_bench.py --out profiles/transducer_beam_bench.json"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PHASES = ("prediction_network", "joiner_scan_emit", "vocab_row_topk_select", "commit_reorder")


def median(xs):
    return sorted(xs)[len(xs) // 2]


class Marks:
    """events on the handle's stream; five per step (one before each phase and one behind the last)"""

    def __init__(self, stream, on=True):
        self.stream, self.on, self.ev = stream, on, []

    def __call__(self):
        if self.on:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(self.stream)
            self.ev.append(ev)

    def split(self):
        n = len(self.ev) // 5
        tot = [0.0] * 4
        for i in range(n):
            for p in range(4):
                tot[p] += self.ev[5 * i + p].elapsed_time(self.ev[5 * i + p + 1])
        return n, [t / max(n, 1) for t in tot]


def grouped_beam(dec, enc, L, caps, beam, T, mark):
    """beam_offline itself, its phases marked through wrappers of the calls that end them"""
    ops = dec.ops
    orig = dec.features, ops.joiner_emit_beam, ops.beam_select, ops.transducer_beam_reorder

    def wrap(fn, before=False):
        def f(*a, **k):
            if before:
                mark()
            r = fn(*a, **k)
            mark()
            return r
        return f

    dec.features, ops.joiner_emit_beam = wrap(orig[0], before=True), wrap(orig[1])
    ops.beam_select, ops.transducer_beam_reorder = wrap(orig[2]), wrap(orig[3])
    try:
        return dec.beam_offline(enc, L, caps, beam=beam, T=T)
    finally:
        del dec.features, ops.joiner_emit_beam, ops.beam_select, ops.transducer_beam_reorder


def composition_beam(dec, enc, L, caps, beam, T, mark):
    """the same search from the entry points that were there before: one P per ROW, the ungrouped scan / emit over every row,
    index_select of the state"""
    from simulst_amd.beam import BeamSearch
    from simulst_amd.ops import EPI_BIAS_F32OUT
    cfg, ops, V = dec.cfg, dec.ops, dec.cfg.vocab
    bs = BeamSearch(ops, caps, beam=beam, V=V, eos=cfg.eos, pad=cfg.padding_idx, device=dec.device)
    R = bs.R
    st = dec.new_state(R, cap=bs.L + 2)
    dec.set_source(st, enc, L, T)
    st.P = st.P.repeat_interleave(beam, 0).contiguous()
    st.src_len = st.src_len.repeat_interleave(beam).contiguous()
    S = st.P.size(1)
    n_split = ops.joiner_split(R, S, V, dec.dtype)
    st.blank_logit = torch.empty(R, S, device=dec.device, dtype=torch.float32)
    st.best = torch.empty(R, S, n_split, device=dec.device, dtype=torch.float32)
    st.best_idx = torch.empty(R, S, n_split, device=dec.device, dtype=torch.int32)
    st.z = torch.empty(R, cfg.embed_dim, device=dec.device, dtype=dec.dtype)
    st.at_eos = torch.empty(R, device=dec.device, dtype=torch.int32)

    def logits_fn(t, toks):
        mark()
        feats = dec.features(st, toks)
        mark()
        st.g = ops.linear(feats, dec.w.w_tgt, None, epilogue=EPI_BIAS_F32OUT)
        ops.joiner_scan(st.P, st.g, dec.w.out_proj_fm, st.prev_emit, st.src_len, st.blank_logit, st.best, st.best_idx, V=V)
        ops.joiner_emit(st.P, st.g, st.blank_logit, st.best, st.best_idx, st.prev_emit, st.src_len, st.z, st.at_eos, V=V)
        mark()
        logits = ops.linear(st.z, dec.w.out_proj, None, epilogue=EPI_BIAS_F32OUT)
        return ops.joiner_mask_blank(logits, st.at_eos)

    def after_select(t):
        mark()
        dec.commit(st)
        idx = bs.reorder.long()
        st.k_cache = [k.index_select(0, idx) for k in st.k_cache]
        st.v_cache = [v.index_select(0, idx) for v in st.v_cache]
        st.prev_emit = st.prev_emit.index_select(0, idx)
        mark()

    return bs.run(logits_fn, after_select)


def main(argv=None):
    from simulst_amd.config import transducer_model_s
    from simulst_amd.transducer import TransducerDecoder
    from simulst_amd.weights import init_model
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--beams", default="1,4,5")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev, dt = "cuda", torch.bfloat16
    cfg = transducer_model_s()
    w = dict(init_model(cfg, seed=999))
    out_proj = w["decoder.output_projection.weight"].clone()
    out_proj[0] *= 6.0                                                          # as tools/transducer_bench.py
    w["decoder.output_projection.weight"] = w["decoder.joiner.output_projection.weight"] = out_proj
    w["decoder.joiner.target_projection.weight"] = w["decoder.joiner.target_projection.weight"] * 3.0
    w["decoder.joiner.source_projection.weight"] = w["decoder.joiner.source_projection.weight"] * 4.0
    dec = TransducerDecoder(cfg, w, device=dev, dtype=dt)
    T, B = args.frames, args.batch
    S_enc = ((T - 1) // 2 + 1 - 1) // 2 + 1
    n_steps = int(0.1 * T + 10)
    enc = torch.randn(B, S_enc, cfg.embed_dim, generator=torch.Generator().manual_seed(1)).to(dev, dt)
    L = torch.full((B,), S_enc, dtype=torch.int32, device=dev)
    caps = [n_steps] * B
    stream = torch.cuda.current_stream()                                        # the handle's stream

    ts_all = []

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        ts_all[:] = ts
        return median(ts), out

    res = {"rows_greedy": B, "frames": T, "encoder_rows": S_enc, "steps_cap": n_steps, "dtype": "bf16", "V": cfg.vocab,
           "D": cfg.embed_dim, "decoder_layers": cfg.decoder_layers, "reps": args.reps, "beams": {}}
    with torch.no_grad():
        sec, (toks, emit, st) = timed(lambda: dec.greedy_offline(enc, L, n_steps, T=S_enc))
        res["pooled_positions"] = int(st.P.shape[1])
        res["greedy"] = {"ms": round(sec * 1e3, 2), "ms_min_max": [round(min(ts_all) * 1e3, 2), round(max(ts_all) * 1e3, 2)], "tokens": B * n_steps, "tokens_per_s": round(B * n_steps / sec, 1)}
        print(json.dumps({"decode": "greedy", **res["greedy"]}), flush=True)
        for beam in [int(b) for b in args.beams.split(",")]:
            entry = {"rows": B * beam}
            forms = (("grouped", grouped_beam), ("composition", composition_beam))
            off = Marks(stream, on=False)
            outs, secs, splits, steps = {}, {n: [] for n, _ in forms}, {n: [] for n, _ in forms}, 0
            for name, fn in forms:                                              # warm-up of both forms
                outs[name] = fn(dec, enc, L, caps, beam, S_enc, off)
            torch.cuda.synchronize()
            for _ in range(args.reps):                                          # the two forms alternate within one pass
                for name, fn in forms:
                    t0 = time.perf_counter()
                    fn(dec, enc, L, caps, beam, S_enc, off)
                    torch.cuda.synchronize()
                    secs[name].append(time.perf_counter() - t0)
            for _ in range(args.reps):                                          # the split, in passes of their own (events cost host time)
                for name, fn in forms:
                    marks = Marks(stream)
                    fn(dec, enc, L, caps, beam, S_enc, marks)
                    torch.cuda.synchronize()
                    steps, sp = marks.split()
                    splits[name].append(sp)
            for name, _ in forms:
                sec, n_tok = median(secs[name]), int(outs[name][1][:, 0].sum())
                per = {p: round(median([s[i] for s in splits[name]]), 4) for i, p in enumerate(PHASES)}
                entry[name] = {"ms": round(sec * 1e3, 2), "ms_min_max": [round(min(secs[name]) * 1e3, 2), round(max(secs[name]) * 1e3, 2)],
                               "tokens": n_tok, "tokens_per_s": round(n_tok / sec, 1), "steps": steps,
                               "device_ms_per_step": per, "device_ms_per_step_total": round(sum(per.values()), 4)}
            g, c = outs["grouped"], outs["composition"]
            lens = g[1][:, 0].cpu()
            entry["best_hypothesis_agreement_with_composition"] = round(
                sum(bool(torch.equal(g[0][s, 0, :int(lens[s])], c[0][s, 0, :int(lens[s])])) for s in range(B)) / B, 4)
            entry["grouped_over_composition_tokens_per_s"] = round(entry["grouped"]["tokens_per_s"] /
                                                                   entry["composition"]["tokens_per_s"], 3)
            res["beams"][str(beam)] = entry
            print(json.dumps({"decode": f"beam {beam}", **entry}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
