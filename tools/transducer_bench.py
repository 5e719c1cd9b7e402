"""Greedy transducer decoding (simulst_amd/transducer.py) at the bench shape, encoder excluded: 64 utterances of 1000 frames (250
encoder rows -> 32 pooled positions with --downsample 8), bf16, transducer_model_s dims, V = 4096, random-init weights whose blank row
is scaled up so that the emit positions move through the source (with plain random weights the blank never wins).

Reports
  * tokens/s of decoder.greedy_offline (pooling + source projection + 110 steps),
  * the share of a step spent in the joiner's scan + emit launches (the library's HIP-event timers, class "scan"),
  * the joiner of a step both ways, replayed over the (g, prev_emit) of every step of that run with HIP events around each:
      fused        simulst_joiner_scan + simulst_joiner_emit + simulst_linear of the emitted row + simulst_joiner_mask_blank
      composition  the straightforward form from what was there before: the tanh rows of every position materialised, simulst_linear
                   to fp32 [B S', V] logits, then the reference's tensor ops (blank forced at the last position, past positions
                   masked, argmax, first non-blank, gather).  It exists in this tool only.
and writes them to --out as one JSON object.

    python tools/transducer_bench.py --out profiles/r09_transducer_bench.json"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def composition_step(ops, dec, P, g, prev_emit, src_len):
    """the joiner step of models/transducer_model.py:163-209 over materialised [B, S', V] logits"""
    from simulst_amd.ops import EPI_BIAS_F32OUT
    B, S, D = P.shape
    z = torch.tanh(P + g.unsqueeze(1)).to(dec.dtype).view(B * S, D)
    logits = ops.linear(z, dec.w.out_proj, None, epilogue=EPI_BIAS_F32OUT).view(B, S, -1)
    last = (src_len - 1).long()
    logits[torch.arange(B, device=P.device), last, 0] = -1e4
    pos = torch.arange(S, device=P.device).view(1, S)
    preds = logits.argmax(-1)
    nonblank = preds.ne(0) & (pos >= prev_emit.view(B, 1))
    new_emit = nonblank.long().cumsum(1).eq(1).long().argmax(1)
    return new_emit, logits[torch.arange(B, device=P.device), new_emit]


def fused_step(ops, dec, st, g, prev_emit):
    from simulst_amd.ops import EPI_BIAS_F32OUT
    V = dec.cfg.vocab
    ops.joiner_scan(st.P, g, dec.w.out_proj_fm, prev_emit, st.src_len, st.blank_logit, st.best, st.best_idx, V=V)
    ops.joiner_emit(st.P, g, st.blank_logit, st.best, st.best_idx, prev_emit, st.src_len, st.z, st.at_eos, V=V)
    logits = ops.linear(st.z, dec.w.out_proj, None, epilogue=EPI_BIAS_F32OUT)
    return prev_emit, ops.joiner_mask_blank(logits, st.at_eos)


def main(argv=None):
    from simulst_amd import _lib
    from simulst_amd.config import transducer_model_s
    from simulst_amd.transducer import TransducerDecoder
    from simulst_amd.weights import init_model
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev, dt = "cuda", torch.bfloat16
    cfg = transducer_model_s()
    w = dict(init_model(cfg, seed=999))
    out_proj = w["decoder.output_projection.weight"].clone()
    out_proj[0] *= 6.0
    w["decoder.output_projection.weight"] = w["decoder.joiner.output_projection.weight"] = out_proj
    w["decoder.joiner.target_projection.weight"] = w["decoder.joiner.target_projection.weight"] * 3.0
    w["decoder.joiner.source_projection.weight"] = w["decoder.joiner.source_projection.weight"] * 4.0
    dec = TransducerDecoder(cfg, w, device=dev, dtype=dt)
    ops = dec.ops
    T, B = args.frames, args.batch
    S_enc = ((T - 1) // 2 + 1 - 1) // 2 + 1
    n_steps = int(0.1 * T + 10)
    enc = torch.randn(B, S_enc, cfg.embed_dim, generator=torch.Generator().manual_seed(1)).to(dev, dt)
    L = torch.full((B,), S_enc, dtype=torch.int32, device=dev)

    with torch.no_grad():
        dec.greedy_offline(enc, L, n_steps, T=S_enc)                       # warm-up
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            toks, emit, st = dec.greedy_offline(enc, L, n_steps, T=S_enc)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        sec = sorted(ts)[len(ts) // 2]
        # the scan + emit launches' share of a step: the library's HIP-event timers over one more run
        ops.h.timer_reset()
        ops.h.timer_enable(-1, True)
        t0 = time.perf_counter()
        dec.greedy_offline(enc, L, n_steps, T=S_enc)
        torch.cuda.synchronize()
        timed_sec = time.perf_counter() - t0
        per_class = {}
        for c, name in enumerate(_lib.KERNEL_CLASS_NAMES):
            ms, n = ops.h.timer_read(c)
            if n:
                per_class[name] = {"ms": round(ms, 3), "launches": n}
        ops.h.timer_enable(-1, False)
        device_ms = sum(v["ms"] for v in per_class.values())
        scan_ms = per_class.get("scan", {"ms": 0.0})["ms"]

        # the joiner of a step both ways, over the states of that run: g of every step is recomputed by stepping again
        st = dec.new_state(B, cap=n_steps + 2)
        dec.set_source(st, enc, L, S_enc)
        snaps = []
        tk = torch.zeros(B, device=dev, dtype=torch.int64)
        for s in range(n_steps):
            before = st.prev_emit.clone()
            dec.step(st, tk)
            snaps.append((st.g.clone(), before, st.prev_emit.clone()))
            dec.commit(st)
            tk = toks[:, s].contiguous()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        agree = 0
        for g, before, after in snaps:                                     # warm-up + agreement of the two forms
            ne, _ = composition_step(ops, dec, st.P, g, before, st.src_len)
            agree += int((ne.int() == after).sum())
        fused_ms, comp_ms = [], []
        for _ in range(args.reps):
            ev[0].record()
            for g, before, _ in snaps:
                fused_step(ops, dec, st, g, before.clone())
            ev[1].record()
            ev[2].record()
            for g, before, _ in snaps:
                composition_step(ops, dec, st.P, g, before, st.src_len)
            ev[3].record()
            torch.cuda.synchronize()
            fused_ms.append(ev[0].elapsed_time(ev[1]) / len(snaps))
            comp_ms.append(ev[2].elapsed_time(ev[3]) / len(snaps))
    S = st.P.shape[1]
    scanned = float(sum(int((st.src_len - b).sum()) for _, b, _ in snaps)) / len(snaps)
    res = {"rows": B, "frames": T, "encoder_rows": S_enc, "pooled_positions": S, "steps": n_steps, "dtype": "bf16", "V": cfg.vocab,
           "D": cfg.embed_dim, "decoder_layers": cfg.decoder_layers, "n_split": int(st.best.shape[2]),
           "greedy_ms_per_batch": round(sec * 1e3, 2), "tokens_per_s": round(B * n_steps / sec, 1),
           "timed_run_ms": round(timed_sec * 1e3, 2), "device_ms_by_class": per_class,
           "scan_emit_ms_per_step": round(scan_ms / n_steps, 4), "scan_emit_share_of_device_time": round(scan_ms / max(device_ms, 1e-9), 4),
           "joiner_fused_ms_per_step": round(sorted(fused_ms)[len(fused_ms) // 2], 4),
           "joiner_composition_ms_per_step": round(sorted(comp_ms)[len(comp_ms) // 2], 4),
           "composition_emit_agreement": round(agree / (B * len(snaps)), 4),
           "mean_scanned_positions_per_step": round(scanned, 1),
           "scan_gflop_per_step_mean": round(2 * scanned * cfg.vocab * cfg.embed_dim / 1e9, 3),
           "distinct_emit_positions": int(emit.unique().numel())}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
