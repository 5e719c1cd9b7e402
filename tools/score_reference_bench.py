#!/usr/bin/env python3
"""Scoring a given translation: the one-pass (whole-target) decoder forward against the same scoring done position by position.

configs[1] dims (mma_model_s decoder: D 256, 4 heads, 6 layers, vocabulary 4096), 64 utterances x 1000 frames (250 encoder rows),
bf16, wait-k 5 with fixed pre-decision ratio 8, targets of 110 tokens; the encoder is excluded (random encoder states).

  one_pass       MMADecoder.forward_teacher_forced over [eos] + target[:-1] (the K / V projections of the source included)
  step_by_step   the same tokens through decoder.step + decoder.commit, one position at a time (the form that existed before the
                 whole-target pass; K / V projections included as well)
  + the one-pass form of hard_aligned_fixed_pre_decision and infinite_lookback_fixed_pre_decision

Timed under HIP events after warm-up, median of the repeats; rates are scored target tokens per second.  Prints ONE JSON line.
Run each GPU step under its own time limit, e.g.  timeout -k 10 300 python tools/score_reference_bench.py
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--target", type=int, default=110)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--classes", action="store_true", help="also time the one-pass form per kernel class (library timers)")
    args = ap.parse_args()
    from simulst_amd import _lib
    from simulst_amd.config import mma_model_s
    from simulst_amd.decoder import MMADecoder
    from simulst_amd.ops import Ops
    from simulst_amd.weights import init_model
    ops = Ops()
    B, U = args.batch, args.target
    S = args.frames // 4
    g = torch.Generator().manual_seed(0)
    enc = (torch.randn(B, S, 256, generator=g) * 0.5).to(torch.bfloat16).cuda()
    enc_len = torch.full((B,), S, dtype=torch.int32)
    res = {"tool": "score_reference_bench", "batch": B, "frames": args.frames, "encoder_rows": S, "target_tokens": U, "dtype": "bf16",
           "warmup": args.warmup, "repeats": args.repeats}
    for name in ("waitk_fixed_pre_decision", "hard_aligned_fixed_pre_decision", "infinite_lookback_fixed_pre_decision"):
        cfg = mma_model_s(simul_attn_type=name, waitk_lagging=5, fixed_pre_decision_ratio=8)
        dec = MMADecoder(cfg, init_model(cfg, seed=1), dtype=torch.bfloat16, ops=ops)
        tokens = torch.cat([torch.full((B, 1), cfg.eos), torch.randint(4, cfg.vocab, (B, U - 1), generator=g)], 1).cuda()

        def one_pass():
            return dec.forward_teacher_forced(tokens, enc, enc_len, want_attn=False)[0]

        med, lo, hi = timed(one_pass, args.warmup, args.repeats)
        res[name] = {"one_pass_ms": round(med, 3), "one_pass_ms_min_max": [round(lo, 3), round(hi, 3)],
                     "one_pass_tokens_per_s": round(B * U / med * 1e3, 1)}
        if name == "waitk_fixed_pre_decision":
            cols = [tokens[:, u].contiguous() for u in range(U)]

            def step_by_step():
                st = dec._offline_state(B, U, S, None, None)
                dec.append_encoder_out(st, enc, enc_len)
                for u in range(U):
                    logits, _ = dec.step(st, cols[u])
                    dec.commit(st)
                return logits

            med_s, lo_s, hi_s = timed(step_by_step, max(1, args.warmup // 2), max(3, args.repeats // 3))
            res[name].update({"step_by_step_ms": round(med_s, 3), "step_by_step_ms_min_max": [round(lo_s, 3), round(hi_s, 3)],
                              "step_by_step_tokens_per_s": round(B * U / med_s * 1e3, 1),
                              "one_pass_over_step_by_step": round(med_s / med, 2)})
        if args.classes:
            ops.h.timer_enable(-1, True)
            ops.h.timer_reset()
            one_pass()
            torch.cuda.synchronize()
            res[name]["one_pass_ms_by_class"] = {_lib.KERNEL_CLASS_NAMES[c]: round(ops.h.timer_read(c)[0], 3)
                                                 for c in range(_lib.K_COUNT) if ops.h.timer_read(c)[1] > 0}
            ops.h.timer_enable(-1, False)
            ops.h.timer_reset()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
