#!/usr/bin/env python3
"""Scoring a given translation with the transducer: the fused pass (simulst_joiner_lattice + simulst_rnnt_forward, the
[B, S', U + 1, V] logits never written) against the composition of the entry points that existed before it.

The transducer bench shape: transducer_model_s dims (D 256, vocabulary 4096), 64 utterances x 1000 frames (250 encoder rows -> 32
pooled positions), bf16, targets of 110 tokens (111 decoder-input positions), the encoder excluded (random encoder states).

  fused         TransducerDecoder.forward_lattice (pooling, source projection, the prediction network over the whole target, the
                lattice kernel) + Ops.rnnt_forward
  composition   the same pooling, projections and prediction network, then per batch chunk that fits: the tanh rows materialised,
                simulst_linear to fp32 logits [chunk, S', U + 1, V], torch log_softmax + gather; then a torch anti-diagonal recursion.
                It lives in this tool only.
  lattice       Ops.joiner_lattice alone on the run's own P and G: its time and achieved FLOP rate (2 V D per valid cell) against the
                dense bf16 MFMA peak

Timed under HIP events after warm-up, median of the repeats with min / max; rates are scored target tokens per second.
Prints ONE JSON line (and writes it to --out).  Run each GPU step under its own time limit, e.g.
    timeout -k 10 300 python tools/transducer_score_bench.py --out profiles/r13_transducer_score_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BF16_MFMA_PEAK_TFLOPS = 2500.0          # MI355X dense bf16 matrix peak (datasheet)


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


def torch_rnnt_forward(lpb, lpl, src_len, tgt_len):
    """anti-diagonal forward recursion in torch over [B, S, U1] (every row walks the padded lattice; ll is read at its own corner)"""
    B, S, U1 = lpb.shape
    dev = lpb.device
    alpha = torch.full((B, S, U1), -float("inf"), device=dev)
    alpha[:, 0, 0] = 0
    ninf = torch.tensor(-float("inf"), device=dev)
    for d in range(1, S + U1 - 1):
        u = torch.arange(max(0, d - S + 1), min(U1 - 1, d) + 1, device=dev)
        s = d - u
        sm, um = (s - 1).clamp_min(0), (u - 1).clamp_min(0)
        vb = torch.where(s > 0, alpha[:, sm, u] + lpb[:, sm, u], ninf)
        vl = torch.where(u > 0, alpha[:, s, um] + lpl[:, s, um], ninf)
        alpha[:, s, u] = torch.logaddexp(vb, vl)
    b = torch.arange(B, device=dev)
    s_last, n = (src_len.long() - 1).clamp_min(0), tgt_len.long()
    return alpha[b, s_last, n] + lpb[b, s_last, n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--target", type=int, default=110)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--chunk-bytes", type=int, default=1 << 30, help="largest materialised logits chunk of the composition")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from simulst_amd.config import transducer_model_s
    from simulst_amd.ops import EPI_BIAS_F32OUT, Ops
    from simulst_amd.transducer import BLANK, TransducerDecoder
    from simulst_amd.weights import init_model
    ops = Ops()
    dt = torch.bfloat16
    cfg = transducer_model_s()
    dec = TransducerDecoder(cfg, init_model(cfg, seed=1), dtype=dt, ops=ops)
    B, U, V, D = args.batch, args.target, cfg.vocab, cfg.embed_dim
    rows = args.frames // 4
    g = torch.Generator().manual_seed(0)
    enc = (torch.randn(B, rows, D, generator=g) * 0.5).to(dt).cuda()
    enc_len = torch.full((B,), rows, dtype=torch.int32)
    prev = torch.cat([torch.full((B, 1), cfg.eos), torch.randint(4, V, (B, U - 1), generator=g)], 1).cuda()

    def fused():
        out = dec.forward_lattice(prev, enc, enc_len, T=rows)
        return ops.rnnt_forward(out["lp_blank"], out["lp_label"], out["src_len"], out["tgt_len"]), out

    ll_fused, out = fused()
    S, U1 = out["lp_blank"].shape[1], out["lp_blank"].shape[2]
    chunk = max(1, min(B, args.chunk_bytes // (S * U1 * V * 4)))

    def composition():
        inp, labels, tgt_len = dec.lattice_inputs(prev)
        pooled, src_len = dec.downsample(enc, enc_len, rows)
        P = ops.linear(pooled.view(B * S, D), dec.w.w_src, dec.w.b_src, epilogue=EPI_BIAS_F32OUT).view(B, S, D)
        feats = dec.features_teacher_forced(inp)
        G = ops.linear(feats.view(B * U1, D), dec.w.w_tgt, None, epilogue=EPI_BIAS_F32OUT).view(B, U1, D)
        lpb = torch.empty(B, S, U1, device=P.device)
        lpl = torch.empty(B, S, U1, device=P.device)
        for b0 in range(0, B, chunk):
            b1 = min(B, b0 + chunk)
            z = torch.tanh(P[b0:b1].unsqueeze(2) + G[b0:b1].unsqueeze(1)).to(dt).view(-1, D)
            lp = torch.log_softmax(ops.linear(z, dec.w.out_proj, None, epilogue=EPI_BIAS_F32OUT).view(b1 - b0, S, U1, V), -1)
            lpb[b0:b1] = lp[..., BLANK]
            lpl[b0:b1] = lp.gather(3, labels[b0:b1].long().view(b1 - b0, 1, U1, 1).expand(b1 - b0, S, U1, 1)).squeeze(3)
        return torch_rnnt_forward(lpb, lpl, src_len, tgt_len), lpb, lpl

    ll_comp, lpb_c, lpl_c = composition()
    torch.cuda.synchronize()
    label_cells = (torch.arange(U1, device=prev.device).view(1, 1, U1) < out["tgt_len"].view(B, 1, 1)).expand(B, S, U1)
    agree = {"ll_max_abs_diff": float((ll_fused - ll_comp).abs().max()), "ll_mean": float(ll_fused.mean()),
             "lp_blank_max_abs_diff": float((out["lp_blank"] - lpb_c).abs().max()),
             "lp_label_max_abs_diff": float(((out["lp_label"] - lpl_c).abs() * label_cells).max())}
    del lpb_c, lpl_c

    P, G = out["P"], out["G"]
    labels = dec.lattice_inputs(prev)[1]
    lpb, lpl = torch.empty_like(out["lp_blank"]), torch.empty_like(out["lp_label"])

    def lattice():
        return ops.joiner_lattice(P, G, dec.w.out_proj_fm, labels, out["src_len"], out["tgt_len"], V=V, blank=BLANK, lp_blank=lpb, lp_label=lpl)

    f_med, f_lo, f_hi = timed(lambda: fused()[0], args.warmup, args.repeats)
    c_med, c_lo, c_hi = timed(lambda: composition()[0], max(1, args.warmup // 2), max(5, args.repeats - 2))
    l_med, l_lo, l_hi = timed(lattice, args.warmup, args.repeats)
    cells = int(((torch.arange(U1, device=prev.device).view(1, U1) <= out["tgt_len"].view(B, 1)).sum(1) * out["src_len"]).sum())
    tflops = 2.0 * cells * V * D / (l_med * 1e-3) / 1e12
    res = {"tool": "transducer_score_bench", "batch": B, "frames": args.frames, "encoder_rows": rows, "pooled_positions": S,
           "target_tokens": U, "decoder_inputs": U1, "vocab": V, "dtype": "bf16", "warmup": args.warmup, "repeats": args.repeats,
           "lattice_cells": cells, "logits_bytes_never_written": cells * V * 4,
           "fused_ms": round(f_med, 3), "fused_ms_min_max": [round(f_lo, 3), round(f_hi, 3)],
           "fused_tokens_per_s": round(B * U / f_med * 1e3, 1),
           "composition_ms": round(c_med, 3), "composition_ms_min_max": [round(c_lo, 3), round(c_hi, 3)],
           "composition_tokens_per_s": round(B * U / c_med * 1e3, 1), "composition_chunk_batch": chunk,
           "fused_over_composition": round(c_med / f_med, 2),
           "lattice_kernel_ms": round(l_med, 3), "lattice_kernel_ms_min_max": [round(l_lo, 3), round(l_hi, 3)],
           "lattice_n_split": Ops.lattice_split(B, S, U1, V, dt), "lattice_tflops": round(tflops, 1),
           "lattice_fraction_of_bf16_mfma_peak": round(tflops / BF16_MFMA_PEAK_TFLOPS, 4), "agreement": agree}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
