"""Offline decode rates of the s2t_emformer model (full encoder-decoder attention, SIMULST_ATTN_FULL) against wait-k 5 with ratio 8
(mma_model_s) on the same box, encoder excluded: 64 utterances of 1000 frames (250 encoder rows each), bf16, s2t_emformer_s dims,
random-init weights (tied output projection: EOS rarely wins, so rows run to their cap of int(0.1 T + 10) = 110 tokens).

Per model: greedy decoder.generate_offline(stop_at_eos=True) and beam search (decoder.beam_offline) at beam 1 and 5 -- ms per
batch (median of --reps) and hypothesis tokens/s (EOS excluded).  One JSON line per case.

--kernel-shapes: instead, run the FULL decode loop at 448 and 1024 rows over 250 and 750 keys (--kernel-steps steps each) for a kernel
trace, e.g.
  rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/s2t_decode_bench.py --kernel-shapes
Bytes per step of the cross-attention = rows x layers x keys x 2 D x 2 B (K and V, bf16)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def bench_case(fn, reps):
    fn()                                      # warm-up: code objects, graph of this shape, allocator
    torch.cuda.synchronize()
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2], out


def main(argv=None):
    from simulst_amd.config import mma_model_s, s2t_emformer_s
    from simulst_amd.decoder import MMADecoder
    from simulst_amd.weights import init_model
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--kernel-shapes", action="store_true")
    ap.add_argument("--kernel-steps", type=int, default=16)
    args = ap.parse_args(argv)
    dt = torch.bfloat16
    dev = "cuda"
    full = s2t_emformer_s()
    if args.kernel_shapes:
        dec = MMADecoder(full, init_model(full, seed=999), device=dev, dtype=dt)
        for rows in (448, 1024):
            for keys in (250, 750):
                enc = torch.randn(rows, keys, full.embed_dim, generator=torch.Generator().manual_seed(keys)).to(dev, dt)
                L = torch.full((rows,), keys, dtype=torch.int32, device=dev)
                dec.greedy_offline(enc, L, args.kernel_steps, mask_eos=False)
                torch.cuda.synchronize()
                gb = rows * full.decoder_layers * keys * 2 * full.embed_dim * 2 / 1e9
                print(json.dumps({"rows": rows, "keys": keys, "steps": args.kernel_steps, "cross_attn_GB_per_step": round(gb, 3)}))
        return
    T = args.frames
    S = ((T - 1) // 2 + 1 - 1) // 2 + 1                   # encoder rows after the two stride-2 convolutions
    B = args.batch
    cap = min(int(0.1 * T + 10), full.max_target_positions - 1)
    enc = torch.randn(B, S, full.embed_dim, generator=torch.Generator().manual_seed(1)).to(dev, dt)
    L = torch.full((B,), S, dtype=torch.int32, device=dev)
    models = {"s2t_emformer_full": full, "mma_model_waitk5_r8": mma_model_s(simul_attn_type="waitk_fixed_pre_decision", waitk_lagging=5)}
    for name, cfg in models.items():
        dec = MMADecoder(cfg, init_model(cfg, seed=999), device=dev, dtype=dt)
        cases = {"greedy_stop_at_eos": lambda: dec.generate_offline(enc, L, [cap] * B, stop_at_eos=True)[:2]}
        for beam in (1, 5):
            cases[f"beam{beam}"] = (lambda beam=beam: (lambda r: (r[0][:, 0], r[1][:, 0]))(
                dec.beam_offline(enc, L, cap, beam=beam, nbest=1)))
        for case, fn in cases.items():
            with torch.no_grad():
                sec, (toks, lengths) = bench_case(fn, args.reps)
            n_tok = int((toks != cfg.padding_idx).sum() - (toks == cfg.eos).sum())
            print(json.dumps({"model": name, "case": case, "rows": B, "frames": T, "keys": S, "cap": cap, "dtype": "bf16",
                              "ms_per_batch": round(sec * 1e3, 2), "tokens": n_tok, "tokens_per_s": round(n_tok / sec, 1)}))


if __name__ == "__main__":
    main()
