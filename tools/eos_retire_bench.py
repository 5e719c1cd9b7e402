"""Offline decode with and without hypotheses finalised at EOS: offline_eval.decode_batch(stop_at_eos=False) (rows leave at their
own cap, decoder.greedy_offline_ragged) against stop_at_eos=True (rows also leave at their first EOS, decoder.generate_offline +
simulst_mma_retire_rows), one launch sequence at a time on one GPU, encoder included.

Workloads: a configs[1]-shaped sequence (448 rows x 1000 frames, 110 steps each) and one ragged sequence of a rank's shard of the
synthetic length distribution (offline_eval.plan_shard_by_work, rank 3 of 8).  Weights: random init (ties the output projection to
the embedding: EOS almost never wins) and an untied projection whose EOS row is scaled by --alpha (rows end at EOS early).
Reports per case: ms per sequence (median of --reps), hypothesis tokens/s, row-steps launched, rows ending at EOS.

The retire step's own time: run once more under the kernel tracer in a process of its own, e.g.
  rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/eos_retire_bench.py --reps 2 --only-eos
and read the retire_* rows of the kernel statistics (tools/kernel_stats_summary.py)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def biased(w, cfg, alpha, seed=5):
    w = dict(w)
    W = torch.randn(cfg.vocab, cfg.embed_dim, generator=torch.Generator().manual_seed(seed)) * cfg.embed_dim ** -0.5
    W[cfg.eos] *= alpha
    w["decoder.output_projection.weight"] = W
    return w


def main(argv=None):
    from simulst_amd.config import mma_model_s
    from simulst_amd.model import SimulSTModel
    from simulst_amd.offline_eval import decode_batch, make_batch, plan_shard_by_work, synthetic_lengths, trim_hypotheses
    from simulst_amd.weights import init_model
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--alpha", type=float, default=3.0, help="scale of the EOS row of the untied output projection")
    ap.add_argument("--only-eos", action="store_true", help="the EOS-biased weights and stop_at_eos=True only (profiling runs)")
    args = ap.parse_args(argv)
    cfg = mma_model_s(simul_attn_type="waitk_fixed_pre_decision", waitk_lagging=3)
    w0 = init_model(cfg, seed=999)
    lengths = synthetic_lengths(40000)
    seqs = plan_shard_by_work(lengths, 8, 3, 1024, 3)
    ragged = seqs[len(seqs) // 2]
    flat = {i: 1000 for i in range(448)}
    work = {"configs1_448x1000": (list(range(448)), [flat[i] for i in range(448)]),
            f"shard_sequence_{len(ragged)}_rows": (list(range(len(ragged))), [lengths[i] for i in ragged])}
    weights = {"random": w0, f"eos_biased_{args.alpha}": biased(w0, cfg, args.alpha)}
    if args.only_eos:
        weights.pop("random")
    for wname, w in weights.items():
        model = SimulSTModel(cfg, w, dtype=torch.bfloat16)
        dec = model.decoder
        row_steps = []
        orig = dec.decode_steps
        dec.decode_steps = lambda st, t, n, m, rows=None: (row_steps.append(n * (rows or st.B)), orig(st, t, n, m, rows=rows))[1]
        for case, (idx, L) in work.items():
            batch = make_batch(idx, L, "cuda", torch.bfloat16)
            modes = (True,) if args.only_eos else (False, True)
            rec = {"weights": wname, "workload": case, "rows": len(idx)}
            outs = {}
            for stop in modes:
                with torch.no_grad():
                    decode_batch(model, batch, stop_at_eos=stop)          # warm-up: code objects, graph of this shape, allocator
                    torch.cuda.synchronize()
                    ts = []
                    for _ in range(args.reps):
                        row_steps.clear()
                        t0 = time.perf_counter()
                        toks = decode_batch(model, batch, stop_at_eos=stop)
                        torch.cuda.synchronize()
                        ts.append(time.perf_counter() - t0)
                ms = sorted(ts)[len(ts) // 2] * 1e3
                n_tok = int(trim_hypotheses(toks, batch[2], cfg.eos).sum())
                key = "stop_at_eos" if stop else "cap_only"
                outs[key] = toks.cpu()
                rec[key] = {"ms_per_sequence": round(ms, 2), "hyp_tokens": n_tok, "hyp_tokens_per_s": round(n_tok / ms * 1e3, 1),
                            "row_steps": sum(row_steps), "ms_all": [round(t * 1e3, 2) for t in ts]}
            if len(outs) == 2:
                a, b = outs["cap_only"], outs["stop_at_eos"]
                n = trim_hypotheses(a, batch[2], cfg.eos)
                rec["rows_ending_at_eos"] = int(sum(int(n[r]) > 0 and int(a[r, int(n[r]) - 1]) == cfg.eos for r in range(a.size(0))))
                rec["hypotheses_identical"] = all(a[r, :int(n[r])].tolist() == b[r, :int(n[r])].tolist() for r in range(a.size(0)))
                rec["stop_at_eos_over_cap_only"] = round(rec["stop_at_eos"]["ms_per_sequence"] / rec["cap_only"]["ms_per_sequence"], 4)
            print(json.dumps(rec), flush=True)
        del dec.decode_steps


if __name__ == "__main__":
    main()
