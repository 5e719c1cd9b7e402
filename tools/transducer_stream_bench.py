"""Simultaneous transducer decoding (simulst_amd/transducer_agent.py) at the bench shape: 64 streams of 1000 frames, bf16,
transducer_model_s dims, random-init weights whose blank row is scaled up as in tools/transducer_bench.py (with plain random weights
the blank never wins and no row ever waits).

Reports
  * tokens/s and the mean Average Lagging of the lockstep (microphone) form and of the self-paced (evaluation) form, the encoder
    included (chunk by chunk in both),
  * the resume step of waiting rows -- the first step_online behind a new chunk, when every live row waits -- with the cached g (the
    scan of the new positions + emit + the emitted row's logits) against the same run with recompute_g=True (prediction network and
    the whole scan again): HIP events around the step, and the library's kernel timers inside it,
and writes them to --out as one JSON object.  No threshold is attached to any of them.

    python tools/transducer_stream_bench.py --out profiles/transducer_stream_bench.json"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def median(xs):
    return sorted(xs)[len(xs) // 2] if xs else None


def resume_steps(agent, states, positions, schedule, recompute):
    """the lockstep loop over given encoder states with HIP events around every resume step -> (event ms per resume step, kernel ms
    per resume step, tokens written)"""
    model, dec = agent.model, agent.model.decoder
    ops, cfg, dev = model.ops, model.cfg, model.device
    B = states.size(0)
    st = agent._new_state(B, positions[-1])
    toks = torch.full((B,), cfg.eos, device=dev, dtype=torch.int64)
    n_tok = torch.zeros(B, device=dev, dtype=torch.int64)
    ev_ms, k_ms, written = [], [], 0
    for c, pos in enumerate(positions):
        dec.append_source(st, states[:, (schedule[c - 1] if c else 0):schedule[c]], schedule[c] - (schedule[c - 1] if c else 0),
                          c == len(positions) - 1)
        cap = agent.max_len(pos)
        first_round = True
        while True:
            timed = first_round and c > 0 and st.n_wrote == 0             # every live row waits on its cached g
            if timed:
                ops.h.timer_reset()
                ops.h.timer_enable(-1, True)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            logits, wrote = dec.step_online(st, toks, recompute_g=recompute)
            if timed:
                e1.record()
                torch.cuda.synchronize()
                ev_ms.append(e0.elapsed_time(e1))
                k_ms.append(sum(ops.h.timer_read(k)[0] for k in range(len(_lib().KERNEL_CLASS_NAMES))))
                ops.h.timer_enable(-1, False)
            first_round = False
            if st.n_wrote == 0:
                break
            pick = torch.where(n_tok == 0, agent._pick(logits, True), agent._pick(logits, False))
            toks = torch.where(wrote, pick, toks)
            n_tok += wrote
            written += int(wrote.sum())
            ended = wrote & ((pick == cfg.eos) | (n_tok > cap))
            if bool(ended.any()):
                st.done |= ended.to(torch.int32)
                dec.sync_source(st)
        if bool((st.done != 0).all()):
            break
    return ev_ms, k_ms, written


def _lib():
    from simulst_amd import _lib as lib
    return lib


def main(argv=None):
    from simulst_amd.config import transducer_model_s
    from simulst_amd.transducer import TransducerModel
    from simulst_amd.transducer_agent import BatchedTransducerStreamingAgent
    from simulst_amd.weights import init_model
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=3)
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
    model = TransducerModel(cfg, w, device=dev, dtype=dt)
    B, T = args.batch, args.frames
    fb = torch.randn(B, T, 80, generator=torch.Generator().manual_seed(1)).to(dev)
    agent = BatchedTransducerStreamingAgent(model, max_len_a=0.1, max_len_b=10)
    res = {"rows": B, "frames": T, "dtype": "bf16", "V": cfg.vocab, "D": cfg.embed_dim, "decoder_layers": cfg.decoder_layers,
           "downsample": cfg.downsample}
    with torch.no_grad():
        for name, kw in (("lockstep", dict()), ("self_paced", dict(self_paced=True))):
            agent.run_batch(fb, **kw)                                      # warm-up
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                recs = agent.run_batch(fb, **kw)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            n = sum(len(r["tokens"]) for r in recs)
            res[name] = {"ms_per_batch": round(median(ts) * 1e3, 2), "tokens": n, "tokens_per_s": round(n / median(ts), 1),
                         "AL_ms_mean": round(sum(r["AL"] for r in recs) / B, 1),
                         "reads_mean": round(sum(r["actions"].count("R") for r in recs) / B, 2),
                         "distinct_emit_positions": len({e for r in recs for e in r["emit"]})}
        res["records_equal"] = all(a[k] == b[k] for a, b in zip(agent.run_batch(fb), agent.run_batch(fb, self_paced=True))
                                   for k in ("tokens", "delays_ms", "actions", "emit"))
        from simulst_amd.stream_source import offline_states
        sched = agent._schedule(T)
        positions, schedule = sched.positions, sched.rows
        states, _ = offline_states(model.encoder, fb, [T] * B, [sched] * B)
        for name, rc in (("cached_g", False), ("recompute_g", True)):
            resume_steps(agent, states, positions, schedule, rc)           # warm-up
            ev, km, written = resume_steps(agent, states, positions, schedule, rc)
            res["resume_step_" + name] = {"steps_timed": len(ev), "event_ms_median": round(median(ev), 4) if ev else None,
                                          "kernel_ms_median": round(median(km), 4) if km else None, "tokens": written}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
