"""Offline beam search against greedy decode on the configs[1] shape: 64 sentences x 1000 frames, bf16, wait-k 5, cap
int(0.1 T + 10) = 110 tokens.  Greedy is MMADecoder.generate_offline(stop_at_eos=True) (the device decode loop with EOS retirement);
beam N is MMADecoder.beam_offline (per-op decoder step over 64 N rows + the four beam kernels).  Tokens are counted as
eval/generate.py counts them: the best hypothesis of each sentence, EOS included.  Encoder excluded (the same for both).

Per beam width it also splits each step's device time between the decoder step and the beam kernels (topk, select, reorder) with
events on the handle's stream.  The kernels' own times come from the kernel tracer, in a process of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/beam_bench.py --reps 1 --beams 5
  python tools/beam_bench.py --kernel-stats OUT/.../run_kernel_stats.csv        # share of the beam_* kernels in all kernel time"""
import argparse
import csv
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def kernel_stats(path):
    """share of the beam kernels in the kernel time of a rocprofv3 --stats CSV"""
    tot, beam, rows = 0.0, 0.0, {}
    for r in csv.DictReader(open(path)):
        ns = float(r["TotalDurationNs"]) if "TotalDurationNs" in r else float(r["AverageNs"]) * int(r["Calls"])
        tot += ns
        if "beam_" in r["Name"]:
            beam += ns
            name = r["Name"].split("(")[0].replace("void ", "").replace("(anonymous namespace)::", "")
            rows[name] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2)}
    print(json.dumps({"beam_kernels": rows, "beam_share_of_kernel_time": round(beam / max(tot, 1.0), 4)}))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--beams", default="1,4,5")
    ap.add_argument("--sentences", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--kernel-stats", default=None, help="summarise a rocprofv3 kernel statistics CSV instead of running")
    args = ap.parse_args(argv)
    if args.kernel_stats is not None:
        return kernel_stats(args.kernel_stats)
    from simulst_amd.config import mma_model_s
    from simulst_amd.model import SimulSTModel
    from simulst_amd.offline_eval import make_batch, max_steps
    from simulst_amd.weights import init_model
    cfg = mma_model_s(simul_attn_type="waitk_fixed_pre_decision", waitk_lagging=5)
    model = SimulSTModel(cfg, init_model(cfg, seed=999), dtype=torch.bfloat16)
    n = args.sentences
    fb, Ld, L, steps, Tpad = make_batch(list(range(n)), [args.frames] * n, "cuda", torch.bfloat16)
    caps = [max_steps(int(t)) for t in L]
    dec = model.decoder
    with torch.no_grad():
        enc = model.encoder.forward(fb, Ld)
    e, el = enc["encoder_out_btd"], enc["encoder_lengths"]

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return sorted(ts)[len(ts) // 2], out

    with torch.no_grad():
        s, (hyp, lens, _) = timed(lambda: dec.generate_offline(e, el, caps, stop_at_eos=True))
        n_tok = int(lens.sum())
        print(json.dumps({"decode": "greedy generate_offline(stop_at_eos=True)", "sentences": n, "ms": round(s * 1e3, 2),
                          "tokens": n_tok, "tokens_per_s": round(n_tok / s, 1)}), flush=True)
        for beam in [int(b) for b in args.beams.split(",")]:
            s, out = timed(lambda: dec.beam_offline(e, el, caps, beam=beam))
            n_tok = int(out[1][:, 0].sum())
            # per-step split of the device time: events around the decoder step and around the beam kernels of each step
            split = {"step": 0.0, "beam_kernels": 0.0}
            evs = []
            orig_step, orig_reorder = dec.step, dec.ops.beam_reorder
            stream = torch.cuda.ExternalStream(dec.ops.h.stream_ptr) if getattr(dec.ops.h, "stream_ptr", None) else \
                torch.cuda.current_stream()

            def mark():
                ev = torch.cuda.Event(enable_timing=True)
                ev.record(stream)
                evs.append(ev)

            def step(*a, **k):
                mark()
                r = orig_step(*a, **k)
                mark()
                return r

            def reorder(*a, **k):
                r = orig_reorder(*a, **k)
                mark()
                return r

            dec.step, dec.ops.beam_reorder = step, reorder
            try:
                dec.beam_offline(e, el, caps, beam=beam)
                torch.cuda.synchronize()
            finally:
                del dec.step
                dec.ops.beam_reorder = orig_reorder
            for i in range(0, len(evs) - 2, 3):
                split["step"] += evs[i].elapsed_time(evs[i + 1])
                split["beam_kernels"] += evs[i + 1].elapsed_time(evs[i + 2])
            n_steps = len(evs) // 3
            print(json.dumps({"decode": f"beam {beam}", "sentences": n, "rows": n * beam, "ms": round(s * 1e3, 2), "tokens": n_tok,
                              "tokens_per_s": round(n_tok / s, 1), "steps": n_steps,
                              "ms_per_step_decoder": round(split["step"] / max(n_steps, 1), 3),
                              "ms_per_step_beam_kernels": round(split["beam_kernels"] / max(n_steps, 1), 3),
                              "beam_share_of_step": round(split["beam_kernels"] / max(split["step"] + split["beam_kernels"], 1e-9), 4)}),
                  flush=True)


if __name__ == "__main__":
    main()
