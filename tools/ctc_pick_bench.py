#!/usr/bin/env python3
"""The CTC head's best path: the fused call (Ops.linear_pick: simulst_linear with SIMULST_EPI_ROW_PICK, no logits in memory) against
the composition the library offered before it -- ops.linear(..., EPI_BIAS_F32OUT) to fp32 logits [rows, V], then torch argmax, max
and logsumexp over them.

bf16, D = 256, V = 4096 (s2t_emformer_s / cif_transformer_s), no bias (the reference's head has none).  Shapes:
  64 x 250 rows     the bench batch (64 utterances of 1000 frames)
  1280 x 250 rows   the large offline batch
  16 rows           one stream's chunk (one segment)
  64 x 16 rows      one lockstep round of 64 streams
The rows are read through the strided view the encoder returns ([B, Te, D] with a batch stride) by the fused call; the composition
needs them contiguous and gets them so (its copy is NOT timed: the comparison is of the head alone).

Method: warm-up, then 7 passes that ALTERNATE the two forms; each pass times `inner` back-to-back calls of one form under a pair of HIP
events and reports the per-call time; the figure of a form is the median of its 7 passes (min / max beside it).  Bytes are what each
form must move through HBM, computed from the shapes: the fraction of the HBM roofline is bytes / 8 TB/s over the measured time.

Prints ONE JSON line and writes it to --out.  Run under a time limit:
    timeout -k 10 300 python tools/ctc_pick_bench.py --out profiles/ctc_pick_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_TBS = 8.0            # MI355X HBM3E peak (datasheet)
D, V = 256, 4096
SHAPES = [("64x250", 64, 250, True), ("1280x250", 1280, 250, True), ("16", 1, 16, False), ("64x16", 64, 16, False)]


def time_calls(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--passes", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    from simulst_amd._lib import EPI_BIAS_F32OUT
    from simulst_amd.ops import Ops
    ops = Ops()
    g = torch.Generator(device="cuda").manual_seed(4096)
    W = (torch.randn(V, D, generator=g, device="cuda") * 4 / D ** 0.5).to(torch.bfloat16)
    result = {"tool": "ctc_pick_bench", "dtype": "bf16", "D": D, "V": V, "passes": args.passes, "hbm_peak_TBs": HBM_PEAK_TBS, "shapes": {}}
    ok_tall = True
    for name, B, T, gated in SHAPES:
        rows = B * T
        gap = 32                                                  # the encoder's right-context rows in front of every utterance
        buf = torch.randn(B, gap + T, D, generator=g, device="cuda").to(torch.bfloat16)
        view = buf[:, gap:]                                       # what forward() returns as encoder_out_btd
        flat = view.reshape(rows, D).contiguous()
        logits = torch.empty(rows, V, device="cuda", dtype=torch.float32)

        def fused():
            return ops.linear_pick(view, W)

        def composed():
            ops.linear(flat, W, None, epilogue=EPI_BIAS_F32OUT, out=logits)
            return logits.argmax(-1), logits.max(-1).values, torch.logsumexp(logits, -1)

        # the two forms agree before they are timed (picks where the two largest logits are a rounding apart may differ)
        pf, zf, lf = fused()
        pc, zc, lc = composed()
        torch.cuda.synchronize()
        agree = float((pf.reshape(-1).long() == pc).float().mean())
        assert agree > 0.999 and float((zf.reshape(-1) - zc).abs().max()) < 1e-3 and float((lf.reshape(-1) - lc).abs().max()) < 1e-3, name
        inner = max(2, min(200, int(2e6 // rows)))
        for _ in range(2):
            time_calls(fused, inner), time_calls(composed, inner)
        tf, tc = [], []
        for _ in range(args.passes):
            tf.append(time_calls(fused, inner))
            tc.append(time_calls(composed, inner))
        bytes_fused = rows * D * 2 + V * D * 2 + rows * 12                       # rows in, the head once, (int32, fp32 pair) out
        bytes_comp = rows * D * 2 + V * D * 2 + rows * V * 4 * 4 + rows * 16     # logits written once and read by three reductions
        mf, mc = statistics.median(tf), statistics.median(tc)
        entry = {"rows": rows, "inner_calls": inner, "gated": gated,
                 "fused_ms": {"median": mf, "min": min(tf), "max": max(tf)},
                 "composition_ms": {"median": mc, "min": min(tc), "max": max(tc)},
                 "speedup": mc / mf, "bytes_fused": bytes_fused, "bytes_composition": bytes_comp,
                 "hbm_roofline_fraction_fused": bytes_fused / (HBM_PEAK_TBS * 1e12) / (mf * 1e-3),
                 "hbm_roofline_fraction_composition": bytes_comp / (HBM_PEAK_TBS * 1e12) / (mc * 1e-3),
                 "fused_tflops": 2.0 * rows * V * D / (mf * 1e-3) / 1e12, "pick_agreement": agree}
        result["shapes"][name] = entry
        if gated and mf > mc:
            ok_tall = False
        del buf, view, flat, logits
    result["fused_not_slower_at_tall_shapes"] = ok_tall
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
