#!/usr/bin/env python3
"""Scoring given transcripts with the CTC head: ctc.ctc_score (Ops.linear_gather: simulst_linear with SIMULST_EPI_ROW_GATHER, only the
[B, Te, L + 1] log-probabilities of the blank and the transcript's labels in memory, then ctc_align.ctc_nll over them) against the
composition the library offered before it -- ops.linear(..., EPI_BIAS_F32OUT) to fp32 logits [rows, V], torch log_softmax over them,
and torch's ctc_loss on the device.  A third form keeps the logits and log_softmax and runs the library's own recursion
(ctc_align.ctc_nll) over the full log-probabilities: it separates what the gather saves from what the recursion kernel does.

bf16, D = 256, V = 4096 (s2t_emformer_s / cif_transformer_s), no bias (the reference's head has none), transcripts of 30 random labels
with a repeated pair, every utterance at full length.  Shapes:
  64 x 250 rows     the bench batch (64 utterances of 1000 frames)
  1280 x 250 rows   the large offline batch
The rows are read through the strided view the encoder returns ([B, Te, D] with a batch stride) by ctc_score; the composition needs
them contiguous and gets them so (its copy is NOT timed: the comparison is of the head alone).

Method: warm-up, then 7 passes that ALTERNATE the forms; each pass times `inner` back-to-back calls of one form under a pair of HIP
events and reports the per-call time; the figure of a form is the median of its 7 passes (min / max beside it).  Bytes are what each
form must move through HBM, computed from the shapes.  No speed-up is asserted: the ratio is what the run records.

Prints ONE JSON line and writes it to --out.  Run under a time limit:
    timeout -k 10 400 python tools/ctc_score_bench.py --out profiles/ctc_score_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_TBS = 8.0            # MI355X HBM3E peak (datasheet)
D, V, L = 256, 4096, 30
SHAPES = [("64x250", 64, 250), ("1280x250", 1280, 250)]


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
    from simulst_amd import ctc, ctc_align
    from simulst_amd._lib import EPI_BIAS_F32OUT
    from simulst_amd.ops import Ops
    ops = Ops()
    g = torch.Generator(device="cuda").manual_seed(4096)
    W = (torch.randn(V, D, generator=g, device="cuda") * 4 / D ** 0.5).to(torch.bfloat16)
    result = {"tool": "ctc_score_bench", "dtype": "bf16", "D": D, "V": V, "target_labels": L, "passes": args.passes,
              "hbm_peak_TBs": HBM_PEAK_TBS, "shapes": {}}
    for name, B, T in SHAPES:
        rows = B * T
        gap = 32                                                  # the encoder's right-context rows in front of every utterance
        buf = torch.randn(B, gap + T, D, generator=g, device="cuda").to(torch.bfloat16)
        view = buf[:, gap:]                                       # what forward() returns as encoder_out_btd
        flat = view.reshape(rows, D).contiguous()
        logits = torch.empty(rows, V, device="cuda", dtype=torch.float32)
        tg = torch.randint(1, V, (B, L), generator=g, device="cuda")
        tg[:, 7] = tg[:, 6]
        il = torch.full((B,), T, dtype=torch.int64, device="cuda")
        tl = torch.full((B,), L, dtype=torch.int64, device="cuda")

        def fused():
            return ctc.ctc_score(ops, W, view, il, tg, tl)["nll"]

        def log_probs():
            ops.linear(flat, W, None, epilogue=EPI_BIAS_F32OUT, out=logits)
            return torch.log_softmax(logits, -1).view(B, T, V).transpose(0, 1)

        def composed_torch():
            return F.ctc_loss(log_probs(), tg, il, tl, blank=0, reduction="none")

        def composed_kernel():
            return ctc_align.ctc_nll(log_probs(), tg, il, tl, blank=0, ops=ops)

        forms = {"fused": fused, "composition_torch": composed_torch, "composition_nll_kernel": composed_kernel}
        # the forms agree before they are timed
        nf, nt, nk = fused(), composed_torch(), composed_kernel()
        torch.cuda.synchronize()
        dev_t = float((nf - nt).abs().max() / nt.abs().max())
        dev_k = float((nf - nk).abs().max() / nk.abs().max())
        assert dev_t < 1e-4 and dev_k < 1e-4, (name, dev_t, dev_k)
        inner = max(2, min(50, int(2e6 // rows)))
        for _ in range(2):
            for fn in forms.values():
                time_calls(fn, inner)
        times = {k: [] for k in forms}
        for _ in range(args.passes):
            for k, fn in forms.items():
                times[k].append(time_calls(fn, inner))
        med = {k: statistics.median(v) for k, v in times.items()}
        head = rows * D * 2 + V * D * 2                                          # rows in, the head once
        bytes_fused = head + 2 * rows * (L + 1) * 4                              # the gathered matrix written, then read by the recursion
        bytes_comp = head + 3 * rows * V * 4 + rows * (L + 1) * 32               # logits written, read and written again by log_softmax;
        #                                                                          the loss reads a 32-byte sector per gathered element
        entry = {"rows": rows, "utterances": B, "inner_calls": inner,
                 "ms": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in times.items()},
                 "speedup_over_composition_torch": med["composition_torch"] / med["fused"],
                 "speedup_over_composition_nll_kernel": med["composition_nll_kernel"] / med["fused"],
                 "bytes_fused": bytes_fused, "bytes_composition": bytes_comp,
                 "hbm_roofline_fraction_fused": bytes_fused / (HBM_PEAK_TBS * 1e12) / (med["fused"] * 1e-3),
                 "hbm_roofline_fraction_composition_torch": bytes_comp / (HBM_PEAK_TBS * 1e12) / (med["composition_torch"] * 1e-3),
                 "max_relative_difference_to_torch": dev_t, "max_relative_difference_to_nll_kernel": dev_k}
        result["shapes"][name] = entry
        del buf, view, flat, logits
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
