#!/usr/bin/env python3
"""The CTC head's n-best path: (a) the per-frame candidates -- the fused call (Ops.linear_topk(k=8, keep=0): simulst_linear with
SIMULST_EPI_ROW_TOPK, no logits in memory) against the composition the library offered before it -- ops.linear(..., EPI_BIAS_F32OUT) to
fp32 logits [rows, V], then torch.topk and logsumexp over them; (b) the whole prefix beam search (ctc.ctc_prefix_beam_search, beam 8,
8 candidates) at 64 x 250 and 1280 x 250 rows, and one chunk of 64 x 16 rows continuing a search over 234 rows from its state, in three
forms: the search whose recursion is ONE launch (csrc/ctc_prefix.hip), the same search with the recursion as torch tensor operations
(composed=True: the code path before the kernel) and ctc.ctc_greedy -- with the recursion launch's own time (the handle's timer over
the launch; and HIP events around ctc_prefix_beam_advance, which adds the state's copies) beside the top-k launch's, and the device
launches of one search in both forms.

bf16, D = 256, V = 4096 (s2t_emformer_s / cif_transformer_s), no bias (the reference's head has none).  Shapes of (a):
  64 x 250 rows     the bench batch (64 utterances of 1000 frames)
  1280 x 250 rows   the large offline batch
  16 rows           one stream's chunk (one segment)
  64 x 16 rows      one lockstep round of 64 streams
The rows are read through the strided view the encoder returns ([B, Te, D] with a batch stride) by the fused call; the composition
needs them contiguous and gets them so (its copy is NOT timed: the comparison is of the head alone).

Method: warm-up, then 7 passes that ALTERNATE the forms; each pass times `inner` back-to-back calls of one form under a pair of HIP
events and reports the per-call time; the figure of a form is the median of its 7 passes (min / max beside it).  Bytes are what each
form must move through HBM, computed from the shapes.

Prints ONE JSON line and writes it to --out.  Run under a time limit:
    timeout -k 10 600 python tools/ctc_beam_bench.py --out profiles/ctc_prefix_beam_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_TBS = 8.0            # MI355X HBM3E peak (datasheet)
D, V, K_CAND, BLANK = 256, 4096, 8, 0
SHAPES = [("64x250", 64, 250), ("1280x250", 1280, 250), ("16", 1, 16), ("64x16", 64, 16)]


def time_calls(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def stats(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def composed_candidates(ops, flat, W, logits, B, T):
    """the candidate lists in ctc.ctc_topk's form from materialised logits"""
    from simulst_amd._lib import EPI_BIAS_F32OUT
    ops.linear(flat, W, None, epilogue=EPI_BIAS_F32OUT, out=logits)
    lse = torch.logsumexp(logits, -1)
    zb = logits[:, BLANK].clone()
    logits[:, BLANK] = float("-inf")
    top = torch.topk(logits, K_CAND, dim=-1)
    ids = torch.cat([torch.full_like(top.indices[:, :1], BLANK), top.indices], 1).to(torch.int32)
    lprob = torch.cat([zb.unsqueeze(1), top.values], 1) - lse.unsqueeze(1)
    return ids.view(B, T, K_CAND + 1), lprob.view(B, T, K_CAND + 1), lse.view(B, T)


def count_launches(fn):
    """device launches of one call, from a torch profiler trace; None (and why) where the profiler gives no device events"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
        return (n, None) if n else (None, "the profiler recorded no device events")
    except Exception as ex:  # noqa: BLE001 -- the count is an extra; the timings stand without it
        return None, f"{type(ex).__name__}: {ex}"


SEARCH_SHAPES = ("64x250", "1280x250", "64x16")


def search_block(ops, W, view, B, T, passes, chunk_after=0, gen=None):
    """(b): beam 8, 8 candidates over view [B, T, D]; chunk_after > 0: the T rows continue a search over that many earlier rows"""
    from simulst_amd import _lib, ctc
    lens = torch.full((B,), T, device="cuda", dtype=torch.int64)
    state = None
    if chunk_after:
        before = torch.randn(B, chunk_after, D, generator=gen, device="cuda").to(torch.bfloat16)
        state = ctc.ctc_prefix_beam_search(ops, W, before, torch.full_like(lens, chunk_after), beam=8, candidates=K_CAND, return_state=True)["state"]
    cand = ctc.ctc_topk(ops, W, view, lens, k=K_CAND)
    st0 = state if state is not None else ctc.ctc_prefix_beam_init(B, 8, "cuda")

    def search(composed=False):
        return ctc.ctc_prefix_beam_search(ops, W, view, lens, beam=8, candidates=K_CAND, nbest=1, state=state, composed=composed)

    forms = {"search": search, "search_composed": lambda: search(True), "greedy": lambda: ctc.ctc_greedy(ops, W, view, lens),
             "topk": lambda: ctc.ctc_topk(ops, W, view, lens, k=K_CAND),
             "advance": lambda: ctc.ctc_prefix_beam_advance(cand["ids"], cand["lprob"], lens, st0, ops=ops)}
    a, b = search(), search(True)
    torch.cuda.synchronize()
    same_best = float((a["n"] == b["n"]).float().mean())
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(passes):
        for k, fn in forms.items():
            times[k].append(time_calls(fn, 1))
    kern = []                                                      # the recursion launch alone: the handle's event pair around it
    for _ in range(passes):
        ops.h.timer_reset()
        ops.h.timer_enable(_lib.K_SCAN, True)
        forms["advance"]()
        torch.cuda.synchronize()
        kern.append(ops.h.timer_read(_lib.K_SCAN)[0])
        ops.h.timer_enable(_lib.K_SCAN, False)
    ops.h.timer_reset()
    n_launch, why = count_launches(search)
    n_comp, why_c = count_launches(lambda: search(True))
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"beam": 8, "candidates": K_CAND, "utterances": B, "frames": T, "frames_before_in_state": chunk_after,
            **{k + "_ms": stats(v) for k, v in times.items()}, "recursion_kernel_ms": stats(kern),
            "search_speedup_over_composed": med["search_composed"] / med["search"],
            "search_over_greedy": med["search"] / med["greedy"],
            "recursion_kernel_share_of_search": statistics.median(kern) / med["search"],
            "topk_share_of_search": med["topk"] / med["search"],
            "best_length_agreement_with_composed": same_best,
            "launches_per_search": n_launch, "launches_per_search_composed": n_comp, "launch_count_note": why or why_c}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--passes", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    from simulst_amd.ops import Ops
    ops = Ops()
    g = torch.Generator(device="cuda").manual_seed(4096)
    W = (torch.randn(V, D, generator=g, device="cuda") * 4 / D ** 0.5).to(torch.bfloat16)
    result = {"tool": "ctc_beam_bench", "dtype": "bf16", "D": D, "V": V, "k": K_CAND, "keep": BLANK, "passes": args.passes,
              "hbm_peak_TBs": HBM_PEAK_TBS, "shapes": {}}
    faster_everywhere = True
    for name, B, T in SHAPES:
        rows = B * T
        gap = 32                                                  # the encoder's right-context rows in front of every utterance
        buf = torch.randn(B, gap + T, D, generator=g, device="cuda").to(torch.bfloat16)
        view = buf[:, gap:]                                       # what forward() returns as encoder_out_btd
        flat = view.reshape(rows, D).contiguous()
        logits = torch.empty(rows, V, device="cuda", dtype=torch.float32)

        def fused():
            return ops.linear_topk(view, W, k=K_CAND, keep=BLANK)

        def composed():
            return composed_candidates(ops, flat, W, logits, B, T)

        # the two forms agree before they are timed (ranks whose logits are a rounding apart may swap)
        i_f, l_f, s_f = fused()
        i_c, l_c, s_c = composed()
        torch.cuda.synchronize()
        agree = float((i_f == i_c).float().mean())
        assert agree > 0.999 and float((l_f - l_c).abs().max()) < 1e-3 and float((s_f - s_c).abs().max()) < 1e-3, (name, agree)
        inner = max(2, min(200, int(2e6 // rows)))
        for _ in range(2):
            time_calls(fused, inner), time_calls(composed, inner)
        tf, tc = [], []
        for _ in range(args.passes):
            tf.append(time_calls(fused, inner))
            tc.append(time_calls(composed, inner))
        kp = K_CAND + 1
        bytes_fused = rows * D * 2 + V * D * 2 + rows * (kp * 8 + 4)             # rows in, the head once, k' (int32, fp32) + lse out
        bytes_comp = rows * D * 2 + V * D * 2 + rows * V * 4 * 4 + rows * (kp * 12 + 4)   # logits written, read by logsumexp, topk, masked
        mf, mc = statistics.median(tf), statistics.median(tc)
        result["shapes"][name] = {"rows": rows, "inner_calls": inner, "fused_ms": stats(tf), "composition_ms": stats(tc),
                                  "speedup": mc / mf, "bytes_fused": bytes_fused, "bytes_composition": bytes_comp,
                                  "hbm_roofline_fraction_fused": bytes_fused / (HBM_PEAK_TBS * 1e12) / (mf * 1e-3),
                                  "fused_tflops": 2.0 * rows * V * D / (mf * 1e-3) / 1e12, "id_agreement": agree}
        faster_everywhere = faster_everywhere and mf < mc
        if name in SEARCH_SHAPES:
            result["search_" + name] = search_block(ops, W, view, B, T, args.passes, chunk_after=234 if name == "64x16" else 0, gen=g)
        del buf, view, flat, logits
    result["topk_faster_than_composition_at_every_shape"] = faster_everywhere
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
