"""simulst_policy_cross_attention (csrc/decode_driver.hip: policy_cross_attn_kernel, and for long wait-k / full-attention sources
waitk_cross_attn_block_kernel + cross_attn_merge_kernel) and the unfused triple it promises to equal (simulst_step_p_choose +
simulst_mma_step_search + simulst_decoder_cross_attention) against a plain fp64 reference of the operation, at the edges of the
kernel's branches: four attention types, both pre-decision poolings at ratios 1 .. 8, the flags, every value-aggregation path.

The reference (`reference`) takes what the entry point takes and never restates the kernel's index arithmetic: the step
probabilities are oracle.monotonic.p_choose on float64 tensors (identity projections: the entry point receives projected queries
and keys, and pooling commutes with the projection), one utterance at a time (the per-utterance semantics of the header); wait-k
builds the oracle's one-hot p_choose and runs the SAME generic oracle.monotonic.step_search as the learned policies, which is
what checks the kernel's closed form; the soft energies are oracle.monotonic.energy_from_qk, the softmax over keys <= step with
"zero while the head has not moved" is restated from attention_infer (which itself casts to fp32).  The CPU tests pin it to the
fixtures recorded from the reference implementation (g6, g7, g19, g20) before it is used on the GPU.

Decisions (head_step, head_read) must equal the reference exactly in fp32 and bf16.  That is fair because the inputs are drawn so
that |energy + energy_bias| >= 1e-3 at every pooled key of the reference (asserted before every GPU call): both dtype paths pool
and dot in fp32 over inputs the reference sees exactly, and an fp32 dot of d <= 64 O(1) terms errs by orders of magnitude less.

Bounds on ctx.  Hard-aligned: a gather, bit-identical to the V row the reference names, exactly zero for a dead row.  fp32:
atol 2e-5, rtol 1e-4 (the project's fp32 attention bound).  bf16: the operands are exact in the reference; scores, softmax and
P.V are fp32, P is NOT rounded, the key-block path adds fp32 partials -- so the one bf16 rounding is the store.  The stored value x
is a convex combination of the attended V values, |x| <= max_j |v_j|; a bf16 rounding errs by at most 2^-9 relative to the top of
x's binade, i.e. by at most 2^-8 |x| = 2 * 2^-9 |x|.  Asserted per (row, head, channel): |got - ref| <= 2 * 2^-9 * max_j |v_j|
over the keys j the reference attends (BF16_C = 2).  The fp32 terms (~2^-22 relative) are not added to the bound: they matter only
if |x| lies within 2^-14 of max |v_j| AND of a power of two, i.e. all weight on one key, where the result is that key's value
exactly.

key_len[b] == 0 is reachable (the offline entry points of decoder.py pass the caller's enc_len through unchecked, and the
subsampler's length formula maps an empty utterance to 0 rows); the kernels write a zero ctx row for it without loading a key or
value row (include/simulst_hip.h), which the `empty_*` cases check.  The oracle has no answer for an empty source (its step search
indexes position -1), so the reference states the header's convention for it.

Found by these cases and fixed: the row-per-lane attention core that simulst_decoder_cross_attention (and
simulst_decoder_self_attention) uses for head dims without a lanes-per-row instantiation covers 256 / (d / 4) * (d / 4) key rows
-- 252 at d = 24, 250 at d = 40 -- and was given up to 256, dropping the last rows from P.V; such key ranges now take the looped
path (attn::row_lane_rows).  test_decoder_self_attention_row_lane_limit holds the self-attention kernel to the same reference
across that limit.

test_reference_mutations_change_a_case (CPU) shows the cases can fail: each of eight one-off mistakes, applied to the reference,
changes a decision or moves ctx by more than 10 x the bf16 bound on at least one case.
"""
import functools

import pytest
import torch

from conftest import load_golden, split_weights
from oracle import monotonic as omo

SENTINEL = 123.0                       # exact in bf16
STEP_SENTINEL, READ_SENTINEL = 77, 9
BF16_C = 2.0
BF16_BOUND = BF16_C * 2.0 ** -9
MARGIN = 1e-3
DTYPES = (torch.float32, torch.bfloat16)
LEARNED = ("hard_aligned", "infinite_lookback", "chunkwise")
MUTATIONS = ("window_shift", "no_floor_trim", "no_last_col", "stop_at_len", "past_le", "keys_lt_step", "waitk_off_by_one",
             "no_zero_unmoved")


def _case(attn, d, H, S_cap, ratio, lens, hs=None, mp=True, bias=0.0, k=3, tgt=None, online=False):
    B = len(lens)
    hs = list(hs) if hs is not None else (["0", "mid", "cand", "len-1", "past", "len"] * 2)[:B]
    tgt = list(tgt) if tgt is not None else (["0", "mid", "P-k", "beyond", "mid", "0"] * 2)[:B]
    assert len(hs) == B and len(tgt) == B and B <= 6 and H * d <= 256 and S_cap <= 513 and max(lens) <= S_cap
    return dict(attn=attn, d=d, H=H, S_cap=S_cap, ratio=ratio, lens=list(lens), hs=hs, mp=mp, bias=bias, k=k, tgt=tgt, online=online)


# row lengths: 1, 2, |ratio| - 1, |ratio|, |ratio| + 1, a multiple (+ 1), S_cap - 1, S_cap; around the key blocks 255 / 256 / 257 / 100
CASES = {
    # ---- hard_aligned: the gather
    "hard_d16_r1_S24": _case("hard_aligned", 16, 4, 24, 1, [1, 2, 23, 24, 12, 7]),
    "hard_d8_r2_S24_nomp_bias": _case("hard_aligned", 8, 3, 24, 2, [1, 2, 3, 4, 5, 24], hs=["0", "len", "0", "mid", "len", "past"],
                                      mp=False, bias=-0.5),
    "hard_d24_r4_S64": _case("hard_aligned", 24, 3, 64, 4, [3, 4, 5, 8, 9, 64]),
    "hard_d32_r8_S64_bias": _case("hard_aligned", 32, 1, 64, 8, [7, 8, 9, 16, 17, 63], bias=-0.5),
    "hard_d40_last2_S24_nomp": _case("hard_aligned", 40, 3, 24, -2, [1, 2, 3, 4, 5, 23], mp=False),
    "hard_d64_last4_S256": _case("hard_aligned", 64, 4, 256, -4, [3, 4, 5, 8, 255, 256]),
    "hard_d64_r4_S300": _case("hard_aligned", 64, 3, 300, 4, [299, 300, 257, 100, 1, 2]),
    # ---- infinite_lookback / chunkwise: fast (S_cap <= 256, NP > 0) and looped (NP == 0, or S_cap > 256)
    "il_d8_r1_S24": _case("infinite_lookback", 8, 3, 24, 1, [1, 2, 23, 24, 12, 7]),
    "il_d16_r2_S64_nomp_bias": _case("infinite_lookback", 16, 4, 64, 2, [1, 2, 3, 63, 64, 33], hs=["0", "len", "0", "mid", "past", "cand"],
                                     mp=False, bias=-0.5),
    "il_d24_r4_S24": _case("infinite_lookback", 24, 3, 24, 4, [3, 4, 5, 8, 9, 24]),
    "il_d32_r8_S256": _case("infinite_lookback", 32, 4, 256, 8, [7, 8, 9, 255, 256, 129]),
    "il_d40_last2_S64": _case("infinite_lookback", 40, 3, 64, -2, [1, 2, 3, 4, 5, 64]),
    "il_d64_last4_S256_bias": _case("infinite_lookback", 64, 4, 256, -4, [3, 4, 5, 9, 255, 256], bias=-0.5),
    "il_d64_r4_S257": _case("infinite_lookback", 64, 3, 257, 4, [257, 256, 255, 100, 5, 1], hs=["len-1", "past", "mid", "0", "cand", "0"]),
    "il_d32_r2_S300": _case("infinite_lookback", 32, 4, 300, 2, [300, 299, 257, 256, 101, 3], hs=["past", "len-1", "mid", "cand", "0", "0"]),
    "il_d16_r8_S513": _case("infinite_lookback", 16, 3, 513, 8, [513, 512, 257, 9, 8, 7], hs=["len-1", "past", "mid", "0", "cand", "0"]),
    "cw_d64_r2_S64": _case("chunkwise", 64, 4, 64, 2, [1, 2, 3, 63, 64, 32]),
    "cw_d24_r1_S257_nomp": _case("chunkwise", 24, 3, 257, 1, [257, 256, 100, 2, 1, 255], hs=["len", "past", "mid", "0", "0", "len-1"], mp=False),
    # few live keys: forced stop at len - 1 -> n = len keys; bf16 d = 64 is NP = 8, 32 rows per pass, 8 per wave
    "il_d64_fewkeys_S64": _case("infinite_lookback", 64, 1, 64, 1, [2, 31, 32, 33, 17, 9], hs=["len-1"] * 6),
    # ---- wait-k: the closed form against the generic search
    "wk1_d16_r1_S24": _case("waitk", 16, 4, 24, 1, [1, 2, 23, 24, 12, 7], k=1),
    "wk3_d8_r2_S24_online": _case("waitk", 8, 3, 24, 2, [1, 2, 3, 4, 5, 24], online=True),
    "wk3_d32_r4_S64_nomp": _case("waitk", 32, 4, 64, 4, [3, 4, 5, 8, 9, 64], hs=["0", "len", "0", "mid", "past", "len"], mp=False),
    "wk1_d64_last2_S64_online": _case("waitk", 64, 4, 64, -2, [1, 2, 3, 4, 5, 64], k=1, online=True),
    "wk3_d24_r8_S256": _case("waitk", 24, 3, 256, 8, [7, 8, 9, 255, 256, 129]),
    "wk3_d40_last4_S24_online_nomp": _case("waitk", 40, 3, 24, -4, [3, 4, 5, 8, 9, 24], online=True, mp=False),
    "wk3_d64_fewkeys_S64": _case("waitk", 64, 1, 64, 1, [2, 31, 32, 33, 17, 9], tgt=["beyond"] * 6, hs=["0"] * 6),
    # key blocks of 256 + merge (S_cap > 256, NP > 0): rows ending in the first block leave -inf partials behind them
    "wk3_d64_r1_S257": _case("waitk", 64, 4, 257, 1, [257, 256, 255, 100, 2, 1], tgt=["beyond", "P-k", "mid", "beyond", "0", "0"],
                             hs=["0", "mid", "0", "0", "0", "0"]),
    "wk1_d32_r2_S300_online": _case("waitk", 32, 4, 300, 2, [300, 299, 257, 256, 101, 3], k=1, online=True,
                                    tgt=["beyond", "P-k", "mid", "beyond", "mid", "0"], hs=["0", "0", "cand", "len-1", "0", "0"]),
    "wk3_d16_r4_S513": _case("waitk", 16, 3, 513, 4, [513, 512, 300, 257, 100, 4], tgt=["beyond", "P-k", "mid", "beyond", "mid", "0"],
                             hs=["mid", "0", "0", "past", "0", "0"]),
    "wk3_d64_last4_S513_nomp": _case("waitk", 64, 4, 513, -4, [513, 512, 258, 255, 100, 3], mp=False,
                                     tgt=["beyond", "P-k", "beyond", "mid", "beyond", "0"], hs=["0", "0", "len", "0", "mid", "0"]),
    "wk3_d40_r2_S300": _case("waitk", 40, 3, 300, 2, [300, 257, 100], tgt=["beyond", "mid", "P-k"], hs=["0", "0", "0"]),      # NP == 0: looped
    # ---- FULL: no policy
    "full_d8_S24": _case("full", 8, 3, 24, 1, [1, 2, 23, 24, 12, 7]),
    "full_d64_fewkeys_S64": _case("full", 64, 1, 64, 1, [1, 2, 31, 32, 33, 9]),
    "full_d24_S256": _case("full", 24, 3, 256, 1, [256, 255, 100, 1, 17, 2]),
    "full_d32_S300": _case("full", 32, 4, 300, 1, [300, 299, 257, 256, 255, 100]),
    "full_d64_S513": _case("full", 64, 4, 513, 1, [513, 512, 257, 100, 1, 256]),
    "full_d40_S257": _case("full", 40, 3, 257, 1, [257, 256, 100, 1]),
    "full_d16_S257_H1": _case("full", 16, 1, 257, 1, [257, 1, 256]),
    # ---- an empty source in the batch (key_len == 0): zero ctx, no load; its neighbours unchanged
    "empty_hard_r2": _case("hard_aligned", 16, 4, 24, 2, [5, 0, 9], hs=["0", "0", "mid"]),
    "empty_hard_nomp": _case("hard_aligned", 16, 4, 24, 1, [5, 0, 9], hs=["0", "0", "mid"], mp=False),
    "empty_il_r4": _case("infinite_lookback", 32, 2, 24, 4, [0, 8, 24], hs=["0", "mid", "len-1"]),
    "empty_wk_S300": _case("waitk", 64, 2, 300, 2, [300, 0, 100], tgt=["beyond", "0", "mid"], hs=["0", "0", "0"]),
    "empty_full_S300": _case("full", 64, 2, 300, 1, [0, 300, 1]),
}


def lanes_per_row(d, dtype):
    """attn::lanes_per_row restated: 16-byte chunks per head row when that is an instantiated power of two, else 0"""
    lpr, rem = divmod(d, 8 if dtype == torch.bfloat16 else 4)
    return lpr if rem == 0 and lpr in (2, 4, 8, 16) else 0


def fused_path(c, dtype, unfused_opt=False):
    """the value-aggregation path of simulst_policy_cross_attention (launch_policy_cross), restated"""
    if c["attn"] == "hard_aligned":
        return "gather"
    np_ = lanes_per_row(c["d"], dtype)
    if c["attn"] in ("waitk", "full") and c["S_cap"] > 256 and np_ > 0 and not unfused_opt:
        return "blocks"
    return "fast" if np_ > 0 and c["S_cap"] <= 256 else "looped"


# ------------------------------------------------------------------ the reference
@functools.lru_cache(maxsize=None)
def _identity(D):
    eye = torch.eye(D, dtype=torch.float64)
    return {f"a.{n}.weight": eye for n in ("q_proj", "k_proj", "q_proj_soft", "k_proj_soft")}


def _rows(K, b, n):
    """head-major [B, H, S_cap, d], utterance b, first n frames -> the oracle's [src, 1, D]"""
    H, d = K.shape[1], K.shape[3]
    return K[b, :, :n].permute(1, 0, 2).reshape(n, 1, H * d)


def reference(qm, qs, Kmono, Ksoft, V, *, energy_bias, key_len, tgt_idx, head_step, ratio, attn_type, waitk_k, online,
              mass_preservation, mutation=None):
    """float64 tensors in the entry point's layout (qm / qs [B, D]; Kmono / Ksoft / V [B, H, S_cap, d]; unused ones None), key_len /
    tgt_idx lists, head_step [B, H] long.  -> dict: p, pooled, beta (lists over b of [H, len_b]), head_step [B, H], head_read [B, H]
    (None for 'full'), ctx [B, D], vmax [B, D] (max |v_j| over the attended keys), keys[b][h] (attended key indices)."""
    B, H, S_cap, d = V.shape
    D = H * d
    w = dict(_identity(D))
    w["a.energy_bias"] = torch.tensor(float(energy_bias), dtype=torch.float64)
    full = attn_type == "full"
    cfg = omo.AttnCfg(attn_type="infinite_lookback" if full else attn_type, num_heads=H, mass_preservation=bool(mass_preservation),
                      energy_bias=True, waitk_lagging=waitk_k, chunk_size=3 if attn_type == "chunkwise" else None,
                      pre_decision_ratio=abs(ratio), pre_decision_type="last" if ratio < 0 else "average")
    out = dict(p=[], pooled=[], beta=[], keys=[], ctx=torch.zeros(B, D, dtype=torch.float64), vmax=torch.zeros(B, D, dtype=torch.float64),
               head_step=None if full else head_step.clone(), head_read=None if full else torch.zeros(B, H, dtype=torch.bool))
    for b in range(B):
        n = int(key_len[b])
        if n == 0:
            # the project's own convention (include/simulst_hip.h), not the oracle's: nothing attended, the search ends at 0
            out["p"].append(torch.zeros(H, 0, dtype=torch.float64)); out["pooled"].append(torch.zeros(H, 0, dtype=torch.float64))
            out["beta"].append(torch.zeros(H, 0, dtype=torch.float64)); out["keys"].append([torch.zeros(0, dtype=torch.long)] * H)
            if not full:
                out["head_step"][b] = 0
                out["head_read"][b] = not mass_preservation
            continue
        cols = torch.arange(n)
        if full:
            e = omo.energy_from_qk(w, "a", cfg, qs[b].view(1, 1, D), _rows(Ksoft, b, n), "soft")
            beta = torch.softmax(e, dim=-1).squeeze(1)
            p = pooled = torch.zeros(H, 0, dtype=torch.float64)
            keys = [cols] * H
        else:
            waitk = attn_type == "waitk"
            q1 = (qs if waitk else qm)[b].view(1, 1, D)
            key = _rows(Ksoft if waitk else Kmono, b, n)
            if mutation == "window_shift":
                key = torch.roll(key, -1, 0)
            state = {"tgt_len": int(tgt_idx[b]) + (1 if mutation == "waitk_off_by_one" else 0), "online": bool(online)}
            if mutation == "no_floor_trim" and not waitk:
                p = omo.p_choose(w, "a", cfg, q1, key, None, {}, False).squeeze(1)
            else:
                p = omo.p_choose(w, "a", cfg, q1, key, None, state, True).squeeze(1)
            pooled = state["pooled_p"].squeeze(1) if "pooled_p" in state else p
            if mutation == "no_last_col" and "pooled_p" in state:
                p = omo.insert_zeros(state["pooled_p"], abs(ratio)).squeeze(1)
                p = torch.cat([p, p.new_zeros(H, max(n - p.size(1), 0))], dim=1)[:, :n]
            assert p.dtype == torch.float64 and p.shape == (H, n)
            hs = head_step[b] + (1 if mutation == "past_le" else 0)
            new_step, head_read, alpha = omo.step_search(p, hs, torch.full((H,), n, dtype=torch.long),
                                                         bool(mass_preservation) and mutation != "stop_at_len")
            out["head_step"][b], out["head_read"][b] = new_step, head_read
            if attn_type == "hard_aligned":
                beta = alpha
                keys = [alpha[h].nonzero().flatten() for h in range(H)]
            else:
                # attention_infer's softmax over the keys up to the step, restated in fp64 (monotonic_multihead_attention.py:278-293)
                e = omo.energy_from_qk(w, "a", cfg, qs[b].view(1, 1, D), _rows(Ksoft, b, n), "soft").squeeze(1)
                masked = cols.view(1, -1) >= new_step.view(-1, 1) if mutation == "keys_lt_step" else cols.view(1, -1) > new_step.view(-1, 1)
                beta = torch.softmax(e.masked_fill(masked, -1e8), dim=-1)
                beta = beta.masked_fill(masked, 0.0)              # exp(-1e8 - max) is 0 in fp64 unless every key is masked
                if mutation != "no_zero_unmoved":
                    beta = beta.masked_fill(new_step.eq(0).view(-1, 1), 0.0)
                keys = [beta[h].nonzero().flatten() for h in range(H)]
        v = V[b, :, :n]                                               # [H, n, d]
        out["ctx"][b] = torch.bmm(beta.unsqueeze(1), v).reshape(D)
        out["vmax"][b] = torch.stack([v[h, keys[h]].abs().amax(dim=0) if keys[h].numel() else torch.zeros(d, dtype=torch.float64)
                                      for h in range(H)]).reshape(D)
        out["p"].append(p); out["pooled"].append(pooled); out["beta"].append(beta); out["keys"].append(keys)
    return out


# ------------------------------------------------------------------ inputs: drawn on the CPU until the decisions are fair
def _draw(c, seed, dtype):
    """fp32 draws rounded to dtype, widened to float64.  Queries x 3: few energies near 0.  Rows >= key_len hold values too."""
    g = torch.Generator().manual_seed(seed)
    B, H, d, S = len(c["lens"]), c["H"], c["d"], c["S_cap"]
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dtype).double()      # noqa: E731
    return dict(qm=rnd(B, H * d, scale=3.0), qs=rnd(B, H * d, scale=2.0), Kmono=rnd(B, H, S, d), Ksoft=rnd(B, H, S, d),
                V=rnd(B, H, S, d, scale=1.5))


def _ref(c, inp, head_step, tgt, mutation=None, bias=None):
    return reference(inp["qm"], inp["qs"], inp["Kmono"], inp["Ksoft"], inp["V"], energy_bias=c["bias"] if bias is None else bias,
                     key_len=c["lens"], tgt_idx=tgt, head_step=head_step, ratio=c["ratio"], attn_type=c["attn"], waitk_k=c["k"],
                     online=c["online"], mass_preservation=c["mp"], mutation=mutation)


def _resolve(c, inp):
    """the incoming head_step [B, H] and tgt_idx [B] the case's words stand for, from the reference's own probabilities"""
    B, H = len(c["lens"]), c["H"]
    zero = torch.zeros(B, H, dtype=torch.long)
    if c["attn"] == "full":
        return zero, [0] * B
    P = [x.size(1) for x in _ref(c, inp, zero, [0] * B)["pooled"]]                 # pooled positions of every row
    tgt = [{"0": 0, "mid": P[b] // 2, "P-k": max(P[b] - c["k"], 0), "beyond": P[b] + 2}[c["tgt"][b]] for b in range(B)]
    p = _ref(c, inp, zero, tgt)["p"]
    hs = zero.clone()
    for b, n in enumerate(c["lens"]):
        for h in range(H):
            cand, stop = (p[b][h] > 0).nonzero().flatten().tolist(), (p[b][h] >= 0.5).nonzero().flatten().tolist()
            v = {"0": 0, "mid": n // 2 + h, "cand": cand[len(cand) // 2] if cand else 0, "len-1": n - 1, "len": n,
                 "past": (stop[-1] + 1) if stop else 0}[c["hs"][b]]
            hs[b, h] = max(0, min(v, n - 1 if c["mp"] else n))
    return hs, tgt


def _margin(ref):
    """min |energy + energy_bias| over every pooled key of the reference (the logit of its pooled probabilities)"""
    pp = torch.cat([x.flatten() for x in ref["pooled"]] + [torch.ones(1, dtype=torch.float64)])
    pp = pp[(pp > 0) & (pp < 1)]                       # wait-k's 0 / 1 and saturated sigmoids are far from 0.5
    return float((pp.log() - (-pp).log1p()).abs().min()) if pp.numel() else float("inf")


def _decisions_differ(x, y):
    return not (torch.equal(x["head_step"], y["head_step"]) and torch.equal(x["head_read"], y["head_read"]))


@functools.lru_cache(maxsize=None)
def prepared(name):
    """-> {dtype: (inp, head_step_in, tgt, ref)}: the first seed whose margin holds (and whose energy_bias matters) in both dtypes"""
    c = CASES[name]
    for attempt in range(200):
        seed = 7300 + 1000 * attempt + list(CASES).index(name)
        out = {}
        for dtype in DTYPES:
            inp = _draw(c, seed, dtype)
            hs, tgt = _resolve(c, inp)
            ref = _ref(c, inp, hs, tgt)
            if c["attn"] in LEARNED and _margin(ref) < MARGIN:
                break
            if c["bias"] != 0.0 and not _decisions_differ(_ref(c, inp, hs, tgt, bias=0.0), ref):
                break                                      # the bias must move a decision: test_case_preconditions
            out[dtype] = (inp, hs, tgt, ref)
        if len(out) == len(DTYPES):
            return out
    raise AssertionError(f"{name}: no seed with |energy + bias| >= {MARGIN} at every pooled key")


# ------------------------------------------------------------------ CPU: the reference pinned to the reference implementation's fixtures
def _head_major(t, H, S_cap=None):
    """[S, B, D] -> [B, H, S_cap, d] float64"""
    S, B, D = t.shape
    out = torch.zeros(B, S_cap or S, D, dtype=torch.float64)
    out[:, :S] = t.transpose(0, 1)
    return out.view(B, S_cap or S, H, D // H).permute(0, 2, 1, 3).contiguous()


def _lin(w, name, x):
    return torch.nn.functional.linear(x.double(), w[name + ".weight"].double(), w[name + ".bias"].double())


def _fixture_p(w, base, ratio, q, keys, lens, *, k=3, online=True, tgt=0, hs=None, with_soft=False):
    """project q [B, D] / keys [S, B, D] with the fixture's weights (fp64) and run the reference -> its dict"""
    H = 2
    B = keys.size(1)
    Km = _head_major(_lin(w, "k_proj", keys), H)
    soft = "k_proj_soft.weight" in w and base != "waitk"
    Ks = _head_major(_lin(w, "k_proj_soft" if soft else "k_proj", keys), H)
    Vc = _head_major(_lin(w, "v_proj", keys), H) if "v_proj.weight" in w else torch.zeros_like(Km)
    qm = _lin(w, "q_proj", q)
    qs = _lin(w, "q_proj_soft" if soft else "q_proj", q)
    hs = torch.zeros(B, H, dtype=torch.long) if hs is None else hs
    return reference(qm, qs, Km, Ks, Vc, energy_bias=0.0, key_len=lens, tgt_idx=[tgt] * B, head_step=hs, ratio=ratio, attn_type=base,
                     waitk_k=k, online=online, mass_preservation=True)


def _stack_p(ref):
    return torch.cat(ref["p"], dim=0)                         # [B * H, len] for equal lengths


G7_NAMES = ["hard_aligned_fixed_pre_decision", "infinite_lookback_fixed_pre_decision", "waitk_fixed_pre_decision"]


@pytest.mark.parametrize("name", G7_NAMES)
def test_reference_vs_g7_predecision(name):
    """'average' pooling at ratio 2: the incremental p_choose of the reference implementation at source lengths 1 .. 21"""
    a, _ = load_golden("g7_predecision")
    g10, _ = load_golden("g10_mma_forward")
    w = split_weights(g10, f"{name}.mp1")
    base = name.replace("_fixed_pre_decision", "")
    B = a["keys"].size(1)
    for sl in (1, 2, 3, 4, 5, 8, 9, 21):
        ref = _fixture_p(w, base, 2, a["q"][0], a["keys"][:sl], [sl] * B)
        torch.testing.assert_close(_stack_p(ref), a[f"{name}.incr.{sl}"][:, 0].double(), atol=2e-5, rtol=1e-4)


@pytest.mark.parametrize("name", G7_NAMES)
@pytest.mark.parametrize("ratio", [2, 4])
def test_reference_vs_g19_predecision_last(name, ratio):
    """'last' pooling: p_choose at every source length, and the growing-source traces -- head_step / head_read exact, p to 1e-5, the
    out-projected context to 1e-4 (the tolerances of tests/test_oracle_golden.py::test_g19_fixed_pre_decision_last)"""
    a, _ = load_golden("g19_predecision_last")
    tag = f"{name}.r{ratio}"
    w = split_weights(a, tag)
    base = name.replace("_fixed_pre_decision", "")
    keys, B, H = a["keys"], a["keys"].size(1), 2
    for sl in (1, 2, 3, 4, 5, 7, 8, 9, 21):
        ref = _fixture_p(w, base, -ratio, a["q"][0], keys[:sl], [sl] * B)
        torch.testing.assert_close(_stack_p(ref), a[f"{tag}.incr.{sl}"][:, 0].double(), atol=2e-5, rtol=1e-4)
    for online in (True, False):
        hs, tgt = torch.zeros(B, H, dtype=torch.long), 0
        for step, sl in enumerate(a[f"{tag}.src_sizes"].tolist()):
            pre = f"{tag}.on{int(online)}.{step}"
            ref = _fixture_p(w, base, -ratio, a[pre + ".q"][0], keys[:sl], [sl] * B, online=online, tgt=tgt, hs=hs)
            assert torch.equal(ref["head_step"], a[pre + ".head_step"].view(B, H)), pre
            assert torch.equal(ref["head_read"], a[pre + ".head_read"].view(B, H)), pre
            torch.testing.assert_close(_stack_p(ref), a[pre + ".p_choose"].reshape(B * H, sl).double(), atol=1e-5, rtol=1e-4)
            torch.testing.assert_close(_lin(w, "out_proj", ref["ctx"]), a[pre + ".out"][0].double(), atol=1e-4, rtol=1e-4)
            hs = ref["head_step"]
            if base == "waitk" and not (online and bool(a[pre + ".head_read"].any())):
                tgt += 1


def test_reference_vs_g6_waitk():
    """the wait-k one-hot, k in {1, 3, 5}, online and not, with and without shorter rows: exact on the columns
    below the row's length (online, the fixture's one-hot may lie in the padding, which the per-utterance form does not have)"""
    a, _ = load_golden("g6_waitk")
    d = 8
    z = torch.zeros(4, 1, 9, d, dtype=torch.float64)
    for k in (1, 3, 5):
        for online in (True, False):
            for pad in (False, True):
                lens = [9, 9, 6, 6] if pad else [9] * 4
                for tl in (1, 4, 8):
                    fx = a[f"k{k}.on{int(online)}.pad{int(pad)}.t{tl}"]
                    ref = reference(None, torch.zeros(4, d, dtype=torch.float64), None, z, z, energy_bias=0.0, key_len=lens,
                                    tgt_idx=[tl - 1] * 4, head_step=torch.zeros(4, 1, dtype=torch.long), ratio=1, attn_type="waitk",
                                    waitk_k=k, online=online, mass_preservation=True)
                    for b, n in enumerate(lens):
                        assert torch.equal(ref["p"][b][0], fx[b, 0, :n].double()), (k, online, pad, tl, b)


@pytest.mark.parametrize("name", ["hard_aligned_fixed_pre_decision", "infinite_lookback_fixed_pre_decision"])
@pytest.mark.parametrize("ptype", ["average", "last"])
@pytest.mark.parametrize("ratio", [2, 4])
def test_reference_vs_g20_predecision_padded(name, ptype, ratio):
    """the reference implementation's padded-batch p_choose on a ragged batch: the per-utterance form agrees with it on every column
    below key_len of the rows that hold at least one whole window (include/simulst_hip.h, simulst_step_p_choose_padded); atol 1e-6 as
    tests/test_oracle_golden.py::test_g20_padded_batch_incremental_p_choose"""
    a, _ = load_golden("g20_predecision_padded")
    tag = f"{name}.{ptype}.r{ratio}"
    w = split_weights(a, tag)
    base = name.replace("_fixed_pre_decision", "")
    lens = a[f"lens.r{ratio}"].tolist()
    ref = _fixture_p(w, base, -ratio if ptype == "last" else ratio, a["q"][0], a["keys"], lens)
    fx = a[f"{tag}.incr"][:, 0].double()
    checked = 0
    for b, n in enumerate(lens):
        if n >= ratio:
            torch.testing.assert_close(ref["p"][b], fx[2 * b:2 * b + 2, :n], atol=1e-6, rtol=1e-4)
            checked += 1
    assert checked >= 2


# ------------------------------------------------------------------ CPU: preconditions of the GPU cases, and that they can fail
@pytest.mark.parametrize("name", list(CASES))
def test_case_preconditions(name):
    """every pooled key's |energy + bias| >= 1e-3 in both dtypes; the incoming head_step stays inside the reachable range; a nonzero
    energy_bias moves at least one decision of the reference"""
    c = CASES[name]
    for dtype, (inp, hs, tgt, ref) in prepared(name).items():
        if c["attn"] in LEARNED:
            assert _margin(ref) >= MARGIN, (name, dtype)
        for b, n in enumerate(c["lens"]):
            assert 0 <= int(hs[b].min()) and int(hs[b].max()) <= max(n - 1 if c["mp"] else n, 0)
        if c["bias"] != 0.0:
            other = _ref(c, inp, hs, tgt, bias=0.0)
            assert _decisions_differ(other, ref), (name, dtype, "energy_bias moves no decision")


def test_cases_cover_every_path():
    bf, f32 = torch.bfloat16, torch.float32
    for dtype in DTYPES:
        assert {fused_path(c, dtype) for c in CASES.values()} == {"gather", "fast", "looped", "blocks"}
    assert {lanes_per_row(c["d"], bf) for c in CASES.values()} == {0, 2, 4, 8}
    assert {lanes_per_row(c["d"], f32) for c in CASES.values()} == {0, 2, 4, 8, 16}
    assert {abs(c["ratio"]) for c in CASES.values()} == {1, 2, 4, 8} and {c["ratio"] for c in CASES.values()} >= {-2, -4}
    for attn in LEARNED + ("waitk",):
        assert {c["mp"] for c in CASES.values() if c["attn"] == attn} == {True, False} or attn == "chunkwise"
    assert any(c["attn"] in LEARNED and c["attn"] != "hard_aligned" and c["S_cap"] > 256 for c in CASES.values())
    # dead rows (no mass preservation, the head ran off the end) and unmoved heads exist in the reference
    dead = unmoved = 0
    for name, c in CASES.items():
        ref = prepared(name)[bf][3]
        if c["attn"] == "full":
            continue
        lens = torch.tensor(c["lens"]).view(-1, 1)
        dead += int(((ref["head_step"] == lens) & (lens > 0)).sum()) if not c["mp"] else 0
        unmoved += int((ref["head_step"] == 0).sum()) if c["attn"] != "hard_aligned" else 0
    assert dead >= 4 and unmoved >= 4


def test_reference_mutations_change_a_case():
    """each one-off mistake changes a decision of the reference, or moves its ctx by more than 10 x the bf16 bound of that element,
    on at least one case: a kernel with that mistake cannot pass the GPU cases"""
    hits = {m: [] for m in MUTATIONS}
    for name, c in CASES.items():
        if c["attn"] == "full":
            continue
        inp, hs, tgt, ref = prepared(name)[torch.bfloat16]
        for m in MUTATIONS:
            mut = _ref(c, inp, hs, tgt, mutation=m)
            decision = _decisions_differ(mut, ref)
            bound = BF16_BOUND * torch.maximum(ref["vmax"], mut["vmax"])
            moved = bool(((mut["ctx"] - ref["ctx"]).abs() > 10 * bound).any())
            if decision or moved:
                hits[m].append(name)
    for m, names in hits.items():
        print(f"mutation {m}: {len(names)} cases change")
        assert names, m


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ops():
    from simulst_amd.ops import Ops
    return Ops()


@pytest.fixture(scope="module")
def worst():
    """worst |got - ref| / bound (bf16) per value-aggregation path, and the worst energy error the step probabilities imply"""
    w = {}
    yield w
    for k, (r, name) in sorted(w.items()):
        print(f"\npolicy + cross-attention, worst over all cases: {k}: {r:.3e} ({name})")


def _note(worst, key, value, name):
    if value > worst.get(key, (-1.0, ""))[0]:
        worst[key] = (value, name)


def _device(c, inp, tgt, dtype):
    dev = lambda t: t.to(dtype).cuda().contiguous()          # noqa: E731
    g = {k: dev(v) for k, v in inp.items()}
    g["key_len"] = torch.tensor(c["lens"], dtype=torch.int32).cuda()
    g["tgt"] = torch.tensor(tgt, dtype=torch.int32).cuda()
    return g


def _fused(ops, c, g, hs_in, dtype, *, unfused_opt=False, null_step=False):
    """simulst_policy_cross_attention with the unused operands NULL -> (ctx, head_step, head_read) on the CPU"""
    from simulst_amd import _lib
    from simulst_amd.ops import _p, dt
    B, H, d = len(c["lens"]), c["H"], c["d"]
    attn, full = c["attn"], c["attn"] == "full"
    learned = attn in LEARNED
    hs = torch.full((B * H,), STEP_SENTINEL, dtype=torch.int64).cuda() if full else hs_in.reshape(-1).clone().cuda()
    hr = torch.full((B * H,), READ_SENTINEL, dtype=torch.uint8).cuda()
    ctx = torch.full((B, H * d), SENTINEL, dtype=dtype).cuda()
    try:
        ops.h.set_option(_lib.OPT_UNFUSED_DECODE, int(unfused_opt))
        ops.h.check(ops.lib.simulst_policy_cross_attention(
            ops.h.ptr, _p(g["qm"] if learned else None), _p(None if attn == "hard_aligned" else g["qs"]),
            _p(g["Kmono"] if learned else None), _p(None if attn == "hard_aligned" else g["Ksoft"]), _p(g["V"]), float(c["bias"]),
            _p(g["key_len"]), _p(None if full else g["tgt"]), _p(None if null_step else hs), _p(None if null_step else hr), _p(ctx),
            B, H, d, c["S_cap"], c["ratio"], _lib.ATTN_ENUM[attn], c["k"], int(c["online"]), int(c["mp"]), dt(g["V"])),
            "simulst_policy_cross_attention")
        torch.cuda.synchronize()
    finally:
        ops.h.set_option(_lib.OPT_UNFUSED_DECODE, 0)
    return ctx.cpu(), hs.cpu().view(B, H), hr.cpu().view(B, H)


def _unfused(ops, c, g, hs_in, dtype):
    """simulst_step_p_choose + simulst_mma_step_search + simulst_decoder_cross_attention -> (p, ctx, head_step, head_read, beta)"""
    from simulst_amd import _lib
    B, H, d, S = len(c["lens"]), c["H"], c["d"], c["S_cap"]
    attn = c["attn"]
    ctx = torch.full((B, H * d), SENTINEL, dtype=dtype).cuda()
    if attn == "full":
        _, beta = ops.decoder_cross_attention(g["qs"], g["Ksoft"], g["V"], None, H=H, attn_type=_lib.ATTN_FULL, mass_preservation=False,
                                              key_len=g["key_len"], want_beta=True, out=ctx)
        torch.cuda.synchronize()
        return None, ctx.cpu(), None, None, beta.cpu()
    p = torch.full((B * H, S), -1.0, device="cuda")
    learned = attn in LEARNED
    ops.step_p_choose(g["qm"] if learned else None, g["Kmono"] if learned else None, p, B=B, S_cap=S, H=H, d=d, ratio=c["ratio"],
                      incremental=True, attn_type=_lib.ATTN_ENUM[attn], key_len=g["key_len"], energy_bias=c["bias"], waitk_k=c["k"],
                      tgt_idx=g["tgt"], online=c["online"], dtype=_lib.BF16 if dtype == torch.bfloat16 else _lib.F32)
    hs = hs_in.reshape(-1).clone().cuda()
    hr, _ = ops.mma_step_search(p, hs, src_len=g["key_len"].repeat_interleave(H).contiguous(), mass_preservation=c["mp"], want_alpha=False)
    soft = attn != "hard_aligned"
    _, beta = ops.decoder_cross_attention(g["qs"] if soft else None, g["Ksoft"] if soft else None, g["V"], hs, H=H,
                                          attn_type=_lib.ATTN_ENUM[attn], mass_preservation=c["mp"], key_len=g["key_len"], want_beta=True,
                                          out=ctx)
    torch.cuda.synchronize()
    return p.cpu(), ctx.cpu(), hs.cpu().view(B, H), hr.cpu().view(B, H), beta.cpu()


def _check_ctx(name, c, way, path, dtype, got, ref, worst):
    r, vmax = ref["ctx"], ref["vmax"]
    o = got.double()
    if c["attn"] == "hard_aligned":
        assert torch.equal(o, r), (name, way, "the gather is not bit-identical to the V row of the reference")
        return
    err = (o - r).abs()
    ratio = float((err / (BF16_BOUND * vmax).clamp_min(1e-300)).max())
    print(f"{name}: {way} [{path}] {str(dtype)[6:]}: max |got - ref| = {float(err.max()):.3e}, worst / bf16 bound = {ratio:.3f}")
    assert torch.equal(o[vmax == 0], torch.zeros_like(o[vmax == 0])), (name, way, "a row that attends to nothing is not zero")
    if dtype == torch.float32:
        torch.testing.assert_close(o, r, atol=2e-5, rtol=1e-4, msg=lambda m: f"{name}: {way} [{path}]: {m}")
    else:
        _note(worst, f"bf16 ctx / bound, {path}", ratio, name)
        assert bool((err <= BF16_BOUND * vmax).all()), (name, way, path, ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_policy_cross_attention_vs_fp64(ops, worst, name):
    c = CASES[name]
    B, H, S = len(c["lens"]), c["H"], c["S_cap"]
    full = c["attn"] == "full"
    for dtype, (inp, hs_in, tgt, ref) in prepared(name).items():
        if c["attn"] in LEARNED:
            assert _margin(ref) >= MARGIN                      # the decisions below are fair
        g = _device(c, inp, tgt, dtype)
        ways = [("fused", fused_path(c, dtype), _fused(ops, c, g, hs_in, dtype))]
        if c["attn"] in ("waitk", "full") and S > 256:
            ways.append(("fused, OPT_UNFUSED_DECODE", fused_path(c, dtype, True), _fused(ops, c, g, hs_in, dtype, unfused_opt=True)))
        p, ctx_u, hs_u, hr_u, beta = _unfused(ops, c, g, hs_in, dtype)
        # ---- decisions: exact, every (row, head), every way
        for way, path, (ctx, hs, hr) in ways:
            if full:
                assert bool((hs == STEP_SENTINEL).all()) and bool((hr == READ_SENTINEL).all()), (name, way, "FULL touched head_step / head_read")
            else:
                assert torch.equal(hs, ref["head_step"]), (name, way, dtype, hs, ref["head_step"])
                assert torch.equal(hr.bool(), ref["head_read"]), (name, way, dtype, hr, ref["head_read"])
            _check_ctx(name, c, way, path, dtype, ctx, ref, worst)
        if not full:
            assert torch.equal(hs_u, ref["head_step"]), (name, "unfused", dtype, hs_u, ref["head_step"])
            assert torch.equal(hr_u.bool(), ref["head_read"]), (name, "unfused", dtype, hr_u, ref["head_read"])
        _check_ctx(name, c, "unfused", "unfused", dtype, ctx_u, ref, worst)
        if full:                                               # step == NULL is accepted
            ctx_n, _, _ = _fused(ops, c, g, hs_in, dtype, null_step=True)
            assert torch.equal(ctx_n, ways[0][2][0]), (name, "FULL with head_step / head_read NULL")
        # ---- step probabilities (observable in the unfused triple) and the energy error they imply
        for b, n in enumerate(c["lens"]):
            if not full:
                got = p[b * H:(b + 1) * H].double()
                assert float(got[:, n:].abs().max()) == 0.0 if n < S else True, (name, "p beyond key_len")
                torch.testing.assert_close(got[:, :n], ref["p"][b], atol=1e-5, rtol=1e-4, msg=lambda m: f"{name}: p, row {b}: {m}")
                if c["attn"] in LEARNED:
                    rp = ref["p"][b]
                    sel = (rp > 0.02) & (rp < 0.98)
                    if bool(sel.any()):
                        logit = lambda x: x.log() - (-x).log1p()      # noqa: E731
                        _note(worst, f"|energy error| implied by p, {str(dtype)[6:]}", float((logit(got[:, :n][sel]) - logit(rp[sel])).abs().max()), name)
            # ---- beta of simulst_decoder_cross_attention: the reference softmax on the attended keys, zero elsewhere
            if c["attn"] != "hard_aligned":
                gb = beta[b * H:(b + 1) * H].double()
                torch.testing.assert_close(gb[:, :n], ref["beta"][b], atol=1e-5, rtol=1e-4, msg=lambda m: f"{name}: beta, row {b}: {m}")
                assert float(gb[:, :n][ref["beta"][b] == 0].abs().sum()) == 0.0 and float(gb[:, n:].abs().sum()) == 0.0, (name, "beta outside the keys")


@pytest.mark.gpu
@pytest.mark.parametrize("d", [24, 40])
def test_decoder_self_attention_row_lane_limit(ops, d):
    """simulst_decoder_self_attention at head dims without a lanes-per-row instantiation, 249 .. 257 keys: below, at and above the
    rows its row-per-lane core covers (252 / 250) and the 256 where the looped path always began.  Same rounding points as the
    cross-attention (one rounding, at the store), same bounds; the appended K / V rows must be this step's, bit for bit."""
    B, H, cap = 6, 2, 260
    D = H * d
    n_prev = [248, 250, 251, 252, 255, 256]
    g = torch.Generator().manual_seed(8800 + d)
    draws = [torch.randn(B, 3 * D, generator=g) * 1.5, torch.randn(B, H, cap, d, generator=g), torch.randn(B, H, cap, d, generator=g) * 1.5]
    for dtype in DTYPES:
        qkv, kc, vc = [t.to(dtype) for t in draws]
        q, k_new, v_new = [t.double().view(B, H, d) for t in qkv.split(D, dim=-1)]
        ref, vmax = torch.zeros(B, H, d, dtype=torch.float64), torch.zeros(B, H, d, dtype=torch.float64)
        for b, n in enumerate(n_prev):
            K = torch.cat([kc[b, :, :n].double(), k_new[b].unsqueeze(1)], dim=1)             # [H, n + 1, d]
            V = torch.cat([vc[b, :, :n].double(), v_new[b].unsqueeze(1)], dim=1)
            beta = torch.softmax(torch.bmm(K, q[b].unsqueeze(2)).squeeze(2) * d ** -0.5, dim=-1)
            ref[b], vmax[b] = torch.bmm(beta.unsqueeze(1), V).squeeze(1), V.abs().amax(dim=1)
        kc_d, vc_d = kc.cuda(), vc.cuda()
        got = ops.decoder_self_attention(qkv.cuda(), kc_d, vc_d, torch.tensor(n_prev, dtype=torch.int32).cuda())
        torch.cuda.synchronize()
        for b, n in enumerate(n_prev):
            assert torch.equal(kc_d[b, :, n].cpu().double(), k_new[b]) and torch.equal(vc_d[b, :, n].cpu().double(), v_new[b]), (d, dtype, b)
        err = (got.cpu().double().view(B, H, d) - ref).abs()
        ratio = (err / (BF16_BOUND * vmax)).amax(dim=(1, 2))
        print(f"self-attention d={d} {str(dtype)[6:]}: max |got - ref| per row {err.amax(dim=(1, 2)).tolist()}, / bf16 bound {ratio.tolist()}")
        if dtype == torch.float32:
            torch.testing.assert_close(got.cpu().double().view(B, H, d), ref, atol=2e-5, rtol=1e-4)
        else:
            assert bool((err <= BF16_BOUND * vmax).all()), (d, ratio.tolist())
