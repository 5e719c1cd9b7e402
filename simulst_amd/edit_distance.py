"""Error rates for the ASR paths: the batched Levenshtein alignment of label strings, on the device where the hypotheses are.

The reference's ASR stage is judged by word error rate (exp/infer_asr.yaml eval_wer, tasks/speech_to_text_infer.py:206-215: fairseq's
WerScorer, the sum of edit distances over the sum of reference lengths, summed over workers at :263-289).  `edit_distance` is that
distance for N (reference, hypothesis) pairs of int64 label strings in ONE launch (csrc/edit_distance.hip,
simulst_edit_distance), with the substitution / deletion / insertion counts of ONE alignment fixed by a tie rule, and optionally
that alignment.  Pairs are named by row indices, so the shapes a host loop is bad at cost nothing extra: a 16-best list against its
reference (`oracle_error`) and an n-best list against itself (`mbr_select`, minimum-Bayes-risk selection).

Tie rule (the contract; tests/edit_distance_ref.py spells out the same): D[i][j] is the distance of the first i reference labels and
the first j hypothesis labels; among the predecessors that attain the minimum a cell takes, in this order, the diagonal (a match if the
labels are equal, else a substitution), a deletion (D[i-1][j] + 1: reference label i has no counterpart), an insertion
(D[i][j-1] + 1).  sub / del / ins are counted along the path from (Lr, Lh) back to (0, 0).  Codes: 0 match, 1 substitution,
2 deletion, 3 insertion.

composed=True is the same rule as torch tensor operations on the host (every pair at once, one reference row at a time, the insertion
chain of a row by a running minimum), the convention of ctc_prefix_beam_advance(composed=True): it is what runs for CPU tensors and
for strings above the kernel's 1023 labels, and what the kernel is measured against (tools/error_rate_bench.py)."""
import torch

from ._lib import EDIT_MAX_LABELS

MATCH, SUB, DEL, INS = 0, 1, 2, 3
OPS_PAD = -1


def _check_idx(idx, rows, N, who):
    """indices the host holds are checked here, before any launch; indices on the device are compared with the row count by the
    kernel (such a pair's counts are -1)"""
    if idx is None:
        if N > rows:
            raise ValueError(f"edit_distance: {N} pairs by position but {rows} {who} rows")
        return None
    if not isinstance(idx, torch.Tensor):
        idx = torch.as_tensor(idx, dtype=torch.int64)
    if not idx.is_cuda and idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= rows):
        raise ValueError(f"edit_distance: a {who} index outside [0, {rows})")
    return idx


def edit_distance(ops, ref: torch.Tensor, ref_len: torch.Tensor, hyp: torch.Tensor, hyp_len: torch.Tensor, *, ref_idx=None,
                  hyp_idx=None, path: bool = False, composed: bool = False, ops_dtype=torch.int8):
    """ref [Rr, Wr] / hyp [Rh, Wh] int64 label strings with lengths ref_len [Rr] / hyp_len [Rh]; pair p compares reference row
    ref_idx[p] with hypothesis row hyp_idx[p] (None: row p) -> counts int32 [N, 4] = (distance, sub, del, ins).  With path also
    (ops [N, Wr + Wh] in ops_dtype, the alignment front to back with -1 behind it, n_ops int32 [N]).  On the GPU one launch and no
    read-back (`ops`: the Ops whose stream it goes to, None = a new one); composed / CPU tensors / strings above 1023 labels: the torch
    form on the host, results on the strings' device.  Both give the same integers."""
    N = len(ref_idx) if ref_idx is not None else len(hyp_idx) if hyp_idx is not None else ref.size(0)
    ref_idx, hyp_idx = _check_idx(ref_idx, ref.size(0), N, "reference"), _check_idx(hyp_idx, hyp.size(0), N, "hypothesis")
    for idx in (ref_idx, hyp_idx):
        if idx is not None and idx.numel() != N:
            raise ValueError("edit_distance: one index per pair on each side")
    dev = ref.device
    ref_len, hyp_len = torch.as_tensor(ref_len, device=dev).to(torch.int64), torch.as_tensor(hyp_len, device=hyp.device).to(torch.int64)
    if composed or not ref.is_cuda or not hyp.is_cuda or max(ref.size(1), hyp.size(1)) > EDIT_MAX_LABELS:
        return _edit_distance_composed(ref, ref_len, hyp, hyp_len, ref_idx, hyp_idx, N, path, ops_dtype)
    from .ops import Ops
    ops = ops or Ops()
    ri = None if ref_idx is None else ref_idx.to(device=dev, dtype=torch.int32).contiguous()
    hi = None if hyp_idx is None else hyp_idx.to(device=dev, dtype=torch.int32).contiguous()
    return ops.edit_distance(ref.to(torch.int64), ref_len.contiguous(), hyp.to(torch.int64), hyp_len.contiguous(), ref_idx=ri, hyp_idx=hi,
                             n_pairs=N, path=path, pad=OPS_PAD, ops_dtype=ops_dtype)


def _edit_distance_composed(ref, ref_len, hyp, hyp_len, ref_idx, hyp_idx, N, path, ops_dtype):
    dev = ref.device
    ref, ref_len, hyp, hyp_len = ref.cpu().to(torch.int64), ref_len.cpu(), hyp.cpu().to(torch.int64), hyp_len.cpu()
    ri = torch.arange(N) if ref_idx is None else ref_idx.cpu().to(torch.int64)
    hi = torch.arange(N) if hyp_idx is None else hyp_idx.cpu().to(torch.int64)
    ok = (ri >= 0) & (ri < ref.size(0)) & (hi >= 0) & (hi < hyp.size(0))               # (device indices: as the kernel answers)
    ri, hi = ri.clamp(0, max(ref.size(0) - 1, 0)), hi.clamp(0, max(hyp.size(0) - 1, 0))
    Lr = ref_len[ri] if ref.size(0) else torch.zeros(N, dtype=torch.int64)
    Lh = hyp_len[hi] if hyp.size(0) else torch.zeros(N, dtype=torch.int64)
    ok &= (Lr >= 0) & (Lr <= ref.size(1)) & (Lh >= 0) & (Lh <= hyp.size(1))
    Lr, Lh = torch.where(ok, Lr, 0), torch.where(ok, Lh, 0)
    R, W = (int(Lr.max()), int(Lh.max())) if N else (0, 0)
    r = ref[ri, :R] if ref.size(0) else torch.zeros(N, 0, dtype=torch.int64)
    h = hyp[hi, :W] if hyp.size(0) else torch.zeros(N, 0, dtype=torch.int64)
    cols = torch.arange(W + 1)
    S1, D1, I1 = 1, 1 << 21, 1 << 42                                                   # the three counts in one int64
    d = cols.repeat(N, 1)                                                              # D[0][j] = j insertions
    c = d * I1
    keep = torch.zeros(N, R + 1, W + 1, dtype=torch.int8) if path else None
    if path:
        keep[:, 0, 1:] = INS
    for i in range(1, R + 1):
        ne = (r[:, i - 1:i] != h).to(torch.int64)                                      # [N, W]
        cand_d, cand_c = d[:, :-1] + ne, c[:, :-1] + ne * S1                           # the diagonal first
        up = d[:, 1:] + 1 < cand_d                                                     # then a deletion, only if strictly better
        cand_d, cand_c = torch.where(up, d[:, 1:] + 1, cand_d), torch.where(up, c[:, 1:] + D1, cand_c)
        cand_d = torch.cat([torch.full((N, 1), i, dtype=torch.int64), cand_d], 1)      # D[i][0] = i deletions
        cand_c = torch.cat([torch.full((N, 1), i * D1, dtype=torch.int64), cand_c], 1)
        # an insertion only if strictly better: D[i][j] = min_{j' <= j} cand[j'] + (j - j'), taken from the nearest cell to the left
        # that is not itself an insertion
        new_d = torch.cummin(cand_d - cols, 1).values + cols
        ins = new_d < cand_d
        src = torch.cummax(torch.where(ins, -1, cols.expand(N, -1)), 1).values
        new_c = cand_c.gather(1, src) + (cols - src) * I1
        live = (Lr >= i)[:, None]
        d, c = torch.where(live, new_d, d), torch.where(live, new_c, c)
        if path:
            keep[:, i, 0] = DEL
            keep[:, i, 1:] = torch.where(ins[:, 1:], INS, torch.where(up, DEL, ne)).to(torch.int8)
    at = Lh[:, None]
    fd, fc = d.gather(1, at)[:, 0], c.gather(1, at)[:, 0]
    counts = torch.stack([fd, fc & (D1 - 1), (fc >> 21) & (D1 - 1), fc >> 42], 1)
    counts = torch.where(ok[:, None], counts, -1).to(torch.int32)
    if not path:
        return counts.to(dev)
    cap = max(ref.size(1) + hyp.size(1), 1)
    out = torch.full((N, cap), OPS_PAD, dtype=ops_dtype)
    n_ops = torch.zeros(N, dtype=torch.int32)
    for p in range(N):
        if not bool(ok[p]):
            continue
        i, j, seq = int(Lr[p]), int(Lh[p]), []
        kp = keep[p]
        while i > 0 or j > 0:
            o = int(kp[i, j])
            seq.append(o)
            if o <= SUB:
                i, j = i - 1, j - 1
            elif o == DEL:
                i -= 1
            else:
                j -= 1
        n_ops[p] = len(seq)
        out[p, :len(seq)] = torch.tensor(seq[::-1], dtype=ops_dtype)
    return counts.to(dev), out.to(dev), n_ops.to(dev)


def oracle_error(ref: torch.Tensor, ref_len: torch.Tensor, nbest: torch.Tensor, nbest_len: torch.Tensor, *, ops=None,
                 composed: bool = False):
    """The oracle error of an n-best list: ref [B, Wr] with ref_len [B], nbest [B, K, W] with nbest_len [B, K] -> (index [B] int64 of
    the hypothesis nearest to the reference, ties to the lower index; counts int32 [B, 4] of that hypothesis; counts int32 [B, K, 4] of
    all).  B x K pairs in one launch, the reference read through its index, nothing copied."""
    B, K, W = nbest.shape
    dev = nbest.device
    ri = torch.arange(B, device=dev, dtype=torch.int32).repeat_interleave(K)
    counts = edit_distance(ops, ref, ref_len, nbest.reshape(B * K, W), nbest_len.reshape(B * K), ref_idx=ri, composed=composed)
    counts = counts.view(B, K, 4)
    key = counts[:, :, 0].to(torch.int64) * K + torch.arange(K, device=counts.device)   # the minimum, then the lower index
    idx = key.argmin(1)
    return idx, counts[torch.arange(B, device=counts.device), idx], counts


def mbr_select(nbest: torch.Tensor, nbest_len: torch.Tensor, scores: torch.Tensor, *, ops=None, composed: bool = False):
    """Minimum-Bayes-risk selection: nbest [B, K, W] with nbest_len [B, K] and scores [B, K] (log-domain, -inf for an absent entry) ->
    (index [B] int64, risk [B, K] fp64).  risk[b, i] = sum_j softmax(scores[b])_j * distance(nbest[b, i], nbest[b, j]), summed in fp64
    in index order; the lowest risk wins, ties to the lower index; an absent entry's risk is +inf.  B x K x K pairs in one launch, the
    list on both sides."""
    B, K, W = nbest.shape
    dev = nbest.device
    flat, flat_len = nbest.reshape(B * K, W), nbest_len.reshape(B * K)
    base = (torch.arange(B, device=dev, dtype=torch.int32) * K)[:, None, None]
    k = torch.arange(K, device=dev, dtype=torch.int32)
    ri = (base + k[None, :, None]).expand(B, K, K).reshape(-1)
    hi = (base + k[None, None, :]).expand(B, K, K).reshape(-1)
    counts = edit_distance(ops, flat, flat_len, flat, flat_len, ref_idx=ri, hyp_idx=hi, composed=composed)
    dist = counts[:, 0].view(B, K, K).to(torch.float64)
    w = torch.softmax(scores.to(device=dist.device, dtype=torch.float64), 1)
    risk = torch.zeros(B, K, dtype=torch.float64, device=dist.device)
    for j in range(K):                                                                  # a fixed order of summation
        risk = risk + torch.where(w[:, j:j + 1] > 0, w[:, j:j + 1] * dist[:, :, j], 0.0)
    risk = torch.where(torch.isinf(scores.to(risk.device)) & (scores.to(risk.device) < 0), float("inf"), risk)
    kk = torch.arange(K, device=risk.device)
    idx = torch.where(risk == risk.min(1, keepdim=True).values, kk, K).min(1).values
    return idx, risk


def error_sums(counts: torch.Tensor, ref_len: torch.Tensor) -> torch.Tensor:
    """counts int32 [N, 4] of N sentences and their reference lengths [N] -> int64 [5] = sums of (errors, sub, del, ins, ref_labels),
    on the counts' device: what an error rate is made of, and what sharding.reduce_error_counts adds up over ranks"""
    return torch.cat([counts.to(torch.int64).sum(0), ref_len.to(counts.device, torch.int64).sum().view(1)])


def error_rate(sums) -> float:
    """100 * errors / reference labels of error_sums (a host read)"""
    s = [int(x) for x in sums]
    return 100.0 * s[0] / s[4] if s[4] else 0.0
