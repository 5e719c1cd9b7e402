"""What a user does with the encoder's CTC head: read its best path, and score a given transcript.

``ctc_greedy`` takes the head's per-row pick straight out of the projection (Ops.linear_pick: simulst_linear with
SIMULST_EPI_ROW_PICK -- the [B, Te, V] logits never reach memory), ``ctc_collapse`` turns a path into a transcript with a frame stamp per
token, ``ctc_report`` is the accuracy report of the reference's JointCTCCriterion (criterion/joint_ctc_criterion.py:24-48, 92-101) and
``CTCTranscriber.transcribe_ctc`` the model-level call: encoder forward + greedy path.

``ctc_score`` is the CTC loss value of given transcripts (the sum over alignments, F.ctc_loss of criterion/joint_ctc_criterion.py:78-90
and the CTC term of criterion/cif_criterion.py), optionally with the forced alignment: the projection writes only the log-probabilities
of the blank and of the transcript's own labels, [B, Te, L + 1] (Ops.linear_gather: SIMULST_EPI_ROW_GATHER), and the recursion of
ctc_align.ctc_nll runs over them.  ``ctc_rescore`` re-ranks n-best lists with that score, one gather per utterance for all its
hypotheses, and ``CTCTranscriber.score_ctc`` is the model-level call.

``ctc_topk`` is the head's per-frame candidate list -- the blank and the best k other labels with their log-probabilities, again
without the logits (Ops.linear_topk: SIMULST_EPI_ROW_TOPK) --, ``ctc_prefix_beam_advance`` the time-synchronous prefix beam search over
such lists (on the GPU every frame of a call in ONE launch, simulst_ctc_prefix_beam in csrc/ctc_prefix.hip, with
the same recursion as device tensor operations kept as the comparison; the state goes in and comes out, so that chunks of rows continue
one search), ``ctc_prefix_beam_search`` the two together and ``CTCTranscriber.transcribe_ctc_nbest`` the model-level call,
whose hypotheses ``ctc_rescore`` gives their exact likelihoods.  No language model is fused in, and no gradient is computed.

``CTCPrefixScorer`` is the CTC side of joint CTC / attention decoding: inside the attention beam search (beam.BeamSearch, rescore=)
every candidate of every step is scored by the CTC prefix probability of the extended string -- ``ctc_prefix_score``, one launch a step
(simulst_ctc_prefix_score, csrc/ctc_prefix_score.hip) over log-probabilities gathered at the candidates alone --
and ``ctc_prefix_commit`` moves the chosen candidates' states behind the selection; both have a torch form (composed=True).

The blank index is a keyword everywhere (default 0, the criterion's fallback, joint_ctc_criterion.py:76).

``token_error_report`` counts the ERRORS of hypotheses against references (edit distance and its substitutions / deletions / insertions,
summed over the batch on the device: simulst_amd/edit_distance.py, csrc/edit_distance.hip) where ``ctc_report`` counts bag-of-labels
matches; ``CTCTranscriber.ctc_error_report`` runs it over the head's greedy transcript.
"""
from typing import Dict, List, Optional

import torch

SHIFT_MS = 10          # fbank frame shift (agent.SHIFT_SIZE)


def ctc_collapse(path: torch.Tensor, lengths: torch.Tensor, blank: int = 0, pad: int = 1):
    """path [B, T] integer labels, lengths [B] -> (tokens [B, Lmax] int64 padded with `pad`, n [B] int64, frames [B, Lmax] int32 padded
    with -1).  Row t keeps its label iff t < lengths[b], path[b, t] != blank and (t == 0 or path[b, t] != path[b, t - 1]); frames holds
    the row at which the kept label's run starts.  Tensor ops only (one read-back: Lmax); CPU and device tensors alike."""
    B, T = path.shape
    dev = path.device
    lengths = torch.as_tensor(lengths, device=dev).to(torch.int64)
    t = torch.arange(T, device=dev)
    starts = torch.ones(B, T, dtype=torch.bool, device=dev)
    if T > 1:
        starts[:, 1:] = path[:, 1:] != path[:, :-1]
    keep = (t.unsqueeze(0) < lengths.unsqueeze(1)) & (path != blank) & starts
    n = keep.sum(1)
    Lmax = int(n.max().item()) if B and T else 0
    tokens = torch.full((B, Lmax), pad, dtype=torch.int64, device=dev)
    frames = torch.full((B, Lmax), -1, dtype=torch.int32, device=dev)
    if Lmax:
        slot = keep.cumsum(1) - 1
        b_idx, t_idx = keep.nonzero(as_tuple=True)
        tokens[b_idx, slot[b_idx, t_idx]] = path[b_idx, t_idx].to(torch.int64)
        frames[b_idx, slot[b_idx, t_idx]] = t_idx.to(torch.int32)
    return tokens, n, frames


def _label_counts(tokens: torch.Tensor, n_labels: int) -> torch.Tensor:
    c = torch.zeros(tokens.size(0), n_labels, dtype=torch.int64, device=tokens.device)
    return c.scatter_add_(1, tokens, torch.ones_like(tokens))


def ctc_report(path: torch.Tensor, lengths: Optional[torch.Tensor], target: torch.Tensor, blank: int = 0, pad: int = 1,
               eps: float = 1e-8) -> Dict[str, torch.Tensor]:
    """The accuracy report of JointCTCCriterion over a batch, as SUMS over its sentences like the criterion logs them: path [N, S] (the
    head's argmax), target [N, T] padded with `pad` ->
      recall     sum_n match_n / (#target_n != pad + eps)      match_n = sum over labels of min(count in path_n, count in target_n)
      precision  sum_n match_n / (#path_n != blank + eps)        (every label counts, frame by frame: no collapse, as in the reference)
      blank_rate sum_n mean_s [path_n,s == blank]
    With lengths=None this is the reference's calc_recall_precision and blank rate exactly.  With lengths [N], rows at and past
    lengths[n] count as blank -- which the reference does NOT do: it takes the argmax of the padded rows as it comes, so a padded batch
    there reports whatever the head says about padding."""
    path = path.to(torch.int64)
    target = target.to(device=path.device, dtype=torch.int64)
    if lengths is not None:
        lengths = torch.as_tensor(lengths, device=path.device).to(torch.int64)
        inside = torch.arange(path.size(1), device=path.device).unsqueeze(0) < lengths.unsqueeze(1)
        path = torch.where(inside, path, torch.full_like(path, blank))
    n_labels = int(max(path.max().item() if path.numel() else 0, target.max().item() if target.numel() else 0)) + 1
    match = torch.minimum(_label_counts(target, n_labels), _label_counts(path, n_labels)).sum(-1)
    recall = match / (target.ne(pad).sum(-1) + eps)
    precision = match / (path.ne(blank).sum(-1) + eps)
    return {"recall": recall.sum(), "precision": precision.sum(), "blank_rate": path.eq(blank).float().mean(-1).sum()}


def token_error_report(tokens: torch.Tensor, n: torch.Tensor, target: torch.Tensor, target_lengths: torch.Tensor, *, ops=None,
                       composed: bool = False) -> Dict[str, torch.Tensor]:
    """The companion of ctc_report that counts ERRORS: tokens [B, L] with n [B] labels each (ctc_collapse's output, or any hypotheses)
    against target [B, T] with target_lengths [B] -> the batch's SUMS {"errors", "sub", "del", "ins", "ref_labels"} as int64 scalars on
    the tokens' device, with no host read-back.  errors / ref_labels is the token error rate (edit_distance.py: one launch over the
    batch, the alignment's tie rule there); sums of several batches or ranks add (sharding.reduce_error_counts)."""
    from .edit_distance import edit_distance, error_sums
    target = target.to(device=tokens.device, dtype=torch.int64)
    target_lengths = torch.as_tensor(target_lengths, device=tokens.device).to(torch.int64)
    counts = edit_distance(ops, target, target_lengths, tokens.to(torch.int64), torch.as_tensor(n, device=tokens.device).to(torch.int64),
                           composed=composed)
    s = error_sums(counts, target_lengths)
    return {"errors": s[0], "sub": s[1], "del": s[2], "ins": s[3], "ref_labels": s[4]}


def ctc_greedy(ops, head_w: torch.Tensor, enc_btd: torch.Tensor, enc_len: torch.Tensor, *, blank: int = 0, pad: int = 1,
               head_b: Optional[torch.Tensor] = None):
    """Best path of the head over encoder rows enc_btd [B, Te, D] (any batch stride), enc_len [B] valid rows ->
    {"path" [B, Te] int32 (blank past the length), "lprob" [B, Te] fp32 log-probability of the picked label (0 past the length),
     "tokens" / "n" / "frames" (ctc_collapse of the path), "score" [B] = sum of lprob over the valid rows}."""
    pick, zmax, lse = ops.linear_pick(enc_btd, head_w, head_b)
    Te = enc_btd.size(1)
    enc_len = torch.as_tensor(enc_len, device=pick.device).to(torch.int64)
    inside = torch.arange(Te, device=pick.device).unsqueeze(0) < enc_len.unsqueeze(1)
    path = torch.where(inside, pick, torch.full_like(pick, blank))
    lprob = torch.where(inside, zmax - lse, torch.zeros_like(zmax))
    tokens, n, frames = ctc_collapse(path, enc_len, blank, pad)
    return {"path": path, "lprob": lprob, "tokens": tokens, "n": n, "frames": frames, "score": lprob.sum(1)}


def ctc_columns(targets: torch.Tensor) -> torch.Tensor:
    """targets [B, L] labels -> [B, L] int64 column ids into a matrix gathered at [blank, targets...]: position j lies in column j + 1,
    and CONSECUTIVE EQUAL labels share a column (col[j] = col[j - 1] if targets[j] == targets[j - 1] else j + 1), so that the
    recursion's repeated-label rule -- no s-2 move between equal labels, which it decides by comparing the ids it is given -- reads the
    same on column ids as on labels.  (A plain 1..L would allow the skip across "aa".)  Equal labels hold equal values in the gathered
    matrix, so reading the run's first column changes nothing else."""
    B, L = targets.shape
    pos = torch.arange(1, L + 1, device=targets.device, dtype=torch.int64).unsqueeze(0).expand(B, L)
    if L < 2:
        return pos.clone()
    start = torch.ones(B, L, dtype=torch.bool, device=targets.device)
    start[:, 1:] = targets[:, 1:] != targets[:, :-1]
    return torch.where(start, pos, torch.zeros_like(pos)).cummax(dim=1).values


def _gather_labels(targets: torch.Tensor, target_lengths: torch.Tensor, blank: int) -> torch.Tensor:
    """[B, L] targets -> int32 [B, L + 1] label list of the gather: the blank, then the transcript (blank again past its length)"""
    B, L = targets.shape
    inside = torch.arange(L, device=targets.device).unsqueeze(0) < target_lengths.unsqueeze(1)
    lab = torch.full((B, L + 1), blank, dtype=torch.int32, device=targets.device)
    lab[:, 1:] = torch.where(inside, targets, torch.full_like(targets, blank)).to(torch.int32)
    return lab


def ctc_score(ops, head_w: torch.Tensor, enc_btd: torch.Tensor, enc_len: torch.Tensor, targets: torch.Tensor,
              target_lengths: torch.Tensor, *, blank: int = 0, pad: int = 1, head_b: Optional[torch.Tensor] = None,
              align: bool = False) -> Dict[str, torch.Tensor]:
    """How likely the head finds given transcripts: targets [B, Lmax] (padded with `pad` past target_lengths [B]) over encoder rows
    enc_btd [B, Te, D] (any batch stride), enc_len [B] valid rows ->
      "nll"    [B] fp32: the CTC negative log-likelihood, F.ctc_loss(reduction="none") (criterion/joint_ctc_criterion.py:78-90);
               +inf where the transcript does not fit into the rows
      "lprobs" [B, Te, Lmax + 1] fp32: the head's log-probabilities at the blank (column 0) and at the transcript's labels -- all
               the recursion reads.  The [B, Te, V] logits are never written (Ops.linear_gather, SIMULST_EPI_ROW_GATHER).
    align=True adds "alignment" [B, Te] int64 (the label of every frame on the best path, blank past the length) and "best_nll" [B]
    (ctc_align.best_alignment's return_nll) from the Viterbi run over the same gathered matrix."""
    from . import ctc_align
    dev = enc_btd.device
    B, Te = enc_btd.shape[:2]
    targets = torch.as_tensor(targets, device=dev).to(torch.int64)
    if targets.dim() != 2 or targets.size(0) != B:
        raise ValueError("ctc_score: targets is [B, Lmax]")
    tl = torch.as_tensor(target_lengths, device=dev).to(torch.int64)
    il = torch.as_tensor(enc_len, device=dev).to(torch.int64)
    lab = _gather_labels(targets, tl, blank)
    lprobs = ops.linear_gather(enc_btd, head_w, head_b, lab)
    cols = ctc_columns(targets)
    lp_sbv = lprobs.transpose(0, 1)                          # (S, N, V') view: the recursion takes any strides
    out = {"nll": ctc_align.ctc_nll(lp_sbv, cols, il, tl, blank=0, ops=ops), "lprobs": lprobs}
    if align:
        states, best = ctc_align.best_alignment(lp_sbv, cols, il, tl, blank=0, as_labels=True, ops=ops, return_nll=True)
        out["alignment"] = lab.to(torch.int64).gather(1, states)             # column id -> label
        out["best_nll"] = best
    return out


def ctc_rescore(ops, head_w: torch.Tensor, enc_btd: torch.Tensor, enc_len: torch.Tensor, nbest, *, weight: float, blank: int = 0,
                head_b: Optional[torch.Tensor] = None) -> List[List[dict]]:
    """Re-rank n-best lists with the head's CTC score: nbest[b] is the list of (tokens, score) of utterance b (at least one; lists
    shorter than the longest, n, leave their last slots of the gather empty; tokens without blanks) -> per utterance the hypotheses sorted by
      "combined" = (1 - weight) * score + weight * (-nll),
    each {"tokens", "score", "nll", "combined"}.  ONE gather serves all hypotheses of an utterance: their label lists are concatenated,
    each padded to Lmax + 1 columns, and the result is written time-major [Te][B][n][Lmax + 1], which the B * n recursions read as
    (S, B * n, Lmax + 1) log-probabilities with uniform strides."""
    from . import ctc_align
    dev = enc_btd.device
    B, Te = enc_btd.shape[:2]
    if len(nbest) != B or B == 0 or any(len(h) < 1 for h in nbest):
        raise ValueError("ctc_rescore: nbest holds at least one hypothesis for each of the B utterances")
    n = max(len(h) for h in nbest)
    Lmax = max(max(len(t) for t, _ in hyps) for hyps in nbest)
    targets = torch.full((B * n, max(Lmax, 1)), blank, dtype=torch.int64)
    for b, hyps in enumerate(nbest):
        for k, (t, _) in enumerate(hyps):
            targets[b * n + k, :len(t)] = torch.as_tensor(t, dtype=torch.int64)
    tl = torch.zeros(B, n, dtype=torch.int64)
    for b, hyps in enumerate(nbest):
        tl[b, :len(hyps)] = torch.tensor([len(t) for t, _ in hyps], dtype=torch.int64)
    tl = tl.view(-1).to(dev)
    targets = targets[:, :Lmax].to(dev)
    lab = _gather_labels(targets, tl, blank).view(B, n * (Lmax + 1))
    buf = torch.empty(Te, B, n * (Lmax + 1), device=dev, dtype=torch.float32)
    ops.linear_gather(enc_btd, head_w, head_b, lab, out=buf.transpose(0, 1))
    il = torch.as_tensor(enc_len, device=dev).to(torch.int64).repeat_interleave(n)
    nll = ctc_align.ctc_nll(buf.view(Te, B * n, Lmax + 1), ctc_columns(targets), il, tl, blank=0, ops=ops).cpu()
    ranked = []
    for b, hyps in enumerate(nbest):
        rows = [{"tokens": list(t), "score": float(s), "nll": float(nll[b * n + k]),
                 "combined": (1.0 - weight) * float(s) + (weight * -float(nll[b * n + k]) if weight else 0.0)}
                for k, (t, s) in enumerate(hyps)]
        ranked.append(sorted(rows, key=lambda r: -r["combined"]))
    return ranked


def ctc_topk(ops, head_w: torch.Tensor, enc_btd: torch.Tensor, enc_len: torch.Tensor, *, k: int = 8, blank: int = 0,
             head_b: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The head's candidates of every frame of enc_btd [B, Te, D] (any batch stride), enc_len [B] valid rows ->
    {"ids" [B, Te, k + 1] int32: slot 0 the blank, then the k other labels with the largest logits, descending, lower label first on
     equal logits, -1 where the vocabulary has fewer; "lprob" [B, Te, k + 1] fp32 their log-probabilities (-inf at -1); "lse" [B, Te]}.
    Past the length a frame holds ids -1 except the blank slot and lprob 0 at the blank, -inf elsewhere.  The logits are never
    written (Ops.linear_topk)."""
    ids, lprob, lse = ops.linear_topk(enc_btd, head_w, head_b, k=k, keep=blank)
    Te = enc_btd.size(1)
    enc_len = torch.as_tensor(enc_len, device=ids.device).to(torch.int64)
    inside = (torch.arange(Te, device=ids.device).unsqueeze(0) < enc_len.unsqueeze(1)).unsqueeze(-1)
    pad_ids = torch.full_like(ids, -1)
    pad_ids[..., 0] = blank
    pad_lp = torch.full_like(lprob, float("-inf"))
    pad_lp[..., 0] = 0.0
    return {"ids": torch.where(inside, ids, pad_ids), "lprob": torch.where(inside, lprob, pad_lp), "lse": lse}


BEAM_MAX = 16


def _lae(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """log(exp a + exp b), -inf where both are: max + log1p(exp(-|a - b|))"""
    d = -(a - b).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float("-inf")), d)
    return torch.maximum(a, b) + torch.log1p(torch.exp(d))


def ctc_prefix_beam_init(B: int, beam: int, device, pad: int = 1):
    """The state before the first frame: (strings [B, beam, 0] int64, lengths [B, beam] int64, p_b [B, beam], p_nb [B, beam] fp32) --
    slot 0 the empty prefix at (0, -inf), the other slots empty (-inf, -inf).  Slots are kept in descending order of p_b (+) p_nb."""
    ninf = float("-inf")
    p_b = torch.full((B, beam), ninf, dtype=torch.float32, device=device)
    p_b[:, 0] = 0.0
    return (torch.full((B, beam, 0), pad, dtype=torch.int64, device=device), torch.zeros(B, beam, dtype=torch.int64, device=device),
            p_b, torch.full((B, beam), ninf, dtype=torch.float32, device=device))


def ctc_prefix_beam_advance(ids: torch.Tensor, lprob: torch.Tensor, enc_len: torch.Tensor, state, *, pad: int = 1, ops=None,
                            composed: bool = False):
    """Time-synchronous CTC prefix beam search over candidate lists: ids [B, T, k + 1] (slot 0 the blank, -1 = no candidate), lprob
    [B, T, k + 1] fp32 (ctc_topk's outputs, or any lists of that form, any batch / frame strides), enc_len [B] frames to take of each row
    of the batch, state (strings, lengths, p_b, p_nb) as ctc_prefix_beam_init makes it -> the state after the frames (new tensors; the
    state given is not written); strings grows by T to hold them.

    Per frame and kept prefix l with last label e (pool index order: the beam's own entries first, then prefix-major, candidate-minor
    extensions):
      p_b'(l) = (p_b (+) p_nb) + lp[blank];  p_nb'(l) = p_nb + lp[e] if e is a candidate;
      p_nb'(l + c) = p_b + lp[c] if c == e else (p_b (+) p_nb) + lp[c].
    An extension that spells a prefix already in the beam is added to that entry's p_nb' (the strings are compared, label by label: a
    beam entry has ONE parent string, so at most one extension reaches it and the sum has one order) and leaves the pool; the beam
    best of the pool by p_b' (+) p_nb' survive, ties in pool index order (a stable sort).  A frame at or past enc_len[b] leaves row b's
    state as it is.

    On the GPU all T frames run in ONE launch (simulst_ctc_prefix_beam, csrc/ctc_prefix.hip: one wave per
    utterance, the strings in LDS for the call), with no read-back; `ops` is the Ops whose stream it goes to (default: a new one).  The
    same recursion as torch tensor operations -- about 120 small launches a frame -- is kept as the comparison and is what runs with
    composed=True, for CPU tensors, and where the kernel has no place for the call: strings longer than _lib.ctc_prefix_cap(beam)
    labels (1104 at beam 16, 2208 at beam 8), more than 16 prefixes or more than 8 candidates.  (Lists of the blank alone, k = 0, are the
    kernel's only: the torch form reduces over the candidates.)  Both forms hold the fp64 reference's
    bound; they need not agree in the last bit with each other, but each gives the same bits however the frames are cut into calls."""
    from ._lib import ctc_prefix_cap
    strings, lengths, p_b, p_nb = state
    B, T, kp = ids.shape
    beam = p_b.size(1)
    if composed or not ids.is_cuda or kp - 1 > 8 or not (1 <= beam <= BEAM_MAX) or strings.size(2) + T > ctc_prefix_cap(beam):
        return _prefix_beam_advance_composed(ids, lprob, enc_len, state, pad)
    if T == 0 or B == 0:
        return strings, lengths, p_b, p_nb
    import ctypes
    from ._lib import CtcPrefixDesc
    from .ops import Ops, _p
    ops = ops or Ops()
    dev = ids.device
    if ids.dtype != torch.int32 or ids.stride(2) != 1:
        ids = ids.to(torch.int32).contiguous()
    if lprob.dtype != torch.float32:
        lprob = lprob.float()
    il = torch.as_tensor(enc_len, device=dev).to(torch.int64).contiguous()
    strings = torch.cat([strings.to(torch.int64), torch.full((B, beam, T), pad, dtype=torch.int64, device=dev)], dim=2)
    lengths = lengths.to(torch.int64).clone(memory_format=torch.contiguous_format)
    p_b = p_b.float().clone(memory_format=torch.contiguous_format)
    p_nb = p_nb.float().clone(memory_format=torch.contiguous_format)
    d = CtcPrefixDesc()
    d.cand_ids, d.id_stride_b, d.id_stride_t = ids.data_ptr(), ids.stride(0), ids.stride(1)
    d.k, d.pad, d.cap = kp - 1, int(pad), strings.size(2)
    d.lengths, d.p_b, d.p_nb = lengths.data_ptr(), p_b.data_ptr(), p_nb.data_ptr()
    ops.h.check(ops.lib.simulst_ctc_prefix_beam(ops.h.ptr, _p(lprob), lprob.stride(1), lprob.stride(0), lprob.stride(2), _p(il), T, B,
                                                beam, 0, ctypes.byref(d), _p(strings)),
                "simulst_ctc_prefix_beam")
    return strings, lengths, p_b, p_nb


def _prefix_beam_advance_composed(ids, lprob, enc_len, state, pad):
    """ctc_prefix_beam_advance as device tensor operations, no read-back (and the form for CPU tensors)"""
    strings, lengths, p_b, p_nb = state
    B, T, kp = ids.shape
    k, beam, dev = kp - 1, p_b.size(1), ids.device
    ninf = float("-inf")
    enc_len = torch.as_tensor(enc_len, device=dev).to(torch.int64)
    if T:
        strings = torch.cat([strings, torch.full((B, beam, T), pad, dtype=torch.int64, device=dev)], dim=2)
    Lcap = strings.size(2)
    pos_l = torch.arange(Lcap, device=dev)
    ids = ids.to(torch.int64)
    for t in range(T):
        cid, lp = ids[:, t, 1:], lprob[:, t, 1:]                                    # [B, k] the non-blank candidates
        lp_blank = lprob[:, t, :1]                                                   # [B, 1]
        has = lengths > 0
        last = torch.where(has, strings.gather(2, (lengths - 1).clamp(min=0).unsqueeze(-1)).squeeze(-1), torch.full_like(lengths, -2))
        tot = _lae(p_b, p_nb)                                                        # [B, beam]
        live = tot > ninf
        same = (cid.unsqueeze(1) == last.unsqueeze(2)) & (cid.unsqueeze(1) >= 0)     # [B, beam, k]: candidate j repeats the last label
        lp_e = torch.where(same, lp.unsqueeze(1).expand(B, beam, k), torch.full((), ninf, device=dev)).amax(2)
        stay_b = tot + lp_blank
        stay_nb = torch.where(lp_e > ninf, p_nb + lp_e, torch.full_like(p_nb, ninf))
        ext = torch.where(same, p_b.unsqueeze(2), tot.unsqueeze(2)) + lp.unsqueeze(1)   # [B, beam, k]
        ext = torch.where((cid.unsqueeze(1) >= 0) & live.unsqueeze(2), ext, torch.full_like(ext, ninf))
        # entry i2 spells prefix i + one label: same first lengths[i] labels, one label longer
        eq = (strings.unsqueeze(2) == strings.unsqueeze(1)) | (pos_l.view(1, 1, 1, Lcap) >= lengths.view(B, beam, 1, 1))
        child = eq.all(3) & (lengths.unsqueeze(1) == lengths.unsqueeze(2) + 1) & live.unsqueeze(1) & live.unsqueeze(2)   # [B, i, i2]
        nxt = strings.gather(2, lengths.clamp(max=Lcap - 1).unsqueeze(1).expand(B, beam, beam))    # [B, i2, i] = strings[i2][lengths[i]]
        hit = child.unsqueeze(3) & (nxt.transpose(1, 2).unsqueeze(3) == cid.view(B, 1, 1, k))      # [B, i, i2, j]
        gain = torch.where(hit, ext.unsqueeze(2), torch.full((), ninf, device=dev)).amax(dim=(1, 3))   # [B, i2]: at most one term
        stay_nb = _lae(stay_nb, gain)
        ext = torch.where(hit.any(2), torch.full_like(ext, ninf), ext)
        pool_b = torch.cat([stay_b, torch.full((B, beam * k), ninf, device=dev)], dim=1)
        pool_nb = torch.cat([stay_nb, ext.reshape(B, beam * k)], dim=1)
        order = torch.sort(_lae(pool_b, pool_nb), dim=1, descending=True, stable=True).indices[:, :beam]     # [B, beam] pool indices
        n_b, n_nb = pool_b.gather(1, order), pool_nb.gather(1, order)
        grown = order >= beam
        e_idx = (order - beam).clamp(min=0)
        src = torch.where(grown, e_idx // max(k, 1), order)
        tok = cid.gather(1, e_idx % max(k, 1)) if k else torch.zeros_like(order)
        n_len = lengths.gather(1, src)
        n_str = strings.gather(1, src.unsqueeze(-1).expand(B, beam, Lcap))
        at = n_len.clamp(max=Lcap - 1).unsqueeze(-1)
        n_str = n_str.scatter(2, at, torch.where(grown.unsqueeze(-1), tok.unsqueeze(-1), n_str.gather(2, at)))
        n_len = n_len + grown.to(torch.int64)
        dead = ~(_lae(n_b, n_nb) > ninf)
        n_len = torch.where(dead, torch.zeros_like(n_len), n_len)
        n_str = torch.where(dead.unsqueeze(-1), torch.full_like(n_str, pad), n_str)
        on = (enc_len > t).unsqueeze(1)
        strings = torch.where(on.unsqueeze(-1), n_str, strings)
        lengths = torch.where(on, n_len, lengths)
        p_b, p_nb = torch.where(on, n_b, p_b), torch.where(on, n_nb, p_nb)
    return strings, lengths, p_b, p_nb


def ctc_prefix_beam_search(ops, head_w: torch.Tensor, enc_btd: torch.Tensor, enc_len: torch.Tensor, *, beam: int = 8, candidates: int = 8,
                           nbest: int = 1, blank: int = 0, pad: int = 1, head_b: Optional[torch.Tensor] = None, state=None,
                           return_state: bool = False, composed: bool = False):
    """Prefix beam search over the head's top `candidates` labels of every frame (ctc_topk + ctc_prefix_beam_advance) ->
    {"tokens" [B, nbest, Lmax] int64 padded with `pad`, "n" [B, nbest], "score" [B, nbest] = log(p_b + p_nb), descending; a slot the
    search has no prefix for holds n = 0 and score -inf} and, with return_state, "state" to pass to the next call: rows released chunk
    by chunk (encoder.infer) give the bits one call over all rows gives.  1 <= nbest <= beam <= 16, 1 <= candidates <= 8.  The frame
    loop runs on the device, in one launch (composed=True: as tensor operations, ctc_prefix_beam_advance); the one read-back is Lmax."""
    if not (1 <= nbest <= beam <= BEAM_MAX):
        raise ValueError("ctc_prefix_beam_search: 1 <= nbest <= beam <= 16")
    B = enc_btd.size(0)
    cand = ctc_topk(ops, head_w, enc_btd, enc_len, k=candidates, blank=blank, head_b=head_b)
    if state is None:
        state = ctc_prefix_beam_init(B, beam, enc_btd.device, pad)
    elif state[2].shape != (B, beam):
        raise ValueError("ctc_prefix_beam_search: state belongs to another batch or beam")
    strings, lengths, p_b, p_nb = ctc_prefix_beam_advance(cand["ids"], cand["lprob"], enc_len, state, pad=pad, ops=ops, composed=composed)
    Lmax = int(lengths.max().item()) if B else 0
    strings = strings[:, :, :Lmax].contiguous()
    out = {"tokens": strings[:, :nbest], "n": lengths[:, :nbest], "score": _lae(p_b, p_nb)[:, :nbest]}
    if return_state:
        out["state"] = (strings, lengths, p_b, p_nb)
    return out


SCORE_FLOOR = -1.0e4      # the CTC term of an extension no alignment spells (PS_FLOOR of csrc/ctc_prefix_score.hip)
SCORE_KMAX = 32


def ctc_prefix_score(ops, x, xb, state, psi, last, plen, in_len, finished, cand_lp, cand_tok, cand_slot, cand_state, cand_psi, *,
                     G: int, blank: int, eos: int, pad: int, weight: float, first_only: bool = False, composed: bool = False):
    """One step's CTC prefix scores (DESIGN.md "Beam search", "CTC prefix scores inside the beam"; simulst_ctc_prefix_score,
    csrc/ctc_prefix_score.hip), for R = Bs * G beam rows of K candidates each:
      x [Bs, S, G * K] fp32 (any strides): the candidates' log-probabilities under the head;  xb [Bs, S] fp32: the blank's
      state [R, S, 2] fp32 (gn, gb), psi [R] fp32, last [R] int64, plen [R] int64: the rows' hypotheses;  in_len [R] int64 frames
      finished [Bs] int32 or None;  cand_lp [R, K] fp32 / cand_tok [R, K] int32: simulst_beam_topk's lists, REWRITTEN in place
      (combined score, candidate order);  cand_slot [R, K] int32, cand_state [R, S, K, 2], cand_psi [R, K]: outputs.
    Rows of finished sentences, and with first_only the rows j > 0, are left as they are.  composed=True (and CPU tensors): the same
    arithmetic as torch tensor operations over rows x candidates with a Python loop over the frames."""
    R, K = cand_tok.shape
    S = state.size(1)
    if composed or not cand_tok.is_cuda:
        return _prefix_score_composed(x, xb, state, psi, last, plen, in_len, finished, cand_lp, cand_tok, cand_slot, cand_state,
                                      cand_psi, G=G, blank=blank, eos=eos, pad=pad, weight=weight, first_only=first_only)
    import ctypes
    from ._lib import CtcScoreDesc
    from .ops import _chk_contig, _p
    _chk_contig(xb[0] if xb.size(0) else xb, state, psi, last, plen, in_len, finished, cand_lp, cand_tok, cand_slot, cand_state, cand_psi)
    assert x.dtype == torch.float32 and xb.dtype == torch.float32 and tuple(x.shape[:2]) == (R // G, S) and x.size(2) == G * K
    assert cand_tok.dtype == torch.int32 and cand_slot.dtype == torch.int32 and last.dtype == plen.dtype == in_len.dtype == torch.int64
    assert tuple(cand_state.shape) == (R, S, K, 2) and tuple(state.shape) == (R, S, 2)
    d = CtcScoreDesc()
    d.op, d.G, d.eos, d.pad, d.weight, d.first_only = 0, int(G), int(eos), int(pad), float(weight), int(bool(first_only))
    d.blank_lp, d.blank_stride_b = xb.data_ptr(), xb.stride(0)
    d.state, d.psi, d.cand_state, d.cand_psi = state.data_ptr(), psi.data_ptr(), cand_state.data_ptr(), cand_psi.data_ptr()
    d.cand_lp, d.cand_tok, d.cand_slot = cand_lp.data_ptr(), cand_tok.data_ptr(), cand_slot.data_ptr()
    d.finished = finished.data_ptr() if finished is not None else None
    ops.h.check(ops.lib.simulst_ctc_prefix_score(ops.h.ptr, _p(x), x.stride(1), x.stride(0), x.stride(2), _p(last), _p(in_len), _p(plen),
                                                 S, R, K, int(blank), ctypes.byref(d)),
                "simulst_ctc_prefix_score")


def ctc_prefix_commit(ops, cand_state, cand_psi, cand_tok, cand_slot, next_tok, reorder, finished, last, plen, in_len, state_out,
                      psi_out, last_out, len_out, result, *, G: int, composed: bool = False):
    """Behind simulst_beam_select: row r of an unfinished sentence takes the state and psi of candidate next_tok[r] (int64 [R]) of its
    parent row reorder[r] (int32 [R]) into state_out [R, S, 2] / psi_out [R], last_out[r] = next_tok[r], len_out[r] = plen[parent] + 1.
    A token that is not among the parent's candidates (or a parent outside the sentence) adds 1 to result[0] (int32) and leaves the
    row.  `last` is unused."""
    R, K = cand_tok.shape
    S = state_out.size(1)
    if composed or not cand_tok.is_cuda:
        return _prefix_commit_composed(cand_state, cand_psi, cand_tok, cand_slot, next_tok, reorder, finished, plen, in_len, state_out,
                                       psi_out, last_out, len_out, result, G=G)
    import ctypes
    from ._lib import CtcScoreDesc
    from .ops import _chk_contig, _p
    _chk_contig(cand_state, cand_psi, cand_tok, cand_slot, next_tok, reorder, finished, last, plen, in_len, state_out, psi_out, last_out,
                len_out)
    assert next_tok.dtype == torch.int64 and reorder.dtype == torch.int32 and result.dtype == torch.int32
    assert tuple(cand_state.shape) == (R, S, K, 2) and tuple(state_out.shape) == (R, S, 2)
    d = CtcScoreDesc()
    d.op, d.G = 1, int(G)
    d.cand_state, d.cand_psi, d.cand_tok, d.cand_slot = cand_state.data_ptr(), cand_psi.data_ptr(), cand_tok.data_ptr(), cand_slot.data_ptr()
    d.finished = finished.data_ptr() if finished is not None else None
    d.next_tok, d.reorder, d.state_out, d.psi_out = next_tok.data_ptr(), reorder.data_ptr(), state_out.data_ptr(), psi_out.data_ptr()
    d.last_out, d.len_out, d.result = last_out.data_ptr(), len_out.data_ptr(), result.data_ptr()
    ops.h.check(ops.lib.simulst_ctc_prefix_score(ops.h.ptr, _p(None), 0, 0, 0, _p(None), _p(in_len), _p(plen), S, R, K, 0,
                                                 ctypes.byref(d)),
                "simulst_ctc_prefix_score (commit)")


def _score_rows(R, G, finished, first_only, dev):
    """[R] bool: the rows a scoring step touches"""
    act = torch.ones(R, dtype=torch.bool, device=dev)
    if finished is not None:
        act &= ~finished.bool().repeat_interleave(G)
    if first_only:
        act &= (torch.arange(R, device=dev) % G) == 0
    return act


def _prefix_score_composed(x, xb, state, psi, last, plen, in_len, finished, cand_lp, cand_tok, cand_slot, cand_state, cand_psi, *, G,
                           blank, eos, pad, weight, first_only):
    R, K = cand_tok.shape
    S, dev = state.size(1), cand_tok.device
    ninf = torch.full((), float("-inf"), device=dev)
    act = _score_rows(R, G, finished, first_only, dev)
    xr = x.reshape(R // G, S, G, K).permute(0, 2, 1, 3).reshape(R, S, K)
    xbr = xb.repeat_interleave(G, 0)
    tok = cand_tok.to(torch.int64)
    special = (tok < 0) | (tok == blank) | (tok == pad)
    ext = ~special & (tok != eos)
    is_eos = ~special & (tok == eos)
    empty = (plen <= 0).unsqueeze(1)
    same = ext & ~empty & (tok == last.unsqueeze(1))
    T = in_len.clamp(0, S)
    inside = torch.arange(S, device=dev).unsqueeze(0) < T.unsqueeze(1)                 # [R, S]
    gb_g = torch.where(inside, state[..., 1], ninf)
    tot_g = torch.where(inside, _lae(torch.where(inside, state[..., 0], ninf), gb_g), ninf)
    pn = torch.full((R, K), float("-inf"), device=dev)
    pb, acc = pn.clone(), pn.clone()
    phi = torch.where(empty, torch.zeros((), device=dev), ninf).expand(R, K)
    new_state = cand_state.clone()
    for t in range(S):
        on = inside[:, t:t + 1]
        if not bool(on.any()):
            break
        xt = torch.where(ext & on, xr[:, t], ninf)
        gn = _lae(pn, phi) + xt
        gb = _lae(pn, pb) + torch.where(on, xbr[:, t:t + 1], torch.zeros((), device=dev))
        acc = torch.where(on, _lae(acc, phi + xt), acc)
        new_state[:, t] = torch.where((on & act.unsqueeze(1)).unsqueeze(-1), torch.stack([gn, gb], dim=-1), new_state[:, t])
        pn, pb = torch.where(on, gn, pn), torch.where(on, gb, pb)
        phi = torch.where(on, torch.where(same, gb_g[:, t:t + 1], tot_g[:, t:t + 1]), phi)
    psi_end = torch.where(T > 0, tot_g.gather(1, (T - 1).clamp(min=0).unsqueeze(1)).squeeze(1),
                          torch.where(empty.squeeze(1), torch.zeros((), device=dev), ninf))
    psi_h = torch.where(ext, acc, torch.where(is_eos, psi_end.unsqueeze(1), ninf))
    floor = torch.full((), SCORE_FLOOR, device=dev)
    dead = psi_h == ninf
    delta = torch.where(dead, floor, torch.maximum(torch.where(dead, floor, psi_h) - psi.unsqueeze(1), floor))
    delta = torch.where(torch.isnan(delta), floor, delta)
    if weight == 0:
        sc = cand_lp.clone()
    else:
        sc = torch.where(cand_lp == ninf, ninf, (1.0 - weight) * cand_lp + weight * delta)
    # candidate order: descending score, equal scores to the lower token (then the lower slot): two stable sorts
    by_tok = torch.sort(tok, dim=1, stable=True).indices
    order = by_tok.gather(1, torch.sort(sc.gather(1, by_tok), dim=1, descending=True, stable=True).indices)
    a = act.unsqueeze(1)
    cand_state.copy_(new_state)
    cand_psi.copy_(torch.where(a, psi_h, cand_psi))
    cand_lp.copy_(torch.where(a, sc.gather(1, order), cand_lp))
    cand_tok.copy_(torch.where(a, cand_tok.gather(1, order), cand_tok))
    cand_slot.copy_(torch.where(a, order.to(torch.int32), cand_slot))


def _prefix_commit_composed(cand_state, cand_psi, cand_tok, cand_slot, next_tok, reorder, finished, plen, in_len, state_out, psi_out,
                            last_out, len_out, result, *, G):
    R, K = cand_tok.shape
    S, dev = state_out.size(1), cand_tok.device
    rows = torch.arange(R, device=dev)
    act = _score_rows(R, G, finished, False, dev)
    par = reorder.to(torch.int64)
    ok = (par >= 0) & (par < R) & (torch.div(par.clamp(0, R - 1), G, rounding_mode="floor") == torch.div(rows, G, rounding_mode="floor"))
    par = torch.where(ok, par, rows)
    hit = cand_tok[par].to(torch.int64) == next_tok.unsqueeze(1)
    q = hit.to(torch.int32).argmax(1)                                              # the first match
    slot = cand_slot[par, q].to(torch.int64)
    ok = ok & hit.any(1) & (slot >= 0) & (slot < K)
    slot = slot.clamp(0, K - 1)
    result[:1] += (act & ~ok).sum().to(torch.int32)
    good = act & ok
    T = in_len[par].clamp(0, S)
    take = good.unsqueeze(1) & (torch.arange(S, device=dev).unsqueeze(0) < T.unsqueeze(1))
    state_out.copy_(torch.where(take.unsqueeze(-1), cand_state[par, :, slot], state_out))
    psi_out.copy_(torch.where(good, cand_psi[par, slot], psi_out))
    last_out.copy_(torch.where(good, next_tok, last_out))
    len_out.copy_(torch.where(good, plen[par].clamp(min=0) + 1, len_out))


class CTCPrefixScorer:
    """The CTC side of joint CTC / attention beam search (DESIGN.md "Beam search", "CTC prefix scores inside the beam") over one
    batch: enc_btd [Bs, S, D] encoder rows (any batch stride), enc_len [Bs] valid rows, head_w [V, D] the CTC head (same dictionary as
    the decoder), `beam` rows per sentence, `weight` the lambda of the combined score.

    The blank's column is gathered once; per beam step rescore(step, bs) gathers the log-probabilities of the K = 2 beam candidates
    simulst_beam_topk left in bs.cand_tok (Ops.linear_gather over the list viewed as [Bs, beam * K]: no copy, no logits), runs the
    scoring launch and leaves bs.cand_lp / bs.cand_tok combined and in candidate order for simulst_beam_select; commit(step, bs),
    behind the selection, moves each new row's state into the second of the two state sets, which then swap.  A committed token that
    was not among its parent's candidates is counted in bs.result[3], which BeamSearch.run asserts to be 0.

    composed=True (and CPU tensors) runs the torch form of both steps; on CPU tensors the gather is a log_softmax of the full
    product.  log_probs [Bs, S, V] fp32 may stand in for (head_w, enc_btd): the gathers then read it (tests, scripted models)."""

    def __init__(self, ops, head_w, enc_btd, enc_len, *, beam: int, weight: float, blank: int = 0, pad: int, eos: int,
                 head_b: Optional[torch.Tensor] = None, composed: bool = False, log_probs: Optional[torch.Tensor] = None):
        if not 0.0 <= float(weight) <= 1.0:
            raise ValueError(f"ctc_weight must be in [0, 1], got {weight}")
        if not 1 <= 2 * beam <= SCORE_KMAX:
            raise ValueError(f"beam must be in [1, {SCORE_KMAX // 2}], got {beam}")
        src = log_probs if log_probs is not None else enc_btd
        self.ops, self.w, self.b, self.enc, self.lp = ops, head_w, head_b, enc_btd, log_probs
        self.G, self.K, self.weight, self.blank, self.pad, self.eos = beam, 2 * beam, float(weight), int(blank), int(pad), int(eos)
        self.Bs, self.S = Bs, S = src.size(0), src.size(1)
        self.dev = dev = src.device
        self.composed = bool(composed) or not src.is_cuda
        R, G, K = Bs * beam, beam, 2 * beam
        self.R = R
        f32, i64 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int64)
        self.xb = self.gather(torch.full((Bs, 1), self.blank, device=dev, dtype=torch.int32))[:, :, 0].contiguous()      # [Bs, S]
        il = torch.as_tensor(enc_len, device=dev).to(torch.int64).clamp(0, S)
        self.in_len = il.repeat_interleave(G).contiguous()
        # the empty prefix: gn = -inf, gb[t] = the blanks' running sum, psi = 0 (rows past a length are never read)
        inside = torch.arange(S, device=dev).unsqueeze(0) < il.unsqueeze(1)
        gb = torch.where(inside, self.xb, torch.zeros((), **f32)).cumsum(1)
        st = torch.stack([torch.full_like(gb, float("-inf")), gb], dim=-1).repeat_interleave(G, 0).contiguous()           # [R, S, 2]
        self.state = [st, torch.zeros_like(st)]
        self.psi = [torch.zeros(R, **f32), torch.zeros(R, **f32)]
        self.last = [torch.full((R,), -1, **i64), torch.full((R,), -1, **i64)]
        self.plen = [torch.zeros(R, **i64), torch.zeros(R, **i64)]
        self.cur = 0
        self.xc = torch.empty(Bs, S, G * K, **f32)
        self.cand_state = torch.empty(R, S, K, 2, **f32)
        self.cand_psi = torch.empty(R, K, **f32)
        self.cand_slot = torch.zeros(R, K, device=dev, dtype=torch.int32)

    def gather(self, labels: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """labels int32 [Bs, n] -> fp32 [Bs, S, n]: the head's log-probabilities at the labels (values outside the vocabulary are
        clamped into it, as Ops.linear_gather does)"""
        if self.lp is None and self.enc.is_cuda:
            return self.ops.linear_gather(self.enc, self.w, self.b, labels, out=out)
        if self.lp is None:
            z = self.enc.float() @ self.w.float().t()
            self.lp = torch.log_softmax(z if self.b is None else z + self.b.float(), dim=-1)
        idx = labels.to(torch.int64).clamp(0, self.lp.size(2) - 1).unsqueeze(1).expand(-1, self.lp.size(1), -1)
        g = self.lp.float().gather(2, idx)
        return g if out is None else out.copy_(g)

    def rescore(self, step: int, bs):
        """between simulst_beam_topk and simulst_beam_select of step `step` of the BeamSearch bs"""
        c = self.cur
        self.gather(bs.cand_tok.view(self.Bs, self.G * self.K), out=self.xc)
        ctc_prefix_score(self.ops, self.xc, self.xb, self.state[c], self.psi[c], self.last[c], self.plen[c], self.in_len, bs.finished,
                         bs.cand_lp, bs.cand_tok, self.cand_slot, self.cand_state, self.cand_psi, G=self.G, blank=self.blank,
                         eos=self.eos, pad=self.pad, weight=self.weight, first_only=step == 0, composed=self.composed)

    def commit(self, step: int, bs):
        """behind simulst_beam_select of step `step`: bs.next_tok / bs.reorder name each new row's candidate"""
        c = self.cur
        ctc_prefix_commit(self.ops, self.cand_state, self.cand_psi, bs.cand_tok, self.cand_slot, bs.next_tok, bs.reorder, bs.finished,
                          self.last[c], self.plen[c], self.in_len, self.state[1 - c], self.psi[1 - c], self.last[1 - c],
                          self.plen[1 - c], bs.result[3:4], G=self.G, composed=self.composed)
        self.cur = 1 - c


class CTCTranscriber:
    """transcribe_ctc for the models whose encoder can carry the head (SimulSTModel and its registered subclasses, CIFTransformerModel)."""

    def score_ctc(self, src_tokens, src_lengths, targets, *, blank: int = 0) -> List[dict]:
        """Encoder forward + the head's CTC score of given transcripts: targets is a list of token lists (or a [B, L] tensor padded with
        the model's padding index).  One {"nll" (float: the CTC negative log-likelihood, inf where the transcript does not fit),
        "score" (-nll / max(n, 1), n the transcript's length)} per utterance.  Raises ValueError when the model has no CTC head."""
        enc = self.encoder.forward(src_tokens, src_lengths)
        pad = self.encoder.cfg.padding_idx
        if torch.is_tensor(targets):
            tgt = targets.to(torch.int64)
            n = tgt.ne(pad).sum(1)
        else:
            n = torch.tensor([len(t) for t in targets], dtype=torch.int64)
            tgt = torch.full((len(targets), int(n.max()) if len(targets) else 0), pad, dtype=torch.int64)
            for b, t in enumerate(targets):
                tgt[b, :len(t)] = torch.as_tensor(t, dtype=torch.int64)
        s = self.encoder.ctc_score(enc["encoder_out_btd"], enc["encoder_lengths"], tgt, n, blank=blank)
        nll, n = s["nll"].cpu(), n.cpu()
        return [{"nll": float(nll[b]), "score": -float(nll[b]) / max(int(n[b]), 1)} for b in range(nll.numel())]

    def ctc_error_report(self, enc, targets, target_lengths, *, blank: int = 0) -> Dict[str, torch.Tensor]:
        """Token errors of the head's greedy transcript over an encoder output (the dict encoder.forward returns) against targets
        [B, T] / target_lengths [B]: ctc_greedy + ctc_collapse + token_error_report, sums on the device."""
        g = self.encoder.ctc_greedy(enc["encoder_out_btd"], enc["encoder_lengths"], blank=blank)
        return token_error_report(g["tokens"], g["n"], targets, target_lengths, ops=self.encoder.ops)

    def transcribe_ctc_nbest(self, src_tokens, src_lengths, *, beam: int = 8, nbest: int = 1, candidates: int = 8, blank: int = 0,
                             rescore: bool = True) -> List[List[dict]]:
        """Encoder forward + prefix beam search over the head.  Per utterance a list of up to nbest hypotheses {"tokens" (list),
        "beam_score" (the search's log(p_b + p_nb): the likelihood mass of the alignments it kept)}, best first.  With rescore every
        hypothesis gets "nll", its exact CTC negative log-likelihood (ctc_rescore: one gather per utterance for all its hypotheses),
        the list is sorted by nll, and its first hypothesis gets "frames" / "frames_ms": the encoder row at which each token's run
        starts on its best alignment (ctc_score(align=True)).  Raises ValueError when the model has no CTC head."""
        enc = self.encoder.forward(src_tokens, src_lengths)
        rows, lens = enc["encoder_out_btd"], enc["encoder_lengths"]
        pad = self.encoder.cfg.padding_idx
        r = self.encoder.ctc_prefix_beam_search(rows, lens, beam=beam, candidates=candidates, nbest=nbest, blank=blank, pad=pad)
        tokens, n, score = r["tokens"].cpu(), r["n"].cpu(), r["score"].cpu()
        hyps = []
        for b in range(tokens.size(0)):
            keep = [j for j in range(tokens.size(1)) if float(score[b, j]) > float("-inf")] or [0]
            hyps.append([(tokens[b, j, :int(n[b, j])].tolist(), float(score[b, j])) for j in keep])
        if not rescore:
            return [[{"tokens": t, "beam_score": s} for t, s in h] for h in hyps]
        ranked = ctc_rescore(self.encoder.ops, self.encoder.w.ctc, rows, lens, hyps, weight=1.0, blank=blank)
        out = [[{"tokens": x["tokens"], "beam_score": x["score"], "nll": x["nll"]} for x in h] for h in ranked]
        B = len(out)
        Lb = max((len(h[0]["tokens"]) for h in out), default=0)
        for h in out:
            h[0]["frames"], h[0]["frames_ms"] = [], []
        if B and Lb:
            tgt = torch.full((B, max(Lb, 1)), pad, dtype=torch.int64)
            for b, h in enumerate(out):
                tgt[b, :len(h[0]["tokens"])] = torch.as_tensor(h[0]["tokens"], dtype=torch.int64)
            tl = torch.tensor([len(h[0]["tokens"]) for h in out], dtype=torch.int64)
            al = self.encoder.ctc_score(rows, lens, tgt, tl, blank=blank, align=True)["alignment"]
            _, _, frames = ctc_collapse(al, lens, blank, pad)
            frames = frames.cpu()
            step_ms = self.encoder.conv_layer_stride() * SHIFT_MS
            for b, h in enumerate(out):
                fr = frames[b, :len(h[0]["tokens"])].tolist()
                h[0]["frames"], h[0]["frames_ms"] = fr, [f * step_ms for f in fr]
        return out

    def transcribe_ctc(self, src_tokens, src_lengths, *, blank: int = 0) -> List[dict]:
        """Encoder forward + the head's greedy path.  One {"tokens" (list), "score" (float: sum of the picked labels' log-probabilities
        over the utterance's rows), "frames" (encoder row at which each token's run starts), "frames_ms" (frame x encoder stride x 10 ms)}
        per utterance.  Raises ValueError when the model has no CTC head."""
        enc = self.encoder.forward(src_tokens, src_lengths)
        g = self.encoder.ctc_greedy(enc["encoder_out_btd"], enc["encoder_lengths"], blank=blank)
        tokens, n, frames, score = g["tokens"].cpu(), g["n"].cpu(), g["frames"].cpu(), g["score"].cpu()
        step_ms = self.encoder.conv_layer_stride() * SHIFT_MS
        out = []
        for b in range(tokens.size(0)):
            k = int(n[b])
            fr = frames[b, :k].tolist()
            out.append({"tokens": tokens[b, :k].tolist(), "score": float(score[b]), "frames": fr, "frames_ms": [f * step_ms for f in fr]})
        return out
