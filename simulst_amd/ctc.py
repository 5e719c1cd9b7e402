"""What a user does with the encoder's CTC head: read its best path, and score a given transcript.

``ctc_greedy`` takes the head's per-row pick straight out of the projection (Ops.linear_pick: simulst_linear with
SIMULST_EPI_ROW_PICK -- the [B, Te, V] logits never reach memory), ``ctc_collapse`` turns a path into a transcript with a frame stamp per
token, ``ctc_report`` is the accuracy report of the reference's JointCTCCriterion (criterion/joint_ctc_criterion.py:24-48, 92-101) and
``CTCTranscriber.transcribe_ctc`` the model-level call: encoder forward + greedy path.

``ctc_score`` is the CTC loss value of given transcripts (the sum over alignments, F.ctc_loss of criterion/joint_ctc_criterion.py:78-90
and the CTC term of criterion/cif_criterion.py), optionally with the forced alignment: the projection writes only the log-probabilities
of the blank and of the transcript's own labels, [B, Te, L + 1] (Ops.linear_gather: SIMULST_EPI_ROW_GATHER), and the recursion of
ctc_align.ctc_nll runs over them.  ``ctc_rescore`` re-ranks n-best lists with that score, one gather per utterance for all its
hypotheses, and ``CTCTranscriber.score_ctc`` is the model-level call.  Prefix beam search is not here, and no gradient is computed.

The blank index is a keyword everywhere (default 0, the criterion's fallback, joint_ctc_criterion.py:76).
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
