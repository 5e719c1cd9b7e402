"""What a user does with the encoder's CTC head: read its best path.

``ctc_greedy`` takes the head's per-row pick straight out of the projection (Ops.linear_pick: simulst_linear with
SIMULST_EPI_ROW_PICK -- the [B, Te, V] logits never reach memory), ``ctc_collapse`` turns a path into a transcript with a frame stamp per
token, ``ctc_report`` is the accuracy report of the reference's JointCTCCriterion (criterion/joint_ctc_criterion.py:24-48, 92-101) and
``CTCTranscriber.transcribe_ctc`` the model-level call: encoder forward + greedy path.  CTC loss values (the sum over alignments), prefix
beam search and rescoring are not here.

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


class CTCTranscriber:
    """transcribe_ctc for the models whose encoder can carry the head (SimulSTModel and its registered subclasses, CIFTransformerModel)."""

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
