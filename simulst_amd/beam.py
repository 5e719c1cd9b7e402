"""Beam search for offline decoding: fairseq's SequenceGenerator with search.BeamSearch (eval/generate.py --beam N --lenpen X
--nbest M) at the defaults the reference runs -- normalize_scores, min_len 1, no unk penalty, temperature 1, no prefix tokens,
constraints or n-gram blocking.  DESIGN.md section "Beam search" lists the semantics.

BeamSearch owns the device buffers of one batch of Bs sentences x beam rows and runs the step loop over any source of logits: the
decoder (MMADecoder.beam_offline) or a scripted model in a test.  Per step, on the handle's stream: the logits source,
simulst_beam_topk, the caller's rescore if there is one (joint CTC / attention decoding: ctc.CTCPrefixScorer.rescore rewrites the
candidate lists with the combined scores), simulst_beam_select, then the caller's after_select (the decoder commits the step and
reorders its incremental state, simulst_beam_reorder); once at the end simulst_beam_backtrack.  Every `chunk` steps the count of unfinished sentences is read
back on the handle's stream, and the loop ends when it is zero.

ReorderBuffers is the double buffer that reorder works on, for the MMA decoder's state and the transducer's alike.
"""
from typing import Callable, List, Optional, Sequence

import torch

from . import _lib
from .decoder import regrow

MAX_BEAM = 16


def check_args(beam: int, nbest: int, V: int):
    if not 1 <= beam <= MAX_BEAM:
        raise ValueError(f"beam must be in [1, {MAX_BEAM}], got {beam}")
    if not 1 <= nbest <= beam:
        raise ValueError(f"nbest must be in [1, beam = {beam}], got {nbest}")
    if 2 * beam > V - 1:
        raise ValueError(f"2 beam must be at most V - 1 = {V - 1}, got beam {beam}")


def sentence_caps(max_len, Bs: int) -> List[int]:
    """max_len of a beam_offline call, an int or one cap per sentence, as one cap per sentence"""
    caps = [int(max_len)] * Bs if isinstance(max_len, int) else [int(x) for x in max_len]
    assert len(caps) == Bs, "one cap per sentence"
    return caps


class ReorderBuffers:
    """The double buffer of the beam-state reorder (simulst_beam_reorder, simulst_transducer_beam_reorder) of one decoder state `st`:
    the second set of its self-attention caches st.k_cache / st.v_cache ([R, H, cap, d] per layer) and of the attributes `extra`
    names (a tensor per row set, or one per layer: head_step for the MMA decoder, prev_emit for the transducer), the two
    _lib.DecLayer arrays (src: the set the state holds, dst: the second one, self.other[name]) and the descriptor the entry points
    read.  It lives on the state (st.reorder_buf), so the addresses last as long as the state does."""

    def __init__(self, st, extra: Sequence[str] = ()):
        self.st, self.names = st, ("k_cache", "v_cache") + tuple(extra)

        def second(v):
            return [torch.zeros_like(t) for t in v] if isinstance(v, list) else torch.zeros_like(v)
        self.other = {n: second(getattr(st, n)) for n in self.names}
        R, H, cap, d = st.k_cache[0].shape
        self.desc = desc = _lib.DecoderDesc()
        desc.B, desc.D, desc.H, desc.n_layers, desc.cap = R, H * d, H, len(st.k_cache), cap
        desc.dtype = _lib.F32 if st.k_cache[0].dtype == torch.float32 else _lib.BF16
        self._point()

    @classmethod
    def of(cls, st, extra: Sequence[str] = ()):
        """the state's own, made on first use"""
        if getattr(st, "reorder_buf", None) is None:
            st.reorder_buf = cls(st, extra)
        return st.reorder_buf

    def _point(self):
        def layers(get):
            arr = (_lib.DecLayer * self.desc.n_layers)()
            for n in self.names:
                if isinstance(get(n), list):                    # per layer: the _lib.DecLayer field of that name
                    for l, t in enumerate(get(n)):
                        setattr(arr[l], n, t.data_ptr())
            return arr
        self.src, self.dst = layers(lambda n: getattr(self.st, n)), layers(self.other.__getitem__)

    def swap(self):
        """behind a reorder: the set it wrote becomes the state's"""
        for n in self.names:
            cur = getattr(self.st, n)
            setattr(self.st, n, self.other[n])
            self.other[n] = cur
        self.src, self.dst = self.dst, self.src

    def grow(self, cap: int):
        """the caches of both sets to `cap` positions, contents kept"""
        for n in ("k_cache", "v_cache"):
            setattr(self.st, n, regrow(getattr(self.st, n), cap))
            self.other[n] = regrow(self.other[n], cap)
        self.desc.cap = cap
        self._point()


class BeamSearch:
    """Buffers and kernels of one beam search over Bs sentences of `beam` rows each (row r = s * beam + j).  max_len[s] is the
    sentence's cap: steps 0 .. max_len[s] run, so a hypothesis holds at most max_len[s] tokens and EOS."""

    def __init__(self, ops, max_len: Sequence[int], *, beam: int, V: int, eos: int, pad: int, lenpen: float = 1.0, nbest: int = 1,
                 device="cuda"):
        check_args(beam, nbest, V)
        self.ops, self.beam, self.V, self.eos, self.pad, self.lenpen, self.nbest = ops, beam, V, eos, pad, float(lenpen), nbest
        caps = [int(x) for x in max_len]
        assert len(caps) >= 1 and min(caps) >= 0, "one cap >= 0 per sentence"
        self.caps = caps
        self.Bs = Bs = len(caps)
        self.R = R = Bs * beam
        self.L = L = max(caps) + 1                              # rows of the back-pointer tables: steps 0 .. max(max_len)
        K = 2 * beam
        i32, f32 = dict(device=device, dtype=torch.int32), dict(device=device, dtype=torch.float32)
        self.max_len = torch.tensor(caps, dtype=torch.int32).to(device)
        self.cand_lp = torch.empty(R, K, **f32)
        self.cand_tok = torch.empty(R, K, **i32)
        self.cum = torch.zeros(R, **f32)
        self.next_tok = torch.full((R,), eos, device=device, dtype=torch.int64)
        self.reorder = torch.arange(R, **i32)
        self.bp_parent = torch.zeros(L, R, **i32)
        self.bp_token = torch.zeros(L, R, **i32)
        self.bp_cum = torch.zeros(L, R, **f32)
        self.fin_step = torch.zeros(Bs, beam, **i32)
        self.fin_row = torch.zeros(Bs, beam, **i32)
        self.fin_score = torch.zeros(Bs, beam, **f32)
        self.fin_raw = torch.zeros(Bs, beam, **f32)
        self.fin_count = torch.zeros(Bs, **i32)
        self.finished = torch.zeros(Bs, **i32)
        # [0] unfinished sentences after the last step, [1] select: sentences short of beam next rows, [2] reorders out of a block,
        # [3] a rescorer's commits of a token that was not among its parent's candidates
        self.result = torch.zeros(4, **i32)
        self.host = torch.zeros(4, dtype=torch.int32, pin_memory=True)
        self.event = torch.cuda.Event()
        self.device = torch.device(device)
        self.steps = 0

    def _read_result(self):
        """the result words, read on the handle's stream alone (as MMADecoder.generate_offline reads its counts)"""
        sp = getattr(self.ops.h, "stream_ptr", None)
        stream = torch.cuda.ExternalStream(sp, device=self.device) if sp else torch.cuda.default_stream(self.device)
        with torch.cuda.stream(stream):
            self.host.copy_(self.result, non_blocking=True)
            self.event.record(stream)
        self.event.synchronize()
        return [int(x) for x in self.host]

    def run(self, logits_fn: Callable[[int, torch.Tensor], torch.Tensor], after_select: Optional[Callable[[int], None]] = None,
            chunk: int = 8, rescore: Optional[Callable[[int], None]] = None):
        """logits_fn(step, tokens [R] int64) -> fp32 logits [R, V] of the step; after_select(step) runs behind the selection (the
        reorder index of the step is in self.reorder); rescore(step), if given, runs between simulst_beam_topk and the selection and
        may rewrite self.cand_lp / self.cand_tok (each row's list in candidate order again, and still beam finite candidates a
        sentence: the selection, cum, lenpen, finalisation and the scores returned are then all of the rewritten score).  Returns (tokens [Bs, nbest, L] int64, lengths [Bs, nbest] int32,
        scores [Bs, nbest] fp32, positional scores [Bs, nbest, L] fp32), on the device."""
        ops, beam = self.ops, self.beam
        t = 0
        while t < self.L:
            logits = logits_fn(t, self.next_tok)
            assert logits.dtype == torch.float32 and tuple(logits.shape) == (self.R, self.V), "fp32 logits [R, V]"
            ops.beam_topk(logits, self.max_len, self.finished, self.cand_lp, self.cand_tok, beam=beam, step=t, pad_idx=self.pad,
                          eos_idx=self.eos)
            if rescore is not None:
                rescore(t)
            ops.beam_select(self.cand_lp, self.cand_tok, self.max_len, beam=beam, V=self.V, step=t, lenpen=self.lenpen,
                            eos_idx=self.eos, cum=self.cum, next_tok=self.next_tok, reorder=self.reorder, bp_parent=self.bp_parent,
                            bp_token=self.bp_token, bp_cum=self.bp_cum, fin_step=self.fin_step, fin_row=self.fin_row,
                            fin_score=self.fin_score, fin_raw=self.fin_raw, fin_count=self.fin_count, finished=self.finished,
                            result=self.result)
            if after_select is not None:
                after_select(t)
            t += 1
            if t % chunk == 0 and t < self.L and self._read_result()[0] == 0:
                break
        self.steps = t
        res = self._read_result()
        assert res[0] == 0, f"{res[0]} sentences unfinished after {t} steps"
        assert res[1] == 0, "a sentence ran short of beam finite non-EOS candidates (fairseq's cands_to_ignore case)"
        assert res[2] == 0, "a reorder left its sentence's block of beam rows"
        assert res[3] == 0, "a rescorer committed a token that was not among its parent's candidates"
        Bs, nb, L, dev = self.Bs, self.nbest, self.L, self.device
        tokens = torch.empty(Bs, nb, L, device=dev, dtype=torch.int64)
        lengths = torch.empty(Bs, nb, device=dev, dtype=torch.int32)
        scores = torch.empty(Bs, nb, device=dev, dtype=torch.float32)
        pos = torch.empty(Bs, nb, L, device=dev, dtype=torch.float32)
        ops.beam_backtrack(beam=beam, nbest=nb, bp_parent=self.bp_parent, bp_token=self.bp_token, bp_cum=self.bp_cum,
                           fin_step=self.fin_step, fin_row=self.fin_row, fin_score=self.fin_score, fin_raw=self.fin_raw,
                           fin_count=self.fin_count, pad_idx=self.pad, eos_idx=self.eos, tokens=tokens, lengths=lengths, scores=scores,
                           pos_scores=pos)
        return tokens, lengths, scores, pos


def hypotheses(tokens, lengths, scores, pos_scores) -> List[List[dict]]:
    """BeamSearch.run's tensors as task.inference_step returns them to eval/generate.py: per sentence a list of
    {"tokens", "score", "positional_scores", "alignment", "attention"}, best first"""
    tokens, lengths, scores, pos_scores = tokens.cpu(), lengths.cpu(), scores.cpu(), pos_scores.cpu()
    out = []
    for s in range(tokens.size(0)):
        hyps = []
        for k in range(tokens.size(1)):
            n = int(lengths[s, k])
            if n == 0:
                continue
            hyps.append({"tokens": tokens[s, k, :n].clone(), "score": scores[s, k].clone(),
                         "positional_scores": pos_scores[s, k, :n].clone(), "alignment": None, "attention": None})
        out.append(hyps)
    return out
