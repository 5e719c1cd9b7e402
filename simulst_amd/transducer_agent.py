"""Simultaneous decoding of the transducer_model: the joiner decides "emit at pooled position s" from P[s] and the prediction
network's g alone, so a row can be decoded while its source still grows -- READ while none of the positions released so far emits,
WRITE otherwise (the case the reference's TransducerDecoder.rollback, models/transducer_model.py:214-239, was written for; here
nothing is rolled back, TransducerDecoder.step_online commits per row).

The invariant of every form below: WHAT IS WRITTEN SIMULTANEOUSLY IS WHAT ``generate_offline`` WRITES UP TO EOS (or the agent's
length cap) OVER THE SAME ENCODER STATES; ONLY THE DELAYS ARE NEW.  A token emitted at pooled position e is written as soon as the
encoder has released the rows of window e; the last position, where the offline decode forces the emission, exists only once the
source has ended.

* ``TransducerAgent.run_utterance``                 one stream, chunk sizes and ``finish`` rule of FairseqSimulSTAgent
* ``BatchedTransducerStreamingAgent.run_batch``    B streams in lockstep (microphones), or self-paced (evaluation from files): one
                                                    offline greedy decode, every token's delay from its emit position (``emit_delays``)

These are classes of their own: ``refuse_offline_model`` keeps sending the callers of the attention-policy agents
(FairseqSimulSTAgent, BatchedStreamingAgent, the SimulEval agent) back to ``generate_offline``.
"""
from bisect import bisect_left
from typing import List, Sequence

import torch

from .stream_source import ChunkedAgent, FrameSource, encoder_chunks, offline_states, source_ms


def emit_delays(emit: Sequence[int], n_tokens: int, enc_len: int, k: int, schedule: Sequence[int]) -> List[int]:
    """The chunk at which each of the first n_tokens tokens of a hypothesis is written: emit[i] is the pooled position token i was
    emitted at, enc_len the row's encoder rows, k the pooling window, schedule[c] the encoder rows released after chunk c
    (cumulative, schedule[-1] == enc_len: the last chunk carries ``finish``).  Position e is available once the encoder has
    released min((e + 1) k, enc_len) rows -- its whole window --, and the true last position ceil(enc_len / k) - 1, where the offline
    decode forces the emission, only at the final chunk (until then the row cannot know that nothing follows).  This equals what
    the lockstep form does as long as the final chunk releases at least one encoder row, which ``stream_row_schedule`` gives
    whenever the encoder has a right context (its look-ahead rows are held back until ``finish``); were all of enc_len = S' k rows out before the final chunk,
    a lockstep row could write a token that truly emits at the last position one chunk earlier than stated here.  Pure host
    arithmetic;the delay in ms and the READ / WRITE string follow from the chunk index (``records_from_chunks``)."""
    if n_tokens == 0:
        return []
    assert len(schedule) > 0 and schedule[-1] == enc_len and k >= 1
    last_pos = (enc_len + k - 1) // k - 1
    out = []
    for e in emit[:n_tokens]:
        e = int(e)
        if e >= last_pos:
            c = len(schedule) - 1
        else:
            c = bisect_left(schedule, min((e + 1) * k, enc_len))
        out.append(max(c, out[-1]) if out else c)
    return out


def records_from_chunks(tokens, emit, chunks, positions, max_len, eos, total_ms, n_enc_of):
    """One record from a row's offline hypothesis and the chunk of every token: the row writes until EOS or until it holds more
    tokens than max_len(frames read so far) allows (the cap rule of FairseqSimulSTAgent.run_utterance), then stops reading."""
    from .latency import average_lagging
    toks, delays, emits, tc = [], [], [], []
    for t, e, c in zip(tokens, emit, chunks):
        toks.append(int(t)), emits.append(int(e)), tc.append(c)
        delays.append(source_ms(positions[c]))
        if int(t) == eos or len(toks) > max_len(positions[c]):
            break
    n_read = tc[-1] + 1 if tc else len(positions)
    actions = "".join("R" + "W" * tc.count(c) for c in range(n_read))
    return {"tokens": toks, "delays_ms": delays, "actions": actions, "AL": average_lagging(delays, total_ms),
            "n_enc": n_enc_of(n_read - 1), "emit": emits}


class TransducerAgent(ChunkedAgent):
    """One simultaneous stream (B = 1) over TransducerModel: READ while the row waits and the source has not ended, otherwise
    WRITE.  Tokens are picked as greedy_offline picks them (pad masked, EOS masked at the first step); the hypothesis ends at EOS
    or when it outgrows max_len(frames read), FairseqSimulSTAgent's rule.  What is written is what generate_offline writes up to
    there; only the delays are new."""

    def __init__(self, model, max_len_a: float = 1, max_len_b: int = 0):
        if getattr(model.cfg, "model", None) != "transducer_model":
            raise ValueError(f"{type(self).__name__} decodes transducer_model, not {getattr(model.cfg, 'model', None)!r}")
        self.model = model
        self._init_chunks(model)
        self.max_len = lambda x: min(max_len_a * x + max_len_b, model.max_decoder_positions())

    def _new_state(self, B: int, T: int):
        dec, k = self.model.decoder, self.model.cfg.downsample
        st = dec.new_state(B, cap=max(int(self.max_len(T)) + 4, 8))
        dec.open_source(st, S_cap=(T // self.model.encoder.stride) // k + 2)
        return st

    def _pick(self, logits, first: bool):
        cfg = self.model.cfg
        return self.model.ops.greedy_argmax(logits, pad_idx=cfg.padding_idx, eos_idx=cfg.eos, mask_eos=first)

    def run_utterance(self, fbank: torch.Tensor):
        """fbank [T, 80] -> {"tokens", "delays_ms", "actions", "AL", "n_enc", "emit": the pooled position of every token}"""
        from .latency import average_lagging
        model, dec, dev = self.model, self.model.decoder, self.model.device
        src = FrameSource(fbank)
        enc_state, st = {}, None
        expected = self.first_frames
        tokens, delays, emits, actions = [], [], [], []
        toks = torch.full((1,), self.eos, device=dev, dtype=torch.int64)
        while True:
            wrote = False
            if st is not None:
                logits, _ = dec.step_online(st, toks)
                wrote = st.n_wrote > 0
            if not wrote:                                                  # READ: the row waits (or has no encoder state yet)
                if src.finished:
                    if st is None or st.avail_host[0] == 0:                # the source ended before a single pooled position
                        break                                              # ... existed: the hypothesis ends empty
                    raise RuntimeError("READ after source finished")
                actions.append("R")
                finish = src.take(expected)                                # agents/default_agent.py:303-342
                new = model.encoder.infer(fbank[:src.pos].unsqueeze(0), torch.tensor([src.pos]), enc_state, finish=finish)["encoder_out_btd"]
                if st is None:
                    st = self._new_state(1, fbank.size(0))
                dec.append_source(st, new, new.size(1), finish)
                expected = self.next_frames
                continue
            actions.append("W")
            toks = self._pick(logits, first=not tokens)
            tok = int(toks.item())
            tokens.append(tok), delays.append(src.elapsed_ms()), emits.append(int(st.prev_emit.item()))
            if tok == self.eos or len(tokens) > self.max_len(src.pos):
                break
        return {"tokens": tokens, "delays_ms": delays, "actions": "".join(actions), "AL": average_lagging(delays, src.total_ms()),
                "n_enc": st.enc_rows if st is not None else 0, "emit": emits}


class BatchedTransducerStreamingAgent(TransducerAgent):
    """B simultaneous transducer streams in one batch.  Every row's record is that of TransducerAgent.run_utterance on its
    utterance alone: a row's decisions depend only on its own prefix and on the source released to it, and what it writes is what
    generate_offline writes up to EOS; only the delays are new."""

    def run_batch(self, fbank: torch.Tensor, self_paced: bool = False, encoder: str = "chunked", lengths=None):
        """fbank [B, T, 80] -> one record per row, the keys of run_utterance.

        self_paced=False, the microphone form: the sources advance in lockstep (equal lengths); per chunk one encoder.infer and one
        append_source, then rounds of step_online over the rows until every row waits or has ended.
        self_paced=True, the evaluation form: the whole source is encoded first, ONE greedy_offline decodes it, and every token's
        delay follows from its emit position and the encoder's release schedule (``emit_delays``) -- no decode work is repeated
        per chunk.
        encoder="offline": the encoder states come from one offline forward, released by ``stream_row_schedule``; with
        self_paced=True the sources may then have different lengths (``lengths`` [B] frame counts, fbank padded)."""
        if encoder not in ("chunked", "offline"):
            raise ValueError(f"encoder={encoder!r}: 'chunked' or 'offline'")
        B, T = fbank.size(0), fbank.size(1)
        Ls = [T] * B if lengths is None else [int(x) for x in lengths]
        if len(Ls) != B or min(Ls) <= 0 or max(Ls) > T:
            raise ValueError("lengths: one positive frame count per row, at most fbank.size(1)")
        if len(set(Ls)) > 1 and not (self_paced and encoder == "offline"):
            raise ValueError("sources of different lengths need self_paced=True, encoder='offline'")
        if self_paced:
            return self._run_batch_self_paced(fbank, encoder, Ls)
        return self._run_batch_lockstep(fbank[:, :Ls[0]], encoder)

    def _run_batch_lockstep(self, fbank: torch.Tensor, encoder: str):
        from .latency import average_lagging
        model, dec, enc, dev = self.model, self.model.decoder, self.model.encoder, self.model.device
        B, T = fbank.size(0), fbank.size(1)
        fbank = fbank.to(dev)
        sched = self._schedule(T)
        schedule = sched.rows
        chunks = encoder_chunks(enc, fbank, sched, encoder)
        st = self._new_state(B, T)
        toks = torch.full((B,), self.eos, device=dev, dtype=torch.int64)
        tokens, delays, emits, actions = ([[] for _ in range(B)] for _ in range(4))
        done = [False] * B
        for c, pos, finish, new in chunks:
            for b in range(B):
                if not done[b]:
                    actions[b].append("R")
            dec.append_source(st, new, new.size(1), finish)
            ms, cap = sched.ms[c], self.max_len(pos)
            while True:                                                    # rounds until every row waits or has ended
                logits, wrote = dec.step_online(st, toks)
                if st.n_wrote:                                             # some row wrote
                    first = [not tokens[b] for b in range(B)]
                    pick = self._pick(logits, first=False)
                    if any(first):
                        pick = torch.where(torch.tensor(first, device=dev), self._pick(logits, first=True), pick)
                    toks = torch.where(wrote, pick, toks)
                    w_h, p_h, e_h = torch.stack([wrote.to(torch.int64), pick, st.prev_emit.to(torch.int64)]).tolist()
                    ended = False
                    for b in range(B):
                        if w_h[b]:
                            tokens[b].append(p_h[b]), delays[b].append(ms), emits[b].append(e_h[b]), actions[b].append("W")
                            if p_h[b] == self.eos or len(tokens[b]) > cap:
                                done[b] = ended = True
                    if ended:
                        st.done.copy_(torch.tensor(done, dtype=torch.int32))
                        dec.sync_source(st)
                    continue
                break
            if all(done) or (finish and any(a == 0 for a in st.avail_host)):
                break                                  # every row has ended, or no pooled position at all: the hypotheses end empty
        if not all(done) and all(a > 0 for a in st.avail_host):
            raise RuntimeError("rows still waiting after the source finished")
        return [{"tokens": tokens[b], "delays_ms": delays[b], "actions": "".join(actions[b]),
                 "AL": average_lagging(delays[b], sched.total_ms), "n_enc": schedule[len(actions[b]) - len(tokens[b]) - 1], "emit": emits[b]}
                for b in range(B)]

    def _run_batch_self_paced(self, fbank: torch.Tensor, encoder: str, Ls):
        model, dec, enc, dev = self.model, self.model.decoder, self.model.encoder, self.model.device
        k = model.cfg.downsample
        B, T = fbank.size(0), fbank.size(1)
        fbank = fbank.to(dev)
        per_T = {t: self._schedule(t) for t in set(Ls)}
        if encoder == "offline":
            states, _ = offline_states(enc, fbank, Ls, [per_T[t] for t in Ls])
        else:
            states = torch.cat([new for _, _, _, new in encoder_chunks(enc, fbank, per_T[T])], 1)
        enc_len = [per_T[t].rows[-1] for t in Ls]
        empty = [n == 0 for n in enc_len]
        # every row is its own utterance: pooled over whole windows (the buffer padded to a multiple of k), a row's partial last
        # window is the mean of its valid rows, as append_source flushes it
        rows = max((max(enc_len) + k - 1) // k * k, k)
        buf = torch.zeros(B, rows, states.size(2), device=dev, dtype=states.dtype)
        buf[:, :min(rows, states.size(1))] = states[:, :rows]
        n_steps = max(int(self.max_len(t)) for t in Ls) + 1
        hyp, emit, _ = dec.greedy_offline(buf, torch.tensor([max(n, 1) for n in enc_len]), n_steps, T=rows, until_all_eos=True)
        hyp, emit = hyp.tolist(), emit.tolist()
        recs = []
        for b, t in enumerate(Ls):
            s = per_T[t]
            n = 0 if empty[b] else len(hyp[b])
            chunks = emit_delays(emit[b], n, enc_len[b], k, s.rows)
            recs.append(records_from_chunks(hyp[b][:n], emit[b][:n], chunks, s.positions, self.max_len, self.eos, s.total_ms,
                                            lambda c, s=s: s.rows[c]))
        return recs
