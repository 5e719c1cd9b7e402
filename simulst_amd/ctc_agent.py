"""A streaming transcript at the cost of the encoder alone: the CTC head's best path, read chunk by chunk.

``CTCAgent`` follows FairseqSimulSTAgent's chunk schedule (agents/default_agent.py:367,407: the first READ offers segment + right
context, every later one a segment).  After each READ the chunked encoder (``encoder.infer``) releases new rows, the head's pick is
taken over those rows only (Ops.linear_pick: no logits in memory) and collapsed with the last label carried over from the rows
before, so a run of one label that spans a chunk boundary is written once, at its first row.  Every new token is a WRITE stamped with
the source milliseconds released by that READ; EOS is written when the source ends.

This is the synthetic harness's loop (stream_source.py), not a SimulEval-facing agent.  Any model whose encoder carries the head
streams here, the offline s2t_emformer included: there is no decoder and no read/write policy to ask for.
"""
import torch

from .stream_source import ChunkedAgent, encoder_chunks


class CTCAgent(ChunkedAgent):
    """One stream (B = 1).  Record keys are the other agents': "tokens" (EOS last), "delays_ms", "actions", "AL", plus "frames": the
    encoder row at which each token's run starts (EOS: the number of rows the source gave)."""

    def __init__(self, model, blank: int = 0):
        enc = model.encoder
        if getattr(enc.w, "ctc", None) is None:
            raise ValueError(f"{type(self).__name__}: this model has no CTC head (ModelConfig.ctc_layer is off)")
        self.model, self.blank = model, int(blank)
        self._init_chunks(model)

    def _run(self, fbank: torch.Tensor, return_states: bool):
        """fbank [B, T, 80], rows advancing in lockstep -> (records, rows seen [B, n, D] or None)"""
        from .latency import average_lagging
        model, enc = self.model, self.model.encoder
        B, T = fbank.size(0), fbank.size(1)
        sched = self._schedule(T)
        recs = [{"tokens": [], "delays_ms": [], "frames": [], "actions": []} for _ in range(B)]
        seen, n_rows, now = [], 0, 0
        carry = torch.full((B, 1), -1, device=model.device, dtype=torch.int32)       # no label yet: row 0 never continues a run
        # the Emformer's own rows: what a subclass adds behind them (the CIF layer) is nothing the head reads
        for c, _, _, new in encoder_chunks(enc, fbank, sched):
            for r in recs:
                r["actions"].append("R")
            n, now = new.size(1), sched.ms[c]
            if n == 0:
                continue
            if return_states:
                seen.append(new.clone())
            pick, _, _ = model.ops.linear_pick(new, enc.w.ctc)                         # [B, n] int32, the new rows only
            before = torch.cat([carry, pick[:, :-1]], dim=1)
            keep = (pick != self.blank) & (pick != before)
            b_idx, t_idx = keep.nonzero(as_tuple=True)                                 # row-major: each stream's tokens in row order
            labels = pick[b_idx, t_idx].tolist()
            for b, t, tok in zip(b_idx.tolist(), t_idx.tolist(), labels):
                r = recs[b]
                r["tokens"].append(tok), r["frames"].append(n_rows + t), r["delays_ms"].append(now), r["actions"].append("W")
            carry = pick[:, -1:].clone()
            n_rows += n
        for r in recs:
            r["tokens"].append(self.eos), r["frames"].append(n_rows), r["delays_ms"].append(now), r["actions"].append("W")
            r["actions"] = "".join(r["actions"])
            r["AL"] = average_lagging(r["delays_ms"], sched.total_ms)
        states = None
        if return_states:
            states = torch.cat(seen, dim=1) if seen else fbank.new_zeros(B, 0, model.cfg.embed_dim)
        return recs, states

    def run_utterance(self, fbank: torch.Tensor, return_states: bool = False):
        """fbank [T, 80] -> the record; with return_states also the encoder rows the head saw, [n, D]."""
        recs, states = self._run(fbank.unsqueeze(0), return_states)
        return (recs[0], states[0]) if return_states else recs[0]


class BatchedCTCStreamingAgent(CTCAgent):
    """B streams of EQUAL length advancing in lockstep through one encoder batch and one pick launch per chunk; every row's record is
    that of CTCAgent.run_utterance on the utterance alone."""

    def run_batch(self, fbank: torch.Tensor, lengths=None, return_states: bool = False):
        """fbank [B, T, 80]; lengths, if given, must all equal T (ragged chunked streaming is not implemented)."""
        if lengths is not None and {int(x) for x in torch.as_tensor(lengths).tolist()} - {fbank.size(1)}:
            raise ValueError("BatchedCTCStreamingAgent: the rows advance in lockstep and need sources of equal length")
        recs, states = self._run(fbank, return_states)
        return (recs, states) if return_states else recs
