"""A streaming loop around the fp64 restatement of the transducer (tests/transducer_ref.py): ONE row whose source is released
chunk by chunk.  A row READs while none of the pooled positions released so far emits and the source has not ended, and WRITEs
otherwise; once the source has ended its last position is forced, as in the offline decode.  Only complete windows of k encoder rows
are pooled while the source is open; the partial last window is the mean of its valid rows.

``stream_row`` returns what was written (tokens, emit positions), at which chunk, the READ / WRITE string, and per token the smallest
fp64 margin of the decisions behind it (every scanned position's |best non-blank - blank|, and top-1 against top-2 of the row the
token is picked from): a comparison excuses the tokens behind the first unclear one."""
import torch

import transducer_ref as tr


def pooled_row(enc_nd, k):
    """[n, D] -> fp64 [ceil(n / k), D]: window means (the partial last window over its valid rows)"""
    x = enc_nd.to(tr.F64)
    return torch.stack([x[j:j + k].mean(0) for j in range(0, x.shape[0], k)])


def stream_row(ref, enc_nd, schedule, n_max, stop=None):
    """ref: a TransducerRef; enc_nd [n, D] the row's encoder states; schedule[c]: encoder rows released after chunk c (cumulative,
    the last chunk ends the source); at most n_max tokens; stop(tokens, chunk) -> True ends the row after a token (EOS / cap rule).
    -> {"tokens", "emit", "chunk": per token, "actions", "margin": per token}"""
    k, n = ref.k, enc_nd.shape[0]
    assert schedule[-1] == n
    w = ref.w
    P_all = pooled_row(enc_nd, k) @ w["decoder.joiner.source_projection.weight"].t() + w["decoder.joiner.source_projection.bias"] \
        if n > 0 else torch.zeros(0, ref.D, dtype=tr.F64)
    W = w["decoder.output_projection.weight"]
    S = P_all.shape[0]
    tokens, emit, chunk, margin, actions = [], [], [], [], []
    pe, pending = 0, float("inf")
    for c in range(len(schedule)):
        actions.append("R")
        closed = c == len(schedule) - 1
        a = S if closed else schedule[c] // k
        while len(tokens) < n_max and a > 0:
            hyp = torch.tensor([tokens], dtype=torch.int64).view(1, len(tokens))
            g = ref.features(hyp) @ w["decoder.joiner.target_projection.weight"].t()
            logits = tr.joiner_logits(P_all[:a].unsqueeze(0), g, W)[0]             # [a, V]
            ne, m = None, []
            for s in range(min(pe, a if not closed else a - 1), a):
                row = logits[s].clone()
                if closed and s == a - 1:
                    row[tr.BLANK] = tr.BLANK_AT_EOS
                nb = torch.cat([row[:tr.BLANK], row[tr.BLANK + 1:]]).max()
                m.append(float((nb - row[tr.BLANK]).abs()))
                if nb > row[tr.BLANK]:
                    ne = s
                    break
            if ne is None:                        # the row waits; its margins count for the token it writes later
                pending = min([pending] + m)
                break
            first = not tokens
            tok = tr.greedy_pick(row, ref.pad, ref.eos, first)
            mm = min(m + [tr.top2_margin(row, ref.pad, ref.eos, first)])
            mm, pending = min(mm, pending), float("inf")
            tokens.append(tok), emit.append(ne), chunk.append(c), margin.append(mm), actions.append("W")
            pe = ne
            if stop is not None and stop(tokens, c):
                return {"tokens": tokens, "emit": emit, "chunk": chunk, "actions": "".join(actions), "margin": margin}
        if len(tokens) >= n_max:
            break
    return {"tokens": tokens, "emit": emit, "chunk": chunk, "actions": "".join(actions), "margin": margin}


def reads_between_writes(chunks):
    """a row READ between two WRITEs: two consecutive tokens written at different chunks"""
    return any(b > a for a, b in zip(chunks, chunks[1:]))
