"""fp64 restatement, in plain torch on the CPU, of what criterion/rnnt_criterion.py:82-147 computes from the transducer's lattice
(models/transducer_model.py:143-163 with no incremental state):

* ``lattice_inputs``        the decoder input of :143-156 from prev_output_tokens
* ``joiner_lattice``        lp_blank / lp_label [B, S, U1] from P, G, W_out (the joiner alone: what simulst_joiner_lattice is held to)
* ``model_lattice_logits``  the [B, S', U1, V] logits of the whole decoder (tests/transducer_ref.py's prediction network per prefix)
* ``forward_ll``            warp_rnnt's forward recursion (natural log), ``best_alignment`` the same with max and a back-track,
                            ``path_score`` the score of one alignment, ``enumerate_ll`` the brute-force sum over every alignment,
                            ``closed_form_ll`` the value for a lattice whose every entry is log 1/2

An alignment of a row with S frames and n labels is ``emit`` [n], non-decreasing frames in [0, S): label u is taken at frame
emit[u]; the blank is taken once in every frame s at target position #{u: emit[u] <= s} (the last of them leaves the lattice).
"""
import itertools
import math

import torch

import transducer_ref as tr

F64 = torch.float64
NEG = -float("inf")


def lattice_inputs(prev_output_tokens, pad=1, eos=2, bos=0):
    """-> (input [B, U1] = [bos, y_1 .. y_{n-1}, eos, pad ..], labels [B, U1] = input shifted left, tgt_len [B])"""
    prev = prev_output_tokens.clone().to(torch.int64)
    B = prev.shape[0]
    prev[:, 0] = bos
    inp = torch.cat([prev, torch.full((B, 1), pad, dtype=torch.int64)], 1)
    n = inp.ne(pad).sum(1, keepdim=True)
    inp.scatter_(1, n, eos)
    labels = torch.cat([inp[:, 1:], torch.full((B, 1), pad, dtype=torch.int64)], 1)
    return inp, labels, n.view(B)


def joiner_lattice(P, G, W, labels, blank=0, round_z=None):
    """P [B, S, D], G [B, U1, D], W [V, D], labels [B, U1] -> (lp_blank, lp_label, logits [B, S, U1, V]) fp64; every cell is
    computed (the caller masks); round_z: a dtype the tanh is rounded to first"""
    z = torch.tanh(P.to(F64).unsqueeze(2) + G.to(F64).unsqueeze(1))
    if round_z is not None:
        z = z.to(round_z).to(F64)
    logits = z @ W.to(F64).t()
    lp = torch.log_softmax(logits, -1)
    B, S, U1, _ = lp.shape
    idx = labels.to(torch.int64).view(B, 1, U1, 1).expand(B, S, U1, 1)
    return lp[..., blank], lp.gather(3, idx).squeeze(3), logits


def valid_cells(src_len, tgt_len, S, U1):
    """(blank cells, label cells) [B, S, U1] bool: s < src_len[b] and u <= tgt_len[b] (u < tgt_len[b] for the label)"""
    s = torch.arange(S).view(1, S, 1) < torch.as_tensor(src_len).view(-1, 1, 1)
    u = torch.arange(U1).view(1, 1, U1)
    t = torch.as_tensor(tgt_len).view(-1, 1, 1)
    return s & (u <= t), s & (u < t)


def model_lattice_logits(ref: "tr.TransducerRef", enc_btd, enc_len, inp, T=None):
    """the whole decoder: ref.set_source, then the prediction network on every prefix of inp [B, U1] (column 0 is bos) ->
    (logits [B, S', U1, V] fp64, features [B, U1, D], src_len')"""
    ref.set_source(enc_btd, enc_len, T)
    feats = torch.stack([ref.features(inp[:, 1:u + 1]) for u in range(inp.shape[1])], 1)
    G = feats @ ref.w["decoder.joiner.target_projection.weight"].t()
    z = torch.tanh(ref.P.unsqueeze(2) + G.unsqueeze(1))
    return z @ ref.w["decoder.output_projection.weight"].t(), feats, ref.src_len


def logaddexp(a, b):
    if a == NEG:
        return b
    if b == NEG:
        return a
    m = max(a, b)
    return m + math.log1p(math.exp(min(a, b) - m))


def _recursion(lp_blank, lp_label, S, n, join):
    lb, lt = lp_blank.to(F64).tolist(), lp_label.to(F64).tolist()
    a = [[NEG] * (n + 1) for _ in range(S)]
    move = [[0] * (n + 1) for _ in range(S)]
    a[0][0] = 0.0
    for s in range(S):
        for u in range(n + 1):
            if s == 0 and u == 0:
                continue
            vb = a[s - 1][u] + lb[s - 1][u] if s > 0 else NEG
            vl = a[s][u - 1] + lt[s][u - 1] if u > 0 else NEG
            a[s][u] = join(vb, vl)
            move[s][u] = 1 if vl > vb else 0          # the label move only when strictly better (include/simulst_hip.h)
    return a, move, a[S - 1][n] + lb[S - 1][n]


def forward_ll(lp_blank, lp_label, S, n):
    """one row: lp_blank / lp_label [>= S, >= n + 1] -> (ll, max |alpha|) in fp64"""
    a, _, ll = _recursion(lp_blank, lp_label, S, n, logaddexp)
    return ll, max(abs(v) for row in a for v in row if v != NEG)


def best_alignment(lp_blank, lp_label, S, n):
    """-> (best_ll, emit [n]) in fp64, the header's tie rule"""
    _, move, best = _recursion(lp_blank, lp_label, S, n, max)
    emit, s, u = [0] * n, S - 1, n
    while s > 0 or u > 0:
        if u > 0 and (s == 0 or move[s][u]):
            emit[u - 1] = s
            u -= 1
        else:
            s -= 1
    return best, emit


def path_score(lp_blank, lp_label, S, n, emit):
    lb, lt = lp_blank.to(F64), lp_label.to(F64)
    total = sum(float(lt[emit[u], u]) for u in range(n))
    for s in range(S):
        total += float(lb[s, sum(1 for e in emit if e <= s)])
    return total


def enumerate_ll(lp_blank, lp_label, S, n):
    """log of the sum over EVERY alignment (combinations with replacement of n frames out of S)"""
    scores = [path_score(lp_blank, lp_label, S, n, list(emit)) for emit in itertools.combinations_with_replacement(range(S), n)]
    return float(torch.logsumexp(torch.tensor(scores, dtype=F64), 0)), max(scores)


def closed_form_ll(S, n):
    """every entry log 1/2: C(S - 1 + n, n) alignments of S + n moves each"""
    return math.lgamma(S + n) - math.lgamma(S) - math.lgamma(n + 1) + (S + n) * math.log(0.5)


def ll_bound(S, n, max_alpha):
    """|ll - ref| of an fp32 recursion: one rounding of the sum and one of the log-add per move, S + n + 1 of them"""
    return (S + n + 1) * 2.0 ** -22 * max(1.0, max_alpha)


def random_lattice(B, S, U1, seed, classes=8, scale=3.0):
    """log_softmax of scale * N(0, 1) over `classes`: class 0 the blank, class 1 the label"""
    lp = torch.log_softmax(scale * torch.randn(B, S, U1, classes, generator=torch.Generator().manual_seed(seed)), -1)
    return lp[..., 0].contiguous(), lp[..., 1].contiguous()
