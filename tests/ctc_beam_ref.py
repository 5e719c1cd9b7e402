"""fp64 references for the CTC head's candidate lists and prefix beam search (tests only; nothing here is imported by the package).

topk64 / check_topk: the best k columns of fp64 logits under the total order (value descending, lower column first) and the clear /
unclear rule of the top-k tests.  prefix_beam_ref: the textbook time-synchronous prefix beam search as a plain-Python dict of tuples,
over candidate lists it is GIVEN (so that a device search is compared on the device's own candidates).  brute_force: every path."""
import itertools
import math

import torch

NEG = float("-inf")


def lae(a, b):
    """log(exp a + exp b) in the form the search uses: max + log1p(exp(-|a - b|)), -inf where both are"""
    if a == NEG and b == NEG:
        return NEG
    return max(a, b) + math.log1p(math.exp(-abs(a - b))) if a != NEG and b != NEG else max(a, b)


def topk64(z, k, keep=None):
    """z [M, N] fp64 -> (ids [M, k'] int64, lprob [M, k'] fp64, lse [M], vals [M, min(k + 1, N')] fp64: the best k + 1 values among the
    N' columns other than keep, descending).  k' = k + (keep is not None): slot 0 = keep, then the k best other columns, ties to the
    lower column; -1 / -inf where there are fewer."""
    M, N = z.shape
    lse = torch.logsumexp(z, dim=1)
    zz = z.clone()
    if keep is not None:
        zz[:, keep] = NEG
    order = torch.sort(zz, dim=1, descending=True, stable=True)
    n_other = N - (keep is not None)
    kk = min(k, n_other)
    ids = torch.full((M, k), -1, dtype=torch.int64)
    val = torch.full((M, k), NEG, dtype=torch.float64)
    ids[:, :kk], val[:, :kk] = order.indices[:, :kk], order.values[:, :kk]
    vals = order.values[:, :min(k + 1, n_other)]
    if keep is not None:
        ids = torch.cat([torch.full((M, 1), keep, dtype=torch.int64), ids], dim=1)
        val = torch.cat([z[:, keep:keep + 1], val], dim=1)
    return ids, val - lse.unsqueeze(1), lse, vals


def unclear_rows(z, k, keep, e):
    """rows in which two neighbours among the best k + 1 non-keep values lie within 2e of each other"""
    vals = topk64(z, k, keep)[3]
    if vals.size(1) < 2:
        return torch.zeros(z.size(0), dtype=torch.bool)
    return ((vals[:, :-1] - vals[:, 1:]) <= 2 * e).any(dim=1)


def check_topk(z, ids, lprob, lse, k, keep, e, what=""):
    """The rule of the top-k tests -> boolean mask of the unclear rows.
    every row: lprob and lse within e (+ 1e-6 |lse|) of fp64 AT THE RETURNED COLUMNS, the keep slot first, -1 slots at the end with -inf;
    clear row: the fp64 ids exactly, in order; unclear row: distinct columns other than keep whose fp64 value is within 2e of the fp64
    k-th value or above, in an order descending to within 2e."""
    M, N = z.shape
    kb = int(keep is not None)
    ids = ids.detach().cpu().to(torch.int64).view(M, k + kb)
    lprob = lprob.detach().cpu().double().view(M, k + kb)
    lse = lse.detach().cpu().double().view(M)
    r_ids, _, r_lse, vals = topk64(z, k, keep)
    kk = min(k, N - kb)
    tol = e + 1e-6 * r_lse.abs()
    assert bool(((lse - r_lse).abs() <= tol).all()), f"{what}: lse off by {float((lse - r_lse).abs().max()):.3e} (e {e:.3e})"
    if kb:
        assert bool((ids[:, 0] == keep).all()), f"{what}: slot 0 is not keep"
    assert bool((ids[:, kb + kk:] == -1).all()) and bool((lprob[:, kb + kk:] == NEG).all()), f"{what}: slots past the columns"
    got = ids[:, :kb + kk]
    assert int(got.min()) >= 0 and int(got.max()) < N, f"{what}: column out of range"
    zg = z.gather(1, got)
    dl = ((lprob[:, :kb + kk] - (zg - r_lse.unsqueeze(1))).abs() - tol.unsqueeze(1)).max()
    assert float(dl) <= 0, f"{what}: lprob off by {float(dl):.3e} beyond e {e:.3e}"
    unclear = unclear_rows(z, k, keep, e)
    wrong = (~unclear) & (ids != r_ids).any(dim=1)
    assert not bool(wrong.any()), f"{what}: {int(wrong.sum())} clear rows differ from fp64, first row {int(wrong.nonzero()[0])}"
    if kk and bool(unclear.any()):
        g, zk = got[unclear, kb:], zg[unclear, kb:]
        gs = g.sort(dim=1).values
        assert bool((gs[:, 1:] != gs[:, :-1]).all()), f"{what}: repeated column"
        if kb:
            assert bool((g != keep).all()), f"{what}: keep among the candidates"
        kth = vals[unclear, kk - 1].unsqueeze(1)
        assert bool((zk >= kth - 2 * e).all()), f"{what}: unclear row holds a column more than 2e below the k-th value"
        if kk > 1:
            assert bool((zk[:, 1:] <= zk[:, :-1] + 2 * e).all()), f"{what}: unclear row not descending to within 2e"
    return unclear


def prefix_beam_ref(ids, lp, beam, nbest=1):
    """ids [T][k + 1] ints (slot 0 the blank, -1 = no candidate), lp [T][k + 1] floats -> (hyps: [(tuple of labels, score)] best first,
    at most beam; margin: the smallest gap, over all frames, between the last prefix kept and the first one dropped, and between
    neighbours among the final best nbest + 1).  Pool order: the beam's own entries, then prefix-major candidate-minor extensions;
    ties keep that order (a stable sort)."""
    hyps = [((), 0.0, NEG)]
    margin = float("inf")
    for t in range(len(ids)):
        pool = {}
        for l, pb, pnb in hyps:
            stay_nb = NEG
            if l:
                for j in range(1, len(ids[t])):
                    if ids[t][j] == l[-1]:
                        stay_nb = pnb + lp[t][j]
            pool[l] = [lae(pb, pnb) + lp[t][0], stay_nb]
        for l, pb, pnb in hyps:
            for j in range(1, len(ids[t])):
                c = ids[t][j]
                if c < 0:
                    continue
                v = (pb if l and c == l[-1] else lae(pb, pnb)) + lp[t][j]
                key = l + (c,)
                if key in pool:
                    pool[key][1] = lae(pool[key][1], v)
                else:
                    pool[key] = [NEG, v]
        items = [(l, b, nb) for l, (b, nb) in pool.items() if lae(b, nb) > NEG]
        items.sort(key=lambda it: -lae(it[1], it[2]))
        if len(items) > beam:
            margin = min(margin, lae(items[beam - 1][1], items[beam - 1][2]) - lae(items[beam][1], items[beam][2]))
        hyps = items[:beam]
    out = [(l, lae(b, nb)) for l, b, nb in hyps]
    for a, b in zip(out[:nbest], out[1:nbest + 1]):
        margin = min(margin, a[1] - b[1])
    return out, margin


def collapse(path, blank=0):
    out = []
    prev = None
    for c in path:
        if c != blank and c != prev:
            out.append(c)
        prev = c
    return tuple(out)


def brute_force(lp, blank=0):
    """lp [T][V] log-probabilities -> {labeling: log of the summed probability of all V^T paths that collapse to it}"""
    T, V = len(lp), len(lp[0])
    acc = {}
    for path in itertools.product(range(V), repeat=T):
        s = sum(lp[t][c] for t, c in enumerate(path))
        key = collapse(path, blank)
        acc[key] = lae(acc[key], s) if key in acc else s
    return acc


def full_candidates(lp_row, blank=0):
    """every label of a frame as a candidate list: (ids, lp) with the blank first, then the others by descending value, lower label first"""
    others = sorted((c for c in range(len(lp_row)) if c != blank), key=lambda c: (-lp_row[c], c))
    ids = [blank] + others
    return ids, [lp_row[c] for c in ids]


# ---- the operands of the top-k cases: made here so that the CPU test of the seeds and the GPU tests read the same ones ---------------
TOPK_SHAPES = [(1, 256, 4096), (17, 256, 4096), (130, 256, 4097), (513, 64, 100), (64, 256, 16), (33, 32, 1), (5, 32, 8)]
TOPK_SPLIT_SHAPES = [(8128, 64, 272), (8129, 64, 272)]
TOPK_SEED_SHIFT = {(130, 256, 4097, "float32", True): 100, (64, 256, 16, "float32", False): 100}       # (M, K, N, dtype name, with_bias) -> added to the seed where the default one left too many unclear rows


def topk_operands(M, K, N, dtype, with_bias):
    """x ~ N(0, 1), W ~ N(0, 1) 4 / sqrt(K) rounded to dtype, bias ~ N(0, 1) fp32 or None, and the fp64 logits of the rounded operands"""
    key = (M, K, N, str(dtype).replace("torch.", ""), bool(with_bias))
    g = torch.Generator().manual_seed(1000 * M + N + K + int(with_bias) + TOPK_SEED_SHIFT.get(key, 0))
    x = torch.randn(M, K, generator=g).to(dtype)
    W = (torch.randn(N, K, generator=g) * 4 / math.sqrt(K)).to(dtype)
    bias = torch.randn(N, generator=g) if with_bias else None
    z = x.double() @ W.double().t()
    if bias is not None:
        z = z + bias.double()
    return x, W, bias, z


# ---- the inputs of the beam-search cases (bare head: D = 64, V = 40, B = 6, ragged lengths with 0 and 1, Te = 48) -----------------------
BEAM_LENGTHS = [48, 0, 1, 17, 33, 41]
BEAM_SEEDS = {"float32": 5, "bfloat16": 6}


def beam_operands(dtype, seed=None, D=64, V=40, spread=6.0):
    """rows ~ N(0, 1), head ~ N(0, 1) spread / sqrt(D), both rounded to dtype, the lengths, and the fp64 log-probabilities [B, Te, V]"""
    name = str(dtype).replace("torch.", "")
    g = torch.Generator().manual_seed(BEAM_SEEDS[name] if seed is None else seed)
    B, Te = len(BEAM_LENGTHS), max(BEAM_LENGTHS)
    enc = torch.randn(B, Te, D, generator=g).to(dtype)
    W = (torch.randn(V, D, generator=g) * spread / math.sqrt(D)).to(dtype)
    lp = torch.log_softmax(enc.double() @ W.double().t(), dim=-1)
    return enc, W, torch.tensor(BEAM_LENGTHS), lp


def beam_bound(n_frames, score):
    """(Te_b + 1) 2^-22 max(1, |score|): the form tests/test_hip_ctc_nll.py uses for fp32 recursions over Te_b frames"""
    return (n_frames + 1) * 2.0 ** -22 * max(1.0, abs(score))


def candidates_of(ids_bt, lp_bt, n_frames):
    """device candidate tensors of one utterance [Te, k + 1] -> the Python lists prefix_beam_ref takes, its valid frames only"""
    return ids_bt[:n_frames].tolist(), lp_bt[:n_frames].double().tolist()
