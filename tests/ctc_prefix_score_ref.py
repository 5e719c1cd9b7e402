"""fp64 restatement of the CTC prefix scores inside the attention beam (DESIGN.md "Beam search", "CTC prefix scores inside the beam";
tests only, nothing here is imported by the package): plain Python over lists of floats, one hypothesis and one candidate at a time.

x[t][v] are the head's log-probabilities of a sentence, T its frames.  A state is (gn, gb, psi): two lists of T floats and the prefix
log-probability.  brute_psi is the DEFINITION of psi: every one of the V^T frame labellings, collapsed, summed where the string starts
with the prefix."""
import itertools
import math

from ctc_beam_ref import NEG, beam_bound, collapse, lae   # noqa: F401  (beam_bound: the tests' tolerance)

FLOOR = -1.0e4


def empty_state(x, T, blank=0):
    gb, run = [], 0.0
    for t in range(T):
        run += x[t][blank]
        gb.append(run)
    return [NEG] * T, gb, 0.0


def extend(x, T, state, last, c, blank=0):
    """the state of g + (c,) from the state of g; last = the last label of g, None for the empty g; c a label (not blank)"""
    gn, gb, _ = state
    assert c != blank

    def phi(t):
        if t < 0:
            return 0.0 if last is None else NEG
        return gb[t] if c == last else lae(gn[t], gb[t])

    n_gn, n_gb, psi = [], [], NEG
    pn = pb = NEG
    for t in range(T):
        a = lae(pn, phi(t - 1)) + x[t][c]
        b = lae(pn, pb) + x[t][blank]
        psi = lae(psi, phi(t - 1) + x[t][c])
        n_gn.append(a)
        n_gb.append(b)
        pn, pb = a, b
    return n_gn, n_gb, psi


def psi_end(T, state, empty):
    """psi(g . eos): the probability of g as the whole transcript"""
    gn, gb, _ = state
    if T == 0:
        return 0.0 if empty else NEG
    return lae(gn[T - 1], gb[T - 1])


def string_state(x, T, labels, blank=0):
    """the state of a string, extended label by label from the empty prefix"""
    st, last = empty_state(x, T, blank), None
    for c in labels:
        st, last = extend(x, T, st, last, c, blank), c
    return st


def candidate(x, T, state, last, c, *, blank=0, pad=1, eos=2):
    """-> (psi(h), state of h or None) for candidate c of hypothesis g (state, last)"""
    if c < 0 or c == blank or c == pad:
        return NEG, None
    if c == eos:
        return psi_end(T, state, last is None), None
    st = extend(x, T, state, last, c, blank)
    return st[2], st


def delta(psi_h, psi_g):
    return FLOOR if psi_h == NEG else max(psi_h - psi_g, FLOOR)


def combine(lp_att, d, lam):
    if lp_att == NEG:
        return NEG
    if lam == 0:
        return lp_att
    return (1.0 - lam) * lp_att + lam * d


def score_row(x, T, state, last, toks, lps, lam, *, blank=0, pad=1, eos=2):
    """one beam row: candidates toks / lps (attention log-probabilities) -> {"psi": per slot, "state": per slot (None: no label),
    "score": per slot, "order": the slots in candidate order (descending score, equal scores to the lower token, then the lower slot),
    "floored": per slot}"""
    psi, states, score, floored = [], [], [], []
    for c, lp in zip(toks, lps):
        p, st = candidate(x, T, state, last, c, blank=blank, pad=pad, eos=eos)
        d = delta(p, state[2])
        psi.append(p)
        states.append(st)
        floored.append(d == FLOOR)
        score.append(combine(lp, d, lam))
    order = sorted(range(len(toks)), key=lambda k: (-score[k], toks[k], k))
    return {"psi": psi, "state": states, "score": score, "order": order, "floored": floored}


def brute_psi(x, T, h, blank=0):
    """log of the summed probability of all V^T labellings of T frames whose collapsed string starts with h (h = (): every labelling)"""
    V = len(x[0]) if T else 0
    h = tuple(h)
    acc = NEG
    for path in itertools.product(range(V), repeat=T):
        if collapse(path, blank)[:len(h)] == h:
            acc = lae(acc, sum(x[t][c] for t, c in enumerate(path)))
    if T == 0:
        return 0.0 if not h else NEG
    return acc


def log_softmax_rows(rows):
    out = []
    for r in rows:
        m = max(r)
        z = m + math.log(sum(math.exp(v - m) for v in r))
        out.append([v - z for v in r])
    return out


# ---- cases for the scoring step: tensors for ctc.ctc_prefix_score and the restatement's answer, shared by the CPU and GPU tests ------
def make_case(seed, Bs, G, K, V, S, lens, lam, *, blank=0, pad=1, eos=2, first_only=False, finished=(), att_inf=True):
    """Random hypotheses (0..3 labels, repeats included) with their fp32 states and K distinct candidates a row: where K allows, the
    row's last label (c == e), EOS, the blank, pad and a negative id are among them, in random slots.  Frames at and past a sentence's
    length are NaN in every input.  Returns the tensors (CPU) and what the restatement needs."""
    import torch
    g = torch.Generator().manual_seed(seed)
    R = Bs * G
    x = torch.log_softmax(torch.randn(Bs, S, V, generator=g, dtype=torch.float64) * 2.0, dim=-1).float()
    nan = float("nan")
    state = torch.full((R, S, 2), nan)
    psi = torch.zeros(R)
    last = torch.full((R,), -1, dtype=torch.int64)
    plen = torch.zeros(R, dtype=torch.int64)
    in_len = torch.tensor([lens[r // G] for r in range(R)], dtype=torch.int64)
    cand_tok = torch.zeros(R, K, dtype=torch.int32)
    cand_lp = -(torch.rand(R, K, generator=g) * 6.0 + 0.01)
    rows = []
    labels_ok = [v for v in range(V) if v not in (blank, pad, eos)]
    for r in range(R):
        s, T = r // G, lens[r // G]
        xs = x[s].double().tolist()
        n = int(torch.randint(0, 4, (1,), generator=g)) if r % 3 else (r // 3) % 2       # some empty, some one-label prefixes
        lab = [labels_ok[int(torch.randint(0, len(labels_ok), (1,), generator=g))] for _ in range(n)]
        if n >= 2 and r % 2:
            lab[-1] = lab[-2]                                                            # a repeated label
        st = string_state(xs, T, lab, blank)
        for t in range(T):
            state[r, t, 0], state[r, t, 1] = st[0][t], st[1][t]
        psi[r] = st[2]
        plen[r] = n
        if n:
            last[r] = lab[-1]
        want = ([lab[-1]] if n else []) + [eos, blank, pad, -1]
        pool = [v for v in labels_ok if v not in want]
        perm = torch.randperm(len(pool), generator=g).tolist()
        toks = (want + [pool[i] for i in perm])[:K] if K >= 6 else ([pool[i] for i in perm] + want)[:K]
        if K < 6 and n and r % 2 == 0:
            toks[0] = lab[-1]
        order = torch.randperm(K, generator=g).tolist()
        toks = [toks[i] for i in order]
        cand_tok[r] = torch.tensor(toks, dtype=torch.int32)
        if att_inf and K >= 2:
            cand_lp[r, int(torch.randint(0, K, (1,), generator=g))] = NEG
        f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))   # noqa: E731
        rows.append({"x": xs, "T": T, "state": ([f32(v) for v in st[0]], [f32(v) for v in st[1]], float(psi[r])),
                     "last": lab[-1] if n else None, "toks": toks, "lps": cand_lp[r].double().tolist(), "labels": lab})
    idx = cand_tok.view(Bs, 1, G * K).to(torch.int64).clamp(0, V - 1).expand(Bs, S, G * K)
    xc = x.gather(2, idx).contiguous()
    xb = x[:, :, blank].contiguous()
    for s in range(Bs):
        xc[s, lens[s]:] = nan
        xb[s, lens[s]:] = nan
    fin = torch.zeros(Bs, dtype=torch.int32)
    for s in finished:
        fin[s] = 1
    return {"x": xc, "xb": xb, "state": state, "psi": psi, "last": last, "plen": plen, "in_len": in_len, "finished": fin,
            "cand_lp": cand_lp, "cand_tok": cand_tok, "rows": rows, "G": G, "K": K, "S": S, "lam": lam, "first_only": first_only,
            "kw": dict(G=G, blank=blank, eos=eos, pad=pad, weight=lam, first_only=first_only)}


SENTINEL = -12345.0


def run_case(case, ops, device, composed=False):
    """ctc.ctc_prefix_score on the case's tensors (moved to `device`); the output buffers start sentinel-filled -> the tensors, on the CPU"""
    import torch

    from simulst_amd import ctc
    R, K, S = case["cand_tok"].size(0), case["K"], case["S"]
    t = {k: case[k].clone().to(device) for k in ("x", "xb", "state", "psi", "last", "plen", "in_len", "finished", "cand_lp", "cand_tok")}
    t["cand_slot"] = torch.full((R, K), -7, dtype=torch.int32, device=device)
    t["cand_state"] = torch.full((R, S, K, 2), SENTINEL, device=device)
    t["cand_psi"] = torch.full((R, K), SENTINEL, device=device)
    ctc.ctc_prefix_score(ops, t["x"], t["xb"], t["state"], t["psi"], t["last"], t["plen"], t["in_len"], t["finished"], t["cand_lp"],
                         t["cand_tok"], t["cand_slot"], t["cand_state"], t["cand_psi"], composed=composed, **case["kw"])
    return {k: v.cpu() for k, v in t.items()}


def score_tol(lam, T, psi_h, lp, d):
    """what fp32 may lose on a combined score: lam x the recursion's bound on psi(h), plus a few roundings of the combination's terms"""
    return lam * beam_bound(T, psi_h if psi_h != NEG else 1.0) + 4 * 2.0 ** -24 * (abs(lp) + abs(d) + 1.0)


def check_case(case, out):
    """every touched row against the restatement; every other row bit for bit as it was.  -> rows checked"""
    import torch
    G, K, lam = case["G"], case["K"], case["lam"]
    checked = 0
    for r, row in enumerate(case["rows"]):
        s, j, T = r // G, r % G, row["T"]
        if int(case["finished"][s]) or (case["first_only"] and j > 0):
            assert torch.equal(out["cand_lp"][r], case["cand_lp"][r]) and torch.equal(out["cand_tok"][r], case["cand_tok"][r]), r
            assert bool((out["cand_state"][r] == SENTINEL).all()) and bool((out["cand_psi"][r] == SENTINEL).all()), r
            assert bool((out["cand_slot"][r] == -7).all()), r
            continue
        checked += 1
        ref = score_row(row["x"], T, row["state"], row["last"], row["toks"], row["lps"], lam)
        assert not bool(torch.isnan(out["cand_psi"][r]).any()) and not bool(torch.isnan(out["cand_lp"][r]).any()), r
        assert not bool(torch.isnan(out["cand_state"][r, :T]).any()), r
        assert bool((out["cand_state"][r, T:] == SENTINEL).all()), (r, "frames past T written")
        got_state, got_psi = out["cand_state"][r, :T].tolist(), out["cand_psi"][r].tolist()
        for k in range(K):
            p = got_psi[k]
            if ref["psi"][k] == NEG:
                assert p == NEG, (r, k, p)
            else:
                assert abs(p - ref["psi"][k]) <= beam_bound(T, ref["psi"][k]), (r, k, p, ref["psi"][k])
            st = ref["state"][k]
            for t in range(T):
                for i in (0, 1):
                    v, w = got_state[t][k][i], (st[i][t] if st is not None else NEG)
                    assert (v == w) if w == NEG else abs(v - w) <= beam_bound(t + 1, w), (r, k, t, i, v, w)
        slots = out["cand_slot"][r].tolist()
        assert sorted(slots) == list(range(K)), (r, slots)
        tols = []
        for pos, k in enumerate(slots):
            assert int(out["cand_tok"][r, pos]) == row["toks"][k], (r, pos)
            v, w = float(out["cand_lp"][r, pos]), ref["score"][k]
            tol = score_tol(lam, T, ref["psi"][k], row["lps"][k], delta(ref["psi"][k], row["state"][2]))
            tols.append(tol)
            if w == NEG:
                assert v == NEG, (r, pos, v)
            elif lam == 0:
                assert v == float(torch.tensor(row["lps"][k], dtype=torch.float32)), (r, pos)
            else:
                assert abs(v - w) <= tol, (r, pos, v, w, tol)
        got = out["cand_lp"][r].tolist()
        assert all(a >= b for a, b in zip(got, got[1:])), (r, got)
        srt = sorted(ref["score"], reverse=True)
        fin = [v for v in srt if v != NEG]
        clear = all(a - b > 2 * max(tols) or a == b for a, b in zip(fin, fin[1:]))
        if clear:                                               # no near-tie fp32 may resolve the other way: the order itself
            assert slots == ref["order"], (r, slots, ref["order"])
    return checked
