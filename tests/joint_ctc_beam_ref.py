"""CPU restatement of beam search with CTC prefix scores inside the beam (DESIGN.md "Beam search" with its subsection "CTC prefix
scores inside the beam"; tests only): tests/test_hip_beam.py's cpu_beam with the rescoring step between the per-row top 2 beam and the
sentence's selection.  The attention side is fp32 log_softmax as the device computes it; the CTC side is the fp64 restatement of
tests/ctc_prefix_score_ref.py, one candidate at a time; cumulative scores are fp64."""
import math

import torch

import ctc_prefix_score_ref as ps

NEG = -float("inf")


def joint_beam(logits_fn, ctc_lp, caps, beam, V, eos, pad, lenpen, nbest, lam, blank=0, on_select=None):
    """logits_fn(step, tokens [R] int64) -> fp32 logits [R, V] (CPU); ctc_lp[s]: the head's log-probabilities of sentence s over its own
    frames, [T_s][V] floats; on_select(step, reorder [R] int64) reorders the caller's state.  lam = 0 is the plain search.
    -> (per sentence the nbest list of (tokens, score, positional scores, floored: the CTC floor applied somewhere on the hypothesis),
        per sentence the gaps of every step it ran: the smallest difference that decides something -- between the last candidate the
        attention pre-selection keeps in a row and the first it drops, and between neighbours of the sentence's sorted combined
        candidates up to the first one past the 2 beam the selection reads)."""
    Bs, K = len(caps), 2 * beam
    R = Bs * beam
    toks = torch.full((R,), eos, dtype=torch.int64)
    cum = [0.0] * R
    paths, cums, flo = [[] for _ in range(R)], [[] for _ in range(R)], [False] * R
    states = [ps.empty_state(ctc_lp[r // beam], len(ctc_lp[r // beam]), blank) for r in range(R)]
    lasts = [None] * R
    fin, done, gaps = [[] for _ in range(Bs)], [False] * Bs, [[] for _ in range(Bs)]
    for t in range(max(caps) + 1):
        if all(done):
            break
        lp = torch.log_softmax(logits_fn(t, toks).float(), dim=-1)
        reorder = torch.arange(R)
        new = {"tok": toks.clone(), "cum": list(cum), "paths": [list(p) for p in paths], "cums": [list(c) for c in cums],
               "flo": list(flo), "states": list(states), "lasts": list(lasts)}
        for s in range(Bs):
            if done[s]:
                continue
            x, T = ctc_lp[s], len(ctc_lp[s])
            pool, gap = [], math.inf
            for j in range(1 if t == 0 else beam):
                r = s * beam + j
                lps = lp[r].clone()
                lps[pad] = NEG
                if t == 0:
                    lps[eos] = NEG
                if t >= caps[s]:
                    keep = lps[eos].clone()
                    lps[:] = NEG
                    lps[eos] = keep
                vals, idx = torch.sort(lps, descending=True, stable=True)
                if float(vals[K]) > NEG:
                    gap = min(gap, float(vals[K - 1] - vals[K]))
                ctoks, clps = [int(i) for i in idx[:K]], [float(v) for v in vals[:K]]
                res = ps.score_row(x, T, states[r], lasts[r], ctoks, clps, lam, blank=blank, pad=pad, eos=eos)
                for k in range(K):
                    pool.append(((0.0 if t == 0 else cum[r]) + res["score"][k], j * V + ctoks[k], j, ctoks[k], res["state"][k],
                                 res["floored"][k] and lam != 0))
            pool.sort(key=lambda c: (-c[0], c[1]))
            fv = [c[0] for c in pool[:K + 1] if c[0] > NEG]
            gap = min([gap] + [a - b for a, b in zip(fv, fv[1:])])
            gaps[s].append(gap)
            top = pool[:K]
            for score, _, j, v, _, fl in top[:beam]:
                if v == eos and score > NEG and len(fin[s]) < beam:
                    parent = s * beam + j
                    c = torch.tensor(cums[parent] + [score], dtype=torch.float64)
                    fin[s].append((paths[parent] + [eos], score / (t + 1) ** lenpen, torch.cat([c[:1], c[1:] - c[:-1]]), flo[parent] or fl))
            if len(fin[s]) == beam or t == caps[s]:
                done[s] = True
                continue
            active = [c for c in top if not (c[3] == eos and c[0] > NEG)][:beam]
            assert len(active) == beam and all(c[0] > NEG and c[3] != eos for c in active)
            for jn, (score, _, j, v, st, fl) in enumerate(active):
                r, parent = s * beam + jn, s * beam + j
                reorder[r] = parent
                new["tok"][r], new["cum"][r] = v, score
                new["paths"][r], new["cums"][r] = paths[parent] + [v], cums[parent] + [score]
                new["flo"][r] = flo[parent] or fl
                # a candidate that is no label (the blank, chosen by the attention side) has no alignment: every score behind it is -inf
                new["states"][r] = st if st is not None else ([NEG] * T, [NEG] * T, NEG)
                new["lasts"][r] = v
        toks, cum, paths, cums, flo, states, lasts = (new[k] for k in ("tok", "cum", "paths", "cums", "flo", "states", "lasts"))
        if on_select is not None:
            on_select(t, reorder)
    return [sorted(fin[s], key=lambda h: h[1], reverse=True)[:nbest] for s in range(Bs)], gaps


def rows_of(lp_btv, lens):
    """[Bs, S, V] tensor -> what joint_beam takes: per sentence its own frames as lists of fp64 floats"""
    return [lp_btv[s, :int(lens[s])].double().tolist() for s in range(lp_btv.size(0))]
