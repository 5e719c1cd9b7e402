"""Hand-made candidate lists for the prefix beam recursion kernel (csrc/ctc_prefix.hip behind ctc.ctc_prefix_beam_advance) and what the
fp64 reference of tests/ctc_beam_ref.py says about them (tests only; nothing here is imported by the package).

Two generators, both on the CPU in fp64 with the log-probabilities rounded to fp32 (the reference reads the ROUNDED values, like the
device): peaky frames, whose best prefix is one label a frame -- long strings, hundreds of merges --, and flat small vocabularies, where
prefixes leave the beam and come back.  reentry_events counts the case the kernel's parent cache must not miss: an extension that is
added to a beam entry whose parent string was OUT of the beam at some frame since that entry came in.

A case is a batch, one utterance per seed.  Everything is made once per process and shared by the tests that read it."""
import torch

import ctc_beam_ref as br

NEG = float("-inf")


def peaky_lists(T, V, k, seed):
    """z = randn(T, V) fp64 with +12 on one label a frame (1..V-1, never the label of the frame before) -> (ids [T, k + 1] int64, lp
    [T, k + 1] fp32)"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(T, V, generator=g, dtype=torch.float64)
    lab = torch.randint(1, V, (T,), generator=g).tolist()
    for t in range(1, T):
        if lab[t] == lab[t - 1]:
            lab[t] = lab[t] + 1 if lab[t] + 1 < V else 1
    z[torch.arange(T), torch.tensor(lab)] += 12.0
    ids, lp, _, _ = br.topk64(z, k, keep=0)
    return ids, lp.to(torch.float32)


def flat_lists(T, V, k, spread, seed):
    """z = spread * randn(T, V) fp64 -> (ids [T, k + 1] int64, lp [T, k + 1] fp32)"""
    g = torch.Generator().manual_seed(seed)
    z = spread * torch.randn(T, V, generator=g, dtype=torch.float64)
    ids, lp, _, _ = br.topk64(z, k, keep=0)
    return ids, lp.to(torch.float32)


# name -> (generator, per-utterance arguments without the seed, seeds, beam)
PEAKY_SEEDS = list(range(500, 516))
FLAT_SEEDS = list(range(1000, 1032))
CASES = {
    "peaky_T130_V12_k8_beam16": ("peaky", (130, 12, 8), PEAKY_SEEDS, 16),
    "peaky_T130_V40_k8_beam8": ("peaky", (130, 40, 8), PEAKY_SEEDS, 8),
    "peaky_T70_V12_k8_beam16": ("peaky", (70, 12, 8), PEAKY_SEEDS, 16),
    "peaky_T130_V12_k3_beam2": ("peaky", (130, 12, 3), PEAKY_SEEDS, 2),
    "flat_T48_V40_k8_beam8": ("flat", (48, 40, 8, 6.0), FLAT_SEEDS, 8),
    "flat_T48_V40_k8_beam1": ("flat", (48, 40, 8, 6.0), FLAT_SEEDS, 1),
    "flat_T48_V40_k1_beam8": ("flat", (48, 40, 1, 6.0), FLAT_SEEDS, 8),
    "flat_T48_V6_k3_beam4": ("flat", (48, 6, 3, 4.0), FLAT_SEEDS, 4),
}
# (V, beam, spread, seed), T = 24, k = V - 1: each holds a merge onto the child of a parent that had left the beam and come back
REENTRY = [(4, 3, 1.5, 71), (4, 3, 1.5, 91), (4, 3, 1.5, 132), (4, 3, 1.5, 140), (5, 3, 2.0, 190), (5, 4, 2.0, 9), (6, 4, 2.5, 54),
           (4, 2, 1.5, 604)]
REENTRY_T = 24
for _V, _beam, _spread, _seed in REENTRY:
    CASES[f"reentry_V{_V}_beam{_beam}_seed{_seed}"] = ("flat", (REENTRY_T, _V, _V - 1, _spread), [_seed], _beam)

_MADE = {}


NBEST = 4          # the n-best whose identity is compared (tests/test_hip_ctc_beam.py's), or the beam where that is smaller


def case(name):
    """-> {"ids" [B, T, k + 1] int32, "lp" [B, T, k + 1] fp32, "beam", "T", "lengths", "nbest" = min(NBEST, beam), "ref": per utterance (hyps,
    margin) of prefix_beam_ref for that n-best, "unclear": per utterance, the rule of tests/test_hip_ctc_beam.py (margin <= 2 x bound),
    "unclear_beam": the same rule with the margin taken over the whole beam's ranking -- where that is clear too, every slot is compared}"""
    if name not in _MADE:
        kind, args, seeds, beam = CASES[name]
        gen = peaky_lists if kind == "peaky" else flat_lists
        lists = [gen(*args, seed) for seed in seeds]
        _MADE[name] = _with_reference(torch.stack([i for i, _ in lists]), torch.stack([l for _, l in lists]), beam)
    return _MADE[name]


def _with_reference(ids, lp, beam, lengths=None):
    ids = ids.to(torch.int32)
    T = ids.size(1)
    lengths = [T] * ids.size(0) if lengths is None else list(lengths)
    ref, unclear, unclear_beam = [], [], []
    for b, n in enumerate(lengths):
        lists_b = br.candidates_of(ids[b], lp[b], n)
        hyps, margin = br.prefix_beam_ref(*lists_b, beam=beam, nbest=min(NBEST, beam))
        ref.append((hyps, margin))
        unclear.append(margin <= 2 * br.beam_bound(n, hyps[0][1]))
        unclear_beam.append(br.prefix_beam_ref(*lists_b, beam=beam, nbest=beam)[1] <= 2 * br.beam_bound(n, hyps[0][1]))
    return {"ids": ids, "lp": lp, "beam": beam, "T": T, "lengths": lengths, "nbest": min(NBEST, beam), "ref": ref, "unclear": unclear,
            "unclear_beam": unclear_beam}


# ---- every beam x candidate count the kernel takes, with the frames that make it take its other paths --------------------------------
GRID_BEAMS, GRID_KS, GRID_SEEDS, GRID_T, GRID_V, GRID_SPREAD = (1, 2, 8, 16), (0, 1, 3, 8), list(range(2000, 2010)), 20, 12, 3.0
GRID_EMPTY_FRAMES, GRID_INF_FRAME = (5, 6), 9


def grid_case(beam, k):
    """flat lists of GRID_T frames (the first frames hold fewer live prefixes than the beam; 16 x 8 fills the 144-entry pool) in which
    frames GRID_EMPTY_FRAMES have no candidate but the blank (ids -1, lp -inf) and frame GRID_INF_FRAME gives its first candidate the
    log-probability -inf -> the dict of case()"""
    key = ("grid", beam, k)
    if key not in _MADE:
        lists = [flat_lists(GRID_T, GRID_V, k, GRID_SPREAD, seed) for seed in GRID_SEEDS]
        ids, lp = torch.stack([i for i, _ in lists]), torch.stack([l for _, l in lists])
        for t in GRID_EMPTY_FRAMES:
            ids[:, t, 1:], lp[:, t, 1:] = -1, NEG
        if k:
            lp[:, GRID_INF_FRAME, 1] = NEG
        _MADE[key] = _with_reference(ids, lp, beam)
    return _MADE[key]


def ragged_case():
    """the lists of peaky_T70_V12_k8_beam16 cut to ragged_lengths -> the dict of case() for the cut lists"""
    if "ragged" not in _MADE:
        c = case("peaky_T70_V12_k8_beam16")
        _MADE["ragged"] = _with_reference(c["ids"], c["lp"], c["beam"], ragged_lengths(c["T"], c["ids"].size(0)))
    return _MADE["ragged"]


def reentry_events(ids, lp, beam):
    """prefix_beam_ref's frame loop with the beam's history watched -> (merges, re-entry merges): extensions added to a beam entry, and
    those among them whose target had been in the beam WITHOUT its parent at some frame since it came in (the parent left, and is back
    as a fresh extension)"""
    hyps = [((), 0.0, NEG)]
    orphaned = set()                       # beam entries that have seen a frame without their parent in the beam
    merges = back = 0
    for t in range(len(ids)):
        pool = {}
        for l, pb, pnb in hyps:
            stay_nb = NEG
            if l:
                for j in range(1, len(ids[t])):
                    if ids[t][j] == l[-1]:
                        stay_nb = pnb + lp[t][j]
            pool[l] = [br.lae(pb, pnb) + lp[t][0], stay_nb]
        for l, pb, pnb in hyps:
            for j in range(1, len(ids[t])):
                c = ids[t][j]
                if c < 0:
                    continue
                v = (pb if l and c == l[-1] else br.lae(pb, pnb)) + lp[t][j]
                key = l + (c,)
                if key in pool:
                    merges += 1
                    back += key in orphaned
                    pool[key][1] = br.lae(pool[key][1], v)
                else:
                    pool[key] = [NEG, v]
        items = [(l, b, nb) for l, (b, nb) in pool.items() if br.lae(b, nb) > NEG]
        items.sort(key=lambda it: -br.lae(it[1], it[2]))
        hyps = items[:beam]
        now = {l for l, _, _ in hyps}
        orphaned = {l for l in now if l and (l in orphaned or l[:-1] not in now)}
    return merges, back


def ragged_lengths(T, B):
    """[T, 0, 1, 17, T - 1, ...]: full, empty, one frame, a length inside the first staged block, one short of full, then a spread"""
    head = [T, 0, 1, min(17, T), T - 1]
    return (head + [(7 * i + 3) % (T + 1) for i in range(B)])[:B]
