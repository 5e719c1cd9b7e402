"""The batched edit distance on the MI355X (csrc/edit_distance.hip: simulst_edit_distance, behind
simulst_amd.edit_distance) against tests/edit_distance_ref.py.  Everything is an integer, so every
comparison is equality: the four counts of every pair, and the alignment operation by operation.

The length grid {0, 1, 2, 63, 64, 65, 127, 128, 129, 1022, 1023} sits on the kernel's edges: a hypothesis is laid over the 64 lanes of a
wave in strips of 64 columns (one strip, its last lane, the first lane of the second, two strips, sixteen), the reference feeds the
wavefront one label a step, and 1023 is the label limit.  Alphabet 4 makes nearly every cell a tie between predecessors, alphabet 4096
nearly none."""
import random

import pytest
import torch

import edit_distance_ref as er

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 1022, 1023)


@pytest.fixture(scope="module")
def ops():
    from simulst_amd.ops import Ops
    return Ops()


def _pack(strings, width=None, fill=-7):
    """label strings -> (int64 [n, width] with `fill` behind each length, int64 [n] lengths)"""
    width = max([len(s) for s in strings] + [1]) if width is None else width
    t = torch.full((len(strings), width), fill, dtype=torch.int64)
    for n, s in enumerate(strings):
        t[n, :len(s)] = torch.tensor(list(s), dtype=torch.int64)
    return t, torch.tensor([len(s) for s in strings], dtype=torch.int64)


def _rand(rng, n, alphabet):
    return [rng.randrange(alphabet) for _ in range(n)]


def _run(ops, refs, hyps, **kw):
    from simulst_amd.edit_distance import edit_distance
    r, rl = _pack(refs)
    h, hl = _pack(hyps)
    out = edit_distance(ops, r.to(DEV), rl.to(DEV), h.to(DEV), hl.to(DEV), **kw)
    torch.cuda.synchronize()
    return tuple(x.cpu() for x in out) if isinstance(out, tuple) else out.cpu()


_REF = {}


def _expect(r, h):
    key = (tuple(r), tuple(h))
    if key not in _REF:
        _REF[key] = er.align(r, h)
    return _REF[key]


def _check_batch(ops, refs, hyps):
    """counts-only and path launches of the pairs (refs[p], hyps[p]) against the reference, pair by pair"""
    counts_only = _run(ops, refs, hyps)
    counts, path, n_ops = _run(ops, refs, hyps, path=True)
    assert torch.equal(counts_only, counts)                                   # the path changes no count
    assert counts.dtype == torch.int32 and path.dtype == torch.int8 and n_ops.dtype == torch.int32
    for p, (r, h) in enumerate(zip(refs, hyps)):
        want, want_ops = _expect(r, h)
        assert tuple(counts[p].tolist()) == want, (len(r), len(h), counts[p].tolist(), want)
        n = int(n_ops[p])
        assert n == len(want_ops) == len(r) + want[3]
        assert path[p, :n].tolist() == want_ops, (len(r), len(h))
        assert bool((path[p, n:] == -1).all())


# ---------------------------------------------------------------- lane and register edges
def test_all_121_length_pairs_at_alphabet_4(ops):
    rng = random.Random(20240)
    refs, hyps = [], []
    for lr in LENS:
        for lh in LENS:
            refs.append(_rand(rng, lr, 4))
            hyps.append(_rand(rng, lh, 4))
    assert len(refs) == 121
    _check_batch(ops, refs, hyps)


def test_a_sample_of_length_pairs_at_alphabet_4096(ops):
    rng = random.Random(20241)
    sample = [(1023, 1023), (1022, 1023), (1023, 64), (65, 1023), (0, 1023), (1023, 0), (63, 64), (64, 63), (64, 64), (65, 65), (127, 129),
              (129, 127), (128, 128), (1, 65), (2, 1), (0, 0), (1, 1)]
    refs, hyps = [], []
    for lr, lh in sample:
        r = _rand(rng, lr, 4096)
        # a hypothesis that shares long runs with the reference (else every cell is a substitution), with its own labels between
        h = [r[q] if q < lr and rng.random() < 0.8 else rng.randrange(4096) for q in range(lh)]
        refs.append(r)
        hyps.append(h)
    _check_batch(ops, refs, hyps)


def test_adversarial_ties(ops):
    base = _rand(random.Random(20242), 130, 5)
    refs = [[3] * 129, [3] * 65, [3] * 1023, base[1:], base[:-1], [0, 1, 2] * 43, [0, 1, 2], [0, 1] * 64, [1, 0] * 64, [7] * 64]
    hyps = [[3] * 65, [3] * 129, [3] * 1022, base[:-1], base[1:], [0, 1, 2], [0, 1, 2] * 43, [1, 0] * 64, [0, 1] * 64, [8] * 64]
    _check_batch(ops, refs, hyps)


def test_labels_are_compared_as_int64(ops):
    """labels that differ only above bit 31, and negative ones"""
    big = 1 << 40
    refs = [[5, big + 5, -1, 6], [big, big, big]]
    hyps = [[5, 5, -1, (1 << 32) + 6], [big, 0, big]]
    _check_batch(ops, refs, hyps)
    assert _run(ops, refs, hyps)[:, 0].tolist() == [2, 1]


def test_int32_ops(ops):
    refs, hyps = [list(b"kitten"), []], [list(b"sitting"), [4, 4]]
    counts, path, n_ops = _run(ops, refs, hyps, path=True, ops_dtype=torch.int32)
    assert path.dtype == torch.int32 and counts.tolist() == [[3, 2, 0, 1], [2, 0, 0, 2]]
    assert path[0, :7].tolist() == [1, 0, 0, 0, 1, 0, 3] and path[1, :2].tolist() == [3, 3] and n_ops.tolist() == [7, 2]
    assert bool((path[0, 7:] == -1).all()) and bool((path[1, 2:] == -1).all())


# ---------------------------------------------------------------- index indirection
def test_pairs_by_scrambled_indices_with_repeats(ops):
    from simulst_amd.edit_distance import edit_distance
    rng = random.Random(20243)
    refs = [_rand(rng, n, 4) for n in (40, 0, 70)]
    hyps = [_rand(rng, n, 4) for n in (66, 35, 0, 64, 9)]
    ri = [2, 0, 0, 1, 2, 2, 0, 1, 0]
    hi = [4, 0, 3, 1, 4, 2, 0, 2, 1]
    r, rl = _pack(refs)
    h, hl = _pack(hyps)
    counts, path, n_ops = edit_distance(ops, r.to(DEV), rl.to(DEV), h.to(DEV), hl.to(DEV), ref_idx=torch.tensor(ri, dtype=torch.int32, device=DEV),
                                        hyp_idx=torch.tensor(hi, dtype=torch.int32, device=DEV), path=True)
    for p, (a, b) in enumerate(zip(ri, hi)):
        want, want_ops = _expect(refs[a], hyps[b])
        assert tuple(counts[p].tolist()) == want and path[p, :int(n_ops[p])].tolist() == want_ops
    # indices the host holds are refused before a launch; indices on the device mark the pair
    with pytest.raises(ValueError):
        edit_distance(ops, r.to(DEV), rl.to(DEV), h.to(DEV), hl.to(DEV), ref_idx=[0, 3], hyp_idx=[0, 0])
    got = edit_distance(ops, r.to(DEV), rl.to(DEV), h.to(DEV), hl.to(DEV), ref_idx=torch.tensor([0, 3, -1, 2], dtype=torch.int32, device=DEV),
                        hyp_idx=torch.tensor([5, 0, 0, 1], dtype=torch.int32, device=DEV)).cpu()
    assert got[:3].tolist() == [[-1] * 4] * 3 and tuple(got[3].tolist()) == _expect(refs[2], hyps[1])[0]


def test_null_indices_are_the_identity_and_unnamed_rows_keep_a_sentinel(ops):
    rng = random.Random(20244)
    strings = [_rand(rng, n, 4) for n in (30, 64, 65, 1, 0, 100)]
    others = [_rand(rng, n, 4) for n in (33, 60, 70, 0, 2, 90)]
    r, rl = _pack(strings)
    h, hl = _pack(others)
    r, rl, h, hl = r.to(DEV), rl.to(DEV), h.to(DEV), hl.to(DEV)
    ident = torch.arange(6, dtype=torch.int32, device=DEV)
    a = ops.edit_distance(r, rl, h, hl, path=True, pad=-1)
    b = ops.edit_distance(r, rl, h, hl, ref_idx=ident, hyp_idx=ident, path=True, pad=-1)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # the output of 4 pairs lives inside larger sentinel buffers: the kernel writes its rows and nothing else.  Rows 2 and 4 of either
    # side are named by no pair: the strings are read-only, so what can be held is that the inputs are unchanged
    keep = [t.clone() for t in (r, rl, h, hl)]
    sub = torch.tensor([0, 1, 3, 5], dtype=torch.int32, device=DEV)
    c = ops.edit_distance(r, rl, h, hl, ref_idx=sub, hyp_idx=sub).cpu()
    assert torch.equal(c, a[0].cpu()[[0, 1, 3, 5]])
    assert all(torch.equal(x, y) for x, y in zip(keep, (r, rl, h, hl)))
    # a length above a row's capacity would read past the row: the pair is marked instead (row 2's length is a sentinel no pair reads)
    rl_bad = rl.clone()
    rl_bad[2] = 10 ** 9
    c2 = ops.edit_distance(r, rl_bad, h, hl, ref_idx=sub, hyp_idx=sub).cpu()
    assert torch.equal(c2, c)
    c3 = ops.edit_distance(r, rl_bad, h, hl).cpu()
    assert c3[2].tolist() == [-1] * 4 and torch.equal(c3[[0, 1, 3, 4, 5]], a[0].cpu()[[0, 1, 3, 4, 5]])


def test_one_buffer_as_both_sides(ops):
    from simulst_amd.edit_distance import edit_distance
    rng = random.Random(20245)
    strings = [_rand(rng, n, 3) for n in (20, 66, 0, 64)]
    t, tl = _pack(strings)
    t, tl = t.to(DEV), tl.to(DEV)
    ri = torch.arange(4, dtype=torch.int32, device=DEV).repeat_interleave(4)
    hi = torch.arange(4, dtype=torch.int32, device=DEV).repeat(4)
    counts = edit_distance(ops, t, tl, t, tl, ref_idx=ri, hyp_idx=hi).cpu().view(4, 4, 4)
    for a in range(4):
        for b in range(4):
            assert tuple(counts[a, b].tolist()) == _expect(strings[a], strings[b])[0]
            # symmetric; del and ins swap whenever the two directions' paths have the same substitutions (each is ITS rule's path)
            assert counts[a, b, 0] == counts[b, a, 0] and counts[a, b, 2] - counts[a, b, 3] == counts[b, a, 3] - counts[b, a, 2]
        assert counts[a, a].tolist() == [0, 0, 0, 0]


# ---------------------------------------------------------------- independence
def test_a_pair_does_not_depend_on_its_place_or_on_the_path(ops):
    rng = random.Random(20246)
    r0, h0 = _rand(rng, 97, 4), _rand(rng, 110, 4)
    alone = _run(ops, [r0], [h0], path=True)
    alone_counts = _run(ops, [r0], [h0])
    assert torch.equal(alone_counts, alone[0]) and tuple(alone[0][0].tolist()) == _expect(r0, h0)[0]
    refs = [_rand(rng, rng.randrange(30, 111), 4) for _ in range(300)]
    hyps = [_rand(rng, rng.randrange(30, 111), 4) for _ in range(300)]
    for at in (0, 1, 299):
        refs[at], hyps[at] = r0, h0
    # (the same widths as the single pair's launch would have been a different capacity: the result may not depend on that either)
    batch = _run(ops, refs, hyps, path=True)
    batch_counts = _run(ops, refs, hyps)
    assert torch.equal(batch_counts, batch[0])
    n = int(alone[2][0])
    for at in (0, 1, 299):
        assert torch.equal(batch[0][at], alone[0][0]) and int(batch[2][at]) == n
        assert torch.equal(batch[1][at, :n], alone[1][0, :n]) and bool((batch[1][at, n:] == -1).all())
    for p in (2, 150, 298):
        assert tuple(batch[0][p].tolist()) == _expect(refs[p], hyps[p])[0]


def test_counts_only_runs_with_a_null_scratch(ops):
    """the raw call: no ops, no n_ops, no back-pointer scratch in the descriptor"""
    import ctypes
    from simulst_amd import _lib
    r, rl = _pack([list(b"kitten"), list(b"flaw")])
    h, hl = _pack([list(b"sitting"), list(b"lawn")])
    r, rl, h, hl = r.to(DEV), rl.to(DEV), h.to(DEV), hl.to(DEV)
    counts = torch.full((3, 4), -99, dtype=torch.int32, device=DEV)
    d = _lib.EditDesc()
    d.hyp, d.hyp_stride_b, d.n_ref, d.n_hyp, d.counts = h.data_ptr(), h.stride(0), 2, 2, counts.data_ptr()
    vp = ctypes.c_void_p
    rc = ops.lib.simulst_edit_distance(ops.h.ptr, vp(r.data_ptr()), r.stride(0), vp(rl.data_ptr()), vp(hl.data_ptr()), r.size(1), h.size(1),
                                       2, ctypes.byref(d), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [[3, 2, 0, 1], [2, 0, 1, 1], [-99] * 4]


def test_composed_form_gives_the_same_integers(ops):
    from simulst_amd.edit_distance import edit_distance
    rng = random.Random(20247)
    refs = [_rand(rng, rng.choice((0, 1, 30, 64, 65, 110)), 4) for _ in range(40)]
    hyps = [_rand(rng, rng.choice((0, 1, 30, 64, 65, 110)), 4) for _ in range(40)]
    r, rl = _pack(refs)
    h, hl = _pack(hyps)
    a = edit_distance(ops, r.to(DEV), rl.to(DEV), h.to(DEV), hl.to(DEV), path=True)
    b = edit_distance(ops, r.to(DEV), rl.to(DEV), h.to(DEV), hl.to(DEV), path=True, composed=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and a[0].is_cuda and b[0].is_cuda
    # above 1023 labels the torch form answers
    long_r, long_h = _rand(rng, 1030, 4), _rand(rng, 1025, 4)
    c = _run(ops, [long_r], [long_h])
    assert tuple(c[0].tolist()) == _expect(long_r, long_h)[0]


# ---------------------------------------------------------------- surface
def _host_oracle(refs, lists):
    out = []
    for r, hs in zip(refs, lists):
        d = [_expect(r, h)[0] for h in hs]
        k = min(range(len(hs)), key=lambda q: (d[q][0], q))
        out.append((k, d[k], d))
    return out


def test_oracle_error_of_a_16_best_list(ops):
    from simulst_amd.edit_distance import oracle_error
    rng = random.Random(20248)
    refs = [_rand(rng, n, 6) for n in (50, 31, 0, 80)]
    lists = []
    for r in refs:
        hs = []
        for _ in range(16):
            h = [x for x in r if rng.random() > 0.1]
            for _ in range(rng.randrange(4)):
                h.insert(rng.randrange(len(h) + 1), rng.randrange(6))
            hs.append(h)
        hs[9] = list(hs[4])                                   # an exact tie between two entries: the lower index wins
        lists.append(hs)
    r, rl = _pack(refs)
    W = max(len(h) for hs in lists for h in hs)
    nb = torch.stack([_pack(hs, W)[0] for hs in lists])
    nl = torch.stack([_pack(hs, W)[1] for hs in lists])
    idx, best, allc = oracle_error(r.to(DEV), rl.to(DEV), nb.to(DEV), nl.to(DEV), ops=ops)
    for b, (k, dk, d) in enumerate(_host_oracle(refs, lists)):
        assert int(idx[b]) == k and tuple(best[b].tolist()) == dk
        assert [tuple(x) for x in allc[b].tolist()] == d


def _host_mbr(lists, scores):
    import math
    out = []
    for hs, sc in zip(lists, scores):
        m = max(sc)
        w = [math.exp(s - m) for s in sc]
        z = math.fsum(w)
        risk = [math.fsum(w[j] / z * _expect(hs[i], hs[j])[0][0] for j in range(len(hs))) for i in range(len(hs))]
        out.append(risk)
    return out


def test_mbr_select_clear_gaps_and_an_exact_tie(ops):
    from simulst_amd.edit_distance import mbr_select
    rng = random.Random(20249)
    lists, scores = [], []
    for b in range(3):
        centre = _rand(rng, 40 + 10 * b, 8)
        hs = [list(centre)]
        for _ in range(7):
            h = list(centre)
            for _ in range(rng.randrange(2, 9)):
                h[rng.randrange(len(h))] = rng.randrange(8)
            hs.append(h)
        rng.shuffle(hs)
        lists.append(hs)
        scores.append([-0.37 * q - 0.011 * rng.random() for q in range(8)])
    # the constructed tie: two mirrored strings with equal scores and nothing else of weight -> equal risks in every bit, lower index wins
    a = _rand(rng, 20, 8)
    lists.append([a[::-1], a, a[::-1], a] + [_rand(rng, 20, 8) for _ in range(4)])
    scores.append([0.0, 0.0, float("-inf"), float("-inf")] + [float("-inf")] * 4)
    W = max(len(h) for hs in lists for h in hs)
    nb = torch.stack([_pack(hs, W)[0] for hs in lists]).to(DEV)
    nl = torch.stack([_pack(hs, W)[1] for hs in lists]).to(DEV)
    sc = torch.tensor(scores, dtype=torch.float32, device=DEV)
    idx, risk = mbr_select(nb, nl, sc, ops=ops)
    idx, risk = idx.cpu(), risk.cpu()
    assert risk.dtype == torch.float64
    want = _host_mbr(lists, [[float(x) for x in torch.tensor(s, dtype=torch.float32).tolist()] for s in scores])
    for b in range(3):
        order = sorted(range(8), key=lambda q: want[b][q])
        assert want[b][order[1]] - want[b][order[0]] >= 1e-3, "the case must have a clear winner"
        assert int(idx[b]) == order[0]
        # the risks are sums of 8 products of a weight in [0, 1] and an integer distance <= 70: 1e-9 covers fp64 summation order
        assert max(abs(float(risk[b, q]) - want[b][q]) for q in range(8)) <= 1e-9
    assert float(risk[3, 0]) == float(risk[3, 1]) and int(idx[3]) == 0
    assert bool(torch.isinf(risk[3, 2:]).all())


def test_token_error_report_over_ctc_collapse_output(ops):
    from simulst_amd.ctc import ctc_collapse, token_error_report
    g = torch.Generator().manual_seed(20250)
    B, T = 9, 150
    path = torch.randint(0, 5, (B, T), generator=g)                          # label 0 is the blank; runs of equal labels collapse
    lengths = torch.tensor([150, 149, 1, 0, 77, 130, 64, 65, 100])
    tokens, n, _ = ctc_collapse(path.to(DEV), lengths.to(DEV))
    rng = random.Random(20250)
    targets = [_rand(rng, k, 5) for k in (70, 0, 1, 3, 64, 65, 40, 90, 63)]
    tgt, tl = _pack(targets, fill=1)
    rep = token_error_report(tokens, n, tgt.to(DEV), tl.to(DEV), ops=ops)
    assert all(v.is_cuda and v.dtype == torch.int64 and v.dim() == 0 for v in rep.values())
    tokens, n = tokens.cpu(), n.cpu()
    want = [0, 0, 0, 0]
    for b in range(B):
        c = _expect(targets[b], tokens[b, :int(n[b])].tolist())[0]
        want = [x + y for x, y in zip(want, c)]
    assert [int(rep[k]) for k in ("errors", "sub", "del", "ins")] == want
    assert int(rep["ref_labels"]) == sum(len(t) for t in targets) and want[0] > 0


def test_evaluate_wer_on_the_tiny_model():
    """the model's own beam-5 hypotheses with a scripted corruption as references: word counters against a host WerScorer fed the same
    strings, token counters against the reference over the same token lists"""
    from simulst_amd.config import tiny
    from simulst_amd.harness import Dictionary, WerScorer
    from simulst_amd.model import S2TEmformerModel
    from simulst_amd.weights import init_model
    cfg = tiny(model="s2t_emformer", simul_attn_type="full", ctc_layer=True, mass_preservation=False)
    w = init_model(cfg, seed=31)
    g = torch.Generator().manual_seed(32)
    W = torch.randn(cfg.vocab, cfg.embed_dim, generator=g) * cfg.embed_dim ** -0.5
    W[cfg.eos] *= 3.0
    w["decoder.output_projection.weight"] = W                                # untied, EOS reachable (tests/test_hip_joint_ctc_beam.py)
    w["encoder.ctc_layer.weight"] = torch.randn(cfg.vocab, cfg.embed_dim, generator=g) * 4.0 * cfg.embed_dim ** -0.5
    frames = [150, 96, 56]
    fb = torch.randn(3, 150, 80, generator=torch.Generator().manual_seed(33))
    for b, f in enumerate(frames):
        fb[b, f:] = 0
    T = torch.tensor(frames)
    model = S2TEmformerModel(cfg, w, device="cuda:0")
    # every third label opens a word, as a sentencepiece dictionary's would
    tgt_dict = Dictionary([("▁" if v % 3 == 0 else "") + f"u{v}" for v in range(cfg.vocab)], eos_index=cfg.eos)
    for lam in (0.0, 0.3):
        hyp = [h[0]["tokens"].tolist() for h in model.generate(fb.to(DEV), T, beam=5, ctc_weight=lam)]
        hyp = [t[:-1] if t and t[-1] == cfg.eos else t for t in hyp]
        assert all(len(t) >= 3 for t in hyp)
        refs = []
        for b, t in enumerate(hyp):                                          # drop a label, change one, append one
            r = list(t)
            del r[1 + b % 2]
            r[0] = (r[0] + 3) % cfg.vocab if (r[0] + 3) % cfg.vocab not in (cfg.eos, cfg.padding_idx) else 5
            refs.append(r + [7, cfg.eos])
        out = model.evaluate_wer(fb.to(DEV), T, refs, tgt_dict, beam=5, ctc_weight=lam)
        host = WerScorer(device=None)
        want_tok = [0, 0, 0, 0]
        for b in range(3):
            ref_toks = [x for x in refs[b] if x != cfg.eos]
            assert out["hyps"][b] == tgt_dict.string(hyp[b], "sentencepiece") and out["refs"][b] == tgt_dict.string(ref_toks, "sentencepiece")
            host.add_string(out["refs"][b], out["hyps"][b])
            want_tok = [x + y for x, y in zip(want_tok, _expect(ref_toks, hyp[b])[0])]
        assert (out["w_errors"], out["wv_errors"], out["w_total"]) == (host.distance, host.distance, host.ref_length)
        assert 0 < out["w_errors"] and out["w_total"] > 0
        assert [int(out[k]) for k in ("t_errors", "t_sub", "t_del", "t_ins")] == want_tok and out["t_errors"].is_cuda
        assert int(out["t_total"]) == sum(len(r) - 1 for r in refs) and 0 < want_tok[0] < int(out["t_total"])
