"""CPU-side checks of the error-rate work: the reference of tests/edit_distance_ref.py against exhaustive enumeration, known answers
and identities; the composed (host) form of simulst_amd.edit_distance against it; harness.WerScorer / corpus_wer / corpus_scores;
simulst_edit_distance at the ABI (declared, refusals made before any launch on host buffers); sharding.reduce_error_counts under two gloo ranks.  Everything compared is an integer: every assertion is equality."""
import ctypes
import os
import random
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import abi_pins
import edit_distance_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE = -1, -2


def _rand(rng, n, alphabet):
    return [rng.randrange(alphabet) for _ in range(n)]


# ---------------------------------------------------------------- the reference itself
def _check_against_enumeration(r, h):
    counts, ops = er.align_plain(r, h)
    assert counts[0] == er.min_cost(tuple(r), tuple(h))                    # minimal over ALL alignments
    assert ops == er.rule_path(r, h)                                       # and the path is the rule's
    assert tuple(ops) in set(er.enumerate_alignments(r, h)) and er.cost(ops) == counts[0]


def test_reference_against_exhaustive_enumeration():
    """every pair of strings of <= 3 labels over 3 labels (1600 pairs), and 400 seeded pairs of <= 5 labels (a 5 x 5 pair has 1683
    alignments; all 132 496 pairs of that size would take minutes)"""
    short = list(er.all_strings(3, 3))
    assert len(short) == 40
    for r in short:
        for h in short:
            _check_against_enumeration(r, h)
    longer = list(er.all_strings(3, 5))
    assert len(longer) == 364
    rng = random.Random(5)
    for _ in range(400):
        _check_against_enumeration(rng.choice(longer), rng.choice(longer))


def test_known_answers():
    assert er.align_plain("kitten", "sitting") == ((3, 2, 0, 1), [1, 0, 0, 0, 1, 0, 3])
    assert er.align_plain("", "") == ((0, 0, 0, 0), [])
    assert er.align_plain("", "abc") == ((3, 0, 0, 3), [3, 3, 3])
    assert er.align_plain("abcd", "") == ((4, 0, 4, 0), [2, 2, 2, 2])
    assert er.align_plain("simul", "simul") == ((0, 0, 0, 0), [0] * 5)
    # disjoint strings of unequal length: the shorter one's labels are all substituted, the rest deleted / inserted
    assert er.align_plain("abcde", "xy")[0] == (5, 2, 3, 0)
    assert er.align_plain("xy", "abcde")[0] == (5, 2, 0, 3)
    # where the tie rule shows
    assert er.align_plain("ab", "ba") == ((2, 2, 0, 0), [1, 1])          # two substitutions, not delete + insert
    assert er.align_plain("a", "aa") == ((1, 0, 0, 1), [3, 0])           # the LAST a is matched: the diagonal comes first at (1, 2)


def test_plain_and_antidiagonal_forms_agree():
    rng = random.Random(6)
    for _ in range(150):
        a = rng.choice((2, 4, 4096))
        r, h = _rand(rng, rng.randrange(0, 40), a), _rand(rng, rng.randrange(0, 40), a)
        assert er.align_plain(r, h) == er.align(r, h)


def test_identities_on_random_pairs():
    rng = random.Random(7)
    for _ in range(120):
        a = rng.choice((2, 3, 50))
        r, h, g = (_rand(rng, rng.randrange(0, 30), a) for _ in range(3))
        (d, s, dl, ins), ops = er.align(r, h)
        assert d == s + dl + ins and len(h) == len(r) - dl + ins and len(ops) == len(r) + ins
        assert er.replay(r, h, ops)                                        # consumes both exactly; 0 joins equal, 1 unequal labels
        back = er.align(h, r)[0]
        assert back[0] == d                                                # symmetric
        # del and ins swap between the two directions whenever the substitutions agree (both alignments are optimal, but the rule
        # may pick paths with different numbers of substitutions; Lh - Lr = ins - del holds for each)
        assert back[3] - back[2] == dl - ins
        if back[1] == s:
            assert (back[2], back[3]) == (ins, dl)
        assert er.align(r, g)[0][0] <= d + er.align(h, g)[0][0]            # the triangle inequality
    assert not er.replay([1, 2], [1, 3], [0, 0]) and not er.replay([1], [1, 1], [0])


# ---------------------------------------------------------------- the composed form
def _pack(strings, width=None):
    width = max([len(s) for s in strings] + [1]) if width is None else width
    t = torch.full((len(strings), width), -7, dtype=torch.int64)
    for n, s in enumerate(strings):
        t[n, :len(s)] = torch.tensor(list(s), dtype=torch.int64)
    return t, torch.tensor([len(s) for s in strings], dtype=torch.int64)


def test_composed_form_equals_the_reference():
    from simulst_amd.edit_distance import edit_distance
    rng = random.Random(8)
    refs = [_rand(rng, rng.choice((0, 1, 2, 17, 64, 65, 90)), rng.choice((2, 4, 4096))) for _ in range(60)]
    hyps = [_rand(rng, rng.choice((0, 1, 2, 17, 64, 65, 90)), 4) for _ in range(60)]
    r, rl = _pack(refs)
    h, hl = _pack(hyps)
    for kw in ({}, {"composed": True}):                                    # CPU tensors take the composed form either way
        counts, ops, n_ops = edit_distance(None, r, rl, h, hl, path=True, **kw)
        assert counts.dtype == torch.int32 and ops.dtype == torch.int8 and ops.shape == (60, r.size(1) + h.size(1))
        for p in range(60):
            want, want_ops = er.align(refs[p], hyps[p])
            assert tuple(counts[p].tolist()) == want
            assert ops[p, :int(n_ops[p])].tolist() == want_ops and bool((ops[p, int(n_ops[p]):] == -1).all())
        assert torch.equal(edit_distance(None, r, rl, h, hl, **kw), counts)
    # pairs by index; one buffer on both sides; a host index out of range is refused, one on a tensor marks its pair
    ri, hi = [3, 3, 0, 59], [0, 3, 3, 58]
    got = edit_distance(None, r, rl, r, rl, ref_idx=ri, hyp_idx=hi)
    assert [tuple(x) for x in got.tolist()] == [er.align(refs[a], refs[b])[0] for a, b in zip(ri, hi)]
    with pytest.raises(ValueError):
        edit_distance(None, r, rl, h, hl, ref_idx=[0, 60], hyp_idx=[0, 0])
    # strings above the kernel's 1023 labels
    long_r, long_h = _rand(rng, 1100, 3), _rand(rng, 1050, 3)
    a, al = _pack([long_r])
    b, bl = _pack([long_h])
    assert tuple(edit_distance(None, a, al, b, bl)[0].tolist()) == er.align(long_r, long_h)[0]


def test_oracle_error_and_mbr_select_on_the_host():
    from simulst_amd.edit_distance import mbr_select, oracle_error
    ref, rl = _pack([[1, 2, 3, 4], [5, 6]])
    lists = [[[1, 2, 4], [1, 2, 3, 4, 4], [9, 2, 3, 4]], [[6, 5], [5], [5, 6, 7]]]
    nb = torch.stack([_pack(hs, 5)[0] for hs in lists])
    nl = torch.stack([_pack(hs, 5)[1] for hs in lists])
    idx, best, allc = oracle_error(ref, rl, nb, nl)
    assert idx.tolist() == [0, 1] and best.tolist() == [[1, 0, 1, 0], [1, 0, 1, 0]]       # three-way / two-way ties: the lower index
    assert allc[:, :, 0].tolist() == [[1, 1, 1], [2, 1, 1]]
    idx, risk = mbr_select(nb, nl, torch.zeros(2, 3))
    d0 = [[0, 2, 2], [2, 0, 2], [2, 2, 0]]
    assert [er.align(a, b)[0][0] for a in lists[0] for b in lists[0]] == sum(d0, [])
    assert risk.dtype == torch.float64 and idx[0] == 0                                     # all risks 4/3: the lower index
    assert float(risk[0, 0]) == float(risk[0, 1]) == float(risk[0, 2])


# ---------------------------------------------------------------- the scorer
def test_wer_scorer_on_hand_written_sentences():
    from simulst_amd.harness import WerScorer
    s = WerScorer()
    s.add_string("the cat sat on the mat", "the cat sat on mat")               # one deletion
    s.add_string("hello world", "hello there world")                           # one insertion
    assert (s.distance, s.ref_length) == (2, 8) and s.score() == 25.0 and s.result_string() == "WER: 25.00"
    assert s.counts == {"errors": 2, "sub": 0, "del": 1, "ins": 1, "ref_words": 8}
    s.add_string("a b", "")                                                    # an empty hypothesis: every word deleted
    assert (s.distance, s.ref_length) == (4, 10)
    s.reset()
    assert s.score() == 0 and s.ref_length == 0
    # case counts unless lowercased
    a, b = WerScorer(), WerScorer(wer_lowercase=True)
    for x in (a, b):
        x.add_string("Hello World", "hello world")
    assert (a.distance, b.distance) == (2, 0)
    # punctuation: tokens made ONLY of category-P characters go; "mat." stays a word of its own
    a, b = WerScorer(), WerScorer(wer_remove_punct=True)
    for x in (a, b):
        x.add_string("well , the mat . « yes »", "well the mat. yes !")
    assert (a.distance, a.ref_length) == (5, 8)
    assert (b.distance, b.ref_length) == (1, 4)
    # characters: a space is a token of its own (U+2581)
    c = WerScorer(wer_char_level=True)
    assert c.tokenize("ab c") == ["a", "b", "▁", "c"]
    c.add_string("ab c", "abc")
    assert (c.distance, c.ref_length) == (1, 4)
    with pytest.raises(NotImplementedError, match="sacrebleu"):
        WerScorer(wer_tokenizer="13a")
    # device=None and a machine without a GPU take the composed form: the same numbers
    d = WerScorer(device=None)
    d.add_string("x y z", "x z")
    assert d.distance == 1


def test_corpus_wer_and_corpus_scores():
    from simulst_amd.harness import corpus_scores, corpus_wer
    hyps, refs = ["the cat sat", "a dog"], ["the cat sat down", "A dog barks"]
    assert corpus_wer(hyps, refs) == 100.0 * 3 / 7
    assert corpus_wer(hyps, refs, wer_lowercase=True) == 100.0 * 2 / 7
    lat = {k: 1.0 for k in ("AL", "AL_CA", "AP", "AP_CA", "DAL", "DAL_CA")}
    inst = [{"prediction": h, "metric": {"latency": lat}} for h in hyps]
    plain = corpus_scores(inst, refs)
    assert "WER" not in plain["Quality"] and set(plain["Quality"]) == {"BLEU"}
    with_wer = corpus_scores(inst, refs, wer=True, wer_lowercase=True)
    assert with_wer["Quality"]["WER"] == 100.0 * 2 / 7 and with_wer["Quality"]["BLEU"] == plain["Quality"]["BLEU"]
    assert with_wer["Latency"] == plain["Latency"]
    with pytest.raises(ValueError):
        corpus_scores(inst, None, wer=True)


def test_token_error_report_on_the_host():
    from simulst_amd.ctc import ctc_collapse, token_error_report
    path = torch.tensor([[0, 5, 5, 0, 6, 7, 7, 0], [4, 4, 0, 4, 9, 9, 9, 9]])
    tokens, n, _ = ctc_collapse(path, torch.tensor([8, 6]))
    assert [tokens[b, :int(n[b])].tolist() for b in range(2)] == [[5, 6, 7], [4, 4, 9]]
    tgt, tl = _pack([[5, 7], [4, 8, 4, 9]])
    rep = token_error_report(tokens, n, tgt, tl)
    want = [sum(x) for x in zip(er.align([5, 7], [5, 6, 7])[0], er.align([4, 8, 4, 9], [4, 4, 9])[0])]
    assert [int(rep[k]) for k in ("errors", "sub", "del", "ins")] == want == [2, 0, 1, 1] and int(rep["ref_labels"]) == 6
    assert all(v.dtype == torch.int64 and v.dim() == 0 for v in rep.values())


# ---------------------------------------------------------------- the ABI
@pytest.fixture
def handle():
    from simulst_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.simulst_create(ctypes.byref(h), None) == 0
    yield lib, h
    assert lib.simulst_destroy(h) == 0


def test_descriptor_is_declared_and_nothing_else_moved():
    from simulst_amd import _lib
    d = _lib.EditDesc
    assert ctypes.sizeof(d) == 88
    names = ("hyp", "hyp_stride_b", "ref_idx", "hyp_idx", "n_ref", "n_hyp", "counts", "n_ops", "bp", "bp_bytes", "ops_cap", "ops_width",
             "pad", "reserved")
    assert [getattr(d, n).offset for n in names] == [0, 8, 16, 24, 32, 36, 40, 48, 56, 64, 72, 76, 80, 84]
    header = open(os.path.join(ROOT, "include", "simulst_hip.h")).read()
    assert "} simulst_edit_desc;" in header and "SIMULST_EDIT_BP_BYTES" in header
    assert _lib.edit_bp_bytes(3, 1023, 1023) == 3 * 16 * 1086 * 64 and _lib.edit_bp_bytes(1, 10, 64) == 73 * 64
    assert len(_lib.SIGNATURES) == abi_pins.N_SIGNATURES
    assert _lib.load().simulst_version() == abi_pins.VERSION == _lib.ABI_VERSION
    assert ctypes.sizeof(_lib.LinearDesc) == abi_pins.LINEAR_DESC_BYTES
    assert ctypes.sizeof(_lib.CtcPrefixDesc) == abi_pins.CTC_PREFIX_DESC_BYTES


def test_mode_refusals_on_host_buffers(handle):
    """every pointer below is host memory or null: a launch would fault, so each answer is made before one"""
    from simulst_amd import _lib
    lib, h = handle
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))

    def desc(**kw):
        d = _lib.EditDesc()
        d.hyp, d.hyp_stride_b, d.n_ref, d.n_hyp, d.counts = p.value, 8, 4, 4, p.value
        d.n_ops, d.bp, d.bp_bytes, d.ops_cap, d.ops_width, d.pad = p.value, p.value, 1 << 40, 2046, 1, -1
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def call(d, N=0, refs=p, il=p, tl=p, S=8, cap=8, out=None):          # il: the hypothesis lengths, tl: the reference lengths
        return lib.simulst_edit_distance(h, refs, 8, tl, il, cap, S, N, ctypes.byref(d) if d is not None else None, out)

    err = lambda: lib.simulst_last_error(h)   # noqa: E731
    assert call(None) == E_NULL and call(None, N=2) == E_NULL and b": desc" in err()
    assert call(desc(counts=None), N=2) == E_NULL and b"counts" in err()
    assert call(desc(hyp=None), N=2) == E_NULL and b"d->hyp" in err()
    assert call(desc(), N=2, refs=None) == E_NULL and b": refs" in err()
    assert call(desc(), N=2, il=None) == E_NULL and b"hyp_lengths" in err()
    assert call(desc(), N=2, tl=None) == E_NULL and b"ref_lengths" in err()
    # the capacities: 1023 labels at the most, on either side
    assert call(desc(), cap=1024) == E_SHAPE and b"1023" in err()
    assert call(desc(), S=1024) == E_SHAPE and b"1023" in err()
    assert call(desc(), N=2, cap=1024) == E_SHAPE and b"1023" in err()
    assert call(desc(), cap=1023, S=1023) == 0
    assert call(desc(), cap=-1) == E_SHAPE and call(desc(), S=-1) == E_SHAPE and b"shape" in err()
    # pairs by position name rows 0 .. N-1: the host knows them
    assert call(desc(), N=5) == E_SHAPE and b"index" in err()
    # the path's own arguments
    assert call(desc(n_ops=None), out=p) == E_NULL and b"n_ops" in err()
    assert call(desc(ops_width=2), out=p) == E_SHAPE and b"ops_width" in err()
    assert call(desc(ops_cap=15), out=p) == E_SHAPE and b"ops_cap" in err()
    assert call(desc(bp=None), N=2, out=p) == E_NULL and b"bp" in err()
    assert call(desc(bp_bytes=2 * 73 * 64 - 1), N=2, cap=10, S=64, out=p) == E_SHAPE and b"scratch" in err()
    # no pair: nothing is launched, whatever the buffers are
    assert call(desc()) == 0 and call(desc(), N=-3) == 0 and call(desc(), out=p) == 0 and call(desc(bp=None), out=p) == 0


def test_best_alignment_compares_no_strings(handle):
    """what was the edit-distance call through simulst_ctc_best_alignment (NULL log_probs) is a null pointer, whatever the rest says"""
    lib, h = handle
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    for mtl in (8, -8):
        assert lib.simulst_ctc_best_alignment(h, None, 0, 0, 0, p, 8, p, p, 8, 2, mtl, 0, 0, p, p, None) == E_NULL
        assert b"log_probs" in lib.simulst_last_error(h)
    assert lib.simulst_ctc_best_alignment(h, p, 8, 4, 1, p, 3, p, p, 5, 2, -8, 0, 0, None, p, None) == E_SHAPE
    assert b"shape" in lib.simulst_last_error(h)
    assert lib.simulst_ctc_best_alignment(h, p, 8, 4, 1, None, 3, p, p, 5, 0, 3, 0, 0, None, p, p) == E_NULL
    assert b"targets" in lib.simulst_last_error(h)


# ---------------------------------------------------------------- the collective
def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from simulst_amd.sharding import reduce_error_counts
    mine = {"w_errors": 3 + rank, "wv_errors": torch.tensor(3 + rank), "w_total": 10 + 90 * rank}
    red = reduce_error_counts(mine, dist)
    vec = reduce_error_counts(torch.tensor([1, 2, 3, 4, 5 + rank], dtype=torch.int32), dist)
    if rank == 0:
        q.put(({k: int(v) for k, v in red.items()}, vec.tolist(), str(vec.dtype)))
    dist.barrier()
    dist.destroy_process_group()


def test_reduce_error_counts_two_ranks_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31700 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    red, vec, dtype = q.get(timeout=120)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert red == {"w_errors": 7, "wv_errors": 7, "w_total": 110}
    assert vec == [2, 4, 6, 8, 11] and dtype == "torch.int64"
    # the rate of the sums (7 / 110), not the mean of the ranks' rates (30 % and 4 %)
    assert 100.0 * red["w_errors"] / red["w_total"] != (30.0 + 4.0) / 2


def test_reduce_error_counts_refuses_rates():
    from simulst_amd.sharding import reduce_error_counts
    with pytest.raises(TypeError):
        reduce_error_counts(torch.tensor([0.3]), dist)
