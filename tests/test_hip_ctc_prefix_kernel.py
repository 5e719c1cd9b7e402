"""The prefix beam recursion in one launch (csrc/ctc_prefix.hip: simulst_ctc_prefix_beam, behind
ctc.ctc_prefix_beam_advance) on the MI355X, fed with the hand-made candidate lists of tests/ctc_prefix_ref.py -- no projection
is involved -- against the fp64 reference of tests/ctc_beam_ref.py on the same lists and against the torch form (composed=True).

The rule is tests/test_hip_ctc_beam.py's: a score lies within beam_bound(n, score) = (n + 1) 2^-22 max(1, |score|) of the reference; an
utterance whose reference margin (over the ranking of the first min(4, beam) hypotheses and every frame's selection boundary) is <=
twice that bound is UNCLEAR and its identity is not compared; at most 10 % of a case may be unclear.  Where the margin over the WHOLE
beam's ranking is clear as well, every slot is compared, the dead ones included.  The shares are known before any device runs
(tests/test_ctc_prefix_cases_cpu.py)."""
import ctypes
import math

import pytest
import torch

import ctc_beam_ref as br
import ctc_prefix_ref as pr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 1
NEG = float("-inf")


@pytest.fixture(scope="module")
def ops():
    from simulst_amd.ops import Ops
    return Ops()


def _advance(ops, ids, lp, lengths, beam, state=None, **kw):
    from simulst_amd import ctc
    if state is None:
        state = ctc.ctc_prefix_beam_init(ids.size(0), beam, DEV, PAD)
    return ctc.ctc_prefix_beam_advance(ids, lp, torch.as_tensor(lengths, device=DEV), state, pad=PAD, ops=ops, **kw)


def _cpu(state):
    torch.cuda.synchronize()
    return tuple(x.cpu() for x in state)


_RUNS = {}


def _run(ops, key, c, composed=True):
    """kernel and torch form over a case's lists, once"""
    if key not in _RUNS:
        ids, lp = c["ids"].to(DEV), c["lp"].to(DEV)
        _RUNS[key] = (_cpu(_advance(ops, ids, lp, c["lengths"], c["beam"])),
                      _cpu(_advance(ops, ids, lp, c["lengths"], c["beam"], composed=True)) if composed else None)
    return _RUNS[key]


def _score(p_b, p_nb):
    return br.lae(float(p_b), float(p_nb))


def _check_reference(c, state, what):
    strings, lengths, p_b, p_nb = state
    B, beam = p_b.shape
    assert strings.shape[:2] == (B, beam) and strings.dtype == lengths.dtype == torch.int64 and p_b.dtype == p_nb.dtype == torch.float32
    assert not bool(torch.isnan(p_b).any()) and not bool(torch.isnan(p_nb).any())
    worst = 0.0
    for b, n in enumerate(c["lengths"]):
        hyps, margin = c["ref"][b]
        for j in range(beam):                                             # every slot, clear or not: pad behind the length, dead slots whole
            k = int(lengths[b, j])
            assert bool((strings[b, j, k:] == PAD).all()), (what, b, j)
            if _score(p_b[b, j], p_nb[b, j]) == NEG:
                assert k == 0 and float(p_b[b, j]) == NEG and float(p_nb[b, j]) == NEG, (what, b, j)
        if c["unclear"][b]:
            continue
        for j in range(beam if not c["unclear_beam"][b] else c["nbest"]):
            k = int(lengths[b, j])
            if j >= len(hyps):
                assert k == 0 and _score(p_b[b, j], p_nb[b, j]) == NEG, (what, b, j)
                continue
            assert tuple(strings[b, j, :k].tolist()) == hyps[j][0], (what, b, j, strings[b, j, :k].tolist(), hyps[j])
            d = abs(_score(p_b[b, j], p_nb[b, j]) - hyps[j][1])
            worst = max(worst, d / br.beam_bound(n, hyps[j][1]))
            assert d <= br.beam_bound(n, hyps[j][1]), (what, b, j, d, br.beam_bound(n, hyps[j][1]), margin)
    print(f"{what}: {sum(c['unclear'])} of {B} unclear, worst |score - ref| / bound {worst:.3f}")
    assert sum(c["unclear"]) <= 0.1 * B


def _check_composed(c, got, comp, what):
    for b, n in enumerate(c["lengths"]):
        if c["unclear"][b]:
            continue
        slots = slice(0, c["beam"] if not c["unclear_beam"][b] else c["nbest"])
        assert torch.equal(got[1][b, slots], comp[1][b, slots]), (what, b)
        w = min(got[0].size(2), comp[0].size(2))
        assert torch.equal(got[0][b, slots, :w], comp[0][b, slots, :w]), (what, b)
        for x, y in ((got[2], comp[2]), (got[3], comp[3])):
            for j in range(slots.stop):
                a, r = float(x[b, j]), float(y[b, j])
                assert (a == r) if NEG in (a, r) else abs(a - r) <= br.beam_bound(n, r), (what, b, j, a, r)


@pytest.mark.parametrize("name", list(pr.CASES))
def test_lists_against_the_reference_and_the_torch_form(ops, name):
    c = pr.case(name)
    got, comp = _run(ops, name, c)
    _check_reference(c, got, name)
    _check_composed(c, got, comp, name)
    if name.startswith("peaky_T130"):                                      # the best prefix is the labels themselves: past one wave of string
        assert int(got[1][:, 0].min()) == c["T"]


@pytest.mark.parametrize("beam", pr.GRID_BEAMS)
@pytest.mark.parametrize("k", pr.GRID_KS)
def test_every_beam_and_candidate_count(ops, beam, k):
    """beam x k up to the 144-entry pool; the first frames hold fewer live prefixes than the beam, two frames have no candidate but the
    blank, one gives a live candidate the log-probability -inf"""
    c = pr.grid_case(beam, k)
    got, comp = _run(ops, ("grid", beam, k), c, composed=k > 0)           # (the torch form has no k = 0: it reduces over the candidates)
    _check_reference(c, got, f"beam {beam} k {k}")
    if k:
        _check_composed(c, got, comp, f"beam {beam} k {k}")
    if k == 0:
        assert bool((got[1] == 0).all()) and bool((got[3] == NEG).all())


def test_ragged_lengths_and_untouched_rows(ops):
    """lengths [T, 0, 1, 17, T - 1, ...] in one batch, the candidates past each length overwritten with garbage; then a second call in
    which only utterance 0 has frames: every other row's state keeps its bits"""
    from simulst_amd import ctc
    c = pr.ragged_case()
    ids, lp = c["ids"].clone(), c["lp"].clone()
    g = torch.Generator().manual_seed(3)
    for b, n in enumerate(c["lengths"]):
        ids[b, n:] = torch.randint(-1, 12, ids[b, n:].shape, generator=g).to(torch.int32)
        lp[b, n:] = torch.randn(lp[b, n:].shape, generator=g) * 3
        lp[b, n:, 0] = float("nan")
    idsd, lpd = ids.to(DEV), lp.to(DEV)
    st = _advance(ops, idsd, lpd, c["lengths"], c["beam"])
    got = _cpu(st)
    _check_reference(c, got, "ragged")
    _check_composed(c, got, _cpu(_advance(ops, idsd, lpd, c["lengths"], c["beam"], composed=True)), "ragged")
    init = _cpu(ctc.ctc_prefix_beam_init(ids.size(0), c["beam"], DEV, PAD))
    empty = c["lengths"].index(0)
    assert bool((got[0][empty] == PAD).all()) and all(torch.equal(got[i][empty], init[i][empty]) for i in (1, 2, 3))
    lens2 = [5] + [0] * (ids.size(0) - 1)
    nxt = _cpu(_advance(ops, idsd[:, :9], lpd[:, :9], lens2, c["beam"], state=st))
    w = got[0].size(2)
    assert nxt[0].size(2) == w + 9 and bool((nxt[0][1:, :, w:] == PAD).all())
    assert torch.equal(nxt[0][1:, :, :w], got[0][1:]) and all(torch.equal(nxt[i][1:], got[i][1:]) for i in (1, 2, 3))
    assert not torch.equal(nxt[3][0], got[3][0])                          # (utterance 0 did move)


@pytest.mark.parametrize("beam", [2, 4])
def test_exact_ties_resolve_in_pool_order(ops, beam):
    """one frame from the initial state, the blank and three candidates all at log 0.25: the empty prefix first, then the candidates in
    list order (not label order)"""
    q = math.log(0.25)
    ids = torch.tensor([[[0, 5, 3, 7]]], dtype=torch.int32, device=DEV)
    lp = torch.full((1, 1, 4), q, dtype=torch.float32, device=DEV)
    strings, lengths, p_b, p_nb = _cpu(_advance(ops, ids, lp, [1], beam))
    q32 = float(torch.tensor(q, dtype=torch.float32))
    want = [(), (5,), (3,), (7,)][:beam]
    assert lengths[0].tolist() == [len(w) for w in want]
    assert [tuple(strings[0, j, :len(w)].tolist()) for j, w in enumerate(want)] == want
    assert p_b[0].tolist() == [q32] + [NEG] * (beam - 1) and p_nb[0].tolist() == [NEG] + [q32] * (beam - 1)


def test_repeated_label_takes_p_b_only(ops):
    """three frames with the one candidate c: the prefix "cc" can only follow a blank after "c", so it is fed by p_b("c") alone"""
    a, q, cl = 0.5, 0.3, 4
    ids = torch.tensor([[[0, cl]] * 3], dtype=torch.int32, device=DEV)
    lp = torch.tensor([[[math.log(a), math.log(q)]] * 3], dtype=torch.float32, device=DEV)
    strings, lengths, p_b, p_nb = _cpu(_advance(ops, ids, lp, [3], 3))
    assert lengths[0].tolist() == [1, 0, 2] and strings[0, 0, 0] == cl and strings[0, 2, :2].tolist() == [cl, cl]
    want_b = [math.log((q * a + q * q + a * q) * a), 3 * math.log(a), NEG]
    want_nb = [math.log((q * q + a * q) * q + a * a * q), NEG, math.log(q * a * q)]
    for j in range(3):
        for got, want in ((float(p_b[0, j]), want_b[j]), (float(p_nb[0, j]), want_nb[j])):
            assert (got == want) if want == NEG else abs(got - want) <= br.beam_bound(3, want), (j, got, want)


@pytest.mark.parametrize("name,chunk", [("flat_T48_V6_k3_beam4", 1), ("flat_T48_V6_k3_beam4", 7), ("peaky_T70_V12_k8_beam16", 7),
                                        ("reentry_V4_beam3_seed140", 1)])
def test_cuts_with_the_state_carried_give_the_same_bits(ops, name, chunk):
    c = pr.case(name)
    whole = _run(ops, name, c)[0]
    ids, lp = c["ids"].to(DEV), c["lp"].to(DEV)
    lens = torch.tensor(pr.ragged_lengths(c["T"], ids.size(0)) if ids.size(0) > 1 else [c["T"]])
    one = _cpu(_advance(ops, ids, lp, lens, c["beam"])) if ids.size(0) > 1 else whole
    state = None
    for t0 in range(0, c["T"], chunk):
        state = _advance(ops, ids[:, t0:t0 + chunk], lp[:, t0:t0 + chunk], (lens - t0).clamp(0, chunk), c["beam"], state=state)
    cut = _cpu(state)
    assert cut[0].shape == one[0].shape
    for x, y in zip(cut, one):
        assert torch.equal(x, y)


def test_strided_views_and_batch_position(ops):
    c = pr.case("flat_T48_V40_k8_beam8")
    want = _run(ops, "flat_T48_V40_k8_beam8", c)[0]
    B, T, kp = c["ids"].shape
    big_i = torch.full((B, T + 5, kp + 3), 7, dtype=torch.int32, device=DEV)
    big_l = torch.full((B, T + 5, kp + 3), 0.5, dtype=torch.float32, device=DEV)
    big_i[:, 2:T + 2, :kp], big_l[:, 2:T + 2, 1:kp + 1] = c["ids"].to(DEV), c["lp"].to(DEV)
    vi, vl = big_i[:, 2:T + 2, :kp], big_l[:, 2:T + 2, 1:kp + 1]
    assert not vi.is_contiguous() and not vl.is_contiguous()
    for x, y in zip(_cpu(_advance(ops, vi, vl, c["lengths"], c["beam"])), want):
        assert torch.equal(x, y)
    # a frame-major list (the batch stride is the small one), and an utterance alone instead of at position 9
    tl = c["lp"].to(DEV).transpose(0, 1).contiguous().transpose(0, 1)
    assert tl.stride(0) < tl.stride(1)
    for x, y in zip(_cpu(_advance(ops, c["ids"].to(DEV), tl, c["lengths"], c["beam"])), want):
        assert torch.equal(x, y)
    for x, y in zip(_cpu(_advance(ops, c["ids"][9:10].to(DEV), c["lp"][9:10].to(DEV), [T], c["beam"])), want):
        assert torch.equal(x, y[9:10])


def test_capacity_limit_and_fallback(ops, monkeypatch):
    """strings of SIMULST_CTC_PREFIX_CAP(beam) labels run on the kernel; one more, and the Python call answers through the torch form
    while the entry point itself refuses the shape"""
    from simulst_amd import _lib, ctc
    beam, T = 16, 6
    limit = _lib.ctc_prefix_cap(beam)
    assert limit >= 1024
    c = pr.case("peaky_T70_V12_k8_beam16")
    ids, lp = c["ids"][:3, :T].to(DEV), c["lp"][:3, :T].to(DEV)
    calls = []
    real = ctc._prefix_beam_advance_composed
    monkeypatch.setattr(ctc, "_prefix_beam_advance_composed", lambda *a: calls.append(1) or real(*a))
    results = []
    for width in (limit - T, limit - T + 1):
        st = list(ctc.ctc_prefix_beam_init(3, beam, DEV, PAD))
        st[0] = torch.full((3, beam, width), PAD, dtype=torch.int64, device=DEV)
        results.append(_cpu(_advance(ops, ids, lp, [T, T, 3], beam, state=tuple(st))))
        assert len(calls) == (width + T > limit)
    short = _cpu(_advance(ops, ids, lp, [T, T, 3], beam))
    for r in results:
        assert torch.equal(r[1], short[1]) and torch.equal(r[0][:, :, :T], short[0]) and bool((r[0][:, :, T:] == PAD).all())
    for x, y in zip(results[0][1:], short[1:]):
        assert torch.equal(x, y)
    # the raw call at limit + 1
    d = _lib.CtcPrefixDesc()
    strings = torch.full((3, beam, limit + 1), PAD, dtype=torch.int64, device=DEV)
    lengths, p_b, p_nb = (x.clone() for x in ctc.ctc_prefix_beam_init(3, beam, DEV, PAD)[1:])
    il = torch.tensor([T, T, 3], device=DEV)
    d.cand_ids, d.id_stride_b, d.id_stride_t, d.k, d.pad, d.cap = ids.data_ptr(), ids.stride(0), ids.stride(1), 8, PAD, limit + 1
    d.lengths, d.p_b, d.p_nb = lengths.data_ptr(), p_b.data_ptr(), p_nb.data_ptr()
    vp = ctypes.c_void_p
    rc = ops.lib.simulst_ctc_prefix_beam(ops.h.ptr, vp(lp.data_ptr()), lp.stride(1), lp.stride(0), lp.stride(2), vp(il.data_ptr()), T, 3,
                                         beam, 0, ctypes.byref(d), vp(strings.data_ptr()))
    assert rc == -2 and b"cap is" in ops.lib.simulst_last_error(ops.h.ptr)
    torch.cuda.synchronize()
    assert bool((strings == PAD).all())


def _launches(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))


def test_launch_count_does_not_grow_with_the_frames(ops):
    c = pr.case("flat_T48_V40_k8_beam8")
    ids, lp = c["ids"].to(DEV), c["lp"].to(DEV)
    lens = torch.full((ids.size(0),), 48, device=DEV)
    counts = {}
    for T in (4, 32):
        _advance(ops, ids[:, :T], lp[:, :T], lens.clamp(max=T), c["beam"])                        # (first call: module load, LDS limit)
        counts[T] = _launches(lambda: _advance(ops, ids[:, :T], lp[:, :T], lens.clamp(max=T), c["beam"]))
    composed = _launches(lambda: _advance(ops, ids[:, :4], lp[:, :4], lens.clamp(max=4), c["beam"], composed=True))
    print(f"device launches: kernel form {counts}, torch form over 4 frames {composed}")
    assert counts[4] > 0 and counts[4] == counts[32] and counts[4] <= 32 < composed
