"""Beam search over the transducer on the MI355X: simulst_joiner_scan_beam / simulst_joiner_emit_beam against the ungrouped entry
points (bit for bit: the same arithmetic in the same order), simulst_transducer_beam_reorder against index_select,
TransducerDecoder.beam_offline against greedy decode (beam 1) and against the fp64 restatement (tests/transducer_beam_ref.py), the
fairseq call shape (forward + reorder_incremental_state) and TransducerModel.generate.  GPU only."""
import functools

import pytest
import torch

import transducer_beam_ref as br
from test_hip_transducer import SENT_F, SENT_I, _prev_emit, _scan_inputs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope="module")
def ops():
    from simulst_amd.ops import Ops
    return Ops()


# ------------------------------------------------------------------------------------------- scan / emit over beam rows
BEAM_SHAPES = [(3, 5, 17, 32, 100), (2, 4, 1, 32, 64), (3, 3, 40, 256, 203)]           # Bs, beam, S, D, V


def _beam_inputs(Bs, beam, S, D, V, pattern):
    seed = 300 + 7 * Bs + S
    P, g, W, src_len = _scan_inputs(Bs, S, D, V, seed)                 # ragged src_len: S first, 1 last
    g_rows = g.repeat_interleave(beam, 0) + 0.1 * torch.randn(Bs * beam, D, generator=torch.Generator().manual_seed(seed + 5))
    pe = _prev_emit(pattern, src_len.repeat_interleave(beam), seed)    # differs between the rows of one sentence
    return P, g_rows.contiguous(), W, src_len, pe


def _scan_outputs(R, S, n_split):
    return (torch.full((R, S), SENT_F, device=DEV), torch.full((R, S, n_split), SENT_F, device=DEV),
            torch.full((R, S, n_split), SENT_I, device=DEV, dtype=torch.int32))


def _emit_outputs(R, D, dtype):
    return (torch.full((R, D), SENT_F, device=DEV, dtype=dtype), torch.full((R,), SENT_I, device=DEV, dtype=torch.int32),
            torch.full((R,), SENT_I, device=DEV, dtype=torch.int32))


def _run_pair(ops, shape, pattern, dtype, n_split, finished=None):
    """the grouped calls on P [Bs, S, D] -> (scan outputs, prev_emit, z, at_eos, emit_log), all on the CPU"""
    Bs, beam, S, D, V = shape
    R = Bs * beam
    P, g, W, src_len, pe = _beam_inputs(Bs, beam, S, D, V, pattern)
    Wp = ops.pack_joiner_weight(W.to(dtype).to(DEV))
    Pd, gd, sl = P.to(DEV), g.to(DEV), src_len.to(DEV)
    fin = None if finished is None else torch.tensor(finished, dtype=torch.int32, device=DEV)
    blank, best, idx = _scan_outputs(R, S, n_split)
    ped = pe.to(DEV)
    ops.joiner_scan_beam(Pd, gd, Wp, ped, sl, fin, blank, best, idx, group=beam, V=V)
    z, at_eos, log = _emit_outputs(R, D, dtype)
    ops.joiner_emit_beam(Pd, gd, blank, best, idx, ped, sl, fin, z, at_eos, log, group=beam, V=V)
    torch.cuda.synchronize()
    return [t.cpu() for t in (blank, best, idx, ped, z, at_eos, log)], (P, g, W, src_len, pe, Wp)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pattern", ["zero", "last", "random"])
@pytest.mark.parametrize("shape", BEAM_SHAPES)
def test_scan_beam_and_emit_beam_are_the_ungrouped_calls_bit_for_bit(ops, shape, pattern, dtype):
    Bs, beam, S, D, V = shape
    R = Bs * beam
    for n_split in (1, 3):
        (blank, best, idx, pe_new, z, at_eos, log), (P, g, W, src_len, pe, Wp) = _run_pair(ops, shape, pattern, dtype, n_split)
        # the earlier entry points on the replicated source
        Pr, slr = P.repeat_interleave(beam, 0).contiguous().to(DEV), src_len.repeat_interleave(beam).contiguous().to(DEV)
        rblank, rbest, ridx = _scan_outputs(R, S, n_split)
        rpe = pe.to(DEV)
        ops.joiner_scan(Pr, g.to(DEV), Wp, rpe, slr, rblank, rbest, ridx, V=V)
        rz, rat, _ = _emit_outputs(R, D, dtype)
        ops.joiner_emit(Pr, g.to(DEV), rblank, rbest, ridx, rpe, slr, rz, rat, V=V)
        torch.cuda.synchronize()
        s_idx = torch.arange(S).view(1, S)
        scanned = (s_idx >= pe.view(R, 1)) & (s_idx < src_len.repeat_interleave(beam).view(R, 1))
        assert int(scanned.sum()) >= R
        assert bool((blank[~scanned] == SENT_F).all()) and bool((best[~scanned] == SENT_F).all()) and bool((idx[~scanned] == SENT_I).all())
        assert bool((blank[scanned] != SENT_F).all()) and bool((idx[scanned] != SENT_I).all())
        # exact: sentinels and every scanned position
        assert torch.equal(blank, rblank.cpu()) and torch.equal(best, rbest.cpu()) and torch.equal(idx, ridx.cpu()), (n_split,)
        assert torch.equal(pe_new, rpe.cpu()) and torch.equal(at_eos, rat.cpu()) and torch.equal(z.view(torch.uint8), rz.cpu().view(torch.uint8))
        assert torch.equal(log, pe_new)
        last = src_len.repeat_interleave(beam) - 1
        assert bool((pe_new >= pe.clamp(max=last)).all()) and bool((pe_new <= last).all())
        assert at_eos.tolist() == (pe_new == last).int().tolist()


@pytest.mark.parametrize("dtype", DTYPES)
def test_finished_sentences_are_not_scanned(ops, dtype):
    shape = BEAM_SHAPES[0]
    Bs, beam, S, D, V = shape
    rows = slice(beam, 2 * beam)                                       # the rows of sentence 1
    for n_split in (1, 3):
        full, (_, _, _, _, pe, _) = _run_pair(ops, shape, "random", dtype, n_split)
        got, _ = _run_pair(ops, shape, "random", dtype, n_split, finished=[0, 1, 0])
        blank, best, idx, pe_new, z, at_eos, log = got
        assert bool((blank[rows] == SENT_F).all()) and bool((best[rows] == SENT_F).all()) and bool((idx[rows] == SENT_I).all())
        assert torch.equal(pe_new[rows], pe[rows]), "prev_emit kept"
        assert bool((z[rows] == torch.tensor(SENT_F, dtype=dtype)).all()) and bool((at_eos[rows] == SENT_I).all()) and bool((log[rows] == SENT_I).all())
        keep = torch.ones(Bs * beam, dtype=torch.bool)
        keep[rows] = False
        for a, b in zip(got, full):
            assert torch.equal(a[keep].view(torch.uint8) if a.dtype == torch.bfloat16 else a[keep],
                               b[keep].view(torch.uint8) if b.dtype == torch.bfloat16 else b[keep])


# ------------------------------------------------------------------------------------------------------------ reorder
def _reorder_case(ops, dtype, R, block, n_prev, order, finished=None, H=4, d=8, cap=9, n_layers=2):
    from simulst_amd import _lib
    gen = torch.Generator().manual_seed(17 + n_prev)
    mk = lambda: [torch.randn(R, H, cap, d, generator=gen).to(dtype).to(DEV) for _ in range(n_layers)]
    k, v = mk(), mk()
    ko, vo = [torch.full_like(t, 7.0) for t in k], [torch.full_like(t, 7.0) for t in v]
    pe = torch.randint(0, 50, (R,), generator=gen, dtype=torch.int32).to(DEV)
    peo = torch.full((R,), SENT_I, dtype=torch.int32, device=DEV)
    desc = _lib.DecoderDesc()
    desc.B, desc.D, desc.H, desc.n_layers, desc.cap = R, H * d, H, n_layers, cap
    desc.dtype = _lib.F32 if dtype == torch.float32 else _lib.BF16

    def structs(ks, vs):
        arr = (_lib.DecLayer * n_layers)()
        for l in range(n_layers):
            arr[l].k_cache, arr[l].v_cache = ks[l].data_ptr(), vs[l].data_ptr()          # head_step stays null
        return arr

    result = torch.zeros(1, dtype=torch.int32, device=DEV)
    fin = None if finished is None else torch.tensor(finished, dtype=torch.int32, device=DEV)
    ops.transducer_beam_reorder(desc, structs(k, v), structs(ko, vo), pe, peo, torch.tensor(order, dtype=torch.int32, device=DEV), fin,
                                result, block=block, n_prev=n_prev)
    torch.cuda.synchronize()
    return k, v, ko, vo, pe.cpu(), peo.cpu(), int(result.item())


def _check_reorder(k, v, ko, vo, pe, peo, expect, copied, n_prev):
    """expect[r]: the row whose state row r holds; copied[r]: whether its K/V were copied"""
    idx = torch.tensor(expect, device=DEV)
    rows = torch.tensor(copied, device=DEV)
    for src, dst in zip(k + v, ko + vo):
        assert torch.equal(dst[rows, :, :n_prev], src.index_select(0, idx)[rows, :, :n_prev])
        assert bool((dst[:, :, n_prev:] == 7.0).all()), "positions >= n_prev untouched"
        assert bool((dst[~rows] == 7.0).all()), "rows that copy nothing"
    assert peo.tolist() == pe[torch.tensor(expect)].tolist()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_prev", [0, 1, 7, 9])
def test_reorder_against_index_select(ops, dtype, n_prev):
    Bs, beam = 3, 4
    R = Bs * beam
    # block = beam: in-block permutations with repeated parents
    order = [1, 1, 0, 3, 7, 4, 4, 4, 11, 10, 9, 9]
    out = _reorder_case(ops, dtype, R, beam, n_prev, order)
    _check_reorder(*out[:6], order, [True] * R, n_prev)
    assert out[6] == 0
    # block = R: an arbitrary permutation over all rows (with a repeat)
    anyo = [11, 0, 5, 5, 2, 9, 3, 8, 1, 10, 7, 4]
    out = _reorder_case(ops, dtype, R, R, n_prev, anyo)
    _check_reorder(*out[:6], anyo, [True] * R, n_prev)
    assert out[6] == 0
    # a finished sentence's rows keep prev_emit and copy nothing
    out = _reorder_case(ops, dtype, R, beam, n_prev, order, finished=[0, 1, 0])
    expect = order[:4] + [4, 5, 6, 7] + order[8:]
    _check_reorder(*out[:6], expect, [True] * 4 + [False] * 4 + [True] * 4, n_prev)
    assert out[6] == 0
    # one index out of its block: counted, not performed (the row keeps its own state); a negative one likewise
    bad = list(order)
    bad[2] = 6
    out = _reorder_case(ops, dtype, R, beam, n_prev, bad)
    _check_reorder(*out[:6], order[:2] + [2] + order[3:], [True] * R, n_prev)
    assert out[6] == 1
    bad[9] = -1
    assert _reorder_case(ops, dtype, R, beam, n_prev, bad)[6] == 2


@pytest.mark.parametrize("dtype", DTYPES)
def test_both_reorder_entry_points_move_the_same_bytes(ops, dtype):
    """simulst_beam_reorder and simulst_transducer_beam_reorder launch one kernel: the same K/V sets, reorder (one index out of its
    block, one negative), finished list and block = beam give the same K/V bytes and the same count; each call moves its own
    payload and nothing of the other's"""
    from simulst_amd import _lib
    Bs, beam, H, d, cap, Ld, n_prev = 3, 3, 2, 8, 5, 2, 3
    R = Bs * beam
    gen = torch.Generator().manual_seed(29)
    mk = lambda: [torch.randn(R, H, cap, d, generator=gen).to(dtype).to(DEV) for _ in range(Ld)]    # noqa: E731
    k, v = mk(), mk()
    hs = [torch.randint(0, 50, (R * H,), generator=gen).to(DEV) for _ in range(Ld)]
    pe = torch.randint(0, 50, (R,), generator=gen, dtype=torch.int32).to(DEV)
    order = torch.tensor([1, 1, 5, 4, 3, 3, 8, -1, 6], dtype=torch.int32, device=DEV)          # row 2: out of its block; row 7: negative
    fin = torch.tensor([0, 1, 0], dtype=torch.int32, device=DEV)
    desc = _lib.DecoderDesc()
    desc.B, desc.D, desc.H, desc.n_layers, desc.cap = R, H * d, H, Ld, cap
    desc.dtype = _lib.F32 if dtype == torch.float32 else _lib.BF16

    def structs(ks, vs, ss=None):
        arr = (_lib.DecLayer * Ld)()
        for l in range(Ld):
            arr[l].k_cache, arr[l].v_cache = ks[l].data_ptr(), vs[l].data_ptr()
            if ss is not None:
                arr[l].head_step = ss[l].data_ptr()
        return arr

    sentinel = lambda ts: [torch.full_like(t, 7.0) for t in ts]                                   # noqa: E731
    ko_m, vo_m, ko_t, vo_t = sentinel(k), sentinel(v), sentinel(k), sentinel(v)
    hso = [torch.full_like(t, -5) for t in hs]
    peo = torch.full((R,), SENT_I, dtype=torch.int32, device=DEV)      # the guard of the MMA call: where a per-row int32 would land
    res_m, res_t = (torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(2))
    ops.beam_reorder(desc, structs(k, v, hs), structs(ko_m, vo_m, hso), order, fin, res_m, beam=beam, n_prev=n_prev)
    torch.cuda.synchronize()
    assert bool((peo == SENT_I).all()), "the MMA call writes no per-row int32"
    hso_m = [t.clone() for t in hso]
    ops.transducer_beam_reorder(desc, structs(k, v), structs(ko_t, vo_t), pe, peo, order, fin, res_t, block=beam, n_prev=n_prev)
    torch.cuda.synchronize()
    for a, b in zip(ko_m + vo_m, ko_t + vo_t):
        assert torch.equal(a, b)
    assert int(res_m.item()) == int(res_t.item()) == 2
    expect = [1, 1, 2, 3, 4, 5, 8, 7, 6]
    _check_reorder(k, v, ko_t, vo_t, pe.cpu(), peo.cpu(), expect, [True] * 3 + [False] * 3 + [True] * 3, n_prev)
    idx = torch.tensor(expect, device=DEV)
    for l in range(Ld):
        assert torch.equal(hso_m[l].view(R, H), hs[l].view(R, H).index_select(0, idx))
        assert torch.equal(hso[l], hso_m[l]), "the transducer call moves no head_step"


# ------------------------------------------------------------------------------------------------------------ decoder
SEED, CAPS, BEAM = 83, [12, 10, 8, 6], 4


@functools.lru_cache(None)
def _model():
    return br.beam_model(SEED)


@functools.lru_cache(None)
def _decoder(dtype):
    from simulst_amd.transducer import TransducerDecoder
    cfg, w, _, _ = _model()
    return TransducerDecoder(cfg, w, device=DEV, dtype=dtype)


@functools.lru_cache(None)
def _reference(lenpen, round_to=None):
    cfg, w, enc, lens = _model()
    return br.ref_beam(w, cfg, enc, lens, CAPS, BEAM, lenpen, BEAM, round_to=round_to)


def _device_hyps(tokens, lengths, scores, pos, emit):
    tokens, lengths, scores, pos, emit = (t.cpu() for t in (tokens, lengths, scores, pos, emit))
    out = []
    for s in range(tokens.size(0)):
        hyps = []
        for k in range(tokens.size(1)):
            n = int(lengths[s, k])
            if n:
                assert bool((emit[s, k, n:] == -1).all())
                hyps.append((tokens[s, k, :n].tolist(), float(scores[s, k]), pos[s, k, :n], emit[s, k, :n].tolist()))
        out.append(hyps)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_beam_one_is_greedy(dtype):
    """beam_offline(beam=1) gives greedy_offline's tokens up to and including the first EOS (EOS appended where greedy ran to the
    cap) and the same emit positions, exactly: the same kernels over the same number of rows"""
    cfg, _, enc, lens = _model()
    dec = _decoder(dtype)
    n = max(CAPS) + 1
    gt, ge, _ = dec.greedy_offline(enc.to(DEV), torch.tensor(lens), n)
    gt, ge = gt.cpu(), ge.cpu()
    got = _device_hyps(*dec.beam_offline(enc.to(DEV), torch.tensor(lens), CAPS, beam=1)[:5])
    for s, cap in enumerate(CAPS):
        toks = gt[s, :cap].tolist()
        toks = toks[:toks.index(cfg.eos) + 1] if cfg.eos in toks else toks + [cfg.eos]
        assert len(got[s]) == 1
        assert got[s][0][0] == toks, (s, got[s][0][0], toks)
        assert got[s][0][3] == ge[s, :len(toks)].tolist(), s


@pytest.mark.parametrize("lenpen", [1.0, 0.6])
def test_full_model_against_the_fp64_restatement(lenpen):
    """Beam 4, nbest 4, caps 12 / 10 / 8 / 6 over 4 ragged sentences (12, 10, 5 and 2 pooled positions), fp32.  The weight / input
    seed was chosen on the CPU: seed 83 is the one of the first 200 with the largest smallest margin of the reference over the whole
    run, 2.02e-3 at both length penalties (23 seeds reach 1e-3; caps as first tried), and sentence 0 finalises hypotheses of 3, 4, 4
    and 6 tokens before its cap.  At that margin nothing is excused."""
    cfg, w, enc, lens = _model()
    ref, margins, src_len = _reference(lenpen)
    smallest = br.smallest_margin(margins)
    print(f"lenpen {lenpen}: smallest reference margin {smallest:.3e}")
    assert smallest >= 1e-3, smallest
    dec = _decoder(torch.float32)
    got = _device_hyps(*dec.beam_offline(enc.to(DEV), torch.tensor(lens), CAPS, beam=BEAM, lenpen=lenpen, nbest=BEAM)[:5])
    single = br.tr.TransducerRef(w, heads=cfg.num_heads, downsample=cfg.downsample, pad=cfg.padding_idx, eos=cfg.eos)
    worst = 0.0
    for s in range(len(lens)):
        last = int(src_len[s]) - 1
        assert [h[0] for h in got[s]] == [h[0] for h in ref[s]], (s, got[s], ref[s])
        for (gt, gs, gp, ge), (rt, rs, rp, re_) in zip(got[s], ref[s]):
            assert ge == re_, (s, gt, ge, re_)
            worst = max(worst, abs(gs - rs), float((gp - rp.float()).abs().max()))
            assert abs(gs - rs) <= 1e-4, (s, gs, rs)
            torch.testing.assert_close(gp, rp.float(), atol=1e-4, rtol=0)
            assert all(a <= b for a, b in zip(ge, ge[1:])) and 0 <= ge[0] and ge[-1] <= last, (s, ge)
            # the blank is a candidate only where it was not forced out: never a token emitted at the last position
            assert all(e < last for t, e in zip(gt, ge) if t == br.tr.BLANK), (s, gt, ge)
            # the hypothesis alone, teacher-forced through the fp64 step: its own emit positions, and a blank forced out exactly at
            # the last position (elsewhere the row keeps its blank logit)
            single.set_source(enc[s:s + 1, :], [lens[s]], T=max(lens))
            rows, emits, _ = single.run_forced(torch.tensor([gt[:-1] + [0]]))
            assert emits[:, 0].tolist() == ge, (s, ge, emits[:, 0].tolist())
            for u, e in enumerate(ge):
                assert (float(rows[u, 0, br.tr.BLANK]) == br.tr.BLANK_AT_EOS) == (e == last), (s, u, e)
    print(f"lenpen {lenpen}: largest score / positional-score error {worst:.3e}")


def test_fairseq_surface_matches_beam_offline():
    """a SequenceGenerator-style driver: the encoder output repeated per row, decoder.forward per step, reorder_incremental_state
    at the start of every step t > 0, the selection by BeamSearch's own kernels"""
    from simulst_amd.beam import BeamSearch
    cfg, _, enc, lens = _model()
    dec = _decoder(torch.float32)
    lenpen = 0.6
    want = _device_hyps(*dec.beam_offline(enc.to(DEV), torch.tensor(lens), CAPS, beam=BEAM, lenpen=lenpen, nbest=BEAM)[:5])
    Bs, R = len(lens), len(lens) * BEAM
    pad = torch.arange(enc.shape[1]).view(1, -1) >= torch.tensor(lens).view(Bs, 1)
    eo = {"encoder_out": [enc.repeat_interleave(BEAM, 0).transpose(0, 1).contiguous().to(DEV)],
          "encoder_padding_mask": [pad.repeat_interleave(BEAM, 0).to(DEV)]}
    bs = BeamSearch(dec.ops, CAPS, beam=BEAM, V=cfg.vocab, eos=cfg.eos, pad=cfg.padding_idx, lenpen=lenpen, nbest=BEAM, device=DEV)
    inc = {}
    st = {"prev": torch.full((R, 1), cfg.eos, dtype=torch.int64, device=DEV), "order": None}
    emit_log = torch.full((bs.L, R), -1, dtype=torch.int32, device=DEV)

    def logits_fn(t, toks):
        if t > 0:
            dec.reorder_incremental_state(inc, st["order"])
            st["prev"] = torch.cat([st["prev"].index_select(0, st["order"]), toks.view(R, 1)], 1)
        logits, _ = dec.forward(st["prev"], encoder_out=eo, incremental_state=inc)
        emit_log[t].copy_(inc[dec.STATE_KEY].prev_emit)
        return logits[:, 0].contiguous()

    def after_select(t):
        st["order"] = bs.reorder.clone().long()

    tokens, lengths, scores, pos = bs.run(logits_fn, after_select)
    got = _device_hyps(tokens, lengths, scores, pos, dec._hypothesis_emit(bs, emit_log))
    for s in range(Bs):
        assert [h[0] for h in got[s]] == [h[0] for h in want[s]], s
        for (gt, gs, gp, ge), (wt, ws, wp, we) in zip(got[s], want[s]):
            assert ge == we and abs(gs - ws) <= 1e-6
            torch.testing.assert_close(gp, wp, atol=1e-6, rtol=0)
    with pytest.raises(ValueError):
        dec.reorder_incremental_state(inc, torch.arange(R - 1, device=DEV))
    with pytest.raises(NotImplementedError):                     # the index is read on the device: a host one is refused
        dec.reorder_incremental_state(inc, torch.arange(R))


def test_bf16_best_hypothesis_agreement():
    """bf16, beam 4, against the fp64 restatement on bf16-rounded weights and encoder states: first-token and whole-hypothesis
    agreement of the best hypothesis are REPORTED; this is a report, not a bound -- asserted as loosely as
    test_hip_beam.test_bf16_best_hypothesis_agreement (the first token on at least half of the sentences)"""
    cfg, _, enc, lens = _model()
    ref, _, _ = _reference(1.0, torch.bfloat16)
    dec = _decoder(torch.bfloat16)
    got = _device_hyps(*dec.beam_offline(enc.to(DEV), torch.tensor(lens), CAPS, beam=BEAM)[:5])
    n = len(lens)
    first = sum(g[0][0][0] == r[0][0][0] for g, r in zip(got, ref)) / n
    same = sum(g[0][0] == r[0][0] for g, r in zip(got, ref)) / n
    emit = sum(g[0][0] == r[0][0] and g[0][3] == r[0][3] for g, r in zip(got, ref)) / n
    print(f"bf16 beam 4 best hypothesis: first token {first:.2f}, whole hypothesis {same:.2f}, with its emit positions {emit:.2f}")
    assert first >= 0.5


# ------------------------------------------------------------------------------------------------------- the public surface
def test_generate_surface():
    from simulst_amd.transducer import TransducerModel
    cfg, w, _, _ = _model()
    model = TransducerModel(cfg, w, device=DEV)
    fb = torch.randn(3, 200, 80, generator=torch.Generator().manual_seed(9))
    L = torch.tensor([200, 160, 90])
    for b in range(3):
        fb[b, L[b]:] = 0
    out = model.generate(fb.to(DEV), L, beam=5, nbest=3, lenpen=1.0)
    assert len(out) == 3
    for s, hyps in enumerate(out):
        assert len(hyps) == 3
        assert set(hyps[0]) == {"tokens", "score", "positional_scores", "alignment", "attention"}
        sc = [float(h["score"]) for h in hyps]
        assert sc == sorted(sc, reverse=True)
        for h in hyps:
            n = h["tokens"].numel()
            assert int(h["tokens"][-1]) == cfg.eos and n <= int(0.1 * int(L[s]) + 10) + 1
            assert h["positional_scores"].numel() == n and h["attention"] is None
            al = h["alignment"].tolist()
            assert len(al) == n and al == sorted(al) and al[0] >= 0
            assert abs(float(h["positional_scores"].sum()) / n - float(h["score"])) < 1e-4
    again = model.generate_offline(fb.to(DEV), L, beam=5, nbest=3)
    assert [[h["tokens"].tolist() for h in hyps] for hyps in again] == [[h["tokens"].tolist() for h in hyps] for hyps in out]
    # without beam arguments: greedy, the tuple of before
    toks, info = model.generate_offline(fb.to(DEV), L, n_steps=7)
    enc = model.encoder.forward(fb.to(DEV), L)
    gt, ge, _ = model.decoder.greedy_offline(enc["encoder_out_btd"], enc["encoder_lengths"], 7, False,
                                             T=int(enc["encoder_lengths"].max().item()))
    assert toks.shape == (3, 7) and torch.equal(toks, gt) and torch.equal(info["emit"], ge) and set(info) == {"emit", "encoder", "state"}
