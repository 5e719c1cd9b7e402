"""Scoring a given translation with the transducer on the MI355X: simulst_joiner_lattice and simulst_rnnt_forward
(csrc/transducer.hip) against the fp64 restatement tests/rnnt_ref.py computed from the kernels' own inputs, and
TransducerDecoder.forward_lattice / features_teacher_forced / TransducerModel.score_reference against fixture g27 (the reference's
own lattice).  GPU only.

Bound of a lattice cell, from the number formats: the logit of column v is within tol[v] = c sum_k |W[v, k]| of fp64 (c = 2^-8 for
bf16: the half-ulp of the rounded tanh plus as much for its approximation; 2^-16 for fp32 -- the joiner tolerance of
tests/test_hip_transducer.py), log-sum-exp is 1-Lipschitz in the sup norm, so
    |lp - ref| <= tol[v] + max_v tol[v] + V 2^-24 + 2^-20
with the last two terms for the fp32 sum of V exponentials and the exp / log roundings.  Bound of the recursion:
(S + n + 1) 2^-22 max(1, max |alpha_ref|), one rounding of the sum and one of the log-add per move (rnnt_ref.ll_bound)."""
import math
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

import rnnt_ref as rr
import transducer_ref as tr
from test_hip_transducer import _big_model, _scan_inputs, tol_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G25 = os.path.join(ROOT, "tests", "golden", "g25_transducer.npz")
G27 = os.path.join(ROOT, "tests", "golden", "g27_transducer_lattice.npz")
DEV = "cuda:0"
SENT = -777.0
I32 = dict(dtype=torch.int32)


@pytest.fixture(scope="module")
def ops():
    from simulst_amd.ops import Ops
    return Ops()


# ---------------------------------------------------------------------------------------------------------------- lattice kernel
def _lattice_inputs(B, S, U1, D, V, seed, src_len, tgt_len, blank, integer_w=False):
    P, g, W, _ = _scan_inputs(B, S, D, V, seed, integer_w=integer_w)
    gen = torch.Generator().manual_seed(seed + 5)
    G = (g.unsqueeze(1) + 0.3 * torch.randn(B, U1, D, generator=gen)).contiguous()
    labels = torch.randint(0, V, (B, U1), generator=gen)
    labels[0, :4] = torch.tensor([V - 1, (blank + 1) % V, (blank - 1) % V, blank])      # the last column, the blank's neighbours, the blank
    return P, G, W, labels.to(torch.int32), torch.tensor(src_len, **I32), torch.tensor(tgt_len, **I32)


def _check_lattice(ops, P, G, W, labels, src_len, tgt_len, dtype, n_split, blank):
    B, S, D = P.shape
    U1, V = G.shape[1], W.shape[0]
    Wr = W.to(dtype)
    lpb = torch.full((B, S, U1), SENT, device=DEV)
    lpl = torch.full((B, S, U1), SENT, device=DEV)
    ops.joiner_lattice(P.to(DEV), G.to(DEV), ops.pack_joiner_weight(Wr.to(DEV)), labels.to(DEV), src_len.to(DEV), tgt_len.to(DEV), V=V,
                       blank=blank, n_split=n_split, lp_blank=lpb, lp_label=lpl)
    torch.cuda.synchronize()
    lpb, lpl = lpb.cpu().double(), lpl.cpu().double()
    rb, rl, _ = rr.joiner_lattice(P, G, Wr, labels, blank=blank)                  # fp64, on the dtype-rounded W
    vb, vl = rr.valid_cells(src_len, tgt_len, S, U1)
    assert int(vl.sum()) > 0
    assert bool((lpb[~vb] == SENT).all()) and bool((lpl[~vl] == SENT).all()), "cells outside the valid ranges are not written"
    tol = tol_rows(Wr, dtype)
    slack = float(tol.max()) + V * 2.0 ** -24 + 2.0 ** -20
    eb = (lpb - rb).abs()[vb]
    el = ((lpl - rl).abs() - tol[labels.long()].view(B, 1, U1))[vl]
    print(f"lattice {tuple(P.shape)} U1 {U1} V {V} {dtype} n_split {n_split}: blank err {float(eb.max()):.3e} (bound "
          f"{float(tol[blank]) + slack:.3e}), label err - tol[v] {float(el.max()):.3e} (bound {slack:.3e})")
    assert bool((eb <= float(tol[blank]) + slack).all()), float(eb.max())
    assert bool((el <= slack).all()), float(el.max())
    assert bool((lpb[vb] < 0).all()) and bool((lpl[vl] <= 0).all())


SMALL = dict(B=3, S=19, U1=5, D=32, V=70, src_len=[19, 16, 1], tgt_len=[4, 1, 3])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("blank", [0, 17])
@pytest.mark.parametrize("n_split", [1, 3])
def test_lattice_small_against_fp64(ops, n_split, blank, dtype):
    """V no multiple of 16; with 3 parts (2, 2 and 1 column tiles) one part holds no label of row 0 and one holds the blank"""
    _check_lattice(ops, *_lattice_inputs(seed=300, blank=blank, **SMALL), dtype, n_split, blank)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_lattice_model_dims_against_fp64(ops, dtype):
    """the product's D and V, several row panels (2 * 17 * 2 row tiles), two u tiles per (b, s), n_split from Ops.joiner_split"""
    from simulst_amd.ops import Ops
    B, S, U1, D, V = 2, 17, 18, 256, 4096
    n_split = Ops.joiner_split(B, S, V, dtype)
    assert n_split > 1 and Ops.lattice_split(B, S, U1, V, dtype) >= 1
    _check_lattice(ops, *_lattice_inputs(B, S, U1, D, V, 301, [17, 9], [17, 5], 0), dtype, n_split, 0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_lattice_integer_weights(ops, dtype):
    """weights exact in bf16 and asymmetric: a transposed or permuted fragment map gives other logits, not rounding noise"""
    _check_lattice(ops, *_lattice_inputs(seed=302, blank=0, integer_w=True, **SMALL), dtype, 2, 0)


# ---------------------------------------------------------------------------------------------------------------- recursion
def _run_forward(ops, lb, lt, src_len, tgt_len, want_best=True):
    out = ops.rnnt_forward(lb.float().to(DEV).contiguous(), lt.float().to(DEV).contiguous(), torch.tensor(src_len, **I32).to(DEV),
                           torch.tensor(tgt_len, **I32).to(DEV), want_best=want_best)
    torch.cuda.synchronize()
    return [o.cpu() for o in out] if want_best else out.cpu()


def _check_rows(lb, lt, src_len, tgt_len, ll, best_ll, emit, exact_emit=None):
    """every row against the fp64 recursion: ll within the bound; the returned alignment monotone and in range, its fp64 score within
    the bound of best_ll and of the fp64 optimum (tie-robust: no row is excluded); best_ll <= ll"""
    lb, lt = lb.float(), lt.float()                                   # the kernel's inputs
    for b, (S, n) in enumerate(zip(src_len, tgt_len)):
        ref, amax = rr.forward_ll(lb[b], lt[b], S, n)
        bound = rr.ll_bound(S, n, amax)
        err = abs(float(ll[b]) - ref)
        print(f"row {b} (S {S}, n {n}): ll {float(ll[b]):.6f} ref {ref:.6f} err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (b, err, bound)
        if best_ll is None:
            continue
        e = emit[b, :n].tolist()
        assert e == sorted(e) and all(0 <= x < S for x in e), (b, e)
        assert bool((emit[b, n:] == -1).all())
        opt, ref_emit = rr.best_alignment(lb[b], lt[b], S, n)
        score = rr.path_score(lb[b], lt[b], S, n, e)
        bbound = rr.ll_bound(S, n, abs(opt))
        assert abs(score - float(best_ll[b])) <= bbound and abs(score - opt) <= bbound, (b, score, float(best_ll[b]), opt)
        assert float(best_ll[b]) <= float(ll[b])
        if exact_emit is not None:
            assert e == exact_emit[b], (b, e, exact_emit[b])


SHAPES = [(1, 1), (2, 3), (17, 33), (65, 130)]


@pytest.mark.parametrize("S,n", SHAPES)
def test_forward_random_lattice(ops, S, n):
    lb, lt = rr.random_lattice(2, S, n + 1, seed=400 + S)
    ll, best, emit = _run_forward(ops, lb, lt, [S, S], [n, n])
    _check_rows(lb, lt, [S, S], [n, n], ll, best, emit)
    only = _run_forward(ops, lb, lt, [S, S], [n, n], want_best=False)
    assert torch.equal(only, ll)                                      # the same sum recursion with and without the best alignment


def test_forward_ragged_batch_with_an_empty_target(ops):
    src_len, tgt_len = [9, 5, 1, 9, 3], [6, 0, 3, 2, 0]
    lb, lt = rr.random_lattice(5, 9, 7, seed=410)
    ll, best, emit = _run_forward(ops, lb, lt, src_len, tgt_len)
    _check_rows(lb, lt, src_len, tgt_len, ll, best, emit)
    assert abs(float(ll[1]) - float(lb[1, :5, 0].double().sum())) < 1e-5            # n == 0: the sum of the blanks
    assert float(best[1]) == float(ll[1])


@pytest.mark.parametrize("S,n", SHAPES)
def test_forward_closed_form(ops, S, n):
    half = torch.full((1, S, n + 1), math.log(0.5))
    ll, best, emit = _run_forward(ops, half, half, [S], [n])
    ref = rr.closed_form_ll(S, n)
    _, amax = rr.forward_ll(half[0], half[0], S, n)
    print(f"closed form (S {S}, n {n}): ll {float(ll[0]):.6f} ref {ref:.6f} bound {rr.ll_bound(S, n, amax):.3e}")
    assert abs(float(ll[0]) - ref) <= rr.ll_bound(S, n, amax), (float(ll[0]), ref)
    assert abs(float(best[0]) - (S + n) * math.log(0.5)) <= rr.ll_bound(S, n, (S + n) * math.log(2.0))


def test_forward_planted_path(ops):
    """lp_label log 0.9 at one chosen non-decreasing frame per token and log 0.01 elsewhere; blanks log 0.9 off the path"""
    S, n, B = 17, 12, 3
    gen = torch.Generator().manual_seed(420)
    lb = torch.full((B, S, n + 1), math.log(0.9))
    lt = torch.full((B, S, n + 1), math.log(0.01))
    planted = []
    for b in range(B):
        frames = sorted(torch.randint(0, S, (n,), generator=gen).tolist())
        if b == 0:
            frames[0], frames[-1] = 0, S - 1                          # a label in the first and in the last frame
        planted.append(frames)
        for u, s in enumerate(frames):
            lt[b, s, u] = math.log(0.9)
    ll, best, emit = _run_forward(ops, lb, lt, [S] * B, [n] * B)
    _check_rows(lb, lt, [S] * B, [n] * B, ll, best, emit, exact_emit=planted)


# ---------------------------------------------------------------------------------------------------------------- decoder / model
@pytest.fixture(scope="module")
def fix():
    g, g27 = np.load(G25), np.load(G27)
    w = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w:")}
    args = {k[5:]: g[k].item() for k in g.files if k.startswith("args.")}
    from simulst_amd.checkpoint import config_from_args
    cfg = replace(config_from_args(dict(args, arch="transducer_model_s")), vocab=w["decoder.embed_tokens.weight"].shape[0])
    enc = torch.from_numpy(g["enc_out"]).transpose(0, 1).contiguous()          # [B, T, D]
    enc_len = torch.from_numpy(g["enc_len"])
    prev = torch.from_numpy(g27["prev_output_tokens"])
    inp, labels, n = rr.lattice_inputs(prev, pad=cfg.padding_idx, eos=cfg.eos)
    logits = torch.from_numpy(g27["lattice_logits"]).double()                  # the reference's own lattice, read-only below
    lp = torch.log_softmax(logits, -1)
    lpb = lp[..., 0]
    lpl = lp.gather(3, labels.view(4, 1, 7, 1).expand(4, 10, 7, 1)).squeeze(3)
    src_len = g27["pooled_len"].tolist()
    return dict(g=g, w=w, cfg=cfg, enc=enc, enc_len=enc_len, prev=prev, inp=inp, labels=labels, n=n.tolist(), src_len=src_len,
                logits=logits, lpb=lpb, lpl=lpl, targets=[g27["targets"][b, :m].tolist() for b, m in enumerate(n.tolist())])


def _decoder(fix, dtype=torch.float32, **kw):
    from simulst_amd.transducer import TransducerDecoder
    return TransducerDecoder(fix["cfg"], fix["w"], device=DEV, dtype=dtype, **kw)


def test_forward_lattice_matches_g27(fix):
    dec = _decoder(fix)
    out = dec.forward_lattice(fix["prev"], fix["enc"].to(DEV), fix["enc_len"], return_logits=True)
    assert out["src_len"].cpu().tolist() == fix["src_len"] and out["tgt_len"].cpu().tolist() == fix["n"] == [6, 4, 1, 3]
    assert out["padding_mask"].cpu().tolist() == (torch.arange(10).view(1, -1) >= torch.tensor(fix["src_len"]).view(4, 1)).tolist()
    vb, vl = rr.valid_cells(fix["src_len"], fix["n"], 10, 7)
    assert out["logits"].shape == (4, 10, 7, 64) and out["logits"].dtype == torch.float32
    assert float((out["logits"].cpu().double() - fix["logits"])[vb].abs().max()) < 1e-4
    assert float((out["lp_blank"].cpu().double() - fix["lpb"])[vb].abs().max()) < 1e-4
    assert float((out["lp_label"].cpu().double() - fix["lpl"])[vl].abs().max()) < 1e-4
    assert bool((out["lp_blank"].cpu()[~vb] == 0).all()) and bool((out["lp_label"].cpu()[~vl] == 0).all())
    with pytest.raises(NotImplementedError, match="forward_lattice"):
        dec.forward(fix["prev"].to(DEV), encoder_out={"encoder_out": [fix["enc"].transpose(0, 1).to(DEV)]}, incremental_state=None)


def test_features_teacher_forced_match_the_prefix_features(fix):
    dec = _decoder(fix)
    feats = dec.features_teacher_forced(fix["inp"].to(DEV)).cpu().double()
    ref = tr.TransducerRef(fix["w"], heads=fix["cfg"].num_heads, downsample=fix["cfg"].downsample)
    for u in range(7):
        want = ref.features(fix["inp"][:, 1:u + 1])
        rows = [b for b in range(4) if u <= fix["n"][b]]               # positions behind a row's EOS hold pads
        assert float((feats[rows, u] - want[rows]).abs().max()) < 1e-4, u


def _model(fix, dtype=torch.float32):
    from simulst_amd.transducer import TransducerModel
    from simulst_amd.weights import init_model
    weights = dict(init_model(fix["cfg"], seed=1))
    weights.update(fix["w"])
    model = TransducerModel(fix["cfg"], weights, device=DEV, dtype=dtype)
    enc_len = fix["enc_len"].to(DEV)
    buf = fix["enc"].to(DEV, dtype)
    model.encoder.forward = lambda *a, **k: {"encoder_out_btd": buf, "encoder_lengths": enc_len}     # the fixture records decoder inputs
    return model


def test_score_reference_matches_the_restatement_on_g27(fix):
    model = _model(fix)
    hyps = model.score_reference(torch.zeros(4, 160, 80, device=DEV), torch.full((4,), 160), fix["targets"], return_alignments=True)
    plain = model.score_reference(torch.zeros(4, 160, 80, device=DEV), torch.full((4,), 160), fix["targets"])
    for b, h in enumerate(hyps):
        S, n = fix["src_len"][b], fix["n"][b]
        ll, amax = rr.forward_ll(fix["lpb"][b], fix["lpl"][b], S, n)
        best, emit = rr.best_alignment(fix["lpb"][b], fix["lpl"][b], S, n)
        # every one of the S + n cells on a path is within 1e-4 (the test above), the recursion within its own bound
        bound = (S + n) * 1e-4 + rr.ll_bound(S, n, amax)
        assert h["tokens"].tolist() == fix["targets"][b]
        assert abs(float(h["nll"]) + ll) <= bound and abs(float(h["score"]) - ll / n) <= bound
        off = -float(fix["lpl"][b, S - 1, :n].sum())
        assert abs(float(h["nll_offline"]) - off) <= n * 1e-4
        assert h["alignment"].tolist() == emit, (b, h["alignment"].tolist(), emit)
        want_pos = [float(fix["lpl"][b, s, u]) for u, s in enumerate(emit)]
        assert float((h["positional_scores"].double() - torch.tensor(want_pos, dtype=torch.float64)).abs().max()) < 1e-4
        assert plain[b]["alignment"] is None and float(plain[b]["nll"]) == float(h["nll"])
    with pytest.raises(AssertionError):
        model.score_reference(torch.zeros(1, 160, 80, device=DEV), torch.full((1,), 160), [[5, 6]])          # no EOS at the end


def test_bf16_lattice_and_score_within_the_composed_bounds(fix):
    """bf16: the lattice against fp64 from the decoder's OWN P and G (the lattice bound), the log-likelihood against the fp64
    recursion on that fp64 lattice: every cell of a path moves ll by at most its own error, then the recursion's bound"""
    dt = torch.bfloat16
    model = _model(fix, dt)
    dec = model.decoder
    out = dec.forward_lattice(fix["prev"], fix["enc"].to(DEV), fix["enc_len"])
    Wr = dec.w.out_proj.cpu()
    rb, rl, _ = rr.joiner_lattice(out["P"].cpu(), out["G"].cpu(), Wr, fix["labels"])
    vb, vl = rr.valid_cells(fix["src_len"], fix["n"], 10, 7)
    tol = tol_rows(Wr, dt)
    cell = 2 * float(tol.max()) + 64 * 2.0 ** -24 + 2.0 ** -20
    assert float((out["lp_blank"].cpu().double() - rb)[vb].abs().max()) <= cell
    assert float((out["lp_label"].cpu().double() - rl)[vl].abs().max()) <= cell
    hyps = model.score_reference(torch.zeros(4, 160, 80, device=DEV), torch.full((4,), 160), fix["targets"], return_alignments=True)
    for b, h in enumerate(hyps):
        S, n = fix["src_len"][b], fix["n"][b]
        ll, amax = rr.forward_ll(rb[b], rl[b], S, n)
        bound = (S + n) * cell + rr.ll_bound(S, n, amax)
        assert abs(float(h["nll"]) + ll) <= bound, (b, float(h["nll"]), ll, bound)
        assert abs(float(h["nll_offline"]) + float(rl[b, S - 1, :n].sum())) <= n * cell
        e = h["alignment"].tolist()
        opt, _ = rr.best_alignment(rb[b], rl[b], S, n)
        assert e == sorted(e) and all(0 <= x < S for x in e)
        assert abs(rr.path_score(rb[b], rl[b], S, n, e) - opt) <= 2 * bound


def test_the_lattice_is_not_materialised():
    """B = 2, S' = 40, U1 = 61, V = 4096: the fp32 logits would take 80 MB; the pass allocates less than 16 MB"""
    from simulst_amd.transducer import TransducerDecoder
    cfg, w, _, _ = _big_model(seed=31)
    dec = TransducerDecoder(cfg, w, device=DEV, dtype=torch.bfloat16, lattice_logits_cap_bytes=64 << 20)
    gen = torch.Generator().manual_seed(32)
    enc = torch.randn(2, 320, 256, generator=gen).to(DEV, torch.bfloat16)
    enc_len = torch.tensor([320, 200])
    prev = torch.randint(4, cfg.vocab, (2, 60), generator=gen)
    prev[:, 0] = cfg.eos
    prev[1, 40:] = cfg.padding_idx
    dec.forward_lattice(prev[:, :8], enc, enc_len)                    # position table, first-call setup
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = dec.forward_lattice(prev, enc, enc_len)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    assert out["lp_blank"].shape == (2, 40, 61) and out["tgt_len"].cpu().tolist() == [60, 40]
    assert 2 * 40 * 61 * 4096 * 4 > 79e6
    print(f"forward_lattice raised the allocated peak by {grown / 2 ** 20:.2f} MiB")
    assert grown < 16 << 20, grown
    assert bool(torch.isfinite(out["lp_blank"]).all()) and bool((out["lp_blank"][0] < 0).all())
    with pytest.raises(ValueError, match="lattice_logits_cap_bytes"):
        dec.forward_lattice(prev, enc, enc_len, return_logits=True)
