"""The transducer on the MI355X (csrc/transducer.hip, simulst_amd/transducer.py): the pooling, joiner-scan and emit kernels against
the fp64 restatement (tests/transducer_ref.py) computed from the kernels' own inputs, and the decoder / model against fixture g25
(the reference's own TransducerDecoder).  GPU only.

Tolerances of the joiner logits, per vocabulary row v, derived from the number formats: bf16 2^-8 sum_k |W[v, k]| (the bf16 half-ulp
of z = tanh(.), |z| < 1, plus as much for the tanh approximation; the fp32 accumulation over D <= 256 is negligible beside it),
fp32 2^-16 sum_k |W[v, k]|.  A decision (which column is best, blank or not) must be the fp64 one wherever the fp64 margin exceeds
the two tolerances involved; at most 10 % of the scanned positions may be excused that way."""
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

import transducer_ref as tr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G25 = os.path.join(ROOT, "tests", "golden", "g25_transducer.npz")
DEV = "cuda:0"
SENT_F, SENT_I = -777.0, -7


@pytest.fixture(scope="module")
def ops():
    from simulst_amd.ops import Ops
    return Ops()


@pytest.fixture(scope="module")
def g25():
    g = np.load(G25)
    w = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w:")}
    args = {k[5:]: g[k].item() for k in g.files if k.startswith("args.")}
    from simulst_amd.checkpoint import config_from_args
    cfg = replace(config_from_args(dict(args, arch="transducer_model_s")), vocab=w["decoder.embed_tokens.weight"].shape[0])
    enc = torch.from_numpy(g["enc_out"]).transpose(0, 1).contiguous()          # [B, T, D]
    return g, w, cfg, enc


def tol_rows(W, dtype):
    return W.double().abs().sum(1) * (2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -16)


# ---------------------------------------------------------------------------------------------------------------- pooling
def _pool_case(ops, x, lens, k, dtype):
    xd = x.to(dtype)
    y, n = ops.transducer_pool(xd.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), T_max=max(lens), k=k)
    ref, rn = tr.pool(xd, lens, k)                       # fp64 from the kernel's own (rounded) input
    assert n.cpu().tolist() == rn.tolist()
    y = y.cpu().double()
    assert y.shape == ref.shape
    for b, m in enumerate(rn.tolist()):
        assert bool((y[b, m:] == 0).all()), "padded positions are exactly zero"
    err = (y - ref).abs()
    # fp32 accumulation of a window: (k - 1) additions, a division and a product, each within 2^-24 relative of the running sum of
    # magnitudes -> below 1e-6 relative to the pooled magnitudes (the same pooling of |x|)
    acc = 1e-6 * tr.pool(xd.abs(), lens, k)[0]
    if dtype == torch.float32:
        bound = acc
    else:          # one bf16 ulp of the fp64 value (the rounding of the result), on top of the fp32 accumulation
        bound = 2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 7) + acc
    assert bool((err <= bound).all()), float((err - bound).max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pooling_g25_batch(ops, g25, dtype):
    g, _, cfg, enc = g25
    _pool_case(ops, enc, g["enc_len"].tolist(), cfg.downsample, dtype)
    if dtype == torch.float32:                             # ... and the reference's own output
        y, _ = ops.transducer_pool(enc.to(DEV), torch.from_numpy(g["enc_len"]).to(DEV, torch.int32), T_max=39, k=cfg.downsample)
        assert (y.cpu() - torch.from_numpy(g["pooled"]).transpose(0, 1)).abs().max() < 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pooling_bench_rows(ops, dtype):
    x = torch.randn(5, 250, 256, generator=torch.Generator().manual_seed(7))
    _pool_case(ops, x, [250, 249, 200, 8, 1], 8, dtype)


def test_pooling_reads_a_strided_batch_and_the_batch_T(ops):
    """rows of a wider buffer (the encoder returns a view behind its right-context blocks), and T below the buffer's rows"""
    big = torch.randn(3, 20, 64, generator=torch.Generator().manual_seed(8)).to(DEV)
    x = big[:, 4:]                                         # [3, 16, 64], batch stride 20 * 64
    lens = [11, 10, 5]
    y, n = ops.transducer_pool(x, torch.tensor(lens, dtype=torch.int32, device=DEV), T_max=11, k=4)
    ref, rn = tr.pool(x.cpu(), lens, 4, T=11)
    assert y.shape == (3, 3, 64) and n.cpu().tolist() == rn.tolist()
    assert (y.cpu().double() - ref).abs().max() < 1e-5
    # the quirk: row 1's last window is also the batch's clipped one -> sum / 3 * 4 / 2, 4/3 of the mean of its two valid rows
    assert torch.allclose(y[1, 2].cpu().double(), x[1, 8:10].cpu().double().mean(0) * 4 / 3, atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------- scan
def _scan_inputs(B, S, D, V, seed, integer_w=False):
    """confident joiner inputs: the pre-activation of (b, s) leans towards one token's row and towards the blank's, each by a
    random amount, as a trained model's does -- random gaussian rows would leave the best two of thousands of columns closer than
    any bf16 kernel can tell apart"""
    gen = torch.Generator().manual_seed(seed)
    if integer_w:
        W = torch.randint(-3, 4, (V, D), generator=gen).float() / 4.0      # asymmetric, exact in bf16: a transposed or permuted
        W[:, 0] += 0.25                                                   # fragment map gives other logits, not rounding noise
    else:
        W = torch.randn(V, D, generator=gen) * D ** -0.5
    tgt = torch.randint(1, V, (B, S), generator=gen)
    unit = W / W.norm(dim=-1, keepdim=True).clamp_min(1e-6) * D ** 0.5
    a_tok = 0.8 + 1.2 * torch.rand(B, S, 1, generator=gen)
    a_blank = 2.0 * torch.rand(B, S, 1, generator=gen)
    u = a_tok * unit[tgt] + a_blank * unit[0] + 0.3 * torch.randn(B, S, D, generator=gen)
    g = 0.3 * torch.randn(B, D, generator=gen)
    P = u - g.unsqueeze(1)
    src_len = torch.randint(1, S + 1, (B,), generator=gen)
    src_len[0] = S
    if B > 1:
        src_len[-1] = 1
    return P.contiguous(), g.contiguous(), W.contiguous(), src_len.to(torch.int32)


def _prev_emit(pattern, src_len, seed):
    if pattern == "zero":
        return torch.zeros_like(src_len)
    if pattern == "last":
        return src_len - 1
    gen = torch.Generator().manual_seed(seed + 1)
    return (torch.rand(src_len.shape, generator=gen) * src_len).floor().to(torch.int32).clamp_max(src_len - 1)


def _fold_parts(best, idx):
    """the scan's per-part (max, index) pairs -> one pair per position: the larger value, on a tie the lower index"""
    m = best.max(-1, keepdim=True).values
    cand = torch.where(best == m, idx, torch.full_like(idx, 2 ** 31 - 1))
    return m.squeeze(-1), cand.min(-1).values


def _run_scan(ops, P, g, W, prev_emit, src_len, dtype):
    from simulst_amd.ops import Ops
    B, S, D = P.shape
    V = W.shape[0]
    Wd = W.to(dtype).to(DEV)
    n_split = Ops.joiner_split(B, S, V, dtype)
    blank = torch.full((B, S), SENT_F, device=DEV)
    best = torch.full((B, S, n_split), SENT_F, device=DEV)
    idx = torch.full((B, S, n_split), SENT_I, device=DEV, dtype=torch.int32)
    ops.joiner_scan(P.to(DEV), g.to(DEV), ops.pack_joiner_weight(Wd), prev_emit.to(DEV), src_len.to(DEV), blank, best, idx, V=V)
    torch.cuda.synchronize()
    return blank.cpu(), best.cpu(), idx.cpu(), n_split


SCAN_SHAPES = [(3, 10, 32, 64), (2, 1, 32, 64), (5, 33, 256, 203), (64, 32, 256, 4096), (1, 40, 256, 4099)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("pattern", ["zero", "last", "random"])
@pytest.mark.parametrize("shape", SCAN_SHAPES)
def test_joiner_scan_against_fp64(ops, shape, pattern, dtype):
    B, S, D, V = shape
    seed = 100 + 7 * B + S
    P, g, W, src_len = _scan_inputs(B, S, D, V, seed, integer_w=(shape == SCAN_SHAPES[0] and pattern == "random"))
    pe = _prev_emit(pattern, src_len, seed)
    blank, best, idx, n_split = _run_scan(ops, P, g, W, pe, src_len, dtype)
    Wr = W.to(dtype)
    ref = tr.joiner_logits(P, g, Wr)                                   # fp64, on the dtype-rounded W
    tol = tol_rows(Wr, dtype)
    s_idx = torch.arange(S).view(1, S)
    scanned = (s_idx >= pe.view(B, 1)) & (s_idx < src_len.view(B, 1))
    # outside [prev_emit, src_len'): untouched
    assert bool((blank[~scanned] == SENT_F).all()) and bool((best[~scanned] == SENT_F).all()) and bool((idx[~scanned] == SENT_I).all())
    kb, ki = _fold_parts(best, idx)
    kb, ki, kblank, r = kb[scanned].double(), ki[scanned].long(), blank[scanned].double(), ref[scanned]
    n = r.shape[0]
    assert n > 0 and bool(((ki >= 1) & (ki < V)).all())
    # values: the blank logit, and the best non-blank at the column the kernel names
    assert bool(((kblank - r[:, 0]).abs() <= tol[0]).all()), float((kblank - r[:, 0]).abs().max())
    at = r.gather(1, ki.view(n, 1)).squeeze(1)
    assert bool(((kb - at).abs() <= tol[ki]).all()), float(((kb - at).abs() - tol[ki]).max())
    # decisions where fp64 is clear
    nb = r.clone()
    nb[:, 0] = -float("inf")
    top = nb.topk(2, dim=1)
    tol_nb = tol[1:].max()
    clear_idx = (top.values[:, 0] - top.values[:, 1]) > 2 * tol_nb
    clear_blank = (top.values[:, 0] - r[:, 0]).abs() > tol[0] + tol_nb
    assert bool((ki[clear_idx] == top.indices[clear_idx, 0]).all())
    assert bool(((kb > kblank)[clear_blank] == (top.values[:, 0] > r[:, 0])[clear_blank]).all())
    excused = 1.0 - float((clear_idx & clear_blank).double().mean())
    print(f"shape {shape} {pattern} {dtype}: {n} scanned, n_split {n_split}, excused {excused:.3f}, "
          f"max blank err / tol {float(((kblank - r[:, 0]).abs() / tol[0]).max()):.3f}")
    assert excused <= 0.10, excused


def test_emit_kernel_from_scan_outputs(ops):
    """hand-made scan outputs: first winning position, the forced emit at src_len' - 1, ties to the blank, parts folded, clamping"""
    B, S, D, V, n_split = 5, 6, 32, 64, 2
    P = torch.randn(B, S, D, generator=torch.Generator().manual_seed(3))
    g = torch.randn(B, D, generator=torch.Generator().manual_seed(4))
    blank = torch.zeros(B, S)
    best = torch.full((B, S, n_split), -1.0)
    idx = torch.full((B, S, n_split), 5, dtype=torch.int32)
    src_len = torch.tensor([6, 6, 4, 1, 6], dtype=torch.int32)
    prev = torch.tensor([0, 2, 0, 0, 99], dtype=torch.int32)          # row 4: out of range, clamped to 5
    best[0, 3, 1] = 0.5                                                 # row 0: position 3, through the second part
    best[1, 1, 0] = 9.0                                                 # row 1: a win BEFORE prev_emit is not looked at ...
    best[1, 4, 0] = 0.0                                                 # ... a tie goes to the blank (lower column) ...
    # ... so row 1 is forced at 5; row 2: nothing wins, forced at src_len' - 1 = 3; row 3: S' = 1; row 4: starts at 5
    z = torch.empty(B, D, device=DEV)
    at_eos = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    pd = prev.to(DEV)
    ops.joiner_emit(P.to(DEV), g.to(DEV), blank.to(DEV), best.to(DEV), idx.to(DEV), pd, src_len.to(DEV), z, at_eos, V=V)
    assert pd.cpu().tolist() == [3, 5, 3, 0, 5]
    assert at_eos.cpu().tolist() == [0, 1, 1, 1, 1]
    want = torch.tanh(P[torch.arange(B), pd.cpu().long()].double() + g.double())
    assert (z.cpu().double() - want).abs().max() < 1e-6
    logits = torch.ones(B, V, device=DEV)
    ops.joiner_mask_blank(logits, at_eos)
    assert logits[:, 0].cpu().tolist() == [1.0, -1e4, -1e4, -1e4, -1e4] and bool((logits[:, 1:] == 1).all())


# ---------------------------------------------------------------------------------------------------------------- step / greedy
def _decoder(cfg, w, dtype=torch.float32):
    from simulst_amd.transducer import TransducerDecoder
    return TransducerDecoder(cfg, w, device=DEV, dtype=dtype)


def test_teacher_forced_steps_match_g25(g25):
    g, w, cfg, enc = g25
    dec = _decoder(cfg, w)
    B = enc.shape[0]
    st = dec.new_state(B)
    dec.set_source(st, enc.to(DEV), torch.from_numpy(g["enc_len"]))
    assert st.src_len.cpu().tolist() == g["pooled_len"].tolist()
    forced = torch.from_numpy(g["forced"]).to(DEV)
    toks = torch.full((B,), cfg.eos, device=DEV, dtype=torch.int64)           # the first token is read as bos whatever it is
    for t in range(forced.shape[1]):
        logits = dec.step(st, toks)
        err = float((logits.cpu() - torch.from_numpy(g["step_logits"][t])).abs().max())
        assert err < 1e-4, (t, err)
        assert st.prev_emit.cpu().tolist() == g["step_emit"][t].tolist(), t
        dec.commit(st)
        toks = forced[:, t].contiguous()


def test_generate_offline_matches_g25(g25):
    from simulst_amd.transducer import TransducerModel
    from simulst_amd.weights import init_model
    g, w, cfg, enc = g25
    weights = dict(init_model(cfg, seed=1))
    weights.update(w)
    model = TransducerModel(cfg, weights, device=DEV)
    enc_len = torch.from_numpy(g["enc_len"]).to(DEV)
    # the fixture records decoder inputs: the encoder's output is g25's states, in a buffer with more rows than T
    buf = torch.zeros(enc.shape[0], enc.shape[1] + 5, enc.shape[2], device=DEV)
    buf[:, :enc.shape[1]] = enc.to(DEV)
    model.encoder.forward = lambda *a, **k: {"encoder_out_btd": buf, "encoder_lengths": enc_len}
    n = g["greedy"].shape[1]
    toks, info = model.generate_offline(torch.zeros(4, 160, 80, device=DEV), torch.full((4,), 160), n_steps=n)
    assert toks.cpu().tolist() == g["greedy"].tolist()
    assert info["emit"].cpu().tolist() == g["greedy_emit"].tolist()
    from simulst_amd.model import refuse_offline_model
    with pytest.raises(ValueError, match="transducer_model"):
        refuse_offline_model(model, "agent")


def _big_model(seed=11):
    from simulst_amd.config import transducer_model_s
    from simulst_amd.weights import init_model
    cfg = transducer_model_s(encoder_layers=1, decoder_layers=2)
    w = dict(init_model(cfg, seed=seed))
    out = w["decoder.output_projection.weight"].clone()                      # untied, the blank row scaled so that it wins at times
    out[0] *= 6.0
    w["decoder.output_projection.weight"] = w["decoder.joiner.output_projection.weight"] = out
    w["decoder.joiner.target_projection.weight"] = w["decoder.joiner.target_projection.weight"] * 3.0
    w["decoder.joiner.source_projection.weight"] = w["decoder.joiner.source_projection.weight"] * 4.0
    lens = [96, 95, 64, 33, 9, 1]
    enc = torch.randn(6, 96, 256, generator=torch.Generator().manual_seed(seed + 1))
    enc = enc.masked_fill((torch.arange(96).view(1, 96) >= torch.tensor(lens).view(6, 1)).unsqueeze(-1), 0.0)
    return cfg, w, enc, lens


def test_greedy_at_model_size_against_the_restatement():
    cfg, w, enc, lens = _big_model()
    n = 12
    ref = tr.TransducerRef(w, heads=cfg.num_heads, downsample=cfg.downsample)
    ref.set_source(enc, lens)
    rt, re_, margins = ref.run_greedy(n)
    dec = _decoder(cfg, w)
    toks, emit, _ = dec.greedy_offline(enc.to(DEV), torch.tensor(lens), n)
    toks, emit = toks.cpu(), emit.cpu().long()
    # a row is compared up to its first unclear step (the trajectories may part there); at most 10 % of the steps are excused
    clear = (margins.t() > 1e-3).long().cumprod(1).bool()                 # [B, n]
    assert float((~clear).double().mean()) <= 0.10
    assert bool((toks[clear] == rt[clear]).all()) and bool((emit[clear] == re_[clear]).all())
    assert len(set(re_.flatten().tolist())) > 3, "the emit positions move"


def test_bf16_steps_against_the_fp64_joiner_of_their_own_buffers():
    cfg, w, enc, lens = _big_model(seed=21)
    dt = torch.bfloat16
    dec = _decoder(cfg, w, dt)
    B, V = len(lens), cfg.vocab
    st = dec.new_state(B)
    dec.set_source(st, enc.to(DEV), torch.tensor(lens))
    Wr = dec.w.out_proj.cpu()
    tol = tol_rows(Wr, dt)
    tol_nb = tol[1:].max()
    forced = torch.randint(4, V, (B, 12), generator=torch.Generator().manual_seed(5))
    toks = torch.zeros(B, device=DEV, dtype=torch.int64)
    last_emit = torch.zeros(B, dtype=torch.long)
    n_dec = n_excused = 0
    for t in range(forced.shape[1]):
        before = st.prev_emit.cpu().clone()
        logits = dec.step(st, toks).cpu().double()
        emit = st.prev_emit.cpu().long()
        ref = tr.joiner_logits(st.P.cpu(), st.g.cpu(), Wr)               # fp64 from the kernel's own P and g
        ne, rows, margins = tr.emit_decisions(ref, before, st.src_len.cpu())
        for b in range(B):
            n_dec += 1
            if min(margins[b]) > tol[0] + tol_nb:
                assert int(emit[b]) == int(ne[b]), (t, b)
            else:
                n_excused += 1
            row = ref[b, emit[b]].clone()                                 # the returned row, at the KERNEL's emit
            if int(emit[b]) == int(st.src_len[b]) - 1:
                row[0] = tr.BLANK_AT_EOS
            assert bool(((logits[b] - row).abs() <= tol).all()), (t, b, float(((logits[b] - row).abs() - tol).max()))
        assert bool((emit >= last_emit).all()) and bool((emit <= st.src_len.cpu().long() - 1).all())
        last_emit = emit
        pick = dec.ops.greedy_argmax(logits.float().to(DEV), pad_idx=cfg.padding_idx, eos_idx=cfg.eos, mask_eos=t == 0)
        assert bool((pick != cfg.padding_idx).all())
        dec.commit(st)
        toks = forced[:, t].to(DEV).contiguous()
    print(f"bf16 steps: {n_dec} emit decisions, {n_excused} excused")
    assert n_excused <= 0.10 * n_dec


def test_forward_surface(g25):
    g, w, cfg, enc = g25
    dec = _decoder(cfg, w)
    B = enc.shape[0]
    pad = torch.arange(enc.shape[1]).view(1, -1) >= torch.from_numpy(g["enc_len"]).view(B, 1)
    eo = {"encoder_out": [enc.transpose(0, 1).to(DEV)], "encoder_padding_mask": [pad.to(DEV)]}
    forced = torch.from_numpy(g["forced"])
    inc = {}
    for t in range(6):
        prev = torch.cat([torch.full((B, 1), cfg.eos), forced[:, :t]], 1).to(DEV)
        logits, extra = dec.forward(prev, encoder_out=eo, incremental_state=inc)
        assert logits.shape == (B, 1, cfg.vocab)
        assert float((logits[:, 0].cpu() - torch.from_numpy(g["step_logits"][t])).abs().max()) < 1e-4
        assert inc[dec.STATE_KEY].prev_emit.cpu().tolist() == g["step_emit"][t].tolist()
        assert extra["padding_mask"].cpu().tolist() == (torch.arange(10).view(1, -1) >= torch.from_numpy(g["pooled_len"]).view(B, 1)).tolist()
        if t in (2, 4):          # a discarded prediction: the same prefix again, no rollback call in between
            again, _ = dec.forward(prev, encoder_out=eo, incremental_state=inc)
            assert torch.equal(again, logits)
            assert inc[dec.STATE_KEY].prev_emit.cpu().tolist() == g["step_emit"][t].tolist()
    with pytest.raises(NotImplementedError):
        dec.forward(prev, encoder_out=eo, incremental_state=None)
    with pytest.raises(NotImplementedError):
        dec.reorder_incremental_state(inc, torch.arange(B))
