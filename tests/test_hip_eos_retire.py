"""Offline decode with hypotheses finalised at EOS (MMADecoder.generate_offline, simulst_mma_retire_rows): fairseq's
SequenceGenerator at beam 1 drops a hypothesis from the batch at its first EOS or at its cap (eval/generate.py:187-209); the
product compacts the live rows to the front of the batch on the device between chunks of steps.  GPU only.

Random-init weights almost never emit EOS, so the batches here decode with an untied output projection whose EOS row is scaled,
calibrated against the non-retiring decode so that a good share of the rows end at EOS before their cap, on many different steps,
and some still run to the cap."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu


def _biased(w, cfg, alpha, seed=5):
    """an untied output projection (random rows) whose EOS row is scaled by alpha"""
    w = dict(w)
    W = torch.randn(cfg.vocab, cfg.embed_dim, generator=torch.Generator().manual_seed(seed)) * cfg.embed_dim ** -0.5
    W[cfg.eos] *= alpha
    w["decoder.output_projection.weight"] = W
    return w


def _ends(toks, caps, eos):
    """per row: tokens kept (through the first EOS, at most the cap) and whether the row ended at EOS before its cap"""
    out = []
    for r, c in enumerate(caps):
        row = toks[r, :c].tolist()
        k = row.index(eos) + 1 if eos in row else c
        out.append((k, eos in row[:k] and k <= c))
    return out


def _lengths(n, lo, hi, seed, uniform=False):
    if uniform:
        return [hi] * n
    return sorted(torch.randint(lo, hi, (n,), generator=torch.Generator().manual_seed(seed)).tolist(), reverse=True)


@pytest.fixture(scope="module")
def bf16_model():
    """mma_model_s (6 decoder layers, D = 256, bf16: the layer chains from 129 rows on), wait-k 3, EOS row calibrated on a
    448-row ragged batch: >= 1/3 of the rows end at EOS before their cap, on >= 12 different steps, some run to the cap"""
    from simulst_amd.config import mma_model_s
    from simulst_amd.model import SimulSTModel
    from simulst_amd.offline_eval import decode_batch, make_batch, max_steps
    from simulst_amd.weights import init_model
    cfg = mma_model_s(simul_attn_type="waitk_fixed_pre_decision", waitk_lagging=3)
    w0 = init_model(cfg, seed=999)
    lengths = _lengths(448, 120, 1200, 448)
    batch = make_batch(list(range(448)), lengths, "cuda", torch.bfloat16)
    caps = [max_steps(t) for t in lengths]
    for alpha in (2.0, 2.5, 3.0, 3.5, 4.0, 5.0):
        model = SimulSTModel(cfg, _biased(w0, cfg, alpha), dtype=torch.bfloat16)
        with torch.no_grad():
            toks = decode_batch(model, batch, retire=False).cpu()
        ends = _ends(toks, caps, cfg.eos)
        early = [k for k, e in ends if e and k < caps[0]]
        if len(early) >= 448 // 3 and len(set(early)) >= 12 and any(not e for _, e in ends):
            return cfg, model, alpha
    pytest.fail("no EOS scaling gives the wanted mix of EOS-finished and capped rows")


def _check_rows(got, ref, caps, eos, pad):
    """got (stop_at_eos) against ref (every row to its cap): per row identical through the first EOS or the cap, padding behind"""
    n_eos, bad = 0, 0
    for r, c in enumerate(caps):
        row = ref[r, :c].tolist()
        k = row.index(eos) + 1 if eos in row else c
        n_eos += int(k < c or row[k - 1] == eos)
        bad += int(got[r, :k].tolist() != row[:k] or bool((got[r, k:] != pad).any()))
    return n_eos, bad


@pytest.mark.parametrize("n,uniform", [(100, False), (100, True), (330, False), (330, True), (448, False), (448, True),
                                       (1100, False), (1100, True)])
def test_hypotheses_unchanged_bf16(bf16_model, n, uniform):
    """every kernel class (<= 128 rows: fused query projection; 129-1024: the layer chains; > 1024): the hypotheses of
    decode_batch(stop_at_eos=True) are bit for bit the tokens of decode_batch(retire=False) through each row's first EOS or cap,
    padding behind, and their lengths are trim_hypotheses'"""
    from simulst_amd.offline_eval import decode_batch, make_batch, max_steps, trim_hypotheses
    cfg, model, _ = bf16_model
    lengths = _lengths(n, 120, 1200, n + 7, uniform=uniform)
    batch = make_batch(list(range(n)), lengths, "cuda", torch.bfloat16)
    with torch.no_grad():
        got = decode_batch(model, batch, stop_at_eos=True).cpu()
        ref = decode_batch(model, batch, retire=False).cpu()
    caps = [max_steps(t) for t in lengths]
    n_eos, bad = _check_rows(got, ref, caps, cfg.eos, cfg.padding_idx)
    assert bad == 0, (n, uniform, bad)
    assert n_eos >= n // 4, n_eos                   # the batch does exercise EOS retirement
    assert torch.equal((got != cfg.padding_idx).sum(1), trim_hypotheses(ref, batch[2], cfg.eos))


def test_against_the_oracle_fp32():
    """16 rows with the batch cap for all (oracle.agent.greedy_offline): rows that end at EOS before the cap have the oracle's
    tokens and length; rows at the cap match on cap - 1 tokens (the oracle forces EOS at its last step, the product keeps its cap
    convention)"""
    from oracle import agent as oag
    from oracle.configs import from_model_config
    from simulst_amd.config import tiny
    from simulst_amd.model import SimulSTModel
    from simulst_amd.weights import init_model
    cfg = tiny(waitk_lagging=3)
    w0 = init_model(cfg, seed=999)
    ecfg, dcfg = from_model_config(cfg)
    fb = torch.randn(16, 240, 80, generator=torch.Generator().manual_seed(11))
    L = torch.tensor([240 - 9 * i for i in range(16)])
    for i in range(16):
        fb[i, int(L[i]):] = 0
    U = 24
    for alpha in (2.0, 3.0, 4.0, 6.0):
        w = _biased(w0, cfg, alpha)
        ref, ref_len, _ = oag.greedy_offline(w, ecfg, dcfg, fb, L, n_steps=U, mask_eos=False)
        early = int((ref_len < U).sum())
        if 16 // 3 <= early < 16:
            break
    else:
        pytest.fail("no EOS scaling ends between a third and all but one of the 16 rows early")
    model = SimulSTModel(cfg, w, dtype=torch.float32)
    with torch.no_grad():
        enc = model.encoder.forward(fb.cuda(), L.cuda())
        toks, lengths, stats = model.decoder.generate_offline(enc["encoder_out_btd"], enc["encoder_lengths"], [U] * 16)
    toks, lengths = toks.cpu(), lengths.cpu()
    for r in range(16):
        n = int(ref_len[r])
        if n < U:
            assert int(lengths[r]) == n and toks[r, :n].tolist() == ref[r, :n].tolist(), r
            assert (toks[r, n:] == cfg.padding_idx).all()
        else:
            assert int(lengths[r]) == U and toks[r, :U - 1].tolist() == ref[r, :U - 1].tolist(), r
    assert stats["calls"] >= 1 and stats["row_steps"] <= 16 * U


@pytest.mark.parametrize("attn", ["waitk_fixed_pre_decision", "hard_aligned_fixed_pre_decision", "infinite_lookback_fixed_pre_decision"])
def test_every_per_row_buffer_moves(attn):
    """one direct call of simulst_mma_retire_rows after a chunk of decode steps, with EOS planted in chosen rows of the chunk's
    tokens: every live slot in front of the live count holds, in its valid regions, exactly what its source slot held (self K/V,
    cross K/V, soft keys, pooled keys, head_step, n_prev, enc_len, enc_len_bh, row_cap, last_tokens); dead rows are out of
    slot_row; the hypotheses hold the chunk's tokens through the planted EOS"""
    from simulst_amd.config import tiny
    from simulst_amd.model import SimulSTModel
    from simulst_amd.weights import init_model
    kw = dict(simul_attn_type=attn, fixed_pre_decision_ratio=4, fixed_pre_decision_type="average")
    if attn.startswith("waitk"):
        kw["waitk_lagging"] = 3
    cfg = tiny(**kw)
    model = SimulSTModel(cfg, init_model(cfg, seed=999), dtype=torch.float32)
    dec = model.decoder
    B, S, n_steps, U = 40, 72, 5, 12
    g = torch.Generator().manual_seed(3)
    enc = torch.randn(B, S, cfg.embed_dim, generator=g).cuda()
    enc_len = torch.randint(20, S + 1, (B,), generator=g).cuda()
    st = dec._offline_state(B, U, S, None, None)
    dec.append_encoder_out(st, enc, enc_len)
    st.enc_len = st.enc_len.clone()
    # learned policies with 'average' pre-decision cache pooled keys; infinite lookback has its own soft keys as well
    assert (st.Kpool is not None) == (not attn.startswith("waitk")) and (st.Ksoft is not None) == attn.startswith("infinite")
    toks = st.tok_buf.fill_(cfg.eos)
    chunk = dec.decode_steps(st, toks, n_steps, False).clone()
    # plant EOS: rows 3 k at step k % n_steps; row 5 reaches its cap (3) inside the chunk; what ends a row is read off the tokens
    for r in range(0, B, 3):
        chunk[(r // 3) % n_steps, r] = cfg.eos
    row_cap = torch.full((B,), U, dtype=torch.int32, device="cuda")
    row_cap[5] = 3
    cc, caps = chunk.cpu(), row_cap.tolist()
    want = {}
    for r in range(B):
        col = cc[:min(n_steps, caps[r]), r].tolist()
        want[r] = col[:col.index(cfg.eos) + 1] if cfg.eos in col else col
    live = [r for r in range(B) if cfg.eos not in want[r] and len(want[r]) < caps[r]]
    assert 8 <= len(live) < B - 8
    snap = {n: [t.clone() for t in getattr(st, n)] for n in ("k_cache", "v_cache", "Kmono", "V", "head_step")}
    if st.Ksoft is not None:
        snap["Ksoft"] = [t.clone() for t in st.Ksoft]
    if st.Kpool is not None:
        snap["Kpool"] = [t.clone() for t in st.Kpool]
    n_prev0, enc_len0, bh0 = st.n_prev.clone(), st.enc_len.clone(), st.enc_len_bh.clone()
    slot_row = torch.arange(B, dtype=torch.int32, device="cuda")
    last = (torch.arange(B, device="cuda") + 100).to(torch.int64)
    hyp = torch.full((B, U), cfg.padding_idx, dtype=torch.int64, device="cuda")
    res = torch.zeros(4 + 2 * B, dtype=torch.int32, device="cuda")
    d = dec._decoder_desc(st, st.n_prev_host)
    h = dec.ops.h
    h.check(dec.ops.lib.simulst_mma_retire_rows(h.ptr, C.byref(d), st.layer_structs, chunk.data_ptr(), n_steps, B, B,
                                                slot_row.data_ptr(), row_cap.data_ptr(), last.data_ptr(), hyp.data_ptr(), U,
                                                st.enc_len_bh.data_ptr(), res.data_ptr()), "simulst_mma_retire_rows")
    torch.cuda.synchronize()
    n_live = int(res[0])
    assert n_live == len(live) and int(res[1]) == min(B, (n_live + 15) // 16 * 16)
    sr = slot_row.cpu().tolist()
    assert sorted(sr[:n_live]) == live and all(x == -1 for x in sr[n_live:])
    # stable: a live row in front of the live count stays, the k-th live row behind it fills the k-th hole
    holes = [k for k in range(n_live) if k not in live]
    assert all(sr[k] == k for k in range(n_live) if k in live)
    assert [sr[k] for k in holes] == [r for r in live if r >= n_live]
    H = cfg.num_heads
    moved = 0
    for k in range(n_live):
        src = sr[k]                                      # slot_row started as the identity: the source slot is the row
        moved += int(src != k)
        np_, el = int(n_prev0[src]), int(enc_len0[src])
        assert int(st.n_prev[k]) == np_ and int(st.enc_len[k]) == el and int(row_cap[k]) == U and int(last[k]) == src + 100
        assert torch.equal(st.enc_len_bh[k * H:(k + 1) * H], bh0[src * H:(src + 1) * H])
        for l in range(cfg.decoder_layers):
            assert torch.equal(st.k_cache[l][k, :, :np_], snap["k_cache"][l][src, :, :np_])
            assert torch.equal(st.v_cache[l][k, :, :np_], snap["v_cache"][l][src, :, :np_])
            assert torch.equal(st.Kmono[l][k, :, :el], snap["Kmono"][l][src, :, :el])
            assert torch.equal(st.V[l][k, :, :el], snap["V"][l][src, :, :el])
            assert torch.equal(st.head_step[l][k * H:(k + 1) * H], snap["head_step"][l][src * H:(src + 1) * H])
            if "Ksoft" in snap:
                assert torch.equal(st.Ksoft[l][k, :, :el], snap["Ksoft"][l][src, :, :el])
            if "Kpool" in snap:
                npl = min(st.P_cap, el // cfg.pre_decision_ratio)
                assert npl > 0 and torch.equal(st.Kpool[l][k, :, :npl], snap["Kpool"][l][src, :, :npl])
    assert moved > 0
    hc = hyp.cpu()
    for r in range(B):
        k = len(want[r])
        assert hc[r, :k].tolist() == want[r] and (hc[r, k:] == cfg.padding_idx).all(), r


def test_work_shrinks(bf16_model):
    """half the rows ending before half the cap: far fewer row-steps than B x U, never fewer rows than the class floor of the
    batch; every row ending in the first chunk: one decode call; no EOS (random tied weights): the tokens of the full-batch decode
    and as many decode calls as the existing ragged path (whose tokens may differ from both where its prefix drops below 256 rows
    and a near-tied pick flips with the GEMM kernel)"""
    from simulst_amd.config import mma_model_s
    from simulst_amd.model import SimulSTModel
    from simulst_amd.offline_eval import make_batch, max_steps
    from simulst_amd.weights import init_model
    cfg, model, alpha = bf16_model
    n = 448
    lengths = _lengths(n, 500, 1200, 91)
    fb, Ld, L, steps, Tpad = make_batch(list(range(n)), lengths, "cuda", torch.bfloat16)
    caps = [max_steps(t) for t in lengths]
    kw = dict(s_cap=Tpad // 4 + 1, cap=(steps + 2 + 31) // 32 * 32)
    with torch.no_grad():
        enc = model.encoder.forward(fb, Ld)
        toks, lengths_t, stats = model.decoder.generate_offline(enc["encoder_out_btd"], enc["encoder_lengths"], caps, **kw)
    U = max(caps)
    ln = lengths_t.cpu()
    if int((ln < U // 2).sum()) >= n // 2:
        assert stats["row_steps"] < 0.75 * n * U, stats
    else:
        assert stats["row_steps"] < n * U
    assert min(stats["rows"]) >= 256 and stats["rows"][0] == n        # the 64 x 64 tile GEMMs' class of a 448-row batch

    # every row ends at its first free step (EOS is masked at position 0 only): a constant final LayerNorm output that the EOS row
    # of the projection dominates -> one decode call, nothing behind the EOS
    w = _biased(init_model(cfg, seed=999), cfg, 1.0)
    w["decoder.layer_norm.weight"] = torch.zeros(cfg.embed_dim)
    w["decoder.layer_norm.bias"] = torch.full((cfg.embed_dim,), 0.1)
    w["decoder.output_projection.weight"][cfg.eos] = 10.0
    eos_now = SimulSTModel(cfg, w, dtype=torch.bfloat16)
    with torch.no_grad():
        enc = eos_now.encoder.forward(fb, Ld)
        toks, lengths_t, stats = eos_now.decoder.generate_offline(enc["encoder_out_btd"], enc["encoder_lengths"], caps, **kw)
    assert stats["calls"] == 1 and (lengths_t == 2).all()
    assert (toks[:, 1] == cfg.eos).all() and (toks[:, 2:] == cfg.padding_idx).all()

    # no EOS to speak of (random tied weights): the tokens and the number of decode calls of greedy_offline_ragged
    plain = SimulSTModel(cfg, init_model(cfg, seed=999), dtype=torch.bfloat16)
    dec = plain.decoder
    calls = []
    orig = dec.decode_steps
    dec.decode_steps = lambda *a, **k: (calls.append(k.get("rows")), orig(*a, **k))[1]
    try:
        with torch.no_grad():
            enc = plain.encoder.forward(fb, Ld)
            dec.greedy_offline_ragged(enc["encoder_out_btd"], enc["encoder_lengths"], caps, False, **kw)
            n_ref = len(calls)
            ref = dec.greedy_offline(enc["encoder_out_btd"], enc["encoder_lengths"], U, False, **kw)[0].clone()
            del calls[n_ref:]
            got, lengths_t, stats = dec.generate_offline(enc["encoder_out_btd"], enc["encoder_lengths"], caps, **kw)
    finally:
        del dec.decode_steps
    n_eos, bad = _check_rows(got.cpu(), ref.cpu(), caps, cfg.eos, cfg.padding_idx)
    assert bad == 0 and n_eos <= n // 50
    assert stats["calls"] == n_ref == len(calls) - n_ref


@pytest.mark.parametrize("n", [1, 37])
def test_edges(bf16_model, n):
    """B = 1 and a batch that is not a whole number of 16-row tiles, rows in no particular order"""
    from simulst_amd.offline_eval import decode_batch, make_batch, max_steps
    cfg, model, _ = bf16_model
    lengths = torch.randint(150, 900, (n,), generator=torch.Generator().manual_seed(n)).tolist()
    fb, Ld, L, steps, Tpad = make_batch(list(range(n)), lengths, "cuda", torch.bfloat16)
    caps = [max_steps(t) for t in lengths]
    with torch.no_grad():
        enc = model.encoder.forward(fb, Ld)
        got, lengths_t, stats = model.decoder.generate_offline(enc["encoder_out_btd"], enc["encoder_lengths"], caps,
                                                               s_cap=Tpad // 4 + 1)
        ref, _ = model.decoder.greedy_offline(enc["encoder_out_btd"], enc["encoder_lengths"], max(caps), False,
                                              s_cap=Tpad // 4 + 1)
    n_eos, bad = _check_rows(got.cpu(), ref.cpu(), caps, cfg.eos, cfg.padding_idx)
    assert bad == 0
    assert torch.equal(lengths_t.cpu(), (got.cpu() != cfg.padding_idx).sum(1))
