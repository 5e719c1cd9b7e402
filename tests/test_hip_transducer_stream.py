"""Simultaneous decoding of the transducer on the MI355X: the OPEN-source form of the joiner scan / emit kernels (src_len < 0:
-1 - src_len positions are available, nothing is forced, a row may wait), the decoder's growing source (open_source /
append_source / step_online) and the agents (simulst_amd/transducer_agent.py).  GPU only.

Decisions are held to the fp64 restatement (tests/transducer_ref.py, the streaming loop of tests/transducer_stream_ref.py) under the
excuse rule and tolerances of tests/test_hip_transducer.py:5-8: a decision must be the fp64 one wherever the fp64 margin exceeds the
derived tolerances (tol_rows; 1e-3 for an fp32 trajectory, as test_greedy_at_model_size_against_the_restatement); at most 10 % may
be excused.  Every streaming test first asserts, on the REFERENCE's records, that at least two rows READ between two WRITEs."""
import pytest
import torch

import transducer_ref as tr
import transducer_stream_ref as sr
from test_hip_transducer import _big_model, _fold_parts, _scan_inputs, tol_rows

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT_F, SENT_I = -777.0, -7
K = 8                       # cfg.downsample of transducer_model_s
CHUNK = 16                  # encoder rows per chunk in the decoder tests (the Emformer segment)


@pytest.fixture(scope="module")
def ops():
    from simulst_amd.ops import Ops
    return Ops()


# ---------------------------------------------------------------------------------------------------------------- kernels
def _joiner_call(ops, P, g, Wd, W_fm, pe, src_len, dtype, mode, group):
    """scan + emit through the plain entry points (mode "plain", group 1) or the _beam ones -> every output on the host.
    P [Bs, S, D], g / pe [R = Bs * group], src_len [Bs]; all buffers pre-filled with sentinels."""
    from simulst_amd.ops import Ops
    Bs, S, D = P.shape
    R, V = g.shape[0], Wd.shape[0]
    n_split = Ops.joiner_split(R, S, V, dtype)
    blank = torch.full((R, S), SENT_F, device=DEV)
    best = torch.full((R, S, n_split), SENT_F, device=DEV)
    idx = torch.full((R, S, n_split), SENT_I, device=DEV, dtype=torch.int32)
    z = torch.full((R, D), SENT_F, device=DEV, dtype=dtype)
    at_eos = torch.full((R,), SENT_I, device=DEV, dtype=torch.int32)
    log = torch.full((R,), SENT_I, device=DEV, dtype=torch.int32)
    ped, sl = pe.to(DEV).contiguous(), src_len.to(DEV).contiguous()
    if mode == "plain":
        ops.joiner_scan(P, g, W_fm, ped, sl, blank, best, idx, V=V)
        ops.joiner_emit(P, g, blank, best, idx, ped, sl, z, at_eos, V=V)
        log = None
    else:
        ops.joiner_scan_beam(P, g, W_fm, ped, sl, None, blank, best, idx, group=group, V=V)
        ops.joiner_emit_beam(P, g, blank, best, idx, ped, sl, None, z, at_eos, log, group=group, V=V)
    torch.cuda.synchronize()
    return {"blank": blank.cpu(), "best": best.cpu(), "idx": idx.cpu(), "z": z.float().cpu(), "at_eos": at_eos.cpu(),
            "prev_emit": ped.cpu(), "log": None if log is None else log.cpu()}


AVAIL = [0, 1, 15, 16, 17, None]          # None: S


def _open_cases(B, S, group, seed):
    """(avail [Bs], closed [Bs] bool, prev_emit [R]) for 6 rotations x 4 prev_emit patterns: every source meets every availability,
    and in every call some sources are CLOSED (at their availability, at least 1) beside the open ones"""
    gen = torch.Generator().manual_seed(seed)
    for shift in range(6):
        avail = torch.tensor([S if AVAIL[(b + shift) % 6] is None else min(AVAIL[(b + shift) % 6], S) for b in range(B)])
        closed = torch.tensor([(b + shift) % 4 == 3 for b in range(B)])
        a_r = avail.repeat_interleave(group)
        for pattern in ("zero", "a-1", "a", "random"):
            if pattern == "zero":
                pe = torch.zeros_like(a_r)
            elif pattern == "a-1":
                pe = (a_r - 1).clamp_min(0)
            elif pattern == "a":
                pe = a_r.clone()
            else:
                pe = (torch.rand(a_r.shape, generator=gen) * (a_r + 1)).floor().long().clamp_max(a_r)
            yield avail, closed, pe.to(torch.int32), pattern


@pytest.mark.parametrize("mode,group", [("plain", 1), ("beam", 1), ("beam", 3)])
@pytest.mark.parametrize("shape", [(6, 40, 32, 64), (3, 33, 256, 203)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_open_source_kernels_exact_and_against_fp64(ops, dtype, shape, mode, group):
    """For an OPEN row with a positions available: the scan touches [prev_emit, a) only, with the bits of the closed scan; the row
    emits at the first of these positions whose best non-blank beats the blank (no forced blank), prev_emit / z / at_eos = 0 /
    emit_log as the closed call on src_len = S wherever that one emits below a; otherwise it WAITS: at_eos = -1, emit_log = -1,
    prev_emit and z untouched.  Closed rows in the same call: every bit of an all-closed call.  And the decisions (where, or
    wait) are the fp64 ones of the kernel's own P and g wherever fp64 is clear; at most 10 % excused."""
    B, S, D, V = shape
    seed = 300 + 7 * B + S
    P, g, W, _ = _scan_inputs(B, S, D, V, seed)
    gr = g.repeat_interleave(group, 0).contiguous()
    if group > 1:                                        # the rows of a group differ in g
        gr = gr + 0.05 * torch.randn(gr.shape, generator=torch.Generator().manual_seed(seed + 2))
    Wd = W.to(dtype).to(DEV)
    W_fm = ops.pack_joiner_weight(Wd)
    Pd, gd = P.to(DEV), gr.to(DEV).contiguous()
    R = B * group
    ref = tr.joiner_logits(P.repeat_interleave(group, 0), gr, W.to(dtype))               # fp64 [R, S, V]
    tol = tol_rows(W.to(dtype), dtype)
    tol_dec = float(tol[0] + tol[1:].max())
    nb64 = ref[:, :, 1:].max(-1).values
    margin64, wins64 = (nb64 - ref[:, :, 0]).abs(), nb64 > ref[:, :, 0]
    full = torch.full((B,), S, dtype=torch.int32)
    n_open = n_excused = n_wait = n_emit = 0
    for avail, closed, pe, pattern in _open_cases(B, S, group, seed):
        a_closed = avail.clamp_min(1)
        src_len = torch.where(closed, a_closed, -1 - avail).to(torch.int32)
        got = _joiner_call(ops, Pd, gd, Wd, W_fm, pe, src_len, dtype, mode, group)
        all_closed = _joiner_call(ops, Pd, gd, Wd, W_fm, pe, a_closed.to(torch.int32), dtype, mode, group)
        at_S = _joiner_call(ops, Pd, gd, Wd, W_fm, pe, full, dtype, mode, group)
        kb, _ = _fold_parts(at_S["best"], at_S["idx"])
        for r in range(R):
            b = r // group
            a, p0 = int(avail[b]), int(pe[r])
            if bool(closed[b]):                          # a closed row beside open ones: the bits of the all-closed call
                for key in ("blank", "best", "idx", "z", "at_eos", "prev_emit") + (("log",) if got["log"] is not None else ()):
                    assert torch.equal(got[key][r], all_closed[key][r]), (key, r, pattern)
                assert int(got["at_eos"][r]) in (0, 1)
                continue
            lo = min(max(p0, 0), a)
            scanned = torch.zeros(S, dtype=torch.bool)
            scanned[lo:a] = True
            # the scan: nothing outside [prev_emit, a), inside it the closed scan's bits
            assert bool((got["blank"][r][~scanned] == SENT_F).all()) and bool((got["best"][r][~scanned] == SENT_F).all())
            assert bool((got["idx"][r][~scanned] == SENT_I).all())
            for key in ("blank", "best", "idx"):
                assert torch.equal(got[key][r][scanned], at_S[key][r][scanned]), (key, r, pattern)
            # the emission, from the closed scan's own values (the true blank logit everywhere: nothing is forced)
            win = (kb[r] > at_S["blank"][r]) & scanned
            e = int(win.nonzero()[0]) if bool(win.any()) else None
            if e is not None:
                n_emit += 1
                assert int(got["prev_emit"][r]) == e and int(got["at_eos"][r]) == 0, (r, pattern, a, p0)
                assert int(at_S["prev_emit"][r]) == e, "the closed call on src_len = S emits there too"
                assert torch.equal(got["z"][r], at_S["z"][r])
                assert got["log"] is None or int(got["log"][r]) == e
            else:
                n_wait += 1
                assert int(got["at_eos"][r]) == -1 and int(got["prev_emit"][r]) == p0, (r, pattern, a, p0)
                assert bool((got["z"][r] == float(torch.tensor(SENT_F, dtype=dtype))).all())
                assert got["log"] is None or int(got["log"][r]) == -1
                if a > lo:                               # the closed call emits at or behind a (or is forced)
                    assert int(at_S["prev_emit"][r]) >= min(a, S - 1)
            # ... and against fp64: clear when every scanned position up to fp64's emit is clear
            w64 = (wins64[r] & scanned).nonzero()
            e64 = int(w64[0]) if w64.numel() else None
            upto = scanned.clone()
            if e64 is not None:
                upto[e64 + 1:] = False
            n_open += 1
            if bool((margin64[r][upto] > tol_dec).all()):
                assert e == e64, (r, pattern, a, p0, e, e64)
            else:
                n_excused += 1
    print(f"{dtype} {shape} {mode}/{group}: {n_open} open decisions ({n_emit} emit, {n_wait} wait), {n_excused} excused")
    assert n_emit > 0 and n_wait > 0
    assert n_excused <= 0.10 * n_open


def test_mask_blank_leaves_waiting_rows_alone(ops):
    logits = torch.ones(4, 64, device=DEV)
    ops.joiner_mask_blank(logits, torch.tensor([-1, 0, 1, -1], dtype=torch.int32, device=DEV))
    assert logits[:, 0].cpu().tolist() == [1.0, 1.0, -1e4, 1.0] and bool((logits[:, 1:] == 1).all())


# ---------------------------------------------------------------------------------------------------------------- decoder
def _decoder(cfg, w, dtype):
    from simulst_amd.transducer import TransducerDecoder
    return TransducerDecoder(cfg, w, device=DEV, dtype=dtype)


def _drive(dec, st, releases, n, recompute, check=None):
    """rounds of step_online behind every release until no row writes; a row ends after n tokens (NOT at EOS: the offline
    decode it is compared with goes on too).  -> tokens, emit, chunk per row.  check(before, src_len, logits, wrote): called
    behind every round with the round's prev_emit / src_len as they were before it"""
    cfg, ops, B = dec.cfg, dec.ops, st.B
    toks = torch.zeros(B, device=DEV, dtype=torch.int64)
    out, em, ch = [[] for _ in range(B)], [[] for _ in range(B)], [[] for _ in range(B)]
    for c, release in enumerate(releases):
        release()
        for _ in range(n + 1):
            before, sl = st.prev_emit.cpu().clone(), st.src_len.cpu().clone()
            logits, wrote = dec.step_online(st, toks, recompute_g=recompute)
            if check is not None:
                check(before, sl, logits, wrote)
            w = wrote.tolist()
            if not any(w):
                break
            first = torch.tensor([not o for o in out], device=DEV)
            pick = torch.where(first, ops.greedy_argmax(logits, pad_idx=cfg.padding_idx, eos_idx=cfg.eos, mask_eos=True),
                               ops.greedy_argmax(logits, pad_idx=cfg.padding_idx, eos_idx=cfg.eos, mask_eos=False))
            toks = torch.where(wrote, pick, toks)
            p, e = pick.tolist(), st.prev_emit.tolist()
            for b in range(B):
                if w[b]:
                    out[b].append(p[b]), em[b].append(e[b]), ch[b].append(c)
            st.done.copy_(torch.tensor([len(o) >= n for o in out], dtype=torch.int32))
            dec.sync_source(st)
        else:
            raise AssertionError("rows still writing after n rounds")
    return out, em, ch


@pytest.mark.parametrize("recompute", [False, True], ids=["cached_g", "recompute_g"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_step_online_is_greedy_offline_bit_for_bit(dtype, recompute):
    """rows of 96 encoder states released in chunks of 16, the OFFLINE P installed into the streaming state (so that both paths
    read the same bits): tokens, emit positions and the committed K/V positions are those of greedy_offline"""
    cfg, w, _, _ = _big_model(seed=21)
    B, n = 6, 16
    enc = torch.randn(B, 96, 256, generator=torch.Generator().manual_seed(22))
    dec = _decoder(cfg, w, dtype)
    lens = torch.full((B,), 96)
    toks, emit, off = dec.greedy_offline(enc.to(DEV), lens, n)
    toks, emit = toks.cpu().tolist(), emit.cpu().tolist()
    S = off.P.size(1)
    assert S == 12
    # the offline run is the reference here: its emit positions say at which chunk a token can be written
    need = [[min(e // 2, 5) if e < S - 1 else 5 for e in row] for row in emit]
    assert sum(sr.reads_between_writes(c) for c in need) >= 2, need
    st = dec.new_state(B, cap=n + 2)
    dec.open_source(st, S)
    st.P.copy_(off.P)

    def release(c):
        def go():
            st.avail_host = [S if c == 5 else 2 * (c + 1)] * B
            st.open_host = [0 if c == 5 else 1] * B
            dec.sync_source(st)
        return go
    out, em, ch = _drive(dec, st, [release(c) for c in range(6)], n, recompute)
    assert out == toks and em == emit
    assert ch == need, "a token is written at the chunk that releases its position, the forced last one at the end"
    assert st.n_prev.tolist() == [n] * B
    for l in range(cfg.decoder_layers):
        assert torch.equal(st.k_cache[l][:, :, :n], off.k_cache[l][:, :, :n])
        assert torch.equal(st.v_cache[l][:, :, :n], off.v_cache[l][:, :, :n])


def test_greedy_offline_mask_first_eos_keyword():
    """mask_first_eos=True is the default (EOS cannot be the first token); False lets a row whose first row of logits prefers EOS
    write it -- the EOS row of the output projection scaled up so that some row does -- and changes nothing for the other rows"""
    cfg, w, enc, lens = _big_model(seed=21)
    w = dict(w)
    out = w["decoder.output_projection.weight"].clone()
    out[cfg.eos] *= 10.0
    w["decoder.output_projection.weight"] = w["decoder.joiner.output_projection.weight"] = out
    dec = _decoder(cfg, w, torch.float32)
    args = (enc.to(DEV), torch.tensor(lens), 4)
    default, emit_d, _ = dec.greedy_offline(*args)
    masked, emit_m, _ = dec.greedy_offline(*args, mask_first_eos=True)
    free, emit_f, _ = dec.greedy_offline(*args, mask_first_eos=False)
    assert torch.equal(default, masked) and torch.equal(emit_d, emit_m)
    assert bool((default[:, 0] != cfg.eos).all())
    first_eos = free[:, 0] == cfg.eos
    assert bool(first_eos.any()), free[:, 0].tolist()
    assert torch.equal(free[~first_eos], default[~first_eos]) and torch.equal(emit_f[:, 0], emit_d[:, 0])


LENS = [96, 95, 64, 33, 9, 1]


def _append_all(dec, st, enc, lens):
    """releases of 16 encoder rows per chunk; a row's source ends with its last rows"""
    def release(c):
        def go():
            n_new = [min(max(L - CHUNK * c, 0), CHUNK) for L in lens]
            fin = [CHUNK * c < L <= CHUNK * (c + 1) for L in lens]
            dec.append_source(st, enc[:, CHUNK * c:CHUNK * (c + 1)].to(DEV), n_new, fin)
        return go
    return [release(c) for c in range((max(lens) + CHUNK - 1) // CHUNK)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_append_source_pools_what_set_source_pools(dtype):
    """complete windows: the bits of set_source's pooled rows; the flushed partial window: the mean of its valid rows, which is
    what AvgPool1dTBCPad gives a row shorter than the batch (to 1e-6 in fp32, one bf16 ulp in bf16)"""
    cfg, w, enc, lens = _big_model(seed=21)
    assert lens == LENS
    dec = _decoder(cfg, w, dtype)
    off = dec.new_state(6)
    dec.set_source(off, enc.to(DEV), torch.tensor(lens))
    st = dec.new_state(6)
    dec.open_source(st, 4)                               # grows past its capacity on the way
    for go in _append_all(dec, st, enc, lens):
        go()
    assert st.avail_host == [12, 12, 8, 5, 2, 1] and st.open_host == [0] * 6 and st.src_len.tolist() == off.src_len.tolist()
    mean = sr.pooled_row
    for b, L in enumerate(lens):
        full = L // K
        assert torch.equal(st.pooled[b, :full], off.pooled[b, :full]), b
        if L % K:
            want = mean(enc[b, :L].to(dtype), K)[-1]
            err = (st.pooled[b, full].double().cpu() - want).abs()
            bound = 1e-6 if dtype == torch.float32 else 2.0 ** (torch.floor(torch.log2(want.abs().clamp_min(2.0 ** -126))) - 7) + 1e-6
            assert bool((err <= bound).all()), (b, float(err.max()))
        n_p = full + (L % K > 0 and dtype == torch.float32)          # P rows of equal (or, flushed in fp32, all but equal) pooled rows
        if n_p:
            assert float((st.P[b, :n_p] - off.P[b, :n_p]).abs().max()) < 1e-4, b


def test_step_online_over_an_appended_source_against_the_restatement():
    """P built by append_source (fp32), rows of 96, 95, 64, 33, 9 and 1 encoder states: tokens and emit positions against the fp64
    streaming loop, a row compared up to its first unclear token"""
    cfg, w, enc, lens = _big_model(seed=21)
    n = 16
    ref = tr.TransducerRef(w, heads=cfg.num_heads, downsample=cfg.downsample)
    recs = []
    for b, L in enumerate(lens):
        sched = [min(CHUNK * (c + 1), L) for c in range((L + CHUNK - 1) // CHUNK)]
        recs.append(sr.stream_row(ref, enc[b, :L], sched, n))
    assert sum(sr.reads_between_writes(r["chunk"]) for r in recs) >= 2, [r["chunk"] for r in recs]
    dec = _decoder(cfg, w, torch.float32)
    st = dec.new_state(6, cap=n + 2)
    dec.open_source(st, 12)
    out, em, ch = _drive(dec, st, _append_all(dec, st, enc, lens), n, recompute=False)
    n_tok = n_excused = 0
    for b, r in enumerate(recs):
        assert len(r["tokens"]) == n and len(out[b]) == n
        clear = 0
        while clear < n and r["margin"][clear] > 1e-3:
            clear += 1
        n_tok, n_excused = n_tok + n, n_excused + n - clear
        assert out[b][:clear] == r["tokens"][:clear] and em[b][:clear] == r["emit"][:clear] and ch[b][:clear] == r["chunk"][:clear], b
    print(f"appended source: {n_tok} tokens, {n_excused} excused; chunks {[r['chunk'] for r in recs]}")
    assert n_excused <= 0.10 * n_tok


def test_bf16_rounds_over_an_appended_source_against_the_fp64_joiner_of_their_own_buffers():
    """the same appended source in bf16: every round's decision of every live row (emit where, or wait) against the fp64 joiner of
    the kernel's OWN P and g (as test_bf16_steps_against_the_fp64_joiner_of_their_own_buffers holds the closed step), and the
    returned row of a row that wrote"""
    cfg, w, enc, lens = _big_model(seed=21)
    dt, n = torch.bfloat16, 16
    ref16 = tr.TransducerRef(w, heads=cfg.num_heads, downsample=cfg.downsample, round_to=dt)
    recs = [sr.stream_row(ref16, enc[b, :L].to(dt), [min(CHUNK * (c + 1), L) for c in range((L + CHUNK - 1) // CHUNK)], n)
            for b, L in enumerate(lens)]
    assert sum(sr.reads_between_writes(r["chunk"]) for r in recs) >= 2, [r["chunk"] for r in recs]
    dec = _decoder(cfg, w, dt)
    st = dec.new_state(6, cap=n + 2)
    dec.open_source(st, 12)
    Wr = dec.w.out_proj.cpu()
    tol = tol_rows(Wr, dt)
    tol_dec = float(tol[0] + tol[1:].max())
    count = {"decisions": 0, "excused": 0, "waits": 0, "writes": 0}

    def check(before, sl, logits, wrote):
        ref = tr.joiner_logits(st.P.cpu(), st.g.cpu(), Wr)                    # fp64 [B, S_cap, V]
        w_h, emit, done, got = wrote.tolist(), st.prev_emit.cpu().tolist(), st.done.tolist(), logits.cpu().double()
        for b in range(6):
            if done[b]:
                assert not w_h[b]
                continue
            is_open = int(sl[b]) < 0
            a = -1 - int(sl[b]) if is_open else int(sl[b])
            e64, m = None, []
            for s in range(min(int(before[b]), a if is_open else a - 1), a):
                row = ref[b, s].clone()
                if not is_open and s == a - 1:
                    row[0] = tr.BLANK_AT_EOS
                m.append(float((row[1:].max() - row[0]).abs()))
                if row[1:].max() > row[0]:
                    e64 = s
                    break
            count["decisions"] += 1
            count["writes" if w_h[b] else "waits"] += 1
            assert is_open or w_h[b], "a closed row always writes"
            if all(x > tol_dec for x in m):
                assert (emit[b] if w_h[b] else None) == e64, (b, a, is_open, emit[b], e64)
            else:
                count["excused"] += 1
            if w_h[b]:
                row = ref[b, emit[b]].clone()                                 # the returned row, at the KERNEL's emit
                if not is_open and emit[b] == a - 1:
                    row[0] = tr.BLANK_AT_EOS
                assert bool(((got[b] - row).abs() <= tol).all()), (b, float(((got[b] - row).abs() - tol).max()))
    out, em, ch = _drive(dec, st, _append_all(dec, st, enc, lens), n, recompute=False, check=check)
    print(f"bf16 rounds over an appended source: {count}; chunks {ch}")
    assert all(len(o) == n for o in out) and count["waits"] >= 4
    assert sum(sr.reads_between_writes(c) for c in ch) >= 2
    assert count["excused"] <= 0.10 * count["decisions"]


# ---------------------------------------------------------------------------------------------------------------- agents
@pytest.fixture(scope="module")
def agent_case():
    """the _big_model weights (blank row x 6, target projection x 3, source projection x 4) with their encoder, 4 utterances of
    400 frames, and per row: the streamed encoder states, the chunk positions and the rows released"""
    from simulst_amd.transducer import TransducerModel
    from simulst_amd.transducer_agent import TransducerAgent
    cfg, w, _, _ = _big_model(seed=21)
    model = TransducerModel(cfg, w, device=DEV, dtype=torch.float32)
    fb = torch.randn(4, 400, 80, generator=torch.Generator().manual_seed(77))
    agent = TransducerAgent(model)
    positions = agent._chunk_positions(400)
    schedule = model.encoder.stream_row_schedule(positions)
    state, outs = {}, []
    for i, pos in enumerate(positions):
        outs.append(model.encoder.infer(fb[:, :pos].to(DEV), torch.full((4,), pos), state, finish=i == len(positions) - 1)["encoder_out_btd"])
    assert [sum(o.size(1) for o in outs[:i + 1]) for i in range(len(outs))] == schedule
    return cfg, w, model, fb, positions, schedule, torch.cat(outs, 1).cpu()


def _ref_records(cfg, w, enc, positions, schedule, max_len, n_max=64):
    from simulst_amd.latency import average_lagging
    ref = tr.TransducerRef(w, heads=cfg.num_heads, downsample=cfg.downsample)
    recs = []
    for b in range(enc.shape[0]):
        r = sr.stream_row(ref, enc[b], schedule, n_max, stop=lambda toks, c: toks[-1] == cfg.eos or len(toks) > max_len(positions[c]))
        r["delays_ms"] = [positions[c] * 10 + 15 for c in r["chunk"]]
        r["AL"] = average_lagging(r["delays_ms"], positions[-1] * 10 + 15)
        recs.append(r)
    return recs


def _same(a, b, keys=("tokens", "actions", "delays_ms", "AL", "emit", "n_enc")):
    for k in keys:
        assert a[k] == b[k], (k, a[k], b[k])


def _actions_upto(actions, n_tokens):
    """the READ / WRITE string up to and including its n_tokens-th WRITE"""
    if n_tokens == 0:
        return ""
    seen = 0
    for i, ch in enumerate(actions):
        seen += ch == "W"
        if seen == n_tokens:
            return actions[:i + 1]
    raise AssertionError(f"{actions!r} holds fewer than {n_tokens} WRITEs")


def _held_to_reference(refs, gots, what):
    """Every row against the fp64 streaming loop, up to its first unclear token (fp64 margin <= 1e-3, the bound of
    test_greedy_at_model_size_against_the_restatement for an fp32 trajectory): tokens, emit positions, delays and the action string
    up to there; a row that is clear throughout also in its whole action string and AL.  Everything behind a row's first unclear
    token counts as excused, at most 10 % of all tokens; and at least two rows that READ between two WRITEs are compared in full."""
    n_tok = n_excused = n_full_with_reads = 0
    for r, got in zip(refs, gots):
        n = len(r["tokens"])
        clear = 0
        while clear < n and r["margin"][clear] > 1e-3:
            clear += 1
        n_tok, n_excused = n_tok + n, n_excused + n - clear
        assert len(got["tokens"]) >= clear
        for key in ("tokens", "emit", "delays_ms"):
            assert got[key][:clear] == r[key][:clear], (key, got[key], r[key])
        assert _actions_upto(got["actions"], clear) == _actions_upto(r["actions"], clear), (got["actions"], r["actions"])
        if clear == n:
            _same(got, r, ("tokens", "actions", "delays_ms", "AL", "emit"))
            n_full_with_reads += sr.reads_between_writes(r["chunk"])
    print(f"{what}: {n_tok} tokens, {n_excused} excused, {n_full_with_reads} rows with READs between WRITEs compared in full; "
          f"actions {[g_['actions'] for g_ in gots]}; emit {[g_['emit'] for g_ in gots]}")
    assert n_tok > 0 and n_excused <= 0.10 * n_tok
    assert n_full_with_reads >= 2


def test_agents_against_the_reference_loop_and_each_other(agent_case):
    """B = 1 agent records (tokens, actions, delays, AL) against the fp64 streaming loop over the same encoder states; lockstep rows
    against the B = 1 agent; self-paced records against lockstep ones over encoder='offline' states; the forced last position is
    written only after the source has ended; the cap rule (max_len_a = 0.05: a row may not hold more than 0.05 x frames read)"""
    from simulst_amd.model import refuse_offline_model
    from simulst_amd.transducer_agent import BatchedTransducerStreamingAgent, TransducerAgent
    cfg, w, model, fb, positions, schedule, enc = agent_case
    a, b_ = 0.05, 0
    max_len = lambda x: min(a * x + b_, cfg.max_target_positions)            # noqa: E731
    refs = _ref_records(cfg, w, enc, positions, schedule, max_len)
    assert sum(sr.reads_between_writes(r["chunk"]) for r in refs) >= 2, [r["actions"] for r in refs]
    single = TransducerAgent(model, max_len_a=a, max_len_b=b_)
    ones = [single.run_utterance(fb[i].to(DEV)) for i in range(4)]
    _held_to_reference(refs, ones, "B = 1 agent")
    S_last = (schedule[-1] + K - 1) // K - 1
    last_ms = positions[-1] * 10 + 15
    assert any(e == S_last for got in ones for e in got["emit"]), "some row reaches the forced last position"
    for got in ones:
        assert all(d == last_ms for e, d in zip(got["emit"], got["delays_ms"]) if e == S_last), "forced emission only after finish"
        assert got["tokens"][-1] == cfg.eos or len(got["tokens"]) > max_len(positions[got["actions"].count("R") - 1]), "the cap rule"
    batched = BatchedTransducerStreamingAgent(model, max_len_a=a, max_len_b=b_)
    for got, one in zip(batched.run_batch(fb), ones):
        _same(got, one)
    paced = batched.run_batch(fb, self_paced=True)
    for got, one in zip(paced, ones):
        _same(got, one)
    lock_off = batched.run_batch(fb, encoder="offline")
    paced_off = batched.run_batch(fb, self_paced=True, encoder="offline")
    for got, want in zip(paced_off, lock_off):
        _same(got, want)
    with pytest.raises(ValueError, match="transducer_model"):
        refuse_offline_model(model, "agent")
    from simulst_amd.agent import BatchedStreamingAgent, FairseqSimulSTAgent
    for cls in (FairseqSimulSTAgent, BatchedStreamingAgent):
        with pytest.raises(ValueError, match="transducer_model"):
            cls(model)


def test_self_paced_rows_of_different_lengths(agent_case):
    """encoder='offline' admits ``lengths``: every row follows the chunk schedule of its own length.  Records against the fp64
    streaming loop over the same offline encoder states, row by row"""
    from simulst_amd.latency import average_lagging
    from simulst_amd.transducer_agent import BatchedTransducerStreamingAgent
    cfg, w, model, fb, _, _, _ = agent_case
    Ls = [400, 333, 230, 20]
    fbp = fb[[2, 3, 0, 1]].clone()                       # the two utterances whose rows READ between WRITEs get the long lengths
    for b, L in enumerate(Ls):
        fbp[b, L:] = 0
    a = 0.05
    agent = BatchedTransducerStreamingAgent(model, max_len_a=a)
    states = model.encoder.forward(fbp.to(DEV), torch.tensor(Ls, device=DEV))
    enc, enc_len = states["encoder_out_btd"].cpu(), states["encoder_lengths"].tolist()
    ref = tr.TransducerRef(w, heads=cfg.num_heads, downsample=cfg.downsample)
    refs = []
    for b, L in enumerate(Ls):
        positions = agent._chunk_positions(L)
        schedule = model.encoder.stream_row_schedule(positions)
        assert schedule[-1] == enc_len[b]
        r = sr.stream_row(ref, enc[b, :enc_len[b]], schedule, 64,
                          stop=lambda toks, c, p=positions: toks[-1] == cfg.eos or len(toks) > min(a * p[c], cfg.max_target_positions))
        r["delays_ms"] = [positions[c] * 10 + 15 for c in r["chunk"]]
        r["AL"] = average_lagging(r["delays_ms"], L * 10 + 15)
        refs.append(r)
    assert sum(sr.reads_between_writes(r["chunk"]) for r in refs) >= 2, [r["actions"] for r in refs]
    got = agent.run_batch(fbp, self_paced=True, encoder="offline", lengths=Ls)
    _held_to_reference(refs, got, "ragged self-paced rows")
    assert len({g_["actions"].count("R") for g_ in got}) >= 3, "rows of different lengths read different numbers of chunks"
    with pytest.raises(ValueError, match="different lengths"):
        agent.run_batch(fbp, lengths=Ls)
    with pytest.raises(ValueError, match="different lengths"):
        agent.run_batch(fbp, self_paced=True, lengths=Ls)


def test_eos_ends_a_row_while_the_others_go_on(agent_case):
    """the EOS row of the output projection scaled up: rows end at different lengths, each as its own B = 1 run and as what
    generate_offline writes up to EOS"""
    from simulst_amd.transducer import TransducerModel
    from simulst_amd.transducer_agent import BatchedTransducerStreamingAgent, TransducerAgent
    cfg, w, _, fb, positions, schedule, _ = agent_case
    w = dict(w)
    out = w["decoder.output_projection.weight"].clone()
    out[cfg.eos] *= 2.5
    w["decoder.output_projection.weight"] = w["decoder.joiner.output_projection.weight"] = out
    model = TransducerModel(cfg, w, device=DEV, dtype=torch.float32)
    recs = BatchedTransducerStreamingAgent(model, max_len_a=0.1).run_batch(fb)
    ends = [r["tokens"][-1] == cfg.eos for r in recs]
    print(f"EOS rows {ends}, lengths {[len(r['tokens']) for r in recs]}, actions {[r['actions'] for r in recs]}")
    assert sum(ends) >= 1 and len({len(r["tokens"]) for r in recs}) >= 2, [r["tokens"] for r in recs]
    single = TransducerAgent(model, max_len_a=0.1)
    for i, r in enumerate(recs):
        assert cfg.eos not in r["tokens"][:-1]
        _same(r, single.run_utterance(fb[i].to(DEV)))
    # what is written simultaneously is what the offline decode writes up to EOS, over the same (streamed) encoder states
    paced = BatchedTransducerStreamingAgent(model, max_len_a=0.1).run_batch(fb, self_paced=True)
    for r, p in zip(recs, paced):
        _same(r, p)


def test_a_source_that_ends_before_the_first_pooled_window(agent_case):
    """20 frames: fewer encoder rows than one pooling window -- one flushed position, every token forced at it after finish"""
    from simulst_amd.transducer_agent import BatchedTransducerStreamingAgent, TransducerAgent
    cfg, _, model, fb, _, _, _ = agent_case
    short = fb[:2, :20].contiguous()
    single = TransducerAgent(model, max_len_a=0.2)
    one = single.run_utterance(short[0].to(DEV))
    assert 0 < one["n_enc"] < K
    assert one["actions"] == "R" + "W" * len(one["tokens"]) and one["emit"] == [0] * len(one["tokens"]) and len(one["tokens"]) == 5
    assert one["delays_ms"] == [215] * 5
    batched = BatchedTransducerStreamingAgent(model, max_len_a=0.2)
    for form in (dict(), dict(self_paced=True), dict(self_paced=True, encoder="offline")):
        recs = batched.run_batch(short, **form)
        _same(recs[0], one)
