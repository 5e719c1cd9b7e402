"""CPU side of tests/test_hip_front_end.py: the float64 references of tests/front_end_ref.py are tied to their oracle counterparts on
every case the GPU file runs, a mutation table shows that those cases can fail, and the margins the cases rely on are asserted on
the inputs.  Nothing here needs a GPU.

Mutations (front_end_ref.MUTATIONS): each is applied to the reference alone and must move at least one compared element of at least
one GPU case beyond that case's bound.  Three of the mistakes the table was asked to cover cannot be seen by ANY case, for a reason
that lies in the operation and not in the cases; for these the test asserts the opposite -- that no compared element moves at all:
  * preemph0_zero (sample 0 pre-emphasised against zero instead of itself): the Povey window is exactly 0 at sample 0
    ((0.5 - 0.5 cos 0)^0.85), in float64 and in the kernel's float32 table, so whatever sample 0 holds is multiplied by 0;
  * cnt_no_max (the summary count len - t0 without max(len, t0 + 1)): the two counts differ only where len <= t0, which is a segment
    wholly at or beyond len -- the one declared exclusion of the GPU file;
  * no_last_zero (pack-rows without zeroing the last segment's block): the last block's sources are frames N S + r >= T, which the
    `beyond the utterance` rule zeroes anyway.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import front_end_ref as fr
import test_hip_front_end as fe

INVISIBLE = ("preemph0_zero", "cnt_no_max", "no_last_zero")


# ---- fbank ----------------------------------------------------------------------------------------------------------------------------
def test_fbank_reference_equals_oracle():
    """ln max(e, eps) of the reference against oracle.fbank.kaldi_fbank (float32 frames, float64 rfft, float32 mel product): inside
    the bound the kernel is held to"""
    from oracle.fbank import kaldi_fbank, mel_banks, povey_window
    assert float(np.abs(povey_window(400) - fr.povey_window64()).max()) <= 2.0 ** -24
    assert fr.povey_window64()[0] == 0.0 and float(povey_window(400)[0]) == 0.0
    for m in (64, 80, 128):
        assert float(np.abs(mel_banks(m) - fr.mel_weights64(m)).max()) <= 2.0 ** -24
    Cs = fe.fb_C()
    worst = 0.0
    for name in fe.FB_NAMES:
        c = fe.fb_case(name)
        for b, r in enumerate(fe.fb_ref(name)):
            o = kaldi_fbank(c["wave"][b], num_mel_bins=c["n_mel"], preemphasis=c["preemph"]).astype(np.float64)
            assert o.shape == r["e"].shape == (fe.fb_frames(c["n"]), c["n_mel"])
            bound, ee = fe.fb_bound(r, 4.0 * Cs[c["kinds"][b]])
            worst = max(worst, fe._ratio(np.exp(o), ee, bound))
    print("C_measured", {k: round(v, 2) for k, v in Cs.items()}, f"; oracle worst |exp(o) - ee| / bound {worst:.4f}")
    assert worst <= 1.0


def test_fbank_frame_totals_and_margins():
    """frame totals 0, 1, 2, 3 mod 4 with one workgroup over two utterances; floor rows have every energy exactly 0; in every other
    row the bound stays below max(e, eps) at every element -- except in the three declared narrow-spectrum classes (FB_PARTIAL_FLOOR),
    whose far bins lie 1e-13 below the peak: there the bins that hold the energy are well above their bound and the rest may hide"""
    totals = {len(fe.fb_case(n)["kinds"]) * fe.fb_frames(fe.fb_case(n)["n"]) for n in fe.FB_NAMES}
    assert {t % 4 for t in totals} == {0, 1, 2, 3}, totals
    c = fe.fb_case("noise_n720")
    assert c["wave"].shape == (3, 720) and fe.fb_frames(720) == 3
    assert {fe.fb_case(n)["n"] for n in fe.FB_NAMES} == set(fe.FB_N)
    assert {fe.fb_case(n)["n_mel"] for n in fe.FB_NAMES} == {64, 80, 128}
    assert {fe.fb_case(n)["preemph"] for n in fe.FB_NAMES} == {float(np.float32(0.97)), 0.0}
    Cs = fe.fb_C()
    assert set(Cs) == set(fe.FB_SIGNALS) and all(Cs[k] == 0.0 for k in fe.FB_FLOOR)
    assert all(0.5 < Cs[k] < 16.0 for k in fe.FB_SIGNALS if k not in fe.FB_FLOOR + ("imp399",)), Cs
    assert Cs["imp399"] < 256.0           # a constant after the mean is removed: cur - 0.97 prev cancels, the error scales with x, not y
    worst, hidden = 0.0, {}
    for name in fe.FB_NAMES:
        c = fe.fb_case(name)
        for b, r in enumerate(fe.fb_ref(name)):
            kind = c["kinds"][b]
            if kind in fe.FB_FLOOR:
                assert not r["e"].any() and not r["ynorm"].any(), (name, b)
                continue
            bound, ee = fe.fb_bound(r, 4.0 * Cs[kind])
            q = bound / ee
            if kind in fe.FB_PARTIAL_FLOOR:
                assert (q.min(axis=1) < 1e-2).all() and float((q < 1.0).mean()) > 0.1, (name, b, kind)
                hidden[kind] = max(hidden.get(kind, 0.0), float((q >= 1.0).mean()))
                continue
            worst = max(worst, float(q.max()))
            assert (q < 1.0).all(), (name, b, kind, float(q.max()))
    print(f"largest bound / max(e, eps) outside the declared classes: {worst:.3e}; share of elements below their bound in the "
          f"narrow-spectrum classes: {hidden}")
    r = fe.fb_ref("signals_m80_p0.97")[fe.FB_SIGNALS.index("tone")]
    assert float((r["e"].min(axis=1) / r["e"].max(axis=1)).max()) < 1e-7       # the tone's far bins


def test_fbank_log_term():
    """why the bound's last term carries 1.5 * 2^-23 |ln ee|: the CPU float32 chain followed by a float32 log, which is what a correct
    kernel stores, against the asserted bound with 2^-21 alone and with the term"""
    Cs = fe.fb_C()
    without = with_ = 0.0
    for name in fe.FB_NAMES:
        c = fe.fb_case(name)
        for b, r in enumerate(fe.fb_ref(name)):
            e32 = fe.fb_f32_chain(c["wave"][b], c["n_mel"], c["preemph"]).numpy()
            got = np.log(np.maximum(e32, np.float32(fr.EPS32))).astype(np.float32).astype(np.float64)
            for lt in (False, True):
                bound, ee = fe.fb_bound(r, 4.0 * Cs[c["kinds"][b]], log_term=lt)
                q = fe._ratio(np.exp(got), ee, bound)
                without, with_ = (max(without, q), with_) if not lt else (without, max(with_, q))
    print(f"float32 chain + float32 log: |exp(got) - ee| / bound {without:.3f} with 2^-21 alone, {with_:.3f} with 1.5 * 2^-23 |ln ee| added")
    assert with_ <= 1.0 < without


def _fb_mutation_seen(mut):
    Cs = fe.fb_C()
    n = 0
    for name in fe.FB_NAMES:
        c = fe.fb_case(name)
        for b, (r, m) in enumerate(zip(fe.fb_ref(name), fe.fb_ref(name, mut))):
            bound, ee = fe.fb_bound(r, 4.0 * Cs[c["kinds"][b]])
            n += fe._ratio(np.maximum(m["e"], fr.EPS32), ee, bound) > 1.0
    return n


# ---- conv-pos -------------------------------------------------------------------------------------------------------------------------
def _conv_cases():
    for cls in fe.CONV_CLASSES:
        for D in fe.MFMA_D:
            for (k, T, hist, lens) in fe.MFMA_GRID:
                yield fe.conv_case(cls, True, k, 16, D, T, hist, lens)
        for bf16 in (False, True):
            for cpg in fe.VALU_CPG:
                for (k, T, hist, lens) in fe.VALU_GRID:
                    if (k, cpg) not in fe.VALU_REFUSED:
                        yield fe.conv_case(cls, bf16, k, cpg, 4 * cpg, T, hist, lens)


def _conv_oracle(c, dtype):
    """x + gelu(oracle.causal_conv.causal_conv1d) in `dtype` on the row's valid frames (NaN padding set to 0: the conv is causal)"""
    from oracle.causal_conv import causal_conv1d
    x = torch.from_numpy(np.nan_to_num(c["x"])).to(dtype)
    state = {"prev_feat": torch.from_numpy(c["hist"]).to(dtype).transpose(1, 2)} if c["hist"] is not None else None
    y = causal_conv1d(x.transpose(1, 2), torch.from_numpy(c["W"]).to(dtype), torch.from_numpy(c["bias"]).to(dtype), groups=c["groups"],
                      state=state)
    y = (x + F.gelu(y.transpose(1, 2))).double().numpy()
    if c["lens"] is not None:
        for b, L in enumerate(c["lens"]):
            y[b, L:] = 0.0
    return y


def test_conv_reference_equals_oracle_and_margins():
    """float64 oracle within 1e-12 (+ 1e-12 relative) on every case; EXACT inputs are exact; an fp32 evaluation of the oracle on the
    CPU stays inside the bound the kernels are held to (the bound can be met); ragged cases hold NaN exactly at t >= len"""
    n = 0
    worst32 = {}
    for c in _conv_cases():
        ref = fe.conv_ref(c)
        o = _conv_oracle(c, torch.float64)
        assert np.isfinite(ref[0]).all()
        assert float((np.abs(o - ref[0]) / (1.0 + np.abs(o))).max()) <= 1e-12, (c["cls"], c["k"], c["cpg"], c["T"])
        if c["cls"] == "exact":
            fe.conv_exact_margins(c)
        if c["lens"] is not None:
            for b, L in enumerate(c["lens"]):
                assert np.isnan(c["x"][b, L:]).all() and np.isfinite(c["x"][b, :L]).all()
        else:
            assert np.isfinite(c["x"]).all()
        if not c["bf16"]:
            bound, eg = fe.conv_bound(c, ref)
            q = fe._ratio(_conv_oracle(c, torch.float32), ref[0], bound)
            key = c["cls"]
            worst32[key] = max(worst32.get(key, 0.0), q)
        n += 1
    print(f"{n} conv cases; torch fp32 on the CPU, worst |y32 - ref| / bound: {worst32}")
    assert all(v <= 1.0 for v in worst32.values()), worst32


def test_conv_grids():
    ks = {k for (k, _, _, _) in fe.MFMA_GRID}
    assert ks == {16, 32, 64} and {T for (_, T, _, _) in fe.MFMA_GRID} == set(fe.MFMA_T)
    for grid, Ts in ((fe.MFMA_GRID, fe.MFMA_T), (fe.VALU_GRID, fe.VALU_T)):
        seen = set()
        for (k, T, hist, lens) in grid:
            seen.add((hist, lens is not None))
            if lens is not None:
                assert all(0 <= L <= T for L in lens) and (lens[0] != lens[1] or T == 0)
        assert seen == {(False, False), (False, True), (True, False), (True, True)}
        used = {L if L < T else None for (k, T, hist, lens) in grid if lens is not None for L in lens}
        assert used >= {0, 1, 16, 64, None}, used
    assert any(lens is not None and 256 in lens for (_, T, _, lens) in fe.MFMA_GRID if T > 256)
    assert any(T < k - 1 for (k, T, _, _) in fe.VALU_GRID) and any(T < k - 1 and hist for (k, T, hist, _) in fe.MFMA_GRID)
    assert any(hist and T > 256 for (_, T, hist, _) in fe.MFMA_GRID)


def _conv_mutation_seen(mut):
    for c in _conv_cases():
        if c["T"] > 65 or c["D"] > 64:
            continue                                           # the small cases are enough, and quick
        ref = fe.conv_ref(c)
        bound, _ = fe.conv_bound(c, ref)
        if fe._ratio(fe.conv_ref(c, mut)[0], ref[0], bound) > 1.0:
            return 1
    return 0


# ---- LayerNorm, pre-norm, segment mean ----------------------------------------------------------------------------------------------------
def test_layernorm_reference_equals_torch():
    for bf16 in (False, True):
        for D in fe.LN_D:
            for rows in fe.LN_ROWS:
                for cls in fe.LN_CLASSES:
                    c = fe.ln_case(D, rows, cls, bf16)
                    o = F.layer_norm(torch.from_numpy(c["x"]).double(), (D,), torch.from_numpy(c["g"]).double(),
                                     torch.from_numpy(c["b"]).double(), 1e-5).numpy()
                    assert float((np.abs(o - c["y"]) / (1.0 + np.abs(o))).max()) <= 1e-11, (D, rows, cls)
                    if cls == "const":
                        assert np.array_equal(c["y"], np.broadcast_to(c["b"].astype(np.float64), c["y"].shape)) and c["e32"] == 0.0
    assert any(256 < D < 1024 and D % 256 for D in fe.LN_D)


def _pn_cases():
    seen = set()
    for (T, S, n_rc, n_mem, with_sum, lens) in fe.PN_GRID:
        if (T, S, n_rc, lens) not in seen:
            seen.add((T, S, n_rc, lens))
            yield T, S, n_rc, lens


def test_prenorm_reference_equals_oracle_and_lengths():
    """LayerNorm rows against torch float64; summaries against oracle.emformer.avg_pool_ceil over the row cut at len (the ragged
    last window divides by its real count); the length classes T, 1, mid-segment, exactly t0 and t0 + 1 all occur"""
    from oracle.emformer import avg_pool_ceil
    classes = set()
    for D in fe.PN_D:
        for bf16 in (False, True):
            for (T, S, n_rc, lens) in _pn_cases():
                c = fe.pn_case(D, bf16, T, S, n_rc, lens)
                live = fe.pn_live(T, S, lens)
                for b in range(fe.PN_B):
                    L = T if lens is None else lens[b]
                    x = torch.from_numpy(c["X"][b, :n_rc + L]).double()
                    o = F.layer_norm(x, (D,), torch.from_numpy(c["g"]).double(), torch.from_numpy(c["b"]).double(), 1e-5)
                    assert float((o.numpy() - c["ln"][b, :n_rc + L]).__abs__().max()) <= 1e-11
                    pooled = avg_pool_ceil(o[n_rc:].unsqueeze(1), S)[:, 0].numpy()
                    assert pooled.shape[0] == int(live[b].sum())
                    assert float(np.abs(pooled - c["summ"][b][live[b]]).max()) <= 1e-11, (T, S, n_rc, lens, b)
                    assert np.isfinite(c["summ"][b][live[b]]).all()
                    if lens is not None:
                        assert np.isnan(c["X"][b, n_rc + L:]).all()
                        t0s = [t0 for t0 in range(0, T, S)]
                        classes |= {"T"} if L == T else set()
                        classes |= {"1"} if L == 1 else set()
                        classes |= {"t0"} if L in t0s and L > 0 else set()
                        classes |= {"t0+1"} if (L - 1) in t0s and L - 1 > 0 else set()
                        classes |= {"mid"} if L not in t0s and (L - 1) not in t0s and L != T else set()
    assert classes == {"T", "1", "t0", "t0+1", "mid"}, classes
    assert any(S > 16 for (_, S) in fe.PN_TS) and any(S == 1 for (_, S) in fe.PN_TS)


def test_segment_mean_reference_equals_oracle():
    """every D and both dtypes; the n_out the GPU test asks for are prefixes of these N segments"""
    from oracle.emformer import avg_pool_ceil
    for D in fe.SM_D:
        for bf16 in (False, True):
            for (T, S) in fe.PN_TS:
                for lens in fe.pn_lens(T, S):
                    c = fe.sm_case(D, bf16, T, S, lens)
                    live = fe.pn_live(T, S, lens)
                    for b in range(fe.PN_B):
                        L = T if lens is None else lens[b]
                        pooled = avg_pool_ceil(torch.from_numpy(c["X"][b, :L]).double().unsqueeze(1), S)[:, 0].numpy()
                        assert float(np.abs(pooled - c["out"][b][live[b]]).max()) <= 1e-12


def _ln_mutation_seen(mut):
    n = 0
    for D in fe.LN_D:
        c = fe.ln_case(D, 17, "random", False)
        m = fr.ref_layernorm(c["x"].astype(np.float64), c["g"].astype(np.float64), c["b"].astype(np.float64), mut=mut)[0]
        n += fe._ratio(m, c["y"], fe.ln_bound(c["y"], c["z"], c["g"], c["b"], fe.ln_e32_max(D, "random", False), False)) > 1.0
    return n


def _pn_mutation_seen(mut):
    n = 0
    D = 64
    for (T, S, n_rc, lens) in _pn_cases():
        c = fe.pn_case(D, False, T, S, n_rc, lens)
        m = fr.ref_prenorm(c["X"].astype(np.float64), c["g"].astype(np.float64), c["b"].astype(np.float64), lens, T, n_rc, S, mut)
        live = fe.pn_live(T, S, lens)
        sb = fe.pn_summary_bound(c, T, S, n_rc, False)
        n += fe._ratio(m[2][live], c["summ"][live], sb[live]) > 1.0
    return n


# ---- pack-rows, argmax --------------------------------------------------------------------------------------------------------------------
def test_pack_rows_reference_equals_oracle():
    """oracle.emformer.gen_right_context over the utterance with R zero frames appended, then the utterance rows"""
    from oracle.emformer import gen_right_context
    from types import SimpleNamespace
    for (T, S, R) in fe.PK_TSR:
        N = -(-T // S)
        for D in fe.PK_D:
            for B in fe.PK_B:
                for bf16 in (False, True):
                    x = fe.pk_case(T, S, R, D, B, bf16)
                    ref = fr.ref_pack_rows(x, S, R, N)
                    assert ref.shape == (B, N * R + T, D) and np.array_equal(ref[:, N * R:], x)
                    if R > 0:
                        xt = torch.from_numpy(x).transpose(0, 1)
                        padded = torch.cat([xt, torch.zeros(R, B, D)])
                        rc = gen_right_context(padded, SimpleNamespace(segment_length=S, right_context=R))
                        assert torch.equal(rc.transpose(0, 1), torch.from_numpy(ref[:, :N * R])), (T, S, R, D, B)
    assert any(T < S for (T, S, R) in fe.PK_TSR) and any(R == 0 for (T, S, R) in fe.PK_TSR) and any(R >= S for (T, S, R) in fe.PK_TSR)
    assert any((i + 1) * S + r == T for (T, S, R) in fe.PK_TSR for i in range(-(-T // S) - 1) for r in range(R))
    assert any(((-(-T // S)) * R + T) * (D // 4) > 64 * 256 for (T, S, R) in fe.PK_TSR for D in fe.PK_D)


def _pk_mutation_seen(mut):
    n = 0
    for (T, S, R) in fe.PK_TSR:
        N = -(-T // S)
        x = fe.pk_case(T, S, R, 8, 1, False)
        n += not np.array_equal(fr.ref_pack_rows(x, S, R, N, mut), fr.ref_pack_rows(x, S, R, N))
    return n


def test_argmax_reference_and_cases():
    """the reference is numpy's argmax (first maximum) of the adjusted row; every tie class is present at the V that can hold it"""
    for V in fe.AM_V:
        logits, bias, pad, eos, names = fe.am_case(V)
        assert np.isfinite(logits).all() or "all_neg_inf" in names
        for mask_eos in (False, True):
            for use_bias in (False, True):
                adj = logits.astype(np.float64).copy()
                if use_bias and eos >= 0:
                    adj[:, eos] += bias
                if pad >= 0:
                    adj[:, pad] = -np.inf
                if mask_eos and eos >= 0:
                    adj[:, eos] = -np.inf
                ref = fr.ref_argmax(logits.astype(np.float64), pad, eos, mask_eos, bias.astype(np.float64) if use_bias else None)
                assert np.array_equal(ref, adj.argmax(axis=1))
        assert {"last", "first", "all_neg_inf"} <= set(names)
        if V >= 1000:
            assert {"two_lanes", "two_waves", "same_thread", "all_at_once", "pad_max", "eos_max", "eos_bias_wins", "eos_bias_ties_lower",
                    "eos_bias_ties_higher"} <= set(names)
        if V == 257:
            assert "same_thread_0_256" in names
    # the planted ties sit where they are meant to: one wave, two waves, one thread
    assert 5 // 64 == 37 // 64 and 10 // 64 != 138 // 64 and (263 - 7) % 256 == 0 and 7 % 256 == 263 % 256


def _am_mutation_seen(mut):
    n = 0
    for V in fe.AM_V:
        logits, bias, pad, eos, names = fe.am_case(V)
        l64 = logits.astype(np.float64)
        n += not np.array_equal(fr.ref_argmax(l64, pad, eos, False, None, mut), fr.ref_argmax(l64, pad, eos, False, None))
    return n


def test_embed_reference():
    E = np.arange(12, dtype=np.float64).reshape(4, 3)
    pos = 0.5 * np.ones((2, 3))
    val, mag = fr.ref_embed([3, 0], E, pos, [1, 1], 2.0)
    assert np.array_equal(val, np.array([[18.5, 20.5, 22.5], [0.5, 2.5, 4.5]])) and np.array_equal(mag, np.abs(val))


# ---- the mutation table -----------------------------------------------------------------------------------------------------------------
SEEN_BY = {"fbank": _fb_mutation_seen, "conv": _conv_mutation_seen, "layernorm": _ln_mutation_seen, "prenorm": _pn_mutation_seen,
           "pack": _pk_mutation_seen, "argmax": _am_mutation_seen}


@pytest.mark.parametrize("family,mut", [(f, m) for f, ms in fr.MUTATIONS.items() for m in ms])
def test_mutation_changes_a_case(family, mut):
    """cases that notice each mistake: at least one, except for the three mistakes no case can see (module docstring), where it is none"""
    n = SEEN_BY[family](mut)
    print(f"{family} / {mut}: noticed by {n} case(s)")
    if mut in INVISIBLE:
        assert n == 0, (mut, "is visible after all: take it out of INVISIBLE")
    else:
        assert n > 0, (mut, "no case notices")


def test_invisible_mutations_move_nothing():
    """the three: identical on every compared element, not merely inside the bound"""
    for name in fe.FB_NAMES:
        for r, m in zip(fe.fb_ref(name), fe.fb_ref(name, "preemph0_zero")):
            assert np.array_equal(r["e"], m["e"])
    for (T, S, n_rc, lens) in _pn_cases():
        c = fe.pn_case(64, False, T, S, n_rc, lens)
        m = fr.ref_prenorm(c["X"].astype(np.float64), c["g"].astype(np.float64), c["b"].astype(np.float64), lens, T, n_rc, S, "cnt_no_max")
        live = fe.pn_live(T, S, lens)
        assert np.array_equal(m[2][live], c["summ"][live]) and np.array_equal(m[3][live], c["cnt"][live])
        assert (m[3][~live] <= 0).all() and (c["cnt"][~live] == 1).all()
    for (T, S, R) in fe.PK_TSR:
        assert all((-(-T // S)) * S + r >= T for r in range(R))


def test_every_instantiation_has_a_case():
    fe.test_every_instantiation_has_a_case()
