"""CPU checks of the float64 reference of the decoder layer chains (tests/dec_chain_ref.py) and of its case table
(tests/dec_chain_cases.py): the rounding helpers on hand-computed values, the reference against the torch emulation of
tests/test_hip_dec_chain.py, every mutant seen by the table, and the bounds not vacuous (at most 2 % of the elements compared by bound
have |ref| below their own bound, per case and stage output)."""
import numpy as np
import pytest
import torch

import dec_chain_cases as C
import dec_chain_ref as R

_REF = {}


def _ref(c):
    """(operands, reference stages, the visible arrays a later stage reads) of a case, computed once"""
    if c["name"] not in _REF:
        if c in C.PROJ_CASES:
            o = C.proj_operands(c)
            st = C.proj_stages(o)
            seen = {"x": R.round_once(st["x"][0])}
        elif c in C.FFN_CASES:
            o = C.ffn_operands(c)
            info = []
            st = C.ffn_stages(o, info=info)
            st["info"] = info
            seen = {"x_mid": R.round_once(st["x_mid"][0]), "slabs": C.f32(st["slabs"][0])}
        elif c in C.SUM_CASES:
            o = C.sum_operands(c)
            st = C.sum_stages(o)
            seen = {"x": R.round_once(st["x"][0])}
        else:
            o = C.vocab_operands(c)
            st = C.vocab_stages(o)
            seen = {"x": R.round_once(st["x"][0])}
        _REF[c["name"]] = (o, st, seen)
    return _REF[c["name"]]


def _stages(c, o, seen, mut):
    f = C.proj_stages if c in C.PROJ_CASES else C.ffn_stages if c in C.FFN_CASES else C.sum_stages if c in C.SUM_CASES else C.vocab_stages
    return f(o, seen=seen, mut=mut)


# ======================================================================================================================================
# helpers on hand-computed values
# ======================================================================================================================================
def test_bf16_helpers_on_hand_computed_values():
    sp = R.bf16_spacing
    assert sp(1.0) == 2.0 ** -7 and sp(1.5) == 2.0 ** -7 and sp(1.9999) == 2.0 ** -7      # [1, 2): 8 significant bits
    assert sp(2.0) == 2.0 ** -6 and sp(-2.0) == 2.0 ** -6                                  # a binade boundary: the spacing above
    assert sp(0.999) == 2.0 ** -8 and sp(0.5) == 2.0 ** -8 and sp(300.0) == 2.0
    assert sp(0.0) == 2.0 ** -133 and sp(2.0 ** -130) == 2.0 ** -133                       # subnormal spacing
    r = R.round_once
    assert r(1.0 + 2.0 ** -8) == 1.0                                                       # a midpoint: to the even significand (128)
    assert r(1.0 + 3 * 2.0 ** -8) == 1.0 + 2.0 ** -6                                       # 129.5 -> 130
    assert r(1.0 + 2.0 ** -8 + 2.0 ** -30) == 1.0 + 2.0 ** -7 and r(1.0 + 2.0 ** -8 - 2.0 ** -30) == 1.0
    assert r(2.0 - 2.0 ** -9) == 2.0                                                       # 255.5 -> 256: into the next binade
    assert r(-0.3) == -0.30078125 and r(0.0) == 0.0 and r(4.0) == 4.0
    v = np.random.default_rng(0).standard_normal(4096).astype(np.float32) * np.float32(37.0)
    assert np.array_equal(r(v.astype(np.float64)), torch.from_numpy(v).bfloat16().double().numpy())      # torch on fp32 numbers
    assert np.array_equal(R.to_bf16_bits(r(v.astype(np.float64))), torch.from_numpy(v).bfloat16().view(torch.int16).numpy())
    md = R.midpoint_distance
    assert md(1.0 + 2.0 ** -8) == 0.0 and R.fragile(1.0 + 2.0 ** -8, 0.0)                  # exactly on a midpoint: fragile at e = 0
    assert md(1.0 + 2.0 ** -7) == 2.0 ** -8 and not R.fragile(1.0 + 2.0 ** -7, 2.0 ** -9)  # a bf16 number: half a spacing away
    assert R.fragile(1.0 + 2.0 ** -7, 2.0 ** -8)
    assert md(2.0) == 2.0 ** -8                                                            # at a binade boundary the midpoint BELOW is nearer:
    assert md(1.0) == 2.0 ** -9                                                            # 1 - 2^-9, not 1 + 2^-8
    assert md(1.0 + 2.0 ** -12) == 2.0 ** -9 + 2.0 ** -12
    assert md(1.0 - 2.0 ** -12) == 2.0 ** -9 - 2.0 ** -12
    assert md(2.0 - 2.0 ** -10) == 3 * 2.0 ** -10                                          # own last midpoint 2 - 2^-8
    assert R.fragile(1.0 + 2.0 ** -12, 2.0 ** -8) and not R.fragile(1.0 + 2.0 ** -12, 2.0 ** -10)
    assert R.flip_amount(1.0, 2.0 ** -12) == 2.0 ** -7                                     # one spacing
    assert R.flip_amount(2.0 - 2.0 ** -12, 2.0 ** -10) == 2.0 ** -6                        # ... of the binade |v| + e reaches
    assert R.flip_amount(2.0 ** -20, 2.0 ** -10) == 2.0 ** -10 + R.bf16_spacing(2.0 ** -10 + 2.0 ** -20)      # e above half a spacing
    y, amt = R.hidden_round(np.array([1.0 + 2.0 ** -8, 1.25]), np.array([0.0, 1e-6]))
    assert y.tolist() == [1.0, 1.25] and amt.tolist() == [2.0 ** -7, 0.0]


def test_layer_norm_classes():
    """a constant row normalises to beta exactly and carries no error; the offset rows' bound carries the cancellation term"""
    o = C.proj_operands(C.BY_NAME["proj-q-B17"])
    x = R.round_once(R.stage_residual(o["ctx"], o["x"], o["Wo"], o["bo"])[0])
    rows = C.class_rows(o["classes"])
    y, e = R.layer_norm(x, o["gamma"], o["beta"])
    i = rows["const"][0]
    assert (x[i] == 4.0).all() and np.array_equal(y[i], o["beta"]) and (e[i] == 0).all()
    var = x.var(1)
    assert 5e-6 < var[rows["tiny"][0]] < 1e-4                                              # the size of eps
    assert abs(x[rows["off32"][0]].mean() - 32) < 0.5 and abs(x[rows["off8"][0]].mean() - 8) < 0.5
    rel = (e / (np.abs(y) + 1e-3)).mean(1)
    assert rel[rows["off32"][0]] > 4 * rel[rows["off8"][0]] > 40 * rel[rows["normal"][0]]
    assert (x[rows["ctx0"][0]] == R.round_once(o["x"][rows["ctx0"][0]] + o["bo"])).all()


# ======================================================================================================================================
# the reference against the torch emulation of tests/test_hip_dec_chain.py, on that test's inputs and within its tolerance
# ======================================================================================================================================
def _bf(t):
    return t.to(torch.bfloat16).float()


def _ln(x, g, b):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), g, b, 1e-5)


def _rand(shape, gen, scale=1.0):
    return torch.randn(*shape, generator=gen) * scale


def _np(t):
    return t.double().numpy()


def test_reference_agrees_with_the_torch_emulation():
    D, B, F = 256, 130, 2048
    g = torch.Generator().manual_seed(B + 1)                 # test_proj_chain_vs_torch, soft
    ctx, x = _bf(_rand((B, D), g)), _bf(_rand((B, D), g))
    Wo, Wq, Wq2 = (_bf(_rand((D, D), g, D ** -0.5)) for _ in range(3))
    bo, bq, bq2 = (_rand((D,), g, 0.1) for _ in range(3))
    lg, lb = 1 + _rand((D,), g, 0.1), _rand((D,), g, 0.1)
    x_ref = _bf(x + ctx @ Wo.T + bo)
    xn = _bf(_ln(x_ref, lg, lb))
    q_ref, q2_ref = _bf(xn @ Wq.T + bq), _bf(xn @ Wq2.T + bq2)
    o = dict(ctx=_np(ctx), x=_np(x), Wo=_np(Wo), bo=_np(bo), gamma=_np(lg), beta=_np(lb), Wq=_np(Wq), bq=_np(bq), Wq2=_np(Wq2), bq2=_np(bq2),
             kk=None)
    st = C.proj_stages(o)
    rnd = lambda k: torch.from_numpy(R.round_once(st[k][0])).float()
    torch.testing.assert_close(rnd("x"), x_ref, atol=0.04, rtol=0.01)
    assert (rnd("x") == x_ref).float().mean() > 0.98
    torch.testing.assert_close(rnd("q"), q_ref, atol=0.06, rtol=0.02)
    torch.testing.assert_close(rnd("q2"), q2_ref, atol=0.06, rtol=0.02)
    g = torch.Generator().manual_seed(B + F)                 # test_ffn_chain_vs_torch
    ctx, x = _bf(_rand((B, D), g)), _bf(_rand((B, D), g))
    Wco = _bf(_rand((D, D), g, D ** -0.5))
    W1, W2 = _bf(_rand((F, D), g, D ** -0.5)), _bf(_rand((D, F), g, F ** -0.5))
    bco, b1, b2 = _rand((D,), g, 0.1), _rand((F,), g, 0.1), _rand((D,), g, 0.1)
    lg, lb = 1 + _rand((D,), g, 0.1), _rand((D,), g, 0.1)
    x1 = _bf(x + ctx @ Wco.T + bco)
    hid = _bf(torch.nn.functional.gelu(_bf(_ln(x1, lg, lb)) @ W1.T + b1))
    ref = _bf(x1 + hid @ W2.T + b2)
    Wqkv, bqkv = _bf(_rand((3 * D, D), g, D ** -0.5)), _rand((3 * D,), g, 0.1)
    l1g, l1b = 1 + _rand((D,), g, 0.1), _rand((D,), g, 0.1)
    ref_qkv = _bf(_bf(_ln(ref, l1g, l1b)) @ Wqkv.T + bqkv)
    o = dict(ctx=_np(ctx), x=_np(x), Wco=_np(Wco), bco=_np(bco), gamma=_np(lg), beta=_np(lb), W1=_np(W1), b1=_np(b1), W2=_np(W2), b2=_np(b2))
    st = C.ffn_stages(o)
    x2 = R.round_once(st["x"][0])
    torch.testing.assert_close(torch.from_numpy(x2).float(), ref, atol=0.06, rtol=0.02)
    qkv = R.stage_ln_proj(x2, _np(l1g), _np(l1b), _np(Wqkv), _np(bqkv))[0]
    torch.testing.assert_close(torch.from_numpy(R.round_once(qkv)).float(), ref_qkv, atol=0.06, rtol=0.02)


# ======================================================================================================================================
# the case table
# ======================================================================================================================================
def test_case_table_covers_what_it_claims():
    for cases in (C.PROJ_CASES, C.FFN_CASES, C.SUM_CASES):
        assert {c["B"] for c in cases} == set(C.ROWS)
        assert len({c["rot"] for c in cases if c["B"] == 1}) == len([c for c in cases if c["B"] == 1])
    assert {c["F"] // 256 for c in C.FFN_CASES} == {1, 8, 9, 32} == {c["n"] for c in C.SUM_CASES}
    assert {c["B"] for c in C.FFN_CASES if c["F"] == 8192} == {1, 17, 33}
    for n in (1, 8, 9, 32):
        assert {c["qkv"] for c in C.SUM_CASES if c["n"] == n} == {True, False}
    assert {(c["V"], c["split"]) for c in C.VOCAB_CASES} == {(256, 1), (512, 2), (1024, 1), (4096, 16), (16384, 64)}
    assert [c["B"] for c in C.VOCAB_CASES if c["V"] == 16384] == [17]
    assert {c["mode"] for c in C.VOCAB_CASES} == {0, 1, 2, 3, 4} and {c["row_bias"] for c in C.VOCAB_CASES} == {True, False}
    assert any(c["row_bias_col"] >= c["V"] // c["split"] for c in C.VOCAB_CASES)
    for c in C.ALL_CASES:
        if c["B"] >= 15:
            o = _ref(c)[0]
            assert set(o["classes"]) == set(C.SUM_CLASSES if "x_mid" in o else C.CLASSES), c["name"]
    # every tie partner of column 5 is a row's largest logit somewhere: same lane, lane group, column tile, wave, weight block, range
    seen = set()
    for c in C.VOCAB_CASES:
        o, st, _ = _ref(c)
        Lb = st["logits"][0].copy()
        for s in (o["skip_a"], o["skip_b"]):
            if s >= 0:
                Lb[:, s] = -np.inf
        top = Lb.argmax(1)
        kind = "range" if c["tie"] == o["VC"] + 5 else c["tie"]
        assert c["tie"] in (6, 9, 21, 69, 261, o["VC"] + 5)
        if np.isin(top, o["tie_group"]).any():
            seen.add(kind)
    assert seen == {6, 9, 21, 69, 261, "range"}, seen


def test_exact_rows_are_exact_in_bf16():
    """x + W ctx + b and x_mid + b2 + slabs of the exact rows are bf16 numbers, so the kernels' x must carry exactly these bits"""
    for c in C.ALL_CASES:
        o, st, _ = _ref(c)
        rows = C.class_rows(o["classes"]).get("exact")
        if rows is None:
            continue
        first = st["x_mid"] if c in C.FFN_CASES else st["x"]
        v = first[0][rows]
        assert np.array_equal(R.round_once(v), v) and np.abs(v).max() < 32 and np.abs(v).max() > 1, c["name"]
        if c in C.SUM_CASES or c in C.VOCAB_CASES:           # ... and every partial sum is a multiple of 1/8
            assert np.array_equal(o["slabs"][:, rows] * 4, np.round(o["slabs"][:, rows] * 4))


def test_feed_forward_blocks_flush_and_pass():
    for c in C.FFN_CASES:
        o, st, _ = _ref(c)
        for inf in st["info"]:
            assert (inf["pre"][:, o["flush"]] < -6).all() and (inf["pre"][:, o["ident"]] > 6).all(), c["name"]


def _compared(c, o, st):
    """(stage name, |ref|, bound) of every element compared by bound; the exact rows of the bf16 sums are compared by bits"""
    rows = np.array([cl not in C.EXACT_CLASSES for cl in o["classes"]])
    first = {"proj": "x", "ffn": "x_mid", "sum": "x", "vocab": "x"}[c["name"].split("-")[0]]
    for k, v in st.items():
        if k in ("info", "plain"):
            continue
        val, bound = v
        if k == first:
            if not rows.any():
                continue
            val, bound = val[rows], bound[rows]
        yield k, np.abs(val), bound


@pytest.mark.parametrize("family", ["proj", "ffn", "sum", "vocab"])
def test_bounds_are_not_vacuous(family):
    """at most 2 % of the elements compared by bound have |ref| below their own bound, per case and stage output"""
    for c in C.ALL_CASES:
        if not c["name"].startswith(family):
            continue
        o, st, _ = _ref(c)
        for k, a, b in _compared(c, o, st):
            assert np.isfinite(a).all() and np.isfinite(b).all() and (b > 0).all(), (c["name"], k)
            share = float((a < b).mean())
            print(f"{c['name']}: {k}: {100 * share:.2f} % of {a.size} elements below their bound, median bound / median |ref| = "
                  f"{np.median(b) / np.median(a):.2e}")
            assert share <= 0.02, (c["name"], k, share)


def test_method_figures():
    """the figures of the flip-term method on the real module (printed; DESIGN.md records them)"""
    c = C.BY_NAME["ffn-F2048-B129"]
    o, st, seen = _ref(c)
    rows = np.array([cl == "normal" for cl in o["classes"]])
    val, bound = st["slabs"][0][:, rows], st["slabs"][1][:, rows]
    inf = st["info"]
    allflip = np.stack([i["allflip"] for i in inf])[:, rows]
    drop = np.stack([(i["hb"][:, -32:] @ i["W2s"][:, -32:].T) for i in inf])[:, rows]      # what the last k-step of fc2 contributes
    figs = dict(frag_ln=np.mean([i["frag_ln"][rows] for i in inf]), frag_h=np.mean([i["frag_h"][rows] for i in inf]), med_bound=np.median(bound),
                med_mag=np.median(np.abs(val)), med_allflip=np.median(allflip), dropped_seen=float((np.abs(drop) > bound).mean()),
                below=float((np.abs(val) < bound).mean()))
    print("ffn-F2048-B129, N(0, 1) rows: fragile LayerNorm outputs %.3f %%, fragile GELU outputs %.1f %%, median slab bound %.2e, median "
          "slab magnitude %.2e, median all-flip bound %.2e, elements where a slab without its last k-step leaves its bound %.1f %%, "
          "reference elements below their own bound %.2f %%" % (100 * figs["frag_ln"], 100 * figs["frag_h"], figs["med_bound"], figs["med_mag"],
                                                               figs["med_allflip"], 100 * figs["dropped_seen"], 100 * figs["below"]))
    assert figs["med_bound"] < 0.1 * figs["med_allflip"] * 8 and figs["dropped_seen"] > 0.5


# ======================================================================================================================================
# mutants
# ======================================================================================================================================
PICK_MUTANTS = ("pick_highest_column_on_tie", "pick_ge_instead_of_gt_across_lanes", "skip_before_row_bias", "row_bias_on_every_range",
                "skip_b_ignored", "fold_takes_first_pair")


def _mutant_seen(c, mut):
    o, st, seen = _ref(c)
    if mut in PICK_MUTANTS:
        if c not in C.VOCAB_CASES:
            return False
        Lb, bound = st["logits"]
        vals, cols = C.ref_pairs(c, o, st["plain"], mut)
        folded = R.fold(*C.ref_pairs(c, o, st["plain"]), mut=mut) if mut == "fold_takes_first_pair" else R.fold(vals, cols, mut=mut)
        if mut == "fold_takes_first_pair":
            vals, cols = C.ref_pairs(c, o, st["plain"])
        return bool(C.check_pairs(c, o, vals, cols, Lb, bound, folded)[0])
    got = _stages(c, o, seen, mut)
    for k, a, b in _compared(c, o, st):
        rows = slice(None)
        if a.shape != got[k][0].shape:                       # the first stage: the rows compared by bound
            rows = np.array([cl not in C.EXACT_CLASSES for cl in o["classes"]])
        ref = st[k][0][rows] if a.shape != got[k][0].shape else st[k][0]
        if (np.abs(got[k][0][rows] - ref) > b).any():
            return True
    return False


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_every_mutant_is_seen(mut):
    """with the unmutated stage inputs, at least one case has an element where |mutant - reference| exceeds that element's bound (the
    pick mutants: a pair that breaks check_pick's conditions)"""
    hits = []
    for c in C.ALL_CASES:
        if c["B"] == 129 and c not in C.VOCAB_CASES and hits:
            continue                                          # (the long cases only while nothing has seen it)
        if _mutant_seen(c, mut):
            hits.append(c["name"])
            if len(hits) >= 3:
                break
    print(f"{mut}: seen by {hits}")
    assert hits, mut


def test_reference_pairs_meet_their_own_conditions():
    for c in C.VOCAB_CASES:
        o, st, _ = _ref(c)
        vals, cols = C.ref_pairs(c, o, st["plain"])
        bad, worst = C.check_pairs(c, o, vals, cols, *st["logits"])
        assert not bad and worst < 1e-3, (c["name"], bad, worst)
        if o["row_bias"] is not None and c["mode"] == 3:      # the addend does not resurrect the skipped column
            assert not (cols == c["row_bias_col"]).any()
        elif o["row_bias"] is not None:
            s = c["row_bias_col"] // o["VC"]
            assert (cols[::3, s] == c["row_bias_col"]).all()
