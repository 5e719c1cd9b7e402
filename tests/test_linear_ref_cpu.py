"""The float64 reference of simulst_linear (tests/linear_ref.py) and the case table (tests/linear_cases.py), checked without a GPU:

  * the reference against independent code: torch's F.linear / F.gelu / F.layer_norm / F.glu in float64 over strided views of the raw
    buffers, the convolution cases against oracle.causal_conv.causal_conv1d from the un-packed Conv1d weight, EMF_OUT against the lines
    of oracle/emformer.py attention_impl that split, tanh and drop the summaries;
  * every case's plan (csrc/gemm_plan.cpp through tests/linear_plan_table.cpp) is the family and variant it declares, and the table
    reaches all ten families and every variant flag test_linear_plan.py wants;
  * a correct float32 implementation on the CPU stays inside every RANDOM case's bound (worst ratio printed);
  * each mutant of the reference moves at least one case past its bound;
  * at most 2 % of the RANDOM elements lie below their own bound.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import linear_cases as lc
import linear_ref as lr
from linear_ref import BF16, BIAS, EMF_OUT, F32, F32OUT, GELU, GLU, RES, RES_GELU
from oracle.causal_conv import causal_conv1d
from test_linear_plan import _parse, _plan_lines, table_program  # noqa: F401  (table_program: the fixture)

SMALL = 1 << 24                       # M * N * K up to which the slow checks run on every case


def _work(c):
    d = c["d"]
    return d["M_batches"] * d["rows_per_batch"] * d["N"] * d["K"]


def _a_view(c, o):
    """the rows of A as a strided view of the raw buffer, left padding zeroed -- torch.as_strided, not the reference's gather"""
    d = c["d"]
    B, M, K = d["M_batches"], d["rows_per_batch"], d["K"]
    buf = torch.from_numpy(o["A64"])
    a = torch.as_strided(buf, (B, M, K), (d["a_batch_stride"], d["a_row_stride"], 1), o["a0"] - d["a_lead"]).clone()
    for i in range(M):
        pad = d["a_lead"] - i * d["a_row_stride"]
        if pad <= 0:
            break
        a[:, i, :min(pad, K)] = 0.0
    return a


def _w_rows(c, o):
    d = c["d"]
    N, K, G = d["N"], d["K"], lr.vec_elems(c["dtype"])
    w = torch.from_numpy(o["W64"])[:N * K]
    if d["w_fragment_major"]:            # [n / 16][k / KS][(k % KS) / G][n % 16][k % G]
        return w.view(N // 16, K // (4 * G), 4, 16, G).permute(0, 3, 1, 2, 4).reshape(N, K)
    return w.view(N, K)


def _glu_unpack(wp, bp):
    """inverse of the 64-row block order: channel c pairs with c + N / 2 (F.glu)"""
    N = wp.shape[0]
    idx = torch.arange(N // 2).view(-1, 32)
    perm = torch.cat([idx, idx + N // 2], dim=1).reshape(-1)
    w, b = torch.empty_like(wp), torch.empty_like(bp)
    w[perm], b[perm] = wp, bp
    return w, b


def _c_view(c, rows_c, N):
    """flat output offsets [B][rows][N] from torch.as_strided over an arange"""
    d = c["d"]
    B, hd, th = d["M_batches"], d["c_head_dim"], d["c_tensor_heads"]
    if not hd:
        n = (B - 1) * d["c_batch_stride"] + (rows_c - 1) * d["c_row_stride"] + N
        return torch.as_strided(torch.arange(n), (B, rows_c, N), (d["c_batch_stride"], d["c_row_stride"], 1))
    heads = N // hd
    if not th:
        n = (B - 1) * d["c_batch_stride"] + (heads - 1) * d["c_head_stride"] + (rows_c - 1) * d["c_row_stride"] + hd
        v = torch.as_strided(torch.arange(n), (B, heads, rows_c, hd), (d["c_batch_stride"], d["c_head_stride"], d["c_row_stride"], 1))
        return v.permute(0, 2, 1, 3).reshape(B, rows_c, N)
    T = heads // th
    n = (T - 1) * d["c_tensor_stride"] + (B - 1) * d["c_batch_stride"] + (th - 1) * d["c_head_stride"] + (rows_c - 1) * d["c_row_stride"] + hd
    v = torch.as_strided(torch.arange(n), (T, B, th, rows_c, hd),
                         (d["c_tensor_stride"], d["c_batch_stride"], d["c_head_stride"], d["c_row_stride"], 1))
    return v.permute(1, 3, 0, 2, 4).reshape(B, rows_c, N)


def _independent(c, o):
    """{stream: (idx, val)} from torch float64 library calls"""
    d = c["d"]
    B, M, N, K, epi = d["M_batches"], d["rows_per_batch"], d["N"], d["K"], d["epilogue"]
    a, w, b = _a_view(c, o), _w_rows(c, o), torch.from_numpy(o["bias64"])[:N]
    if c["ln"]:
        a = F.layer_norm(a, (K,), torch.from_numpy(o["gamma64"]), torch.from_numpy(o["beta64"]), 1e-5)
    r = None
    if o["R"] is not None:
        rows_c = d["n_main"] if epi == EMF_OUT else M
        r = torch.as_strided(torch.from_numpy(o["R64"]), (B, rows_c, N), (d["r_batch_stride"], d["r_row_stride"], 1), o["r0"])
    if epi == GLU:
        wu, bu = _glu_unpack(w, b)
        if c["flags"].get("conv"):       # the call as the Conv1d it stands for: channel-last x, W [C_out][k][C_in]
            cin = K - d["a_lead"]
            k, stride = K // cin, d["a_row_stride"] // cin
            T = stride * (M - 1) + 1
            x = torch.as_strided(torch.from_numpy(o["A64"]), (B, T, cin), (d["a_batch_stride"], cin, 1), o["a0"])
            y = causal_conv1d(x.transpose(1, 2), wu.view(N, k, cin).permute(0, 2, 1), bu, stride=stride)
            y = F.glu(y, dim=1).transpose(1, 2) * d["scale"]
        else:
            y = F.glu(F.linear(a, wu, bu), dim=-1) * d["scale"]
        return {"C": (_c_view(c, M, N // 2), y)}
    if c["flags"].get("conv"):
        cin = K - d["a_lead"]
        k, stride = K // cin, d["a_row_stride"] // cin
        T = stride * (M - 1) + 1
        x = torch.as_strided(torch.from_numpy(o["A64"]), (B, T, cin), (d["a_batch_stride"], cin, 1), o["a0"])
        y = causal_conv1d(x.transpose(1, 2), w.view(N, k, cin).permute(0, 2, 1), b, stride=stride).transpose(1, 2)
    else:
        y = F.linear(a, w, b)
    if epi == EMF_OUT:
        # oracle/emformer.py attention_impl: out = _lin(out_proj, ctx); out_rc_utt, out_mems = out[:T - n_sum], out[T - n_sum:];
        # out_mems = tanh(out_mems); emformer_forward keeps mems[:-1] (here: the first aux_rows) -- per utterance, rows first
        n_sum = M - d["n_main"]
        out = y.transpose(0, 1)
        out_rc_utt, out_mems = out[:M - n_sum], out[M - n_sum:]
        out_mems = torch.tanh(out_mems)[:d["aux_rows"]]
        main = out_rc_utt.transpose(0, 1) + r
        na = out_mems.shape[0]
        aidx = torch.as_strided(torch.arange(B * d["aux_batch_stride"] + na * N + 1), (B, na, N), (d["aux_batch_stride"], N, 1))
        return {"C": (_c_view(c, d["n_main"], N), main), "aux": (aidx, out_mems.transpose(0, 1))}
    if epi in (RES, RES_GELU):
        y = y + r
    if epi in (GELU, RES_GELU):
        y = F.gelu(y)
    return {"C": (_c_view(c, M, N), y)}


SMALL_CASES = [c for c in lc.CASES if _work(c) <= SMALL]


def _rule_key(c):
    """what of the reference a case exercises: epilogue, C address form, LayerNorm, weight order, A addressing, strides, class"""
    d = c["d"]
    return (c["family"], c["dtype"], d["epilogue"], (d["c_head_dim"] > 0) + (d["c_tensor_heads"] > 0), c["ln"], d["w_fragment_major"],
            d["a_lead"] > 0, d["a_row_stride"] < d["K"], d["M_batches"] > 1, bool(c["flags"].get("conv")), c["cls"])


def _independent_cases(family):
    """every case up to SMALL, and above it the smallest case of every rule combination: each rule the reference states is compared
    with independent code in every family that uses it"""
    picked, have = [], set()
    for c in sorted((c for c in lc.CASES if c["family"] == family), key=_work):
        if _work(c) <= SMALL or _rule_key(c) not in have:
            picked.append(c)
        have.add(_rule_key(c))
    return picked


@pytest.mark.parametrize("family", lc.FAMILIES)
def test_reference_against_independent_code(family):
    cases = _independent_cases(family)
    assert cases
    forms = {(c["d"]["c_head_dim"] > 0) + (c["d"]["c_tensor_heads"] > 0) for c in lc.CASES if c["family"] == family}
    assert {(c["d"]["c_head_dim"] > 0) + (c["d"]["c_tensor_heads"] > 0) for c in cases} == forms
    kinds = set()
    for c in cases:
        o = lc.operands(c)
        streams, _ = lc.run_reference(c, o)
        ind = _independent(c, o)
        assert set(ind) == set(streams), c["name"]
        for name, (idx, val) in ind.items():
            st = streams[name]
            assert np.array_equal(st["idx"].ravel(), idx.reshape(-1).numpy()), (c["name"], name, "addresses")
            got, want = st["val"].ravel(), val.reshape(-1).numpy()
            assert np.isfinite(want).all() and np.isfinite(got).all(), (c["name"], name, "a guard NaN reached an output")
            assert np.all(np.abs(got - want) <= 1e-12 * (1.0 + np.abs(want)) + 1e-13 * np.abs(want).max(initial=0.0)), (c["name"], name)
        kinds.add((c["d"]["epilogue"], bool(c["flags"].get("conv"))))
    if family in ("tile128", "tile64"):
        assert {e for e, _ in kinds} >= ({GLU, EMF_OUT, GELU} if family == "tile128" else {BIAS, GELU, RES, F32OUT, RES_GELU, EMF_OUT})
    if family == "tile128":
        assert (GLU, True) in kinds and (GELU, True) in kinds


def test_fragment_index_is_a_permutation():
    for dtype in (F32, BF16):
        KS = 4 * lr.vec_elems(dtype)
        for N, K in ((16, KS), (48, 8 * KS), (768, 256)):
            assert np.array_equal(np.sort(lr.fragment_index(N, K, dtype).ravel()), np.arange(N * K))


# ---- plan coverage ----------------------------------------------------------------------------------------------------------------------
FLAG_OF = {"ln_": "ln", "tall": "tall", "ring": "ring", "pairs": "pairs", "MTs": "MTs", "NTs": "NTs", "splits": "splits"}


def test_every_case_reaches_the_kernel_it_declares(table_program):  # noqa: F811
    out = _plan_lines(table_program, "plan", [lc.plan_line(c) for c in lc.CASES])
    seen, flags = set(), set()
    for c, line in zip(lc.CASES, out):
        fam, p = _parse(line)
        assert fam == c["family"], (c["name"], line)
        for k, v in c["flags"].items():
            if k in FLAG_OF:
                assert p[FLAG_OF[k]] == v, (c["name"], k, line)
        if fam == "skinny":
            assert (p["splits"] > 1) == bool(c["flags"].get("split", False)), (c["name"], line)
            assert p["splits"] == c["flags"].get("splits", 1), (c["name"], line)
        assert p["ln"] == int(c["ln"]) or fam in ("tile128", "tile64", "tile256", "wstat", "panel_wide"), (c["name"], line)
        seen.add(fam)
        flags |= {(fam, f, p[f]) for f in ("ln", "tall", "ring", "pairs", "MTs", "NTs") if (fam, f) in
                  {("panel", "ln"), ("panel_split", "ln"), ("mid", "ln"), ("mid", "tall"), ("wave_tile", "ln"), ("skinny", "ln"),
                   ("skinny", "MTs"), ("skinny", "NTs"), ("tile256", "ring"), ("wstat", "pairs")}}
        if fam == "skinny":
            flags.add(("skinny", "split", p["splits"] > 1))
            flags.add(("skinny", "tile", p["MTs"], p["NTs"]))
    assert seen == set(lc.FAMILIES)
    want = {(f, "ln", v) for f in ("panel", "panel_split", "mid", "wave_tile", "skinny") for v in (0, 1)}
    want |= {("mid", "tall", 0), ("mid", "tall", 1), ("tile256", "ring", 0), ("tile256", "ring", 1), ("wstat", "pairs", 6), ("wstat", "pairs", 8),
             ("skinny", "split", False), ("skinny", "split", True)}
    want |= {("skinny", "MTs", v) for v in (1, 2, 4)} | {("skinny", "NTs", v) for v in (1, 2)}
    assert {f for f in flags if f[1] != "tile"} == want
    # every (MTs, NTs) plan_skinny can end on: the shrink loop stops at (4, 2), (4, 1), (2, 1) or (1, 1), the M <= 64 policy turns
    # (1, 1) into (1, 2), split-K forces MTs = 1 and the LayerNorm's limit turns 4 row tiles into 2: (2, 2) and (2, 1)
    assert {f[2:] for f in flags if f[1] == "tile"} == {(4, 2), (4, 1), (2, 1), (1, 1), (1, 2), (2, 2)}
    # both dtypes wherever the family takes fp32
    for fam in ("skinny", "wave_tile", "mid", "tile128", "tile64"):
        assert {c["dtype"] for c in lc.CASES if c["family"] == fam} == {F32, BF16}


# ---- the bound is reachable, and little hides below it -------------------------------------------------------------------------------
def _emulate32(c, o):
    """the call in torch float32 on the CPU: operands as stored, the LayerNorm rounded to the operand dtype, one rounded store"""
    d = c["d"]
    B, M, N, K, epi = d["M_batches"], d["rows_per_batch"], d["N"], d["K"], d["epilogue"]
    t = lc.tdt(c["dtype"])
    a = _a_view(c, o).float().reshape(B * M, K)
    if c["ln"]:
        a = lc.ln_formula32(a, o["gamma"], o["beta"]).to(t).float()
    pre = a @ _w_rows(c, o).float().t() + o["bias"][:N]
    rows_c = d["n_main"] if epi == EMF_OUT else M
    if o["R"] is not None:
        r = torch.as_strided(o["R"], (B, rows_c, N), (d["r_batch_stride"], d["r_row_stride"], 1), o["r0"]).float()
    ot = torch.float32 if epi == F32OUT else t
    pre = pre.view(B, M, N)
    if epi == EMF_OUT:
        return {"C": (pre[:, :rows_c] + r).to(ot).double().numpy().reshape(-1, N),
                "aux": torch.tanh(pre[:, rows_c:rows_c + d["aux_rows"]]).to(ot).double().numpy().reshape(-1, N)}
    if epi in (RES, RES_GELU):
        pre = pre + r
    if epi in (GELU, RES_GELU):
        pre = F.gelu(pre)
    if epi == GLU:
        q, j = torch.arange(N // 2) // 32, torch.arange(N // 2) % 32
        pre = d["scale"] * pre[..., 64 * q + j] * torch.sigmoid(pre[..., 64 * q + 32 + j])
    return {"C": pre.to(ot).double().numpy().reshape(B * M, -1)}


def test_float32_on_the_cpu_stays_inside_the_bound_and_little_hides_below_it():
    worst, below, total, most = {}, 0, 0, (0.0, None)
    for c in lc.CASES:
        if c["cls"] != "RANDOM":
            continue
        o = lc.operands(c)
        streams, mags = lc.run_reference(c, o)
        k = lc.measured_constants(c, o, mags)
        bnd = lc.bounds(c, streams, mags, k)
        emu = _emulate32(c, o)
        for name, st in streams.items():
            assert np.isfinite(st["val"]).all(), (c["name"], name)
            q = np.abs(emu[name] - st["val"]) / bnd[name]
            key = (c["family"], "bf16" if c["dtype"] == BF16 else "f32")
            worst[key] = max(worst.get(key, 0.0), float(q.max()))
            assert float(q.max()) <= 1.0, (c["name"], name, float(q.max()), k)
            hid = int((np.abs(st["val"]) < bnd[name]).sum())
            below, total = below + hid, total + st["val"].size
            if st["val"].size and hid / st["val"].size > most[0]:
                most = (hid / st["val"].size, c["name"])
    for key in sorted(worst):
        print(f"float32 on the CPU, worst |got - ref| / bound, {key[0]} {key[1]}: {worst[key]:.3f}")
    print(f"elements below their own bound: {below} of {total} ({100.0 * below / total:.3f} %)")
    print(f"the case with the largest share: {most[1]}, {100.0 * most[0]:.1f} %")
    assert below <= 0.02 * total


# ---- the cases can fail -----------------------------------------------------------------------------------------------------------------
def _res(c):
    return c["d"]["epilogue"] in (RES, EMF_OUT, RES_GELU)


APPLIES = {      # which cases a mutant changes at all
    "last_k_group_dropped": lambda c: True,
    "last_split_tail_dropped": lambda c: c["flags"].get("splits", 1) > 1 and c["d"]["K"] % (c["flags"]["splits"] * 4 * lr.vec_elems(c["dtype"])) != 0,
    "last_row_from_the_row_before": lambda c: c["d"]["M_batches"] * c["d"]["rows_per_batch"] > 1,
    "batch_row_through_row_stride": lambda c: c["d"]["M_batches"] > 1 and c["d"]["a_batch_stride"] != c["d"]["rows_per_batch"] * c["d"]["a_row_stride"],
    "bias_shifted_on_n_tail": lambda c: c["d"]["N"] % 16 != 0,
    "residual_with_c_strides": lambda c: _res(c) and (c["d"]["r_row_stride"], c["d"]["r_batch_stride"]) != (c["d"]["c_row_stride"], c["d"]["c_batch_stride"]),
    "a_lead_minus_G": lambda c: True,
    "negative_offsets_not_zeroed": lambda c: c["d"]["a_lead"] > 0,
    "glu_value_gate_swapped": lambda c: c["d"]["epilogue"] == GLU,
    "glu_scale_dropped": lambda c: c["d"]["epilogue"] == GLU and c["d"]["scale"] != 1.0,
    "last_summary_kept": lambda c: c["d"]["epilogue"] == EMF_OUT and c["d"]["rows_per_batch"] - c["d"]["n_main"] > c["d"]["aux_rows"],
    "tanh_from_n_main_plus_1": lambda c: c["d"]["epilogue"] == EMF_OUT and c["d"]["aux_rows"] > 0,
    "head_plane_by_hd_plus_8": lambda c: c["d"]["c_head_dim"] > 0,
    "tensor_and_head_stride_swapped": lambda c: c["d"]["c_tensor_heads"] > 0,
    "ln_eps_1e-6": lambda c: c["ln"],
    "ln_over_k_rounded_to_KS": lambda c: c["ln"] and c["d"]["K"] % (4 * lr.vec_elems(c["dtype"])) != 0,
    "gelu_tanh_form": lambda c: c["d"]["epilogue"] in (GELU, RES_GELU),
}


def _seen(streams, bnd, mutated, exact_bits):
    """would the GPU test see the mutated result?  another address set, or a value past its bound (or a NaN from a guard)"""
    for name, st in streams.items():
        mt = mutated.get(name)
        if mt is None:
            return True
        oa, ob = np.argsort(st["idx"].ravel()), np.argsort(mt["idx"].ravel())
        if oa.size != ob.size or not np.array_equal(st["idx"].ravel()[oa], mt["idx"].ravel()[ob]):
            return True
        diff = np.abs(mt["val"].ravel()[ob] - st["val"].ravel()[oa])
        b = bnd[name].ravel()[oa]
        if exact_bits and st["act"] is None:
            if np.any(diff != 0):
                return True
        elif not np.all(diff <= b):
            return True
    return False


@pytest.mark.parametrize("mut", lr.MUTANTS)
def test_a_case_sees_every_mutant(mut):
    assert set(APPLIES) == set(lr.MUTANTS)
    cand = sorted((c for c in lc.CASES if APPLIES[mut](c)), key=_work)
    assert cand, f"no case of the table is changed by {mut}"
    caught, fams, tried = [], set(), 0
    for c in cand:
        if _work(c) > SMALL and (c["family"], c["dtype"]) in fams:      # the tall cases: one per family and dtype is enough
            continue
        o = lc.operands(c)
        streams, mags = lc.run_reference(c, o)
        bnd = lc.bounds(c, streams, mags, lc.measured_constants(c, o, mags))
        mutated, _ = lc.run_reference(c, o, mut=mut)
        if _seen(streams, bnd, mutated, c["cls"] == "EXACT"):
            caught.append(c["name"])
        fams.add((c["family"], c["dtype"]))
        tried += 1
        if _work(c) > SMALL:
            assert c["name"] in caught, (mut, c["name"])
    print(f"{mut}: seen by {len(caught)} of the {tried} cases tried ({len(cand)} it changes), e.g. {caught[:3]}")
    assert caught, f"{mut} is invisible to every case"
    if mut in ("last_k_group_dropped", "last_row_from_the_row_before", "a_lead_minus_G"):      # these change every case: every family must see them
        assert {f for f, _ in fams} == set(lc.FAMILIES), (mut, fams)
