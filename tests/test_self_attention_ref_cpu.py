"""tests/self_attention_ref.py held before it is used on the GPU (CPU only).

Anchors.  step_reference, run step after step on its own expected caches, equals the attention inside oracle.decoder._self_attn_step
(the oracle is pinned to the fixtures recorded from the reference implementation; identity projections, so its `out` is the
attention); causal_reference equals the _causal_self_attn restatement of tests/test_teacher_forced_oracle.py; row u of
causal_reference equals step_reference at n_prev = u on the same qkv.  Both oracle forms cast the scores to fp32 for the softmax,
hence 1e-6 and not 1e-12.

Fairness.  What the GPU tests rely on holds for the reference alone: every planted key carries a weight in [0.3, 0.7], vmax > 0
everywhere, no n_prev reaches cap, no row map names a stream row twice, and every named edge position is planted somewhere.

Mutations.  Each one-off mistake below, applied to the reference, moves some element of ctx by more than 10 x that element's bf16
bound on at least one case of EVERY kernel family it covers (the rule of test_reference_mutations_change_a_case in
tests/test_hip_policy_cross_attention.py), so a kernel with that mistake cannot pass the GPU cases.  What each stands for:

  drop_newest / attend_n_prev   the `j == np ? k_new : cache` select of prefetch / prefetch2 / looped / the wave kernel never taken,
                                or `n = np` for `n = np + 1` (self_attn_kernel, self_attn_wave_kernel); both leave keys 0 .. n_prev - 1.
                                Causal: the mask `k0 + 16 n + r > u` written `>=` (exclude_diagonal).
  stale_newest_k / _v           the newest row read from the cache (where an earlier step's or no value lies) instead of qkv: the
                                append to the cache is issued AFTER the loads in every step kernel, so the cache row is stale
  attend_one_more               `n = np + 2`, or `rg + RP i <= n` for `<` in finish3 / the wave kernel; causal: the mask `> u + 1`
  scale_eighth                  a head_dim^-0.5 fixed at the production head dim 64 (wrong at every other d; the wave kernel has no
                                other d, so it is not covered)
  k_head_next                   K taken at head h + 1: `h * d` / `(b * H + h)` offsets of K not matching those of q and V
  drop_pass_first               key RP i of pass i lost: the pass stride of prefetch2 / the wave kernel (`rg + RP * i`) or its guard
                                `i * RP < n` off by one; row-per-lane core: its row limit (attn::row_lane_rows)
  drop_behind_256               `looped` never entered or its `j += 256` stride stopping after one round: keys 256 .. lost
  exclude_diagonal              (causal) see above
  drop_diagonal_tile            (causal) the wave-uniform skip `k0 > w0 + 15` taken one 32-key block early: the strip loses the last
                                block it may see
  no_rescale                    (causal) the running sum not multiplied by exp(m - m') when a later block raises the maximum
"""
import pytest
import torch

import self_attention_ref as R
from oracle import decoder as odec
from test_teacher_forced_oracle import _causal_self_attn

BF16 = torch.bfloat16


# ------------------------------------------------------------------ anchors
def _identity_weights(D, prefix):
    w = {}
    for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
        w[f"{prefix}.{n}.weight"] = torch.eye(D, dtype=torch.float64)
        w[f"{prefix}.{n}.bias"] = torch.zeros(D, dtype=torch.float64)
    return w


class _Cfg:
    def __init__(self, H):
        self.num_heads = H


@pytest.mark.parametrize("d,H", [(8, 3), (24, 1), (64, 4)])
def test_step_reference_equals_oracle_step_by_step(d, H):
    B, steps, D = 3, 9, H * d
    g = torch.Generator().manual_seed(d)
    w, lst = _identity_weights(D, "sa"), {"self_k": None, "self_v": None}
    kc = torch.full((B, H, steps, d), float("nan"), dtype=torch.float64)
    vc = kc.clone()
    for t in range(steps):
        x = torch.randn(1, B, D, generator=g, dtype=torch.float64)
        want = odec._self_attn_step(w, "sa", _Cfg(H), x, lst)[0]                  # identity projections: q = k = v = x
        ref = R.step_reference(x[0].repeat(1, 3), kc, vc, [t] * B)
        torch.testing.assert_close(ref["ctx"].view(B, D), want, atol=1e-6, rtol=1e-6)
        kc, vc = ref["k_cache"], ref["v_cache"]
        assert torch.equal(kc[:, :, :t + 1], lst["self_k"]) and bool(torch.isnan(kc[:, :, t + 1:]).all())
        assert torch.equal(vc[:, :, :t + 1], lst["self_v"]) and bool(torch.isnan(vc[:, :, t + 1:]).all())


@pytest.mark.parametrize("d,H,U", [(8, 3, 33), (40, 1, 17), (64, 2, 65)])
def test_causal_reference_equals_oracle_restatement(d, H, U):
    B, D = 2, H * d
    x = torch.randn(U, B, D, generator=torch.Generator().manual_seed(U), dtype=torch.float64)
    want = _causal_self_attn(_identity_weights(D, "sa"), "sa", _Cfg(H), x)       # [U, B, D]
    ref = R.causal_reference(x.transpose(0, 1).repeat(1, 1, 3), H)
    torch.testing.assert_close(ref["ctx"].reshape(B, U, D), want.transpose(0, 1), atol=1e-6, rtol=1e-6)


@pytest.mark.parametrize("name", ["d8_U33", "d24_U65", "d64_U129", "d40_U17"])
@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_tag)
def test_causal_row_equals_step_reference(name, dtype):
    """row u of the whole-target form is the step form at n_prev = u on the same qkv, vmax included"""
    c = R.CAUSAL_CASES[name]
    d, U, H, D = c["d"], c["U"], c["H"], c["H"] * c["d"]
    qkv = R.causal_inputs(name, dtype)["qkv"]
    ref = R.causal_expected(name, dtype)
    for b in range(c["B"]):
        k, v = [t.view(U, H, d).transpose(0, 1) for t in qkv[b].split(D, dim=-1)[1:]]
        poison = lambda t: torch.cat([t, torch.full_like(t[:, :1], float("nan"))], dim=1)        # noqa: E731
        for u in sorted({0, 1, U // 2, U - 1}):
            kc, vc = poison(k).clone(), poison(v).clone()
            kc[:, u:], vc[:, u:] = float("nan"), float("nan")
            st = R.step_reference(qkv[b, u:u + 1], kc.unsqueeze(0), vc.unsqueeze(0), [u])
            torch.testing.assert_close(st["ctx"][0], ref["ctx"][b, u], atol=1e-12, rtol=1e-12)
            assert torch.equal(st["vmax"][0], ref["vmax"][b, u])


# ------------------------------------------------------------------ fairness of the inputs
@pytest.mark.parametrize("name", list(R.ALL_STEP_CASES))
def test_step_case_preconditions(name):
    c, inp, ref = R.ALL_STEP_CASES[name], R.step_inputs(name), R.step_expected(name)
    assert all(0 <= n < c["cap"] for n in inp["n_prev"]), "n_prev[b] >= cap must never reach the device"
    if c["np_uniform"] >= 0:
        assert all(n == c["np_uniform"] for n in inp["n_prev"]) and c["np_uniform"] < c["cap"]
    live = [b for b in (inp["row_map"] or range(len(inp["n_prev"]))) if b >= 0]
    assert len(set(live)) == len(live)
    ok = ref["live"]
    assert not bool(torch.isnan(ref["ctx"][ok]).any()) and bool((ref["vmax"][ok] > 0).all())
    for b, n0 in enumerate(inp["n_prev"]):                       # what must never be read is NaN
        assert bool(torch.isnan(inp["k_cache"][b, :, n0:].float()).all()) and bool(torch.isnan(inp["v_cache"][b, :, n0:].float()).all())
        assert not bool(torch.isnan(inp["k_cache"][b, :, :n0].float()).any())
    assert inp["planted"] or max(c["ns"]) < 2                    # one key: its weight is 1, nothing to plant
    for i, h, j, label in inp["planted"]:
        assert 0.3 <= float(ref["weights"][i][h][j]) <= 0.7, (name, i, h, j, label, float(ref["weights"][i][h][j]))
    if c["H"] > 1:                                               # and the unplanted head is diffuse
        assert all(float(ref["weights"][i][c["H"] - 1].max()) < 0.95 or len(ref["weights"][i][0]) < 4 for i in range(len(ok)) if ok[i])


@pytest.mark.parametrize("name", list(R.CAUSAL_CASES))
def test_causal_case_preconditions(name):
    for dtype in R.DTYPES:
        inp, ref = R.causal_inputs(name, dtype), R.causal_expected(name, dtype)
        assert not bool(torch.isnan(ref["ctx"]).any()) and bool((ref["vmax"] > 0).all())
        for b, h, u, j, label in inp["planted"]:
            assert 0.3 <= float(ref["weights"][b, h, u, j]) <= 0.7, (name, dtype, b, h, u, j, label, float(ref["weights"][b, h, u, j]))


def _family(name):
    c = R.ALL_STEP_CASES[name]
    if R.uses_wave_kernel(c["d"], c["cap"], c["dtype"]):
        return "wave"
    return "workgroup NP>0" if R.lanes_per_row(c["d"], c["dtype"]) else "workgroup NP=0"


def test_cases_cover_every_launch_form():
    """every NP in both dtypes, the row-per-lane core below and at its limit, looped for NP > 0 and NP = 0, wave <8> and <16>,
    np_uniform, row maps with a skipped slot, every causal head dim -- and every named edge is planted"""
    paths, labels = set(), {}
    for name, c in R.ALL_STEP_CASES.items():
        fam = _family(name)
        for n in c["ns"]:
            paths.add((R.dtype_tag(c["dtype"]), "wave" if fam == "wave" else R.workgroup_path(c["d"], c["dtype"], n)))
        labels.setdefault(fam, set()).update(label for *_, label in R.step_inputs(name)["planted"])
    for t, nps in (("fp32", (2, 4, 8, 16)), ("bf16", (2, 4, 8))):
        for np_ in nps:
            assert (t, f"workgroup NP={np_}") in paths and (t, f"looped NP={np_}") in paths, (t, np_)
        assert (t, "workgroup NP=0 row-per-lane") in paths and (t, "looped NP=0") in paths
    assert ("bf16", "wave") in paths
    for d in (24, 40, 48, 56):
        lim = R.row_lane_rows(d)
        assert any(c["d"] == d and {lim - 1, lim, lim + 1} <= set(c["ns"]) for c in R.STEP_CASES.values())
    for fam in ("wave", "workgroup NP>0"):
        assert {"key0", "newest", "pass_first", "pass_last"} <= labels[fam], (fam, labels[fam])
    assert {"key255", "key256"} <= labels["workgroup NP>0"] and {"key0", "newest", "key255", "key256"} <= labels["workgroup NP=0"]
    assert {"key63", "key64"} <= labels["wave"]
    uni = {c["np_uniform"] for n, c in R.ROWS_CASES.items() if "wave" in n}
    assert uni == {-1, 0, 7, 8, 62, 63, 64, 127}
    assert any(c["row_map"] and min(c["row_map"]) < 0 and c["np_uniform"] < 0 for c in R.ROWS_CASES.values())
    assert any(c["row_map"] and min(c["row_map"]) < 0 and c["np_uniform"] >= 0 for c in R.ROWS_CASES.values())
    assert any(c["row_map"] and len(c["row_map"]) < len(c["ns"]) for c in R.ROWS_CASES.values())
    assert any(c["H"] * len(c["ns"]) % 4 for n, c in R.STEP_CASES.items() if "wave" in n)
    assert all(len(c["ns"]) <= 8 and c["H"] in (1, 3, 4) for c in R.ALL_STEP_CASES.values())
    assert {c["d"] for c in R.CAUSAL_CASES.values()} == set(R.CAUSAL_DIMS) and {c["U"] for c in R.CAUSAL_CASES.values()} == set(R.CAUSAL_U)
    assert {(c["H"], c["B"]) for c in R.CAUSAL_CASES.values()} == {(1, 1), (3, 1), (1, 2), (3, 2)}
    clabels = {label for name in R.CAUSAL_CASES for *_, label in R.causal_inputs(name, BF16)["planted"]}
    assert clabels == {"diagonal", "tile_first", "tile_half", "key0", "strip_first_diagonal"}


# ------------------------------------------------------------------ the cases can fail
def _moved(ref, mut, c_bf16):
    ok = ~torch.isnan(ref["ctx"])
    bound = c_bf16 * R.EPS_BF16 * torch.maximum(ref["vmax"][ok], mut["vmax"][ok])
    return bool(((mut["ctx"][ok] - ref["ctx"][ok]).abs() > 10 * bound).any())


def _drop_pass_first(c):
    return ("drop_keys", lambda n: range(c["rp"], n, c["rp"])) if c["rp"] else ("drop_keys", lambda n: [R.row_lane_rows(c["d"])])


STEP_MUTATION_FAMILIES = {m: ("wave", "workgroup NP>0", "workgroup NP=0") for m in R.STEP_MUTATIONS}
STEP_MUTATION_FAMILIES["scale_eighth"] = ("workgroup NP>0", "workgroup NP=0")          # the wave kernel has d = 64 only
STEP_MUTATION_FAMILIES["drop_pass_first"] = ("wave", "workgroup NP>0", "workgroup NP=0")
STEP_MUTATION_FAMILIES["drop_behind_256"] = ("workgroup NP>0", "workgroup NP=0")       # looped: the wave kernel ends at 128 keys


@pytest.mark.parametrize("mutation", list(STEP_MUTATION_FAMILIES))
def test_step_mutations_change_a_case_of_every_family(mutation):
    hits = {f: [] for f in STEP_MUTATION_FAMILIES[mutation]}
    for name, c in R.ALL_STEP_CASES.items():
        fam = _family(name)
        if fam not in hits or c["dtype"] != BF16:
            continue
        stale = "random" if mutation in ("stale_newest_k", "stale_newest_v", "attend_one_more") else "nan"
        m = {"drop_pass_first": _drop_pass_first(c), "drop_behind_256": ("drop_keys", lambda n: range(256, n))}.get(mutation, mutation)
        if _moved(R.step_ref(name, stale=stale), R.step_ref(name, mutation=m, stale=stale), R.BF16_C_STEP):
            hits[fam].append(name)
    for fam, names in hits.items():
        print(f"step mutation {mutation}, {fam}: {len(names)} cases change")
        assert names, (mutation, fam)


CAUSAL_MUTATION_SET = R.CAUSAL_MUTATIONS + ("drop_diagonal_tile",)


@pytest.mark.parametrize("mutation", CAUSAL_MUTATION_SET)
def test_causal_mutations_change_a_case_of_every_head_dim(mutation):
    """the causal kernel is one family; its column tiles and padding depend on the head dim, so every head dim must catch each"""
    m = ("drop_keys", lambda u: range(R.diagonal_tile(u), R.diagonal_tile(u) + 32)) if mutation == "drop_diagonal_tile" else mutation
    for d in R.CAUSAL_DIMS:
        if d == 64 and mutation == "scale_eighth":
            continue
        hits = []
        for name, c in R.CAUSAL_CASES.items():
            if c["d"] != d or (mutation == "k_head_next" and c["H"] == 1):
                continue
            ref = R.causal_expected(name, BF16)
            if _moved(ref, R.causal_reference(R.causal_inputs(name, BF16)["qkv"], c["H"], mutation=m), R.BF16_C_CAUSAL):
                hits.append(name)
        print(f"causal mutation {mutation}, d = {d}: {len(hits)} cases change")
        assert hits, (mutation, d)
