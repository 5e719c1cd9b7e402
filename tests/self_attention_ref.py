"""Decoder self-attention: a plain fp64 reference of the operation and the case tables of tests/test_self_attention_ref_cpu.py (which
holds the reference before it is used) and tests/test_hip_self_attention.py (which holds the kernels to it).  CPU only.

The operation (include/simulst_hip.h).  One step, `step_reference`: for slot i (stream row b = row_map[i], or i), head h, the keys and
values are cache rows 0 .. n_prev[b] - 1 of that head followed by this step's k / v from qkv row i; ctx = softmax(q.K^T d^-0.5) V; the
caches afterwards are unchanged except row n_prev[b] of every head, which holds this step's k / v.  The whole target,
`causal_reference`: query u attends keys 0 .. u by the same rule.  Both take tensors already rounded to the activation dtype and
compute in float64; neither restates kernel index arithmetic (no passes, lanes or tiles).  Both return vmax = max_j |v_j[c]| over the
attended keys, the scale of the per-channel bounds.

`mutation=` applies one mistake to the reference (tests/test_self_attention_ref_cpu.py says which kernel branch each stands for).  A
string names a mistake of the operation; the tuple ("drop_keys", f) drops the keys f(n) -> iterable names (step: n attended keys;
causal: f(u) for query u), which is how the CPU tests express "a key at a kernel's internal boundary is lost" without this module
knowing the boundary.  Only "no_rescale" walks keys in blocks: it IS the statement of a blocked running softmax whose sum is not
rescaled when the maximum moves.

Inputs (`step_inputs`, `causal_inputs`): fixed generators, q and v scaled by 1.5 as the policy cases are, rounded to the dtype.  Cache
rows at and behind n_prev[b] are NaN (never to be read; the row at n_prev must be overwritten) -- `stale="random"` leaves the random
draw there instead, for the mutations that read it.  *Planted* (slot, head) pairs: one key at a named edge position is set along q
with the norm that gives it the softmax weight 1/2 against the other attended keys (before its own rounding to the dtype), so a
kernel that loses, doubles or misplaces exactly that key moves ctx by about |v| / 2.  Heads without a plant keep the diffuse softmax
of random draws.
"""
import functools

import torch

SENTINEL = 123.0                       # exact in bf16
DTYPES = (torch.float32, torch.bfloat16)
EPS_BF16 = 2.0 ** -9
BF16_C_STEP, BF16_C_CAUSAL = 2.0, 3.0          # derived in tests/test_hip_self_attention.py
STEP_MUTATIONS = ("drop_newest", "stale_newest_k", "stale_newest_v", "attend_n_prev", "attend_one_more", "scale_eighth", "k_head_next")
CAUSAL_MUTATIONS = ("exclude_diagonal", "attend_one_more", "scale_eighth", "k_head_next", "no_rescale")


def dtype_tag(dtype):
    return "bf16" if dtype == torch.bfloat16 else "fp32"


# ------------------------------------------------------------------ the reference
def _scale(d, mutation):
    return 0.125 if mutation == "scale_eighth" else d ** -0.5


def step_reference(qkv, k_cache, v_cache, n_prev, *, row_map=None, mutation=None):
    """qkv [slots, 3 D], k_cache / v_cache [streams, H, cap, d] (activation dtype or wider), n_prev: ints per stream row, row_map: ints
    per slot or None.  -> dict: ctx, vmax [slots, H, d] float64 (rows of skipped slots: NaN), live [slots] bool, weights[slot][h]
    (softmax weights over the attended keys, in key order), k_cache / v_cache (the expected contents after the call, input dtype)."""
    _, H, cap, d = k_cache.shape
    slots, D = qkv.shape[0], H * d
    assert qkv.shape[1] == 3 * D
    rows = list(range(slots)) if row_map is None else [int(x) for x in row_map]
    live = [b for b in rows if b >= 0]
    assert len(rows) == slots and len(set(live)) == len(live), "a row map never names a stream row twice"
    q, k_new, v_new = [t.double().view(slots, H, d) for t in qkv.split(D, dim=-1)]
    kc, vc = k_cache.double(), v_cache.double()
    out = dict(ctx=torch.full((slots, H, d), float("nan"), dtype=torch.float64), vmax=torch.full((slots, H, d), float("nan"), dtype=torch.float64),
               live=torch.tensor([b >= 0 for b in rows]), weights=[None] * slots, k_cache=k_cache.clone(), v_cache=v_cache.clone())
    for i, b in enumerate(rows):
        if b < 0:
            continue
        n0 = int(n_prev[b])
        assert 0 <= n0 < cap, "n_prev[b] < cap is the caller's contract"
        out["k_cache"][b, :, n0] = qkv[i, D:2 * D].view(H, d)
        out["v_cache"][b, :, n0] = qkv[i, 2 * D:].view(H, d)
        out["weights"][i] = []
        for h in range(H):
            hk = (h + 1) % H if mutation == "k_head_next" else h
            K = torch.cat([kc[b, hk, :n0], k_new[i, hk].unsqueeze(0)])
            V = torch.cat([vc[b, h, :n0], v_new[i, h].unsqueeze(0)])
            if mutation == "stale_newest_k":
                K[n0] = kc[b, hk, n0]
            elif mutation == "stale_newest_v":
                V[n0] = vc[b, h, n0]
            elif mutation in ("drop_newest", "attend_n_prev") and n0 > 0:
                K, V = K[:n0], V[:n0]
            elif mutation == "attend_one_more" and n0 + 1 < cap:
                K, V = torch.cat([K, kc[b, hk, n0 + 1].unsqueeze(0)]), torch.cat([V, vc[b, h, n0 + 1].unsqueeze(0)])
            elif isinstance(mutation, tuple) and mutation[0] == "drop_keys":
                keep = torch.ones(n0 + 1, dtype=torch.bool)
                keep[[j for j in mutation[1](n0 + 1) if 0 <= j <= n0]] = False
                if bool(keep.any()):
                    K, V = K[keep], V[keep]
            w = torch.softmax((K @ q[i, h]) * _scale(d, mutation), dim=0)
            out["ctx"][i, h], out["vmax"][i, h] = w @ V, V.abs().amax(dim=0)
            out["weights"][i].append(w)
    return out


def causal_reference(qkv, H, *, mutation=None):
    """qkv [B, U, 3 D] -> dict: ctx, vmax [B, U, H, d] float64, weights [B, H, U, U] (row u: softmax over keys 0 .. u, 0 behind)"""
    B, U, D3 = qkv.shape
    D = D3 // 3
    d = D // H
    q, k, v = [t.double().view(B, U, H, d).transpose(1, 2) for t in qkv.split(D, dim=-1)]          # [B, H, U, d]
    if mutation == "k_head_next":
        k = torch.roll(k, -1, dims=1)
    u, j = torch.arange(U).view(U, 1), torch.arange(U).view(1, U)
    seen = j <= u
    if mutation == "exclude_diagonal":
        seen = (j < u) | (j == 0)
    elif mutation == "attend_one_more":
        seen = j <= u + 1
    elif isinstance(mutation, tuple) and mutation[0] == "drop_keys":
        for uu in range(U):
            drop = [x for x in mutation[1](uu) if 0 <= x <= uu]
            if len(set(drop)) < uu + 1:
                seen[uu, drop] = False
    s = (q @ k.transpose(-1, -2)) * _scale(d, mutation)
    s = s.masked_fill(~seen, float("-inf"))
    if mutation == "no_rescale":
        m, l, o = torch.full((B, H, U), float("-inf"), dtype=torch.float64), torch.zeros(B, H, U, dtype=torch.float64), torch.zeros_like(q)
        for k0 in range(0, U, 32):
            st = s[..., k0:k0 + 32]
            mt = torch.maximum(m, st.amax(-1))
            p = (st - mt.unsqueeze(-1)).exp()
            l = l + p.sum(-1)                                         # the mistake: l * exp(m - mt) + ...
            o = o * (m - mt).exp().unsqueeze(-1) + p @ v[:, :, k0:k0 + 32]
            m = mt
        ctx, w = o / l.unsqueeze(-1), torch.softmax(s, dim=-1)
    else:
        w = torch.softmax(s, dim=-1)
        ctx = w @ v
    vmax = v.abs().unsqueeze(2).expand(B, H, U, U, d).masked_fill(~seen.view(1, 1, U, U, 1), 0.0).amax(dim=3)
    return dict(ctx=ctx.transpose(1, 2).contiguous(), vmax=vmax.transpose(1, 2).contiguous(), weights=w)


# ------------------------------------------------------------------ which launch form a row takes (dec_attn.hip's dispatch, restated for the ids and the notes only)
def lanes_per_row(d, dtype):
    """attn::lanes_per_row: 16-byte chunks per head row when that is an instantiated power of two, else 0"""
    lpr, rem = divmod(d, 8 if dtype == torch.bfloat16 else 4)
    return lpr if rem == 0 and lpr in (2, 4, 8, 16) else 0


def row_lane_rows(d):
    return 256 // (d // 4) * (d // 4)


def uses_wave_kernel(d, cap, dtype):
    return dtype == torch.bfloat16 and d == 64 and cap <= 128


def workgroup_path(d, dtype, n):
    """the core of self_attn_kernel a row of n keys runs on"""
    np_ = lanes_per_row(d, dtype)
    if np_ > 0 and n <= 256:
        return f"workgroup NP={np_}"
    if np_ == 0 and n <= row_lane_rows(d):
        return "workgroup NP=0 row-per-lane"
    return f"looped NP={np_}"


# ------------------------------------------------------------------ step cases
def _uniq(xs, cap):
    out = []
    for x in xs:
        if 1 <= x <= cap and x not in out:
            out.append(x)
    return out


def _step_case(dtype, d, H, cap, ns, *, rp, edges=(), row_map=None, np_uniform=-1, streams=None):
    """ns: attended keys n = n_prev + 1 per STREAM row; rp: keys per pass of the kernel the case aims at (0: none), which only places
    the plants; edges: further key positions to plant at"""
    ns = list(ns)
    assert len(ns) <= 8 and all(1 <= n <= cap for n in ns) and d % 8 == 0 and d <= 64
    return dict(dtype=dtype, d=d, H=H, cap=cap, ns=ns, rp=rp, edges=tuple(edges), row_map=row_map, np_uniform=np_uniform)


def _build_step_cases():
    cases = {}
    heads = {8: 3, 16: 4, 24: 1, 32: 3, 40: 4, 48: 3, 56: 1, 64: 4}
    for dtype in DTYPES:
        t = dtype_tag(dtype)
        for d in (8, 16, 24, 32, 40, 48, 56, 64):
            np_, H = lanes_per_row(d, dtype), heads[d]
            if np_ > 0:
                rp = 256 // np_
                # every pass boundary of the instantiation, the last keys of the register core, n = cap on the looped core
                cases[f"{t}_d{d}_NP{np_}_cap260"] = _step_case(dtype, d, H, 260, _uniq([1, 2, rp - 1, rp, rp + 1, 255, 256, 260], 260), rp=rp)
                # looped with NP > 0: first looped key range, two full strides and one key (n = cap = 513), a second pass boundary
                cases[f"{t}_d{d}_NP{np_}_looped_cap513"] = _step_case(dtype, d, 4 if H == 3 else 3, 513,
                                                                    _uniq([257, 513, 2 * rp + 1, 512, 256, 3 * rp, 258], 513), rp=rp)
            else:
                R = row_lane_rows(d)
                cases[f"{t}_d{d}_NP0_rowlane_cap300"] = _step_case(dtype, d, H, 300, _uniq([1, 2, 100, R - 1, R, R + 1, 257, 300], 300), rp=0,
                                                                  edges=(R - 1, R))
                cases[f"{t}_d{d}_NP0_looped_cap513"] = _step_case(dtype, d, 4 if H == 3 else 3, 513, _uniq([249, 253, 255, 256, 300, 513], 513),
                                                                 rp=0, edges=(255, 256, 512))
    bf = torch.bfloat16
    # bf16 d = 64 at cap 129: one row too many for the wave kernel, so the workgroup kernel without any option
    cases["bf16_d64_NP8_cap129"] = _step_case(bf, 64, 3, 129, [1, 2, 31, 32, 33, 128, 129], rp=32)
    # the wave kernel (cap <= 128; device n_prev: <16>), B * H odd; every case also runs on the workgroup kernel under the option
    cases["bf16_d64_wave16_cap64"] = _step_case(bf, 64, 3, 64, [1, 2, 7, 8, 9, 63, 64], rp=8)
    cases["bf16_d64_wave16_cap128"] = _step_case(bf, 64, 3, 128, [2, 8, 63, 64, 65, 127, 128], rp=8, edges=(63, 64))
    cases["bf16_d64_wave16_cap128_H1"] = _step_case(bf, 64, 1, 128, [1, 7, 9, 65, 128], rp=8, edges=(63, 64))
    return cases


def _build_rows_cases():
    """the launch forms of simulst_decoder_self_attention_rows: np_uniform (lockstep rows: every row at the same position) and row_map"""
    cases = {}
    bf, f32 = torch.bfloat16, torch.float32
    kernels = (("bf16_d64_wave", bf, 64, 8), ("fp32_d64_NP16", f32, 64, 16), ("bf16_d32_NP4", bf, 32, 64))
    for tag, dtype, d, rp in kernels:
        for npu in (0, 7, 8, 62, 63, 64, 127):
            form = tag if "wave" not in tag else f"{tag}{8 if npu < 64 else 16}"
            cases[f"{form}_uniform{npu}"] = _step_case(dtype, d, 3, 128, [npu + 1] * 5, rp=rp, np_uniform=npu, edges=(63, 64))
        maps = {"permuted": [3, 0, 4, 1, 2], "fewer_slots": [4, 1, 2], "skipped_slot": [2, -1, 0, 4]}
        for mname, rm in maps.items():
            # device-side n_prev: every stream row at its own position; unmapped stream rows must stay as they were
            cases[f"{tag}{16 if 'wave' in tag else ''}_rowmap_{mname}_nprev"] = _step_case(dtype, d, 3, 128, [9, 64, 65, 128, 33], rp=rp, row_map=rm,
                                                                                         edges=(63, 64))
            for npu in (63, 64):
                form = tag if "wave" not in tag else f"{tag}{8 if npu < 64 else 16}"
                cases[f"{form}_rowmap_{mname}_uniform{npu}"] = _step_case(dtype, d, 3, 128, [npu + 1] * 5, rp=rp, row_map=rm, np_uniform=npu,
                                                                        edges=(63, 64))
    return cases


STEP_CASES = _build_step_cases()
ROWS_CASES = _build_rows_cases()
ALL_STEP_CASES = {**STEP_CASES, **ROWS_CASES}


def step_edges(c, n):
    """the named edge positions among keys 0 .. n - 1 of a case: {label: key}"""
    e = {"key0": 0, "newest": n - 1}
    if c["rp"]:
        firsts = [j for j in range(c["rp"], n, c["rp"])]
        if firsts:
            e["pass_first"], e["pass_last"] = firsts[-1], firsts[-1] - 1
            if len(firsts) > 1:
                e["pass_first_1"], e["pass_last_1"] = firsts[0], firsts[0] - 1
    for j in (255, 256) + tuple(c["edges"]):
        if j < n:
            e[f"key{j}"] = j
    return e


def _plant(q, K, j, scale):
    """the key along q whose score equals log sum exp of the other attended scores: weight 1/2.  q [d], K [n, d] float64"""
    others = torch.ones(K.shape[0], dtype=torch.bool)
    others[j] = False
    target = float(torch.logsumexp((K[others] @ q) * scale, dim=0))
    return q * (target / (float(q @ q) * scale))


@functools.lru_cache(maxsize=None)
def step_inputs(name, stale="nan"):
    """-> dict: qkv [slots, 3 D], k_cache / v_cache [streams, H, cap, d] in the case's dtype, n_prev (list per stream row), row_map
    (list or None), planted [(slot, head, key, label)]"""
    c = ALL_STEP_CASES[name]
    dtype, d, H, cap = c["dtype"], c["d"], c["H"], c["cap"]
    streams, D = len(c["ns"]), H * d
    rows = list(range(streams)) if c["row_map"] is None else c["row_map"]
    slots = len(rows)
    g = torch.Generator().manual_seed(9100 + list(ALL_STEP_CASES).index(name))
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dtype).double()      # noqa: E731
    q, k_new, v_new = rnd(slots, H, d, scale=1.5), rnd(slots, H, d), rnd(slots, H, d, scale=1.5)
    kc, vc = rnd(streams, H, cap, d), rnd(streams, H, cap, d, scale=1.5)
    n_prev = [n - 1 for n in c["ns"]]
    planted, turn = [], 0
    for i, b in enumerate(rows):
        if b < 0 or c["ns"][b] < 2:
            continue
        n = c["ns"][b]
        edges = sorted(step_edges(c, n).items())
        for h in range(H if H == 1 else H - 1):                # the last head of a multi-head case keeps its random softmax
            label, j = edges[turn % len(edges)]
            turn += 1
            K = torch.cat([kc[b, h, :n - 1], k_new[i, h].unsqueeze(0)])
            key = _plant(q[i, h], K, j, d ** -0.5).to(dtype).double()
            if j == n - 1:
                k_new[i, h] = key
            else:
                kc[b, h, j] = key
            planted.append((i, h, j, label))
    if stale == "nan":
        for b in range(streams):
            kc[b, :, n_prev[b]:] = float("nan")
            vc[b, :, n_prev[b]:] = float("nan")
    qkv = torch.cat([q.view(slots, D), k_new.view(slots, D), v_new.view(slots, D)], dim=1).to(dtype)
    return dict(qkv=qkv, k_cache=kc.to(dtype), v_cache=vc.to(dtype), n_prev=n_prev, row_map=c["row_map"], planted=planted)


def step_ref(name, mutation=None, stale="nan"):
    inp = step_inputs(name, stale)
    return step_reference(inp["qkv"], inp["k_cache"], inp["v_cache"], inp["n_prev"], row_map=inp["row_map"], mutation=mutation)


@functools.lru_cache(maxsize=None)
def step_expected(name):
    """the unmutated reference of a case, computed once and shared"""
    return step_ref(name)


# ------------------------------------------------------------------ causal cases
CAUSAL_DIMS = (8, 16, 24, 32, 40, 48, 56, 64)
CAUSAL_U = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129)
CAUSAL_CASES = {f"d{d}_U{U}": dict(d=d, U=U, H=(1, 3)[(i + k) % 2], B=(1, 2)[((i + k) // 2) % 2])
                for i, d in enumerate(CAUSAL_DIMS) for k, U in enumerate(CAUSAL_U)}


def diagonal_tile(u):
    """first key of the last 32-key block that holds a key the 16-query strip of u may see (teacher_forced.hip walks keys in
    blocks of 32 and a wave's strip of 16 queries skips the blocks wholly in its future)"""
    return 32 * ((16 * (u // 16) + 15) // 32)


def causal_plants(U):
    """(query, key, label): the diagonal, the first key of the query's 32-key block, key 16 of that block, key 0, the first row of the
    second strip -- distinct queries and distinct keys"""
    want = [(U - 1, U - 1, "diagonal")]
    if U >= 3:
        want.append((U - 2, 32 * ((U - 2) // 32), "tile_first"))
    if U >= 20:
        want.append((U - 3, 32 * ((U - 3) // 32) + 16, "tile_half"))
    if U >= 6:
        want.append((U - 4, 0, "key0"))
    if U >= 24:
        want.append((16, 16, "strip_first_diagonal"))
    out, keys = [], set()
    for u, j, label in want:
        if 0 <= j <= u and j not in keys and u >= 1:
            out.append((u, j, label))
            keys.add(j)
    return out


@functools.lru_cache(maxsize=None)
def causal_inputs(name, dtype):
    """-> dict: qkv [B, U, 3 D] in dtype, planted [(b, h, query, key, label)]"""
    c = CAUSAL_CASES[name]
    d, U, H, B = c["d"], c["U"], c["H"], c["B"]
    D = H * d
    g = torch.Generator().manual_seed(9700 + list(CAUSAL_CASES).index(name))
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dtype).double()      # noqa: E731
    q, k, v = rnd(B, U, H, d, scale=1.5), rnd(B, U, H, d), rnd(B, U, H, d, scale=1.5)
    planted = []
    plants = causal_plants(U)
    for b in range(B):
        for h in range(H if H == 1 else H - 1):
            for _ in range(6):                                   # a planted key is seen by the later planted queries too: sweep until it settles
                for u, j, _label in plants:
                    k[b, j, h] = _plant(q[b, u, h], k[b, :u + 1, h], j, d ** -0.5).to(dtype).double()
            planted += [(b, h, u, j, label) for u, j, label in plants]
    qkv = torch.cat([q.view(B, U, D), k.view(B, U, D), v.view(B, U, D)], dim=-1).to(dtype)
    return dict(qkv=qkv, planted=planted)


@functools.lru_cache(maxsize=None)
def causal_expected(name, dtype):
    return causal_reference(causal_inputs(name, dtype)["qkv"], CAUSAL_CASES[name]["H"])


def bound_ratio(got, ref, vmax, c_bf16):
    """max |got - ref| / (c * 2^-9 * vmax) over the elements, NaN-safe on the rows both leave out"""
    ok = ~torch.isnan(ref)
    err = (got.double()[ok] - ref[ok]).abs()
    return float((err / (c_bf16 * EPS_BF16 * vmax[ok]).clamp_min(1e-300)).max()) if err.numel() else 0.0

