"""The decoder self-attention kernels against the fp64 reference of tests/self_attention_ref.py, at the edges of their branches:
self_attn_kernel<T, NP> in every instantiation and core (csrc/dec_attn.hip, csrc/attn_core.h: the register core per NP, the
row-per-lane core of NP = 0 below and at its row limit, `looped` for NP > 0 and NP = 0), self_attn_wave_kernel<8> / <16>, the launch
forms of the device loops (np_uniform, row_map: simulst_decoder_self_attention_rows) and causal_self_attn_kernel at every head dim
(csrc/teacher_forced.hip).  The reference, the cases and the proof that they can fail live in tests/self_attention_ref.py and
tests/test_self_attention_ref_cpu.py.

Asserted for every case and launch form.
  caches   each cache equals the expected cache bit for bit over the WHOLE buffer, SENTINEL guard rows before and behind it included:
           row n_prev is this step's k / v, the rows behind it are still NaN (they were never to be read: a read shows as NaN in ctx),
           the caches of unmapped stream rows are unchanged.
  writes   ctx (prefilled with SENTINEL, guard rows around it) is written at exactly the live slots; no NaN in a live row.
  bounds   per (row, head, channel), vmax = max_j |v_j[c]| over the attended keys:
           fp32: atol 2e-5, rtol 1e-4 (the project's fp32 attention bound).
           bf16, step kernels (workgroup and wave): the operands are exact in the reference; scores, softmax and P.V are fp32 and P is
           NOT rounded, so the one rounding is the store: the stored x is a convex combination of the attended values, |x| <= vmax, a
           bf16 rounding errs by at most 2^-9 of the top of x's binade <= 2 * 2^-9 |x|  ->  |got - ref| <= 2 * 2^-9 vmax.
           bf16, causal kernel: P is additionally rounded to bf16 for the second product (<= 2^-9 relative each) while the normaliser
           sums the unrounded exponentials, which adds at most 2^-9 sum_j p_j |v_j| / sum_j p_j <= 2^-9 vmax  ->  3 * 2^-9 vmax.
           The fp32 terms are left out of both (tests/test_hip_policy_cross_attention.py argues why).  The constants are derived,
           not measured; the module prints the worst |got - ref| / bound per path, and DESIGN.md records them.
  agreement  the wave kernel and the workgroup kernel (SIMULST_OPT_VALU_ATTENTION) on the same inputs EACH meet the reference and
           leave bit-identical caches; row u of the causal kernel and the step kernel at n_prev = u each meet the same reference.  No
           tolerance between two GPU results stands in for either comparison.

n_prev[b] >= cap is never placed in a device array (the kernels do not check it and would write out of bounds); the host-side
refusals are tested through their status codes, with nothing launched.

Found by these cases and fixed: causal_self_attn_kernel multiplied q by head_dim^-0.5 BEFORE rounding it to the activation dtype as
the A operand of the first product.  That rounding is exact only for a power-of-two scale (d = 16, 64 -- the head dims the suite
had); at d = 8, 24, 32, 40, 48, 56 the bf16 kernel carried a second rounding of q (2^-9 relative per element, so ~2^-9 |score| on a
score, which a peaked softmax turns into a weight error far above the store's) and exceeded the 3 * 2^-9 bound: worst ratios before
the fix are in DESIGN.md.  The kernel now stages q as given and scales the fp32 scores after the first product; for d = 16 and 64
the scale is a power of two, which commutes with every rounding involved, so those head dims keep their bits.
"""
import ctypes

import pytest
import torch

import self_attention_ref as R
from self_attention_ref import SENTINEL

BF16 = torch.bfloat16
GUARD = 2                               # guard rows (of a whole stream row / ctx row) before and behind every output buffer


@pytest.fixture(scope="module")
def ops():
    from simulst_amd.ops import Ops
    return Ops()


@pytest.fixture(scope="module")
def worst():
    """worst |got - ref| / bound of the bf16 results per kernel path"""
    w = {}
    yield w
    for k, (r, name) in sorted(w.items()):
        print(f"\nself-attention, worst bf16 |got - ref| / bound over all cases: {k}: {r:.3f} ({name})")


def _note(worst, key, value, name):
    if value > worst.get(key, (-1.0, ""))[0]:
        worst[key] = (value, name)


def _guarded(t):
    """a device copy of t with GUARD sentinel rows (of t[0]'s shape) before and behind it -> (whole buffer, the view to hand out)"""
    whole = torch.full((t.shape[0] + 2 * GUARD,) + tuple(t.shape[1:]), SENTINEL, dtype=t.dtype).cuda()
    whole[GUARD:-GUARD] = t.cuda()
    return whole, whole[GUARD:-GUARD]


def _same_bits(a, b):
    """bit-for-bit equality, NaNs included"""
    view = torch.int16 if a.dtype == BF16 else torch.int32
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def _expected_whole(t):
    whole = torch.full((t.shape[0] + 2 * GUARD,) + tuple(t.shape[1:]), SENTINEL, dtype=t.dtype)
    whole[GUARD:-GUARD] = t
    return whole


def _run_step(ops, name, *, entry, valu=False):
    """one launch of a step case -> (ctx [slots, H, d] on the CPU, k_cache, v_cache whole buffers on the CPU); asserts what holds for
    every launch form: the caches bit for bit, ctx written at exactly the live slots"""
    from simulst_amd import _lib
    c, inp, ref = R.ALL_STEP_CASES[name], R.step_inputs(name), R.step_expected(name)
    H, d, cap, dtype = c["H"], c["d"], c["cap"], c["dtype"]
    slots = inp["qkv"].shape[0]
    assert all(0 <= n < cap for n in inp["n_prev"])               # never an out-of-range position on the device
    kc_w, kc = _guarded(inp["k_cache"])
    vc_w, vc = _guarded(inp["v_cache"])
    ctx_w, ctx = _guarded(torch.full((slots, H * d), SENTINEL, dtype=dtype))
    qkv = inp["qkv"].cuda()
    n_prev = torch.tensor(inp["n_prev"], dtype=torch.int32).cuda()
    row_map = None if inp["row_map"] is None else torch.tensor(inp["row_map"], dtype=torch.int32).cuda()
    try:
        ops.h.set_option(_lib.OPT_VALU_ATTENTION, int(valu))
        if entry == "plain":
            assert row_map is None and c["np_uniform"] < 0
            ops.decoder_self_attention(qkv, kc, vc, n_prev, out=ctx)
        else:
            # lockstep rows: the position is host-known and n_prev[] may be NULL
            ops.decoder_self_attention_rows(qkv, kc, vc, None if c["np_uniform"] >= 0 else n_prev, np_uniform=c["np_uniform"],
                                            row_map=row_map, out=ctx)
        torch.cuda.synchronize()
    finally:
        ops.h.set_option(_lib.OPT_VALU_ATTENTION, 0)
    kc_w, vc_w, ctx_w = kc_w.cpu(), vc_w.cpu(), ctx_w.cpu()
    assert _same_bits(kc_w, _expected_whole(ref["k_cache"])), (name, entry, valu, "k_cache differs from the expected cache")
    assert _same_bits(vc_w, _expected_whole(ref["v_cache"])), (name, entry, valu, "v_cache differs from the expected cache")
    got = ctx_w[GUARD:-GUARD].view(slots, H, d)
    live = ref["live"]
    assert bool((ctx_w[:GUARD] == SENTINEL).all()) and bool((ctx_w[-GUARD:] == SENTINEL).all()), (name, "ctx written outside its rows")
    assert bool((got[~live] == SENTINEL).all()), (name, "a skipped slot's ctx row was written")
    assert not bool(torch.isnan(got[live].float()).any()), (name, entry, valu, "NaN in ctx: a row at or behind n_prev was read")
    assert not bool((got[live] == SENTINEL).all(dim=-1).any()), (name, "a live ctx row was not written")
    return got, kc_w, vc_w


def _check_step_ctx(name, way, got, worst, wave):
    c, ref = R.ALL_STEP_CASES[name], R.step_expected(name)
    dtype, rows = c["dtype"], (R.step_inputs(name)["row_map"] or range(len(c["ns"])))
    for i, b in enumerate(rows):
        if b < 0:
            continue
        n = c["ns"][b]
        path = (f"wave <{8 if 0 <= c['np_uniform'] < 64 else 16}>" if wave else R.workgroup_path(c["d"], dtype, n))
        ratio = R.bound_ratio(got[i], ref["ctx"][i], ref["vmax"][i], R.BF16_C_STEP)
        print(f"{name}: {way}, slot {i} (stream row {b}, {n} keys) [{path}] {R.dtype_tag(dtype)}: max |got - ref| = "
              f"{float((got[i].double() - ref['ctx'][i]).abs().max()):.3e}, / bf16 bound = {ratio:.3f}")
        if dtype == torch.float32:
            torch.testing.assert_close(got[i].double(), ref["ctx"][i], atol=2e-5, rtol=1e-4, msg=lambda m: f"{name}: {way}, slot {i} [{path}]: {m}")
        else:
            _note(worst, f"step, {path}", ratio, f"{name} slot {i}")
            assert ratio <= 1.0, (name, way, i, path, ratio)


# ------------------------------------------------------------------ the step kernels through simulst_decoder_self_attention
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(R.STEP_CASES))
def test_step_kernels_vs_fp64(ops, worst, name):
    c = R.STEP_CASES[name]
    wave = R.uses_wave_kernel(c["d"], c["cap"], c["dtype"])
    got, kc, vc = _run_step(ops, name, entry="plain")
    _check_step_ctx(name, "wave kernel" if wave else "workgroup kernel", got, worst, wave)
    if wave:                                                     # the same inputs on the workgroup kernel: each meets the reference
        got_b, kc_b, vc_b = _run_step(ops, name, entry="plain", valu=True)
        _check_step_ctx(name, "workgroup kernel (VALU_ATTENTION)", got_b, worst, False)
        assert _same_bits(kc, kc_b) and _same_bits(vc, vc_b), (name, "the two kernels leave different caches")


# ------------------------------------------------------------------ the launch forms of the device loops
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(R.ROWS_CASES))
def test_rows_entry_point_vs_fp64(ops, worst, name):
    c = R.ROWS_CASES[name]
    wave = R.uses_wave_kernel(c["d"], c["cap"], c["dtype"])
    got, kc, vc = _run_step(ops, name, entry="rows")
    _check_step_ctx(name, "rows entry, " + ("wave kernel" if wave else "workgroup kernel"), got, worst, wave)
    if wave:
        got_b, kc_b, vc_b = _run_step(ops, name, entry="rows", valu=True)
        _check_step_ctx(name, "rows entry, workgroup kernel (VALU_ATTENTION)", got_b, worst, False)
        assert _same_bits(kc, kc_b) and _same_bits(vc, vc_b), (name, "the two kernels leave different caches")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bf16_d64_wave16_cap128", "fp32_d24_NP0_rowlane_cap300"])
def test_plain_entry_is_the_rows_entry(ops, name):
    """simulst_decoder_self_attention is simulst_decoder_self_attention_rows with np_uniform = -1 and no row map: same bits"""
    a, b = _run_step(ops, name, entry="plain"), _run_step(ops, name, entry="rows")
    assert all(_same_bits(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------ the causal kernel
def _check_causal(name, dtype, got, worst):
    c, ref = R.CAUSAL_CASES[name], R.causal_expected(name, dtype)
    ratio = R.bound_ratio(got, ref["ctx"], ref["vmax"], R.BF16_C_CAUSAL)
    print(f"causal {name} {R.dtype_tag(dtype)}: max |got - ref| = {float((got.double() - ref['ctx']).abs().max()):.3e}, / bf16 bound = {ratio:.3f}")
    assert not bool(torch.isnan(got.float()).any())
    if dtype == torch.float32:
        torch.testing.assert_close(got.double(), ref["ctx"], atol=2e-5, rtol=1e-4, msg=lambda m: f"causal {name}: {m}")
    else:
        _note(worst, f"causal, d = {c['d']:2d}", ratio, name)
        assert ratio <= 1.0, (name, ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(R.CAUSAL_CASES))
def test_causal_kernel_vs_fp64(ops, worst, name):
    c = R.CAUSAL_CASES[name]
    B, U, H, d = c["B"], c["U"], c["H"], c["d"]
    for dtype in R.DTYPES:
        qkv = R.causal_inputs(name, dtype)["qkv"]
        ctx_w, ctx = _guarded(torch.full((B, U, H * d), SENTINEL, dtype=dtype))
        ops.decoder_self_attention_causal(qkv.cuda(), H=H, out=ctx)
        torch.cuda.synchronize()
        ctx_w = ctx_w.cpu()
        assert bool((ctx_w[:GUARD] == SENTINEL).all()) and bool((ctx_w[-GUARD:] == SENTINEL).all()), (name, "ctx written outside its rows")
        _check_causal(name, dtype, ctx_w[GUARD:-GUARD].view(B, U, H, d), worst)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["d8_U65", "d24_U65", "d32_U65", "d64_U65", "d48_U129"])
@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_tag)
def test_causal_rows_and_step_kernel_meet_one_reference(ops, worst, name, dtype):
    """row u of the causal kernel and the step kernel at n_prev = u, on the same qkv, each within ITS bound of the same reference row
    (tests/test_self_attention_ref_cpu.py shows the two forms of the reference coincide)"""
    c, ref = R.CAUSAL_CASES[name], R.causal_expected(name, dtype)
    U, H, d = c["U"], c["H"], c["d"]
    D = H * d
    qkv = R.causal_inputs(name, dtype)["qkv"][:1]                                   # utterance 0
    us = sorted({0, 1, 15, 16, 31, 32, 63, U - 1})                                  # <= 8 step rows
    got_c = ops.decoder_self_attention_causal(qkv.cuda(), H=H).cpu().view(U, H, d)
    k, v = [t.view(U, H, d).transpose(0, 1) for t in qkv[0].split(D, dim=-1)[1:]]   # [H, U, d]
    kc, vc = k.unsqueeze(0).repeat(len(us), 1, 1, 1), v.unsqueeze(0).repeat(len(us), 1, 1, 1)
    for i, u in enumerate(us):
        kc[i, :, u:], vc[i, :, u:] = float("nan"), float("nan")
    kc_d, vc_d = kc.cuda(), vc.cuda()
    got_s = ops.decoder_self_attention(qkv[0, us].contiguous().cuda(), kc_d, vc_d, torch.tensor(us, dtype=torch.int32).cuda()).cpu().view(len(us), H, d)
    for i, u in enumerate(us):
        assert _same_bits(kc_d[i, :, u].cpu(), k[:, u].contiguous()) and _same_bits(vc_d[i, :, u].cpu(), v[:, u].contiguous())
        for way, got, cst in (("causal", got_c[u], R.BF16_C_CAUSAL), ("step", got_s[i], R.BF16_C_STEP)):
            ratio = R.bound_ratio(got, ref["ctx"][0, u], ref["vmax"][0, u], cst)
            print(f"{name} {R.dtype_tag(dtype)} u = {u}: {way} / its bf16 bound = {ratio:.3f}")
            if dtype == torch.float32:
                torch.testing.assert_close(got.double(), ref["ctx"][0, u], atol=2e-5, rtol=1e-4)
            else:
                assert ratio <= 1.0, (name, u, way, ratio)


# ------------------------------------------------------------------ refusals: status codes only, nothing is launched
def test_refusals_by_status_code():
    """np_uniform >= cap, head dims that are no multiple of 8 or exceed 64, a capacity whose scores do not fit LDS, NULL n_prev without
    np_uniform: refused on the host before any launch (the pointers below are never dereferenced; runs without a device)"""
    from simulst_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.simulst_create(ctypes.byref(h), None) == 0
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    E_NULL, E_SHAPE = -1, lib.simulst_decoder_self_attention_rows(h, p, p, p, p, 128, None, p, 4, 4, 64, 128, _lib.BF16)
    assert E_SHAPE not in (0, E_NULL) and b"capacity exceeded" in lib.simulst_last_error(h)
    rows = lambda n_prev, npu, H, d, cap, dtype=_lib.BF16: lib.simulst_decoder_self_attention_rows(h, p, p, p, n_prev, npu, None, p, 4, H, d, cap, dtype)   # noqa: E731
    assert rows(p, 129, 4, 64, 128) == E_SHAPE and rows(None, 300, 4, 32, 260, _lib.F32) == E_SHAPE
    for d in (12, 4, 72, 0):
        assert rows(p, -1, 4, d, 128) == E_SHAPE and b"head_dim" in lib.simulst_last_error(h), d
        assert lib.simulst_decoder_self_attention(h, p, p, p, p, p, 4, 4, d, 128, _lib.F32) == E_SHAPE, d
    lds_cap = 64 * 1024 // 4 - 64 - 2056                         # the largest capacity whose fp32 scores fit beside the scratch
    assert rows(p, lds_cap, 4, 64, lds_cap + 1) == E_SHAPE and b"LDS" in lib.simulst_last_error(h)
    assert rows(None, -1, 4, 64, 128) == E_NULL and b"null pointer" in lib.simulst_last_error(h)
    assert lib.simulst_decoder_self_attention(h, p, p, p, None, p, 4, 4, 64, 128, _lib.BF16) == E_NULL
    assert rows(None, -5, 4, 64, 128) == E_NULL
    assert lib.simulst_decoder_self_attention_rows(None, p, p, p, p, -1, None, p, 4, 4, 64, 128, _lib.BF16) == E_NULL
    assert rows(p, 0, 4, 64, 128, 7) not in (0, E_NULL, E_SHAPE)            # dtype
    assert lib.simulst_destroy(h) == 0
