"""simulst_emformer_attention -- the VALU kernel (emformer_attn.hip) and the MFMA kernel (emformer_attn_mfma.hip) -- against a
plain fp64 attention over the kernel's own input, at the edges of both kernels' domains.

The reference never restates the kernels' index arithmetic.  Offline, the key set of every query row is a row of
oracle.emformer.gen_attention_mask (pinned to the reference's own mask by g4_mask) or-ed with the key-padding rule of
oracle.emformer.attention_impl; streaming, it is a Python list [valid memory | rc | valid cached left context | utterance].

Bounds.  fp32: atol 2e-5, rtol 1e-4 (the project's fp32 attention bound).  bf16: the operands are exact in the reference and the
scores are accumulated in fp32, so what differs is the bf16 rounding of P before the second product (MFMA only; <= 2^-9 relative
per probability, numerator and denominator) and the bf16 store (2^-9 relative).  The output is a convex combination of the attended
V values, so per (query row, channel) |got - ref| <= 3 * 2^-9 * max_j |v_j| over the keys j the reference attends; asserted is
4 * 2^-9 * max_j |v_j| (one more 2^-9 for the fp32 exponentials), computed per row from the reference's own key set.
(2^-9 is a bf16 rounding relative to the top of its binade; relative to the value itself the worst case is the unit roundoff
2^-8.  The asserted bound covers that too: the MFMA kernel sums its denominator from the unrounded fp32 probabilities, so its worst
case is 2^-8 for P in the numerator + 2^-8 for the store = 4 * 2^-9; the VALU kernel rounds at the store alone, 2^-8.)
Where the default path is the MFMA kernel its output is also compared with the bf16 VALU kernel's: by those worst cases the two
lie within 2^-8 + 2 * 2^-8 = 6 * 2^-9 of each other, times the same max_j |v_j|.

test_reference_mutations_move_the_output (CPU) shows the cases can fail: one key dropped or admitted moves the reference itself by
more than ten times the bf16 bound.
"""
import math

import pytest
import torch

from oracle.emformer import EncCfg, gen_attention_mask

SENTINEL = 123.0                      # exact in bf16; no softmax output of the random inputs equals it
BF16_BOUND = 4 * 2.0 ** -9
BF16_CROSS_BOUND = 6 * 2.0 ** -9         # bf16 VALU against bf16 MFMA (module docstring)
VARIANTS = ("fp32 VALU", "bf16 VALU", "bf16 default")
MODEL_LENGTHS = [250, 249, 131, 17, 1]


def _case(**kw):
    c = dict(S=16, R=8, Lc=32, M=5, H=4, d=64, T=250, B=5, summary=True, lengths=None, streaming=False)
    c.update(kw)
    if c["lengths"] is None and not c["streaming"]:
        T, S, B = c["T"], c["S"], c["B"]
        # whole, one short, a segment boundary + 1, a segment boundary, mid-segment, ..., 1
        pool = [T, T - 1, (T - 1) // S * S + 1, (T - 1) // S * S, S + 1, S, 1]
        c["lengths"] = MODEL_LENGTHS if (T, B) == (250, 5) else [min(max(x, 1), T) for x in (pool[:B - 1] + [1])[:B]]
    return c


OFFLINE = {
    "model": _case(),
    "M8_nk64": _case(M=8),
    "M9_nk65": _case(M=9),
    "R15_M1_nq32": _case(R=15, M=1),
    "R16_M0_nosum": _case(R=16, M=0, summary=False),
    "R17_M0_nosum_nq33": _case(R=17, M=0, summary=False),
    "nosum_nomem": _case(M=0, summary=False),
    "Lc0": _case(Lc=0),
    "M1": _case(M=1),
    "R0": _case(R=0),
    "T37": _case(T=37),
    "T5": _case(T=5, lengths=[5, 4, 3, 2, 1]),
    "T1": _case(T=1),
    "boundary_lengths": _case(T=48, lengths=[48, 33, 32, 1, 0]),
    "H1": _case(H=1),
    "H3": _case(H=3),
    "H8": _case(H=8),
    "B3_T48_grid9": _case(B=3, T=48, lengths=[48, 33, 17]),
    "B1_T48_grid3": _case(B=1, T=48, lengths=[41]),
    "B7_T37_grid21": _case(B=7, T=37),
    "d16_H2": _case(d=16, H=2),
    "d32_H2": _case(d=32, H=2),
    "d40_H2": _case(d=40, H=2),
}
STREAMING = {
    "stream_T16": _case(streaming=True, T=16, lc_valid=[32, 16, 0, 5, 32], n_mem_valid=[5, 2, 0, 1, 3]),
    "stream_T11": _case(streaming=True, T=11, lc_valid=[32, 16, 0, 5, 32], n_mem_valid=[5, 2, 0, 1, 3]),
    "stream_T1": _case(streaming=True, T=1, lc_valid=[32, 16, 0, 5, 32], n_mem_valid=[5, 2, 0, 1, 3]),
    "stream_T11_empty_state": _case(streaming=True, T=11, lc_valid=[0] * 5, n_mem_valid=[0] * 5),
}
CASES = {**OFFLINE, **STREAMING}

OFFLINE_MUTATIONS = ("lc_short", "lc_long", "mem_shift", "sum_sees_mem", "pad_plus_one", "rc_next_block")
STREAMING_MUTATIONS = ("lc_short", "lc_long", "mem_shift", "sum_sees_mem")      # lc_short: the last lc_valid - 1 cached rows


def layout(c):
    """Row counts of QKV [memory | rc | utterance | summaries] and CTX [rc | utterance | summaries], and the descriptor."""
    S = max(c["S"], c["T"]) if c["streaming"] else c["S"]       # streaming: as encoder.py passes it
    N = 1 if c["streaming"] else math.ceil(c["T"] / S)
    n_mem = (c["M"] if c["streaming"] else N - 1) if c["summary"] else 0
    n_sum = N if c["summary"] else 0
    D = c["d"] * c["H"]
    return dict(S=S, N=N, n_mem=n_mem, n_rc=N * c["R"], n_sum=n_sum, D=D,
                rows_z=n_mem + N * c["R"] + c["T"] + n_sum, rows_c=N * c["R"] + c["T"] + n_sum)


def mfma_eligible(c, dtype):
    """The dispatch rule of simulst_emformer_attention, restated."""
    S, u = layout(c)["S"], int(c["summary"])
    return (dtype == torch.bfloat16 and c["d"] == 64 and c["R"] + S + u <= 32
            and c["M"] * u + c["R"] + c["Lc"] + S <= 64)


def kernel_class(c, dtype):
    if mfma_eligible(c, dtype):
        return "MFMA"
    nk_max = c["M"] * int(c["summary"]) + c["R"] + c["Lc"] + layout(c)["S"]
    return "VALU KPL=%d" % (1 if nk_max <= 64 else 2)


def make_inputs(c, seed):
    """fp32 draws (randn * 1.5: the softmax is not flat); a variant rounds them to its dtype."""
    g = torch.Generator().manual_seed(seed)
    lay = layout(c)
    inp = {"QKV": torch.randn(c["B"], lay["rows_z"], 3 * lay["D"], generator=g) * 1.5}
    if c["streaming"]:
        inp["lc_k"] = torch.randn(c["B"], c["Lc"], lay["D"], generator=g) * 1.5
        inp["lc_v"] = torch.randn(c["B"], c["Lc"], lay["D"], generator=g) * 1.5
    return inp


def _attend(q, k, v, allow, H):
    """softmax(q d^-0.5 k^T + mask) v per head in fp64 -> (out [nq, D], max_j |v_j| over the attended keys [nq, D])."""
    nq, D = q.shape
    d = D // H
    assert bool(allow.any(dim=1).all()), "a query row with every key masked"
    qh = q.view(nq, H, d).transpose(0, 1) * d ** -0.5
    kh = k.view(-1, H, d).transpose(0, 1)
    vh = v.view(-1, H, d).transpose(0, 1)
    s = (qh @ kh.transpose(1, 2)).masked_fill(~allow.unsqueeze(0), float("-inf"))
    out = (torch.softmax(s, dim=-1) @ vh).transpose(0, 1).reshape(nq, D)
    pats, inv = torch.unique(allow, dim=0, return_inverse=True)
    va = v.abs()
    vmax = torch.stack([va[p].amax(dim=0) for p in pats])[inv]
    return out, vmax


def _offline_mask(c, lay, mutation):
    """[rows_c, n_mem + n_rc + T], True = masked: the oracle's mask, then at most one mutation of it."""
    Lc = c["Lc"] + {"lc_short": -1, "lc_long": 1}.get(mutation, 0)
    cfg = EncCfg(embed_dim=lay["D"], num_heads=c["H"], segment_length=c["S"], left_context=Lc, right_context=c["R"],
                 max_memory_size=c["M"] if c["summary"] else 0)
    mask = gen_attention_mask(c["T"], cfg)
    n_mem, n_rc, N, R = lay["n_mem"], lay["n_rc"], lay["N"], c["R"]
    assert mask.shape == (lay["rows_c"], n_mem + n_rc + c["T"])
    if mutation == "mem_shift":            # segment i takes the window of segment i - 1
        assert n_mem > 1
        mem = mask[:, :n_mem].clone()
        mask[:, :n_mem - 1] = mem[:, 1:]
        mask[:, n_mem - 1] = True
    elif mutation == "sum_sees_mem":       # summary i sees what the first utterance row of segment i sees
        for i in range(N):
            mask[n_rc + c["T"] + i, :n_mem] = mask[n_rc + i * c["S"], :n_mem]
    elif mutation == "rc_next_block":      # segment i reads the rc block of segment i + 1 (the last one wraps)
        mask[:, n_mem:n_mem + n_rc] = torch.roll(mask[:, n_mem:n_mem + n_rc], R, dims=1)
    return mask


def reference(c, inp, dtype, mutation=None):
    """-> (ref [B, rows_c, D] fp64, max_j |v_j| [B, rows_c, D], written [B, rows_c] bool).  Rows of segments the kernel must
    leave alone (t0 >= len_b) are not computed: ref is NaN and written False there."""
    lay = layout(c)
    B, T, D, H, R, S = c["B"], c["T"], lay["D"], c["H"], c["R"], lay["S"]
    n_mem, n_rc = lay["n_mem"], lay["n_rc"]
    Z = inp["QKV"].to(dtype).double()                       # rounded to the test dtype first: the operands are exact
    ref = torch.full((B, lay["rows_c"], D), float("nan"), dtype=torch.float64)
    vmax = torch.zeros_like(ref)
    written = torch.zeros(B, lay["rows_c"], dtype=torch.bool)
    if not c["streaming"]:
        mask = _offline_mask(c, lay, mutation)
        row_seg = torch.cat([torch.arange(lay["N"]).repeat_interleave(R), torch.arange(T) // S]
                            + ([torch.arange(lay["N"])] if c["summary"] else []))
        for b in range(B):
            n = c["lengths"][b] + (1 if mutation == "pad_plus_one" else 0)
            pad = torch.cat([torch.zeros(n_mem + n_rc, dtype=torch.bool), torch.arange(T) >= n])   # attention_impl's key padding
            rows = (row_seg * S < c["lengths"][b]).nonzero().flatten()
            if rows.numel() == 0:
                continue
            allow = ~(mask | pad.unsqueeze(0))[rows]
            o, vm = _attend(Z[b, n_mem:, :D][rows], Z[b, :n_mem + n_rc + T, D:2 * D], Z[b, :n_mem + n_rc + T, 2 * D:], allow, H)
            ref[b, rows], vmax[b, rows], written[b, rows] = o, vm, True
        return ref, vmax, written
    lc_k, lc_v = inp["lc_k"].to(dtype).double(), inp["lc_v"].to(dtype).double()
    for b in range(B):
        nv, lv = c["n_mem_valid"][b], c["lc_valid"][b]
        mem_rows = list(range(n_mem - nv, n_mem))
        if mutation == "lc_short":
            lv = max(lv - 1, 0)
        elif mutation == "lc_long":
            lv = min(lv + 1, c["Lc"])
        elif mutation == "mem_shift" and 0 < nv < n_mem:
            mem_rows = [r - 1 for r in mem_rows]
        lc_rows = list(range(c["Lc"] - lv, c["Lc"]))
        z_rows = mem_rows + list(range(n_mem, n_mem + R))
        u_rows = list(range(n_mem + R, n_mem + R + T))
        k = torch.cat([Z[b, z_rows, D:2 * D], lc_k[b, lc_rows], Z[b, u_rows, D:2 * D]])
        v = torch.cat([Z[b, z_rows, 2 * D:], lc_v[b, lc_rows], Z[b, u_rows, 2 * D:]])
        allow = torch.ones(lay["rows_c"], k.size(0), dtype=torch.bool)
        if c["summary"] and mutation != "sum_sees_mem":
            allow[-1, :nv] = False                           # the summary query does not see the memory keys
        ref[b], vmax[b] = _attend(Z[b, n_mem:, :D], k, v, allow, H)
        written[b] = True
    return ref, vmax, written


# ------------------------------------------------------------------ CPU: the cases can fail
@pytest.mark.parametrize("name", ["model", "stream_T11"])
def test_reference_mutations_move_the_output(name):
    """One key dropped, admitted or swapped (each mutation on its own) moves at least one element of the fp64 reference by more
    than 10 x that element's bf16 bound: a kernel with that mistake cannot pass the GPU cases.  A statement about the inputs."""
    c = CASES[name]
    inp = make_inputs(c, seed=_seed(name))
    ref, vmax, written = reference(c, inp, torch.bfloat16)
    assert bool(written.any()) and float(ref[written].abs().max()) > 0.1
    for mutation in (STREAMING_MUTATIONS if c["streaming"] else OFFLINE_MUTATIONS):
        mut, _, w2 = reference(c, inp, torch.bfloat16, mutation)
        assert torch.equal(w2, written)
        ratio = ((mut - ref).abs() / (BF16_BOUND * vmax))[written]
        print(f"{name}: {mutation}: max |mutated - ref| / bound = {float(ratio.max()):.1f}, "
              f"{int((ratio > 10).sum())} elements above 10")
        assert float(ratio.max()) > 10, (name, mutation, float(ratio.max()))


def test_eligibility_classes_of_the_cases():
    """The cases reach all three kernels: MFMA (at its nq = 32 and nk = 64 limits too) and both VALU instantiations."""
    bf = torch.bfloat16
    assert {kernel_class(c, bf) for c in CASES.values()} == {"MFMA", "VALU KPL=1", "VALU KPL=2"}
    assert {kernel_class(c, torch.float32) for c in CASES.values()} == {"VALU KPL=1", "VALU KPL=2"}
    for name in ("model", "M8_nk64", "R15_M1_nq32", "H3", "H8", "B3_T48_grid9", "B1_T48_grid3", "B7_T37_grid21", "stream_T11"):
        assert mfma_eligible(CASES[name], bf), name
    for name in ("M9_nk65", "R17_M0_nosum_nq33", "d16_H2", "d32_H2", "d40_H2"):
        assert not mfma_eligible(CASES[name], bf), name
    assert kernel_class(CASES["M9_nk65"], bf) == "VALU KPL=2"


def _seed(name):
    return 4100 + list(CASES).index(name)


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ops():
    from simulst_amd.ops import Ops
    return Ops()


@pytest.fixture(scope="module")
def worst():
    """worst |got - ref| / bound per variant over the module's cases, printed once at the end"""
    w = {}
    yield w
    for k, (r, name) in sorted(w.items()):
        print(f"\nemformer attention, worst |got - ref| / bound over all cases: {k}: {r:.3f} ({name})")


def _run(ops, c, inp, dtype, force_valu):
    from simulst_amd import _lib
    lay = layout(c)
    dev = lambda t: t.to(dtype).cuda()       # noqa: E731
    kw = dict(B=c["B"], T=c["T"], D=lay["D"], H=c["H"], S=lay["S"], R=c["R"], Lc=c["Lc"], M=c["M"], n_mem=lay["n_mem"],
              n_seg=lay["N"], use_summary=c["summary"])
    lengths = None
    if c["streaming"]:
        kw.update(lc_k=dev(inp["lc_k"]), lc_v=dev(inp["lc_v"]),
                  lc_valid=torch.tensor(c["lc_valid"], dtype=torch.int32).cuda(),
                  n_mem_valid=torch.tensor(c["n_mem_valid"], dtype=torch.int32).cuda())
    else:
        lengths = torch.tensor(c["lengths"], dtype=torch.int32).cuda()
    CTX = torch.full((c["B"], lay["rows_c"], lay["D"]), SENTINEL, device="cuda", dtype=dtype)
    try:
        ops.h.set_option(_lib.OPT_VALU_ATTENTION, int(force_valu))
        ops.emformer_attention(dev(inp["QKV"]), lengths, CTX, **kw)
        torch.cuda.synchronize()
    finally:
        ops.h.set_option(_lib.OPT_VALU_ATTENTION, 0)
    return CTX.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_emformer_attention_vs_fp64(ops, worst, name):
    c = CASES[name]
    inp = make_inputs(c, seed=_seed(name))
    refs = {dt: reference(c, inp, dt) for dt in (torch.float32, torch.bfloat16)}
    got = {}
    for variant, dtype, force in zip(VARIANTS, (torch.float32, torch.bfloat16, torch.bfloat16), (True, True, False)):
        ref, vmax, written = refs[dtype]
        cls = kernel_class(c, dtype) if not force else kernel_class(c, torch.float32)
        out = _run(ops, c, inp, dtype, force)
        got[variant] = out
        # segments past an utterance's length: nothing written, rc | utterance | summary rows bit-for-bit as they were
        assert torch.equal(out[~written], torch.full_like(out[~written], SENTINEL)), (name, variant, "sentinel rows touched")
        o, r = out.double()[written], ref[written]
        assert float(r.abs().max()) > 0.1
        bound = BF16_BOUND * vmax[written]
        err = (o - r).abs()
        ratio = float((err / bound).max())
        print(f"{name}: {variant} [{cls}]: max |got - ref| = {float(err.max()):.3e}, worst / bf16 bound = {ratio:.3f}")
        if dtype == torch.float32:
            torch.testing.assert_close(o, r, atol=2e-5, rtol=1e-4, msg=lambda m: f"{name}: {variant} [{cls}]: {m}")
        else:
            if ratio > worst.get(variant, (0.0, ""))[0]:
                worst[variant] = (ratio, name)
            assert bool((err <= bound).all()), (name, variant, cls, ratio)
    if mfma_eligible(c, torch.bfloat16):
        _, vmax, written = refs[torch.bfloat16]
        diff = (got["bf16 default"].double() - got["bf16 VALU"].double()).abs()[written]
        ratio = float((diff / (BF16_CROSS_BOUND * vmax[written])).max())
        print(f"{name}: bf16 MFMA vs bf16 VALU: worst / (6 * 2^-9 * max |v|) = {ratio:.3f}")
        if ratio > worst.get("MFMA vs VALU", (0.0, ""))[0]:
            worst["MFMA vs VALU"] = (ratio, name)
        assert ratio <= 1.0, (name, "MFMA vs VALU", ratio)
