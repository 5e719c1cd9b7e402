"""simulst_emformer_attention at segment geometries of more than 128 keys -- the blocked kernels of emformer_attn_tiled.hip -- against
the plain fp64 attention of test_hip_emformer_attention.py (its inputs, layout, reference, launcher, sentinel and bounds are
imported, not restated).  That reference takes its key sets from oracle.emformer.gen_attention_mask and knows no key limit.

Variants: fp32 (looped general form), bf16 under OPT_VALU_ATTENTION (looped general form), bf16 default (tiled MFMA form at
head_dim 64, looped otherwise).  kernel_class restates the dispatch rule; every case asserts the class the rule gives it, and where
two variants must (must not) be the same kernel their outputs are compared bit for bit.

Bounds, unchanged.  fp32: atol 2e-5 / rtol 1e-4.  bf16: 4 * 2^-9 * max_j |v_j| per (row, channel): under the online softmax every
probability is still rounded to bf16 exactly once (a relative rounding does not depend on the running max it was taken against),
the denominator is still summed from fp32 values, and the rescales are fp32 products adding <= 2^-24 per block.  Tiled MFMA
against bf16 looped: 6 * 2^-9 * max_j |v_j|.

The cases are the smallest at which a blocked kernel can go wrong (key blocks of 64 in the MFMA form, 128 in the looped form,
query blocks of 32): see the table in CASES.  test_reference_mutations_move_the_output_tiled (CPU) shows they can fail.
"""
import pytest
import torch

import test_hip_emformer_attention as base
from test_hip_emformer_attention import (BF16_BOUND, BF16_CROSS_BOUND, OFFLINE_MUTATIONS, SENTINEL, STREAMING_MUTATIONS, VARIANTS,
                                         _case, _run, layout, make_inputs, reference)
from test_hip_emformer_attention import ops, worst  # noqa: F401  (module-scoped fixtures)

_G1 = dict(S=64, R=8, Lc=48, M=9, T=200, H=2)                    # case 1: 129 keys, 73 queries
_ST = dict(streaming=True, S=16, R=8, Lc=120, M=5, H=2)
_STATE = dict(lc_valid=[120, 64, 0, 5, 119], n_mem_valid=[5, 2, 0, 1, 3])

OFFLINE = {
    # 1: one key past the old limit; nq 73 = two query blocks + 9
    "nk129_nq73": _case(**_G1),
    # 2: three MFMA key blocks + 1; nq 65 = two query blocks + 1
    "nk193_nq65": _case(S=56, R=8, Lc=120, M=9, T=170, H=2),
    # 3: query-block boundaries
    "nq32": _case(S=23, R=8, Lc=100, M=5, T=100, H=2),
    "nq33": _case(S=24, R=8, Lc=100, M=5, T=100, H=2),
    # 4: no memory, no summaries
    "nk136_nosum": _case(S=64, R=8, Lc=64, M=0, summary=False, T=130, H=2),
    # 5: exactly 128 keys: still the all-keys-at-once VALU kernel
    "nk128_old_kernel": _case(S=64, R=8, Lc=56, M=0, summary=False, T=130, H=2),
    # 6: piece boundaries against block edges.  135 segments of 2 rows: segment i has min(i, 130) memory keys, so memory|rc falls
    #    on key 63, 64, 65 and 127, 128, 129 (i = 63 .. 65, 127 .. 129) and rc|utterance on the same keys (i = 55 .. 57, 119 .. 121)
    "edges_mem_rc_utt": _case(S=2, R=8, Lc=60, M=130, T=270, H=2),
    # 7: the summary query's first key block is all memory keys (segments i >= 64; M = 70)
    "summary_first_block_memory": _case(S=4, R=2, Lc=56, M=70, T=300, H=2),
    # 8: lengths at a segment start, a start + 1 and 0: first segments far shorter than a block, later segments skipped
    "boundary_lengths": _case(**_G1, lengths=[128, 129, 64, 65, 0]),
    # 9: degenerate key-list pieces
    "R0": _case(S=64, R=0, Lc=64, M=5, T=200, H=2),
    "Lc0_S136": _case(S=136, R=8, Lc=0, M=5, T=300, H=2),
    # 10: head shapes at case 1's geometry
    "d16_H2": _case(**{**_G1, "d": 16}),
    "d32_H2": _case(**{**_G1, "d": 32}),
    "d40_H2": _case(**{**_G1, "d": 40}),
    "H1": _case(**{**_G1, "H": 1}),
    "H3": _case(**{**_G1, "H": 3}),
    "H8": _case(**{**_G1, "H": 8}),
}
STREAMING = {
    # 11: carried left context and memory bank
    "stream_T16": _case(**_ST, T=16, **_STATE),
    "stream_T11": _case(**_ST, T=11, **_STATE),
    "stream_T1": _case(**_ST, T=1, **_STATE),
    "stream_T11_empty_state": _case(**_ST, T=11, lc_valid=[0] * 5, n_mem_valid=[0] * 5),
    # 12: a full chunk
    "stream_T64_full_chunk": _case(streaming=True, S=64, R=8, Lc=64, M=5, H=2, T=64, lc_valid=[64, 63, 0, 1, 32],
                                   n_mem_valid=[5, 2, 0, 1, 3]),
    # 6, streaming: rc|lc is fixed by n_mem_valid + R; lc|utterance = n_mem_valid + 8 + lc_valid falls on key 64, 63, 65, 64, 64 ...
    "stream_edge64": _case(**_ST, T=16, lc_valid=[51, 50, 52, 56, 55], n_mem_valid=[5, 5, 5, 0, 1]),
    # ... and on key 128, 127, 129, 128, 128
    "stream_edge128": _case(**_ST, T=16, lc_valid=[115, 114, 116, 120, 119], n_mem_valid=[5, 5, 5, 0, 1]),
    # memory|rc on key 64, 63, 65, 70, 0: the summary query's first block is all memory keys in rows 0 and 2, 3
    "stream_mem_edge": _case(streaming=True, S=4, R=2, Lc=56, M=70, H=2, T=4, lc_valid=[56, 55, 1, 0, 56],
                             n_mem_valid=[64, 63, 65, 70, 0]),
}
CASES = {**OFFLINE, **STREAMING}


def nk_max(c):
    return c["M"] * int(c["summary"]) + c["R"] + c["Lc"] + layout(c)["S"]


def kernel_class(c, dtype, force_valu):
    """The dispatch rule of simulst_emformer_attention, restated: the blocked kernels for more than 128 keys and only for those."""
    if nk_max(c) <= 128:
        return base.kernel_class(c, torch.float32 if force_valu else dtype)
    if dtype == torch.bfloat16 and c["d"] == 64 and not force_valu:
        return "tiled MFMA"
    return "looped"


def _seed(name):
    return 5200 + list(CASES).index(name)


def test_classes_of_the_cases():
    """Every case but the nk = 128 one reaches the blocked kernels: the tiled MFMA form for bf16 at head_dim 64, the looped form
    for fp32, forced VALU and the other head dims; the geometry of 128 keys stays on the VALU kernel with two keys per lane."""
    bf, f32 = torch.bfloat16, torch.float32
    for name, c in CASES.items():
        if name == "nk128_old_kernel":
            assert nk_max(c) == 128
            assert {kernel_class(c, f32, True), kernel_class(c, bf, True), kernel_class(c, bf, False)} == {"VALU KPL=2"}
            continue
        assert nk_max(c) > 128, name
        assert kernel_class(c, f32, True) == kernel_class(c, bf, True) == "looped", name
        assert kernel_class(c, bf, False) == ("looped" if name in ("d16_H2", "d32_H2", "d40_H2") else "tiled MFMA"), name
    assert nk_max(CASES["nk129_nq73"]) == 129 and nk_max(CASES["nk193_nq65"]) == 193
    lay = layout(CASES["nq32"])
    assert CASES["nq32"]["R"] + lay["S"] + 1 == 32 and CASES["nq33"]["R"] + layout(CASES["nq33"])["S"] + 1 == 33


@pytest.mark.parametrize("name", ["nk193_nq65", "stream_T11"])
def test_reference_mutations_move_the_output_tiled(name):
    """As test_reference_mutations_move_the_output: one key dropped, admitted or swapped moves at least one element of the fp64
    reference by more than 10 x that element's bf16 bound.  A statement about the inputs of these cases."""
    c = CASES[name]
    inp = make_inputs(c, seed=_seed(name))
    ref, vmax, written = reference(c, inp, torch.bfloat16)
    assert bool(written.any()) and float(ref[written].abs().max()) > 0.1
    for mutation in (STREAMING_MUTATIONS if c["streaming"] else OFFLINE_MUTATIONS):
        mut, _, w2 = reference(c, inp, torch.bfloat16, mutation)
        assert torch.equal(w2, written)
        ratio = ((mut - ref).abs() / (BF16_BOUND * vmax))[written]
        print(f"{name}: {mutation}: max |mutated - ref| / bound = {float(ratio.max()):.1f}")
        assert float(ratio.max()) > 10, (name, mutation, float(ratio.max()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_emformer_attention_tiled_vs_fp64(ops, worst, name):  # noqa: F811
    c = CASES[name]
    inp = make_inputs(c, seed=_seed(name))
    refs = {dt: reference(c, inp, dt) for dt in (torch.float32, torch.bfloat16)}
    got, classes = {}, {}
    for variant, dtype, force in zip(VARIANTS, (torch.float32, torch.bfloat16, torch.bfloat16), (True, True, False)):
        ref, vmax, written = refs[dtype]
        cls = classes[variant] = kernel_class(c, dtype, force)
        out = got[variant] = _run(ops, c, inp, dtype, force)
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
            key = "tiled: " + variant
            if ratio > worst.get(key, (0.0, ""))[0]:
                worst[key] = (ratio, name)
            assert bool((err <= bound).all()), (name, variant, cls, ratio)
    _, vmax, written = refs[torch.bfloat16]
    same = torch.equal(got["bf16 default"], got["bf16 VALU"])
    if classes["bf16 default"] == "tiled MFMA":
        assert classes["bf16 VALU"] == "looped"
        # the matrix-core form rounds P to bf16 and the looped form does not: identical bits would mean the option chose nothing
        assert not same, (name, "bf16 default and bf16 VALU gave identical bits: the tiled MFMA form did not run")
        diff = (got["bf16 default"].double() - got["bf16 VALU"].double()).abs()[written]
        ratio = float((diff / (BF16_CROSS_BOUND * vmax[written])).max())
        print(f"{name}: bf16 tiled MFMA vs bf16 looped: worst / (6 * 2^-9 * max |v|) = {ratio:.3f}")
        if ratio > worst.get("tiled MFMA vs looped", (0.0, ""))[0]:
            worst["tiled MFMA vs looped"] = (ratio, name)
        assert ratio <= 1.0, (name, "tiled MFMA vs looped", ratio)
    else:
        # one and the same kernel with and without the option (looped for the other head dims; VALU KPL=2 at 128 keys)
        assert classes["bf16 default"] == classes["bf16 VALU"] and same, (name, classes)
