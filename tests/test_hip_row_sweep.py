"""The identities between the row-pick, row-gather and row-top-k epilogues of simulst_linear: their column sweeps (csrc/row_sweep.h:
the top-k kernel runs sweep_columns, the pick kernel a copy of that loop, the gather phase one accumulator of it) make z and the
running (max, sum exp) of every column with the same k order and accumulator start, so the three entry points agree in every bit,
not within a tolerance.  GPU only.

Per case (tests/ctc_beam_ref.py topk_operands; with and without bias; W row-major and, where the plan takes it -- bf16 on the matrix
cores with N % 16 == 0 -- fragment-major):
  top-k lse == pick lse;
  top-k lprob[:, 0] (no keep column) == pick zmax - lse;
  linear_gather at labels = the pick's columns == pick zmax - lse (row-major W only: the plan refuses fragment-major weights for the
  gather form).
Shapes: bf16 (17, 256, 4096) column parts + fold launch, (130, 256, 4097) a ragged last tile, (8129, 64, 272) one workgroup per
panel over the whole width, (33, 32, 1) a single column; fp32 (5, 32, 8) the VALU form."""
import pytest
import torch

import ctc_beam_ref as br

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(17, 256, 4096, torch.bfloat16), (130, 256, 4097, torch.bfloat16), (8129, 64, 272, torch.bfloat16),
         (33, 32, 1, torch.bfloat16), (5, 32, 8, torch.float32)]
# (M, K, N, dtype, with_bias, fragment_major) -- fragment-major only where plan_row_pick takes it
PARAMS = [c + (wb, fm) for c in CASES for wb in (False, True) for fm in (False, True)
          if not fm or (c[3] == torch.bfloat16 and c[2] % 16 == 0)]


@pytest.fixture(scope="module")
def ops():
    from simulst_amd.ops import Ops
    return Ops()


def _id(c):
    return f"{c[0]}x{c[1]}x{c[2]}-{str(c[3]).replace('torch.', '')}-{'bias' if c[4] else 'nobias'}-{'fragment' if c[5] else 'rowmajor'}"


@pytest.mark.parametrize("M,K,N,dtype,with_bias,fragment_major", PARAMS, ids=[_id(c) for c in PARAMS])
def test_pick_topk_and_gather_see_the_same_sweep(ops, M, K, N, dtype, with_bias, fragment_major):
    x, W, b, _ = br.topk_operands(M, K, N, dtype, with_bias)
    x, W, b = x.to(DEV), W.to(DEV), None if b is None else b.to(DEV)
    Wl = ops.pack_fragment_major(W) if fragment_major else W
    pick, zmax, lse = ops.linear_pick(x, Wl, b, w_fragment_major=fragment_major)
    want = zmax - lse
    differ = []                                              # every identity is evaluated before the assertion names the broken ones
    for k in (1, 8):
        ids, lprob, lse_k = ops.linear_topk(x, Wl, b, k=k, w_fragment_major=fragment_major)
        differ += [] if torch.equal(lse_k, lse) else [f"top-k lse (k={k})"]
        differ += [] if torch.equal(lprob[:, 0], want) else [f"top-k lprob[:, 0] (k={k})"]
        differ += [] if torch.equal(ids[:, 0], pick) else [f"top-k ids[:, 0] (k={k})"]
    if not fragment_major:
        got = ops.linear_gather(x.view(M, 1, K), W, b, pick.view(M, 1))
        differ += [] if torch.equal(got.view(M), want) else ["gather at the pick's columns"]
    assert not differ, differ
