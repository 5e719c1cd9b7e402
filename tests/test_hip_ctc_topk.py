"""simulst_linear's row top-k epilogue (SIMULST_EPI_ROW_TOPK, csrc/gemm_pick.hip; Ops.linear_topk) on the MI355X against the fp64 top-k
of the SAME rounded operands (tests/ctc_beam_ref.py).  GPU only.

Error bound of a case, e = 2 x the largest |fp32 - fp64| of the logits that simulst_linear writes for that same case with
SIMULST_EPI_BIAS_F32OUT, measured here: the error of a contraction kernel that existed before, not of the code under test.
  lprob and lse within e (+ 1e-6 |lse|) of fp64;
  a row in which two neighbours among its best k + 1 non-keep fp64 values lie within 2e is UNCLEAR: there the columns must be within 2e
  of the fp64 k-th value or above, in an order descending to within 2e; every other row holds the fp64 ids exactly and in order; at
  most 1 % of a case's rows may be unclear (tests/test_ctc_beam_cpu.py checks the seeds for that without a GPU).
Inputs: x ~ N(0, 1), W ~ N(0, 1) 4 / sqrt(K): logits of spread ~4."""
import math

import pytest
import torch

import ctc_beam_ref as br

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope="module")
def ops():
    from simulst_amd.ops import Ops
    return Ops()


_CASES = {}


def _case(ops, M, K, N, dtype, with_bias):
    """operands on the device, the fp64 logits and the measured bound e of one case, made once and shared"""
    key = (M, K, N, dtype, with_bias)
    if key not in _CASES:
        from simulst_amd._lib import EPI_BIAS_F32OUT
        x, W, bias, z = br.topk_operands(M, K, N, dtype, with_bias)
        xd, Wd, bd = x.to(DEV), W.to(DEV), None if bias is None else bias.to(DEV)
        logits = ops.linear(xd, Wd, bd, epilogue=EPI_BIAS_F32OUT)
        e = 2 * float((logits.cpu().double() - z).abs().max())
        _CASES[key] = (xd, Wd, bd, z, e)
    return _CASES[key]


def _keep(which, N):
    return {"none": None, "first": 0, "last": N - 1}[which]


@pytest.mark.parametrize("which", ["none", "first", "last"])
@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,K,N", br.TOPK_SHAPES)
def test_topk_against_fp64(ops, M, K, N, dtype, with_bias, k, which):
    x, W, b, z, e = _case(ops, M, K, N, dtype, with_bias)
    keep = _keep(which, N)
    ids, lprob, lse = ops.linear_topk(x, W, b, k=k, keep=keep)
    torch.cuda.synchronize()
    kp = k + (keep is not None)
    assert ids.dtype == torch.int32 and ids.shape == lprob.shape == (M, kp) and lse.shape == (M,)
    unclear = br.check_topk(z, ids, lprob, lse, k, keep, e, f"{(M, K, N)} {dtype} bias={with_bias} k={k} keep={keep}")
    print(f"M={M} K={K} N={N} {dtype} bias={with_bias} k={k} keep={keep}: e {e:.3e}  unclear rows {int(unclear.sum())}")
    assert int(unclear.sum()) <= 0.01 * M
    if keep is None:
        assert torch.equal(ids[:, 0], ops.linear_pick(x, W, b)[0])      # the same instruction sequence per column: the pick on EVERY row


@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_operands_and_untouched_surroundings(ops, dtype):
    """A: [3][21] rows, each K of a 2K-wide buffer row, inside a [3][30] buffer whose every other element is NaN; C: a window of a
    sentinel-filled int32 buffer [3][40][k' + 3] (batch stride 40 rows, row stride k' + 3)."""
    B, T, K, N, k, keep = 3, 21, 256, 100, 8, 0
    kp = k + 1
    g = torch.Generator().manual_seed(7)
    buf = torch.full((B, 30, 2 * K), float("nan")).to(dtype)
    rows = torch.randn(B, T, K, generator=g).to(dtype)
    buf[:, 4:4 + T, :K] = rows
    W = (torch.randn(N, K, generator=g) * 4 / math.sqrt(K)).to(dtype)
    bias = torch.randn(N, generator=g)
    z = rows.reshape(B * T, K).double() @ W.double().t() + bias.double()
    from simulst_amd._lib import EPI_BIAS_F32OUT
    e = 2 * float((ops.linear(rows.reshape(B * T, K).to(DEV), W.to(DEV), bias.to(DEV), epilogue=EPI_BIAS_F32OUT).cpu().double() - z).abs().max())
    bufd = buf.to(DEV)
    view = bufd[:, 4:4 + T, :K]
    Cbuf = torch.full((B, 40, kp + 3), -7, dtype=torch.int32, device=DEV)
    win = Cbuf[:, 5:5 + T, 1:1 + kp]
    ids, lprob, lse = ops.linear_topk(view, W.to(DEV), bias.to(DEV), k=k, keep=keep, out=win)
    torch.cuda.synchronize()
    assert ids.shape == lprob.shape == (B, T, kp) and lse.shape == (B, T) and ids.data_ptr() == win.data_ptr()
    assert bool(torch.isfinite(lprob).all()) and bool(torch.isfinite(lse).all())          # no gap element was read
    br.check_topk(z, ids.reshape(B * T, kp), lprob.reshape(B * T, kp), lse.reshape(-1), k, keep, e, f"strided {dtype}")
    outside = torch.ones(B, 40, kp + 3, dtype=torch.bool)
    outside[:, 5:5 + T, 1:1 + kp] = False
    assert bool((Cbuf.cpu()[outside] == -7).all())
    # the same rows as a 2-D [B * T', K] view with rows_per_batch: the batch stride is rows_per_batch row strides
    flat = bufd.view(B * 30, 2 * K)[:, :K]
    i2, l2, s2 = ops.linear_topk(flat, W.to(DEV), bias.to(DEV), k=k, keep=keep, rows_per_batch=30)
    assert i2.shape == (B, 30, kp) and torch.equal(i2[:, 4:4 + T], ids) and torch.equal(l2[:, 4:4 + T], lprob) and torch.equal(s2[:, 4:4 + T], lse)


@pytest.mark.parametrize("M,K,N", br.TOPK_SPLIT_SHAPES)
def test_both_sides_of_the_column_split(ops, M, K, N):
    """bf16 on the matrix cores: 127 row panels split the column tiles over several workgroups and fold the parts in a second launch,
    128 panels give every workgroup the whole width (csrc/gemm_plan.cpp plan_row_pick).  Same bounds as above."""
    x, W, b, z, e = _case(ops, M, K, N, torch.bfloat16, True)
    for k, keep in ((8, 0), (8, None), (1, N - 1)):
        ids, lprob, lse = ops.linear_topk(x, W, b, k=k, keep=keep)
        unclear = br.check_topk(z, ids, lprob, lse, k, keep, e, f"M={M} k={k} keep={keep}")
        print(f"M={M} k={k} keep={keep}: e {e:.3e} unclear rows {int(unclear.sum())}")
        assert int(unclear.sum()) <= 0.01 * M
        if keep is None:
            assert torch.equal(ids[:, 0], ops.linear_pick(x, W, b)[0])


@pytest.mark.parametrize("M,K,N", [(17, 256, 4096), (8129, 64, 272)])
def test_fragment_major_weights_give_the_same_bits(ops, M, K, N):
    """bf16 weights in simulst_pack_fragment_major's order (N % 16 == 0, K % 32 == 0): the same fragments reach the same instructions,
    split over column parts (17 rows) or not (8129 rows)"""
    x, W, b, _, _ = _case(ops, M, K, N, torch.bfloat16, True)
    want = ops.linear_topk(x, W, b, k=8, keep=0)
    got = ops.linear_topk(x, ops.pack_fragment_major(W), b, k=8, keep=0, w_fragment_major=True)
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    with pytest.raises(RuntimeError, match="fragment-major"):
        ops.linear_topk(x.float(), W.float(), b, k=8, keep=0, w_fragment_major=True)


TIES = {"first and last": lambda N: (0, N - 1), "15 | 16": lambda N: (15, 16), "63 | 64": lambda N: (63, 64),
        "last two": lambda N: (N - 2, N - 1), "three": lambda N: (5, 70, N - 3)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [100, 4097])
def test_exact_ties_keep_both_columns_the_lower_one_first(ops, dtype, N):
    """rows of W duplicated: the tied columns hold the same bits.  Row 0 of A points along the duplicated weight row, so the tie is
    the row's maximum by a wide margin: with k = 8 every tied column is present, ascending, in the first slots; with k = 1 the lowest."""
    K = 256
    g = torch.Generator().manual_seed(N)
    base = (torch.randn(N, K, generator=g) * 4 / math.sqrt(K)).to(dtype)
    for with_bias in (False, True):
        for name, cols in TIES.items():
            cols = cols(N)
            W = base.clone()
            for c in cols[1:]:
                W[c] = W[cols[0]]
            bias = None
            if with_bias:
                bias = torch.randn(N, generator=g)
                bias[list(cols)] = float(bias[cols[0]])
            x = torch.cat([(W[cols[0]].float() * 2).unsqueeze(0), torch.randn(3, K, generator=g)]).to(dtype)
            z = x.double() @ W.double().t() + (0 if bias is None else bias.double())
            top = z[0].max()
            assert float((z[0, list(cols)] - top).abs().max()) < 1e-9 and int((z[0] > top - 1.0).sum()) == len(cols), name
            xd, Wd, bd = x.to(DEV), W.to(DEV), None if bias is None else bias.to(DEV)
            ids, lprob, _ = ops.linear_topk(xd, Wd, bd, k=8)
            assert ids[0, :len(cols)].tolist() == sorted(cols), (name, N, dtype, with_bias, ids[0].tolist())
            assert len(set(lprob[0, :len(cols)].tolist())) == 1
            assert int(ops.linear_topk(xd, Wd, bd, k=1)[0][0, 0]) == min(cols)
            if 0 not in cols:
                ids, _, _ = ops.linear_topk(xd, Wd, bd, k=8, keep=0)
                assert ids[0, :1 + len(cols)].tolist() == [0] + sorted(cols)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [1, 16, 100, 4096, 4097])
def test_all_zero_rows(ops, dtype, N):
    """A = 0 and no bias: every column ties at 0.  The columns come out as 0 .. k - 1 (after keep), each at -log N, -1 past N"""
    K, M, k = 256, 19, 8
    g = torch.Generator().manual_seed(N)
    W = torch.randn(N, K, generator=g).to(dtype).to(DEV)
    x = torch.zeros(M, K, dtype=dtype, device=DEV)
    for keep in (None, 0, N - 1):
        ids, lprob, lse = ops.linear_topk(x, W, k=k, keep=keep)
        others = [c for c in range(N) if c != keep][:k]
        want = ([] if keep is None else [keep]) + others + [-1] * (k - len(others))
        assert ids.cpu().tolist() == [want] * M, (N, keep, ids[0].tolist())
        assert float((lse.cpu().double() - math.log(N)).abs().max()) <= 1e-6 * max(1.0, math.log(N))
        n_real = len(want) - want.count(-1)
        assert float((lprob[:, :n_real].cpu().double() + math.log(N)).abs().max()) <= 1e-6 * max(1.0, math.log(N))
        assert bool((lprob[:, n_real:] == float("-inf")).all())


def test_cpu_tensors_raise_and_no_rows(ops):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.linear_topk(torch.zeros(4, 32), torch.zeros(8, 32), k=2)
    ids, lprob, lse = ops.linear_topk(torch.zeros(0, 32, device=DEV), torch.zeros(8, 32, device=DEV), k=3, keep=0)
    assert ids.shape == lprob.shape == (0, 4) and lse.shape == (0,)
    ids, lprob, lse = ops.linear_topk(torch.zeros(2, 0, 32, device=DEV), torch.zeros(8, 32, device=DEV), k=3)
    assert ids.shape == lprob.shape == (2, 0, 3) and lse.shape == (2, 0)
    with pytest.raises(RuntimeError, match="aux_rows"):
        ops.linear_topk(torch.zeros(4, 32, device=DEV), torch.zeros(8, 32, device=DEV), k=9)
    with pytest.raises(RuntimeError, match="n_main"):
        ops.linear_topk(torch.zeros(4, 32, device=DEV), torch.zeros(8, 32, device=DEV), k=2, keep=8)
