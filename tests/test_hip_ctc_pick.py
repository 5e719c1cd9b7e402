"""simulst_linear's row-pick epilogue (SIMULST_EPI_ROW_PICK, csrc/gemm_pick.hip; Ops.linear_pick) on the MI355X against an fp64 pick
computed from the SAME rounded operands (tests/ctc_ref.py).  GPU only.

Error bound of a case, e = 2 x the largest |fp32 - fp64| of the logits that simulst_linear writes for that same case with
SIMULST_EPI_BIAS_F32OUT, measured here: the error of the contraction kernels that existed before, not of the code under test.
  zmax within e of fp64, lse within e + 1e-6 |lse|;
  a row whose fp64 top-2 margin is <= 2e is UNCLEAR: there the pick must be a column within 2e of the maximum, everywhere else it must
  be the fp64 pick (the lowest maximal column) exactly; at most 1 % of a case's rows may be unclear.
Inputs: x ~ N(0, 1), W ~ N(0, 1) 4 / sqrt(K): logits of spread ~4."""
import math

import pytest
import torch

import ctc_ref as cr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 256, 4096), (17, 256, 4096), (130, 256, 4097), (513, 64, 100), (64, 256, 16), (33, 32, 1)]
DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope="module")
def ops():
    from simulst_amd.ops import Ops
    return Ops()


_CASES = {}


def _case(ops, M, K, N, dtype, with_bias):
    """operands, the fp64 logits and the measured bound e of one case, made once and shared"""
    key = (M, K, N, dtype, with_bias)
    if key not in _CASES:
        from simulst_amd._lib import EPI_BIAS_F32OUT
        g = torch.Generator().manual_seed(1000 * M + N + K + int(with_bias))
        x = torch.randn(M, K, generator=g).to(dtype)
        W = (torch.randn(N, K, generator=g) * 4 / math.sqrt(K)).to(dtype)
        bias = torch.randn(N, generator=g) if with_bias else None
        z = cr.logits64(x, W, bias)
        xd, Wd, bd = x.to(DEV), W.to(DEV), None if bias is None else bias.to(DEV)
        logits = ops.linear(xd, Wd, bd, epilogue=EPI_BIAS_F32OUT)
        e = 2 * float((logits.cpu().double() - z).abs().max())
        _CASES[key] = (xd, Wd, bd, z, e)
    return _CASES[key]


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,K,N", SHAPES)
def test_pick_zmax_lse_against_fp64(ops, M, K, N, dtype, with_bias):
    x, W, b, z, e = _case(ops, M, K, N, dtype, with_bias)
    pick, zmax, lse = ops.linear_pick(x, W, b)
    torch.cuda.synchronize()
    assert pick.dtype == torch.int32 and pick.shape == zmax.shape == lse.shape == (M,)
    _, zmax64, lse64, _ = cr.pick64(z)
    dz = float((zmax.cpu().double() - zmax64).abs().max())
    dl = ((lse.cpu().double() - lse64).abs() - 1e-6 * lse64.abs())
    unclear = cr.check_pick(z, pick, e, f"{(M, K, N)} {dtype} bias={with_bias}")
    print(f"M={M} K={K} N={N} {dtype} bias={with_bias}: e {e:.3e}  |zmax - fp64| {dz:.3e}  max(|lse - fp64| - 1e-6 |lse|) {float(dl.max()):.3e}  "
          f"unclear rows {int(unclear.sum())}")
    assert dz <= e
    assert float(dl.max()) <= e
    assert int(unclear.sum()) <= 0.01 * M


@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_operands_and_untouched_surroundings(ops, dtype):
    """A: [3][21] rows, each K of a 2K-wide buffer row, inside a [3][30] buffer whose every other element is NaN (gap rows and the
    right half of the addressed rows); C: a window of a sentinel-filled int32 buffer with c_batch_stride 40 > 21 rows."""
    B, T, K, N = 3, 21, 256, 100
    g = torch.Generator().manual_seed(7)
    buf = torch.full((B, 30, 2 * K), float("nan")).to(dtype)
    rows = torch.randn(B, T, K, generator=g).to(dtype)
    buf[:, 4:4 + T, :K] = rows
    W = (torch.randn(N, K, generator=g) * 4 / math.sqrt(K)).to(dtype)
    bias = torch.randn(N, generator=g)
    z = cr.logits64(rows.reshape(B * T, K), W, bias)
    from simulst_amd._lib import EPI_BIAS_F32OUT
    e = 2 * float((ops.linear(rows.reshape(B * T, K).to(DEV), W.to(DEV), bias.to(DEV), epilogue=EPI_BIAS_F32OUT).cpu().double() - z).abs().max())
    bufd = buf.to(DEV)
    view = bufd[:, 4:4 + T, :K]
    assert view.stride() == (30 * 2 * K, 2 * K, 1)
    Cbuf = torch.full((B, 40), -7, dtype=torch.int32, device=DEV)
    pick, zmax, lse = ops.linear_pick(view, W.to(DEV), bias.to(DEV), out=Cbuf[:, 5:5 + T])
    torch.cuda.synchronize()
    assert pick.shape == zmax.shape == lse.shape == (B, T) and pick.data_ptr() == Cbuf[:, 5:].data_ptr()
    assert bool(torch.isfinite(zmax).all()) and bool(torch.isfinite(lse).all())          # no gap element was read
    cr.check_pick(z, pick.reshape(-1), e, f"strided {dtype}")
    _, zmax64, lse64, _ = cr.pick64(z)
    assert float((zmax.reshape(-1).cpu().double() - zmax64).abs().max()) <= e
    assert float(((lse.reshape(-1).cpu().double() - lse64).abs() - 1e-6 * lse64.abs()).max()) <= e
    outside = torch.ones(B, 40, dtype=torch.bool)
    outside[:, 5:5 + T] = False
    assert bool((Cbuf.cpu()[outside] == -7).all())
    # the same rows as a 2-D [B * T', K] view with rows_per_batch: the batch stride is rows_per_batch row strides
    flat = bufd.view(B * 30, 2 * K)[:, :K]
    p2, z2, l2 = ops.linear_pick(flat, W.to(DEV), bias.to(DEV), rows_per_batch=30)
    assert p2.shape == (B, 30) and torch.equal(p2[:, 4:4 + T], pick) and torch.equal(z2[:, 4:4 + T], zmax) and torch.equal(l2[:, 4:4 + T], lse)


@pytest.mark.parametrize("M", [8128, 8129])
def test_both_sides_of_the_column_split(ops, M):
    """bf16 on the matrix cores: 127 row panels split the column tiles over several workgroups and fold the parts in a second launch,
    128 panels give every workgroup the whole width (csrc/gemm_plan.cpp plan_row_pick).  Same bounds as above."""
    K, N = 64, 272
    x, W, b, z, e = _case(ops, M, K, N, torch.bfloat16, True)
    pick, zmax, lse = ops.linear_pick(x, W, b)
    unclear = cr.check_pick(z, pick, e, f"M={M}")
    _, zmax64, lse64, _ = cr.pick64(z)
    assert float((zmax.cpu().double() - zmax64).abs().max()) <= e
    assert float(((lse.cpu().double() - lse64).abs() - 1e-6 * lse64.abs()).max()) <= e
    assert int(unclear.sum()) <= 0.01 * M


@pytest.mark.parametrize("M,K,N", [(17, 256, 4096), (8129, 64, 272)])
def test_fragment_major_weights_give_the_same_bits(ops, M, K, N):
    """bf16 weights in simulst_pack_fragment_major's order (N % 16 == 0, K % 32 == 0): the same fragments reach the same instructions,
    split over column parts (17 rows) or not (8129 rows)"""
    x, W, b, _, _ = _case(ops, M, K, N, torch.bfloat16, True)
    want = ops.linear_pick(x, W, b)
    got = ops.linear_pick(x, ops.pack_fragment_major(W), b, w_fragment_major=True)
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    with pytest.raises(RuntimeError, match="fragment-major"):
        ops.linear_pick(x.float(), W.float(), b, w_fragment_major=True)


TIES = {"first and last": lambda N: (0, N - 1), "15 | 16": lambda N: (15, 16), "63 | 64": lambda N: (63, 64),
        "last two": lambda N: (N - 2, N - 1), "three": lambda N: (5, 70, N - 3)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [100, 4097])
def test_exact_ties_go_to_the_lowest_column(ops, dtype, N):
    """rows of W duplicated: the tied columns hold the same bits.  Row i of A points along the duplicated weight row of tie i, so the
    tie is the row's maximum by a wide margin."""
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
            z = cr.logits64(x, W, bias)
            # (the fp64 product's own summation order may differ between columns in the last bit: the tie is exact for the kernel,
            #  whose every column runs the same instruction sequence, and exact to 1e-9 here)
            top = z[0].max()
            assert float((z[0, list(cols)] - top).abs().max()) < 1e-9 and int((z[0] > top - 1.0).sum()) == len(cols), name
            pick, _, _ = ops.linear_pick(x.to(DEV), W.to(DEV), None if bias is None else bias.to(DEV))
            assert int(pick[0]) == min(cols), (name, N, dtype, with_bias, int(pick[0]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [1, 16, 100, 4096, 4097])
def test_all_zero_rows(ops, dtype, N):
    """A = 0: every column ties at its bias.  Without one the pick is column 0 and lse = log N; with one it is the bias's first maximum."""
    K, M = 256, 19
    g = torch.Generator().manual_seed(N)
    W = torch.randn(N, K, generator=g).to(dtype).to(DEV)
    x = torch.zeros(M, K, dtype=dtype, device=DEV)
    pick, zmax, lse = ops.linear_pick(x, W)
    assert bool((pick == 0).all()) and bool((zmax == 0).all())
    # "lse = log N to 1e-6": of log N's own size, as the other lse bounds are (fp32 holds log 4097 = 8.318 to 4.8e-7 at best), and
    # absolutely where log N < 1
    assert float((lse.cpu().double() - math.log(N)).abs().max()) <= 1e-6 * max(1.0, math.log(N))
    bias = torch.randn(N, generator=g)
    hi = float(bias.max() + 1.0)                            # (an fp32 value)
    first = min(N - 1, 37)
    bias[first:] = torch.where(torch.rand(N - first, generator=g) < 0.5, torch.tensor(hi), bias[first:])
    bias[first] = hi
    pick, zmax, lse = ops.linear_pick(x, W, bias.to(DEV))
    assert bool((pick == first).all()) and bool((zmax.cpu() == hi).all())
    assert float((lse.cpu().double() - torch.logsumexp(bias.double(), 0)).abs().max()) <= 1e-6 * float(torch.logsumexp(bias.double(), 0).abs())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [100, 4097])
def test_range_and_the_last_column_of_a_ragged_tail(ops, dtype, N):
    """logits of about +-60: lse stays finite and within 1e-6 relative; the maximum placed in the last column is found"""
    K, M = 256, 40
    g = torch.Generator().manual_seed(3 * N)
    W = (torch.randn(N, K, generator=g) * 18 / math.sqrt(K)).to(dtype)
    x = torch.randn(M, K, generator=g)
    x[::2] = W[N - 1].float() * (3.5 / float(W[N - 1].float().norm()))             # every other row: the last column wins, z ~ 60
    x = x.to(dtype)
    z = cr.logits64(x, W)
    ref, zmax64, lse64, margin = cr.pick64(z)
    assert bool((ref[::2] == N - 1).all()) and float(margin[::2].min()) > 1.0 and 45 < float(z.abs().max()) < 90
    pick, zmax, lse = ops.linear_pick(x.to(DEV), W.to(DEV))
    assert bool((pick.cpu()[::2] == N - 1).all())
    assert bool(torch.isfinite(lse).all()) and bool(torch.isfinite(zmax).all())
    rel = ((lse.cpu().double() - lse64).abs() / lse64.abs())
    print(f"N={N} {dtype}: max |z| {float(z.abs().max()):.1f}  max relative lse error {float(rel.max()):.3e}")
    assert float(rel.max()) <= 1e-6


def test_cpu_tensors_raise(ops):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.linear_pick(torch.zeros(4, 32), torch.zeros(8, 32))
    pick, zmax, lse = ops.linear_pick(torch.zeros(0, 32, device=DEV), torch.zeros(8, 32, device=DEV))
    assert pick.shape == zmax.shape == lse.shape == (0,)
