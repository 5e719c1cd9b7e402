"""simulst_linear's row-gather epilogue (SIMULST_EPI_ROW_GATHER, csrc/gemm_pick.hip; Ops.linear_gather) on the MI355X against fp64:
log_softmax of the logits computed from the SAME rounded operands (tests/ctc_ref.logits64), gathered at the labels.  GPU only.

Bound per element: 2e + N 2^-24 + 2^-20, with e measured as in tests/test_hip_ctc_pick.py (2 x the largest |fp32 - fp64| of the logits
simulst_linear writes for the same operands with SIMULST_EPI_BIAS_F32OUT: the error of a kernel that existed before, not of the code
under test) -- one e for the label's logit, one for the logsumexp; N 2^-24 + 2^-20 is the slack of tests/test_hip_transducer_lattice.py
for a sum of N exponentials.  A log-probability is at most that slack above 0.
Inputs: x ~ N(0, 1), W ~ N(0, 1) 4 / sqrt(K): logits of spread ~4."""
import math

import pytest
import torch

import ctc_ref as cr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, T = 3, 21                                    # 63 rows: the 16-row tiles straddle the utterances
GUARD = -7.25


@pytest.fixture(scope="module")
def ops():
    from simulst_amd.ops import Ops
    return Ops()


def _labels(Bb, Lp, N, seed):
    """a different list per utterance, with 0, N - 1 and repeats"""
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, N, (Bb, Lp), generator=g, dtype=torch.int32)
    for b in range(Bb):
        lo, hi = (0, N - 1) if b % 2 == 0 else (N - 1, 0)
        lab[b, 0] = lo
        if Lp >= 5:
            lab[b, 2] = lab[b, 3] = hi           # a repeat, next to each other
            lab[b, Lp - 1] = lab[b, 1]           # ... and apart
    return lab


_CASES = {}


def _case(ops, Bb, Tt, K, N, dtype, with_bias):
    """operands (x inside a wider NaN-filled buffer: batch stride > T K), the fp64 log-probabilities and the bound, made once"""
    key = (Bb, Tt, K, N, dtype, with_bias)
    if key not in _CASES:
        from simulst_amd._lib import EPI_BIAS_F32OUT
        g = torch.Generator().manual_seed(1000 * Bb + N + K + int(with_bias))
        x = torch.randn(Bb, Tt, K, generator=g).to(dtype)
        W = (torch.randn(N, K, generator=g) * 4 / math.sqrt(K)).to(dtype)
        bias = torch.randn(N, generator=g) if with_bias else None
        z = cr.logits64(x.reshape(Bb * Tt, K), W, bias)
        Wd, bd = W.to(DEV), None if bias is None else bias.to(DEV)
        logits = ops.linear(x.reshape(Bb * Tt, K).to(DEV), Wd, bd, epilogue=EPI_BIAS_F32OUT)
        e = 2 * float((logits.cpu().double() - z).abs().max())
        buf = torch.full((Bb, Tt + 5, K), float("nan")).to(dtype)
        buf[:, 2:2 + Tt] = x
        view = buf.to(DEV)[:, 2:2 + Tt]
        assert view.stride(0) > Tt * K
        lp = z.log_softmax(-1).view(Bb, Tt, N)
        _CASES[key] = (view, Wd, bd, lp, 2 * e + N * 2.0 ** -24 + 2.0 ** -20)
    return _CASES[key]


def _check(got, lp, lab, bound, N, what):
    want = lp.gather(2, lab.long().unsqueeze(1).expand(-1, lp.size(1), -1))
    got = got.cpu().double()
    assert got.shape == want.shape
    assert bool(torch.isfinite(got).all()), what
    err = float((got - want).abs().max())
    print(f"{what}: max |got - fp64| {err:.3e}  bound {bound:.3e}  max value {float(got.max()):.3e}")
    assert err <= bound, what
    assert float(got.max()) <= N * 2.0 ** -24 + 2.0 ** -20, what


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("Lp", [1, 16, 17, 37])
@pytest.mark.parametrize("N", [100, 4096])
def test_gather_against_fp64_bf16_split_form(ops, N, Lp, with_bias):
    """bf16, K = 256 on the matrix cores; one row panel: the column tiles are split over workgroups, the gather phase writes raw z and
    the fold launch subtracts the logsumexp.  x is read through a strided view; C is a window of a guard-filled buffer."""
    x, W, b, lp, bound = _case(ops, B, T, 256, N, torch.bfloat16, with_bias)
    lab = _labels(B, Lp, N, 7 * N + Lp)
    Cbuf = torch.full((B, T + 2, Lp + 3), GUARD, device=DEV)
    out = ops.linear_gather(x, W, b, lab.to(DEV), out=Cbuf[:, 1:1 + T, 2:2 + Lp])
    torch.cuda.synchronize()
    assert out.data_ptr() == Cbuf[:, 1:, 2:].data_ptr()
    _check(out, lp, lab, bound, N, f"N={N} L'={Lp} bias={with_bias}")
    outside = torch.ones(B, T + 2, Lp + 3, dtype=torch.bool)
    outside[:, 1:1 + T, 2:2 + Lp] = False
    assert bool((Cbuf.cpu()[outside] == GUARD).all())
    # the default output: a new contiguous tensor with the same bits
    assert torch.equal(ops.linear_gather(x, W, b, lab.to(DEV)), out)


@pytest.mark.parametrize("N,Lp", [(100, 17), (4096, 37)])
def test_time_major_output(ops, N, Lp):
    """C [T][B][L'] addressed as [B, T, L'] with c_row_stride = B L', c_batch_stride = L' -- the layout ctc.ctc_rescore asks for"""
    x, W, b, lp, bound = _case(ops, B, T, 256, N, torch.bfloat16, True)
    lab = _labels(B, Lp, N, 11 * N + Lp)
    buf = torch.full((T + 2, B, Lp), GUARD, device=DEV)
    out = ops.linear_gather(x, W, b, lab.to(DEV), out=buf[1:1 + T].transpose(0, 1))
    torch.cuda.synchronize()
    assert out.stride() == (Lp, B * Lp, 1)
    _check(out, lp, lab, bound, N, f"time-major N={N} L'={Lp}")
    assert bool((buf[0] == GUARD).all()) and bool((buf[T + 1] == GUARD).all())
    assert torch.equal(buf[1:1 + T].transpose(0, 1), ops.linear_gather(x, W, b, lab.to(DEV)))


def test_unsplit_form_at_128_row_panels(ops):
    """389 x 21 = 8169 rows = 128 panels of 64: every workgroup sweeps the whole width and subtracts the logsumexp itself; utterances
    of 21 rows against 16-row tiles: every tile straddles two label lists"""
    Bb, N, K, Lp = 389, 128, 32, 17
    x, W, b, lp, bound = _case(ops, Bb, T, K, N, torch.bfloat16, True)
    lab = _labels(Bb, Lp, N, 5)
    Cbuf = torch.full((Bb * T * Lp + 64,), GUARD, device=DEV)
    out = ops.linear_gather(x, W, b, lab.to(DEV), out=Cbuf[32:32 + Bb * T * Lp].view(Bb, T, Lp))
    torch.cuda.synchronize()
    _check(out, lp, lab, bound, N, "unsplit")
    assert bool((Cbuf[:32] == GUARD).all()) and bool((Cbuf[-32:] == GUARD).all())


@pytest.mark.parametrize("dtype,K", [(torch.float32, 256), (torch.float32, 40), (torch.bfloat16, 40)])
@pytest.mark.parametrize("N,Lp", [(100, 17), (4096, 37)])
def test_valu_form(ops, dtype, K, N, Lp):
    """fp32, and bf16 with K % 32 != 0: the VALU kernels (correctness only), 4 rows per workgroup: 21-row utterances straddle them too"""
    x, W, b, lp, bound = _case(ops, B, T, K, N, dtype, True)
    lab = _labels(B, Lp, N, 13 * N + Lp + K)
    Cbuf = torch.full((B, T + 2, Lp + 3), GUARD, device=DEV)
    out = ops.linear_gather(x, W, b, lab.to(DEV), out=Cbuf[:, 1:1 + T, 2:2 + Lp])
    torch.cuda.synchronize()
    _check(out, lp, lab, bound, N, f"VALU {dtype} K={K} N={N} L'={Lp}")
    outside = torch.ones(B, T + 2, Lp + 3, dtype=torch.bool)
    outside[:, 1:1 + T, 2:2 + Lp] = False
    assert bool((Cbuf.cpu()[outside] == GUARD).all())


def test_out_of_range_labels_are_clamped_and_bad_arguments_raise(ops):
    x, W, b, lp, bound = _case(ops, B, T, 256, 100, torch.bfloat16, True)
    lab = _labels(B, 5, 100, 3)
    wild = lab.clone()
    wild[0, 0], wild[1, 1] = -4, 100 + 17
    want = lab.clone()
    want[0, 0], want[1, 1] = 0, 99
    assert torch.equal(ops.linear_gather(x, W, b, wild.to(DEV)), ops.linear_gather(x, W, b, want.to(DEV)))
    with pytest.raises(ValueError, match="labels"):
        ops.linear_gather(x, W, b, lab.long().to(DEV))
    with pytest.raises(ValueError, match="labels"):
        ops.linear_gather(x, W, b, lab[:, :0].to(DEV))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.linear_gather(x.cpu(), W, b, lab.to(DEV))
    empty = ops.linear_gather(x[:0], W, b, lab[:0].to(DEV))
    assert tuple(empty.shape) == (0, T, 5)
