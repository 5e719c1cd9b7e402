"""Every entry point whose kernels ask for more dynamic LDS than the default limit raises that limit itself, per handle, before its
first launch (csrc/common.h sl_raise_lds): on a FRESH handle the first call succeeds and writes the bytes the module's shared handle
writes, and so does the same call on a second fresh handle (a slot left set by the first could not hide a missing raise there).
A limit that is not raised is a launch error, i.e. a RuntimeError out of Handle.check.

Shapes: the smallest at which each launcher's request exceeds its threshold.  The feed-forward launches always ask for theirs (128
rows, F = 64); simulst_linear's two big-LDS routes start at 8192 rows; conv_pos asks for (k cpg^2 + cpg (64 + k)) * 4 bytes: 16
channels per group pass 48 KiB at k = 42 (49 792; k = 41: 48 704); the CTC alignment for 72 (2 L + 1) + 16: past 48 KiB at L = 341
labels (49 192; L = 340: 49 048); the joiner lattice for 16 R (D + pad) elements: past the 64 KiB default at D = 256 in both dtypes.
"""
import pytest
import torch

from simulst_amd import _lib

pytestmark = pytest.mark.gpu
D = 256


def _rn(g, *shape, scale=1.0, dtype=torch.bfloat16):
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


def _ffn_weights(g, F):
    from simulst_amd.encoder import ffn_pack_w1, ffn_pack_w2
    W1, W2 = _rn(g, F, D, scale=D ** -0.5), _rn(g, D, F, scale=F ** -0.5)
    return (1 + 0.1 * torch.randn(D, generator=g)).cuda(), (0.1 * torch.randn(D, generator=g)).cuda(), ffn_pack_w1(W1), \
        _rn(g, F, scale=0.1, dtype=torch.float32), ffn_pack_w2(W2), _rn(g, D, scale=0.1, dtype=torch.float32)


def _ffn(ops, g):
    x, out = _rn(g, 128, D), torch.zeros(128, D, device="cuda", dtype=torch.bfloat16)
    return [ops.emformer_ffn(x, *_ffn_weights(g, 64), out)]


def _ffn_block_form(ops, g):
    ops.h.set_option(_lib.OPT_FFN_WAVES, 4)
    try:
        return _ffn(ops, g)
    finally:
        ops.h.set_option(_lib.OPT_FFN_WAVES, 0)


def _ffn_prenorm_qkv_and_mem_sum(ops, g):
    B, T, S, R = 2, 37, 16, 8
    N = -(-T // S)
    n_rc, n_mem, n_sum = ((N * R + 31) // 32) * 32, N - 1, N
    rows_x, rows_z = n_rc + T, n_mem + n_rc + T + n_sum
    x = _rn(g, B, rows_x, D)
    wts = _ffn_weights(g, 64)
    g2, b2 = (1 + 0.1 * torch.randn(D, generator=g)).cuda(), (0.1 * torch.randn(D, generator=g)).cuda()
    wq_fm, bq = ops.pack_fragment_major(_rn(g, 3 * D, D, scale=D ** -0.5)), _rn(g, 3 * D, scale=0.1, dtype=torch.float32)
    lengths = torch.tensor([T, 20], dtype=torch.int32).cuda()
    Z = torch.zeros(B, rows_z, D, device="cuda", dtype=torch.bfloat16)
    Z[:, :n_mem] = _rn(g, B, n_mem, D)
    out = torch.zeros_like(x)
    Q = torch.zeros(B * rows_z + 16, 3 * D, device="cuda", dtype=torch.bfloat16)
    kw = dict(T=T, n_mem=n_mem, n_rc=n_rc, n_sum=n_sum)
    ops.emformer_ffn_prenorm_qkv(x, *wts, out, g2, b2, lengths, Z, wq_fm, bq, Q, seg_len=S, **kw)
    ops.emformer_qkv_mem_sum(Z, wq_fm, bq, Q, **kw)
    return [out, Z, Q]


def _linear_weight_stationary(ops, g):
    x, W, b = _rn(g, 8192, D), _rn(g, D, D, scale=D ** -0.5), _rn(g, D, dtype=torch.float32)
    return [ops.linear(x, ops.pack_fragment_major(W), b, w_fragment_major=True)]


def _linear_tile256(ops, g, form):
    x, Wp, bp = _rn(g, 1, 8192, 64), _rn(g, 512, 64, scale=0.125), _rn(g, 512, dtype=torch.float32)
    ops.h.set_option(_lib.OPT_CONV_TILE256, form)
    try:
        return [ops.causal_conv1d_glu(x, Wp, bp, ksize=1, stride=1)]
    finally:
        ops.h.set_option(_lib.OPT_CONV_TILE256, 2)


def _conv_pos(ops, g):
    groups, cpg, k, T = 2, 16, 42, 70
    lengths = torch.tensor([T], dtype=torch.int32).cuda()
    outs = []
    for dtype in (torch.float32, torch.bfloat16):
        x, W = _rn(g, 1, T, groups * cpg, dtype=dtype), _rn(g, groups * cpg, cpg, k, scale=0.05, dtype=dtype)
        outs.append(ops.conv_pos(x, None, W, _rn(g, groups * cpg, dtype=torch.float32), lengths, groups))
    return outs


def _ctc_best_alignment(ops, g):
    from simulst_amd.ctc_align import best_alignment
    S, L, V = 400, 341, 12
    lp = torch.log_softmax(torch.randn(S, 1, V, generator=g), -1).cuda()
    tg = torch.randint(1, V, (1, L), generator=g)
    return list(best_alignment(lp, tg, torch.tensor([S]), torch.tensor([L]), ops=ops, return_nll=True))


def _decode_chains_at_129_rows(ops, g):
    B, F = 129, 256
    fm = lambda *s: ops.pack_fragment_major(_rn(g, *s, scale=s[1] ** -0.5))
    vec = lambda n: _rn(g, n, scale=0.1, dtype=torch.float32)
    ln = ((1 + 0.1 * torch.randn(D, generator=g)).cuda(), vec(D))
    ctx, x = _rn(g, B, D), _rn(g, B, D)
    q, _ = ops.decoder_proj_chain(ctx, x, fm(D, D), vec(D), ln, fm(D, D), vec(D))
    ops.decoder_ffn_chain(q, x, fm(D, D), vec(D), ln, fm(F, D), vec(F), fm(D, F), vec(D))
    return [q, x]


def _joiner_lattice(ops, g, dtype):
    B, S, U1, V = 1, 3, 5, 70
    P, G = _rn(g, B, S, D, dtype=torch.float32), _rn(g, B, U1, D, dtype=torch.float32)
    W_fm = ops.pack_joiner_weight(_rn(g, V, D, scale=D ** -0.5, dtype=dtype))
    labels = torch.randint(1, V, (B, U1), generator=g).to(torch.int32).cuda()
    i32 = lambda v: torch.tensor([v], dtype=torch.int32).cuda()
    return list(ops.joiner_lattice(P, G, W_fm, labels, i32(S), i32(U1 - 1), V=V))


CASES = {"emformer_ffn": _ffn, "emformer_ffn_block_form": _ffn_block_form, "emformer_ffn_prenorm_qkv+qkv_mem_sum": _ffn_prenorm_qkv_and_mem_sum,
         "linear_weight_stationary": _linear_weight_stationary, "linear_tile256_ring": lambda o, g: _linear_tile256(o, g, 2),
         "linear_tile256_staged": lambda o, g: _linear_tile256(o, g, 1), "conv_pos": _conv_pos, "ctc_best_alignment": _ctc_best_alignment,
         "decode_chains_at_129_rows": _decode_chains_at_129_rows, "joiner_lattice_fp32": lambda o, g: _joiner_lattice(o, g, torch.float32),
         "joiner_lattice_bf16": lambda o, g: _joiner_lattice(o, g, torch.bfloat16)}


@pytest.fixture(scope="module")
def ops():
    from simulst_amd.ops import Ops
    return Ops()


@pytest.mark.parametrize("name", list(CASES))
def test_first_call_on_a_fresh_handle_equals_the_shared_handle(ops, name):
    from simulst_amd.ops import Ops
    run = lambda o: CASES[name](o, torch.Generator().manual_seed(27))      # the same operands for every handle
    first, shared, second = run(Ops()), run(ops), run(Ops())               # the fresh handle goes first
    torch.cuda.synchronize()
    assert len(first) == len(shared) == len(second) > 0
    for a, b, c in zip(first, shared, second):
        assert torch.isfinite(b.float()).all() and float(b.float().abs().max()) > 0
        assert torch.equal(a, b) and torch.equal(c, b), name
