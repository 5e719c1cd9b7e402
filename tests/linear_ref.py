"""simulst_linear in float64, written from the simulst_linear_desc comment of include/simulst_hip.h and from nothing in csrc/.

reference(d, A, a0, W, bias, R, r0, gamma, beta) takes the descriptor fields under the header's names (a dict) and the RAW operand
buffers as float64 numpy arrays, a0 / r0 being the index of the element the A / R pointer of the call points at, and returns one
`stream` per output buffer ("C", and "aux" for EMF_OUT): the flat index of every element the call must write (relative to the C / aux
pointer), its expected value, and the magnitudes the bounds of tests/linear_cases.py need.  Elements it does not list must not be written.

Every rule of the header is stated here once:
  A          element (b, i, k) lies at b * a_batch_stride + i * a_row_stride + k - a_lead and reads as 0 where
             i * a_row_stride + k - a_lead < 0 (per batch: the left padding of a causal convolution); rows may overlap
  LayerNorm  prologue over the K elements of a row, eps 1e-5, biased variance; kept unrounded
  W          [N][K] row-major, or fragment-major through fragment_index()
  epilogues  0 BIAS, 1 gelu_erf(. + b), 2 . + b + R, 3 GLU (64-row blocks of W: 32 value rows then 32 gate rows; output width N / 2,
             column 32 q + j from rows 64 q + j and 64 q + 32 + j; scale * (v + b_v) * sigmoid(g + b_g)), 4 EMF_OUT (rows i < n_main of
             a batch: . + b + R to C; row n_main + s: tanh(. + b) to aux + b * aux_batch_stride + s * N for s < aux_rows, else nothing),
             5 BIAS in fp32 whatever the operands, 6 gelu_erf(. + b + R)
  C          plain: b * c_batch_stride + i * c_row_stride + c; head-major (c_head_dim): b * c_batch_stride + (c / c_head_dim) *
             c_head_stride + i * c_row_stride + c % c_head_dim; several tensors (c_tensor_heads): plane p = c / c_head_dim goes to
             (p / c_tensor_heads) * c_tensor_stride + b * c_batch_stride + (p % c_tensor_heads) * c_head_stride + i * c_row_stride +
             c % c_head_dim.  R like plain C with the r_* strides.

`mut` names one deliberate error (MUTANTS); tests/test_linear_ref_cpu.py shows that the case table sees each of them.
"""
import math

import numpy as np

F32, BF16 = 0, 1
BIAS, GELU, RES, GLU, EMF_OUT, F32OUT, RES_GELU = range(7)
LN_EPS = 1e-5

MUTANTS = ("last_k_group_dropped", "last_split_tail_dropped", "last_row_from_the_row_before", "batch_row_through_row_stride",
           "bias_shifted_on_n_tail", "residual_with_c_strides", "a_lead_minus_G", "negative_offsets_not_zeroed", "glu_value_gate_swapped",
           "glu_scale_dropped", "last_summary_kept", "tanh_from_n_main_plus_1", "head_plane_by_hd_plus_8", "tensor_and_head_stride_swapped",
           "ln_eps_1e-6", "ln_over_k_rounded_to_KS", "gelu_tanh_form")

_erf = np.vectorize(math.erf, otypes=[np.float64])


def vec_elems(dtype):
    """G: elements of a 16-byte vector"""
    return 4 if dtype == F32 else 8


def gelu64(x):
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def gelu_tanh64(x):
    return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-x))


def fragment_index(N, K, dtype):
    """[N][K] index map of the header: where element (n, k) of W lies in fragment-major storage"""
    G = vec_elems(dtype)
    KS = 4 * G
    assert N % 16 == 0 and K % KS == 0
    n, k = np.arange(N, dtype=np.int64)[:, None], np.arange(K, dtype=np.int64)[None, :]
    return ((n // 16 * (K // KS) + k // KS) * 64 + (k % KS) // G * 16 + n % 16) * G + k % G


def a_index(d, mut=None):
    """rel [rpb][K] = i * a_row_stride + k - a_lead, and the buffer offset [B][rpb][K] of every element (relative to the A pointer)"""
    B, rpb, K = d["M_batches"], d["rows_per_batch"], d["K"]
    lead = d["a_lead"] - (vec_elems(d["dtype"]) if mut == "a_lead_minus_G" else 0)
    rel = np.arange(rpb, dtype=np.int64)[:, None] * d["a_row_stride"] + np.arange(K, dtype=np.int64)[None, :] - lead
    off = np.arange(B, dtype=np.int64)[:, None, None] * d["a_batch_stride"] + rel[None]
    return rel, off


def effective_a(d, A, a0, mut=None):
    """[B * rpb][K] float64: the rows the contraction sees"""
    B, rpb, K = d["M_batches"], d["rows_per_batch"], d["K"]
    rel, off = a_index(d, mut)
    if mut == "batch_row_through_row_stride" and B > 1:      # row 0 of batch b >= 1 continues batch b - 1's rows
        off = off.copy()
        off[1:, 0, :] = off[:-1, 0, :] + rpb * d["a_row_stride"]
    if mut == "last_row_from_the_row_before" and B * rpb > 1:
        off = off.reshape(B * rpb, K).copy()
        off[-1] = off[-2]
        off = off.reshape(B, rpb, K)
        rel = rel.copy()
        if rpb > 1:
            rel[-1] = rel[-2]
    got = A[np.clip(off + a0, 0, A.size - 1)]
    if mut != "negative_offsets_not_zeroed":
        got = np.where((rel >= 0)[None], got, 0.0)
    return got.reshape(B * rpb, K)


def layer_norm64(x, gamma, beta, mut=None, dtype=BF16):
    K = x.shape[1]
    n = K
    if mut == "ln_over_k_rounded_to_KS":
        KS = 4 * vec_elems(dtype)
        n = (K + KS - 1) // KS * KS
    mean = x.sum(1, keepdims=True) / n
    var = (x * x).sum(1, keepdims=True) / n - mean * mean if n != K else ((x - mean) ** 2).sum(1, keepdims=True) / K
    zhat = (x - mean) / np.sqrt(var + (1e-6 if mut == "ln_eps_1e-6" else LN_EPS))
    return zhat * gamma[None] + beta[None], zhat


def c_index(d, rows_b, rows_i, N, mut=None):
    """[rows][N] flat offsets of the output columns of logical rows (b, i)"""
    c = np.arange(N, dtype=np.int64)[None, :]
    b, i = rows_b.astype(np.int64)[:, None], rows_i.astype(np.int64)[:, None]
    hd, th = d.get("c_head_dim", 0), d.get("c_tensor_heads", 0)
    if not hd:
        return b * d["c_batch_stride"] + i * d["c_row_stride"] + c
    p = c // (hd + 8 if mut == "head_plane_by_hd_plus_8" else hd)
    hs, ts = d["c_head_stride"], d.get("c_tensor_stride", 0)
    if not th:
        return b * d["c_batch_stride"] + p * hs + i * d["c_row_stride"] + c % hd
    if mut == "tensor_and_head_stride_swapped":
        hs, ts = ts, hs
    return (p // th) * ts + b * d["c_batch_stride"] + (p % th) * hs + i * d["c_row_stride"] + c % hd


def reference(d, A, a0, W, bias, R=None, r0=0, gamma=None, beta=None, mut=None, splits=1):
    assert mut is None or mut in MUTANTS
    B, rpb, N, K, epi, dtype = d["M_batches"], d["rows_per_batch"], d["N"], d["K"], d["epilogue"], d["dtype"]
    G = vec_elems(dtype)
    M = B * rpb
    a = effective_a(d, A, a0, mut)
    mags = {}
    if gamma is not None:
        a, zhat = layer_norm64(a, gamma, beta, mut, dtype)
        mags["ln_gz"] = np.abs(gamma)[None] * np.abs(zhat) + np.abs(beta)[None]      # [M][K]
    w = W[fragment_index(N, K, dtype).ravel()].reshape(N, K) if d.get("w_fragment_major", 0) else W[:N * K].reshape(N, K)
    a_used = a
    if mut == "last_k_group_dropped":
        a_used = a.copy()
        a_used[:, K - G:] = 0.0
    if mut == "last_split_tail_dropped" and splits > 1:          # the k of one split rounded DOWN to whole k-steps
        kps = K // splits // (4 * G) * (4 * G)
        a_used = a.copy()
        a_used[:, kps * splits:] = 0.0
    acc = a_used @ w.T
    S = np.abs(a) @ np.abs(w).T
    bv = np.zeros(N) if bias is None else bias[:N].astype(np.float64)
    if mut == "bias_shifted_on_n_tail" and bias is not None:
        bv = bv.copy()
        t0 = N // 16 * 16
        bv[t0:] = bias[np.minimum(np.arange(t0, N) + 1, bias.size - 1)]
    rows_b, rows_i = np.arange(M) // rpb, np.arange(M) % rpb
    pre = acc + bv[None]
    babs = np.broadcast_to(np.abs(bv)[None], pre.shape)
    rabs = np.zeros_like(pre)
    if epi in (RES, EMF_OUT, RES_GELU):
        rd = dict(c_batch_stride=d["c_batch_stride"], c_row_stride=d["c_row_stride"]) if mut == "residual_with_c_strides" else \
            dict(c_batch_stride=d["r_batch_stride"], c_row_stride=d["r_row_stride"])
        ridx = c_index(rd, rows_b, rows_i, N) + r0
        ok = np.ones(M, bool) if epi != EMF_OUT else rows_i < d["n_main"]
        r = np.where(ok[:, None], R[np.clip(ridx, 0, R.size - 1)], 0.0)
        pre = pre + r
        rabs = np.abs(r)
    mags.update(S=S, babs=babs, rabs=rabs, pre=pre, absw=np.abs(w), absz=np.abs(a))
    gelu = gelu_tanh64 if mut == "gelu_tanh_form" else gelu64
    streams = {}
    allr = np.arange(M)
    if epi in (BIAS, RES, F32OUT):
        streams["C"] = dict(idx=c_index(d, rows_b, rows_i, N, mut), val=pre, rows=allr, act=None)
    elif epi in (GELU, RES_GELU):
        streams["C"] = dict(idx=c_index(d, rows_b, rows_i, N, mut), val=gelu(pre), rows=allr, act="gelu")
    elif epi == GLU:
        assert N % 64 == 0
        q, j = np.arange(N // 2) // 32, np.arange(N // 2) % 32
        vrow, grow = 64 * q + j, 64 * q + 32 + j
        if mut == "glu_value_gate_swapped":
            vrow, grow = grow, vrow
        s = 1.0 if mut == "glu_scale_dropped" else float(d["scale"])
        val = s * pre[:, vrow] * sigmoid64(pre[:, grow])
        streams["C"] = dict(idx=c_index(d, rows_b, rows_i, N // 2, mut), val=val, rows=allr, act="glu", vrow=vrow, grow=grow, scale=s)
    elif epi == EMF_OUT:
        main = rows_i < d["n_main"]
        streams["C"] = dict(idx=c_index(d, rows_b[main], rows_i[main], N, mut), val=pre[main], rows=allr[main], act=None)
        s = rows_i - d["n_main"] - (1 if mut == "tanh_from_n_main_plus_1" else 0)
        keep = ~main & (s >= 0) & (s < d["aux_rows"] + (1 if mut == "last_summary_kept" else 0))
        aidx = rows_b[keep].astype(np.int64)[:, None] * d["aux_batch_stride"] + s[keep].astype(np.int64)[:, None] * N + np.arange(N)[None]
        streams["aux"] = dict(idx=aidx, val=np.tanh(pre[keep]), rows=allr[keep], act="tanh")
    else:
        raise ValueError(f"epilogue {epi} is not one of the seven this reference states")
    for st in streams.values():
        assert mut is not None or np.unique(st["idx"]).size == st["idx"].size, "two outputs at one address"
    return streams, mags
