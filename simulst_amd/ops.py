"""Tensor-level wrappers over the C ABI: validate torch-ROCm tensors, pass data_ptr()s.

PyTorch is plumbing here (device memory + the current stream); every op below
runs a hand-written HIP kernel from libsimulst_hip.so.  No fallbacks.
"""
import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import (ATTN_ENUM, BF16, EPI_BIAS, EPI_BIAS_F32OUT, EPI_BIAS_GELU, EPI_BIAS_RES, EPI_EMF_OUT,
                   EPI_GLU, F32, EmfAttnDesc, LinearDesc)

_vp = C.c_void_p


def dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"simulst_amd: unsupported dtype {t.dtype} (float32 or bfloat16)")


def _p(t: Optional[torch.Tensor]):
    if t is None:
        return _vp(0)
    if not t.is_cuda:
        raise RuntimeError("simulst_amd: tensors must live on the HIP device (no CPU fallback)")
    return _vp(t.data_ptr())


def _chk_contig(*ts):
    for t in ts:
        if t is not None and not t.is_contiguous():
            raise ValueError("simulst_amd: tensor must be contiguous")


def _row_view(who, x, W, rows_per_batch):
    """x of linear_pick / linear_topk, [rows, K] (with rows_per_batch) or a [B, T, K] view, as simulst_linear addresses it:
    -> (batches, rows per batch, K, batch stride, row stride)"""
    if x.dim() == 3:
        if rows_per_batch is not None and rows_per_batch != x.shape[1]:
            raise ValueError(f"{who}: rows_per_batch belongs to 2-D x")
        Bb, rpb, K = x.shape
        a_bs, a_rs = x.stride(0), x.stride(1)
    elif x.dim() == 2:
        rows, K = x.shape
        rpb = max(rows, 1) if rows_per_batch is None else int(rows_per_batch)
        if rpb <= 0 or rows % rpb:
            raise ValueError(f"{who}: rows_per_batch must divide the rows")
        Bb, a_rs = rows // rpb, x.stride(0)
        a_bs = rpb * a_rs
    else:
        raise ValueError(f"{who}: x is [rows, K] or [B, T, K]")
    if x.stride(-1) != 1 and x.numel():
        raise ValueError(f"{who}: the rows of x must be contiguous")
    if W.shape[1] != K or W.dtype != x.dtype:
        raise ValueError(f"{who}: W is [N, K] in x's dtype")
    return Bb, rpb, K, a_bs, a_rs


class Ops:
    """All kernels, bound to one Handle (one HIP stream)."""

    def __init__(self, handle: Optional[_lib.Handle] = None):
        self.h = handle or _lib.Handle()
        self.lib = self.h.lib

    # ------------------------------------------------------------------ dense
    def linear_raw(self, A, W, bias, C_out, *, M_batches, rows_per_batch, N, K, a_bs, a_rs, a_lead=0,
                   c_bs, c_rs, epilogue=EPI_BIAS, R=None, r_bs=0, r_rs=0, scale=1.0, n_main=0, aux=None,
                   aux_rows=0, aux_bs=0, ln=None, w_fragment_major=False, c_head_dim=0, c_head_stride=0, c_tensor_heads=0,
                   c_tensor_stride=0):
        d = LinearDesc(M_batches, rows_per_batch, N, K, a_bs, a_rs, a_lead, c_bs, c_rs, r_bs, r_rs,
                       epilogue, dt(A), scale, n_main, aux_rows, aux_bs,
                       ln[0].data_ptr() if ln is not None else None, ln[1].data_ptr() if ln is not None else None,
                       int(w_fragment_major), c_head_dim, c_head_stride, c_tensor_heads, c_tensor_stride)
        self.h.check(self.lib.simulst_linear(self.h.ptr, C.byref(d), _p(A), _p(W), _p(bias), _p(R), _p(C_out),
                                             _p(aux)), "simulst_linear")
        return C_out

    def pack_fragment_major(self, W):
        """Row-major weight [N, K] -> the MFMA-fragment order the decode-step kernels stream with 1 KB contiguous
        wave loads (simulst_linear_desc.w_fragment_major).  Returned tensor keeps the [N, K] shape (storage order
        only)."""
        _chk_contig(W)
        out = torch.empty_like(W)
        self.h.check(self.lib.simulst_pack_fragment_major(self.h.ptr, _p(W), _p(out), W.shape[0], W.shape[1], dt(W)),
                     "simulst_pack_fragment_major")
        return out

    def linear(self, x, W, bias=None, *, epilogue=EPI_BIAS, residual=None, out=None, ln=None,
               w_fragment_major=False):
        """y[rows, N] = epi(LN?(x)[rows, K] @ W[N, K]^T + bias). x 2-D contiguous. ln = (gamma, beta) fuses a
        LayerNorm prologue (decode-step shapes only)."""
        _chk_contig(x, W, residual, out)
        rows, K = x.shape
        N = W.shape[0]
        assert W.shape[1] == K
        if out is None:
            odt = torch.float32 if epilogue == EPI_BIAS_F32OUT else x.dtype
            out = torch.empty(rows, N, device=x.device, dtype=odt)
        return self.linear_raw(x, W, bias, out, M_batches=1, rows_per_batch=rows, N=N, K=K, a_bs=0, a_rs=K,
                               c_bs=0, c_rs=N, epilogue=epilogue, R=residual, r_bs=0, r_rs=N, ln=ln,
                               w_fragment_major=w_fragment_major)

    def linear_pick(self, x, W, bias=None, *, rows_per_batch=None, out=None, w_fragment_major=False):
        """Best column of every row of z = x @ W[N, K]^T + bias without the logits (simulst_linear, SIMULST_EPI_ROW_PICK):
        -> (pick int32, zmax fp32, lse fp32), each shaped like x without its last dimension; pick is the lowest column at which z is
        largest (torch.argmax's rule), zmax - lse its log-probability.

        x: [rows, K] (rows K-contiguous, any row stride) or a [B, T, K] view with a batch stride -- the encoder's output rows are read
        where they lie.  rows_per_batch (2-D x only, default all rows): the rows form rows / rows_per_batch batches, which is how `out`
        is addressed.  out: an int32 tensor (or view) [batches, rows_per_batch] to take the pick, any strides.  Runs on the handle's
        stream like every op here; CPU tensors raise."""
        _chk_contig(W)
        _p(x), _p(W)                                           # (CPU tensors raise here, whatever the row count)
        Bb, rpb, K, a_bs, a_rs = _row_view("linear_pick", x, W, rows_per_batch)
        N = W.shape[0]
        if out is None:
            out = torch.empty(Bb, rpb, device=x.device, dtype=torch.int32)
        elif out.dtype != torch.int32 or tuple(out.shape) != (Bb, rpb):
            raise ValueError("linear_pick: out is an int32 [batches, rows_per_batch] tensor")
        aux = torch.empty(Bb * rpb, 2, device=x.device, dtype=torch.float32)
        if Bb * rpb:                                           # (no rows: nothing to launch, and nothing to point at)
            self.linear_raw(x, W, bias, out, M_batches=Bb, rows_per_batch=rpb, N=N, K=K, a_bs=a_bs, a_rs=a_rs, c_bs=out.stride(0),
                            c_rs=out.stride(1), epilogue=_lib.EPI_ROW_PICK, aux=aux, w_fragment_major=w_fragment_major)
        zmax, lse = aux[:, 0].view(Bb, rpb), aux[:, 1].view(Bb, rpb)
        if x.dim() == 2 and rows_per_batch is None:
            return (out[0], zmax[0], lse[0]) if Bb else (out.reshape(0), zmax.reshape(0), lse.reshape(0))
        return out, zmax, lse

    def linear_topk(self, x, W, bias=None, *, k, keep=None, rows_per_batch=None, out=None, w_fragment_major=False):
        """The best k columns of every row of z = x @ W[N, K]^T + bias without the logits (simulst_linear, SIMULST_EPI_ROW_TOPK):
        -> (ids int32 [..., k'], lprob fp32 [..., k'], lse fp32 [...]), k' = k + (keep is not None), the leading dimensions those of x
        without its last.  keep: a column that is always reported, in slot 0 (a CTC head's blank); the other k slots hold the columns
        other than keep with the largest z, descending, on equal z the lower column first (rank 0 without keep is linear_pick's pick);
        slots past the columns that exist hold -1 and lprob -inf.  lprob = z - lse.  1 <= k <= 8.

        x, rows_per_batch and w_fragment_major as for linear_pick.  out: an int32 tensor (or view) [batches, rows_per_batch, k'] to take
        the ids, last dimension contiguous, any other strides.  CPU tensors raise."""
        _chk_contig(W)
        _p(x), _p(W)                                           # (CPU tensors raise here, whatever the row count)
        Bb, rpb, K, a_bs, a_rs = _row_view("linear_topk", x, W, rows_per_batch)
        N = W.shape[0]
        k = int(k)
        kp = k + (keep is not None)
        if out is None:
            out = torch.empty(Bb, rpb, kp, device=x.device, dtype=torch.int32)
        elif out.dtype != torch.int32 or tuple(out.shape) != (Bb, rpb, kp) or (out.stride(2) != 1 and out.numel()):
            raise ValueError("linear_topk: out is an int32 [batches, rows_per_batch, k'] tensor with a contiguous last dimension")
        aux = torch.empty(Bb * rpb, kp + 1, device=x.device, dtype=torch.float32)
        if Bb * rpb:                                           # (no rows: nothing to launch, and nothing to point at)
            self.linear_raw(x, W, bias, out, M_batches=Bb, rows_per_batch=rpb, N=N, K=K, a_bs=a_bs, a_rs=a_rs, c_bs=out.stride(0),
                            c_rs=out.stride(1), epilogue=_lib.EPI_ROW_TOPK, aux=aux, aux_rows=k, n_main=-1 if keep is None else int(keep),
                            w_fragment_major=w_fragment_major)
        lprob, lse = aux[:, :kp].view(Bb, rpb, kp), aux[:, kp].view(Bb, rpb)
        if x.dim() == 2 and rows_per_batch is None:
            return (out[0], lprob[0], lse[0]) if Bb else (out.reshape(0, kp), lprob.reshape(0, kp), lse.reshape(0))
        return out, lprob, lse

    def linear_gather(self, x, W, bias, labels, out=None):
        """Log-probabilities of given labels under z = x @ W[N, K]^T + bias without the logits (simulst_linear, SIMULST_EPI_ROW_GATHER):
        out[b, t, j] = z[b, t, labels[b, j]] - logsumexp_n z[b, t, n], fp32.

        x: [B, T, K] (rows K-contiguous, any batch and row stride -- the encoder's output rows are read where they lie); W [N, K]
        row-major in x's dtype; labels int32 [B, L'] on the device, L' >= 1, rows L'-contiguous (values outside [0, N) are clamped into
        it); out: an fp32 tensor or view [B, T, L'] whose last dimension is contiguous, any other strides (a time-major buffer viewed
        as [B, T, L'] is how ctc.ctc_rescore lays its result out); default a new contiguous one."""
        _chk_contig(W)
        _p(x), _p(W), _p(labels)
        if x.dim() != 3 or (x.stride(-1) != 1 and x.numel()):
            raise ValueError("linear_gather: x is [B, T, K] with contiguous rows")
        Bb, T, K = x.shape
        N = W.shape[0]
        if W.shape[1] != K or W.dtype != x.dtype:
            raise ValueError("linear_gather: W is [N, K] in x's dtype")
        if labels.dtype != torch.int32 or labels.dim() != 2 or labels.size(0) != Bb or labels.size(1) < 1 or labels.stride(1) != 1:
            raise ValueError("linear_gather: labels is an int32 [B, L' >= 1] tensor with contiguous rows")
        Lp = labels.size(1)
        if out is None:
            out = torch.empty(Bb, T, Lp, device=x.device, dtype=torch.float32)
        elif out.dtype != torch.float32 or tuple(out.shape) != (Bb, T, Lp) or (out.stride(2) != 1 and out.numel()):
            raise ValueError("linear_gather: out is an fp32 [B, T, L'] tensor or view with a contiguous last dimension")
        if Bb * T:
            self.linear_raw(x, W, bias, out, M_batches=Bb, rows_per_batch=T, N=N, K=K, a_bs=x.stride(0), a_rs=x.stride(1),
                            c_bs=out.stride(0), c_rs=out.stride(1), epilogue=_lib.EPI_ROW_GATHER, aux=labels, aux_rows=Lp,
                            aux_bs=labels.stride(0))
        return out

    def causal_conv1d_glu(self, x, Wp, bp, *, ksize, stride, scale=1.0, out=None):
        """Strided causal Conv1d + GLU over channel-last frames.
        x [B, T_in, C_in] whose first (ksize-1) frames are LEFT CONTEXT (zeros at utterance start,
        the cached tail when streaming); Wp [2*C_out prepacked][ksize*C_in]; output
        [B, (T_in-(ksize-1))//stride ... ] frames t_out -> input window ending at frame
        (ksize-1) + stride*t_out ... see subsampler() for the framing."""
        _chk_contig(x, Wp, out)
        B, T_in, Cin = x.shape
        N = Wp.shape[0]
        T_out = (T_in - ksize) // stride + 1
        if out is None:
            out = torch.empty(B, T_out, N // 2, device=x.device, dtype=x.dtype)
        if T_out <= 0:
            return out
        return self.linear_raw(x, Wp, bp, out, M_batches=B, rows_per_batch=T_out, N=N, K=ksize * Cin,
                               a_bs=T_in * Cin, a_rs=stride * Cin, a_lead=0, c_bs=T_out * (N // 2),
                               c_rs=N // 2, epilogue=EPI_GLU, scale=scale)

    # ------------------------------------------------------------------ row ops
    def layernorm(self, x, gamma, beta, out=None):
        _chk_contig(x, out)
        D = x.shape[-1]
        rows = x.numel() // D
        if out is None:
            out = torch.empty_like(x)
        self.h.check(self.lib.simulst_layernorm(self.h.ptr, _p(x), _p(gamma), _p(beta), _p(out), rows, D, D, D,
                                                dt(x)), "simulst_layernorm")
        return out

    def emformer_pack_rows(self, x, S, R, N):
        """x [B, T, D] -> X [B, N*R + T, D]: right-context block rows (first-layer copies), then the utterance rows."""
        _chk_contig(x)
        B, T, D = x.shape
        X = torch.empty(B, N * R + T, D, device=x.device, dtype=x.dtype)
        self.h.check(self.lib.simulst_emformer_pack_rows(self.h.ptr, _p(x), _p(X), B, T, D, S, R, N, dt(x)),
                     "simulst_emformer_pack_rows")
        return X

    def emformer_ffn(self, x, ln_g, ln_b, w1p, b1, w2p, b2, out):
        """out[rows, D] = x + fc2(gelu(fc1(LayerNorm(x)))) in one launch (simulst_emformer_ffn; bf16, D == 256)."""
        _chk_contig(x, out, w1p, w2p)
        rows, D = x.shape
        F = b1.numel()
        self.h.check(self.lib.simulst_emformer_ffn(self.h.ptr, _p(x), _p(ln_g), _p(ln_b), _p(w1p), _p(b1), _p(w2p),
                                                   _p(b2), _p(out), rows, D, F, dt(x)), "simulst_emformer_ffn")
        return out

    def emformer_ffn_prenorm(self, x, ln_g, ln_b, w1p, b1, w2p, b2, out, next_g, next_b, lengths, Z, *, T, n_mem, n_rc, n_sum, seg_len):
        """emformer_ffn over x / out [B, n_rc + T, D] + the next layer's emformer_prenorm(out, next_g, next_b, lengths, Z) in the same
        launch (simulst_emformer_ffn_prenorm)."""
        _chk_contig(x, out, w1p, w2p, Z)
        B, _, D = x.shape
        self.h.check(self.lib.simulst_emformer_ffn_prenorm(self.h.ptr, _p(x), _p(ln_g), _p(ln_b), _p(w1p), _p(b1), _p(w2p), _p(b2),
                                                           _p(out), _p(next_g), _p(next_b), _p(lengths), _p(Z), B, T, D, b1.numel(),
                                                           n_mem, n_rc, n_sum, seg_len, dt(x)), "simulst_emformer_ffn_prenorm")
        return out

    def emformer_ffn_prenorm_qkv(self, x, ln_g, ln_b, w1p, b1, w2p, b2, out, next_g, next_b, lengths, Z, wqkv_fm, bqkv, QKV, *, T, n_mem,
                                 n_rc, n_sum, seg_len):
        """emformer_ffn_prenorm + the next layer's Q | K | V rows of the rc | utterance rows (simulst_emformer_ffn_prenorm_qkv).  QKV: the
        flat [B * rows_z + 16, 768] buffer (16 spare rows); Z gets its summary rows only."""
        _chk_contig(x, out, w1p, w2p, Z, wqkv_fm, QKV)
        B, _, D = x.shape
        rows_z = n_mem + n_rc + T + n_sum
        if QKV.numel() < (B * rows_z + 16) * 3 * D:
            raise ValueError("emformer_ffn_prenorm_qkv: QKV needs 16 spare rows behind its B * rows_z")
        self.h.check(self.lib.simulst_emformer_ffn_prenorm_qkv(self.h.ptr, _p(x), _p(ln_g), _p(ln_b), _p(w1p), _p(b1), _p(w2p), _p(b2),
                                                               _p(out), _p(next_g), _p(next_b), _p(lengths), _p(Z), _p(wqkv_fm), _p(bqkv),
                                                               _p(QKV), B, T, D, b1.numel(), n_mem, n_rc, n_sum, seg_len, dt(x)),
                     "simulst_emformer_ffn_prenorm_qkv")
        return out

    def emformer_qkv_mem_sum(self, Z, wqkv_fm, bqkv, QKV, *, T, n_mem, n_rc, n_sum):
        """Q | K | V rows of the memory and summary rows of Z [B, rows_z, D] into the same rows of the flat QKV buffer
        (simulst_emformer_qkv_mem_sum): what emformer_ffn_prenorm_qkv leaves."""
        _chk_contig(Z, wqkv_fm, QKV)
        B, rows_z, D = Z.shape
        if QKV.numel() < (B * rows_z + 16) * 3 * D:
            raise ValueError("emformer_qkv_mem_sum: QKV needs 16 spare rows behind its B * rows_z")
        self.h.check(self.lib.simulst_emformer_qkv_mem_sum(self.h.ptr, _p(Z), _p(wqkv_fm), _p(bqkv), _p(QKV), B, T, D, n_mem, n_rc, n_sum,
                                                           dt(Z)), "simulst_emformer_qkv_mem_sum")
        return QKV

    def emformer_prenorm(self, X, gamma, beta, lengths, Z, *, T, n_mem, n_rc, n_sum, seg_len):
        B, _, D = X.shape
        self.h.check(self.lib.simulst_emformer_prenorm(self.h.ptr, _p(X), _p(gamma), _p(beta), _p(lengths), _p(Z),
                                                       B, T, D, n_mem, n_rc, n_sum, seg_len, dt(X)),
                     "simulst_emformer_prenorm")
        return Z

    def segment_mean(self, X, lengths, out, *, T, x_bs, o_bs, seg_len, n_out):
        B = out.shape[0]
        D = out.shape[-1]
        self.h.check(self.lib.simulst_segment_mean(self.h.ptr, _p(X), _p(lengths), _p(out), B, T, D, x_bs, o_bs,
                                                   seg_len, n_out, dt(out)), "simulst_segment_mean")
        return out

    def conv_pos(self, x, hist, W, bias, lengths, groups, out=None):
        _chk_contig(x, hist, W, out)
        B, T, D = x.shape
        k = W.shape[2]
        if out is None:
            out = torch.empty_like(x)
        self.h.check(self.lib.simulst_conv_pos(self.h.ptr, _p(x), _p(hist), _p(W), _p(bias), _p(lengths), _p(out),
                                               B, T, D, groups, k, dt(x)), "simulst_conv_pos")
        return out

    @staticmethod
    def pack_conv_pos_weight(W):
        """W [D, 16, k] (weight norm folded) -> the fragment order of simulst_conv_pos_mfma."""
        D, cpg, k = W.shape
        assert cpg == 16 and k % 2 == 0
        return W.view(D // 16, 16, 2, 8, k // 2, 2).permute(0, 4, 5, 2, 1, 3).contiguous().view(D, cpg, k)

    def conv_pos_mfma(self, x, hist, Wp, bias, lengths, groups, out=None):
        _chk_contig(x, hist, Wp, out)
        B, T, D = x.shape
        k = Wp.shape[2]
        if out is None:
            out = torch.empty_like(x)
        self.h.check(self.lib.simulst_conv_pos_mfma(self.h.ptr, _p(x), _p(hist), _p(Wp), _p(bias), _p(lengths), _p(out),
                                                    B, T, D, groups, k), "simulst_conv_pos_mfma")
        return out

    def emformer_attention(self, QKV, lengths, CTX, *, B, T, D, H, S, R, Lc, M, n_mem, n_seg, use_summary,
                           lc_k=None, lc_v=None, lc_valid=None, n_mem_valid=None):
        d = EmfAttnDesc(B, T, D, H, S, R, Lc, M, n_mem, n_seg, int(use_summary), dt(QKV))
        self.h.check(self.lib.simulst_emformer_attention(self.h.ptr, C.byref(d), _p(QKV), _p(lengths), _p(lc_k),
                                                         _p(lc_v), _p(lc_valid), _p(n_mem_valid), _p(CTX)),
                     "simulst_emformer_attention")
        return CTX

    # ------------------------------------------------------------------ scans
    def waitk_p_choose(self, BH, tgt_len, S, k, *, key_len=None, tgt_offset=0, online=False, device="cuda"):
        p = torch.empty(BH, tgt_len, S, device=device, dtype=torch.float32)
        self.h.check(self.lib.simulst_waitk_p_choose(self.h.ptr, _p(p), _p(key_len), BH, tgt_len, tgt_offset, S, k,
                                                     int(online)), "simulst_waitk_p_choose")
        return p

    def mma_step_search(self, p, head_step, *, src_len=None, mass_preservation=True, want_alpha=True):
        """p [BH,S] fp32; head_step [BH] int64 updated IN PLACE. -> head_read uint8 [BH], alpha."""
        _chk_contig(p, head_step)
        BH, S = p.shape
        head_read = torch.empty(BH, device=p.device, dtype=torch.uint8)
        alpha = torch.empty(BH, S, device=p.device, dtype=torch.float32) if want_alpha else None
        self.h.check(self.lib.simulst_mma_step_search(self.h.ptr, _p(p), _p(head_step), _p(head_read), _p(alpha),
                                                      _p(src_len), BH, S, int(mass_preservation)),
                     "simulst_mma_step_search")
        return head_read, alpha

    def expected_alignment(self, p, key_len=None, eps=1e-6, out=None):
        _chk_contig(p, out)
        BH, U, S = p.shape
        alpha = torch.empty_like(p) if out is None else out
        self.h.check(self.lib.simulst_expected_alignment(self.h.ptr, _p(p), _p(alpha), _p(key_len), BH, U, S, eps),
                     "simulst_expected_alignment")
        return alpha

    def mass_preservation(self, alpha, key_len=None):
        _chk_contig(alpha)
        BH, U, S = alpha.shape
        self.h.check(self.lib.simulst_mass_preservation(self.h.ptr, _p(alpha), _p(key_len), BH, U, S),
                     "simulst_mass_preservation")
        return alpha

    def expected_soft_attention(self, alpha, energy, key_len=None, chunk_size=None, eps=1e-10, out=None):
        _chk_contig(alpha, energy, out)
        BH, U, S = alpha.shape
        beta = torch.empty_like(alpha) if out is None else out
        self.h.check(self.lib.simulst_expected_soft_attention(self.h.ptr, _p(alpha), _p(energy), _p(beta),
                                                              _p(key_len), BH, U, S, int(chunk_size or 0), eps),
                     "simulst_expected_soft_attention")
        return beta

    def step_p_choose(self, q, Kmono, p, *, B, S_cap, H, d, ratio, incremental, attn_type, key_len=None,
                      energy_bias=0.0, waitk_k=0, tgt_idx=None, online=False, dtype=None):
        dd = dtype if dtype is not None else dt(Kmono if Kmono is not None else q)
        self.h.check(self.lib.simulst_step_p_choose(self.h.ptr, _p(q), _p(Kmono), float(energy_bias), _p(key_len),
                                                    _p(p), B, S_cap, H, d, ratio, int(incremental), attn_type,
                                                    waitk_k, _p(tgt_idx), int(online), dd),
                     "simulst_step_p_choose")
        return p

    def step_p_choose_padded(self, q, Kmono, p, key_len, *, S_pad, ratio, incremental, attn_type, energy_bias=0.0,
                             pad_threshold=0.3):
        """step probabilities with the reference's padded-batch pooling and its pad-threshold mask
        (simulst_step_p_choose_padded; modules/fixed_pre_decision.py:104-131).  Kmono [B, H, S_cap, d] must hold the
        projections of all S_pad rows of the padded encoder output."""
        B, H, S_cap, d = Kmono.shape
        self.h.check(self.lib.simulst_step_p_choose_padded(self.h.ptr, _p(q), _p(Kmono), float(energy_bias), _p(key_len), _p(p), B,
                                                           int(S_pad), S_cap, H, d, int(ratio), int(incremental), attn_type,
                                                           float(pad_threshold), dt(Kmono)), "simulst_step_p_choose_padded")
        return p

    def cif_integrate(self, x, alpha, *, beta, tail_thres, src_len=None, T_cap=None):
        _chk_contig(x, alpha)
        B, S, Cc = x.shape
        if T_cap is None:
            T_cap = int(S / beta) + 2
        out = torch.empty(B, T_cap, Cc, device=x.device, dtype=x.dtype)
        cif_len = torch.empty(B, device=x.device, dtype=torch.int32)
        delays = torch.empty(B, T_cap, device=x.device, dtype=torch.float32)
        tail_w = torch.empty(B, device=x.device, dtype=torch.float32)
        alpha_sum = torch.empty(B, device=x.device, dtype=torch.float32)
        self.h.check(self.lib.simulst_cif_integrate(self.h.ptr, _p(x), _p(alpha), _p(src_len), _p(out), _p(cif_len),
                                                    _p(delays), _p(tail_w), _p(alpha_sum), B, S, Cc, T_cap,
                                                    float(beta), float(tail_thres), dt(x)), "simulst_cif_integrate")
        return out, cif_len, delays, tail_w, alpha_sum

    def pool_keys(self, Kmono, Kpool, key_len, *, ratio, j_lo, j_hi):
        """pooled monotonic keys of the complete pre-decision windows [j_lo, j_hi) (simulst_pool_keys); Kmono [B, H, S_cap, d],
        Kpool [B, H, P_cap, d] fp32"""
        B, H, S_cap, d = Kmono.shape
        self.h.check(self.lib.simulst_pool_keys(self.h.ptr, _p(Kmono), _p(Kpool), _p(key_len), B, H, d, S_cap, Kpool.shape[2],
                                                int(ratio), int(j_lo), int(j_hi), dt(Kmono)), "simulst_pool_keys")

    def cif_stream_append(self, out, n, tail_w, acc, acc_len, prev_feat, prev_weight, *, beta, finish):
        """bookkeeping of a batched CIFLayer.infer call (simulst_cif_stream_append): append all but the withheld tail slot of
        every row to its accumulated vectors, carry the tail"""
        _chk_contig(out, acc, prev_feat)
        B, T_cap, D = out.shape
        self.h.check(self.lib.simulst_cif_stream_append(self.h.ptr, _p(out), _p(n), _p(tail_w), _p(acc), _p(acc_len),
                                                        _p(prev_feat), _p(prev_weight), B, T_cap, acc.shape[1], D,
                                                        float(beta), int(finish), dt(out)), "simulst_cif_stream_append")

    def cif_alpha_head(self, hidden, gamma, beta_ln, w, bias):
        _chk_contig(hidden, w)
        D = hidden.shape[-1]
        rows = hidden.numel() // D
        alpha = torch.empty(hidden.shape[:-1], device=hidden.device, dtype=torch.float32)
        self.h.check(self.lib.simulst_cif_alpha_head(self.h.ptr, _p(hidden), _p(gamma), _p(beta_ln), _p(w),
                                                     float(bias), _p(alpha), rows, D, dt(hidden)),
                     "simulst_cif_alpha_head")
        return alpha

    # ------------------------------------------------------------------ decoder step
    def embed_tokens(self, tokens, E, pos_table, pos_row, scale, out=None):
        B = tokens.shape[0]
        D = E.shape[1]
        if out is None:
            out = torch.empty(B, D, device=E.device, dtype=E.dtype)
        self.h.check(self.lib.simulst_embed_tokens(self.h.ptr, _p(tokens), _p(E), _p(pos_table), _p(pos_row), _p(out),
                                                   B, D, float(scale), dt(E)), "simulst_embed_tokens")
        return out

    def decoder_self_attention(self, qkv, k_cache, v_cache, n_prev, out=None):
        B, H, cap, d = k_cache.shape
        if out is None:
            out = torch.empty(B, H * d, device=qkv.device, dtype=qkv.dtype)
        self.h.check(self.lib.simulst_decoder_self_attention(self.h.ptr, _p(qkv), _p(k_cache), _p(v_cache),
                                                             _p(n_prev), _p(out), B, H, d, cap, dt(qkv)),
                     "simulst_decoder_self_attention")
        return out

    def decoder_self_attention_rows(self, qkv, k_cache, v_cache, n_prev=None, *, np_uniform=-1, row_map=None, out=None):
        """simulst_decoder_self_attention_rows: qkv [slots, 3D] -> ctx [slots, D]; np_uniform >= 0 is the host-known position of
        lockstep rows (n_prev may be None), row_map [slots] int32 names the stream row (caches, n_prev) of every slot, < 0 skips it"""
        _chk_contig(qkv, k_cache, v_cache, n_prev, row_map, out)
        _, H, cap, d = k_cache.shape
        slots = qkv.shape[0]
        if out is None:
            out = torch.empty(slots, H * d, device=qkv.device, dtype=qkv.dtype)
        self.h.check(self.lib.simulst_decoder_self_attention_rows(self.h.ptr, _p(qkv), _p(k_cache), _p(v_cache), _p(n_prev),
                                                                  int(np_uniform), _p(row_map), _p(out), slots, H, d, cap, dt(qkv)),
                     "simulst_decoder_self_attention_rows")
        return out

    def decoder_cross_attention(self, q, Kc, Vc, step, *, H, attn_type, mass_preservation, key_len=None,
                                want_beta=False, out=None):
        B, H_, S_cap, d = Vc.shape              # head-major [B, H, S_cap, head_dim]
        assert H_ == H
        D = H * d
        if out is None:
            out = torch.empty(B, D, device=Vc.device, dtype=Vc.dtype)
        beta = torch.empty(B * H, S_cap, device=Vc.device, dtype=torch.float32) if want_beta else None
        self.h.check(self.lib.simulst_decoder_cross_attention(self.h.ptr, _p(q), _p(Kc), _p(Vc), _p(step),
                                                              _p(key_len), _p(out), _p(beta), B, H, d, S_cap,
                                                              attn_type, int(mass_preservation), dt(Vc)),
                     "simulst_decoder_cross_attention")
        return out, beta

    # ------------------------------------------------------------------ whole-target (teacher-forced) pass
    def decoder_self_attention_causal(self, qkv, *, H, out=None):
        """qkv [B, U, 3D] -> ctx [B, U, D]: query u attends keys 0 .. u (simulst_decoder_self_attention_causal)"""
        _chk_contig(qkv, out)
        B, U, D3 = qkv.shape
        D = D3 // 3
        if out is None:
            out = torch.empty(B, U, D, device=qkv.device, dtype=qkv.dtype)
        self.h.check(self.lib.simulst_decoder_self_attention_causal(self.h.ptr, _p(qkv), _p(out), B, U, H, D // H, dt(qkv)),
                     "simulst_decoder_self_attention_causal")
        return out

    def mma_energy(self, q, K, *, mode, S, B=None, U=None, key_len=None, ratio=1, energy_bias=0.0, pad_threshold=0.3, waitk_k=0,
                   out=None):
        """head energies / step probabilities of every (target, source) pair (simulst_mma_energy): q [B, U, D], K [B, H, S_cap, d]
        -> [B*H, U, S] fp32.  mode ENERGY_WAITK reads neither q nor K's contents (K still gives the head geometry)."""
        _chk_contig(q, K, out)
        Bk, H, S_cap, d = K.shape
        if q is not None:
            B, U = q.shape[0], q.shape[1]
        if out is None:
            out = torch.empty(B * H, U, S, device=K.device, dtype=torch.float32)
        self.h.check(self.lib.simulst_mma_energy(self.h.ptr, _p(q), _p(K), _p(out), _p(key_len), float(energy_bias),
                                                 float(pad_threshold), B, U, int(S), S_cap, H, d, int(ratio), int(mode),
                                                 int(waitk_k), dt(K)), "simulst_mma_energy")
        return out

    def mma_softmax(self, energy, key_len, *, H):
        """in-place softmax over the valid keys of energy [B*H, U, S] (simulst_mma_softmax)"""
        _chk_contig(energy)
        BH, U, S = energy.shape
        self.h.check(self.lib.simulst_mma_softmax(self.h.ptr, _p(energy), _p(key_len), BH // H, U, S, H), "simulst_mma_softmax")
        return energy

    def mma_context(self, beta, V, out=None):
        """beta [B*H, U, S] fp32 x V [B, H, S_cap, d] -> ctx [B, U, D] (simulst_mma_context)"""
        _chk_contig(beta, V, out)
        B, H, S_cap, d = V.shape
        BH, U, S = beta.shape
        assert BH == B * H
        if out is None:
            out = torch.empty(B, U, H * d, device=V.device, dtype=V.dtype)
        self.h.check(self.lib.simulst_mma_context(self.h.ptr, _p(beta), _p(V), _p(out), B, U, S, S_cap, H, d, dt(V)),
                     "simulst_mma_context")
        return out

    def decoder_proj_chain(self, ctx, x, wo_fm, bo, ln, wq_fm, bq, q=None, wq2_fm=None, bq2=None, q2=None):
        """x <- x + Wo ctx + bo (in place);  q = Wq LN(x) + bq  (and q2 with wq2_fm) in ONE launch
        (simulst_decoder_proj_chain; bf16, D == 256, fragment-major weights)."""
        B, D = x.shape
        if q is None:
            q = torch.empty_like(x)
        if wq2_fm is not None and q2 is None:
            q2 = torch.empty_like(x)
        self.h.check(self.lib.simulst_decoder_proj_chain(self.h.ptr, _p(ctx), _p(x), _p(wo_fm), _p(bo), _p(ln[0]), _p(ln[1]),
                                                         _p(wq_fm), _p(bq), _p(q), _p(wq2_fm), _p(bq2), _p(q2), B, D, dt(x)),
                     "simulst_decoder_proj_chain")
        return q, q2

    def decoder_proj_chain_kk(self, ctx, x, wo_fm, bo, ln, wq_fm, bq, kk, q=None):
        """x <- x + Wo ctx + bo (in place);  q = gelu(Wq LN(x) + bq + kk), bq may be None: the CIF decoder's form of the
        projection chain in ONE launch (simulst_decoder_proj_chain_kk; bf16, D == 256, fragment-major weights)."""
        B, D = x.shape
        if q is None:
            q = torch.empty_like(x)
        self.h.check(self.lib.simulst_decoder_proj_chain_kk(self.h.ptr, _p(ctx), _p(x), _p(wo_fm), _p(bo), _p(ln[0]), _p(ln[1]),
                                                            _p(wq_fm), _p(bq), _p(q), _p(kk), B, D, dt(x)),
                     "simulst_decoder_proj_chain_kk")
        return q

    def decoder_attn_proj_chain(self, qkv, k_cache, v_cache, n_prev, x, wo_fm, bo, ln, wq_fm, bq, q=None, wq2_fm=None, bq2=None,
                                q2=None, kk_gelu=None, rows_per_workgroup=0, n_prev_uniform=-1):
        """self-attention over the caches [B][4][cap][64] (appending this step's k / v rows at n_prev) + x <- x + Wo ctx + bo +
        q = Wq LN(x) + bq (+ q2, or gelu(. + kk_gelu)) in ONE launch (simulst_decoder_attn_proj_chain): the same results as
        decoder_self_attention followed by decoder_proj_chain, bit for bit."""
        B, D = x.shape
        H, cap, d = k_cache.shape[1], k_cache.shape[2], k_cache.shape[3]
        if q is None:
            q = torch.empty_like(x)
        if wq2_fm is not None and q2 is None:
            q2 = torch.empty_like(x)
        if not hasattr(self.lib, "simulst_decoder_attn_proj_chain") or not _lib.has_experiments():
            raise RuntimeError("simulst_decoder_attn_proj_chain: an EXPERIMENTS build of the library only (measured slower than the two launches)")
        self.h.check(self.lib.simulst_decoder_attn_proj_chain(self.h.ptr, _p(qkv), _p(k_cache), _p(v_cache), _p(n_prev), _p(x),
                                                              _p(wo_fm), _p(bo), _p(ln[0]), _p(ln[1]), _p(wq_fm), _p(bq), _p(q),
                                                              _p(wq2_fm), _p(bq2), _p(q2), _p(kk_gelu), B, H, d, cap,
                                                              int(n_prev_uniform), rows_per_workgroup, dt(x)),
                     "simulst_decoder_attn_proj_chain")
        return q, q2

    def decoder_ffn_chain(self, ctx, x, wco_fm, bco, ln, w1_fm, b1, w2_fm, b2, partial=None, sem=None, x_mid=None):
        """x <- x' + W2 gelu(W1 LN(x') + b1) + b2 with x' = x + Wco ctx + bco, in ONE launch
        (simulst_decoder_ffn_chain; bf16, D == 256, F % 256 == 0, fragment-major weights).  With x_mid the launch stops
        at the fp32 slabs (x' in x_mid, x untouched) and decoder_slab_sum_qkv finishes the sum."""
        B, D = x.shape
        F = w1_fm.shape[0]
        if partial is None:
            partial = torch.empty(F // 256, B, D, device=x.device, dtype=torch.float32)
        if sem is None and x_mid is None:
            sem = torch.zeros((B + 15) // 16, device=x.device, dtype=torch.int32)
        self.h.check(self.lib.simulst_decoder_ffn_chain(self.h.ptr, _p(ctx), _p(x), _p(wco_fm), _p(bco), _p(ln[0]), _p(ln[1]),
                                                        _p(w1_fm), _p(b1), _p(w2_fm), _p(b2), _p(partial), _p(sem),
                                                        _p(x_mid), B, D, F, dt(x)), "simulst_decoder_ffn_chain")
        return partial

    def decoder_slab_sum_qkv(self, x_mid, x, partial, b2, ln=None, wqkv_fm=None, bqkv=None, qkv=None):
        """x <- x_mid + b2 + sum of the slabs; with wqkv_fm also qkv = Wqkv LN(x) + bqkv (simulst_decoder_slab_sum_qkv)"""
        B, D = x.shape
        F = partial.shape[0] * 256
        if wqkv_fm is not None and qkv is None:
            qkv = torch.empty(B, 3 * D, device=x.device, dtype=x.dtype)
        g, b = ln if ln is not None else (None, None)
        self.h.check(self.lib.simulst_decoder_slab_sum_qkv(self.h.ptr, _p(x_mid), _p(x), _p(partial), _p(b2), _p(g), _p(b),
                                                           _p(wqkv_fm), _p(bqkv), _p(qkv), B, D, F, dt(x)),
                     "simulst_decoder_slab_sum_qkv")
        return qkv

    def decoder_vocab_chain(self, x_mid, x, partial, b2, ln, wout_fm, V, split, skip_a=-1, skip_b=-1, row_bias=None, row_bias_col=-1,
                            pairs=None):
        """x <- x_mid + b2 + sum of the slabs; pairs[row][s] = (largest logit, its lowest column) of Wout LN(x) over the s-th of
        `split` column ranges (simulst_decoder_vocab_chain).  Returns (values [B, split] fp32, columns [B, split] int32).
        pairs: the [B, split, 2] fp32 buffer to write (default: a new one)."""
        B, D = x.shape
        F = partial.shape[0] * 256
        if pairs is None:
            pairs = torch.empty(B, split, 2, device=x.device, dtype=torch.float32)
        self.h.check(self.lib.simulst_decoder_vocab_chain(self.h.ptr, _p(x_mid), _p(x), _p(partial), _p(b2), _p(ln[0]), _p(ln[1]),
                                                          _p(wout_fm), _p(pairs), B, D, F, V, split, skip_a, skip_b, _p(row_bias),
                                                          row_bias_col, dt(x)),
                     "simulst_decoder_vocab_chain")
        return pairs[..., 0].contiguous(), pairs[..., 1].contiguous().view(torch.int32)

    def policy_cross_attention(self, qm, qs, Kmono, Ksoft, V, head_step, *, H, ratio, attn_type, key_len,
                               tgt_idx=None, energy_bias=0.0, waitk_k=0, online=False, mass_preservation=True,
                               out=None):
        B, H_, S_cap, d = V.shape               # head-major [B, H, S_cap, head_dim]
        assert H_ == H
        D = H * d
        if out is None:
            out = torch.empty(B, D, device=V.device, dtype=V.dtype)
        head_read = torch.empty(B * H, device=V.device, dtype=torch.uint8)
        self.h.check(self.lib.simulst_policy_cross_attention(
            self.h.ptr, _p(qm), _p(qs), _p(Kmono), _p(Ksoft), _p(V), float(energy_bias), _p(key_len), _p(tgt_idx),
            _p(head_step), _p(head_read), _p(out), B, H, d, S_cap, ratio, attn_type, waitk_k, int(online),
            int(mass_preservation), dt(V)), "simulst_policy_cross_attention")
        return out, head_read

    def greedy_argmax(self, logits, *, pad_idx, eos_idx, mask_eos=False, eos_bias=None, out=None):
        _chk_contig(logits)
        B, V = logits.shape
        if out is None:
            out = torch.empty(B, device=logits.device, dtype=torch.int64)
        self.h.check(self.lib.simulst_greedy_argmax(self.h.ptr, _p(logits), _p(eos_bias), _p(out), B, V, pad_idx,
                                                    eos_idx, int(mask_eos)), "simulst_greedy_argmax")
        return out

    # ------------------------------------------------------------------ transducer (csrc/transducer.hip)
    def transducer_pool(self, x, lengths, *, T_max, k):
        """AvgPool1dTBCPad (models/transducer_model.py:79-98): x [B, S_in, D] (rows contiguous, any batch stride), lengths [B] int32,
        T_max the batch's longest valid length -> (y [B, ceil(T_max / k), D], new lengths [B] int32)."""
        B, S_in, D = x.shape
        assert x.stride(2) == 1 and x.stride(1) == D
        S_out = (max(int(T_max), 1) + max(int(k), 1) - 1) // max(int(k), 1)
        y = torch.empty(B, S_out, D, device=x.device, dtype=x.dtype)
        new_len = torch.empty(B, device=x.device, dtype=torch.int32)
        self.h.check(self.lib.simulst_transducer_pool(self.h.ptr, _p(x), _p(lengths), _p(y), _p(new_len), B, S_in, D, x.stride(0),
                                                      int(T_max), int(k), dt(x)), "simulst_transducer_pool")
        return y, new_len

    def pack_joiner_weight(self, W):
        """output projection [V, D] -> simulst_pack_fragment_major of its rows padded with zeros to a multiple of 16
        ([ceil(V / 16) * 16, D]), what simulst_joiner_scan reads"""
        V, D = W.shape
        V16 = (V + 15) // 16 * 16
        Wz = W if V16 == V else torch.cat([W, torch.zeros(V16 - V, D, device=W.device, dtype=W.dtype)], 0)
        return self.pack_fragment_major(Wz.contiguous())

    @staticmethod
    def joiner_split(B, S, V, dtype):
        """column ranges of the joiner scan: enough workgroups for the chip's 256 compute units, at least 4 column tiles each"""
        rows_per_wg = 64 if dtype == torch.bfloat16 else 32
        row_wgs = max(1, (B * ((S + 15) // 16) * 16 + rows_per_wg - 1) // rows_per_wg)
        return max(1, min(64, (V + 15) // 16 // 4, (512 + row_wgs - 1) // row_wgs))

    def joiner_scan(self, P, g, W_fm, prev_emit, src_len, blank_logit, best, best_idx, *, V, blank=0):
        """simulst_joiner_scan: P [B, S, D] fp32, g [B, D] fp32, W_fm from pack_joiner_weight, prev_emit / src_len [B] int32;
        writes blank_logit [B, S], best / best_idx [B, S, n_split] at the scanned positions only."""
        _chk_contig(P, g, W_fm, prev_emit, src_len, blank_logit, best, best_idx)
        B, S, D = P.shape
        n_split = best.shape[2]
        assert P.dtype == torch.float32 and g.dtype == torch.float32 and best_idx.dtype == torch.int32
        self.h.check(self.lib.simulst_joiner_scan(self.h.ptr, _p(P), _p(g), _p(W_fm), _p(prev_emit), _p(src_len), _p(blank_logit),
                                                  _p(best), _p(best_idx), B, S, D, int(V), int(blank), n_split, dt(W_fm)),
                     "simulst_joiner_scan")

    def joiner_emit(self, P, g, blank_logit, best, best_idx, prev_emit, src_len, z, at_eos, *, V, blank=0):
        """simulst_joiner_emit: prev_emit [B] int32 updated IN PLACE, z [B, D] (model dtype) and at_eos [B] int32 written"""
        _chk_contig(P, g, blank_logit, best, best_idx, prev_emit, src_len, z, at_eos)
        B, S, D = P.shape
        self.h.check(self.lib.simulst_joiner_emit(self.h.ptr, _p(P), _p(g), _p(blank_logit), _p(best), _p(best_idx), _p(prev_emit),
                                                  _p(src_len), _p(z), _p(at_eos), B, S, D, int(V), int(blank), best.shape[2], dt(z)),
                     "simulst_joiner_emit")

    def joiner_scan_beam(self, P, g, W_fm, prev_emit, src_len, finished, blank_logit, best, best_idx, *, group, V, blank=0):
        """simulst_joiner_scan_beam: joiner_scan over R = g.shape[0] rows of which every `group` consecutive ones share a source:
        P [Bs, S, D], src_len [Bs], finished [Bs] int32 or None; g [R, D], prev_emit [R], blank_logit [R, S], best / best_idx
        [R, S, n_split]"""
        _chk_contig(P, g, W_fm, prev_emit, src_len, finished, blank_logit, best, best_idx)
        Bs, S, D = P.shape
        R = g.shape[0]
        assert P.dtype == torch.float32 and g.dtype == torch.float32 and best_idx.dtype == torch.int32
        assert group >= 1 and R == Bs * group and src_len.numel() == Bs and prev_emit.numel() == R and best.shape[:2] == (R, S)
        assert finished is None or (finished.dtype == torch.int32 and finished.numel() == Bs)
        self.h.check(self.lib.simulst_joiner_scan_beam(self.h.ptr, _p(P), _p(g), _p(W_fm), _p(prev_emit), _p(src_len), _p(finished),
                                                       _p(blank_logit), _p(best), _p(best_idx), R, int(group), S, D, int(V), int(blank),
                                                       best.shape[2], dt(W_fm)), "simulst_joiner_scan_beam")

    def joiner_emit_beam(self, P, g, blank_logit, best, best_idx, prev_emit, src_len, finished, z, at_eos, emit_log, *, group, V,
                         blank=0):
        """simulst_joiner_emit_beam: joiner_emit with joiner_scan_beam's row-to-source map; emit_log [R] int32 or None"""
        _chk_contig(P, g, blank_logit, best, best_idx, prev_emit, src_len, finished, z, at_eos, emit_log)
        Bs, S, D = P.shape
        R = g.shape[0]
        assert group >= 1 and R == Bs * group and src_len.numel() == Bs and prev_emit.numel() == R and z.shape == (R, D)
        assert at_eos.numel() == R and best.shape[:2] == (R, S) and prev_emit.dtype == torch.int32
        assert finished is None or (finished.dtype == torch.int32 and finished.numel() == Bs)
        assert emit_log is None or (emit_log.dtype == torch.int32 and emit_log.numel() == R)
        self.h.check(self.lib.simulst_joiner_emit_beam(self.h.ptr, _p(P), _p(g), _p(blank_logit), _p(best), _p(best_idx), _p(prev_emit),
                                                       _p(src_len), _p(finished), _p(z), _p(at_eos), _p(emit_log), R, int(group), S, D,
                                                       int(V), int(blank), best.shape[2], dt(z)), "simulst_joiner_emit_beam")

    def transducer_beam_reorder(self, desc, src_layers, dst_layers, prev_emit_src, prev_emit_dst, reorder, finished, result, *, block,
                                n_prev):
        """simulst_transducer_beam_reorder: desc a _lib.DecoderDesc with B (rows), D, H, n_layers, cap and dtype set; src_layers /
        dst_layers: _lib.DecLayer arrays whose k_cache / v_cache point at the two buffer sets; prev_emit_src / prev_emit_dst /
        reorder [R] int32, finished [R / block] int32 or None, result [1] int32"""
        _chk_contig(prev_emit_src, prev_emit_dst, reorder, finished, result)
        R = desc.B
        assert prev_emit_src.dtype == prev_emit_dst.dtype == reorder.dtype == result.dtype == torch.int32
        assert prev_emit_src.numel() == prev_emit_dst.numel() == reorder.numel() == R and result.numel() >= 1
        assert finished is None or (finished.dtype == torch.int32 and finished.numel() * block == R)
        self.h.check(self.lib.simulst_transducer_beam_reorder(self.h.ptr, C.byref(desc), src_layers, dst_layers, _p(prev_emit_src),
                                                              _p(prev_emit_dst), _p(reorder), _p(finished), int(block), int(n_prev),
                                                              _p(result)), "simulst_transducer_beam_reorder")

    def joiner_mask_blank(self, logits, at_eos, *, blank=0):
        _chk_contig(logits, at_eos)
        B, V = logits.shape
        assert logits.dtype == torch.float32
        self.h.check(self.lib.simulst_joiner_mask_blank(self.h.ptr, _p(logits), _p(at_eos), B, V, int(blank)),
                     "simulst_joiner_mask_blank")
        return logits

    @staticmethod
    def lattice_split(B, S, U1, V, dtype):
        """column ranges of the lattice kernel: as joiner_split, over its taller row panels (128 rows bf16, 64 rows fp32)"""
        tiles_per_wg = 8 if dtype == torch.bfloat16 else 4
        row_wgs = max(1, (B * S * ((U1 + 15) // 16) + tiles_per_wg - 1) // tiles_per_wg)
        return max(1, min(64, (V + 15) // 16 // 8, (512 + row_wgs - 1) // row_wgs))

    def joiner_lattice(self, P, G, W_fm, labels, src_len, tgt_len, *, V, blank=0, n_split=None, lp_blank=None, lp_label=None):
        """simulst_joiner_lattice: P [B, S, D] fp32, G [B, U1, D] fp32, W_fm from pack_joiner_weight, labels [B, U1] int32,
        src_len / tgt_len [B] int32 -> (lp_blank, lp_label) fp32 [B, S, U1], written at the valid cells only (new outputs are
        zero-filled).  The [B, S, U1, V] logits are never made: the only scratch is the parts' [B, S, U1, n_split, 4] floats."""
        _chk_contig(P, G, W_fm, labels, src_len, tgt_len, lp_blank, lp_label)
        B, S, D = P.shape
        U1 = G.shape[1]
        assert P.dtype == torch.float32 and G.dtype == torch.float32 and G.shape == (B, U1, D)
        assert labels.dtype == torch.int32 and labels.shape == (B, U1) and src_len.dtype == torch.int32 and tgt_len.dtype == torch.int32
        if n_split is None:
            n_split = Ops.lattice_split(B, S, U1, V, W_fm.dtype)
        if lp_blank is None:
            lp_blank = torch.zeros(B, S, U1, device=P.device, dtype=torch.float32)
        if lp_label is None:
            lp_label = torch.zeros(B, S, U1, device=P.device, dtype=torch.float32)
        assert lp_blank.shape == (B, S, U1) and lp_label.shape == (B, S, U1) and lp_blank.dtype == lp_label.dtype == torch.float32
        partials = torch.empty(B, S, U1, int(n_split), 4, device=P.device, dtype=torch.float32)
        self.h.check(self.lib.simulst_joiner_lattice(self.h.ptr, _p(P), _p(G), _p(W_fm), _p(labels), _p(src_len), _p(tgt_len),
                                                     _p(partials), _p(lp_blank), _p(lp_label), B, S, U1, D, int(V), int(blank),
                                                     int(n_split), dt(W_fm)), "simulst_joiner_lattice")
        return lp_blank, lp_label

    def rnnt_forward(self, lp_blank, lp_label, src_len, tgt_len, *, want_best=False):
        """simulst_rnnt_forward: lp_blank / lp_label [B, S, U1] fp32 -> ll [B] fp32; with want_best also (best_ll [B] fp32,
        emit [B, U1] int32: the frame of label u on the best alignment for u < tgt_len[b], -1 behind it)."""
        _chk_contig(lp_blank, lp_label, src_len, tgt_len)
        B, S, U1 = lp_blank.shape
        assert lp_blank.dtype == torch.float32 and lp_label.dtype == torch.float32 and lp_label.shape == lp_blank.shape
        assert src_len.dtype == torch.int32 and tgt_len.dtype == torch.int32
        dev = lp_blank.device
        ll = torch.empty(B, device=dev, dtype=torch.float32)
        best_ll = emit = backptr = None
        if want_best:
            best_ll = torch.empty(B, device=dev, dtype=torch.float32)
            emit = torch.full((B, U1), -1, device=dev, dtype=torch.int32)
            backptr = torch.empty(B, S, U1, device=dev, dtype=torch.uint8)
        self.h.check(self.lib.simulst_rnnt_forward(self.h.ptr, _p(lp_blank), _p(lp_label), _p(src_len), _p(tgt_len), _p(ll),
                                                   _p(best_ll), _p(emit), _p(backptr), B, S, U1), "simulst_rnnt_forward")
        return (ll, best_ll, emit) if want_best else ll

    # ------------------------------------------------------------------ error rates (csrc/edit_distance.hip)
    def edit_distance(self, ref, ref_len, hyp, hyp_len, *, ref_idx=None, hyp_idx=None, n_pairs=None, path=False, pad=-1,
                      ops_dtype=torch.int8, ref_cap=None, hyp_cap=None):
        """simulst_edit_distance: ref [Rr, >= ref_cap] / hyp [Rh, >= hyp_cap] int64 label strings (rows
        contiguous, any row stride; the same tensor may be both), ref_len [Rr] / hyp_len [Rh] int64, ref_idx / hyp_idx int32 [N] or
        None (pair p is rows p, p) -> counts int32 [N, 4] = (distance, sub, del, ins); with path also (ops [N, ref_cap + hyp_cap] in
        ops_dtype -- 0 match, 1 substitution, 2 deletion, 3 insertion, `pad` behind --, n_ops int32 [N]).  The capacities default to the
        tensors' widths, at most 1023.  No read-back."""
        for t in (ref, hyp, ref_len, hyp_len):
            if t.dtype != torch.int64:
                raise TypeError("edit_distance: strings and lengths are int64")
        for t in (ref, hyp):
            if t.dim() != 2 or (t.size(1) > 1 and t.stride(1) != 1):
                raise ValueError("edit_distance: strings are [rows, labels] with contiguous rows")
        _chk_contig(ref_len, hyp_len, ref_idx, hyp_idx)
        if ref_len.numel() != ref.size(0) or hyp_len.numel() != hyp.size(0):
            raise ValueError("edit_distance: one length per row")
        for t in (ref_idx, hyp_idx):
            if t is not None and t.dtype != torch.int32:
                raise TypeError("edit_distance: indices are int32")
        if n_pairs is None:
            n_pairs = ref_idx.numel() if ref_idx is not None else hyp_idx.numel() if hyp_idx is not None else ref.size(0)
        N = int(n_pairs)
        for t in (ref_idx, hyp_idx):
            if t is not None and t.numel() != N:
                raise ValueError("edit_distance: one index per pair")
        ref_cap = ref.size(1) if ref_cap is None else int(ref_cap)
        hyp_cap = hyp.size(1) if hyp_cap is None else int(hyp_cap)
        if ref_cap > ref.size(1) or hyp_cap > hyp.size(1):
            raise ValueError("edit_distance: a capacity above the strings' width")
        dev = ref.device
        if ref.size(1) == 0:                                       # (an empty tensor has no address to pass)
            ref = torch.zeros(max(ref.size(0), 1), 1, device=dev, dtype=torch.int64)[:ref.size(0)]
        if hyp.size(1) == 0:
            hyp = torch.zeros(max(hyp.size(0), 1), 1, device=dev, dtype=torch.int64)[:hyp.size(0)]
        counts = torch.empty(N, 4, device=dev, dtype=torch.int32)
        if N == 0:
            return (counts, torch.empty(0, max(ref_cap + hyp_cap, 1), device=dev, dtype=ops_dtype),
                    torch.empty(0, device=dev, dtype=torch.int32)) if path else counts
        d = _lib.EditDesc()
        d.hyp, d.hyp_stride_b = hyp.data_ptr(), hyp.stride(0)
        d.ref_idx = ref_idx.data_ptr() if ref_idx is not None else None
        d.hyp_idx = hyp_idx.data_ptr() if hyp_idx is not None else None
        d.n_ref, d.n_hyp, d.counts, d.pad = ref.size(0), hyp.size(0), counts.data_ptr(), int(pad)
        out = n_ops = bp = None
        if path:
            if ops_dtype not in (torch.int8, torch.int32):
                raise TypeError("edit_distance: ops are int8 or int32")
            cap = max(ref_cap + hyp_cap, 1)
            out = torch.empty(N, cap, device=dev, dtype=ops_dtype)
            n_ops = torch.empty(N, device=dev, dtype=torch.int32)
            bp = torch.empty(max(_lib.edit_bp_bytes(N, ref_cap, hyp_cap), 16), device=dev, dtype=torch.uint8)
            d.n_ops, d.bp, d.bp_bytes, d.ops_cap, d.ops_width = n_ops.data_ptr(), bp.data_ptr(), bp.numel(), cap, out.element_size()
        self.h.check(self.lib.simulst_edit_distance(self.h.ptr, _p(ref), ref.stride(0), _p(ref_len), _p(hyp_len), ref_cap, hyp_cap, N,
                                                    C.byref(d), _p(out)),
                     "simulst_edit_distance")
        return (counts, out, n_ops) if path else counts

    # ------------------------------------------------------------------ beam search (csrc/beam.hip)
    def beam_topk(self, logits, max_len, finished, cand_lp, cand_tok, *, beam, step, pad_idx, eos_idx):
        _chk_contig(logits, max_len, finished, cand_lp, cand_tok)
        R, V = logits.shape
        self.h.check(self.lib.simulst_beam_topk(self.h.ptr, _p(logits), R, V, beam, step, _p(max_len), _p(finished), pad_idx, eos_idx,
                                                _p(cand_lp), _p(cand_tok)), "simulst_beam_topk")

    def beam_select(self, cand_lp, cand_tok, max_len, *, beam, V, step, lenpen, eos_idx, cum, next_tok, reorder, bp_parent, bp_token,
                    bp_cum, fin_step, fin_row, fin_score, fin_raw, fin_count, finished, result):
        Bs, L = max_len.numel(), bp_parent.shape[0]
        self.h.check(self.lib.simulst_beam_select(self.h.ptr, _p(cand_lp), _p(cand_tok), Bs, beam, V, step, _p(max_len), L, float(lenpen),
                                                  eos_idx, _p(cum), _p(next_tok), _p(reorder), _p(bp_parent), _p(bp_token), _p(bp_cum),
                                                  _p(fin_step), _p(fin_row), _p(fin_score), _p(fin_raw), _p(fin_count), _p(finished),
                                                  _p(result)), "simulst_beam_select")

    def beam_reorder(self, desc, src_layers, dst_layers, reorder, finished, result, *, beam, n_prev):
        """desc: a _lib.DecoderDesc with B (rows), D, H, n_layers, cap and dtype set; src_layers / dst_layers: _lib.DecLayer arrays
        whose k_cache, v_cache, head_step (and head_read) point at the two buffer sets"""
        self.h.check(self.lib.simulst_beam_reorder(self.h.ptr, C.byref(desc), src_layers, dst_layers, _p(reorder), _p(finished), beam,
                                                   n_prev, _p(result)), "simulst_beam_reorder")

    def beam_backtrack(self, *, beam, nbest, bp_parent, bp_token, bp_cum, fin_step, fin_row, fin_score, fin_raw, fin_count, pad_idx,
                       eos_idx, tokens, lengths, scores, pos_scores):
        Bs, L = fin_count.numel(), bp_parent.shape[0]
        self.h.check(self.lib.simulst_beam_backtrack(self.h.ptr, Bs, beam, nbest, L, _p(bp_parent), _p(bp_token), _p(bp_cum), _p(fin_step),
                                                     _p(fin_row), _p(fin_score), _p(fin_raw), _p(fin_count), pad_idx, eos_idx,
                                                     _p(tokens), _p(lengths), _p(scores), _p(pos_scores)), "simulst_beam_backtrack")
