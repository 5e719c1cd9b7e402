/*
 * simulst_hip.h -- C ABI of libsimulst_hip.so: the MI355X (gfx950) hot path of
 * streaming speech translation (conv subsampler -> Emformer -> wait-k / MMA /
 * CIF policy + greedy decoder), drop-in behind the reference's Python surface.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer into caller-owned memory (the Python
 *    host passes torch-ROCm tensor.data_ptr()); the library owns nothing but
 *    the handle (a HIP stream + per-kernel-class event timers).
 *  - all entry points are asynchronous on the handle's stream, return
 *    0 on success, <0 for an invalid argument (SIMULST_E_*), >0 for a
 *    hipError_t; they never throw and never exit.  simulst_last_error() gives
 *    the message.  (The reference's only native precedent reports errors via
 *    TORCH_CHECK -> RuntimeError, criterion/best_alignment/best_alignment.cu:233-238;
 *    the Python binding turns a non-zero status into RuntimeError too.)
 *  - dtype: activations/weights are SIMULST_F32 or SIMULST_BF16 (one dtype per
 *    call); biases, LayerNorm affine parameters, probabilities, energies,
 *    scan outputs and logits are always fp32; indices/lengths int32 unless
 *    stated; accumulation is always fp32 and softmax is fp32 like
 *    torchaudio_models/emformer.py:143-145.
 *  - row-major everywhere; "rows" are batch-major (utterance b, then time).
 *
 * Each entry point cites the reference interface (file:line under
 * /root/reference/codebase) it replaces.  INTEGRATION.md shows the binding.
 */
#ifndef SIMULST_HIP_H
#define SIMULST_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct simulst_handle simulst_handle;

enum { SIMULST_F32 = 0, SIMULST_BF16 = 1 };

enum {
  SIMULST_OK = 0,
  SIMULST_E_NULL = -1,     /* null pointer */
  SIMULST_E_SHAPE = -2,    /* unsupported / inconsistent shape */
  SIMULST_E_DTYPE = -3,    /* unknown dtype enum */
  SIMULST_E_ARG = -4       /* other invalid argument */
};

/* GEMM epilogues (simulst_linear) */
enum {
  SIMULST_EPI_BIAS = 0,        /* C = A W^T + b                                   */
  SIMULST_EPI_BIAS_GELU = 1,   /* C = gelu_erf(A W^T + b)                         */
  SIMULST_EPI_BIAS_RES = 2,    /* C = A W^T + b + R                               */
  SIMULST_EPI_GLU = 3,         /* C[:, j] = s * (a_j + b_j) * sigmoid(g_j + bg_j), W prepacked
                                  in 64-row blocks [32 value rows | 32 gate rows]     */
  SIMULST_EPI_EMF_OUT = 4,     /* Emformer out_proj: rows < n_main of each utterance: C = . + b + R;
                                  summary rows: tanh(. + b) -> next layer's memory rows */
  SIMULST_EPI_BIAS_F32OUT = 5, /* C (always fp32) = A W^T + b   (logits, energies)  */
  SIMULST_EPI_BIAS_RES_GELU = 6, /* C = gelu_erf(A W^T + b + R)   (CIF FakeCrossAttn, models/cif_transformer.py:357-362) */
  /* (7 is skipped: it is the value the plan tests record as refused with "unknown epilogue", and stays refused) */
  SIMULST_EPI_ROW_PICK = 8,    /* z = A W^T + b in fp32 is never written: C (int32, ONE element per row at the row's C address) = the
                                  lowest column at which z is largest, aux (fp32 [M][2], logical row order) = (max z, logsumexp z).
                                  The best path of a CTC head (criterion/joint_ctc_criterion.py:92-101) and its log-probabilities,
                                  aux[r][0] - aux[r][1].  aux is required; a residual, a LayerNorm prologue, a_lead, c_head_dim and
                                  c_tensor_heads are refused (E_ARG).  Any N >= 1, W row-major (or fragment-major in bf16 with
                                  N % 16 == 0, K % 32 == 0, K <= 448).  bf16 with K % 32 == 0 and K <= 448 runs on the matrix
                                  cores (csrc/gemm_pick.hip), other shapes on the VALU.  Fewer than 128 panels of 64 rows: the columns are
                                  split over workgroups and the parts folded from the library's own scratch (no caller buffer). */
  SIMULST_EPI_ROW_GATHER = 9,  /* z as above, never written: C (fp32) [b * c_batch_stride + i * c_row_stride + j] = z[r][lab[b][j]] -
                                  logsumexp_n z[r][n] for j < aux_rows: the log-probabilities of the caller's labels, which is all a CTC
                                  recursion over a given transcript reads (F.ctc_loss of criterion/joint_ctc_criterion.py:78-90 without
                                  the [B, Te, V] logits).  aux is an INPUT here: int32 labels, lab[b][j] at aux + b * aux_batch_stride + j
                                  (device memory, so not checked on the host: a label outside [0, N) is CLAMPED into it).  Any
                                  c_batch_stride / c_row_stride (a time-major result is a choice of strides).  aux is required,
                                  aux_rows >= 1 (E_SHAPE); a residual, a LayerNorm prologue, a_lead, c_head_dim and c_tensor_heads are
                                  refused (E_ARG) as for ROW_PICK; W is row-major ONLY (w_fragment_major: E_SHAPE -- the gather reads
                                  whole rows of W by label).  Same kernels, same forms and the same column split as ROW_PICK; the
                                  gathered z runs the sweep's own instruction sequence.  (No new entry point, no descriptor field:
                                  the value was refused as unknown before, so simulst_version() stays 108.) */
  /* (10 is skipped like 7: the tests record it as refused with "unknown epilogue", and it stays refused) */
  SIMULST_EPI_ROW_TOPK = 11    /* z as above, never written: the best k = aux_rows columns of every row (1 <= k <= 8, E_SHAPE) and their
                                  log-probabilities -- the per-frame candidates of a CTC prefix beam search.  n_main = keep: a column
                                  that is always reported (the blank), or -1 for none (keep >= N or < -1: E_SHAPE); k' = k +
                                  (keep >= 0) slots a row.  C (int32, k' elements at the row's C address, b * c_batch_stride + i *
                                  c_row_stride): slot 0 = keep when given, then the k columns other than keep with the largest z,
                                  descending, on equal z the lower column first; slots past the columns that exist hold -1.  aux
                                  (fp32 [M][k' + 1], logical row order, required): z - logsumexp(z) of every slot (-inf for a -1
                                  slot), then the row's logsumexp.  Refusals, fragment-major rule, kernel classes and column split
                                  as for ROW_PICK; a column's z runs the pick sweep's instruction sequence, so the rank-0 column
                                  without keep is ROW_PICK's pick.  (No new entry point, no descriptor field, version 108.) */
};

/* monotonic attention flavours (modules/__init__.py:11-16 registry names minus the
 * _fixed_pre_decision suffix, which is the `ratio` argument), and FULL: the plain encoder-decoder attention of
 * fairseq's TransformerDecoder (the s2t_emformer model, models/s2t_emformer.py:297-379): softmax over every valid
 * key, no policy, no step search.  FULL is not a simultaneous policy: the streaming and p_choose entry points refuse it. */
enum { SIMULST_ATTN_HARD = 0, SIMULST_ATTN_INFINITE_LOOKBACK = 1, SIMULST_ATTN_WAITK = 2,
       SIMULST_ATTN_CHUNKWISE = 3, SIMULST_ATTN_FULL = 4 };

/* kernel classes for simulst_timer_* (roofline accounting in bench.py) */
enum { SIMULST_K_LINEAR = 0, SIMULST_K_LAYERNORM = 1, SIMULST_K_EMF_ATTN = 2, SIMULST_K_CONV_POS = 3,
       SIMULST_K_DEC_SELF_ATTN = 4, SIMULST_K_DEC_CROSS_ATTN = 5, SIMULST_K_SCAN = 6,
       SIMULST_K_ARGMAX = 7, SIMULST_K_MISC = 8, SIMULST_K_LINEAR_SKINNY = 9, SIMULST_K_LINEAR_TILE64 = 10,
       /* round 4: the row-local layer chains of the decode step, one class per kernel (csrc/dec_chain.hip) */
       SIMULST_K_DEC_QKV_CHAIN = 11, SIMULST_K_DEC_PROJ_CHAIN = 12, SIMULST_K_DEC_FFN_CHAIN = 13,
       SIMULST_K_DEC_ATTN_CHAIN = 14, SIMULST_K_DEC_VOCAB_CHAIN = 15,
       /* the pipelined tile of the decode step's tall GEMMs (fc2 above the feed-forward chain's rows, csrc/dec_gemm_tall.hip) */
       SIMULST_K_DEC_TALL_GEMM = 16, SIMULST_K_COUNT = 17 };

/* ---- handle ------------------------------------------------------------------ */
int simulst_create(simulst_handle** out, void* hip_stream);
int simulst_destroy(simulst_handle* h);
int simulst_set_stream(simulst_handle* h, void* hip_stream);
const char* simulst_last_error(simulst_handle* h);
int simulst_version(void);            /* 108 (round 6: simulst_emformer_ffn_prenorm_qkv + simulst_emformer_qkv_mem_sum; 107: simulst_stream_ctl grew row_map / compact_rows; 106: simulst_emformer_ffn_prenorm; 105, round 5: simulst_get_option and simulst_stream_ctl grew p_probe / step_probe / step_force / probe_P); a binding built for another value must not use the library */
/* HIP streams with a compute-unit mask (hipExtStreamCreateWithCUMask) or a priority, for hosts whose framework cannot create them.
 * cu_mask: mask_words 32-bit words; on MI355X bit i is compute unit (i / 8) of XCD (i % 8) (tools/microbench_cumask.hip), every XCD
 * must keep at least one unit; NULL / 0: no mask.  priority: 0 default, > 0 greatest, < 0 least (ignored with a mask).  Used by
 * tools/partitioned_offline.py: the encoder of the next utterances beside the decode loops of the previous ones on DISJOINT
 * compute units (the offline evaluation loop of eval/generate.py:187-209 over independent batches).  Returns 0, SIMULST_E_NULL, or the
 * positive hipError_t of the failing HIP call (these two entry points take no handle, so there is no simulst_last_error text). */
int simulst_stream_create(void** out_stream, int32_t priority, const uint32_t* cu_mask, int32_t mask_words);
int simulst_stream_destroy(void* stream);
/* per-kernel-class HIP-event timing on the handle's stream (off by default) */
int simulst_timer_enable(simulst_handle* h, int kernel_class, int on);
int simulst_timer_read(simulst_handle* h, int kernel_class, double* total_ms, int64_t* launches);
int simulst_timer_reset(simulst_handle* h);
/* hipGraph replay of simulst_mma_decode: when on (and the handle's stream is not the null stream and no
 * timer is enabled) the kernel sequence of a call is captured once and replayed whenever the call repeats
 * with identical arguments (same buffers, steps, flags) -- removes the per-launch host cost and about a
 * microsecond of dependent-kernel gap per kernel. */
int simulst_graph_enable(simulst_handle* h, int on);
/* Run-time options of a handle.  Path selection -- every alternative is a complete implementation of the same operator, the
 * parity tests run both -- and the tuning values simulst_create reads from the environment (csrc/handle.cpp).
 *   VALU_ATTENTION          1: bf16 Emformer attention through the fp32-VALU kernel instead of the MFMA one, bf16 decoder
 *                              self-attention through its workgroup kernel instead of the wave-per-head one
 *   UNFUSED_DECODE          1: simulst_mma_decode / simulst_mma_stream_steps with one launch per GEMM (no layer chains)
 *   FFN_WAVES               simulst_emformer_ffn: 0 the library's choice (43 while F <= 2048, else the block form); 43 the software-pipelined
 *                           form (4 waves, GELU behind the 32 MFMAs of a tile iteration, csrc/ffn_pipe.hip); 4 / 8 the block form (GELU
 *                           between the two products) with that many waves per workgroup -- all bit-identical.  EXPERIMENTS builds also
 *                           take 41 / 81 / 83 / 45 (GELU behind the 16 fc1 MFMAs; 8 waves; 64 rows per wave: measured slower) and
 *                           47 / 87 (round 6: the tile's LDS-DMA pieces as one burst behind the barrier -- 43 issues one per MFMA gap --
 *                           and the 8-wave form with the pieces spread)
 *   DEC_CHAIN               0: no row-local layer chains (csrc/dec_chain.hip) in the decode loops
 *   DEC_ATTN_CHAIN_MAX_ROWS EXPERIMENTS builds only (E_ARG otherwise): rows up to which self-attention rides inside the projection chain
 *   DEC_ATTN_CHAIN_ROWS     EXPERIMENTS builds only: rows per workgroup of that launch: 0 chosen from the row count, 4, 8, 16
 *   FUSED_ARGMAX            0: the decode loops write fp32 logits and pick from them (default 1: partial maxima out of the
 *                              vocabulary projection's epilogue where the shapes allow)
 *   DEC_VOCAB_CHAIN_SPLIT   workgroups per 16-row tile of the decode step's closing launch (last layer's slab sum + final LayerNorm +
 *                              vocabulary projection + partial greedy pick, simulst_decoder_vocab_chain): 0 off (reduction launch +
 *                              64 x 64 tile GEMM), 1, 2, 4, 8, 16 (halved until V is a multiple of 256 x the split)
 *   DEC_EMBED_QKV_CHAIN     0: every decode step ends with its own commit launch (default 1: in simulst_mma_decode over lockstep rows
 *                              -- n_prev_uniform >= 0, more than 128 bf16 rows -- a step's commit and the new token's embedding are the
 *                              prologue of the next step's first launch, layer 0's LayerNorm + QKV; the call's last step commits as before)
 *   PANEL_WIDE              0: simulst_linear keeps tall bias-only K = 256 projections (8192 rows and more: the encoder's QKV, the joint
 *                              cross K / V projection) on the 32-rows-per-wave row panel (default 1: 64 rows per wave, LDS-DMA weights,
 *                              csrc/gemm_panel.hip panel_wide_kernel; identical results; 2, EXPERIMENTS builds: the same with plain stores)
 *   DEC_FUSE_PROJ_CROSS     EXPERIMENTS builds only, measured slower; 1 (default 0): in simulst_mma_decode over lockstep wait-k rows with the layer chains, the
 *                              projection chain and the cross-attention of a layer run as ONE launch with two kinds of workgroups: the
 *                              attention workgroups request their K / V rows first and then wait for their row's tile of the chain
 *                              (csrc/dec_chain.hip dec_proj_cross_fused_kernel; identical results)
 *   WEIGHT_STATIONARY       0: simulst_linear keeps the encoder's tall K = 256 projections (8192 rows and more, plain row-major bf16 output:
 *                              QKV, attention out-proj with the Emformer epilogue) on the row-panel kernels (default 1: one persistent
 *                              workgroup per CU holds a 192- / 256-column slice of the packed weights in LDS, rows stream through,
 *                              csrc/gemm_wstat.hip; identical results)
 *   CONV_TILE256            0: the bf16 GLU contractions of the subsampler (8192 rows and more, width a multiple of 256) stay on the
 *                              128 x 128 tile kernel (default 1: 256 x 256 tiles, one 8-wave workgroup per CU, two LDS stages,
 *                              csrc/gemm_tile256.hip; identical results)
 *   DEC_FUSE_FFN_QKV        EXPERIMENTS builds only, measured slower; 1 (default 0): in the decode loops with the layer chains, the feed-forward
 *                              chain of layer l and the slab sum + LayerNorm + QKV projection of layer l + 1 run as ONE launch, the hand-off
 *                              a ticket counter per row tile and device-coherent (sc1) slab accesses (csrc/dec_chain.hip
 *                              dec_ffn_qkv_chain_kernel; identical results)
 *   DEC_CHAIN_ROWS32        EXPERIMENTS builds only, measured slower; 1 (default 0): the projection / feed-forward / QKV chains of the decode
 *                              loops take 32-row tiles from 256 rows on (a weight fragment serves two row tiles; the 16 MFMAs of a unit
 *                              and row tile are one asm statement, csrc/dec_chain.hip mfma_block; identical results)
 *   DEC_TALL_FFN            0: above the feed-forward chain's rows the decode loops launch fc2 + residual and LN3 + fc1 + GELU through
 *                              simulst_linear (its k-interleaved 64 x 32 tile, its split row panel); default 1: fc1 from 2560 rows on its
 *                              two-stage panel and bf16 rows with fragment-major weights take the pipelined
 *                              64 x 64 tile of csrc/dec_gemm_tall.hip (two LDS stages of the weight block, the next chunk's loads in
 *                              flight behind the MFMAs; the same k partition and summation order: identical results)
 * Returns SIMULST_E_ARG for an unknown option or a value outside its range. */
enum { SIMULST_OPT_VALU_ATTENTION = 0, SIMULST_OPT_UNFUSED_DECODE = 1, SIMULST_OPT_FFN_WAVES = 2, SIMULST_OPT_DEC_CHAIN = 3,
       SIMULST_OPT_DEC_ATTN_CHAIN_MAX_ROWS = 4, SIMULST_OPT_DEC_ATTN_CHAIN_ROWS = 5, SIMULST_OPT_FUSED_ARGMAX = 6,
       SIMULST_OPT_DEC_VOCAB_CHAIN_SPLIT = 7, SIMULST_OPT_DEC_EMBED_QKV_CHAIN = 8, SIMULST_OPT_PANEL_WIDE = 9,
       SIMULST_OPT_DEC_FUSE_PROJ_CROSS = 10, SIMULST_OPT_WEIGHT_STATIONARY = 11, SIMULST_OPT_CONV_TILE256 = 12, SIMULST_OPT_DEC_FUSE_FFN_QKV = 13, SIMULST_OPT_DEC_CHAIN_ROWS32 = 14,
       SIMULST_OPT_DEC_TALL_FFN = 15 };
int simulst_set_option(simulst_handle* h, int32_t option, int32_t value);
/* the value a handle currently runs with (simulst_create's environment overrides included) */
int simulst_get_option(simulst_handle* h, int32_t option, int32_t* value);
/* 1 in a `make EXPERIMENTS=1` build of the library (csrc/Makefile: the measured-slower kernel families and their option values), else 0 */
int simulst_has_experiments(void);

#ifdef SIMULST_DEBUG_HOOKS
/* ---- investigation hooks: compiled only by `make DEBUG_HOOKS=1` (csrc/Makefile); the shipped library does not export them ----
 * measurement hook for tools/ffn_bench.py --ablations: variant 1 runs simulst_emformer_ffn WITHOUT the GELU arithmetic, 12-15 without
 * one or both products / the GELU in the 4-wave geometry (timing ablations -- their results are not the operator's); 0 restores it */
int simulst_debug_ffn_variant(simulst_handle* h, int variant);

/* Reproducibility investigation of the row-local layer chains (tools/chain_race_probe.py):
 * simulst_debug_chain_lds_bytes sets the dynamic LDS a chain workgroup REQUESTS (0 = default; the kernels use 23 KB, a larger
 * request only keeps other LDS-holding workgroups off the compute unit).  simulst_debug_chain_probe runs the projection chain
 * (simulst_decoder_proj_chain without the second query projection) in a form that also writes, after its last contraction,
 * every value that crossed an LDS hand-off inside the launch to dbg (simulst_debug_chain_probe_bytes(B) bytes; layout in
 * csrc/dec_chain.hip); variant 0 is the production instruction sequence, 1-3 are timing variants of its barriers / LDS writes. */
int simulst_debug_chain_lds_bytes(simulst_handle* h, int32_t bytes);
/* how the chains' MFMAs get their activation fragments from LDS and how their LayerNorm reduces, a BITMASK 0..3 (default 3):
 * bit 0 set = all eight ds_read_b128 of a contraction issued first into distinct register quads (clear: one at a time into ONE quad,
 * the round-2 form); bit 1 set = the LayerNorm's wave reductions on the DPP data path (clear: ds_bpermute butterfly) */
int simulst_debug_chain_xmode(simulst_handle* h, int32_t mode);
/* dbg != NULL: every simulst_decoder_proj_chain launch of this handle ends by copying its two LDS row buffers (rows entering the
 * LayerNorm, rows leaving it; 16 x 256 bf16 each per 16-row workgroup) to dbg [ceil(B / 16)][2][16][256]; NULL switches it off */
int simulst_debug_chain_tail(simulst_handle* h, void* dbg);
int64_t simulst_debug_chain_probe_bytes(int32_t B);
int simulst_debug_chain_probe(simulst_handle* h, const void* ctx, void* x, const void* wo_fm, const float* bo,
                              const float* ln_g, const float* ln_b, const void* wq_fm, const float* bq, void* q,
                              int32_t B, int32_t variant, void* dbg);
#endif /* SIMULST_DEBUG_HOOKS */

/* ---- dense contraction ----------------------------------------------------------
 * C[r, :] = epi(A[r, :] . W^T) for logical rows r = b * rows_per_batch + i.
 * A row address  = A + b*a_batch_stride + i*a_row_stride (elements), K contiguous;
 *   elements whose offset (i*a_row_stride + k - a_lead) is negative read as 0
 *   (left zero padding of a causal convolution).  A rows may OVERLAP
 *   (a_row_stride < K): a stride-s causal Conv1d over channel-last input is this
 *   GEMM with a_row_stride = s*C_in, K = k*C_in, a_lead = (k-1)*C_in and W laid
 *   out [C_out][k][C_in].
 * C row address  = C + b*c_batch_stride + i*c_row_stride.
 * W is [N][K] (torch Linear layout). bias fp32 [N] or NULL.
 * R (residual, EPI_BIAS_RES / EMF_OUT) addressed like C with r_* strides.
 * EMF_OUT: n_main = rows per utterance that take the residual path; the remaining
 *   rows_per_batch - n_main rows are summary rows s, written tanh'ed to
 *   aux + b*aux_batch_stride + s*N for s < aux_rows (the LAST summary is dropped,
 *   torchaudio_models/emformer.py:256,828).
 * Replaces: nn.Linear / nn.Conv1d+GLU calls of modules/causal_conv.py:140-155,
 * torchaudio_models/emformer.py:111-113,164-167,209,371-378, fairseq decoder
 * projections (models/cif_transformer.py:391-537 witness). */
typedef struct {
  int32_t M_batches, rows_per_batch, N, K;
  int64_t a_batch_stride, a_row_stride, a_lead;
  int64_t c_batch_stride, c_row_stride;
  int64_t r_batch_stride, r_row_stride;
  int32_t epilogue, dtype;
  float scale;                 /* GLU output scale (embed_scale), else unused */
  int32_t n_main, aux_rows;    /* EMF_OUT; ROW_GATHER: aux_rows = labels per batch (n_main unused); ROW_TOPK: aux_rows = k, n_main = keep */
  int64_t aux_batch_stride;    /* EMF_OUT; ROW_GATHER: elements between two batches' label lists */
  const float* ln_gamma;       /* optional LayerNorm PROLOGUE: A rows are normalised (eps 1e-5, fp32 stats,   */
  const float* ln_beta;        /* rounded to the operand dtype) before the contraction; NULL = none.          */
                               /* Supported when M <= 128 and rows do not overlap (decode-step shapes).       */
  int32_t w_fragment_major;    /* W is stored in MFMA-fragment order instead of row-major [N][K] (decode-step    */
                               /* shapes only, N % 16 == 0, K % KS == 0): element (n, k) at                      */
                               /*   ((n/16 * K/KS + k/KS) * 64 + (k%KS)/G * 16 + n%16) * G + k%G,                */
                               /* G = 8 (bf16) / 4 (fp32) elements, KS = 4 G: each wave load is 1 KB contiguous. */
                               /* simulst_pack_fragment_major produces it.                                       */
  int32_t c_head_dim;          /* > 0 (bias epilogue only): HEAD-MAJOR output, column c of row (b, i) is stored at */
  int64_t c_head_stride;       /*   b*c_batch_stride + (c / c_head_dim)*c_head_stride + i*c_row_stride + c % c_head_dim */
                               /* -- how the cross-attention K / V projections land in [B][H][S_cap][head_dim].   */
  int32_t c_tensor_heads;      /* > 0 (with c_head_dim): the output columns are SEVERAL head-major tensors side by side, each   */
  int64_t c_tensor_stride;     /*   c_tensor_heads heads wide and c_tensor_stride elements apart: head plane p = c / c_head_dim */
                               /*   goes to (p / c_tensor_heads)*c_tensor_stride + b*c_batch_stride +                           */
                               /*   (p % c_tensor_heads)*c_head_stride + ...  -- the K and V projections of EVERY decoder layer */
                               /*   (models/mma_model.py: 2 x decoder_layers nn.Linear calls over the same encoder states) as   */
                               /*   ONE contraction that reads the encoder states once.                                         */
} simulst_linear_desc;

int simulst_linear(simulst_handle* h, const simulst_linear_desc* d, const void* A, const void* W,
                   const float* bias, const void* R, void* C, void* aux);
/* The decode step's tall fc2 launch on its own (csrc/dec_gemm_tall.hip; the decode loops take it above the feed-forward chain's rows,
 * SIMULST_OPT_DEC_TALL_FFN): C [B][N] = A [B][K] . W^T + bias + R, bf16, W fragment-major (simulst_pack_fragment_major), contiguous
 * 16-byte aligned operands, C may alias R.  Bit for bit what simulst_linear writes for the same operands with SIMULST_EPI_BIAS_RES; taken
 * only where that call runs its k-interleaved tile without split-K (N < 512, 256 < K < 4096, N % 16 == 0, K % 32 == 0, up to 8192
 * rows), else SIMULST_E_SHAPE. */
int simulst_dec_tall_gemm(simulst_handle* h, const void* A, const void* W, const float* bias, const void* R, void* C,
                          int32_t B, int32_t N, int32_t K, int32_t dtype);
/* ... and its fc1 launch: C [B][N] = gelu(LayerNorm(A [B][K]) . W^T + bias), K <= 256, bias (if given) 16-byte aligned.  Bit for bit what
 * simulst_linear writes with ln_gamma / ln_beta and SIMULST_EPI_BIAS_GELU; taken only where that call runs its split row panel (2560 rows
 * and more at the defaults, N >= 512), else SIMULST_E_SHAPE. */
int simulst_dec_tall_fc1(simulst_handle* h, const void* A, const void* W, const float* bias, const float* ln_g, const float* ln_b,
                         void* C, int32_t B, int32_t N, int32_t K, int32_t dtype);

/* ---- feature front-end -----------------------------------------
 * Kaldi-compatible log-mel filterbank of B waveforms: frame f of row b covers samples [160 f, 160 f + 400) of
 * wave[b * wave_stride ...] (16 kHz, 25 ms window, 10 ms shift, snip_edges), DC removal, pre-emphasis, Povey window,
 * 512-point power spectrum, n_mel triangular mel filters, log(max(e, FLT_EPSILON)).  Replaces the
 * _get_kaldi_fbank / _get_torchaudio_fbank call of OnlineFeatureExtractor.__call__ (agents/default_agent.py:66-71)
 * and DATA/data_utils.py:73-98.  Tables are caller-made, once (simulst_amd/fbank.py shows how):
 *   window [400] fp32; tw_cos / tw_sin [256] = cos / sin(2 pi k / 512);
 *   mel_lo [n_mel] first FFT bin of each filter, mel_w [n_mel][24] its weights (zero padded).
 * out [B][n_frames][n_mel] in out_dtype.  The residual-sample carry between READs stays on the host
 * (fbank.OnlineFeatureExtractor), as in the reference. */
int simulst_fbank(simulst_handle* h, const float* wave, int64_t wave_stride, const float* window, const float* tw_cos,
                  const float* tw_sin, const int32_t* mel_lo, const float* mel_w, void* out, int32_t B,
                  int32_t n_frames, int32_t n_mel, float preemphasis, int32_t out_dtype);

/* ---- causal conv front-end ------------------------------------------------------
 * conv-pos: y = x + gelu(causal grouped Conv1d(x)) then rows t >= lengths[b] zeroed.
 * x, y [B][T][D] (+ optional `hist` [B][k-1][D] = the k-1 frames before x for streaming,
 * NULL = zeros). W [D][D/groups][k] fp32/bf16 with weight-norm already folded.
 * Replaces make_conv_pos(causal=True) + the add + masked_fill of
 * models/s2t_transformer.py:114-143, models/s2t_emformer.py:140-151,208-215. */
int simulst_conv_pos(simulst_handle* h, const void* x, const void* hist, const void* W,
                     const float* bias, const int32_t* lengths, void* y,
                     int32_t B, int32_t T, int32_t D, int32_t groups, int32_t k, int32_t dtype);

/* The same operator on the matrix cores: bf16, 16 channels per group, kernel width 16 / 32 / 64.  Wp is the weight
 * prepacked ONCE into MFMA-fragment order (two taps x 16 input channels per k-step, 1 KB contiguous per wave load):
 *   Wp[((g * k/2 + s) * 64 + lane) * 8 + j] = W[g*16 + (lane & 15)][((lane >> 4) & 1) * 8 + j][2*s + (lane >> 5)]
 * for group g, k-step s < k/2, lane < 64, j < 8.  Same x / hist / lengths / y contract as simulst_conv_pos. */
int simulst_conv_pos_mfma(simulst_handle* h, const void* x, const void* hist, const void* Wp, const float* bias,
                          const int32_t* lengths, void* y, int32_t B, int32_t T, int32_t D, int32_t groups,
                          int32_t k);

/* First-layer Emformer input X [B][n_seg * R + T][D] from the encoder front-end's x [B][T][D]: the right-context block rows
 * (row (i, r) = frame (i + 1) * S + r of the utterance, zero for the last segment and past the utterance) in front of the
 * utterance rows.  Replaces F.pad(R zero frames) + Emformer._gen_right_context + the concatenation with the utterance
 * (models/s2t_emformer.py:153, torchaudio_models/emformer.py:700-709,810-818) in one pass. */
int simulst_emformer_pack_rows(simulst_handle* h, const void* x, void* X, int32_t B, int32_t T, int32_t D, int32_t seg_len,
                               int32_t right_context, int32_t n_seg, int32_t dtype);

/* The Emformer feed-forward block in ONE launch (bf16, D == 256, F % 64 == 0, F <= 4096):
 *   out[rows][D] = x + W2 . gelu(W1 . LayerNorm(x) + b1) + b2
 * with the [rows][F] hidden activations kept in registers (the accumulator tile of the first product is the operand of
 * the second).  Replaces `self.pos_ff(result) + result` of _EmformerLayer._process_attention_output /
 * _apply_post_attention_ffn (torchaudio_models/emformer.py:365-378,431-441,454-462) -- LayerNorm, Linear, GELU, Linear
 * and the residual -- i.e. the layernorm + two simulst_linear launches the encoder used before.
 * Weight images (made once on the host side, simulst_amd/encoder.py ffn_pack_w1 / ffn_pack_w2), in the fragment order of
 * v_mfma_f32_32x32x16_bf16, 64 hidden units (two 32-unit tiles) per 32 KB chunk, lane < 64, j < 8:
 *   w1_packed[(((t * 16 + s) * 64 + lane) * 8 + j] = W1[32 t + (lane & 31)][16 s + 8 (lane >> 5) + j]      t < F/32, s < 16
 *   w2_packed[((((t * 2 + s) * 8 + n) * 64 + lane) * 8 + j]
 *       = W2[32 n + (lane & 31)][32 t + 16 s + 8 (j >> 2) + 4 (lane >> 5) + (j & 3)]                        s < 2, n < 8
 * x and out must not alias (the residual rows are re-read at the end).  rows == 0 is a no-op. */
int simulst_emformer_ffn(simulst_handle* h, const void* x, const float* ln_gamma, const float* ln_beta,
                         const void* w1_packed, const float* b1, const void* w2_packed, const float* b2, void* out,
                         int64_t rows, int32_t D, int32_t F, int32_t dtype);

/* simulst_emformer_ffn over the rows of B utterances, x / out [B][n_rc + T][D], with the NEXT layer's pre-attention LayerNorm
 * (_EmformerLayer.layer_norm_input, torchaudio_models/emformer.py:431-452: feed-forward -> residual -> next layer's pre-LN) and its
 * segment summaries (:163-167; AvgPool1d(ceil_mode) of the normalised utterance rows, per utterance as simulst_emformer_prenorm) in
 * the same launch: besides out, the rc | utterance rows of z_next [B][n_mem + n_rc + T + n_sum][D] get LayerNorm(out rows; next_gamma,
 * next_beta) and its summary rows the segment means -- what simulst_emformer_prenorm(out, ...) would write; the memory rows of z_next
 * are not touched.  lengths [B] int32 (encoder frames) or NULL.  bf16, D == 256, F <= 2048 and a multiple of 64, seg_len == 16,
 * n_rc a multiple of 32 (a 32-row wave never straddles the right-context block or a segment); n_sum == 0 or ceil(T / 16). */
int simulst_emformer_ffn_prenorm(simulst_handle* h, const void* x, const float* ln_gamma, const float* ln_beta,
                                 const void* w1_packed, const float* b1, const void* w2_packed, const float* b2, void* out,
                                 const float* next_gamma, const float* next_beta, const int32_t* lengths, void* z_next,
                                 int32_t B, int32_t T, int32_t D, int32_t F, int32_t n_mem, int32_t n_rc, int32_t n_sum,
                                 int32_t seg_len, int32_t dtype);

/* ... and the next layer's fused Q | K | V projection (torchaudio_models/emformer.py:109-131: emb_to_query over rc | utterance | summary,
 * emb_to_key_value over memory | rc | utterance; here one [768][256] matrix over every row, as the layer loop's simulst_linear) of the
 * rc | utterance rows in the same launch: the normalised rows go from the epilogue's registers straight into the product and never
 * reach HBM.  Rows [n_mem, n_mem + n_rc + T) of every utterance of qkv_next [B * (n_mem + n_rc + T + n_sum) + 16][768] are written
 * exactly as simulst_linear(z_next, wqkv, bqkv) would write them (same instruction, k order, bias add and rounding: bit for bit); the
 * 16 spare rows behind the buffer take the stores of a workgroup's rows past its utterance's end.  z_next gets its summary rows
 * only (its rc | utterance rows are NOT written); the Q | K | V rows of its memory and summary rows: simulst_emformer_qkv_mem_sum.
 * wqkv_fm: simulst_pack_fragment_major of the [768][256] weight; bqkv [768] fp32.  Shape limits as simulst_emformer_ffn_prenorm. */
int simulst_emformer_ffn_prenorm_qkv(simulst_handle* h, const void* x, const float* ln_gamma, const float* ln_beta,
                                     const void* w1_packed, const float* b1, const void* w2_packed, const float* b2, void* out,
                                     const float* next_gamma, const float* next_beta, const int32_t* lengths, void* z_next,
                                     const void* wqkv_fm, const float* bqkv, void* qkv_next,
                                     int32_t B, int32_t T, int32_t D, int32_t F, int32_t n_mem, int32_t n_rc, int32_t n_sum,
                                     int32_t seg_len, int32_t dtype);

/* The rest of that layer's Q | K | V buffer: the memory rows [0, n_mem) and the summary rows [n_mem + n_rc + T, + n_sum) of every
 * utterance of z [B][n_mem + n_rc + T + n_sum][256] (memory rows: the previous layer's out-projection; summary rows:
 * simulst_emformer_ffn_prenorm_qkv) through the same product -- the rows simulst_linear(z, wqkv, bqkv) would write, bit for bit --
 * into the same rows of qkv [B * rows_z + 16][768] (the 16 spare rows as above).  One launch, one wave per 32 such rows. */
int simulst_emformer_qkv_mem_sum(simulst_handle* h, const void* z, const void* wqkv_fm, const float* bqkv, void* qkv,
                                 int32_t B, int32_t T, int32_t D, int32_t n_mem, int32_t n_rc, int32_t n_sum, int32_t dtype);

/* ---- Emformer layer pieces ------------------------------------------------------
 * Per-utterance row blocks of a layer buffer Z [B][n_mem + n_rc + T + n_sum][D]:
 *   [memory rows | right-context block rows | utterance rows | summary rows].
 * simulst_emformer_prenorm: LayerNorm rows of X [B][n_rc+T][D] into Z's rc|utt rows and
 * write per-segment means of the normed utterance rows (AvgPool1d ceil_mode: a ragged last
 * segment divides by its real frame count) into Z's summary rows.  `seg_len` = S.
 * valid utterance frames of b = lengths[b] (NULL = T).
 * Replaces _apply_pre_attention_layer_norm + memory_op (torchaudio_models/emformer.py:443-452,
 * 368,472,497-498). */
int simulst_emformer_prenorm(simulst_handle* h, const void* X, const float* gamma, const float* beta,
                             const int32_t* lengths, void* Z, int32_t B, int32_t T, int32_t D,
                             int32_t n_mem, int32_t n_rc, int32_t n_sum, int32_t seg_len, int32_t dtype);

/* Plain row LayerNorm: Y[r] = LN(X[r]) (final_layer_norm, pos_ff.0, decoder norms). */
int simulst_layernorm(simulst_handle* h, const void* X, const float* gamma, const float* beta, void* Y,
                      int64_t rows, int32_t D, int64_t x_row_stride, int64_t y_row_stride, int32_t dtype);

/* Segment means of RAW utterance rows -> first-layer memory (Emformer.forward mems,
 * torchaudio_models/emformer.py:827-831; Emformer.infer mems :878-882). out [B][n_out][D]. */
int simulst_segment_mean(simulst_handle* h, const void* X, const int32_t* lengths, void* out,
                         int32_t B, int32_t T, int32_t D, int64_t x_batch_stride, int64_t out_batch_stride,
                         int32_t seg_len, int32_t n_out, int32_t dtype);

/* Block attention of one Emformer layer, all segments of all utterances in one launch.
 * QKV [B][n_mem+n_rc+T+n_sum][3D] = (q|k|v) projections of Z rows.  For segment i of b:
 *   queries: rc block i (R rows), utterance rows [iS, min((i+1)S, T)), summary i
 *   keys   : memory [max(0,i-M), i) (hidden from the summary query), rc block i,
 *            cached left-context K/V (streaming only), utterance [max(0,iS-Lc), min((i+1)S, len_b))
 * CTX [B][n_rc+T+n_sum][D] receives softmax(QK^T/sqrt(d))V per head.
 * Streaming (lc_k != NULL): n_seg == 1, memory rows come from the carried bank
 * (n_mem_valid[b] newest rows valid), lc_k/lc_v [B][Lc][D] ring of the last Lc projected
 * utterance rows of which lc_valid[b] are valid (oldest first).
 * Replaces _EmformerAttention._forward_impl/_gen_attention_probs + the mask of
 * Emformer._gen_attention_mask (torchaudio_models/emformer.py:127-219,259-318,711-793).
 * Any S, R, Lc, M is accepted (head_dim <= 64).  With nk_max = (use_summary ? M : 0) + R + Lc + S and
 * nq_max = R + S + use_summary, three kernel classes serve a call:
 *   one-tile MFMA : bf16, head_dim 64, nq_max <= 32, nk_max <= 64 (P rounded to bf16 once, fp32 denominator)
 *   VALU          : every other call with nk_max <= 128: all keys of a segment in LDS, one or two per lane, fp32 throughout
 *   blocked       : nk_max > 128: the key list walked in blocks under an online softmax -- bf16 at head_dim 64 on the
 *                   matrix cores (query blocks of 32 x key blocks of 64, same roundings as the one-tile MFMA kernel), everything
 *                   else in the VALU scheme over key blocks of 128; no bound on nk_max or nq_max.  Its only limit:
 *                   one utterance's QKV block must stay below 2^31 elements (32-bit row offsets), SIMULST_E_SHAPE otherwise.
 * SIMULST_OPT_VALU_ATTENTION routes bf16 calls to the VALU scheme in every class. */
typedef struct {
  int32_t B, T, D, H, S, R, Lc, M;
  int32_t n_mem, n_seg;         /* rows in the memory block, segments (= rc blocks = summaries) */
  int32_t use_summary;          /* 0 when max_memory_size == 0 */
  int32_t dtype;
} simulst_emf_attn_desc;

int simulst_emformer_attention(simulst_handle* h, const simulst_emf_attn_desc* d, const void* QKV,
                               const int32_t* lengths, const void* lc_k, const void* lc_v,
                               const int32_t* lc_valid, const int32_t* n_mem_valid, void* CTX);

/* ---- monotonic policies (scans) -------------------------------------------------
 * wait-k step probability: p[bh][t][s] = (s == min(t0 + t + k - 1, online ? inf : key_len[bh]-1)).
 * Replaces utils/p_choose_strategy.py:6-53. p fp32 {0,1}. key_len NULL = S. */
int simulst_waitk_p_choose(simulst_handle* h, float* p, const int32_t* key_len, int32_t BH,
                           int32_t tgt_len, int32_t tgt_offset, int32_t S, int32_t k, int32_t online);

/* Inference step search: for each row bh, zero p below head_step, force 1 at the last
 * allowed step, take the FIRST index with p >= 0.5.
 * in : p [BH][S] fp32, head_step [BH] int64 (in/out), src_len [BH] int32 or NULL (= S)
 * out: head_read [BH] uint8, alpha [BH][S] fp32 one-hot (may be NULL).
 * An EMPTY source (src_len[bh] == 0; the reference cannot run one, its search indexes position -1): no probability is read,
 * head_step = 0, head_read = !mass_preservation (the forced stop at index len = 0), alpha all zero.
 * Replaces modules/monotonic_multihead_attention.py:196-275. */
int simulst_mma_step_search(simulst_handle* h, const float* p, int64_t* head_step, uint8_t* head_read,
                            float* alpha, const int32_t* src_len, int32_t BH, int32_t S,
                            int32_t mass_preservation);

/* Expected alignment (train-mode forward): alpha [BH][U][S] from p_choose [BH][U][S], fp32,
 * key padding via key_len [BH] (NULL = S): log-space exclusive cumprod along S, recurrence along U.
 * Replaces utils/monotonic_attention.py:12-76 + utils/functions.py:20-66. */
int simulst_expected_alignment(simulst_handle* h, const float* p, float* alpha, const int32_t* key_len,
                               int32_t BH, int32_t U, int32_t S, float eps);

/* alpha += residual mass on the last valid key (in place). utils/monotonic_attention.py:155-197. */
int simulst_mass_preservation(simulst_handle* h, float* alpha, const int32_t* key_len,
                              int32_t BH, int32_t U, int32_t S);

/* Expected delays of an expected alignment: out[r] = sum_j (j + 1) * alpha[r][j], alpha [rows][S] fp32
 * (rows = batch * layers * heads * target steps).  Replaces the `steps * alpha_all` reduction of
 * criterion/mma_criterion.py:147-156 (MMACriterion.compute_latency_loss). */
int simulst_expected_delays(simulst_handle* h, const float* alpha, float* out, int64_t rows, int32_t S);

/* Latency metric of every row of delays [B][T] (fp32, source steps): metric = SIMULST_LATENCY_AL (Average Lagging),
 * _AP (Average Proportion) or _DAL (Differentiable Average Lagging); src_len / tgt_len [B] fp32;
 * target_padding_mask [B][T] bytes or NULL (then tgt_len must hold T).  Replaces the
 * simuleval.metrics.latency.{AverageLagging, AverageProportion, DifferentiableAverageLagging} calls at
 * criterion/mma_criterion.py:171-176 and criterion/cif_criterion.py:210-215 (SimulEval itself is external). */
enum { SIMULST_LATENCY_AL = 0, SIMULST_LATENCY_AP = 1, SIMULST_LATENCY_DAL = 2 };
int simulst_latency_metric(simulst_handle* h, const float* delays, const float* src_len, const float* tgt_len,
                           const uint8_t* target_padding_mask, float* out, int32_t B, int32_t T, int32_t metric);

/* ---- gradients of the training-mode scans and latency reductions (the criteria back-propagate through
 * them, criterion/mma_criterion.py:138-207 -> modules/monotonic_multihead_attention.py:301-352 ->
 * utils/monotonic_attention.py:12-76).  All fp32; same shapes as the forward entry points.
 * simulst_expected_alignment_backward: grad_p = d L / d p_choose given grad_alpha = d L / d alpha and the SAVED p / alpha of
 *   simulst_expected_alignment (one wave per row, targets in reverse, two reverse wavefront scans per target; the clamps
 *   pass the gradient inside their closed ranges like torch.clamp).  Padded source positions (>= key_len) get 0.
 * simulst_expected_delays_backward: grad_alpha[r][j] = grad_out[r] * (j + 1).
 * simulst_latency_metric_backward: grad_delays[b][i] = grad_out[b] * d metric / d delays[b][i]; the cut-off of
 *   AverageLagging and the padding are constants of the row, DifferentiableAverageLagging routes through its running
 *   maximum. */
int simulst_expected_alignment_backward(simulst_handle* h, const float* p, const float* alpha, const float* grad_alpha,
                                        float* grad_p, const int32_t* key_len, int32_t BH, int32_t U, int32_t S,
                                        float eps);
int simulst_expected_delays_backward(simulst_handle* h, const float* grad_out, float* grad_alpha, int64_t rows, int32_t S);
int simulst_latency_metric_backward(simulst_handle* h, const float* delays, const float* src_len, const float* tgt_len,
                                    const uint8_t* target_padding_mask, const float* grad_out, float* grad_delays,
                                    int32_t B, int32_t T, int32_t metric);

/* Expected soft attention beta from alpha and soft energy; chunk_size <= 0 = infinite lookback.
 * utils/monotonic_attention.py:79-152 (+ moving_sum utils/functions.py:69-125). */
int simulst_expected_soft_attention(simulst_handle* h, const float* alpha, const float* energy,
                                    float* beta, const int32_t* key_len, int32_t BH, int32_t U,
                                    int32_t S, int32_t chunk_size, float eps);

/* Step probabilities for ONE decode step of every utterance, with fixed pre-decision:
 * p [B*H][S_cap] fp32 (zero beyond key_len[b]; an empty source, key_len[b] == 0, has a zero row).
 *   q     [B][D]  monotonic-energy query = q_proj(x) (1/sqrt(d) scaling applied inside)
 *   Kmono [B][H][S_cap][head_dim] (HEAD-MAJOR) = k_proj(encoder states), cached by the caller as the source grows
 *         (simulst_linear with c_head_dim writes it in this order).
 *   Pooled key j = mean of Kmono frames [j*ratio, min((j+1)*ratio, len)): AvgPool1d(ceil_mode)
 *   commutes with the affine k_proj, so pool -> k_proj of the reference
 *   (modules/fixed_pre_decision.py:97-121) equals k_proj -> pool up to fp32 rounding; the pooled
 *   count is floor-trimmed when `incremental` (:123-131); p_j = sigmoid(q.k_j/sqrt(d) + energy_bias)
 *   (monotonic_multihead_attention.py:88-149, utils/p_choose_strategy.py:56-76, eval mode) is
 *   upsampled by zero insertion to frame (j+1)*ratio-1, cropped/padded to len with the last
 *   column overwritten when cropped (:85-95,143-159).  ratio == 1 = no pre-decision.
 *   A NEGATIVE ratio selects --fixed-pre-decision-type last with ratio |ratio| (:38-52): pooled key j is the single
 *   frame (j+1)*|ratio| - 1 (the last frame for a ragged final window of a training-mode forward); while
 *   len < |ratio| the reference leaves the keys unpooled (:38-40) and its floor-trim drops one, so there are
 *   max(1, len - 1) pooled positions, position j = frame j.  The same sign convention holds for the `ratio` of
 *   simulst_policy_cross_attention and of simulst_decoder_desc.
 *   WAITK: p_j = (j == min(tgt_idx[b] + k - 1, online ? inf : P-1)) (p_choose_strategy.py:6-53),
 *   q/Kmono unused.
 * Per-utterance (B == 1) semantics for ragged batches: windows never mix padded frames. */
int simulst_step_p_choose(simulst_handle* h, const void* q, const void* Kmono, float energy_bias,
                          const int32_t* key_len, float* p, int32_t B, int32_t S_cap, int32_t H, int32_t d,
                          int32_t ratio, int32_t incremental, int32_t attn_type, int32_t waitk_k,
                          const int32_t* tgt_idx, int32_t online, int32_t dtype);

/* The same step probabilities with the reference's PADDED-BATCH pooling (modules/fixed_pre_decision.py:104-131), for learned
 * policies: Kmono holds the projections of ALL S_pad rows of the padded encoder output of every utterance (rows beyond
 * key_len[b] included); the S_pad rows are pooled, floor-trimmed (`incremental`) and cropped as one tensor, so the window that
 * straddles the end of a shorter utterance averages valid and padded rows, and a pooled position j > 0 whose window holds more
 * than pad_threshold (--fixed-pre-decision-pad-threshold, default 0.3) padding is masked (p = 0, :112-121); p [B*H][S_cap] is
 * written for columns < S_pad.  At INFERENCE (incremental) the two forms agree on every column < key_len[b] -- the straddling
 * window's value lands on frame (j + 1) * ratio - 1 >= key_len[b], beyond the forced stop -- which is why the decode loop keeps the
 * per-utterance form; in a training-mode forward (incremental == 0) they differ at column key_len[b] - 1. */
int simulst_step_p_choose_padded(simulst_handle* h, const void* q, const void* Kmono, float energy_bias,
                                 const int32_t* key_len, float* p, int32_t B, int32_t S_pad, int32_t S_cap, int32_t H,
                                 int32_t d, int32_t ratio, int32_t incremental, int32_t attn_type, float pad_threshold,
                                 int32_t dtype);

/* ---- CIF integrate-and-fire -------------------------------------------------------
 * x [B][S][C], alpha [B][S] fp32 -> out [B][T_cap][C] (zero beyond cif_len), cif_len [B] int32,
 * delays [B][T_cap] fp32, tail_w [B] fp32, alpha_sum [B] fp32.  One wavefront prefix-sum of
 * alpha per utterance, fire index floor(csum/beta), segmented weighted sum.
 * Replaces torch_cif.cif_function as called from models/cif_transformer.py:171-178,228-233
 * (inference form: no target_lengths).
 * src_len [B] or NULL (every row S frames): row b integrates its first min(src_len[b], S) frames; x and alpha at or beyond
 * src_len[b] are never read, so padded rows may hold anything, NaN included.
 * T_cap below a row's slot count: the slots below T_cap are written as usual, nothing is written outside out / delays, and
 * cif_len[b] still reports the row's TRUE count -- cif_len[b] > T_cap is how a caller detects the overflow.
 * A total that is an exact multiple of beta (0 included) with tail_thres == 0 has a tail of weight 0 >= 0: the tail slot is
 * 0 * (beta / 0) = NaN, as in cif_function.
 * SIMULST_E_SHAPE: C % 4 != 0, beta <= 0, or more than 64 KB of LDS (4 S + T_cap + 1 floats). */
int simulst_cif_integrate(simulst_handle* h, const void* x, const float* alpha, const int32_t* src_len,
                          void* out, int32_t* cif_len, float* delays, float* tail_w, float* alpha_sum,
                          int32_t B, int32_t S, int32_t C, int32_t T_cap, float beta, float tail_thres,
                          int32_t dtype);

/* CIF weight head: alpha[r] = sigmoid(w . gelu(LayerNorm(hidden[r])) + bias), hidden = output of
 * the causal ConvTBC (itself a simulst_linear with overlapping rows).
 * Replaces CIFLayer.alpha_proj[1:] + sigmoid (models/cif_transformer.py:124-130,160,211). */
int simulst_cif_alpha_head(simulst_handle* h, const void* hidden, const float* gamma, const float* beta_ln,
                           const void* w, float bias, float* alpha, int64_t rows, int32_t D, int32_t dtype);

/* ---- decoder step ---------------------------------------------------------------
 * token embedding * sqrt(D) + sinusoidal position row (padding_idx + n_prev) -> x [B][D].
 * Replaces MMADecoder.pre_attention (models/mma_model.py:79-124). pos_table fp32 [rows][D]. */
int simulst_embed_tokens(simulst_handle* h, const int64_t* tokens, const void* E, const float* pos_table,
                         const int32_t* pos_row, void* x, int32_t B, int32_t D, float scale, int32_t dtype);

/* Incremental self-attention: append this step's k,v (from qkv [B][3D]) at row n_prev[b] of the
 * caches [B][H][cap][d], attend over n_prev[b]+1 keys. ctx [B][D].
 * Replaces fairseq MultiheadAttention incremental self-attention + prev_key/prev_value cache
 * (pruned at models/mma_model.py:34-54: a READ simply does not advance n_prev). */
int simulst_decoder_self_attention(simulst_handle* h, const void* qkv, void* k_cache, void* v_cache,
                                   const int32_t* n_prev, void* ctx, int32_t B, int32_t H, int32_t d,
                                   int32_t cap, int32_t dtype);

/* The same operation in the launch forms of the device-resident decode loops; simulst_decoder_self_attention is this call with
 * np_uniform = -1 and row_map = NULL.
 *   np_uniform >= 0: the host-known position of lockstep rows, used for every row in place of n_prev[] (which may then be NULL);
 *                    np_uniform >= cap is refused (SIMULST_E_SHAPE).  np_uniform < 0: n_prev[] is read, and must not be NULL.
 *   row_map (optional, [slots] int32, active-row compaction): slot i reads qkv row i and writes ctx row i, and uses the caches and
 *                    n_prev[] of STREAM row row_map[i]; a negative entry leaves ctx row i and every cache untouched.  The caches hold
 *                    at least max(row_map) + 1 stream rows.  A row map never names a stream row twice: two slots would append to and
 *                    read the same cache row in one launch (a race) -- that is the caller's contract, nothing checks it.
 * n_prev[b] < cap is the caller's contract as well (the kernels do not check the device array).
 * Rounding points in both forms and every kernel behind them: scores (q scaled by head_dim^-0.5), softmax and P.V in fp32 -- the
 * probabilities are NOT rounded -- and one rounding to the activation dtype at the store. */
int simulst_decoder_self_attention_rows(simulst_handle* h, const void* qkv, void* k_cache, void* v_cache,
                                        const int32_t* n_prev, int32_t np_uniform, const int32_t* row_map, void* ctx,
                                        int32_t slots, int32_t H, int32_t d, int32_t cap, int32_t dtype);

/* Monotonic cross-attention value aggregation for one decode step.
 * q [B][D] (soft-energy query = q_proj(x), the 1/sqrt(d) scaling is applied inside), Kc/Vc [B][H][S_cap][head_dim] (head-major) cached
 * projections of the encoder states, step [B*H] int64 = head_step after the search.
 *   HARD : ctx = Vc[clamp(step)] (zero if !mass_preservation && step == len)
 *   soft : ctx = softmax_{s <= step}(q.Kc[s]) Vc, zero if step == 0  (CHUNKWISE == INFINITE_LOOKBACK at
 *          inference: the reference's inference softmax ignores the chunk size, :278-293)
 *   FULL : ctx = softmax_{s < key_len[b]}(q.Kc[s]) Vc (a 1-row source attends to its one key); `step` is not read
 *          and may be NULL, beta (if given) holds the softmax weights
 * An EMPTY source (key_len[b] == 0): the ctx row (and beta) is zero for every attention type and no row of Kc / Vc is loaded.
 * Replaces modules/monotonic_multihead_attention.py:278-297,401-409. */
int simulst_decoder_cross_attention(simulst_handle* h, const void* q, const void* Kc, const void* Vc,
                                    const int64_t* step, const int32_t* key_len, void* ctx, float* beta,
                                    int32_t B, int32_t H, int32_t d, int32_t S_cap, int32_t attn_type,
                                    int32_t mass_preservation, int32_t dtype);

/* Greedy pick: argmax over fp32 logits [B][V] of log_softmax (== argmax of logits), with
 * optional -inf at pad, optional -inf at eos, optional additive eos bias per row (CIF overshoot,
 * models/cif_transformer.py:716-722). Ties resolve to the LOWEST index like torch.argmax.
 * Replaces default_agent.predict (agents/default_agent.py:415-424). */
int simulst_greedy_argmax(simulst_handle* h, const float* logits, const float* eos_bias, int64_t* out,
                          int32_t B, int32_t V, int32_t pad_idx, int32_t eos_idx, int32_t mask_eos);

/* Reorder a row-major weight matrix W [N][K] (device) into the fragment-major order described at
 * simulst_linear_desc.w_fragment_major; out has N*K elements.  One-off, at model load. */
int simulst_pack_fragment_major(simulst_handle* h, const void* W, void* out, int32_t N, int32_t K, int32_t dtype);

/* ---- CTC best alignment ----------------------------------------
 * Maximum-probability CTC state sequence of each utterance given log-probabilities and its target labels: the
 * reference's CUDA kernel (criterion/best_alignment/best_alignment.cu:58-187) together with the final-state choice,
 * back-tracking and optional label translation its Python wrapper does (criterion/best_alignment/__init__.py:56-111).
 *   log_probs  fp32, element (t, b, v) at t*lp_stride_t + b*lp_stride_b + v*lp_stride_v (after log_softmax)
 *   targets    int64 [N][>= max_target_length], row stride tg_stride_b;  input_lengths / target_lengths int64 [N];
 *              max_target_length 0..1023 (E_SHAPE "shape" below 0, "1023" above)
 *   out        int64 [N][S]: CTC state in [0, 2T+1) per frame (as_labels: the label, blank for even states);
 *              frames >= input_lengths[b] get state 0 / blank, as the reference returns
 *   scratch    simulst_ctc_best_alignment_scratch_bytes(N, S, max_target_length) bytes (1-byte back-pointers)
 *   neg_log_likelihood  optional fp32 [N]: -log of the two final Viterbi scores' sum (the kernel's first output)
 * Tie rules are the reference's: predecessor preference s, s-1, s-2 under strict '>', first maximum at the end.
 * out == NULL (pointer presence, as simulst_rnnt_forward): the SUM over alignments instead.  neg_log_likelihood is then required
 * (E_NULL) and receives the true CTC negative log-likelihood of each utterance -- F.ctc_loss(reduction="none"),
 * criterion/joint_ctc_criterion.py:78-90: the same state recursion with log-add over the legal predecessors in place of max (s-2 only
 * between different labels), -log of the two final states' sum, +inf when no alignment exists (never NaN), T = 0 the sum of the
 * blanks.  No back-pointers: scratch is not read and may be NULL; as_labels is ignored; the 1023-label limit is the same. */
int64_t simulst_ctc_best_alignment_scratch_bytes(int32_t N, int32_t S, int32_t max_target_length);
int simulst_ctc_best_alignment(simulst_handle* h, const float* log_probs, int64_t lp_stride_t, int64_t lp_stride_b,
                               int64_t lp_stride_v, const int64_t* targets, int64_t tg_stride_b,
                               const int64_t* input_lengths, const int64_t* target_lengths, int32_t S, int32_t N,
                               int32_t max_target_length, int32_t blank, int32_t as_labels, void* scratch,
                               int64_t* out, float* neg_log_likelihood);

/* CTC prefix beam search: every frame of the time-synchronous search over per-frame candidate lists in one launch
 * (csrc/ctc_prefix.hip), the recursion simulst_amd/ctc.py ctc_prefix_beam_advance spells out, with its pool order and tie rule.
 *   cand_log_probs  the CANDIDATES' log-probabilities, fp32, element (t, b, j) at t*lp_stride_t + b*lp_stride_b + j*lp_stride_v,
 *              j = 0..k; slot 0 is the blank
 *   input_lengths  int64 [N]: the frames of this call to take of utterance b, t = 0 .. min(S, input_lengths[b]) - 1; with none
 *              (<= 0) the utterance's state is not touched, bit for bit.  Candidates of frames at and past it are not read
 *   S          the frames in the call (S > 0);  N utterances (N <= 0: nothing is launched, OK);  beam 1..16 (E_SHAPE otherwise)
 *   strings    int64 [N][beam][cap]: the beam's strings, read at entry and written at exit, `pad` behind each length and in dead slots
 *   desc       a HOST simulst_ctc_prefix_desc (below), read during the call;  blank >= 0, informational (the blank is candidate slot 0)
 * State of utterance b and beam slot i (in / out): lengths[b][i], p_b[b][i], p_nb[b][i] (log-probability of the prefix ending in a
 * blank / in its last label) and the string strings[b][i][:lengths].  Slots are in descending order of p_b (+) p_nb; a dead slot is
 * (-inf, -inf), length 0, all `pad`.  Per frame and live prefix l with last label e, lp the frame's candidate log-probabilities:
 *   p_b'(l) = (p_b (+) p_nb) + lp[blank];   p_nb'(l) = p_nb + lp[e] if e is a candidate;
 *   p_nb'(l + c) = p_b + lp[c] if c == e else (p_b (+) p_nb) + lp[c]        for every candidate c >= 0 (candidates of a frame are distinct)
 * An extension that spells a prefix already in the beam (decided on the labels; a hash only filters) is added to that entry's p_nb'
 * and leaves the pool; the best `beam` pool entries by p_b' (+) p_nb' survive, ties in pool index order: the beam's own entries, then
 * the extensions prefix-major, candidate-minor.  (+) is max + log1p(exp(-|a - b|)) in fp32 with the accurate expf / log1pf, -inf when
 * both operands are, never NaN.  An utterance's result depends neither on its position in the batch nor on how its frames are cut into
 * calls: the state after frames [0, a) then [a, T) is the state after [0, T) in every bit.
 * The strings stay in LDS for the call (int32, two buffers), which bounds the capacity: cap <= SIMULST_CTC_PREFIX_CAP(beam) -- 1104
 * labels at beam 16, 2208 at beam 8.  The caller provides cap >= the longest length at entry + the frames taken (a string grows by at
 * most one label a frame; a label that would not fit is dropped).
 * Refusals, before any launch: E_NULL for a NULL desc, strings, cand_log_probs, input_lengths, cand_ids, lengths, p_b or p_nb; E_SHAPE
 * for S <= 0 or blank < 0 ("shape"), beam outside 1..16 ("beam is"), k outside 0..8 ("k is"), cap < 1 or above the limit ("cap is") */
#define SIMULST_CTC_PREFIX_STRING_BYTES 141312                                        /* LDS for the two string buffers: 138 KB */
#define SIMULST_CTC_PREFIX_CAP(beam) ((SIMULST_CTC_PREFIX_STRING_BYTES / (8 * (beam))) & ~3)
typedef struct simulst_ctc_prefix_desc {
  const int32_t* cand_ids;        /* device int32: the candidates' labels, element (b, t, j) at b*id_stride_b + t*id_stride_t + j,
                                     j = 0..k (simulst_linear's SIMULST_EPI_ROW_TOPK output as it is); -1 = no candidate; slot 0 unused */
  int64_t id_stride_b, id_stride_t;
  int32_t k;                      /* non-blank candidates per frame, 0..8 */
  int32_t pad;                    /* label written behind each string and into dead slots */
  int32_t cap;                    /* labels per string of `strings` */
  int64_t* lengths;               /* device int64 [N][beam], in / out */
  float* p_b;                     /* device fp32 [N][beam], in / out */
  float* p_nb;                    /* device fp32 [N][beam], in / out */
} simulst_ctc_prefix_desc;
int simulst_ctc_prefix_beam(simulst_handle* h, const float* cand_log_probs, int64_t lp_stride_t, int64_t lp_stride_b,
                            int64_t lp_stride_v, const int64_t* input_lengths, int32_t S, int32_t N, int32_t beam, int32_t blank,
                            const simulst_ctc_prefix_desc* desc, int64_t* strings);

/* CTC prefix scores inside the attention beam search: the call scores the candidates of one step by their CTC prefix probability, or
 * commits the step's selection (csrc/ctc_prefix_score.hip; DESIGN.md "Beam search", subsection "CTC prefix scores inside the beam").
 *   K          1..32: the candidates of a row (2 * beam)
 *   N          beam rows r = s * G + j of N / G sentences (N <= 0: nothing is launched, OK);  S the frames of the buffers
 *   cand_log_probs  the CANDIDATES' log-probabilities under the CTC head, fp32: element (t, s, j * K + k) at t*lp_stride_t +
 *              s*lp_stride_b + (j * K + k)*lp_stride_v -- simulst_linear's SIMULST_EPI_ROW_GATHER over cand_tok viewed as [N / G][G * K]
 *   last_labels     int64 [N]: the last label of each row's hypothesis (not read where the prefix is empty).  Both are read by op 0 alone
 *   prefix_lengths  int64 [N]: the labels of each row's hypothesis, 0 = the empty prefix
 *   input_lengths   int64 [N]: the frames T of each row, cut to S; frames at and past T are not read
 *   desc       a HOST simulst_ctc_score_desc (below), read during the call;  blank >= 0: a candidate equal to it, to pad, or negative
 *              has psi = -inf
 * op 0, score (one launch, a wave per row, a lane per candidate; rows of finished sentences, and with first_only the rows j > 0, are
 * not touched).  The row's state is gn[t], gb[t] (state [N][S][2]: log-probability of the alignments of frames 0..t that spell the
 * hypothesis g and end in its last label / in a blank) and psi [N].  For a candidate c that is a label, e the last label of g:
 *   phi[t] = gb[t] if c == e else gn[t] (+) gb[t];  phi[-1] = 0 for the empty g, else -inf;  gn'[-1] = gb'[-1] = -inf
 *   gn'[t] = (gn'[t-1] (+) phi[t-1]) + x[t][c];  gb'[t] = (gn'[t-1] (+) gb'[t-1]) + x[t][blank];  psi(g c) = (+)_t (phi[t-1] + x[t][c])
 * (psi(g c) = -inf with T = 0); for c == eos psi = gn[T-1] (+) gb[T-1] (T = 0: 0 for the empty g, else -inf).  (+) as in
 * simulst_ctc_prefix_beam.  delta = -1e4 if psi(h) is -inf, else max(psi(h) - psi(g), -1e4); the candidate's score becomes cand_lp
 * unchanged where it is -inf or weight == 0, else (1 - weight) cand_lp + weight delta.  Outputs: cand_state [N][S][K][2] (gn', gb' of
 * lane k; -inf for a candidate that is no label), cand_psi [N][K], and cand_lp / cand_tok REWRITTEN IN PLACE in candidate order
 * (descending score, equal scores to the lower token) with cand_slot [N][K] = the slot each entry came from (the k of cand_state /
 * cand_psi).  A candidate's result does not depend on its slot, its row or the other candidates.
 * op 1, commit (behind simulst_beam_select): row r of an unfinished sentence takes cand_state / cand_psi of candidate next_tok[r] of
 * row reorder[r] into state_out [N][S][2] / psi_out [N], with last_out[r] = next_tok[r] and len_out[r] = prefix_lengths[reorder[r]] + 1.
 * A parent outside the row's sentence or a token that is not among the parent's candidates adds 1 to *result and leaves the row.
 * Refusals, before any launch: E_NULL for a NULL desc, prefix_lengths, input_lengths, cand_state, cand_psi, cand_tok, cand_slot, and
 * for op 0 last_labels, cand_log_probs, blank_lp, state, psi, cand_lp, for op 1 next_tok, reorder, state_out, psi_out, last_out,
 * len_out, result; E_SHAPE for K outside 1..32, G < 1, S <= 0, blank < 0, an op other than 0 / 1, N not a multiple of G. */
typedef struct simulst_ctc_score_desc {
  int32_t op;                     /* 0 = score, 1 = commit */
  int32_t G;                      /* rows per sentence (the beam) */
  int32_t eos, pad;
  float weight;                   /* lambda, the CTC weight of the combined score */
  int32_t first_only;             /* score: only row j = 0 of every sentence (step 0 of the beam search) */
  const float* blank_lp;          /* device fp32: the blank's log-probability, element (s, t) at s*blank_stride_b + t */
  int64_t blank_stride_b;
  const float* state;             /* device fp32 [N][S][2] */
  const float* psi;               /* device fp32 [N] */
  float* cand_state;              /* device fp32 [N][S][K][2]: written by score, read by commit */
  float* cand_psi;                /* device fp32 [N][K] */
  float* cand_lp;                 /* device fp32 [N][K], in / out (simulst_beam_topk's) */
  int32_t* cand_tok;              /* device int32 [N][K], in / out */
  int32_t* cand_slot;             /* device int32 [N][K] */
  const int32_t* finished;        /* device int32 [N / G] or NULL */
  const int64_t* next_tok;        /* commit: device int64 [N] (simulst_beam_select's) */
  const int32_t* reorder;         /* commit: device int32 [N] */
  float* state_out;               /* commit: device fp32 [N][S][2], the second state set */
  float* psi_out;                 /* commit: device fp32 [N] */
  int64_t* last_out;              /* commit: device int64 [N] */
  int64_t* len_out;               /* commit: device int64 [N] */
  int32_t* result;                /* commit: device int32, + 1 per row whose token was not found */
} simulst_ctc_score_desc;
int simulst_ctc_prefix_score(simulst_handle* h, const float* cand_log_probs, int64_t lp_stride_t, int64_t lp_stride_b,
                             int64_t lp_stride_v, const int64_t* last_labels, const int64_t* input_lengths, const int64_t* prefix_lengths,
                             int32_t S, int32_t N, int32_t K, int32_t blank, const simulst_ctc_score_desc* desc);

/* Batched edit distance: the call compares label strings -- the batched Levenshtein alignment of N (reference, hypothesis) pairs in
 * one launch (csrc/edit_distance.hip; DESIGN.md "CTC head", subsection "Error rates"), what the word error rate of the reference's
 * ASR stage is summed from (tasks/speech_to_text_infer.py:206-215, :263-289).  desc: a HOST simulst_edit_desc (below), read during the call
 *   refs       int64: the REFERENCE strings, row r at r*ref_stride_b;  ref_lengths int64 [n_ref]: their lengths
 *   hyp_lengths  int64 [n_hyp]: the HYPOTHESIS lengths (the strings themselves are simulst_edit_desc.hyp)
 *   ref_cap, hyp_cap   the two capacities: no reference is longer than ref_cap, no hypothesis longer than hyp_cap; both 0..1023
 *              (E_SHAPE "1023" above it), the label limit of simulst_ctc_best_alignment
 *   N          the PAIRS (N <= 0: nothing is launched, OK).  Pair p compares reference row ref_idx[p] with hypothesis row hyp_idx[p];
 *              a NULL index array means p.  Strings and lengths are read through the indices, in place: one reference can face 16
 *              hypotheses, and a list can face itself (the same buffer on both sides)
 *   ops        the alignment [N][ops_cap], int8 or int32 (ops_width), or NULL (pointer presence): counts only
 * With D[i][j] the distance of the first i reference labels and the first j hypothesis labels, the predecessor of a cell is, among
 * those that attain the minimum, the first of: the DIAGONAL (D[i-1][j-1]; a match if the labels are equal, else a substitution), a
 * DELETION (D[i-1][j] + 1: reference label i has no counterpart), an INSERTION (D[i][j-1] + 1).  counts[p] = (distance, sub, del,
 * ins), int32, the last three counted along the path from (Lr, Lh) back to (0, 0) under this rule; they are carried forward with the
 * minimum, so the counts-only form writes 16 bytes a pair and reads nothing but the strings.  Empty strings are ordinary: distance Lh,
 * Lr or 0.  Nothing at or past a length is read; rows no pair names are not touched.
 * With `ops`: ops[p][0 .. n_ops[p]) is that alignment front to back, 0 match, 1 substitution, 2 deletion, 3 insertion, `pad` behind
 * it; n_ops[p] = Lr + ins <= ops_cap.  One-byte back-pointers go to `bp` (SIMULST_EDIT_BP_BYTES, 16-byte aligned), the back-track runs
 * on the device.  A pair's counts do not depend on its position, on the other pairs, or on whether the path was asked for.
 * A pair whose index is outside [0, n_ref) / [0, n_hyp), or whose string is longer than its capacity, reads no string: its counts are
 * (-1, -1, -1, -1), n_ops 0, ops all `pad`.  With a NULL index array the host knows the indices: N above n_ref / n_hyp is E_SHAPE.
 * Refusals, before any launch: E_NULL for a NULL desc, refs, ref_lengths, hyp_lengths, hyp, counts, and with `ops` n_ops and bp
 * (N > 0); E_SHAPE for a capacity above 1023 ("1023") or below 0, ops_width other than 1 / 4, ops_cap < ref_cap + hyp_cap, bp_bytes
 * below SIMULST_EDIT_BP_BYTES; E_ARG for a misaligned bp. */
#define SIMULST_EDIT_BP_BYTES(N, ref_cap, hyp_cap) ((int64_t)(N) * (((hyp_cap) + 63) / 64) * ((ref_cap) + 63) * 64)
typedef struct simulst_edit_desc {
  const int64_t* hyp;             /* device int64: the hypothesis strings, row r at r*hyp_stride_b */
  int64_t hyp_stride_b;
  const int32_t* ref_idx;         /* device int32 [N] or NULL (= p) */
  const int32_t* hyp_idx;         /* device int32 [N] or NULL (= p) */
  int32_t n_ref, n_hyp;           /* rows of the two sides: what an index is compared with */
  int32_t* counts;                /* device int32 [N][4]: distance, sub, del, ins */
  int32_t* n_ops;                 /* device int32 [N]; read only with `ops` */
  void* bp;                       /* device scratch for the back-pointers; read only with `ops` */
  int64_t bp_bytes;
  int32_t ops_cap;                /* elements per row of `ops`, >= ref_cap + hyp_cap */
  int32_t ops_width;              /* bytes per element of `ops`: 1 (int8) or 4 (int32) */
  int32_t pad;                    /* written behind each alignment */
  int32_t reserved;               /* 0 */
} simulst_edit_desc;
int simulst_edit_distance(simulst_handle* h, const int64_t* refs, int64_t ref_stride_b, const int64_t* ref_lengths,
                          const int64_t* hyp_lengths, int32_t ref_cap, int32_t hyp_cap, int32_t N, const simulst_edit_desc* desc, void* ops);

/* ---- whole decode steps on the device ----------------------------------------------
 * Runs n_steps consecutive WRITE steps of the MMA / wait-k decoder for a batch in lockstep with no
 * host round trip: embed -> n_layers x { LN+QKV, self-attention, out-proj+res, LN+q-proj,
 * policy (p_choose + step search) + cross-attention, out-proj+res, LN+fc1+GELU, fc2+res } -> LN+logits
 * -> greedy pick, which feeds the next step's embedding.  This is the offline loop of
 * eval/generate.py:187-209 ('online' unset => never READs, models/mma_model.py:191-193); with
 * n_steps == 1 it is one policy()/predict() pair of agents/default_agent.py:378-424 after which the
 * caller inspects head_read.  Pointers per layer in simulst_dec_layer, shared ones in
 * simulst_decoder_desc; all device memory is caller-owned.
 * attn_type SIMULST_ATTN_FULL (offline encoder-decoder attention): the policy is skipped, every layer attends over
 * all enc_len[b] rows; head_step / head_read are neither read nor written (they must still be valid buffers: the
 * retire and beam-reorder calls move them), c_wq_soft is unused and Kmono / Ksoft may be the same K buffer. */
typedef struct {
  const void* wqkv; const float* bqkv;           /* self-attention [3D][D] (q|k|v) */
  const void* wo; const float* bo;
  const float *ln1_g, *ln1_b, *ln2_g, *ln2_b, *ln3_g, *ln3_b;
  const void* c_wq; const float* c_bq;           /* monotonic-energy query projection */
  const void* c_wq_soft; const float* c_bq_soft; /* soft-energy query projection (NULL: shares c_wq) */
  const void* c_wo; const float* c_bo;
  const void* fc1; const float* b1; const void* fc2; const float* b2;
  float energy_bias;
  void *k_cache, *v_cache;                       /* [B][H][cap][d] */
  int64_t* head_step;                            /* [B*H] in/out */
  uint8_t* head_read;                            /* [B*H] out */
  const void *Kmono, *Ksoft, *V;                 /* [B][H][S_cap][head_dim] (head-major) cached projections of the
                                                    encoder states: a head's key rows are contiguous 128-byte lines */
  const float* Kpool;                            /* optional [B][H][P_cap][head_dim] fp32: the pooled monotonic keys of every
                                                    COMPLETE pre-decision window (simulst_pool_keys, 'average' pooling), read
                                                    by the policy instead of the window's frames; NULL: pooled per step */
} simulst_dec_layer;

typedef struct {
  int32_t B, D, H, F, V, n_layers, cap, S_cap, dtype;
  int32_t attn_type, ratio, waitk_k, mass_preservation, online;
  int32_t pad_idx, eos_idx;
  int32_t n_prev_uniform;                        /* >= 0: every row has written exactly this many tokens (lockstep
                                                    batches; saves a dependent device read per kernel); -1: use n_prev[] */
  float embed_scale;
  const void* E;                                 /* [V][D] token embedding */
  const void* out_proj;                          /* [V][D] output projection (shared with E in the reference runs) */
  const float* pos_table;                        /* [rows][D] sinusoidal table */
  const float *ln_g, *ln_b;                      /* final LayerNorm */
  const int32_t* enc_len;                        /* [B] valid source rows */
  int32_t* n_prev;                               /* [B] in/out: tokens written so far */
  void *x, *qkv, *ctx, *q, *q2, *hidden;         /* workspace: [B][D], [B][3D], [B][D], [B][D], [B][D], [B][F] */
  float* logits;                                 /* workspace [B][V] (with SIMULST_OPT_FUSED_ARGMAX the decode loops keep
                                                    [B][V / 64] (largest value, its index) pairs of the vocabulary projection's
                                                    column tiles here instead of fp32 rows) */
  /* optional workspace of the head-split self-attention block (both non-NULL, cap <= 256, head_dim % 16 == 0,
   * D <= 512): { LN + QKV GEMM, self-attention, out-proj GEMM } become ONE launch per layer in which every
   * (head, utterance) workgroup projects its own q/k/v rows, appends to the cache, attends, and multiplies by
   * its head's columns of the output projection; the fp32 per-head partials are added (head order, deterministic)
   * together with the bias and the residual by the following policy/cross-attention launch.  NULL: 7-launch layer. */
  void* x_mid;                                   /* [B][D] */
  float* partial_self;                           /* [B][H][D] */
  int32_t weights_fragment_major;                /* every weight MATRIX of simulst_dec_layer and out_proj is in the
                                                    fragment-major order of simulst_linear_desc.w_fragment_major
                                                    (E stays row-major: it is read by row); required by the
                                                    head-split block */
  /* optional workspace of the row-local layer chains (ffn_partial and x_mid non-NULL, bf16, D == 256, F % 256 == 0, fragment-major
   * weights, more than 128 rows): { out-proj + residual, LN + q-proj } become one launch and { cross out-proj +
   * residual, LN + fc1 + GELU, fc2 + residual } another, the hidden units split over F / 256 workgroups per row tile
   * whose fp32 slabs the last-arriving workgroup adds in split order (deterministic).  NULL: one launch per GEMM. */
  float* ffn_partial;                            /* [F / 256][B][D] */
  int32_t P_cap;                                 /* pooled positions per row of simulst_dec_layer.Kpool (0 when no layer has one) */
  int32_t* ffn_sem;                              /* unused by the decode loop (it runs the feed-forward chain without the in-launch
                                                    hand-off); may be NULL.  simulst_decoder_ffn_chain(x_mid = NULL) takes its own */
} simulst_decoder_desc;

/* tokens_io [B] int64: in = newest token of [eos]+hyp, out = last token picked.
 * out_tokens [n_steps][B] int64.  EOS is masked when mask_eos != 0 or while n_prev == 0
 * (SequenceGenerator min_len = 1). */
int simulst_mma_decode(simulst_handle* h, const simulst_decoder_desc* d, const simulst_dec_layer* layers,
                       int64_t* tokens_io, int64_t* out_tokens, int32_t n_steps, int32_t mask_eos);

/* Offline decode with hypotheses finalised at EOS (fairseq's SequenceGenerator, beam 1: a finished hypothesis leaves the
 * batch): run between two chunks of simulst_mma_decode over the first `rows` slots of a lockstep batch of B rows.
 * Slot i holds original row slot_row[i] (-1: dead), whose step cap is row_cap[i].  In order on the handle's stream:
 *  1. every live slot's tokens of the chunk (chunk_tokens [n_steps][rows], simulst_mma_decode's out_tokens) go to
 *     hyp[slot_row[i]][n_prev[i] - n_steps + s] ([B][U] int64, by original row) up to the row's first EOS (kept; eos_idx < 0:
 *     never) or its cap; padding_idx behind that, and the finished slot leaves slot_row (-1);
 *  2. a stable partition of the live slots of [0, rows): the k-th dead slot in front of the live count n_live takes the state
 *     of the k-th live slot behind it -- self K/V [0, n_prev), cross K/V and soft keys [0, enc_len), pooled keys of complete
 *     windows, head_step, head_read, n_prev, enc_len, enc_len_bh (may be NULL; [B][H]), slot_row, row_cap and
 *     last_tokens ([B] int64: the tokens_io of the next chunk);
 *  3. result ([4 + 2 B] int32 device scratch): [0] n_live, [1] rows_next = n_live rounded up to 16 rows, clamped into the
 *     kernel class the decode loop runs a batch of B rows in (csrc/decode_plan.cpp sl_retire_floor_rows, beside the launch
 *     plan whose row switch points it keeps; 0 when no row is live), [2] pairs moved.
 * The next chunk runs simulst_mma_decode with d->B = rows_next; the slots behind n_live ride along dead. */
int simulst_mma_retire_rows(simulst_handle* h, const simulst_decoder_desc* d, const simulst_dec_layer* layers,
                            const int64_t* chunk_tokens, int32_t n_steps, int32_t rows, int32_t B, int32_t* slot_row,
                            int32_t* row_cap, int64_t* last_tokens, int64_t* hyp, int32_t U, int32_t* enc_len_bh,
                            int32_t* result);

/* Beam search over offline MMA / wait-k decoding (csrc/beam.hip): fairseq's SequenceGenerator with search.BeamSearch at the
 * reference's defaults (normalize_scores, min_len 1, no unk penalty, temperature 1, no prefix tokens or constraints).  Bs sentences
 * of `beam` rows each (row r = s * beam + j, R = Bs * beam), K = 2 beam candidates per row.  Limits: 1 <= beam <= 16,
 * 1 <= nbest <= beam, 2 beam <= V - 1.  Candidate order: descending score, equal scores to the lower flat index j * V + token.
 * Every launch goes on the handle's stream, with no allocation and no synchronisation (capturable).
 *
 * simulst_beam_topk: per row of logits [R][V] fp32, lp = log_softmax(row) with lp[pad] = -inf, lp[eos] = -inf at step 0 and every
 * entry but EOS -inf from step max_len[s] on; its top K (lp, token) pairs in candidate order -> cand_lp / cand_tok [R][K].  Rows of
 * finished sentences (finished [Bs] int32, may be NULL) and, at step 0, rows j > 0 are skipped. */
int simulst_beam_topk(simulst_handle* h, const float* logits, int32_t R, int32_t V, int32_t beam, int32_t step,
                      const int32_t* max_len, const int32_t* finished, int32_t pad_idx, int32_t eos_idx, float* cand_lp,
                      int32_t* cand_tok);

/* simulst_beam_select: one wave per unfinished sentence.  The top K of cum[r] + cand_lp over the sentence's rows (step 0: row j = 0
 * with cum 0).  Among the first beam, EOS candidates with a finite score are finalised while the sentence holds fewer than beam:
 * slot fin_count[s] of the tables fin_step / fin_row (the parent row) / fin_raw (the score) / fin_score (score / (step + 1)^lenpen),
 * [Bs][beam].  The sentence is finished (finished[s] = 1) when it holds beam of them or step == max_len[s].  Otherwise the first beam
 * candidates that are not finalised EOS become rows j = 0 .. beam - 1: reorder[r] (parent row), next_tok[r] (int64, the next step's
 * input), cum[r], and the back-pointers bp_parent / bp_token / bp_cum [L][R] at row `step`.  result [2] int32 (device scratch):
 * [0] sentences unfinished after this step (cleared here), [1] += sentences short of beam finite non-EOS next rows (never under
 * the masks above; fairseq's cands_to_ignore is not implemented). */
int simulst_beam_select(simulst_handle* h, const float* cand_lp, const int32_t* cand_tok, int32_t Bs, int32_t beam, int32_t V,
                        int32_t step, const int32_t* max_len, int32_t L, double lenpen, int32_t eos_idx, float* cum,
                        int64_t* next_tok, int32_t* reorder, int32_t* bp_parent, int32_t* bp_token, float* bp_cum,
                        int32_t* fin_step, int32_t* fin_row, float* fin_score, float* fin_raw, int32_t* fin_count,
                        int32_t* finished, int32_t* result);

/* simulst_beam_reorder: row r of the second buffer set `dst` takes row reorder[r] of `src`, per layer: the self-attention K/V
 * positions [0, n_prev) (k_cache / v_cache [R][H][cap][d]), head_step [R H] and head_read [R H] (when both sets carry it).  d gives
 * R = d->B, H, D, n_layers, cap and dtype; only those fields of the simulst_dec_layer entries are read.  Rows of finished sentences
 * (finished [Bs], may be NULL) keep their own head_step and copy no K/V.  The cross-attention buffers are the same for every row of
 * a sentence and are not touched.  A reorder that leaves its sentence's block of beam rows is not performed (the row keeps its own
 * state) and added to result [1] int32 (device scratch, cleared by the caller). */
int simulst_beam_reorder(simulst_handle* h, const simulst_decoder_desc* d, const simulst_dec_layer* src, const simulst_dec_layer* dst,
                         const int32_t* reorder, const int32_t* finished, int32_t beam, int32_t n_prev, int32_t* result);

/* simulst_beam_backtrack: once, after the last step.  Per sentence its finalised hypotheses by descending fin_score (equal scores
 * in finalisation order), the first nbest, walked back through the back-pointers: tokens [Bs][nbest][L] int64 (EOS included,
 * pad_idx behind), lengths [Bs][nbest] int32, scores [Bs][nbest] fp32 and positional scores [Bs][nbest][L] fp32 (the differences
 * of the cumulative scores along the path, 0 behind).  Slots no hypothesis reached: length 0, score -inf. */
int simulst_beam_backtrack(simulst_handle* h, int32_t Bs, int32_t beam, int32_t nbest, int32_t L, const int32_t* bp_parent,
                           const int32_t* bp_token, const float* bp_cum, const int32_t* fin_step, const int32_t* fin_row,
                           const float* fin_score, const float* fin_raw, const int32_t* fin_count, int32_t pad_idx,
                           int32_t eos_idx, int64_t* tokens, int32_t* lengths, float* scores, float* pos_scores);

/* BATCHED STREAMING decode steps (no counterpart in the reference, which asserts B == 1 when streaming,
 * models/s2t_emformer.py:200): n_iter policy()/predict() rounds for every row of a batch whose rows decide
 * READ / WRITE independently.  Per row and round: the layers run until one wants more source while the row is
 * online (models/mma_model.py:191-210) -- then the row is parked (active = 0) with its target position not
 * advanced -- else the greedy token (plain argmax, agents/default_agent.py:415-424) is committed to hyp, stamped
 * with cur_ms, and the row finishes on EOS or when it holds more than max_len_now tokens
 * (agents/default_agent.py:268-271).  The host re-activates parked rows after feeding the next source chunk.
 * Device arrays of length B unless noted; dd->n_prev_uniform must be -1.
 *
 * SELF-PACED ROWS (sched_rows != NULL; evaluation of a streaming policy over sources that are already on the device, the way
 * SimulEval feeds an agent from a file: agents/default_agent.py:303-342,364-412).  The caller has pushed EVERY chunk through the
 * streaming encoder and appended it to the cached keys / values, and hands over every row's chunk schedule: after its chunk c row b
 * holds sched_rows[b][c] encoder rows, sched_ms[b][c] milliseconds of source and may hold sched_max_len[b][c] tokens; its source has
 * row_chunks[b] chunks (sources of different lengths ride in one batch).  A row that asks for source
 * is not parked: the commit takes the next chunk for it (chunk_idx[b] += 1, enc_len[b] = sched_rows[b][chunk_idx[b]],
 * online[b] = chunk is not the last) and the row tries the same target position again in the next round, so rows advance through
 * their sources independently of each other with no host round trip -- at most cap + n_chunks rounds per row.  cur_ms and
 * max_len_now are then read from the schedule at the row's chunk.  A row's READ / WRITE sequence, tokens and delays are those of
 * the parked form (tests/test_hip_streaming.py); the READs are recovered from tok_chunk. */
typedef struct {
  uint8_t* active;        /* in/out */
  uint8_t* read_flag;     /* scratch, zero before the first call */
  uint8_t* online;        /* row's source has not ended (written by the commit for self-paced rows) */
  uint8_t* done;          /* out: hypothesis finished */
  int32_t* delays_ms;     /* [B][cap] or NULL */
  int64_t* hyp;           /* [B][cap] committed tokens */
  int32_t cap, cur_ms, max_len_now;
  int32_t n_chunks;               /* self-paced rows: width of the schedule tables (the longest source's chunks) */
  const int32_t* sched_rows;      /* [B][n_chunks] or NULL (parked form) */
  const int32_t* sched_ms;        /* [B][n_chunks] */
  const int32_t* sched_max_len;   /* [B][n_chunks] */
  int32_t* chunk_idx;             /* [B] in/out: the chunk each row has read up to (0 at the start) */
  int32_t* enc_len;               /* [B] in/out: simulst_decoder_desc.enc_len, advanced with the row's chunk */
  int32_t* tok_chunk;             /* [B][cap] out or NULL: chunk index at which each token was committed */
  const int32_t* row_chunks;      /* [B] chunks of each row's source, or NULL: n_chunks for every row */
  int32_t ff_waitk, ff_ratio;     /* wait-k rows (0: off): the descriptor's waitk_k and ratio.  Wait-k's READ is a closed form of the row's
                                     position and source length, so the commit takes every chunk the row is going to ask for on the
                                     spot (position u can be written once the source holds u + k pooled keys) and no round is spent on
                                     asking; the caller starts every row at the first chunk that allows position 0 */
  /* Parity audit of the learned policies (tools/teacher_forced_audit.py; NULL in production).  p_probe [n_layers][B][H][probe_P] receives
   * the pooled step probabilities sigmoid(energy) every (layer, row, head) computed in the round (modules/monotonic_multihead_attention.py:
   * 88-149 over the pooled keys of modules/fixed_pre_decision.py:97-131), step_probe [n_layers][B][H] the step its own search found
   * (:196-257); a step_force [n_layers][B][H] entry >= 0 replaces the found step for head_step and the value aggregation, so a run can
   * be driven along another implementation's trajectory (teacher forcing) while its own decisions are recorded. */
  float* p_probe; int64_t* step_probe; const int64_t* step_force; int32_t probe_P;
  /* Active-row compaction (round 6; compact_rows <= 0: off).  A batch of LIVE streams (the microphone form: the reference's agent
   * runs the same loop for one stream, agents/default_agent.py:364-413, models/mma_model.py:191-210) has only a fraction of its rows
   * taking part in a given round -- a row that asked for source is parked until the next chunk -- while the row-local GEMMs of a round
   * cost by the rows they are launched over.  With compact_rows > 0 every round first lists the rows that take part (active[b] != 0)
   * into row_map [compact_rows] int32 (device scratch), at most compact_rows of them in row order, the others wait for a later round
   * with their masks untouched; every launch of the round then runs over compact_rows SLOTS: the step's activations (x, qkv, ctx, q,
   * logits) are indexed by slot, everything a stream owns (K / V caches, enc_len, n_prev, head_step, tokens_io, hyp, the masks) by
   * its own row.  A row's tokens, delays and READ / WRITE sequence do not depend on the slots it travelled in.  Needs
   * 128 < compact_rows <= B, S_cap <= 256 and no audit hooks; the decoder descriptor's step buffers must hold max(B, compact_rows) rows. */
  int32_t* row_map; int32_t compact_rows;
} simulst_stream_ctl;

int simulst_mma_stream_steps(simulst_handle* h, const simulst_decoder_desc* d, const simulst_dec_layer* layers,
                             int64_t* tokens_io, const simulst_stream_ctl* ctl, int32_t n_iter);


/* ---- whole CIF decode steps on the device --------------------------------------------
 * The position-synchronous decoder of models/cif_transformer.py:579-724 (CIFDecoder.extract_features_scriptable / forward with
 * incremental_state) for a batch, n_steps target positions with no host round trip -- the loop eval/generate.py:187-209 runs
 * through SequenceGenerator and, with n_steps == 1, one policy()/predict() pair of agents/cif_agent.py:368-436.  At position u
 * (= tokens in [eos] + hypothesis) row b looks at integrated vector cif[b][min(cif_len[b], u) - 1] (:622-628); its decoder layer is
 * fairseq's with FakeCrossAttn out_proj(gelu(q_proj(LN x) + k_proj(c))) in place of attention (:340-362); the EOS logit gets
 * max(0, u - cif_len[b]) * overshoot_weight (:716-722).  k_proj(c) is projected ONCE per integrated vector by the caller
 * (Kc = simulst_linear over the new slots, bias included) and gathered per step.  Same workspace / weight-order conventions as
 * simulst_decoder_desc. */
typedef struct {
  const void* wqkv; const float* bqkv;           /* self-attention [3D][D] (q|k|v) */
  const void* wo; const float* bo;
  const float *ln1_g, *ln1_b, *ln2_g, *ln2_b, *ln3_g, *ln3_b;
  const void* c_wq;                              /* FakeCrossAttn.q_proj [D][D] (no bias, models/cif_transformer.py:344) */
  const void* c_wo; const float* c_bo;           /* FakeCrossAttn.out_proj */
  const void* fc1; const float* b1; const void* fc2; const float* b2;
  void *k_cache, *v_cache;                       /* [B][H][cap][d] */
  const void* Kc;                                /* [B][n_cap][D] = k_proj(cif_out) + bias of this layer, row-major */
} simulst_cif_dec_layer;

typedef struct {
  int32_t B, D, H, F, V, n_layers, cap, n_cap, dtype;
  int32_t pad_idx, eos_idx;
  int32_t highway;                               /* --cif-highway: logits = E^T (LN(x) + c) (models/cif_transformer.py:681-682) */
  int32_t n_prev_uniform;                        /* >= 0: every row has written exactly this many tokens; -1: use n_prev[] */
  float embed_scale, overshoot_weight;
  const void* E; const void* out_proj; const float* pos_table; const float *ln_g, *ln_b;
  const int32_t* cif_len;                        /* [B] integrated vectors available per row */
  const void* cif;                               /* [B][n_cap][D] the vectors themselves (highway only, else may be NULL) */
  int32_t* n_prev;                               /* [B] in/out: tokens written so far */
  void *x, *qkv, *ctx, *q, *hidden;              /* workspace: [B][D], [B][3D], [B][D], [B][D], [B][F] */
  float* logits;                                 /* workspace [B][V] */
  void* kk;                                      /* workspace [n_layers][B][D]: the gathered Kc rows of the current step */
  void* cif_t;                                   /* workspace [B][D] (highway only) */
  float* eos_bias;                               /* workspace [B] */
  void* x_mid; float* ffn_partial;               /* optional: row-local layer chains, as in simulst_decoder_desc */
  int32_t weights_fragment_major;
} simulst_cif_decoder_desc;

/* tokens_io [B]: in = newest token of [eos] + hyp, out = last token picked; out_tokens [n_steps][B].  pad is never picked; EOS is
 * masked when mask_eos != 0 or while n_prev == 0 (SequenceGenerator min_len = 1). */
int simulst_cif_decode(simulst_handle* h, const simulst_cif_decoder_desc* d, const simulst_cif_dec_layer* layers,
                       int64_t* tokens_io, int64_t* out_tokens, int32_t n_steps, int32_t mask_eos);

/* BATCHED STREAMING CIF decode (no counterpart in the reference: CIFLayer.infer raises for B > 1, models/cif_transformer.py:199-200):
 * n_iter policy()/predict() rounds for every row.  A row WRITES in a round iff it is not done and (cif_len > n_prev or its source has
 * ended) -- the complement of the agent's READ condition (agents/cif_agent.py:385-389) -- committing the plain argmax
 * (agents/cif_agent.py:414-436) to hyp with the stamp cur_ms; it is done on EOS or when it holds more than max_len_now tokens.
 * Rows that cannot write are left untouched; the host feeds the next chunk (simulst_cif_stream_append + Kc projection) and calls again.
 *
 * SELF-PACED ROWS (sched_cif_len != NULL; evaluation over sources already on the device, as for simulst_stream_ctl): every chunk has
 * been encoded, integrated and its vectors projected; sched_cif_len[b][c] is the number of integrated vectors row b holds after its
 * chunk c, sched_ms[b][c] / sched_max_len[b][c] the source time and the length cap there, row_chunks[b] the chunks of its source.  A row that would READ takes chunks by itself inside
 * the commit -- as many as it needs, since this policy's READ does not depend on the decoder -- so every round of an unfinished row
 * is a WRITE and a row needs at most cap rounds.  chunk_idx [B] (zero at the start), cif_len (the descriptor's array) and online are
 * advanced by the commit; tok_chunk records the chunk of every token (from which the READs are recovered). */
typedef struct {
  uint8_t* online;        /* [B] row's source has not ended (written by the commit for self-paced rows) */
  uint8_t* done;          /* [B] in/out */
  int32_t* delays_ms;     /* [B][cap] or NULL */
  int64_t* hyp;           /* [B][cap] committed tokens */
  int32_t cap, cur_ms, max_len_now;
  int32_t n_chunks;               /* self-paced rows: width of the schedule tables */
  const int32_t* sched_cif_len;   /* [B][n_chunks] or NULL (parked form) */
  const int32_t* sched_ms;        /* [B][n_chunks] */
  const int32_t* sched_max_len;   /* [B][n_chunks] */
  int32_t* chunk_idx;             /* [B] in/out */
  int32_t* cif_len;               /* [B] in/out: simulst_cif_decoder_desc.cif_len */
  int32_t* tok_chunk;             /* [B][cap] out or NULL */
  const int32_t* row_chunks;      /* [B] or NULL */
} simulst_cif_stream_ctl;

int simulst_cif_stream_steps(simulst_handle* h, const simulst_cif_decoder_desc* d, const simulst_cif_dec_layer* layers,
                             int64_t* tokens_io, const simulst_cif_stream_ctl* ctl, int32_t n_iter);

/* Bookkeeping of a BATCHED CIFLayer.infer call (models/cif_transformer.py:235-255): of the n[b] slots simulst_cif_integrate produced
 * for this chunk (out [B][T_cap][D], tail_w [B]) all but the last -- the un-fired tail, withheld unless finish -- are appended to the
 * row's accumulated vectors acc [B][n_cap][D] at acc_len[b] (updated); the tail is carried as prev_weight[b] = tail_w[b],
 * prev_feat[b] = out[b][n[b] - 1] / beta (:239-251) to be put in front of the next chunk by the caller. */
int simulst_cif_stream_append(simulst_handle* h, const void* out, const int32_t* n, const float* tail_w, void* acc,
                              int32_t* acc_len, void* prev_feat, float* prev_weight, int32_t B, int32_t T_cap, int32_t n_cap,
                              int32_t D, float beta, int32_t finish, int32_t dtype);

/* Row-local chains of the decoder layer for co-scheduled batches (bf16, D == 256, fragment-major weights); the decode
 * loops use them where their launch plan says so (csrc/decode_plan.cpp sl_plan_decode: by default from 129 rows on when
 * simulst_decoder_desc.ffn_partial / x_mid are given).  Same rounding points as the
 * launches they replace (bf16 after bias + residual, after LayerNorm, after GELU).
 *   proj chain:  x <- bf16(x + Wo ctx + bo);  q <- Wq LN(x) + bq;  q2 <- Wq2 LN(x) + bq2 (wq2_fm may be NULL)
 *                = the self-attention output projection + residual of fairseq's TransformerDecoderLayer followed by
 *                encoder_attn_layer_norm and the (monotonic / soft) query projections of
 *                modules/monotonic_multihead_attention.py as run by models/mma_model.py:99-135
 *   proj chain, kk form (simulst_decoder_proj_chain_kk):  x as above;  q <- bf16(gelu(Wq LN(x) + bq + kk)), exact (erf) GELU,
 *                kk [B][256] bf16 required, bq may be NULL (taken as 0), no second projection
 *                = the CIF decoder's FakeCrossAttn, activation(q_proj(query) + k_proj(key)) (models/cif_transformer.py:357-362):
 *                the launch simulst_cif_decode makes, as an entry point of its own so that it can be checked alone
 *   ffn chain:  x' = bf16(x + Wco ctx + bco);  x <- bf16(x' + W2 gelu(W1 LN(x') + b1) + b2)
 *                = encoder_attn out_proj + residual, final_layer_norm, fc1, activation, fc2, residual of the same layer.
 *                partial: fp32 [F / 256][B][D] slabs (one per 256 hidden units).  x_mid == NULL: the last-arriving
 *                workgroup of a row tile adds the slabs inside the launch (sem: (B + 15) / 16 int32, zero on entry, zero on
 *                return).  x_mid != NULL: x' is written to x_mid, x is left alone and the slabs are added by the following
 *                simulst_decoder_slab_sum_qkv (the form the decode loop uses: the launch boundary is the hand-off).
 *   slab sum:    x <- bf16(x_mid + b2 + slab 0 + slab 1 + ...) (split order: deterministic);  with wqkv_fm != NULL also
 *                qkv [B][3 D] <- Wqkv LN(x) + bqkv, the next layer's self_attn_layer_norm + q / k / v projections.
 * LayerNorm here is eps 1e-5, biased variance, from one-pass moments in fp32 (E[x^2] - mean^2, clamped at 0).  Checked domain
 * (tests/test_hip_dec_chain_fp64.py against float64): rows whose common offset is up to 32 standard deviations (worst |got - ref| /
 * bound 0.46 there, 0.93 at 8), variance down to 1.5e-5 (the size of eps) and 0 (a constant row gives beta exactly), scale up to
 * 2^6; the variance loses about (offset / deviation)^2 2^-19 of its relative accuracy, so far larger offsets are outside it. */
int simulst_decoder_proj_chain(simulst_handle* h, const void* ctx, void* x, const void* wo_fm, const float* bo,
                               const float* ln_g, const float* ln_b, const void* wq_fm, const float* bq, void* q,
                               const void* wq2_fm, const float* bq2, void* q2, int32_t B, int32_t D, int32_t dtype);
int simulst_decoder_proj_chain_kk(simulst_handle* h, const void* ctx, void* x, const void* wo_fm, const float* bo,
                                  const float* ln_g, const float* ln_b, const void* wq_fm, const float* bq /* may be NULL */,
                                  void* q, const void* kk /* [B][256], required */, int32_t B, int32_t D, int32_t dtype);
int simulst_decoder_ffn_chain(simulst_handle* h, const void* ctx, void* x, const void* wco_fm, const float* bco,
                              const float* ln_g, const float* ln_b, const void* w1_fm, const float* b1, const void* w2_fm,
                              const float* b2, float* partial, int32_t* sem, void* x_mid, int32_t B, int32_t D, int32_t F,
                              int32_t dtype);
int simulst_decoder_slab_sum_qkv(simulst_handle* h, const void* x_mid, void* x, const float* partial, const float* b2,
                                 const float* ln_g, const float* ln_b, const void* wqkv_fm, const float* bqkv, void* qkv,
                                 int32_t B, int32_t D, int32_t F, int32_t dtype);

/* The closing launch of a decode step for co-scheduled bf16 batches (csrc/dec_chain.hip dec_vocab_chain_kernel): the last layer's
 * slab sum (as simulst_decoder_slab_sum_qkv), the decoder's final LayerNorm, the output projection (models/mma_model.py:212-220;
 * fairseq TransformerDecoder.output_layer, no bias) and the first half of the greedy choice (SequenceGenerator with beam 1,
 * eval/generate.py:141-155):  x <- bf16(x_mid + b2 + slabs);  pairs[row][s] = (largest logit, its lowest column, the column's
 * int32 bits in the second float) over columns [s V / split, (s + 1) V / split) of Wout LN(x), columns skip_a / skip_b (pad, a
 * masked eos; -1: none) excluded.  The fold over the `split` pairs of a row uses the same (value, lowest column) rule
 * (simulst_mma_decode's commit kernel).  wout_fm: [V][256] in fragment-major order; pairs [B][split][2] floats.
 * row_bias != NULL: row_bias[row] is added to the logit of column row_bias_col before the exclusions (simulst_cif_decode's per-row
 * eos bias, simulst_cif_decoder_desc.eos_bias).  bf16, D == 256, V a multiple of 256 x split. */
int simulst_decoder_vocab_chain(simulst_handle* h, const void* x_mid, void* x, const float* partial, const float* b2,
                                const float* ln_g, const float* ln_b, const void* wout_fm, float* pairs, int32_t B, int32_t D,
                                int32_t F, int32_t V, int32_t split, int32_t skip_a, int32_t skip_b, const float* row_bias,
                                int32_t row_bias_col, int32_t dtype);

#ifdef SIMULST_EXPERIMENTS
/* ---- `make EXPERIMENTS=1` builds only (measured slower than what ships; kept for the A/B record) ---- */
/* Self-attention INSIDE the projection chain (round 4): simulst_decoder_self_attention + simulst_decoder_proj_chain in ONE launch,
 * same results bit for bit.  qkv [B][3*256] = this step's q | k | v rows (fairseq MultiheadAttention in_proj of the decoder layer's
 * self-attention; witness models/cif_transformer.py:405-470), k_cache / v_cache [B][4][cap][64] updated in place at position
 * n_prev[b], x [B][256] the residual row (in: before the self-attention block, out: after it), q = wq LN(x) + bq, q2 likewise when
 * wq2_fm != NULL (the soft-energy query of MMA variants, modules/monotonic_multihead_attention.py:88-130), or, when kk_gelu != NULL,
 * q = gelu(wq LN(x) + bq + kk_gelu[b]) (CIF FakeCrossAttn, models/cif_transformer.py:357-362).  A workgroup owns
 * rows_per_workgroup rows (0: chosen from B; 4, 8 or 16) and its wave w runs head w.  n_prev_uniform >= 0: every row holds exactly
 * that many cached positions (lockstep batches: n_prev[] is not read, and below 64 the 8-pass instantiation runs).  bf16, 4 heads x 64, cap <= 128,
 * fragment-major weights (simulst_pack_fragment_major). */
int simulst_decoder_attn_proj_chain(simulst_handle* h, const void* qkv, void* k_cache, void* v_cache, const int32_t* n_prev,
                                    void* x, const void* wo_fm, const float* bo, const float* ln_g, const float* ln_b,
                                    const void* wq_fm, const float* bq, void* q, const void* wq2_fm, const float* bq2, void* q2,
                                    const void* kk_gelu, int32_t B, int32_t H, int32_t d, int32_t cap, int32_t n_prev_uniform,
                                    int32_t rows_per_workgroup, int32_t dtype);
#endif  /* SIMULST_EXPERIMENTS */

/* Pooled monotonic keys for fixed pre-decision with 'average' pooling (modules/fixed_pre_decision.py:23-29,104-110): for the
 * windows j in [j_lo, j_hi) that are complete for row b ((j + 1) * ratio <= key_len[b]), Kpool[b][h][j][:] = mean of frames
 * [j * ratio, (j + 1) * ratio) of Kmono [B][H][S_cap][head_dim] -- the sum in frame order divided by ratio, exactly what the policy
 * computes from the frames at every step when no cache is given.  Called once per batch of new encoder frames; a window that is
 * still incomplete (only the first one while key_len < ratio, :123-131) is pooled from its frames by the policy as before. */
int simulst_pool_keys(simulst_handle* h, const void* Kmono, float* Kpool, const int32_t* key_len, int32_t B, int32_t H, int32_t d,
                      int32_t S_cap, int32_t P_cap, int32_t ratio, int32_t j_lo, int32_t j_hi, int32_t dtype);

/* policy + cross-attention of one layer for one step in ONE launch (simulst_step_p_choose +
 * simulst_mma_step_search + simulst_decoder_cross_attention, same results). qm/qs: monotonic / soft
 * queries [B][D] (qm unused for WAITK and FULL, qs unused for HARD).  FULL: no policy, ctx = softmax over
 * the key_len[b] keys of Ksoft; tgt_idx and Kmono may be NULL, head_step / head_read are not touched (may be NULL).
 * An EMPTY source (key_len[b] == 0, reachable: the offline decode entry points take the caller's lengths as they are) gives what
 * the three calls give: step probabilities all zero, head_step = 0, head_read = !mass_preservation, a zero ctx row, and no key or
 * value row is loaded for the gather. */
int simulst_policy_cross_attention(simulst_handle* h, const void* qm, const void* qs, const void* Kmono,
                                   const void* Ksoft, const void* Vc, float energy_bias, const int32_t* key_len,
                                   const int32_t* tgt_idx, int64_t* head_step, uint8_t* head_read, void* ctx,
                                   int32_t B, int32_t H, int32_t d, int32_t S_cap, int32_t ratio, int32_t attn_type,
                                   int32_t waitk_k, int32_t online, int32_t mass_preservation, int32_t dtype);

/* ---- whole-target (teacher-forced) decoder pass ------------------------------------
 * The train-mode FORWARD of MMADecoder (models/mma_model.py:156-220, modules/monotonic_multihead_attention.py:301-352) over a known
 * target of U positions at once; csrc/teacher_forced.hip.  All three products run on the matrix cores: bf16 MFMAs for bf16
 * activations, fp32 MFMAs for fp32 activations; fp32 accumulation in both.  head_dim <= 64, B * H <= 65535.
 *
 * Causal self-attention: qkv [B][U][3D] -> ctx [B][U][D], query u attends keys 0 .. u (fairseq's buffered_future_mask; no
 * target padding mask, as in the reference).  Scores and softmax in fp32 (the fp32 scores are scaled by head_dim^-0.5 after the
 * first product, so q enters it as given), P.V accumulated in fp32, one rounding to the activation dtype at the store.  With bf16
 * activations the probabilities are ALSO rounded to bf16, as the A operand of the second product (the normaliser sums the unrounded
 * exponentials): one rounding more than simulst_decoder_self_attention, which keeps P in fp32.  Keys are tiled with a running
 * maximum and sum, so U is not bounded by LDS. */
int simulst_decoder_self_attention_causal(simulst_handle* h, const void* qkv, void* ctx, int32_t B, int32_t U, int32_t H,
                                          int32_t d, int32_t dtype);

/* Head energies of every (target, source) pair: q [B][U][D] (projected; scaled by head_dim^-0.5 inside), K [B][H][S_cap][head_dim]
 * (the cached head-major projections) -> out [B*H][U][S] fp32, 0 < S <= S_cap <= 4096.
 *   SOFT      raw energies over all S keys; no padding fill (simulst_expected_soft_attention masks by key_len itself)
 *   MONOTONIC p_choose of a learned policy in train mode: keys pooled over the PADDED source (ceil(S / |ratio|) windows, no floor
 *             trim; sign of ratio = pooling type as in simulst_step_p_choose, 'last' needs S >= |ratio|), energy + energy_bias,
 *             -1e8 on pooled positions j > 0 whose window holds more than pad_threshold padding (key_len [B], NULL: none),
 *             sigmoid, zero-inserted to source resolution with column S - 1 taking the last pooled value
 *             (modules/fixed_pre_decision.py:97-167).  ratio 1: no pooling.
 *   WAITK     q, K unused (may be NULL): target u is the one-hot of pooled position u + waitk_k - 1 clipped to the last pooled
 *             position that mask leaves valid (utils/p_choose_strategy.py:6-53, online unset), zero-inserted the same way. */
enum { SIMULST_ENERGY_SOFT = 0, SIMULST_ENERGY_MONOTONIC = 1, SIMULST_ENERGY_WAITK = 2 };
int simulst_mma_energy(simulst_handle* h, const void* q, const void* K, float* out, const int32_t* key_len, float energy_bias,
                       float pad_threshold, int32_t B, int32_t U, int32_t S, int32_t S_cap, int32_t H, int32_t d, int32_t ratio,
                       int32_t mode, int32_t waitk_k, int32_t dtype);

/* In-place softmax over the key_len[b] (NULL: S) valid keys of every row of energy [B*H][U][S] fp32, zeros behind them: the
 * attention weights of full encoder-decoder attention (SIMULST_ATTN_FULL) from SOFT energies. */
int simulst_mma_softmax(simulst_handle* h, float* energy, const int32_t* key_len, int32_t B, int32_t U, int32_t S, int32_t H);

/* Expected context: beta [B*H][U][S] fp32, cast to the activation dtype first (the reference's beta.to(v.dtype)), times
 * V [B][H][S_cap][head_dim] -> ctx [B][U][D], accumulated in fp32.  Replaces modules/monotonic_multihead_attention.py:401-409
 * for a whole target. */
int simulst_mma_context(simulst_handle* h, const float* beta, const void* V, void* ctx, int32_t B, int32_t U, int32_t S,
                        int32_t S_cap, int32_t H, int32_t d, int32_t dtype);

/* ---- transducer inference (models/transducer_model.py:28-212; csrc/transducer.hip) ----------------------------------------
 * Every entry point below refuses with SIMULST_E_ARG, BEFORE it looks at a pointer: an unknown dtype, D % 32 != 0, V < 4, k < 1,
 * S' < 1 (T_max < 1), a blank index outside [0, V), n_split outside [1, 64].
 *
 * AvgPool1dTBCPad (:79-98): x [B][S_in][D] rows (batch stride x_batch_stride elements), lengths [B], T_max = the batch's longest
 * valid length (the reference's time dimension, <= S_in), window k.  y [B][S'][D], S' = ceil(T_max / k):
 *   y[b][j] = (sum of x[b][t], t in [jk, min(jk + k, T_max)), t < lengths[b]) / (min(jk + k, T_max) - jk)
 *   times k / r at j = (lengths[b] - 1) / k when lengths[b] < T_max, r = (lengths[b] - 1) % k + 1   -- so a row's pooled states
 *   depend on the batch's T_max; positions j >= ceil(lengths[b] / k) are zero.  new_len[b] = ceil(lengths[b] / k). */
int simulst_transducer_pool(simulst_handle* h, const void* x, const int32_t* lengths, void* y, int32_t* new_len, int32_t B,
                            int32_t S_in, int32_t D, int64_t x_batch_stride, int32_t T_max, int32_t k, int32_t dtype);

/* Joiner scan of one decode step (:60-76 with one target position, the argmax of :191).  P fp32 [B][S][D] = source_projection of
 * the pooled states, g fp32 [B][D] = target_projection of the prediction network's output, W_fm = simulst_pack_fragment_major of
 * the output projection [ceil(V / 16) * 16][D] (rows >= V zero) in the model dtype.  For every (b, s) with
 * clamp(prev_emit[b], 0, src_len[b] - 1) <= s < src_len[b], logits = W . tanh(P[b][s] + g[b]) (the tanh rounded to the model
 * dtype, fp32 accumulation) and part p of the n_split column ranges:
 *   blank_logit[b][s]           the logit of column `blank` (written by the part that holds that column)
 *   best[b][s][p], best_idx[..] the largest logit of the part's columns other than `blank` and its lowest index
 *                               (-inf / INT32_MAX for a part without such a column)
 * Other positions of the outputs are not written; the [B][S][V] logits never exist.  Row tiles of 16 positions that lie wholly
 * outside the scanned range are skipped.
 * An OPEN source (simultaneous decoding): src_len[b] = -1 - a < 0 says that a pooled positions of row b are available so far
 * (a clamped to [0, S]) and that more may follow (0 stays what it is, a closed source without a position, so the open count is
 * offset by one: open with nothing available is -1).  The scanned range is then [clamp(prev_emit[b], 0, a), a) -- empty for
 * a == 0 or prev_emit[b] >= a --, same arithmetic, same tile skipping.  src_len[b] >= 0 is the closed source described above. */
int simulst_joiner_scan(simulst_handle* h, const float* P, const float* g, const void* W_fm, const int32_t* prev_emit,
                        const int32_t* src_len, float* blank_logit, float* best, int32_t* best_idx, int32_t B, int32_t S,
                        int32_t D, int32_t V, int32_t blank, int32_t n_split, int32_t dtype);

/* Emission (:170-209) from the scan's outputs: new_emit[b] = the first scanned s whose best non-blank logit beats the blank one
 * (ties go to the lower column, as torch.argmax), the blank logit taken as -1e4 at s = src_len[b] - 1.  prev_emit[b] <- new_emit[b],
 * z[b] = tanh(P[b][new_emit] + g[b]) in the model dtype ([B][D]; the returned vocabulary row is simulst_linear of it),
 * at_eos[b] = (new_emit[b] == src_len[b] - 1).
 * An OPEN source (src_len[b] = -1 - a < 0, see simulst_joiner_scan): no position gets the forced blank.  If a scanned s in
 * [clamp(prev_emit[b], 0, a), a) emits, the row does what a closed one does (same tie rule, prev_emit[b] <- s, z[b] written) with
 * at_eos[b] = 0.  Otherwise the row WAITS for more source: prev_emit[b] and z[b] are not written and at_eos[b] = -1. */
int simulst_joiner_emit(simulst_handle* h, const float* P, const float* g, const float* blank_logit, const float* best,
                        const int32_t* best_idx, int32_t* prev_emit, const int32_t* src_len, void* z, int32_t* at_eos, int32_t B,
                        int32_t S, int32_t D, int32_t V, int32_t blank, int32_t n_split, int32_t dtype);

/* The scan and the emission of one BEAM step: R rows of which every `group` consecutive ones (a sentence's beam rows) share one
 * source.  P [Bs][S][D], src_len [Bs] and finished [Bs] (int32, may be NULL) are read at r / group, Bs = R / group -- P is never
 * replicated; g [R][D], prev_emit [R], z [R][D], at_eos [R] and blank_logit [R][S], best / best_idx [R][S][n_split] are the row's.
 * The arithmetic of every (row, position, column) is simulst_joiner_scan's / simulst_joiner_emit's, and with group 1 and finished
 * NULL the two calls ARE those.  Rows of a finished sentence (finished[r / group] != 0) scan nothing -- their row tiles are empty
 * and take no matrix-core work -- and the emission leaves their prev_emit, z and at_eos as they are.  emit_log (int32 [R], one
 * row of the caller's [L][R] table, may be NULL) also receives the new emit position of every row that ran.  SIMULST_E_ARG as
 * above, and for group < 1 or R % group != 0.
 * An OPEN source (src_len[r / group] = -1 - a < 0) is read by both calls as by simulst_joiner_scan / simulst_joiner_emit: every
 * row of the group scans [clamp(prev_emit[r], 0, a), a) without a forced position, and a row that waits keeps prev_emit[r] and
 * z[r], gets at_eos[r] = -1 and emit_log[r] = -1.  (Beam search itself runs over closed sources only.) */
int simulst_joiner_scan_beam(simulst_handle* h, const float* P, const float* g, const void* W_fm, const int32_t* prev_emit,
                             const int32_t* src_len, const int32_t* finished, float* blank_logit, float* best, int32_t* best_idx,
                             int32_t R, int32_t group, int32_t S, int32_t D, int32_t V, int32_t blank, int32_t n_split,
                             int32_t dtype);
int simulst_joiner_emit_beam(simulst_handle* h, const float* P, const float* g, const float* blank_logit, const float* best,
                             const int32_t* best_idx, int32_t* prev_emit, const int32_t* src_len, const int32_t* finished, void* z,
                             int32_t* at_eos, int32_t* emit_log, int32_t R, int32_t group, int32_t S, int32_t D, int32_t V,
                             int32_t blank, int32_t n_split, int32_t dtype);

/* The transducer's state reorder of beam search (the role of reorder_incremental_state, :241-251), one launch: row r of the second
 * buffer set takes from row reorder[r] of the first the self-attention K/V positions [0, n_prev) of every layer (k_cache / v_cache
 * [R][H][cap][d], 16-byte copies, as simulst_beam_reorder) and prev_emit (prev_emit_src [R] -> prev_emit_dst [R]).  d gives
 * R = d->B, H, D, n_layers, cap and dtype; of the simulst_dec_layer entries only k_cache / v_cache are read.  `block` is the number
 * of rows a reorder may move within (1 <= block <= R, R % block == 0, no cap at 16): a beam driver passes beam, a driver that
 * reorders over the whole batch passes R.  Rows of finished blocks (finished [R / block], may be NULL) keep their own prev_emit and
 * copy no K/V.  A reorder that leaves its block is not performed (the row keeps its own state) and is added to result [1] int32
 * (device scratch, cleared by the caller).  R == 0 returns 0.  SIMULST_E_ARG: dtype, shape (more than 16 layers, head_dim % 8,
 * cap < 1), block, n_prev outside [0, cap]. */
int simulst_transducer_beam_reorder(simulst_handle* h, const simulst_decoder_desc* d, const simulst_dec_layer* src,
                                    const simulst_dec_layer* dst, const int32_t* prev_emit_src, int32_t* prev_emit_dst,
                                    const int32_t* reorder, const int32_t* finished, int32_t block, int32_t n_prev, int32_t* result);

/* logits fp32 [B][V]: column `blank` of the rows with at_eos[b] > 0 becomes -1e4 (the row gathered at :203-206 keeps the
 * scatter of :176-180); a row that waits on an open source (at_eos[b] = -1) is left alone. */
int simulst_joiner_mask_blank(simulst_handle* h, float* logits, const int32_t* at_eos, int32_t B, int32_t V, int32_t blank);

/* The joiner over a whole target (:143-163 with no incremental state, and what criterion/rnnt_criterion.py:82-147 reads from it):
 * P fp32 [B][S][D] as above, G fp32 [B][U1][D] = target_projection of the prediction network at every decoder-input position
 * (U1 = longest target + 1), W_fm as above, labels int32 [B][U1] (labels[b][u] = the token taken from input position u; values
 * outside [0, V) are clamped), src_len[b] (clamped to [0, S]) and tgt_len[b] = n_b, the target length with its EOS (clamped to
 * [0, U1 - 1]).  For every cell with s < src_len[b] and u <= tgt_len[b], logits = W . tanh(P[b][s] + G[b][u]) (the tanh rounded to
 * the model dtype, fp32 accumulation; no forced blank -- that edit is incremental-only) and
 *   lp_blank[b][s][u] = logits[blank]        - logsumexp(logits)
 *   lp_label[b][s][u] = logits[labels[b][u]] - logsumexp(logits)      for u < tgt_len[b]
 * both fp32 [B][S][U1]; other cells are not written.  The [B][S][U1][V] logits never exist: every vocabulary part p of n_split
 * leaves (max, sum of exp(. - max), blank logit, label logit) in partials, fp32 [B][S][U1][n_split][4] (a part that does not hold
 * the blank / label column leaves -1e30 there), and a fold kernel of the same call finishes them.  Row tiles that lie wholly
 * outside the valid cells are skipped.  SIMULST_E_ARG as above and for U1 < 1; SIMULST_E_SHAPE when the row panel
 * (128 rows bf16 / 64 rows fp32 of D + 8 / D + 4 elements) exceeds 144 KB of LDS. */
int simulst_joiner_lattice(simulst_handle* h, const float* P, const float* G, const void* W_fm, const int32_t* labels,
                           const int32_t* src_len, const int32_t* tgt_len, float* partials, float* lp_blank, float* lp_label,
                           int32_t B, int32_t S, int32_t U1, int32_t D, int32_t V, int32_t blank, int32_t n_split, int32_t dtype);

/* RNN-T forward recursion over lp_blank / lp_label fp32 [B][S][U1] (natural log; warp_rnnt's definition), per row with
 * S_b = src_len[b], n_b = tgt_len[b] (n_b == 0 is valid: the sum of the blanks):
 *   alpha[0][0] = 0,  alpha[s][u] = logaddexp(alpha[s-1][u] + lp_blank[s-1][u], alpha[s][u-1] + lp_label[s][u-1])
 *   ll[b] = alpha[S_b-1][n_b] + lp_blank[S_b-1][n_b]                   (-inf for S_b < 1)
 * One workgroup per row, anti-diagonals in LDS, fp32.  With best_ll, emit and backptr all non-NULL (all NULL otherwise) the same
 * recursion runs with max in place of logaddexp: best_ll[b] is the best single alignment's score, backptr (bytes, [B][S][U1],
 * scratch) holds one move per cell, and emit[b][u] int32 [B][U1] is the frame s at which label u is taken on that alignment, for
 * u < n_b (other entries are not written).  Tie rule: a cell takes the label move (from (s, u-1)) only when it is STRICTLY better
 * than the blank move (from (s-1, u)); on equal scores the blank move is kept, so the back-track from (S_b-1, n_b) places a tied
 * label at the earlier frame.  SIMULST_E_ARG: S < 1, U1 < 1, B < 0; SIMULST_E_SHAPE: U1 > 4096 (the diagonal does not fit in LDS --
 * refused, not truncated). */
int simulst_rnnt_forward(simulst_handle* h, const float* lp_blank, const float* lp_label, const int32_t* src_len,
                         const int32_t* tgt_len, float* ll, float* best_ll, int32_t* emit, uint8_t* backptr, int32_t B, int32_t S,
                         int32_t U1);

#ifdef __cplusplus
}
#endif
#endif /* SIMULST_HIP_H */
