// Path selection of the decoder step loops (simulst_mma_decode, simulst_mma_stream_steps, simulst_cif_decode,
// simulst_cif_stream_steps): which launches a step is made of is decided ONCE per call, here, from the handle's options, the
// descriptor's shapes and optional buffers and the call mode.  The loops read the plan; the leaves it is built from are the
// kernels' own predicates (sl_dec_chain_ok, sl_dec_attn_chain_ok, sl_dec_ffn_qkv_chain_ok, sl_dec_proj_cross_fused_ok,
// sl_dec_vocab_chain_split, sl_vocab_argmax_ok, sl_self_attention_fused_ok, sl_dec_tall_fc2_ok).  Host code only.
// Row classes of a step (handle.cpp thresholds): <= fuse_q_max_rows (128) the query projection rides in the policy launch;
// dec_chain_min_rows (129) .. dec_chain_ffn_max_rows (1024) projection chain + feed-forward chain; above, up to the decode-step GEMMs'
// row limit (8192), projection chain + three feed-forward launches, of which fc2 runs on the tall tile and, from panel_split_min_rows
// (2560) on, LN3 + fc1 + GELU on the two-stage panel of dec_gemm_tall.hip (each the bits of its simulst_linear launch).
#pragma once
#include "common.h"

// cross-attention over more keys than this runs in key blocks on their own workgroups + a merge (decode_driver.hip)
constexpr int SL_CROSS_KEY_BLOCK = 256;

enum { SL_CALL_OFFLINE = 0,      // host-stepped rows: lockstep (np_uniform >= 0) or ragged (-1)
       SL_CALL_GRAPH_STEP = 1,   // one device-indexed step (captured and replayed): positions are known to the device only
       SL_CALL_STREAM = 2 };     // per-row stream control: rows READ / WRITE independently, nothing is masked

// what the decision reads
struct sl_decode_call {
  int dtype, B, D, H, F, V, cap, S_cap, attn_type;      // B: rows every launch runs over (under compaction: the slots)
  bool packed;                                          // fragment-major weights
  bool x_mid, partial_self, ffn_partial, final_ln;      // optional buffers present
  int mode;                                             // SL_CALL_*
  int np_uniform;                                       // host-known position of lockstep rows, else -1
  bool compact, mask_eos;
  bool force_unfused;                                   // test hook: one launch per GEMM (MMA loops; the CIF loops never had it)
  bool cif;                                             // CIF decoder: no policy launch (nothing to fuse a query projection into), no
                                                        //   head-split block, its own commit kernel (pairs from the closing chain only)
  bool highway;                                         //   ... whose output projection reads LN(x) + c: no closing chain
};

// the path of every step of the call
struct sl_decode_plan {
  bool full_blocked;     // FULL attention over more than SL_CROSS_KEY_BLOCK keys: the blocked kernel reads a separate query
  bool split;            // head-split self-attention block (decode_fused.hip, EXPERIMENTS builds)
  bool fuse_q;           // LN2 + query projection(s) inside the policy / cross-attention launch
  bool chain;            // row-local projection chain (dec_chain.hip)
  bool chain_ffn;        // ... and feed-forward chain, its slabs added by the next LN + QKV launch
  bool attn_chain;       // self-attention inside the projection chain (EXPERIMENTS builds)
  bool proj_cross;       // projection chain + wait-k cross-attention in one launch (EXPERIMENTS builds; layers with one query projection)
  bool fuse_commit;      // a step's commit + next embedding ride in the next step's first launch with layer 0's LN + QKV
  bool fuse_ffn_qkv;     // feed-forward chain of layer l + slab sum, LN1, QKV of layer l + 1 in one launch (EXPERIMENTS builds)
  bool tall_ffn;         // no feed-forward chain (rows above dec_chain_ffn_max_rows): fc2 + residual on the pipelined tile of
                         //   dec_gemm_tall.hip instead of simulst_linear's k-interleaved one (the same bits: no row class of its own)
  bool tall_fc1;         //   ... and LN3 + fc1 + GELU on that file's two-stage row panel instead of the split row panel (the same bits)
  // how a step closes: vsplit > 0 the closing chain (slab sum + final LayerNorm + projection + partial pick over vsplit column ranges),
  // else tile_argmax: per-tile maxima out of the vocabulary GEMM's epilogue, else fp32 logits
  int vsplit;
  bool tile_argmax;
  int n_pairs;           // (value, index) pairs per row the commit folds; 0: it scans fp32 logits
};

sl_decode_plan sl_plan_decode(const simulst_handle* h, const sl_decode_call& c);

// simulst_mma_retire_rows: the row count below which a shrinking batch would leave the kernel class the plan put it in
int sl_retire_floor_rows(const simulst_handle* h, int B);

// ---- the parts of a layer that the MMA and the CIF loop launch alike ----------------------------------------------------------------
struct sl_step_bufs {                    // shapes and workspace of the call
  int dtype, B, D, F, packed;
  void *x, *x_mid, *qkv, *hidden;
  float* ffn_partial;
  int32_t* ffn_sem;
};
struct sl_qkv_weights { const float *ln_g, *ln_b; const void* w; const float* b; };
struct sl_ffn_weights { const void* c_wo; const float* c_bo; const float *ln_g, *ln_b; const void* fc1; const float* b1; const void* fc2; const float* b2; };
template <typename Layer> sl_qkv_weights sl_qkv_of(const Layer& L) { return {L.ln1_g, L.ln1_b, L.wqkv, L.bqkv}; }
template <typename Layer> sl_ffn_weights sl_ffn_of(const Layer& L) { return {L.c_wo, L.c_bo, L.ln3_g, L.ln3_b, L.fc1, L.b1, L.fc2, L.b2}; }

int sl_lin(simulst_handle* h, int dtype, int B, int N, int K, const void* A, const void* W, const float* bias, const void* R,
           void* C, int epi, const float* ln_g, const float* ln_b, int w_packed);
// The pipelined tall tile (dec_gemm_tall.hip).  shape_ok: bf16, fragment-major weights, and simulst_linear would run this fc2 on its
// k-interleaved tile without split-K -- the summation order the tall tile reproduces; fc2_ok: ... and the handle's option and row
// threshold admit it.  operands_ok: 16-byte aligned (row segments of R / C move as 16-byte vectors).
bool sl_dec_tall_fc2_shape_ok(const simulst_handle* h, int dtype, int B, int N, int K, bool packed);
bool sl_dec_tall_fc2_ok(const simulst_handle* h, int dtype, int B, int D, int F, bool packed);
static inline bool sl_dec_tall_operands_ok(const void* A, const void* W, const void* R, const void* C) {
  return (((uintptr_t)A | (uintptr_t)W | (uintptr_t)R | (uintptr_t)C) & 15) == 0;
}
int sl_dec_tall_fc2(simulst_handle* h, const void* A, const void* W, const float* bias, const void* R, void* C, int B, int N, int K);
// ... and fc1 (LN3 + GELU): taken where simulst_linear would run the split row panel (from panel_split_min_rows rows on; below, that
// launch is the 64 x 64 tile, whose MFMA operand roles differ: it keeps its kernel)
bool sl_dec_tall_fc1_shape_ok(const simulst_handle* h, int dtype, int B, int N, int K, bool packed);
bool sl_dec_tall_fc1_ok(const simulst_handle* h, int dtype, int B, int D, int F, bool packed);
int sl_dec_tall_fc1(simulst_handle* h, const void* A, const void* W, const float* bias, const float* ln_g, const float* ln_b, void* C,
                    int B, int N, int K);
// LN1 + QKV of layer l (prev_b2: fc2 bias of layer l - 1, whose feed-forward slabs a chained layer adds here first); nothing when the
// previous layer's feed-forward launch wrote them
int sl_step_qkv(simulst_handle* h, const sl_decode_plan& p, const sl_step_bufs& w, int l, const float* prev_b2, const sl_qkv_weights& q);
// cross out-proj + residual, LN3 + fc1 + GELU, fc2 + residual; next: the following layer's QKV weights, all null behind the last layer
int sl_step_ffn(simulst_handle* h, const sl_decode_plan& p, const sl_step_bufs& w, const void* ctx, const void* res,
                const sl_ffn_weights& f, const sl_qkv_weights& next);
// the last layer's slabs of a chained step that does not close with the vocabulary chain
int sl_step_last_slabs(simulst_handle* h, const sl_decode_plan& p, const sl_step_bufs& w, const float* last_b2);
