// Path selection of the decoder step loops, the retire floor that follows from it, and the launches the MMA and the CIF loop share
// (decode_plan.h).  Host code only.
#include "decode_plan.h"
#include "gemm_plan.h"

// the head-split self-attention block is an EXPERIMENTS build's (decode_fused.hip: measured slower); the product never plans it
#ifdef SL_EXPERIMENTS
static constexpr bool HEAD_SPLIT_BUILT = true;
#else
static constexpr bool HEAD_SPLIT_BUILT = false;
#endif

// The row classes of a step, in ascending order of their switch points (handle.cpp): up to fuse_q_max_rows the query projection
// rides inside the policy launch; from dec_chain_min_rows on sl_dec_chain_ok admits the layer chains; up to dec_chain_ffn_max_rows
// the feed-forward chain runs as well; above that the projection chain stays and the feed-forward block is three launches (cross
// out-proj + residual, LN3 + fc1 + GELU, fc2 + residual) -- the first two through simulst_linear, from dec_tall_min_rows on fc2, and from
// panel_split_min_rows on fc1 too, on the kernels of dec_gemm_tall.hip (tall_ffn, tall_fc1: the bits of the simulst_linear launches
// they replace, so no row class of their own and no entry in the retire floor).  The plan and the retire floor both read them here.
static bool rows_fuse_q(const simulst_handle* h, int B) { return B <= h->fuse_q_max_rows; }
static bool rows_chain_ffn(const simulst_handle* h, int B) { return B <= h->dec_chain_ffn_max_rows; }

// fc2 + residual as sl_step_ffn hands it to sl_lin: what simulst_linear would launch decides whether the tall tile may stand in
bool sl_dec_tall_fc2_shape_ok(const simulst_handle* h, int dtype, int B, int N, int K, bool packed) {
  if (dtype != SIMULST_BF16 || !packed || B <= 0 || N <= 0 || K <= 0) return false;
  LinArgs p = {};
  p.M = B; p.rpb = B; p.N = N; p.K = K;
  p.a_rs = K; p.c_rs = N; p.r_rs = N;
  p.scale = 1.f; p.w_packed = 1; p.amax_skip_a = p.amax_skip_b = -1;
  const sl_linear_ops o = {};
  const sl_linear_plan pl = sl_plan_linear(h, dtype, SIMULST_EPI_BIAS_RES, p, o);
  return pl.family == SL_LIN_SKINNY && pl.splits == 1;
}
bool sl_dec_tall_fc1_shape_ok(const simulst_handle* h, int dtype, int B, int N, int K, bool packed) {
  if (dtype != SIMULST_BF16 || !packed || B <= 0 || N <= 0 || K <= 0 || K > 256) return false;
  LinArgs p = {};
  p.M = B; p.rpb = B; p.N = N; p.K = K;
  p.a_rs = K; p.c_rs = N; p.r_rs = N;
  p.scale = 1.f; p.w_packed = 1; p.amax_skip_a = p.amax_skip_b = -1;
  p.ln_g = p.ln_b = (const float*)h;              // any non-null affine: the prologue is part of the shape test
  const sl_linear_ops o = {};
  const sl_linear_plan pl = sl_plan_linear(h, dtype, SIMULST_EPI_BIAS_GELU, p, o);
  return pl.family == SL_LIN_PANEL_SPLIT;
}
bool sl_dec_tall_fc1_ok(const simulst_handle* h, int dtype, int B, int D, int F, bool packed) {
  return h->dec_tall_ffn && B >= h->dec_tall_min_rows && sl_dec_tall_fc1_shape_ok(h, dtype, B, F, D, packed);
}
bool sl_dec_tall_fc2_ok(const simulst_handle* h, int dtype, int B, int D, int F, bool packed) {
  return h->dec_tall_ffn && B >= h->dec_tall_min_rows && sl_dec_tall_fc2_shape_ok(h, dtype, B, D, F, packed);
}

sl_decode_plan sl_plan_decode(const simulst_handle* h, const sl_decode_call& c) {
  sl_decode_plan p = {};
  const int d = c.D / c.H;
  const bool lockstep = c.mode == SL_CALL_OFFLINE && c.np_uniform >= 0;
  // Active-row compaction: a slot's state (caches, positions) lives at row_map[slot].  sl_self_attention and the policy launch take
  // the map; the launches that fold self- or cross-attention into a block or chain do not, so compacted rounds never plan them.
  const bool own_rows = !c.compact;
  p.full_blocked = c.attn_type == SIMULST_ATTN_FULL && c.S_cap > SL_CROSS_KEY_BLOCK && !c.force_unfused;
  // 5 launches per layer instead of 7 when the host supplied the partial buffer, the weights are fragment-major and the shapes fit
  p.split = HEAD_SPLIT_BUILT && own_rows && !c.cif && !p.full_blocked && c.packed && c.x_mid && c.partial_self && !c.force_unfused &&
            sl_self_attention_fused_ok(c.H, d, c.cap) && c.B <= 128 && (c.dtype == SIMULST_BF16 ? c.D <= 512 : c.D <= 256);
  // few rows: one launch less on the dependent chain; many rows: a GEMM of its own, no per-workgroup re-read of the projection weights
  p.fuse_q = !c.cif && (p.split || rows_fuse_q(h, c.B)) && !p.full_blocked;
  // { out-proj + residual, LN + q-proj(s) } in one launch, { cross out-proj + residual, LN + fc1 + GELU, fc2 + residual } in another.
  // The feed-forward chain is always launched in its hand-off-free form (x_mid given, slabs added by the next LN + QKV launch).
  // The MMA loop takes the projection chain with ffn_partial alone; the CIF loop asks for both buffers before it chains at all.
  p.chain = !p.split && !p.fuse_q && !c.force_unfused && c.ffn_partial && !(c.cif && !c.x_mid) &&
            sl_dec_chain_ok(h, c.dtype, c.B, c.D, c.F, c.packed);
  p.chain_ffn = p.chain && rows_chain_ffn(h, c.B) && c.x_mid;
  p.attn_chain = own_rows && p.chain && sl_dec_attn_chain_ok(h, c.dtype, c.B, c.H, d, c.cap);
  p.proj_cross = own_rows && !c.cif && p.chain && !p.attn_chain &&
                 sl_dec_proj_cross_fused_ok(h, c.dtype, c.B, c.H, d, c.S_cap, c.attn_type, lockstep, false);
  p.fuse_ffn_qkv = p.chain_ffn && !p.attn_chain && sl_dec_ffn_qkv_chain_ok(h, c.B, c.F);
  p.tall_ffn = !p.chain_ffn && !c.force_unfused && sl_dec_tall_fc2_ok(h, c.dtype, c.B, c.D, c.F, c.packed);
  p.tall_fc1 = !p.chain_ffn && !c.force_unfused && sl_dec_tall_fc1_ok(h, c.dtype, c.B, c.D, c.F, c.packed);
  // Greedy pick fused into the vocabulary projection: the masks must be known when the projection is launched.  Streaming masks
  // nothing, forced decoding masks pad + eos, free offline decoding masks eos only at position 0, which the host can tell only for
  // lockstep rows.
  const bool masks_known = c.mode == SL_CALL_STREAM || c.mask_eos || lockstep;
  p.vsplit = (p.chain_ffn && masks_known && h->fused_argmax && !c.highway)
                 ? sl_dec_vocab_chain_split(h, c.dtype, c.B, c.V, c.D, c.packed, c.final_ln) : 0;
  p.tile_argmax = !p.vsplit && !c.cif && masks_known && sl_vocab_argmax_ok(h, c.dtype, c.B, c.V, c.D, c.packed);
  p.n_pairs = p.vsplit ? p.vsplit : p.tile_argmax ? c.V / 64 : 0;
  // lockstep offline rows only (dec_embed_qkv_chain_kernel folds at most 64 pairs); the last step of a call commits on its own
  p.fuse_commit = !c.cif && p.chain_ffn && lockstep && h->dec_embed_qkv_chain && p.n_pairs > 0 && p.n_pairs <= 64;
  return p;
}

// A batch that retires rows keeps the launches, and with them the rounding, it started with: near-tied greedy picks flip between
// kernels.  So it never shrinks past a row switch point of the plan, nor past one of the GEMM dispatch behind the plan's sl_lin and
// vocabulary launches (the tile kernels and the skinny kernel below them round differently).  Every switch point counts whether or
// not the batch's dtype and buffers let it take the path above it.  Tiles of 16 rows, at most the batch.
int sl_retire_floor_rows(const simulst_handle* h, int B) {
  int f = 1;
  if (!rows_chain_ffn(h, B)) f = h->dec_chain_ffn_max_rows + 1;               // layer chains without the feed-forward chain
  else if (B >= h->dec_chain_min_rows) f = h->dec_chain_min_rows;             // layer chains
  else if (!rows_fuse_q(h, B)) f = h->fuse_q_max_rows + 1;                    // separate query projection, no chains
  for (int t : {TILE_MIN_ROWS, h->mid_narrow_min_rows, h->panel_split_min_rows})      // gemm_plan.cpp plan_decode_step
    if (B >= t && f < t) f = t;
  if (B > SKINNY_MAX_ROWS_PACKED) f = B;                                      // beyond the decode-step GEMMs' row limit
  return min((f + 15) / 16 * 16, B);
}

int sl_lin(simulst_handle* h, int dtype, int B, int N, int K, const void* A, const void* W, const float* bias, const void* R,
           void* C, int epi, const float* ln_g, const float* ln_b, int w_packed) {
  simulst_linear_desc d;
  d.M_batches = 1; d.rows_per_batch = B; d.N = N; d.K = K;
  d.a_batch_stride = 0; d.a_row_stride = K; d.a_lead = 0;
  d.c_batch_stride = 0; d.c_row_stride = N;
  d.r_batch_stride = 0; d.r_row_stride = N;
  d.epilogue = epi; d.dtype = dtype; d.scale = 1.f; d.n_main = 0; d.aux_rows = 0; d.aux_batch_stride = 0;
  d.ln_gamma = ln_g; d.ln_beta = ln_b; d.w_fragment_major = w_packed; d.c_head_dim = 0; d.c_head_stride = 0; d.c_tensor_heads = 0; d.c_tensor_stride = 0;
  return simulst_linear(h, &d, A, W, bias, R, C, nullptr);
}

int sl_step_qkv(simulst_handle* h, const sl_decode_plan& p, const sl_step_bufs& w, int l, const float* prev_b2, const sl_qkv_weights& q) {
  if (l > 0 && p.fuse_ffn_qkv) return SIMULST_OK;        // x and qkv of this layer were written by the previous layer's launch
  if (l > 0 && p.chain_ffn)                              // the previous layer's feed-forward slabs are added here, then LN1 + QKV
    return sl_dec_qkv_chain(h, w.x_mid, w.x, w.ffn_partial, prev_b2, q.ln_g, q.ln_b, q.w, q.b, w.qkv, w.B, w.F);
  return sl_lin(h, w.dtype, w.B, 3 * w.D, w.D, w.x, q.w, q.b, nullptr, w.qkv, SIMULST_EPI_BIAS, q.ln_g, q.ln_b, w.packed);
}

int sl_step_ffn(simulst_handle* h, const sl_decode_plan& p, const sl_step_bufs& w, const void* ctx, const void* res,
                const sl_ffn_weights& f, const sl_qkv_weights& next) {
  if (p.chain_ffn && p.fuse_ffn_qkv && next.w)
    return sl_dec_ffn_qkv_chain(h, ctx, w.x, f.c_wo, f.c_bo, f.ln_g, f.ln_b, f.fc1, f.b1, f.fc2, f.b2, w.ffn_partial, w.B, w.F,
                                next.ln_g, next.ln_b, next.w, next.b, w.qkv);
  if (p.chain_ffn)
    return sl_dec_ffn_chain(h, ctx, w.x, f.c_wo, f.c_bo, f.ln_g, f.ln_b, f.fc1, f.b1, f.fc2, f.b2, w.ffn_partial, w.ffn_sem, w.x_mid,
                            w.B, w.F);
  int rc;
  if ((rc = sl_lin(h, w.dtype, w.B, w.D, w.D, ctx, f.c_wo, f.c_bo, res, w.x, SIMULST_EPI_BIAS_RES, nullptr, nullptr, w.packed))) return rc;
  // (the workspace rows and packed weights of a decode call are whole allocations or 16-byte multiples into them, and the launches
  //  around these read the same buffers with 16-byte loads: the alignment test guards the tall tiles' vector accesses of a caller's
  //  odd buffer, which then takes the simulst_linear launch -- the same bits, its own timer class)
  if (p.tall_fc1 && f.ln_g && f.ln_b && sl_dec_tall_operands_ok(w.x, f.fc1, w.hidden, f.b1))
    rc = sl_dec_tall_fc1(h, w.x, f.fc1, f.b1, f.ln_g, f.ln_b, w.hidden, w.B, w.F, w.D);
  else
    rc = sl_lin(h, w.dtype, w.B, w.F, w.D, w.x, f.fc1, f.b1, nullptr, w.hidden, SIMULST_EPI_BIAS_GELU, f.ln_g, f.ln_b, w.packed);
  if (rc) return rc;
  if (p.tall_ffn && sl_dec_tall_operands_ok(w.hidden, f.fc2, w.x, w.x))
    return sl_dec_tall_fc2(h, w.hidden, f.fc2, f.b2, w.x, w.x, w.B, w.D, w.F);
  return sl_lin(h, w.dtype, w.B, w.D, w.F, w.hidden, f.fc2, f.b2, w.x, w.x, SIMULST_EPI_BIAS_RES, nullptr, nullptr, w.packed);
}

int sl_step_last_slabs(simulst_handle* h, const sl_decode_plan& p, const sl_step_bufs& w, const float* last_b2) {
  if (!p.chain_ffn || p.vsplit) return SIMULST_OK;
  return sl_dec_qkv_chain(h, w.x_mid, w.x, w.ffn_partial, last_b2, nullptr, nullptr, nullptr, nullptr, nullptr, w.B, w.F);
}
