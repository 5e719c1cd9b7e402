// Launchers of csrc/dec_chain.hip's measured-slower forms (`make EXPERIMENTS=1` only; included by dec_chain.hip after its launch helpers
// -- lds_request, SL_XMODE, SL_CHAIN_TAIL, raise_lds_limits' declaration -- and before the product launchers).  The product build has one-line stubs
// instead (dec_chain.hip), so no launch function of the product carries a build switch.

// row tiles per workgroup of the projection / feed-forward / QKV chains: 2 (32 rows, round 5: a weight fragment serves two row tiles, half
// the L2 -> CU weight stream these launches are bound by) from dec_chain_rows32_min rows on, else 1
// MEASURED (driver form, same box): 96.8 ms per pass against 91.2 -- a chain workgroup is paced by ITS OWN weight stream (the per-CU
// L2 -> CU rate, ~50 GB/s: 256 KB of the projection chain in ~5 us), not by the chip-wide one, so half as many workgroups doing twice
// the rows each stream as long and finish later.  EXPERIMENTS builds only, off.
static int chain_rtl(const simulst_handle* h, int B) { return h->dec_chain_rows32 && B >= h->dec_chain_rows32_min ? 2 : 1; }

// this file's part of raise_lds_limits' list (dec_chain.hip), per fragment-read mode
#define SL_EXP_CHAIN_LDS_LIMITS(XM)                                                                                    \
  {(const void*)dec_ffn_qkv_chain_kernel<1, XM>, LDS_WHOLE_CU}, {(const void*)dec_proj_chain_kernel<2, XM>, LDS_WHOLE_CU},            \
  {(const void*)dec_ffn_chain_kernel<2, false, XM>, LDS_WHOLE_CU}, {(const void*)dec_qkv_chain_kernel<2, XM>, LDS_WHOLE_CU},

// the three chains on 32-row tiles: true = launched (the caller then skips its 16-row launch)
static bool exp_proj_chain_rows32(simulst_handle* h, const void* ctx, void* x, const void* Wo, const float* bo, const float* ln_g,
                                  const float* ln_b, const void* Wq, const float* bq, void* q, const void* Wq2, const float* bq2,
                                  void* q2, int B, const void* kk_gelu) {
  if (chain_rtl(h, B) != 2 || SL_CHAIN_TAIL(h)) return false;
#define PC2(XM)                                                                                                        \
  hipLaunchKernelGGL((dec_proj_chain_kernel<2, XM>), dim3((B + 31) / 32), dim3(256), lds_request(h, 2), h->stream,     \
                     (const bf16*)ctx, (bf16*)x, (const uint4*)Wo, bo, ln_g, ln_b, (const uint4*)Wq, bq, (bf16*)q,     \
                     (const uint4*)Wq2, bq2, (bf16*)q2, B, SL_CHAIN_TAIL(h), (const bf16*)kk_gelu)
  SL_XMODE(h, PC2);
#undef PC2
  return true;
}

static bool exp_ffn_chain_rows32(simulst_handle* h, const void* ctx, void* x, const void* Wco, const float* bco, const float* ln_g,
                                 const float* ln_b, const void* W1, const float* b1, const void* W2, const float* b2, float* partial,
                                 int32_t* sem, void* x_mid, int B, int F) {
  if (chain_rtl(h, B) != 2) return false;
  const int splits = F / 256;
#define FC2(XM)                                                                                                        \
  hipLaunchKernelGGL((dec_ffn_chain_kernel<2, false, XM>), dim3(((B + 31) / 32) * splits), dim3(256), lds_request(h, 2), \
                     h->stream, (const bf16*)ctx, (bf16*)x, (const uint4*)Wco, bco, ln_g, ln_b, (const uint4*)W1, b1,  \
                     (const uint4*)W2, b2, partial, sem, (bf16*)x_mid, B, F, splits)
  SL_XMODE(h, FC2);
#undef FC2
  return true;
}

static bool exp_qkv_chain_rows32(simulst_handle* h, const void* x_mid, void* x, const float* partial, const float* b2, const float* ln_g,
                                 const float* ln_b, const void* Wqkv, const float* bqkv, void* qkv, int B, int F) {
  if (chain_rtl(h, B) != 2) return false;
  const int splits = F / 256, n_cb = 3;
#define QC2(XM)                                                                                                        \
  hipLaunchKernelGGL((dec_qkv_chain_kernel<2, XM>), dim3(((B + 31) / 32) * n_cb), dim3(256), lds_request(h, 2),        \
                     h->stream, (const bf16*)x_mid, (bf16*)x, partial, b2, ln_g, ln_b, (const uint4*)Wqkv, bqkv,       \
                     (bf16*)qkv, B, splits, n_cb)
  SL_XMODE(h, QC2);
#undef QC2
  return true;
}

// EXPERIMENT: projection chain + wait-k cross-attention of a layer in one launch (dec_proj_cross_fused_kernel)
bool sl_dec_proj_cross_fused_ok(const simulst_handle* h, int dtype, int B, int H, int d, int S_cap, int attn_type, bool lockstep_offline,
                                bool separate_soft) {
  return h->dec_fuse_proj_cross && dtype == SIMULST_BF16 && H * d == CD && d == 64 && S_cap <= 256 && attn_type == SIMULST_ATTN_WAITK &&
         lockstep_offline && !separate_soft && (B + 15) / 16 <= 1000;
}

int sl_dec_proj_cross_fused(simulst_handle* h, const void* ctx_in, void* x, const void* Wo, const float* bo, const float* ln_g,
                            const float* ln_b, const void* Wq, const float* bq, void* q, const void* Ks, const void* Vc,
                            const int32_t* key_len, const int32_t* tgt_idx, int64_t* head_step, uint8_t* head_read, void* ctx_out, int B,
                            int H, int S_cap, int ratio, int waitk_k, int online, int mass_pres, int n_hint) {
  if (int rc = raise_lds_limits(h)) return rc;
  if (!h->fuse_flags) {
    hipError_t e = hipMalloc((void**)&h->fuse_flags, 1024 * sizeof(int));
    if (e == hipSuccess) e = hipMemsetAsync(h->fuse_flags, 0, 1024 * sizeof(int), h->stream);
    if (e != hipSuccess) { h->err = "simulst_mma_decode: flag words of the fused projection / cross-attention launch"; return (int)e; }
    h->fuse_epoch = 0;
  }
  const int n_tiles = (B + 15) / 16;
  const int epoch = ++h->fuse_epoch;
  KTimer t(h, SIMULST_K_DEC_CROSS_ATTN);
  // dynamic LDS: the chain's row buffers (lds_request) cover the attention's reduction scratch (64 + RED_FLOATS floats)
  const int lds = lds_request(h) > (int)((64 + attn::RED_FLOATS) * sizeof(float)) ? lds_request(h) : (int)((64 + attn::RED_FLOATS) * sizeof(float));
  // the attention workgroups are persistent: as many as stay resident beside the chain (2 per compute unit), each walks its problems
  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0);
  const int slots = 2 * cus - n_tiles;
  const int n_attn = H * B < slots ? H * B : (slots > 64 ? slots : 64);
  hipLaunchKernelGGL((dec_proj_cross_fused_kernel<3>), dim3(n_tiles + n_attn), dim3(256), lds, h->stream, (const bf16*)ctx_in, (bf16*)x,
                     (const uint4*)Wo, bo, ln_g, ln_b, (const uint4*)Wq, bq, (bf16*)q, B, n_tiles, h->fuse_flags, epoch, (const bf16*)Ks,
                     (const bf16*)Vc, key_len, tgt_idx, (long*)head_step, head_read, (bf16*)ctx_out, H, S_cap, ratio, waitk_k, online,
                     mass_pres, n_hint);
  return sl_launch_status(h, "simulst_mma_decode(projection chain + wait-k cross-attention, one launch)");
}

// feed-forward chain of a layer + slab sum, LayerNorm and QKV projection of the NEXT layer in one launch (dec_ffn_qkv_chain_kernel)
constexpr int CHAIN_SEM_TILES = 4096;
bool sl_dec_ffn_qkv_chain_ok(const simulst_handle* h, int B, int F) {
  return h->dec_fuse_ffn_qkv && F / 256 >= 3 && (B + 15) / 16 <= CHAIN_SEM_TILES;
}

int sl_dec_ffn_qkv_chain(simulst_handle* h, const void* ctx, void* x, const void* Wco, const float* bco, const float* ln_g,
                         const float* ln_b, const void* W1, const float* b1, const void* W2, const float* b2, float* partial, int B,
                         int F, const float* nln_g, const float* nln_b, const void* nWqkv, const float* nbqkv, void* qkv) {
  if (int rc = raise_lds_limits(h)) return rc;
  const int splits = F / 256;
  if (!h->chain_sem) {
    hipError_t e = hipMalloc((void**)&h->chain_sem, CHAIN_SEM_TILES * sizeof(int));
    if (e != hipSuccess) { h->err = "simulst_mma_decode: ticket words of the feed-forward + QKV launch"; return (int)e; }
    h->chain_sem_splits = 0;
  }
  if (h->chain_sem_splits != splits) {                           // the tickets count in units of `splits`: restart them in stream order
    const hipError_t e = hipMemsetAsync(h->chain_sem, 0, CHAIN_SEM_TILES * sizeof(int), h->stream);
    if (e != hipSuccess) { h->err = "simulst_mma_decode: ticket words of the feed-forward + QKV launch"; return (int)e; }
    h->chain_sem_splits = splits;
  }
  KTimer t(h, SIMULST_K_DEC_FFN_CHAIN);
#define FQ(XM)                                                                                                         \
  hipLaunchKernelGGL((dec_ffn_qkv_chain_kernel<1, XM>), dim3(((B + 15) / 16) * splits), dim3(256), lds_request(h),     \
                     h->stream, (const bf16*)ctx, (bf16*)x, (const uint4*)Wco, bco, ln_g, ln_b, (const uint4*)W1, b1,  \
                     (const uint4*)W2, b2, partial, h->chain_sem, B, F, splits, nln_g, nln_b, (const uint4*)nWqkv, nbqkv, \
                     (bf16*)qkv, 3)
  SL_XMODE(h, FQ);
#undef FQ
  return sl_launch_status(h, "simulst_mma_decode(feed-forward chain + next layer's LN + QKV)");
}


// self-attention + projection chain in one launch (dec_attn_proj_chain_kernel): bf16, 4 heads x 64, cache capacity <= 128
bool sl_dec_attn_chain_ok(const simulst_handle* h, int dtype, int B, int H, int d, int cap) {
  return dtype == SIMULST_BF16 && H == 4 && d == 64 && cap <= 128 && !h->force_valu_attention && B <= h->dec_attn_chain_max_rows;
}

int sl_dec_attn_proj_chain(simulst_handle* h, const void* qkv, void* k_cache, void* v_cache, const int32_t* n_prev, int np_uniform,
                           int cap, void* x, const void* Wo, const float* bo, const float* ln_g, const float* ln_b, const void* Wq,
                           const float* bq, void* q, const void* Wq2, const float* bq2, void* q2, int B, const void* kk_gelu) {
  SL_REQUIRE(h, np_uniform < cap, SIMULST_E_SHAPE, "simulst_decoder_attn_proj_chain: cache capacity exceeded");
  KTimer t(h, SIMULST_K_DEC_ATTN_CHAIN);
  // rows per workgroup: 4 while that gives at most ~160 workgroups (each pulls 256 KB of weights from L2), 8 beyond
  const int vr = h->dec_attn_chain_rows > 0 ? h->dec_attn_chain_rows : (B <= 640 ? 4 : 8);
  const bool few = np_uniform >= 0 && np_uniform < 64;       // every row holds < 64 cached positions: 8 passes cover them
#define AC(VR, MAXP)                                                                                                   \
  hipLaunchKernelGGL((dec_attn_proj_chain_kernel<VR, MAXP, 3>), dim3((B + VR - 1) / VR), dim3(256), 0, h->stream,      \
                     (const bf16*)qkv, (bf16*)k_cache, (bf16*)v_cache, n_prev, np_uniform, cap, (bf16*)x, (const uint4*)Wo, bo, \
                     ln_g, ln_b, (const uint4*)Wq, bq, (bf16*)q, (const uint4*)Wq2, bq2, (bf16*)q2, B, (const bf16*)kk_gelu)
  if (vr == 4) { if (few) AC(4, 8); else AC(4, 16); }
  else if (vr == 8) { if (few) AC(8, 8); else AC(8, 16); }
  else { if (few) AC(16, 8); else AC(16, 16); }
#undef AC
  return sl_launch_status(h, "simulst_mma_decode(self-attention + out-proj + LN + q-proj chain)");
}

extern "C" int simulst_decoder_attn_proj_chain(simulst_handle* h, const void* qkv, void* k_cache, void* v_cache,
                                               const int32_t* n_prev, void* x, const void* wo_fm, const float* bo,
                                               const float* ln_g, const float* ln_b, const void* wq_fm, const float* bq, void* q,
                                               const void* wq2_fm, const float* bq2, void* q2, const void* kk_gelu, int32_t B,
                                               int32_t H, int32_t d, int32_t cap, int32_t n_prev_uniform,
                                               int32_t rows_per_workgroup, int32_t dtype) {
  if (!h) return SIMULST_E_NULL;
  SL_CHECK_NULL(h, qkv); SL_CHECK_NULL(h, k_cache); SL_CHECK_NULL(h, v_cache); SL_CHECK_NULL(h, x);
  if (n_prev_uniform < 0) SL_CHECK_NULL(h, n_prev);
  SL_CHECK_NULL(h, wo_fm); SL_CHECK_NULL(h, bo); SL_CHECK_NULL(h, ln_g); SL_CHECK_NULL(h, ln_b); SL_CHECK_NULL(h, wq_fm);
  SL_CHECK_NULL(h, q);
  if (wq2_fm) { SL_CHECK_NULL(h, bq2); SL_CHECK_NULL(h, q2); }
  SL_REQUIRE(h, !(wq2_fm && kk_gelu), SIMULST_E_ARG, "simulst_decoder_attn_proj_chain: a second query projection or the gathered-row GELU, not both");
  SL_REQUIRE(h, dtype == SIMULST_BF16, SIMULST_E_DTYPE, "simulst_decoder_attn_proj_chain: bf16 only");
  SL_REQUIRE(h, H == 4 && d == 64 && cap > 0 && cap <= 128 && B >= 0, SIMULST_E_SHAPE,
             "simulst_decoder_attn_proj_chain: 4 heads x 64, cache capacity <= 128");
  SL_REQUIRE(h, rows_per_workgroup == 0 || rows_per_workgroup == 4 || rows_per_workgroup == 8 || rows_per_workgroup == 16, SIMULST_E_ARG,
             "simulst_decoder_attn_proj_chain: rows_per_workgroup 0 (library's choice), 4, 8 or 16");
  if (B == 0) return SIMULST_OK;
  const int keep = h->dec_attn_chain_rows;
  if (rows_per_workgroup) h->dec_attn_chain_rows = rows_per_workgroup;
  const int rc = sl_dec_attn_proj_chain(h, qkv, k_cache, v_cache, n_prev, n_prev_uniform < 0 ? -1 : n_prev_uniform, cap, x, wo_fm, bo, ln_g, ln_b, wq_fm, bq, q, wq2_fm, bq2,
                                        q2, B, kk_gelu);
  h->dec_attn_chain_rows = keep;
  return rc;
}
