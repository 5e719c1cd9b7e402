// Handle lifecycle + timers of libsimulst_hip.so.
#include "ffn_variant.h"
#include <cstdlib>
#include <initializer_list>

// 100: rounds 1-2.  103: round 3 -- simulst_linear_desc, simulst_stream_ctl and simulst_cif_stream_ctl grew at their ends
// (c_tensor_heads / c_tensor_stride; the chunk schedules of self-paced rows), simulst_decoder_desc gained P_cap.
// 104: round 4 -- kernel classes 11-15 (one per layer-chain kernel), simulst_set_option replaces the two path-selection hooks,
// simulst_decoder_attn_proj_chain, the simulst_debug_* entry points only in DEBUG_HOOKS builds.
// 105: round 5 -- simulst_get_option (what a handle actually runs with, for the roofline models of bench.py).
// 106: round 6 -- simulst_emformer_ffn_prenorm (the next layer's LayerNorm + summaries in the feed-forward launch); no structure changed.
// 107: round 6 -- simulst_stream_ctl grew row_map / compact_rows (active-row compaction of simulst_mma_stream_steps).
// 108: round 6 -- simulst_emformer_ffn_prenorm_qkv (... and the next layer's Q | K | V projection of the rc | utterance rows) and
// simulst_emformer_qkv_mem_sum; no structure changed.
extern "C" int simulst_version(void) { return 108; }

// ---- the tunables: one row each ---------------------------------------------------------------------------------------------------
// Run-time options of a handle: path selection (each alternative is a complete, valid implementation -- the tests use them for
// A/B parity) and the tuning values that simulst_create reads from the environment.  A new tunable is a member of simulst_handle
// with its default (common.h), a row here and, if it is an option, its id in the header's enum.
//   env_ok / set_ok: the values the environment / simulst_set_option may give it; none: any (atoi of the text, as it is).  The
//   environment ignores a value outside, simulst_set_option refuses it with `refusal`.  A `flag` is stored as value != 0.
//   flavour: the build that has it (common.h); elsewhere the environment is not read and simulst_set_option refuses.
// Not rows, because they are not one value in one member: SIMULST_DEC_TALL_MIN_ROWS (its default depends on another row),
// PANEL_WIDE (one value, two members) and what simulst_get_option(DEC_FUSE_PROJ_CROSS) adds from the device.
namespace {

typedef bool (*legal_fn)(int);
bool one_of(int v, std::initializer_list<int> set) {
  for (int s : set) if (s == v) return true;
  return false;
}
#define ONE_OF(...) [](int v) { return one_of(v, {__VA_ARGS__}); }
#define RANGE(lo, hi) [](int v) { return v >= (lo) && v <= (hi); }
constexpr legal_fn ANY = nullptr;
constexpr legal_fn VOCAB_SPLITS = ONE_OF(0, 1, 2, 4, 8, 16);
constexpr legal_fn TILE256_FORMS = RANGE(0, 2);
constexpr legal_fn NOT_NEGATIVE = [](int v) { return v >= 0; };
constexpr int NO_OPTION = -1;
constexpr int EXP = SL_EXPERIMENTS_BUILD, DBG = SL_DEBUG_HOOKS_BUILD;

struct tunable {
  int option;
  const char* env;
  int simulst_handle::*member;
  bool flag;
  legal_fn env_ok, set_ok;
  int flavour;
  const char* refusal;
};

#define M(name) &simulst_handle::name
const tunable TUNABLES[] = {
    {SIMULST_OPT_VALU_ATTENTION, nullptr, M(force_valu_attention), true, ANY, ANY, SL_PRODUCT, ""},
    {SIMULST_OPT_UNFUSED_DECODE, nullptr, M(force_unfused_decode), true, ANY, ANY, SL_PRODUCT, ""},
    {SIMULST_OPT_FFN_WAVES, nullptr, M(ffn_waves), false, ANY, [](int v) { return sl_ffn_code_legal(v); }, SL_PRODUCT,
#ifdef SL_EXPERIMENTS
     "simulst_set_option(FFN_WAVES): 0 (the library's choice), 4 / 8 (GELU as a block between the products), 41 / 81 (GELU inside the "
     "MFMA stream, 4 / 8 waves; 42 / 82: packed GELU, DEBUG_HOOKS builds only), 43 / 83 (GELU spread over all 32 MFMAs; 47 / 87: LDS-DMA "
     "pieces as a burst / spread), 45 (64 rows per wave)"},
#else
     "simulst_set_option(FFN_WAVES): 0 (the library's choice: 43 while F <= 2048), 43 (GELU inside the MFMA stream), 4 / 8 (the block form "
     "with that many waves: GELU between the two products); the measured-slower forms exist in EXPERIMENTS builds"},
#endif
    {NO_OPTION, "SIMULST_PANEL_SPLIT_MIN_ROWS", M(panel_split_min_rows), false, ANY, ANY, SL_PRODUCT, ""},
    {NO_OPTION, "SIMULST_PANEL_SPLIT_BLOCKS", M(panel_split_blocks), false, ANY, ANY, SL_PRODUCT, ""},
    {NO_OPTION, "SIMULST_MID_MIN_BLOCKS", M(mid_min_blocks), false, ANY, ANY, SL_PRODUCT, ""},
    {NO_OPTION, "SIMULST_MID_NARROW_MIN_ROWS", M(mid_narrow_min_rows), false, ANY, ANY, SL_PRODUCT, ""},
    {NO_OPTION, "SIMULST_SKINNY_MIN_BLOCKS_TALL", M(skinny_min_blocks_tall), false, ANY, ANY, SL_PRODUCT, ""},
    {NO_OPTION, "SIMULST_FUSE_Q_MAX_ROWS", M(fuse_q_max_rows), false, ANY, ANY, SL_PRODUCT, ""},
    {NO_OPTION, "SIMULST_EA_GENERAL", M(ea_general_only), true, ANY, ANY, SL_PRODUCT, ""},
    {SIMULST_OPT_DEC_CHAIN, "SIMULST_DEC_CHAIN", M(dec_chain_on), true, ANY, ANY, SL_PRODUCT, ""},
    {NO_OPTION, "SIMULST_DEC_CHAIN_MIN_ROWS", M(dec_chain_min_rows), false, ANY, ANY, SL_PRODUCT, ""},
    {NO_OPTION, "SIMULST_DEC_CHAIN_MAX_ROWS", M(dec_chain_max_rows), false, ANY, ANY, SL_PRODUCT, ""},
    {NO_OPTION, "SIMULST_DEC_CHAIN_FFN_MAX_ROWS", M(dec_chain_ffn_max_rows), false, ANY, ANY, SL_PRODUCT, ""},
    {SIMULST_OPT_DEC_TALL_FFN, "SIMULST_DEC_TALL_FFN", M(dec_tall_ffn), true, ANY, ANY, SL_PRODUCT, ""},
    // investigation knobs (xmode: bitmask, bit 0 hoisted fragment reads, bit 1 DPP reductions; LDS request up to the CU's 160 KB)
    {NO_OPTION, "SIMULST_DEC_CHAIN_XMODE", M(dec_chain_xmode), false, RANGE(0, 3), ANY, DBG, ""},
    {NO_OPTION, "SIMULST_DEC_CHAIN_LDS_BYTES", M(dec_chain_lds_bytes), false, RANGE(0, 160 * 1024), ANY, DBG, ""},
    {SIMULST_OPT_DEC_ATTN_CHAIN_MAX_ROWS, "SIMULST_DEC_ATTN_CHAIN_MAX_ROWS", M(dec_attn_chain_max_rows), false, ANY, NOT_NEGATIVE, EXP,
     "simulst_set_option(DEC_ATTN_CHAIN_MAX_ROWS): >= 0; self-attention inside the projection chain exists in EXPERIMENTS builds only (measured slower)"},
    {SIMULST_OPT_DEC_ATTN_CHAIN_ROWS, "SIMULST_DEC_ATTN_CHAIN_ROWS", M(dec_attn_chain_rows), false, ONE_OF(4, 8, 16), ONE_OF(0, 4, 8, 16), EXP,
     "simulst_set_option(DEC_ATTN_CHAIN_ROWS): 0, 4, 8 or 16; self-attention inside the projection chain exists in EXPERIMENTS builds only (measured slower)"},
    {SIMULST_OPT_FUSED_ARGMAX, "SIMULST_FUSED_ARGMAX", M(fused_argmax), true, ANY, ANY, SL_PRODUCT, ""},
    {SIMULST_OPT_DEC_VOCAB_CHAIN_SPLIT, "SIMULST_DEC_VOCAB_CHAIN_SPLIT", M(dec_vocab_chain_split), false, VOCAB_SPLITS, VOCAB_SPLITS, SL_PRODUCT,
     "simulst_set_option(DEC_VOCAB_CHAIN_SPLIT): 0 (off), 1, 2, 4, 8 or 16"},
    {SIMULST_OPT_DEC_EMBED_QKV_CHAIN, "SIMULST_DEC_EMBED_QKV_CHAIN", M(dec_embed_qkv_chain), true, ANY, ANY, SL_PRODUCT, ""},
    {SIMULST_OPT_DEC_CHAIN_ROWS32, "SIMULST_DEC_CHAIN_ROWS32", M(dec_chain_rows32), true, ANY, ANY, EXP,
     "simulst_set_option(DEC_CHAIN_ROWS32): 0 or 1; the layer chains on 32-row tiles exist in EXPERIMENTS builds only (measured slower)"},
    {NO_OPTION, "SIMULST_DEC_CHAIN_ROWS32_MIN", M(dec_chain_rows32_min), false, ANY, ANY, EXP, ""},
    {SIMULST_OPT_DEC_FUSE_FFN_QKV, "SIMULST_DEC_FUSE_FFN_QKV", M(dec_fuse_ffn_qkv), true, ANY, ANY, EXP,
     "simulst_set_option(DEC_FUSE_FFN_QKV): 0 or 1; the feed-forward chain + next layer's QKV in one launch exists in EXPERIMENTS builds only (measured slower)"},
    {SIMULST_OPT_DEC_FUSE_PROJ_CROSS, "SIMULST_DEC_FUSE_PROJ_CROSS", M(dec_fuse_proj_cross), true, ANY, ANY, EXP,
     "simulst_set_option(DEC_FUSE_PROJ_CROSS): 0 or 1; the one-launch projection chain + cross-attention exists in EXPERIMENTS builds only (measured slower)"},
    {SIMULST_OPT_CONV_TILE256, "SIMULST_CONV_TILE256", M(tile256), false, TILE256_FORMS, TILE256_FORMS, SL_PRODUCT,
     "simulst_set_option(CONV_TILE256): 0 (128 x 128 tiles), 1 (256 x 256, register stage), 2 (256 x 256, LDS-DMA ring)"},
    {SIMULST_OPT_WEIGHT_STATIONARY, "SIMULST_WEIGHT_STATIONARY", M(wstat), true, ANY, ANY, SL_PRODUCT, ""},
    {NO_OPTION, "SIMULST_POLICY_LDS_BYTES", M(policy_lds_bytes), false, RANGE(0, 64 * 1024), ANY, SL_PRODUCT, ""},
};
#undef M

bool in_this_build(const tunable& t) { return (t.flavour & SL_BUILD_FLAVOUR) == t.flavour; }
const tunable* find_option(int option) {
  for (const tunable& t : TUNABLES) if (t.option == option) return &t;
  return nullptr;
}

}  // namespace

extern "C" int simulst_create(simulst_handle** out, void* hip_stream) {
  if (!out) return SIMULST_E_NULL;
  simulst_handle* h = new (std::nothrow) simulst_handle();
  if (!h) return SIMULST_E_ARG;
  h->stream = (hipStream_t)hip_stream;
  for (const tunable& t : TUNABLES) {
    const char* e = t.env && in_this_build(t) ? getenv(t.env) : nullptr;
    if (!e) continue;
    const int v = atoi(e);
    if (!t.env_ok || t.env_ok(v)) h->*t.member = t.flag ? v != 0 : v;
  }
  const char* tall = getenv("SIMULST_DEC_TALL_MIN_ROWS");
  h->dec_tall_min_rows = tall ? atoi(tall) : h->dec_chain_ffn_max_rows + 1;      // where the feed-forward chain ends
  if (const char* e = getenv("SIMULST_PANEL_WIDE")) {
    h->panel_wide = atoi(e) != 0;
    h->panel_wide_plain_stores = (SL_BUILD_FLAVOUR & SL_EXPERIMENTS_BUILD) && atoi(e) == 2;
  }
  int dev = 0, n = 0;
  // a failed query leaves 0: the persistent one-workgroup-per-CU kernels (gemm_wstat.hip) then decline and the row panels run
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 8) n = 0;
  h->n_cus = n;
  *out = h;
  return SIMULST_OK;
}

extern "C" int simulst_destroy(simulst_handle* h) {
  if (!h) return SIMULST_E_NULL;
  for (auto& p : h->ev_pool) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
  if (h->ws) (void)hipFree(h->ws);
  if (h->fuse_flags) (void)hipFree(h->fuse_flags);
  if (h->chain_sem) (void)hipFree(h->chain_sem);
  if (h->graph_exec) (void)hipGraphExecDestroy(h->graph_exec);
  delete h;
  return SIMULST_OK;
}

int sl_raise_lds_limits(simulst_handle* h, sl_lds_slot slot, const sl_lds_limit* list, int n, const char* who) {
  for (int i = 0; i < n; ++i) {
    const hipError_t e = hipFuncSetAttribute(list[i].kernel, hipFuncAttributeMaxDynamicSharedMemorySize, list[i].bytes);
    if (e != hipSuccess) { h->err = std::string(who) + ": cannot raise the dynamic LDS limit: " + hipGetErrorString(e); return (int)e; }
  }
  h->lds_raised[slot] = true;
  return SIMULST_OK;
}

int sl_workspace(simulst_handle* h, size_t need, size_t floor_bytes, const char* who) {
  if (h->ws_bytes >= need) return SIMULST_OK;
  if (h->capturing) { h->err = std::string(who) + ": scratch too small while capturing a graph"; return SIMULST_E_ARG; }
  if (h->ws) (void)hipFree(h->ws);
  h->ws = nullptr; h->ws_bytes = 0;
  const size_t want = need < floor_bytes ? floor_bytes : need;
  const hipError_t e = hipMalloc(&h->ws, want);
  if (e != hipSuccess) { h->err = std::string(who) + ": scratch allocation failed"; return (int)e; }
  h->ws_bytes = want;
  return SIMULST_OK;
}

extern "C" int simulst_set_stream(simulst_handle* h, void* hip_stream) {
  if (!h) return SIMULST_E_NULL;
  h->stream = (hipStream_t)hip_stream;
  return SIMULST_OK;
}

extern "C" const char* simulst_last_error(simulst_handle* h) { return h ? h->err.c_str() : "null handle"; }

extern "C" int simulst_timer_enable(simulst_handle* h, int cls, int on) {
  if (!h) return SIMULST_E_NULL;
  if (cls < 0) { for (int i = 0; i < SIMULST_K_COUNT; ++i) h->timer_on[i] = on != 0; return SIMULST_OK; }
  SL_REQUIRE(h, cls < SIMULST_K_COUNT, SIMULST_E_ARG, "simulst_timer_enable: kernel class");
  h->timer_on[cls] = on != 0;
  return SIMULST_OK;
}

#include <algorithm>
static void resolve_events(simulst_handle* h) {
  if (h->ev_used == 0) return;
  (void)hipStreamSynchronize(h->stream);
  for (int i = 0; i < h->ev_used; ++i) {
    float ms = 0.f;
    hipEvent_t from = i == 0 ? h->ev_pool[0].a : h->ev_pool[i - 1].b;
    if (hipEventElapsedTime(&ms, from, h->ev_pool[i].b) == hipSuccess) {
      h->timer_ms[h->ev_pool[i].cls] += ms;
      h->timer_n[h->ev_pool[i].cls] += 1;
    }
  }
  h->ev_used = 0;
}

extern "C" int simulst_timer_read(simulst_handle* h, int cls, double* total_ms, int64_t* launches) {
  if (!h) return SIMULST_E_NULL;
  SL_REQUIRE(h, cls >= 0 && cls < SIMULST_K_COUNT, SIMULST_E_ARG, "simulst_timer_read: kernel class");
  resolve_events(h);
  if (total_ms) *total_ms = h->timer_ms[cls];
  if (launches) *launches = h->timer_n[cls];
  return SIMULST_OK;
}

extern "C" int simulst_timer_reset(simulst_handle* h) {
  if (!h) return SIMULST_E_NULL;
  resolve_events(h);
  for (int i = 0; i < SIMULST_K_COUNT; ++i) { h->timer_ms[i] = 0.0; h->timer_n[i] = 0; }
  return SIMULST_OK;
}

extern "C" int simulst_graph_enable(simulst_handle* h, int on) {
  if (!h) return SIMULST_E_NULL;
  h->graph_on = on != 0;
  if (!h->graph_on && h->graph_exec) { (void)hipGraphExecDestroy(h->graph_exec); h->graph_exec = nullptr; h->graph_key = 0; }
  if (h->graph_on && h->ws_bytes < (size_t)(16u << 20)) {     // no allocation may happen inside a capture
    if (h->ws) (void)hipFree(h->ws);
    h->ws = nullptr; h->ws_bytes = 0;
    hipError_t e = hipMalloc(&h->ws, (size_t)(16u << 20));
    if (e != hipSuccess) { h->err = "simulst_graph_enable: scratch allocation failed"; return (int)e; }
    h->ws_bytes = (size_t)(16u << 20);
  }
  return SIMULST_OK;
}

extern "C" int simulst_set_option(simulst_handle* h, int32_t option, int32_t value) {
  if (!h) return SIMULST_E_NULL;
  if (option == SIMULST_OPT_PANEL_WIDE) {
    if (value < 0 || value > ((SL_BUILD_FLAVOUR & SL_EXPERIMENTS_BUILD) ? 2 : 1)) {
      h->err = "simulst_set_option(PANEL_WIDE): 0, 1 or 2 (plain stores: EXPERIMENTS builds only)";
      return SIMULST_E_ARG;
    }
    h->panel_wide = value != 0; h->panel_wide_plain_stores = value == 2;
    return SIMULST_OK;
  }
  const tunable* t = find_option(option);
  if (!t) { h->err = "simulst_set_option: unknown option"; return SIMULST_E_ARG; }
  if (!in_this_build(*t) || (t->set_ok && !t->set_ok(value))) { h->err = t->refusal; return SIMULST_E_ARG; }
  h->*t->member = t->flag ? value != 0 : value;
  return SIMULST_OK;
}

// What the handle currently runs with (the environment overrides of simulst_create included): callers that MODEL the launches of a
// decode step (bench.py's per-class byte counts) read the values back instead of re-deriving the library's defaults.
extern "C" int simulst_get_option(simulst_handle* h, int32_t option, int32_t* value) {
  if (!h) return SIMULST_E_NULL;
  SL_CHECK_NULL(h, value);
  if (option == SIMULST_OPT_PANEL_WIDE) { *value = h->panel_wide ? (h->panel_wide_plain_stores ? 2 : 1) : 0; return SIMULST_OK; }
  const tunable* t = find_option(option);
  if (!t) { h->err = "simulst_get_option: unknown option"; return SIMULST_E_ARG; }
  *value = h->*t->member;
  if (option == SIMULST_OPT_DEC_FUSE_PROJ_CROSS && h->fuse_flags) {
    // bit 0: on; bit 1: a waiting workgroup's bounded spin ran out at some point (synchronises the stream: tests only)
    int err = 0;
    (void)hipStreamSynchronize(h->stream);
    (void)hipMemcpy(&err, h->fuse_flags + 1023, sizeof(int), hipMemcpyDeviceToHost);
    *value |= err ? 2 : 0;
  }
  return SIMULST_OK;
}

// HIP streams with a compute-unit mask and / or a priority, for callers whose framework cannot create them (torch wraps the returned
// pointer as an external stream).  cu_mask: mask_words 32-bit words, bit i = compute unit (i / 8) of XCD (i % 8) on MI355X (measured:
// tools/microbench_cumask.hip; every XCD must keep at least one unit or the runtime ignores the mask); nullptr / 0: no mask.
// priority: 0 default, > 0 the device's greatest, < 0 its least (ignored with a mask: the extension takes none).
extern "C" int simulst_stream_create(void** out_stream, int32_t priority, const uint32_t* cu_mask, int32_t mask_words) {
  if (!out_stream) return SIMULST_E_NULL;
  hipStream_t s = nullptr;
  hipError_t e;
  if (cu_mask && mask_words > 0) {
    e = hipExtStreamCreateWithCUMask(&s, (uint32_t)mask_words, cu_mask);
  } else if (priority != 0) {
    int least = 0, greatest = 0;
    e = hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority > 0 ? greatest : least);
  } else {
    e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
  }
  if (e != hipSuccess) return (int)e;      // (no handle here to carry a message: a positive return is the hipError_t, as everywhere in this ABI)
  *out_stream = (void*)s;
  return SIMULST_OK;
}

extern "C" int simulst_stream_destroy(void* stream) {
  if (!stream) return SIMULST_E_NULL;
  hipError_t e = hipStreamDestroy((hipStream_t)stream);
  return e == hipSuccess ? SIMULST_OK : (int)e;
}

// 1 in a `make EXPERIMENTS=1` build (the measured-slower kernel families and their option values are compiled in), else 0
extern "C" int simulst_has_experiments(void) { return (SL_BUILD_FLAVOUR & SL_EXPERIMENTS_BUILD) ? 1 : 0; }
