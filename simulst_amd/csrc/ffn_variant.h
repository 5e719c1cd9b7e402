// SIMULST_OPT_FFN_WAVES decoded once (host only): which form of the fused Emformer feed-forward a code selects.  The option table of
// handle.cpp takes the legal codes from here, simulst_emformer_ffn (ffn_fused.hip) switches on the result, sl_launch_ffn_pipe
// (ffn_pipe.hip) takes it as it is.
#pragma once
#include "common.h"

struct sl_ffn_variant {
  bool pipelined;      // ffn_pipe.hip (GELU inside the MFMA stream, 128 rows per 4-wave workgroup) or the block form of ffn_fused.hip
  int waves;           // 4 or 8
  int packed;          // pipelined: packed GELU (DEBUG_HOOKS builds)
  int uniform;         // pipelined: 0 GELU as a phase, 1 a quarter of an element pair's GELU behind each of the 32 MFMAs of an iteration with the
                       //   LDS-DMA pieces one per MFMA gap, 2 64 rows per wave (ffn_wide_kernel), 3 as 1 with the pieces as a burst behind the barrier
};

constexpr int SL_FFN_PIPE_MAX_F = 2048;       // the pipelined form's fc1 bias lives in LDS
constexpr int SL_FFN_BLOCK4_MAX_F = 2048;     // ... and the 4-wave block form's (ffn_fused.hip FFG<4>::MAX_F); above: 8 waves, one workgroup per CU

// The pipelined codes and the builds that accept them.  What ships is 0 = 43: 439 / 830 / 941 / 927 TFLOP/s at 64 / 256 / 1280 / 4096
// utterances against 394 / 743 / 889 / 881 for the phase form (41) on the same device, and 804 / 887 / 875 TFLOP/s at 448 / 1280 / 4096
// utterances against 758 / 863 / 851 for the 4-wave block form.  The 8-wave, phase and 64-rows-per-wave forms measured slower and exist in
// EXPERIMENTS builds; packed GELU inside the MFMA stream measured SLOWER still (826 vs 887 TFLOP/s at 1280 utterances: an anti-lever
// beside MFMAs) and exists in DEBUG_HOOKS builds only.
struct sl_ffn_code { int code, waves, packed, uniform, flavour; };
constexpr sl_ffn_code SL_FFN_PIPELINED[] = {
    {0, 4, 0, 1, SL_PRODUCT},           {43, 4, 0, 1, SL_PRODUCT},
    {41, 4, 0, 0, SL_EXPERIMENTS_BUILD}, {45, 4, 0, 2, SL_EXPERIMENTS_BUILD}, {47, 4, 0, 3, SL_EXPERIMENTS_BUILD},
    {81, 8, 0, 0, SL_EXPERIMENTS_BUILD}, {83, 8, 0, 1, SL_EXPERIMENTS_BUILD}, {87, 8, 0, 3, SL_EXPERIMENTS_BUILD},
    {42, 4, 1, 0, SL_EXPERIMENTS_BUILD | SL_DEBUG_HOOKS_BUILD}, {82, 8, 1, 0, SL_EXPERIMENTS_BUILD | SL_DEBUG_HOOKS_BUILD}};

// 4 / 8: the block form (GELU between the two products) with that many waves, in every build
static inline bool sl_ffn_code_legal(int code, int flavour = SL_BUILD_FLAVOUR) {
  if (code == 4 || code == 8) return true;
  for (const sl_ffn_code& c : SL_FFN_PIPELINED)
    if (c.code == code) return (c.flavour & flavour) == c.flavour;
  return false;
}

static inline sl_ffn_variant sl_decode_ffn_variant(int code, int F, int flavour = SL_BUILD_FLAVOUR) {
  for (const sl_ffn_code& c : SL_FFN_PIPELINED)
    if (c.code == code && F <= SL_FFN_PIPE_MAX_F) {
      sl_ffn_variant v = {true, c.waves, c.packed, c.uniform};
      if (!(flavour & SL_DEBUG_HOOKS_BUILD)) v.packed = 0;                       // instantiations this build does not have
      if (!(flavour & SL_EXPERIMENTS_BUILD)) { v.waves = 4; v.uniform = 1; }
      return v;
    }
  // the library's choice (0) and 4: two 4-wave workgroups per CU while the fc1 bias fits their LDS budget, else one 8-wave workgroup;
  // 8 and a pipelined code above its F: 8 waves
  return {false, (code == 0 || code == 4) && F <= SL_FFN_BLOCK4_MAX_F ? 4 : 8, 0, 0};
}
