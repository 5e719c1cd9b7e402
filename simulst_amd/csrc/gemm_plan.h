// Kernel selection of simulst_linear: which contraction kernel a call takes, and with what launch geometry, is decided ONCE per call,
// here, from the handle's options, dtype, epilogue, the LinArgs and the alignment of the operand pointers.  The sl_launch_* functions of
// the gemm*.hip files read the plan; the decode loops' vocabulary projection (sl_plan_vocab_argmax) and the retire floor
// (decode_plan.cpp) read the same decision and the same constants.  Host code only.
#pragma once
#include "gemm_args.h"

// tile shapes the decision reads (the kernels use the same names)
constexpr int PB_M = 128, PB_N = 64, PB_KS = 32;      // row panel (gemm_panel.hip): rows per workgroup, columns per step, k per k-step
constexpr int PW_M = 256, PW_N = 32;                  // wide row panel: rows per workgroup, columns per step
// 256 x 256 tiles (gemm_tile256.hip): tile edge; k depth and LDS row stride (272-byte rows: conflict-free b128) of the register-staged
// form, whose one LDS stage holds A rows then W rows (136 KB); k depth of the LDS-DMA ring, whose stage is 32 KB of A + 32 KB of W rows
constexpr int TB = 256, TBK = 128, TLD = TBK + 8, RBK = 64;
constexpr int T_STAGE = 2 * TB * TLD;                 // bf16 elements
constexpr int R_STAGE = 2 * TB * RBK * 2;             // bytes
constexpr unsigned T256_STAGE_LDS = T_STAGE * 2;      // dynamic LDS of the two forms: the ring's two stages or its epilogue's staged tile
constexpr unsigned T256_RING_LDS = 2 * R_STAGE > TB * (TB / 2 + 8) * 2 ? 2 * R_STAGE : TB * (TB / 2 + 8) * 2;
// rows from which the tile kernels of gemm_mid.hip (64 x 64, wave per 16 x 16) replace the skinny kernel
constexpr int TILE_MIN_ROWS = 256;
// decode-step shapes: up to 2048 rows, up to 8192 when the caller packed the weights for them (co-scheduled batches)
constexpr int SKINNY_MAX_ROWS = 2048, SKINNY_MAX_ROWS_PACKED = 8192;
// row pick (gemm_pick.hip): rows of a workgroup's LDS panel on the matrix cores, the panel's byte limit (with the kernel's 3 KB of
// static LDS inside the default 64 KB: no raise), rows per workgroup of the VALU form
constexpr int PICK_M = 64, PICK_LDS_MAX = 60 * 1024, PICK_VM = 4;
// SIMULST_EPI_ROW_TOPK: at most 8 columns a row; every wave keeps a list of 16 eight-byte candidates per row behind the panel (the
// launcher raises the kernel's dynamic-LDS limit); bytes of a column part's record of one row in the library's scratch
constexpr int PICK_TOPK_MAX = 8, PICK_TOPK_CAP = 16, PICK_TOPK_REC_BYTES = 80;
constexpr unsigned PICK_TOPK_LDS = 4 * PICK_M * PICK_TOPK_CAP * 8;

enum sl_linear_family {
  SL_LIN_REFUSED = 0,
  SL_LIN_WSTAT,          // weight-stationary persistent kernel, 6 or 8 column-tile pairs per slice (gemm_wstat.hip)
  SL_LIN_PANEL_WIDE,     // 256-row panel, bias only (gemm_panel.hip panel_wide_kernel)
  SL_LIN_PANEL,          // 128-row panel over the whole width, plain or LayerNorm prologue (gemm_panel.hip panel_kernel)
  SL_LIN_PANEL_SPLIT,    // ... with the column range split over blockIdx.y (co-scheduled decode batches)
  SL_LIN_MID,            // 64 x 64 decode tile, short (64 rows) or tall (128) (gemm_mid.hip mid_kernel)
  SL_LIN_WAVE_TILE,      // one wave per 16 x 16 tile (gemm_mid.hip wave_tile_kernel)
  SL_LIN_SKINNY,         // 16 MTs x 16 NTs tile, k over the waves, optional split-K (gemm_skinny.hip)
  SL_LIN_TILE256,        // 256 x 256 GLU tiles, register-staged or on the LDS-DMA ring (gemm_tile256.hip)
  SL_LIN_TILE128,        // 128 x 128 tiles (gemm.hip)
  SL_LIN_TILE64,         // 64 x 64 tiles (gemm.hip)
  SL_LIN_ROW_PICK,       // SIMULST_EPI_ROW_PICK: per-row (argmax, max, logsumexp), logits never written (gemm_pick.hip);
                         //   SIMULST_EPI_ROW_GATHER (plan.epi): log-probabilities at the caller's labels, same kernels;
                         //   SIMULST_EPI_ROW_TOPK (plan.epi): the best k columns of a row, same sweep and plan
};

struct sl_linear_plan {
  int family;
  int status;            // SL_LIN_REFUSED: what simulst_linear returns ...
  const char* err;       //   ... and leaves as the handle's message
  int dtype, epi;
  int timer;             // SIMULST_K_* class of every launch of the call
  unsigned grid[3];
  unsigned lds;          // dynamic LDS bytes
  bool ln;               // LayerNorm prologue form
  int MTs, NTs, splits, kps;      // SKINNY: 16-row / 16-column tiles per workgroup, split-K ranges and the k of one; ROW_PICK: splits =
                                  //   column parts (grid[1]), folded by a second launch when > 1
  bool tall;             // MID: 128-row tiles
  int tiles_n;           // WAVE_TILE: 16-column tiles of a row
  int spb;               // PANEL, PANEL_SPLIT: column steps (of PB_N) per workgroup
  int pairs, n_slices;   // WSTAT: column-tile pairs of a slice, slices of the width
  bool ring;             // TILE256: LDS-DMA ring (option value 2) instead of the register stage (1)
  bool pick_mfma;        // ROW_PICK: matrix-core form (bf16, K % 32 == 0, the row panel within PICK_LDS_MAX) instead of the VALU one
};

// the operands of a call, as simulst_linear got them
struct sl_linear_ops { const void *A, *W; const float* bias; const void* R; void *C, *aux; };

sl_linear_plan sl_plan_linear(const simulst_handle* h, int dtype, int epi, const LinArgs& p, const sl_linear_ops& o);

// The decode loops' vocabulary projection with the greedy pick's per-tile maxima as its output (bf16, fragment-major weights, the
// model's final LayerNorm, if it has one, as prologue, no bias): partial [B][V / 64] (value, index) pairs.  The plan is that of the
// decode-step link of sl_plan_linear for these rows -- the split row panel from thousands of rows on (with a LayerNorm only), else the
// 64 x 64 tile; any other family: not taken.
static inline LinArgs sl_vocab_args(int B, int V, int D, const float* ln_g, const float* ln_b) {
  LinArgs p = {};
  p.M = B; p.rpb = B; p.N = V; p.K = D;
  p.a_rs = D; p.c_rs = V; p.r_rs = V;
  p.scale = 1.f; p.ln_g = ln_g; p.ln_b = ln_b; p.w_packed = 1;
  return p;
}
sl_linear_plan sl_plan_vocab_argmax(const simulst_handle* h, int dtype, int B, int V, int D, bool packed, bool has_ln);
static inline bool sl_vocab_argmax_ok(const simulst_handle* h, int dtype, int B, int V, int D, bool packed) {
  return sl_plan_vocab_argmax(h, dtype, B, V, D, packed, true).family != SL_LIN_REFUSED;
}
int sl_launch_vocab_argmax(simulst_handle* h, const void* x, const void* W, const float* ln_g, const float* ln_b, float2* partial,
                           int B, int V, int D, int skip_a, int skip_b);

// one launcher per file; each launches what the plan says
int sl_launch_skinny(simulst_handle* h, const sl_linear_plan& pl, const sl_linear_ops& o, const LinArgs& p);        // gemm_skinny.hip
int sl_launch_mid(simulst_handle* h, const sl_linear_plan& pl, const sl_linear_ops& o, const LinArgs& p);           // gemm_mid.hip
int sl_launch_wave_tile(simulst_handle* h, const sl_linear_plan& pl, const sl_linear_ops& o, const LinArgs& p);     // gemm_mid.hip
int sl_launch_panel(simulst_handle* h, const sl_linear_plan& pl, const sl_linear_ops& o, const LinArgs& p);         // gemm_panel.hip:
int sl_launch_panel_wide(simulst_handle* h, const sl_linear_plan& pl, const sl_linear_ops& o, const LinArgs& p);    //   PANEL, PANEL_WIDE,
int sl_launch_panel_split(simulst_handle* h, const sl_linear_plan& pl, const sl_linear_ops& o, const LinArgs& p);   //   PANEL_SPLIT
int sl_launch_wstat(simulst_handle* h, const sl_linear_plan& pl, const sl_linear_ops& o, const LinArgs& p);         // gemm_wstat.hip
int sl_launch_tile256(simulst_handle* h, const sl_linear_plan& pl, const sl_linear_ops& o, const LinArgs& p);       // gemm_tile256.hip
int sl_launch_row_pick(simulst_handle* h, const sl_linear_plan& pl, const sl_linear_ops& o, const LinArgs& p);      // gemm_pick.hip

// The <TA, TC, EPI> of a decode-step epilogue: f(TA(), TC(), std::integral_constant<int, EPI>()).  The plan refuses every other
// epilogue before a launcher is reached.
template <typename TA, typename F>
int sl_by_decode_epilogue(simulst_handle* h, int epi, F&& f) {
  switch (epi) {
    case SIMULST_EPI_BIAS: return f(TA(), TA(), std::integral_constant<int, SIMULST_EPI_BIAS>());
    case SIMULST_EPI_BIAS_GELU: return f(TA(), TA(), std::integral_constant<int, SIMULST_EPI_BIAS_GELU>());
    case SIMULST_EPI_BIAS_RES: return f(TA(), TA(), std::integral_constant<int, SIMULST_EPI_BIAS_RES>());
    case SIMULST_EPI_BIAS_F32OUT: return f(TA(), float(), std::integral_constant<int, SIMULST_EPI_BIAS>());
    case SIMULST_EPI_BIAS_RES_GELU: return f(TA(), TA(), std::integral_constant<int, SIMULST_EPI_BIAS_RES_GELU>());
    default: h->err = "simulst_linear: epilogue not available for decode-step shapes"; return SIMULST_E_ARG;
  }
}
