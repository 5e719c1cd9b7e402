// simulst_linear's kernel selection (gemm_plan.h).  Host code only.  The ORDER of the tests below decides which kernel, and with it
// which rounding, a call gets: the decode loops' retire floor (decode_plan.cpp) and tests/test_linear_plan.py hold it in place.
#include "gemm_plan.h"

static unsigned cdiv(long a, long b) { return (unsigned)((a + b - 1) / b); }

static sl_linear_plan refused(sl_linear_plan pl, int status, const char* err) {
  pl.family = SL_LIN_REFUSED; pl.status = status; pl.err = err;
  return pl;
}

// ---- tall problems: row panels and the weight-stationary kernel ---------------------------------------------------------------------
// shapes the panel kernels take: bf16, fragment-major weights, tall problems with a short contraction
static bool panel_shape(int dtype, int epi, const LinArgs& p) {
  return dtype == SIMULST_BF16 && p.w_packed && p.M >= 4096 && p.K <= 256 && p.K % PB_KS == 0 && p.N % 16 == 0 &&
         p.a_lead == 0 && p.a_rs >= p.K && (p.c_hd == 0 || p.c_hd % 8 == 0) &&
         // LayerNorm prologue (the encoder's pre-FFN LayerNorm rides in fc1: applied ONCE to the stationary A
         // fragments of a panel, one launch and 0.8 MB of HBM traffic per utterance and layer less)
         (!p.ln_g || epi == SIMULST_EPI_BIAS || epi == SIMULST_EPI_BIAS_GELU) &&
         // (fc1 + GELU: 1568 us here vs 1795 us on the 128 x 128 tile kernel at 605 k rows, N = 2048, now that the
         //  GELU issues on the packed fp32 pipe; with the exp-based form the tile kernel had been the faster one)
         (epi == SIMULST_EPI_BIAS || epi == SIMULST_EPI_BIAS_GELU || epi == SIMULST_EPI_BIAS_RES || epi == SIMULST_EPI_EMF_OUT);
}

// column slices of a width-N projection: 256- or 192-column slices, at most 4, preferring a count that divides the 32 CUs of an XCD
// (768 = 4 x 192 uses every CU; 3 x 256 would leave two of 32 idle)
static bool wstat_split(int N, int& pairs, int& n_slices) {
  const bool a = N % 256 == 0 && N / 256 <= 4, b = N % 192 == 0 && N / 192 <= 4;
  if (!a && !b) return false;
  const bool use_a = a && (!b || 32 % (N / 256) == 0 || 32 % (N / 192) != 0);      // (QKV as 3 x 256: 357 us against 338)
  pairs = use_a ? 8 : 6;
  n_slices = N / (32 * pairs);
  return true;
}

// Weight-stationary kernel: bf16, fragment-major weights, K == 256, plain row-major output, 16-byte aligned rows; N == 256 (one slice)
// with the Emformer out-proj epilogue, or a bias-only projection whose width splits into slices over an XCD's CUs.
static bool wstat_ok(const simulst_handle* h, int epi, const LinArgs& p, const sl_linear_ops& o, int& pairs, int& n_slices) {
  if (!h->wstat || !p.w_packed || p.K != 256 || p.M < 8192 || p.c_hd != 0 || p.a_lead != 0 || p.ln_g) return false;
  if ((((uintptr_t)o.A | (uintptr_t)o.C | (uintptr_t)o.R) & 15) != 0) return false;
  if (((p.a_rs | p.a_bs | p.c_rs | p.c_bs) & 7) != 0) return false;
  if (epi != SIMULST_EPI_EMF_OUT && epi != SIMULST_EPI_BIAS) return false;
  if (epi == SIMULST_EPI_EMF_OUT && !(p.N == 256 && ((p.r_rs | p.r_bs | p.aux_bs) & 7) == 0 && h->n_cus >= 8)) return false;
  // every slice of a row tile needs its own compute unit inside ONE XCD (groups of n_slices workgroups per XCD): a device or partition
  // with fewer than 8 x n_slices units, or an unknown count (n_cus 0), keeps the row panels (the kernel would return at once)
  return wstat_split(p.N, pairs, n_slices) && (h->n_cus >> 3) >= n_slices;
}

// the wide panel: bias-only epilogue, K == 256, whole 32-column steps, 16-byte aligned output rows / heads
static bool panel_wide_ok(const simulst_handle* h, int epi, const LinArgs& p, const sl_linear_ops& o) {
  // 16-byte loads of A rows and 16-byte streaming stores of C rows: the base pointers must be aligned like the strides; the bias
  // travels by 4-byte DMA
  if ((((uintptr_t)o.A | (uintptr_t)o.C) & 15) != 0 || ((uintptr_t)o.bias & 3) != 0) return false;
  return h->panel_wide && epi == SIMULST_EPI_BIAS && !p.ln_g && p.K == 256 && p.N % PW_N == 0 && p.M >= 8192 &&
         ((p.c_rs | p.c_bs | p.c_hs | p.c_ts) & 7) == 0 && (p.c_hd == 0 || p.c_hd % 8 == 0) && (p.a_rs & 7) == 0 && (p.a_bs & 7) == 0;
}

static sl_linear_plan plan_tall_panel(const simulst_handle* h, sl_linear_plan pl, const LinArgs& p, const sl_linear_ops& o) {
  pl.timer = SIMULST_K_LINEAR;
  if (wstat_ok(h, pl.epi, p, o, pl.pairs, pl.n_slices)) {
    pl.family = SL_LIN_WSTAT;
    pl.grid[0] = h->n_cus & ~7;                                    // one workgroup per CU, whole XCD rounds
    pl.lds = 2 * pl.pairs * 8 * 64 * 16 + 32 * pl.pairs * sizeof(float);     // the slice's fragments + its bias
  } else if (panel_wide_ok(h, pl.epi, p, o)) {
    pl.family = SL_LIN_PANEL_WIDE;
    pl.grid[0] = cdiv(p.M, PW_M);
  } else {
    pl.family = SL_LIN_PANEL;
    pl.grid[0] = cdiv(p.M, PB_M);
    pl.spb = cdiv(p.N, PB_N);
  }
  return pl;
}

// ---- decode-step shapes -------------------------------------------------------------------------------------------------------------
// Co-scheduled decode batches: thousands of rows are too few panels to fill 256 CUs, so the column range is split:
// ~panel_split_blocks workgroups, each keeping its (LayerNorm-ed) A fragments for >= 2 column steps.  With one step per workgroup this
// would be the 64 x 64 kernel of gemm_mid.hip, which keeps those shapes.
static int split_steps(const simulst_handle* h, const LinArgs& p) {
  const int panels = cdiv(p.M, PB_M), n_all = cdiv(p.N, PB_N);
  int nsplit = (h->panel_split_blocks + panels - 1) / panels;
  if (nsplit < 1) nsplit = 1;
  if (nsplit > n_all) nsplit = n_all;
  return (n_all + nsplit - 1) / nsplit;
}

static bool panel_split_ok(const simulst_handle* h, int dtype, int epi, const LinArgs& p) {
  if (!(dtype == SIMULST_BF16 && p.w_packed && p.M >= h->panel_split_min_rows && p.K <= 256 && p.K % PB_KS == 0 &&
        p.N % 16 == 0 && p.N >= 512 && p.a_lead == 0 && p.a_rs >= p.K && (p.c_hd == 0 || p.c_hd % 8 == 0)))
    return false;
  if (p.ln_g ? !(epi == SIMULST_EPI_BIAS || epi == SIMULST_EPI_BIAS_GELU || epi == SIMULST_EPI_BIAS_F32OUT)
             : !(epi == SIMULST_EPI_BIAS || epi == SIMULST_EPI_BIAS_GELU || epi == SIMULST_EPI_BIAS_RES))
    return false;
  if (epi == SIMULST_EPI_BIAS_F32OUT && p.c_hd != 0) return false;
  return split_steps(h, p) >= 2;
}

// the 64 x 64 tile takes over from the 16 x BN kernel: co-scheduled batches with a wide output
static bool mid_ok(const simulst_handle* h, int KS, const LinArgs& p) {
  const long blocks = (long)cdiv(p.M, 64) * cdiv(p.N, 64);            // 64 x 64 tiles: most of the chip gets one
  // narrow outputs with a short contraction (out-proj, q-proj: N = 256, K = 256) from mid_narrow_min_rows rows on:
  // one wave per 16 x 16 tile re-reads 16 KB of operands per 131 kflop and is L2-bound there (4096 rows: 9.3 -> 7.9 us
  // out-proj, 12.8 -> 7.6 us LN + q-proj).  fc2 (K = 2048) measured the same on both kernels and keeps the k-split one.
  const bool narrow = p.N >= 64 && p.N < 512 && p.K <= 8 * KS && p.M >= h->mid_narrow_min_rows;
  return p.M >= TILE_MIN_ROWS && (p.N >= 512 || narrow) && blocks >= h->mid_min_blocks && p.K % KS == 0 && (!p.ln_g || p.K <= 8 * KS);
}

// narrow outputs of co-scheduled batches with a short contraction: one wave per tile
static bool wave_tile_ok(int KS, const LinArgs& p) { return p.M >= TILE_MIN_ROWS && p.N < 512 && p.K % KS == 0 && p.K <= 8 * KS; }

static sl_linear_plan plan_skinny(const simulst_handle* h, sl_linear_plan pl, int KS, const LinArgs& p) {
  // spread over the chip: start from 64 x 32 tiles (a weight fragment reused by 4 row tiles) and shrink -- columns
  // first, then rows -- until the grid has >= 512 workgroups (two per CU) or the tile is the 16 x 16 minimum
  int MTs = 4, NTs = 2;
  auto blocks = [&](int m_, int n_) { return (long)cdiv(p.M, 16 * m_) * cdiv(p.N, 16 * n_); };
  // co-scheduled batches (more rows than columns: fc2) keep the 64 x 32 tile down to 192 workgroups: measured at
  // 1536 / 2048 / 3072 rows 14.9 / 15.1 / 22.7 us against 15.6 / 19.3 / 26.8 us for the tiles the 512 rule picks
  // (the 64 x 16 tile in between is the worst of the three: 19.3 us at 1536 rows)
  const bool keep_big = p.M > p.N && blocks(4, 2) >= h->skinny_min_blocks_tall;
  while (!keep_big && blocks(MTs, NTs) < 512 && (MTs > 1 || NTs > 1)) {
    if (NTs > 1) NTs = 1; else MTs >>= 1;
  }
  if (MTs == 1 && NTs == 1 && blocks(1, 1) > 512) NTs = 2;      // the M <= 64 policy of the 16 x BN kernel
  const int mt = cdiv(p.M, 16 * MTs), nt = cdiv(p.N, 16 * NTs);
  int splits = 1;
  // measured on MI355X (bench.py, K = 2048 fc2): one 16x16-tile launch streaming 128 KB per workgroup is as
  // fast end to end as 4-way split-K + epilogue launch, so splitting starts only at K >= 4096
  if (!p.ln_g && p.K >= 4096) {
    splits = p.K / 1024;
    while (splits > 1 && (long)mt * nt * splits > 1024) splits >>= 1;
    if (splits > 1) MTs = 1;
  }
  int kps = (p.K + splits - 1) / splits;
  kps = (kps + KS - 1) / KS * KS;
  splits = (p.K + kps - 1) / kps;
  if (p.ln_g && p.K > 4 * 4 * KS) return refused(pl, SIMULST_E_SHAPE, "simulst_linear: LN prologue needs K <= 512 (bf16) / 256 (fp32)");
  if (p.ln_g && MTs > 2 && p.K > 4 * 2 * KS) MTs = 2;           // 64-row tiles keep 2 k-steps per wave in flight
  pl.family = SL_LIN_SKINNY;
  pl.timer = SIMULST_K_LINEAR_SKINNY;
  pl.MTs = MTs; pl.NTs = NTs; pl.splits = splits; pl.kps = kps;
  pl.grid[0] = nt; pl.grid[1] = cdiv(p.M, 16 * MTs); pl.grid[2] = splits;
  return pl;
}

// 128-row tiles only when they still give every CU two workgroups (measured at 1024 rows: fc1 with 256 tall
// workgroups 14.0 us, with 512 of 64 rows 11.5 us; the vocabulary projection 20.7 vs 21.2 us)
static sl_linear_plan plan_mid(sl_linear_plan pl, const LinArgs& p) {
  pl.family = SL_LIN_MID;
  pl.timer = SIMULST_K_LINEAR_TILE64;
  pl.grid[0] = cdiv(p.N, 64);
  pl.tall = (long)cdiv(p.M, 128) * pl.grid[0] >= 512;
  pl.grid[1] = cdiv(p.M, pl.tall ? 128 : 64);
  return pl;
}

// split panel -> 64 x 64, short or tall -> wave tile -> skinny
static sl_linear_plan plan_decode_step(const simulst_handle* h, sl_linear_plan pl, const LinArgs& p) {
  const int KS = pl.dtype == SIMULST_F32 ? 16 : 32, epi = pl.epi;
  if (panel_split_ok(h, pl.dtype, epi, p)) {
    pl.family = SL_LIN_PANEL_SPLIT;
    pl.timer = SIMULST_K_LINEAR_TILE64;
    pl.spb = split_steps(h, p);
    pl.grid[0] = cdiv(p.M, PB_M); pl.grid[1] = cdiv(cdiv(p.N, PB_N), pl.spb);
    return pl;
  }
  if (epi != SIMULST_EPI_BIAS && epi != SIMULST_EPI_BIAS_GELU && epi != SIMULST_EPI_BIAS_RES && epi != SIMULST_EPI_BIAS_F32OUT &&
      epi != SIMULST_EPI_BIAS_RES_GELU)
    return refused(pl, SIMULST_E_ARG, "simulst_linear: epilogue not available for decode-step shapes");
  if (mid_ok(h, KS, p)) return plan_mid(pl, p);
  if (wave_tile_ok(KS, p)) {
    pl.family = SL_LIN_WAVE_TILE;
    pl.timer = SIMULST_K_LINEAR_SKINNY;
    pl.tiles_n = cdiv(p.N, 16);
    pl.grid[0] = cdiv((long)cdiv(p.M, 16) * pl.tiles_n, 4);
    return pl;
  }
  return plan_skinny(h, pl, KS, p);
}

// ---- 256 x 256 GLU tiles ------------------------------------------------------------------------------------------------------------
// bf16 GLU contractions of tall problems whose width is a multiple of 256 (the subsampler at the model's widths), 16-byte aligned
// output rows
static bool tile256_ok(const simulst_handle* h, int dtype, int epi, const LinArgs& p, const void* C) {
  // the kernel addresses its operands with 32-bit element offsets: both must span fewer than 2^31 elements (a 5 000-utterance batch of
  // the second convolution does not -- it stays on the 128 x 128 kernel's 64-bit pointers)
  const long a_span = (long)((p.M + p.rpb - 1) / p.rpb) * p.a_bs + (long)p.rpb * p.a_rs + p.K, w_span = (long)p.N * p.K;
  return h->tile256 && dtype == SIMULST_BF16 && epi == SIMULST_EPI_GLU && p.M >= 8192 && p.N % TB == 0 && p.K % 8 == 0 &&
         ((p.c_rs | p.c_bs) & 7) == 0 && ((uintptr_t)C & 15) == 0 && !p.w_packed && !p.ln_g && a_span < (1L << 31) && w_span < (1L << 31) &&
         p.a_bs >= 0 && p.a_rs >= 0;
}

// ---- row pick -----------------------------------------------------------------------------------------------------------------------
// bf16 with whole 32-element k-steps and a panel that fits the default dynamic-LDS limit (K <= 448) runs on the matrix cores,
// everything else on the VALU.  One workgroup per row panel over the whole width where the panels fill the chip; fewer than 128 panels
// (a stream's chunk, a lockstep round: under 8192 rows) split the column tiles over blockIdx.y, at least 8 tiles a part (one pair per
// wave), towards one workgroup per compute unit -- the parts fold through the library's scratch in a second launch.
// SIMULST_EPI_ROW_GATHER takes the same plan (row-major weights only): its gather phase rides behind the sweep of the same launch.
// SIMULST_EPI_ROW_TOPK takes it too, column split included (a part's record is PICK_TOPK_REC_BYTES a row, in the same scratch: 2 MB at
// most, 127 panels in 3 parts); its per-wave candidate lists follow the panel in dynamic LDS.
static sl_linear_plan plan_row_pick(sl_linear_plan pl, const LinArgs& p) {
  const long panel = (long)PICK_M * (p.K + 8) * 2;
  pl.family = SL_LIN_ROW_PICK;
  pl.timer = SIMULST_K_LINEAR;
  pl.pick_mfma = pl.dtype == SIMULST_BF16 && p.K % 32 == 0 && panel <= PICK_LDS_MAX;
  if (p.w_packed && pl.epi == SIMULST_EPI_ROW_GATHER)
    return refused(pl, SIMULST_E_SHAPE, "simulst_linear: row gather reads rows of W by label: row-major weights only (no fragment-major)");
  if (p.w_packed && !(pl.pick_mfma && p.N % 16 == 0))
    return refused(pl, SIMULST_E_SHAPE, "simulst_linear: row pick takes fragment-major weights in bf16 with N % 16 == 0, K % 32 == 0, K <= 448");
  pl.grid[0] = cdiv(p.M, pl.pick_mfma ? PICK_M : PICK_VM);
  pl.lds = pl.pick_mfma ? (unsigned)panel + (pl.epi == SIMULST_EPI_ROW_TOPK ? PICK_TOPK_LDS : 0) : 0;
  pl.splits = 1;
  if (pl.pick_mfma && pl.grid[0] < 128) {
    const unsigned by_width = cdiv(cdiv(p.N, 16), 8), by_chip = cdiv(256, pl.grid[0]);
    pl.splits = (int)(by_width < by_chip ? by_width : by_chip);
    if (pl.splits < 1) pl.splits = 1;
  }
  pl.grid[1] = pl.splits;
  return pl;
}

sl_linear_plan sl_plan_linear(const simulst_handle* h, int dtype, int epi, const LinArgs& p, const sl_linear_ops& o) {
  sl_linear_plan pl = {};
  pl.dtype = dtype; pl.epi = epi; pl.ln = p.ln_g != nullptr;
  pl.grid[0] = pl.grid[1] = pl.grid[2] = 1;
  if (epi == SIMULST_EPI_ROW_PICK || epi == SIMULST_EPI_ROW_GATHER || epi == SIMULST_EPI_ROW_TOPK) return plan_row_pick(pl, p);
  const int G = dtype == SIMULST_F32 ? 4 : 8;
  const bool skinny_ok = p.M <= (p.w_packed ? SKINNY_MAX_ROWS_PACKED : SKINNY_MAX_ROWS) && p.a_lead == 0 && p.a_rs >= p.K &&
                         epi != SIMULST_EPI_GLU && epi != SIMULST_EPI_EMF_OUT;
  if (!skinny_ok && panel_shape(dtype, epi, p)) return plan_tall_panel(h, pl, p, o);
  // (the two refusals below used to be SL_REQUIREs, which append the condition's text: callers match on the whole message, so the
  //  suffix is spelled out as it was)
  if (p.w_packed && !(skinny_ok && p.N % 16 == 0 && p.K % (4 * G) == 0))
    return refused(pl, SIMULST_E_SHAPE,
                   "simulst_linear: fragment-major weights need a decode-step shape (or a tall bf16 problem with K <= 256), "
                   "N % 16 == 0 and K % (64 bytes) == 0 [skinny_ok && d->N % 16 == 0 && d->K % (4 * G) == 0]");
  if (skinny_ok) return plan_decode_step(h, pl, p);
  if (p.ln_g) return refused(pl, SIMULST_E_SHAPE, "simulst_linear: LN prologue needs a decode-step shape [!p.ln_g]");
  pl.timer = SIMULST_K_LINEAR;
  if (tile256_ok(h, dtype, epi, p, o.C)) {
    pl.family = SL_LIN_TILE256;
    pl.ring = h->tile256 == 2;
    pl.grid[0] = cdiv(p.M, TB) * (p.N / TB);
    pl.lds = pl.ring ? T256_RING_LDS : T256_STAGE_LDS;
    return pl;
  }
  if (epi < SIMULST_EPI_BIAS || epi > SIMULST_EPI_BIAS_RES_GELU) return refused(pl, SIMULST_E_ARG, "simulst_linear: unknown epilogue");
  // tall problems get the 128 x 128 tile, mid-size the 64 x 64 one (a 256 x 128 tile was measured 2x SLOWER on MI355X for the
  // encoder shapes: 272+ VGPRs and 55 KB of LDS leave one workgroup per CU)
  const int edge = (epi == SIMULST_EPI_GLU || p.M > 512) ? 128 : 64;
  pl.family = edge == 128 ? SL_LIN_TILE128 : SL_LIN_TILE64;
  pl.grid[0] = cdiv(p.M, edge) * cdiv(p.N, edge);
  return pl;
}

sl_linear_plan sl_plan_vocab_argmax(const simulst_handle* h, int dtype, int B, int V, int D, bool packed, bool has_ln) {
  sl_linear_plan base = {};
  base.dtype = dtype; base.epi = SIMULST_EPI_BIAS_F32OUT; base.ln = has_ln;
  base.grid[0] = base.grid[1] = base.grid[2] = 1;
  if (!h->fused_argmax || dtype != SIMULST_BF16 || !packed || V % 64 != 0 || D % 32 != 0 || D > 256)
    return refused(base, SIMULST_E_SHAPE, "vocabulary projection with the greedy pick: shape not taken");
  // Whether the shape is taken is asked WITH a LayerNorm, whatever the model has (any non-null affine: the prologue is part of the
  // shape test).  The split panel writes fp32 pairs in its LayerNorm form only: without a final LayerNorm the 64 x 64 tile runs.
  const LinArgs p = sl_vocab_args(B, V, D, (const float*)h, (const float*)h);
  const sl_linear_plan pl = plan_decode_step(h, base, p);
  if (pl.family != SL_LIN_PANEL_SPLIT && pl.family != SL_LIN_MID)
    return refused(base, SIMULST_E_SHAPE, "vocabulary projection with the greedy pick: shape not taken");
  return has_ln ? pl : plan_mid(base, p);
}
