// Stand-alone driver of the host-side launch decisions (tests/test_linear_plan.py builds it against the library's object files; it
// needs no GPU and launches nothing).  Every input line starts with the handle: n_cus and the nine GEMM options, -1 = as created.
//   plan   < rows    one line per simulst_linear call: sl_plan_linear's family, grid, dynamic LDS and variant flags, or its refusal
//   vocab  < rows    B V D has_ln per line: what sl_plan_vocab_argmax takes (mid / panel_split / none), its grid and LayerNorm form
//   floor            sl_retire_floor_rows for B = 1 .. 9000, at the defaults and at one override of each of the five GEMM thresholds
// `floor` also builds against the sources of the commit before gemm_plan.h existed: that is how its expected table
// (tests/golden/g26_linear_plan.json) was recorded.
#include <cstdio>
#include <cstring>
#include "decode_plan.h"
#if __has_include("gemm_plan.h")
#include "gemm_plan.h"
#define HAVE_PLAN 1
#else
#define HAVE_PLAN 0
#endif

static simulst_handle* make_handle(const long* v) {
  simulst_handle* h = nullptr;
  if (simulst_create(&h, nullptr) != SIMULST_OK) { fprintf(stderr, "simulst_create failed\n"); exit(2); }
  if (v[0] >= 0) h->n_cus = (int)v[0];
  if (v[1] >= 0) h->wstat = v[1] != 0;
  if (v[2] >= 0) h->panel_wide = v[2] != 0;
  if (v[3] >= 0) h->tile256 = (int)v[3];
  if (v[4] >= 0) h->fused_argmax = v[4] != 0;
  if (v[5] >= 0) h->panel_split_min_rows = (int)v[5];
  if (v[6] >= 0) h->panel_split_blocks = (int)v[6];
  if (v[7] >= 0) h->mid_min_blocks = (int)v[7];
  if (v[8] >= 0) h->mid_narrow_min_rows = (int)v[8];
  if (v[9] >= 0) h->skinny_min_blocks_tall = (int)v[9];
  return h;
}

static int read_longs(long* v, int n) {
  for (int i = 0; i < n; ++i)
    if (scanf("%ld", &v[i]) != 1) return i == 0 ? 0 : -1;
  return 1;
}

#if HAVE_PLAN
static const char* FAMILY[] = {"refused", "wstat", "panel_wide", "panel", "panel_split", "mid", "wave_tile", "skinny", "tile256", "tile128", "tile64"};

static void print_plan(const sl_linear_plan& pl) {
  if (pl.family == SL_LIN_REFUSED) { printf("refused %d %s\n", pl.status, pl.err); return; }
  printf("%s grid %u %u %u lds %u timer %d ln %d tall %d ring %d pairs %d n_slices %d MTs %d NTs %d splits %d kps %d spb %d tiles_n %d\n",
         FAMILY[pl.family], pl.grid[0], pl.grid[1], pl.grid[2], pl.lds, pl.timer, (int)pl.ln, (int)pl.tall, (int)pl.ring, pl.pairs, pl.n_slices,
         pl.MTs, pl.NTs, pl.splits, pl.kps, pl.spb, pl.tiles_n);
}

static int plan_mode() {
  long v[10 + 26];
  static float affine[1];
  int r;
  while ((r = read_longs(v, 36)) == 1) {
    simulst_handle* h = make_handle(v);
    const long* c = v + 10;      // dtype epi batches rpb N K a_bs a_rs a_lead c_bs c_rs r_bs r_rs n_main aux_rows aux_bs ln packed c_hd c_hs c_th c_ts misA misC misR misBias
    LinArgs p = {};
    p.M = (int)(c[2] * c[3]); p.rpb = (int)c[3]; p.N = (int)c[4]; p.K = (int)c[5];
    p.a_bs = c[6]; p.a_rs = c[7]; p.a_lead = c[8]; p.c_bs = c[9]; p.c_rs = c[10]; p.r_bs = c[11]; p.r_rs = c[12];
    p.scale = 1.f; p.n_main = (int)c[13]; p.aux_rows = (int)c[14]; p.aux_bs = c[15];
    p.ln_g = p.ln_b = c[16] ? affine : nullptr;
    p.w_packed = (int)c[17]; p.c_hd = (int)c[18]; p.c_hs = c[19]; p.c_th = (int)c[20]; p.c_ts = c[21];
    p.amax_skip_a = p.amax_skip_b = -1;
    // only the low bits of the operand pointers enter the decision
    const uintptr_t base = 1 << 20;
    const sl_linear_ops o = {(const void*)(base + 8 * c[22]), (const void*)base, (const float*)(base + 2 * c[25]), (const void*)(base + 8 * c[24]),
                             (void*)(base + 8 * c[23]), (void*)base};
    print_plan(sl_plan_linear(h, (int)c[0], (int)c[1], p, o));
    simulst_destroy(h);
  }
  return r < 0 ? 2 : 0;
}

static int vocab_mode() {
  long v[14];
  int r;
  while ((r = read_longs(v, 14)) == 1) {
    simulst_handle* h = make_handle(v);
    const sl_linear_plan pl = sl_plan_vocab_argmax(h, SIMULST_BF16, (int)v[10], (int)v[11], (int)v[12], true, v[13] != 0);
    if (pl.family == SL_LIN_REFUSED) printf("none\n");
    else printf("%s grid %u %u ln %d\n", FAMILY[pl.family], pl.grid[0], pl.grid[1], (int)pl.ln);
    simulst_destroy(h);
  }
  return r < 0 ? 2 : 0;
}
#endif

static int floor_mode() {
  //                    panel_split_min_rows, panel_split_blocks, mid_min_blocks, mid_narrow_min_rows, skinny_min_blocks_tall
  static const long sets[6][10] = {{-1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {-1, -1, -1, -1, -1, 2048, -1, -1, -1, -1},
                                   {-1, -1, -1, -1, -1, -1, 128, -1, -1, -1}, {-1, -1, -1, -1, -1, -1, -1, 40, -1, -1},
                                   {-1, -1, -1, -1, -1, -1, -1, -1, 1024, -1}, {-1, -1, -1, -1, -1, -1, -1, -1, -1, 184}};
  for (int s = 0; s < 6; ++s) {
    simulst_handle* h = make_handle(sets[s]);
    for (int B = 1; B <= 9000; ++B) printf("%d %d %d\n", s, B, sl_retire_floor_rows(h, B));
    simulst_destroy(h);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "floor")) return floor_mode();
#if HAVE_PLAN
  if (argc == 2 && !strcmp(argv[1], "plan")) return plan_mode();
  if (argc == 2 && !strcmp(argv[1], "vocab")) return vocab_mode();
#endif
  fprintf(stderr, "usage: linear_plan_table plan|vocab|floor\n");
  return 2;
}
