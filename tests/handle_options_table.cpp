// Stand-alone driver of the handle's tunables (tests/test_handle_options.py builds it with csrc/handle.cpp in each build flavour; it
// needs no GPU and launches nothing: simulst_create then leaves n_cus 0).
//   table  < lines   one handle per line, "NAME=value NAME=value ; option value option value": created under that environment, then the
//                    simulst_set_option calls in order.  Prints one line: the status of each call, every tunable field by name, and
//                    simulst_get_option's status:value for ids 0 .. 16 and 99.
//   ffn    < lines   "code F" per line: sl_decode_ffn_variant's pipelined, waves, packed, uniform for that SIMULST_OPT_FFN_WAVES code
//   time N           N simulst_create / simulst_destroy pairs, nanoseconds per pair
// It builds unchanged against the sources of the commit before the option table existed: that is how its expected output
// (tests/golden/g27_handle_options.json) was recorded.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "common.h"
#if __has_include("ffn_variant.h")
#include "ffn_variant.h"
#define HAVE_FFN_VARIANT 1
#else
#define HAVE_FFN_VARIANT 0
#endif

static void print_fields(const simulst_handle* h) {
#define F(name) printf(" " #name " %d", (int)h->name)
  F(force_valu_attention); F(force_unfused_decode); F(ffn_waves); F(ffn_variant); F(ea_general_only);
  F(panel_split_min_rows); F(panel_split_blocks); F(mid_min_blocks); F(mid_narrow_min_rows); F(skinny_min_blocks_tall); F(fuse_q_max_rows);
  F(dec_chain_on); F(dec_chain_min_rows); F(dec_chain_max_rows); F(dec_chain_ffn_max_rows); F(dec_tall_ffn); F(dec_tall_min_rows);
  F(dec_chain_lds_bytes); F(dec_chain_xmode); F(dec_attn_chain_max_rows); F(dec_attn_chain_rows); F(dec_vocab_chain_split);
  F(dec_embed_qkv_chain); F(dec_chain_rows32); F(dec_chain_rows32_min); F(dec_fuse_ffn_qkv); F(dec_fuse_proj_cross);
  F(tile256); F(wstat); F(n_cus); F(panel_wide); F(panel_wide_plain_stores); F(policy_lds_bytes); F(fused_argmax);
#undef F
}

static int table_mode() {
  char line[4096];
  std::vector<std::string> set_names;
  while (fgets(line, sizeof line, stdin)) {
    for (const std::string& n : set_names) unsetenv(n.c_str());
    set_names.clear();
    char* calls = strchr(line, ';');
    if (!calls) { fprintf(stderr, "no ';' in: %s", line); return 2; }
    *calls++ = 0;
    for (char* tok = strtok(line, " \t\n"); tok; tok = strtok(nullptr, " \t\n")) {
      char* eq = strchr(tok, '=');
      if (!eq) { fprintf(stderr, "not NAME=value: %s\n", tok); return 2; }
      *eq = 0;
      setenv(tok, eq + 1, 1);
      set_names.push_back(tok);
    }
    simulst_handle* h = nullptr;
    if (simulst_create(&h, nullptr) != SIMULST_OK) { fprintf(stderr, "simulst_create failed\n"); return 2; }
    printf("set");
    int opt, val, used;
    while (sscanf(calls, "%d %d%n", &opt, &val, &used) == 2) {
      printf(" %d", simulst_set_option(h, opt, val));
      calls += used;
    }
    printf(" fields");
    print_fields(h);
    printf(" get");
    for (int id = 0; id <= 17; ++id) {
      int32_t v = -12345;
      const int rc = simulst_get_option(h, id == 17 ? 99 : id, &v);
      printf(" %d:%d", rc, (int)v);
    }
    printf("\n");
    simulst_destroy(h);
  }
  return 0;
}

#if HAVE_FFN_VARIANT
static int ffn_mode() {
  int code, F;
  while (scanf("%d %d", &code, &F) == 2) {
    const sl_ffn_variant v = sl_decode_ffn_variant(code, F);
    printf("%d %d %d %d\n", (int)v.pipelined, v.waves, v.packed, v.uniform);
  }
  return 0;
}
#endif

static int time_mode(int n) {
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < n; ++i) {
    simulst_handle* h = nullptr;
    if (simulst_create(&h, nullptr) != SIMULST_OK) return 2;
    simulst_destroy(h);
  }
  const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
  printf("%d create / destroy pairs: %.0f ns per pair\n", n, ns / n);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "table")) return table_mode();
#if HAVE_FFN_VARIANT
  if (argc == 2 && !strcmp(argv[1], "ffn")) return ffn_mode();
#endif
  if (argc == 3 && !strcmp(argv[1], "time")) return time_mode(atoi(argv[2]));
  fprintf(stderr, "usage: handle_options_table table | ffn | time N\n");
  return 2;
}
