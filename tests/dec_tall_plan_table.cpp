// Stand-alone driver of the decode plan's tall-GEMM flag (tests/test_hip_dec_tall_gemm.py builds it against the library's object
// files; it needs no GPU and launches nothing).  One line "set B tall_ffn chain_ffn tall_fc1" for B = 1 .. 9000 and every set:
//   0 bf16 MMA loop at the handle's defaults      1 the same with SIMULST_OPT_DEC_TALL_FFN = 0      2 fp32
//   3 bf16 with the one-launch-per-GEMM test hook (force_unfused)      4 bf16 CIF loop at the defaults
//   5 bf16 MMA loop, row-major weights      6 bf16 MMA loop at D = 512 (simulst_linear runs that fc2 on the 64 x 64 tile: not taken)
#include <cstdio>
#include "decode_plan.h"

int main() {
  for (int set = 0; set < 7; ++set) {
    simulst_handle* h = nullptr;
    if (simulst_create(&h, nullptr) != SIMULST_OK) { fprintf(stderr, "simulst_create failed\n"); return 2; }
    if (set == 1 && simulst_set_option(h, SIMULST_OPT_DEC_TALL_FFN, 0) != SIMULST_OK) return 2;
    for (int B = 1; B <= 9000; ++B) {
      sl_decode_call c = {};
      c.dtype = set == 2 ? SIMULST_F32 : SIMULST_BF16;
      c.B = B; c.D = set == 6 ? 512 : 256; c.H = 4; c.F = 2048; c.V = 8192; c.cap = 128; c.S_cap = 128;
      c.attn_type = SIMULST_ATTN_WAITK;
      c.packed = set != 5;
      c.x_mid = true; c.partial_self = false; c.ffn_partial = true; c.final_ln = true;
      c.mode = SL_CALL_OFFLINE; c.np_uniform = 0; c.compact = false; c.mask_eos = true;
      c.force_unfused = set == 3;
      c.cif = set == 4; c.highway = false;
      const sl_decode_plan p = sl_plan_decode(h, c);
      printf("%d %d %d %d %d\n", set, B, (int)p.tall_ffn, (int)p.chain_ffn, (int)p.tall_fc1);
    }
    simulst_destroy(h);
  }
  return 0;
}
