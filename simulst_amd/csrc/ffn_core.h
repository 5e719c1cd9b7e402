// What the fused Emformer feed-forward kernels share (ffn_fused.hip: the block form; ffn_pipe.hip: the software-pipelined forms and,
// in EXPERIMENTS builds, experiments/ffn_pipe_forms.inc) -- gfx950, bf16, D = 256: the pieces AROUND the tile loop.  A wave owns 32
// rows; lane (lr = lane & 31, lh = lane >> 5).  Everything here is __forceinline__ and so compiled under the including file's own
// flags (ffn_pipe.hip: without the SLP vectoriser, Makefile).
#pragma once
#include "gemm_args.h"
#include "ffn_variant.h"

// the launchers of ffn_pipe.hip that simulst_emformer_ffn* (ffn_fused.hip) hand over to
int sl_launch_qkv_rows(simulst_handle* h, const void* z, const void* wqkv_fm, const float* bqkv, void* qkv, int n_utt, int rows_z, int n_mem,
                       int sum0, int n_sum);
int sl_launch_ffn_pipe(simulst_handle* h, const void* x, const float* ln_g, const float* ln_b, const void* w1p, const float* b1,
                       const void* w2p, const float* b2, void* out, long rows, int F, sl_ffn_variant v, const sl_ffn_z* zout = nullptr);

namespace ffn {

constexpr int FF_D = 256;              // model width (K of fc1, N of fc2)
constexpr int FF_PF = 4;               // weight fragments requested ahead of the MFMA that consumes them
constexpr int FF_RS = FF_D * 2;        // a staged output row in bytes: a wave's 32 rows = 16 KB
constexpr int FF_PARAM_BYTES = 3072;   // LDS parameter block without the fc1 bias

typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void gbl_void;

__device__ __forceinline__ unsigned int pack_bf16x2(float lo, float hi) {
  const bf16 l = __float2bfloat16(lo), h = __float2bfloat16(hi);
  return (unsigned int)(*reinterpret_cast<const unsigned short*>(&l)) |
         ((unsigned int)(*reinterpret_cast<const unsigned short*>(&h)) << 16);
}

// The LDS parameter block behind the weight buffers: LayerNorm gamma | beta | fc2 bias (FF_D floats each) | fc1 bias (F floats).
// The fc1 bias is there because an ordinary global load inside the loop would make hipcc drain the in-flight LDS-DMA (vmcnt(0)) at
// its use.  The kernels fill it themselves, two loops over their threads (the uniform schedule of ffn_pipe.hip stores HALF the fc1 bias):
// as a function here the fill cost every shipped kernel one more scalar instruction, and they are compared opcode for opcode.
struct Params { float *lng, *lnb, *b2s, *b1s; };
__device__ __forceinline__ Params params_at(char* at) {
  float* f = reinterpret_cast<float*>(at);
  return {f, f + FF_D, f + 2 * FF_D, f + 3 * FF_D};
}

// rows [row0, row0 + 32) as B-operand fragments of Ht = W1 . LN(x)^T: lane (lr, lh) holds x[row lr][16 s + 8 lh + j]; rows from
// row_end on are zeros
__device__ __forceinline__ void load_rows(uint4 (&xa)[16], const bf16* X, long row0, long row_end, int lr, int lh) {
  const long r = row0 + lr;
  const bool ok = r < row_end;
  const bf16* xr = X + (ok ? r : 0) * FF_D + lh * 8;
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const uint4 v = ld16(xr + s * 16);
    xa[s] = make_uint4(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u);
  }
}

// ... LayerNorm-ed in place: the two lanes of a row add their moments, gamma / beta from LDS
__device__ __forceinline__ void layer_norm_rows(uint4 (&xa)[16], const float* lng, const float* lnb, int lh) {
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int s = 0; s < 16; ++s) moments_mid(xa[s], s1, s2, bf16());
  s1 += __shfl_xor(s1, 32, 64);
  s2 += __shfl_xor(s2, 32, 64);
  const float mean = s1 * (1.0f / FF_D);
  const float rstd = 1.0f / sqrtf(fmaxf(s2 * (1.0f / FF_D) - mean * mean, 0.f) + 1e-5f);
#pragma unroll
  for (int s = 0; s < 16; ++s) xa[s] = ln_frag_mid(xa[s], mean, rstd, lng, lnb, s * 16 + lh * 8, bf16());
}

// Epilogue, first half: y[n][e] = Y[row (e & 3) + 8 (e >> 2) + 4 lh][col 32 n + lr], + b2, as bf16 rows into staging area `slot` of
// the weight buffers (16 KB each, the wave's own; every wave must be done with the weights).  stage_sync() before the rows are read
// back.  (The area is given as base and number, not as a pointer: the address arithmetic of the stores then comes out of hipcc as it
// did written inside the kernels, which the shipped kernels are compared against.)
__device__ __forceinline__ void stage_rows(char* lds, int slot, const f32x16 (&y)[8], const float* b2s, int lr, int lh) {
  char* st = lds + slot * (32 * FF_RS);
#pragma unroll
  for (int n = 0; n < 8; ++n) {
    const float bv = b2s[n * 32 + lr];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int r = (e & 3) + 8 * (e >> 2) + 4 * lh;
      *reinterpret_cast<bf16*>(st + r * FF_RS + (n * 32 + lr) * 2) = __float2bfloat16(y[n][e] + bv);
    }
  }
}
__device__ __forceinline__ void stage_sync() {
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// 16 bytes of a staged row + the same 16 bytes of the residual row -> 8 bf16 of the output row
__device__ __forceinline__ uint4 add_residual(const uint4 yv, const uint4 xv) {
  const unsigned int yu[4] = {yv.x, yv.y, yv.z, yv.w}, xu[4] = {xv.x, xv.y, xv.z, xv.w};
  unsigned int ou[4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
    ou[q] = pack_bf16x2(__uint_as_float(yu[q] << 16) + __uint_as_float(xu[q] << 16),
                        __uint_as_float(yu[q] & 0xffff0000u) + __uint_as_float(xu[q] & 0xffff0000u));
  return make_uint4(ou[0], ou[1], ou[2], ou[3]);
}

// Epilogue, second half: the 2 * PAIRS rows staged from area `slot` on leave whole, with the residual added (32 lanes x 16 B = one
// 512-byte row), by streaming stores
template <int PAIRS = 16>
__device__ __forceinline__ void store_rows(const char* lds, int slot, const bf16* X, bf16* out, long row0, long row_end, int lr, int lh) {
  const char* st = lds + slot * (32 * FF_RS);
#pragma unroll
  for (int it = 0; it < PAIRS; ++it) {
    const int rl = it * 2 + lh;
    const long r = row0 + rl;
    if (r >= row_end) continue;
    const uint4 yv = *reinterpret_cast<const uint4*>(st + rl * FF_RS + lr * 16);
    const uint4 xv = ld16(X + r * FF_D + lr * 8);
    st_stream16(out + r * FF_D + lr * 8, add_residual(yv, xv));
  }
}

}  // namespace ffn
