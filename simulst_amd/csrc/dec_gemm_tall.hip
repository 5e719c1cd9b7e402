// Tall decode-step GEMM with a long contraction for gfx950: fc2 + residual of co-scheduled batches (thousands of rows, K = F = 2048,
// N = D = 256), bf16, fragment-major weights.
//
// simulst_linear runs this shape on skinny_kernel (gemm_skinny.hip): a 64 x 32 tile per workgroup whose four waves interleave the
// k-steps and add their partial tiles through LDS -- 384 KB of operands through the L1 per 8 MFLOP, every wave waiting for its own
// loads before each group of MFMAs.  Here a workgroup owns a 64 x 64 tile, wave w its rows [16 w, 16 w + 16) and all 64 columns:
//   * A fragments go global -> registers (a row is read by one wave only); the 64 x K weight block, the only operand the waves share,
//     goes through LDS in chunks of 8 k-steps (32 KB), TWO stages
//   * the global loads of chunk c + 1 (A and W) are issued BEFORE the MFMAs of chunk c, the registers holding the weight block are
//     written to the other LDS stage AFTER them: one barrier per chunk, the next operands in flight while the matrix core works
//   * workgroup ids are permuted like skinny_kernel's so that an XCD works through consecutive tiles (the column tiles of a row tile
//     share that XCD's L2 copy of the rows)
// THE SAME BITS as skinny_kernel: that kernel's wave w accumulates the k-steps s = w (mod 4) in ascending order and the four partial
// tiles are added as ((p0 + p1) + p2) + p3, then + bias, + residual, one rounding.  A wave here keeps FOUR accumulators per 16 x 16
// tile, k-step s goes to accumulator s & 3, and the epilogue adds them in that order (tests/test_hip_dec_tall_gemm.py compares bytes).
// Rows >= M and columns >= N are loaded from clamped (in-bounds) addresses: a row of A / a column of W reaches only its own output row /
// column, which is never stored.  K tail k-steps are zeroed on both operands, as in skinny_kernel; the two kernels pad to different
// trip counts (8 k-steps here, 4 * UNR there), so an accumulator sees a different number of all-zero MFMAs -- neutral, because an
// accumulator that starts at +0 never holds -0 (x + y is -0 only when both are), and +0 products leave every other value as it is.
#include "decode_plan.h"
#include "gemm_plan.h"

namespace {

constexpr int DT_CH = 8;                           // k-steps per chunk
constexpr int DT_STAGE = 4 * DT_CH * 64;           // uint4 slots of one weight stage: 4 column tiles x CH k-steps x 64 lanes (32 KB)

__global__ __launch_bounds__(256) void dec_tall_fc2_kernel(const bf16* __restrict__ A, const bf16* __restrict__ W,
                                                           const float* __restrict__ bias, const bf16* R, bf16* C, int M, int N, int K) {
  constexpr int KS = 32, G = 8;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * DT_STAGE * 16];
  uint4* wl = reinterpret_cast<uint4*>(smem);                            // [stage][j][s][lane]
  float (*tile)[65] = reinterpret_cast<float (*)[65]>(smem);             // epilogue: 64 x 65 fp32, then the tile's 64 bias values
  float* lbias = reinterpret_cast<float*>(smem + 64 * 65 * sizeof(float));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  int bx, by;
  {
    const int id = (int)blockIdx.x + (int)gridDim.x * (int)blockIdx.y, total = (int)(gridDim.x * gridDim.y);
    const int full = total & ~7;
    const int bid = id < full ? (id & 7) * (full >> 3) + (id >> 3) : id;
    bx = bid % (int)gridDim.x;
    by = bid / (int)gridDim.x;
  }
  const int n0 = bx * 64, m0 = by * 64;
  const int nks = K / KS, nch = (nks + DT_CH - 1) / DT_CH, ntile = N >> 4;      // host: K % 32 == 0, N % 16 == 0
  // ---- epilogue operands requested up front: row m0 + tid / 4, 16 consecutive columns per thread (C may alias R: a thread reads
  //      exactly the elements it writes)
  const int er = tid >> 2, ec = (tid & 3) * 16;
  const bool eok = m0 + er < M && n0 + ec < N;
  const long eoff = eok ? (long)(m0 + er) * N + n0 + ec : 0;
  const uint4 rpre0 = ld16(R + eoff), rpre1 = ld16(R + eoff + 8);
  const float bpre = (tid < 64 && bias && n0 + tid < N) ? bias[n0 + tid] : 0.f;
  // ---- operand sources
  const bf16* arow = A + (long)min(m0 + wave * 16 + lr, M - 1) * K + lg * G;
  const bf16* wlane = W + lane * G;
  uint4 faN[DT_CH], wv[DT_CH];
  // chunk c: this lane's A fragments of its k-steps; weight slot q * 256 + tid = (column tile q / 2, k-step (q & 1) * 4 + wave, lane)
  auto load_chunk = [&](int c) {
#pragma unroll
    for (int u = 0; u < DT_CH; ++u) {
      const int s = c * DT_CH + u;
      faN[u] = ld16(arow + (s < nks ? s : 0) * KS);
    }
#pragma unroll
    for (int q = 0; q < DT_CH; ++q) {
      const int s = c * DT_CH + (q & 1) * 4 + wave, tj = (n0 >> 4) + (q >> 1);
      const bool ok = s < nks && tj < ntile;
      wv[q] = ld16(wlane + ((long)(ok ? tj : 0) * nks + (ok ? s : 0)) * (64 * G));
    }
  };
  auto store_chunk = [&](int c, uint4* dst) {
#pragma unroll
    for (int q = 0; q < DT_CH; ++q) {
      const int s = c * DT_CH + (q & 1) * 4 + wave, tj = (n0 >> 4) + (q >> 1);
      const bool ok = s < nks && tj < ntile;
      dst[q * 256 + tid] = make_uint4(ok ? wv[q].x : 0u, ok ? wv[q].y : 0u, ok ? wv[q].z : 0u, ok ? wv[q].w : 0u);
    }
  };
  f32x4 acc[4][4];                                                       // [k-step & 3][column tile]
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  load_chunk(0);
  store_chunk(0, wl);
  for (int c = 0; c < nch; ++c) {
    uint4 fa[DT_CH];
#pragma unroll
    for (int u = 0; u < DT_CH; ++u) fa[u] = faN[u];
    if ((c + 1) * DT_CH > nks) {                                         // k tail (last chunk only)
#pragma unroll
      for (int u = 0; u < DT_CH; ++u)
        if (c * DT_CH + u >= nks) fa[u] = make_uint4(0u, 0u, 0u, 0u);
    }
    const bool more = c + 1 < nch;
    if (more) load_chunk(c + 1);                                         // in flight across this chunk's MFMAs
    __syncthreads();                                                     // stage c & 1 is written; the other stage's readers are done
    const uint4* wb = wl + (c & 1) * DT_STAGE;
    uint4 wf[2][4];                                                      // the four fragments of k-step u + 1 are read behind u's MFMAs
#pragma unroll
    for (int j = 0; j < 4; ++j) wf[0][j] = wb[(j * DT_CH) * 64 + lane];
#pragma unroll
    for (int u = 0; u < DT_CH; ++u) {
      if (u + 1 < DT_CH) {
#pragma unroll
        for (int j = 0; j < 4; ++j) wf[(u + 1) & 1][j] = wb[(j * DT_CH + u + 1) * 64 + lane];
      }
      __builtin_amdgcn_sched_barrier(0);                                 // (the scheduler would sink each read to just above its MFMA)
      const bf16x8_t af = *reinterpret_cast<const bf16x8_t*>(&fa[u]);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[u & 3][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, *reinterpret_cast<const bf16x8_t*>(&wf[u & 1][j]), acc[u & 3][j], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (more) store_chunk(c + 1, wl + ((c + 1) & 1) * DT_STAGE);
  }
  // ---- the four k-step streams in skinny_kernel's order -> LDS tile: acc[.][j][e] = C[wave*16 + lg*4 + e][j*16 + lr]
  __syncthreads();                                                       // every wave is past its last fragment read
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      tile[wave * 16 + lg * 4 + e][j * 16 + lr] = ((acc[0][j][e] + acc[1][j][e]) + acc[2][j][e]) + acc[3][j][e];
  if (tid < 64) lbias[tid] = bpre;
  __syncthreads();
  if (!eok) return;
  float y[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const unsigned int w = reinterpret_cast<const unsigned int*>(e < 8 ? &rpre0 : &rpre1)[(e & 7) >> 1];
    float v = tile[er][ec + e] + lbias[ec + e];
    v += __uint_as_float((e & 1) ? (w & 0xffff0000u) : (w << 16));
    y[e] = v;
  }
  bf16* cp = C + eoff;
#pragma unroll
  for (int e = 0; e < 16; e += 4) store4(cp + e, reinterpret_cast<const float(&)[4]>(y[e]));
}

// fc1 of the same step: LN3 + [B][K <= 256] x [N][K]^T + bias + GELU, the launch simulst_linear runs on the split row panel
// (gemm_panel.hip panel_kernel<BIAS_GELU, true>).  That kernel writes a step's weight block to its ONE LDS stage at the top of the step
// behind s_waitcnt vmcnt(0) -- which also waits for the previous step's output stores, issued later than the weight request -- between
// two barriers.  Here: the same 128-row panel and A fragments held in registers, TWO weight stages, the next step's block requested at the
// top of a step and written to the other stage right after the step's MFMAs (the only older requests then are the stores of the step
// BEFORE, a whole MFMA phase old), one barrier per step, outputs stored straight from the accumulators (a lane holds 4 consecutive
// columns of a row: 8-byte stores), and column ranges of DT_F1_STEPS steps so that two workgroups share a CU.
// THE SAME BITS as panel_kernel: the same LayerNorm (moments per lane over ascending k-steps, the xor 16 / xor 32 exchange, ln_frag_mid),
// the weights as the MFMA's first operand, ONE accumulator per tile over ascending k-steps, bias add, gelu_fast2 on the column pairs
// (0, 1) and (2, 3), one rounding.
constexpr int DT_F1_STEPS = 2;                     // 64-column steps per workgroup
constexpr int DT_F1_PF = 3;                        // weight fragments in flight from LDS per wave (register ring, as panel_kernel)

__global__ __launch_bounds__(256, 2) void dec_tall_fc1_kernel(const bf16* __restrict__ A, const bf16* __restrict__ Wp,
                                                              const float* __restrict__ bias, const float* __restrict__ ln_g,
                                                              const float* __restrict__ ln_b, bf16* __restrict__ C, int M, int N, int K) {
  __shared__ __attribute__((aligned(16))) uint4 wl[2][4 * 8 * 64];       // [stage][j][s][lane], 2 x 32 KB
  // the LayerNorm affine sits in stage 1 until the first step's barrier: nobody writes that stage before it
  float* lng = reinterpret_cast<float*>(wl[1]);
  float* lnb = lng + 256;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int m0 = blockIdx.x * 128;
  const int nks = K / 32;                                                // host: K % 32 == 0, K <= 256
  uint4 fa[2][8];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int ar = m0 + wave * 32 + m * 16 + lr;
    const bool aok = ar < M;
    const bf16* arow = A + (long)(aok ? ar : 0) * K;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const bool ok = aok && s < nks;
      const uint4 v = ld16(arow + (ok ? s * 32 + lg * 8 : 0));
      fa[m][s] = make_uint4(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u);
    }
  }
  const int n_all = (N + 63) / 64;
  const int step0 = blockIdx.y * DT_F1_STEPS, n_steps = min(n_all, step0 + DT_F1_STEPS);
  uint4 wv[8];
  auto wload = [&](int step) {                                           // slot q * 256 + tid = (j, s, lane)
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int slot = q * 256 + tid;
      const int ln = slot & 63, s = (slot >> 6) & 7, j = slot >> 9;
      const int ntile = step * 4 + j;
      const bool ok = s < nks && ntile * 16 < N;
      const uint4 v = ld16(Wp + (((long)(ok ? ntile : 0) * nks + (ok ? s : 0)) * 64 + ln) * 8);
      wv[q] = make_uint4(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u);
    }
  };
  float4 bnext[4];
  auto bload = [&](int step) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = step * 64 + j * 16 + 4 * lg;
      bnext[j] = (bias && c < N) ? *reinterpret_cast<const float4*>(bias + c) : float4{0.f, 0.f, 0.f, 0.f};
    }
  };
  wload(step0);
  bload(step0);
  for (int k = tid; k < K; k += 256) { lng[k] = ln_g[k]; lnb[k] = ln_b[k]; }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int s = 0; s < 8; ++s) moments_mid(fa[m][s], s1, s2, bf16());
    s1 += __shfl_xor(s1, 16, 64); s2 += __shfl_xor(s2, 16, 64);
    s1 += __shfl_xor(s1, 32, 64); s2 += __shfl_xor(s2, 32, 64);
    const float mean = s1 / (float)K;
    const float rstd = 1.0f / sqrtf(fmaxf(s2 / (float)K - mean * mean, 0.f) + 1e-5f);
#pragma unroll
    for (int s = 0; s < 8; ++s)
      if (s < nks) fa[m][s] = ln_frag_mid(fa[m][s], mean, rstd, lng, lnb, s * 32 + lg * 8, bf16());
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) wl[0][q * 256 + tid] = wv[q];
  for (int step = step0; step < n_steps; ++step) {
    const int cur = (step - step0) & 1;
    float4 bcur[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bcur[j] = bnext[j];
    const bool more = step + 1 < n_steps;
    if (more) { wload(step + 1); bload(step + 1); }
    __syncthreads();                                                     // stage cur is written; the other stage's readers are done
    f32x4 acc[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[m][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const uint4* wb = wl[cur];
    u32x4_t wfr[DT_F1_PF];
#pragma unroll
    for (int f = 0; f < DT_F1_PF - 1; ++f) wfr[f] = *reinterpret_cast<const u32x4_t*>(&wb[((f & 3) * 8 + (f >> 2)) * 64 + lane]);
#pragma unroll
    for (int f = 0; f < 32; ++f) {                                       // fragment f = (k-step f / 4, column tile f % 4)
      const int s = f >> 2, j = f & 3;
      if (f + DT_F1_PF - 1 < 32) {
        const int g2 = f + DT_F1_PF - 1;
        wfr[g2 % DT_F1_PF] = *reinterpret_cast<const u32x4_t*>(&wb[((g2 & 3) * 8 + (g2 >> 2)) * 64 + lane]);
      }
#pragma unroll
      for (int m = 0; m < 2; ++m)
        acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wfr[f % DT_F1_PF]),
                                                           *reinterpret_cast<const bf16x8_t*>(&fa[m][s]), acc[m][j], 0, 0, 0);
      // the fragment stays alive past both MFMAs that read it (panel_kernel explains the destination-on-source allocation)
      asm volatile("" :: "v"(wfr[f % DT_F1_PF]), "v"(acc[0][j]), "v"(acc[1][j]));
    }
    if (more) {
#pragma unroll
      for (int q = 0; q < 8; ++q) wl[cur ^ 1][q * 256 + tid] = wv[q];
    }
    // ---- epilogue from the accumulators: acc[m][j][e] = C[32 w + 16 m + lr][64 step + 16 j + 4 lg + e]
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int r = m0 + wave * 32 + m * 16 + lr;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = step * 64 + j * 16 + 4 * lg;
        const float4 bv = bcur[j];
        f32x2 v0 = f32x2{acc[m][j][0] + bv.x, acc[m][j][1] + bv.y};
        f32x2 v1 = f32x2{acc[m][j][2] + bv.z, acc[m][j][3] + bv.w};
        v0 = gelu_fast2(v0);
        v1 = gelu_fast2(v1);
        const bf16 o0 = __float2bfloat16(v0.x), o1 = __float2bfloat16(v0.y), o2 = __float2bfloat16(v1.x), o3 = __float2bfloat16(v1.y);
        const unsigned int lo = (unsigned int)(*reinterpret_cast<const unsigned short*>(&o0)) |
                                ((unsigned int)(*reinterpret_cast<const unsigned short*>(&o1)) << 16);
        const unsigned int hi = (unsigned int)(*reinterpret_cast<const unsigned short*>(&o2)) |
                                ((unsigned int)(*reinterpret_cast<const unsigned short*>(&o3)) << 16);
        if (r < M && c < N) *reinterpret_cast<uint2*>(C + (long)r * N + c) = make_uint2(lo, hi);      // N % 16 == 0: 4 columns in or out
      }
    }
  }
}

}  // namespace

// contiguous operands: A [B][K], W fragment-major [N][K], R / C [B][N] (C may alias R); the caller has asked sl_dec_tall_fc2_ok
int sl_dec_tall_fc2(simulst_handle* h, const void* A, const void* W, const float* bias, const void* R, void* C, int B, int N, int K) {
  KTimer t(h, SIMULST_K_DEC_TALL_GEMM);
  hipLaunchKernelGGL(dec_tall_fc2_kernel, dim3((N + 63) / 64, (B + 63) / 64), dim3(256), 0, h->stream, (const bf16*)A, (const bf16*)W,
                     bias, (const bf16*)R, (bf16*)C, B, N, K);
  return sl_launch_status(h, "decode step: tall fc2 tile");
}

// contiguous operands: A [B][K], W fragment-major [N][K], C [B][N]; the caller has asked sl_dec_tall_fc1_ok
int sl_dec_tall_fc1(simulst_handle* h, const void* A, const void* W, const float* bias, const float* ln_g, const float* ln_b, void* C,
                    int B, int N, int K) {
  KTimer t(h, SIMULST_K_DEC_TALL_GEMM);
  const int n_all = (N + 63) / 64;
  hipLaunchKernelGGL(dec_tall_fc1_kernel, dim3((B + 127) / 128, (n_all + DT_F1_STEPS - 1) / DT_F1_STEPS), dim3(256), 0, h->stream,
                     (const bf16*)A, (const bf16*)W, bias, ln_g, ln_b, (bf16*)C, B, N, K);
  return sl_launch_status(h, "decode step: tall fc1 panel");
}

extern "C" int simulst_dec_tall_fc1(simulst_handle* h, const void* A, const void* W, const float* bias, const float* ln_g,
                                    const float* ln_b, void* C, int32_t B, int32_t N, int32_t K, int32_t dtype) {
  if (!h) return SIMULST_E_NULL;
  SL_CHECK_NULL(h, A);
  SL_CHECK_NULL(h, W);
  SL_CHECK_NULL(h, ln_g);
  SL_CHECK_NULL(h, ln_b);
  SL_CHECK_NULL(h, C);
  SL_REQUIRE(h, B > 0 && N > 0 && K > 0, SIMULST_E_SHAPE, "simulst_dec_tall_fc1: non-positive shape");
  SL_REQUIRE(h, sl_dec_tall_fc1_shape_ok(h, dtype, B, N, K, true), SIMULST_E_SHAPE,
             "simulst_dec_tall_fc1: bf16 rows whose simulst_linear launch is the split row panel");
  SL_REQUIRE(h, sl_dec_tall_operands_ok(A, W, C, bias), SIMULST_E_ARG, "simulst_dec_tall_fc1: operands must be 16-byte aligned");
  return sl_dec_tall_fc1(h, A, W, bias, ln_g, ln_b, C, B, N, K);
}

extern "C" int simulst_dec_tall_gemm(simulst_handle* h, const void* A, const void* W, const float* bias, const void* R, void* C,
                                     int32_t B, int32_t N, int32_t K, int32_t dtype) {
  if (!h) return SIMULST_E_NULL;
  SL_CHECK_NULL(h, A);
  SL_CHECK_NULL(h, W);
  SL_CHECK_NULL(h, R);
  SL_CHECK_NULL(h, C);
  SL_REQUIRE(h, B > 0 && N > 0 && K > 0, SIMULST_E_SHAPE, "simulst_dec_tall_gemm: non-positive shape");
  SL_REQUIRE(h, sl_dec_tall_fc2_shape_ok(h, dtype, B, N, K, true), SIMULST_E_SHAPE,
             "simulst_dec_tall_gemm: bf16 rows whose simulst_linear launch is the k-interleaved 16 MT x 16 NT tile without split-K");
  SL_REQUIRE(h, sl_dec_tall_operands_ok(A, W, R, C), SIMULST_E_ARG, "simulst_dec_tall_gemm: operands must be 16-byte aligned");
  return sl_dec_tall_fc2(h, A, W, bias, R, C, B, N, K);
}
