// Whole-target (teacher-forced) decoder pass on the matrix cores (gfx950): causal self-attention over all U target positions,
// the monotonic / soft head energies of every (target, source) pair, and the expected context beta . V.
//
// Every product here is a batch of small per-head GEMMs (head_dim <= 64), so the three kernels share one shape: a 256-thread
// workgroup owns 64 query rows of one (utterance, head), each of its four waves a 16-row strip; operand tiles are staged in LDS as
// [row][k] and a wave builds 16 x 16 output tiles with v_mfma_f32_16x16x32_bf16 (bf16 activations) or v_mfma_f32_16x16x4_f32 (fp32
// activations: the matrix cores at full fp32 precision, so the fp32 pass agrees with the step kernels' fp32 dot products up to
// summation order).  Accumulators are fp32 in both: scores and softmax in fp32 (q enters the first product as given; the fp32 scores
// are scaled by head_dim^-0.5), P . V accumulated in fp32, one rounding to the activation dtype at the store.  With bf16 activations the
// probabilities are ALSO rounded to bf16 as the A operand of the second product, which is the reference's own `.type_as(q)` /
// `beta.to(v.dtype)` -- one rounding more than the step kernels (dec_attn.hip), which keep P in fp32.
#include "policy_core.h"

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

namespace {

constexpr int TF_ROWS = 64;      // query rows per workgroup (16 per wave)
constexpr int TF_KT = 32;        // keys (or pooled keys) per staged tile
constexpr int TF_DMAX = 64;      // head_dim limit

// One 16 x 16 tile per wave: acc[i] = C(row 4 (lane >> 4) + i, column lane & 15) += sum_k A[row][k] B[column][k].
// A and B live in LDS as [row][k]; KP is a multiple of 32, the leading dimensions are multiples of 16 bytes.
template <typename T> struct Tile;
template <> struct Tile<float> {
  static constexpr int PAD = 4;
  static __device__ __forceinline__ f32x4 mma(f32x4 acc, const float* A, int lda, const float* B, int ldb, int KP) {
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const float* a = A + r * lda + g;
    const float* b = B + r * ldb + g;
    for (int k = 0; k < KP; k += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[k], b[k], acc, 0, 0, 0);
    return acc;
  }
};
template <> struct Tile<bf16> {
  static constexpr int PAD = 8;
  static __device__ __forceinline__ f32x4 mma(f32x4 acc, const bf16* A, int lda, const bf16* B, int ldb, int KP) {
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const bf16* a = A + r * lda + 8 * g;
    const bf16* b = B + r * ldb + 8 * g;
    for (int k = 0; k < KP; k += 32)
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(a + k),
                                                    *reinterpret_cast<const bf16x8_t*>(b + k), acc, 0, 0, 0);
    return acc;
  }
};

// max / sum over the 16 lanes that hold one row of a 16 x 16 accumulator tile (lane & 15 = column)
__device__ __forceinline__ float row16_max(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float row16_sum(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// rows [r0, r0 + n_rows) x channels [0, d) of a [row][ld] global matrix -> LDS [n_rows][lds_ld], scaled, zero beyond row_end / d
// (the scale is applied BEFORE the rounding to T: callers pass 1 unless that rounding is meant)
template <typename T>
__device__ __forceinline__ void stage_rows(T* dst, int lds_ld, const T* src, long ld, int r0, int n_rows, int row_end, int d,
                                           int dp, float scale) {
  for (int idx = threadIdx.x; idx < n_rows * dp; idx += 256) {
    const int i = idx / dp, c = idx - i * dp;
    const int row = r0 + i;
    const float v = (row < row_end && c < d) ? to_f32(src[(long)row * ld + c]) * scale : 0.f;
    dst[i * lds_ld + c] = from_f32<T>(v);
  }
}
// keys [k0, k0 + TF_KT) x channels of V -> LDS TRANSPOSED [channel][key] (the B operand of P . V is indexed [column = channel][k = key])
template <typename T>
__device__ __forceinline__ void stage_v_t(T* dst, int lds_ld, const T* src, long ld, int k0, int key_end, int d) {
  for (int idx = threadIdx.x; idx < TF_KT * TF_DMAX; idx += 256) {
    const int kj = idx >> 6, c = idx & 63;
    const int key = k0 + kj;
    const float v = (key < key_end && c < d) ? to_f32(src[(long)key * ld + c]) : 0.f;
    dst[c * lds_ld + kj] = from_f32<T>(v);
  }
}

// ---- (a) causal self-attention over the whole target --------------------------------------------------------------------------
// qkv [B][U][3 D] -> ctx [B][U][D]; query u attends keys 0 .. u.  Keys are walked in tiles of TF_KT with a running maximum and sum
// (K / V of a head never have to fit LDS); a wave skips the tiles that lie wholly above its strip's diagonal.
template <typename T>
__global__ __launch_bounds__(256) void causal_self_attn_kernel(const T* __restrict__ qkv, T* __restrict__ ctx, int U, int H, int d,
                                                               float scale) {
  constexpr int LDQ = TF_DMAX + Tile<T>::PAD, LDV = TF_KT + Tile<T>::PAD;
  __shared__ __attribute__((aligned(16))) T Qs[TF_ROWS * LDQ];
  __shared__ __attribute__((aligned(16))) T Ks[TF_KT * LDQ];
  __shared__ __attribute__((aligned(16))) T Vt[TF_DMAX * LDV];
  __shared__ __attribute__((aligned(16))) T Ps[TF_ROWS * LDV];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * TF_ROWS, h = blockIdx.y, b = blockIdx.z;
  const int D = H * d, D3 = 3 * D, dp = (d + 31) & ~31, n_ct = (d + 15) >> 4;
  const T* base = qkv + (long)b * U * D3 + h * d;
  // q is staged as given and the fp32 scores are scaled below: head_dim^-0.5 is a power of two only at d = 16 and 64, and a scaled q
  // rounded to bf16 here would be a second rounding of q (2^-9 of every score's terms) that the step kernels do not have
  stage_rows<T>(Qs, LDQ, base, D3, q0, TF_ROWS, U, d, dp, 1.0f);
  f32x4 o[4];
  float m[4], l[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { o[i] = f32x4{0.f, 0.f, 0.f, 0.f}; m[i] = -INFINITY; l[i] = 0.f; }
  const int w0 = q0 + 16 * wave;                         // first query of this wave's strip
  const int key_end = min(U, q0 + TF_ROWS);
  for (int k0 = 0; k0 < key_end; k0 += TF_KT) {
    __syncthreads();                                     // the previous tile is consumed (first pass: Qs is complete)
    stage_rows<T>(Ks, LDQ, base + D, D3, k0, TF_KT, U, d, dp, 1.0f);
    stage_v_t<T>(Vt, LDV, base + 2 * D, D3, k0, U, d);
    __syncthreads();
    if (k0 > w0 + 15) continue;                          // wave-uniform: every key of the tile is in the strip's future
    f32x4 s[2];
#pragma unroll
    for (int n = 0; n < 2; ++n)
      s[n] = Tile<T>::mma(f32x4{0.f, 0.f, 0.f, 0.f}, Qs + 16 * wave * LDQ, LDQ, Ks + 16 * n * LDQ, LDQ, dp);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int u = w0 + 4 * g + i;
      float mx = -INFINITY;
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        s[n][i] = k0 + 16 * n + r > u ? -INFINITY : s[n][i] * scale;
        mx = fmaxf(mx, s[n][i]);
      }
      const float mt = fmaxf(m[i], row16_max(mx));       // key 0 is never in a query's future: finite from the first tile on
      const float corr = expf(m[i] - mt);
      float rs = 0.f;
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const float p = expf(s[n][i] - mt);
        rs += p;
        Ps[(16 * wave + 4 * g + i) * LDV + 16 * n + r] = from_f32<T>(p);
      }
      l[i] = l[i] * corr + row16_sum(rs);
      m[i] = mt;
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c][i] *= corr;
    }
    __builtin_amdgcn_wave_barrier();                     // the strip's P rows are written and read by this wave alone
    for (int c = 0; c < n_ct; ++c) o[c] = Tile<T>::mma(o[c], Ps + 16 * wave * LDV, LDV, Vt + 16 * c * LDV, LDV, TF_KT);
    __builtin_amdgcn_wave_barrier();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int u = w0 + 4 * g + i;
    if (u >= U) continue;
    const float inv = 1.0f / l[i];
    for (int c = 0; c < n_ct; ++c)
      if (16 * c + r < d) ctx[((long)b * U + u) * D + h * d + 16 * c + r] = from_f32<T>(o[c][i] * inv);
  }
}

// ---- (b) head energies of every (target, source) pair ---------------------------------------------------------------------------
// q [B][U][D] (projected; scaled by head_dim^-0.5 here), K [B][H][S_cap][d] -> out [B H][U][S] fp32.
// soft: raw energies of all S keys, no padding fill (expected_soft_attention masks by itself).
// monotonic: the keys are pooled as the PADDED batch is (train mode: ceil(S / ratio) windows over all S rows, no floor trim; mean and
// the affine key projection commute), energy + bias, -1e8 on pooled positions j > 0 whose window holds more than pad_thr padding,
// sigmoid, then zero insertion: pooled j lands on source frame (j + 1) ratio - 1 and column S - 1 takes the last pooled value
// (modules/fixed_pre_decision.py:143-159; ratio 1: the identity).  A workgroup owns TF_KT pooled positions and writes every source
// column of their windows, zeros included.
template <typename T>
__global__ __launch_bounds__(256) void mma_energy_kernel(const T* __restrict__ q, const T* __restrict__ K, float* __restrict__ out,
                                                         const int* __restrict__ key_len, int U, int S, int S_cap, int H, int d,
                                                         int ratio, int monotonic, float scale, float bias, float pad_thr) {
  constexpr int LDQ = TF_DMAX + Tile<T>::PAD, LDE = TF_KT + 1;
  __shared__ __attribute__((aligned(16))) T Qs[TF_ROWS * LDQ];
  __shared__ __attribute__((aligned(16))) T Ks[TF_KT * LDQ];
  __shared__ float Es[TF_ROWS * LDE];
  const bool pool_last = ratio < 0;                      // sign of ratio = pooling type (common.h)
  ratio = ratio < 0 ? -ratio : ratio;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int j0 = blockIdx.x * TF_KT, u0 = blockIdx.y * TF_ROWS, bh = blockIdx.z;
  const int b = bh / H, h = bh - b * H, D = H * d, dp = (d + 31) & ~31;
  const int P = pooled_count(S, ratio, false, pool_last);
  const int len = key_len ? key_len[b] : S;
  stage_rows<T>(Qs, LDQ, q + (long)b * U * D + h * d, D, u0, TF_ROWS, U, d, dp, 1.0f);      // as given: the fp32 energies are scaled (see (a))
  const T* Kh = K + (long)bh * S_cap * d;
  for (int idx = threadIdx.x; idx < TF_KT * dp; idx += 256) {
    const int kj = idx / dp, c = idx - kj * dp;
    const int j = j0 + kj;
    float v = 0.f;
    if (j < P && c < d) {
      int f0, f1;
      pooled_frames(j, S, ratio, pool_last, f0, f1);
      float acc = 0.f;
      for (int f = f0; f < f1; ++f) acc += to_f32(Kh[(long)f * d + c]);
      v = acc / (float)(f1 - f0);
    }
    Ks[kj * LDQ + c] = from_f32<T>(v);
  }
  __syncthreads();
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const f32x4 e = Tile<T>::mma(f32x4{0.f, 0.f, 0.f, 0.f}, Qs + 16 * wave * LDQ, LDQ, Ks + 16 * n * LDQ, LDQ, dp);
    const int j = j0 + 16 * n + r;
    bool masked = false;
    if (monotonic && j < P) {
      int f0, f1;
      pooled_frames(j, S, ratio, pool_last, f0, f1);
      masked = policy::window_masked(j, f0, f1, len, pad_thr);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v = e[i] * scale;
      if (monotonic) {
        v = masked ? -1e8f : v + bias;
        v = 1.0f / (1.0f + expf(-v));
      }
      Es[(16 * wave + 4 * g + i) * LDE + 16 * n + r] = v;
    }
  }
  __syncthreads();
  const int s_lo = j0 * ratio, s_hi = min((j0 + TF_KT) * ratio, S);
  const int span = s_hi - s_lo;
  for (int idx = threadIdx.x; idx < TF_ROWS * span; idx += 256) {
    const int row = idx / span, s = s_lo + (idx - row * span);
    const int u = u0 + row;
    if (u >= U) break;
    const int j = policy::pooled_index_at(s, S, ratio, P);
    out[((long)bh * U + u) * S + s] = j >= 0 ? Es[row * LDE + j - j0] : 0.f;
  }
}

// wait-k's whole-target p_choose (utils/p_choose_strategy.py:6-53, online unset): target u is the one-hot of pooled position
// u + k - 1, clipped to the last pooled position the pooled padding mask leaves valid, zero-inserted like the learned policies
__global__ __launch_bounds__(64) void mma_waitk_p_kernel(float* __restrict__ p, const int* __restrict__ key_len, int U, int S, int H,
                                                         int ratio, int k, float pad_thr) {
  const bool pool_last = ratio < 0;
  ratio = ratio < 0 ? -ratio : ratio;
  const int u = blockIdx.x, bh = blockIdx.y;
  const int len = key_len ? key_len[bh / H] : S;
  const int P = pooled_count(S, ratio, false, pool_last);
  int valid = 1;
  for (int j = P - 1; j > 0; --j) {
    int f0, f1;
    pooled_frames(j, S, ratio, pool_last, f0, f1);
    if (!policy::window_masked(j, f0, f1, len, pad_thr)) { valid = j + 1; break; }
  }
  const int step = min(u + k - 1, valid - 1);
  float* row = p + ((long)bh * U + u) * S;
  for (int s = threadIdx.x; s < S; s += 64) {
    const int j = policy::pooled_index_at(s, S, ratio, P);
    row[s] = (j >= 0 && j == step) ? 1.f : 0.f;
  }
}

// softmax over the valid keys of every (head, target) row, in place (full encoder-decoder attention); zeros behind key_len
__global__ __launch_bounds__(256) void mma_softmax_kernel(float* __restrict__ e, const int* __restrict__ key_len, long rows, int U,
                                                          int S, int H) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  float* x = e + r * S;
  const int len = key_len ? min(key_len[(r / U) / H], S) : S;
  float mx = -INFINITY;
  for (int j = lane; j < len; j += 64) mx = fmaxf(mx, x[j]);
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j = lane; j < len; j += 64) sum += expf(x[j] - mx);
  const float inv = 1.0f / wave_sum(sum);
  for (int j = lane; j < S; j += 64) x[j] = j < len ? expf(x[j] - mx) * inv : 0.f;
}

// ---- (c) expected context ---------------------------------------------------------------------------------------------------------
// beta [B H][U][S] fp32 (cast to the activation dtype as it is staged: the reference's beta.to(v.dtype)) times V [B][H][S_cap][d]
// -> ctx [B][U][D], accumulated in fp32
template <typename T>
__global__ __launch_bounds__(256) void mma_context_kernel(const float* __restrict__ beta, const T* __restrict__ V,
                                                          T* __restrict__ ctx, int U, int S, int S_cap, int H, int d) {
  constexpr int LDV = TF_KT + Tile<T>::PAD;
  __shared__ __attribute__((aligned(16))) T Ps[TF_ROWS * LDV];
  __shared__ __attribute__((aligned(16))) T Vt[TF_DMAX * LDV];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int u0 = blockIdx.x * TF_ROWS, bh = blockIdx.y;
  const int b = bh / H, h = bh - b * H, D = H * d, n_ct = (d + 15) >> 4;
  const float* Bh = beta + (long)bh * U * S;
  const T* Vh = V + (long)bh * S_cap * d;
  f32x4 o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < S; k0 += TF_KT) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < TF_ROWS * TF_KT; idx += 256) {
      const int row = idx >> 5, kj = idx & 31;
      const int u = u0 + row, s = k0 + kj;
      Ps[row * LDV + kj] = from_f32<T>((u < U && s < S) ? Bh[(long)u * S + s] : 0.f);
    }
    stage_v_t<T>(Vt, LDV, Vh, d, k0, S, d);
    __syncthreads();
    for (int c = 0; c < n_ct; ++c) o[c] = Tile<T>::mma(o[c], Ps + 16 * wave * LDV, LDV, Vt + 16 * c * LDV, LDV, TF_KT);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int u = u0 + 16 * wave + 4 * g + i;
    if (u >= U) continue;
    for (int c = 0; c < n_ct; ++c)
      if (16 * c + r < d) ctx[((long)b * U + u) * D + h * d + 16 * c + r] = from_f32<T>(o[c][i]);
  }
}

}  // namespace

#define TF_SHAPE_OK(B, U, H, d) ((B) >= 0 && (U) >= 0 && (H) > 0 && (d) > 0 && (d) <= TF_DMAX && (long)(B) * (H) <= 65535 && (U) <= 65535 * TF_ROWS)

extern "C" int simulst_decoder_self_attention_causal(simulst_handle* h, const void* qkv, void* ctx, int32_t B, int32_t U, int32_t H,
                                                     int32_t d, int32_t dtype) {
  if (!h) return SIMULST_E_NULL;
  SL_CHECK_NULL(h, qkv); SL_CHECK_NULL(h, ctx);
  SL_REQUIRE(h, dtype == SIMULST_F32 || dtype == SIMULST_BF16, SIMULST_E_DTYPE, "simulst_decoder_self_attention_causal: dtype");
  SL_REQUIRE(h, TF_SHAPE_OK(B, U, H, d), SIMULST_E_SHAPE, "simulst_decoder_self_attention_causal: shape (head_dim <= 64, B H <= 65535)");
  if (B == 0 || U == 0) return SIMULST_OK;
  KTimer t(h, SIMULST_K_DEC_SELF_ATTN);
  const dim3 grid((U + TF_ROWS - 1) / TF_ROWS, H, B);
  const float scale = 1.0f / sqrtf((float)d);
  if (dtype == SIMULST_F32)
    hipLaunchKernelGGL(causal_self_attn_kernel<float>, grid, dim3(256), 0, h->stream, (const float*)qkv, (float*)ctx, U, H, d, scale);
  else
    hipLaunchKernelGGL(causal_self_attn_kernel<bf16>, grid, dim3(256), 0, h->stream, (const bf16*)qkv, (bf16*)ctx, U, H, d, scale);
  return sl_launch_status(h, "simulst_decoder_self_attention_causal");
}

extern "C" int simulst_mma_energy(simulst_handle* h, const void* q, const void* K, float* out, const int32_t* key_len,
                                  float energy_bias, float pad_threshold, int32_t B, int32_t U, int32_t S, int32_t S_cap, int32_t H,
                                  int32_t d, int32_t ratio, int32_t mode, int32_t waitk_k, int32_t dtype) {
  if (!h) return SIMULST_E_NULL;
  SL_CHECK_NULL(h, out);
  SL_REQUIRE(h, mode == SIMULST_ENERGY_SOFT || mode == SIMULST_ENERGY_MONOTONIC || mode == SIMULST_ENERGY_WAITK, SIMULST_E_ARG,
             "simulst_mma_energy: mode");
  if (mode == SIMULST_ENERGY_WAITK) SL_REQUIRE(h, waitk_k > 0, SIMULST_E_ARG, "simulst_mma_energy: waitk lagging");
  else { SL_CHECK_NULL(h, q); SL_CHECK_NULL(h, K); }
  SL_REQUIRE(h, dtype == SIMULST_F32 || dtype == SIMULST_BF16, SIMULST_E_DTYPE, "simulst_mma_energy: dtype");
  const int ra = ratio < 0 ? -ratio : ratio;
  SL_REQUIRE(h, TF_SHAPE_OK(B, U, H, d) && S > 0 && S <= S_cap && S_cap <= 4096 && ratio != 0 && ra <= 4096 && (ratio > 0 || S >= ra),
             SIMULST_E_SHAPE, "simulst_mma_energy: shape (0 < S <= S_cap <= 4096, head_dim <= 64, B H <= 65535, 'last' pooling: S >= ratio)");
  if (B == 0 || U == 0) return SIMULST_OK;
  KTimer t(h, SIMULST_K_DEC_CROSS_ATTN);
  if (mode == SIMULST_ENERGY_WAITK) {
    hipLaunchKernelGGL(mma_waitk_p_kernel, dim3(U, B * H), dim3(64), 0, h->stream, out, key_len, U, S, H, ratio, waitk_k, pad_threshold);
    return sl_launch_status(h, "simulst_mma_energy(waitk)");
  }
  const int mono = mode == SIMULST_ENERGY_MONOTONIC;
  const int r_eff = mono ? ratio : 1;
  const int P = pooled_count(S, r_eff < 0 ? -r_eff : r_eff, false, r_eff < 0);
  const dim3 grid((P + TF_KT - 1) / TF_KT, (U + TF_ROWS - 1) / TF_ROWS, B * H);
  const float scale = 1.0f / sqrtf((float)d);
  if (dtype == SIMULST_F32)
    hipLaunchKernelGGL(mma_energy_kernel<float>, grid, dim3(256), 0, h->stream, (const float*)q, (const float*)K, out, key_len, U, S,
                       S_cap, H, d, r_eff, mono, scale, energy_bias, pad_threshold);
  else
    hipLaunchKernelGGL(mma_energy_kernel<bf16>, grid, dim3(256), 0, h->stream, (const bf16*)q, (const bf16*)K, out, key_len, U, S,
                       S_cap, H, d, r_eff, mono, scale, energy_bias, pad_threshold);
  return sl_launch_status(h, "simulst_mma_energy");
}

extern "C" int simulst_mma_softmax(simulst_handle* h, float* energy, const int32_t* key_len, int32_t B, int32_t U, int32_t S,
                                   int32_t H) {
  if (!h) return SIMULST_E_NULL;
  SL_CHECK_NULL(h, energy);
  SL_REQUIRE(h, B >= 0 && U >= 0 && S > 0 && H > 0, SIMULST_E_SHAPE, "simulst_mma_softmax: shape");
  const long rows = (long)B * H * U;
  if (rows == 0) return SIMULST_OK;
  KTimer t(h, SIMULST_K_DEC_CROSS_ATTN);
  hipLaunchKernelGGL(mma_softmax_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, h->stream, energy, key_len, rows, U, S, H);
  return sl_launch_status(h, "simulst_mma_softmax");
}

extern "C" int simulst_mma_context(simulst_handle* h, const float* beta, const void* V, void* ctx, int32_t B, int32_t U, int32_t S,
                                   int32_t S_cap, int32_t H, int32_t d, int32_t dtype) {
  if (!h) return SIMULST_E_NULL;
  SL_CHECK_NULL(h, beta); SL_CHECK_NULL(h, V); SL_CHECK_NULL(h, ctx);
  SL_REQUIRE(h, dtype == SIMULST_F32 || dtype == SIMULST_BF16, SIMULST_E_DTYPE, "simulst_mma_context: dtype");
  SL_REQUIRE(h, TF_SHAPE_OK(B, U, H, d) && S > 0 && S <= S_cap, SIMULST_E_SHAPE,
             "simulst_mma_context: shape (0 < S <= S_cap, head_dim <= 64, B H <= 65535)");
  if (B == 0 || U == 0) return SIMULST_OK;
  KTimer t(h, SIMULST_K_DEC_CROSS_ATTN);
  const dim3 grid((U + TF_ROWS - 1) / TF_ROWS, B * H);
  if (dtype == SIMULST_F32)
    hipLaunchKernelGGL(mma_context_kernel<float>, grid, dim3(256), 0, h->stream, beta, (const float*)V, (float*)ctx, U, S, S_cap, H, d);
  else
    hipLaunchKernelGGL(mma_context_kernel<bf16>, grid, dim3(256), 0, h->stream, beta, (const bf16*)V, (bf16*)ctx, U, S, S_cap, H, d);
  return sl_launch_status(h, "simulst_mma_context");
}
