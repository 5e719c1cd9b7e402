// Transducer inference (models/transducer_model.py:28-212): average-pool downsample of the encoder states, the joiner's
// per-step scan over the remaining source positions, and the emission.
//
//   simulst_transducer_pool   AvgPool1dTBCPad (:79-98) over [B][S_in][D] rows, with the reference's k / r rescale of a shorter
//                             row's last window
//   simulst_joiner_scan       for every (b, s) with prev_emit[b] <= s < src_len'[b]: the blank logit and the best non-blank
//                             (value, lowest index) of  W_out . tanh(P[b, s] + g[b])  (SimpleJoiner.forward :60-76 with T == 1, and
//                             the argmax of :191) -- the [B][S'][V] logits of the reference are never written
//   simulst_joiner_emit       first scanned position whose best non-blank beats the blank, -1e4 blank at src_len' - 1 (:170-200);
//                             prev_emit <- new_emit, z[b] = tanh(P[b, new_emit] + g[b]), at_eos[b]
//   simulst_joiner_mask_blank logits[b][blank] <- -1e4 where at_eos[b] (the gathered row of :203-206 keeps the scatter of :176-180)
//
// The scan is a [16 R positions] x [V] x [D] contraction per workgroup on the matrix cores: the A operand rows are made on the fly
// (tanh of P + g, rounded to the model dtype) into LDS, the B operand is W_out in fragment-major order (gemv_mfma.h), one 16-byte
// contiguous load per lane and k-step.  No workgroup waits for another one: every part of a vocabulary split writes its own
// (max, index) pair and the emit kernel folds them.
#include "gemv_mfma.h"

namespace {

constexpr int SCAN_THREADS = 256;         // 4 waves, each sweeps every 4th 16-column vocabulary tile of the workgroup's range

template <typename T> struct ScanCfg;
template <> struct ScanCfg<bf16> { static constexpr int R = 4; };     // row tiles (16 positions each) per workgroup
template <> struct ScanCfg<float> { static constexpr int R = 2; };

// the joiner activation; bf16 rows take the exp form (|error| ~1e-7 absolute, far below the bf16 half-ulp of |z| < 1)
template <typename T> __device__ __forceinline__ float join_act(float x);
template <> __device__ __forceinline__ float join_act<float>(float x) { return tanhf(x); }
template <> __device__ __forceinline__ float join_act<bf16>(float x) {
  const float a = fminf(fabsf(x), 15.0f);
  const float e = __expf(2.0f * a);
  const float t = 1.0f - 2.0f / (e + 1.0f);
  return copysignf(t, x);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// (value, index) with torch.argmax's order: the larger value, on a tie the lower index
__device__ __forceinline__ void take_better(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

// ---------------------------------------------------------------------------------------------------------------- pooling
template <typename T>
__global__ void transducer_pool_kernel(const T* __restrict__ x, const int32_t* __restrict__ lengths, T* __restrict__ y,
                                       int32_t* __restrict__ new_len, long x_bs, int S_in, int D, int T_max, int k, int S_out) {
  const int j = blockIdx.x, b = blockIdx.y;
  const int len = clampi(lengths[b], 0, T_max);
  const int n_valid = (len + k - 1) / k;
  if (j == 0 && threadIdx.x == 0) new_len[b] = n_valid;
  const int t0 = j * k;
  const int t1 = min(t0 + k, T_max);                 // the window as avg_pool1d(ceil_mode) clips it to the batch's T
  const int t1v = min(t1, len);                      // rows of it that are not padding (zeroed at :85)
  float scale = 0.0f;
  if (j < n_valid) {
    scale = 1.0f / (float)(t1 - t0);
    if (len < T_max && j == (len - 1) / k) scale *= (float)k / (float)((len - 1) % k + 1);      // :91-97
  }
  T* yo = y + ((long)b * S_out + j) * D;
  const T* xb = x + (long)b * x_bs;
  for (int c = threadIdx.x * 4; c < D; c += blockDim.x * 4) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (j < n_valid) {
      for (int t = t0; t < t1v; ++t) {
        float v[4];
        load4(xb + (long)t * D + c, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += v[e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] *= scale;
    }
    store4(yo + c, acc);
  }
}

// ------------------------------------------------------------------------------------------------------------------- scan
// grid (ceil(B * tiles_per_row / R), n_split).  Row r of the workgroup: tile gt = blockIdx.x * R + r / 16 of the list
// [b][t] (t < tiles_per_row), position s = 16 t + r % 16.
template <typename T>
__global__ __launch_bounds__(SCAN_THREADS) void joiner_scan_kernel(
    const float* __restrict__ P, const float* __restrict__ g, const T* __restrict__ Wp, const int32_t* __restrict__ prev_emit,
    const int32_t* __restrict__ src_len, float* __restrict__ blank_out, float* __restrict__ best_out, int32_t* __restrict__ idx_out,
    int B, int S, int D, int V, int blank, int n_split, int tiles_per_row) {
  constexpr int R = ScanCfg<T>::R, ROWS = 16 * R;
  constexpr int KS = gemv::MF<T>::KS, G = gemv::MF<T>::G;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int ldz = D + G;                                    // 16 bytes of padding per row: the 16 rows of a fragment read
  T* zs = reinterpret_cast<T*>(smem_raw);                   // ... start on different banks
  __shared__ float red_v[4][ROWS];
  __shared__ int red_i[4][ROWS];
  __shared__ int tile_lo[R], tile_hi[R], tile_b[R];         // scanned positions [lo, hi) of each row tile (empty: lo >= hi)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < R) {
    const int gt = blockIdx.x * R + tid;
    int lo = 0, hi = 0, b = 0;
    if (gt < B * tiles_per_row) {
      b = gt / tiles_per_row;
      const int t = gt - b * tiles_per_row;
      const int len = clampi(src_len[b], 0, S);
      const int pe = clampi(prev_emit[b], 0, len > 0 ? len - 1 : 0);
      lo = max(pe, 16 * t);
      hi = min(len, 16 * t + 16);
    }
    tile_lo[tid] = lo; tile_hi[tid] = hi; tile_b[tid] = b;
  }
  __syncthreads();
  bool any = false;
#pragma unroll
  for (int r = 0; r < R; ++r) any |= tile_lo[r] < tile_hi[r];
  if (!any) return;                                         // every row tile lies outside [prev_emit, src_len'): nothing to do

  // A operand: z = tanh(P + g) rounded to T; rows that are not scanned are zero
  const int groups = D / 4;
  for (int i = tid; i < ROWS * groups; i += SCAN_THREADS) {
    const int r = i / groups, c = (i - r * groups) * 4;
    const int rt = r >> 4;
    const int gt = blockIdx.x * R + rt;
    const int s = 16 * (gt % tiles_per_row) + (r & 15);
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if (s >= tile_lo[rt] && s < tile_hi[rt]) {
      const int b = tile_b[rt];
      float pv[4], gv[4];
      load4(P + ((long)b * S + s) * D + c, pv);
      load4(g + (long)b * D + c, gv);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = join_act<T>(pv[e] + gv[e]);
    }
    store4(zs + (long)r * ldz + c, o);
  }
  __syncthreads();

  // this workgroup's vocabulary tiles [vt0, vt1)
  const int n_vt = (V + 15) / 16;
  const int per = (n_vt + n_split - 1) / n_split;
  const int vt0 = blockIdx.y * per, vt1 = min(vt0 + per, n_vt);
  const int nks = D / KS;
  const int col = lane & 15, lg = lane >> 4;

  float bv[R][4];
  int bi[R][4];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int e = 0; e < 4; ++e) { bv[r][e] = -INFINITY; bi[r][e] = 0x7fffffff; }

  for (int vt = vt0 + wave; vt < vt1; vt += 4) {
    f32x4 acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
    const T* wbase = Wp + ((long)vt * nks * 64 + lane) * G;
    for (int ks = 0; ks < nks; ++ks) {
      const uint4 w = ld16(wbase + (long)ks * 64 * G);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (tile_lo[r] >= tile_hi[r]) continue;             // uniform over the workgroup
        const uint4 a = *reinterpret_cast<const uint4*>(zs + (long)(16 * r + col) * ldz + ks * KS + lg * G);
        if constexpr (std::is_same<T, float>::value) {
          const float* af = reinterpret_cast<const float*>(&a);
          const float* wf = reinterpret_cast<const float*>(&w);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[e], wf[e], acc[r], 0, 0, 0);
        } else {
          acc[r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(&a),
                                                           *reinterpret_cast<const bf16x8_t*>(&w), acc[r], 0, 0, 0);
        }
      }
    }
    // lane holds logits[row 4 lg + e][column v] of every row tile
    const int v = vt * 16 + col;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (tile_lo[r] >= tile_hi[r]) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float val = acc[r][e];
        if (v == blank) {
          const int gt = blockIdx.x * R + r;
          const int s = 16 * (gt % tiles_per_row) + 4 * lg + e;
          if (s >= tile_lo[r] && s < tile_hi[r]) blank_out[(long)tile_b[r] * S + s] = val;
        } else if (v < V && val > bv[r][e]) {               // tiles come in rising v: strict > keeps the lowest index
          bv[r][e] = val; bi[r][e] = v;
        }
      }
    }
  }
  // fold the 16 columns of a lane group, then the 4 waves
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        const float ov = __shfl_xor(bv[r][e], o, 64);
        const int oi = __shfl_xor(bi[r][e], o, 64);
        take_better(bv[r][e], bi[r][e], ov, oi);
      }
      if (col == 0) { red_v[wave][16 * r + 4 * lg + e] = bv[r][e]; red_i[wave][16 * r + 4 * lg + e] = bi[r][e]; }
    }
  __syncthreads();
  if (tid < ROWS) {
    const int rt = tid >> 4;
    const int gt = blockIdx.x * R + rt;
    const int s = 16 * (gt % tiles_per_row) + (tid & 15);
    if (s >= tile_lo[rt] && s < tile_hi[rt]) {
      float v = red_v[0][tid];
      int i = red_i[0][tid];
#pragma unroll
      for (int w = 1; w < 4; ++w) take_better(v, i, red_v[w][tid], red_i[w][tid]);
      const long o = ((long)tile_b[rt] * S + s) * n_split + blockIdx.y;
      best_out[o] = v;
      idx_out[o] = i;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------- emit
template <typename T>
__global__ __launch_bounds__(64) void joiner_emit_kernel(const float* __restrict__ P, const float* __restrict__ g,
                                                         const float* __restrict__ blank_in, const float* __restrict__ best_in,
                                                         const int32_t* __restrict__ idx_in, int32_t* __restrict__ prev_emit,
                                                         const int32_t* __restrict__ src_len, T* __restrict__ z,
                                                         int32_t* __restrict__ at_eos, int S, int D, int blank, int n_split) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int len = clampi(src_len[b], 0, S);
  const int last = len > 0 ? len - 1 : 0;
  const int pe = clampi(prev_emit[b], 0, last);
  int first = 0x7fffffff;
  for (int s = pe + lane; s < len; s += 64) {                // bounded by S
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int p = 0; p < n_split; ++p) take_better(bv, bi, best_in[((long)b * S + s) * n_split + p], idx_in[((long)b * S + s) * n_split + p]);
    const float blank_v = s == last ? -1e4f : blank_in[(long)b * S + s];       // force emit at source eos (:170-180)
    if (bv > blank_v || (bv == blank_v && bi < blank)) { first = s; break; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
  const int ne = first <= last ? first : last;
  if (lane == 0) { prev_emit[b] = ne; at_eos[b] = ne == last ? 1 : 0; }
  const float* pr = P + ((long)b * S + ne) * D;
  for (int c = lane * 4; c < D; c += 256) {
    float pv[4], gv[4], o[4];
    load4(pr + c, pv);
    load4(g + (long)b * D + c, gv);
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = join_act<T>(pv[e] + gv[e]);
    store4(z + (long)b * D + c, o);
  }
}

__global__ void joiner_mask_blank_kernel(float* __restrict__ logits, const int32_t* __restrict__ at_eos, int B, int V, int blank) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B && at_eos[b]) logits[(long)b * V + blank] = -1e4f;
}

// the refusals shared by the joiner entry points, made before any pointer is looked at
int joiner_check(simulst_handle* h, const char* who, int B, int S, int D, int V, int blank, int n_split, int dtype) {
  const std::string w(who);
  SL_REQUIRE(h, dtype == SIMULST_F32 || dtype == SIMULST_BF16, SIMULST_E_ARG, w + ": dtype");
  SL_REQUIRE(h, D > 0 && D % 32 == 0, SIMULST_E_ARG, w + ": D % 32");
  SL_REQUIRE(h, V >= 4, SIMULST_E_ARG, w + ": V >= 4");
  SL_REQUIRE(h, S >= 1, SIMULST_E_ARG, w + ": S' >= 1");
  SL_REQUIRE(h, blank >= 0 && blank < V, SIMULST_E_ARG, w + ": blank index");
  SL_REQUIRE(h, n_split >= 1 && n_split <= 64, SIMULST_E_ARG, w + ": n_split in [1, 64]");
  SL_REQUIRE(h, B >= 0, SIMULST_E_ARG, w + ": B");
  return SIMULST_OK;
}

template <typename T> size_t scan_lds_bytes(int D) { return (size_t)16 * ScanCfg<T>::R * (D + gemv::MF<T>::G) * sizeof(T); }

}  // namespace

extern "C" int simulst_transducer_pool(simulst_handle* h, const void* x, const int32_t* lengths, void* y, int32_t* new_len,
                                       int32_t B, int32_t S_in, int32_t D, int64_t x_batch_stride, int32_t T_max, int32_t k,
                                       int32_t dtype) {
  if (!h) return SIMULST_E_NULL;
  SL_REQUIRE(h, dtype == SIMULST_F32 || dtype == SIMULST_BF16, SIMULST_E_ARG, "simulst_transducer_pool: dtype");
  SL_REQUIRE(h, k >= 1, SIMULST_E_ARG, "simulst_transducer_pool: k >= 1");
  SL_REQUIRE(h, T_max >= 1, SIMULST_E_ARG, "simulst_transducer_pool: S' >= 1 (T >= 1)");
  SL_REQUIRE(h, D > 0 && D % 32 == 0, SIMULST_E_ARG, "simulst_transducer_pool: D % 32");
  SL_REQUIRE(h, T_max <= S_in && x_batch_stride >= (int64_t)S_in * D && B >= 0, SIMULST_E_ARG,
             "simulst_transducer_pool: T <= S_in, batch stride >= S_in * D");
  SL_CHECK_NULL(h, x); SL_CHECK_NULL(h, lengths); SL_CHECK_NULL(h, y); SL_CHECK_NULL(h, new_len);
  if (B == 0) return SIMULST_OK;
  const int S_out = (T_max + k - 1) / k;
  KTimer t(h, SIMULST_K_MISC);
  const int threads = D >= 1024 ? 256 : 64;
  if (dtype == SIMULST_F32)
    hipLaunchKernelGGL(transducer_pool_kernel<float>, dim3(S_out, B), dim3(threads), 0, h->stream, (const float*)x, lengths, (float*)y,
                       new_len, (long)x_batch_stride, S_in, D, T_max, k, S_out);
  else
    hipLaunchKernelGGL(transducer_pool_kernel<bf16>, dim3(S_out, B), dim3(threads), 0, h->stream, (const bf16*)x, lengths, (bf16*)y,
                       new_len, (long)x_batch_stride, S_in, D, T_max, k, S_out);
  return sl_launch_status(h, "simulst_transducer_pool");
}

extern "C" int simulst_joiner_scan(simulst_handle* h, const float* P, const float* g, const void* W_fm, const int32_t* prev_emit,
                                   const int32_t* src_len, float* blank_logit, float* best, int32_t* best_idx, int32_t B, int32_t S,
                                   int32_t D, int32_t V, int32_t blank, int32_t n_split, int32_t dtype) {
  if (!h) return SIMULST_E_NULL;
  const int rc = joiner_check(h, "simulst_joiner_scan", B, S, D, V, blank, n_split, dtype);
  if (rc != SIMULST_OK) return rc;
  const size_t lds = dtype == SIMULST_F32 ? scan_lds_bytes<float>(D) : scan_lds_bytes<bf16>(D);
  SL_REQUIRE(h, lds <= 48 * 1024, SIMULST_E_SHAPE, "simulst_joiner_scan: D too large for the row tiles in LDS");
  SL_CHECK_NULL(h, P); SL_CHECK_NULL(h, g); SL_CHECK_NULL(h, W_fm); SL_CHECK_NULL(h, prev_emit); SL_CHECK_NULL(h, src_len);
  SL_CHECK_NULL(h, blank_logit); SL_CHECK_NULL(h, best); SL_CHECK_NULL(h, best_idx);
  if (B == 0) return SIMULST_OK;
  const int tiles_per_row = (S + 15) / 16;
  KTimer t(h, SIMULST_K_SCAN);
  if (dtype == SIMULST_F32) {
    const int Rr = ScanCfg<float>::R;
    hipLaunchKernelGGL(joiner_scan_kernel<float>, dim3((B * tiles_per_row + Rr - 1) / Rr, n_split), dim3(SCAN_THREADS), lds, h->stream,
                       P, g, (const float*)W_fm, prev_emit, src_len, blank_logit, best, best_idx, B, S, D, V, blank, n_split,
                       tiles_per_row);
  } else {
    const int Rr = ScanCfg<bf16>::R;
    hipLaunchKernelGGL(joiner_scan_kernel<bf16>, dim3((B * tiles_per_row + Rr - 1) / Rr, n_split), dim3(SCAN_THREADS), lds, h->stream,
                       P, g, (const bf16*)W_fm, prev_emit, src_len, blank_logit, best, best_idx, B, S, D, V, blank, n_split,
                       tiles_per_row);
  }
  return sl_launch_status(h, "simulst_joiner_scan");
}

extern "C" int simulst_joiner_emit(simulst_handle* h, const float* P, const float* g, const float* blank_logit, const float* best,
                                   const int32_t* best_idx, int32_t* prev_emit, const int32_t* src_len, void* z, int32_t* at_eos,
                                   int32_t B, int32_t S, int32_t D, int32_t V, int32_t blank, int32_t n_split, int32_t dtype) {
  if (!h) return SIMULST_E_NULL;
  const int rc = joiner_check(h, "simulst_joiner_emit", B, S, D, V, blank, n_split, dtype);
  if (rc != SIMULST_OK) return rc;
  SL_CHECK_NULL(h, P); SL_CHECK_NULL(h, g); SL_CHECK_NULL(h, blank_logit); SL_CHECK_NULL(h, best); SL_CHECK_NULL(h, best_idx);
  SL_CHECK_NULL(h, prev_emit); SL_CHECK_NULL(h, src_len); SL_CHECK_NULL(h, z); SL_CHECK_NULL(h, at_eos);
  if (B == 0) return SIMULST_OK;
  KTimer t(h, SIMULST_K_SCAN);
  if (dtype == SIMULST_F32)
    hipLaunchKernelGGL(joiner_emit_kernel<float>, dim3(B), dim3(64), 0, h->stream, P, g, blank_logit, best, best_idx, prev_emit,
                       src_len, (float*)z, at_eos, S, D, blank, n_split);
  else
    hipLaunchKernelGGL(joiner_emit_kernel<bf16>, dim3(B), dim3(64), 0, h->stream, P, g, blank_logit, best, best_idx, prev_emit,
                       src_len, (bf16*)z, at_eos, S, D, blank, n_split);
  return sl_launch_status(h, "simulst_joiner_emit");
}

extern "C" int simulst_joiner_mask_blank(simulst_handle* h, float* logits, const int32_t* at_eos, int32_t B, int32_t V,
                                         int32_t blank) {
  if (!h) return SIMULST_E_NULL;
  SL_REQUIRE(h, V >= 4 && blank >= 0 && blank < V && B >= 0, SIMULST_E_ARG, "simulst_joiner_mask_blank: V >= 4, blank in [0, V)");
  SL_CHECK_NULL(h, logits); SL_CHECK_NULL(h, at_eos);
  if (B == 0) return SIMULST_OK;
  KTimer t(h, SIMULST_K_MISC);
  hipLaunchKernelGGL(joiner_mask_blank_kernel, dim3((B + 63) / 64), dim3(64), 0, h->stream, logits, at_eos, B, V, blank);
  return sl_launch_status(h, "simulst_joiner_mask_blank");
}
