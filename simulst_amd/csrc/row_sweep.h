// The column sweep of the kernels that reduce a vocabulary row on chip.  A panel of activation rows sits in LDS with row stride
// K + G (16 bytes of padding: the 16 rows of a fragment start on different banks); W streams past it in 16-column tiles, two per
// pass, the next k-step's fragments in flight; 4 waves stride the tiles, every lane keeps a running (max, sum exp) per row and column
// stripe; a 16-lane fold and a 4-wave join close it.  gemm_pick.hip's row_topk_mfma_kernel runs sweep_columns; row_pick_mfma_kernel
// and transducer.hip's joiner_lattice_kernel keep a copy of that pass loop each (through the helper they measured slower) and take
// every other piece from here.  tests/test_hip_row_sweep.py holds the copies to one another bit for bit.
#pragma once
#include "gemv_mfma.h"

// one 16 x 16 tile step: a = 16 bytes of an activation row (lane's row lane % 16, k-group lane / 16), w = the weight fragment
template <typename T> __device__ __forceinline__ f32x4 lat_mma(const uint4& a, const uint4& w, f32x4 acc) {
  if constexpr (std::is_same<T, float>::value) {
    const float* af = reinterpret_cast<const float*>(&a);
    const float* wf = reinterpret_cast<const float*>(&w);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[e], wf[e], acc, 0, 0, 0);
    return acc;
  } else {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8_t*>(&a), *reinterpret_cast<const bf16x8_t*>(&w),
                                                   acc, 0, 0, 0);
  }
}

constexpr float LAT_NEG = -1e30f;         // "no column yet": finite, so that max - max never makes a NaN

// (m, s) <- (m, s) joined with (om, os): s counts exp(x - m)
__device__ __forceinline__ void lse_join(float& m, float& s, float om, float os) {
  const float mx = fmaxf(m, om);
  s = s * __expf(m - mx) + os * __expf(om - mx);
  m = mx;
}

// the running (max, sum) of one row after the two columns of a pass
__device__ __forceinline__ void lse_pair(float& m, float& s, float x0, float x1) {
  const float mx = fmaxf(m, fmaxf(x0, x1));
  s = s * __expf(m - mx) + __expf(x0 - mx) + __expf(x1 - mx);
  m = mx;
}

// 16 bytes of a row as floats
template <typename T> __device__ __forceinline__ void load_g(const T* p, float (&o)[gemv::MF<T>::G]);
template <> __device__ __forceinline__ void load_g<float>(const float* p, float (&o)[4]) { load4(p, o); }
template <> __device__ __forceinline__ void load_g<bf16>(const bf16* p, float (&o)[8]) {
  float t[4];
  load4(p, t); o[0] = t[0]; o[1] = t[1]; o[2] = t[2]; o[3] = t[3];
  load4(p + 4, t); o[4] = t[0]; o[5] = t[1]; o[6] = t[2]; o[7] = t[3];
}

// rows m0 .. m0 + 16 n_rt - 1 of A (row r of batch r / rpb, any strides) into zs + r * ldz, 16 bytes a thread; zero rows past M
template <typename T>
__device__ __forceinline__ void sweep_stage_rows(T* zs, int ldz, const T* __restrict__ A, const LinArgs& p, int m0, int n_rt, int tid) {
  constexpr int G = gemv::MF<T>::G;
  const int groups = p.K / G;
  for (int i = tid; i < 16 * n_rt * groups; i += 256) {
    const int r = i / groups, c = (i - r * groups) * G, row = m0 + r;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (row < p.M) {
      const int b = row / p.rpb, ii = row - b * p.rpb;
      v = ld16(A + (long)b * p.a_bs + (long)ii * p.a_rs + c);
    }
    *reinterpret_cast<uint4*>(zs + (long)r * ldz + c) = v;
  }
}

// Wave `wave` of 4 takes the column tiles vt0 + 2 wave, + 8, ... of [vt1), two per pass, against the first n_rt of the panel's R row
// tiles.  W is [N][K] row-major or fragment-major (gemv_mfma.h); a masked column reads W's last row instead of one past it.
// consume(c0, ok0, ok1, acc0, acc1), once per pass: the lane (threadIdx.x % 64) holds z[row 16 r + 4 (lane / 16) + e][column c0] in
// acc0[r][e] and column c0 + 16 in acc1[r][e]; ok0 / ok1: the column exists.  Bias, masking and the running state are the caller's.
template <typename T, int R, bool W_FM, typename Consume>
__device__ __forceinline__ void sweep_columns(const T* zs, int ldz, int n_rt, const T* __restrict__ W, int K, int N, int vt0, int vt1,
                                              int wave, Consume consume) {
  constexpr int KS = gemv::MF<T>::KS, G = gemv::MF<T>::G;
  constexpr long step = W_FM ? 64 * G : KS;
  const int lane = threadIdx.x & 63, col = lane & 15, lg = lane >> 4, nks = K / KS;
  for (int vt = vt0 + 2 * wave; vt < vt1; vt += 8) {
    const bool two = vt + 1 < vt1;
    const int c0 = vt * 16 + col, c1 = c0 + 16;
    const bool ok0 = c0 < N, ok1 = two && c1 < N;
    const T *w0, *w1;
    if constexpr (W_FM) {
      w0 = W + ((long)vt * nks * 64 + lane) * G;
      w1 = two ? w0 + (long)nks * 64 * G : w0;
    } else {
      w0 = W + (long)(ok0 ? c0 : N - 1) * K + lg * G;
      w1 = W + (long)(ok1 ? c1 : N - 1) * K + lg * G;
    }
    f32x4 acc0[R], acc1[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { acc0[r] = f32x4{0.f, 0.f, 0.f, 0.f}; acc1[r] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    uint4 wa = ld16(w0), wb = ld16(w1);
    for (int ks = 0; ks < nks; ++ks) {
      const uint4 ca = wa, cb = wb;
      if (ks + 1 < nks) { wa = ld16(w0 + (ks + 1) * step); wb = ld16(w1 + (ks + 1) * step); }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (r >= n_rt) continue;
        const uint4 a = *reinterpret_cast<const uint4*>(zs + (long)(16 * r + col) * ldz + ks * KS + lg * G);
        acc0[r] = lat_mma<T>(a, ca, acc0[r]);
        acc1[r] = lat_mma<T>(a, cb, acc1[r]);
      }
    }
    consume(c0, ok0, ok1, acc0, acc1);
  }
}

// z of row tile `row_tile` at the 16 rows of W that w0 points into: one accumulator of sweep_columns (k order, zero start, prefetch)
template <typename T> __device__ __forceinline__ f32x4 sweep_one_tile(const T* zs, int ldz, int row_tile, const T* __restrict__ w0, int K) {
  constexpr int KS = gemv::MF<T>::KS, G = gemv::MF<T>::G;
  const int lane = threadIdx.x & 63, col = lane & 15, lg = lane >> 4, nks = K / KS;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  uint4 wa = ld16(w0);
  for (int ks = 0; ks < nks; ++ks) {
    const uint4 ca = wa;
    if (ks + 1 < nks) wa = ld16(w0 + (ks + 1) * KS);
    const uint4 a = *reinterpret_cast<const uint4*>(zs + (long)(16 * row_tile + col) * ldz + ks * KS + lg * G);
    acc = lat_mma<T>(a, ca, acc);
  }
  return acc;
}

// the 16 columns of a lane group joined (lane xor 1, 2, 4, 8); rows 4 lg + e of every row tile go to red_*_w, the wave's join row
template <int RW>
__device__ __forceinline__ void fold_lane_group(float (&rm)[RW][4], float (&rs)[RW][4], float* red_m_w, float* red_s_w,
                                                int first_row_tile) {
  const int lane = threadIdx.x & 63, col = lane & 15, lg = lane >> 4;
#pragma unroll
  for (int r = 0; r < RW; ++r)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        const float om = __shfl_xor(rm[r][e], o, 64), os = __shfl_xor(rs[r][e], o, 64);
        lse_join(rm[r][e], rs[r][e], om, os);
      }
      const int row = 16 * (first_row_tile + r) + 4 * lg + e;
      if (col == 0) { red_m_w[row] = rm[r][e]; red_s_w[row] = rs[r][e]; }
    }
}

// ... and the 4 waves of a row, in wave order
template <int ROWS>
__device__ __forceinline__ void join_waves_lse(const float (&red_m)[4][ROWS], const float (&red_s)[4][ROWS], int row, float& m, float& s) {
  m = red_m[0][row]; s = red_s[0][row];
#pragma unroll
  for (int w = 1; w < 4; ++w) lse_join(m, s, red_m[w][row], red_s[w][row]);
}
