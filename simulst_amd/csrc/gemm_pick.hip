// simulst_linear, SIMULST_EPI_ROW_PICK: per logical row r of z = A . W^T + bias, the lowest column at which z is largest (int32 at C's
// row address) and (max z, logsumexp z) (fp32 pairs at aux[r]) -- the best path of a CTC head and its log-probabilities.  The [M][N]
// logits stay in registers: a row panel of A is staged once in LDS, W streams past it in 16-column tiles (the column sweep of
// row_sweep.h), every lane keeps a running (max, index, sum of exp(z - max)) for the rows and the column stripe it sees, and one fold
// per row closes the launch.  Comparison is on the fp32 accumulators (+ bias); on equal values the lower column wins at every join,
// so the pick does not depend on the order in which tiles, lanes or waves meet.
//
//   bf16, K % 32 == 0, panel within 60 KB of LDS: v_mfma_f32_16x16x32_bf16, the fragment layout of gemv_mfma.h and the (max, sum)
//     bookkeeping of row_sweep.h.  W row-major (a lane's 16 bytes of a fragment are 16 bytes of a row: every 64-byte segment a wave
//     touches is used whole) or fragment-major.
//   everything else (fp32, other K): a thread per column over 4 rows on the VALU, fmaf chains in four partial sums.  Correctness only.
//
// Neither output has room for per-part partials: tall problems give one workgroup the whole width; where the row panels alone would
// leave most of the chip idle (a stream's chunk, a lockstep round) the matrix-core form splits the column tiles over blockIdx.y, the
// parts' (max, sum, index) go to the library's own scratch and a second small launch folds them, in part order.
//
// SIMULST_EPI_ROW_GATHER runs the same kernels (GATHER = true): the same sweep, without the index, gives the row's logsumexp, and a
// gather phase over the SAME staged rows computes z at the caller's labels of the row's batch -- C[row][j] = z[row][lab[b][j]] - lse,
// the log-probabilities a CTC recursion over a given transcript reads.  The gathered z is sweep_one_tile's, one accumulator of the
// sweep, so it is the value the sweep saw for that column.  Labels outside [0, N) are clamped into it.
//
// SIMULST_EPI_ROW_TOPK has kernels of its own further down (row_topk_*): the same sweep (sweep_columns) and the same plan, with
// per-row candidate lists in place of the single running index (tests/test_hip_row_sweep.py: the three agree bit for bit).
#include "gemm_plan.h"
#include "row_sweep.h"

namespace {

constexpr int PICK_NONE = 0x7fffffff;          // index of "no column yet": loses every tie

// (m, i, s) <- joined with (om, oi, os): larger value, on equal values the lower index; s counts exp(z - m)
__device__ __forceinline__ void pick_join(float& m, int& i, float& s, float om, int oi, float os) {
  const bool take = om > m || (om == m && oi < i);
  i = take ? oi : i;
  lse_join(m, s, om, os);
}

// the running state of one row after column c with value x (columns arrive in ascending order: strict > keeps the lowest)
__device__ __forceinline__ void pick_pair(float& m, int& i, float& s, float x0, int c0, float x1, int c1) {
  const float mx = fmaxf(m, fmaxf(x0, x1));
  s = s * __expf(m - mx) + __expf(x0 - mx) + __expf(x1 - mx);
  i = x0 > m ? c0 : i;
  i = x1 > fmaxf(m, x0) ? c1 : i;
  m = mx;
}

__device__ __forceinline__ void pick_store(const LinArgs& p, int32_t* __restrict__ C, float* __restrict__ aux, int row, float m, int i,
                                           float s) {
  const int b = row / p.rpb, ii = row - b * p.rpb;
  C[(long)b * p.c_bs + (long)ii * p.c_rs] = i;
  *reinterpret_cast<float2*>(aux + 2 * (long)row) = make_float2(m, m + logf(s));
}

// label j of batch b, clamped into [0, N); j past the list reads W's row 0
__device__ __forceinline__ int gather_label(const LinArgs& p, const int32_t* __restrict__ lab, int b, int j) {
  return j < p.aux_rows ? min(max(lab[(long)b * p.aux_bs + j], 0), p.N - 1) : 0;
}

// ---- matrix cores: PICK_M rows per workgroup, 4 waves, each sweeping every row tile over its own column tiles (two per pass) -------------
// part != nullptr: gridDim.y column parts, part[row * gridDim.y + blockIdx.y] = (max, sum, index bits, -) instead of the outputs
// GATHER: C is fp32 [row][aux_rows] and aux the int32 labels [batch][aux_rows] (an input); with parts the gather phase writes raw z and
// the fold launch subtracts the folded logsumexp
template <bool W_FM, bool GATHER>
__global__ __launch_bounds__(256) void row_pick_mfma_kernel(const bf16* __restrict__ A, const bf16* __restrict__ W,
                                                            const float* __restrict__ bias, void* __restrict__ Cv,
                                                            void* __restrict__ auxv, float4* __restrict__ part, LinArgs p) {
  constexpr int KS = gemv::MF<bf16>::KS, G = gemv::MF<bf16>::G, R = PICK_M / 16;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  bf16* zs = reinterpret_cast<bf16*>(smem_raw);
  __shared__ float red_m[4][PICK_M], red_s[4][PICK_M];
  __shared__ int red_i[4][PICK_M];
  const int ldz = p.K + G;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * PICK_M;
  const int n_rt = min(R, (p.M - m0 + 15) >> 4);           // row tiles with a row in them

  sweep_stage_rows<bf16>(zs, ldz, A, p, m0, n_rt, tid);
  __syncthreads();

  const int n_vt = (p.N + 15) >> 4, nks = p.K / KS;
  const int per = (n_vt + (int)gridDim.y - 1) / (int)gridDim.y;
  const int vt0 = blockIdx.y * per, vt1 = min(vt0 + per, n_vt);
  const int col = lane & 15, lg = lane >> 4;
  float rm[R][4], rs[R][4];
  int ri[R][4];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int e = 0; e < 4; ++e) { rm[r][e] = LAT_NEG; rs[r][e] = 0.f; ri[r][e] = PICK_NONE; }

  // sweep_columns (row_sweep.h) as a loop of its own: through the helper tools/ctc_pick_bench.py's 64 x 250 rows took 0.142, not 0.139 ms
  for (int vt = vt0 + 2 * wave; vt < vt1; vt += 8) {
    const bool two = vt + 1 < vt1;
    const int c0 = vt * 16 + col, c1 = c0 + 16;
    const bool ok0 = c0 < p.N, ok1 = two && c1 < p.N;
    // a masked column reads the last row of W instead of one past it
    const bf16 *w0, *w1;
    long step;
    if constexpr (W_FM) {
      w0 = W + ((long)vt * nks * 64 + lane) * G;
      w1 = two ? w0 + (long)nks * 64 * G : w0;
      step = 64 * G;
    } else {
      w0 = W + (long)(ok0 ? c0 : p.N - 1) * p.K + lg * G;
      w1 = W + (long)(ok1 ? c1 : p.N - 1) * p.K + lg * G;
      step = KS;
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
        if (r >= n_rt) continue;                            // uniform over the workgroup
        const uint4 a = *reinterpret_cast<const uint4*>(zs + (long)(16 * r + col) * ldz + ks * KS + lg * G);
        acc0[r] = lat_mma<bf16>(a, ca, acc0[r]);
        acc1[r] = lat_mma<bf16>(a, cb, acc1[r]);
      }
    }
    const float b0 = (bias && ok0) ? bias[c0] : 0.f, b1 = (bias && ok1) ? bias[c1] : 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
        const float x0 = ok0 ? acc0[r][e] + b0 : -INFINITY, x1 = ok1 ? acc1[r][e] + b1 : -INFINITY;
        if constexpr (GATHER) lse_pair(rm[r][e], rs[r][e], x0, x1);
        else pick_pair(rm[r][e], ri[r][e], rs[r][e], x0, c0, x1, c1);
      }
  }
  // fold the 16 columns of a lane group, then the 4 waves
  if constexpr (GATHER) {
    fold_lane_group<R>(rm, rs, red_m[wave], red_s[wave], 0);
  } else {                                                   // fold_lane_group with the index
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          const float om = __shfl_xor(rm[r][e], o, 64), os = __shfl_xor(rs[r][e], o, 64);
          const int oi = __shfl_xor(ri[r][e], o, 64);
          pick_join(rm[r][e], ri[r][e], rs[r][e], om, oi, os);
        }
        const int row = 16 * r + 4 * lg + e;
        if (col == 0) { red_m[wave][row] = rm[r][e]; red_s[wave][row] = rs[r][e]; red_i[wave][row] = ri[r][e]; }
      }
  }
  __syncthreads();
  if constexpr (!GATHER) {
    int32_t* C = static_cast<int32_t*>(Cv);
    float* aux = static_cast<float*>(auxv);
    if (tid < PICK_M && m0 + tid < p.M) {
      float m = red_m[0][tid], s = red_s[0][tid];
      int i = red_i[0][tid];
#pragma unroll
      for (int w = 1; w < 4; ++w) pick_join(m, i, s, red_m[w][tid], red_i[w][tid], red_s[w][tid]);
      if (part) part[(long)(m0 + tid) * gridDim.y + blockIdx.y] = make_float4(m, s, __int_as_float(i), 0.f);
      else pick_store(p, C, aux, m0 + tid, m, i, s);
    }
  } else {
    float* C = static_cast<float*>(Cv);
    const int32_t* lab = static_cast<const int32_t*>(auxv);
    float my_lse = 0.f;
    if (tid < PICK_M && m0 + tid < p.M) {
      float m, s;
      join_waves_lse(red_m, red_s, tid, m, s);
      if (part) part[(long)(m0 + tid) * gridDim.y + blockIdx.y] = make_float4(m, s, 0.f, 0.f);
      else my_lse = m + logf(s);
    }
    if (tid < PICK_M) red_m[0][tid] = my_lse;                // (column tid is this thread's alone) the rows' logsumexp; 0 with parts
    __syncthreads();
    // gather phase: unit (label tile jt, row tile r) over the waves of every part; a row tile takes the label list of each batch it
    // has rows of in turn, and a row stores what its own batch's list gave
    const int n_jt = (p.aux_rows + 15) >> 4;
    const int workers = 4 * (int)gridDim.y;
    for (int u = (int)blockIdx.y * 4 + wave; u < n_jt * n_rt; u += workers) {
      const int jt = u / n_rt, r = u - jt * n_rt;
      const int j = jt * 16 + col;
      const int row_lo = m0 + 16 * r, row_hi = min(row_lo + 15, p.M - 1);
      const int b_lo = row_lo / p.rpb, b_hi = row_hi / p.rpb;
      for (int bb = b_lo; bb <= b_hi; ++bb) {
        const int lb = gather_label(p, lab, bb, j);
        const f32x4 acc = sweep_one_tile<bf16>(zs, ldz, r, W + (long)lb * p.K + lg * G, p.K);
        const float bv = bias ? bias[lb] : 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int lr = 16 * r + 4 * lg + e, row = m0 + lr;
          if (row >= p.M || j >= p.aux_rows) continue;
          const int b = row / p.rpb, ii = row - b * p.rpb;
          if (b != bb) continue;
          C[(long)b * p.c_bs + (long)ii * p.c_rs + j] = (acc[e] + bv) - red_m[0][lr];
        }
      }
    }
  }
}

// one thread per row: the column parts joined in part order
__global__ void row_pick_fold_kernel(const float4* __restrict__ part, int n_split, int32_t* __restrict__ C, float* __restrict__ aux,
                                     LinArgs p) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= p.M) return;
  float m = LAT_NEG, s = 0.f;
  int i = PICK_NONE;
  for (int q = 0; q < n_split; ++q) {
    const float4 v = part[(long)row * n_split + q];
    pick_join(m, i, s, v.x, __float_as_int(v.z), v.y);
  }
  pick_store(p, C, aux, row, m, i, s);
}

// GATHER: 16 lanes per row: each joins the parts in part order, then takes every 16th of the row's raw z and subtracts the logsumexp
__global__ void row_gather_fold_kernel(const float4* __restrict__ part, int n_split, float* __restrict__ C, LinArgs p) {
  const int row = blockIdx.x * (blockDim.x >> 4) + (threadIdx.x >> 4), l = threadIdx.x & 15;
  if (row >= p.M) return;
  float m = LAT_NEG, s = 0.f;
  for (int q = 0; q < n_split; ++q) {
    const float4 v = part[(long)row * n_split + q];
    lse_join(m, s, v.x, v.y);
  }
  const float lse = m + logf(s);
  const int b = row / p.rpb, ii = row - b * p.rpb;
  float* c = C + (long)b * p.c_bs + (long)ii * p.c_rs;
  for (int j = l; j < p.aux_rows; j += 16) c[j] -= lse;
}

// ---- VALU: PICK_VM rows per workgroup, thread t takes columns t, t + 256, ... -------------------------------------------------------------
// the PICK_VM rows of a workgroup: rows past the end repeat the last one and are not stored
template <typename T> __device__ __forceinline__ void valu_rows(const T* __restrict__ A, const LinArgs& p, int m0, const T* (&arow)[PICK_VM]) {
#pragma unroll
  for (int r = 0; r < PICK_VM; ++r) {
    const int row = min(m0 + r, p.M - 1);
    const int b = row / p.rpb, ii = row - b * p.rpb;
    arow[r] = A + (long)b * p.a_bs + (long)ii * p.a_rs;
  }
}

// z of PICK_VM rows at one column: the fmaf chains of the sweep and of the gather phase
template <typename T>
__device__ __forceinline__ void valu_column(const T* const (&arow)[PICK_VM], const T* __restrict__ wrow, int K, float bv,
                                            float (&x)[PICK_VM]) {
  constexpr int G = gemv::MF<T>::G;
  float part[PICK_VM][4];
#pragma unroll
  for (int r = 0; r < PICK_VM; ++r)
#pragma unroll
    for (int e = 0; e < 4; ++e) part[r][e] = 0.f;
  for (int k = 0; k < K; k += G) {
    float wv[G];
    load_g<T>(wrow + k, wv);
#pragma unroll
    for (int r = 0; r < PICK_VM; ++r) {
      float av[G];
      load_g<T>(arow[r] + k, av);
#pragma unroll
      for (int e = 0; e < G; ++e) part[r][e & 3] = fmaf(av[e], wv[e], part[r][e & 3]);
    }
  }
#pragma unroll
  for (int r = 0; r < PICK_VM; ++r) x[r] = ((part[r][0] + part[r][1]) + (part[r][2] + part[r][3])) + bv;
}

template <typename T, bool GATHER>
__global__ __launch_bounds__(256) void row_pick_valu_kernel(const T* __restrict__ A, const T* __restrict__ W,
                                                            const float* __restrict__ bias, void* __restrict__ Cv,
                                                            void* __restrict__ auxv, LinArgs p) {
  __shared__ float red_m[4][PICK_VM], red_s[4][PICK_VM];
  __shared__ int red_i[4][PICK_VM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * PICK_VM;
  const T* arow[PICK_VM];
  valu_rows<T>(A, p, m0, arow);
  float rm[PICK_VM], rs[PICK_VM];
  int ri[PICK_VM];
#pragma unroll
  for (int r = 0; r < PICK_VM; ++r) { rm[r] = LAT_NEG; rs[r] = 0.f; ri[r] = PICK_NONE; }
  for (int c = tid; c < p.N; c += 256) {
    float x[PICK_VM];
    valu_column<T>(arow, W + (long)c * p.K, p.K, bias ? bias[c] : 0.f, x);
#pragma unroll
    for (int r = 0; r < PICK_VM; ++r) pick_pair(rm[r], ri[r], rs[r], x[r], c, -INFINITY, c);
  }
#pragma unroll
  for (int r = 0; r < PICK_VM; ++r) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float om = __shfl_xor(rm[r], o, 64), os = __shfl_xor(rs[r], o, 64);
      const int oi = __shfl_xor(ri[r], o, 64);
      pick_join(rm[r], ri[r], rs[r], om, oi, os);
    }
    if (lane == 0) { red_m[wave][r] = rm[r]; red_s[wave][r] = rs[r]; red_i[wave][r] = ri[r]; }
  }
  __syncthreads();
  float m = LAT_NEG, s = 0.f;
  int i = PICK_NONE;
  if (tid < PICK_VM) {
    m = red_m[0][tid]; s = red_s[0][tid]; i = red_i[0][tid];
#pragma unroll
    for (int w = 1; w < 4; ++w) pick_join(m, i, s, red_m[w][tid], red_i[w][tid], red_s[w][tid]);
  }
  if constexpr (!GATHER) {
    if (tid < PICK_VM && m0 + tid < p.M) pick_store(p, static_cast<int32_t*>(Cv), static_cast<float*>(auxv), m0 + tid, m, i, s);
  } else {
    float* C = static_cast<float*>(Cv);
    const int32_t* lab = static_cast<const int32_t*>(auxv);
    __syncthreads();
    if (tid < PICK_VM) red_m[0][tid] = m + logf(s);
    __syncthreads();
    // gather phase: thread t takes labels t, t + 256, ... of each batch the workgroup has rows of
    const int row_hi = min(m0 + PICK_VM - 1, p.M - 1);
    for (int bb = m0 / p.rpb; bb <= row_hi / p.rpb; ++bb)
      for (int j = tid; j < p.aux_rows; j += 256) {
        const int lb = gather_label(p, lab, bb, j);
        float x[PICK_VM];
        valu_column<T>(arow, W + (long)lb * p.K, p.K, bias ? bias[lb] : 0.f, x);
#pragma unroll
        for (int r = 0; r < PICK_VM; ++r) {
          const int row = m0 + r;
          if (row >= p.M) continue;
          const int b = row / p.rpb, ii = row - b * p.rpb;
          if (b == bb) C[(long)b * p.c_bs + (long)ii * p.c_rs + j] = x[r] - red_m[0][r];
        }
      }
  }
}

// ---- SIMULST_EPI_ROW_TOPK: the best k columns of a row (value descending, on equal values the lower column first) ------------------------
// A candidate is ONE 64-bit key: the order-preserving integer image of its fp32 z in the high word, ~column in the low one.  A larger
// key is a better candidate, keys of different columns differ, so every selection below is a total order and its result does not depend
// on the order in which tiles, lanes, waves or column parts meet.  0 is "no candidate" (below the key of every real value).
//   sweep: the pick's (same k order, same accumulator start), with the running (max, sum) of the gather form.  Every row has a bound
//     thr[row] -- the key of the k-th best candidate some wave has seen so far, never above the true k-th -- and each WAVE its own
//     candidate list cand[wave][row][TOPK_CAP]: a column at or above the bound is appended (one compare per element in the common case,
//     about k ln(N / k) appends a row); a full list is reduced to its best k by rank (16 lanes a row, every lane counts the entries
//     that beat its own), which raises the bound.  The lists are the wave's own: no barrier inside the sweep.
//   close: every list is reduced to its best k, then 32 lanes a row rank the 4 x k survivors and store the row (or its part record).
typedef unsigned long long topk_key;
constexpr int TOPK_MAX = PICK_TOPK_MAX, TOPK_CAP = PICK_TOPK_CAP;
constexpr int TOPK_REC = PICK_TOPK_REC_BYTES / 4;           // floats of a part record: (max, sum, z at keep, -) and TOPK_MAX keys
static_assert(TOPK_REC * 4 == 16 + TOPK_MAX * 8, "part record");

__device__ __forceinline__ topk_key topk_make(float x, int c) {
  x = x == 0.f ? 0.f : x;                                   // (-0 and +0 are one value)
  const int b = __float_as_int(x);
  const unsigned hi = (unsigned)(b ^ ((b >> 31) & 0x7fffffff)) ^ 0x80000000u;
  return ((topk_key)hi << 32) | (unsigned)~c;
}
__device__ __forceinline__ int topk_col(topk_key v) { return v ? (int)~(unsigned)v : -1; }
__device__ __forceinline__ float topk_val(topk_key v) {
  const int k = (int)((unsigned)(v >> 32) ^ 0x80000000u);
  return v ? __int_as_float(k ^ ((k >> 31) & 0x7fffffff)) : -INFINITY;
}
__device__ __forceinline__ topk_key topk_shfl_xor(topk_key v, int o) {
  const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
  return ((topk_key)hi << 32) | lo;
}

// one row's k' ids at C, its k' log-probabilities and its logsumexp at aux: slot j of the k non-keep columns
__device__ __forceinline__ void topk_store_slot(const LinArgs& p, int32_t* __restrict__ C, float* __restrict__ aux, int row, int j,
                                                topk_key v, float lse) {
  const int b = row / p.rpb, ii = row - b * p.rpb, kb = p.n_main >= 0, kp = p.aux_rows + kb;
  C[(long)b * p.c_bs + (long)ii * p.c_rs + kb + j] = topk_col(v);
  aux[(long)row * (kp + 1) + kb + j] = topk_val(v) - lse;
}
__device__ __forceinline__ void topk_store_row(const LinArgs& p, int32_t* __restrict__ C, float* __restrict__ aux, int row, float zkeep,
                                               float lse) {
  const int b = row / p.rpb, ii = row - b * p.rpb, kb = p.n_main >= 0, kp = p.aux_rows + kb;
  if (kb) {
    C[(long)b * p.c_bs + (long)ii * p.c_rs] = p.n_main;
    aux[(long)row * (kp + 1)] = zkeep - lse;
  }
  aux[(long)row * (kp + 1) + kp] = lse;
}

// a wave's lists reduced to their best k, sorted: the full ones (all = false) or every one.  16 lanes a row, 4 rows a step.
__device__ __noinline__ void topk_compact(volatile topk_key* cand_w, volatile int* cnt_w, topk_key* thr, int k, bool all, int lane) {
  const int g = lane >> 4, i = lane & 15;
  for (int step = 0; step < PICK_M / 4; ++step) {
    const int row = step * 4 + g;
    const int n_raw = cnt_w[row];
    const bool act = all || n_raw >= TOPK_CAP;
    if (!__any(act)) continue;                              // (uniform over the wave)
    const int n = min(n_raw, TOPK_CAP);
    topk_key my = 0;
    int rank = 0;
    if (act) {
      my = i < n ? cand_w[row * TOPK_CAP + i] : 0;
#pragma unroll
      for (int j = 0; j < TOPK_CAP; ++j) {
        const topk_key o = cand_w[row * TOPK_CAP + j];
        rank += (j < n && o > my) ? 1 : 0;
      }
    }
    __threadfence_block();                                  // every lane has read the list before one writes into it
    if (act && i < n && rank < k) {
      cand_w[row * TOPK_CAP + rank] = my;
      if (rank == k - 1) atomicMax(&thr[row], my);
    }
    if (act && i == 0) cnt_w[row] = min(n, k);
    __threadfence_block();
  }
}

template <bool W_FM>
__global__ __launch_bounds__(256, 2) void row_topk_mfma_kernel(const bf16* __restrict__ A, const bf16* __restrict__ W,
                                                            const float* __restrict__ bias, int32_t* __restrict__ C,
                                                            float* __restrict__ aux, float* __restrict__ part, LinArgs p) {
  constexpr int G = gemv::MF<bf16>::G, R = PICK_M / 16;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  bf16* zs = reinterpret_cast<bf16*>(smem_raw);
  __shared__ float red_m[4][PICK_M], red_s[4][PICK_M], zkeep[PICK_M];
  __shared__ int cnt[4][PICK_M];
  __shared__ topk_key thr[PICK_M];
  const int ldz = p.K + G;
  topk_key* cand = reinterpret_cast<topk_key*>(smem_raw + (size_t)PICK_M * ldz * sizeof(bf16));     // [4][PICK_M][TOPK_CAP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * PICK_M;
  const int n_rt = min(R, (p.M - m0 + 15) >> 4);
  const int k = p.aux_rows, keep = p.n_main;
  topk_key* cand_w = cand + (size_t)wave * PICK_M * TOPK_CAP;

  cnt[wave][lane] = 0;
  if (tid < PICK_M) { thr[tid] = 0; zkeep[tid] = -INFINITY; }
  sweep_stage_rows<bf16>(zs, ldz, A, p, m0, n_rt, tid);
  __syncthreads();

  const int n_vt = (p.N + 15) >> 4;
  const int per = (n_vt + (int)gridDim.y - 1) / (int)gridDim.y;
  const int vt0 = blockIdx.y * per, vt1 = min(vt0 + per, n_vt);
  const int lg = lane >> 4;
  float rm[R][4], rs[R][4];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int e = 0; e < 4; ++e) { rm[r][e] = LAT_NEG; rs[r][e] = 0.f; }

  sweep_columns<bf16, R, W_FM>(zs, ldz, n_rt, W, p.K, p.N, vt0, vt1, wave, [&](int c0, bool ok0, bool ok1, const f32x4(&acc0)[R],
                                                                               const f32x4(&acc1)[R]) {
    const int c1 = c0 + 16;
    const float b0 = (bias && ok0) ? bias[c0] : 0.f, b1 = (bias && ok1) ? bias[c1] : 0.f;
    const bool in0 = ok0 && c0 != keep, in1 = ok1 && c1 != keep;
    unsigned pend = 0;                                      // bit 2 (4 r + e) + j: column cj of row 16 r + 4 lg + e waits for a slot
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int lr = 16 * r + 4 * lg + e;
        const float x0 = ok0 ? acc0[r][e] + b0 : -INFINITY, x1 = ok1 ? acc1[r][e] + b1 : -INFINITY;
        lse_pair(rm[r][e], rs[r][e], x0, x1);
        if (ok0 && c0 == keep) zkeep[lr] = x0;
        if (ok1 && c1 == keep) zkeep[lr] = x1;
        const topk_key t = __hip_atomic_load(&thr[lr], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);     // (one 8-byte read)
        if (r >= n_rt) continue;                            // (a row tile without rows collects nothing)
        if (in0 && topk_make(x0, c0) >= t) pend |= 1u << (2 * (4 * r + e));
        if (in1 && topk_make(x1, c1) >= t) pend |= 2u << (2 * (4 * r + e));
      }
    while (__any(pend != 0)) {
      unsigned fail = 0;
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int lr = 16 * r + 4 * lg + e;
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const unsigned bit = (1u << j) << (2 * (4 * r + e));
            if (!(pend & bit)) continue;
            const topk_key v = j ? topk_make(acc1[r][e] + b1, c1) : topk_make(acc0[r][e] + b0, c0);
            if (v < __hip_atomic_load(&thr[lr], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) continue;                // the bound has passed it meanwhile
            const int slot = atomicAdd(&cnt[wave][lr], 1);
            if (slot < TOPK_CAP) cand_w[lr * TOPK_CAP + slot] = v;
            else fail |= bit;
          }
        }
      pend = fail;
      __threadfence_block();
      if (__any(fail != 0)) topk_compact(cand_w, cnt[wave], thr, k, false, lane);
    }
  });
  __threadfence_block();
  topk_compact(cand_w, cnt[wave], thr, k, true, lane);
  fold_lane_group<R>(rm, rs, red_m[wave], red_s[wave], 0);      // the 16 columns of a lane group; the 4 waves meet below
  __syncthreads();
  // 32 lanes a row: lane j holds entry j & 7 of wave j >> 3 and counts the survivors that beat it
  const int half = lane >> 5, j = lane & 31, jw = j >> 3, ji = j & 7;
  for (int step = 0; step < PICK_M / 8; ++step) {
    const int lr = wave * (PICK_M / 4) + step * 2 + half, row = m0 + lr;
    if (row >= p.M) continue;
    const topk_key my = ji < cnt[jw][lr] ? cand[((size_t)jw * PICK_M + lr) * TOPK_CAP + ji] : 0;
    int rank = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int n = cnt[w][lr];
      total += n;
#pragma unroll
      for (int i = 0; i < TOPK_MAX; ++i) {
        const topk_key o = cand[((size_t)w * PICK_M + lr) * TOPK_CAP + i];
        rank += (i < n && o > my) ? 1 : 0;
      }
    }
    total = min(total, k);
    float m, s;
    join_waves_lse(red_m, red_s, lr, m, s);
    if (part) {
      float* rec = part + ((long)row * gridDim.y + blockIdx.y) * TOPK_REC;
      topk_key* keys = reinterpret_cast<topk_key*>(rec + 4);
      if (my && rank < k) keys[rank] = my;
      if (j < TOPK_MAX && j >= total) keys[j] = 0;
      if (j == 0) *reinterpret_cast<float4*>(rec) = make_float4(m, s, zkeep[lr], 0.f);
    } else {
      const float lse = m + logf(s);
      if (my && rank < k) topk_store_slot(p, C, aux, row, rank, my, lse);
      if (j < k && j >= total) topk_store_slot(p, C, aux, row, j, 0, lse);
      if (j == 0) topk_store_row(p, C, aux, row, zkeep[lr], lse);
    }
  }
}

// a wave per row: the (max, sum) of the parts joined in part order, then k rounds of "the best key below the last one"
__global__ __launch_bounds__(256) void row_topk_fold_kernel(const float* __restrict__ part, int n_split, int32_t* __restrict__ C,
                                                            float* __restrict__ aux, LinArgs p) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= p.M) return;
  const float* rec0 = part + (long)row * n_split * TOPK_REC;
  float m = LAT_NEG, s = 0.f, zk = -INFINITY;
  for (int q = 0; q < n_split; ++q) {
    const float4 v = *reinterpret_cast<const float4*>(rec0 + (long)q * TOPK_REC);
    lse_join(m, s, v.x, v.y);
    zk = fmaxf(zk, v.z);
  }
  const float lse = m + logf(s);
  topk_key prev = ~0ull;
  for (int r = 0; r < p.aux_rows; ++r) {
    topk_key best = 0;
    for (int c = lane; c < n_split * TOPK_MAX; c += 64) {
      const topk_key v = reinterpret_cast<const topk_key*>(rec0 + (long)(c / TOPK_MAX) * TOPK_REC + 4)[c % TOPK_MAX];
      if (v < prev && v > best) best = v;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const topk_key ov = topk_shfl_xor(best, o);
      best = ov > best ? ov : best;
    }
    if (lane == 0) topk_store_slot(p, C, aux, row, r, best, lse);
    prev = best;
  }
  if (lane == 0) topk_store_row(p, C, aux, row, zk, lse);
}

// VALU: the pick's sweep once per rank -- round r takes, per row, the best key below round r - 1's.  Correctness only.
template <typename T>
__global__ __launch_bounds__(256) void row_topk_valu_kernel(const T* __restrict__ A, const T* __restrict__ W,
                                                            const float* __restrict__ bias, int32_t* __restrict__ C,
                                                            float* __restrict__ aux, LinArgs p) {
  __shared__ float red_m[4][PICK_VM], red_s[4][PICK_VM], zkeep[PICK_VM], lse_s[PICK_VM];
  __shared__ topk_key red_k[4][PICK_VM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * PICK_VM;
  const T* arow[PICK_VM];
  valu_rows<T>(A, p, m0, arow);
  if (tid < PICK_VM) zkeep[tid] = -INFINITY;
  __syncthreads();
  topk_key prev[PICK_VM];
#pragma unroll
  for (int r = 0; r < PICK_VM; ++r) prev[r] = ~0ull;
  for (int round = 0; round < p.aux_rows; ++round) {
    float rm[PICK_VM], rs[PICK_VM];
    topk_key best[PICK_VM];
#pragma unroll
    for (int r = 0; r < PICK_VM; ++r) { rm[r] = LAT_NEG; rs[r] = 0.f; best[r] = 0; }
    for (int c = tid; c < p.N; c += 256) {
      float x[PICK_VM];
      valu_column<T>(arow, W + (long)c * p.K, p.K, bias ? bias[c] : 0.f, x);
#pragma unroll
      for (int r = 0; r < PICK_VM; ++r) {
        if (round == 0) {
          lse_pair(rm[r], rs[r], x[r], -INFINITY);
          if (c == p.n_main) zkeep[r] = x[r];
        }
        const topk_key v = topk_make(x[r], c);
        if (c != p.n_main && v < prev[r] && v > best[r]) best[r] = v;
      }
    }
#pragma unroll
    for (int r = 0; r < PICK_VM; ++r) {
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const topk_key ov = topk_shfl_xor(best[r], o);
        best[r] = ov > best[r] ? ov : best[r];
        if (round == 0) {
          const float om = __shfl_xor(rm[r], o, 64), os = __shfl_xor(rs[r], o, 64);
          lse_join(rm[r], rs[r], om, os);
        }
      }
      if (lane == 0) { red_k[wave][r] = best[r]; if (round == 0) { red_m[wave][r] = rm[r]; red_s[wave][r] = rs[r]; } }
    }
    __syncthreads();
    if (round == 0 && tid < PICK_VM) {
      float m = red_m[0][tid], s = red_s[0][tid];
#pragma unroll
      for (int w = 1; w < 4; ++w) lse_join(m, s, red_m[w][tid], red_s[w][tid]);
      lse_s[tid] = m + logf(s);
    }
#pragma unroll
    for (int r = 0; r < PICK_VM; ++r) {
      topk_key b = red_k[0][r];
#pragma unroll
      for (int w = 1; w < 4; ++w) b = red_k[w][r] > b ? red_k[w][r] : b;
      prev[r] = b;
    }
    __syncthreads();
    if (tid < PICK_VM && m0 + tid < p.M) {
      topk_key mine = prev[0];
#pragma unroll
      for (int r = 1; r < PICK_VM; ++r) mine = tid == r ? prev[r] : mine;
      topk_store_slot(p, C, aux, m0 + tid, round, mine, lse_s[tid]);
      if (round == 0) topk_store_row(p, C, aux, m0 + tid, zkeep[tid], lse_s[tid]);
    }
  }
}

}  // namespace

static int sl_launch_row_topk(simulst_handle* h, const sl_linear_plan& pl, const sl_linear_ops& o, const LinArgs& p, float* part) {
  // panel + lists pass the default dynamic-LDS limit from K = 224 on
  static const sl_lds_limit limits[] = {{(const void*)row_topk_mfma_kernel<false>, 100 * 1024}, {(const void*)row_topk_mfma_kernel<true>, 100 * 1024}};
  const dim3 grid(pl.grid[0], pl.grid[1]), block(256);
  int32_t* C = (int32_t*)o.C;
  float* aux = (float*)o.aux;
  if (pl.pick_mfma) {
    if (int rc = sl_raise_lds(h, SL_LDS_ROW_TOPK, limits, "simulst_linear (row top-k)")) return rc;
    KTimer t(h, pl.timer);
    const bf16 *A = (const bf16*)o.A, *W = (const bf16*)o.W;
    if (p.w_packed) hipLaunchKernelGGL((row_topk_mfma_kernel<true>), grid, block, pl.lds, h->stream, A, W, o.bias, C, aux, part, p);
    else hipLaunchKernelGGL((row_topk_mfma_kernel<false>), grid, block, pl.lds, h->stream, A, W, o.bias, C, aux, part, p);
    if (part) hipLaunchKernelGGL(row_topk_fold_kernel, dim3((p.M + 3) / 4), block, 0, h->stream, part, pl.splits, C, aux, p);
  } else {
    KTimer t(h, pl.timer);
    if (pl.dtype == SIMULST_F32)
      hipLaunchKernelGGL((row_topk_valu_kernel<float>), grid, block, 0, h->stream, (const float*)o.A, (const float*)o.W, o.bias, C, aux, p);
    else
      hipLaunchKernelGGL((row_topk_valu_kernel<bf16>), grid, block, 0, h->stream, (const bf16*)o.A, (const bf16*)o.W, o.bias, C, aux, p);
  }
  return sl_launch_status(h, "simulst_linear (row top-k)");
}

int sl_launch_row_pick(simulst_handle* h, const sl_linear_plan& pl, const sl_linear_ops& o, const LinArgs& p) {
  float4* part = nullptr;
  if (pl.splits > 1) {                                       // the library's own scratch, as simulst_linear's split-K partials
    const bool topk = pl.epi == SIMULST_EPI_ROW_TOPK;
    const size_t need = (size_t)pl.splits * p.M * (topk ? TOPK_REC * sizeof(float) : sizeof(float4));
    if (int rc = sl_workspace(h, need, 0, "simulst_linear")) return rc;
    part = (float4*)h->ws;
  }
  if (pl.epi == SIMULST_EPI_ROW_TOPK) return sl_launch_row_topk(h, pl, o, p, (float*)part);
  KTimer t(h, pl.timer);
  const dim3 grid(pl.grid[0], pl.grid[1]), block(256);
  const bool gather = pl.epi == SIMULST_EPI_ROW_GATHER;
  const char* what = gather ? "simulst_linear (row gather)" : "simulst_linear (row pick)";
  if (pl.pick_mfma) {
    const bf16 *A = (const bf16*)o.A, *W = (const bf16*)o.W;
    if (gather)                                              // (the plan refused fragment-major weights)
      hipLaunchKernelGGL((row_pick_mfma_kernel<false, true>), grid, block, pl.lds, h->stream, A, W, o.bias, o.C, o.aux, part, p);
    else if (p.w_packed)
      hipLaunchKernelGGL((row_pick_mfma_kernel<true, false>), grid, block, pl.lds, h->stream, A, W, o.bias, o.C, o.aux, part, p);
    else
      hipLaunchKernelGGL((row_pick_mfma_kernel<false, false>), grid, block, pl.lds, h->stream, A, W, o.bias, o.C, o.aux, part, p);
    if (part && gather)
      hipLaunchKernelGGL(row_gather_fold_kernel, dim3((p.M + 15) / 16), block, 0, h->stream, part, pl.splits, (float*)o.C, p);
    else if (part)
      hipLaunchKernelGGL(row_pick_fold_kernel, dim3((p.M + 255) / 256), block, 0, h->stream, part, pl.splits, (int32_t*)o.C,
                         (float*)o.aux, p);
  } else if (pl.dtype == SIMULST_F32) {
    const float *A = (const float*)o.A, *W = (const float*)o.W;
    if (gather) hipLaunchKernelGGL((row_pick_valu_kernel<float, true>), grid, block, 0, h->stream, A, W, o.bias, o.C, o.aux, p);
    else hipLaunchKernelGGL((row_pick_valu_kernel<float, false>), grid, block, 0, h->stream, A, W, o.bias, o.C, o.aux, p);
  } else {
    const bf16 *A = (const bf16*)o.A, *W = (const bf16*)o.W;
    if (gather) hipLaunchKernelGGL((row_pick_valu_kernel<bf16, true>), grid, block, 0, h->stream, A, W, o.bias, o.C, o.aux, p);
    else hipLaunchKernelGGL((row_pick_valu_kernel<bf16, false>), grid, block, 0, h->stream, A, W, o.bias, o.C, o.aux, p);
  }
  return sl_launch_status(h, what);
}
