// simulst_linear, SIMULST_EPI_ROW_PICK: per logical row r of z = A . W^T + bias, the lowest column at which z is largest (int32 at C's
// row address) and (max z, logsumexp z) (fp32 pairs at aux[r]) -- the best path of a CTC head and its log-probabilities.  The [M][N]
// logits stay in registers: a row panel of A is staged once in LDS, W streams past it in 16-column tiles, every lane keeps a running
// (max, index, sum of exp(z - max)) for the rows and the column stripe it sees, and one fold per row closes the launch.  Comparison is
// on the fp32 accumulators (+ bias); on equal values the lower column wins at every join, so the pick does not depend on the order in
// which tiles, lanes or waves meet.
//
//   bf16, K % 32 == 0, panel within 60 KB of LDS: v_mfma_f32_16x16x32_bf16, the fragment layout of gemv_mfma.h and the (max, sum)
//     bookkeeping of transducer.hip's joiner_lattice_kernel.  W row-major (a lane's 16 bytes of a fragment are 16 bytes of a row:
//     every 64-byte segment a wave touches is used whole) or fragment-major.
//   everything else (fp32, other K): a thread per column over 4 rows on the VALU, fmaf chains in four partial sums.  Correctness only.
//
// Neither output has room for per-part partials: tall problems give one workgroup the whole width; where the row panels alone would
// leave most of the chip idle (a stream's chunk, a lockstep round) the matrix-core form splits the column tiles over blockIdx.y, the
// parts' (max, sum, index) go to the library's own scratch and a second small launch folds them, in part order.
//
// SIMULST_EPI_ROW_GATHER runs the same kernels (GATHER = true): the same sweep, without the index, gives the row's logsumexp, and a
// gather phase over the SAME staged rows computes z at the caller's labels of the row's batch -- C[row][j] = z[row][lab[b][j]] - lse,
// the log-probabilities a CTC recursion over a given transcript reads.  The gathered z runs the sweep's instruction sequence (same k
// order, same accumulator start), so it is the value the sweep saw for that column.  Labels outside [0, N) are clamped into it.
#include "gemm_plan.h"
#include "gemv_mfma.h"

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

// GATHER: the running state without the index
__device__ __forceinline__ void lse_pair(float& m, float& s, float x0, float x1) {
  const float mx = fmaxf(m, fmaxf(x0, x1));
  s = s * __expf(m - mx) + __expf(x0 - mx) + __expf(x1 - mx);
  m = mx;
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
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        const float om = __shfl_xor(rm[r][e], o, 64), os = __shfl_xor(rs[r][e], o, 64);
        if constexpr (GATHER) {
          lse_join(rm[r][e], rs[r][e], om, os);
        } else {
          const int oi = __shfl_xor(ri[r][e], o, 64);
          pick_join(rm[r][e], ri[r][e], rs[r][e], om, oi, os);
        }
      }
      const int row = 16 * r + 4 * lg + e;
      if (col == 0) {
        red_m[wave][row] = rm[r][e]; red_s[wave][row] = rs[r][e];
        if constexpr (!GATHER) red_i[wave][row] = ri[r][e];
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
      float m = red_m[0][tid], s = red_s[0][tid];
#pragma unroll
      for (int w = 1; w < 4; ++w) lse_join(m, s, red_m[w][tid], red_s[w][tid]);
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
        const bf16* w0 = W + (long)lb * p.K + lg * G;
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        uint4 wa = ld16(w0);
        for (int ks = 0; ks < nks; ++ks) {
          const uint4 ca = wa;
          if (ks + 1 < nks) wa = ld16(w0 + (ks + 1) * KS);
          const uint4 a = *reinterpret_cast<const uint4*>(zs + (long)(16 * r + col) * ldz + ks * KS + lg * G);
          acc = lat_mma<bf16>(a, ca, acc);
        }
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
template <typename T> __device__ __forceinline__ void load_g(const T* p, float (&o)[gemv::MF<T>::G]);
template <> __device__ __forceinline__ void load_g<float>(const float* p, float (&o)[4]) { load4(p, o); }
template <> __device__ __forceinline__ void load_g<bf16>(const bf16* p, float (&o)[8]) {
  float t[4];
  load4(p, t); o[0] = t[0]; o[1] = t[1]; o[2] = t[2]; o[3] = t[3];
  load4(p + 4, t); o[4] = t[0]; o[5] = t[1]; o[6] = t[2]; o[7] = t[3];
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
#pragma unroll
  for (int r = 0; r < PICK_VM; ++r) {
    const int row = min(m0 + r, p.M - 1);                   // rows past the end repeat the last one and are not stored
    const int b = row / p.rpb, ii = row - b * p.rpb;
    arow[r] = A + (long)b * p.a_bs + (long)ii * p.a_rs;
  }
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

}  // namespace

int sl_launch_row_pick(simulst_handle* h, const sl_linear_plan& pl, const sl_linear_ops& o, const LinArgs& p) {
  float4* part = nullptr;
  if (pl.splits > 1) {                                       // the library's own scratch, as simulst_linear's split-K partials
    const size_t need = (size_t)pl.splits * p.M * sizeof(float4);
    if (h->ws_bytes < need) {
      if (h->capturing) { h->err = "simulst_linear: scratch too small while capturing a graph"; return SIMULST_E_ARG; }
      if (h->ws) (void)hipFree(h->ws);
      h->ws = nullptr; h->ws_bytes = 0;
      hipError_t e = hipMalloc(&h->ws, need);
      if (e != hipSuccess) { h->err = "simulst_linear: scratch allocation failed"; return (int)e; }
      h->ws_bytes = need;
    }
    part = (float4*)h->ws;
  }
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
