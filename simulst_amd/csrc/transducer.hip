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
//   simulst_joiner_mask_blank logits[b][blank] <- -1e4 where at_eos[b] > 0 (the gathered row of :203-206 keeps the scatter of :176-180)
//   an OPEN source (simultaneous decoding): src_len[b] = -1 - a < 0 says that a pooled positions are available and more may follow;
//                             the scan covers [prev_emit, a), no position is forced, and a row in which no scanned position emits
//                             WAITS: prev_emit and z stay, at_eos[b] = -1 (include/simulst_hip.h)
//   simulst_joiner_scan_beam / simulst_joiner_emit_beam   the same two kernels over R beam rows of which every `group` consecutive
//                             ones share one source (P and src_len are read at r / group, never replicated); the rows of a finished
//                             sentence scan nothing
//   simulst_transducer_beam_reorder   beam search's state reorder: a row's self-attention K/V prefix and its prev_emit from its
//                             parent row into the second buffer set (the role reorder_incremental_state has at :241-251), on
//                             beam.hip's beam_reorder_kernel
//   simulst_joiner_lattice    the joiner over a whole target (:143-163 with no incremental state): log p(blank) and log p(label) of
//                             every (s, u) cell, an online log-sum-exp over vocabulary tiles -- the [B][S'][U + 1][V] logits that
//                             criterion/rnnt_criterion.py:90-92 normalises are never written
//   simulst_rnnt_forward      the forward recursion over that lattice (warp_rnnt's log-likelihood, :112-122) and, on request, the
//                             best single alignment with the frame each label is emitted at
//
// The scan is a [16 R positions] x [V] x [D] contraction per workgroup on the matrix cores: the A operand rows are made on the fly
// (tanh of P + g, rounded to the model dtype) into LDS, the B operand is W_out in fragment-major order (gemv_mfma.h), one 16-byte
// contiguous load per lane and k-step.  No workgroup waits for another one: every part of a vocabulary split writes its own
// (max, index) pair and the emit kernel folds them.
#include "row_sweep.h"

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

// src_len of the scan / emit kernels: sl >= 0 a closed source of sl pooled positions; sl < 0 an OPEN source (more may follow) of
// which -1 - sl positions are available so far.  Either way clamped to the buffer's S.
__device__ __forceinline__ int open_len(int sl, int S) { return clampi(sl < 0 ? -1 - sl : sl, 0, S); }

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
// [b][t] (t < tiles_per_row), position s = 16 t + r % 16.  B counts rows; row b reads the source b / group (P, src_len, finished)
// and its own g, prev_emit and outputs.  The tiles of a finished source are empty.
template <typename T>
__global__ __launch_bounds__(SCAN_THREADS) void joiner_scan_kernel(
    const float* __restrict__ P, const float* __restrict__ g, const T* __restrict__ Wp, const int32_t* __restrict__ prev_emit,
    const int32_t* __restrict__ src_len, const int32_t* __restrict__ finished, float* __restrict__ blank_out,
    float* __restrict__ best_out, int32_t* __restrict__ idx_out, int B, int group, int S, int D, int V, int blank, int n_split,
    int tiles_per_row) {
  constexpr int R = ScanCfg<T>::R, ROWS = 16 * R;
  constexpr int KS = gemv::MF<T>::KS, G = gemv::MF<T>::G;
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int ldz = D + G;                                    // 16 bytes of padding per row: the 16 rows of a fragment read
  T* zs = reinterpret_cast<T*>(smem_raw);                   // ... start on different banks
  __shared__ float red_v[4][ROWS];
  __shared__ int red_i[4][ROWS];
  __shared__ int tile_lo[R], tile_hi[R], tile_b[R];         // scanned positions [lo, hi) of each row tile (empty: lo >= hi)
  __shared__ int tile_src[R];                               // the source the tile's row reads P from

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < R) {
    const int gt = blockIdx.x * R + tid;
    int lo = 0, hi = 0, b = 0, src = 0;
    if (gt < B * tiles_per_row) {
      b = gt / tiles_per_row;
      const int t = gt - b * tiles_per_row;
      src = b / group;
      if (!(finished && finished[src])) {
        const int sl = src_len[src];
        const int len = open_len(sl, S);
        const int pe = clampi(prev_emit[b], 0, sl < 0 ? len : (len > 0 ? len - 1 : 0));    // an open row may have nothing left to scan
        lo = max(pe, 16 * t);
        hi = min(len, 16 * t + 16);
      }
    }
    tile_lo[tid] = lo; tile_hi[tid] = hi; tile_b[tid] = b; tile_src[tid] = src;
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
      load4(P + ((long)tile_src[rt] * S + s) * D + c, pv);
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
        acc[r] = lat_mma<T>(a, w, acc[r]);
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
                                                         const int32_t* __restrict__ src_len, const int32_t* __restrict__ finished,
                                                         T* __restrict__ z, int32_t* __restrict__ at_eos,
                                                         int32_t* __restrict__ emit_log, int group, int S, int D, int blank,
                                                         int n_split) {
  const int b = blockIdx.x, lane = threadIdx.x, src = b / group;     // row b of source b / group
  if (finished && finished[src]) return;                             // uniform over the workgroup: the row keeps prev_emit, z, at_eos
  const int sl = src_len[src];
  const bool open = sl < 0;                                  // no position is the source's last one yet: nothing is forced
  const int len = open_len(sl, S);
  const int last = len > 0 ? len - 1 : 0;
  const int pe = clampi(prev_emit[b], 0, open ? len : last);
  int first = 0x7fffffff;
  for (int s = pe + lane; s < len; s += 64) {                // bounded by S
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int p = 0; p < n_split; ++p) take_better(bv, bi, best_in[((long)b * S + s) * n_split + p], idx_in[((long)b * S + s) * n_split + p]);
    const float blank_v = (s == last && !open) ? -1e4f : blank_in[(long)b * S + s];      // force emit at source eos (:170-180)
    if (bv > blank_v || (bv == blank_v && bi < blank)) { first = s; break; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
  if (open && first == 0x7fffffff) {                         // uniform over the workgroup: the row waits for more source and
    if (lane == 0) {                                         // ... keeps prev_emit and z
      at_eos[b] = -1;
      if (emit_log) emit_log[b] = -1;
    }
    return;
  }
  const int ne = first <= last ? first : last;
  if (lane == 0) {
    prev_emit[b] = ne;
    at_eos[b] = (ne == last && !open) ? 1 : 0;
    if (emit_log) emit_log[b] = ne;
  }
  const float* pr = P + ((long)src * S + ne) * D;
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
  if (b < B && at_eos[b] > 0) logits[(long)b * V + blank] = -1e4f;
}

// ---------------------------------------------------------------------------------------------------------------- lattice
// The whole-target joiner: rows are the cells (b, s, u).  A row tile is one (b, s) with 16 consecutive u; the list of tiles is
// [b][s][ut] (ut < u_tiles) and a workgroup takes R consecutive ones as its LDS panel, 16 R rows of tanh(P[b][s] + G[b][u]).
// The panel is tall (128 rows bf16, 64 rows fp32: about 66 KB at D = 256, two workgroups per compute unit) so that W_out is read
// from L2 once per 128 rows (by each of a bf16 workgroup's two row groups), and every A fragment read from LDS feeds two
// vocabulary tiles (2 MFMAs per ds_read_b128: one read per MFMA would need the LDS array's whole 256 B/clk).  Each lane keeps a running (max, sum) of its own column stripe per row;
// the 16 columns and the 4 waves fold at the end.  The blank and label logits are plain dot products of the same panel (2 of the
// V columns per row), taken by the vocabulary part that holds the column.
template <typename T> struct LatCfg;
// R row tiles per workgroup in THREADS / 256 row groups, each swept by 4 waves that split the vocabulary.  bf16: two groups of 4 tiles
// (8 waves, 4 per SIMD with two workgroups per compute unit) measured 0.78 ms against 0.90 ms for one group of 8 tiles on 4 waves and
// 0.95 ms for 6 tiles on 4 waves with three workgroups per compute unit (the bench shape of tools/transducer_score_bench.py)
template <> struct LatCfg<bf16> { static constexpr int R = 8, THREADS = 512; };
template <> struct LatCfg<float> { static constexpr int R = 4, THREADS = 256; };

// (everything but the pass loop is row_sweep.h's; the loop is a copy of its sweep_columns over the RW row tiles of a row group: through
//  the helper this kernel measured 0.82 ms against 0.76 / 0.77 ms on the shape of tools/transducer_score_bench.py)

// grid (ceil(B * S * u_tiles / R), n_split).  part[cell][p] = (max, sum, blank logit, label logit) of vocabulary part p.
template <typename T>
__global__ __launch_bounds__(LatCfg<T>::THREADS, LatCfg<T>::THREADS / 128) void joiner_lattice_kernel(
    const float* __restrict__ P, const float* __restrict__ Gt, const T* __restrict__ Wp, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ src_len, const int32_t* __restrict__ tgt_len, float* __restrict__ part, int B, int S, int U1, int D,
    int V, int blank, int n_split, int u_tiles) {
  constexpr int R = LatCfg<T>::R, ROWS = 16 * R, THREADS = LatCfg<T>::THREADS;
  constexpr int RW = R / (THREADS / 256);                   // row tiles of one wave
  constexpr int KS = gemv::MF<T>::KS, G = gemv::MF<T>::G;
  static_assert(R % (THREADS / 256) == 0 && ROWS <= 256, "row groups");
  extern __shared__ __align__(16) unsigned char smem_raw[];
  const int ldz = D + G;
  T* zs = reinterpret_cast<T*>(smem_raw);
  __shared__ float red_m[4][ROWS], red_s[4][ROWS];
  __shared__ float cap[ROWS][2];                            // blank / label logit of the row (LAT_NEG: not in this part)
  __shared__ int row_lab[ROWS];                             // label column of the row, -1: none
  __shared__ int tile_b[R], tile_s[R], tile_u0[R], tile_n[R];      // rows u0 .. u0 + n - 1 of (b, s) are valid cells (n == 0: none)

  const int tid = threadIdx.x, lane = tid & 63, wave = (tid >> 6) & 3, rbase = (tid >> 8) * RW;
  const long n_tiles = (long)B * S * u_tiles;
  if (tid < R) {
    const long gt = (long)blockIdx.x * R + tid;
    int b = 0, s = 0, u0 = 0, n = 0;
    if (gt < n_tiles) {
      b = (int)(gt / ((long)S * u_tiles));
      const int rem = (int)(gt - (long)b * S * u_tiles);
      s = rem / u_tiles;
      u0 = 16 * (rem - s * u_tiles);
      const int sl = clampi(src_len[b], 0, S), tl = clampi(tgt_len[b], 0, U1 - 1);
      if (s < sl) n = clampi(tl + 1 - u0, 0, 16);
    }
    tile_b[tid] = b; tile_s[tid] = s; tile_u0[tid] = u0; tile_n[tid] = n;
  }
  __syncthreads();
  bool any = false;
#pragma unroll
  for (int r = 0; r < R; ++r) any |= tile_n[r] > 0;
  if (!any) return;                                         // every row tile lies outside the valid cells

  if (tid < ROWS) {
    const int rt = tid >> 4, i = tid & 15;
    int lab = -1;
    if (i < tile_n[rt]) {
      const int b = tile_b[rt], u = tile_u0[rt] + i;
      if (u < clampi(tgt_len[b], 0, U1 - 1)) lab = clampi(labels[(long)b * U1 + u], 0, V - 1);
    }
    row_lab[tid] = lab;
    cap[tid][0] = LAT_NEG; cap[tid][1] = LAT_NEG;
  }
  const int groups = D / 4;
  for (int i = tid; i < ROWS * groups; i += THREADS) {
    const int r = i / groups, c = (i - r * groups) * 4;
    const int rt = r >> 4;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if ((r & 15) < tile_n[rt]) {
      const int b = tile_b[rt];
      float pv[4], gv[4];
      load4(P + ((long)b * S + tile_s[rt]) * D + c, pv);
      load4(Gt + ((long)b * U1 + tile_u0[rt] + (r & 15)) * D + c, gv);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = join_act<T>(pv[e] + gv[e]);
    }
    store4(zs + (long)r * ldz + c, o);
  }
  __syncthreads();

  const int n_vt = (V + 15) / 16;
  const int per = (n_vt + n_split - 1) / n_split;
  const int vt0 = blockIdx.y * per, vt1 = min(vt0 + per, n_vt);
  const int nks = D / KS;
  const int col = lane & 15, lg = lane >> 4;

  float rm[RW][4], rs[RW][4];
#pragma unroll
  for (int r = 0; r < RW; ++r)
#pragma unroll
    for (int e = 0; e < 4; ++e) { rm[r][e] = LAT_NEG; rs[r][e] = 0.f; }

  // two vocabulary tiles per pass; the weight fragments of the next k-step are loaded while this one's MFMAs run
  for (int vt = vt0 + 2 * wave; vt < vt1; vt += 8) {
    const bool two = vt + 1 < vt1;
    f32x4 acc0[RW], acc1[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) { acc0[r] = f32x4{0.f, 0.f, 0.f, 0.f}; acc1[r] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    const T* w0 = Wp + ((long)vt * nks * 64 + lane) * G;
    const T* w1 = two ? w0 + (long)nks * 64 * G : w0;
    uint4 wa = ld16(w0), wb = ld16(w1);
    for (int ks = 0; ks < nks; ++ks) {
      const uint4 ca = wa, cb = wb;
      if (ks + 1 < nks) { wa = ld16(w0 + (long)(ks + 1) * 64 * G); wb = ld16(w1 + (long)(ks + 1) * 64 * G); }
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        if (tile_n[rbase + r] == 0) continue;               // uniform over the wave
        const uint4 a = *reinterpret_cast<const uint4*>(zs + (long)(16 * (rbase + r) + col) * ldz + ks * KS + lg * G);
        acc0[r] = lat_mma<T>(a, ca, acc0[r]);
        acc1[r] = lat_mma<T>(a, cb, acc1[r]);
      }
    }
    const bool ok0 = vt * 16 + col < V, ok1 = two && (vt + 1) * 16 + col < V;
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
      for (int e = 0; e < 4; ++e) lse_pair(rm[r][e], rs[r][e], ok0 ? acc0[r][e] : -INFINITY, ok1 ? acc1[r][e] : -INFINITY);
  }
  // fold the 16 columns of a lane group, then (below) the 4 waves of the row group
  fold_lane_group<RW>(rm, rs, red_m[wave], red_s[wave], rbase);
  // the blank and label logits of every row: thread (row, which) takes one dot product over D if this part holds the column
  for (int i = tid; i < 2 * ROWS; i += THREADS) {
    const int r = i >> 1, which = i & 1;
    const int c = which ? row_lab[r] : ((r & 15) < tile_n[r >> 4] ? blank : -1);
    if (c < 0 || (c >> 4) < vt0 || (c >> 4) >= vt1) continue;
    const T* wrow = Wp + ((long)(c >> 4) * nks * 64 + (c & 15)) * G;
    const T* zrow = zs + (long)r * ldz;
    float acc = 0.f;
    for (int ks = 0; ks < nks; ++ks)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float wv[G], zv[G];
        load_g<T>(wrow + ((long)ks * 64 + q * 16) * G, wv);
        load_g<T>(zrow + ks * KS + q * G, zv);
#pragma unroll
        for (int e = 0; e < G; ++e) acc = fmaf(zv[e], wv[e], acc);
      }
    cap[r][which] = acc;
  }
  __syncthreads();
  if (tid < ROWS) {
    const int rt = tid >> 4, i = tid & 15;
    if (i < tile_n[rt]) {
      float m, s;
      join_waves_lse(red_m, red_s, tid, m, s);
      const long cell = ((long)tile_b[rt] * S + tile_s[rt]) * U1 + tile_u0[rt] + i;
      *reinterpret_cast<float4*>(part + (cell * n_split + blockIdx.y) * 4) = make_float4(m, s, cap[tid][0], cap[tid][1]);
    }
  }
}

// one thread per cell: the parts' (max, sum) joined, lp = logit - max - log(sum)
__global__ void joiner_lattice_fold_kernel(const float* __restrict__ part, const int32_t* __restrict__ src_len,
                                           const int32_t* __restrict__ tgt_len, float* __restrict__ lp_blank,
                                           float* __restrict__ lp_label, int B, int S, int U1, int n_split) {
  const long cell = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= (long)B * S * U1) return;
  const int u = (int)(cell % U1);
  const int s = (int)((cell / U1) % S);
  const int b = (int)(cell / ((long)U1 * S));
  const int tl = clampi(tgt_len[b], 0, U1 - 1);
  if (s >= clampi(src_len[b], 0, S) || u > tl) return;
  float m = LAT_NEG, sum = 0.f, bl = LAT_NEG, lb = LAT_NEG;
  for (int p = 0; p < n_split; ++p) {
    const float4 v = *reinterpret_cast<const float4*>(part + (cell * n_split + p) * 4);
    lse_join(m, sum, v.x, v.y);
    bl = fmaxf(bl, v.z);
    lb = fmaxf(lb, v.w);
  }
  const float ls = logf(sum);
  lp_blank[cell] = (bl - m) - ls;
  if (u < tl) lp_label[cell] = (lb - m) - ls;
}

// ---------------------------------------------------------------------------------------------------------- RNN-T forward
// The differences and sums of two neighbouring cells pass through an opaque register (empty asm with a "+v" operand), the guard of
// ln_apply in dec_chain.hip: the SLP vectoriser cannot fuse them into a packed fp32 instruction with an op_sel source swizzle.
__device__ __forceinline__ float opaque(float x) {
  asm volatile("" : "+v"(x));
  return x;
}
__device__ __forceinline__ float log_add(float a, float b) {
  const float mx = fmaxf(a, b), mn = fminf(a, b);
  if (mx == -INFINITY) return -INFINITY;
  const float d = opaque(mn - mx);
  return mx + __logf(1.0f + __expf(d));          // 1 + e^d in [1, 2]: v_exp / v_log, absolute error below 2^-22
}

// One workgroup per batch row; anti-diagonal d holds the cells (s, u) with s + u = d, kept in LDS indexed by u.
// WITH_BEST: the same recursion with max, one back-pointer byte per cell (1: the label move from (s, u - 1), 0: the blank move
// from (s - 1, u); the label move is taken only when it is STRICTLY better), back-tracked by thread 0.
template <bool WITH_BEST>
__global__ __launch_bounds__(256) void rnnt_forward_kernel(const float* __restrict__ lp_blank, const float* __restrict__ lp_label,
                                                           const int32_t* __restrict__ src_len, const int32_t* __restrict__ tgt_len,
                                                           float* __restrict__ ll, float* __restrict__ best_ll,
                                                           int32_t* __restrict__ emit, unsigned char* __restrict__ bp, int S, int U1) {
  extern __shared__ __align__(16) unsigned char smem_raw[];
  float* diag = reinterpret_cast<float*>(smem_raw);         // [2][U1] sum recursion, then [2][U1] max recursion
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Sb = clampi(src_len[b], 0, S), n = clampi(tgt_len[b], 0, U1 - 1);
  if (Sb < 1) {                                             // no source position: no path
    if (tid == 0) { ll[b] = -INFINITY; if (WITH_BEST) best_ll[b] = -INFINITY; }
    return;
  }
  const float* lb = lp_blank + (long)b * S * U1;
  const float* lt = lp_label + (long)b * S * U1;
  unsigned char* bpb = WITH_BEST ? bp + (long)b * S * U1 : nullptr;
  float* a0 = diag;
  float* a1 = diag + U1;
  float* m0 = diag + 2 * U1;
  float* m1 = diag + 3 * U1;
  if (tid == 0) { a0[0] = 0.f; if (WITH_BEST) m0[0] = 0.f; }
  __syncthreads();
  for (int d = 1; d <= Sb - 1 + n; ++d) {
    const int ulo = max(0, d - (Sb - 1)), uhi = min(n, d);
    for (int u = ulo + tid; u <= uhi; u += blockDim.x) {
      const int s = d - u;
      const bool from_blank = s >= 1, from_label = u >= 1;            // (s - 1, u) and (s, u - 1) lie on diagonal d - 1
      const float pb = from_blank ? lb[(long)(s - 1) * U1 + u] : 0.f;
      const float pl = from_label ? lt[(long)s * U1 + u - 1] : 0.f;
      const float sb = opaque(a0[u] + pb), sl = opaque(a0[from_label ? u - 1 : u] + pl);
      a1[u] = log_add(from_blank ? sb : -INFINITY, from_label ? sl : -INFINITY);
      if (WITH_BEST) {
        const float tb = opaque(m0[u] + pb), tl = opaque(m0[from_label ? u - 1 : u] + pl);
        const float vb = from_blank ? tb : -INFINITY, vl = from_label ? tl : -INFINITY;
        const bool label = vl > vb;
        m1[u] = label ? vl : vb;
        bpb[(long)s * U1 + u] = label ? 1 : 0;
      }
    }
    __syncthreads();
    float* t = a0; a0 = a1; a1 = t;
    t = m0; m0 = m1; m1 = t;
  }
  if (tid == 0) {
    const float last = lb[(long)(Sb - 1) * U1 + n];
    ll[b] = a0[n] + last;
    if (WITH_BEST) {
      best_ll[b] = m0[n] + last;
      int s = Sb - 1, u = n;
      while (s > 0 || u > 0) {                              // S_b - 1 + n moves
        if (u > 0 && (s == 0 || bpb[(long)s * U1 + u])) { emit[(long)b * U1 + u - 1] = s; --u; } else { --s; }
      }
    }
  }
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
template <typename T> size_t lattice_lds_bytes(int D) { return (size_t)16 * LatCfg<T>::R * (D + gemv::MF<T>::G) * sizeof(T); }
constexpr size_t LATTICE_LDS_MAX = 144 * 1024;      // of the compute unit's 160 KiB; the kernel's static arrays take the rest
constexpr int RNNT_MAX_U1 = 4096;                   // four diagonals of U1 floats in 64 KB of LDS

template <typename T>
int lattice_launch(simulst_handle* h, const float* P, const float* G, const void* W_fm, const int32_t* labels, const int32_t* src_len,
                   const int32_t* tgt_len, float* partials, int B, int S, int U1, int D, int V, int blank, int n_split) {
  const size_t lds = lattice_lds_bytes<T>(D);
  static const sl_lds_limit limits[] = {{(const void*)joiner_lattice_kernel<float>, (int)LATTICE_LDS_MAX},      // more than 64 KB of dynamic LDS
                                        {(const void*)joiner_lattice_kernel<bf16>, (int)LATTICE_LDS_MAX}};
  if (int rc = sl_raise_lds(h, SL_LDS_JOINER_LATTICE, limits, "simulst_joiner_lattice")) return rc;
  const int u_tiles = (U1 + 15) / 16;
  const long n_tiles = (long)B * S * u_tiles;
  const long wgs = (n_tiles + LatCfg<T>::R - 1) / LatCfg<T>::R;
  hipLaunchKernelGGL(joiner_lattice_kernel<T>, dim3((unsigned)wgs, n_split), dim3(LatCfg<T>::THREADS), lds, h->stream, P, G, (const T*)W_fm,
                     labels, src_len, tgt_len, partials, B, S, U1, D, V, blank, n_split, u_tiles);
  return SIMULST_OK;
}

template <typename T>
void scan_launch(simulst_handle* h, const float* P, const float* g, const void* W_fm, const int32_t* prev_emit, const int32_t* src_len,
                 const int32_t* finished, float* blank_logit, float* best, int32_t* best_idx, int R, int group, int S, int D, int V,
                 int blank, int n_split) {
  const int tiles_per_row = (S + 15) / 16;
  constexpr int Rr = ScanCfg<T>::R;
  hipLaunchKernelGGL(joiner_scan_kernel<T>, dim3((R * tiles_per_row + Rr - 1) / Rr, n_split), dim3(SCAN_THREADS), scan_lds_bytes<T>(D),
                     h->stream, P, g, (const T*)W_fm, prev_emit, src_len, finished, blank_logit, best, best_idx, R, group, S, D, V,
                     blank, n_split, tiles_per_row);
}

// simulst_joiner_scan (group 1, no finished list) and simulst_joiner_scan_beam
int scan_entry(simulst_handle* h, const char* who, const float* P, const float* g, const void* W_fm, const int32_t* prev_emit,
               const int32_t* src_len, const int32_t* finished, float* blank_logit, float* best, int32_t* best_idx, int R, int group,
               int S, int D, int V, int blank, int n_split, int dtype) {
  const std::string w(who);
  const int rc = joiner_check(h, who, R, S, D, V, blank, n_split, dtype);
  if (rc != SIMULST_OK) return rc;
  SL_REQUIRE(h, group >= 1 && R % group == 0, SIMULST_E_ARG, w + ": group >= 1, rows a multiple of group");
  const size_t lds = dtype == SIMULST_F32 ? scan_lds_bytes<float>(D) : scan_lds_bytes<bf16>(D);
  SL_REQUIRE(h, lds <= 48 * 1024, SIMULST_E_SHAPE, w + ": D too large for the row tiles in LDS");
  SL_REQUIRE(h, (int64_t)R * ((S + 15) / 16) < ((int64_t)1 << 31), SIMULST_E_SHAPE, w + ": rows * S' tiles");
  SL_CHECK_NULL(h, P); SL_CHECK_NULL(h, g); SL_CHECK_NULL(h, W_fm); SL_CHECK_NULL(h, prev_emit); SL_CHECK_NULL(h, src_len);
  SL_CHECK_NULL(h, blank_logit); SL_CHECK_NULL(h, best); SL_CHECK_NULL(h, best_idx);
  if (R == 0) return SIMULST_OK;
  KTimer t(h, SIMULST_K_SCAN);
  if (dtype == SIMULST_F32)
    scan_launch<float>(h, P, g, W_fm, prev_emit, src_len, finished, blank_logit, best, best_idx, R, group, S, D, V, blank, n_split);
  else
    scan_launch<bf16>(h, P, g, W_fm, prev_emit, src_len, finished, blank_logit, best, best_idx, R, group, S, D, V, blank, n_split);
  return sl_launch_status(h, who);
}

// simulst_joiner_emit (group 1, no finished list, no log) and simulst_joiner_emit_beam
int emit_entry(simulst_handle* h, const char* who, const float* P, const float* g, const float* blank_logit, const float* best,
               const int32_t* best_idx, int32_t* prev_emit, const int32_t* src_len, const int32_t* finished, void* z, int32_t* at_eos,
               int32_t* emit_log, int R, int group, int S, int D, int V, int blank, int n_split, int dtype) {
  const std::string w(who);
  const int rc = joiner_check(h, who, R, S, D, V, blank, n_split, dtype);
  if (rc != SIMULST_OK) return rc;
  SL_REQUIRE(h, group >= 1 && R % group == 0, SIMULST_E_ARG, w + ": group >= 1, rows a multiple of group");
  SL_CHECK_NULL(h, P); SL_CHECK_NULL(h, g); SL_CHECK_NULL(h, blank_logit); SL_CHECK_NULL(h, best); SL_CHECK_NULL(h, best_idx);
  SL_CHECK_NULL(h, prev_emit); SL_CHECK_NULL(h, src_len); SL_CHECK_NULL(h, z); SL_CHECK_NULL(h, at_eos);
  if (R == 0) return SIMULST_OK;
  KTimer t(h, SIMULST_K_SCAN);
  if (dtype == SIMULST_F32)
    hipLaunchKernelGGL(joiner_emit_kernel<float>, dim3(R), dim3(64), 0, h->stream, P, g, blank_logit, best, best_idx, prev_emit,
                       src_len, finished, (float*)z, at_eos, emit_log, group, S, D, blank, n_split);
  else
    hipLaunchKernelGGL(joiner_emit_kernel<bf16>, dim3(R), dim3(64), 0, h->stream, P, g, blank_logit, best, best_idx, prev_emit,
                       src_len, finished, (bf16*)z, at_eos, emit_log, group, S, D, blank, n_split);
  return sl_launch_status(h, who);
}

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
  return scan_entry(h, "simulst_joiner_scan", P, g, W_fm, prev_emit, src_len, nullptr, blank_logit, best, best_idx, B, 1, S, D, V,
                    blank, n_split, dtype);
}

extern "C" int simulst_joiner_scan_beam(simulst_handle* h, const float* P, const float* g, const void* W_fm, const int32_t* prev_emit,
                                        const int32_t* src_len, const int32_t* finished, float* blank_logit, float* best,
                                        int32_t* best_idx, int32_t R, int32_t group, int32_t S, int32_t D, int32_t V, int32_t blank,
                                        int32_t n_split, int32_t dtype) {
  if (!h) return SIMULST_E_NULL;
  return scan_entry(h, "simulst_joiner_scan_beam", P, g, W_fm, prev_emit, src_len, finished, blank_logit, best, best_idx, R, group, S,
                    D, V, blank, n_split, dtype);
}

extern "C" int simulst_joiner_emit(simulst_handle* h, const float* P, const float* g, const float* blank_logit, const float* best,
                                   const int32_t* best_idx, int32_t* prev_emit, const int32_t* src_len, void* z, int32_t* at_eos,
                                   int32_t B, int32_t S, int32_t D, int32_t V, int32_t blank, int32_t n_split, int32_t dtype) {
  if (!h) return SIMULST_E_NULL;
  return emit_entry(h, "simulst_joiner_emit", P, g, blank_logit, best, best_idx, prev_emit, src_len, nullptr, z, at_eos, nullptr, B, 1,
                    S, D, V, blank, n_split, dtype);
}

extern "C" int simulst_joiner_emit_beam(simulst_handle* h, const float* P, const float* g, const float* blank_logit, const float* best,
                                        const int32_t* best_idx, int32_t* prev_emit, const int32_t* src_len, const int32_t* finished,
                                        void* z, int32_t* at_eos, int32_t* emit_log, int32_t R, int32_t group, int32_t S, int32_t D,
                                        int32_t V, int32_t blank, int32_t n_split, int32_t dtype) {
  if (!h) return SIMULST_E_NULL;
  return emit_entry(h, "simulst_joiner_emit_beam", P, g, blank_logit, best, best_idx, prev_emit, src_len, finished, z, at_eos, emit_log,
                    R, group, S, D, V, blank, n_split, dtype);
}

extern "C" int simulst_transducer_beam_reorder(simulst_handle* h, const simulst_decoder_desc* dd, const simulst_dec_layer* src,
                                               const simulst_dec_layer* dst, const int32_t* prev_emit_src, int32_t* prev_emit_dst,
                                               const int32_t* reorder, const int32_t* finished, int32_t block, int32_t n_prev,
                                               int32_t* result) {
  if (!h) return SIMULST_E_NULL;
  SL_CHECK_NULL(h, dd);
  const int R = dd->B;
  SL_REQUIRE(h, dd->dtype == SIMULST_F32 || dd->dtype == SIMULST_BF16, SIMULST_E_ARG, "simulst_transducer_beam_reorder: dtype");
  SL_REQUIRE(h, R >= 0, SIMULST_E_ARG, "simulst_transducer_beam_reorder: rows B");
  SL_REQUIRE(h, dd->n_layers > 0 && dd->n_layers <= SL_REORDER_MAX_LAYERS && dd->H > 0 && dd->D > 0 && dd->D % dd->H == 0 &&
                (dd->D / dd->H) % 8 == 0 && dd->cap > 0,
             SIMULST_E_ARG, "simulst_transducer_beam_reorder: shape (at most 16 layers, head_dim a multiple of 8, cap > 0)");
  SL_REQUIRE(h, block >= 1 && (R == 0 || (block <= R && R % block == 0)), SIMULST_E_ARG,
             "simulst_transducer_beam_reorder: 1 <= block <= rows, rows a multiple of block");
  SL_REQUIRE(h, n_prev >= 0 && n_prev <= dd->cap, SIMULST_E_ARG, "simulst_transducer_beam_reorder: 0 <= n_prev <= cap");
  if (R == 0) return SIMULST_OK;
  SL_CHECK_NULL(h, src); SL_CHECK_NULL(h, dst); SL_CHECK_NULL(h, prev_emit_src); SL_CHECK_NULL(h, prev_emit_dst);
  SL_CHECK_NULL(h, reorder); SL_CHECK_NULL(h, result);
  for (int l = 0; l < dd->n_layers; ++l) {
    SL_CHECK_NULL(h, src[l].k_cache); SL_CHECK_NULL(h, src[l].v_cache); SL_CHECK_NULL(h, dst[l].k_cache); SL_CHECK_NULL(h, dst[l].v_cache);
  }
  return sl_beam_reorder(h, "simulst_transducer_beam_reorder", src, dst, false, prev_emit_src, prev_emit_dst, reorder, finished, result,
                         R, block, dd->n_layers, dd->H, dd->D / dd->H, dd->dtype, dd->cap, n_prev);
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

extern "C" int simulst_joiner_lattice(simulst_handle* h, const float* P, const float* G, const void* W_fm, const int32_t* labels,
                                      const int32_t* src_len, const int32_t* tgt_len, float* partials, float* lp_blank,
                                      float* lp_label, int32_t B, int32_t S, int32_t U1, int32_t D, int32_t V, int32_t blank,
                                      int32_t n_split, int32_t dtype) {
  if (!h) return SIMULST_E_NULL;
  const int rc = joiner_check(h, "simulst_joiner_lattice", B, S, D, V, blank, n_split, dtype);
  if (rc != SIMULST_OK) return rc;
  SL_REQUIRE(h, U1 >= 1, SIMULST_E_ARG, "simulst_joiner_lattice: U1 >= 1");
  const size_t lds = dtype == SIMULST_F32 ? lattice_lds_bytes<float>(D) : lattice_lds_bytes<bf16>(D);
  SL_REQUIRE(h, lds <= LATTICE_LDS_MAX, SIMULST_E_SHAPE, "simulst_joiner_lattice: D too large for the row panel in LDS");
  SL_REQUIRE(h, (int64_t)B * S * ((U1 + 15) / 16) < ((int64_t)1 << 31), SIMULST_E_SHAPE, "simulst_joiner_lattice: B * S' * U1 tiles");
  SL_CHECK_NULL(h, P); SL_CHECK_NULL(h, G); SL_CHECK_NULL(h, W_fm); SL_CHECK_NULL(h, labels); SL_CHECK_NULL(h, src_len);
  SL_CHECK_NULL(h, tgt_len); SL_CHECK_NULL(h, partials); SL_CHECK_NULL(h, lp_blank); SL_CHECK_NULL(h, lp_label);
  if (B == 0) return SIMULST_OK;
  KTimer t(h, SIMULST_K_SCAN);
  const int lrc = dtype == SIMULST_F32
                      ? lattice_launch<float>(h, P, G, W_fm, labels, src_len, tgt_len, partials, B, S, U1, D, V, blank, n_split)
                      : lattice_launch<bf16>(h, P, G, W_fm, labels, src_len, tgt_len, partials, B, S, U1, D, V, blank, n_split);
  if (lrc != SIMULST_OK) return lrc;
  const long cells = (long)B * S * U1;
  hipLaunchKernelGGL(joiner_lattice_fold_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, h->stream, partials, src_len,
                     tgt_len, lp_blank, lp_label, B, S, U1, n_split);
  return sl_launch_status(h, "simulst_joiner_lattice");
}

extern "C" int simulst_rnnt_forward(simulst_handle* h, const float* lp_blank, const float* lp_label, const int32_t* src_len,
                                    const int32_t* tgt_len, float* ll, float* best_ll, int32_t* emit, uint8_t* backptr, int32_t B,
                                    int32_t S, int32_t U1) {
  if (!h) return SIMULST_E_NULL;
  SL_REQUIRE(h, S >= 1, SIMULST_E_ARG, "simulst_rnnt_forward: S' >= 1");
  SL_REQUIRE(h, U1 >= 1, SIMULST_E_ARG, "simulst_rnnt_forward: U1 >= 1");
  SL_REQUIRE(h, B >= 0, SIMULST_E_ARG, "simulst_rnnt_forward: B");
  SL_REQUIRE(h, U1 <= RNNT_MAX_U1, SIMULST_E_SHAPE, "simulst_rnnt_forward: the diagonal (U1 floats, four of them) does not fit in LDS");
  SL_CHECK_NULL(h, lp_blank); SL_CHECK_NULL(h, lp_label); SL_CHECK_NULL(h, src_len); SL_CHECK_NULL(h, tgt_len); SL_CHECK_NULL(h, ll);
  const bool with_best = best_ll != nullptr || emit != nullptr || backptr != nullptr;
  if (with_best) { SL_CHECK_NULL(h, best_ll); SL_CHECK_NULL(h, emit); SL_CHECK_NULL(h, backptr); }
  if (B == 0) return SIMULST_OK;
  KTimer t(h, SIMULST_K_SCAN);
  const size_t lds = (size_t)4 * U1 * sizeof(float);
  if (with_best)
    hipLaunchKernelGGL(rnnt_forward_kernel<true>, dim3(B), dim3(256), lds, h->stream, lp_blank, lp_label, src_len, tgt_len, ll,
                       best_ll, emit, backptr, S, U1);
  else
    hipLaunchKernelGGL(rnnt_forward_kernel<false>, dim3(B), dim3(256), lds, h->stream, lp_blank, lp_label, src_len, tgt_len, ll,
                       best_ll, emit, backptr, S, U1);
  return sl_launch_status(h, "simulst_rnnt_forward");
}
