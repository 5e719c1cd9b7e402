// Offline decode with hypotheses finalised at EOS (gfx950): simulst_mma_retire_rows runs between two chunks of
// simulst_mma_decode and takes the rows that have finished -- at their first EOS or at their own step cap -- out of the
// batch, the way fairseq's SequenceGenerator drops finished hypotheses (eval/generate.py:187-209, beam 1).  Finished rows
// are scattered through the batch, so the live ones are compacted on the device: a stable partition pairs the k-th dead
// slot in front of the live count with the k-th live slot behind it, and every per-row buffer of the source slot is
// copied into its hole.  The next chunk then runs simulst_mma_decode over a prefix of the rows, in the kernel class the
// full batch started in.
//   retire_scan_kernel      thread per slot: the chunk's tokens into the row's hypothesis, finished rows leave slot_row
//   retire_partition_kernel one workgroup: live count, (hole, source) pairs, the small per-row fields, rows_next
//   retire_move_kernel      workgroup per (pair, layer, head): self K/V [0, n_prev), cross K/V (+ soft keys) [0, enc_len),
//                           pooled keys of complete windows, in 16-byte copies
#include "decode_plan.h"

namespace {

constexpr int RT_MAX_LAYERS = 16;

// the per-layer pointers the kernels need (the simulst_dec_layer array itself is host memory)
struct RetireLayers {
  char* kc[RT_MAX_LAYERS];
  char* vc[RT_MAX_LAYERS];
  char* km[RT_MAX_LAYERS];
  char* ks[RT_MAX_LAYERS];        // soft-attention keys, may be null
  char* vx[RT_MAX_LAYERS];
  char* kp[RT_MAX_LAYERS];        // pooled monotonic keys (fp32), may be null
  long* head_step[RT_MAX_LAYERS];
  unsigned char* head_read[RT_MAX_LAYERS];   // may be null
};

// result[] layout: [0] n_live, [1] rows_next, [2] pairs, [3] 0, then the holes [B] and the sources [B] of the pairs
constexpr int RT_HDR = 4;

__global__ __launch_bounds__(256) void retire_scan_kernel(const long* __restrict__ chunk, int n_steps, int rows,
                                                          const int* __restrict__ n_prev, int* __restrict__ slot_row,
                                                          const int* __restrict__ row_cap, long* __restrict__ hyp, int U, int B,
                                                          int pad_idx, int eos_idx) {
  const int slot = blockIdx.x * 256 + threadIdx.x;
  if (slot >= rows) return;
  const int r = slot_row[slot];
  if (r < 0 || r >= B) return;
  const int cap = min(row_cap[slot], U);
  const int s0 = n_prev[slot] - n_steps;        // tokens the row held before this chunk
  long* hr = hyp + (long)r * U;
  int end = -1;                                 // the hypothesis ends before this position
  for (int i = 0; i < n_steps; ++i) {
    const int pos = s0 + i;
    if (pos < 0) continue;
    if (pos >= cap) { end = pos; break; }
    const long t = chunk[(long)i * rows + slot];
    hr[pos] = t;
    if (t == eos_idx || pos + 1 >= cap) { end = pos + 1; break; }
  }
  if (end >= 0) {
    for (int p = max(end, 0); p < U; ++p) hr[p] = pad_idx;
    slot_row[slot] = -1;
  }
}

// slots s of [lo, hi) whose liveness (slot_row[s] >= 0) is want_live, in slot order -> out[0..) (out may be null); returns the
// count.  Every thread of the 1024-thread workgroup calls it (wave ballots + a prefix over the 16 waves' counts).
__device__ int rt_compact(const int* __restrict__ slot_row, int lo, int hi, bool want_live, int* __restrict__ out, int* wsum,
                          int* base) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __syncthreads();                              // every thread has read the previous call's count
  if (tid == 0) *base = 0;
  __syncthreads();
  for (int s0 = lo; s0 < hi; s0 += 1024) {
    const int s = s0 + tid;
    const bool p = s < hi && ((slot_row[s] >= 0) == want_live);
    const unsigned long long m = __ballot(p);
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int off = *base;
    for (int w = 0; w < wave; ++w) off += wsum[w];
    if (p && out) out[off + __popcll(m & ((1ull << lane) - 1ull))] = s;
    __syncthreads();
    if (tid == 0) { int t = 0; for (int w = 0; w < 16; ++w) t += wsum[w]; *base += t; }
    __syncthreads();
  }
  return *base;
}

__global__ __launch_bounds__(1024) void retire_partition_kernel(int rows, int B, int H, int n_layers, int floor_rows,
                                                                int* __restrict__ slot_row, int* __restrict__ row_cap,
                                                                long* __restrict__ last_tokens, int* __restrict__ n_prev,
                                                                int* __restrict__ enc_len, int* __restrict__ enc_len_bh,
                                                                RetireLayers L, int* __restrict__ result) {
  __shared__ int wsum[16];
  __shared__ int base;
  int* holes = result + RT_HDR;
  int* srcs = result + RT_HDR + B;
  const int n_live = rt_compact(slot_row, 0, rows, true, nullptr, wsum, &base);
  // dead slots in front of the live count and live slots behind it: as many of one as of the other
  const int n_holes = rt_compact(slot_row, 0, n_live, false, holes, wsum, &base);
  rt_compact(slot_row, n_live, rows, true, srcs, wsum, &base);
  __syncthreads();
  // the small per-row fields of every pair (sources and holes are disjoint: no ordering hazard)
  for (int k = threadIdx.x; k < n_holes; k += 1024) {
    const int dst = holes[k], src = srcs[k];
    slot_row[dst] = slot_row[src];
    slot_row[src] = -1;
    row_cap[dst] = row_cap[src];
    last_tokens[dst] = last_tokens[src];
    n_prev[dst] = n_prev[src];
    enc_len[dst] = enc_len[src];
    for (int h = 0; h < H; ++h) {
      if (enc_len_bh) enc_len_bh[dst * H + h] = enc_len_bh[src * H + h];
      for (int l = 0; l < n_layers; ++l) {
        L.head_step[l][dst * H + h] = L.head_step[l][src * H + h];
        if (L.head_read[l]) L.head_read[l][dst * H + h] = L.head_read[l][src * H + h];
      }
    }
  }
  if (threadIdx.x == 0) {
    // whole 16-row tiles, never below the floor of the full batch's kernel class, never more rows than this chunk ran
    int next = 0;
    if (n_live > 0) next = min(rows, max(floor_rows, (n_live + 15) / 16 * 16));
    result[0] = n_live;
    result[1] = next;
    result[2] = n_holes;
    result[3] = 0;
  }
}

__device__ __forceinline__ void rt_copy(char* base, long dst_off, long src_off, long bytes) {
  uint4* d = reinterpret_cast<uint4*>(base + dst_off);
  const uint4* s = reinterpret_cast<const uint4*>(base + src_off);
  for (long i = threadIdx.x; i < (bytes >> 4); i += 256) d[i] = s[i];
}

__global__ __launch_bounds__(256) void retire_move_kernel(const int* __restrict__ result, int B, int H, int d, int esz, int cap,
                                                          int S_cap, int P_cap, int ratio, const int* __restrict__ n_prev,
                                                          const int* __restrict__ enc_len, RetireLayers L) {
  const int k = blockIdx.x, l = blockIdx.y, h = blockIdx.z;
  if (k >= result[2]) return;
  const int dst = result[RT_HDR + k], src = result[RT_HDR + B + k];
  const int np = min(max(n_prev[src], 0), cap);
  const int el = min(max(enc_len[src], 0), S_cap);
  const long row = (long)d * esz;                                   // bytes per position of one head
  // self-attention caches [B][H][cap][d]: the positions written so far
  const long so = (long)cap * row;
  rt_copy(L.kc[l], ((long)dst * H + h) * so, ((long)src * H + h) * so, np * row);
  rt_copy(L.vc[l], ((long)dst * H + h) * so, ((long)src * H + h) * so, np * row);
  // cross-attention projections [B][H][S_cap][d]: the valid source rows
  const long co = (long)S_cap * row;
  rt_copy(L.km[l], ((long)dst * H + h) * co, ((long)src * H + h) * co, el * row);
  rt_copy(L.vx[l], ((long)dst * H + h) * co, ((long)src * H + h) * co, el * row);
  if (L.ks[l]) rt_copy(L.ks[l], ((long)dst * H + h) * co, ((long)src * H + h) * co, el * row);
  // pooled keys [B][H][P_cap][d] fp32: the complete pre-decision windows (the only ones the policy reads from the cache)
  if (L.kp[l] && ratio > 0) {
    const long pr = (long)d * 4, po = (long)P_cap * pr;
    rt_copy(L.kp[l], ((long)dst * H + h) * po, ((long)src * H + h) * po, (long)min(P_cap, el / ratio) * pr);
  }
}

}  // namespace

extern "C" int simulst_mma_retire_rows(simulst_handle* h, const simulst_decoder_desc* dd, const simulst_dec_layer* layers,
                                       const int64_t* chunk_tokens, int32_t n_steps, int32_t rows, int32_t B, int32_t* slot_row,
                                       int32_t* row_cap, int64_t* last_tokens, int64_t* hyp, int32_t U, int32_t* enc_len_bh,
                                       int32_t* result) {
  if (!h) return SIMULST_E_NULL;
  SL_CHECK_NULL(h, dd); SL_CHECK_NULL(h, layers); SL_CHECK_NULL(h, chunk_tokens); SL_CHECK_NULL(h, slot_row);
  SL_CHECK_NULL(h, row_cap); SL_CHECK_NULL(h, last_tokens); SL_CHECK_NULL(h, hyp); SL_CHECK_NULL(h, result);
  SL_REQUIRE(h, n_steps > 0, SIMULST_E_SHAPE, "simulst_mma_retire_rows: n_steps must be positive");
  SL_REQUIRE(h, rows > 0 && rows <= B, SIMULST_E_SHAPE, "simulst_mma_retire_rows: 0 < rows <= B");
  SL_REQUIRE(h, U > 0, SIMULST_E_SHAPE, "simulst_mma_retire_rows: hypothesis length U");
  SL_REQUIRE(h, dd->dtype == SIMULST_F32 || dd->dtype == SIMULST_BF16, SIMULST_E_DTYPE, "simulst_mma_retire_rows: dtype");
  SL_REQUIRE(h, dd->n_layers > 0 && dd->n_layers <= RT_MAX_LAYERS && dd->H > 0 && dd->D % dd->H == 0 && (dd->D / dd->H) % 8 == 0 &&
                dd->cap > 0 && dd->S_cap > 0 && dd->P_cap >= 0,
             SIMULST_E_SHAPE, "simulst_mma_retire_rows: shape (at most 16 layers, head_dim a multiple of 8)");
  SL_CHECK_NULL(h, dd->n_prev); SL_CHECK_NULL(h, dd->enc_len);
  RetireLayers L = {};
  for (int l = 0; l < dd->n_layers; ++l) {
    const simulst_dec_layer& a = layers[l];
    SL_CHECK_NULL(h, a.k_cache); SL_CHECK_NULL(h, a.v_cache); SL_CHECK_NULL(h, a.Kmono); SL_CHECK_NULL(h, a.V);
    SL_CHECK_NULL(h, a.head_step);
    SL_REQUIRE(h, !a.Kpool || dd->P_cap > 0, SIMULST_E_SHAPE, "simulst_mma_retire_rows: Kpool needs P_cap");
    L.kc[l] = (char*)a.k_cache; L.vc[l] = (char*)a.v_cache; L.km[l] = (char*)a.Kmono; L.ks[l] = (char*)a.Ksoft;
    L.vx[l] = (char*)a.V; L.kp[l] = (char*)a.Kpool; L.head_step[l] = (long*)a.head_step; L.head_read[l] = a.head_read;
  }
  const int H = dd->H, d = dd->D / dd->H, esz = dd->dtype == SIMULST_F32 ? 4 : 2;
  KTimer t(h, SIMULST_K_MISC);
  hipLaunchKernelGGL(retire_scan_kernel, dim3((rows + 255) / 256), dim3(256), 0, h->stream, (const long*)chunk_tokens, n_steps, rows,
                     (const int*)dd->n_prev, slot_row, (const int*)row_cap, (long*)hyp, U, B, dd->pad_idx, dd->eos_idx);
  int rc = sl_launch_status(h, "simulst_mma_retire_rows(scan)");
  if (rc) return rc;
  hipLaunchKernelGGL(retire_partition_kernel, dim3(1), dim3(1024), 0, h->stream, rows, B, H, dd->n_layers, sl_retire_floor_rows(h, B),
                     slot_row, row_cap, (long*)last_tokens, dd->n_prev, (int*)dd->enc_len, enc_len_bh, L, result);
  if ((rc = sl_launch_status(h, "simulst_mma_retire_rows(partition)"))) return rc;
  // at most rows / 2 pairs: a workgroup per (pair, layer, head), those beyond the device-side pair count leave at once
  if (rows / 2 > 0) {
    hipLaunchKernelGGL(retire_move_kernel, dim3(rows / 2, dd->n_layers, H), dim3(256), 0, h->stream, (const int*)result, B, H, d, esz,
                       dd->cap, dd->S_cap, dd->P_cap, dd->ratio, (const int*)dd->n_prev, (const int*)dd->enc_len, L);
    rc = sl_launch_status(h, "simulst_mma_retire_rows(move)");
  }
  return rc;
}
