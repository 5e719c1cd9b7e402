// Batched Levenshtein alignment of int64 label strings for gfx950 -- simulst_edit_distance (include/simulst_hip.h; DESIGN.md "CTC
// head", subsection "Error rates").  The word / token error rate of the reference's ASR stage (tasks/speech_to_text_infer.py:206-215, fairseq's WerScorer over the editdistance
// package) is the sum of these distances over the sum of the reference lengths.
//
// One WAVE per pair, pairs by index (one reference row can face 16 hypotheses, a list can face itself), strings read in place.
//   * the hypothesis lies across the lanes, 64 columns a strip; the reference's labels are staged once in LDS and enter at lane 0
//   * inside a strip the cells run as an anti-diagonal wavefront: lane l works on row s - l + 1 at step s, takes D[i][j-1] from lane
//     l - 1 with ONE wave shift (DPP wave_shr:1) per value, keeps D[i-1][j] and D[i-1][j-1] in registers
//   * a cell is (distance, sub | del << 10 | ins << 20): the three counts travel forward with the minimum (each is at most the
//     distance, at most 1023), so the counts-only form has no back-pointers, no global traffic but the strings and 16 bytes out
//   * hypotheses above 64 labels: the last column of a strip goes through an LDS column [Lr + 1] to lane 0 of the next strip (written
//     63 steps behind where it is read, so one buffer serves).  A call whose hypothesis capacity is <= 64 allocates no such column,
//     and LDS is sized by the call's capacities, not by the 1023-label limit
//   * tie rule (the contract): diagonal, then deletion, then insertion -- the two strict '<' below
//   * path: one byte per cell in caller scratch, in the ORDER THE WAVEFRONT WRITES THEM ([strip][step][lane]: 64 contiguous bytes a
//     step); the back-track runs on the device like ctc_align_kernel's: 64 steps of back-pointers (4 KB, contiguous) are staged in
//     LDS by the wave, then lane 0 walks them.  The number of operations is Lr + ins, known before the walk, so the alignment is
//     written front to back in one pass
// Integers throughout: a pair's result depends on nothing but its two strings.
#include "common.h"

namespace {

constexpr int ED_MAX = 1023;            // labels of a string (the limit simulst_ctc_best_alignment has)
constexpr int ED_TILE = 64 * 64;        // staged back-pointers: 64 steps x 64 lanes

// value of lane l - 1 (lane 0 keeps `own`): v_mov_b32_dpp wave_shr:1
__device__ __forceinline__ int wave_shr1(int own, int v) { return __builtin_amdgcn_update_dpp(own, v, 0x138, 0xf, 0xf, false); }

// LDS writes of some lanes are read by other lanes of the SAME wave: DS operations of a wave complete in order, what is needed is
// that the compiler keeps the order and the data has arrived
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

__host__ __device__ inline long ed_bp_pair_bytes(int capR, int capH) { return (long)((capH + 63) / 64) * (capR + 63) * 64; }
// LDS of one wave, each part a multiple of 16 bytes: the reference's labels, the strip-boundary column, the staged back-pointers
__host__ __device__ inline int ed_ref_lds(int capR) { return ((capR + 1) & ~1) * 8; }
__host__ __device__ inline int ed_col_lds(int capR, int capH) { return capH > 64 ? ((capR + 2) & ~1) * 8 : 0; }
__host__ __device__ inline int ed_wave_lds(int capR, int capH, bool path) {
  return ed_ref_lds(capR) + ed_col_lds(capR, capH) + (path ? ED_TILE : 0);
}

template <bool PATH>
__global__ __launch_bounds__(256) void edit_distance_kernel(const long* __restrict__ ref, long ref_b, const long* __restrict__ ref_len,
                                                            const long* __restrict__ hyp, long hyp_b, const long* __restrict__ hyp_len,
                                                            const int* __restrict__ ref_idx, const int* __restrict__ hyp_idx, int N,
                                                            int n_ref, int n_hyp, int capR, int capH, int* __restrict__ counts,
                                                            unsigned char* __restrict__ bp, void* __restrict__ ops,
                                                            int* __restrict__ n_ops, int ops_cap, int ops_width, int pad) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (p >= N) return;                                                        // (no workgroup barrier anywhere below)
  unsigned char* mine = smem_raw + (size_t)(threadIdx.x >> 6) * ed_wave_lds(capR, capH, PATH);
  long* rs = reinterpret_cast<long*>(mine);                                  // [capR]: the reference's labels
  uint2* bnd = reinterpret_cast<uint2*>(mine + ed_ref_lds(capR));            // [capR + 1]: D[i][64 k] of the strip before (capH > 64)
  unsigned char* tile = mine + ed_ref_lds(capR) + ed_col_lds(capR, capH);
  const int ri = ref_idx ? ref_idx[p] : p, hi = hyp_idx ? hyp_idx[p] : p;
  bool ok = ri >= 0 && ri < n_ref && hi >= 0 && hi < n_hyp;
  const long lr64 = ok ? ref_len[ri] : 0, lh64 = ok ? hyp_len[hi] : 0;
  ok = ok && lr64 >= 0 && lr64 <= capR && lh64 >= 0 && lh64 <= capH;
  auto put_op = [&](int at, int code) {
    if (ops_width == 4) reinterpret_cast<int*>(ops)[(long)p * ops_cap + at] = code;
    else reinterpret_cast<signed char*>(ops)[(long)p * ops_cap + at] = (signed char)code;
  };
  if (!ok) {                                                                 // an index or a length the buffers do not have: no string is read
    if (lane < 4) counts[4 * (long)p + lane] = -1;
    if (PATH) {
      if (lane == 0) n_ops[p] = 0;
      for (int q = lane; q < ops_cap; q += 64) put_op(q, pad);
    }
    return;
  }
  const int Lr = (int)lr64, Lh = (int)lh64;
  const long* r = ref + (long)ri * ref_b;
  const long* h = hyp + (long)hi * hyp_b;
  for (int q = lane; q < Lr; q += 64) rs[q] = r[q];
  wave_lds_sync();
  const int n_strips = (Lh + 63) >> 6, row_steps = capR + 63;
  unsigned char* bpp = PATH ? bp + (long)p * ed_bp_pair_bytes(capR, capH) : nullptr;
  int myd = 0;
  unsigned myc = 0;
  for (int k = 0; k < n_strips; ++k) {
    const int j = k * 64 + lane + 1;                                         // this lane's column, 1-based
    const bool col = j <= Lh, last = k == n_strips - 1;
    const long hl = col ? h[j - 1] : 0;
    const int hl_lo = (int)hl, hl_hi = (int)(hl >> 32);
    myd = j; myc = (unsigned)j << 20;                                        // D[0][j]: j insertions
    int dgd = j - 1;                                                         // D[0][j-1]
    unsigned dgc = (unsigned)(j - 1) << 20;
    const int steps = Lr > 0 ? Lr + (last ? ((Lh - 1) & 63) : 63) : 0;       // (no reference label: row 0 is the answer)
    // what lane 0 takes in at a step is loaded a step ahead (the addresses depend on s alone): reference label s + 1, which then
    // travels up the lanes with the cells (lane l is on row s - l + 1), and D[s + 1][64 k] of the strip before
    long r_in = Lr > 0 ? rs[0] : 0;
    uint2 e_in = make_uint2(0u, 0u);
    if (k > 0) e_in = bnd[min(1, Lr)];
    int rl_lo = 0, rl_hi = 0;
    for (int s = 0; s < steps; ++s) {
      const int i = s - lane + 1;                                            // this lane's row, 1-based
      const int i0 = min(s + 1, Lr);                                         // lane 0's row
      uint2 edge = make_uint2((unsigned)i0, (unsigned)i0 << 10);             // D[i][0]: i deletions
      if (k > 0) edge = e_in;
      const long r_now = r_in;
      r_in = rs[min(s + 1, Lr - 1)];
      if (k > 0) e_in = bnd[min(s + 2, Lr)];                                 // (written 63 steps from now at the earliest)
      const int ld = wave_shr1((int)edge.x, myd);                            // D[i][j-1]
      const unsigned lc = (unsigned)wave_shr1((int)edge.y, (int)myc);
      rl_lo = wave_shr1((int)r_now, rl_lo);
      rl_hi = wave_shr1((int)(r_now >> 32), rl_hi);
      if (col && i >= 1 && i <= Lr) {
        const bool eq = rl_lo == hl_lo && rl_hi == hl_hi;
        int bd = dgd + (eq ? 0 : 1);
        unsigned bc = dgc + (eq ? 0u : 1u);
        int op = eq ? 0 : 1;
        if (myd + 1 < bd) { bd = myd + 1; bc = myc + (1u << 10); op = 2; }   // deletion: reference label i has no counterpart
        if (ld + 1 < bd) { bd = ld + 1; bc = lc + (1u << 20); op = 3; }      // insertion
        dgd = ld; dgc = lc;
        myd = bd; myc = bc;
        if (PATH) bpp[((long)k * row_steps + s) * 64 + lane] = (unsigned char)op;
        if (lane == 63 && !last) bnd[i] = make_uint2((unsigned)bd, bc);
      }
    }
    if (!last) wave_lds_sync();
  }
  int d = Lr;
  unsigned c = (unsigned)Lr << 10;                                           // an empty hypothesis: Lr deletions
  if (Lh > 0) {
    d = __shfl(myd, (Lh - 1) & 63, 64);
    c = (unsigned)__shfl((int)myc, (Lh - 1) & 63, 64);
  }
  const int n_sub = c & 1023, n_del = (c >> 10) & 1023, n_ins = (c >> 20) & 1023;
  if (lane < 4) counts[4 * (long)p + lane] = lane == 0 ? d : lane == 1 ? n_sub : lane == 2 ? n_del : n_ins;
  if (!PATH) return;
  // ---- the alignment, front to back: Lr + ins operations (every reference label is matched, substituted or deleted)
  const int n = Lr + n_ins;
  if (lane == 0) n_ops[p] = n;
  for (int q = n + lane; q < ops_cap; q += 64) put_op(q, pad);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");                         // the back-pointers other lanes wrote are read below
  __builtin_amdgcn_wave_barrier();
  int i = Lr, j = Lh, at = n - 1;
  while (i > 0 && j > 0) {
    const int k = (j - 1) >> 6, l0 = (j - 1) & 63;
    const int s_hi = i - 1 + l0, s_lo = max(s_hi - 63, 0);
    const uint4* src = reinterpret_cast<const uint4*>(bpp + ((long)k * row_steps + s_lo) * 64);
    for (int q = lane; q < (s_hi - s_lo + 1) * 4; q += 64) reinterpret_cast<uint4*>(tile)[q] = src[q];
    wave_lds_sync();
    if (lane == 0) {
      int l = l0, s = s_hi;
      while (i > 0 && l >= 0 && s >= s_lo) {                                 // (l >= 0: j stays in the strip, so j > 0)
        const int op = tile[(s - s_lo) * 64 + l];
        if (at >= 0) put_op(at, op);                                         // (at >= 0 always: the walk has Lr + ins steps)
        --at;
        if (op <= 1) { --i; --j; --l; s -= 2; }
        else if (op == 2) { --i; --s; }
        else { --j; --l; --s; }
      }
    }
    i = __shfl(i, 0, 64); j = __shfl(j, 0, 64); at = __shfl(at, 0, 64);
    wave_lds_sync();
  }
  // what is left of one string: the head of the alignment (at + 1 == i + j here)
  for (int q = lane; q <= at; q += 64) put_op(q, i > 0 ? 2 : 3);
}

}  // namespace

extern "C" int simulst_edit_distance(simulst_handle* h, const int64_t* refs, int64_t ref_stride_b, const int64_t* ref_lengths,
                                     const int64_t* hyp_lengths, int32_t ref_cap, int32_t hyp_cap, int32_t N,
                                     const simulst_edit_desc* desc, void* ops) {
  if (!h) return SIMULST_E_NULL;
  const char* who = "simulst_edit_distance";
  SL_CHECK_NULL(h, desc);
  const simulst_edit_desc* d = desc;
  SL_CHECK_NULL(h, refs); SL_CHECK_NULL(h, ref_lengths); SL_CHECK_NULL(h, hyp_lengths);
  SL_CHECK_NULL(h, d->hyp); SL_CHECK_NULL(h, d->counts);
  SL_REQUIRE(h, ref_cap <= ED_MAX && hyp_cap <= ED_MAX, SIMULST_E_SHAPE,
             "simulst_edit_distance: more than 1023 labels in a string");
  SL_REQUIRE(h, ref_cap >= 0 && hyp_cap >= 0 && d->n_ref >= 0 && d->n_hyp >= 0, SIMULST_E_SHAPE, "simulst_edit_distance: shape");
  // pairs by position name rows 0 .. N-1: known here.  Indices on the device are compared with n_ref / n_hyp by the kernel
  SL_REQUIRE(h, d->ref_idx || N <= d->n_ref, SIMULST_E_SHAPE, "simulst_edit_distance: pair index past the reference rows");
  SL_REQUIRE(h, d->hyp_idx || N <= d->n_hyp, SIMULST_E_SHAPE, "simulst_edit_distance: pair index past the hypothesis rows");
  const bool path = ops != nullptr;
  if (path) {
    SL_CHECK_NULL(h, d->n_ops);
    SL_REQUIRE(h, d->ops_width == 1 || d->ops_width == 4, SIMULST_E_SHAPE, "simulst_edit_distance: ops_width is 1 or 4");
    SL_REQUIRE(h, d->ops_cap >= ref_cap + hyp_cap, SIMULST_E_SHAPE,
               "simulst_edit_distance: ops_cap below the two capacities' sum");
  }
  if (N <= 0) return SIMULST_OK;
  if (path) {
    SL_CHECK_NULL(h, d->bp);
    SL_REQUIRE(h, (reinterpret_cast<uintptr_t>(d->bp) & 15) == 0, SIMULST_E_ARG,
               "simulst_edit_distance: back-pointer scratch is not 16-byte aligned");
    SL_REQUIRE(h, d->bp_bytes >= (int64_t)N * ed_bp_pair_bytes(ref_cap, hyp_cap), SIMULST_E_SHAPE,
               "simulst_edit_distance: back-pointer scratch below SIMULST_EDIT_BP_BYTES");
  }
  // several pairs a workgroup while their LDS fits the default 48 KB; the 1023-label layout runs a wave a workgroup
  const int per_wave = ed_wave_lds(ref_cap, hyp_cap, path);
  const int waves = per_wave * 4 <= 48 * 1024 ? 4 : per_wave * 2 <= 48 * 1024 ? 2 : 1;
  const dim3 grid((N + waves - 1) / waves), block(64 * waves);
  const size_t lds = (size_t)per_wave * waves;
  KTimer t(h, SIMULST_K_SCAN);
  if (path)
    hipLaunchKernelGGL(edit_distance_kernel<true>, grid, block, lds, h->stream, (const long*)refs, (long)ref_stride_b,
                       (const long*)ref_lengths, (const long*)d->hyp, (long)d->hyp_stride_b, (const long*)hyp_lengths, d->ref_idx,
                       d->hyp_idx, N, d->n_ref, d->n_hyp, ref_cap, hyp_cap, d->counts, (unsigned char*)d->bp, ops, d->n_ops, d->ops_cap,
                       d->ops_width, d->pad);
  else
    hipLaunchKernelGGL(edit_distance_kernel<false>, grid, block, lds, h->stream, (const long*)refs, (long)ref_stride_b,
                       (const long*)ref_lengths, (const long*)d->hyp, (long)d->hyp_stride_b, (const long*)hyp_lengths, d->ref_idx,
                       d->hyp_idx, N, d->n_ref, d->n_hyp, ref_cap, hyp_cap, d->counts, (unsigned char*)nullptr, (void*)nullptr,
                       (int*)nullptr, 0, 1, d->pad);
  return sl_launch_status(h, who);
}
