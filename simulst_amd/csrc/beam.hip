// Beam search over offline MMA / wait-k decoding (gfx950): fairseq's SequenceGenerator with search.BeamSearch at the defaults the
// reference runs (normalize_scores, min_len 1, no unk penalty, temperature 1).  Sentence s owns the beam rows r = s * beam + j;
// K = 2 * beam candidates per row and per sentence.  Each decode step runs, on the handle's stream:
//   beam_topk_kernel      workgroup per row: masked log-softmax of the row's fp32 logits and its top K (lp, token) pairs
//   beam_select_kernel    wave per sentence: merge of the beam candidate lists into the sentence's top K, finalisation of EOS
//                         candidates, the next rows (reorder index, input token, cumulative score) and the step's back-pointers
//   beam_reorder_kernel   workgroup per (row, layer, head): the parent row's self-attention K/V prefix and monotonic step (and
//                         head_read) into the second buffer set, in 16-byte copies; the transducer's reorder
//                         (simulst_transducer_beam_reorder) is the same kernel with a per-row prev_emit in place of the steps
// and once at the end
//   beam_backtrack_kernel wave per sentence: the finalised hypotheses by descending score, walked back through the back-pointers.
// Order of candidates everywhere: descending score, equal scores to the lower flat index j * V + token.
#include <math.h>

#include "common.h"

namespace {

constexpr int BM_MAX_BEAM = 16;
constexpr int BM_TOPK_THREADS = 256;

// a before b in candidate order
__device__ __forceinline__ bool bm_before(float va, int ia, float vb, int ib) { return va > vb || (va == vb && ia < ib); }

// the (value, index) pair of the wave that comes first in candidate order, on every lane
__device__ __forceinline__ void bm_wave_best(float& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(i, o);
    if (bm_before(ov, oi, v, i)) { v = ov; i = oi; }
  }
}

// rule 2: log_softmax in fp32 as torch computes it ((x - max) - log(sum exp(x - max))), then the masks (NaN -> -inf as fairseq does)
__device__ __forceinline__ float bm_masked_lp(float x, int v, float m, float lse, int pad, int eos, bool no_eos, bool eos_only) {
  float y = (x - m) - lse;
  if (y != y || v == pad || (no_eos && v == eos) || (eos_only && v != eos)) y = -INFINITY;
  return y;
}

// every element of this thread's share of a row, f(value, index): float4 quads when V % 4 == 0, single elements otherwise
template <bool VEC, typename F>
__device__ __forceinline__ void bm_for_each(const float* __restrict__ row, int V, F f) {
  if (VEC) {
    const float4* q = reinterpret_cast<const float4*>(row);
    for (int i = threadIdx.x; i < (V >> 2); i += BM_TOPK_THREADS) {
      const float4 x = q[i];
      f(x.x, 4 * i); f(x.y, 4 * i + 1); f(x.z, 4 * i + 2); f(x.w, 4 * i + 3);
    }
  } else {
    for (int i = threadIdx.x; i < V; i += BM_TOPK_THREADS) f(row[i], i);
  }
}

template <bool VEC>
__global__ __launch_bounds__(BM_TOPK_THREADS) void beam_topk_kernel(const float* __restrict__ logits, int V, int beam, int step,
                                                                     const int* __restrict__ max_len, const int* __restrict__ finished,
                                                                     int pad, int eos, float* __restrict__ cand_lp,
                                                                     int* __restrict__ cand_tok) {
  __shared__ float red_v[2][BM_TOPK_THREADS / 64];
  __shared__ int red_i[2][BM_TOPK_THREADS / 64];
  __shared__ float red_s[BM_TOPK_THREADS / 64];
  const int r = blockIdx.x, s = r / beam, j = r % beam, K = 2 * beam;
  if ((finished && finished[s]) || (step == 0 && j > 0)) return;     // finished sentence; step 0 reads beam row 0 alone
  const float* row = logits + (long)r * V;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // pass 1: max and sum of exp(x - max) over the whole row (online)
  float m = -INFINITY, sum = 0.f;
  bm_for_each<VEC>(row, V, [&](float x, int) {
    if (x > m) { sum = sum * expf(m - x) + 1.f; m = x; }
    else if (x > -INFINITY) sum += expf(x - m);
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o), os = __shfl_xor(sum, o);
    const float nm = fmaxf(m, om);
    sum = (nm == -INFINITY) ? 0.f : sum * expf(m - nm) + os * expf(om - nm);
    m = nm;
  }
  if (lane == 0) { red_v[0][wave] = m; red_s[wave] = sum; }
  __syncthreads();
  float M = -INFINITY, S = 0.f;
  for (int w = 0; w < BM_TOPK_THREADS / 64; ++w) {
    const float wm = red_v[0][w], ws = red_s[w], nm = fmaxf(M, wm);
    S = (nm == -INFINITY) ? 0.f : S * expf(M - nm) + ws * expf(wm - nm);
    M = nm;
  }
  __syncthreads();
  const float lse = logf(S);
  const bool no_eos = step == 0, eos_only = step >= max_len[s];
  // pass 2: K rounds of a workgroup arg-max.  Each thread keeps the first element of its share that comes after everything already
  // taken; only the thread whose element was taken looks for its next one.
  float bv = -INFINITY;
  int bi = 0x7fffffff;                                               // sentinel: after every real element
  auto next_after = [&](float tv, int ti) {
    float nv = -INFINITY;
    int ni = 0x7fffffff;
    bm_for_each<VEC>(row, V, [&](float x, int v) {
      const float y = bm_masked_lp(x, v, M, lse, pad, eos, no_eos, eos_only);
      if (bm_before(tv, ti, y, v) && bm_before(y, v, nv, ni)) { nv = y; ni = v; }
    });
    bv = nv;
    bi = ni;
  };
  next_after(INFINITY, -1);
  for (int k = 0; k < K; ++k) {
    float wv = bv;
    int wi = bi;
    bm_wave_best(wv, wi);
    const int buf = k & 1;                                           // two buffers: one barrier per round
    if (lane == 0) { red_v[buf][wave] = wv; red_i[buf][wave] = wi; }
    __syncthreads();
    float gv = red_v[buf][0];
    int gi = red_i[buf][0];
    for (int w = 1; w < BM_TOPK_THREADS / 64; ++w)
      if (bm_before(red_v[buf][w], red_i[buf][w], gv, gi)) { gv = red_v[buf][w]; gi = red_i[buf][w]; }
    if (threadIdx.x == 0) { cand_lp[(long)r * K + k] = gv; cand_tok[(long)r * K + k] = gi; }
    if (bi == gi) next_after(gv, gi);                                // indices are unique: the owner of the taken element
  }
}

constexpr int BM_SEL_PER_LANE = (BM_MAX_BEAM * 2 * BM_MAX_BEAM + 63) / 64;   // beam lists of 2 beam candidates over 64 lanes

__global__ __launch_bounds__(256) void beam_select_kernel(const float* __restrict__ cand_lp, const int* __restrict__ cand_tok, int Bs,
                                                          int beam, int V, int step, const int* __restrict__ max_len, int R, double lenpen,
                                                          int eos, float* __restrict__ cum, long* __restrict__ next_tok,
                                                          int* __restrict__ reorder, int* __restrict__ bp_parent, int* __restrict__ bp_token,
                                                          float* __restrict__ bp_cum, int* __restrict__ fin_step, int* __restrict__ fin_row,
                                                          float* __restrict__ fin_score, float* __restrict__ fin_raw,
                                                          int* __restrict__ fin_count, int* __restrict__ finished, int* __restrict__ result) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= Bs || finished[s]) return;                                // the whole wave leaves: no workgroup barrier below
  const int K = 2 * beam, n_lists = step == 0 ? 1 : beam, N = n_lists * K;
  // this lane's candidates: flat candidate c = lane + 64 i of list c / K (beam row), rank c % K in that list
  float sc[BM_SEL_PER_LANE];
  int fl[BM_SEL_PER_LANE];
#pragma unroll
  for (int i = 0; i < BM_SEL_PER_LANE; ++i) {
    const int c = lane + 64 * i;
    sc[i] = -INFINITY;
    fl[i] = 0x7fffffff;
    if (c < N) {
      const int jl = c / K, r = s * beam + jl;
      sc[i] = (step == 0 ? 0.f : cum[r]) + cand_lp[(long)r * K + c % K];
      fl[i] = jl * V + cand_tok[(long)r * K + c % K];
    }
  }
  // K rounds of a wave arg-max over the untaken candidates; lane k keeps the k-th
  float my_sc = -INFINITY;
  int my_fl = 0x7fffffff;
  for (int k = 0; k < K; ++k) {
    float v = -INFINITY;
    int f = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < BM_SEL_PER_LANE; ++i)
      if (bm_before(sc[i], fl[i], v, f)) { v = sc[i]; f = fl[i]; }
    bm_wave_best(v, f);
#pragma unroll
    for (int i = 0; i < BM_SEL_PER_LANE; ++i)
      if (fl[i] == f) { sc[i] = -INFINITY; fl[i] = 0x7fffffff; }      // flat indices are unique
    if (lane == k) { my_sc = v; my_fl = f; }
  }
  const bool have = lane < K;
  const int tok = have ? my_fl % V : -1;
  const int parent = have ? s * beam + my_fl / V : 0;
  const unsigned long long below = (1ull << lane) - 1ull;
  // rule 4: EOS candidates with a finite score among the first beam are finalised while the sentence holds fewer than beam
  const bool eos_fin = have && tok == eos && my_sc > -INFINITY;
  const unsigned long long m_eos = __ballot(eos_fin && lane < beam);
  const int fc = fin_count[s];
  if (eos_fin && lane < beam) {
    const int slot = fc + __popcll(m_eos & below);
    if (slot < beam) {
      const int o = s * beam + slot;
      fin_step[o] = step;
      fin_row[o] = parent;
      fin_raw[o] = my_sc;
      fin_score[o] = my_sc / (float)pow((double)(step + 1), lenpen);
    }
  }
  const int nf = min(beam, fc + (int)__popcll(m_eos));
  const bool done = nf == beam || step >= max_len[s];                // rule 5
  if (lane == 0) {
    fin_count[s] = nf;
    if (done) finished[s] = 1;
    else atomicAdd(&result[0], 1);
  }
  if (done) return;
  // rule 6: the first beam candidates that are not finalisable EOS become the next rows
  const bool elig = have && !eos_fin;
  const unsigned long long m_el = __ballot(elig);
  const int rank = __popcll(m_el & below);
  if (elig && rank < beam) {
    const int r = s * beam + rank;
    reorder[r] = parent;
    next_tok[r] = tok;
    cum[r] = my_sc;
    bp_parent[(long)step * R + r] = parent;
    bp_token[(long)step * R + r] = tok;
    bp_cum[(long)step * R + r] = my_sc;
    if (!(my_sc > -INFINITY) || tok == eos) atomicAdd(&result[1], 1);   // fairseq's cands_to_ignore would have been needed
  }
  if (lane == 0 && __popcll(m_el) < beam) atomicAdd(&result[1], 1);
}

struct BeamLayers {
  const char* kc[SL_REORDER_MAX_LAYERS];
  const char* vc[SL_REORDER_MAX_LAYERS];
  const long* hs[SL_REORDER_MAX_LAYERS];            // null: the layer carries no monotonic step (the transducer's prediction network)
  const unsigned char* hr[SL_REORDER_MAX_LAYERS];   // may be null
  char* kc_o[SL_REORDER_MAX_LAYERS];
  char* vc_o[SL_REORDER_MAX_LAYERS];
  long* hs_o[SL_REORDER_MAX_LAYERS];
  unsigned char* hr_o[SL_REORDER_MAX_LAYERS];
};

// grid (R, n_layers, H): head (r, l, h) of the second set takes positions [0, n_prev) of head (reorder[r], l, h) of the first in
// 16-byte copies, then the payload: the head's monotonic step (and head_read) where the layer has one, and, by workgroup (r, 0, 0),
// the row's int32 of pe_src / pe_dst (the transducer's prev_emit; null: none).  A reorder stays within the `block` rows of r's
// block; the rows of a finished block keep their own payload and copy no K/V.
__global__ __launch_bounds__(256) void beam_reorder_kernel(BeamLayers L, const int* __restrict__ reorder, const int* __restrict__ finished,
                                                           const int* __restrict__ pe_src, int* __restrict__ pe_dst, int R, int block,
                                                           int H, long head_bytes, long prefix_bytes, int* __restrict__ result) {
  const int r = blockIdx.x, l = blockIdx.y, h = blockIdx.z, s = r / block;
  const bool first = l == 0 && h == 0 && threadIdx.x == 0;
  int src = reorder[r];
  bool kv = true;
  if (finished && finished[s]) {                                     // a finished sentence's rows: their K/V are never read again
    src = r;
    kv = false;
  } else if (src < 0 || src >= R || src / block != s) {              // reorders never leave a row's block
    if (first) atomicAdd(result, 1);
    src = r;
  }
  if (kv) {
    const long so = ((long)src * H + h) * head_bytes, dof = ((long)r * H + h) * head_bytes;
    const uint4* ks = reinterpret_cast<const uint4*>(L.kc[l] + so);
    const uint4* vs = reinterpret_cast<const uint4*>(L.vc[l] + so);
    uint4* kd = reinterpret_cast<uint4*>(L.kc_o[l] + dof);
    uint4* vd = reinterpret_cast<uint4*>(L.vc_o[l] + dof);
    for (long i = threadIdx.x; i < (prefix_bytes >> 4); i += 256) { kd[i] = ks[i]; vd[i] = vs[i]; }
  }
  if (threadIdx.x == 0) {
    if (L.hs[l]) {
      L.hs_o[l][r * H + h] = L.hs[l][src * H + h];
      if (L.hr[l]) L.hr_o[l][r * H + h] = L.hr[l][src * H + h];
    }
    if (first && pe_dst) pe_dst[r] = pe_src[src];
  }
}

__global__ __launch_bounds__(256) void beam_backtrack_kernel(int Bs, int beam, int nbest, int Lr, int R, const int* __restrict__ bp_parent,
                                                             const int* __restrict__ bp_token, const float* __restrict__ bp_cum,
                                                             const int* __restrict__ fin_step, const int* __restrict__ fin_row,
                                                             const float* __restrict__ fin_score, const float* __restrict__ fin_raw,
                                                             const int* __restrict__ fin_count, int pad, int eos, long* __restrict__ tokens,
                                                             int* __restrict__ lengths, float* __restrict__ scores,
                                                             float* __restrict__ pos_scores) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= Bs) return;
  const int cnt = min(max(fin_count[s], 0), beam);
  // rule 7: rank by descending score, equal scores keep finalisation order
  if (lane < cnt) {
    const float me = fin_score[s * beam + lane];
    int rank = 0;
    for (int k = 0; k < cnt; ++k) {
      const float o = fin_score[s * beam + k];
      rank += (o > me || (o == me && k < lane)) ? 1 : 0;
    }
    if (rank < nbest) {
      const long o = (long)s * nbest + rank;
      long* tk = tokens + o * Lr;
      float* ps = pos_scores + o * Lr;
      const int t = min(max(fin_step[s * beam + lane], 0), Lr - 1);
      int row = min(max(fin_row[s * beam + lane], 0), R - 1);
      tk[t] = eos;
      ps[t] = fin_raw[s * beam + lane] - (t > 0 ? bp_cum[(long)(t - 1) * R + row] : 0.f);
      for (int p = t - 1; p >= 0; --p) {
        const long e = (long)p * R + row;
        const int par = min(max(bp_parent[e], 0), R - 1);
        tk[p] = bp_token[e];
        ps[p] = bp_cum[e] - (p > 0 ? bp_cum[(long)(p - 1) * R + par] : 0.f);
        row = par;
      }
      for (int p = t + 1; p < Lr; ++p) { tk[p] = pad; ps[p] = 0.f; }
      lengths[o] = t + 1;
      scores[o] = fin_score[s * beam + lane];
    }
  }
  // output slots no hypothesis reached (a sentence that was not decoded to its end)
  for (int q = cnt + lane; q < nbest; q += 64) {
    const long o = (long)s * nbest + q;
    for (int p = 0; p < Lr; ++p) { tokens[o * Lr + p] = pad; pos_scores[o * Lr + p] = 0.f; }
    lengths[o] = 0;
    scores[o] = -INFINITY;
  }
}

}  // namespace

#define BM_CHECK_BEAM(h, beam, V, what)                                                                                  \
  SL_REQUIRE(h, (beam) >= 1 && (beam) <= BM_MAX_BEAM, SIMULST_E_SHAPE, what ": beam must be in [1, 16]");               \
  SL_REQUIRE(h, 2 * (beam) <= (V) - 1 && (V) <= (1 << 26), SIMULST_E_SHAPE, what ": 2 beam <= V - 1 (V <= 2^26)")

extern "C" int simulst_beam_topk(simulst_handle* h, const float* logits, int32_t R, int32_t V, int32_t beam, int32_t step,
                                 const int32_t* max_len, const int32_t* finished, int32_t pad_idx, int32_t eos_idx, float* cand_lp,
                                 int32_t* cand_tok) {
  if (!h) return SIMULST_E_NULL;
  SL_CHECK_NULL(h, logits); SL_CHECK_NULL(h, max_len); SL_CHECK_NULL(h, cand_lp); SL_CHECK_NULL(h, cand_tok);
  BM_CHECK_BEAM(h, beam, V, "simulst_beam_topk");
  SL_REQUIRE(h, R > 0 && R % beam == 0, SIMULST_E_SHAPE, "simulst_beam_topk: rows R a positive multiple of beam");
  SL_REQUIRE(h, step >= 0, SIMULST_E_SHAPE, "simulst_beam_topk: step");
  KTimer t(h, SIMULST_K_MISC);
  if (V % 4 == 0 && ((uintptr_t)logits & 15) == 0)
    hipLaunchKernelGGL(beam_topk_kernel<true>, dim3(R), dim3(BM_TOPK_THREADS), 0, h->stream, logits, V, beam, step, (const int*)max_len,
                       (const int*)finished, pad_idx, eos_idx, cand_lp, (int*)cand_tok);
  else
    hipLaunchKernelGGL(beam_topk_kernel<false>, dim3(R), dim3(BM_TOPK_THREADS), 0, h->stream, logits, V, beam, step, (const int*)max_len,
                       (const int*)finished, pad_idx, eos_idx, cand_lp, (int*)cand_tok);
  return sl_launch_status(h, "simulst_beam_topk");
}

extern "C" int simulst_beam_select(simulst_handle* h, const float* cand_lp, const int32_t* cand_tok, int32_t Bs, int32_t beam, int32_t V,
                                   int32_t step, const int32_t* max_len, int32_t L, double lenpen, int32_t eos_idx, float* cum,
                                   int64_t* next_tok, int32_t* reorder, int32_t* bp_parent, int32_t* bp_token, float* bp_cum,
                                   int32_t* fin_step, int32_t* fin_row, float* fin_score, float* fin_raw, int32_t* fin_count,
                                   int32_t* finished, int32_t* result) {
  if (!h) return SIMULST_E_NULL;
  SL_CHECK_NULL(h, cand_lp); SL_CHECK_NULL(h, cand_tok); SL_CHECK_NULL(h, max_len); SL_CHECK_NULL(h, cum); SL_CHECK_NULL(h, next_tok);
  SL_CHECK_NULL(h, reorder); SL_CHECK_NULL(h, bp_parent); SL_CHECK_NULL(h, bp_token); SL_CHECK_NULL(h, bp_cum);
  SL_CHECK_NULL(h, fin_step); SL_CHECK_NULL(h, fin_row); SL_CHECK_NULL(h, fin_score); SL_CHECK_NULL(h, fin_raw);
  SL_CHECK_NULL(h, fin_count); SL_CHECK_NULL(h, finished); SL_CHECK_NULL(h, result);
  BM_CHECK_BEAM(h, beam, V, "simulst_beam_select");
  SL_REQUIRE(h, Bs > 0 && (long)Bs * beam <= (1 << 24), SIMULST_E_SHAPE, "simulst_beam_select: sentences Bs");
  SL_REQUIRE(h, step >= 0 && step < L, SIMULST_E_SHAPE, "simulst_beam_select: 0 <= step < L (rows of the back-pointer tables)");
  SL_REQUIRE(h, isfinite(lenpen), SIMULST_E_SHAPE, "simulst_beam_select: lenpen");
  KTimer t(h, SIMULST_K_MISC);
  if (hipMemsetAsync(result, 0, sizeof(int32_t), h->stream) != hipSuccess) {
    h->err = "simulst_beam_select: clearing the unfinished count failed";
    return SIMULST_E_SHAPE;
  }
  hipLaunchKernelGGL(beam_select_kernel, dim3((Bs + 3) / 4), dim3(256), 0, h->stream, cand_lp, (const int*)cand_tok, Bs, beam, V, step,
                     (const int*)max_len, Bs * beam, lenpen, eos_idx, cum, (long*)next_tok, (int*)reorder, (int*)bp_parent, (int*)bp_token,
                     bp_cum, (int*)fin_step, (int*)fin_row, fin_score, fin_raw, (int*)fin_count, (int*)finished, (int*)result);
  return sl_launch_status(h, "simulst_beam_select");
}

// The launch behind simulst_beam_reorder and simulst_transducer_beam_reorder, whose refusals have passed: every layer's K/V pointers
// are set, head_step in all layers of both sets or (head_step false) read in none, pe_src / pe_dst both set or both null.
int sl_beam_reorder(simulst_handle* h, const char* who, const simulst_dec_layer* src, const simulst_dec_layer* dst, bool head_step,
                    const int32_t* pe_src, int32_t* pe_dst, const int32_t* reorder, const int32_t* finished, int32_t* result, int R,
                    int block, int n_layers, int H, int head_dim, int dtype, int cap, int n_prev) {
  BeamLayers L = {};
  for (int l = 0; l < n_layers; ++l) {
    L.kc[l] = (const char*)src[l].k_cache; L.vc[l] = (const char*)src[l].v_cache;
    L.kc_o[l] = (char*)dst[l].k_cache; L.vc_o[l] = (char*)dst[l].v_cache;
    if (head_step) {
      L.hs[l] = (const long*)src[l].head_step; L.hr[l] = src[l].head_read;
      L.hs_o[l] = (long*)dst[l].head_step; L.hr_o[l] = dst[l].head_read;
    }
  }
  const long pos_bytes = (long)head_dim * (dtype == SIMULST_F32 ? 4 : 2);     // one position of one head: a multiple of 16 bytes
  KTimer t(h, SIMULST_K_MISC);
  hipLaunchKernelGGL(beam_reorder_kernel, dim3(R, n_layers, H), dim3(256), 0, h->stream, L, (const int*)reorder, (const int*)finished,
                     (const int*)pe_src, (int*)pe_dst, R, block, H, (long)cap * pos_bytes, (long)n_prev * pos_bytes, (int*)result);
  return sl_launch_status(h, who);
}

extern "C" int simulst_beam_reorder(simulst_handle* h, const simulst_decoder_desc* dd, const simulst_dec_layer* src,
                                    const simulst_dec_layer* dst, const int32_t* reorder, const int32_t* finished, int32_t beam,
                                    int32_t n_prev, int32_t* result) {
  if (!h) return SIMULST_E_NULL;
  SL_CHECK_NULL(h, dd); SL_CHECK_NULL(h, src); SL_CHECK_NULL(h, dst); SL_CHECK_NULL(h, reorder); SL_CHECK_NULL(h, result);
  SL_REQUIRE(h, beam >= 1 && beam <= BM_MAX_BEAM, SIMULST_E_SHAPE, "simulst_beam_reorder: beam must be in [1, 16]");
  SL_REQUIRE(h, dd->B > 0 && dd->B % beam == 0, SIMULST_E_SHAPE, "simulst_beam_reorder: rows B a positive multiple of beam");
  SL_REQUIRE(h, dd->dtype == SIMULST_F32 || dd->dtype == SIMULST_BF16, SIMULST_E_DTYPE, "simulst_beam_reorder: dtype");
  SL_REQUIRE(h, dd->n_layers > 0 && dd->n_layers <= SL_REORDER_MAX_LAYERS && dd->H > 0 && dd->D % dd->H == 0 &&
                (dd->D / dd->H) % 8 == 0 && dd->cap > 0,
             SIMULST_E_SHAPE, "simulst_beam_reorder: shape (at most 16 layers, head_dim a multiple of 8)");
  SL_REQUIRE(h, n_prev >= 0 && n_prev <= dd->cap, SIMULST_E_SHAPE, "simulst_beam_reorder: 0 <= n_prev <= cap");
  for (int l = 0; l < dd->n_layers; ++l) {
    SL_CHECK_NULL(h, src[l].k_cache); SL_CHECK_NULL(h, src[l].v_cache); SL_CHECK_NULL(h, src[l].head_step);
    SL_CHECK_NULL(h, dst[l].k_cache); SL_CHECK_NULL(h, dst[l].v_cache); SL_CHECK_NULL(h, dst[l].head_step);
    SL_REQUIRE(h, !src[l].head_read == !dst[l].head_read, SIMULST_E_SHAPE, "simulst_beam_reorder: head_read in both sets or in neither");
  }
  return sl_beam_reorder(h, "simulst_beam_reorder", src, dst, true, nullptr, nullptr, reorder, finished, result, dd->B, beam,
                         dd->n_layers, dd->H, dd->D / dd->H, dd->dtype, dd->cap, n_prev);
}

extern "C" int simulst_beam_backtrack(simulst_handle* h, int32_t Bs, int32_t beam, int32_t nbest, int32_t L, const int32_t* bp_parent,
                                      const int32_t* bp_token, const float* bp_cum, const int32_t* fin_step, const int32_t* fin_row,
                                      const float* fin_score, const float* fin_raw, const int32_t* fin_count, int32_t pad_idx,
                                      int32_t eos_idx, int64_t* tokens, int32_t* lengths, float* scores, float* pos_scores) {
  if (!h) return SIMULST_E_NULL;
  SL_CHECK_NULL(h, bp_parent); SL_CHECK_NULL(h, bp_token); SL_CHECK_NULL(h, bp_cum); SL_CHECK_NULL(h, fin_step);
  SL_CHECK_NULL(h, fin_row); SL_CHECK_NULL(h, fin_score); SL_CHECK_NULL(h, fin_raw); SL_CHECK_NULL(h, fin_count);
  SL_CHECK_NULL(h, tokens); SL_CHECK_NULL(h, lengths); SL_CHECK_NULL(h, scores); SL_CHECK_NULL(h, pos_scores);
  SL_REQUIRE(h, beam >= 1 && beam <= BM_MAX_BEAM, SIMULST_E_SHAPE, "simulst_beam_backtrack: beam must be in [1, 16]");
  SL_REQUIRE(h, nbest >= 1 && nbest <= beam, SIMULST_E_SHAPE, "simulst_beam_backtrack: 1 <= nbest <= beam");
  SL_REQUIRE(h, Bs > 0 && (long)Bs * beam <= (1 << 24), SIMULST_E_SHAPE, "simulst_beam_backtrack: sentences Bs");
  SL_REQUIRE(h, L > 0, SIMULST_E_SHAPE, "simulst_beam_backtrack: L (rows of the back-pointer tables)");
  KTimer t(h, SIMULST_K_MISC);
  hipLaunchKernelGGL(beam_backtrack_kernel, dim3((Bs + 3) / 4), dim3(256), 0, h->stream, Bs, beam, nbest, L, Bs * beam,
                     (const int*)bp_parent, (const int*)bp_token, bp_cum, (const int*)fin_step, (const int*)fin_row, fin_score, fin_raw,
                     (const int*)fin_count, pad_idx, eos_idx, (long*)tokens, (int*)lengths, scores, pos_scores);
  return sl_launch_status(h, "simulst_beam_backtrack");
}
