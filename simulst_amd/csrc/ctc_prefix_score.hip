// CTC prefix scores inside the attention beam search (joint CTC / attention decoding) for gfx950 --
// simulst_ctc_prefix_score (include/simulst_hip.h; DESIGN.md "Beam search", "CTC prefix scores inside the beam").
//
// ctc_prefix_score_kernel, once per beam step: ONE wave per beam row r = s * G + j, ONE lane per candidate (K <= 32).  Lane k extends
// the row's hypothesis g by its candidate c and runs the prefix-score recursion over the sentence's frames, serially, in fp32:
//   gn'[t] = (gn'[t-1] (+) phi[t-1]) + x[t][c]     gb'[t] = (gn'[t-1] (+) gb'[t-1]) + x[t][blank]     psi (+)= phi[t-1] + x[t][c]
// with phi[t] = gb[t] if c repeats g's last label, else gn[t] (+) gb[t] of the row's own state.  What a frame reads -- x[t][c] of
// every lane, the blank, gb[t] and gn[t] (+) gb[t] -- is staged in LDS PS_FB frames at a time: the next block's global loads go out
// before the staged block is worked through and are stored to LDS behind it, so that no load is inside the dependent chain (the
// log-add of the row's own state is taken at staging, by the lane that loaded the frame).  A lane's arithmetic reads nothing of the
// other lanes, so a candidate's result is the same bits in every slot and row.  Behind the recursion the wave forms the combined
// scores and puts the row's list back into candidate order (descending score, equal scores to the lower token) by ranking.
//
// ctc_prefix_commit_kernel, behind simulst_beam_select: row r takes the state and psi of candidate next_tok[r] of its parent row
// reorder[r] into the second state set.
#include <math.h>

#include "common.h"

namespace {

constexpr int PS_KMAX = 32;                          // candidates of a row: one lane each
constexpr int PS_FB = 32;                            // frames staged at a time
constexpr int PS_PER_LANE = PS_FB * PS_KMAX / 64;
constexpr float PS_FLOOR = -1.0e4f;                  // the CTC term of an extension no alignment spells

struct ps_shared {
  float x[PS_FB * PS_KMAX];                          // [frame][candidate], K floats a frame
  float gb[PS_FB], tot[PS_FB], xb[PS_FB];            // the row's gb[t], gn[t] (+) gb[t] and the blank's log-probability
};

// a before b in candidate order; the slot decides between equal tokens, which a caller's list does not hold, so that the ranks are a
// permutation whatever the list
__device__ __forceinline__ bool ps_before(float va, int ta, int ka, float vb, int tb, int kb) {
  return va > vb || (va == vb && (ta < tb || (ta == tb && ka < kb)));
}

__global__ __launch_bounds__(64) void ctc_prefix_score_kernel(const float* __restrict__ lp, long lp_t, long lp_b, long lp_v,
                                                              const float* __restrict__ blank_lp, long bl_b,
                                                              const float* __restrict__ state, const float* __restrict__ psi,
                                                              const long* __restrict__ last, const long* __restrict__ plen,
                                                              const long* __restrict__ in_len, const int* __restrict__ finished, int S,
                                                              int G, int K, int blank, int eos, int pad, float weight, int first_only,
                                                              float* __restrict__ cand_state, float* __restrict__ cand_psi,
                                                              float* __restrict__ cand_lp, int* __restrict__ cand_tok,
                                                              int* __restrict__ cand_slot) {
  __shared__ ps_shared sh;
  const int r = blockIdx.x, lane = threadIdx.x;
  const int s = r / G, j = r - s * G;
  if ((finished && finished[s]) || (first_only && j > 0)) return;    // the row's buffers stay as they are
  const long n_in = in_len[r];
  const int T = (int)(n_in < 0 ? 0 : (n_in < (long)S ? n_in : (long)S));
  const bool own = lane < K;
  const bool empty = plen[r] <= 0;
  const int e = (int)last[r];
  const int tok = own ? cand_tok[(long)r * K + lane] : -1;
  const float lp_att = own ? cand_lp[(long)r * K + lane] : -INFINITY;
  const bool special = tok < 0 || tok == blank || tok == pad;
  const bool ext = own && !special && tok != eos;                    // the candidate extends the hypothesis by a label
  const bool same = ext && !empty && tok == e;
  const float* lpr = lp + (long)s * lp_b + (long)j * K * lp_v;
  const float2* str = reinterpret_cast<const float2*>(state) + (long)r * S;
  const float* blr = blank_lp + (long)s * bl_b;
  float2* out = reinterpret_cast<float2*>(cand_state) + (long)r * S * K;

  float rx[PS_PER_LANE];
  float2 rst = make_float2(-INFINITY, -INFINITY);
  float rxb = 0.f;
  auto prefetch = [&](int t0) {
#pragma unroll
    for (int u = 0; u < PS_PER_LANE; ++u) {
      const int idx = lane + 64 * u;
      const int f = idx / K, k = idx - f * K;
      rx[u] = -INFINITY;
      if (f < PS_FB && t0 + f < T) rx[u] = lpr[(long)(t0 + f) * lp_t + (long)k * lp_v];
    }
    if (lane < PS_FB && t0 + lane < T) { rst = str[t0 + lane]; rxb = blr[t0 + lane]; }
  };
  prefetch(0);

  float pn = -INFINITY, pb = -INFINITY, acc = -INFINITY;
  float phi = empty ? 0.f : -INFINITY;                               // phi[-1]
  for (int t0 = 0; t0 < T; t0 += PS_FB) {
    // the block loaded one block ago -> LDS (every lane is past the previous block: the barrier at its end)
#pragma unroll
    for (int u = 0; u < PS_PER_LANE; ++u) {
      const int idx = lane + 64 * u;
      if (idx < PS_FB * K) sh.x[idx] = rx[u];
    }
    if (lane < PS_FB) { sh.gb[lane] = rst.y; sh.tot[lane] = lae(rst.x, rst.y); sh.xb[lane] = rxb; }
    __syncthreads();
    if (t0 + PS_FB < T) prefetch(t0 + PS_FB);
    const int t1 = T - t0 < PS_FB ? T - t0 : PS_FB;
    for (int f = 0; f < t1; ++f) {
      const float x = ext ? sh.x[f * K + lane] : -INFINITY;
      const float gn = lae(pn, phi) + x;
      const float gb = lae(pn, pb) + sh.xb[f];
      acc = lae(acc, phi + x);
      if (own) out[(long)(t0 + f) * K + lane] = make_float2(gn, gb);
      phi = same ? sh.gb[f] : sh.tot[f];
      pn = gn;
      pb = gb;
    }
    __syncthreads();
  }
  if (!own) return;
  // psi of the extended string; of the hypothesis ended here for the EOS candidate
  float psi_h = -INFINITY;
  if (ext) psi_h = acc;
  else if (!special && tok == eos) {
    if (T > 0) { const float2 st = str[T - 1]; psi_h = lae(st.x, st.y); }
    else psi_h = empty ? 0.f : -INFINITY;
  }
  cand_psi[(long)r * K + lane] = psi_h;
  float d = PS_FLOOR;
  if (psi_h > -INFINITY) d = fmaxf(psi_h - psi[r], PS_FLOOR);
  float sc = lp_att;
  if (weight != 0.f && lp_att != -INFINITY) sc = (1.f - weight) * lp_att + weight * d;
  // candidate order again: this lane's rank among the row's K
  int rank = 0;
  for (int q = 0; q < K; ++q) {
    const float oq = __shfl(sc, q, 64);
    const int tq = __shfl(tok, q, 64);
    rank += ps_before(oq, tq, q, sc, tok, lane) ? 1 : 0;
  }
  cand_lp[(long)r * K + rank] = sc;
  cand_tok[(long)r * K + rank] = tok;
  cand_slot[(long)r * K + rank] = lane;
}

__global__ __launch_bounds__(64) void ctc_prefix_commit_kernel(const float* __restrict__ cand_state, const float* __restrict__ cand_psi,
                                                               const int* __restrict__ cand_tok, const int* __restrict__ cand_slot,
                                                               const long* __restrict__ next_tok, const int* __restrict__ reorder,
                                                               const int* __restrict__ finished, const long* __restrict__ plen,
                                                               const long* __restrict__ in_len, int S, int N, int G, int K,
                                                               float* __restrict__ state_out, float* __restrict__ psi_out,
                                                               long* __restrict__ last_out, long* __restrict__ len_out,
                                                               int* __restrict__ result) {
  const int r = blockIdx.x, lane = threadIdx.x, s = r / G;
  if (finished && finished[s]) return;
  const int p = reorder[r];
  const long tok = next_tok[r];
  int slot = -1;
  if (p >= 0 && p < N && p / G == s) {                               // (uniform) a parent of the row's own sentence
    const bool hit = lane < K && (long)cand_tok[(long)p * K + lane] == tok;
    const unsigned long long m = __ballot(hit);
    if (m) slot = cand_slot[(long)p * K + __builtin_ctzll(m)];
  }
  if (slot < 0 || slot >= K) {                                       // not among the parent's candidates: counted, the row stays
    if (lane == 0) atomicAdd(result, 1);
    return;
  }
  const long n_in = in_len[p];
  const int T = (int)(n_in < 0 ? 0 : (n_in < (long)S ? n_in : (long)S));
  const float2* from = reinterpret_cast<const float2*>(cand_state) + (long)p * S * K + slot;
  float2* to = reinterpret_cast<float2*>(state_out) + (long)r * S;
  for (int t = lane; t < T; t += 64) to[t] = from[(long)t * K];
  if (lane == 0) {
    psi_out[r] = cand_psi[(long)p * K + slot];
    last_out[r] = tok;
    len_out[r] = (plen[p] < 0 ? 0 : plen[p]) + 1;
  }
}

}  // namespace

extern "C" int simulst_ctc_prefix_score(simulst_handle* h, const float* cand_log_probs, int64_t lp_stride_t, int64_t lp_stride_b,
                                        int64_t lp_stride_v, const int64_t* last_labels, const int64_t* input_lengths,
                                        const int64_t* prefix_lengths, int32_t S, int32_t N, int32_t K, int32_t blank,
                                        const simulst_ctc_score_desc* desc) {
  if (!h) return SIMULST_E_NULL;
  SL_CHECK_NULL(h, desc);
  const simulst_ctc_score_desc* d = desc;
  SL_CHECK_NULL(h, prefix_lengths); SL_CHECK_NULL(h, input_lengths);
  SL_CHECK_NULL(h, d->cand_state); SL_CHECK_NULL(h, d->cand_psi); SL_CHECK_NULL(h, d->cand_tok); SL_CHECK_NULL(h, d->cand_slot);
  SL_REQUIRE(h, d->op == 0 || d->op == 1, SIMULST_E_SHAPE, "simulst_ctc_prefix_score: op is 0 (score) or 1 (commit)");
  if (d->op == 0) {
    SL_CHECK_NULL(h, last_labels); SL_CHECK_NULL(h, cand_log_probs); SL_CHECK_NULL(h, d->blank_lp); SL_CHECK_NULL(h, d->state);
    SL_CHECK_NULL(h, d->psi); SL_CHECK_NULL(h, d->cand_lp);
  } else {
    SL_CHECK_NULL(h, d->next_tok); SL_CHECK_NULL(h, d->reorder); SL_CHECK_NULL(h, d->state_out); SL_CHECK_NULL(h, d->psi_out);
    SL_CHECK_NULL(h, d->last_out); SL_CHECK_NULL(h, d->len_out); SL_CHECK_NULL(h, d->result);
  }
  SL_REQUIRE(h, K >= 1 && K <= PS_KMAX, SIMULST_E_SHAPE, "simulst_ctc_prefix_score: K is 1..32");
  SL_REQUIRE(h, d->G >= 1, SIMULST_E_SHAPE, "simulst_ctc_prefix_score: G >= 1");
  SL_REQUIRE(h, S > 0 && blank >= 0, SIMULST_E_SHAPE, "simulst_ctc_prefix_score: shape");
  if (N <= 0) return SIMULST_OK;
  SL_REQUIRE(h, N % d->G == 0, SIMULST_E_SHAPE, "simulst_ctc_prefix_score: N rows a multiple of G");
  KTimer t(h, SIMULST_K_SCAN);
  if (d->op == 0)
    hipLaunchKernelGGL(ctc_prefix_score_kernel, dim3(N), dim3(64), 0, h->stream, cand_log_probs, (long)lp_stride_t, (long)lp_stride_b,
                       (long)lp_stride_v, d->blank_lp, (long)d->blank_stride_b, d->state, d->psi, (const long*)last_labels,
                       (const long*)prefix_lengths, (const long*)input_lengths, (const int*)d->finished, S, d->G, K, blank, d->eos,
                       d->pad, d->weight, d->first_only, d->cand_state, d->cand_psi, d->cand_lp, (int*)d->cand_tok, (int*)d->cand_slot);
  else
    hipLaunchKernelGGL(ctc_prefix_commit_kernel, dim3(N), dim3(64), 0, h->stream, d->cand_state, d->cand_psi, (const int*)d->cand_tok,
                       (const int*)d->cand_slot, (const long*)d->next_tok, (const int*)d->reorder, (const int*)d->finished,
                       (const long*)prefix_lengths, (const long*)input_lengths, S, N, d->G, K, d->state_out, d->psi_out,
                       (long*)d->last_out, (long*)d->len_out, (int*)d->result);
  return sl_launch_status(h, "simulst_ctc_prefix_score");
}
