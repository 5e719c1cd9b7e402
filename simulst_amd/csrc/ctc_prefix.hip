// CTC prefix beam search for gfx950: every frame of the time-synchronous recursion of simulst_amd/ctc.py ctc_prefix_beam_advance for a
// batch in ONE launch -- simulst_ctc_prefix_beam (include/simulst_hip.h).
//
// One workgroup of ONE wave per utterance: a frame is a chain of small dependent steps over at most 16 prefixes and 16 + 16 * 8 = 144
// pool entries, so a second wave would only add barriers.  The wave keeps
//   * the beam's strings in LDS as int32, two buffers [2][beam][cap4] (cap4 = cap rounded up to 4): the survivors of a frame are
//     copied from one into the other, 16 bytes a lane, lanes (slot, quarter); loaded from the int64 state at entry, written back with
//     `pad` behind each length at exit.  That is the capacity limit: 2 * beam * cap4 * 4 <= SIMULST_CTC_PREFIX_STRING_BYTES
//   * lengths, p_b, p_nb, the last label, a hash and the parent slot of prefix i in lane i, mirrored in small LDS arrays for the
//     lanes that hold the extensions (pool entry idx in lane idx % 64, register idx / 64)
//   * the candidates of PB_FB frames in LDS; the next PB_FB frames are loaded into registers BEFORE the staged ones are worked
//     through and stored to LDS after them, so that no frame waits for a global load
// Selection: beam rounds of a DPP wave maximum over the pool scores; the winner is the first (register, lane) holding the maximum,
// which is the lowest pool index -- the stable descending sort of the torch form.
//
// Prefix identity ("extension (i, c) spells beam entry i2") is exact.  Lane i2 keeps par = the slot of the entry that spells its
// string without the last label, or -1.  A relation enters this cache in two ways only: by construction (i2 was made as i + c in this
// call and both survived), or by COMPARING THE LABELS: whenever an entry without a known parent and a new entry (one the cache has
// not been checked against: every entry at the start of a call, the grown survivors after a frame) meet, an additive position-keyed
// hash and the lengths filter the pairs, and a hit is confirmed label by label across the wave.  The hash never decides.  A parent that
// left the beam and re-enters as a fresh extension is a new entry, so it is compared with its orphaned child in the frame it
// arrives.  The cache is rebuilt from the strings at every call: it cannot make the result depend on how frames are cut into calls.
#include <math.h>

#include "common.h"

namespace {

constexpr int PB_BEAM = 16, PB_K = 8, PB_POOL = PB_BEAM + PB_BEAM * PB_K;      // 144 pool entries: 3 registers a lane
constexpr int PB_FB = 32;                                                      // frames of candidates staged at a time
constexpr int PB_STAGE = PB_FB * (PB_K + 1);
constexpr int PB_PER_LANE = (PB_STAGE + 63) / 64;
constexpr int PB_STATIC_LDS = 6144;                                            // bound on the static arrays below (checked)

__device__ __forceinline__ unsigned mix(int pos, int label) {
  unsigned x = ((unsigned)(pos + 1) * 0x9E3779B1u) ^ (((unsigned)label + 0x7F4A7C15u) * 0x85EBCA6Bu);
  x ^= x >> 15; x *= 0x2C1B3C6Du; x ^= x >> 13;
  return x;
}

// maximum over the wave in every lane: the row-shift / row-broadcast ladder of wave_scan_incl_dpp with max in place of add (lanes
// without a source keep their own value), lane 63 read back as a scalar
__device__ __forceinline__ float wave_max_dpp(float v) {
#define PB_DPP_MAX(ctrl, row_mask)                                                                                    \
  v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, v), __builtin_bit_cast(int, v), ctrl, \
                                                                     row_mask, 0xf, false)))
  PB_DPP_MAX(0x111, 0xf);
  PB_DPP_MAX(0x112, 0xf);
  PB_DPP_MAX(0x114, 0xf);
  PB_DPP_MAX(0x118, 0xf);
  PB_DPP_MAX(0x142, 0xa);
  PB_DPP_MAX(0x143, 0xc);
#undef PB_DPP_MAX
  return wave_last(v);
}

struct pb_shared {
  int c_id[PB_STAGE];
  float c_lp[PB_STAGE];
  float pool_b[PB_POOL], pool_nb[PB_POOL];
  unsigned char tab_i[PB_POOL], tab_j[PB_POOL];        // pool index -> (prefix, candidate)
  int removed[PB_BEAM * PB_K];                         // extension (i, j) was added to a beam entry
  float pb[PB_BEAM], tot[PB_BEAM];
  int e[PB_BEAM], len[PB_BEAM], par[PB_BEAM], newslot[PB_BEAM], src[PB_BEAM];
  unsigned h[PB_BEAM], hp[PB_BEAM];
};
static_assert(sizeof(pb_shared) <= PB_STATIC_LDS, "static LDS of the prefix beam kernel");

__global__ __launch_bounds__(64) void ctc_prefix_kernel(const float* __restrict__ lp, long lp_t, long lp_b, long lp_v,
                                                        const int* __restrict__ ids, long id_b, long id_t,
                                                        const long* __restrict__ in_len, int S, int beam, int k, int cap, int pad,
                                                        long* __restrict__ strings, long* __restrict__ lengths,
                                                        float* __restrict__ p_b, float* __restrict__ p_nb) {
  extern __shared__ __align__(16) int pb_str[];                           // [2][beam][cap4]
  __shared__ pb_shared sh;
  const int b = blockIdx.x, lane = threadIdx.x;
  const long n_in = in_len[b];
  const int L = (int)(n_in < (long)S ? n_in : (long)S);
  if (L <= 0) return;                                        // no frame to take: the state stays as it is, bit for bit
  const int kp = k + 1, P = beam + beam * k;
  const int cap4 = (cap + 3) & ~3;
  int* cur = pb_str;
  int* nxt = pb_str + beam * cap4;
  long* gs = strings + (long)b * beam * cap;
  const int* idb = ids + (long)b * id_b;
  const float* lpb = lp + (long)b * lp_b;
  const bool own = lane < beam;                              // lane i holds prefix i

  // ---- candidates: the first block's loads go out before anything else
  int rid[PB_PER_LANE];
  float rlp[PB_PER_LANE];
  auto prefetch = [&](int t0) {
#pragma unroll
    for (int u = 0; u < PB_PER_LANE; ++u) {
      const int x = lane + 64 * u;
      const int f = x / kp, j = x - f * kp;
      rid[u] = -1; rlp[u] = -INFINITY;
      if (f < PB_FB && t0 + f < L) {
        rid[u] = idb[(long)(t0 + f) * id_t + j];
        rlp[u] = lpb[(long)(t0 + f) * lp_t + (long)j * lp_v];
      }
    }
  };
  prefetch(0);

  // ---- the state: scalars into lane i, strings into LDS
  float pb = -INFINITY, pnb = -INFINITY;
  int len = 0;
  if (own) {
    pb = p_b[(long)b * beam + lane];
    pnb = p_nb[(long)b * beam + lane];
    len = (int)lengths[(long)b * beam + lane];
    len = len < 0 ? 0 : (len > cap ? cap : len);
    sh.len[lane] = len;
    sh.par[lane] = -1;
  }
  for (int idx = lane; idx < P; idx += 64) {
    const int q = idx - beam;
    sh.tab_i[idx] = (unsigned char)(idx < beam ? idx : q / k);
    sh.tab_j[idx] = (unsigned char)(idx < beam ? 0 : q % k);
  }
  __syncthreads();
  int maxlen = 0;                                            // upper bound of the beam's lengths (uniform)
  for (int s = 0; s < beam; ++s) {
    const int ls = sh.len[s];
    maxlen = ls > maxlen ? ls : maxlen;
    for (int p = lane; p < ls; p += 64) cur[s * cap4 + p] = (int)gs[(long)s * cap + p];
  }
  __syncthreads();
  const int slot4 = lane >> 2, sub = lane & 3;               // the (slot, quarter) layout of the copy and of the hash at entry
  {
    unsigned acc = 0;
    if (slot4 < beam) {
      const int ls = sh.len[slot4];
      for (int p = sub; p < ls; p += 4) acc += mix(p, cur[slot4 * cap4 + p]);
    }
    acc += (unsigned)__shfl_xor((int)acc, 1, 64);
    acc += (unsigned)__shfl_xor((int)acc, 2, 64);
    if (slot4 < beam && sub == 0) sh.h[slot4] = acc;
  }
  __syncthreads();
  int e = -2, par = -1;
  unsigned h = 0, hp = 0;
  bool live = false;
  if (own) {
    h = sh.h[lane];
    if (len > 0) { e = cur[lane * cap4 + len - 1]; hp = h - mix(len - 1, e); }
    sh.hp[lane] = hp;
    live = lae(pb, pnb) > -INFINITY;
  }
  unsigned long long fresh = __ballot(own && live);          // entries the parent cache has not been checked against

  // pool entries of this lane: idx = lane + 64 r
  int pi[3], pj[3];
  bool ext_valid[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int idx = lane + 64 * r;
    ext_valid[r] = idx >= beam && idx < P;
    pi[r] = ext_valid[r] ? sh.tab_i[idx] : 0;
    pj[r] = ext_valid[r] ? sh.tab_j[idx] : 0;
  }

  for (int t0 = 0; t0 < L; t0 += PB_FB) {
    // the block loaded one block ago -> LDS (every lane is past the previous block: the barrier at the end of its last frame)
#pragma unroll
    for (int u = 0; u < PB_PER_LANE; ++u) {
      const int x = lane + 64 * u;
      if (x < PB_FB * kp) { sh.c_id[x] = rid[u]; sh.c_lp[x] = rlp[u]; }
    }
    __syncthreads();
    if (t0 + PB_FB < L) prefetch(t0 + PB_FB);
    const int t1 = L - t0 < PB_FB ? L - t0 : PB_FB;
    for (int f = 0; f < t1; ++f) {
      const int base = f * kp;
      // ---- entries without a known parent against the new entries: hash and length filter, labels decide
      {
        bool orphan = own && live && len > 0 && par < 0;
        if (fresh && __ballot(orphan)) {
          for (unsigned long long fr = fresh; fr; fr &= fr - 1) {
            const int i = __builtin_ctzll(fr);
            const int li = sh.len[i];
            const unsigned hi = sh.h[i];
            unsigned long long hits = __ballot(orphan && len == li + 1 && hp == hi);
            for (; hits; hits &= hits - 1) {
              const int i2 = __builtin_ctzll(hits);
              bool diff = false;
              for (int p = lane; p < li; p += 64) diff |= cur[i * cap4 + p] != cur[i2 * cap4 + p];
              if (!__ballot(diff) && lane == i2) { par = i; orphan = false; }
            }
          }
        }
        fresh = 0;
      }
      // ---- A: the prefixes' own terms
      float tot = -INFINITY, stay_b = -INFINITY, stay_nb = -INFINITY;
      int je = 0;                                              // the candidate slot that repeats the last label (0: none)
      sh.removed[lane] = 0;
      sh.removed[lane + 64] = 0;
      if (own) {
        tot = lae(pb, pnb);
        live = tot > -INFINITY;
        if (e >= 0)
          for (int j = 1; j < kp; ++j)
            if (sh.c_id[base + j] == e) je = j;
        stay_b = tot + sh.c_lp[base];
        if (je) stay_nb = pnb + sh.c_lp[base + je];
        sh.pb[lane] = pb; sh.tot[lane] = tot; sh.e[lane] = e; sh.par[lane] = par;
      }
      __syncthreads();
      // ---- B: the extension of the parent by this entry's last label is added here and leaves the pool
      if (own && live && par >= 0 && je) {
        const float from = e == sh.e[par] ? sh.pb[par] : sh.tot[par];
        stay_nb = lae(stay_nb, from + sh.c_lp[base + je]);
        sh.removed[par * PB_K + je - 1] = 1;
      }
      if (own) { sh.pool_b[lane] = stay_b; sh.pool_nb[lane] = stay_nb; }
      __syncthreads();
      // ---- C: the pool's scores
      float sc[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        sc[r] = -INFINITY;
        if (r == 0 && own) sc[0] = lae(stay_b, stay_nb);
        if (ext_valid[r]) {
          const int i = pi[r], j = pj[r];
          const int c = sh.c_id[base + 1 + j];
          const float ti = sh.tot[i];
          float v = -INFINITY;
          if (c >= 0 && ti > -INFINITY && !sh.removed[i * PB_K + j]) v = (c == sh.e[i] ? sh.pb[i] : ti) + sh.c_lp[base + 1 + j];
          sh.pool_b[lane + 64 * r] = -INFINITY;
          sh.pool_nb[lane + 64 * r] = v;
          sc[r] = v;
        }
      }
      // ---- D: the beam best, ties to the lower pool index
      int ord = -1, nsel = 0;
      for (int s = 0; s < beam; ++s) {
        const float m = wave_max_dpp(fmaxf(fmaxf(sc[0], sc[1]), sc[2]));
        if (!(m > -INFINITY)) break;
        int r = 0;
        unsigned long long eq = __ballot(sc[0] == m);
        if (!eq) { r = 1; eq = __ballot(sc[1] == m); }
        if (!eq) { r = 2; eq = __ballot(sc[2] == m); }
        if (!eq) break;                                         // (the maximum is one of the scores: never taken)
        const int wl = __builtin_ctzll(eq);
        if (lane == s) ord = wl + 64 * r;
        if (lane == wl) {
          if (r == 0) sc[0] = -INFINITY;
          else if (r == 1) sc[1] = -INFINITY;
          else sc[2] = -INFINITY;
        }
        nsel = s + 1;
      }
      __syncthreads();                                          // pool_b / pool_nb of every lane are written
      // ---- the survivors' state (slots from nsel on are dead: length 0, (-inf, -inf))
      const bool alive = lane < nsel;
      bool grown = false;
      int src = lane, at = -1, tok = -1, opar = -1;
      float n_pb = -INFINITY, n_pnb = -INFINITY;
      int n_len = 0, n_e = -2;
      unsigned n_h = 0, n_hp = 0;
      if (alive) {
        grown = ord >= beam;
        src = sh.tab_i[ord];
        n_pb = sh.pool_b[ord]; n_pnb = sh.pool_nb[ord];
        const int li = sh.len[src];
        if (grown) {
          tok = sh.c_id[base + 1 + sh.tab_j[ord]];
          at = li < cap ? li : -1;                              // (the caller's capacity holds lengths + frames: never taken)
          n_len = li < cap ? li + 1 : cap;
          n_e = tok; n_hp = sh.h[src]; n_h = n_hp + mix(li, tok);
        } else {
          n_len = li; n_e = sh.e[src]; n_h = sh.h[src]; n_hp = sh.hp[src]; opar = sh.par[src];
        }
      }
      if (own) sh.newslot[lane] = -1;
      __syncthreads();
      if (alive && !grown) sh.newslot[src] = lane;
      __syncthreads();
      if (own) {
        par = !alive ? -1 : grown ? sh.newslot[src] : opar >= 0 ? sh.newslot[opar] : -1;
        pb = n_pb; pnb = n_pnb; len = n_len; e = n_e; h = n_h; hp = n_hp;
        live = alive;
        sh.len[lane] = len; sh.h[lane] = h; sh.hp[lane] = hp; sh.src[lane] = src;
      }
      fresh = __ballot(alive && grown);
      __syncthreads();
      // ---- the survivors' strings into the other buffer, 16 bytes a lane, then the new labels
      if (slot4 < beam) {
        const int4* from = reinterpret_cast<const int4*>(cur + sh.src[slot4] * cap4);
        int4* to = reinterpret_cast<int4*>(nxt + slot4 * cap4);
        const int n4 = (maxlen + 3) >> 2;
        for (int q = sub; q < n4; q += 4) to[q] = from[q];
      }
      __syncthreads();
      if (at >= 0) nxt[lane * cap4 + at] = tok;
      { int* tmp = cur; cur = nxt; nxt = tmp; }
      maxlen = maxlen < cap ? maxlen + 1 : cap;
      __syncthreads();
    }
  }
  // ---- the state goes back: `pad` behind each length, dead slots all pad
  if (own) {
    lengths[(long)b * beam + lane] = len;
    p_b[(long)b * beam + lane] = pb;
    p_nb[(long)b * beam + lane] = pnb;
  }
  for (int s = 0; s < beam; ++s) {
    const int ls = sh.len[s];
    for (int p = lane; p < cap; p += 64) gs[(long)s * cap + p] = p < ls ? (long)cur[s * cap4 + p] : (long)pad;
  }
}

}  // namespace

extern "C" int simulst_ctc_prefix_beam(simulst_handle* h, const float* cand_log_probs, int64_t lp_stride_t, int64_t lp_stride_b,
                                       int64_t lp_stride_v, const int64_t* input_lengths, int32_t S, int32_t N, int32_t beam,
                                       int32_t blank, const simulst_ctc_prefix_desc* desc, int64_t* strings) {
  if (!h) return SIMULST_E_NULL;
  SL_CHECK_NULL(h, desc);
  const simulst_ctc_prefix_desc* d = desc;
  SL_CHECK_NULL(h, strings); SL_CHECK_NULL(h, cand_log_probs); SL_CHECK_NULL(h, input_lengths);
  SL_CHECK_NULL(h, d->cand_ids); SL_CHECK_NULL(h, d->lengths); SL_CHECK_NULL(h, d->p_b); SL_CHECK_NULL(h, d->p_nb);
  SL_REQUIRE(h, S > 0 && blank >= 0, SIMULST_E_SHAPE, "simulst_ctc_prefix_beam: shape");
  SL_REQUIRE(h, beam >= 1 && beam <= PB_BEAM, SIMULST_E_SHAPE, "simulst_ctc_prefix_beam: beam is 1..16");
  SL_REQUIRE(h, d->k >= 0 && d->k <= PB_K, SIMULST_E_SHAPE, "simulst_ctc_prefix_beam: k is 0..8");
  SL_REQUIRE(h, d->cap >= 1 && d->cap <= SIMULST_CTC_PREFIX_CAP(beam), SIMULST_E_SHAPE,
             "simulst_ctc_prefix_beam: cap is 1..SIMULST_CTC_PREFIX_CAP(beam)");
  if (N <= 0) return SIMULST_OK;
  const size_t lds = (size_t)2 * beam * ((d->cap + 3) & ~3) * sizeof(int);
  static_assert(SIMULST_CTC_PREFIX_STRING_BYTES + PB_STATIC_LDS <= 160 * 1024, "LDS of a compute unit");
  static const sl_lds_limit limits[] = {{(const void*)ctc_prefix_kernel, SIMULST_CTC_PREFIX_STRING_BYTES}};
  if (lds + PB_STATIC_LDS > 48 * 1024)
    if (int rc = sl_raise_lds(h, SL_LDS_CTC_PREFIX, limits, "simulst_ctc_prefix_beam")) return rc;
  KTimer t(h, SIMULST_K_SCAN);
  hipLaunchKernelGGL(ctc_prefix_kernel, dim3(N), dim3(64), lds, h->stream, cand_log_probs, (long)lp_stride_t, (long)lp_stride_b,
                     (long)lp_stride_v, d->cand_ids, (long)d->id_stride_b, (long)d->id_stride_t, (const long*)input_lengths, S, beam,
                     d->k, d->cap, d->pad, (long*)strings, (long*)d->lengths, d->p_b, d->p_nb);
  return sl_launch_status(h, "simulst_ctc_prefix_beam");
}
