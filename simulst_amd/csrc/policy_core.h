// The decision rules of the monotonic policy, each written once: every decode-step and scoring kernel that masks the past, forces
// the stop, inserts zeros between pooled probabilities, masks a padded pooling window or picks the keys a step attends to calls
// these (callers: DESIGN.md, "Policy rules").  Integer / boolean rules of scalars only -- how a kernel computes its energies and
// which value it writes for a masked position stay with the kernel.  The fp64 reference of tests/test_hip_policy_cross_attention.py
// restates none of this: it is built from oracle.monotonic.
#pragma once
#include "common.h"

namespace policy {

// the forced stop of the step search (monotonic_multihead_attention.py:196-257): the last frame with mass preservation, one past it without
__host__ __device__ __forceinline__ int max_steps_of(int len, int mass_pres) { return mass_pres ? len - 1 : len; }
// a step as a row index: -1 for an empty source (len == 0), which has no row
template <typename I>                    // int, or long as head_step stores it
__host__ __device__ __forceinline__ I clamp_step(I found, int len) {
  const I lo = found > 0 ? found : 0;
  return lo < len - 1 ? lo : len - 1;
}

struct Step { int found; bool read; };   // head_step, head_read

// wait-k in closed form: the one-hot pooled probability sits at pooled index wk, i.e. at frame (wk+1)*ratio - 1, and/or at the last
// frame when the final window is the pooled position wk (fixed_pre_decision.py:133-167; p_choose_strategy.py:6-53); the search
// then is a minimum over <= 3 candidates.  tg: target index, hs: the head's previous step, P = pooled_count(len, ratio, true, .)
__host__ __device__ __forceinline__ Step waitk_step(int tg, int waitk_k, int online, int P, int ratio, int len, int mass_pres, long hs) {
  int wk = tg + waitk_k - 1;
  if (!online) wk = min(wk, P - 1);
  int s1 = -1, s2 = -1;                               // frames with p = 1
  if (wk < P) {
    const int c1 = (wk + 1) * ratio - 1;
    if (c1 < len) s1 = c1;
    if (wk == P - 1 && P * ratio >= len) s2 = len - 1;
  }
  const int max_steps = max_steps_of(len, mass_pres);
  int found = max_steps;                              // the forced stop, valid even below head_step
  if (s1 >= 0 && (long)s1 >= hs) found = min(found, s1);
  if (s2 >= 0 && (long)s2 >= hs) found = min(found, s2);
  if (found < 0) found = 0;
  const int clampi = clamp_step(found, len);
  const bool one = clampi >= 0 && (clampi == s1 || clampi == s2);
  return {found, found == max_steps && !one};
}

// first index with p >= 0.5 of a row of S step probabilities (LDS or global), by one wave in 64-wide chunks: the past (j < hs) is
// masked, the stop is forced (1.0 at max_steps); without mass preservation the searched row is one longer than the source
__device__ __forceinline__ int first_step(const float* p, int S, int len, int mass_pres, long hs, int lane) {
  const int max_steps = max_steps_of(len, mass_pres);
  const int n = mass_pres ? S : S + 1;
  int found = -1;
  for (int j0 = 0; j0 < n && found < 0; j0 += 64) {
    const int j = j0 + lane;
    float v = 0.f;
    if (j < n) {
      v = (j < S) ? p[j] : 0.f;
      if ((long)j < hs) v = 0.f;
      if (j == max_steps) v = 1.f;
    }
    const unsigned long long m = __ballot(j < n && v >= 0.5f);
    if (m) found = j0 + __ffsll((long long)m) - 1;
  }
  return found < 0 ? 0 : found;                       // unreachable: the forced 1.0 always hits
}
// the row's probability at the clamped step (nothing to load for an empty source), and the READ decision from it: the search ran
// into the forced stop and the frame there did not fire by itself; an empty source (len == 0, clamp -1) always reads
__device__ __forceinline__ float p_at_clamp(const float* p, int found, int len) {
  const int c = clamp_step(found, len);
  return c >= 0 ? p[c] : 0.f;
}
__host__ __device__ __forceinline__ bool head_read_of(int found, int len, int mass_pres, float p_at_clamp) {
  const bool at_stop = mass_pres ? found == len - 1 : found == len;      // found == max_steps_of(len, mass_pres)
  return at_stop && (len <= 0 || p_at_clamp < 0.5f);
}

// zero insertion (fixed_pre_decision.py:143-159): the pooled position whose value lands on source frame s, -1 for an inserted
// zero (and behind the source).  Pooled j lands on frame (j+1)*ratio - 1; when the upsampled row reaches the end of the source
// it is cropped and the LAST frame takes the last pooled value.  A training-mode forward has P = ceil(len / ratio) (P = len for
// 'last' with len < ratio), so P * ratio >= len always holds there.
__host__ __device__ __forceinline__ int pooled_index_at(int s, int len, int ratio, int P) {
  if (s >= len) return -1;
  int j = -1;
  if ((s + 1) % ratio == 0 && (s + 1) / ratio - 1 < P) j = (s + 1) / ratio - 1;
  if (s == len - 1 && P * ratio >= len) j = P - 1;
  return j;
}

// pooled padding mask of a padded batch (fixed_pre_decision.py:104-131): pooled position j over frames [f0, f1) of a row with
// len_b valid frames is masked when more than pad_thr of its window is padding; the first position never is
__device__ __forceinline__ bool window_masked(int j, int f0, int f1, int len_b, float pad_thr) {
  if (j <= 0) return false;
  const int n_pad = f1 - max(f0, min(f1, len_b));
  return (float)n_pad / (float)(f1 - f0) > pad_thr;
}

// soft attention (monotonic_multihead_attention.py:278-293): keys [0, n) with n = min(st, len - 1) + 1 take part; 0 -- attend to
// nothing -- while the head has not moved (st == 0; `full`, plain encoder-decoder attention, has no such rule) and for an empty source
__host__ __device__ __forceinline__ int attended_keys(long st, int len, bool full) {
  const int n = (int)(st < len - 1 ? st : len - 1) + 1;
  return ((st > 0 || full) && n > 0) ? n : 0;
}
// hard attention (:261-275): the row at clamp(st), -1 (attend to nothing) for a head that ran off the end without mass
// preservation (st == len) and for an empty source (whose clamp is -1 already)
template <typename I>
__host__ __device__ __forceinline__ I hard_row(I st, int len, int mass_pres) {
  const bool dead = (!mass_pres) && st == max_steps_of(len, mass_pres);   // the forced stop, one past the last frame
  return dead ? -1 : clamp_step(st, len);
}

}  // namespace policy
