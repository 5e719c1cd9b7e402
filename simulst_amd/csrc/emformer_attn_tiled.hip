// Emformer chunk+memory block attention for segment geometries beyond 128 keys (gfx950): the key list of a segment is walked
// in blocks under an online softmax, so neither the number of keys M + R + Lc + S nor the number of queries R + S + 1 of a
// segment is bounded by registers or LDS.  Two forms:
//
//   * TILED MFMA (bf16, head_dim 64): emformer_attn_mfma.hip's scheme -- S^T = K . Q^T with v_mfma_f32_32x32x16_bf16 so that a lane
//     owns ONE query column, P kept in the accumulators and fed back as an operand, V staged row-major in LDS and read by the
//     transpose read, masks through the accumulator's initial value (0, -inf, the summary query's -1e8 on memory keys),
//     exp2(fma(...)) -- over query blocks of 32 and key blocks of 64.  Because a lane owns one query, the running max, the
//     running sum and the rescale exp2((m_old - m_new) c) of the output accumulators are lane scalars: the only exchange is the
//     lane <-> lane + 32 swap of the block max (and of the sum, once, at the end).  Every probability is rounded to bf16 once,
//     the denominator is summed from the unrounded fp32 values, 1 / sum is applied once, in fp32, at the end.
//     WORK SPLIT: one workgroup per (segment, utterance) in the XCD-aware order of the one-tile kernel, and the (head, query
//     block) units of that segment dealt round-robin to its 4 waves.  The reason is reuse: every unit of a segment reads the same
//     <= M + R + Lc + S key rows (one 128-byte slice per head and row), and neighbouring segments share the left context, so
//     keeping a segment's units on one CU and consecutive segments on one XCD turns all but the first read of a row into an L1 /
//     L2 hit; query blocks on a grid axis would spread those reads over the XCDs.  A segment of the quality-end geometry has
//     3 query blocks x 4..8 heads = 12..24 units, three to six per wave, and a batch has hundreds of segments, so the grid fills
//     the 256 CUs without a finer split.  LDS is one 12 KB V block per wave whatever nk and nq are; the next block's K fragments
//     and V rows are requested before the current block's products (a wave's life is its chain of dependent memory round
//     trips), which costs 64 registers and is why the kernel runs two workgroups per CU.
//   * LOOPED GENERAL (fp32, any head_dim <= 64 in either dtype, or bf16 under SIMULST_OPT_VALU_ATTENTION): emformer_attn.hip's
//     scheme -- key per lane for the scores, channel per lane for PV, fp32 throughout, rounding at the store alone -- with an
//     outer loop over key blocks of 128 staged in LDS.  A wave carries the (max, sum, output channel) of 20 queries in registers
//     across the key blocks; a workgroup therefore passes over the key list once per 80 queries.  The cross-check of the form
//     above and the path of the fp32 oracle tests.
//
// Every key block kb < ceil(nk / 64) (128) holds the present key 64 kb (128 kb), so no query ever meets a block of all -inf; the
// summary query's block of memory keys alone has the finite maximum -1e8, and its later rescale factor is exactly 0.
#include "emformer_attn_core.h"

namespace {

struct EmfArgsT {
  int T, D, H, d, S, R, Lc, M;
  int n_mem, n_seg, use_summary;
  int rows_z, rows_c;
};

// ------------------------------------------------------------------------------------------------ tiled MFMA form
template <bool STREAMING>
__global__ __launch_bounds__(256, 2) void emformer_attn_tiled_mfma_kernel(
    const bf16* __restrict__ QKV, const int* __restrict__ lengths, const bf16* __restrict__ lc_k,
    const bf16* __restrict__ lc_v, const int* __restrict__ lc_valid, const int* __restrict__ n_mem_valid,
    bf16* __restrict__ CTX, EmfArgsT a) {
  __shared__ __attribute__((aligned(16))) unsigned short vt_all[4][64 * VR_STRIDE];
  // XCD-aware order (emformer_attn_mfma.hip): every XCD walks through consecutive (utterance, segment) pairs
  const int nb_full = (int)gridDim.x & ~7;
  const int bid = (int)blockIdx.x < nb_full ? ((int)blockIdx.x & 7) * (nb_full >> 3) + ((int)blockIdx.x >> 3)
                                            : (int)blockIdx.x;
  const int i = bid % a.n_seg, b = bid / a.n_seg;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 31, lh = lane >> 5;
  const int D3 = 3 * a.D;
  const int len = lengths ? lengths[b] : a.T;
  const int t0 = i * a.S, t1 = min(t0 + a.S, a.T);
  if (t0 >= len && !STREAMING) return;
  const int n_rc = a.n_seg * a.R;
  int mem_lo, mem_hi;
  if (STREAMING) {
    const int nv = n_mem_valid ? n_mem_valid[b] : 0;
    mem_lo = a.n_mem - nv; mem_hi = a.n_mem;
  } else {
    mem_lo = a.use_summary ? max(0, i - a.M) : 0;
    mem_hi = a.use_summary ? i : 0;
  }
  const int n_memk = mem_hi - mem_lo;
  const int n_lck = STREAMING ? (lc_valid ? lc_valid[b] : 0) : 0;
  const int u_lo = STREAMING ? 0 : max(0, t0 - a.Lc);
  const int u_hi = min(t1, max(len, 0));
  const int n_uk = max(0, u_hi - u_lo);
  const int nk = n_memk + a.R + n_lck + n_uk;
  const int nk1 = max(nk - 1, 0);                        // absent keys read key nk - 1: a present row, masked
  const int nq = a.R + (t1 - t0) + (a.use_summary ? 1 : 0);
  const int nkb = max((nk + 63) >> 6, 1), nqb = (nq + 31) >> 5;
  const bf16* Zb = QKV + (long)b * a.rows_z * D3;
  bf16* Cb = CTX + (long)b * a.rows_c * a.D;
  unsigned short* vt = vt_all[wave];

  // key j (clamped to a present key) -> its row in the utterance's QKV block; order [memory | rc | left context | utterance]:
  // three affine pieces, written as sums of masked differences (emformer_attn_mfma.hip)
  const int c_utt = a.n_mem + n_rc + u_lo - n_memk - a.R - n_lck;
  const int d_rc = (a.n_mem + i * a.R - n_memk) - c_utt, d_mem = mem_lo - (a.n_mem + i * a.R - n_memk);
  auto key_row = [&](int j) {
    return j + c_utt + (j < n_memk + a.R ? d_rc : 0) + (j < n_memk ? d_mem : 0);
  };
  auto key_off = [&](int j) { return (unsigned)(key_row(min(j, nk1)) * D3); };
  auto key_ptrs = [&](int j, const bf16*& kp, const bf16*& vp) {      // streaming: the left-context keys live in lc_k / lc_v
    const int jc = min(j, nk1);
    const bf16* row = Zb + (unsigned)(key_row(jc) * D3);      // of a left-context key: computed, never read
    kp = row + a.D; vp = row + 2 * a.D;
    const int jl = jc - n_memk - a.R;
    const bool in_lc = jl >= 0 && jl < n_lck;
    const long r = (long)b * a.Lc + (a.Lc - n_lck + (in_lc ? jl : 0));
    kp = in_lc ? lc_k + r * a.D : kp;
    vp = in_lc ? lc_v + r * a.D : vp;
  };
  // query q (clamped) -> rows in Z (source) and CTX (destination): [rc block i | utterance rows of the segment | summary i]
  const int n_u = t1 - t0;
  const int c_sum = n_rc + a.T + i - a.R - n_u, e_utt = (n_rc + t0 - a.R) - c_sum, e_rc = i * a.R - (n_rc + t0 - a.R);
  auto q_rows = [&](int qi, int& zrow, int& crow) {
    const int q = min(qi, nq - 1);
    crow = q + c_sum + (q < a.R + n_u ? e_utt : 0) + (q < a.R ? e_rc : 0);
    zrow = crow + a.n_mem;
  };
  constexpr float kScale = 0.125f * 1.44269504088896341f;       // 64^-0.5 * log2(e)
  const int vc8 = (lane & 7) * 8;

  // K fragments (keys 64 kb + 32 t + lr; k = 16 kk + 8 lh + j) and V rows (16-byte chunks, 8 lanes per key row) of key block kb
  auto load_kv = [&](int kb, int hc, uint4 (&kf)[2][4], uint4 (&vrows)[8]) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if constexpr (STREAMING) {
        const bf16 *kp, *vp;
        key_ptrs(64 * kb + 32 * t + lr, kp, vp);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) kf[t][kk] = *reinterpret_cast<const uint4*>(kp + hc + 16 * kk + 8 * lh);
      } else {
        const unsigned ko = key_off(64 * kb + 32 * t + lr) + a.D + hc + 8 * lh;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) kf[t][kk] = ld_off(Zb, ko + 16 * kk);
      }
    }
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      if constexpr (STREAMING) {
        const bf16 *kp, *vp;
        key_ptrs(64 * kb + 8 * it + (lane >> 3), kp, vp);
        vrows[it] = *reinterpret_cast<const uint4*>(vp + hc + vc8);
      } else {
        vrows[it] = ld_off(Zb, key_off(64 * kb + 8 * it + (lane >> 3)) + 2 * a.D + hc + vc8);
      }
    }
  };

  for (int u = wave; u < a.H * nqb; u += 4) {
    const int hc = (u % a.H) * 64, q0 = (u / a.H) * 32;
    uint4 qf[4];
    {
      int zrow, crow;
      q_rows(q0 + lr, zrow, crow);
      const unsigned qo = (unsigned)(zrow * D3) + hc + 8 * lh;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) qf[kk] = ld_off(Zb, qo + 16 * kk);
    }
    const bool q_is_sum = a.use_summary && q0 + lr == nq - 1;
    uint4 kf[2][4], vrows[8];
    if constexpr (!STREAMING) load_kv(0, hc, kf, vrows);
    float m = -INFINITY, l = 0.f;                  // running max (of the unscaled scores) and this lane's half of the running sum
    f32x16 o[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[nt][e] = 0.f;

    for (int kb = 0; kb < nkb; ++kb) {
      uint4 kn[2][4], vn[8];
      if constexpr (STREAMING) {                                   // one short segment per call: no request ahead, fewer registers
        load_kv(kb, hc, kf, vrows);
      } else if (kb + 1 < nkb) {                                   // uniform
        load_kv(kb + 1, hc, kn, vn);
      } else {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) kn[t][kk] = kf[t][kk];
#pragma unroll
        for (int it = 0; it < 8; ++it) vn[it] = vrows[it];
      }
      // ---- S^T tiles: st[t][e] = score(key 64 kb + 32 t + (e&3) + 8 (e>>2) + 4 lh, query q0 + lr) + its mask value
      const int rem = nk - 64 * kb, mem_rem = n_memk - 64 * kb;    // present keys / memory keys from this block's first key on
      const int lim_hi = rem - 4 * lh;
      const int lim_mem = q_is_sum ? mem_rem - 4 * lh : -64;
      f32x16 st[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (rem >= 32 * t + 36) {                                  // uniform: every key of the tile is present
#pragma unroll
          for (int e = 0; e < 16; ++e) st[t][e] = 0.f;
        } else {
#pragma unroll
          for (int e = 0; e < 16; ++e) st[t][e] = 32 * t + (e & 3) + 8 * (e >> 2) < lim_hi ? 0.f : -INFINITY;
        }
        if (a.use_summary && mem_rem > 32 * t) {                   // uniform: memory keys in this tile
#pragma unroll
          for (int e = 0; e < 16; ++e) st[t][e] = 32 * t + (e & 3) + 8 * (e >> 2) < lim_mem ? -8e8f : st[t][e];
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
          st[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(&kf[t][kk]),
                                                          *reinterpret_cast<const bf16x8_t*>(&qf[kk]), st[t], 0, 0, 0);
      }
      // ---- online softmax: the block's max joins the running max; everything accumulated so far is rescaled by alpha
      float mx = -INFINITY;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) mx = fmaxf(mx, st[t][e]);
      {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
        mx = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
      }
      const float m_new = fmaxf(m, mx);
      // first block: nothing accumulated yet (and exp2(-inf - -inf) would be NaN for a query whose first block were all absent)
      const float alpha = m == -INFINITY ? 0.f : __builtin_amdgcn_exp2f((m - m_new) * kScale);
      m = m_new;
      const float mxs = m_new * kScale;
      float sum = 0.f;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(st[t][e], kScale, -mxs));
          st[t][e] = p;
          sum += p;
        }
      l = __builtin_fmaf(l, alpha, sum);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[nt][e] *= alpha;
      // ---- V rows into LDS as they came (row-major); rows of absent keys hold a present key's values (P is exactly 0 there)
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        const int j = 8 * it + (lane >> 3);
        *reinterpret_cast<uint4*>(vt + j * VR_STRIDE + vc8) = vrows[it];
      }
      __builtin_amdgcn_wave_barrier();
      // ---- O^T += V^T . P^T (fragment orders as in emformer_attn_mfma.hip)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          uint4 pa;
          pa.x = pack2(st[t][8 * s + 0], st[t][8 * s + 1]);
          pa.y = pack2(st[t][8 * s + 2], st[t][8 * s + 3]);
          pa.z = pack2(st[t][8 * s + 4], st[t][8 * s + 5]);
          pa.w = pack2(st[t][8 * s + 6], st[t][8 * s + 7]);
          const int key0 = 32 * t + 16 * s + 4 * lh;
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) {
            const int li = lane & 15;
            const unsigned short* blk = vt + (key0 + (li >> 2)) * VR_STRIDE + 32 * nt + 16 * ((lane >> 4) & 1) + 4 * (li & 3);
            const tr_v4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)blk);                      // keys key0 .. key0+3
            const tr_v4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(blk + 8 * VR_STRIDE));    // keys key0+8 .. key0+11
            uint4 vb;
            __builtin_memcpy(&vb.x, &lo, 8);
            __builtin_memcpy(&vb.z, &hi, 8);
            o[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(&vb),
                                                            *reinterpret_cast<const bf16x8_t*>(&pa), o[nt], 0, 0, 0);
          }
        }
      __builtin_amdgcn_wave_barrier();                             // the V image is consumed before the next block overwrites it
      if constexpr (!STREAMING) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) kf[t][kk] = kn[t][kk];
#pragma unroll
        for (int it = 0; it < 8; ++it) vrows[it] = vn[it];
      }
    }
    {
      const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(l), __float_as_uint(l), false, false);
      l = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
    const float inv = 1.0f / l;
    // ---- o[nt][e] = ctx(query q0 + lr, channel 32 nt + 8 (e>>2) + 4 lh + (e&3)) * sum: through LDS as [query][64 channels], then
    //      16-byte row-contiguous stores
    constexpr int OT_STRIDE = 72;
    unsigned short* ot = vt;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        uint2 pk;
        pk.x = pack2(o[nt][4 * g + 0] * inv, o[nt][4 * g + 1] * inv);
        pk.y = pack2(o[nt][4 * g + 2] * inv, o[nt][4 * g + 3] * inv);
        *reinterpret_cast<uint2*>(&ot[lr * OT_STRIDE + 32 * nt + 8 * g + 4 * lh]) = pk;
      }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int ql = 8 * it + (lane >> 3);
      int zrow, crow;
      q_rows(q0 + ql, zrow, crow);
      if (q0 + ql < nq)
        *reinterpret_cast<uint4*>(reinterpret_cast<char*>(Cb) + (size_t)((unsigned)(crow * a.D + hc + (lane & 7) * 8) * 2u)) =
            *reinterpret_cast<const uint4*>(&ot[ql * OT_STRIDE + (lane & 7) * 8]);
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// ------------------------------------------------------------------------------------------------ looped general form
constexpr int LOOP_KB = 128;    // keys staged per block: two per lane
// queries a wave carries across the key blocks: 4 x 20 = 80 per pass over the key list, so the R + S + 1 = 73 queries of a 64-row
// segment need one pass (the staging loop is a chain of dependent loads: a second pass costs as much as the products).  The two
// staged blocks are 65 KB of LDS, two workgroups per CU, so the registers this costs buy no occupancy back.
constexpr int LOOP_QPW = 20;

template <typename T>
__global__ __launch_bounds__(256) void emformer_attn_looped_kernel(
    const T* __restrict__ QKV, const int* __restrict__ lengths, const T* __restrict__ lc_k,
    const T* __restrict__ lc_v, const int* __restrict__ lc_valid, const int* __restrict__ n_mem_valid,
    T* __restrict__ CTX, EmfArgsT a) {
  extern __shared__ float sm[];
  const int i = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d = a.d, dp = d + 1, D3 = 3 * a.D;
  float* Ks = sm;                   // [LOOP_KB][dp]
  float* Vs = sm + LOOP_KB * dp;    // [LOOP_KB][dp]
  const bool streaming = lc_k != nullptr;
  const int len = lengths ? lengths[b] : a.T;
  const int t0 = i * a.S, t1 = min(t0 + a.S, a.T);
  if (t0 >= len && !streaming) return;            // segment beyond this utterance
  const int n_rc = a.n_seg * a.R;

  // ---- key list: [memory | rc block i | cached left context | utterance]
  int mem_lo, mem_hi;
  if (streaming) {
    int nv = n_mem_valid ? n_mem_valid[b] : 0;
    mem_lo = a.n_mem - nv; mem_hi = a.n_mem;
  } else {
    mem_lo = a.use_summary ? max(0, i - a.M) : 0;
    mem_hi = a.use_summary ? i : 0;
  }
  const int n_memk = mem_hi - mem_lo;
  const int n_lck = streaming ? (lc_valid ? lc_valid[b] : 0) : 0;
  const int u_lo = streaming ? 0 : max(0, t0 - a.Lc);
  const int u_hi = min(t1, max(len, 0));
  const int n_uk = max(0, u_hi - u_lo);
  const int nk = n_memk + a.R + n_lck + n_uk;
  const int nq = a.R + (t1 - t0) + (a.use_summary ? 1 : 0);
  const int nkb = max((nk + LOOP_KB - 1) / LOOP_KB, 1);
  const float scaling = rsqrtf((float)d);
  const T* Zb = QKV + (long)b * a.rows_z * D3;

  for (int h = 0; h < a.H; ++h) {
    for (int q0 = 0; q0 < nq; q0 += 4 * LOOP_QPW) {
      // ---- this wave's queries q0 + wave + 4 u: scaled q (channel per lane), running max, running sum, output channel
      float qv[LOOP_QPW], mrun[LOOP_QPW], den[LOOP_QPW], o[LOOP_QPW];
#pragma unroll
      for (int u = 0; u < LOOP_QPW; ++u) {
        const int qi = min(q0 + wave + 4 * u, nq - 1);
        int zrow;
        if (qi < a.R) zrow = a.n_mem + i * a.R + qi;
        else if (qi < a.R + (t1 - t0)) zrow = a.n_mem + n_rc + t0 + qi - a.R;
        else zrow = a.n_mem + n_rc + a.T + i;
        qv[u] = lane < d ? to_f32(Zb[(long)zrow * D3 + h * d + lane]) * scaling : 0.f;
        mrun[u] = -INFINITY; den[u] = 0.f; o[u] = 0.f;
      }
      for (int kb = 0; kb < nkb; ++kb) {
        const int j0 = kb * LOOP_KB, jn = min(LOOP_KB, nk - j0);
        __syncthreads();                               // the previous block's readers are done
        // ---- stage K_h, V_h of keys j0 .. j0 + jn - 1: one wave per key row, lane = channel
        for (int jl = wave; jl < jn; jl += 4) {
          const T *kp, *vp;
          int jj = j0 + jl;
          if (jj < n_memk) {
            const T* row = Zb + (long)(mem_lo + jj) * D3;
            kp = row + a.D; vp = row + 2 * a.D;
          } else if ((jj -= n_memk) < a.R) {
            const T* row = Zb + (long)(a.n_mem + i * a.R + jj) * D3;
            kp = row + a.D; vp = row + 2 * a.D;
          } else if ((jj -= a.R) < n_lck) {
            long r = (long)b * a.Lc + (a.Lc - n_lck + jj);
            kp = lc_k + r * a.D; vp = lc_v + r * a.D;
          } else {
            jj -= n_lck;
            const T* row = Zb + (long)(a.n_mem + n_rc + u_lo + jj) * D3;
            kp = row + a.D; vp = row + 2 * a.D;
          }
          if (lane < d) {
            Ks[jl * dp + lane] = to_f32(kp[h * d + lane]);
            Vs[jl * dp + lane] = to_f32(vp[h * d + lane]);
          }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < LOOP_QPW; ++u) {
          const int qi = q0 + wave + 4 * u;
          if (qi >= nq) continue;                      // wave-uniform
          const bool is_sum = a.use_summary && qi == nq - 1;
          float s[2] = {0.f, 0.f};
          if (jn > 64) {
            for (int c = 0; c < d; ++c) {
              const float qc = __shfl(qv[u], c, 64);
#pragma unroll
              for (int kc = 0; kc < 2; ++kc) s[kc] = fmaf(qc, Ks[(kc * 64 + lane) * dp + c], s[kc]);
            }
          } else {                                     // a short last block: one key per lane
            for (int c = 0; c < d; ++c) s[0] = fmaf(__shfl(qv[u], c, 64), Ks[lane * dp + c], s[0]);
          }
          float mx = -INFINITY;
#pragma unroll
          for (int kc = 0; kc < 2; ++kc) {
            const int jl = kc * 64 + lane;
            if (jl >= jn) s[kc] = -INFINITY;
            else if (is_sum && j0 + jl < n_memk) s[kc] = -1e8f;   // summary query does not see memory (:301-302,760)
            mx = fmaxf(mx, s[kc]);
          }
          const float m_new = fmaxf(mrun[u], wave_max(mx));
          // first block: nothing accumulated yet (expf(-inf - -inf) would be NaN)
          const float alpha = mrun[u] == -INFINITY ? 0.f : expf(mrun[u] - m_new);
          mrun[u] = m_new;
          float part = 0.f;
#pragma unroll
          for (int kc = 0; kc < 2; ++kc) {
            s[kc] = (kc * 64 + lane < jn) ? expf(s[kc] - m_new) : 0.f;
            part += s[kc];
          }
          den[u] = fmaf(den[u], alpha, part);          // this lane's share; summed over the wave once, at the end
          float acc = o[u] * alpha;
#pragma unroll
          for (int kc = 0; kc < 2; ++kc) {
            const int jc = min(64, jn - kc * 64);
            for (int j = 0; j < jc; ++j) {
              const float pj = __shfl(s[kc], j, 64);
              acc = fmaf(pj, Vs[(kc * 64 + j) * dp + min(lane, d - 1)], acc);
            }
          }
          o[u] = acc;
        }
      }
#pragma unroll
      for (int u = 0; u < LOOP_QPW; ++u) {
        const int qi = q0 + wave + 4 * u;
        if (qi >= nq) continue;
        int crow;
        if (qi < a.R) crow = i * a.R + qi;
        else if (qi < a.R + (t1 - t0)) crow = n_rc + t0 + qi - a.R;
        else crow = n_rc + a.T + i;
        const float inv = 1.0f / wave_sum(den[u]);
        if (lane < d) CTX[((long)b * a.rows_c + crow) * a.D + h * d + lane] = from_f32<T>(o[u] * inv);
      }
    }
  }
}

}  // namespace

// internal entry used by simulst_emformer_attention (emformer_attn.hip) for segments of more than 128 keys
int sl_emformer_attention_tiled(simulst_handle* h, const simulst_emf_attn_desc* d, const void* QKV,
                                const int32_t* lengths, const void* lc_k, const void* lc_v, const int32_t* lc_valid,
                                const int32_t* n_mem_valid, void* CTX) {
  EmfArgsT a;
  a.T = d->T; a.D = d->D; a.H = d->H; a.d = d->D / d->H; a.S = d->S; a.R = d->R; a.Lc = d->Lc; a.M = d->M;
  a.n_mem = d->n_mem; a.n_seg = d->n_seg; a.use_summary = d->use_summary;
  const int n_sum = d->use_summary ? d->n_seg : 0;
  a.rows_z = d->n_mem + d->n_seg * d->R + d->T + n_sum;
  a.rows_c = d->n_seg * d->R + d->T + n_sum;
  if (d->dtype == SIMULST_BF16 && a.d == 64 && !h->force_valu_attention) {
    // rows are addressed as 32-bit element offsets from the utterance's first QKV / CTX row
    SL_REQUIRE(h, (long)a.rows_z * 3 * a.D < (1L << 31), SIMULST_E_SHAPE,
               "simulst_emformer_attention: one utterance's QKV block (rows x 3 D) must stay below 2^31 elements");
    SL_REQUIRE(h, (long)d->n_seg * d->B < (1L << 31), SIMULST_E_SHAPE, "simulst_emformer_attention: n_seg x B must stay below 2^31");
    KTimer t(h, SIMULST_K_EMF_ATTN);
    if (lc_k)
      hipLaunchKernelGGL(emformer_attn_tiled_mfma_kernel<true>, dim3(d->n_seg * d->B), dim3(256), 0, h->stream,
                         (const bf16*)QKV, lengths, (const bf16*)lc_k, (const bf16*)lc_v, lc_valid, n_mem_valid, (bf16*)CTX, a);
    else
      hipLaunchKernelGGL(emformer_attn_tiled_mfma_kernel<false>, dim3(d->n_seg * d->B), dim3(256), 0, h->stream,
                         (const bf16*)QKV, lengths, (const bf16*)lc_k, (const bf16*)lc_v, lc_valid, n_mem_valid, (bf16*)CTX, a);
    return sl_launch_status(h, "simulst_emformer_attention(tiled mfma)");
  }
  const size_t lds = (size_t)2 * LOOP_KB * (a.d + 1) * sizeof(float);
  KTimer t(h, SIMULST_K_EMF_ATTN);
  dim3 grid(d->n_seg, d->B);
  if (d->dtype == SIMULST_F32)
    hipLaunchKernelGGL(emformer_attn_looped_kernel<float>, grid, dim3(256), lds, h->stream, (const float*)QKV, lengths,
                       (const float*)lc_k, (const float*)lc_v, lc_valid, n_mem_valid, (float*)CTX, a);
  else
    hipLaunchKernelGGL(emformer_attn_looped_kernel<bf16>, grid, dim3(256), lds, h->stream, (const bf16*)QKV, lengths,
                       (const bf16*)lc_k, (const bf16*)lc_v, lc_valid, n_mem_valid, (bf16*)CTX, a);
  return sl_launch_status(h, "simulst_emformer_attention(looped)");
}
