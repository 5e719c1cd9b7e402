// Forms of csrc/ffn_pipe.hip that measured SLOWER than what ships (ffn_variant.h has the figures): the phase forms -- scalar GELU,
// `make EXPERIMENTS=1`, SIMULST_OPT_FFN_WAVES 41 / 81; packed GELU, `make DEBUG_HOOKS=1`, 42 / 82 -- and, EXPERIMENTS only, 64 rows per
// wave (45).  ffn_pipe.hip includes this file twice: once inside its anonymous namespace in front of ffn_pipe_kernel (gelu_fast1 and
// ffn_wide_kernel, which see its building blocks: cvt_pk_bf16, gelu_quarter, stage_tile), and once, with SL_FFN_PHASE_BODY defined, as
// the UNI = false branch of ffn_pipe_kernel's tile iteration -- as text, not as a function: the phase forms' register allocation
// (256 VGPRs, 24 to 80 bytes of scratch) does not survive a call boundary, and no test runs the packed ones.
// tests/test_hip_kernels.py::test_emformer_ffn_pipelined_equals_the_block_form keeps 41 / 45 / 81 bit-identical to the block form.

#ifdef SL_FFN_PHASE_BODY
// In scope (ffn_pipe_kernel's `iteration`): PK, MORE; hcur / hnext, the fc1 accumulators of tiles t / t + 1; wfa, the first FF_PF
// fragments of w1; w2; bt, the tile's fc1 bias (whole, not halved); hb, where the packed GELU outputs go; y; xa; lane
    // ---- phase A: one fc1 MFMA of tile t + 1, then bias + GELU of element s of tile t (pairs packed as they complete)
    float4 bv = *reinterpret_cast<const float4*>(bt);
    float gprev = 0.f;
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (!PK) {
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        if constexpr (MORE)
          hnext = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(&wfa[s % FF_PF]),
                                                          *reinterpret_cast<const bf16x8_t*>(&xa[s]), hnext, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (MORE) { if (s + FF_PF < 16) wfa[s % FF_PF] = w1[(s + FF_PF) * 64 + lane]; }
        const float bias = (s & 3) == 0 ? bv.x : (s & 3) == 1 ? bv.y : (s & 3) == 2 ? bv.z : bv.w;
        const float gv = gelu_fast1(hcur[s] + bias);
        if ((s & 3) == 3 && s < 15) bv = *reinterpret_cast<const float4*>(bt + 8 * ((s + 1) >> 2));
        if (s & 1) hb[s >> 1] = cvt_pk_bf16(gprev, gv); else gprev = gv;
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      // packed form: the GELU of an element PAIR (gelu_fast2, the arithmetic of ffn_fused_kernel) in two halves behind two MFMAs --
      // 15 packed instructions + 2 v_rcp per pair instead of 2 x 17 scalar ones (the phase probe of the scalar form: both waves of a
      // SIMD sit in phase A 74 % of the time and their 2 x 21 vector instructions per MFMA, not the matrix cores, pace it)
      f32x2 ph, pha, pq;
#pragma unroll
      for (int sp = 0; sp < 8; ++sp) {
        if constexpr (MORE)
          hnext = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(&wfa[(2 * sp) % FF_PF]),
                                                          *reinterpret_cast<const bf16x8_t*>(&xa[2 * sp]), hnext, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (MORE) { if (2 * sp + FF_PF < 16) wfa[(2 * sp) % FF_PF] = w1[(2 * sp + FF_PF) * 64 + lane]; }
        {
          const f32x2 b2v = (sp & 1) ? f32x2{bv.z, bv.w} : f32x2{bv.x, bv.y};
          const f32x2 xv = f32x2{hcur[2 * sp] + b2v.x, hcur[2 * sp + 1] + b2v.y};
          ph = xv * 0.5f;
          pha = __builtin_elementwise_abs(ph);
          pq = pha * SL_GELU_C5 + SL_GELU_C4;
          pq = pq * pha + SL_GELU_C3;
          pq = pq * pha + SL_GELU_C2;
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (MORE)
          hnext = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(&wfa[(2 * sp + 1) % FF_PF]),
                                                          *reinterpret_cast<const bf16x8_t*>(&xa[2 * sp + 1]), hnext, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (MORE) { if (2 * sp + 1 + FF_PF < 16) wfa[(2 * sp + 1) % FF_PF] = w1[(2 * sp + 1 + FF_PF) * 64 + lane]; }
        {
          pq = pq * pha + SL_GELU_C1;
          pq = pq * pha;
          f32x2 r;
          r.x = __builtin_amdgcn_exp2f(pq.x);
          r.y = __builtin_amdgcn_exp2f(pq.y);
          const f32x2 gv2 = (ph + pha) - pha * r;
          hb[sp] = pack_bf16x2(gv2.x, gv2.y);
          if ((sp & 1) && sp < 7) bv = *reinterpret_cast<const float4*>(bt + 8 * ((sp + 1) >> 1));
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    FP_STAMP(p3);
    // ---- phase B: the 16 fc2 MFMAs of tile t
    {
      uint4 wf[FF_PF];
#pragma unroll
      for (int i = 0; i < FF_PF; ++i) wf[i] = w2[i * 64 + lane];
      const uint4 hb0 = make_uint4(hb[0], hb[1], hb[2], hb[3]), hb1 = make_uint4(hb[4], hb[5], hb[6], hb[7]);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        y[i & 7] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(i < 8 ? &hb0 : &hb1),
                                                           *reinterpret_cast<const bf16x8_t*>(&wf[i % FF_PF]), y[i & 7], 0, 0, 0);
        if (i + FF_PF < 16) wf[i % FF_PF] = w2[(i + FF_PF) * 64 + lane];
      }
    }
#else

__device__ __forceinline__ float gelu_fast1(float x) {
  // gelu_fast2 (common.h), one element: the same operations in the same order
  const float h = x * 0.5f;
  const float a = __builtin_fabsf(h);
  float q = __builtin_fmaf(a, SL_GELU_C5, SL_GELU_C4);
  q = __builtin_fmaf(q, a, SL_GELU_C3);
  q = __builtin_fmaf(q, a, SL_GELU_C2);
  q = __builtin_fmaf(q, a, SL_GELU_C1);
  q = q * a;
  const float e = __builtin_amdgcn_exp2f(q);
  return __builtin_fmaf(-a, e, h + a);
}

#ifdef SL_EXPERIMENTS     // 64 rows per wave, one 4-wave workgroup per compute unit: 0.52-0.54 PFLOP/s against 0.87 (profiles/r04_ffn_bench_wide.json)
// ---------------------------------------------------------------------------------------------------------------------------------------
// WIDE form (round 4, third form): 64 rows per wave -- RT = 2 row tiles of 32 -- in ONE 4-wave workgroup per compute unit (one wave per
// SIMD, 512 registers).  Every weight fragment a wave reads from LDS then feeds TWO MFMAs (one per row tile): the uniform form's third
// budget, the LDS reads of the fragments (8 waves x 32 KB per compute unit and iteration), is halved, and so is the number of waves
// sharing the SIMD's vector issue.  The schedule is the uniform one scaled by RT: per iteration 32 RT MFMAs
//   fc1 of tile t + 1 (16 k-steps x RT)  |  fc2 k-step 0 of tile t (8 column tiles x RT)  |  fc2 k-step 1 of tile t (8 x RT)
// each followed by a quarter of the GELU of one element pair of one row tile: pairs 2 .. 5 of tile t behind the fc1 MFMAs, pairs 6, 7
// behind fc2's k-step 0, pairs 0, 1 of tile t + 1 behind k-step 1 (row tiles alternate inside a pair index).  With one wave per SIMD
// nothing else hides a stall, so the weight rings are four slots deep and tiles are requested two iterations ahead (counted vmcnt).
// fc2's accumulators (RT x 8 x 16 = 256 registers) live in the AGPR half of the file.  Arithmetic and rounding points unchanged.
struct FWG {
  static constexpr int THREADS = 256, NS = 4, AHEAD = 2, PIECES = FP_W / (THREADS * 16);
  static constexpr int LDS = 2 * NS * FP_W + FF_PARAM_BYTES + 2048 * 4;
};

template <int RT>
__global__ __launch_bounds__(256, 1) void ffn_wide_kernel(
    const bf16* __restrict__ X, const float* __restrict__ ln_g, const float* __restrict__ ln_b, const bf16* __restrict__ W1p,
    const float* __restrict__ b1, const bf16* __restrict__ W2p, const float* __restrict__ b2, bf16* __restrict__ out, long M, int F,
    sl_ffn_z) {                                                   // (the launch table's kernel type; no ZOUT in this form)
  constexpr int NS = FWG::NS, AH = FWG::AHEAD;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  char* w1ring = lds;
  char* w2ring = lds + NS * FP_W;
  const Params p = params_at(lds + 2 * NS * FP_W);
  float* const b1s = p.b1s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 31, lh = lane >> 5;
  const long row0 = (long)blockIdx.x * (32 * RT * 4) + wave * (32 * RT);
  const int nt = F / 32;
  const unsigned voff = (unsigned)tid * 16u;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  stage_tile<4>(W1p, 0, w1ring, voff, wave_u);
  stage_tile<4>(W2p, 0, w2ring, voff, wave_u);
#pragma unroll
  for (int a = 1; a <= AH; ++a) {
    if (a < nt) stage_tile<4>(W1p, a, w1ring + (a % NS) * FP_W, voff, wave_u);
    if (a < AH && a < nt) stage_tile<4>(W2p, a, w2ring + (a % NS) * FP_W, voff, wave_u);
  }
  for (int k = tid; k < FF_D; k += 256) { p.lng[k] = ln_g[k]; p.lnb[k] = ln_b[k]; p.b2s[k] = b2[k]; }
  for (int k = tid; k < F; k += 256) b1s[k] = 0.5f * b1[k];                  // half the bias (gelu_q1)
  uint4 xa[RT][16];
#pragma unroll
  for (int r = 0; r < RT; ++r) load_rows(xa[r], X, row0 + r * 32, M, lr, lh);
  __syncthreads();
#pragma unroll
  for (int r = 0; r < RT; ++r) layer_norm_rows(xa[r], p.lng, p.lnb, lh);
  f32x16 y[RT][8];
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int n = 0; n < 8; ++n)
#pragma unroll
      for (int e = 0; e < 16; ++e) y[r][n][e] = 0.f;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  f32x16 hcur[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int e = 0; e < 16; ++e) hcur[r][e] = 0.f;
  {
    const uint4* w1 = reinterpret_cast<const uint4*>(w1ring);
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const uint4 wf = w1[s * 64 + lane];
#pragma unroll
      for (int r = 0; r < RT; ++r)
        hcur[r] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(&wf),
                                                          *reinterpret_cast<const bf16x8_t*>(&xa[r][s]), hcur[r], 0, 0, 0);
    }
  }
  // packed GELU outputs (fc2's A operand) per row tile: [r][0] = elements 0 .. 7 (k-step 0), [r][1] = elements 8 .. 15
  uint4 hbv[RT][2];
  float4 bv_carry;
  {
    const float* bt0 = b1s + 4 * lh;
    const float4 b0 = *reinterpret_cast<const float4*>(bt0);
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      unsigned int* hb = reinterpret_cast<unsigned int*>(hbv[r]);
      GeluPair g0;
      gelu_q1(g0, hcur[r][0], hcur[r][1], b0.x, b0.y); gelu_q2(g0); gelu_q3(g0); hb[0] = gelu_q4(g0);
      gelu_q1(g0, hcur[r][2], hcur[r][3], b0.z, b0.w); gelu_q2(g0); gelu_q3(g0); hb[1] = gelu_q4(g0);
    }
    bv_carry = *reinterpret_cast<const float4*>(bt0 + 8);
  }
  auto iteration = [&](int t, auto more_tag) {
    constexpr bool MORE = decltype(more_tag)::value;
    if (t == 0 || t + AH + 1 > nt) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * FWG::PIECES) : "memory");
    __syncthreads();
    if (t + 1 + AH < nt) stage_tile<4>(W1p, t + 1 + AH, w1ring + ((t + 1 + AH) % NS) * FP_W, voff, wave_u);
    if (t + AH < nt) stage_tile<4>(W2p, t + AH, w2ring + ((t + AH) % NS) * FP_W, voff, wave_u);
    const uint4* w1 = reinterpret_cast<const uint4*>(w1ring + ((t + 1) % NS) * FP_W);    // fc1 weights of tile t + 1
    const uint4* w2 = reinterpret_cast<const uint4*>(w2ring + (t % NS) * FP_W);          // fc2 weights of tile t
    const float* bt = b1s + t * 32 + 4 * lh;
    f32x16 hnext[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
      for (int e = 0; e < 16; ++e) hnext[r][e] = 0.f;
    uint4 wfa[FF_PF];
    if constexpr (MORE) {
#pragma unroll
      for (int i = 0; i < FF_PF; ++i) wfa[i] = w1[i * 64 + lane];
    }
    float4 bv = bv_carry;                                       // half-bias of elements 4 .. 7 (pairs 2, 3)
    GeluPair gp;
    // one quarter of job (pair, row tile) -- q 0 .. 3; src = the fc1 accumulator holding the pair; nxt = bias group to fetch afterwards
    auto quarter = [&](int q, int pair, int r, const f32x16& src, const float* nxt_bias, float4& dst_bias, bool fetch) {
      gelu_quarter(gp, q, pair, src, bv, reinterpret_cast<unsigned int*>(hbv[r]), fetch, nxt_bias, dst_bias);
    };
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 16 * RT; ++k) {                         // fc1 of tile t + 1
      const int s = k / RT, r = k % RT;
      if constexpr (MORE)
        hnext[r] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(&wfa[s % FF_PF]),
                                                           *reinterpret_cast<const bf16x8_t*>(&xa[r][s]), hnext[r], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (MORE) { if (r == RT - 1 && s + FF_PF < 16) wfa[s % FF_PF] = w1[(s + FF_PF) * 64 + lane]; }
      const int j = k / 4, pair = 2 + j / RT, jr = j % RT;      // pairs 2 .. 5 of tile t
      quarter(k % 4, pair, jr, hcur[jr], bt + 8 * ((pair + 1) >> 1), bv, (pair & 1) && jr == RT - 1);
      __builtin_amdgcn_sched_barrier(0);
    }
    uint4 wf[FF_PF];
#pragma unroll
    for (int i = 0; i < FF_PF; ++i) wf[i] = w2[i * 64 + lane];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 16 * RT; ++k) {                         // fc2 of tile t: k-step 0 (i < 8), then k-step 1
      const int i = k / RT, r = k % RT;
      y[r][i & 7] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8_t*>(&hbv[r][i >> 3]),
                                                            *reinterpret_cast<const bf16x8_t*>(&wf[i % FF_PF]), y[r][i & 7], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (r == RT - 1 && i + FF_PF < 16) wf[i % FF_PF] = w2[(i + FF_PF) * 64 + lane];
      if (k < 8 * RT) {
        const int j = k / 4, pair = 6 + j / RT, jr = j % RT;    // pairs 6, 7 of tile t; then the half-bias of tile t + 1, elements 0 .. 3
        quarter(k % 4, pair, jr, hcur[jr], bt + 32, bv, MORE && pair == 7 && jr == RT - 1);
      } else if constexpr (MORE) {
        const int j = (k - 8 * RT) / 4, pair = j / RT, jr = j % RT;   // pairs 0, 1 of tile t + 1: their registers were read by k-step 0
        quarter(k % 4, pair, jr, hnext[jr], bt + 32 + 8, bv_carry, pair == 1 && jr == RT - 1);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (MORE) {
#pragma unroll
      for (int r = 0; r < RT; ++r) hcur[r] = hnext[r];
    }
  };
  for (int t = 0; t + 1 < nt; ++t) iteration(t, std::true_type());
  iteration(nt - 1, std::false_type());
  // ---- epilogue: as ffn_pipe_kernel, 64 rows per wave (4 x 32 KB staging = the 2 * NS weight slots)
  __syncthreads();
#pragma unroll
  for (int r = 0; r < RT; ++r) stage_rows(lds, wave * RT + r, y[r], p.b2s, lr, lh);
  stage_sync();
  store_rows<16 * RT>(lds, wave * RT, X, out, row0, M, lr, lh);
}

#endif  // SL_EXPERIMENTS
#endif  // SL_FFN_PHASE_BODY
