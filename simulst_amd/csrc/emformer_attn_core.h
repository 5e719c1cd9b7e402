// Pieces shared by the matrix-core Emformer attention kernels: the one-tile kernel (emformer_attn_mfma.hip) and the tiled kernel for
// segments of more than 128 keys (emformer_attn_tiled.hip).
#pragma once
#include "common.h"

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef short tr_v4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) tr_v4 lds_v4;

namespace {

constexpr int VR_STRIDE = 96;   // bf16 elements per staged V row (64 channels + pad): 192 B -- rows k, k+1, k+2, k+3 of a
                                // transpose read then start at banks 0, 48, 32, 16 of 64

// two floats -> one register of two bf16 in ONE instruction (hipcc's own lowering of two __float2bfloat16 + shift + or was
// v_cvt_pk_bf16_f32 twice and an SDWA merge)
__device__ __forceinline__ unsigned int pack2(float lo, float hi) {
  unsigned int r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

// 16 bytes at element offset `off` from a uniform base: base in scalar registers, 32-bit lane offset
__device__ __forceinline__ uint4 ld_off(const bf16* base, unsigned off) {
  return *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(base) + (size_t)(off * 2u));
}

}  // namespace
