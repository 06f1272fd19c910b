// te_bf16_tile.h -- what the GEMM loops on bf16 operands share (te_bf16.hip: the Linear and attention rules of a bf16 model;
// te_conv_bf16.hip: the z^B rule of its patch embedding): 256 threads stage BR x 32 tiles of bf16 in LDS, four waves read
// them back as fragments of v_mfma_f32_16x16x32_bf16.  Every bf16 x bf16 product is exact in that MFMA's fp32 accumulator.
#pragma once

#include "te_common.h"

typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

constexpr int kThreads = 256;
constexpr int kBK = 32;
constexpr int kLd = kBK + 8;          // LDS row pitch in bf16 elements (80 B: 16-byte aligned rows)

__device__ __forceinline__ float bf(uint16_t b) { return __uint_as_float((unsigned)b << 16); }

// the A / B fragment of lane `lane` for row `row` of a staged tile: 8 consecutive k
__device__ __forceinline__ bf16x8 frag(const uint16_t (*lds)[kLd], int row, int lane) {
  return __builtin_bit_cast(bf16x8, *reinterpret_cast<const u16x8*>(&lds[row][8 * (lane >> 4)]));
}

// (te_common.h's TE_MFMA16 is the fp32 16x16x4 one)
#define TE_MFMA16_BF16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)
