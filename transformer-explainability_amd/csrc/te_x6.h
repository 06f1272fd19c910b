// te_x6.h -- split operands ("x6"): an fp32 product on bf16 MFMAs at fp32 accuracy.  Every fp32 operand is the EXACT sum of three
// bf16 planes; of the nine plane products the six above 2^-24 are kept, summed smallest first in an fp32 accumulator.  The split
// below is the accuracy contract of every x6 kernel (te_linear_x6.hip, te_attn_kb / rc / fwd6 / fwd6l / bwd6l.hip, te_bf16.hip's
// S planes): ONE definition, so that a producer that writes planes and a kernel that splits in registers give the same bits.
#pragma once

#include "te_common.h"

#define TE_MFMA_BF16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)

constexpr int kFrag = 1024;             // bytes of one plane fragment: 32 rows x 16 k bf16 as [kh 2][r 32][8 bf16]

// x = p[0] + p[1] + p[2] exactly: round to nearest even (v_cvt_pk_bf16_f32), subtract (the residual of a round-to-nearest
// bf16 is representable in fp32), repeat.  Pairs: p[q] = the packed bf16 pair (x0 low half, x1 high half) of plane q.
__device__ __forceinline__ void split3_pk(float x0, float x1, unsigned (&p)[3]) {
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const unsigned u = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{x0, x1}, bf16x2));
    p[q] = u;
    x0 = x0 - __uint_as_float(u << 16);
    x1 = x1 - __uint_as_float(u & 0xffff0000u);
  }
}
// one value: p[q] = plane q in the low half
__device__ __forceinline__ void split3(float x, unsigned (&p)[3]) {
  unsigned pk[3];
  split3_pk(x, 0.0f, pk);
#pragma unroll
  for (int q = 0; q < 3; ++q) p[q] = pk[q] & 0xffffu;
}
// eight consecutive K values (K order t = 0..7) -> one MFMA operand fragment per plane
__device__ __forceinline__ void planes_of8(const float (&x)[8], bf16x8 (&b)[3]) {
  unsigned pk[4][3];
#pragma unroll
  for (int t2 = 0; t2 < 4; ++t2) split3_pk(x[2 * t2], x[2 * t2 + 1], pk[t2]);
#pragma unroll
  for (int q = 0; q < 3; ++q) b[q] = __builtin_bit_cast(bf16x8, u32x4{pk[0][q], pk[1][q], pk[2][q], pk[3][q]});
}

// The six partial products in the order they are summed: a[PA[i]] b[PB[i]], i = 0..5
constexpr int PA[6] = {1, 0, 2, 0, 1, 0}, PB[6] = {1, 2, 0, 1, 0, 0};      // planes (1,1) (0,2) (2,0) (0,1) (1,0) (0,0): smallest first
// acc += a b with the six partial products, smallest first
__device__ __forceinline__ void mfma_x6(f32x16& acc, const bf16x8 (&a)[3], const bf16x8 (&b)[3]) {
#pragma unroll
  for (int i = 0; i < 6; ++i) acc = TE_MFMA_BF16(a[PA[i]], b[PB[i]], acc);
}

// safe_divide (te_common.h: te_sd; modules/layers_ours.py:10-13) of two element pairs on packed fp32 instructions: den = b + 1e-9
// (one rounding), an exact-zero den replaced by 1e-9, a / den, zero where b == 0.  The quotient is formed as in the hardware's own
// expansion of an IEEE division without its range scaling (v_rcp_f32, one Newton step on the reciprocal, q = a rc, the exact
// residual r = a - den q by fma, q + r rc): correctly rounded wherever no intermediate leaves the normal range -- |den| >= 1e-16 by
// construction, relevance values and attention scores are far inside it -- at 8 instead of 17 vector instructions per element.
// (te_attn_rc.hip is bound by vector-instruction issue -- phase stamps: profiles/r06_attention_qk_rc_*.log -- and evaluates S twice
// per element; the six-product sums that consume the quotient are re-associated against the reference anyway.)
__device__ __forceinline__ f32x2 sd2(f32x2 a, f32x2 b) {
  f32x2 den = b + f32x2{1e-9f, 1e-9f};
  den[0] = (den[0] == 0.0f) ? 1e-9f : den[0];
  den[1] = (den[1] == 0.0f) ? 1e-9f : den[1];
  f32x2 rc = {__builtin_amdgcn_rcpf(den[0]), __builtin_amdgcn_rcpf(den[1])};
  const f32x2 e = __builtin_elementwise_fma(-den, rc, f32x2{1.0f, 1.0f});
  rc = __builtin_elementwise_fma(e, rc, rc);
  f32x2 q = a * rc;
  const f32x2 r = __builtin_elementwise_fma(-den, q, a);
  q = __builtin_elementwise_fma(r, rc, q);
  q[0] = (b[0] != 0.0f) ? q[0] : 0.0f;
  q[1] = (b[1] != 0.0f) ? q[1] : 0.0f;
  return q;
}

// e / s, correctly rounded wherever no intermediate leaves the normal range (the same expansion; rcs = the refined reciprocal of
// s = a row's sum of exponentials, in [1, N])
__device__ __forceinline__ f32x2 div2(f32x2 e, float s, float rcs) {
  f32x2 q = e * f32x2{rcs, rcs};
  const f32x2 r = __builtin_elementwise_fma(f32x2{-s, -s}, q, e);
  return __builtin_elementwise_fma(r, f32x2{rcs, rcs}, q);
}

// v_permlane32_swap: lanes 32-63 of the first operand <-> lanes 0-31 of the second.  After the call lanes 0-31 hold {own lo_keep,
// partner's lo_keep}; lanes 32-63 hold {partner's hi_keep, own hi_keep}.
__device__ __forceinline__ void swap_halves(unsigned& lo_keep, unsigned& hi_keep) {
  const u32x2 r = __builtin_amdgcn_permlane32_swap(lo_keep, hi_keep, false, false);
  lo_keep = r[0];
  hi_keep = r[1];
}
