// te_common.h -- shared device helpers for libte_relprop (gfx950 / CDNA4 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "te_relprop.h"

#define TE_WAVE 64

// Launch-check: kernels are enqueued asynchronously; only launch-configuration errors surface here.
#define TE_RETURN_IF_LAUNCH_FAILED()            \
  do {                                          \
    hipError_t e__ = hipGetLastError();         \
    if (e__ != hipSuccess) return (int)e__;     \
  } while (0)

// Vector types of the kernels.  f32x4_u: a 16-byte access that only promises 4-byte alignment (legal for gfx950 global loads /
// stores; attention rows are N = 197 floats long).
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4_u __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// fp32 MFMAs: exact k-ordered fma chains at the fp32 vector rate (the bf16 ones live in te_x6.h)
#define TE_MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)
#define TE_MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)
// the fp64 MFMA (te_f64.hip): A / B one double per lane, [row = lane & 15][k = lane >> 4]; C / D col = lane & 15,
// row = (lane >> 4) + 4 reg -- not the row map of TE_MFMA16
typedef double f64x4 __attribute__((ext_vector_type(4)));
#define TE_MFMA64(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

// A [B,H,N,D] view with D contiguous: element (b, h, n, d) at base + b sb + h sh + n sn + d, so that q / k / v inside the fused
// qkv activation and the 'b n (h d)' layouts are read and written in place.
struct Strided {
  int64_t sb, sh, sn;
  __device__ __forceinline__ int64_t at(int64_t b, int64_t h, int64_t n) const { return b * sb + h * sh + n * sn; }
};

// row (inside a 32-row block) of accumulator element e of lane half kh (C/D layout of the 32x32 MFMAs: D[i][j], j = lane & 31)
__device__ __forceinline__ int crow(int e, int kh) { return (e & 3) + 8 * (e >> 2) + 4 * kh; }

__device__ __forceinline__ void zero16(f32x16& a) {
#pragma unroll
  for (int e = 0; e < 16; ++e) a[e] = 0.0f;
}

// guarded 4-wide access at a dword-aligned address: elements [c, c+4) of a row with `cols_valid` valid columns
__device__ __forceinline__ f32x4 load4(const float* __restrict__ p, int c, int cols_valid) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (c + 3 < cols_valid) {
    v = *reinterpret_cast<const f32x4_u*>(p + c);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (c + e < cols_valid) v[e] = p[c + e];
  }
  return v;
}
__device__ __forceinline__ void store4(float* __restrict__ p, int c, int cols_valid, f32x4 v) {
  if (c + 3 < cols_valid) {
    *reinterpret_cast<f32x4_u*>(p + c) = v;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (c + e < cols_valid) p[c + e] = v[e];
  }
}

// f(integral_constant<int, I>) for I = I .. END - 1: a loop whose index is a constant expression inside the body
template <int I, int END, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < END) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, END>(f);
  }
}

// nn.GELU, exact erf form (modules/layers_ours.py:70, ViT_LRP.py:57) and its derivative times an incoming gradient: ONE
// definition for the stand-alone producers (te_norm_act.hip) and for the producers that emit operand planes instead of
// fp32 (te_linear_x6.hip), so that both give the same bits.  That is the house rule for every device helper two files need:
// it lives in a header -- here what is not specific to a number format, te_x6.h the split-operand primitives, te_buffer.h buffer
// addressing and the hidden loads -- and tests/test_csrc_shared.py fails on a second definition.
constexpr float kTeInvSqrt2 = 0.70710678118654752440f;
constexpr float kTeInvSqrt2Pi = 0.39894228040143267794f;      // 1 / sqrt(2 pi)
__device__ __forceinline__ float te_gelu(float v) { return (v * 0.5f) * (1.0f + erff(v * kTeInvSqrt2)); }
__device__ __forceinline__ float te_gelu_grad(float g, float v) {
  const float cdf = 0.5f * (1.0f + erff(v * kTeInvSqrt2));
  const float pdf = expf(-0.5f * (v * v)) * kTeInvSqrt2Pi;
  return g * (cdf + v * pdf);
}

// safe_divide of the reference (modules/layers_ours.py:10-13), evaluated exactly as the reference
// does in fp32: den = b + 1e-9 (one rounding), an exact-zero den is replaced by 1e-9, IEEE
// division, then a multiplication by the 0/1 mask (b != 0).  Compiled with -ffp-contract=off.
__device__ __forceinline__ float te_sd(float a, float b) {
  float den = b + 1e-9f;
  den = (den == 0.0f) ? 1e-9f : den;
  float q = a / den;
  return q * ((b != 0.0f) ? 1.0f : 0.0f);
}
// ... and in double (te_f64.hip), as the reference's expression evaluates on double tensors: the same four steps in fp64
__device__ __forceinline__ double te_sd(double a, double b) {
  double den = b + 1e-9;
  den = (den == 0.0) ? 1e-9 : den;
  double q = a / den;
  return q * ((b != 0.0) ? 1.0 : 0.0);
}

// order-preserving key of the radix select (te_perturb.hip) and the radix sort (te_segmetrics.hip):
// a > b (as floats, -0 == +0, NaN largest as in torch.topk) <=> key(a) > key(b)
__device__ __forceinline__ uint32_t te_key(float v) {
  uint32_t u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0;                       // -0 -> +0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ double te_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, TE_WAVE);
  return v;
}

// The radix sorts (te_segmetrics.hip, te_curves.hip, te_block_sort_passes below): the lanes of the wave that hold the same 8-bit digit as this lane, among the `live` ones
__device__ __forceinline__ uint64_t match_digit(uint32_t digit, bool live) {
  uint64_t m = __ballot(live);
#pragma unroll
  for (int bit = 0; bit < 8; ++bit) {
    const bool one = (digit >> bit) & 1u;
    const uint64_t b = __ballot(live && one);
    m &= one ? b : ~b;
  }
  return m;
}

// exclusive prefix of v over the block's threads; wtot: one word of LDS per wave
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* wtot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int off = 1; off < TE_WAVE; off <<= 1) {
    const uint32_t n = __shfl_up(incl, off, TE_WAVE);
    if (lane >= off) incl += n;
  }
  if (lane == TE_WAVE - 1) wtot[wave] = incl;
  __syncthreads();
  uint32_t before = 0;
  for (int w = 0; w < wave; ++w) before += wtot[w];
  __syncthreads();
  return before + incl - v;
}

// The four stable 8-bit passes of the per-sample LSD radix sort (te_mapsim.hip, te_robust.hip), one workgroup of 1024 threads
// = 16 waves: n elements `key << 32 | index` ascending by key, equal keys in index order.  The caller has built src[0 .. n)
// and counted, in cnt[0][digit * 16 + j / S], the elements of every lowest digit in every wave segment of S = ceil(n / 1024)
// * 64 positions, cnt[1] zeroed, a barrier behind it.  A pass turns the (digit, wave) counts into the start of each wave's
// elements of each digit, ranks the lanes of a digit by ballots and counts the next digit at the destination; src and dst
// swap after every pass, so on return src is the caller's first buffer again and holds the sorted elements, dst is idle.
// tid, lane, wave and below = (1 << lane) - 1 are the caller's own values (it needs them before and after the passes).
constexpr int kTeSortThreads = 1024;
constexpr int kTeSortWaves = kTeSortThreads / TE_WAVE;
constexpr int kTeSortDigits = 256;
__device__ __forceinline__ void te_block_sort_passes(uint64_t*& src, uint64_t*& dst, uint32_t n, uint32_t S,
                                                     uint32_t (*cnt)[kTeSortDigits * kTeSortWaves], uint32_t* wtot,
                                                     int tid, int lane, int wave, uint64_t below) {
  for (int pass = 0; pass < 4; ++pass) {
    volatile uint32_t* cur = cnt[pass & 1];
    uint32_t* nxt = cnt[(pass + 1) & 1];
    const int shift = 32 + 8 * pass;
    {                                              // (digit, wave) counts -> start of each wave's elements of each digit
      uint32_t v[4], sum = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[k] = cur[4 * tid + k];
        sum += v[k];
      }
      uint32_t off = block_exclusive_scan(sum, wtot);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        cur[4 * tid + k] = off;
        off += v[k];
      }
      for (int k = 0; k < 4; ++k) nxt[4 * tid + k] = 0;
    }
    __syncthreads();
    const uint32_t seg0 = (uint32_t)wave * S, seg1 = min(seg0 + S, n);
    uint32_t idx = seg0 + lane;
    uint64_t e_next = idx < seg1 ? src[idx] : 0ull;
    for (uint32_t base = seg0; base < seg1; base += TE_WAVE) {
      const uint64_t e = e_next;
      const bool live = idx < seg1;
      idx += TE_WAVE;
      e_next = idx < seg1 ? src[idx] : 0ull;
      const uint32_t digit = (uint32_t)(e >> shift) & 0xffu;
      const uint64_t m = match_digit(digit, live);
      const uint32_t rank = (uint32_t)__popcll(m & below), same = (uint32_t)__popcll(m);
      if (live) {
        const uint32_t at = cur[digit * kTeSortWaves + wave];
        const uint32_t pos = at + rank;
        dst[pos] = e;
        if (rank == same - 1) cur[digit * kTeSortWaves + wave] = at + same;      // after every lane of the digit has read it
        if (pass < 3) atomicAdd(&nxt[((uint32_t)(e >> (shift + 8)) & 0xffu) * kTeSortWaves + pos / S], 1u);
      }
    }
    __syncthreads();
    uint64_t* t = src;
    src = dst;
    dst = t;
  }
}

// Block-wide sum of up to 3 doubles; result valid in thread 0.  `smem` holds 3*(blockDim/64) doubles.
__device__ __forceinline__ void te_block_sum3(double& a, double& b, double& c, double* smem) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  a = te_wave_sum(a);
  b = te_wave_sum(b);
  c = te_wave_sum(c);
  if (lane == 0) {
    smem[wave * 3 + 0] = a;
    smem[wave * 3 + 1] = b;
    smem[wave * 3 + 2] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sa = 0, sb = 0, sc = 0;
    for (int w = 0; w < nw; ++w) {
      sa += smem[w * 3 + 0];
      sb += smem[w * 3 + 1];
      sc += smem[w * 3 + 2];
    }
    a = sa;
    b = sb;
    c = sc;
  }
}

// The counter-based random stream of the noisy copies (te_robust.hip) and of the random subsets (te_faithful.hip).
// Philox4x32-10 (Salmon et al., SC 2011): counter c[4], key (k0, k1) -> c[4]
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0;
    c[1] = lo1;
    c[2] = n2;
    c[3] = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// fp32 -> the bits of the nearest bf16, ties to even (te_robust.hip, te_faithful.hip)
__device__ __forceinline__ uint16_t bf16_bits(float v) {      // to nearest even
  return (uint16_t)(__builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{v, 0.0f}, bf16x2)) & 0xffffu);
}

// Patch geometry of a stride == kernel convolution (ViT patch embedding): row t = (b, py, px) of the im2col matrix,
// column k = (c, dy, dx); te_zb_index maps (t, k) to the element's offset in the NCHW image.
struct TeZbGeom {
  const float* lohi;    // [B][2] per-sample pixel min / max
  int64_t P;            // patches per sample = Hp * Wp
  int C, H, W, p, Wp;
};
__host__ __device__ __forceinline__ int64_t te_zb_index(const TeZbGeom& g, int64_t t, int64_t k) {
  const int64_t b = t / g.P;
  const int tl = (int)(t - b * g.P), py = tl / g.Wp, px = tl - py * g.Wp;
  const int pp = g.p * g.p, c = (int)(k / pp), rem = (int)(k - (int64_t)c * pp), dy = rem / g.p, dx = rem - dy * g.p;
  return ((b * g.C + c) * g.H + (int64_t)py * g.p + dy) * g.W + (int64_t)px * g.p + dx;
}

static inline bool te_aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }
static inline int64_t te_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline size_t te_align_up(size_t a, size_t b) { return (a + b - 1) / b * b; }
