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

// The one-product Z of the Linear rule (te_linear.hip K1f, te_linear_x6.hip MODE_Z / MODE_ZS / MODE_ZI) is formed from the
// cached forward output, Z = ((Y - b) +- |X||W|^T) / 2, and is only as good as Y - b.  Two things spoil it, and either sends
// the element to the exact k-ordered part sum (exact_z / exact_zi):
//   kCancelTol      |Z| <= 2^-7 |X||W|^T: the two halves cancel (nearly every product has the other sign, or the row is zero);
//   kCancelBiasTol  |Z| <= 2^-4 |b_j|: Y was rounded at the magnitude of X W^T + b, so Y - b carries ~2^-24 |b_j| of absolute
//                   error whatever the size of X W^T (a small row of X, an outlier bias element), i.e. 2^-25 |b_j| / |Z| of
//                   Z after the halving -- 2^-21 at the threshold, a thirtieth of the rule's 2e-5 bar; below it the error
//                   grows without bound (measured 1e-1 for a row of X at 2^-30) while the reference's Z stays exact.
constexpr float kCancelTol = 0.0078125f;
constexpr float kCancelBiasTol = 0.0625f;
// mag = |Z| (Z itself for MODE_Z, -Z' for the inhibitor's Z' <= 0); written so that a NaN falls back too
__device__ __forceinline__ bool te_z_cancels(float mag, float a_abs, float b) {
  return !(mag > kCancelTol * a_abs) || !(mag > kCancelBiasTol * fabsf(b));
}

// The limits the evaluation kernels share: the values of one map (one per-sample sort; te_segmetrics.hip sorts two elements
// per pixel), and the samples of one launch (a grid dimension)
constexpr int64_t kTeMaxSortN = (int64_t)1 << 20;
constexpr int64_t kTeMaxBatch = 65535;

// order-preserving key of the radix selects (te_perturb.hip, te_localise.hip, te_classes.hip) and of the radix sort below:
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
__device__ __forceinline__ uint32_t te_wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, TE_WAVE);
  return v;
}

// te_block_sort_passes below: the lanes of the wave that hold the same 8-bit digit as this lane, among the `live` ones
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

// The per-sample LSD radix sort of the evaluation kernels (te_mapsim.hip, te_robust.hip, te_curves.hip, te_segmetrics.hip),
// one workgroup of 1024 threads = 16 waves per job: n <= 2 kTeMaxSortN 8-byte elements whose 32-bit key starts at bit KEY_BIT
// (32 for `key << 32 | index`, 1 for te_segmetrics.hip's `key << 1 | truth`) come out ascending by key, equal keys in the
// order of their positions.  Four stable passes of 8 bits, ping-pong between the job's two buffers in the workspace (L2).
// Every wave owns a contiguous segment of S = ceil(n / 1024) * 64 source positions; a (digit, wave) table in LDS, scanned
// digit-major, gives each wave its destination per digit, and inside a 64-element step the lanes of one digit are ranked by
// ballots -- so every pass is stable.  The table of the next pass is counted while this pass scatters (integer LDS atomics:
// the counts do not depend on the order of arrival).  A kernel keeps its own key construction and what it does with the
// sorted elements, and writes
//     __shared__ uint32_t cnt[2][kTeSortDigits * kTeSortWaves], wtot[kTeSortWaves];
//     TeSortJob job = te_sort_begin(ws, j, n, cnt, tid);      job j of the launch: its buffers, S, the table zeroed
//     __syncthreads();
//     te_sort_put<KEY_BIT>(job, cnt, pos, element);           every position 0 .. n - 1 once, by whichever thread
//     __syncthreads();
//     te_block_sort_passes<KEY_BIT>(job, cnt, wtot, tid, lane, wave);
// The buffers swap after every pass, so after four job.src, the job's first buffer, holds the sorted elements and job.dst
// is idle.  A wave's segment is [wave S, min(wave S + S, n)) with no min() on its start: n <= 2^21 keeps wave S <=
// 15 * 131072 far inside 32 bits, and a wave whose start is >= n gets the end n, runs no trip and reads nothing.
constexpr int kTeSortThreads = 1024;
constexpr int kTeSortWaves = kTeSortThreads / TE_WAVE;
constexpr int kTeSortDigits = 256;
struct TeSortJob {
  uint64_t *src, *dst;      // n elements each
  uint32_t n, S;
};
__device__ __forceinline__ uint64_t* te_sort_buffers(uint64_t* ws, size_t j, uint32_t n) { return ws + j * 2 * (size_t)n; }
__device__ __forceinline__ TeSortJob te_sort_begin(uint64_t* ws, size_t j, uint32_t n,
                                                   uint32_t (*cnt)[kTeSortDigits * kTeSortWaves], int tid) {
  for (int i = tid; i < 2 * kTeSortDigits * kTeSortWaves; i += kTeSortThreads) (&cnt[0][0])[i] = 0;
  uint64_t* src = te_sort_buffers(ws, j, n);
  return TeSortJob{src, src + n, n, (n + kTeSortThreads - 1) / kTeSortThreads * TE_WAVE};
}
template <int KEY_BIT>
__device__ __forceinline__ void te_sort_put(const TeSortJob& job, uint32_t (*cnt)[kTeSortDigits * kTeSortWaves], uint32_t pos,
                                            uint64_t e) {
  job.src[pos] = e;
  atomicAdd(&cnt[0][((uint32_t)(e >> KEY_BIT) & 0xffu) * kTeSortWaves + pos / job.S], 1u);
}
template <int KEY_BIT>
__device__ __forceinline__ void te_block_sort_passes(const TeSortJob& job, uint32_t (*cnt)[kTeSortDigits * kTeSortWaves],
                                                     uint32_t* wtot, int tid, int lane, int wave) {
  uint64_t *src = job.src, *dst = job.dst;
  const uint32_t n = job.n, S = job.S;
  const uint64_t below = (1ull << lane) - 1;
  for (int pass = 0; pass < 4; ++pass) {
    volatile uint32_t* cur = cnt[pass & 1];
    uint32_t* nxt = cnt[(pass + 1) & 1];
    const int shift = KEY_BIT + 8 * pass;
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

// Block-wide sum of one double; result valid in thread 0.  `smem` holds blockDim/64 doubles.  The order of every fp64 sum of
// the evaluation kernels: te_wave_sum's shuffle-down tree, then the waves in index order in thread 0.
__device__ __forceinline__ void te_block_sum(double& a, double* smem) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  a = te_wave_sum(a);
  if (lane == 0) smem[wave] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    double sa = 0;
    for (int w = 0; w < nw; ++w) sa += smem[w];
    a = sa;
  }
}
// ... and of up to 3 doubles, each in that order.  `smem` holds 3*(blockDim/64) doubles.
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

// bf16 outputs of the evaluation kernels: two fp32 -> the bits of their nearest bf16, ties to even (v_cvt_pk_bf16_f32), a in
// the low half; and of one
__device__ __forceinline__ uint32_t te_pack_bf16(float a, float b) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{a, b}, bf16x2));
}
__device__ __forceinline__ uint16_t bf16_bits(float v) { return (uint16_t)(te_pack_bf16(v, 0.0f) & 0xffffu); }

// fp32 / bf16 operands of the fp64 sums (map_distance, perturbation_dot, curve_scores): element i by its exact upcast ...
__device__ __forceinline__ float te_bf16_up(te_bf16_t v) { return __uint_as_float((uint32_t)v << 16); }
__device__ __forceinline__ double te_load_f64(const float* p, int64_t i) { return (double)p[i]; }
__device__ __forceinline__ double te_load_f64(const te_bf16_t* p, int64_t i) { return (double)te_bf16_up(p[i]); }
// ... and the group of four consecutive elements e0 .. e0 + 3 of p[0 .. n).  VEC: one 16-byte (fp32) or 8-byte (bf16) access
// -- the group lies inside the row and on that boundary; otherwise element by element, 0.0 for an element past the end.  The
// values and their order are the same either way, so a sum over them has the same bits.
template <bool VEC, typename T, typename I>
__device__ __forceinline__ void te_load4_f64(const T* __restrict__ p, I e0, I n, double (&v)[4]) {
  if constexpr (!VEC) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (e0 + j < n) ? te_load_f64(p, e0 + j) : 0.0;
  } else if constexpr (std::is_same<T, float>::value) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(p + e0);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (double)q[j];
  } else {
    const u32x2 q = *reinterpret_cast<const u32x2*>(p + e0);
#pragma unroll
    for (int j = 0; j < 2; ++j) {                  // element 2j in the low half
      v[2 * j] = (double)__uint_as_float(q[j] << 16);
      v[2 * j + 1] = (double)__uint_as_float(q[j] & 0xffff0000u);
    }
  }
}

// fp32 / bf16 operands of the fp32 rules (te_attnlrp.hip, te_attnlrp_patch.hip): one element as fp32, and four consecutive
// ones in one access (element 2j of a bf16 pair in the low half)
__device__ __forceinline__ float te_up(float v) { return v; }
__device__ __forceinline__ float te_up(te_bf16_t v) { return te_bf16_up(v); }
__device__ __forceinline__ f32x4 te_up4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 te_up4(const te_bf16_t* p) {
  const u32x2 q = *reinterpret_cast<const u32x2*>(p);
  return f32x4{__uint_as_float(q[0] << 16), __uint_as_float(q[0] & 0xffff0000u), __uint_as_float(q[1] << 16),
               __uint_as_float(q[1] & 0xffff0000u)};
}

// AttnLRP (te_relprop.h, section "AttnLRP"): stab(y) = y + eps sgn(y), sgn(+-0) = +1; damp = (g y) / stab(y): one multiply, one
// add, one IEEE division.  eps == 0: g itself.  te_alrp_damp_f32's bits wherever a kernel damps while it stages.
struct TeAlrpDamp {
  float eps;
  __device__ __forceinline__ float operator()(float g, float y) const {
    if (eps == 0.0f) return g;
    const float st = y + ((y >= 0.0f) ? eps : -eps);
    return (g * y) / st;
  }
};

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

// the workspace of `jobs` sorts of n elements (te_sort_begin): two buffers of n 8-byte elements each
static inline size_t te_sort_workspace_bytes(size_t jobs, size_t n) { return te_align_up(jobs * 2 * n * sizeof(uint64_t), 256); }

// The per-channel constants of the kernels that write model inputs (te_perturb.hip, te_curves.hip, te_faithful.hip), passed
// by value: normalisation z = (x - mean[c]) / std[c] and the substrate's constant fill[c]; a null array gives 0 / 1 / 0.  A
// kernel reads the members it needs: the others cost nothing but bytes of its argument block.
struct TeChannels {
  float mean[TE_PERTURB_MAX_CHANNELS], std[TE_PERTURB_MAX_CHANNELS], fill[TE_PERTURB_MAX_CHANNELS];
};
static inline TeChannels te_channels(int64_t C, const float* mean, const float* std_, const float* fill) {
  TeChannels ch;
  for (int c = 0; c < TE_PERTURB_MAX_CHANNELS; ++c) {
    ch.mean[c] = (mean && c < C) ? mean[c] : 0.0f;
    ch.std[c] = (std_ && c < C) ? std_[c] : 1.0f;
    ch.fill[c] = (fill && c < C) ? fill[c] : 0.0f;
  }
  return ch;
}

// The launch shape of the kernels that write n_d random copies of every sample (te_robust.hip, te_faithful.hip): all draws
// of the call inside one thread once the `blocks` = B * bx workgroups of one draw fill the chip (256 CUs x 4 resident
// blocks), else one draw per workgroup -- more where the grid's z would pass 65535.  -> draws per workgroup, *grid_z
static inline int64_t te_draws_per_block(int64_t blocks, int64_t n_d, unsigned* grid_z) {
  int64_t dpg = (blocks >= 1024) ? n_d : 1;
  if (te_ceil_div(n_d, dpg) > 65535) dpg = te_ceil_div(n_d, 65535);
  *grid_z = (unsigned)te_ceil_div(n_d, dpg);
  return dpg;
}
