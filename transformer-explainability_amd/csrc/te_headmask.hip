// te_headmask.hip -- the head-mask rule and the per-head relevance score (gfx950).
//
//   te_mul_head_relprop_*: Mul.relprop of BertSelfAttention (BERT.py:375-377, RelPropSimple of layers_ours.py:49-61,77-79) for
//                          the operands [attention_probs, head_mask]: one streaming pass, no sums.
//   te_head_relevance_*  : head_relevance[b][h] = sum over (n, d) of the relevance entering an attention layer, in fp64.
#include "te_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 4;                        // 16-byte accesses of one operand in flight per thread

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef double f64x2_u __attribute__((ext_vector_type(2), aligned(8)));
typedef unsigned short u16x4_u __attribute__((ext_vector_type(4), aligned(2)));

// an operand element as the relevance type (bf16 -> fp32 is exact: the upper half of the word)
__device__ __forceinline__ float widen(float x) { return x; }
__device__ __forceinline__ float widen(te_bf16_t x) { return __uint_as_float((unsigned)x << 16); }
__device__ __forceinline__ double widen(double x) { return x; }

// W consecutive elements = 16 bytes of relevance per access; `valid` guards the tail of the span (load4 / store4 of te_common.h)
template <typename TR>
struct Span;

template <>
struct Span<float> {
  static constexpr int W = 4;
  typedef f32x4 V;
  static __device__ __forceinline__ V ld(const float* p, int c, int valid) { return load4(p, c, valid); }
  static __device__ __forceinline__ V ld(const te_bf16_t* p, int c, int valid) {
    V v = {0.f, 0.f, 0.f, 0.f};
    if (c + 3 < valid) {
      const u16x4_u raw = *reinterpret_cast<const u16x4_u*>(p + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = widen((te_bf16_t)raw[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c + e < valid) v[e] = widen(p[c + e]);
    }
    return v;
  }
  static __device__ __forceinline__ void st(float* p, int c, int valid, V v) { store4(p, c, valid, v); }
};

template <>
struct Span<double> {
  static constexpr int W = 2;
  typedef f64x2 V;
  static __device__ __forceinline__ V ld(const double* p, int c, int valid) {
    V v = {0.0, 0.0};
    if (c + 1 < valid) v = *reinterpret_cast<const f64x2_u*>(p + c);
    else if (c < valid) v[0] = p[c];
    return v;
  }
  static __device__ __forceinline__ void st(double* p, int c, int valid, V v) {
    if (c + 1 < valid) *reinterpret_cast<f64x2_u*>(p + c) = v;
    else if (c < valid) p[c] = v[0];
  }
};

// the rule on one element: Z = P m ; S = sd(R, Z) ; out = P (S m), every operation rounded on its own
template <typename T>
__device__ __forceinline__ T mul_rule(T r, T p, T m) {
  const T s = te_sd(r, p * m);
  return p * (s * m);
}

// One workgroup = kChunk consecutive elements of one [rows, cols] plane (flattened grid: plane = blockIdx.x / chunks).  The
// plane's first elements up to the next 16-byte boundary of `out` are single accesses (an odd plane size moves that boundary
// from plane to plane); the rest are 16-byte accesses with a guarded tail.  R and out are not __restrict__: out == R is allowed,
// and every element is read by the thread that writes it, before it writes it.
template <typename TR, typename TP>
__global__ __launch_bounds__(kThreads) void mul_head_kernel(const TR* R, const TP* __restrict__ P, const TP* __restrict__ m,
                                                            int64_t m_sb, TR* out, int64_t H, int64_t n, int64_t chunks) {
  typedef Span<TR> S;
  constexpr int W = S::W;
  constexpr int kChunk = kThreads * W * kUnroll;
  const int64_t plane = blockIdx.x / chunks, chunk = blockIdx.x - plane * chunks;
  const int64_t b = plane / H, h = plane - b * H;
  const TR mv = widen(m[b * m_sb + h]);
  const int64_t p0 = plane * n;
  TR* o = out + p0;
  int64_t head = (W - (int64_t)((reinterpret_cast<uintptr_t>(o) / sizeof(TR)) & (W - 1))) & (W - 1);
  if (head > n) head = n;
  const int64_t body = n - head, c0 = chunk * kChunk;
  if (c0 >= body && !(chunk == 0 && head > 0)) return;
  const int tid = threadIdx.x;
  const bool masked = mv == (TR)0;                       // a masked head: zeros, neither R nor P is read
  if (chunk == 0 && tid < head) o[tid] = masked ? (TR)0 : mul_rule<TR>(R[p0 + tid], widen(P[p0 + tid]), mv);
  if (c0 >= body) return;
  const int valid = (int)((body - c0 < kChunk) ? body - c0 : kChunk);
  o += head + c0;
  if (masked) {
    const typename S::V z = {};
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) S::st(o, (u * kThreads + tid) * W, valid, z);
    return;
  }
  const TR* r = R + p0 + head + c0;
  const TP* p = P + p0 + head + c0;
  typename S::V rv[kUnroll], pv[kUnroll];
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    rv[u] = S::ld(r, (u * kThreads + tid) * W, valid);
    pv[u] = S::ld(p, (u * kThreads + tid) * W, valid);
  }
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    typename S::V ov;
#pragma unroll
    for (int e = 0; e < W; ++e) ov[e] = mul_rule<TR>(rv[u][e], pv[u][e], mv);
    S::st(o, (u * kThreads + tid) * W, valid, ov);
  }
}

template <typename TR, typename TP>
int mul_head_relprop(const TR* R, const TP* P, const TP* m, int64_t m_sb, TR* out, int64_t B, int64_t H, int64_t rows,
                     int64_t cols, te_stream_t stream) {
  if (!R || !P || !m || !out || B <= 0 || H <= 0 || rows <= 0 || cols <= 0 || (m_sb != 0 && m_sb < H))
    return TE_ERR_INVALID_ARG;
  constexpr int64_t kChunk = (int64_t)kThreads * Span<TR>::W * kUnroll;
  if (rows > INT64_MAX / cols) return TE_ERR_UNSUPPORTED;
  const int64_t n = rows * cols, chunks = te_ceil_div(n, kChunk);
  if (B > INT64_MAX / H || B * H > 0x7fffffff / chunks || B * H > INT64_MAX / n) return TE_ERR_UNSUPPORTED;
  mul_head_kernel<TR, TP><<<dim3((unsigned)(B * H * chunks)), dim3(kThreads), 0, (hipStream_t)stream>>>(R, P, m, m_sb, out, H,
                                                                                                      n, chunks);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

// One workgroup per (b, h).  Thread t adds the 4-wide spans t, t + 256, ... of the head's [N, D] slice in that order, each as
// (x0 + x1) + (x2 + x3) in fp64; the wave's shuffle tree and the in-order sum over the waves follow (te_block_sum3).  The order
// depends on (N, D) alone: a call repeated gives the same bits, and a batch equals its samples.
template <typename T>
__global__ __launch_bounds__(kThreads) void head_relevance_kernel(const T* __restrict__ R, Strided s, double* __restrict__ out,
                                                                  int64_t H, int N, int D) {
  __shared__ double red[3 * (kThreads / TE_WAVE)];
  const int64_t b = blockIdx.x / H, h = blockIdx.x - b * H;
  const T* base = R + s.at(b, h, 0);
  double acc = 0.0, z0 = 0.0, z1 = 0.0;
  if constexpr (std::is_same<T, float>::value) {
    const unsigned nv = ((unsigned)D + 3u) / 4u, total = (unsigned)N * nv;
    for (unsigned i = threadIdx.x; i < total; i += kThreads) {
      const unsigned row = i / nv, v = i - row * nv;
      const f32x4 x = load4(base + (int64_t)row * s.sn, (int)(4 * v), D);
      acc += ((double)x[0] + (double)x[1]) + ((double)x[2] + (double)x[3]);
    }
  } else {
    const unsigned total = (unsigned)N * (unsigned)D;
    for (unsigned i = threadIdx.x; i < total; i += kThreads) {
      const unsigned row = i / (unsigned)D, d = i - row * (unsigned)D;
      acc += base[(int64_t)row * s.sn + d];
    }
  }
  te_block_sum3(acc, z0, z1, red);
  if (threadIdx.x == 0) out[blockIdx.x] = acc;
}

template <typename T>
int head_relevance(const T* R, int64_t r_sb, int64_t r_sh, int64_t r_sn, double* out, int64_t B, int64_t H, int64_t N,
                   int64_t D, te_stream_t stream) {
  if (!R || !out || B <= 0 || H <= 0 || N <= 0 || D <= 0 || r_sb < 0 || r_sh < 0 || r_sn < 0 || (N > 1 && r_sn < D))
    return TE_ERR_INVALID_ARG;
  // 32-bit span counters inside one head, one workgroup per head
  if (D > 0x3fffffff || N > 0x7fffffff / (D + 3) || B > 0x7fffffff / H) return TE_ERR_UNSUPPORTED;
  head_relevance_kernel<T><<<dim3((unsigned)(B * H)), dim3(kThreads), 0, (hipStream_t)stream>>>(
      R, Strided{r_sb, r_sh, r_sn}, out, H, (int)N, (int)D);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

}  // namespace

extern "C" int te_mul_head_relprop_f32(const float* R, const float* P, const float* m, int64_t m_sb, float* out, int64_t B,
                                       int64_t H, int64_t rows, int64_t cols, te_stream_t stream) {
  return mul_head_relprop(R, P, m, m_sb, out, B, H, rows, cols, stream);
}

extern "C" int te_mul_head_relprop_bf16(const float* R, const te_bf16_t* P, const te_bf16_t* m, int64_t m_sb, float* out,
                                        int64_t B, int64_t H, int64_t rows, int64_t cols, te_stream_t stream) {
  return mul_head_relprop(R, P, m, m_sb, out, B, H, rows, cols, stream);
}

extern "C" int te_mul_head_relprop_f64(const double* R, const double* P, const double* m, int64_t m_sb, double* out, int64_t B,
                                       int64_t H, int64_t rows, int64_t cols, te_stream_t stream) {
  return mul_head_relprop(R, P, m, m_sb, out, B, H, rows, cols, stream);
}

extern "C" int te_head_relevance_f32(const float* R, int64_t r_sb, int64_t r_sh, int64_t r_sn, double* out, int64_t B,
                                     int64_t H, int64_t N, int64_t D, te_stream_t stream) {
  return head_relevance(R, r_sb, r_sh, r_sn, out, B, H, N, D, stream);
}

extern "C" int te_head_relevance_f64(const double* R, int64_t r_sb, int64_t r_sh, int64_t r_sn, double* out, int64_t B,
                                     int64_t H, int64_t N, int64_t D, te_stream_t stream) {
  return head_relevance(R, r_sb, r_sh, r_sn, out, B, H, N, D, stream);
}
