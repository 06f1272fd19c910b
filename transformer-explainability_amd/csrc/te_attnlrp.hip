// te_attnlrp.hip -- the rule kernels of AttnLRP (include/te_relprop.h, section "AttnLRP"): streaming fp32 kernels, no atomics,
// every reduction in an order fixed by the indices alone.  The products of the chain (Linear input gradient, attention backward)
// are the package's existing kernels; what lives here is what sits between them.
// The kernels are templated on the type T of the cached operand (Y, x, gamma, x0): float, or te_bf16_t read exactly (bf16 ->
// fp32 is exact), which changes how an element is loaded and nothing else -- a _bf16 entry gives its _f32 entry's bits on an
// exact fp32 copy of the operand.  G, rstd and every result are fp32 in both.
#include "te_internal.h"
#include "te_x6.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRowsPerBlock = kThreads / TE_WAVE;      // the row kernels: one row per wave
constexpr int64_t kMaxGrid = (int64_t)0x7fffffff;

static inline bool aligned4(const void* p) { return (((uintptr_t)p) & 3u) == 0; }
static inline bool aligned2(const void* p) { return (((uintptr_t)p) & 1u) == 0; }
static inline bool aligned_elem(const float* p) { return aligned4(p); }
static inline bool aligned_elem(const te_bf16_t* p) { return aligned2(p); }
static inline unsigned off16(const void* p) { return (unsigned)(((uintptr_t)p) & 15u); }
// a group of four T on its natural boundary: 16 bytes of fp32, 8 bytes of bf16
static inline bool aligned_group(const float* p) { return te_aligned16(p); }
static inline bool aligned_group(const te_bf16_t* p) { return (((uintptr_t)p) & 7u) == 0; }

// ------------------------------------------------------------------------------------------------ element-wise rules
// damp(g, y): the one definition of te_common.h, shared with te_attnlrp_patch.hip
using DampOp = TeAlrpDamp;
// the identity rule: g (f(x) / x), f'(0) at x == +-0: one IEEE division, one multiply
struct ActOp {
  int kind;
  __device__ __forceinline__ float operator()(float g, float x) const {
    float r;
    if (kind == TE_ALRP_ACT_GELU)
      r = (x == 0.0f) ? 0.5f : te_gelu(x) / x;
    else
      r = (x == 0.0f) ? 1.0f : tanhf(x) / x;
    return g * r;
  }
};

// out[i] = op(a[i], b[i]).  Items 0 .. nvec - 1 are the 16-byte groups that start at element `head`; the items behind them are
// the single elements in front of the first group and behind the last one.  nvec == 0: every element on its own.
template <class T, class Op>
__global__ __launch_bounds__(kThreads) void binary_kernel(const float* a, const T* b, float* out,
                                                           int64_t n, int64_t head, int64_t nvec, Op op) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < nvec) {
    const int64_t e = head + 4 * i;
    const f32x4 va = *reinterpret_cast<const f32x4*>(a + e), vb = te_up4(b + e);
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = op(va[j], vb[j]);
    *reinterpret_cast<f32x4*>(out + e) = r;
    return;
  }
  const int64_t s = i - nvec;
  const int64_t e = (s < head) ? s : s + 4 * nvec;
  if (e < n) out[e] = op(a[e], te_up(b[e]));
}

template <class T, class Op>
int binary_launch(const float* a, const T* b, float* out, int64_t n, Op op, hipStream_t stream) {
  if (!a || !b || !out || n <= 0) return TE_ERR_INVALID_ARG;
  if (!aligned4(a) || !aligned_elem(b) || !aligned4(out)) return TE_ERR_UNSUPPORTED;
  int64_t head = 0, nvec = 0;
  if (off16(a) == off16(out)) {      // one 16-byte phase (of b: its groups on their boundary): vectors from the first boundary on
    head = ((16 - off16(a)) & 15) / 4;
    if (aligned_group(b + head)) {
      if (head > n) head = n;
      nvec = (n - head) / 4;
    } else {
      head = 0;
    }
  }
  const int64_t items = nvec + (n - 4 * nvec);
  const int64_t blocks = te_ceil_div(items, kThreads);
  if (blocks > kMaxGrid) return TE_ERR_UNSUPPORTED;
  binary_kernel<T, Op><<<dim3((unsigned)blocks), dim3(kThreads), 0, stream>>>(a, b, out, n, head, nvec, op);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

// q *= 1/4, k *= 1/4, v *= 1/2 on rows of C elements, row t of each at pointer + t ld.  One item = one element (VEC: four).
template <bool VEC>
__global__ __launch_bounds__(kThreads) void scale3_kernel(float* q, float* k, float* v, int64_t ld, int64_t T, int64_t C) {
  const int64_t per_row = VEC ? C / 4 : C;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= 3 * T * per_row) return;
  const int64_t t = i / (3 * per_row), r = i - t * 3 * per_row;
  const int third = (int)(r / per_row);
  const int64_t c = (r - third * per_row) * (VEC ? 4 : 1);
  float* p = (third == 0 ? q : third == 1 ? k : v) + t * ld + c;
  const float f = (third == 2) ? 0.5f : 0.25f;
  if constexpr (VEC) {
    f32x4 x = *reinterpret_cast<f32x4*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = x[j] * f;
    *reinterpret_cast<f32x4*>(p) = x;
  } else {
    *p = *p * f;
  }
}

// ------------------------------------------------------------------------------------------------ row kernels
// The fp32 row sum of the LayerNorm rule and of the row statistics: lane l adds the terms of the groups l, l + 64, ... (a
// group = four consecutive elements, added in index order) to one accumulator that starts at +0; then the shuffle-down tree
// (offsets 32, 16, .. 1), whose lane 0 holds the sum, which every lane receives.  VEC only changes how a group is loaded.
template <bool VEC, class Term>
__device__ __forceinline__ float wave_row_sum(int lane, int64_t C, Term term) {
  float acc = 0.0f;
  for (int64_t c = (int64_t)lane * 4; c < C; c += TE_WAVE * 4) {
    float t[4];
    term(c, t);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (VEC || c + j < C) acc = acc + t[j];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc = acc + __shfl_down(acc, off, TE_WAVE);
  return __shfl(acc, 0, TE_WAVE);
}

template <bool VEC, class T>
__device__ __forceinline__ void load_group(const T* __restrict__ p, int64_t c, int64_t C, float (&v)[4]) {
  if constexpr (VEC) {
    const f32x4 q = te_up4(p + c);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = q[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (c + j < C) ? te_up(p[c + j]) : 0.0f;
  }
}

template <bool VEC>
__device__ __forceinline__ void store_group(float* p, int64_t c, int64_t C, const float (&v)[4]) {
  if constexpr (VEC) {
    *reinterpret_cast<f32x4*>(p + c) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c + j < C) p[c + j] = v[j];
  }
}

// out[r][i] = rstd[r] (gamma_i G[r][i] - mean_j(gamma_j G[r][j]))
template <bool VEC, class T>
__global__ __launch_bounds__(kThreads) void layernorm_rule_kernel(const float* G, const T* __restrict__ gamma,
                                                                   const float* __restrict__ rstd, float* out, int64_t rows,
                                                                   int64_t C) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float* g = G + r * C;
  float* o = out + r * C;
  auto term = [&](int64_t c, float (&t)[4]) {
    float a[4], w[4];
    load_group<VEC>(g, c, C, a);
    load_group<VEC>(gamma, c, C, w);
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = w[j] * a[j];
  };
  const float mean = wave_row_sum<VEC>(lane, C, term) / (float)C;
  const float rs = rstd[r];
  for (int64_t c = (int64_t)lane * 4; c < C; c += TE_WAVE * 4) {
    float t[4];
    term(c, t);
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = rs * (t[j] - mean);
    store_group<VEC>(o, c, C, t);
  }
}

// rstd[r] = 1 / sqrt(mean_j((x[r][j] - mean_j x[r][j])^2) + eps): the biased variance of nn.LayerNorm, two passes
template <bool VEC, class T>
__global__ __launch_bounds__(kThreads) void row_rstd_kernel(const T* __restrict__ x, float* __restrict__ rstd, int64_t rows,
                                                             int64_t C, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (r >= rows) return;
  const T* xr = x + r * C;
  const float mean = wave_row_sum<VEC>(lane, C, [&](int64_t c, float (&t)[4]) { load_group<VEC>(xr, c, C, t); }) / (float)C;
  const float var = wave_row_sum<VEC>(lane, C, [&](int64_t c, float (&t)[4]) {
    load_group<VEC>(xr, c, C, t);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = t[j] - mean;
      t[j] = d * d;
    }
  }) / (float)C;
  if (lane == 0) rstd[r] = 1.0f / sqrtf(var + eps);
}

// out[b][t - skip] = sum_c x0[b][t][c] G[b][t][c]: exact fp64 products, thread i adds the groups i, i + 64, ... of four
// elements in index order, then te_block_sum; rounded to fp32 once.  One workgroup of one wave per token.
template <bool VEC, class T>
__global__ __launch_bounds__(TE_WAVE) void token_relevance_kernel(const T* __restrict__ x0, const float* __restrict__ G,
                                                                  float* __restrict__ out, int64_t N, int64_t C, int64_t skip) {
  __shared__ double red[1];
  const int64_t row = blockIdx.x, per = N - skip;
  const int64_t b = row / per, t = row - b * per + skip;
  const T* xr = x0 + (b * N + t) * C;
  const float* gr = G + (b * N + t) * C;
  double acc = 0.0;
  for (int64_t e0 = (int64_t)threadIdx.x * 4; e0 < C; e0 += TE_WAVE * 4) {
    double vx[4], vg[4];
    te_load4_f64<VEC>(xr, e0, C, vx);
    te_load4_f64<VEC>(gr, e0, C, vg);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc += vx[j] * vg[j];      // (an element past the end adds +0.0 * +0.0)
  }
  te_block_sum(acc, red);
  if (threadIdx.x == 0) out[row] = (float)acc;
}

// ------------------------------------------------------------------------------------------------ plane passes
// The fp32 operand of a product on bf16 MFMAs (te_bf16.hip) as three exact bf16 planes [3][rows][C] (split3_pk of te_x6.h), plane
// q at planes + q rows C.  One row per wave; lane l takes the groups l, l + 64, ... of four elements.  VEC only changes how a
// group is loaded and stored.
template <bool VEC>
__device__ __forceinline__ void store_planes(uint16_t* planes, int64_t plane_stride, int64_t c, int64_t C, const float (&x)[4]) {
  unsigned lo[3], hi[3];
  split3_pk(x[0], x[1], lo);
  split3_pk(x[2], x[3], hi);
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    uint16_t* p = planes + q * plane_stride + c;
    if constexpr (VEC) {
      *reinterpret_cast<u32x2*>(p) = u32x2{lo[q], hi[q]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c + j < C) p[j] = (uint16_t)(((j < 2) ? lo[q] : hi[q]) >> (16 * (j & 1)));
    }
  }
}

// planes of damp(G, Y) -- te_attnlrp_damp_bf16's bits -- or, DAMP == false, of G itself; row r = (b, h, n) of the strided views
template <bool VEC, bool DAMP>
__global__ __launch_bounds__(kThreads) void damp_planes_kernel(const float* __restrict__ G, Strided gs, const te_bf16_t* __restrict__ Y,
                                                                Strided ys, uint16_t* __restrict__ planes, int64_t H, int64_t N, int64_t C,
                                                                int64_t rows, DampOp op) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int64_t n = r % N, bh = r / N, h = bh % H, b = bh / H;
  const float* g = G + gs.at(b, h, n);
  const te_bf16_t* y = DAMP ? Y + ys.at(b, h, n) : nullptr;
  for (int64_t c = (int64_t)lane * 4; c < C; c += TE_WAVE * 4) {
    float a[4];
    load_group<VEC>(g, c, C, a);
    if constexpr (DAMP) {
      float v[4];
      load_group<VEC>(y, c, C, v);
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = op(a[j], v[j]);
    }
    store_planes<VEC>(planes + r * C, rows * C, c, C, a);
  }
}

// planes of d_s[r][j] = p[r][j] (d[r][j] - s_r), s_r = the fp32 row sum of t_j = d[r][j] p[r][j] (rounded) in wave_row_sum's order
template <bool VEC>
__global__ __launch_bounds__(kThreads) void softmax_bwd_planes_kernel(const float* __restrict__ d_attn, const te_bf16_t* __restrict__ attn,
                                                                       uint16_t* __restrict__ planes, int64_t rows, int64_t N) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float* d = d_attn + r * N;
  const te_bf16_t* p = attn + r * N;
  const float s = wave_row_sum<VEC>(lane, N, [&](int64_t c, float (&t)[4]) {
    float w[4];
    load_group<VEC>(d, c, N, t);
    load_group<VEC>(p, c, N, w);
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = t[j] * w[j];
  });
  for (int64_t c = (int64_t)lane * 4; c < N; c += TE_WAVE * 4) {
    float a[4], w[4];
    load_group<VEC>(d, c, N, a);
    load_group<VEC>(p, c, N, w);
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = w[j] * (a[j] - s);
    store_planes<VEC>(planes + r * N, rows * N, c, N, a);
  }
}

bool finite_not_negative(float v) { return v >= 0.0f && v <= 3.402823466e+38f; }
static inline bool strides4(Strided s) { return s.sb % 4 == 0 && s.sh % 4 == 0 && s.sn % 4 == 0; }

template <class T>
int damp(const float* G, const T* Y, float* out, int64_t n, float eps, hipStream_t stream) {
  if (!finite_not_negative(eps)) return TE_ERR_INVALID_ARG;
  return binary_launch(G, Y, out, n, DampOp{eps}, stream);
}

template <class T>
int act(const float* G, const T* x, float* out, int64_t n, int kind, hipStream_t stream) {
  if (kind != TE_ALRP_ACT_GELU && kind != TE_ALRP_ACT_TANH) return TE_ERR_INVALID_ARG;
  return binary_launch(G, x, out, n, ActOp{kind}, stream);
}

template <class T>
int layernorm(const float* G, const T* gamma, const float* rstd, float* out, int64_t rows, int64_t C, hipStream_t stream) {
  if (!G || !gamma || !rstd || !out || rows <= 0 || C <= 0) return TE_ERR_INVALID_ARG;
  if (!aligned4(G) || !aligned_elem(gamma) || !aligned4(rstd) || !aligned4(out)) return TE_ERR_UNSUPPORTED;
  const int64_t blocks = te_ceil_div(rows, kRowsPerBlock);
  if (blocks > kMaxGrid || C > kMaxGrid) return TE_ERR_UNSUPPORTED;
  const bool vec = C % 4 == 0 && te_aligned16(G) && aligned_group(gamma) && te_aligned16(out);
  if (vec)
    layernorm_rule_kernel<true, T><<<dim3((unsigned)blocks), dim3(kThreads), 0, stream>>>(G, gamma, rstd, out, rows, C);
  else
    layernorm_rule_kernel<false, T><<<dim3((unsigned)blocks), dim3(kThreads), 0, stream>>>(G, gamma, rstd, out, rows, C);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

template <class T>
int row_rstd(const T* x, float* rstd, int64_t rows, int64_t C, float eps, hipStream_t stream) {
  if (!x || !rstd || rows <= 0 || C <= 0 || !finite_not_negative(eps)) return TE_ERR_INVALID_ARG;
  if (!aligned_elem(x) || !aligned4(rstd)) return TE_ERR_UNSUPPORTED;
  const int64_t blocks = te_ceil_div(rows, kRowsPerBlock);
  if (blocks > kMaxGrid || C > kMaxGrid) return TE_ERR_UNSUPPORTED;
  if (C % 4 == 0 && aligned_group(x))
    row_rstd_kernel<true, T><<<dim3((unsigned)blocks), dim3(kThreads), 0, stream>>>(x, rstd, rows, C, eps);
  else
    row_rstd_kernel<false, T><<<dim3((unsigned)blocks), dim3(kThreads), 0, stream>>>(x, rstd, rows, C, eps);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

template <class T>
int token_relevance(const T* x0, const float* G, float* out, int64_t B, int64_t N, int64_t C, int skip_first,
                    hipStream_t stream) {
  if (!x0 || !G || !out || B <= 0 || N <= 0 || C <= 0 || (skip_first != 0 && skip_first != 1) || N - skip_first <= 0)
    return TE_ERR_INVALID_ARG;
  if (!aligned_elem(x0) || !aligned4(G) || !aligned4(out)) return TE_ERR_UNSUPPORTED;
  if (B > kMaxGrid / N || C > kMaxGrid) return TE_ERR_UNSUPPORTED;
  const int64_t rows = B * (N - skip_first);
  if (C % 4 == 0 && aligned_group(x0) && te_aligned16(G))
    token_relevance_kernel<true, T><<<dim3((unsigned)rows), dim3(TE_WAVE), 0, stream>>>(x0, G, out, N, C, skip_first);
  else
    token_relevance_kernel<false, T><<<dim3((unsigned)rows), dim3(TE_WAVE), 0, stream>>>(x0, G, out, N, C, skip_first);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

// ------------------------------------------------------------------------------------------------ a class axis
// te_relprop.h, "AttnLRP, a class axis": G and out are [K, *shape] class-major, the cached operand has `shape` and is read
// once for the K slices.  Slice k of a result has the bits of the kernel above on (G[k], operand): the same operations in the
// same order per element, the same lane order per row.  The part of a rule that does not depend on G is formed once per item.
struct DampClassesOp {      // TeAlrpDamp: st = stab(y) once; per class (g y) / st
  float eps;
  __device__ __forceinline__ float prepare(float y) const { return y + ((y >= 0.0f) ? eps : -eps); }
  __device__ __forceinline__ float operator()(float g, float y, float st) const { return (eps == 0.0f) ? g : (g * y) / st; }
};
struct ActClassesOp {       // ActOp: r = f(x) / x or f'(0) once; per class g r
  int kind;
  __device__ __forceinline__ float prepare(float x) const {
    if (kind == TE_ALRP_ACT_GELU) return (x == 0.0f) ? 0.5f : te_gelu(x) / x;
    return (x == 0.0f) ? 1.0f : tanhf(x) / x;
  }
  __device__ __forceinline__ float operator()(float g, float, float r) const { return g * r; }
};

// out[k][i] = op(a[k][i], b[i]) for k < K: the items of binary_kernel over the n elements of b; slice k of a and out at + k n.
template <class T, class Op>
__global__ __launch_bounds__(kThreads) void binary_classes_kernel(const float* a, const T* b, float* out, int64_t n, int64_t K,
                                                                   int64_t head, int64_t nvec, Op op) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < nvec) {
    const int64_t e = head + 4 * i;
    const f32x4 vb = te_up4(b + e);
    f32x4 pre;
#pragma unroll
    for (int j = 0; j < 4; ++j) pre[j] = op.prepare(vb[j]);
    for (int64_t k = 0; k < K; ++k) {
      const f32x4 va = *reinterpret_cast<const f32x4*>(a + k * n + e);
      f32x4 r;
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = op(va[j], vb[j], pre[j]);
      *reinterpret_cast<f32x4*>(out + k * n + e) = r;
    }
    return;
  }
  const int64_t s = i - nvec;
  const int64_t e = (s < head) ? s : s + 4 * nvec;
  if (e >= n) return;
  const float vb = te_up(b[e]), pre = op.prepare(vb);
  for (int64_t k = 0; k < K; ++k) out[k * n + e] = op(a[k * n + e], vb, pre);
}

template <class T, class Op>
int binary_classes_launch(const float* a, const T* b, float* out, int64_t K, int64_t n, Op op, hipStream_t stream) {
  if (!a || !b || !out || K <= 0 || n <= 0) return TE_ERR_INVALID_ARG;
  if (!aligned4(a) || !aligned_elem(b) || !aligned4(out)) return TE_ERR_UNSUPPORTED;
  if (K > kMaxGrid || n > INT64_MAX / K) return TE_ERR_UNSUPPORTED;
  int64_t head = 0, nvec = 0;
  // binary_launch's phase rule, and every slice on slice 0's phase: the class stride n a multiple of 4 (or one slice)
  if (off16(a) == off16(out) && (K == 1 || n % 4 == 0)) {
    head = ((16 - off16(a)) & 15) / 4;
    if (aligned_group(b + head)) {
      if (head > n) head = n;
      nvec = (n - head) / 4;
    } else {
      head = 0;
    }
  }
  const int64_t items = nvec + (n - 4 * nvec);
  const int64_t blocks = te_ceil_div(items, kThreads);
  if (blocks > kMaxGrid) return TE_ERR_UNSUPPORTED;
  binary_classes_kernel<T, Op><<<dim3((unsigned)blocks), dim3(kThreads), 0, stream>>>(a, b, out, n, K, head, nvec, op);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

// out[k][r][i] = rstd[r] (gamma_i G[k][r][i] - mean_j(gamma_j G[k][r][j])): one wave per operand row r, which walks the K slices;
// per (k, r) the loads, the lane order and the shuffle tree of layernorm_rule_kernel
template <bool VEC, class T>
__global__ __launch_bounds__(kThreads) void layernorm_rule_classes_kernel(const float* G, const T* __restrict__ gamma,
                                                                           const float* __restrict__ rstd, float* out, int64_t K,
                                                                           int64_t rows, int64_t C) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float rs = rstd[r];
  for (int64_t k = 0; k < K; ++k) {
    const float* g = G + (k * rows + r) * C;
    float* o = out + (k * rows + r) * C;
    auto term = [&](int64_t c, float (&t)[4]) {
      float a[4], w[4];
      load_group<VEC>(g, c, C, a);
      load_group<VEC>(gamma, c, C, w);
#pragma unroll
      for (int j = 0; j < 4; ++j) t[j] = w[j] * a[j];
    };
    const float mean = wave_row_sum<VEC>(lane, C, term) / (float)C;
    for (int64_t c = (int64_t)lane * 4; c < C; c += TE_WAVE * 4) {
      float t[4];
      term(c, t);
#pragma unroll
      for (int j = 0; j < 4; ++j) t[j] = rs * (t[j] - mean);
      store_group<VEC>(o, c, C, t);
    }
  }
}

// out[b][k][t - skip] = sum_c x0[b][t][c] G[k][b][t][c]: one workgroup of one wave per token (b, t), which walks the K slices;
// per (k, b, t) the fp64 order of token_relevance_kernel
template <bool VEC, class T>
__global__ __launch_bounds__(TE_WAVE) void token_relevance_classes_kernel(const T* __restrict__ x0, const float* __restrict__ G,
                                                                          float* __restrict__ out, int64_t K, int64_t B, int64_t N,
                                                                          int64_t C, int64_t skip) {
  __shared__ double red[1];
  const int64_t row = blockIdx.x, per = N - skip;
  const int64_t b = row / per, t = row - b * per + skip;
  const T* xr = x0 + (b * N + t) * C;
  for (int64_t k = 0; k < K; ++k) {
    const float* gr = G + ((k * B + b) * N + t) * C;
    double acc = 0.0;
    for (int64_t e0 = (int64_t)threadIdx.x * 4; e0 < C; e0 += TE_WAVE * 4) {
      double vx[4], vg[4];
      te_load4_f64<VEC>(xr, e0, C, vx);
      te_load4_f64<VEC>(gr, e0, C, vg);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc += vx[j] * vg[j];
    }
    te_block_sum(acc, red);      // (one wave: thread 0 alone writes and reads red[0])
    if (threadIdx.x == 0) out[(b * K + k) * per + (t - skip)] = (float)acc;
  }
}

template <class T>
int damp_classes(const float* G, const T* Y, float* out, int64_t K, int64_t n, float eps, hipStream_t stream) {
  if (!finite_not_negative(eps)) return TE_ERR_INVALID_ARG;
  return binary_classes_launch(G, Y, out, K, n, DampClassesOp{eps}, stream);
}

template <class T>
int act_classes(const float* G, const T* x, float* out, int64_t K, int64_t n, int kind, hipStream_t stream) {
  if (kind != TE_ALRP_ACT_GELU && kind != TE_ALRP_ACT_TANH) return TE_ERR_INVALID_ARG;
  return binary_classes_launch(G, x, out, K, n, ActClassesOp{kind}, stream);
}

template <class T>
int layernorm_classes(const float* G, const T* gamma, const float* rstd, float* out, int64_t K, int64_t rows, int64_t C,
                      hipStream_t stream) {
  if (!G || !gamma || !rstd || !out || K <= 0 || rows <= 0 || C <= 0) return TE_ERR_INVALID_ARG;
  if (!aligned4(G) || !aligned_elem(gamma) || !aligned4(rstd) || !aligned4(out)) return TE_ERR_UNSUPPORTED;
  const int64_t blocks = te_ceil_div(rows, kRowsPerBlock);
  if (blocks > kMaxGrid || C > kMaxGrid || K > kMaxGrid || rows > INT64_MAX / C / K) return TE_ERR_UNSUPPORTED;
  const bool vec = C % 4 == 0 && te_aligned16(G) && aligned_group(gamma) && te_aligned16(out);
  if (vec)
    layernorm_rule_classes_kernel<true, T><<<dim3((unsigned)blocks), dim3(kThreads), 0, stream>>>(G, gamma, rstd, out, K, rows, C);
  else
    layernorm_rule_classes_kernel<false, T><<<dim3((unsigned)blocks), dim3(kThreads), 0, stream>>>(G, gamma, rstd, out, K, rows, C);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

template <class T>
int token_relevance_classes(const T* x0, const float* G, float* out, int64_t K, int64_t B, int64_t N, int64_t C, int skip_first,
                            hipStream_t stream) {
  if (!x0 || !G || !out || K <= 0 || B <= 0 || N <= 0 || C <= 0 || (skip_first != 0 && skip_first != 1) || N - skip_first <= 0)
    return TE_ERR_INVALID_ARG;
  if (!aligned_elem(x0) || !aligned4(G) || !aligned4(out)) return TE_ERR_UNSUPPORTED;
  if (B > kMaxGrid / N || C > kMaxGrid || K > kMaxGrid || B * N > INT64_MAX / C / K) return TE_ERR_UNSUPPORTED;
  const int64_t rows = B * (N - skip_first);
  if (C % 4 == 0 && aligned_group(x0) && te_aligned16(G))
    token_relevance_classes_kernel<true, T><<<dim3((unsigned)rows), dim3(TE_WAVE), 0, stream>>>(x0, G, out, K, B, N, C, skip_first);
  else
    token_relevance_classes_kernel<false, T><<<dim3((unsigned)rows), dim3(TE_WAVE), 0, stream>>>(x0, G, out, K, B, N, C, skip_first);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

}  // namespace

int te_alrp::damp_planes_launch(const float* G, Strided gs, const te_bf16_t* Y, Strided ys, uint16_t* planes, int64_t B, int64_t H,
                                int64_t N, int64_t C, float eps, hipStream_t stream) {
  if (!G || !planes || B <= 0 || H <= 0 || N <= 0 || C <= 0 || !finite_not_negative(eps)) return TE_ERR_INVALID_ARG;
  if (!aligned4(G) || (Y && !aligned2(Y)) || !aligned2(planes)) return TE_ERR_UNSUPPORTED;
  const int64_t rows = B * H * N, blocks = te_ceil_div(rows, kRowsPerBlock);
  if (blocks > kMaxGrid || C > kMaxGrid) return TE_ERR_UNSUPPORTED;
  const bool vec = C % 4 == 0 && te_aligned16(G) && strides4(gs) && (!Y || (aligned_group(Y) && strides4(ys))) &&
                   aligned_group(planes);
  const dim3 grid((unsigned)blocks), block(kThreads);
  const DampOp op{eps};
  if (Y && vec)
    damp_planes_kernel<true, true><<<grid, block, 0, stream>>>(G, gs, Y, ys, planes, H, N, C, rows, op);
  else if (Y)
    damp_planes_kernel<false, true><<<grid, block, 0, stream>>>(G, gs, Y, ys, planes, H, N, C, rows, op);
  else if (vec)
    damp_planes_kernel<true, false><<<grid, block, 0, stream>>>(G, gs, Y, ys, planes, H, N, C, rows, op);
  else
    damp_planes_kernel<false, false><<<grid, block, 0, stream>>>(G, gs, Y, ys, planes, H, N, C, rows, op);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

int te_alrp::softmax_bwd_planes_launch(const float* d_attn, const te_bf16_t* p, uint16_t* planes, int64_t rows, int64_t N,
                                       hipStream_t stream) {
  if (!d_attn || !p || !planes || rows <= 0 || N <= 0) return TE_ERR_INVALID_ARG;
  if (!aligned4(d_attn) || !aligned2(p) || !aligned2(planes)) return TE_ERR_UNSUPPORTED;
  const int64_t blocks = te_ceil_div(rows, kRowsPerBlock);
  if (blocks > kMaxGrid || N > kMaxGrid) return TE_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)blocks), block(kThreads);
  if (N % 4 == 0 && te_aligned16(d_attn) && aligned_group(p) && aligned_group(planes))
    softmax_bwd_planes_kernel<true><<<grid, block, 0, stream>>>(d_attn, p, planes, rows, N);
  else
    softmax_bwd_planes_kernel<false><<<grid, block, 0, stream>>>(d_attn, p, planes, rows, N);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

extern "C" int te_alrp_damp_f32(const float* G, const float* Y, float* out, int64_t n, float eps, te_stream_t stream) {
  return damp(G, Y, out, n, eps, (hipStream_t)stream);
}
extern "C" int te_attnlrp_damp_bf16(const float* G, const te_bf16_t* Y, float* out, int64_t n, float eps, te_stream_t stream) {
  return damp(G, Y, out, n, eps, (hipStream_t)stream);
}

extern "C" int te_alrp_act_f32(const float* G, const float* x, float* out, int64_t n, int kind, te_stream_t stream) {
  return act(G, x, out, n, kind, (hipStream_t)stream);
}
extern "C" int te_attnlrp_act_bf16(const float* G, const te_bf16_t* x, float* out, int64_t n, int kind, te_stream_t stream) {
  return act(G, x, out, n, kind, (hipStream_t)stream);
}

extern "C" int te_alrp_scale3_f32(float* q, float* k, float* v, int64_t ld, int64_t T, int64_t C, te_stream_t stream) {
  if (!q || !k || !v || T <= 0 || C <= 0 || ld < C) return TE_ERR_INVALID_ARG;
  if (!aligned4(q) || !aligned4(k) || !aligned4(v)) return TE_ERR_UNSUPPORTED;
  if (T > kMaxGrid || C > kMaxGrid || 3 * T * C > kMaxGrid * kThreads) return TE_ERR_UNSUPPORTED;
  const bool vec = C % 4 == 0 && ld % 4 == 0 && te_aligned16(q) && te_aligned16(k) && te_aligned16(v);
  const int64_t blocks = te_ceil_div(3 * T * (vec ? C / 4 : C), kThreads);
  if (vec)
    scale3_kernel<true><<<dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream>>>(q, k, v, ld, T, C);
  else
    scale3_kernel<false><<<dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream>>>(q, k, v, ld, T, C);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

extern "C" int te_alrp_layernorm_f32(const float* G, const float* gamma, const float* rstd, float* out, int64_t rows, int64_t C,
                                     te_stream_t stream) {
  return layernorm(G, gamma, rstd, out, rows, C, (hipStream_t)stream);
}
extern "C" int te_attnlrp_layernorm_bf16(const float* G, const te_bf16_t* gamma, const float* rstd, float* out, int64_t rows,
                                      int64_t C, te_stream_t stream) {
  return layernorm(G, gamma, rstd, out, rows, C, (hipStream_t)stream);
}

extern "C" int te_alrp_row_rstd_f32(const float* x, float* rstd, int64_t rows, int64_t C, float eps, te_stream_t stream) {
  return row_rstd(x, rstd, rows, C, eps, (hipStream_t)stream);
}
extern "C" int te_attnlrp_row_rstd_bf16(const te_bf16_t* x, float* rstd, int64_t rows, int64_t C, float eps, te_stream_t stream) {
  return row_rstd(x, rstd, rows, C, eps, (hipStream_t)stream);
}

extern "C" int te_alrp_token_relevance_f32(const float* x0, const float* G, float* out, int64_t B, int64_t N, int64_t C,
                                           int skip_first, te_stream_t stream) {
  return token_relevance(x0, G, out, B, N, C, skip_first, (hipStream_t)stream);
}
extern "C" int te_attnlrp_token_relevance_bf16(const te_bf16_t* x0, const float* G, float* out, int64_t B, int64_t N, int64_t C,
                                            int skip_first, te_stream_t stream) {
  return token_relevance(x0, G, out, B, N, C, skip_first, (hipStream_t)stream);
}

// ---- a class axis (te_relprop.h, "AttnLRP, a class axis"): G and out [K, *shape], the operand shared by the K slices
extern "C" int te_alrpk_damp_f32(const float* G, const float* Y, float* out, int64_t K, int64_t n, float eps, te_stream_t stream) {
  return damp_classes(G, Y, out, K, n, eps, (hipStream_t)stream);
}
extern "C" int te_alrpk_damp_bf16(const float* G, const te_bf16_t* Y, float* out, int64_t K, int64_t n, float eps,
                                  te_stream_t stream) {
  return damp_classes(G, Y, out, K, n, eps, (hipStream_t)stream);
}

extern "C" int te_alrpk_act_f32(const float* G, const float* x, float* out, int64_t K, int64_t n, int kind, te_stream_t stream) {
  return act_classes(G, x, out, K, n, kind, (hipStream_t)stream);
}
extern "C" int te_alrpk_act_bf16(const float* G, const te_bf16_t* x, float* out, int64_t K, int64_t n, int kind,
                                 te_stream_t stream) {
  return act_classes(G, x, out, K, n, kind, (hipStream_t)stream);
}

extern "C" int te_alrpk_layernorm_f32(const float* G, const float* gamma, const float* rstd, float* out, int64_t K, int64_t rows,
                                      int64_t C, te_stream_t stream) {
  return layernorm_classes(G, gamma, rstd, out, K, rows, C, (hipStream_t)stream);
}
extern "C" int te_alrpk_layernorm_bf16(const float* G, const te_bf16_t* gamma, const float* rstd, float* out, int64_t K,
                                       int64_t rows, int64_t C, te_stream_t stream) {
  return layernorm_classes(G, gamma, rstd, out, K, rows, C, (hipStream_t)stream);
}

extern "C" int te_alrpk_token_relevance_f32(const float* x0, const float* G, float* out, int64_t K, int64_t B, int64_t N,
                                            int64_t C, int skip_first, te_stream_t stream) {
  return token_relevance_classes(x0, G, out, K, B, N, C, skip_first, (hipStream_t)stream);
}
extern "C" int te_alrpk_token_relevance_bf16(const te_bf16_t* x0, const float* G, float* out, int64_t K, int64_t B, int64_t N,
                                             int64_t C, int skip_first, te_stream_t stream) {
  return token_relevance_classes(x0, G, out, K, B, N, C, skip_first, (hipStream_t)stream);
}
