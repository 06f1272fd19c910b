// te_gradients.hip -- what surrounds the forward / backward loop of the gradient baselines (Input x Gradient, SmoothGrad,
// Integrated Gradients) on the device (gfx950), as include/te_relprop.h ("gradient baselines") defines it.  The reference
// tree has no such methods: the header is the specification, gradients.py restates it in numpy / torch.
//
// Four kernels, no host read-back, no memset node, no atomics:
//   path       : store-shaped.  A thread owns four consecutive elements of one sample, reads x and base once, forms x - base
//                in fp64 and walks the nodes of its block: one fp64 multiply and add, one rounding, one 16-byte (bf16: 8-byte)
//                non-temporal store per node.
//   gauss      : store-shaped.  A thread owns one Philox group of four elements, reads x once and walks the draws of its block:
//                one Philox4x32-10 call and two Box-Muller pairs in fp64 per draw.  The words depend on (element, draw, sample
//                id, seed) alone: not on the batch, the chunk of draws or the grid.
//   accumulate : read-shaped.  A thread owns four consecutive elements of acc, loads them once, walks the n_s gradient rows in
//                order (one fp64 multiply, one fp64 add each) and stores them once.
//   finish     : one workgroup of 1024 per sample.  Thread t takes the pixel pairs t, t + 1024, ..., walks the channels in
//                order, writes the fp32 map and keeps the sample's fp64 sum for te_block_sum.
// Every kernel has a vector form and an element-wise form that visit the same values in the same order.
#include "te_common.h"

namespace {

typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int kThreads = 256;                      // path, gauss, accumulate
constexpr int kFinishThreads = 1024;
constexpr double kTwoPi = 6.283185307179586;       // the fp64 nearest 2 pi: numpy's 2 * np.pi
constexpr uint32_t kGaussStream = 0x40000000u;     // bit 30 of the first counter word: not the noise, not the subset stream

template <typename T>
inline bool on_element_boundary(const T* p) { return (((uintptr_t)p) % sizeof(T)) == 0; }
inline bool aligned8(const void* p) { return (((uintptr_t)p) & 7u) == 0; }

// four fp32 values -> out[0 .. 4) of a row with `valid` elements left (VEC: all four, one store)
template <bool VEC>
__device__ __forceinline__ void store_copy4(float* dst, const float (&y)[4], int64_t valid) {
  if constexpr (VEC) {
    __builtin_nontemporal_store(f32x4{y[0], y[1], y[2], y[3]}, reinterpret_cast<f32x4*>(dst));
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < valid) dst[i] = y[i];
  }
}
template <bool VEC>
__device__ __forceinline__ void store_copy4(te_bf16_t* dst, const float (&y)[4], int64_t valid) {
  if constexpr (VEC) {
    __builtin_nontemporal_store(u32x2{te_pack_bf16(y[0], y[1]), te_pack_bf16(y[2], y[3])}, reinterpret_cast<u32x2*>(dst));
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < valid) dst[i] = bf16_bits(y[i]);
  }
}

template <bool VEC>
__device__ __forceinline__ void load_f32x4(const float* src, int64_t valid, float (&v)[4]) {
  if constexpr (VEC) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(src);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = q[i];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (i < valid) ? src[i] : 0.0f;
  }
}

// ------------------------------------------------------------------------------------------------ path
// out[b n_s + j][e] = (float)(base + alphas[s0 + j] * (x - base)) in fp64, the three operations rounded one by one
template <typename OutT, bool VEC>
__global__ __launch_bounds__(kThreads) void path_inputs_kernel(const float* __restrict__ x, const float* __restrict__ base,
                                                               const float* __restrict__ alphas, OutT* __restrict__ out,
                                                               int64_t n, int64_t s0, int64_t n_s, int spb) {
  const int64_t b = blockIdx.y;
  const int64_t e0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 4;
  if (e0 >= n) return;
  float xv[4], bv[4];
  load_f32x4<VEC>(x + b * n + e0, n - e0, xv);
  load_f32x4<VEC>(base + b * n + e0, n - e0, bv);
  double b64[4], d64[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    b64[i] = (double)bv[i];
    d64[i] = __dsub_rn((double)xv[i], b64[i]);
  }
  const int64_t j0 = (int64_t)blockIdx.z * spb, j1 = min(n_s, j0 + (int64_t)spb);      // this block's nodes, counted from s0
  for (int64_t j = j0; j < j1; ++j) {
    const double a = (double)alphas[s0 + j];
    float y[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = (float)__dadd_rn(b64[i], __dmul_rn(a, d64[i]));
    store_copy4<VEC>(out + (b * n_s + j) * n + e0, y, n - e0);
  }
}

template <typename OutT>
int path_inputs(const float* x, const float* base, const float* alphas, OutT* out, int64_t B, int64_t n, int64_t S, int64_t s0,
                int64_t n_s, hipStream_t stream) {
  if (!x || !base || !alphas || !out || B <= 0 || n <= 0 || S <= 0 || n_s <= 0 || s0 < 0 || n_s > S || s0 > S - n_s)
    return TE_ERR_INVALID_ARG;
  if (!on_element_boundary(x) || !on_element_boundary(base) || !on_element_boundary(alphas) || !on_element_boundary(out))
    return TE_ERR_UNSUPPORTED;
  if (B > kTeMaxBatch || n > (int64_t)0x7fffffff || n_s > (int64_t)0x7fffffff) return TE_ERR_UNSUPPORTED;
  const bool out_ok = std::is_same<OutT, float>::value ? te_aligned16(out) : aligned8(out);
  const bool vec = (n % 4 == 0) && te_aligned16(x) && te_aligned16(base) && out_ok;
  const int64_t bx = te_ceil_div(te_ceil_div(n, 4), kThreads);
  unsigned gz;
  const int64_t spb = te_draws_per_block(bx * B, n_s, &gz);
  const dim3 grid((unsigned)bx, (unsigned)B, gz);
  if (vec)
    path_inputs_kernel<OutT, true><<<grid, dim3(kThreads), 0, stream>>>(x, base, alphas, out, n, s0, n_s, (int)spb);
  else
    path_inputs_kernel<OutT, false><<<grid, dim3(kThreads), 0, stream>>>(x, base, alphas, out, n, s0, n_s, (int)spb);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

// ------------------------------------------------------------------------------------------------ gauss
// the two normals of one pair of words: u = (w + 0.5) 2^-32 is exact in fp64 and lies in (0, 1)
__device__ __forceinline__ void box_muller(uint32_t w0, uint32_t w1, double& z0, double& z1) {
  const double u1 = ((double)w0 + 0.5) * 0x1p-32, u2 = ((double)w1 + 0.5) * 0x1p-32;
  const double r = sqrt(-2.0 * log(u1)), t = kTwoPi * u2;
  z0 = r * cos(t);
  z1 = r * sin(t);
}

// out[b n_d + j][e] = (float)(x[b][e] + sigma z), z from philox(kGaussStream | e >> 2, d0 + j, id0 + b; seed)
template <typename OutT, bool VEC>
__global__ __launch_bounds__(kThreads) void gauss_inputs_kernel(const float* __restrict__ x, OutT* __restrict__ out, int64_t n,
                                                                uint32_t d0, int64_t n_d, int dpb, double sigma, uint32_t k0,
                                                                uint32_t k1, uint64_t id0) {
  const int64_t b = blockIdx.y;
  const int64_t e0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 4;
  if (e0 >= n) return;
  const uint64_t id = id0 + (uint64_t)b;
  float xv[4];
  load_f32x4<VEC>(x + b * n + e0, n - e0, xv);
  const int64_t j0 = (int64_t)blockIdx.z * dpb, j1 = min(n_d, j0 + (int64_t)dpb);      // this block's draws, counted from d0
  for (int64_t j = j0; j < j1; ++j) {
    uint32_t c[4] = {kGaussStream | (uint32_t)(e0 >> 2), d0 + (uint32_t)j, (uint32_t)id, (uint32_t)(id >> 32)};
    philox4x32_10(c, k0, k1);
    double z[4];
    box_muller(c[0], c[1], z[0], z[1]);
    box_muller(c[2], c[3], z[2], z[3]);
    float y[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = (float)__dadd_rn((double)xv[i], __dmul_rn(sigma, z[i]));
    store_copy4<VEC>(out + (b * n_d + j) * n + e0, y, n - e0);
  }
}

template <typename OutT>
int gauss_inputs(const float* x, OutT* out, int64_t B, int64_t n, int64_t d0, int64_t n_d, double sigma, int64_t seed,
                 int64_t id0, hipStream_t stream) {
  if (!x || !out || B <= 0 || n <= 0 || n_d <= 0 || d0 < 0 || !(sigma >= 0.0) || sigma > 1.7976931348623157e308)
    return TE_ERR_INVALID_ARG;                       // (!(sigma >= 0): negative or NaN; above DBL_MAX: infinite)
  if (d0 > ((int64_t)1 << 32) || n_d > ((int64_t)1 << 32) - d0) return TE_ERR_INVALID_ARG;      // draws are 32-bit counters
  if (!on_element_boundary(x) || !on_element_boundary(out)) return TE_ERR_UNSUPPORTED;
  if (B > kTeMaxBatch || n > (int64_t)0x7fffffff || n_d > (int64_t)0x7fffffff) return TE_ERR_UNSUPPORTED;
  const bool out_ok = std::is_same<OutT, float>::value ? te_aligned16(out) : aligned8(out);
  const bool vec = (n % 4 == 0) && te_aligned16(x) && out_ok;
  const int64_t bx = te_ceil_div(te_ceil_div(n, 4), kThreads);
  unsigned gz;
  const int64_t dpb = te_draws_per_block(bx * B, n_d, &gz);
  const dim3 grid((unsigned)bx, (unsigned)B, gz);
  const uint64_t key = (uint64_t)seed;
  if (vec)
    gauss_inputs_kernel<OutT, true><<<grid, dim3(kThreads), 0, stream>>>(x, out, n, (uint32_t)d0, n_d, (int)dpb, sigma,
                                                                         (uint32_t)key, (uint32_t)(key >> 32), (uint64_t)id0);
  else
    gauss_inputs_kernel<OutT, false><<<grid, dim3(kThreads), 0, stream>>>(x, out, n, (uint32_t)d0, n_d, (int)dpb, sigma,
                                                                          (uint32_t)key, (uint32_t)(key >> 32), (uint64_t)id0);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

// ------------------------------------------------------------------------------------------------ accumulate
// acc[b][e] += w[s0 + j] * t(g[b][j][e]) for j = 0 .. n_s - 1 in order; VEC only changes how g and acc are loaded and stored
template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void grad_accumulate_kernel(const T* __restrict__ g, const double* __restrict__ w,
                                                                   double* __restrict__ acc, int64_t n, int64_t n_s, int64_t s0,
                                                                   int square) {
  const int64_t b = blockIdx.y;
  const int64_t e0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 4;
  if (e0 >= n) return;
  double* a = acc + b * n + e0;
  double v[4];
  if constexpr (VEC) {
    const f64x2 lo = *reinterpret_cast<const f64x2*>(a), hi = *reinterpret_cast<const f64x2*>(a + 2);
    v[0] = lo[0], v[1] = lo[1], v[2] = hi[0], v[3] = hi[1];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (e0 + i < n) ? a[i] : 0.0;
  }
  for (int64_t j = 0; j < n_s; ++j) {
    const double wj = w[s0 + j];
    double t[4];
    te_load4_f64<VEC>(g + (b * n_s + j) * n, e0, n, t);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (square) t[i] = __dmul_rn(t[i], t[i]);      // 48 bits at most: exact
      v[i] = __dadd_rn(v[i], __dmul_rn(wj, t[i]));
    }
  }
  if constexpr (VEC) {
    *reinterpret_cast<f64x2*>(a) = f64x2{v[0], v[1]};
    *reinterpret_cast<f64x2*>(a + 2) = f64x2{v[2], v[3]};
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (e0 + i < n) a[i] = v[i];
  }
}

template <typename T>
int grad_accumulate(const T* g, const double* w, double* acc, int64_t B, int64_t n, int64_t n_s, int64_t s0, int square,
                    hipStream_t stream) {
  if (!g || !w || !acc || B <= 0 || n <= 0 || n_s <= 0 || s0 < 0) return TE_ERR_INVALID_ARG;
  if (!on_element_boundary(g) || !on_element_boundary(w) || !on_element_boundary(acc)) return TE_ERR_UNSUPPORTED;
  if (B > kTeMaxBatch || n > (int64_t)0x7fffffff || n_s > (int64_t)0x7fffffff) return TE_ERR_UNSUPPORTED;
  const bool g_ok = std::is_same<T, float>::value ? te_aligned16(g) : aligned8(g);
  const bool vec = (n % 4 == 0) && g_ok && te_aligned16(acc);
  const dim3 grid((unsigned)te_ceil_div(te_ceil_div(n, 4), kThreads), (unsigned)B);
  if (vec)
    grad_accumulate_kernel<T, true><<<grid, dim3(kThreads), 0, stream>>>(g, w, acc, n, n_s, s0, square);
  else
    grad_accumulate_kernel<T, false><<<grid, dim3(kThreads), 0, stream>>>(g, w, acc, n, n_s, s0, square);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

// ------------------------------------------------------------------------------------------------ finish
// v, folded with the term t of the next channel.  MAX_ABS keeps a NaN once it has one (no comparison with a NaN is true).
template <int REDUCE>
__device__ __forceinline__ double fold(double v, double t) {
  if constexpr (REDUCE == TE_GRAD_SUM) return __dadd_rn(v, t);
  const double a = fabs(t);
  if constexpr (REDUCE == TE_GRAD_ABS_SUM) return __dadd_rn(v, a);
  return (a > v || a != a) ? a : v;
}

// out[b][p] = (float)v(p), sums[b] = sum_p v(p).  Thread t takes the pixel pairs t, t + 1024, ...: VEC only changes how a
// pair is loaded and stored; the pixel past the end of an odd row adds +0.0 to the sum, which changes no bit of it (v = +0.0
// there and the running sum is never -0.0: it starts at +0.0).
template <int REDUCE, bool VEC>
__global__ __launch_bounds__(kFinishThreads) void grad_finish_kernel(const double* __restrict__ acc, const float* __restrict__ m,
                                                                     float* __restrict__ out, double* __restrict__ sums,
                                                                     int64_t C, int64_t HW) {
  __shared__ double red[kFinishThreads / TE_WAVE];
  const int64_t b = blockIdx.x;
  const double* a = acc + b * C * HW;
  const float* mb = m ? m + b * C * HW : nullptr;
  double total = 0.0;
  for (int64_t p0 = (int64_t)threadIdx.x * 2; p0 < HW; p0 += (int64_t)kFinishThreads * 2) {
    double v[2] = {0.0, 0.0};
    for (int64_t c = 0; c < C; ++c) {
      double t[2];
      float mv[2] = {1.0f, 1.0f};
      if constexpr (VEC) {
        const f64x2 q = *reinterpret_cast<const f64x2*>(a + c * HW + p0);
        t[0] = q[0], t[1] = q[1];
        if (mb) {
          const f32x2 mq = *reinterpret_cast<const f32x2*>(mb + c * HW + p0);
          mv[0] = mq[0], mv[1] = mq[1];
        }
      } else {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          t[i] = (p0 + i < HW) ? a[c * HW + p0 + i] : 0.0;
          if (mb) mv[i] = (p0 + i < HW) ? mb[c * HW + p0 + i] : 0.0f;
        }
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if (mb) t[i] = __dmul_rn((double)mv[i], t[i]);
        v[i] = fold<REDUCE>(v[i], t[i]);
      }
    }
    if constexpr (VEC) {
      *reinterpret_cast<f32x2*>(out + b * HW + p0) = f32x2{(float)v[0], (float)v[1]};
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (p0 + i < HW) out[b * HW + p0 + i] = (float)v[i];
    }
    total = __dadd_rn(__dadd_rn(total, v[0]), v[1]);
  }
  te_block_sum(total, red);
  if (sums && threadIdx.x == 0) sums[b] = total;
}

template <int REDUCE>
int grad_finish_launch(const double* acc, const float* m, float* out, double* sums, int64_t B, int64_t C, int64_t HW, bool vec,
                       hipStream_t stream) {
  const dim3 grid((unsigned)B);
  if (vec)
    grad_finish_kernel<REDUCE, true><<<grid, dim3(kFinishThreads), 0, stream>>>(acc, m, out, sums, C, HW);
  else
    grad_finish_kernel<REDUCE, false><<<grid, dim3(kFinishThreads), 0, stream>>>(acc, m, out, sums, C, HW);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

}  // namespace

extern "C" int te_path_inputs_f32(const float* x, const float* base, const float* alphas, float* out, int64_t B, int64_t n,
                                  int64_t S, int64_t s0, int64_t n_s, te_stream_t stream) {
  return path_inputs<float>(x, base, alphas, out, B, n, S, s0, n_s, (hipStream_t)stream);
}

extern "C" int te_path_inputs_bf16(const float* x, const float* base, const float* alphas, te_bf16_t* out, int64_t B, int64_t n,
                                   int64_t S, int64_t s0, int64_t n_s, te_stream_t stream) {
  return path_inputs<te_bf16_t>(x, base, alphas, out, B, n, S, s0, n_s, (hipStream_t)stream);
}

extern "C" int te_gauss_inputs_f32(const float* x, float* out, int64_t B, int64_t n, int64_t d0, int64_t n_d, double sigma,
                                   int64_t seed, int64_t id0, te_stream_t stream) {
  return gauss_inputs<float>(x, out, B, n, d0, n_d, sigma, seed, id0, (hipStream_t)stream);
}

extern "C" int te_gauss_inputs_bf16(const float* x, te_bf16_t* out, int64_t B, int64_t n, int64_t d0, int64_t n_d, double sigma,
                                    int64_t seed, int64_t id0, te_stream_t stream) {
  return gauss_inputs<te_bf16_t>(x, out, B, n, d0, n_d, sigma, seed, id0, (hipStream_t)stream);
}

extern "C" int te_grad_accumulate_f32(const float* g, const double* w, double* acc, int64_t B, int64_t n, int64_t n_s,
                                      int64_t s0, int square, te_stream_t stream) {
  return grad_accumulate<float>(g, w, acc, B, n, n_s, s0, square, (hipStream_t)stream);
}

extern "C" int te_grad_accumulate_bf16(const te_bf16_t* g, const double* w, double* acc, int64_t B, int64_t n, int64_t n_s,
                                       int64_t s0, int square, te_stream_t stream) {
  return grad_accumulate<te_bf16_t>(g, w, acc, B, n, n_s, s0, square, (hipStream_t)stream);
}

extern "C" int te_grad_finish_f64(const double* acc, const float* m, float* out, double* sums, int64_t B, int64_t C, int64_t HW,
                                  int reduce, te_stream_t stream) {
  if (!acc || !out || B <= 0 || C <= 0 || HW <= 0) return TE_ERR_INVALID_ARG;
  if (reduce != TE_GRAD_SUM && reduce != TE_GRAD_ABS_SUM && reduce != TE_GRAD_MAX_ABS) return TE_ERR_INVALID_ARG;
  if (!on_element_boundary(acc) || !on_element_boundary(out) || (m && !on_element_boundary(m)) ||
      (sums && !on_element_boundary(sums)))
    return TE_ERR_UNSUPPORTED;
  if (B > kTeMaxBatch || HW > (int64_t)0x7fffffff || C > (int64_t)0x7fffffff) return TE_ERR_UNSUPPORTED;
  const bool vec = (HW % 2 == 0) && te_aligned16(acc) && aligned8(out) && (!m || aligned8(m));
  const hipStream_t s = (hipStream_t)stream;
  switch (reduce) {
    case TE_GRAD_SUM: return grad_finish_launch<TE_GRAD_SUM>(acc, m, out, sums, B, C, HW, vec, s);
    case TE_GRAD_ABS_SUM: return grad_finish_launch<TE_GRAD_ABS_SUM>(acc, m, out, sums, B, C, HW, vec, s);
    default: return grad_finish_launch<TE_GRAD_MAX_ABS>(acc, m, out, sums, B, C, HW, vec, s);
  }
}
