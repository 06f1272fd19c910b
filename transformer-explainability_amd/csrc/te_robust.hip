// te_robust.hip -- robustness and complexity of a relevance map on the device (gfx950), as include/te_relprop.h
// ("robustness and complexity") defines them: the noisy copies of max- / average-sensitivity (Yeh et al., NeurIPS 2019) and of
// the local Lipschitz estimate (Alvarez-Melis & Jaakkola, 2018), the squared distances of B x D pairs of maps or inputs, and
// Gini sparseness (Chalasani et al., ICML 2020), entropy (Bhatt et al., IJCAI 2020) and effective complexity (Nguyen &
// Martinez, 2020) of a map.  The reference tree has no such protocol: the header is the specification, robustness.py restates
// it in numpy / torch.
//
// Three kernels, no host read-back, no memset node, no floating-point atomics:
//   noise      : store-shaped.  A thread owns the Philox groups of 4 (fp32 output) or 8 (bf16) consecutive elements of one
//                sample, reads x once and walks the draws of its block, one Philox4x32-10 call per group and draw (two per
//                16-byte store for bf16), one 16-byte non-temporal store per draw.  The words depend on (element, draw,
//                sample id, seed) alone: not on the batch, the chunk of draws or the grid.
//   distance   : one workgroup of 256 per (sample, draw) pair: thread t takes the groups of four elements t, t + 256, ...,
//                every term in fp64 from the exact upcasts, te_block_sum3 at the end -- an order fixed by n alone, the same
//                for the 16-byte and the element-wise loads.
//   complexity : one workgroup of 1024 per sample on v = |map|: a pass for NaN, S, max and the count of v > 0; a pass for the
//                entropy and the count above eps max; the per-sample radix sort of te_common.h on te_key(v) << 32 | index
//                and a pass over the sorted elements for Gini.  fp64 sums: thread-strided, then te_block_sum3.
#include "te_common.h"

namespace {

constexpr int kThreads = kTeSortThreads;           // complexity
constexpr int kWaves = kTeSortWaves;
constexpr int kDigits = kTeSortDigits;
constexpr int kDistThreads = 256;

// ------------------------------------------------------------------------------------------------ noise
// y = x + (2 u - 1) radius with u = (w >> 8) 2^-24: u and 2 u - 1 are exact, the product and the sum round once each and
// are never contracted into an FMA (torch's x + s * radius)
__device__ __forceinline__ float noisy(float x, uint32_t w, float radius) {
  const float u = (float)(w >> 8) * 0x1p-24f;
  const float s = __fsub_rn(__fmul_rn(2.0f, u), 1.0f);
  return __fadd_rn(x, __fmul_rn(s, radius));
}

// out[b n_d + j][e] = noisy(x[b][e], word e & 3 of philox(e >> 2, d0 + j, id0 + b; seed)).  OutT float: a thread owns 4
// elements, te_bf16_t: 8.  VEC: 16-byte accesses (n a multiple of the thread's elements, aligned bases); else element-wise
// with a guard, which also serves the last, partial group of a row.
template <typename OutT, bool VEC>
__global__ __launch_bounds__(256) void noise_inputs_kernel(const float* __restrict__ x, OutT* __restrict__ out, int64_t n,
                                                           uint32_t d0, int64_t n_d, int dpg, float radius, uint32_t k0,
                                                           uint32_t k1, uint64_t id0) {
  constexpr int E = std::is_same<OutT, float>::value ? 4 : 8;
  const int64_t b = blockIdx.y;
  const int64_t e0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * E;
  if (e0 >= n) return;
  const uint64_t id = id0 + (uint64_t)b;
  const uint32_t id_lo = (uint32_t)id, id_hi = (uint32_t)(id >> 32);
  const float* src = x + b * n + e0;
  float xv[E];
  if constexpr (VEC) {
#pragma unroll
    for (int q = 0; q < E / 4; ++q) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(src + 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j) xv[4 * q + j] = v[j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < E; ++j) xv[j] = (e0 + j < n) ? src[j] : 0.0f;
  }
  const int64_t j0 = (int64_t)blockIdx.z * dpg, j1 = min(n_d, j0 + (int64_t)dpg);      // this block's draws, counted from d0
  for (int64_t j = j0; j < j1; ++j) {
    float y[E];
#pragma unroll
    for (int q = 0; q < E / 4; ++q) {
      uint32_t c[4] = {(uint32_t)((e0 >> 2) + q), d0 + (uint32_t)j, id_lo, id_hi};
      philox4x32_10(c, k0, k1);
#pragma unroll
      for (int i = 0; i < 4; ++i) y[4 * q + i] = noisy(xv[4 * q + i], c[i], radius);
    }
    OutT* dst = out + (b * n_d + j) * n + e0;
    if constexpr (std::is_same<OutT, float>::value) {
      if constexpr (VEC) {
        __builtin_nontemporal_store(f32x4{y[0], y[1], y[2], y[3]}, reinterpret_cast<f32x4*>(dst));
      } else {
#pragma unroll
        for (int i = 0; i < E; ++i)
          if (e0 + i < n) dst[i] = y[i];
      }
    } else {
      if constexpr (VEC) {
        u32x4 p;
#pragma unroll
        for (int i = 0; i < 4; ++i) p[i] = te_pack_bf16(y[2 * i], y[2 * i + 1]);
        __builtin_nontemporal_store(p, reinterpret_cast<u32x4*>(dst));
      } else {
#pragma unroll
        for (int i = 0; i < E; ++i)
          if (e0 + i < n) dst[i] = bf16_bits(y[i]);
      }
    }
  }
}

template <typename OutT>
int noise_inputs(const float* x, OutT* out, int64_t B, int64_t n, int64_t d0, int64_t n_d, float radius, int64_t seed,
                 int64_t id0, hipStream_t stream) {
  if (!x || !out || B <= 0 || n <= 0 || n_d <= 0 || d0 < 0 || !(radius >= 0.0f) || radius > 3.402823466e+38f)
    return TE_ERR_INVALID_ARG;                       // (!(radius >= 0): negative or NaN; above FLT_MAX: infinite)
  if (d0 > ((int64_t)1 << 32) || n_d > ((int64_t)1 << 32) - d0) return TE_ERR_INVALID_ARG;      // draws are 32-bit counters
  if (B > kTeMaxBatch || n > (int64_t)0x7fffffff) return TE_ERR_UNSUPPORTED;
  constexpr int E = std::is_same<OutT, float>::value ? 4 : 8;
  const bool vec = (n % E == 0) && te_aligned16(x) && te_aligned16(out);
  const int64_t bx = te_ceil_div(te_ceil_div(n, E), 256);
  unsigned gz;
  const int64_t dpg = te_draws_per_block(bx * B, n_d, &gz);
  if (dpg > (int64_t)0x7fffffff) return TE_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)bx, (unsigned)B, gz);
  const uint64_t key = (uint64_t)seed;
  if (vec)
    noise_inputs_kernel<OutT, true><<<grid, dim3(256), 0, stream>>>(x, out, n, (uint32_t)d0, n_d, (int)dpg, radius,
                                                                    (uint32_t)key, (uint32_t)(key >> 32), (uint64_t)id0);
  else
    noise_inputs_kernel<OutT, false><<<grid, dim3(256), 0, stream>>>(x, out, n, (uint32_t)d0, n_d, (int)dpg, radius,
                                                                     (uint32_t)key, (uint32_t)(key >> 32), (uint64_t)id0);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

// ------------------------------------------------------------------------------------------------ distance
// sums[b][d] = (sum (y - a)^2, sum a^2, sum y^2) over the n elements of a[b] and y = bb[b][d].  Thread t takes the groups of
// four elements t, t + 256, ... and the elements of a group in order: VEC only changes how they are loaded.
template <typename T, bool VEC>
__global__ __launch_bounds__(kDistThreads) void map_distance_kernel(const float* __restrict__ a, const T* __restrict__ bb,
                                                                    double* __restrict__ sums, int64_t D, int64_t n) {
  __shared__ double red[3 * (kDistThreads / TE_WAVE)];
  const int64_t d = blockIdx.x, b = blockIdx.y;
  const float* xa = a + b * n;
  const T* xb = bb + (b * D + d) * n;
  double sd = 0.0, sa = 0.0, sb = 0.0;
  for (int64_t e0 = (int64_t)threadIdx.x * 4; e0 < n; e0 += (int64_t)kDistThreads * 4) {
    double va[4], vb[4];
    te_load4_f64<VEC>(xa, e0, n, va);
    te_load4_f64<VEC>(xb, e0, n, vb);
#pragma unroll
    for (int j = 0; j < 4; ++j) {                  // (a missing element adds +0.0 to non-negative sums: no bit changes)
      const double df = vb[j] - va[j];
      sd += df * df;
      sa += va[j] * va[j];
      sb += vb[j] * vb[j];
    }
  }
  te_block_sum3(sd, sa, sb, red);
  if (threadIdx.x == 0) {
    double* o = sums + (b * D + d) * 3;
    o[0] = sd;
    o[1] = sa;
    o[2] = sb;
  }
}

template <typename T>
int map_distance(const float* a, const T* b, double* sums, int64_t B, int64_t D, int64_t n, hipStream_t stream) {
  if (!a || !b || !sums || B <= 0 || D <= 0 || n <= 0) return TE_ERR_INVALID_ARG;
  if (B > kTeMaxBatch || D > (int64_t)0x7fffffff || n > (int64_t)0x7fffffff) return TE_ERR_UNSUPPORTED;
  const bool vec = (n % 4 == 0) && te_aligned16(a) && te_aligned16(b);
  const dim3 grid((unsigned)D, (unsigned)B);
  if (vec)
    map_distance_kernel<T, true><<<grid, dim3(kDistThreads), 0, stream>>>(a, b, sums, D, n);
  else
    map_distance_kernel<T, false><<<grid, dim3(kDistThreads), 0, stream>>>(a, b, sums, D, n);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

// ------------------------------------------------------------------------------------------------ complexity
__global__ __launch_bounds__(kThreads) void map_complexity_kernel(const float* __restrict__ maps, double* __restrict__ out,
                                                                  int64_t* __restrict__ counts, uint32_t n, double eps,
                                                                  uint64_t* ws) {
  __shared__ uint32_t cnt[2][kDigits * kWaves];      // [digit][wave]: elements of a digit in a wave's source segment
  __shared__ uint32_t wtot[kWaves];
  __shared__ double red[3 * kWaves];
  __shared__ float wmax[kWaves];
  __shared__ double total[2];                        // S, max v
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t sample = blockIdx.x;
  const float* x = maps + (size_t)sample * n;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double* o = out + sample * 2;
  int64_t* c = counts + sample * 2;

  // ---- S = sum v, max v, the number of v > 0; a NaN anywhere
  double s = 0.0, npos = 0.0, unused = 0.0;      // (a count below 2^20 is exact in fp64, whatever the order)
  float mx = 0.0f;
  int bad = 0;
  for (uint32_t j = tid; j < n; j += kThreads) {
    const float v = fabsf(x[j]);
    bad |= (v != v);
    s += (double)v;
    npos += (v > 0.0f) ? 1.0 : 0.0;
    mx = fmaxf(mx, v);
  }
  if (__syncthreads_or(bad)) {                     // the NaN rule
    if (tid < 2) {
      o[tid] = nan;
      c[tid] = 0;
    }
    return;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, TE_WAVE));
  if (lane == 0) wmax[wave] = mx;
  te_block_sum3(s, npos, unused, red);             // (its barrier covers wmax)
  if (tid == 0) {
    float m = 0.0f;
    for (int w = 0; w < kWaves; ++w) m = fmaxf(m, wmax[w]);
    total[0] = s;
    total[1] = (double)m;
    c[1] = (int64_t)npos;
  }
  __syncthreads();
  const double S = total[0], threshold = eps * total[1];
  if (S == 0.0) {                                  // the zero map (uniform: S is shared)
    if (tid < 2) o[tid] = nan;
    if (tid == 0) c[0] = 0;
    return;
  }

  // ---- entropy -sum p ln p, p = v / S, 0 ln 0 = 0; the number of v > eps max v
  double h = 0.0, above = 0.0;
  for (uint32_t j = tid; j < n; j += kThreads) {
    const double v = (double)fabsf(x[j]);
    above += (v > threshold) ? 1.0 : 0.0;
    if (v > 0.0) {
      const double p = v / S;
      h += p * log(p);
    }
  }
  te_block_sum3(h, above, unused, red);
  if (tid == 0) {
    o[1] = 0.0 - h;
    c[0] = (int64_t)above;
  }

  // ---- sort v ascending
  const TeSortJob job = te_sort_begin(ws, (size_t)sample, n, cnt, tid);
  __syncthreads();
  for (uint32_t j = tid; j < n; j += kThreads) te_sort_put<32>(job, cnt, j, ((uint64_t)te_key(fabsf(x[j])) << 32) | j);
  __syncthreads();
  te_block_sort_passes<32>(job, cnt, wtot, tid, lane, wave);

  // ---- Gini = sum_k (2k - n - 1) v_(k) / (n S), k = j + 1 the 1-based sorted position; every product is exact in fp64
  double g = 0.0;
  for (uint32_t j = tid; j < n; j += kThreads) {
    const float v = __uint_as_float((uint32_t)(job.src[j] >> 32) & 0x7fffffffu);      // te_key of v >= 0 sets the top bit
    g += (double)(2 * (int64_t)j + 1 - (int64_t)n) * (double)v;
  }
  te_block_sum(g, red);
  if (tid == 0) o[0] = g / ((double)n * S);
}

}  // namespace

extern "C" int te_noise_inputs_f32(const float* x, float* out, int64_t B, int64_t n, int64_t d0, int64_t n_d, float radius,
                                   int64_t seed, int64_t id0, te_stream_t stream) {
  return noise_inputs<float>(x, out, B, n, d0, n_d, radius, seed, id0, (hipStream_t)stream);
}

extern "C" int te_noise_inputs_bf16(const float* x, te_bf16_t* out, int64_t B, int64_t n, int64_t d0, int64_t n_d,
                                    float radius, int64_t seed, int64_t id0, te_stream_t stream) {
  return noise_inputs<te_bf16_t>(x, out, B, n, d0, n_d, radius, seed, id0, (hipStream_t)stream);
}

extern "C" int te_map_distance_f32(const float* a, const float* b, double* sums, int64_t B, int64_t D, int64_t n,
                                   te_stream_t stream) {
  return map_distance<float>(a, b, sums, B, D, n, (hipStream_t)stream);
}

extern "C" int te_map_distance_bf16(const float* a, const te_bf16_t* b, double* sums, int64_t B, int64_t D, int64_t n,
                                    te_stream_t stream) {
  return map_distance<te_bf16_t>(a, b, sums, B, D, n, (hipStream_t)stream);
}

extern "C" size_t te_map_complexity_workspace_bytes(int64_t B, int64_t n) {
  if (B <= 0 || n <= 0 || B > kTeMaxBatch || n > kTeMaxSortN) return 0;
  return te_sort_workspace_bytes((size_t)B, (size_t)n);
}

extern "C" int te_map_complexity_f32(const float* maps, double* out, int64_t* counts, int64_t B, int64_t n, double eps,
                                     void* ws, size_t ws_bytes, te_stream_t stream) {
  if (!maps || !out || !counts || B <= 0 || n <= 0 || !(eps >= 0.0) || eps > 1.7976931348623157e308) return TE_ERR_INVALID_ARG;
  if (B > kTeMaxBatch || n > kTeMaxSortN) return TE_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < te_map_complexity_workspace_bytes(B, n)) return TE_ERR_WORKSPACE;
  if (((uintptr_t)ws) & 7u) return TE_ERR_INVALID_ARG;
  map_complexity_kernel<<<dim3((unsigned)B), dim3(kThreads), 0, (hipStream_t)stream>>>(maps, out, counts, (uint32_t)n, eps,
                                                                                        (uint64_t*)ws);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}
