// te_faithful.hip -- faithfulness of a relevance map under random perturbations on the device (gfx950), as
// include/te_relprop.h ("faithfulness") defines it: the random subsets of patches and the perturbed images of the
// faithfulness correlation (Bhatt et al., IJCAI 2020), and the weighted sums `perturbation . attribution` of infidelity (Yeh
// et al., NeurIPS 2019).  The reference tree has no such protocol: the header is the specification, faithfulness.py restates
// it in numpy / torch.
//
// Three kernels, no host read-back, no memset node, no floating-point atomics:
//   select  : one workgroup of 256 per (sample, draw).  The G <= 4096 keys `philox word << 32 | cell` go to LDS (one Philox
//             call per four cells); a thread then ranks its cells t, t + 256, ... by counting the smaller keys (every lane
//             reads the same LDS address: a broadcast) and writes member = rank < k.  attr_sum: the thread's own cells in
//             order, then te_block_sum -- an order fixed by G alone.
//   compose : store-shaped, the form of noise_inputs_kernel.  A thread owns 4 (fp32 output) or 8 (bf16) consecutive elements
//             of one sample -- one cell when p is a multiple of that --, reads x and the substrate once and walks the draws
//             of its block: one member byte and one 16-byte non-temporal store per draw.  Element-wise otherwise.
//   dot     : map_distance_kernel's loop with a weight: one workgroup of 256 per (sample, draw), thread t takes the groups of
//             four elements t, t + 256, ..., every term in fp64 from the exact upcasts, te_block_sum3 at the end.
#include "te_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int64_t kMaxCells = TE_SUBSET_MAX_CELLS;
constexpr int64_t kMaxInt = 0x7fffffff;
constexpr int kMaxC = TE_PERTURB_MAX_CHANNELS;

// ------------------------------------------------------------------------------------------------ select
// member[b][j][c] = (the rank of key_c among the G keys of draw d0 + j of sample id0 + b) < k;
// attr_sum[b][j] = sum over the members of (double)attr[b][c]
__global__ __launch_bounds__(kThreads) void subset_select_kernel(const float* __restrict__ attr, uint8_t* __restrict__ member,
                                                                 double* __restrict__ attr_sum, uint32_t G, uint32_t k,
                                                                 uint32_t d0, int64_t n_d, uint32_t k0, uint32_t k1,
                                                                 uint64_t id0) {
  __shared__ uint64_t keys[kMaxCells];
  __shared__ double red[3 * (kThreads / TE_WAVE)];
  const int64_t j = blockIdx.x, b = blockIdx.y;
  const uint32_t tid = threadIdx.x;
  const uint64_t id = id0 + (uint64_t)b;
  for (uint32_t q = tid; 4 * q < G; q += kThreads) {
    uint32_t c[4] = {0x80000000u | q, d0 + (uint32_t)j, (uint32_t)id, (uint32_t)(id >> 32)};
    philox4x32_10(c, k0, k1);
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i)
      if (4 * q + i < G) keys[4 * q + i] = ((uint64_t)c[i] << 32) | (uint64_t)(4 * q + i);
  }
  __syncthreads();
  uint8_t* mrow = member + (b * n_d + j) * (int64_t)G;
  double s = 0.0;
  for (uint32_t cell = tid; cell < G; cell += kThreads) {
    const uint64_t key = keys[cell];
    uint32_t rank = 0;
    for (uint32_t o = 0; o < G; ++o) rank += (keys[o] < key) ? 1u : 0u;
    const bool in = rank < k;
    mrow[cell] = in ? 1 : 0;
    if (attr != nullptr && in) s += (double)attr[b * (int64_t)G + cell];
  }
  if (attr != nullptr) {                             // (uniform: the barrier inside is reached by all or by none)
    te_block_sum(s, red);
    if (tid == 0) attr_sum[b * n_d + j] = s;
  }
}

// ------------------------------------------------------------------------------------------------ compose
// out[b][j][e] = member[b][j][cell(e)] ? sub[e] : x[b][e], e = (c, row, col) of the [C,H,W] image, cell = (row / p) g_w +
// col / p, sub = substrate[b][e] or fill[c].  OutT float: VEC 4 or 1; te_bf16_t: VEC 8 or 1, the value rounded once.
template <typename OutT, int VEC>
__global__ __launch_bounds__(256) void subset_inputs_kernel(const float* __restrict__ x, const float* __restrict__ substrate,
                                                            const uint8_t* __restrict__ member, OutT* __restrict__ out,
                                                            uint32_t n, uint32_t HW, uint32_t W, uint32_t p, uint32_t g_w,
                                                            uint32_t G, int64_t n_d, int dpg, TeChannels ch) {
  const int64_t b = blockIdx.y;
  const int64_t e0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC;
  if (e0 >= (int64_t)n) return;
  const uint32_t e = (uint32_t)e0, c = e / HW, pix = e - c * HW, row = pix / W, col = pix - row * W;
  const uint32_t cell = (row / p) * g_w + col / p;   // (VEC > 1: p % VEC == 0, the thread's elements share the cell)
  const float* src = x + b * (int64_t)n + e0;
  const float fv = substrate ? 0.0f : ch.fill[c];    // (constants: C <= kMaxC; with a tensor c may be larger and is not used)
  float xv[VEC], sv[VEC];
  if constexpr (VEC == 1) {
    xv[0] = src[0];
    sv[0] = substrate ? substrate[b * (int64_t)n + e0] : fv;
  } else {
#pragma unroll
    for (int q = 0; q < VEC / 4; ++q) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(src + 4 * q);
      f32x4 s = {fv, fv, fv, fv};
      if (substrate) s = *reinterpret_cast<const f32x4*>(substrate + b * (int64_t)n + e0 + 4 * q);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        xv[4 * q + i] = v[i];
        sv[4 * q + i] = s[i];
      }
    }
  }
  const int64_t j0 = (int64_t)blockIdx.z * dpg, j1 = min(n_d, j0 + (int64_t)dpg);      // this block's draws, counted from d0
  for (int64_t j = j0; j < j1; ++j) {
    const bool in = member[(b * n_d + j) * (int64_t)G + cell] != 0;
    float y[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) y[i] = in ? sv[i] : xv[i];
    OutT* dst = out + (b * n_d + j) * (int64_t)n + e0;
    if constexpr (std::is_same<OutT, float>::value) {
      if constexpr (VEC == 4)
        __builtin_nontemporal_store(f32x4{y[0], y[1], y[2], y[3]}, reinterpret_cast<f32x4*>(dst));
      else
        dst[0] = y[0];
    } else {
      if constexpr (VEC == 8) {
        u32x4 pk;
#pragma unroll
        for (int i = 0; i < 4; ++i) pk[i] = te_pack_bf16(y[2 * i], y[2 * i + 1]);
        __builtin_nontemporal_store(pk, reinterpret_cast<u32x4*>(dst));
      } else {
        dst[0] = bf16_bits(y[0]);
      }
    }
  }
}

template <typename OutT>
int subset_inputs(const float* x, const float* substrate, const float* fill, const float* attr, OutT* out, uint8_t* member,
                  double* attr_sum, int64_t B, int64_t C, int64_t g_h, int64_t g_w, int64_t p, int64_t k, int64_t d0,
                  int64_t n_d, int64_t seed, int64_t id0, hipStream_t stream) {
  if (!x || !out || !member || (!substrate && !fill) || (attr && !attr_sum) || B <= 0 || C <= 0 || g_h <= 0 || g_w <= 0 ||
      p <= 0 || n_d <= 0 || d0 < 0 || k < 1)
    return TE_ERR_INVALID_ARG;
  if (d0 > ((int64_t)1 << 32) || n_d > ((int64_t)1 << 32) - d0) return TE_ERR_INVALID_ARG;      // draws are 32-bit counters
  if (g_h <= kMaxCells && g_w <= kMaxCells && k > g_h * g_w) return TE_ERR_INVALID_ARG;
  if (g_h > kMaxCells || g_w > kMaxCells || g_h * g_w > kMaxCells || B > kTeMaxBatch || n_d > kMaxInt) return TE_ERR_UNSUPPORTED;
  const int64_t G = g_h * g_w;
  if (p > kMaxInt || p * p > kMaxInt || C > kMaxInt || G * p * p > kMaxInt || C * G * p * p > kMaxInt)
    return TE_ERR_UNSUPPORTED;                       // (every product is formed after its factors are known to be small)
  if (!substrate && C > kMaxC) return TE_ERR_UNSUPPORTED;
  const int64_t W = g_w * p, HW = G * p * p, n = C * HW;
  const uint64_t key = (uint64_t)seed;
  subset_select_kernel<<<dim3((unsigned)n_d, (unsigned)B), dim3(kThreads), 0, stream>>>(
      attr, member, attr_sum, (uint32_t)G, (uint32_t)k, (uint32_t)d0, n_d, (uint32_t)key, (uint32_t)(key >> 32), (uint64_t)id0);
  TE_RETURN_IF_LAUNCH_FAILED();
  const TeChannels f = te_channels(C, nullptr, nullptr, fill);
  constexpr int V = std::is_same<OutT, float>::value ? 4 : 8;
  const bool vec = (p % V == 0) && te_aligned16(x) && te_aligned16(out) && (!substrate || te_aligned16(substrate));
  const int64_t bx = te_ceil_div(vec ? n / V : n, 256);
  unsigned gz;
  const int64_t dpg = te_draws_per_block(bx * B, n_d, &gz);      // (<= n_d <= kMaxInt)
  const dim3 grid((unsigned)bx, (unsigned)B, gz);
  if (vec)
    subset_inputs_kernel<OutT, V><<<grid, dim3(256), 0, stream>>>(x, substrate, member, out, (uint32_t)n, (uint32_t)HW,
                                                                  (uint32_t)W, (uint32_t)p, (uint32_t)g_w, (uint32_t)G, n_d,
                                                                  (int)dpg, f);
  else
    subset_inputs_kernel<OutT, 1><<<grid, dim3(256), 0, stream>>>(x, substrate, member, out, (uint32_t)n, (uint32_t)HW,
                                                                  (uint32_t)W, (uint32_t)p, (uint32_t)g_w, (uint32_t)G, n_d,
                                                                  (int)dpg, f);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

// ------------------------------------------------------------------------------------------------ dot
// sums[b][d] = (sum (x - y) w[e mod m], sum (x - y)^2) over the n elements of x[b] and y = yy[b][d].  Thread t takes the groups
// of four elements t, t + 256, ... and the elements of a group in order: VEC only changes how they are loaded (VEC: m % 4 ==
// 0, so that a group's weights are consecutive).
template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void perturbation_dot_kernel(const float* __restrict__ x, const T* __restrict__ yy,
                                                                    const float* __restrict__ w, double* __restrict__ sums,
                                                                    int64_t D, uint32_t n, uint32_t m) {
  __shared__ double red[3 * (kThreads / TE_WAVE)];
  const int64_t d = blockIdx.x, b = blockIdx.y;
  const float* xa = x + b * (int64_t)n;
  const T* yb = yy + (b * D + d) * (int64_t)n;
  const float* wb = w + b * (int64_t)m;
  double sw = 0.0, sq = 0.0, unused = 0.0;
  uint32_t wi = (threadIdx.x * 4u) % m;            // (e0 mod m, kept up to date without a division per group)
  const uint32_t wstep = (kThreads * 4u) % m;
  for (uint32_t e0 = threadIdx.x * 4u; e0 < n; e0 += kThreads * 4u) {
    double va[4], vb[4], vw[4];
    te_load4_f64<VEC>(xa, e0, n, va);              // (n <= 2^31 - 1 and e0 < n: e0 + 3 does not wrap)
    te_load4_f64<VEC>(yb, e0, n, vb);
    if constexpr (VEC) {
      te_load4_f64<true>(wb, wi, m, vw);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) vw[j] = (e0 + j < n) ? (double)wb[(wi + j) % m] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double df = va[j] - vb[j];
      sw += df * vw[j];
      sq += df * df;
    }
    wi += wstep;
    if (wi >= m) wi -= m;
  }
  te_block_sum3(sw, sq, unused, red);
  if (threadIdx.x == 0) {
    double* o = sums + (b * D + d) * 2;
    o[0] = sw;
    o[1] = sq;
  }
}

template <typename T>
int perturbation_dot(const float* x, const T* y, const float* w, double* sums, int64_t B, int64_t D, int64_t n, int64_t m,
                     hipStream_t stream) {
  if (!x || !y || !w || !sums || B <= 0 || D <= 0 || n <= 0 || m <= 0 || n % m != 0) return TE_ERR_INVALID_ARG;
  if (B > kTeMaxBatch || D > kMaxInt || n > kMaxInt) return TE_ERR_UNSUPPORTED;
  const bool vec = (n % 4 == 0) && (m % 4 == 0) && te_aligned16(x) && te_aligned16(y) && te_aligned16(w);
  const dim3 grid((unsigned)D, (unsigned)B);
  if (vec)
    perturbation_dot_kernel<T, true><<<grid, dim3(kThreads), 0, stream>>>(x, y, w, sums, D, (uint32_t)n, (uint32_t)m);
  else
    perturbation_dot_kernel<T, false><<<grid, dim3(kThreads), 0, stream>>>(x, y, w, sums, D, (uint32_t)n, (uint32_t)m);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

}  // namespace

extern "C" int te_subset_inputs_f32(const float* x, const float* substrate, const float* fill, const float* attr, float* out,
                                    uint8_t* member, double* attr_sum, int64_t B, int64_t C, int64_t g_h, int64_t g_w,
                                    int64_t p, int64_t k, int64_t d0, int64_t n_d, int64_t seed, int64_t id0,
                                    te_stream_t stream) {
  return subset_inputs<float>(x, substrate, fill, attr, out, member, attr_sum, B, C, g_h, g_w, p, k, d0, n_d, seed, id0,
                              (hipStream_t)stream);
}

extern "C" int te_subset_inputs_bf16(const float* x, const float* substrate, const float* fill, const float* attr,
                                     te_bf16_t* out, uint8_t* member, double* attr_sum, int64_t B, int64_t C, int64_t g_h,
                                     int64_t g_w, int64_t p, int64_t k, int64_t d0, int64_t n_d, int64_t seed, int64_t id0,
                                     te_stream_t stream) {
  return subset_inputs<te_bf16_t>(x, substrate, fill, attr, out, member, attr_sum, B, C, g_h, g_w, p, k, d0, n_d, seed, id0,
                                  (hipStream_t)stream);
}

extern "C" int te_perturbation_dot_f32(const float* x, const float* y, const float* w, double* sums, int64_t B, int64_t D,
                                       int64_t n, int64_t m, te_stream_t stream) {
  return perturbation_dot<float>(x, y, w, sums, B, D, n, m, (hipStream_t)stream);
}

extern "C" int te_perturbation_dot_bf16(const float* x, const te_bf16_t* y, const float* w, double* sums, int64_t B, int64_t D,
                                        int64_t n, int64_t m, te_stream_t stream) {
  return perturbation_dot<te_bf16_t>(x, y, w, sums, B, D, n, m, (hipStream_t)stream);
}
