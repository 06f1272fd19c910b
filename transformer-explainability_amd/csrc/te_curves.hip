// te_curves.hip -- deletion / insertion curves (RISE's CausalMetric, Petsiuk et al., BMVC 2018) on the device (gfx950), as
// include/te_relprop.h ("deletion / insertion curves") defines them.  The reference tree has no such protocol: the header is
// the specification, curves.py restates it in torch.
//
// Five kernels, no host read-back, no memset node:
//   blur    : one workgroup per (image plane, 32 x 32 tile).  The tile and its halo are normalised on load into LDS (zeros
//             outside the image), the horizontal pass goes to a second LDS tile, the vertical pass from there to the output.
//             Every output runs the same klen + klen FMAs in tap order whatever tile it falls in: its bits do not depend on
//             tiling, batch or grid.  LDS: (32 + 2r)(32 + 2 r4) + (32 + 2r) 32 floats, r4 = r rounded up to 4 -- 13.1 KiB at
//             klen = 11 (occupancy is then bound by the 32 waves of a CU: 8 workgroups of 256), 47 KiB at klen = 63 (3 per CU).
//   rank    : the per-sample LSD radix sort of te_common.h on the COMPLEMENTED key: a stable ascending sort of
//             ~te_key(v) << 32 | index is descending by value with ties in index order; every element then writes its
//             sorted position to its original index.
//   compose : store-bound.  A thread owns 8 consecutive pixels (4 for fp32 output), reads rank, image and substrate once
//             per channel and walks the steps of its group, one 16-byte non-temporal store per step and channel (the
//             structure of perturb_apply_bf16_kernel).  A pixel switches at image rank / step + 1: no selection table.
//   scores  : one wave per (step, sample) row of logits: fp64 max, fp64 sum of exponentials in a fixed order, the target's term.
//   auc     : one thread per sample, the trapezoid in step order.
#include "te_common.h"

namespace {

constexpr int kThreads = kTeSortThreads;           // rank
constexpr int kWaves = kTeSortWaves;
constexpr int kDigits = kTeSortDigits;
constexpr int kMaxC = TE_PERTURB_MAX_CHANNELS;
constexpr int kTile = 32;                          // blur: outputs per tile side

struct Taps {
  float t[TE_BLUR_MAX_TAPS];
};

// ------------------------------------------------------------------------------------------------ blur
// VEC: 16-byte global accesses (W % 4 == 0, aligned bases); otherwise element-wise.  LDS: in[rows][inw], then hz[rows][kTile]
template <bool VEC>
__global__ __launch_bounds__(256) void blur_kernel(const float* __restrict__ data, float* __restrict__ out, int C, int H,
                                                   int W, int tiles_x, int tiles_y, int klen, Taps taps, TeChannels nm) {
  extern __shared__ float lds[];
  const int r = klen / 2, r4 = (r + 3) & ~3;
  const int rows = kTile + 2 * r, inw = kTile + 2 * r4;
  float* in = lds;
  float* hz = lds + rows * inw;
  const int tid = threadIdx.x;
  const int tiles = tiles_x * tiles_y;
  const int64_t plane = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x - plane * tiles);
  const int y0 = (tile / tiles_x) * kTile, x0 = (tile % tiles_x) * kTile;
  const int c = (int)(plane % C);
  const float mean = nm.mean[c], sd = nm.std[c];
  const float* src = data + plane * (int64_t)H * W;
  float* dst = out + plane * (int64_t)H * W;

  // ---- the tile and its halo, normalised; zeros outside the image.  LDS column j is image column x0 - r4 + j
  if constexpr (VEC) {
    const int groups = inw / 4;
    for (int e = tid; e < rows * groups; e += 256) {
      const int ly = e / groups, g = e - ly * groups;
      const int y = y0 - r + ly, x = x0 - r4 + 4 * g;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (y >= 0 && y < H && x >= 0 && x < W) {    // W % 4 == 0 and x % 4 == 0: a group is inside or outside as a whole
        v = *reinterpret_cast<const f32x4*>(src + (int64_t)y * W + x);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (v[j] - mean) / sd;
      }
      *reinterpret_cast<f32x4*>(in + ly * inw + 4 * g) = v;
    }
  } else {
    for (int e = tid; e < rows * inw; e += 256) {
      const int ly = e / inw, lx = e - ly * inw;
      const int y = y0 - r + ly, x = x0 - r4 + lx;
      float v = 0.f;
      if (y >= 0 && y < H && x >= 0 && x < W) v = (src[(int64_t)y * W + x] - mean) / sd;
      in[e] = v;
    }
  }
  __syncthreads();

  // ---- horizontal pass: hz[ly][lx] = sum_j t_j z[y][x + j - r], taps in index order, one FMA per tap
  const int shift = r4 - r;
  for (int e = tid; e < rows * kTile; e += 256) {
    const int ly = e / kTile, lx = e - ly * kTile;
    const float* p = in + ly * inw + lx + shift;
    float acc = 0.f;
    for (int j = 0; j < klen; ++j) acc = __builtin_fmaf(taps.t[j], p[j], acc);
    hz[e] = acc;
  }
  __syncthreads();

  // ---- vertical pass: a thread takes 4 neighbouring columns of one row
  const int ty = tid >> 3, tx = (tid & 7) * 4;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < klen; ++i) {
    const f32x4 h = *reinterpret_cast<const f32x4*>(hz + (ty + i) * kTile + tx);
    const float t = taps.t[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(t, h[j], acc[j]);
  }
  const int y = y0 + ty, x = x0 + tx;
  if (y >= H) return;
  if constexpr (VEC) {
    if (x < W) *reinterpret_cast<f32x4*>(dst + (int64_t)y * W + x) = f32x4{acc[0], acc[1], acc[2], acc[3]};
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x + j < W) dst[(int64_t)y * W + x + j] = acc[j];
  }
}

// ------------------------------------------------------------------------------------------------ rank
__global__ __launch_bounds__(kThreads) void pixel_rank_kernel(const float* __restrict__ vis, int32_t* __restrict__ rank,
                                                              uint32_t n, uint64_t* ws) {
  __shared__ uint32_t cnt[2][kDigits * kWaves];      // [digit][wave]: elements of a digit in a wave's source segment
  __shared__ uint32_t wtot[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t sample = blockIdx.x;
  const float* x = vis + (size_t)sample * n;
  const TeSortJob job = te_sort_begin(ws, (size_t)sample, n, cnt, tid);
  __syncthreads();

  // ---- build: the complemented key, so that ascending is descending by value
  for (uint32_t j = tid; j < n; j += kThreads) te_sort_put<32>(job, cnt, j, ((uint64_t)~te_key(x[j]) << 32) | j);
  __syncthreads();

  // ---- sort (ascending, stable: equal keys stay in index order)
  te_block_sort_passes<32>(job, cnt, wtot, tid, lane, wave);

  // ---- position j of the sorted elements holds the j-th most relevant pixel
  for (uint32_t j = tid; j < n; j += kThreads) rank[(size_t)sample * n + (uint32_t)job.src[j]] = (int32_t)j;
}

// ------------------------------------------------------------------------------------------------ compose
// out[s - s0][b][c][p] = (s >= rank[b][p] / step + 1) ? after : before, with (before, after) = (z, sub) for deletion and
// (sub, z) for insertion; z = (data - mean[c]) / std[c], sub = substrate[b][c][p] or fill[c].  OutT float: VEC 4 or 1; bf16
// (te_bf16_t): VEC 8 or 1, the fp32 value rounded once to nearest even.
template <typename OutT, int VEC>
__global__ __launch_bounds__(256) void curve_inputs_kernel(const float* __restrict__ data, const float* __restrict__ substrate,
                                                           const int32_t* __restrict__ rank, OutT* __restrict__ out, int64_t B,
                                                           int64_t C, int64_t HW, uint32_t step, int s0, int n_s, int spg,
                                                           int insertion, TeChannels nm) {
  const int64_t b = blockIdx.y;
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC;
  if (i0 >= HW) return;
  const int g0 = (int)blockIdx.z * spg, g1 = min(n_s, g0 + spg);      // this group's images, counted from s0
  int sw[VEC];                                     // the first image (counted from s0) in which the pixel is switched
  {
    const int32_t* rp = rank + b * HW + i0;
    if constexpr (VEC == 1) {
      sw[0] = (int)((uint32_t)rp[0] / step) + 1 - s0;
    } else {
#pragma unroll
      for (int q = 0; q < VEC / 4; ++q) {
        const u32x4 rv = *reinterpret_cast<const u32x4*>(rp + 4 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j) sw[4 * q + j] = (int)(rv[j] / step) + 1 - s0;
      }
    }
  }
  for (int64_t c = 0; c < C; ++c) {
    const float* src = data + (b * C + c) * HW + i0;
    const float mean = nm.mean[c], sd = nm.std[c];
    float before[VEC], after[VEC];
    if constexpr (VEC == 1) {
      before[0] = src[0];
      after[0] = substrate ? substrate[(b * C + c) * HW + i0] : nm.fill[c];
    } else {
#pragma unroll
      for (int q = 0; q < VEC / 4; ++q) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(src + 4 * q);
        f32x4 sv = {nm.fill[c], nm.fill[c], nm.fill[c], nm.fill[c]};
        if (substrate) sv = *reinterpret_cast<const f32x4*>(substrate + (b * C + c) * HW + i0 + 4 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          before[4 * q + j] = xv[j];
          after[4 * q + j] = sv[j];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const float z = (before[j] - mean) / sd, sub = after[j];
      before[j] = insertion ? sub : z;
      after[j] = insertion ? z : sub;
    }
    for (int g = g0; g < g1; ++g) {
      OutT* dst = out + (((int64_t)g * B + b) * C + c) * HW + i0;
      float y[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) y[j] = (g >= sw[j]) ? after[j] : before[j];
      if constexpr (std::is_same<OutT, float>::value) {
        if constexpr (VEC == 4)
          __builtin_nontemporal_store(f32x4{y[0], y[1], y[2], y[3]}, reinterpret_cast<f32x4*>(dst));
        else
          dst[0] = y[0];
      } else {
        if constexpr (VEC == 8) {
          u32x4 p;
#pragma unroll
          for (int j = 0; j < 4; ++j) p[j] = te_pack_bf16(y[2 * j], y[2 * j + 1]);
          __builtin_nontemporal_store(p, reinterpret_cast<u32x4*>(dst));
        } else {
          dst[0] = bf16_bits(y[0]);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ scores
// one wave per row of logits [rows, K]: prob[s0 + row / B][row % B] = softmax(row)[target[row % B]] in fp64.  Lane l takes the
// classes l, l + 64, ... in order; the 64 partial sums meet in te_wave_sum: an order fixed by K alone.
template <typename T>
__global__ __launch_bounds__(256) void curve_scores_kernel(const T* __restrict__ logits, const int64_t* __restrict__ target,
                                                           double* __restrict__ prob, int64_t B, int64_t K, int64_t s0,
                                                           int64_t rows) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;                         // wave-uniform
  const T* x = logits + row * K;
  const int64_t b = row % B;
  const int64_t t = target[b];
  double m = -__builtin_huge_val();
  for (int64_t k = lane; k < K; k += TE_WAVE) m = fmax(m, te_load_f64(x, k));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, TE_WAVE));
  double sum = 0.0;
  for (int64_t k = lane; k < K; k += TE_WAVE) sum += exp(te_load_f64(x, k) - m);
  sum = te_wave_sum(sum);
  if (lane == 0) {
    double p = __longlong_as_double(0x7ff8000000000000ll);      // a target outside [0, K): NaN
    if (t >= 0 && t < K) p = exp(te_load_f64(x, t) - m) / sum;
    prob[(s0 + row / B) * B + b] = p;
  }
}

// auc[b] = (sum_i p[i][b] - p[0][b] / 2 - p[S][b] / 2) / S, S = S1 - 1, summed in step order
__global__ __launch_bounds__(256) void curve_auc_kernel(const double* __restrict__ prob, double* __restrict__ auc, int64_t S1,
                                                        int64_t B) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  double sum = 0.0;
  for (int64_t i = 0; i < S1; ++i) sum += prob[i * B + b];
  sum -= prob[b] / 2.0;
  sum -= prob[(S1 - 1) * B + b] / 2.0;
  auc[b] = sum / (double)(S1 - 1);
}

template <typename OutT>
int curve_inputs(const float* data, const float* substrate, const float* fill, const int32_t* rank, OutT* out, int64_t B,
                 int64_t C, int64_t HW, int64_t step, int64_t s0, int64_t n_s, int insertion, const float* mean,
                 const float* std_, hipStream_t stream) {
  if (!data || !rank || !out || (!substrate && !fill) || B <= 0 || C <= 0 || HW <= 0 || step < 1 || s0 < 0 || n_s < 1 ||
      (insertion != 0 && insertion != 1))
    return TE_ERR_INVALID_ARG;
  if (B > kTeMaxBatch || C > kMaxC || HW > kTeMaxSortN) return TE_ERR_UNSUPPORTED;
  const int64_t S = te_ceil_div(HW, step);
  if (s0 > S || n_s > S + 1 - s0) return TE_ERR_INVALID_ARG;      // images s0 .. s0 + n_s - 1 of the S + 1
  const TeChannels nm = te_channels(C, mean, std_, fill);
  constexpr int V = std::is_same<OutT, float>::value ? 4 : 8;
  // 16-B accesses: a row of the output starts on a 16-B boundary when HW % V == 0; anything else, and unaligned bases, take
  // the element-wise form
  const bool vec = (HW % V == 0) && te_aligned16(data) && te_aligned16(rank) && te_aligned16(out) &&
                   (!substrate || te_aligned16(substrate));
  const int64_t bx = te_ceil_div(vec ? HW / V : HW, 256);
  // all images of the call inside one thread once B * bx blocks fill the chip (256 CUs x 4 resident blocks); else one per block
  const int spg = (bx * B >= 1024) ? (int)n_s : 1;
  const dim3 grid((unsigned)bx, (unsigned)B, (unsigned)te_ceil_div(n_s, spg));
  if (grid.z > 65535u) return TE_ERR_UNSUPPORTED;
  const uint32_t st = (uint32_t)(step > kTeMaxSortN ? kTeMaxSortN : step);      // step >= HW: S = 1 whatever the value
  if (vec)
    curve_inputs_kernel<OutT, V><<<grid, dim3(256), 0, stream>>>(data, substrate, rank, out, B, C, HW, st, (int)s0, (int)n_s,
                                                                  spg, insertion, nm);
  else
    curve_inputs_kernel<OutT, 1><<<grid, dim3(256), 0, stream>>>(data, substrate, rank, out, B, C, HW, st, (int)s0, (int)n_s,
                                                                  spg, insertion, nm);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

template <typename T>
int curve_scores(const T* logits, const int64_t* target, double* prob, int64_t B, int64_t K, int64_t s0, int64_t n_s,
                 hipStream_t stream) {
  if (!logits || !target || !prob || B <= 0 || K <= 0 || s0 < 0 || n_s < 1) return TE_ERR_INVALID_ARG;
  if (B > kTeMaxBatch || s0 > kTeMaxSortN || n_s > kTeMaxSortN + 1) return TE_ERR_UNSUPPORTED;      // S <= HW <= 2^20
  const int64_t rows = n_s * B;
  curve_scores_kernel<T><<<dim3((unsigned)te_ceil_div(rows, 4)), dim3(256), 0, stream>>>(logits, target, prob, B, K, s0, rows);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

}  // namespace

extern "C" int te_blur_normalised_f32(const float* data, float* out, int64_t B, int64_t C, int64_t H, int64_t W,
                                      const float* taps, int64_t klen, const float* mean, const float* std_,
                                      te_stream_t stream) {
  if (!data || !out || !taps || B <= 0 || C <= 0 || H <= 0 || W <= 0 || klen < 1 || klen % 2 == 0) return TE_ERR_INVALID_ARG;
  if (klen > TE_BLUR_MAX_TAPS || B > kTeMaxBatch || C > kMaxC || H > kTeMaxSortN || W > kTeMaxSortN || H * W > kTeMaxSortN)
    return TE_ERR_UNSUPPORTED;
  const TeChannels nm = te_channels(C, mean, std_, nullptr);
  Taps tp;
  for (int j = 0; j < TE_BLUR_MAX_TAPS; ++j) tp.t[j] = j < klen ? taps[j] : 0.0f;
  const int tiles_x = (int)te_ceil_div(W, kTile), tiles_y = (int)te_ceil_div(H, kTile);
  const int64_t blocks = B * C * tiles_x * tiles_y;      // <= 65535 * 4 * 2^20 / 32: below 2^31 only for sane shapes
  if (blocks > (int64_t)0x7fffffff) return TE_ERR_UNSUPPORTED;
  const int r = (int)klen / 2, r4 = (r + 3) & ~3;
  const size_t lds = (size_t)(kTile + 2 * r) * (size_t)(kTile + 2 * r4 + kTile) * sizeof(float);      // <= 48128 B at klen = 63
  hipStream_t st = (hipStream_t)stream;
  if (W % 4 == 0 && te_aligned16(data) && te_aligned16(out))
    blur_kernel<true><<<dim3((unsigned)blocks), dim3(256), lds, st>>>(data, out, (int)C, (int)H, (int)W, tiles_x, tiles_y,
                                                                      (int)klen, tp, nm);
  else
    blur_kernel<false><<<dim3((unsigned)blocks), dim3(256), lds, st>>>(data, out, (int)C, (int)H, (int)W, tiles_x, tiles_y,
                                                                       (int)klen, tp, nm);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

extern "C" size_t te_pixel_rank_workspace_bytes(int64_t B, int64_t n) {
  if (B <= 0 || n <= 0 || B > kTeMaxBatch || n > kTeMaxSortN) return 0;
  return te_sort_workspace_bytes((size_t)B, (size_t)n);
}

extern "C" int te_pixel_rank_f32(const float* vis, int32_t* rank, int64_t B, int64_t n, void* ws, size_t ws_bytes,
                                 te_stream_t stream) {
  if (!vis || !rank || B <= 0 || n <= 0) return TE_ERR_INVALID_ARG;
  if (B > kTeMaxBatch || n > kTeMaxSortN) return TE_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < te_pixel_rank_workspace_bytes(B, n)) return TE_ERR_WORKSPACE;
  if (((uintptr_t)ws) & 7u) return TE_ERR_INVALID_ARG;
  pixel_rank_kernel<<<dim3((unsigned)B), dim3(kThreads), 0, (hipStream_t)stream>>>(vis, rank, (uint32_t)n, (uint64_t*)ws);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

extern "C" int te_curve_inputs_f32(const float* data, const float* substrate, const float* fill, const int32_t* rank,
                                   float* out, int64_t B, int64_t C, int64_t HW, int64_t step, int64_t s0, int64_t n_s,
                                   int insertion, const float* mean, const float* std_, te_stream_t stream) {
  return curve_inputs<float>(data, substrate, fill, rank, out, B, C, HW, step, s0, n_s, insertion, mean, std_,
                             (hipStream_t)stream);
}

extern "C" int te_curve_inputs_bf16(const float* data, const float* substrate, const float* fill, const int32_t* rank,
                                    te_bf16_t* out, int64_t B, int64_t C, int64_t HW, int64_t step, int64_t s0, int64_t n_s,
                                    int insertion, const float* mean, const float* std_, te_stream_t stream) {
  return curve_inputs<te_bf16_t>(data, substrate, fill, rank, out, B, C, HW, step, s0, n_s, insertion, mean, std_,
                                 (hipStream_t)stream);
}

extern "C" int te_curve_scores_f32(const float* logits, const int64_t* target, double* prob, int64_t B, int64_t K, int64_t s0,
                                   int64_t n_s, te_stream_t stream) {
  return curve_scores<float>(logits, target, prob, B, K, s0, n_s, (hipStream_t)stream);
}

extern "C" int te_curve_scores_bf16(const te_bf16_t* logits, const int64_t* target, double* prob, int64_t B, int64_t K,
                                    int64_t s0, int64_t n_s, te_stream_t stream) {
  return curve_scores<te_bf16_t>(logits, target, prob, B, K, s0, n_s, (hipStream_t)stream);
}

extern "C" int te_curve_auc_f64(const double* prob, double* auc, int64_t S1, int64_t B, te_stream_t stream) {
  if (!prob || !auc || B <= 0 || S1 < 2) return TE_ERR_INVALID_ARG;
  if (B > kTeMaxBatch || S1 > kTeMaxSortN + 1) return TE_ERR_UNSUPPORTED;
  curve_auc_kernel<<<dim3((unsigned)te_ceil_div(B, 256)), dim3(256), 0, (hipStream_t)stream>>>(prob, auc, S1, B);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}
