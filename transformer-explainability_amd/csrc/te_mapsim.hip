// te_mapsim.hip -- the similarity of two relevance maps on the device (gfx950): Pearson, Spearman on the values and on the
// absolute values, and SSIM, per sample, as include/te_relprop.h ("map similarity") defines them.  What the sanity-check
// protocol (sanity.py: cascading randomisation, class sensitivity) asks of every pair of maps.
//
// Two launches, no host involvement:
//   1. rank  : one workgroup of 16 waves per (sample, which of a, b, |a|, |b|): 4B sort jobs.  The n elements
//              (te_key(value) << 32 | index) are sorted by the per-sample LSD radix sort of te_common.h.  Then the runs of equal keys: the sorted positions where a run starts are compacted into the idle
//              buffer, and every element of a run s .. e-1 writes d = s + e - n = 2 rank - (n + 1) as int32 to its ORIGINAL
//              index, in the other half of that buffer.  Integers only.
//   2. reduce: one workgroup per sample: the fp64 means and centred sums of Pearson (two passes over a, b), the int64 sums
//              cov, va, vb of the d of both pairs, and the 7x7 windows of SSIM in fp64, thread t taking the windows t,
//              t + 1024, ...  Every fp64 sum is te_wave_sum and then the wave sums in order: an order fixed by the sample.
#include "te_common.h"

namespace {

constexpr int kThreads = kTeSortThreads;
constexpr int kWaves = kTeSortWaves;
constexpr int kDigits = kTeSortDigits;
constexpr int kWin = 7;                            // scikit-image's default window

// the sort job of (sample, which)
__device__ __forceinline__ size_t job_index(int64_t sample, int which) { return (size_t)sample * 4 + (size_t)which; }

__global__ __launch_bounds__(kThreads) void mapsim_rank_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                               uint32_t n, uint64_t* ws) {
  __shared__ uint32_t cnt[2][kDigits * kWaves];      // [digit][wave]: elements of a digit in a wave's source segment
  __shared__ uint32_t wtot[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int which = blockIdx.x;                      // 0: a, 1: b, 2: |a|, 3: |b|
  const int64_t sample = blockIdx.y;
  const float* x = ((which & 1) ? b : a) + (size_t)sample * n;
  const bool magnitude = which >= 2;
  const uint64_t below = (1ull << lane) - 1;
  const TeSortJob job = te_sort_begin(ws, job_index(sample, which), n, cnt, tid);
  const uint32_t S = job.S;
  __syncthreads();

  // ---- build
  for (uint32_t j = tid; j < n; j += kThreads) {
    float v = x[j];
    if (magnitude) v = fabsf(v);
    te_sort_put<32>(job, cnt, j, ((uint64_t)te_key(v) << 32) | j);
  }
  __syncthreads();

  // ---- sort (ascending, stable: equal keys stay in index order)
  te_block_sort_passes<32>(job, cnt, wtot, tid, lane, wave);

  // ---- runs of equal keys: the job's first buffer holds the sorted elements; the second one is idle: its first n words take
  // the sorted positions where a run starts, its last n words the d of every index
  const uint64_t* src = job.src;
  uint32_t* starts = reinterpret_cast<uint32_t*>(job.dst);
  int32_t* d = reinterpret_cast<int32_t*>(job.dst) + n;
  const uint32_t seg0 = (uint32_t)wave * S, seg1 = min(seg0 + S, n);
  {
    uint32_t ns = 0;
    for (uint32_t base = seg0; base < seg1; base += TE_WAVE) {
      const uint32_t j = base + lane;
      bool start = false;
      if (j < seg1) start = (j == 0) || ((src[j - 1] >> 32) != (src[j] >> 32));
      ns += (uint32_t)__popcll(__ballot(start));
    }
    if (lane == 0) wtot[wave] = ns;
  }
  __syncthreads();
  uint32_t runs_before = 0, nruns = 0;
  for (int w = 0; w < kWaves; ++w) {
    if (w < wave) runs_before += wtot[w];
    nruns += wtot[w];
  }
  {
    uint32_t rb = runs_before;
    for (uint32_t base = seg0; base < seg1; base += TE_WAVE) {
      const uint32_t j = base + lane;
      bool start = false;
      if (j < seg1) start = (j == 0) || ((src[j - 1] >> 32) != (src[j] >> 32));
      const uint64_t sb = __ballot(start);
      if (start) starts[rb + (uint32_t)__popcll(sb & below)] = j;
      rb += (uint32_t)__popcll(sb);
    }
  }
  __syncthreads();
  {
    uint32_t rb = runs_before;
    for (uint32_t base = seg0; base < seg1; base += TE_WAVE) {
      const uint32_t j = base + lane;
      const bool live = j < seg1;
      uint64_t e = 0;
      bool start = false;
      if (live) {
        e = src[j];
        start = (j == 0) || ((src[j - 1] >> 32) != (e >> 32));
      }
      const uint64_t sb = __ballot(start);
      if (live) {
        const uint32_t r = rb + (uint32_t)__popcll(sb & (below | (1ull << lane))) - 1;      // the run of position j
        const uint32_t s = starts[r], end = (r + 1 < nruns) ? starts[r + 1] : n;
        d[(uint32_t)e] = (int32_t)(s + end) - (int32_t)n;
      }
      rb += (uint32_t)__popcll(sb);
    }
  }
}

__device__ __forceinline__ double clamp_unit(double v) { return v > 1.0 ? 1.0 : (v < -1.0 ? -1.0 : v); }      // keeps NaN

__global__ __launch_bounds__(kThreads) void mapsim_reduce_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                 uint32_t n, int H, int W, int flags, double data_range,
                                                                 uint64_t* ws, int64_t* __restrict__ rank_sums,
                                                                 double* __restrict__ sim) {
  __shared__ double red[3 * kWaves];
  __shared__ long long ired[3 * kWaves];
  __shared__ double mean[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t sample = blockIdx.x;
  const float* xa = a + (size_t)sample * n;
  const float* xb = b + (size_t)sample * n;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);

  // ---- the means; a NaN anywhere
  double sa = 0.0, sb = 0.0, unused = 0.0;
  int bad = 0;
  for (uint32_t j = tid; j < n; j += kThreads) {
    const float va = xa[j], vb = xb[j];
    bad |= (va != va) || (vb != vb);
    sa += (double)va;
    sb += (double)vb;
  }
  if (__syncthreads_or(bad)) {                     // the NaN rule: nan_policy="propagate"
    if (tid < 6) rank_sums[sample * 6 + tid] = 0;
    if (tid < 4) sim[sample * 4 + tid] = nan;
    return;
  }
  te_block_sum3(sa, sb, unused, red);
  if (tid == 0) {
    mean[0] = sa / (double)n;
    mean[1] = sb / (double)n;
  }
  __syncthreads();

  // ---- Pearson: the centred sums
  const double ma = mean[0], mb = mean[1];
  double sab = 0.0, saa = 0.0, sbb = 0.0;
  for (uint32_t j = tid; j < n; j += kThreads) {
    const double ca = (double)xa[j] - ma, cb = (double)xb[j] - mb;
    sab += ca * cb;
    saa += ca * ca;
    sbb += cb * cb;
  }
  te_block_sum3(sab, saa, sbb, red);
  double pearson = nan;
  if (tid == 0 && saa != 0.0 && sbb != 0.0) pearson = clamp_unit(sab / (sqrt(saa) * sqrt(sbb)));

  // ---- Spearman on the values (pair 0) and on the absolute values (pair 1): exact integers
  double rho[2] = {nan, nan};
  for (int pair = 0; pair < 2; ++pair) {
    const int32_t* da = reinterpret_cast<const int32_t*>(te_sort_buffers(ws, job_index(sample, 2 * pair), n) + n) + n;
    const int32_t* db = reinterpret_cast<const int32_t*>(te_sort_buffers(ws, job_index(sample, 2 * pair + 1), n) + n) + n;
    long long cov = 0, va = 0, vb = 0;
    for (uint32_t j = tid; j < n; j += kThreads) {
      const long long p = da[j], q = db[j];
      cov += p * q;
      va += p * p;
      vb += q * q;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      cov += __shfl_down(cov, off, TE_WAVE);
      va += __shfl_down(va, off, TE_WAVE);
      vb += __shfl_down(vb, off, TE_WAVE);
    }
    __syncthreads();
    if (lane == 0) {
      ired[wave * 3 + 0] = cov;
      ired[wave * 3 + 1] = va;
      ired[wave * 3 + 2] = vb;
    }
    __syncthreads();
    if (tid == 0) {
      long long c = 0, p = 0, q = 0;
      for (int w = 0; w < kWaves; ++w) {
        c += ired[w * 3 + 0];
        p += ired[w * 3 + 1];
        q += ired[w * 3 + 2];
      }
      int64_t* out = rank_sums + sample * 6 + pair * 3;
      out[0] = c;
      out[1] = p;
      out[2] = q;
      if (p != 0 && q != 0) {
        // the same (or the reversed) ranking is exactly +-1, which sqrt(va) * sqrt(va) == va does not promise
        const bool exact = p == q && (c == p || c == -p);
        rho[pair] = exact ? (c > 0 ? 1.0 : -1.0) : clamp_unit((double)c / (sqrt((double)p) * sqrt((double)q)));
      }
    }
  }

  // ---- SSIM: the mean of S over the (H - 6)(W - 6) windows inside the image
  double ssim = nan;
  if (flags & TE_MAPSIM_SSIM) {
    const int Hm = H - (kWin - 1), Wm = W - (kWin - 1);
    const uint32_t nwin = (uint32_t)Hm * (uint32_t)Wm;
    const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
    const double np = (double)(kWin * kWin), cov_norm = np / (np - 1.0);
    double acc = 0.0;
    for (uint32_t w = tid; w < nwin; w += kThreads) {
      const int r = (int)(w / (uint32_t)Wm), c = (int)(w - (uint32_t)r * (uint32_t)Wm);
      double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
      for (int dy = 0; dy < kWin; ++dy) {
        const float* ra = xa + (size_t)(r + dy) * W + c;
        const float* rb = xb + (size_t)(r + dy) * W + c;
#pragma unroll
        for (int dx = 0; dx < kWin; ++dx) {
          const double x = (double)ra[dx], y = (double)rb[dx];
          sx += x;
          sy += y;
          sxx += x * x;
          syy += y * y;
          sxy += x * y;
        }
      }
      const double ux = sx / np, uy = sy / np, uxx = sxx / np, uyy = syy / np, uxy = sxy / np;
      const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
      acc += ((2.0 * ux * uy + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2));
    }
    te_block_sum(acc, red);                        // (the barriers of the rank sums lie between this use of red and the last)
    if (tid == 0) ssim = acc / (double)nwin;
  }

  if (tid == 0) {
    double* out = sim + sample * 4;
    out[0] = pearson;
    out[1] = rho[0];
    out[2] = rho[1];
    out[3] = ssim;
  }
}

}  // namespace

extern "C" size_t te_map_similarity_workspace_bytes(int64_t B, int64_t n) {
  if (B <= 0 || n <= 0 || B > kTeMaxBatch || n > kTeMaxSortN) return 0;
  return te_sort_workspace_bytes((size_t)B * 4, (size_t)n);      // per sample four sort jobs (a, b, |a|, |b|)
}

extern "C" int te_map_similarity_f32(const float* a, const float* b, int64_t* rank_sums, double* sim, int64_t B, int64_t n,
                                     int64_t H, int64_t W, int flags, double data_range, void* ws, size_t ws_bytes,
                                     te_stream_t stream) {
  if (!a || !b || !rank_sums || !sim || B <= 0 || n <= 0 || (flags & ~TE_MAPSIM_SSIM)) return TE_ERR_INVALID_ARG;
  if ((flags & TE_MAPSIM_SSIM) && (H < kWin || W < kWin || n % W != 0 || n / W != H)) return TE_ERR_INVALID_ARG;      // H * W != n
  if (B > kTeMaxBatch || n > kTeMaxSortN) return TE_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < te_map_similarity_workspace_bytes(B, n)) return TE_ERR_WORKSPACE;
  if (((uintptr_t)ws) & 7u) return TE_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  mapsim_rank_kernel<<<dim3(4, (unsigned)B), dim3(kThreads), 0, st>>>(a, b, (uint32_t)n, (uint64_t*)ws);
  TE_RETURN_IF_LAUNCH_FAILED();
  mapsim_reduce_kernel<<<dim3((unsigned)B), dim3(kThreads), 0, st>>>(a, b, (uint32_t)n, (int)H, (int)W, flags, data_range,
                                                                     (uint64_t*)ws, rank_sums, sim);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}
