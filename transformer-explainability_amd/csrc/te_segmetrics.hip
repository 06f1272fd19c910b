// te_segmetrics.hip -- the segmentation test of a relevance map on the device (gfx950), SURVEY.md section 8(f) row 2:
// pixel accuracy, intersection / union, average precision and the per-row F1 of baselines/ViT/imagenet_seg_eval.py:219-232,
// 263-273 with utils/metrices.py:26-38, 81-99, 135-178, per image, from the heat map, the foreground mask and the labels.
//
// One workgroup of 16 waves per image (a batch is B independent images, so every output of an image is the same bits in
// any batch), one launch, no host involvement:
//   1. build : a wave per image row reads heat / mask / labels once: the six counts, the row's F1, and the 2*H*W sort
//              elements (te_key(score) << 1 | truth) -- class 0 scores the fp32 value 1 - h, class 1 scores h.  A pixel with
//              label < 0 gets key 0, which no cleaned score has: it sorts behind every real score and is never scanned.
//   2. sort  : the per-sample LSD radix sort of te_common.h on the 32 key bits above the truth bit; stable, so equal scores
//              stay in pixel order, class 0 before class 1.
//   3. scan  : over the sorted scores in descending order, the runs of equal keys: (tp_i, n_i) at the end of every run,
//              compacted into the idle half of the workspace -- integers only.
//   4. sum   : AP = sum_i (R_i - R_{i-1}) P_i in fp64, P_i = tp_i / n_i, R_i = tp_i / npos: thread t adds the runs t, t + 1024,
//              ... in that order, then a fixed tree -- an order that depends on the image alone.
#include "te_common.h"

namespace {

constexpr int kThreads = kTeSortThreads;
constexpr int kWaves = kTeSortWaves;
constexpr int kDigits = kTeSortDigits;

__global__ __launch_bounds__(kThreads) void seg_metrics_kernel(const float* __restrict__ heat,
                                                               const float* __restrict__ mask,
                                                               const int64_t* __restrict__ labels,
                                                               int64_t* __restrict__ counts, double* __restrict__ ap,
                                                               double* __restrict__ f1, int H, int W, uint64_t* ws) {
  __shared__ uint32_t cnt[2][kDigits * kWaves];      // [digit][wave]: elements of a digit in a wave's source segment
  __shared__ uint32_t wtot[kWaves], wend[kWaves];
  __shared__ uint32_t tally[8];
  __shared__ double red[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  const uint32_t N = (uint32_t)H * (uint32_t)W, T2 = 2 * N;
  const uint64_t below = (1ull << lane) - 1;
  const float* hb = heat + b * N;
  const float* mb = mask + b * N;
  const int64_t* lb = labels + b * N;

  const TeSortJob job = te_sort_begin(ws, (size_t)b, T2, cnt, tid);
  const uint32_t S = job.S;
  if (tid < 8) tally[tid] = 0;
  __syncthreads();

  // ---- 1. build
  uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // correct, labeled, inter 0/1, predicted 0/1, labelled 0/1
  for (int r = wave; r < H; r += kWaves) {
    uint32_t tp = 0, fp = 0, fn = 0;
    for (int c0 = 0; c0 < W; c0 += TE_WAVE) {
      const int c = c0 + lane;
      const bool live = c < W;
      const uint32_t p = (uint32_t)r * (uint32_t)W + (uint32_t)c;
      float h = 0.0f, mf = 0.0f;
      int64_t lab = -1;
      if (live) {
        h = hb[p];
        mf = mb[p];
        lab = lb[p];
      }
      if (h != h) {                                // foreground_split's clean-up: NaN heat -> 0, its mask -> 0
        h = 0.0f;
        mf = 0.0f;
      }
      const int64_t mi = (int64_t)mf;
      const bool valid = live && lab >= 0;
      const int64_t pred = valid ? mi + 1 : 0, tgt = lab + 1;
      const int64_t inter = (pred == tgt) ? pred : 0;
      acc[0] += (valid && mi == lab) ? 1u : 0u;
      acc[1] += valid ? 1u : 0u;
      acc[2] += (inter == 1) ? 1u : 0u;
      acc[3] += (inter == 2) ? 1u : 0u;
      acc[4] += (pred == 1) ? 1u : 0u;
      acc[5] += (pred == 2) ? 1u : 0u;
      acc[6] += (tgt == 1) ? 1u : 0u;
      acc[7] += (tgt == 2) ? 1u : 0u;
      const bool P = live && mi == 1, T = live && lab == 1;
      tp += (uint32_t)__popcll(__ballot(P && T));
      fp += (uint32_t)__popcll(__ballot(P && !T));
      fn += (uint32_t)__popcll(__ballot(live && !P && T));
      if (live) {
        const uint64_t e0 = valid ? (((uint64_t)te_key(1.0f - h) << 1) | (lab == 0 ? 1u : 0u)) : 0ull;
        const uint64_t e1 = valid ? (((uint64_t)te_key(h) << 1) | (lab == 1 ? 1u : 0u)) : 0ull;
        te_sort_put<1>(job, cnt, p, e0);
        te_sort_put<1>(job, cnt, N + p, e1);
      }
    }
    if (lane == 0) {
      const uint32_t den = 2 * tp + fp + fn;
      f1[b * H + r] = den > 0 ? (double)(2 * tp) / (double)den : 0.0;
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t v = te_wave_sum_u32(acc[k]);
    if (lane == 0) atomicAdd(&tally[k], v);
  }
  __syncthreads();
  if (tid < 6) {
    const uint32_t v = tid < 4 ? tally[tid] : tally[tid] + tally[tid + 2] - tally[tid - 2];   // union = pred + lab - inter
    counts[b * 6 + tid] = (int64_t)v;
  }
  const uint32_t M = 2 * tally[1];                 // scores that take part in AP

  // ---- 2. sort (ascending; the ignored pixels' key 0 comes first)
  te_block_sort_passes<1>(job, cnt, wtot, tid, lane, wave);
  const uint64_t* src = job.src;
  uint64_t* dst = job.dst;

  // ---- 3. runs of equal scores, descending: element j is src[T2 - 1 - j], j < M
  const uint32_t seg0 = (uint32_t)wave * S, seg1 = min(seg0 + S, M);
  {
    uint32_t nt = 0, ne = 0;
    for (uint32_t base = seg0; base < seg1; base += TE_WAVE) {
      const uint32_t j = base + lane;
      const bool live = j < seg1;
      bool t = false, end = false;
      if (live) {
        const uint64_t e = src[T2 - 1 - j];
        t = e & 1u;
        end = (j + 1 == M) || ((src[T2 - 2 - j] >> 1) != (e >> 1));
      }
      nt += (uint32_t)__popcll(__ballot(t));
      ne += (uint32_t)__popcll(__ballot(end));
    }
    if (lane == 0) {
      wtot[wave] = nt;
      wend[wave] = ne;
    }
  }
  __syncthreads();
  uint32_t tp_before = 0, runs_before = 0, npos = 0, nruns = 0;
  for (int w = 0; w < kWaves; ++w) {
    if (w < wave) {
      tp_before += wtot[w];
      runs_before += wend[w];
    }
    npos += wtot[w];
    nruns += wend[w];
  }
  for (uint32_t base = seg0; base < seg1; base += TE_WAVE) {
    const uint32_t j = base + lane;
    const bool live = j < seg1;
    bool t = false, end = false;
    if (live) {
      const uint64_t e = src[T2 - 1 - j];
      t = e & 1u;
      end = (j + 1 == M) || ((src[T2 - 2 - j] >> 1) != (e >> 1));
    }
    const uint64_t tb = __ballot(t), eb = __ballot(end);
    if (end) {
      const uint32_t tp = tp_before + (uint32_t)__popcll(tb & (below | (1ull << lane)));
      dst[runs_before + (uint32_t)__popcll(eb & below)] = (uint64_t)tp | ((uint64_t)(j + 1) << 32);
    }
    tp_before += (uint32_t)__popcll(tb);
    runs_before += (uint32_t)__popcll(eb);
  }
  __syncthreads();

  // ---- 4. AP (utils/metrices.py:81-99 = sklearn.average_precision_score): 0 when nothing is labelled or nothing is positive
  double sum = 0.0;
  if (npos > 0) {
    const double dpos = (double)npos;
    for (uint32_t k = tid; k < nruns; k += kThreads) {
      const uint64_t rk = dst[k];
      const uint32_t tp = (uint32_t)rk, n = (uint32_t)(rk >> 32);
      const uint32_t tp_prev = k ? (uint32_t)dst[k - 1] : 0u;
      const double precision = (double)tp / (double)n, recall = (double)tp / dpos, prev = (double)tp_prev / dpos;
      sum += (recall - prev) * precision;
    }
  }
  te_block_sum(sum, red);
  if (tid == 0) ap[b] = sum;
}

}  // namespace

extern "C" size_t te_seg_metrics_workspace_bytes(int64_t B, int64_t H, int64_t W) {
  if (B <= 0 || H <= 0 || W <= 0 || B > kTeMaxBatch || H > kTeMaxSortN || W > kTeMaxSortN || H * W > kTeMaxSortN) return 0;
  return te_sort_workspace_bytes((size_t)B, 2 * (size_t)(H * W));      // per image one sort of 2*H*W elements
}

extern "C" int te_seg_metrics_f32(const float* heat, const float* fg_mask, const int64_t* labels, int64_t* counts,
                                  double* ap, double* f1, int64_t B, int64_t H, int64_t W, void* ws, size_t ws_bytes,
                                  te_stream_t stream) {
  if (!heat || !fg_mask || !labels || !counts || !ap || !f1 || B <= 0 || H <= 0 || W <= 0) return TE_ERR_INVALID_ARG;
  if (B > kTeMaxBatch || H > kTeMaxSortN || W > kTeMaxSortN || H * W > kTeMaxSortN) return TE_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < te_seg_metrics_workspace_bytes(B, H, W)) return TE_ERR_WORKSPACE;
  if (((uintptr_t)ws) & 7u) return TE_ERR_INVALID_ARG;
  seg_metrics_kernel<<<dim3((unsigned)B), dim3(kThreads), 0, (hipStream_t)stream>>>(heat, fg_mask, labels, counts, ap, f1,
                                                                                   (int)H, (int)W, (uint64_t*)ws);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}
