// te_localise.hip -- the localisation test of a relevance map against a ground-truth region on the device (gfx950), as
// include/te_relprop.h ("localisation test") defines it: the pointing game (Zhang et al., IJCV 2018), the energy-based
// pointing game / relevance mass accuracy (Wang et al., CVPRW 2020; Arras et al., Information Fusion 2022) and relevance
// rank accuracy (Arras et al. 2022), per (image, class) pair.  The reference tree has no such protocol: the header is the
// specification, localisation.py restates it in torch.
//
// One workgroup of 16 waves per pair, ONE launch, no host involvement, nothing to zero (every output word of a pair is
// stored once, by the pair's own workgroup -- a skipped pair stores its fixed rows):
//   1. build  : the map and its label map (or boxes) are read ONCE.  Wave w takes the 64 consecutive pixels of a 1024-pixel
//               trip, so one ballot is one word of the pair's target bit mask.  Per pixel: key = te_key(cleaned heat), 0 for a
//               pixel that is not valid (no cleaned value has key 0) -> workspace; the counts, the argmax as the maximum of
//               key << 32 | ~index (largest key, then lowest index), the two fp64 energies, and the histogram of the select's
//               first digit (it does not depend on K = n_target).
//   2. d2_min : with the block's argmax known, the minimum of dy^2 + dx^2 over the set bits of the mask, in int64.
//   3. select : te_perturb.hip's 8-bit radix select for the K-th largest key among the valid pixels (three more histogram
//               passes over the keys in the workspace, which L2 holds), then the hits: every wave owns a contiguous segment of
//               the pixels, counts its keys equal to the threshold, and after one prefix over the 16 waves ranks them by
//               ballots -- a tied pixel is among the top K iff fewer than `need` tied pixels precede it in index order.
//               The walk over a pass's 256 digit counts is one wave's prefix sum; when every tied pixel is taken (always so
//               without ties) the ranking and its read of the keys are skipped.
// The loops are bound by latency, not by bandwidth (a pair is one workgroup): each issues the loads of kBatch trips together,
// ahead of the ballots and LDS atomics that consume them.
// fp64 sums: thread t adds the pixels t, t + 1024, ... in that order, te_wave_sum folds the 64 lanes, thread 0 adds the 16
// waves in order: an order the image size alone fixes.  Everything else is integer.
#include "te_common.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / TE_WAVE;
constexpr int64_t kMaxBoxes = 64;
constexpr int kBatch = 8;                          // trips of a loop whose loads are issued together: the loops are latency-bound

// per pair: H*W 4-byte keys (padded to 8 bytes), then ceil(H*W / 64) 8-byte words of the target mask
__host__ __device__ __forceinline__ size_t pair_ws_words(uint32_t n) {      // in 8-byte words
  return ((size_t)n + 1) / 2 + ((size_t)n + 63) / 64;
}

// hist[digit] += 1 for every live lane.  Neighbouring pixels of a heat map mostly share the leading digits (sign and
// exponent): the lanes that agree with the wave's first live lane are added as ONE atomic, the others one each.  Integer LDS
// atomics: the counts do not depend on the order of arrival.
__device__ __forceinline__ void hist_add(uint32_t* hist, uint32_t digit, bool live, int lane) {
  const uint64_t lv = __ballot(live);
  if (lv == 0) return;                                                      // wave-uniform
  const int first = __ffsll((long long)lv) - 1;
  const uint32_t d0 = (uint32_t)__shfl((int)digit, first, TE_WAVE);
  const uint64_t same = __ballot(live && digit == d0);
  if (lane == first) atomicAdd(&hist[d0], (uint32_t)__popcll(same));
  if (live && digit != d0) atomicAdd(&hist[digit], 1u);
}

__global__ __launch_bounds__(kThreads) void localisation_kernel(const float* __restrict__ heat,
                                                                const int64_t* __restrict__ labels,
                                                                const int64_t* __restrict__ image_index,
                                                                const int64_t* __restrict__ target_id,
                                                                const int64_t* __restrict__ boxes, int M,
                                                                int64_t* __restrict__ stats, double* __restrict__ energy,
                                                                int64_t B, int H, int W, uint64_t* ws) {
  __shared__ uint32_t hist[256];
  __shared__ int64_t box[kMaxBoxes * 4];
  __shared__ unsigned long long red_best[kWaves];
  __shared__ long long red_d2[kWaves];
  __shared__ double red_e[2 * kWaves];
  __shared__ uint32_t red_cnt[2];                  // n_valid, n_target
  __shared__ uint32_t wave_ties[kWaves];
  __shared__ uint32_t hits;
  __shared__ uint32_t sel_prefix, sel_need, sel_ties;      // the select's state, written by thread 0
  __shared__ unsigned long long best_all;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t p = blockIdx.x;
  const uint32_t n = (uint32_t)H * (uint32_t)W;
  int64_t* st = stats + p * 5;
  double* en = energy + p * 2;

  // ---- a skipped pair: its image index is never used as an address.  (Boxes without an image index: nothing to skip.)
  const int64_t img = image_index ? image_index[p] : labels ? p : 0;
  const int64_t tgt_id = labels ? target_id[p] : 0;
  if (img < 0 || img >= B || tgt_id < 0) {         // block-uniform
    if (tid == 0) {
      st[0] = 0;
      st[1] = 0;
      st[2] = -1;
      st[3] = -1;
      st[4] = 0;
      en[0] = 0.0;
      en[1] = 0.0;
    }
    return;
  }

  const float* hp = heat + (size_t)p * n;
  const int64_t* lb = labels ? labels + (size_t)img * n : nullptr;
  uint32_t* keys = reinterpret_cast<uint32_t*>(ws + (size_t)p * pair_ws_words(n));
  uint64_t* maskw = ws + (size_t)p * pair_ws_words(n) + ((size_t)n + 1) / 2;

  if (tid < 256) hist[tid] = 0;
  if (tid < 2) red_cnt[tid] = 0;
  if (tid == 0) hits = 0;
  if (!labels)
    for (int i = tid; i < M * 4; i += kThreads) box[i] = boxes[p * M * 4 + i];
  __syncthreads();

  // ---- 1. build
  uint32_t nv = 0, nt = 0;
  unsigned long long best = 0;                     // 0: no valid pixel (a valid pixel's key is > 0)
  double e_t = 0.0, e_v = 0.0;
  for (uint32_t base = 0; base < n; base += kBatch * kThreads) {
    float hv[kBatch];
    int64_t lv[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {             // the loads of kBatch trips in flight together
      const uint32_t i = base + (uint32_t)u * kThreads + (uint32_t)tid;
      hv[u] = i < n ? hp[i] : 0.0f;
      lv[u] = (lb && i < n) ? lb[i] : -1;
    }
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const uint32_t i = base + (uint32_t)u * kThreads + (uint32_t)tid;
      if (i - (uint32_t)lane >= n) continue;                                 // wave-uniform: the wave's 64 pixels are past the end
      const bool live = i < n;
      float h = hv[u];
      bool valid = false, tgt = false;
      if (live) {
        if (lb) {
          valid = lv[u] >= 0;
          tgt = lv[u] == tgt_id;                   // tgt_id >= 0: a target is valid
        } else {
          valid = true;
          const int64_t y = i / (uint32_t)W, x = i - (uint32_t)y * (uint32_t)W;
          for (int m = 0; m < M; ++m)
            tgt = tgt || (box[4 * m] <= x && x < box[4 * m + 2] && box[4 * m + 1] <= y && y < box[4 * m + 3]);
        }
      }
      if (h != h) h = 0.0f;                        // the clean-up of te_seg_metrics_f32
      const uint32_t key = valid ? te_key(h) : 0u;
      if (live) keys[i] = key;
      const uint64_t tb = __ballot(tgt);
      if (lane == 0) maskw[i >> 6] = tb;
      nv += valid ? 1u : 0u;
      nt += tgt ? 1u : 0u;
      if (valid) {
        const unsigned long long cand = ((unsigned long long)key << 32) | (0xffffffffu - i);
        best = cand > best ? cand : best;
        const double e = h > 0.0f ? (double)h : 0.0;
        e_v += e;
        if (tgt) e_t += e;
      }
      hist_add(hist, key >> 24, valid, lane);
    }
  }
  nv = te_wave_sum_u32(nv);
  nt = te_wave_sum_u32(nt);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_down(best, off, TE_WAVE);
    best = o > best ? o : best;
  }
  e_t = te_wave_sum(e_t);
  e_v = te_wave_sum(e_v);
  if (lane == 0) {
    atomicAdd(&red_cnt[0], nv);
    atomicAdd(&red_cnt[1], nt);
    red_best[wave] = best;
    red_e[2 * wave] = e_t;
    red_e[2 * wave + 1] = e_v;
  }
  __syncthreads();                                 // also: the keys and the mask words of this pair are written
  if (tid == 0) {
    unsigned long long b = 0;
    double st_ = 0.0, sv = 0.0;
    for (int w = 0; w < kWaves; ++w) {
      b = red_best[w] > b ? red_best[w] : b;
      st_ += red_e[2 * w];
      sv += red_e[2 * w + 1];
    }
    best_all = b;
    en[0] = st_;
    en[1] = sv;
  }
  __syncthreads();
  const uint32_t n_valid = red_cnt[0], K = red_cnt[1];
  const bool have_max = n_valid > 0;
  const uint32_t amax = 0xffffffffu - (uint32_t)best_all;

  // ---- 2. d2_min over the target pixels
  long long d2 = -1;
  if (have_max && K > 0) {                         // block-uniform
    const long long ay = amax / (uint32_t)W, ax = amax - (uint32_t)ay * (uint32_t)W;
    d2 = 0x7fffffffffffffffll;
    for (uint32_t base = 0; base < n; base += kBatch * kThreads) {
      uint64_t mw[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const uint32_t i = base + (uint32_t)u * kThreads + (uint32_t)tid;
        mw[u] = i < n ? maskw[i >> 6] : 0ull;
      }
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const uint32_t i = base + (uint32_t)u * kThreads + (uint32_t)tid;
        if ((mw[u] >> lane) & 1ull) {
          const long long y = i / (uint32_t)W, x = i - (uint32_t)y * (uint32_t)W;
          const long long d = (y - ay) * (y - ay) + (x - ax) * (x - ax);
          d2 = d < d2 ? d : d2;
        }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const long long o = __shfl_down(d2, off, TE_WAVE);
      d2 = o < d2 ? o : d2;
    }
    if (lane == 0) red_d2[wave] = d2;
  }

  // ---- 3. the K-th largest key among the valid pixels: first digit from the histogram of the build
  if (tid == 0) {
    sel_prefix = 0;
    sel_need = K;
  }
  for (int pass = 0; pass < 4 && K > 0; ++pass) {
    const int shift = 24 - 8 * pass;
    if (pass > 0) {
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      const uint32_t want = sel_prefix >> (shift + 8);
      for (uint32_t base = 0; base < n; base += kBatch * kThreads) {
        uint32_t kv[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
          const uint32_t i = base + (uint32_t)u * kThreads + (uint32_t)tid;
          kv[u] = i < n ? keys[i] : 0u;            // key 0: not valid, or past the end
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u)
          hist_add(hist, (kv[u] >> shift) & 0xffu, kv[u] != 0u && (kv[u] >> (shift + 8)) == want, lane);
      }
    }
    __syncthreads();
    if (wave == 0) {
      // the digit of the r-th largest key under the prefix, 1 <= r <= their number: lane l takes the digits 255 - 4 l ..
      // 252 - 4 l, a prefix sum over the lanes says which lane's four hold the r-th, and that lane walks them
      const uint32_t r = sel_need;
      uint32_t c[4], mine4 = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        c[k] = hist[255 - 4 * lane - k];
        mine4 += c[k];
      }
      uint32_t incl = mine4;
#pragma unroll
      for (int off = 1; off < TE_WAVE; off <<= 1) {
        const uint32_t o = __shfl_up(incl, off, TE_WAVE);
        if (lane >= off) incl += o;
      }
      uint32_t left = r - (incl - mine4);          // the rank inside this lane's digits, if the r-th key is here
      if (incl - mine4 < r && r <= incl) {         // one lane
        int k = 0;
        for (; k < 3; ++k) {
          if (left <= c[k]) break;
          left -= c[k];
        }
        sel_prefix |= (uint32_t)(255 - 4 * lane - k) << shift;
        sel_need = left;
        sel_ties = c[k];
      }
    }
    __syncthreads();
  }

  // ---- hits: targets above the threshold, and targets among the first `need` pixels equal to it in index order
  if (K > 0) {
    const uint32_t thr = sel_prefix, need = sel_need;
    const uint32_t S = (n + kThreads - 1) / kThreads * TE_WAVE;      // pixels per wave segment, a multiple of 64
    const uint32_t seg0 = min((uint32_t)wave * S, n), seg1 = min(seg0 + S, n);
    const uint64_t below = (1ull << lane) - 1;
    // every pixel equal to the threshold is among the top K (always so without ties): no ranking, no second read of the keys
    const bool all_ties = need >= sel_ties;        // block-uniform
    uint32_t before = 0;
    if (!all_ties) {
      uint32_t ties = 0;
      for (uint32_t base = seg0; base < seg1; base += kBatch * TE_WAVE) {
        uint32_t kv[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
          const uint32_t i = base + (uint32_t)u * TE_WAVE + lane;
          kv[u] = i < seg1 ? keys[i] : 0u;         // key 0 is no valid pixel's: never equal to the threshold
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) ties += kv[u] == thr ? 1u : 0u;
      }
      ties = te_wave_sum_u32(ties);
      if (lane == 0) wave_ties[wave] = ties;
      __syncthreads();
      for (int w = 0; w < wave; ++w) before += wave_ties[w];
    }
    uint32_t mine = 0;
    for (uint32_t base = seg0; base < seg1; base += kBatch * TE_WAVE) {
      uint32_t kv[kBatch];
      uint64_t mw[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const uint32_t c = base + (uint32_t)u * TE_WAVE;                     // a multiple of 64: bit `lane` of word c / 64
        kv[u] = c + lane < seg1 ? keys[c + lane] : 0u;
        mw[u] = c < seg1 ? maskw[c >> 6] : 0ull;
      }
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const bool tie = kv[u] == thr;
        const uint64_t tb = __ballot(tie);
        const bool taken = kv[u] > thr || (tie && (all_ties || before + (uint32_t)__popcll(tb & below) < need));
        mine += (taken && ((mw[u] >> lane) & 1ull)) ? 1u : 0u;
        before += (uint32_t)__popcll(tb);
      }
    }
    mine = te_wave_sum_u32(mine);
    if (lane == 0) atomicAdd(&hits, mine);
  }
  __syncthreads();
  if (tid == 0) {
    long long d = -1;
    if (have_max && K > 0) {
      d = red_d2[0];
      for (int w = 1; w < kWaves; ++w) d = red_d2[w] < d ? red_d2[w] : d;
    }
    st[0] = (int64_t)n_valid;
    st[1] = (int64_t)K;
    st[2] = have_max ? (int64_t)amax : -1;
    st[3] = (int64_t)d;
    st[4] = (int64_t)hits;
  }
}

}  // namespace

extern "C" size_t te_localisation_workspace_bytes(int64_t P, int64_t H, int64_t W) {
  if (P <= 0 || H <= 0 || W <= 0 || P > kTeMaxBatch || H > kTeMaxSortN || W > kTeMaxSortN || H * W > kTeMaxSortN) return 0;
  return te_align_up((size_t)P * pair_ws_words((uint32_t)(H * W)) * sizeof(uint64_t), 256);
}

extern "C" int te_localisation_f32(const float* heat, const int64_t* labels, const int64_t* image_index,
                                   const int64_t* target_id, const int64_t* boxes, int64_t M, int64_t* stats, double* energy,
                                   int64_t P, int64_t B, int64_t H, int64_t W, void* ws, size_t ws_bytes, te_stream_t stream) {
  if (!heat || !stats || !energy || P <= 0 || B <= 0 || H <= 0 || W <= 0) return TE_ERR_INVALID_ARG;
  if ((labels != nullptr) == (boxes != nullptr)) return TE_ERR_INVALID_ARG;      // exactly one of the two
  if (labels && !target_id) return TE_ERR_INVALID_ARG;
  if (boxes && M <= 0) return TE_ERR_INVALID_ARG;
  if (((uintptr_t)ws) & 7u) return TE_ERR_INVALID_ARG;                           // (a null workspace: TE_ERR_WORKSPACE below)
  if (H > kTeMaxSortN || W > kTeMaxSortN || H * W > kTeMaxSortN || P > kTeMaxBatch || (boxes && M > kMaxBoxes))
    return TE_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < te_localisation_workspace_bytes(P, H, W)) return TE_ERR_WORKSPACE;
  localisation_kernel<<<dim3((unsigned)P), dim3(kThreads), 0, (hipStream_t)stream>>>(
      heat, labels, image_index, target_id, boxes, boxes ? (int)M : 0, stats, energy, B, (int)H, (int)W, (uint64_t*)ws);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}
