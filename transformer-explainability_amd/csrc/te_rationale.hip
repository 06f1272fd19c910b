// te_rationale.hip -- the rationale test of a BERT relevance vector on the device (gfx950), SURVEY.md section 8(f):
// ERASER Movie Reviews, token F1 at top-k (BERT_rationale_benchmark/models/pipeline/bert_pipeline.py:547-582 produces the
// rationales, BERT_rationale_benchmark/metrics.py:168-215, 242-253 scores them) and the erased inputs of ERASER's two
// faithfulness numbers (metrics.py:255-282, 301-313 consume them; the reference tree has no producer).
//
// rationale_metrics_kernel: one workgroup of 16 waves per document, one launch, no host involvement.  Every output of a
// document depends on that document alone, so it is the same bits in any batch:
//   1. pool  : word score = maximum over the word's wordpieces (bert_pipeline.py:109-124), an integer LDS atomicMax on
//              te_key(score): exact, and independent of the order of arrival.  NaN counts as 0; flags select clamp(min=0).
//   2. sort  : bitonic sort, descending, of te_key(score) << 32 | ~word in LDS: the composite keys are distinct, so the
//              result does not depend on the sorting network -- descending score, ties in ascending word index.
//   3. counts: an inclusive prefix of the truth bits along the order (a ballot per wave plus the waves' totals) gives
//              tp at every rank: (tp_k, pred_k) per k, and (tp_i, n_i) at the end of every run of equal scores, compacted
//              into the workspace -- integers only.
//   4. soft  : average precision, AUPRC (trapezoid) and ROC-AUC from the runs, in fp64: thread t adds the runs t and
//              t + 1024, then a fixed tree -- an order that depends on the document alone.
//
// token_erase_kernel: one workgroup per (document, fraction): marks the words of the rationale in LDS, then writes the
// comprehensiveness copy (rationale wordpieces dropped) and the sufficiency copy (only those kept), the kept tokens
// compacted to the left in their original order (ballot prefix per wave + wave offsets + a carry per 1024 tokens).
#include <math.h>

#include "te_common.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / TE_WAVE;
constexpr int kMaxLen = 2048;                      // tokens and words per document

struct Ks {
  int n;
  int k[TE_RATIONALE_MAX_KS];
};
struct Fractions {
  int n;
  double t[TE_TOKEN_ERASE_MAX_FRACTIONS];
};

// inverse of te_key for the keys of real floats
__device__ __forceinline__ float float_of_key(uint32_t key) {
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

// Two flags per thread (element `tid` of two rounds of kThreads elements): the number of set flags among the elements
// 0 .. tid of each round (inc0 / inc1) and in each whole round (tot0 / tot1).  seg: 2 * kWaves words of LDS.
__device__ __forceinline__ void flag_prefix2(bool f0, bool f1, uint32_t* seg, uint32_t& inc0, uint32_t& inc1,
                                             uint32_t& tot0, uint32_t& tot1) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t upto = (lane == 63) ? ~0ull : ((1ull << (lane + 1)) - 1);
  const uint64_t b0 = __ballot(f0), b1 = __ballot(f1);
  if (lane == 0) {
    seg[wave] = (uint32_t)__popcll(b0);
    seg[kWaves + wave] = (uint32_t)__popcll(b1);
  }
  __syncthreads();
  uint32_t before0 = 0, before1 = 0;
  tot0 = tot1 = 0;
  for (int w = 0; w < kWaves; ++w) {
    const uint32_t c0 = seg[w], c1 = seg[kWaves + w];
    if (w < wave) {
      before0 += c0;
      before1 += c1;
    }
    tot0 += c0;
    tot1 += c1;
  }
  inc0 = before0 + (uint32_t)__popcll(b0 & upto);
  inc1 = before1 + (uint32_t)__popcll(b1 & upto);
  __syncthreads();
}

__global__ __launch_bounds__(kThreads) void rationale_metrics_kernel(
    const float* __restrict__ scores, const int32_t* __restrict__ word_ids, const uint8_t* __restrict__ truth,
    float* __restrict__ word_scores, int32_t* __restrict__ n_words, int32_t* __restrict__ order,
    int32_t* __restrict__ counts, double* __restrict__ soft, int N, int Wmax, Ks ks, int clamp, uint64_t* ws) {
  __shared__ uint64_t skey[kMaxLen];               // sort elements
  __shared__ uint32_t wkey[kMaxLen];               // 1-2: te_key of the word maximum (0 = no wordpiece); 3: tp at rank r
  __shared__ uint32_t seg[2 * kWaves];
  __shared__ double red[3 * kWaves];
  __shared__ int nw_s;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const float* sb = scores + b * N;
  const int32_t* wb = word_ids + b * N;
  const uint8_t* tb = truth + b * Wmax;
  uint64_t* runs = ws + b * Wmax;

  for (int w = tid; w < kMaxLen; w += kThreads) wkey[w] = 0;
  if (tid == 0) nw_s = 0;
  __syncthreads();

  // ---- 1. pool
  for (int i = tid; i < N; i += kThreads) {
    const int32_t wid = wb[i];
    if (wid >= 0 && wid < Wmax) {
      float s = sb[i];
      if (s != s) s = 0.0f;
      if (clamp && s < 0.0f) s = 0.0f;
      atomicMax(&wkey[wid], te_key(s));
      atomicMax(&nw_s, wid + 1);
    }
  }
  __syncthreads();
  const int nw = nw_s;
  int P = 2;                                       // sort length: a power of two >= nw
  while (P < nw) P <<= 1;
  for (int w = tid; w < kMaxLen; w += kThreads) {
    uint32_t key = wkey[w];
    if (key == 0) key = te_key(0.0f);              // a word without a wordpiece scores 0 (no real score has key 0)
    if (w < nw)
      skey[w] = ((uint64_t)key << 32) | (uint32_t)~(uint32_t)w;
    else if (w < P)
      skey[w] = 0;                                 // below every real element
    if (w < Wmax) word_scores[b * Wmax + w] = w < nw ? float_of_key(key) : 0.0f;
  }
  if (tid == 0) n_words[b] = nw;
  __syncthreads();

  // ---- 2. sort, descending
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (P >> 1); t += kThreads) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const uint64_t a = skey[i], c = skey[l];
        const bool desc = (i & k) == 0;
        if ((a < c) == desc) {
          skey[i] = c;
          skey[l] = a;
        }
      }
      __syncthreads();
    }
  }

  // ---- 3. rank r of round 0 / 1 = tid / tid + 1024
  const int r0 = tid, r1 = tid + kThreads;
  const uint64_t e0 = r0 < nw ? skey[r0] : 0ull, e1 = r1 < nw ? skey[r1] : 0ull;
  const int w0 = (int)~(uint32_t)e0, w1 = (int)~(uint32_t)e1;
  const bool t0 = r0 < nw && tb[w0] != 0, t1 = r1 < nw && tb[w1] != 0;
  const bool end0 = r0 < nw && (r0 + 1 == nw || (uint32_t)(skey[r0 + 1] >> 32) != (uint32_t)(e0 >> 32));
  const bool end1 = r1 < nw && (r1 + 1 == nw || (uint32_t)(skey[r1 + 1] >> 32) != (uint32_t)(e1 >> 32));
  if (r0 < Wmax) order[b * Wmax + r0] = r0 < nw ? w0 : -1;
  if (r1 < Wmax) order[b * Wmax + r1] = r1 < nw ? w1 : -1;
  uint32_t tp0, tp1, tpa, tpb, ri0, ri1, ra, rb;
  flag_prefix2(t0, t1, seg, tp0, tp1, tpa, tpb);
  tp1 += tpa;
  const uint32_t npos = tpa + tpb;
  flag_prefix2(end0, end1, seg, ri0, ri1, ra, rb);
  ri1 += ra;
  const uint32_t nruns = ra + rb;
  if (r0 < nw) wkey[r0] = tp0;
  if (r1 < nw) wkey[r1] = tp1;
  if (end0) runs[ri0 - 1] = (uint64_t)tp0 | ((uint64_t)(r0 + 1) << 32);
  if (end1) runs[ri1 - 1] = (uint64_t)tp1 | ((uint64_t)(r1 + 1) << 32);
  __syncthreads();
  if (tid < ks.n) {
    const int pk = min(ks.k[tid], nw);
    counts[(b * ks.n + tid) * 2] = pk > 0 ? (int32_t)wkey[pk - 1] : 0;
    counts[(b * ks.n + tid) * 2 + 1] = pk;
  }

  // ---- 4. soft scores; 0 for a document of one class
  double ap = 0.0, pr = 0.0, roc = 0.0;
  if (npos > 0 && npos < (uint32_t)nw) {
    const double dpos = (double)npos, dneg = (double)((uint32_t)nw - npos);
    for (uint32_t k = tid; k < nruns; k += kThreads) {
      const uint64_t rk = runs[k];
      const uint32_t tp = (uint32_t)rk, n = (uint32_t)(rk >> 32);
      uint32_t tpp = 0, np = 0;
      if (k) {
        const uint64_t rp = runs[k - 1];
        tpp = (uint32_t)rp;
        np = (uint32_t)(rp >> 32);
      }
      const double p = (double)tp / (double)n, r = (double)tp / dpos, f = (double)(n - tp) / dneg;
      const double pp = k ? (double)tpp / (double)np : 1.0, rp = (double)tpp / dpos, fp = (double)(np - tpp) / dneg;
      ap += (r - rp) * p;
      pr += (r - rp) * ((p + pp) / 2.0);
      roc += (f - fp) * ((r + rp) / 2.0);
    }
  }
  te_block_sum3(ap, pr, roc, red);
  if (tid == 0) {
    soft[b * 4 + 0] = ap;
    soft[b * 4 + 1] = pr;
    soft[b * 4 + 2] = roc;
    soft[b * 4 + 3] = (double)npos;
  }
}

__global__ __launch_bounds__(kThreads) void token_erase_kernel(
    const int64_t* __restrict__ ids, const int64_t* __restrict__ mask, const int32_t* __restrict__ word_ids,
    const int32_t* __restrict__ order, const int32_t* __restrict__ n_words, int64_t* __restrict__ ids_out,
    int64_t* __restrict__ mask_out, int32_t* __restrict__ n_rationale, int B, int N, int Wmax, Fractions fr,
    int64_t pad_id) {
  __shared__ uint8_t inrat[kMaxLen];               // word w belongs to the rationale
  __shared__ uint32_t seg[2 * kWaves];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x, ti = blockIdx.y;
  const int nw = min(max(n_words[b], 0), Wmax);
  int m = 0;                                       // min(nw, max(1, ceil(t nw))): one IEEE fp64 product, as on the host
  if (nw > 0) {
    const double c = ceil(fr.t[ti] * (double)nw);
    m = c < 1.0 ? 1 : (c > (double)nw ? nw : (int)c);
  }
  for (int w = tid; w < kMaxLen; w += kThreads) inrat[w] = 0;
  __syncthreads();
  for (int r = tid; r < m; r += kThreads) {
    const int32_t w = order[b * Wmax + r];
    if (w >= 0 && w < Wmax) inrat[w] = 1;
  }
  if (tid == 0) n_rationale[ti * B + b] = m;
  __syncthreads();

  const int64_t* ib = ids + b * N;
  const int64_t* mb = mask + b * N;
  const int32_t* wb = word_ids + b * N;
  const int64_t oc = ((0 * (int64_t)fr.n + ti) * B + b) * N, os = ((1 * (int64_t)fr.n + ti) * B + b) * N;
  uint32_t kept_c = 0, kept_s = 0;
  for (int base = 0; base < N; base += kThreads) {
    const int i = base + tid;
    int64_t id = 0;
    bool keep_c = false, keep_s = false;
    if (i < N) {
      id = ib[i];
      const bool on = mb[i] != 0;
      const int32_t wid = wb[i];
      const bool rat = wid >= 0 && wid < Wmax && inrat[wid];
      keep_c = on && !rat;                         // [CLS] / [SEP] / [UNK] (wid < 0, mask 1) stay in both copies
      keep_s = on && (wid < 0 || rat);
    }
    uint32_t ic, is, tc, ts;
    flag_prefix2(keep_c, keep_s, seg, ic, is, tc, ts);
    if (keep_c) {
      ids_out[oc + kept_c + ic - 1] = id;
      mask_out[oc + kept_c + ic - 1] = 1;
    }
    if (keep_s) {
      ids_out[os + kept_s + is - 1] = id;
      mask_out[os + kept_s + is - 1] = 1;
    }
    kept_c += tc;
    kept_s += ts;
  }
  for (int i = tid; i < N; i += kThreads) {
    if ((uint32_t)i >= kept_c) {
      ids_out[oc + i] = pad_id;
      mask_out[oc + i] = 0;
    }
    if ((uint32_t)i >= kept_s) {
      ids_out[os + i] = pad_id;
      mask_out[os + i] = 0;
    }
  }
}

}  // namespace

extern "C" size_t te_rationale_metrics_workspace_bytes(int64_t B, int64_t N, int64_t Wmax) {
  if (B <= 0 || N <= 0 || Wmax <= 0 || B > kTeMaxBatch || N > kMaxLen || Wmax > kMaxLen) return 0;
  // one (tp, n) pair of 8 bytes per run of equal word scores, at most Wmax runs per document
  return te_align_up((size_t)B * (size_t)Wmax * sizeof(uint64_t), 256);
}

extern "C" int te_rationale_metrics_f32(const float* scores, const int32_t* word_ids, const uint8_t* truth,
                                        float* word_scores, int32_t* n_words, int32_t* order, int32_t* counts,
                                        double* soft, int64_t B, int64_t N, int64_t Wmax, const int64_t* ks,
                                        int64_t n_ks, int flags, void* ws, size_t ws_bytes, te_stream_t stream) {
  if (!scores || !word_ids || !truth || !word_scores || !n_words || !order || !counts || !soft || !ks || B <= 0 ||
      N <= 0 || Wmax <= 0 || n_ks <= 0 || n_ks > TE_RATIONALE_MAX_KS || (flags & ~TE_RATIONALE_CLAMP))
    return TE_ERR_INVALID_ARG;
  Ks k;
  k.n = (int)n_ks;
  for (int s = 0; s < TE_RATIONALE_MAX_KS; ++s) k.k[s] = 0;
  for (int s = 0; s < k.n; ++s) {
    if (ks[s] <= 0) return TE_ERR_INVALID_ARG;
    k.k[s] = (int)(ks[s] > kMaxLen ? kMaxLen : ks[s]);       // pred_k = min(k, n_words) and n_words <= 2048
  }
  if (B > kTeMaxBatch || N > kMaxLen || Wmax > kMaxLen) return TE_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < te_rationale_metrics_workspace_bytes(B, N, Wmax)) return TE_ERR_WORKSPACE;
  if (((uintptr_t)ws) & 7u) return TE_ERR_INVALID_ARG;
  rationale_metrics_kernel<<<dim3((unsigned)B), dim3(kThreads), 0, (hipStream_t)stream>>>(
      scores, word_ids, truth, word_scores, n_words, order, counts, soft, (int)N, (int)Wmax, k,
      (flags & TE_RATIONALE_CLAMP) ? 1 : 0, (uint64_t*)ws);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

extern "C" int te_token_erase(const int64_t* input_ids, const int64_t* attention_mask, const int32_t* word_ids,
                              const int32_t* order, const int32_t* n_words, int64_t* ids_out, int64_t* mask_out,
                              int32_t* n_rationale, int64_t B, int64_t N, int64_t Wmax, const double* fractions,
                              int64_t n_t, int64_t pad_id, te_stream_t stream) {
  if (!input_ids || !attention_mask || !word_ids || !order || !n_words || !ids_out || !mask_out || !n_rationale ||
      !fractions || B <= 0 || N <= 0 || Wmax <= 0 || n_t <= 0 || n_t > TE_TOKEN_ERASE_MAX_FRACTIONS)
    return TE_ERR_INVALID_ARG;
  Fractions fr;
  fr.n = (int)n_t;
  for (int s = 0; s < TE_TOKEN_ERASE_MAX_FRACTIONS; ++s) fr.t[s] = 0.0;
  for (int s = 0; s < fr.n; ++s) {
    if (!(fractions[s] > 0.0) || fractions[s] > 1.0) return TE_ERR_INVALID_ARG;      // (NaN included)
    fr.t[s] = fractions[s];
  }
  if (B > kTeMaxBatch || N > kMaxLen || Wmax > kMaxLen) return TE_ERR_UNSUPPORTED;
  token_erase_kernel<<<dim3((unsigned)B, (unsigned)n_t), dim3(kThreads), 0, (hipStream_t)stream>>>(
      input_ids, attention_mask, word_ids, order, n_words, ids_out, mask_out, n_rationale, (int)B, (int)N, (int)Wmax,
      fr, pad_id);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}
