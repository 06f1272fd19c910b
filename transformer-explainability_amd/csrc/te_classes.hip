// te_classes.hip -- the classes a batch is explained for, chosen and seeded on the device (gfx950).
//
//   te_class_targets_*: per sample, K classes -- the K largest logits of the row (radix select on order-preserving keys, as
//                       te_perturb.hip selects pixels) or K given ones -- with their logits and the K one-hot relevance rows
//                       that seed the relprop chains.  One kernel, one workgroup per sample, nothing read back by the host.
#include "te_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / TE_WAVE;
constexpr int kMaxTopK = TE_CLASS_TARGETS_MAX_TOPK;

typedef double f64x2 __attribute__((ext_vector_type(2)));

// the 64-bit twin of te_key: a > b (as doubles, -0 == +0, NaN largest) <=> key(a) > key(b)
__device__ __forceinline__ uint64_t key_f64(double v) {
  uint64_t u = (uint64_t)__double_as_longlong(v);
  if (u == 0x8000000000000000ull) u = 0;              // -0 -> +0
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// A logit type: its radix key, and the relevance type its scores and seeds are written in (an exact upcast)
template <typename T>
struct Logit;
template <>
struct Logit<float> {
  typedef uint32_t Key;
  typedef float Rel;
  typedef f32x4 Vec;
  static __device__ __forceinline__ Key key(float v) { return te_key(v); }
  static __device__ __forceinline__ Rel up(float v) { return v; }
};
template <>
struct Logit<te_bf16_t> {
  typedef uint32_t Key;
  typedef float Rel;
  typedef f32x4 Vec;
  static __device__ __forceinline__ Rel up(te_bf16_t v) { return te_bf16_up(v); }
  static __device__ __forceinline__ Key key(te_bf16_t v) { return te_key(up(v)); }
};
template <>
struct Logit<double> {
  typedef uint64_t Key;
  typedef double Rel;
  typedef f64x2 Vec;
  static __device__ __forceinline__ Key key(double v) { return key_f64(v); }
  static __device__ __forceinline__ Rel up(double v) { return v; }
};

// Row [0, C) of a seed: 1 at `hot` (none if hot < 0), 0 elsewhere.  Single elements up to the row's first 16-byte boundary
// (an odd C moves it from row to row) and behind the last whole vector, 16-byte stores between; every element is written once,
// by one thread, with its final value.
template <typename Rel, typename Vec>
__device__ __forceinline__ void write_one_hot_row(Rel* __restrict__ o, int C, int hot) {
  constexpr int W = (int)(sizeof(Vec) / sizeof(Rel));
  const int tid = threadIdx.x;
  int head = (int)((W - (int)((reinterpret_cast<uintptr_t>(o) / sizeof(Rel)) & (W - 1))) & (W - 1));
  if (head > C) head = C;
  if (tid < head) o[tid] = (tid == hot) ? (Rel)1 : (Rel)0;
  const int nvec = (C - head) / W;
  Vec* body = reinterpret_cast<Vec*>(o + head);
  for (int v = tid; v < nvec; v += kThreads) {
    const int c = head + v * W;
    Vec x;
#pragma unroll
    for (int e = 0; e < W; ++e) x[e] = (c + e == hot) ? (Rel)1 : (Rel)0;
    body[v] = x;
  }
  const int t0 = head + nvec * W;
  if (tid < C - t0) o[t0 + tid] = (t0 + tid == hot) ? (Rel)1 : (Rel)0;
}

// One workgroup = one sample.  classes_in == nullptr: the K largest keys of the row, descending, equal keys in ascending class
// index -- an 8-bit radix select finds the K-th largest key and how many of its equals are wanted, the keys above it are
// gathered in any order, its first equals in index order (a ballot scan over the row), and the K candidates are ranked by
// (key descending, index ascending) in LDS.  Otherwise the given classes, -1 for one outside [0, C).
template <typename T>
__global__ __launch_bounds__(kThreads) void class_targets_kernel(const T* __restrict__ logits, int64_t ld, int64_t B, int C,
                                                                 int K, const int64_t* __restrict__ classes_in,
                                                                 int64_t* __restrict__ classes_out,
                                                                 typename Logit<T>::Rel* __restrict__ scores,
                                                                 typename Logit<T>::Rel* __restrict__ seeds) {
  typedef Logit<T> L;
  typedef typename L::Key Key;
  typedef typename L::Rel Rel;
  constexpr int kBits = (int)(8 * sizeof(Key));
  __shared__ uint32_t hist[256];
  __shared__ Key s_prefix;                 // key bits fixed so far (high bits)
  __shared__ uint32_t s_need;              // remaining rank (1-based, from the top) inside the prefix group
  __shared__ uint32_t s_greater, s_carry, wave_cnt[kWaves];
  __shared__ Key cand_key[kMaxTopK];
  __shared__ int cand_idx[kMaxTopK];
  __shared__ int sel[kMaxTopK];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const T* row = logits + b * ld;
  const bool topk = classes_in == nullptr;

  if (topk) {                              // (block-uniform; the host has checked 1 <= K <= min(C, kMaxTopK))
    if (tid == 0) {
      s_prefix = 0;
      s_need = (uint32_t)K;
      s_greater = 0;
      s_carry = 0;
    }
    for (int pass = 0; pass < kBits / 8; ++pass) {
      const int shift = kBits - 8 - 8 * pass;
      hist[tid] = 0;                       // (kThreads == 256 bins)
      __syncthreads();
      const Key prefix = s_prefix;
      for (int i = tid; i < C; i += kThreads) {
        const Key key = L::key(row[i]);
        // (pass 0: every element is a candidate; later: only those that match the digits fixed so far)
        if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(unsigned)(key >> shift) & 0xffu], 1u);
      }
      __syncthreads();
      if (tid == 0) {
        uint32_t r = s_need;
        int d = 255;
        for (; d > 0; --d) {
          const uint32_t c = hist[d];
          if (r <= c) break;
          r -= c;
        }
        s_prefix = prefix | ((Key)d << shift);
        s_need = r;
      }
      __syncthreads();
    }
    const Key thr = s_prefix;
    const uint32_t need = s_need;                        // 1 <= need <= number of keys equal to thr
    const uint32_t greater = (uint32_t)K - need;         // = number of keys above thr
    for (int i = tid; i < C; i += kThreads) {
      const Key key = L::key(row[i]);
      if (key > thr) {
        const uint32_t slot = atomicAdd(&s_greater, 1u);
        if (slot < greater) {
          cand_key[slot] = key;
          cand_idx[slot] = i;
        }
      }
    }
    const int lane = tid & 63, wave = tid >> 6;
    for (int base = 0; base < C; base += kThreads) {
      const int i = base + tid;
      const bool tie = (i < C) && L::key(row[i]) == thr;
      const uint64_t bal = __ballot(tie);
      if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(bal);
      __syncthreads();
      uint32_t before = s_carry;
      for (int w = 0; w < wave; ++w) before += wave_cnt[w];
      const uint32_t excl = before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
      if (tie && excl < need) {
        cand_key[greater + excl] = thr;
        cand_idx[greater + excl] = i;
      }
      __syncthreads();
      if (tid == 0) {
        uint32_t tot = s_carry;
        for (int w = 0; w < kWaves; ++w) tot += wave_cnt[w];
        s_carry = tot;
      }
      __syncthreads();
      if (s_carry >= need) break;                        // block-uniform
    }
    __syncthreads();
    for (int c = tid; c < K; c += kThreads) {
      const Key mk = cand_key[c];
      const int mi = cand_idx[c];
      int rank = 0;
      for (int j = 0; j < K; ++j) {
        const Key ok = cand_key[j];
        rank += (ok > mk || (ok == mk && cand_idx[j] < mi)) ? 1 : 0;
      }
      sel[rank] = mi;                                    // (the indices are distinct: the ranks are a permutation)
    }
    __syncthreads();
  }

  auto class_of = [&](int k) -> int {
    const int64_t c = topk ? (int64_t)sel[k] : classes_in[b * K + k];
    return (c >= 0 && c < (int64_t)C) ? (int)c : -1;
  };
  for (int k = tid; k < K; k += kThreads) {
    const int c = class_of(k);
    classes_out[b * K + k] = (int64_t)c;
    scores[b * K + k] = c < 0 ? (Rel)__builtin_nanf("") : L::up(row[c]);
  }
  if (seeds != nullptr)
    for (int k = 0; k < K; ++k)
      write_one_hot_row<Rel, typename L::Vec>(seeds + ((int64_t)k * B + b) * C, C, class_of(k));
}

template <typename T>
int class_targets(const T* logits, int64_t ld, int64_t B, int64_t C, int64_t K, const int64_t* classes_in,
                  int64_t* classes_out, typename Logit<T>::Rel* scores, typename Logit<T>::Rel* seeds, te_stream_t stream) {
  if (!logits || !classes_out || !scores || B <= 0 || C <= 0 || K <= 0 || ld < C) return TE_ERR_INVALID_ARG;
  if (!classes_in && K > C) return TE_ERR_INVALID_ARG;
  if (C > TE_CLASS_TARGETS_MAX_CLASSES || B > 0x7fffffff || K > TE_CLASS_TARGETS_MAX_CLASSES) return TE_ERR_UNSUPPORTED;
  if (!classes_in && K > kMaxTopK) return TE_ERR_UNSUPPORTED;
  class_targets_kernel<T><<<dim3((unsigned)B), dim3(kThreads), 0, (hipStream_t)stream>>>(logits, ld, B, (int)C, (int)K, classes_in,
                                                                                        classes_out, scores, seeds);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

}  // namespace

extern "C" int te_class_targets_f32(const float* logits, int64_t ld, int64_t B, int64_t C, int64_t K, const int64_t* classes_in,
                                    int64_t* classes_out, float* scores, float* seeds, te_stream_t stream) {
  return class_targets(logits, ld, B, C, K, classes_in, classes_out, scores, seeds, stream);
}

extern "C" int te_class_targets_bf16(const te_bf16_t* logits, int64_t ld, int64_t B, int64_t C, int64_t K,
                                     const int64_t* classes_in, int64_t* classes_out, float* scores, float* seeds,
                                     te_stream_t stream) {
  return class_targets(logits, ld, B, C, K, classes_in, classes_out, scores, seeds, stream);
}

extern "C" int te_class_targets_f64(const double* logits, int64_t ld, int64_t B, int64_t C, int64_t K, const int64_t* classes_in,
                                    int64_t* classes_out, double* scores, double* seeds, te_stream_t stream) {
  return class_targets(logits, ld, B, C, K, classes_in, classes_out, scores, seeds, stream);
}
