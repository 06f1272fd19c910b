// te_attnlrp_patch.hip -- the last step of AttnLRP on a ViT: the eps-rule through the patch-embedding convolution, then
// input x G per pixel (include/te_relprop.h, section "AttnLRP, pixel level": the specification).  The convolution has
// stride == kernel, so it is a Linear layer on non-overlapping patches and the rule is the product
//     acc[t][(c,i,j)] = sum_e damp(G, y)[t][e] W[e][(c,i,j)]           [B P, E] x [E, C p p]
// whose epilogue reads the image through the patch geometry and sums the channels in fp64.  The [B P, C p p] intermediate is
// never written: a workgroup keeps its piece in MFMA accumulators and folds it into fp64 pixel sums channel by channel.
// Every output is ONE fp32 fma chain over e ascending per channel (an fp32-input MFMA is exactly that chain), so the bits do
// not depend on the tiling: the tiled kernel, the one-thread-per-pixel kernel, a sample alone and the same sample in a batch
// agree bit for bit.  No split along e, no atomics, no workspace.
// Templated on the type T of the cached operands Y, X, W: float, or te_bf16_t read exactly; G and out are fp32.
#include "te_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int64_t kMaxGrid = (int64_t)0x7fffffff;
// the tiled kernel: a workgroup of four waves owns kTM tokens x kTN pixel columns q = i p + j of every channel; wave w the
// 32 x 32 block at rows 32 (w >> 1), columns 32 (w & 1).  e is walked in chunks of kKE through LDS.
constexpr int kTM = 64, kTN = 64, kKE = 32;
constexpr int kAS = kKE + 1;      // row stride of the A tile: lanes 0 .. 31 read one column of 32 rows -> 32 banks
constexpr int kWS = 96;           // row stride of the W tile: the two lane halves read rows k, k + 1 -> banks 0 .. 31, 32 .. 63

static inline bool aligned_elem(const float* p) { return (((uintptr_t)p) & 3u) == 0; }
static inline bool aligned_elem(const te_bf16_t* p) { return (((uintptr_t)p) & 1u) == 0; }
// a group of four T on its natural boundary: 16 bytes of fp32, 8 bytes of bf16
static inline bool aligned_group(const float* p) { return te_aligned16(p); }
static inline bool aligned_group(const te_bf16_t* p) { return (((uintptr_t)p) & 7u) == 0; }

struct PatchArgs {
  int64_t g_bs, y_bs;      // batch strides of G and Y, in elements
  int64_t T, P;            // tokens = B P, patches per sample = Hp Wp
  int64_t C, H, W, E;
  int64_t p, pp, Wp;       // patch edge, p p, patches per row
  float eps;
};

template <bool VEC, class T>
__device__ __forceinline__ f32x4 stage4(const T* __restrict__ p) {
  if constexpr (VEC) {
    return te_up4(p);
  } else {
    return f32x4{te_up(p[0]), te_up(p[1]), te_up(p[2]), te_up(p[3])};
  }
}

// offset of pixel (token t, column q) inside one [H, W] plane, and the token's sample
__device__ __forceinline__ int64_t pixel_of(const PatchArgs& a, int64_t t, int64_t q, int64_t* b) {
  *b = t / a.P;
  const int64_t tl = t - *b * a.P, hp = tl / a.Wp, wp = tl - hp * a.Wp, i = q / a.p, j = q - i * a.p;
  return (hp * a.p + i) * a.W + wp * a.p + j;
}

// grid: (token tiles, column tiles).  E % kKE == 0, p p % kTN == 0 (te_patch_alrp_relevance_supported); any T.  One channel per
// walk over e, plain staging: the A tile is staged and damped again on every channel's walk (G and y are read C times).  Three
// channels sharing a walk (A staged once, three accumulator sets, 45 KB of LDS) and the next chunk prefetched into registers
// (254 VGPRs) both measured slower than this loop at ViT-B/16, batch 64 (DESIGN.md section 6 has the figures).
template <bool VEC, class T>
__global__ __launch_bounds__(kThreads) void patch_tiled_kernel(const float* __restrict__ G, const T* __restrict__ Y,
                                                                const T* __restrict__ X, const T* __restrict__ Wt,
                                                                float* __restrict__ out, PatchArgs a) {
  __shared__ __attribute__((aligned(16))) float As[kTM * kAS];
  __shared__ __attribute__((aligned(16))) float Ws[kKE * kWS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r31 = lane & 31, kh = lane >> 5;
  const int rowb = 32 * (wave >> 1), colb = 32 * (wave & 1);
  const int64_t t0 = (int64_t)blockIdx.x * kTM, q0 = (int64_t)blockIdx.y * kTN;
  const int64_t K = a.C * a.pp, HW = a.H * a.W;

  // the A rows this thread stages: groups g = tid, tid + 256 of four e; row g >> 3, columns 4 (g & 7) ..
  const float* grow[2];
  const T* yrow[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int g = tid + kThreads * s;
    const int64_t t = t0 + (g >> 3);
    grow[s] = nullptr;
    yrow[s] = nullptr;
    if (t < a.T) {
      const int64_t b = t / a.P, tl = t - b * a.P;
      grow[s] = G + b * a.g_bs + tl * a.E + 4 * (g & 7);
      yrow[s] = Y + b * a.y_bs + tl * a.E + 4 * (g & 7);
    }
  }

  // the 16 pixels of this lane: accumulator element r is token row rowb + crow(r, kh), column q0 + colb + r31
  int64_t pix[16], smp[16];
  double sum[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t t = t0 + rowb + crow(r, kh);
    sum[r] = 0.0;
    smp[r] = -1;
    pix[r] = 0;
    if (t < a.T) pix[r] = pixel_of(a, t, q0 + colb + r31, &smp[r]);
  }

  for (int64_t c = 0; c < a.C; ++c) {
    f32x16 acc;
    zero16(acc);
    for (int64_t e0 = 0; e0 < a.E; e0 += kKE) {
      __syncthreads();      // the previous chunk has been read
      const TeAlrpDamp damp{a.eps};
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int g = tid + kThreads * s;
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (grow[s]) {
          const f32x4 vg = stage4<VEC>(grow[s] + e0), vy = stage4<VEC>(yrow[s] + e0);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = damp(vg[j], vy[j]);
        }
        float* dst = As + (g >> 3) * kAS + 4 * (g & 7);
#pragma unroll
        for (int j = 0; j < 4; ++j) dst[j] = v[j];
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int g = tid + kThreads * s, er = g >> 4, c4 = 4 * (g & 15);
        const f32x4 v = stage4<VEC>(Wt + (e0 + er) * K + c * a.pp + q0 + c4);
        *reinterpret_cast<f32x4*>(Ws + er * kWS + c4) = v;
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < kKE / 2; ++kk) {      // k = 2 kk + kh: e ascending inside the MFMA and from one MFMA to the next
        const float av = As[(rowb + r31) * kAS + 2 * kk + kh];
        const float bv = Ws[(2 * kk + kh) * kWS + colb + r31];
        acc = TE_MFMA32(av, bv, acc);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (smp[r] >= 0) {
        const float x = te_up(X[(smp[r] * a.C + c) * HW + pix[r]]);
        sum[r] = sum[r] + (double)x * (double)acc[r];
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (smp[r] >= 0) out[smp[r] * HW + pix[r]] = (float)sum[r];      // lanes along q: runs of p pixels along w
}

// one thread per output pixel, literal fmaf chains; any C, E, p >= 1.  Four channels share one walk over e (each its own
// chain); the channels are folded in ascending order.
template <class T>
__global__ __launch_bounds__(kThreads) void patch_simple_kernel(const float* __restrict__ G, const T* __restrict__ Y,
                                                                 const T* __restrict__ X, const T* __restrict__ Wt,
                                                                 float* __restrict__ out, PatchArgs a, int64_t n) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= n) return;
  const int64_t HW = a.H * a.W, K = a.C * a.pp;
  const int64_t b = idx / HW, rem = idx - b * HW, h = rem / a.W, w = rem - h * a.W;
  const int64_t hp = h / a.p, i = h - hp * a.p, wp = w / a.p, j = w - wp * a.p;
  const int64_t tl = hp * a.Wp + wp, q = i * a.p + j;
  const float* g = G + b * a.g_bs + tl * a.E;
  const T* y = Y + b * a.y_bs + tl * a.E;
  const TeAlrpDamp damp{a.eps};
  double sum = 0.0;
  for (int64_t c0 = 0; c0 < a.C; c0 += 4) {
    const int nc = (int)((a.C - c0 < 4) ? a.C - c0 : 4);
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const T* wcol = Wt + c0 * a.pp + q;
    for (int64_t e = 0; e < a.E; ++e) {
      const float av = damp(g[e], te_up(y[e]));
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (u < nc) acc[u] = __builtin_fmaf(av, te_up(wcol[e * K + u * a.pp]), acc[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (u < nc) {
        const float x = te_up(X[(b * a.C + c0 + u) * HW + rem]);
        sum = sum + (double)x * (double)acc[u];
      }
  }
  out[idx] = (float)sum;
}

bool tiled_takes(int64_t C, int64_t E, int64_t p) {
  return C >= 1 && E >= kKE && E % kKE == 0 && p >= 1 && p <= 1024 && (p * p) % kTN == 0;
}

bool finite_not_negative(float v) { return v >= 0.0f && v <= 3.402823466e+38f; }

template <class T>
int patch_relevance(const float* G, int64_t g_bs, const T* Y, int64_t y_bs, const T* X, const T* W, float* out, int64_t B,
                    int64_t C, int64_t H, int64_t Wd, int64_t E, int64_t p, float eps, int flags, hipStream_t stream) {
  if (!G || !Y || !X || !W || !out || B <= 0 || C <= 0 || H <= 0 || Wd <= 0 || E <= 0 || p <= 0) return TE_ERR_INVALID_ARG;
  if ((flags & ~TE_IMPL_SIMPLE) != 0 || !finite_not_negative(eps)) return TE_ERR_INVALID_ARG;
  if (H % p != 0 || Wd % p != 0) return TE_ERR_INVALID_ARG;
  if (H > kMaxGrid || Wd > kMaxGrid || E > kMaxGrid || C > kMaxGrid) return TE_ERR_UNSUPPORTED;
  const int64_t Hp = H / p, Wp = Wd / p, P = Hp * Wp;
  if (P > kMaxGrid / E) return TE_ERR_UNSUPPORTED;
  if (g_bs < P * E || y_bs < P * E) return TE_ERR_INVALID_ARG;
  if (((uintptr_t)G & 3u) || !aligned_elem(Y) || !aligned_elem(X) || !aligned_elem(W) || ((uintptr_t)out & 3u))
    return TE_ERR_UNSUPPORTED;
  // every index of both kernels stays far inside 63 bits
  if (C > kMaxGrid / (p * p) || B > kMaxGrid / P || H * Wd > kMaxGrid || B * C > ((int64_t)1 << 40) / (H * Wd) ||
      E * C > ((int64_t)1 << 40) / (p * p) || g_bs > ((int64_t)1 << 40) / B || y_bs > ((int64_t)1 << 40) / B)
    return TE_ERR_UNSUPPORTED;
  const PatchArgs a{g_bs, y_bs, B * P, P, C, H, Wd, E, p, p * p, Wp, eps};
  if (!(flags & TE_IMPL_SIMPLE) && tiled_takes(C, E, p)) {
    const int64_t tiles = te_ceil_div(a.T, kTM), qtiles = a.pp / kTN;
    if (tiles > kMaxGrid || qtiles > 65535) return TE_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)tiles, (unsigned)qtiles), block(kThreads);
    const bool vec = te_aligned16(G) && aligned_group(Y) && aligned_group(W) && g_bs % 4 == 0 && y_bs % 4 == 0;
    if (vec)
      patch_tiled_kernel<true, T><<<grid, block, 0, stream>>>(G, Y, X, W, out, a);
    else
      patch_tiled_kernel<false, T><<<grid, block, 0, stream>>>(G, Y, X, W, out, a);
  } else {
    const int64_t n = B * H * Wd, blocks = te_ceil_div(n, kThreads);
    if (blocks > kMaxGrid) return TE_ERR_UNSUPPORTED;
    patch_simple_kernel<T><<<dim3((unsigned)blocks), dim3(kThreads), 0, stream>>>(G, Y, X, W, out, a, n);
  }
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

}  // namespace

extern "C" int te_patch_alrp_relevance_supported(int64_t C, int64_t E, int64_t p) { return tiled_takes(C, E, p) ? 1 : 0; }

extern "C" int te_patch_alrp_relevance_f32(const float* G, int64_t g_bs, const float* Y, int64_t y_bs, const float* X,
                                           const float* W, float* out, int64_t B, int64_t C, int64_t H, int64_t W_, int64_t E,
                                           int64_t p, float eps, int flags, te_stream_t stream) {
  return patch_relevance(G, g_bs, Y, y_bs, X, W, out, B, C, H, W_, E, p, eps, flags, (hipStream_t)stream);
}

extern "C" int te_patch_attnlrp_relevance_bf16(const float* G, int64_t g_bs, const te_bf16_t* Y, int64_t y_bs,
                                               const te_bf16_t* X, const te_bf16_t* W, float* out, int64_t B, int64_t C,
                                               int64_t H, int64_t W_, int64_t E, int64_t p, float eps, int flags,
                                               te_stream_t stream) {
  return patch_relevance(G, g_bs, Y, y_bs, X, W, out, B, C, H, W_, E, p, eps, flags, (hipStream_t)stream);
}
