// te_conv_bf16.hip -- Conv2d.relprop, z^B rule, of a bf16 model's patch embedding (method="full") on bf16 MFMAs.
//
// Semantics (include/te_relprop.h, "bf16 operands"): the rule of te_conv.hip evaluated in fp32 on the model's own bf16 X and W;
// relevance in, relevance out fp32.  Per sample b, l_b / h_b = min / max pixel of X[b]:
//     Za  = conv(X, W) - l_b sum_k W+[e,k] - h_b sum_k W-[e,k] + 1e-9 ;  S = R / Za                 (plain division)
//     out = X convT(S, W) - l_b convT(S, W+) - h_b convT(S, W-)
// The fp32 kernel takes conv(X, W) from the layer's cached output; a bf16 layer's cached output is rounded to 8 significand
// bits, so here the product is RECOMPUTED from the bf16 operands (the cached output and the bias are not arguments).
//
// A stride == kernel convolution is a Linear layer on the im2col matrix [T = B Hp Wp, K = C p p]; both products run on
// v_mfma_f32_16x16x32_bf16 in the tile structure of te_bf16.hip's Linear rule (128 x 128 x 32 in LDS, four waves of 64 x 64):
//   Z-pass  A = X read THROUGH THE PATCH GEOMETRY of the NCHW image (p % 16 == 0: the 8 consecutive k of a lane's 16-byte load
//           lie in one image row, 16-byte aligned), B = W [E][K]: one plane each, every product exact in the fp32 accumulator.
//           Epilogue: Za with the per-ROW l_b / h_b (a 128-row tile holds patches of several samples), S = R / Za split into
//           three bf16 planes [3][T][E] (split3 of te_x6.h: S = p0 + p1 + p2 exactly).
//   C-pass  A = the three S planes, B = W+^T, W-^T [K][E]; P+ = S W+ and P- = S W- in one accumulator per weight sign, planes
//           smallest first inside a K step.  Epilogue: out = (x (P+ + P-) - l_b P+) - h_b P- (the expression of te_conv.hip),
//           x read from and out written to the image through the patch geometry.
// No fp32 copy of X or W, no im2col copy.  Every output's k-order is the plain k loop, independent of the grid and of T: a
// batch equals its samples bit for bit.  Rounding points: the fp32 accumulation of exact products (Z-pass), the subtraction
// of the two constant-image terms, the division, the fp32 accumulation of the C-pass, the epilogue's five operations.
#include "te_bf16_tile.h"
#include "te_x6.h"

namespace {

constexpr int kTile = 128;            // E and K = 3 p p must be multiples of it
constexpr int kMinMaxThreads = 1024;

// l_b, h_b of the bf16 image: one block per sample (zb_minmax_kernel of te_conv.hip on bf16 pixels)
__global__ __launch_bounds__(kMinMaxThreads) void zb16_minmax_kernel(const uint16_t* __restrict__ X, float* __restrict__ lohi,
                                                                   int64_t n) {
  __shared__ float s_lo[kMinMaxThreads / TE_WAVE], s_hi[kMinMaxThreads / TE_WAVE];
  const uint16_t* x = X + (int64_t)blockIdx.x * n;
  float lo = INFINITY, hi = -INFINITY;
  for (int64_t i = threadIdx.x; i < n; i += kMinMaxThreads) {
    const float v = bf(x[i]);
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = fminf(lo, __shfl_down(lo, off, TE_WAVE));
    hi = fmaxf(hi, __shfl_down(hi, off, TE_WAVE));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    s_lo[wave] = lo;
    s_hi[wave] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kMinMaxThreads / TE_WAVE; ++w) {
      lo = fminf(lo, s_lo[w]);
      hi = fmaxf(hi, s_hi[w]);
    }
    lohi[2 * blockIdx.x] = lo;
    lohi[2 * blockIdx.x + 1] = hi;
  }
}

// W [E][K] -> W+^T [K][E], W-^T [K][E]
__global__ __launch_bounds__(kThreads) void zb16_wplanes_kernel(const uint16_t* __restrict__ W, uint16_t* __restrict__ P,
                                                                int64_t E, int64_t K) {
  const int64_t n = E * K, stride = (int64_t)gridDim.x * kThreads;
  for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += stride) {
    const int64_t e = idx / K, k = idx % K, t = k * E + e;
    const uint16_t w = W[idx];
    const bool neg = (w & 0x8000u) != 0;
    P[t] = neg ? 0 : w;
    P[n + t] = neg ? w : 0;
  }
}

// cp[e] = sum_k max(W[e,k], 0), cn[e] = sum_k min(W[e,k], 0): one wave per output channel, fp64 accumulation
// (zb_wsum_kernel of te_conv.hip on the bf16 weight)
__global__ __launch_bounds__(256) void zb16_wsum_kernel(const uint16_t* __restrict__ W, float* __restrict__ cpn, int64_t E,
                                                        int64_t K) {
  const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= E) return;
  const int lane = threadIdx.x & 63;
  double sp = 0.0, sn = 0.0;
  for (int64_t k = lane; k < K; k += TE_WAVE) {
    const float w = bf(W[e * K + k]);
    sp += (double)fmaxf(w, 0.0f);
    sn += (double)fminf(w, 0.0f);
  }
  sp = te_wave_sum(sp);
  sn = te_wave_sum(sn);
  if (lane == 0) {
    cpn[2 * e] = (float)sp;
    cpn[2 * e + 1] = (float)sn;
  }
}

enum { PASS_Z = 0, PASS_C = 1 };

struct ZbArgs {
  const uint16_t* X;        // the NCHW image
  const uint16_t* W;        // PASS_Z: W [E][K]
  const uint16_t* Wt;       // PASS_C: W+^T [K][E], then W-^T [K][E]
  const float* R;           // PASS_Z: token-major relevance, samples r_bs floats apart
  int64_t r_bs;
  const float* cpn;         // PASS_Z: [E][2] channel sums of W+ / W-
  uint16_t* S;              // the planes [3][T][E]: written by PASS_Z, read by PASS_C
  float* out;               // PASS_C: NCHW
  int64_t T, E, K;
  TeZbGeom zb;              // lohi = the per-sample min / max
};

// C[m][n] = sum_k A[m][k] B[n][k], M = T rows of patches.  PASS_Z: N = E, k over K; PASS_C: N = K, k over E.
template <int PASS>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2))) void zb16_kernel(ZbArgs a) {
  constexpr int NPA = (PASS == PASS_C) ? 3 : 1, NB = (PASS == PASS_C) ? 2 : 1;
  constexpr int FM = kTile / 32, FN = kTile / 32;
  __shared__ uint16_t sA[NPA][kTile][kLd];
  __shared__ uint16_t sB[NB][kTile][kLd];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wm = w >> 1, wn = w & 1;
  const int64_t m0 = (int64_t)blockIdx.y * kTile, n0 = (int64_t)blockIdx.x * kTile;
  const int64_t KD = (PASS == PASS_C) ? a.E : a.K, plane = a.T * a.E;
  // staging: this thread moves 16 bytes (8 k) of rows sr and sr + 64 of every operand tile per K step
  const int sr = threadIdx.x >> 2, kc = (threadIdx.x & 3) * 8;
  const uint16_t* arow[2];
  const uint16_t* brow[NB][2];
  bool aok[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int64_t t = m0 + sr + 64 * c;
    aok[c] = t < a.T;                       // rows past T are staged as zeros and never written
    const int64_t tt = aok[c] ? t : 0;
    arow[c] = (PASS == PASS_C) ? a.S + tt * a.E : a.X + te_zb_index(a.zb, tt, 0);
#pragma unroll
    for (int j = 0; j < NB; ++j)            // N is a multiple of the tile: every B row exists
      brow[j][c] = ((PASS == PASS_C) ? a.Wt + j * (a.K * a.E) : a.W) + (n0 + sr + 64 * c) * KD;
  }

  f32x4 acc[NB][FM][FN];
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int mi = 0; mi < FM; ++mi)
#pragma unroll
      for (int ni = 0; ni < FN; ++ni) acc[j][mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

  u16x8 ra[NPA][2], rb[NB][2];
  auto fetch = [&](int64_t k0) {
    // PASS_Z: k -> (c, dy, dx) of the patch; the 8 k of this lane share (c, dy) because p % 8 == 0
    const int64_t ak = (PASS == PASS_C) ? k0 + kc : te_zb_index(a.zb, 0, k0 + kc);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
      for (int q = 0; q < NPA; ++q)
        ra[q][c] = aok[c] ? *reinterpret_cast<const u16x8*>(arow[c] + q * plane + ak) : u16x8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < NB; ++j) rb[j][c] = *reinterpret_cast<const u16x8*>(brow[j][c] + k0 + kc);
    }
  };
  fetch(0);

  for (int64_t k0 = 0; k0 < KD; k0 += kBK) {
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
      for (int q = 0; q < NPA; ++q) *reinterpret_cast<u16x8*>(&sA[q][sr + 64 * c][kc]) = ra[q][c];
#pragma unroll
      for (int j = 0; j < NB; ++j) *reinterpret_cast<u16x8*>(&sB[j][sr + 64 * c][kc]) = rb[j][c];
    }
    __syncthreads();
    if (k0 + kBK < KD) fetch(k0 + kBK);       // the next K step's loads are in flight while this one computes
    bf16x8 b[NB][FN];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int ni = 0; ni < FN; ++ni) b[j][ni] = frag(sB[j], wn * (kTile / 2) + ni * 16 + (lane & 15), lane);
#pragma unroll
    for (int mi = 0; mi < FM; ++mi) {
      const int ar = wm * (kTile / 2) + mi * 16 + (lane & 15);
      bf16x8 af[NPA];
#pragma unroll
      for (int q = 0; q < NPA; ++q) af[q] = frag(sA[q], ar, lane);
#pragma unroll
      for (int ni = 0; ni < FN; ++ni)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
          for (int q = NPA - 1; q >= 0; --q) acc[j][mi][ni] = TE_MFMA16_BF16(af[q], b[j][ni], acc[j][mi][ni]);
    }
  }

  // epilogue: lane holds D[4 (lane >> 4) + i][lane & 15] of each 16 x 16 block
  int64_t coff[FN];       // PASS_C: column k = (c, dy, dx) inside a patch
#pragma unroll
  for (int ni = 0; ni < FN; ++ni)
    coff[ni] = (PASS == PASS_C) ? te_zb_index(a.zb, 0, n0 + wn * (kTile / 2) + ni * 16 + (lane & 15)) : 0;
#pragma unroll
  for (int mi = 0; mi < FM; ++mi)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t m = m0 + wm * (kTile / 2) + mi * 16 + 4 * (lane >> 4) + i;
      if (m >= a.T) continue;
      const int64_t sb = m / a.zb.P;          // the row's sample: l_b / h_b are per row, not per tile
      const float lo = a.zb.lohi[2 * sb], hi = a.zb.lohi[2 * sb + 1];
      if constexpr (PASS == PASS_Z) {
        const float* r = a.R + sb * a.r_bs + (m - sb * a.zb.P) * a.E;
#pragma unroll
        for (int ni = 0; ni < FN; ++ni) {
          const int64_t n = n0 + wn * (kTile / 2) + ni * 16 + (lane & 15);
          const float za = ((acc[0][mi][ni][i] - lo * a.cpn[2 * n]) - hi * a.cpn[2 * n + 1]) + 1e-9f;
          unsigned p[3];
          split3(r[n] / za, p);
#pragma unroll
          for (int q = 0; q < 3; ++q) a.S[q * plane + m * a.E + n] = (uint16_t)p[q];
        }
      } else {
        const int64_t roff = te_zb_index(a.zb, m, 0);
#pragma unroll
        for (int ni = 0; ni < FN; ++ni) {
          const int64_t at = roff + coff[ni];
          const float pp = acc[0][mi][ni][i], pn = acc[1][mi][ni][i];
          a.out[at] = (bf(a.X[at]) * (pp + pn) - lo * pp) - hi * pn;
        }
      }
    }
}

inline size_t s_bytes(int64_t T, int64_t E) { return te_align_up((size_t)3 * T * E * sizeof(uint16_t), 256); }
inline size_t wt_bytes(int64_t E, int64_t K) { return te_align_up((size_t)2 * E * K * sizeof(uint16_t), 256); }

}  // namespace

extern "C" int te_conv2d_zb_relprop_bf16_supported(int64_t C, int64_t E, int64_t p) {
  return C == 3 && p > 0 && p <= 1024 && E >= kTile && E % kTile == 0 && (C * p * p) % kTile == 0;
}

extern "C" size_t te_conv2d_zb_relprop_bf16_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W, int64_t E,
                                                            int64_t p) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || E <= 0 || p <= 0 || H % p || W % p) return 0;
  return s_bytes(B * (H / p) * (W / p), E) + te_align_up((size_t)B * 2 * sizeof(float), 256);
}

extern "C" size_t te_conv2d_zb_bf16_weight_planes_bytes(int64_t C, int64_t E, int64_t p) {
  if (C <= 0 || E <= 0 || p <= 0) return 0;
  return wt_bytes(E, C * p * p) + te_align_up((size_t)E * 2 * sizeof(float), 256);
}

extern "C" int te_conv2d_zb_bf16_prepare_weights(const te_bf16_t* W, int64_t C, int64_t E, int64_t p, void* planes,
                                                 size_t planes_bytes, te_stream_t stream_) {
  if (!W || !planes || C <= 0 || E <= 0 || p <= 0) return TE_ERR_INVALID_ARG;
  if (planes_bytes < te_conv2d_zb_bf16_weight_planes_bytes(C, E, p) || !te_aligned16(planes)) return TE_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t K = C * p * p;
  int64_t blocks = te_ceil_div(E * K, kThreads);
  if (blocks > 16384) blocks = 16384;
  zb16_wplanes_kernel<<<dim3((unsigned)blocks), dim3(kThreads), 0, stream>>>(W, (uint16_t*)planes, E, K);
  TE_RETURN_IF_LAUNCH_FAILED();
  zb16_wsum_kernel<<<dim3((unsigned)te_ceil_div(E, 4)), dim3(256), 0, stream>>>(
      W, (float*)((char*)planes + wt_bytes(E, K)), E, K);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

extern "C" int te_conv2d_zb_relprop_bf16(const float* R, int64_t r_bs, const te_bf16_t* X, const te_bf16_t* Wt,
                                         const void* w_planes, float* out, int64_t B, int64_t C, int64_t H, int64_t W,
                                         int64_t E, int64_t p, void* ws, size_t ws_bytes, te_stream_t stream_) {
  if (!R || !X || !Wt || !w_planes || !out || B <= 0 || C <= 0 || H <= 0 || W <= 0 || E <= 0 || p <= 0)
    return TE_ERR_INVALID_ARG;
  if (H % p || W % p) return TE_ERR_UNSUPPORTED;          // stride == kernel, no padding: whole patches only
  if (!te_conv2d_zb_relprop_bf16_supported(C, E, p)) return TE_ERR_UNSUPPORTED;
  const int64_t Hp = H / p, Wp = W / p, P = Hp * Wp, K = C * p * p, T = B * P;
  if (r_bs < P * E) return TE_ERR_INVALID_ARG;
  if (H * W * C > INT32_MAX || te_ceil_div(T, kTile) > 65535 || K / kTile > 65535) return TE_ERR_UNSUPPORTED;
  // the 16-byte loads of the GEMM loop: image rows (W % 16 == 0), weight rows and planes start 16-byte aligned
  if (!te_aligned16(X) || !te_aligned16(Wt) || !te_aligned16(w_planes)) return TE_ERR_INVALID_ARG;
  if (!ws || ws_bytes < te_conv2d_zb_relprop_bf16_workspace_bytes(B, C, H, W, E, p) || !te_aligned16(ws))
    return TE_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  ZbArgs a;
  a.X = X;
  a.W = Wt;
  a.Wt = (const uint16_t*)w_planes;
  a.R = R;
  a.r_bs = r_bs;
  a.cpn = (const float*)((const char*)w_planes + wt_bytes(E, K));
  a.S = (uint16_t*)ws;
  a.out = out;
  a.T = T, a.E = E, a.K = K;
  float* lohi = (float*)((char*)ws + s_bytes(T, E));
  a.zb.lohi = lohi;
  a.zb.P = P;
  a.zb.C = (int)C;
  a.zb.H = (int)H;
  a.zb.W = (int)W;
  a.zb.p = (int)p;
  a.zb.Wp = (int)Wp;
  const unsigned gy = (unsigned)te_ceil_div(T, kTile);
  // a refused launch returns before the kernels that would read what it did not write
  zb16_minmax_kernel<<<dim3((unsigned)B), dim3(kMinMaxThreads), 0, stream>>>(X, lohi, C * H * W);
  TE_RETURN_IF_LAUNCH_FAILED();
  zb16_kernel<PASS_Z><<<dim3((unsigned)(E / kTile), gy), dim3(kThreads), 0, stream>>>(a);
  TE_RETURN_IF_LAUNCH_FAILED();
  zb16_kernel<PASS_C><<<dim3((unsigned)(K / kTile), gy), dim3(kThreads), 0, stream>>>(a);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}
