// te_bf16.hip -- the GEMM-shaped relprop rules of a bf16 model (Linear, the two attention products) on bf16 MFMAs.
//
// Semantics (include/te_relprop.h, "bf16 operands"): the reference's rule evaluated in fp32 on the model's own bf16
// tensors.  A bf16 operand is read exactly (bf16 -> fp32 is exact) and enters an MFMA as ONE bf16 plane; the only fp32
// operand of a product is S = safe_divide(R, Z), which enters as the exact sum of three bf16 planes (split3_u16, the split
// of te_x6.h).  Every bf16 x bf16 product is exact in the fp32 accumulator of v_mfma_f32_16x16x32_bf16, so each
// product of a rule is an fp32-accumulated sum of exact terms.
//
//   Linear   Z-pass   Z = [X+ | X-] . [W+ | W-]^T        (X+ / X- split from the bf16 X in registers; all terms >= 0)
//                     epilogue: S = sd(R * f, Z) written as three bf16 planes [3][T][out]
//            C-pass   C+ = S . W+, C- = S . W-          (3 planes x 2 weight signs: 6 products)
//                     epilogue: out = X+ . C+ + X- . C-
//   AV       S = sd(R, Z) as planes [3][B H][N][D]; cam_attn = attn . (S v^T), cam_v = v . (attn^T S)   (3 products each)
//   QK       S = sd(R * f, Z) as planes [3][B H][N][N]; cam_q = q . (S k), cam_k = k . (S^T q)          (3 products each)
//   (Z of an attention rule is the forward product the model cached; when it is absent it is recomputed in fp32 from the
//    bf16 operands by the same GEMM loop.)
//
// The two products of the AttnLRP chain on a bf16 model (te_relprop.h, "AttnLRP", bf16 operands) run on the same loop: their
// fp32 operand (damp(G, Y); G_o; d_s) is written as three planes by a streaming pass of te_attnlrp.hip, the other operand is a
// bf16 tensor of the model read in place, one accumulator per plane, summed smallest first.
//   Linear     out = A . W, A = damp(G, Y) as planes [3][T][out]; W [out][in] read in place as the transposed view, or its
//              transpose [in][out] (a cached plane) read along k
//   Attention  d_attn = G_o . v^T, d_v = attn^T . G_o (G_o as planes); d_s = p (.) (d_attn - rowsum(d_attn (.) p)) as planes;
//              d_q = scale d_s . k, d_k = scale d_s^T . q
//
// One GEMM loop (gemm_kernel): C[m][n] = sum_k A[m][k] B[n][k] over a batch z, every operand a bf16 view with arbitrary
// strides (row stride sr, k stride sk), so strided views -- q / k / v inside the fused qkv activation, the cls rows of
// Block.relprop_cls_only -- are read in place.  Tile BM x BN x 32 in LDS, four waves of (BM/2) x (BN/2), 16x16x32 MFMAs.
// Every output's k-order is the plain k loop (planes / weight signs in a fixed order inside a K step), independent of the
// grid and of the number of rows: a batch equals its samples bit for bit.
#include <cstring>

#include "te_bf16_tile.h"
#include "te_internal.h"

namespace {

constexpr int kLinTile = 128;         // Linear tiles (and the multiple in_f / out_f must have)
constexpr int kAttTile = 64;

// x = p[0] + p[1] + p[2] exactly: the split of te_x6.h, one value at a time, planes as stored (16 bits).  Local on purpose: the
// same bits as te_x6.h's split3, but that one is a view of split3_pk and carries a second (zero) lane through the three
// rounds, which changes the instructions of the two kernels below (scripts/isa_diff.py); kept so that they stay as measured.
__device__ __forceinline__ void split3_u16(float x, uint16_t (&p)[3]) {
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const unsigned u = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{x, 0.0f}, bf16x2));
    p[q] = (uint16_t)(u & 0xffffu);
    x = x - __uint_as_float(u << 16);
  }
}

struct Mat {        // bf16 [rows x K] of batch z: element (r, k) at p + (z / zh) sb + (z % zh) sh + q ps + r sr + k sk
  const uint16_t* p;
  int64_t sb, sh, sr, sk, ps;
};

enum { A_PLAIN = 0, A_SIGNS = 1, A_PLANES3 = 3 };
enum { EPI_F32 = 0, EPI_GATE = 1, EPI_SIGNS = 2, EPI_SPLANES = 3, EPI_SCALE = 4 };

struct GemmArgs {
  Mat A, B[2];
  int64_t M, N, K, zh;
  float* out;                         // EPI_F32 / EPI_GATE / EPI_SIGNS: fp32 element (z, m, n)
  int64_t o_sb, o_sh, o_sm, o_sn;
  const uint16_t* g;                  // EPI_GATE / EPI_SIGNS: bf16 multiplier at (z, m, n)
  int64_t g_sb, g_sh, g_sm, g_sn;
  float scale;                        // EPI_GATE, EPI_SCALE
  const float* R;                     // EPI_SPLANES: R [M][r_ld], optional per-sample factor rs[(m / rps) rs_stride]
  int64_t r_ld;
  const float* rs;
  int64_t rs_stride, rps;
  uint16_t* planes;                   // EPI_SPLANES: [3][M][N]
};

// One BR x 32 tile of a bf16 view, staged global -> registers (fetch, issued one K step ahead) -> LDS (store); zero
// outside [rows) x [K).  k-contiguous views stream 16 B per lane; row-contiguous views (sr == 1) load 16 B along the rows
// and are stored transposed.
template <int BR>
struct Stage {
  u16x8 v[BR / 64];
};

__device__ __forceinline__ bool transposed(int64_t sr, int64_t sk) { return sr == 1 && sk != 1; }

template <int BR>
__device__ __forceinline__ void fetch(Stage<BR>& st, const uint16_t* base, int64_t sr, int64_t sk, int64_t rows,
                                      int64_t K, int64_t r0, int64_t k0) {
  const bool tr = transposed(sr, sk);
#pragma unroll
  for (int c = 0; c < BR / 64; ++c) {
    const int idx = threadIdx.x + c * kThreads;
    u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (tr) {
      const int kk = idx / (BR / 8), rc = (idx % (BR / 8)) * 8;
      const int64_t gr = r0 + rc, gk = k0 + kk;
      if (gk < K) {
        const uint16_t* p = base + gk * sk + gr;
        if (gr + 8 <= rows && (((uintptr_t)p) & 15) == 0) {
          v = *reinterpret_cast<const u16x8*>(p);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (gr + e < rows) v[e] = p[e];
        }
      }
    } else {
      const int r = idx >> 2, kc = (idx & 3) * 8;
      const int64_t gr = r0 + r, gk = k0 + kc;
      if (gr < rows) {
        const uint16_t* p = base + gr * sr + gk * sk;
        if (sk == 1 && gk + 8 <= K && (((uintptr_t)p) & 15) == 0) {
          v = *reinterpret_cast<const u16x8*>(p);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (gk + e < K) v[e] = p[e * sk];
        }
      }
    }
    st.v[c] = v;
  }
}

template <int BR>
__device__ __forceinline__ void store(const Stage<BR>& st, int64_t sr, int64_t sk, uint16_t (*lds)[kLd]) {
  const bool tr = transposed(sr, sk);
#pragma unroll
  for (int c = 0; c < BR / 64; ++c) {
    const int idx = threadIdx.x + c * kThreads;
    if (tr) {
      const int kk = idx / (BR / 8), rc = (idx % (BR / 8)) * 8;
#pragma unroll
      for (int e = 0; e < 8; ++e) lds[rc + e][kk] = st.v[c][e];
    } else {
      *reinterpret_cast<u16x8*>(&lds[idx >> 2][(idx & 3) * 8]) = st.v[c];
    }
  }
}

template <int BM, int BN, int AK, int NB, int EPI>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2))) void gemm_kernel(GemmArgs g) {
  constexpr int NPA = (AK == A_PLANES3) ? 3 : 1;
  // accumulators: one per weight sign (Linear C-pass), or -- a single B operand times three planes (attention) -- one
  // per plane, summed smallest first at the end: each plane's products are then rounded against their own magnitude
  // (64 x 64 tiles; a larger tile keeps the C-pass's arrangement, one accumulator that takes the planes smallest first inside
  // every K step: three accumulators of it do not fit the 256 registers of two waves per SIMD)
  constexpr bool PER_PLANE = (AK == A_PLANES3 && NB == 1 && BM * BN <= kAttTile * kAttTile);
  constexpr int NACC = (AK == A_SIGNS) ? 1 : (PER_PLANE ? 3 : NB);
  constexpr int FM = BM / 32, FN = BN / 32;
  __shared__ uint16_t sA[NPA][BM][kLd];
  __shared__ uint16_t sB[NB][BN][kLd];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wm = w >> 1, wn = w & 1;
  const int64_t z = blockIdx.z, zb = z / g.zh, zhh = z % g.zh;
  const int64_t m0 = (int64_t)blockIdx.y * BM, n0 = (int64_t)blockIdx.x * BN;
  const uint16_t* abase = g.A.p + zb * g.A.sb + zhh * g.A.sh;
  const uint16_t* bbase[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) bbase[j] = g.B[j].p + zb * g.B[j].sb + zhh * g.B[j].sh;

  f32x4 acc[NACC][FM][FN];
#pragma unroll
  for (int j = 0; j < NACC; ++j)
#pragma unroll
    for (int mi = 0; mi < FM; ++mi)
#pragma unroll
      for (int ni = 0; ni < FN; ++ni) acc[j][mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

  Stage<BM> ra[NPA];
  Stage<BN> rb[NB];
#pragma unroll
  for (int q = 0; q < NPA; ++q) fetch<BM>(ra[q], abase + q * g.A.ps, g.A.sr, g.A.sk, g.M, g.K, m0, 0);
#pragma unroll
  for (int j = 0; j < NB; ++j) fetch<BN>(rb[j], bbase[j], g.B[j].sr, g.B[j].sk, g.N, g.K, n0, 0);

  for (int64_t k0 = 0; k0 < g.K; k0 += kBK) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NPA; ++q) store<BM>(ra[q], g.A.sr, g.A.sk, sA[q]);
#pragma unroll
    for (int j = 0; j < NB; ++j) store<BN>(rb[j], g.B[j].sr, g.B[j].sk, sB[j]);
    __syncthreads();
    if (k0 + kBK < g.K) {       // the next K step's loads are in flight while this one computes
#pragma unroll
      for (int q = 0; q < NPA; ++q) fetch<BM>(ra[q], abase + q * g.A.ps, g.A.sr, g.A.sk, g.M, g.K, m0, k0 + kBK);
#pragma unroll
      for (int j = 0; j < NB; ++j) fetch<BN>(rb[j], bbase[j], g.B[j].sr, g.B[j].sk, g.N, g.K, n0, k0 + kBK);
    }
    bf16x8 b[NB][FN];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int ni = 0; ni < FN; ++ni) b[j][ni] = frag(sB[j], wn * (BN / 2) + ni * 16 + (lane & 15), lane);
#pragma unroll
    for (int mi = 0; mi < FM; ++mi) {
      const int ar = wm * (BM / 2) + mi * 16 + (lane & 15);
      if constexpr (AK == A_SIGNS) {
        // X+ / X- of one bf16 fragment: the sign bit selects the plane (-0 lands in X-, where it adds 0)
        const u16x8 x = *reinterpret_cast<const u16x8*>(&sA[0][ar][8 * (lane >> 4)]);
        const u16x8 neg = (u16x8)(-(x >> 15));
        const bf16x8 xp = __builtin_bit_cast(bf16x8, (u16x8)(x & ~neg));
        const bf16x8 xn = __builtin_bit_cast(bf16x8, (u16x8)(x & neg));
#pragma unroll
        for (int ni = 0; ni < FN; ++ni) {
          acc[0][mi][ni] = TE_MFMA16_BF16(xp, b[0][ni], acc[0][mi][ni]);
          acc[0][mi][ni] = TE_MFMA16_BF16(xn, b[NB - 1][ni], acc[0][mi][ni]);
        }
      } else {
        bf16x8 a[NPA];
#pragma unroll
        for (int q = 0; q < NPA; ++q) a[q] = frag(sA[q], ar, lane);
#pragma unroll
        for (int ni = 0; ni < FN; ++ni)
#pragma unroll
          for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int q = NPA - 1; q >= 0; --q) {
              f32x4& c = acc[PER_PLANE ? q : j][mi][ni];
              c = TE_MFMA16_BF16(a[q], b[j][ni], c);
            }
      }
    }
  }

  // epilogue: lane holds D[4 (lane >> 4) + i][lane & 15] of each 16 x 16 block
#pragma unroll
  for (int mi = 0; mi < FM; ++mi)
#pragma unroll
    for (int ni = 0; ni < FN; ++ni)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t m = m0 + wm * (BM / 2) + mi * 16 + 4 * (lane >> 4) + i;
        const int64_t n = n0 + wn * (BN / 2) + ni * 16 + (lane & 15);
        if (m >= g.M || n >= g.N) continue;
        float v = acc[0][mi][ni][i];
        if constexpr (PER_PLANE) v = (acc[2][mi][ni][i] + acc[1][mi][ni][i]) + v;
        if constexpr (EPI == EPI_SPLANES) {
          float r = g.R[m * g.r_ld + n];
          if (g.rs) r = r * g.rs[(m / g.rps) * g.rs_stride];
          uint16_t p[3];
          split3_u16(te_sd(r, v), p);
          const int64_t o = m * g.N + n, ps = g.M * g.N;
#pragma unroll
          for (int q = 0; q < 3; ++q) g.planes[q * ps + o] = p[q];
        } else {
          float* o = g.out + zb * g.o_sb + zhh * g.o_sh + m * g.o_sm + n * g.o_sn;
          if constexpr (EPI == EPI_F32) {
            *o = v;
          } else if constexpr (EPI == EPI_SCALE) {
            *o = v * g.scale;
          } else {
            const float x = bf(g.g[zb * g.g_sb + zhh * g.g_sh + m * g.g_sm + n * g.g_sn]);
            if constexpr (EPI == EPI_GATE) {
              *o = (x * v) * g.scale;
            } else {       // EPI_SIGNS: X+ C+ + X- C-
              const float xp = fmaxf(x, 0.0f), xn = fminf(x, 0.0f);
              *o = xp * v + xn * acc[NACC - 1][mi][ni][i];
            }
          }
        }
      }
}

// S = sd(R * f, Z) of an attention rule as three bf16 planes [3][B H][N][C] (contiguous); R and Z strided per (b, h, n),
// contiguous in the last dimension; Z is the model's bf16 product (TZ = uint16_t) or an fp32 recomputation.  One row
// (b, h, n) per 64-lane block.
template <typename TZ>
__global__ __launch_bounds__(64) void s_planes_kernel(const float* __restrict__ R, int64_t r_sb, int64_t r_sh,
                                                      int64_t r_sn, const float* __restrict__ rs, int64_t rs_stride,
                                                      const TZ* __restrict__ Z, int64_t z_sb, int64_t z_sh, int64_t z_sn,
                                                      uint16_t* __restrict__ planes, int64_t H, int64_t N, int64_t C,
                                                      int64_t total) {
  const int64_t row = blockIdx.x, n = row % N, bh = row / N, h = bh % H, b = bh / H;
  const float* r = R + b * r_sb + h * r_sh + n * r_sn;
  const TZ* zr = Z + b * z_sb + h * z_sh + n * z_sn;
  const float f = rs ? rs[b * rs_stride] : 1.0f;
  uint16_t* out = planes + row * C;
  for (int64_t c = threadIdx.x; c < C; c += 64) {
    float rv = r[c];
    if (rs) rv = rv * f;
    float zv;
    if constexpr (sizeof(TZ) == 2) zv = bf(zr[c]);
    else zv = zr[c];
    uint16_t p[3];
    split3_u16(te_sd(rv, zv), p);
#pragma unroll
    for (int q = 0; q < 3; ++q) out[q * total + c] = p[q];
  }
}

// W [out][in] -> W+ [out][in], W- [out][in], W+^T [in][out], W-^T [in][out]
__global__ __launch_bounds__(kThreads) void weight_planes_kernel(const uint16_t* __restrict__ W, uint16_t* __restrict__ P,
                                                                 int64_t in_f, int64_t out_f) {
  const int64_t n = in_f * out_f, stride = (int64_t)gridDim.x * kThreads;
  for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += stride) {
    const int64_t o = idx / in_f, i = idx % in_f, t = i * out_f + o;
    const uint16_t w = W[idx];
    const bool neg = (w & 0x8000u) != 0;
    P[idx] = neg ? 0 : w;
    P[n + idx] = neg ? w : 0;
    P[2 * n + t] = neg ? 0 : w;
    P[3 * n + t] = neg ? w : 0;
  }
}

template <int BM, int BN, int AK, int NB, int EPI>
int launch(const GemmArgs& g, int64_t Z, hipStream_t stream) {
  const int64_t gx = te_ceil_div(g.N, BN), gy = te_ceil_div(g.M, BM);
  if (gx > 65535 || gy > 65535 || Z > 65535) return TE_ERR_UNSUPPORTED;
  gemm_kernel<BM, BN, AK, NB, EPI><<<dim3((unsigned)gx, (unsigned)gy, (unsigned)Z), dim3(kThreads), 0, stream>>>(g);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

GemmArgs blank() {
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.zh = 1;
  g.scale = 1.0f;
  g.rps = 1;
  return g;
}

int s_planes(const float* R, int64_t r_sb, int64_t r_sh, int64_t r_sn, const float* rs, int64_t rs_stride,
             const void* Z, bool z_bf16, int64_t z_sb, int64_t z_sh, int64_t z_sn, uint16_t* planes, int64_t B,
             int64_t H, int64_t N, int64_t C, hipStream_t stream) {
  const int64_t total = B * H * N * C, rows = B * H * N;
  if (rows > 0x7fffffff) return TE_ERR_UNSUPPORTED;
  const dim3 blocks((unsigned)rows);
  if (z_bf16)
    s_planes_kernel<uint16_t><<<blocks, dim3(64), 0, stream>>>(
        R, r_sb, r_sh, r_sn, rs, rs_stride, (const uint16_t*)Z, z_sb, z_sh, z_sn, planes, H, N, C, total);
  else
    s_planes_kernel<float><<<blocks, dim3(64), 0, stream>>>(
        R, r_sb, r_sh, r_sn, rs, rs_stride, (const float*)Z, z_sb, z_sh, z_sn, planes, H, N, C, total);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

inline size_t planes_bytes(int64_t n) { return te_align_up((size_t)3 * n * sizeof(uint16_t), 256); }

}  // namespace

// ================================================================================================ Linear
extern "C" int te_linear_relprop_bf16_supported(int64_t T, int64_t in_f, int64_t out_f) {
  return T > 0 && in_f >= kLinTile && out_f >= kLinTile && in_f % kLinTile == 0 && out_f % kLinTile == 0 &&
         te_ceil_div(T, kLinTile) <= 65535;
}

extern "C" size_t te_linear_relprop_bf16_workspace_bytes(int64_t T, int64_t in_f, int64_t out_f) {
  if (T <= 0 || in_f <= 0 || out_f <= 0) return 0;
  return planes_bytes(T * out_f);
}

extern "C" size_t te_linear_bf16_weight_planes_bytes(int64_t in_f, int64_t out_f) {
  if (in_f <= 0 || out_f <= 0) return 0;
  return te_align_up((size_t)4 * in_f * out_f * sizeof(uint16_t), 256);
}

extern "C" int te_linear_bf16_prepare_weights(const te_bf16_t* W, int64_t in_f, int64_t out_f, void* planes,
                                              size_t planes_bytes_, te_stream_t stream_) {
  if (!W || !planes || in_f <= 0 || out_f <= 0) return TE_ERR_INVALID_ARG;
  if (planes_bytes_ < te_linear_bf16_weight_planes_bytes(in_f, out_f)) return TE_ERR_WORKSPACE;
  int64_t blocks = te_ceil_div(in_f * out_f, kThreads);
  if (blocks > 16384) blocks = 16384;
  weight_planes_kernel<<<dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream_>>>(W, (uint16_t*)planes, in_f,
                                                                                            out_f);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

extern "C" int te_linear_relprop_bf16(const float* R, int64_t r_ld, const float* r_scale, int64_t r_scale_stride,
                                      int64_t rows_per_scale, const te_bf16_t* X, int64_t x_ld, const void* w_planes,
                                      float* out, int64_t T, int64_t in_f, int64_t out_f, void* ws, size_t ws_bytes,
                                      te_stream_t stream_) {
  if (!R || !X || !w_planes || !out || T <= 0 || in_f <= 0 || out_f <= 0) return TE_ERR_INVALID_ARG;
  if (r_ld < out_f || x_ld < in_f || (r_scale && rows_per_scale <= 0)) return TE_ERR_INVALID_ARG;
  if (!te_linear_relprop_bf16_supported(T, in_f, out_f)) return TE_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < te_linear_relprop_bf16_workspace_bytes(T, in_f, out_f)) return TE_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const uint16_t* P = (const uint16_t*)w_planes;
  const int64_t nw = in_f * out_f;
  uint16_t* S = (uint16_t*)ws;
  // Z-pass + S planes
  GemmArgs z = blank();
  z.A = Mat{X, 0, 0, x_ld, 1, 0};
  z.B[0] = Mat{P, 0, 0, in_f, 1, 0};
  z.B[1] = Mat{P + nw, 0, 0, in_f, 1, 0};
  z.M = T, z.N = out_f, z.K = in_f;
  z.R = R, z.r_ld = r_ld, z.rs = r_scale, z.rs_stride = r_scale_stride, z.rps = r_scale ? rows_per_scale : 1;
  z.planes = S;
  int rc = launch<kLinTile, kLinTile, A_SIGNS, 2, EPI_SPLANES>(z, 1, stream);
  if (rc != TE_OK) return rc;
  // C-pass
  GemmArgs c = blank();
  c.A = Mat{S, 0, 0, out_f, 1, T * out_f};
  c.B[0] = Mat{P + 2 * nw, 0, 0, out_f, 1, 0};
  c.B[1] = Mat{P + 3 * nw, 0, 0, out_f, 1, 0};
  c.M = T, c.N = in_f, c.K = out_f;
  c.out = out, c.o_sm = in_f, c.o_sn = 1;
  c.g = X, c.g_sm = x_ld, c.g_sn = 1;
  return launch<kLinTile, kLinTile, A_PLANES3, 2, EPI_SIGNS>(c, 1, stream);
}

// ================================================================================================ attention
extern "C" int te_matmul_relprop_bf16_supported(int64_t N, int64_t D) {
  return N >= 1 && N <= 1024 && D == 64;
}

extern "C" size_t te_matmul_relprop_av_bf16_workspace_bytes(int64_t B, int64_t H, int64_t N, int64_t D) {
  if (B <= 0 || H <= 0 || N <= 0 || D <= 0) return 0;
  return planes_bytes(B * H * N * D) + te_align_up((size_t)B * H * N * D * sizeof(float), 256);
}

extern "C" size_t te_matmul_relprop_qk_bf16_workspace_bytes(int64_t B, int64_t H, int64_t N, int64_t D) {
  if (B <= 0 || H <= 0 || N <= 0 || D <= 0) return 0;
  return planes_bytes(B * H * N * N) + te_align_up((size_t)B * H * N * N * sizeof(float), 256);
}

extern "C" int te_matmul_relprop_av_bf16(const float* R, int64_t r_sb, int64_t r_sh, int64_t r_sn, const te_bf16_t* attn,
                                         const te_bf16_t* v, int64_t v_sb, int64_t v_sh, int64_t v_sn, const te_bf16_t* Z,
                                         int64_t z_sb, int64_t z_sh, int64_t z_sn, float* cam_attn, float* cam_v,
                                         int64_t cv_sb, int64_t cv_sh, int64_t cv_sn, int64_t B, int64_t H, int64_t N,
                                         int64_t D, float out_scale, int variant, void* ws, size_t ws_bytes,
                                         te_stream_t stream_) {
  if (!R || !attn || !v || !cam_attn || !cam_v || B <= 0 || H <= 0 || N <= 0 || D <= 0) return TE_ERR_INVALID_ARG;
  if ((variant & 0xff) != TE_VARIANT_OURS) return TE_ERR_UNSUPPORTED;
  if (!te_matmul_relprop_bf16_supported(N, D) || B * H > 65535) return TE_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < te_matmul_relprop_av_bf16_workspace_bytes(B, H, N, D)) return TE_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t nd = N * D, nn = N * N;
  uint16_t* S = (uint16_t*)ws;
  float* zf = (float*)((char*)ws + planes_bytes(B * H * nd));
  int rc;
  if (Z) {
    rc = s_planes(R, r_sb, r_sh, r_sn, nullptr, 0, Z, true, z_sb, z_sh, z_sn, S, B, H, N, D, stream);
  } else {      // Z = attn v in fp32 from the bf16 operands
    GemmArgs g = blank();
    g.A = Mat{attn, H * nn, nn, N, 1, 0};
    g.B[0] = Mat{v, v_sb, v_sh, 1, v_sn, 0};
    g.M = N, g.N = D, g.K = N, g.zh = H;
    g.out = zf, g.o_sb = H * nd, g.o_sh = nd, g.o_sm = D, g.o_sn = 1;
    rc = launch<kAttTile, kAttTile, A_PLAIN, 1, EPI_F32>(g, B * H, stream);
    if (rc == TE_OK) rc = s_planes(R, r_sb, r_sh, r_sn, nullptr, 0, zf, false, H * nd, nd, D, S, B, H, N, D, stream);
  }
  if (rc != TE_OK) return rc;
  // cam_attn[i][j] = attn[i][j] sum_d S[i][d] v[j][d]
  GemmArgs a = blank();
  a.A = Mat{S, H * nd, nd, D, 1, B * H * nd};
  a.B[0] = Mat{v, v_sb, v_sh, v_sn, 1, 0};
  a.M = N, a.N = N, a.K = D, a.zh = H;
  a.out = cam_attn, a.o_sb = H * nn, a.o_sh = nn, a.o_sm = N, a.o_sn = 1;
  a.g = attn, a.g_sb = H * nn, a.g_sh = nn, a.g_sm = N, a.g_sn = 1;
  a.scale = out_scale;
  rc = launch<kAttTile, kAttTile, A_PLANES3, 1, EPI_GATE>(a, B * H, stream);
  if (rc != TE_OK) return rc;
  // cam_v[j][d] = v[j][d] sum_i attn[i][j] S[i][d], evaluated as the transposed product (m = d, n = j)
  GemmArgs c = blank();
  c.A = Mat{S, H * nd, nd, 1, D, B * H * nd};
  c.B[0] = Mat{attn, H * nn, nn, 1, N, 0};
  c.M = D, c.N = N, c.K = N, c.zh = H;
  c.out = cam_v, c.o_sb = cv_sb, c.o_sh = cv_sh, c.o_sm = 1, c.o_sn = cv_sn;
  c.g = v, c.g_sb = v_sb, c.g_sh = v_sh, c.g_sm = 1, c.g_sn = v_sn;
  c.scale = out_scale;
  return launch<kAttTile, kAttTile, A_PLANES3, 1, EPI_GATE>(c, B * H, stream);
}

extern "C" int te_matmul_relprop_qk_bf16(const float* R_nn, const float* r_scale, int64_t r_scale_stride,
                                         const te_bf16_t* q, int64_t q_sb, int64_t q_sh, int64_t q_sn, const te_bf16_t* k,
                                         int64_t k_sb, int64_t k_sh, int64_t k_sn, const te_bf16_t* Z, float* cam_q,
                                         int64_t cq_sb, int64_t cq_sh, int64_t cq_sn, float* cam_k, int64_t ck_sb,
                                         int64_t ck_sh, int64_t ck_sn, int64_t B, int64_t H, int64_t N, int64_t D,
                                         float out_scale, int variant, void* ws, size_t ws_bytes, te_stream_t stream_) {
  if (!R_nn || !q || !k || !cam_q || !cam_k || B <= 0 || H <= 0 || N <= 0 || D <= 0) return TE_ERR_INVALID_ARG;
  if ((variant & 0xff) != TE_VARIANT_OURS) return TE_ERR_UNSUPPORTED;
  if (!te_matmul_relprop_bf16_supported(N, D) || B * H > 65535) return TE_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < te_matmul_relprop_qk_bf16_workspace_bytes(B, H, N, D)) return TE_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t nn = N * N;
  uint16_t* S = (uint16_t*)ws;
  float* zf = (float*)((char*)ws + planes_bytes(B * H * nn));
  int rc;
  if (Z) {
    rc = s_planes(R_nn, H * nn, nn, N, r_scale, r_scale_stride, Z, true, H * nn, nn, N, S, B, H, N, N, stream);
  } else {      // Z = q k^T (unscaled) in fp32 from the bf16 operands
    GemmArgs g = blank();
    g.A = Mat{q, q_sb, q_sh, q_sn, 1, 0};
    g.B[0] = Mat{k, k_sb, k_sh, k_sn, 1, 0};
    g.M = N, g.N = N, g.K = D, g.zh = H;
    g.out = zf, g.o_sb = H * nn, g.o_sh = nn, g.o_sm = N, g.o_sn = 1;
    rc = launch<kAttTile, kAttTile, A_PLAIN, 1, EPI_F32>(g, B * H, stream);
    if (rc == TE_OK)
      rc = s_planes(R_nn, H * nn, nn, N, r_scale, r_scale_stride, zf, false, H * nn, nn, N, S, B, H, N, N, stream);
  }
  if (rc != TE_OK) return rc;
  // cam_q[i][d] = q[i][d] sum_j S[i][j] k[j][d]
  GemmArgs a = blank();
  a.A = Mat{S, H * nn, nn, N, 1, B * H * nn};
  a.B[0] = Mat{k, k_sb, k_sh, 1, k_sn, 0};
  a.M = N, a.N = D, a.K = N, a.zh = H;
  a.out = cam_q, a.o_sb = cq_sb, a.o_sh = cq_sh, a.o_sm = cq_sn, a.o_sn = 1;
  a.g = q, a.g_sb = q_sb, a.g_sh = q_sh, a.g_sm = q_sn, a.g_sn = 1;
  a.scale = out_scale;
  rc = launch<kAttTile, kAttTile, A_PLANES3, 1, EPI_GATE>(a, B * H, stream);
  if (rc != TE_OK) return rc;
  // cam_k[j][d] = k[j][d] sum_i S[i][j] q[i][d]
  GemmArgs c = blank();
  c.A = Mat{S, H * nn, nn, 1, N, B * H * nn};
  c.B[0] = Mat{q, q_sb, q_sh, 1, q_sn, 0};
  c.M = N, c.N = D, c.K = N, c.zh = H;
  c.out = cam_k, c.o_sb = ck_sb, c.o_sh = ck_sh, c.o_sm = ck_sn, c.o_sn = 1;
  c.g = k, c.g_sb = k_sb, c.g_sh = k_sh, c.g_sm = k_sn, c.g_sn = 1;
  c.scale = out_scale;
  return launch<kAttTile, kAttTile, A_PLANES3, 1, EPI_GATE>(c, B * H, stream);
}

// ================================================================================================ AttnLRP
extern "C" int te_attnlrp_linear_bf16_supported(int64_t T, int64_t in_f, int64_t out_f) {
  return te_linear_relprop_bf16_supported(T, in_f, out_f);
}

extern "C" size_t te_attnlrp_linear_bf16_workspace_bytes(int64_t T, int64_t in_f, int64_t out_f) {
  if (T <= 0 || in_f <= 0 || out_f <= 0) return 0;
  return planes_bytes(T * out_f);
}

extern "C" int te_attnlrp_linear_bf16(const float* G, int64_t g_ld, const te_bf16_t* Y, int64_t y_ld, const te_bf16_t* W,
                                   int w_transposed, float* out, int64_t T, int64_t in_f, int64_t out_f, float eps, void* ws, size_t ws_bytes,
                                   te_stream_t stream_) {
  if (!G || !Y || !W || !out || T <= 0 || in_f <= 0 || out_f <= 0) return TE_ERR_INVALID_ARG;
  if (g_ld < out_f || y_ld < out_f) return TE_ERR_INVALID_ARG;
  if (!te_attnlrp_linear_bf16_supported(T, in_f, out_f)) return TE_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < te_attnlrp_linear_bf16_workspace_bytes(T, in_f, out_f)) return TE_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  uint16_t* A = (uint16_t*)ws;
  int rc = te_alrp::damp_planes_launch(G, Strided{0, 0, g_ld}, Y, Strided{0, 0, y_ld}, A, 1, 1, T, out_f, eps, stream);
  if (rc != TE_OK) return rc;
  // out[t][i] = sum_o A[t][o] W[o][i]: row i of the second operand is column i of W (sr == 1: staged transposed), or row i of
  // the contiguous W^T the caller keeps.  The same products in the same order either way.
  GemmArgs c = blank();
  c.A = Mat{A, 0, 0, out_f, 1, T * out_f};
  c.B[0] = w_transposed ? Mat{W, 0, 0, out_f, 1, 0} : Mat{W, 0, 0, 1, in_f, 0};
  c.M = T, c.N = in_f, c.K = out_f;
  c.out = out, c.o_sm = in_f, c.o_sn = 1;
  // (128 rows x 64 columns: with three staged planes of A and the transposed staging of W the 128 x 128 tile spills 63 VGPRs)
  return launch<kLinTile, kAttTile, A_PLANES3, 1, EPI_F32>(c, 1, stream);
}

extern "C" int te_attnlrp_attention_bf16_supported(int64_t N, int64_t D) { return te_matmul_relprop_bf16_supported(N, D); }

extern "C" size_t te_attnlrp_attention_bf16_workspace_bytes(int64_t B, int64_t H, int64_t N, int64_t D) {
  if (B <= 0 || H <= 0 || N <= 0 || D <= 0) return 0;
  return planes_bytes(B * H * N * D) + planes_bytes(B * H * N * N) + te_align_up((size_t)B * H * N * N * sizeof(float), 256);
}

extern "C" int te_attnlrp_attention_bf16(const float* G_o, int64_t g_sb, int64_t g_sh, int64_t g_sn, const te_bf16_t* q, int64_t q_sb,
                                      int64_t q_sh, int64_t q_sn, const te_bf16_t* k, int64_t k_sb, int64_t k_sh, int64_t k_sn,
                                      const te_bf16_t* v, int64_t v_sb, int64_t v_sh, int64_t v_sn, const te_bf16_t* attn,
                                      float scale, float* G_q, int64_t gq_sb, int64_t gq_sh, int64_t gq_sn, float* G_k,
                                      int64_t gk_sb, int64_t gk_sh, int64_t gk_sn, float* G_v, int64_t gv_sb, int64_t gv_sh,
                                      int64_t gv_sn, int64_t B, int64_t H, int64_t N, int64_t D, void* ws, size_t ws_bytes,
                                      te_stream_t stream_) {
  if (!G_o || !q || !k || !v || !attn || !G_q || !G_k || !G_v || B <= 0 || H <= 0 || N <= 0 || D <= 0) return TE_ERR_INVALID_ARG;
  if (!te_attnlrp_attention_bf16_supported(N, D) || B * H > 65535) return TE_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < te_attnlrp_attention_bf16_workspace_bytes(B, H, N, D)) return TE_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t nd = N * D, nn = N * N, BH = B * H;
  uint16_t* P = (uint16_t*)ws;                                         // G_o   [3][B H][N][D]
  uint16_t* S = (uint16_t*)((char*)ws + planes_bytes(BH * nd));        // d_s   [3][B H][N][N]
  float* dA = (float*)((char*)S + planes_bytes(BH * nn));             // d_attn   [B H][N][N]
  int rc = te_alrp::damp_planes_launch(G_o, Strided{g_sb, g_sh, g_sn}, nullptr, Strided{0, 0, 0}, P, B, H, N, D, 0.0f, stream);
  if (rc != TE_OK) return rc;
  // d_attn[i][j] = sum_d G_o[i][d] v[j][d]
  GemmArgs a = blank();
  a.A = Mat{P, H * nd, nd, D, 1, BH * nd};
  a.B[0] = Mat{v, v_sb, v_sh, v_sn, 1, 0};
  a.M = N, a.N = N, a.K = D, a.zh = H;
  a.out = dA, a.o_sb = H * nn, a.o_sh = nn, a.o_sm = N, a.o_sn = 1;
  rc = launch<kAttTile, kAttTile, A_PLANES3, 1, EPI_SCALE>(a, BH, stream);
  if (rc != TE_OK) return rc;
  // d_v[j][d] = sum_i attn[i][j] G_o[i][d], evaluated as the transposed product (m = d, n = j)
  GemmArgs c = blank();
  c.A = Mat{P, H * nd, nd, 1, D, BH * nd};
  c.B[0] = Mat{attn, H * nn, nn, 1, N, 0};
  c.M = D, c.N = N, c.K = N, c.zh = H;
  c.out = G_v, c.o_sb = gv_sb, c.o_sh = gv_sh, c.o_sm = 1, c.o_sn = gv_sn;
  rc = launch<kAttTile, kAttTile, A_PLANES3, 1, EPI_SCALE>(c, BH, stream);
  if (rc != TE_OK) return rc;
  rc = te_alrp::softmax_bwd_planes_launch(dA, attn, S, BH * N, N, stream);
  if (rc != TE_OK) return rc;
  // d_q[i][d] = scale sum_j d_s[i][j] k[j][d]
  GemmArgs e = blank();
  e.A = Mat{S, H * nn, nn, N, 1, BH * nn};
  e.B[0] = Mat{k, k_sb, k_sh, 1, k_sn, 0};
  e.M = N, e.N = D, e.K = N, e.zh = H;
  e.out = G_q, e.o_sb = gq_sb, e.o_sh = gq_sh, e.o_sm = gq_sn, e.o_sn = 1;
  e.scale = scale;
  rc = launch<kAttTile, kAttTile, A_PLANES3, 1, EPI_SCALE>(e, BH, stream);
  if (rc != TE_OK) return rc;
  // d_k[j][d] = scale sum_i d_s[i][j] q[i][d]
  GemmArgs f = blank();
  f.A = Mat{S, H * nn, nn, 1, N, BH * nn};
  f.B[0] = Mat{q, q_sb, q_sh, 1, q_sn, 0};
  f.M = N, f.N = D, f.K = N, f.zh = H;
  f.out = G_k, f.o_sb = gk_sb, f.o_sh = gk_sh, f.o_sm = gk_sn, f.o_sn = 1;
  f.scale = scale;
  return launch<kAttTile, kAttTile, A_PLANES3, 1, EPI_SCALE>(f, BH, stream);
}
