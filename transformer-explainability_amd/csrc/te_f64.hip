// te_f64.hip -- the relprop rules of an fp64 model (model.double()): variant ours, alpha = 1, evaluated in double on the
// model's own fp64 tensors.  Relevance, safe_divide, per-sample sums, head mean: all fp64; nothing here reads or writes a
// narrower format.  Semantics: include/te_relprop.h, "fp64 operands".
//
//   Linear   Z-pass   Z = X+ W+^T + X- W-^T        (sign split of both operands in registers after the LDS read; per K group of
//                                                   four the + product, then the - product, into ONE accumulator: all terms >= 0)
//                     epilogue: S = sd(R, Z) -> fp64 [T, out] in the workspace
//            C-pass   C+ = S W+, C- = S W-         (W read through its transposed strides, sign split in registers, two accumulators)
//                     epilogue: out = X+ . C+ + X- . C-
//   AV       S = sd(R, Z) -> workspace; cam_attn = attn . (S v^T), cam_v = v . (attn^T S), each times out_scale
//   QK       S = sd(R, Z) -> workspace; cam_q = q . (S k), cam_k = k . (S^T q), each times out_scale
//
// One GEMM loop (gemm64_kernel) on v_mfma_f64_16x16x4_f64: C[m][n] = sum_k A[m][k] B[n][k] over a batch z = (b, h), every
// operand a double view with arbitrary strides (row stride sr, k stride sk), edges zero-filled, any M, N, K >= 1.  Tile
// 64 x 64 x 16 in LDS, four waves of 32 x 32 (2 x 2 fragments).  Fragments: A / B one double per lane, [row = lane & 15]
// [k = lane >> 4]; C / D col = lane & 15, row = (lane >> 4) + 4 reg -- NOT the row map of the f32 16x16x4 form.  Every output's
// k-order is the plain k loop in groups of four, independent of grid, tile position and number of rows: a batch equals its
// samples bit for bit.
//
// The streaming rules (Add ours, Clone, IndexSelect, gradient x relevance head mean) are plain fp64 kernels; Add's three
// per-sample sums are accumulated in fp64 in an order fixed by the element index inside the sample alone.
#include "te_common.h"

namespace {

constexpr int kBM = 64, kBN = 64, kBK = 16, kLd64 = kBK + 1, kThreads64 = 256;
constexpr int kPer = kBM * kBK / kThreads64;      // doubles of one operand tile a thread stages

struct Mat64 {      // double [rows x K] of batch z: element (r, k) at p + (z / zh) sb + (z % zh) sh + r sr + k sk
  const double* p;
  int64_t sb, sh, sr, sk;
};

enum { G_GATE = 0, G_LIN_Z = 1, G_LIN_C = 2 };

struct Gemm64 {
  Mat64 A, B;
  int64_t M, N, K, zh, tiles_m;
  double* out;                        // element (z, m, n)
  int64_t o_sb, o_sh, o_sm, o_sn;
  const double* g;                    // G_GATE: the multiplier; G_LIN_Z: R; G_LIN_C: X -- at (z, m, n)
  int64_t g_sb, g_sh, g_sm, g_sn;
  double scale;                       // G_GATE
};

__device__ __forceinline__ double pos64(double v) { return v > 0.0 ? v : 0.0; }
__device__ __forceinline__ double neg64(double v) { return v < 0.0 ? v : 0.0; }

// One 64 x 16 tile of a double view, global -> registers (issued one K step ahead) -> LDS; zero outside [rows) x [K).
// k-contiguous views: 16 lanes along k; row-contiguous views (sr == 1, sk != 1): 64 lanes along the rows.
__device__ __forceinline__ void fetch64(double (&v)[kPer], const double* base, int64_t sr, int64_t sk, int64_t rows,
                                        int64_t K, int64_t r0, int64_t k0) {
  const bool tr = sr == 1 && sk != 1;
#pragma unroll
  for (int c = 0; c < kPer; ++c) {
    const int idx = threadIdx.x + c * kThreads64;
    const int r = tr ? (idx & (kBM - 1)) : (idx / kBK), k = tr ? (idx / kBM) : (idx & (kBK - 1));
    const int64_t gr = r0 + r, gk = k0 + k;
    v[c] = (gr < rows && gk < K) ? base[gr * sr + gk * sk] : 0.0;
  }
}

__device__ __forceinline__ void store64(const double (&v)[kPer], int64_t sr, int64_t sk, double (*lds)[kLd64]) {
  const bool tr = sr == 1 && sk != 1;
#pragma unroll
  for (int c = 0; c < kPer; ++c) {
    const int idx = threadIdx.x + c * kThreads64;
    const int r = tr ? (idx & (kBM - 1)) : (idx / kBK), k = tr ? (idx / kBM) : (idx & (kBK - 1));
    lds[r][k] = v[c];
  }
}

template <int MODE>
__global__ __launch_bounds__(kThreads64) void gemm64_kernel(Gemm64 g) {
  constexpr int NACC = MODE == G_LIN_C ? 2 : 1;
  __shared__ double sA[kBM][kLd64];
  __shared__ double sB[kBN][kLd64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int fr = lane & 15, fk = lane >> 4;
  const int64_t z = blockIdx.x / g.tiles_m;
  const int64_t m0 = (blockIdx.x - z * g.tiles_m) * kBM, n0 = (int64_t)blockIdx.y * kBN;
  const int64_t zb = z / g.zh, zi = z - zb * g.zh;
  const double* pa = g.A.p + zb * g.A.sb + zi * g.A.sh;
  const double* pb = g.B.p + zb * g.B.sb + zi * g.B.sh;

  f64x4 acc[NACC][2][2];
#pragma unroll
  for (int s = 0; s < NACC; ++s)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[s][i][j] = f64x4{0.0, 0.0, 0.0, 0.0};

  double ra[kPer], rb[kPer];
  fetch64(ra, pa, g.A.sr, g.A.sk, g.M, g.K, m0, 0);
  fetch64(rb, pb, g.B.sr, g.B.sk, g.N, g.K, n0, 0);
  for (int64_t k0 = 0; k0 < g.K; k0 += kBK) {
    store64(ra, g.A.sr, g.A.sk, sA);
    store64(rb, g.B.sr, g.B.sk, sB);
    __syncthreads();
    if (k0 + kBK < g.K) {
      fetch64(ra, pa, g.A.sr, g.A.sk, g.M, g.K, m0, k0 + kBK);
      fetch64(rb, pb, g.B.sr, g.B.sk, g.N, g.K, n0, k0 + kBK);
    }
#pragma unroll
    for (int kk = 0; kk < kBK; kk += 4) {
      double a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i] = sA[wm + i * 16 + fr][kk + fk];
        b[i] = sB[wn + i * 16 + fr][kk + fk];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if constexpr (MODE == G_GATE) {
            acc[0][i][j] = TE_MFMA64(a[i], b[j], acc[0][i][j]);
          } else if constexpr (MODE == G_LIN_Z) {
            acc[0][i][j] = TE_MFMA64(pos64(a[i]), pos64(b[j]), acc[0][i][j]);
            acc[0][i][j] = TE_MFMA64(neg64(a[i]), neg64(b[j]), acc[0][i][j]);
          } else {
            acc[0][i][j] = TE_MFMA64(a[i], pos64(b[j]), acc[0][i][j]);
            acc[1][i][j] = TE_MFMA64(a[i], neg64(b[j]), acc[1][i][j]);
          }
        }
    }
    __syncthreads();
  }

  const double* pg = g.g + zb * g.g_sb + zi * g.g_sh;
  double* po = g.out + zb * g.o_sb + zi * g.o_sh;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t m = m0 + wm + i * 16 + fk + 4 * e, n = n0 + wn + j * 16 + fr;
        if (m < g.M && n < g.N) {
          const double gv = pg[m * g.g_sm + n * g.g_sn];
          double r;
          if constexpr (MODE == G_GATE) {
            r = (gv * acc[0][i][j][e]) * g.scale;
          } else if constexpr (MODE == G_LIN_Z) {
            r = te_sd(gv, acc[0][i][j][e]);
          } else {
            r = pos64(gv) * acc[0][i][j][e] + neg64(gv) * acc[1][i][j][e];
          }
          po[m * g.o_sm + n * g.o_sn] = r;
        }
      }
}

template <int MODE>
int launch_gemm64(Gemm64 g, int64_t Z, hipStream_t stream) {
  g.tiles_m = te_ceil_div(g.M, kBM);
  const int64_t gx = Z * g.tiles_m, gy = te_ceil_div(g.N, kBN);
  if (gx > 0x7fffffffLL || gy > 65535) return TE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(gemm64_kernel<MODE>, dim3((unsigned)gx, (unsigned)gy), dim3(kThreads64), 0, stream, g);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

// S[b][h][n][d] (contiguous) = sd(R, Z), both [B,H,N,D] views with a contiguous last dim
__global__ __launch_bounds__(256) void sd64_kernel(const double* __restrict__ R, Strided rs, const double* __restrict__ Zp,
                                                   Strided zs, double* __restrict__ S, int64_t H, int64_t N, int64_t D,
                                                   int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int64_t d = e % D, t = e / D, n = t % N, u = t / N, h = u % H, b = u / H;
  S[e] = te_sd(R[rs.at(b, h, n) + d], Zp[zs.at(b, h, n) + d]);
}

// ------------------------------------------------------------------------------------------------ Add (ours)
constexpr int kAddThreads = 256, kAddPer = 8, kAddChunk = kAddThreads * kAddPer;

struct Add64 {
  const double *R, *X0, *X1;
  int64_t n, x1_bs, x1_mod;           // X1 element of (b, e): X1[b x1_bs + e % x1_mod]  (x1_mod = n, or N for the mask form)
};

__device__ __forceinline__ void add_terms(const Add64& a, int64_t b, int64_t e, double& r, double& av, double& bv) {
  r = a.R[b * a.n + e];
  const double x0 = a.X0[b * a.n + e], x1 = a.X1[b * a.x1_bs + e % a.x1_mod];
  const double s = te_sd(r, x0 + x1);
  av = x0 * s;
  bv = x1 * s;
}

// part[b][blk][3] = sums of a, b, R over elements [blk kAddChunk, (blk + 1) kAddChunk) of sample b: each thread adds its
// kAddPer elements in index order, then the fixed tree of te_block_sum3
__global__ __launch_bounds__(kAddThreads) void add64_partial_kernel(Add64 a, double* __restrict__ part) {
  __shared__ double smem[3 * (kAddThreads / 64)];
  const int64_t b = blockIdx.y, base = (int64_t)blockIdx.x * kAddChunk;
  double sa = 0.0, sb = 0.0, sr = 0.0;
#pragma unroll
  for (int i = 0; i < kAddPer; ++i) {
    const int64_t e = base + threadIdx.x + (int64_t)i * kAddThreads;
    if (e < a.n) {
      double r, av, bv;
      add_terms(a, b, e, r, av, bv);
      sa += av;
      sb += bv;
      sr += r;
    }
  }
  te_block_sum3(sa, sb, sr, smem);
  if (threadIdx.x == 0) {
    double* p = part + (b * gridDim.x + blockIdx.x) * 3;
    p[0] = sa;
    p[1] = sb;
    p[2] = sr;
  }
}

// mask form: cols[b][j] = sum over the H N rows of S[b][row][j], rows added in index order inside each of four row classes
// (row % 4), the four classes in order
__global__ __launch_bounds__(256) void add64_colsum_kernel(Add64 a, int64_t rows, int64_t N, double* __restrict__ cols) {
  __shared__ double sm[4][64];
  const int64_t b = blockIdx.y, j = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
  const int rg = threadIdx.x >> 6;
  double s = 0.0;
  if (j < N) {
    const double x1 = a.X1[b * a.x1_bs + j];
    for (int64_t r = rg; r < rows; r += 4) {
      const int64_t e = b * a.n + r * N + j;
      s += te_sd(a.R[e], a.X0[e] + x1);
    }
  }
  sm[rg][threadIdx.x & 63] = s;
  __syncthreads();
  if (rg == 0 && j < N) cols[b * N + j] = ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
}

// one workgroup per sample: the three sums from the partials (in block order), the two factors of layers_ours.py:113-118
// into fac[b][2]; mask form: b = mask . cols, its sum, and out1 = b fac[1]
__global__ __launch_bounds__(256) void add64_finish_kernel(Add64 a, const double* __restrict__ part, int64_t nblk,
                                                           const double* __restrict__ cols, int64_t N,
                                                           double* __restrict__ fac, double* __restrict__ out1) {
  __shared__ double smem[3 * 4];
  __shared__ double fb_s;
  const int64_t b = blockIdx.x;
  double bm = 0.0, u0 = 0.0, u1 = 0.0;
  if (cols != nullptr)
    for (int64_t j = threadIdx.x; j < N; j += 256) bm += a.X1[b * a.x1_bs + j] * cols[b * N + j];
  te_block_sum3(bm, u0, u1, smem);
  if (threadIdx.x == 0) {
    double sa = 0.0, sb = 0.0, sr = 0.0;
    for (int64_t i = 0; i < nblk; ++i) {
      const double* p = part + (b * nblk + i) * 3;
      sa += p[0];
      sb += p[1];
      sr += p[2];
    }
    if (cols != nullptr) sb = bm;
    const double den = fabs(sa) + fabs(sb);
    const double a_fact = te_sd(fabs(sa), den) * sr, b_fact = te_sd(fabs(sb), den) * sr;
    const double fa = te_sd(a_fact, sa), fb = te_sd(b_fact, sb);
    fac[b * 2 + 0] = fa;
    fac[b * 2 + 1] = fb;
    fb_s = fb;
  }
  if (cols != nullptr) {
    __syncthreads();
    const double fb = fb_s;
    for (int64_t j = threadIdx.x; j < N; j += 256) out1[b * N + j] = (a.X1[b * a.x1_bs + j] * cols[b * N + j]) * fb;
  }
}

template <bool MASK>
__global__ __launch_bounds__(kAddThreads) void add64_apply_kernel(Add64 a, const double* __restrict__ fac,
                                                                  double* __restrict__ out0, double* __restrict__ out1) {
  const int64_t b = blockIdx.y, base = (int64_t)blockIdx.x * kAddChunk;
  const double fa = fac[b * 2 + 0], fb = fac[b * 2 + 1];
#pragma unroll
  for (int i = 0; i < kAddPer; ++i) {
    const int64_t e = base + threadIdx.x + (int64_t)i * kAddThreads;
    if (e < a.n) {
      double r, av, bv;
      add_terms(a, b, e, r, av, bv);
      out0[b * a.n + e] = av * fa;
      if constexpr (!MASK) out1[b * a.n + e] = bv * fb;
    }
  }
}

struct AddWs {
  int64_t nblk;
  size_t fac_at, cols_at, bytes;      // offsets in doubles: part at 0, fac, cols
};

AddWs add_ws(int64_t B, int64_t n, int64_t N) {
  AddWs w;
  w.nblk = te_ceil_div(n, kAddChunk);
  w.fac_at = (size_t)(B * w.nblk * 3);
  w.cols_at = w.fac_at + (size_t)(B * 2);
  w.bytes = sizeof(double) * (w.cols_at + (size_t)(B * N));
  return w;
}

int add64_launch(const Add64& a, int64_t B, int64_t H, int64_t N, bool mask, double* out0, double* out1, void* ws,
                 size_t ws_bytes, hipStream_t stream) {
  const AddWs w = add_ws(B, a.n, mask ? N : 0);
  if (ws == nullptr || ws_bytes < w.bytes) return TE_ERR_WORKSPACE;
  if (w.nblk > 0x7fffffffLL || B > 65535) return TE_ERR_UNSUPPORTED;
  double* part = static_cast<double*>(ws);
  double* fac = part + w.fac_at;
  double* cols = mask ? part + w.cols_at : nullptr;
  const dim3 grid((unsigned)w.nblk, (unsigned)B);
  hipLaunchKernelGGL(add64_partial_kernel, grid, dim3(kAddThreads), 0, stream, a, part);
  if (mask)
    hipLaunchKernelGGL(add64_colsum_kernel, dim3((unsigned)te_ceil_div(N, 64), (unsigned)B), dim3(256), 0, stream, a,
                       H * N, N, cols);
  hipLaunchKernelGGL(add64_finish_kernel, dim3((unsigned)B), dim3(256), 0, stream, a, (const double*)part, w.nblk,
                     (const double*)cols, N, fac, out1);
  if (mask)
    hipLaunchKernelGGL(add64_apply_kernel<true>, grid, dim3(kAddThreads), 0, stream, a, (const double*)fac, out0, out1);
  else
    hipLaunchKernelGGL(add64_apply_kernel<false>, grid, dim3(kAddThreads), 0, stream, a, (const double*)fac, out0, out1);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

// ------------------------------------------------------------------------------------------------ Clone, IndexSelect, head mean
__global__ __launch_bounds__(256) void clone64_kernel(const double* __restrict__ R0, const double* __restrict__ R1,
                                                      const double* __restrict__ R2, const double* __restrict__ X,
                                                      double* __restrict__ out, int64_t n) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const double x = X[e];
  double c = te_sd(R0[e], x) + te_sd(R1[e], x);
  if (R2 != nullptr) c = c + te_sd(R2[e], x);
  out[e] = x * c;
}

__global__ __launch_bounds__(256) void index_select64_kernel(const double* __restrict__ R, const double* __restrict__ X,
                                                             double* __restrict__ out, int64_t N, int64_t C, int64_t index,
                                                             int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int64_t c = e % C, t = e / C, n = t % N, b = t / N;
  const double s = (n == index) ? te_sd(R[b * C + c], X[(b * N + index) * C + c]) : 0.0;
  out[e] = X[e] * s;
}

__global__ __launch_bounds__(256) void headmean64_kernel(const double* __restrict__ grad, const double* __restrict__ cam,
                                                         double* __restrict__ out, int64_t H, int64_t nn, int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int64_t b = e / nn, i = e - b * nn;
  double s = 0.0;
  for (int64_t h = 0; h < H; ++h) {
    const int64_t at = (b * H + h) * nn + i;
    s += pos64(grad[at] * cam[at]);
  }
  out[e] = s / (double)H;
}

bool grid1d(int64_t total, unsigned& blocks) {
  const int64_t nb = te_ceil_div(total, 256);
  blocks = (unsigned)nb;
  return nb <= 0x7fffffffLL;
}

}  // namespace

// ================================================================================================ C ABI
extern "C" size_t te_linear_relprop_f64_workspace_bytes(int64_t T, int64_t in_f, int64_t out_f) {
  if (T <= 0 || in_f <= 0 || out_f <= 0) return 0;
  return sizeof(double) * (size_t)T * (size_t)out_f;
}

extern "C" int te_linear_relprop_f64(const double* R, int64_t r_ld, const double* X, int64_t x_ld, const double* W,
                                     int64_t w_ld, double* out, int64_t T, int64_t in_f, int64_t out_f, void* ws,
                                     size_t ws_bytes, te_stream_t stream) {
  if (!R || !X || !W || !out || T <= 0 || in_f <= 0 || out_f <= 0) return TE_ERR_INVALID_ARG;
  if (r_ld < out_f || w_ld < in_f || (T > 1 && x_ld < in_f)) return TE_ERR_INVALID_ARG;
  if (!ws || ws_bytes < te_linear_relprop_f64_workspace_bytes(T, in_f, out_f)) return TE_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* S = static_cast<double*>(ws);
  Gemm64 z = {};
  z.A = Mat64{X, 0, 0, x_ld, 1};
  z.B = Mat64{W, 0, 0, w_ld, 1};
  z.M = T, z.N = out_f, z.K = in_f, z.zh = 1;
  z.out = S, z.o_sm = out_f, z.o_sn = 1;
  z.g = R, z.g_sm = r_ld, z.g_sn = 1;
  int rc = launch_gemm64<G_LIN_Z>(z, 1, st);
  if (rc != TE_OK) return rc;
  Gemm64 c = {};
  c.A = Mat64{S, 0, 0, out_f, 1};
  c.B = Mat64{W, 0, 0, 1, w_ld};        // B[n][k] = W[k][n]
  c.M = T, c.N = in_f, c.K = out_f, c.zh = 1;
  c.out = out, c.o_sm = in_f, c.o_sn = 1;
  c.g = X, c.g_sm = x_ld, c.g_sn = 1;
  return launch_gemm64<G_LIN_C>(c, 1, st);
}

extern "C" size_t te_matmul_relprop_av_f64_workspace_bytes(int64_t B, int64_t H, int64_t N, int64_t D) {
  if (B <= 0 || H <= 0 || N <= 0 || D <= 0) return 0;
  return sizeof(double) * (size_t)B * (size_t)H * (size_t)N * (size_t)D;
}

extern "C" size_t te_matmul_relprop_qk_f64_workspace_bytes(int64_t B, int64_t H, int64_t N, int64_t D) {
  if (B <= 0 || H <= 0 || N <= 0 || D <= 0) return 0;
  return sizeof(double) * (size_t)B * (size_t)H * (size_t)N * (size_t)N;
}

extern "C" int te_matmul_relprop_av_f64(const double* R, int64_t r_sb, int64_t r_sh, int64_t r_sn, const double* attn,
                                        const double* v, int64_t v_sb, int64_t v_sh, int64_t v_sn, const double* Z,
                                        int64_t z_sb, int64_t z_sh, int64_t z_sn, double* cam_attn, double* cam_v,
                                        int64_t cv_sb, int64_t cv_sh, int64_t cv_sn, int64_t B, int64_t H, int64_t N,
                                        int64_t D, double out_scale, void* ws, size_t ws_bytes, te_stream_t stream) {
  if (!R || !attn || !v || !Z || !cam_attn || !cam_v || B <= 0 || H <= 0 || N <= 0 || D <= 0) return TE_ERR_INVALID_ARG;
  if (!ws || ws_bytes < te_matmul_relprop_av_f64_workspace_bytes(B, H, N, D)) return TE_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* S = static_cast<double*>(ws);
  const int64_t total = B * H * N * D;
  unsigned blocks;
  if (!grid1d(total, blocks)) return TE_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(sd64_kernel, dim3(blocks), dim3(256), 0, st, R, Strided{r_sb, r_sh, r_sn}, Z,
                     Strided{z_sb, z_sh, z_sn}, S, H, N, D, total);
  Gemm64 a = {};                        // cam_attn[i][j] = attn[i][j] sum_d S[i][d] v[j][d]
  a.A = Mat64{S, H * N * D, N * D, D, 1};
  a.B = Mat64{v, v_sb, v_sh, v_sn, 1};
  a.M = N, a.N = N, a.K = D, a.zh = H;
  a.out = cam_attn, a.o_sb = H * N * N, a.o_sh = N * N, a.o_sm = N, a.o_sn = 1;
  a.g = attn, a.g_sb = H * N * N, a.g_sh = N * N, a.g_sm = N, a.g_sn = 1;
  a.scale = out_scale;
  int rc = launch_gemm64<G_GATE>(a, B * H, st);
  if (rc != TE_OK) return rc;
  Gemm64 c = {};                        // cam_v[j][d] = v[j][d] sum_i attn[i][j] S[i][d]
  c.A = Mat64{attn, H * N * N, N * N, 1, N};
  c.B = Mat64{S, H * N * D, N * D, 1, D};
  c.M = N, c.N = D, c.K = N, c.zh = H;
  c.out = cam_v, c.o_sb = cv_sb, c.o_sh = cv_sh, c.o_sm = cv_sn, c.o_sn = 1;
  c.g = v, c.g_sb = v_sb, c.g_sh = v_sh, c.g_sm = v_sn, c.g_sn = 1;
  c.scale = out_scale;
  return launch_gemm64<G_GATE>(c, B * H, st);
}

extern "C" int te_matmul_relprop_qk_f64(const double* R, const double* q, int64_t q_sb, int64_t q_sh, int64_t q_sn,
                                        const double* k, int64_t k_sb, int64_t k_sh, int64_t k_sn, const double* Z,
                                        double* cam_q, int64_t cq_sb, int64_t cq_sh, int64_t cq_sn, double* cam_k,
                                        int64_t ck_sb, int64_t ck_sh, int64_t ck_sn, int64_t B, int64_t H, int64_t N,
                                        int64_t D, double out_scale, void* ws, size_t ws_bytes, te_stream_t stream) {
  if (!R || !q || !k || !Z || !cam_q || !cam_k || B <= 0 || H <= 0 || N <= 0 || D <= 0) return TE_ERR_INVALID_ARG;
  if (!ws || ws_bytes < te_matmul_relprop_qk_f64_workspace_bytes(B, H, N, D)) return TE_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* S = static_cast<double*>(ws);
  const int64_t total = B * H * N * N;
  unsigned blocks;
  if (!grid1d(total, blocks)) return TE_ERR_UNSUPPORTED;
  const Strided nn{H * N * N, N * N, N};
  hipLaunchKernelGGL(sd64_kernel, dim3(blocks), dim3(256), 0, st, R, nn, Z, nn, S, H, N, N, total);
  Gemm64 a = {};                        // cam_q[i][d] = q[i][d] sum_j S[i][j] k[j][d]
  a.A = Mat64{S, nn.sb, nn.sh, N, 1};
  a.B = Mat64{k, k_sb, k_sh, 1, k_sn};
  a.M = N, a.N = D, a.K = N, a.zh = H;
  a.out = cam_q, a.o_sb = cq_sb, a.o_sh = cq_sh, a.o_sm = cq_sn, a.o_sn = 1;
  a.g = q, a.g_sb = q_sb, a.g_sh = q_sh, a.g_sm = q_sn, a.g_sn = 1;
  a.scale = out_scale;
  int rc = launch_gemm64<G_GATE>(a, B * H, st);
  if (rc != TE_OK) return rc;
  Gemm64 c = {};                        // cam_k[j][d] = k[j][d] sum_i S[i][j] q[i][d]
  c.A = Mat64{S, nn.sb, nn.sh, 1, N};
  c.B = Mat64{q, q_sb, q_sh, 1, q_sn};
  c.M = N, c.N = D, c.K = N, c.zh = H;
  c.out = cam_k, c.o_sb = ck_sb, c.o_sh = ck_sh, c.o_sm = ck_sn, c.o_sn = 1;
  c.g = k, c.g_sb = k_sb, c.g_sh = k_sh, c.g_sm = k_sn, c.g_sn = 1;
  c.scale = out_scale;
  return launch_gemm64<G_GATE>(c, B * H, st);
}

extern "C" size_t te_add_relprop_f64_workspace_bytes(int64_t B, int64_t n) {
  if (B <= 0 || n <= 0) return 0;
  return add_ws(B, n, 0).bytes;
}

extern "C" int te_add_relprop_f64(const double* R, const double* X0, const double* X1, double* out0, double* out1,
                                  int64_t B, int64_t n, int64_t x1_batch_stride, void* ws, size_t ws_bytes,
                                  te_stream_t stream) {
  if (!R || !X0 || !X1 || !out0 || !out1 || B <= 0 || n <= 0 || (x1_batch_stride != 0 && x1_batch_stride < n))
    return TE_ERR_INVALID_ARG;
  const Add64 a{R, X0, X1, n, x1_batch_stride, n};
  return add64_launch(a, B, 0, 0, false, out0, out1, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

extern "C" size_t te_add_bcast_relprop_f64_workspace_bytes(int64_t B, int64_t H, int64_t N) {
  if (B <= 0 || H <= 0 || N <= 0) return 0;
  return add_ws(B, H * N * N, N).bytes;
}

extern "C" int te_add_bcast_relprop_f64(const double* R, const double* X0, const double* mask, int64_t mask_batch_stride,
                                        double* out0, double* out1, int64_t B, int64_t H, int64_t N, void* ws,
                                        size_t ws_bytes, te_stream_t stream) {
  if (!R || !X0 || !mask || !out0 || !out1 || B <= 0 || H <= 0 || N <= 0 ||
      (mask_batch_stride != 0 && mask_batch_stride < N))
    return TE_ERR_INVALID_ARG;
  const Add64 a{R, X0, mask, H * N * N, mask_batch_stride, N};
  return add64_launch(a, B, H, N, true, out0, out1, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int te_clone_relprop_f64(const double* R0, const double* R1, const double* R2, const double* X, double* out,
                                    int64_t n, te_stream_t stream) {
  unsigned blocks;
  if (!R0 || !R1 || !X || !out || n <= 0 || !grid1d(n, blocks)) return TE_ERR_INVALID_ARG;
  hipLaunchKernelGGL(clone64_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), R0, R1, R2, X, out, n);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

extern "C" int te_index_select_relprop_f64(const double* R, const double* X, double* out, int64_t B, int64_t N, int64_t C,
                                           int64_t index, te_stream_t stream) {
  unsigned blocks;
  if (!R || !X || !out || B <= 0 || N <= 0 || C <= 0 || index < 0 || index >= N || !grid1d(B * N * C, blocks))
    return TE_ERR_INVALID_ARG;
  hipLaunchKernelGGL(index_select64_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), R, X, out, N, C,
                     index, B * N * C);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

extern "C" int te_gradcam_headmean_f64(const double* grad, const double* cam, double* out, int64_t B, int64_t H, int64_t N,
                                       te_stream_t stream) {
  unsigned blocks;
  if (!grad || !cam || !out || B <= 0 || H <= 0 || N <= 0 || !grid1d(B * N * N, blocks)) return TE_ERR_INVALID_ARG;
  hipLaunchKernelGGL(headmean64_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), grad, cam, out, H,
                     N * N, B * N * N);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}
