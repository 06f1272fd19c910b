// te_elementwise.hip -- HBM-bound relprop rules for gfx950: Add (ours / lrp / broadcast mask), Clone,
// IndexSelect, gradient x relevance head-mean.  All kernels stream 16 B per lane where alignment
// allows, reduce per SAMPLE (batch = independent batch-1 problems) with fp64 accumulators in a fixed
// order (bit-reproducible, no atomics), and evaluate safe_divide exactly like the reference.
//
// Build flags matter: -ffp-contract=off (the reference rounds every product and sum separately).
#include <stdlib.h>

#include "te_common.h"

namespace {

constexpr int kThreads = 256;

// (te_common.h: f32x4_u, the 16-byte access that only promises 4-byte alignment -- used where per-(b,h) bases are odd multiples of 4 B)

template <typename V>
__device__ __forceinline__ V ld(const float* p) { return *reinterpret_cast<const V*>(p); }
template <typename V>
__device__ __forceinline__ void st(float* p, V v) { *reinterpret_cast<V*>(p) = v; }

// Operand (activation) loads, templated on the operand type TX: fp32 exactly as before, or bf16 (te_bf16_t) widened
// exactly to fp32 -- a bf16 model's rules read its own bf16 tensors; relevance, sums and outputs stay fp32.
__device__ __forceinline__ float ldx(const float* p) { return *p; }
__device__ __forceinline__ float ldx(const te_bf16_t* p) { return __uint_as_float((unsigned)*p << 16); }
template <typename V>
__device__ __forceinline__ V ldx4(const float* p) { return ld<V>(p); }
template <typename V>
__device__ __forceinline__ V ldx4(const te_bf16_t* p) { return V{ldx(p), ldx(p + 1), ldx(p + 2), ldx(p + 3)}; }
// host: the vector path needs 16-byte fp32 operands; bf16 operands are read element by element
static inline bool vec_aligned(const float* p) { return te_aligned16(p); }
static inline bool vec_aligned(const te_bf16_t*) { return true; }

// ------------------------------------------------------------------------------------------------
// Add.relprop (modules/layers_ours.py:97-120).  Pass 1: per-(sample, chunk) partial sums.
// ------------------------------------------------------------------------------------------------
template <int VEC, typename TX>
__global__ __launch_bounds__(kThreads) void add_sums_kernel(
    const float* __restrict__ R, const TX* __restrict__ X0, const TX* __restrict__ X1,
    double* __restrict__ partial, int64_t n, int64_t x1_bs, int64_t chunk) {
  __shared__ double smem[3 * (kThreads / 64)];
  const int64_t b = blockIdx.y;
  const int64_t start = (int64_t)blockIdx.x * chunk;
  const int64_t end = min(n, start + chunk);
  const float* r = R + b * n;
  const TX* x0 = X0 + b * n;
  const TX* x1 = X1 + b * x1_bs;
  double sa = 0.0, sb = 0.0, sr = 0.0;
  for (int64_t i = start + (int64_t)threadIdx.x * VEC; i < end; i += (int64_t)kThreads * VEC) {
    if constexpr (VEC == 4) {
      const f32x4 rv = ld<f32x4>(r + i), av = ldx4<f32x4>(x0 + i), bv = ldx4<f32x4>(x1 + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float s = te_sd(rv[e], av[e] + bv[e]);
        sa += (double)(av[e] * s);
        sb += (double)(bv[e] * s);
        sr += (double)rv[e];
      }
    } else {
      const float rv = r[i], av = ldx(x0 + i), bv = ldx(x1 + i);
      const float s = te_sd(rv, av + bv);
      sa += (double)(av * s);
      sb += (double)(bv * s);
      sr += (double)rv;
    }
  }
  te_block_sum3(sa, sb, sr, smem);
  if (threadIdx.x == 0) {
    double* p = partial + (b * gridDim.x + blockIdx.x) * 3;
    p[0] = sa;
    p[1] = sb;
    p[2] = sr;
  }
}

// Deferred form (te_add_relprop_deferred_f32): the same pass also stores the UNSCALED a = X0.S and b = X1.S; the
// per-sample factors are applied by whoever reads them next (Clone / the Linear Z-pass epilogue multiply R by the
// sample's factor -- the identical fp32 product the apply pass would have stored), so Add.relprop moves its
// algorithmic 5 n floats per sample exactly once.
template <int VEC, typename TX>
__global__ __launch_bounds__(kThreads) void add_deferred_kernel(
    const float* __restrict__ R, const TX* __restrict__ X0, const TX* __restrict__ X1,
    float* __restrict__ a_out, float* __restrict__ b_out, double* __restrict__ partial, int64_t n, int64_t x1_bs,
    int64_t chunk) {
  __shared__ double smem[3 * (kThreads / 64)];
  const int64_t b = blockIdx.y;
  const int64_t start = (int64_t)blockIdx.x * chunk;
  const int64_t end = min(n, start + chunk);
  const float* r = R + b * n;
  const TX* x0 = X0 + b * n;
  const TX* x1 = X1 + b * x1_bs;
  float* o0 = a_out + b * n;
  float* o1 = b_out + b * n;
  double sa = 0.0, sb = 0.0, sr = 0.0;
  for (int64_t i = start + (int64_t)threadIdx.x * VEC; i < end; i += (int64_t)kThreads * VEC) {
    if constexpr (VEC == 4) {
      const f32x4 rv = ld<f32x4>(r + i), av = ldx4<f32x4>(x0 + i), bv = ldx4<f32x4>(x1 + i);
      f32x4 oa, ob;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float s = te_sd(rv[e], av[e] + bv[e]);
        oa[e] = av[e] * s;
        ob[e] = bv[e] * s;
        sa += (double)oa[e];
        sb += (double)ob[e];
        sr += (double)rv[e];
      }
      st<f32x4>(o0 + i, oa);
      st<f32x4>(o1 + i, ob);
    } else {
      const float rv = r[i], av = ldx(x0 + i), bv = ldx(x1 + i);
      const float s = te_sd(rv, av + bv);
      const float a = av * s, bb = bv * s;
      o0[i] = a;
      o1[i] = bb;
      sa += (double)a;
      sb += (double)bb;
      sr += (double)rv;
    }
  }
  te_block_sum3(sa, sb, sr, smem);
  if (threadIdx.x == 0) {
    double* p = partial + (b * gridDim.x + blockIdx.x) * 3;
    p[0] = sa;
    p[1] = sb;
    p[2] = sr;
  }
}

// The scalar tail of Add.relprop: a_fact / b_fact and the two rescale factors, in fp32 like the
// reference's 0-d tensors (layers_ours.py:112-116).
__device__ __forceinline__ void add_factors(double A, double Bs, double Rs, float& fa, float& fb) {
  const float a_sum = (float)A, b_sum = (float)Bs, r_sum = (float)Rs;
  const float a_abs = fabsf(a_sum), b_abs = fabsf(b_sum);
  const float den = a_abs + b_abs;
  const float a_fact = te_sd(a_abs, den) * r_sum;
  const float b_fact = te_sd(b_abs, den) * r_sum;
  fa = te_sd(a_fact, a_sum);
  fb = te_sd(b_fact, b_sum);
}

// One wave folds the chunk partials of sample b in a fixed tree (the order every user of the partials shares).
__device__ __forceinline__ void fold_partials(const double* __restrict__ partial, int64_t b, int nb, double& sa,
                                              double& sb, double& sr) {
  sa = sb = sr = 0.0;
  for (int p = threadIdx.x; p < nb; p += 64) {
    const double* q = partial + (b * nb + p) * 3;
    sa += q[0];
    sb += q[1];
    sr += q[2];
  }
  sa = te_wave_sum(sa);
  sb = te_wave_sum(sb);
  sr = te_wave_sum(sr);
}

// fac[b] = {fa, fb} from the chunk partials: one wave per sample
__global__ __launch_bounds__(64) void add_factors_kernel(const double* __restrict__ partial, float* __restrict__ fac,
                                                         int nb) {
  const int64_t b = blockIdx.x;
  double sa, sb, sr;
  fold_partials(partial, b, nb, sa, sb, sr);
  if (threadIdx.x == 0) {
    float fa, fb;
    add_factors(sa, sb, sr, fa, fb);
    fac[2 * b] = fa;
    fac[2 * b + 1] = fb;
  }
}

// Pass 2 (ours) / the only pass (lrp): recompute a, b and apply the per-sample factors.
template <int VEC, bool OURS, typename TX>
__global__ __launch_bounds__(kThreads) void add_apply_kernel(
    const float* __restrict__ R, const TX* __restrict__ X0, const TX* __restrict__ X1,
    float* __restrict__ out0, float* __restrict__ out1, const double* __restrict__ partial,
    int64_t n, int64_t x1_bs, int64_t chunk) {
  __shared__ float fac[2];
  const int64_t b = blockIdx.y;
  float fa = 1.0f, fb = 1.0f;
  if constexpr (OURS) {
    if (threadIdx.x < 64) {  // one wave folds the chunk partials of this sample in a fixed tree
      double sa, sb, sr;
      fold_partials(partial, b, gridDim.x, sa, sb, sr);
      if (threadIdx.x == 0) {
        add_factors(sa, sb, sr, fa, fb);
        fac[0] = fa;
        fac[1] = fb;
      }
    }
    __syncthreads();
    fa = fac[0];
    fb = fac[1];
  }
  const int64_t start = (int64_t)blockIdx.x * chunk;
  const int64_t end = min(n, start + chunk);
  const float* r = R + b * n;
  const TX* x0 = X0 + b * n;
  const TX* x1 = X1 + b * x1_bs;
  float* o0 = out0 + b * n;
  float* o1 = out1 + b * n;
  for (int64_t i = start + (int64_t)threadIdx.x * VEC; i < end; i += (int64_t)kThreads * VEC) {
    if constexpr (VEC == 4) {
      const f32x4 rv = ld<f32x4>(r + i), av = ldx4<f32x4>(x0 + i), bv = ldx4<f32x4>(x1 + i);
      f32x4 oa, ob;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float s = te_sd(rv[e], av[e] + bv[e]);
        float a = av[e] * s, bb = bv[e] * s;
        if constexpr (OURS) {
          a = a * fa;
          bb = bb * fb;
        }
        oa[e] = a;
        ob[e] = bb;
      }
      st<f32x4>(o0 + i, oa);
      st<f32x4>(o1 + i, ob);
    } else {
      const float rv = r[i], av = ldx(x0 + i), bv = ldx(x1 + i);
      const float s = te_sd(rv, av + bv);
      float a = av * s, bb = bv * s;
      if constexpr (OURS) {
        a = a * fa;
        bb = bb * fb;
      }
      o0[i] = a;
      o1[i] = bb;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Broadcast-mask Add of BERT self-attention (BERT.py:342,386-388).  Rows are the H*N (h,i) pairs of a
// sample, columns j index the key token / mask entry.  Each thread owns columns j = tid + 256*c.
// TX: the operand type of X0 and the mask (fp32, or bf16 read through ldx); R, the fp64 column / sample sums, the
// factors and the outputs are fp32 / fp64 for both, in the same order, so a bf16 call gives the fp32 call's bits on
// exact fp32 copies of its operands.
// ------------------------------------------------------------------------------------------------
constexpr int kMaxColsPerThread = 8;  // N <= 2048

// STORE: also write the unscaled a = X0 . S (deferred form: the per-sample factor goes to the consumer, the QK rule)
template <bool STORE, typename TX>
__global__ __launch_bounds__(kThreads) void addb_sums_kernel(
    const float* __restrict__ R, const TX* __restrict__ X0, const TX* __restrict__ mask,
    double* __restrict__ partial, float* __restrict__ a_out, int64_t rows, int64_t N, int64_t rows_per_block) {
  __shared__ double smem[3 * (kThreads / 64)];
  const int64_t b = blockIdx.y;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = min(rows, r0 + rows_per_block);
  const float* r = R + b * rows * N;
  const TX* x0 = X0 + b * rows * N;
  const TX* m = mask + b * N;
  double csum[kMaxColsPerThread];
  float mv[kMaxColsPerThread];
#pragma unroll
  for (int c = 0; c < kMaxColsPerThread; ++c) {
    csum[c] = 0.0;
    const int64_t j = threadIdx.x + (int64_t)c * kThreads;
    mv[c] = (j < N) ? ldx(m + j) : 0.0f;
  }
  double sa = 0.0, sr = 0.0, dummy = 0.0;
  float* ao = STORE ? a_out + b * rows * N : nullptr;
  constexpr int RU = 4;       // rows in flight per thread: 2 RU loads per column slot issued before the first use
  for (int64_t row = r0; row < r1; row += RU) {
#pragma unroll
    for (int c = 0; c < kMaxColsPerThread; ++c) {
      const int64_t j = threadIdx.x + (int64_t)c * kThreads;
      if (j < N) {
        float rv[RU], av[RU];
#pragma unroll
        for (int u = 0; u < RU; ++u) {
          const bool ok = row + u < r1;
          rv[u] = ok ? r[(row + u) * N + j] : 0.0f;
          av[u] = ok ? ldx(x0 + ((row + u) * N + j)) : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < RU; ++u)
          if (row + u < r1) {
            const float s = te_sd(rv[u], av[u] + mv[c]);
            const float a = av[u] * s;
            if constexpr (STORE) ao[(row + u) * N + j] = a;
            sa += (double)a;
            sr += (double)rv[u];
            csum[c] += (double)s;
          }
      }
    }
  }
  double* p = partial + (b * gridDim.x + blockIdx.x) * (N + 2);
#pragma unroll
  for (int c = 0; c < kMaxColsPerThread; ++c) {
    const int64_t j = threadIdx.x + (int64_t)c * kThreads;
    if (j < N) p[2 + j] = csum[c];
  }
  te_block_sum3(sa, sr, dummy, smem);
  if (threadIdx.x == 0) {
    p[0] = sa;
    p[1] = sr;
  }
}

// One block per sample: fold the partials, form b_j = mask_j * C1_j, the three sums and the factors.
// fac[b] = {fa, fb}; bvec[b][j] = b_j (unscaled).
// out1 (optional): the mask's relevance b_j * fb, written here in the deferred form (addb_apply_kernel writes it else)
template <typename TX>
__global__ __launch_bounds__(kThreads) void addb_finalize_kernel(
    const double* __restrict__ partial, const TX* __restrict__ mask, float* __restrict__ fac,
    float* __restrict__ bvec, int64_t N, int nblk, int ours, float* __restrict__ out1) {
  __shared__ double smem[3 * (kThreads / 64)];
  __shared__ float fb_s;
  const int64_t b = blockIdx.x;
  const double* base = partial + b * nblk * (N + 2);
  double sb = 0.0, sa = 0.0, sr = 0.0;
  for (int64_t j = threadIdx.x; j < N; j += kThreads) {
    double c1 = 0.0;
    for (int p = 0; p < nblk; ++p) c1 += base[(int64_t)p * (N + 2) + 2 + j];
    const float bj = ldx(mask + (b * N + j)) * (float)c1;
    bvec[b * N + j] = bj;
    sb += (double)bj;
  }
  for (int p = threadIdx.x; p < nblk; p += kThreads) {
    sa += base[(int64_t)p * (N + 2) + 0];
    sr += base[(int64_t)p * (N + 2) + 1];
  }
  te_block_sum3(sa, sb, sr, smem);
  if (threadIdx.x == 0) {
    float fa = 1.0f, fb = 1.0f;
    if (ours) add_factors(sa, sb, sr, fa, fb);
    fac[b * 2 + 0] = fa;
    fac[b * 2 + 1] = fb;
    fb_s = fb;
  }
  if (out1 != nullptr) {
    __syncthreads();
    const float fb = fb_s;
    for (int64_t j = threadIdx.x; j < N; j += kThreads) out1[b * N + j] = bvec[b * N + j] * fb;
  }
}

template <typename TX>
__global__ __launch_bounds__(kThreads) void addb_apply_kernel(
    const float* __restrict__ R, const TX* __restrict__ X0, const TX* __restrict__ mask,
    const float* __restrict__ fac, const float* __restrict__ bvec, float* __restrict__ out0,
    float* __restrict__ out1, int64_t rows, int64_t N, int64_t rows_per_block) {
  const int64_t b = blockIdx.y;
  const float fa = fac[b * 2 + 0], fb = fac[b * 2 + 1];
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = min(rows, r0 + rows_per_block);
  const float* r = R + b * rows * N;
  const TX* x0 = X0 + b * rows * N;
  const TX* m = mask + b * N;
  float* o0 = out0 + b * rows * N;
  if (out1 != nullptr && blockIdx.x == 0) {
    for (int64_t j = threadIdx.x; j < N; j += kThreads) out1[b * N + j] = bvec[b * N + j] * fb;
  }
  float mv[kMaxColsPerThread];
#pragma unroll
  for (int c = 0; c < kMaxColsPerThread; ++c) {
    const int64_t j = threadIdx.x + (int64_t)c * kThreads;
    mv[c] = (j < N) ? ldx(m + j) : 0.0f;
  }
  for (int64_t row = r0; row < r1; ++row) {
#pragma unroll
    for (int c = 0; c < kMaxColsPerThread; ++c) {
      const int64_t j = threadIdx.x + (int64_t)c * kThreads;
      if (j < N) {
        const float rv = r[row * N + j], av = ldx(x0 + (row * N + j));
        const float s = te_sd(rv, av + mv[c]);
        o0[row * N + j] = (av * s) * fa;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Clone.relprop (modules/layers_ours.py:151-169): out = X * (sd(R0,X) + sd(R1,X) [+ sd(R2,X)])
// ------------------------------------------------------------------------------------------------
template <int VEC, int NUM, typename TX>
__global__ __launch_bounds__(kThreads) void clone_kernel(
    const float* __restrict__ R0, const float* __restrict__ R1, const float* __restrict__ R2,
    const TX* __restrict__ X, float* __restrict__ out, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * kThreads * VEC;
  for (int64_t i = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * VEC; i < n; i += stride) {
    if constexpr (VEC == 4) {
      const f32x4 x = ldx4<f32x4>(X + i), a = ld<f32x4>(R0 + i), b = ld<f32x4>(R1 + i);
      f32x4 c = {0.f, 0.f, 0.f, 0.f};
      if constexpr (NUM == 3) c = ld<f32x4>(R2 + i);
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float s = te_sd(a[e], x[e]) + te_sd(b[e], x[e]);
        if constexpr (NUM == 3) s = s + te_sd(c[e], x[e]);
        o[e] = x[e] * s;
      }
      st<f32x4>(out + i, o);
    } else {
      const float x = ldx(X + i);
      float s = te_sd(R0[i], x) + te_sd(R1[i], x);
      if constexpr (NUM == 3) s = s + te_sd(R2[i], x);
      out[i] = x * s;
    }
  }
}

// Clone.relprop whose relevance operands carry a deferred per-sample factor (the unscaled outputs of
// te_add_relprop_deferred_f32): R_i enters as R_i[e] * s_i[sample]; s_i == NULL means 1.  2-D grid (chunks, samples).
template <int VEC, int NUM, typename TX>
__global__ __launch_bounds__(kThreads) void clone_scaled_kernel(
    const float* __restrict__ R0, const float* __restrict__ s0, int64_t s0_stride, const float* __restrict__ R1,
    const float* __restrict__ s1, int64_t s1_stride, const float* __restrict__ R2, const float* __restrict__ s2,
    int64_t s2_stride, const TX* __restrict__ X, float* __restrict__ out, int64_t n) {
  const int64_t b = blockIdx.y;
  const float f0 = s0 ? s0[b * s0_stride] : 1.0f, f1 = s1 ? s1[b * s1_stride] : 1.0f;
  const float f2 = (NUM == 3 && s2) ? s2[b * s2_stride] : 1.0f;
  const float* r0 = R0 + b * n;
  const float* r1 = R1 + b * n;
  const float* r2 = (NUM == 3) ? R2 + b * n : nullptr;
  const TX* x_ = X + b * n;
  float* o = out + b * n;
  const int64_t stride = (int64_t)gridDim.x * kThreads * VEC;
  for (int64_t i = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * VEC; i < n; i += stride) {
    if constexpr (VEC == 4) {
      const f32x4 x = ldx4<f32x4>(x_ + i), a = ld<f32x4>(r0 + i), bq = ld<f32x4>(r1 + i);
      f32x4 c = {0.f, 0.f, 0.f, 0.f};
      if constexpr (NUM == 3) c = ld<f32x4>(r2 + i);
      f32x4 ov;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float ra = s0 ? a[e] * f0 : a[e], rb = s1 ? bq[e] * f1 : bq[e];
        float s = te_sd(ra, x[e]) + te_sd(rb, x[e]);
        if constexpr (NUM == 3) s = s + te_sd(s2 ? c[e] * f2 : c[e], x[e]);
        ov[e] = x[e] * s;
      }
      st<f32x4>(o + i, ov);
    } else {
      const float x = ldx(x_ + i);
      float s = te_sd(s0 ? r0[i] * f0 : r0[i], x) + te_sd(s1 ? r1[i] * f1 : r1[i], x);
      if constexpr (NUM == 3) s = s + te_sd(s2 ? r2[i] * f2 : r2[i], x);
      o[i] = x * s;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// IndexSelect.relprop (modules/layers_ours.py:129-147), dim = 1, single index.
// ------------------------------------------------------------------------------------------------
template <typename TX>
__global__ __launch_bounds__(kThreads) void index_select_kernel(
    const float* __restrict__ R, const TX* __restrict__ X, float* __restrict__ out,
    int64_t B, int64_t N, int64_t C, int64_t index) {
  const int64_t total = B * N * C;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += stride) {
    const int64_t c = i % C;
    const int64_t nrow = (i / C) % N;
    const int64_t b = i / (C * N);
    float v = 0.0f;
    if (nrow == index) {
      const float x = ldx(X + i);
      v = x * te_sd(R[b * C + c], x);
    }
    out[i] = v;
  }
}

// ------------------------------------------------------------------------------------------------
// Tail a10: out[b,e] = (sum_h max(grad[b,h,e] * cam[b,h,e], 0)) / H over e in [0, N*N)
// (ViT_LRP.py:359-366; ExplanationGenerator.py:49-56).  torch's mean sums heads in order then divides.
// Per-(b,h) bases are (b*H+h)*N*N elements: only dword-aligned when N*N is odd, hence f32x4_u.
// ------------------------------------------------------------------------------------------------
template <int VEC, typename TG>
__global__ __launch_bounds__(kThreads) void headmean_kernel(
    const TG* __restrict__ grad, const float* __restrict__ cam, float* __restrict__ out,
    int64_t H, int64_t NN) {
  const int64_t b = blockIdx.y;
  const float fH = (float)H;
  const TG* g = grad + b * H * NN;
  const float* c = cam + b * H * NN;
  float* o = out + b * NN;
  const int64_t stride = (int64_t)gridDim.x * kThreads * VEC;
  for (int64_t e = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * VEC; e < NN; e += stride) {
    if (VEC == 4 && e + 3 < NN) {
      f32x4_u acc = {0.f, 0.f, 0.f, 0.f};
      int64_t h = 0;
      // four heads = eight independent 16-B loads in flight per thread (H is a run-time value: the plain loop
      // waits for each pair before issuing the next); the heads are still added in index order
      for (; h + 4 <= H; h += 4) {
        f32x4_u gv[4], cv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          gv[u] = ldx4<f32x4_u>(g + (h + u) * NN + e);
          cv[u] = ld<f32x4_u>(c + (h + u) * NN + e);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] = acc[k] + fmaxf(gv[u][k] * cv[u][k], 0.0f);
      }
      for (; h < H; ++h) {
        const f32x4_u gv = ldx4<f32x4_u>(g + h * NN + e), cv = ld<f32x4_u>(c + h * NN + e);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = acc[k] + fmaxf(gv[k] * cv[k], 0.0f);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] = acc[k] / fH;
      st<f32x4_u>(o + e, acc);
    } else {
      const int64_t lim = min(NN, e + VEC);
      for (int64_t ee = e; ee < lim; ++ee) {
        float acc = 0.0f;
        for (int64_t h = 0; h < H; ++h) acc = acc + fmaxf(ldx(g + h * NN + ee) * c[h * NN + ee], 0.0f);
        o[ee] = acc / fH;
      }
    }
  }
}

// All heads' loads of a thread in flight at once (2 H independent 16-B loads, H <= HMAX), one float4 per thread, grid =
// (ceil(NN / 1024), B): every block does the same amount of work and the dispatcher back-fills finished blocks
// (the grid-stride form above gives 6 of 32 blocks per sample a second trip at N = 197).  Heads are still added in
// index order.
template <int HMAX, typename TG>
__global__ __launch_bounds__(kThreads) void headmean_flat_kernel(
    const TG* __restrict__ grad, const float* __restrict__ cam, float* __restrict__ out, int H, int64_t NN) {
  const int64_t b = blockIdx.y;
  const float fH = (float)H;
  const TG* g = grad + b * H * NN;
  const float* c = cam + b * H * NN;
  float* o = out + b * NN;
  const int64_t e = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 4;
  if (e >= NN) return;
  if (e + 3 < NN) {
    f32x4_u gv[HMAX], cv[HMAX];
#pragma unroll
    for (int h = 0; h < HMAX; ++h)
      if (h < H) {
        if constexpr (sizeof(TG) == 4) gv[h] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_u*>(g + h * NN + e));
        else gv[h] = ldx4<f32x4_u>(g + h * NN + e);
        cv[h] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_u*>(c + h * NN + e));
      }
    f32x4_u acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int h = 0; h < HMAX; ++h)
      if (h < H) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = acc[k] + fmaxf(gv[h][k] * cv[h][k], 0.0f);
      }
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = acc[k] / fH;
    st<f32x4_u>(o + e, acc);
  } else {
    for (int64_t ee = e; ee < NN; ++ee) {
      float acc = 0.0f;
      for (int h = 0; h < H; ++h) acc = acc + fmaxf(ldx(g + h * NN + ee) * c[h * NN + ee], 0.0f);
      o[ee] = acc / fH;
    }
  }
}

// Head mean of a bf16 model's attention probabilities (te_attn_headmean_bf16): out[b,e] = (sum_h f(attn[b,h,e])) / H over
// e in [0, n), f = identity or max(., 0), heads added in index order in fp32 (torch's mean; the bf16 -> fp32 widening is
// exact).  n = N*N, or N for the class-token row alone.  A thread owns 8 consecutive elements: one 16-B load per head --
// up to HB heads' loads in flight, as in headmean_flat_kernel -- and two 16-B stores.  Head bases are arbitrary element
// offsets (N*N is odd at N = 197), hence the 2-byte-aligned vector type: gfx950 global loads take any alignment.
typedef uint32_t u32x4_u2 __attribute__((ext_vector_type(4), aligned(2)));

template <int HB, bool CLAMP>
__global__ __launch_bounds__(kThreads) void attn_headmean_kernel(
    const te_bf16_t* __restrict__ attn, int64_t a_sb, int64_t a_sh, float* __restrict__ out, int H, int64_t n) {
  const int64_t b = blockIdx.y;
  const float fH = (float)H;
  const te_bf16_t* a = attn + b * a_sb;
  float* o = out + b * n;
  const int64_t e = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 8;
  if (e >= n) return;
  if (e + 7 < n) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int h0 = 0; h0 < H; h0 += HB) {
      u32x4_u2 v[HB];
#pragma unroll
      for (int u = 0; u < HB; ++u)
        if (h0 + u < H) v[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_u2*>(a + (h0 + u) * a_sh + e));
#pragma unroll
      for (int u = 0; u < HB; ++u)
        if (h0 + u < H) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float lo = __uint_as_float(v[u][k] << 16), hi = __uint_as_float(v[u][k] & 0xffff0000u);
            acc[2 * k] = acc[2 * k] + (CLAMP ? fmaxf(lo, 0.0f) : lo);
            acc[2 * k + 1] = acc[2 * k + 1] + (CLAMP ? fmaxf(hi, 0.0f) : hi);
          }
        }
    }
    st<f32x4_u>(o + e, f32x4_u{acc[0] / fH, acc[1] / fH, acc[2] / fH, acc[3] / fH});
    st<f32x4_u>(o + e + 4, f32x4_u{acc[4] / fH, acc[5] / fH, acc[6] / fH, acc[7] / fH});
  } else {
    for (int64_t ee = e; ee < n; ++ee) {
      float acc = 0.0f;
      for (int h = 0; h < H; ++h) {
        const float x = ldx(a + h * a_sh + ee);
        acc = acc + (CLAMP ? fmaxf(x, 0.0f) : x);
      }
      o[ee] = acc / fH;
    }
  }
}

inline int pick_blocks_per_sample(int64_t B, int64_t n) {
  // >= ~2048 blocks in flight for the chip (256 CUs x 8), each block >= 4096 elements, <= 64 chunks.
  int64_t bps = te_ceil_div(2048, B);
  const int64_t max_by_size = te_ceil_div(n, 4096);
  if (bps > max_by_size) bps = max_by_size;
  if (bps > 64) bps = 64;
  if (bps < 1) bps = 1;
  return (int)bps;
}

}  // namespace

// ================================================================================================
extern "C" size_t te_add_relprop_workspace_bytes(int64_t B, int64_t n) {
  if (B <= 0 || n <= 0) return 0;
  return te_align_up((size_t)B * 64 * 3 * sizeof(double), 256);
}

namespace {
template <typename TX>
int add_relprop(const float* R, const TX* X0, const TX* X1, float* out0, float* out1, int64_t B, int64_t n,
                int64_t x1_batch_stride, int variant, void* ws, size_t ws_bytes, te_stream_t stream_) {
  if (!R || !X0 || !X1 || !out0 || !out1 || B <= 0 || n <= 0) return TE_ERR_INVALID_ARG;
  if (x1_batch_stride != 0 && x1_batch_stride != n) return TE_ERR_INVALID_ARG;
  const int var = variant & 0xff;
  if (var != TE_VARIANT_OURS && var != TE_VARIANT_LRP) return TE_ERR_INVALID_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  const bool vec = (n % 4 == 0) && te_aligned16(R) && vec_aligned(X0) && vec_aligned(X1) &&
                   te_aligned16(out0) && te_aligned16(out1);
  const int bps = pick_blocks_per_sample(B, n);
  int64_t chunk = te_ceil_div(n, bps);
  chunk = te_ceil_div(chunk, 4) * 4;
  dim3 grid(bps, (unsigned)B), block(kThreads);
  double* partial = (double*)ws;
  if (var == TE_VARIANT_OURS) {
    if (!ws || ws_bytes < te_add_relprop_workspace_bytes(B, n)) return TE_ERR_WORKSPACE;
    if (vec) {
      add_sums_kernel<4><<<grid, block, 0, stream>>>(R, X0, X1, partial, n, x1_batch_stride, chunk);
      add_apply_kernel<4, true><<<grid, block, 0, stream>>>(R, X0, X1, out0, out1, partial, n,
                                                            x1_batch_stride, chunk);
    } else {
      add_sums_kernel<1><<<grid, block, 0, stream>>>(R, X0, X1, partial, n, x1_batch_stride, chunk);
      add_apply_kernel<1, true><<<grid, block, 0, stream>>>(R, X0, X1, out0, out1, partial, n,
                                                            x1_batch_stride, chunk);
    }
  } else {
    if (vec)
      add_apply_kernel<4, false><<<grid, block, 0, stream>>>(R, X0, X1, out0, out1, nullptr, n,
                                                             x1_batch_stride, chunk);
    else
      add_apply_kernel<1, false><<<grid, block, 0, stream>>>(R, X0, X1, out0, out1, nullptr, n,
                                                             x1_batch_stride, chunk);
  }
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

}  // namespace

extern "C" int te_add_relprop_f32(const float* R, const float* X0, const float* X1, float* out0,
                                  float* out1, int64_t B, int64_t n, int64_t x1_batch_stride,
                                  int variant, void* ws, size_t ws_bytes, te_stream_t stream_) {
  return add_relprop(R, X0, X1, out0, out1, B, n, x1_batch_stride, variant, ws, ws_bytes, stream_);
}

extern "C" int te_add_relprop_bf16(const float* R, const te_bf16_t* X0, const te_bf16_t* X1, float* out0, float* out1,
                                   int64_t B, int64_t n, int64_t x1_batch_stride, int variant, void* ws,
                                   size_t ws_bytes, te_stream_t stream_) {
  return add_relprop(R, X0, X1, out0, out1, B, n, x1_batch_stride, variant, ws, ws_bytes, stream_);
}

// ---- Add with the per-sample rescale deferred to the consumers ---------------------------------------
extern "C" size_t te_add_relprop_deferred_workspace_bytes(int64_t B, int64_t n) {
  return te_add_relprop_workspace_bytes(B, n);
}

namespace {
template <typename TX>
int add_relprop_deferred(const float* R, const TX* X0, const TX* X1, float* a, float* b, float* fac, int64_t B,
                         int64_t n, int64_t x1_batch_stride, void* ws, size_t ws_bytes, te_stream_t stream_) {
  if (!R || !X0 || !X1 || !a || !b || !fac || B <= 0 || n <= 0) return TE_ERR_INVALID_ARG;
  if (x1_batch_stride != 0 && x1_batch_stride != n) return TE_ERR_INVALID_ARG;
  if (B > 65535) return TE_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < te_add_relprop_workspace_bytes(B, n)) return TE_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const bool vec = (n % 4 == 0) && te_aligned16(R) && vec_aligned(X0) && vec_aligned(X1) && te_aligned16(a) &&
                   te_aligned16(b);
  const int bps = pick_blocks_per_sample(B, n);      // the same chunking (and fold order) as te_add_relprop_f32
  int64_t chunk = te_ceil_div(n, bps);
  chunk = te_ceil_div(chunk, 4) * 4;
  dim3 grid(bps, (unsigned)B), block(kThreads);
  double* partial = (double*)ws;
  if (vec) add_deferred_kernel<4><<<grid, block, 0, stream>>>(R, X0, X1, a, b, partial, n, x1_batch_stride, chunk);
  else add_deferred_kernel<1><<<grid, block, 0, stream>>>(R, X0, X1, a, b, partial, n, x1_batch_stride, chunk);
  add_factors_kernel<<<dim3((unsigned)B), dim3(64), 0, stream>>>(partial, fac, bps);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

}  // namespace

extern "C" int te_add_relprop_deferred_f32(const float* R, const float* X0, const float* X1, float* a, float* b,
                                           float* fac, int64_t B, int64_t n, int64_t x1_batch_stride, void* ws,
                                           size_t ws_bytes, te_stream_t stream_) {
  return add_relprop_deferred(R, X0, X1, a, b, fac, B, n, x1_batch_stride, ws, ws_bytes, stream_);
}

extern "C" int te_add_relprop_deferred_bf16(const float* R, const te_bf16_t* X0, const te_bf16_t* X1, float* a, float* b,
                                            float* fac, int64_t B, int64_t n, int64_t x1_batch_stride, void* ws,
                                            size_t ws_bytes, te_stream_t stream_) {
  return add_relprop_deferred(R, X0, X1, a, b, fac, B, n, x1_batch_stride, ws, ws_bytes, stream_);
}

// ---- broadcast-mask Add ---------------------------------------------------------------------------
namespace {
inline int addb_blocks(int64_t B, int64_t rows) {
  int64_t nb = te_ceil_div(1024, B);
  if (nb > rows) nb = rows;
  if (nb > 64) nb = 64;
  if (nb < 1) nb = 1;
  return (int)nb;
}
}  // namespace

extern "C" size_t te_add_bcast_relprop_workspace_bytes(int64_t B, int64_t H, int64_t N) {
  if (B <= 0 || H <= 0 || N <= 0) return 0;
  const size_t part = te_align_up((size_t)B * 64 * (N + 2) * sizeof(double), 256);
  const size_t fac = te_align_up((size_t)B * 2 * sizeof(float), 256);
  const size_t bvec = te_align_up((size_t)B * N * sizeof(float), 256);
  return part + fac + bvec;
}

namespace {
// TX = float: te_add_bcast_relprop_f32; TX = te_bf16_t: the bf16 form, variant ours only (as every bf16 rule)
template <typename TX>
int add_bcast_relprop(const float* R, const TX* X0, const TX* mask, float* out0, float* out1, int64_t B, int64_t H,
                      int64_t N, int variant, void* ws, size_t ws_bytes, te_stream_t stream_) {
  if (!R || !X0 || !mask || !out0 || B <= 0 || H <= 0 || N <= 0) return TE_ERR_INVALID_ARG;
  const int var = variant & 0xff;
  if (var != TE_VARIANT_OURS && var != TE_VARIANT_LRP) return TE_ERR_INVALID_ARG;
  if (sizeof(TX) != sizeof(float) && var != TE_VARIANT_OURS) return TE_ERR_UNSUPPORTED;
  if (N > (int64_t)kMaxColsPerThread * kThreads) return TE_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < te_add_bcast_relprop_workspace_bytes(B, H, N)) return TE_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t rows = H * N;
  const int nblk = addb_blocks(B, rows);
  const int64_t rpb = te_ceil_div(rows, nblk);
  char* p = (char*)ws;
  double* partial = (double*)p;
  p += te_align_up((size_t)B * 64 * (N + 2) * sizeof(double), 256);
  float* fac = (float*)p;
  p += te_align_up((size_t)B * 2 * sizeof(float), 256);
  float* bvec = (float*)p;
  dim3 grid(nblk, (unsigned)B), block(kThreads);
  addb_sums_kernel<false, TX><<<grid, block, 0, stream>>>(R, X0, mask, partial, nullptr, rows, N, rpb);
  addb_finalize_kernel<TX><<<dim3((unsigned)B), block, 0, stream>>>(partial, mask, fac, bvec, N, nblk,
                                                                   var == TE_VARIANT_OURS ? 1 : 0, nullptr);
  addb_apply_kernel<TX><<<grid, block, 0, stream>>>(R, X0, mask, fac, bvec, out0, out1, rows, N, rpb);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

template <typename TX>
int add_bcast_relprop_deferred(const float* R, const TX* X0, const TX* mask, float* a, float* out1, float* fac,
                               int64_t B, int64_t H, int64_t N, void* ws, size_t ws_bytes, te_stream_t stream_) {
  if (!R || !X0 || !mask || !a || !fac || B <= 0 || H <= 0 || N <= 0) return TE_ERR_INVALID_ARG;
  if (N > (int64_t)kMaxColsPerThread * kThreads || B > 65535) return TE_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < te_add_bcast_relprop_workspace_bytes(B, H, N)) return TE_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t rows = H * N;
  const int nblk = addb_blocks(B, rows);
  const int64_t rpb = te_ceil_div(rows, nblk);
  char* p = (char*)ws;
  double* partial = (double*)p;
  p += te_align_up((size_t)B * 64 * (N + 2) * sizeof(double), 256);
  p += te_align_up((size_t)B * 2 * sizeof(float), 256);        // (the two-pass form's factor slot: unused here)
  float* bvec = (float*)p;
  dim3 grid(nblk, (unsigned)B), block(kThreads);
  addb_sums_kernel<true, TX><<<grid, block, 0, stream>>>(R, X0, mask, partial, a, rows, N, rpb);
  addb_finalize_kernel<TX><<<dim3((unsigned)B), block, 0, stream>>>(partial, mask, fac, bvec, N, nblk, 1, out1);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}
}  // namespace

extern "C" int te_add_bcast_relprop_f32(const float* R, const float* X0, const float* mask,
                                        float* out0, float* out1, int64_t B, int64_t H, int64_t N,
                                        int variant, void* ws, size_t ws_bytes, te_stream_t stream_) {
  return add_bcast_relprop(R, X0, mask, out0, out1, B, H, N, variant, ws, ws_bytes, stream_);
}

extern "C" int te_add_bcast_relprop_bf16(const float* R, const te_bf16_t* X0, const te_bf16_t* mask, float* out0,
                                         float* out1, int64_t B, int64_t H, int64_t N, int variant, void* ws,
                                         size_t ws_bytes, te_stream_t stream_) {
  return add_bcast_relprop(R, X0, mask, out0, out1, B, H, N, variant, ws, ws_bytes, stream_);
}

// Deferred form (variant ours): ONE pass over R and X0 writes the unscaled a = X0 . S; fac [B,2] = {fa, fb} goes to the
// consumer (te_matmul_relprop_qk_f32 multiplies the relevance operand by fa in its S tile); out1 [B,N]
// (optional) = the mask's relevance, already scaled.  a * fa is bitwise te_add_bcast_relprop_f32's out0.
extern "C" int te_add_bcast_relprop_deferred_f32(const float* R, const float* X0, const float* mask, float* a,
                                                 float* out1, float* fac, int64_t B, int64_t H, int64_t N, void* ws,
                                                 size_t ws_bytes, te_stream_t stream_) {
  return add_bcast_relprop_deferred(R, X0, mask, a, out1, fac, B, H, N, ws, ws_bytes, stream_);
}

extern "C" int te_add_bcast_relprop_deferred_bf16(const float* R, const te_bf16_t* X0, const te_bf16_t* mask, float* a,
                                                  float* out1, float* fac, int64_t B, int64_t H, int64_t N, void* ws,
                                                  size_t ws_bytes, te_stream_t stream_) {
  return add_bcast_relprop_deferred(R, X0, mask, a, out1, fac, B, H, N, ws, ws_bytes, stream_);
}

// ---- Clone ------------------------------------------------------------------------------------------
namespace {
template <typename TX>
int clone_relprop(const float* R0, const float* R1, const float* R2, const TX* X, float* out, int64_t n,
                  te_stream_t stream_) {
  if (!R0 || !R1 || !X || !out || n <= 0) return TE_ERR_INVALID_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  const bool vec = (n % 4 == 0) && te_aligned16(R0) && te_aligned16(R1) && vec_aligned(X) &&
                   te_aligned16(out) && (!R2 || te_aligned16(R2));
  const int vecw = vec ? 4 : 1;
  // one float4 per thread (every block the same work, back-filled by the dispatcher) up to 64 K blocks; the
  // grid-stride loop takes over beyond
  int64_t blocks = te_ceil_div(n, (int64_t)kThreads * vecw);
  if (blocks > 65535) blocks = 65535;
  if (blocks < 1) blocks = 1;
  dim3 grid((unsigned)blocks), block(kThreads);
  if (R2) {
    if (vec) clone_kernel<4, 3><<<grid, block, 0, stream>>>(R0, R1, R2, X, out, n);
    else clone_kernel<1, 3><<<grid, block, 0, stream>>>(R0, R1, R2, X, out, n);
  } else {
    if (vec) clone_kernel<4, 2><<<grid, block, 0, stream>>>(R0, R1, nullptr, X, out, n);
    else clone_kernel<1, 2><<<grid, block, 0, stream>>>(R0, R1, nullptr, X, out, n);
  }
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

template <typename TX>
int clone_relprop_scaled(const float* R0, const float* s0, int64_t s0_stride, const float* R1, const float* s1,
                         int64_t s1_stride, const float* R2, const float* s2, int64_t s2_stride, const TX* X, float* out,
                         int64_t B, int64_t n, te_stream_t stream_) {
  if (!R0 || !R1 || !X || !out || B <= 0 || n <= 0) return TE_ERR_INVALID_ARG;
  if (B > 65535) return TE_ERR_UNSUPPORTED;
  hipStream_t stream = (hipStream_t)stream_;
  const bool vec = (n % 4 == 0) && te_aligned16(R0) && te_aligned16(R1) && vec_aligned(X) && te_aligned16(out) &&
                   (!R2 || te_aligned16(R2));
  const int vecw = vec ? 4 : 1;
  int64_t bx = te_ceil_div(n, (int64_t)kThreads * vecw);       // one float4 per thread
  const int64_t want = te_ceil_div(65535, B);
  if (bx > want) bx = want;
  if (bx < 1) bx = 1;
  dim3 grid((unsigned)bx, (unsigned)B), block(kThreads);
#define TE_CLONE_S(V, NUM) \
  clone_scaled_kernel<V, NUM><<<grid, block, 0, stream>>>(R0, s0, s0_stride, R1, s1, s1_stride, R2, s2, s2_stride, X, out, n)
  if (R2) {
    if (vec) TE_CLONE_S(4, 3);
    else TE_CLONE_S(1, 3);
  } else {
    if (vec) TE_CLONE_S(4, 2);
    else TE_CLONE_S(1, 2);
  }
#undef TE_CLONE_S
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

}  // namespace

extern "C" int te_clone_relprop_f32(const float* R0, const float* R1, const float* R2, const float* X,
                                    float* out, int64_t n, te_stream_t stream_) {
  return clone_relprop(R0, R1, R2, X, out, n, stream_);
}

extern "C" int te_clone_relprop_bf16(const float* R0, const float* R1, const float* R2, const te_bf16_t* X, float* out,
                                     int64_t n, te_stream_t stream_) {
  return clone_relprop(R0, R1, R2, X, out, n, stream_);
}

extern "C" int te_clone_relprop_scaled_f32(const float* R0, const float* s0, int64_t s0_stride, const float* R1,
                                           const float* s1, int64_t s1_stride, const float* R2, const float* s2,
                                           int64_t s2_stride, const float* X, float* out, int64_t B, int64_t n,
                                           te_stream_t stream_) {
  return clone_relprop_scaled(R0, s0, s0_stride, R1, s1, s1_stride, R2, s2, s2_stride, X, out, B, n, stream_);
}

extern "C" int te_clone_relprop_scaled_bf16(const float* R0, const float* s0, int64_t s0_stride, const float* R1,
                                            const float* s1, int64_t s1_stride, const float* R2, const float* s2,
                                            int64_t s2_stride, const te_bf16_t* X, float* out, int64_t B, int64_t n,
                                            te_stream_t stream_) {
  return clone_relprop_scaled(R0, s0, s0_stride, R1, s1, s1_stride, R2, s2, s2_stride, X, out, B, n, stream_);
}

// ---- IndexSelect ------------------------------------------------------------------------------------
namespace {
template <typename TX>
int index_select_relprop(const float* R, const TX* X, float* out, int64_t B, int64_t N, int64_t C, int64_t index,
                         te_stream_t stream_) {
  if (!R || !X || !out || B <= 0 || N <= 0 || C <= 0 || index < 0 || index >= N)
    return TE_ERR_INVALID_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  int64_t blocks = te_ceil_div(B * N * C, (int64_t)kThreads * 4);
  if (blocks > 4096) blocks = 4096;
  index_select_kernel<<<dim3((unsigned)blocks), dim3(kThreads), 0, stream>>>(R, X, out, B, N, C, index);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

}  // namespace

extern "C" int te_index_select_relprop_f32(const float* R, const float* X, float* out, int64_t B,
                                           int64_t N, int64_t C, int64_t index, te_stream_t stream_) {
  return index_select_relprop(R, X, out, B, N, C, index, stream_);
}

extern "C" int te_index_select_relprop_bf16(const float* R, const te_bf16_t* X, float* out, int64_t B, int64_t N,
                                            int64_t C, int64_t index, te_stream_t stream_) {
  return index_select_relprop(R, X, out, B, N, C, index, stream_);
}

// ---- gradient x relevance head mean ----------------------------------------------------------------
namespace {
template <typename TG>
int gradcam_headmean(const TG* grad, const float* cam, float* out, int64_t B, int64_t H, int64_t N,
                     te_stream_t stream_) {
  if (!grad || !cam || !out || B <= 0 || H <= 0 || N <= 0) return TE_ERR_INVALID_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t NN = N * N;
  int64_t bx = te_ceil_div(NN, (int64_t)kThreads * 4);
  // flat kernel, every head in flight; the grid-stride kernel (<= 2048 blocks) covers H > 16 and B > 65535
  if (H <= 16 && B <= 65535) {
    const dim3 grid((unsigned)bx, (unsigned)B), blk(kThreads);
    if (H <= 12) headmean_flat_kernel<12><<<grid, blk, 0, stream>>>(grad, cam, out, (int)H, NN);
    else headmean_flat_kernel<16><<<grid, blk, 0, stream>>>(grad, cam, out, (int)H, NN);
    TE_RETURN_IF_LAUNCH_FAILED();
    return TE_OK;
  }
  const int64_t want = te_ceil_div(2048, B);
  if (bx > want) bx = want;
  if (bx < 1) bx = 1;
  headmean_kernel<4><<<dim3((unsigned)bx, (unsigned)B), dim3(kThreads), 0, stream>>>(grad, cam, out, H, NN);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}
}  // namespace

extern "C" int te_gradcam_headmean_f32(const float* grad, const float* cam, float* out, int64_t B,
                                       int64_t H, int64_t N, te_stream_t stream_) {
  return gradcam_headmean(grad, cam, out, B, H, N, stream_);
}

extern "C" int te_gradcam_headmean_bf16(const te_bf16_t* grad, const float* cam, float* out, int64_t B, int64_t H,
                                        int64_t N, te_stream_t stream_) {
  return gradcam_headmean(grad, cam, out, B, H, N, stream_);
}

// ---- head mean of bf16 attention probabilities --------------------------------------------------------
extern "C" int te_attn_headmean_bf16(const te_bf16_t* attn, int64_t a_sb, int64_t a_sh, float* out, int64_t B, int64_t H,
                                     int64_t N, int flags, te_stream_t stream_) {
  if (!attn || !out || B <= 0 || H <= 0 || N <= 0 || a_sb < 0 || a_sh < 0) return TE_ERR_INVALID_ARG;
  if (flags & ~(TE_HEADMEAN_CLAMP | TE_HEADMEAN_ROW0)) return TE_ERR_INVALID_ARG;
  if (B > 65535 || H > 0x7fffffff) return TE_ERR_UNSUPPORTED;
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t n = (flags & TE_HEADMEAN_ROW0) ? N : N * N;
  const dim3 grid((unsigned)te_ceil_div(n, (int64_t)kThreads * 8), (unsigned)B), blk(kThreads);
  const bool clamp = (flags & TE_HEADMEAN_CLAMP) != 0;
  // every head in flight for H <= 12 (ViT-B, BERT-base) and H <= 16 (ViT-L); more heads take several trips of 16
  if (H <= 12) {
    if (clamp) attn_headmean_kernel<12, true><<<grid, blk, 0, stream>>>(attn, a_sb, a_sh, out, (int)H, n);
    else attn_headmean_kernel<12, false><<<grid, blk, 0, stream>>>(attn, a_sb, a_sh, out, (int)H, n);
  } else {
    if (clamp) attn_headmean_kernel<16, true><<<grid, blk, 0, stream>>>(attn, a_sb, a_sh, out, (int)H, n);
    else attn_headmean_kernel<16, false><<<grid, blk, 0, stream>>>(attn, a_sb, a_sh, out, (int)H, n);
  }
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}
