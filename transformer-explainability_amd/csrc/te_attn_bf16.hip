// te_attn_bf16.hip -- attention producers of a bf16 model: the forward of an attention block and its
// attention-gradient backward on bf16 operands, head dim 64, 1 <= N <= 640, any [B,H,N,64] strides (thirds of ViT's fused qkv
// activation, BERT's three Linear outputs).  The counterpart of te_attn_long.hip / te_attn_fwd6l.hip / te_attn_bwd6l.hip, which
// take fp32 operands.
//
// Rounding contract (include/te_relprop.h): every output is bf16, rounded to nearest even exactly ONCE from an fp32 value, at the
// points where the stock bf16 path rounds -- z_qk = bf16(q k^T), x = bf16(z_qk * scale) from the rounded z_qk,
// s = bf16(x + mask), attn = bf16(softmax_fp32(s)), out = bf16(attn v) with the rounded attn; d_attn = bf16(d_out v^T),
// d_s = bf16(attn (d_attn - rowsum(attn d_attn))) from the rounded d_attn, d_q = bf16(scale d_s k), d_k = bf16(scale d_s^T q),
// d_v = bf16(attn^T d_out).  A bf16 x bf16 product is exact in the fp32 accumulator of v_mfma_f32_32x32x16_bf16, so every
// product is an fp32-accumulated sum of exact terms.
//
// Structure.  One bf16 plane per operand means one MFMA product where the fp32 producers run three to six: these kernels are
// bound by the N x N loads and stores.
//   forward / backward rows   one WAVE per 32 query rows, four waves (128 rows) per workgroup.  The score block of 32 keys is
//        formed TRANSPOSED, X[key][query] = K_block . Q^T: the query sits on the lane, the keys in the 16 accumulator registers,
//        so a row's softmax is a walk over the lane's own registers plus one exchange with lane ^ 32, and the rounded block is
//        at once the B operand of the second product out^T[d][query] += v^T[d][key] X[key][query] (no LDS round trip).  Because
//        the softmax input is a bf16 value, the whole [N][32] score strip stays in registers as packed bf16 (N = 640: 160
//        VGPRs).  v^T (k^T in the backward) of the head is staged once per workgroup in LDS, the keys of a 32-block permuted so
//        that the eight a lane needs for one MFMA step are 16 contiguous bytes.  N x N tensors travel through a wave-private
//        LDS tile of [32 rows][128 keys]: whole 256-byte row segments go to (come from) global memory.
//   backward columns          one wave per 32 keys, four key blocks per workgroup: attn and d_attn blocks are read as
//        X[query][key] (key on the lane: a row's 32 keys are one 64-byte segment), d_s is formed as in the row kernel from the
//        row sums that kernel left in the workspace, and d_v^T = d_out^T X, d_k^T = q^T d_s with d_out^T / q^T staged 64 query
//        rows at a time.
// Every sum has an order that depends on N and the position only: a batch equals its samples bit for bit.
#include "te_x6.h"

namespace {

// (te_common.h: the vector types, Strided, crow; te_x6.h: TE_MFMA_BF16 -- one plane per operand here, no split)
typedef uint32_t u32x2_u __attribute__((ext_vector_type(2), aligned(2)));      // four bf16 of a row of an N x N tensor (N odd: 2-byte aligned)

constexpr int kT = 256;          // threads: four waves
constexpr int TI = 32;           // query rows (keys) per wave
constexpr int NMAX = 640;
constexpr int CH = 4;            // key blocks per pass of the wave-private tile (128 keys)
constexpr int TP = CH * TI + 4;  // tile row pitch in bf16 (264 B: 8-byte aligned rows, lanes 2 banks apart)
constexpr int QC = 64;           // query rows staged per step of the column kernel

__device__ __forceinline__ float bf2f(uint32_t b) { return __uint_as_float(b << 16); }
// two fp32 -> two bf16, round to nearest even (v_cvt_pk_bf16_f32); a in the low half.  (pack2, exp_neg and tpos are local: the
// rounding points of a bf16 model have no twin among the fp32 kernels)
__device__ __forceinline__ uint32_t pack2(float a, float b) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{a, b}, bf16x2));
}
__device__ __forceinline__ float lo(uint32_t p) { return __uint_as_float(p << 16); }
__device__ __forceinline__ float hi(uint32_t p) { return __uint_as_float(p & 0xffff0000u); }
__device__ __forceinline__ float rbf(float x) { return lo(pack2(x, 0.0f)); }      // x rounded to bf16, as fp32
// exp(x) for x <= 0 as v_exp_f32(x log2 e): the argument's rounding is a relative error of |x| 2^-24 in the result (scores are
// bf16 values and the result is rounded to bf16, 2^-9), in a handful of instructions where the library routine takes ~40 -- the
// softmax is two exponentials per element of the N x N tensor and bounded the kernel (VALU) before
__device__ __forceinline__ float exp_neg(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }

// Position of row kk of a 32-block in a transposed LDS operand: MFMA step s (rows 16 s ..) of lane half kh takes the rows
// 16 s + 4 kh + {0..3, 8..11} -- registers 8 s .. 8 s + 7 of the block that is the other operand -- from 8 contiguous elements.
__device__ __forceinline__ int tpos(int kk) { return (kk & 16) | (((kk >> 2) & 1) << 3) | (((kk >> 3) & 1) << 2) | (kk & 3); }

__device__ __forceinline__ bf16x8 as_frag(u32x4 v) { return __builtin_bit_cast(bf16x8, v); }

// dst[64][pitch] (LDS) = the transpose of rows [0, npad) of a strided [rows][64] bf16 operand, rows of a 32-block at tpos();
// rows >= valid are zero.  Whole workgroup; the caller synchronises.
__device__ __forceinline__ void stage_transposed(uint16_t* __restrict__ dst, int pitch, const uint16_t* __restrict__ src,
                                                 int64_t sn, int valid, int npad) {
  for (int idx = threadIdx.x; idx < npad * 8; idx += kT) {
    const int row = idx >> 3, c = idx & 7;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (row < valid) v = *reinterpret_cast<const u32x4*>(src + (int64_t)row * sn + 8 * c);
    const int p = (row & ~31) | tpos(row & 31);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      dst[(8 * c + 2 * e) * pitch + p] = (uint16_t)(v[e] & 0xffffu);
      dst[(8 * c + 2 * e + 1) * pitch + p] = (uint16_t)(v[e] >> 16);
    }
  }
}

// the four 16-byte pieces of row `row` of a strided operand a lane feeds to the four MFMA steps over the 64 features
__device__ __forceinline__ void load_frags(bf16x8 (&f)[4], const uint16_t* __restrict__ base, int64_t sn, int row, bool ok,
                                           int kh) {
#pragma unroll
  for (int st = 0; st < 4; ++st) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if (ok) v = *reinterpret_cast<const u32x4*>(base + (int64_t)row * sn + 16 * st + 8 * kh);
    f[st] = as_frag(v);
  }
}

// Wave-private tile [32][TP] <-> rows of an N x N tensor.  g = the tensor's element (row 0 of the tile, first key of the pass);
// rows < nrow and keys < cnt exist.  A lane moves four keys; 32 lanes cover 256 bytes of one row.
__device__ __forceinline__ void tile_store(const uint16_t* __restrict__ tile, uint16_t* __restrict__ g, int64_t ld, int nrow,
                                           int cnt, int lane) {
  const int c4 = (lane & 31) * 4;
  if (c4 >= cnt) return;
#pragma unroll 4
  for (int p = 0; p < TI / 2; ++p) {
    const int row = 2 * p + (lane >> 5);
    if (row >= nrow) continue;
    const u32x2 v = *reinterpret_cast<const u32x2*>(tile + row * TP + c4);
    uint16_t* d = g + (int64_t)row * ld + c4;
    if (c4 + 4 <= cnt) {
      *reinterpret_cast<u32x2_u*>(d) = v;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c4 + e < cnt) d[e] = (uint16_t)(v[e >> 1] >> (16 * (e & 1)));
    }
  }
}
// the same pass, additionally x = bf16(z * scale) of every element to a second tensor
__device__ __forceinline__ void tile_store_scaled(const uint16_t* __restrict__ tile, uint16_t* __restrict__ g,
                                                  uint16_t* __restrict__ gx, float scale, int64_t ld, int nrow, int cnt,
                                                  int lane) {
  const int c4 = (lane & 31) * 4;
  if (c4 >= cnt) return;
#pragma unroll 4
  for (int p = 0; p < TI / 2; ++p) {
    const int row = 2 * p + (lane >> 5);
    if (row >= nrow) continue;
    const u32x2 v = *reinterpret_cast<const u32x2*>(tile + row * TP + c4);
    const u32x2 x = {pack2(lo(v[0]) * scale, hi(v[0]) * scale), pack2(lo(v[1]) * scale, hi(v[1]) * scale)};
    const int64_t off = (int64_t)row * ld + c4;
    if (c4 + 4 <= cnt) {
      if (g) *reinterpret_cast<u32x2_u*>(g + off) = v;
      if (gx) *reinterpret_cast<u32x2_u*>(gx + off) = x;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c4 + e < cnt) {
          if (g) g[off + e] = (uint16_t)(v[e >> 1] >> (16 * (e & 1)));
          if (gx) gx[off + e] = (uint16_t)(x[e >> 1] >> (16 * (e & 1)));
        }
    }
  }
}
// global -> registers (tile_fetch: the request can be issued long before the tile is free) -> tile (tile_commit); rows >= nrow and
// keys >= cnt are zero
struct TileRegs {
  u32x2 v[TI / 2];
};
__device__ __forceinline__ void tile_fetch(TileRegs& t, const uint16_t* __restrict__ g, int64_t ld, int nrow, int cnt, int lane) {
  const int c4 = (lane & 31) * 4;
#pragma unroll
  for (int p = 0; p < TI / 2; ++p) {
    const int row = 2 * p + (lane >> 5);
    u32x2 v = {0u, 0u};
    if (row < nrow && c4 < cnt) {
      const uint16_t* s = g + (int64_t)row * ld + c4;
      if (c4 + 4 <= cnt) {
        v = *reinterpret_cast<const u32x2_u*>(s);
      } else {
        uint32_t e4[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (c4 + e < cnt) e4[e] = s[e];
        v = u32x2{e4[0] | (e4[1] << 16), e4[2] | (e4[3] << 16)};
      }
    }
    t.v[p] = v;
  }
}
__device__ __forceinline__ void tile_commit(uint16_t* __restrict__ tile, const TileRegs& t, int lane) {
  const int c4 = (lane & 31) * 4;
#pragma unroll
  for (int p = 0; p < TI / 2; ++p) *reinterpret_cast<u32x2*>(tile + (2 * p + (lane >> 5)) * TP + c4) = t.v[p];
}
// a [32][64] result held transposed (acc[db][e] = element (row lane & 31, feature 32 db + crow(e, kh))) times `mul`, rounded,
// through the tile to rows of a strided [rows][64] operand
__device__ __forceinline__ void store_rows64(uint16_t* __restrict__ tile, const f32x16 (&acc)[2], float mul,
                                             uint16_t* __restrict__ dst, int64_t sn, int nrow, int lane) {
  const int lr = lane & 31, kh = lane >> 5;
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<u32x2*>(tile + lr * TP + 32 * db + 8 * g + 4 * kh) =
          u32x2{pack2(acc[db][4 * g] * mul, acc[db][4 * g + 1] * mul), pack2(acc[db][4 * g + 2] * mul, acc[db][4 * g + 3] * mul)};
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int row = 8 * p + (lane >> 3), c8 = (lane & 7) * 8;
    if (row < nrow) {
      const u32x2 a = *reinterpret_cast<const u32x2*>(tile + row * TP + c8);
      const u32x2 b = *reinterpret_cast<const u32x2*>(tile + row * TP + c8 + 4);
      *reinterpret_cast<u32x4*>(dst + (int64_t)row * sn + c8) = u32x4{a[0], a[1], b[0], b[1]};
    }
  }
  __builtin_amdgcn_wave_barrier();
}

struct FwdArgs {
  const uint16_t *q, *k, *v, *mask;
  uint16_t *zqk, *xsc, *attn, *out;
  Strided qs, ks, vs, os;
  int H, N, ntile, nwg;
  float scale;
};

// ------------------------------------------------------------------------------------------------
// forward.  NB = key blocks the register strip holds (32 NB >= N).
// ------------------------------------------------------------------------------------------------
template <int NB>
__global__ __launch_bounds__(kT) void attn_fwd_bf16_kernel(FwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint16_t smem16[];
  const int N = a.N, nb = (N + TI - 1) / TI, npad = nb * TI, pitch = npad + 8;
  uint16_t* vT = smem16;                                     // [64][pitch]
  uint16_t* tiles = vT + 64 * pitch;                         // [4][32][TP]
  float* mk = reinterpret_cast<float*>(tiles + 4 * TI * TP); // [npad] additive mask of the sample; -inf past the last key
  const int bh = blockIdx.x / a.nwg, wg = blockIdx.x - bh * a.nwg, b = bh / a.H, h = bh - b * a.H;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 31, kh = lane >> 5;
  const uint16_t* q_bh = a.q + b * a.qs.sb + h * a.qs.sh;
  const uint16_t* k_bh = a.k + b * a.ks.sb + h * a.ks.sh;
  stage_transposed(vT, pitch, a.v + b * a.vs.sb + h * a.vs.sh, a.vs.sn, N, npad);
  for (int j = threadIdx.x; j < npad; j += kT)
    mk[j] = j < N ? (a.mask ? bf2f(a.mask[(int64_t)b * N + j]) : 0.0f) : -INFINITY;
  __syncthreads();
  const int it = wg * 4 + wave;
  if (it >= a.ntile) return;
  const int i0 = it * TI, nrow = min(TI, N - i0);
  uint16_t* tile = tiles + wave * TI * TP;
  const int64_t rowoff = ((int64_t)bh * N + i0) * N;

  bf16x8 qf[4];
  load_frags(qf, q_bh, a.qs.sn, i0 + lr, lr < nrow, kh);
  uint32_t sp[NB][8];          // s = bf16(bf16(z * scale) + mask) of (key 32 jb + crow(e, kh), query i0 + lr), e = 2 t, 2 t + 1
  const bool want_zx = a.zqk || a.xsc;
#pragma unroll
  for (int jb = 0; jb < NB; ++jb) {
    if (jb < nb) {
      bf16x8 kf[4];
      load_frags(kf, k_bh, a.ks.sn, jb * TI + lr, jb * TI + lr < N, kh);
      f32x16 z;
#pragma unroll
      for (int e = 0; e < 16; ++e) z[e] = 0.0f;
#pragma unroll
      for (int st = 0; st < 4; ++st) z = TE_MFMA_BF16(kf[st], qf[st], z);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const u32x2 zb = {pack2(z[4 * g], z[4 * g + 1]), pack2(z[4 * g + 2], z[4 * g + 3])};
        if (want_zx) *reinterpret_cast<u32x2*>(tile + lr * TP + (jb % CH) * TI + 8 * g + 4 * kh) = zb;
        const f32x4 m = *reinterpret_cast<const f32x4*>(mk + jb * TI + 8 * g + 4 * kh);
        sp[jb][2 * g] = pack2(rbf(lo(zb[0]) * a.scale) + m[0], rbf(hi(zb[0]) * a.scale) + m[1]);
        sp[jb][2 * g + 1] = pack2(rbf(lo(zb[1]) * a.scale) + m[2], rbf(hi(zb[1]) * a.scale) + m[3]);
      }
      if (want_zx && (jb % CH == CH - 1 || jb == nb - 1)) {
        const int j0 = (jb / CH) * CH * TI;
        __builtin_amdgcn_wave_barrier();
        tile_store_scaled(tile, a.zqk ? a.zqk + rowoff + j0 : nullptr, a.xsc ? a.xsc + rowoff + j0 : nullptr, a.scale, N, nrow,
                          min(CH * TI, N - j0), lane);
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
  // softmax of the lane's row, fp32: the lane's keys, then the other half's (lane ^ 32)
  float mx = -INFINITY;
#pragma unroll
  for (int jb = 0; jb < NB; ++jb)
    if (jb < nb) {
#pragma unroll
      for (int t = 0; t < 8; ++t) mx = fmaxf(mx, fmaxf(lo(sp[jb][t]), hi(sp[jb][t])));
    }
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  float sum = 0.0f;
#pragma unroll
  for (int jb = 0; jb < NB; ++jb)
    if (jb < nb) {
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        sum = sum + exp_neg(lo(sp[jb][t]) - mx);
        sum = sum + exp_neg(hi(sp[jb][t]) - mx);
      }
    }
  {
    const float other = __shfl_xor(sum, 32, 64);
    sum = kh ? other + sum : sum + other;          // the same order of the two halves in both lanes
  }
  const float inv = 1.0f / sum;
  f32x16 o[2];
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[db][e] = 0.0f;
#pragma unroll
  for (int jb = 0; jb < NB; ++jb) {
    if (jb < nb) {
      uint32_t pb[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) pb[t] = pack2(exp_neg(lo(sp[jb][t]) - mx) * inv, exp_neg(hi(sp[jb][t]) - mx) * inv);
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<u32x2*>(tile + lr * TP + (jb % CH) * TI + 8 * g + 4 * kh) = u32x2{pb[2 * g], pb[2 * g + 1]};
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8 pf = as_frag(u32x4{pb[4 * s], pb[4 * s + 1], pb[4 * s + 2], pb[4 * s + 3]});
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          const bf16x8 vf = as_frag(*reinterpret_cast<const u32x4*>(vT + (32 * db + lr) * pitch + jb * TI + 16 * s + 8 * kh));
          o[db] = TE_MFMA_BF16(vf, pf, o[db]);
        }
      }
      if (jb % CH == CH - 1 || jb == nb - 1) {
        const int j0 = (jb / CH) * CH * TI;
        __builtin_amdgcn_wave_barrier();
        tile_store(tile, a.attn + rowoff + j0, N, nrow, min(CH * TI, N - j0), lane);
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
  store_rows64(tile, o, 1.0f, a.out + b * a.os.sb + h * a.os.sh + (int64_t)i0 * a.os.sn, a.os.sn, nrow, lane);
}

struct BwdRowArgs {
  const uint16_t *dout, *k, *v, *attn;
  uint16_t *dattn, *dq;
  float* rowdot;
  Strided dos, ks, vs, dqs;
  int H, N, ntile, nwg, need_qk;
  float scale;
};

// d_s = bf16(attn (d_attn - rowsum)): ONE definition for the row and the column kernel, which must agree bit for bit
__device__ __forceinline__ uint32_t ds_pair(uint32_t p, uint32_t g, float r0, float r1) {
  return pack2(lo(p) * (lo(g) - r0), hi(p) * (hi(g) - r1));
}

// ------------------------------------------------------------------------------------------------
// backward, row side: d_attn = d_out v^T ; rowsum_i = sum_j attn d_attn ; d_q = scale (d_s k)
// ------------------------------------------------------------------------------------------------
template <int NB>
__global__ __launch_bounds__(kT) void attn_bwd_rows_bf16_kernel(BwdRowArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint16_t smem16[];
  const int N = a.N, nb = (N + TI - 1) / TI, npad = nb * TI, pitch = npad + 8;
  uint16_t* kT_ = smem16;                                    // [64][pitch] (need_qk)
  uint16_t* tiles = a.need_qk ? kT_ + 64 * pitch : smem16;   // [4][32][TP]
  const int bh = blockIdx.x / a.nwg, wg = blockIdx.x - bh * a.nwg, b = bh / a.H, h = bh - b * a.H;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 31, kh = lane >> 5;
  const uint16_t* v_bh = a.v + b * a.vs.sb + h * a.vs.sh;
  if (a.need_qk) {
    stage_transposed(kT_, pitch, a.k + b * a.ks.sb + h * a.ks.sh, a.ks.sn, N, npad);
    __syncthreads();
  }
  const int it = wg * 4 + wave;
  if (it >= a.ntile) return;
  const int i0 = it * TI, nrow = min(TI, N - i0);
  uint16_t* tile = tiles + wave * TI * TP;
  const int64_t rowoff = ((int64_t)bh * N + i0) * N;

  bf16x8 gf[4];
  load_frags(gf, a.dout + b * a.dos.sb + h * a.dos.sh, a.dos.sn, i0 + lr, lr < nrow, kh);
  uint32_t dap[NB][8];         // d_attn (bf16) of (key 32 jb + crow(e, kh), query i0 + lr)
  float dot = 0.0f;
  constexpr int NCH = (NB + CH - 1) / CH;
  TileRegs pre;                // the attn rows of a pass, requested before the work that hides their latency
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    if (c * CH < nb) {
      const int j0 = c * CH * TI, cnt = min(CH * TI, N - j0);
      if (a.need_qk) tile_fetch(pre, a.attn + rowoff + j0, N, nrow, cnt, lane);
#pragma unroll
      for (int t = 0; t < CH; ++t) {
        const int jb = c * CH + t;
        if (jb < NB && jb < nb) {
          bf16x8 vf[4];
          load_frags(vf, v_bh, a.vs.sn, jb * TI + lr, jb * TI + lr < N, kh);
          f32x16 z;
#pragma unroll
          for (int e = 0; e < 16; ++e) z[e] = 0.0f;
#pragma unroll
          for (int st = 0; st < 4; ++st) z = TE_MFMA_BF16(vf[st], gf[st], z);
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            dap[jb][2 * g] = pack2(z[4 * g], z[4 * g + 1]);
            dap[jb][2 * g + 1] = pack2(z[4 * g + 2], z[4 * g + 3]);
            *reinterpret_cast<u32x2*>(tile + lr * TP + t * TI + 8 * g + 4 * kh) = u32x2{dap[jb][2 * g], dap[jb][2 * g + 1]};
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
      tile_store(tile, a.dattn + rowoff + j0, N, nrow, cnt, lane);
      __builtin_amdgcn_wave_barrier();
      if (a.need_qk) {
        tile_commit(tile, pre, lane);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int t = 0; t < CH; ++t) {
          const int jb = c * CH + t;
          if (jb < NB && jb < nb) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const u32x2 p = *reinterpret_cast<const u32x2*>(tile + lr * TP + t * TI + 8 * g + 4 * kh);
              dot = dot + lo(p[0]) * lo(dap[jb][2 * g]);
              dot = dot + hi(p[0]) * hi(dap[jb][2 * g]);
              dot = dot + lo(p[1]) * lo(dap[jb][2 * g + 1]);
              dot = dot + hi(p[1]) * hi(dap[jb][2 * g + 1]);
            }
          }
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
  if (!a.need_qk) return;
  {
    const float other = __shfl_xor(dot, 32, 64);
    dot = kh ? other + dot : dot + other;
  }
  if (kh == 0 && lr < nrow) a.rowdot[(int64_t)bh * N + i0 + lr] = dot;
  f32x16 o[2];
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[db][e] = 0.0f;
  tile_fetch(pre, a.attn + rowoff, N, nrow, min(CH * TI, N), lane);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    if (c * CH < nb) {
      tile_commit(tile, pre, lane);
      __builtin_amdgcn_wave_barrier();
      if ((c + 1) * CH < nb) tile_fetch(pre, a.attn + rowoff + (c + 1) * CH * TI, N, nrow, min(CH * TI, N - (c + 1) * CH * TI), lane);
#pragma unroll
      for (int t = 0; t < CH; ++t) {
        const int jb = c * CH + t;
        if (jb < NB && jb < nb) {
          uint32_t ds[8];
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const u32x2 p = *reinterpret_cast<const u32x2*>(tile + lr * TP + t * TI + 8 * g + 4 * kh);
            ds[2 * g] = ds_pair(p[0], dap[jb][2 * g], dot, dot);
            ds[2 * g + 1] = ds_pair(p[1], dap[jb][2 * g + 1], dot, dot);
          }
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            const bf16x8 pf = as_frag(u32x4{ds[4 * s], ds[4 * s + 1], ds[4 * s + 2], ds[4 * s + 3]});
#pragma unroll
            for (int db = 0; db < 2; ++db) {
              const bf16x8 kf = as_frag(*reinterpret_cast<const u32x4*>(kT_ + (32 * db + lr) * pitch + jb * TI + 16 * s + 8 * kh));
              o[db] = TE_MFMA_BF16(kf, pf, o[db]);
            }
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
  store_rows64(tile, o, a.scale, a.dq + b * a.dqs.sb + h * a.dqs.sh + (int64_t)i0 * a.dqs.sn, a.dqs.sn, nrow, lane);
}

struct BwdColArgs {
  const uint16_t *attn, *dattn, *dout, *q;
  const float* rowdot;
  uint16_t *dv, *dk;
  Strided dos, qs, dvs, dks;
  int H, N, nwg, need_qk;
  float scale;
};

// ------------------------------------------------------------------------------------------------
// backward, column side: d_v^T[d][key] = sum_i d_out^T[d][i] attn[i][key] ; d_k^T = scale sum_i q^T[d][i] d_s[i][key]
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void attn_bwd_cols_bf16_kernel(BwdColArgs a) {
  constexpr int pitch = QC + 8;
  __shared__ __attribute__((aligned(16))) uint16_t doT[64 * pitch];
  __shared__ __attribute__((aligned(16))) uint16_t qT[64 * pitch];
  __shared__ float rd[QC];
  const int N = a.N;
  const int bh = blockIdx.x / a.nwg, wg = blockIdx.x - bh * a.nwg, b = bh / a.H, h = bh - b * a.H;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 31, kh = lane >> 5;
  const int j0 = (wg * 4 + wave) * TI;
  const bool wave_ok = j0 < N;
  const bool key_ok = j0 + lr < N;
  // lanes past the last key read column N - 1 (their values are zeroed): column j0 + lr of the last row would lie past the buffer
  const int jc = key_ok ? j0 + lr : N - 1;
  const uint16_t* a_bh = a.attn + (int64_t)bh * N * N + jc;
  const uint16_t* g_bh = a.dattn + (int64_t)bh * N * N + jc;
  const uint16_t* do_bh = a.dout + b * a.dos.sb + h * a.dos.sh;
  const uint16_t* q_bh = a.need_qk ? a.q + b * a.qs.sb + h * a.qs.sh : nullptr;
  f32x16 av[2], ak[2];
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      av[db][e] = 0.0f;
      ak[db][e] = 0.0f;
    }
  for (int ic = 0; ic < N; ic += QC) {
    const int valid = min(QC, N - ic);
    __syncthreads();
    stage_transposed(doT, pitch, do_bh + (int64_t)ic * a.dos.sn, a.dos.sn, valid, QC);
    if (a.need_qk) {
      stage_transposed(qT, pitch, q_bh + (int64_t)ic * a.qs.sn, a.qs.sn, valid, QC);
      if (threadIdx.x < QC) rd[threadIdx.x] = threadIdx.x < valid ? a.rowdot[(int64_t)bh * N + ic + threadIdx.x] : 0.0f;
    }
    __syncthreads();
    if (!wave_ok) continue;
#pragma unroll
    for (int ib = 0; ib < QC / TI; ++ib) {
      if (ic + ib * TI < N) {
        uint32_t pa[8], ga[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          uint32_t pv[2], gv[2];
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const int i = ic + ib * TI + crow(2 * t + u, kh);
            const bool ok = key_ok && i < N;
            const int64_t off = (int64_t)(i < N ? i : 0) * N;
            pv[u] = a_bh[off];
            gv[u] = a.need_qk ? g_bh[off] : 0u;
            if (!ok) pv[u] = gv[u] = 0u;
          }
          pa[t] = pv[0] | (pv[1] << 16);
          ga[t] = gv[0] | (gv[1] << 16);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const bf16x8 pf = as_frag(u32x4{pa[4 * s], pa[4 * s + 1], pa[4 * s + 2], pa[4 * s + 3]});
#pragma unroll
          for (int db = 0; db < 2; ++db) {
            const bf16x8 df = as_frag(*reinterpret_cast<const u32x4*>(doT + (32 * db + lr) * pitch + ib * TI + 16 * s + 8 * kh));
            av[db] = TE_MFMA_BF16(df, pf, av[db]);
          }
        }
        if (a.need_qk) {
          uint32_t ds[8];
#pragma unroll
          for (int t = 0; t < 8; ++t)
            ds[t] = ds_pair(pa[t], ga[t], rd[ib * TI + crow(2 * t, kh)], rd[ib * TI + crow(2 * t + 1, kh)]);
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            const bf16x8 pf = as_frag(u32x4{ds[4 * s], ds[4 * s + 1], ds[4 * s + 2], ds[4 * s + 3]});
#pragma unroll
            for (int db = 0; db < 2; ++db) {
              const bf16x8 qf = as_frag(*reinterpret_cast<const u32x4*>(qT + (32 * db + lr) * pitch + ib * TI + 16 * s + 8 * kh));
              ak[db] = TE_MFMA_BF16(qf, pf, ak[db]);
            }
          }
        }
      }
    }
  }
  if (!key_ok) return;
  uint16_t* dv_row = a.dv + b * a.dvs.sb + h * a.dvs.sh + (int64_t)(j0 + lr) * a.dvs.sn;
  uint16_t* dk_row = a.need_qk ? a.dk + b * a.dks.sb + h * a.dks.sh + (int64_t)(j0 + lr) * a.dks.sn : nullptr;
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = 32 * db + 8 * g + 4 * kh;
      *reinterpret_cast<u32x2*>(dv_row + d) = u32x2{pack2(av[db][4 * g], av[db][4 * g + 1]), pack2(av[db][4 * g + 2], av[db][4 * g + 3])};
      if (a.need_qk)
        *reinterpret_cast<u32x2*>(dk_row + d) = u32x2{pack2(ak[db][4 * g] * a.scale, ak[db][4 * g + 1] * a.scale),
                                                      pack2(ak[db][4 * g + 2] * a.scale, ak[db][4 * g + 3] * a.scale)};
    }
}

inline size_t lds_strip(int64_t N, bool operand, bool mask) {
  const size_t npad = (size_t)te_ceil_div(N, TI) * TI;
  return (operand ? 64 * (npad + 8) * sizeof(uint16_t) : 0) + 4 * TI * TP * sizeof(uint16_t) + (mask ? npad * sizeof(float) : 0);
}

template <typename K>
inline bool allow_lds(K kern, size_t bytes) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
}

// 16-byte loads of whole feature rows: every stride a multiple of 8 elements, the base 16-byte aligned
inline bool view_ok(const void* p, int64_t sb, int64_t sh, int64_t sn) {
  return te_aligned16(p) && sb >= 0 && sh >= 0 && sn >= 64 && (sn % 8) == 0 && (sh % 8) == 0 && (sb % 8) == 0;
}

inline int launch_status() { return hipGetLastError() == hipSuccess ? TE_OK : TE_ERR_UNSUPPORTED; }

}  // namespace

extern "C" int te_attention_bf16_supported(int64_t N, int64_t D) { return (D == 64 && N >= 1 && N <= NMAX) ? 1 : 0; }

extern "C" size_t te_attention_backward_strided_bf16_workspace_bytes(int64_t B, int64_t H, int64_t N) {
  if (B <= 0 || H <= 0 || N <= 0) return 0;
  return te_align_up((size_t)(B * H * N) * sizeof(float), 256);
}

extern "C" int te_attention_forward_strided_bf16(const te_bf16_t* q, int64_t q_sb, int64_t q_sh, int64_t q_sn,
                                                 const te_bf16_t* k, int64_t k_sb, int64_t k_sh, int64_t k_sn,
                                                 const te_bf16_t* v, int64_t v_sb, int64_t v_sh, int64_t v_sn,
                                                 const te_bf16_t* mask, te_bf16_t* z_qk, te_bf16_t* x_scaled, te_bf16_t* attn,
                                                 te_bf16_t* out, int64_t o_sb, int64_t o_sh, int64_t o_sn, int64_t B, int64_t H,
                                                 int64_t N, int64_t D, float scale, te_stream_t stream_) {
  if (!q || !k || !v || !attn || !out || B <= 0 || H <= 0 || N <= 0) return TE_ERR_INVALID_ARG;
  if (!te_attention_bf16_supported(N, D)) return TE_ERR_UNSUPPORTED;
  const int64_t ntile = te_ceil_div(N, TI), nwg = te_ceil_div(ntile, 4);
  if (B * H * nwg > 0x7fffffff) return TE_ERR_UNSUPPORTED;
  if (!view_ok(q, q_sb, q_sh, q_sn) || !view_ok(k, k_sb, k_sh, k_sn) || !view_ok(v, v_sb, v_sh, v_sn) ||
      !view_ok(out, o_sb, o_sh, o_sn))
    return TE_ERR_UNSUPPORTED;
  FwdArgs a{q, k, v, mask, z_qk, x_scaled, attn, out, Strided{q_sb, q_sh, q_sn}, Strided{k_sb, k_sh, k_sn},
            Strided{v_sb, v_sh, v_sn}, Strided{o_sb, o_sh, o_sn}, (int)H, (int)N, (int)ntile, (int)nwg, scale};
  const dim3 grid((unsigned)(B * H * nwg)), block(kT);
  const size_t lds = lds_strip(N, true, true);
  hipStream_t stream = (hipStream_t)stream_;
  (void)hipGetLastError();
  if (N <= 256) {
    if (!allow_lds(attn_fwd_bf16_kernel<8>, lds_strip(256, true, true))) return TE_ERR_UNSUPPORTED;
    attn_fwd_bf16_kernel<8><<<grid, block, lds, stream>>>(a);
  } else if (N <= 512) {
    if (!allow_lds(attn_fwd_bf16_kernel<16>, lds_strip(512, true, true))) return TE_ERR_UNSUPPORTED;
    attn_fwd_bf16_kernel<16><<<grid, block, lds, stream>>>(a);
  } else {
    if (!allow_lds(attn_fwd_bf16_kernel<20>, lds_strip(NMAX, true, true))) return TE_ERR_UNSUPPORTED;
    attn_fwd_bf16_kernel<20><<<grid, block, lds, stream>>>(a);
  }
  return launch_status();
}

extern "C" int te_attention_backward_strided_bf16(const te_bf16_t* d_out, int64_t do_sb, int64_t do_sh, int64_t do_sn,
                                                  const te_bf16_t* q, int64_t q_sb, int64_t q_sh, int64_t q_sn,
                                                  const te_bf16_t* k, int64_t k_sb, int64_t k_sh, int64_t k_sn,
                                                  const te_bf16_t* v, int64_t v_sb, int64_t v_sh, int64_t v_sn,
                                                  const te_bf16_t* attn, te_bf16_t* d_attn,
                                                  te_bf16_t* d_q, int64_t dq_sb, int64_t dq_sh, int64_t dq_sn,
                                                  te_bf16_t* d_k, int64_t dk_sb, int64_t dk_sh, int64_t dk_sn,
                                                  te_bf16_t* d_v, int64_t dv_sb, int64_t dv_sh, int64_t dv_sn,
                                                  int64_t B, int64_t H, int64_t N, int64_t D, float scale, int need_qk,
                                                  void* ws, size_t ws_bytes, te_stream_t stream_) {
  if (!d_out || !v || !attn || !d_attn || !d_v || B <= 0 || H <= 0 || N <= 0) return TE_ERR_INVALID_ARG;
  if (need_qk && (!q || !k || !d_q || !d_k)) return TE_ERR_INVALID_ARG;
  if (!te_attention_bf16_supported(N, D)) return TE_ERR_UNSUPPORTED;
  const int64_t ntile = te_ceil_div(N, TI), nwg = te_ceil_div(ntile, 4);
  if (B * H * nwg > 0x7fffffff) return TE_ERR_UNSUPPORTED;
  if (!view_ok(d_out, do_sb, do_sh, do_sn) || !view_ok(v, v_sb, v_sh, v_sn) || !view_ok(d_v, dv_sb, dv_sh, dv_sn))
    return TE_ERR_UNSUPPORTED;
  if (need_qk && (!view_ok(q, q_sb, q_sh, q_sn) || !view_ok(k, k_sb, k_sh, k_sn) || !view_ok(d_q, dq_sb, dq_sh, dq_sn) ||
                  !view_ok(d_k, dk_sb, dk_sh, dk_sn)))
    return TE_ERR_UNSUPPORTED;
  if (need_qk && (!ws || ws_bytes < te_attention_backward_strided_bf16_workspace_bytes(B, H, N))) return TE_ERR_WORKSPACE;
  const int nq = need_qk ? 1 : 0;
  BwdRowArgs r{d_out, k, v, attn, d_attn, d_q, (float*)ws, Strided{do_sb, do_sh, do_sn}, Strided{k_sb, k_sh, k_sn},
               Strided{v_sb, v_sh, v_sn}, Strided{dq_sb, dq_sh, dq_sn}, (int)H, (int)N, (int)ntile, (int)nwg, nq, scale};
  BwdColArgs c{attn, d_attn, d_out, q, (const float*)ws, d_v, d_k, Strided{do_sb, do_sh, do_sn}, Strided{q_sb, q_sh, q_sn},
               Strided{dv_sb, dv_sh, dv_sn}, Strided{dk_sb, dk_sh, dk_sn}, (int)H, (int)N, (int)nwg, nq, scale};
  const dim3 grid((unsigned)(B * H * nwg)), block(kT);
  const size_t lds = lds_strip(N, nq != 0, false);
  hipStream_t stream = (hipStream_t)stream_;
  (void)hipGetLastError();
  if (N <= 256) {
    if (!allow_lds(attn_bwd_rows_bf16_kernel<8>, lds_strip(256, true, false))) return TE_ERR_UNSUPPORTED;
    attn_bwd_rows_bf16_kernel<8><<<grid, block, lds, stream>>>(r);
  } else if (N <= 512) {
    if (!allow_lds(attn_bwd_rows_bf16_kernel<16>, lds_strip(512, true, false))) return TE_ERR_UNSUPPORTED;
    attn_bwd_rows_bf16_kernel<16><<<grid, block, lds, stream>>>(r);
  } else {
    if (!allow_lds(attn_bwd_rows_bf16_kernel<20>, lds_strip(NMAX, true, false))) return TE_ERR_UNSUPPORTED;
    attn_bwd_rows_bf16_kernel<20><<<grid, block, lds, stream>>>(r);
  }
  if (launch_status() != TE_OK) return TE_ERR_UNSUPPORTED;
  attn_bwd_cols_bf16_kernel<<<grid, block, 0, stream>>>(c);
  return launch_status();
}
