// te_attn_rules.hip -- the ONE-PASS QK rule for gfx950 (head dim 64): it reads its N x N operands once and never writes
// S = safe_divide(R, Z) to memory (modules/layers_ours.py:48-60,122-127; ViT_LRP.py:157-173; BERT.py:367-393).  The same kernel
// evaluates the softmax half of the attention backward.
//
//   QK rule (RULE):  S = sd(R_nn, Z_qk) [N,N];  cam_q = q .(S k);  cam_k = k .(S^T q)
//   backward (BWD):  d_s = attn .(d_attn - rowsum(d_attn . attn)) * scale;  d_q = d_s k;  d_k = d_s^T q
//
// Z is the cached forward product of the very einsum / MatMul whose rule is evaluated (te_attn_mfma.hip header).  The host side of
// this file only launches: which calls reach it (the rule for 224 < N <= 4096, the backward for 160 < N <= 224 without the forward output) is
// the dispatch of te_attn.hip.  The AV rule's one-pass kernel lives in te_attn_kb.hip.
//
// qk_rule_kernel: one workgroup (512 threads = 8 waves, one per (b, h, key group of <= 256 keys)) keeps k (<= 256 x 64)
// resident in LDS and walks the query rows in tiles of 32.  Per tile the row-side product AND the column-side product
// are formed from the same LDS image of the [32, keys] tile:
//
//   S tile [32,keys] = sd(R_nn, Z_qk) and the q tile [32,64] -> LDS
//   cam_q  = S k         32x64 output as eight 16x16 blocks, one per wave (v_mfma_f32_16x16x4_f32), K = keys:
//                        every wave busy without a split-K reduction
//   cam_k += S^T q       (keys x 64) as 32x32 blocks, two per wave, accumulators live across all row tiles
//
// Every tile of the next step is requested (global -> registers) before the MFMAs of the current one start, so HBM
// latency hides under ~4000 MFMA-pipe cycles per wave and tile.  Traffic per (b,h): R_nn, Z_qk, q, k read once, cam_q,
// cam_k written once = the rule's algorithmic bytes (the 64 x 64-tile kernels of te_attn_mfma.hip wrote S to a workspace
// and re-read it: ~8 N^2 passes per layer).  N > 256: the keys are cut into groups of <= 256 (one workgroup each); the
// column side of a group is complete, the row side (cam_q) is a per-group partial that a small finishing kernel sums in
// group order.
//
// All reductions run in a fixed order that depends on N only: a batch equals its samples run one by one, bit for bit.
// LDS images: PADDED row-major tiles (row strides 68 / 260 floats, see below) -- every MFMA fragment address is a per-lane
// base plus a compile-time offset, and both products read the same row-major tile (the row side as 16-B fragments along a
// row, the column side as 4-byte fragments down the rows).
#include "te_internal.h"

namespace te_attn_rules {

namespace {

constexpr int TI = 32;         // query rows per tile
constexpr int kT = 512;        // threads per workgroup
constexpr int kWaves = kT / 64;

// (te_common.h: Strided, f32x4_u, crow, zero16, load4, TE_MFMA32 / TE_MFMA16)

// The [TI][nj] tile of an [N,N] operand in flight: thread t holds float4 slots idx = t + 512 r (r < 4) of the
// [TI][NJ32 / 4] float4 grid; (row, c4) per slot are loop-invariant.
struct WideTile {
  f32x4 v[4];
};
struct WideMap {
  int row[4], c4[4];   // row < 0: no slot
};
// `per_row` float4 slots per tile row: nj32 / 4 packs the tile densely; 64 gives every wave one whole row (the QK rule:
// with its 260-float row stride a wave that straddles two rows puts 16-B stores of one pass on the same banks)
__device__ __forceinline__ WideMap wide_map(int per_row) {
  WideMap m;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int idx = threadIdx.x + r * kT;
    const int row = idx / per_row;
    m.row[r] = (row < TI) ? row : -1;
    m.c4[r] = idx - row * per_row;
  }
  return m;
}
// slot r alone (the QK kernel requests the next tile's slots one at a time between its MFMA groups)
__device__ __forceinline__ f32x4 load_wide_slot(const WideMap& m, int r, const float* __restrict__ src, int64_t ld,
                                                int rows_valid, int cols_valid) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (m.row[r] >= 0 && m.row[r] < rows_valid) v = load4(src + (int64_t)m.row[r] * ld, m.c4[r] << 2, cols_valid);
  return v;
}
// Branch-free variant for the rule kernels (every key group has nj >= 4 keys: supported()).  The guarded loads above
// cost ~35 vector / scalar instructions per float4 (64-bit addresses, a divergent branch per slot, a scalar tail) --
// and a vector instruction beside MFMAs is not free.  Here a slot is ONE 16-B load at uniform
// base + 32-bit offset: rows beyond N re-read the tile's last row, chunks at / beyond the row's end read its last four
// columns (always in bounds); fast_fix(), run when the tile is consumed, assembles the partial chunk and zeroes what
// lies outside.  kind: 0 outside the tile, 1 whole chunk, 2 the row's partial last chunk.
struct FastMap {
  int row[4], coff[4], kind[4];
  int nslots;     // float4 slots of the tile (TI * nj32 / 4): slot round r is wholly outside from r * kT >= nslots on
  bool fast;      // nj >= 4: the branch-free loads are legal (else the guarded load_wide_slot)
  bool plain;     // every slot of every thread is a whole in-tile chunk (nj == 256): full tiles need no fast_fix
};
__device__ __forceinline__ FastMap fast_map(int per_row, int nj32, int nj) {
  FastMap m;
  const int tailc = nj >> 2, rem = nj & 3;
  m.nslots = TI * per_row;
  m.fast = nj >= 4;
  m.plain = nj == nj32 && nj32 == 256;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int idx = threadIdx.x + r * kT;
    const int row = idx / per_row, c4 = idx - row * per_row;
    const bool in = row < TI;
    m.kind[r] = !in ? 0 : (c4 < tailc ? 1 : ((c4 == tailc && rem != 0) ? 2 : 0));
    m.row[r] = in ? row : 0;
    m.coff[r] = (m.kind[r] == 1) ? (c4 << 2) : nj - 4;
  }
  return m;
}
__device__ __forceinline__ f32x4 fast_load(const FastMap& m, int r, const float* __restrict__ base, int i0, int N,
                                           int rows_valid) {
  const unsigned off = (unsigned)(i0 + min(m.row[r], rows_valid - 1)) * (unsigned)N + (unsigned)m.coff[r];
  return *reinterpret_cast<const f32x4_u*>(base + off);
}
__device__ __forceinline__ f32x4 fast_fix(const FastMap& m, int r, f32x4 L, int nj, int rows_valid) {
  const int rem = nj & 3;
  f32x4 t;
  t[0] = rem == 1 ? L[3] : (rem == 2 ? L[2] : L[1]);
  t[1] = rem == 2 ? L[3] : (rem == 3 ? L[2] : 0.0f);
  t[2] = rem == 3 ? L[3] : 0.0f;
  t[3] = 0.0f;
  const bool ok = m.row[r] < rows_valid, full = ok && m.kind[r] == 1, tail = ok && m.kind[r] == 2;
  f32x4 out;
#pragma unroll
  for (int e = 0; e < 4; ++e) out[e] = full ? L[e] : (tail ? t[e] : 0.0f);
  return out;
}

// ------------------------------------------------------------------------------------------------
// PADDED LDS images of the rule kernel.  [rows][64] tiles have a row stride of SLD = 68 floats, the [TI][keys] tile
// QLD = 260 (also read as 16-B fragments down 16 rows), the transposed k image [64][QLD].  Every fragment address is then a per-lane base plus a compile-time offset -- no XOR per read, no
// address registers -- and the column-side products read their K = query-row operands as 4-byte fragments straight
// from the row-major tiles, so the TRANSPOSED copies of the tile (64 scalar ds_write_b32 + address arithmetic per
// thread and tile) are gone.  Vector-ALU instructions are not free beside MFMAs: a CU's time for these rules is the
// SUM of its MFMA cycles and its other vector-instruction cycles.
// ------------------------------------------------------------------------------------------------
constexpr int SLD = 68;
constexpr int QLD = 260;

__device__ __forceinline__ void p_store_wide(float* __restrict__ lds, const WideMap& m, const WideTile& t, int ld) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (m.row[r] >= 0) *reinterpret_cast<f32x4*>(lds + m.row[r] * ld + (m.c4[r] << 2)) = t.v[r];
}
// ... transposed: element (j, d) -> KtT[d][j], lanes along j (conflict-free scalar LDS stores; the 16-B global loads of
// a wave touch 64 rows, whose other chunks the same wave fetches in its next trips)
__device__ __forceinline__ void p_stage_keys_T(float* __restrict__ KtT, const float* __restrict__ src, int64_t sn, int nj,
                                               int nj32) {
  const int row = threadIdx.x & 255;
  if (row < nj32) {
    for (int c = threadIdx.x >> 8; c < 16; c += 2) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (row < nj) v = *reinterpret_cast<const f32x4_u*>(src + (int64_t)row * sn + (c << 2));
#pragma unroll
      for (int e = 0; e < 4; ++e) KtT[((c << 2) + e) * QLD + row] = v[e];
    }
  }
}

// column-side product of one row tile: acc[s] += W^T[32 keys x 32 rows] Y[32 rows x 32 d] for the 32x32 blocks
// t = wave + 8 s = 2 jb + db, straight from the ROW-MAJOR tiles: Wp = W + kh * WLD + lr, Yp = Y + kh * SLD + lr; the
// fragment of query rows (2 m, 2 m + 1) is one 4-byte read at + 2 m * stride.  `between(g)`, g = 0..7, runs after
// every group of four MFMAs (whether or not the wave owns a block there): one global memory instruction of the caller.
// Only the first `kgmax` groups of four MFMAs (eight query rows each) run: the rows of the last tile beyond N are zero.
template <int WLD, class F>
__device__ __forceinline__ void p_col_product(f32x16 (&acc)[2], const float* __restrict__ Wp, const float* __restrict__ Yp,
                                              int wave, int nblk, int kgmax, F&& between) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int t = wave + s * kWaves;
    const bool active = t < nblk;
    const float* wp = Wp + (t >> 1) * 32;
    const float* yp = Yp + (t & 1) * 32;
    float a[TI / 2], bq[TI / 2];
    if (active) {
#pragma unroll
      for (int m = 0; m < TI / 2; ++m) {
        a[m] = wp[2 * m * WLD];
        bq[m] = yp[2 * m * SLD];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kg = 0; kg < TI / 8; ++kg) {
      if (active && kg < kgmax) {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[s] = TE_MFMA32(a[4 * kg + j], bq[4 * kg + j], acc[s]);
      }
      between(s * (TI / 8) + kg);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// out = RAW ? acc : (x . acc) * scale for the column accumulators; x from global memory -- all sixteen values of a block
// requested before the first is used
template <bool RAW>
__device__ __forceinline__ void p_col_epilogue(const f32x16 (&acc)[2], const float* __restrict__ XG, int64_t xsn,
                                               float* __restrict__ out, int64_t osn, int nj, int wave, int lr, int kh, int nblk,
                                               float scale) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int t = wave + s * kWaves;
    if (t < nblk) {
      const int d = (t & 1) * 32 + lr;
      float x[16];
      if constexpr (!RAW) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int j = (t >> 1) * 32 + crow(e, kh);
          x[e] = XG[(int64_t)min(j, nj - 1) * xsn + d];
        }
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int j = (t >> 1) * 32 + crow(e, kh);
        float val = acc[s][e];
        if constexpr (!RAW) val = (x[e] * val) * scale;
        if (j < nj) out[(int64_t)j * osn + d] = val;
      }
    }
  }
}

// row-side product with a 16x16 output block over the first n16 16-key groups (keys beyond nj are zero in both images):
// acc += W[16 x keys] X[keys x 16], Wp = W + arow * QLD + 4 kq (the S tile), Xp = k^T + dcol * QLD + 4 kq; two groups per
// trip (an odd last group alone), the next trip's fragments requested before this trip's eight MFMAs
__device__ __forceinline__ void p_row_product16(f32x4& acc, const float* __restrict__ Wp, const float* __restrict__ Xp,
                                                int n16) {
  const int np = (n16 + 1) >> 1;
  f32x4 a0 = *reinterpret_cast<const f32x4*>(Wp), a1 = *reinterpret_cast<const f32x4*>(Wp + 16);
  f32x4 b0 = *reinterpret_cast<const f32x4*>(Xp), b1 = *reinterpret_cast<const f32x4*>(Xp + 16);
  for (int kp = 0; kp < np; ++kp) {
    const int o = (kp + 1 < np) ? (kp + 1) * 32 : 0;      // (last trip: a harmless re-read)
    const f32x4 na0 = *reinterpret_cast<const f32x4*>(Wp + o), na1 = *reinterpret_cast<const f32x4*>(Wp + o + 16);
    const f32x4 nb0 = *reinterpret_cast<const f32x4*>(Xp + o), nb1 = *reinterpret_cast<const f32x4*>(Xp + o + 16);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = TE_MFMA16(a0[j], b0[j], acc);
    if (2 * kp + 1 < n16) {
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = TE_MFMA16(a1[j], b1[j], acc);
    }
    __builtin_amdgcn_sched_barrier(0);
    a0 = na0, a1 = na1, b0 = nb0, b1 = nb1;
  }
}

enum { RULE = 0, BWD = 1 };

// Phase timing of workgroup 0: prof[wave * 8 + phase] accumulates shader-clock cycles between the marks of one tile.
// Every launch passes nullptr.  The argument stays because dropping it and its never-taken branches changes the
// kernel's code (120 instructions, 4 VGPRs): a kernel change that needs its own same-box measurement.
#define TE_MARK(slot)                                                          \
  do {                                                                         \
    if (prof != nullptr && blockIdx.x == 0 && (threadIdx.x & 63) == 0) {       \
      const long long now__ = clock64();                                       \
      prof[(threadIdx.x >> 6) * 8 + (slot)] += now__ - tprev;                  \
      tprev = now__;                                                           \
    }                                                                          \
  } while (0)

// ------------------------------------------------------------------------------------------------
// QK rule.  Rnn, Z contiguous [B*H,N,N]; q, k, cam_q, cam_k strided.  ngroups > 1: cam_q goes to `qpart`
// [ngroups][B*H][N][64] unscaled (qk_finish_kernel folds the groups); cam_k of a group is complete.
// ------------------------------------------------------------------------------------------------
// MODE BWD: Rnn = d_attn, Z = attn; the S tile is the softmax backward d_s = attn .(d_attn - rowdot) * scale with
// rowdot[i] = sum_j d_attn[i,j] attn[i,j] (single key group only: the row sum needs every key), outputs are the raw
// products d_q = d_s k and d_k = d_s^T q.
template <int MODE>
__global__ __launch_bounds__(kT) void qk_rule_kernel(
    const float* __restrict__ Rnn, const float* __restrict__ Z, const float* __restrict__ q, Strided qs,
    const float* __restrict__ k, Strided ks, float* __restrict__ cam_q, Strided cqs, float* __restrict__ cam_k,
    Strided cks, float* __restrict__ qpart, int H, int N, int BH, int JG, int ngroups, float scale,
    long long* __restrict__ prof, const float* __restrict__ r_scale, int64_t r_scale_stride) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  long long tprev = prof ? clock64() : 0;
  float* KtT = smem;                   // [64][QLD]  k of this group TRANSPOSED (row-side B operand, K = key contiguous)
  float* Qt = KtT + 64 * QLD;          // [TI][SLD]  q tile (column-side B operand; the rule's own factor of cam_q)
  float* Wt = Qt + TI * SLD;           // [TI][QLD]  the S tile: row-side A operand (16-B fragments along the keys),
                                       //            column-side A operand (4-byte fragments down the rows)
  float* Pt = Wt + TI * QLD;           // BWD only: [TI][64] per-float4 partial dots, then [TI] row dots
  const int bh = blockIdx.x % BH, g = blockIdx.x / BH;
  const int b = bh / H, h = bh % H;
  const int j0 = g * JG, nj = min(JG, N - j0), nj32 = (nj + 31) & ~31, njb = nj32 >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, lr = lane & 31, kh = lane >> 5;
  const float* r_bh = Rnn + (int64_t)bh * N * N + j0;
  const float* z_bh = Z + (int64_t)bh * N * N + j0;
  const float* q_bh = q + (int64_t)b * qs.sb + (int64_t)h * qs.sh;
  const float* k_bh = k + (int64_t)b * ks.sb + (int64_t)h * ks.sh + (int64_t)j0 * ks.sn;
  const int ntiles = (N + TI - 1) / TI;
  const WideMap wm = wide_map(64);
  const FastMap fm = fast_map(64, nj32, nj);
  const int srow = threadIdx.x >> 4, sc = threadIdx.x & 15;

  WideTile tr, tz;                              // raw (fast_load) until the tile is consumed
  f32x4 qq = {0.f, 0.f, 0.f, 0.f};
  // part p = 0..8 of tile `it`: the four float4 slots of the R tile, of the Z tile, then the q float4
  // (branch-free: rows beyond N re-read the tile's last row and are zeroed when the tile is consumed)
  auto fetch_part = [&](int it, int p) __attribute__((always_inline)) {
    const int i0 = it * TI, rows_valid = min(TI, N - i0);
    if (p < 4) {
      if (!fm.fast) tr.v[p] = load_wide_slot(wm, p, r_bh + (int64_t)i0 * N, N, rows_valid, nj);
      else if (p * kT < fm.nslots) tr.v[p] = fast_load(fm, p, r_bh, i0, N, rows_valid);
    } else if (p < 8) {
      if (!fm.fast) tz.v[p - 4] = load_wide_slot(wm, p - 4, z_bh + (int64_t)i0 * N, N, rows_valid, nj);
      else if ((p - 4) * kT < fm.nslots) tz.v[p - 4] = fast_load(fm, p - 4, z_bh, i0, N, rows_valid);
    } else {
      qq = *reinterpret_cast<const f32x4_u*>(q_bh + ((unsigned)(i0 + min(srow, rows_valid - 1)) * (unsigned)qs.sn + (unsigned)(sc << 2)));
    }
  };
#pragma unroll
  for (int p = 0; p < 9; ++p) fetch_part(0, p);
  p_stage_keys_T(KtT, k_bh, ks.sn, nj, nj32);        // (after the requests of tile 0: one HBM round trip for both)
  f32x16 acck[2];
  zero16(acck[0]);
  zero16(acck[1]);
  // cam_q: eight 16x16 output blocks of the [32][64] tile, one per wave
  const int ib = wave >> 2, db = wave & 3, l15 = lane & 15, kq = lane >> 4;
  for (int it = 0; it < ntiles; ++it) {
    const int i0 = it * TI;
    TE_MARK(0);
    __syncthreads();
    TE_MARK(1);
    {
      const int rows_valid = min(TI, N - i0);
      if (fm.fast && !(fm.plain && rows_valid == TI)) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          tr.v[r] = fast_fix(fm, r, tr.v[r], nj, rows_valid);
          tz.v[r] = fast_fix(fm, r, tz.v[r], nj, rows_valid);
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) qq[e] = (srow < rows_valid) ? qq[e] : 0.0f;
    }
    if constexpr (MODE == RULE) {
      if (r_scale != nullptr) {            // deferred per-sample factor of the broadcast-mask Add (BERT.py:386-388)
        const float f = r_scale[(int64_t)b * r_scale_stride];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int e = 0; e < 4; ++e) tr.v[r][e] = tr.v[r][e] * f;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) tr.v[r][e] = te_sd(tr.v[r][e], tz.v[r][e]);   // zero-filled slots: sd(0, 0) = 0
    } else {
      // rowdot: per-float4 partials -> LDS, 16 lanes per row fold them in a fixed order
      const int per_row = nj32 >> 2;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (wm.row[r] >= 0) {
          float p = 0.0f;
#pragma unroll
          for (int e = 0; e < 4; ++e) p = fmaf(tr.v[r][e], tz.v[r][e], p);
          Pt[wm.row[r] * 64 + wm.c4[r]] = p;
        }
      __syncthreads();
      {
        float part = 0.0f;
#pragma unroll
        for (int m = 0; m < 4; ++m)
          if (sc + 16 * m < per_row) part = part + Pt[srow * 64 + sc + 16 * m];
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) part = part + __shfl_xor(part, off, 64);
        __syncthreads();                       // every partial has been read
        if (sc == 0) Pt[srow] = part;
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (wm.row[r] >= 0) {
          const float rd = Pt[wm.row[r]];
#pragma unroll
          for (int e = 0; e < 4; ++e) tr.v[r][e] = (tz.v[r][e] * (tr.v[r][e] - rd)) * scale;   // zero-filled: 0
        }
    }
    p_store_wide(Wt, wm, tr, QLD);
    *reinterpret_cast<f32x4*>(Qt + srow * SLD + (sc << 2)) = qq;
    TE_MARK(2);
    __syncthreads();
    TE_MARK(3);
    // column side first: the nine loads of the next tile go out one per MFMA group (two with the first)
    const bool more = it + 1 < ntiles;
    p_col_product<QLD>(acck, Wt + kh * QLD + lr, Qt + kh * SLD + lr, wave, 2 * njb, (min(TI, N - i0) + 7) >> 3, [&](int g) __attribute__((always_inline)) {
      if (more) {
        fetch_part(it + 1, g);
        if (g == 7) fetch_part(it + 1, 8);
      }
    });
    TE_MARK(4);
    {
      // cam_q block (ib, db) = S[16 x keys] k[keys x 16]
      f32x4 cq = {0.f, 0.f, 0.f, 0.f};
      const int arow = ib * 16 + l15, dcol = db * 16 + l15;
      p_row_product16(cq, Wt + arow * QLD + 4 * kq, KtT + dcol * QLD + 4 * kq, (nj + 15) >> 4);
      TE_MARK(5);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int il = ib * 16 + kq * 4 + r;
        if (i0 + il < N) {
          if (ngroups == 1) {
            cam_q[(int64_t)b * cqs.sb + (int64_t)h * cqs.sh + (int64_t)(i0 + il) * cqs.sn + dcol] =
                (MODE == RULE) ? (Qt[il * SLD + dcol] * cq[r]) * scale : cq[r];
          } else {
            qpart[(((int64_t)g * BH + bh) * N + i0 + il) * 64 + dcol] = cq[r];
          }
        }
      }
    }
    TE_MARK(6);
  }
  float* o_bh = cam_k + (int64_t)b * cks.sb + (int64_t)h * cks.sh + (int64_t)j0 * cks.sn;
  p_col_epilogue<MODE == BWD>(acck, k_bh, ks.sn, o_bh, cks.sn, nj, wave, lr, kh, 2 * njb, scale);
}

// cam_q[i,d] = q[i,d] * (sum over groups of qpart[g][bh][i][d], in group order) * scale
__global__ __launch_bounds__(256) void qk_finish_kernel(const float* __restrict__ qpart, const float* __restrict__ q,
                                                        Strided qs, float* __restrict__ cam_q, Strided cqs, int H, int N,
                                                        int BH, int ngroups, float scale) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;      // float4 index into [BH][N][16]
  if (idx >= (int64_t)BH * N * 16) return;
  const int c = (int)(idx & 15);
  const int64_t row = idx >> 4;
  const int i = (int)(row % N), bh = (int)(row / N), b = bh / H, h = bh % H;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  for (int g = 0; g < ngroups; ++g) {
    const f32x4 p = *reinterpret_cast<const f32x4*>(qpart + (((int64_t)g * BH + bh) * N + i) * 64 + (c << 2));
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = s[e] + p[e];
  }
  const f32x4 qv = *reinterpret_cast<const f32x4_u*>(q + (int64_t)b * qs.sb + (int64_t)h * qs.sh + (int64_t)i * qs.sn + (c << 2));
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = (qv[e] * s[e]) * scale;
  *reinterpret_cast<f32x4_u*>(cam_q + (int64_t)b * cqs.sb + (int64_t)h * cqs.sh + (int64_t)i * cqs.sn + (c << 2)) = o;
}

inline size_t lds_qk(int /*jg*/, bool bwd) {                                                          // 106 (114) KB
  return (size_t)(64 * QLD + TI * SLD + TI * QLD + (bwd ? TI * 64 : 0)) * sizeof(float);
}

// Keys per workgroup: 256 (one 112-136 KB workgroup per CU).  Groups of 128 keys (64-72 KB: two workgroups per CU) were
// measured SLOWER on the MI355X (ViT-B B=64: AV 202 vs 170 us, QK 319 vs 257 us; N = 577 / 512 alike): the time of a
// row tile is dominated by per-tile costs that do not shrink with the tile, so halving the keys
// doubles them.
inline void groups_for(int64_t N, int& ng, int& jg) {
  ng = (int)((N + 255) / 256);
  jg = (int)(((N + ng - 1) / ng + 63) & ~(int64_t)63);      // equal groups, whole 64-key units (the LDS row stride)
}

template <typename K>
inline void allow_lds(K kern, size_t bytes) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace

bool supported(int64_t B, int64_t H, int64_t N, int64_t D) {
  int ng, jg;
  groups_for(N, ng, jg);
  // (32-bit offsets inside a (b, h) view: N <= 4096 and, asked of the rule's q by the dispatch, a row stride <= 2^16 floats)
  return D == 64 && N >= 1 && N <= 4096 && B * H * ng <= 0x7fffffff;
}

// mode RULE: the QK rule (Rnn = relevance of the scores, Z = the cached unscaled q k^T; qpart: [ng][B*H][N][64] floats when
// ng > 1).  mode BWD: softmax backward (Rnn = d_attn, Z = attn; cam_q / cam_k receive d_q / d_k) -- one key group only.
int qk_launch(int mode, const float* Rnn, const float* q, Strided qs, const float* k, Strided ks, const float* Z, float* cam_q,
              Strided cqs, float* cam_k, Strided cks, int64_t B, int64_t H, int64_t N, float scale, float* qpart, const float* r_scale,
              int64_t r_scale_stride, hipStream_t stream) {
  int ng, jg;
  groups_for(N, ng, jg);
  const int BH = (int)(B * H);
  const dim3 grid((unsigned)(BH * ng)), blk(kT);
  if (mode == RULE) {
    allow_lds(qk_rule_kernel<RULE>, lds_qk(256, false));
    qk_rule_kernel<RULE><<<grid, blk, lds_qk(jg, false), stream>>>(Rnn, Z, q, qs, k, ks, cam_q, cqs, cam_k, cks, qpart, (int)H, (int)N, BH,
                                                                  jg, ng, scale, nullptr, r_scale, r_scale_stride);
    if (ng > 1) {
      const int64_t n4 = (int64_t)BH * N * 16;
      qk_finish_kernel<<<dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream>>>(qpart, q, qs, cam_q, cqs, (int)H, (int)N, BH, ng,
                                                                                    scale);
    }
    return TE_OK;
  }
  if (ng != 1) return TE_ERR_UNSUPPORTED;      // the softmax backward needs every key of a row in one group
  allow_lds(qk_rule_kernel<BWD>, lds_qk(256, true));
  qk_rule_kernel<BWD><<<grid, blk, lds_qk(jg, true), stream>>>(Rnn, Z, q, qs, k, ks, cam_q, cqs, cam_k, cks, nullptr, (int)H, (int)N, BH, jg,
                                                              1, scale, nullptr, nullptr, 0);
  return TE_OK;
}

}  // namespace te_attn_rules
