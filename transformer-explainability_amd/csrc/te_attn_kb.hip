// te_attn_kb.hip -- attention relprop rules (modules/layers_ours.py:48-60,122-127 via ViT_LRP.py:154-177, BERT.py:367-393) and
// the attention-gradient producers on the same machinery, with WAVE-OWNED KEY BLOCKS (round 5).
//
// The one-pass kernels of te_attn_rules.hip move every [32, keys] tile of an N x N operand global -> registers -> LDS ->
// registers, all eight waves of the workgroup in lock-step through load / form-S / barrier / product / barrier phases:
// 15-23 vector instructions per MFMA, 45 % of a tile's cycles in MFMAs, 0.26-0.37 of the roofline for three rounds.
// Here the N x N operand NEVER touches LDS:
//
//   * wave w owns key block jb (32 keys) of its (b, h [, key group]) for the whole kernel.  A [32 rows x 32 keys] block of the
//     N x N operand arrives as four 16-byte-per-lane buffer loads (eight rows x 128 contiguous bytes each), requested two
//     tiles ahead, and changes to the MFMA ACCUMULATOR layout -- lane (lr, kh) holds column lr, rows
//     crow(e, kh) = (e & 3) + 8 (e >> 2) + 4 kh, e < 16 -- through a wave-private 4.6 KB LDS block (no barrier: a wave's LDS
//     instructions execute in order).  Because the contraction index of an MFMA may be visited in any order, that very
//     register set IS
//       - the A operand of the column-side product (K = query rows in accumulator order),
//       - the element-wise factor of the row-side result (cam_attn = attn . G lands in the same layout), and
//       - (back through the staging block) the layout the N x N result is stored from, as 16-byte pieces.
//   * the key-side operand of the row product (v of the wave's 32 keys) lives in registers for the whole kernel; only the
//     [32, 64] row-side tile (S = sd(R, Z), or d_out) is shared: THREE LDS buffers and an LDS arrival counter instead of a
//     barrier per tile -- no wave ever waits for another wave's MFMAs.
//   * the products run on bf16 MFMAs with every fp32 operand split into three bf16 planes, six partial products, fp32
//     accumulation (fp32 MFMA runs at the fp32 vector rate and its time ADDS to the vector work of the SIMD).
//   * global loads and stores of the tile loop are inline asm hipcc's s_waitcnt insertion does not see, waited for with
//     hand-counted vmcnt; a register with such a load in flight must never be copied -- register sets alternate over a
//     two-tile loop body, and scripts/check_hidden_loads.py (tests/test_isa_hazards.py) checks the compiled ISA for it.
//   DESIGN.md, "Attention rules with wave-owned key blocks", has the measurements behind each of these choices.
//
// Reductions run in an order that depends on N only: a batch equals its samples run one by one, bit for bit.
#include <type_traits>

#include "te_buffer.h"
#include "te_internal.h"
#include "te_x6.h"

namespace te_attn_kb {

namespace {

constexpr int TI = 32;         // query rows per tile
constexpr int kT = 512;        // threads per workgroup
constexpr int kWaves = kT / 64;
constexpr int XLD = 36;        // row stride (floats) of a wave's [32][32] staging block

enum { RULE = 0, BWD = 1 };

// (te_buffer.h: the descriptor, the plain and the hidden loads / stores of the tile loop and why they are hidden)

// ------------------------------------------------------------------------------------------------
// AV rule (MODE RULE):  S = sd(R, Z) [N,64];  cam_attn = attn . (S v^T) * scale;  cam_v = v . (attn^T S) * scale
// attention backward, first half (MODE BWD):  d_attn = d_out v^T;  d_v = attn^T d_out          (R = d_out, Z unused)
// R, Z strided [B,H,N,64]; attn, cam_attn contiguous [B*H,N,N]; v, cam_v strided.
// grid = BH * ngroups (bh fastest); workgroup g of a (b, h) owns key blocks [g KBG, (g + 1) KBG), wave w block g KBG + w.
//
// The products run on bf16 MFMAs at fp32 accuracy ("x6", te_x6.h): every fp32 operand is the exact sum of three
// bf16 planes, the six partial products above 2^-24 are kept (a1 b1 + a0 b2 + a2 b0 + a0 b1 + a1 b0 + a0 b0, smallest first),
// fp32 accumulation.  Why: v_mfma_f32_32x32x2_f32 runs at the fp32 VECTOR rate and its time ADDS to the vector-ALU time of
// the SIMD's waves (per-wave phase profile of the round-5 fp32-MFMA version of this kernel,
// profiles/r05_attention_av_kb_phase_profile.log: MFMA blocks at full rate, every other phase 2-3x longer while the partner
// wave multiplies; tile = 8 200 MFMA cycles + ~4 000 others), while the bf16 matrix pipe is a separate unit: 48 MFMAs of
// 32 cycles per tile and wave instead of 64 of 64, beside ~300 vector instructions (sd, the three-way splits, the result's
// factor).
//   row product   G = S v^T:  A = S planes [row][d] from LDS (16-byte fragments, K = d in four steps of 16), B = v planes of
//                 the wave's 32 keys, resident in 48 registers
//   column product  cam_v += attn^T S:  A = the attn block's planes, split in registers from the accumulator-layout values
//                 (K step s covers rows crow(8 s .. 8 s + 7, kh): the contraction order is free), B = S planes TRANSPOSED
//                 [d][row position] from LDS, the row positions permuted to that order (pos = row with bits 2 and 3 swapped)
// The S producer (all 512 threads, one float4 each) writes both plane images of its tile.
// ------------------------------------------------------------------------------------------------
// (te_x6.h: split3_pk, planes_of8, mfma_x6)

constexpr int kRLD = 144;                  // bytes per row of a row-major S plane [32 rows][64 d] (128 + 16: conflict-free b128)
constexpr int kTLD = 80;                   // bytes per row of a transposed S plane [64 d][32 row positions] (64 + 16)
constexpr int kPlR = TI * kRLD;            // 4 608
constexpr int kPlT = 64 * kTLD;            // 5 120
constexpr int kSBuf = 3 * kPlR + 3 * kPlT; // 29 184 bytes per S tile: both images, three planes each

template <int MODE>
__global__ __launch_bounds__(kT) void av6_kb_kernel(
    const float* __restrict__ R, Strided rs, const float* __restrict__ Z, Strided zs, const float* __restrict__ attn,
    const float* __restrict__ v, Strided vs, float* __restrict__ cam_attn, float* __restrict__ cam_v, Strided cs, int H,
    int N, int BH, int KBG, float scale) {
  // Row-side tiles in LDS: THREE buffers and an arrival counter instead of a barrier per tile.  S(k) lives in buffer k % 3; a
  // wave that has written its part of S(k) adds 1 to `arrived` (LDS operations of a wave execute in order: the add follows
  // its write); S(k) is complete at 8 (k + 1).  In iteration it every wave first waits for S(it) -- complete since the other
  // waves' previous iteration, so the poll normally falls through -- then writes its part of S(it + 1) over S(it - 2), whose
  // last readers (the MFMAs of iteration it - 2) every wave finished before it contributed to S(it).  No wave ever waits for
  // another wave's MFMAs: measured with s_barrier per tile (profiles/r05_attention_av_kb_phase_profile.log), the older wave
  // of a SIMD ran its 64 MFMAs at full rate, the younger one's only started when those had finished (issue arbitration
  // prefers the older wave, whose dependent MFMA is always ready), and then BOTH waited at the barrier and formed the next S
  // with the matrix pipe idle: 12 500 cycles per tile for 8 200 cycles of MFMAs.
  __shared__ __attribute__((aligned(16))) unsigned char Sb[3][kSBuf];
  // Wave-private staging of the wave's [32 rows x 32 keys] blocks: the N x N operand is read and the N x N result written as
  // 16-byte pieces per lane -- lane l moves keys 4 (l & 7) .. + 3 of row 8 p + (l >> 3), four instructions per block, each
  // covering eight rows x 128 contiguous bytes -- and changes to / from the accumulator layout through LDS (no barrier: a
  // wave's LDS instructions execute in order).  Measured (profiles/r05_attention_av_kb_study.log): with one dword per lane
  // and instruction (16 + 16 instructions per block) the stores alone cost 57 of the kernel's 130 us at N = 197.
  __shared__ __attribute__((aligned(16))) float Xw[kWaves][TI * XLD];
  __shared__ unsigned arrived;
  if (threadIdx.x == 0) arrived = 0;
  __syncthreads();
  const int bh = blockIdx.x % BH, g = blockIdx.x / BH;
  const int b = bh / H, h = bh - b * H;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, lr = lane & 31, kh = lane >> 5;
  const int nkb = (N + 31) >> 5, kb = g * KBG + wave;
  const bool has_blk = wave < KBG && kb < nkb;            // wave-uniform
  const int j = kb * 32 + lr;                             // this lane's key
  const int ntiles = (N + TI - 1) / TI;
  const int srow = threadIdx.x >> 4, sc = threadIdx.x & 15;      // this thread's float4 of the [32][64] row-side tile
  const int spos = (srow & 0x13) | ((srow & 4) << 1) | ((srow & 8) >> 1);      // its row's position in the transposed image

  // Buffer descriptors of this (b, h)'s views: uniform base + ONE 32-bit per-lane byte offset per access (no 64-bit vector
  // address arithmetic).  The hardware range check on that offset does the edge handling: rows at or beyond N lie past the
  // end of a view, so their loads return 0 without touching memory (S = sd(0, 0) = 0: they contribute nothing) and their
  // stores are dropped -- which also makes every prefetch unconditional (a tile beyond the last one reads zeros).  Lanes
  // whose KEY is beyond N wrap into the next row of the N x N operands: finite values that only reach those lanes' own,
  // never stored, results.  (The scalar offset field is left at 0: it is not part of the range check.)
  const unsigned nn_bytes = (unsigned)N * (unsigned)N * 4u;
  const Rsrc a_rs = make_rsrc(attn + (int64_t)bh * N * N, nn_bytes);
  const Rsrc ca_rs = make_rsrc(cam_attn + (int64_t)bh * N * N, nn_bytes);
  const Rsrc r_rs = make_rsrc(R + (int64_t)b * rs.sb + (int64_t)h * rs.sh, view_bytes(N, rs.sn));
  const Rsrc z_rs = make_rsrc(MODE == RULE ? Z + (int64_t)b * zs.sb + (int64_t)h * zs.sh : R, MODE == RULE ? view_bytes(N, zs.sn) : 0u);
  const Rsrc v_rs = make_rsrc(v + (int64_t)b * vs.sb + (int64_t)h * vs.sh, view_bytes(N, vs.sn));
  const Rsrc cv_rs = make_rsrc(cam_v + (int64_t)b * cs.sb + (int64_t)h * cs.sh, view_bytes(N, cs.sn));
  const unsigned row_bytes = (unsigned)N * 4u;

  f32x4 rr = {0.f, 0.f, 0.f, 0.f}, zz = {0.f, 0.f, 0.f, 0.f};
  const unsigned r_off = ((unsigned)srow * (unsigned)rs.sn + 4u * sc) * 4u, z_off = ((unsigned)srow * (unsigned)zs.sn + 4u * sc) * 4u;
  const unsigned r_tile = (unsigned)TI * (unsigned)rs.sn * 4u, z_tile = (unsigned)TI * (unsigned)zs.sn * 4u;
  auto fetch_rz = [&](int it) __attribute__((always_inline)) {          // (any it: tiles beyond the last read zeros)
    ld128_hidden(rr, r_rs, r_off + (unsigned)it * r_tile);
    if constexpr (MODE == RULE) ld128_hidden(zz, z_rs, z_off + (unsigned)it * z_tile);
  };
  constexpr int kRz = (MODE == RULE) ? 2 : 1;
  auto pin_rz = [&]() __attribute__((always_inline)) {
    TE_PIN(rr);
    if constexpr (MODE == RULE) TE_PIN(zz);
  };
  // S(it) of this thread's four elements -> both plane images of buffer it % 3, then arrive
  auto put_s = [&](int it) __attribute__((always_inline)) {
    f32x4 s = rr;
    if constexpr (MODE == RULE) {
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] = te_sd(rr[e], zz[e]);       // rows beyond N: sd(0, 0) = 0
    }
    unsigned p01[3], p23[3];
    split3_pk(s[0], s[1], p01);
    split3_pk(s[2], s[3], p23);
    unsigned char* base = Sb[it % 3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      *reinterpret_cast<u32x2*>(base + q * kPlR + srow * kRLD + sc * 8) = u32x2{p01[q], p23[q]};
      unsigned char* t = base + 3 * kPlR + q * kPlT + (4 * sc) * kTLD + spos * 2;
      *reinterpret_cast<unsigned short*>(t) = (unsigned short)(p01[q] & 0xffffu);
      *reinterpret_cast<unsigned short*>(t + kTLD) = (unsigned short)(p01[q] >> 16);
      *reinterpret_cast<unsigned short*>(t + 2 * kTLD) = (unsigned short)(p23[q] & 0xffffu);
      *reinterpret_cast<unsigned short*>(t + 3 * kTLD) = (unsigned short)(p23[q] >> 16);
    }
    // RELAXED atomics + compiler barriers, NOT release / acquire: data and counter both live in LDS, whose instructions a
    // wave executes in order, so the hardware needs nothing more -- while hipcc turns a workgroup-scope acquire (and a
    // __syncthreads()) into s_waitcnt vmcnt(0), i.e. a full drain of the wave's global-memory pipeline at every tile: the
    // prefetches just issued, two tiles ahead, and the stores (found in the ISA after the phase profile showed every wave
    // waiting ~2 500 cycles where it forms S: with the drain the kernel's time was memory time PLUS MFMA time)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the wave's LDS writes have been PERFORMED before it arrives: a
                                                            // later single-lane atomic can overtake the tail of a 64-lane write
    if (lane == 0) __hip_atomic_fetch_add(&arrived, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  };
  auto wait_s = [&](int it) __attribute__((always_inline)) {            // S(it) complete
    const unsigned target = (unsigned)kWaves * (unsigned)(it + 1);
    while (__builtin_amdgcn_readfirstlane(__hip_atomic_load(&arrived, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) < target)
      __builtin_amdgcn_s_sleep(1);
    asm volatile("" ::: "memory");
  };

  if (!has_blk) {
    fetch_rz(0);
    TE_VM_WAIT(0);
    pin_rz();
    put_s(0);
    fetch_rz(1);
    for (int it = 0; it < ntiles; ++it) {
      wait_s(it);                                  // (throttle: S(it + 1) overwrites S(it - 2))
      TE_VM_WAIT(0);
      pin_rz();
      put_s(it + 1);
      fetch_rz(it + 2);
    }
    TE_VM_WAIT(0);
    return;
  }

  // key-side operand of the row product, resident: the planes of v[j][16 s + 8 kh + 0..7], s = 0..3 (keys beyond N: zeros)
  bf16x8 vpl[4][3];
  {
    const unsigned off = ((unsigned)j * (unsigned)vs.sn + 8u * kh) * 4u;
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      const f32x4 lo = ld128(v_rs, off + 64u * s4), hi = ld128(v_rs, off + 64u * s4 + 16u);
      const float x[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      planes_of8(x, vpl[s4]);
    }
  }
  float* const Xb = Xw[wave];
  const int xr = lane >> 3, xc = (lane & 7) << 2;                  // this lane's row (+ 8 p) and first key of a 16-byte piece
  const unsigned lane_x4 = ((unsigned)xr * (unsigned)N + (unsigned)(kb * 32 + xc)) * 4u;
  const unsigned lane_nn = ((unsigned)(4 * kh) * (unsigned)N + (unsigned)j) * 4u;
  const bool key_ok = j < N;
  const bool blk_full = kb * 32 + 32 <= N;         // wave-uniform: every key of the block exists (else: dword stores, masked)
  auto fetch_attn = [&](int it, f32x4 (&dst)[4]) __attribute__((always_inline)) {
    const unsigned base = (unsigned)(it * TI) * row_bytes;
#pragma unroll
    for (int p = 0; p < 4; ++p) ld128_hidden(dst[p], a_rs, lane_x4 + (base + (unsigned)(8 * p) * row_bytes));
  };
  auto to_acc = [&](const f32x4 (&src)[4], float (&dst)[16]) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < 4; ++p) *reinterpret_cast<f32x4*>(Xb + (8 * p + xr) * XLD + xc) = src[p];
#pragma unroll
    for (int e = 0; e < 16; ++e) dst[e] = Xb[crow(e, kh) * XLD + lr];
  };

  float ac[16];
  f32x4 an[4], an2[4];
  fetch_rz(0);
  fetch_attn(0, an2);
  TE_VM_WAIT(0);                                   // (prologue: hipcc's own loads of v above included)
  pin_rz();
#pragma unroll
  for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
    for (int q = 0; q < 3; ++q) TE_PIN(vpl[s4][q]);
#pragma unroll
  for (int p = 0; p < 4; ++p) TE_PIN(an2[p]);
  put_s(0);
  fetch_rz(1);
  fetch_attn(1, an);
  to_acc(an2, ac);
  // In flight when the loop starts, oldest first: R / Z(1), attn(1).  Every iteration issues R / Z(it + 2), attn(it + 2) at
  // its top and the stores of its own result at its end.

  f32x16 accv[2];
  zero16(accv[0]);
  zero16(accv[1]);
  auto tile = [&](int it, f32x4 (&ax)[4], f32x4 (&ay)[4]) __attribute__((always_inline)) {
    const unsigned char* Sc = Sb[it % 3];
    wait_s(it);
    TE_VM_WAIT(4);                                 // R / Z(it + 1): younger loads in flight = attn(it + 1)
    pin_rz();
    put_s(it + 1);
    fetch_rz(it + 2);
    fetch_attn(it + 2, ax);
    __builtin_amdgcn_sched_barrier(0);
    if (it < ntiles) {                             // (the pair loop runs one tile beyond an odd tile count: no products there)
      // ---- row side: G = S v^T for this wave's key block ----
      f32x16 gacc;
      zero16(gacc);
      {
        const unsigned char* Ab = Sc + lr * kRLD + 16 * kh;
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
          bf16x8 a[3];
#pragma unroll
          for (int q = 0; q < 3; ++q) a[q] = *reinterpret_cast<const bf16x8*>(Ab + q * kPlR + 32 * s4);
          mfma_x6(gacc, a, vpl[s4]);
        }
      }
      // ---- the N x N result of this tile: cam_attn = attn . G straight from the accumulators, to rows through LDS, stored as
      // 16-byte pieces (full key blocks), else dword stores masked by key ----
      float gp[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) gp[e] = (MODE == RULE) ? (ac[e] * gacc[e]) * scale : gacc[e];
      const unsigned base = (unsigned)(it * TI) * row_bytes;
      if (blk_full) {
#pragma unroll
        for (int e = 0; e < 16; ++e) Xb[crow(e, kh) * XLD + lr] = gp[e];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const f32x4 t = *reinterpret_cast<const f32x4*>(Xb + (8 * p + xr) * XLD + xc);
          st128_hidden(t, ca_rs, lane_x4 + (base + (unsigned)(8 * p) * row_bytes));
        }
      } else if (key_ok) {
#pragma unroll
        for (int e = 0; e < 16; ++e) st32_hidden(gp[e], ca_rs, lane_nn + (base + (unsigned)((e & 3) + 8 * (e >> 2)) * row_bytes));
      }
      // ---- column side: cam_v += attn^T S (keys x 64); K step s = rows crow(8 s .. 8 s + 7, kh) ----
      bf16x8 apl[2][3];
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const float x[8] = {ac[8 * s2], ac[8 * s2 + 1], ac[8 * s2 + 2], ac[8 * s2 + 3],
                            ac[8 * s2 + 4], ac[8 * s2 + 5], ac[8 * s2 + 6], ac[8 * s2 + 7]};
        planes_of8(x, apl[s2]);
      }
#pragma unroll
      for (int db = 0; db < 2; ++db) {
        const unsigned char* Bb = Sc + 3 * kPlR + (db * 32 + lr) * kTLD + 16 * kh;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          bf16x8 bq[3];
#pragma unroll
          for (int q = 0; q < 3; ++q) bq[q] = *reinterpret_cast<const bf16x8*>(Bb + q * kPlT + 32 * s2);
          mfma_x6(accv[db], apl[s2], bq);
        }
      }
    }
    // attn(it + 1) was requested a tile ago; younger loads in flight: R / Z(it + 2) and attn(it + 2) of this tile
    if constexpr (kRz == 2) TE_VM_WAIT(6);
    else TE_VM_WAIT(5);
#pragma unroll
    for (int p = 0; p < 4; ++p) TE_PIN(ay[p]);
    to_acc(ay, ac);                                // the next tile's attn block (the staging block is free: its rows were read)
  };
#pragma unroll 1
  for (int it = 0; it < ntiles; it += 2) {
    tile(it, an2, an);
    tile(it + 1, an, an2);
  }
  TE_VM_WAIT(0);                                   // (requests beyond the last tile: zeros, but their registers are in flight)

  // ---- column epilogue: accv[db][e] = (attn^T S)[key = 32 kb + crow(e, kh)][d = 32 db + lr]; keys beyond N: dropped ----
#pragma unroll
  for (int db = 0; db < 2; ++db) {
    const unsigned d4 = (unsigned)(db * 32 + lr) * 4u;
    float x[16];
    if constexpr (MODE == RULE) {
      const unsigned xoff = (unsigned)(kb * 32 + 4 * kh) * (unsigned)vs.sn * 4u + d4;
#pragma unroll
      for (int e = 0; e < 16; ++e) x[e] = ld32(v_rs, xoff + (unsigned)((e & 3) + 8 * (e >> 2)) * (unsigned)vs.sn * 4u);
    }
    const unsigned ooff = (unsigned)(kb * 32 + 4 * kh) * (unsigned)cs.sn * 4u + d4;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      float val = accv[db][e];
      if constexpr (MODE == RULE) val = (x[e] * val) * scale;
      st32(val, cv_rs, ooff + (unsigned)((e & 3) + 8 * (e >> 2)) * (unsigned)cs.sn * 4u);
    }
  }
}

// key blocks per workgroup: at most eight (one per wave), the blocks of a (b, h) spread evenly over ceil(nkb / 8) workgroups
inline void groups_for(int64_t N, int& ng, int& kbg) {
  const int nkb = (int)((N + 31) / 32);
  ng = (nkb + kWaves - 1) / kWaves;
  kbg = (nkb + ng - 1) / ng;
}

}  // namespace

bool supported(int64_t B, int64_t H, int64_t N, int64_t D) {
  int ng, kbg;
  groups_for(N, ng, kbg);
  // (32-bit offsets inside a (b, h) view: N <= 4096 and, checked by the launchers, a row stride <= 2^16 floats)
  return D == 64 && N >= 1 && N <= 4096 && B * H * ng <= 0x7fffffff;
}

// mode 0: the AV rule; mode 1: d_attn / d_v of the attention backward (R = d_out, Z ignored, scale ignored)
int av_launch(int mode, const float* R, Strided rs, const float* attn, const float* v, Strided vs, const float* Z, Strided zs,
              float* cam_attn, float* cam_v, Strided cs, int64_t B, int64_t H, int64_t N, float scale, hipStream_t stream) {
  int ng, kbg;
  groups_for(N, ng, kbg);
  const int BH = (int)(B * H);
  // 32-bit row offsets inside a (b, h) view, and the hardware range check that drops the rows >= N of a partial key block needs
  // a row stride of at least the 64 floats a row holds: every strided view of the launch
  auto stride_ok = [](int64_t sn) { return sn >= 64 && sn <= 65536; };
  if (!stride_ok(rs.sn) || !stride_ok(vs.sn) || !stride_ok(cs.sn) || (mode == 0 && !stride_ok(zs.sn))) return TE_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)(BH * ng)), blk(kT);
  if (mode == 0)
    av6_kb_kernel<RULE><<<grid, blk, 0, stream>>>(R, rs, Z, zs, attn, v, vs, cam_attn, cam_v, cs, (int)H, (int)N, BH, kbg, scale);
  else
    av6_kb_kernel<BWD><<<grid, blk, 0, stream>>>(R, rs, nullptr, Strided{0, 0, 0}, attn, v, vs, cam_attn, cam_v, cs, (int)H,
                                                 (int)N, BH, kbg, 1.0f);
  return TE_OK;
}

}  // namespace te_attn_kb
