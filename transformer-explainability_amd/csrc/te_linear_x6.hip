// te_linear_x6.hip -- Linear.relprop (modules/layers_ours.py:207-230, variant "ours", alpha = 1, Z from the cached
// forward output) with its three GEMM-shaped products on bf16 MFMAs at fp32 accuracy.
//
// An fp32 number is exactly the sum of three bf16 numbers, a = a0 + a1 + a2 (8 + 8 + 8 significand bits), and a product
// of two bf16 values is exact in the fp32 accumulator of v_mfma_f32_32x32x16_bf16.  Of the nine partial products of
// a b the six above 2^-24 |a||b| are kept, smallest first:
//        a b  ~=  a1 b1 + a0 b2 + a2 b0 + a0 b1 + a1 b0 + a0 b0          ("x6": what is dropped is below fp32 rounding)
// so every product of the rule is an fp32-accumulated sum of exact terms -- at least as accurate against fp64 as the
// fp32-MFMA kernels of te_linear.hip (tests/test_gpu_rules.py::test_linear_x6_*).
//
// Round 3 design:
//   plane tensors   an fp32 [R, K] operand lives as bf16 planes in FRAGMENT-MAJOR order
//                        P3[R / 32][K / 16][3 planes][kh 2][r 32][8 bf16]          (1 KiB per plane fragment)
//                   i.e. exactly the image one wave needs as an MFMA operand of a 32-row block and one K16 step: one
//                   global_load_lds_dwordx4 (64 lanes x 16 B, fully coalesced 1 KiB) stages it, one ds_read_b128 per
//                   lane reads it back conflict-free.  The C-pass weights interleave W+^T and W-^T per block:
//                        P6[in / 32][out / 16][sign 2][3 planes][1 KiB].
//   weights         split ONCE per weight version (te_linear_x6_prepare_weights_f32; the host caches the planes)
//   |X| planes      te_linear_x6_split_abs_f32 (one streaming pass)
//   one GEMM kernel x6_kernel<WM, MODE>: the product is evaluated TRANSPOSED, D[w][t] (weight rows x activation rows),
//                   so a lane of the 32x32 accumulator block owns ONE activation row t and runs of four consecutive
//                   features: R / Y / X are read and the fp32 result is stored as 16-byte pieces, and the Z-pass writes
//                   S straight into the plane layout of the C-pass's operand (halves exchanged with
//                   v_permlane32_swap) -- S never exists in fp32.
//                   Tile = (128 WM) weight rows x 256 activation rows, 4 WM waves of 128 x 64 (eight 32x32 blocks, 48
//                   MFMAs per K16 step), two LDS stages filled by direct-to-LDS loads one step ahead, one barrier per
//                   step.  C-pass: the "weight rows" of a wave are (32 i) x {+, -} pairs, P+ and P- side by side.
//   schedule        persistent grid, SEQUENTIAL stream-K: the (tile, K-step) iteration space is cut into equal
//                   contiguous ranges, one per workgroup.  A tile cut in two is computed as ONE k-ordered chain: the
//                   workgroup holding its head (k = 0 ...) runs that fragment FIRST and publishes the accumulators
//                   (agent-scope release), the workgroup holding its tail runs it LAST, starting from those accumulators
//                   (agent-scope acquire).  Every output therefore sees the same fused-multiply-add chain wherever the cut
//                   falls: a batch equals its samples run one by one, bit for bit, and no tile quantisation is left (at
//                   ViT-B batch 64 the 256-wide tiles of the eight launches of a block fill 59-94 % of whole rounds).
//                   Waits only ever go to a LOWER workgroup index of the same XCD slot order.
//                   Where whole tiles cost little or no wall time (plan_x6: rounds x lock-step time against tiles per workgroup
//                   x skewed step time) the work is handed out in whole tiles instead: the workgroups of an XCD then walk k
//                   in lock-step on shared operand panels and a K16 step takes 2.0-2.3 us instead of 2.3-2.6 us; each takes
//                   the XCD's next tile from a counter until none is left (no hand-over, no wait on another workgroup).
//   plain GEMM      MODE_G: out = X W^T + b on the same loop (te_gemm_x6_f32: the Linear layers' own forward product and
//                   input gradient); te_linear_x6_split_dual_f32 writes the planes of a layer input and
//                   of its absolute value in one pass, so the rule reuses what the forward product split.
// Round 4:
//   geometries      WM = 2 / 1 / 0: 256 x 256, 128 x 256 and 128 x 128 tiles (X6Geo); the last for launches with few weight rows
//   other rules     variant lrp (layers_lrp.py:188-211) and alpha != 1 (layers_ours.py:225-228) as further epilogue modes of
//                   the same loop: MODE_ZI, MODE_Z1, MODE_CI, MODE_X (te_linear_relprop_x6_general_f32)
//   loud hand-over  a wait for another workgroup's accumulators is bounded (250 ms), sets a sticky status word, poisons the
//                   tile with NaN and makes every later wait give up at once: never a plausible wrong result, never a hang
//   main loop       raw s_barrier + counted s_waitcnt (a __syncthreads() drains direct-to-LDS loads), two LDS stages
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "te_x6.h"

namespace {

// (te_x6.h: TE_MFMA_BF16, kFrag = one plane fragment, the split -- split3_pk, split3 --, sd2, swap_halves, PA / PB)
constexpr int kRB = 3 * kFrag;                // one 32-row block, one K16 step
constexpr int kMinFrag = 4;                   // a cut closer than this many K-steps to a tile boundary snaps onto it
constexpr int kSpinMillis = 250;               // bounded wait for a predecessor's accumulators: never hang the GPU
constexpr int kErrWord = 1023;                 // flags[0 .. 767] = hand-over flags of a pass, flags[kErrWord] = its error word
constexpr int kClaimWord = 1024, kClaimStride = 32;   // flags[kClaimWord + 32 xcd] = next unclaimed tile of XCD xcd (a 128-B line each;
                                                      // beyond the words te_linear_relprop_x6_check reads: a used counter is no error)


// Z-pass, C-pass, plain GEMM out = B A^T + bias; round 4, for variant lrp and alpha != 1 (layers_lrp.py:188-211,
// layers_ours.py:225-228): MODE_ZI = the inhibitor's Z-pass of variant ours from the same product, Z' = ((Y - b) - |X||W|^T)/2
// = X+ W-^T + X- W+^T (exact k-ordered sum, exact_zi, where te_z_cancels(-Z', |X||W|^T, b_j): the two criteria of MODE_Z);
// MODE_Z1 = a one-sided Z-pass, S = sd(R, acc) (acc = X+ W+^T ...: same-sign terms, no cancellation);
// MODE_CI = the C-pass with the signs crossed, out += scale (X+ . (S W-) + X- . (S W+)); MODE_X = a product masked by one
// sign of X, out (+)= scale (X+- . acc).
// MODE_ZS = MODE_Z whose activation operand is the SIGNED planes of X (what the forward product read): |X| is formed while the
// planes are staged (x6_kernel: SGN), so no producer has to store a second plane set.
enum { MODE_Z = 0, MODE_C = 1, MODE_G = 2, MODE_ZI = 3, MODE_Z1 = 4, MODE_CI = 5, MODE_X = 6, MODE_ZS = 7 };

__device__ __forceinline__ float bf16_f32(unsigned b) { return __uint_as_float(b << 16); }

enum { OP_ABS = 0, OP_POS = 1, OP_NEG = 2, OP_ID = 3 };
template <int OP>
__device__ __forceinline__ float apply_op(float x) {
  if constexpr (OP == OP_ID) return x;
  if constexpr (OP == OP_ABS) return __int_as_float(__float_as_int(x) & 0x7fffffff);
  const int b = __float_as_int(x);
  if constexpr (OP == OP_POS) return __int_as_float(b > 0 ? b : 0);
  return __int_as_float(b < 0 ? b : 0);
}

// ------------------------------------------------------------------------------------------------
// fp32 -> planes.  One 256-thread block = 32 rows x 8 K16 steps; thread (r = t & 31, step = t >> 5) reads 16
// consecutive k of its row and writes the six 16-B pieces (3 planes x 2 k-halves) of its (row, step): a half-wave
// writes 512 contiguous bytes per store.  TRANSPOSE: element (r, k) is src[k * R + r] (W^T operands of the C-pass);
// the destination then is the P6 layout with `sign` selecting the W+ / W- half.
// ------------------------------------------------------------------------------------------------
// dst_abs (optional, OP_ID only): the planes of |src| as well, from the same pass -- the three planes of |x| are the planes
// of x times sign(x) exactly (bf16 rounding is sign-symmetric and every residual negates with x), and sign(x) is the
// sign bit of plane 0: clear it there, flip the low planes' sign bits where it was set.
template <int OP, bool TRANSPOSE>
__global__ __launch_bounds__(256) void split_kernel(const float* __restrict__ src, unsigned char* __restrict__ dst,
                                                    int64_t R, int64_t K, int group, int sign,
                                                    unsigned char* __restrict__ dst_abs = nullptr) {
  const int r = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int64_t rb = blockIdx.x;
  const int64_t ks = (int64_t)blockIdx.y * 8 + sl;
  const int64_t nks = K >> 4;
  if (ks >= nks) return;
  const int64_t row = rb * 32 + r;
  float v[16];
  if (row < R) {
    if constexpr (!TRANSPOSE) {
      const float* s = src + row * K + ks * 16;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(s + 4 * c);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * c + e] = q[e];
      }
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e) v[e] = src[(ks * 16 + e) * R + row];
    }
  } else {
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = 0.0f;
  }
  unsigned p[8][3];                    // [pair of consecutive k][plane]
#pragma unroll
  for (int e = 0; e < 8; ++e) split3_pk(apply_op<OP>(v[2 * e]), apply_op<OP>(v[2 * e + 1]), p[e]);
  unsigned char* d = dst + ((rb * nks + ks) * group + sign * 3) * kFrag + r * 16;
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      u32x4 w;
#pragma unroll
      for (int e = 0; e < 4; ++e) w[e] = p[4 * kh + e][q];
      *reinterpret_cast<u32x4*>(d + q * kFrag + kh * 512) = w;
    }
  if constexpr (OP == OP_ID) {
    if (dst_abs) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const unsigned m = p[e][0] & 0x80008000u;
        p[e][0] &= 0x7fff7fffu;
        // a zero residual is +0 whatever the sign of x (x - x = +0): flip the sign bit of non-zero halves only, so that
        // the planes are bit for bit those of split3(|x|).  (h & 0x7fff) + 0x7fff has bit 15 set iff the half is non-zero.
        p[e][1] ^= m & (((p[e][1] & 0x7fff7fffu) + 0x7fff7fffu) & 0x80008000u);
        p[e][2] ^= m & (((p[e][2] & 0x7fff7fffu) + 0x7fff7fffu) & 0x80008000u);
      }
      unsigned char* da = dst_abs + ((rb * nks + ks) * 3) * kFrag + r * 16;
#pragma unroll
      for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
          u32x4 w;
#pragma unroll
          for (int e = 0; e < 4; ++e) w[e] = p[4 * kh + e][q];
          *reinterpret_cast<u32x4*>(da + q * kFrag + kh * 512) = w;
        }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Producers that emit operand planes themselves (round 5): nn.GELU between the two Linear
// layers of an Mlp block (ViT_LRP.py:57-69, BERT.py: BertIntermediate).  Thread mapping and plane layout of split_kernel.
//   SRC_GELU_BWD  d_h = d_a . gelu'(h) goes straight into the planes of fc1's input-gradient product (te_gemm_x6_f32's
//                 x_planes): the fp32 d_h is never written or read (22 -> 14 B per element against the two passes it replaces)
//   SRC_GELU_FWD  a = gelu(h) is written as fp32 (the rule and the backward pass read it) AND as the signed planes of fc2's
//                 forward product plus the planes of |a| for fc2's rule (te_linear_x6_split_dual_f32's outputs, bit for bit)
// ------------------------------------------------------------------------------------------------
enum { SRC_GELU_BWD = 0, SRC_GELU_FWD = 1 };
// The elementwise work runs in a COALESCED mapping: a block's 32 rows x 128 k tile is read as 1024 float4 (a wave covers 512
// contiguous bytes of two rows per instruction, four values per thread and step -- the shape of the stand-alone gelu kernels),
// the results cross to split_kernel's (row, K16 step) mapping through LDS, and only the split and the plane stores run there
// (measured in round 5 against a kernel doing the erf / exp arithmetic on 16 values per thread behind row-strided loads:
// DESIGN.md section 6).
constexpr int kGsPitch = 132;               // floats per tile row in LDS: 128 + 4 (16-B reads of 32 rows hit every bank once)
template <int SRC>
__global__ __launch_bounds__(256) void gelu_split_lds_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                             float* __restrict__ y, unsigned char* __restrict__ dst,
                                                             unsigned char* __restrict__ dst_abs, int64_t R, int64_t K) {
  __shared__ __attribute__((aligned(16))) float tile[32 * kGsPitch];
  const int64_t rb = blockIdx.x;
  const int64_t k0 = (int64_t)blockIdx.y * 128;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = threadIdx.x + 256 * j;
    const int tr = i >> 5, c4 = i & 31;
    const int64_t row = rb * 32 + tr, col = k0 + 4 * c4;
    f32x4 o = {0.0f, 0.0f, 0.0f, 0.0f};
    if (row < R && col < K) {                        // (K % 16 == 0: a float4 never straddles the end of a row)
      const int64_t at = row * K + col;
      const f32x4 xv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(x + at));
      if constexpr (SRC == SRC_GELU_BWD) {
        const f32x4 gv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g + at));
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = te_gelu_grad(gv[e], xv[e]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = te_gelu(xv[e]);
        *reinterpret_cast<f32x4*>(y + at) = o;
      }
    }
    *reinterpret_cast<f32x4*>(&tile[tr * kGsPitch + 4 * c4]) = o;
  }
  __syncthreads();
  const int r = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int64_t ks = (int64_t)blockIdx.y * 8 + sl;
  const int64_t nks = K >> 4;
  if (ks >= nks) return;
  float v[16];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(&tile[r * kGsPitch + sl * 16 + 4 * c]);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[4 * c + e] = q[e];
  }
  unsigned p[8][3];
#pragma unroll
  for (int e = 0; e < 8; ++e) split3_pk(v[2 * e], v[2 * e + 1], p[e]);
  auto store = [&](unsigned char* d) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
        u32x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = p[4 * kh + e][q];
        *reinterpret_cast<u32x4*>(d + q * kFrag + kh * 512) = w;
      }
  };
  store(dst + ((rb * nks + ks) * 3) * kFrag + r * 16);
  if (SRC == SRC_GELU_FWD && dst_abs) {        // (dst_abs = NULL: the consumer's rule takes the signed planes)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const unsigned m = p[e][0] & 0x80008000u;
      p[e][0] &= 0x7fff7fffu;
      p[e][1] ^= m & (((p[e][1] & 0x7fff7fffu) + 0x7fff7fffu) & 0x80008000u);
      p[e][2] ^= m & (((p[e][2] & 0x7fff7fffu) + 0x7fff7fffu) & 0x80008000u);
    }
    store(dst_abs + ((rb * nks + ks) * 3) * kFrag + r * 16);
  }
}

__global__ __launch_bounds__(256) void zero_words_kernel(u32x4* __restrict__ p) {
  p[(size_t)blockIdx.x * 256 + threadIdx.x] = u32x4{0u, 0u, 0u, 0u};
}

// plain positive-part sum of one output element (the reference's Z), k-ordered: the cancellation fallback
__device__ __forceinline__ float exact_z(const float* __restrict__ x, const float* __restrict__ w, int64_t K) {
  float z1 = 0.0f, z2 = 0.0f;
  for (int64_t k = 0; k < K; ++k) {
    const float xv = x[k], wv = w[k];
    z1 = fmaf(fmaxf(xv, 0.0f), fmaxf(wv, 0.0f), z1);
    z2 = fmaf(fminf(xv, 0.0f), fminf(wv, 0.0f), z2);
  }
  return z1 + z2;
}

// the inhibitor's Z of variant ours, k-ordered: X+ W-^T + X- W+^T (layers_ours.py:226: f(nw, pw, px, nx))
__device__ __forceinline__ float exact_zi(const float* __restrict__ x, const float* __restrict__ w, int64_t K) {
  float z1 = 0.0f, z2 = 0.0f;
  for (int64_t k = 0; k < K; ++k) {
    const float xv = x[k], wv = w[k];
    z1 = fmaf(fmaxf(xv, 0.0f), fminf(wv, 0.0f), z1);
    z2 = fmaf(fminf(xv, 0.0f), fmaxf(wv, 0.0f), z2);
  }
  return z1 + z2;
}

struct X6Params {
  const unsigned char* A;      // weight-side planes: P3 of |W| (Z-pass) or P6 of W+^T / W-^T (C-pass)
  const unsigned char* B;      // activation-side planes (P3): |X| (Z-pass) or S (C-pass)
  int64_t a_group_stride;      // bytes between consecutive 32-row groups of A  = nks * (3 or 6) KiB
  int64_t b_rb_stride;         // bytes between consecutive 32-row blocks of B  = nks * 3 KiB
  int nks;                     // K / 16
  // pad0_ / pad1_: bytes no kernel reads, which keep every field at its offset in the kernel arguments.  Without them hipcc
  // merges the scalar loads of nks and ntm / ntn, allocates SGPRs differently and changes the spills of the 128 x 256 Z- and
  // C-pass kernels: a kernel change that would need its own same-box measurement.  The static_asserts on sizeof / offsetof
  // below x6_kernel pin the block.
  unsigned char pad0_[20];
  int ntm, ntn;                // tiles along the weight side / the activation side (set by launch_x6 from rows_w, T)
  int rows_w;                  // weight-side rows of the product: out_f (Z-pass, plain product), 2 in_f (C-pass: +/- pairs)
  int t_fast;                  // tile order inside the launch: 0 = weight side fastest, 1 = activation side fastest
  int whole_tiles;             // 1: ranges are cut at tile boundaries only (all workgroups of a round in k lock-step);
                               // 2: whole tiles, claimed from the XCD's counter instead of cut into static ranges
  int pad1_;
  int ncb;                     // 32-row blocks of the activation side = ceil(T / 32)
  int64_t T;
  int in_f, out_f;
  float* partial;              // [grid][threads][32] float4: accumulators of a cut tile
  unsigned* flags;             // [grid] hand-over flags, zero before the launch; [kErrWord] = error word of this pass
  unsigned* status;            // sticky error word (the caller's, else = flags + kErrWord): OR-ed, never cleared here
  long long spin_ticks;        // wall_clock64 ticks a workgroup waits for a predecessor before it gives up
  int drop_handover;           // TE_X6_TEST_DROP_HANDOVER: publishers keep their flag down (tests: a wait must expire)
  int small_grid;              // TE_X6_TEST_SMALL_GRID: 16 workgroups (tests: stream-K cuts on small shapes)
  int sched_flags;             // host side only: the call's TE_X6_WHOLE_TILES | TE_X6_SLACK_RULE | TE_X6_STATIC_TILES and geometry pin (plan_x6)
  // Z-pass epilogue
  const float* R;
  const float* Y;
  const float* bias;
  const float* X;              // fp32 operands: the cancellation fallback (Z) / the sign select (C)
  const float* W;
  unsigned char* S;            // out: P3 planes of S, rows = T, K = out_f
  const float* rs;             // optional per-sample factor on R
  int64_t rs_stride;
  int rps;
  // C-pass epilogue
  float* out;
  float scale;                 // MODE_C / MODE_CI / MODE_X: factor on the result (alpha, -beta)
  int accum;                   // MODE_X: 1 = add to what out holds (MODE_CI always does)
  int x_sign;                  // MODE_X: +1 = X+ masks the product, -1 = X-
};
// (round 6, measured and removed: requesting the NEXT tile's first stage before the epilogue, non-temporal epilogue accesses, and
// warm-up requests of the tile's R / Y lines during the last loop steps -- all neutral or negative, profiles/r06_x6_epilogue_study.log)

// a no-op four loaded vectors pass through.  Device pass only: a "v" constraint in the HOST pass of a kernel template silently
// drops the host stub of the instantiation.
#if defined(__HIP_DEVICE_COMPILE__)
#define X6_PASS4(a, b, c, d) asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d))
#else
#define X6_PASS4(a, b, c, d) (void)0
#endif

__device__ __forceinline__ void glds16(const unsigned char* src, unsigned char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// ------------------------------------------------------------------------------------------------
// Two LDS stages: stage ks + 1 lands while ks is multiplied (a third stage, prefetch distance 2, ran the C-pass 7 % slower:
// DESIGN.md 3.1b item 1, profiles/r04_x6_variants.log).
constexpr int kStages = 2;
// Tile geometry WM (weight rows x activation rows of a workgroup tile; waves as NWM x NWN, each MI x 2 blocks of 32 x 32):
//   2: 256 x 256, 2 x 4 waves of 128 x 64 (one 512-thread workgroup per CU)
//   1: 128 x 256, 1 x 4 waves of 128 x 64 (two 256-thread workgroups per CU)
//   0: 128 x 128, 2 x 2 waves of  64 x 64 (three 256-thread workgroups per CU, 168 VGPRs) -- round 4, for launches with
//      few weight rows (out_f = 768: 150 / 300 tiles of the larger geometries for 256 CUs): every output is ONE k-ordered
//      chain, so a tile takes K / 16 sequential steps whatever the schedule, and with one 4-wave workgroup on most CUs a
//      SIMD held a single wave (1.38 us per step of 48 MFMAs: half the pipe idle).  Smaller tiles = shorter steps, 594
//      tiles, three waves per SIMD to cover each other's LDS / barrier / fill latency.
template <int WM>
struct X6Geo {
  static constexpr int NWM = (WM == 1) ? 1 : 2, NWN = (WM == 0) ? 2 : 4, MI = (WM == 0) ? 2 : 4;
  static constexpr int NW = NWM * NWN, THREADS = 64 * NW, WPS = (WM == 0) ? 3 : 2;       // waves, waves per SIMD aimed at
  static constexpr int TM = NWM * MI * 32, TT = NWN * 64;                                // tile: weight rows, activation rows
  static constexpr int NPA = 3 * NWM * MI, NPB = 3 * NWN * 2;                            // 1-KiB pieces of one stage
  static constexpr int ACC = MI * 2 * 16;                                                // accumulator floats per lane
  static constexpr int MAX_SPX = (WM == 2) ? 32 : (WM == 1) ? 64 : 96;                   // workgroups per XCD
};

// LDS of a workgroup: the stages, or -- Z modes of the 128-row wave tiles -- the epilogue's staging area if that is larger (16 KiB per
// wave: two buffers of one 32 x 32 block of R and of Y), then one 512-B bias slot per wave and the hand-over word
template <int WM, int MODE>
struct X6Lds {
  using GEO = X6Geo<WM>;
  static constexpr bool STAGED = (MODE == MODE_Z || MODE == MODE_ZS || MODE == MODE_ZI || MODE == MODE_Z1) && GEO::MI == 4;
  static constexpr int STAGES = kStages * (GEO::NPA + GEO::NPB) * kFrag;
  static constexpr int MAIN = (STAGED && GEO::NW * 16384 > STAGES) ? GEO::NW * 16384 : STAGES;
  static constexpr int TOTAL = MAIN + GEO::NW * 512 + 16;
};

template <int WM, int MODE>
__global__ __launch_bounds__(X6Geo<WM>::THREADS, X6Geo<WM>::WPS) void x6_kernel(const X6Params p) {
  using GEO = X6Geo<WM>;
  constexpr int NW = GEO::NW, NWM = GEO::NWM, NWN = GEO::NWN, MI = GEO::MI;
  constexpr bool SGN = MODE == MODE_ZS;              // B holds the planes of X, not of |X|: the sign goes while staging
  constexpr bool Z_ABS = MODE == MODE_Z || SGN;      // Z from (Y - b) + |X||W|^T
  constexpr bool IS_Z = (Z_ABS || MODE == MODE_ZI || MODE == MODE_Z1);
  constexpr bool IS_C = (MODE == MODE_C || MODE == MODE_CI);
  constexpr int G = IS_C ? 6 : 3;                    // pieces of one A group (32 rows [x 2 signs]) per K16 step
  constexpr int NPA = GEO::NPA, NPB = GEO::NPB;      // 1-KiB pieces of one stage: weight side, activation side
  constexpr int NP = NPA + NPB;
  static_assert(NPA / 3 == NW, "each wave stages one weight-side block");
  constexpr int PBW = NPB / 3 / NW;                  // activation-side 32-row blocks each wave stages (2 or 1)
  constexpr int STAGE = NP * kFrag;
  constexpr int GROUPS = NPA / G;                    // A groups per tile: 4 WM (Z) or 2 WM (C)
  // Z modes on 128-row wave tiles stage the R / Y blocks of the epilogue through the (then idle) LDS: 16 KiB per wave (X6Staged)
  constexpr int LDS_MAIN = X6Lds<WM, MODE>::MAIN;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // Wave -> block of the tile: the NWM waves of one 64-row activation column are CONSECUTIVE waves, i.e. they sit on different
  // SIMDs (wave w runs on SIMD w % 4), and the activation blocks a wave stages (wave * PBW ...) are those of its own column.
  const int wm = wave % NWM, wn = wave / NWM;
  const int lane16 = lane * 16;

  // ---- this workgroup's range of the (tile, K-step) space: whole tiles per XCD, equal ranges inside one ----
  const int bid = blockIdx.x, spx = gridDim.x >> 3;
  const int xcd = bid & 7, slot = bid >> 3;
  const int nks = p.nks;
  const int tiles = p.ntm * p.ntn;
  const int tx0 = (int)((int64_t)tiles * xcd / 8), tx1 = (int)((int64_t)tiles * (xcd + 1) / 8);
  const int ntx = tx1 - tx0;
  const int64_t iters = (int64_t)ntx * nks;
  auto cut = [&](int s) -> int64_t {
    int64_t b = iters * s / spx;
    const int r = (int)(b % nks);
    if (p.whole_tiles) return (2 * r < nks) ? b - r : b + (nks - r);
    if (r < kMinFrag) b -= r;
    else if (nks - r < kMinFrag) b += nks - r;
    return b;
  };
  // whole_tiles == 2: the whole tiles of the XCD are CLAIMED, not assigned -- each workgroup takes the next tile index of the
  // XCD's range from the XCD's counter in the flag region (zero before the launch, like the flags) until the range is empty.
  // Under concurrent streams the workgroups of a launch become resident whenever a CU frees up: a late one then takes what is
  // left instead of owning one to three tiles an early one had to leave waiting.  A whole tile has no hand-over, so there is no
  // wait on another workgroup anywhere on this path, and every output is the same k-ordered chain whoever computes its tile.
  const bool claim = p.whole_tiles == 2;
  unsigned* const claim_ctr = p.flags + kClaimWord + xcd * kClaimStride;
  const int64_t ib = cut(slot), ie = cut(slot + 1);
  if (!claim && ib >= ie) return;
  const int f_tile = (int)(ib / nks), kb = (int)(ib - (int64_t)f_tile * nks);
  const int l_tile = (int)((ie - 1) / nks), ke = (int)(ie - (int64_t)l_tile * nks);
  const bool tail = kb > 0;                                            // first tile: its head belongs to slot - 1
  const bool head = (ke < nks) && !(f_tile == l_tile && tail);         // last tile: its tail belongs to slot + 1
  const int full0 = tail ? f_tile + 1 : f_tile, full1 = (ke < nks) ? l_tile - 1 : l_tile;
  const int nseq = (head ? 1 : 0) + (full1 >= full0 ? full1 - full0 + 1 : 0) + (tail ? 1 : 0);

  float* my_part = p.partial + (size_t)bid * GEO::THREADS * GEO::ACC;
  const float* in_part = p.partial + (size_t)(bid - 8) * GEO::THREADS * GEO::ACC;

  for (int seq = 0; claim || seq < nseq; ++seq) {
    int tile, k0, k1;
    if (claim) {
      // one lane takes the index, the workgroup reads it from LDS behind a barrier (the word after wait_for's; the barrier that
      // ends the previous tile lies between this store and that tile's reads of it)
      unsigned* const claimed = reinterpret_cast<unsigned*>(smem + X6Lds<WM, MODE>::MAIN + NW * 512) + 1;
      if (threadIdx.x == 0) *claimed = __hip_atomic_fetch_add(claim_ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __syncthreads();
      tile = (int)__builtin_amdgcn_readfirstlane(*claimed);
      if (tile >= ntx) break;
      k0 = 0, k1 = nks;
    } else if (head && seq == 0) {
      tile = l_tile, k0 = 0, k1 = ke;
    } else if (tail && seq == nseq - 1) {
      tile = f_tile, k0 = kb, k1 = (f_tile == l_tile) ? ke : nks;
    } else {
      tile = full0 + seq - (head ? 1 : 0), k0 = 0, k1 = nks;
    }
    tile += tx0;
    int tn, tm;
    if (p.t_fast) {
      tm = tile / p.ntn, tn = tile - tm * p.ntn;
    } else {
      tn = tile / p.ntm, tm = tile - tn * p.ntm;
    }
    // A ragged tile (fewer than TT live rows): a wave whose whole 64-row column lies at or beyond T is DEAD for this tile -- nothing it
    // would compute is ever stored.  It stages its weight-side block and keeps every barrier, and does nothing else: no activation
    // loads (the blocks it would stage are those of its own column), no fragment reads, no MFMAs, no hand-over traffic, no epilogue.
    // Wave-uniform, and the same on both sides of a cut.
    const bool dead = (int64_t)tn * GEO::TT + wn * 64 >= p.T;

    // ---- what this wave stages per step: the three planes of ONE weight-side 32-row block [one sign] and of PBW
    //      activation-side blocks -- each 3 KiB contiguous in memory and in the stage; wave-uniform pointers ----
    const unsigned char* srcA;
    if constexpr (!IS_C)
      srcA = p.A + (int64_t)(tm * GROUPS + wave) * p.a_group_stride + (int64_t)k0 * kRB;
    else
      srcA = p.A + (int64_t)(tm * GROUPS + (wave >> 1)) * p.a_group_stride + (int64_t)k0 * (2 * kRB) + (wave & 1) * kRB;
    const unsigned char* srcB[PBW];
#pragma unroll
    for (int u = 0; u < PBW; ++u) {
      const int cb = min(tn * (GEO::TT / 32) + wave * PBW + u, p.ncb - 1);
      srcB[u] = p.B + (int64_t)cb * p.b_rb_stride + (int64_t)k0 * kRB;
    }
    unsigned char* const ldsA = smem + wave * kRB;
    unsigned char* const ldsB = smem + NPA * kFrag + wave * (PBW * kRB);
    // adv = 0 re-requests the step already staged (branch-free last step: no control-flow join between the fragment
    // reads and the MFMAs, which is what lets hipcc wait for the reads piecemeal)
    // SGN: the activation blocks go through registers (plain loads, requested where the direct-to-LDS loads are) and reach the
    // stage through sign_and_store after the step's MFMAs: each block is fixed once per workgroup, by the wave that stages it,
    // and the pinned read / MFMA body below is that of MODE_Z.
    u32x4 breg[SGN ? PBW : 1][3];
    auto stage_a = [&](int stg, int adv) __attribute__((always_inline)) {       // the weight side alone: all a dead wave stages
      srcA += adv * (G * kFrag);
#pragma unroll
      for (int q = 0; q < 3; ++q) glds16(srcA + q * kFrag + lane16, ldsA + stg * STAGE + q * kFrag);
    };
    auto stage_in = [&](int stg, int adv) __attribute__((always_inline)) {
      srcA += adv * (G * kFrag);
#pragma unroll
      for (int u = 0; u < PBW; ++u) srcB[u] += adv * kRB;
#pragma unroll
      for (int q = 0; q < 3; ++q) glds16(srcA + q * kFrag + lane16, ldsA + stg * STAGE + q * kFrag);
#pragma unroll
      for (int u = 0; u < PBW; ++u)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          if constexpr (SGN) breg[u][q] = *reinterpret_cast<const u32x4*>(srcB[u] + q * kFrag + lane16);
          else glds16(srcB[u] + q * kFrag + lane16, ldsB + stg * STAGE + (u * 3 + q) * kFrag);
        }
    };
    // planes of x -> planes of |x| (split_kernel's dst_abs without its zero-residual mask: a low plane may hold -0 where
    // split3(|x|) has +0, and a -0 product leaves every accumulator -- which starts from +0 -- as it is), then into the stage
    auto sign_and_store = [&](int stg) __attribute__((always_inline)) {
#pragma unroll
      for (int u = 0; u < (SGN ? PBW : 0); ++u) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const unsigned m = breg[u][0][e] & 0x80008000u;
          breg[u][0][e] &= 0x7fff7fffu;
          breg[u][1][e] ^= m;
          breg[u][2][e] ^= m;
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) *reinterpret_cast<u32x4*>(ldsB + stg * STAGE + (u * 3 + q) * kFrag + lane16) = breg[u][q];
      }
    };

    // Bounded, loud wait for a flag another workgroup raises (release) once its accumulators are in memory; uniform
    // result.  On expiry: the caller's sticky status word and this pass's error word are set, `false` comes back.
    auto wait_for = [&](unsigned* flag) -> bool {
      unsigned* const ok_word = reinterpret_cast<unsigned*>(smem + LDS_MAIN + NW * 512);
      if (threadIdx.x == 0) {
        unsigned spins = 0, ok = 1u;
        const long long t_begin = wall_clock64();
        while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
          __builtin_amdgcn_s_sleep(8);
          if ((++spins & 63u) == 0u &&
              (__hip_atomic_load(p.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u ||
               wall_clock64() - t_begin > p.spin_ticks)) {
            ok = 0u;
            break;
          }
        }
        if (!ok) {
          __hip_atomic_fetch_or(p.status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(p.flags + kErrWord, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        __hip_atomic_store(flag, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *ok_word = ok;
      }
      __syncthreads();
      return __builtin_amdgcn_readfirstlane(*ok_word) != 0u;     // (a main loop's barriers lie between two waits)
    };
    f32x16 acc[MI][2];
    if (k0 > 0) {
      // the head of this tile was computed by the workgroup 8 below: wait for its accumulators, continue its chain.
      // The wait is bounded (a predecessor that never becomes resident must not hang the GPU) and LOUD: on expiry the
      // workgroup ORs the caller's sticky status word and its pass's error word and continues from NaN accumulators, so
      // the C-pass / plain-GEMM outputs of the tile are NaN (the Z-pass then takes its exact fallback for every element
      // of the tile: correct values, slowly).  Once any workgroup of any launch has failed, later waits give up at once.
      // (a dead wave keeps the wait's barrier and skips the loads, as the publishing side skipped the stores)
      const bool handed_over = wait_for(p.flags + bid - 8);
      if (!dead) {
      const f32x4* ip = reinterpret_cast<const f32x4*>(in_part) + (size_t)wave * (GEO::ACC / 4) * 64 + lane;
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const f32x4 v = ip[c * 64];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[mi][ni][4 * c + e] = handed_over ? v[e] : __builtin_nanf("");
          }
          ip += 4 * 64;
          asm volatile("" : "+v"(ip));      // one running pointer, not 32 precomputed ones
        }
      }
    } else {
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.0f;
    }

    // ---- main loop: stage ks + 1 lands while stage ks is multiplied ----
    int st = 0;
    if (dead) {
      // the same waits and barriers, step for step, around the weight-side loads alone.  Nothing is requested in the last step: a
      // dead wave goes straight on to the epilogue's barrier, behind which the live waves reuse the stages, so no load of its own
      // may still be on its way into them.
      stage_a(0, 0);
      for (int ks = k0; ks < k1; ++ks) {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (ks + 1 < k1) stage_a((st + 1) % kStages, 1);
        st = (st + 1 == kStages) ? 0 : st + 1;
      }
    } else {
    stage_in(0, 0);
    if constexpr (SGN) sign_and_store(0);
    bf16x8 a[MI][3], b[2][3];
    for (int ks = k0; ks < k1; ++ks) {
      // This step's stage has landed (own loads: vmcnt; every wave's: the barrier), and the stage of step ks - 1 is free
      // again (every wave finished its fragment reads before it arrived here: lgkmcnt(0) at the last MFMA round).  A RAW
      // s_barrier: __syncthreads() carries a workgroup fence, for which hipcc drains vmcnt(0) -- a direct-to-LDS load is a
      // pending LDS write -- i.e. it would cut the prefetch distance back to one step.
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      const unsigned char* sA = smem + st * STAGE + wm * (MI * kRB) + lane16;
      const unsigned char* sB = smem + st * STAGE + NPA * kFrag + wn * (2 * kRB) + lane16;
      // The order below is pinned with sched_barrier: left to itself hipcc's scheduler flips between an order that
      // chains dependent MFMAs two apart behind piecemeal LDS waits and a good one on unrelated source edits (+-17 % on
      // the whole kernel, measured).  Six partial products per block, smallest first (PA / PB); one ROUND = the same
      // partial product of all eight blocks (eight independent accumulators between dependent MFMAs), so the order of
      // the blocks inside a round is free: it is chosen so that every MFMA needs at most ONE fragment the previous ones
      // did not ((a0,b0) (a1,b0) (a1,b1) (a0,b1) (a2,b1) (a2,b0) (a3,b0) (a3,b1)), the fragment reads are issued in that
      // order (b0 a0 a1 b1 a2 a3; round 0 = plane 1 of both sides, round 1 planes (0, 2), round 2 planes (2, 0); rounds
      // 3-5 reuse what is resident), three to six at a time between the MFMAs, and each MFMA waits for exactly its own
      // operands.  After the barrier all eight waves read at once and the LDS delivers one 1 KiB fragment per 8 clocks:
      // waiting for a whole round (6 fragments x 8 waves) before the first MFMA idled the pipe for ~13 % of the step.
      // The reads are inline asm with hand-counted waits (guide 5.7): hipcc waits lgkmcnt(0) before the first MFMA once a
      // direct-to-LDS load is in flight.  lgkmcnt counts LDS returns in order: with I reads issued, fragment n (0-based)
      // is present once at most I - 1 - n are outstanding.  (Waits the compiler adds for its own LDS operations can only
      // be longer than needed.)
      const unsigned aA = (unsigned)(uintptr_t)sA, aB = (unsigned)(uintptr_t)sB;
#define X6_SB __builtin_amdgcn_sched_barrier(0)
#define X6_RDB(ni, r) \
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(b[ni][PB[r]]) : "v"(aB), "i"((ni) * kRB + PB[r] * kFrag))
#define X6_RDA(mi, r) \
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(a[mi][PA[r]]) : "v"(aA), "i"((mi) * kRB + PA[r] * kFrag))
#define X6_WAIT(n)                                                           \
  X6_SB;                                                                     \
  asm volatile("s_waitcnt lgkmcnt(" #n ")" ::: "memory"); \
  X6_SB
#define X6_MM(mi, ni, q) acc[mi][ni] = TE_MFMA_BF16(a[mi][PA[q]], b[ni][PB[q]], acc[mi][ni])
#define X6_RD_HEAD(r) X6_SB; X6_RDB(0, r); X6_RDA(0, r); X6_RDA(1, r); X6_SB
#define X6_RD_TAIL(r) X6_SB; X6_RDB(1, r); X6_RDA(2, r); X6_RDA(3, r); X6_SB
      if constexpr (MI == 2) {
        // 64 x 64 wave tile: four blocks, 24 MFMAs and 12 fragment reads per step (three waves per SIMD cover the rest).
        // Round r reads (b0 a0 a1 b1) of its plane pair; with I reads issued fragment n is present at lgkmcnt <= I - 1 - n.
#define X6_RD4(r) X6_SB; X6_RDB(0, r); X6_RDA(0, r); X6_RDA(1, r); X6_RDB(1, r); X6_SB
        X6_RD4(0);
        X6_RD4(1);                                                   // 8 issued
        stage_in((st + 1) % kStages, (ks + 1 < k1) ? 1 : 0);
        X6_WAIT(6); X6_MM(0, 0, 0);
        X6_WAIT(5); X6_MM(1, 0, 0);
        X6_WAIT(4); X6_MM(1, 1, 0); X6_MM(0, 1, 0);
        X6_RD4(2);                                                   // 12 issued
        X6_WAIT(6); X6_MM(0, 0, 1);
        X6_WAIT(5); X6_MM(1, 0, 1);
        X6_WAIT(4); X6_MM(1, 1, 1); X6_MM(0, 1, 1);
        X6_WAIT(2); X6_MM(0, 0, 2);
        X6_WAIT(1); X6_MM(1, 0, 2);
        X6_WAIT(0); X6_MM(1, 1, 2); X6_MM(0, 1, 2);
        X6_SB;
#pragma unroll
        for (int q6 = 3; q6 < 6; ++q6) {
          X6_MM(0, 0, q6); X6_MM(1, 0, q6); X6_MM(1, 1, q6); X6_MM(0, 1, q6);
          X6_SB;
        }
#undef X6_RD4
      } else {
      X6_RD_HEAD(0);
      X6_RD_TAIL(0);                                                 // 6 issued
      // the next step's stage is requested before the first MFMA (a direct-to-LDS load between MFMAs costs issue slots)
      stage_in((st + 1) % kStages, (ks + 1 < k1) ? 1 : 0);
      X6_WAIT(4); X6_MM(0, 0, 0);
      X6_WAIT(3); X6_MM(1, 0, 0);
      X6_WAIT(2); X6_MM(1, 1, 0); X6_MM(0, 1, 0);
      X6_RD_HEAD(1);                                                 // 9 issued
      X6_WAIT(4); X6_MM(2, 1, 0); X6_MM(2, 0, 0);
      X6_WAIT(3); X6_MM(3, 0, 0); X6_MM(3, 1, 0);
      X6_RD_TAIL(1);                                                 // 12 issued
      X6_WAIT(4); X6_MM(0, 0, 1);
      X6_WAIT(3); X6_MM(1, 0, 1);
      X6_WAIT(2); X6_MM(1, 1, 1); X6_MM(0, 1, 1);
      X6_RD_HEAD(2);                                                 // 15 issued
      X6_WAIT(4); X6_MM(2, 1, 1); X6_MM(2, 0, 1);
      X6_WAIT(3); X6_MM(3, 0, 1); X6_MM(3, 1, 1);
      X6_RD_TAIL(2);                                                 // 18 issued
      X6_WAIT(4); X6_MM(0, 0, 2);
      X6_WAIT(3); X6_MM(1, 0, 2);
      X6_WAIT(2); X6_MM(1, 1, 2); X6_MM(0, 1, 2);
      X6_WAIT(1); X6_MM(2, 1, 2); X6_MM(2, 0, 2);
      X6_WAIT(0); X6_MM(3, 0, 2); X6_MM(3, 1, 2);
      X6_SB;
#pragma unroll
      for (int q6 = 3; q6 < 6; ++q6) {
        X6_MM(0, 0, q6); X6_MM(1, 0, q6); X6_MM(1, 1, q6); X6_MM(0, 1, q6);
        X6_MM(2, 1, q6); X6_MM(2, 0, q6); X6_MM(3, 0, q6); X6_MM(3, 1, q6);
        X6_SB;
      }
      }
#undef X6_SB
#undef X6_RDB
#undef X6_RDA
#undef X6_WAIT
#undef X6_MM
#undef X6_RD_HEAD
#undef X6_RD_TAIL
      // (the stage of step ks - 1: every wave left it before this step's barrier; the next barrier's lgkmcnt(0) covers the writes)
      if constexpr (SGN) sign_and_store((st + 1) % kStages);
      st = (st + 1 == kStages) ? 0 : st + 1;
    }
    }
    // (the last step staged itself again: those writes are in the LDS before the epilogue's barrier lets anything reuse the stages)
    if constexpr (SGN) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    // ---- accumulators to memory + flag (guide: plain stores -> vmcnt(0) -> barrier -> release -> flag) ----
    auto publish = [&](float* dst, unsigned* flag) __attribute__((always_inline)) {
      f32x4* op = reinterpret_cast<f32x4*>(dst) + (size_t)wave * (GEO::ACC / 4) * 64 + lane;
      if (!dead) {
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = acc[mi][ni][4 * c + e];
            op[c * 64] = v;
          }
          op += 4 * 64;
          asm volatile("" : "+v"(op));
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (!p.drop_handover) __hip_atomic_store(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    };
    if (k1 < nks) {            // a cut work item: the workgroup 8 above continues this chain
      publish(my_part, p.flags + bid);
      continue;
    }
    // ---- epilogue.  32x32 block (mi, ni): lane (tc = lane & 31, h = lane >> 5) holds activation row t and, for
    //      g = 0..3, weight rows 8 g + 4 h + (0..3) in acc[4 g .. 4 g + 3] ----
    const int tc = lane & 31, h = lane >> 5;
    // The loads of a block are issued as one batch BEFORE the previous block's stores (hipcc keeps loads behind stores
    // that may alias, and a store then costs a full round trip per `s_waitcnt vmcnt`): first light of this kernel spent
    // 110 us per tile in a load -> wait -> store -> wait chain.
    if (dead) {
      // the barrier of the staged Z epilogue below ("the stages are free"); everything else there is private to its wave
      if constexpr (X6Lds<WM, MODE>::STAGED) __builtin_amdgcn_s_barrier();
    } else if constexpr (IS_Z) {
      const int nksS = p.out_f >> 4;
      int64_t tl[2];
      bool live[2], blk[2];
      float f[2];
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int cb = tn * (GEO::TT / 32) + wn * 2 + ni;
        const int64_t t = (int64_t)cb * 32 + tc;
        blk[ni] = cb < p.ncb;
        live[ni] = t < p.T;
        tl[ni] = live[ni] ? t : p.T - 1;
        f[ni] = p.rs ? p.rs[(tl[ni] / p.rps) * p.rs_stride] : 1.0f;
      }
      // the wave's 128 bias values go through a private 512-B LDS slot: reading them back counts on lgkmcnt, so no wait
      // for a bias value drains the prefetched R / Y loads of the next block
      float* const bias_lds = reinterpret_cast<float*>(smem + LDS_MAIN) + wave * 128;
      if (lane < MI * 8) {
        f32x4 bv = {0.0f, 0.0f, 0.0f, 0.0f};
        if (p.bias) bv = *reinterpret_cast<const f32x4*>(p.bias + (tm * (NWM * MI) + wm * MI) * 32 + lane * 4);
        *reinterpret_cast<f32x4*>(bias_lds + lane * 4) = bv;
      }
      if constexpr (X6Lds<WM, MODE>::STAGED) {
        // Round 6 (profiles/r06_x6_epilogue_study.log (5)): a lane of the accumulator layout owns the 16-byte pieces g = 0..3 of ONE
        // 128-byte line of its row, so the four load instructions of a block touched the same 32 lines back to back and the in-order L1
        // stalled on the pending fills.  Here every line is requested by ONE instruction: a direct-to-LDS load covers 8 rows x 128 B
        // (8 lanes per line), chunk order XOR-permuted by the row so that the read-back in the accumulator layout -- lane (tc, h),
        // piece g = chunk 2g + h of row tc -- is bank-conflict free: [row][128 B] images, row r holds chunk c at slot c ^ ((r >> 1) & 7).
        constexpr int NL = (MODE == MODE_Z1) ? 4 : 8;                 // direct-to-LDS loads per block
        __builtin_amdgcn_s_barrier();                                 // every wave has read its last fragments: the stages are free
        unsigned char* const stg = smem + wave * 16384;               // two buffers of (R block, Y block)
        unsigned rda[4];
#pragma unroll
        for (int g = 0; g < 4; ++g)
          rda[g] = (unsigned)(uintptr_t)stg + tc * 128 + (((2 * g + h) ^ ((tc >> 1) & 7)) << 4);
        const unsigned bia = (unsigned)(uintptr_t)bias_lds + h * 16;
        const int r8 = lane >> 3;
        auto request = [&](int bi, int buf) __attribute__((always_inline)) {
          const int ni = bi / MI, mi = bi % MI;
          const int cb = tn * (GEO::TT / 32) + wn * 2 + ni;
          const int j0 = (tm * (NWM * MI) + wm * MI + mi) * 32;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int row = 8 * i + r8;
            const int64_t t = min((int64_t)cb * 32 + row, p.T - 1);
            const int64_t off = t * p.out_f + j0 + (((lane & 7) ^ ((row >> 1) & 7)) << 2);
            glds16(reinterpret_cast<const unsigned char*>(p.R + off), stg + buf * 8192 + i * 1024);
            if constexpr (MODE != MODE_Z1)
              glds16(reinterpret_cast<const unsigned char*>(p.Y + off), stg + buf * 8192 + 4096 + i * 1024);
          }
        };
        // Two blocks in flight: block bi + 2 is requested into block bi's buffer as soon as block bi sits in registers.  The wait for
        // block bi is hand-counted: younger in the queue are the loads of block bi + 1 and the S stores of blocks bi - 2 and bi - 1
        // (six each, if the wave's row blocks exist: `all_blk`; else only the loads are counted, which waits longer, never shorter).
        const bool all_blk = blk[0] && blk[1];
        request(0, 0);
        request(1, 1);
#pragma unroll
        for (int bi = 0; bi < 2 * MI; ++bi) {
          const int ni = bi / MI, mi = bi % MI, buf = bi & 1;
          const int cb = tn * (GEO::TT / 32) + wn * 2 + ni;
          const int j0 = (tm * (NWM * MI) + wm * MI + mi) * 32;
          constexpr int kStore = 6;
          const int yl = (bi + 1 < 2 * MI) ? NL : 0, ys = (bi >= 2 ? kStore : 0) + (bi >= 1 ? kStore : 0);
          if (all_blk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(yl + ys) : "memory");
          else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(yl) : "memory");
          f32x4 r4[4], y4[4], b4[4];
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r4[g]) : "v"(rda[g]), "i"(buf * 8192));
            if constexpr (MODE != MODE_Z1)
              asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(y4[g]) : "v"(rda[g]), "i"(buf * 8192 + 4096));
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(b4[g]) : "v"(bia), "i"((mi * 32 + 8 * g) * 4));
          }
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          if (bi + 2 < 2 * MI) request(bi + 2, buf);
          X6_PASS4(r4[0], r4[1], r4[2], r4[3]);
          if constexpr (MODE != MODE_Z1) X6_PASS4(y4[0], y4[1], y4[2], y4[3]);
          X6_PASS4(b4[0], b4[1], b4[2], b4[3]);
          // Element pairs on packed fp32 instructions (z, the division: sd2 -- an IEEE quotient without its range scaling, correctly
          // rounded inside the normal range).  Which elements cancel is kept as wave-level lane masks (the compare's own result,
          // OR-ed on the scalar unit); the per-lane bit mask the fallback wants is rebuilt only if one is set.
          unsigned w[4][3][2];
          unsigned long long any_cancel = 0;
          auto z_of = [&](int g, int c0, f32x2& z2, f32x2& a2) __attribute__((always_inline)) {
            a2 = f32x2{acc[mi][ni][4 * g + c0], acc[mi][ni][4 * g + c0 + 1]};
            if constexpr (Z_ABS)                     // Z  = X+ W+^T + X- W-^T = ((Y - b) + |X||W|^T) / 2  (>= 0)
              z2 = f32x2{0.5f, 0.5f} * ((f32x2{y4[g][c0], y4[g][c0 + 1]} - f32x2{b4[g][c0], b4[g][c0 + 1]}) + a2);
            else if constexpr (MODE == MODE_ZI)      // Z' = X+ W-^T + X- W+^T = ((Y - b) - |X||W|^T) / 2  (<= 0)
              z2 = f32x2{0.5f, 0.5f} * ((f32x2{y4[g][c0], y4[g][c0 + 1]} - f32x2{b4[g][c0], b4[g][c0 + 1]}) - a2);
            else                                     // one-sided product: the accumulator is Z
              z2 = a2;
          };
          // (te_common.h: te_z_cancels -- the halves cancel, or Z drowns in the rounding Y inherited from the bias)
          auto cancels = [&](float z, float a_abs, float b) __attribute__((always_inline)) -> bool {
            if constexpr (Z_ABS) return te_z_cancels(z, a_abs, b);
            else if constexpr (MODE == MODE_ZI) return te_z_cancels(-z, a_abs, b);
            else return false;
          };
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            float sv4[4];
#pragma unroll
            for (int c0 = 0; c0 < 4; c0 += 2) {
              f32x2 z2, a2;
              z_of(g, c0, z2, a2);
              f32x2 rr = {r4[g][c0], r4[g][c0 + 1]};
              if (p.rs) rr = rr * f32x2{f[ni], f[ni]};
              const f32x2 sv = sd2(rr, z2);
#pragma unroll
              for (int e = 0; e < 2; ++e) {
                const bool cancel = cancels(z2[e], a2[e], b4[g][c0 + e]);
                if constexpr (MODE != MODE_Z1) any_cancel |= __builtin_amdgcn_ballot_w64(cancel);
                sv4[c0 + e] = (live[ni] && !cancel) ? sv[e] : 0.0f;
              }
            }
            unsigned lo[3], hi[3];
            split3_pk(sv4[0], sv4[1], lo);
            split3_pk(sv4[2], sv4[3], hi);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
              w[g][q][0] = lo[q];
              w[g][q][1] = hi[q];
            }
          }
          unsigned bad = 0;                          // elements whose Z needs the cancellation fallback
          if (any_cancel != 0) {
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
              for (int c0 = 0; c0 < 4; c0 += 2) {
                f32x2 z2, a2;
                z_of(g, c0, z2, a2);
                bad |= (cancels(z2[0], a2[0], b4[g][c0]) ? 1u : 0u) << (4 * g + c0);
                bad |= (cancels(z2[1], a2[1], b4[g][c0 + 1]) ? 1u : 0u) << (4 * g + c0 + 1);
              }
          }
#pragma unroll
          for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int q = 0; q < 3; ++q)
#pragma unroll
              for (int d = 0; d < 2; ++d) swap_halves(w[g][q][d], w[g + 2][q][d]);
          if (blk[ni]) {
            unsigned char* Srow = p.S + (int64_t)cb * nksS * kRB + tc * 16;
            unsigned char* sp = Srow + (int64_t)((j0 >> 4) + h) * kRB;
#pragma unroll
            for (int q = 0; q < 3; ++q)
#pragma unroll
              for (int c = 0; c < 2; ++c) {
                u32x4 v = {w[c][q][0], w[c][q][1], w[c + 2][q][0], w[c + 2][q][1]};
                *reinterpret_cast<u32x4*>(sp + q * kFrag + c * 512) = v;
              }
            if (!live[ni]) bad = 0;
            if (__builtin_amdgcn_ballot_w64(bad != 0) != 0) {
              asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
              const float* Rrow = p.R + tl[ni] * p.out_f;
#pragma clang loop unroll(disable)
              for (int e = 0; e < 16; ++e) {
                if ((bad >> e) & 1u) {
                  const int jj = j0 + 8 * (e >> 2) + 4 * h + (e & 3);
                  const float z = (MODE == MODE_ZI) ? exact_zi(p.X + tl[ni] * p.in_f, p.W + (int64_t)jj * p.in_f, p.in_f)
                                                    : exact_z(p.X + tl[ni] * p.in_f, p.W + (int64_t)jj * p.in_f, p.in_f);
                  float rr = Rrow[jj];
                  if (p.rs) rr = rr * f[ni];
                  unsigned pl[3];
                  split3(te_sd(rr, z), pl);
                  unsigned short* d = reinterpret_cast<unsigned short*>(Srow + (int64_t)(jj >> 4) * kRB + ((jj >> 3) & 1) * 512) + (jj & 7);
                  d[0] = (unsigned short)pl[0];
                  d[kFrag / 2] = (unsigned short)pl[1];
                  d[kFrag] = (unsigned short)pl[2];
                }
              }
            }
          }
        }
      } else {
      // (128 x 128 geometry: three waves per SIMD cover the load latency, and 168 VGPRs do not hold a second buffer)
      constexpr int NBUF = (MI == 4) ? 2 : 1;
      f32x4 r4[NBUF][4], y4[NBUF][4];
      auto load_block = [&](int bi, int buf) __attribute__((always_inline)) {
        const int ni = bi / MI, mi = bi % MI;
        const int j0 = (tm * (NWM * MI) + wm * MI + mi) * 32;
        const float* Rrow = p.R + tl[ni] * p.out_f + j0 + 4 * h;
#pragma unroll
        for (int g = 0; g < 4; ++g) r4[buf][g] = *reinterpret_cast<const f32x4*>(Rrow + 8 * g);
        if constexpr (MODE != MODE_Z1) {
          const float* Yrow = p.Y + tl[ni] * p.out_f + j0 + 4 * h;
#pragma unroll
          for (int g = 0; g < 4; ++g) y4[buf][g] = *reinterpret_cast<const f32x4*>(Yrow + 8 * g);
        }
      };
      if constexpr (NBUF == 2) load_block(0, 0);
#pragma unroll
      for (int bi = 0; bi < 2 * MI; ++bi) {
        const int ni = bi / MI, mi = bi % MI, buf = bi % NBUF;
        const int cb = tn * (GEO::TT / 32) + wn * 2 + ni;
        const int j0 = (tm * (NWM * MI) + wm * MI + mi) * 32;
        if constexpr (NBUF == 2) {
          if (bi + 1 < 2 * MI) load_block(bi + 1, buf ^ 1);      // in flight during this block's arithmetic
        } else {
          load_block(bi, 0);
        }
        unsigned w[4][3][2];                       // [g][plane][dword]: four bf16 of one plane = weight rows 8g+4h+0..3
        unsigned bad = 0;                          // elements whose Z needs the cancellation fallback
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 b4 = *reinterpret_cast<const f32x4*>(bias_lds + mi * 32 + 8 * g + 4 * h);
          float sv4[4];
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float a_abs = acc[mi][ni][4 * g + c];
            float z;
            bool cancel;
            if constexpr (Z_ABS) {                       // Z  = X+ W+^T + X- W-^T = ((Y - b) + |X||W|^T) / 2  (>= 0)
              z = 0.5f * ((y4[buf][g][c] - b4[c]) + a_abs);
              cancel = te_z_cancels(z, a_abs, b4[c]);
            } else if constexpr (MODE == MODE_ZI) {      // Z' = X+ W-^T + X- W+^T = ((Y - b) - |X||W|^T) / 2  (<= 0)
              z = 0.5f * ((y4[buf][g][c] - b4[c]) - a_abs);
              cancel = te_z_cancels(-z, a_abs, b4[c]);
            } else {                                     // one-sided product: the accumulator is Z
              z = a_abs;
              cancel = false;
            }
            bad |= (cancel ? 1u : 0u) << (4 * g + c);
            float rr = r4[buf][g][c];
            if (p.rs) rr = rr * f[ni];
            float sv = te_sd(rr, z);
            asm volatile("" : "+v"(sv));            // evaluated for every lane: a select below, not a branch around the division
            sv4[c] = (live[ni] && !cancel) ? sv : 0.0f;
          }
          unsigned lo[3], hi[3];
          split3_pk(sv4[0], sv4[1], lo);
          split3_pk(sv4[2], sv4[3], hi);
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            w[g][q][0] = lo[q];
            w[g][q][1] = hi[q];
          }
        }
        // lanes h = 0 end up with the 16-B pieces g = 0, 1 (8 consecutive features each), lanes h = 1 with g = 2, 3
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
          for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int d = 0; d < 2; ++d) swap_halves(w[g][q][d], w[g + 2][q][d]);
        if (blk[ni]) {
          unsigned char* Srow = p.S + (int64_t)cb * nksS * kRB + tc * 16;
          unsigned char* sp = Srow + (int64_t)((j0 >> 4) + h) * kRB;
#pragma unroll
          for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int c = 0; c < 2; ++c) {           // c = k-half of the K16 step (j0 / 16 + h)
              // h = 0: piece g = c is {own w[c], partner's w[c]} = (w[c], w[c + 2]) after the swap
              // h = 1: piece g = 2 + c is {partner's w[2 + c], own w[2 + c]} = (w[c], w[c + 2]) after the swap
              u32x4 v = {w[c][q][0], w[c][q][1], w[c + 2][q][0], w[c + 2][q][1]};
              *reinterpret_cast<u32x4*>(sp + q * kFrag + c * 512) = v;
            }
          // rare: (Y - b) and |X||W|^T cancel (nearly every product of the element is negative), or |Z| <= 2^-4 |b_j| (Y - b
          // carries the bias's rounding; te_common.h: te_z_cancels): the reference's plain positive-part sum, k-ordered,
          // written over the element's three plane values
          if (!live[ni]) bad = 0;
          if (__builtin_amdgcn_ballot_w64(bad != 0) != 0) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the 16-B pieces above are in memory first
            const float* Rrow = p.R + tl[ni] * p.out_f;
#pragma clang loop unroll(disable)
            for (int e = 0; e < 16; ++e) {
              if ((bad >> e) & 1u) {
                const int jj = j0 + 8 * (e >> 2) + 4 * h + (e & 3);
                const float z = (MODE == MODE_ZI) ? exact_zi(p.X + tl[ni] * p.in_f, p.W + (int64_t)jj * p.in_f, p.in_f)
                                                  : exact_z(p.X + tl[ni] * p.in_f, p.W + (int64_t)jj * p.in_f, p.in_f);
                float rr = Rrow[jj];
                if (p.rs) rr = rr * f[ni];
                unsigned pl[3];
                split3(te_sd(rr, z), pl);
                unsigned short* d = reinterpret_cast<unsigned short*>(Srow + (int64_t)(jj >> 4) * kRB + ((jj >> 3) & 1) * 512) + (jj & 7);
                d[0] = (unsigned short)pl[0];
                d[kFrag / 2] = (unsigned short)pl[1];
                d[kFrag] = (unsigned short)pl[2];
              }
            }
          }
        }
      }
      }
    } else if constexpr (MODE == MODE_G) {
      // plain product: out[t][m] = acc + bias[m] (fp32 row-major [T, M]); the wave's 128 bias values through its LDS slot
      float* const bias_lds = reinterpret_cast<float*>(smem + LDS_MAIN) + wave * 128;
      if (lane < MI * 8) {
        f32x4 bv = {0.0f, 0.0f, 0.0f, 0.0f};
        if (p.bias) bv = *reinterpret_cast<const f32x4*>(p.bias + (tm * (NWM * MI) + wm * MI) * 32 + lane * 4);
        *reinterpret_cast<f32x4*>(bias_lds + lane * 4) = bv;
      }
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int64_t t = ((int64_t)tn * (GEO::TT / 32) + wn * 2 + ni) * 32 + tc;
        float* orow = p.out + (t < p.T ? t : 0) * p.out_f + (tm * (NWM * MI) + wm * MI) * 32 + 4 * h;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(bias_lds + mi * 32 + 8 * g + 4 * h);
            f32x4 o;
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = acc[mi][ni][4 * g + c] + b4[c];
            if (t < p.T) *reinterpret_cast<f32x4*>(orow + mi * 32 + 8 * g) = o;
          }
      }
    } else if constexpr (MODE == MODE_X) {
      // masked product (variant lrp's C-pass, one sign at a time: layers_lrp.py:201-202): out[t][m] (+)= scale * (X+-[t][m] * acc)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int64_t t = ((int64_t)tn * (GEO::TT / 32) + wn * 2 + ni) * 32 + tc;
        const int64_t off = (t < p.T ? t : 0) * p.out_f + (tm * (NWM * MI) + wm * MI) * 32 + 4 * h;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          f32x4 xv[4], pv[4];
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            xv[g] = *reinterpret_cast<const f32x4*>(p.X + off + mi * 32 + 8 * g);
            pv[g] = p.accum ? *reinterpret_cast<const f32x4*>(p.out + off + mi * 32 + 8 * g) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
          }
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            f32x4 o;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const float xm = (p.x_sign > 0) ? fmaxf(xv[g][c], 0.0f) : fminf(xv[g][c], 0.0f);
              const float v = p.scale * (xm * acc[mi][ni][4 * g + c]);
              o[c] = p.accum ? pv[g][c] + v : v;
            }
            if (t < p.T) *reinterpret_cast<f32x4*>(p.out + off + mi * 32 + 8 * g) = o;
          }
        }
      }
    } else {
      f32x4 x4[2][MI / 2][4];
      int64_t tt[2];
      bool live[2];
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int64_t t = ((int64_t)tn * (GEO::TT / 32) + wn * 2 + ni) * 32 + tc;
        live[ni] = t < p.T;
        tt[ni] = live[ni] ? t : p.T - 1;
#pragma unroll
        for (int il = 0; il < MI / 2; ++il) {
          const float* xr = p.X + tt[ni] * p.in_f + (tm * (NWM * MI / 2) + wm * (MI / 2) + il) * 32 + 4 * h;
#pragma unroll
          for (int g = 0; g < 4; ++g) x4[ni][il][g] = *reinterpret_cast<const f32x4*>(xr + 8 * g);
        }
      }
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int il = 0; il < MI / 2; ++il) {
          float* orow = p.out + tt[ni] * p.in_f + (tm * (NWM * MI / 2) + wm * (MI / 2) + il) * 32 + 4 * h;
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            f32x4 o;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const float xv = x4[ni][il][g][c];
              const float xp = fmaxf(xv, 0.0f), xn = fminf(xv, 0.0f);
              if constexpr (MODE == MODE_C)     // alpha * (X+ . (S W+) + X- . (S W-))                  layers_ours.py:222-228
                o[c] = p.scale * (xp * acc[2 * il][ni][4 * g + c] + xn * acc[2 * il + 1][ni][4 * g + c]);
              else                              // out - beta * (X+ . (S' W-) + X- . (S' W+)): scale = -beta
                o[c] = p.scale * (xp * acc[2 * il + 1][ni][4 * g + c] + xn * acc[2 * il][ni][4 * g + c]);
            }
            if constexpr (MODE == MODE_CI) {
              const f32x4 prev = *reinterpret_cast<const f32x4*>(orow + 8 * g);
#pragma unroll
              for (int c = 0; c < 4; ++c) o[c] = prev[c] + o[c];
            }
            if (live[ni]) *reinterpret_cast<f32x4*>(orow + 8 * g) = o;
          }
        }
    }
    __syncthreads();       // every wave is done with the stages before the next fragment's first loads land in them
  }
}

// The kernel-argument block of x6_kernel, pinned (the comment at pad0_): the values of the build the spills were measured on.
static_assert(sizeof(X6Params) == 248, "X6Params is the kernel-argument block of x6_kernel");
static_assert(offsetof(X6Params, ntm) == 56 && offsetof(X6Params, ncb) == 80 && offsetof(X6Params, T) == 88 &&
              offsetof(X6Params, partial) == 104 && offsetof(X6Params, R) == 152 && offsetof(X6Params, out) == 224,
              "a field of X6Params moved in the kernel arguments");

inline size_t planes_bytes(int64_t rows, int64_t K) {
  return (size_t)te_ceil_div(rows, 32) * 32 * (size_t)K * 6;
}
inline bool bad_k(int64_t K) { return K < 16 || K % 16; }         // planes are cut in K16 steps
// (A fixed K split -- two k-ordered chains per output for long-K, few-row products -- was measured and not shipped:
// 5 % over the 128 x 128 geometry in isolated launches, nothing in the step)
constexpr size_t kPartialBytes = (size_t)512 * 256 * 128 * 4;       // grid x threads x accumulators: 64 MiB covers every geometry
constexpr size_t kFlagBytes = 65536;                                 // 512 flags + the error word, per pass
constexpr int kFlagWords = kFlagBytes / 4;                           // one pass's flag region, in words ...
constexpr int kUsedFlagWords = kErrWord + 1;                         // ... of which a launch touches these (the check reads them)
constexpr int kRulePasses = 2;                                       // default rule: Z-pass, C-pass
constexpr int kGeneralPasses = 8;                                    // general rule: four per half + the per-call error word's

// ---- where things lie: ONE statement per buffer, read by the *_bytes query, the call that writes and the call that reads ----
// Workspace of a call, byte offsets (every region 256-byte aligned): `xsets` plane sets of the input side ([T, K] each) from 0,
// `ssets` of the output side ([T, M] each) from s, the accumulators of cut tiles, one flag region per pass.
struct X6Workspace {
  size_t x_stride, s, s_stride, partial, flags, total;
  unsigned char* x(void* ws, int set) const { return (unsigned char*)ws + set * x_stride; }
  unsigned char* sp(void* ws, int set) const { return (unsigned char*)ws + s + set * s_stride; }
  float* acc(void* ws) const { return (float*)((unsigned char*)ws + partial); }
  unsigned* flag_region(const void* ws, int pass) const { return (unsigned*)((unsigned char*)ws + flags) + (size_t)pass * kFlagWords; }
};
inline X6Workspace x6_workspace(int64_t T, int64_t K, int64_t M, int xsets, int ssets, int passes) {
  X6Workspace l;
  l.x_stride = te_align_up(planes_bytes(T, K), 256);
  l.s_stride = te_align_up(planes_bytes(T, M), 256);
  l.s = xsets * l.x_stride;
  l.partial = l.s + ssets * l.s_stride;
  l.flags = l.partial + kPartialBytes;
  l.total = l.flags + passes * kFlagBytes;
  return l;
}
// plain product: X planes | default rule: |X| planes, S planes | general rule: |X| or X+, X-, then S / S' or S1, S2
inline X6Workspace gemm_workspace(int64_t T, int64_t K, int64_t M) { return x6_workspace(T, K, M, 1, 0, 1); }
inline X6Workspace rule_workspace(int64_t T, int64_t in_f, int64_t out_f) { return x6_workspace(T, in_f, out_f, 1, 1, kRulePasses); }
inline X6Workspace general_workspace(int64_t T, int64_t in_f, int64_t out_f) { return x6_workspace(T, in_f, out_f, 2, 2, kGeneralPasses); }

// weight planes of the default rule: P3 of |W| (rows = out_f, K = in_f) at 0, P6 of W+^T / W-^T (rows = in_f, K = out_f) at c
struct X6WeightPlanes { size_t c, total; };
inline X6WeightPlanes weight_planes(int64_t in_f, int64_t out_f) {
  const size_t c = te_align_up(planes_bytes(out_f, in_f), 256);
  return {c, c + te_align_up(2 * planes_bytes(in_f, out_f), 256)};
}
// weight planes of variant lrp: P3 of W+ at 0 and of W- at wn (rows = out_f, K = in_f), of W+^T at wpT and of W-^T at wnT (rows = in_f, K = out_f)
struct X6WeightPlanesLrp { size_t wn, wpT, wnT, total; };
inline X6WeightPlanesLrp weight_planes_lrp(int64_t in_f, int64_t out_f) {
  const size_t za = te_align_up(planes_bytes(out_f, in_f), 256), ca = te_align_up(planes_bytes(in_f, out_f), 256);
  return {za, 2 * za, 2 * za + ca, 2 * za + 2 * ca};
}

// ---- flags (te_relprop.h) ----
constexpr int kTileMask = TE_X6_TILE_128 | TE_X6_TILE_256 | TE_X6_TILE_128x128;
constexpr int kScheduleFlags = TE_X6_WHOLE_TILES | TE_X6_SLACK_RULE | TE_X6_STATIC_TILES;
constexpr int kProductFlags = kTileMask | kScheduleFlags | TE_X6_TEST_DROP_HANDOVER | TE_X6_TEST_SMALL_GRID;   // plain product, general rule
constexpr int kRuleFlags = kProductFlags | TE_X6_PHASE_MASK | TE_X6_X_PLANES_SIGNED | (kTileMask << TE_X6_TILE_Z_SHIFT) | (kTileMask << TE_X6_TILE_C_SHIFT);

inline int pick_wm(int64_t in_f, int64_t out_f) {
  if (out_f % 256 == 0 && in_f % 128 == 0) return 2;
  if (out_f % 128 == 0 && in_f % 64 == 0) return 1;
  return 0;
}

// wall_clock64 rate of the current device (constant-frequency counter), per device, cached
inline long long spin_ticks_for_current_device() {
  static long long cached[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (cached[dev] == 0) {
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) khz = 100000;
    cached[dev] = (long long)khz * kSpinMillis;
  }
  return cached[dev];
}

// ---- the schedule of one launch: host arithmetic only (te_linear_x6_schedule answers from it without a device) ----
// Stream-K or whole tiles?  With equal (tile, k) ranges the workgroups of an XCD sit at different k offsets of their tiles and
// nothing one of them fetches is still in the 4 MB L2 when its neighbour needs it; cut at tile boundaries they run a round in k
// lock-step on shared operand panels and a K16 step is shorter.  r = tiles per workgroup.  Per K16 step of a tile,
//   whole tiles cost  ceil(r) t_lock       of wall time and  tiles t_lock  of CU-time (a workgroup that is done leaves its CU),
//   stream-K costs    r t_skew(nks)        of wall time and  tiles t_skew  of CU-time (8 spx workgroups for the whole launch),
// so whole tiles always cost less CU-time and are taken where their wall time is within a margin of stream-K's.  Either
// way every output is the same k-ordered chain: results do not change.
// The step times: launch time / (rounds x K16 steps) of the plain products and C-passes on 256 x 256 tiles at T = 12 608, MI355X
// (profiles/x6_schedule_per_launch.log; DESIGN.md section 6 "The x6 schedule"): lock-step 2.27 us at 48 steps (fc1 forward, fc2 input
// gradient: 327 us in 3 rounds) and 2.00 us at 144 / 192 steps (the C-passes of qkv and fc1 on whole tiles), stream-K 2.60 us (293 us
// for r = 2.34) and 2.32 us.  Only their ratio enters (1.15), and it is used for every geometry.
// The margin.  A launch that runs alone pays wall time: kWallMargin = the launch-to-launch spread of those launches (median
// against minimum, 1-4 %).  A caller that packs whole-chip kernels of several streams pays CU-time and says
// so by pinning the call to 256 x 256 tiles -- that is what the pin is for: kWallMarginPacked, between the 600-tile launches (whole
// tiles 12-16 % longer, 13 % less CU-time: the step gains) and the 300-tile C-passes (38-49 % longer: the step loses, 3.1b item 2).
constexpr double kStepLockShort = 2.27, kStepLockLong = 2.00;      // us per K16 step, workgroups of an XCD in k lock-step: nks <= 48 ... >= 144
constexpr double kStepSkewShort = 2.60, kStepSkewLong = 2.32;      // us per K16 step under stream-K cuts
constexpr int kShortSteps = 48, kLongSteps = 144;
constexpr double kWallMargin = 0.05, kWallMarginPacked = 0.20;
constexpr double kWholeTileSlack = 1.15;                           // TE_X6_SLACK_RULE: whole tiles if ceil(r) <= 1.15 r (before the cost rule)
inline double step_time(int nks, double t_short, double t_long) {
  if (nks <= kShortSteps) return t_short;
  if (nks >= kLongSteps) return t_long;
  return t_short + (t_long - t_short) * (nks - kShortSteps) / (kLongSteps - kShortSteps);
}
struct X6Schedule { int ntm, ntn, tiles, spx, whole_tiles; };    // whole_tiles: X6Params' (0 stream-K, 1 static ranges, 2 claimed)
// sched_flags: the call's TE_X6_WHOLE_TILES | TE_X6_SLACK_RULE | TE_X6_STATIC_TILES and its geometry pin (not the per-pass pins)
inline X6Schedule plan_x6(int wm, int64_t T, int rows_w, int nks, int small_grid, int sched_flags) {
  const int tm = (wm == 2) ? 256 : 128, tt = (wm == 0) ? 128 : 256, geo_max_spx = (wm == 2) ? 32 : (wm == 1) ? 64 : 96;   // X6Geo<wm>
  X6Schedule s;
  s.ntm = rows_w / tm;
  s.ntn = (int)te_ceil_div(T, tt);
  const int64_t tiles = (int64_t)s.ntm * s.ntn;
  s.tiles = (int)tiles;
  const int max_spx = small_grid ? 2 : geo_max_spx;
  s.spx = (int)std::min<int64_t>(max_spx, std::max<int64_t>(1, te_ceil_div(tiles, 8)));
  const double r = (double)tiles / (8.0 * s.spx), rounds = std::ceil(r);
  bool whole;
  if (sched_flags & TE_X6_WHOLE_TILES) whole = true;          // the caller runs concurrent streams and wants no hand-over at all
  else if (small_grid) whole = false;                         // the test hook is there for the cuts
  else if (sched_flags & TE_X6_SLACK_RULE) whole = rounds <= kWholeTileSlack * r;
  else {
    const double margin = ((sched_flags & kTileMask) == TE_X6_TILE_256) ? kWallMarginPacked : kWallMargin;
    whole = rounds * step_time(nks, kStepLockShort, kStepLockLong) <= (1.0 + margin) * r * step_time(nks, kStepSkewShort, kStepSkewLong);
  }
  s.whole_tiles = !whole ? 0 : (sched_flags & TE_X6_STATIC_TILES) ? 1 : 2;
  return s;
}

template <int WM, int MODE>
int launch_x6(const X6Params& p, hipStream_t stream) {
  using GEO = X6Geo<WM>;
  static_assert(GEO::TM == ((WM == 2) ? 256 : 128) && GEO::TT == ((WM == 0) ? 128 : 256), "plan_x6 restates the tile sizes");
  constexpr int lds = X6Lds<WM, MODE>::TOTAL;
  static_assert(lds * (WM == 0 ? 3 : WM == 1 ? 2 : 1) <= 160 * 1024, "LDS of the workgroups of one CU");
  static_assert((size_t)8 * GEO::MAX_SPX * GEO::THREADS * GEO::ACC * 4 <= kPartialBytes && 8 * GEO::MAX_SPX < kErrWord, "workspace");
  auto kern = x6_kernel<WM, MODE>;
  // an attribute of the code object ON THE CURRENT DEVICE: set per launch (idempotent, no data-path state)
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e != hipSuccess) return (int)e;
  X6Params q = p;
  // stream-K, static whole-tile ranges or claimed whole tiles: plan_x6 (above), the one place that decides
  const X6Schedule s = plan_x6(WM, p.T, p.rows_w, p.nks, p.small_grid, p.sched_flags);
  static_assert(GEO::MAX_SPX == ((WM == 2) ? 32 : (WM == 1) ? 64 : 96), "plan_x6 restates the grid limit");
  q.ntm = s.ntm;
  q.ntn = s.ntn;
  q.whole_tiles = s.whole_tiles;
  if (!q.status) q.status = q.flags + kErrWord;
  q.spin_ticks = spin_ticks_for_current_device();
  kern<<<dim3(8 * s.spx), dim3(GEO::THREADS), lds, stream>>>(q);
  return TE_OK;
}

template <int MODE>
int launch_x6_mode(int wm, const X6Params& p, hipStream_t stream) {
  if (wm == 2) return launch_x6<2, MODE>(p, stream);
  if (wm == 1) return launch_x6<1, MODE>(p, stream);
  return launch_x6<0, MODE>(p, stream);
}

// Tile geometry of a launch (2 / 1 / 0 = 256 x 256 / 128 x 256 / 128 x 128; the result does not depend on it, bit for bit).
// wm_max = the largest geometry the feature counts divide into; rows_w = weight-side rows; pin = TE_X6_TILE_* or 0.
// small_ok: the launch may use the 128 x 128 geometry (Z-pass, plain products; the C-pass never gains from it).
// Measured per launch on the MI355X (profiles/r04_x6_geometry.log; ViT-B/16 batch 64, BERT-512 batch 32, ViT-L/16-384 batch
// 32): out_f = 768 at T = 12 608 / 16 384 (300 / 384 tiles of 128 x 256) runs 8-15 % faster on 128 x 128 tiles (Z-pass
// 143 -> 121 us and 431 -> 368 us, products 119 -> 106, 401 -> 360, 313 -> 280, 408 -> 368 us); out_f = 1024 at T = 18 464
// (584 tiles) is 10 % faster on 128 x 256.
inline int choose_geo(int wm_max, int64_t T, int64_t rows_w, int pin, int min_tiles_256 = 256, bool small_ok = false) {
  if (pin == TE_X6_TILE_128) return 1;
  if (pin == TE_X6_TILE_256) return wm_max;
  if (pin == TE_X6_TILE_128x128) return 0;
  const int64_t t256 = te_ceil_div(T, 256);
  // 256-row tiles (one 512-thread workgroup per CU, every operand byte staged once for eight waves) where that gives
  // every CU a tile ...
  if (wm_max == 2 && t256 * (rows_w / 256) >= min_tiles_256) return 2;
  // ... 128 x 256 (two workgroups per CU) while there are at least ~1.75 tiles per CU, else 128 x 128 (three per CU)
  if (small_ok && t256 * (rows_w / 128) < 448) return 0;
  return 1;
}
// the geometry of a rule's Z-pass and C-pass (per-pass pins win over the call's pin) and of the plain product [T, K] -> [T, M]:
// 256 weight rows / one 512-thread workgroup per CU where that gives every CU at least one tile, else the smaller tiles
inline int geo_z(int64_t T, int64_t in_f, int64_t out_f, int flags) {
  const int pz = (flags >> TE_X6_TILE_Z_SHIFT) & kTileMask;
  return choose_geo(pick_wm(in_f, out_f), T, out_f, pz ? pz : (flags & kTileMask), 256, true);
}
inline int geo_c(int64_t T, int64_t in_f, int64_t out_f, int flags) {
  const int pc = (flags >> TE_X6_TILE_C_SHIFT) & kTileMask;
  return choose_geo(pick_wm(in_f, out_f), T, 2 * in_f, pc ? pc : (flags & kTileMask));
}
inline int geo_product(int64_t T, int64_t M, int flags) { return choose_geo((M % 256 == 0) ? 2 : 1, T, M, flags & kTileMask, 192, true); }

// ---- X6Params: what every launch of a call shares, then what one pass adds ----
// shape, accumulators, the operands of the plain product's epilogue, the status word and the schedule flags
inline X6Params call_params(int64_t T, float* partial, const float* bias, float* out, unsigned* status, int flags) {
  X6Params p{};
  p.T = T;
  p.ncb = (int)te_ceil_div(T, 32);
  p.partial = partial;
  p.bias = bias;
  p.out = out;
  p.status = status;
  p.drop_handover = (flags & TE_X6_TEST_DROP_HANDOVER) ? 1 : 0;
  p.small_grid = (flags & TE_X6_TEST_SMALL_GRID) ? 1 : 0;
  p.sched_flags = flags & (kScheduleFlags | kTileMask);
  return p;
}
// + the fp32 operands of a rule's epilogues
inline X6Params rule_params(X6Params p, const float* R, const float* r_scale, int64_t r_scale_stride, int64_t rows_per_sample,
                            const float* X, const float* W, const float* Y) {
  p.R = R;
  p.Y = Y;
  p.X = X;
  p.W = W;
  p.rs = r_scale;
  p.rs_stride = r_scale_stride;
  p.rps = (int)(r_scale ? rows_per_sample : 1);
  return p;
}
inline bool bad_r_scale(const float* r_scale, int64_t rows_per_sample, int64_t T) {
  return r_scale && (rows_per_sample <= 0 || rows_per_sample > 0x7fffffff || T % rows_per_sample);
}

// One launch of a Linear layer [T, in_f] -> [T, out_f] on tile geometry wm, with its own flag region.  The mode fixes the shape
// of the product:  Z-like (MODE_Z / ZI / Z1) and the plain product (in_f = K, out_f = M): sums over in_f, out_f weight-side rows;
// C-like (MODE_C / CI): sums over out_f, weight side = the (+, -) pairs of P6 planes, 2 in_f rows;
// MODE_X (out (+)= scale * (X^sign . (S W^t))): sums over out_f, in_f weight-side rows, and the kernel's plain-product naming (K, M).
template <int MODE>
int launch_pass(X6Params p, int wm, const unsigned char* A, const unsigned char* B, unsigned char* S, int64_t in_f,
                int64_t out_f, unsigned* flag_region, hipStream_t stream, float scale = 0.0f, int accum = 0, int x_sign = 0) {
  constexpr bool c_like = MODE == MODE_C || MODE == MODE_CI;
  constexpr bool over_out = c_like || MODE == MODE_X;
  p.A = A, p.B = B, p.S = S;
  p.nks = (int)((over_out ? out_f : in_f) / 16);
  p.a_group_stride = (int64_t)p.nks * (c_like ? 2 : 1) * kRB;
  p.b_rb_stride = (int64_t)p.nks * kRB;
  p.rows_w = (int)(c_like ? 2 * in_f : MODE == MODE_X ? in_f : out_f);
  p.in_f = (int)(MODE == MODE_X ? out_f : in_f);
  p.out_f = (int)(MODE == MODE_X ? in_f : out_f);
  p.scale = scale, p.accum = accum, p.x_sign = x_sign;
  p.flags = flag_region;
  return launch_x6_mode<MODE>(wm, p, stream);
}

// the hand-over flags of `passes` passes start from zero (a kernel, not a memset node: a rule stays a chain of kernel nodes
// when it is captured in a HIP graph)
inline void zero_flag_regions(unsigned* flag_words, int passes, hipStream_t stream) {
  zero_words_kernel<<<dim3(passes * kFlagBytes / 16 / 256), dim3(256), 0, stream>>>(reinterpret_cast<u32x4*>(flag_words));
}

// ---- the plane producers: one argument check, one grid ----
// have_all: no NULL among the pointers; rows >= 1: else INVALID_ARG.  K in K16 steps, the fp32 side 16-byte aligned, rows <= 2^26:
// else UNSUPPORTED.  planes_bytes_ covers [rows, K], the planes 16-byte aligned: else WORKSPACE.
inline int check_producer(bool have_all, bool f32_aligned, bool planes_aligned, int64_t rows, int64_t K, size_t planes_bytes_) {
  if (!have_all || rows < 1) return TE_ERR_INVALID_ARG;
  if (bad_k(K) || !f32_aligned || rows > ((int64_t)1 << 26)) return TE_ERR_UNSUPPORTED;
  if (planes_bytes_ < planes_bytes(rows, K) || !planes_aligned) return TE_ERR_WORKSPACE;
  return TE_OK;
}
// one 256-thread workgroup per 32-row block and eight K16 steps
inline dim3 producer_grid(int64_t rows, int64_t K) { return dim3((unsigned)te_ceil_div(rows, 32), (unsigned)te_ceil_div(K / 16, 8)); }

}  // namespace

// ----------------------------------------------------------------------------------------------------------------------
extern "C" int te_linear_relprop_x6_supported(int64_t T, int64_t in_f, int64_t out_f) {
  return (T >= 1 && in_f >= 128 && out_f >= 128 && pick_wm(in_f, out_f) != 0 && in_f <= (1 << 20) && out_f <= (1 << 20) &&
          T <= (int64_t)1 << 26) ? 1 : 0;
}

extern "C" size_t te_linear_x6_weight_planes_bytes(int64_t in_f, int64_t out_f) {
  return te_linear_relprop_x6_supported(1, in_f, out_f) ? weight_planes(in_f, out_f).total : 0;
}

extern "C" int te_linear_x6_prepare_weights_f32(const float* W, int64_t in_f, int64_t out_f, void* planes,
                                                size_t planes_bytes_, te_stream_t stream_) {
  if (!W || !planes) return TE_ERR_INVALID_ARG;
  if (!te_linear_relprop_x6_supported(1, in_f, out_f) || !te_aligned16(W)) return TE_ERR_UNSUPPORTED;
  if (planes_bytes_ < te_linear_x6_weight_planes_bytes(in_f, out_f) || !te_aligned16(planes)) return TE_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  unsigned char* pz = (unsigned char*)planes;
  unsigned char* pc = pz + weight_planes(in_f, out_f).c;
  split_kernel<OP_ABS, false><<<producer_grid(out_f, in_f), dim3(256), 0, stream>>>(W, pz, out_f, in_f, 3, 0);
  const dim3 gc = producer_grid(in_f, out_f);
  split_kernel<OP_POS, true><<<gc, dim3(256), 0, stream>>>(W, pc, in_f, out_f, 6, 0);
  split_kernel<OP_NEG, true><<<gc, dim3(256), 0, stream>>>(W, pc, in_f, out_f, 6, 1);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

extern "C" size_t te_linear_x6_planes_bytes(int64_t rows, int64_t K) {
  return (rows < 1 || bad_k(K)) ? 0 : planes_bytes(rows, K);
}

extern "C" int te_linear_x6_split_abs_f32(const float* X, int64_t rows, int64_t K, void* planes, size_t planes_bytes_,
                                          te_stream_t stream_) {
  const int rc = check_producer(X && planes, te_aligned16(X), te_aligned16(planes), rows, K, planes_bytes_);
  if (rc != TE_OK) return rc;
  split_kernel<OP_ABS, false><<<producer_grid(rows, K), dim3(256), 0, (hipStream_t)stream_>>>(X, (unsigned char*)planes, rows, K, 3, 0);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

// ---- plain GEMM on the same machinery (the forward / input-gradient products of a Linear layer) -------
// out [T, M] = X [T, K] . Wp^T + bias [M], Wp = signed P3 planes of an [M, K] matrix (te_linear_x6_split_matrix_f32: of W
// itself for the forward product, of W^T for the input gradient d_x = d_y W).
extern "C" int te_gemm_x6_supported(int64_t T, int64_t K, int64_t M) {
  return (T >= 1 && K >= 128 && M >= 128 && K % 16 == 0 && M % 128 == 0 && K <= (1 << 20) && M <= (1 << 20) &&
          T <= (int64_t)1 << 26) ? 1 : 0;
}

extern "C" int te_linear_x6_split_matrix_f32(const float* A, int64_t rows, int64_t K, int transposed, void* planes,
                                             size_t planes_bytes_, te_stream_t stream_) {
  const int rc = check_producer(A && planes, te_aligned16(A), te_aligned16(planes), rows, K, planes_bytes_);
  if (rc != TE_OK) return rc;
  const dim3 grid = producer_grid(rows, K);
  if (transposed)       // A is [K, rows] in memory
    split_kernel<OP_ID, true><<<grid, dim3(256), 0, (hipStream_t)stream_>>>(A, (unsigned char*)planes, rows, K, 3, 0);
  else
    split_kernel<OP_ID, false><<<grid, dim3(256), 0, (hipStream_t)stream_>>>(A, (unsigned char*)planes, rows, K, 3, 0);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

// planes of A [rows, K] AND of |A| from one pass over A (the forward product of a Linear layer wants the first, its
// relprop rule the second: te_linear_relprop_x6_f32's x_planes)
extern "C" int te_linear_x6_split_dual_f32(const float* A, int64_t rows, int64_t K, void* planes, void* planes_abs,
                                           size_t planes_bytes_, te_stream_t stream_) {
  const int rc = check_producer(A && planes && planes_abs, te_aligned16(A), te_aligned16(planes) && te_aligned16(planes_abs), rows, K, planes_bytes_);
  if (rc != TE_OK) return rc;
  split_kernel<OP_ID, false><<<producer_grid(rows, K), dim3(256), 0, (hipStream_t)stream_>>>(A, (unsigned char*)planes, rows, K, 3, 0,
                                                                                           (unsigned char*)planes_abs);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

// GELU producers that write operand planes (gelu_split_lds_kernel above); planes / planes_abs: te_linear_x6_planes_bytes(rows, K)
extern "C" int te_gelu_backward_x6_planes_f32(const float* dy, const float* x, int64_t rows, int64_t K, void* planes,
                                              size_t planes_bytes_, te_stream_t stream_) {
  const int rc = check_producer(dy && x && planes, te_aligned16(dy) && te_aligned16(x), te_aligned16(planes), rows, K, planes_bytes_);
  if (rc != TE_OK) return rc;
  gelu_split_lds_kernel<SRC_GELU_BWD><<<producer_grid(rows, K), dim3(256), 0, (hipStream_t)stream_>>>(
      dy, x, nullptr, (unsigned char*)planes, nullptr, rows, K);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

extern "C" int te_gelu_forward_x6_planes_f32(const float* x, float* y, int64_t rows, int64_t K, void* planes, void* planes_abs,
                                             size_t planes_bytes_, te_stream_t stream_) {
  // planes_abs = NULL: only the signed planes are written (te_linear_relprop_x6_f32 takes them with TE_X6_X_PLANES_SIGNED)
  const int rc = check_producer(x && y && planes, te_aligned16(x) && te_aligned16(y),
                                te_aligned16(planes) && (!planes_abs || te_aligned16(planes_abs)), rows, K, planes_bytes_);
  if (rc != TE_OK) return rc;
  gelu_split_lds_kernel<SRC_GELU_FWD><<<producer_grid(rows, K), dim3(256), 0, (hipStream_t)stream_>>>(
      nullptr, x, y, (unsigned char*)planes, (unsigned char*)planes_abs, rows, K);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

extern "C" size_t te_gemm_x6_workspace_bytes(int64_t T, int64_t K, int64_t M) {
  return te_gemm_x6_supported(T, K, M) ? gemm_workspace(T, K, M).total : 0;
}

extern "C" int te_gemm_x6_f32(const float* X, const void* x_planes, const void* w_planes, const float* bias, float* out,
                              int64_t T, int64_t K, int64_t M, int flags, unsigned* status, void* ws, size_t ws_bytes,
                              te_stream_t stream_) {
  if ((!X && !x_planes) || !w_planes || !out) return TE_ERR_INVALID_ARG;
  if ((flags & ~kProductFlags) != 0) return TE_ERR_INVALID_ARG;
  if (!te_gemm_x6_supported(T, K, M)) return TE_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < te_gemm_x6_workspace_bytes(T, K, M) || !te_aligned16(ws)) return TE_ERR_WORKSPACE;
  if ((X && !te_aligned16(X)) || !te_aligned16(out) || !te_aligned16(w_planes) || (bias && !te_aligned16(bias)) ||
      (x_planes && !te_aligned16(x_planes)))
    return TE_ERR_UNSUPPORTED;
  hipStream_t stream = (hipStream_t)stream_;
  const X6Workspace l = gemm_workspace(T, K, M);
  zero_flag_regions(l.flag_region(ws, 0), 1, stream);
  if (!x_planes) {
    int rc = te_linear_x6_split_matrix_f32(X, T, K, 0, l.x(ws, 0), planes_bytes(T, K), stream_);
    if (rc != TE_OK) return rc;
    x_planes = l.x(ws, 0);
  }
  const int wm = geo_product(T, M, flags);
  const int rc = launch_pass<MODE_G>(call_params(T, l.acc(ws), bias, out, status, flags), wm, (const unsigned char*)w_planes,
                                     (const unsigned char*)x_planes, nullptr, K, M, l.flag_region(ws, 0), stream);
  if (rc != TE_OK) return rc;
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

// workspace: |X| planes, S planes, the accumulators of cut tiles, flags (Z-pass, C-pass)
extern "C" size_t te_linear_relprop_x6_workspace_bytes(int64_t T, int64_t in_f, int64_t out_f) {
  return te_linear_relprop_x6_supported(T, in_f, out_f) ? rule_workspace(T, in_f, out_f).total : 0;
}

extern "C" int te_linear_relprop_x6_f32(const float* R, const float* r_scale, int64_t r_scale_stride,
                                        int64_t rows_per_sample, const float* X, const float* W, const void* w_planes,
                                        const void* x_planes, const float* Y, const float* bias, float* out, int64_t T,
                                        int64_t in_f, int64_t out_f, int flags, unsigned* status, void* ws,
                                        size_t ws_bytes, te_stream_t stream_) {
  // every refusal comes before the first launch: a refused call leaves workspace and out as they were
  if (!R || !X || !W || !w_planes || !Y || !out || T <= 0) return TE_ERR_INVALID_ARG;
  if (!te_linear_relprop_x6_supported(T, in_f, out_f)) return TE_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < te_linear_relprop_x6_workspace_bytes(T, in_f, out_f) || !te_aligned16(ws)) return TE_ERR_WORKSPACE;
  if (!te_aligned16(X) || !te_aligned16(W) || !te_aligned16(R) || !te_aligned16(Y) || !te_aligned16(out) ||
      !te_aligned16(w_planes) || (bias && !te_aligned16(bias)) || (x_planes && !te_aligned16(x_planes)))
    return TE_ERR_UNSUPPORTED;
  if (bad_r_scale(r_scale, rows_per_sample, T)) return TE_ERR_INVALID_ARG;
  if ((flags & ~kRuleFlags) != 0) return TE_ERR_INVALID_ARG;
  const int phases = (flags & TE_X6_PHASE_MASK) ? (flags & TE_X6_PHASE_MASK) : TE_X6_PHASE_MASK;
  hipStream_t stream = (hipStream_t)stream_;
  const X6Workspace l = rule_workspace(T, in_f, out_f);
  unsigned char* Ss = l.sp(ws, 0);
  const unsigned char* wz = (const unsigned char*)w_planes;
  const unsigned char* wc = wz + weight_planes(in_f, out_f).c;

  if (phases & TE_X6_PHASE_SPLIT) zero_flag_regions(l.flag_region(ws, 0), kRulePasses, stream);
  else {   // one phase per call: the tile counters of a claimed launch do not clear themselves as the hand-over flags do
    const int first = (phases & TE_X6_PHASE_Z) ? 0 : 1, last = (phases & TE_X6_PHASE_C) ? 1 : 0;
    zero_flag_regions(l.flag_region(ws, first), last - first + 1, stream);
  }
  const bool x_signed = (flags & TE_X6_X_PLANES_SIGNED) != 0;      // x_planes = the planes of X: the Z-pass forms |X| as it stages them
  if (!x_planes) {
    if (phases & TE_X6_PHASE_SPLIT) {
      int rc = x_signed ? te_linear_x6_split_matrix_f32(X, T, in_f, 0, l.x(ws, 0), planes_bytes(T, in_f), stream_)
                        : te_linear_x6_split_abs_f32(X, T, in_f, l.x(ws, 0), planes_bytes(T, in_f), stream_);
      if (rc != TE_OK) return rc;
    }
    x_planes = l.x(ws, 0);
  }
  // Tile geometry per pass (the result does not depend on it, bit for bit)
  const int wm_z = geo_z(T, in_f, out_f, flags), wm_c = geo_c(T, in_f, out_f, flags);
  const X6Params p = rule_params(call_params(T, l.acc(ws), bias, out, status, flags), R, r_scale, r_scale_stride, rows_per_sample,
                                 X, W, Y);
  int rc;
  if (phases & TE_X6_PHASE_Z) {   // Z-pass: D[j][t] = sum_k |W|[j][k] |X|[t][k]
    rc = x_signed ? launch_pass<MODE_ZS>(p, wm_z, wz, (const unsigned char*)x_planes, Ss, in_f, out_f, l.flag_region(ws, 0), stream, 1.0f)
                  : launch_pass<MODE_Z>(p, wm_z, wz, (const unsigned char*)x_planes, Ss, in_f, out_f, l.flag_region(ws, 0), stream, 1.0f);
    if (rc != TE_OK) return rc;
  }
  if (phases & TE_X6_PHASE_C) {   // C-pass: D[(i, +-)][t] = sum_j W+-[j][i] S[t][j]
    rc = launch_pass<MODE_C>(p, wm_c, wc, Ss, Ss, in_f, out_f, l.flag_region(ws, 1), stream, 1.0f);
    if (rc != TE_OK) return rc;
  }
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

// ----------------------------------------------------------------------------------------------------------------------
// The rule for EVERY variant and alpha on the same kernels: modules/layers_lrp.py:188-211 (variant lrp:
// S1 = sd(R, X+ W+^T), S2 = sd(R, X- W-^T) -- separate denominators) and the inhibitor half of both variants
// (layers_ours.py:225-228: R = alpha * f(pw, nw, px, nx) - beta * f(nw, pw, px, nx), beta = alpha - 1).
//   ours: Z-pass (S) -> C-pass scaled by alpha -> [beta != 0] MODE_ZI (S' from the SAME |X||W|^T product, Z' = ((Y - b) - A)/2)
//         -> MODE_CI: out += -beta (X+ . (S' W-) + X- . (S' W+))                                   18 (+18) bf16 product units
//   lrp : four one-sided launches per half: MODE_Z1 on (W+, X+) -> S1, on (W-, X-) -> S2; MODE_X on (W+^T, S1) masked by X+,
//         on (W-^T, S2) masked by X- (accumulating); the inhibitor half crosses the weight signs.   24 (+24) units
// Every product is an x6 product (six bf16 partial products, fp32 accumulation), every output one k-ordered chain: bitwise
// batch-invariant like the default rule.
extern "C" int te_linear_relprop_x6_general_supported(int64_t T, int64_t in_f, int64_t out_f, int variant) {
  if (!te_linear_relprop_x6_supported(T, in_f, out_f)) return 0;
  if (variant == TE_VARIANT_LRP) return (in_f % 128 == 0) ? 1 : 0;       // the masked products have in_f weight-side rows
  return variant == TE_VARIANT_OURS ? 1 : 0;
}

extern "C" size_t te_linear_x6_weight_planes_lrp_bytes(int64_t in_f, int64_t out_f) {
  return te_linear_relprop_x6_general_supported(1, in_f, out_f, TE_VARIANT_LRP) ? weight_planes_lrp(in_f, out_f).total : 0;
}

extern "C" int te_linear_x6_prepare_weights_lrp_f32(const float* W, int64_t in_f, int64_t out_f, void* planes,
                                                    size_t planes_bytes_, te_stream_t stream_) {
  if (!W || !planes) return TE_ERR_INVALID_ARG;
  if (!te_linear_relprop_x6_general_supported(1, in_f, out_f, TE_VARIANT_LRP) || !te_aligned16(W)) return TE_ERR_UNSUPPORTED;
  if (planes_bytes_ < te_linear_x6_weight_planes_lrp_bytes(in_f, out_f) || !te_aligned16(planes)) return TE_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  unsigned char* q = (unsigned char*)planes;
  const X6WeightPlanesLrp wl = weight_planes_lrp(in_f, out_f);
  const dim3 gz = producer_grid(out_f, in_f), gc = producer_grid(in_f, out_f);
  split_kernel<OP_POS, false><<<gz, dim3(256), 0, stream>>>(W, q, out_f, in_f, 3, 0);
  split_kernel<OP_NEG, false><<<gz, dim3(256), 0, stream>>>(W, q + wl.wn, out_f, in_f, 3, 0);
  split_kernel<OP_POS, true><<<gc, dim3(256), 0, stream>>>(W, q + wl.wpT, in_f, out_f, 3, 0);
  split_kernel<OP_NEG, true><<<gc, dim3(256), 0, stream>>>(W, q + wl.wnT, in_f, out_f, 3, 0);
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

// workspace: two plane sets of the input side (|X|, or X+ and X-), two of the output side (S / S', or S1 and S2), ...
extern "C" size_t te_linear_relprop_x6_general_workspace_bytes(int64_t T, int64_t in_f, int64_t out_f, int variant) {
  return te_linear_relprop_x6_general_supported(T, in_f, out_f, variant) ? general_workspace(T, in_f, out_f).total : 0;
}

extern "C" int te_linear_relprop_x6_general_f32(const float* R, const float* r_scale, int64_t r_scale_stride,
                                                int64_t rows_per_sample, const float* X, const float* W,
                                                const void* w_planes, const void* w_planes_lrp, const void* x_abs_planes,
                                                const float* Y, const float* bias, float* out, int64_t T, int64_t in_f,
                                                int64_t out_f, float alpha, int variant, int flags, unsigned* status,
                                                void* ws, size_t ws_bytes, te_stream_t stream_) {
  if (!R || !X || !W || !out || T <= 0) return TE_ERR_INVALID_ARG;
  if (!te_linear_relprop_x6_general_supported(T, in_f, out_f, variant)) return TE_ERR_UNSUPPORTED;
  const bool lrp = variant == TE_VARIANT_LRP;
  if (lrp ? !w_planes_lrp : (!w_planes || !Y)) return TE_ERR_INVALID_ARG;
  if (!ws || ws_bytes < te_linear_relprop_x6_general_workspace_bytes(T, in_f, out_f, variant) || !te_aligned16(ws))
    return TE_ERR_WORKSPACE;
  if (!te_aligned16(X) || !te_aligned16(W) || !te_aligned16(R) || (Y && !te_aligned16(Y)) || !te_aligned16(out) ||
      (w_planes && !te_aligned16(w_planes)) || (w_planes_lrp && !te_aligned16(w_planes_lrp)) ||
      (bias && !te_aligned16(bias)) || (x_abs_planes && !te_aligned16(x_abs_planes)))
    return TE_ERR_UNSUPPORTED;
  if (bad_r_scale(r_scale, rows_per_sample, T)) return TE_ERR_INVALID_ARG;
  if ((flags & ~kProductFlags) != 0) return TE_ERR_INVALID_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  const float beta = alpha - 1.0f;
  const X6Workspace l = general_workspace(T, in_f, out_f);
  unsigned char* Xa = l.x(ws, 0), *Xb = l.x(ws, 1);        // |X|, -      or X+, X-
  unsigned char* Sa = l.sp(ws, 0), *Sb = l.sp(ws, 1);      // S / S', -   or S1, S2
  zero_flag_regions(l.flag_region(ws, 0), kGeneralPasses, stream);

  // status = NULL: ONE per-call error word for all launches of the rule, in the last flag region -- which no launch uses (at
  // most four passes per half) and which the reset between the two halves of variant lrp leaves alone, so a failure of the
  // first half is not lost
  const X6Params p = rule_params(call_params(T, l.acc(ws), bias, out, status ? status : l.flag_region(ws, kGeneralPasses - 1) + kErrWord, flags),
                                 R, r_scale, r_scale_stride, rows_per_sample, X, W, Y);
  const int pin = flags & kTileMask;
  const int wm_z = choose_geo(pick_wm(in_f, out_f), T, out_f, pin, 256, true);
  int pass = 0;          // every launch takes the next flag region
  int rc;
  if (!lrp) {
    const unsigned char* wz = (const unsigned char*)w_planes;
    const unsigned char* wc = wz + weight_planes(in_f, out_f).c;
    if (!x_abs_planes) {
      rc = te_linear_x6_split_abs_f32(X, T, in_f, Xa, planes_bytes(T, in_f), stream_);
      if (rc != TE_OK) return rc;
      x_abs_planes = Xa;
    }
    const int wm_c = choose_geo(pick_wm(in_f, out_f), T, 2 * in_f, pin);
    rc = launch_pass<MODE_Z>(p, wm_z, wz, (const unsigned char*)x_abs_planes, Sa, in_f, out_f, l.flag_region(ws, pass++), stream);
    if (rc != TE_OK) return rc;
    rc = launch_pass<MODE_C>(p, wm_c, wc, Sa, nullptr, in_f, out_f, l.flag_region(ws, pass++), stream, alpha);
    if (rc != TE_OK) return rc;
    if (beta != 0.0f) {
      rc = launch_pass<MODE_ZI>(p, wm_z, wz, (const unsigned char*)x_abs_planes, Sa, in_f, out_f, l.flag_region(ws, pass++), stream);      // S' over S
      if (rc != TE_OK) return rc;
      rc = launch_pass<MODE_CI>(p, wm_c, wc, Sa, nullptr, in_f, out_f, l.flag_region(ws, pass++), stream, -beta);
      if (rc != TE_OK) return rc;
    }
  } else {
    const X6WeightPlanesLrp wl = weight_planes_lrp(in_f, out_f);
    const unsigned char* Wp = (const unsigned char*)w_planes_lrp;
    const unsigned char* Wn = Wp + wl.wn, *WpT = Wp + wl.wpT, *WnT = Wp + wl.wnT;
    split_kernel<OP_POS, false><<<producer_grid(T, in_f), dim3(256), 0, stream>>>(X, Xa, T, in_f, 3, 0);
    split_kernel<OP_NEG, false><<<producer_grid(T, in_f), dim3(256), 0, stream>>>(X, Xb, T, in_f, 3, 0);
    // out (+)= scale * (X^sign . (S W^t)):  product [T, out_f] x [out_f, in_f], weight-side rows = in_f
    const int wm_x = choose_geo((in_f % 256 == 0) ? 2 : 1, T, in_f, pin, 192, true);
    auto x_pass = [&](const unsigned char* AT, const unsigned char* S, int sign, float scale, int accum) -> int {
      return launch_pass<MODE_X>(p, wm_x, AT, S, nullptr, in_f, out_f, l.flag_region(ws, pass++), stream, scale, accum, sign);
    };
    for (int half = 0; half < (beta != 0.0f ? 2 : 1); ++half) {
      // half 0: f(pw, nw, px, nx) (activator); half 1: f(nw, pw, px, nx) (inhibitor) -- the weight signs cross
      const unsigned char* w1 = half ? Wn : Wp, *w2 = half ? Wp : Wn, *w1T = half ? WnT : WpT, *w2T = half ? WpT : WnT;
      const float sc = half ? -beta : alpha;
      if (half) {       // the second half reuses the flag regions of the first: reset them (stream-ordered after their use)
        pass = 0;
        static_assert(kGeneralPasses >= 5, "four passes per half + the region of the per-call error word");
        zero_flag_regions(l.flag_region(ws, 0), 4, stream);
      }
      rc = launch_pass<MODE_Z1>(p, wm_z, w1, Xa, Sa, in_f, out_f, l.flag_region(ws, pass++), stream);
      if (rc != TE_OK) return rc;
      rc = launch_pass<MODE_Z1>(p, wm_z, w2, Xb, Sb, in_f, out_f, l.flag_region(ws, pass++), stream);
      if (rc != TE_OK) return rc;
      rc = x_pass(w1T, Sa, +1, sc, half);
      if (rc != TE_OK) return rc;
      rc = x_pass(w2T, Sb, -1, sc, 1);
      if (rc != TE_OK) return rc;
    }
  }
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

// What a launch of this shape would do: geometry, schedule and grid, from the same functions the entry points call.  Host arithmetic
// only: no device is needed or touched.
extern "C" int te_linear_x6_schedule(int64_t T, int64_t in_f, int64_t out_f, int pass, int flags, int* schedule) {
  if (!schedule) return TE_ERR_INVALID_ARG;
  const bool product = pass == TE_X6_PASS_PRODUCT;
  if (pass != TE_X6_PASS_Z && pass != TE_X6_PASS_C && !product) return TE_ERR_INVALID_ARG;
  if ((flags & ~(product ? kProductFlags : kRuleFlags)) != 0) return TE_ERR_INVALID_ARG;
  if (!(product ? te_gemm_x6_supported(T, in_f, out_f) : te_linear_relprop_x6_supported(T, in_f, out_f))) return TE_ERR_UNSUPPORTED;
  const bool c = pass == TE_X6_PASS_C;
  const int wm = product ? geo_product(T, out_f, flags) : c ? geo_c(T, in_f, out_f, flags) : geo_z(T, in_f, out_f, flags);
  const X6Schedule s = plan_x6(wm, T, (int)(c ? 2 * in_f : out_f), (int)((c ? out_f : in_f) / 16),
                               (flags & TE_X6_TEST_SMALL_GRID) ? 1 : 0, flags & (kScheduleFlags | kTileMask));
  schedule[0] = wm == 2 ? TE_X6_TILE_256 : wm == 1 ? TE_X6_TILE_128 : TE_X6_TILE_128x128;
  schedule[1] = s.whole_tiles;
  schedule[2] = 8 * s.spx;
  schedule[3] = s.tiles;
  return TE_OK;
}

// 1 if a bounded wait of the last te_linear_relprop_x6_f32 call on this workspace expired (a predecessor workgroup never
// published its accumulators): the result of that call is invalid.  Synchronises the stream.
extern "C" int te_linear_relprop_x6_check(const void* ws, int64_t T, int64_t in_f, int64_t out_f, te_stream_t stream_) {
  if (!ws || !te_linear_relprop_x6_supported(T, in_f, out_f)) return TE_ERR_INVALID_ARG;
  const X6Workspace l = rule_workspace(T, in_f, out_f);
  unsigned host[kRulePasses][kUsedFlagWords];      // the 512 flags + the error word of each pass
  hipError_t e = hipSuccess;
  for (int pass = 0; pass < kRulePasses && e == hipSuccess; ++pass)
    e = hipMemcpyAsync(host[pass], l.flag_region(ws, pass), sizeof(host[pass]), hipMemcpyDeviceToHost, (hipStream_t)stream_);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream_);
  if (e != hipSuccess) return (int)e;
  // any non-zero word after a completed call is an error (a flag nobody consumed, or the error word)
  for (int pass = 0; pass < kRulePasses; ++pass)
    for (int i = 0; i < kUsedFlagWords; ++i)
      if (host[pass][i]) return 1;
  return 0;
}
