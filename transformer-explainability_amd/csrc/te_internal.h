// te_internal.h -- the launchers one translation unit of libte_relprop defines and another calls, each declared ONCE (default
// arguments included).  The defining file and every caller include this header; the comments are the map of the dispatch:
// which file, which round, which shapes.  Nothing here is part of the C ABI (include/te_relprop.h).
#pragma once

#include "te_common.h"

// te_linear.hip: the LDS-tiled C-pass of the z^B rule on the im2col view of a patch embedding (caller: te_conv.hip); false if
// the shape is not covered by the tiled kernel
bool te_internal_zb_cpass_tiled(const float* S, const float* W, const float* X, float* out, int64_t T, int64_t in_f,
                                int64_t out_f, const TeZbGeom& zb, hipStream_t stream);

// The fp32 attention launchers below have ONE caller, the dispatch in te_attn.hip (te_rollout.hip for the rollout product): no
// launcher calls a launcher of another file.  A [B,H,N,64] view crosses a file boundary as (pointer, Strided).
enum { TE_ATTN_RULE = 0, TE_ATTN_BWD = 1 };      // `mode` of the launchers that serve a relprop rule and the attention backward

namespace te_attn_mfma {    // te_attn_mfma.hip: LDS-tiled fp32-MFMA rule kernels (round 1), any N <= 2^20 with head dim 64; Z for callers without one
bool supported(int64_t N, int64_t D);
int z_av_launch(const float* attn, const float* v, Strided vs, float* Z, int64_t B, int64_t H, int64_t N, hipStream_t stream);
int z_qk_launch(const float* q, Strided qs, const float* k, Strided ks, float* Z, int64_t B, int64_t H, int64_t N, hipStream_t stream);
int av_launch(const float* R, Strided rs, const float* attn, const float* v, Strided vs, const float* Z, Strided zs, float* cam_attn,
              float* cam_v, Strided cs, int64_t B, int64_t H, int64_t N, float scale, float* S, hipStream_t stream);
int qk_launch(const float* Rnn, const float* q, Strided qs, const float* k, Strided ks, const float* Z, float* cam_q, Strided cqs,
              float* cam_k, Strided cks, int64_t B, int64_t H, int64_t N, float scale, float* S, hipStream_t stream);
int rollout_bmm_launch(const float* A, const float* Bm, float* C, int64_t B, int64_t N, hipStream_t stream);
}  // namespace te_attn_mfma

namespace te_attn_rules {   // te_attn_rules.hip: the one-pass kernel (round 2) -- the QK rule for 224 < N <= 4096, the softmax backward for 160 < N <= 224
bool supported(int64_t B, int64_t H, int64_t N, int64_t D);
int qk_launch(int mode, const float* Rnn, const float* q, Strided qs, const float* k, Strided ks, const float* Z, float* cam_q,
              Strided cqs, float* cam_k, Strided cks, int64_t B, int64_t H, int64_t N, float scale, float* qpart, const float* r_scale,
              int64_t r_scale_stride, hipStream_t stream);
}  // namespace te_attn_rules

namespace te_attn_kb {      // te_attn_kb.hip: wave-owned key blocks (round 5) -- the AV rule (N <= 4096) and the first half of the backward
bool supported(int64_t B, int64_t H, int64_t N, int64_t D);
int av_launch(int mode, const float* R, Strided rs, const float* attn, const float* v, Strided vs, const float* Z, Strided zs,
              float* cam_attn, float* cam_v, Strided cs, int64_t B, int64_t H, int64_t N, float scale, hipStream_t stream);
}  // namespace te_attn_kb

namespace te_attn_rc {      // te_attn_rc.hip: row-block and key-block owners (round 6) -- the QK rule / softmax backward, N <= 224
bool supported(int64_t B, int64_t H, int64_t N, int64_t D);
int qk_launch(int mode, const float* Rnn, const float* q, Strided qs, const float* k, Strided ks, const float* Z, float* cam_q,
              Strided cqs, float* cam_k, Strided cks, int64_t B, int64_t H, int64_t N, float scale, const float* r_scale,
              int64_t r_scale_stride, hipStream_t stream, const float* d_out = nullptr, const float* out = nullptr, Strided os = Strided());
}  // namespace te_attn_rc

namespace te_attn_fwd6 {      // te_attn_fwd6.hip: row-block owners on bf16 MFMAs (round 6) -- the attention forward, N <= 224
bool supported(int64_t B, int64_t H, int64_t N, int64_t D);
int launch(const float* qkv, float* z_qk, float* attn, float* out, int64_t B, int64_t H, int64_t N, float scale, hipStream_t stream,
           void* out_planes = nullptr, void* out_abs_planes = nullptr);
}  // namespace te_attn_fwd6

namespace te_attn_fwd6l {      // te_attn_fwd6l.hip: row-block owners on bf16 MFMAs, two walks over the keys (round 6) -- the default forward, 64 < N <= 640
bool supported(int64_t B, int64_t H, int64_t N, int64_t D);
int launch(const float* q, Strided qs, const float* k, Strided ks, const float* v, Strided vs, const float* mask, float* z_qk,
           float* x_scaled, float* attn, float* out, Strided os, int64_t B, int64_t H, int64_t N, float scale, hipStream_t stream);
}  // namespace te_attn_fwd6l

namespace te_attn_bwd6l {      // te_attn_bwd6l.hip: both sides of the backward pass in the same structure (round 6), 64 < N <= 640
bool supported(int64_t B, int64_t H, int64_t N, int64_t D);
int launch_rows(const float* d_out, Strided dos, const float* out, Strided os, const float* k, Strided ks, const float* v, Strided vs,
                const float* attn, float* d_attn, float* rowdot, float* d_q, Strided dqs, int64_t B, int64_t H, int64_t N, float scale,
                int need_qk, hipStream_t stream);
int launch_cols(const float* attn, const float* d_attn, const float* rowdot, const float* d_out, Strided dos, const float* q, Strided qs,
                float* d_v, Strided dvs, float* d_k, Strided dks, int64_t B, int64_t H, int64_t N, float scale, int need_qk,
                hipStream_t stream);
}  // namespace te_attn_bwd6l

namespace te_attn_long {      // te_attn_long.hip: row-tile producers on fp32 MFMAs (round 3), N <= 640 -- what the round-6 files do not take
bool supported(int64_t B, int64_t H, int64_t N, int64_t D);
bool strides_ok(Strided s);      // 16-byte pieces of rows of at least 64 floats: asked of every view of a strided producer call
int fwd_launch(const float* q, Strided qs, const float* k, Strided ks, const float* v, Strided vs, const float* mask, float* z_qk,
               float* x_scaled, float* attn, float* out, Strided os, int64_t B, int64_t H, int64_t N, float scale, hipStream_t stream);
int bwd_rows_launch(const float* d_out, Strided dos, const float* k, Strided ks, const float* v, Strided vs, const float* attn, float* d_attn,
                    float* rowdot, float* d_q, Strided dqs, int64_t B, int64_t H, int64_t N, float scale, int need_qk, hipStream_t stream);
int bwd_cols_launch(const float* attn, const float* d_attn, const float* rowdot, const float* d_out, Strided dos, const float* q, Strided qs,
                    float* d_v, Strided dvs, float* d_k, Strided dks, int64_t B, int64_t H, int64_t N, float scale, int need_qk,
                    hipStream_t stream);
}  // namespace te_attn_long

namespace te_alrp {      // te_attnlrp.hip: the streaming passes that hand an fp32 operand to a product on bf16 MFMAs as three exact bf16 planes (caller: te_bf16.hip)
// planes [3][B H N][C] of damp(G, Y) (Y == nullptr: of G itself); row (b, h, n) of G / Y at the strides, C contiguous elements
int damp_planes_launch(const float* G, Strided gs, const te_bf16_t* Y, Strided ys, uint16_t* planes, int64_t B, int64_t H, int64_t N,
                       int64_t C, float eps, hipStream_t stream);
// planes [3][rows][N] of d_s = p (.) (d_attn - sum_j d_attn (.) p): d_attn fp32 [rows][N], p bf16 [rows][N], both contiguous
int softmax_bwd_planes_launch(const float* d_attn, const te_bf16_t* p, uint16_t* planes, int64_t rows, int64_t N, hipStream_t stream);
}  // namespace te_alrp
