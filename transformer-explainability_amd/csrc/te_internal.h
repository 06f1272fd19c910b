// te_internal.h -- the launchers one translation unit of libte_relprop defines and another calls, each declared ONCE (default
// arguments included).  The defining file and every caller include this header; the comments are the map of the dispatch:
// which file, which round, which shapes.  Nothing here is part of the C ABI (include/te_relprop.h).
#pragma once

#include "te_common.h"

// te_linear.hip: the LDS-tiled C-pass of the z^B rule on the im2col view of a patch embedding (caller: te_conv.hip); false if
// the shape is not covered by the tiled kernel
bool te_internal_zb_cpass_tiled(const float* S, const float* W, const float* X, float* out, int64_t T, int64_t in_f,
                                int64_t out_f, const TeZbGeom& zb, hipStream_t stream);

namespace te_attn_mfma {    // te_attn_mfma.hip: LDS-tiled fp32-MFMA rule kernels (round 1), any N with head dim 64; they hand over to te_attn_rules
// (callers: te_attn.hip, te_rollout.hip)  the *_supported return false if the shape is not covered by the tiled kernels
bool av_supported(int64_t N, int64_t D);
int av_launch(const float* R, int64_t r_sb, int64_t r_sh, int64_t r_sn, const float* attn,
              const float* v, int64_t v_sb, int64_t v_sh, int64_t v_sn, const float* Z, int64_t z_sb, int64_t z_sh,
              int64_t z_sn, float* cam_attn, float* cam_v, int64_t cv_sb, int64_t cv_sh, int64_t cv_sn, int64_t B,
              int64_t H, int64_t N, int64_t D, float scale, float* ws, hipStream_t stream);
bool qk_supported(int64_t N, int64_t D);
int qk_launch(const float* Rnn, const float* q, int64_t q_sb, int64_t q_sh, int64_t q_sn,
              const float* k, int64_t k_sb, int64_t k_sh, int64_t k_sn, const float* Z, float* cam_q, int64_t cq_sb,
              int64_t cq_sh, int64_t cq_sn, float* cam_k, int64_t ck_sb, int64_t ck_sh, int64_t ck_sn,
              int64_t B, int64_t H, int64_t N, int64_t D, float scale, float* ws, const float* r_scale,
              int64_t r_scale_stride, hipStream_t stream);
int rollout_bmm_launch(const float* A, const float* Bm, float* C, int64_t B, int64_t N, hipStream_t stream);
}  // namespace te_attn_mfma

namespace te_attn_rules {   // te_attn_rules.hip: the one-pass rule kernels (default)
bool supported(int64_t B, int64_t H, int64_t N, int64_t D);
int av_launch(const float* R, int64_t r_sb, int64_t r_sh, int64_t r_sn, const float* attn, const float* v, int64_t v_sb,
              int64_t v_sh, int64_t v_sn, const float* Z, int64_t z_sb, int64_t z_sh, int64_t z_sn, float* cam_attn,
              float* cam_v, int64_t cv_sb, int64_t cv_sh, int64_t cv_sn, int64_t B, int64_t H, int64_t N, float scale,
              hipStream_t stream);
int qk_launch(const float* Rnn, const float* q, int64_t q_sb, int64_t q_sh, int64_t q_sn, const float* k, int64_t k_sb,
              int64_t k_sh, int64_t k_sn, const float* Z, float* cam_q, int64_t cq_sb, int64_t cq_sh, int64_t cq_sn,
              float* cam_k, int64_t ck_sb, int64_t ck_sh, int64_t ck_sn, int64_t B, int64_t H, int64_t N, float scale,
              float* qpart, const float* r_scale, int64_t r_scale_stride, hipStream_t stream);
}  // namespace te_attn_rules

namespace te_attn_kb {      // te_attn_kb.hip: wave-owned key blocks (round 5) -- the AV rule and the first half of the backward
bool supported(int64_t B, int64_t H, int64_t N, int64_t D);
int av_launch(int mode, const float* R, int64_t r_sb, int64_t r_sh, int64_t r_sn, const float* attn, const float* v,
              int64_t v_sb, int64_t v_sh, int64_t v_sn, const float* Z, int64_t z_sb, int64_t z_sh, int64_t z_sn,
              float* cam_attn, float* cam_v, int64_t cv_sb, int64_t cv_sh, int64_t cv_sn, int64_t B, int64_t H, int64_t N,
              float scale, hipStream_t stream);
}  // namespace te_attn_kb

namespace te_attn_rc {      // te_attn_rc.hip: row-block and key-block owners (round 6) -- the QK rule / softmax backward, N <= 224
bool supported(int64_t B, int64_t H, int64_t N, int64_t D);
int qk_launch(int mode, const float* Rnn, const float* q, int64_t q_sb, int64_t q_sh, int64_t q_sn, const float* k, int64_t k_sb,
              int64_t k_sh, int64_t k_sn, const float* Z, float* cam_q, int64_t cq_sb, int64_t cq_sh, int64_t cq_sn, float* cam_k,
              int64_t ck_sb, int64_t ck_sh, int64_t ck_sn, int64_t B, int64_t H, int64_t N, float scale, const float* r_scale,
              int64_t r_scale_stride, hipStream_t stream, const float* d_out = nullptr, const float* out = nullptr, int64_t o_sb = 0,
              int64_t o_sh = 0, int64_t o_sn = 0);
}  // namespace te_attn_rc

namespace te_attn_fwd6 {      // te_attn_fwd6.hip: row-block owners on bf16 MFMAs (round 6) -- the attention forward, N <= 224
bool supported(int64_t B, int64_t H, int64_t N, int64_t D);
int launch(const float* qkv, float* z_qk, float* attn, float* out, int64_t B, int64_t H, int64_t N, float scale, hipStream_t stream,
           void* out_planes = nullptr, void* out_abs_planes = nullptr);
}  // namespace te_attn_fwd6

namespace te_attn_fwd6l {      // te_attn_fwd6l.hip: row-block owners on bf16 MFMAs, two walks over the keys (round 6) -- the default forward, 64 < N <= 640
bool supported(int64_t B, int64_t H, int64_t N, int64_t D);
int launch(const float* q, int64_t q_sb, int64_t q_sh, int64_t q_sn, const float* k, int64_t k_sb, int64_t k_sh, int64_t k_sn,
           const float* v, int64_t v_sb, int64_t v_sh, int64_t v_sn, const float* mask, float* z_qk, float* x_scaled, float* attn,
           float* out, int64_t o_sb, int64_t o_sh, int64_t o_sn, int64_t B, int64_t H, int64_t N, float scale, hipStream_t stream);
}  // namespace te_attn_fwd6l

namespace te_attn_bwd6l {      // te_attn_bwd6l.hip: the row side of the backward pass in the same structure (round 6), 64 < N <= 640
bool supported(int64_t B, int64_t H, int64_t N, int64_t D);
int launch_rows(const float* d_out, int64_t do_sb, int64_t do_sh, int64_t do_sn, const float* out, int64_t o_sb, int64_t o_sh,
                int64_t o_sn, const float* k, int64_t k_sb, int64_t k_sh, int64_t k_sn, const float* v, int64_t v_sb, int64_t v_sh,
                int64_t v_sn, const float* attn, float* d_attn, float* rowdot, float* d_q, int64_t dq_sb, int64_t dq_sh, int64_t dq_sn,
                int64_t B, int64_t H, int64_t N, float scale, int need_qk, hipStream_t stream);
int launch_cols(const float* attn, const float* d_attn, const float* rowdot, const float* d_out, int64_t do_sb, int64_t do_sh, int64_t do_sn,
                const float* q, int64_t q_sb, int64_t q_sh, int64_t q_sn, float* d_v, int64_t dv_sb, int64_t dv_sh, int64_t dv_sn, float* d_k,
                int64_t dk_sb, int64_t dk_sh, int64_t dk_sn, int64_t B, int64_t H, int64_t N, float scale, int need_qk, hipStream_t stream);
}  // namespace te_attn_bwd6l
