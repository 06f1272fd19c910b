// te_attn.hip -- einsum / MatMul relprop of self-attention (modules/layers_ours.py:48-60,122-127;
// BERT_explainability/modules/layers_ours.py:89-91) for gfx950.
//
//   AV rule:  Z = attn v ; S = sd(R, Z) ; cam_attn = attn .(S v^T) ; cam_v = v .(attn^T S)
//   QK rule:  Z = q k^T  ; S = sd(R, Z) ; cam_q = q .(S k)         ; cam_k = k .(S^T q)
//
// q / k / v / R(AV) / cam_q / cam_k / cam_v are strided [B,H,N,D] views (element (b,h,n,d) at
// base + b*sb + h*sh + n*sn + d) so the fused qkv activation and the 'b n (qkv h d)' relevance layout
// are read and written in place -- the reference's four einops rearrange copies per block
// (ViT_LRP.py:135,148,157,175) do not exist here.
//
// This file is the DISPATCH of every fp32 attention call: it holds the extern "C" entry points of the rules and of the producers
// (attention forward / backward on the fused qkv activation and on strided q / k / v views), their argument checks, the partition
// of their workspaces, and per entry point one chain of `if (X::supported(...)) return X::launch(...)` in the order of preference,
// each line with its reason.  The kernels live in te_attn_{kb,rc,rules,mfma,fwd6,fwd6l,bwd6l,long}.hip, whose host side only launches
// (te_internal.h: which file, which round, which shapes); a launcher that refuses ends the call.  A new kernel is one more line here.
//
// The SIMPLE kernels below (one thread per output element, k-ordered fmaf chains) are the dispatch's own last resort: the rules
// with TE_IMPL_SIMPLE set or a head dim other than 64.
#include "te_internal.h"

namespace {

constexpr int kThreads = 256;

// S[b,h,i,d] = sd(R[b,h,i,d], sum_j attn[b,h,i,j] v[b,h,j,d])             (contiguous workspace)
__global__ __launch_bounds__(kThreads) void av_s_simple(
    const float* __restrict__ R, Strided rs, const float* __restrict__ attn, const float* __restrict__ v,
    Strided vs, float* __restrict__ S, int64_t B, int64_t H, int64_t N, int64_t D) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= B * H * N * D) return;
  const int64_t d = idx % D, i = (idx / D) % N, h = (idx / (D * N)) % H, b = idx / (D * N * H);
  const float* arow = attn + ((b * H + h) * N + i) * N;
  float z = 0.0f;
  for (int64_t j = 0; j < N; ++j) z = fmaf(arow[j], v[vs.at(b, h, j) + d], z);
  S[idx] = te_sd(R[rs.at(b, h, i) + d], z);
}

// the same with Z = the cached forward product attn v, contiguous [B,H,N,D]
__global__ __launch_bounds__(kThreads) void av_s_from_z_simple(
    const float* __restrict__ R, Strided rs, const float* __restrict__ Z, float* __restrict__ S, int64_t B, int64_t H,
    int64_t N, int64_t D) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= B * H * N * D) return;
  const int64_t d = idx % D, i = (idx / D) % N, h = (idx / (D * N)) % H, b = idx / (D * N * H);
  S[idx] = te_sd(R[rs.at(b, h, i) + d], Z[idx]);
}
__global__ __launch_bounds__(kThreads) void qk_s_from_z_simple(const float* __restrict__ R, const float* __restrict__ Z,
                                                               float* __restrict__ S, int64_t n) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx < n) S[idx] = te_sd(R[idx], Z[idx]);
}

// cam_attn[b,h,i,j] = attn[b,h,i,j] * (sum_d S[b,h,i,d] v[b,h,j,d]) * scale
__global__ __launch_bounds__(kThreads) void av_cam_attn_simple(
    const float* __restrict__ S, const float* __restrict__ attn, const float* __restrict__ v, Strided vs,
    float* __restrict__ cam, int64_t B, int64_t H, int64_t N, int64_t D, float scale) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= B * H * N * N) return;
  const int64_t j = idx % N, i = (idx / N) % N, h = (idx / (N * N)) % H, b = idx / (N * N * H);
  const float* srow = S + ((b * H + h) * N + i) * D;
  const float* vrow = v + vs.at(b, h, j);
  float g = 0.0f;
  for (int64_t d = 0; d < D; ++d) g = fmaf(srow[d], vrow[d], g);
  cam[idx] = (attn[idx] * g) * scale;
}

// cam_v[b,h,j,d] = v[b,h,j,d] * (sum_i attn[b,h,i,j] S[b,h,i,d]) * scale
__global__ __launch_bounds__(kThreads) void av_cam_v_simple(
    const float* __restrict__ S, const float* __restrict__ attn, const float* __restrict__ v, Strided vs,
    float* __restrict__ cam_v, Strided cs, int64_t B, int64_t H, int64_t N, int64_t D, float scale) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= B * H * N * D) return;
  const int64_t d = idx % D, j = (idx / D) % N, h = (idx / (D * N)) % H, b = idx / (D * N * H);
  const float* a = attn + (b * H + h) * N * N + j;
  const float* s = S + (b * H + h) * N * D + d;
  float u = 0.0f;
  for (int64_t i = 0; i < N; ++i) u = fmaf(a[i * N], s[i * D], u);
  cam_v[cs.at(b, h, j) + d] = (v[vs.at(b, h, j) + d] * u) * scale;
}

// S[b,h,i,j] = sd(R[b,h,i,j], sum_d q[b,h,i,d] k[b,h,j,d])
__global__ __launch_bounds__(kThreads) void qk_s_simple(
    const float* __restrict__ R, const float* __restrict__ q, Strided qs, const float* __restrict__ k,
    Strided ks, float* __restrict__ S, int64_t B, int64_t H, int64_t N, int64_t D) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= B * H * N * N) return;
  const int64_t j = idx % N, i = (idx / N) % N, h = (idx / (N * N)) % H, b = idx / (N * N * H);
  const float* qrow = q + qs.at(b, h, i);
  const float* krow = k + ks.at(b, h, j);
  float z = 0.0f;
  for (int64_t d = 0; d < D; ++d) z = fmaf(qrow[d], krow[d], z);
  S[idx] = te_sd(R[idx], z);
}

// cam_q[b,h,i,d] = q[b,h,i,d] * (sum_j S[b,h,i,j] k[b,h,j,d]) * scale
__global__ __launch_bounds__(kThreads) void qk_cam_q_simple(
    const float* __restrict__ S, const float* __restrict__ q, Strided qs, const float* __restrict__ k,
    Strided ks, float* __restrict__ cam_q, Strided cs, int64_t B, int64_t H, int64_t N, int64_t D, float scale) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= B * H * N * D) return;
  const int64_t d = idx % D, i = (idx / D) % N, h = (idx / (D * N)) % H, b = idx / (D * N * H);
  const float* srow = S + ((b * H + h) * N + i) * N;
  float u = 0.0f;
  for (int64_t j = 0; j < N; ++j) u = fmaf(srow[j], k[ks.at(b, h, j) + d], u);
  cam_q[cs.at(b, h, i) + d] = (q[qs.at(b, h, i) + d] * u) * scale;
}

// cam_k[b,h,j,d] = k[b,h,j,d] * (sum_i S[b,h,i,j] q[b,h,i,d]) * scale
__global__ __launch_bounds__(kThreads) void qk_cam_k_simple(
    const float* __restrict__ S, const float* __restrict__ q, Strided qs, const float* __restrict__ k,
    Strided ks, float* __restrict__ cam_k, Strided cs, int64_t B, int64_t H, int64_t N, int64_t D, float scale) {
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= B * H * N * D) return;
  const int64_t d = idx % D, j = (idx / D) % N, h = (idx / (D * N)) % H, b = idx / (D * N * H);
  const float* s = S + (b * H + h) * N * N + j;
  float u = 0.0f;
  for (int64_t i = 0; i < N; ++i) u = fmaf(s[i * N], q[qs.at(b, h, i) + d], u);
  cam_k[cs.at(b, h, j) + d] = (k[ks.at(b, h, j) + d] * u) * scale;
}

// (not te_attn_long::strides_ok, which asks for 16-byte rows: the rule kernels take any non-negative strides)
inline bool view_ok(Strided s) { return s.sb >= 0 && s.sh >= 0 && s.sn > 0; }

// what every entry point does with its launcher's answer: a refusal ends the call (no fall-through to an older kernel)
inline int finish(int rc) {
  if (rc != TE_OK) return rc;
  TE_RETURN_IF_LAUNCH_FAILED();
  return TE_OK;
}

}  // namespace

// ================================================================================================
// The relprop rules.  Workspace of both: S, then Z of the same size (Z only for a caller without the cached forward product).
// ================================================================================================
extern "C" size_t te_matmul_relprop_av_workspace_bytes(int64_t B, int64_t H, int64_t N, int64_t D) {
  if (B <= 0 || H <= 0 || N <= 0 || D <= 0) return 0;
  return te_align_up((size_t)2 * B * H * N * D * sizeof(float), 256);
}

// Z (optional): the cached forward product attn v, element (b,h,n,d) at Z + b*z_sb + h*z_sh + n*z_sn + d
extern "C" int te_matmul_relprop_av_f32(const float* R, int64_t r_sb, int64_t r_sh, int64_t r_sn,
                                        const float* attn, const float* v, int64_t v_sb, int64_t v_sh,
                                        int64_t v_sn, const float* Z, int64_t z_sb, int64_t z_sh, int64_t z_sn,
                                        float* cam_attn, float* cam_v, int64_t cv_sb, int64_t cv_sh,
                                        int64_t cv_sn, int64_t B, int64_t H, int64_t N, int64_t D,
                                        float out_scale, int variant, void* ws, size_t ws_bytes,
                                        te_stream_t stream_) {
  if (!R || !attn || !v || !cam_attn || !cam_v || B <= 0 || H <= 0 || N <= 0 || D <= 0)
    return TE_ERR_INVALID_ARG;
  const Strided rs{r_sb, r_sh, r_sn}, vs{v_sb, v_sh, v_sn}, cs{cv_sb, cv_sh, cv_sn}, contig{H * N * D, N * D, D};
  if (!view_ok(rs) || !view_ok(vs) || !view_ok(cs)) return TE_ERR_INVALID_ARG;
  if (!ws || ws_bytes < te_matmul_relprop_av_workspace_bytes(B, H, N, D)) return TE_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  float* S = (float*)ws;
  float* Zws = S + (size_t)(B * H) * N * D;
  Strided zs = Z ? Strided{z_sb, z_sh, z_sn} : contig;
  if ((variant & TE_IMPL_SIMPLE) || !te_attn_mfma::supported(N, D)) {      // asked for, or a head dim (a length) no MFMA kernel takes
    if (zs.sn != contig.sn || zs.sh != contig.sh || zs.sb != contig.sb) return TE_ERR_UNSUPPORTED;      // the simple kernels read Z as contiguous [B,H,N,D]
    const int64_t nd = B * H * N * D, nn = B * H * N * N;
    dim3 blk(kThreads);
    if (Z) av_s_from_z_simple<<<dim3((unsigned)te_ceil_div(nd, kThreads)), blk, 0, stream>>>(R, rs, Z, S, B, H, N, D);
    else av_s_simple<<<dim3((unsigned)te_ceil_div(nd, kThreads)), blk, 0, stream>>>(R, rs, attn, v, vs, S, B, H, N, D);
    av_cam_attn_simple<<<dim3((unsigned)te_ceil_div(nn, kThreads)), blk, 0, stream>>>(S, attn, v, vs, cam_attn, B,
                                                                                     H, N, D, out_scale);
    av_cam_v_simple<<<dim3((unsigned)te_ceil_div(nd, kThreads)), blk, 0, stream>>>(S, attn, v, vs, cam_v, cs, B, H,
                                                                                  N, D, out_scale);
    TE_RETURN_IF_LAUNCH_FAILED();
    return TE_OK;
  }
  if (!Z) {      // no cached forward product: every MFMA kernel takes Z as an input (te_attn_mfma.hip header)
    const int rc = te_attn_mfma::z_av_launch(attn, v, vs, Zws, B, H, N, stream);
    if (rc != TE_OK) return rc;
    Z = Zws;
  }
  // one pass over attn on wave-owned key blocks (round 5): every N <= 4096.  A row stride outside 64 ... 65536 floats ends the call
  // there: the tile kernels below are for the lengths beyond, not for the views it refuses.
  if (te_attn_kb::supported(B, H, N, D))
    return finish(te_attn_kb::av_launch(TE_ATTN_RULE, R, rs, attn, v, vs, Z, zs, cam_attn, cam_v, cs, B, H, N, out_scale, stream));
  // 64 x 64 tiles with S through the workspace (round 1): N <= 2^20, contiguous Z
  return finish(te_attn_mfma::av_launch(R, rs, attn, v, vs, Z, zs, cam_attn, cam_v, cs, B, H, N, out_scale, S, stream));
}

extern "C" size_t te_matmul_relprop_qk_workspace_bytes(int64_t B, int64_t H, int64_t N, int64_t D) {
  if (B <= 0 || H <= 0 || N <= 0 || D <= 0) return 0;
  return te_align_up((size_t)2 * B * H * N * N * sizeof(float), 256);
}

// r_scale (optional): the deferred per-sample factor of R_nn ; Z (optional): the cached forward product q k^T, contiguous
extern "C" int te_matmul_relprop_qk_f32(const float* R_nn, const float* r_scale, int64_t r_scale_stride,
                                        const float* q, int64_t q_sb, int64_t q_sh, int64_t q_sn,
                                        const float* k, int64_t k_sb, int64_t k_sh, int64_t k_sn,
                                        const float* Z, float* cam_q, int64_t cq_sb, int64_t cq_sh,
                                        int64_t cq_sn, float* cam_k, int64_t ck_sb, int64_t ck_sh,
                                        int64_t ck_sn, int64_t B, int64_t H, int64_t N, int64_t D,
                                        float out_scale, int variant, void* ws, size_t ws_bytes,
                                        te_stream_t stream_) {
  if (!R_nn || !q || !k || !cam_q || !cam_k || B <= 0 || H <= 0 || N <= 0 || D <= 0) return TE_ERR_INVALID_ARG;
  const Strided qs{q_sb, q_sh, q_sn}, ks{k_sb, k_sh, k_sn}, cqs{cq_sb, cq_sh, cq_sn}, cks{ck_sb, ck_sh, ck_sn};
  if (!view_ok(qs) || !view_ok(ks) || !view_ok(cqs) || !view_ok(cks)) return TE_ERR_INVALID_ARG;
  if (!ws || ws_bytes < te_matmul_relprop_qk_workspace_bytes(B, H, N, D)) return TE_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  float* S = (float*)ws;
  float* Zws = S + (size_t)(B * H) * N * N;
  if ((variant & TE_IMPL_SIMPLE) || !te_attn_mfma::supported(N, D)) {      // asked for, or a head dim (a length) no MFMA kernel takes
    if (r_scale) return TE_ERR_UNSUPPORTED;        // the simple kernels take a plain relevance operand
    const int64_t nd = B * H * N * D, nn = B * H * N * N;
    dim3 blk(kThreads);
    if (Z) qk_s_from_z_simple<<<dim3((unsigned)te_ceil_div(nn, kThreads)), blk, 0, stream>>>(R_nn, Z, S, nn);
    else qk_s_simple<<<dim3((unsigned)te_ceil_div(nn, kThreads)), blk, 0, stream>>>(R_nn, q, qs, k, ks, S, B, H, N, D);
    qk_cam_q_simple<<<dim3((unsigned)te_ceil_div(nd, kThreads)), blk, 0, stream>>>(S, q, qs, k, ks, cam_q, cqs, B, H,
                                                                                  N, D, out_scale);
    qk_cam_k_simple<<<dim3((unsigned)te_ceil_div(nd, kThreads)), blk, 0, stream>>>(S, q, qs, k, ks, cam_k, cks, B, H,
                                                                                  N, D, out_scale);
    TE_RETURN_IF_LAUNCH_FAILED();
    return TE_OK;
  }
  if (!Z) {      // no cached forward product (as for the AV rule)
    const int rc = te_attn_mfma::z_qk_launch(q, qs, k, ks, Zws, B, H, N, stream);
    if (rc != TE_OK) return rc;
    Z = Zws;
  }
  // 32-bit row offsets inside a (b, h) view of q in both one-pass kernels: such a view ends the call, at every N they serve
  if (te_attn_rules::supported(B, H, N, D) && q_sn > 65536) return TE_ERR_UNSUPPORTED;
  // row-block and key-block owners, S evaluated per owner and never shared (round 6): N <= 224
  if (te_attn_rc::supported(B, H, N, D))
    return finish(te_attn_rc::qk_launch(TE_ATTN_RULE, R_nn, q, qs, k, ks, Z, cam_q, cqs, cam_k, cks, B, H, N, out_scale, r_scale, r_scale_stride,
                                        stream));
  // one pass with k resident in LDS, groups of <= 256 keys (round 2): N <= 4096.  The per-group cam_q partials of N > 256 live
  // in the S region of the workspace, which no kernel of this path writes: ngroups * 64 <= N whenever ngroups > 1
  if (te_attn_rules::supported(B, H, N, D))
    return finish(te_attn_rules::qk_launch(TE_ATTN_RULE, R_nn, q, qs, k, ks, Z, cam_q, cqs, cam_k, cks, B, H, N, out_scale, /*qpart=*/S, r_scale,
                                           r_scale_stride, stream));
  // 64 x 64 tiles with S through the workspace (round 1): N <= 2^20
  if (r_scale) return TE_ERR_UNSUPPORTED;        // only the one-pass kernels take the deferred factor
  return finish(te_attn_mfma::qk_launch(R_nn, q, qs, k, ks, Z, cam_q, cqs, cam_k, cks, B, H, N, out_scale, S, stream));
}

// ================================================================================================
// The producers on the fused qkv activation [B,N,3C]: N <= 224, one workgroup per (b, h)
// ================================================================================================
extern "C" int te_attention_forward_supported(int64_t N, int64_t D) { return te_attn_fwd6::supported(1, 1, N, D) ? 1 : 0; }

// out_planes (optional; round 6): the operand planes of `out` for the projection layer's x6 kernels = the signed
// planes of out [B N, H D] (te_linear_x6_planes_bytes(B N, H D) bytes each), out_abs_planes (optional with them) = the planes of
// |out| -- bit for bit what te_linear_x6_split_dual_f32 writes from the fp32 tensor.
extern "C" int te_attention_forward_f32(const float* qkv, float* z_qk, float* attn, float* out, void* out_planes,
                                        void* out_abs_planes, size_t planes_bytes, int64_t B, int64_t H, int64_t N,
                                        int64_t D, float scale, te_stream_t stream_) {
  if (!qkv || !z_qk || !attn || !out || (out_abs_planes && !out_planes) || B <= 0 || H <= 0 || N <= 0) return TE_ERR_INVALID_ARG;
  if (!te_attn_fwd6::supported(B, H, N, D)) return TE_ERR_UNSUPPORTED;
  if (out_planes) {
    const size_t need = te_linear_x6_planes_bytes(B * N, H * D);
    if (need == 0) return TE_ERR_UNSUPPORTED;
    if (planes_bytes < need || !te_aligned16(out_planes) || (out_abs_planes && !te_aligned16(out_abs_planes))) return TE_ERR_WORKSPACE;
  }
  return finish(te_attn_fwd6::launch(qkv, z_qk, attn, out, B, H, N, scale, (hipStream_t)stream_, out_planes, out_abs_planes));
}

// `out` (optional): the block's forward output [B,N,C]; without it the row sums of the softmax backward come from the N x N tensors
extern "C" int te_attention_backward_f32(const float* d_out, const float* out, const float* qkv, const float* attn,
                                         float* d_attn, float* d_qkv, int64_t B, int64_t H, int64_t N, int64_t D,
                                         float scale, int need_qk, te_stream_t stream_) {
  if (!d_out || !qkv || !attn || !d_attn || !d_qkv || B <= 0 || H <= 0 || N <= 0) return TE_ERR_INVALID_ARG;
  if (!te_attn_fwd6::supported(B, H, N, D)) return TE_ERR_UNSUPPORTED;      // (the backward serves what the forward serves)
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t C = H * 64;
  const Strided heads{N * C, 64, C};            // [B,N,C] seen as [B,H,N,64]
  const Strided fused{N * 3 * C, 64, 3 * C};    // one of q / k / v inside [B,N,3C]
  const float *q = qkv, *k = qkv + C, *v = qkv + 2 * C;
  float *d_q = d_qkv, *d_k = d_qkv + C, *d_v = d_qkv + 2 * C;
  // d_attn = d_out v^T (the tensor save_attn_gradients receives, ViT_LRP.py:144-145) ; d_v = attn^T d_out: always on wave-owned key blocks
  const int rc = te_attn_kb::av_launch(TE_ATTN_BWD, d_out, heads, attn, v, fused, nullptr, Strided(), d_attn, d_v, fused, B, H, N, 1.0f, stream);
  if (rc != TE_OK || !need_qk) return finish(rc);
  // d_s = softmax backward * scale ; d_q = d_s k ; d_k = d_s^T q.  te_attn_rc.hip measured against qk_rule_kernel<BWD> on one box
  // (profiles/r06_attention_qk_rc_ab.log): it wins below ~160 tokens (69 vs 75 us at N = 128), ties at 224 and LOSES at 197 (the
  // headline: 272 vs 257 us for the whole backward pair -- its separate rowdot pass over the row panels), so it serves N <= 160.
  // With the forward output at hand its row dots sum_j attn d_attn = sum_d d_out out cost no pass over the N x N tensors, and it
  // serves every N <= 224.
  if ((N <= 160 || out) && te_attn_rc::supported(B, H, N, D))
    return finish(te_attn_rc::qk_launch(TE_ATTN_BWD, d_attn, q, fused, k, fused, attn, d_q, fused, d_k, fused, B, H, N, scale, nullptr, 0, stream,
                                        out ? d_out : nullptr, out, heads));
  // the one-pass kernel with every key of a row in its one group
  return finish(te_attn_rules::qk_launch(TE_ATTN_BWD, d_attn, q, fused, k, fused, attn, d_q, fused, d_k, fused, B, H, N, scale, nullptr, nullptr, 0,
                                         stream));
}

// ================================================================================================
// The producers on separate, strided q / k / v views: N <= 640 (ViT-L/16-384: 577; BERT: 512)
// ================================================================================================
extern "C" int te_attention_strided_supported(int64_t N, int64_t D) { return te_attn_long::supported(1, 1, N, D) ? 1 : 0; }

// rowdot [B*H,N]: what the row side of the backward leaves for the column side
extern "C" size_t te_attention_backward_strided_workspace_bytes(int64_t B, int64_t H, int64_t N) {
  return te_align_up((size_t)(B * H * N) * sizeof(float), 256);
}

extern "C" int te_attention_forward_strided_f32(const float* q, int64_t q_sb, int64_t q_sh, int64_t q_sn, const float* k,
                                                int64_t k_sb, int64_t k_sh, int64_t k_sn, const float* v, int64_t v_sb,
                                                int64_t v_sh, int64_t v_sn, const float* mask, float* z_qk,
                                                float* x_scaled, float* attn, float* out, int64_t o_sb, int64_t o_sh,
                                                int64_t o_sn, int64_t B, int64_t H, int64_t N, int64_t D, float scale,
                                                te_stream_t stream_) {
  using te_attn_long::strides_ok;
  if (!q || !k || !v || !attn || !out || B <= 0 || H <= 0 || N <= 0) return TE_ERR_INVALID_ARG;
  const Strided qs{q_sb, q_sh, q_sn}, ks{k_sb, k_sh, k_sn}, vs{v_sb, v_sh, v_sn}, os{o_sb, o_sh, o_sn};
  if (!te_attn_long::supported(B, H, N, D)) return TE_ERR_UNSUPPORTED;
  if (!strides_ok(qs) || !strides_ok(ks) || !strides_ok(vs) || !strides_ok(os)) return TE_ERR_UNSUPPORTED;
  hipStream_t stream = (hipStream_t)stream_;
  // row-block owners on bf16 MFMAs (round 6), 1.4-2.2 x the row tiles: 64 < N, B H <= 2^24
  if (te_attn_fwd6l::supported(B, H, N, D))
    return finish(te_attn_fwd6l::launch(q, qs, k, ks, v, vs, mask, z_qk, x_scaled, attn, out, os, B, H, N, scale, stream));
  // row tiles on fp32 MFMAs (round 3): the rest, N <= 64 above all
  return finish(te_attn_long::fwd_launch(q, qs, k, ks, v, vs, mask, z_qk, x_scaled, attn, out, os, B, H, N, scale, stream));
}

// out (optional): the forward output attention_forward returned for these inputs ([B,H,N,64] view)
extern "C" int te_attention_backward_strided_f32(const float* d_out, int64_t do_sb, int64_t do_sh, int64_t do_sn,
                                                 const float* out, int64_t o_sb, int64_t o_sh, int64_t o_sn, const float* q,
                                                 int64_t q_sb, int64_t q_sh, int64_t q_sn, const float* k, int64_t k_sb,
                                                 int64_t k_sh, int64_t k_sn, const float* v, int64_t v_sb, int64_t v_sh,
                                                 int64_t v_sn, const float* attn, float* d_attn, float* d_q, int64_t dq_sb,
                                                 int64_t dq_sh, int64_t dq_sn, float* d_k, int64_t dk_sb, int64_t dk_sh,
                                                 int64_t dk_sn, float* d_v, int64_t dv_sb, int64_t dv_sh, int64_t dv_sn,
                                                 int64_t B, int64_t H, int64_t N, int64_t D, float scale, int need_qk, void* ws,
                                                 size_t ws_bytes, te_stream_t stream_) {
  using te_attn_long::strides_ok;
  const Strided dos{do_sb, do_sh, do_sn}, qs{q_sb, q_sh, q_sn}, ks{k_sb, k_sh, k_sn}, vs{v_sb, v_sh, v_sn};
  const Strided dqs{dq_sb, dq_sh, dq_sn}, dks{dk_sb, dk_sh, dk_sn}, dvs{dv_sb, dv_sh, dv_sn};
  const Strided os = out ? Strided{o_sb, o_sh, o_sn} : Strided();
  if (!d_out || !k || !v || !attn || !d_attn || !d_v || B <= 0 || H <= 0 || N <= 0) return TE_ERR_INVALID_ARG;
  if (need_qk && (!q || !d_q || !d_k)) return TE_ERR_INVALID_ARG;
  if (!te_attn_long::supported(B, H, N, D)) return TE_ERR_UNSUPPORTED;
  if (!strides_ok(dos) || !strides_ok(ks) || !strides_ok(vs) || !strides_ok(dvs) || (out && !strides_ok(os))) return TE_ERR_UNSUPPORTED;
  if (need_qk && (!strides_ok(qs) || !strides_ok(dqs) || !strides_ok(dks))) return TE_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < te_attention_backward_strided_workspace_bytes(B, H, N)) return TE_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  float* rowdot = (float*)ws;
  need_qk = need_qk ? 1 : 0;
  const bool l6 = te_attn_bwd6l::supported(B, H, N, D);      // row-block / key-block owners on bf16 MFMAs (round 6): 64 < N, B H <= 2^24
  // The row side: d_attn = d_out v^T, the row sums, d_q.  The round-6 kernel takes its row sums from d_out . out, so it serves a
  // caller with the forward output at hand, or one that needs no row sum (need_qk = 0); the row tiles of round 3 form them from
  // d_attn . attn
  int rc;
  if ((out || !need_qk) && l6)
    rc = te_attn_bwd6l::launch_rows(d_out, dos, out, os, k, ks, v, vs, attn, d_attn, rowdot, d_q, dqs, B, H, N, scale, need_qk, stream);
  else
    rc = te_attn_long::bwd_rows_launch(d_out, dos, k, ks, v, vs, attn, d_attn, rowdot, d_q, dqs, B, H, N, scale, need_qk, stream);
  if (rc != TE_OK) return rc;
  // The column side: d_v = attn^T d_out, d_k = d_s^T q from attn, d_attn and rowdot, whichever kernel left them
  if (l6) return finish(te_attn_bwd6l::launch_cols(attn, d_attn, rowdot, d_out, dos, q, qs, d_v, dvs, d_k, dks, B, H, N, scale, need_qk, stream));
  return finish(te_attn_long::bwd_cols_launch(attn, d_attn, rowdot, d_out, dos, q, qs, d_v, dvs, d_k, dks, B, H, N, scale, need_qk, stream));
}
