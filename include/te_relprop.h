/*
 * te_relprop.h -- C ABI of libte_relprop.so: the MI355X (gfx950) relevance-propagation hot path of
 * hila-chefer/Transformer-Explainability ("transformer_attribution": LRP relprop rules ->
 * gradient x attention head-mean -> rollout).
 *
 * Drop-in boundary.  The reference is pure Python; every entry point below replaces the body of one
 * `relprop` method (or one tail function) that the reference expresses as torch.autograd.grad on a
 * re-built micro-graph.  The reference-side binding is a ctypes stub; the
 * shipped host side is transformer-explainability_amd/ (same class / method names as the reference).
 *
 * Conventions
 *   - all tensors are fp32, row-major, device (HBM) pointers; shapes are int64 element counts,
 *     strides are in ELEMENTS; the innermost dimension is always contiguous.
 *   - BATCH SEMANTICS: the reference is batch-1 only (ViT_explanation_generator.py:31-32); a batch
 *     of B samples here means B independent batch-1 problems -- every "whole tensor" reduction of
 *     the reference (Add.relprop sums, modules/layers_ours.py:109-116) is taken per sample.
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); no call synchronises,
 *     allocates, frees, or keeps a pointer after it returns; the library has no global state.
 *   - scratch memory is caller-provided: query te_<op>_workspace_bytes(...) and pass a device
 *     buffer of at least that size (16-byte aligned).  Ops without a query need none.
 *   - return value: 0 = TE_OK; negative = TE_ERR_* below; positive = a hipError_t from the launch.
 *   - `variant`: low byte TE_VARIANT_OURS (modules/layers_ours.py) or TE_VARIANT_LRP
 *     (modules/layers_lrp.py); OR-in TE_IMPL_SIMPLE to force the simple (non-MFMA) device kernels,
 *     which tests use as an on-device cross-check of the tiled kernels.
 *   - safe_divide(a,b) = a / (b + 1e-9 [==0 -> 1e-9]) * (b != 0)     modules/layers_ours.py:10-13
 */
#ifndef TE_RELPROP_H
#define TE_RELPROP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* te_stream_t; /* hipStream_t */
typedef uint16_t te_bf16_t; /* one bf16 value (the upper half of an fp32) */

enum {
  TE_OK = 0,
  TE_ERR_INVALID_ARG = -1, /* null pointer, non-positive size, bad variant */
  TE_ERR_WORKSPACE = -2,   /* ws == NULL or ws_bytes too small */
  TE_ERR_UNSUPPORTED = -3, /* shape outside what the kernels implement */
  TE_ERR_NO_DEVICE = -4    /* no gfx950 device visible */
};

enum { TE_VARIANT_OURS = 0, TE_VARIANT_LRP = 1, TE_IMPL_SIMPLE = 0x100 };

enum { TE_ROLLOUT_NORMALISE = 1, TE_ROLLOUT_CLS_FIXUP = 2, TE_ROLLOUT_ROW0 = 4 };

/* library version (major*10000 + minor*100 + patch) and status strings */
int te_version(void);
const char* te_status_string(int status);
/* 0 if device 0..n-1 contains a gfx950 agent usable by this library, TE_ERR_NO_DEVICE otherwise */
int te_device_check(void);
/* Provenance of this binary: "<16 hex>-<8 hex>" = sha256 over csrc/{*.hip,*.h} + include/{*.h} (names and contents,
 * sorted) and over the compiler flags, baked in by build.py.  The Python loader recomputes the first half from the tree it
 * was imported from and refuses a library built from other sources; bench.py and smoke() print it. */
const char* te_build_id(void);

/* ---- a3  Linear.relprop -------------------------------------------------------------------
 * replaces modules/layers_ours.py:207-230 (ours) and modules/layers_lrp.py:188-211 (lrp), and the
 * BERT copies BERT_explainability/modules/layers_ours.py:219-242.
 *   R [T,out_f], X [T,in_f], W [out_f,in_f] -> out [T,in_f]          (T = B*N rows, bias unused)
 *   ours: Z = X+ W+^T + X- W-^T ; S = sd(R,Z) ; act = X+ .(S W+) + X- .(S W-)
 *   lrp : S1 = sd(R, X+ W+^T) ; S2 = sd(R, X- W-^T) ; act = X+ .(S1 W+) + X- .(S2 W-)
 *   out = alpha*act - (alpha-1)*inh, inh = the same with W+ and W- exchanged (skipped at alpha==1).
 */
size_t te_linear_relprop_workspace_bytes(int64_t T, int64_t in_f, int64_t out_f, int variant);
int te_linear_relprop_f32(const float* R, const float* X, const float* W, float* out,
                          int64_t T, int64_t in_f, int64_t out_f, float alpha, int variant,
                          void* ws, size_t ws_bytes, te_stream_t stream);

/* The two kernels of te_linear_relprop_f32 (variant ours, alpha = 1, in_f and out_f multiples of 4,
 * 16-byte aligned pointers) as separate launches:
 *   zpass: S [T,out_f] = sd(R, X+ W+^T + X- W-^T)      (layers_ours.py:216-219)
 *   cpass: out [T,in_f] = X+ .(S W+) + X- .(S W-)       (layers_ours.py:220-223,225)
 * Callers that want to time or overlap a single kernel launch use these; results are identical to
 * the composed call. */
int te_linear_zpass_f32(const float* R, const float* X, const float* W, float* S,
                        int64_t T, int64_t in_f, int64_t out_f, te_stream_t stream);
int te_linear_cpass_f32(const float* S, const float* X, const float* W, float* out,
                        int64_t T, int64_t in_f, int64_t out_f, te_stream_t stream);

/* Linear.relprop (variant ours, alpha = 1) using the FORWARD OUTPUT the rule module already caches
 * (forward_hook: `self.Y = output`, modules/layers_ours.py:16-27):  Y [T,out_f] = X W^T + bias  (bias may be
 * NULL).  Same-sign products sum to Z = X+ W+^T + X- W-^T and opposite-sign ones to X W^T - Z, while |X| |W|^T is
 * their difference, so   Z = ((Y - bias) + |X| |W|^T) / 2   needs ONE product instead of two (25 % fewer FLOPs per
 * Linear.relprop).  Elements where the halves cancel (Z < 2^-7 |X||W|^T) are recomputed as the plain positive-part
 * sum, so zero rows and near-zero Z behave as in layers_ours.py:216-219.  in_f, out_f multiples of 4 and 16-byte
 * aligned pointers (else TE_ERR_UNSUPPORTED: use te_linear_relprop_f32).  Workspace: te_linear_relprop_workspace_bytes
 * (T, in_f, out_f, TE_VARIANT_OURS).
 *   zpass_fwd: S [T,out_f] = sd(R, Z)          relprop_fwd: zpass_fwd, then te_linear_cpass_f32
 * r_scale (optional, NULL = plain R): a DEFERRED per-sample factor on the relevance operand.  Row t of R enters the rule as
 * R[t,:] * r_scale[(t / rows_per_sample) * r_scale_stride] (the fp32 product Add.relprop's rescale would have stored,
 * layers_ours.py:117-118) -- the consumer side of te_add_relprop_deferred_f32.  Without it r_scale_stride and
 * rows_per_sample are ignored. */
int te_linear_zpass_fwd_f32(const float* R, const float* r_scale, int64_t r_scale_stride,
                            int64_t rows_per_sample, const float* X, const float* W, const float* Y,
                            const float* bias, float* S, int64_t T, int64_t in_f, int64_t out_f,
                            te_stream_t stream);
int te_linear_relprop_fwd_f32(const float* R, const float* r_scale, int64_t r_scale_stride,
                              int64_t rows_per_sample, const float* X, const float* W, const float* Y,
                              const float* bias, float* out, int64_t T, int64_t in_f, int64_t out_f,
                              void* ws, size_t ws_bytes, te_stream_t stream);

/* ---- a4  einsum / MatMul relprop (RelPropSimple) ---------------------------------------------
 * replaces modules/layers_ours.py:48-60,122-127 and BERT_explainability/modules/layers_ours.py:89-91
 * for the two products of self-attention.  Element (b,h,n,d) of a strided operand T lives at
 * T + b*sb + h*sh + n*sn + d, so q/k/v can be read in place from the fused qkv activation
 * [B,N,3*H*D] (ViT_LRP.py:135) or from separate [B,N,H*D] tensors (BERT.py:330-336), and the
 * outputs can be written straight into the concatenated 'b n (qkv h d)' layout (ViT_LRP.py:175).
 * attn / cam_attn / R_nn are contiguous [B,H,N,N].  Both outputs are multiplied by out_scale
 * (callers pass 0.5: ViT_LRP.py:161-162,172-173; BERT.py:373-374,392-393).
 *
 * AV  (einsum 'bhij,bhjd->bhid'; BERT MatMul([probs, V])):
 *   Z = attn v ; S = sd(R,Z) ; cam_attn = attn .(S v^T) ; cam_v = v .(attn^T S)
 * QK  (einsum 'bhid,bhjd->bhij'; BERT MatMul([Q, K^T])), Z uses the UNSCALED q k^T:
 *   Z = q k^T ; S = sd(R_nn,Z) ; cam_q = q .(S k) ; cam_k = k .(S^T q)
 *
 * Optional operands (NULL = absent; the strides of an absent operand are ignored):
 *   Z        the FORWARD output of the product whose rule is evaluated (einsum / MatMul modules cache it as self.Y,
 *            forward_hook layers_ours.py:16-27).  The reference's autograd re-evaluates that product and gets the same
 *            bits, so the rule needs two products instead of three and S matches the forward pass exactly.  Absent: the
 *            product is formed in the workspace.
 *            AV: element (b,h,n,d) at Z + b*z_sb + h*z_sh + n*z_sn + d.  The product attn v usually lives only as the
 *            'b n (h d)' activation that feeds the output projection (ViT_LRP.py:148): z_sb = N*C, z_sh = D, z_sn = C
 *            reads it in place; a contiguous [B,H,N,D] copy has z_sb = H*N*D, z_sh = N*D, z_sn = D.  Only the one-pass
 *            kernels (head dim 64) take other strides than the contiguous ones: TE_ERR_UNSUPPORTED otherwise.
 *            QK: contiguous [B,H,N,N].
 *   r_scale  (QK) a DEFERRED per-sample factor on the relevance operand: sample b's R_nn enters as
 *            R_nn[b] * r_scale[b * r_scale_stride] -- the consumer side of te_add_bcast_relprop_deferred_f32
 *            (BERT.py:386-393).  One-pass kernels only (head dim 64): TE_ERR_UNSUPPORTED otherwise.
 */
size_t te_matmul_relprop_av_workspace_bytes(int64_t B, int64_t H, int64_t N, int64_t D);
int te_matmul_relprop_av_f32(const float* R, int64_t r_sb, int64_t r_sh, int64_t r_sn,
                             const float* attn,
                             const float* v, int64_t v_sb, int64_t v_sh, int64_t v_sn,
                             const float* Z, int64_t z_sb, int64_t z_sh, int64_t z_sn,
                             float* cam_attn,
                             float* cam_v, int64_t cv_sb, int64_t cv_sh, int64_t cv_sn,
                             int64_t B, int64_t H, int64_t N, int64_t D, float out_scale, int variant,
                             void* ws, size_t ws_bytes, te_stream_t stream);
size_t te_matmul_relprop_qk_workspace_bytes(int64_t B, int64_t H, int64_t N, int64_t D);
int te_matmul_relprop_qk_f32(const float* R_nn, const float* r_scale, int64_t r_scale_stride,
                             const float* q, int64_t q_sb, int64_t q_sh, int64_t q_sn,
                             const float* k, int64_t k_sb, int64_t k_sh, int64_t k_sn,
                             const float* Z,
                             float* cam_q, int64_t cq_sb, int64_t cq_sh, int64_t cq_sn,
                             float* cam_k, int64_t ck_sb, int64_t ck_sh, int64_t ck_sn,
                             int64_t B, int64_t H, int64_t N, int64_t D, float out_scale, int variant,
                             void* ws, size_t ws_bytes, te_stream_t stream);

/* ---- a5  Add.relprop ---------------------------------------------------------------------------
 * replaces modules/layers_ours.py:97-120 (ours: three per-sample sums + rescale) and
 * modules/layers_lrp.py:98-100 (lrp: plain RelPropSimple).  R, X0, out0, out1 are [B,n]; X1 is [B,n]
 * (x1_batch_stride = n) or shared by all samples (x1_batch_stride = 0, e.g. pos_embed).
 *   S = sd(R, X0+X1) ; a = X0.S ; b = X1.S ;
 *   ours: a *= sd(sd(|Sa|,|Sa|+|Sb|)*SR, Sa) ; b *= sd(sd(|Sb|,|Sa|+|Sb|)*SR, Sb)   (per sample)
 */
size_t te_add_relprop_workspace_bytes(int64_t B, int64_t n);
int te_add_relprop_f32(const float* R, const float* X0, const float* X1, float* out0, float* out1,
                       int64_t B, int64_t n, int64_t x1_batch_stride, int variant,
                       void* ws, size_t ws_bytes, te_stream_t stream);

/* Add.relprop, variant ours, with the per-sample rescale DEFERRED to the consumers: ONE streaming pass (the rule's
 * algorithmic 5 n floats per sample) writes a = X0.S and b = X1.S unscaled and fac [B,2] = {fa, fb} per sample, where
 * te_add_relprop_f32 would have stored out0 = a*fa, out1 = b*fb (layers_ours.py:117-118).  The consumers take the
 * factor with the operand and form the identical product in registers: te_clone_relprop_scaled_f32,
 * te_linear_relprop_fwd_f32.  Workspace: te_add_relprop_deferred_workspace_bytes. */
size_t te_add_relprop_deferred_workspace_bytes(int64_t B, int64_t n);
int te_add_relprop_deferred_f32(const float* R, const float* X0, const float* X1, float* a, float* b, float* fac,
                                int64_t B, int64_t n, int64_t x1_batch_stride,
                                void* ws, size_t ws_bytes, te_stream_t stream);

/* Broadcast-operand Add of BERT self-attention (BERT.py:342,386-388): X0 = scaled scores
 * [B,H,N,N], X1 = extended mask [B,1,1,N] given as mask [B,N].  out0 [B,H,N,N] (relevance of the
 * scores); out1 [B,N] (relevance of the mask, discarded by the reference) may be NULL.
 *   S = sd(R, X0 + mask_j) ; a = X0.S ; C1_j = sum_{h,i} S ; b_j = mask_j C1_j ; rescale as above.
 */
size_t te_add_bcast_relprop_workspace_bytes(int64_t B, int64_t H, int64_t N);
int te_add_bcast_relprop_f32(const float* R, const float* X0, const float* mask, float* out0,
                             float* out1, int64_t B, int64_t H, int64_t N, int variant,
                             void* ws, size_t ws_bytes, te_stream_t stream);

/* The same rule (variant ours) with the rescale deferred: ONE pass over R and X0 writes a = X0.S unscaled and
 * fac [B,2] = {fa, fb}; out1 [B,N] (optional) is written scaled.  a * fa is bitwise te_add_bcast_relprop_f32's out0;
 * the consumer is te_matmul_relprop_qk_f32.  Workspace: te_add_bcast_relprop_workspace_bytes. */
int te_add_bcast_relprop_deferred_f32(const float* R, const float* X0, const float* mask, float* a, float* out1,
                                      float* fac, int64_t B, int64_t H, int64_t N,
                                      void* ws, size_t ws_bytes, te_stream_t stream);

/* ---- a6  Clone.relprop --------------------------------------------------------------------------
 * replaces modules/layers_ours.py:151-169.  out = X .(sd(R0,X) + sd(R1,X) [+ sd(R2,X)]); R2 may be
 * NULL (num = 2: ViT_LRP.py:194-196, BERT.py:247,527) or not (num = 3: BERT.py:407). n elements. */
int te_clone_relprop_f32(const float* R0, const float* R1, const float* R2, const float* X,
                         float* out, int64_t n, te_stream_t stream);

/* Clone.relprop on [B,n] operands whose relevance inputs carry deferred per-sample factors: R_i enters as
 * R_i[b,:] * s_i[b * s_i_stride]; s_i == NULL means no factor (R2 == NULL: two aliases). */
int te_clone_relprop_scaled_f32(const float* R0, const float* s0, int64_t s0_stride,
                                const float* R1, const float* s1, int64_t s1_stride,
                                const float* R2, const float* s2, int64_t s2_stride,
                                const float* X, float* out, int64_t B, int64_t n, te_stream_t stream);

/* ---- a7  IndexSelect.relprop ----------------------------------------------------------------------
 * replaces modules/layers_ours.py:129-147 for dim=1, one index (ViT_LRP.py:319,329; BERT.py:170,189).
 * R [B,C], X [B,N,C] -> out [B,N,C]: row `index` = X_row . sd(R, X_row), all other rows zero. */
int te_index_select_relprop_f32(const float* R, const float* X, float* out,
                                int64_t B, int64_t N, int64_t C, int64_t index, te_stream_t stream);

/* ---- a10  gradient x relevance, clamp, head mean ------------------------------------------------
 * replaces ViT_LRP.py:359-366 and ExplanationGenerator.py:49-56 (per sample):
 * grad, cam [B,H,N,N] -> out [B,N,N] = (sum_h max(grad*cam, 0)) / H. */
int te_gradcam_headmean_f32(const float* grad, const float* cam, float* out,
                            int64_t B, int64_t H, int64_t N, te_stream_t stream);

/* ---- a11  rollout ---------------------------------------------------------------------------------
 * replaces compute_rollout_attention, ViT_LRP.py:38-49 (flags = 0) and ExplanationGenerator.py:7-18
 * (TE_ROLLOUT_NORMALISE), plus the CLS fix-up ExplanationGenerator.py:58 (TE_ROLLOUT_CLS_FIXUP:
 * joint[b,0,0] = min_j joint[b,0,j]).  cams [L,B,N,N] -> joint [B,N,N]:
 *   M_l = cams_l + I (/ rowsum) ; J = M_start ; J = M_i J for i = start+1 .. L-1.
 * The (N x N)(N x N) products run on fp32 MFMA tiles; OR TE_IMPL_SIMPLE into `flags` for the plain fmaf kernel.
 * TE_ROLLOUT_ROW0: only row 0 of the joint matrix is produced -- what both generators consume (ViT_LRP.py:369
 * `rollout[:, 0, 1:]`, ExplanationGenerator.py:58-59 `rollout[:, 0]`) -- as the vector chain r = e_0^T M_{L-1},
 * r = r M_i (i = L-2 .. start): every layer matrix is read once (HBM-bound) instead of L-1-start N^3 products.
 * `joint` is then [B,N]; the workspace query is te_rollout_row0_workspace_bytes; N <= 1024. */
size_t te_rollout_workspace_bytes(int64_t L, int64_t B, int64_t N);
size_t te_rollout_row0_workspace_bytes(int64_t B, int64_t N);
int te_rollout_f32(const float* cams, int64_t L, int64_t start_layer, int64_t B, int64_t N,
                   int flags, float* joint, void* ws, size_t ws_bytes, te_stream_t stream);

/* te_linear_relprop_fwd_f32 (same rule: modules/layers_ours.py:207-230, variant ours, alpha = 1, Z from the
 * forward output, optional per-sample factor on R) with its three products on bf16 MFMAs at fp32 accuracy: every fp32
 * operand is used as the exact sum of three bf16 parts and the six partial products above 2^-24 are accumulated in fp32
 * (csrc/te_linear_x6.hip).  in_f, out_f >= 128, out_f % 128 == 0, in_f % 64 == 0.
 *
 * Operand planes ("P3"): an fp32 [rows, K] operand as bf16 planes in MFMA-fragment order
 * [ceil(rows / 32)][K / 16][3 planes][k-half 2][row 32][8 bf16]; te_linear_x6_planes_bytes gives the size.
 *   te_linear_x6_prepare_weights_f32   W [out_f, in_f] -> the weight-side planes of both passes (|W| as P3, then
 *                                      max(W,0)^T / min(W,0)^T interleaved per 32-row block); a caller evaluates this
 *                                      ONCE per weight version and passes the result as w_planes
 *   te_linear_x6_split_abs_f32         X [rows, K] -> P3 planes of |X| (what a producer of X may emit itself)
 *   te_linear_relprop_x6_f32           x_planes = NULL: |X| is split into the workspace first.
 * Workspace = |X| planes, S planes (the Z-pass writes S only in plane form), 64 MiB of accumulator hand-over between
 * workgroups that share a tile (sequential stream-K: one k-ordered chain per output wherever a tile is cut), flags.
 * flags: TE_X6_TILE_AUTO (per pass: 256 weight rows per tile / one 512-thread workgroup per CU where that gives every CU
 * a tile, else 128 rows / two 256-thread workgroups per CU; the result does not depend on the tile geometry, bit for
 * bit), TE_X6_TILE_128 / TE_X6_TILE_256 pin it; shifted left by TE_X6_TILE_Z_SHIFT / TE_X6_TILE_C_SHIFT they pin one pass.
 * TE_X6_TILE_128x128: 128 x 128 tiles, three 256-thread workgroups per CU (launches with few weight rows).
 * Unknown flag bits: TE_ERR_INVALID_ARG.
 *
 * Failure is loud.  A workgroup that continues a tile another workgroup started waits for that one's accumulators for at
 * most 250 ms.  If the wait expires it ORs 1 into *status -- a caller-owned, caller-zeroed device word that is NEVER
 * cleared by the library (sticky across calls: read it once where the caller synchronises anyway) -- sets the error word
 * te_linear_relprop_x6_check reads, and continues from NaN accumulators: every output of that tile is NaN (te_gemm_x6_f32,
 * C-pass) or recomputed by the rule's exact fallback (Z-pass).  Once *status is non-zero, later waits give up at once.
 * status = NULL: the per-call error word only.  TE_X6_TEST_DROP_HANDOVER (tests): publishers keep their flags down, so
 * every such wait expires; TE_X6_TEST_SMALL_GRID (tests): sixteen workgroups, i.e. cut tiles on small shapes.
 * te_linear_relprop_x6_check (synchronises) returns 1 if a bounded hand-over wait of the last call expired. */
#define TE_X6_TILE_AUTO 0
#define TE_X6_TILE_128 1
#define TE_X6_TILE_256 2
#define TE_X6_TILE_128x128 3
#define TE_X6_TEST_DROP_HANDOVER 0x200
#define TE_X6_WHOLE_TILES 0x10000       /* ranges cut at tile boundaries only, whatever the fill of the last round: for callers that
                                          keep several streams busy (the idle CUs of a last round are used by their other kernels,
                                          and no tile is handed over between workgroups).  Same results, bit for bit */
#define TE_X6_TEST_SMALL_GRID 0x4000   /* tests: a persistent grid of 16 workgroups, so that small shapes get stream-K cuts
                                          (with TE_X6_WHOLE_TILES: several whole tiles per workgroup) */
/* The schedule of a launch (same results, bit for bit, whichever is taken).  Default: whole tiles where their wall time is
 * within a margin of stream-K's by the measured K16 step times of the two schedules (csrc/te_linear_x6.hip, plan_x6), and the
 * whole tiles of an XCD are claimed by its workgroups from a counter in the workspace, one at a time.  The margin is the
 * launch-to-launch spread (5 %); a call pinned to TE_X6_TILE_256 -- the pin of a caller that keeps several streams busy, where
 * CU-time counts and not the length of one launch -- trades up to 20 % of a launch's wall time for the lower CU-time of whole
 * tiles.  For A/B runs and tests: */
#define TE_X6_SLACK_RULE 0x100000       /* decide as before the cost rule: whole tiles only if the last round is at least 1/1.15 full */
#define TE_X6_STATIC_TILES 0x80000      /* whole-tile launches cut the XCD's tiles into one static range per workgroup: no counter */
#define TE_X6_X_PLANES_SIGNED 0x20000   /* te_linear_relprop_x6_f32: x_planes holds the SIGNED planes of X (te_gemm_x6_f32's x_planes, what
                                          the layer's forward product read) instead of the planes of |X|: the Z-pass clears the sign of
                                          plane 0 and flips the low planes as it stages them.  Same results, bit for bit; with
                                          x_planes = NULL the split into the workspace writes signed planes */
#define TE_X6_TILE_Z_SHIFT 10
#define TE_X6_TILE_C_SHIFT 12
/* optional phase mask (measurement: one phase per call on the same workspace, in this order); 0 = the whole rule */
#define TE_X6_PHASE_SPLIT 4    /* clear the flags, |X| -> planes (unless x_planes is given) */
#define TE_X6_PHASE_Z 8        /* S planes */
#define TE_X6_PHASE_C 16       /* out */
#define TE_X6_PHASE_MASK 28
int te_linear_relprop_x6_supported(int64_t T, int64_t in_f, int64_t out_f);
size_t te_linear_relprop_x6_workspace_bytes(int64_t T, int64_t in_f, int64_t out_f);
size_t te_linear_x6_weight_planes_bytes(int64_t in_f, int64_t out_f);
size_t te_linear_x6_planes_bytes(int64_t rows, int64_t K);
int te_linear_x6_prepare_weights_f32(const float* W, int64_t in_f, int64_t out_f, void* planes, size_t planes_bytes,
                                     te_stream_t stream);
int te_linear_x6_split_abs_f32(const float* X, int64_t rows, int64_t K, void* planes, size_t planes_bytes,
                               te_stream_t stream);
int te_linear_relprop_x6_f32(const float* R, const float* r_scale, int64_t r_scale_stride, int64_t rows_per_sample,
                             const float* X, const float* W, const void* w_planes, const void* x_planes,
                             const float* Y, const float* bias, float* out,
                             int64_t T, int64_t in_f, int64_t out_f, int flags, unsigned* status, void* ws,
                             size_t ws_bytes, te_stream_t stream);
int te_linear_relprop_x6_check(const void* ws, int64_t T, int64_t in_f, int64_t out_f, te_stream_t stream);
/* What a launch would do, without a device: pass = TE_X6_PASS_Z / TE_X6_PASS_C of te_linear_relprop_x6_f32 on [T, in_f] ->
 * [T, out_f], or TE_X6_PASS_PRODUCT = te_gemm_x6_f32 with K = in_f, M = out_f; flags as that call takes them.  schedule[0 .. 3] =
 * the tile geometry (TE_X6_TILE_128 / _256 / _128x128), the schedule (TE_X6_SCHEDULE_*), the grid in workgroups, the tiles. */
#define TE_X6_PASS_Z 0
#define TE_X6_PASS_C 1
#define TE_X6_PASS_PRODUCT 2
#define TE_X6_SCHEDULE_STREAM_K 0
#define TE_X6_SCHEDULE_WHOLE_STATIC 1
#define TE_X6_SCHEDULE_WHOLE_CLAIMED 2
int te_linear_x6_schedule(int64_t T, int64_t in_f, int64_t out_f, int pass, int flags, int* schedule);

/* The same rule for EVERY variant and alpha on the x6 kernels (csrc/te_linear_x6.hip): variant TE_VARIANT_LRP =
 * modules/layers_lrp.py:188-211 (S1 = sd(R, X+ W+^T), S2 = sd(R, X- W-^T), separate denominators), and the inhibitor half
 * alpha * f(pw, nw, px, nx) - beta * f(nw, pw, px, nx), beta = alpha - 1, of both variants (layers_ours.py:225-228).
 *   variant ours: w_planes as above, Y (the forward output) required; x_abs_planes optional (the |X| planes).
 *   variant lrp : w_planes_lrp from te_linear_x6_prepare_weights_lrp_f32 (P3 planes of max(W,0), min(W,0) and of their
 *                 transposes); in_f % 128 == 0; Y, bias, w_planes unused (may be NULL).
 * flags: TE_X6_TILE_* | test hooks; status as te_linear_relprop_x6_f32. */
int te_linear_relprop_x6_general_supported(int64_t T, int64_t in_f, int64_t out_f, int variant);
size_t te_linear_x6_weight_planes_lrp_bytes(int64_t in_f, int64_t out_f);
int te_linear_x6_prepare_weights_lrp_f32(const float* W, int64_t in_f, int64_t out_f, void* planes, size_t planes_bytes,
                                         te_stream_t stream);
size_t te_linear_relprop_x6_general_workspace_bytes(int64_t T, int64_t in_f, int64_t out_f, int variant);
int te_linear_relprop_x6_general_f32(const float* R, const float* r_scale, int64_t r_scale_stride, int64_t rows_per_sample,
                                     const float* X, const float* W, const void* w_planes, const void* w_planes_lrp,
                                     const void* x_abs_planes, const float* Y, const float* bias, float* out,
                                     int64_t T, int64_t in_f, int64_t out_f, float alpha, int variant, int flags,
                                     unsigned* status, void* ws, size_t ws_bytes, te_stream_t stream);

/* The plain fp32 product on the same kernels (the forward output and the input gradient of a Linear layer,
 * modules/layers_ours.py:207 = nn.Linear): out [T, M] = X [T, K] . W^T + bias [M] with W given as signed P3 planes of an
 * [M, K] matrix.  te_linear_x6_split_matrix_f32 builds such planes from a row-major [rows, K] matrix (transposed = 0) or
 * from its transpose stored as [K, rows] (transposed = 1: the planes of W^T for d_x = d_y W).  M % 128 == 0, K % 16 == 0.
 * x_planes = NULL: X is split into the workspace first.  flags: TE_X6_TILE_* | TE_X6_TEST_DROP_HANDOVER | TE_X6_TEST_SMALL_GRID;
 * status: as te_linear_relprop_x6_f32. */
int te_gemm_x6_supported(int64_t T, int64_t K, int64_t M);
size_t te_gemm_x6_workspace_bytes(int64_t T, int64_t K, int64_t M);
int te_linear_x6_split_matrix_f32(const float* A, int64_t rows, int64_t K, int transposed, void* planes,
                                  size_t planes_bytes, te_stream_t stream);
int te_gemm_x6_f32(const float* X, const void* x_planes, const void* w_planes, const float* bias, float* out,
                   int64_t T, int64_t K, int64_t M, int flags, unsigned* status, void* ws, size_t ws_bytes,
                   te_stream_t stream);
/* One pass over a row-major A [rows, K]: its signed planes (the x_planes of te_gemm_x6_f32) AND the planes of |A| (the
 * x_planes of te_linear_relprop_x6_f32 for the same layer input: layers_ours.py:215 clamps / pairs X by sign, the rule's Z
 * is |X| |W|^T).  Both buffers te_linear_x6_planes_bytes(rows, K) bytes; planes_bytes = the size of each. */
int te_linear_x6_split_dual_f32(const float* A, int64_t rows, int64_t K, void* planes, void* planes_abs,
                                size_t planes_bytes, te_stream_t stream);
/* nn.GELU between the two Linear layers of an Mlp block (modules/layers_ours.py:70; ViT_LRP.py:57-69: fc1 -> act -> fc2;
 * BERT.py BertIntermediate) as a producer of operand planes -- the split passes of its two neighbours disappear (round 5):
 *   te_gelu_backward_x6_planes_f32  planes of d_h = d_a . gelu'(h), [rows, K] row-major inputs: the x_planes of the
 *                                   te_gemm_x6_f32 that forms fc1's input gradient.  Bit for bit the planes
 *                                   te_linear_x6_split_matrix_f32 builds from te_gelu_backward_f32's output, which is never
 *                                   written.
 *   te_gelu_forward_x6_planes_f32   y = gelu(x) as fp32 (te_gelu_forward_f32's bits) AND the two plane sets
 *                                   te_linear_x6_split_dual_f32 builds from y (fc2's forward product, fc2's rule).
 * K % 16 == 0; planes / planes_abs: te_linear_x6_planes_bytes(rows, K) bytes each = planes_bytes.  planes_abs = NULL (forward): the
 * second set is not written (fc2's rule then takes the signed planes with TE_X6_X_PLANES_SIGNED). */
int te_gelu_backward_x6_planes_f32(const float* dy, const float* x, int64_t rows, int64_t K, void* planes,
                                   size_t planes_bytes, te_stream_t stream);
int te_gelu_forward_x6_planes_f32(const float* x, float* y, int64_t rows, int64_t K, void* planes, void* planes_abs,
                                  size_t planes_bytes, te_stream_t stream);

/* ---- producers of the cached tensors ----------------------------------------------------
 * The attention block of baselines/ViT/ViT_LRP.py:132-152 (and its gradient, the tensor save_attn_gradients receives,
 * :144-145) on the fused qkv activation [B,N,3*H*D] ('b n (qkv h d)'), head dim 64, N <= 224 (k and v of a head stay
 * in LDS; te_attention_forward_supported says whether a shape qualifies -- callers keep stock PyTorch otherwise):
 *   forward : z_qk [B,H,N,N] = q k^T (unscaled: the QK rule's Z) ; attn [B,H,N,N] = softmax(z_qk * scale) ;
 *             out [B,N,H*D] = attn v in the 'b n (h d)' layout the projection consumes (= the AV rule's Z, strided)
 *   backward: d_attn [B,H,N,N] = d_out v^T (the attention gradient of the explanation) ; d_qkv [B,N,3*H*D]:
 *             d_v = attn^T d_out always ; need_qk != 0 additionally d_s = attn .(d_attn - rowsum(d_attn . attn)) * scale,
 *             d_q = d_s k, d_k = d_s^T q (need_qk == 0: the q / k thirds of d_qkv are left untouched -- the lowest
 *             block whose attention gradient is wanted has no consumer for them).
 * Optional operands (NULL = absent):
 *   out_planes (forward, round 6): the operand planes of `out` for the projection layer's x6 kernels -- the signed planes of
 *             out [B N, H D]; out_abs_planes (optional with them; alone it is TE_ERR_INVALID_ARG) = the planes of |out|.  Each
 *             te_linear_x6_planes_bytes(B N, H D) bytes = planes_bytes (else TE_ERR_WORKSPACE), bit for bit what
 *             te_linear_x6_split_dual_f32 writes from the fp32 tensor (te_gemm_x6_f32's x_planes / the rule's x_abs_planes).
 *             Absent: no planes are written and planes_bytes is ignored.
 *   out (backward, round 6): the block's forward output [B,N,H*D] (what te_attention_forward_f32 wrote).  The row sums of the
 *             softmax backward are then taken as sum_d d_out[i][d] out[i][d] (= sum_j attn[i][j] d_attn[i][j]: out = attn v,
 *             d_attn = d_out v^T) instead of from a pass over the two N x N tensors.  The two agree to fp32 rounding
 *             (another summation of the same quantity), not bit for bit. */
int te_attention_forward_supported(int64_t N, int64_t D);
int te_attention_forward_f32(const float* qkv, float* z_qk, float* attn, float* out, void* out_planes,
                             void* out_abs_planes, size_t planes_bytes, int64_t B, int64_t H, int64_t N, int64_t D,
                             float scale, te_stream_t stream);
int te_attention_backward_f32(const float* d_out, const float* out, const float* qkv, const float* attn, float* d_attn,
                              float* d_qkv, int64_t B, int64_t H, int64_t N, int64_t D, float scale, int need_qk,
                              te_stream_t stream);

/* The same producers for the shapes the one-workgroup-per-head kernels cannot hold (csrc/te_attn_long.hip): head dim 64,
 * N <= 640 (ViT-L/16 at 384^2: 577, baselines/ViT/ViT_LRP.py:419-425; BERT: 512), q / k / v / out / gradients as
 * [B,H,N,64] views with element strides (sb, sh, sn) -- the fused 'b n (qkv h d)' activation of ViT or the three separate
 * 'b n (h d)' activations of BERT (BERT_explainability/modules/BERT/BERT.py:307-365).
 *   forward : z_qk (optional) = q k^T unscaled ; x_scaled (optional) = z_qk * scale, WITHOUT the mask: the first operand of
 *             the Add module, BERT.py:339-342 (Add.relprop divides by x_scaled + mask: the mask must not be in it twice) ;
 *             x = x_scaled + mask[b, key] (mask [B,N] additive, NULL = none) ; attn = softmax(x) ; out = attn v
 *   backward: d_attn = d_out v^T ; d_v = attn^T d_out ; need_qk: d_q = d_s k, d_k = d_s^T q with
 *             d_s = ((d_attn - rowsum(d_attn . attn)) . attn) * scale.  Workspace: B*H*N floats.
 *             out (optional, NULL = absent and o_sb / o_sh / o_sn ignored): the block's forward output, the [B,H,N,64] view
 *             te_attention_forward_strided_f32 wrote.  The row sums sum_j d_attn . attn are then taken as d_out . out
 *             (out = attn v, d_attn = d_out v^T), which lets the row side run in ONE walk over the keys on bf16 MFMAs
 *             (csrc/te_attn_bwd6l.hip, 64 < N <= 640; other lengths: the same kernels as without it). */
int te_attention_strided_supported(int64_t N, int64_t D);
size_t te_attention_backward_strided_workspace_bytes(int64_t B, int64_t H, int64_t N);
int te_attention_forward_strided_f32(const float* q, int64_t q_sb, int64_t q_sh, int64_t q_sn,
                                     const float* k, int64_t k_sb, int64_t k_sh, int64_t k_sn,
                                     const float* v, int64_t v_sb, int64_t v_sh, int64_t v_sn,
                                     const float* mask, float* z_qk, float* x_scaled, float* attn,
                                     float* out, int64_t o_sb, int64_t o_sh, int64_t o_sn,
                                     int64_t B, int64_t H, int64_t N, int64_t D, float scale, te_stream_t stream);
int te_attention_backward_strided_f32(const float* d_out, int64_t do_sb, int64_t do_sh, int64_t do_sn,
                                      const float* out, int64_t o_sb, int64_t o_sh, int64_t o_sn,
                                      const float* q, int64_t q_sb, int64_t q_sh, int64_t q_sn,
                                      const float* k, int64_t k_sb, int64_t k_sh, int64_t k_sn,
                                      const float* v, int64_t v_sb, int64_t v_sh, int64_t v_sn,
                                      const float* attn, float* d_attn,
                                      float* d_q, int64_t dq_sb, int64_t dq_sh, int64_t dq_sn,
                                      float* d_k, int64_t dk_sb, int64_t dk_sh, int64_t dk_sn,
                                      float* d_v, int64_t dv_sb, int64_t dv_sh, int64_t dv_sn,
                                      int64_t B, int64_t H, int64_t N, int64_t D, float scale, int need_qk,
                                      void* ws, size_t ws_bytes, te_stream_t stream);

/* The LayerNorm and GELU layers around the Linear rules (modules/layers_ours.py:70-77; ViT_LRP.py:57,184,187,266;
 * BERT.py:18,52,416,463): their relprop rules are the identity, the path needs their forward values (the X / Y the
 * neighbouring rules cache) and their input gradient on the way to the attention maps.
 *   te_layernorm_forward_f32 : x [T,C] -> y = (x - mean) * rstd * weight + bias (bias may be NULL); mean, rstd [T] are
 *                              kept for the backward.  C a multiple of 4, <= 2048 (te_layernorm_supported).
 *   te_layernorm_backward_f32: dx = rstd * (a - mean_C(a) - xhat * mean_C(a * xhat)) + add,  a = dy * weight,
 *                              xhat = (x - mean) * rstd; `add` (NULL = none) is the gradient of the residual branch
 *                              that bypasses the LayerNorm (ViT_LRP.py:203-205: clone -> norm -> ... -> add).
 *   te_gelu_forward_f32      : y = 0.5 x (1 + erf(x / sqrt 2)), n a multiple of 4
 *   te_gelu_backward_f32     : dx = dy (0.5 (1 + erf(x / sqrt 2)) + x exp(-x^2 / 2) / sqrt(2 pi)) */
int te_layernorm_supported(int64_t C);
int te_layernorm_forward_f32(const float* x, const float* weight, const float* bias, float* y, float* mean, float* rstd,
                             int64_t T, int64_t C, float eps, te_stream_t stream);
int te_layernorm_backward_f32(const float* dy, const float* x, const float* weight, const float* mean, const float* rstd,
                              const float* add, float* dx, int64_t T, int64_t C, te_stream_t stream);
int te_gelu_forward_f32(const float* x, float* y, int64_t n, te_stream_t stream);
int te_gelu_backward_f32(const float* dy, const float* x, float* dx, int64_t n, te_stream_t stream);

/* ---- consumer of a relevance map ---------------------------------------------------
 * replaces baselines/ViT/imagenet_seg_eval.py:214-222 and generate_visualizations.py:99-100 (per map):
 * maps [B,g,g] -> heat [B, g*scale, g*scale] = F.interpolate(scale_factor=scale, mode='bilinear') of each map,
 * then (normalise != 0) (heat - min) / (max - min) per map; fg_mask (optional, NULL to skip) = heat > mean(heat)
 * as 0/1 floats (Res.gt(Res.mean())). */
int te_heatmap_f32(const float* maps, float* heat, float* fg_mask, int64_t B, int64_t g, int64_t scale,
                   int normalise, te_stream_t stream);

/* ---- segmentation test of a relevance map ---------------------------------------------
 * replaces, per image, the metrics of baselines/ViT/imagenet_seg_eval.py:219-232,263-273 = utils/metrices.py:26-38
 * (F1), :81-99 (average precision), :135-178 (pixel accuracy, intersection / union), in ONE launch with no host
 * synchronisation (a HIP graph captures it).  heat fp32 [B,H,W], fg_mask fp32 [B,H,W] of 0.0 / 1.0 (te_heatmap_f32's
 * outputs as they are), labels int64 [B,H,W], all contiguous.
 *   counts [B,6] = correct, labeled, inter0, inter1, union0, union1: a pixel is valid iff label >= 0; correct =
 *                  #(valid and mask == label); inter_c = #(valid and mask == c and label == c); union_c = #(valid and
 *                  mask == c) + #(label == c) - inter_c.  Labels >= 2 are valid and belong to neither class.
 *   f1 [B,H]     = the F1 of every image ROW (the script hands a 2-D mask to get_f1_scores, whose batch loop then runs
 *                  over the rows): 2 tp / (2 tp + fp + fn) with prediction mask == 1 and target label == 1 (a label of -1
 *                  is not-target); 0 for a row with 2 tp + fp + fn = 0.
 *   ap [B]       = sklearn.average_precision_score over the 2*H*W class scores: class 1 scores h, class 0 scores the
 *                  fp32 value 1 - h, truth is clamp(label, 0) == c; thresholds are the DISTINCT scores in descending
 *                  order, AP = sum_i (R_i - R_{i-1}) P_i with P_i = tp_i / n_i, R_i = tp_i / npos in fp64; 0 when no pixel is
 *                  valid or npos = 0.
 * NaN rule: a NaN heat value counts as 0 and its mask value as 0 (the clean-up of :227-230 / foreground_split).
 * Ignore rule: pixels with label < 0 drop out of counts and of both classes of AP; F1 sees them as not-target.
 * The integers are exact; the fp64 sum of AP is taken in an order fixed by the image alone, without floating-point
 * atomics: every output of image b is the same 64-bit pattern alone or in any batch, wherever the workspace lies.
 * Refused on the host before any HIP call: null pointers / non-positive sizes TE_ERR_INVALID_ARG; H*W > 2^20 or
 * B > 65535 TE_ERR_UNSUPPORTED; a workspace smaller than te_seg_metrics_workspace_bytes TE_ERR_WORKSPACE (the query
 * gives 0 for sizes the entry point refuses).  ws: 8-byte aligned. */
size_t te_seg_metrics_workspace_bytes(int64_t B, int64_t H, int64_t W);
int te_seg_metrics_f32(const float* heat, const float* fg_mask, const int64_t* labels, int64_t* counts, double* ap,
                       double* f1, int64_t B, int64_t H, int64_t W, void* ws, size_t ws_bytes, te_stream_t stream);

/* ---- map similarity (the sanity-check protocol: Adebayo et al., Sanity Checks for Saliency Maps, NeurIPS 2018) ----
 * compares, per sample, two relevance maps a, b fp32 [B,n] (contiguous rows) in TWO launches with no host synchronisation, no
 * allocation and no memset node (a HIP graph captures the call).  H, W: the image the n values are (H*W == n) when flags has
 * TE_MAPSIM_SSIM, else 0, 0.
 *   rank_sums [B,2,3] int64 = (cov, va, vb) for the plain values (index 0) and the absolute values (index 1).  Ranks: the n
 *                  values ascending in the order of te_key (-0 == +0); a run of equal values at the 0-based sorted positions
 *                  s .. e-1 gets the average rank (s + e + 1) / 2 (scipy.stats.rankdata(method="average")); the kernels keep
 *                  the integer d = 2 rank - (n + 1) = s + e - n, |d| < n; cov = sum d_a d_b, va = sum d_a^2, vb = sum d_b^2.
 *                  For n <= 2^20 every sum is below 2^60: exact, whatever the order.
 *   sim [B,4]    fp64 = pearson, spearman, spearman_abs, ssim.
 *                  spearman = (double)cov / (sqrt((double)va) * sqrt((double)vb)) clamped to [-1, 1]; NaN when va == 0 or
 *                  vb == 0 (a constant map, n == 1); exactly +-1 when |cov| == va == vb (the same or the reversed ranking:
 *                  sqrt(va) * sqrt(va) == va is not promised in floating point).  spearman_abs: the same on |a|, |b|.
 *                  pearson: two passes in fp64 over the fp32 values -- the means, then sab, saa, sbb of the centred values --
 *                  sab / (sqrt(saa) * sqrt(sbb)) clamped; NaN when saa == 0 or sbb == 0.
 *                  ssim: scikit-image's structural_similarity at its defaults for a 2-D image: 7x7 uniform window, sample
 *                  covariance (cov_norm = 49/48), C1 = (0.01 L)^2, C2 = (0.03 L)^2 with L = data_range; per window ux, uy,
 *                  vx = cov_norm (uxx - ux^2), vy, vxy = cov_norm (uxy - ux uy), S = ((2 ux uy + C1)(2 vxy + C2)) /
 *                  ((ux^2 + uy^2 + C1)(vx + vy + C2)); the mean of S over the (H-6)(W-6) windows inside the image (what
 *                  the border crop leaves), window statistics in fp64.  NaN without TE_MAPSIM_SSIM.
 * NaN rule: a sample with a NaN anywhere in a or b gives an all-NaN sim row and an all-zero rank_sums row (scipy's
 * nan_policy="propagate"); its neighbours in the batch are unaffected.  +-inf are ordinary values for the ranks.
 * The integers are exact; every fp64 sum runs in an order fixed by the sample alone, without floating-point atomics: every
 * output of sample b is the same bit pattern alone or in any batch, wherever the workspace lies.
 * Refused on the host before any HIP call: null pointers, sizes <= 0, unknown flag bits, SSIM with H*W != n or H < 7 or
 * W < 7 TE_ERR_INVALID_ARG; n > 2^20 or B > 65535 TE_ERR_UNSUPPORTED; a workspace smaller than
 * te_map_similarity_workspace_bytes TE_ERR_WORKSPACE (the query gives 0 for sizes the entry point refuses).
 * ws: 8-byte aligned. */
#define TE_MAPSIM_SSIM 1
size_t te_map_similarity_workspace_bytes(int64_t B, int64_t n);
int te_map_similarity_f32(const float* a, const float* b, int64_t* rank_sums, double* sim, int64_t B, int64_t n, int64_t H,
                          int64_t W, int flags, double data_range, void* ws, size_t ws_bytes, te_stream_t stream);

/* ---- rationale test of a BERT relevance vector (ERASER Movie Reviews) ---------------------
 * replaces, per document, the rationale production of BERT_rationale_benchmark/models/pipeline/bert_pipeline.py:547-582
 * (clamp(min=0) :552, scores_per_word_from_scores_per_token :96-138, sixteen topk calls :567-569) and the per-document
 * part of BERT_rationale_benchmark/metrics.py:168-215 (hard rationales) and :217-253 (soft scores), in ONE launch with
 * no host synchronisation (a HIP graph captures it).  scores fp32 [B,N] relevance per wordpiece; word_ids int32 [B,N]:
 * the word a wordpiece belongs to, -1 for [CLS] / [SEP] / [UNK] / [PAD] and for everything beyond the scored words (ids
 * >= Wmax are ignored as well); truth uint8 [B,Wmax]: the human rationale, nonzero = rationale word; ks: HOST array of
 * n_ks <= TE_RATIONALE_MAX_KS positive rationale sizes.  flags: TE_RATIONALE_CLAMP clamps the scores at 0 first (:552).
 *   word_scores [B,Wmax] fp32 = the maximum over the word's wordpieces (:109-124); a word without a wordpiece, and every
 *                  entry at or past n_words, is 0.
 *   n_words [B]  int32 = highest word id + 1.
 *   order [B,Wmax] int32 = the word indices by descending score, ties in ASCENDING WORD INDEX (torch.topk leaves ties
 *                  unspecified, and after the clamp every non-positive word ties at 0: the rule of te_perturb_f32); -1 at
 *                  and past n_words.
 *   counts [B,n_ks,2] int32 = (tp_k, pred_k): pred_k = min(k, n_words) (the reference's topk raises for k > n_words; this
 *                  library clips), tp_k = the rationale words among the first pred_k of order.
 *   soft [B,4]   fp64 = average precision, AUPRC, ROC-AUC, npos of the word scores against truth over the n_words words
 *                  (sklearn.average_precision_score, auc(precision_recall_curve), roc_auc_score): with (tp_i, n_i) at
 *                  the end of the i-th run of equal scores in descending order, P_i = tp_i / n_i, R_i = tp_i / npos,
 *                  F_i = (n_i - tp_i) / nneg, P_0 = 1, R_0 = F_0 = 0:  AP = sum (R_i - R_{i-1}) P_i,
 *                  AUPRC = sum (R_i - R_{i-1}) (P_i + P_{i-1}) / 2,  ROC-AUC = sum (F_i - F_{i-1}) (R_i + R_{i-1}) / 2.
 *                  A document of one class (npos = 0 or npos = n_words) gets 0 for all three; npos tells the caller to
 *                  discard it, as _score_aggregator(..., True) does.
 * NaN rule: a NaN score counts as 0 (sklearn raises on NaN; the explanation path never produces one).
 * Integers and the word maximum are exact; the fp64 sums run in an order fixed by the document alone, without
 * floating-point atomics: every output of document b is the same bit pattern alone or in any batch.
 * Refused on the host before any HIP call: null pointers, non-positive sizes, n_ks outside 1..16, a non-positive k or
 * unknown flag bits TE_ERR_INVALID_ARG; N or Wmax > 2048 or B > 65535 TE_ERR_UNSUPPORTED; a workspace smaller than
 * te_rationale_metrics_workspace_bytes TE_ERR_WORKSPACE (the query gives 0 for sizes the entry point refuses).
 * ws: 8-byte aligned. */
#define TE_RATIONALE_MAX_KS 16
#define TE_RATIONALE_CLAMP 1
size_t te_rationale_metrics_workspace_bytes(int64_t B, int64_t N, int64_t Wmax);
int te_rationale_metrics_f32(const float* scores, const int32_t* word_ids, const uint8_t* truth, float* word_scores,
                             int32_t* n_words, int32_t* order, int32_t* counts, double* soft, int64_t B, int64_t N,
                             int64_t Wmax, const int64_t* ks, int64_t n_ks, int flags, void* ws, size_t ws_bytes,
                             te_stream_t stream);

/* ---- erased inputs of ERASER's faithfulness numbers ----------------------------------------------------
 * builds, in ONE launch, every erased copy of a batch that comprehensiveness and sufficiency (metrics.py:255-282,
 * 301-313) need.  THE REFERENCE TREE HAS NO PRODUCER FOR THESE, only the consumer: what follows is this project's
 * definition.  input_ids / attention_mask int64 [B,N]; word_ids int32 [B,N], order int32 [B,Wmax] and n_words int32 [B]
 * as te_rationale_metrics_f32 takes / gives them; fractions: HOST array of n_t <= TE_TOKEN_ERASE_MAX_FRACTIONS values
 * in (0, 1] (metrics.py:610 defaults to 0.01, 0.05, 0.1, 0.2, 0.5).  For fraction t the rationale of document b is the
 * first m = min(n_words, max(1, ceil(t * n_words))) entries of order (the product and ceil in IEEE fp64, i.e. the value
 * the host computes; 0 for a document without words) -> n_rationale int32 [n_t,B].
 *   ids_out / mask_out int64 [2,n_t,B,N]: copy [0][t] (comprehensiveness) drops every wordpiece of a rationale word,
 *   copy [1][t] (sufficiency) keeps only those.  Tokens with word id -1 and mask 1 ([CLS], [SEP], [UNK]) are kept in
 *   both; tokens with mask 0 are dropped.  The kept tokens are compacted to the left in their original order with
 *   mask 1; the rest is pad_id with mask 0.
 * Refused on the host before any HIP call: null pointers, non-positive sizes, n_t outside 1..8, a fraction outside
 * (0, 1] TE_ERR_INVALID_ARG; N or Wmax > 2048 or B > 65535 TE_ERR_UNSUPPORTED. */
#define TE_TOKEN_ERASE_MAX_FRACTIONS 8
int te_token_erase(const int64_t* input_ids, const int64_t* attention_mask, const int32_t* word_ids,
                   const int32_t* order, const int32_t* n_words, int64_t* ids_out, int64_t* mask_out,
                   int32_t* n_rationale, int64_t B, int64_t N, int64_t Wmax, const double* fractions, int64_t n_t,
                   int64_t pad_id, te_stream_t stream);

/* ---- Conv2d.relprop, z^B rule of the patch embedding (method="full") ------------------
 * replaces modules/layers_ours.py:242-256 (= modules/layers_lrp.py:223-237), the `X.shape[1] == 3` branch, for a
 * convolution with stride == kernel == p and no padding (baselines/ViT/ViT_LRP.py:215-242, PatchEmbed):
 *   Za = conv(X,W) - conv(L,W+) - conv(H,W-) + 1e-9 ; S = R / Za ; out = X convT(S,W) - L convT(S,W+) - H convT(S,W-)
 * with L / H = per-sample pixel min / max.  R: relevance of the conv output in TOKEN-MAJOR layout [B, P, E]
 * (P = (H/p)(W/p); what PatchEmbed.relprop holds before its transpose), consecutive samples r_bs floats apart
 * (r_bs >= P*E; (P+1)*E when R is cam[:, 1:] of a [B, P+1, E] tensor).  X [B,C,H,W]; W [E,C,p,p]; Y [B,E,H/p,W/p] =
 * the layer's forward output (conv(X,W) is taken as Y - bias; bias may be NULL); out [B,C,H,W].
 * flags: TE_IMPL_SIMPLE selects the one-thread-per-element C-pass. */
size_t te_conv2d_zb_relprop_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W, int64_t E, int64_t p);
int te_conv2d_zb_relprop_f32(const float* R, int64_t r_bs, const float* X, const float* W, const float* Y,
                             const float* bias, float* out, int64_t B, int64_t C, int64_t H, int64_t W_, int64_t E,
                             int64_t p, int flags, void* ws, size_t ws_bytes, te_stream_t stream);

/* ---- perturbation-test input builder ---------------------------------------------------
 * replaces baselines/ViT/pertubation_eval_from_hdf5.py:88-101 for ALL perturbation steps of a batch in two launches:
 *   for each step s:  idx = topk(vis[b], ks[s]) ; out[s][b][c][idx] = 0 for every channel c, data elsewhere ;
 *                     out = (out - mean[c]) / std[c]
 * vis [B,HW] relevance per pixel (negate it first for the script's --neg mode); data [B,C,HW] pixels; ks: HOST array
 * of n_steps pixel counts (int(base_size * step)), clamped to [0, HW]; mean / std: HOST arrays [C] (NULL = 0 / 1);
 * out [n_steps,B,C,HW].  Equal relevance values are removed in ascending pixel-index order (torch.topk leaves the
 * order among ties unspecified).  NaN relevance counts as largest, as in torch.topk. */
#define TE_PERTURB_MAX_STEPS 16
#define TE_PERTURB_MAX_CHANNELS 4
size_t te_perturb_workspace_bytes(int64_t B, int64_t n_steps);
int te_perturb_f32(const float* vis, const float* data, float* out, int64_t B, int64_t C, int64_t HW,
                   const int64_t* ks, int64_t n_steps, const float* mean, const float* std_, void* ws,
                   size_t ws_bytes, te_stream_t stream);

/* ---- deletion / insertion curves (RISE: Petsiuk et al., BMVC 2018, CausalMetric) ----------------------------------
 * THE REFERENCE TREE HAS NO SUCH PROTOCOL: what follows is this project's definition, restated in torch by curves.py.
 * Inputs: data [B,C,H,W] fp32 in [0,1]; vis [B,HW] fp32 relevance; target [B] int64; mean[c], std[c] HOST arrays [C] (NULL =
 * 0 / 1), C <= TE_PERTURB_MAX_CHANNELS.  z = (data - mean[c]) / std[c] is the normalised image (the fp32 expression of
 * te_perturb_f32).  No entry synchronises, reads back or issues a memset node: a HIP graph captures every call.
 *
 * Order.  rank [B,n] int32: rank[b,p] = the position of pixel p when vis[b] is sorted by DESCENDING value, equal values in
 *   ASCENDING pixel index; the comparison is te_perturb_f32's (-0 == +0, a positive NaN is largest, a negative NaN
 *   smallest); rank 0 is the most relevant pixel.  torch.sort(vis, 1, descending=True, stable=True), scattered back.
 *   n <= 2^20, B <= 65535; integers only.  One workgroup per sample: four stable 8-bit passes over ~key << 32 | index,
 *   ping-pong in the workspace (8-byte aligned).
 * Steps.  step >= 1 pixels per step, S = ceil(HW / step); image i (0 <= i <= S) has the k_i = min(i step, HW) top-ranked
 *   pixels switched: S + 1 images per sample and curve.
 * Substrate sub [B,C,HW] in normalised space: a device tensor (te_blur_normalised_f32 gives RISE's blur) or, when
 *   substrate == NULL, the constant fill[c] (HOST array [C], already normalised: 0 = the mean colour, (0 - mean[c]) / std[c]
 *   = black).
 * Images.  deletion (insertion == 0): x_i[b,c,p] = rank[b,p] < k_i ? sub : z;  insertion (== 1): rank[b,p] < k_i ? z : sub.
 *   te_curve_inputs_* writes the images s0 .. s0 + n_s - 1 to out [n_s,B,C,HW], fp32 or bf16 (the fp32 value rounded once,
 *   to nearest even).  HW <= 2^20.
 * Blur.  taps: HOST array of klen fp32 values (curves.gaussian_taps: RISE's gkern computed in fp64), klen odd,
 *   <= TE_BLUR_MAX_TAPS; r = klen / 2.  out[y,x] = sum_i t_i sum_j t_j z[y+i-r, x+j-r], out-of-image terms 0 (zero padding in
 *   normalised space, conv2d(..., padding=klen//2)).  fp32: the horizontal pass first, then the vertical one, taps in index
 *   order from a zero accumulator, one FMA per tap, out-of-image terms included as zeros: the bits of a pixel do not depend
 *   on tiling, batch or grid.  H W <= 2^20.
 * Scores.  logits [n_s B, K] fp32 or bf16, row (s - s0) B + b; prob fp64 [S+1,B] (the base of the table: the call writes rows
 *   s0 .. s0 + n_s - 1): prob[i,b] = softmax(logits_i[b])[target[b]] in fp64, max-subtracted, summed in a fixed order; NaN for
 *   a target outside [0, K).
 * AUC.  auc[b] = (sum_i prob[i,b] - prob[0,b] / 2 - prob[S,b] / 2) / S, S = S1 - 1 >= 1, summed in step order in fp64.
 * Refused on the host before any HIP call: null pointers (substrate AND fill NULL), sizes <= 0, klen even or < 1, step < 1,
 *   s0 < 0, n_s < 1, s0 + n_s > S + 1, insertion not 0 / 1, S1 < 2 TE_ERR_INVALID_ARG; klen > TE_BLUR_MAX_TAPS, n or HW > 2^20,
 *   B > 65535, C > TE_PERTURB_MAX_CHANNELS TE_ERR_UNSUPPORTED; a workspace smaller than te_pixel_rank_workspace_bytes
 *   TE_ERR_WORKSPACE (the query gives 0 for sizes the entry point refuses). */
#define TE_BLUR_MAX_TAPS 63
int te_blur_normalised_f32(const float* data, float* out, int64_t B, int64_t C, int64_t H, int64_t W, const float* taps,
                           int64_t klen, const float* mean, const float* std_, te_stream_t stream);
size_t te_pixel_rank_workspace_bytes(int64_t B, int64_t n);
int te_pixel_rank_f32(const float* vis, int32_t* rank, int64_t B, int64_t n, void* ws, size_t ws_bytes, te_stream_t stream);
int te_curve_inputs_f32(const float* data, const float* substrate, const float* fill, const int32_t* rank, float* out,
                        int64_t B, int64_t C, int64_t HW, int64_t step, int64_t s0, int64_t n_s, int insertion,
                        const float* mean, const float* std_, te_stream_t stream);
int te_curve_inputs_bf16(const float* data, const float* substrate, const float* fill, const int32_t* rank, te_bf16_t* out,
                         int64_t B, int64_t C, int64_t HW, int64_t step, int64_t s0, int64_t n_s, int insertion,
                         const float* mean, const float* std_, te_stream_t stream);
int te_curve_scores_f32(const float* logits, const int64_t* target, double* prob, int64_t B, int64_t K, int64_t s0,
                        int64_t n_s, te_stream_t stream);
int te_curve_scores_bf16(const te_bf16_t* logits, const int64_t* target, double* prob, int64_t B, int64_t K, int64_t s0,
                         int64_t n_s, te_stream_t stream);
int te_curve_auc_f64(const double* prob, double* auc, int64_t S1, int64_t B, te_stream_t stream);

/* ---- localisation test (pointing game: Zhang et al., IJCV 2018; energy-based pointing game / relevance mass accuracy: Wang
 * et al., CVPRW 2020, Arras et al., Information Fusion 2022; relevance rank accuracy: Arras et al. 2022) --------------------
 * THE REFERENCE TREE HAS NO SUCH PROTOCOL: what follows is this project's definition, restated in torch by localisation.py.
 * Scores P (image, class) pairs, each a heat map against a ground-truth region, in ONE launch (one workgroup per pair) with no
 * host synchronisation, no allocation and no memset node: a HIP graph captures the call.
 * Inputs, all contiguous: heat fp32 [P,H,W], one map per pair; EXACTLY ONE of labels int64 [B,H,W] (mask mode) and boxes int64
 *   [P,M,4] = x0, y0, x1, y1 (box mode), the other NULL; image_index int64 [P] or NULL: pair p reads labels[image_index[p]]
 *   (NULL: labels[p]), so the K pairs of one image share one label map and nothing is materialised as [P,H,W]; target_id
 *   int64 [P] (mask mode; not read in box mode).
 * Valid and target pixels.  Mask mode: a pixel is valid iff label >= 0, and a target iff it is valid and label == target_id[p].
 *   Box mode: every pixel is valid; a pixel (x, y) is a target iff it lies in the union of the pair's M boxes, x0 <= x < x1 and
 *   y0 <= y < y1 (half-open pixel coordinates: that test clips a box to the image); a row with x1 <= x0 or y1 <= y0 is empty
 *   (the padding row).
 * Heat values: a NaN counts as +0.0 everywhere (the clean-up of te_seg_metrics_f32), -0 == +0, the order is te_key's.
 *   stats [P,5] int64 = n_valid, n_target, argmax, d2_min, topk_hits.
 *     argmax    = the flat index y W + x of the largest valid pixel, ties to the lowest index; -1 when no pixel is valid.
 *     d2_min    = the minimum over the target pixels of dy^2 + dx^2 from the argmax pixel, an exact integer: a distance, not a
 *                 flag -- the caller picks the tolerance afterwards, a pointing-game hit is 0 <= d2_min <= tol^2; -1 when there
 *                 is no target or no valid pixel.
 *     topk_hits = the number of target pixels among the n_target highest-ranked valid pixels, ranked by descending value with
 *                 ties in ascending pixel index (the order of te_pixel_rank_f32 and te_perturb_f32); rank accuracy is
 *                 topk_hits / n_target.
 *   energy [P,2] fp64 = e_target, e_valid: the sums of max(h, 0) over the target and over the valid pixels; the quotient and its
 *                 0/0 rule are the caller's.
 * Skipped pairs: target_id[p] < 0 (mask mode) or image_index[p] outside [0, B) (either mode; never used as an address) gives
 *   the rows {0, 0, -1, -1, 0} and {0, 0}; the neighbours of the pair are unaffected.  Box mode without image_index skips nothing.
 * The integers are exact; the fp64 sums run in an order fixed by the image size alone, without floating-point atomics: every
 * output of pair p is the same 64-bit pattern alone or in any batch, wherever the workspace lies.
 * Refused on the host before any HIP call, in this order: null pointers (heat, stats, energy; target_id with labels),
 *   sizes <= 0, both or neither of labels / boxes, M <= 0 with boxes, a workspace address that is not 8-byte aligned
 *   TE_ERR_INVALID_ARG; H*W > 2^20, P > 65535 or M > 64
 *   TE_ERR_UNSUPPORTED; a workspace smaller than te_localisation_workspace_bytes TE_ERR_WORKSPACE (the query gives 0 for sizes
 *   the entry point refuses).  ws: per pair H*W 4-byte keys and H*W mask bits. */
size_t te_localisation_workspace_bytes(int64_t P, int64_t H, int64_t W);
int te_localisation_f32(const float* heat, const int64_t* labels, const int64_t* image_index, const int64_t* target_id,
                        const int64_t* boxes, int64_t M, int64_t* stats, double* energy, int64_t P, int64_t B, int64_t H,
                        int64_t W, void* ws, size_t ws_bytes, te_stream_t stream);

/* ---- robustness and complexity (max- / average-sensitivity: Yeh et al., NeurIPS 2019; local Lipschitz estimate: Alvarez-Melis
 * & Jaakkola, 2018; Gini sparseness: Chalasani et al., ICML 2020; entropy: Bhatt et al., IJCAI 2020; effective complexity:
 * Nguyen & Martinez, 2020) -------------------------------------------------------------------------------------------------
 * THE REFERENCE TREE HAS NO SUCH PROTOCOL: what follows is this project's definition, restated in numpy / torch by
 * robustness.py.  No entry synchronises, reads back or issues a memset node: a HIP graph captures every call.  There are no
 * floating-point atomics: every output of sample b is the same bit pattern alone or in any batch.
 *
 * Noise.  x [B,n] fp32: the model's input, already normalised, n = C H W.  out [B,n_d,n], fp32 or bf16: row b n_d + j is draw
 *   d = d0 + j of the sample whose global id is id0 + b (64-bit, wrapping).  Element e takes word e & 3 of Philox4x32-10
 *   (Salmon et al., SC 2011: multipliers 0xD2511F53, 0xCD9E8D57, Weyl increments 0x9E3779B9, 0xBB67AE85, ten rounds) with the
 *   counter (e >> 2, d, low32(id), high32(id)) and the key (low32(seed), high32(seed)); the 64 bits of seed are read as
 *   unsigned.  From the word w, in this order: u = float(w >> 8) * 2^-24 (exact); s = 2 u - 1 (exact); delta = s * radius (one
 *   fp32 rounding); y = x + delta (one fp32 rounding) -- never an FMA: torch's x + s * radius gives the same bits.  _bf16
 *   rounds y once more, to nearest even.  radius == 0 gives exact copies.  The draws are uniform in the L-infinity ball of
 *   that radius (s in [-1, 1 - 2^-23]).  A sample's copies depend on (element, draw, id, seed) alone: the same bits alone, in
 *   any batch and in any chunking (d0, n_d) of the draws.  16-byte accesses where n % 4 == 0 (bf16: n % 8 == 0) and x, out
 *   are 16-byte aligned; an element-wise form otherwise.
 * Distance.  a [B,n] fp32, b [B,D,n] fp32 or bf16, sums [B,D,3] fp64 = sum_e (b - a)^2, sum_e a^2, sum_e b^2, every term
 *   formed in fp64 from the exact upcasts.  Thread t of 256 takes the groups of four elements t, t + 256, ... in order, then
 *   the 64 lanes of a wave and the four waves meet in a fixed order: the order depends on n alone.
 * Complexity.  maps [B,n] fp32; v = |maps[b]|, S = sum v (fp64).  out [B,2] fp64 = gini, entropy; counts [B,2] int64.
 *     gini    = sum_k (2k - n - 1) v_(k) / (n S) over v sorted ascending, k = 1 .. n (ties do not change it; every product is
 *               exact in fp64); 0 for n == 1.
 *     entropy = 0 - sum p ln p, p = v / S in fp64, 0 ln 0 = 0 (natural logarithm).
 *     counts  = the number of v > eps max v, compared in fp64 as (double)v > eps * (double)max v (the effective complexity at
 *               the relative threshold eps), and the number of v > 0.
 *   S == 0 gives NaN, NaN, 0, 0.  A NaN anywhere in the row gives a NaN row and zero counts; its neighbours are unaffected.
 *   One workgroup per sample; the order is that of te_key on te_key(v) << 32 | index, four stable 8-bit passes ping-pong in
 *   the workspace (8-byte aligned), as te_map_similarity_f32.  n <= 2^20, B <= 65535.
 * Refused on the host before any HIP call: null pointers, sizes <= 0, radius or eps negative or not finite, d0 < 0,
 *   d0 + n_d > 2^32 TE_ERR_INVALID_ARG; B > 65535, n > 2^20 (complexity), n > 2^31 - 1 (noise, distance), D > 2^31 - 1
 *   TE_ERR_UNSUPPORTED; a workspace smaller than te_map_complexity_workspace_bytes TE_ERR_WORKSPACE (the query gives 0 for
 *   sizes the entry point refuses). */
int te_noise_inputs_f32(const float* x, float* out, int64_t B, int64_t n, int64_t d0, int64_t n_d, float radius, int64_t seed,
                        int64_t id0, te_stream_t stream);
int te_noise_inputs_bf16(const float* x, te_bf16_t* out, int64_t B, int64_t n, int64_t d0, int64_t n_d, float radius,
                         int64_t seed, int64_t id0, te_stream_t stream);
int te_map_distance_f32(const float* a, const float* b, double* sums, int64_t B, int64_t D, int64_t n, te_stream_t stream);
int te_map_distance_bf16(const float* a, const te_bf16_t* b, double* sums, int64_t B, int64_t D, int64_t n,
                         te_stream_t stream);
size_t te_map_complexity_workspace_bytes(int64_t B, int64_t n);
int te_map_complexity_f32(const float* maps, double* out, int64_t* counts, int64_t B, int64_t n, double eps, void* ws,
                          size_t ws_bytes, te_stream_t stream);

/* ---- faithfulness (infidelity: Yeh et al., NeurIPS 2019, captum's `infidelity`; faithfulness correlation: Bhatt et al.,
 * IJCAI 2020) -- csrc/te_faithful.hip -------------------------------------------------------------------------------------
 * THE REFERENCE TREE HAS NO SUCH PROTOCOL: what follows is this project's definition, restated in numpy / torch by
 * faithfulness.py.  Parity with captum or quantus is not claimed.  No entry synchronises, reads back or issues a memset node:
 * a HIP graph captures every call.  There are no floating-point atomics: every output of sample b is the same bit pattern
 * alone, in any batch and in any chunking (d0, n_d) of the draws.
 *
 * Subsets.  The image [C,H,W] is cut into G = g_h g_w cells of p x p pixels, H = g_h p, W = g_w p; cell c = row g_w + col.
 *   Draw d of the sample with the global 64-bit id `id` (id0 + b, wrapping) gives cell c the key (w_c << 32) | c, where w_c
 *   is word c & 3 of Philox4x32-10 (the generator of the noise above) with the counter (0x80000000 | (c >> 2), d, low32(id),
 *   high32(id)) and the key (low32(seed), high32(seed)); the 64 bits of seed are read as unsigned.  The set top bit of the
 *   first counter word keeps this stream apart from the noise stream, whose first word stays below 2^29.  S(id, d) is the k
 *   cells with the smallest keys, 1 <= k <= G; ties cannot occur, because the index is part of the key.
 * Subset inputs.  x [B,C,H,W] fp32: the normalised input the model saw, upcast.  The substrate, in normalised space, is a
 *   [B,C,H,W] fp32 tensor or, when that pointer is NULL, the C per-channel constants `fill` (C <= TE_PERTURB_MAX_CHANNELS
 *   then).  out [B,n_d,C,H,W], fp32 or bf16: row b n_d + j is draw d0 + j of sample id0 + b; a pixel whose cell is in
 *   S(id0 + b, d0 + j) takes the substrate's value, every other pixel x's.  The bits are copied; _bf16 rounds once, to
 *   nearest even.  member [B,n_d,G] uint8: 1 for the cells of S, else 0.  attr [B,G] fp32 (the token-level map) may be NULL;
 *   when it is given, attr_sum [B,n_d] fp64 = sum over c in S of (double)attr[b,c]: thread t of 256 adds its cells t, t + 256,
 *   ... in order, then the 64 lanes of a wave and the four waves meet in a fixed order -- an order fixed by G alone.
 *   Two launches on the stream: one workgroup per (sample, draw) ranks the keys in LDS by counting and writes member and
 *   attr_sum; a store-shaped pass then writes the images, 16-byte accesses where p % 4 == 0 (bf16: p % 8 == 0) and x, out and
 *   the substrate are 16-byte aligned, an element-wise form otherwise.
 * Perturbation dot.  x [B,n] fp32, y [B,D,n] fp32 or bf16, w [B,m] fp32 with n % m == 0 (the pixel-level attribution, shared
 *   by the n / m channels).  sums [B,D,2] fp64 = sum_e (x_e - y_e) w_(e mod m), sum_e (x_e - y_e)^2, every term formed in
 *   fp64 from the exact upcasts.  The summation order is that of te_map_distance_*: thread, then lane, then wave; it depends
 *   on n alone, and the second sum has the bits of te_map_distance_*'s first.
 * Scores (torch, fp64, on the device: faithfulness.scores_from_sums) from ip [B,D] = the first sum, delta [B,D] = f(clean) -
 *   f(copy) and, in subset mode, attr_sum [B,D]:
 *     infidelity      = mean_d (ip - delta)^2
 *     beta            = sum_d ip delta / sum_d ip^2, or 1 when the denominator is 0 (captum's normalize=True)
 *     infidelity_norm = mean_d (beta ip - delta)^2
 *     faith_corr      = Pearson_d(attr_sum, delta) from centred sums, clamped to [-1, 1]; NaN for D < 2 or a constant side.
 * Refused on the host before any HIP call: null pointers (x, out, member; substrate and fill both; attr without attr_sum; x, y,
 *   w, sums), sizes <= 0, k outside [1, G], d0 < 0, d0 + n_d > 2^32, n % m != 0 TE_ERR_INVALID_ARG; G > TE_SUBSET_MAX_CELLS,
 *   B > 65535, C H W > 2^31 - 1, n_d > 2^31 - 1, constants for C > TE_PERTURB_MAX_CHANNELS, n > 2^31 - 1, D > 2^31 - 1
 *   TE_ERR_UNSUPPORTED. */
#define TE_SUBSET_MAX_CELLS 4096
int te_subset_inputs_f32(const float* x, const float* substrate, const float* fill, const float* attr, float* out,
                         uint8_t* member, double* attr_sum, int64_t B, int64_t C, int64_t g_h, int64_t g_w, int64_t p,
                         int64_t k, int64_t d0, int64_t n_d, int64_t seed, int64_t id0, te_stream_t stream);
int te_subset_inputs_bf16(const float* x, const float* substrate, const float* fill, const float* attr, te_bf16_t* out,
                          uint8_t* member, double* attr_sum, int64_t B, int64_t C, int64_t g_h, int64_t g_w, int64_t p,
                          int64_t k, int64_t d0, int64_t n_d, int64_t seed, int64_t id0, te_stream_t stream);
int te_perturbation_dot_f32(const float* x, const float* y, const float* w, double* sums, int64_t B, int64_t D, int64_t n,
                            int64_t m, te_stream_t stream);
int te_perturbation_dot_bf16(const float* x, const te_bf16_t* y, const float* w, double* sums, int64_t B, int64_t D, int64_t n,
                             int64_t m, te_stream_t stream);

/* ---- bf16 operands (a bf16 ViT / DeiT or BERT model: model.to(torch.bfloat16)) ----------------------------
 * The rules of variant "ours", alpha = 1, evaluated in fp32 on the model's own bf16 tensors (te_bf16_t, read exactly:
 * bf16 -> fp32 is exact).  Relevance operands and outputs, safe_divide, per-sample sums and factors are fp32 as in the
 * _f32 entry points; the arguments mean what they mean there.  csrc/te_bf16.hip (GEMM-shaped rules, bf16 MFMAs) and
 * csrc/te_elementwise.hip (streaming rules, the _f32 kernels templated on the operand type).
 *
 * Linear.relprop: Z = X+ W+^T + X- W-^T from the bf16 X and W (never from the cached output Y), S = sd(R f, Z) kept as
 * three bf16 planes, out = X+ (S W+) + X- (S W-).  R [T, r_ld >= out_f] fp32 with the optional per-sample factor
 * r_scale[(t / rows_per_scale) * r_scale_stride]; X [T, x_ld >= in_f] bf16 (a row stride: cls rows in place); w_planes =
 * te_linear_bf16_prepare_weights of W [out_f, in_f] bf16 (build once per weight version); out [T, in_f] fp32.
 * Shapes: te_linear_relprop_bf16_supported (in_f, out_f multiples of 128); TE_ERR_UNSUPPORTED otherwise. */
int te_linear_relprop_bf16_supported(int64_t T, int64_t in_f, int64_t out_f);
size_t te_linear_relprop_bf16_workspace_bytes(int64_t T, int64_t in_f, int64_t out_f);
size_t te_linear_bf16_weight_planes_bytes(int64_t in_f, int64_t out_f);
int te_linear_bf16_prepare_weights(const te_bf16_t* W, int64_t in_f, int64_t out_f, void* planes, size_t planes_bytes,
                                   te_stream_t stream);
int te_linear_relprop_bf16(const float* R, int64_t r_ld, const float* r_scale, int64_t r_scale_stride,
                           int64_t rows_per_scale, const te_bf16_t* X, int64_t x_ld, const void* w_planes, float* out,
                           int64_t T, int64_t in_f, int64_t out_f, void* ws, size_t ws_bytes, te_stream_t stream);
/* The two attention rules with bf16 operands: the argument lists of te_matmul_relprop_av_f32 and
 * te_matmul_relprop_qk_f32.  attn, Z (QK) contiguous; q / k / v / Z (AV) strided with a contiguous last dim
 * (views of the fused qkv activation are read in place).  Z == NULL: recomputed in fp32 from the bf16 operands.
 * Shapes: te_matmul_relprop_bf16_supported (head dim 64, N <= 1024); variant ours only. */
int te_matmul_relprop_bf16_supported(int64_t N, int64_t D);
size_t te_matmul_relprop_av_bf16_workspace_bytes(int64_t B, int64_t H, int64_t N, int64_t D);
size_t te_matmul_relprop_qk_bf16_workspace_bytes(int64_t B, int64_t H, int64_t N, int64_t D);
int te_matmul_relprop_av_bf16(const float* R, int64_t r_sb, int64_t r_sh, int64_t r_sn,
                              const te_bf16_t* attn,
                              const te_bf16_t* v, int64_t v_sb, int64_t v_sh, int64_t v_sn,
                              const te_bf16_t* Z, int64_t z_sb, int64_t z_sh, int64_t z_sn,
                              float* cam_attn,
                              float* cam_v, int64_t cv_sb, int64_t cv_sh, int64_t cv_sn,
                              int64_t B, int64_t H, int64_t N, int64_t D, float out_scale, int variant,
                              void* ws, size_t ws_bytes, te_stream_t stream);
int te_matmul_relprop_qk_bf16(const float* R_nn, const float* r_scale, int64_t r_scale_stride,
                              const te_bf16_t* q, int64_t q_sb, int64_t q_sh, int64_t q_sn,
                              const te_bf16_t* k, int64_t k_sb, int64_t k_sh, int64_t k_sn,
                              const te_bf16_t* Z,
                              float* cam_q, int64_t cq_sb, int64_t cq_sh, int64_t cq_sn,
                              float* cam_k, int64_t ck_sb, int64_t ck_sh, int64_t ck_sn,
                              int64_t B, int64_t H, int64_t N, int64_t D, float out_scale, int variant,
                              void* ws, size_t ws_bytes, te_stream_t stream);
/* Streaming rules: the _f32 entry points with bf16 operands X0 / X1 / X / grad (workspaces as there). */
int te_add_relprop_bf16(const float* R, const te_bf16_t* X0, const te_bf16_t* X1, float* out0, float* out1, int64_t B,
                        int64_t n, int64_t x1_batch_stride, int variant, void* ws, size_t ws_bytes, te_stream_t stream);
int te_add_relprop_deferred_bf16(const float* R, const te_bf16_t* X0, const te_bf16_t* X1, float* a, float* b,
                                 float* fac, int64_t B, int64_t n, int64_t x1_batch_stride, void* ws, size_t ws_bytes,
                                 te_stream_t stream);
/* The broadcast-mask Add of BERT self-attention (te_add_bcast_relprop_f32 / _deferred_f32) with bf16 X0 [B,H,N,N] and
 * mask [B,N]: same arguments, workspace (te_add_bcast_relprop_workspace_bytes), N <= 2048 and validation; variant ours
 * only.  Same arithmetic and summation order: the _f32 call's bits on exact fp32 copies of X0 and the mask. */
int te_add_bcast_relprop_bf16(const float* R, const te_bf16_t* X0, const te_bf16_t* mask, float* out0, float* out1,
                              int64_t B, int64_t H, int64_t N, int variant, void* ws, size_t ws_bytes,
                              te_stream_t stream);
int te_add_bcast_relprop_deferred_bf16(const float* R, const te_bf16_t* X0, const te_bf16_t* mask, float* a,
                                       float* out1, float* fac, int64_t B, int64_t H, int64_t N, void* ws,
                                       size_t ws_bytes, te_stream_t stream);
int te_clone_relprop_bf16(const float* R0, const float* R1, const float* R2, const te_bf16_t* X, float* out, int64_t n,
                          te_stream_t stream);
int te_clone_relprop_scaled_bf16(const float* R0, const float* s0, int64_t s0_stride, const float* R1, const float* s1,
                                 int64_t s1_stride, const float* R2, const float* s2, int64_t s2_stride,
                                 const te_bf16_t* X, float* out, int64_t B, int64_t n, te_stream_t stream);
int te_index_select_relprop_bf16(const float* R, const te_bf16_t* X, float* out, int64_t B, int64_t N, int64_t C,
                                 int64_t index, te_stream_t stream);
int te_gradcam_headmean_bf16(const te_bf16_t* grad, const float* cam, float* out, int64_t B, int64_t H, int64_t N,
                             te_stream_t stream);
/* Head mean of a bf16 model's attention probabilities, the input of the attention rollouts and of the last-layer
 * baselines (ViT_explanation_generator.py:74-83, ViT_LRP.py:391-397, ExplanationGenerator.py:108-127):
 *   out[b,i,j] = (sum_h f(attn[b,h,i,j])) / H,   f = identity, or max(., 0) with TE_HEADMEAN_CLAMP,
 * heads added in index order in fp32, one division at the end (torch's mean on the exact fp32 upcast).  attn: element
 * (b,h,i,j) at attn + b*a_sb + h*a_sh + i*N + j (any element offsets: no alignment requirement); out: contiguous fp32
 * [B,N,N] -- e.g. one layer's slice of the [L,B,N,N] stack te_rollout_f32 reads -- or, with TE_HEADMEAN_ROW0, [B,N] =
 * query row 0 alone (the same values bit for bit).  Fixed order, no atomics: a batch equals its samples.
 * B <= 65535 (TE_ERR_UNSUPPORTED otherwise); unknown flag bits: TE_ERR_INVALID_ARG. */
enum { TE_HEADMEAN_CLAMP = 1, TE_HEADMEAN_ROW0 = 2 };
int te_attn_headmean_bf16(const te_bf16_t* attn, int64_t a_sb, int64_t a_sh, float* out, int64_t B, int64_t H, int64_t N,
                          int flags, te_stream_t stream);
/* te_perturb_f32 with a bf16 result (the input of a bf16 classifier): vis and data stay fp32, every value is evaluated
 * in fp32 exactly as te_perturb_f32 does and rounded once to bf16, to nearest even.  Same workspace, same limits. */
int te_perturb_bf16(const float* vis, const float* data, te_bf16_t* out, int64_t B, int64_t C, int64_t HW,
                    const int64_t* ks, int64_t n_steps, const float* mean, const float* std_, void* ws,
                    size_t ws_bytes, te_stream_t stream);
/* The attention producers (te_attention_forward_strided_f32 / te_attention_backward_strided_f32) of a bf16 model: the same
 * argument order with te_bf16_t operands and outputs, head dim 64, 1 <= N <= 640 (te_attention_bf16_supported;
 * TE_ERR_UNSUPPORTED otherwise, and for views whose base is not 16-byte aligned or whose strides are not multiples of 8
 * elements).  csrc/te_attn_bf16.hip.  Every output is rounded to bf16 exactly once, from an fp32 value, where the stock bf16
 * path rounds, so that a rule's Z is the product of the very operands the cache holds:
 *   forward : z_qk (optional) = bf16(q k^T) ; x_scaled (optional) = bf16(z_qk * scale) from the rounded z_qk, WITHOUT the mask
 *             (BERT's Add.X[0]) ; attn = bf16(softmax(s)), evaluated in fp32, s = bf16(x_scaled + mask[b, key]) (mask [B,N]
 *             bf16 additive, NULL = none: s = x_scaled) ; out = bf16(attn v) from the rounded attn, fp32 accumulation
 *   backward: d_attn = bf16(d_out v^T) ; d_v = bf16(attn^T d_out) ; need_qk: d_s = bf16(attn (d_attn - rowsum(attn d_attn)))
 *             from the rounded d_attn (the sums are taken over the N x N tensors, not from d_out . out),
 *             d_q = bf16(scale d_s k), d_k = bf16(scale d_s^T q).  need_qk == 0: d_q / d_k are not written, q / k / the
 *             workspace may be NULL.  Workspace (need_qk): te_attention_backward_strided_bf16_workspace_bytes, B*H*N floats.
 * A launch that the runtime refuses is reported as TE_ERR_UNSUPPORTED, not as a hipError_t. */
int te_attention_bf16_supported(int64_t N, int64_t D);
size_t te_attention_backward_strided_bf16_workspace_bytes(int64_t B, int64_t H, int64_t N);
int te_attention_forward_strided_bf16(const te_bf16_t* q, int64_t q_sb, int64_t q_sh, int64_t q_sn,
                                      const te_bf16_t* k, int64_t k_sb, int64_t k_sh, int64_t k_sn,
                                      const te_bf16_t* v, int64_t v_sb, int64_t v_sh, int64_t v_sn,
                                      const te_bf16_t* mask, te_bf16_t* z_qk, te_bf16_t* x_scaled, te_bf16_t* attn,
                                      te_bf16_t* out, int64_t o_sb, int64_t o_sh, int64_t o_sn,
                                      int64_t B, int64_t H, int64_t N, int64_t D, float scale, te_stream_t stream);
int te_attention_backward_strided_bf16(const te_bf16_t* d_out, int64_t do_sb, int64_t do_sh, int64_t do_sn,
                                       const te_bf16_t* q, int64_t q_sb, int64_t q_sh, int64_t q_sn,
                                       const te_bf16_t* k, int64_t k_sb, int64_t k_sh, int64_t k_sn,
                                       const te_bf16_t* v, int64_t v_sb, int64_t v_sh, int64_t v_sn,
                                       const te_bf16_t* attn, te_bf16_t* d_attn,
                                       te_bf16_t* d_q, int64_t dq_sb, int64_t dq_sh, int64_t dq_sn,
                                       te_bf16_t* d_k, int64_t dk_sb, int64_t dk_sh, int64_t dk_sn,
                                       te_bf16_t* d_v, int64_t dv_sb, int64_t dv_sh, int64_t dv_sn,
                                       int64_t B, int64_t H, int64_t N, int64_t D, float scale, int need_qk,
                                       void* ws, size_t ws_bytes, te_stream_t stream);
/* Conv2d.relprop, z^B rule, of a bf16 patch embedding (method="full" on a bf16 ViT; csrc/te_conv_bf16.hip): the rule of
 * te_conv2d_zb_relprop_f32 evaluated in fp32 on the bf16 X [B,C,H,W] and W [E,C,p,p], fp32 R (token-major [B,P,E],
 * samples r_bs >= P*E floats apart, any 4-byte alignment: cam[:, 1:] is consumed in place) and fp32 out [B,C,H,W].
 *   Za = conv(X,W) - l_b sum_k W+[e,k] - h_b sum_k W-[e,k] + 1e-9 ; S = R / Za ; out = X convT(S,W) - l_b convT(S,W+) - h_b convT(S,W-)
 * conv(X,W) is RECOMPUTED from the bf16 operands on bf16 MFMAs with fp32 accumulation (every product exact): the layer's
 * cached bf16 output and its bias are not arguments.  S enters the second product as three bf16 planes (its exact split).
 * w_planes = te_conv2d_zb_bf16_prepare_weights of W: W+^T, W-^T [K = C p p][E] and the two channel sums (fp64-accumulated),
 * te_conv2d_zb_bf16_weight_planes_bytes bytes, built once per weight version.  X, W, w_planes and ws 16-byte aligned
 * (TE_ERR_INVALID_ARG / TE_ERR_WORKSPACE otherwise).  Shapes: te_conv2d_zb_relprop_bf16_supported -- C == 3, E and K = 3 p p
 * multiples of 128 (p a multiple of 16) -- with H % p == W % p == 0; TE_ERR_UNSUPPORTED otherwise (callers then run
 * te_conv2d_zb_relprop_f32 on exact fp32 copies with Y = their fp32 convolution).  Fixed k-order: a batch equals its samples. */
int te_conv2d_zb_relprop_bf16_supported(int64_t C, int64_t E, int64_t p);
size_t te_conv2d_zb_relprop_bf16_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W, int64_t E, int64_t p);
size_t te_conv2d_zb_bf16_weight_planes_bytes(int64_t C, int64_t E, int64_t p);
int te_conv2d_zb_bf16_prepare_weights(const te_bf16_t* W, int64_t C, int64_t E, int64_t p, void* planes,
                                      size_t planes_bytes, te_stream_t stream);
int te_conv2d_zb_relprop_bf16(const float* R, int64_t r_bs, const te_bf16_t* X, const te_bf16_t* W, const void* w_planes,
                              float* out, int64_t B, int64_t C, int64_t H, int64_t W_, int64_t E, int64_t p, void* ws,
                              size_t ws_bytes, te_stream_t stream);

/* ---- fp64 operands (an fp64 ViT / DeiT or BERT model: model.double()) ------------------------------------------------
 * The rules of variant "ours", alpha = 1, evaluated in DOUBLE on the model's own fp64 tensors: operands, relevance,
 * safe_divide, per-sample sums, factors and outputs are all fp64; nothing is routed through an fp32 or bf16 kernel.
 * csrc/te_f64.hip: the GEMM-shaped rules on v_mfma_f64_16x16x4_f64 (one loop, any M, N, K >= 1, every operand a strided
 * view read in place: no shape predicate and no other route), the streaming rules as plain fp64 kernels.  No pointer needs
 * more than the 8-byte alignment of a double.  Every output's summation order is fixed by its own indices: a batch equals
 * its samples bit for bit, and a call repeated gives the same bits.
 *
 * Linear.relprop: R [T,out_f] (row stride r_ld), X [T,in_f] (row stride x_ld: the cls rows of a [B,N,C] activation are read
 * in place), W [out_f,in_f] (row stride w_ld) -> out [T,in_f] contiguous.
 *   Z = X+ W+^T + X- W-^T (both operands sign-split in registers: no weight planes, nothing cached; the layer's forward
 *   output is not an argument) ; S = sd(R, Z) as fp64 [T,out_f] in ws ; out = X+ . (S W+) + X- . (S W-) */
size_t te_linear_relprop_f64_workspace_bytes(int64_t T, int64_t in_f, int64_t out_f);
int te_linear_relprop_f64(const double* R, int64_t r_ld, const double* X, int64_t x_ld, const double* W, int64_t w_ld,
                          double* out, int64_t T, int64_t in_f, int64_t out_f, void* ws, size_t ws_bytes,
                          te_stream_t stream);
/* The two attention rules: the arguments of te_matmul_relprop_av_f32 / te_matmul_relprop_qk_f32 without a
 * variant and a relevance factor.  Z (the product whose rule is evaluated: attn v [B,H,N,D] strided, the UNSCALED q k^T
 * [B,H,N,N] contiguous) is always an operand.  attn, R (QK) and cam_attn contiguous; R (AV), q, k, v and the cam_q / cam_k /
 * cam_v outputs strided with a contiguous last dim.  S = sd(R, Z) in ws;
 *   cam_attn = attn . (S v^T), cam_v = v . (attn^T S), cam_q = q . (S k), cam_k = k . (S^T q), each times out_scale. */
size_t te_matmul_relprop_av_f64_workspace_bytes(int64_t B, int64_t H, int64_t N, int64_t D);
size_t te_matmul_relprop_qk_f64_workspace_bytes(int64_t B, int64_t H, int64_t N, int64_t D);
int te_matmul_relprop_av_f64(const double* R, int64_t r_sb, int64_t r_sh, int64_t r_sn, const double* attn,
                             const double* v, int64_t v_sb, int64_t v_sh, int64_t v_sn,
                             const double* Z, int64_t z_sb, int64_t z_sh, int64_t z_sn,
                             double* cam_attn, double* cam_v, int64_t cv_sb, int64_t cv_sh, int64_t cv_sn,
                             int64_t B, int64_t H, int64_t N, int64_t D, double out_scale,
                             void* ws, size_t ws_bytes, te_stream_t stream);
int te_matmul_relprop_qk_f64(const double* R, const double* q, int64_t q_sb, int64_t q_sh, int64_t q_sn,
                             const double* k, int64_t k_sb, int64_t k_sh, int64_t k_sn, const double* Z,
                             double* cam_q, int64_t cq_sb, int64_t cq_sh, int64_t cq_sn,
                             double* cam_k, int64_t ck_sb, int64_t ck_sh, int64_t ck_sn,
                             int64_t B, int64_t H, int64_t N, int64_t D, double out_scale,
                             void* ws, size_t ws_bytes, te_stream_t stream);
/* Add.relprop, variant ours (te_add_relprop_f32's arguments): the three per-sample sums in fp64, 2048 consecutive elements
 * per workgroup in a fixed tree, the workgroups' sums added in index order.  te_add_bcast_relprop_f64: the BERT mask form,
 * X0 [B,H,N,N], mask [B,N] mask_batch_stride elements apart (0: one mask for every sample), out1 [B,N]. */
size_t te_add_relprop_f64_workspace_bytes(int64_t B, int64_t n);
int te_add_relprop_f64(const double* R, const double* X0, const double* X1, double* out0, double* out1, int64_t B,
                       int64_t n, int64_t x1_batch_stride, void* ws, size_t ws_bytes, te_stream_t stream);
size_t te_add_bcast_relprop_f64_workspace_bytes(int64_t B, int64_t H, int64_t N);
int te_add_bcast_relprop_f64(const double* R, const double* X0, const double* mask, int64_t mask_batch_stride,
                             double* out0, double* out1, int64_t B, int64_t H, int64_t N, void* ws, size_t ws_bytes,
                             te_stream_t stream);
/* Clone (R2 may be NULL), IndexSelect (dim 1, one index) and the gradient x relevance head mean, as their _f32 entries. */
int te_clone_relprop_f64(const double* R0, const double* R1, const double* R2, const double* X, double* out, int64_t n,
                         te_stream_t stream);
int te_index_select_relprop_f64(const double* R, const double* X, double* out, int64_t B, int64_t N, int64_t C,
                                int64_t index, te_stream_t stream);
int te_gradcam_headmean_f64(const double* grad, const double* cam, double* out, int64_t B, int64_t H, int64_t N,
                            te_stream_t stream);

/* ---- head_mask (csrc/te_headmask.hip) ---------------------------------------------------------------------------------
 * Mul.relprop of BertSelfAttention for the operands [attention_probs, head_mask] (BERT.py:375-377; Mul is RelPropSimple,
 * BERT_explainability/modules/layers_ours.py:49-61,77-79); the mask operand's relevance is discarded, as the reference does.
 *   R, out [B,H,rows,cols] contiguous, in the relevance type; P [B,H,rows,cols] contiguous, in the operand type; the mask value
 *   of plane (b, h) is m[b * m_sb + h] in the operand type, m_sb = 0: one mask for the whole batch (else m_sb >= H).
 *     Z = P m ; S = sd(R, Z) ; out = P (S m)              every operation rounded on its own, in this order
 *   _f32: all fp32.  _bf16: P and m bf16, read exactly, Z = float(P) float(m) (exact in fp32), R and out fp32.  _f64: all fp64.
 *   out == R is allowed (each element is read before it is written).  A plane whose m is exactly 0 is written as zeros; its R and
 *   P are not read.  One streaming pass without sums or atomics: 16-byte accesses from the first 16-byte boundary of `out`
 *   inside each plane, single elements in front of it and at the tail; pointers need their element's alignment only.  The grid
 *   is flat (B*H may exceed 65535); a batch equals its samples by construction.
 *   TE_ERR_INVALID_ARG: a null pointer, a size <= 0, 0 < m_sb < H. */
int te_mul_head_relprop_f32(const float* R, const float* P, const float* m, int64_t m_sb, float* out, int64_t B, int64_t H,
                            int64_t rows, int64_t cols, te_stream_t stream);
int te_mul_head_relprop_bf16(const float* R, const te_bf16_t* P, const te_bf16_t* m, int64_t m_sb, float* out, int64_t B,
                             int64_t H, int64_t rows, int64_t cols, te_stream_t stream);
int te_mul_head_relprop_f64(const double* R, const double* P, const double* m, int64_t m_sb, double* out, int64_t B, int64_t H,
                            int64_t rows, int64_t cols, te_stream_t stream);
/* Per-head relevance (Voita et al. 2019): out[b][h] = sum over n, d of R[b][h][n][d], R a strided [B,H,N,D] view with a
 * contiguous last dimension (the 'b n (h d)' relevance entering an attention layer is read in place), out [B,H] fp64.
 * One workgroup per (b, h); every addend enters an fp64 accumulator, and the order of the additions is fixed by the indices
 * alone (spans of 4 per thread in index order, a shuffle tree, the waves in order; no atomics): a call repeated gives the same
 * bits and a batch equals its samples.  TE_ERR_INVALID_ARG: a null pointer, a size <= 0, a negative stride, r_sn < D. */
int te_head_relevance_f32(const float* R, int64_t r_sb, int64_t r_sh, int64_t r_sn, double* out, int64_t B, int64_t H,
                          int64_t N, int64_t D, te_stream_t stream);
int te_head_relevance_f64(const double* R, int64_t r_sb, int64_t r_sh, int64_t r_sn, double* out, int64_t B, int64_t H,
                          int64_t N, int64_t D, te_stream_t stream);

/* ---- class targets (csrc/te_classes.hip) ------------------------------------------------------------------------------
 * The classes a batch is explained for, on the device: per sample K classes, their logits, and the K one-hot relevance rows
 * that seed the relprop chains (LRP.generate_classes / Generator.generate_classes).  One kernel, one workgroup per sample; no
 * allocation, no synchronisation, no memset node (graph-capturable), nothing read back by the host.
 *   logits      [B] rows of C values, row b at logits + b * ld (ld >= C, in elements); any element alignment (bf16 rows may
 *               start at an odd element).  _f32 / _bf16 / _f64: the logits' type; the relevance type of scores and seeds is
 *               float, float, double.
 *   classes_in  NULL: the K largest logits of each row, in descending order, equal values in ascending class index, -0 == +0,
 *               NaN largest (the order of te_key; an 8-bit radix select, then a rank sort of the K candidates in LDS).
 *               1 <= K <= min(C, TE_CLASS_TARGETS_MAX_TOPK).
 *               else [B,K] int64 on the device: these classes, in this order, duplicates allowed.  A class outside [0, C) is
 *               never used as an address: its classes_out is -1, its score NaN, its seed row all zero.
 *   classes_out [B,K] int64; scores [B,K]: the logit of that class, upcast exactly (no arithmetic).
 *   seeds       [K,B,C] (class k's seed is one contiguous [B,C]) or NULL (not written): 1 at the class, 0 elsewhere, every
 *               element written once with 16-byte vector stores between the row's first 16-byte boundary and its last whole vector.
 *   The buffers must not overlap.  Limits: C <= TE_CLASS_TARGETS_MAX_CLASSES (2^20), K <= 2^20, top-K K <=
 *   TE_CLASS_TARGETS_MAX_TOPK (1024): TE_ERR_UNSUPPORTED beyond.  TE_ERR_INVALID_ARG: a null logits / classes_out / scores, a
 *   size <= 0, ld < C, top-K K > C. */
#define TE_CLASS_TARGETS_MAX_CLASSES (1 << 20)
#define TE_CLASS_TARGETS_MAX_TOPK 1024
int te_class_targets_f32(const float* logits, int64_t ld, int64_t B, int64_t C, int64_t K, const int64_t* classes_in,
                         int64_t* classes_out, float* scores, float* seeds, te_stream_t stream);
int te_class_targets_bf16(const te_bf16_t* logits, int64_t ld, int64_t B, int64_t C, int64_t K, const int64_t* classes_in,
                          int64_t* classes_out, float* scores, float* seeds, te_stream_t stream);
int te_class_targets_f64(const double* logits, int64_t ld, int64_t B, int64_t C, int64_t K, const int64_t* classes_in,
                         int64_t* classes_out, double* scores, double* seeds, te_stream_t stream);

/* ---- AttnLRP (csrc/te_attnlrp.hip) ------------------------------------------------------------------------------------
 * A second explanation method beside the reference's: AttnLRP (Achtibat et al., "AttnLRP: Attention-Aware Layer-Wise
 * Relevance Propagation for Transformers", ICML 2024) for the ViT / DeiT and BERT models of this package, fp32 or bf16
 * (below: "AttnLRP, bf16 operands").  The
 * reference has no such method and no parity with the authors' library (LXT) is claimed: THIS SECTION IS THE SPECIFICATION,
 * and tests/attnlrp_ref.py restates it with torch autograd.
 *
 * The chain carries G, relevance per unit of activation: the relevance of an activation a is a (.) G_a.  Write
 *     stab(y) = y + eps sgn(y), sgn(+-0) = +1          damp(G, y) = G y / stab(y)
 * eps >= 0 is an argument (default 1e-6); eps = 0 means damp(G, y) = G, for every y.
 *   Seed       G_logits = the one-hot of the class.
 *   Linear     y = x W^T + b:  G_x = damp(G_y, y) W, y the cached output WITH the bias -- the bias absorbs its share.  The
 *              product is te_gemm_x6_f32 on the planes of W^T wherever te_gemm_x6_supported, the stock fp32 GEMM elsewhere.
 *   Add        o = a + b (residual):  G_a = G_b = damp(G_o, o).  Two paths that meet at one tensor add their G (plain).
 *   LayerNorm  y = gamma (x - mu) rstd + beta with rstd held constant:  G_x[i] = rstd (gamma_i G_y[i] - mean_j(gamma_j G_y[j])),
 *              rstd = 1 / sqrt(var + the layer's own eps).  No damping; beta absorbs its share.
 *   GELU, tanh y = f(x):  G_x = G_y (f(x) / x), the factor f'(0) at x == +-0 (0.5 / 1).  f = te_gelu (te_gelu_forward_f32's
 *              bits) / tanhf; one IEEE division, one multiply, no contraction.
 *   Attention  s = scale q k^T (+ mask), p = softmax(s), o = p v: each operand of a product takes half (uniform rule), softmax
 *              is plain gradient, the additive mask is a constant and absorbs nothing, no damping.  With d_* the gradients
 *              of the block for d_out = G_o:  G_v = d_v / 2, G_q = d_q / 4, G_k = d_k / 4 (G_p = d_attn / 2) -- the existing
 *              backward (te_attention_backward_strided_f32 where te_attention_strided_supported) and exact scalings.
 *   Others     class-token select, position-embedding Add (a parameter), dropout in eval mode: plain gradient.
 *   Result     ViT / DeiT: R[b][t] = sum_c x0[b][t][c] G[b][t][c] over the patch tokens, x0 the patch embedding (with the class
 *              token in front) BEFORE the position embedding is added, the class token dropped: fp32 [B, N - 1].  BERT: x0 the
 *              input of the embedding LayerNorm (word + position + type): fp32 [B, N].
 *   Relevance is absorbed by: biases (Linear, LayerNorm beta), eps, the mean subtraction of LayerNorm, softmax, the additive
 *   mask, the position embedding.  With all of them absent the chain conserves sum_t R = logit_c.
 *
 * The entries: contiguous fp32 tensors, pointers 4-byte aligned (TE_ERR_UNSUPPORTED otherwise); 16-byte accesses where the
 * alignment allows, single elements elsewhere, and the same bits either way; no atomics, no workspace; every refusal comes
 * before the launch.  TE_ERR_INVALID_ARG: a null pointer, a size <= 0, and what each entry names.
 *   te_alrp_damp_f32            out[i] = (G[i] Y[i]) / stab(Y[i]): one multiply, one add, one IEEE division; eps == 0: out = G.
 *                               out == G is allowed.  Vectors where G, Y and out share one 16-byte phase, from the first
 *                               boundary on.  TE_ERR_INVALID_ARG: eps negative, NaN or infinite.
 *   te_alrp_act_f32             out[i] = G[i] r, r = f(x[i]) / x[i] or f'(0); kind TE_ALRP_ACT_GELU / TE_ALRP_ACT_TANH (another
 *                               kind: TE_ERR_INVALID_ARG).  out == G is allowed.  Vectors as in te_alrp_damp_f32.
 *   te_alrp_scale3_f32          in place: rows t < T of C elements at q + t ld, k + t ld, v + t ld are multiplied by 1/4, 1/4,
 *                               1/2 (exact).  A fused [T, 3C] gradient: q = g, k = g + C, v = g + 2C, ld = 3C; BERT's three
 *                               tensors: ld = C.  The three row sets must not overlap.  TE_ERR_INVALID_ARG: ld < C.
 *   te_alrp_row_rstd_f32        rstd[r] = 1 / sqrt(var_r + eps), var_r the biased variance of row r of x [rows, C], two passes
 *                               (mean, then the squared distances), each an fp32 row sum in the lane order below, each
 *                               divided by C once; IEEE sqrt and division.  Any C >= 1.
 *   te_alrp_layernorm_f32       out[r][i] = rstd[r] (t_i - m), t_i = gamma[i] G[r][i] rounded, m = (fp32 row sum of t) / C.
 *                               One row per wave.  LANE ORDER of the row sum: lane l adds t of the groups l, l + 64, ... (a
 *                               group: elements 4g .. 4g + 3, in index order) to an accumulator that starts at +0; then the
 *                               shuffle-down tree, offsets 32, 16, .. 1: lane j adds lane j + offset's value; lane 0 holds the
 *                               sum.  A row's result does not depend on its position or on its neighbours: a row alone
 *                               equals the same row in a batch.  out == G is allowed.  Any C >= 1.
 *   te_alrp_token_relevance_f32 out[b][t - skip_first] = sum_c x0[b][t][c] G[b][t][c] for skip_first <= t < N; x0, G [B,N,C], out
 *                               [B, N - skip_first].  The products are exact in fp64; thread i of the token's 64 adds the groups
 *                               i, i + 64, ... of four elements in index order in fp64, then te_block_sum's order; one rounding
 *                               to fp32.  TE_ERR_INVALID_ARG: skip_first not 0 or 1, N - skip_first == 0. */
enum { TE_ALRP_ACT_GELU = 0, TE_ALRP_ACT_TANH = 1 };
int te_alrp_damp_f32(const float* G, const float* Y, float* out, int64_t n, float eps, te_stream_t stream);
int te_alrp_act_f32(const float* G, const float* x, float* out, int64_t n, int kind, te_stream_t stream);
int te_alrp_scale3_f32(float* q, float* k, float* v, int64_t ld, int64_t T, int64_t C, te_stream_t stream);
int te_alrp_row_rstd_f32(const float* x, float* rstd, int64_t rows, int64_t C, float eps, te_stream_t stream);
int te_alrp_layernorm_f32(const float* G, const float* gamma, const float* rstd, float* out, int64_t rows, int64_t C,
                          te_stream_t stream);
int te_alrp_token_relevance_f32(const float* x0, const float* G, float* out, int64_t B, int64_t N, int64_t C, int skip_first,
                                te_stream_t stream);

/* ---- AttnLRP, bf16 operands (a bf16 model: model.to(torch.bfloat16); csrc/te_attnlrp.hip, csrc/te_bf16.hip) ---------------
 * The rules above, evaluated in fp32 on the model's own bf16 tensors, which are read exactly (bf16 -> fp32 is exact): the
 * contract of "bf16 operands" above.  G (relevance per unit of activation), the seed, rstd and the result are fp32; the token
 * sums are fp64, rounded once.  Nothing of G is ever rounded to bf16, and no cached bf16 tensor is replaced by a recomputation.
 * The bf16 operands of a rule are the cached tensors the fp32 chain reads: the outputs of Linears and Adds, the inputs of
 * LayerNorms, GELU and tanh, qkv.Y (BERT: query.Y, key.Y, value.Y), the probabilities the accessor holds, gamma, W and x0.
 *
 * Streaming rules: te_attnlrp_damp_bf16, _act_bf16, _row_rstd_bf16, _layernorm_bf16, _token_relevance_bf16 are the _f32 kernels
 * templated on the operand type.  SPECIFICATION: each gives the bits of its _f32 entry on an exact fp32 copy of the bf16
 * operand -- the same operations, the same lane order, the same te_block_sum order.  A bf16 pointer needs 2-byte alignment
 * (TE_ERR_UNSUPPORTED otherwise); a group of four bf16 is read in one 8-byte access where the fp32 operands allow their
 * 16-byte one and the group lies on an 8-byte boundary, single elements elsewhere, and the bits are the same either way.  The
 * refusals are those of the _f32 entries.  te_alrp_scale3_f32 works on G and has no bf16 form.
 *
 * Linear: out[t][i] = sum_o A[t][o] W[o][i], A = damp(G, Y) with te_attnlrp_damp_bf16's bits.  G [T, g_ld >= out_f] fp32 and Y
 * [T, y_ld >= out_f] bf16 are read in place (row strides); W bf16 contiguous; out [T, in_f] fp32 contiguous.  A
 * streaming pass writes A as three exact bf16 planes [3][T][out_f] (the split of csrc/te_x6.h, the layout of the S planes of
 * te_linear_relprop_bf16) into the workspace; the product is then planes x ONE bf16 operand -- three plane-products, every
 * bf16 x bf16 product exact in the fp32 accumulator.  THE WEIGHT SIDE: w_transposed == 0: W [out_f, in_f] itself, read in place
 * as the transposed view (row i of the operand = column i of W, staged through a transposing store); w_transposed != 0: W points
 * to a contiguous copy of W^T [in_f, out_f] that the caller keeps (ops.alrp_weight_t: cached per weight version), read along k.
 * The products and their order are the same: the same bits either way.
 * ACCUMULATION ORDER: one fp32 accumulator per output, which starts at +0; K steps of 32 in index order; inside a K step plane
 * 2, then plane 1, then plane 0 (smallest first), each adding its 32 exact products by one v_mfma_f32_16x16x32_bf16.  The
 * order does not depend on T or on the grid: a row alone equals the same row in a batch bit for bit.  Tiles are 128 rows x 64
 * columns x 32.  Shapes: te_attnlrp_linear_bf16_supported -- in_f and out_f multiples of 128, any T >= 1 (TE_ERR_UNSUPPORTED
 * otherwise).  TE_ERR_INVALID_ARG: a null pointer, a size <= 0, g_ld or y_ld < out_f, eps negative, NaN or infinite;
 * TE_ERR_WORKSPACE: ws NULL or smaller than te_attnlrp_linear_bf16_workspace_bytes.
 *
 * Attention: the block's backward for d_out = G_o in fp32 on the exact bf16 operands.  G_o fp32, element (b, h, n, d) at
 * g_sb b + g_sh h + g_sn n + d (a [B,N,C] tensor: sb = N C, sh = D, sn = C); q, k, v bf16 and the fp32 outputs G_q, G_k, G_v with
 * strides of the same meaning, so the thirds of a fused [B,N,3C] activation (and of a fused gradient) and BERT's three tensors
 * are read (written) in place; attn bf16 [B,H,N,N] contiguous.  The additive mask is a constant and no argument.
 *     d_attn = G_o v^T, d_v = attn^T G_o                    (G_o as three planes, one streaming pass)
 *     d_s = p (.) (d_attn - s), s_i = sum_j t_ij, t_ij = d_attn[i][j] p[i][j] rounded; d_s written as three planes
 *     d_q = scale (d_s k), d_k = scale (d_s^T q)            (one multiply by scale in the epilogue)
 * G_q = d_q, G_k = d_k, G_v = d_v: the uniform rule's exact factors 1/4, 1/4, 1/2 are NOT applied here -- the caller runs
 * te_alrp_scale3_f32 on the outputs afterwards, as the fp32 chain does.  The row sum s_i is the fp32 row sum in the LANE ORDER
 * of te_alrp_layernorm_f32, fixed by the indices alone.  The four products are planes x one bf16 operand on 64 x 64 x 32 tiles:
 * one accumulator per plane, plain k loop, summed (plane 2 + plane 1) + plane 0 at the end -- the arrangement of
 * te_matmul_relprop_av_bf16 / _qk_bf16.  A (b, h) alone equals the same pair in a batch bit for bit.  N == 1: G_v = G_o and
 * G_q = G_k = 0 exactly.  Shapes: te_attnlrp_attention_bf16_supported where te_matmul_relprop_bf16_supported (head dim 64,
 * N <= 1024), B H <= 65535; TE_ERR_UNSUPPORTED otherwise. */
int te_attnlrp_damp_bf16(const float* G, const te_bf16_t* Y, float* out, int64_t n, float eps, te_stream_t stream);
int te_attnlrp_act_bf16(const float* G, const te_bf16_t* x, float* out, int64_t n, int kind, te_stream_t stream);
int te_attnlrp_row_rstd_bf16(const te_bf16_t* x, float* rstd, int64_t rows, int64_t C, float eps, te_stream_t stream);
int te_attnlrp_layernorm_bf16(const float* G, const te_bf16_t* gamma, const float* rstd, float* out, int64_t rows, int64_t C,
                           te_stream_t stream);
int te_attnlrp_token_relevance_bf16(const te_bf16_t* x0, const float* G, float* out, int64_t B, int64_t N, int64_t C,
                                 int skip_first, te_stream_t stream);
int te_attnlrp_linear_bf16_supported(int64_t T, int64_t in_f, int64_t out_f);
size_t te_attnlrp_linear_bf16_workspace_bytes(int64_t T, int64_t in_f, int64_t out_f);
int te_attnlrp_linear_bf16(const float* G, int64_t g_ld, const te_bf16_t* Y, int64_t y_ld, const te_bf16_t* W,
                        int w_transposed, float* out, int64_t T, int64_t in_f, int64_t out_f, float eps, void* ws, size_t ws_bytes, te_stream_t stream);
int te_attnlrp_attention_bf16_supported(int64_t N, int64_t D);
size_t te_attnlrp_attention_bf16_workspace_bytes(int64_t B, int64_t H, int64_t N, int64_t D);
int te_attnlrp_attention_bf16(const float* G_o, int64_t g_sb, int64_t g_sh, int64_t g_sn,
                           const te_bf16_t* q, int64_t q_sb, int64_t q_sh, int64_t q_sn,
                           const te_bf16_t* k, int64_t k_sb, int64_t k_sh, int64_t k_sn,
                           const te_bf16_t* v, int64_t v_sb, int64_t v_sh, int64_t v_sn,
                           const te_bf16_t* attn, float scale,
                           float* G_q, int64_t gq_sb, int64_t gq_sh, int64_t gq_sn,
                           float* G_k, int64_t gk_sb, int64_t gk_sh, int64_t gk_sn,
                           float* G_v, int64_t gv_sb, int64_t gv_sh, int64_t gv_sn,
                           int64_t B, int64_t H, int64_t N, int64_t D, void* ws, size_t ws_bytes, te_stream_t stream);

/* ---- AttnLRP, pixel level (csrc/te_attnlrp_patch.hip) -------------------------------------------------------------------
 * The last step of the chain on a ViT / DeiT: the eps-rule through the patch-embedding convolution, then input x G per pixel
 * -- an fp32 [B, H, W] map, the shape of the z^B rule's (te_conv2d_zb_relprop_f32).  The convolution has stride == kernel and
 * no padding, so it is a Linear layer on non-overlapping patches.  Notation: X [B,C,H,W] the image, W [E,C,p,p] the weight
 * (W.view(E, C p p) is the row-major operand: no transposed copy), P = (H/p)(W_/p) patches per sample; y[b,t,e] the cached
 * output of the convolution WITH its bias = the patch rows of x0 (the patch embedding before the position embedding is
 * added), token-major; G[b,t,e] the chain's G at x0 (the position-embedding Add is plain).  Token t = hp (W_/p) + wp covers
 * the pixels (hp p + i, wp p + j).
 *     A[b,t,e]               = damp(G[b,t,e], y[b,t,e])     te_alrp_damp_f32's bits; eps == 0: A = G
 *     acc_c[b,t,i,j]         = the fp32 fma chain over e = 0 .. E-1 ASCENDING of A[b,t,e] W[e,c,i,j], from +0
 *     out[b, hp p+i, wp p+j] = fp32( sum_c (double)X[b,c,h,w] (double)acc_c ): c ascending from +0.0, every product exact in
 *                              fp64, every add rounded in fp64, one rounding to fp32
 * The bias absorbs its share, as in the Linear rule; nothing else is damped; there is no mean or zero-point term: this is
 * eps-LRP, input x G in the normalised input space.  Conservation: with a zero bias and eps = 0 the sum of out over the pixels
 * of patch t equals the token relevance sum_e x0[b,t,e] G[b,t,e] (both are sum_e A_e (y_e - b_e)).
 * An fp32-input MFMA is exactly the k-ordered chain, so the result depends on no tiling decision: the tiled kernel, the
 * one-thread-per-pixel kernel, a sample alone and the same sample in a batch give the same bits.  No split along e, no
 * atomics, no workspace.
 *   G, Y      point at the first PATCH row (a caller that holds [B, P+1, E] tensors adds E to skip the class token); g_bs, y_bs
 *             >= P E are the batch strides in elements.  G and out are fp32; Y, X, W are fp32 (_f32) or bf16 read exactly
 *             (_bf16: the _f32 entry's bits on exact fp32 copies, the convention of "AttnLRP, bf16 operands").
 *   Kernels   te_patch_alrp_relevance_supported(C, E, p) == 1: the tiled kernel (fp32 MFMA 32x32x2; a workgroup owns 64 tokens x
 *             64 pixel columns (i, j) of every channel, stages G and y through LDS and damps while staging, walks e in chunks
 *             of 32 once per channel -- G and y are read and damped again on every channel's walk, C times in all -- and folds
 *             X acc into fp64 pixel sums, c ascending) -- E a multiple of 32, p a multiple of 8,
 *             any C >= 1, any B, H, W_.  Otherwise, and with flags = TE_IMPL_SIMPLE, one thread per pixel with literal fmaf
 *             chains: any C, E, p >= 1.
 *   Alignment pointers on their element's boundary (4 bytes; bf16: 2), TE_ERR_UNSUPPORTED otherwise.  The tiled kernel stages
 *             G, Y and W in groups of four elements (16 bytes; bf16: 8) where G, Y, W lie on that boundary and g_bs, y_bs are
 *             multiples of 4, single elements elsewhere: the same bits either way.
 *   TE_ERR_INVALID_ARG: a null pointer, a size <= 0, H or W_ not a multiple of p, g_bs or y_bs < P E, eps negative, NaN or
 *             infinite, unknown flag bits.  TE_ERR_UNSUPPORTED: sizes beyond 2^31 - 1 (B P, H W_, C p p, P E).  Every refusal
 *             comes before the launch. */
int te_patch_alrp_relevance_supported(int64_t C, int64_t E, int64_t p);
int te_patch_alrp_relevance_f32(const float* G, int64_t g_bs, const float* Y, int64_t y_bs, const float* X, const float* W,
                                float* out, int64_t B, int64_t C, int64_t H, int64_t W_, int64_t E, int64_t p, float eps,
                                int flags, te_stream_t stream);
int te_patch_attnlrp_relevance_bf16(const float* G, int64_t g_bs, const te_bf16_t* Y, int64_t y_bs, const te_bf16_t* X,
                                    const te_bf16_t* W, float* out, int64_t B, int64_t C, int64_t H, int64_t W_, int64_t E,
                                    int64_t p, float eps, int flags, te_stream_t stream);

/* ---- AttnLRP, a class axis (csrc/te_attnlrp.hip) ------------------------------------------------------------------------
 * The chain is linear in the seed: every rule is G_in = (something of the cached activations) . G_out, and the cached
 * operands do not depend on the class.  K classes of the same inputs therefore share ONE forward pass and one read of every
 * cached operand: G carries a leading class axis.
 *   G and out are [K, *shape], class-major and contiguous; the cached operand of a rule has `shape` and is shared by the K
 *   slices.  SPECIFICATION: for every k, slice k of a rule's output has the bits of the entry without a class axis (above)
 *   on (G[k], operand) -- the same operations in the same order per element, the same lane order per row, the same fp64
 *   order per token.  K = 1 is that entry, bit for bit.
 * Because te_gemm_x6_f32 and the row / token kernels give a row the same bits alone and in a batch, the map of class k from
 * a chain with a class axis has the bits of the chain of that class alone wherever "a batch equals its samples" holds for
 * the single chain: every product on this library's kernels, and one-hot seeds at a stock head product.  Not covered:
 * general seeds where the head's product runs on the stock GEMM (its order may depend on the number of rows), and shapes
 * whose Linear products run on the stock GEMM.
 *   te_alrpk_damp_f32             out[k][i] = (G[k][i] Y[i]) / stab(Y[i]), Y [n]: an item is one 16-byte group of Y (or one
 *                                 element); it loads Y and forms stab(Y) ONCE, then walks k: load G[k], one multiply, one IEEE
 *                                 division, store out[k].  eps == 0: out = G.  out == G is allowed.  Vectors where G, Y and
 *                                 out share one 16-byte phase AND the class stride n is a multiple of 4 (or K == 1); single
 *                                 elements elsewhere; the same bits either way.
 *   te_alrpk_act_f32              out[k][i] = G[k][i] r_i, r_i = f(x[i]) / x[i] or f'(0) formed ONCE per element (the GELU /
 *                                 tanh evaluation and the division); per class one multiply.  Items and vectors as above.
 *   te_alrpk_layernorm_f32        G, out [K, rows, C], gamma [C], rstd [rows] (te_alrp_row_rstd_f32, computed once, not K times):
 *                                 one wave per operand row r, which walks k; per (k, r) the loads, LANE ORDER and shuffle tree
 *                                 of te_alrp_layernorm_f32.  out == G is allowed.
 *   te_alrpk_token_relevance_f32  x0 [B,N,C], G [K,B,N,C] -> out [B, K, N - skip_first]: batch-major, the layout the callers
 *                                 return, so no permuted copy follows.  Per (k, b, t) the fp64 order of
 *                                 te_alrp_token_relevance_f32.
 *   _bf16: the operand (Y, x, gamma, x0) is bf16, read exactly: the _f32 entry's bits on an exact fp32 copy, the convention
 *   of "AttnLRP, bf16 operands".
 * te_alrp_scale3_f32 runs on K T rows and te_alrp_row_rstd_f32 has no class dependence: neither has a class form.  The Linear
 * product is one te_gemm_x6_f32 over the K T rows (bf16: K calls of te_attnlrp_linear_bf16), the attention rule K calls of
 * its entry.
 * Alignment and refusals as for the entries without a class axis, all before the launch.  TE_ERR_INVALID_ARG: a null pointer,
 * K <= 0, a size <= 0, eps negative, NaN or infinite, an unknown kind, skip_first not 0 or 1, N - skip_first == 0.
 * TE_ERR_UNSUPPORTED: a pointer off its element's boundary, sizes beyond the grid limit (2^31 - 1 workgroups; K, C). */
int te_alrpk_damp_f32(const float* G, const float* Y, float* out, int64_t K, int64_t n, float eps, te_stream_t stream);
int te_alrpk_damp_bf16(const float* G, const te_bf16_t* Y, float* out, int64_t K, int64_t n, float eps, te_stream_t stream);
int te_alrpk_act_f32(const float* G, const float* x, float* out, int64_t K, int64_t n, int kind, te_stream_t stream);
int te_alrpk_act_bf16(const float* G, const te_bf16_t* x, float* out, int64_t K, int64_t n, int kind, te_stream_t stream);
int te_alrpk_layernorm_f32(const float* G, const float* gamma, const float* rstd, float* out, int64_t K, int64_t rows,
                           int64_t C, te_stream_t stream);
int te_alrpk_layernorm_bf16(const float* G, const te_bf16_t* gamma, const float* rstd, float* out, int64_t K, int64_t rows,
                            int64_t C, te_stream_t stream);
int te_alrpk_token_relevance_f32(const float* x0, const float* G, float* out, int64_t K, int64_t B, int64_t N, int64_t C,
                                 int skip_first, te_stream_t stream);
int te_alrpk_token_relevance_bf16(const te_bf16_t* x0, const float* G, float* out, int64_t K, int64_t B, int64_t N, int64_t C,
                                  int skip_first, te_stream_t stream);

/* ---- gradient baselines (Input x Gradient: Shrikumar et al., 2016; SmoothGrad: Smilkov et al., 2017; Integrated Gradients:
 * Sundararajan et al., ICML 2017) -- csrc/te_gradients.hip -----------------------------------------------------------------
 * THE REFERENCE TREE HAS NO SUCH METHODS: what follows is this project's definition, restated in numpy / torch by
 * gradients.py.  Parity with captum is not claimed.  The methods are a loop around the model's own forward and backward pass;
 * the entries below are what surrounds the loop: the path or noise copies of a batch, written in the model's dtype, and the
 * reduction of the B S input gradients to B maps.  No entry synchronises, reads back or issues a memset node: a HIP graph
 * captures every call.  There are no atomics: every output of sample b is the same bit pattern alone, in any batch and in any
 * chunking (s0, n_s) / (d0, n_d) of the copies.
 *
 * Path inputs.  x, base [B,n] fp32, n = C H W: the input the model saw, upcast, and the baseline.  alphas [S] fp32, on the
 *   device.  out [B,n_s,n], fp32 or bf16: row b n_s + j is node s0 + j of sample b,
 *       out = round((double)base + (double)alphas[s0 + j] * ((double)x - (double)base)):
 *   one fp64 subtraction, one fp64 multiplication and one fp64 addition (never an FMA), ONE rounding to fp32; _bf16 rounds that
 *   fp32 once more, to nearest even.  Every step is IEEE: numpy's float64 expression followed by astype(float32) gives the same
 *   bits.  alpha = 0 gives base; alpha = 1 gives x wherever x - base is exact in fp64 (exponents less than 2^29 apart).  A
 *   thread owns four consecutive elements, reads x and base once and walks j.
 * Gauss inputs.  x [B,n] fp32, out [B,n_d,n], fp32 or bf16: row b n_d + j is draw d = d0 + j of the sample with the global
 *   64-bit id id0 + b (wrapping), out = round((double)x + sigma * z): one fp64 multiplication, one fp64 addition, ONE rounding
 *   to fp32 (_bf16: once more, to nearest even).  The four elements 4g .. 4g + 3 take the words w0 .. w3 of Philox4x32-10
 *   (the generator of "robustness and complexity") with the counter (0x40000000 | g, d, low32(id), high32(id)) and the key
 *   (low32(seed), high32(seed)): bit 30 of the first counter word keeps this stream apart from the noise stream (first word
 *   below 2^29) and from the subset stream (bit 31).  Box-Muller in fp64, one pair of words per pair of normals:
 *       u1 = (w0 + 0.5) 2^-32, u2 = (w1 + 0.5) 2^-32 (exact, in (0, 1)); r = sqrt(-2 ln u1); t = 6.283185307179586 u2;
 *       z0 = r cos t, z1 = r sin t for the elements 4g, 4g + 1; the same from (w2, w3) for 4g + 2, 4g + 3.
 *   ln, sqrt, cos and sin are the device library's fp64 functions (a few fp64 ulp): a restatement in another libm agrees within
 *   one step of the rounded fp32 (bf16) result, and device results agree with device results bit for bit.  sigma == 0 gives x
 *   exactly (|z| < 6.8).  A sample's copies depend on (element, draw, id, seed, sigma) alone.
 * Accumulate.  g [B,n_s,n] fp32 or bf16: the gradients of the copies s0 .. s0 + n_s - 1.  w [S] fp64, on the device, with
 *   S >= s0 + n_s (the caller's promise: the entry does not know S).
 *   acc [B,n] fp64, zeroed by the caller before the first chunk:  for j = 0 .. n_s - 1 in order
 *       acc[b][i] = acc[b][i] + w[s0 + j] * t,   t = (double)g, or (double)g * (double)g (exact) when square != 0:
 *   one fp64 multiplication and one fp64 addition per step, never an FMA.  The order is fixed by (b, i, s) alone, so any
 *   chunking of S gives the same bits.
 * Finish.  acc [B,C,HW] fp64; m [B,C,HW] fp32 or NULL (then the terms are acc's); out [B,HW] fp32; sums [B] fp64 or NULL.
 *   Per pixel, with the terms t_c = (double)m * acc (one fp64 multiplication) for c = 0 .. C - 1 in order, from +0.0:
 *       TE_GRAD_SUM      v = sum_c t_c            TE_GRAD_ABS_SUM  v = sum_c |t_c|            TE_GRAD_MAX_ABS  v = max_c |t_c|
 *   (a NaN term makes v NaN in every mode).  out = v rounded once to fp32.  sums[b] = sum over the pixels of v in fp64: one
 *   workgroup of 1024 per sample, thread t adds the pixel pairs t, t + 1024, ... in order, then the 64 lanes of a wave and the
 *   16 waves meet in te_block_sum's fixed order -- an order fixed by HW alone.  It is the completeness side of Integrated
 *   Gradients: sum of the map against f(x) - f(base).
 * Alignment: pointers on their element's boundary (fp32 4 bytes, bf16 2, fp64 8), TE_ERR_UNSUPPORTED otherwise.  16-byte
 *   accesses (8-byte for four bf16) where n % 4 == 0 (finish: HW % 2 == 0) and every pointer lies on the boundary of its
 *   access, single elements elsewhere; the values and their order are the same either way.
 * Refused on the host before any HIP call.  TE_ERR_INVALID_ARG: null pointers (all but m and sums), sizes <= 0, s0 < 0,
 *   s0 + n_s > S (path inputs), d0 < 0, d0 + n_d > 2^32, sigma negative, NaN or infinite, an unknown `reduce`.  TE_ERR_UNSUPPORTED: a pointer
 *   off its element's boundary, B > 65535, n, C or HW > 2^31 - 1, n_s or n_d > 2^31 - 1. */
#define TE_GRAD_SUM 0
#define TE_GRAD_ABS_SUM 1
#define TE_GRAD_MAX_ABS 2
int te_path_inputs_f32(const float* x, const float* base, const float* alphas, float* out, int64_t B, int64_t n, int64_t S,
                       int64_t s0, int64_t n_s, te_stream_t stream);
int te_path_inputs_bf16(const float* x, const float* base, const float* alphas, te_bf16_t* out, int64_t B, int64_t n, int64_t S,
                        int64_t s0, int64_t n_s, te_stream_t stream);
int te_gauss_inputs_f32(const float* x, float* out, int64_t B, int64_t n, int64_t d0, int64_t n_d, double sigma, int64_t seed,
                        int64_t id0, te_stream_t stream);
int te_gauss_inputs_bf16(const float* x, te_bf16_t* out, int64_t B, int64_t n, int64_t d0, int64_t n_d, double sigma,
                         int64_t seed, int64_t id0, te_stream_t stream);
int te_grad_accumulate_f32(const float* g, const double* w, double* acc, int64_t B, int64_t n, int64_t n_s, int64_t s0,
                           int square, te_stream_t stream);
int te_grad_accumulate_bf16(const te_bf16_t* g, const double* w, double* acc, int64_t B, int64_t n, int64_t n_s, int64_t s0,
                            int square, te_stream_t stream);
int te_grad_finish_f64(const double* acc, const float* m, float* out, double* sums, int64_t B, int64_t C, int64_t HW,
                       int reduce, te_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TE_RELPROP_H */
