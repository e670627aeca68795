/*
 * s3g_mlp.h -- C ABI of the fused deformation-MLP kernels (fp32 MFMA on gfx950, libs3g.so).
 *
 *   s3g_deform_mlp_forward   <- Deformation.query_time's feature_out + the pos_deform / shs_deform / dino_head
 *                               Sequentials of forward_dynamic   (/root/reference/scene/deformation.py:53-76,78-94,108-166)
 *   s3g_deform_mlp_backward  <- their autograd (10 nn.Linear backward GEMM pairs + ReLU masks)
 *
 * Network (reference defaults, arguments/__init__.py:204-233: net_width 64, defor_depth 1, feat_head on):
 *   hidden = W0 x + b0                                   x: HexPlane features [P,128]
 *   dx     = P2 relu(P1 relu(hidden) + pb1) + pb2        [P,3]
 *   dshs   = S2 relu(S1 relu(hidden) + sb1) + sb2        [P,48]
 *   feat   = D2 relu(D1 relu(D0 hidden + db0) + db1) + db2   [P,3]   (dino_head has NO leading ReLU, deformation.py:70-76)
 * Weights are torch nn.Linear tensors as they are: weight [out,in] row-major, bias [out], device fp32.
 * Arithmetic: v_mfma_f32_32x32x2_f32 = exact fp32 fma chains (no reduced precision).
 */
#ifndef S3G_MLP_H
#define S3G_MLP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct s3g_mlp_params {  /* the same struct describes weights (const use) and their gradients */
  float *W0, *b0;   /* feature_out.0  [64,128], [64] */
  float *P1, *pb1;  /* pos_deform.1   [64,64],  [64] */
  float *P2, *pb2;  /* pos_deform.3   [3,64],   [3]  */
  float *S1, *sb1;  /* shs_deform.1   [64,64],  [64] */
  float *S2, *sb2;  /* shs_deform.3   [48,64],  [48] */
  float *D0, *db0;  /* dino_head.0    [64,64],  [64] */
  float *D1, *db1;  /* dino_head.2    [64,64],  [64] */
  float *D2, *db2;  /* dino_head.4    [3,64],   [3]  */
} s3g_mlp_params;

/* bytes of the stash written by forward and read by backward: the packed LDS images of the weights
 * (s3g_deform_mlp_pack_bytes) followed by 5 x [P,64] fp32 activations (hidden, pos1, shs1, dino1, dino2).  The
 * backward workspace (5 gradient signals) needs 5 * P * 64 * 4 bytes. */
size_t s3g_deform_mlp_stash_bytes(int P);
size_t s3g_deform_mlp_pack_bytes(void);

/* features [P,128] -> dx [P,3], dshs [P,48], feat [P,3].  `stash`: device scratch of s3g_deform_mlp_stash_bytes(P)
 * bytes when save_activations != 0 (a backward will follow), else at least s3g_deform_mlp_pack_bytes().
 * feat may be NULL when save_activations == 0: the feature (dino) head is then skipped -- a render that does not draw the
 * feature image (gaussian_renderer/__init__.py:153, render_feat=False) has no use for it.
 * dx may be NULL (static scenes, ModelHiddenParams no_dx=True: scene/deformation.py:119-121 never calls the head): the position
 * head is skipped -- P1, its ReLU, P2 and the dx store are not computed, and with save_activations != 0 stash plane 1 (pos1) and
 * mask word 1 of every tile are left unwritten.  dshs, feat and every other stash plane / mask word are bit for bit what the call
 * writes with a non-NULL dx.  Combines with feat == NULL.  w->P1..pb2 stay valid pointers in every case: the weight images are
 * packed whole.
 * feat == NULL with save_activations != 0 is valid too (a network without a feature head, ModelHiddenParams feat_head=False): stash
 * planes 3 and 4 (dino1, dino2) and mask words 3 and 4 of every tile are left unwritten, and the backward must be given g_feat == NULL.
 * w->D0..db2 stay valid pointers (a zero block will do).
 * dshs may be NULL (no_dshs=True): no S1, no ReLU, no S2 and no [P,48] store; stash plane 2 (shs1) and mask word 2 stay unwritten.
 * These calls run the exact fp32 MFMA chain in EVERY arithmetic mode below (csrc/mlp_heads.hip); in S3G_MLP_F32 dx and feat are bit
 * for bit what the call writes with a non-NULL dshs.  Combines with dx == NULL or feat == NULL, but at least one of the three outputs
 * must be given: with P > 0 a call whose dx, dshs and feat are all NULL returns S3G_ERR_INVALID_ARG (P == 0 returns S3G_OK before
 * looking at them). */
int s3g_deform_mlp_forward(const s3g_mlp_params* w, int P, const float* features, float* dx, float* dshs, float* feat,
                           float* stash, int save_activations, void* stream);

/* g_dx [P,3], g_dshs [P,48], g_feat [P,3] (upstream gradients) -> g_features [P,128] (written) and the parameter
 * gradients in `gw` (ACCUMULATED: the caller zero-fills them).  `stash` from the matching forward (weights must be
 * unchanged since); `workspace` of 5 * P * 64 * 4 bytes, uninitialised.
 * g_feat may be NULL = the feature output received no gradient (the feature image is not in the loss): the dino head's
 * backward is skipped and gw->D0..db2 are left untouched, like autograd leaving those parameters' .grad at None.
 * g_dx may be NULL = the forward ran with dx == NULL: the position head's backward is skipped -- no read of g_dx, of mask word 1 or of
 * stash plane 1, workspace plane 2 (the pos1 signal) is not written -- and gw->P1, pb1, P2, pb2 are left untouched and may be NULL.
 * g_dshs may be NULL = the forward ran with dshs == NULL: the exact fp32 chain without the SH head, in every arithmetic mode -- no
 * read of g_dshs, of mask word 2 or of stash plane 2, workspace plane 3 (the shs1 signal) is not written -- and gw->S1, sb1, S2, sb2
 * are left untouched and may be NULL; s3g_deform_mlp_wgrad_partial_bytes() stays an upper bound.  In S3G_MLP_F32 the results are
 * those of the call fed an all-zero g_dshs.
 * Every combination of g_dx / g_dshs / g_feat being NULL or not is valid except all three NULL, which (with P > 0) returns
 * S3G_ERR_INVALID_ARG, as does a NULL gw->W0 / b0 or a NULL gw slot of a head whose upstream gradient is given
 * (s3g_deform_mlp_backward_ordered alike). */
int s3g_deform_mlp_backward(const s3g_mlp_params* w, int P, const float* features, const float* stash, const float* g_dx,
                            const float* g_dshs, const float* g_feat, float* g_features, const s3g_mlp_params* gw,
                            float* workspace, void* stream);

/* The same with an ORDERED flush of the weight gradients (ABI 13).  s3g_deform_mlp_backward lets the up to 256 workgroups of the
 * weight-gradient kernel add their partial [out][in] blocks onto `gw` with float atomics: the order of the additions, and with it
 * the last bits of every weight gradient, differs from run to run.  Here each workgroup stores its partial blocks into
 * `wgrad_partials` (device scratch of s3g_deform_mlp_wgrad_partial_bytes() bytes, uninitialised) and a second kernel adds them in
 * workgroup order: the weight gradients are bit-reproducible (tests/test_mlp_gpu.py), for 38 MB of scratch traffic and one launch. */
size_t s3g_deform_mlp_wgrad_partial_bytes(void);
int s3g_deform_mlp_backward_ordered(const s3g_mlp_params* w, int P, const float* features, const float* stash, const float* g_dx,
                                    const float* g_dshs, const float* g_feat, float* g_features, const s3g_mlp_params* gw,
                                    float* workspace, float* wgrad_partials, void* stream);

/* Arithmetic of the per-point GEMM chains of the two calls above (process-wide setting, default S3G_MLP_F32):
 *   S3G_MLP_F32     v_mfma_f32_32x32x2_f32, exact fp32 fma chains.
 *   S3G_MLP_BF16X3  v_mfma_f32_32x32x16_bf16 (the bf16 matrix pipe, 16 x the rate) with every fp32 operand -- weights, activations,
 *                   gradients -- split EXACTLY into three bf16 pieces and six piece products accumulated in fp32 per product: what
 *                   is dropped is <= 2^-23 of each product (fp32 accuracy; not bit-identical to S3G_MLP_F32).  The split is
 *                   exact for 2^-110 <= |x| < 3.39e38 (smaller numbers keep an absolute error below 2^-133; larger ones
 *                   become infinite like any bf16 conversion): tests/test_split_arith_cpu.py.
 *                   Round 5: the weight fragments of both chain kernels are split ONCE per call into 159 KiB LDS images
 *                   (mlp_forward_presplit_kernel / mlp_backward_presplit_kernel; P1 alone is split by the lanes that read it, the
 *                   3-row heads of the backward run on the exact fp32 MFMA): forward 0.71 -> 0.55 ms, backward 0.76 -> 0.63 ms at
 *                   1.2 M points on one box.  (The backward writes its transposed image into the slot the stash reserves for it;
 *                   forward and backward may run in different modes.)
 *   S3G_MLP_BF16X3_ONTHEFLY  the same arithmetic with every fragment split by the wave that uses it (rounds 3-4; bit-identical
 *                   results, 15-20 % slower): kept as the checker of the pre-split kernels.
 * The weight-gradient GEMMs (K = points) are the exact fp32 chain in every mode.  Returns S3G_ERR_INVALID_ARG for another mode. */
enum { S3G_MLP_F32 = 0, S3G_MLP_BF16X3 = 1, S3G_MLP_BF16X3_ONTHEFLY = 2 };
int s3g_deform_mlp_set_arithmetic(int mode);
int s3g_deform_mlp_get_arithmetic(void);

/* Inference only (no autograd): HexPlane sampler (+) feature_out + position / SH heads in ONE kernel -- what
 * deform_network.forward_dynamic computes under torch.no_grad() for a render that does not draw the feature image
 * (/root/reference/scene/deformation.py:108-166 with the default switches, called from gaussian_renderer/__init__.py:82-97).
 * xyz [P,3], time [P] -> dx [P,3], dshs [P,48]; the [P,128] feature array is never materialised.  Results are bit-identical to
 * s3g_hexplane_forward followed by s3g_deform_mlp_forward(feat = NULL).  The descriptor must have 4 levels (4 x 32 = the 128 inputs
 * of feature_out).  `workspace`: s3g_deform_infer_workspace_bytes(d) bytes, uninitialised.  proc_order as in s3g_hexplane_forward. */
#include "s3g_hexplane.h"
size_t s3g_deform_infer_workspace_bytes(const s3g_hexplane_desc* d);
int s3g_deform_infer(const s3g_hexplane_desc* d, const s3g_mlp_params* w, int P, const float* xyz, const float* time,
                     const unsigned int* proc_order, float* dx, float* dshs, void* workspace, void* stream);
/* The same call with the three GEMM layers on the bf16 matrix pipe (v_mfma_f32_32x32x16_bf16, 16 x the fp32 MFMA rate): every fp32
 * operand -- weights and activations -- is the EXACT sum of three bf16 pieces and a product is accumulated (in fp32) as the six
 * piece products of weight >= 2^-16; what is dropped is <= 2^-23 of each product, i.e. fp32 accuracy (measured against fp64 beside
 * the exact path: tests/test_infer_gpu.py), but not bit-identical to s3g_deform_infer.  The sampler half is the same code. */
int s3g_deform_infer_split(const s3g_hexplane_desc* d, const s3g_mlp_params* w, int P, const float* xyz, const float* time,
                           const unsigned int* proc_order, float* dx, float* dshs, void* workspace, void* stream);

/* The one-kernel inference form for the OTHER head sets: sampler (+) feature_out (+) any subset of the position / scale / rotation /
 * opacity / SH heads whose weight image fits the CU's LDS beside the sampler's staging tiles (csrc/deform_infer_heads.hip).  Exact fp32
 * only; there is no feature head here.
 *   head_mask   bit 0 dx, bit 1 ds, bit 2 dr, bit 3 do, bit 4 dshs.
 *   served      every non-empty subset of {dx, ds, dr, do} with at most three heads (14 sets), dshs alone, dshs with exactly one of
 *               ds / dr / do (3 sets): 18 sets.  Not served: the empty set, dx + dshs alone (s3g_deform_infer's set) and every set whose
 *               image does not fit (four first layers beside W0 and the second layers, e.g. all five heads).
 * s3g_deform_infer_heads_lds_bytes: the dynamic LDS the kernel is launched with for that set (weight image + 8 x 6 912 B of staging; at
 * most 160 KiB, a multiple of 16), or 0 for a set that is not served.  Pure host code: callable without a GPU.
 * s3g_deform_infer_heads: xyz [P,3], time [P] -> the outputs whose pointer is not NULL (dx [P,3], dshs [P,48], ds [P,3], dr [P,4],
 * dopac [P,1]); a NULL output is an absent head, and the weight pointers of an absent head are never read (`gw` may be NULL when none
 * of ds / dr / dopac is given; feature_out's W0 / b0 are taken from `w`).  Every output is bit-identical to s3g_hexplane_forward ->
 * s3g_deform_mlp_forward(feat = NULL, save_activations = 0) in S3G_MLP_F32 (without dshs that call is the exact chain in every mode)
 * -> s3g_deform_geom_forward(save_activations = 0) on the same (xyz, time, proc_order, uniform_time), and what a present head
 * computes does not depend on which others are present.  The descriptor must have 4 levels; `workspace`:
 * s3g_deform_infer_workspace_bytes(d) bytes, uninitialised; proc_order as in s3g_hexplane_forward.  P == 0 returns S3G_OK at once
 * (after the argument checks that need no buffer); a set that is not served returns S3G_ERR_INVALID_ARG with a message naming it. */
#include "s3g_mlp_geom.h"
size_t s3g_deform_infer_heads_lds_bytes(int head_mask);
int s3g_deform_infer_heads(const s3g_hexplane_desc* d, const s3g_mlp_params* w, const s3g_geom_params* gw, int P, const float* xyz,
                           const float* time, const unsigned int* proc_order, float* dx, float* dshs, float* ds, float* dr,
                           float* dopac, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
