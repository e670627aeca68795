/*
 * s3g_mlp_geom.h -- C ABI of the "geometry heads" of the deformation MLP: the scale, rotation and opacity heads of
 * scene/deformation.py:61-65,126-152 (ModelHiddenParams no_ds / no_dr / no_do = False) as a second, self-contained kernel family
 * beside s3g_mlp.h (fp32 MFMA on gfx950, libs3g.so).
 *
 * Network (the reference's module names; index 1 and 3 are the two nn.Linear of Sequential(ReLU, Linear, ReLU, Linear)):
 *   hidden = W0 x + b0                                   x: HexPlane features [P,128]      feature_out.0
 *   ds     = C2 relu(C1 relu(hidden) + cb1) + cb2        [P,3]                             scales_deform
 *   dr     = R2 relu(R1 relu(hidden) + rb1) + rb2        [P,4]                             rotations_deform
 *   dopac  = O2 relu(O1 relu(hidden) + ob1) + ob2        [P,1]                             opacity_deform
 * The three heads hang off `hidden` like the heads of s3g_mlp.h, so their contribution to dL/dfeatures, dL/dW0 and dL/db0 is
 * ADDITIVE to that of s3g_deform_mlp_backward: this family recomputes `hidden` from the features (one more read of them and one
 * more 64 x 128 GEMM per direction) and returns its own terms; the caller adds the two (autograd's accumulation does).
 * Weights are torch nn.Linear tensors as they are: weight [out,in] row-major, bias [out], device fp32.
 * Arithmetic: v_mfma_f32_32x32x2_f32 = exact fp32 fma chains, whatever s3g_deform_mlp_set_arithmetic selects for s3g_mlp.h.
 *
 * Which heads run: any non-empty subset.  A head is PRESENT in the forward when its output pointer is not NULL, in the backward
 * when its upstream-gradient pointer is not NULL; the weight (and gradient) pointers of an absent head may be NULL and are never
 * read.  The outputs of a present head are bit for bit the same in every subset.
 */
#ifndef S3G_MLP_GEOM_H
#define S3G_MLP_GEOM_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct s3g_geom_params {  /* the same struct describes weights (const use) and their gradients */
  float *W0, *b0;   /* feature_out.0       [64,128], [64] */
  float *C1, *cb1;  /* scales_deform.1     [64,64],  [64] */
  float *C2, *cb2;  /* scales_deform.3     [3,64],   [3]  */
  float *R1, *rb1;  /* rotations_deform.1  [64,64],  [64] */
  float *R2, *rb2;  /* rotations_deform.3  [4,64],   [4]  */
  float *O1, *ob1;  /* opacity_deform.1    [64,64],  [64] */
  float *O2, *ob2;  /* opacity_deform.3    [1,64],   [1]  */
} s3g_geom_params;

/* bytes of the stash written by forward and read by backward: the packed LDS image of the weights (114 KiB) followed by
 * 4 x [P,64] fp32 activations (hidden, scales1, rotations1, opacity1) and their ReLU masks as bit words.
 * s3g_deform_geom_stash_bytes(0) is the size of the image alone: what a forward with save_activations == 0 needs.
 * The backward workspace holds 4 x [P,64] gradient signals and the weight-gradient kernel's partial blocks (34 MB whatever P). */
size_t s3g_deform_geom_stash_bytes(int P);
size_t s3g_deform_geom_workspace_bytes(int P);

/* features [P,128] -> ds [P,3], dr [P,4], dopac [P,1]; an output pointer that is NULL skips that head (at least one must be
 * given).  `stash`: device scratch of s3g_deform_geom_stash_bytes(P) bytes when save_activations != 0 (a backward will
 * follow), else at least s3g_deform_geom_stash_bytes(0).  The outputs do not depend on save_activations.  P == 0 returns at once. */
int s3g_deform_geom_forward(const s3g_geom_params* w, int P, const float* features, float* ds, float* dr, float* dopac,
                            float* stash, int save_activations, void* stream);

/* g_ds [P,3], g_dr [P,4], g_do [P,1] (upstream gradients; NULL = that head was absent in the forward) -> g_features [P,128]
 * (WRITTEN, not accumulated) and the parameter gradients in `gw` (ACCUMULATED: the caller zero-fills them; the slots of an absent
 * head are not touched and may be NULL).  `features` and `stash` from the matching forward (save_activations != 0, the same head
 * subset, weights unchanged since); `workspace` of s3g_deform_geom_workspace_bytes(P) bytes, uninitialised.
 * The weight gradients use no float atomics: every workgroup stores its partial blocks and a second kernel adds them in
 * workgroup order, so every result of this call is bit-identical from run to run. */
int s3g_deform_geom_backward(const s3g_geom_params* w, int P, const float* features, const float* stash, const float* g_ds,
                             const float* g_dr, const float* g_do, float* g_features, const s3g_geom_params* gw,
                             float* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
