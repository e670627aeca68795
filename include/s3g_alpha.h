/*
 * s3g_alpha.h -- C ABI of the accumulated-opacity image and the sky-mask loss on it (libs3g.so).
 *
 * The blend forward keeps the final transmittance of every pixel, T_final = prod (1 - alpha_i) over the Gaussians it blended
 * (ImageState::final_T, the first H*W floats of the image arena).  The accumulated opacity is A = 1 - T_final: what a render
 * of unit colours on a black background would give, without rendering again.  Street scenes supervise it against a sky
 * mask (the reference loads `sky_mask` per frame and consumes it nowhere): A should be 0 where the mask says sky, 1 elsewhere.
 *
 * The gradient of a loss on A goes back through the ordinary blend backward: s3g_raster_backward_alpha below.
 */
#ifndef S3G_ALPHA_H
#define S3G_ALPHA_H
#include <stddef.h>

#include "s3g_raster.h"
#ifdef __cplusplus
extern "C" {
#endif

/* out_alpha [1,H,W] fp32 device: A[pix] = 1 - final_T[pix] of the forward that filled `image_arena` (synchronous,
 * asynchronous, two-image or reuse; an asynchronous forward that overflowed blended nothing: A = 0 everywhere).  A pixel
 * without contributor gives exactly 0.  Reads the first width*height floats of the arena and nothing else. */
int s3g_raster_alpha(int width, int height, const void* image_arena, float* out_alpha, void* stream);

/* Blend + geometry backward with an upstream gradient on A as well: the arguments of s3g_raster_backward2_accum, plus
 * dL_dalpha [1,H,W] (required) and dL_dsh (the one-image shape with SH colours).  colors2, dL_dpix2 and dL_dcolor2 are all
 * three NULL (one image, the shape of s3g_raster_backward; workspace of s3g_raster_backward_workspace_bytes) or all three
 * given (two images, s3g_raster_backward2; workspace of s3g_raster_backward2_workspace_bytes).  dens may be NULL, or carry
 * three NULL arrays (no bookkeeping), or all three.  With dL_dalpha all zero every output equals the matching existing
 * entry point's bit for bit. */
int s3g_raster_backward_alpha(const s3g_raster_inputs* in, const float* colors2, int R, const int* radii,
                              const void* geometry_arena, const void* binning_arena, const void* image_arena,
                              void* workspace, const float* dL_dpix, const float* dL_dpix_depth, const float* dL_dpix2,
                              const float* dL_dalpha, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity,
                              float* dL_dcolor, float* dL_dcolor2, float* dL_ddepth, float* dL_dmean3D, float* dL_dcov3D,
                              float* dL_dsh, float* dL_dscale, float* dL_drot, const s3g_densify_accum* dens, void* stream);

/* Sky-mask loss of one view, one pass over the image:
 *     a     = clamp(A, 1e-6, 1 - 1e-6)                              (fp32, like torch.clamp on an fp32 image)
 *     loss  = weight * mean over H*W of  -(1 - s) log(a) - s log(1 - a)     (binary cross entropy against 1 - s)
 *     grad  = d loss / d A = weight / (H*W) * ( -(1 - s) / a + s / (1 - a) ),  0 where the clamp is active
 * alpha [H*W] fp32: the opacity image A (s3g_raster_alpha's output).
 * mask [H*W] fp32, s in [0,1] (soft values allowed: 1 = sky).  out_grad [H*W] fp32, written: the quotient, the difference and
 * the scale are formed in double and rounded to fp32 once.
 * The per-pixel loss terms are evaluated in fp32 and summed in double: one partial per workgroup in `workspace`
 * (s3g_sky_loss_workspace_bytes), added in a fixed order by a second one-workgroup kernel.  No floating-point atomics:
 * two runs on the same inputs are bit-identical.
 * slot: views that share one total call with slot = 0, 1, 2, ... on the same stream and the same `total`: slot 0 stores
 * its weighted loss into total[0] (double, device), every later slot adds its own; each call also stores (float)total[0]
 * into loss[0].  V views with weight = lambda / V each give lambda * the mean over V*H*W.
 * Asynchronous on `stream`; nothing waits for the device. */
size_t s3g_sky_loss_workspace_bytes(int width, int height);
int s3g_sky_loss(int width, int height, const float* alpha, const float* mask, float weight, int slot, float* out_grad,
                 double* total, float* loss, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* S3G_ALPHA_H */
