/*
 * s3g_skymodel.h -- C ABI of the sky colour model (libs3g.so): the direction MLP fused with the opacity composite, and its backward.
 *
 * The model (the reference's SkyModel, scene/background_model.py), per pixel (x, y) of an H x W image:
 *
 *   d     = R ((x - cx + 0.5) / fx, (y - cy + 0.5) / fy, 1),   v = d / (|d| + 1e-8)            fp32, R the camera-to-world rotation
 *   e     = [v, sin(2^i v) scale-major for i = 0..4, sin(2^i v + pi/2) likewise]               33 values, fp32, accurate sinf
 *   h0    = relu(W0 e + b0)                          W0 [256,33]
 *   h1    = relu(W1 [h0, e] + b1)                    W1 [256,289]
 *   sky   = sigmoid(W2 h1 + b2)                      W2 [3,256]
 *   image = render + (1 - A) sky                     render made over a ZERO background, A the accumulated opacity
 *
 * ARITHMETIC.  Every layer is a product on v_mfma_f32_32x32x2_f32: each output is a k-ordered chain of fp32 fused multiply-adds
 * (k in the order of the concatenation above), the bias added after the chain.  Nothing is rounded to a narrower format.
 *
 * STATE.  None.  Every entry point works on the buffers it is handed and keeps nothing between calls: no cached pack, no cached
 * size, no per-device set-up (the kernels use static LDS only).  Camera quantities are HOST doubles, read during the call and
 * passed to the kernels by value.  Every extent (tiles, bands, chunks, workspace bytes) comes from s3g_skymodel_plan, which the
 * launchers call themselves; every kernel receives n_pixels = H W and guards the partial tile, band and chunk with it.
 *
 * ORDER.  No floating-point atomics.  A weight gradient is summed over the pixels of one chunk (S3G_SKYMODEL_CHUNK_PIXELS) as an
 * fp32 chain in pixel order, stored, and the chunks are added in double in ascending pixel order, band after band; bias
 * gradients are summed in double from the first pixel on.  Two runs on the same inputs give the same bits.
 */
#ifndef S3G_SKYMODEL_H
#define S3G_SKYMODEL_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define S3G_SKYMODEL_PARAMS 83715          /* W0 8448, b0 256, W1 73984, b1 256, W2 768, b2 3: the flat order of every gradient */
#define S3G_SKYMODEL_CHUNK_PIXELS 256      /* pixels of one fp32 weight-gradient chain */
#define S3G_SKYMODEL_DEFAULT_BAND 16384    /* band_pixels <= 0 selects it */

/* camera, HOST: R_c2w row-major [3][3], then fx, fy, cx, cy (pixel units; pixel (x, y) looks along (x - cx + 0.5, ...)). */
typedef struct s3g_skymodel_camera {
  double R[9];
  double fx, fy, cx, cy;
} s3g_skymodel_camera;

/* What s3g_skymodel_plan decides.  band_pixels is the EFFECTIVE band: the request (or the default) rounded up to whole tiles and
 * cut to the image's whole tiles.  workspace_bytes covers one band's scratch, its chunk partials and the double accumulator. */
typedef struct s3g_skymodel_extents {
  int tile_pixels;     /* pixels one workgroup owns */
  int tiles;           /* ceil(n_pixels / tile_pixels): the forward grid */
  int band_pixels;     /* a multiple of tile_pixels */
  int bands;           /* ceil(n_pixels / band_pixels) */
  int chunks;          /* ceil(band_pixels / S3G_SKYMODEL_CHUNK_PIXELS): weight-gradient partials of a full band */
  int reserved;
  size_t workspace_bytes;
} s3g_skymodel_extents;

/* Pixels per tile (one workgroup). */
int s3g_skymodel_tile_pixels(void);

/* The one function that decides extents.  n_pixels < 1 or >= 2^31 - tile_pixels, or a NULL `out`: S3G_ERR_INVALID_ARG. */
int s3g_skymodel_plan(long long n_pixels, int band_pixels, s3g_skymodel_extents* out);

/* Bytes of the packed weight image s3g_sky_pack writes (transposed copies of the three matrices, the biases, and the h0 columns
 * of W1 and W2 in their own layout for the backward). */
size_t s3g_skymodel_pack_bytes(void);

/* pack <- the six parameter tensors (device, fp32, contiguous, the reference's shapes).  One launch. */
int s3g_sky_pack(const float* W0, const float* b0, const float* W1, const float* b1, const float* W2, const float* b2, float* pack,
                 void* stream);

/* out [3,H,W] <- render + (1 - alpha) sky.  render [3,H,W] and alpha [H,W] may each be NULL: zero render, A = 0 (both NULL:
 * the sky image).  One launch of s3g_skymodel_plan(H W).tiles workgroups; no per-pixel activation leaves the chip. */
int s3g_sky_forward(int H, int W, const s3g_skymodel_camera* cam, const float* pack, const float* render, const float* alpha,
                    float* out, void* stream);

/* Backward of s3g_sky_forward for the upstream gradient g_image [3,H,W]:
 *   d_params [S3G_SKYMODEL_PARAMS]: dW0, db0, dW1, db1, dW2, db2, flat, in that order (written completely)
 *   g_alpha [H,W] (may be NULL): - sum_c g_c sky_c
 * (the gradient of `render` is g_image itself).  Band by band: the band's tiles recompute their activations into the workspace
 * and form dz2, dz1, dz0; three products with K = the chunk's pixels give the weight-gradient partials; a fold adds them to the
 * double accumulator.  workspace: s3g_skymodel_plan(H W, band_pixels).workspace_bytes, contents irrelevant on entry. */
int s3g_sky_backward(int H, int W, const s3g_skymodel_camera* cam, const float* pack, const float* alpha, const float* g_image,
                     int band_pixels, float* d_params, float* g_alpha, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* S3G_SKYMODEL_H */
