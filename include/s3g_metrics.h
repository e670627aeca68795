/*
 * s3g_metrics.h -- C ABI of the evaluation metrics (libs3g.so): PSNR, SSIM and their masked forms for one rendered frame.
 *
 * What the reference's evaluation loop does per frame (utils/video_utils.py:210-241) with two device-to-host image copies, two
 * scikit-image SSIMs on the CPU and a host synchronisation per number:
 *
 *   psnr          psnr(rgb, gt_rgb).mean()                      utils/video_utils.py:211 over utils/image_utils.py:17-19:
 *                                                               per channel 20 * log10(1 / sqrt(mean (rgb - gt)^2)), then the mean of
 *                                                               the three channel values (NOT the PSNR of the pooled error)
 *   ssim          structural_similarity(rgb, gt, data_range=1.0, channel_axis=0)          utils/video_utils.py:213-220
 *   masked_psnr   the same psnr over the pixels of camera.dynamic_mask only               utils/video_utils.py:223-232
 *   masked_ssim   structural_similarity(..., full=True)[1][dynamic_mask].mean()           utils/video_utils.py:233-241
 *
 * structural_similarity with its defaults, restated (this is NOT the training loss of s3g_loss.h, which uses an 11x11 Gaussian
 * window, zero padding, population covariance and the mean over the whole map):
 *   per channel, a 7x7 uniform window with the borders of scipy.ndimage.uniform_filter(mode='reflect') -- the edge pixel is
 *   repeated: index -1 reads 0, -2 reads 1, H reads H-1 (numpy's 'symmetric', not torch's 'reflect');
 *   box means ux, uy, uxx, uyy, uxy;  sample covariance vx = 49/48 (uxx - ux ux), vy, vxy alike;  C1 = 0.01^2, C2 = 0.03^2;
 *   S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2))
 *   ssim        = mean of S over the interior [3:H-3, 3:W-3] and the three channels
 *   masked_ssim = mean of the UNCROPPED S over the masked pixels and the three channels
 *
 * One workgroup takes a 32 x 16 pixel tile of all three channels with a 3-pixel halo in LDS; the box sums are separable (rows, then
 * columns), accumulated in double and rounded to fp32 once per box mean, S itself is fp32 like scikit-image's for fp32 images.
 * image, gt and mask are read once (plus halo).  Every workgroup stores nine double partial sums into the workspace with plain
 * stores; a second one-workgroup kernel adds them in a fixed order and evaluates the record: there is no floating-point atomic in
 * this path, two runs on the same inputs are bit-identical.
 */
#ifndef S3G_METRICS_H
#define S3G_METRICS_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define S3G_METRICS_PSNR 0
#define S3G_METRICS_SSIM 1
#define S3G_METRICS_MASKED_PSNR 2
#define S3G_METRICS_MASKED_SSIM 3
#define S3G_METRICS_MASKED_PIXELS 4
#define S3G_METRICS_RECORD 5 /* doubles per record */

/* Bytes of device workspace s3g_image_metrics needs for an H x W frame (the per-workgroup partial sums); non-decreasing in H and W. */
size_t s3g_image_metrics_workspace_bytes(int H, int W);

/* image, gt: [3,H,W] fp32 device, values in [0,1].  mask: [H,W] bytes on the device, non-zero = dynamic pixel, or NULL.
 * record: S3G_METRICS_RECORD doubles on the device, written: {psnr, ssim, masked_psnr, masked_ssim, masked_pixels}.
 * ssim_map: [3,H,W] fp32 device or NULL; receives the full (uncropped) S map.
 * workspace: s3g_image_metrics_workspace_bytes(H, W) bytes on the device, contents irrelevant on entry.
 * Asynchronous on `stream`; writes record[0..4], the workspace and the map, nothing else.
 *
 * Edge cases follow the reference: a channel without error has PSNR +inf (log10(1/0)) and so has the mean over the channels; an
 * empty or absent mask gives NaN in both masked entries and 0 in masked_pixels (the reference's loop skips such a frame,
 * `if dynamic_mask.sum() > 0`).  H < 7 or W < 7 is refused with S3G_ERR_INVALID_ARG before any device call (scikit-image raises
 * for an image smaller than its window, too). */
int s3g_image_metrics(int H, int W, const float* image, const float* gt, const unsigned char* mask, double* record,
                      float* ssim_map, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
