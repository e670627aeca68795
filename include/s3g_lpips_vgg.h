/*
 * s3g_lpips_vgg.h -- C ABI of the evaluation LPIPS, VGG16 variant (libs3g.so): the number the reference's metrics.py reports.
 *
 * What the reference computes (metrics.py:74 calls lpips(render, gt, net_type='vgg'), lpipsPyTorch/__init__.py:6-21, which builds the
 * network and reloads both weight files on every call) for x, y of shape [3,H,W] fp32:
 *
 *   z-score        z = (img - mean) / std                              lpipsPyTorch/modules/networks.py:41-44, 50-51
 *                  the same fp32 constants as the AlexNet variant (s3g_lpips.h).  The image is used as it is, in [0,1]: no rescale
 *                  to [-1,1], no clamp.  Zero padding applies AFTER the z-score.
 *   feature stack  torchvision's vgg16().features                                                 networks.py:53-63, 88-96
 *                  Conv2d modules at indices 0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28, every one k3 s1 p1 and followed by
 *                  a ReLU; 2x2 stride-2 floor-mode max pools at indices 4, 9, 16, 23:
 *                    conv   3 ->  64, conv  64 ->  64 (tap 0); pool
 *                    conv  64 -> 128, conv 128 -> 128 (tap 1); pool
 *                    conv 128 -> 256, conv 256 -> 256, conv 256 -> 256 (tap 2); pool
 *                    conv 256 -> 512, conv 512 -> 512, conv 512 -> 512 (tap 3); pool
 *                    conv 512 -> 512, conv 512 -> 512, conv 512 -> 512 (tap 4)
 *                  target_layers = [4, 9, 16, 23, 30] counts modules from 1 (networks.py:57-59): the taps are the ReLU outputs of
 *                  conv1_2, conv2_2, conv3_3, conv4_3 and conv5_3, each BEFORE the pool that follows it; the fifth pool is never
 *                  reached (networks.py:61-62).  n_channels_list = [64, 128, 256, 512, 512].
 *   per tap        n = sqrt(sum_c a_c^2),  a^ = a / (n + 1e-10)        lpipsPyTorch/modules/utils.py:6-8: a division, eps outside
 *                  d_c = (a^x_c - a^y_c)^2                             lpipsPyTorch/modules/lpips.py:33            the square root
 *                  tap value = mean over pixels of sum_c w_c d_c       lpips.py:34, networks.py:23-30
 *   result         the sum of the five tap values                      lpips.py:36
 *
 * Smallest valid image: H, W >= 16 (16 -> 8 -> 4 -> 2 -> 1); at 16 x 16 the fifth tap is one pixel.
 *
 * Here.  The conventions of s3g_lpips.h: activations [image][H][W][C], channels innermost, both images in one buffer and one launch.
 * A front kernel writes the z-scored images once, channels innermost and padded to 4 channels, so conv1_1 (K = 27, one K step of
 * 32) gathers 16-byte pixels.  One implicit-GEMM kernel template over (ci, co, channel tile) runs the thirteen convolutions on
 * v_mfma_f32_32x32x2_f32: every output is an exact fp32 fma chain over K ordered (kh, kw, ci), bias added and ReLU applied in the
 * epilogue.  A workgroup of 256 threads owns 128 pixels x 128 channels (128 x 64 where co = 64) and stages K in steps of 32 through
 * two LDS buffers.  The pool is one vectorised pass; the tap kernel and the one-workgroup finalise are those of the AlexNet variant.
 * No floating-point atomic anywhere: two runs are bit-identical; lpips(x, x) is exactly 0.0 and lpips(x, y) equals lpips(y, x) bit
 * for bit.  Each tap is consumed right after its layer, so the workspace is two alternating buffers of the block-1 size.
 *
 * The arithmetic does not depend on which weights it is given.  Equality with published LPIPS values rests on the caller's weights
 * (torchvision's vgg16-397923af.pth and the LPIPS v0.1 vgg.pth).
 */
#ifndef S3G_LPIPS_VGG_H
#define S3G_LPIPS_VGG_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define S3G_LPIPS_VGG_CONVS 13
#define S3G_LPIPS_VGG_MIN_SIZE 16
/* The record is s3g_lpips.h's: S3G_LPIPS_RECORD doubles {total, tap0..tap4}, total == (((tap0 + tap1) + tap2) + tap3) + tap4. */

/* Bytes of the packed weight blob. */
size_t s3g_lpips_vgg_weights_bytes(void);

/* One-time repack on the device.  conv_w[l]: OIHW fp32 [co,ci,3,3] of the thirteen convolutions in network order, conv_b[l]: [co],
 * lin_w[t]: [64], [128], [256], [512], [512] -- host arrays of DEVICE pointers.  packed: s3g_lpips_vgg_weights_bytes() bytes on the
 * device, 16-byte aligned.  Per convolution the blob holds the conv kernel's B operand [K][co] with K ordered (kh, kw, ci) and
 * zero-padded to the K step of 32 (only conv1_1, K = 27, is padded), then the bias, then -- after a tapped convolution -- the tap's
 * lin weights.  Asynchronous on `stream`; writes only `packed`. */
int s3g_lpips_vgg_pack_weights(const float* const conv_w[13], const float* const conv_b[13], const float* const lin_w[5],
                               void* packed, void* stream);

/* Bytes of device workspace s3g_lpips_vgg needs for an H x W frame pair: the z-scored pixels, two alternating activation buffers of
 * A1 = 2 * 4 * H * W * 64 bytes each and the per-workgroup partial sums -- at most 2 A1 + A1 / 8 + 1 MiB (about 1.80 GB at
 * 1066 x 1600); non-decreasing in H and W; 0 for H or W < S3G_LPIPS_VGG_MIN_SIZE. */
size_t s3g_lpips_vgg_workspace_bytes(int H, int W);

/* image, gt: [3,H,W] fp32 device, contiguous.  packed: the blob of s3g_lpips_vgg_pack_weights.
 * record: S3G_LPIPS_RECORD doubles on the device, written: {total, tap0, tap1, tap2, tap3, tap4}.
 * workspace: s3g_lpips_vgg_workspace_bytes(H, W) bytes on the device, 16-byte aligned, contents irrelevant on entry.
 * Asynchronous on `stream`; writes record[0..5] and the workspace, nothing else.
 * H < 16 or W < 16, a NULL pointer, or a frame with 2^31 or more activation elements in a layer is refused with S3G_ERR_INVALID_ARG
 * before any device call. */
int s3g_lpips_vgg(int H, int W, const float* image, const float* gt, const void* packed, double* record, void* workspace,
                  void* stream);

#ifdef __cplusplus
}
#endif
#endif
