/*
 * s3g_lpips.h -- C ABI of the evaluation LPIPS (libs3g.so): the AlexNet variant the reference's evaluation loop reports per frame.
 *
 * What the reference computes (utils/video_utils.py:210-241 calls lpips(rgb, gt, net_type='alex'), lpipsPyTorch/__init__.py:6-21,
 * which builds the network and reloads both weight files on every call) for x, y of shape [3,H,W] fp32:
 *
 *   z-score        z = (img - mean) / std                              lpipsPyTorch/modules/networks.py:41-44, 50-51
 *                  fp32 constants mean = (-.030, -.088, -.188), std = (.458, .448, .450).  The image is used as it is, in [0,1]:
 *                  this variant does NOT rescale to [-1,1] first and does not clamp.
 *   feature stack  torchvision's AlexNet `features`, tapped after each of its five ReLUs          networks.py:53-63, 77-85
 *                  (target_layers = [2, 5, 8, 10, 12], n_channels_list = [64, 192, 384, 256, 256]):
 *                    conv   3 ->  64, k11 s4 p2; ReLU (tap 0); maxpool 3 s2
 *                    conv  64 -> 192, k5  p2;    ReLU (tap 1); maxpool 3 s2
 *                    conv 192 -> 384, k3  p1;    ReLU (tap 2)
 *                    conv 384 -> 256, k3  p1;    ReLU (tap 3)
 *                    conv 256 -> 256, k3  p1;    ReLU (tap 4)          the last pool is never reached (networks.py:61-62)
 *                  Zero padding applies AFTER the z-score, so the z-score cannot be folded into conv1's weights.  Floor-mode pools.
 *   per tap        n = sqrt(sum_c a_c^2),  a^ = a / (n + 1e-10)        lpipsPyTorch/modules/utils.py:6-8: a division, eps outside
 *                  d_c = (a^x_c - a^y_c)^2                             lpipsPyTorch/modules/lpips.py:33            the square root
 *                  tap value = mean over pixels of sum_c w_c d_c       lpips.py:34, networks.py:23-30: w = the tap's [C] lin weights,
 *                                                                      a 1x1 convolution without bias
 *   result         the sum of the five tap values                      lpips.py:36
 *
 * The evaluation loop appends torch.tensor(...).mean().item() per frame and reports non_zero_mean over the frames.
 * Smallest valid image: H, W >= 31 (conv2's output must be >= 3 for the second pool); at 31 the three deep layers are 1 x 1.
 *
 * Here.  Activations are stored [image][Ho][Wo][C], channels innermost, both images in one buffer.  One implicit-GEMM kernel template
 * over (kh, kw, stride, pad, ci, co) convolves BOTH images in one launch (the pixel dimension is 2 Ho Wo) on v_mfma_f32_32x32x2_f32:
 * every output is an exact fp32 fma chain over K ordered (kh, kw, ci), bias added and ReLU applied in the epilogue.  A workgroup of
 * 256 threads owns 128 pixels x 64 channels and stages K in steps of 32 through two LDS buffers.  conv1 gathers from the planar
 * [3,H,W] inputs and applies the z-score at load (a subtraction, then a division); out-of-image taps contribute 0.  The pool is one
 * vectorised pass.  The tap kernel gives a wave the channel vectors of the same pixel of both images: norms by wave reduction, the
 * divisions, sum_c w_c d_c in fp32; every workgroup stores one double partial sum with a plain store and a one-workgroup kernel adds
 * them in a fixed order, divides by Ho Wo and writes the record.  No floating-point atomic anywhere: two runs are bit-identical.
 * Both images go through the same instructions in the same order whichever slot they sit in: lpips(x, x) is exactly 0.0 and
 * lpips(x, y) equals lpips(y, x) bit for bit.
 *
 * The arithmetic does not depend on which weights it is given.  Equality with published LPIPS values rests on the caller's weights
 * (torchvision's alexnet-owt-*.pth and the LPIPS v0.1 alex.pth).
 */
#ifndef S3G_LPIPS_H
#define S3G_LPIPS_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define S3G_LPIPS_TOTAL 0
#define S3G_LPIPS_TAP0 1
#define S3G_LPIPS_RECORD 6 /* doubles per record: {total, tap0..tap4} */
#define S3G_LPIPS_MIN_SIZE 31

/* Bytes of the packed weight blob. */
size_t s3g_lpips_weights_bytes(void);

/* One-time repack on the device.  conv_w[l]: OIHW fp32 ([64,3,11,11], [192,64,5,5], [384,192,3,3], [256,384,3,3], [256,256,3,3]),
 * conv_b[l]: [co], lin_w[l]: [co] -- host arrays of five DEVICE pointers.  packed: s3g_lpips_weights_bytes() bytes on the device,
 * 16-byte aligned.  Per layer the blob holds the conv kernel's B operand [K][co] with K ordered (kh, kw, ci) and zero-padded to the
 * K step of 32, then the bias and the lin weights.  Asynchronous on `stream`; writes only `packed`. */
int s3g_lpips_pack_weights(const float* const conv_w[5], const float* const conv_b[5], const float* const lin_w[5], void* packed,
                           void* stream);

/* Bytes of device workspace s3g_lpips needs for an H x W frame pair: the activations of both images of every layer and the
 * per-workgroup partial sums (about 165 MB at 1066 x 1600); non-decreasing in H and W; 0 for H or W < S3G_LPIPS_MIN_SIZE. */
size_t s3g_lpips_workspace_bytes(int H, int W);

/* image, gt: [3,H,W] fp32 device, contiguous.  packed: the blob of s3g_lpips_pack_weights.
 * record: S3G_LPIPS_RECORD doubles on the device, written: {total, tap0, tap1, tap2, tap3, tap4}.
 * workspace: s3g_lpips_workspace_bytes(H, W) bytes on the device, 16-byte aligned, contents irrelevant on entry.
 * Asynchronous on `stream`; writes record[0..5] and the workspace, nothing else.
 * H < 31 or W < 31, a NULL pointer, or a frame with 2^31 or more activation elements in a layer is refused with S3G_ERR_INVALID_ARG
 * before any device call. */
int s3g_lpips(int H, int W, const float* image, const float* gt, const void* packed, double* record, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
