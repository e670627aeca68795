// Per-pixel photometric terms of train.py:395-425 for gfx950, in one pass each way, and the combine of the loss stage's slotted
// accumulators into the scalar loss (the strip-walking SSIM kernels of ssim.hip add into the same accumulators):
//   l1_loss(image, gt)            utils/loss_utils.py:50-51    mean |image - gt|
//   compute_depth("l2", pred, gt) utils/loss_utils.py:21-45    gt in (0.01, max_depth) selects pixels, both sides are
//                                                              clamp(x / max_depth, 0, 1), mean squared error
//   l2_loss(feat, gt_feat)        utils/loss_utils.py:53-54    mean (feat - gt)^2
// The reference spends ~45 launches here, among them a nonzero + gather for the boolean mask and a radix sort inside
// index_put's backward.
#include "common.hpp"

#include "../../include/s3g_loss.h"

namespace s3g {

struct PixelLossArgs {
  int HW;
  const float *image, *gt_image, *depth, *gt_depth, *feat, *gt_feat;  // [3,HW] [3,HW] [HW] [HW] [3,HW] [3,HW]; pairs may be NULL
  float max_depth;
  double* sums;           // forward: 5 slotted accumulators ([1] l1 [2] depth sq. error [3] depth count [4] feat sq. error);
                          // backward: the 5 collapsed totals
  // backward
  const float* g;         // upstream gradient of the combined loss (device scalar)
  float w_l1, w_depth, w_feat;
  float *g_image, *g_depth, *g_feat;
  int accumulate_image;   // g_image already holds the SSIM gradient
};

__device__ __forceinline__ double block_sum(double v, double* part) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return part[0] + part[1] + part[2] + part[3];
}

__global__ void __launch_bounds__(256) pixel_loss_forward_kernel(const PixelLossArgs a) {
  __shared__ double part[4];
  float l1 = 0.f, dsq = 0.f, cnt = 0.f, fsq = 0.f;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < a.HW; i += gridDim.x * 256) {
    if (a.image != nullptr) {
#pragma unroll
      for (int c = 0; c < 3; c++) l1 += fabsf(a.image[(size_t)c * a.HW + i] - a.gt_image[(size_t)c * a.HW + i]);
    }
    if (a.depth != nullptr) {
      const float gd = a.gt_depth[i];
      if (gd > 0.01f && gd < a.max_depth) {
        const float cp = fminf(fmaxf(a.depth[i] / a.max_depth, 0.f), 1.f), cg = fminf(fmaxf(gd / a.max_depth, 0.f), 1.f);
        dsq += (cp - cg) * (cp - cg);
        cnt += 1.f;
      }
    }
    if (a.feat != nullptr) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const float d = a.feat[(size_t)c * a.HW + i] - a.gt_feat[(size_t)c * a.HW + i];
        fsq += d * d;
      }
    }
  }
  const double s1 = block_sum((double)l1, part), s2 = block_sum((double)dsq, part), s3 = block_sum((double)cnt, part),
               s4 = block_sum((double)fsq, part);
  if (threadIdx.x == 0) {
    double* slot = a.sums + (blockIdx.x % S3G_SUM_SLOTS) * S3G_SUM_STRIDE;
    if (a.image != nullptr) atomicAdd(&slot[1 * S3G_SUM_DOUBLES], s1);
    if (a.depth != nullptr) { atomicAdd(&slot[2 * S3G_SUM_DOUBLES], s2); atomicAdd(&slot[3 * S3G_SUM_DOUBLES], s3); }
    if (a.feat != nullptr) atomicAdd(&slot[4 * S3G_SUM_DOUBLES], s4);
  }
}

__global__ void __launch_bounds__(256) pixel_loss_backward_kernel(const PixelLossArgs a) {
  const float g = *a.g;
  const float k_l1 = g * a.w_l1 / (3.0f * (float)a.HW), k_feat = g * a.w_feat * 2.0f / (3.0f * (float)a.HW);
  // empty mask: the reference's mean over zero elements is NaN and so is its gradient; 0/0 reproduces that
  const float k_depth = a.g_depth != nullptr ? g * a.w_depth * 2.0f / ((float)a.sums[3] * a.max_depth) : 0.f;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < a.HW; i += gridDim.x * 256) {
    if (a.g_image != nullptr) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const float d = a.image[(size_t)c * a.HW + i] - a.gt_image[(size_t)c * a.HW + i];
        const float v = d > 0.f ? k_l1 : (d < 0.f ? -k_l1 : 0.f);
        float* dst = &a.g_image[(size_t)c * a.HW + i];
        *dst = a.accumulate_image ? *dst + v : v;
      }
    }
    if (a.g_depth != nullptr) {
      const float gd = a.gt_depth[i], x = a.depth[i] / a.max_depth;
      float v = 0.f;
      if (gd > 0.01f && gd < a.max_depth && x >= 0.f && x <= 1.f)  // clamp passes the gradient on its closed interval
        v = k_depth * (x - fminf(fmaxf(gd / a.max_depth, 0.f), 1.f));
      a.g_depth[i] = v;
    }
    if (a.g_feat != nullptr) {
#pragma unroll
      for (int c = 0; c < 3; c++)
        a.g_feat[(size_t)c * a.HW + i] = k_feat * (a.feat[(size_t)c * a.HW + i] - a.gt_feat[(size_t)c * a.HW + i]);
    }
  }
}

// totals[q] = sum of accumulator q; loss = w_l1 * T1 / N + w_depth * T2 / T3 + w_ssim * (1 - T0 / N) + w_feat * T4 / NF for
// accumulators that n_views views of one H x W added into: the image terms are means over N = n_views * 3 HW elements, the feature
// term over NF = n_feat_views * 3 HW (the reference supervises the last view's feature image only), the depth term over the batch's
// joint count of valid pixels, which the accumulators already hold.  One view: the factors are 1.0, which is exact.
__global__ void __launch_bounds__(64) pixel_loss_combine_views_kernel(const double* __restrict__ sums, double* __restrict__ totals,
                                                                      int HW, int n_views, int n_feat_views, float w_l1,
                                                                      float w_depth, float w_ssim, float w_feat,
                                                                      float* __restrict__ loss) {
  double T[5];
#pragma unroll
  for (int q = 0; q < 5; q++) {
    double v = sums[(size_t)q * S3G_SUM_DOUBLES + threadIdx.x * S3G_SUM_STRIDE];   // S3G_SUM_SLOTS == 64 == one wave
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    T[q] = v;
  }
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int q = 0; q < 5; q++) totals[q] = T[q];
  const double N = 3.0 * (double)HW * (double)n_views, NF = 3.0 * (double)HW * (double)n_feat_views;
  double v = 0.0;
  if (w_l1 != 0.f) v += (double)w_l1 * T[1] / N;
  if (w_depth != 0.f) v += (double)w_depth * T[2] / T[3];
  if (w_ssim != 0.f) v += (double)w_ssim * (1.0 - T[0] / N);
  if (w_feat != 0.f) v += (double)w_feat * T[4] / NF;
  *loss = (float)v;
}

}  // namespace s3g

using namespace s3g;

extern "C" int s3g_pixel_losses_forward(int H, int W, const float* image, const float* gt_image, const float* depth,
                                        const float* gt_depth, const float* feat, const float* gt_feat, float max_depth,
                                        double* sums, void* stream_) {
  if (H <= 0 || W <= 0 || !sums || (image && !gt_image) || (depth && !gt_depth) || (feat && !gt_feat)) {
    set_error("s3g_pixel_losses_forward: bad argument");
    return S3G_ERR_INVALID_ARG;
  }
  PixelLossArgs a;
  memset(&a, 0, sizeof a);
  a.HW = H * W; a.image = image; a.gt_image = gt_image; a.depth = depth; a.gt_depth = gt_depth; a.feat = feat;
  a.gt_feat = gt_feat; a.max_depth = max_depth; a.sums = sums;
  const int blocks = min((a.HW + 255) / 256, 1024);
  hipLaunchKernelGGL(pixel_loss_forward_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream_, a);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

static int launch_combine(int HW, int n_views, int n_feat_views, const double* sums, double* totals, float w_l1, float w_depth,
                          float w_ssim, float w_feat, float* loss, void* stream_) {
  static_assert(S3G_SUM_SLOTS == 64, "the combine kernel reduces the slots with one wave");
  hipLaunchKernelGGL(pixel_loss_combine_views_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream_, sums, totals, HW, n_views,
                     n_feat_views, w_l1, w_depth, w_ssim, w_feat, loss);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" int s3g_pixel_losses_combine(int H, int W, const double* sums, double* totals, float w_l1, float w_depth,
                                        float w_ssim, float w_feat, float* loss, void* stream_) {
  if (H <= 0 || W <= 0 || !sums || !totals || !loss) {
    set_error("s3g_pixel_losses_combine: bad argument");
    return S3G_ERR_INVALID_ARG;
  }
  return launch_combine(H * W, 1, 1, sums, totals, w_l1, w_depth, w_ssim, w_feat, loss, stream_);
}

extern "C" int s3g_pixel_losses_combine_views(int H, int W, int n_views, int n_feat_views, const double* sums, double* totals,
                                              float w_l1, float w_depth, float w_ssim, float w_feat, float* loss, void* stream_) {
  if (H <= 0 || W <= 0 || n_views < 1 || n_feat_views < 0 || (n_feat_views == 0 && w_feat != 0.f) || !sums || !totals || !loss) {
    set_error("s3g_pixel_losses_combine_views: bad argument");
    return S3G_ERR_INVALID_ARG;
  }
  return launch_combine(H * W, n_views, n_feat_views, sums, totals, w_l1, w_depth, w_ssim, w_feat, loss, stream_);
}

extern "C" int s3g_pixel_losses_backward(int H, int W, const float* image, const float* gt_image, const float* depth,
                                         const float* gt_depth, const float* feat, const float* gt_feat, float max_depth,
                                         const double* sums, const float* g, float w_l1, float w_depth, float w_feat,
                                         float* g_image, int accumulate_image, float* g_depth, float* g_feat, void* stream_) {
  if (H <= 0 || W <= 0 || !sums || !g || (g_image && (!image || !gt_image)) || (g_depth && (!depth || !gt_depth)) ||
      (g_feat && (!feat || !gt_feat))) {
    set_error("s3g_pixel_losses_backward: bad argument");
    return S3G_ERR_INVALID_ARG;
  }
  PixelLossArgs a;
  memset(&a, 0, sizeof a);
  a.HW = H * W; a.image = image; a.gt_image = gt_image; a.depth = depth; a.gt_depth = gt_depth; a.feat = feat;
  a.gt_feat = gt_feat; a.max_depth = max_depth; a.sums = const_cast<double*>(sums); a.g = g;
  a.w_l1 = w_l1; a.w_depth = w_depth; a.w_feat = w_feat;
  a.g_image = g_image; a.accumulate_image = accumulate_image; a.g_depth = g_depth; a.g_feat = g_feat;
  const int blocks = min((a.HW + 255) / 256, 4096);
  hipLaunchKernelGGL(pixel_loss_backward_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream_, a);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}
