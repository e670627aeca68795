// Evaluation metrics of one rendered frame for gfx950: PSNR, scikit-image's SSIM (7x7 uniform window, edge-repeating borders,
// sample covariance) and both under a dynamic mask.  Reference: utils/video_utils.py:210-241 = psnr() of utils/image_utils.py:17-19,
// two structural_similarity() calls on CPU copies of the image and a boolean gather, one host synchronisation per number.
// Here: one kernel over 32x16 pixel tiles of all three channels (38x22 halo tile in LDS, separable box sums in double) that leaves
// nine partial sums per workgroup, and a one-workgroup kernel that adds them in a fixed order and writes the 5-double record.
#include "common.hpp"

#include "../../include/s3g_metrics.h"

namespace s3g {

constexpr int MT_W = 32, MT_H = 16, MT_R = 3;                    // tile, window radius
constexpr int MT_HW = MT_W + 2 * MT_R, MT_HH = MT_H + 2 * MT_R;  // halo tile 38 x 22
constexpr int MT_ROWS = MT_H / 8;                                // output rows per thread (256 threads = 32 columns x 8 rows)
// partial sums of one workgroup: [0..2] squared error per channel, [3..5] the same under the mask, [6] S over the interior,
// [7] S under the mask, [8] masked pixels
constexpr int MT_PART = 9;

// scipy.ndimage mode='reflect' (numpy 'symmetric'): ... 2 1 0 | 0 1 2 ... n-1 | n-1 n-2 ...   One fold covers the three halo pixels
// of n >= 7; positions further out belong to pixels beyond the image (ragged last tile) and are only kept inside the array.
__device__ __forceinline__ int symmetric_index(int i, int n) {
  if (i < 0) i = -1 - i;
  if (i >= n) i = 2 * n - 1 - i;
  return min(max(i, 0), n - 1);
}

// Sum of each of the MT_PART values over the workgroup, in a fixed order: xor butterfly inside a wave, then wave 0..3.
__device__ __forceinline__ void block_sum_parts(double (&v)[MT_PART], double (*red)[MT_PART]) {
#pragma unroll
  for (int q = 0; q < MT_PART; q++) {
    for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_xor(v[q], o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][q] = v[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < MT_PART; q++) v[q] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
}

__global__ void __launch_bounds__(256) image_metrics_tile_kernel(int H, int W, const float* __restrict__ image,
                                                                 const float* __restrict__ gt,
                                                                 const unsigned char* __restrict__ mask,
                                                                 float* __restrict__ ssim_map, double* __restrict__ partial) {
  __shared__ float t1[MT_HH][MT_HW + 1], t2[MT_HH][MT_HW + 1];
  __shared__ double hb[5][MT_HH][MT_W + 1];
  __shared__ double red[4][MT_PART];
  const int x0 = blockIdx.x * MT_W, y0 = blockIdx.y * MT_H;
  const int tid = threadIdx.x, lx = tid & (MT_W - 1), ly = tid >> 5;
  const int gx = x0 + lx;
  const size_t HW = (size_t)H * W;
  bool valid[MT_ROWS], masked[MT_ROWS], interior[MT_ROWS];
  double acc[MT_PART];
#pragma unroll
  for (int q = 0; q < MT_PART; q++) acc[q] = 0.0;
#pragma unroll
  for (int j = 0; j < MT_ROWS; j++) {
    const int gy = y0 + ly + 8 * j;
    valid[j] = gx < W && gy < H;
    masked[j] = valid[j] && mask != nullptr && mask[(size_t)gy * W + gx] != 0;
    interior[j] = gx >= MT_R && gx < W - MT_R && gy >= MT_R && gy < H - MT_R;
    if (masked[j]) acc[8] += 1.0;
  }
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const size_t plane = (size_t)c * HW;
    __syncthreads();   // the previous channel's column pass is done with hb and with the centre pixels of t1 / t2
    for (int i = tid; i < MT_HH * MT_HW; i += 256) {
      const int r = i / MT_HW, q = i - r * MT_HW;
      const size_t o = plane + (size_t)symmetric_index(y0 + r - MT_R, H) * W + symmetric_index(x0 + q - MT_R, W);
      t1[r][q] = image[o];
      t2[r][q] = gt[o];
    }
    __syncthreads();
    // row pass: seven fp32 taps (products rounded to fp32 like scikit-image's im1 * im2), summed in double
    for (int i = tid; i < MT_HH * MT_W; i += 256) {
      const int r = i / MT_W, q = i - r * MT_W;
      double a = 0.0, b = 0.0, aa = 0.0, bb = 0.0, ab = 0.0;
#pragma unroll
      for (int k = 0; k < 2 * MT_R + 1; k++) {
        const float u = t1[r][q + k], v = t2[r][q + k];
        a += (double)u; b += (double)v; aa += (double)(u * u); bb += (double)(v * v); ab += (double)(u * v);
      }
      hb[0][r][q] = a; hb[1][r][q] = b; hb[2][r][q] = aa; hb[3][r][q] = bb; hb[4][r][q] = ab;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < MT_ROWS; j++) {
      if (!valid[j]) continue;
      const int row = ly + 8 * j;
      double s[5];
#pragma unroll
      for (int m = 0; m < 5; m++) {   // column pass
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < 2 * MT_R + 1; k++) v += hb[m][row + k][lx];
        s[m] = v;
      }
      // each box mean is rounded to fp32 once; from here on fp32 in scikit-image's order of operations
      const float ux = (float)(s[0] / 49.0), uy = (float)(s[1] / 49.0), uxx = (float)(s[2] / 49.0), uyy = (float)(s[3] / 49.0),
                  uxy = (float)(s[4] / 49.0);
      const float cov_norm = (float)(49.0 / 48.0), C1 = (float)(0.01 * 0.01), C2 = (float)(0.03 * 0.03);
      const float vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
      const float A1 = 2.f * ux * uy + C1, A2 = 2.f * vxy + C2, B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
      const float S = (A1 * A2) / (B1 * B2);
      const float d = t1[row + MT_R][lx + MT_R] - t2[row + MT_R][lx + MT_R];
      const double d2 = (double)d * (double)d;
      acc[c] += d2;
      if (masked[j]) { acc[3 + c] += d2; acc[7] += (double)S; }
      if (interior[j]) acc[6] += (double)S;
      if (ssim_map != nullptr) ssim_map[plane + (size_t)(y0 + row) * W + gx] = S;
    }
  }
  block_sum_parts(acc, red);
  if (tid == 0) {
    double* dst = partial + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * MT_PART;
#pragma unroll
    for (int q = 0; q < MT_PART; q++) dst[q] = acc[q];
  }
}

__device__ __forceinline__ double psnr_of_mse(double mse) { return 20.0 * log10(1.0 / sqrt(mse)); }   // image_utils.py:17-19

__global__ void __launch_bounds__(256) image_metrics_reduce_kernel(int H, int W, int nblocks, const double* __restrict__ partial,
                                                                   double* __restrict__ record) {
  __shared__ double red[4][MT_PART];
  double acc[MT_PART];
#pragma unroll
  for (int q = 0; q < MT_PART; q++) acc[q] = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += 256) {
#pragma unroll
    for (int q = 0; q < MT_PART; q++) acc[q] += partial[(size_t)b * MT_PART + q];
  }
  block_sum_parts(acc, red);
  if (threadIdx.x != 0) return;
  const double n = (double)H * (double)W, count = acc[8], nan = __builtin_nan("");
  record[S3G_METRICS_PSNR] = (psnr_of_mse(acc[0] / n) + psnr_of_mse(acc[1] / n) + psnr_of_mse(acc[2] / n)) / 3.0;
  record[S3G_METRICS_SSIM] = acc[6] / (3.0 * (double)(H - 2 * MT_R) * (double)(W - 2 * MT_R));
  record[S3G_METRICS_MASKED_PSNR] =
      count > 0.0 ? (psnr_of_mse(acc[3] / count) + psnr_of_mse(acc[4] / count) + psnr_of_mse(acc[5] / count)) / 3.0 : nan;
  record[S3G_METRICS_MASKED_SSIM] = count > 0.0 ? acc[7] / (3.0 * count) : nan;
  record[S3G_METRICS_MASKED_PIXELS] = count;
}

static inline int tiles_x(int W) { return (W + MT_W - 1) / MT_W; }
static inline int tiles_y(int H) { return (H + MT_H - 1) / MT_H; }

}  // namespace s3g

using namespace s3g;

extern "C" size_t s3g_image_metrics_workspace_bytes(int H, int W) {
  if (H <= 0 || W <= 0) return 0;
  const size_t bytes = (size_t)tiles_x(W) * (size_t)tiles_y(H) * MT_PART * sizeof(double);
  return (bytes + 127) & ~size_t(127);
}

extern "C" int s3g_image_metrics(int H, int W, const float* image, const float* gt, const unsigned char* mask, double* record,
                                 float* ssim_map, void* workspace, void* stream_) {
  if (H < 2 * MT_R + 1 || W < 2 * MT_R + 1) {
    set_error("s3g_image_metrics: a %d x %d image is smaller than the 7 x 7 SSIM window", H, W);
    return S3G_ERR_INVALID_ARG;
  }
  if (!image || !gt || !record || !workspace) {
    set_error("s3g_image_metrics: NULL argument");
    return S3G_ERR_INVALID_ARG;
  }
  if ((size_t)tiles_x(W) * (size_t)tiles_y(H) > 0x7fffffffu || tiles_y(H) > 65535) {
    set_error("s3g_image_metrics: a %d x %d image has more tiles than one launch covers", H, W);
    return S3G_ERR_INVALID_ARG;
  }
  const dim3 grid(tiles_x(W), tiles_y(H));
  hipLaunchKernelGGL(image_metrics_tile_kernel, grid, dim3(256), 0, (hipStream_t)stream_, H, W, image, gt, mask, ssim_map,
                     reinterpret_cast<double*>(workspace));
  S3G_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(image_metrics_reduce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream_, H, W, (int)(grid.x * grid.y),
                     reinterpret_cast<const double*>(workspace), record);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}
