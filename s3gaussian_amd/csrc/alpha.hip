// Accumulated-opacity image A = 1 - final_T of a rasterizer forward and the sky-mask loss on it (include/s3g_alpha.h) for gfx950.
// Both are single passes over H*W floats, HBM-bound: the opacity image costs one read and one write per pixel, the loss two reads
// and one write.  The loss sum follows metrics.hip: double partials per workgroup with plain stores, a one-workgroup kernel
// that adds them in a fixed order -- no floating-point atomic, bit-identical run to run.
#include "common.hpp"

#include "../../include/s3g_alpha.h"

namespace s3g {

constexpr int SKY_THREADS = 256;
constexpr int SKY_PER_THREAD = 4;                               // pixels per thread, SKY_THREADS apart (coalesced)
constexpr int SKY_BLOCK_PIXELS = SKY_THREADS * SKY_PER_THREAD;  // 1024 pixels per workgroup

__global__ void __launch_bounds__(256) raster_alpha_kernel(size_t N, const float* __restrict__ final_T, float* __restrict__ out_alpha) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < N) out_alpha[i] = 1.f - final_T[i];   // no contributor: T = 1 exactly, A = 0 exactly
}

// Sum over the workgroup in a fixed order: xor butterfly inside a wave, then wave 0..3 (metrics.hip::block_sum_parts).
__device__ __forceinline__ double block_sum(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ void __launch_bounds__(SKY_THREADS)
sky_loss_pixel_kernel(size_t N, const float* __restrict__ alpha, const float* __restrict__ mask, double grad_scale /* weight / N */,
                      float* __restrict__ out_grad, double* __restrict__ partial) {
  __shared__ double red[4];
  const float lo = (float)1e-6, hi = (float)(1.0 - 1e-6);
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < SKY_PER_THREAD; k++) {
    const size_t i = (size_t)blockIdx.x * SKY_BLOCK_PIXELS + (size_t)k * SKY_THREADS + threadIdx.x;
    if (i >= N) continue;
    const float A = alpha[i];
    const float s = mask[i];
    const float a = fminf(fmaxf(A, lo), hi);
    const float one_m_a = 1.f - a, one_m_s = 1.f - s;
    const float term = -(one_m_s * logf(a)) - s * logf(one_m_a);
    acc += (double)term;
    // torch.clamp passes the gradient where lo <= A <= hi (both ends included) and nowhere else.  Two divisions, a difference
    // and the scale in double, rounded to fp32 once: the stored gradient is within half an ulp of the exact one (in fp32 the
    // rounded scale alone would put a common relative error of up to 6e-8 on every pixel).
    const double d = (A < lo || A > hi) ? 0.0 : ((double)s / (1.0 - (double)a) - (1.0 - (double)s) / (double)a);
    out_grad[i] = (float)(grad_scale * d);
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ void __launch_bounds__(256) sky_loss_reduce_kernel(int nblocks, const double* __restrict__ partial, double scale /* weight / N */,
                                                              int slot, double* __restrict__ total, float* __restrict__ loss) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += 256) acc += partial[b];
  acc = block_sum(acc, red);
  if (threadIdx.x != 0) return;
  const double t = (slot > 0 ? total[0] : 0.0) + scale * acc;
  total[0] = t;
  loss[0] = (float)t;
}

static inline size_t sky_blocks(size_t N) { return (N + SKY_BLOCK_PIXELS - 1) / SKY_BLOCK_PIXELS; }

}  // namespace s3g

using namespace s3g;

extern "C" int s3g_raster_alpha(int width, int height, const void* image_arena, float* out_alpha, void* stream_) {
  clear_error();
  if (width <= 0 || height <= 0 || !image_arena || !out_alpha) {
    set_error("s3g_raster_alpha: bad argument (needs the image arena of a forward and a [1,H,W] output)");
    return S3G_ERR_INVALID_ARG;
  }
  const size_t N = (size_t)width * (size_t)height;
  if ((N + 255) / 256 > 0x7fffffffu) {
    set_error("s3g_raster_alpha: a %d x %d image has more pixels than one launch covers", width, height);
    return S3G_ERR_INVALID_ARG;
  }
  // ImageState::carve (raster_dev.hpp) takes final_T first: the arena starts with its H*W floats
  hipLaunchKernelGGL(raster_alpha_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, N,
                     reinterpret_cast<const float*>(image_arena), out_alpha);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" size_t s3g_sky_loss_workspace_bytes(int width, int height) {
  if (width <= 0 || height <= 0) return 0;
  const size_t bytes = sky_blocks((size_t)width * (size_t)height) * sizeof(double);
  return (bytes + 127) & ~size_t(127);
}

extern "C" int s3g_sky_loss(int width, int height, const float* alpha, const float* mask, float weight, int slot, float* out_grad,
                            double* total, float* loss, void* workspace, void* stream_) {
  clear_error();
  if (width <= 0 || height <= 0 || !alpha || !mask || !out_grad || !total || !loss || !workspace || slot < 0) {
    set_error("s3g_sky_loss: bad argument (NULL array, empty image or negative slot)");
    return S3G_ERR_INVALID_ARG;
  }
  const size_t N = (size_t)width * (size_t)height;
  const size_t nb = sky_blocks(N);
  if (nb > 0x7fffffffu) {
    set_error("s3g_sky_loss: a %d x %d image has more pixels than one launch covers", width, height);
    return S3G_ERR_INVALID_ARG;
  }
  hipStream_t stream = (hipStream_t)stream_;
  double* partial = reinterpret_cast<double*>(workspace);
  const double scale = (double)weight / (double)N;
  hipLaunchKernelGGL(sky_loss_pixel_kernel, dim3((unsigned)nb), dim3(SKY_THREADS), 0, stream, N, alpha, mask, scale, out_grad,
                     partial);
  S3G_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(sky_loss_reduce_kernel, dim3(1), dim3(256), 0, stream, (int)nb, partial, scale, slot, total, loss);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}
