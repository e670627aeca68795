// Device code the two LPIPS variants share (lpips.hip: AlexNet, lpips_vgg.hip: VGG16): the z-score constants, the tap kernel and the
// record layout of the finalise.  Both variants store activations [image][H][W][C], channels innermost, both images in one buffer.
// lpips_conv.hpp, which both include, adds the layer description, the conv and pool kernels and the launch helpers on top of this.
#pragma once
#include "common.hpp"

#include "../../include/s3g_lpips.h"

namespace s3g {

constexpr int LP_LAYERS = 5;         // taps of either variant
constexpr int LP_TAP_PIXELS = 8;     // pixels per wave of the tap kernel (32 per workgroup)

typedef float lp_f32x16 __attribute__((ext_vector_type(16)));

// networks.py:41-44: the z-score constants are fp32 tensors
__device__ __forceinline__ float lp_zscore(float v, int c) {
  const float mean = c == 0 ? -.030f : (c == 1 ? -.088f : -.188f);
  const float sd = c == 0 ? .458f : (c == 1 ? .448f : .450f);
  return (v - mean) / sd;
}

__device__ __forceinline__ float lp_wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// act: [2][npix][C].  partial[blockIdx.x] = sum over this workgroup's 32 pixels of sum_c w_c (a^x_c - a^y_c)^2.
template <int C>
__global__ void __launch_bounds__(256) lpips_tap_kernel(int npix, const float* __restrict__ act, const float* __restrict__ lin,
                                                        double* __restrict__ partial) {
  constexpr int J = C / WAVE;
  static_assert(C % WAVE == 0, "whole channel rounds per wave");
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float w[J];
#pragma unroll
  for (int j = 0; j < J; j++) w[j] = lin[j * WAVE + lane];
  double wsum = 0.0;
  for (int i = 0; i < LP_TAP_PIXELS; i++) {
    const int pix = (blockIdx.x * 4 + wave) * LP_TAP_PIXELS + i;
    if (pix >= npix) break;   // uniform over the wave
    const float* px = act + (size_t)pix * C + lane;
    const float* py = act + ((size_t)npix + pix) * C + lane;
    float ax[J], ay[J], sx = 0.f, sy = 0.f;
#pragma unroll
    for (int j = 0; j < J; j++) {
      ax[j] = px[j * WAVE];
      ay[j] = py[j * WAVE];
      sx += ax[j] * ax[j];
      sy += ay[j] * ay[j];
    }
    const float nx = sqrtf(lp_wave_sum(sx)) + 1e-10f, ny = sqrtf(lp_wave_sum(sy)) + 1e-10f;   // utils.py:6-8: eps outside the root
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < J; j++) {
      const float d = ax[j] / nx - ay[j] / ny;
      acc += w[j] * (d * d);
    }
    wsum += (double)lp_wave_sum(acc);
  }
  if (lane == 0) red[wave] = wsum;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

static inline int tap_blocks(int npix) { return (npix + 4 * LP_TAP_PIXELS - 1) / (4 * LP_TAP_PIXELS); }

struct LpFinal {
  const double* partial[LP_LAYERS];
  int nparts[LP_LAYERS];
  int npix[LP_LAYERS];
};

// ---- host functions that cross files (a __global__ function is launched only from the file that defines it; both in lpips.hip) -----
// one workgroup adds every tap's partials in a fixed order, divides by the tap's pixel count, writes {total, tap0..tap4}
void lpips_launch_finalize(const LpFinal& f, double* record, hipStream_t stream);
// OIHW -> B [KPAD][CO], K ordered (kh, kw, ci), rows K..KPAD-1 zero
void lpips_launch_pack(int KS, int CI, int CO, int K, int KPAD, const float* w, float* B, hipStream_t stream);

}  // namespace s3g
