// Scene-flow colours for gfx950: scene_flow_to_rgb(dx_b - dx_a, background="bright", flow_max_radius=1.0) of the reference
// (utils/visualization_tools.py:242-322, called per frame by utils/video_utils.py:252-299 through a host round trip).
// Two launches, no float atomics: a min / max reduction that leaves one pair per workgroup, and a per-Gaussian pass that folds the
// pairs in its prologue.  Why the colour wheel needs no table here: include/s3g_flow.h.
#include "common.hpp"

#include "../../include/s3g_flow.h"

namespace s3g {

constexpr int FLOW_THREADS = 256;
constexpr int FLOW_RANGE_BLOCKS = 512;     // partial pairs at most: the colour pass folds two per thread in its prologue
constexpr int FLOW_COLOR_BLOCKS = 2048;    // 256 CUs x 8 workgroups, the rest by grid stride
constexpr int FLOW_RANGE_PER_BLOCK = FLOW_THREADS * 4 * 4;   // floats one workgroup is sized for: four 16-byte loads per lane

static inline int range_blocks(int P) {
  const size_t n = 3 * (size_t)P;
  const size_t nb = (n + FLOW_RANGE_PER_BLOCK - 1) / FLOW_RANGE_PER_BLOCK;
  return nb < 1 ? 1 : (nb > (size_t)FLOW_RANGE_BLOCKS ? FLOW_RANGE_BLOCKS : (int)nb);
}

// (min, max) over the workgroup, valid in every thread: xor butterfly inside a wave, then the four waves through LDS.
__device__ __forceinline__ void block_min_max(float& mn, float& mx, float (*red)[2]) {
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o));
    mx = fmaxf(mx, __shfl_xor(mx, o));
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = mn;
    red[threadIdx.x >> 6][1] = mx;
  }
  __syncthreads();
  mn = fminf(fminf(red[0][0], red[1][0]), fminf(red[2][0], red[3][0]));
  mx = fmaxf(fmaxf(red[0][1], red[1][1]), fmaxf(red[2][1], red[3][1]));
}

// Pass 1.  n = 3P floats.  VEC: both pointers are 16-byte aligned, the first n / 4 float4 go through 16-byte loads and the last
// n % 4 floats through the scalar tail; otherwise (a view that starts inside an allocation) every float is a scalar load.
template <bool VEC>
__global__ void __launch_bounds__(FLOW_THREADS) flow_range_kernel(size_t n, const float* __restrict__ a, const float* __restrict__ b,
                                                                  float2* __restrict__ partial) {
  __shared__ float red[4][2];
  float mn = __builtin_inff(), mx = -__builtin_inff();
  const size_t tid = (size_t)blockIdx.x * FLOW_THREADS + threadIdx.x, stride = (size_t)gridDim.x * FLOW_THREADS;
  size_t done = 0;
  if (VEC) {
    const size_t n4 = n / 4;
    const float4* __restrict__ a4 = reinterpret_cast<const float4*>(a);
    const float4* __restrict__ b4 = reinterpret_cast<const float4*>(b);
    for (size_t i = tid; i < n4; i += stride) {
      const float4 u = a4[i], v = b4[i];
      const float d0 = v.x - u.x, d1 = v.y - u.y, d2 = v.z - u.z, d3 = v.w - u.w;
      mn = fminf(fminf(mn, d0), fminf(fminf(d1, d2), d3));
      mx = fmaxf(fmaxf(mx, d0), fmaxf(fmaxf(d1, d2), d3));
    }
    done = n4 * 4;
  }
  for (size_t i = done + tid; i < n; i += stride) {
    const float d = b[i] - a[i];
    mn = fminf(mn, d);
    mx = fmaxf(mx, d);
  }
  block_min_max(mn, mx, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = make_float2(mn, mx);
}

// Pass 2: one Gaussian per lane and trip.  Steps 1-4 of include/s3g_flow.h in the reference's order of fp32 operations (the
// library is built with -ffp-contract=off: nothing below fuses into an fma).
__global__ void __launch_bounds__(FLOW_THREADS) flow_color_kernel(int P, int npartial, const float* __restrict__ a,
                                                                  const float* __restrict__ b, const float2* __restrict__ partial,
                                                                  float* __restrict__ colors, float* __restrict__ range) {
  __shared__ float red[4][2];
  float mn = __builtin_inff(), mx = -__builtin_inff();
  for (int k = threadIdx.x; k < npartial; k += FLOW_THREADS) {
    const float2 p = partial[k];
    mn = fminf(mn, p.x);
    mx = fmaxf(mx, p.y);
  }
  block_min_max(mn, mx, red);
  if (range != nullptr && blockIdx.x == 0 && threadIdx.x == 0) {
    range[0] = mn;
    range[1] = mx;
  }
  const float span = (mx - mn) + 1e-6f;
  const float per_radian = (float)(54.0 / (2.0 * 3.14159265358979323846));   // (N_COLS - 1) / (2 pi), rounded to fp32 like the reference's scalar
  for (size_t i = (size_t)blockIdx.x * FLOW_THREADS + threadIdx.x; i < (size_t)P; i += (size_t)gridDim.x * FLOW_THREADS) {
    const size_t o = 3 * i;
    const float x = ((b[o] - a[o]) - mn) / span, y = ((b[o + 1] - a[o + 1]) - mn) / span;
    // |x + iy| and angle(x + iy), evaluated in double and rounded to fp32 once: the distance from the reference's fp32 hypot / atan2
    // is then that library's own last-bit error, not the sum of two (the kernel is memory-bound: the double ops are hidden).
    // x, y >= 0: the reference's "+ 2 pi below zero" never applies.
    const double xd = (double)x, yd = (double)y;
    const float r = (float)sqrt(xd * xd + yd * yd);
    const float A = (float)atan2(yd, xd) * per_radian;
    // wheel entries trunc(A) and ceil(A) on the red -> yellow transition are (255, 17 k, 0); fmod(A, 1) = A - trunc(A) for A >= 0
    const float lo = truncf(A), hi = ceilf(A), frac = A - lo;
    const float g = (17.0f * lo) * (1.0f - frac) + (17.0f * hi) * frac;
    float cr, cg, cb;
    if (r > 1.0f) {                                     // hue * (1 / r)
      const float inv = 1.0f / r;
      cr = 255.0f * inv;
      cg = g * inv;
      cb = 0.0f * inv;
    } else {                                            // 255 - r * (255 - hue)
      cr = 255.0f - r * (255.0f - 255.0f);
      cg = 255.0f - r * (255.0f - g);
      cb = 255.0f - r * (255.0f - 0.0f);
    }
    colors[o] = cr / 255.0f;
    colors[o + 1] = cg / 255.0f;
    colors[o + 2] = cb / 255.0f;
  }
}

}  // namespace s3g

using namespace s3g;

extern "C" size_t s3g_scene_flow_workspace_bytes(int P) {
  if (P <= 0) return 0;
  return ((size_t)range_blocks(P) * sizeof(float2) + 127) & ~size_t(127);
}

extern "C" int s3g_scene_flow_colors(int P, const float* dx_a, const float* dx_b, float* colors, float* range, void* workspace,
                                     void* stream_) {
  if (P < 0) {
    set_error("s3g_scene_flow_colors: P = %d", P);
    return S3G_ERR_INVALID_ARG;
  }
  if (P == 0) return S3G_OK;
  if (!dx_a || !dx_b || !colors || !workspace) {
    set_error("s3g_scene_flow_colors: NULL argument");
    return S3G_ERR_INVALID_ARG;
  }
  const hipStream_t stream = (hipStream_t)stream_;
  const size_t n = 3 * (size_t)P;
  const int nb = range_blocks(P);
  float2* partial = reinterpret_cast<float2*>(workspace);
  const bool aligned = ((reinterpret_cast<uintptr_t>(dx_a) | reinterpret_cast<uintptr_t>(dx_b)) & 15) == 0;
  if (aligned)
    hipLaunchKernelGGL(flow_range_kernel<true>, dim3(nb), dim3(FLOW_THREADS), 0, stream, n, dx_a, dx_b, partial);
  else
    hipLaunchKernelGGL(flow_range_kernel<false>, dim3(nb), dim3(FLOW_THREADS), 0, stream, n, dx_a, dx_b, partial);
  S3G_HIP_CHECK(hipGetLastError());
  const size_t want = ((size_t)P + FLOW_THREADS - 1) / FLOW_THREADS;
  const int grid = want > (size_t)FLOW_COLOR_BLOCKS ? FLOW_COLOR_BLOCKS : (int)want;
  hipLaunchKernelGGL(flow_color_kernel, dim3(grid), dim3(FLOW_THREADS), 0, stream, P, nb, dx_a, dx_b, partial, colors, range);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}
