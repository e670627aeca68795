// Densification statistics as passes of their own (include/s3g_optim.h; train.py:489-493, scene/gaussian_model.py:693-695):
// xyz_gradient_accum += ||viewspace gradient||, denom += 1, max_radii2D = max(max_radii2D, radii) where a Gaussian was visible,
// for one view or for a batch of views.  The rasterizer's geometry backward does the one-view update fused
// (raster_geom_backward.hip, s3g_raster_backward*_accum); these kernels serve gradients that were accumulated or all-reduced first.
#include "common.hpp"

#include "../../include/s3g_optim.h"

namespace s3g {

__global__ void __launch_bounds__(256) densify_stats_kernel(int P, const float* __restrict__ g, int stride,
                                                            const int* __restrict__ radii, const unsigned char* __restrict__ visible,
                                                            float* __restrict__ accum, float* __restrict__ denom,
                                                            float* __restrict__ max_radii, const uint32_t* __restrict__ skip) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  if (skip && *skip != 0u) return;   // the view's asynchronous forward overflowed: its statistics do not exist (uniform load)
  const int r = radii[i];
  if (!(visible ? visible[i] != 0 : r > 0)) return;
  const float gx = g[(size_t)i * stride], gy = g[(size_t)i * stride + 1];
  accum[i] += sqrtf(gx * gx + gy * gy);
  denom[i] += 1.f;
  max_radii[i] = fmaxf(max_radii[i], (float)r);
}

// Densification statistics of a batch of views (train.py:387-388, 435-437, 489-493): the viewspace gradients are summed first
// (left to right) and the norm is taken of the sum; a Gaussian counts once if any view saw it; the radius is the largest.
struct StatsViewsArgs {
  int P, V, stride;
  const float* grad[S3G_DENSIFY_MAX_VIEWS];
  const int* radii[S3G_DENSIFY_MAX_VIEWS];
  float *accum, *denom, *max_radii;
  const uint32_t* skip;
};

__global__ void __launch_bounds__(256) densify_stats_views_kernel(const StatsViewsArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.P) return;
  if (a.skip && *a.skip != 0u) return;   // a forward of the batch overflowed: the batch's statistics do not exist (uniform load)
  int r = a.radii[0][i];
  bool vis = r > 0;
  float gx = a.grad[0][(size_t)i * a.stride], gy = a.grad[0][(size_t)i * a.stride + 1];
  for (int v = 1; v < a.V; v++) {
    const int rv = a.radii[v][i];
    vis = vis || rv > 0;
    r = max(r, rv);
    gx = gx + a.grad[v][(size_t)i * a.stride];
    gy = gy + a.grad[v][(size_t)i * a.stride + 1];
  }
  if (!vis) return;
  a.accum[i] += sqrtf(gx * gx + gy * gy);
  a.denom[i] += 1.f;
  a.max_radii[i] = fmaxf(a.max_radii[i], (float)r);
}

}  // namespace s3g

using namespace s3g;

static int densify_stats_impl(int P, const float* grad_xy, int grad_stride, const int* radii, const unsigned char* visible,
                              float* xyz_gradient_accum, float* denom, float* max_radii2D, const uint32_t* skip, void* stream_) {
  if (P < 0 || grad_stride < 2 || (P > 0 && (!grad_xy || !radii || !xyz_gradient_accum || !denom || !max_radii2D))) {
    set_error("s3g_densify_stats: bad argument");
    return S3G_ERR_INVALID_ARG;
  }
  if (P == 0) return S3G_OK;
  hipLaunchKernelGGL(densify_stats_kernel, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream_, P, grad_xy, grad_stride,
                     radii, visible, xyz_gradient_accum, denom, max_radii2D, skip);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" int s3g_densify_stats(int P, const float* grad_xy, int grad_stride, const int* radii, const unsigned char* visible,
                                 float* xyz_gradient_accum, float* denom, float* max_radii2D, void* stream_) {
  return densify_stats_impl(P, grad_xy, grad_stride, radii, visible, xyz_gradient_accum, denom, max_radii2D, nullptr, stream_);
}
extern "C" int s3g_densify_stats_guarded(int P, const float* grad_xy, int grad_stride, const int* radii, const unsigned char* visible,
                                         float* xyz_gradient_accum, float* denom, float* max_radii2D, const uint32_t* skip_flag,
                                         void* stream_) {
  return densify_stats_impl(P, grad_xy, grad_stride, radii, visible, xyz_gradient_accum, denom, max_radii2D, skip_flag, stream_);
}

static int densify_stats_views_impl(int P, int V, const float* const* grad_xy, int grad_stride, const int* const* radii,
                                    float* xyz_gradient_accum, float* denom, float* max_radii2D, const uint32_t* skip, void* stream_) {
  bool ok = P >= 0 && V >= 1 && V <= S3G_DENSIFY_MAX_VIEWS && grad_stride >= 2 && grad_xy != nullptr && radii != nullptr;
  if (ok && P > 0) {
    ok = xyz_gradient_accum && denom && max_radii2D;
    for (int v = 0; ok && v < V; v++) ok = grad_xy[v] != nullptr && radii[v] != nullptr;
  }
  if (!ok) {
    set_error("s3g_densify_stats_views: bad argument (1 <= V <= %d)", S3G_DENSIFY_MAX_VIEWS);
    return S3G_ERR_INVALID_ARG;
  }
  if (P == 0) return S3G_OK;
  StatsViewsArgs a;
  memset(&a, 0, sizeof a);
  a.P = P; a.V = V; a.stride = grad_stride;
  for (int v = 0; v < V; v++) { a.grad[v] = grad_xy[v]; a.radii[v] = radii[v]; }
  a.accum = xyz_gradient_accum; a.denom = denom; a.max_radii = max_radii2D; a.skip = skip;
  hipLaunchKernelGGL(densify_stats_views_kernel, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream_, a);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" int s3g_densify_stats_views(int P, int V, const float* const* grad_xy, int grad_stride, const int* const* radii,
                                       float* xyz_gradient_accum, float* denom, float* max_radii2D, void* stream_) {
  return densify_stats_views_impl(P, V, grad_xy, grad_stride, radii, xyz_gradient_accum, denom, max_radii2D, nullptr, stream_);
}
extern "C" int s3g_densify_stats_views_guarded(int P, int V, const float* const* grad_xy, int grad_stride, const int* const* radii,
                                               float* xyz_gradient_accum, float* denom, float* max_radii2D,
                                               const uint32_t* skip_flag, void* stream_) {
  return densify_stats_views_impl(P, V, grad_xy, grad_stride, radii, xyz_gradient_accum, denom, max_radii2D, skip_flag, stream_);
}
