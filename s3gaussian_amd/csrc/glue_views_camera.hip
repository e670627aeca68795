// Per-view camera-centre gradients of the shared glue backward (include/s3g_glue.h::s3g_glue_backward_views_campos) for gfx950.
//
// The colours of view v depend on xyz - campos_v only, so dL/dcampos_v = -sum_p t_v[p], t_v the direction term of view v that
// glue_backward_views_kernel forms in registers and adds into g_xyz.  Its TV instantiations (glue_views.hip) also store each t_v
// to a [P,3] fp32 array; the two kernels here sum those arrays over P.
//
// The order of the sum is camera_backward_kernel's and camera_fold_kernel's for their g_dir term (raster_camera_backward.hip),
// statement by statement: cam_blocks(P) workgroups of CAM_THREADS striding over P, a double accumulator per thread that takes
// 0.0 - (double)t, the xor butterfly inside a wave, waves 0..3 in order, one plain-stored partial per workgroup, then 32 groups
// that each add every 32nd partial and are added in order.  A single-camera glue backward followed by s3g_camera_backward on its
// g_xyz -- the route of glue.activations_and_colors -- therefore gives the same three doubles, bit for bit.  grid.y = view: V
// cameras take one launch each of the two kernels.  No floating-point atomics.
#include "camera_sum.hpp"
#include "glue_dev.hpp"

#include "../../include/s3g_glue.h"

namespace s3g {

struct GlueCamposArgs {
  int P;
  const float* tv[S3G_GLUE_MAX_VIEWS];   // [P,3] each
  double* partial;                       // [V][gridDim.x][3]
};

__global__ void __launch_bounds__(CAM_THREADS) glue_views_campos_sum_kernel(const GlueCamposArgs a) {
  __shared__ double red[4][3];
  const float* __restrict__ t = a.tv[blockIdx.y];
  double acc[3] = {0.0, 0.0, 0.0};
  for (long long base = (long long)blockIdx.x * CAM_THREADS; base < a.P; base += (long long)gridDim.x * CAM_THREADS) {
    const long long idx = base + threadIdx.x;
    if (idx >= a.P) continue;
    const size_t i3 = 3 * (size_t)idx;
    double tc[3] = {0.0, 0.0, 0.0};
    tc[0] -= (double)t[i3];
    tc[1] -= (double)t[i3 + 1];
    tc[2] -= (double)t[i3 + 2];
#pragma unroll
    for (int s = 0; s < 3; s++) acc[s] += tc[s];
  }
#pragma unroll
  for (int s = 0; s < 3; s++) {
    double v = acc[s];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][s] = v;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int s = threadIdx.x;
    a.partial[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3 + s] = ((red[0][s] + red[1][s]) + red[2][s]) + red[3][s];
  }
}

// One workgroup per view, 32 groups of 4 lanes (lane = component, the fourth idle): group q adds the partials of workgroups q,
// q + 32, ... -- at most 16 --, then lane s of group 0 adds the 32 group sums in order.
constexpr int GLUE_CAMPOS_FOLD_THREADS = 128;

__global__ void __launch_bounds__(GLUE_CAMPOS_FOLD_THREADS) glue_views_campos_fold_kernel(int nblocks, const double* __restrict__ partial,
                                                                                          double* __restrict__ g_campos) {
  __shared__ double red[32][3];
  const int s = threadIdx.x & 3, q = threadIdx.x >> 2;
  const double* __restrict__ part = partial + (size_t)blockIdx.x * nblocks * 3;
  if (s < 3) {
    double acc = 0.0;
#pragma unroll 4
    for (int b = q; b < nblocks; b += 32) acc += part[(size_t)b * 3 + s];
    red[q][s] = acc;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int t = threadIdx.x;
    double v = red[0][t];
#pragma unroll
    for (int g = 1; g < 32; g++) v += red[g][t];
    g_campos[3 * (size_t)blockIdx.x + t] = v;
  }
}

}  // namespace s3g

using namespace s3g;

extern "C" size_t s3g_glue_backward_views_campos_workspace_bytes(int P, int V) {
  if (P <= 0 || V <= 0) return 0;
  return ((size_t)V * cam_blocks(P) * 3 * sizeof(double) + 127) & ~size_t(127);
}

extern "C" int s3g_glue_backward_views_campos(int P, int deg, int V, const float* f_dc, const float* f_rest, const float* dshs,
                                              const float* xyz, const float* campos, const float* rot_raw,
                                              const float* const* colors, const float* scales, const float* rot, const float* opacity,
                                              const float* const* g_colors, const float* g_scales, const float* g_rot,
                                              const float* g_opacity, float* g_f_dc, float* g_f_rest, float* g_dshs, float* g_xyz,
                                              float* g_log_scales, float* g_rot_raw, float* g_opacity_logit, const float* g_dshs_l1,
                                              float* const* tv, void* workspace, double* g_campos, void* stream_) {
  const char* who = "s3g_glue_backward_views_campos";
  if (tv == nullptr || g_campos == nullptr || (P > 0 && workspace == nullptr)) {
    set_error("%s: NULL scratch array, workspace or output", who);
    return S3G_ERR_INVALID_ARG;
  }
  const int code = glue_backward_views_launch(who, P, deg, V, f_dc, f_rest, dshs, xyz, campos, rot_raw, colors, scales, rot, opacity,
                                              g_colors, g_scales, g_rot, g_opacity, g_f_dc, g_f_rest, g_dshs, g_xyz, g_log_scales,
                                              g_rot_raw, g_opacity_logit, g_dshs_l1, tv, stream_);
  if (code != S3G_OK) return code;
  hipStream_t st = (hipStream_t)stream_;
  if (P == 0) {
    S3G_HIP_CHECK(hipMemsetAsync(g_campos, 0, (size_t)V * 3 * sizeof(double), st));
    return S3G_OK;
  }
  GlueCamposArgs a;
  memset(&a, 0, sizeof a);
  a.P = P;
  for (int v = 0; v < V; v++) a.tv[v] = tv[v];
  a.partial = reinterpret_cast<double*>(workspace);
  const int nb = cam_blocks(P);
  hipLaunchKernelGGL(glue_views_campos_sum_kernel, dim3(nb, V), dim3(CAM_THREADS), 0, st, a);
  S3G_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(glue_views_campos_fold_kernel, dim3(V), dim3(GLUE_CAMPOS_FOLD_THREADS), 0, st, nb, a.partial, g_campos);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}
