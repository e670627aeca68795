// Render glue for V cameras that share one timestamp (a Waymo rig delivers three): the deformed coefficients, the activations
// and their gradients do not depend on the camera, only the view direction does.  One kernel each way reads f_dc / f_rest / dshs
// once per Gaussian (421 B) and serves V cameras: V x 12 B of colours forward, V x 24 B backward, against V x ~440 B for V calls
// of glue.hip.  Arithmetic per camera is glue.hip's, from the same source (glue_dev.hpp): colours are bit-identical to a
// single-camera call, and with V = 1 so is every gradient.
#include "glue_dev.hpp"

#include "../../include/s3g_glue.h"
#include "../../include/s3g_loss.h"  // S3G_SUM_* (slotted accumulators)

namespace s3g {

struct GlueViewsArgs {
  GlueArgs g;   // campos: [V,3]; colors / g_colors unused (per camera below)
  int V;
  float* colors[S3G_GLUE_MAX_VIEWS];           // forward: written; backward: read
  const float* g_colors[S3G_GLUE_MAX_VIEWS];   // backward; an entry may be null (zero)
  float* tv[S3G_GLUE_MAX_VIEWS];               // backward, TV instantiations only: each view's own direction term, [P,3]
};

__device__ __forceinline__ void glue_forward_views_point(const GlueViewsArgs& a, int p, const float (&sh)[16][3]) {
  glue_activations_point(a.g, p);
  for (int v = 0; v < a.V; v++) glue_colors_point(a.g, p, sh, a.g.campos + 3 * v, a.colors[v]);
}

// dshs present: glue_forward_kernel's coalesced staging (glue_dev.hpp), then the V polynomials from the same 48 registers
__global__ void __launch_bounds__(256) glue_forward_views_kernel(const GlueViewsArgs a) {
  __shared__ float rows[256 * GLUE_ROW];
  __shared__ double part[4];
  const int p0 = blockIdx.x * 256, p = p0 + threadIdx.x, nrows = min(256, a.g.P - p0);
  const float s = nrows == 256 ? glue_stage_rows<true>(a.g, p0, nrows, rows) : glue_stage_rows<false>(a.g, p0, nrows, rows);
  if (a.g.dshs_abs_sum != nullptr) {
    double t = (double)s;
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = t;
  }
  __syncthreads();
  if (a.g.dshs_abs_sum != nullptr && threadIdx.x == 0)
    atomicAdd(&a.g.dshs_abs_sum[(blockIdx.x % S3G_SUM_SLOTS) * S3G_SUM_STRIDE], part[0] + part[1] + part[2] + part[3]);
  if (p >= a.g.P) return;
  float sh[16][3];
#pragma unroll
  for (int k = 0; k < 16; k++)
#pragma unroll
    for (int c = 0; c < 3; c++) sh[k][c] = rows[threadIdx.x * GLUE_ROW + 3 * k + c];
  glue_forward_views_point(a, p, sh);
}

__global__ void __launch_bounds__(256) glue_forward_views_rows_kernel(const GlueViewsArgs a) {   // no dshs (coarse stage)
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= a.g.P) return;
  float sh[16][3];
  load_sh(a.g, p, sh);
  glue_forward_views_point(a, p, sh);
}

// The two halves of glue.hip's glue_backward_point, same statements in the same order (why that function is not built from them:
// glue_dev.hpp).  thread = Gaussian: gradients of the three activations (they do not depend on the camera)
__device__ __forceinline__ void glue_backward_activations_point(const GlueArgs& a, int p) {
#pragma unroll
  for (int k = 0; k < 3; k++)
    a.g_log_scales[3 * (size_t)p + k] = a.g_scales ? a.g_scales[3 * (size_t)p + k] * a.scales[3 * (size_t)p + k] : 0.f;
  {
    const float4 q = reinterpret_cast<const float4*>(a.rot_raw)[p];
    const float nrm = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    float4 gq = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.g_rot) {
      const float4 g = reinterpret_cast<const float4*>(a.g_rot)[p];
      if (nrm > 1e-12f) {  // d(x/n) = (g - y (y.g)) / n
        const float4 yv = reinterpret_cast<const float4*>(a.rot)[p];
        const float dot = yv.x * g.x + yv.y * g.y + yv.z * g.z + yv.w * g.w;
        gq = make_float4((g.x - yv.x * dot) / nrm, (g.y - yv.y * dot) / nrm, (g.z - yv.z * dot) / nrm, (g.w - yv.w * dot) / nrm);
      } else {
        gq = make_float4(g.x / 1e-12f, g.y / 1e-12f, g.z / 1e-12f, g.w / 1e-12f);
      }
    }
    reinterpret_cast<float4*>(a.g_rot_raw)[p] = gq;
  }
  {
    const float o = a.opacity[p];
    a.g_opacity_logit[p] = a.g_opacity ? a.g_opacity[p] * o * (1.f - o) : 0.f;
  }
}

// thread = Gaussian, one camera: SH backward (same derivation as backward.cu:20-139, coefficients split over f_dc / f_rest /
// dshs).  The 16 basis values and the 3 clamped colour gradients go to stage[19]; this camera's direction term of g_xyz goes to
// gx[3], which the caller sums over its cameras.
__device__ __forceinline__ void glue_backward_sh_point(const GlueArgs& a, int p, const float (&sh)[16][3], const float* campos,
                                                       const float* colors, const float* g_colors, float* stage, float (&gx)[3]) {
  float dRGB[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float g = g_colors ? g_colors[3 * (size_t)p + c] : 0.f;
    dRGB[c] = colors[3 * (size_t)p + c] > 0.f ? g : 0.f;  // clamp_min(., 0): zero gradient where the clamp is active
  }
  const float ox = a.xyz[3 * (size_t)p] - campos[0], oy = a.xyz[3 * (size_t)p + 1] - campos[1], oz = a.xyz[3 * (size_t)p + 2] - campos[2];
  const float len = sqrtf(ox * ox + oy * oy + oz * oz);
  const float x = ox / len, y = oy / len, z = oz / len;
  const int deg = a.deg;
  float dsh[16], dRdx[3] = {0.f, 0.f, 0.f}, dRdy[3] = {0.f, 0.f, 0.f}, dRdz[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 16; k++) dsh[k] = 0.f;
  dsh[0] = SH_C0;
  if (deg > 0) {
    dsh[1] = -SH_C1 * y; dsh[2] = SH_C1 * z; dsh[3] = -SH_C1 * x;
#pragma unroll
    for (int c = 0; c < 3; c++) { dRdx[c] = -SH_C1 * sh[3][c]; dRdy[c] = -SH_C1 * sh[1][c]; dRdz[c] = SH_C1 * sh[2][c]; }
    if (deg > 1) {
      const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
      dsh[4] = SH_C2[0] * xy; dsh[5] = SH_C2[1] * yz; dsh[6] = SH_C2[2] * (2.f * zz - xx - yy);
      dsh[7] = SH_C2[3] * xz; dsh[8] = SH_C2[4] * (xx - yy);
#pragma unroll
      for (int c = 0; c < 3; c++) {
        dRdx[c] += SH_C2[0] * y * sh[4][c] + SH_C2[2] * 2.f * -x * sh[6][c] + SH_C2[3] * z * sh[7][c] + SH_C2[4] * 2.f * x * sh[8][c];
        dRdy[c] += SH_C2[0] * x * sh[4][c] + SH_C2[1] * z * sh[5][c] + SH_C2[2] * 2.f * -y * sh[6][c] + SH_C2[4] * 2.f * -y * sh[8][c];
        dRdz[c] += SH_C2[1] * y * sh[5][c] + SH_C2[2] * 2.f * 2.f * z * sh[6][c] + SH_C2[3] * x * sh[7][c];
      }
      if (deg > 2) {
        dsh[9] = SH_C3[0] * y * (3.f * xx - yy); dsh[10] = SH_C3[1] * xy * z; dsh[11] = SH_C3[2] * y * (4.f * zz - xx - yy);
        dsh[12] = SH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy); dsh[13] = SH_C3[4] * x * (4.f * zz - xx - yy);
        dsh[14] = SH_C3[5] * z * (xx - yy); dsh[15] = SH_C3[6] * x * (xx - 3.f * yy);
#pragma unroll
        for (int c = 0; c < 3; c++) {
          dRdx[c] += (SH_C3[0] * sh[9][c] * 3.f * 2.f * xy + SH_C3[1] * sh[10][c] * yz + SH_C3[2] * sh[11][c] * -2.f * xy +
                      SH_C3[3] * sh[12][c] * -3.f * 2.f * xz + SH_C3[4] * sh[13][c] * (-3.f * xx + 4.f * zz - yy) +
                      SH_C3[5] * sh[14][c] * 2.f * xz + SH_C3[6] * sh[15][c] * 3.f * (xx - yy));
          dRdy[c] += (SH_C3[0] * sh[9][c] * 3.f * (xx - yy) + SH_C3[1] * sh[10][c] * xz + SH_C3[2] * sh[11][c] * (-3.f * yy + 4.f * zz - xx) +
                      SH_C3[3] * sh[12][c] * -3.f * 2.f * yz + SH_C3[4] * sh[13][c] * -2.f * xy + SH_C3[5] * sh[14][c] * -2.f * yz +
                      SH_C3[6] * sh[15][c] * -3.f * 2.f * xy);
          dRdz[c] += (SH_C3[1] * sh[10][c] * xy + SH_C3[2] * sh[11][c] * 4.f * 2.f * yz + SH_C3[3] * sh[12][c] * 3.f * (2.f * zz - xx - yy) +
                      SH_C3[4] * sh[13][c] * 4.f * 2.f * xz + SH_C3[5] * sh[14][c] * (xx - yy));
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 16; k++) stage[k] = dsh[k];
#pragma unroll
  for (int c = 0; c < 3; c++) stage[16 + c] = dRGB[c];
  const float ddx = dRdx[0] * dRGB[0] + dRdx[1] * dRGB[1] + dRdx[2] * dRGB[2];
  const float ddy = dRdy[0] * dRGB[0] + dRdy[1] * dRGB[1] + dRdy[2] * dRGB[2];
  const float ddz = dRdz[0] * dRGB[0] + dRdz[1] * dRGB[1] + dRdz[2] * dRGB[2];
  const float sum2 = ox * ox + oy * oy + oz * oz;
  const float inv = 1.0f / sqrtf(sum2 * sum2 * sum2);  // d normalize(v)/dv, auxiliary.h:107-117
  gx[0] = ((sum2 - ox * ox) * ddx - oy * ox * ddy - oz * ox * ddz) * inv;
  gx[1] = (-ox * oy * ddx + (sum2 - oy * oy) * ddy - oz * oy * ddz) * inv;
  gx[2] = (-ox * oz * ddx - oy * oz * ddy + (sum2 - oz * oz) * ddz) * inv;
}

// Backward.  Phase 1 (thread = Gaussian): activation gradients once, coefficient rows loaded once, then per camera the 16 basis
// values and 3 clamped colour gradients into LDS and the direction term of g_xyz into registers, summed view 0 first.  Phase 2
// (workgroup, coalesced): a coefficient gradient is sum_v basis_v[k] * dRGB_v[c], each product rounded on its own and added left
// to right (the build has -ffp-contract=off and nothing here asks for an FMA), so the result is the fp32 sum of V single-camera
// calls; the sign term of mean|dshs| comes last.  The stage is [V][R][19] floats; glue.hip's 256 rows times 8 cameras would be
// 155 KB, so the block shrinks as V grows: R = 256 rows up to 2 cameras, 128 up to 4, 64 up to 8 -- at most 38 912 B, four
// blocks to a CU.  One thread per row, so a wave's store in a sweep is still 256 consecutive bytes.  Row stride 19 (odd) keeps
// phase 1's writes free of bank conflicts for every V.
constexpr int GLUE_VIEWS_STAGE = 2 * 256 * 19;   // floats; = 4 * 128 * 19 = 8 * 64 * 19

// TV: each view's direction term t_v also goes to a.tv[v] (zeros for a view without a colour gradient): what the per-view camera
// centre gradients are summed from (glue_views_camera.hip).  Nothing else differs, and the TV = false instantiations are the
// kernels as they were (profiles/pose_views_isa_identity.txt).
template <int R, bool TV>
__global__ void __launch_bounds__(R) glue_backward_views_kernel(const GlueViewsArgs a) {
  __shared__ float stage[GLUE_VIEWS_STAGE];
  const int V = a.V, p0 = blockIdx.x * R, p = p0 + threadIdx.x;
  if (p < a.g.P) {
    glue_backward_activations_point(a.g, p);
    float sh[16][3];
    load_sh(a.g, p, sh);
    float gx[3] = {0.f, 0.f, 0.f};
    for (int v = 0; v < V; v++) {
      float t[3];
      glue_backward_sh_point(a.g, p, sh, a.g.campos + 3 * v, a.colors[v], a.g_colors[v], stage + (v * R + threadIdx.x) * 19, t);
#pragma unroll
      for (int k = 0; k < 3; k++) gx[k] = v == 0 ? t[k] : gx[k] + t[k];   // view 0 as it is (not 0 + t: keeps a -0)
      if (TV) {
#pragma unroll
        for (int k = 0; k < 3; k++) a.tv[v][3 * (size_t)p + k] = a.g_colors[v] != nullptr ? t[k] : 0.f;
      }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) a.g.g_xyz[3 * (size_t)p + k] = gx[k];
  }
  __syncthreads();
  const int n = min(R, a.g.P - p0);
  // sum over the cameras of basis[k] * dRGB[c] for row q of the block
  auto coeff = [&](int q, int k, int c) {
    float s = stage[q * 19 + k] * stage[q * 19 + 16 + c];
    for (int v = 1; v < V; v++) s = s + stage[(v * R + q) * 19 + k] * stage[(v * R + q) * 19 + 16 + c];
    return s;
  };
  for (int e = threadIdx.x; e < n * 3; e += R) a.g.g_f_dc[(size_t)p0 * 3 + e] = coeff(e / 3, 0, e % 3);
  for (int e = threadIdx.x; e < n * 45; e += R) {
    const int q = e / 45, kc = e % 45 + 3;
    a.g.g_f_rest[(size_t)p0 * 45 + e] = coeff(q, kc / 3, kc % 3);
  }
  if (a.g.g_dshs != nullptr) {
    const float l1 = a.g.g_dshs_l1 != nullptr ? *a.g.g_dshs_l1 / (48.0f * (float)a.g.P) : 0.f;
    for (int e = threadIdx.x; e < n * 48; e += R) {
      const int q = e / 48, kc = e % 48;
      float v = coeff(q, kc / 3, kc % 3);
      if (a.g.g_dshs_l1 != nullptr) {
        const float d = a.g.dshs[(size_t)p0 * 48 + e];
        v += d > 0.f ? l1 : (d < 0.f ? -l1 : 0.f);
      }
      a.g.g_dshs[(size_t)p0 * 48 + e] = v;
    }
  }
}

}  // namespace s3g

using namespace s3g;

extern "C" int s3g_glue_forward_views(int P, int deg, int V, const float* f_dc, const float* f_rest, const float* dshs,
                                      const float* xyz, const float* campos, const float* log_scales, const float* rot_raw,
                                      const float* opacity_logit, float* const* colors, float* scales, float* rot, float* opacity,
                                      double* dshs_abs_sum, void* stream_) {
  bool ok = P >= 0 && deg >= 0 && deg <= 3 && V >= 1 && V <= S3G_GLUE_MAX_VIEWS && colors != nullptr;
  if (ok && P > 0) {
    ok = f_dc && f_rest && xyz && campos && log_scales && rot_raw && opacity_logit && scales && rot && opacity;
    for (int v = 0; ok && v < V; v++) ok = colors[v] != nullptr;
  }
  if (!ok) {
    set_error("s3g_glue_forward_views: bad argument (1 <= V <= %d)", S3G_GLUE_MAX_VIEWS);
    return S3G_ERR_INVALID_ARG;
  }
  if (P == 0) return S3G_OK;
  GlueViewsArgs a;
  memset(&a, 0, sizeof a);
  a.g.P = P; a.g.deg = deg; a.g.f_dc = f_dc; a.g.f_rest = f_rest; a.g.dshs = dshs; a.g.xyz = xyz; a.g.campos = campos;
  a.g.log_scales = log_scales; a.g.rot_raw = rot_raw; a.g.opacity_logit = opacity_logit;
  a.g.scales = scales; a.g.rot = rot; a.g.opacity = opacity;
  a.g.dshs_abs_sum = dshs_abs_sum;
  a.V = V;
  for (int v = 0; v < V; v++) a.colors[v] = colors[v];
  if (dshs != nullptr) hipLaunchKernelGGL(glue_forward_views_kernel, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream_, a);
  else hipLaunchKernelGGL(glue_forward_views_rows_kernel, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream_, a);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

// Both entry points of the backward: s3g_glue_backward_views (tv == nullptr) and s3g_glue_backward_views_campos
// (glue_views_camera.hip; tv: V device pointers, each [P,3], written).
int s3g::glue_backward_views_launch(const char* who, int P, int deg, int V, const float* f_dc, const float* f_rest, const float* dshs,
                                    const float* xyz, const float* campos, const float* rot_raw, const float* const* colors,
                                    const float* scales, const float* rot, const float* opacity, const float* const* g_colors,
                                    const float* g_scales, const float* g_rot, const float* g_opacity, float* g_f_dc,
                                    float* g_f_rest, float* g_dshs, float* g_xyz, float* g_log_scales, float* g_rot_raw,
                                    float* g_opacity_logit, const float* g_dshs_l1, float* const* tv, void* stream_) {
  bool ok = P >= 0 && deg >= 0 && deg <= 3 && V >= 1 && V <= S3G_GLUE_MAX_VIEWS && colors != nullptr && g_colors != nullptr;
  if (ok && P > 0) {
    ok = f_dc && f_rest && xyz && campos && rot_raw && scales && rot && opacity && g_f_dc && g_f_rest && g_xyz && g_log_scales &&
         g_rot_raw && g_opacity_logit;
    for (int v = 0; ok && v < V; v++) ok = colors[v] != nullptr && (tv == nullptr || tv[v] != nullptr);
  }
  if (!ok) {
    set_error("%s: bad argument (1 <= V <= %d)", who, S3G_GLUE_MAX_VIEWS);
    return S3G_ERR_INVALID_ARG;
  }
  if (P == 0) return S3G_OK;
  GlueViewsArgs a;
  memset(&a, 0, sizeof a);
  a.g.P = P; a.g.deg = deg; a.g.f_dc = f_dc; a.g.f_rest = f_rest; a.g.dshs = dshs; a.g.xyz = xyz; a.g.campos = campos;
  a.g.rot_raw = rot_raw;
  a.g.scales = const_cast<float*>(scales); a.g.rot = const_cast<float*>(rot); a.g.opacity = const_cast<float*>(opacity);
  a.g.g_scales = g_scales; a.g.g_rot = g_rot; a.g.g_opacity = g_opacity;
  a.g.g_f_dc = g_f_dc; a.g.g_f_rest = g_f_rest; a.g.g_dshs = g_dshs; a.g.g_xyz = g_xyz; a.g.g_log_scales = g_log_scales;
  a.g.g_rot_raw = g_rot_raw; a.g.g_opacity_logit = g_opacity_logit;
  a.g.g_dshs_l1 = (dshs != nullptr && g_dshs != nullptr) ? g_dshs_l1 : nullptr;
  a.V = V;
  for (int v = 0; v < V; v++) { a.colors[v] = const_cast<float*>(colors[v]); a.g_colors[v] = g_colors[v]; }
  if (tv != nullptr)
    for (int v = 0; v < V; v++) a.tv[v] = tv[v];
  hipStream_t st = (hipStream_t)stream_;
  static_assert(8 * 64 * 19 <= GLUE_VIEWS_STAGE && 4 * 128 * 19 <= GLUE_VIEWS_STAGE && S3G_GLUE_MAX_VIEWS == 8, "stage rows per block follow V");
  if (tv == nullptr) {
    if (V <= 2) hipLaunchKernelGGL((glue_backward_views_kernel<256, false>), dim3((P + 255) / 256), dim3(256), 0, st, a);
    else if (V <= 4) hipLaunchKernelGGL((glue_backward_views_kernel<128, false>), dim3((P + 127) / 128), dim3(128), 0, st, a);
    else hipLaunchKernelGGL((glue_backward_views_kernel<64, false>), dim3((P + 63) / 64), dim3(64), 0, st, a);
  } else {
    if (V <= 2) hipLaunchKernelGGL((glue_backward_views_kernel<256, true>), dim3((P + 255) / 256), dim3(256), 0, st, a);
    else if (V <= 4) hipLaunchKernelGGL((glue_backward_views_kernel<128, true>), dim3((P + 127) / 128), dim3(128), 0, st, a);
    else hipLaunchKernelGGL((glue_backward_views_kernel<64, true>), dim3((P + 63) / 64), dim3(64), 0, st, a);
  }
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" int s3g_glue_backward_views(int P, int deg, int V, const float* f_dc, const float* f_rest, const float* dshs,
                                       const float* xyz, const float* campos, const float* rot_raw, const float* const* colors,
                                       const float* scales, const float* rot, const float* opacity, const float* const* g_colors,
                                       const float* g_scales, const float* g_rot, const float* g_opacity, float* g_f_dc,
                                       float* g_f_rest, float* g_dshs, float* g_xyz, float* g_log_scales, float* g_rot_raw,
                                       float* g_opacity_logit, const float* g_dshs_l1, void* stream_) {
  return glue_backward_views_launch("s3g_glue_backward_views", P, deg, V, f_dc, f_rest, dshs, xyz, campos, rot_raw, colors, scales, rot,
                                    opacity, g_colors, g_scales, g_rot, g_opacity, g_f_dc, g_f_rest, g_dshs, g_xyz, g_log_scales,
                                    g_rot_raw, g_opacity_logit, g_dshs_l1, nullptr, stream_);
}
