// Per-Gaussian device functions of the render glue's forward pass, shared by glue.hip (one camera) and glue_views.hip (V cameras
// of one timestamp): the argument block, the coefficient loads and the staging sweep, the activations, SH -> RGB.  Everything is
// __forceinline__: a kernel's arithmetic is the source order of these bodies, whichever file it is in.  (The backward's
// per-Gaussian function stays in glue.hip as it was: split into a camera-free and a per-camera half it computes the same bits,
// but glue_backward_kernel came out with other registers and another schedule, and that kernel's machine code is pinned --
// profiles/glue_views_isa_identity.txt.  glue_views.hip has the two halves.)
#pragma once
#include "geom_math.hpp"

namespace s3g {

struct GlueArgs {
  int P, deg;
  const float *f_dc, *f_rest, *dshs, *xyz, *campos, *log_scales, *rot_raw, *opacity_logit;
  float *colors, *scales, *rot, *opacity;
  // backward only
  const float *g_colors, *g_scales, *g_rot, *g_opacity;
  float *g_f_dc, *g_f_rest, *g_dshs, *g_xyz, *g_log_scales, *g_rot_raw, *g_opacity_logit;
  // optional L1 regulariser on dshs (train.py:407-410: lambda_dshs * mean|dshs|), folded in because both kernels stream
  // dshs anyway: forward accumulates sum|dshs|, backward adds (*g_dshs_l1 / (48 P)) * sign(dshs)
  double* dshs_abs_sum;
  const float* g_dshs_l1;
};

__device__ __forceinline__ void load_sh(const GlueArgs& a, int p, float (&sh)[16][3]) {
#pragma unroll
  for (int c = 0; c < 3; c++) sh[0][c] = a.f_dc[3 * (size_t)p + c];
#pragma unroll
  for (int k = 1; k < 16; k++)
#pragma unroll
    for (int c = 0; c < 3; c++) sh[k][c] = a.f_rest[(size_t)p * 45 + (k - 1) * 3 + c];
  if (a.dshs != nullptr) {
#pragma unroll
    for (int k = 0; k < 16; k++)
#pragma unroll
      for (int c = 0; c < 3; c++) sh[k][c] += a.dshs[(size_t)p * 48 + k * 3 + c];
  }
}

// thread = Gaussian: the three activations (they do not depend on the camera)
__device__ __forceinline__ void glue_activations_point(const GlueArgs& a, int p) {
#pragma unroll
  for (int k = 0; k < 3; k++) a.scales[3 * (size_t)p + k] = expf(a.log_scales[3 * (size_t)p + k]);
  const float4 q = reinterpret_cast<const float4*>(a.rot_raw)[p];
  const float n = fmaxf(sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w), 1e-12f);  // F.normalize eps
  reinterpret_cast<float4*>(a.rot)[p] = make_float4(q.x / n, q.y / n, q.z / n, q.w / n);
  a.opacity[p] = 1.0f / (1.0f + expf(-a.opacity_logit[p]));
}

// thread = Gaussian: SH -> RGB from the summed coefficient rows sh (registers) for the camera centre campos[3]
// (utils/sh_utils.py:57-112; same polynomial order as the rasterizer's in-kernel path)
__device__ __forceinline__ void glue_colors_point(const GlueArgs& a, int p, const float (&sh)[16][3], const float* campos,
                                                  float* colors) {
  float dx = a.xyz[3 * (size_t)p] - campos[0], dy = a.xyz[3 * (size_t)p + 1] - campos[1], dz = a.xyz[3 * (size_t)p + 2] - campos[2];
  const float len = sqrtf(dx * dx + dy * dy + dz * dz);
  const float x = dx / len, y = dy / len, z = dz / len;
  const int deg = a.deg;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    float v = SH_C0 * sh[0][c];
    if (deg > 0) {
      v = v - SH_C1 * y * sh[1][c] + SH_C1 * z * sh[2][c] - SH_C1 * x * sh[3][c];
      if (deg > 1) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        v = v + SH_C2[0] * xy * sh[4][c] + SH_C2[1] * yz * sh[5][c] + SH_C2[2] * (2.0f * zz - xx - yy) * sh[6][c] +
            SH_C2[3] * xz * sh[7][c] + SH_C2[4] * (xx - yy) * sh[8][c];
        if (deg > 2) {
          v = v + SH_C3[0] * y * (3.0f * xx - yy) * sh[9][c] + SH_C3[1] * xy * z * sh[10][c] +
              SH_C3[2] * y * (4.0f * zz - xx - yy) * sh[11][c] + SH_C3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy) * sh[12][c] +
              SH_C3[4] * x * (4.0f * zz - xx - yy) * sh[13][c] + SH_C3[5] * z * (xx - yy) * sh[14][c] +
              SH_C3[6] * x * (xx - 3.0f * yy) * sh[15][c];
        }
      }
    }
    colors[3 * (size_t)p + c] = fmaxf(v + 0.5f, 0.f);
  }
}

// thread = Gaussian: activations, then SH -> RGB
__device__ __forceinline__ void glue_forward_point(const GlueArgs& a, int p, const float (&sh)[16][3]) {
  glue_activations_point(a, p);
  glue_colors_point(a, p, sh, a.campos, a.colors);
}

// Forward with a deformation (dshs present).  Phase 1 (workgroup, coalesced): the block's 256 coefficient rows of dshs go through
// LDS as contiguous sweeps -- a wave instruction covers 256 consecutive bytes -- and pick up (f_dc | f_rest) on the way: element
// e = 48 q + r of the slice is f_rest[45 q + r - 3] = rest[e - 3 (q + 1)], contiguous but for a three-float step per row; the
// three f_dc columns follow in a short second sweep.  (Read per lane as 45- / 48-float rows, every load instruction touched 64
// different lines: 24 x dwordx4 per lane, 151 us for 0.57 GB -- the address path, not HBM.  Without dshs the 12 row loads that are
// left run at the HBM rate and that kernel is kept: glue_forward_rows_kernel.)  The |dshs| sum of the regulariser is taken from
// the same registers instead of a second sweep.  Phase 2 (thread = Gaussian): rows read back at an odd stride (conflict-free),
// same polynomial, and every coefficient is the same single addition f + d as before: colours are bit-identical.
constexpr int GLUE_ROW = 49;

template <bool FULL>   // FULL: all 256 rows of the block exist (compile-time trip counts: the loads of a sweep are issued back to back)
__device__ __forceinline__ float glue_stage_rows(const GlueArgs& a, int p0, int nrows, float* rows) {
  const float* dc = a.f_dc + (size_t)p0 * 3;
  const float* rest = a.f_rest + (size_t)p0 * 45;
  const float* d = a.dshs + (size_t)p0 * 48;
  const int n48 = FULL ? 256 * 48 : nrows * 48, n3 = FULL ? 256 * 3 : nrows * 3;
  // e = tid + 256 i; 256 = 5 * 48 + 16: (q, r) advance by (5, 16) with one carry; LDS word q * 49 + r, rest index e - 3 (q + 1)
  int r = threadIdx.x % 48, q = threadIdx.x / 48;
  int word = q * GLUE_ROW + r, src = (int)threadIdx.x - 3 * (q + 1);
  float s = 0.f;
#pragma unroll 16
  for (int e = threadIdx.x; e < n48; e += 256) {
    const float v = d[e];
    const float f = rest[src < 0 ? 0 : src];   // unconditional (no branch around the load): r < 3 reads a neighbour it does not use
    s += fabsf(v);
    rows[word] = r >= 3 ? f + v : v;
    r += 16; word += 5 * GLUE_ROW + 16; src += 256 - 15;
    if (r >= 48) { r -= 48; word += GLUE_ROW - 48; src -= 3; }
  }
  __syncthreads();   // the f_dc columns are added by other threads than the ones that stored dshs there
  for (int e = threadIdx.x; e < n3; e += 256) rows[(e / 3) * GLUE_ROW + e % 3] += dc[e];
  return s;
}

// host: the launch behind s3g_glue_backward_views and s3g_glue_backward_views_campos (glue_views.hip).  tv: nullptr, or V device
// pointers ([P,3] each) that also receive each view's own direction term.
int glue_backward_views_launch(const char* who, int P, int deg, int V, const float* f_dc, const float* f_rest, const float* dshs,
                               const float* xyz, const float* campos, const float* rot_raw, const float* const* colors,
                               const float* scales, const float* rot, const float* opacity, const float* const* g_colors,
                               const float* g_scales, const float* g_rot, const float* g_opacity, float* g_f_dc, float* g_f_rest,
                               float* g_dshs, float* g_xyz, float* g_log_scales, float* g_rot_raw, float* g_opacity_logit,
                               const float* g_dshs_l1, float* const* tv, void* stream);

}  // namespace s3g
