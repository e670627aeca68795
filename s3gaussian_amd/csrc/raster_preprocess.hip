// Rasterizer forward, stage 1: the per-Gaussian preprocess (EWA projection).  HBM-bound: 56 B read + ~68 B written per Gaussian.
// Bit-exact with the fp32 oracle: contraction is disabled so every op rounds once, in source order
// (glm mat3 products expanded in glm's summation order, type_mat3x3.inl:486-518).
#include "geom_math.hpp"

namespace s3g {

// forward.cu:20-71
__device__ __forceinline__ float3 sh_to_rgb(int idx, int deg, int M, const float3 pos, const float3 campos,
                                            const float* __restrict__ shs, uint8_t* __restrict__ clamped) {
  float3 dir = make_float3(pos.x - campos.x, pos.y - campos.y, pos.z - campos.z);
  const float len = sqrtf(dir.x * dir.x + dir.y * dir.y + dir.z * dir.z);
  const float x = dir.x / len, y = dir.y / len, z = dir.z / len;
  const float* sh = shs + (size_t)idx * M * 3;
  float res[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
#define SH(k) sh[(k)*3 + c]
    float v = SH_C0 * SH(0);
    if (deg > 0) {
      v = v - SH_C1 * y * SH(1) + SH_C1 * z * SH(2) - SH_C1 * x * SH(3);
      if (deg > 1) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        v = v + SH_C2[0] * xy * SH(4) + SH_C2[1] * yz * SH(5) + SH_C2[2] * (2.0f * zz - xx - yy) * SH(6) +
            SH_C2[3] * xz * SH(7) + SH_C2[4] * (xx - yy) * SH(8);
        if (deg > 2) {
          v = v + SH_C3[0] * y * (3.0f * xx - yy) * SH(9) + SH_C3[1] * xy * z * SH(10) +
              SH_C3[2] * y * (4.0f * zz - xx - yy) * SH(11) + SH_C3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy) * SH(12) +
              SH_C3[4] * x * (4.0f * zz - xx - yy) * SH(13) + SH_C3[5] * z * (xx - yy) * SH(14) +
              SH_C3[6] * x * (xx - 3.0f * yy) * SH(15);
        }
      }
    }
#undef SH
    v += 0.5f;
    clamped[3 * idx + c] = (v < 0.f);
    res[c] = fmaxf(v, 0.f);
  }
  return make_float3(res[0], res[1], res[2]);
}

struct PreprocessArgs {
  int P, D, M, W, H, gx, gy;
  int cull;  // exact (tile, Gaussian) culling: tile_mask is filled here for rects of <= TILE_MASK_BITS tiles
  const float* means3D;
  const float* scales;
  float scale_modifier;
  const float* rotations;
  const float* opacities;
  const float* shs;
  const float* cov3D_precomp;
  const float* colors_precomp;
  const float* viewmatrix;
  const float* projmatrix;
  const float* cam_pos;
  float tan_fovx, tan_fovy, focal_x, focal_y;
  int prefiltered;
  int* radii;
  GeomState g;
  uint32_t* ctrl;
};

__global__ void __launch_bounds__(256) preprocess_kernel(const PreprocessArgs a) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.P) return;
  a.radii[idx] = 0;
  a.g.rect[idx] = make_ushort4(0, 0, 0, 0);

  const float3 p = make_float3(a.means3D[3 * idx], a.means3D[3 * idx + 1], a.means3D[3 * idx + 2]);
  const float3 p_view = xform_4x3(p, a.viewmatrix);
  if (p_view.z <= 0.2f) {  // in_frustum, auxiliary.h:154
    if (a.prefiltered) atomicOr(&a.ctrl[2], 1u);
    return;
  }
  const float4 p_hom = xform_4x4(p, a.projmatrix);
  const float p_w = 1.0f / (p_hom.w + 0.0000001f);
  const float2 p_proj = make_float2(p_hom.x * p_w, p_hom.y * p_w);

  float cov3D[6];
  if (a.cov3D_precomp != nullptr) {
#pragma unroll
    for (int k = 0; k < 6; k++) cov3D[k] = a.cov3D_precomp[6 * (size_t)idx + k];
  } else {
    const float3 s = make_float3(a.scales[3 * idx], a.scales[3 * idx + 1], a.scales[3 * idx + 2]);
    const float4 q = reinterpret_cast<const float4*>(a.rotations)[idx];
    cov3d_from_scale_rot(s, a.scale_modifier, q, cov3D);
#pragma unroll
    for (int k = 0; k < 6; k++) a.g.cov3D[6 * (size_t)idx + k] = cov3D[k];
  }
  const Cov2DCtx cc = cov2d_common(p, a.focal_x, a.focal_y, a.tan_fovx, a.tan_fovy, cov3D, a.viewmatrix);
  const float3 cov = make_float3(cc.cov.m[0][0] + 0.3f, cc.cov.m[0][1], cc.cov.m[1][1] + 0.3f);
  const float det = cov.x * cov.z - cov.y * cov.y;
  if (det == 0.0f) return;
  const float det_inv = 1.f / det;
  const float3 conic = make_float3(cov.z * det_inv, -cov.y * det_inv, cov.x * det_inv);
  const float mid = 0.5f * (cov.x + cov.z);
  const float lambda1 = mid + sqrtf(fmaxf(0.1f, mid * mid - det));
  const float lambda2 = mid - sqrtf(fmaxf(0.1f, mid * mid - det));
  const float my_radius = ceilf(3.f * sqrtf(fmaxf(lambda1, lambda2)));
  // ndc2Pix (auxiliary.h:41-44) is double arithmetic in the reference (double literals)
  const float px = (float)((((double)p_proj.x + 1.0) * a.W - 1.0) * 0.5);
  const float py = (float)((((double)p_proj.y + 1.0) * a.H - 1.0) * 0.5);
  // getRect (auxiliary.h:46-56)
  const int r = (int)my_radius;
  const int rx0 = min(a.gx, max(0, (int)((px - r) / TILE_X)));
  const int ry0 = min(a.gy, max(0, (int)((py - r) / TILE_Y)));
  const int rx1 = min(a.gx, max(0, (int)((px + r + TILE_X - 1) / TILE_X)));
  const int ry1 = min(a.gy, max(0, (int)((py + r + TILE_Y - 1) / TILE_Y)));
  if ((rx1 - rx0) * (ry1 - ry0) == 0) return;

  if (a.colors_precomp == nullptr) {
    const float3 cp = make_float3(a.cam_pos[0], a.cam_pos[1], a.cam_pos[2]);
    const float3 c = sh_to_rgb(idx, a.D, a.M, p, cp, a.shs, a.g.clamped);
    a.g.rgb[3 * (size_t)idx + 0] = c.x;
    a.g.rgb[3 * (size_t)idx + 1] = c.y;
    a.g.rgb[3 * (size_t)idx + 2] = c.z;
  }
  a.g.depths[idx] = p_view.z;
  a.radii[idx] = r;
  a.g.means2D[idx] = make_float2(px, py);
  a.g.conic_opacity[idx] = make_float4(conic.x, conic.y, conic.z, a.opacities[idx]);
  a.g.rect[idx] = make_ushort4((unsigned short)rx0, (unsigned short)ry0, (unsigned short)rx1, (unsigned short)ry1);
  // exact tile culling (geom_math.hpp::tile_can_contribute) evaluated HERE, one well-occupied thread per Gaussian; the two
  // binning passes (few fat workgroups, latency-bound) only replay the mask
  if (a.cull && (rx1 - rx0) * (ry1 - ry0) <= TILE_MASK_BITS) {
    const TileCull tc = tile_cull_prepare(make_float2(px, py), make_float4(conic.x, conic.y, conic.z, a.opacities[idx]));
    uint32_t mask = 0u, bit = 1u;
    for (int y = ry0; y < ry1; y++)
      for (int x = rx0; x < rx1; x++, bit <<= 1)
        if (tile_can_contribute(tc, x, y, a.W, a.H)) mask |= bit;
    a.g.tile_mask[idx] = mask;
  }
}

__global__ void __launch_bounds__(256) check_frustum_kernel(int P, const float* __restrict__ means3D,
                                                            const float* __restrict__ viewmatrix,
                                                            uint8_t* __restrict__ present) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= P) return;
  const float3 p = make_float3(means3D[3 * idx], means3D[3 * idx + 1], means3D[3 * idx + 2]);
  present[idx] = xform_4x3(p, viewmatrix).z > 0.2f ? 1 : 0;
}

int launch_preprocess(const s3g_raster_inputs* in, const Arenas& a, bool exact_cull, int* radii, hipStream_t stream) {
  const int P = in->P;
  PreprocessArgs pa;
  pa.P = P; pa.D = in->D; pa.M = in->M; pa.W = a.W; pa.H = a.H; pa.gx = a.gx; pa.gy = a.gy;
  pa.cull = exact_cull ? 1 : 0;
  pa.means3D = in->means3D; pa.scales = in->scales; pa.scale_modifier = in->scale_modifier;
  pa.rotations = in->rotations; pa.opacities = in->opacities; pa.shs = in->shs;
  pa.cov3D_precomp = in->cov3D_precomp; pa.colors_precomp = in->colors_precomp;
  pa.viewmatrix = in->viewmatrix; pa.projmatrix = in->projmatrix; pa.cam_pos = in->cam_pos;
  pa.tan_fovx = in->tan_fovx; pa.tan_fovy = in->tan_fovy;
  pa.focal_y = a.H / (2.0f * in->tan_fovy); pa.focal_x = a.W / (2.0f * in->tan_fovx);
  pa.prefiltered = in->prefiltered; pa.radii = radii; pa.g = a.g; pa.ctrl = a.im.ctrl;
  hipLaunchKernelGGL(preprocess_kernel, dim3((P + 255) / 256), dim3(256), 0, stream, pa);
  S3G_KERNEL_CHECK(stream, in->debug != 0);
  return S3G_OK;
}

}  // namespace s3g

using namespace s3g;

extern "C" int s3g_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                                uint8_t* present, void* stream_) {
  clear_error();
  (void)projmatrix;
  if (P < 0 || (P > 0 && (!means3D || !viewmatrix || !present))) {
    set_error("s3g_mark_visible: bad argument");
    return S3G_ERR_INVALID_ARG;
  }
  if (P == 0) return S3G_OK;
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(check_frustum_kernel, dim3((P + 255) / 256), dim3(256), 0, stream, P, means3D, viewmatrix, present);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}
