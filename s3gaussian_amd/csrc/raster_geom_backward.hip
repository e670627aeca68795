// Rasterizer backward, stage 2: per-Gaussian geometry backward, one thread per Gaussian, bound by the latency of its gather.
// Step 5 of the scheme in raster_backward.hip: gather the Gaussian's records, then
// conic -> cov2D -> (cov3D, mean) ; mean2D, depth -> mean ; SH ; cov3D -> scale, rot, and the densification bookkeeping.
// Formulae follow backward.cu:144-412 term by term (fp32, no contraction).
#include "geom_math.hpp"
#include "raster_dev.hpp"

namespace s3g {

// ---- wave64 reduction: inclusive scan with DPP, total lands in lane 63 (LLVM's gfx9 atomic-optimizer sequence) ----
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add(float v) {
  const int t = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, false);
  return v + __int_as_float(t);
}
__device__ __forceinline__ float wave_sum_lane63(float v) {
  v = dpp_add<0x111, 0xf>(v);  // row_shr:1
  v = dpp_add<0x112, 0xf>(v);  // row_shr:2
  v = dpp_add<0x114, 0xf>(v);  // row_shr:4
  v = dpp_add<0x118, 0xf>(v);  // row_shr:8   -> lane 15 of every row holds the row total
  v = dpp_add<0x142, 0xa>(v);  // row_bcast:15 into rows 1,3
  v = dpp_add<0x143, 0xc>(v);  // row_bcast:31 into rows 2,3 -> lane 63 holds the wave total
  return v;
}

// Sum the records of the tiles k = k0, k0+stride, ... of one Gaussian's rect (row-major inside the rect), in that order.
// The walk is a chain of dependent loads (slot_pos -> record; tile_hi beside it) and the kernel is bound by that latency, not by
// bytes: GATHER_BATCH tiles are therefore in flight at a time -- all their positions and tile ends are requested first, then all
// their records, then the sums are taken in ascending k exactly as a one-at-a-time walk would take them (a tile that contributes
// nothing adds +0: the totals are bit-identical).
#ifndef S3G_GATHER_BATCH
#define S3G_GATHER_BATCH 3   // cfg3, two-image pass: 192 / 164 / 145 / 154 / 160 / 158 us for 1 / 2 / 3 / 4 / 6 / 8 (profiles/r04_gather.txt)
#endif
template <int NR>
__device__ __forceinline__ void gather_records(const GeomBwdArgs& a, const ushort4 r, uint32_t o, int k0, int stride,
                                               float* acc) {
  constexpr int B = S3G_GATHER_BATCH;
  const int w = (int)r.z - (int)r.x, n = w * ((int)r.w - (int)r.y);
  for (int k = k0; k < n; k += B * stride) {
    uint32_t pos[B], hi[B];
#pragma unroll
    for (int j = 0; j < B; j++) {
      const int kk = k + j * stride;
      const int kc = kk < n ? kk : k;   // past the rect: a valid address whose value is not used
      const int ty = (int)r.y + kc / w, tx = (int)r.x + kc % w;
      pos[j] = a.slot_pos[o + kc];
      hi[j] = a.tile_hi[ty * a.gx + tx];  // tile_hi = absolute end of the positions the blend backward wrote
    }
    float2 v[B][NR / 2];
#pragma unroll
    for (int j = 0; j < B; j++) {
#pragma unroll
      for (int q = 0; q < NR / 2; q++) v[j][q] = make_float2(0.f, 0.f);
      if (k + j * stride < n && pos[j] < hi[j]) {
        const float2* rec = reinterpret_cast<const float2*>(a.records + (size_t)pos[j] * NR);
#pragma unroll
        for (int q = 0; q < NR / 2; q++) v[j][q] = rec[q];
      }
    }
#pragma unroll
    for (int j = 0; j < B; j++)
#pragma unroll
      for (int q = 0; q < NR / 2; q++) {
        acc[2 * q] += v[j][q].x;
        acc[2 * q + 1] += v[j][q].y;
      }
  }
}

template <int NX>
__global__ void __launch_bounds__(256) geometry_backward_kernel(const GeomBwdArgs a) {
  constexpr int NR = NX ? NREC + 4 : NREC;
  const int gid = blockIdx.x * 256 + threadIdx.x;
  const bool live = gid < a.P;
  const int idx = live ? gid : a.P - 1;  // keep every lane alive for the wave-cooperative gather below
  const size_t i3 = 3 * (size_t)idx;
  const bool vis = live && a.radii[idx] > 0 && a.ctrl[4] == 0u;   // overflowed asynchronous forward: zero gradients, no bookkeeping

  // ---- gather the per-instance records of this Gaussian (one per tile of its rect) ----
  float acc[NR];
#pragma unroll
  for (int k = 0; k < NR; k++) acc[k] = 0.f;
  const ushort4 r = vis ? a.rect[idx] : make_ushort4(0, 0, 0, 0);
  const uint32_t o = vis ? a.gauss_off[idx] : 0u;
  const int n = ((int)r.z - (int)r.x) * ((int)r.w - (int)r.y);
  constexpr int BIG = 24;
  if (n > 0 && n <= BIG) gather_records<NR>(a, r, o, 0, 1, acc);
  uint64_t big = __ballot(n > BIG);
  const int lane = threadIdx.x & 63;
  while (big) {  // wave-uniform: all 64 lanes gather one large rect together, then reduce with DPP
    const int src = __ffsll((unsigned long long)big) - 1;
    big &= big - 1;
    ushort4 br;
    br.x = (unsigned short)__shfl((int)r.x, src); br.y = (unsigned short)__shfl((int)r.y, src);
    br.z = (unsigned short)__shfl((int)r.z, src); br.w = (unsigned short)__shfl((int)r.w, src);
    const uint32_t bo = (uint32_t)__shfl((int)o, src);
    float part[NR];
#pragma unroll
    for (int k = 0; k < NR; k++) part[k] = 0.f;
    gather_records<NR>(a, br, bo, lane, 64, part);
#pragma unroll
    for (int k = 0; k < NR; k++) {
      const float tot = __shfl(wave_sum_lane63(part[k]), 63);
      if (lane == src) acc[k] = tot;
    }
  }
  if (!live) return;
  if (!vis) {  // culled: the reference leaves its zero-initialised outputs untouched
    a.dL_dmean2D[i3] = a.dL_dmean2D[i3 + 1] = a.dL_dmean2D[i3 + 2] = 0.f;
    a.dL_dcolor[i3] = a.dL_dcolor[i3 + 1] = a.dL_dcolor[i3 + 2] = 0.f;
    if (NX) a.dL_dcolor2[i3] = a.dL_dcolor2[i3 + 1] = a.dL_dcolor2[i3 + 2] = 0.f;
    a.dL_dmean3D[i3] = a.dL_dmean3D[i3 + 1] = a.dL_dmean3D[i3 + 2] = 0.f;
    a.dL_dscale[i3] = a.dL_dscale[i3 + 1] = a.dL_dscale[i3 + 2] = 0.f;
    a.dL_dopacity[idx] = 0.f;
    reinterpret_cast<float4*>(a.dL_drot)[idx] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < 6; k++) a.dL_dcov3D[6 * (size_t)idx + k] = 0.f;
    if (a.dL_dconic) reinterpret_cast<float4*>(a.dL_dconic)[idx] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.dL_ddepth) a.dL_ddepth[idx] = 0.f;
    if (a.shs != nullptr)
      for (int k = 0; k < a.M * 3; k++) a.dL_dsh[(size_t)idx * a.M * 3 + k] = 0.f;
    return;
  }
  const float4 co = a.conic_opacity[idx];
  const float S0 = acc[4], Sx = acc[5], Sy = acc[6], Sxx = acc[7], Sxy = acc[8], Syy = acc[9];
  // dL_dG = o * dL_dalpha ; dG_ddelx = -G*dx*conic.x - G*dy*conic.y ; times 0.5*W (backward.cu:571-584)
  const float g2x = (0.5f * a.W) * co.w * (-(co.x * Sx) - co.y * Sy);
  const float g2y = (0.5f * a.H) * co.w * (-(co.z * Sy) - co.y * Sx);
  const float dcx = -0.5f * co.w * Sxx, dcy = -0.5f * co.w * Sxy, dcz = -0.5f * co.w * Syy;
  const float gdep = acc[3];
  a.dL_dmean2D[i3] = g2x; a.dL_dmean2D[i3 + 1] = g2y; a.dL_dmean2D[i3 + 2] = 0.f;
  a.dL_dcolor[i3] = acc[0]; a.dL_dcolor[i3 + 1] = acc[1]; a.dL_dcolor[i3 + 2] = acc[2];
  if (NX) { a.dL_dcolor2[i3] = acc[NREC]; a.dL_dcolor2[i3 + 1] = acc[NREC + 1]; a.dL_dcolor2[i3 + 2] = acc[NREC + 2]; }
  a.dL_dopacity[idx] = S0;
  if (a.dL_dconic) reinterpret_cast<float4*>(a.dL_dconic)[idx] = make_float4(dcx, dcy, 0.f, dcz);
  if (a.dL_ddepth) a.dL_ddepth[idx] = gdep;
  if (a.dens_accum) {  // the viewspace gradient and the radius are in registers: no separate passes over [P]
    a.dens_accum[idx] += sqrtf(g2x * g2x + g2y * g2y);
    a.dens_denom[idx] += 1.f;
    a.dens_max_radii[idx] = fmaxf(a.dens_max_radii[idx], (float)a.radii[idx]);
  }

  const float3 mean = make_float3(a.means3D[3 * idx], a.means3D[3 * idx + 1], a.means3D[3 * idx + 2]);
  const float* V = a.view;
  const float* proj = a.proj;

  // ---- computeCov2DCUDA (backward.cu:144-274) ----
  float cov3D[6];
#pragma unroll
  for (int k = 0; k < 6; k++) cov3D[k] = a.cov3Ds[6 * (size_t)idx + k];
  const Cov2DCtx c = cov2d_common(mean, a.fx, a.fy, a.tan_fovx, a.tan_fovy, cov3D, V);
  const float x_grad_mul = (c.txtz < -c.limx || c.txtz > c.limx) ? 0.f : 1.f;
  const float y_grad_mul = (c.tytz < -c.limy || c.tytz > c.limy) ? 0.f : 1.f;
  const float ca = c.cov.m[0][0] + 0.3f, cb = c.cov.m[0][1], cc = c.cov.m[1][1] + 0.3f;
  const float denom = ca * cc - cb * cb;
  float dL_da = 0.f, dL_db = 0.f, dL_dc = 0.f;
  const float denom2inv = 1.0f / ((denom * denom) + 0.0000001f);
  float dcov[6];
#define TM(c_, r_) c.T.m[c_][r_]
#define VM(c_, r_) c.Vrk.m[c_][r_]
  if (denom2inv != 0.f) {
    dL_da = denom2inv * (-cc * cc * dcx + 2 * cb * cc * dcy + (denom - ca * cc) * dcz);
    dL_dc = denom2inv * (-ca * ca * dcz + 2 * ca * cb * dcy + (denom - ca * cc) * dcx);
    dL_db = denom2inv * 2 * (cb * cc * dcx - (denom + 2 * cb * cb) * dcy + ca * cb * dcz);
    dcov[0] = (TM(0, 0) * TM(0, 0) * dL_da + TM(0, 0) * TM(1, 0) * dL_db + TM(1, 0) * TM(1, 0) * dL_dc);
    dcov[3] = (TM(0, 1) * TM(0, 1) * dL_da + TM(0, 1) * TM(1, 1) * dL_db + TM(1, 1) * TM(1, 1) * dL_dc);
    dcov[5] = (TM(0, 2) * TM(0, 2) * dL_da + TM(0, 2) * TM(1, 2) * dL_db + TM(1, 2) * TM(1, 2) * dL_dc);
    dcov[1] = 2 * TM(0, 0) * TM(0, 1) * dL_da + (TM(0, 0) * TM(1, 1) + TM(0, 1) * TM(1, 0)) * dL_db + 2 * TM(1, 0) * TM(1, 1) * dL_dc;
    dcov[2] = 2 * TM(0, 0) * TM(0, 2) * dL_da + (TM(0, 0) * TM(1, 2) + TM(0, 2) * TM(1, 0)) * dL_db + 2 * TM(1, 0) * TM(1, 2) * dL_dc;
    dcov[4] = 2 * TM(0, 2) * TM(0, 1) * dL_da + (TM(0, 1) * TM(1, 2) + TM(0, 2) * TM(1, 1)) * dL_db + 2 * TM(1, 1) * TM(1, 2) * dL_dc;
  } else {
#pragma unroll
    for (int k = 0; k < 6; k++) dcov[k] = 0.f;
  }
#pragma unroll
  for (int k = 0; k < 6; k++) a.dL_dcov3D[6 * (size_t)idx + k] = dcov[k];

  const float dL_dT00 = 2 * (TM(0, 0) * VM(0, 0) + TM(0, 1) * VM(0, 1) + TM(0, 2) * VM(0, 2)) * dL_da + (TM(1, 0) * VM(0, 0) + TM(1, 1) * VM(0, 1) + TM(1, 2) * VM(0, 2)) * dL_db;
  const float dL_dT01 = 2 * (TM(0, 0) * VM(1, 0) + TM(0, 1) * VM(1, 1) + TM(0, 2) * VM(1, 2)) * dL_da + (TM(1, 0) * VM(1, 0) + TM(1, 1) * VM(1, 1) + TM(1, 2) * VM(1, 2)) * dL_db;
  const float dL_dT02 = 2 * (TM(0, 0) * VM(2, 0) + TM(0, 1) * VM(2, 1) + TM(0, 2) * VM(2, 2)) * dL_da + (TM(1, 0) * VM(2, 0) + TM(1, 1) * VM(2, 1) + TM(1, 2) * VM(2, 2)) * dL_db;
  const float dL_dT10 = 2 * (TM(1, 0) * VM(0, 0) + TM(1, 1) * VM(0, 1) + TM(1, 2) * VM(0, 2)) * dL_dc + (TM(0, 0) * VM(0, 0) + TM(0, 1) * VM(0, 1) + TM(0, 2) * VM(0, 2)) * dL_db;
  const float dL_dT11 = 2 * (TM(1, 0) * VM(1, 0) + TM(1, 1) * VM(1, 1) + TM(1, 2) * VM(1, 2)) * dL_dc + (TM(0, 0) * VM(1, 0) + TM(0, 1) * VM(1, 1) + TM(0, 2) * VM(1, 2)) * dL_db;
  const float dL_dT12 = 2 * (TM(1, 0) * VM(2, 0) + TM(1, 1) * VM(2, 1) + TM(1, 2) * VM(2, 2)) * dL_dc + (TM(0, 0) * VM(2, 0) + TM(0, 1) * VM(2, 1) + TM(0, 2) * VM(2, 2)) * dL_db;
#undef TM
#undef VM
  const float dL_dJ00 = c.W.m[0][0] * dL_dT00 + c.W.m[0][1] * dL_dT01 + c.W.m[0][2] * dL_dT02;
  const float dL_dJ02 = c.W.m[2][0] * dL_dT00 + c.W.m[2][1] * dL_dT01 + c.W.m[2][2] * dL_dT02;
  const float dL_dJ11 = c.W.m[1][0] * dL_dT10 + c.W.m[1][1] * dL_dT11 + c.W.m[1][2] * dL_dT12;
  const float dL_dJ12 = c.W.m[2][0] * dL_dT10 + c.W.m[2][1] * dL_dT11 + c.W.m[2][2] * dL_dT12;
  const float tz = 1.f / c.t.z, tz2 = tz * tz, tz3 = tz2 * tz;
  const float dL_dtx = x_grad_mul * -a.fx * tz2 * dL_dJ02;
  const float dL_dty = y_grad_mul * -a.fy * tz2 * dL_dJ12;
  const float dL_dtz = -a.fx * tz2 * dL_dJ00 - a.fy * tz2 * dL_dJ11 + (2 * a.fx * c.t.x) * tz3 * dL_dJ02 +
                       (2 * a.fy * c.t.y) * tz3 * dL_dJ12;
  // transformVec4x3Transpose (auxiliary.h:89-97); the reference ASSIGNS here (backward.cu:273)
  float dmx = V[0] * dL_dtx + V[1] * dL_dty + V[2] * dL_dtz;
  float dmy = V[4] * dL_dtx + V[5] * dL_dty + V[6] * dL_dtz;
  float dmz = V[8] * dL_dtx + V[9] * dL_dty + V[10] * dL_dtz;

  // ---- preprocessCUDA backward (backward.cu:346-412) ----
  const float4 m_hom = xform_4x4(mean, proj);
  const float m_w = 1.0f / (m_hom.w + 0.0000001f);
  const float mul1 = (proj[0] * mean.x + proj[4] * mean.y + proj[8] * mean.z + proj[12]) * m_w * m_w;
  const float mul2 = (proj[1] * mean.x + proj[5] * mean.y + proj[9] * mean.z + proj[13]) * m_w * m_w;
  dmx += (proj[0] * m_w - proj[3] * mul1) * g2x + (proj[1] * m_w - proj[3] * mul2) * g2y;
  dmy += (proj[4] * m_w - proj[7] * mul1) * g2x + (proj[5] * m_w - proj[7] * mul2) * g2y;
  dmz += (proj[8] * m_w - proj[11] * mul1) * g2x + (proj[9] * m_w - proj[11] * mul2) * g2y;
  const float mul3 = V[2] * mean.x + V[6] * mean.y + V[10] * mean.z + V[14];
  dmx += (V[2] - V[3] * mul3) * gdep;
  dmy += (V[6] - V[7] * mul3) * gdep;
  dmz += (V[10] - V[11] * mul3) * gdep;

  // ---- SH backward (backward.cu:20-139) ----
  if (a.shs != nullptr) {
    const int deg = a.D;
    const float3 dir_orig = make_float3(mean.x - a.campos[0], mean.y - a.campos[1], mean.z - a.campos[2]);
    const float len = sqrtf(dir_orig.x * dir_orig.x + dir_orig.y * dir_orig.y + dir_orig.z * dir_orig.z);
    const float x = dir_orig.x / len, y = dir_orig.y / len, z = dir_orig.z / len;
    const float* sh = a.shs + (size_t)idx * a.M * 3;
    float* dsh = a.dL_dsh + (size_t)idx * a.M * 3;
    float dRGB[3], dRdx[3] = {0.f, 0.f, 0.f}, dRdy[3] = {0.f, 0.f, 0.f}, dRdz[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int ch = 0; ch < 3; ch++) dRGB[ch] = acc[ch] * (a.clamped[3 * (size_t)idx + ch] ? 0.f : 1.f);
    for (int k = (deg + 1) * (deg + 1) * 3; k < a.M * 3; k++) dsh[k] = 0.f;  // coefficients above the active degree
#define SH(k) sh[(k)*3 + ch]
#define DSH(k, v) dsh[(k)*3 + ch] = (v)*dRGB[ch]
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      DSH(0, SH_C0);
      if (deg > 0) {
        DSH(1, -SH_C1 * y); DSH(2, SH_C1 * z); DSH(3, -SH_C1 * x);
        dRdx[ch] = -SH_C1 * SH(3); dRdy[ch] = -SH_C1 * SH(1); dRdz[ch] = SH_C1 * SH(2);
        if (deg > 1) {
          const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
          DSH(4, SH_C2[0] * xy); DSH(5, SH_C2[1] * yz); DSH(6, SH_C2[2] * (2.f * zz - xx - yy));
          DSH(7, SH_C2[3] * xz); DSH(8, SH_C2[4] * (xx - yy));
          dRdx[ch] += SH_C2[0] * y * SH(4) + SH_C2[2] * 2.f * -x * SH(6) + SH_C2[3] * z * SH(7) + SH_C2[4] * 2.f * x * SH(8);
          dRdy[ch] += SH_C2[0] * x * SH(4) + SH_C2[1] * z * SH(5) + SH_C2[2] * 2.f * -y * SH(6) + SH_C2[4] * 2.f * -y * SH(8);
          dRdz[ch] += SH_C2[1] * y * SH(5) + SH_C2[2] * 2.f * 2.f * z * SH(6) + SH_C2[3] * x * SH(7);
          if (deg > 2) {
            DSH(9, SH_C3[0] * y * (3.f * xx - yy)); DSH(10, SH_C3[1] * xy * z); DSH(11, SH_C3[2] * y * (4.f * zz - xx - yy));
            DSH(12, SH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy)); DSH(13, SH_C3[4] * x * (4.f * zz - xx - yy));
            DSH(14, SH_C3[5] * z * (xx - yy)); DSH(15, SH_C3[6] * x * (xx - 3.f * yy));
            dRdx[ch] += (SH_C3[0] * SH(9) * 3.f * 2.f * xy + SH_C3[1] * SH(10) * yz + SH_C3[2] * SH(11) * -2.f * xy +
                         SH_C3[3] * SH(12) * -3.f * 2.f * xz + SH_C3[4] * SH(13) * (-3.f * xx + 4.f * zz - yy) +
                         SH_C3[5] * SH(14) * 2.f * xz + SH_C3[6] * SH(15) * 3.f * (xx - yy));
            dRdy[ch] += (SH_C3[0] * SH(9) * 3.f * (xx - yy) + SH_C3[1] * SH(10) * xz + SH_C3[2] * SH(11) * (-3.f * yy + 4.f * zz - xx) +
                         SH_C3[3] * SH(12) * -3.f * 2.f * yz + SH_C3[4] * SH(13) * -2.f * xy + SH_C3[5] * SH(14) * -2.f * yz +
                         SH_C3[6] * SH(15) * -3.f * 2.f * xy);
            dRdz[ch] += (SH_C3[1] * SH(10) * xy + SH_C3[2] * SH(11) * 4.f * 2.f * yz + SH_C3[3] * SH(12) * 3.f * (2.f * zz - xx - yy) +
                         SH_C3[4] * SH(13) * 4.f * 2.f * xz + SH_C3[5] * SH(14) * (xx - yy));
          }
        }
      }
    }
#undef SH
#undef DSH
    const float ddx = dRdx[0] * dRGB[0] + dRdx[1] * dRGB[1] + dRdx[2] * dRGB[2];
    const float ddy = dRdy[0] * dRGB[0] + dRdy[1] * dRGB[1] + dRdy[2] * dRGB[2];
    const float ddz = dRdz[0] * dRGB[0] + dRdz[1] * dRGB[1] + dRdz[2] * dRGB[2];
    // dnormvdv (auxiliary.h:107-117)
    const float3 v = dir_orig;
    const float sum2 = v.x * v.x + v.y * v.y + v.z * v.z;
    const float invsum32 = 1.0f / sqrtf(sum2 * sum2 * sum2);
    dmx += ((+sum2 - v.x * v.x) * ddx - v.y * v.x * ddy - v.z * v.x * ddz) * invsum32;
    dmy += (-v.x * v.y * ddx + (sum2 - v.y * v.y) * ddy - v.z * v.y * ddz) * invsum32;
    dmz += (-v.x * v.z * ddx - v.y * v.z * ddy + (sum2 - v.z * v.z) * ddz) * invsum32;
  }
  a.dL_dmean3D[3 * (size_t)idx + 0] = dmx;
  a.dL_dmean3D[3 * (size_t)idx + 1] = dmy;
  a.dL_dmean3D[3 * (size_t)idx + 2] = dmz;

  // ---- computeCov3D backward (backward.cu:278-341) ----
  if (a.scales != nullptr) {
    const float4 rot = reinterpret_cast<const float4*>(a.rotations)[idx];
    const float r = rot.x, x = rot.y, y = rot.z, z = rot.w;
    const M3 R = quat_to_R(rot);
    const float3 s = make_float3(a.scale_modifier * a.scales[3 * idx], a.scale_modifier * a.scales[3 * idx + 1],
                                 a.scale_modifier * a.scales[3 * idx + 2]);
    M3 S = {{{s.x, 0.f, 0.f}, {0.f, s.y, 0.f}, {0.f, 0.f, s.z}}};
    M3 Mm = m3_mul(S, R);
    M3 dSigma = {{{dcov[0], 0.5f * dcov[1], 0.5f * dcov[2]}, {0.5f * dcov[1], dcov[3], 0.5f * dcov[4]}, {0.5f * dcov[2], 0.5f * dcov[4], dcov[5]}}};
    M3 M2;
#pragma unroll
    for (int cc_ = 0; cc_ < 3; cc_++)
#pragma unroll
      for (int rr = 0; rr < 3; rr++) M2.m[cc_][rr] = 2.0f * Mm.m[cc_][rr];
    M3 dM = m3_mul(M2, dSigma);
    M3 Rt = m3_T(R), dMt = m3_T(dM);
    a.dL_dscale[3 * (size_t)idx + 0] = Rt.m[0][0] * dMt.m[0][0] + Rt.m[0][1] * dMt.m[0][1] + Rt.m[0][2] * dMt.m[0][2];
    a.dL_dscale[3 * (size_t)idx + 1] = Rt.m[1][0] * dMt.m[1][0] + Rt.m[1][1] * dMt.m[1][1] + Rt.m[1][2] * dMt.m[1][2];
    a.dL_dscale[3 * (size_t)idx + 2] = Rt.m[2][0] * dMt.m[2][0] + Rt.m[2][1] * dMt.m[2][1] + Rt.m[2][2] * dMt.m[2][2];
    const float sv[3] = {s.x, s.y, s.z};
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int rr = 0; rr < 3; rr++) dMt.m[k][rr] *= sv[k];
#define Dm(c_, r_) dMt.m[c_][r_]
    float4 dq;
    dq.x = 2 * z * (Dm(0, 1) - Dm(1, 0)) + 2 * y * (Dm(2, 0) - Dm(0, 2)) + 2 * x * (Dm(1, 2) - Dm(2, 1));
    dq.y = 2 * y * (Dm(1, 0) + Dm(0, 1)) + 2 * z * (Dm(2, 0) + Dm(0, 2)) + 2 * r * (Dm(1, 2) - Dm(2, 1)) - 4 * x * (Dm(2, 2) + Dm(1, 1));
    dq.z = 2 * x * (Dm(1, 0) + Dm(0, 1)) + 2 * r * (Dm(2, 0) - Dm(0, 2)) + 2 * z * (Dm(1, 2) + Dm(2, 1)) - 4 * y * (Dm(2, 2) + Dm(0, 0));
    dq.w = 2 * r * (Dm(0, 1) - Dm(1, 0)) + 2 * x * (Dm(2, 0) + Dm(0, 2)) + 2 * y * (Dm(1, 2) + Dm(2, 1)) - 4 * z * (Dm(1, 1) + Dm(0, 0));
#undef Dm
    reinterpret_cast<float4*>(a.dL_drot)[idx] = dq;
  } else {
    a.dL_dscale[i3] = a.dL_dscale[i3 + 1] = a.dL_dscale[i3 + 2] = 0.f;
    reinterpret_cast<float4*>(a.dL_drot)[idx] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

int launch_geometry_backward(const GeomBwdArgs& ga, bool two_images, hipStream_t stream, bool debug) {
  hipLaunchKernelGGL(two_images ? geometry_backward_kernel<3> : geometry_backward_kernel<0>, dim3((ga.P + 255) / 256), dim3(256),
                     0, stream, ga);
  S3G_KERNEL_CHECK(stream, debug);
  return S3G_OK;
}

}  // namespace s3g
