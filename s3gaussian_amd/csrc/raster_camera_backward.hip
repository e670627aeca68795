// Camera gradients of the rasterizer backward and the pose map in front of them (include/s3g_camera.h) for gfx950.
//
// camera_backward_kernel: one thread per Gaussian, after a rasterizer backward, on that backward's per-Gaussian outputs.  It
// reads about 90 B per Gaussian ([P]-sized arrays only, never the per-instance records) and is bound by them, so the
// per-Gaussian terms are evaluated in double from the fp32 inputs: t, J, T = W J, the 2D covariance and the chain
// dL_dconic -> (dL_da, dL_db, dL_dc) -> dL_dT -> (dL_dW, dL_dJ -> dL_dt) follow geometry_backward_kernel line by line, the SH
// direction term follows its SH block.  A Gaussian's terms are formed completely before they are added to the thread's 27 sums
// (12 + 12 + 3: the entries of view, proj and campos that enter a product), so that a restatement which forms the same terms
// differs in the order of the sum over P and in nothing else.
// The sum follows alpha.hip / metrics.hip: a workgroup adds its threads' sums in a fixed order and stores one partial per slot
// with plain stores; camera_fold_kernel, one workgroup, adds the partials in a fixed order.  No floating-point atomics.
//
// pose_apply_kernel / pose_apply_backward_kernel: the six-parameter camera correction, a few hundred double operations in one
// thread (forward) or in six threads, one tangent each (backward, forward-mode).
#include "raster_dev.hpp"
#include "camera_sum.hpp"   // CAM_THREADS, CAM_MAX_BLOCKS, cam_blocks

#include "../../include/s3g_camera.h"

namespace s3g {

constexpr int CAM_SLOTS = 27;          // view[4k+i] k<4,i<3 | proj[4k+{0,1,3}] k<4 | campos[3]
constexpr int CAM_FOLD_THREADS = 1024; // camera_fold_kernel: 32 groups of 32 lanes, lane = slot

__host__ __device__ inline int cam_slot_out(int s) {   // slot -> index into the 35 outputs
  if (s < 12) return 4 * (s / 3) + s % 3;
  if (s < 24) return 16 + 4 * ((s - 12) / 3) + ((s - 12) % 3 == 2 ? 3 : (s - 12) % 3);
  return 32 + (s - 24);
}

struct CamBwdArgs {
  int P, D, M;
  const float* means3D;
  const int* radii;
  const float* cov3Ds;      // precomputed or the forward's own
  const uint8_t* clamped;   // [P,3] of the forward (SH path)
  const float* shs;
  const float* view;
  const float* proj;
  const float* campos;
  double fx, fy, limx, limy;
  const float* dL_dmean2D;  // each of the five may be NULL: its terms are dropped
  const float* dL_dconic;
  const float* dL_ddepth;
  const float* dL_dcolor;
  const float* g_dir;
  double* partial;          // [blocks][CAM_SLOTS]
};

// SH constants in double (auxiliary.h:22-39), the values geom_math.hpp rounds to fp32
__device__ const double DSH_C1 = 0.4886025119029199;
__device__ const double DSH_C2[5] = {1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792,
                                     0.5462742152960396};
__device__ const double DSH_C3[7] = {-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154,
                                     -0.4570457994644658, 1.445305721320277, -0.5900435899266435};

// The 27 terms of Gaussian idx: tv = view slots, tp = proj slots, tc = campos.
__device__ __forceinline__ void camera_terms(const CamBwdArgs& a, int idx, double* tv, double* tp, double* tc) {
#pragma unroll
  for (int k = 0; k < 12; k++) tv[k] = tp[k] = 0.0;
  tc[0] = tc[1] = tc[2] = 0.0;
  const size_t i3 = 3 * (size_t)idx;
  const bool vis = a.radii != nullptr && a.radii[idx] > 0;
  if (vis) {
    const double m[3] = {(double)a.means3D[i3], (double)a.means3D[i3 + 1], (double)a.means3D[i3 + 2]};
    // ---- view: covariance path (computeCov2DCUDA backward) + depth ----
    if (a.dL_dconic != nullptr || a.dL_ddepth != nullptr) {
      double dcx = 0.0, dcy = 0.0, dcz = 0.0;
      if (a.dL_dconic != nullptr) {
        const float4 dc = reinterpret_cast<const float4*>(a.dL_dconic)[idx];
        dcx = (double)dc.x; dcy = (double)dc.y; dcz = (double)dc.w;
      }
      const double gdep = a.dL_ddepth != nullptr ? (double)a.dL_ddepth[idx] : 0.0;
      const bool conic_live = dcx != 0.0 || dcy != 0.0 || dcz != 0.0;
      if (conic_live || gdep != 0.0) {
        double gt[3] = {0.0, 0.0, gdep};
        if (conic_live) {
          double V[12];   // V[3k+i] = view[4k+i]
#pragma unroll
          for (int k = 0; k < 4; k++)
#pragma unroll
            for (int i = 0; i < 3; i++) V[3 * k + i] = (double)a.view[4 * k + i];
          double t[3];
#pragma unroll
          for (int i = 0; i < 3; i++) t[i] = V[i] * m[0] + V[3 + i] * m[1] + V[6 + i] * m[2] + V[9 + i];
          const double tz = t[2];
          const double txtz = t[0] / tz, tytz = t[1] / tz;
          const double xm = (txtz < -a.limx || txtz > a.limx) ? 0.0 : 1.0;
          const double ym = (tytz < -a.limy || tytz > a.limy) ? 0.0 : 1.0;
          const double txc = fmin(a.limx, fmax(-a.limx, txtz)) * tz;
          const double tyc = fmin(a.limy, fmax(-a.limy, tytz)) * tz;
          const double J00 = a.fx / tz, J11 = a.fy / tz;
          const double J02 = -(a.fx * txc) / (tz * tz), J12 = -(a.fy * tyc) / (tz * tz);
          double S[6];
#pragma unroll
          for (int k = 0; k < 6; k++) S[k] = (double)a.cov3Ds[6 * (size_t)idx + k];
          const double Sm[3][3] = {{S[0], S[1], S[2]}, {S[1], S[3], S[4]}, {S[2], S[4], S[5]}};
          double T0[3], T1[3], U0[3], U1[3];   // T = W J (columns 0, 1), U = Sigma T
#pragma unroll
          for (int k = 0; k < 3; k++) {
            T0[k] = V[3 * k] * J00 + V[3 * k + 2] * J02;
            T1[k] = V[3 * k + 1] * J11 + V[3 * k + 2] * J12;
          }
#pragma unroll
          for (int k = 0; k < 3; k++) {
            U0[k] = Sm[k][0] * T0[0] + Sm[k][1] * T0[1] + Sm[k][2] * T0[2];
            U1[k] = Sm[k][0] * T1[0] + Sm[k][1] * T1[1] + Sm[k][2] * T1[2];
          }
          const double ca = (T0[0] * U0[0] + T0[1] * U0[1] + T0[2] * U0[2]) + 0.3;
          const double cb = T0[0] * U1[0] + T0[1] * U1[1] + T0[2] * U1[2];
          const double cc = (T1[0] * U1[0] + T1[1] * U1[1] + T1[2] * U1[2]) + 0.3;
          const double denom = ca * cc - cb * cb;
          const double denom2inv = 1.0 / ((denom * denom) + 0.0000001);
          const double dL_da = denom2inv * (-cc * cc * dcx + 2.0 * cb * cc * dcy + (denom - ca * cc) * dcz);
          const double dL_dc = denom2inv * (-ca * ca * dcz + 2.0 * ca * cb * dcy + (denom - ca * cc) * dcx);
          const double dL_db = denom2inv * 2.0 * (cb * cc * dcx - (denom + 2.0 * cb * cb) * dcy + ca * cb * dcz);
          double G0[3], G1[3];   // dL/dT[k][0], dL/dT[k][1]
#pragma unroll
          for (int k = 0; k < 3; k++) {
            G0[k] = 2.0 * U0[k] * dL_da + U1[k] * dL_db;
            G1[k] = 2.0 * U1[k] * dL_dc + U0[k] * dL_db;
          }
          // dL/dW = dL/dT J^T
#pragma unroll
          for (int k = 0; k < 3; k++) {
            tv[3 * k] = G0[k] * J00;
            tv[3 * k + 1] = G1[k] * J11;
            tv[3 * k + 2] = G0[k] * J02 + G1[k] * J12;
          }
          // dL/dJ = W^T dL/dT, then dL/dt
          const double dJ00 = V[0] * G0[0] + V[3] * G0[1] + V[6] * G0[2];
          const double dJ02 = V[2] * G0[0] + V[5] * G0[1] + V[8] * G0[2];
          const double dJ11 = V[1] * G1[0] + V[4] * G1[1] + V[7] * G1[2];
          const double dJ12 = V[2] * G1[0] + V[5] * G1[1] + V[8] * G1[2];
          const double itz = 1.0 / tz, tz2 = itz * itz, tz3 = tz2 * itz;
          gt[0] = xm * -a.fx * tz2 * dJ02;
          gt[1] = ym * -a.fy * tz2 * dJ12;
          gt[2] = (-a.fx * tz2 * dJ00 - a.fy * tz2 * dJ11 + (2.0 * a.fx * txc) * tz3 * dJ02 + (2.0 * a.fy * tyc) * tz3 * dJ12) + gdep;
        }
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
          for (int i = 0; i < 3; i++) tv[3 * k + i] += m[k] * gt[i];
#pragma unroll
        for (int i = 0; i < 3; i++) tv[9 + i] += gt[i];
      }
    }
    // ---- proj: mean2D path (preprocessCUDA backward) ----
    if (a.dL_dmean2D != nullptr) {
      const double g2x = (double)a.dL_dmean2D[i3], g2y = (double)a.dL_dmean2D[i3 + 1];
      if (g2x != 0.0 || g2y != 0.0) {
        const float* Pm = a.proj;
        const double hx = (double)Pm[0] * m[0] + (double)Pm[4] * m[1] + (double)Pm[8] * m[2] + (double)Pm[12];
        const double hy = (double)Pm[1] * m[0] + (double)Pm[5] * m[1] + (double)Pm[9] * m[2] + (double)Pm[13];
        const double hw = (double)Pm[3] * m[0] + (double)Pm[7] * m[1] + (double)Pm[11] * m[2] + (double)Pm[15];
        const double pw = 1.0 / (hw + 0.0000001);
        const double gh[3] = {g2x * pw, g2y * pw, -(hx * g2x + hy * g2y) * pw * pw};
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
          for (int c = 0; c < 3; c++) tp[3 * k + c] = m[k] * gh[c];
#pragma unroll
        for (int c = 0; c < 3; c++) tp[9 + c] = gh[c];
      }
    }
    // ---- campos: SH direction term (backward.cu:20-139, dnormvdv), minus what dL_dmean3D gets ----
    if (a.shs != nullptr && a.dL_dcolor != nullptr) {
      double dRGB[3];
#pragma unroll
      for (int ch = 0; ch < 3; ch++) dRGB[ch] = a.clamped[i3 + ch] ? 0.0 : (double)a.dL_dcolor[i3 + ch];
      if ((dRGB[0] != 0.0 || dRGB[1] != 0.0 || dRGB[2] != 0.0) && a.D > 0) {
        const int deg = a.D;
        const double v[3] = {m[0] - (double)a.campos[0], m[1] - (double)a.campos[1], m[2] - (double)a.campos[2]};
        const double sum2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
        const double len = sqrt(sum2);
        const double x = v[0] / len, y = v[1] / len, z = v[2] / len;
        const float* sh = a.shs + (size_t)idx * a.M * 3;
        double dd[3] = {0.0, 0.0, 0.0};   // dL/d(normalised direction)
#define SH(k) ((double)sh[(k)*3 + ch])
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
          double dRdx = -DSH_C1 * SH(3), dRdy = -DSH_C1 * SH(1), dRdz = DSH_C1 * SH(2);
          if (deg > 1) {
            const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            dRdx += DSH_C2[0] * y * SH(4) + DSH_C2[2] * 2.0 * -x * SH(6) + DSH_C2[3] * z * SH(7) + DSH_C2[4] * 2.0 * x * SH(8);
            dRdy += DSH_C2[0] * x * SH(4) + DSH_C2[1] * z * SH(5) + DSH_C2[2] * 2.0 * -y * SH(6) + DSH_C2[4] * 2.0 * -y * SH(8);
            dRdz += DSH_C2[1] * y * SH(5) + DSH_C2[2] * 2.0 * 2.0 * z * SH(6) + DSH_C2[3] * x * SH(7);
            if (deg > 2) {
              dRdx += (DSH_C3[0] * SH(9) * 3.0 * 2.0 * xy + DSH_C3[1] * SH(10) * yz + DSH_C3[2] * SH(11) * -2.0 * xy +
                       DSH_C3[3] * SH(12) * -3.0 * 2.0 * xz + DSH_C3[4] * SH(13) * (-3.0 * xx + 4.0 * zz - yy) +
                       DSH_C3[5] * SH(14) * 2.0 * xz + DSH_C3[6] * SH(15) * 3.0 * (xx - yy));
              dRdy += (DSH_C3[0] * SH(9) * 3.0 * (xx - yy) + DSH_C3[1] * SH(10) * xz + DSH_C3[2] * SH(11) * (-3.0 * yy + 4.0 * zz - xx) +
                       DSH_C3[3] * SH(12) * -3.0 * 2.0 * yz + DSH_C3[4] * SH(13) * -2.0 * xy + DSH_C3[5] * SH(14) * -2.0 * yz +
                       DSH_C3[6] * SH(15) * -3.0 * 2.0 * xy);
              dRdz += (DSH_C3[1] * SH(10) * xy + DSH_C3[2] * SH(11) * 4.0 * 2.0 * yz + DSH_C3[3] * SH(12) * 3.0 * (2.0 * zz - xx - yy) +
                       DSH_C3[4] * SH(13) * 4.0 * 2.0 * xz + DSH_C3[5] * SH(14) * (xx - yy));
            }
          }
          dd[0] += dRdx * dRGB[ch];
          dd[1] += dRdy * dRGB[ch];
          dd[2] += dRdz * dRGB[ch];
        }
#undef SH
        const double invsum32 = 1.0 / sqrt(sum2 * sum2 * sum2);
        tc[0] = -(((sum2 - v[0] * v[0]) * dd[0] - v[1] * v[0] * dd[1] - v[2] * v[0] * dd[2]) * invsum32);
        tc[1] = -((-v[0] * v[1] * dd[0] + (sum2 - v[1] * v[1]) * dd[1] - v[2] * v[1] * dd[2]) * invsum32);
        tc[2] = -((-v[0] * v[2] * dd[0] - v[1] * v[2] * dd[1] + (sum2 - v[2] * v[2]) * dd[2]) * invsum32);
      }
    }
  }
  if (a.g_dir != nullptr) {
    tc[0] -= (double)a.g_dir[i3];
    tc[1] -= (double)a.g_dir[i3 + 1];
    tc[2] -= (double)a.g_dir[i3 + 2];
  }
}

__global__ void __launch_bounds__(CAM_THREADS) camera_backward_kernel(const CamBwdArgs a) {
  __shared__ double red[4][CAM_SLOTS];
  double acc[CAM_SLOTS];
#pragma unroll
  for (int s = 0; s < CAM_SLOTS; s++) acc[s] = 0.0;
  for (long long base = (long long)blockIdx.x * CAM_THREADS; base < a.P; base += (long long)gridDim.x * CAM_THREADS) {
    const long long idx = base + threadIdx.x;
    if (idx >= a.P) continue;
    double tv[12], tp[12], tc[3];
    camera_terms(a, (int)idx, tv, tp, tc);
#pragma unroll
    for (int s = 0; s < 12; s++) { acc[s] += tv[s]; acc[12 + s] += tp[s]; }
#pragma unroll
    for (int s = 0; s < 3; s++) acc[24 + s] += tc[s];
  }
  // fixed order: xor butterfly inside a wave, then wave 0..3 (alpha.hip::block_sum)
#pragma unroll
  for (int s = 0; s < CAM_SLOTS; s++) {
    double v = acc[s];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][s] = v;
  }
  __syncthreads();
  if (threadIdx.x < CAM_SLOTS) {
    const int s = threadIdx.x;
    a.partial[(size_t)blockIdx.x * CAM_SLOTS + s] = ((red[0][s] + red[1][s]) + red[2][s]) + red[3][s];
  }
}

// One workgroup of 32 groups of 32 lanes: group q adds the partials of workgroups q, q + 32, ... of slot (lane) -- at most 16
// of them, their loads independent of each other --, then lane s of group 0 adds the 32 group sums in order.
__global__ void __launch_bounds__(CAM_FOLD_THREADS) camera_fold_kernel(int nblocks, const double* __restrict__ partial,
                                                                       double* __restrict__ out) {
  __shared__ double red[32][CAM_SLOTS];
  const int s = threadIdx.x & 31, q = threadIdx.x >> 5;
  if (s < CAM_SLOTS) {
    double acc = 0.0;
#pragma unroll 4
    for (int b = q; b < nblocks; b += 32) acc += partial[(size_t)b * CAM_SLOTS + s];
    red[q][s] = acc;
  }
  __syncthreads();
  if (threadIdx.x < CAM_SLOTS) {
    const int t = threadIdx.x;
    double v = red[0][t];
#pragma unroll
    for (int g = 1; g < 32; g++) v += red[g][t];
    out[cam_slot_out(t)] = v;
  } else if (threadIdx.x < S3G_CAMERA_GRAD_DOUBLES) {   // view[3,7,11,15], proj[2,6,10,14]: in no product of the forward
    const int u = threadIdx.x - CAM_SLOTS;              // 0..7
    out[u < 4 ? 4 * u + 3 : 16 + 4 * (u - 4) + 2] = 0.0;
  }
}

// ---- pose map ------------------------------------------------------------------------------------------------------------
// A value with one tangent: the forward kernel ignores d, thread k of the backward kernel seeds d(delta_k) = 1.
struct Dual {
  double v, d;
};
__device__ __forceinline__ Dual dual(double v, double d = 0.0) { Dual r; r.v = v; r.d = d; return r; }
__device__ __forceinline__ Dual operator+(Dual a, Dual b) { return dual(a.v + b.v, a.d + b.d); }
__device__ __forceinline__ Dual operator-(Dual a, Dual b) { return dual(a.v - b.v, a.d - b.d); }
__device__ __forceinline__ Dual operator-(Dual a) { return dual(-a.v, -a.d); }
__device__ __forceinline__ Dual operator*(Dual a, Dual b) { return dual(a.v * b.v, a.d * b.v + a.v * b.d); }
__device__ __forceinline__ Dual operator*(double a, Dual b) { return dual(a * b.v, a * b.d); }
__device__ __forceinline__ Dual operator/(Dual a, Dual b) {
  const double q = a.v / b.v;
  return dual(q, (a.d - q * b.d) / b.v);
}

constexpr double POSE_SERIES_BELOW = 1e-4;   // theta^2: the first dropped terms are theta^8 / 9! and theta^8 / 10!

// view [16], proj [16], campos [3] of the corrected camera; w = omega, tau as Duals.
__device__ __forceinline__ void pose_map(const Dual* w, const Dual* tau, const float* view0, const float* proj0, Dual* view,
                                         Dual* proj, Dual* campos) {
  const Dual s = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];   // theta^2
  Dual A, B;                                                // sin(th)/th, (1 - cos th)/th^2
  if (s.v < POSE_SERIES_BELOW) {
    A = dual(1.0) - (1.0 / 6.0) * s + (1.0 / 120.0) * (s * s) - (1.0 / 5040.0) * (s * s * s);
    B = dual(0.5) - (1.0 / 24.0) * s + (1.0 / 720.0) * (s * s) - (1.0 / 40320.0) * (s * s * s);
  } else {
    const double th = sqrt(s.v);
    const Dual theta = dual(th, s.d / (2.0 * th));
    const double sn = sin(th), cs = cos(th);
    A = dual(sn, cs * theta.d) / theta;
    B = dual(1.0 - cs, sn * theta.d) / s;
  }
  const Dual zero = dual(0.0);
  const Dual Kx[3][3] = {{zero, -w[2], w[1]}, {w[2], zero, -w[0]}, {-w[1], w[0], zero}};
  Dual E[3][3];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) {
      Dual k2 = w[r] * w[c];
      if (r == c) k2 = k2 - s;
      E[r][c] = A * Kx[r][c] + B * k2;
      if (r == c) E[r][c] = dual(1.0) + E[r][c];
    }
  double A0[16], P0[16];
#pragma unroll
  for (int k = 0; k < 16; k++) { A0[k] = (double)view0[k]; P0[k] = (double)proj0[k]; }
  // view' = view0 D^T
#pragma unroll
  for (int r = 0; r < 4; r++) {
#pragma unroll
    for (int c = 0; c < 3; c++)
      view[4 * r + c] = A0[4 * r] * E[c][0] + A0[4 * r + 1] * E[c][1] + A0[4 * r + 2] * E[c][2] + A0[4 * r + 3] * tau[c];
    view[4 * r + 3] = dual(A0[4 * r + 3]);
  }
  // K = view0^-1 proj0, rigid inverse: [R^T 0; -t R^T 1]
  double Ainv[16], K[16];
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int c = 0; c < 3; c++) Ainv[4 * r + c] = A0[4 * c + r];
    Ainv[4 * r + 3] = 0.0;
  }
#pragma unroll
  for (int c = 0; c < 3; c++) Ainv[12 + c] = -(A0[12] * A0[4 * c] + A0[13] * A0[4 * c + 1] + A0[14] * A0[4 * c + 2]);
  Ainv[15] = 1.0;
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 4; c++)
      K[4 * r + c] = Ainv[4 * r] * P0[c] + Ainv[4 * r + 1] * P0[4 + c] + Ainv[4 * r + 2] * P0[8 + c] + Ainv[4 * r + 3] * P0[12 + c];
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 4; c++)
      proj[4 * r + c] = K[c] * view[4 * r] + K[4 + c] * view[4 * r + 1] + K[8 + c] * view[4 * r + 2] + K[12 + c] * view[4 * r + 3];
  // campos' = -t' R'^T
#pragma unroll
  for (int c = 0; c < 3; c++) campos[c] = -(view[12] * view[4 * c] + view[13] * view[4 * c + 1] + view[14] * view[4 * c + 2]);
}

__global__ void __launch_bounds__(64) pose_apply_kernel(const double* __restrict__ delta6, const float* __restrict__ view0,
                                                        const float* __restrict__ proj0, float* __restrict__ view,
                                                        float* __restrict__ proj, float* __restrict__ campos) {
  if (threadIdx.x != 0) return;
  Dual w[3], tau[3], v[16], p[16], c[3];
#pragma unroll
  for (int k = 0; k < 3; k++) { w[k] = dual(delta6[k]); tau[k] = dual(delta6[3 + k]); }
  pose_map(w, tau, view0, proj0, v, p, c);
#pragma unroll
  for (int k = 0; k < 16; k++) { view[k] = (float)v[k].v; proj[k] = (float)p[k].v; }
#pragma unroll
  for (int k = 0; k < 3; k++) campos[k] = (float)c[k].v;
}

__global__ void __launch_bounds__(64) pose_apply_backward_kernel(const double* __restrict__ delta6, const float* __restrict__ view0,
                                                                 const float* __restrict__ proj0, const double* __restrict__ g35,
                                                                 double* __restrict__ g_delta6) {
  const int j = threadIdx.x;
  if (j >= 6) return;
  Dual w[3], tau[3], v[16], p[16], c[3];
#pragma unroll
  for (int k = 0; k < 3; k++) { w[k] = dual(delta6[k], j == k ? 1.0 : 0.0); tau[k] = dual(delta6[3 + k], j == 3 + k ? 1.0 : 0.0); }
  pose_map(w, tau, view0, proj0, v, p, c);
  double g = 0.0;
#pragma unroll
  for (int k = 0; k < 16; k++) g += g35[k] * v[k].d;
#pragma unroll
  for (int k = 0; k < 16; k++) g += g35[16 + k] * p[k].d;
#pragma unroll
  for (int k = 0; k < 3; k++) g += g35[32 + k] * c[k].d;
  g_delta6[j] = g;
}

// The two kernels above for V cameras, one workgroup each: camera blockIdx.x takes row rows[blockIdx.x] of delta [N,6] and slot
// blockIdx.x of every packed array.  The same statements on the same values: each camera's outputs are the single-camera kernels'.
__global__ void __launch_bounds__(64) pose_apply_views_kernel(const double* __restrict__ delta, const int* __restrict__ rows,
                                                              const float* __restrict__ view0s, const float* __restrict__ proj0s,
                                                              float* __restrict__ views, float* __restrict__ projs,
                                                              float* __restrict__ camposs) {
  if (threadIdx.x != 0) return;
  const size_t cam = blockIdx.x;
  const double* delta6 = delta + 6 * (size_t)rows[cam];
  Dual w[3], tau[3], v[16], p[16], c[3];
#pragma unroll
  for (int k = 0; k < 3; k++) { w[k] = dual(delta6[k]); tau[k] = dual(delta6[3 + k]); }
  pose_map(w, tau, view0s + 16 * cam, proj0s + 16 * cam, v, p, c);
#pragma unroll
  for (int k = 0; k < 16; k++) { views[16 * cam + k] = (float)v[k].v; projs[16 * cam + k] = (float)p[k].v; }
#pragma unroll
  for (int k = 0; k < 3; k++) camposs[3 * cam + k] = (float)c[k].v;
}

__global__ void __launch_bounds__(64) pose_apply_backward_views_kernel(const double* __restrict__ delta, const int* __restrict__ rows,
                                                                       const float* __restrict__ view0s,
                                                                       const float* __restrict__ proj0s, const double* __restrict__ g35s,
                                                                       double* __restrict__ g_delta) {
  const int j = threadIdx.x;
  if (j >= 6) return;
  const size_t cam = blockIdx.x;
  const double* delta6 = delta + 6 * (size_t)rows[cam];
  const double* g35 = g35s + S3G_CAMERA_GRAD_DOUBLES * cam;
  Dual w[3], tau[3], v[16], p[16], c[3];
#pragma unroll
  for (int k = 0; k < 3; k++) { w[k] = dual(delta6[k], j == k ? 1.0 : 0.0); tau[k] = dual(delta6[3 + k], j == 3 + k ? 1.0 : 0.0); }
  pose_map(w, tau, view0s + 16 * cam, proj0s + 16 * cam, v, p, c);
  double g = 0.0;
#pragma unroll
  for (int k = 0; k < 16; k++) g += g35[k] * v[k].d;
#pragma unroll
  for (int k = 0; k < 16; k++) g += g35[16 + k] * p[k].d;
#pragma unroll
  for (int k = 0; k < 3; k++) g += g35[32 + k] * c[k].d;
  g_delta[6 * cam + j] = g;
}

}  // namespace s3g

using namespace s3g;

extern "C" size_t s3g_camera_backward_workspace_bytes(int P) {
  if (P <= 0) return 0;
  return ((size_t)cam_blocks(P) * CAM_SLOTS * sizeof(double) + 127) & ~size_t(127);
}

extern "C" int s3g_camera_backward(const s3g_raster_inputs* in, const int* radii, const void* geometry_arena,
                                   const float* dL_dmean2D, const float* dL_dconic, const float* dL_ddepth,
                                   const float* dL_dcolor, const float* g_dir, void* workspace, double* out, void* stream_) {
  clear_error();
  const char* who = "s3g_camera_backward";
  if (!in) {
    set_error("%s: NULL inputs", who);
    return S3G_ERR_INVALID_ARG;
  }
  if (!out || in->P < 0) {
    set_error("%s: bad argument (NULL output or negative P)", who);
    return S3G_ERR_INVALID_ARG;
  }
  hipStream_t stream = (hipStream_t)stream_;
  const int P = in->P;
  if (P == 0) {
    S3G_HIP_CHECK(hipMemsetAsync(out, 0, S3G_CAMERA_GRAD_DOUBLES * sizeof(double), stream));
    return S3G_OK;
  }
  const bool sh = in->shs != nullptr && dL_dcolor != nullptr;
  const bool cov = dL_dconic != nullptr || dL_ddepth != nullptr;
  const bool raster = cov || dL_dmean2D != nullptr || sh;
  if (!workspace || (raster && (!radii || !in->means3D)) || (cov && !in->viewmatrix) ||
      (dL_dconic && !in->cov3D_precomp && !geometry_arena) || (dL_dmean2D && !in->projmatrix) ||
      (sh && (!geometry_arena || !in->cam_pos))) {
    set_error("%s: NULL array argument", who);
    return S3G_ERR_INVALID_ARG;
  }
  if (dL_dconic && (in->width <= 0 || in->height <= 0 || !(in->tan_fovx > 0.f) || !(in->tan_fovy > 0.f))) {
    set_error("%s: the covariance path needs the image size and the field of view", who);
    return S3G_ERR_INVALID_ARG;
  }
  if (sh && (in->D < 0 || in->D > 3 || in->M < (in->D + 1) * (in->D + 1))) {
    set_error("%s: SH degree %d does not fit %d stored coefficients", who, in->D, in->M);
    return S3G_ERR_INVALID_ARG;
  }
  CamBwdArgs a = {};
  a.P = P; a.D = in->D; a.M = in->M; a.means3D = in->means3D; a.radii = raster ? radii : nullptr;
  if (geometry_arena) {
    const GeomState g = GeomState::carve(const_cast<void*>(geometry_arena), (size_t)P, nullptr);
    a.cov3Ds = g.cov3D;
    a.clamped = g.clamped;
  }
  if (in->cov3D_precomp) a.cov3Ds = in->cov3D_precomp;
  a.shs = sh ? in->shs : nullptr;
  a.view = in->viewmatrix; a.proj = in->projmatrix; a.campos = in->cam_pos;
  if (dL_dconic) {
    a.fx = (double)in->width / (2.0 * (double)in->tan_fovx);
    a.fy = (double)in->height / (2.0 * (double)in->tan_fovy);
    a.limx = 1.3 * (double)in->tan_fovx;
    a.limy = 1.3 * (double)in->tan_fovy;
  }
  a.dL_dmean2D = dL_dmean2D; a.dL_dconic = dL_dconic; a.dL_ddepth = dL_ddepth; a.dL_dcolor = sh ? dL_dcolor : nullptr;
  a.g_dir = g_dir;
  a.partial = reinterpret_cast<double*>(workspace);
  const int nb = cam_blocks(P);
  hipLaunchKernelGGL(camera_backward_kernel, dim3(nb), dim3(CAM_THREADS), 0, stream, a);
  S3G_KERNEL_CHECK(stream, in->debug != 0);
  hipLaunchKernelGGL(camera_fold_kernel, dim3(1), dim3(CAM_FOLD_THREADS), 0, stream, nb, a.partial, out);
  S3G_KERNEL_CHECK(stream, in->debug != 0);
  return S3G_OK;
}

extern "C" int s3g_pose_apply(const double* delta6, const float* view0, const float* proj0, float* view, float* proj, float* campos,
                              void* stream_) {
  clear_error();
  if (!delta6 || !view0 || !proj0 || !view || !proj || !campos) {
    set_error("s3g_pose_apply: NULL array argument");
    return S3G_ERR_INVALID_ARG;
  }
  hipLaunchKernelGGL(pose_apply_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream_, delta6, view0, proj0, view, proj, campos);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" int s3g_pose_apply_backward(const double* delta6, const float* view0, const float* proj0, const double* g35,
                                       double* g_delta6, void* stream_) {
  clear_error();
  if (!delta6 || !view0 || !proj0 || !g35 || !g_delta6) {
    set_error("s3g_pose_apply_backward: NULL array argument");
    return S3G_ERR_INVALID_ARG;
  }
  hipLaunchKernelGGL(pose_apply_backward_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream_, delta6, view0, proj0, g35, g_delta6);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" int s3g_pose_apply_views(int V, const double* delta, const int* rows, const float* view0s, const float* proj0s,
                                    float* views, float* projs, float* camposs, void* stream_) {
  clear_error();
  if (V < 0 || (V > 0 && (!delta || !rows || !view0s || !proj0s || !views || !projs || !camposs))) {
    set_error("s3g_pose_apply_views: negative V or NULL array argument");
    return S3G_ERR_INVALID_ARG;
  }
  if (V == 0) return S3G_OK;
  hipLaunchKernelGGL(pose_apply_views_kernel, dim3(V), dim3(64), 0, (hipStream_t)stream_, delta, rows, view0s, proj0s, views, projs,
                     camposs);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" int s3g_pose_apply_backward_views(int V, const double* delta, const int* rows, const float* view0s, const float* proj0s,
                                             const double* g35, double* g_delta, void* stream_) {
  clear_error();
  if (V < 0 || (V > 0 && (!delta || !rows || !view0s || !proj0s || !g35 || !g_delta))) {
    set_error("s3g_pose_apply_backward_views: negative V or NULL array argument");
    return S3G_ERR_INVALID_ARG;
  }
  if (V == 0) return S3G_OK;
  hipLaunchKernelGGL(pose_apply_backward_views_kernel, dim3(V), dim3(64), 0, (hipStream_t)stream_, delta, rows, view0s, proj0s, g35,
                     g_delta);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}
