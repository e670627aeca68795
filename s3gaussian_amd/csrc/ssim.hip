// Photometric loss stage for gfx950: SSIM (11x11 Gaussian window, sigma 1.5, zero padding) forward + backward, with the
// per-pixel L1 / depth / feature terms folded into the same two launches (s3g_photometric_*).
// Reference: utils/loss_utils.py:56-96 = 5 grouped conv2d + ~15 elementwise kernels forward, the same again backward
// (on MI355X MIOpen picks miopenSp3AsmConv for the grouped 11x11 convolutions: ~13 ms per step at 1066x1600).
// Here: one kernel per direction.  A WAVE owns a strip of SS_SW columns x SS_RH rows of one channel and walks down its
// SS_RH + 10 input rows: each row goes through a wave-private LDS row buffer (no workgroup barrier) for the 11-tap
// horizontal sums, a register ring of the last 11 rows of sums gives the vertical sums.  Per pixel the arithmetic is the
// window of make_window(), taps k = 0..10 accumulated from 0 as mul then add, horizontally and then vertically, no FMA.
#include "common.hpp"

#include "../../include/s3g_loss.h"

namespace s3g {

constexpr int SS_R = 5;                       // window radius
constexpr int SS_SW = 64;                     // strip width: one lane per column
constexpr int SS_RH = 21;                     // output rows per wave: 31 input rows, 3825 waves at 1066 x 1600 x 3
constexpr int SS_WAVES = 8;                   // waves per workgroup, each on a strip of its own
constexpr int SS_PITCH = SS_SW + 2 * SS_R + 6;  // one staged row: 74 floats, padded to 80

struct SsimWindow {
  float g[11];
};
static SsimWindow make_window() {  // gaussian(11, 1.5), loss_utils.py:56-58, computed in fp32 like torch.Tensor([...])
  SsimWindow w;
  float s = 0.f;
  for (int x = 0; x < 11; x++) {
    w.g[x] = (float)exp(-(double)((x - 5) * (x - 5)) / (2.0 * 1.5 * 1.5));
    s += w.g[x];
  }
  for (int x = 0; x < 11; x++) w.g[x] /= s;
  return w;
}

// Where a wave works: strips are numbered x fastest, then y, then channel; the divisions happen once per wave.
struct Strip {
  int c, x0, y0;
  int nrows;  // input rows walked: output rows + 2 * SS_R; 0 = no strip for this wave
};
__device__ __forceinline__ Strip locate_strip(int C, int H, int W) {
  const int sx = (W + SS_SW - 1) / SS_SW, sy = (H + SS_RH - 1) / SS_RH;
  const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * SS_WAVES + (threadIdx.x >> 6)));
  Strip s;
  s.c = wave / (sx * sy);
  const int rem = wave - s.c * (sx * sy), ys = rem / sx;
  s.x0 = (rem - ys * sx) * SS_SW;
  s.y0 = ys * SS_RH;
  s.nrows = s.c < C ? min(SS_RH, H - s.y0) + 2 * SS_R : 0;
  return s;
}
static int strip_workgroups(int C, int H, int W) {
  const int waves = C * ((W + SS_SW - 1) / SS_SW) * ((H + SS_RH - 1) / SS_RH);
  return (waves + SS_WAVES - 1) / SS_WAVES;
}

// A lane's columns: its own (gx -> staged[lane + SS_R]) and, for lanes 0..9, one of the ten halo columns (hx -> staged[hj]).
// staged[j] holds column x0 - SS_R + j; lane l reads staged[l + k] for tap k.  Bounds are decided here, once per column.
struct LaneCols {
  int gx, hx, hj;
  bool colok, hok, halo;
};
__device__ __forceinline__ LaneCols lane_columns(int lane, int x0, int W) {
  LaneCols q;
  q.gx = x0 + lane;
  q.colok = q.gx < W;
  q.halo = lane < 2 * SS_R;
  q.hx = lane < SS_R ? x0 - SS_R + lane : x0 + SS_SW - SS_R + lane;
  q.hj = lane < SS_R ? lane : SS_SW + lane;
  q.hok = q.halo && q.hx >= 0 && q.hx < W;
  return q;
}

// The staged row is written by some lanes and read by others of the same wave.  A wave's LDS instructions execute in
// order, so no hardware wait is needed; the fence keeps the compiler from moving the accesses across each other.
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

struct SsimFwdArgs {
  int C, H, W;
  const float *img1, *img2;
  SsimWindow win;
  double* sums;                     // slotted accumulator [0] (SSIM map); fused: the five of s3g_loss.h
  float *m_mu1, *m_s11, *m_s12;
  // fused pixel terms (C == 3): channel c's waves take feature channel c, channel 0's also the depth
  const float *depth, *gt_depth, *feat, *gt_feat;
  float max_depth;
};

template <int P>
struct RingSlot {
  static constexpr int value = P;
};

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <bool FUSED>
__global__ void __launch_bounds__(SS_WAVES * 64) ssim_strip_forward_kernel(const SsimFwdArgs a) {
  __shared__ float stage[SS_WAVES][2][SS_PITCH];
  const Strip s = locate_strip(a.C, a.H, a.W);
  if (s.nrows == 0) return;
  const int H = a.H, W = a.W, lane = threadIdx.x & 63;
  const LaneCols q = lane_columns(lane, s.x0, W);
  float* const bu = stage[threadIdx.x >> 6][0];
  float* const bv = stage[threadIdx.x >> 6][1];
  const size_t plane = (size_t)s.c * H * W;
  const float *p1 = a.img1 + plane, *p2 = a.img2 + plane;
  const bool do_depth = FUSED && s.c == 0 && a.depth != nullptr, do_feat = FUSED && a.feat != nullptr;

  // one input row: the lane's pixel of both images, its halo pixel, and on the strip's own rows the pixel-term inputs
  struct Row {
    float u, v, hu, hv, d, gd, f, gf;
  };
  auto fetch = [&](int r, Row& n) {
    const int gy = s.y0 - SS_R + r;
    if (r < s.nrows && gy >= 0 && gy < H) {  // uniform
      const size_t ro = (size_t)gy * W;
      n.u = q.colok ? p1[ro + q.gx] : 0.f;
      n.v = q.colok ? p2[ro + q.gx] : 0.f;
      n.hu = q.hok ? p1[ro + q.hx] : 0.f;
      n.hv = q.hok ? p2[ro + q.hx] : 0.f;
      if (FUSED && r >= SS_R && r < s.nrows - SS_R && q.colok) {
        if (do_depth) { n.d = a.depth[ro + q.gx]; n.gd = a.gt_depth[ro + q.gx]; }
        if (do_feat) { n.f = a.feat[plane + ro + q.gx]; n.gf = a.gt_feat[plane + ro + q.gx]; }
      }
    }
  };

  float ring[11][5];
  double vsum = 0.0, l1 = 0.0, dsq = 0.0, fsq = 0.0;   // per-lane sums in double: a total is then the double sum of the fp32 pixel values
  float cnt = 0.f;
  const Row kNoRow = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  Row cur = kNoRow;
  fetch(0, cur);
  // one input row; p = r % 11 is the row's ring slot, a compile-time constant so that the ring stays in registers
  auto step = [&](auto slot, int r) {
    constexpr int p = decltype(slot)::value;
    {
      if (r >= s.nrows) return;                // uniform
      const int gy = s.y0 - SS_R + r;
      const bool rowin = gy >= 0 && gy < H;    // uniform
      if (rowin) {
        bu[lane + SS_R] = cur.u;
        bv[lane + SS_R] = cur.v;
        if (q.halo) { bu[q.hj] = cur.hu; bv[q.hj] = cur.hv; }
      }
      Row nxt = kNoRow;
      fetch(r + 1, nxt);                       // in flight during this row's arithmetic
      wave_lds_fence();
      float ha = 0.f, hb = 0.f, haa = 0.f, hbb = 0.f, hab = 0.f;
      if (rowin) {                             // a row outside the image sums to +0 in every quantity
#pragma unroll
        for (int k = 0; k < 11; k++) {
          const float w = a.win.g[k], u = bu[lane + k], v = bv[lane + k];
          ha += w * u; hb += w * v; haa += w * (u * u); hbb += w * (v * v); hab += w * (u * v);
        }
      }
      wave_lds_fence();
      ring[p][0] = ha; ring[p][1] = hb; ring[p][2] = haa; ring[p][3] = hbb; ring[p][4] = hab;
      if (FUSED && r >= SS_R && r < s.nrows - SS_R && q.colok) {   // the strip's own rows: all inside the image
        l1 += (double)fabsf(cur.u - cur.v);
        if (do_depth) {
          const float gd = cur.gd;
          if (gd > 0.01f && gd < a.max_depth) {
            const float cp = fminf(fmaxf(cur.d / a.max_depth, 0.f), 1.f), cg = fminf(fmaxf(gd / a.max_depth, 0.f), 1.f);
            dsq += (double)((cp - cg) * (cp - cg));
            cnt += 1.f;
          }
        }
        if (do_feat) {
          const float d = cur.f - cur.gf;
          fsq += (double)(d * d);
        }
      }
      if (r >= 2 * SS_R) {                     // ring full: emit output row gy - SS_R (inside the image by construction)
        float mu1 = 0.f, mu2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
        for (int k = 0; k < 11; k++) {
          const float w = a.win.g[k];
          const float* h = ring[(p + 1 + k) % 11];
          mu1 += w * h[0]; mu2 += w * h[1]; e11 += w * h[2]; e22 += w * h[3]; e12 += w * h[4];
        }
        if (q.colok) {
          const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
          const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
          const float s11 = e11 - mu1_sq, s22 = e22 - mu2_sq, s12 = e12 - mu12;
          const float aa = 2.f * mu12 + C1, b = 2.f * s12 + C2, cc = mu1_sq + mu2_sq + C1, d = s11 + s22 + C2;
          const float inv = 1.f / (cc * d);
          const float val = (aa * b) * inv;
          const float dm_ds11 = -val / d;                 // d map / d sigma1_sq
          const float dm_ds12 = 2.f * aa * inv;           // d map / d sigma12
          const float dm_dmu1 = 2.f * mu2 * b * inv - 2.f * mu1 * val / cc + dm_ds11 * (-2.f * mu1) + dm_ds12 * (-mu2);
          const size_t o = plane + (size_t)(gy - SS_R) * W + q.gx;
          a.m_mu1[o] = dm_dmu1; a.m_s11[o] = dm_ds11; a.m_s12[o] = dm_ds12;
          vsum += (double)val;
        }
      }
      cur = nxt;
    }
  };
  for (int base = 0; base < s.nrows; base += 11) {
    step(RingSlot<0>{}, base); step(RingSlot<1>{}, base + 1); step(RingSlot<2>{}, base + 2); step(RingSlot<3>{}, base + 3);
    step(RingSlot<4>{}, base + 4); step(RingSlot<5>{}, base + 5); step(RingSlot<6>{}, base + 6); step(RingSlot<7>{}, base + 7);
    step(RingSlot<8>{}, base + 8); step(RingSlot<9>{}, base + 9); step(RingSlot<10>{}, base + 10);
  }
  vsum = wave_sum(vsum);
  const unsigned wave = blockIdx.x * SS_WAVES + (threadIdx.x >> 6);
  double* slot = a.sums + (wave % S3G_SUM_SLOTS) * S3G_SUM_STRIDE;
  if (FUSED) {
    const double s1 = wave_sum(l1), s2 = wave_sum(dsq), s3 = wave_sum((double)cnt), s4 = wave_sum(fsq);
    if (lane == 0) {
      atomicAdd(&slot[1 * S3G_SUM_DOUBLES], s1);
      if (do_depth) { atomicAdd(&slot[2 * S3G_SUM_DOUBLES], s2); atomicAdd(&slot[3 * S3G_SUM_DOUBLES], s3); }
      if (do_feat) atomicAdd(&slot[4 * S3G_SUM_DOUBLES], s4);
    }
  }
  if (lane == 0) atomicAdd(&slot[0], vsum);
}

struct SsimBwdArgs {
  int C, H, W;
  const float *img1, *img2;
  SsimWindow win;
  const float *m_mu1, *m_s11, *m_s12;
  const float* g;                   // device scalar; the upstream gradient of the mean SSIM is g[0] * gmul
  float gmul;
  float* g_image;
  // fused pixel terms (C == 3), as pixel_loss_backward_kernel below
  const float *depth, *gt_depth, *feat, *gt_feat;
  float max_depth;
  const double* totals;
  float w_l1, w_depth, w_feat;
  float *g_depth, *g_feat;
};

template <bool FUSED>
__global__ void __launch_bounds__(SS_WAVES * 64) ssim_strip_backward_kernel(const SsimBwdArgs a) {
  __shared__ float stage[SS_WAVES][3][SS_PITCH];
  const Strip s = locate_strip(a.C, a.H, a.W);
  if (s.nrows == 0) return;
  const int H = a.H, W = a.W, lane = threadIdx.x & 63;
  const LaneCols q = lane_columns(lane, s.x0, W);
  float* const b0 = stage[threadIdx.x >> 6][0];
  float* const b1 = stage[threadIdx.x >> 6][1];
  float* const b2 = stage[threadIdx.x >> 6][2];
  const size_t plane = (size_t)s.c * H * W;
  const float *m0 = a.m_mu1 + plane, *m1 = a.m_s11 + plane, *m2 = a.m_s12 + plane;
  const float *p1 = a.img1 + plane, *p2 = a.img2 + plane;
  const bool do_depth = FUSED && s.c == 0 && a.g_depth != nullptr, do_feat = FUSED && a.g_feat != nullptr;
  const float scale = (a.g[0] * a.gmul) / (float)((size_t)a.C * H * W);
  float k_l1 = 0.f, k_feat = 0.f, k_depth = 0.f;
  if (FUSED) {
    const float g = a.g[0];
    const int HW = H * W;
    k_l1 = g * a.w_l1 / (3.0f * (float)HW);
    k_feat = g * a.w_feat * 2.0f / (3.0f * (float)HW);
    // empty mask: the reference's mean over zero elements is NaN and so is its gradient; 0/0 reproduces that
    k_depth = a.g_depth != nullptr ? g * a.w_depth * 2.0f / ((float)a.totals[3] * a.max_depth) : 0.f;
  }

  // one input row of the three maps (own column + halo column), and the pixels of the output row emitted with it
  struct Row {
    float t0, t1, t2, h0, h1, h2;
    float x1, x2, d, gd, f, gf;
  };
  auto fetch = [&](int r, Row& n) {
    const int gy = s.y0 - SS_R + r;
    if (r < s.nrows && gy >= 0 && gy < H) {  // uniform
      const size_t ro = (size_t)gy * W;
      n.t0 = q.colok ? m0[ro + q.gx] : 0.f;
      n.t1 = q.colok ? m1[ro + q.gx] : 0.f;
      n.t2 = q.colok ? m2[ro + q.gx] : 0.f;
      n.h0 = q.hok ? m0[ro + q.hx] : 0.f;
      n.h1 = q.hok ? m1[ro + q.hx] : 0.f;
      n.h2 = q.hok ? m2[ro + q.hx] : 0.f;
    }
    if (r >= 2 * SS_R && r < s.nrows && q.colok) {  // output row gy - SS_R: inside the image by construction
      const size_t oo = (size_t)(gy - SS_R) * W + q.gx;
      n.x1 = p1[oo];
      n.x2 = p2[oo];
      if (do_depth) { n.d = a.depth[oo]; n.gd = a.gt_depth[oo]; }
      if (do_feat) { n.f = a.feat[plane + oo]; n.gf = a.gt_feat[plane + oo]; }
    }
  };

  float ring[11][3];
  const Row kNoRow = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  Row cur = kNoRow;
  fetch(0, cur);
  // one input row; p = r % 11 is the row's ring slot, a compile-time constant so that the ring stays in registers
  auto step = [&](auto slot, int r) {
    constexpr int p = decltype(slot)::value;
    {
      if (r >= s.nrows) return;                // uniform
      const int gy = s.y0 - SS_R + r;
      const bool rowin = gy >= 0 && gy < H;    // uniform
      if (rowin) {
        b0[lane + SS_R] = cur.t0;
        b1[lane + SS_R] = cur.t1;
        b2[lane + SS_R] = cur.t2;
        if (q.halo) { b0[q.hj] = cur.h0; b1[q.hj] = cur.h1; b2[q.hj] = cur.h2; }
      }
      Row nxt = kNoRow;
      fetch(r + 1, nxt);                       // in flight during this row's arithmetic
      wave_lds_fence();
      float ha = 0.f, hb = 0.f, hd = 0.f;
      if (rowin) {                             // a row outside the image sums to +0
#pragma unroll
        for (int k = 0; k < 11; k++) {
          const float w = a.win.g[k];
          ha += w * b0[lane + k]; hb += w * b1[lane + k]; hd += w * b2[lane + k];
        }
      }
      wave_lds_fence();
      ring[p][0] = ha; ring[p][1] = hb; ring[p][2] = hd;
      if (r >= 2 * SS_R) {
        float A = 0.f, B = 0.f, D = 0.f;
#pragma unroll
        for (int k = 0; k < 11; k++) {
          const float w = a.win.g[k];
          const float* h = ring[(p + 1 + k) % 11];
          A += w * h[0]; B += w * h[1]; D += w * h[2];
        }
        if (q.colok) {
          const size_t oo = (size_t)(gy - SS_R) * W + q.gx;
          float out = scale * (A + 2.f * cur.x1 * B + cur.x2 * D);
          if (FUSED) {
            const float d = cur.x1 - cur.x2;
            const float v = d > 0.f ? k_l1 : (d < 0.f ? -k_l1 : 0.f);
            out = out + v;                     // SSIM term + L1 term, the order of the accumulate_image path
            if (do_depth) {
              const float gd = cur.gd, x = cur.d / a.max_depth;
              float gv = 0.f;
              if (gd > 0.01f && gd < a.max_depth && x >= 0.f && x <= 1.f)  // clamp passes the gradient on its closed interval
                gv = k_depth * (x - fminf(fmaxf(gd / a.max_depth, 0.f), 1.f));
              a.g_depth[oo] = gv;
            }
            if (do_feat) a.g_feat[plane + oo] = k_feat * (cur.f - cur.gf);
          }
          a.g_image[plane + oo] = out;
        }
      }
      cur = nxt;
    }
  };
  for (int base = 0; base < s.nrows; base += 11) {
    step(RingSlot<0>{}, base); step(RingSlot<1>{}, base + 1); step(RingSlot<2>{}, base + 2); step(RingSlot<3>{}, base + 3);
    step(RingSlot<4>{}, base + 4); step(RingSlot<5>{}, base + 5); step(RingSlot<6>{}, base + 6); step(RingSlot<7>{}, base + 7);
    step(RingSlot<8>{}, base + 8); step(RingSlot<9>{}, base + 9); step(RingSlot<10>{}, base + 10);
  }
}

}  // namespace s3g

using namespace s3g;

extern "C" int s3g_ssim_forward(int C, int H, int W, const float* img1, const float* img2, double* ssim_sum, float* dm_dmu1,
                                float* dm_dsigma1_sq, float* dm_dsigma12, void* stream_) {
  if (C <= 0 || H <= 0 || W <= 0 || !img1 || !img2 || !ssim_sum || !dm_dmu1 || !dm_dsigma1_sq || !dm_dsigma12) {
    set_error("s3g_ssim_forward: bad argument");
    return S3G_ERR_INVALID_ARG;
  }
  static const SsimWindow win = make_window();
  SsimFwdArgs a;
  memset(&a, 0, sizeof a);
  a.C = C; a.H = H; a.W = W; a.img1 = img1; a.img2 = img2; a.win = win; a.sums = ssim_sum;
  a.m_mu1 = dm_dmu1; a.m_s11 = dm_dsigma1_sq; a.m_s12 = dm_dsigma12;
  hipLaunchKernelGGL(ssim_strip_forward_kernel<false>, dim3(strip_workgroups(C, H, W)), dim3(SS_WAVES * 64), 0,
                     (hipStream_t)stream_, a);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" int s3g_ssim_backward(int C, int H, int W, const float* img1, const float* img2, const float* dm_dmu1,
                                 const float* dm_dsigma1_sq, const float* dm_dsigma12, const float* dL_dmean,
                                 float* dL_dimg1, void* stream_) {
  if (C <= 0 || H <= 0 || W <= 0 || !img1 || !img2 || !dm_dmu1 || !dm_dsigma1_sq || !dm_dsigma12 || !dL_dmean || !dL_dimg1) {
    set_error("s3g_ssim_backward: bad argument");
    return S3G_ERR_INVALID_ARG;
  }
  static const SsimWindow win = make_window();
  SsimBwdArgs a;
  memset(&a, 0, sizeof a);
  a.C = C; a.H = H; a.W = W; a.img1 = img1; a.img2 = img2; a.win = win;
  a.m_mu1 = dm_dmu1; a.m_s11 = dm_dsigma1_sq; a.m_s12 = dm_dsigma12; a.g = dL_dmean; a.gmul = 1.0f; a.g_image = dL_dimg1;
  hipLaunchKernelGGL(ssim_strip_backward_kernel<false>, dim3(strip_workgroups(C, H, W)), dim3(SS_WAVES * 64), 0,
                     (hipStream_t)stream_, a);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" int s3g_photometric_forward(int H, int W, const float* image, const float* gt_image, const float* depth,
                                       const float* gt_depth, const float* feat, const float* gt_feat, float max_depth,
                                       double* sums, float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12, void* stream_) {
  if (H <= 0 || W <= 0 || !image || !gt_image || !sums || !dm_dmu1 || !dm_dsigma1_sq || !dm_dsigma12 || (depth && !gt_depth) ||
      (feat && !gt_feat)) {
    set_error("s3g_photometric_forward: bad argument");
    return S3G_ERR_INVALID_ARG;
  }
  static const SsimWindow win = make_window();
  SsimFwdArgs a;
  memset(&a, 0, sizeof a);
  a.C = 3; a.H = H; a.W = W; a.img1 = image; a.img2 = gt_image; a.win = win; a.sums = sums;
  a.m_mu1 = dm_dmu1; a.m_s11 = dm_dsigma1_sq; a.m_s12 = dm_dsigma12;
  a.depth = depth; a.gt_depth = gt_depth; a.feat = feat; a.gt_feat = gt_feat; a.max_depth = max_depth;
  hipLaunchKernelGGL(ssim_strip_forward_kernel<true>, dim3(strip_workgroups(3, H, W)), dim3(SS_WAVES * 64), 0,
                     (hipStream_t)stream_, a);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" int s3g_photometric_backward(int H, int W, const float* image, const float* gt_image, const float* depth,
                                        const float* gt_depth, const float* feat, const float* gt_feat, float max_depth,
                                        const float* dm_dmu1, const float* dm_dsigma1_sq, const float* dm_dsigma12,
                                        const double* totals, const float* g, float w_ssim, float w_l1, float w_depth,
                                        float w_feat, float* g_image, float* g_depth, float* g_feat, void* stream_) {
  if (H <= 0 || W <= 0 || !image || !gt_image || !dm_dmu1 || !dm_dsigma1_sq || !dm_dsigma12 || !totals || !g || !g_image ||
      (g_depth && (!depth || !gt_depth)) || (g_feat && (!feat || !gt_feat))) {
    set_error("s3g_photometric_backward: bad argument");
    return S3G_ERR_INVALID_ARG;
  }
  static const SsimWindow win = make_window();
  SsimBwdArgs a;
  memset(&a, 0, sizeof a);
  a.C = 3; a.H = H; a.W = W; a.img1 = image; a.img2 = gt_image; a.win = win;
  a.m_mu1 = dm_dmu1; a.m_s11 = dm_dsigma1_sq; a.m_s12 = dm_dsigma12; a.g = g; a.gmul = -w_ssim; a.g_image = g_image;
  a.depth = depth; a.gt_depth = gt_depth; a.feat = feat; a.gt_feat = gt_feat; a.max_depth = max_depth; a.totals = totals;
  a.w_l1 = w_l1; a.w_depth = w_depth; a.w_feat = w_feat; a.g_depth = g_depth; a.g_feat = g_feat;
  hipLaunchKernelGGL(ssim_strip_backward_kernel<true>, dim3(strip_workgroups(3, H, W)), dim3(SS_WAVES * 64), 0,
                     (hipStream_t)stream_, a);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}
