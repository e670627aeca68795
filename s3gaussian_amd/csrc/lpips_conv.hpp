// The layer machinery both LPIPS variants share (lpips.hip: AlexNet, lpips_vgg.hip: VGG16): the layer description and the blob
// layout that follows from it, the convolution and pool kernels, and one launch helper per kernel.  Each variant keeps its own layer
// table, plan and walk.  A convolution is ONE implicit GEMM with 2 Ho Wo rows (pixels), co columns and K = ks ks ci ordered
// (kh, kw, ci):
//   conv kernel   256 threads own 128 pixels x BN channels; K is staged 32 at a time through two LDS buffers (registers hold the
//                 next step's global loads while the matrix pipe works on the current one).  BN = 64: a wave per 32 pixels, two
//                 tiles of v_mfma_f32_32x32x2_f32 side by side.  BN = 128: the four waves sit 2 x 2, each multiplies 64 pixels by
//                 64 channels as 2 x 2 tiles, so an A tile is gathered by co / 128 workgroups and four matrix instructions share
//                 four LDS reads.  Every output is an exact k-ordered fp32 fma chain; bias and ReLU in the epilogue.
//   pool kernel   WIN x WIN stride 2, floor mode, one float4 of channels per thread.
#pragma once
#include "lpips_dev.hpp"

namespace s3g {

constexpr int LP_BM = 128, LP_BK = 32;   // block tile: pixels, K step

struct LpLayer {
  int ks, stride, pad, ci, co;
  int tap;    // the index of the tap after this layer's ReLU, or -1
  int pool;   // the window of the stride-2 pool that follows, or 0
};
constexpr int lp_k(const LpLayer* T, int l) { return T[l].ks * T[l].ks * T[l].ci; }
constexpr int lp_kpad(const LpLayer* T, int l) { return (lp_k(T, l) + LP_BK - 1) / LP_BK * LP_BK; }
// blob, per conv: B [kpad][co], bias [co], and after a tapped conv its lin weights [co]; every piece is a multiple of 64 floats
constexpr size_t lp_layer_floats(const LpLayer* T, int l) {
  return (size_t)lp_kpad(T, l) * T[l].co + (size_t)T[l].co * (T[l].tap >= 0 ? 2 : 1);
}
constexpr size_t lp_layer_offset(const LpLayer* T, int l) { return l == 0 ? 0 : lp_layer_offset(T, l - 1) + lp_layer_floats(T, l - 1); }

// where a conv kernel's A operand comes from
enum LpSrc {
  LP_SRC_ACT,      // in0: activations [2][Hi][Wi][CI]
  LP_SRC_PLANAR,   // in0, in1: the two images [3][Hi][Wi], z-scored as they are gathered (AlexNet conv1)
  LP_SRC_PIXEL4    // in0: z-scored pixels [2][Hi][Wi] float4 {z0, z1, z2, 0} (VGG conv1_1, after lpips_vgg_front_kernel)
};

// Half a K step of a planar first layer: k = k0 + j, j < 16, is channel k % CI of tap k / CI; k >= K pads K with zeros.
// Zero padding applies after the z-score; so does the padding of K.
template <int KS, int CI>
__device__ __forceinline__ void lp_gather_planar(bool mvalid, int Hi, int Wi, int iy0, int ix0, int k0, const float* __restrict__ src,
                                                 float (&a_reg)[16]) {
  constexpr int K = KS * KS * CI;
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const int k = k0 + j;
    const int kh = k / (KS * CI), rem = k - kh * (KS * CI), kw = rem / CI, c = rem - kw * CI;
    const int iy = iy0 + kh, ix = ix0 + kw;
    float v = 0.f;
    if (mvalid && k < K && iy >= 0 && iy < Hi && ix >= 0 && ix < Wi) v = lp_zscore(src[(size_t)c * Hi * Wi + (size_t)iy * Wi + ix], c);
    a_reg[j] = v;
  }
}

__device__ __forceinline__ float lp_comp(const float4 v, int c) { return c == 0 ? v.x : (c == 1 ? v.y : v.z); }

// Half KQ of the only K step of a 3x3 pad-1 first layer over float4 pixels: k = 16 KQ + j, j < 16, is channel k % 3 of tap k / 3;
// k >= 27 pads K with zeros.  An out-of-image tap contributes 0.
template <int KQ>
__device__ __forceinline__ void lp_gather_pixel4(bool mvalid, int H, int W, int oy, int ox, const float4* __restrict__ src,
                                                 float (&a_reg)[16]) {
  constexpr int T0 = KQ * 16 / 3, T1 = (KQ * 16 + 15) / 3 < 8 ? (KQ * 16 + 15) / 3 : 8;
  float4 px[T1 - T0 + 1];
#pragma unroll
  for (int t = T0; t <= T1; t++) {
    const int iy = oy + t / 3 - 1, ix = ox + t % 3 - 1;
    px[t - T0] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (mvalid && iy >= 0 && iy < H && ix >= 0 && ix < W) px[t - T0] = src[(size_t)iy * W + ix];
  }
#pragma unroll
  for (int j = 0; j < 16; j++) {
    constexpr int K0 = KQ * 16;
    const int t = (K0 + j) / 3 < T1 ? (K0 + j) / 3 : T1;
    a_reg[j] = K0 + j < 27 ? lp_comp(px[t - T0], (K0 + j) % 3) : 0.f;
  }
}

// in0, in1: see LpSrc (in1 is read by LP_SRC_PLANAR only).  out: [2][Ho][Wo][CO].  Bmat: [KPAD][CO].
// Workgroup b owns pixel tile b / (CO/BN) and channel tile b % (CO/BN): the workgroups that gather one A tile are neighbours.
template <int KS, int STRIDE, int PAD, int CI, int CO, int BN, LpSrc SRC>
__global__ void __launch_bounds__(256) lpips_conv_kernel(int Hi, int Wi, int Ho, int Wo, const float* __restrict__ in0,
                                                         const float* __restrict__ in1, const float* __restrict__ Bmat,
                                                         const float* __restrict__ bias, float* __restrict__ out) {
  constexpr int K = KS * KS * CI, KPAD = (K + LP_BK - 1) / LP_BK * LP_BK, STEPS = KPAD / LP_BK, NT = CO / BN;
  constexpr int WN = BN / 64, WM = 4 / WN, TM = LP_BM / WM / 32;   // waves WM x WN, each TM x 2 tiles of 32 x 32
  constexpr int BTPR = BN / 4, BROWS = 256 / BTPR, NB = LP_BK / BROWS;     // B staging: float4s per row, rows per pass, passes
  static_assert((BN == 64 && NB == 2) || (BN == 128 && NB == 4), "one or two wave columns of 64 channels");
  static_assert(CO % BN == 0, "channel tiles are whole");
  static_assert(SRC != LP_SRC_ACT || CI % LP_BK == 0, "a K step lies inside one (kh, kw) tap");
  static_assert(SRC != LP_SRC_PIXEL4 || (KS == 3 && STRIDE == 1 && PAD == 1 && CI == 3 && STEPS == 1), "what lp_gather_pixel4 gathers");
  __shared__ float As[2][LP_BK][LP_BM];   // [k][pixel]: the lanes of an operand read are consecutive words
  __shared__ float Bs[2][LP_BK][BN];      // [k][channel]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, r = lane & 31;
  const int wm = wave / WN, wn = wave % WN;
  const int nt = blockIdx.x % NT, mt = blockIdx.x / NT;
  const int HW = Ho * Wo, M = 2 * HW;
  // staging role: pixel p of the tile, K half kq of the step (16 consecutive k)
  const int p = tid & (LP_BM - 1), kq = tid >> 7;
  const int m = mt * LP_BM + p;
  const bool mvalid = m < M;
  int img = 0, oy = 0, ox = 0;
  if (mvalid) {
    img = m / HW;
    const int rem = m - img * HW;
    oy = rem / Wo;
    ox = rem - oy * Wo;
  }
  const int iy0 = oy * STRIDE - PAD, ix0 = ox * STRIDE - PAD;
  const float* src = SRC == LP_SRC_PLANAR ? (img ? in1 : in0) : in0 + (size_t)img * Hi * Wi * (SRC == LP_SRC_PIXEL4 ? 4 : CI);
  const int brow = tid / BTPR, bcol = (tid % BTPR) * 4;
  float a_reg[16];
  float4 b_reg0, b_reg1, b_reg2, b_reg3;   // NB = 2 uses the first two

  auto load = [&](int step) __attribute__((always_inline)) {
    const int k0 = step * LP_BK;
    if constexpr (SRC == LP_SRC_PLANAR) {
      lp_gather_planar<KS, CI>(mvalid, Hi, Wi, iy0, ix0, k0 + kq * 16, src, a_reg);
    } else if constexpr (SRC == LP_SRC_PIXEL4) {
      if (kq == 0)   // uniform over the wave
        lp_gather_pixel4<0>(mvalid, Hi, Wi, oy, ox, reinterpret_cast<const float4*>(src), a_reg);
      else
        lp_gather_pixel4<1>(mvalid, Hi, Wi, oy, ox, reinterpret_cast<const float4*>(src), a_reg);
    } else {
      const int tap = k0 / CI, c0 = k0 - tap * CI + kq * 16;
      const int kh = tap / KS, kw = tap - kh * KS;
      const int iy = iy0 + kh, ix = ix0 + kw;
      if (mvalid && iy >= 0 && iy < Hi && ix >= 0 && ix < Wi) {
        const float4* q = reinterpret_cast<const float4*>(src + ((size_t)iy * Wi + ix) * CI + c0);
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const float4 v = q[j];
          a_reg[4 * j] = v.x; a_reg[4 * j + 1] = v.y; a_reg[4 * j + 2] = v.z; a_reg[4 * j + 3] = v.w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 16; j++) a_reg[j] = 0.f;
      }
    }
    const float* bq = Bmat + (size_t)(k0 + brow) * CO + nt * BN + bcol;
    b_reg0 = *reinterpret_cast<const float4*>(bq);
    b_reg1 = *reinterpret_cast<const float4*>(bq + (size_t)BROWS * CO);
    if constexpr (NB == 4) {
      b_reg2 = *reinterpret_cast<const float4*>(bq + 2 * (size_t)BROWS * CO);
      b_reg3 = *reinterpret_cast<const float4*>(bq + 3 * (size_t)BROWS * CO);
    }
  };
  auto store = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 16; j++) As[buf][kq * 16 + j][p] = a_reg[j];
    *reinterpret_cast<float4*>(&Bs[buf][brow][bcol]) = b_reg0;
    *reinterpret_cast<float4*>(&Bs[buf][brow + BROWS][bcol]) = b_reg1;
    if constexpr (NB == 4) {
      *reinterpret_cast<float4*>(&Bs[buf][brow + 2 * BROWS][bcol]) = b_reg2;
      *reinterpret_cast<float4*>(&Bs[buf][brow + 3 * BROWS][bcol]) = b_reg3;
    }
  };

  // The wave's two column tiles.  Not one [TM][2] array: with it the planar conv1 copies all 32 accumulator registers out of
  // the AGPRs and back on every K step.
  lp_f32x16 acc0[TM], acc1[TM];
#pragma unroll
  for (int tm = 0; tm < TM; tm++)
#pragma unroll
    for (int i = 0; i < 16; i++) acc0[tm][i] = acc1[tm][i] = 0.f;
  for (int step = -1; step < STEPS; step++) {   // step -1 only stages step 0
    const int buf = step & 1;
    if (step + 1 < STEPS) load(step + 1);
    if (step >= 0) {
#pragma unroll
      for (int s = 0; s < LP_BK / 2; s++) {   // operand maps: A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31]
        const int kk = 2 * s + half;
        const float b0 = Bs[buf][kk][wn * 64 + r], b1 = Bs[buf][kk][wn * 64 + 32 + r];
        float a[TM];
#pragma unroll
        for (int tm = 0; tm < TM; tm++) a[tm] = As[buf][kk][(wm * TM + tm) * 32 + r];
#pragma unroll
        for (int tm = 0; tm < TM; tm++) {
          acc0[tm] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm], b0, acc0[tm], 0, 0, 0);
          acc1[tm] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm], b1, acc1[tm], 0, 0, 0);
        }
      }
    }
    if (step + 1 < STEPS) store(buf ^ 1);
    __syncthreads();   // buf ^ 1 is complete; everyone is done reading buf, which the next iteration overwrites
  }
  // C/D map: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  Rows beyond 2 Ho Wo are never stored.
  const int n0 = nt * BN + wn * 64 + r;
  const float bias0 = bias[n0], bias1 = bias[n0 + 32];
#pragma unroll
  for (int tm = 0; tm < TM; tm++)
#pragma unroll
    for (int reg = 0; reg < 16; reg++) {
      const int mm = mt * LP_BM + (wm * TM + tm) * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * half;
      if (mm < M) {
        out[(size_t)mm * CO + n0] = fmaxf(acc0[tm][reg] + bias0, 0.f);
        out[(size_t)mm * CO + n0 + 32] = fmaxf(acc1[tm][reg] + bias1, 0.f);
      }
    }
}

// WIN x WIN stride-2 floor-mode max pool, [2][Hi][Wi][C] -> [2][Ho][Wo][C]; C4 = C / 4; every window lies inside the image.
template <int WIN>
__global__ void __launch_bounds__(256) lpips_pool_kernel(int Hi, int Wi, int Ho, int Wo, int C4, const float4* __restrict__ in,
                                                         float4* __restrict__ out, size_t total) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % C4);
  size_t pix = idx / C4;
  const int ox = (int)(pix % Wo);
  pix /= Wo;
  const int oy = (int)(pix % Ho), img = (int)(pix / Ho);
  const float4* q = in + (((size_t)img * Hi + 2 * oy) * Wi + 2 * ox) * C4 + c;
  float4 v = q[0];
#pragma unroll
  for (int d = 1; d < WIN * WIN; d++) {
    const float4 u = q[((size_t)(d / WIN) * Wi + d % WIN) * C4];
    v.x = fmaxf(v.x, u.x); v.y = fmaxf(v.y, u.y); v.z = fmaxf(v.z, u.z); v.w = fmaxf(v.w, u.w);
  }
  out[idx] = v;
}

// ---- launches: layer L of table T; the caller checks hipGetLastError() ----------------------------------------------------------
template <const LpLayer* T, int L, int BN, LpSrc SRC>
static void lp_launch_conv(int Hi, int Wi, int Ho, int Wo, const float* in0, const float* in1, const float* blob, float* out,
                           hipStream_t stream) {
  constexpr LpLayer S = T[L];
  const float* B = blob + lp_layer_offset(T, L);
  const float* bias = B + (size_t)lp_kpad(T, L) * S.co;
  const int M = 2 * Ho * Wo;
  const unsigned blocks = (unsigned)((M + LP_BM - 1) / LP_BM) * (S.co / BN);
  hipLaunchKernelGGL((lpips_conv_kernel<S.ks, S.stride, S.pad, S.ci, S.co, BN, SRC>), dim3(blocks), dim3(256), 0, stream, Hi, Wi, Ho,
                     Wo, in0, in1, B, bias, out);
}

template <const LpLayer* T, int L>
static void lp_launch_tap(int npix, const float* act, const float* blob, int nparts, double* partial, hipStream_t stream) {
  constexpr LpLayer S = T[L];
  static_assert(S.tap >= 0, "a tapped layer");
  const float* lin = blob + lp_layer_offset(T, L) + (size_t)lp_kpad(T, L) * S.co + S.co;
  hipLaunchKernelGGL((lpips_tap_kernel<S.co>), dim3(nparts), dim3(256), 0, stream, npix, act, lin, partial);
}

template <int WIN>
static void lp_launch_pool(int Hi, int Wi, int Ho, int Wo, int C, const float* in, float* out, hipStream_t stream) {
  const int C4 = C / 4;
  const size_t total = 2 * (size_t)Ho * Wo * C4;
  hipLaunchKernelGGL(lpips_pool_kernel<WIN>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, Hi, Wi, Ho, Wo, C4,
                     reinterpret_cast<const float4*>(in), reinterpret_cast<float4*>(out), total);
}

}  // namespace s3g
