// Evaluation LPIPS (VGG16 variant) for gfx950: what lpipsPyTorch's lpips(x, y, net_type='vgg') computes for one frame pair
// (include/s3g_lpips_vgg.h restates it with citations).  The conventions are those of lpips.hip: activations live [image][H][W][C],
// channels innermost, both images in one buffer, so a 3x3 stride-1 pad-1 convolution is ONE implicit GEMM with 2 H W rows (pixels),
// co columns and K = 9 ci ordered (kh, kw, ci):
//   front kernel  z-scores both planar images once into [2][H][W][4] (the fourth channel is 0): conv1_1 gathers 16-byte pixels.
//   conv kernel   256 threads own 128 pixels x BN channels; K is staged 32 at a time through two LDS buffers (registers hold the
//                 next step's global loads while the matrix pipe works on the current one).  BN = 128 wherever co allows it: the
//                 four waves sit 2 x 2, each multiplies 64 pixels by 64 channels as 2 x 2 tiles of v_mfma_f32_32x32x2_f32, so an
//                 A tile is gathered by co / 128 workgroups and four matrix instructions share four LDS reads.  co = 64 (block 1)
//                 keeps lpips.hip's 128 x 64 shape, a wave per 32 pixels.  Every output is an exact k-ordered fp32 fma chain; bias
//                 and ReLU in the epilogue.
//   pool kernel   2x2 stride 2, floor mode, one float4 of channels per thread.
//   tap kernel    lpips_dev.hpp's, for C = 64, 128, 256, 512; fixed-order double partials; lpips.hip's one-workgroup finalise.
// Each tap is consumed right after its layer, so two activation buffers of the block-1 size alternate.
// No floating-point atomics; the two images take the same instructions whichever slot they sit in.
#include "lpips_dev.hpp"

#include "../../include/s3g_lpips_vgg.h"

namespace s3g {

constexpr int VG_CONVS = 13;
constexpr int VG_BM = 128, VG_BK = 32;   // block tile: pixels, K step

struct VgLayer {
  int ci, co, tap;   // tap: the index of the tap after this layer's ReLU, or -1; a pool follows every tap but the last
};
constexpr VgLayer VG_LAYER[VG_CONVS] = {{3, 64, -1},    {64, 64, 0},    {64, 128, -1},  {128, 128, 1},  {128, 256, -1},
                                        {256, 256, -1}, {256, 256, 2},  {256, 512, -1}, {512, 512, -1}, {512, 512, 3},
                                        {512, 512, -1}, {512, 512, -1}, {512, 512, 4}};
constexpr int vg_k(int l) { return 9 * VG_LAYER[l].ci; }
constexpr int vg_kpad(int l) { return (vg_k(l) + VG_BK - 1) / VG_BK * VG_BK; }
// blob, per conv: B [kpad][co], bias [co], and after a tapped conv its lin weights [co]; every piece is a multiple of 64 floats
constexpr size_t vg_layer_floats(int l) {
  return (size_t)vg_kpad(l) * VG_LAYER[l].co + (size_t)VG_LAYER[l].co * (VG_LAYER[l].tap >= 0 ? 2 : 1);
}
constexpr size_t vg_layer_offset(int l) { return l == 0 ? 0 : vg_layer_offset(l - 1) + vg_layer_floats(l - 1); }
constexpr size_t VG_BLOB_FLOATS = vg_layer_offset(VG_CONVS - 1) + vg_layer_floats(VG_CONVS - 1);

// image, gt: [3,H,W] planar -> z [2][H][W] float4 {z0, z1, z2, 0}
__global__ void __launch_bounds__(256) lpips_vgg_front_kernel(int HW, const float* __restrict__ image, const float* __restrict__ gt,
                                                              float4* __restrict__ z) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= 2 * HW) return;
  const int img = idx >= HW, pix = idx - img * HW;
  const float* src = img ? gt : image;
  z[idx] = make_float4(lp_zscore(src[pix], 0), lp_zscore(src[(size_t)HW + pix], 1), lp_zscore(src[2 * (size_t)HW + pix], 2), 0.f);
}

__device__ __forceinline__ float vg_comp(const float4 v, int c) { return c == 0 ? v.x : (c == 1 ? v.y : v.z); }

// conv1_1's half K step: k = 16 KQ + j, j < 16, is channel k % 3 of tap k / 3; k >= 27 pads K with zeros.
// Zero padding applies after the z-score: an out-of-image tap contributes 0.
template <int KQ>
__device__ __forceinline__ void vg_gather_first(bool mvalid, int H, int W, int oy, int ox, const float4* __restrict__ src,
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
    a_reg[j] = K0 + j < 27 ? vg_comp(px[t - T0], (K0 + j) % 3) : 0.f;
  }
}

// in: FIRST ? z-scored pixels [2][H][W][4] : activations [2][H][W][CI].  out: [2][H][W][CO].  Bmat: [KPAD][CO].
// Workgroup b owns pixel tile b / (CO/BN) and channel tile b % (CO/BN): the workgroups that gather one A tile are neighbours.
template <int CI, int CO, int BN, bool FIRST>
__global__ void __launch_bounds__(256) lpips_vgg_conv_kernel(int H, int W, const float* __restrict__ in, const float* __restrict__ Bmat,
                                                             const float* __restrict__ bias, float* __restrict__ out) {
  constexpr int K = 9 * CI, KPAD = (K + VG_BK - 1) / VG_BK * VG_BK, STEPS = KPAD / VG_BK, NT = CO / BN;
  constexpr int WN = BN / 64, WM = 4 / WN, TM = VG_BM / WM / 32, TN = 2;   // waves WM x WN, each TM x TN tiles of 32 x 32
  constexpr int BTPR = BN / 4, BROWS = 256 / BTPR, NB = VG_BK / BROWS;     // B staging: float4s per row, rows per pass, passes
  static_assert((BN == 64 && NB == 2) || (BN == 128 && NB == 4), "one or two wave columns of 64 channels");
  static_assert(CO % BN == 0, "channel tiles are whole");
  static_assert(FIRST ? (CI == 3 && STEPS == 1) : CI % VG_BK == 0, "a K step lies inside one (kh, kw) tap");
  __shared__ float As[2][VG_BK][VG_BM];   // [k][pixel]: the lanes of an operand read are consecutive words
  __shared__ float Bs[2][VG_BK][BN];      // [k][channel]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, r = lane & 31;
  const int wm = wave / WN, wn = wave % WN;
  const int nt = blockIdx.x % NT, mt = blockIdx.x / NT;
  const int HW = H * W, M = 2 * HW;
  // staging role: pixel p of the tile, K half kq of the step (16 consecutive k)
  const int p = tid & (VG_BM - 1), kq = tid >> 7;
  const int m = mt * VG_BM + p;
  const bool mvalid = m < M;
  int img = 0, oy = 0, ox = 0;
  if (mvalid) {
    img = m / HW;
    const int rem = m - img * HW;
    oy = rem / W;
    ox = rem - oy * W;
  }
  const float* src = in + (size_t)img * HW * (FIRST ? 4 : CI);
  const int brow = tid / BTPR, bcol = (tid % BTPR) * 4;
  float a_reg[16];
  float4 b_reg0, b_reg1, b_reg2, b_reg3;   // NB = 2 uses the first two

  auto load = [&](int step) __attribute__((always_inline)) {
    const int k0 = step * VG_BK;
    if constexpr (FIRST) {
      if (kq == 0)   // uniform over the wave
        vg_gather_first<0>(mvalid, H, W, oy, ox, reinterpret_cast<const float4*>(src), a_reg);
      else
        vg_gather_first<1>(mvalid, H, W, oy, ox, reinterpret_cast<const float4*>(src), a_reg);
    } else {
      const int tap = k0 / CI, c0 = k0 - tap * CI + kq * 16;
      const int kh = tap / 3, kw = tap - kh * 3;
      const int iy = oy + kh - 1, ix = ox + kw - 1;
      if (mvalid && iy >= 0 && iy < H && ix >= 0 && ix < W) {
        const float4* q = reinterpret_cast<const float4*>(src + ((size_t)iy * W + ix) * CI + c0);
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

  lp_f32x16 acc[TM][TN];
#pragma unroll
  for (int tm = 0; tm < TM; tm++)
#pragma unroll
    for (int tn = 0; tn < TN; tn++)
#pragma unroll
      for (int i = 0; i < 16; i++) acc[tm][tn][i] = 0.f;
  for (int step = -1; step < STEPS; step++) {   // step -1 only stages step 0
    const int buf = step & 1;
    if (step + 1 < STEPS) load(step + 1);
    if (step >= 0) {
#pragma unroll
      for (int s = 0; s < VG_BK / 2; s++) {   // operand maps: A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31]
        const int kk = 2 * s + half;
        float a[TM], b[TN];
#pragma unroll
        for (int tm = 0; tm < TM; tm++) a[tm] = As[buf][kk][(wm * TM + tm) * 32 + r];
#pragma unroll
        for (int tn = 0; tn < TN; tn++) b[tn] = Bs[buf][kk][(wn * TN + tn) * 32 + r];
#pragma unroll
        for (int tm = 0; tm < TM; tm++)
#pragma unroll
          for (int tn = 0; tn < TN; tn++) acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm], b[tn], acc[tm][tn], 0, 0, 0);
      }
    }
    if (step + 1 < STEPS) store(buf ^ 1);
    __syncthreads();   // buf ^ 1 is complete; everyone is done reading buf, which the next iteration overwrites
  }
  // C/D map: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  Rows beyond 2 H W are never stored.
#pragma unroll
  for (int tn = 0; tn < TN; tn++) {
    const int n = nt * BN + (wn * TN + tn) * 32 + r;
    const float bv = bias[n];
#pragma unroll
    for (int tm = 0; tm < TM; tm++)
#pragma unroll
      for (int reg = 0; reg < 16; reg++) {
        const int mm = mt * VG_BM + (wm * TM + tm) * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * half;
        if (mm < M) out[(size_t)mm * CO + n] = fmaxf(acc[tm][tn][reg] + bv, 0.f);
      }
  }
}

// 2x2 stride-2 floor-mode max pool, [2][Hi][Wi][C] -> [2][Ho][Wo][C] with Ho = Hi / 2, Wo = Wi / 2; C4 = C / 4.
__global__ void __launch_bounds__(256) lpips_vgg_pool_kernel(int Hi, int Wi, int Ho, int Wo, int C4, const float4* __restrict__ in,
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
  for (int d = 1; d < 4; d++) {
    const float4 u = q[((size_t)(d >> 1) * Wi + (d & 1)) * C4];
    v.x = fmaxf(v.x, u.x); v.y = fmaxf(v.y, u.y); v.z = fmaxf(v.z, u.z); v.w = fmaxf(v.w, u.w);
  }
  out[idx] = v;
}

struct VgPlan {
  int H[VG_CONVS], W[VG_CONVS];   // every conv's input = output extent
  float4* z;
  float* act[2];                  // the two alternating activation buffers, each of the block-1 size
  double* partial[LP_LAYERS];
  int nparts[LP_LAYERS];
  size_t bytes;
};

// H, W >= S3G_LPIPS_VGG_MIN_SIZE.  Returns false when a layer has 2^31 or more activation elements (block 1 is the largest).
static bool lpips_vgg_plan(int H, int W, void* workspace, VgPlan& p) {
  Carver carve(workspace);
  const size_t a1 = 2 * (size_t)H * W * 64;
  const bool ok = a1 < ((size_t)1 << 31);
  p.z = carve.take<float4>(2 * (size_t)H * W);
  p.act[0] = carve.take<float>(a1);
  p.act[1] = carve.take<float>(a1);
  int h = H, w = W;
  for (int l = 0; l < VG_CONVS; l++) {
    p.H[l] = h;
    p.W[l] = w;
    const int t = VG_LAYER[l].tap;
    if (t < 0) continue;
    const size_t blocks = ((size_t)h * w + 4 * LP_TAP_PIXELS - 1) / (4 * LP_TAP_PIXELS);
    p.nparts[t] = ok ? (int)blocks : 0;
    p.partial[t] = carve.take<double>(blocks);
    h /= 2;
    w /= 2;
  }
  p.bytes = carve.bytes();
  return ok;
}

template <int L>
static void launch_conv(const VgPlan& p, const float* in, float* out, const float* blob, hipStream_t stream) {
  constexpr VgLayer S = VG_LAYER[L];
  constexpr int BN = S.co >= 128 ? 128 : 64;
  const float* B = blob + vg_layer_offset(L);
  const float* bias = B + (size_t)vg_kpad(L) * S.co;
  const int M = 2 * p.H[L] * p.W[L];
  const unsigned blocks = (unsigned)((M + VG_BM - 1) / VG_BM) * (S.co / BN);
  hipLaunchKernelGGL((lpips_vgg_conv_kernel<S.ci, S.co, BN, L == 0>), dim3(blocks), dim3(256), 0, stream, p.H[L], p.W[L], in, B, bias,
                     out);
}

template <int L>
static void launch_tap(const VgPlan& p, const float* act, const float* blob, hipStream_t stream) {
  constexpr VgLayer S = VG_LAYER[L];
  const float* lin = blob + vg_layer_offset(L) + (size_t)vg_kpad(L) * S.co + S.co;
  hipLaunchKernelGGL((lpips_tap_kernel<S.co>), dim3(p.nparts[S.tap]), dim3(256), 0, stream, p.H[L] * p.W[L], act, lin,
                     p.partial[S.tap]);
}

// Layer L from act[cur] into act[cur ^ 1]; after a tapped layer its tap, and (but for the last) the pool back into act[cur].
// Returns the buffer that holds the next layer's input, or -1 after a failed launch.
template <int L>
static int run_layer(const VgPlan& p, int cur, const float* blob, hipStream_t stream) {
  constexpr VgLayer S = VG_LAYER[L];
  const float* in = L == 0 ? reinterpret_cast<const float*>(p.z) : p.act[cur];
  launch_conv<L>(p, in, p.act[cur ^ 1], blob, stream);
  if (hipGetLastError() != hipSuccess) return -1;
  if constexpr (S.tap < 0) return cur ^ 1;
  else {
    launch_tap<L>(p, p.act[cur ^ 1], blob, stream);
    if (hipGetLastError() != hipSuccess) return -1;
    if constexpr (L == VG_CONVS - 1) return cur ^ 1;
    else {
      const int C4 = S.co / 4, Ho = p.H[L] / 2, Wo = p.W[L] / 2;
      const size_t total = 2 * (size_t)Ho * Wo * C4;
      hipLaunchKernelGGL(lpips_vgg_pool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, p.H[L], p.W[L], Ho, Wo, C4,
                         reinterpret_cast<const float4*>(p.act[cur ^ 1]), reinterpret_cast<float4*>(p.act[cur]), total);
      if (hipGetLastError() != hipSuccess) return -1;
      return cur;
    }
  }
}

template <int L>
static bool run_from(const VgPlan& p, int cur, const float* blob, hipStream_t stream) {
  if constexpr (L == VG_CONVS) return true;
  else {
    const int next = run_layer<L>(p, cur, blob, stream);
    return next >= 0 && run_from<L + 1>(p, next, blob, stream);
  }
}

}  // namespace s3g

using namespace s3g;

extern "C" size_t s3g_lpips_vgg_weights_bytes(void) { return VG_BLOB_FLOATS * sizeof(float); }

extern "C" int s3g_lpips_vgg_pack_weights(const float* const conv_w[13], const float* const conv_b[13], const float* const lin_w[5],
                                          void* packed, void* stream_) {
  if (!conv_w || !conv_b || !lin_w || !packed) {
    set_error("s3g_lpips_vgg_pack_weights: NULL argument");
    return S3G_ERR_INVALID_ARG;
  }
  for (int l = 0; l < VG_CONVS; l++)
    if (!conv_w[l] || !conv_b[l] || (VG_LAYER[l].tap >= 0 && !lin_w[VG_LAYER[l].tap])) {
      set_error("s3g_lpips_vgg_pack_weights: NULL weight pointer of conv %d", l);
      return S3G_ERR_INVALID_ARG;
    }
  hipStream_t stream = (hipStream_t)stream_;
  float* blob = reinterpret_cast<float*>(packed);
  for (int l = 0; l < VG_CONVS; l++) {
    const VgLayer& L = VG_LAYER[l];
    float* B = blob + vg_layer_offset(l);
    const int n = vg_kpad(l) * L.co;
    lpips_launch_pack(3, L.ci, L.co, vg_k(l), vg_kpad(l), conv_w[l], B, stream);
    S3G_HIP_CHECK(hipGetLastError());
    S3G_HIP_CHECK(hipMemcpyAsync(B + n, conv_b[l], L.co * sizeof(float), hipMemcpyDeviceToDevice, stream));
    if (L.tap >= 0)
      S3G_HIP_CHECK(hipMemcpyAsync(B + n + L.co, lin_w[L.tap], L.co * sizeof(float), hipMemcpyDeviceToDevice, stream));
  }
  return S3G_OK;
}

extern "C" size_t s3g_lpips_vgg_workspace_bytes(int H, int W) {
  if (H < S3G_LPIPS_VGG_MIN_SIZE || W < S3G_LPIPS_VGG_MIN_SIZE) return 0;
  VgPlan p;
  lpips_vgg_plan(H, W, nullptr, p);
  return p.bytes;
}

extern "C" int s3g_lpips_vgg(int H, int W, const float* image, const float* gt, const void* packed, double* record, void* workspace,
                             void* stream_) {
  if (H < S3G_LPIPS_VGG_MIN_SIZE || W < S3G_LPIPS_VGG_MIN_SIZE) {
    set_error("s3g_lpips_vgg: a %d x %d image is smaller than 16 x 16, the smallest the VGG16 feature stack taps five times", H, W);
    return S3G_ERR_INVALID_ARG;
  }
  VgPlan p;
  if (!lpips_vgg_plan(H, W, workspace, p)) {
    set_error("s3g_lpips_vgg: a %d x %d image has more activation elements in a layer than one launch indexes", H, W);
    return S3G_ERR_INVALID_ARG;
  }
  if (!image || !gt || !packed || !record || !workspace) {
    set_error("s3g_lpips_vgg: NULL argument");
    return S3G_ERR_INVALID_ARG;
  }
  hipStream_t stream = (hipStream_t)stream_;
  const float* blob = reinterpret_cast<const float*>(packed);
  const int HW = H * W;
  hipLaunchKernelGGL(lpips_vgg_front_kernel, dim3((2 * HW + 255) / 256), dim3(256), 0, stream, HW, image, gt, p.z);
  S3G_HIP_CHECK(hipGetLastError());
  if (!run_from<0>(p, 0, blob, stream)) {
    set_error("s3g_lpips_vgg: a kernel launch failed");
    return S3G_ERR_HIP;
  }
  LpFinal f;
  for (int l = 0; l < VG_CONVS; l++) {
    const int t = VG_LAYER[l].tap;
    if (t < 0) continue;
    f.partial[t] = p.partial[t];
    f.nparts[t] = p.nparts[t];
    f.npix[t] = p.H[l] * p.W[l];
  }
  lpips_launch_finalize(f, record, stream);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}
