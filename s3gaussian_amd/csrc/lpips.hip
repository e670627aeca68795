// Evaluation LPIPS (AlexNet variant) for gfx950: what lpipsPyTorch's lpips(x, y, net_type='alex') computes for one frame pair
// (include/s3g_lpips.h restates it with citations).  Activations live [image][Ho][Wo][C], channels innermost, both images in one
// buffer, so a convolution is ONE implicit GEMM with 2 Ho Wo rows (pixels), co columns and K = kh kw ci ordered (kh, kw, ci):
//   conv kernel   256 threads own 128 pixels x 64 channels; K is staged 32 at a time through two LDS buffers (registers hold the next
//                 step's global loads while the matrix pipe works on the current one); a wave multiplies its 32 pixels by the 64
//                 channels with v_mfma_f32_32x32x2_f32 -- an exact k-ordered fp32 fma chain per output; bias and ReLU in the epilogue.
//   pool kernel   3x3 stride 2, floor mode, one float4 of channels per thread.
//   tap kernel    a wave takes the channel vectors of the same pixel of both images: norms by xor butterfly, the divisions,
//                 sum_c w_c d_c in fp32, added per wave in double; one double per workgroup, plain stores.
//   finalise      one workgroup adds every tap's partials in a fixed order, divides by Ho Wo, writes {total, tap0..tap4}.
// No floating-point atomics; the two images take the same instructions whichever slot they sit in.
#include "lpips_dev.hpp"

namespace s3g {

constexpr int LP_BM = 128, LP_BN = 64, LP_BK = 32;   // block tile: pixels x channels, K step

struct LpLayer {
  int ks, stride, pad, ci, co, pool;
};
constexpr LpLayer LP_LAYER[LP_LAYERS] = {{11, 4, 2, 3, 64, 1}, {5, 1, 2, 64, 192, 1}, {3, 1, 1, 192, 384, 0}, {3, 1, 1, 384, 256, 0},
                                         {3, 1, 1, 256, 256, 0}};
constexpr int lp_k(int l) { return LP_LAYER[l].ks * LP_LAYER[l].ks * LP_LAYER[l].ci; }
constexpr int lp_kpad(int l) { return (lp_k(l) + LP_BK - 1) / LP_BK * LP_BK; }
// blob, per layer: B [kpad][co], bias [co], lin [co]; every piece is a multiple of 64 floats
constexpr size_t lp_layer_floats(int l) { return (size_t)lp_kpad(l) * LP_LAYER[l].co + 2 * (size_t)LP_LAYER[l].co; }
constexpr size_t lp_layer_offset(int l) { return l == 0 ? 0 : lp_layer_offset(l - 1) + lp_layer_floats(l - 1); }
constexpr size_t LP_BLOB_FLOATS = lp_layer_offset(LP_LAYERS - 1) + lp_layer_floats(LP_LAYERS - 1);

// in0: FIRST ? image [3,Hi,Wi] planar : activations [2][Hi][Wi][CI];  in1: FIRST ? gt : unused.  out: [2][Ho][Wo][CO].
// Bmat: [KPAD][CO].  Workgroup b owns pixel tile b / (CO/64) and channel tile b % (CO/64).
template <int KS, int STRIDE, int PAD, int CI, int CO, bool FIRST>
__global__ void __launch_bounds__(256) lpips_conv_kernel(int Hi, int Wi, int Ho, int Wo, const float* __restrict__ in0,
                                                         const float* __restrict__ in1, const float* __restrict__ Bmat,
                                                         const float* __restrict__ bias, float* __restrict__ out) {
  constexpr int K = KS * KS * CI, KPAD = (K + LP_BK - 1) / LP_BK * LP_BK, STEPS = KPAD / LP_BK, NT = CO / LP_BN;
  static_assert(CO % LP_BN == 0, "channel tiles are whole");
  static_assert(FIRST || CI % LP_BK == 0, "a K step lies inside one (kh, kw) tap");
  __shared__ float As[2][LP_BK][LP_BM];   // [k][pixel]: the lanes of an operand read are consecutive words
  __shared__ float Bs[2][LP_BK][LP_BN];   // [k][channel]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, r = lane & 31;
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
  const float* src = FIRST ? (img ? in1 : in0) : in0 + (size_t)img * Hi * Wi * CI;
  const int brow = tid >> 4, bcol = (tid & 15) * 4;   // B staging: rows brow and brow + 16 of the step, 4 channels
  float a_reg[16];
  float4 b_reg0, b_reg1;

  auto load = [&](int step) __attribute__((always_inline)) {
    const int k0 = step * LP_BK;
    if constexpr (FIRST) {
#pragma unroll
      for (int j = 0; j < 16; j++) {
        const int k = k0 + kq * 16 + j;
        const int kh = k / (KS * CI), rem = k - kh * (KS * CI), kw = rem / CI, c = rem - kw * CI;
        const int iy = iy0 + kh, ix = ix0 + kw;
        float v = 0.f;   // zero padding applies after the z-score; so does the padding of K
        if (mvalid && k < K && iy >= 0 && iy < Hi && ix >= 0 && ix < Wi)
          v = lp_zscore(src[(size_t)c * Hi * Wi + (size_t)iy * Wi + ix], c);
        a_reg[j] = v;
      }
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
    const float* bq = Bmat + (size_t)(k0 + brow) * CO + nt * LP_BN + bcol;
    b_reg0 = *reinterpret_cast<const float4*>(bq);
    b_reg1 = *reinterpret_cast<const float4*>(bq + 16 * (size_t)CO);
  };
  auto store = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 16; j++) As[buf][kq * 16 + j][p] = a_reg[j];
    *reinterpret_cast<float4*>(&Bs[buf][brow][bcol]) = b_reg0;
    *reinterpret_cast<float4*>(&Bs[buf][brow + 16][bcol]) = b_reg1;
  };

  lp_f32x16 acc0, acc1;
#pragma unroll
  for (int i = 0; i < 16; i++) acc0[i] = acc1[i] = 0.f;
  for (int step = -1; step < STEPS; step++) {   // step -1 only stages step 0
    const int buf = step & 1;
    if (step + 1 < STEPS) load(step + 1);
    if (step >= 0) {
#pragma unroll
      for (int s = 0; s < LP_BK / 2; s++) {   // operand maps: A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31]
        const int kk = 2 * s + half;
        const float a = As[buf][kk][wave * 32 + r];
        const float b0 = Bs[buf][kk][r], b1 = Bs[buf][kk][32 + r];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
      }
    }
    if (step + 1 < STEPS) store(buf ^ 1);
    __syncthreads();   // buf ^ 1 is complete; everyone is done reading buf, which the next iteration overwrites
  }
  // C/D map: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  Rows beyond 2 Ho Wo are never stored.
  const int n0 = nt * LP_BN + r;
  const float bias0 = bias[n0], bias1 = bias[n0 + 32];
#pragma unroll
  for (int reg = 0; reg < 16; reg++) {
    const int mm = mt * LP_BM + wave * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * half;
    if (mm < M) {
      out[(size_t)mm * CO + n0] = fmaxf(acc0[reg] + bias0, 0.f);
      out[(size_t)mm * CO + n0 + 32] = fmaxf(acc1[reg] + bias1, 0.f);
    }
  }
}

// 3x3 stride-2 floor-mode max pool, [2][Hi][Wi][C] -> [2][Ho][Wo][C]; C4 = C / 4; every window lies inside the image.
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
  for (int dy = 0; dy < 3; dy++)
#pragma unroll
    for (int dx = 0; dx < 3; dx++) {
      const float4 u = q[((size_t)dy * Wi + dx) * C4];
      v.x = fmaxf(v.x, u.x); v.y = fmaxf(v.y, u.y); v.z = fmaxf(v.z, u.z); v.w = fmaxf(v.w, u.w);
    }
  out[idx] = v;
}

__global__ void __launch_bounds__(256) lpips_finalize_kernel(LpFinal f, double* __restrict__ record) {
  __shared__ double red[LP_LAYERS][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < LP_LAYERS; t++) {
    double a = 0.0;
    for (int b = threadIdx.x; b < f.nparts[t]; b += 256) a += f.partial[t][b];
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    if (lane == 0) red[t][wave] = a;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double total = 0.0;
#pragma unroll
  for (int t = 0; t < LP_LAYERS; t++) {
    const double v = (((red[t][0] + red[t][1]) + red[t][2]) + red[t][3]) / (double)f.npix[t];
    record[S3G_LPIPS_TAP0 + t] = v;
    total += v;
  }
  record[S3G_LPIPS_TOTAL] = total;
}

// OIHW -> B [KPAD][CO], K ordered (kh, kw, ci), rows K..KPAD-1 zero
__global__ void __launch_bounds__(256) lpips_pack_kernel(int KS, int CI, int CO, int K, int KPAD, const float* __restrict__ w,
                                                         float* __restrict__ B) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= KPAD * CO) return;
  const int k = idx / CO, n = idx - k * CO;
  float v = 0.f;
  if (k < K) {
    const int tap = k / CI, c = k - tap * CI, kh = tap / KS, kw = tap - kh * KS;
    v = w[(((size_t)n * CI + c) * KS + kh) * KS + kw];
  }
  B[idx] = v;
}

// the two launches lpips_vgg.hip shares (declared in lpips_dev.hpp, next to the tap kernel and the z-score both variants use)
void lpips_launch_finalize(const LpFinal& f, double* record, hipStream_t stream) {
  hipLaunchKernelGGL(lpips_finalize_kernel, dim3(1), dim3(256), 0, stream, f, record);
}

void lpips_launch_pack(int KS, int CI, int CO, int K, int KPAD, const float* w, float* B, hipStream_t stream) {
  hipLaunchKernelGGL(lpips_pack_kernel, dim3((KPAD * CO + 255) / 256), dim3(256), 0, stream, KS, CI, CO, K, KPAD, w, B);
}

struct LpPlan {
  int Ho[LP_LAYERS], Wo[LP_LAYERS], Hp[LP_LAYERS], Wp[LP_LAYERS];   // conv outputs; the layer's pooled size (= Ho, Wo without a pool)
  float* conv[LP_LAYERS];
  float* pool[LP_LAYERS];
  double* partial[LP_LAYERS];
  int nparts[LP_LAYERS];
  size_t bytes;
};

// H, W >= S3G_LPIPS_MIN_SIZE.  Returns false when a layer has 2^31 or more activation elements.
static bool lpips_plan(int H, int W, void* workspace, LpPlan& p) {
  Carver carve(workspace);
  int h = H, w = W;
  bool ok = true;
  for (int l = 0; l < LP_LAYERS; l++) {
    const LpLayer& L = LP_LAYER[l];
    p.Ho[l] = (h + 2 * L.pad - L.ks) / L.stride + 1;
    p.Wo[l] = (w + 2 * L.pad - L.ks) / L.stride + 1;
    const size_t npix = (size_t)p.Ho[l] * p.Wo[l];
    if (2 * npix * L.co >= ((size_t)1 << 31)) ok = false;
    p.conv[l] = carve.take<float>(2 * npix * L.co);
    p.nparts[l] = ok ? tap_blocks((int)npix) : 0;
    p.partial[l] = carve.take<double>((npix + 4 * LP_TAP_PIXELS - 1) / (4 * LP_TAP_PIXELS));
    h = p.Ho[l];
    w = p.Wo[l];
    p.pool[l] = nullptr;
    if (L.pool) {
      h = (h - 3) / 2 + 1;
      w = (w - 3) / 2 + 1;
      p.pool[l] = carve.take<float>(2 * (size_t)h * w * L.co);
    }
    p.Hp[l] = h;
    p.Wp[l] = w;
  }
  p.bytes = carve.bytes();
  return ok;
}

template <int L, bool FIRST>
static void launch_conv(const LpPlan& p, int Hi, int Wi, const float* in0, const float* in1, const float* blob, hipStream_t stream) {
  constexpr LpLayer S = LP_LAYER[L];
  const float* B = blob + lp_layer_offset(L);
  const float* bias = B + (size_t)lp_kpad(L) * S.co;
  const int M = 2 * p.Ho[L] * p.Wo[L];
  const unsigned blocks = (unsigned)((M + LP_BM - 1) / LP_BM) * (S.co / LP_BN);
  hipLaunchKernelGGL((lpips_conv_kernel<S.ks, S.stride, S.pad, S.ci, S.co, FIRST>), dim3(blocks), dim3(256), 0, stream, Hi, Wi,
                     p.Ho[L], p.Wo[L], in0, in1, B, bias, p.conv[L]);
}

template <int L>
static void launch_tap(const LpPlan& p, const float* blob, hipStream_t stream) {
  constexpr LpLayer S = LP_LAYER[L];
  const float* lin = blob + lp_layer_offset(L) + (size_t)lp_kpad(L) * S.co + S.co;
  hipLaunchKernelGGL((lpips_tap_kernel<S.co>), dim3(p.nparts[L]), dim3(256), 0, stream, p.Ho[L] * p.Wo[L], p.conv[L], lin,
                     p.partial[L]);
}

static void launch_pool(const LpPlan& p, int l, hipStream_t stream) {
  const int C4 = LP_LAYER[l].co / 4;
  const size_t total = 2 * (size_t)p.Hp[l] * p.Wp[l] * C4;
  hipLaunchKernelGGL(lpips_pool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, p.Ho[l], p.Wo[l], p.Hp[l],
                     p.Wp[l], C4, reinterpret_cast<const float4*>(p.conv[l]), reinterpret_cast<float4*>(p.pool[l]), total);
}

}  // namespace s3g

using namespace s3g;

extern "C" size_t s3g_lpips_weights_bytes(void) { return LP_BLOB_FLOATS * sizeof(float); }

extern "C" int s3g_lpips_pack_weights(const float* const conv_w[5], const float* const conv_b[5], const float* const lin_w[5],
                                      void* packed, void* stream_) {
  if (!conv_w || !conv_b || !lin_w || !packed) {
    set_error("s3g_lpips_pack_weights: NULL argument");
    return S3G_ERR_INVALID_ARG;
  }
  for (int l = 0; l < LP_LAYERS; l++)
    if (!conv_w[l] || !conv_b[l] || !lin_w[l]) {
      set_error("s3g_lpips_pack_weights: NULL weight pointer of layer %d", l);
      return S3G_ERR_INVALID_ARG;
    }
  hipStream_t stream = (hipStream_t)stream_;
  float* blob = reinterpret_cast<float*>(packed);
  for (int l = 0; l < LP_LAYERS; l++) {
    const LpLayer& L = LP_LAYER[l];
    float* B = blob + lp_layer_offset(l);
    const int n = lp_kpad(l) * L.co;
    lpips_launch_pack(L.ks, L.ci, L.co, lp_k(l), lp_kpad(l), conv_w[l], B, stream);
    S3G_HIP_CHECK(hipGetLastError());
    S3G_HIP_CHECK(hipMemcpyAsync(B + n, conv_b[l], L.co * sizeof(float), hipMemcpyDeviceToDevice, stream));
    S3G_HIP_CHECK(hipMemcpyAsync(B + n + L.co, lin_w[l], L.co * sizeof(float), hipMemcpyDeviceToDevice, stream));
  }
  return S3G_OK;
}

extern "C" size_t s3g_lpips_workspace_bytes(int H, int W) {
  if (H < S3G_LPIPS_MIN_SIZE || W < S3G_LPIPS_MIN_SIZE) return 0;
  LpPlan p;
  lpips_plan(H, W, nullptr, p);
  return p.bytes;
}

extern "C" int s3g_lpips(int H, int W, const float* image, const float* gt, const void* packed, double* record, void* workspace,
                         void* stream_) {
  if (H < S3G_LPIPS_MIN_SIZE || W < S3G_LPIPS_MIN_SIZE) {
    set_error("s3g_lpips: a %d x %d image is smaller than 31 x 31, the smallest the AlexNet feature stack accepts", H, W);
    return S3G_ERR_INVALID_ARG;
  }
  if (!image || !gt || !packed || !record || !workspace) {
    set_error("s3g_lpips: NULL argument");
    return S3G_ERR_INVALID_ARG;
  }
  LpPlan p;
  if (!lpips_plan(H, W, workspace, p)) {
    set_error("s3g_lpips: a %d x %d image has more activation elements in a layer than one launch indexes", H, W);
    return S3G_ERR_INVALID_ARG;
  }
  hipStream_t stream = (hipStream_t)stream_;
  const float* blob = reinterpret_cast<const float*>(packed);
  launch_conv<0, true>(p, H, W, image, gt, blob, stream);
  S3G_HIP_CHECK(hipGetLastError());
  launch_tap<0>(p, blob, stream);
  S3G_HIP_CHECK(hipGetLastError());
  launch_pool(p, 0, stream);
  S3G_HIP_CHECK(hipGetLastError());
  launch_conv<1, false>(p, p.Hp[0], p.Wp[0], p.pool[0], nullptr, blob, stream);
  S3G_HIP_CHECK(hipGetLastError());
  launch_tap<1>(p, blob, stream);
  S3G_HIP_CHECK(hipGetLastError());
  launch_pool(p, 1, stream);
  S3G_HIP_CHECK(hipGetLastError());
  launch_conv<2, false>(p, p.Hp[1], p.Wp[1], p.pool[1], nullptr, blob, stream);
  S3G_HIP_CHECK(hipGetLastError());
  launch_tap<2>(p, blob, stream);
  S3G_HIP_CHECK(hipGetLastError());
  launch_conv<3, false>(p, p.Ho[2], p.Wo[2], p.conv[2], nullptr, blob, stream);
  S3G_HIP_CHECK(hipGetLastError());
  launch_tap<3>(p, blob, stream);
  S3G_HIP_CHECK(hipGetLastError());
  launch_conv<4, false>(p, p.Ho[3], p.Wo[3], p.conv[3], nullptr, blob, stream);
  S3G_HIP_CHECK(hipGetLastError());
  launch_tap<4>(p, blob, stream);
  S3G_HIP_CHECK(hipGetLastError());
  LpFinal f;
  for (int l = 0; l < LP_LAYERS; l++) {
    f.partial[l] = p.partial[l];
    f.nparts[l] = p.nparts[l];
    f.npix[l] = p.Ho[l] * p.Wo[l];
  }
  lpips_launch_finalize(f, record, stream);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}
