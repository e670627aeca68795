// Evaluation LPIPS (AlexNet variant) for gfx950: what lpipsPyTorch's lpips(x, y, net_type='alex') computes for one frame pair
// (include/s3g_lpips.h restates it with citations).  Activations live [image][Ho][Wo][C], channels innermost, both images in one
// buffer.  The conv, pool and tap kernels and their launches are lpips_conv.hpp's and lpips_dev.hpp's, shared with lpips_vgg.hip:
//   conv kernel   BN = 64 for all five layers; conv1 gathers from the planar images and z-scores on the way.
//   pool kernel   3x3 stride 2 after conv1 and conv2.
//   tap kernel    after every conv; fixed-order double partials, one double per workgroup, plain stores.
//   finalise      one workgroup adds every tap's partials in a fixed order, divides by Ho Wo, writes {total, tap0..tap4}.
// Every layer keeps its own output buffer.  No floating-point atomics; the two images take the same instructions whichever slot
// they sit in.
#include "lpips_conv.hpp"

namespace s3g {

constexpr LpLayer LP_LAYER[LP_LAYERS] = {{11, 4, 2, 3, 64, 0, 3},    {5, 1, 2, 64, 192, 1, 3},   {3, 1, 1, 192, 384, 2, 0},
                                         {3, 1, 1, 384, 256, 3, 0}, {3, 1, 1, 256, 256, 4, 0}};
constexpr size_t LP_BLOB_FLOATS = lp_layer_offset(LP_LAYER, LP_LAYERS - 1) + lp_layer_floats(LP_LAYER, LP_LAYERS - 1);

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
      h = (h - L.pool) / 2 + 1;
      w = (w - L.pool) / 2 + 1;
      p.pool[l] = carve.take<float>(2 * (size_t)h * w * L.co);
    }
    p.Hp[l] = h;
    p.Wp[l] = w;
  }
  p.bytes = carve.bytes();
  return ok;
}

// Layers L.. of the stack: conv, its tap, its pool if it has one.  in0 (and for conv1 in1) is layer L's input of Hi x Wi.
// Returns the first failed launch's error.
template <int L>
static hipError_t run_from(const LpPlan& p, int Hi, int Wi, const float* in0, const float* in1, const float* blob, hipStream_t stream) {
  if constexpr (L == LP_LAYERS) return hipSuccess;
  else {
    constexpr LpLayer S = LP_LAYER[L];
    hipError_t e;
    lp_launch_conv<LP_LAYER, L, 64, L == 0 ? LP_SRC_PLANAR : LP_SRC_ACT>(Hi, Wi, p.Ho[L], p.Wo[L], in0, in1, blob, p.conv[L], stream);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    lp_launch_tap<LP_LAYER, L>(p.Ho[L] * p.Wo[L], p.conv[L], blob, p.nparts[L], p.partial[L], stream);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if constexpr (S.pool != 0) {
      lp_launch_pool<S.pool>(p.Ho[L], p.Wo[L], p.Hp[L], p.Wp[L], S.co, p.conv[L], p.pool[L], stream);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return run_from<L + 1>(p, p.Hp[L], p.Wp[L], S.pool != 0 ? p.pool[L] : p.conv[L], nullptr, blob, stream);
  }
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
    float* B = blob + lp_layer_offset(LP_LAYER, l);
    const int n = lp_kpad(LP_LAYER, l) * L.co;
    lpips_launch_pack(L.ks, L.ci, L.co, lp_k(LP_LAYER, l), lp_kpad(LP_LAYER, l), conv_w[l], B, stream);
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
  S3G_HIP_CHECK(run_from<0>(p, H, W, image, gt, blob, stream));
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
