// Evaluation LPIPS (VGG16 variant) for gfx950: what lpipsPyTorch's lpips(x, y, net_type='vgg') computes for one frame pair
// (include/s3g_lpips_vgg.h restates it with citations).  Activations live [image][H][W][C], channels innermost, both images in one
// buffer.  The conv, pool and tap kernels and their launches are lpips_conv.hpp's and lpips_dev.hpp's, shared with lpips.hip:
//   front kernel  z-scores both planar images once into [2][H][W][4] (the fourth channel is 0): conv1_1 gathers 16-byte pixels.
//   conv kernel   thirteen 3x3 stride-1 pad-1 layers; BN = 128 wherever co allows it, BN = 64 in block 1 (co = 64).
//   pool kernel   2x2 stride 2 after every tap but the last.
//   tap kernel    for C = 64, 128, 256, 512; fixed-order double partials; lpips.hip's one-workgroup finalise.
// Each tap is consumed right after its layer, so two activation buffers of the block-1 size alternate.
// No floating-point atomics; the two images take the same instructions whichever slot they sit in.
#include "lpips_conv.hpp"

#include "../../include/s3g_lpips_vgg.h"

namespace s3g {

constexpr int VG_CONVS = 13;
constexpr LpLayer vg(int ci, int co, int tap) { return {3, 1, 1, ci, co, tap, tap >= 0 && tap < LP_LAYERS - 1 ? 2 : 0}; }
constexpr LpLayer VG_LAYER[VG_CONVS] = {vg(3, 64, -1),    vg(64, 64, 0),    vg(64, 128, -1),  vg(128, 128, 1),  vg(128, 256, -1),
                                        vg(256, 256, -1), vg(256, 256, 2),  vg(256, 512, -1), vg(512, 512, -1), vg(512, 512, 3),
                                        vg(512, 512, -1), vg(512, 512, -1), vg(512, 512, 4)};
constexpr size_t VG_BLOB_FLOATS = lp_layer_offset(VG_LAYER, VG_CONVS - 1) + lp_layer_floats(VG_LAYER, VG_CONVS - 1);

// image, gt: [3,H,W] planar -> z [2][H][W] float4 {z0, z1, z2, 0}
__global__ void __launch_bounds__(256) lpips_vgg_front_kernel(int HW, const float* __restrict__ image, const float* __restrict__ gt,
                                                              float4* __restrict__ z) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= 2 * HW) return;
  const int img = idx >= HW, pix = idx - img * HW;
  const float* src = img ? gt : image;
  z[idx] = make_float4(lp_zscore(src[pix], 0), lp_zscore(src[(size_t)HW + pix], 1), lp_zscore(src[2 * (size_t)HW + pix], 2), 0.f);
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

// Layer L from act[cur] into act[cur ^ 1]; after a tapped layer its tap, and (but for the last) the pool back into act[cur].
// Returns the buffer that holds the next layer's input, or -1 after a failed launch.
template <int L>
static int run_layer(const VgPlan& p, int cur, const float* blob, hipStream_t stream) {
  constexpr LpLayer S = VG_LAYER[L];
  const int H = p.H[L], W = p.W[L];
  const float* in = L == 0 ? reinterpret_cast<const float*>(p.z) : p.act[cur];
  lp_launch_conv<VG_LAYER, L, S.co >= 128 ? 128 : 64, L == 0 ? LP_SRC_PIXEL4 : LP_SRC_ACT>(H, W, H, W, in, nullptr, blob, p.act[cur ^ 1],
                                                                                         stream);
  if (hipGetLastError() != hipSuccess) return -1;
  if constexpr (S.tap < 0) return cur ^ 1;
  else {
    lp_launch_tap<VG_LAYER, L>(H * W, p.act[cur ^ 1], blob, p.nparts[S.tap], p.partial[S.tap], stream);
    if (hipGetLastError() != hipSuccess) return -1;
    if constexpr (S.pool == 0) return cur ^ 1;
    else {
      lp_launch_pool<S.pool>(H, W, H / 2, W / 2, S.co, p.act[cur ^ 1], p.act[cur], stream);
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
    const LpLayer& L = VG_LAYER[l];
    float* B = blob + lp_layer_offset(VG_LAYER, l);
    const int n = lp_kpad(VG_LAYER, l) * L.co;
    lpips_launch_pack(3, L.ci, L.co, lp_k(VG_LAYER, l), lp_kpad(VG_LAYER, l), conv_w[l], B, stream);
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
