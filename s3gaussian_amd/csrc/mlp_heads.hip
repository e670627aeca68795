// Deformation MLP without the SH head (ModelHiddenParams no_dshs = True; with feat_head = False and the geometry heads on this is
// 4D-Gaussian-Splatting's default): the chain kernels behind s3g_deform_mlp_forward(dshs = NULL) / _backward(g_dshs = NULL).
//
// A small family of its own beside mlp.hip, whose kernels keep their machine code (profiles/mlp_heads_isa_identity.txt), built from
// the same primitives (mlp_dev.hpp) on the same fp32 [in][out+1] weight image (mlp_pack_kernel) and the same stash / mask-word /
// workspace layout, so that mlp_wgrad.hip serves it with a shorter job table:
//   mlp_nosh_forward_kernel    hidden = W0 x + b0, then the position head and / or the feature (dino) head, each behind a wave-uniform
//                              branch on its output pointer.  No S1, no S2, no [P,48] store; stash plane 2 and mask word 2 stay unwritten.
//   mlp_nosh_backward_kernel   the transposed chain of the heads that have an upstream gradient -> g_features and the signals of
//                              workspace planes 0, 1 (dino), 2 (pos) and 4 (hidden); plane 3 (the shs1 signal) is not written, mask word 2
//                              is not read.
// Arithmetic: v_mfma_f32_32x32x2_f32 (and head3_fw's 4x4x1), exact fp32 fma chains, in EVERY S3G_MLP_ARITHMETIC mode, as mlp_geom.hip
// does: without the SH head the chain is 40 % (dx + feat) to 75 % (dx alone) shorter than the full one, and one exact kernel serves all
// three modes.  Per output the order of operations is mlp_forward_kernel<false>'s / mlp_backward_kernel<false>'s (bias first, k
// ascending, the same helper calls), so in S3G_MLP_F32 every present output is bit-identical to the full call's, and the backward to a
// full backward fed g_dshs = 0 (tests/test_head_subsets_gpu.py).
// Layout: persistent 8-wave workgroups, one per CU (the 155 KB image fills its LDS), a wave owns a 32-point tile, activations stay in
// the MFMA accumulators (gemm_reg), next tile's inputs prefetched a whole tile ahead.
#include "mlp_dev.hpp"

namespace s3g {

#define WSLAB(k) (lds + (k) * SLAB)
#define BIAS(k) (lds + NSLAB * SLAB + (k) * 64)  // b0 | pb1 | sb1 | pb2 | sb2 | db0 | db1 | db2

struct NoShFwdArgs {
  int P;
  const float* x;
  const float* packed;   // the fp32 image of mlp_pack_kernel
  float *dx, *feat;      // either may be NULL (not both)
  float* stash;          // the five [P,64] planes, or NULL when no backward follows
  uint32_t* maskbits;    // [tiles][5][64], or NULL
};

__global__ void __launch_bounds__(NWAVE * 64) mlp_nosh_forward_kernel(const NoShFwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  load_weights(lds, a.packed, wave, lane);
  const int ntiles = (a.P + MT - 1) / MT;
  const size_t PS = (size_t)a.P * HID;  // one stash plane
  // the 128 input features of the NEXT tile are requested before this tile's MFMAs are issued (raw loads, clamped row: lanes past
  // the end of the array re-read the last point, whose outputs are never stored)
  struct XIn { float4 v[16]; };   // chunk c = columns 8c + 4h .. +3 of the lane's point
  const int jj = lane & 31, hh = lane >> 5;
  auto issue = [&](XIn& X, int tile) {
    const float* row = a.x + (size_t)min(tile * MT + jj, a.P - 1) * FEAT + 4 * hh;
#pragma unroll
    for (int c = 0; c < 16; c++) X.v[c] = *reinterpret_cast<const float4*>(row + 8 * c);
  };
  auto unpack = [&](f32x16 (&x)[2], const XIn& X, int half) {
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const float4 v = X.v[8 * half + c];
      x[c >> 2][4 * (c & 3) + 0] = v.x; x[c >> 2][4 * (c & 3) + 1] = v.y;
      x[c >> 2][4 * (c & 3) + 2] = v.z; x[c >> 2][4 * (c & 3) + 3] = v.w;
    }
  };
  const int stride = gridDim.x * NWAVE, t0 = blockIdx.x * NWAVE + wave;
  XIn cur, nxt;
  if (t0 < ntiles) issue(cur, t0);
  for (int tile = t0; tile < ntiles; tile += stride) {
    issue(nxt, min(tile + stride, ntiles - 1));
    __builtin_amdgcn_sched_barrier(0);
    const int p0 = tile * MT, npts = min(MT, a.P - p0);
    f32x16 hid[2], act[2], acc[2];
    float o3[3];
    {  // hidden = W0 x + b0, K = 128 in two halves
      f32x16 x[2];
      acc_bias<2>(hid, BIAS(0), lane);
      unpack(x, cur, 0);
      gemm_reg<2, 2, false>(WSLAB(0), 65, x, hid, lane);
      unpack(x, cur, 1);
      gemm_reg<2, 2, false>(WSLAB(1), 65, x, hid, lane);
    }
    uint32_t* mw = a.maskbits ? a.maskbits + (size_t)tile * 5 * 64 + lane : nullptr;
    if (a.stash) act_store<HID, 2, false>(hid, a.stash + 0 * PS, 0, p0, npts, lane);
    if (mw) mw[0 * 64] = pack_positive<2>(hid);
    if (a.dx != nullptr) {
      // pos head: dx = P2 relu(P1 relu(hidden) + pb1) + pb2
      acc_bias<2>(act, BIAS(1), lane);
      gemm_reg<2, 2, true>(WSLAB(2), 65, hid, act, lane);
      relu_inplace<2>(act);
      if (a.stash) act_store<HID, 2, false>(act, a.stash + 1 * PS, 0, p0, npts, lane);
      if (mw) mw[1 * 64] = pack_positive<2>(act);
      head3_fw(WSLAB(4), BIAS(3), act, o3, lane);
      store3(o3, a.dx, p0, npts, lane);
    }
    if (a.feat != nullptr) {
      // dino head: feat = D2 relu(D1 relu(D0 hidden + db0) + db1) + db2   (input is the raw hidden)
      acc_bias<2>(act, BIAS(5), lane);
      gemm_reg<2, 2, false>(WSLAB(6), 65, hid, act, lane);
      relu_inplace<2>(act);
      if (a.stash) act_store<HID, 2, false>(act, a.stash + 3 * PS, 0, p0, npts, lane);
      if (mw) mw[3 * 64] = pack_positive<2>(act);
      acc_bias<2>(acc, BIAS(6), lane);
      gemm_reg<2, 2, false>(WSLAB(7), 65, act, acc, lane);
      relu_inplace<2>(acc);
      if (a.stash) act_store<HID, 2, false>(acc, a.stash + 4 * PS, 0, p0, npts, lane);
      if (mw) mw[4 * 64] = pack_positive<2>(acc);
      head3_fw(WSLAB(8), BIAS(7), acc, o3, lane);
      store3(o3, a.feat, p0, npts, lane);
    }
    __builtin_amdgcn_sched_barrier(0);
    cur = nxt;   // copies at the very end: the prefetch has had the whole tile to land
  }
}

struct NoShBwdArgs {
  int P;
  const float* packed;
  const uint32_t* maskbits;      // [tiles][5][64] from the forward: hidden | pos1 | (shs1: unwritten) | dino1 | dino2
  const float *g_dx, *g_feat;    // either may be NULL (not both)
  float *g_x, *ws;
};

// What the chain of one tile reads from memory, requested for the NEXT tile before the current tile's MFMAs are issued.  The loads are
// unconditional: an absent head's slots re-read a word / a row that IS there (mask word 0; the other head's gradient), never the
// unwritten words 1 / 3 / 4 of a head the forward skipped, and nothing reads them.
struct NoShBwdIn {
  float gd[3], gf[3];
  uint32_t b0, b1, b3, b4;
};

__global__ void __launch_bounds__(NWAVE * 64) mlp_nosh_backward_kernel(const NoShBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  load_weights(lds, a.packed, wave, lane);
  const int ntiles = (a.P + MT - 1) / MT;
  const size_t PS = (size_t)a.P * HID;
  const int j = lane & 31, h = lane >> 5;
  const bool pos = a.g_dx != nullptr, dino = a.g_feat != nullptr;
  const float* gdp = pos ? a.g_dx : a.g_feat;
  const float* gfp = dino ? a.g_feat : a.g_dx;
  const int k1 = pos ? 1 : 0, k3 = dino ? 3 : 0, k4 = dino ? 4 : 0;
  auto issue = [&](NoShBwdIn& I, int tile) {
    const size_t p = (size_t)min(tile * MT + j, a.P - 1);
    const uint32_t* mw = a.maskbits + (size_t)tile * 5 * 64 + lane;
    I.b0 = mw[0]; I.b1 = mw[k1 * 64]; I.b3 = mw[k3 * 64]; I.b4 = mw[k4 * 64];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      I.gd[k] = gdp[p * 3 + k];
      I.gf[k] = gfp[p * 3 + k];
    }
  };
  auto head3 = [&](f32x16 (&g3)[1], const float (&v)[3]) {  // features 0..2 live in registers 0..2 of the h = 0 lanes
    acc_zero<1>(g3);
#pragma unroll
    for (int k = 0; k < 3; k++) g3[0][k] = h == 0 ? v[k] : 0.f;
  };
  const int stride = gridDim.x * NWAVE, t0 = blockIdx.x * NWAVE + wave;
  NoShBwdIn cur, nxt;
  if (t0 < ntiles) issue(cur, t0);
  for (int tile = t0; tile < ntiles; tile += stride) {
    issue(nxt, min(tile + stride, ntiles - 1));   // unconditional (clamped): lets the compiler count the outstanding loads
    __builtin_amdgcn_sched_barrier(0);
    const int p0 = tile * MT, npts = min(MT, a.P - p0);
    f32x16 ghid[2], g[2], acc[2], g3[1];
    acc_zero<2>(ghid);
    if (dino) {
      head3(g3, cur.gf);
      acc_zero<2>(acc);
      gemm_reg_t<2, 1, 3>(WSLAB(8), 33, g3, acc, lane);              // D2^T g_feat (3 live K steps)
      masked_bits<2, false>(g, acc, cur.b4);                       // gradient wrt dino2 pre-activation
      act_store<HID, 2, false>(g, a.ws + 0 * PS, 0, p0, npts, lane);
      acc_zero<2>(acc);
      gemm_reg_t<2, 2>(WSLAB(7), 65, g, acc, lane);                  // D1^T
      masked_bits<2, false>(g, acc, cur.b3);
      act_store<HID, 2, false>(g, a.ws + 1 * PS, 0, p0, npts, lane);
      gemm_reg_t<2, 2>(WSLAB(6), 65, g, ghid, lane);                 // ghid = D0^T (dino input is the raw hidden: no mask)
    }
    acc_zero<2>(acc);
    if (pos) {
      head3(g3, cur.gd);
      gemm_reg_t<2, 1, 3>(WSLAB(4), 33, g3, acc, lane);              // P2^T g_dx
      masked_bits<2, false>(g, acc, cur.b1);
      act_store<HID, 2, false>(g, a.ws + 2 * PS, 0, p0, npts, lane);
      acc_zero<2>(acc);
      gemm_reg_t<2, 2>(WSLAB(2), 65, g, acc, lane);                  // P1^T
    }
    masked_bits<2, true>(ghid, acc, cur.b0);                         // (+ 0 without a position head: the full kernel's sum, term for term)
    act_store<HID, 2, false>(ghid, a.ws + 4 * PS, 0, p0, npts, lane);
    // ---- feature_out: g_x[:, half] = W0[:, half]^T ghid ----
    acc_zero<2>(acc);
    gemm_reg_t<2, 2>(WSLAB(0), 65, ghid, acc, lane);
    act_store<FEAT, 2, false>(acc, a.g_x, 0, p0, npts, lane);
    acc_zero<2>(acc);
    gemm_reg_t<2, 2>(WSLAB(1), 65, ghid, acc, lane);
    act_store<FEAT, 2, false>(acc, a.g_x, 64, p0, npts, lane);
    __builtin_amdgcn_sched_barrier(0);
    cur = nxt;
  }
}
#undef WSLAB
#undef BIAS

static int nosh_set_attrs() {
  static std::atomic<uint64_t> done{0};
  if (device_needs_setup(done)) {
    S3G_HIP_CHECK(hipFuncSetAttribute((const void*)mlp_nosh_forward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, MLP_LDS_FLOATS * 4));
    S3G_HIP_CHECK(hipFuncSetAttribute((const void*)mlp_nosh_backward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, MLP_LDS_FLOATS * 4));
    device_setup_done(done);
  }
  return S3G_OK;
}

static int nosh_blocks(int P) {
  const int ntiles = (P + MT - 1) / MT;
  return min((ntiles + NWAVE - 1) / NWAVE, 256);
}

int mlp_nosh_forward_launch(int P, const float* features, const float* packed, float* dx, float* feat, float* planes, uint32_t* maskbits,
                            hipStream_t stream) {
  if (int e = nosh_set_attrs()) return e;
  NoShFwdArgs a;
  a.P = P; a.x = features; a.packed = packed; a.dx = dx; a.feat = feat; a.stash = planes; a.maskbits = maskbits;
  hipLaunchKernelGGL(mlp_nosh_forward_kernel, dim3(nosh_blocks(P)), dim3(NWAVE * 64), MLP_LDS_FLOATS * 4, stream, a);
  return S3G_OK;
}

int mlp_nosh_backward_launch(int P, const float* packed, const uint32_t* maskbits, const float* g_dx, const float* g_feat, float* g_features,
                             float* workspace, hipStream_t stream) {
  if (int e = nosh_set_attrs()) return e;
  NoShBwdArgs b;
  b.P = P; b.packed = packed; b.maskbits = maskbits; b.g_dx = g_dx; b.g_feat = g_feat; b.g_x = g_features; b.ws = workspace;
  hipLaunchKernelGGL(mlp_nosh_backward_kernel, dim3(nosh_blocks(P)), dim3(NWAVE * 64), MLP_LDS_FLOATS * 4, stream, b);
  return S3G_OK;
}

}  // namespace s3g
