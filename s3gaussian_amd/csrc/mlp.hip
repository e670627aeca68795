// Fused deformation MLP on the matrix cores: the per-point chain kernels and the C API of include/s3g_mlp.h.
//
// Reference: 10 nn.Linear + 7 ReLU modules (scene/deformation.py:53-76) = ~20 library GEMM/elementwise launches forward
// and ~40 backward on [P,128]/[P,64] activations; with P = 1.2 M the skinny GEMMs (N = 3..128) cost ~23 ms per
// iteration through hipBLASLt.  Here:
//   mlp_pack_kernel      builds, once per call, the LDS image [in][out+1] of every layer (odd stride -> conflict-free as
//                        MFMA A operand both straight and transposed); 9 slabs + biases = 155 KB.
//   mlp_forward_kernel   one persistent workgroup per CU keeps the WHOLE weight image in LDS (one DMA burst,
//                        global_load_lds_dwordx4).  A wave owns a 32-point tile and its activations never leave the
//                        MFMA accumulator registers: the K order of an MFMA is free, so the accumulator registers of one
//                        layer are fed back, as they are, as the B operand of the next (gemm_reg, mlp_dev.hpp).  No activation
//                        LDS traffic, no barriers after the weight load; waves run independently.  The 5 hidden
//                        activations are stashed for the backward with 16-byte stores, their ReLU masks as bit words.
//   mlp_backward_kernel  the per-point chain (transposed-weight reads of the same image + the ReLU mask words) ->
//                        g_features and 5 gradient signals, same register-resident scheme.
//   mlp_static_*         the six chain kernels without the position head (static scenes, no_dx: dx / g_dx == NULL)
//   <SPLIT = false>      exact fp32 (v_mfma_f32_32x32x2_f32: 64 FLOP/clk/SIMD) -- S3G_MLP_F32;
//   <SPLIT = true>       every operand split into three bf16 pieces on the fly (v_mfma_f32_32x32x16_bf16, fp32 accuracy) --
//                        S3G_MLP_BF16X3_ONTHEFLY, the checker of:
//   mlp_forward_presplit_kernel / mlp_backward_presplit_kernel   the same bf16 x 3 arithmetic on weight images split ONCE by
//                        mlp_pack_presplit_fwd_kernel / _bwd_kernel (layouts tpw / tbw below), bit-identical to <true> -- S3G_MLP_BF16X3.
// The weight gradients (K dimension = the points) are mlp_wgrad.hip, reached through mlp_wgrad_launch(); the fused sampler (+) MLP
// inference kernel is deform_infer.hip; the chain kernels without the SH head (dshs / g_dshs == NULL) are mlp_heads.hip, reached
// through mlp_nosh_forward_launch() / mlp_nosh_backward_launch().
// HBM scratch is spent freely (2 x 1280 B per point): 3 GB of the 288 GB, ~1 ms of traffic for ~20 ms saved.
#include "mlp_dev.hpp"

namespace s3g {

__global__ void __launch_bounds__(256) mlp_pack_kernel(const s3g_mlp_params w, float* __restrict__ packed) {
  const int k = blockIdx.x, tid = threadIdx.x;
  float* dst = packed + (size_t)k * SLAB;
  if (k == NSLAB) {  // biases
    float* bl = packed + (size_t)NSLAB * SLAB;
    const float* src[8] = {w.b0, w.pb1, w.sb1, w.pb2, w.sb2, w.db0, w.db1, w.db2};
    const int n[8] = {64, 64, 64, 3, 48, 64, 64, 3};
    for (int e = tid; e < 8 * 64; e += 256) bl[e] = (e & 63) < n[e >> 6] ? src[e >> 6][e & 63] : 0.f;
    return;
  }
  const float* W = k <= 1 ? w.W0 : k == 2 ? w.P1 : k == 3 ? w.S1 : k == 4 ? w.P2 : k == 5 ? w.S2 : k == 6 ? w.D0 : k == 7 ? w.D1 : w.D2;
  const int out = (k == 4 || k == 8) ? 3 : (k == 5 ? 48 : 64), outpad = (k == 4 || k == 8) ? 32 : 64;
  const int in = k <= 1 ? FEAT : HID, in0 = k == 1 ? 64 : 0, ld = outpad + 1;
  for (int e = tid; e < SLAB; e += 256) dst[e] = 0.f;
  __syncthreads();
  for (int e = tid; e < outpad * 64; e += 256) {
    const int o = e / 64, i = e % 64;
    dst[i * ld + o] = o < out ? W[(size_t)o * in + in0 + i] : 0.f;
  }
}
void mlp_pack_launch(const s3g_mlp_params& w, float* packed, hipStream_t stream) {
  hipLaunchKernelGGL(mlp_pack_kernel, dim3(NSLAB + 1), dim3(256), 0, stream, w, packed);
}

#define WSLAB(k) (lds + (k) * SLAB)
#define BIAS(k) (lds + NSLAB * SLAB + (k) * 64)  // b0 | pb1 | sb1 | pb2 | sb2 | db0 | db1 | db2

struct MlpFwdArgs {
  int P;
  const float* x;
  const float* packed;
  float *dx, *dshs, *feat, *stash;
  uint32_t* maskbits;  // [tiles][5][64] ReLU mask words (NULL when no backward follows)
};

// The forward kernels are thin __global__ wrappers of body templates with one more argument, POS.  <POS = false>: the position head
// is compiled out (static scenes, no_dx: a.dx == NULL) -- stash plane 1 and mask word 1 stay unwritten.  The mlp_static_forward_*
// kernels are those instantiations; the kernels of the default configuration keep their names and their machine code
// (profiles/mlp_static_isa_identity.txt).
template <bool SPLIT, bool POS>
__device__ __forceinline__ void mlp_forward_body(const MlpFwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  load_weights(lds, a.packed, wave, lane);
  const int ntiles = (a.P + MT - 1) / MT;
  const size_t PS = (size_t)a.P * HID;  // one stash plane
  // the 128 input features of the NEXT tile are requested before this tile's MFMAs are issued (raw loads, clamped row: lanes
  // past the end of the array re-read the last point, whose outputs are never stored)
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
    f32x16 hid[2], act[2], acc[2], o[1];
    int ln = lane;   // SPLIT: per-tile copy, so that the seven per-lane output pointers are not carried (and spilled) across the loop
    if constexpr (SPLIT) asm volatile("" : "+v"(ln));
    {  // hidden = W0 x + b0, K = 128 in two halves
      f32x16 x[2];
      acc_bias<2>(hid, BIAS(0), ln);
      unpack(x, cur, 0);
      gemm_fw<SPLIT, 2, 2, false>(WSLAB(0), 65, x, hid, ln);
      unpack(x, cur, 1);
      gemm_fw<SPLIT, 2, 2, false>(WSLAB(1), 65, x, hid, ln);
    }
    uint32_t* mw = a.maskbits ? a.maskbits + (size_t)tile * 5 * 64 + ln : nullptr;
    if (a.stash) act_store<HID, 2, false>(hid, a.stash + 0 * PS, 0, p0, npts, ln);
    if (mw) mw[0 * 64] = pack_positive<2>(hid);
    if constexpr (POS) {
    // pos head: dx = P2 relu(P1 relu(hidden) + pb1) + pb2
    acc_bias<2>(act, BIAS(1), ln);
    gemm_fw<SPLIT, 2, 2, true>(WSLAB(2), 65, hid, act, ln);
    relu_inplace<2>(act);
    if (a.stash) act_store<HID, 2, false>(act, a.stash + 1 * PS, 0, p0, npts, ln);
    if (mw) mw[1 * 64] = pack_positive<2>(act);
    if constexpr (SPLIT) {
      acc_bias<1>(o, BIAS(3), ln);
      gemm_fw<SPLIT, 1, 2, false>(WSLAB(4), 33, act, o, ln);
      act_store3(o, a.dx, p0, npts, ln);
    } else {
      float o3[3];
      head3_fw(WSLAB(4), BIAS(3), act, o3, ln);
      store3(o3, a.dx, p0, npts, ln);
    }
    }
    // shs head: dshs = S2 relu(S1 relu(hidden) + sb1) + sb2
    acc_bias<2>(act, BIAS(2), ln);
    gemm_fw<SPLIT, 2, 2, true>(WSLAB(3), 65, hid, act, ln);
    relu_inplace<2>(act);
    if (a.stash) act_store<HID, 2, false>(act, a.stash + 2 * PS, 0, p0, npts, ln);
    if (mw) mw[2 * 64] = pack_positive<2>(act);
    acc_bias<2>(acc, BIAS(4), ln);
    gemm_fw<SPLIT, 2, 2, false>(WSLAB(5), 65, act, acc, ln);
    act_store<48, 2, false, 48>(acc, a.dshs, 0, p0, npts, ln);
    if (a.feat != nullptr) {  // inference renders that do not draw the feature image skip the head (31 % of the MFMAs)
    // dino head: feat = D2 relu(D1 relu(D0 hidden + db0) + db1) + db2   (input is the raw hidden, deformation.py:126)
    acc_bias<2>(act, BIAS(5), ln);
    gemm_fw<SPLIT, 2, 2, false>(WSLAB(6), 65, hid, act, ln);
    relu_inplace<2>(act);
    if (a.stash) act_store<HID, 2, false>(act, a.stash + 3 * PS, 0, p0, npts, ln);
    if (mw) mw[3 * 64] = pack_positive<2>(act);
    acc_bias<2>(acc, BIAS(6), ln);
    gemm_fw<SPLIT, 2, 2, false>(WSLAB(7), 65, act, acc, ln);
    relu_inplace<2>(acc);
    if (a.stash) act_store<HID, 2, false>(acc, a.stash + 4 * PS, 0, p0, npts, ln);
    if (mw) mw[4 * 64] = pack_positive<2>(acc);
    if constexpr (SPLIT) {
      acc_bias<1>(o, BIAS(7), ln);
      gemm_fw<SPLIT, 1, 2, false>(WSLAB(8), 33, acc, o, ln);
      act_store3(o, a.feat, p0, npts, ln);
    } else {
      float o3[3];
      head3_fw(WSLAB(8), BIAS(7), acc, o3, ln);
      store3(o3, a.feat, p0, npts, ln);
    }
    }
    __builtin_amdgcn_sched_barrier(0);
    cur = nxt;   // copies at the very end: the prefetch has had the whole tile to land
  }
}
template <bool SPLIT>
__global__ void __launch_bounds__(NWAVE * 64) mlp_forward_kernel(const MlpFwdArgs a) { mlp_forward_body<SPLIT, true>(a); }
template <bool SPLIT>
__global__ void __launch_bounds__(NWAVE * 64) mlp_static_forward_kernel(const MlpFwdArgs a) { mlp_forward_body<SPLIT, false>(a); }

struct MlpBwdArgs {
  int P;
  const float* packed;
  const uint32_t* maskbits;  // [tiles][5][64] from the forward: hidden | pos1 | shs1 | dino1 | dino2
  const float *g_dx, *g_dshs, *g_feat;
  float *g_x, *ws;
};

// Everything the backward chain of one tile reads from memory: the three upstream gradients of the lane's point and the five
// ReLU mask words -- 45 registers, requested for the NEXT tile before the current tile's ~600 MFMAs are issued.
struct BwdIn {
  float gd[3], gf[3];
  float4 gs[6];       // g_dshs columns 8q + 4h .. +3 (q = 0..3) and 32 + 8q + 4h .. +3 (q = 0, 1): the 48 live columns
  uint32_t bits[5];
};


// Per-point backward chain, same register-resident scheme with the transposed weight reads.
template <bool SPLIT>
__global__ void __launch_bounds__(NWAVE * 64) mlp_backward_kernel(const MlpBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  load_weights(lds, a.packed, wave, lane);
  const int ntiles = (a.P + MT - 1) / MT;
  const size_t PS = (size_t)a.P * HID;
  const int j = lane & 31, h = lane >> 5;
  const bool dino = a.g_feat != nullptr;
  // Raw, select-free loads with clamped addresses (lanes past the end of the array re-read the last point: their columns are
  // never stored): a bounds select on a loaded value would be scheduled where the load was issued and stall there.
  auto issue = [&](BwdIn& I, int tile) {
    const size_t p = (size_t)min(tile * MT + j, a.P - 1);
    const uint32_t* mw = a.maskbits + (size_t)tile * 5 * 64 + lane;
#pragma unroll
    for (int k = 0; k < 5; k++) I.bits[k] = mw[k * 64];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      I.gd[k] = a.g_dx[p * 3 + k];
      I.gf[k] = dino ? a.g_feat[p * 3 + k] : 0.f;
    }
    const float* row = a.g_dshs + p * 48 + 4 * h;
#pragma unroll
    for (int c = 0; c < 6; c++) I.gs[c] = *reinterpret_cast<const float4*>(row + 8 * c);
  };
  auto head3 = [&](f32x16 (&g3)[1], const float (&v)[3]) {  // features 0..2 live in registers 0..2 of the h = 0 lanes
    acc_zero<1>(g3);
#pragma unroll
    for (int k = 0; k < 3; k++) g3[0][k] = h == 0 ? v[k] : 0.f;
  };
  const int stride = gridDim.x * NWAVE, t0 = blockIdx.x * NWAVE + wave;
  BwdIn cur, nxt;
  if (t0 < ntiles) issue(cur, t0);
  for (int tile = t0; tile < ntiles; tile += stride) {
    issue(nxt, min(tile + stride, ntiles - 1));   // unconditional (clamped): lets the compiler count the outstanding loads
    __builtin_amdgcn_sched_barrier(0);
    const int p0 = tile * MT, npts = min(MT, a.P - p0);
    f32x16 ghid[2], g[2], acc[2], g3[1];
    acc_zero<2>(ghid);
    // ---- dino head (skipped when the feature image has no gradient: g_feat == NULL) ----
    if (dino) {
      head3(g3, cur.gf);
      acc_zero<2>(acc);
      gemm_reg_t<2, 1, 3>(WSLAB(8), 33, g3, acc, lane);              // D2^T g_feat (3 live K steps: exact fp32 MFMAs in both arithmetics)
      masked_bits<2, false>(g, acc, cur.bits[4]);                  // gradient wrt dino2 pre-activation
      act_store<HID, 2, false>(g, a.ws + 0 * PS, 0, p0, npts, lane);
      acc_zero<2>(acc);
      gemm_bw<SPLIT, 2, 2>(WSLAB(7), 65, g, acc, lane);               // D1^T
      masked_bits<2, false>(g, acc, cur.bits[3]);
      act_store<HID, 2, false>(g, a.ws + 1 * PS, 0, p0, npts, lane);
      gemm_bw<SPLIT, 2, 2>(WSLAB(6), 65, g, ghid, lane);              // ghid = D0^T (dino input is the raw hidden: no mask)
    }
    // ---- pos head ----
    head3(g3, cur.gd);
    acc_zero<2>(acc);
    gemm_reg_t<2, 1, 3>(WSLAB(4), 33, g3, acc, lane);                // P2^T g_dx (exact fp32 MFMAs in both arithmetics)
    masked_bits<2, false>(g, acc, cur.bits[1]);
    act_store<HID, 2, false>(g, a.ws + 2 * PS, 0, p0, npts, lane);
    acc_zero<2>(acc);
    gemm_bw<SPLIT, 2, 2>(WSLAB(2), 65, g, acc, lane);                 // P1^T
    // ---- shs head ----
    {
      f32x16 gs[2], t[2];
#pragma unroll
      for (int c = 0; c < 8; c++) {  // chunk c = columns 8c + 4h .. +3; chunks 6, 7 (columns >= 48) do not exist
        const float4 v = c < 6 ? cur.gs[c < 6 ? c : 0] : make_float4(0.f, 0.f, 0.f, 0.f);
        gs[c >> 2][4 * (c & 3) + 0] = v.x; gs[c >> 2][4 * (c & 3) + 1] = v.y;
        gs[c >> 2][4 * (c & 3) + 2] = v.z; gs[c >> 2][4 * (c & 3) + 3] = v.w;
      }
      acc_zero<2>(t);
      gemm_bw<SPLIT, 2, 2>(WSLAB(5), 65, gs, t, lane);                // S2^T g_dshs (rows 48..63 of the image are zero)
      masked_bits<2, false>(g, t, cur.bits[2]);
    }
    act_store<HID, 2, false>(g, a.ws + 3 * PS, 0, p0, npts, lane);
    gemm_bw<SPLIT, 2, 2>(WSLAB(3), 65, g, acc, lane);                 // + S1^T  (same relu(hidden) mask as P1^T)
    masked_bits<2, true>(ghid, acc, cur.bits[0]);
    act_store<HID, 2, false>(ghid, a.ws + 4 * PS, 0, p0, npts, lane);
    // ---- feature_out: g_x[:, half] = W0[:, half]^T ghid ----
    acc_zero<2>(acc);
    gemm_bw<SPLIT, 2, 2>(WSLAB(0), 65, ghid, acc, lane);
    act_store<FEAT, 2, false>(acc, a.g_x, 0, p0, npts, lane);
    acc_zero<2>(acc);
    gemm_bw<SPLIT, 2, 2>(WSLAB(1), 65, ghid, acc, lane);
    act_store<FEAT, 2, false>(acc, a.g_x, 64, p0, npts, lane);
    __builtin_amdgcn_sched_barrier(0);
    cur = nxt;
  }
}

// The same chain without the position head (static scenes, no_dx: a.g_dx == NULL): g_dx, mask word 1 and the pos1 plane are not read,
// workspace plane 2 is not written.  Its own function, not an instantiation of a shared body: behind a common body the kernels above
// lose their machine code (two instructions, operand orders), and the default configuration's kernels do not change for this one
// (profiles/mlp_static_isa_identity.txt).  What it computes is mlp_backward_kernel with g_dx = 0, checked bit for bit
// (tests/test_static_mlp_gpu.py).
template <bool SPLIT>
__global__ void __launch_bounds__(NWAVE * 64) mlp_static_backward_kernel(const MlpBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  load_weights(lds, a.packed, wave, lane);
  const int ntiles = (a.P + MT - 1) / MT;
  const size_t PS = (size_t)a.P * HID;
  const int j = lane & 31, h = lane >> 5;
  const bool dino = a.g_feat != nullptr;
  auto issue = [&](BwdIn& I, int tile) {   // (I.gd and I.bits[1] stay unset: nothing reads them)
    const size_t p = (size_t)min(tile * MT + j, a.P - 1);
    const uint32_t* mw = a.maskbits + (size_t)tile * 5 * 64 + lane;
#pragma unroll
    for (int k = 0; k < 5; k++)
      if (k != 1) I.bits[k] = mw[k * 64];
#pragma unroll
    for (int k = 0; k < 3; k++) I.gf[k] = dino ? a.g_feat[p * 3 + k] : 0.f;
    const float* row = a.g_dshs + p * 48 + 4 * h;
#pragma unroll
    for (int c = 0; c < 6; c++) I.gs[c] = *reinterpret_cast<const float4*>(row + 8 * c);
  };
  const int stride = gridDim.x * NWAVE, t0 = blockIdx.x * NWAVE + wave;
  BwdIn cur, nxt;
  if (t0 < ntiles) issue(cur, t0);
  for (int tile = t0; tile < ntiles; tile += stride) {
    issue(nxt, min(tile + stride, ntiles - 1));
    __builtin_amdgcn_sched_barrier(0);
    const int p0 = tile * MT, npts = min(MT, a.P - p0);
    f32x16 ghid[2], g[2], acc[2], g3[1];
    acc_zero<2>(ghid);
    if (dino) {
      acc_zero<1>(g3);
#pragma unroll
      for (int k = 0; k < 3; k++) g3[0][k] = h == 0 ? cur.gf[k] : 0.f;
      acc_zero<2>(acc);
      gemm_reg_t<2, 1, 3>(WSLAB(8), 33, g3, acc, lane);              // D2^T g_feat
      masked_bits<2, false>(g, acc, cur.bits[4]);
      act_store<HID, 2, false>(g, a.ws + 0 * PS, 0, p0, npts, lane);
      acc_zero<2>(acc);
      gemm_bw<SPLIT, 2, 2>(WSLAB(7), 65, g, acc, lane);               // D1^T
      masked_bits<2, false>(g, acc, cur.bits[3]);
      act_store<HID, 2, false>(g, a.ws + 1 * PS, 0, p0, npts, lane);
      gemm_bw<SPLIT, 2, 2>(WSLAB(6), 65, g, ghid, lane);              // ghid = D0^T
    }
    acc_zero<2>(acc);                                                // (where the position head's P1^T term would have started the sum)
    {
      f32x16 gs[2], t[2];
#pragma unroll
      for (int c = 0; c < 8; c++) {
        const float4 v = c < 6 ? cur.gs[c < 6 ? c : 0] : make_float4(0.f, 0.f, 0.f, 0.f);
        gs[c >> 2][4 * (c & 3) + 0] = v.x; gs[c >> 2][4 * (c & 3) + 1] = v.y;
        gs[c >> 2][4 * (c & 3) + 2] = v.z; gs[c >> 2][4 * (c & 3) + 3] = v.w;
      }
      acc_zero<2>(t);
      gemm_bw<SPLIT, 2, 2>(WSLAB(5), 65, gs, t, lane);                // S2^T g_dshs
      masked_bits<2, false>(g, t, cur.bits[2]);
    }
    act_store<HID, 2, false>(g, a.ws + 3 * PS, 0, p0, npts, lane);
    gemm_bw<SPLIT, 2, 2>(WSLAB(3), 65, g, acc, lane);                 // S1^T
    masked_bits<2, true>(ghid, acc, cur.bits[0]);
    act_store<HID, 2, false>(ghid, a.ws + 4 * PS, 0, p0, npts, lane);
    acc_zero<2>(acc);
    gemm_bw<SPLIT, 2, 2>(WSLAB(0), 65, ghid, acc, lane);
    act_store<FEAT, 2, false>(acc, a.g_x, 0, p0, npts, lane);
    acc_zero<2>(acc);
    gemm_bw<SPLIT, 2, 2>(WSLAB(1), 65, ghid, acc, lane);
    act_store<FEAT, 2, false>(acc, a.g_x, 64, p0, npts, lane);
    __builtin_amdgcn_sched_barrier(0);
    cur = nxt;
  }
}
#undef WSLAB
#undef BIAS

// ---- training forward on the bf16 matrix pipe with the weights split ONCE (round 5; S3G_MLP_BF16X3) ------------------------------
// mlp_forward_kernel<true> splits every weight fragment on the fly, in every wave, for every 32-point tile: 44 VALU instructions per
// fragment, 64 fragments per tile -- the kernel is VALU-bound and gains 15 % where the instruction rates promise 2.7 x.
// Here the A operands of all layers but P1 are pre-split by mlp_pack_presplit_fwd_kernel into fragment order (three pieces x 64 lanes
// x 16 bytes: one conflict-free ds_read_b128 per piece and lane) and stay in LDS; P1 stays fp32 and is split by the lanes that read
// it (everything pre-split would need 168 KB; this image is 159 KiB of the 160).  Same pieces, same MFMA order as the on-the-fly
// kernel: outputs, stash and mask words are BIT-IDENTICAL to mlp_forward_kernel<true> (tests/test_mlp_gpu.py), which stays in the
// tree as the checker of this one (S3G_MLP_BF16X3_ONTHEFLY).
namespace tpw {   // 32-bit words
constexpr int FRAG = FRAG_WORDS;
constexpr int W0 = 0;                                 // [mbo 2][ks 8][piece 3][FRAG]
constexpr int S1 = W0 + 2 * 8 * 3 * FRAG;             // [mbo 2][ks 4][piece 3][FRAG]
constexpr int D0 = S1 + 2 * 4 * 3 * FRAG;
constexpr int D1 = D0 + 2 * 4 * 3 * FRAG;
constexpr int S2A = D1 + 2 * 4 * 3 * FRAG;            // [ks 4][piece 3][FRAG]        rows 0..31
constexpr int S2B = S2A + 4 * 3 * FRAG;               // [ks 4][piece 3][FRAG / 2]    rows 32..47: slot = 16 * h + (row & 15)
constexpr int P2 = S2B + 4 * 3 * (FRAG / 2);          // [ks 4][piece 3][h 2][row 3][4 words]
constexpr int D2 = P2 + 4 * 3 * 2 * 3 * 4;
constexpr int P1LD = 68;
constexpr int P1 = D2 + 4 * 3 * 2 * 3 * 4;            // fp32 [row 64][64 inputs + 4]
constexpr int BIAS = P1 + 64 * P1LD;
constexpr int B_B0 = 0, B_PB1 = 64, B_SB1 = 128, B_SB2 = 192, B_DB0 = 256, B_DB1 = 320, B_PB2 = 384, B_DB2 = 416, NBIAS = 448;   // the two 3-row biases zero padded to 32
constexpr int WORDS = BIAS + NBIAS;
static_assert(WORDS % 256 == 0 && WORDS * 4 <= 160 * 1024, "whole 1 KiB DMA rows, inside the CU's LDS");
static_assert(P2 % 4 == 0 && D2 % 4 == 0 && P1 % 4 == 0 && BIAS % 4 == 0, "16-byte aligned regions");
}  // namespace tpw

// The backward's image: the TRANSPOSED layers in fragment order -- A[row = input feature][k = output feature] -- for W0 (four
// 32-row blocks: the 128 inputs), D1, D0, S1 and S2 (K = 48: three K steps); P1^T stays fp32 [64 in][64 out + 4] and is split by the
// lanes that read it; the two 3-row heads (K = 3) run on the exact fp32 MFMA from a compact fp32 [64 in][8] image (columns 0..2 = the
// three output rows, 3..7 zero: what the h = 1 lanes read).  159 KiB like the forward's.
namespace tbw {   // 32-bit words
constexpr int FRAG = FRAG_WORDS;
constexpr int W0T = 0;                                // [mbo 4][ks 4][piece 3][FRAG]
constexpr int D1T = W0T + 4 * 4 * 3 * FRAG;           // [mbo 2][ks 4][piece 3][FRAG]
constexpr int D0T = D1T + 2 * 4 * 3 * FRAG;
constexpr int S1T = D0T + 2 * 4 * 3 * FRAG;
constexpr int S2T = S1T + 2 * 4 * 3 * FRAG;           // [mbo 2][ks 3][piece 3][FRAG]   (48 output features = 3 K steps)
constexpr int P1LD = 68;
constexpr int P1T = S2T + 2 * 3 * 3 * FRAG;           // fp32 [in 64][64 outputs + 4]
constexpr int H3LD = 8;
constexpr int P2T = P1T + 64 * P1LD;                  // fp32 [in 64][8]
constexpr int D2T = P2T + 64 * H3LD;
constexpr int WORDS = D2T + 64 * H3LD;
static_assert(WORDS % 256 == 0 && WORDS * 4 <= 160 * 1024, "whole 1 KiB DMA rows, inside the CU's LDS");
static_assert(P1T % 4 == 0 && P2T % 4 == 0, "16-byte aligned regions");
}  // namespace tbw
constexpr int PACK_TOTAL = PACK_FLOATS + tpw::WORDS + tbw::WORDS;   // floats in front of the activation stash

__global__ void __launch_bounds__(256) mlp_pack_presplit_fwd_kernel(const s3g_mlp_params w, uint32_t* __restrict__ img) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= tpw::WORDS) return;
  uint32_t out = 0;
  if (x < tpw::S2B) {   // full fragments
    const float* W; int KS, ld, rows, y;
    if (x < tpw::S1) { W = w.W0; KS = 8; ld = FEAT; rows = 64; y = x - tpw::W0; }
    else if (x < tpw::D0) { W = w.S1; KS = 4; ld = HID; rows = 64; y = x - tpw::S1; }
    else if (x < tpw::D1) { W = w.D0; KS = 4; ld = HID; rows = 64; y = x - tpw::D0; }
    else if (x < tpw::S2A) { W = w.D1; KS = 4; ld = HID; rows = 64; y = x - tpw::D1; }
    else { W = w.S2; KS = 4; ld = HID; rows = 48; y = x - tpw::S2A; }
    const int t = y & 3, lane = (y >> 2) & 63, piece = (y >> 8) % 3, fr = (y >> 8) / 3, ks = fr % KS, mbo = fr / KS;
    out = split_word(W, rows, ld, 32 * mbo + (lane & 31), split_feature(ks, lane >> 5, 2 * t), split_feature(ks, lane >> 5, 2 * t + 1), piece);
  } else if (x < tpw::P2) {   // S2 rows 32..47
    const int y = x - tpw::S2B, t = y & 3, slot = (y >> 2) & 31, piece = (y >> 7) % 3, ks = (y >> 7) / 3;
    out = split_word(w.S2, 48, HID, 32 + (slot & 15), split_feature(ks, slot >> 4, 2 * t), split_feature(ks, slot >> 4, 2 * t + 1), piece);
  } else if (x < tpw::P1) {   // the two 3-row heads
    const bool dino = x >= tpw::D2;
    const int y = x - (dino ? tpw::D2 : tpw::P2), t = y & 3, q = y >> 2, row = q % 3, h = (q / 3) & 1, piece = (q / 6) % 3, ks = q / 18;
    out = split_word(dino ? w.D2 : w.P2, 3, HID, row, split_feature(ks, h, 2 * t), split_feature(ks, h, 2 * t + 1), piece);
  } else if (x < tpw::BIAS) {   // P1 as it is, rows padded
    const int y = x - tpw::P1, row = y / tpw::P1LD, f = y % tpw::P1LD;
    out = f < HID ? __float_as_uint(w.P1[row * HID + f]) : 0u;
  } else {
    const int y = x - tpw::BIAS;
    float v = 0.f;
    if (y < 64) v = w.b0[y];
    else if (y < 128) v = w.pb1[y - 64];
    else if (y < 192) v = w.sb1[y - 128];
    else if (y < 256) v = y - 192 < 48 ? w.sb2[y - 192] : 0.f;
    else if (y < 320) v = w.db0[y - 256];
    else if (y < 384) v = w.db1[y - 320];
    else if (y < 416) v = y - 384 < 3 ? w.pb2[y - 384] : 0.f;
    else v = y - 416 < 3 ? w.db2[y - 416] : 0.f;
    out = __float_as_uint(v);
  }
  img[x] = out;
}

// word t of piece `piece` of the transposed pair (W[o0][in], W[o1][in]); output features >= outs are zero
__device__ __forceinline__ uint32_t split_word_t(const float* __restrict__ W, int outs, int ld, int in, int o0, int o1, int piece) {
  uint32_t p[3];
  const float a = o0 < outs ? W[(size_t)o0 * ld + in] : 0.f, b = o1 < outs ? W[(size_t)o1 * ld + in] : 0.f;
  split_pair(a, b, p[0], p[1], p[2]);
  return piece == 0 ? p[0] : (piece == 1 ? p[1] : p[2]);
}
__global__ void __launch_bounds__(256) mlp_pack_presplit_bwd_kernel(const s3g_mlp_params w, uint32_t* __restrict__ img) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= tbw::WORDS) return;
  uint32_t out = 0;
  if (x < tbw::P1T) {   // full fragments of W^T: row = input feature, k = output feature
    const float* W; int KS, ld, outs, y;
    if (x < tbw::D1T) { W = w.W0; KS = 4; ld = FEAT; outs = 64; y = x - tbw::W0T; }
    else if (x < tbw::D0T) { W = w.D1; KS = 4; ld = HID; outs = 64; y = x - tbw::D1T; }
    else if (x < tbw::S1T) { W = w.D0; KS = 4; ld = HID; outs = 64; y = x - tbw::D0T; }
    else if (x < tbw::S2T) { W = w.S1; KS = 4; ld = HID; outs = 64; y = x - tbw::S1T; }
    else { W = w.S2; KS = 3; ld = HID; outs = 48; y = x - tbw::S2T; }
    const int t = y & 3, lane = (y >> 2) & 63, piece = (y >> 8) % 3, fr = (y >> 8) / 3, ks = fr % KS, mbo = fr / KS;
    out = split_word_t(W, outs, ld, 32 * mbo + (lane & 31), split_feature(ks, lane >> 5, 2 * t), split_feature(ks, lane >> 5, 2 * t + 1), piece);
  } else if (x < tbw::P2T) {   // P1^T as fp32 rows
    const int y = x - tbw::P1T, in = y / tbw::P1LD, o = y % tbw::P1LD;
    out = o < HID ? __float_as_uint(w.P1[o * HID + in]) : 0u;
  } else {   // the 3-row heads, transposed: [in][8]
    const bool dino = x >= tbw::D2T;
    const int y = x - (dino ? tbw::D2T : tbw::P2T), in = y / tbw::H3LD, o = y % tbw::H3LD;
    out = o < 3 ? __float_as_uint((dino ? w.D2 : w.P2)[o * HID + in]) : 0u;
  }
  img[x] = out;
}

// Per-point backward chain on the pre-split image: mlp_backward_kernel<true> with every fragment split ONCE (bit-identical to it).
__global__ void __launch_bounds__(NWAVE * 64) mlp_backward_presplit_kernel(const MlpBwdArgs a) {   // a.packed = the tbw image
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const uint32_t* wsplit = reinterpret_cast<const uint32_t*>(lds);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = wave; c < tbw::WORDS / 256; c += NWAVE)
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.packed + c * 256 + lane * 4),
                                     (__attribute__((address_space(3))) void*)(lds + c * 256), 16, 0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const int ntiles = (a.P + MT - 1) / MT;
  const size_t PS = (size_t)a.P * HID;
  const int j = lane & 31, h = lane >> 5;
  const bool dino = a.g_feat != nullptr;
  auto issue = [&](BwdIn& I, int tile) {
    const size_t p = (size_t)min(tile * MT + j, a.P - 1);
    const uint32_t* mw = a.maskbits + (size_t)tile * 5 * 64 + lane;
#pragma unroll
    for (int k = 0; k < 5; k++) I.bits[k] = mw[k * 64];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      I.gd[k] = a.g_dx[p * 3 + k];
      I.gf[k] = dino ? a.g_feat[p * 3 + k] : 0.f;
    }
    const float* row = a.g_dshs + p * 48 + 4 * h;
#pragma unroll
    for (int c = 0; c < 6; c++) I.gs[c] = *reinterpret_cast<const float4*>(row + 8 * c);
  };
  auto head3 = [&](f32x16 (&g3)[1], const float (&v)[3]) {
    acc_zero<1>(g3);
#pragma unroll
    for (int k = 0; k < 3; k++) g3[0][k] = h == 0 ? v[k] : 0.f;
  };
  const int stride = gridDim.x * NWAVE, t0 = blockIdx.x * NWAVE + wave;
  BwdIn cur, nxt;
  if (t0 < ntiles) issue(cur, t0);
  for (int tile = t0; tile < ntiles; tile += stride) {
    issue(nxt, min(tile + stride, ntiles - 1));
    __builtin_amdgcn_sched_barrier(0);
    const int p0 = tile * MT, npts = min(MT, a.P - p0);
    int ln = lane;
    asm volatile("" : "+v"(ln));
    f32x16 ghid[2], g[2], acc[2], g3[1];
    ActSplit<2> gsp;
    acc_zero<2>(ghid);
    if (dino) {
      head3(g3, cur.gf);
      acc_zero<2>(acc);
      gemm_reg_t<2, 1, 3>(lds + tbw::D2T, tbw::H3LD, g3, acc, ln);          // D2^T g_feat: exact fp32 MFMAs (3 live K steps)
      masked_bits<2, false>(g, acc, cur.bits[4]);
      act_store<HID, 2, false>(g, a.ws + 0 * PS, 0, p0, npts, ln);
      acc_zero<2>(acc);
      act_split<2, false>(gsp, g);
      gemm_split<2, 2>(wsplit + tbw::D1T, 4, 0, gsp, acc, ln);              // D1^T
      masked_bits<2, false>(g, acc, cur.bits[3]);
      act_store<HID, 2, false>(g, a.ws + 1 * PS, 0, p0, npts, ln);
      act_split<2, false>(gsp, g);
      gemm_split<2, 2>(wsplit + tbw::D0T, 4, 0, gsp, ghid, ln);             // ghid = D0^T (dino input is the raw hidden: no mask)
    }
    // ---- pos head ----
    head3(g3, cur.gd);
    acc_zero<2>(acc);
    gemm_reg_t<2, 1, 3>(lds + tbw::P2T, tbw::H3LD, g3, acc, ln);            // P2^T g_dx
    masked_bits<2, false>(g, acc, cur.bits[1]);
    act_store<HID, 2, false>(g, a.ws + 2 * PS, 0, p0, npts, ln);
    acc_zero<2>(acc);
    act_split<2, false>(gsp, g);
#pragma unroll
    for (int ks = 0; ks < 4; ks++)      // P1^T: fp32 rows in LDS, split by the lanes that read them (same element order as gemm_reg_t_split)
#pragma unroll
      for (int mbo = 0; mbo < 2; mbo++) {
        const float* wr = lds + tbw::P1T + (32 * mbo + (ln & 31)) * tbw::P1LD + 4 * (ln >> 5) + 16 * ks;
        const float4 lo = *reinterpret_cast<const float4*>(wr);
        const float4 hi = *reinterpret_cast<const float4*>(wr + 8);
        const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        acc[mbo] = mfma_split(acc[mbo], split8(v), gsp.b[ks >> 1][ks & 1]);
      }
    // ---- shs head ----
    {
      f32x16 gs[2], t[2];
#pragma unroll
      for (int c = 0; c < 8; c++) {
        const float4 v = c < 6 ? cur.gs[c < 6 ? c : 0] : make_float4(0.f, 0.f, 0.f, 0.f);
        gs[c >> 2][4 * (c & 3) + 0] = v.x; gs[c >> 2][4 * (c & 3) + 1] = v.y;
        gs[c >> 2][4 * (c & 3) + 2] = v.z; gs[c >> 2][4 * (c & 3) + 3] = v.w;
      }
      acc_zero<2>(t);
      ActSplit<2> ssp;
      act_split<2, false>(ssp, gs);
#pragma unroll
      for (int ks = 0; ks < 3; ks++) {    // S2^T g_dshs: K = 48 (the on-the-fly kernel's fourth K step multiplies zeros by zeros)
        Split8 aw[2];
#pragma unroll
        for (int mbo = 0; mbo < 2; mbo++)
#pragma unroll
          for (int pc = 0; pc < 3; pc++)
            aw[mbo].p[pc] = *reinterpret_cast<const u32x4*>(wsplit + tbw::S2T + ((mbo * 3 + ks) * 3 + pc) * tbw::FRAG + ln * 4);
#pragma unroll
        for (int mbo = 0; mbo < 2; mbo++) t[mbo] = mfma_split(t[mbo], aw[mbo], ssp.b[ks >> 1][ks & 1]);
      }
      masked_bits<2, false>(g, t, cur.bits[2]);
    }
    act_store<HID, 2, false>(g, a.ws + 3 * PS, 0, p0, npts, ln);
    act_split<2, false>(gsp, g);
    gemm_split<2, 2>(wsplit + tbw::S1T, 4, 0, gsp, acc, ln);                // + S1^T  (same relu(hidden) mask as P1^T)
    masked_bits<2, true>(ghid, acc, cur.bits[0]);
    act_store<HID, 2, false>(ghid, a.ws + 4 * PS, 0, p0, npts, ln);
    // ---- feature_out: g_x[:, half] = W0[:, half]^T ghid ----
    act_split<2, false>(gsp, ghid);
    acc_zero<2>(acc);
    gemm_split<2, 2>(wsplit + tbw::W0T, 4, 0, gsp, acc, ln);
    act_store<FEAT, 2, false>(acc, a.g_x, 0, p0, npts, ln);
    acc_zero<2>(acc);
    gemm_split<2, 2>(wsplit + tbw::W0T + 2 * 4 * 3 * tbw::FRAG, 4, 0, gsp, acc, ln);
    act_store<FEAT, 2, false>(acc, a.g_x, 64, p0, npts, ln);
    __builtin_amdgcn_sched_barrier(0);
    cur = nxt;
  }
}

// mlp_backward_presplit_kernel without the position head: mlp_static_backward_kernel<true> with every fragment split ONCE (bit-identical
// to it); its own function for the same reason.  The P1T / P2T regions of the image are loaded with the rest and not read.
__global__ void __launch_bounds__(NWAVE * 64) mlp_static_backward_presplit_kernel(const MlpBwdArgs a) {   // a.packed = the tbw image
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const uint32_t* wsplit = reinterpret_cast<const uint32_t*>(lds);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = wave; c < tbw::WORDS / 256; c += NWAVE)
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.packed + c * 256 + lane * 4),
                                     (__attribute__((address_space(3))) void*)(lds + c * 256), 16, 0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const int ntiles = (a.P + MT - 1) / MT;
  const size_t PS = (size_t)a.P * HID;
  const int j = lane & 31, h = lane >> 5;
  const bool dino = a.g_feat != nullptr;
  auto issue = [&](BwdIn& I, int tile) {   // (I.gd and I.bits[1] stay unset: nothing reads them)
    const size_t p = (size_t)min(tile * MT + j, a.P - 1);
    const uint32_t* mw = a.maskbits + (size_t)tile * 5 * 64 + lane;
#pragma unroll
    for (int k = 0; k < 5; k++)
      if (k != 1) I.bits[k] = mw[k * 64];
#pragma unroll
    for (int k = 0; k < 3; k++) I.gf[k] = dino ? a.g_feat[p * 3 + k] : 0.f;
    const float* row = a.g_dshs + p * 48 + 4 * h;
#pragma unroll
    for (int c = 0; c < 6; c++) I.gs[c] = *reinterpret_cast<const float4*>(row + 8 * c);
  };
  const int stride = gridDim.x * NWAVE, t0 = blockIdx.x * NWAVE + wave;
  BwdIn cur, nxt;
  if (t0 < ntiles) issue(cur, t0);
  for (int tile = t0; tile < ntiles; tile += stride) {
    issue(nxt, min(tile + stride, ntiles - 1));
    __builtin_amdgcn_sched_barrier(0);
    const int p0 = tile * MT, npts = min(MT, a.P - p0);
    int ln = lane;
    asm volatile("" : "+v"(ln));
    f32x16 ghid[2], g[2], acc[2], g3[1];
    ActSplit<2> gsp;
    acc_zero<2>(ghid);
    if (dino) {
      acc_zero<1>(g3);
#pragma unroll
      for (int k = 0; k < 3; k++) g3[0][k] = h == 0 ? cur.gf[k] : 0.f;
      acc_zero<2>(acc);
      gemm_reg_t<2, 1, 3>(lds + tbw::D2T, tbw::H3LD, g3, acc, ln);          // D2^T g_feat: exact fp32 MFMAs
      masked_bits<2, false>(g, acc, cur.bits[4]);
      act_store<HID, 2, false>(g, a.ws + 0 * PS, 0, p0, npts, ln);
      acc_zero<2>(acc);
      act_split<2, false>(gsp, g);
      gemm_split<2, 2>(wsplit + tbw::D1T, 4, 0, gsp, acc, ln);              // D1^T
      masked_bits<2, false>(g, acc, cur.bits[3]);
      act_store<HID, 2, false>(g, a.ws + 1 * PS, 0, p0, npts, ln);
      act_split<2, false>(gsp, g);
      gemm_split<2, 2>(wsplit + tbw::D0T, 4, 0, gsp, ghid, ln);             // ghid = D0^T
    }
    acc_zero<2>(acc);                                                      // (where the position head's P1^T term would have started the sum)
    {
      f32x16 gs[2], t[2];
#pragma unroll
      for (int c = 0; c < 8; c++) {
        const float4 v = c < 6 ? cur.gs[c < 6 ? c : 0] : make_float4(0.f, 0.f, 0.f, 0.f);
        gs[c >> 2][4 * (c & 3) + 0] = v.x; gs[c >> 2][4 * (c & 3) + 1] = v.y;
        gs[c >> 2][4 * (c & 3) + 2] = v.z; gs[c >> 2][4 * (c & 3) + 3] = v.w;
      }
      acc_zero<2>(t);
      ActSplit<2> ssp;
      act_split<2, false>(ssp, gs);
#pragma unroll
      for (int ks = 0; ks < 3; ks++) {    // S2^T g_dshs: K = 48
        Split8 aw[2];
#pragma unroll
        for (int mbo = 0; mbo < 2; mbo++)
#pragma unroll
          for (int pc = 0; pc < 3; pc++)
            aw[mbo].p[pc] = *reinterpret_cast<const u32x4*>(wsplit + tbw::S2T + ((mbo * 3 + ks) * 3 + pc) * tbw::FRAG + ln * 4);
#pragma unroll
        for (int mbo = 0; mbo < 2; mbo++) t[mbo] = mfma_split(t[mbo], aw[mbo], ssp.b[ks >> 1][ks & 1]);
      }
      masked_bits<2, false>(g, t, cur.bits[2]);
    }
    act_store<HID, 2, false>(g, a.ws + 3 * PS, 0, p0, npts, ln);
    act_split<2, false>(gsp, g);
    gemm_split<2, 2>(wsplit + tbw::S1T, 4, 0, gsp, acc, ln);                // S1^T
    masked_bits<2, true>(ghid, acc, cur.bits[0]);
    act_store<HID, 2, false>(ghid, a.ws + 4 * PS, 0, p0, npts, ln);
    act_split<2, false>(gsp, ghid);
    acc_zero<2>(acc);
    gemm_split<2, 2>(wsplit + tbw::W0T, 4, 0, gsp, acc, ln);
    act_store<FEAT, 2, false>(acc, a.g_x, 0, p0, npts, ln);
    acc_zero<2>(acc);
    gemm_split<2, 2>(wsplit + tbw::W0T + 2 * 4 * 3 * tbw::FRAG, 4, 0, gsp, acc, ln);
    act_store<FEAT, 2, false>(acc, a.g_x, 64, p0, npts, ln);
    __builtin_amdgcn_sched_barrier(0);
    cur = nxt;
  }
}

template <bool POS>
__device__ __forceinline__ void mlp_forward_presplit_body(const MlpFwdArgs a) {   // a.packed = the tpw image
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const uint32_t* wsplit = reinterpret_cast<const uint32_t*>(lds);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = wave; c < tpw::WORDS / 256; c += NWAVE)
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.packed + c * 256 + lane * 4),
                                     (__attribute__((address_space(3))) void*)(lds + c * 256), 16, 0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  auto bias = [&](int off) { return lds + tpw::BIAS + off; };
  const int ntiles = (a.P + MT - 1) / MT;
  const size_t PS = (size_t)a.P * HID;
  struct XIn { float4 v[16]; };
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
  // the two 3-row heads: rows 0..2 are stored; the other lanes read row 0 (their accumulator rows are never written out)
  auto head3 = [&](int region, const ActSplit<2>& B, f32x16 (&o)[1], int ln) {
    const int j3 = (ln & 31) < 3 ? (ln & 31) : 0, h3 = ln >> 5;
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {
      Split8 w;
#pragma unroll
      for (int pc = 0; pc < 3; pc++)
        w.p[pc] = *reinterpret_cast<const u32x4*>(wsplit + region + ((((ks * 3 + pc) * 2 + h3) * 3 + j3) << 2));
      o[0] = mfma_split(o[0], w, B.b[ks >> 1][ks & 1]);
    }
  };
  const int stride = gridDim.x * NWAVE, t0 = blockIdx.x * NWAVE + wave;
  // ONE input buffer: the 128 features of a tile are consumed by the first GEMM (split into `as`), after which their registers are free
  // again -- the NEXT tile's rows are requested right there and have the remaining three quarters of the tile's work to arrive
  // (the exact kernel keeps two buffers across the whole tile: 64 more live registers, which this kernel does not have)
  XIn cur;
  if (t0 < ntiles) issue(cur, t0);
  for (int tile = t0; tile < ntiles; tile += stride) {
    const int p0 = tile * MT, npts = min(MT, a.P - p0);
    f32x16 hid[2], act[2], acc[2], o[1];
    int ln = lane;   // per-tile copy: LDS / output addresses are re-derived instead of being carried (and spilled) across the loop
    asm volatile("" : "+v"(ln));
    ActSplit<2> hs, as;
    {  // hidden = W0 x + b0, K = 128 in two halves
      f32x16 x[2];
      acc_bias<2>(hid, bias(tpw::B_B0), ln);
      unpack(x, cur, 0);
      act_split<2, false>(as, x);
      gemm_split<2, 2>(wsplit + tpw::W0, 8, 0, as, hid, ln);
      unpack(x, cur, 1);
      act_split<2, false>(as, x);
      __builtin_amdgcn_sched_barrier(0);
      issue(cur, min(tile + stride, ntiles - 1));   // unconditional (clamped): lets the compiler count the outstanding loads
      __builtin_amdgcn_sched_barrier(0);
      gemm_split<2, 2>(wsplit + tpw::W0, 8, 4, as, hid, ln);
    }
    uint32_t* mw = a.maskbits ? a.maskbits + (size_t)tile * 5 * 64 + ln : nullptr;
    if (a.stash) act_store<HID, 2, false>(hid, a.stash + 0 * PS, 0, p0, npts, ln);
    if (mw) mw[0 * 64] = pack_positive<2>(hid);
    act_split<2, true>(hs, hid);   // relu(hidden): the input of the position and SH heads
    if constexpr (POS) {
    // pos head: dx = P2 relu(P1 relu(hidden) + pb1) + pb2.  P1 is fp32 in LDS: a lane's eight weights of a fragment are two 16-byte chunks of its row
    acc_bias<2>(act, bias(tpw::B_PB1), ln);
#pragma unroll
    for (int ks = 0; ks < 4; ks++)
#pragma unroll
      for (int mbo = 0; mbo < 2; mbo++) {
        const float* wr = lds + tpw::P1 + (32 * mbo + (ln & 31)) * tpw::P1LD + 4 * (ln >> 5) + 16 * ks;   // inputs 16 ks + 4 h + {0..3, 8..11}
        const float4 lo = *reinterpret_cast<const float4*>(wr);
        const float4 hi = *reinterpret_cast<const float4*>(wr + 8);
        const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        act[mbo] = mfma_split(act[mbo], split8(v), hs.b[ks >> 1][ks & 1]);
      }
    relu_inplace<2>(act);
    if (a.stash) act_store<HID, 2, false>(act, a.stash + 1 * PS, 0, p0, npts, ln);
    if (mw) mw[1 * 64] = pack_positive<2>(act);
    act_split<2, false>(as, act);
    acc_bias<1>(o, bias(tpw::B_PB2), ln);
    head3(tpw::P2, as, o, ln);
    act_store3(o, a.dx, p0, npts, ln);
    }
    // shs head: dshs = S2 relu(S1 relu(hidden) + sb1) + sb2
    acc_bias<2>(act, bias(tpw::B_SB1), ln);
    gemm_split<2, 2>(wsplit + tpw::S1, 4, 0, hs, act, ln);
    relu_inplace<2>(act);
    if (a.stash) act_store<HID, 2, false>(act, a.stash + 2 * PS, 0, p0, npts, ln);
    if (mw) mw[2 * 64] = pack_positive<2>(act);
    act_split<2, false>(as, act);
    acc_bias<2>(acc, bias(tpw::B_SB2), ln);
    gemm_split<1, 2>(wsplit + tpw::S2A, 4, 0, as, *reinterpret_cast<f32x16(*)[1]>(&acc[0]), ln);
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {   // rows 32..47: lanes of rows 48..63 read rows 32..47 again (never written out)
      Split8 w;
#pragma unroll
      for (int pc = 0; pc < 3; pc++)
        w.p[pc] = *reinterpret_cast<const u32x4*>(wsplit + tpw::S2B + (ks * 3 + pc) * (tpw::FRAG / 2) + ((16 * (ln >> 5) + (ln & 15)) << 2));
      acc[1] = mfma_split(acc[1], w, as.b[ks >> 1][ks & 1]);
    }
    act_store<48, 2, false, 48>(acc, a.dshs, 0, p0, npts, ln);
    if (a.feat != nullptr) {
      // dino head: feat = D2 relu(D1 relu(D0 hidden + db0) + db1) + db2   (input is the RAW hidden, deformation.py:126)
      act_split<2, false>(hs, hid);
      acc_bias<2>(act, bias(tpw::B_DB0), ln);
      gemm_split<2, 2>(wsplit + tpw::D0, 4, 0, hs, act, ln);
      relu_inplace<2>(act);
      if (a.stash) act_store<HID, 2, false>(act, a.stash + 3 * PS, 0, p0, npts, ln);
      if (mw) mw[3 * 64] = pack_positive<2>(act);
      act_split<2, false>(as, act);
      acc_bias<2>(acc, bias(tpw::B_DB1), ln);
      gemm_split<2, 2>(wsplit + tpw::D1, 4, 0, as, acc, ln);
      relu_inplace<2>(acc);
      if (a.stash) act_store<HID, 2, false>(acc, a.stash + 4 * PS, 0, p0, npts, ln);
      if (mw) mw[4 * 64] = pack_positive<2>(acc);
      act_split<2, false>(as, acc);
      acc_bias<1>(o, bias(tpw::B_DB2), ln);
      head3(tpw::D2, as, o, ln);
      act_store3(o, a.feat, p0, npts, ln);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}
__global__ void __launch_bounds__(NWAVE * 64) mlp_forward_presplit_kernel(const MlpFwdArgs a) { mlp_forward_presplit_body<true>(a); }
__global__ void __launch_bounds__(NWAVE * 64) mlp_static_forward_presplit_kernel(const MlpFwdArgs a) { mlp_forward_presplit_body<false>(a); }

}  // namespace s3g

using namespace s3g;

// stash = [packed weight slabs + biases (PACK_FLOATS)] [pre-split forward image (tpw::WORDS)] [pre-split backward image (tbw::WORDS)]
//         [5 x P x 64 activations] [tiles x 5 x 64 ReLU mask words]
static size_t mask_words(int P) { return (size_t)((P > 0 ? P : 0) + MT - 1) / MT * 5 * 64; }
extern "C" size_t s3g_deform_mlp_stash_bytes(int P) {
  return ((size_t)PACK_TOTAL + (size_t)5 * (size_t)(P > 0 ? P : 0) * HID + mask_words(P)) * sizeof(float);
}
extern "C" size_t s3g_deform_mlp_pack_bytes(void) { return (size_t)PACK_TOTAL * sizeof(float); }

// arithmetic of the per-point GEMM chains of s3g_deform_mlp_forward / _backward (process-wide; the weight-gradient GEMMs, whose K
// dimension is the points, are always the exact fp32 chain)
static std::atomic<int> g_mlp_arithmetic{S3G_MLP_F32};
extern "C" int s3g_deform_mlp_set_arithmetic(int mode) {
  if (mode != S3G_MLP_F32 && mode != S3G_MLP_BF16X3 && mode != S3G_MLP_BF16X3_ONTHEFLY) {
    set_error("s3g_deform_mlp_set_arithmetic: mode must be S3G_MLP_F32, S3G_MLP_BF16X3 or S3G_MLP_BF16X3_ONTHEFLY");
    return S3G_ERR_INVALID_ARG;
  }
  g_mlp_arithmetic.store(mode, std::memory_order_relaxed);
  return S3G_OK;
}
extern "C" int s3g_deform_mlp_get_arithmetic(void) { return g_mlp_arithmetic.load(std::memory_order_relaxed); }

static int mlp_set_attrs() {
  static std::atomic<uint64_t> done{0};
  if (device_needs_setup(done)) {
    const void* exact[] = {(const void*)mlp_forward_kernel<false>,  (const void*)mlp_static_forward_kernel<false>,
                           (const void*)mlp_backward_kernel<false>, (const void*)mlp_static_backward_kernel<false>,
                           (const void*)mlp_forward_kernel<true>,   (const void*)mlp_static_forward_kernel<true>,
                           (const void*)mlp_backward_kernel<true>,  (const void*)mlp_static_backward_kernel<true>};
    for (const void* k : exact) S3G_HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, MLP_LDS_FLOATS * 4));
    S3G_HIP_CHECK(hipFuncSetAttribute((const void*)mlp_forward_presplit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, tpw::WORDS * 4));
    S3G_HIP_CHECK(hipFuncSetAttribute((const void*)mlp_static_forward_presplit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, tpw::WORDS * 4));
    S3G_HIP_CHECK(hipFuncSetAttribute((const void*)mlp_backward_presplit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, tbw::WORDS * 4));
    S3G_HIP_CHECK(hipFuncSetAttribute((const void*)mlp_static_backward_presplit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, tbw::WORDS * 4));
    device_setup_done(done);
  }
  return S3G_OK;
}

extern "C" int s3g_deform_mlp_forward(const s3g_mlp_params* w, int P, const float* features, float* dx, float* dshs,
                                      float* feat, float* stash, int save_activations, void* stream_) {
  if (!w || P < 0 || (P > 0 && (!features || !stash))) {
    set_error("s3g_deform_mlp_forward: bad argument");
    return S3G_ERR_INVALID_ARG;
  }
  if (P > 0 && !dx && !dshs && !feat) {
    set_error("s3g_deform_mlp_forward: dx, dshs and feat are all NULL: no head to compute");
    return S3G_ERR_INVALID_ARG;
  }
  if (P == 0) return S3G_OK;
  hipStream_t stream = (hipStream_t)stream_;
  if (!dshs) {   // no SH head (no_dshs): the exact fp32 family of mlp_heads.hip on the fp32 image, whatever the arithmetic mode
    mlp_pack_launch(*w, stash, stream);
    profile_begin(S3G_PROFILE_MLP_FORWARD, stream);
    float* planes = save_activations ? stash + PACK_TOTAL : nullptr;
    uint32_t* words = save_activations ? reinterpret_cast<uint32_t*>(stash + PACK_TOTAL + (size_t)5 * P * HID) : nullptr;
    if (int e = mlp_nosh_forward_launch(P, features, stash, dx, feat, planes, words, stream)) return e;
    profile_end(S3G_PROFILE_MLP_FORWARD, stream, (double)P, 0.0);
    S3G_HIP_CHECK(hipGetLastError());
    return S3G_OK;
  }
  if (int e = mlp_set_attrs()) return e;
  MlpFwdArgs a;
  a.P = P; a.x = features; a.packed = stash; a.dx = dx; a.dshs = dshs; a.feat = feat;
  a.stash = save_activations ? stash + PACK_TOTAL : nullptr;
  a.maskbits = save_activations ? reinterpret_cast<uint32_t*>(stash + PACK_TOTAL + (size_t)5 * P * HID) : nullptr;
  const int ntiles = (P + MT - 1) / MT;
  const int blocks = min((ntiles + NWAVE - 1) / NWAVE, 256);
  const int arith = g_mlp_arithmetic.load(std::memory_order_relaxed);
  const bool pos = dx != nullptr;   // dx == NULL: the kernels with the position head compiled out (static scenes, no_dx)
  // each arithmetic packs only the image its forward kernel reads: the pre-split one sits behind the slot of the fp32 one, which a
  // bf16x3 forward leaves unwritten (a backward in another mode packs the fp32 image itself)
  if (arith == S3G_MLP_BF16X3)
    hipLaunchKernelGGL(mlp_pack_presplit_fwd_kernel, dim3((tpw::WORDS + 255) / 256), dim3(256), 0, stream, *w,
                       reinterpret_cast<uint32_t*>(stash + PACK_FLOATS));
  else
    mlp_pack_launch(*w, stash, stream);
  profile_begin(S3G_PROFILE_MLP_FORWARD, stream);
  if (arith == S3G_MLP_BF16X3) {
    MlpFwdArgs s = a;
    s.packed = stash + PACK_FLOATS;
    auto k = pos ? mlp_forward_presplit_kernel : mlp_static_forward_presplit_kernel;
    hipLaunchKernelGGL(k, dim3(blocks), dim3(NWAVE * 64), tpw::WORDS * 4, stream, s);
  } else if (arith == S3G_MLP_BF16X3_ONTHEFLY) {
    auto k = pos ? mlp_forward_kernel<true> : mlp_static_forward_kernel<true>;
    hipLaunchKernelGGL(k, dim3(blocks), dim3(NWAVE * 64), MLP_LDS_FLOATS * 4, stream, a);
  } else {
    auto k = pos ? mlp_forward_kernel<false> : mlp_static_forward_kernel<false>;
    hipLaunchKernelGGL(k, dim3(blocks), dim3(NWAVE * 64), MLP_LDS_FLOATS * 4, stream, a);
  }
  profile_end(S3G_PROFILE_MLP_FORWARD, stream, (double)P, 0.0);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

static int mlp_backward_impl(const s3g_mlp_params* w, int P, const float* features, const float* stash_, const float* g_dx,
                             const float* g_dshs, const float* g_feat, float* g_features, const s3g_mlp_params* gw, float* workspace,
                             float* partials, void* stream_) {
  if (!w || !gw || P < 0 || (P > 0 && (!features || !stash_ || !g_features || !workspace))) {
    set_error("s3g_deform_mlp_backward: bad argument");
    return S3G_ERR_INVALID_ARG;
  }
  if (P > 0 && !g_dx && !g_dshs && !g_feat) {
    set_error("s3g_deform_mlp_backward: g_dx, g_dshs and g_feat are all NULL: no head to differentiate");
    return S3G_ERR_INVALID_ARG;
  }
  if (P > 0 && (!gw->W0 || !gw->b0 || (g_dx && (!gw->P1 || !gw->pb1 || !gw->P2 || !gw->pb2)) ||
                (g_dshs && (!gw->S1 || !gw->sb1 || !gw->S2 || !gw->sb2)) ||
                (g_feat && (!gw->D0 || !gw->db0 || !gw->D1 || !gw->db1 || !gw->D2 || !gw->db2)))) {
    set_error("s3g_deform_mlp_backward: gw has a NULL slot for feature_out or for a head whose upstream gradient is given");
    return S3G_ERR_INVALID_ARG;
  }
  if (P == 0) return S3G_OK;
  hipStream_t stream = (hipStream_t)stream_;
  const float* stash = stash_ + PACK_TOTAL;  // activations; the packed weight images of the forward sit in front
  if (!g_dshs) {   // no SH head: mlp_heads.hip's exact fp32 chain on the fp32 image (packed here: a forward in another process-wide mode
                   // would not have; only the image region of the caller's buffer is written), then the job table without the two SH jobs
    mlp_pack_launch(*w, const_cast<float*>(stash_), stream);
    profile_begin(S3G_PROFILE_MLP_BACKWARD, stream);
    if (int e = mlp_nosh_backward_launch(P, stash_, reinterpret_cast<const uint32_t*>(stash + (size_t)5 * P * HID), g_dx, g_feat, g_features,
                                         workspace, stream))
      return e;
    profile_end(S3G_PROFILE_MLP_BACKWARD, stream, (double)P, 0.0);
    S3G_HIP_CHECK(hipGetLastError());
    profile_begin(S3G_PROFILE_MLP_WGRAD, stream);
    if (int e = mlp_wgrad_launch(P, features, stash, workspace, g_dx, nullptr, g_feat, gw, partials, stream)) return e;
    profile_end(S3G_PROFILE_MLP_WGRAD, stream, (double)P, 0.0);
    return S3G_OK;
  }
  if (int e = mlp_set_attrs()) return e;
  MlpBwdArgs b;
  b.P = P; b.packed = stash_; b.maskbits = reinterpret_cast<const uint32_t*>(stash + (size_t)5 * P * HID); b.g_dx = g_dx; b.g_dshs = g_dshs; b.g_feat = g_feat; b.g_x = g_features; b.ws = workspace;
  const int ntiles = (P + MT - 1) / MT;
  const int blocks = min((ntiles + NWAVE - 1) / NWAVE, 256);
  const int arith = g_mlp_arithmetic.load(std::memory_order_relaxed);
  const bool pos = g_dx != nullptr;   // g_dx == NULL: the position head's backward is compiled out, gw->P1..pb2 are not touched
  // S3G_MLP_BF16X3: the transposed pre-split image goes into the slot the stash reserves for it; the other modes read the fp32 image,
  // which a bf16x3 forward does not build, so they pack it into its slot (the caller's buffer: only the image regions are written)
  float* img = const_cast<float*>(stash_) + PACK_FLOATS + tpw::WORDS;
  if (arith == S3G_MLP_BF16X3)
    hipLaunchKernelGGL(mlp_pack_presplit_bwd_kernel, dim3((tbw::WORDS + 255) / 256), dim3(256), 0, stream, *w, reinterpret_cast<uint32_t*>(img));
  else
    mlp_pack_launch(*w, const_cast<float*>(stash_), stream);
  profile_begin(S3G_PROFILE_MLP_BACKWARD, stream);
  if (arith == S3G_MLP_BF16X3) {
    MlpBwdArgs sb = b;
    sb.packed = img;
    auto k = pos ? mlp_backward_presplit_kernel : mlp_static_backward_presplit_kernel;
    hipLaunchKernelGGL(k, dim3(blocks), dim3(NWAVE * 64), tbw::WORDS * 4, stream, sb);
  } else if (arith != S3G_MLP_F32) {
    auto k = pos ? mlp_backward_kernel<true> : mlp_static_backward_kernel<true>;
    hipLaunchKernelGGL(k, dim3(blocks), dim3(NWAVE * 64), MLP_LDS_FLOATS * 4, stream, b);
  } else {
    auto k = pos ? mlp_backward_kernel<false> : mlp_static_backward_kernel<false>;
    hipLaunchKernelGGL(k, dim3(blocks), dim3(NWAVE * 64), MLP_LDS_FLOATS * 4, stream, b);
  }
  profile_end(S3G_PROFILE_MLP_BACKWARD, stream, (double)P, 0.0);
  S3G_HIP_CHECK(hipGetLastError());
  profile_begin(S3G_PROFILE_MLP_WGRAD, stream);
  if (int e = mlp_wgrad_launch(P, features, stash, workspace, g_dx, g_dshs, g_feat, gw, partials, stream)) return e;
  profile_end(S3G_PROFILE_MLP_WGRAD, stream, (double)P, 0.0);
  return S3G_OK;
}

extern "C" int s3g_deform_mlp_backward(const s3g_mlp_params* w, int P, const float* features, const float* stash_,
                                       const float* g_dx, const float* g_dshs, const float* g_feat, float* g_features,
                                       const s3g_mlp_params* gw, float* workspace, void* stream_) {
  return mlp_backward_impl(w, P, features, stash_, g_dx, g_dshs, g_feat, g_features, gw, workspace, nullptr, stream_);
}

extern "C" int s3g_deform_mlp_backward_ordered(const s3g_mlp_params* w, int P, const float* features, const float* stash_,
                                               const float* g_dx, const float* g_dshs, const float* g_feat, float* g_features,
                                               const s3g_mlp_params* gw, float* workspace, float* wgrad_partials, void* stream_) {
  if (!wgrad_partials && P > 0) {
    set_error("s3g_deform_mlp_backward_ordered: wgrad_partials is NULL");
    return S3G_ERR_INVALID_ARG;
  }
  return mlp_backward_impl(w, P, features, stash_, g_dx, g_dshs, g_feat, g_features, gw, workspace, wgrad_partials, stream_);
}
