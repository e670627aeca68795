// Inference: HexPlane sampler (+) feature_out (+) ANY SUBSET of the position / scale / rotation / opacity / SH heads that fits, in ONE
// kernel -- deform_infer.hip's scheme for the networks it does not serve (static scenes: no_dx; no_dshs; 4D-Gaussian-Splatting's
// default dx + ds + dr; ...).  Their no_grad renders used to write the [P,128] features (614 MB at 1.2 M Gaussians), read them back in
// mlp_forward / mlp_nosh_forward and once more in geom_forward_kernel, which also recomputed `hidden`.  Here the features never exist
// and `hidden` is formed once.
//   infer_heads_pack_kernel        the fp32 weight image of the heads PRESENT, laid out per call (HeadsLayout):
//                                    W0 (two K halves) | ten bias vectors of 64 | one [64 in][65] slab per first layer present
//                                    (P1 S1 C1 R1 O1) | S2 [64][65] | P2 [64][33] | the geometry second layers in ONE [64][33] block
//                                    (columns 0..2 C2, 3..6 R2, 7 O2)
//   deform_infer_heads_kernel<UT>  sampler half: InferSampler (deform_infer_dev.hpp), the statements of deform_infer_kernel<UT, false>;
//                                  heads half: each head behind a wave-uniform branch on the head mask, built from the device functions
//                                  its training kernel uses, in its order (bias first, k ascending) --
//                                    dx    gemm_reg<2,2,true> + head3_fw            as mlp_forward_kernel<false> / mlp_nosh_forward_kernel
//                                    dshs  gemm_reg<2,2,true> + gemm_reg<2,2,false> as mlp_forward_kernel<false> / mlp_static_forward_kernel<false>
//                                    ds / dr / do  gemm_reg<2,2,true> + gemm_reg<1,2,false>  as geom_forward_kernel
//                                  so every output is bit for bit that of s3g_hexplane_forward -> s3g_deform_mlp_forward (S3G_MLP_F32 where
//                                  the SH head is present; the SH-less chain is exact in every mode) -> s3g_deform_geom_forward, and what
//                                  a present head computes does not depend on which others are present (an MFMA output row is its own
//                                  fma chain; a geometry head reads the shared block through a pointer moved to its first column, so its
//                                  rows are rows 0 .. N-1 of its accumulator as in geom_forward_kernel; rows >= N hold the neighbours'
//                                  products and are never stored).
// LDS: the image + 8 waves x 6 912 B of staging (a 32 x 32 tile + two sets of tap slots per wave).  The largest image served is W0 + three
// first layers + P2 + the geometry block + biases = 108 032 B -> 163 328 of 163 840 B.  Sets whose image does not fit (four or more first
// layers beside S2, ...) and dx + dshs alone (deform_infer.hip's own) are refused: heads_layout().
#include "deform_infer_dev.hpp"

#include "../../include/s3g_mlp_geom.h"

namespace s3g {

enum { IH_DX = 1, IH_DS = 2, IH_DR = 4, IH_DO = 8, IH_DSHS = 16, IH_ALL = 31 };
constexpr int IH_SLAB33 = 9 * 256;               // floats of a [64 in][32 out + 1] block, padded to whole 1 KiB DMA rows
constexpr int IH_NBIAS = 10;                     // b0 | pb1 | sb1 | cb1 | rb1 | ob1 | sb2 | cb2 (0..2) rb2 (4..7) ob2 (8) | pb2 | zeros
constexpr int IH_BIAS_FLOATS = IH_NBIAS * 64;
constexpr int IH_BIAS = 2 * SLAB;                // behind the two W0 slabs in every layout: the offsets the sampler loop carries are constants
constexpr int IH_STAGE_FLOATS = NWAVE * INF_WAVE_FLOATS;
constexpr int IH_LDS_LIMIT = 160 * 1024;
static_assert(64 * 33 + 7 + 32 <= IH_SLAB33, "a geometry head reads the shared block from column 7 at most");

// first-layer slots: P1 S1 C1 R1 O1
__host__ __device__ constexpr int ih_first_bit(int k) { return k == 0 ? IH_DX : k == 1 ? IH_DSHS : k == 2 ? IH_DS : k == 3 ? IH_DR : IH_DO; }

struct HeadsLayout {      // offsets in floats from the image's start; -1: region absent
  int mask;
  int first[5];           // P1 S1 C1 R1 O1
  int s2, p2, g2;
  int floats;             // the image; rows() * 256 are built and copied (the tail lands in wave 0's staging tile, before its first use)
  __host__ __device__ int rows() const { return (floats + 255) / 256; }
  __host__ __device__ size_t lds_bytes() const { return ((size_t)floats + IH_STAGE_FLOATS) * sizeof(float); }
};

// the layout of a head set, or floats == 0 for a set this kernel does not serve
static HeadsLayout heads_layout(int mask) {
  HeadsLayout L;
  memset(&L, 0, sizeof L);
  L.mask = mask;
  if (mask <= 0 || mask > IH_ALL || mask == (IH_DX | IH_DSHS)) return L;
  int off = IH_BIAS + IH_BIAS_FLOATS;
  for (int k = 0; k < 5; k++) {
    L.first[k] = (mask & ih_first_bit(k)) ? off : -1;
    if (L.first[k] >= 0) off += SLAB;
  }
  L.s2 = (mask & IH_DSHS) ? off : -1;
  if (L.s2 >= 0) off += SLAB;
  L.p2 = (mask & IH_DX) ? off : -1;
  if (L.p2 >= 0) off += IH_SLAB33;
  L.g2 = (mask & (IH_DS | IH_DR | IH_DO)) ? off : -1;
  if (L.g2 >= 0) off += IH_SLAB33;
  L.floats = off;
  if (L.lds_bytes() > (size_t)IH_LDS_LIMIT || L.rows() * 256 > PACK_FLOATS) L.floats = 0;
  return L;
}

static void heads_set_name(int mask, char* buf, size_t n) {
  static const char* names[5] = {"dx", "ds", "dr", "do", "dshs"};
  size_t at = 0;
  buf[0] = 0;
  for (int k = 0; k < 5; k++)
    if ((mask >> k) & 1) at += snprintf(buf + at, at < n ? n - at : 0, "%s%s", at ? " + " : "", names[k]);
  if (!at) snprintf(buf, n, "(empty)");
}

// one workgroup per region: 0, 1 W0 halves | 2..6 first layers | 7 S2 | 8 P2 | 9 geometry second layers | 10 biases and the zeros
// behind the image up to the end of its last DMA row.
// The pointers of an absent head are never read.
__global__ void __launch_bounds__(256) infer_heads_pack_kernel(const s3g_mlp_params w, const s3g_geom_params gw, const HeadsLayout L,
                                                               float* __restrict__ img) {
  const int k = blockIdx.x, tid = threadIdx.x;
  auto slab65 = [&](float* dst, const float* W, int in, int in0, int out) {   // [64 in][65]: dst[i][o] = W[o][in0 + i], rows >= out zero
    for (int e = tid; e < SLAB; e += 256) dst[e] = 0.f;
    __syncthreads();
    for (int e = tid; e < out * 64; e += 256) {
      const int o = e / 64, i = e % 64;
      dst[i * 65 + o] = W[(size_t)o * in + in0 + i];
    }
  };
  if (k <= 1) {
    slab65(img + k * SLAB, w.W0, FEAT, 64 * k, 64);
  } else if (k <= 6) {
    if (L.first[k - 2] < 0) return;
    const float* W = k == 2 ? w.P1 : k == 3 ? w.S1 : k == 4 ? gw.C1 : k == 5 ? gw.R1 : gw.O1;
    slab65(img + L.first[k - 2], W, HID, 0, 64);
  } else if (k == 7) {
    if (L.s2 >= 0) slab65(img + L.s2, w.S2, HID, 0, 48);
  } else if (k == 8) {
    if (L.p2 < 0) return;
    float* dst = img + L.p2;
    for (int e = tid; e < IH_SLAB33; e += 256) dst[e] = 0.f;
    __syncthreads();
    for (int e = tid; e < 3 * 64; e += 256) dst[(e % 64) * 33 + e / 64] = w.P2[e];
  } else if (k == 9) {
    if (L.g2 < 0) return;
    float* dst = img + L.g2;
    for (int e = tid; e < IH_SLAB33; e += 256) dst[e] = 0.f;
    __syncthreads();
    if (L.mask & IH_DS) for (int e = tid; e < 3 * 64; e += 256) dst[(e % 64) * 33 + e / 64] = gw.C2[e];
    if (L.mask & IH_DR) for (int e = tid; e < 4 * 64; e += 256) dst[(e % 64) * 33 + 3 + e / 64] = gw.R2[e];
    if (L.mask & IH_DO) for (int e = tid; e < 1 * 64; e += 256) dst[(e % 64) * 33 + 7] = gw.O2[e];
  } else {
    float* bl = img + IH_BIAS;
    const int m = L.mask;
    for (int e = L.floats + tid; e < L.rows() * 256; e += 256) img[e] = 0.f;
    for (int e = tid; e < IH_BIAS_FLOATS; e += 256) {
      const int v = e >> 6, i = e & 63;
      float x = 0.f;
      if (v == 0) x = w.b0[i];
      else if (v == 1) { if (m & IH_DX) x = w.pb1[i]; }
      else if (v == 2) { if (m & IH_DSHS) x = w.sb1[i]; }
      else if (v == 3) { if (m & IH_DS) x = gw.cb1[i]; }
      else if (v == 4) { if (m & IH_DR) x = gw.rb1[i]; }
      else if (v == 5) { if (m & IH_DO) x = gw.ob1[i]; }
      else if (v == 6) { if ((m & IH_DSHS) && i < 48) x = w.sb2[i]; }
      else if (v == 7) {
        if ((m & IH_DS) && i < 3) x = gw.cb2[i];
        else if ((m & IH_DR) && i >= 4 && i < 8) x = gw.rb2[i - 4];
        else if ((m & IH_DO) && i == 8) x = gw.ob2[0];
      } else if (v == 8) { if ((m & IH_DX) && i < 3) x = w.pb2[i]; }
      bl[e] = x;
    }
  }
}

struct InferHeadsArgs {
  HexArgs h;            // sampler side: descriptor (row tables already swapped in when uniform_time), xyz, time, proc_order, P
  const float* packed;  // infer_heads_pack_kernel's image
  HeadsLayout L;
  float *dx, *ds, *dr, *dopac, *dshs;
};

// geometry head K (0 scales, 1 rotations, 2 opacity) of one tile: geom_head_forward's chain on this image
template <int K>
__device__ __forceinline__ void infer_geom_head(const float* img, const HeadsLayout& L, const f32x16 (&hid)[2], float* out, bool store, size_t pm,
                                                int lane) {
  constexpr int N = K == 0 ? 3 : (K == 1 ? 4 : 1), COL = K == 0 ? 0 : (K == 1 ? 3 : 7), BCOL = 4 * K;
  f32x16 act[2], o[1];
  acc_bias<2>(act, img + IH_BIAS + (3 + K) * 64, lane);
  gemm_reg<2, 2, true>(img + L.first[2 + K], 65, hid, act, lane);
  relu_inplace<2>(act);
  acc_bias<1>(o, img + IH_BIAS + 7 * 64 + BCOL, lane);
  gemm_reg<1, 2, false>(img + L.g2 + COL, 33, act, o, lane);
  if (store) {
    float* row = out + pm * N;
#pragma unroll
    for (int k = 0; k < N; k++) row[k] = o[0][k];
  }
}

template <bool UT>
__global__ void __launch_bounds__(NWAVE * 64) deform_infer_heads_kernel(const InferHeadsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // weights global -> LDS through the DMA path, once per persistent workgroup: whole 1 KiB rows
  for (int c = wave; c < a.L.rows(); c += NWAVE)
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.packed + c * 256 + lane * 4),
                                     (__attribute__((address_space(3))) void*)(lds + c * 256), 16, 0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const float* img = lds;
  auto bias = [&](int v) { return img + IH_BIAS + v * 64; };
  float* stage = lds + a.L.floats + wave * INF_WAVE_FLOATS;
  const int slot = lane >> 3, j8 = lane & 7, c4 = j8 * 4;   // sampler role: point slot, channel quad
  const int jj = lane & 31, hh = lane >> 5;                 // MFMA role: point column, row half
  float4* tp0 = reinterpret_cast<float4*>(stage + STG_FLOATS) + slot * INF_TAP_STRIDE;   // two sets of tap slots per point slot
  float4* tp1 = tp0 + 8 * INF_TAP_STRIDE;
  const InferSampler<UT> sampler{a.h, stage, slot, j8, c4, tp0, tp1};
  const int P = a.h.P, ntiles = (P + MT - 1) / MT;
  const int mask = a.L.mask;
  for (int tile = blockIdx.x * NWAVE + wave; tile < ntiles; tile += gridDim.x * NWAVE) {
    const int p0 = tile * MT;
    const int posm = p0 + jj;
    const bool livem = posm < P;
    const size_t pm = livem ? (size_t)(a.h.proc_order ? a.h.proc_order[posm] : (uint32_t)posm) : 0;
    if (hh == 0) {   // one lane per point: coordinates -> the pad of the point's staging row
      float u[4];
      point_coords(a.h, (int)pm, u);
      *reinterpret_cast<float4*>(stage + jj * STG_LD + 32) = make_float4(u[0], u[1], u[2], u[3]);
    }
    f32x16 hid[2];
    acc_bias<2>(hid, bias(0), lane);
    wave_lds_sync();
    auto level_gemm = [&](int l) {   // the level's tile is complete: re-read it in the MFMA B-operand layout, K quarter l of feature_out
      f32x16 x[1];
      wave_lds_sync();
#pragma unroll
      for (int q = 0; q < 4; q++) {   // channels 8q + 4h .. +3 of point jj: the chunk act_load would have read from HBM
        const float4 v = *reinterpret_cast<const float4*>(stage + jj * STG_LD + 8 * q + 4 * hh);
        x[0][4 * q + 0] = v.x; x[0][4 * q + 1] = v.y; x[0][4 * q + 2] = v.z; x[0][4 * q + 3] = v.w;
      }
      gemm_reg<2, 1, false>(img + (l >> 1) * SLAB + 32 * (l & 1) * 65, 65, x, hid, lane);
    };
    sampler.run(level_gemm);
    const bool store = livem && hh == 0;   // the 3 / 4 / 1-wide outputs: rows 0 .. N-1 sit in registers 0 .. N-1 of the h = 0 lanes
    int ln = lane;
    asm volatile("" : "+v"(ln));   // the heads' LDS addresses (image offsets from the argument struct) are derived here, not carried across the sampler steps
    if (mask & IH_DX) {
      // pos head: dx = P2 relu(P1 relu(hidden) + pb1) + pb2
      f32x16 act[2];
      acc_bias<2>(act, bias(1), ln);
      gemm_reg<2, 2, true>(img + a.L.first[0], 65, hid, act, ln);
      relu_inplace<2>(act);
      float o3[3] = {0.f, 0.f, 0.f};
      head3_fw(img + a.L.p2, bias(8), act, o3, ln);
      if (store) {
        float* row = a.dx + pm * 3;
        row[0] = o3[0]; row[1] = o3[1]; row[2] = o3[2];
      }
    }
    if (mask & IH_DSHS) {
      // shs head: dshs = S2 relu(S1 relu(hidden) + sb1) + sb2
      f32x16 act[2], acc[2];
      acc_bias<2>(act, bias(2), ln);
      gemm_reg<2, 2, true>(img + a.L.first[1], 65, hid, act, ln);
      relu_inplace<2>(act);
      acc_bias<2>(acc, bias(6), ln);
      gemm_reg<2, 2, false>(img + a.L.s2, 65, act, acc, ln);
      if (livem) {
        float* row = a.dshs + pm * 48 + 4 * (ln >> 5);
#pragma unroll
        for (int mb = 0; mb < 2; mb++)
#pragma unroll
          for (int q = 0; q < 4; q++) {
            if (32 * mb + 8 * q >= 48) continue;
            *reinterpret_cast<float4*>(row + 32 * mb + 8 * q) =
                make_float4(acc[mb][4 * q + 0], acc[mb][4 * q + 1], acc[mb][4 * q + 2], acc[mb][4 * q + 3]);
          }
      }
    }
    if (mask & IH_DS) infer_geom_head<0>(img, a.L, hid, a.ds, store, pm, ln);
    if (mask & IH_DR) infer_geom_head<1>(img, a.L, hid, a.dr, store, pm, ln);
    if (mask & IH_DO) infer_geom_head<2>(img, a.L, hid, a.dopac, store, pm, ln);
    wave_lds_sync();   // the next tile's coordinates go into the pads this tile's taps were derived from
  }
}

}  // namespace s3g

using namespace s3g;

extern "C" size_t s3g_deform_infer_heads_lds_bytes(int head_mask) {
  const HeadsLayout L = heads_layout(head_mask);
  return L.floats ? L.lds_bytes() : 0;
}

extern "C" int s3g_deform_infer_heads(const s3g_hexplane_desc* d, const s3g_mlp_params* w, const s3g_geom_params* gw, int P, const float* xyz,
                                      const float* time, const unsigned int* proc_order, float* dx, float* dshs, float* ds, float* dr,
                                      float* dopac, void* workspace, void* stream_) {
  if (int e = check_desc(d)) return e;
  if (d->levels != 4) {
    set_error("s3g_deform_infer_heads: the fused path is built for 4 levels x 32 channels = feature_out's 128 inputs");
    return S3G_ERR_INVALID_ARG;
  }
  const int mask = (dx ? IH_DX : 0) | (ds ? IH_DS : 0) | (dr ? IH_DR : 0) | (dopac ? IH_DO : 0) | (dshs ? IH_DSHS : 0);
  const HeadsLayout L = heads_layout(mask);
  if (!L.floats) {
    char name[64];
    heads_set_name(mask, name, sizeof name);
    set_error("s3g_deform_infer_heads: the head set %s is not served by this kernel (%s): use s3g_hexplane_forward + s3g_deform_mlp_forward "
              "+ s3g_deform_geom_forward%s", name,
              mask == 0 ? "no head asked for" : mask == (IH_DX | IH_DSHS) ? "s3g_deform_infer's own set" : "its weight image does not fit the LDS",
              mask == (IH_DX | IH_DSHS) ? ", or s3g_deform_infer" : "");
    return S3G_ERR_INVALID_ARG;
  }
  const bool geom = (mask & (IH_DS | IH_DR | IH_DO)) != 0;
  bool ok = w && w->W0 && w->b0 && P >= 0 && (!geom || gw);
  if (ok && dx) ok = w->P1 && w->pb1 && w->P2 && w->pb2;
  if (ok && dshs) ok = w->S1 && w->sb1 && w->S2 && w->sb2;
  if (ok && ds) ok = gw->C1 && gw->cb1 && gw->C2 && gw->cb2;
  if (ok && dr) ok = gw->R1 && gw->rb1 && gw->R2 && gw->rb2;
  if (ok && dopac) ok = gw->O1 && gw->ob1 && gw->O2 && gw->ob2;
  if (!ok || (P > 0 && (!xyz || !time || !workspace))) {
    set_error("s3g_deform_infer_heads: bad argument (NULL weights of a requested head, or a NULL buffer)");
    return S3G_ERR_INVALID_ARG;
  }
  if (P == 0) return S3G_OK;
  hipStream_t stream = (hipStream_t)stream_;
  static std::atomic<uint64_t> done{0};
  if (device_needs_setup(done)) {
    size_t most = 0;   // the largest set served
    for (int m = 1; m <= IH_ALL; m++) {
      const HeadsLayout Lm = heads_layout(m);
      if (Lm.floats) most = max(most, Lm.lds_bytes());
    }
    S3G_HIP_CHECK(hipFuncSetAttribute((const void*)deform_infer_heads_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)most));
    S3G_HIP_CHECK(hipFuncSetAttribute((const void*)deform_infer_heads_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)most));
    device_setup_done(done);
  }
  float* packed = (float*)workspace;
  InferHeadsArgs a;
  memset(&a, 0, sizeof a);
  a.h.d = *d; a.h.P = P; a.h.xyz = xyz; a.h.time = time; a.h.proc_order = proc_order;
  a.packed = packed; a.L = L;
  a.dx = dx; a.ds = ds; a.dr = dr; a.dopac = dopac; a.dshs = dshs;
  TimeRows rows;
  if (d->uniform_time) use_time_rows(a.h, rows, packed + PACK_FLOATS, nullptr, stream);
  s3g_geom_params g;
  memset(&g, 0, sizeof g);
  if (gw) g = *gw;
  hipLaunchKernelGGL(infer_heads_pack_kernel, dim3(11), dim3(256), 0, stream, *w, g, L, packed);
  const int ntiles = (P + MT - 1) / MT;
  const int blocks = min((ntiles + NWAVE - 1) / NWAVE, 256);
  const dim3 grid(blocks), wg(NWAVE * 64);
  const size_t lds_bytes = L.lds_bytes();
  profile_begin(S3G_PROFILE_DEFORM_INFER_HEADS, stream);
  if (d->uniform_time) hipLaunchKernelGGL((deform_infer_heads_kernel<true>), grid, wg, lds_bytes, stream, a);
  else hipLaunchKernelGGL((deform_infer_heads_kernel<false>), grid, wg, lds_bytes, stream, a);
  profile_end(S3G_PROFILE_DEFORM_INFER_HEADS, stream, (double)P, 4.0);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}
