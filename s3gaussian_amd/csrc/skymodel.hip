// Sky colour model (include/s3g_skymodel.h) for gfx950: view direction -> 33 sinusoidal values -> 33->256 -> [256+33]->256 -> 256->3
// -> sigmoid, composited behind the Gaussians, and its backward.  Exact fp32: every product runs on v_mfma_f32_32x32x2_f32 as
// k-ordered fma chains (the arithmetic of lpips_conv.hpp).
//
//   sky_tile_kernel<false>   one workgroup (4 waves) owns SKY_T = 64 pixels.  The activations live in LDS as act[k][pixel]
//                            (rows 0..255 h0, then h1; rows 256..289 the encoding and one zero row that makes K even), so the
//                            operand read of a layer is act[k][lane & 31]: consecutive words.  A wave owns 64 output channels x
//                            64 pixels (2 x 2 tiles); the weights are read from the packed image Wt[k][channel] in global memory
//                            (L2 resident: 0.6 MB), 128 consecutive bytes per half wave.  Output tile D[channel][pixel]: the lane
//                            holds the pixel, so the store back into act[channel][pixel] is conflict free as well.
//   sky_tile_kernel<true>    the same recompute, then dz2, g_alpha, dz1 (K = 3, VALU) and dz0 = W1[:, :256]^T dz1 (MFMA), every
//                            matrix the weight gradients need written to the band's scratch as rows per pixel.
//   sky_wgrad_kernel         dW partial of one chunk: D[out][in] = sum over the chunk's pixels of dz[p][out] x[p][in]; a wave owns a
//                            64 x 64 (or 32 x 64) block and reads both operands from the scratch rows, coalesced.
//   sky_bias_kernel          column sums of dz over a chunk, in double.
//   sky_fold_kernel          accumulator (double) += the chunks in order; the last band also rounds to the fp32 outputs.
// No kernel keeps or reads anything but its arguments; every extent comes from s3g_skymodel_plan.
#include "common.hpp"

#include <algorithm>

#include "../../include/s3g_skymodel.h"

namespace s3g {

typedef float sky_f32x16 __attribute__((ext_vector_type(16)));

constexpr int SKY_T = 64;                    // pixels per tile
constexpr int SKY_C = 256;                   // width
constexpr int SKY_E = 33, SKY_EP = 34;       // encoding, padded to an even K
constexpr int SKY_K1 = SKY_C + SKY_EP;       // 290: K of layer 1 ([h0, e, 0])
constexpr int SKY_LD = SKY_T + 1;            // LDS row stride: a transposed read (lanes along k) is conflict free
constexpr int SKY_XLD = 320, SKY_ZLD = 32;   // scratch row strides of [h0, e, 0...] and of dz2
constexpr int SKY_CHUNK = S3G_SKYMODEL_CHUNK_PIXELS;
constexpr int SKY_NP = S3G_SKYMODEL_PARAMS, SKY_NB = 2 * SKY_C + 3;
// flat parameter order
constexpr int SKY_OFF_W0 = 0, SKY_OFF_B0 = SKY_C * SKY_E, SKY_OFF_W1 = SKY_OFF_B0 + SKY_C, SKY_OFF_B1 = SKY_OFF_W1 + SKY_C * (SKY_C + SKY_E),
              SKY_OFF_W2 = SKY_OFF_B1 + SKY_C, SKY_OFF_B2 = SKY_OFF_W2 + 3 * SKY_C;
static_assert(SKY_OFF_B2 + 3 == SKY_NP, "flat parameter order");
// packed image (floats)
constexpr int PK_WT0 = 0;                               // [34][256]   Wt0[k][c] = W0[c][k], row 33 zero
constexpr int PK_WT1 = PK_WT0 + SKY_EP * SKY_C;         // [290][256]  Wt1[k][c] = W1[c][k], row 289 zero
constexpr int PK_WT2 = PK_WT1 + SKY_K1 * SKY_C;         // [256][32]   Wt2[k][c] = W2[c][k], columns 3.. zero
constexpr int PK_B0 = PK_WT2 + SKY_C * 32, PK_B1 = PK_B0 + SKY_C, PK_B2 = PK_B1 + SKY_C;   // b2 padded to 32
constexpr int PK_W1H = PK_B2 + 32;                      // [256 out][256 in]  W1[:, :256]
constexpr int PK_W2 = PK_W1H + SKY_C * SKY_C;           // [3][256]
constexpr int PK_FLOATS = PK_W2 + 3 * SKY_C;

struct SkyCam {
  float R[9];
  float fx, fy, cx, cy;
  int width, n_pixels;
};

__global__ void __launch_bounds__(256) sky_pack_kernel(const float* __restrict__ W0, const float* __restrict__ b0, const float* __restrict__ W1,
                                                       const float* __restrict__ b1, const float* __restrict__ W2, const float* __restrict__ b2,
                                                       float* __restrict__ pack) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= PK_FLOATS) return;
  float v = 0.f;
  if (i < PK_WT1) {
    const int k = i / SKY_C, c = i - k * SKY_C;
    if (k < SKY_E) v = W0[c * SKY_E + k];
  } else if (i < PK_WT2) {
    const int j = i - PK_WT1, k = j / SKY_C, c = j - k * SKY_C;
    if (k < SKY_C + SKY_E) v = W1[c * (SKY_C + SKY_E) + k];
  } else if (i < PK_B0) {
    const int j = i - PK_WT2, k = j >> 5, c = j & 31;
    if (c < 3) v = W2[c * SKY_C + k];
  } else if (i < PK_B1) {
    v = b0[i - PK_B0];
  } else if (i < PK_B2) {
    v = b1[i - PK_B1];
  } else if (i < PK_W1H) {
    if (i - PK_B2 < 3) v = b2[i - PK_B2];
  } else if (i < PK_W2) {
    const int j = i - PK_W1H, o = j / SKY_C, c = j - o * SKY_C;
    v = W1[o * (SKY_C + SKY_E) + c];
  } else {
    v = W2[i - PK_W2];
  }
  pack[i] = v;
}

// Value j of the encoding of the unit direction (v0, v1, v2): [v, sin(2^s v_a) at 3 + 3 s + a, sin(2^s v_a + pi/2) at 18 + 3 s + a].
__device__ __forceinline__ float sky_encode(float v0, float v1, float v2, int j) {
  if (j < 3) return j == 0 ? v0 : (j == 1 ? v1 : v2);
  if (j >= SKY_E) return 0.f;
  const bool shifted = j >= 18;
  const int q = j - (shifted ? 18 : 3), s = q / 3, a = q - 3 * s;
  float x = (a == 0 ? v0 : (a == 1 ? v1 : v2)) * (float)(1 << s);   // exact
  if (shifted) x = x + (float)(0.5 * 3.141592653589793);
  return sinf(x);
}

#define SKY_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

// tile_begin: the first pixel of this launch (0 for the forward, the band's first pixel for the backward).  Scratch rows are
// relative to tile_begin.  Pixels >= cam.n_pixels are computed on zeros and never read from or written to memory.
template <bool BWD>
__global__ void __launch_bounds__(256) sky_tile_kernel(SkyCam cam, int tile_begin, const float* __restrict__ pack,
                                                       const float* __restrict__ render, const float* __restrict__ alpha,
                                                       float* __restrict__ out, const float* __restrict__ g_image, float* __restrict__ g_alpha,
                                                       float* __restrict__ X1, float* __restrict__ H1, float* __restrict__ dZ1,
                                                       float* __restrict__ dZ0, float* __restrict__ dZ2) {
  __shared__ float act[SKY_K1][SKY_LD];
  __shared__ float dz2s[3][SKY_T];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, r = lane & 31;
  const int n = cam.n_pixels;
  const int row0 = blockIdx.x * SKY_T;          // first scratch row of the tile
  const int p0 = tile_begin + row0;             // first pixel of the tile
  const int c0 = wave * 64;                     // the wave's output channels

  {  // direction and encoding: pixel tid & 63, values (tid >> 6) + 4 i
    const int pl = tid & (SKY_T - 1), part = tid >> 6, p = p0 + pl;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;
    const bool valid = p < n;
    if (valid) {
      const int y = p / cam.width, x = p - y * cam.width;
      const float dx = ((float)x - cam.cx + 0.5f) / cam.fx, dy = ((float)y - cam.cy + 0.5f) / cam.fy;
      const float d0 = (cam.R[0] * dx + cam.R[1] * dy) + cam.R[2];
      const float d1 = (cam.R[3] * dx + cam.R[4] * dy) + cam.R[5];
      const float d2 = (cam.R[6] * dx + cam.R[7] * dy) + cam.R[8];
      const float inv = sqrtf((d0 * d0 + d1 * d1) + d2 * d2) + 1e-8f;
      v0 = d0 / inv; v1 = d1 / inv; v2 = d2 / inv;
    }
    for (int j = part; j < SKY_EP; j += 4) act[SKY_C + j][pl] = valid ? sky_encode(v0, v1, v2, j) : 0.f;
  }
  __syncthreads();

  sky_f32x16 acc00, acc01, acc10, acc11;   // [channel tile][pixel tile]; separate objects (lpips_conv.hpp on why)
  auto zero = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 16; i++) acc00[i] = acc01[i] = acc10[i] = acc11[i] = 0.f;
  };
  // acc[ct][pt] += sum_k A[k][c0 + 32 ct + i] act[krow0 + k][32 pt + j]; operand maps A[i = lane & 31][k = lane >> 5], B[k][j]
  auto gemm = [&](const float* __restrict__ A, int K, int krow0) __attribute__((always_inline)) {
#pragma unroll 4
    for (int k = 0; k < K; k += 2) {
      const int kk = k + half;
      const float a0 = A[kk * SKY_C + c0 + r], a1 = A[kk * SKY_C + c0 + 32 + r];
      const float b0 = act[krow0 + kk][r], b1 = act[krow0 + kk][32 + r];
      acc00 = SKY_MFMA(a0, b0, acc00);
      acc01 = SKY_MFMA(a0, b1, acc01);
      acc10 = SKY_MFMA(a1, b0, acc10);
      acc11 = SKY_MFMA(a1, b1, acc11);
    }
  };
  // C/D map: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  act[channel][pixel] <- f(acc + bias)
  auto store = [&](const float* __restrict__ bias, bool relu) __attribute__((always_inline)) {
#pragma unroll
    for (int reg = 0; reg < 16; reg++) {
      const int cr = (reg & 3) + 8 * (reg >> 2) + 4 * half;
      const int ca = c0 + cr, cb = c0 + 32 + cr;
      const float ba = bias ? bias[ca] : 0.f, bb = bias ? bias[cb] : 0.f;
      float v00 = acc00[reg] + ba, v01 = acc01[reg] + ba, v10 = acc10[reg] + bb, v11 = acc11[reg] + bb;
      if (relu) { v00 = fmaxf(v00, 0.f); v01 = fmaxf(v01, 0.f); v10 = fmaxf(v10, 0.f); v11 = fmaxf(v11, 0.f); }
      act[ca][r] = v00; act[ca][32 + r] = v01; act[cb][r] = v10; act[cb][32 + r] = v11;
    }
  };
  // scratch rows <- act rows 0 .. nreal - 1 (zeros up to ncols), one pixel row per pass, thread = column: coalesced, and the
  // LDS read act[c][pl] over consecutive c is conflict free with the odd row stride
  auto dump = [&](float* __restrict__ dst, int ld, int ncols, int nreal, bool mask_h0) __attribute__((always_inline)) {
    for (int pl = 0; pl < SKY_T && p0 + pl < n; pl++)
      for (int c = tid; c < ncols; c += 256) {
        float v = c < nreal ? act[c][pl] : 0.f;
        if (mask_h0 && !(X1[(size_t)(row0 + pl) * SKY_XLD + c] > 0.f)) v = 0.f;   // the same thread wrote X1[.][c]
        dst[(size_t)(row0 + pl) * ld + c] = v;
      }
  };

  // layer 0: K = 34 over the encoding rows
  zero();
  gemm(pack + PK_WT0, SKY_EP, SKY_C);
  store(pack + PK_B0, true);   // rows 0..255 are not read by layer 0: no barrier in front
  __syncthreads();
  if constexpr (BWD) dump(X1, SKY_XLD, SKY_XLD, SKY_K1, false);

  // layer 1: K = 290 over [h0, e, 0]
  zero();
  gemm(pack + PK_WT1, SKY_K1, 0);
  __syncthreads();             // everyone is done reading h0
  store(pack + PK_B1, true);
  __syncthreads();
  if constexpr (BWD) dump(H1, SKY_C, SKY_C, SKY_C, false);

  // layer 2: 3 channels padded to one tile of 32; waves 0 and 1 take one pixel tile each (the branch is uniform over the wave)
  if (wave < 2) {
    sky_f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; i++) z[i] = 0.f;
    const float* __restrict__ A = pack + PK_WT2;
#pragma unroll 4
    for (int k = 0; k < SKY_C; k += 2) {
      const int kk = k + half;
      z = SKY_MFMA(A[kk * 32 + r], act[kk][wave * 32 + r], z);
    }
    const int pl = wave * 32 + r, p = p0 + pl;
    if (half == 0 && p < n) {   // rows 0, 1, 2 of the tile are registers 0, 1, 2 of the lower half wave
      const float s0 = 1.f / (1.f + expf(-(z[0] + pack[PK_B2 + 0])));
      const float s1 = 1.f / (1.f + expf(-(z[1] + pack[PK_B2 + 1])));
      const float s2 = 1.f / (1.f + expf(-(z[2] + pack[PK_B2 + 2])));
      const float one_m_a = 1.f - (alpha ? alpha[p] : 0.f);
      if constexpr (!BWD) {
        const size_t N = (size_t)n;
        out[p] = (render ? render[p] : 0.f) + one_m_a * s0;
        out[N + p] = (render ? render[N + p] : 0.f) + one_m_a * s1;
        out[2 * N + p] = (render ? render[2 * N + p] : 0.f) + one_m_a * s2;
      } else {
        const size_t N = (size_t)n;
        const float g0 = g_image[p], g1 = g_image[N + p], g2 = g_image[2 * N + p];
        if (g_alpha) g_alpha[p] = -((g0 * s0 + g1 * s1) + g2 * s2);
        const float q0 = (g0 * one_m_a) * (s0 * (1.f - s0)), q1 = (g1 * one_m_a) * (s1 * (1.f - s1)),
                    q2 = (g2 * one_m_a) * (s2 * (1.f - s2));
        dz2s[0][pl] = q0; dz2s[1][pl] = q1; dz2s[2][pl] = q2;
        float4* zrow = reinterpret_cast<float4*>(dZ2 + (size_t)(row0 + pl) * SKY_ZLD);
        zrow[0] = make_float4(q0, q1, q2, 0.f);
#pragma unroll
        for (int i = 1; i < SKY_ZLD / 4; i++) zrow[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    } else if (BWD && half == 0) {
      dz2s[0][pl] = 0.f; dz2s[1][pl] = 0.f; dz2s[2][pl] = 0.f;
    }
  }
  if constexpr (BWD) {
    __syncthreads();
    // dz1 = (W2^T dz2) where h1 > 0, in place; one channel per wave and pass (its three weights are uniform)
    const float* __restrict__ W2 = pack + PK_W2;
    for (int idx = tid; idx < SKY_C * SKY_T; idx += 256) {
      const int c = idx >> 6, pl = idx & 63;
      const float d = (W2[c] * dz2s[0][pl] + W2[SKY_C + c] * dz2s[1][pl]) + W2[2 * SKY_C + c] * dz2s[2][pl];
      act[c][pl] = act[c][pl] > 0.f ? d : 0.f;
    }
    __syncthreads();
    dump(dZ1, SKY_C, SKY_C, SKY_C, false);
    // dz0 = (W1[:, :256]^T dz1) where h0 > 0: K = the 256 output channels of layer 1
    zero();
    gemm(pack + PK_W1H, SKY_C, 0);
    __syncthreads();           // everyone is done reading dz1
    store(nullptr, false);
    __syncthreads();
    dump(dZ0, SKY_C, SKY_C, SKY_C, true);
  }
}

// Partial weight gradient of one chunk: D[m][n] = sum over the chunk's rows p of A[p][m] B[p][n].  Wave-block wb = 4 blockIdx.x +
// wave owns rows 32 TM (wb / nblk_n) .. and columns 64 (wb % nblk_n) ..; rows p >= n_rows contribute zeros.  A and B have at
// least 32 TM nblk_m and 64 nblk_n columns.  Stored where m < m_real and n < n_real into partial[chunk][m n_real + n].
template <int TM>
__global__ void __launch_bounds__(256) sky_wgrad_kernel(const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb, int n_rows,
                                                        int nblk_m, int nblk_n, int m_real, int n_real, float* __restrict__ partial) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, r = lane & 31;
  const int wb = blockIdx.x * 4 + wave;
  if (wb >= nblk_m * nblk_n) return;    // uniform over the wave; the kernel has no barrier
  const int bm = wb / nblk_n, bn = wb - bm * nblk_n;
  const int k0 = blockIdx.y * SKY_CHUNK;
  const int kend = min(k0 + SKY_CHUNK, n_rows);
  const float* __restrict__ Ap = A + bm * 32 * TM + r;
  const float* __restrict__ Bp = B + bn * 64 + r;
  sky_f32x16 acc00, acc01, acc10, acc11;
#pragma unroll
  for (int i = 0; i < 16; i++) acc00[i] = acc01[i] = acc10[i] = acc11[i] = 0.f;
#pragma unroll 4
  for (int s = 0; s < SKY_CHUNK; s += 2) {   // a fixed trip count (it unrolls); the rows past the band's end are zeros
    const int kk = k0 + s + half;
    const bool valid = kk < kend;
    const float a0 = valid ? Ap[(size_t)kk * lda] : 0.f;
    const float b0 = valid ? Bp[(size_t)kk * ldb] : 0.f, b1 = valid ? Bp[(size_t)kk * ldb + 32] : 0.f;
    acc00 = SKY_MFMA(a0, b0, acc00);
    acc01 = SKY_MFMA(a0, b1, acc01);
    if constexpr (TM == 2) {
      const float a1 = valid ? Ap[(size_t)kk * lda + 32] : 0.f;
      acc10 = SKY_MFMA(a1, b0, acc10);
      acc11 = SKY_MFMA(a1, b1, acc11);
    }
  }
  float* __restrict__ dst = partial + (size_t)blockIdx.y * SKY_NP;
  const int na = bn * 64 + r, nb = na + 32;
#pragma unroll
  for (int reg = 0; reg < 16; reg++) {
    const int ma = bm * 32 * TM + (reg & 3) + 8 * (reg >> 2) + 4 * half, mb = ma + 32;
    if (ma < m_real) {
      if (na < n_real) dst[(size_t)ma * n_real + na] = acc00[reg];
      if (nb < n_real) dst[(size_t)ma * n_real + nb] = acc01[reg];
    }
    if (TM == 2 && mb < m_real) {
      if (na < n_real) dst[(size_t)mb * n_real + na] = acc10[reg];
      if (nb < n_real) dst[(size_t)mb * n_real + nb] = acc11[reg];
    }
  }
}

// Column sums of dz0 (blockIdx.x = 0), dz1 (1) and dz2 (2) over chunk blockIdx.y, in double, rows in order.
__global__ void __launch_bounds__(256) sky_bias_kernel(const float* __restrict__ dZ0, const float* __restrict__ dZ1, const float* __restrict__ dZ2,
                                                       int n_rows, double* __restrict__ bpart) {
  const int which = blockIdx.x, c = threadIdx.x;
  const float* __restrict__ M = which == 0 ? dZ0 : (which == 1 ? dZ1 : dZ2);
  const int ld = which == 2 ? SKY_ZLD : SKY_C, ncols = which == 2 ? 3 : SKY_C;
  if (c >= ncols) return;
  const int k0 = blockIdx.y * SKY_CHUNK, kend = min(k0 + SKY_CHUNK, n_rows);
  double s = 0.0;
  for (int k = k0; k < kend; k++) s += (double)M[(size_t)k * ld + c];
  bpart[(size_t)blockIdx.y * SKY_NB + which * SKY_C + c] = s;
}

// accum[i] = (first band ? 0 : accum[i]) + the band's chunks in order; the last band rounds to d_params.
__global__ void __launch_bounds__(256) sky_fold_kernel(int nchunks, const float* __restrict__ wpart, const double* __restrict__ bpart,
                                                       int first, int last, double* __restrict__ accum, float* __restrict__ d_params) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= SKY_NP) return;
  int bias = -1;   // index into a chunk's bias partials, or -1 for a weight
  if (i >= SKY_OFF_B2) bias = 2 * SKY_C + (i - SKY_OFF_B2);
  else if (i >= SKY_OFF_B1 && i < SKY_OFF_W2) bias = SKY_C + (i - SKY_OFF_B1);
  else if (i >= SKY_OFF_B0 && i < SKY_OFF_W1) bias = i - SKY_OFF_B0;
  double s = first ? 0.0 : accum[i];
  if (bias >= 0)
    for (int c = 0; c < nchunks; c++) s += bpart[(size_t)c * SKY_NB + bias];
  else
    for (int c = 0; c < nchunks; c++) s += (double)wpart[(size_t)c * SKY_NP + i];
  accum[i] = s;
  if (last) d_params[i] = (float)s;
}

// The band's scratch, its chunk partials and the accumulator, carved from one workspace.
struct SkyWork {
  float *X1, *H1, *dZ1, *dZ0, *dZ2, *wpart;
  double *bpart, *accum;
  size_t bytes;
  SkyWork(void* base, const s3g_skymodel_extents& e) {
    Carver cv(base);
    const size_t rows = (size_t)e.band_pixels;
    X1 = cv.take<float>(rows * SKY_XLD);
    H1 = cv.take<float>(rows * SKY_C);
    dZ1 = cv.take<float>(rows * SKY_C);
    dZ0 = cv.take<float>(rows * SKY_C);
    dZ2 = cv.take<float>(rows * SKY_ZLD);
    wpart = cv.take<float>((size_t)e.chunks * SKY_NP);
    bpart = cv.take<double>((size_t)e.chunks * SKY_NB);
    accum = cv.take<double>(SKY_NP);
    bytes = cv.bytes();
  }
};

static SkyCam sky_cam(const s3g_skymodel_camera* c, int W, int n) {
  SkyCam k;
  for (int i = 0; i < 9; i++) k.R[i] = (float)c->R[i];
  k.fx = (float)c->fx; k.fy = (float)c->fy; k.cx = (float)c->cx; k.cy = (float)c->cy;
  k.width = W;
  k.n_pixels = n;
  return k;
}

}  // namespace s3g

using namespace s3g;

extern "C" int s3g_skymodel_tile_pixels(void) { return SKY_T; }

extern "C" size_t s3g_skymodel_pack_bytes(void) { return (size_t)PK_FLOATS * sizeof(float); }

extern "C" int s3g_skymodel_plan(long long n_pixels, int band_pixels, s3g_skymodel_extents* out) {
  clear_error();
  if (!out || n_pixels < 1 || n_pixels >= 0x7fffffffLL - SKY_T) {
    set_error("s3g_skymodel_plan: needs 1 <= n_pixels < 2^31 - %d and an output record", SKY_T);
    return S3G_ERR_INVALID_ARG;
  }
  const long long tiles = (n_pixels + SKY_T - 1) / SKY_T;
  long long band = band_pixels > 0 ? band_pixels : S3G_SKYMODEL_DEFAULT_BAND;
  band = (band + SKY_T - 1) / SKY_T * SKY_T;
  if (band > tiles * SKY_T) band = tiles * SKY_T;
  s3g_skymodel_extents e;
  e.tile_pixels = SKY_T;
  e.tiles = (int)tiles;
  e.band_pixels = (int)band;
  e.bands = (int)((n_pixels + band - 1) / band);
  e.chunks = (int)((band + SKY_CHUNK - 1) / SKY_CHUNK);
  e.reserved = 0;
  e.workspace_bytes = 0;
  e.workspace_bytes = SkyWork(nullptr, e).bytes;
  *out = e;
  return S3G_OK;
}

extern "C" int s3g_sky_pack(const float* W0, const float* b0, const float* W1, const float* b1, const float* W2, const float* b2,
                            float* pack, void* stream_) {
  clear_error();
  if (!W0 || !b0 || !W1 || !b1 || !W2 || !b2 || !pack) {
    set_error("s3g_sky_pack: NULL array argument");
    return S3G_ERR_INVALID_ARG;
  }
  hipLaunchKernelGGL(sky_pack_kernel, dim3((PK_FLOATS + 255) / 256), dim3(256), 0, (hipStream_t)stream_, W0, b0, W1, b1, W2, b2, pack);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" int s3g_sky_forward(int H, int W, const s3g_skymodel_camera* cam, const float* pack, const float* render, const float* alpha,
                               float* out, void* stream_) {
  clear_error();
  if (H < 1 || W < 1 || !cam || !pack || !out) {
    set_error("s3g_sky_forward: bad argument (empty image, or NULL camera, pack or output)");
    return S3G_ERR_INVALID_ARG;
  }
  s3g_skymodel_extents e;
  if (int rc = s3g_skymodel_plan((long long)H * W, 0, &e)) return rc;
  const int n = H * W;
  hipLaunchKernelGGL(sky_tile_kernel<false>, dim3((unsigned)e.tiles), dim3(256), 0, (hipStream_t)stream_, sky_cam(cam, W, n), 0, pack,
                     render, alpha, out, (const float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr,
                     (float*)nullptr, (float*)nullptr);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" int s3g_sky_backward(int H, int W, const s3g_skymodel_camera* cam, const float* pack, const float* alpha, const float* g_image,
                                int band_pixels, float* d_params, float* g_alpha, void* workspace, void* stream_) {
  clear_error();
  if (H < 1 || W < 1 || !cam || !pack || !g_image || !d_params || !workspace) {
    set_error("s3g_sky_backward: bad argument (empty image, or NULL camera, pack, gradient, output or workspace)");
    return S3G_ERR_INVALID_ARG;
  }
  s3g_skymodel_extents e;
  if (int rc = s3g_skymodel_plan((long long)H * W, band_pixels, &e)) return rc;
  const int n = H * W;
  const SkyWork w(workspace, e);
  const SkyCam k = sky_cam(cam, W, n);
  hipStream_t stream = (hipStream_t)stream_;
  for (int band = 0; band < e.bands; band++) {
    const int begin = band * e.band_pixels;
    const int rows = std::min(e.band_pixels, n - begin);                 // this band's pixels
    const unsigned tiles = (unsigned)((rows + SKY_T - 1) / SKY_T);
    const unsigned chunks = (unsigned)((rows + SKY_CHUNK - 1) / SKY_CHUNK);   // <= e.chunks
    hipLaunchKernelGGL(sky_tile_kernel<true>, dim3(tiles), dim3(256), 0, stream, k, begin, pack, (const float*)nullptr, alpha,
                       (float*)nullptr, g_image, g_alpha, w.X1, w.H1, w.dZ1, w.dZ0, w.dZ2);
    S3G_HIP_CHECK(hipGetLastError());
    // dW0 [256][33] = dz0^T e: 4 x 1 wave-blocks;  dW1 [256][289] = dz1^T [h0, e]: 4 x 5;  dW2 [3][256] = dz2^T h1: 1 x 4
    hipLaunchKernelGGL(sky_wgrad_kernel<2>, dim3(1, chunks), dim3(256), 0, stream, (const float*)w.dZ0, SKY_C, (const float*)w.X1 + SKY_C,
                       SKY_XLD, rows, 4, 1, SKY_C, SKY_E, w.wpart + SKY_OFF_W0);
    S3G_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(sky_wgrad_kernel<2>, dim3(5, chunks), dim3(256), 0, stream, (const float*)w.dZ1, SKY_C, (const float*)w.X1, SKY_XLD,
                       rows, 4, 5, SKY_C, SKY_C + SKY_E, w.wpart + SKY_OFF_W1);
    S3G_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(sky_wgrad_kernel<1>, dim3(1, chunks), dim3(256), 0, stream, (const float*)w.dZ2, SKY_ZLD, (const float*)w.H1, SKY_C,
                       rows, 1, 4, 3, SKY_C, w.wpart + SKY_OFF_W2);
    S3G_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(sky_bias_kernel, dim3(3, chunks), dim3(256), 0, stream, (const float*)w.dZ0, (const float*)w.dZ1,
                       (const float*)w.dZ2, rows, w.bpart);
    S3G_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(sky_fold_kernel, dim3((SKY_NP + 255) / 256), dim3(256), 0, stream, (int)chunks, (const float*)w.wpart,
                       (const double*)w.bpart, band == 0 ? 1 : 0, band == e.bands - 1 ? 1 : 0, w.accum, d_params);
    S3G_HIP_CHECK(hipGetLastError());
  }
  return S3G_OK;
}
