// Geometry heads of the deformation MLP (scales_deform / rotations_deform / opacity_deform; ModelHiddenParams no_ds / no_dr / no_do
// = False): a second, self-contained kernel family beside mlp.hip, and the C API of include/s3g_mlp_geom.h.
//
// Why its own family: the chain kernels of mlp.hip fill the CU's LDS with their weight image (155-159 of 160 KiB; three more 64 x 64
// layers do not fit) and their machine code is pinned (profiles/mlp_static_isa_identity.txt).  The three heads hang off
// hidden = W0 x + b0 like every other head, so what they add to dL/dfeatures, dL/dW0 and dL/db0 is a separate SUM TERM: this family
// recomputes `hidden` from the features (one more read of [P,128] and one more 64 x 128 GEMM per direction) and returns its own
// terms; the caller's autograd adds them to those of s3g_deform_mlp_backward.
//   geom_pack_kernel       the fp32 [in][out+1] LDS image: two W0 slabs, three 64 x 64 slabs, three second-layer slabs (3 / 4 / 1 live
//                          rows of 32), seven bias vectors = 114 KiB
//   geom_forward_kernel    the scheme of mlp_forward_kernel: persistent workgroups, the whole image in LDS (one DMA burst), a wave owns a
//                          32-point tile and its activations stay in the MFMA accumulators (gemm_reg, mlp_dev.hpp); hidden and the
//                          three first-layer activations are stashed with their ReLU masks as bit words when a backward follows
//   geom_backward_kernel   the per-point chain on the transposed reads of the same image -> g_features (written) and four gradient
//                          signals (the three first-layer pre-activations' and hidden's)
//   geom_wgrad_kernel      the up to eight weight-gradient GEMMs (K dimension = the points), one wave per GEMM, operands straight from
//                          HBM; every workgroup walks a FIXED tile sequence and stores its partial blocks
//   geom_wgrad_reduce_kernel  adds the partial blocks in workgroup order onto the caller's gradients: no float atomics anywhere, so
//                          every weight gradient is bit-identical from run to run
// Arithmetic: v_mfma_f32_32x32x2_f32, exact fp32 fma chains, in every S3G_MLP_ARITHMETIC mode (the bf16 x 3 split is not built here).
// A head whose output (forward) / upstream gradient (backward) pointer is NULL is skipped behind a wave-uniform branch; what a present
// head computes does not depend on which others are present.
#include "mlp_dev.hpp"

#include "../../include/s3g_mlp_geom.h"

namespace s3g {

constexpr int GHEADS = 3;                       // scales | rotations | opacity
constexpr int GSLAB2 = 9 * 256;                 // floats of a second-layer slab: [64 in][32 out + 1], padded to whole 1 KiB DMA rows
constexpr int GW1_OFF = 2 * SLAB;               // C1 | R1 | O1 behind the two W0 slabs
constexpr int GW2_OFF = 5 * SLAB;               // C2 | R2 | O2
constexpr int GBIAS_OFF = GW2_OFF + GHEADS * GSLAB2;   // b0 | cb1 | rb1 | ob1 | cb2 | rb2 | ob2, zero padded to 64 each (+ one unused row)
constexpr int GPACK_FLOATS = GBIAS_OFF + 8 * 64;
constexpr int GPLANES = 1 + GHEADS;             // stash planes / mask words / gradient signals: hidden | scales1 | rotations1 | opacity1
static_assert(GPACK_FLOATS % 256 == 0 && GPACK_FLOATS * 4 <= 160 * 1024, "whole 1 KiB DMA rows, inside the CU's LDS");
static_assert(64 * 33 <= GSLAB2 && 64 * 65 <= SLAB, "slabs hold their layers");

__host__ __device__ constexpr int head_rows(int k) { return k == 0 ? 3 : (k == 1 ? 4 : 1); }

// one workgroup per slab (0, 1: W0 halves; 2..4: first layers; 5..7: second layers) + one for the biases; `present` bit k = head k
__global__ void __launch_bounds__(256) geom_pack_kernel(const s3g_geom_params w, float* __restrict__ packed, int present) {
  const int k = blockIdx.x, tid = threadIdx.x;
  const float* W1[GHEADS] = {w.C1, w.R1, w.O1};
  const float* W2[GHEADS] = {w.C2, w.R2, w.O2};
  if (k == 8) {
    float* bl = packed + GBIAS_OFF;
    const float* src[7] = {w.b0, w.cb1, w.rb1, w.ob1, w.cb2, w.rb2, w.ob2};
    const int n[7] = {64, 64, 64, 64, 3, 4, 1};
    for (int e = tid; e < 8 * 64; e += 256) {
      const int v = e >> 6, head = v == 0 ? -1 : (v - 1) % GHEADS;
      const bool live = v < 7 && (head < 0 || ((present >> head) & 1)) && (e & 63) < n[v < 7 ? v : 0];
      bl[e] = live ? src[v][e & 63] : 0.f;
    }
    return;
  }
  if (k >= 2 && !((present >> ((k - 2) % GHEADS)) & 1)) return;   // an absent head: its slabs are never read (its pointers may be NULL)
  if (k < 5) {
    float* dst = packed + (size_t)k * SLAB;
    const float* W = k <= 1 ? w.W0 : W1[k - 2];
    const int in = k <= 1 ? FEAT : HID, in0 = k == 1 ? 64 : 0;
    for (int e = tid; e < SLAB; e += 256) dst[e] = 0.f;
    __syncthreads();
    for (int e = tid; e < 64 * 64; e += 256) {
      const int o = e / 64, i = e % 64;
      dst[i * 65 + o] = W[(size_t)o * in + in0 + i];
    }
  } else {
    float* dst = packed + GW2_OFF + (size_t)(k - 5) * GSLAB2;
    const float* W = W2[k - 5];
    const int out = head_rows(k - 5);
    for (int e = tid; e < GSLAB2; e += 256) dst[e] = 0.f;
    __syncthreads();
    for (int e = tid; e < out * 64; e += 256) {
      const int o = e / 64, i = e % 64;
      dst[i * 33 + o] = W[(size_t)o * HID + i];
    }
  }
}

#define GW0(half) (lds + (half) * SLAB)
#define GW1(k) (lds + GW1_OFF + (k) * SLAB)
#define GW2(k) (lds + GW2_OFF + (k) * GSLAB2)
#define GBIAS(v) (lds + GBIAS_OFF + (v) * 64)

// whole image global -> LDS through the DMA path, once per workgroup (load_weights' pattern on this family's image)
__device__ __forceinline__ void geom_load_weights(float* lds, const float* __restrict__ packed, int wave, int lane) {
  for (int c = wave; c < GPACK_FLOATS / 256; c += NWAVE)
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(packed + c * 256 + lane * 4),
                                     (__attribute__((address_space(3))) void*)(lds + c * 256), 16, 0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

struct GHeadsFwdArgs {
  int P;
  const float* x;
  const float* packed;
  float* out[GHEADS];    // ds [P,3] | dr [P,4] | dopac [P,1]; NULL = head skipped
  float* stash;          // [GPLANES][P][64] (NULL when no backward follows)
  uint32_t* maskbits;    // [tiles][GPLANES][64] ReLU mask words
};

// head K of one tile: out = W2 relu(W1 relu(hidden) + b1) + b2; rows 0 .. N-1 of the 32-row output block are registers 0 .. N-1 of
// the lanes 0 .. 31 (accumulator layout: row = rrow(r) + 4 * (lane >> 5))
template <int K>
__device__ __forceinline__ void geom_head_forward(const float* lds, const GHeadsFwdArgs& a, const f32x16 (&hid)[2], uint32_t* mw, size_t PS,
                                                  int p0, int npts, int lane) {
  constexpr int N = head_rows(K);
  f32x16 act[2], o[1];
  acc_bias<2>(act, GBIAS(1 + K), lane);
  gemm_reg<2, 2, true>(GW1(K), 65, hid, act, lane);
  relu_inplace<2>(act);
  if (a.stash) act_store<HID, 2, false>(act, a.stash + (1 + K) * PS, 0, p0, npts, lane);
  if (mw) mw[(1 + K) * 64] = pack_positive<2>(act);
  acc_bias<1>(o, GBIAS(4 + K), lane);
  gemm_reg<1, 2, false>(GW2(K), 33, act, o, lane);
  if (lane < npts) {
    float* row = a.out[K] + (size_t)(p0 + lane) * N;
#pragma unroll
    for (int k = 0; k < N; k++) row[k] = o[0][k];
  }
}

__global__ void __launch_bounds__(NWAVE * 64) geom_forward_kernel(const GHeadsFwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  geom_load_weights(lds, a.packed, wave, lane);
  const int ntiles = (a.P + MT - 1) / MT;
  const size_t PS = (size_t)a.P * HID;
  // the 128 input features of the NEXT tile are requested before this tile's MFMAs are issued (clamped row: lanes past the end of
  // the array re-read the last point, whose outputs are never stored)
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
    f32x16 hid[2];
    {  // hidden = W0 x + b0, K = 128 in two halves
      f32x16 x[2];
      acc_bias<2>(hid, GBIAS(0), lane);
      unpack(x, cur, 0);
      gemm_reg<2, 2, false>(GW0(0), 65, x, hid, lane);
      unpack(x, cur, 1);
      gemm_reg<2, 2, false>(GW0(1), 65, x, hid, lane);
    }
    uint32_t* mw = a.maskbits ? a.maskbits + (size_t)tile * GPLANES * 64 + lane : nullptr;
    if (a.stash) act_store<HID, 2, false>(hid, a.stash + 0 * PS, 0, p0, npts, lane);
    if (mw) mw[0] = pack_positive<2>(hid);
    if (a.out[0] != nullptr) geom_head_forward<0>(lds, a, hid, mw, PS, p0, npts, lane);
    if (a.out[1] != nullptr) geom_head_forward<1>(lds, a, hid, mw, PS, p0, npts, lane);
    if (a.out[2] != nullptr) geom_head_forward<2>(lds, a, hid, mw, PS, p0, npts, lane);
    __builtin_amdgcn_sched_barrier(0);
    cur = nxt;   // copies at the very end: the prefetch has had the whole tile to land
  }
}

struct GHeadsBwdArgs {
  int P;
  const float* packed;
  const uint32_t* maskbits;    // [tiles][GPLANES][64] from the forward
  const float* g[GHEADS];      // g_ds | g_dr | g_do; NULL = head absent
  float *g_x, *ws;             // ws: [GPLANES][P][64] gradient signals: ghid | scales1 | rotations1 | opacity1
};
struct GHeadsBwdIn {             // everything one tile's chain reads from memory, requested a tile ahead
  float g[GHEADS][4];
  uint32_t bits[GPLANES];
};

// head K of one tile: signal = relu'(act1) . W2^T g_out (stored for the weight gradients), acc += W1^T signal
template <int K>
__device__ __forceinline__ void geom_head_backward(const float* lds, const GHeadsBwdArgs& a, const GHeadsBwdIn& in, f32x16 (&acc)[2], size_t PS,
                                                   int p0, int npts, int lane) {
  constexpr int N = head_rows(K);
  f32x16 g3[1], t[2], g[2];
  acc_zero<1>(g3);
#pragma unroll
  for (int k = 0; k < N; k++) g3[0][k] = (lane >> 5) == 0 ? in.g[K][k] : 0.f;   // output rows 0 .. N-1 live in registers 0 .. N-1 of the h = 0 lanes
  acc_zero<2>(t);
  gemm_reg_t<2, 1, 4>(GW2(K), 33, g3, t, lane);       // W2^T g_out: four K steps cover the <= 4 live rows (columns >= N of the slab are zero)
  masked_bits<2, false>(g, t, in.bits[1 + K]);
  act_store<HID, 2, false>(g, a.ws + (1 + K) * PS, 0, p0, npts, lane);
  gemm_reg_t<2, 2>(GW1(K), 65, g, acc, lane);         // + W1^T signal (masked by relu'(hidden) once, after the last head)
}

__global__ void __launch_bounds__(NWAVE * 64) geom_backward_kernel(const GHeadsBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  geom_load_weights(lds, a.packed, wave, lane);
  const int ntiles = (a.P + MT - 1) / MT;
  const size_t PS = (size_t)a.P * HID;
  const int j = lane & 31;
  // clamped addresses: lanes past the end of the array re-read the last point, whose columns are never stored
  auto issue = [&](GHeadsBwdIn& I, int tile) {
    const size_t p = (size_t)min(tile * MT + j, a.P - 1);
    const uint32_t* mw = a.maskbits + (size_t)tile * GPLANES * 64 + lane;
    I.bits[0] = mw[0];
#pragma unroll
    for (int k = 0; k < GHEADS; k++) {
      const bool on = a.g[k] != nullptr;
      I.bits[1 + k] = on ? mw[(1 + k) * 64] : 0u;
#pragma unroll
      for (int c = 0; c < 4; c++) I.g[k][c] = (on && c < head_rows(k)) ? a.g[k][p * head_rows(k) + c] : 0.f;
    }
  };
  const int stride = gridDim.x * NWAVE, t0 = blockIdx.x * NWAVE + wave;
  GHeadsBwdIn cur, nxt;
  if (t0 < ntiles) issue(cur, t0);
  for (int tile = t0; tile < ntiles; tile += stride) {
    issue(nxt, min(tile + stride, ntiles - 1));
    __builtin_amdgcn_sched_barrier(0);
    const int p0 = tile * MT, npts = min(MT, a.P - p0);
    f32x16 ghid[2], acc[2];
    acc_zero<2>(acc);
    if (a.g[0] != nullptr) geom_head_backward<0>(lds, a, cur, acc, PS, p0, npts, lane);
    if (a.g[1] != nullptr) geom_head_backward<1>(lds, a, cur, acc, PS, p0, npts, lane);
    if (a.g[2] != nullptr) geom_head_backward<2>(lds, a, cur, acc, PS, p0, npts, lane);
    masked_bits<2, false>(ghid, acc, cur.bits[0]);     // every head reads relu(hidden): one mask for the sum
    act_store<HID, 2, false>(ghid, a.ws + 0 * PS, 0, p0, npts, lane);
    // ---- feature_out: g_x[:, half] = W0[:, half]^T ghid ----
    acc_zero<2>(acc);
    gemm_reg_t<2, 2>(GW0(0), 65, ghid, acc, lane);
    act_store<FEAT, 2, false>(acc, a.g_x, 0, p0, npts, lane);
    acc_zero<2>(acc);
    gemm_reg_t<2, 2>(GW0(1), 65, ghid, acc, lane);
    act_store<FEAT, 2, false>(acc, a.g_x, 64, p0, npts, lane);
    __builtin_amdgcn_sched_barrier(0);
    cur = nxt;
  }
}
#undef GW0
#undef GW1
#undef GW2
#undef GBIAS

// ---- weight gradients:  dW[o][i] += sum_p G[p][o] * A[p][i];  db[o] += sum_p G[p][o] --------------------------------------------------
// One wave per GEMM ("job"), every wave of a workgroup on the same tile sequence blockIdx.x, blockIdx.x + gridDim.x, ...: which
// workgroup adds which points, and in which order, depends on P alone.  At K step s lane (i, k) supplies point p0 + 2s + k: G column
// 32m + i as the A operand (rows of dW), A column 32n + i as the B operand (columns of dW); consecutive lanes read consecutive floats.
// The second layers have 3, 4 and 1 rows: they are the same job with ONE 32-row block (MB = 1) and the columns >= gw read as zero.
struct GJob {
  const float* G;   // [P][gstride], gw columns used
  const float* A;   // [P][astride], 64 columns used
  float* dW;        // [gw][astride] window
  float* db;        // [gw] or NULL
  int gstride, gw, astride;
  float relu_lo;    // 0: A goes through a ReLU first (the stash holds the raw hidden); -inf: as it is
};
constexpr int GMAX_JOBS = 2 + 2 * GHEADS, GMAX_BLOCKS = 256;
// one job's partial block: its gw x 64 window (64 columns per row) + the bias sums as (high, low) float pairs.  A bias gradient is the
// plain sum of up to millions of signed terms -- the one quantity here whose result can be orders of magnitude below its terms -- so
// it is carried in float64 from the first addition to the last and rounded to fp32 once
constexpr int GPART = 64 * 64 + 2 * 64, GPART_BIAS = 64 * 64, GPART_BIAS_LO = GPART_BIAS + 64;
struct GWArgs {
  GJob job[GMAX_JOBS];
  int P, njobs;
  float* part;      // [gridDim.x][njobs][GPART]
};

template <int MB>
__device__ __forceinline__ void geom_wgrad_wave(const GJob& jb, int P, int lane, float* __restrict__ part) {
  constexpr int STEPS = MT / 2;
  const int i = lane & 31, k = lane >> 5;
  f32x16 acc[MB][2];
  double bsum[MB];
#pragma unroll
  for (int m = 0; m < MB; m++) {
    bsum[m] = 0.0;
#pragma unroll
    for (int n = 0; n < 2; n++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[m][n][r] = 0.f;
  }
  // Software pipeline, the one of mlp_wgrad.hip: the operand rows of the NEXT tile are requested (raw loads, clamped addresses, no
  // select on a loaded value) before the MFMAs of the current tile are issued, in two alternating register sets; sched_barrier(0)
  // keeps the scheduler from sinking the loads back to their uses.  Which tiles a workgroup adds, and in which order, is untouched.
  struct Set {
    float g[STEPS][MB], v[STEPS][2];
  };
  const int ntiles = (P + MT - 1) / MT, stride = gridDim.x, t0 = blockIdx.x, last = ntiles - 1;
  auto issue = [&](Set& S, int tile) {
    const int p0 = tile * MT;
#pragma unroll
    for (int s = 0; s < STEPS; s++) {
      const size_t pc = (size_t)min(p0 + 2 * s + k, P - 1);
#pragma unroll
      for (int m = 0; m < MB; m++) S.g[s][m] = jb.G[pc * jb.gstride + min(32 * m + i, jb.gw - 1)];
#pragma unroll
      for (int n = 0; n < 2; n++) S.v[s][n] = jb.A[pc * jb.astride + 32 * n + i];
    }
  };
  auto consume = [&](const Set& S, int tile) {   // points past the array's end and columns past the job's last read as zero
    const int p0 = tile * MT;
#pragma unroll
    for (int s = 0; s < STEPS; s++) {
      const bool live = p0 + 2 * s + k < P;
      float b[2];
#pragma unroll
      for (int n = 0; n < 2; n++) b[n] = live ? fmaxf(S.v[s][n], jb.relu_lo) : 0.f;
#pragma unroll
      for (int m = 0; m < MB; m++) {
        const float ga = (live && 32 * m + i < jb.gw) ? S.g[s][m] : 0.f;
        bsum[m] += (double)ga;
#pragma unroll
        for (int n = 0; n < 2; n++) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(ga, b[n], acc[m][n], 0, 0, 0);
      }
    }
  };
  {
    Set SA, SB;
    const int cnt = t0 < ntiles ? (ntiles - t0 + stride - 1) / stride : 0;
    if (cnt > 0) {
      issue(SA, t0);
      for (int it = 0; it < cnt; it += 2) {
        issue(SB, min(t0 + (it + 1) * stride, last));    // unconditional (clamped): one wasted prefetch per wave at the end
        __builtin_amdgcn_sched_barrier(0);
        consume(SA, t0 + it * stride);
        __builtin_amdgcn_sched_barrier(0);
        if (it + 1 >= cnt) break;
        issue(SA, min(t0 + (it + 2) * stride, last));
        __builtin_amdgcn_sched_barrier(0);
        consume(SB, t0 + (it + 1) * stride);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  // accumulator register r of lane l = dW[32m + rrow(r) + 4 (l >> 5)][32n + (l & 31)]: 32 consecutive floats per register and half
#pragma unroll
  for (int m = 0; m < MB; m++) {
#pragma unroll
    for (int n = 0; n < 2; n++)
#pragma unroll
      for (int r = 0; r < 16; r++) part[(32 * m + acc_row(r, lane)) * 64 + 32 * n + i] = acc[m][n][r];
    const double tot = bsum[m] + __shfl_xor(bsum[m], 32);   // the two K parities of the wave, even points first
    if (k == 0) {
      const float hi = (float)tot;
      part[GPART_BIAS + 32 * m + i] = hi;
      part[GPART_BIAS_LO + 32 * m + i] = (float)(tot - (double)hi);
    }
  }
}

__global__ void __launch_bounds__(GMAX_JOBS * 64) geom_wgrad_kernel(const GWArgs a) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const GJob jb = a.job[wave];
  float* part = a.part + ((size_t)blockIdx.x * a.njobs + wave) * GPART;
  if (jb.gw > 32) geom_wgrad_wave<2>(jb, a.P, lane, part);
  else geom_wgrad_wave<1>(jb, a.P, lane, part);
}

// grid = (element chunks, jobs): one thread per gradient element adds the nb workgroups' partials of it in workgroup order
// 0 .. nb-1 -- one fixed association of the addends -- onto dW / db (which the caller zero-filled, or which hold a sum)
__global__ void __launch_bounds__(256) geom_wgrad_reduce_kernel(const GWArgs a, int nb) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const GJob jb = a.job[blockIdx.y];
  float* dst = nullptr;
  if (e < jb.gw * 64) dst = jb.dW + (size_t)(e >> 6) * jb.astride + (e & 63);
  else if (e >= GPART_BIAS && e < GPART_BIAS + jb.gw && jb.db != nullptr) dst = jb.db + (e - GPART_BIAS);
  if (dst == nullptr) return;
  const size_t stride = (size_t)a.njobs * GPART;
  const float* src = a.part + (size_t)blockIdx.y * GPART + e;
  if (e >= GPART_BIAS) {   // a bias sum: (high, low) pairs added in float64, in workgroup order
    double t = 0.0;
    for (int b = 0; b < nb; b++) t += (double)src[(size_t)b * stride] + (double)src[(size_t)b * stride + 64];
    *dst = (float)((double)*dst + t);
    return;
  }
  float s = 0.f;
  int b = 0;
  for (; b + 8 <= nb; b += 8) {   // eight independent loads in flight, added in order
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) v[u] = src[(size_t)(b + u) * stride];
#pragma unroll
    for (int u = 0; u < 8; u++) s += v[u];
  }
  for (; b < nb; b++) s += src[(size_t)b * stride];
  *dst += s;
}

static size_t geom_mask_words(int P) { return (size_t)((P > 0 ? P : 0) + MT - 1) / MT * GPLANES * 64; }
static size_t geom_planes(int P) { return (size_t)GPLANES * (size_t)(P > 0 ? P : 0) * HID; }

static int geom_set_attrs() {
  static std::atomic<uint64_t> done{0};
  if (device_needs_setup(done)) {
    S3G_HIP_CHECK(hipFuncSetAttribute((const void*)geom_forward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, GPACK_FLOATS * 4));
    S3G_HIP_CHECK(hipFuncSetAttribute((const void*)geom_backward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, GPACK_FLOATS * 4));
    device_setup_done(done);
  }
  return S3G_OK;
}

// the head's four tensors are there (weights, or gradient slots)
static bool geom_head_complete(const s3g_geom_params* w, int k) {
  return k == 0 ? (w->C1 && w->cb1 && w->C2 && w->cb2) : k == 1 ? (w->R1 && w->rb1 && w->R2 && w->rb2) : (w->O1 && w->ob1 && w->O2 && w->ob2);
}

}  // namespace s3g

using namespace s3g;

// stash = [weight image (GPACK_FLOATS)] [4 x P x 64 activations] [tiles x 4 x 64 ReLU mask words]
extern "C" size_t s3g_deform_geom_stash_bytes(int P) { return ((size_t)GPACK_FLOATS + geom_planes(P) + geom_mask_words(P)) * sizeof(float); }
// workspace = [4 x P x 64 gradient signals] [256 x 8 partial blocks of the weight gradients]
extern "C" size_t s3g_deform_geom_workspace_bytes(int P) {
  return (geom_planes(P) + (size_t)GMAX_BLOCKS * GMAX_JOBS * GPART) * sizeof(float);
}

extern "C" int s3g_deform_geom_forward(const s3g_geom_params* w, int P, const float* features, float* ds, float* dr, float* dopac,
                                       float* stash, int save_activations, void* stream_) {
  float* out[GHEADS] = {ds, dr, dopac};
  bool ok = w && P >= 0 && (ds || dr || dopac) && w->W0 && w->b0;
  for (int k = 0; ok && k < GHEADS; k++) ok = !out[k] || geom_head_complete(w, k);
  if (!ok || (P > 0 && (!features || !stash))) {
    set_error("s3g_deform_geom_forward: bad argument (NULL weights of a requested head, no head requested, or a NULL buffer)");
    return S3G_ERR_INVALID_ARG;
  }
  if (P == 0) return S3G_OK;
  if (int e = geom_set_attrs()) return e;
  hipStream_t stream = (hipStream_t)stream_;
  int present = 0;
  GHeadsFwdArgs a;
  a.P = P; a.x = features; a.packed = stash;
  for (int k = 0; k < GHEADS; k++) { a.out[k] = out[k]; present |= (out[k] ? 1 : 0) << k; }
  a.stash = save_activations ? stash + GPACK_FLOATS : nullptr;
  a.maskbits = save_activations ? reinterpret_cast<uint32_t*>(stash + GPACK_FLOATS + geom_planes(P)) : nullptr;
  const int ntiles = (P + MT - 1) / MT;
  const int blocks = min((ntiles + NWAVE - 1) / NWAVE, 256);
  hipLaunchKernelGGL(geom_pack_kernel, dim3(9), dim3(256), 0, stream, *w, stash, present);
  hipLaunchKernelGGL(geom_forward_kernel, dim3(blocks), dim3(NWAVE * 64), GPACK_FLOATS * 4, stream, a);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" int s3g_deform_geom_backward(const s3g_geom_params* w, int P, const float* features, const float* stash_, const float* g_ds,
                                        const float* g_dr, const float* g_do, float* g_features, const s3g_geom_params* gw,
                                        float* workspace, void* stream_) {
  const float* g[GHEADS] = {g_ds, g_dr, g_do};
  bool ok = w && gw && P >= 0 && (g_ds || g_dr || g_do) && gw->W0 && gw->b0;
  for (int k = 0; ok && k < GHEADS; k++) ok = !g[k] || geom_head_complete(gw, k);
  if (!ok || (P > 0 && (!features || !stash_ || !g_features || !workspace))) {
    set_error("s3g_deform_geom_backward: bad argument (NULL gradient slots of a present head, no head present, or a NULL buffer)");
    return S3G_ERR_INVALID_ARG;
  }
  if (P == 0) return S3G_OK;
  if (int e = geom_set_attrs()) return e;
  hipStream_t stream = (hipStream_t)stream_;
  const size_t PS = (size_t)P * HID;
  const float* stash = stash_ + GPACK_FLOATS;   // activations; the forward's weight image sits in front
  GHeadsBwdArgs b;
  b.P = P; b.packed = stash_; b.maskbits = reinterpret_cast<const uint32_t*>(stash + geom_planes(P));
  for (int k = 0; k < GHEADS; k++) b.g[k] = g[k];
  b.g_x = g_features; b.ws = workspace;
  const int ntiles = (P + MT - 1) / MT;
  const int blocks = min((ntiles + NWAVE - 1) / NWAVE, 256);
  hipLaunchKernelGGL(geom_backward_kernel, dim3(blocks), dim3(NWAVE * 64), GPACK_FLOATS * 4, stream, b);
  S3G_HIP_CHECK(hipGetLastError());
  // ---- weight gradients: feature_out's two K halves share ghid; a head's two layers follow ----
  const float NONE = -__builtin_huge_valf(), RELU = 0.f;
  GWArgs wa;
  memset(&wa, 0, sizeof wa);
  int nj = 0;
  wa.job[nj++] = GJob{workspace + 0 * PS, features, gw->W0, gw->b0, HID, HID, FEAT, NONE};
  wa.job[nj++] = GJob{workspace + 0 * PS, features + 64, gw->W0 + 64, nullptr, HID, HID, FEAT, NONE};
  float* dW1[GHEADS] = {gw->C1, gw->R1, gw->O1};
  float* db1[GHEADS] = {gw->cb1, gw->rb1, gw->ob1};
  float* dW2[GHEADS] = {gw->C2, gw->R2, gw->O2};
  float* db2[GHEADS] = {gw->cb2, gw->rb2, gw->ob2};
  for (int k = 0; k < GHEADS; k++) {
    if (!g[k]) continue;
    wa.job[nj++] = GJob{workspace + (1 + k) * PS, stash + 0 * PS, dW1[k], db1[k], HID, HID, HID, RELU};
    wa.job[nj++] = GJob{g[k], stash + (1 + k) * PS, dW2[k], db2[k], head_rows(k), head_rows(k), HID, NONE};
  }
  wa.P = P; wa.njobs = nj;
  wa.part = workspace + geom_planes(P);
  const int wblocks = min(ntiles, GMAX_BLOCKS);
  hipLaunchKernelGGL(geom_wgrad_kernel, dim3(wblocks), dim3(nj * 64), 0, stream, wa);
  hipLaunchKernelGGL(geom_wgrad_reduce_kernel, dim3((GPART + 255) / 256, nj), dim3(256), 0, stream, wa, wblocks);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}
