// Device helpers shared by the kernel families of the deformation MLP, and the host functions that cross their files:
//   mlp.hip           the per-point chain kernels (forward / backward, exact fp32 and bf16 x 3) and their weight-image pack kernels
//   mlp_heads.hip     the per-point chain kernels without the SH head (exact fp32)
//   mlp_wgrad.hip     the weight-gradient kernels (K dimension = the points)
//   deform_infer.hip  the fused HexPlane sampler (+) MLP inference kernel
// Here: the tile constants, the accumulator-layout helpers of v_mfma_f32_32x32x2_f32 (activations stay in the accumulator registers
// from layer to layer: gemm_reg), the three-way bf16 operand split (split_pair .. gemm_fw / gemm_bw, gemm_split), and the fp32
// [in][out+1] weight image with its DMA load.  The pre-split image layouts live with the kernels that read them.
// Private to libs3g.so (not part of the C ABI).
#pragma once
#include "common.hpp"

#include "../../include/s3g_mlp.h"

namespace s3g {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int MT = 32;    // points per wave tile (MFMA N)
constexpr int HID = 64;   // net_width
constexpr int FEAT = 128; // HexPlane feature width

// Accumulator layout of v_mfma_f32_32x32x2_f32: register r of lane l holds (row, col) = (rrow(r) + 4 * (l >> 5), l & 31)
// with rrow(r) = (r & 3) + 8 * (r >> 2).  Rows are output features, columns the 32 points of the tile.
__device__ __forceinline__ constexpr int rrow(int r) { return (r & 3) + 8 * (r >> 2); }
__device__ __forceinline__ int acc_row(int reg, int lane) { return rrow(reg) + 4 * (lane >> 5); }

// The trick that keeps activations out of LDS: the MFMA's K index is a summation index, so its order is free.  At K step
// (mbi, r) lane l supplies as B operand its OWN accumulator register in[mbi][r] -- that is feature
// f = 32*mbi + rrow(r) + 4*(l>>5) of point l&31 -- and the A operand is read from the weight image at that same f.
// A layer's output registers are therefore directly the next layer's input operand: no transposition, no LDS round
// trip, no barrier; waves run independently.
//   straight:   acc[mbo] += W[32*mbo + i][f] * in[f]      A = wl[f * ld + 32*mbo + i]     (wl = [in][out+1] image)
template <int MBO, int MBI, bool RELU_IN, int RSTEPS = 16>
__device__ __forceinline__ void gemm_reg(const float* wl, int ld, const f32x16 (&in)[MBI], f32x16 (&acc)[MBO], int lane) {
  const float* base = wl + 4 * (lane >> 5) * ld + (lane & 31);
#pragma unroll
  for (int mbi = 0; mbi < MBI; mbi++)
#pragma unroll
    for (int r = 0; r < RSTEPS; r++) {
      float b = in[mbi][r];
      if (RELU_IN) b = fmaxf(b, 0.f);
#pragma unroll
      for (int mbo = 0; mbo < MBO; mbo++)
        acc[mbo] = __builtin_amdgcn_mfma_f32_32x32x2f32(base[(32 * mbi + rrow(r)) * ld + 32 * mbo], b, acc[mbo], 0, 0, 0);
    }
}
//   transposed: acc[mbo] += W[f][32*mbo + i] * g[f]       A = wl[(32*mbo + i) * ld + f]   (f runs over OUTPUT features)
template <int MBO, int MBI, int RSTEPS = 16>
__device__ __forceinline__ void gemm_reg_t(const float* wl, int ld, const f32x16 (&g)[MBI], f32x16 (&acc)[MBO], int lane) {
  const float* base = wl + (lane & 31) * ld + 4 * (lane >> 5);
#pragma unroll
  for (int mbi = 0; mbi < MBI; mbi++)
#pragma unroll
    for (int r = 0; r < RSTEPS; r++) {
#pragma unroll
      for (int mbo = 0; mbo < MBO; mbo++)
        acc[mbo] = __builtin_amdgcn_mfma_f32_32x32x2f32(base[32 * mbo * ld + 32 * mbi + rrow(r)], g[mbi][r], acc[mbo], 0, 0, 0);
    }
}

// The two 3-row heads (pos_deform / dino_head output layers, 64 -> 3) on v_mfma_f32_4x4x1_16B_f32 (round 5).  A 32x32x2 MFMA spends
// a full 32-row block (64 cycles per K step) on three live rows: 2 x 32 of the forward's 512 MFMA slots per tile.  The 4x4x1
// instruction is sixteen independent 4x4 outer products (8 cycles): block b = lanes 4b .. 4b+3; lane 4b+j supplies B[j] and receives
// column j of the block in four registers, lane 4b+i supplies A[i].  It fits the register-resident scheme without moving anything:
//   B = the lane's OWN activation register in[mbi][r] -- feature f = 32 mbi + rrow(r) + 4 (lane >> 5) of point lane & 31; the four
//       lanes of a block share f (blocks do not straddle lane 32) and hold four different points;
//   A = W[lane & 3][f] from the [in][out + 1] weight image (rows 3 .. 31 of a head slab are zero, so i = 3 contributes nothing);
//   D = in lane l, registers 0 .. 2: rows 0 .. 2 of the output for point l & 31, summed over the features of the lane's half.
// The two halves (lanes l and l + 32 hold the K steps of features 4h .. 4h + 3 mod 8) meet in one cross-half add.  Summation
// order differs from the 32x32x2 chain (two half-K chains per mbi, added at the end): the training forward and the inference kernel
// use THIS function both, so they stay bit-identical to each other (tests/test_infer_gpu.py).
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void head3_fw(const float* wl /* [64 in][33] head slab */, const float* bias /* LDS, >= 3 floats */,
                                         const f32x16 (&in)[2], float (&o)[3], int lane) {
  const int h = lane >> 5;
  const float* base = wl + 4 * h * 33 + (lane & 3);
  f32x4 c0, c1;
  c0[0] = h == 0 ? bias[0] : 0.f; c0[1] = h == 0 ? bias[1] : 0.f; c0[2] = h == 0 ? bias[2] : 0.f; c0[3] = 0.f;
  c1[0] = c1[1] = c1[2] = c1[3] = 0.f;
#pragma unroll
  for (int r = 0; r < 16; r++) {      // two independent accumulation chains (mbi = 0 / 1): no MFMA waits for its predecessor's result
    c0 = __builtin_amdgcn_mfma_f32_4x4x1f32(base[rrow(r) * 33], in[0][r], c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_4x4x1f32(base[(32 + rrow(r)) * 33], in[1][r], c1, 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float v = c0[i] + c1[i];
    o[i] = v + __shfl_xor(v, 32);   // both halves end up with the total; the stores below use lanes 0 .. 31
  }
}
__device__ __forceinline__ void store3(const float (&o)[3], float* __restrict__ g, int p0, int npts, int lane) {
  if (lane < npts) {   // [P][3] rows, not 16-byte aligned
    float* row = g + (size_t)(p0 + lane) * 3;
    row[0] = o[0]; row[1] = o[1]; row[2] = o[2];
  }
}

template <int MB>
__device__ __forceinline__ void acc_zero(f32x16 (&acc)[MB]) {
#pragma unroll
  for (int mb = 0; mb < MB; mb++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[mb][r] = 0.f;
}
// acc = bias (LDS, zero padded to 64): 4 consecutive features per 16-byte read
template <int MB>
__device__ __forceinline__ void acc_bias(f32x16 (&acc)[MB], const float* bias, int lane) {
#pragma unroll
  for (int mb = 0; mb < MB; mb++)
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const float4 v = *reinterpret_cast<const float4*>(bias + 32 * mb + 8 * q + 4 * (lane >> 5));
      acc[mb][4 * q + 0] = v.x; acc[mb][4 * q + 1] = v.y; acc[mb][4 * q + 2] = v.z; acc[mb][4 * q + 3] = v.w;
    }
}
// Registers <-> a [P][WIDTH] global array, columns col0 .. col0 + 32*MB of it: lane (point j, half h) moves the four
// consecutive features 32*mb + 8*q + 4*h .. +3 as one 16-byte access (features >= VALID are zero / not stored).
template <int WIDTH, int MB, int VALID = 32 * MB>
__device__ __forceinline__ void act_load(f32x16 (&a)[MB], const float* __restrict__ g, int col0, int p0, int npts, int lane) {
  const int j = lane & 31, h = lane >> 5;
  const float* row = g + (size_t)(p0 + j) * WIDTH + col0 + 4 * h;
#pragma unroll
  for (int mb = 0; mb < MB; mb++)
#pragma unroll
    for (int q = 0; q < 4; q++) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (32 * mb + 8 * q < VALID && 32 * mb + 8 * q + 4 * h < VALID && j < npts)
        v = *reinterpret_cast<const float4*>(row + 32 * mb + 8 * q);
      a[mb][4 * q + 0] = v.x; a[mb][4 * q + 1] = v.y; a[mb][4 * q + 2] = v.z; a[mb][4 * q + 3] = v.w;
    }
}
template <int WIDTH, int MB, bool RELU, int VALID = 32 * MB>
__device__ __forceinline__ void act_store(const f32x16 (&a)[MB], float* __restrict__ g, int col0, int p0, int npts, int lane) {
  const int j = lane & 31, h = lane >> 5;
  float* row = g + (size_t)(p0 + j) * WIDTH + col0 + 4 * h;
#pragma unroll
  for (int mb = 0; mb < MB; mb++)
#pragma unroll
    for (int q = 0; q < 4; q++) {
      if (32 * mb + 8 * q >= VALID) continue;
      float4 v = make_float4(a[mb][4 * q + 0], a[mb][4 * q + 1], a[mb][4 * q + 2], a[mb][4 * q + 3]);
      if (RELU) v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
      if (32 * mb + 8 * q + 4 * h < VALID && j < npts) *reinterpret_cast<float4*>(row + 32 * mb + 8 * q) = v;
    }
}
// 3-wide heads ([P][3], not 16-byte aligned): features 0..2 sit in registers 0..2 of the h = 0 lanes
__device__ __forceinline__ void act_load3(f32x16 (&a)[1], const float* __restrict__ g, int p0, int npts, int lane) {
  acc_zero<1>(a);
  if (lane < npts) {
    const float* row = g + (size_t)(p0 + lane) * 3;
    a[0][0] = row[0]; a[0][1] = row[1]; a[0][2] = row[2];
  }
}
__device__ __forceinline__ void act_store3(const f32x16 (&a)[1], float* __restrict__ g, int p0, int npts, int lane) {
  if (lane < npts) {
    float* row = g + (size_t)(p0 + lane) * 3;
    row[0] = a[0][0]; row[1] = a[0][1]; row[2] = a[0][2];
  }
}
template <int MB>
__device__ __forceinline__ void relu_inplace(f32x16 (&a)[MB]) {
#pragma unroll
  for (int mb = 0; mb < MB; mb++)
#pragma unroll
    for (int r = 0; r < 16; r++) a[mb][r] = fmaxf(a[mb][r], 0.f);
}
// dst (op)= acc where mask > 0
template <int MB, bool ACCUM>
__device__ __forceinline__ void masked(f32x16 (&dst)[MB], const f32x16 (&acc)[MB], const f32x16 (&mask)[MB]) {
#pragma unroll
  for (int mb = 0; mb < MB; mb++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const float v = mask[mb][r] > 0.f ? acc[mb][r] : 0.f;
      dst[mb][r] = ACCUM ? dst[mb][r] + v : v;
    }
}

// ReLU masks as bits: bit (16*mb + r) of a lane's word = (a[mb][r] > 0).  The backward chain needs the forward activations
// only as ReLU masks; reading them as one 32-bit word per lane and plane (8 B per point and plane) instead of the fp32
// activation planes (256 B per point and plane) removes 1280 of the 3288 bytes per point the backward used to move AND every
// dependent load from its critical path (the words of the next tile are prefetched a whole tile ahead).
template <int MB>
__device__ __forceinline__ uint32_t pack_positive(const f32x16 (&a)[MB]) {
  uint32_t b = 0;
#pragma unroll
  for (int mb = 0; mb < MB; mb++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      // x > 0  <=>  its bit pattern as a signed integer is >= 1 (negative floats and -0 are negative integers, +0 is 0):
      // med3(x, 0, 1) is the bit, one v_med3_i32 + one v_lshl_or_b32 per element
      const int bit = min(max(__float_as_int(a[mb][r]), 0), 1);
      b |= (uint32_t)bit << (16 * mb + r);
    }
  return b;
}
// dst (op)= acc where the mask bit is set
template <int MB, bool ACCUM>
__device__ __forceinline__ void masked_bits(f32x16 (&dst)[MB], const f32x16 (&acc)[MB], uint32_t bits) {
#pragma unroll
  for (int mb = 0; mb < MB; mb++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const float v = ((bits >> (16 * mb + r)) & 1u) ? acc[mb][r] : 0.f;
      dst[mb][r] = ACCUM ? dst[mb][r] + v : v;
    }
}

// ---- fp32 GEMMs on the bf16 matrix pipe: three-way operand split ------------------------------------------------------------------
// v_mfma_f32_32x32x2_f32 runs at the vector-fma rate (64 cycles per 4096 FLOP and SIMD); v_mfma_f32_32x32x16_bf16 does 32768
// FLOP in 32 cycles on the real matrix pipe, beside the VALU instead of in its place.  Every fp32 operand is written as the EXACT
// sum of three bf16 numbers (round to nearest, subtract, repeat: 8 + 8 + 8 significand bits), and a product a*b is accumulated
// as the six piece products whose weight is >= 2^-16 of it:
//     a*b ~= a0*b0 + (a0*b1 + a1*b0) + (a0*b2 + a1*b1 + a2*b0)          dropped: a1*b2 + a2*b1 + a2*b2 <= 2^-23 |a*b|
// Each piece product is exact in fp32 (8 x 8 bits) and the matrix pipe accumulates in fp32, so a dot product carries the error
// of an fp32 fma chain (rounding 2^-24 per step) plus <= 2^-23 per product: fp32 accuracy, 6 x 32 instead of 8 x 64 cycles per
// K = 16.  Used by deform_infer_kernel<UT, true> and by the S3G_MLP_BF16X3 training chains; the other kernels are the exact chains above.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t bf16_pair(float lo, float hi) {   // one v_cvt_pk_bf16_f32 (round to nearest even)
  const bf16x2 v = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(uint32_t, v);
}
__device__ __forceinline__ float bf16_lo(uint32_t p) { return __uint_as_float(p << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t p) { return __uint_as_float(p & 0xffff0000u); }
// (a, b) -> word t of the three pieces; a == lo(p0) + lo(p1) + lo(p2) exactly (the residuals are exact fp32 differences)
__device__ __forceinline__ void split_pair(float a, float b, uint32_t& p0, uint32_t& p1, uint32_t& p2) {
  p0 = bf16_pair(a, b);
  const float ra = a - bf16_lo(p0), rb = b - bf16_hi(p0);
  p1 = bf16_pair(ra, rb);
  p2 = bf16_pair(ra - bf16_lo(p1), rb - bf16_hi(p1));
}
struct Split8 { u32x4 p[3]; };   // eight values = one lane's share of an MFMA operand (K = 16: k = 8 * (lane >> 5) + e), three pieces
__device__ __forceinline__ Split8 split8(const float (&v)[8]) {
  Split8 s;
#pragma unroll
  for (int t = 0; t < 4; t++) {
    uint32_t p0, p1, p2;
    split_pair(v[2 * t], v[2 * t + 1], p0, p1, p2);
    s.p[0][t] = p0; s.p[1][t] = p1; s.p[2][t] = p2;
  }
  return s;
}
// acc += A * B for one K = 16 step, A and B given as pieces; smallest terms first
__device__ __forceinline__ f32x16 mfma_split(f32x16 acc, const Split8& a, const Split8& b) {
#define S3G_PIECE(i, j) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a.p[i]), __builtin_bit_cast(bf16x8, b.p[j]), acc, 0, 0, 0)
  S3G_PIECE(2, 0); S3G_PIECE(1, 1); S3G_PIECE(0, 2); S3G_PIECE(1, 0); S3G_PIECE(0, 1); S3G_PIECE(0, 0);
#undef S3G_PIECE
  return acc;
}
// The accumulator registers of a layer as the B operand of the next, exactly as in gemm_reg: at K step (mbi, s) lane l supplies
// its own registers in[mbi][8s .. 8s+7] = features 32*mbi + 16*s + 4*(l>>5) + {0,1,2,3, 8,9,10,11} of point l & 31, and the A
// operand holds the weights of those same features in the same element order (split_feature below is that order).
template <int MBI> struct ActSplit { Split8 b[MBI][2]; };
template <int MBI, bool RELU>
__device__ __forceinline__ void act_split(ActSplit<MBI>& S, const f32x16 (&in)[MBI]) {
#pragma unroll
  for (int mbi = 0; mbi < MBI; mbi++)
#pragma unroll
    for (int s = 0; s < 2; s++) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; e++) v[e] = RELU ? fmaxf(in[mbi][8 * s + e], 0.f) : in[mbi][8 * s + e];
      S.b[mbi][s] = split8(v);
    }
}
__host__ __device__ constexpr int split_feature(int ks, int h, int e) { return 16 * ks + 4 * h + (e & 3) + 8 * (e >> 2); }   // ks = 2 * mbi + s

// gemm_reg / gemm_reg_t with both operands split on the fly: the A operand is read from the SAME fp32 [in][out+1] LDS image (eight
// ds_read_b32 per fragment instead of one per fp32 MFMA: the same LDS traffic) and split by the lane that uses it.
template <int MBO, int MBI, bool RELU_IN, int RSTEPS = 16>
__device__ __forceinline__ void gemm_reg_split(const float* wl, int ld, const f32x16 (&in)[MBI], f32x16 (&acc)[MBO], int lane) {
  const float* base = wl + 4 * (lane >> 5) * ld + (lane & 31);
#pragma unroll
  for (int mbi = 0; mbi < MBI; mbi++)
#pragma unroll
    for (int s = 0; s < (RSTEPS + 7) / 8; s++) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; e++) v[e] = RELU_IN ? fmaxf(in[mbi][8 * s + e], 0.f) : in[mbi][8 * s + e];
      const Split8 b = split8(v);
#pragma unroll
      for (int mbo = 0; mbo < MBO; mbo++) {
        float w[8];
#pragma unroll
        for (int e = 0; e < 8; e++) w[e] = base[(32 * mbi + rrow(8 * s + e)) * ld + 32 * mbo];
        acc[mbo] = mfma_split(acc[mbo], split8(w), b);
      }
    }
}
template <int MBO, int MBI, int RSTEPS = 16>
__device__ __forceinline__ void gemm_reg_t_split(const float* wl, int ld, const f32x16 (&g)[MBI], f32x16 (&acc)[MBO], int lane) {
  const float* base = wl + (lane & 31) * ld + 4 * (lane >> 5);
#pragma unroll
  for (int mbi = 0; mbi < MBI; mbi++)
#pragma unroll
    for (int s = 0; s < (RSTEPS + 7) / 8; s++) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; e++) v[e] = g[mbi][8 * s + e];
      const Split8 b = split8(v);
#pragma unroll
      for (int mbo = 0; mbo < MBO; mbo++) {
        float w[8];
#pragma unroll
        for (int e = 0; e < 8; e++) w[e] = base[32 * mbo * ld + 32 * mbi + rrow(8 * s + e)];
        acc[mbo] = mfma_split(acc[mbo], split8(w), b);
      }
    }
}
// arithmetic selected at compile time by the kernels' SPLIT parameter
template <bool SPLIT, int MBO, int MBI, bool RELU_IN, int RSTEPS = 16>
__device__ __forceinline__ void gemm_fw(const float* wl, int ld, const f32x16 (&in)[MBI], f32x16 (&acc)[MBO], int lane) {
  if constexpr (SPLIT) gemm_reg_split<MBO, MBI, RELU_IN, RSTEPS>(wl, ld, in, acc, lane);
  else gemm_reg<MBO, MBI, RELU_IN, RSTEPS>(wl, ld, in, acc, lane);
}
template <bool SPLIT, int MBO, int MBI, int RSTEPS = 16>
__device__ __forceinline__ void gemm_bw(const float* wl, int ld, const f32x16 (&g)[MBI], f32x16 (&acc)[MBO], int lane) {
  if constexpr (SPLIT) gemm_reg_t_split<MBO, MBI, RSTEPS>(wl, ld, g, acc, lane);
  else gemm_reg_t<MBO, MBI, RSTEPS>(wl, ld, g, acc, lane);
}

// ---- pre-split weights: fragments ----------------------------------------------------------------------------------------------------
// A FRAGMENT is the A operand of one (32-row block mbo, K step ks) of a layer, split ONCE by a pack kernel: 64 lanes x 16 bytes per
// piece, stored piece after piece in lane order -- one conflict-free ds_read_b128 per piece and lane.  The images built from them
// (32-bit words; a word = two bf16) are laid out by the files that read them: spw (deform_infer.hip), tpw and tbw (mlp.hip).
constexpr int FRAG_WORDS = 256;   // words per piece of a full fragment

__device__ __forceinline__ uint32_t split_word(const float* __restrict__ W, int rows, int ld, int row, int f0, int f1, int piece) {
  uint32_t p[3];
  const float a = row < rows ? W[(size_t)row * ld + f0] : 0.f, b = row < rows ? W[(size_t)row * ld + f1] : 0.f;
  split_pair(a, b, p[0], p[1], p[2]);
  return piece == 0 ? p[0] : (piece == 1 ? p[1] : p[2]);
}
// acc[mbo] += (rows 32*mbo .. +31 of the layer) x B for the K steps ks0 .. ks0 + 2*MBI - 1, fragments at frag + ((mbo*KS + ks)*3 + piece)*FRAG_WORDS
template <int MBO, int MBI>
__device__ __forceinline__ void gemm_split(const uint32_t* frag, int KS, int ks0, const ActSplit<MBI>& B, f32x16 (&acc)[MBO], int lane) {
#pragma unroll
  for (int mbi = 0; mbi < MBI; mbi++)
#pragma unroll
    for (int s = 0; s < 2; s++) {
      Split8 a[MBO];
#pragma unroll
      for (int mbo = 0; mbo < MBO; mbo++)
#pragma unroll
        for (int pc = 0; pc < 3; pc++)
          a[mbo].p[pc] = *reinterpret_cast<const u32x4*>(frag + ((mbo * KS + ks0 + 2 * mbi + s) * 3 + pc) * FRAG_WORDS + lane * 4);
#pragma unroll
      for (int mbo = 0; mbo < MBO; mbo++) acc[mbo] = mfma_split(acc[mbo], a[mbo], B.b[mbi][s]);
    }
}

// ---- weight slabs: the LDS image is built once per call in global memory and DMA-copied by every workgroup ---------
// Slab k is the [in][out+1] image of one layer (feature_out is cut in two K halves), padded to SLAB floats = 17 KiB =
// 17 global_load_lds_dwordx4 wave-instructions (1 KiB each).
constexpr int SLAB = 17 * 256;  // floats
constexpr int NSLAB = 9;        // W0[:, :64] | W0[:, 64:] | P1 | S1 | P2 | S2 | D0 | D1 | D2
constexpr int PACK_FLOATS = NSLAB * SLAB + 8 * 64;  // + the 8 bias vectors zero padded to 64
constexpr int NWAVE = 8;  // waves per workgroup; one persistent workgroup per CU (the weights fill its LDS)
constexpr int MLP_LDS_FLOATS = PACK_FLOATS;

// Whole packed image (9 slabs + biases, 155 KB) global -> LDS through the DMA path, once per workgroup.
__device__ __forceinline__ void load_weights(float* lds, const float* __restrict__ packed, int wave, int lane) {
  static_assert(PACK_FLOATS % 256 == 0, "image is a whole number of 1 KiB DMA rows");
  for (int c = wave; c < PACK_FLOATS / 256; c += NWAVE)
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(packed + c * 256 + lane * 4),
                                     (__attribute__((address_space(3))) void*)(lds + c * 256), 16, 0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// ---- host functions that cross files (a __global__ function is launched only from the file that defines it) --------------------------
// mlp.hip: mlp_pack_kernel builds the fp32 image of `w` (PACK_FLOATS floats) in `packed`
void mlp_pack_launch(const s3g_mlp_params& w, float* packed, hipStream_t stream);
// mlp_wgrad.hip: all weight and bias gradients of one backward pass, added onto *gw.  `stash` = the forward's five activation planes,
// `signals` = the backward chain's five gradient planes ([5][P][64] each); g_feat == NULL: no dino head.  partials == NULL: float
// atomics; else the s3g_deform_mlp_wgrad_partial_bytes() buffer of the ordered (bit-reproducible) flush.
int mlp_wgrad_launch(int P, const float* features, const float* stash, const float* signals, const float* g_dx, const float* g_dshs,
                     const float* g_feat, const s3g_mlp_params* gw, float* partials, hipStream_t stream);
// mlp_heads.hip: the chain kernels without the SH head (dshs / g_dshs == NULL), exact fp32 in every arithmetic mode.  `packed` = the fp32
// image of mlp_pack_launch; `planes` / `maskbits` = the stash's five activation planes and its mask words (both NULL when no backward
// follows); dx / feat and g_dx / g_feat: either may be NULL, not both.
int mlp_nosh_forward_launch(int P, const float* features, const float* packed, float* dx, float* feat, float* planes, uint32_t* maskbits,
                            hipStream_t stream);
int mlp_nosh_backward_launch(int P, const float* packed, const uint32_t* maskbits, const float* g_dx, const float* g_feat, float* g_features,
                             float* workspace, hipStream_t stream);

}  // namespace s3g
