// Inference: HexPlane sampler (+) deformation MLP heads in ONE kernel (render(): gaussian_renderer/__init__.py:82-97).
// Under no_grad nothing is stashed and the feature (dino) head is not needed, so the weight image shrinks to the first six slabs
// (W0 | W0 | P1 | S1 | P2 | S2 = 104 KB) and 46 KB of LDS are left: each wave gets a 32-point x 32-channel staging tile and one
// level's tap slots.  A wave samples ONE LEVEL of its 32 points the way hexplane_forward_kernel does (8 lanes per point, four
// rounds of 8 points), writes the float4 it would have stored to HBM into the staging tile instead, re-reads it in the MFMA B
// operand layout (lane = point, registers = channels) and runs that level's quarter of the feature_out GEMM (K = 32); after the
// fourth level `hidden` is complete and the two heads follow exactly as in mlp_forward_kernel.  The [P,128] feature array -- 614 MB
// written by the sampler and read back by the MLP at cfg3 -- never exists; the sampler waves of a CU wait on texel gathers while
// its other waves keep the matrix pipe busy.  Same arithmetic in the same order as the two separate kernels (the K order of the
// feature_out GEMM is level 0..3 there too): outputs are bit-identical (tests/test_infer_gpu.py).
//   mlp_pack_split_kernel          the three-way bf16 weight image `spw` of s3g_deform_infer_split (the exact kernel reads the first
//                                  six slabs of mlp_pack_kernel's fp32 image, built through mlp_pack_launch())
//   deform_infer_kernel<UT, SPLIT> UT: uniform time (row tables instead of the time planes); SPLIT: bf16 x 3 arithmetic
// and the three s3g_deform_infer* entry points of include/s3g_mlp.h.  Sampler side: hexplane_dev.hpp; MFMA side: mlp_dev.hpp.
#include "hexplane_dev.hpp"
#include "mlp_dev.hpp"

namespace s3g {

// The split weight image of the inference network (32-bit words; a word = two bf16), in fragments (mlp_dev.hpp).  Rows a layer does
// not have are not stored: the lanes of those rows read some stored row instead, and the accumulator rows they produce are never
// written out (S2 rows 48..63, P2 rows 3..31).
// P1 stays fp32 (split on the fly by the lanes that use it: 44 VALU instructions per fragment) -- all five layers pre-split
// would need 119 KB beside the 48 KB of staging tiles.
namespace spw {
constexpr int FRAG = FRAG_WORDS;                     // words per piece of a full fragment
constexpr int W0 = 0;                                // [mbo 2][ks 8][piece 3][FRAG]
constexpr int S1 = W0 + 2 * 8 * 3 * FRAG;            // [mbo 2][ks 4][piece 3][FRAG]
constexpr int S2A = S1 + 2 * 4 * 3 * FRAG;           // [ks 4][piece 3][FRAG]        rows 0..31
constexpr int S2B = S2A + 4 * 3 * FRAG;              // [ks 4][piece 3][FRAG / 2]    rows 32..47: slot = 16 * h + (row & 15)
constexpr int P2 = S2B + 4 * 3 * (FRAG / 2);         // [ks 4][piece 3][h 2][row 3][4 words]
constexpr int P1LD = 68;                             // fp32 [row 64][64 inputs + 4]: 16 lanes' 16-byte chunks fall in 16 distinct bank groups
constexpr int P1 = P2 + 4 * 3 * 2 * 3 * 4;
constexpr int BIAS = P1 + 64 * P1LD;                 // b0 64 | pb1 64 | sb1 64 | sb2 64 (48 used) | pb2 32 (3 used)
constexpr int B_B0 = 0, B_PB1 = 64, B_SB1 = 128, B_SB2 = 192, B_PB2 = 256, NBIAS = 288;
constexpr int WORDS = (BIAS + NBIAS + 255) / 256 * 256;   // whole 1 KiB DMA rows
static_assert(P2 % 4 == 0 && P1 % 4 == 0 && BIAS % 4 == 0, "16-byte aligned regions");
}  // namespace spw

__global__ void __launch_bounds__(256) mlp_pack_split_kernel(const s3g_mlp_params w, uint32_t* __restrict__ img) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= spw::WORDS) return;
  uint32_t out = 0;
  if (x < spw::S2B) {   // full fragments: W0 | S1 | S2 rows 0..31
    const float* W; int KS, ld, rows, y;
    if (x < spw::S1) { W = w.W0; KS = 8; ld = FEAT; rows = 64; y = x - spw::W0; }
    else if (x < spw::S2A) { W = w.S1; KS = 4; ld = HID; rows = 64; y = x - spw::S1; }
    else { W = w.S2; KS = 4; ld = HID; rows = 48; y = x - spw::S2A; }
    const int t = y & 3, lane = (y >> 2) & 63, piece = (y >> 8) % 3, fr = (y >> 8) / 3, ks = fr % KS, mbo = fr / KS;
    out = split_word(W, rows, ld, 32 * mbo + (lane & 31), split_feature(ks, lane >> 5, 2 * t), split_feature(ks, lane >> 5, 2 * t + 1), piece);
  } else if (x < spw::P2) {   // S2 rows 32..47
    const int y = x - spw::S2B, t = y & 3, slot = (y >> 2) & 31, piece = (y >> 7) % 3, ks = (y >> 7) / 3;
    out = split_word(w.S2, 48, HID, 32 + (slot & 15), split_feature(ks, slot >> 4, 2 * t), split_feature(ks, slot >> 4, 2 * t + 1), piece);
  } else if (x < spw::P1) {   // P2: three rows
    const int y = x - spw::P2, t = y & 3, q = y >> 2, row = q % 3, h = (q / 3) & 1, piece = (q / 6) % 3, ks = q / 18;
    out = split_word(w.P2, 3, HID, row, split_feature(ks, h, 2 * t), split_feature(ks, h, 2 * t + 1), piece);
  } else if (x < spw::BIAS) {   // P1 as it is, rows padded
    const int y = x - spw::P1, row = y / spw::P1LD, f = y % spw::P1LD;
    out = f < HID ? __float_as_uint(w.P1[row * HID + f]) : 0u;
  } else if (x < spw::BIAS + spw::NBIAS) {
    const int y = x - spw::BIAS;
    const float v = y < 64 ? w.b0[y] : y < 128 ? w.pb1[y - 64] : y < 192 ? w.sb1[y - 128] : y < 256 ? (y - 192 < 48 ? w.sb2[y - 192] : 0.f)
                                                                                                  : (y - 256 < 3 ? w.pb2[y - 256] : 0.f);
    out = __float_as_uint(v);
  }
  img[x] = out;
}

struct InferArgs {
  HexArgs h;            // sampler side: descriptor (row tables already swapped in when uniform_time), xyz, time, proc_order, P
  const float* packed;  // mlp_pack_kernel's image
  float *dx, *dshs;
};
constexpr int INF_SLABS = 6;
constexpr int INF_WFLOATS = INF_SLABS * SLAB + 8 * 64;
constexpr int STG_LD = 36;                       // floats per staged point: 32 channels + 4 (16 lanes of a ds_read_b128 hit 16 distinct bank groups)
constexpr int STG_FLOATS = MT * STG_LD;
constexpr int INF_TAP_STRIDE = TAP_SLOTS + 1;    // float4 per point: 6 taps used, padded like tap_stride()
constexpr int INF_WAVE_FLOATS = STG_FLOATS + 2 * 8 * INF_TAP_STRIDE * 4;   // staging tile + two sets of tap slots
constexpr int INF_LDS_FLOATS = INF_WFLOATS + NWAVE * INF_WAVE_FLOATS;
static_assert(INF_LDS_FLOATS * 4 <= 160 * 1024, "inference image + staging must fit the CU's LDS");
// SPLIT (three-way bf16 operands, above): image spw::WORDS, and 6 instead of 9 tap slots per point (the 8 points of a round still
// read 8 disjoint bank groups: 24 words apart)
constexpr int INF_TAP_STRIDE_SPLIT = 6;
constexpr int INF_WAVE_FLOATS_SPLIT = STG_FLOATS + 2 * 8 * INF_TAP_STRIDE_SPLIT * 4;
constexpr int INF_LDS_FLOATS_SPLIT = spw::WORDS + NWAVE * INF_WAVE_FLOATS_SPLIT;
static_assert(INF_LDS_FLOATS_SPLIT * 4 <= 160 * 1024, "split inference image + staging must fit the CU's LDS");

template <bool UT, bool SPLIT>
__global__ void __launch_bounds__(NWAVE * 64) deform_infer_kernel(const InferArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int WIMG = SPLIT ? spw::WORDS : INF_WFLOATS, TAPS = SPLIT ? INF_TAP_STRIDE_SPLIT : INF_TAP_STRIDE;
  constexpr int WAVE_FLOATS = SPLIT ? INF_WAVE_FLOATS_SPLIT : INF_WAVE_FLOATS;
  if constexpr (SPLIT) {
    for (int c = wave; c < spw::WORDS / 256; c += NWAVE)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.packed + c * 256 + lane * 4),
                                       (__attribute__((address_space(3))) void*)(lds + c * 256), 16, 0, 0);
  } else {
    for (int c = wave; c < INF_SLABS * SLAB / 256; c += NWAVE)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.packed + c * 256 + lane * 4),
                                       (__attribute__((address_space(3))) void*)(lds + c * 256), 16, 0, 0);
    if (wave < 2)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.packed + NSLAB * SLAB + wave * 256 + lane * 4),
                                       (__attribute__((address_space(3))) void*)(lds + INF_SLABS * SLAB + wave * 256), 16, 0, 0);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  auto wslab = [&](int k) { return lds + k * SLAB; };
  auto bias = [&](int k) {   // k: b0 | pb1 | sb1 | pb2 | sb2
    if constexpr (SPLIT) return lds + spw::BIAS + (k == 0 ? spw::B_B0 : k == 1 ? spw::B_PB1 : k == 2 ? spw::B_SB1 : k == 3 ? spw::B_PB2 : spw::B_SB2);
    else return lds + INF_SLABS * SLAB + k * 64;
  };
  const uint32_t* wsplit = reinterpret_cast<const uint32_t*>(lds);   // SPLIT: the spw image
  float* stage = lds + WIMG + wave * WAVE_FLOATS;
  const int slot = lane >> 3, j8 = lane & 7, c4 = j8 * 4;   // sampler role: point slot, channel quad
  const int jj = lane & 31, hh = lane >> 5;                 // MFMA role: point column, row half
  float4* tp0 = reinterpret_cast<float4*>(stage + STG_FLOATS) + slot * TAPS;   // two sets of tap slots per point slot
  float4* tp1 = tp0 + 8 * TAPS;
  const int P = a.h.P, ntiles = (P + MT - 1) / MT;
  // texels of one (level, round): spatial planes (x,y) (x,z) (y,z) four corners each; time planes four corners, or -- uniform
  // time -- the two corners of their row tables
  constexpr int NTEX = UT ? 18 : 24;
  struct Tex { float4 v[NTEX]; };
  // normalised coordinates of the tile's 32 points live in the 4 pad floats of their staging rows
  auto taps_for = [&](int l, int rr, float4* tp) {
    const float4 uv = *reinterpret_cast<const float4*>(stage + (8 * rr + slot) * STG_LD + 32);
    const float u[4] = {uv.x, uv.y, uv.z, uv.w};
    produce_taps_level(a.h, u, j8, l, tp);
  };
  auto issue = [&](Tex& T, int l, const float4* tp) {
    int n = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
      const int W = a.h.d.res[l][PAIR0[i]], H = a.h.d.res[l][PAIR1[i]];
      const float* pl = a.h.d.planes[l][i];
      if (UT && IS_TIME_PLANE[i]) {
        const PointTap t = read_tap<true>(tp, 0, i, W, H, c4);
        T.v[n++] = texel4(pl, t.off);
        T.v[n++] = texel4(pl, t.off + t.dx);
      } else {
        const PointTap t = read_tap<false>(tp, 0, i, W, H, c4);
        T.v[n++] = texel4(pl, t.off);
        T.v[n++] = texel4(pl, t.off + t.dx);
        T.v[n++] = texel4(pl, t.off + t.dy);
        T.v[n++] = texel4(pl, t.off + t.dy + t.dx);
      }
    }
  };
  auto consume = [&](const Tex& T, int l, int rr, const float4* tp) {
    float4 prod = make_float4(1.f, 1.f, 1.f, 1.f);
    int n = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
      const int W = a.h.d.res[l][PAIR0[i]], H = a.h.d.res[l][PAIR1[i]];
      float4 s;
      if (UT && IS_TIME_PLANE[i]) {
        const PointTap t = read_tap<true>(tp, 0, i, W, H, c4);
        s = T.v[n] * t.gx;
        s = s + T.v[n + 1] * t.fx;
        n += 2;
      } else {
        const PointTap t = read_tap<false>(tp, 0, i, W, H, c4);
        s = T.v[n] * (t.gx * t.gy);
        s = s + T.v[n + 1] * (t.fx * t.gy);
        s = s + T.v[n + 2] * (t.gx * t.fy);
        s = s + T.v[n + 3] * (t.fx * t.fy);
        n += 4;
      }
      prod = prod * s;
    }
    // SPLIT: the float4 stored below must not come straight out of a PACKED fp32 instruction.  hipcc forms `prod` with
    // v_pk_mul_f32 and issues ds_write_b128 a few slots later; with the other wave of the SIMD issuing v_mfma_f32_32x32x16_bf16 the
    // store then reads STALE data for the last quarter of the wave (lanes 48..63 = two points, errors of 1e-1 in two adjacent rows,
    // different rows every launch): ~800 wrong rows per launch at 1.2 M points, 110 872 over 1000 launches
    // (profiles/r04_split_hazard.jsonl, build `split_nopad`).  It never happens with one wave per SIMD, nor beside the fp32 MFMAs of
    // the exact kernel; waiting for the texel loads, the LDS queue or the wave's own MFMAs does not help.  Round 3 papered over it
    // with 16 wait states (which also happened to make hipcc form the products with plain v_mul_f32).  Round 4 isolates the cause:
    // re-writing the four registers with an ordinary single-pass VALU instruction (v_mov_b32) and NO wait state at all is enough --
    // 0 wrong rows in 1000 launches at 1.2 M points and 400 at 70 001 (build `split_vmov`, now the tree; the 16-wait-state build:
    // also 0) -- i.e. the unsafe pair is "packed-fp32 VALU result -> DS store data" while XDL ops of another wave are in flight,
    // and a real register dependency on a non-packed VALU write removes it independently of timing (forming the products with plain
    // v_mul_f32 is already enough -- build `split_scalarized`, 0 wrong rows --; the v_mov makes that independent of how hipcc chooses
    // to multiply).  ISA of the builds:
    // profiles/r04_split_hazard_isa.txt; stress test: tests/test_infer_gpu.py::test_split_inference_is_bit_reproducible_1000_launches.
    // (The tap slots are stored from v_mov copies, the coordinates by lanes 0..31 only.)
    if (SPLIT) asm volatile("v_mov_b32 %0, %0\n\tv_mov_b32 %1, %1\n\tv_mov_b32 %2, %2\n\tv_mov_b32 %3, %3" : "+v"(prod.x), "+v"(prod.y), "+v"(prod.z), "+v"(prod.w));
    *reinterpret_cast<float4*>(stage + (8 * rr + slot) * STG_LD + c4) = prod;
  };
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
    // 16 steps k = (level k >> 2, round k & 3), two in flight: the texel gathers of step k + 2 are requested before step k's
    // products are formed, and a level's quarter of the feature_out GEMM runs under the next level's first gathers
    auto level_gemm = [&](int l) {   // the level's tile is complete: re-read it in the MFMA B-operand layout, K quarter l of feature_out
      f32x16 x[1];
      wave_lds_sync();
#pragma unroll
      for (int q = 0; q < 4; q++) {   // channels 8q + 4h .. +3 of point jj: the chunk act_load would have read from HBM
        const float4 v = *reinterpret_cast<const float4*>(stage + jj * STG_LD + 8 * q + 4 * hh);
        x[0][4 * q + 0] = v.x; x[0][4 * q + 1] = v.y; x[0][4 * q + 2] = v.z; x[0][4 * q + 3] = v.w;
      }
      if constexpr (SPLIT) {
        ActSplit<1> xs;
        act_split<1, false>(xs, x);
        int ln = lane;
        asm volatile("" : "+v"(ln));   // fragment addresses are derived here, not carried (and spilled) across the sampler steps
        gemm_split<2, 1>(wsplit + spw::W0, 8, 2 * l, xs, hid, ln);
      } else {
        gemm_reg<2, 1, false>(wslab(l >> 1) + 32 * (l & 1) * 65, 65, x, hid, lane);
      }
    };
    if constexpr (UT) {
      Tex A, B;
      taps_for(0, 0, tp0);
      taps_for(0, 1, tp1);
      wave_lds_sync();
      issue(A, 0, tp0);
      issue(B, 0, tp1);
      for (int k = 0; k < 16; k += 2) {
        const int l = k >> 2, rr = k & 3;
        consume(A, l, rr, tp0);
        if (k + 2 < 16) {
          wave_lds_sync();
          taps_for((k + 2) >> 2, (k + 2) & 3, tp0);
          wave_lds_sync();
          issue(A, (k + 2) >> 2, tp0);
        }
        consume(B, l, rr + 1, tp1);
        if (rr == 2) level_gemm(l);   // runs under the gathers of step k + 2 just requested
        if (k + 3 < 16) {
          wave_lds_sync();
          taps_for((k + 3) >> 2, (k + 3) & 3, tp1);
          wave_lds_sync();
          issue(B, (k + 3) >> 2, tp1);
        }
      }
    } else {   // per-point time (24 texels per step): one step in flight
      Tex A;
      for (int l = 0; l < 4; l++) {
        for (int rr = 0; rr < 4; rr++) {
          wave_lds_sync();
          taps_for(l, rr, tp0);
          wave_lds_sync();
          issue(A, l, tp0);
          consume(A, l, rr, tp0);
        }
        level_gemm(l);
      }
    }
    f32x16 act[2], acc[2], o[1];
    if constexpr (SPLIT) {
      ActSplit<2> hs, as;
      act_split<2, true>(hs, hid);   // relu(hidden): the input of both heads
      int ln = lane;
      asm volatile("" : "+v"(ln));   // (as in level_gemm: the heads' LDS addresses are not loop invariants kept in registers)
      const int jj = ln & 31, hh = ln >> 5;
      // pos head.  P1 is fp32 in LDS: a lane's eight weights of a fragment are two swizzled 16-byte chunks of its row
      acc_bias<2>(act, bias(1), ln);
#pragma unroll
      for (int ks = 0; ks < 4; ks++)
#pragma unroll
        for (int mbo = 0; mbo < 2; mbo++) {
          const float* wr = lds + spw::P1 + (32 * mbo + jj) * spw::P1LD + 4 * hh + 16 * ks;   // inputs 16 ks + 4 h + {0..3, 8..11}
          const float4 lo = *reinterpret_cast<const float4*>(wr);
          const float4 hi = *reinterpret_cast<const float4*>(wr + 8);
          const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
          act[mbo] = mfma_split(act[mbo], split8(v), hs.b[ks >> 1][ks & 1]);
        }
      relu_inplace<2>(act);
      act_split<2, false>(as, act);
      acc_bias<1>(o, bias(3), ln);
#pragma unroll
      for (int ks = 0; ks < 4; ks++) {   // P2: rows 0..2 are stored; the other lanes read row 0 (their accumulator rows are never written out)
        Split8 w;
#pragma unroll
        for (int pc = 0; pc < 3; pc++)
          w.p[pc] = *reinterpret_cast<const u32x4*>(wsplit + spw::P2 + ((((ks * 3 + pc) * 2 + hh) * 3 + (jj < 3 ? jj : 0)) << 2));
        o[0] = mfma_split(o[0], w, as.b[ks >> 1][ks & 1]);
      }
      if (livem && hh == 0) {
        float* row = a.dx + pm * 3;
        row[0] = o[0][0]; row[1] = o[0][1]; row[2] = o[0][2];
      }
      // shs head
      acc_bias<2>(act, bias(2), ln);
      gemm_split<2, 2>(wsplit + spw::S1, 4, 0, hs, act, ln);
      relu_inplace<2>(act);
      act_split<2, false>(as, act);
      acc_bias<2>(acc, bias(4), ln);
      gemm_split<1, 2>(wsplit + spw::S2A, 4, 0, as, *reinterpret_cast<f32x16(*)[1]>(&acc[0]), ln);
#pragma unroll
      for (int ks = 0; ks < 4; ks++) {   // rows 32..47: lanes of rows 48..63 read rows 32..47 again (never written out)
        Split8 w;
#pragma unroll
        for (int pc = 0; pc < 3; pc++)
          w.p[pc] = *reinterpret_cast<const u32x4*>(wsplit + spw::S2B + (ks * 3 + pc) * (spw::FRAG / 2) + ((16 * hh + (jj & 15)) << 2));
        acc[1] = mfma_split(acc[1], w, as.b[ks >> 1][ks & 1]);
      }
    } else {
    // pos head
    acc_bias<2>(act, bias(1), lane);
    gemm_reg<2, 2, true>(wslab(2), 65, hid, act, lane);
    relu_inplace<2>(act);
    {
      float o3[3] = {0.f, 0.f, 0.f};
      head3_fw(wslab(4), bias(3), act, o3, lane);
      if (livem && hh == 0) {
        float* row = a.dx + pm * 3;
        row[0] = o3[0]; row[1] = o3[1]; row[2] = o3[2];
      }
    }
    // shs head
    acc_bias<2>(act, bias(2), lane);
    gemm_reg<2, 2, true>(wslab(3), 65, hid, act, lane);
    relu_inplace<2>(act);
    acc_bias<2>(acc, bias(4), lane);
    gemm_reg<2, 2, false>(wslab(5), 65, act, acc, lane);
    }
    if (livem) {
      float* row = a.dshs + pm * 48 + 4 * hh;
#pragma unroll
      for (int mb = 0; mb < 2; mb++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
          if (32 * mb + 8 * q >= 48) continue;
          *reinterpret_cast<float4*>(row + 32 * mb + 8 * q) =
              make_float4(acc[mb][4 * q + 0], acc[mb][4 * q + 1], acc[mb][4 * q + 2], acc[mb][4 * q + 3]);
        }
    }
    wave_lds_sync();   // the next tile's coordinates go into the pads this tile's taps were derived from
  }
}

}  // namespace s3g

using namespace s3g;

extern "C" size_t s3g_deform_infer_workspace_bytes(const s3g_hexplane_desc* d) {
  if (!d || d->levels != 4) return 0;
  return ((size_t)PACK_FLOATS + (d->uniform_time ? time_table_floats(d) : 0)) * sizeof(float);
}

static int deform_infer_impl(const s3g_hexplane_desc* d, const s3g_mlp_params* w, int P, const float* xyz, const float* time,
                             const unsigned int* proc_order, float* dx, float* dshs, void* workspace, void* stream_, bool split) {
  if (int e = check_desc(d)) return e;
  if (d->levels != 4) {
    set_error("s3g_deform_infer: the fused path is built for 4 levels x 32 channels = feature_out's 128 inputs");
    return S3G_ERR_INVALID_ARG;
  }
  if (!w || P < 0 || (P > 0 && (!xyz || !time || !dx || !dshs || !workspace))) {
    set_error("s3g_deform_infer: bad argument");
    return S3G_ERR_INVALID_ARG;
  }
  if (P == 0) return S3G_OK;
  hipStream_t stream = (hipStream_t)stream_;
  static std::atomic<uint64_t> done{0};
  if (device_needs_setup(done)) {
    S3G_HIP_CHECK(hipFuncSetAttribute((const void*)deform_infer_kernel<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, INF_LDS_FLOATS * 4));
    S3G_HIP_CHECK(hipFuncSetAttribute((const void*)deform_infer_kernel<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, INF_LDS_FLOATS * 4));
    S3G_HIP_CHECK(hipFuncSetAttribute((const void*)deform_infer_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, INF_LDS_FLOATS_SPLIT * 4));
    S3G_HIP_CHECK(hipFuncSetAttribute((const void*)deform_infer_kernel<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, INF_LDS_FLOATS_SPLIT * 4));
    device_setup_done(done);
  }
  float* packed = (float*)workspace;
  InferArgs a;
  memset(&a, 0, sizeof a);
  a.h.d = *d; a.h.P = P; a.h.xyz = xyz; a.h.time = time; a.h.proc_order = proc_order;
  a.packed = packed; a.dx = dx; a.dshs = dshs;
  TimeRows rows;
  if (d->uniform_time) use_time_rows(a.h, rows, packed + PACK_FLOATS, nullptr, stream);
  static_assert(spw::WORDS <= PACK_FLOATS, "both weight images fit the front of the workspace");
  if (split) hipLaunchKernelGGL(mlp_pack_split_kernel, dim3(spw::WORDS / 256), dim3(256), 0, stream, *w, reinterpret_cast<uint32_t*>(packed));
  else mlp_pack_launch(*w, packed, stream);
  const int ntiles = (P + MT - 1) / MT;
  const int blocks = min((ntiles + NWAVE - 1) / NWAVE, 256);
  const dim3 grid(blocks), wg(NWAVE * 64);
  profile_begin(S3G_PROFILE_DEFORM_INFER, stream);
  if (split) {
    if (d->uniform_time) hipLaunchKernelGGL((deform_infer_kernel<true, true>), grid, wg, INF_LDS_FLOATS_SPLIT * 4, stream, a);
    else hipLaunchKernelGGL((deform_infer_kernel<false, true>), grid, wg, INF_LDS_FLOATS_SPLIT * 4, stream, a);
  } else {
    if (d->uniform_time) hipLaunchKernelGGL((deform_infer_kernel<true, false>), grid, wg, INF_LDS_FLOATS * 4, stream, a);
    else hipLaunchKernelGGL((deform_infer_kernel<false, false>), grid, wg, INF_LDS_FLOATS * 4, stream, a);
  }
  profile_end(S3G_PROFILE_DEFORM_INFER, stream, (double)P, 4.0);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" int s3g_deform_infer(const s3g_hexplane_desc* d, const s3g_mlp_params* w, int P, const float* xyz, const float* time,
                                const unsigned int* proc_order, float* dx, float* dshs, void* workspace, void* stream) {
  return deform_infer_impl(d, w, P, xyz, time, proc_order, dx, dshs, workspace, stream, false);
}
extern "C" int s3g_deform_infer_split(const s3g_hexplane_desc* d, const s3g_mlp_params* w, int P, const float* xyz, const float* time,
                                      const unsigned int* proc_order, float* dx, float* dshs, void* workspace, void* stream) {
  return deform_infer_impl(d, w, P, xyz, time, proc_order, dx, dshs, workspace, stream, true);
}
