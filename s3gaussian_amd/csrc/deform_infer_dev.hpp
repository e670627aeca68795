// The sampler half of deform_infer_heads_kernel<UT> (deform_infer_heads.hip), as a struct: a wave samples ONE LEVEL of its 32 points
// the way hexplane_forward_kernel does (8 lanes per point, four rounds of 8 points) and parks the float4 it would have stored to HBM in
// its 32-point x 32-channel staging tile; the kernel's `level_gemm` re-reads the tile in the MFMA B operand layout and runs that level's
// quarter of the feature_out GEMM.  Statement for statement the sampler lambdas of deform_infer_kernel<UT, false> (deform_infer.hip),
// which keeps its own: routing that kernel through this struct gives the same results from differently allocated registers, and its
// machine code is pinned (profiles/infer_heads_isa_identity.txt).  A change to either copy belongs in both.
// Private to libs3g.so (not part of the C ABI).
#pragma once
#include "hexplane_dev.hpp"
#include "mlp_dev.hpp"

namespace s3g {

constexpr int STG_LD = 36;                       // floats per staged point: 32 channels + 4 (16 lanes of a ds_read_b128 hit 16 distinct bank groups)
constexpr int STG_FLOATS = MT * STG_LD;
constexpr int INF_TAP_STRIDE = TAP_SLOTS + 1;    // float4 per point: 6 taps used, padded like tap_stride()
constexpr int INF_WAVE_FLOATS = STG_FLOATS + 2 * 8 * INF_TAP_STRIDE * 4;   // staging tile + two sets of tap slots

// One wave's sampler state: `stage` = its staging tile (the normalised coordinates of the tile's 32 points live in the 4 pad floats of
// their staging rows), followed by two sets of tap slots of INF_TAP_STRIDE float4 per point slot.
template <bool UT>
struct InferSampler {
  // texels of one (level, round): spatial planes (x,y) (x,z) (y,z) four corners each; time planes four corners, or -- uniform
  // time -- the two corners of their row tables
  static constexpr int NTEX = UT ? 18 : 24;
  struct Tex { float4 v[NTEX]; };
  const HexArgs& h;
  float* stage;
  int slot, j8, c4;    // sampler role of the lane: point slot, lane of the point, channel quad
  float4 *tp0, *tp1;   // the lane's point slot in the two sets of tap slots (INF_TAP_STRIDE float4 per point slot)

  __device__ __forceinline__ void taps_for(int l, int rr, float4* tp) const {
    const float4 uv = *reinterpret_cast<const float4*>(stage + (8 * rr + slot) * STG_LD + 32);
    const float u[4] = {uv.x, uv.y, uv.z, uv.w};
    produce_taps_level(h, u, j8, l, tp);
  }
  __device__ __forceinline__ void issue(Tex& T, int l, const float4* tp) const {
    int n = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
      const int W = h.d.res[l][PAIR0[i]], H = h.d.res[l][PAIR1[i]];
      const float* pl = h.d.planes[l][i];
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
  }
  __device__ __forceinline__ void consume(const Tex& T, int l, int rr, const float4* tp) const {
    float4 prod = make_float4(1.f, 1.f, 1.f, 1.f);
    int n = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
      const int W = h.d.res[l][PAIR0[i]], H = h.d.res[l][PAIR1[i]];
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
    *reinterpret_cast<float4*>(stage + (8 * rr + slot) * STG_LD + c4) = prod;
  }
  // All four levels of the tile whose coordinates sit in the staging pads; level_gemm(l) is called when level l's tile is complete.
  // 16 steps k = (level k >> 2, round k & 3), two in flight: the texel gathers of step k + 2 are requested before step k's
  // products are formed, and a level's quarter of the feature_out GEMM runs under the next level's first gathers
  template <class LevelGemm>
  __device__ __forceinline__ void run(LevelGemm&& level_gemm) const {
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
  }
};

}  // namespace s3g
