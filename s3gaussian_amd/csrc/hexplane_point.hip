// HexPlane backward, pass A (overview: hexplane.hip): the product-rule form (S3G_HEX_SLAB) and the division form (S3G_HEX_SLAB_DIV).
#include "hexplane_bwd.hpp"

namespace s3g {

// ---- pass A: per point, dL/dxyz and the level's row T = dL/dfeature * feature -> G ----
// G layout (point-major): the `levels` rows of a point are contiguous, points in PROCESSING order, so pass A streams its stores:
// row l of processing position pi = G + (pi * levels + l) * 32; a scatter walk reads it by the position comp[oi][k] of its k-th point.

// Same lane mapping and tap sharing as the forward.  Per plane only the sample s and its two coordinate derivatives are kept:
// ds/dix = (ne - nw)(y1 - iy) + (se - sw)(iy - y0),  ds/diy = (sw - nw)(x1 - ix) + (se - ne)(ix - x0)  (the four terms of
// torch's grid_sampler_2d_backward, grouped).
//
// What bounds pass A (cfg3, 1.2 M points, 1.43 ms; PMC pass in profiles/r02_hexplane_sq_pmc.txt): its waves sit parked on
// s_waitcnt 63 % of their resident time and issue VALU 18 % of it (288 M wave-instructions = 0.5 ms of pure issue) -- at two
// waves per SIMD (172 registers: six samples and their derivatives have to be live for the product rule) nothing hides a
// memory round trip (1.07 ms with the G stores compiled out; issuing the next level's loads BEFORE this level's stores -- vmcnt
// is one in-order counter for loads and stores -- changed nothing: 1.437 vs 1.435 ms).  Everything tried against the latency
// made it slower or did nothing, because each costs registers and this kernel has none to give: a second texel register set prefetching the next level (persistent workgroups,
// next group's index / coordinates / taps prefetched as well): 1.86 ms at 256 VGPRs with spills; the same unrolled so that
// no set crosses a loop back-edge, next level's loads issued between samples() and this level's stores: 1.94 ms (285 VGPRs,
// or 256 with spills); launch_bounds for three waves: 1.69 ms (spills).  Without effect: halving the VALU work (shared taps),
// pointing every texel load at one hot line, the blocked order / XCD-contiguous groups (the forward gains 8 % from those).
// Point-major G (24 rows of a point contiguous, points in processing order -> streaming stores): 1.50 -> 1.43 ms; padding the
// tap slots against LDS bank conflicts: 1.42 -> 1.33 ms; more waves (16 lanes per point: 4 per SIMD) 1.73 ms.
// A lane owns four channels (f4v, 8 lanes per point).  The 2-channel form (16 lanes per point: half the live registers per lane --
// the six samples and their derivatives -- hence twice the waves per SIMD to hide the round trips, for ~20 % more VALU work) was
// measured slower: 106 VGPRs = 4 waves per SIMD, but 1.73 vs 1.53 ms.
__device__ __forceinline__ f4v vsplat(float x) { return f4v{x, x, x, x}; }
__device__ __forceinline__ float vdot(f4v a, f4v b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
__device__ __forceinline__ float vget(f4v v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : (k == 2 ? v.z : v.w)); }
__device__ __forceinline__ f4v texelv(const float* __restrict__ plane, uint32_t byte_off) {
  return *reinterpret_cast<const f4v*>(reinterpret_cast<const char*>(plane) + byte_off);
}
struct LevelIn {       // texels of one level's planes (uniform time: the three spatial planes only) + the dL/dfeature row
  f4v v[6][4];
  f4v g;
};
template <bool UT>
__device__ __forceinline__ void issue_level(const HexArgs& a, const float4* __restrict__ taps, int l, int c0, const float* __restrict__ grow, LevelIn& in) {
#pragma unroll
  for (int i = 0; i < 6; i++) {
    const int W = a.d.res[l][PAIR0[i]], H = a.d.res[l][PAIR1[i]];
    const float* pl = a.d.planes[l][i];
    if (UT && IS_TIME_PLANE[i]) {
      // row tables (a few hundred KB in total, L1 / L2 resident) are read where they are used
    } else {
      const PointTap t = read_tap<false>(taps, l, i, W, H, c0);
      in.v[i][0] = texelv(pl, t.off);
      in.v[i][1] = texelv(pl, t.off + t.dx);
      in.v[i][2] = texelv(pl, t.off + t.dy);
      in.v[i][3] = texelv(pl, t.off + t.dy + t.dx);
    }
  }
  const f4v* src = reinterpret_cast<const f4v*>(grow + l * HEXC);
  in.g = __builtin_nontemporal_load(src);   // dL/dfeature rows are read once
}
// The arithmetic of one level in two halves:
//   samples()  texels -> s, ds/dix, ds/diy per plane (the texel registers are dead afterwards);
//   finish()   product rule -> six G rows (stored when `store`) and this level's share of dL/du.
struct LevelS {
  f4v s[6], dX[6], dY[6];
  float mx[6], my[6];
};
template <bool UT>
__device__ __forceinline__ void samples_level(const HexArgs& a, const float4* __restrict__ taps, int l, int c0, const LevelIn& in, LevelS& S) {
#pragma unroll
  for (int i = 0; i < 6; i++) {
    const int W = a.d.res[l][PAIR0[i]], H = a.d.res[l][PAIR1[i]];
    if (UT && IS_TIME_PLANE[i]) {
      const PointTap t = read_tap<true>(taps, l, i, W, H, c0);
      const float* pl = a.d.planes[l][i];
      const f4v v00 = texelv(pl, t.off), v01 = texelv(pl, t.off + t.dx);
      S.s[i] = v00 * t.gx;
      S.s[i] = S.s[i] + v01 * t.fx;
      S.dX[i] = v01 - v00;
      S.dY[i] = vsplat(0.f);
      S.mx[i] = t.mx; S.my[i] = 0.f;
    } else {
      const PointTap t = read_tap<false>(taps, l, i, W, H, c0);
      const f4v v00 = in.v[i][0], v01 = in.v[i][1], v10 = in.v[i][2], v11 = in.v[i][3];
      f4v acc = v00 * (t.gx * t.gy);
      acc = acc + v01 * (t.fx * t.gy);
      acc = acc + v10 * (t.gx * t.fy);
      acc = acc + v11 * (t.fx * t.fy);
      S.s[i] = acc;
      // a corner that is out of range is the nw / ne / sw texel again: its difference terms are then multiplied by an
      // exactly-zero mask (mx or my) below, as the reference's are by the border clip
      S.dX[i] = (v01 - v00) * t.gy + (v11 - v10) * t.fy;
      S.dY[i] = (v10 - v00) * t.gx + (v11 - v01) * t.fx;
      S.mx[i] = t.mx; S.my[i] = t.my;
    }
  }
}
// one sample of plane i of level l at point coordinates u, channel c: make_tap + the four weighted texels in the order every
// HexPlane kernel uses (with uniform time the (axis, t) planes are height-1 row tables: res[l][3] == 1, iy == 0)
__device__ __forceinline__ float walk_sample(const HexArgs& a, int l, int i, const float* u, int c) {
  const int W = a.d.res[l][PAIR0[i]], H = a.d.res[l][PAIR1[i]];
  const Tap t = make_tap(u[PAIR0[i]], u[PAIR1[i]], W, H);
  const float* pl = a.d.planes[l][i];
  float acc = fetch(pl, t.o00, c) * t.w00;
  acc = acc + fetch(pl, t.o01, c) * t.w01;
  acc = acc + fetch(pl, t.o10, c) * t.w10;
  acc = acc + fetch(pl, t.o11, c) * t.w11;
  return acc;
}
// The scatter walk divides T by the sample it re-derives; where it cannot (same predicate on the same bits) the exact gradient
// g * prod_{j != i} s_j is scattered here with the walk's own corner weights.  Runs for (nearly) zero or non-finite samples only,
// so it keeps nothing of the hot path's registers: everything is re-derived from the point's coordinates.
__device__ __forceinline__ void tslab_exact_scatter(const HexArgs& a, int p, int l, int c0, f4v g, uint32_t badbits) {
  float u[4];
  point_coords(a, p, u);
#pragma unroll 1
  for (int i = 0; i < 6; i++) {
    float* gp = a.gplanes[l][i];
    if (!((badbits >> i) & 1u) || gp == nullptr) continue;
    const int W = a.d.res[l][PAIR0[i]], H = a.d.res[l][PAIR1[i]];
    const Tap t = make_tap(u[PAIR0[i]], u[PAIR1[i]], W, H);
#pragma unroll 1
    for (int k = 0; k < 4; k++) {
      const int c = c0 + k;
      if (tslab_divisible(walk_sample(a, l, i, u, c))) continue;
      float gk = vget(g, k);
#pragma unroll 1
      for (int jj = 0; jj < 6; jj++)
        if (jj != i) gk *= walk_sample(a, l, jj, u, c);
      atomicAdd(gp + (size_t)t.o00 * HEXC + c, t.w00 * gk);
      if (t.o01 >= 0) atomicAdd(gp + (size_t)t.o01 * HEXC + c, t.w01 * gk);
      if (t.o10 >= 0) atomicAdd(gp + (size_t)t.o10 * HEXC + c, t.w10 * gk);
      if (t.o11 >= 0) atomicAdd(gp + (size_t)t.o11 * HEXC + c, t.w11 * gk);
    }
  }
}
template <bool UT>
__device__ __forceinline__ void finish_level(const HexArgs& a, int p, int l, int c0, const LevelS& S, f4v g,
                                             bool store, float* __restrict__ G, size_t gbase, float* du) {
  // product rule in the order autograd applies it to ((((1*s0)*s1)*s2)*s3)*s4)*s5: pre[i] = prod_{j<i} s_j, suffix by recursion
  f4v pre[6];
  pre[0] = vsplat(1.f);
#pragma unroll
  for (int i = 1; i < 6; i++) pre[i] = pre[i - 1] * S.s[i - 1];
  f4v gs = g;  // dL/d(prefix product through plane i)
  uint32_t badbits = 0;   // T-slab: planes with a sample the scatter walk cannot divide by
#pragma unroll
  for (int i = 5; i >= 0; i--) {
    const f4v gi = gs * pre[i];  // dL/ds_i
    gs = gs * S.s[i];
    if (store) {
#pragma unroll
      for (int k = 0; k < 4; k++) badbits |= tslab_near_unsafe(vget(S.s[i], k)) ? (1u << i) : 0u;
      if (PAIR0[i] < 3) du[PAIR0[i]] += S.mx[i] * vdot(S.dX[i], gi);
      if (PAIR1[i] < 3) du[PAIR1[i]] += S.my[i] * vdot(S.dY[i], gi);
    }
  }
  if (store) {   // gs = g * s5 * s4 * ... * s0 = dL/dfeature * feature: the level's ONE row, gbase = position * levels rows
    f4v* trow = reinterpret_cast<f4v*>(G + gbase + (size_t)(l * HEXC + c0));
    __builtin_nontemporal_store(gs, trow);   // streaming stores of the gradient slab: point pass 1.83 -> 1.60 ms
    if (badbits) tslab_exact_scatter(a, p, l, c0, g, badbits);   // rare: a sample that is (nearly) zero or not finite
  }
}

template <bool UT, int LV>   // LV > 0: level count at compile time (unrolled: the per-level plane pointers and resolutions are fetched up front instead of four dependent scalar loads per level)
__global__ void __launch_bounds__(256) hexplane_backward_point_kernel(const HexArgs a, float* __restrict__ G) {
  extern __shared__ float4 tapbuf[];   // [32 points][levels][TAP_SLOTS]
  const int j = threadIdx.x & 7, c0 = j * 4, slot = threadIdx.x >> 3;
  const int L = LV > 0 ? LV : a.d.levels;
  const int F = L * HEXC;
  float4* taps = tapbuf + (size_t)slot * tap_stride(L);
  for (int p0 = xcd_group(blockIdx.x, gridDim.x) * 32; p0 < a.P; p0 += gridDim.x * 32) {  // uniform trip count: shuffles below need all lanes
    const int pi = p0 + slot;
    const bool live = pi < a.P;
    const int p = live ? (a.proc_order ? (int)a.proc_order[pi] : pi) : 0;
    const size_t gbase = (size_t)pi * (size_t)(L * HEXC);   // point-major layout: the rows of this PROCESSING position
    float u[4];
    point_coords(a, p, u);
    wave_lds_sync();
    produce_taps(a, u, j, taps);
    wave_lds_sync();
    const float* grow = a.gfeat + (size_t)p * F + c0;
    float du[3] = {0.f, 0.f, 0.f};
    if constexpr (LV == 4) {
      // T-slab: with the 24 G rows gone the kernel has registers to spare (188 of 256): the NEXT level's texels are requested
      // before this level's arithmetic, in two alternating register sets (fully unrolled: no set crosses a back-edge)
      LevelIn X0, X1;
      issue_level<UT>(a, taps, 0, c0, grow, X0);
#pragma unroll
      for (int l = 0; l < 4; l += 2) {
        issue_level<UT>(a, taps, l + 1, c0, grow, X1);
        __builtin_amdgcn_sched_barrier(0);
        {
          LevelS S;
          samples_level<UT>(a, taps, l, c0, X0, S);
          finish_level<UT>(a, p, l, c0, S, X0.g, live, G, gbase, du);
        }
        if (l + 2 < 4) issue_level<UT>(a, taps, l + 2, c0, grow, X0);
        __builtin_amdgcn_sched_barrier(0);
        {
          LevelS S;
          samples_level<UT>(a, taps, l + 1, c0, X1, S);
          finish_level<UT>(a, p, l + 1, c0, S, X1.g, live, G, gbase, du);
        }
      }
    } else {
#pragma unroll LV > 0 ? LV : 1
    for (int l = 0; l < L; l++) {
      LevelIn X;
      LevelS S;
      issue_level<UT>(a, taps, l, c0, grow, X);
      samples_level<UT>(a, taps, l, c0, X, S);
      finish_level<UT>(a, p, l, c0, S, X.g, live, G, gbase, du);
    }
    }
    // sum over the 32 channels (the 8 lanes of this point), then undo the aabb normalisation
#pragma unroll
    for (int k = 0; k < 3; k++) {
      float v = du[k];
      for (int off = 4; off >= 1; off >>= 1) v += __shfl_xor(v, off);
      du[k] = v;
    }
    if (live && j < 3) a.gxyz[3 * (size_t)p + j] = (j == 0 ? du[0] : (j == 1 ? du[1] : du[2])) * (2.0f / (a.d.aabb_min[j] - a.d.aabb_max[j]));
  }
}

// ---- pass A, DIVISION form (round 4, `algorithm` S3G_HEX_SLAB_DIV: needs the forward's output `feat`) ----
// The product-rule kernel above keeps six samples and their twelve derivative vectors live per level (252 VGPRs with the next
// level's texels in flight: two waves per SIMD, parked on s_waitcnt 63 % of the time) only to form dL/ds_i = g * prod_{j != i} s_j.
// With the forward's own output f = prod_j s_j at hand the level's row is T = g * f in ONE multiply, and dL/ds_i = T / s_i needs
// nothing but plane i's own sample: the planes are processed one after the other like the forward does (texels, sample, two
// derivative vectors, two dot products -- then everything but three scalars is dead), at the forward's register count and
// occupancy, so that the 72 texel-line gathers per point hide behind other waves instead of behind nothing.  Same division and
// same safety predicate as the scatter walk (tv * rcp(s), |s| in (1e-18, inf)); a sample that fails it gets its EXACT
// g * prod_{j != i} s_j -- for the plane gradients through tslab_exact_scatter, for dL/dxyz through exact_du below -- re-derived
// from the coordinates on a path that costs the hot loop no registers.
__device__ __forceinline__ void exact_du(const HexArgs& a, int p, int l, int c0, f4v g, uint32_t badbits, float* du) {
  float u[4];
  point_coords(a, p, u);
#pragma unroll 1
  for (int i = 0; i < 6; i++) {
    if (!((badbits >> i) & 1u)) continue;
    const int W = a.d.res[l][PAIR0[i]], H = a.d.res[l][PAIR1[i]];
    const Tap t = make_tap(u[PAIR0[i]], u[PAIR1[i]], W, H);
    const float* pl = a.d.planes[l][i];
#pragma unroll 1
    for (int k = 0; k < 4; k++) {
      const int c = c0 + k;
      if (!tslab_near_unsafe(walk_sample(a, l, i, u, c))) continue;     // that channel went through the division (same wide predicate)
      float gk = vget(g, k);
#pragma unroll 1
      for (int jj = 0; jj < 6; jj++)
        if (jj != i) gk *= walk_sample(a, l, jj, u, c);
      const float v00 = fetch(pl, t.o00, c), v01 = fetch(pl, t.o01 >= 0 ? t.o01 : t.o00, c);
      const float v10 = fetch(pl, t.o10 >= 0 ? t.o10 : t.o00, c);
      const float v11 = fetch(pl, t.o11 >= 0 ? t.o11 : (t.o10 >= 0 ? t.o10 : (t.o01 >= 0 ? t.o01 : t.o00)), c);
      const float dX = (v01 - v00) * (t.y1f - t.iy) + (v11 - v10) * (t.iy - t.y0f);
      const float dY = (v10 - v00) * (t.x1f - t.ix) + (v11 - v01) * (t.ix - t.x0f);
      if (PAIR0[i] < 3) du[PAIR0[i]] += t.mx * dX * gk;
      if (PAIR1[i] < 3) du[PAIR1[i]] += t.my * dY * gk;
    }
  }
}

#ifndef S3G_HEX_POINTDIV_WAVES
#define S3G_HEX_POINTDIV_WAVES 4
#endif

template <bool UT>
__global__ void __launch_bounds__(256, S3G_HEX_POINTDIV_WAVES) hexplane_backward_pointdiv_kernel(const HexArgs a, const float* __restrict__ feat,
                                                                                                  float* __restrict__ G) {
  extern __shared__ float4 tapbuf[];   // [32 points][levels][TAP_SLOTS]
  const int j = threadIdx.x & 7, c0 = j * 4, slot = threadIdx.x >> 3;
  const int L = a.d.levels, F = L * HEXC;
  float4* taps = tapbuf + (size_t)slot * tap_stride(L);
  for (int p0 = xcd_group(blockIdx.x, gridDim.x) * 32; p0 < a.P; p0 += gridDim.x * 32) {  // uniform trip count: shuffles below need all lanes
    const int pi = p0 + slot;
    const bool live = pi < a.P;
    const int p = live ? (a.proc_order ? (int)a.proc_order[pi] : pi) : 0;
    const size_t gbase = (size_t)pi * (size_t)(L * HEXC);   // T rows of this PROCESSING position
    float u[4];
    point_coords(a, p, u);
    wave_lds_sync();
    produce_taps(a, u, j, taps);
    wave_lds_sync();
    const size_t row = (size_t)p * F + c0;
    float du[3] = {0.f, 0.f, 0.f};
    // (requesting the NEXT level's two rows a level ahead costs the eight registers that keep this kernel at four waves per SIMD:
    // 0.78 -> 1.12 ms with the spills, 0.88 ms at three waves -- measured, tools/variants/r04_pointdiv2.py)
    for (int l = 0; l < L; l++) {
      const f4v g = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(a.gfeat + row + l * HEXC));
      const f4v f = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(feat + row + l * HEXC));
      const f4v T = g * f;
      if (live) __builtin_nontemporal_store(T, reinterpret_cast<f4v*>(G + gbase + (size_t)(l * HEXC + c0)));
      uint32_t badbits = 0;
#pragma unroll
      for (int i = 0; i < 6; i++) {
        const int W = a.d.res[l][PAIR0[i]], H = a.d.res[l][PAIR1[i]];
        const float* pl = a.d.planes[l][i];
        f4v sv, dX, dY;
        float mx, my;
        if (UT && IS_TIME_PLANE[i]) {
          const PointTap t = read_tap<true>(taps, l, i, W, H, c0);
          const f4v v00 = texelv(pl, t.off), v01 = texelv(pl, t.off + t.dx);
          sv = v00 * t.gx;
          sv = sv + v01 * t.fx;
          dX = v01 - v00;
          dY = vsplat(0.f);
          mx = t.mx; my = 0.f;
        } else {
          const PointTap t = read_tap<false>(taps, l, i, W, H, c0);
          const f4v v00 = texelv(pl, t.off), v01 = texelv(pl, t.off + t.dx);
          const f4v v10 = texelv(pl, t.off + t.dy), v11 = texelv(pl, t.off + t.dy + t.dx);
          sv = v00 * (t.gx * t.gy);
          sv = sv + v01 * (t.fx * t.gy);
          sv = sv + v10 * (t.gx * t.fy);
          sv = sv + v11 * (t.fx * t.fy);
          dX = (v01 - v00) * t.gy + (v11 - v10) * t.fy;
          dY = (v10 - v00) * t.gx + (v11 - v01) * t.fx;
          mx = t.mx; my = t.my;
        }
        f4v gi;
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const float sk = vget(sv, k);
          // ONE predicate per channel, the WIDE one: this pass divides only where |s| clears the threshold by a factor of four and
          // hands everything else to the exact fallback (exact_du applies the same wide predicate to the same bits; the plane
          // gradients' fallback, tslab_exact_scatter, applies the strict one the scatter walk uses).  A second, strict compare per
          // channel here cost the two registers that keep the kernel at four waves per SIMD: 0.76 -> 0.92 ms with the spills.
          const bool okk = !tslab_near_unsafe(sk);
          ok = ok && okk;
          const float q = okk ? vget(T, k) * __builtin_amdgcn_rcpf(sk) : 0.f;
          if (k == 0) gi.x = q; else if (k == 1) gi.y = q; else if (k == 2) gi.z = q; else gi.w = q;
        }
        badbits |= ok ? 0u : (1u << i);
        if (PAIR0[i] < 3) du[PAIR0[i]] += mx * vdot(dX, gi);
        if (PAIR1[i] < 3) du[PAIR1[i]] += my * vdot(dY, gi);
      }
      if (badbits && live) {   // rare: a sample that is (nearly) zero or not finite
        tslab_exact_scatter(a, p, l, c0, g, badbits);
        exact_du(a, p, l, c0, g, badbits, du);
      }
    }
    // sum over the 32 channels (the 8 lanes of this point), then undo the aabb normalisation
#pragma unroll
    for (int k = 0; k < 3; k++) {
      float v = du[k];
      for (int off = 4; off >= 1; off >>= 1) v += __shfl_xor(v, off);
      du[k] = v;
    }
    if (live && j < 3) a.gxyz[3 * (size_t)p + j] = (j == 0 ? du[0] : (j == 1 ? du[1] : du[2])) * (2.0f / (a.d.aabb_min[j] - a.d.aabb_max[j]));
  }
}

int hexplane_point_launch(const HexArgs& a, const float* features, int algorithm, float* G, hipStream_t stream) {
  const int P = a.P, blocks = (P + 31) / 32;
  const size_t lds = (size_t)32 * tap_stride(a.d.levels) * sizeof(float4);
  profile_begin(S3G_PROFILE_HEXPLANE_BACKWARD_POINT, stream);
  if (algorithm == S3G_HEX_SLAB_DIV) {
    if (a.d.uniform_time) hipLaunchKernelGGL(hexplane_backward_pointdiv_kernel<true>, dim3(blocks), dim3(256), lds, stream, a, features, G);
    else hipLaunchKernelGGL(hexplane_backward_pointdiv_kernel<false>, dim3(blocks), dim3(256), lds, stream, a, features, G);
  } else if (a.d.uniform_time && a.d.levels == 4) hipLaunchKernelGGL((hexplane_backward_point_kernel<true, 4>), dim3(blocks), dim3(256), lds, stream, a, G);
  else if (a.d.uniform_time) hipLaunchKernelGGL((hexplane_backward_point_kernel<true, 0>), dim3(blocks), dim3(256), lds, stream, a, G);
  else hipLaunchKernelGGL((hexplane_backward_point_kernel<false, 0>), dim3(blocks), dim3(256), lds, stream, a, G);
  profile_end(S3G_PROFILE_HEXPLANE_BACKWARD_POINT, stream, (double)P, (double)a.d.levels);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

}  // namespace s3g
