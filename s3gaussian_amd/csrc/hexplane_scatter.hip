// HexPlane backward, pass B (overview: hexplane.hip): scatter in sorted order with register run-length combining; deterministic
// mode: run records and the stencil gather.
#include "hexplane_bwd.hpp"

namespace s3g {

typedef float f2v_ __attribute__((ext_vector_type(2)));
// One bilinear footprint being accumulated in registers by a walker lane (= one channel): key = texel offset of its nw corner
// (-1 = empty), flags bit0 = ne/se column in range, bit1 = sw/se row in range (the other three corners follow from key, flags and
// the plane width).  The UNPACKED form of Foot1 below, which foot1_flush_all converts to at the end of a walk: issuing those atomics
// straight from Foot1's pairs compiles both atomic walks to another register allocation (68 -> 70 and 72 -> 74 VGPRs).
struct Foot {
  int key, flags;
  float a00, a01, a10, a11;
};
__device__ __forceinline__ void vatomic(char* base, uint32_t k, float v) { atomicAdd(reinterpret_cast<float*>(base + k), v); }
// Offsets are 32-bit BYTE offsets off a uniform base pointer (`base + zext(u32)` selects the scalar-base + VGPR-offset
// addressing mode: no 64-bit address arithmetic per atomic; a plane is at most 2^24 texels).  The corner tests stay
// branches on purpose: an unconditional atomic of an exact zero to a clamped address was measured 6x SLOWER for the whole
// pass -- every empty entry and every out-of-range corner then lands on the same few lines (texel 0 of each plane, the nw
// texel again), and same-address atomics serialise at ~10 ns each.  c = channel of the lane.
__device__ __forceinline__ void foot_flush(const Foot& f, float* __restrict__ gp, int W, int c) {
  if (f.key < 0) return;
  const uint32_t k = ((uint32_t)f.key * HEXC + (uint32_t)c) * 4u;
  const uint32_t dy = (uint32_t)W * (HEXC * 4u);
  char* base = reinterpret_cast<char*>(gp);
  vatomic(base, k, f.a00);
  if (f.flags & 1) vatomic(base, k + HEXC * 4u, f.a01);
  if (f.flags & 2) vatomic(base, k + dy, f.a10);
  if ((f.flags & 3) == 3) vatomic(base, k + dy + HEXC * 4u, f.a11);
}
// The walker's ONE remembered footprint (round 4; rounds 1-3 walked every level in the finest level's order and needed a two-entry
// cache with an MRU bit because foreign cell boundaries made the points alternate between two footprints -- removed in round 5,
// tools/sim/flush_orders.py still prices both).  A walk that is monotone in its OWN level's cells enters a footprint once.
//   hit   (three calls in four): no load at all -- the entry keeps the texel VALUES of its corners next to the partial sums; the
//         sample the footprint produced in the forward is re-derived from them and dL/ds = T / s is accumulated;
//   miss  (uniform inside the walker's lanes): the four (two) texels of the new footprint are loaded, and
//         evict  the old entry is flushed (up to 4 atomics) and restarts empty, or
//         shift  the new footprint is one row BELOW / one column RIGHT of the old one -- the usual step of a walk along the minor
//                axis: two of its texels are already being summed, only the row / column left behind is flushed (2 atomics
//                instead of 4 -- the walk is bound by the rate of atomic line-ops) and the other two sums move up.
// ROW = true: the plane is a height-1 row table (uniform time): only the nw / ne corners exist.
// An out-of-range corner has weight exactly 0 and takes the nw texel's value, like the per-point pass; a sample that is not safely
// divisible contributes nothing here (the per-point pass scattered it exactly: same predicate, same bits).
// Round 6: the corners live in PAIRS (nw, ne) / (sw, se) so that the hit path -- which three calls in four take, and on which the
// kernel is VALU-issue-bound (SQ_INSTS_VALU: 0.83 of its time in round 5) -- runs on packed fp32 instructions: the four products of
// the sample as two v_pk_mul_f32, the four accumulations as two v_pk_fma_f32.  Same values bit for bit: the products are rounded
// one by one and added in the order ((p00 + p01) + p10) + p11 exactly as before (the forward's order), an fma per corner as before.
struct Foot1 {
  int key;            // (texel index << 2 | corner flags), -1 = empty
  f2v_ a01, a23;      // partial sums of the footprint's corners (nw, ne) (sw, se)
  f2v_ v01, v23;      // texel values of the corners
};
__device__ __forceinline__ void foot1_init(Foot1& F) {
  F.key = -1;
  F.a01 = f2v_{0.f, 0.f};
  F.a23 = f2v_{0.f, 0.f};
}
struct PackedTap2 {   // one tap as the walker reads it back from LDS: 8 floats (32 bytes)
  int kf;             // texel index of the nw corner << 2 | flags (bit 0: ne / se column in range, bit 1: sw / se row in range)
  f2v_ w01, w23;      // bilinear weights of (nw, ne) (sw, se)
};
// hit path: re-derive the sample of tap `t` from the remembered texel values, add dL/ds = tv / s to the footprint's sums
template <bool ROW>
__device__ __forceinline__ void foot1_accumulate(Foot1& F, const PackedTap2& t, float tv) {
  const f2v_ p01 = F.v01 * t.w01;
  float sv = p01.x + p01.y;
  if (!ROW) {
    const f2v_ p23 = F.v23 * t.w23;
    sv = sv + p23.x;
    sv = sv + p23.y;
  }
  const float g = tslab_divisible(sv) ? tv * __builtin_amdgcn_rcpf(sv) : 0.f;
  const f2v_ gg = f2v_{g, g};
  F.a01 = __builtin_elementwise_fma(gg, t.w01, F.a01);
  if (!ROW) F.a23 = __builtin_elementwise_fma(gg, t.w23, F.a23);
}
// ---- deterministic mode (round 6, opt-in: s3g_hexplane_set_deterministic) ---------------------------------------------------------
// Plane gradients that are bit-identical from run to run need (1) walk orders that do not depend on the timing of LDS atomics (the
// stable counting sorts of hexplane_sort.hip), (2) ONE writer per sum, and (3) a fixed order in which the sums of a texel are added.  The walk keeps
// its structure -- segments of seg_len sorted points per walker, one remembered footprint -- but a finished footprint ("run": the
// consecutive points of one cell inside one segment) is STORED, not added with atomics:
//   CELL[cell][corner][32]   the run that contains the cell's first point (cells are contiguous in the order: exactly one such run),
//   SEG[segment][corner][32] the first run of a segment when it continues a cell begun in an earlier segment (at most one per segment),
// and hexplane_stencil_kernel adds, for every texel, the four cells around it (nw of its own cell, ne of the cell to the left, sw of
// the cell above, se of the cell above-left), each as CELL + its SEG continuations in segment order.  The walkers also leave the index
// the stencil needs: cstart[cell] (written by whoever meets the cell's first point) and segcell[segment] (which cell a segment's first
// run continues: the walker compares its first point's cell with the cell of the point just before its segment).  No shift reuse here:
// every cell keeps its own four sums.  (A first version derived the cell extents in a kernel of its own -- two sort_cell evaluations
// per sorted position and walk through the order's indirection: 0.62 ms; the walk knows them for free.)
template <bool ROW>
__device__ __forceinline__ void det_store_run(const Foot1& F, const DetWalk& dw, int seg, bool continuation, int c) {
  if (F.key < 0) return;
  const int cellid = F.key >> 2;
  constexpr int NC = ROW ? 2 : 4;
  float* rec = continuation ? (ROW ? dw.tseg : dw.seg) + (size_t)seg * (NC * HEXC) : (ROW ? dw.tcell : dw.cell) + (size_t)cellid * (NC * HEXC);
  rec[c] = F.a01.x;
  rec[HEXC + c] = F.a01.y;
  if (!ROW) {
    rec[2 * HEXC + c] = F.a23.x;
    rec[3 * HEXC + c] = F.a23.y;
  }
}
// the deterministic walker's tap: like foot1_add_t, but a finished footprint is stored as a run record and nothing is shifted.
// cont: the run being accumulated is the segment's first AND continues the cell of the point before the segment (prev_kf);
// kpos: sorted position of this point.
template <bool ROW>
__device__ __forceinline__ void foot1_add_det(Foot1& F, bool& cont, int prev_kf, int kpos, const PackedTap2& t, float tv, const DetWalk& dw, int seg,
                                              const float* __restrict__ pl, int W, int c) {
  const int tkf = t.kf;
  if (tkf != F.key) {
    const int tkey = tkf >> 2, tfl = tkf & 3;
    const float* px = pl + (size_t)tkey * HEXC;
    const float n0 = px[0], n1 = px[(tfl & 1) ? HEXC : 0];
    float n2 = 0.f, n3 = 0.f;
    if (!ROW) {
      n2 = px[(tfl & 2) ? (size_t)W * HEXC : 0];
      n3 = px[(tfl == 3) ? (size_t)W * HEXC + HEXC : 0];
    }
    const bool opening = F.key < 0;                 // the segment's first footprint
    if (!opening) det_store_run<ROW>(F, dw, seg, cont, c);
    cont = opening && tkf == prev_kf;
    if (c == 0) {
      if (opening) (ROW ? dw.tsegcell : dw.segcell)[seg] = cont ? tkey : -1;
      if (!cont) (ROW ? dw.tstart : dw.cstart)[tkey] = (uint32_t)kpos;       // this point is the first of its cell
    }
    F.a01 = f2v_{0.f, 0.f};
    F.v01 = f2v_{n0, n1};
    if (!ROW) {
      F.a23 = f2v_{0.f, 0.f};
      F.v23 = f2v_{n2, n3};
    }
    F.key = tkf;
  }
  foot1_accumulate<ROW>(F, t, tv);
}

template <bool ROW = false>
__device__ __forceinline__ void foot1_add_t(Foot1& F, const PackedTap2& t, float tv, float* __restrict__ gp,
                                            const float* __restrict__ pl /* plane values + channel */, int W, int c) {
  const int tkf = t.kf;
  if (tkf != F.key) {  // miss (uniform inside the walker's lanes)
    const int tkey = tkf >> 2, tfl = tkf & 3;
    const float* px = pl + (size_t)tkey * HEXC;
    const float n0 = px[0], n1 = px[(tfl & 1) ? HEXC : 0];
    float n2 = 0.f, n3 = 0.f;
    if (!ROW) {
      n2 = px[(tfl & 2) ? (size_t)W * HEXC : 0];
      n3 = px[(tfl == 3) ? (size_t)W * HEXC + HEXC : 0];
    }
    const int KF = F.key, K = KF >> 2, FL = KF & 3;
    const bool down = !ROW && KF >= 0 && tkey == K + W;
    const bool right = KF >= 0 && tkey == K + 1 && (FL & 1);
    const bool shift = down || right;
    const float A0 = F.a01.x, A1 = F.a01.y, A2 = ROW ? 0.f : F.a23.x, A3 = ROW ? 0.f : F.a23.y;
    if (KF >= 0) {
      const uint32_t k = ((uint32_t)K * HEXC + (uint32_t)c) * 4u;
      const uint32_t dy = (uint32_t)W * (HEXC * 4u);
      char* base = reinterpret_cast<char*>(gp);
      vatomic(base, k, A0);                                                    // nw leaves in every case
      if ((FL & 1) && !right) vatomic(base, k + HEXC * 4u, A1);               // ne stays when shifting right
      if (!ROW && (FL & 2) && !down) vatomic(base, k + dy, A2);               // sw stays when shifting down
      if (!ROW && (FL & 3) == 3 && !shift) vatomic(base, k + dy + HEXC * 4u, A3);
    }
    // new contents: shift down (nw, ne, sw, se) <- (sw, se, 0, 0); shift right <- (ne, 0, se, 0); evict <- 0
    F.a01 = f2v_{down ? A2 : (right ? A1 : 0.f), down ? A3 : 0.f};
    F.v01 = f2v_{n0, n1};
    if (!ROW) {
      F.a23 = f2v_{right ? A3 : 0.f, 0.f};
      F.v23 = f2v_{n2, n3};
    }
    F.key = tkf;
  }
  foot1_accumulate<ROW>(F, t, tv);
}
template <bool ROW = false>
__device__ __forceinline__ void foot1_flush_all(const Foot1& F, float* __restrict__ gp, int W, int c) {
  if (F.key < 0) return;
  foot_flush(Foot{F.key >> 2, ROW ? (F.key & 1) : (F.key & 3), F.a01.x, F.a01.y, ROW ? 0.f : F.a23.x, ROW ? 0.f : F.a23.y}, gp, W, c);
}

// A WALKER = 32 lanes (one per channel: a half-wave) walks seg_len consecutive points of ONE (orientation, level) order:
// blockIdx.y = orientation * levels + level.  The taps are computed by the walker's lanes for a whole GROUP of points at once
// (lane = point q x tap j), parked in LDS, and every lane reads them back with broadcast loads while it accumulates its channel.
// Round 6: groups of SIXTEEN points (rounds 1-5: four).  make_tap + the coordinate / index loads are ~60 wave-instructions whoever
// needs them; with 8 of a walker's 32 lanes busy they cost 15 per point, a quarter of everything the kernel issued -- with all 32
// lanes busy they cost 4.  The T rows are still requested four points at a time, one batch ahead of their use (their addresses
// come out of the same LDS records: the point's position in the processing order rides in the tap's spare slot).
// (Removed in round 5, measured slower in rounds 2-4: two levels per walk, two channels per lane with v_pk_fma -- twice the flush
// atomics, 2.07 vs 1.14 ms --, the two-entry footprint cache, 512- and 1024-point segments: DESIGN.md section 10.)
#ifndef S3G_HEX_SCATTER_WAVES
#define S3G_HEX_SCATTER_WAVES 6   // waves per SIMD the register budget is set for
#endif
constexpr int TAPF = 8;   // floats per packed tap in LDS: key, flags, w00, w01 | w10, w11, position of the point's T rows, -
constexpr int GRP = 16;   // points per tap group
__device__ __forceinline__ float load_g(const float* p) { return __builtin_nontemporal_load(p); }   // streaming loads of the T rows: 1.28 -> 1.23 ms
template <bool UT, bool DET = false>   // UT: uniform time -- the (axis, t) planes are height-1 row tables; DET: deterministic mode (needs UT)
__global__ void __launch_bounds__(256, UT ? S3G_HEX_SCATTER_WAVES : S3G_HEX_SCATTER_WAVES - 1) hexplane_scatter_kernel(const HexArgs a, const float* __restrict__ G,
                                                               const uint32_t* __restrict__ order_all, const uint32_t* __restrict__ comp_all,
                                                               const DetWork detw) {
  constexpr int LANES = HEXC, WALKERS = 256 / LANES;
  constexpr int NTAP = 2;             // taps per point and walk: the orientation's spatial plane and its (major, t) plane
  static_assert(LANES == GRP * NTAP, "tap phase: one lane per (point of the group, tap)");
  __shared__ __attribute__((aligned(16))) float tapbuf[WALKERS][2][GRP][NTAP][TAPF];  // [walker][double buffer][point][tap]: 16 KiB
  const int oi = blockIdx.y;
  if (!((a.walk_mask >> oi) & 1u)) return;
  const int o = oi / a.d.levels, lv = oi % a.d.levels;
  const int c = threadIdx.x & (LANES - 1), hw = threadIdx.x / LANES;   // channel of this lane, walker of this half-wave
  const int q = c / NTAP, j = c % NTAP;  // tap-phase role: point q of the group, tap j (0 spatial, 1 time plane)
  const int seg = blockIdx.x * WALKERS + hw;
  const int k0 = seg * a.seg_len, k1 = min(a.P, k0 + a.seg_len);
  if (k0 >= a.P) return;  // whole walkers drop out; the LDS traffic below is private to a walker (wave-ordered)
  const uint32_t* order = order_all + (size_t)oi * a.P;
  const uint32_t* comp = comp_all + (size_t)oi * a.P;
  const size_t GP = (size_t)(a.d.levels * HEXC);   // point-major T rows: floats per point
  const int i0 = PLA[o], i1 = PLT[o];
  const int ip = j ? i1 : i0;                         // the plane of this lane's tap
  const int axw = PAIR0[ip], axh = PAIR1[ip];
  Foot1 f1[2];
  foot1_init(f1[0]);
  foot1_init(f1[1]);
  bool cont[2] = {false, false};      // deterministic mode: the open run is the segment's first and continues an earlier segment's cell
  int prev_kf[2] = {-2, -2};          // deterministic mode: hit key (texel << 2 | flags) of the point just before the segment, per tap
  const int Wt = a.d.res[lv][axw], Ht = a.d.res[lv][axh];
  // uniform per workgroup; read ONCE (indexed kernel-argument reads inside the loop were an s_load + s_waitcnt lgkmcnt(0) per tap,
  // i.e. every tap also waited for all of the wave's outstanding LDS reads)
  float* const gp0 = a.gplanes[lv][i0];
  float* const gp1 = a.gplanes[lv][i1];
  const float* const pl0 = a.d.planes[lv][i0] + c;
  const float* const pl1 = a.d.planes[lv][i1] + c;
  const int W0 = a.d.res[lv][PAIR0[i0]], W1 = a.d.res[lv][PAIR0[i1]];
  const float* Grow = G + (size_t)(lv * HEXC + c);    // this lane's column of every T row
  // Software pipeline per lane role (point q of a group, tap j): the sorted index (and T-row position) of group g+2, the
  // coordinates of group g+1 and the taps of group g+1 are produced while group g is accumulated, so neither the
  // index -> position load chain nor the tap arithmetic sits between a group's T loads and their use.
  auto slot_of = [&](int kb) { return min(kb + q, k1 - 1); };
  auto store_taps = [&](const float* u, uint32_t cpos, int buf) {
    const Tap t = make_tap(u[axw], u[axh], Wt, Ht);
    float* dst = &tapbuf[hw][buf][q][j][0];
    // slot 0: (texel index << 2 | corner flags) -- the word the hit test compares; a plane has at most 2^24 texels (check_desc)
    *reinterpret_cast<float4*>(dst) = make_float4(__int_as_float((t.o00 << 2) | (t.o01 >= 0 ? 1 : 0) | (t.o10 >= 0 ? 2 : 0)), 0.f, t.w00, t.w01);
    *reinterpret_cast<float4*>(dst + 4) = make_float4(t.w10, t.w11, __uint_as_float(cpos), 0.f);
  };
  auto row_pos = [&](int buf, int qq) { return __float_as_uint(tapbuf[hw][buf][qq][0][6]); };
  if (DET && k0 > 0) {               // lane j of the walker (q == 0) evaluates tap j of the previous point; broadcast inside the half-wave
    float up[4];
    point_coords(a, (int)order[k0 - 1], up);
    const Tap tp = make_tap(up[axw], up[axh], Wt, Ht);
    const int kfp = (tp.o00 << 2) | (tp.o01 >= 0 ? 1 : 0) | (tp.o10 >= 0 ? 2 : 0);
    prev_kf[0] = __shfl(kfp, (int)(threadIdx.x & 32u));
    prev_kf[1] = __shfl(kfp, (int)(threadIdx.x & 32u) + 1);
  }
  float un[4];                       // coordinates of the NEXT group's point
  uint32_t cn;                       // ... and the position of its T rows
  {
    float u0[4];
    const int s0 = slot_of(k0);
    point_coords(a, (int)order[s0], u0);
    store_taps(u0, comp[s0], 0);
  }
  {
    const int s1 = slot_of(k0 + GRP);
    point_coords(a, (int)order[s1], un);
    cn = comp[s1];
  }
  int snn = slot_of(k0 + 2 * GRP);
  int pnn = (int)order[snn];         // index of the group after next
  uint32_t cnn = comp[snn];
  wave_lds_sync();
  // the first batch of T rows (four points; ONE row per point and level: T = dL/dfeature * feature -- both planes of the walk
  // divide it by their sample)
  float g[4], gn[4];
#pragma unroll
  for (int qq = 0; qq < 4; qq++) g[qq] = load_g(Grow + (size_t)row_pos(0, qq) * GP);
  int buf = 0;
  for (int kb = k0; kb < k1; kb += GRP, buf ^= 1) {
    // 1. the NEXT group's taps from coordinates loaded one iteration ago; then advance the two prefetch stages
    store_taps(un, cn, buf ^ 1);
    point_coords(a, pnn, un);
    cn = cnn;
    snn = slot_of(kb + 3 * GRP);
    pnn = (int)order[snn];
    cnn = comp[snn];
    wave_lds_sync();
    // 2. accumulate this group, four points at a time; each batch first requests the T rows of the batch after it
#pragma unroll 1     // (rolled on purpose: every copy of the body carries eight inlined miss paths)
    for (int sb = 0; sb < GRP / 4; sb++) {
#pragma unroll
      for (int qq = 0; qq < 4; qq++)
        gn[qq] = load_g(Grow + (size_t)row_pos(sb == GRP / 4 - 1 ? buf ^ 1 : buf, (4 * (sb + 1) + qq) % GRP) * GP);
      const int nq = k1 - kb - 4 * sb;       // points left from this batch on (<= 0: nothing)
#pragma unroll
      for (int qq = 0; qq < 4; qq++) {
        if (qq >= nq) break;
#pragma unroll
        for (int m = 0; m < 2; m++) {
          float* gp = m ? gp1 : gp0;
          if (gp == nullptr) continue;
          const float* src = &tapbuf[hw][buf][4 * sb + qq][m][0];
          const float4 lo = *reinterpret_cast<const float4*>(src);
          PackedTap2 t;
          t.kf = __float_as_int(lo.x);
          t.w01 = f2v_{lo.z, lo.w};
          if (DET) {
            const int kpos = kb + 4 * sb + qq;
            if (m == 1) {
              foot1_add_det<true>(f1[1], cont[1], prev_kf[1], kpos, t, g[qq], detw.walk[oi], seg, pl1, W1, c);
            } else {
              const float2 hi = *reinterpret_cast<const float2*>(src + 4);
              t.w23 = f2v_{hi.x, hi.y};
              foot1_add_det<false>(f1[0], cont[0], prev_kf[0], kpos, t, g[qq], detw.walk[oi], seg, pl0, W0, c);
            }
          } else if (UT && m == 1) {
            foot1_add_t<true>(f1[m], t, g[qq], gp, pl1, W1, c);
          } else {
            const float2 hi = *reinterpret_cast<const float2*>(src + 4);
            t.w23 = f2v_{hi.x, hi.y};
            foot1_add_t<false>(f1[m], t, g[qq], gp, m ? pl1 : pl0, m ? W1 : W0, c);
          }
        }
      }
#pragma unroll
      for (int qq = 0; qq < 4; qq++) g[qq] = gn[qq];
    }
  }
#pragma unroll
  for (int m = 0; m < 2; m++) {
    float* gp = m ? gp1 : gp0;
    if (gp == nullptr) continue;
    if (DET) {
      if (m == 1) det_store_run<true>(f1[1], detw.walk[oi], seg, cont[1], c);
      else det_store_run<false>(f1[0], detw.walk[oi], seg, cont[0], c);
    } else if (UT && m == 1) foot1_flush_all<true>(f1[m], gp, W1, c);
    else foot1_flush_all<false>(f1[m], gp, m ? W1 : W0, c);
  }
}

// ---- deterministic mode: the stencil gather ---------------------------------------------------------------------------------------
// sum of one cell's run records for corner `corner`, lane = channel: CELL first, then the SEG continuations in segment order
template <int NC>
__device__ __forceinline__ float det_cell_sum(const float* __restrict__ cellrec, const float* __restrict__ segrec, const uint32_t* __restrict__ cs,
                                              const int* __restrict__ segcell, int cellid, int corner, int seg_len, int nseg, int c) {
  const uint32_t s0 = cs[cellid];
  if (s0 == 0xffffffffu) return 0.f;
  float acc = cellrec[(size_t)cellid * (NC * HEXC) + corner * HEXC + c];
  for (int sg = (int)(s0 / (uint32_t)seg_len) + 1; sg < nseg && segcell[sg] == cellid; sg++)
    acc += segrec[(size_t)sg * (NC * HEXC) + corner * HEXC + c];
  return acc;
}
// grid = (texel groups, walks): a half-wave (lane = channel) per texel of the walk's spatial plane; the row tables' 1-D stencil rides in
// the same launch (texels 0 .. Wmajor-1 of an extra "row" behind the plane).
__global__ void __launch_bounds__(256) hexplane_stencil_kernel(const HexArgs a, const DetWork detw) {
  const int oi = blockIdx.y, o = oi / a.d.levels, lv = oi % a.d.levels;
  if (!((a.walk_mask >> oi) & 1u)) return;
  const int c = threadIdx.x & (HEXC - 1);
  const int ip = PLA[o], it = PLT[o];
  const int Wx = a.d.res[lv][PAIR0[ip]], Wy = a.d.res[lv][PAIR1[ip]], Wm = a.d.res[lv][MAJ[o]];
  const int t = blockIdx.x * (256 / HEXC) + threadIdx.x / HEXC;
  const int sl = a.seg_len, nseg = (a.P + sl - 1) / sl;
  const DetWalk dw = detw.walk[oi];
  if (t < Wx * Wy) {
    float* gp = a.gplanes[lv][ip];
    if (gp == nullptr) return;
    const int x = t % Wx, y = t / Wx;
    // the four cells around the texel, in the fixed order nw (own cell), ne (left), sw (above), se (above-left).  Three rounds of
    // independent loads -- starts, then records + the next segment's link, then (rarely) continuation records -- instead of four
    // dependent chains one after the other: the pass is latency-bound (0.65 -> see profiles/r06_hex_deterministic.txt)
    const int cid[4] = {t, t - 1, t - Wx, t - Wx - 1};
    const bool ok[4] = {true, x > 0, y > 0, x > 0 && y > 0};
    uint32_t s0[4];
#pragma unroll
    for (int k = 0; k < 4; k++) s0[k] = ok[k] ? dw.cstart[cid[k]] : 0xffffffffu;
    float v[4];
    int nxt[4], link[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const bool have = s0[k] != 0xffffffffu;
      v[k] = have ? dw.cell[(size_t)cid[k] * (4 * HEXC) + k * HEXC + c] : 0.f;
      nxt[k] = have ? (int)(s0[k] / (uint32_t)sl) + 1 : nseg;
      link[k] = nxt[k] < nseg ? dw.segcell[nxt[k]] : -1;
    }
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      float part = v[k];
      int sg = nxt[k], lk = link[k];
      while (sg < nseg && lk == cid[k]) {          // the cell straddles segments: its continuation records, in segment order
        part += dw.seg[(size_t)sg * (4 * HEXC) + k * HEXC + c];
        sg++;
        lk = sg < nseg ? dw.segcell[sg] : -1;
      }
      acc += part;
    }
    gp[(size_t)t * HEXC + c] += acc;
  } else if (t < Wx * Wy + Wm) {
    float* gt = a.gplanes[lv][it];       // (uniform time: the row table's gradient, folded back into the plane rows afterwards)
    if (gt == nullptr) return;
    const int x = t - Wx * Wy;
    float acc = det_cell_sum<2>(dw.tcell, dw.tseg, dw.tstart, dw.tsegcell, x, 0, sl, nseg, c);
    if (x > 0) acc += det_cell_sum<2>(dw.tcell, dw.tseg, dw.tstart, dw.tsegcell, x - 1, 1, sl, nseg, c);
    gt[(size_t)x * HEXC + c] += acc;
  }
}

// One launch for the 3 * levels walks (blockIdx.y = orientation * levels + level), a walker per a.seg_len sorted points.
int hexplane_scatter_launch(const HexArgs& a, const float* G, const SortWork& w, int det, const DetWork& detw, void* det_index,
                            size_t det_index_bytes, hipStream_t stream) {
  constexpr int walkers = 256 / HEXC;
  const int NW = n_walk_orders(a.d.levels), nseg = (a.P + a.seg_len - 1) / a.seg_len;
  const dim3 grid((nseg + walkers - 1) / walkers, NW);
  profile_begin(S3G_PROFILE_HEXPLANE_SCATTER, stream);
  if (det) {
    // run records + cell index by the walk (no atomics), then one stencil gather per texel
    S3G_HIP_CHECK(hipMemsetAsync(det_index, 0xff, det_index_bytes, stream));     // cstart / tstart: ~0u = empty cell
    hipLaunchKernelGGL((hexplane_scatter_kernel<true, true>), grid, dim3(256), 0, stream, a, G, w.order, w.comp, detw);
    int maxt = 0;
    for (int l = 0; l < a.d.levels; l++)
      for (int o = 0; o < 3; o++) {
        size_t cells, wm;
        walk_cells(&a.d, o, l, &cells, &wm);
        maxt = max(maxt, (int)(cells + wm));
      }
    hipLaunchKernelGGL(hexplane_stencil_kernel, dim3((maxt + walkers - 1) / walkers, NW), dim3(256), 0, stream, a, detw);
  } else if (a.d.uniform_time)
    hipLaunchKernelGGL((hexplane_scatter_kernel<true>), grid, dim3(256), 0, stream, a, G, w.order, w.comp, detw);
  else
    hipLaunchKernelGGL((hexplane_scatter_kernel<false>), grid, dim3(256), 0, stream, a, G, w.order, w.comp, detw);
  profile_end(S3G_PROFILE_HEXPLANE_SCATTER, stream, (double)a.P, (double)a.d.levels);
  return S3G_OK;
}

}  // namespace s3g
