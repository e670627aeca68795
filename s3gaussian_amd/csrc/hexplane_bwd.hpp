// What the files of the HexPlane backward share: hexplane_point.hip, hexplane_sort.hip, hexplane_scatter.hip and the orchestration
// in hexplane.hip.  Private to libs3g.so (not part of the C ABI).
#pragma once
#include "hexplane_dev.hpp"

namespace s3g {

// G slab contents: ONE row per level,
// T = dL/dfeature * feature = g * prod_j s_j (the per-point pass has it for free at the end of its product rule); the scatter
// walk re-derives the one sample it is about to scatter -- the four texels (two row-table entries) of the footprint it is
// accumulating anyway, L1-resident in the sorted order -- and uses dL/ds_i = T / s_i.  512 B per point written instead of
// 3 KB, 1.5 KB read back instead of 3 KB.  A sample whose magnitude is not safely divisible (|s| <= 1e-18, or not finite) is
// left out by the walk and scattered EXACTLY (g * prod_{j != i} s_j, direct atomics) by the per-point pass, which has all six
// samples: both passes evaluate the same predicate on the same bits of s (same taps, same operation order, contraction off).
// One walk order per orientation AND level: each (orientation, level) walk is monotone in its own cells (see sort_cell below).
constexpr float TSLAB_SAFE = 1e-18f;
__device__ __forceinline__ bool tslab_divisible(float s) { return fabsf(s) > TSLAB_SAFE && fabsf(s) < __builtin_huge_valf(); }
// GATE of the exact fallback in the per-point passes: wider than the predicate itself.  The passes that DIVIDE decide with
// tslab_divisible on the sample they re-derive; the fallback (tslab_exact_scatter / exact_du) re-derives the sample the same way and
// applies the same predicate per channel.  The gate only has to make sure the fallback is ENTERED whenever some pass might refuse
// to divide: a sample within a factor of four of the threshold enters it even if this kernel's own evaluation sits on the safe side.
__device__ __forceinline__ bool tslab_near_unsafe(float s) { return !(fabsf(s) > 4.f * TSLAB_SAFE && fabsf(s) < __builtin_huge_valf()); }

// ---- sort: point indices ordered by (major cell, minor cell) on a 512 x 512 grid, per orientation ----
// orientation o: major axis MAJ[o], minor axis MIN_[o]; handles planes PLA[o] (spatial) and PLT[o] (the major axis vs time)
constexpr int SORT_BINS = 512, SORT_NB = 256;
__device__ constexpr int MAJ[3] = {0, 1, 2};
__device__ constexpr int MIN_[3] = {1, 2, 0};
__device__ constexpr int PLA[3] = {0, 3, 1};  // (x,y) (y,z) (x,z)
__device__ constexpr int PLT[3] = {2, 4, 5};  // (x,t) (y,t) (z,t)

// Sort cell of a point along `axis` = its texel column at level `level`, computed exactly like make_tap does, so all points of
// one cell share their four corner texels at that level.
// Round 4: ONE ORDER PER (orientation, LEVEL).  Rounds 1-3 walked every level in the finest level's cell order: align_corners
// grids of different levels do not nest, a coarse footprint is then re-entered once per fine row that crosses it (eight times at
// level 0) and alternates at every cut -- which is what the two-entry footprint cache was for.  Counted on the bench's own point
// cloud with the cache modelled statement by statement (tools/sim/flush_orders.py): 5.9 M line-atomics per backward in the finest
// order against 2.4 M when every (orientation, level) is walked in ITS OWN cells' order (floor: 1.03 M distinct footprints x 2-4
// corners); measured before that: 7.9 M, i.e. ~0.8 ms of a 1.43 ms kernel at the 10 G line-ops/s the chip retires.
__device__ __forceinline__ int sort_cell(const HexArgs& a, int p, int axis, int level) {
  const float u = (a.xyz[3 * (size_t)p + axis] - a.d.aabb_max[axis]) * (2.0f / (a.d.aabb_min[axis] - a.d.aabb_max[axis])) - 1.0f;
  const int W = a.d.res[level][axis];
  float ix = ((u + 1.f) / 2.f) * (float)(W - 1);
  ix = fminf((float)(W - 1), fmaxf(ix, 0.f));
  int cidx = (int)floorf(ix);
  if (W > SORT_BINS) cidx = (int)(((long long)cidx * SORT_BINS) / W);
  return min(SORT_BINS - 1, max(0, cidx));
}

// Order ids: oi = orientation * levels + level for the 3 * levels walk orders, oi = 3 * levels for the processing order.
static inline int n_walk_orders(int levels) { return 3 * levels; }
static inline int n_orders(int levels) { return n_walk_orders(levels) + 1; }

struct SortWork {
  uint32_t* table;      // [NO][SORT_NB][SORT_BINS]      NO = n_orders(levels), NW = n_walk_orders(levels) = NO - 1
  uint32_t* seg_start;  // [NO][SORT_BINS + 1]
  uint32_t* tmp;        // [NO][P]  indices grouped by major key
  uint32_t* order;      // [NW][P]  final orders of the walks: oi = orientation * levels + level
  uint32_t* comp;       // [NW][P]  comp[oi][k] = position of point order[oi][k] in the processing order (where its T rows are)
  uint32_t* proc;       // [P]      the last order: processing order of the per-point passes
  int nw;               // NW
};

// sorted points walked by one half-wave (HexArgs::seg_len): longer segments flush fewer footprints at their ends, shorter ones
// give more half-waves; 256 measured best at 1.2 M points (1.21 vs 1.30 ms), 128 below a million
static inline int segment_length(int P) { return P >= 1000000 ? 256 : 128; }

// Deterministic mode (design: hexplane_scatter.hip): the records and index of one (orientation, level) walk, carved by hexplane.hip
struct DetWalk {           // one (orientation, level) walk
  uint32_t* cstart;        // [cells] sorted position of the spatial cell's first point (cell id = plane texel index of its nw corner); ~0u: empty
  uint32_t* tstart;        // [Wmajor] the same for the 1-D cells of the (major, t) row table
  int* segcell;            // [segments] the cell the segment's FIRST run continues from an earlier segment, -1 if it opens its cell itself
  int* tsegcell;
  float* cell;             // [cells][4][32]
  float* seg;              // [segments][4][32]
  float* tcell;            // [Wmajor][2][32]
  float* tseg;             // [segments][2][32]
};
struct DetWork {
  DetWalk walk[3 * S3G_HEX_MAX_LEVELS];
};
// spatial cells (texels of the orientation's spatial plane) and major width (cells of its (major, t) row table) of walk (o, l)
static inline void walk_cells(const s3g_hexplane_desc* d, int o, int l, size_t* cells, size_t* wm) {
  static const int PLA_H[3] = {0, 3, 1}, MAJ_H[3] = {0, 1, 2};
  *cells = (size_t)d->res[l][PAIR0_HOST[PLA_H[o]]] * d->res[l][PAIR1_HOST[PLA_H[o]]];
  *wm = (size_t)d->res[l][MAJ_H[o]];
}

// ---- host functions that cross files (a __global__ function is launched only from the file that defines it) --------------------------
// the 3 * levels walk orders, the processing order and comp[][] into `w` (det: stable placement)
int hexplane_sort_launch(const HexArgs& a, const SortWork& w, int det, hipStream_t stream);
// pass A in a.proc_order: dL/dxyz and the T rows -> G; `algorithm` S3G_HEX_SLAB_DIV reads the forward's `features`
int hexplane_point_launch(const HexArgs& a, const float* features, int algorithm, float* G, hipStream_t stream);
// pass B: the walks over w.order / w.comp; det: run records into `detw` (cell index at det_index 0xff-filled first), stencil gather
int hexplane_scatter_launch(const HexArgs& a, const float* G, const SortWork& w, int det, const DetWork& detw, void* det_index,
                            size_t det_index_bytes, hipStream_t stream);

}  // namespace s3g
