// HexPlane backward (overview: hexplane.hip): the counting sorts behind the walk orders and the processing order.
#include "hexplane_bwd.hpp"

namespace s3g {

// The LAST order is the PROCESSING order of the per-point passes (forward, backward pass A): a two-level 3-D blocking -- major
// key = the 8 x 8 x 8 grid of blocks of the volume, minor key = the 8 x 8 x 8 sub-blocks of a block -- so that consecutive
// points are close in x, y AND z and all three spatial planes' texels stay in the L2 of the XCD that works on the block.
// (In an (x, y) order every tap of the (y, z) plane missed: 2.5 GB of 128-byte fetches per pass at 1.2 M points.)
__device__ __forceinline__ int block_key(const HexArgs& a, int p, int shift) {
  int key = 0;
#pragma unroll
  for (int axis = 0; axis < 3; axis++) {
    const int Wc = min(a.d.res[a.d.levels - 1][axis], SORT_BINS);
    const int c = sort_cell(a, p, axis, a.d.levels - 1);
    key = key * 8 + (min(63, (c * 64) / Wc) >> shift & 7);
  }
  return key;
}
__device__ __forceinline__ int order_key(const HexArgs& a, int p, int oi, bool major) {
  const int nw = 3 * a.d.levels;
  if (oi >= nw) return block_key(a, p, major ? 3 : 0);
  const int o = oi / a.d.levels, level = oi % a.d.levels;
  return sort_cell(a, p, major ? MAJ[o] : MIN_[o], level);
}
__device__ __forceinline__ uint32_t* order_of(const SortWork& w, int o, int P) { return o < w.nw ? w.order + (size_t)o * P : w.proc; }

// STABLE placement (round 6, deterministic mode): the position of an element among the elements of its key must not depend on the
// order in which LDS atomics happen to execute.  One round = 256 consecutive elements.  Every wave ranks its lanes per key with one
// ballot per distinct key (registers only), the per-(wave, key) group sizes meet in LDS, and an element's position is
// base[key] + the groups of the earlier waves + its rank: the elements of a key keep their input order.  The bases advance by integer
// atomics (order-independent).  All four waves work in parallel: three barriers per round.  (The first version let the waves take
// turns, with the base read and written inside the ballot loop: 2.6 ms per re-sort against 0.8 ms for the unstable sort.)
// wcnt: [4][SORT_BINS] words of LDS, zero on entry, left zero.  Every thread of the workgroup calls this; inactive lanes pass active = false.
__device__ __forceinline__ uint32_t stable_claim(uint32_t* __restrict__ cell, uint32_t* __restrict__ wcnt, int key, bool active) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t rank = 0, total = 0;
  bool leader = false;
  uint64_t remaining = __ballot(active);
  while (remaining) {   // uniform across the wave
    const int first = __ffsll((long long)remaining) - 1;
    const int k = __shfl(key, first);
    const bool mine = active && key == k;
    const uint64_t same = __ballot(mine);
    if (mine) {
      rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
      total = (uint32_t)__popcll(same);
      leader = lane == first;
    }
    remaining &= ~same;
  }
  if (leader) wcnt[wave * SORT_BINS + key] = total;
  __syncthreads();
  uint32_t pos = 0;
  if (active) {
    pos = cell[key] + rank;
    for (int w = 0; w < wave; w++) pos += wcnt[w * SORT_BINS + key];
  }
  __syncthreads();
  if (leader) {
    atomicAdd(&cell[key], total);          // integer: the result does not depend on the order
    wcnt[wave * SORT_BINS + key] = 0u;
  }
  __syncthreads();
  return pos;
}

template <bool WRITE>
__global__ void __launch_bounds__(256) hexsort_major_kernel(const HexArgs a, const SortWork w, int chunk, int stable) {
  __shared__ uint32_t cell[SORT_BINS];
  __shared__ uint32_t wcnt[4 * SORT_BINS];
  if (WRITE && stable)
    for (int i = threadIdx.x; i < 4 * SORT_BINS; i += 256) wcnt[i] = 0u;
  const int o = blockIdx.y;
  uint32_t* row = w.table + ((size_t)o * SORT_NB + blockIdx.x) * SORT_BINS;
  for (int i = threadIdx.x; i < SORT_BINS; i += 256) cell[i] = WRITE ? w.seg_start[o * (SORT_BINS + 1) + i] + row[i] : 0u;
  __syncthreads();
  const int g0 = blockIdx.x * chunk, g1 = min(a.P, g0 + chunk);
  if (WRITE && stable) {
    for (int gb = g0; gb < g1; gb += 256) {      // uniform trip count: stable_claim synchronises the workgroup
      const int g = gb + threadIdx.x;
      const bool act = g < g1;
      const uint32_t pos = stable_claim(cell, wcnt, act ? order_key(a, g, o, true) : 0, act);
      if (act) w.tmp[(size_t)o * a.P + pos] = (uint32_t)g;
    }
    return;
  }
  for (int g = g0 + threadIdx.x; g < g1; g += 256) {
    const uint32_t pos = atomicAdd(&cell[order_key(a, g, o, true)], 1u);
    if (WRITE) w.tmp[(size_t)o * a.P + pos] = (uint32_t)g;
  }
  if (!WRITE) {
    __syncthreads();
    for (int i = threadIdx.x; i < SORT_BINS; i += 256) row[i] = cell[i];
  }
}

// one workgroup per orientation: per-bin prefix over the SORT_NB workgroups, then exclusive scan of the bin totals
__global__ void __launch_bounds__(512) hexsort_scan_kernel(const SortWork w, int P) {
  __shared__ uint32_t tot[SORT_BINS];
  const int o = blockIdx.x, b = threadIdx.x;
  uint32_t* tab = w.table + (size_t)o * SORT_NB * SORT_BINS;
  uint32_t run = 0;
  for (int k = 0; k < SORT_NB; k++) {
    const uint32_t v = tab[(size_t)k * SORT_BINS + b];
    tab[(size_t)k * SORT_BINS + b] = run;
    run += v;
  }
  tot[b] = run;
  __syncthreads();
  if (b == 0) {
    uint32_t acc = 0;
    for (int i = 0; i < SORT_BINS; i++) {
      w.seg_start[o * (SORT_BINS + 1) + i] = acc;
      acc += tot[i];
    }
    w.seg_start[o * (SORT_BINS + 1) + SORT_BINS] = acc;
  }
}

// one workgroup per (major bin, orientation): counting sort of the segment by minor cell
__global__ void __launch_bounds__(256) hexsort_minor_kernel(const HexArgs a, const SortWork w, int stable) {
  __shared__ uint32_t cnt[SORT_BINS];
  __shared__ uint32_t wsum[4];
  __shared__ uint32_t wcnt[4 * SORT_BINS];
  const int o = blockIdx.y, bin = blockIdx.x, tid = threadIdx.x;
  const uint32_t s0 = w.seg_start[o * (SORT_BINS + 1) + bin], s1 = w.seg_start[o * (SORT_BINS + 1) + bin + 1];
  if (s1 == s0) return;
  const uint32_t* tmp = w.tmp + (size_t)o * a.P;
  uint32_t* order = order_of(w, o, a.P);
  for (int i = tid; i < SORT_BINS; i += 256) cnt[i] = 0u;
  __syncthreads();
  for (uint32_t k = s0 + tid; k < s1; k += 256) atomicAdd(&cnt[order_key(a, (int)tmp[k], o, false)], 1u);
  __syncthreads();
  // exclusive scan of 512 counters: each thread owns two consecutive bins
  const uint32_t c0 = cnt[2 * tid], c1 = cnt[2 * tid + 1];
  uint32_t incl = c0 + c1;
  const int lane = tid & 63, wave = tid >> 6;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)incl, off);
    if (lane >= off) incl += t;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  uint32_t base = s0;
  for (int k = 0; k < wave; k++) base += wsum[k];
  const uint32_t excl = base + incl - (c0 + c1);
  __syncthreads();
  cnt[2 * tid] = excl;
  cnt[2 * tid + 1] = excl + c0;
  __syncthreads();
  if (stable) {
    for (int i = tid; i < 4 * SORT_BINS; i += 256) wcnt[i] = 0u;
    __syncthreads();
    for (uint32_t kb = s0; kb < s1; kb += 256) {   // uniform trip count (stable_claim synchronises); tmp is index-ascending per major bin
      const uint32_t k = kb + tid;
      const bool act = k < s1;
      const uint32_t g = act ? tmp[k] : 0u;
      const uint32_t pos = stable_claim(cnt, wcnt, act ? order_key(a, (int)g, o, false) : 0, act);
      if (act) order[pos] = g;
    }
    return;
  }
  for (uint32_t k = s0 + tid; k < s1; k += 256) {
    const uint32_t g = tmp[k];
    order[atomicAdd(&cnt[order_key(a, (int)g, o, false)], 1u)] = g;
  }
}

__global__ void __launch_bounds__(256) hexsort_rank_kernel(int P, const uint32_t* __restrict__ order, uint32_t* __restrict__ rank) {
  const int k = blockIdx.x * 256 + threadIdx.x, o = blockIdx.y;
  if (k < P) rank[(size_t)o * P + order[(size_t)o * P + k]] = (uint32_t)k;
}
// point-major G: where in the PROCESSING order is the k-th point of orientation o's order?  comp[o][k] = procrank[order[o][k]]
__global__ void __launch_bounds__(256) hexsort_compose_kernel(int P, const uint32_t* __restrict__ order, const uint32_t* __restrict__ procrank,
                                                              uint32_t* __restrict__ comp) {
  const int k = blockIdx.x * 256 + threadIdx.x, o = blockIdx.y;
  if (k < P) comp[(size_t)o * P + k] = procrank[order[(size_t)o * P + k]];
}

// count, scan, place by major key; sort every major bin by minor key; then comp[oi][k], the inverse of the processing order going
// through w.tmp (free after the sorts).  Uses the real resolutions: before the time planes of `a` become row tables.
int hexplane_sort_launch(const HexArgs& a, const SortWork& w, int det, hipStream_t stream) {
  const int P = a.P, NO = n_orders(a.d.levels), NW = n_walk_orders(a.d.levels);
  const int chunk = (((P + SORT_NB - 1) / SORT_NB + 255) / 256) * 256;
  hipLaunchKernelGGL(hexsort_major_kernel<false>, dim3(SORT_NB, NO), dim3(256), 0, stream, a, w, chunk, det);
  hipLaunchKernelGGL(hexsort_scan_kernel, dim3(NO), dim3(512), 0, stream, w, P);
  hipLaunchKernelGGL(hexsort_major_kernel<true>, dim3(SORT_NB, NO), dim3(256), 0, stream, a, w, chunk, det);
  hipLaunchKernelGGL(hexsort_minor_kernel, dim3(SORT_BINS, NO), dim3(256), 0, stream, a, w, det);
  hipLaunchKernelGGL(hexsort_rank_kernel, dim3((P + 255) / 256, 1), dim3(256), 0, stream, P, w.proc, w.tmp);
  hipLaunchKernelGGL(hexsort_compose_kernel, dim3((P + 255) / 256, NW), dim3(256), 0, stream, P, w.order, w.tmp, w.comp);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

}  // namespace s3g
