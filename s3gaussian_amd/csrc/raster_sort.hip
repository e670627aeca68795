// Rasterizer forward, stage 3: per-tile sort of 64-bit (depth bits | index) keys: bitonic network with all comparators ascending
// (first sub-step of each stage mirrors, i ^ (k-1)), so a non-power-of-two list is handled by skipping
// comparators whose upper element is past the end (virtual +inf padding never moves).
// Lists that fit stay in LDS; longer ones run the same network in place in global memory.
#include "geom_math.hpp"

namespace s3g {

// `nthreads` threads share the list and `barrier` makes the writes of a step visible to all of them: the workgroup with
// __syncthreads() (BlockBarrier), or ONE wave on a short list of its own with wave_lds_sync() (WaveBarrier, nthreads = 64).
struct BlockBarrier { __device__ __forceinline__ void operator()() const { __syncthreads(); } };
struct WaveBarrier { __device__ __forceinline__ void operator()() const { wave_lds_sync(); } };
template <typename KeyPtr, typename Barrier>
__device__ __forceinline__ void bitonic_network(KeyPtr a, uint32_t n, uint32_t tid, uint32_t nthreads, Barrier barrier) {
  uint32_t lN = 0;
  while ((1u << lN) < n) lN++;
  const uint32_t half = (1u << lN) >> 1;  // comparators per step
  for (uint32_t lk = 1; lk <= lN; lk++) {
    {  // mirror step: element o of block b against element k-1-o
      const uint32_t k = 1u << lk, lhk = lk - 1, hk = 1u << lhk;
      for (uint32_t c = tid; c < half; c += nthreads) {
        const uint32_t b = c >> lhk, o = c & (hk - 1);
        const uint32_t i = (b << lk) + o, l = (b << lk) + (k - 1 - o);
        if (l < n) {
          const uint64_t x = a[i], y = a[l];
          if (x > y) { a[i] = y; a[l] = x; }
        }
      }
      barrier();
    }
    for (int lj = (int)lk - 2; lj >= 0; lj--) {  // half-cleaners, distance j = 2^lj
      const uint32_t j = 1u << lj;
      for (uint32_t c = tid; c < half; c += nthreads) {
        const uint32_t b = c >> lj, o = c & (j - 1);
        const uint32_t i = (b << (lj + 1)) + o, l = i + j;
        if (l < n) {
          const uint64_t x = a[i], y = a[l];
          if (x > y) { a[i] = y; a[l] = x; }
        }
      }
      barrier();
    }
  }
}

// ---- long lists (round 6): one bucket pass, then small sorts ---------------------------------------------------------------------
// The bitonic network moves every key through LDS log2(n) (log2(n) + 1) / 2 times: 78 steps at 4096 keys -- on a scene whose mean tile
// list is 1800 instances (bench.py's heavy_raster leg: R = 12 M) the per-tile sort was the most expensive kernel of the step (2 x 0.67
// ms).  A list longer than BUCKET_MIN keys is first split into SORT_BINS buckets by the leading bits of (depth bits - smallest depth bits
// of the list) -- monotone in the key, so the buckets are in order and only have to be sorted inside: LDS histogram, one scan, one
// scatter into a second LDS buffer (each an integer atomic per key: WHERE a key lands inside its bucket depends on their order, the
// sorted result does not -- the 64-bit keys of a list are all different) -- and then every key counts the smaller keys of its own
// bucket (<= BUCKET_RANK keys; a bucket holds one or two on average) and goes to bucket start + rank; the rare larger buckets take the
// network, by one wave (<= BUCKET_WAVE keys) or the workgroup.  About ten LDS operations per key instead of a hundred and fifty;
// the result is the same ascending list.
constexpr int SORT_BIN_BITS = 11;
constexpr uint32_t SORT_BINS = 1u << SORT_BIN_BITS, BUCKET_MIN = 512, BUCKET_RANK = 48, BUCKET_WAVE = 512, BUCKET_LIST = 256;
#ifndef S3G_SORT_THREADS_MID
#define S3G_SORT_THREADS_MID 512
#endif
#ifndef S3G_SORT_THREADS_LONG
#define S3G_SORT_THREADS_LONG 1024
#endif
#ifndef S3G_SORT_RANK_DIRECT
#define S3G_SORT_RANK_DIRECT 256
#endif
constexpr uint32_t RANK_DIRECT = S3G_SORT_RANK_DIRECT;   // lists of at most this many keys: one thread per key, rank by counting
constexpr uint32_t SORT_THREADS_MID = S3G_SORT_THREADS_MID, SORT_THREADS_LONG = S3G_SORT_THREADS_LONG;   // workgroup sizes of the two long-list launches
constexpr uint32_t BUCKET_LDS_EXTRA = SORT_BINS * 4 + BUCKET_LIST * 2 * 2;   // bytes behind the two key buffers: cursors, two bucket lists

// A[0, n) holds the list; returns with A[0, n) sorted (B: scratch of n keys).  cur: SORT_BINS words, lists: 2 x BUCKET_LIST uint16.
// nt = 256 ... 1024 threads (the long-list launches bring more waves: the passes below are chains of dependent LDS operations, and a
// workgroup that fills most of a CU's LDS is alone on it).  (n <= 7424 keys: at most n / (BUCKET_RANK + 1) < BUCKET_LIST buckets can be listed.)
__device__ __forceinline__ void bucket_sort_lds(uint64_t* __restrict__ A, uint64_t* __restrict__ B, uint32_t* __restrict__ cur,
                                                uint16_t* __restrict__ lists, uint32_t n, uint32_t tid, uint32_t nt) {
  __shared__ uint32_t red[32];
  __shared__ uint32_t nlist[2];
  const uint32_t lane = tid & 63u, wave = tid >> 6, nwaves = nt >> 6;
  uint32_t mn = 0xffffffffu, mx = 0u;
  for (uint32_t i = tid; i < n; i += nt) {
    const uint32_t h = (uint32_t)(A[i] >> 32);
    mn = min(mn, h); mx = max(mx, h);
  }
  for (int off = 32; off >= 1; off >>= 1) {
    mn = min(mn, (uint32_t)__shfl_xor((int)mn, off));
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, off));
  }
  if (lane == 0) { red[wave] = mn; red[16 + wave] = mx; }
  if (tid < 2) nlist[tid] = 0u;
  for (uint32_t b = tid; b < SORT_BINS; b += nt) cur[b] = 0u;
  __syncthreads();
  mn = red[0]; mx = red[16];
  for (uint32_t w = 1; w < nwaves; w++) { mn = min(mn, red[w]); mx = max(mx, red[16 + w]); }
  const uint32_t range = mx - mn;
  const int sh = range ? max(0, 32 - (int)__clz(range) - SORT_BIN_BITS) : 0;     // (range >> sh) < SORT_BINS
  for (uint32_t i = tid; i < n; i += nt) atomicAdd(&cur[((uint32_t)(A[i] >> 32) - mn) >> sh], 1u);
  __syncthreads();
  {  // exclusive scan of the SORT_BINS counters: thread t < 256 owns PER consecutive bins (the other waves only keep the barriers company)
    constexpr int PER = SORT_BINS / 256;
    uint32_t c[PER], sum = 0;
    if (tid < 256) {
#pragma unroll
      for (int k = 0; k < PER; k++) { c[k] = cur[PER * tid + k]; sum += c[k]; }
    }
    uint32_t incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t t = (uint32_t)__shfl_up((int)incl, off);
      if (lane >= (uint32_t)off) incl += t;
    }
    __syncthreads();               // red[] is read above
    if (lane == 63 && wave < 4) red[wave] = incl;
    __syncthreads();
    if (tid < 256) {
      uint32_t excl = incl - sum;
      for (uint32_t w = 0; w < wave; w++) excl += red[w];
#pragma unroll
      for (int k = 0; k < PER; k++) { cur[PER * tid + k] = excl; excl += c[k]; }
    }
  }
  __syncthreads();
  for (uint32_t i = tid; i < n; i += nt) {
    const uint64_t k = A[i];
    B[atomicAdd(&cur[((uint32_t)(k >> 32) - mn) >> sh], 1u)] = k;
  }
  __syncthreads();
  // cur[b] is now the END of bucket b; it starts where bucket b - 1 ends.  Buckets of more than BUCKET_RANK keys (rare: > 30 x the mean)
  // are listed for a network sort; every other key finds its place by COUNTING the smaller keys of its own bucket -- one thread per
  // key, no thread waits for another, ~(2 + bucket size) LDS reads per key -- and goes back into A at bucket start + rank.
  for (uint32_t b = tid; b < SORT_BINS; b += nt) {
    const uint32_t s0 = b ? cur[b - 1] : 0u, m = cur[b] - s0;
    if (m > BUCKET_RANK) {
      const uint32_t which = m <= BUCKET_WAVE ? 0u : 1u;
      const uint32_t slot = atomicAdd(&nlist[which], 1u);
      if (slot < BUCKET_LIST) lists[which * BUCKET_LIST + slot] = (uint16_t)b;
    }
  }
  for (uint32_t i = tid; i < n; i += nt) {
    const uint64_t k = B[i];
    const uint32_t b = ((uint32_t)(k >> 32) - mn) >> sh;
    const uint32_t s0 = b ? cur[b - 1] : 0u, e0 = cur[b];
    if (e0 - s0 > BUCKET_RANK) continue;
    uint32_t rank = 0;
    for (uint32_t j = s0; j < e0; j++) rank += B[j] < k ? 1u : 0u;
    A[s0 + rank] = k;
  }
  __syncthreads();
  const uint32_t nw = nlist[0], ng = nlist[1];
  for (uint32_t q = wave; q < nw; q += nwaves) {      // one wave per medium bucket: sorted in B, copied to A
    const uint32_t b = lists[q];
    const uint32_t s0 = b ? cur[b - 1] : 0u, m = cur[b] - s0;
    bitonic_network(B + s0, m, lane, 64u, WaveBarrier());
    for (uint32_t i = lane; i < m; i += 64) A[s0 + i] = B[s0 + i];
  }
  __syncthreads();
  for (uint32_t q = 0; q < ng; q++) {            // the workgroup on every large bucket (uniform loop; bitonic_network ends on a barrier)
    const uint32_t b = lists[BUCKET_LIST + q];
    const uint32_t s0 = b ? cur[b - 1] : 0u, m = cur[b] - s0;
    bitonic_network(B + s0, m, tid, nt, BlockBarrier());
    for (uint32_t i = tid; i < m; i += nt) A[s0 + i] = B[s0 + i];
  }
  __syncthreads();
}

// Tiles with lo < n <= hi are handled by this launch; lds_keys = capacity of the dynamic LDS buffer in keys; bucket_keys != 0: the
// buffer is laid out for bucket_sort_lds (two key buffers of bucket_keys keys + BUCKET_LDS_EXTRA bytes) and lists of more than
// BUCKET_MIN and at most bucket_keys keys take it.
// After sorting, slot_pos[gauss_off[g] + (tile's index inside g's rect)] = position of the instance in point_list:
// the instance -> position map that lets the backward gather per-instance gradients without atomics.
__device__ __forceinline__ void emit_instance(uint32_t pos, uint32_t g, int tx, int ty, const ushort4* __restrict__ rect,
                                              const uint32_t* __restrict__ gauss_off, uint32_t* __restrict__ point_list,
                                              uint32_t* __restrict__ slot_pos) {
  point_list[pos] = g;
  if (slot_pos == nullptr) return;   // forward-only render: nobody will gather through the map
  const ushort4 r = rect[g];
  const uint32_t local = (uint32_t)(ty - (int)r.y) * (uint32_t)((int)r.z - (int)r.x) + (uint32_t)(tx - (int)r.x);
  slot_pos[gauss_off[g] + local] = pos;
}

__global__ void __launch_bounds__(1024) sort_tiles_kernel(int tiles, int gx, const uint2* __restrict__ ranges,
                                                         uint64_t* __restrict__ keys, uint32_t* __restrict__ point_list,
                                                         const ushort4* __restrict__ rect,
                                                         const uint32_t* __restrict__ gauss_off,
                                                         uint32_t* __restrict__ slot_pos,
                                                         uint32_t lo, uint32_t hi, uint32_t lds_keys, uint32_t bucket_keys) {
  extern __shared__ __attribute__((aligned(16))) uint64_t skeys[];
  const uint32_t t = xcd_swizzle(blockIdx.x, gridDim.x);
  if (t >= (uint32_t)tiles) return;
  const uint2 rg = ranges[t];
  const uint32_t n = rg.y - rg.x;
  if (n <= lo || n > hi) return;
  uint64_t* gk = keys + rg.x;
  const uint32_t tid = threadIdx.x, nt = blockDim.x;     // 256 threads for the short lists, 512 / 1024 for the launches of the long ones
  const int tx = (int)(t % (uint32_t)gx), ty = (int)(t / (uint32_t)gx);
  if (n > BUCKET_MIN && n <= bucket_keys) {
    uint64_t* B = skeys + bucket_keys;
    uint32_t* cur = reinterpret_cast<uint32_t*>(B + bucket_keys);
    for (uint32_t i = tid; i < n; i += nt) skeys[i] = gk[i];
    __syncthreads();
    bucket_sort_lds(skeys, B, cur, reinterpret_cast<uint16_t*>(cur + SORT_BINS), n, tid, nt);
    for (uint32_t i = tid; i < n; i += nt)
      emit_instance(rg.x + i, (uint32_t)skeys[i], tx, ty, rect, gauss_off, point_list, slot_pos);
  } else if (n <= RANK_DIRECT && n <= lds_keys && nt >= RANK_DIRECT) {
    // a short list: every thread counts the keys smaller than its own (all lanes read the same LDS address: a broadcast) and emits at
    // that rank -- one barrier, no network (36 steps at 256 keys).  Two keys per thread up to 512 keys: slower than the network
    // (profiles/r06_tile_sort_ab.txt).
    const uint64_t k = tid < n ? gk[tid] : ~0ull;
    if (tid < n) skeys[tid] = k;
    __syncthreads();
    if (tid < n) {
      uint32_t rank = 0;
      for (uint32_t j = 0; j < n; j++) rank += skeys[j] < k ? 1u : 0u;
      emit_instance(rg.x + rank, (uint32_t)k, tx, ty, rect, gauss_off, point_list, slot_pos);
    }
  } else if (n <= lds_keys) {
    for (uint32_t i = tid; i < n; i += nt) skeys[i] = gk[i];
    __syncthreads();
    if (n > 1) bitonic_network(skeys, n, tid, nt, BlockBarrier());
    for (uint32_t i = tid; i < n; i += nt)
      emit_instance(rg.x + i, (uint32_t)skeys[i], tx, ty, rect, gauss_off, point_list, slot_pos);
  } else {
    bitonic_network((volatile uint64_t*)gk, n, tid, nt, BlockBarrier());  // same workgroup: coherent through its own L1 after barriers
    for (uint32_t i = tid; i < n; i += nt)
      emit_instance(rg.x + i, (uint32_t)gk[i], tx, ty, rect, gauss_off, point_list, slot_pos);
  }
}

// The launches of the per-tile sort, as data: a pure host function, so that the plan can be walked list length by list length
// without a device (s3g_raster_sort_plan, tests/test_sort_plan_cpu.py).  Every launch runs over all tiles; those with
// lo < n <= hi sort their list (see sort_tiles_kernel for lds_keys / bucket_keys).  max_tile = the longest list: read back
// exactly by the synchronous forward, the caller's ESTIMATE in the asynchronous one (as != NULL), where it may only size
// buffers: every list the counting kernel lets through (sort_list_cap) must be inside exactly one launch whatever it says.
constexpr uint32_t SORT_LARGE_KEYS = 16384;                  // lists <= SORT_SMALL_KEYS in <= 32 KiB of LDS, <= SORT_LARGE_KEYS in 128 KiB
constexpr uint32_t SORT_MAX_LDS_BYTES = SORT_LARGE_KEYS * 8;  // hipFuncAttributeMaxDynamicSharedMemorySize of sort_tiles_kernel
static int tile_sort_plan(uint32_t max_tile, const s3g_raster_async* as, s3g_sort_launch out[3]) {
  constexpr uint32_t SMALL = SORT_SMALL_KEYS, LARGE = SORT_LARGE_KEYS;
  int n = 0;
  auto plan = [&](uint32_t threads, uint32_t lds_bytes, uint32_t lo, uint32_t hi, uint32_t lds_keys, uint32_t bucket_keys) {
    out[n++] = s3g_sort_launch{threads, lds_bytes, lo, hi, lds_keys, bucket_keys};
  };
  // short lists: <= 32 KiB of LDS per workgroup (5 workgroups/CU); long lists: up to 128 KiB, beyond that in global
  // (asynchronous: max_tile is the caller's estimate; a list longer than the LDS buffer is sorted in global memory)
  const uint32_t small_cap = max_tile < SMALL ? max_tile : SMALL;
  // (a separate launch with a 2-8 KiB buffer for the lists of <= 256 / 512 / 1024 keys -- eight workgroups per CU instead of
  // five -- changes nothing: 136 / 127 / 122 us per frame against 123 with one launch, profiles/r04_sort.txt; the network's
  // LDS traffic bounds the kernel, not the workgroups in flight)
  // round 6: lists of (BUCKET_MIN, SMALL] keys in a launch of their own with the LDS layout of bucket_sort_lds (two key buffers +
  // cursors: <= 74 KiB, two workgroups per CU); the short lists keep their small buffer and their occupancy
  const uint32_t short_cap = small_cap < BUCKET_MIN ? small_cap : BUCKET_MIN;
  const bool mid = small_cap > BUCKET_MIN;
  // an estimate of <= BUCKET_MIN keys plans no medium launch, and says nothing about the lists of THIS render: the first launch
  // then takes every list up to SMALL (those beyond its buffer run the network in global memory) instead of leaving them unsorted
  plan(256, short_cap * 8, 0u, (as && !mid) ? SMALL : BUCKET_MIN, short_cap, 0u);
  if (mid) plan(SORT_THREADS_MID, small_cap * 16 + BUCKET_LDS_EXTRA, BUCKET_MIN, SMALL, 2 * small_cap, small_cap);
  if (as ? as->long_lists != 0 : max_tile > SMALL) {
    // up to LARGE keys in 128 KiB: lists that fit twice (+ the cursors) take the bucket pass too, longer ones the network in LDS,
    // still longer ones the network in global memory
    const uint32_t large_cap = as ? LARGE : (max_tile < LARGE ? max_tile : LARGE);
    const uint32_t lds_bytes = large_cap * 8 > 2 * SMALL * 8 + BUCKET_LDS_EXTRA ? large_cap * 8 : 2 * SMALL * 8 + BUCKET_LDS_EXTRA;
    const uint32_t bucket_cap = (lds_bytes - BUCKET_LDS_EXTRA) / 16;
    plan(SORT_THREADS_LONG, lds_bytes, SMALL, 0xffffffffu, lds_bytes / 8, bucket_cap);
  }
  return n;
}

int launch_tile_sort(const Arenas& a, uint32_t* slot_map, uint32_t max_tile, const s3g_raster_async* as, hipStream_t stream, bool debug) {
  static std::atomic<uint64_t> attr_set{0};
  if (device_needs_setup(attr_set)) {
    S3G_HIP_CHECK(hipFuncSetAttribute((const void*)sort_tiles_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SORT_MAX_LDS_BYTES));
    device_setup_done(attr_set);
  }
  s3g_sort_launch plan[3];
  const int launches = tile_sort_plan(max_tile, as, plan);
  for (int i = 0; i < launches; i++) {
    const s3g_sort_launch& l = plan[i];
    hipLaunchKernelGGL(sort_tiles_kernel, dim3(tile_blocks(a.tiles)), dim3(l.threads), (size_t)l.lds_bytes, stream, a.tiles, a.gx,
                       a.im.ranges, a.b.keys, a.b.point_list, a.g.rect, a.g.gauss_off, slot_map, l.lo, l.hi, l.lds_keys, l.bucket_keys);
    S3G_KERNEL_CHECK(stream, debug);
  }
  return S3G_OK;
}

}  // namespace s3g

using namespace s3g;

// testing hook: the plan of a forward as launch_tile_sort and launch_bin_scan would issue it; no device is touched
extern "C" int s3g_raster_sort_plan(int asynchronous, uint32_t keys, int long_lists, s3g_sort_plan* plan) {
  clear_error();
  if (!plan) {
    set_error("s3g_raster_sort_plan: NULL plan");
    return S3G_ERR_INVALID_ARG;
  }
  s3g_raster_async as = {};
  as.sort_lds_keys = keys;
  as.long_lists = long_lists;
  *plan = s3g_sort_plan{};
  plan->launches = (uint32_t)tile_sort_plan(asynchronous ? sort_estimate(&as) : keys, asynchronous ? &as : nullptr, plan->launch);
  plan->count_cap_tile = sort_list_cap(asynchronous ? &as : nullptr);
  plan->max_lds_bytes = SORT_MAX_LDS_BYTES;
  plan->bucket_min = BUCKET_MIN;
  plan->small_keys = SORT_SMALL_KEYS;
  plan->bucket_lds_extra = BUCKET_LDS_EXTRA;
  plan->rank_direct = RANK_DIRECT;
  return S3G_OK;
}
