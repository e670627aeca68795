// Rasterizer forward, stage 2: atomic-free binning ("multisplit" of the R instances into tiles*).
// bin_count : NB fat workgroups, each owns a contiguous chunk of Gaussians and histograms its instances over
//             ALL tiles in LDS (ds_add_u32), then stores its row of table[NB][tiles] + its chunk total.
// bin_scan  : per tile, exclusive prefix over the NB workgroups (in place) and the tile total.
// scan_tiles: exclusive scan over tiles -> ranges, R, longest list; exclusive scan of chunk totals.
// bin_write : same walk as bin_count; LDS cursors start at ranges[t].x + table[wg][t]; every instance key is
//             stored at a private slot.  Also emits gauss_off[g] = exclusive scan of tiles_touched (Gaussian order),
//             the address of g's slots in the instance->position map used by the backward gather.
// Rects wider than BIG_RECT tiles are walked by the whole wave instead of one lane.
// Tile grids larger than the LDS histogram (MAX_TILES_LDS) are processed in BANDS of consecutive tiles: both walks are
// launched once per band and only handle the instances whose tile lies in it (an 8K image is 4 bands).
// (*) order inside a tile is arbitrary here; the per-tile sort fixes it.
#include "geom_math.hpp"

namespace s3g {

static int g_max_tiles_lds = MAX_TILES_LDS;  // band size of the binning histogram; lowered only by the tests (s3g_raster_set_bin_band)

#ifndef S3G_BIN_THREADS
#define S3G_BIN_THREADS 512
#endif
// Both walks are chains of dependent global loads (rect -> tile mask / depth) in front of LDS work, run by 2 workgroups per CU
// (the histogram of ALL tiles lives in LDS: more workgroups would mean more table rows for bin_scan).  What hides the latency is
// (i) more waves per workgroup -- the histogram is shared, so threads are free -- and (ii) the next step's three loads requested
// before this step's walk; the block-wide scan of bin_write therefore synchronises on LDS only (an ordinary __syncthreads()
// would also wait for the prefetch).
constexpr int BIN_THREADS = S3G_BIN_THREADS, BIN_WAVES = BIN_THREADS / 64, BIN_SCRATCH = 2 * BIN_WAVES + 8;
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
constexpr int BIG_RECT = 32;  // rects of more tiles are walked by a whole wave in the binning kernels
static_assert(BIG_RECT <= TILE_MASK_BITS, "smaller rects replay the preprocess' tile mask");

struct BinArgs {
  int P, gx, tiles, chunk;         // chunk = Gaussians per workgroup
  int tile_lo, tile_n;             // the band of tiles this launch handles: [tile_lo, tile_lo + tile_n)
  const ushort4* rect;
  const float* depths;
  uint32_t* table;                 // [NB][tiles]
  uint32_t* chunk_total;           // [NB] instances emitted by each workgroup; after scan_tiles: exclusive prefix
  const uint2* ranges;             // bin_write only
  uint64_t* keys;                  // bin_write only
  uint32_t* gauss_off;             // bin_write only
  // exact (tile, Gaussian) culling (geom_math.hpp::tile_can_contribute); cull == 0: the reference's bounding square
  int cull, W, H;
  const float2* means2D;
  const float4* conic_opacity;
  const uint32_t* tile_mask;       // from preprocess_kernel (rects of <= BIG_RECT tiles)
  const uint32_t* ctrl;            // bin_write only: ctrl[4] != 0 = the speculative arena capacity was exceeded, write nothing
};

template <bool WRITE>
__global__ void __launch_bounds__(BIN_THREADS) bin_kernel(const BinArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];  // [tiles] histogram / cursors, then BIN_SCRATCH words
  uint32_t* cell = lds;
  uint32_t* wsum = lds + a.tile_n;  // [2][BIN_WAVES] wave totals, alternating by step: ONE barrier per step
  if (WRITE && a.ctrl[4] != 0u) return;  // host-asynchronous forward: the instances do not fit the arena (see scan_tiles_kernel)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t* trow = a.table + (size_t)blockIdx.x * a.tiles;
  for (int i = tid; i < a.tile_n; i += BIN_THREADS) cell[i] = WRITE ? a.ranges[a.tile_lo + i].x + trow[a.tile_lo + i] : 0u;
  const bool first_band = a.tile_lo == 0;  // per-Gaussian outputs (gauss_off, chunk totals) are produced once
  uint32_t carry = WRITE ? a.chunk_total[blockIdx.x] : 0u;  // exclusive prefix of previous workgroups' instances
  uint32_t my_total = 0;
  __syncthreads();
  const int g0 = blockIdx.x * a.chunk, g1 = min(a.P, g0 + a.chunk);
  // what a step needs of its Gaussian: rect, the mask of tiles that survive the exact cull (meaningful for 0 < area <= BIG_RECT
  // only; whatever the word holds otherwise is not used) and the depth bits of the key
  ushort4 r_next = make_ushort4(0, 0, 0, 0);
  uint32_t mask_next = 0xffffffffu, depth_next = 0u;
  if (g0 + tid < g1) {
    r_next = a.rect[g0 + tid];
    if (a.cull) mask_next = a.tile_mask[g0 + tid];
    if (WRITE) depth_next = __float_as_uint(a.depths[g0 + tid]);
  }
  int step = 0;
  for (int base = g0; base < g1; base += BIN_THREADS, step ^= 1) {
    const int g = base + tid;
    const ushort4 r = r_next;
    const uint32_t mask = mask_next, dbits = depth_next;
    const int gn = g + BIN_THREADS;
    r_next = make_ushort4(0, 0, 0, 0);
    if (gn < g1) {
      r_next = a.rect[gn];
      if (a.cull) mask_next = a.tile_mask[gn];
      if (WRITE) depth_next = __float_as_uint(a.depths[gn]);
    }
    const int w = (int)r.z - (int)r.x, h = (int)r.w - (int)r.y;
    const uint32_t area = (w > 0 && h > 0) ? (uint32_t)(w * h) : 0u;
    uint64_t key = 0;
    TileCull tc;
    tc.verdict = 1;
    if (a.cull && area > BIG_RECT) tc = tile_cull_prepare(a.means2D[g], a.conic_opacity[g]);  // small rects: mask replay
    if (WRITE) {
      // block-wide exclusive scan of area -> gauss_off (slots are counted per rect tile whether or not it survives)
      uint32_t incl = area;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)incl, off);
        if (lane >= off) incl += t;
      }
      uint32_t* ws = wsum + step * BIN_WAVES;
      if (lane == 63) ws[wave] = incl;
      lds_barrier();
      uint32_t wbase = 0, tot = 0;
#pragma unroll
      for (int k = 0; k < BIN_WAVES; k++) {
        const uint32_t v = ws[k];
        if (k < wave) wbase += v;
        tot += v;
      }
      if (g < g1 && first_band) a.gauss_off[g] = carry + wbase + incl - area;
      carry += tot;
      if (area) key = ((uint64_t)dbits << 32) | (uint32_t)g;
    } else {
      my_total += area;
    }
    if (area != 0 && area <= BIG_RECT) {
      uint32_t bit = 1u;
      for (int y = r.y; y < r.w; y++)
        for (int x = r.x; x < r.z; x++, bit <<= 1) {
          if (!(mask & bit)) continue;
          const uint32_t tb = (uint32_t)(y * a.gx + x - a.tile_lo);
          if (tb >= (uint32_t)a.tile_n) continue;
          const uint32_t pos = atomicAdd(&cell[tb], 1u);
          if (WRITE) a.keys[pos] = key;
        }
    }
    uint64_t big = __ballot(area > BIG_RECT);
    while (big) {  // wave-uniform loop: all 64 lanes walk one large rect together
      const int src = __ffsll((unsigned long long)big) - 1;
      big &= big - 1;
      const int bx = __shfl((int)r.x, src), by = __shfl((int)r.y, src), bw = __shfl(w, src);
      const uint32_t barea = (uint32_t)__shfl((int)area, src);
      const uint32_t klo = (uint32_t)__shfl((int)(uint32_t)key, src), khi = (uint32_t)__shfl((int)(uint32_t)(key >> 32), src);
      TileCull bt;
      bt.a = __shfl(tc.a, src); bt.b = __shfl(tc.b, src); bt.c = __shfl(tc.c, src); bt.inv_a = __shfl(tc.inv_a, src);
      bt.inv_c = __shfl(tc.inv_c, src); bt.budget = __shfl(tc.budget, src); bt.mx = __shfl(tc.mx, src);
      bt.my = __shfl(tc.my, src); bt.verdict = __shfl(tc.verdict, src);
      for (uint32_t k = lane; k < barea; k += 64) {
        const int ty = by + (int)(k / (uint32_t)bw), tx = bx + (int)(k % (uint32_t)bw);
        const uint32_t tb = (uint32_t)(ty * a.gx + tx - a.tile_lo);
        if (tb >= (uint32_t)a.tile_n) continue;
        if (a.cull && !tile_can_contribute(bt, tx, ty, a.W, a.H)) continue;
        const uint32_t pos = atomicAdd(&cell[tb], 1u);
        if (WRITE) a.keys[pos] = ((uint64_t)khi << 32) | klo;
      }
    }
  }
  if (!WRITE) {
    __syncthreads();
    uint32_t* row = a.table + (size_t)blockIdx.x * a.tiles;
    for (int i = tid; i < a.tile_n; i += BIN_THREADS) row[a.tile_lo + i] = cell[i];
    for (int off = 32; off >= 1; off >>= 1) my_total += (uint32_t)__shfl_xor((int)my_total, off);
    if (lane == 0) wsum[wave] = my_total;
    __syncthreads();
    if (tid == 0 && first_band) {
      uint32_t tot = 0;
      for (int k = 0; k < BIN_WAVES; k++) tot += wsum[k];
      a.chunk_total[blockIdx.x] = tot;
    }
  }
}

// Exclusive prefix over the binning workgroups, per tile (coalesced across tiles).  A thread that walks all nb rows of its tile
// is a chain of nb / 32 dependent round trips on 27 workgroups (24 us at 6700 tiles, nb = 512: 1.1 TB/s); the rows are therefore
// split into SCAN_PARTS contiguous parts, one WAVE per part and 64 tiles per workgroup: every part sums its rows (32 independent
// loads in flight), the part sums meet in LDS, and a second sweep over the same rows (L2-resident by then) writes the prefixes.
#ifndef S3G_SCAN_PARTS
#define S3G_SCAN_PARTS 8
#endif
constexpr int SCAN_PARTS = S3G_SCAN_PARTS;
__global__ void __launch_bounds__(64 * SCAN_PARTS) bin_scan_kernel(int tiles, int nb, uint32_t* __restrict__ table,
                                                                    uint32_t* __restrict__ tile_count) {
  constexpr int INFLIGHT = 32;
  __shared__ uint32_t psum[SCAN_PARTS][64];
  const int lane = threadIdx.x & 63, part = threadIdx.x >> 6;
  const int t = blockIdx.x * 64 + lane;
  const bool live = t < tiles;
  const int rows = (nb + SCAN_PARTS - 1) / SCAN_PARTS, b0 = part * rows, b1 = min(nb, b0 + rows);
  uint32_t sum = 0;
  if (live)
    for (int b = b0; b < b1; b += INFLIGHT) {
      uint32_t v[INFLIGHT];
#pragma unroll
      for (int k = 0; k < INFLIGHT; k++) v[k] = (b + k < b1) ? table[(size_t)(b + k) * tiles + t] : 0u;
#pragma unroll
      for (int k = 0; k < INFLIGHT; k++) sum += v[k];
    }
  psum[part][lane] = sum;
  __syncthreads();
  if (!live) return;
  uint32_t run = 0, total = 0;
#pragma unroll
  for (int k = 0; k < SCAN_PARTS; k++) {
    const uint32_t x = psum[k][lane];
    if (k < part) run += x;
    total += x;
  }
  for (int b = b0; b < b1; b += INFLIGHT) {
    uint32_t v[INFLIGHT];
#pragma unroll
    for (int k = 0; k < INFLIGHT; k++) v[k] = (b + k < b1) ? table[(size_t)(b + k) * tiles + t] : 0u;
#pragma unroll
    for (int k = 0; k < INFLIGHT; k++) {
      if (b + k < b1) table[(size_t)(b + k) * tiles + t] = run;
      run += v[k];
    }
  }
  if (part == 0) tile_count[t] = total;
}

// Inclusive scan of one value per thread over the 1024 threads: shuffles inside a wave, the 16 wave totals through LDS (three
// barriers; a Hillis-Steele scan in LDS costs twenty, and scan_tiles_kernel is ONE workgroup on an otherwise idle device: 13 -> 4 us).
__device__ __forceinline__ uint32_t block_inclusive_scan_waves(uint32_t v, uint32_t* wtot, int tid, uint32_t* total) {
  const int lane = tid & 63, wave = tid >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)incl, off);
    if (lane >= off) incl += t;
  }
  __syncthreads();   // wtot may still be read from a previous call
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  uint32_t wbase = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const uint32_t x = wtot[k];
    if (k < wave) wbase += x;
    tot += x;
  }
  *total = tot;
  return wbase + incl;
}

// Exclusive scan over tiles: ranges[t] = [start, end); ctrl[0] = R, ctrl[1] = longest tile list, ctrl[3] = slots; also turns
// chunk_total[nb] into its exclusive prefix.  One 1024-thread workgroup; tiles is O(10^3..10^4), nb <= 1024.
// Host-asynchronous forward (s3g_raster_forward_async): the binning arena was sized BEFORE this kernel knew R.  cap_R != 0
// turns the capacity check on: if R > cap_R, S > cap_S or the longest list > cap_tile, ctrl[4] = 1, every range is emptied and
// R / S read as 0, so that every later kernel of the forward AND of the backward finds nothing to do (bin_write and the
// per-Gaussian backward also look at ctrl[4] themselves); the true counts stay in ctrl[5..6] for the host, which reads them
// late, without stalling.  *status (optional device word, written on every call): bit 0 = overflow, bit 1 = a Gaussian was
// culled although `prefiltered` was set.
// *sticky (optional device word, s3g_raster_async.sticky_device): set by the call that overflows and then honoured by every
// later call that is handed the same word -- they render nothing either (ctrl[4] = 1, ctrl[7] = 1 "because of an earlier call")
// until the host clears it.  With the guarded optimizer step this freezes the model from the overflowed iteration on, so that the
// host, which learns of the overflow a few iterations late, can raise the capacity, clear the word and RE-ISSUE the iterations
// from the overflowed one: the sequence of (view, optimizer step) pairs the model sees is then the reference's, none dropped.
__global__ void __launch_bounds__(1024) scan_tiles_kernel(int tiles, const uint32_t* __restrict__ tile_count,
                                                          uint2* __restrict__ ranges, uint32_t* __restrict__ ctrl,
                                                          int nb, uint32_t* __restrict__ chunk_total, uint32_t cap_R,
                                                          uint32_t cap_S, uint32_t cap_tile, uint32_t* __restrict__ status,
                                                          uint32_t* __restrict__ sticky) {
  __shared__ uint32_t wtot[16];
  __shared__ uint32_t wmax[16];
  const int tid = threadIdx.x;
  // thread t owns the tiles [t * per, (t + 1) * per): a serial sum, ONE block scan of the 1024 sums, a serial pass for the ranges
  const int per = (tiles + 1023) / 1024, t0 = tid * per, t1 = min(tiles, t0 + per);
  uint32_t vmax = 0, mine = 0, total, carry;
  for (int i = t0; i < t1; i++) {
    const uint32_t v = tile_count[i];
    vmax = max(vmax, v);
    mine += v;
  }
  {
    uint32_t start = block_inclusive_scan_waves(mine, wtot, tid, &carry) - mine;   // carry = R
    for (int i = t0; i < t1; i++) {
      const uint32_t v = tile_count[i];
      ranges[i] = make_uint2(start, start + v);
      start += v;
    }
  }
  {
    const uint32_t v = tid < nb ? chunk_total[tid] : 0u;
    const uint32_t incl = block_inclusive_scan_waves(v, wtot, tid, &total);
    if (tid < nb) chunk_total[tid] = incl - v;
    if (tid == 0) ctrl[3] = total;  // S: slots = sum of rect areas (== R without culling)
  }
  for (int off = 32; off >= 1; off >>= 1) vmax = max(vmax, (uint32_t)__shfl_xor((int)vmax, off));
  if ((tid & 63) == 0) wmax[tid >> 6] = vmax;
  __syncthreads();
  uint32_t m = 0;
  for (int w = 0; w < 16; w++) m = max(m, wmax[w]);
  const bool own = cap_R != 0u && (carry > cap_R || total > cap_S || m > cap_tile);   // `total` = S (last scan above)
  const bool frozen = cap_R != 0u && sticky != nullptr && *sticky != 0u;               // an EARLIER call overflowed (uniform load)
  const bool overflow = own || frozen;
  if (overflow)
    for (int i = tid; i < tiles; i += 1024) ranges[i] = make_uint2(0u, 0u);
  if (tid == 0) {
    ctrl[0] = overflow ? 0u : carry;
    ctrl[1] = m;
    if (overflow) ctrl[3] = 0u;
    ctrl[4] = overflow ? 1u : 0u;
    ctrl[5] = carry;
    ctrl[6] = total;
    ctrl[7] = (frozen && !own) ? 1u : 0u;
    if (sticky && own) *sticky = 1u;
    if (status) *status = (overflow ? 1u : 0u) | ((ctrl[2] & 1u) ? 2u : 0u);
  }
}

// slot_pos[0 .. S) = 0xffffffff ("tile culled") with S read on the device (the asynchronous forward does not know it).
__global__ void __launch_bounds__(256) fill_slots_kernel(uint32_t* __restrict__ slot_pos, const uint32_t* __restrict__ ctrl) {
  const uint32_t S = ctrl[3];
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < S; i += gridDim.x * 256u) slot_pos[i] = 0xffffffffu;
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------
static BinArgs bin_args(int P, const Arenas& a, bool exact_cull) {
  BinArgs ba;
  ba.P = P; ba.gx = a.gx; ba.tiles = a.tiles; ba.chunk = bin_chunk(P); ba.rect = a.g.rect; ba.depths = a.g.depths;
  ba.table = a.im.table; ba.chunk_total = a.im.chunk_total; ba.ranges = a.im.ranges; ba.keys = a.b.keys; ba.gauss_off = a.g.gauss_off;
  ba.cull = exact_cull ? 1 : 0; ba.W = a.W; ba.H = a.H; ba.means2D = a.g.means2D; ba.conic_opacity = a.g.conic_opacity;
  ba.tile_mask = a.g.tile_mask; ba.ctrl = a.im.ctrl;
  return ba;
}

// One walk over the Gaussians per band of tiles; tile grids beyond the LDS histogram take several (see bin_kernel).
template <bool WRITE>
static int launch_bin_walk(BinArgs ba, int nb, hipStream_t stream, bool debug) {
  static std::atomic<uint64_t> attr_set{0};
  if (device_needs_setup(attr_set)) {
    S3G_HIP_CHECK(hipFuncSetAttribute((const void*)bin_kernel<WRITE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (MAX_TILES_LDS + BIN_SCRATCH) * 4));
    device_setup_done(attr_set);
  }
  const int band = g_max_tiles_lds < ba.tiles ? g_max_tiles_lds : ba.tiles;
  const size_t bin_lds = ((size_t)band + BIN_SCRATCH) * sizeof(uint32_t);
  for (int lo = 0; lo < ba.tiles; lo += band) {
    ba.tile_lo = lo; ba.tile_n = ba.tiles - lo < band ? ba.tiles - lo : band;
    hipLaunchKernelGGL(bin_kernel<WRITE>, dim3(nb), dim3(BIN_THREADS), bin_lds, stream, ba);
    S3G_KERNEL_CHECK(stream, debug);
  }
  return S3G_OK;
}
int launch_bin_count(int P, const Arenas& a, bool exact_cull, hipStream_t stream, bool debug) {
  return launch_bin_walk<false>(bin_args(P, a, exact_cull), bin_blocks(P), stream, debug);
}
int launch_bin_write(int P, const Arenas& a, bool exact_cull, hipStream_t stream, bool debug) {
  return launch_bin_walk<true>(bin_args(P, a, exact_cull), bin_blocks(P), stream, debug);
}

int launch_bin_scan(int P, const Arenas& a, const s3g_raster_async* as, hipStream_t stream, bool debug) {
  const ImageState& im = a.im;
  const int tiles = a.tiles, nb = bin_blocks(P);
  hipLaunchKernelGGL(bin_scan_kernel, dim3((tiles + 63) / 64), dim3(64 * SCAN_PARTS), 0, stream, tiles, nb, im.table, im.tile_count);
  S3G_KERNEL_CHECK(stream, debug);
  hipLaunchKernelGGL(scan_tiles_kernel, dim3(1), dim3(1024), 0, stream, tiles, im.tile_count, im.ranges, im.ctrl, nb,
                     im.chunk_total, as ? as->capacity_instances : 0u, as ? as->capacity_slots : 0u,
                     sort_list_cap(as), as ? as->status_device : nullptr,
                     (as && !as->forward_only) ? as->sticky_device : nullptr);
  S3G_KERNEL_CHECK(stream, debug);
  return S3G_OK;
}

int launch_fill_slots(const Arenas& a, hipStream_t stream, bool debug) {
  hipLaunchKernelGGL(fill_slots_kernel, dim3(1024), dim3(256), 0, stream, a.b.slot_pos, (const uint32_t*)a.im.ctrl);
  S3G_KERNEL_CHECK(stream, debug);
  return S3G_OK;
}

}  // namespace s3g

using namespace s3g;

extern "C" int s3g_raster_set_bin_band(int tiles) {  // testing hook: returns the previous band size; <= 0 restores the default
  const int prev = g_max_tiles_lds;
  g_max_tiles_lds = (tiles <= 0 || tiles > MAX_TILES_LDS) ? MAX_TILES_LDS : tiles;
  return prev;
}
