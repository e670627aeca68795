// Dynamic / static point-cloud split (include/s3g_split.h): the motion classification of save_ply_split / the "dynamic point" counter
// and the PLY vertex table of save_ply / save_ply_split.  HBM-bound: the packer reads and writes every row once (2 x 248 B per
// Gaussian at SH degree 3); the classification reads dx twice (24 B per Gaussian).
#include "common.hpp"

#include "../../include/s3g_split.h"

namespace s3g {

constexpr int SB = S3G_SPLIT_BLOCK;     // Gaussians (= threads) per workgroup of the classification: four waves
constexpr int SW = SB / WAVE;
static_assert(SB == 256 && SW == 4, "the block counts below are written for four waves");

static inline int split_blocks(int P) { return P > 0 ? (P + SB - 1) / SB : 1; }
// blocks per float64 partial, a function of P alone: the summation order must not depend on anything else
static inline int split_blocks_per_partial(int P) { return (split_blocks(P) + S3G_SPLIT_MAX_PARTIALS - 1) / S3G_SPLIT_MAX_PARTIALS; }
static inline int split_partials(int P) {
  const int per = split_blocks_per_partial(P);
  return (split_blocks(P) + per - 1) / per;
}

__device__ __forceinline__ float max_abs3(const float* __restrict__ dx, long long i) {
  // torch.max(torch.abs(dx), dim=1)[0]
  return fmaxf(fmaxf(fabsf(dx[i * 3]), fabsf(dx[i * 3 + 1])), fabsf(dx[i * 3 + 2]));
}

// partial k = sum over the Gaussians of blocks [k per, (k + 1) per): thread t adds elements t, t + 256, ... in ascending order, then
// a fixed tree over the 256 thread sums
__global__ void __launch_bounds__(SB) split_partial_kernel(int P, const float* __restrict__ dx, int blocks_per,
                                                           double* __restrict__ partials) {
  __shared__ double s_sum[SB];
  const int t = threadIdx.x;
  const long long start = (long long)blockIdx.x * blocks_per * SB;
  const long long end = min((long long)P, start + (long long)blocks_per * SB);
  double s = 0.0;
  for (long long i = start + t; i < end; i += SB) s += (double)max_abs3(dx, i);
  s_sum[t] = s;
  __syncthreads();
  for (int d = SB / 2; d > 0; d >>= 1) {
    if (t < d) s_sum[t] += s_sum[t + d];
    __syncthreads();
  }
  if (t == 0) partials[blockIdx.x] = s_sum[0];
}

// one wave: the partials go to LDS with coalesced loads, lane 0 adds them in index order and rounds the mean to fp32 once
__global__ void __launch_bounds__(WAVE) split_fold_kernel(int P, int n_partials, const double* __restrict__ partials,
                                                          s3g_split_stats* __restrict__ stats) {
  __shared__ double s_part[S3G_SPLIT_MAX_PARTIALS];
  for (int k = threadIdx.x; k < n_partials; k += WAVE) s_part[k] = partials[k];
  wave_lds_sync();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 0; k < n_partials; k++) s += s_part[k];
    stats->thre = (float)(s / (double)P);
  }
}

// the number of dynamic Gaussians of the workgroup's 256 from wave ballots: thread 0 writes the word
__device__ __forceinline__ void block_dynamic_count(bool dyn, uint32_t* __restrict__ counts) {
  __shared__ uint32_t s_cnt[SW];
  const unsigned long long m = __ballot(dyn);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = (uint32_t)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

__global__ void __launch_bounds__(SB) split_mask_kernel(int P, const float* __restrict__ dx, const s3g_split_stats* __restrict__ stats,
                                                        unsigned char* __restrict__ mask, uint32_t* __restrict__ counts) {
  const long long i = (long long)blockIdx.x * SB + threadIdx.x;
  const float thre = stats->thre;
  bool dyn = false;
  if (i < P) {
    dyn = max_abs3(dx, i) > thre;          // mask = max_values > thre
    mask[i] = dyn ? 1 : 0;
  }
  block_dynamic_count(dyn, counts);
}

__global__ void __launch_bounds__(SB) split_count_kernel(int P, const unsigned char* __restrict__ mask, uint32_t* __restrict__ counts) {
  const long long i = (long long)blockIdx.x * SB + threadIdx.x;
  block_dynamic_count(i < P && mask[i] != 0, counts);
}

// One workgroup: every thread sums a contiguous run of block counts, the 1024 run sums are scanned in LDS, every thread then writes
// the exclusive prefixes of its run; counts[nb] and stats->n_dynamic receive the total.  ~10 k counts at 2.5 M Gaussians.
constexpr int SCAN_T = 1024;
__global__ void __launch_bounds__(SCAN_T) split_scan_kernel(int nb, uint32_t* __restrict__ counts, s3g_split_stats* __restrict__ stats) {
  __shared__ uint32_t s[SCAN_T];
  const int t = threadIdx.x;
  const int per = (nb + SCAN_T - 1) / SCAN_T;
  const int b0 = min(t * per, nb), b1 = min(b0 + per, nb);
  uint32_t sum = 0u;
  for (int b = b0; b < b1; b++) sum += counts[b];
  s[t] = sum;
  __syncthreads();
  for (int d = 1; d < SCAN_T; d <<= 1) {     // Hillis-Steele inclusive scan over the run sums
    const uint32_t v = t >= d ? s[t - d] : 0u;
    __syncthreads();
    s[t] += v;
    __syncthreads();
  }
  uint32_t run = s[t] - sum;
  for (int b = b0; b < b1; b++) {
    const uint32_t c = counts[b];
    counts[b] = run;
    run += c;
  }
  if (t == SCAN_T - 1) {
    counts[nb] = s[t];
    if (stats != nullptr) stats->n_dynamic = s[t];
  }
}

// ---- the row packer ---------------------------------------------------------------------------------------------------------------
// One wave per workgroup, 64 consecutive source Gaussians, an LDS tile of 64 x W floats (15.9 KB at W = 62: ten workgroups share a
// CU's LDS).  The tile is laid out in DESTINATION order -- the wave's dynamic rows first, then its static rows, each in source order --
// so each class leaves as one contiguous run.

// `n_rows x WIDTH` contiguous floats of one tensor into columns [col0, col0 + WIDTH) of the tile rows given by s_slot
template <int WIDTH, int W>
__device__ __forceinline__ void stage_rows(const float* __restrict__ src, int n_rows, int col0, float* __restrict__ tile,
                                           const int* __restrict__ s_slot, int lane) {
  const int n = n_rows * WIDTH;
  for (int e = lane; e < n; e += WAVE) {
    const int r = e / WIDTH, c = e - r * WIDTH;
    tile[s_slot[r] * W + col0 + c] = src[e];
  }
}

// n contiguous floats of the tile to dst: scalar stores up to the first 16-byte aligned address, 16-byte stores, a scalar tail
__device__ __forceinline__ void emit_run(const float* __restrict__ src, int n, float* __restrict__ dst, int lane) {
  const int head = min(n, (int)(((16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u) >> 2));
  if (lane < head) dst[lane] = src[lane];
  const int nvec = (n - head) >> 2;
  for (int v = lane; v < nvec; v += WAVE) {
    const int o = head + 4 * v;
    *reinterpret_cast<float4*>(dst + o) = make_float4(src[o], src[o + 1], src[o + 2], src[o + 3]);
  }
  const int done = head + 4 * nvec;
  if (lane < n - done) dst[done + lane] = src[done + lane];
}

template <int R>
__global__ void __launch_bounds__(WAVE) split_pack_kernel(const s3g_split_pack_plan p) {
  constexpr int W = 17 + 3 * R;
  __shared__ float tile[WAVE * W];
  __shared__ int s_slot[WAVE];
  const int lane = threadIdx.x;
  const long long i0 = (long long)blockIdx.x * WAVE;
  const int rows = (int)min((long long)WAVE, (long long)p.P - i0);     // >= 1: the grid has ceil(P / 64) workgroups
  int nd = rows;                     // rows of the first run
  long long row_a = i0, row_b = 0;   // first destination row of each run
  int slot = lane;
  if (p.mask != nullptr) {
    const bool dyn = lane < rows && p.mask[i0 + lane] != 0;
    const unsigned long long md = __ballot(dyn), below = (1ull << lane) - 1ull;
    const int dyn_below = __popcll(md & below);
    nd = __popcll(md);
    slot = dyn ? dyn_below : nd + (lane - dyn_below);
    // dynamic rows in front of this wave: the block's scanned offset + the block's earlier waves (full ones: they precede row i0 < P)
    const long long blk = i0 / SB;
    const int wave_in_block = (int)((i0 - blk * SB) / WAVE);
    uint32_t before = p.block_offsets[blk];
    for (int k = 0; k < wave_in_block; k++) before += (uint32_t)__popcll(__ballot(p.mask[blk * SB + k * WAVE + lane] != 0));
    row_a = (long long)before;
    row_b = i0 - (long long)before;
  }
  s_slot[lane] = slot;
  wave_lds_sync();

  {  // x y z (= xyz + dx, one fp32 add) and the three zero normals
    const float* __restrict__ xyz = p.xyz + i0 * 3;
    const float* __restrict__ dx = p.dx != nullptr ? p.dx + i0 * 3 : nullptr;
    const int n = rows * 3;
    for (int e = lane; e < n; e += WAVE) {
      const int r = e / 3, c = e - r * 3;
      float v = xyz[e];
      if (dx != nullptr) v = v + dx[e];
      float* row = tile + s_slot[r] * W;
      row[c] = v;
      row[3 + c] = 0.f;
    }
  }
  stage_rows<3, W>(p.f_dc + i0 * 3, rows, 6, tile, s_slot, lane);       // [P,1,3]: its transpose(1, 2).flatten(1) is itself
  if (R > 0) {                                                          // [P,R,3] -> [3,R] per row
    const float* __restrict__ fr = p.f_rest + i0 * (3 * R);
    const int n = rows * 3 * R;
    for (int e = lane; e < n; e += WAVE) {
      const int r = e / (3 * R), c = e - r * (3 * R);
      const int k = c / 3, ch = c - k * 3;
      tile[s_slot[r] * W + 9 + ch * R + k] = fr[e];
    }
  }
  stage_rows<1, W>(p.opacity + i0, rows, 9 + 3 * R, tile, s_slot, lane);
  stage_rows<3, W>(p.scaling + i0 * 3, rows, 10 + 3 * R, tile, s_slot, lane);
  stage_rows<4, W>(p.rotation + i0 * 4, rows, 13 + 3 * R, tile, s_slot, lane);
  wave_lds_sync();

  // (a run that does not fit can only come from offsets of another mask: it is dropped, never written past the end)
  if (nd > 0 && p.out_a != nullptr && row_a + nd <= (long long)p.rows_a) emit_run(tile, nd * W, p.out_a + row_a * W, lane);
  if (p.mask != nullptr && rows - nd > 0 && p.out_b != nullptr && row_b >= 0 && row_b + (rows - nd) <= (long long)p.rows_b)
    emit_run(tile + nd * W, (rows - nd) * W, p.out_b + row_b * W, lane);
}

}  // namespace s3g

using namespace s3g;

extern "C" size_t s3g_split_count_words(int P) { return (size_t)split_blocks(P) + 1; }

extern "C" size_t s3g_split_workspace_bytes(int P) {
  (void)P;
  return (size_t)S3G_SPLIT_MAX_PARTIALS * sizeof(double);
}

extern "C" int s3g_split_classify(int P, const float* dx, unsigned char* mask, uint32_t* block_offsets, s3g_split_stats* stats,
                                  void* workspace, void* stream_) {
  if (P < 0) {
    set_error("s3g_split_classify: P = %d", P);
    return S3G_ERR_INVALID_ARG;
  }
  if (P == 0) return S3G_OK;
  if (!dx || !mask || !block_offsets || !stats || !workspace) {
    set_error("s3g_split_classify: NULL dx, mask, block_offsets, stats or workspace");
    return S3G_ERR_INVALID_ARG;
  }
  hipStream_t stream = (hipStream_t)stream_;
  double* partials = reinterpret_cast<double*>(workspace);
  const int nb = split_blocks(P), np = split_partials(P);
  hipLaunchKernelGGL(split_partial_kernel, dim3(np), dim3(SB), 0, stream, P, dx, split_blocks_per_partial(P), partials);
  S3G_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(split_fold_kernel, dim3(1), dim3(WAVE), 0, stream, P, np, (const double*)partials, stats);
  S3G_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(split_mask_kernel, dim3(nb), dim3(SB), 0, stream, P, dx, (const s3g_split_stats*)stats, mask, block_offsets);
  S3G_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(split_scan_kernel, dim3(1), dim3(SCAN_T), 0, stream, nb, block_offsets, stats);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" int s3g_split_mask_offsets(int P, const unsigned char* mask, uint32_t* block_offsets, s3g_split_stats* stats, void* stream_) {
  if (P < 0) {
    set_error("s3g_split_mask_offsets: P = %d", P);
    return S3G_ERR_INVALID_ARG;
  }
  if (P == 0) return S3G_OK;
  if (!mask || !block_offsets) {
    set_error("s3g_split_mask_offsets: NULL mask or block_offsets");
    return S3G_ERR_INVALID_ARG;
  }
  hipStream_t stream = (hipStream_t)stream_;
  const int nb = split_blocks(P);
  hipLaunchKernelGGL(split_count_kernel, dim3(nb), dim3(SB), 0, stream, P, mask, block_offsets);
  S3G_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(split_scan_kernel, dim3(1), dim3(SCAN_T), 0, stream, nb, block_offsets, stats);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" int s3g_split_pack_rows(const s3g_split_pack_plan* plan, void* stream_) {
  if (!plan) {
    set_error("s3g_split_pack_rows: NULL plan");
    return S3G_ERR_INVALID_ARG;
  }
  const s3g_split_pack_plan& p = *plan;
  const int R = p.sh_rest;
  if (p.P < 0 || !(R == 0 || R == 3 || R == 8 || R == 15)) {
    set_error("s3g_split_pack_rows: P = %d, sh_rest = %d (0, 3, 8 or 15)", p.P, R);
    return S3G_ERR_INVALID_ARG;
  }
  if (p.P == 0) return S3G_OK;
  if (!p.xyz || !p.f_dc || (R > 0 && !p.f_rest) || !p.opacity || !p.scaling || !p.rotation) {
    set_error("s3g_split_pack_rows: NULL xyz, f_dc, f_rest, opacity, scaling or rotation");
    return S3G_ERR_INVALID_ARG;
  }
  if (p.rows_a < 0 || p.rows_b < 0 ||
      (p.mask != nullptr ? (!p.block_offsets || (!p.out_a && !p.out_b) || (!p.out_a && p.rows_a > 0) || (!p.out_b && p.rows_b > 0))
                         : (!p.out_a || p.rows_a < p.P))) {
    set_error("s3g_split_pack_rows: a mask needs its block offsets and an output for every row; without a mask out_a holds P rows "
              "(rows_a = %d, rows_b = %d, P = %d)", p.rows_a, p.rows_b, p.P);
    return S3G_ERR_INVALID_ARG;
  }
  const dim3 grid((unsigned)(((long long)p.P + WAVE - 1) / WAVE)), block(WAVE);
  hipStream_t stream = (hipStream_t)stream_;
  switch (R) {
    case 0: hipLaunchKernelGGL(split_pack_kernel<0>, grid, block, 0, stream, p); break;
    case 3: hipLaunchKernelGGL(split_pack_kernel<3>, grid, block, 0, stream, p); break;
    case 8: hipLaunchKernelGGL(split_pack_kernel<8>, grid, block, 0, stream, p); break;
    default: hipLaunchKernelGGL(split_pack_kernel<15>, grid, block, 0, stream, p); break;
  }
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}
