// LiDAR scene set-up (include/s3g_lidar.h): the per-camera depth maps of a sweep (readWaymoInfo, scene/dataset_readers.py:838-887 of
// the reference) and the initial point cloud (:843-856, 909-911, GridSample3D :1102-1144).  Run once per scene, HBM- and launch-bound:
// a sweep of 170 k rows is 6.8 MB, a 1066 x 1600 winner image 6.8 MB per camera.
#include "common.hpp"

#include "../../include/s3g_lidar.h"

namespace s3g {

constexpr int LB = S3G_LIDAR_BLOCK;     // rows (= threads) per workgroup: four waves
constexpr int LW = LB / WAVE;
static_assert(LB == 256 && LW == 4, "the block counts below are written for four waves");

static inline int lidar_blocks(long long n) { return n > 0 ? (int)((n + LB - 1) / LB) : 1; }
// blocks per partial of the grid range, a function of n alone
static inline int lidar_blocks_per_partial(int n) { return (lidar_blocks(n) + S3G_LIDAR_MAX_PARTIALS - 1) / S3G_LIDAR_MAX_PARTIALS; }
static inline int lidar_partials(int n) {
  const int per = lidar_blocks_per_partial(n);
  return (lidar_blocks(n) + per - 1) / per;
}

struct LidarEval {
  double world[3];
  double z;       // pix.z
  int pixel;      // iy * W + ix
};
enum { LIDAR_KEPT = 1, LIDAR_COUNTED = 2 };

// r-th row of a row-major [3][4] rigid transform applied to v: the 3-term sum in float64, k ascending, the translation last
__device__ __forceinline__ double lidar_row34(const double* __restrict__ M, int r, const double v[3]) {
  return ((M[4 * r] * v[0] + M[4 * r + 1] * v[1]) + M[4 * r + 2] * v[2]) + M[4 * r + 3];
}

// THE arithmetic of the family (the contract of include/s3g_lidar.h): every kernel below calls this and nothing else computes.
// -> LIDAR_KEPT if row i passes the x range (e.world is then set), | LIDAR_COUNTED if it also lands in the H x W image of the
// camera (w2c, K) (e.z and e.pixel are then set).  w2c == nullptr: the world point only.  NaNs fail every comparison: not counted.
__device__ __forceinline__ int lidar_eval(const s3g_lidar_sweep& s, int i, const double* __restrict__ w2c, const double* __restrict__ K,
                                          int H, int W, LidarEval& e) {
  const float* __restrict__ row = s.rows + (long long)i * s.row_stride + s.point_offset;
  const double p[3] = {(double)row[0], (double)row[1], (double)row[2]};
  if (!(p[0] > s.x_min && p[0] < s.x_max)) return 0;
  for (int r = 0; r < 3; r++) e.world[r] = lidar_row34(s.l2w, r, p);
  if (w2c == nullptr) return LIDAR_KEPT;
  double cam[3], pix[3];
  for (int r = 0; r < 3; r++) cam[r] = lidar_row34(w2c, r, e.world);
  for (int r = 0; r < 3; r++) pix[r] = (K[3 * r] * cam[0] + K[3 * r + 1] * cam[1]) + K[3 * r + 2] * cam[2];
  if (!(pix[2] > 0.0)) return LIDAR_KEPT;
  const double u = pix[0] / pix[2], v = pix[1] / pix[2];
  if (!(u >= 0.0 && u < (double)W && v >= 0.0 && v < (double)H)) return LIDAR_KEPT;
  e.z = pix[2];
  e.pixel = (int)v * W + (int)u;      // 0 <= (int)v < H, 0 <= (int)u < W by the test above
  return LIDAR_KEPT | LIDAR_COUNTED;
}

// ---- depth maps -------------------------------------------------------------------------------------------------------------------
// grid (ceil(N / 256), V): one thread per (row, camera); the camera index is uniform, its matrices come from the kernel arguments
__global__ void __launch_bounds__(LB) lidar_winner_kernel(const s3g_lidar_sweep s, const s3g_lidar_cams c, int* __restrict__ winner) {
  const long long i = (long long)blockIdx.x * LB + threadIdx.x;
  if (i >= s.N) return;
  const int v = blockIdx.y;
  LidarEval e;
  if (lidar_eval(s, (int)i, c.w2c[v], c.K[v], c.H, c.W, e) & LIDAR_COUNTED)
    atomicMax(winner + (long long)v * c.H * c.W + e.pixel, (int)i);     // the highest source row: numpy's last assignment
}

// grid (ceil(H W / 256), V): one thread per pixel; the winner's pix.z is recomputed by the same function, to the same bits
__global__ void __launch_bounds__(LB) lidar_depth_kernel(const s3g_lidar_sweep s, const s3g_lidar_cams c, const int* __restrict__ winner,
                                                         float* __restrict__ depth) {
  const int hw = c.H * c.W;
  const long long px = (long long)blockIdx.x * LB + threadIdx.x;
  if (px >= hw) return;
  const int v = blockIdx.y;
  const long long at = (long long)v * hw + px;
  const int i = winner[at];
  float z = 0.f;
  if (i >= 0 && i < s.N) {
    LidarEval e;
    if (lidar_eval(s, i, c.w2c[v], c.K[v], c.H, c.W, e) & LIDAR_COUNTED) z = (float)e.z;
  }
  depth[at] = z;
}

// ---- counting, scanning (shared by the cloud and the grid sample) -------------------------------------------------------------------
// the number of kept rows of the workgroup's 256 from wave ballots: thread 0 writes the word
__device__ __forceinline__ void lidar_block_count(bool keep, uint32_t* __restrict__ counts) {
  __shared__ uint32_t s_cnt[LW];
  const unsigned long long m = __ballot(keep);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = (uint32_t)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// the number of kept rows of the workgroup in front of this thread
__device__ __forceinline__ uint32_t lidar_block_rank(bool keep) {
  __shared__ uint32_t s_cnt[LW];
  const unsigned long long m = __ballot(keep);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) s_cnt[w] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t before = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
  for (int k = 0; k < w; k++) before += s_cnt[k];
  return before;
}

// One workgroup: counts[b] <- base + the number of kept rows in front of block b, counts[nb] <- base + their total, where base is
// *running (0 without one); *running <- the same total.  Every thread sums a contiguous run of block counts, the 1024 run sums are
// scanned in LDS, every thread then writes the prefixes of its run.
constexpr int LSCAN_T = 1024;
__global__ void __launch_bounds__(LSCAN_T) lidar_scan_kernel(int nb, uint32_t* __restrict__ counts, uint32_t* __restrict__ running) {
  __shared__ uint32_t s[LSCAN_T];
  const int t = threadIdx.x;
  const uint32_t base = running != nullptr ? *running : 0u;      // read by every thread before the barriers, written after them
  const int per = (nb + LSCAN_T - 1) / LSCAN_T;
  const int b0 = min(t * per, nb), b1 = min(b0 + per, nb);
  uint32_t sum = 0u;
  for (int b = b0; b < b1; b++) sum += counts[b];
  s[t] = sum;
  __syncthreads();
  for (int d = 1; d < LSCAN_T; d <<= 1) {     // Hillis-Steele inclusive scan over the run sums
    const uint32_t v = t >= d ? s[t - d] : 0u;
    __syncthreads();
    s[t] += v;
    __syncthreads();
  }
  uint32_t run = base + s[t] - sum;
  for (int b = b0; b < b1; b++) {
    const uint32_t cnt = counts[b];
    counts[b] = run;
    run += cnt;
  }
  if (t == LSCAN_T - 1) {
    counts[nb] = base + s[t];
    if (running != nullptr) *running = base + s[t];
  }
}

// ---- the cloud ------------------------------------------------------------------------------------------------------------------------
struct LidarBox {
  double lo[3], hi[3];
};

__device__ __forceinline__ bool lidar_in_cloud(const s3g_lidar_sweep& s, long long i, const LidarBox& box, LidarEval& e) {
  if (i >= s.N) return false;
  if (!(lidar_eval(s, (int)i, nullptr, nullptr, 0, 0, e) & LIDAR_KEPT)) return false;
  bool in = true;
  for (int k = 0; k < 3; k++) in = in && e.world[k] >= box.lo[k] && e.world[k] <= box.hi[k];
  return in;
}

__global__ void __launch_bounds__(LB) lidar_cloud_count_kernel(const s3g_lidar_sweep s, const LidarBox box, uint32_t* __restrict__ counts) {
  LidarEval e;
  lidar_block_count(lidar_in_cloud(s, (long long)blockIdx.x * LB + threadIdx.x, box, e), counts);
}

__global__ void __launch_bounds__(LB) lidar_cloud_scatter_kernel(const s3g_lidar_sweep s, const LidarBox box,
                                                                 const uint32_t* __restrict__ offsets, double* __restrict__ cloud,
                                                                 int capacity) {
  LidarEval e;
  const bool keep = lidar_in_cloud(s, (long long)blockIdx.x * LB + threadIdx.x, box, e);
  const uint32_t dst = offsets[blockIdx.x] + lidar_block_rank(keep);
  if (keep && dst < (uint32_t)capacity) {
    double* __restrict__ o = cloud + (size_t)dst * 3;
    o[0] = e.world[0];
    o[1] = e.world[1];
    o[2] = e.world[2];
  }
}

// ---- the grid sample --------------------------------------------------------------------------------------------------------------------
// np.around(p / voxel_size): IEEE division, round half to even; an exact integer held in a double
__device__ __forceinline__ double lidar_quantize(double p, double voxel) { return rint(p / voxel); }

// partial k = the range of q over the rows of blocks [k per, (k + 1) per): thread t folds rows t, t + 256, ... in ascending order,
// then a fixed tree over the 256 thread values.  Layout of a partial: min x y z, max x y z.
__global__ void __launch_bounds__(LB) lidar_range_partial_kernel(int n, const double* __restrict__ cloud, double voxel, int blocks_per,
                                                                 double* __restrict__ partials) {
  __shared__ double s_v[6][LB];
  const int t = threadIdx.x;
  const long long start = (long long)blockIdx.x * blocks_per * LB;
  const long long end = min((long long)n, start + (long long)blocks_per * LB);
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (long long i = start + t; i < end; i += LB)
    for (int k = 0; k < 3; k++) {
      const double q = lidar_quantize(cloud[i * 3 + k], voxel);
      lo[k] = fmin(lo[k], q);
      hi[k] = fmax(hi[k], q);
    }
  for (int k = 0; k < 3; k++) {
    s_v[k][t] = lo[k];
    s_v[3 + k][t] = hi[k];
  }
  __syncthreads();
  for (int d = LB / 2; d > 0; d >>= 1) {
    if (t < d)
      for (int k = 0; k < 3; k++) {
        s_v[k][t] = fmin(s_v[k][t], s_v[k][t + d]);
        s_v[3 + k][t] = fmax(s_v[3 + k][t], s_v[3 + k][t + d]);
      }
    __syncthreads();
  }
  if (t < 6) partials[blockIdx.x * 6 + t] = s_v[t][0];
}

// one wave: lanes 0..5 each fold one column of the partials in index order; lanes 0..2 then write qmin and b = max - min
__global__ void __launch_bounds__(WAVE) lidar_range_fold_kernel(int n_partials, const double* __restrict__ partials,
                                                                s3g_lidar_grid_stats* __restrict__ stats) {
  __shared__ double s_r[6];
  const int t = threadIdx.x;
  if (t < 6) {
    double r = partials[t];
    for (int k = 1; k < n_partials; k++) r = t < 3 ? fmin(r, partials[k * 6 + t]) : fmax(r, partials[k * 6 + t]);
    s_r[t] = r;
  }
  wave_lds_sync();
  if (t < 3) {
    // (the caller bounds |p / voxel_size| below 2^53 on the host: the casts are exact)
    stats->qmin[t] = (int64_t)s_r[t];
    stats->b[t] = (int64_t)s_r[3 + t] - (int64_t)s_r[t];
  }
}

__global__ void __launch_bounds__(LB) lidar_keys_kernel(int n, const double* __restrict__ cloud, double voxel,
                                                        const s3g_lidar_grid_stats* __restrict__ stats, int64_t* __restrict__ keys) {
  const long long i = (long long)blockIdx.x * LB + threadIdx.x;
  if (i >= n) return;
  int64_t q[3];
  for (int k = 0; k < 3; k++) q[k] = (int64_t)lidar_quantize(cloud[i * 3 + k], voxel) - stats->qmin[k];
  const int64_t by = stats->b[1], bz = stats->b[2];
  keys[i] = q[0] * by * bz + q[1] * bz + q[2];
}

__device__ __forceinline__ bool lidar_is_head(int n, const int64_t* __restrict__ keys, long long j) {
  return j < n && (j == 0 || keys[j] != keys[j - 1]);
}

__global__ void __launch_bounds__(LB) lidar_heads_count_kernel(int n, const int64_t* __restrict__ keys, uint32_t* __restrict__ counts) {
  lidar_block_count(lidar_is_head(n, keys, (long long)blockIdx.x * LB + threadIdx.x), counts);
}

__global__ void __launch_bounds__(LB) lidar_gather_kernel(int n, const int64_t* __restrict__ keys, const int64_t* __restrict__ perm,
                                                          const double* __restrict__ cloud, const uint32_t* __restrict__ offsets,
                                                          float* __restrict__ out, int out_rows) {
  const long long j = (long long)blockIdx.x * LB + threadIdx.x;
  const bool head = lidar_is_head(n, keys, j);
  const uint32_t dst = offsets[blockIdx.x] + lidar_block_rank(head);
  if (!head || dst >= (uint32_t)out_rows) return;
  const int64_t src = perm[j];
  if (src < 0 || src >= n) return;
  for (int k = 0; k < 3; k++) out[(size_t)dst * 3 + k] = (float)cloud[src * 3 + k];
}

static bool sweep_ok(const char* who, const s3g_lidar_sweep* s) {
  if (!s) {
    set_error("%s: NULL sweep", who);
    return false;
  }
  if (s->N < 0 || s->point_offset < 0 || (long long)s->row_stride < (long long)s->point_offset + 3) {
    set_error("%s: N = %d, row_stride = %d, point_offset = %d (N >= 0, point_offset >= 0, row_stride >= point_offset + 3)", who, s->N,
              s->row_stride, s->point_offset);
    return false;
  }
  if (s->N > 0 && !s->rows) {
    set_error("%s: NULL rows", who);
    return false;
  }
  return true;
}

static bool cams_ok(int V, int H, int W) {
  return V >= 1 && V <= S3G_LIDAR_MAX_CAMS && H >= 1 && W >= 1 && (long long)V * H * W < (1ll << 31);
}

}  // namespace s3g

using namespace s3g;

extern "C" size_t s3g_lidar_depth_workspace_bytes(int V, int H, int W) {
  return cams_ok(V, H, W) ? (size_t)V * H * W * sizeof(int) : 0;
}

extern "C" int s3g_lidar_depth_maps(const s3g_lidar_sweep* sweep, const s3g_lidar_cams* cams, float* depth, void* workspace,
                                    void* stream_) {
  if (!sweep_ok("s3g_lidar_depth_maps", sweep)) return S3G_ERR_INVALID_ARG;
  if (!cams || !depth || !workspace) {
    set_error("s3g_lidar_depth_maps: NULL cams, depth or workspace");
    return S3G_ERR_INVALID_ARG;
  }
  if (!cams_ok(cams->V, cams->H, cams->W)) {
    set_error("s3g_lidar_depth_maps: V = %d (1..%d), H = %d, W = %d (>= 1, V H W < 2^31)", cams->V, S3G_LIDAR_MAX_CAMS, cams->H, cams->W);
    return S3G_ERR_INVALID_ARG;
  }
  hipStream_t stream = (hipStream_t)stream_;
  const s3g_lidar_sweep& s = *sweep;
  const s3g_lidar_cams& c = *cams;
  int* winner = reinterpret_cast<int*>(workspace);
  S3G_HIP_CHECK(hipMemsetAsync(winner, 0xFF, s3g_lidar_depth_workspace_bytes(c.V, c.H, c.W), stream));      // every word -1
  if (s.N > 0) {
    hipLaunchKernelGGL(lidar_winner_kernel, dim3(lidar_blocks(s.N), c.V), dim3(LB), 0, stream, s, c, winner);
    S3G_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(lidar_depth_kernel, dim3(lidar_blocks((long long)c.H * c.W), c.V), dim3(LB), 0, stream, s, c, (const int*)winner,
                     depth);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" size_t s3g_lidar_count_words(int n) { return (size_t)lidar_blocks(n) + 1; }

extern "C" int s3g_lidar_cloud_add(const s3g_lidar_sweep* sweep, const double* aabb, double* cloud, int capacity, uint32_t* total,
                                   uint32_t* block_offsets, void* stream_) {
  if (!sweep_ok("s3g_lidar_cloud_add", sweep)) return S3G_ERR_INVALID_ARG;
  if (capacity < 0) {
    set_error("s3g_lidar_cloud_add: capacity = %d", capacity);
    return S3G_ERR_INVALID_ARG;
  }
  if (sweep->N == 0) return S3G_OK;
  if (!aabb || !cloud || !total || !block_offsets) {
    set_error("s3g_lidar_cloud_add: NULL aabb, cloud, total or block_offsets");
    return S3G_ERR_INVALID_ARG;
  }
  hipStream_t stream = (hipStream_t)stream_;
  const s3g_lidar_sweep& s = *sweep;
  LidarBox box;
  for (int k = 0; k < 3; k++) {
    box.lo[k] = aabb[k];
    box.hi[k] = aabb[3 + k];
  }
  const int nb = lidar_blocks(s.N);
  hipLaunchKernelGGL(lidar_cloud_count_kernel, dim3(nb), dim3(LB), 0, stream, s, box, block_offsets);
  S3G_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(lidar_scan_kernel, dim3(1), dim3(LSCAN_T), 0, stream, nb, block_offsets, total);
  S3G_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(lidar_cloud_scatter_kernel, dim3(nb), dim3(LB), 0, stream, s, box, (const uint32_t*)block_offsets, cloud, capacity);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" size_t s3g_lidar_grid_workspace_bytes(int n) {
  (void)n;
  return (size_t)S3G_LIDAR_MAX_PARTIALS * 6 * sizeof(double);
}

extern "C" int s3g_lidar_grid_range(int n, const double* cloud, double voxel_size, s3g_lidar_grid_stats* stats, void* workspace,
                                    void* stream_) {
  if (n < 1 || !(voxel_size > 0.0)) {
    set_error("s3g_lidar_grid_range: n = %d (>= 1), voxel_size = %g (> 0)", n, voxel_size);
    return S3G_ERR_INVALID_ARG;
  }
  if (!cloud || !stats || !workspace) {
    set_error("s3g_lidar_grid_range: NULL cloud, stats or workspace");
    return S3G_ERR_INVALID_ARG;
  }
  hipStream_t stream = (hipStream_t)stream_;
  double* partials = reinterpret_cast<double*>(workspace);
  const int np = lidar_partials(n);
  hipLaunchKernelGGL(lidar_range_partial_kernel, dim3(np), dim3(LB), 0, stream, n, cloud, voxel_size, lidar_blocks_per_partial(n), partials);
  S3G_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(lidar_range_fold_kernel, dim3(1), dim3(WAVE), 0, stream, np, (const double*)partials, stats);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" int s3g_lidar_grid_keys(int n, const double* cloud, double voxel_size, const s3g_lidar_grid_stats* stats, int64_t* keys,
                                   void* stream_) {
  if (n < 1 || !(voxel_size > 0.0)) {
    set_error("s3g_lidar_grid_keys: n = %d (>= 1), voxel_size = %g (> 0)", n, voxel_size);
    return S3G_ERR_INVALID_ARG;
  }
  if (!cloud || !stats || !keys) {
    set_error("s3g_lidar_grid_keys: NULL cloud, stats or keys");
    return S3G_ERR_INVALID_ARG;
  }
  hipLaunchKernelGGL(lidar_keys_kernel, dim3(lidar_blocks(n)), dim3(LB), 0, (hipStream_t)stream_, n, cloud, voxel_size, stats, keys);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" int s3g_lidar_grid_heads(int n, const int64_t* sorted_keys, uint32_t* block_offsets, void* stream_) {
  if (n < 1) {
    set_error("s3g_lidar_grid_heads: n = %d (>= 1)", n);
    return S3G_ERR_INVALID_ARG;
  }
  if (!sorted_keys || !block_offsets) {
    set_error("s3g_lidar_grid_heads: NULL sorted_keys or block_offsets");
    return S3G_ERR_INVALID_ARG;
  }
  hipStream_t stream = (hipStream_t)stream_;
  const int nb = lidar_blocks(n);
  hipLaunchKernelGGL(lidar_heads_count_kernel, dim3(nb), dim3(LB), 0, stream, n, sorted_keys, block_offsets);
  S3G_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(lidar_scan_kernel, dim3(1), dim3(LSCAN_T), 0, stream, nb, block_offsets, (uint32_t*)nullptr);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" int s3g_lidar_grid_gather(int n, const int64_t* sorted_keys, const int64_t* perm, const double* cloud,
                                     const uint32_t* block_offsets, float* out, int out_rows, void* stream_) {
  if (n < 1 || out_rows < 0) {
    set_error("s3g_lidar_grid_gather: n = %d (>= 1), out_rows = %d (>= 0)", n, out_rows);
    return S3G_ERR_INVALID_ARG;
  }
  if (!sorted_keys || !perm || !cloud || !block_offsets || (out_rows > 0 && !out)) {
    set_error("s3g_lidar_grid_gather: NULL sorted_keys, perm, cloud, block_offsets or out");
    return S3G_ERR_INVALID_ARG;
  }
  if (out_rows == 0) return S3G_OK;
  hipLaunchKernelGGL(lidar_gather_kernel, dim3(lidar_blocks(n)), dim3(LB), 0, (hipStream_t)stream_, n, sorted_keys, perm, cloud,
                     block_offsets, out, out_rows);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}
