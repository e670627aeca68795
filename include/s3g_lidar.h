/*
 * s3g_lidar.h -- C ABI of the LiDAR scene set-up (libs3g.so): the per-camera depth maps of a sweep and the initial point cloud.
 *
 * What the reference computes once, before its first iteration (readWaymoInfo, scene/dataset_readers.py:824-977, and GridSample3D /
 * get_split_point, :1102-1144), in numpy float64 on the host, for sweep t with rows [N, 10] fp32 (the point in columns 3:6):
 *
 *   keep      = x_min < p.x < x_max                          :843-847   strict, on the fp32 ego-frame value
 *   world     = R_l2w p + t_l2w                              :853-856   float64
 *   per camera v of the timestamp:
 *     cam     = R_w2c world + t_w2c,  pix = K cam            :862-870   w2c = np.linalg.inv(c2w), made by the caller on the host
 *     counted = pix.z > 0, 0 <= u < W, 0 <= v < H            :872-881   u = pix.x / pix.z, v = pix.y / pix.z
 *     depth_map[(int)v, (int)u] = pix.z                      :885-886   numpy keeps the LAST assignment: the counted point with the
 *                                                                       HIGHEST source row wins the pixel; empty pixels are 0
 *   cloud    += world rows with aabb_min <= world <= aabb_max in all three axes   :904-911, sweeps in order, rows in source order
 *   GridSample3D(cloud, voxel_size = 0.013)                  :1102-1144
 *     q       = np.around(p / voxel_size)                    round half to even, per axis
 *     q      -= min(q);  b = max(q)                          b is the maximum, NOT the extent + 1
 *     label   = q.x * b.y * b.z + q.y * b.z + q.z            two distinct voxels can therefore share a label (q.z = b.z and q.y + 1,
 *                                                            q.z = 0 collide): reproduced here, not repaired
 *     one point per distinct label, in ascending label order
 *
 * ARITHMETIC CONTRACT.  One __device__ function (lidar_eval, csrc/lidar.hip) holds all of the arithmetic and every kernel calls it:
 *   the three fp32 coordinates are widened to float64 (exact); every 3-term product sum is float64, k ascending, the translation
 *   added last:  world_r = ((R[r][0] p0 + R[r][1] p1) + R[r][2] p2) + t[r];  cam likewise from world;  pix_r = (K[r][0] cam0 +
 *   K[r][1] cam1) + K[r][2] cam2;  u and v are IEEE float64 divisions; the pixel is the truncation of v and u.  No contraction: the
 *   library is built with -ffp-contract=off and the function asks for no fma.  The x-range test compares the float64 widening of the
 *   fp32 p.x with the float64 bounds.  A depth map holds fp32(pix.z), one rounding (what train.py:392's .float() makes of the
 *   reference's float64 map); the second kernel RECOMPUTES pix.z of the winning row with the same function, to the same bits.
 *   numpy's matmul (BLAS) may sum in another order or contract: world coordinates then differ in the last float64 bit, which changes
 *   a decision only for a point within that distance of a pixel edge, a range bound, the aabb or a rounding boundary.
 *
 * ORDER CONTRACT.  The winner of a pixel is an integer atomicMax of the source row: order-independent, bit-reproducible.  Cloud rows
 * and grid representatives get their destination from per-block ballot counts and an exclusive scan (on top of a device-held running
 * total for the cloud): no atomic slot counters, no floating-point atomics, sizes that decide an order fixed by the row count alone.
 *
 * REPRESENTATIVE RULE (a deliberate difference).  The reference keeps, per label, whichever row numpy's unstable introsort puts
 * first.  Here the rows are sorted STABLY by label and the representative is the row with the lowest position in the accumulated
 * cloud.  The set of labels, their count and their order are the reference's; the point standing for a label may be another point of
 * the same label.
 *
 * HOST READS.  s3g_lidar_depth_maps and s3g_lidar_cloud_add: none.  The grid sample needs three by its caller (lidar.LidarCloud.finish):
 * the kept count (4 bytes, sizes the launches), s3g_lidar_grid_stats (48 bytes, the 2^53 guard) and the number of labels M (4 bytes,
 * sizes the output).
 */
#ifndef S3G_LIDAR_H
#define S3G_LIDAR_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define S3G_LIDAR_MAX_CAMS 8        /* cameras per s3g_lidar_depth_maps call: their matrices travel as kernel arguments */
#define S3G_LIDAR_BLOCK 256         /* rows per counted block: block_offsets has one word per block and one for the total */
#define S3G_LIDAR_MAX_PARTIALS 512  /* partial minima / maxima of the grid range, whatever n */

/* One sweep: a [N, row_stride] fp32 table on the device, the point in columns point_offset .. point_offset + 2 (the reference's raw
 * .bin rows: stride 10, offset 3; a plain [N,3] table: stride 3, offset 0).  4-byte alignment is enough.  l2w: rows 0..2 of the 4x4
 * lidar-to-world matrix, row-major [3][4], float64, HOST values (passed to the kernels by value). */
typedef struct s3g_lidar_sweep {
  const float* rows;
  int N;
  int row_stride;
  int point_offset;
  int reserved;
  double x_min, x_max;   /* a point counts iff x_min < p.x < x_max */
  double l2w[12];
} s3g_lidar_sweep;

/* The V cameras of the sweep's timestamp, HOST values: w2c[v] = rows 0..2 of inv(c2w) row-major [3][4]; K[v] row-major [3][3]. */
typedef struct s3g_lidar_cams {
  int V, H, W;
  int reserved;
  double w2c[S3G_LIDAR_MAX_CAMS][12];
  double K[S3G_LIDAR_MAX_CAMS][9];
} s3g_lidar_cams;

/* What s3g_lidar_grid_range leaves on the device: qmin = min over the cloud of rint(p / voxel_size) per axis, b = max - min. */
typedef struct s3g_lidar_grid_stats {
  int64_t qmin[3];
  int64_t b[3];
} s3g_lidar_grid_stats;

/* Bytes of the winner image (int32 [V,H,W]); 0 for arguments s3g_lidar_depth_maps would refuse. */
size_t s3g_lidar_depth_workspace_bytes(int V, int H, int W);

/* depth: [V,H,W] fp32 on the device, written completely (0 where no point lands; N == 0 gives zeros and sweep->rows may be NULL).
 * workspace: s3g_lidar_depth_workspace_bytes(V,H,W) bytes on the device, contents irrelevant on entry.  Launches: fill of the winner
 * image with -1, one thread per (row, camera) with an integer atomicMax of the row, one thread per pixel.  Asynchronous on `stream`,
 * no host read.  Refused with S3G_ERR_INVALID_ARG before any device call: a NULL pointer, N < 0 (N >= 2^31 cannot be expressed),
 * row_stride < point_offset + 3, point_offset < 0, V outside 1..S3G_LIDAR_MAX_CAMS, H or W < 1, V H W >= 2^31. */
int s3g_lidar_depth_maps(const s3g_lidar_sweep* sweep, const s3g_lidar_cams* cams, float* depth, void* workspace, void* stream);

/* Number of uint32 words of `block_offsets` for n rows: ceil(n / S3G_LIDAR_BLOCK) + 1 (at least 2). */
size_t s3g_lidar_count_words(int n);

/* Appends the world points of the sweep that pass the x range and lie inside aabb (HOST, [2][3]: min then max, inclusive, float64
 * compare) to cloud ([capacity,3] float64, device) behind the *total rows already there, in source order, and adds their number to
 * *total (one uint32 on the device, zeroed by the caller before the first sweep).  block_offsets: s3g_lidar_count_words(N) words of
 * device workspace.  Launches: per-block ballot counts, one-workgroup scan on top of *total, scatter.  No host read: the caller
 * guarantees capacity >= the sum of the N of every sweep added (a row that would not fit is dropped, never written past the end).
 * N == 0 returns S3G_OK without a launch.  Refusals as s3g_lidar_depth_maps, plus capacity < 0 or >= 2^31. */
int s3g_lidar_cloud_add(const s3g_lidar_sweep* sweep, const double* aabb, double* cloud, int capacity, uint32_t* total,
                        uint32_t* block_offsets, void* stream);

/* Bytes of device workspace of s3g_lidar_grid_range (the partial minima / maxima); the same for every n. */
size_t s3g_lidar_grid_workspace_bytes(int n);

/* stats <- the range of rint(cloud / voxel_size) over the n rows ([n,3] float64).  Partial k covers a contiguous run of whole blocks,
 * a fixed tree folds its 256 thread values, one thread folds the partials in index order.  n < 1, voxel_size not > 0, NULL: refused. */
int s3g_lidar_grid_range(int n, const double* cloud, double voxel_size, s3g_lidar_grid_stats* stats, void* workspace, void* stream);

/* keys[i] = (q.x - qmin.x) b.y b.z + (q.y - qmin.y) b.z + (q.z - qmin.z) in int64: the reference's float64 label, exact while
 * b.x b.y b.z < 2^53 (the caller reads stats back and refuses a larger cloud by name). */
int s3g_lidar_grid_keys(int n, const double* cloud, double voxel_size, const s3g_lidar_grid_stats* stats, int64_t* keys, void* stream);

/* sorted_keys: the keys after a STABLE sort.  block_offsets (s3g_lidar_count_words(n) words): word b = number of run heads (rows whose
 * key differs from the row before; row 0 is one) in front of block b, the last word = M, the number of distinct labels. */
int s3g_lidar_grid_heads(int n, const int64_t* sorted_keys, uint32_t* block_offsets, void* stream);

/* out[m] = fp32(cloud[perm[j]]) for the m-th head j: perm [n] int64 is the source row of every sorted row.  out: [out_rows,3] fp32;
 * a head beyond out_rows or a perm entry outside [0, n) is skipped, never followed. */
int s3g_lidar_grid_gather(int n, const int64_t* sorted_keys, const int64_t* perm, const double* cloud, const uint32_t* block_offsets,
                          float* out, int out_rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif
