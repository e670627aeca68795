/*
 * s3g_depthvis.h -- C ABI of the coloured depth frames (libs3g.so): the reference's depth_visualizer (utils/video_utils.py:27-33),
 * visualize_depth(frame, opacity, lo, hi, depth_curve_fn = -log(x + 1e-6)) of utils/visualization_tools.py:117-194 with the turbo map
 * and matte_background = False, written as uint8 into one camera's tile of a strip (include/s3g_frames.h), and the opacity-weighted
 * percentiles visualize_cmap takes its bounds from when lo or hi is None.  tests/depthvis_ref.py restates all of it in numpy.
 *
 * Weighted percentiles (weighted_percentile, visualization_tools.py:106-114, made order-independent and exact).  D, A: [H,W] fp32.
 *   w_i   = llrint(min(max(A_i, 0), 1) * 2^30), a NaN opacity gives 0           integer weights
 *   pixels with a NaN depth take no part; -0.0 counts as +0.0
 *   the others ascending by depth, ties by row-major pixel index; S_j the exact integer prefix sums, total = S_last
 *   q     = p * (double(total) / 100.0)                                          p = 0.5 and 99.5
 *   r(p)  = np.interp(q, S, x) in double: x_0 if q < S_0; x_last if q >= S_last (total = 0 included); else with j the last index
 *           such that S_j <= q:  x_j if q == S_j or x_{j+1} == x_j, else ((x_{j+1} - x_j) / (S_{j+1} - S_j)) * (q - S_j) + x_j,
 *           in that order, no contraction.  No pixel takes part: NaN.
 * H * W <= 2^23, so every sum is below 2^53 and exact in a double.  No float atomics: integer sums only, two runs are bit-identical.
 *
 * The route: a radix selection for both p at once, 8 bits per pass over the order-preserving 32-bit key of a depth.  Each pass is
 * one image-sized kernel (64-bit integer LDS atomics into a workgroup's histogram of weight sums over the pixels that still match a
 * target's prefix; one partial histogram per workgroup, stored with plain vector stores) and one single-workgroup kernel that folds
 * and scans the partials and fixes the next digit of both targets.  That leaves the crossing key K and the weight G below it; a last
 * image-sized pass finds the largest key below K, and the lowest pixel index of group K with its weight w_first; a last
 * single-workgroup kernel evaluates r: x(K) unless G + w_first > q, in which case K's first pixel is the crossing one and r
 * interpolates between the predecessor key and K with slope 1 / w_first.  Ten launches, no host read.
 *
 * Colours.  lo, hi: the given bound, or lo = r(0.5) - 2^-23, hi = r(99.5) + 2^-23 in double.
 *   v    = -log(double(D) + 1e-6); c_lo, c_hi likewise from lo, hi
 *   t    = (v - min(c_lo, c_hi)) / |c_hi - c_lo|, clipped to [0,1], NaN -> 0
 *   u    = t * double(A)   (A as is; no A: u = t)
 *   idx  = min(max(trunc(u * 256), 0), 255);  bytes = TABLE[idx];  a NaN u gives (0,0,0)
 * TABLE[k][c] = trunc(255 * clip(turbo[k][c], 0, 1)) of matplotlib's 256-entry turbo table (s3g_depth_turbo_table).
 * byte(row, x, c) goes to dst + row * dst_row_bytes + (dst_col + x) * 3 + c.  Packed path -- one lane takes 4 consecutive pixels of a
 * row: a 16-byte load per plane, three dword stores -- when W % 4 == 0, depth (and alpha) are 16-byte aligned, and dst + dst_col * 3 and
 * dst_row_bytes are multiples of 4; the byte path otherwise.  The choice is made on the host and is uniform over a workgroup.  On
 * neither path does a store touch a byte outside [dst_col * 3, (dst_col + W) * 3) of a row.
 */
#ifndef S3G_DEPTHVIS_H
#define S3G_DEPTHVIS_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define S3G_DEPTHVIS_MAX_PIXELS (1 << 23)

/* Bytes of device workspace s3g_depth_percentiles needs for an H x W image; 0 for H or W < 1 or H * W > S3G_DEPTHVIS_MAX_PIXELS. */
size_t s3g_depthvis_workspace_bytes(int H, int W);

/* depth, alpha: [H,W] fp32 on the device, contiguous.  bounds_out: two doubles on the device, r(0.5) and r(99.5).  workspace:
 * s3g_depthvis_workspace_bytes(H, W) bytes on the device, 8-byte aligned, contents irrelevant on entry.  Asynchronous on `stream`, no
 * host read.  Writes bounds_out and the workspace, nothing else.  Refused with S3G_ERR_INVALID_ARG before any device call: H or W < 1,
 * H * W > S3G_DEPTHVIS_MAX_PIXELS, a NULL depth / alpha / bounds_out / workspace. */
int s3g_depth_percentiles(int H, int W, const float* depth, const float* alpha, double* bounds_out, void* workspace, void* stream);

/* depth: [H,W] fp32 on the device; alpha: likewise or NULL (no weighting).  lo, hi: the bounds; a NaN means "take it from bounds":
 * bounds[0] - 2^-23 for lo, bounds[1] + 2^-23 for hi, where bounds is what s3g_depth_percentiles left on the device (it may be NULL
 * when neither is NaN).  dst: base of the [H, dst_row_bytes] uint8 strip; dst_col: first pixel column of the tile.  Asynchronous on
 * `stream`, no host read.  Writes the tile's bytes, nothing else.  Refused with S3G_ERR_INVALID_ARG before any device call: H or
 * W < 1, H * W beyond 2^30, a NULL depth / dst, a NaN bound with NULL bounds or with NULL alpha, dst_col < 0 or
 * (dst_col + W) * 3 > dst_row_bytes. */
int s3g_depth_colors(int H, int W, const float* depth, const float* alpha, double lo, double hi, const double* bounds,
                     unsigned char* dst, long long dst_row_bytes, int dst_col, void* stream);

/* The 768 bytes of TABLE, [256][3], in host memory. */
const unsigned char* s3g_depth_turbo_table(void);

#ifdef __cplusplus
}
#endif
#endif
