/*
 * s3g_frames.h -- C ABI of the evaluation video frames (libs3g.so): the uint8 strips the reference hands to its video writer
 * (utils/video_utils.py:439-499 save_seperate_videos over the lists utils/video_utils.py:176-201 fills), written straight from the
 * [C,H,W] fp32 renders on the device.
 *
 * What the reference computes for key k and timestamp i with n = num_cams cameras, everything fp32, on the host after five to seven
 * `.permute(1,2,0).cpu().numpy()` copies per frame:
 *
 *   frames = render_results[k][i*n : (i+1)*n]              n arrays [H,W,C]; C = 3, and C = 1 for "depths"
 *   strip  = to8b(np.concatenate(frames, axis=1))          [H, n*W, C] uint8 -> writer.append_data(strip)
 *   to8b(x) = (255 * np.clip(x, 0, 1)).astype(np.uint8)    one fp32 multiply, then truncation (visualization_tools.py:68-71)
 *   "depths": each frame is divided in place by ITS OWN max() first (video_utils.py:196-198): one correctly rounded fp32 division
 *
 * Here one call composes up to S3G_FRAME_MAX_JOBS "jobs" of one camera -- one job per key -- so a frame costs at most two launches
 * for all of its keys.  A job reads one contiguous [C,H,W] fp32 image and writes its tile, the columns [dst_col, dst_col + W) of an
 * [H, row, C] uint8 strip, where the other cameras' tiles live in the same rows:
 *
 *   byte(row, x, c) at dst + row * dst_row_bytes + (dst_col + x) * C + c
 *                 = (uint8)(int)(255.0f * fminf(fmaxf(q, 0), 1)),   q = normalize ? src[c,row,x] / m : src[c,row,x]
 *
 * with m the maximum over the job's whole image (all C planes; numpy's max(): a NaN anywhere makes m NaN).
 *
 * Defined where the reference's result is an undefined NaN-to-uint8 cast: a NaN pixel gives 0, and a normalised image whose maximum
 * is <= 0 or NaN gives an all-zero tile.
 *
 * Two launches at most, no atomics.  Pass 1 (only if some job has `normalize`; one launch for all such jobs) leaves per-workgroup
 * partial maxima in the workspace, stored with plain vector stores; pass 2 folds a job's partials in its prologue and converts.  The
 * maximum does not depend on the order of its operands: two runs are bit-identical and m equals numpy's max().
 * Pass 2 takes, per job, the packed path -- one lane converts 4 consecutive pixels of a row: one 16-byte load per plane, C dword
 * stores of 4 C packed bytes -- when W % 4 == 0, src is 16-byte aligned, and dst + dst_col * C and dst_row_bytes are multiples of 4;
 * every other job takes the byte path (one pixel per lane, C byte stores).  The choice is made on the host, per job, and is uniform
 * over a workgroup.  On neither path does a store touch a byte outside [dst_col * C, (dst_col + W) * C) of a row.
 */
#ifndef S3G_FRAMES_H
#define S3G_FRAMES_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define S3G_FRAME_MAX_JOBS 8

typedef struct s3g_frame_job {
  const float* src;         /* [channels,H,W] fp32 device, contiguous */
  unsigned char* dst;       /* base of the [H, dst_row_bytes] uint8 strip on the device */
  long long dst_row_bytes;  /* bytes from one strip row to the next: num_cams * W * channels for a contiguous strip */
  int dst_col;              /* first pixel column of this camera's tile: cam * W */
  int channels;             /* 1 or 3 */
  int normalize;            /* non-zero: divide by the image's own maximum first ("depths") */
  int reserved;             /* 0 */
} s3g_frame_job;

/* Bytes of device workspace s3g_frame_tiles needs for `jobs` jobs of H x W images (the per-workgroup partial maxima); 0 for
 * H, W or jobs < 1. */
size_t s3g_frame_workspace_bytes(int H, int W, int jobs);

/* job: `jobs` entries on the HOST, read before the call returns (the table travels in the kernel arguments: no upload).
 * maxima: `jobs` floats on the device or NULL; entry j receives m of job j if that job has `normalize`, and is left alone otherwise.
 * workspace: s3g_frame_workspace_bytes(H, W, jobs) bytes on the device, contents irrelevant on entry; may be NULL when no job has
 * `normalize`.  Asynchronous on `stream`, no host read, nothing waits.  Writes the jobs' tiles, maxima and the workspace, nothing else.
 * Refused with S3G_ERR_INVALID_ARG before any device call: jobs outside 1..S3G_FRAME_MAX_JOBS, H or W < 1, H * W beyond 2^30, a NULL
 * job table / src / dst, channels other than 1 or 3, dst_col < 0 or (dst_col + W) * channels > dst_row_bytes, and a NULL workspace
 * with a normalised job. */
int s3g_frame_tiles(int H, int W, int jobs, const s3g_frame_job* job, float* maxima, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
