/*
 * s3g_split.h -- C ABI of the dynamic / static point-cloud split (libs3g.so): the motion classification and the PLY vertex table.
 *
 * What the reference computes when it exports the decomposed scene (GaussianModel.save_ply_split, scene/gaussian_model.py:277-348,
 * called by utils/video_utils.py:243-250) and when its training loop logs "dynamic point" (train.py:445-452), for dx [P,3]:
 *
 *   max_values = max(|dx|, dim=1)            gaussian_model.py:291-292      m_i = max(|dx_i0|, |dx_i1|, |dx_i2|)
 *   thre       = mean(max_values)            :293
 *   mask       = max_values > thre           :295                           strict
 *   dynamic    = np.where(mask)[0], static = np.where(~mask)[0]             :298-301: both in ascending source order
 *   per class, one vertex row per Gaussian   :261-272, 304-319
 *        [ x y z | 0 0 0 | f_dc (3) | f_rest channel-major (3 R) | opacity | scale (3) | rot (4) ],   x y z = xyz + dx (:289)
 *   with f_rest stored [P, R, 3] and written as transpose(1, 2).flatten(1), i.e. [3, R] per row; R = (degree + 1)^2 - 1.
 *   It fills its structured arrays through list(map(tuple, attributes)): one Python tuple per Gaussian, after seven boolean-index
 *   gathers and seven device-to-host copies per class.  save_ply (:258-275) builds the same table without dx and without a mask.
 *
 * ARITHMETIC OF THE THRESHOLD.  m_i in fp32; thre = fp32(sum_i (double)m_i / P): the sum is accumulated in float64 and rounded to fp32
 * ONCE.  The order of the sum is fixed by P alone: partial k (at most S3G_SPLIT_MAX_PARTIALS of them) covers a contiguous run of whole
 * 256-Gaussian blocks, thread t of its workgroup adds the elements t, t + 256, ... of the run in ascending order, the 256 thread sums
 * are folded by a fixed tree, and the partials are added in index order by one thread.  No floating-point atomics: two runs are
 * bit-identical.  (torch.mean in fp32 may differ from this in the last bit of thre; a point moves only if its m_i lies in between.)
 *
 * ORDER CONTRACT.  Destination rows come from an exclusive scan of per-block dynamic counts -- no atomic slot counters:
 *      dynamic Gaussian i -> row  #{dynamic before i}       of out_a
 *      static  Gaussian i -> row  i - #{dynamic before i}   of out_b
 * which is the order of np.where(mask)[0] / np.where(~mask)[0], and bit-reproducible.
 *
 * Launches.  s3g_split_classify: partial sums -> fold (one wave) -> mask bytes + per-block counts (wave ballots + popcount) -> scan
 * (one workgroup).  s3g_split_pack_rows: ONE launch; a wave owns 64 consecutive source Gaussians, loads each tensor's contiguous
 * 64 x width floats coalesced into an LDS tile of 64 x W floats -- transposing the SH block and compacting its dynamic rows in front
 * of its static rows on the way in -- and writes the tile out as at most two contiguous runs, with 16-byte stores from the first
 * 16-byte aligned address of a run on.  Non-finite dx gives an unspecified classification; nothing is indexed by data.
 */
#ifndef S3G_SPLIT_H
#define S3G_SPLIT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define S3G_SPLIT_BLOCK 256         /* Gaussians per counted block: block_offsets has one word per block and one for the total */
#define S3G_SPLIT_MAX_PARTIALS 512  /* float64 partial sums of the threshold, whatever P */

/* What the classification leaves on the device; it needs to reach the host only where a caller sizes an output from it. */
typedef struct s3g_split_stats {
  float thre;          /* the threshold: mean of m_i, float64 sum rounded once */
  uint32_t n_dynamic;  /* #{i : m_i > thre} */
} s3g_split_stats;

/* Number of uint32 words of `block_offsets` for P Gaussians: ceil(P / S3G_SPLIT_BLOCK) + 1 (at least 2). */
size_t s3g_split_count_words(int P);

/* Bytes of device workspace s3g_split_classify needs (the float64 partials); the same for every P. */
size_t s3g_split_workspace_bytes(int P);

/* dx: [P,3] fp32 device, contiguous.  mask: [P] bytes, 1 = dynamic.  block_offsets: s3g_split_count_words(P) words: word b = number of
 * dynamic Gaussians in front of block b, the last word = n_dynamic.  stats: one record on the device.  workspace:
 * s3g_split_workspace_bytes(P) bytes on the device, contents irrelevant on entry.  Asynchronous on `stream`, no host read.
 * P == 0 returns S3G_OK without a launch (no pointer is looked at); P < 0 or a NULL pointer is refused with S3G_ERR_INVALID_ARG
 * before any device call. */
int s3g_split_classify(int P, const float* dx, unsigned char* mask, uint32_t* block_offsets, s3g_split_stats* stats,
                       void* workspace, void* stream);

/* The count and scan stages alone, for a mask that came from elsewhere (any non-zero byte = dynamic).  stats may be NULL; only its
 * n_dynamic is written.  Same refusals as s3g_split_classify. */
int s3g_split_mask_offsets(int P, const unsigned char* mask, uint32_t* block_offsets, s3g_split_stats* stats, void* stream);

typedef struct s3g_split_pack_plan {
  int P;                         /* source Gaussians */
  int sh_rest;                   /* R, rows of f_rest per Gaussian: 0, 3, 8 or 15 (SH degree 0..3); a table row has 17 + 3 R floats */
  int rows_a;                    /* rows out_a holds: n_dynamic (read back from the stats or the offsets' last word) with a mask, P without */
  int rows_b;                    /* rows out_b holds: P - n_dynamic with a mask; unused without */
  const float* xyz;              /* [P,3] */
  const float* dx;               /* [P,3] or NULL: x y z = xyz + dx (one fp32 add) / xyz */
  const float* f_dc;             /* [P,1,3] */
  const float* f_rest;           /* [P,R,3]; may be NULL when R == 0 */
  const float* opacity;          /* [P,1] */
  const float* scaling;          /* [P,3] */
  const float* rotation;         /* [P,4] */
  const unsigned char* mask;     /* [P] or NULL: every row goes to out_a in source order */
  const uint32_t* block_offsets; /* from s3g_split_classify / s3g_split_mask_offsets OF THIS MASK; required with a mask */
  float* out_a;                  /* [rows_a, W] */
  float* out_b;                  /* [rows_b, W]; with a mask, either may be NULL where it holds no row */
} s3g_split_pack_plan;

/* Builds the vertex table(s) in one launch.  Writes exactly the rows named above, nothing else: a run of rows that would not fit into
 * rows_a / rows_b (offsets that belong to another mask) is left out, never written past the end.  P == 0 returns S3G_OK without a
 * launch; P < 0, another sh_rest, a NULL input, a mask without offsets, negative rows_a / rows_b, rows_a < P without a mask or a
 * missing output is S3G_ERR_INVALID_ARG before any device call.  All pointers need 4-byte alignment only. */
int s3g_split_pack_rows(const s3g_split_pack_plan* plan, void* stream);

#ifdef __cplusplus
}
#endif
#endif
