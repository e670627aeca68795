/*
 * s3g_density.h -- C ABI of adaptive density control (libs3g.so): densify, prune and opacity reset.
 *
 * What the reference does every `densification_interval` iterations (train.py:494-516) with ~40 boolean-index / cat launches,
 * each boolean index hiding a `nonzero` host synchronisation and every tensor reallocated twice:
 *
 *   GaussianModel.densify        scene/gaussian_model.py:673-678   g = xyz_gradient_accum / denom, NaN -> 0
 *     densify_and_clone          :524-561   |g| >= th  and  max(exp(s)) <= percent_dense * extent  -> the row is appended once more
 *     densify_and_split          :496-522   g >= th    and  max(exp(s)) >  percent_dense * extent  -> two children replace the row:
 *                                           xyz' = R(q / |q|) (exp(s) o z) + xyz,  s' = log(exp(s) / (0.8 * 2)),  z ~ N(0, 1)
 *                                           (R: utils/general_utils.py:245-266 build_rotation), everything else copied
 *   GaussianModel.prune          :661-670   sigmoid(o) < min_opacity; and, only when max_screen_size is truthy,
 *                                           max_radii2D > max_screen_size  or  max(exp(s)) > 0.1 * extent
 *   prune_points / cat_tensors_to_optimizer / densification_postfix   :412-494   survivors keep their Adam moments, new rows get 0
 *   GaussianModel.reset_opacity  :350-353, 397-410   o = inverse_sigmoid(min(sigmoid(o), 0.01)), both moments 0
 *
 * Here one event is four launches: classify -> scan -> (the host reads three counts, 12 bytes, to size the outputs) -> apply.
 *
 * ORDER CONTRACT.  Destination rows come from an exclusive scan of per-workgroup class counts -- no atomic slot counters -- so the
 * output order is the reference's and bit-reproducible:
 *      [ kept originals, in order | clones, in order of their source | split children copy 1, in order of source | copy 2 ]
 * which is what densify_and_clone, then densify_and_split, then prune_points leave behind.  With n_keep = P - n_split - n_drop:
 *      original i (class KEEP or CLONE)  -> row  i - #{split or dropped rows before i}
 *      clone of i                        -> row  n_keep + #{clones before i}
 *      child k (0, 1) of split row i     -> row  n_keep + n_clone + k * n_split + #{splits before i}
 * The normal deviate of a child is row (k * n_split + #{splits before i}) of the noise: `.repeat(N, 1)` tiles the same way.
 */
#ifndef S3G_DENSITY_H
#define S3G_DENSITY_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define S3G_DENSITY_KEEP 0
#define S3G_DENSITY_CLONE 1
#define S3G_DENSITY_SPLIT 2
#define S3G_DENSITY_DROP 3

#define S3G_DENSITY_BLOCK 256      /* Gaussians per workgroup of classify / apply: block_counts has 3 words per such block */
#define S3G_DENSITY_MAX_TENSORS 16 /* per apply call */

/* Number of uint32 words of `block_counts` for P Gaussians: 3 * ceil(P / S3G_DENSITY_BLOCK) (at least 3). */
size_t s3g_density_count_words(int P);

/* Classify, densify mode.  One thread per Gaussian: cls[i] = KEEP / CLONE / SPLIT; block_counts[3 b + {0, 1, 2}] = number of
 * CLONE / SPLIT / DROP rows of workgroup b (wave ballots + popcount).  xyz_gradient_accum, denom: [P]; scaling: [P,3] (log scales).
 * scale_threshold = percent_dense * extent. */
int s3g_density_classify_densify(int P, const float* xyz_gradient_accum, const float* denom, const float* scaling,
                                 float grad_threshold, float scale_threshold, unsigned char* cls, uint32_t* block_counts,
                                 void* stream);

/* Classify, prune mode: cls[i] = KEEP / DROP.  opacity: [P] logits; max_radii2D: [P]; max_screen_size <= 0 switches the two size
 * tests off (the reference's `if max_screen_size:`); world_scale_threshold = 0.1 * extent. */
int s3g_density_classify_prune(int P, const float* opacity, const float* scaling, const float* max_radii2D, float min_opacity,
                               float max_screen_size, float world_scale_threshold, unsigned char* cls, uint32_t* block_counts,
                               void* stream);

/* Scan: block_counts becomes, in place, the exclusive prefix per class over the workgroups; totals[0..2] = number of CLONE / SPLIT /
 * DROP rows (device words; the one host read of an event).  One workgroup. */
int s3g_density_scan(int P, uint32_t* block_counts, uint32_t* totals, void* stream);

/* One per-Gaussian tensor of the apply launch.  The kernel knows nothing about which tensor is which: every row of `width` floats
 * moves as the order contract says; moments (all four pointers or none) follow survivors and are written as 0 for clones and
 * children.  children_rewritten != 0: the rows of split children are NOT copied -- the plan's xyz / scaling outputs, which the
 * kernel computes. */
typedef struct s3g_density_tensor {
  const float* src;           /* [P, width] */
  float* dst;                 /* [P_out, width] */
  const float* src_exp_avg;   /* or NULL */
  float* dst_exp_avg;
  const float* src_exp_avg_sq;
  float* dst_exp_avg_sq;
  int width;
  int children_rewritten;
} s3g_density_tensor;

typedef struct s3g_density_plan {
  int P;                         /* rows before */
  int n_clone;                   /* totals read back from s3g_density_scan */
  int n_split;
  int n_drop;
  const unsigned char* cls;      /* [P] from classify */
  const uint32_t* block_offsets; /* block_counts after s3g_density_scan */
  const unsigned char* table_src; /* byte-wide per-Gaussian flag (`_deformation_table`) or NULL */
  unsigned char* table_dst;       /* [P_out] */
  const float* xyz;              /* [P,3]  the three inputs of the split children; required when n_split > 0 */
  const float* scaling;          /* [P,3] */
  const float* rotation;         /* [P,4] */
  float* xyz_dst;                /* [P_out,3] same arrays as the `dst` of the xyz / scaling table entries */
  float* scaling_dst;            /* [P_out,3] */
  const float* noise;            /* [noise_rows,3] standard normal deviates, or NULL: Philox4x32-10 keyed on (seed, row) + Box-Muller */
  size_t noise_rows;             /* must be >= 2 * n_split when noise != NULL */
  uint64_t seed;
  float* noise_out;              /* optional [2 * n_split, 3]: the deviates actually used */
} s3g_density_plan;

/* Apply: ONE launch moves every tensor of the table (P_out = P + n_clone + n_split - n_drop rows each).  A wave owns 64 consecutive
 * source Gaussians and walks each tensor's contiguous 64 x width floats with coalesced loads; destination rows come from LDS. */
int s3g_density_apply(const s3g_density_plan* plan, int n, const s3g_density_tensor* tensors /* host array */, void* stream);

/* Opacity reset: opacity_out[i] = log(y / (1 - y)), y = min(sigmoid(opacity[i]), 0.01); exp_avg / exp_avg_sq (or NULL) zeroed in
 * place.  opacity_out may alias opacity. */
int s3g_density_reset_opacity(int P, const float* opacity, float* opacity_out, float* exp_avg, float* exp_avg_sq, void* stream);

#ifdef __cplusplus
}
#endif
#endif
