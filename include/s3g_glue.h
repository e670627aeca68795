/*
 * s3g_glue.h -- C ABI of the fused per-Gaussian render glue (libs3g.so).
 *
 *   s3g_glue_forward / s3g_glue_backward  <- the PyTorch glue of render()
 *       /root/reference/gaussian_renderer/__init__.py:99-115 :
 *         scales   = exp(_scaling)                       (scaling_activation,  scene/gaussian_model.py:44)
 *         rotation = normalize(_rotation)                (rotation_activation = F.normalize, :53)
 *         opacity  = sigmoid(_opacity)                   (opacity_activation, :49)
 *         shs      = cat(f_dc, f_rest) + dshs            (get_features :120-124, deformation.py:157-162)
 *         colors   = clamp_min(eval_sh(deg, shs^T, normalize(xyz - campos)) + 0.5, 0)   (utils/sh_utils.py:57-112)
 *       (directions use the UN-deformed xyz, like the reference, gaussian_renderer/__init__.py:110)
 *   and the ~80 elementwise kernels autograd replays for them, as ONE kernel per direction.
 */
#ifndef S3G_GLUE_H
#define S3G_GLUE_H
#ifdef __cplusplus
extern "C" {
#endif

/* All device fp32.  f_dc [P,1,3], f_rest [P,15,3], dshs [P,16,3] or NULL, xyz [P,3], campos [3],
 * log_scales [P,3], rot_raw [P,4], opacity_logit [P]  ->  colors [P,3], scales [P,3], rot [P,4], opacity [P].
 * dshs_abs_sum (slotted accumulator of S3G_SUM_DOUBLES doubles as in s3g_loss.h, caller zeroes, may be NULL): += sum |dshs| -- the numerator of the reference's
 * lambda_dshs * mean|dshs| regulariser (/root/reference/train.py:407-410), taken while dshs streams through anyway. */
int s3g_glue_forward(int P, int deg, const float* f_dc, const float* f_rest, const float* dshs, const float* xyz,
                     const float* campos, const float* log_scales, const float* rot_raw, const float* opacity_logit,
                     float* colors, float* scales, float* rot, float* opacity, double* dshs_abs_sum, void* stream);

/* Upstream g_colors [P,3], g_scales [P,3], g_rot [P,4], g_opacity [P] (any may be NULL = zero) ->
 * g_f_dc [P,1,3], g_f_rest [P,15,3], g_dshs [P,16,3] (may be NULL), g_xyz [P,3], g_log_scales [P,3], g_rot_raw [P,4],
 * g_opacity_logit [P]; all written.  `colors`, `scales`, `rot`, `opacity` are the forward outputs.
 * g_dshs_l1 (device float, may be NULL): upstream gradient of mean|dshs|; g_dshs += *g_dshs_l1 / (48 P) * sign(dshs). */
int s3g_glue_backward(int P, int deg, const float* f_dc, const float* f_rest, const float* dshs, const float* xyz,
                      const float* campos, const float* rot_raw, const float* colors, const float* scales,
                      const float* rot, const float* opacity, const float* g_colors, const float* g_scales,
                      const float* g_rot, const float* g_opacity, float* g_f_dc, float* g_f_rest, float* g_dshs,
                      float* g_xyz, float* g_log_scales, float* g_rot_raw, float* g_opacity_logit,
                      const float* g_dshs_l1, void* stream);

/*
 *   s3g_glue_forward_views / s3g_glue_backward_views: the same glue for V cameras that share one timestamp -- a batch of
 *   views (/root/reference/train.py:327-437, opt.batch_size) whose deformation was evaluated once.  1 <= V <= S3G_GLUE_MAX_VIEWS.
 *   f_dc, f_rest and dshs are read once per Gaussian, the activations are written once, sum|dshs| is taken once.
 */
#define S3G_GLUE_MAX_VIEWS 8

/* As s3g_glue_forward with campos [V,3]; colors: HOST array of V device pointers, each [P,3], each written.  A view's colours
 * are bit-identical to s3g_glue_forward with that view's campos. */
int s3g_glue_forward_views(int P, int deg, int V, const float* f_dc, const float* f_rest, const float* dshs, const float* xyz,
                           const float* campos, const float* log_scales, const float* rot_raw, const float* opacity_logit,
                           float* const* colors, float* scales, float* rot, float* opacity, double* dshs_abs_sum, void* stream);

/* colors: host array of the V forward outputs; g_colors: host array of V upstream gradients [P,3], any entry may be NULL = zero
 * (the array itself may not).  One each of the other upstream gradients and of every output; all outputs written.
 *   g_f_dc | g_f_rest | g_dshs row (k, c) = sum_v basis_v[k] * dRGB_v[c]       g_xyz = sum_v (direction term of view v)
 * both accumulated in fp32, view 0 first, left to right, every product rounded before it is added: the result equals the fp32
 * sum of V s3g_glue_backward calls, and with V = 1 that call bit for bit.  The g_dshs_l1 term is added after the sum. */
int s3g_glue_backward_views(int P, int deg, int V, const float* f_dc, const float* f_rest, const float* dshs, const float* xyz,
                            const float* campos, const float* rot_raw, const float* const* colors, const float* scales,
                            const float* rot, const float* opacity, const float* const* g_colors, const float* g_scales,
                            const float* g_rot, const float* g_opacity, float* g_f_dc, float* g_f_rest, float* g_dshs,
                            float* g_xyz, float* g_log_scales, float* g_rot_raw, float* g_opacity_logit,
                            const float* g_dshs_l1, void* stream);

/* s3g_glue_backward_views with the gradient of every view's camera centre beside it (pose refinement of a rig's cameras): every
 * output of s3g_glue_backward_views, bit for bit, and
 *   g_campos[v] = -sum_p t_v[p]      (device, [V,3] doubles, written)
 * where t_v[p] is view v's own fp32 term of g_xyz[p] (the colours depend on xyz - campos_v only).  tv: HOST array of V device
 * pointers, each [P,3] floats of scratch that receives t_v (zeros for a view whose g_colors entry is NULL); workspace:
 * s3g_glue_backward_views_campos_workspace_bytes(P, V) bytes, no initialisation needed.  The sum over P runs in double in the
 * order s3g_camera_backward uses for its g_dir term, so g_campos[v] equals, bit for bit, what s3g_glue_backward for view v alone
 * followed by s3g_camera_backward(g_dir = its g_xyz) returns in out[32..34].  Three launches (the backward, one partial sum per
 * workgroup and view, one fold workgroup per view); no floating-point atomics, bit-identical run to run.  P == 0: zeros, no
 * launch. */
size_t s3g_glue_backward_views_campos_workspace_bytes(int P, int V);
int s3g_glue_backward_views_campos(int P, int deg, int V, const float* f_dc, const float* f_rest, const float* dshs,
                                   const float* xyz, const float* campos, const float* rot_raw, const float* const* colors,
                                   const float* scales, const float* rot, const float* opacity, const float* const* g_colors,
                                   const float* g_scales, const float* g_rot, const float* g_opacity, float* g_f_dc,
                                   float* g_f_rest, float* g_dshs, float* g_xyz, float* g_log_scales, float* g_rot_raw,
                                   float* g_opacity_logit, const float* g_dshs_l1, float* const* tv, void* workspace,
                                   double* g_campos /* [V,3] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
