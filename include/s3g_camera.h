/*
 * s3g_camera.h -- C ABI of the camera gradients of the rasterizer and of the pose map that feeds them (libs3g.so).
 *
 * s3g_raster_backward* return a gradient for every per-Gaussian input and none for the camera: the world-to-view matrix, the
 * full projection matrix and the camera centre of s3g_raster_inputs.  Every per-Gaussian quantity those three gradients need
 * is an output of that backward already (dL_dmean2D, dL_dconic, dL_ddepth, dL_dcolor); s3g_camera_backward forms the
 * per-Gaussian terms from them and sums over P.  s3g_pose_apply maps a six-parameter correction of a camera onto its three
 * matrices, s3g_pose_apply_backward takes the gradient back to the six parameters.
 *
 * Conventions: row-vector 4x4 matrices indexed [4*row + column] like s3g_raster_inputs (scene/cameras.py:59-63), i.e.
 * t_i = sum_k mean_k view[4k+i] + view[12+i]  and  h_j = sum_k mean_k proj[4k+j] + proj[12+j].
 */
#ifndef S3G_CAMERA_H
#define S3G_CAMERA_H
#include <stddef.h>

#include "s3g_raster.h"
#ifdef __cplusplus
extern "C" {
#endif

#define S3G_CAMERA_GRAD_DOUBLES 35 /* dL/dview [16], dL/dproj [16], dL/dcampos [3] */

/* Camera gradients of one rasterizer backward, from that backward's per-Gaussian outputs.  Reads [P]-sized arrays only:
 * in->means3D, the forward's cov3D (in->cov3D_precomp, else the geometry arena) and `clamped` flags (geometry arena), radii,
 * the four gradient arrays (dL_dmean2D [P,3], dL_dconic [P,2,2], dL_ddepth [P], dL_dcolor [P,3]) and, when in->shs is given,
 * in->shs (in->D, in->M) and in->cam_pos.  A Gaussian with radii > 0 contributes, evaluated in double from the fp32 inputs:
 *   view, through t = mean * view:   g_t = the covariance path's dL/dt exactly as the geometry backward forms it (clamped t.x / t.y
 *                                    and the x / y gradient masks of the 1.3 * tan(fov) clamp included), + dL_ddepth on z;
 *                                    view[4k+i] += mean_k g_t[i],  view[12+i] += g_t[i]
 *   view, through W of T = W J:      view[4k+i] += sum_j dL/dT[k][j] J[i][j]       (the transposed product that is not dL/dJ)
 *   proj:                            p_w = 1 / (h_w + 1e-7), (g2x, g2y) = dL_dmean2D (NDC units):
 *                                    dL/dh = (g2x p_w, g2y p_w, -, -(h_x g2x + h_y g2y) p_w^2), scattered with mean_k and 1
 *   campos (in->shs given):          minus the direction term the geometry backward adds to dL_dmean3D (SH backward through
 *                                    dir = mean - campos, normalised; `clamped` channels masked)
 * and every Gaussian p, whatever its radius:   campos -= g_dir[p]   (colours precomputed from mean - campos outside the
 * rasterizer: g_dir is that computation's gradient with respect to the mean, direction part only).
 * view[3,7,11,15] and proj[2,6,10,14] enter no product of the forward: written as 0.
 * Every gradient array may be NULL and drops its terms; with all four NULL, `in` needs P only and radii / geometry_arena may be
 * NULL.  A piece whose incoming gradients are all zero for a Gaussian contributes exactly 0 whatever cov3D / clamped hold (an
 * overflowed asynchronous forward leaves zeros in the gradients and nothing defined in the arena).
 * Two launches: one partial sum of the 35 values per workgroup, stored to `workspace`
 * (s3g_camera_backward_workspace_bytes(P) bytes, no initialisation needed) in an order fixed by P, then one workgroup adds
 * them in a fixed order.  No floating-point atomics: bit-identical run to run.  `out` (device, 35 doubles) is written, not
 * accumulated.  P == 0: zeros, no launch. */
size_t s3g_camera_backward_workspace_bytes(int P);
int s3g_camera_backward(const s3g_raster_inputs* in, const int* radii, const void* geometry_arena,
                        const float* dL_dmean2D, const float* dL_dconic, const float* dL_ddepth, const float* dL_dcolor,
                        const float* g_dir /* [P,3] or NULL */, void* workspace,
                        double* out /* [35] device: dL/dview[16], dL/dproj[16], dL/dcampos[3] */, void* stream);

/* Pose map.  delta6 = (omega, tau) (device, 6 doubles) is a left perturbation in the camera frame,
 * x_cam' = Exp(omega) x_cam + tau; with D = [Exp(omega) tau; 0 1]:
 *     view' = view0 D^T,   proj' = view' (view0^-1 proj0)  (rigid inverse),   campos' = -t' R'^T  (t' = view'[12..14], R' = its 3x3).
 * Exp is Rodrigues' formula with sin(th)/th and (1 - cos th)/th^2 as series in th^2 below th^2 = 1e-4, so that delta = 0 has a
 * finite and correct derivative.  Everything in double, rounded once to fp32: view [16], proj [16], campos [3] (device).
 * s3g_pose_apply_backward runs the same map in forward mode, one tangent per parameter, and dots each with g35 (device,
 * 35 doubles in s3g_camera_backward's layout): g_delta6 [6] (device doubles), written.  One single-workgroup launch each. */
int s3g_pose_apply(const double* delta6, const float* view0, const float* proj0, float* view, float* proj, float* campos,
                   void* stream);
int s3g_pose_apply_backward(const double* delta6, const float* view0, const float* proj0, const double* g35,
                            double* g_delta6, void* stream);

/* The pose map for V cameras (a rig's cameras of one timestamp), one launch each way, one workgroup per camera.  delta [N,6]
 * doubles (device) holds every camera's correction; rows (device, V ints, each in 0 .. N-1) says which row camera v takes.
 * view0s / proj0s [V,16] floats in, views / projs [V,16] and camposs [V,3] floats out; g35 [V,35] doubles in, g_delta [V,6]
 * doubles out (row v = the gradient of delta row rows[v]; scattering it is the caller's).  Camera v's outputs are bit-identical
 * to s3g_pose_apply / s3g_pose_apply_backward on its own row and matrices.  V is not limited; V == 0: nothing is launched. */
int s3g_pose_apply_views(int V, const double* delta, const int* rows, const float* view0s, const float* proj0s, float* views,
                         float* projs, float* camposs, void* stream);
int s3g_pose_apply_backward_views(int V, const double* delta, const int* rows, const float* view0s, const float* proj0s,
                                  const double* g35, double* g_delta, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* S3G_CAMERA_H */
