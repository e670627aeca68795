/*
 * s3g_flow.h -- C ABI of the scene-flow colours (libs3g.so): the per-Gaussian RGB the reference paints its forward / backward
 * "emergent flow" images with (utils/video_utils.py:252-299 over utils/visualization_tools.py:242-322).
 *
 * What the reference computes for flow = dx_b - dx_a [P,3] with about 30 torch launches, a device-to-host copy, a host-to-device copy
 * and a host wait per image -- scene_flow_to_rgb(flow, background="bright", flow_max_radius=1.0), everything fp32:
 *
 *   1. f = (flow - min(flow)) / (max(flow) - min(flow) + 1e-6)          min / max over all 3P elements
 *   2. x = f[:,0], y = f[:,1], r = hypot(x, y), theta = atan2(y, x)      (z only enters through min / max)
 *   3. A = theta * 54 / (2 pi);  hue = the 55-entry cyclic colour wheel, interpolated linearly between entries trunc(A) and ceil(A)
 *   4. r <= 1: colour = 255 - r * (255 - hue);   r > 1: colour = hue / r;   colour / 255
 *
 * Why no table is needed: after step 1 every component lies in [0, 1), so theta is in [0, pi/2] and A in [0, 13.5]: only the
 * first of the wheel's six transitions, red (255,0,0) -> yellow (255,255,0) in 15 steps, can be reached, and on it entry k is
 * exactly (255, 17 k, 0) for k = 0..15 (the wheel's uint8 truncation changes nothing: 17 k is an integer).  The kernel evaluates
 * step 3 with 17 trunc(A) and 17 ceil(A) in place of the two table reads, in the reference's order of fp32 operations (r and theta
 * alone are evaluated in double and rounded to fp32 once, so that they sit within the last bit of any fp32 hypot / atan2); no address is
 * computed from data, so non-finite input cannot cause an out-of-range access (its colours are unspecified).  The table form, with the
 * wheel built by the reference's rule, lives in tests/flow_ref.py; tests/test_flow_cpu.py shows the two agree on the whole reachable domain.
 *
 * Two launches: pass 1 reduces min and max of dx_b - dx_a (16-byte loads where both pointers are 16-byte aligned, wave64 butterflies,
 * one (min, max) pair per workgroup stored with a plain vector store); pass 2 folds those few hundred pairs in its prologue and
 * evaluates steps 1-4 for one Gaussian per lane and trip, recomputing the difference instead of materialising it.  min and max do
 * not depend on the order of their operands and there is no floating-point atomic: two runs are bit-identical.
 */
#ifndef S3G_FLOW_H
#define S3G_FLOW_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of device workspace s3g_scene_flow_colors needs for P Gaussians (the per-workgroup partial pairs); non-decreasing in P,
 * 0 for P <= 0. */
size_t s3g_scene_flow_workspace_bytes(int P);

/* dx_a, dx_b: [P,3] fp32 device, contiguous.  colors: [P,3] fp32 device, written.  range: 2 floats on the device or NULL; receives
 * {min, max} of dx_b - dx_a.  workspace: s3g_scene_flow_workspace_bytes(P) bytes on the device, contents irrelevant on entry.
 * Asynchronous on `stream`, no host read: the range never leaves the device.  Writes colors, range and the workspace, nothing else.
 * P == 0 returns S3G_OK without a launch (no pointer is looked at); P < 0 or a NULL dx_a / dx_b / colors / workspace is refused with
 * S3G_ERR_INVALID_ARG before any device call. */
int s3g_scene_flow_colors(int P, const float* dx_a, const float* dx_b, float* colors, float* range, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
