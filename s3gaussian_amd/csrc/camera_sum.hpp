// The launch shape of the sums over P behind the camera gradients, shared by camera_backward_kernel (raster_camera_backward.hip)
// and glue_views_campos_sum_kernel (glue_views_camera.hip): the second promises the bits of the first, and the order of a sum is
// fixed by these three.
#pragma once

namespace s3g {

constexpr int CAM_THREADS = 256;
constexpr int CAM_MAX_BLOCKS = 512;    // above P = 131 072 the workgroups stride over the Gaussians (two workgroups per CU)

static inline int cam_blocks(int P) {
  const long long nb = ((long long)P + CAM_THREADS - 1) / CAM_THREADS;
  return (int)(nb < 1 ? 1 : (nb > CAM_MAX_BLOCKS ? CAM_MAX_BLOCKS : nb));
}

}  // namespace s3g
