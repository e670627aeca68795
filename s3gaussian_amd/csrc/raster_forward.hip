// Forward half of the MI355X-native differentiable Gaussian rasterizer (gfx950, wave64).
//
// What it computes is the reference's CudaRasterizer::Rasterizer::forward
// (RAST/cuda_rasterizer/rasterizer_impl.cu:198-339); how it computes it is not:
//
//   reference (CUDA)                                   raster_*.hip (CDNA4)
//   -------------------------------------------------  ------------------------------------------------------
//   preprocessCUDA  (forward.cu:155-256)               raster_preprocess.hip: same per-Gaussian math (bit-exact fp32,
//                                                      contraction off) + per-tile instance histogram
//   InclusiveSum over P + duplicateWithKeys + global   raster_bin.hip: ATOMIC-FREE multisplit: device-scope atomics on
//   64-bit radix sort of all R instances + range scan   MI355X execute memory-side (~2-6 G/s measured), so instances are
//   (rasterizer_impl.cu:278-319)                        binned with per-workgroup histograms of ALL tiles held in LDS
//                                                      (27 KB for 6.7k tiles; 160 KB LDS allows ~38k tiles), a
//                                                      [workgroup][tile] offset table and LDS cursors; raster_sort.hip:
//                                                      per-tile sort of (depth bits, index) keys staged in LDS.  Final
//                                                      order == the reference's stable (tile, depth) radix sort: ties
//                                                      in depth resolve by ascending Gaussian index.
//   renderCUDA (forward.cu:261-379)                    raster_blend.hip: 16x16 tile = 4 wave64, Gaussian
//                                                      attributes (incl. colour+depth) staged in LDS, conic
//                                                      pre-scaled so alpha = o * exp2(q) is one v_exp_f32
// This file is the host side: raster_forward_impl issues the stages through the launchers of raster_dev.hpp.
#include "raster_dev.hpp"

using namespace s3g;

// Exact (tile, Gaussian) culling at binning time (geom_math.hpp::tile_can_contribute); on by default, switchable so the
// instance lists can be compared bit for bit with the reference's bounding-square binning.
static bool g_exact_cull = true;

// as != NULL: the host-asynchronous variant (s3g_raster_forward_async) -- arenas are the caller's, sized for a speculative
// capacity, and nothing below waits for the device.
static int raster_forward_impl(const s3g_raster_inputs* in, const float* colors2, float* out_color2,
                               s3g_resize_fn geometry_buffer, void* geometry_user, s3g_resize_fn binning_buffer,
                               void* binning_user, s3g_resize_fn image_buffer, void* image_user, float* out_color,
                               float* out_depth, int* radii, int* num_rendered, void* stream_,
                               const s3g_raster_async* as = nullptr) {
  clear_error();
  hipStream_t stream = (hipStream_t)stream_;
  if (!in || (!as && (!geometry_buffer || !binning_buffer || !image_buffer || !num_rendered))) {
    set_error("s3g_raster_forward: NULL argument");
    return S3G_ERR_INVALID_ARG;
  }
  if (as && (!as->geometry_arena || !as->image_arena || !as->binning_arena || as->capacity_instances == 0 ||
             as->capacity_instances > 0x7fffffffu || as->capacity_slots < as->capacity_instances)) {
    set_error("s3g_raster_forward_async: needs the three arenas and 0 < capacity_instances <= capacity_slots");
    return S3G_ERR_INVALID_ARG;
  }
  if (num_rendered) *num_rendered = 0;
  const int P = in->P, W = in->width, H = in->height;
  if (P < 0 || W <= 0 || H <= 0) {
    set_error("s3g_raster_forward: bad sizes P=%d W=%d H=%d", P, W, H);
    return S3G_ERR_INVALID_ARG;
  }
  if (P == 0) return S3G_OK;  // rasterize_points.cu:82: outputs keep the caller's zero fill
  if ((in->shs == nullptr) == (in->colors_precomp == nullptr)) {
    set_error("Please provide excatly one of either SHs or precomputed colors!");
    return S3G_ERR_INVALID_ARG;
  }
  if (((in->scales == nullptr || in->rotations == nullptr) && in->cov3D_precomp == nullptr) ||
      ((in->scales != nullptr || in->rotations != nullptr) && in->cov3D_precomp != nullptr)) {
    set_error("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
    return S3G_ERR_INVALID_ARG;
  }
  if (!in->means3D || !in->opacities || !in->viewmatrix || !in->projmatrix || !in->cam_pos || !in->background ||
      !out_color || !out_depth || !radii) {
    set_error("s3g_raster_forward: NULL array argument");
    return S3G_ERR_INVALID_ARG;
  }
  Arenas a(W, H);
  if (a.gx > 65535 || a.gy > 65535) {
    set_error("image too large for 16-bit tile coordinates");
    return S3G_ERR_INVALID_ARG;
  }
  const bool debug = in->debug != 0;

  // ---- carve: the geometry and image arenas (the binning arena waits for R)
  size_t geom_bytes = 0, img_bytes = 0;
  GeomState::carve(nullptr, P, &geom_bytes);
  ImageState::carve(nullptr, (size_t)W * H, a.tiles, bin_blocks(P), &img_bytes);
  void* geom_p = as ? as->geometry_arena : geometry_buffer(geometry_user, geom_bytes);
  void* img_p = as ? as->image_arena : image_buffer(image_user, img_bytes);
  if (!geom_p || !img_p) {
    set_error("resize callback returned NULL");
    return S3G_ERR_ALLOC;
  }
  a.g = GeomState::carve(geom_p, P, nullptr);
  a.im = ImageState::carve(img_p, (size_t)W * H, a.tiles, bin_blocks(P), nullptr);
  S3G_HIP_CHECK(hipMemsetAsync(a.im.ctrl, 0, 8 * sizeof(uint32_t), stream));

  // ---- preprocess, count, scan
  S3G_TRY(launch_preprocess(in, a, g_exact_cull, radii, stream));
  S3G_TRY(launch_bin_count(P, a, g_exact_cull, stream, debug));
  S3G_TRY(launch_bin_scan(P, a, as, stream, debug));

  // ---- learn R (synchronous) or assume the caller's capacity (asynchronous)
  uint32_t R, max_tile, S;
  void* bin_p;
  if (!as) {
    // the one host sync of the forward (reference: rasterizer_impl.cu:282): R sizes the binning arena
    static thread_local uint32_t* h_ctrl = nullptr;
    if (!h_ctrl) S3G_HIP_CHECK(hipHostMalloc((void**)&h_ctrl, 8 * sizeof(uint32_t), hipHostMallocDefault));
    S3G_HIP_CHECK(hipMemcpyAsync(h_ctrl, a.im.ctrl, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    S3G_HIP_CHECK(hipStreamSynchronize(stream));
    R = h_ctrl[0]; max_tile = h_ctrl[1]; S = h_ctrl[3];
    if (h_ctrl[2] & 1u) {
      set_error("Point is filtered although prefiltered is set. This shouldn't happen!");
      return S3G_ERR_PREFILTERED;
    }
    if (R > 0x7fffffffu) {
      set_error("too many Gaussian/tile instances (%u)", R);
      return S3G_ERR_INVALID_ARG;
    }
    *num_rendered = (int)R;
    size_t bin_bytes = 0;
    BinningState::carve(nullptr, R, S, &bin_bytes);
    bin_p = binning_buffer(binning_user, bin_bytes);
    if (!bin_p && R > 0) {
      set_error("resize callback returned NULL");
      return S3G_ERR_ALLOC;
    }
  } else {
    // host-asynchronous: the arena was sized for (capacity_instances, capacity_slots) before anything ran; the kernels below
    // read R / S / the ranges on the device and find nothing to do if scan_tiles_kernel saw the capacity exceeded.  The
    // control words travel to the caller's pinned buffer behind the kernels: whoever reads them must first know that the
    // stream has passed this point (an event recorded after this call).
    R = as->capacity_instances; S = as->capacity_slots;
    max_tile = sort_estimate(as);
    bin_p = as->binning_arena;
    if (as->status_host)
      S3G_HIP_CHECK(hipMemcpyAsync(as->status_host, a.im.ctrl, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    if (as->status_event)   // the verdict is on its way: a caller that has to know it waits for THIS, not for the sort / blend below
      S3G_HIP_CHECK(hipEventRecord((hipEvent_t)as->status_event, stream));
    if (num_rendered) *num_rendered = (int)R;
  }
  a.b = BinningState::carve(bin_p, R, S, nullptr);
  const bool forward_only = as && as->forward_only != 0;
  if (as && !forward_only)
    S3G_TRY(launch_fill_slots(a, stream, debug));
  else if (!as && S > 0)
    S3G_HIP_CHECK(hipMemsetAsync(a.b.slot_pos, 0xff, (size_t)S * sizeof(uint32_t), stream));  // culled slots

  // ---- write, sort, blend
  if (R > 0) {
    S3G_TRY(launch_bin_write(P, a, g_exact_cull, stream, debug));
    S3G_TRY(launch_tile_sort(a, forward_only ? nullptr : a.b.slot_pos, max_tile, as, stream, debug));
  }
  return launch_blend_forward(a, in->colors_precomp ? in->colors_precomp : a.g.rgb, in->background, out_color, out_depth, colors2,
                              out_color2, as ? -1.0 : (double)R, stream, debug);   // asynchronous: R is not known here
}

extern "C" int s3g_raster_arena_bytes(int P, int width, int height, uint32_t capacity_instances, uint32_t capacity_slots,
                                      size_t* geometry_bytes, size_t* binning_bytes, size_t* image_bytes) {
  if (P < 0 || width <= 0 || height <= 0) {
    set_error("s3g_raster_arena_bytes: bad sizes");
    return S3G_ERR_INVALID_ARG;
  }
  const Arenas a(width, height);
  size_t n = 0;
  GeomState::carve(nullptr, (size_t)P, &n);
  if (geometry_bytes) *geometry_bytes = n;
  BinningState::carve(nullptr, capacity_instances, capacity_slots, &n);
  if (binning_bytes) *binning_bytes = n;
  ImageState::carve(nullptr, (size_t)width * height, (size_t)a.gx * a.gy, bin_blocks(P), &n);
  if (image_bytes) *image_bytes = n;
  return S3G_OK;
}

extern "C" int s3g_raster_forward_async(const s3g_raster_inputs* in, const float* colors2, const s3g_raster_async* async_,
                                        float* out_color, float* out_depth, float* out_color2, int* radii, void* stream_) {
  if (!async_ || (colors2 != nullptr) != (out_color2 != nullptr) || (colors2 && (!in || !in->colors_precomp))) {
    set_error("s3g_raster_forward_async: needs the async descriptor; colors2 and out_color2 go together (with colors_precomp)");
    return S3G_ERR_INVALID_ARG;
  }
  return raster_forward_impl(in, colors2, out_color2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, out_color, out_depth,
                             radii, nullptr, stream_, async_);
}

extern "C" int s3g_raster_forward(const s3g_raster_inputs* in, s3g_resize_fn geometry_buffer, void* geometry_user,
                                  s3g_resize_fn binning_buffer, void* binning_user, s3g_resize_fn image_buffer,
                                  void* image_user, float* out_color, float* out_depth, int* radii, int* num_rendered,
                                  void* stream_) {
  return raster_forward_impl(in, nullptr, nullptr, geometry_buffer, geometry_user, binning_buffer, binning_user,
                             image_buffer, image_user, out_color, out_depth, radii, num_rendered, stream_);
}

// Forward of two images from one geometry (colours in->colors_precomp -> out_color + out_depth, colors2 -> out_color2)
// with ONE blend pass; the arenas are those of an ordinary forward and feed s3g_raster_backward2.
extern "C" int s3g_raster_forward2(const s3g_raster_inputs* in, const float* colors2, s3g_resize_fn geometry_buffer,
                                   void* geometry_user, s3g_resize_fn binning_buffer, void* binning_user,
                                   s3g_resize_fn image_buffer, void* image_user, float* out_color, float* out_depth,
                                   float* out_color2, int* radii, int* num_rendered, void* stream_) {
  if (!in || !in->colors_precomp || !colors2 || !out_color2) {
    set_error("s3g_raster_forward2: needs colors_precomp, colors2 and out_color2");
    return S3G_ERR_INVALID_ARG;
  }
  return raster_forward_impl(in, colors2, out_color2, geometry_buffer, geometry_user, binning_buffer, binning_user,
                             image_buffer, image_user, out_color, out_depth, radii, num_rendered, stream_);
}

extern "C" void s3g_raster_set_exact_cull(int on) { g_exact_cull = on != 0; }
extern "C" int s3g_raster_get_exact_cull(void) { return g_exact_cull ? 1 : 0; }
