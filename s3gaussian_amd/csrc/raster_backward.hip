// Backward half of the MI355X-native differentiable Gaussian rasterizer (gfx950, wave64).
//
// Computes what CudaRasterizer::Rasterizer::backward computes (RAST/cuda_rasterizer/rasterizer_impl.cu:343-444):
//   blend_backward_kernel      <- BACKWARD::render / renderCUDA       (backward.cu:415-590)
//   geometry_backward_kernel   <- computeCov2DCUDA + preprocessCUDA   (backward.cu:144-274, 346-412) fused into one pass
//
// The reference issues 10 global float atomicAdd per contributing (pixel, Gaussian) pair (backward.cu:550-587).
// Device-scope atomics execute memory-side on MI355X (a few G/s), so this backward has NO global atomics at all and
// is bit-reproducible run to run:
//   1. the six geometry sums are re-associated so that everything depending only on the Gaussian (conic, opacity,
//      0.5*W) is factored out of the pixel sum: with v = dL/dalpha * G the kernel accumulates
//      S0=sum v, Sx=sum v*dx, Sy=sum v*dy, Sxx=sum v*dx*dx, Sxy=sum v*dx*dy, Syy=sum v*dy*dy (+3 colour, +1 depth);
//   2. each of the 10 sums is reduced across the 16 lanes of a row with DPP row-shift adds (no shuffles through memory),
//      skipped outright when no lane of the wave is touched by the Gaussian;
//   3. the 16 lane-rows of the tile (4 waves x 4 rows) park their sums in LDS slots, added in fixed order (no float atomics
//      anywhere);
//   4. once per 32-Gaussian batch eight threads per Gaussian (one per float pair) add its 16 slots and store its 10 sums as
//      one 40-byte record at the instance's position in the sorted list (consecutive lanes -> consecutive records);
//   5. geometry_backward_kernel gathers each Gaussian's records through slot_pos[] (the instance -> position map
//      the forward's sort emitted), applies the factored-out coefficients and runs the per-Gaussian chain.
// The two kernels live in raster_blend_backward.hip and raster_geom_backward.hip; this file is the host side of the five exports.
#include "raster_dev.hpp"

#include "../../include/s3g_alpha.h"

using namespace s3g;

extern "C" size_t s3g_raster_backward_workspace_bytes(int P, int R) {
  (void)P;
  return ((size_t)(R > 0 ? R : 0) * NREC * sizeof(float) + 127) & ~size_t(127);
}
extern "C" size_t s3g_raster_backward2_workspace_bytes(int P, int R) {
  (void)P;
  return ((size_t)(R > 0 ? R : 0) * (NREC + 4) * sizeof(float) + 127) & ~size_t(127);
}

// One backward call.  An export fills what it has; a field it leaves out is NULL / false.
struct BackwardCall {
  const char* who;   // the export's name, for error messages
  bool two_images;   // colors2 / dL_dpix2 / dL_dcolor2 are required; records of NREC + 4 floats
  bool alpha;        // dL_dalpha is required
  const s3g_raster_inputs* in;
  const float* colors2;
  int R;
  const int* radii;
  const void *geometry_arena, *binning_arena, *image_arena;   // of the forward
  void* workspace;
  const float *dL_dpix, *dL_dpix_depth, *dL_dpix2, *dL_dalpha;   // upstream
  float *dL_dmean2D, *dL_dconic, *dL_dopacity, *dL_dcolor, *dL_dcolor2, *dL_ddepth, *dL_dmean3D, *dL_dcov3D, *dL_dsh, *dL_dscale, *dL_drot;
  const s3g_densify_accum* dens;
  void* stream;
};

static int raster_backward(const BackwardCall& c) {
  hipStream_t stream = (hipStream_t)c.stream;
  const s3g_raster_inputs* in = c.in;
  if (c.dens && !(c.dens->xyz_gradient_accum && c.dens->denom && c.dens->max_radii2D)) {
    set_error("%s: s3g_densify_accum needs all three arrays", c.who);
    return S3G_ERR_INVALID_ARG;
  }
  if (!in) {
    set_error("%s: NULL inputs", c.who);
    return S3G_ERR_INVALID_ARG;
  }
  const int P = in->P, W = in->width, H = in->height, R = c.R;
  if (P == 0) return S3G_OK;
  if (!c.radii || !c.geometry_arena || !c.image_arena || (R > 0 && (!c.binning_arena || !c.workspace)) || !c.dL_dpix ||
      !c.dL_dpix_depth || !c.dL_dmean2D || !c.dL_dopacity || !c.dL_dcolor || !c.dL_dmean3D || !c.dL_dcov3D || !c.dL_dscale ||
      !c.dL_drot || (in->shs && !c.dL_dsh) ||
      (c.two_images && (!c.colors2 || !c.dL_dpix2 || !c.dL_dcolor2 || !in->colors_precomp)) || (c.alpha && !c.dL_dalpha)) {
    set_error("%s: NULL array argument", c.who);
    return S3G_ERR_INVALID_ARG;
  }
  const bool debug = in->debug != 0;
  const Arenas a = reopen_arenas(in, R, c.geometry_arena, c.binning_arena, c.image_arena);
  const GeomState& g = a.g;
  float* records = reinterpret_cast<float*>(c.workspace);
  const float* colors = in->colors_precomp ? in->colors_precomp : g.rgb;
  if (R > 0)
    S3G_TRY(launch_blend_backward(a, c.two_images, c.alpha, colors, in->background, c.dL_dpix, c.dL_dpix_depth, records,
                                  c.colors2, c.dL_dpix2, c.dL_dalpha, (double)R, stream, debug));
  GeomBwdArgs ga;
  ga.P = P; ga.D = in->D; ga.M = in->M; ga.means3D = in->means3D; ga.radii = c.radii; ga.shs = in->shs;
  ga.clamped = g.clamped; ga.scales = in->scales; ga.rotations = in->rotations; ga.scale_modifier = in->scale_modifier;
  ga.cov3Ds = in->cov3D_precomp ? in->cov3D_precomp : g.cov3D;
  ga.view = in->viewmatrix; ga.proj = in->projmatrix; ga.campos = in->cam_pos;
  ga.fy = H / (2.0f * in->tan_fovy); ga.fx = W / (2.0f * in->tan_fovx);
  ga.tan_fovx = in->tan_fovx; ga.tan_fovy = in->tan_fovy;
  ga.W = W; ga.H = H; ga.gx = a.gx;
  ga.rect = g.rect; ga.gauss_off = g.gauss_off; ga.slot_pos = a.b.slot_pos; ga.tile_hi = a.im.tile_hi;
  ga.records = records; ga.conic_opacity = g.conic_opacity; ga.ctrl = a.im.ctrl;
  ga.dL_dmean2D = c.dL_dmean2D; ga.dL_dconic = c.dL_dconic; ga.dL_dopacity = c.dL_dopacity; ga.dL_dcolor = c.dL_dcolor;
  ga.dL_dcolor2 = c.dL_dcolor2; ga.dL_ddepth = c.dL_ddepth;
  ga.dL_dmean3D = c.dL_dmean3D; ga.dL_dcov3D = c.dL_dcov3D; ga.dL_dsh = c.dL_dsh; ga.dL_dscale = c.dL_dscale; ga.dL_drot = c.dL_drot;
  ga.dens_accum = c.dens ? c.dens->xyz_gradient_accum : nullptr;
  ga.dens_denom = c.dens ? c.dens->denom : nullptr;
  ga.dens_max_radii = c.dens ? c.dens->max_radii2D : nullptr;
  return launch_geometry_backward(ga, c.two_images, stream, debug);
}

// Every export names the same arrays the same way: a BackwardCall `c` for `name` with the fields that all five shapes have.
#define S3G_BACKWARD_CALL(c, name)                                                                                           \
  BackwardCall c = {};                                                                                                       \
  c.who = name; c.in = in; c.R = R; c.radii = radii; c.geometry_arena = geometry_arena; c.binning_arena = binning_arena;     \
  c.image_arena = image_arena; c.workspace = workspace; c.dL_dpix = dL_dpix; c.dL_dpix_depth = dL_dpix_depth;                \
  c.dL_dmean2D = dL_dmean2D; c.dL_dconic = dL_dconic; c.dL_dopacity = dL_dopacity; c.dL_dcolor = dL_dcolor;                  \
  c.dL_ddepth = dL_ddepth; c.dL_dmean3D = dL_dmean3D; c.dL_dcov3D = dL_dcov3D; c.dL_dscale = dL_dscale; c.dL_drot = dL_drot; \
  c.stream = stream_

extern "C" int s3g_raster_backward(const s3g_raster_inputs* in, int R, const int* radii, const void* geometry_arena,
                                   const void* binning_arena, const void* image_arena, void* workspace,
                                   const float* dL_dpix, const float* dL_dpix_depth, float* dL_dmean2D, float* dL_dconic,
                                   float* dL_dopacity, float* dL_dcolor, float* dL_ddepth, float* dL_dmean3D,
                                   float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot, void* stream_) {
  S3G_BACKWARD_CALL(c, "s3g_raster_backward");
  c.dL_dsh = dL_dsh;
  return raster_backward(c);
}
extern "C" int s3g_raster_backward_accum(const s3g_raster_inputs* in, int R, const int* radii, const void* geometry_arena,
                                         const void* binning_arena, const void* image_arena, void* workspace,
                                         const float* dL_dpix, const float* dL_dpix_depth, float* dL_dmean2D,
                                         float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_ddepth,
                                         float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale,
                                         float* dL_drot, const s3g_densify_accum* dens, void* stream_) {
  S3G_BACKWARD_CALL(c, "s3g_raster_backward_accum");
  c.dL_dsh = dL_dsh; c.dens = dens;
  return raster_backward(c);
}

// Two images from one geometry (colours precomputed, so no dL_dsh): the second image's colours and gradients ride along.
extern "C" int s3g_raster_backward2(const s3g_raster_inputs* in, const float* colors2, int R, const int* radii,
                                    const void* geometry_arena, const void* binning_arena, const void* image_arena,
                                    void* workspace, const float* dL_dpix, const float* dL_dpix_depth,
                                    const float* dL_dpix2, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity,
                                    float* dL_dcolor, float* dL_dcolor2, float* dL_ddepth, float* dL_dmean3D,
                                    float* dL_dcov3D, float* dL_dscale, float* dL_drot, void* stream_) {
  S3G_BACKWARD_CALL(c, "s3g_raster_backward2");
  c.two_images = true; c.colors2 = colors2; c.dL_dpix2 = dL_dpix2; c.dL_dcolor2 = dL_dcolor2;
  return raster_backward(c);
}
extern "C" int s3g_raster_backward2_accum(const s3g_raster_inputs* in, const float* colors2, int R, const int* radii,
                                          const void* geometry_arena, const void* binning_arena, const void* image_arena,
                                          void* workspace, const float* dL_dpix, const float* dL_dpix_depth,
                                          const float* dL_dpix2, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity,
                                          float* dL_dcolor, float* dL_dcolor2, float* dL_ddepth, float* dL_dmean3D,
                                          float* dL_dcov3D, float* dL_dscale, float* dL_drot,
                                          const s3g_densify_accum* dens, void* stream_) {
  S3G_BACKWARD_CALL(c, "s3g_raster_backward2_accum");
  c.two_images = true; c.colors2 = colors2; c.dL_dpix2 = dL_dpix2; c.dL_dcolor2 = dL_dcolor2; c.dens = dens;
  return raster_backward(c);
}

// The four shapes above with an upstream gradient on the opacity image A = 1 - final_T (include/s3g_alpha.h): one image
// (colors2 == dL_dpix2 == dL_dcolor2 == NULL; SH colours allowed) or two, with or without the densification bookkeeping.
extern "C" int s3g_raster_backward_alpha(const s3g_raster_inputs* in, const float* colors2, int R, const int* radii,
                                         const void* geometry_arena, const void* binning_arena, const void* image_arena,
                                         void* workspace, const float* dL_dpix, const float* dL_dpix_depth,
                                         const float* dL_dpix2, const float* dL_dalpha, float* dL_dmean2D, float* dL_dconic,
                                         float* dL_dopacity, float* dL_dcolor, float* dL_dcolor2, float* dL_ddepth,
                                         float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                                         const s3g_densify_accum* dens, void* stream_) {
  S3G_BACKWARD_CALL(c, "s3g_raster_backward_alpha");
  if ((colors2 != nullptr) != (dL_dpix2 != nullptr) || (colors2 != nullptr) != (dL_dcolor2 != nullptr)) {
    set_error("%s: colors2, dL_dpix2 and dL_dcolor2 go together (all three or none)", c.who);
    return S3G_ERR_INVALID_ARG;
  }
  c.alpha = true; c.dL_dalpha = dL_dalpha;
  c.two_images = colors2 != nullptr; c.colors2 = colors2; c.dL_dpix2 = dL_dpix2; c.dL_dcolor2 = dL_dcolor2;
  c.dL_dsh = c.two_images ? nullptr : dL_dsh;   // as s3g_raster_backward2: two images take precomputed colours
  if (dens && (dens->xyz_gradient_accum || dens->denom || dens->max_radii2D)) c.dens = dens;   // three NULL accumulators = none
  return raster_backward(c);
}
