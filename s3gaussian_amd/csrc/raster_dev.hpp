// Private header of the rasterizer (raster_*.hip): tile constants, the three arenas of a forward and the launchers its stages
// offer each other.  Every kernel is launched from the file that defines it; raster_forward.hip strings the launchers together.
#pragma once
#include "common.hpp"

namespace s3g {

constexpr int TILE_X = 16;  // reference BLOCK_X/BLOCK_Y, RAST/cuda_rasterizer/config.h:16-17
constexpr int TILE_Y = 16;
constexpr int MAX_BIN_BLOCKS = 512;   // binning workgroups (2 per CU); each keeps a histogram of ALL tiles in LDS
constexpr int MAX_TILES_LDS = 38000;  // (160 KiB - slack) / 4 B: largest tile grid the single-pass multisplit handles
constexpr int NREC = 10;              // floats per instance gradient record written by the blend backward
constexpr int TILE_MASK_BITS = 32;    // rects of at most this many tiles get a GeomState::tile_mask from the preprocess
constexpr uint32_t SORT_SMALL_KEYS = 4096;  // longest tile list an asynchronous forward without long_lists accepts (raster_sort.hip)
// The two numbers an asynchronous forward takes from its descriptor for the per-tile lists, shared by the stage that uses each and
// by s3g_raster_sort_plan: the longest list the counting kernel lets through (scan_tiles_kernel's cap_tile; 0 = the synchronous
// forward, which checks nothing) -- the sort's launches must reach exactly that far -- and the estimate that sizes the sort's buffers.
inline uint32_t sort_list_cap(const s3g_raster_async* as) { return as ? (as->long_lists ? 0xffffffffu : SORT_SMALL_KEYS) : 0u; }
inline uint32_t sort_estimate(const s3g_raster_async* as) { return as->sort_lds_keys ? as->sort_lds_keys : SORT_SMALL_KEYS; }

// number of binning workgroups / Gaussians per workgroup for a scene of P Gaussians
inline int bin_blocks(int P) {
  int nb = (P + 255) / 256;
  return nb < 1 ? 1 : (nb > MAX_BIN_BLOCKS ? MAX_BIN_BLOCKS : nb);
}
inline int bin_chunk(int P) {
  const int nb = bin_blocks(P);
  const int per = (P + nb - 1) / nb;
  return ((per + 63) / 64) * 64;   // whole waves; the binning workgroups step through their chunk with a guarded tail
}

// Per-Gaussian forward state ("GeometryState").
struct GeomState {
  float* depths;          // [P]   view-space z
  float2* means2D;        // [P]   pixel coordinates
  float4* conic_opacity;  // [P]   (conic a, b, c, opacity)
  float* cov3D;           // [P,6]
  float* rgb;             // [P,3] SH->RGB result (only when shs given)
  uint8_t* clamped;       // [P,3]
  ushort4* rect;          // [P]   tile rect (min.x, min.y, max.x, max.y), zero area when culled
  uint32_t* gauss_off;    // [P]   exclusive scan of tiles_touched: first slot of the Gaussian in slot_pos[]
  uint32_t* tile_mask;    // [P]   rects of <= 32 tiles: bit k = tile k (row-major in the rect) survives the exact cull
  static GeomState carve(void* p, size_t P, size_t* bytes) {
    Carver c(p);
    GeomState g;
    g.depths = c.take<float>(P);
    g.means2D = c.take<float2>(P);
    g.conic_opacity = c.take<float4>(P);
    g.cov3D = c.take<float>(P * 6);
    g.rgb = c.take<float>(P * 3);
    g.clamped = c.take<uint8_t>(P * 3);
    g.rect = c.take<ushort4>(P);
    g.gauss_off = c.take<uint32_t>(P);
    g.tile_mask = c.take<uint32_t>(P);
    if (bytes) *bytes = c.bytes();
    return g;
  }
};

// Per-image state ("ImageState") + the per-tile bucket bookkeeping.
struct ImageState {
  float* final_T;        // [H*W]
  uint32_t* n_contrib;   // [H*W]
  uint2* ranges;         // [tiles]  [start,end) into the sorted instance list
  uint32_t* tile_count;  // [tiles]  instances per tile
  uint32_t* tile_hi;     // [tiles]  ranges[t].x + deepest contributing list position (1-based) over the tile's pixels
  uint32_t* ctrl;        // [8]      ctrl[0]=R (total instances), ctrl[1]=max instances in one tile, ctrl[2]=error flags
  uint32_t* chunk_total; // [MAX_BIN_BLOCKS] instances emitted per binning workgroup (then its exclusive prefix)
  uint32_t* table;       // [nb][tiles] per-workgroup, per-tile instance counts (then exclusive prefix over workgroups)
  static ImageState carve(void* p, size_t N, size_t tiles, size_t nb, size_t* bytes) {
    Carver c(p);
    ImageState s;
    s.final_T = c.take<float>(N);
    s.n_contrib = c.take<uint32_t>(N);
    s.ranges = c.take<uint2>(tiles);
    s.tile_count = c.take<uint32_t>(tiles);
    s.tile_hi = c.take<uint32_t>(tiles);
    s.ctrl = c.take<uint32_t>(8);
    s.chunk_total = c.take<uint32_t>(MAX_BIN_BLOCKS);
    s.table = c.take<uint32_t>(nb * tiles);
    if (bytes) *bytes = c.bytes();
    return s;
  }
};

// Per-instance state ("BinningState").
struct BinningState {
  uint64_t* keys;        // [R]  (depth bits << 32 | gaussian index), sorted ascending inside each tile range
  uint32_t* point_list;  // [R]  gaussian index, tile-major, front-to-back
  uint32_t* slot_pos;    // [S]  slot_pos[gauss_off[g] + k] = position in point_list of g's k-th tile (row-major in its rect),
                         //      0xffffffff if that tile was culled.  S = sum of rect areas >= R; LAST in the arena so that
                         //      code which only knows R (backward, reuse) still finds it.
  static BinningState carve(void* p, size_t R, size_t S, size_t* bytes) {
    Carver c(p);
    BinningState b;
    b.keys = c.take<uint64_t>(R);
    b.point_list = c.take<uint32_t>(R);
    b.slot_pos = c.take<uint32_t>(S);
    if (bytes) *bytes = c.bytes();
    return b;
  }
};

// The arenas of one forward with the sizes that locate everything in them.
struct Arenas {
  int W, H, gx, gy, tiles;
  GeomState g;
  ImageState im;
  BinningState b;
  Arenas(int W_, int H_)
      : W(W_), H(H_), gx((W_ + TILE_X - 1) / TILE_X), gy((H_ + TILE_Y - 1) / TILE_Y), tiles(gx * gy), g(), im(), b() {}
};
// Reopens the arenas of an earlier forward of `in` that rendered R instances (slot_pos is found without knowing S: it is last).
inline Arenas reopen_arenas(const s3g_raster_inputs* in, int R, const void* geometry, const void* binning, const void* image) {
  Arenas a(in->width, in->height);
  a.g = GeomState::carve(const_cast<void*>(geometry), in->P, nullptr);
  a.im = ImageState::carve(const_cast<void*>(image), (size_t)a.W * a.H, a.tiles, bin_blocks(in->P), nullptr);
  a.b = BinningState::carve(const_cast<void*>(binning), (size_t)(R > 0 ? R : 0), 0, nullptr);
  return a;
}
// grid of the one-workgroup-per-tile kernels: whole groups of eight workgroups for xcd_swizzle
inline uint32_t tile_blocks(int tiles) { return ((uint32_t)tiles + 7u) & ~7u; }

#define S3G_TRY(expr) do { const int _rc = (expr); if (_rc != S3G_OK) return _rc; } while (0)

// ---- the stages of the forward, in the order raster_forward_impl issues them; each returns S3G_OK or an error code ----------
// raster_preprocess.hip: per-Gaussian geometry -> a.g, radii
int launch_preprocess(const s3g_raster_inputs* in, const Arenas& a, bool exact_cull, int* radii, hipStream_t stream);
// raster_bin.hip: count = instances per (workgroup, tile) -> a.im.table; scan -> a.im.ranges, a.im.ctrl (as != NULL: with the
// capacity check); fill_slots: slot_pos[0, S) = "culled", S read on the device; write = keys -> a.b.keys
int launch_bin_count(int P, const Arenas& a, bool exact_cull, hipStream_t stream, bool debug);
int launch_bin_scan(int P, const Arenas& a, const s3g_raster_async* as, hipStream_t stream, bool debug);
int launch_fill_slots(const Arenas& a, hipStream_t stream, bool debug);
int launch_bin_write(int P, const Arenas& a, bool exact_cull, hipStream_t stream, bool debug);
// raster_sort.hip: a.b.keys sorted inside every tile -> a.b.point_list (+ slot_map, NULL for a forward-only render); max_tile =
// the longest list (as != NULL: the caller's estimate)
int launch_tile_sort(const Arenas& a, uint32_t* slot_map, uint32_t max_tile, const s3g_raster_async* as, hipStream_t stream, bool debug);
// raster_blend.hip: colors (+ colors2 or NULL) -> out_color, out_depth (+ out_color2); instances = R for the profile, -1 = unknown
int launch_blend_forward(const Arenas& a, const float* colors, const float* bg, float* out_color, float* out_depth,
                         const float* colors2, float* out_color2, double instances, hipStream_t stream, bool debug);

// ---- the stages of the backward, in the order raster_backward.hip issues them ------------------------------------------------
// raster_blend_backward.hip: upstream image gradients -> records [R][NREC], or [R][NREC + 4] with two_images (colors2, dL_dpix2);
// alpha: dL_dalpha [H*W] is the upstream gradient of the opacity image.  instances = R for the profile
int launch_blend_backward(const Arenas& a, bool two_images, bool alpha, const float* colors, const float* bg,
                          const float* dL_dpix, const float* dL_dpix_depth, float* records, const float* colors2,
                          const float* dL_dpix2, const float* dL_dalpha, double instances, hipStream_t stream, bool debug);
// raster_geom_backward.hip: records -> the per-Gaussian gradients.  The kernel's argument block, filled by raster_backward.hip:
struct GeomBwdArgs {
  int P, D, M;
  const float* means3D;
  const int* radii;
  const float* shs;
  const uint8_t* clamped;
  const float* scales;
  const float* rotations;
  float scale_modifier;
  const float* cov3Ds;  // precomputed or the forward's own
  const float* view;
  const float* proj;
  const float* campos;
  float fx, fy, tan_fovx, tan_fovy;
  int W, H, gx;
  // gather side
  const ushort4* rect;
  const uint32_t* gauss_off;
  const uint32_t* slot_pos;
  const uint32_t* tile_hi;        // absolute end of the written records of each tile
  const float* records;           // [R][NREC]
  const float4* conic_opacity;
  const uint32_t* ctrl;           // forward's control words: ctrl[4] != 0 = asynchronous forward overflowed, nothing was binned
  // outputs (every element of every output is written, zeros for culled Gaussians)
  float* dL_dmean2D;        // [P,3]
  float* dL_dconic;         // [P,4]  optional (may be NULL)
  float* dL_dopacity;       // [P]
  float* dL_dcolor;         // [P,3]
  float* dL_dcolor2;        // [P,3]  second image's colours (two-image backward only)
  float* dL_ddepth;         // [P]    optional (may be NULL)
  float* dL_dmean3D;        // [P,3]
  float* dL_dcov3D;         // [P,6]
  float* dL_dsh;            // [P,M,3]
  float* dL_dscale;         // [P,3]
  float* dL_drot;           // [P,4]
  // optional densification bookkeeping (train.py:489-493, scene/gaussian_model.py:693-695), all three or none
  float* dens_accum;        // [P] xyz_gradient_accum += ||dL_dmean2D.xy|| where visible
  float* dens_denom;        // [P] denom += 1 where visible
  float* dens_max_radii;    // [P] max_radii2D = max(max_radii2D, radii) where visible
};
int launch_geometry_backward(const GeomBwdArgs& ga, bool two_images, hipStream_t stream, bool debug);

}  // namespace s3g
