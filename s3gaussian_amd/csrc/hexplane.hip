// MI355X-native multi-resolution HexPlane sampler: forward and backward, one fused pass each.
//
// Reference: scene/hexplane.py:73-106 runs 4 levels x 6 planes = 24 F.grid_sample launches, each materialising a
// [P,32] tensor, then 20 elementwise products and a concat; autograd replays the same 24 in backward.
//
// Planes are stored channel-last, so one texel = 32 channels = one 128-byte line.  Forward and the per-point backward give
// a point to EIGHT lanes (4 channels each, one 16-byte load per texel); the bilinear taps are computed once per point and
// shared through LDS; points are processed in a 3-D blocked order, groups dealt to the XCDs in contiguous eighths.  The
// product over planes never leaves registers.  Arithmetic follows torch's grid_sampler_2d (bilinear, border,
// align_corners=True) op for op; contraction is off.  When all points share one timestamp (desc.uniform_time) the three
// (axis, t) planes of a level are first collapsed to 1-D row tables (see "uniform time" below).
//
// Backward without an atomic storm.  A direct scatter is 96 line-coalesced float atomics per point; MI355X retires
// ~10 G such line-ops/s whatever the contention (tools/ubench/atomic_lines.hip), i.e. 11.5 ms at 1.2 M points.  So:
//   pass A  (blocked order) re-gathers the taps, finishes dL/dxyz and writes to the scratch G ONE row per level,
//                           T = dL/dfeature * feature (point-major, 512 B per point, streamed).  Round 4 (S3G_HEX_SLAB_DIV,
//                           hexplane_backward_pointdiv_kernel): T straight from the forward's saved output, dL/ds_i = T / s_i plane by
//                           plane at four waves per SIMD; rounds 1-3 (hexplane_backward_point_kernel): the product rule with six
//                           samples live at two waves per SIMD (rounds 1-2 also wrote dL/ds of all 24 plane-levels, 3 KB per point);
//   sort    2-level counting sorts of the point indices with LDS histograms (no global atomics, no library sort) -- round 4: ONE
//           ORDER PER (orientation, LEVEL), by (major, minor) texel cell of THAT level (thirteen sorts with the blocked processing
//           order; rounds 1-3: the finest level's cells only, four sorts); the orders only steer the walks, so the caller may keep
//           them for several iterations (sort_state / sort_reuse);
//   pass B  (sorted orders, one launch: blockIdx.y = orientation * levels + level): a half-wave (32 lanes = the 32 channels) walks
//           a run of consecutive points of ITS order keeping one bilinear footprint per plane kind (the spatial plane and the
//           (major, t) plane of the orientation) in registers -- sums AND texel values -- and only issues atomics when the footprint
//           changes (two instead of four when the walk just steps to the neighbouring footprint): the 96 line-ops per point
//           drop to ~2 (rounds 1-3, every level in the finest order with a two-entry cache: ~5-6).  Taps are computed
//           cooperatively (lane = point x tap) and shared through LDS; index, coordinate and tap computation run one to two groups
//           ahead of the accumulation.
// Files: forward kernel, C API, workspace layout and the backward's orchestration here; pass A hexplane_point.hip, sorts
// hexplane_sort.hip, pass B (and the deterministic mode) hexplane_scatter.hip; shared: hexplane_bwd.hpp, hexplane_dev.hpp.
#include <atomic>

#include "hexplane_bwd.hpp"

namespace s3g {

template <bool UT>
__global__ void __launch_bounds__(256) hexplane_forward_kernel(const HexArgs a) {
  extern __shared__ float4 tapbuf[];   // [32 points][levels][TAP_SLOTS]
  const int j = threadIdx.x & 7, c4 = j * 4, slot = threadIdx.x >> 3;
  const int F = a.d.levels * HEXC;
  float4* taps = tapbuf + (size_t)slot * tap_stride(a.d.levels);
  for (int p0 = xcd_group(blockIdx.x, gridDim.x) * 32; p0 < a.P; p0 += gridDim.x * 32) {
    const int pi = p0 + slot;
    const bool live = pi < a.P;
    const int p = live ? (a.proc_order ? (int)a.proc_order[pi] : pi) : 0;
    float u[4];
    point_coords(a, p, u);
    wave_lds_sync();   // the previous point's taps have been read
    produce_taps(a, u, j, taps);
    wave_lds_sync();
    for (int l = 0; l < a.d.levels; l++) {
      float4 prod = make_float4(1.f, 1.f, 1.f, 1.f);
#pragma unroll
      for (int i = 0; i < 6; i++) {
        const int W = a.d.res[l][PAIR0[i]], H = a.d.res[l][PAIR1[i]];
        const float* pl = a.d.planes[l][i];
        float4 s;
        if (UT && IS_TIME_PLANE[i]) {
          const PointTap t = read_tap<true>(taps, l, i, W, H, c4);
          s = texel4(pl, t.off) * t.gx;
          s = s + texel4(pl, t.off + t.dx) * t.fx;
        } else {
          const PointTap t = read_tap<false>(taps, l, i, W, H, c4);
          s = texel4(pl, t.off) * (t.gx * t.gy);
          s = s + texel4(pl, t.off + t.dx) * (t.fx * t.gy);
          s = s + texel4(pl, t.off + t.dy) * (t.gx * t.fy);
          s = s + texel4(pl, t.off + t.dy + t.dx) * (t.fx * t.fy);
        }
        prod = prod * s;
      }
      if (live) {
        f4v v = {prod.x, prod.y, prod.z, prod.w};
        f4v* dst = reinterpret_cast<f4v*>(a.feat + (size_t)p * F + l * HEXC + c4);
        __builtin_nontemporal_store(v, dst);   // feature rows: streaming stores
      }
    }
  }
}

}  // namespace s3g

using namespace s3g;

extern "C" size_t s3g_hexplane_forward_workspace_bytes(const s3g_hexplane_desc* d) {
  if (!d || d->levels < 1 || d->levels > S3G_HEX_MAX_LEVELS || !d->uniform_time) return 0;
  return time_table_floats(d) * sizeof(float);
}

extern "C" int s3g_hexplane_forward(const s3g_hexplane_desc* d, int P, const float* xyz, const float* time,
                                    float* features, const uint32_t* proc_order, void* workspace, void* stream_) {
  if (int e = check_desc(d)) return e;
  if (P < 0 || (P > 0 && (!xyz || !time || !features || (d->uniform_time && !workspace)))) {
    set_error("s3g_hexplane_forward: bad argument");
    return S3G_ERR_INVALID_ARG;
  }
  if (P == 0) return S3G_OK;
  HexArgs a;
  memset(&a, 0, sizeof a);
  a.d = *d; a.P = P; a.xyz = xyz; a.time = time; a.feat = features; a.proc_order = proc_order;
  TimeRows rows;
  if (d->uniform_time) use_time_rows(a, rows, (float*)workspace, nullptr, (hipStream_t)stream_);
  const int blocks = (P + 31) / 32;  // one group of 32 points per workgroup measured best (0.567 -> 0.535 ms vs a 4096 cap)
  profile_begin(S3G_PROFILE_HEXPLANE_FORWARD, (hipStream_t)stream_);
  const size_t lds = (size_t)32 * tap_stride(d->levels) * sizeof(float4);
  if (d->uniform_time) hipLaunchKernelGGL(hexplane_forward_kernel<true>, dim3(blocks), dim3(256), lds, (hipStream_t)stream_, a);
  else hipLaunchKernelGGL(hexplane_forward_kernel<false>, dim3(blocks), dim3(256), lds, (hipStream_t)stream_, a);
  profile_end(S3G_PROFILE_HEXPLANE_FORWARD, (hipStream_t)stream_, (double)P, (double)d->levels);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

// 128-byte rows of scratch the default (slab) backward writes per point and level set: bench.py prices the implementation bytes
extern "C" int s3g_hexplane_backward_scratch_rows(int levels) { return levels; }

// Diagnostics only (tools/hex_probe.py walks): which of the 3 * levels scatter walks run -- bit orientation * levels + level.  With
// anything but all ones the plane gradients are INCOMPLETE; the setting is process-wide and meant for timing the walks one by one.
static std::atomic<uint32_t> g_walk_mask{0xffffffffu};
extern "C" void s3g_hexplane_debug_walk_mask(uint32_t mask) { g_walk_mask.store(mask, std::memory_order_relaxed); }

static std::atomic<int> g_hex_deterministic{0};
// Deterministic mode of the backward (process-wide; include/s3g_hexplane.h): stable walk orders, run records instead of atomics, a
// stencil gather in fixed order -- plane gradients bit-identical from run to run.  Needs uniform_time and resolutions <= 512; the
// workspace grows (s3g_hexplane_backward_workspace_bytes follows the setting).
extern "C" void s3g_hexplane_set_deterministic(int on) { g_hex_deterministic.store(on ? 1 : 0, std::memory_order_relaxed); }
extern "C" int s3g_hexplane_get_deterministic(void) { return g_hex_deterministic.load(std::memory_order_relaxed); }

// 32-bit words per point of the caller-kept `sort_state`: the walk orders, their compositions with the processing order, and the
// processing order itself (round 4: one walk order per orientation AND level, 6 * levels + 1; rounds 1-3: 7)
extern "C" int s3g_hexplane_sort_state_words(int levels) { return 2 * n_walk_orders(levels) + 1; }

static void carve_backward(Carver& c, const s3g_hexplane_desc* d, int P, float** G, float** tables, SortWork* w) {
  const size_t n = (size_t)P;
  float* g = c.take<float>((size_t)d->levels * n * HEXC);   // the T rows: one 128-byte row per point and level
  float* tb = d->uniform_time ? c.take<float>(2 * time_table_floats(d)) : nullptr;
  SortWork s;
  const size_t NO = (size_t)n_orders(d->levels), NW = (size_t)n_walk_orders(d->levels);
  s.nw = (int)NW;
  s.table = c.take<uint32_t>(NO * SORT_NB * SORT_BINS);
  s.seg_start = c.take<uint32_t>(NO * (SORT_BINS + 1));
  s.tmp = c.take<uint32_t>(NO * n);
  s.order = c.take<uint32_t>(NW * n);
  s.comp = c.take<uint32_t>(NW * n);
  s.proc = c.take<uint32_t>(n);
  if (G) *G = g;
  if (tables) *tables = tb;
  if (w) *w = s;
}
static void carve_det(Carver& c, const s3g_hexplane_desc* d, int P, DetWork* dw, void** index_begin, size_t* index_bytes) {
  // deterministic mode: per-walk cell starts (0xff-filled every backward: they come first, contiguous), segment links and run records
  const int nseg = (P + segment_length(P) - 1) / segment_length(P);
  DetWork w;
  memset(&w, 0, sizeof w);
  const size_t b0 = (c.off + 127) & ~size_t(127);
  size_t b1 = b0;
  for (int pass = 0; pass < 2; pass++)
    for (int o = 0; o < 3; o++)
      for (int l = 0; l < d->levels; l++) {
        const int oi = o * d->levels + l;
        size_t cells, wm;
        walk_cells(d, o, l, &cells, &wm);
        if (pass == 0) {
          w.walk[oi].cstart = c.take<uint32_t>(cells);
          w.walk[oi].tstart = c.take<uint32_t>(wm);
          b1 = c.off;
        } else {
          w.walk[oi].segcell = c.take<int>((size_t)nseg); w.walk[oi].tsegcell = c.take<int>((size_t)nseg);
          w.walk[oi].cell = c.take<float>(cells * 4 * HEXC); w.walk[oi].seg = c.take<float>((size_t)nseg * 4 * HEXC);
          w.walk[oi].tcell = c.take<float>(wm * 2 * HEXC); w.walk[oi].tseg = c.take<float>((size_t)nseg * 2 * HEXC);
        }
      }
  if (dw) *dw = w;
  if (index_begin) *index_begin = c.base ? c.base + b0 : nullptr;
  if (index_bytes) *index_bytes = b1 - b0;
}

extern "C" size_t s3g_hexplane_backward_workspace_bytes(const s3g_hexplane_desc* d, int P, int have_features) {
  if (!d || d->levels < 1 || d->levels > S3G_HEX_MAX_LEVELS || P < 0) return 0;
  Carver c(nullptr);
  (void)have_features;   // one layout for both algorithms
  carve_backward(c, d, P, nullptr, nullptr, nullptr);
  if (g_hex_deterministic.load(std::memory_order_relaxed)) carve_det(c, d, P, nullptr, nullptr, nullptr);
  return c.bytes();
}

static int hexplane_backward_impl(const s3g_hexplane_desc* d, int P, const float* xyz, const float* time,
                                  const float* dL_dfeatures, const float* features, int algorithm, float* dL_dxyz,
                                  float* const dL_dplanes[S3G_HEX_MAX_LEVELS][6], void* workspace,
                                  uint32_t* sort_state, int sort_reuse, void* stream_) {
  if (int e = check_desc(d)) return e;
  if (P < 0 || (P > 0 && (!xyz || !time || !dL_dfeatures || !dL_dxyz || !dL_dplanes || !workspace)) ||
      (sort_reuse && !sort_state)) {
    set_error("s3g_hexplane_backward: bad argument");
    return S3G_ERR_INVALID_ARG;
  }
  if (P == 0) return S3G_OK;
  hipStream_t stream = (hipStream_t)stream_;
  HexArgs a;
  memset(&a, 0, sizeof a);
  a.d = *d; a.P = P; a.xyz = xyz; a.time = time; a.gfeat = dL_dfeatures; a.gxyz = dL_dxyz;
  for (int l = 0; l < d->levels; l++)
    for (int i = 0; i < 6; i++) a.gplanes[l][i] = dL_dplanes[l][i];
  Carver c(workspace);
  float *G, *tables;
  SortWork w;
  carve_backward(c, d, P, &G, &tables, &w);
  const int NW = n_walk_orders(d->levels);
  const int det = g_hex_deterministic.load(std::memory_order_relaxed);
  DetWork detw = {};
  void* det_index = nullptr;
  size_t det_index_bytes = 0;
  if (det) {
    if (!d->uniform_time) {
      set_error("s3g_hexplane_backward: the deterministic mode needs desc.uniform_time (the (axis, t) planes as row tables)");
      return S3G_ERR_INVALID_ARG;
    }
    for (int l = 0; l < d->levels; l++)
      for (int k = 0; k < 3; k++)
        if (d->res[l][k] > SORT_BINS) {
          set_error("s3g_hexplane_backward: the deterministic mode needs spatial resolutions <= %d (sort cells = texel cells)", SORT_BINS);
          return S3G_ERR_INVALID_ARG;
        }
    carve_det(c, d, P, &detw, &det_index, &det_index_bytes);
  }
  if (sort_state) {  // caller-owned, persistent: s3g_hexplane_sort_state_words(levels) * P words
    w.order = sort_state;
    w.comp = sort_state + (size_t)NW * P;
    w.proc = sort_state + (size_t)2 * NW * P;
  }

  // 1. the walk orders and the processing order (2-level LDS counting sorts), unless the caller's are reused.
  //    Deterministic mode: ALWAYS -- its run records rely on every cell being contiguous in the walk order, which only holds for orders
  //    sorted on the CURRENT coordinates (the default walk sums with atomics and is indifferent to a stale order).
  if (!sort_reuse || det)
    if (int e = hexplane_sort_launch(a, w, det, stream)) return e;
  //    (the sorts above used the real resolutions; from here on the time planes are height-1 row tables if uniform_time)
  TimeRows rows;
  if (d->uniform_time) {
    const size_t nt = time_table_floats(d);
    S3G_HIP_CHECK(hipMemsetAsync(tables + nt, 0, nt * sizeof(float), stream));
    use_time_rows(a, rows, tables, tables + nt, stream);
  }
  a.seg_len = segment_length(P);
  a.walk_mask = g_walk_mask.load(std::memory_order_relaxed);
  // 2. per-point pass (dL/dxyz; ONE row T = dL/dfeature * feature per point and level -> G), then the scatter walks reading it back
  a.proc_order = w.proc;
  if (int e = hexplane_point_launch(a, features, algorithm, G, stream)) return e;
  if (int e = hexplane_scatter_launch(a, G, w, det, detw, det_index, det_index_bytes, stream)) return e;
  // 3. uniform time: fold the row tables' gradients back into the two plane rows
  if (d->uniform_time) {
    int maxW = 0;
    for (int l = 0; l < d->levels; l++)
      for (int k = 0; k < 3; k++) maxW = max(maxW, d->res[l][k]);
    hipLaunchKernelGGL(hexplane_time_rows_kernel<true>, dim3((maxW * HEXC + 255) / 256, 3, d->levels), dim3(256), 0, stream, rows);
  }
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" int s3g_hexplane_backward(const s3g_hexplane_desc* d, int P, const float* xyz, const float* time,
                                     const float* dL_dfeatures, const float* features, float* dL_dxyz,
                                     float* const dL_dplanes[S3G_HEX_MAX_LEVELS][6], void* workspace,
                                     uint32_t* sort_state, int sort_reuse, void* stream_) {
  return hexplane_backward_impl(d, P, xyz, time, dL_dfeatures, features, features ? S3G_HEX_SLAB_DIV : S3G_HEX_SLAB, dL_dxyz,
                                dL_dplanes, workspace, sort_state, sort_reuse, stream_);
}

extern "C" int s3g_hexplane_backward_algo(const s3g_hexplane_desc* d, int P, const float* xyz, const float* time,
                                          const float* dL_dfeatures, const float* features, int algorithm, float* dL_dxyz,
                                          float* const dL_dplanes[S3G_HEX_MAX_LEVELS][6], void* workspace,
                                          uint32_t* sort_state, int sort_reuse, void* stream_) {
  if (algorithm == S3G_HEX_WALK) {
    set_error("s3g_hexplane_backward_algo: the slab-free walk (algorithm %d) was removed in ABI 12; use S3G_HEX_SLAB_DIV or S3G_HEX_SLAB", algorithm);
    return S3G_ERR_INVALID_ARG;
  }
  if (algorithm != S3G_HEX_SLAB && algorithm != S3G_HEX_SLAB_DIV) {
    set_error("s3g_hexplane_backward_algo: unknown algorithm %d", algorithm);
    return S3G_ERR_INVALID_ARG;
  }
  if (algorithm != S3G_HEX_SLAB && !features && P > 0) {
    set_error("s3g_hexplane_backward_algo: this algorithm needs the forward's output `features`");
    return S3G_ERR_INVALID_ARG;
  }
  return hexplane_backward_impl(d, P, xyz, time, dL_dfeatures, features, algorithm, dL_dxyz, dL_dplanes, workspace, sort_state,
                                sort_reuse, stream_);
}
