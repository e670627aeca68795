// Rasterizer forward, stage 4: front-to-back alpha/depth blending, one 16x16 tile per workgroup (4 wave64), one pixel per lane.
// Per batch of 256 Gaussians the workgroup gathers (mean2D, conic, opacity, rgb, depth) into LDS with one
// coalesced index read + L2-resident attribute gathers; the inner loop then reads wave-uniform LDS
// addresses (broadcast).  The conic is pre-scaled by -0.5*log2(e) / -log2(e) while staging so the
// Gaussian weight is a bare v_exp_f32:  alpha = min(0.99, o * exp2(qa*dx*dx + qc*dy*dy + qb*dx*dy)).
#include "geom_math.hpp"

namespace s3g {

// NX = 3: a second image with other per-Gaussian colours (colors2 -> out_color2) is blended in the same pass; the
// alpha test, exp2 and the transmittance recurrence are shared.
template <int NX>
__global__ void __launch_bounds__(256)
blend_forward_kernel(int W, int H, int gx, int tiles, const uint2* __restrict__ ranges,
                     const uint32_t* __restrict__ point_list, const float2* __restrict__ means2D,
                     const float4* __restrict__ conic_opacity, const float* __restrict__ colors,
                     const float* __restrict__ depths, const float* __restrict__ bg, float* __restrict__ final_T,
                     uint32_t* __restrict__ n_contrib, uint32_t* __restrict__ tile_hi, float* __restrict__ out_color,
                     float* __restrict__ out_depth, const float* __restrict__ colors2, float* __restrict__ out_color2) {
  __shared__ StagedGaussian sg[256];
  __shared__ float4 sg2[NX ? 256 : 1];
  __shared__ uint32_t wave_hi[4];
  const uint32_t tile = xcd_swizzle(blockIdx.x, gridDim.x);
  if (tile >= (uint32_t)tiles) return;
  const int tx = tile % gx, ty = tile / gx;
  const int tid = threadIdx.x;
  const int px = tx * TILE_X + (tid & 15), py = ty * TILE_Y + (tid >> 4);
  const bool inside = px < W && py < H;
  const float pxf = (float)px, pyf = (float)py;
  const uint2 rg = ranges[tile];
  int todo = (int)(rg.y - rg.x);

  bool done = !inside;
  float T = 1.f, Cr = 0.f, Cg = 0.f, Cb = 0.f, D = 0.f;
  float C2r = 0.f, C2g = 0.f, C2b = 0.f;
  uint32_t contributor = 0, last_contributor = 0;

  for (uint32_t base = rg.x; base < rg.y; base += 256, todo -= 256) {
    if (__syncthreads_count(done) == 256) break;  // also protects sg[] reuse
    if (base + tid < rg.y) {
      const uint32_t id = point_list[base + tid];
      sg[tid] = stage_gaussian(id, means2D, conic_opacity, depths, colors);
      if (NX) sg2[tid] = make_float4(colors2[3 * (size_t)id], colors2[3 * (size_t)id + 1], colors2[3 * (size_t)id + 2], 0.f);
    }
    __syncthreads();
    const int cnt = min(256, todo);
    for (int j = 0; !done && j < cnt; j++) {
      contributor++;
      const float4 A = sg[j].a;
      const float dx = A.x - pxf, dy = A.y - pyf;
      const float4 B = sg[j].b;
      const float q = gaussian_exponent2(dx, dy, A.z, A.w, B.x);
      if (q > 0.f) continue;
      const float alpha = fminf(0.99f, B.y * __builtin_amdgcn_exp2f(q));
      if (alpha < 1.0f / 255.0f) continue;
      const float test_T = T * (1.f - alpha);
      if (test_T < 0.0001f) {
        done = true;
        continue;
      }
      const float w = alpha * T;
      const float4 Cc = sg[j].c;
      Cr = __builtin_fmaf(B.w, w, Cr);
      Cg = __builtin_fmaf(Cc.x, w, Cg);
      Cb = __builtin_fmaf(Cc.y, w, Cb);
      D = __builtin_fmaf(B.z, w, D);
      if (NX) {
        const float4 C2 = sg2[j];
        C2r = __builtin_fmaf(C2.x, w, C2r);
        C2g = __builtin_fmaf(C2.y, w, C2g);
        C2b = __builtin_fmaf(C2.z, w, C2b);
      }
      T = test_T;
      last_contributor = contributor;
    }
  }
  if (inside) {
    const size_t pix = (size_t)py * W + px, N = (size_t)H * W;
    final_T[pix] = T;
    n_contrib[pix] = last_contributor;
    out_color[pix] = Cr + T * bg[0];
    out_color[N + pix] = Cg + T * bg[1];
    out_color[2 * N + pix] = Cb + T * bg[2];
    out_depth[pix] = D;
    if (NX) {
      out_color2[pix] = C2r + T * bg[0];
      out_color2[N + pix] = C2g + T * bg[1];
      out_color2[2 * N + pix] = C2b + T * bg[2];
    }
  }
  // end (absolute list position) of the deepest contributor of the tile: the backward never looks behind it
  uint32_t m = inside ? last_contributor : 0u;
  for (int off = 32; off >= 1; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off));
  if ((tid & 63) == 0) wave_hi[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) tile_hi[tile] = rg.x + max(max(wave_hi[0], wave_hi[1]), max(wave_hi[2], wave_hi[3]));
}

// ---- static / dynamic decomposition renders of one geometry in ONE blend pass -------------------------
// gaussian_renderer/__init__.py:168-204 renders the Gaussians with max|dx| above / below the mean a second and third time
// (full preprocess + binning + sort + blend on boolean-masked copies of every input).  A subset's per-tile list is the full
// list with the other class removed -- same depth order, ties still by index -- so both subset images fall out of one walk
// over the FULL sorted lists with one transmittance chain per class: alpha is evaluated once per (pixel, Gaussian) and
// updates only the chain of the Gaussian's class.  Results are bit-identical to the two separate subset renders.
__global__ void __launch_bounds__(256)
blend_decompose_kernel(int W, int H, int gx, int tiles, const uint2* __restrict__ ranges,
                       const uint32_t* __restrict__ point_list, const float2* __restrict__ means2D,
                       const float4* __restrict__ conic_opacity, const float* __restrict__ colors,
                       const float* __restrict__ depths, const float* __restrict__ bg, const uint8_t* __restrict__ cls,
                       const long long* __restrict__ class_counts /* [2]: static, dynamic; NULL = both non-empty */,
                       float* __restrict__ out_color_d, float* __restrict__ out_depth_d, float* __restrict__ out_color_s,
                       float* __restrict__ out_depth_s) {
  __shared__ StagedGaussian sg[256];
  __shared__ uint16_t sub[2][256];      // the batch's entries of each class, in list order
  __shared__ int wave_cnt[2][4];
  const uint32_t tile = xcd_swizzle(blockIdx.x, gridDim.x);
  if (tile >= (uint32_t)tiles) return;
  const int tx = tile % gx, ty = tile / gx;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int px = tx * TILE_X + (tid & 15), py = ty * TILE_Y + (tid >> 4);
  const bool inside = px < W && py < H;
  const float pxf = (float)px, pyf = (float)py;
  const uint2 rg = ranges[tile];
  // one chain per class, each in its own scalar variables and its own loop over the class's sub-list of the batch: a chain
  // stops at ITS saturation, never pays for the other class's entries, and nothing is indexed by a run-time class (the first
  // version walked the full list once with T[k], C[k] selected per entry: 0.70 ms against 0.23 ms for the plain blend pass)
  bool done_s = !inside, done_d = !inside;
  float Ts = 1.f, Crs = 0.f, Cgs = 0.f, Cbs = 0.f, Ds = 0.f;
  float Td = 1.f, Crd = 0.f, Cgd = 0.f, Cbd = 0.f, Dd = 0.f;
  auto chain = [&](const uint16_t* __restrict__ list, int n, bool& done, float& T, float& Cr, float& Cg, float& Cb, float& D) {
    for (int j = 0; !done && j < n; j++) {
      const int e = list[j];
      const float4 A = sg[e].a;
      const float dx = A.x - pxf, dy = A.y - pyf;
      const float4 B = sg[e].b;
      const float q = gaussian_exponent2(dx, dy, A.z, A.w, B.x);
      if (q > 0.f) continue;
      const float alpha = fminf(0.99f, B.y * __builtin_amdgcn_exp2f(q));
      if (alpha < 1.0f / 255.0f) continue;
      const float test_T = T * (1.f - alpha);
      if (test_T < 0.0001f) {
        done = true;
        continue;
      }
      const float w = alpha * T;
      const float4 Cc = sg[e].c;
      Cr = __builtin_fmaf(B.w, w, Cr);
      Cg = __builtin_fmaf(Cc.x, w, Cg);
      Cb = __builtin_fmaf(Cc.y, w, Cb);
      D = __builtin_fmaf(B.z, w, D);
      T = test_T;
    }
  };
  for (uint32_t base = rg.x; base < rg.y; base += 256) {
    if (__syncthreads_count(done_s && done_d) == 256) break;   // also protects sg[] / sub[] reuse
    const bool valid = base + tid < rg.y;
    int c = 0;
    if (valid) {
      const uint32_t id = point_list[base + tid];
      sg[tid] = stage_gaussian(id, means2D, conic_opacity, depths, colors);
      c = cls[id] ? 1 : 0;
    }
    // stable partition of the batch by class: ballots inside the wave, a 4-entry prefix across the waves
    const unsigned long long b1 = __ballot(valid && c == 1), b0 = __ballot(valid && c == 0);
    if (lane == 0) { wave_cnt[0][wave] = __popcll(b0); wave_cnt[1][wave] = __popcll(b1); }
    __syncthreads();
    int off0 = 0, off1 = 0, n0 = 0, n1 = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      if (w < wave) { off0 += wave_cnt[0][w]; off1 += wave_cnt[1][w]; }
      n0 += wave_cnt[0][w]; n1 += wave_cnt[1][w];
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    if (valid) sub[c][(c ? off1 + __popcll(b1 & below) : off0 + __popcll(b0 & below))] = (uint16_t)tid;
    __syncthreads();
    chain(sub[0], n0, done_s, Ts, Crs, Cgs, Cbs, Ds);
    chain(sub[1], n1, done_d, Td, Crd, Cgd, Cbd, Dd);
  }
  const float T[2] = {Ts, Td}, Cr[2] = {Crs, Crd}, Cg[2] = {Cgs, Cgd}, Cb[2] = {Cbs, Cbd}, D[2] = {Ds, Dd};
  if (inside) {
    const size_t pix = (size_t)py * W + px, N = (size_t)H * W;
    // an EMPTY class renders as zeros WITHOUT background, like the reference's P == 0 early-out (rasterize_points.cu:81-116)
    const float ks = (class_counts && class_counts[0] == 0) ? 0.f : 1.f, kd = (class_counts && class_counts[1] == 0) ? 0.f : 1.f;
    out_color_s[pix] = ks * (Cr[0] + T[0] * bg[0]);
    out_color_s[N + pix] = ks * (Cg[0] + T[0] * bg[1]);
    out_color_s[2 * N + pix] = ks * (Cb[0] + T[0] * bg[2]);
    out_depth_s[pix] = D[0];
    out_color_d[pix] = kd * (Cr[1] + T[1] * bg[0]);
    out_color_d[N + pix] = kd * (Cg[1] + T[1] * bg[1]);
    out_color_d[2 * N + pix] = kd * (Cb[1] + T[1] * bg[2]);
    out_depth_d[pix] = D[1];
  }
}

int launch_blend_forward(const Arenas& a, const float* colors, const float* bg, float* out_color, float* out_depth,
                         const float* colors2, float* out_color2, double instances, hipStream_t stream, bool debug) {
  const GeomState& g = a.g;
  const ImageState& im = a.im;
  if (colors2 == nullptr) out_color2 = nullptr;
  profile_begin(S3G_PROFILE_BLEND_FORWARD, stream);
  hipLaunchKernelGGL(colors2 ? blend_forward_kernel<3> : blend_forward_kernel<0>, dim3(tile_blocks(a.tiles)), dim3(256), 0, stream,
                     a.W, a.H, a.gx, a.tiles, im.ranges, a.b.point_list, g.means2D, g.conic_opacity, colors, g.depths, bg,
                     im.final_T, im.n_contrib, im.tile_hi, out_color, out_depth, colors2, out_color2);
  profile_end(S3G_PROFILE_BLEND_FORWARD, stream, instances, (double)a.W * a.H);
  S3G_KERNEL_CHECK(stream, debug);
  return S3G_OK;
}

}  // namespace s3g

using namespace s3g;

// Second (third, ...) render of the SAME geometry with different per-Gaussian colours (the reference renders RGB and
// then the feature image with identical means/scales/rotations/opacities, gaussian_renderer/__init__.py:127-166):
// everything up to the sorted per-tile lists is reused from the arenas of the first call; only the blend runs.
extern "C" int s3g_raster_forward_reuse(const s3g_raster_inputs* in, int R, const void* geometry_arena,
                                        const void* binning_arena, void* image_arena, float* out_color, float* out_depth,
                                        void* stream_) {
  clear_error();
  hipStream_t stream = (hipStream_t)stream_;
  if (!in || !in->colors_precomp || !in->background || !geometry_arena || !image_arena || (R > 0 && !binning_arena) ||
      !out_color || !out_depth || in->P <= 0) {
    set_error("s3g_raster_forward_reuse: bad argument (needs colors_precomp and the arenas of a previous forward)");
    return S3G_ERR_INVALID_ARG;
  }
  const Arenas a = reopen_arenas(in, R, geometry_arena, binning_arena, image_arena);
  return launch_blend_forward(a, in->colors_precomp, in->background, out_color, out_depth, nullptr, nullptr, (double)R, stream,
                              in->debug != 0);
}

extern "C" int s3g_raster_forward_decompose(const s3g_raster_inputs* in, int R, const void* geometry_arena,
                                            const void* binning_arena, const void* image_arena, const uint8_t* is_dynamic,
                                            const long long* class_counts, float* out_color_d, float* out_depth_d, float* out_color_s, float* out_depth_s,
                                            void* stream_) {
  clear_error();
  hipStream_t stream = (hipStream_t)stream_;
  if (!in || !in->background || !geometry_arena || !image_arena || (R > 0 && !binning_arena) || !is_dynamic ||
      !out_color_d || !out_depth_d || !out_color_s || !out_depth_s || in->P <= 0) {
    set_error("s3g_raster_forward_decompose: bad argument (needs the arenas of a previous forward and the class mask)");
    return S3G_ERR_INVALID_ARG;
  }
  const Arenas a = reopen_arenas(in, R, geometry_arena, binning_arena, image_arena);
  const float* color_ptr = in->colors_precomp ? in->colors_precomp : a.g.rgb;   // SH path: the forward's own colours
  hipLaunchKernelGGL(blend_decompose_kernel, dim3(tile_blocks(a.tiles)), dim3(256), 0, stream, a.W, a.H, a.gx, a.tiles,
                     a.im.ranges, a.b.point_list, a.g.means2D, a.g.conic_opacity, color_ptr, a.g.depths, in->background, is_dynamic,
                     class_counts, out_color_d, out_depth_d, out_color_s, out_depth_s);
  S3G_KERNEL_CHECK(stream, in->debug != 0);
  return S3G_OK;
}
