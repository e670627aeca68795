// Rasterizer backward, stage 1: back-to-front blend gradients, one 16x16 tile per workgroup (4 wave64), one pixel per lane.
// VALU-bound.  Steps 1-4 of the scheme in raster_backward.hip: per (pixel, Gaussian) the ten (NX = 3: thirteen) sums, reduced
// over the 16 lanes of a row with DPP adds, parked in LDS slots per (wave, row), and once per 32-Gaussian batch added in fixed
// order into the Gaussian's record at its position in the sorted list.  No atomics; bit-reproducible.
#include "geom_math.hpp"
#include "raster_dev.hpp"

namespace s3g {

// ---- transpose-reduce: NV values summed over the 16 lanes of a row with 29 DPP adds instead of 4 NV = 52 ----
// A plain reduction sums every value in every lane.  Here each step also splits the values between the two partners:
//   A  lane i <-> i ^ 8 (row_ror:8):        lanes 0-7 go on with values 0-7, lanes 8-15 with values 8-15;
//   B  lane i <-> 7 - i (row_half_mirror):  banks (groups of four lanes) 0 / 2 keep the low four of their eight, banks 1 / 3 the high four;
//   C, D  quad_perm butterflies inside a bank: every lane of bank b ends with the row totals of values 4b .. 4b+3.
// "keep these, take the partner's" needs no selects: a DPP instruction writes only the lanes its bank_mask enables (bank =
// four consecutive lanes of a row), so `v_add_f32_dpp r, x, x bank_mask:0x3` followed by `v_add_f32_dpp r, y, y bank_mask:0xc`
// leaves x + x' in lanes 0-7 and y + y' in lanes 8-15 of the same register.  Inline asm because the builtin (update_dpp + add)
// cannot express an add whose WRITE is masked; the s_nop covers the VALU-write -> DPP-read hazard (2 wait states) that the
// compiler does not track through inline asm.  Lanes of a bank whose values do not exist (>= NV) hold finite garbage that is
// never stored.  The reduction stops at row totals, which the kernel parks in LDS: the two row_bcast steps that would finish a
// wave total cost three instructions each (zero, v_mov_dpp, add) per value in a kernel that is bound by VALU issue.
// first write of a register (its other lanes are overwritten by the S3G_DPP_ACC that follows, or never read)
#define S3G_DPP_SET(dst, src, ctrl, bank) \
  asm volatile("v_add_f32_dpp %0, %1, %1 " ctrl " row_mask:0xf bank_mask:" bank : "=v"(dst) : "v"(src))
#define S3G_DPP_ACC(dst, src, ctrl, bank) \
  asm volatile("v_add_f32_dpp %0, %1, %1 " ctrl " row_mask:0xf bank_mask:" bank : "+v"(dst) : "v"(src))
#define S3G_DPP_SELF(dst, ctrl) asm volatile("v_add_f32_dpp %0, %0, %0 " ctrl " row_mask:0xf bank_mask:0xf" : "+v"(dst))
template <int NV>
__device__ __forceinline__ void row_transpose_reduce(const float* v /* [NV] */, float* q /* [4] */) {
  static_assert(NV > 8 && NV <= 16, "values per visit");
  float r[8];
  asm volatile("s_nop 1");
#pragma unroll
  for (int i = 0; i < 8; i++) {
    S3G_DPP_SET(r[i], v[i], "row_ror:8", "0x3");
    if (i + 8 < NV) S3G_DPP_ACC(r[i], v[i + 8], "row_ror:8", "0xc");
  }
  asm volatile("s_nop 1");
#pragma unroll
  for (int i = 0; i < 4; i++) {
    S3G_DPP_SET(q[i], r[i], "row_half_mirror", "0x5");
    S3G_DPP_ACC(q[i], r[i + 4], "row_half_mirror", "0xa");
  }
  asm volatile("s_nop 1");
#pragma unroll
  for (int i = 0; i < 4; i++) S3G_DPP_SELF(q[i], "quad_perm:[1,0,3,2]");
  asm volatile("s_nop 1");
#pragma unroll
  for (int i = 0; i < 4; i++) S3G_DPP_SELF(q[i], "quad_perm:[2,3,0,1]");
}

// record layout (NREC floats): dcolor r,g,b | ddepth | S0 | Sx | Sy | Sxx | Sxy | Syy   [| dcolor2 r,g,b | pad]
//
// NX = 3: TWO images blended from the same geometry (the RGB+depth render and the feature render of one iteration,
// gaussian_renderer/__init__.py:127-166) are back-propagated in ONE pass.  Everything that depends only on the geometry
// -- the alpha test, exp2, the transmittance recurrence, the six S sums and their wave reductions -- is shared; the second
// image adds its three colour-gradient sums and its term of dL/dalpha.  Records grow from 10 to 14 floats.
//
// AL: the accumulated opacity A = 1 - T_final is an output too and dL_dalpha_img [H*W] is its upstream gradient.  The
// background term below is dL/dT_final * dT_final/dalpha with dL/dT_final = bg . dL_dpixel; a loss on A adds -dL/dA to
// dL/dT_final, so the gradient enters as bg_dot - dL/dA[pix], once per pixel, and nowhere else.
template <int NX, bool AL = false>
__global__ void __launch_bounds__(256)
blend_backward_kernel(int W, int H, int gx, int tiles, const uint2* __restrict__ ranges,
                      const uint32_t* __restrict__ tile_hi, const uint32_t* __restrict__ point_list,
                      const float* __restrict__ bg, const float2* __restrict__ means2D,
                      const float4* __restrict__ conic_opacity, const float* __restrict__ colors,
                      const float* __restrict__ depths, const float* __restrict__ final_Ts,
                      const uint32_t* __restrict__ n_contrib, const float* __restrict__ dL_dpixels,
                      const float* __restrict__ dL_dpixel_depths, float* __restrict__ records /*[R][NR]*/,
                      const float* __restrict__ colors2, const float* __restrict__ dL_dpixels2, int wave_bounds,
                      const float* __restrict__ dL_dalpha_img) {
  constexpr uint32_t BATCH = 32;  // Gaussians staged per round (one bit each in a wave's visit mask)
  constexpr int NR = NX ? NREC + 4 : NREC;
  constexpr int SLOTS = 16;       // 4 waves x 4 rows of 16 lanes
  __shared__ StagedGaussian sg[BATCH];
  __shared__ float4 sg2[NX ? BATCH : 1];  // second image's colour
  // one slot per (wave, row): combined in fixed order -> bit-reproducible sums.  A slot holds NV value rows of RS floats (rows >= NV,
  // which the transpose-reduce also produces, are not stored): 29.5 KiB of LDS in all for NX = 3, five workgroups per CU (16 rows
  // of 32 + 16 floats: 35 KiB, four).  RS = BATCH + 1: the eight row leaders of a 32-lane group (four lane banks b x two slots)
  // store row 4b + i of their slots at once; with 33-float rows the four b land 4 LDS banks apart and the two slots 13 (NX = 3)
  // or 10 (NX = 0) apart: eight distinct banks (32-float rows: four leaders per bank).
  constexpr int NV = NX ? NREC + 3 : NREC;   // sums per visit
  constexpr int RS = BATCH + 1;
  constexpr int SLOT_FLOATS = NV * RS;
  __shared__ float acc[SLOTS][SLOT_FLOATS];
  // bit j of visited[w]: wave w stored its four slots of entry j in this batch.  The slots are never cleared; the epilogue adds
  // +0 for an entry a wave did not visit, which is what the cleared slot held -- the same additions in the same order.
  __shared__ uint32_t visited[4];

  const uint32_t tile = xcd_swizzle(blockIdx.x, gridDim.x);
  if (tile >= (uint32_t)tiles) return;
  const uint2 rg = ranges[tile];
  const uint32_t hi = tile_hi[tile] - rg.x;  // deepest contributor of the tile (1-based); nothing behind it gets gradient
  if (hi == 0) return;
  const int tx = tile % gx, ty = tile / gx;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int px = tx * TILE_X + (tid & 15), py = ty * TILE_Y + (tid >> 4);
  const bool inside = px < W && py < H;
  const float pxf = (float)px, pyf = (float)py;
  const size_t pix = (size_t)py * W + px, N = (size_t)H * W;

  const float T_final = inside ? final_Ts[pix] : 0.f;
  const uint32_t last_contributor = inside ? n_contrib[pix] : 0u;
  // The wave's own bound: no pixel of the wave takes gradient from an entry at pos >= whi (the forward's per-wave maximum of
  // n_contrib, whose tile maximum is tile_hi).  Entries between whi and hi are skipped by a scalar loop bound, before their LDS
  // reads; they change no state and store no slot.  wave_bounds = 0 walks every wave from hi (the schedule before the bound).
  uint32_t whi = last_contributor;
  for (int off = 32; off >= 1; off >>= 1) whi = max(whi, (uint32_t)__shfl_xor((int)whi, off));
  whi = wave_bounds ? __builtin_amdgcn_readfirstlane(whi) : hi;
  float gr = 0.f, gg = 0.f, gb = 0.f, gd = 0.f;
  if (inside) {
    gr = dL_dpixels[pix];
    gg = dL_dpixels[N + pix];
    gb = dL_dpixels[2 * N + pix];
    gd = dL_dpixel_depths[pix];
  }
  float g2r = 0.f, g2g = 0.f, g2b = 0.f;
  if (NX && inside) {
    g2r = dL_dpixels2[pix];
    g2g = dL_dpixels2[N + pix];
    g2b = dL_dpixels2[2 * N + pix];
  }
  float bg_dot = bg[0] * gr + bg[1] * gg + bg[2] * gb;
  if (NX) bg_dot += bg[0] * g2r + bg[1] * g2g + bg[2] * g2b;
  if (AL) bg_dot -= inside ? dL_dalpha_img[pix] : 0.f;

  float T = T_final;
  float ar = 0.f, ag = 0.f, ab = 0.f, ad = 0.f;  // accum_rec (colour, depth)
  float last_alpha = 0.f, lr = 0.f, lg = 0.f, lb = 0.f, ld = 0.f;
  float a2r = 0.f, a2g = 0.f, a2b = 0.f, l2r = 0.f, l2g = 0.f, l2b = 0.f;  // second image

  for (uint32_t done_cnt = 0; done_cnt < hi; done_cnt += BATCH) {
    const uint32_t cnt = min(BATCH, hi - done_cnt);
    __syncthreads();  // previous batch fully consumed (sg, acc, visited)
    if ((uint32_t)tid < cnt) {
      const uint32_t pos = hi - 1 - (done_cnt + tid);  // back to front
      const uint32_t id = point_list[rg.x + pos];
      const float2 mm = means2D[id];
      const float4 co = conic_opacity[id];
      StagedGaussian s;
      s.a = make_float4(mm.x, mm.y, -0.5f * LOG2E * co.x, -LOG2E * co.y);
      s.b = make_float4(-0.5f * LOG2E * co.z, co.w, depths[id], colors[3 * (size_t)id]);
      s.c = make_float4(colors[3 * (size_t)id + 1], colors[3 * (size_t)id + 2], 0.f, 0.f);
      sg[tid] = s;
      if (NX) sg2[tid] = make_float4(colors2[3 * (size_t)id], colors2[3 * (size_t)id + 1], colors2[3 * (size_t)id + 2], 0.f);
    }
    __syncthreads();

    // entries j < j0 lie at pos >= whi (wave-uniform); a wave with j0 >= cnt goes straight to the barrier
    const uint32_t j0 = hi - done_cnt > whi ? hi - done_cnt - whi : 0u;
    uint32_t vis = 0u;
    for (uint32_t j = j0; j < cnt; j++) {
      const uint32_t pos = hi - 1 - (done_cnt + j);  // 0-based position in the tile list
      // the reference's `contributor` equals pos after its decrement; it skips when contributor >= last_contributor
      bool valid = pos < last_contributor;
      const float4 A = sg[j].a;
      const float4 B = sg[j].b;
      const float dx = A.x - pxf, dy = A.y - pyf;
      const float q = gaussian_exponent2(dx, dy, A.z, A.w, B.x);
      const float G = __builtin_amdgcn_exp2f(q);
      const float alpha = fminf(0.99f, B.y * G);
      valid = valid && !(q > 0.f) && !(alpha < 1.0f / 255.0f);
      if (__ballot(valid) == 0ull) continue;  // wave-uniform: this Gaussian misses all 64 pixels of the wave
      vis |= 1u << j;

      float p_r = 0.f, p_g = 0.f, p_b = 0.f, p_d = 0.f, s0 = 0.f, sx = 0.f, sy = 0.f, sxx = 0.f, sxy = 0.f, syy = 0.f;
      float p2_r = 0.f, p2_g = 0.f, p2_b = 0.f;
      if (valid) {
        const float4 Cc = sg[j].c;
        const float cr = B.w, cg = Cc.x, cb = Cc.y, cd = B.z;
        const float rcp = __builtin_amdgcn_rcpf(1.f - alpha);
        T = T * rcp;
        const float w = alpha * T;  // dchannel_dcolor
        const float one_m_la = 1.f - last_alpha;
        ar = last_alpha * lr + one_m_la * ar;
        ag = last_alpha * lg + one_m_la * ag;
        ab = last_alpha * lb + one_m_la * ab;
        ad = last_alpha * ld + one_m_la * ad;
        lr = cr; lg = cg; lb = cb; ld = cd;
        float dL_dalpha = (cr - ar) * gr + (cg - ag) * gg + (cb - ab) * gb + (cd - ad) * gd;
        if (NX) {
          const float4 C2 = sg2[j];
          a2r = last_alpha * l2r + one_m_la * a2r;
          a2g = last_alpha * l2g + one_m_la * a2g;
          a2b = last_alpha * l2b + one_m_la * a2b;
          l2r = C2.x; l2g = C2.y; l2b = C2.z;
          dL_dalpha += (C2.x - a2r) * g2r + (C2.y - a2g) * g2g + (C2.z - a2b) * g2b;
          p2_r = w * g2r; p2_g = w * g2g; p2_b = w * g2b;
        }
        dL_dalpha *= T;
        last_alpha = alpha;
        dL_dalpha += (-T_final * rcp) * bg_dot;
        p_r = w * gr; p_g = w * gg; p_b = w * gb; p_d = w * gd;
        const float v = dL_dalpha * G;
        const float vx = v * dx, vy = v * dy;
        s0 = v; sx = vx; sy = vy; sxx = vx * dx; sxy = vx * dy; syy = vy * dy;
      }
      // wave-uniform from here: all 64 lanes take part in the DPP reductions (within rows of 16 lanes); values in record order
      const float vals[13] = {p_r, p_g, p_b, p_d, s0, sx, sy, sxx, sxy, syy, p2_r, p2_g, p2_b};
      float q4[4];
      row_transpose_reduce<NV>(vals, q4);
      if ((lane & 3) == 0) {   // the first lane of bank b stores the row totals of values 4b .. 4b+3 (rows >= NV: not stored)
        float* aw = &acc[wave * 4 + (lane >> 4)][(lane & 12) * RS + j];
#pragma unroll
        for (int i = 0; i < 4; i++)
          if ((lane & 12) + i < NV) aw[i * RS] = q4[i];
      }
    }
    if (lane == 0) visited[wave] = vis;
    __syncthreads();
    // Epilogue of the batch: thread (k, g) adds values 2k, 2k+1 of Gaussian g over the 16 slots in fixed order (rows of wave 0,
    // then wave 1, ...) and stores that float pair of its record (zeros if untouched).  Lanes 0-31 of a read are 32 consecutive
    // floats: no bank conflicts.
    const uint32_t g = (uint32_t)tid % BATCH, k = (uint32_t)tid / BATCH;
    if (k < NR / 2 && g < cnt) {
      uint32_t seen[4];   // all ones if the wave visited Gaussian g, else 0: slot value & seen = the slot or +0.0f
#pragma unroll
      for (int w = 0; w < 4; w++) seen[w] = 0u - ((visited[w] >> g) & 1u);
      auto slot = [&](int q, uint32_t v) { return __uint_as_float(__float_as_uint(acc[q][v * RS + g]) & seen[q / 4]); };
      const uint32_t v1 = 2 * k + 1 < (uint32_t)NV ? 2 * k + 1 : 2 * k;   // the pad float: any row of the slot, not used
      float lo = slot(0, 2 * k), hi2 = slot(0, v1);
#pragma unroll
      for (int q = 1; q < SLOTS; q++) {
        lo += slot(q, 2 * k);
        hi2 += slot(q, v1);
      }
      const uint32_t pos = hi - 1 - (done_cnt + g);
      float2* rec = reinterpret_cast<float2*>(records + (size_t)(rg.x + pos) * NR);
      rec[k] = make_float2(lo, 2 * k + 1 < (uint32_t)NV ? hi2 : 0.f);   // the pad float of a 14-float record stays 0
    }
  }
}

static bool g_wave_bounds = true;   // per-wave visit bounds (s3g_raster_set_backward_wave_bounds)

int launch_blend_backward(const Arenas& a, bool two_images, bool alpha, const float* colors, const float* bg,
                          const float* dL_dpix, const float* dL_dpix_depth, float* records, const float* colors2,
                          const float* dL_dpix2, const float* dL_dalpha, double instances, hipStream_t stream, bool debug) {
  const GeomState& g = a.g;
  const ImageState& im = a.im;
  auto* kernel = blend_backward_kernel<0, false>;
  switch ((two_images ? 2 : 0) | (alpha ? 1 : 0)) {
    case 1: kernel = blend_backward_kernel<0, true>; break;
    case 2: kernel = blend_backward_kernel<3, false>; break;
    case 3: kernel = blend_backward_kernel<3, true>; break;
  }
  profile_begin(S3G_PROFILE_BLEND_BACKWARD, stream);
  hipLaunchKernelGGL(kernel, dim3(tile_blocks(a.tiles)), dim3(256), 0, stream, a.W, a.H, a.gx, a.tiles, im.ranges, im.tile_hi,
                     a.b.point_list, bg, g.means2D, g.conic_opacity, colors, g.depths, im.final_T, im.n_contrib, dL_dpix,
                     dL_dpix_depth, records, colors2, dL_dpix2, g_wave_bounds ? 1 : 0, dL_dalpha);
  profile_end(S3G_PROFILE_BLEND_BACKWARD, stream, instances, (double)a.W * a.H);
  S3G_KERNEL_CHECK(stream, debug);
  return S3G_OK;
}

}  // namespace s3g

extern "C" int s3g_raster_set_backward_wave_bounds(int on) {
  const int prev = s3g::g_wave_bounds ? 1 : 0;
  s3g::g_wave_bounds = on != 0;
  return prev;
}
