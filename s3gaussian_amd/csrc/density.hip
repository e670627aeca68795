// Adaptive density control (include/s3g_density.h): classify -> scan -> apply, and the opacity reset.  HBM-bound: one densify or
// prune event reads and writes every per-Gaussian float and both Adam moments once (708 B per Gaussian at SH degree 3).
#include "common.hpp"

#include "../../include/s3g_density.h"

namespace s3g {

constexpr int DB = S3G_DENSITY_BLOCK;   // Gaussians (= threads) per workgroup of classify and apply: four waves
constexpr int DW = DB / WAVE;
static_assert(DB == 256 && DW == 4, "the block prefix below is written for four waves");

__device__ __forceinline__ float max_scale(const float* __restrict__ scaling, int i) {
  // torch.max(exp(_scaling), dim=1): exp first, then the maximum, like the reference's get_scaling
  const float a = expf(scaling[(size_t)i * 3]), b = expf(scaling[(size_t)i * 3 + 1]), c = expf(scaling[(size_t)i * 3 + 2]);
  return fmaxf(fmaxf(a, b), c);
}

// per-workgroup class counts from wave ballots: thread 0 writes the three words
__device__ __forceinline__ void block_class_counts(int cls, uint32_t* __restrict__ block_counts) {
  __shared__ uint32_t s_cnt[DW][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long mc = __ballot(cls == S3G_DENSITY_CLONE), ms = __ballot(cls == S3G_DENSITY_SPLIT),
                           md = __ballot(cls == S3G_DENSITY_DROP);
  if (lane == 0) {
    s_cnt[wave][0] = (uint32_t)__popcll(mc);
    s_cnt[wave][1] = (uint32_t)__popcll(ms);
    s_cnt[wave][2] = (uint32_t)__popcll(md);
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int k = threadIdx.x;
    block_counts[(size_t)blockIdx.x * 3 + k] = s_cnt[0][k] + s_cnt[1][k] + s_cnt[2][k] + s_cnt[3][k];
  }
}

__global__ void __launch_bounds__(DB) classify_densify_kernel(int P, const float* __restrict__ accum, const float* __restrict__ denom,
                                                              const float* __restrict__ scaling, float th, float scale_th,
                                                              unsigned char* __restrict__ cls, uint32_t* __restrict__ block_counts) {
  const int i = blockIdx.x * DB + threadIdx.x;
  int c = -1;                               // rows past the end belong to no class
  if (i < P) {
    float g = accum[i] / denom[i];          // grads = xyz_gradient_accum / denom; grads[grads.isnan()] = 0.0
    if (g != g) g = 0.f;
    const float ms = max_scale(scaling, i);
    c = S3G_DENSITY_KEEP;
    if (fabsf(g) >= th && ms <= scale_th) c = S3G_DENSITY_CLONE;        // torch.norm(grads, dim=-1) >= th  (a [P,1] norm: |g|)
    else if (g >= th && ms > scale_th) c = S3G_DENSITY_SPLIT;           // padded_grad >= th
    cls[i] = (unsigned char)c;
  }
  block_class_counts(c, block_counts);
}

__global__ void __launch_bounds__(DB) classify_prune_kernel(int P, const float* __restrict__ opacity, const float* __restrict__ scaling,
                                                            const float* __restrict__ max_radii, float min_opacity, float max_screen,
                                                            float world_th, unsigned char* __restrict__ cls,
                                                            uint32_t* __restrict__ block_counts) {
  const int i = blockIdx.x * DB + threadIdx.x;
  int c = -1;
  if (i < P) {
    const float o = 1.f / (1.f + expf(-opacity[i]));     // torch.sigmoid
    bool drop = o < min_opacity;
    if (max_screen > 0.f) drop = drop || max_radii[i] > max_screen || max_scale(scaling, i) > world_th;
    c = drop ? S3G_DENSITY_DROP : S3G_DENSITY_KEEP;
    cls[i] = (unsigned char)c;
  }
  block_class_counts(c, block_counts);
}

// One workgroup: every thread sums a contiguous run of workgroup counts, the 1024 run sums are scanned in LDS, every thread then
// writes the exclusive prefixes of its run.  ~10 k counts at 2.5 M Gaussians.
constexpr int SCAN_T = 1024;
__global__ void __launch_bounds__(SCAN_T) scan_kernel(int nb, uint32_t* __restrict__ counts, uint32_t* __restrict__ totals) {
  __shared__ uint32_t s[3][SCAN_T];
  const int t = threadIdx.x;
  const int per = (nb + SCAN_T - 1) / SCAN_T;
  const int b0 = min(t * per, nb), b1 = min(b0 + per, nb);
  uint32_t sum[3] = {0u, 0u, 0u};
  for (int b = b0; b < b1; b++)
    for (int k = 0; k < 3; k++) sum[k] += counts[(size_t)b * 3 + k];
  for (int k = 0; k < 3; k++) s[k][t] = sum[k];
  __syncthreads();
  for (int d = 1; d < SCAN_T; d <<= 1) {     // Hillis-Steele inclusive scan over the run sums
    uint32_t v[3];
    for (int k = 0; k < 3; k++) v[k] = t >= d ? s[k][t - d] : 0u;
    __syncthreads();
    for (int k = 0; k < 3; k++) s[k][t] += v[k];
    __syncthreads();
  }
  uint32_t run[3];
  for (int k = 0; k < 3; k++) run[k] = s[k][t] - sum[k];
  for (int b = b0; b < b1; b++)
    for (int k = 0; k < 3; k++) {
      const uint32_t c = counts[(size_t)b * 3 + k];
      counts[(size_t)b * 3 + k] = run[k];
      run[k] += c;
    }
  if (t == SCAN_T - 1)
    for (int k = 0; k < 3; k++) totals[k] = s[k][t];
}

// ---- Philox4x32-10 (Salmon et al., SC'11) keyed on (seed, row): counter-based, so a deviate does not depend on the launch shape ----
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t out[4]) {
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// three standard normal deviates for noise row `row`: Box-Muller on 24-bit uniforms in (0, 1) (|z| <= 5.9)
__device__ __forceinline__ void philox_normal3(uint64_t seed, uint32_t row, float z[3]) {
  uint32_t x[4];
  philox4x32_10(row, 0u, 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), x);
  const float k = 1.f / 16777216.f;
  const float u0 = ((float)(x[0] >> 8) + 0.5f) * k, u1 = ((float)(x[1] >> 8) + 0.5f) * k;
  const float u2 = ((float)(x[2] >> 8) + 0.5f) * k, u3 = ((float)(x[3] >> 8) + 0.5f) * k;
  const float r0 = sqrtf(-2.f * logf(u0)), r1 = sqrtf(-2.f * logf(u2));
  float s0, c0, s1, c1;
  sincosf(6.28318530717958647692f * u1, &s0, &c0);
  sincosf(6.28318530717958647692f * u3, &s1, &c1);
  z[0] = r0 * c0; z[1] = r0 * s0; z[2] = r1 * c1;
}

struct ApplyArgs {
  s3g_density_plan p;
  s3g_density_tensor t[S3G_DENSITY_MAX_TENSORS];
  int n;
};

// grid = (workgroups of 256 source Gaussians, tensors + 1).  Slice y < n moves tensor y; slice y == n carries the byte-wide table and
// computes the split children.  Every workgroup rebuilds its destination rows from the class bytes and the scanned offsets (256
// bytes and three words: cheaper than a round trip of three index arrays through memory).
__global__ void __launch_bounds__(DB) apply_kernel(const ApplyArgs a) {
  __shared__ int s_dst[DW][3][WAVE];        // per wave: destination row of the original / its clone / its first child, or -1
  __shared__ uint32_t s_wave[DW][3];
  const s3g_density_plan& p = a.p;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * DB + threadIdx.x;
  const int c = i < p.P ? (int)p.cls[i] : -1;
  const unsigned long long below = (1ull << lane) - 1ull;
  const unsigned long long mc = __ballot(c == S3G_DENSITY_CLONE), ms = __ballot(c == S3G_DENSITY_SPLIT),
                           md = __ballot(c == S3G_DENSITY_DROP);
  if (lane == 0) {
    s_wave[wave][0] = (uint32_t)__popcll(mc);
    s_wave[wave][1] = (uint32_t)__popcll(ms);
    s_wave[wave][2] = (uint32_t)__popcll(md);
  }
  __syncthreads();
  uint32_t before[3];                        // clones / splits / drops in front of row i
  for (int k = 0; k < 3; k++) {
    uint32_t v = p.block_offsets[(size_t)blockIdx.x * 3 + k];
    for (int w = 0; w < wave; w++) v += s_wave[w][k];
    before[k] = v;
  }
  before[0] += (uint32_t)__popcll(mc & below);
  before[1] += (uint32_t)__popcll(ms & below);
  before[2] += (uint32_t)__popcll(md & below);
  const int n_keep = p.P - p.n_split - p.n_drop;
  const int d_keep = (c == S3G_DENSITY_KEEP || c == S3G_DENSITY_CLONE) ? i - (int)before[1] - (int)before[2] : -1;
  const int d_clone = c == S3G_DENSITY_CLONE ? n_keep + (int)before[0] : -1;
  const int d_child = c == S3G_DENSITY_SPLIT ? n_keep + p.n_clone + (int)before[1] : -1;
  const int n_split = p.n_split;

  if ((int)blockIdx.y == a.n) {
    // ---- the per-lane slice: table byte, split children ----
    if (p.table_src != nullptr && c >= 0) {
      const unsigned char b = p.table_src[i];
      if (d_keep >= 0) p.table_dst[d_keep] = b;
      if (d_clone >= 0) p.table_dst[d_clone] = b;
      if (d_child >= 0) { p.table_dst[d_child] = b; p.table_dst[d_child + n_split] = b; }
    }
    if (d_child >= 0) {
      const float* q = p.rotation + (size_t)i * 4;
      const float* sp = p.scaling + (size_t)i * 3;
      const float* xp = p.xyz + (size_t)i * 3;
      const float ls0 = sp[0], ls1 = sp[1], ls2 = sp[2];
      const float e0 = expf(ls0), e1 = expf(ls1), e2 = expf(ls2);
      // build_rotation(self._rotation[mask]): q / sqrt(r r + x x + y y + z z), rounded in that order
      const float norm = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
      const float r = q[0] / norm, x = q[1] / norm, y = q[2] / norm, z = q[3] / norm;
      const float R00 = 1.f - 2.f * (y * y + z * z), R01 = 2.f * (x * y - r * z), R02 = 2.f * (x * z + r * y);
      const float R10 = 2.f * (x * y + r * z), R11 = 1.f - 2.f * (x * x + z * z), R12 = 2.f * (y * z - r * x);
      const float R20 = 2.f * (x * z - r * y), R21 = 2.f * (y * z + r * x), R22 = 1.f - 2.f * (x * x + y * y);
      // scaling_inverse_activation(get_scaling / (0.8 * N)), N = 2
      const float n0 = logf(e0 / 1.6f), n1 = logf(e1 / 1.6f), n2 = logf(e2 / 1.6f);
      const float x0 = xp[0], x1 = xp[1], x2 = xp[2];
      for (int k = 0; k < 2; k++) {
        const size_t row = (size_t)k * n_split + (size_t)(d_child - n_keep - p.n_clone);
        float zz[3];
        if (p.noise != nullptr) { zz[0] = p.noise[row * 3]; zz[1] = p.noise[row * 3 + 1]; zz[2] = p.noise[row * 3 + 2]; }
        else philox_normal3(p.seed, (uint32_t)row, zz);
        if (p.noise_out != nullptr) { p.noise_out[row * 3] = zz[0]; p.noise_out[row * 3 + 1] = zz[1]; p.noise_out[row * 3 + 2] = zz[2]; }
        const float a0 = e0 * zz[0], a1 = e1 * zz[1], a2 = e2 * zz[2];          // torch.normal(mean = 0, std = exp(s))
        const size_t d = (size_t)(d_child + k * n_split) * 3;
        p.xyz_dst[d] = (R00 * a0 + R01 * a1 + R02 * a2) + x0;                     // bmm(R, samples) + xyz
        p.xyz_dst[d + 1] = (R10 * a0 + R11 * a1 + R12 * a2) + x1;
        p.xyz_dst[d + 2] = (R20 * a0 + R21 * a1 + R22 * a2) + x2;
        p.scaling_dst[d] = n0; p.scaling_dst[d + 1] = n1; p.scaling_dst[d + 2] = n2;
      }
    }
    return;
  }

  // ---- the streaming slice: wave `wave` owns source rows [i0, i0 + 64) and walks the tensor's contiguous 64 x width floats ----
  s_dst[wave][0][lane] = d_keep;
  s_dst[wave][1][lane] = d_clone;
  s_dst[wave][2][lane] = d_child;
  __syncthreads();                           // (blockIdx.y is uniform: every thread of a streaming workgroup arrives here)
  const s3g_density_tensor& t = a.t[blockIdx.y];
  const int i0 = blockIdx.x * DB + wave * WAVE;
  if (i0 >= p.P) return;
  const int w = t.width;
  const int rows = min(WAVE, p.P - i0);
  const int n = rows * w;
  const size_t sbase = (size_t)i0 * w;
  const float* __restrict__ src = t.src + sbase;
  float* __restrict__ dst = t.dst;
  const bool moments = t.src_exp_avg != nullptr;
  const float* __restrict__ sm = moments ? t.src_exp_avg + sbase : nullptr;
  const float* __restrict__ sv = moments ? t.src_exp_avg_sq + sbase : nullptr;
  float* __restrict__ dm = t.dst_exp_avg;
  float* __restrict__ dv = t.dst_exp_avg_sq;
  const bool copy_children = t.children_rewritten == 0;
  int r = lane / w, col = lane - r * w;      // element e = lane + 64 k sits in row r, column col; advanced without dividing again
  const int dr = WAVE / w, dc = WAVE - dr * w;
  for (int e = lane; e < n; e += WAVE) {
    const float v = src[e];
    float m1 = 0.f, m2 = 0.f;
    if (moments) { m1 = sm[e]; m2 = sv[e]; }
    const int dk = s_dst[wave][0][r], dl = s_dst[wave][1][r], ds = s_dst[wave][2][r];
    if (dk >= 0) {
      const size_t o = (size_t)dk * w + col;
      dst[o] = v;
      if (moments) { dm[o] = m1; dv[o] = m2; }
    }
    if (dl >= 0) {
      const size_t o = (size_t)dl * w + col;
      dst[o] = v;
      if (moments) { dm[o] = 0.f; dv[o] = 0.f; }
    }
    if (ds >= 0) {
      const size_t o0 = (size_t)ds * w + col, o1 = (size_t)(ds + n_split) * w + col;
      if (copy_children) { dst[o0] = v; dst[o1] = v; }
      if (moments) { dm[o0] = 0.f; dv[o0] = 0.f; dm[o1] = 0.f; dv[o1] = 0.f; }
    }
    col += dc; r += dr;
    if (col >= w) { col -= w; r++; }
  }
}

__global__ void __launch_bounds__(256) reset_opacity_kernel(int P, const float* __restrict__ opacity, float* __restrict__ out,
                                                            float* __restrict__ m, float* __restrict__ v) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const float y = fminf(1.f / (1.f + expf(-opacity[i])), 0.01f);    // torch.min(get_opacity, 0.01)
  out[i] = logf(y / (1.f - y));                                      // inverse_sigmoid
  if (m != nullptr) m[i] = 0.f;
  if (v != nullptr) v[i] = 0.f;
}

static inline int density_blocks(int P) { return P > 0 ? (P + DB - 1) / DB : 1; }

}  // namespace s3g

using namespace s3g;

extern "C" size_t s3g_density_count_words(int P) { return (size_t)3 * (size_t)density_blocks(P); }

extern "C" int s3g_density_classify_densify(int P, const float* xyz_gradient_accum, const float* denom, const float* scaling,
                                            float grad_threshold, float scale_threshold, unsigned char* cls, uint32_t* block_counts,
                                            void* stream_) {
  if (P < 0 || !block_counts || (P > 0 && (!xyz_gradient_accum || !denom || !scaling || !cls))) {
    set_error("s3g_density_classify_densify: bad argument");
    return S3G_ERR_INVALID_ARG;
  }
  hipLaunchKernelGGL(classify_densify_kernel, dim3(density_blocks(P)), dim3(DB), 0, (hipStream_t)stream_, P, xyz_gradient_accum, denom,
                     scaling, grad_threshold, scale_threshold, cls, block_counts);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" int s3g_density_classify_prune(int P, const float* opacity, const float* scaling, const float* max_radii2D, float min_opacity,
                                          float max_screen_size, float world_scale_threshold, unsigned char* cls,
                                          uint32_t* block_counts, void* stream_) {
  const bool sizes = max_screen_size > 0.f;
  if (P < 0 || !block_counts || (P > 0 && (!opacity || !cls || (sizes && (!scaling || !max_radii2D))))) {
    set_error("s3g_density_classify_prune: bad argument");
    return S3G_ERR_INVALID_ARG;
  }
  hipLaunchKernelGGL(classify_prune_kernel, dim3(density_blocks(P)), dim3(DB), 0, (hipStream_t)stream_, P, opacity, scaling, max_radii2D,
                     min_opacity, max_screen_size, world_scale_threshold, cls, block_counts);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" int s3g_density_scan(int P, uint32_t* block_counts, uint32_t* totals, void* stream_) {
  if (P < 0 || !block_counts || !totals) {
    set_error("s3g_density_scan: bad argument");
    return S3G_ERR_INVALID_ARG;
  }
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(SCAN_T), 0, (hipStream_t)stream_, density_blocks(P), block_counts, totals);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" int s3g_density_apply(const s3g_density_plan* plan, int n, const s3g_density_tensor* tensors, void* stream_) {
  if (!plan || n < 0 || n > S3G_DENSITY_MAX_TENSORS || (n > 0 && !tensors)) {
    set_error("s3g_density_apply: bad argument (at most %d tensors per call)", S3G_DENSITY_MAX_TENSORS);
    return S3G_ERR_INVALID_ARG;
  }
  const s3g_density_plan& p = *plan;
  if (p.P < 0 || p.n_clone < 0 || p.n_split < 0 || p.n_drop < 0 || (long long)p.n_clone + p.n_split + p.n_drop > (long long)p.P ||
      (long long)p.P + p.n_clone + p.n_split - p.n_drop > 0x7fffffffLL) {
    set_error("s3g_density_apply: counts (%d clone, %d split, %d drop) do not fit P = %d", p.n_clone, p.n_split, p.n_drop, p.P);
    return S3G_ERR_INVALID_ARG;
  }
  if (p.P == 0) return S3G_OK;
  if (!p.cls || !p.block_offsets || ((p.table_src != nullptr) != (p.table_dst != nullptr))) {
    set_error("s3g_density_apply: NULL class bytes / offsets, or a table with one end only");
    return S3G_ERR_INVALID_ARG;
  }
  if (p.n_split > 0) {
    if (!p.xyz || !p.scaling || !p.rotation || !p.xyz_dst || !p.scaling_dst) {
      set_error("s3g_density_apply: split rows need xyz, scaling, rotation and both outputs");
      return S3G_ERR_INVALID_ARG;
    }
    if (p.noise != nullptr && p.noise_rows < (size_t)2 * (size_t)p.n_split) {
      set_error("s3g_density_apply: noise has %zu rows, %d split rows need %zu", p.noise_rows, p.n_split, (size_t)2 * p.n_split);
      return S3G_ERR_INVALID_ARG;
    }
  }
  ApplyArgs a;
  memset(&a, 0, sizeof a);
  a.p = p;
  a.n = n;
  for (int k = 0; k < n; k++) {
    const s3g_density_tensor& t = tensors[k];
    const int moments = (t.src_exp_avg != nullptr) + (t.dst_exp_avg != nullptr) + (t.src_exp_avg_sq != nullptr) + (t.dst_exp_avg_sq != nullptr);
    if (t.width < 1 || !t.src || !t.dst || (moments != 0 && moments != 4)) {
      set_error("s3g_density_apply: tensor %d: width %d, NULL array, or moments given in part", k, t.width);
      return S3G_ERR_INVALID_ARG;
    }
    if (t.children_rewritten && t.dst != p.xyz_dst && t.dst != p.scaling_dst) {
      set_error("s3g_density_apply: tensor %d leaves its split children to the kernel but is neither xyz_dst nor scaling_dst", k);
      return S3G_ERR_INVALID_ARG;
    }
    a.t[k] = t;
  }
  hipLaunchKernelGGL(apply_kernel, dim3(density_blocks(p.P), n + 1), dim3(DB), 0, (hipStream_t)stream_, a);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" int s3g_density_reset_opacity(int P, const float* opacity, float* opacity_out, float* exp_avg, float* exp_avg_sq,
                                         void* stream_) {
  if (P < 0 || (P > 0 && (!opacity || !opacity_out))) {
    set_error("s3g_density_reset_opacity: bad argument");
    return S3G_ERR_INVALID_ARG;
  }
  if (P == 0) return S3G_OK;
  hipLaunchKernelGGL(reset_opacity_kernel, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream_, P, opacity, opacity_out, exp_avg,
                     exp_avg_sq);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}
