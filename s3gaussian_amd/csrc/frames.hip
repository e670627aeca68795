// Evaluation video frames for gfx950: the uint8 strips of the reference's save_seperate_videos (utils/video_utils.py:439-499),
// to8b (utils/visualization_tools.py:68-71) and the per-image depth normalisation (utils/video_utils.py:196-198), written from the
// [C,H,W] fp32 renders of one camera into that camera's columns of the [H, num_cams * W, C] strips.
// Two launches at most, no atomics: a maximum reduction over the normalised jobs' images that leaves one partial per workgroup,
// and a conversion pass that folds the partials in its prologue.  The contract and the path rule: include/s3g_frames.h.
#include "common.hpp"

#include "../../include/s3g_frames.h"

namespace s3g {

constexpr int FRAME_THREADS = 256;
constexpr int FRAME_PARTS = 256;                              // partial maxima per job at most: one per thread of the fold
constexpr int FRAME_MAX_PER_BLOCK = FRAME_THREADS * 4 * 4;    // floats one reduction workgroup is sized for: four 16-byte loads per lane
constexpr int FRAME_TILE_BLOCKS = 2048;                       // 256 CUs x 8 workgroups per job row of the grid, the rest by grid stride
typedef float frame_f32x4 __attribute__((ext_vector_type(4)));   // one 16-byte load (a float4 struct copy may be split into pieces)
constexpr uint32_t FRAME_NORMALIZE = 1, FRAME_PACKED = 2, FRAME_SRC_ALIGNED = 4;

struct FrameJob {
  const float* src;
  uint8_t* dst;           // dst + dst_col * channels of the ABI's job: the tile's first byte in row 0
  long long row_bytes;
  uint32_t channels;
  uint32_t flags;
};
struct FrameTable {       // travels by value in the kernel arguments (8 x 32 bytes)
  FrameJob job[S3G_FRAME_MAX_JOBS];
};

static inline int frame_parts(int H, int W) {
  const size_t n = 3 * (size_t)H * (size_t)W;
  const size_t nb = (n + FRAME_MAX_PER_BLOCK - 1) / FRAME_MAX_PER_BLOCK;
  return nb < 1 ? 1 : (nb > (size_t)FRAME_PARTS ? FRAME_PARTS : (int)nb);
}

// numpy's max(): the larger operand, and NaN once either is NaN.  Commutative and associative up to the NaN's payload.
__device__ __forceinline__ float nan_max(float a, float b) { return (b > a || b != b) ? b : a; }

// the maximum over the workgroup, valid in every thread: xor butterfly inside a wave, then the four waves through LDS
__device__ __forceinline__ float block_nan_max(float mx, float* red) {
  for (int o = 32; o > 0; o >>= 1) mx = nan_max(mx, __shfl_xor(mx, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  return nan_max(nan_max(red[0], red[1]), nan_max(red[2], red[3]));
}

// Pass 1.  blockIdx.y = job; workgroups of a job without `normalize` leave at once.  n = channels * pix floats: 16-byte loads where
// src is 16-byte aligned (the first n / 4 float4, the last n % 4 floats through the scalar tail), scalar loads otherwise.
__global__ void __launch_bounds__(FRAME_THREADS) frame_max_kernel(FrameTable table, uint32_t pix, float* __restrict__ partial) {
  __shared__ float red[4];
  const FrameJob& jb = table.job[blockIdx.y];
  if (!(jb.flags & FRAME_NORMALIZE)) return;
  const float* __restrict__ src = jb.src;
  const size_t n = (size_t)jb.channels * pix;
  const size_t tid = (size_t)blockIdx.x * FRAME_THREADS + threadIdx.x, stride = (size_t)gridDim.x * FRAME_THREADS;
  float mx = -__builtin_inff();
  size_t done = 0;
  if (jb.flags & FRAME_SRC_ALIGNED) {
    const size_t n4 = n / 4;
    const float4* __restrict__ s4 = reinterpret_cast<const float4*>(src);
    for (size_t i = tid; i < n4; i += stride) {
      const float4 v = s4[i];
      mx = nan_max(nan_max(mx, v.x), nan_max(nan_max(v.y, v.z), v.w));
    }
    done = n4 * 4;
  }
  for (size_t i = done + tid; i < n; i += stride) mx = nan_max(mx, src[i]);
  mx = block_nan_max(mx, red);
  if (threadIdx.x == 0) partial[(size_t)blockIdx.y * FRAME_PARTS + blockIdx.x] = mx;
}

// to8b of one value: np.clip(q, 0, 1) with NaN -> 0, one fp32 multiply, truncation (the library is built with -ffp-contract=off)
__device__ __forceinline__ uint32_t frame_byte(float x, float m, bool normalize) {
  const float q = normalize ? x / m : x;       // the correctly rounded division, not a reciprocal
  const float c = q > 0.0f ? q : 0.0f;
  return (uint32_t)(int)(255.0f * fminf(c, 1.0f));
}

// Pass 2.  blockIdx.y = job.  Packed: one lane takes 4 consecutive pixels of a row (W % 4 == 0: a quad never straddles rows).
__global__ void __launch_bounds__(FRAME_THREADS) frame_tile_kernel(FrameTable table, uint32_t H, uint32_t W, int nparts,
                                                                   const float* __restrict__ partial, float* __restrict__ maxima) {
  __shared__ float red[4];
  const FrameJob& jb = table.job[blockIdx.y];
  const bool normalize = (jb.flags & FRAME_NORMALIZE) != 0;
  float m = 1.0f;
  if (normalize) {       // uniform over the workgroup
    m = block_nan_max((int)threadIdx.x < nparts ? partial[(size_t)blockIdx.y * FRAME_PARTS + threadIdx.x] : -__builtin_inff(), red);
    if (maxima != nullptr && blockIdx.x == 0 && threadIdx.x == 0) maxima[blockIdx.y] = m;
  }
  const bool blank = normalize && !(m > 0.0f);      // maximum <= 0 or NaN: an all-zero tile
  const float* __restrict__ src = jb.src;
  uint8_t* __restrict__ dst = jb.dst;
  const size_t plane = (size_t)H * W;
  const uint32_t C = jb.channels;
  const uint32_t first = blockIdx.x * FRAME_THREADS + threadIdx.x, stride = gridDim.x * FRAME_THREADS;
  if (jb.flags & FRAME_PACKED) {
    const uint32_t wq = W / 4, quads = H * wq;
    for (uint32_t q = first; q < quads; q += stride) {
      const uint32_t row = q / wq, x = (q - row * wq) * 4;
      const size_t at = (size_t)row * W + x;
      uint32_t* out = reinterpret_cast<uint32_t*>(dst + (size_t)row * jb.row_bytes + (size_t)x * C);
      const frame_f32x4 r = *reinterpret_cast<const frame_f32x4*>(src + at);
      if (C == 1) {
        out[0] = blank ? 0u : (frame_byte(r.x, m, normalize) | frame_byte(r.y, m, normalize) << 8 |
                               frame_byte(r.z, m, normalize) << 16 | frame_byte(r.w, m, normalize) << 24);
      } else {
        const frame_f32x4 g = *reinterpret_cast<const frame_f32x4*>(src + plane + at);
        const frame_f32x4 b = *reinterpret_cast<const frame_f32x4*>(src + 2 * plane + at);
        const uint32_t r0 = frame_byte(r.x, m, normalize), r1 = frame_byte(r.y, m, normalize), r2 = frame_byte(r.z, m, normalize),
                       r3 = frame_byte(r.w, m, normalize);
        const uint32_t g0 = frame_byte(g.x, m, normalize), g1 = frame_byte(g.y, m, normalize), g2 = frame_byte(g.z, m, normalize),
                       g3 = frame_byte(g.w, m, normalize);
        const uint32_t b0 = frame_byte(b.x, m, normalize), b1 = frame_byte(b.y, m, normalize), b2 = frame_byte(b.z, m, normalize),
                       b3 = frame_byte(b.w, m, normalize);
        out[0] = blank ? 0u : (r0 | g0 << 8 | b0 << 16 | r1 << 24);
        out[1] = blank ? 0u : (g1 | b1 << 8 | r2 << 16 | g2 << 24);
        out[2] = blank ? 0u : (b2 | r3 << 8 | g3 << 16 | b3 << 24);
      }
    }
  } else {
    const uint32_t pixels = H * W;
    for (uint32_t p = first; p < pixels; p += stride) {
      const uint32_t row = p / W, x = p - row * W;
      uint8_t* out = dst + (size_t)row * jb.row_bytes + (size_t)x * C;
      for (uint32_t c = 0; c < C; ++c) out[c] = blank ? (uint8_t)0 : (uint8_t)frame_byte(src[c * plane + p], m, normalize);
    }
  }
}

}  // namespace s3g

using namespace s3g;

extern "C" size_t s3g_frame_workspace_bytes(int H, int W, int jobs) {
  if (H < 1 || W < 1 || jobs < 1) return 0;
  return ((size_t)jobs * FRAME_PARTS * sizeof(float) + 127) & ~size_t(127);
}

extern "C" int s3g_frame_tiles(int H, int W, int jobs, const s3g_frame_job* job, float* maxima, void* workspace, void* stream_) {
  if (jobs < 1 || jobs > S3G_FRAME_MAX_JOBS) {
    set_error("s3g_frame_tiles: jobs = %d (1..%d)", jobs, S3G_FRAME_MAX_JOBS);
    return S3G_ERR_INVALID_ARG;
  }
  if (H < 1 || W < 1 || (size_t)H * (size_t)W > ((size_t)1 << 30)) {
    set_error("s3g_frame_tiles: H = %d, W = %d", H, W);
    return S3G_ERR_INVALID_ARG;
  }
  if (!job) {
    set_error("s3g_frame_tiles: NULL job table");
    return S3G_ERR_INVALID_ARG;
  }
  FrameTable table;
  memset(&table, 0, sizeof(table));
  bool any_normalize = false, any_bytes = false;
  for (int j = 0; j < jobs; ++j) {
    const s3g_frame_job& in = job[j];
    if (!in.src || !in.dst) {
      set_error("s3g_frame_tiles: job %d has a NULL src or dst", j);
      return S3G_ERR_INVALID_ARG;
    }
    if (in.channels != 1 && in.channels != 3) {
      set_error("s3g_frame_tiles: job %d has channels = %d (1 or 3)", j, in.channels);
      return S3G_ERR_INVALID_ARG;
    }
    if (in.dst_col < 0 || ((long long)in.dst_col + W) * in.channels > in.dst_row_bytes) {
      set_error("s3g_frame_tiles: job %d: columns [%d, %lld) x %d channels do not fit a row of %lld bytes", j, in.dst_col,
                (long long)in.dst_col + W, in.channels, in.dst_row_bytes);
      return S3G_ERR_INVALID_ARG;
    }
    FrameJob& out = table.job[j];
    out.src = in.src;
    out.dst = in.dst + (size_t)in.dst_col * in.channels;
    out.row_bytes = in.dst_row_bytes;
    out.channels = (uint32_t)in.channels;
    const bool src16 = (reinterpret_cast<uintptr_t>(in.src) & 15) == 0;
    const bool packed = src16 && W % 4 == 0 && (reinterpret_cast<uintptr_t>(out.dst) & 3) == 0 && in.dst_row_bytes % 4 == 0;
    out.flags = (in.normalize ? FRAME_NORMALIZE : 0) | (packed ? FRAME_PACKED : 0) | (src16 ? FRAME_SRC_ALIGNED : 0);
    any_normalize |= in.normalize != 0;
    any_bytes |= !packed;
  }
  if (any_normalize && !workspace) {
    set_error("s3g_frame_tiles: NULL workspace with a normalised job");
    return S3G_ERR_INVALID_ARG;
  }
  const hipStream_t stream = (hipStream_t)stream_;
  const int nparts = frame_parts(H, W);
  float* partial = reinterpret_cast<float*>(workspace);
  const uint32_t pix = (uint32_t)H * (uint32_t)W;
  if (any_normalize) {
    hipLaunchKernelGGL(frame_max_kernel, dim3(nparts, jobs), dim3(FRAME_THREADS), 0, stream, table, pix, partial);
    S3G_HIP_CHECK(hipGetLastError());
  }
  const size_t items = any_bytes ? (size_t)pix : (size_t)pix / 4;
  const size_t want = (items + FRAME_THREADS - 1) / FRAME_THREADS;
  const int grid = want > (size_t)FRAME_TILE_BLOCKS ? FRAME_TILE_BLOCKS : (want < 1 ? 1 : (int)want);
  hipLaunchKernelGGL(frame_tile_kernel, dim3(grid, jobs), dim3(FRAME_THREADS), 0, stream, table, (uint32_t)H, (uint32_t)W, nparts,
                     partial, maxima);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}
