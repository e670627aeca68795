// Coloured depth frames for gfx950: the reference's depth_visualizer (utils/video_utils.py:27-33; visualize_depth / visualize_cmap /
// weighted_percentile, utils/visualization_tools.py:106-194) -- turbo map, -log curve, opacity weighting -- written as uint8 into one
// camera's tile of a strip, and the opacity-weighted 0.5 / 99.5 percentiles its automatic bounds come from, found by a radix selection
// over integer weight sums: no sort, no float atomics, no host read.  The arithmetic and the route: include/s3g_depthvis.h.
#include "common.hpp"

#include "../../include/s3g_depthvis.h"

// matplotlib's 256-entry turbo table through to8b: trunc(255 * clip(turbo[k][c], 0, 1)), [256][3]
#define DV_TURBO_BYTES \
    48, 18, 59, 49, 21, 66, 50, 24, 74, 52, 27, 81, 53, 30, 88, 54, 33, 95, 55, 35, 101, 56, 38, 108, \
    57, 41, 114, 58, 44, 121, 59, 47, 127, 60, 50, 133, 60, 53, 139, 61, 55, 145, 62, 58, 150, 63, 61, 156, \
    64, 64, 161, 64, 67, 166, 65, 69, 171, 65, 72, 176, 66, 75, 181, 67, 78, 186, 67, 80, 190, 67, 83, 194, \
    68, 86, 199, 68, 88, 203, 69, 91, 206, 69, 94, 210, 69, 96, 214, 69, 99, 217, 70, 102, 221, 70, 104, 224, \
    70, 107, 227, 70, 109, 230, 70, 112, 232, 70, 115, 235, 70, 117, 237, 70, 120, 240, 70, 122, 242, 70, 125, 244, \
    70, 127, 246, 70, 130, 248, 69, 132, 249, 69, 135, 251, 69, 137, 252, 68, 140, 253, 67, 142, 253, 66, 145, 254, \
    65, 147, 254, 64, 150, 254, 63, 152, 254, 62, 155, 254, 60, 157, 253, 59, 160, 252, 57, 162, 252, 56, 165, 251, \
    54, 168, 249, 52, 170, 248, 51, 172, 246, 49, 175, 245, 47, 177, 243, 45, 180, 241, 43, 182, 239, 42, 185, 237, \
    40, 187, 235, 38, 189, 233, 37, 192, 230, 35, 194, 228, 33, 196, 225, 32, 198, 223, 30, 201, 220, 29, 203, 218, \
    28, 205, 215, 27, 207, 212, 26, 209, 210, 25, 211, 207, 24, 213, 204, 24, 215, 202, 23, 217, 199, 23, 218, 196, \
    23, 220, 194, 23, 222, 191, 24, 224, 189, 24, 225, 186, 25, 227, 184, 26, 228, 182, 27, 229, 180, 29, 231, 177, \
    30, 232, 175, 32, 233, 172, 34, 235, 169, 36, 236, 166, 39, 237, 163, 41, 238, 160, 44, 239, 157, 47, 240, 154, \
    50, 241, 151, 53, 243, 148, 56, 244, 145, 59, 244, 141, 63, 245, 138, 66, 246, 135, 70, 247, 131, 74, 248, 128, \
    77, 249, 124, 81, 249, 121, 85, 250, 118, 89, 251, 114, 93, 251, 111, 97, 252, 108, 101, 252, 104, 105, 253, 101, \
    109, 253, 98, 113, 253, 95, 116, 254, 92, 120, 254, 89, 124, 254, 86, 128, 254, 83, 132, 254, 80, 135, 254, 77, \
    139, 254, 75, 142, 254, 72, 146, 254, 70, 149, 254, 68, 152, 254, 66, 155, 253, 64, 158, 253, 62, 161, 252, 61, \
    164, 252, 59, 166, 251, 58, 169, 251, 57, 172, 250, 55, 174, 249, 55, 177, 248, 54, 179, 248, 53, 182, 247, 53, \
    185, 245, 52, 187, 244, 52, 190, 243, 52, 192, 242, 51, 195, 241, 51, 197, 239, 51, 200, 238, 51, 202, 237, 51, \
    205, 235, 52, 207, 234, 52, 209, 232, 52, 212, 231, 53, 214, 229, 53, 216, 227, 53, 218, 226, 54, 221, 224, 54, \
    223, 222, 54, 225, 220, 55, 227, 218, 55, 229, 216, 56, 231, 215, 56, 232, 213, 56, 234, 211, 57, 236, 209, 57, \
    237, 207, 57, 239, 205, 57, 240, 203, 58, 242, 200, 58, 243, 198, 58, 244, 196, 58, 246, 194, 58, 247, 192, 57, \
    248, 190, 57, 249, 188, 57, 249, 186, 56, 250, 183, 55, 251, 181, 55, 251, 179, 54, 252, 176, 53, 252, 174, 52, \
    253, 171, 51, 253, 169, 50, 253, 166, 49, 253, 163, 48, 254, 161, 47, 254, 158, 46, 254, 155, 45, 254, 152, 44, \
    253, 149, 43, 253, 146, 41, 253, 143, 40, 253, 140, 39, 252, 137, 38, 252, 134, 36, 251, 131, 35, 251, 128, 34, \
    250, 125, 32, 250, 122, 31, 249, 119, 30, 248, 116, 28, 247, 113, 27, 247, 110, 26, 246, 107, 24, 245, 104, 23, \
    244, 101, 22, 243, 99, 21, 242, 96, 20, 241, 93, 19, 239, 90, 17, 238, 88, 16, 237, 85, 15, 236, 82, 14, \
    234, 80, 13, 233, 77, 13, 232, 75, 12, 230, 73, 11, 229, 70, 10, 227, 68, 10, 226, 66, 9, 224, 64, 8, \
    222, 62, 8, 221, 60, 7, 219, 58, 7, 217, 56, 6, 215, 54, 6, 214, 52, 5, 212, 50, 5, 210, 48, 5, \
    208, 47, 4, 206, 45, 4, 203, 43, 3, 201, 41, 3, 199, 40, 3, 197, 38, 2, 195, 36, 2, 192, 35, 2, \
    190, 33, 2, 187, 31, 1, 185, 30, 1, 182, 28, 1, 180, 27, 1, 177, 25, 1, 174, 24, 1, 172, 22, 1, \
    169, 21, 1, 166, 20, 1, 163, 18, 1, 160, 17, 1, 157, 16, 1, 154, 14, 1, 151, 13, 1, 148, 12, 1, \
    145, 11, 1, 142, 10, 1, 139, 9, 1, 135, 8, 1, 132, 7, 1, 129, 6, 2, 125, 5, 2, 122, 4, 2
namespace s3g {

typedef unsigned long long dv_u64;
typedef float dv_f32x4 __attribute__((ext_vector_type(4)));   // one 16-byte load

constexpr int DV_THREADS = 256;
constexpr int DV_BINS = 256;                     // 8 bits per pass, four passes; one histogram row per thread of a workgroup
constexpr int DV_PASSES = 4;
constexpr int DV_BLOCKS = 256;                   // partial histograms at most: one workgroup per CU
constexpr int DV_PIX_PER_BLOCK = DV_THREADS * 8;
constexpr int DV_FOLD_THREADS = 2 * DV_BINS;     // one thread per (target, digit)
constexpr int DV_COLOR_BLOCKS = 2048;
static_assert(DV_THREADS == DV_BINS, "a workgroup clears and stores its histogram one row per thread");
static_assert(DV_BLOCKS <= DV_THREADS, "the last fold reads one partial per thread");

static const unsigned char dv_table_host[768] = {DV_TURBO_BYTES};
__constant__ unsigned char dv_table[768] = {DV_TURBO_BYTES};

struct DvTarget {          // one percentile's selection state, on the device between the passes
  dv_u64 base;             // G: weight of every key below the prefix's range
  double q;                // p * (double(total) / 100.0)
  uint32_t prefix;         // the digits fixed so far, in place; the crossing key K after the last pass
  uint32_t none;           // total == 0: no key is crossed, the answer is the largest key
};
struct DvState {
  DvTarget t[2];
};
struct DvLast {            // one workgroup's findings of the last pass
  dv_u64 first[2];         // (lowest pixel index of group K) << 32 | its weight; ~0 if the workgroup saw none of K
  uint32_t pred[2];        // largest key below K; 0: none
  uint32_t maxkey;         // largest key; 0: no pixel took part
  uint32_t pad;
};

struct DvWorkspace {
  DvState* state;
  dv_u64* hist;            // [blocks][2][DV_BINS]
  DvLast* last;            // [blocks]
  size_t bytes;
};

static inline int dv_blocks(size_t pix) {
  const size_t nb = (pix + DV_PIX_PER_BLOCK - 1) / DV_PIX_PER_BLOCK;
  return nb < 1 ? 1 : (nb > (size_t)DV_BLOCKS ? DV_BLOCKS : (int)nb);
}

static inline DvWorkspace dv_carve(void* base, int blocks) {
  Carver c(base);
  DvWorkspace w;
  w.state = c.take<DvState>(1);
  w.hist = c.take<dv_u64>((size_t)blocks * 2 * DV_BINS);
  w.last = c.take<DvLast>((size_t)blocks);
  w.bytes = c.bytes();
  return w;
}

// The order-preserving key of a depth: 0 for a NaN (no other value maps to 0: -inf gives 0x007fffff), -0.0 as +0.0.
__device__ __forceinline__ uint32_t dv_key(float d) {
  if (d != d) return 0u;
  const uint32_t b = d == 0.0f ? 0u : __float_as_uint(d);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ double dv_value(uint32_t key) {
  return (double)__uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}
// llrint(min(max(a, 0), 1) * 2^30), NaN -> 0: the product is exact in fp32, the rounding is to nearest even
__device__ __forceinline__ dv_u64 dv_weight(float a) {
  const float c = a > 0.0f ? (a < 1.0f ? a : 1.0f) : 0.0f;
  return (dv_u64)__builtin_rintf(c * 1073741824.0f);
}

// One digit pass.  hist[t][digit] += w over the pixels whose key matches target t's prefix above the digit; pass 0 has no prefix,
// so both targets share one histogram.  Integer LDS atomics: the sums do not depend on the order of arrival.
__global__ void __launch_bounds__(DV_THREADS) depth_hist_kernel(const float* __restrict__ depth, const float* __restrict__ alpha,
                                                                uint32_t pix, int pass, const DvState* __restrict__ state,
                                                                dv_u64* __restrict__ partial) {
  __shared__ dv_u64 hist[2][DV_BINS];
  hist[0][threadIdx.x] = 0;
  hist[1][threadIdx.x] = 0;
  const uint32_t shift = 24u - 8u * (uint32_t)pass;
  const uint32_t p0 = pass > 0 ? state->t[0].prefix : 0u, p1 = pass > 0 ? state->t[1].prefix : 0u;
  __syncthreads();
  const uint32_t stride = gridDim.x * DV_THREADS;
  for (uint32_t i = blockIdx.x * DV_THREADS + threadIdx.x; i < pix; i += stride) {
    const uint32_t key = dv_key(depth[i]);
    if (key == 0u) continue;
    const dv_u64 w = dv_weight(alpha[i]);
    if (w == 0) continue;
    const uint32_t digit = (key >> shift) & (DV_BINS - 1);
    if (pass == 0) {
      atomicAdd(&hist[0][digit], w);
    } else {
      const uint32_t above = shift + 8u;       // 8, 16 or 24 here
      if (((key ^ p0) >> above) == 0u) atomicAdd(&hist[0][digit], w);
      if (((key ^ p1) >> above) == 0u) atomicAdd(&hist[1][digit], w);
    }
  }
  __syncthreads();
  dv_u64* out = partial + (size_t)blockIdx.x * 2 * DV_BINS;
  out[threadIdx.x] = hist[0][threadIdx.x];
  out[DV_BINS + threadIdx.x] = hist[pass == 0 ? 0 : 1][threadIdx.x];
}

// One workgroup: thread (t, d) sums digit d of target t over the partials, the workgroup scans the 256 sums of each target, and the
// one thread whose digit holds the crossing -- base + below <= q < base + below + own -- fixes it.  Pass 0 also sets q from the total.
__global__ void __launch_bounds__(DV_FOLD_THREADS) depth_fold_kernel(const dv_u64* __restrict__ partial, int blocks, int pass,
                                                                     DvState* __restrict__ state) {
  __shared__ dv_u64 scan[2][2][DV_BINS];
  const uint32_t t = threadIdx.x / DV_BINS, d = threadIdx.x % DV_BINS;
  const dv_u64* __restrict__ mine = partial + (size_t)t * DV_BINS + d;      // partial b lies 2 * DV_BINS further on
  dv_u64 s0 = 0, s1 = 0, s2 = 0, s3 = 0;                                    // four loads in flight; integer sums: any order
  int b = 0;
  for (; b + 4 <= blocks; b += 4) {
    s0 += mine[(size_t)(b + 0) * 2 * DV_BINS];
    s1 += mine[(size_t)(b + 1) * 2 * DV_BINS];
    s2 += mine[(size_t)(b + 2) * 2 * DV_BINS];
    s3 += mine[(size_t)(b + 3) * 2 * DV_BINS];
  }
  for (; b < blocks; ++b) s0 += mine[(size_t)b * 2 * DV_BINS];
  const dv_u64 sum = (s0 + s1) + (s2 + s3);
  dv_u64 base = 0;
  double q = 0.0;
  uint32_t prefix = 0;
  if (pass > 0) {
    base = state->t[t].base;
    q = state->t[t].q;
    prefix = state->t[t].prefix;
  }
  int cur = 0;
  scan[0][t][d] = sum;
  __syncthreads();
  for (uint32_t o = 1; o < DV_BINS; o <<= 1) {
    dv_u64 v = scan[cur][t][d];
    if (d >= o) v += scan[cur][t][d - o];
    scan[cur ^ 1][t][d] = v;
    __syncthreads();
    cur ^= 1;
  }
  const dv_u64 incl = scan[cur][t][d], excl = d > 0 ? scan[cur][t][d - 1] : 0, total = scan[cur][t][DV_BINS - 1];
  if (pass == 0) {
    q = (t == 0 ? 0.5 : 99.5) * ((double)total / 100.0);
    if (total == 0 && d == 0) {              // q >= S_last: nothing is crossed
      DvTarget none = {0, q, 0u, 1u};
      state->t[t] = none;
    }
  }
  if ((double)(base + excl) <= q && (double)(base + incl) > q) {        // exactly one d per target (none when total == 0)
    DvTarget next = {base + excl, q, prefix | (d << (24u - 8u * (uint32_t)pass)), 0u};
    if (pass == 0 || state->t[t].none == 0u) state->t[t] = next;
  }
}

// The last image-sized pass: what the interpolation needs around the crossing key K of each target.
__global__ void __launch_bounds__(DV_THREADS) depth_last_kernel(const float* __restrict__ depth, const float* __restrict__ alpha,
                                                                uint32_t pix, const DvState* __restrict__ state,
                                                                DvLast* __restrict__ partial) {
  __shared__ dv_u64 s_first[2];
  __shared__ uint32_t s_pred[2], s_max;
  if (threadIdx.x == 0) {
    s_first[0] = s_first[1] = ~(dv_u64)0;
    s_pred[0] = s_pred[1] = s_max = 0u;
  }
  const uint32_t K0 = state->t[0].none ? 0u : state->t[0].prefix, K1 = state->t[1].none ? 0u : state->t[1].prefix;
  __syncthreads();
  dv_u64 first0 = ~(dv_u64)0, first1 = ~(dv_u64)0;
  uint32_t pred0 = 0u, pred1 = 0u, mx = 0u;
  const uint32_t stride = gridDim.x * DV_THREADS;
  for (uint32_t i = blockIdx.x * DV_THREADS + threadIdx.x; i < pix; i += stride) {
    const uint32_t key = dv_key(depth[i]);
    if (key == 0u) continue;
    mx = key > mx ? key : mx;
    if (key < K0) pred0 = key > pred0 ? key : pred0;
    if (key < K1) pred1 = key > pred1 ? key : pred1;
    if (key == K0 || key == K1) {
      const dv_u64 rec = ((dv_u64)i << 32) | dv_weight(alpha[i]);
      if (key == K0) first0 = rec < first0 ? rec : first0;
      if (key == K1) first1 = rec < first1 ? rec : first1;
    }
  }
  atomicMin(&s_first[0], first0);
  atomicMin(&s_first[1], first1);
  atomicMax(&s_pred[0], pred0);
  atomicMax(&s_pred[1], pred1);
  atomicMax(&s_max, mx);
  __syncthreads();
  if (threadIdx.x == 0) {
    DvLast out = {{s_first[0], s_first[1]}, {s_pred[0], s_pred[1]}, s_max, 0u};
    partial[blockIdx.x] = out;
  }
}

// One workgroup folds the last pass's partials; thread 0 evaluates np.interp for both targets in double, in the stated order.
__global__ void __launch_bounds__(DV_THREADS) depth_interp_kernel(const DvLast* __restrict__ partial, int blocks,
                                                                  const DvState* __restrict__ state, double* __restrict__ bounds_out) {
  __shared__ dv_u64 s_first[2];
  __shared__ uint32_t s_pred[2], s_max;
  if (threadIdx.x == 0) {
    s_first[0] = s_first[1] = ~(dv_u64)0;
    s_pred[0] = s_pred[1] = s_max = 0u;
  }
  __syncthreads();
  if ((int)threadIdx.x < blocks) {
    const DvLast in = partial[threadIdx.x];
    atomicMin(&s_first[0], in.first[0]);
    atomicMin(&s_first[1], in.first[1]);
    atomicMax(&s_pred[0], in.pred[0]);
    atomicMax(&s_pred[1], in.pred[1]);
    atomicMax(&s_max, in.maxkey);
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int t = 0; t < 2; ++t) {
    const DvTarget st = state->t[t];
    double r;
    if (s_max == 0u) {
      r = __builtin_nan("");
    } else if (st.none) {
      r = dv_value(s_max);
    } else {
      const double xk = dv_value(st.prefix), g = (double)st.base, q = st.q;
      const dv_u64 w_first = s_first[t] & 0xffffffffull;
      r = xk;
      if (s_pred[t] != 0u && (double)(st.base + w_first) > q) {       // K's first pixel is the crossing one: j is the predecessor
        const double xp = dv_value(s_pred[t]);
        r = q == g ? xp : ((xk - xp) / (double)w_first) * (q - g) + xp;
      }
    }
    bounds_out[t] = r;
  }
}

struct DvColorArgs {
  const float* depth;
  const float* alpha;      // or NULL
  const double* bounds;    // or NULL
  uint8_t* dst;            // the tile's first byte in row 0
  long long row_bytes;
  double lo, hi;           // NaN: from bounds
  uint32_t H, W;
  uint32_t packed;
};

// One pixel: the packed (r | g << 8 | b << 16) table entry, 0 for a NaN u.
__device__ __forceinline__ uint32_t dv_color(float d, float a, bool weighted, double mn, double den, const uint32_t* lut) {
  const double v = -log((double)d + 1e-6);
  double t = (v - mn) / den;
  t = t > 0.0 ? (t < 1.0 ? t : 1.0) : 0.0;       // np.clip(., 0, 1), then NaN -> 0
  const double u = weighted ? t * (double)a : t;
  const double x = u * 256.0;
  if (x != x) return 0u;
  return lut[x >= 256.0 ? 255 : (x > 0.0 ? (int)x : 0)];
}

__global__ void __launch_bounds__(DV_THREADS) depth_color_kernel(DvColorArgs args) {
  __shared__ uint32_t lut[DV_BINS];
  lut[threadIdx.x] = (uint32_t)dv_table[3 * threadIdx.x] | (uint32_t)dv_table[3 * threadIdx.x + 1] << 8 |
                     (uint32_t)dv_table[3 * threadIdx.x + 2] << 16;
  const double eps = 1.1920928955078125e-07;      // 2^-23
  const double lo = args.lo != args.lo ? args.bounds[0] - eps : args.lo;
  const double hi = args.hi != args.hi ? args.bounds[1] + eps : args.hi;
  const double c_lo = -log(lo + 1e-6), c_hi = -log(hi + 1e-6);
  const double mn = c_hi < c_lo ? c_hi : c_lo, den = fabs(c_hi - c_lo);     // a NaN bound makes den NaN: t = 0 everywhere
  __syncthreads();
  const float* __restrict__ depth = args.depth;
  const float* __restrict__ alpha = args.alpha;
  const bool weighted = alpha != nullptr;
  const uint32_t H = args.H, W = args.W;
  const uint32_t first = blockIdx.x * DV_THREADS + threadIdx.x, stride = gridDim.x * DV_THREADS;
  if (args.packed) {       // W % 4 == 0: a quad never straddles rows
    const uint32_t wq = W / 4, quads = H * wq;
    for (uint32_t k = first; k < quads; k += stride) {
      const uint32_t row = k / wq, x = (k - row * wq) * 4;
      const size_t at = (size_t)row * W + x;
      const dv_f32x4 d = *reinterpret_cast<const dv_f32x4*>(depth + at);
      dv_f32x4 a = {1.0f, 1.0f, 1.0f, 1.0f};
      if (weighted) a = *reinterpret_cast<const dv_f32x4*>(alpha + at);
      const uint32_t c0 = dv_color(d.x, a.x, weighted, mn, den, lut), c1 = dv_color(d.y, a.y, weighted, mn, den, lut),
                     c2 = dv_color(d.z, a.z, weighted, mn, den, lut), c3 = dv_color(d.w, a.w, weighted, mn, den, lut);
      uint32_t* out = reinterpret_cast<uint32_t*>(args.dst + (size_t)row * args.row_bytes + (size_t)x * 3);
      out[0] = c0 | c1 << 24;
      out[1] = c1 >> 8 | c2 << 16;
      out[2] = c2 >> 16 | c3 << 8;
    }
  } else {
    const uint32_t pixels = H * W;
    for (uint32_t p = first; p < pixels; p += stride) {
      const uint32_t row = p / W, x = p - row * W;
      const uint32_t c = dv_color(depth[p], weighted ? alpha[p] : 1.0f, weighted, mn, den, lut);
      uint8_t* out = args.dst + (size_t)row * args.row_bytes + (size_t)x * 3;
      out[0] = (uint8_t)c;
      out[1] = (uint8_t)(c >> 8);
      out[2] = (uint8_t)(c >> 16);
    }
  }
}

}  // namespace s3g

using namespace s3g;

extern "C" const unsigned char* s3g_depth_turbo_table(void) { return dv_table_host; }

extern "C" size_t s3g_depthvis_workspace_bytes(int H, int W) {
  if (H < 1 || W < 1 || (size_t)H * (size_t)W > (size_t)S3G_DEPTHVIS_MAX_PIXELS) return 0;
  return dv_carve(nullptr, dv_blocks((size_t)H * (size_t)W)).bytes;
}

extern "C" int s3g_depth_percentiles(int H, int W, const float* depth, const float* alpha, double* bounds_out, void* workspace,
                                     void* stream_) {
  if (H < 1 || W < 1 || (size_t)H * (size_t)W > (size_t)S3G_DEPTHVIS_MAX_PIXELS) {
    set_error("s3g_depth_percentiles: H = %d, W = %d (H * W in 1..2^23: the weight sums stay exact in a double up to there)", H, W);
    return S3G_ERR_INVALID_ARG;
  }
  if (!depth || !alpha || !bounds_out || !workspace) {
    set_error("s3g_depth_percentiles: NULL depth, alpha, bounds_out or workspace");
    return S3G_ERR_INVALID_ARG;
  }
  if (reinterpret_cast<uintptr_t>(workspace) & 7 || reinterpret_cast<uintptr_t>(bounds_out) & 7) {
    set_error("s3g_depth_percentiles: workspace and bounds_out must be 8-byte aligned");
    return S3G_ERR_INVALID_ARG;
  }
  const hipStream_t stream = (hipStream_t)stream_;
  const uint32_t pix = (uint32_t)H * (uint32_t)W;
  const int blocks = dv_blocks(pix);
  const DvWorkspace w = dv_carve(workspace, blocks);
  for (int pass = 0; pass < DV_PASSES; ++pass) {
    hipLaunchKernelGGL(depth_hist_kernel, dim3(blocks), dim3(DV_THREADS), 0, stream, depth, alpha, pix, pass, w.state, w.hist);
    S3G_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(depth_fold_kernel, dim3(1), dim3(DV_FOLD_THREADS), 0, stream, w.hist, blocks, pass, w.state);
    S3G_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(depth_last_kernel, dim3(blocks), dim3(DV_THREADS), 0, stream, depth, alpha, pix, w.state, w.last);
  S3G_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(depth_interp_kernel, dim3(1), dim3(DV_THREADS), 0, stream, w.last, blocks, w.state, bounds_out);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}

extern "C" int s3g_depth_colors(int H, int W, const float* depth, const float* alpha, double lo, double hi, const double* bounds,
                                unsigned char* dst, long long dst_row_bytes, int dst_col, void* stream_) {
  if (H < 1 || W < 1 || (size_t)H * (size_t)W > ((size_t)1 << 30)) {
    set_error("s3g_depth_colors: H = %d, W = %d", H, W);
    return S3G_ERR_INVALID_ARG;
  }
  if (!depth || !dst) {
    set_error("s3g_depth_colors: NULL depth or dst");
    return S3G_ERR_INVALID_ARG;
  }
  const bool automatic = lo != lo || hi != hi;
  if (automatic && !bounds) {
    set_error("s3g_depth_colors: a NaN bound asks for the automatic one, and bounds is NULL");
    return S3G_ERR_INVALID_ARG;
  }
  if (automatic && !alpha) {
    set_error("s3g_depth_colors: the automatic bounds are opacity-weighted percentiles: alpha may be NULL only when lo and hi are given");
    return S3G_ERR_INVALID_ARG;
  }
  if (dst_col < 0 || ((long long)dst_col + W) * 3 > dst_row_bytes) {
    set_error("s3g_depth_colors: columns [%d, %lld) x 3 channels do not fit a row of %lld bytes", dst_col, (long long)dst_col + W,
              dst_row_bytes);
    return S3G_ERR_INVALID_ARG;
  }
  DvColorArgs args;
  args.depth = depth;
  args.alpha = alpha;
  args.bounds = bounds;
  args.dst = dst + (size_t)dst_col * 3;
  args.row_bytes = dst_row_bytes;
  args.lo = lo;
  args.hi = hi;
  args.H = (uint32_t)H;
  args.W = (uint32_t)W;
  const bool src16 = (reinterpret_cast<uintptr_t>(depth) & 15) == 0 && (reinterpret_cast<uintptr_t>(alpha) & 15) == 0;
  args.packed = src16 && W % 4 == 0 && (reinterpret_cast<uintptr_t>(args.dst) & 3) == 0 && dst_row_bytes % 4 == 0;
  const size_t pix = (size_t)H * (size_t)W;
  const size_t items = args.packed ? pix / 4 : pix;
  const size_t want = (items + DV_THREADS - 1) / DV_THREADS;
  const int grid = want > (size_t)DV_COLOR_BLOCKS ? DV_COLOR_BLOCKS : (want < 1 ? 1 : (int)want);
  hipLaunchKernelGGL(depth_color_kernel, dim3(grid), dim3(DV_THREADS), 0, (hipStream_t)stream_, args);
  S3G_HIP_CHECK(hipGetLastError());
  return S3G_OK;
}
