// Shared helpers for the gfx950 kernels of libs3g.so (private; not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <atomic>

#include "../../include/s3g_raster.h"

namespace s3g {

// hipFuncSetAttribute is per DEVICE: a process that drives several GPUs (one Python process, two `cuda:k` tensors) must
// raise the dynamic-LDS limit on each of them.  Protocol: `if (device_needs_setup(seen)) { ...S3G_HIP_CHECK(set attrs)...;
// device_setup_done(seen); }` -- the bit is set only AFTER every attribute call succeeded (a failed attempt is retried by the
// next call instead of leaving the limit low for good), two host threads racing here both set the (idempotent) attributes
// before either launches, and device ids >= 64 simply repeat the cheap attribute calls every time instead of aliasing.
inline bool device_needs_setup(const std::atomic<uint64_t>& seen) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  return dev >= 64 || (seen.load(std::memory_order_acquire) & (1ull << dev)) == 0;
}
inline void device_setup_done(std::atomic<uint64_t>& seen) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 64) seen.fetch_or(1ull << dev, std::memory_order_release);
}

constexpr int WAVE = 64;

// ---- error plumbing ------------------------------------------------------------------------------------
void set_error(const char* fmt, ...);
void clear_error();
#define S3G_HIP_CHECK(expr)                                                                     \
  do {                                                                                          \
    hipError_t _e = (expr);                                                                     \
    if (_e != hipSuccess) {                                                                     \
      s3g::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return S3G_ERR_HIP;                                                                       \
    }                                                                                           \
  } while (0)
// After a kernel launch: always catch launch errors; in debug also synchronise (reference CHECK_CUDA, auxiliary.h:166-173).
#define S3G_KERNEL_CHECK(stream, debug)                          \
  do {                                                           \
    S3G_HIP_CHECK(hipGetLastError());                            \
    if (debug) S3G_HIP_CHECK(hipStreamSynchronize(stream));      \
  } while (0)

// ---- optional in-library kernel timing (bench.py's roofline leg): hipEvent pairs on the launch stream ----------
// id 0 = blend_forward_kernel, id 1 = blend_backward_kernel
void profile_begin(int id, hipStream_t stream);
void profile_end(int id, hipStream_t stream, double instances, double pixels);

// ---- arena carving (128-byte aligned sub-arrays, like the reference's obtain<>(), rasterizer_impl.h) ----
struct Carver {
  char* base;
  size_t off;
  explicit Carver(void* p) : base(reinterpret_cast<char*>(p)), off(0) {}
  template <typename T>
  T* take(size_t count) {
    off = (off + 127) & ~size_t(127);
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += count * sizeof(T);
    return p;
  }
  size_t bytes() const { return (off + 127) & ~size_t(127); }
};

// ---- small device helpers -------------------------------------------------------------------------------
// Row-vector 4x4 matrices are indexed column-major like the reference (auxiliary.h:58-77).
__device__ __forceinline__ float3 xform_4x3(const float3 p, const float* __restrict__ M) {
  return make_float3(M[0] * p.x + M[4] * p.y + M[8] * p.z + M[12], M[1] * p.x + M[5] * p.y + M[9] * p.z + M[13],
                     M[2] * p.x + M[6] * p.y + M[10] * p.z + M[14]);
}
__device__ __forceinline__ float4 xform_4x4(const float3 p, const float* __restrict__ M) {
  return make_float4(M[0] * p.x + M[4] * p.y + M[8] * p.z + M[12], M[1] * p.x + M[5] * p.y + M[9] * p.z + M[13],
                     M[2] * p.x + M[6] * p.y + M[10] * p.z + M[14], M[3] * p.x + M[7] * p.y + M[11] * p.z + M[15]);
}

// The lanes of ONE wave hand data to each other through LDS: earlier LDS writes of the wave are visible to its later reads.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// XCD-aware tile order: hardware places workgroup b on XCD (b % 8); give each XCD a contiguous band of
// tiles so neighbouring tiles (which share most of their Gaussians) hit the same 4 MiB L2.
__device__ __forceinline__ uint32_t xcd_swizzle(uint32_t bid, uint32_t nblocks) {
  constexpr uint32_t XCDS = 8;
  const uint32_t per = (nblocks + XCDS - 1) / XCDS;
  const uint32_t t = (bid % XCDS) * per + bid / XCDS;
  return t;  // may be >= nblocks for the tail: caller must bounds-check
}

}  // namespace s3g
