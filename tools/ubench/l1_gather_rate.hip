// At what rate does a CU's vector-memory path deliver the access shape of the HexPlane per-point kernels when the data is
// cache-resident?  hexplane_forward_kernel / hexplane_backward_pointdiv_kernel gather 128-byte texels with 8 lanes x 16 B: one
// wave-instruction = 8 different lines = 1 KB.  DESIGN.md 4.2 priced the forward with "64 B/clk/CU", a figure nobody had measured.
//
// Every lane issues independent 16-byte loads (address = an LCG of the point index, never of loaded data; 8 loads in flight per
// unrolled body, the values only summed), 16 or 32 waves per CU, from a table of
//   16 KB     L1-resident (the vector L1 is 32 KB)
//   256 KB    the size class of the four levels' uniform-time row tables (360 KB): L2 hits with some L1 reuse
//   8 MB      more than one XCD's 4 MB L2
// in two address shapes:
//   gather    the 8 points of a wave read 8 RANDOM lines            (the texel / row-table gathers)
//   coalesced the 8 points of a wave read 8 CONSECUTIVE lines       (1 KB contiguous per wave-instruction)
// Reported: time, wave-instructions per second, bytes per second, and bytes per clock and CU at the device's nominal clock
// (hipDeviceAttributeClockRate; the sustained clock under load is lower, so the per-clock figure is a lower bound).
//
// build + run (GPU box):  hipcc --offload-arch=gfx950 -O2 tools/ubench/l1_gather_rate.hip -o tools/ubench/l1_gather_rate && tools/ubench/l1_gather_rate
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

constexpr int LOADS = 8;   // per unrolled body

template <bool COALESCED>
__global__ void __launch_bounds__(1024) gather_rate(const float4* __restrict__ tab, uint32_t line_mask, int iters, float* __restrict__ sink) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t piece = t & 7u, point = (t >> 3) & 7u;
  uint32_t state = (COALESCED ? (t >> 6) : (t >> 3)) * 0x9E3779B1u + 12345u;   // per wave / per point
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int it = 0; it < iters; it++) {
#pragma unroll
    for (int k = 0; k < LOADS; k++) {
      state = state * 1664525u + 1013904223u;
      const uint32_t line = ((state >> 8) + (COALESCED ? point : 0u)) & line_mask;   // always inside the table
      const float4 v = tab[(size_t)line * 8u + piece];
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
  }
  if (acc.x + acc.y + acc.z + acc.w == 12345.678f) sink[0] = 1.0f;
}

int main() {
  int dev = 0, cus = 0, khz = 0;
  CHECK(hipGetDevice(&dev));
  CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, dev));
  const size_t MAXB = 8u << 20;
  void* buf;
  float* sink;
  CHECK(hipMalloc(&buf, MAXB));
  CHECK(hipMalloc(&sink, 4));
  CHECK(hipMemset(buf, 0, MAXB));
  hipEvent_t a, b;
  CHECK(hipEventCreate(&a));
  CHECK(hipEventCreate(&b));
  printf("CUs %d, nominal clock %.0f MHz\n", cus, khz / 1e3);
  const int iters = 1000;
  const struct { const char* name; uint32_t lines; } tables[] = {{"16 KB", 128}, {"256 KB", 2048}, {"8 MB", 65536}};   // powers of two (mask); 256 KB stands for the 360 KB of row tables
  for (int wg = 1; wg <= 2; wg++)
    for (const auto& tb : tables)
      for (int shape = 0; shape < 2; shape++) {
        float best = 1e30f;
        for (int rep = 0; rep < 3; rep++) {
          CHECK(hipEventRecord(a));
          if (shape == 0) hipLaunchKernelGGL(gather_rate<false>, dim3(cus * wg), dim3(1024), 0, 0, (const float4*)buf, tb.lines - 1, iters, sink);
          else hipLaunchKernelGGL(gather_rate<true>, dim3(cus * wg), dim3(1024), 0, 0, (const float4*)buf, tb.lines - 1, iters, sink);
          CHECK(hipGetLastError());
          CHECK(hipEventRecord(b));
          CHECK(hipEventSynchronize(b));
          float ms;
          CHECK(hipEventElapsedTime(&ms, a, b));
          if (ms < best) best = ms;
        }
        const double winst = (double)cus * wg * 16 * iters * LOADS, bytes = winst * 1024.0;
        printf("%2d waves/CU  table %-6s  %-9s  %8.3f ms  %6.2f G wave-instr/s  %6.1f TB/s  %6.1f B/clk/CU\n", 16 * wg, tb.name,
               shape == 0 ? "gather" : "coalesced", best, winst / best / 1e6, bytes / best / 1e9, bytes / (best * 1e-3) / cus / (khz * 1e3));
      }
  CHECK(hipDeviceSynchronize());
  return 0;
}
