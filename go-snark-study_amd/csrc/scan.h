// Exclusive prefix sums of u32 counters on the device: the scan between the count and the scatter of an index build (capi_zkey.hip:
// section 4 of a .zkey by row; zkey_setup.hip: the terms of an R1CS by signal).  Three kernels: tiles, the tile totals, the fix-up.
#pragma once
#include "runtime.h"

namespace gs {

constexpr uint32_t kScanPerThread = 8, kScanTile = 256 * kScanPerThread;

// x[0..n) -> its exclusive prefix sums inside every tile of kScanTile, tile_sum[t] = the tile's total
static __global__ void __launch_bounds__(256) k_scan_tiles(uint32_t* __restrict__ x, uint32_t n, uint32_t* __restrict__ tile_sum) {
  __shared__ uint32_t sh[256];
  const size_t base = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kScanPerThread;
  uint32_t v[kScanPerThread], sum = 0;
#pragma unroll
  for (uint32_t j = 0; j < kScanPerThread; ++j) { v[j] = base + j < n ? x[base + j] : 0u; sum += v[j]; }
  sh[threadIdx.x] = sum;
  __syncthreads();
  uint32_t incl = sum;
  for (uint32_t off = 1; off < 256; off <<= 1) {
    const uint32_t o = threadIdx.x >= off ? sh[threadIdx.x - off] : 0u;
    __syncthreads();
    incl += o;
    sh[threadIdx.x] = incl;
    __syncthreads();
  }
  uint32_t run = incl - sum;
#pragma unroll
  for (uint32_t j = 0; j < kScanPerThread; ++j) {
    if (base + j < n) x[base + j] = run;
    run += v[j];
  }
  if (threadIdx.x == 255) tile_sum[blockIdx.x] = incl;
}
// exclusive prefix sums of the tile totals, in place (one workgroup)
static __global__ void __launch_bounds__(1024) k_scan_tile_sums(uint32_t* __restrict__ tile_sum, uint32_t ntiles) {
  __shared__ uint32_t sh[1024];
  const uint32_t per = (ntiles + 1023u) / 1024u, b0 = threadIdx.x * per;
  uint32_t sum = 0;
  for (uint32_t j = 0; j < per; ++j) if (b0 + j < ntiles) sum += tile_sum[b0 + j];
  sh[threadIdx.x] = sum;
  __syncthreads();
  uint32_t incl = sum;
  for (uint32_t off = 1; off < 1024; off <<= 1) {
    const uint32_t o = threadIdx.x >= off ? sh[threadIdx.x - off] : 0u;
    __syncthreads();
    incl += o;
    sh[threadIdx.x] = incl;
    __syncthreads();
  }
  uint32_t run = incl - sum;
  for (uint32_t j = 0; j < per; ++j)
    if (b0 + j < ntiles) {
      const uint32_t t = tile_sum[b0 + j];
      tile_sum[b0 + j] = run;
      run += t;
    }
}
static __global__ void __launch_bounds__(256) k_scan_add(uint32_t* __restrict__ x, uint32_t n, const uint32_t* __restrict__ tile_prefix) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] += tile_prefix[i / kScanTile];
}
inline uint32_t scan_tiles(size_t n) { return (uint32_t)((n + kScanTile - 1) / kScanTile); }
// x[0..n) -> its exclusive prefix sums, in place, on the context's stream; tile_sum: scan_tiles(n) words of scratch
inline void scan_exclusive_dev(Ctx& c, uint32_t* x, size_t n, uint32_t* tile_sum) {
  const uint32_t ntiles = scan_tiles(n);
  hipLaunchKernelGGL(k_scan_tiles, dim3(ntiles), dim3(256), 0, c.stream, x, (uint32_t)n, tile_sum);
  hipLaunchKernelGGL(k_scan_tile_sums, dim3(1), dim3(1024), 0, c.stream, tile_sum, ntiles);
  hipLaunchKernelGGL(k_scan_add, grid1(n), dim3(256), 0, c.stream, x, (uint32_t)n, tile_sum);
  GS_HIP(hipGetLastError());
}

}  // namespace gs
