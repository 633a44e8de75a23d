// The workgroup pieces of the multi-launch exclusive scan (block totals, scan of the totals, add) that isosurface.hip and
// occupancy.hip share: 256 threads, 4 elements per thread, 1024 elements per workgroup at every level.  No workgroup waits on
// another, no atomics, every sum in thread order: the prefixes are a function of the input.
#pragma once
#include "dn_common.h"

namespace dn {

constexpr int kScanThreads = 256;
constexpr int kScanPerThread = 4;
constexpr int kScanElems = kScanThreads * kScanPerThread;   // elements per workgroup at every scan level

__device__ __forceinline__ unsigned wave_scan_add(unsigned v) {
  const int l = lane_id();
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(v, o, 64);
    if (l >= o) v += t;
  }
  return v;
}

// Exclusive prefix of one value per thread over the 256 threads of the workgroup, in thread order; `total`: the workgroup's sum.
// `lds`: 4 words of this call's own.
__device__ __forceinline__ unsigned block_scan_exclusive(unsigned x, unsigned* lds, unsigned& total) {
  const unsigned inc = wave_scan_add(x);
  const int w = threadIdx.x >> 6;
  if (lane_id() == kWave - 1) lds[w] = inc;
  __syncthreads();
  unsigned before = 0, all = 0;
#pragma unroll
  for (int q = 0; q < kScanThreads / kWave; ++q) {
    const unsigned s = lds[q];
    before += q < w ? s : 0u;
    all += s;
  }
  total = all;
  return before + inc - x;
}

// a[0 .. n) -> its exclusive prefix inside every block of 1024, in place; up[b]: the sum of block b
__device__ __forceinline__ void scan_row(unsigned* __restrict__ a, unsigned n, unsigned* __restrict__ up, unsigned* lds) {
  const unsigned e0 = blockIdx.x * kScanElems + threadIdx.x * kScanPerThread;
  unsigned x[kScanPerThread], s = 0;
#pragma unroll
  for (int q = 0; q < kScanPerThread; ++q) { x[q] = e0 + q < n ? a[e0 + q] : 0u; s += x[q]; }
  unsigned all, run = block_scan_exclusive(s, lds, all);
#pragma unroll
  for (int q = 0; q < kScanPerThread; ++q) {
    if (e0 + q < n) a[e0 + q] = run;
    run += x[q];
  }
  if (threadIdx.x == 0) up[blockIdx.x] = all;
}

constexpr size_t up256(size_t x) { return (x + 255) & ~static_cast<size_t>(255); }

}  // namespace dn
