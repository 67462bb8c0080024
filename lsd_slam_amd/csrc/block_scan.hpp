// Scans inside a 256-lane workgroup, as the order-preserving compactions use them (cloud.hip: the viewer's point cloud; kfbank.hip: a
// keyframe's permanent reference).  Integer sums in lane order: no atomics, the same result on every run.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ int lsd_wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d);
    if (lane >= d) v += o;
  }
  return v;
}
// exclusive scan of one value per lane over the 256-lane workgroup (pixel order = lane order); *total = the workgroup's sum
__device__ __forceinline__ int lsd_block_excl_scan(int v, int* total, int* lds) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int inc = lsd_wave_incl_scan(v, lane);
  if (lane == 63) lds[wv] = inc;
  __syncthreads();
  int before = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) { const int s = lds[k]; if (k < wv) before += s; tot += s; }
  __syncthreads();
  *total = tot;
  return before + inc - v;
}
