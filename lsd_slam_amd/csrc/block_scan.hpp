// Scans and sums inside a 256-lane workgroup.  The scans are what the order-preserving compactions use (cloud.hip: the viewer's point
// cloud; kfbank.hip: a keyframe's permanent reference): integer sums in lane order, no atomics, the same result on every run.  The sums
// (further down) are the depth map's (depthmap.hip).
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

// Sums.  Two orders of addition exist in this library and a caller keeps the one it has: where the terms are not exactly summable (whole-map
// sums of 2^18 floats in double) the order is part of the result.
// every lane gets the sum over its wave (butterfly)
template <typename T>
__device__ __forceinline__ T lsd_wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
// (a, b) summed over the 256-lane workgroup by the LDS tree s[t] += s[t + off], off = 128 ... 1; every lane gets both sums.  A second
// call in the same kernel needs a barrier of the caller's before it (the arrays are reused).
template <typename A, typename B>
__device__ __forceinline__ void lsd_block_tree_sum(A& a, B& b) {
  __shared__ A s_a[256];
  __shared__ B s_b[256];
  const int t = threadIdx.x;
  s_a[t] = a; s_b[t] = b;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (t < off) { s_a[t] += s_a[t + off]; s_b[t] += s_b[t + off]; }
    __syncthreads();
  }
  a = s_a[0]; b = s_b[0];
}
// the same pair by a butterfly inside each wave and the four waves' partials through LDS, added ((0 + 1) + 2) + 3; lane 0 gets the sums
template <typename A, typename B>
__device__ __forceinline__ void lsd_block_butterfly_sum(A& a, B& b) {
  __shared__ A s_a[4];
  __shared__ B s_b[4];
  a = lsd_wave_sum(a); b = lsd_wave_sum(b);
  if ((threadIdx.x & 63) == 0) { s_a[threadIdx.x >> 6] = a; s_b[threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x == 0) { a = ((s_a[0] + s_a[1]) + s_a[2]) + s_a[3]; b = ((s_b[0] + s_b[1]) + s_b[2]) + s_b[3]; }
}
