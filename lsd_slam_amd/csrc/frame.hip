// Device-resident Frame: image / gradient / maxGradient / inverse-depth pyramids (K-pyr-*), point-cloud
// export (K0), ground-truth depth initialisation.  gfx950 only.  (The context the frames live on: context.hip.)
//
// Reference behaviour restated on the device:
//   Frame::Frame                 C/DataStructures/Frame.cpp:35-48    uint8 -> float copy (no scaling)
//   UndistorterPTAM::undistort   C/util/Undistorter.cpp:355-411      bilinear gather through the remap table, inside the uint8 -> float copy
//   Frame::initialize            Frame.cpp:397-459                   per-level intrinsics
//   Frame::buildImage            Frame.cpp:491-630                   2x2 box mean, SSE association (:532-544)
//   Frame::buildGradients        Frame.cpp:643-680                   linear-index walk incl. row wrap
//   Frame::buildMaxGradients     Frame.cpp:690-767                   |grad| + separable 3x3 max (linear-index ranges)
//   Frame::buildIDepthAndIDepthVar Frame.cpp:775-877                 inverse-variance 2x2 pooling
//   Frame::setDepthFromGroundTruth Frame.cpp:245-293
//   TrackingReference::makePointCloud C/Tracking/TrackingReference.cpp:96-147
// Unwritten pool memory of the reference is defined as 0 here (rows 0 / h-1 of gradients etc.).
#include <algorithm>
#include "lsdhip_internal.hpp"

// ---------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------

// One 16x16 level-0 tile per workgroup -> 8x8, 4x4, 2x2, 1x1 tiles of levels 1..4, all in one launch.
// HBM traffic: 1 B/px read (uint8) + 4 B * (1 + 1/4 + 1/16 + 1/64 + 1/256) written.
// The same workgroup also writes the level-0 gradient texels (gx, gy, I, 0) and |grad| of its 16x16 pixels, straight from
// the uint8 source (the float image is its exact conversion), with the reference's linear-index neighbour rule.
// The tile has two pixel sources: the frame's own (rectified) uint8 image, and a raw camera image fetched through an undistorter's remap
// table (lsdhip_frame_create_undistorted*), so that a raw frame is rectified inside the launch that converts it — no extra launch, no
// rectified uint8 plane in between.
struct PlainPixels {
  const uint8_t* __restrict__ gray;
  __device__ __forceinline__ float at(int i) const { return (float)gray[i]; }
};
// UndistorterPTAM::undistort (util/Undistorter.cpp:384-410) for one output pixel, as lsd_slam_hip::Undistorter::undistort
// (include/lsd_slam_hip_io.hpp) defines it: float32, left to right, every product and sum rounded on its own (the intrinsics keep the
// compiler from contracting them whatever -ffp-contract says), truncated to a byte with the range clamped.  m = (remapX, remapY) of the
// pixel; a valid entry lies inside (0, in_w - 1) x (0, in_h - 1) — lsdhip_undistorter_create refuses a table with any other — so the four
// taps are inside the raw image.  A tile's taps fall into a small window of the raw image: L2 hits; the streamed traffic is the table.
__device__ __forceinline__ float undistorted_pixel(LSD_G const uint8_t* __restrict__ raw, const float2 m, const int in_w) {
  float xx = m.x, yy = m.y;
  if (xx < 0) return 0.f;
  const int xxi = (int)xx, yyi = (int)yy;
  xx = __fsub_rn(xx, (float)xxi);
  yy = __fsub_rn(yy, (float)yyi);
  const float xxyy = __fmul_rn(xx, yy);
  LSD_G const uint8_t* src = raw + (xxi + yyi * in_w);
  const float s00 = (float)src[0], s10 = (float)src[1], s01 = (float)src[in_w], s11 = (float)src[1 + in_w];
  float v = __fmul_rn(xxyy, s11);
  v = __fadd_rn(v, __fmul_rn(__fsub_rn(yy, xxyy), s01));
  v = __fadd_rn(v, __fmul_rn(__fsub_rn(xx, xxyy), s10));
  v = __fadd_rn(v, __fmul_rn(__fadd_rn(__fsub_rn(__fsub_rn(1.0f, xx), yy), xxyy), s00));
  return !(v > 0.f) ? 0.f : (v >= 255.f ? 255.f : (float)(int)v);
}
// One interleaved (x, y) plane: a lane fetches its coordinate pair in one 8-byte load, a wave four 128-byte row pieces of the table.
struct RemappedPixels {
  LSD_G const uint8_t* __restrict__ raw;
  LSD_G const float2* __restrict__ map;
  int in_w;
  __device__ __forceinline__ float at(int i) const { return undistorted_pixel(raw, map[i], in_w); }
};
template <class Pixels>
__device__ __forceinline__ void image_pyramid_tile(const Pixels gray, float* __restrict__ i0,
                                                   float* __restrict__ i1, float* __restrict__ i2,
                                                   float* __restrict__ i3, float* __restrict__ i4, int w, int h,
                                                   float4* __restrict__ grad0, float* __restrict__ absgrad0) {
  __shared__ float s0[16][17];
  __shared__ float s1[8][9];
  __shared__ float s2[4][5];
  __shared__ float s3[2][3];
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int bx = blockIdx.x, by = blockIdx.y;
  {
    int x = bx * 16 + tx, y = by * 16 + ty;
    const int i = y * w + x;
    float v = gray.at(i);
    i0[i] = v;
    s0[ty][tx] = v;
    // Frame::buildGradients (Frame.cpp:643-680): rows 1..h-2 by linear index, so x = 0 / w-1 wrap into the neighbouring rows
    // (grad0 == nullptr — every frame since round 6: the level-0 gradients and maxGradients are keyframe planes, built when a frame
    // becomes one: lsd_frames_require_level0 below)
    if (grad0) {
      float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
      const bool inner = (i >= w) && (i < w * (h - 1));
      if (inner) {
        g.x = 0.5f * (gray.at(i + 1) - gray.at(i - 1));
        g.y = 0.5f * (gray.at(i + w) - gray.at(i - w));
        g.z = v;
      }
      grad0[i] = g;
      absgrad0[i] = inner ? sqrtf(g.x * g.x + g.y * g.y) : 0.f;
    }
  }
  __syncthreads();
  if (tid < 64) {
    int ax = tid & 7, ay = tid >> 3;
    float c0 = s0[2 * ay][2 * ax] + s0[2 * ay + 1][2 * ax];          // (top + bottom) of the left column
    float c1 = s0[2 * ay][2 * ax + 1] + s0[2 * ay + 1][2 * ax + 1];  // right column
    float r = (c0 + c1) * 0.25f;
    s1[ay][ax] = r;
    i1[(by * 8 + ay) * (w >> 1) + bx * 8 + ax] = r;
  }
  __syncthreads();
  if (tid < 16) {
    int ax = tid & 3, ay = tid >> 2;
    float c0 = s1[2 * ay][2 * ax] + s1[2 * ay + 1][2 * ax];
    float c1 = s1[2 * ay][2 * ax + 1] + s1[2 * ay + 1][2 * ax + 1];
    float r = (c0 + c1) * 0.25f;
    s2[ay][ax] = r;
    i2[(by * 4 + ay) * (w >> 2) + bx * 4 + ax] = r;
  }
  __syncthreads();
  if (tid < 4) {
    int ax = tid & 1, ay = tid >> 1;
    float c0 = s2[2 * ay][2 * ax] + s2[2 * ay + 1][2 * ax];
    float c1 = s2[2 * ay][2 * ax + 1] + s2[2 * ay + 1][2 * ax + 1];
    float r = (c0 + c1) * 0.25f;
    s3[ay][ax] = r;
    i3[(by * 2 + ay) * (w >> 3) + bx * 2 + ax] = r;
  }
  __syncthreads();
  if (tid == 0) {
    float c0 = s3[0][0] + s3[1][0];
    float c1 = s3[0][1] + s3[1][1];
    i4[by * (w >> 4) + bx] = (c0 + c1) * 0.25f;
  }
}
__global__ __launch_bounds__(256) void k_image_pyramid(const uint8_t* __restrict__ gray, float* __restrict__ i0,
                                                        float* __restrict__ i1, float* __restrict__ i2,
                                                        float* __restrict__ i3, float* __restrict__ i4, int w, int h,
                                                        float4* __restrict__ grad0, float* __restrict__ absgrad0) {
  image_pyramid_tile(PlainPixels{gray}, i0, i1, i2, i3, i4, w, h, grad0, absgrad0);
}
// ... of a raw in_w-wide camera image through an undistorter's table (lsdhip_frame_create_undistorted*)
__global__ __launch_bounds__(256) void k_image_pyramid_remap(const uint8_t* __restrict__ raw, const float2* __restrict__ map, int in_w,
                                                              float* __restrict__ i0, float* __restrict__ i1, float* __restrict__ i2,
                                                              float* __restrict__ i3, float* __restrict__ i4, int w, int h) {
  image_pyramid_tile(RemappedPixels{lsd_g(raw), lsd_g(map), in_w}, i0, i1, i2, i3, i4, w, h, (float4*)nullptr, (float*)nullptr);
}
// The rectified uint8 image itself (lsdhip_undistorter_apply): one output pixel per lane
__global__ __launch_bounds__(256) void k_undistort(const uint8_t* __restrict__ raw, const float2* __restrict__ map, int in_w,
                                                    uint8_t* __restrict__ out, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (uint8_t)undistorted_pixel(lsd_g(raw), map[i], in_w);
}
// the same for the new frames of several sequences in one launch (blockIdx.z = frame; lsdhip_frame_create_batch)
struct ImagePyrItem {
  LSD_G const uint8_t* gray;
  LSD_G float* img[LSD_LEVELS];
  LSD_G float4* grad0;
  LSD_G float* absgrad0;
};
__global__ __launch_bounds__(256) void k_image_pyramid_batch(const ImagePyrItem* __restrict__ items, int w, int h) {
  const ImagePyrItem it = items[blockIdx.z];
  image_pyramid_tile(PlainPixels{it.gray}, it.img[0], it.img[1], it.img[2], it.img[3], it.img[4], w, h, it.grad0, it.absgrad0);
}
// ... of raw images (items[].gray) through one undistorter's table (lsdhip_frame_create_undistorted_batch)
__global__ __launch_bounds__(256) void k_image_pyramid_remap_batch(const ImagePyrItem* __restrict__ items, const float2* __restrict__ map,
                                                                    int in_w, int w, int h) {
  const ImagePyrItem it = items[blockIdx.z];
  image_pyramid_tile(RemappedPixels{it.gray, lsd_g(map), in_w}, it.img[0], it.img[1], it.img[2], it.img[3], it.img[4], w, h, (float4*)nullptr,
                     (float*)nullptr);
}

struct GradArgs {
  const float* img[LSD_LEVELS];
  float4* grad[LSD_LEVELS];
  float* absgrad0;
  int w[LSD_LEVELS], h[LSD_LEVELS];
};

// Second launch of a new frame: the gradient texels of levels 1..4 (4 B/px read + neighbours from L2, 16 B/px written); the level-1
// blocks also leave the frame's refPixelWasGood mask in its "never written" state (0xFF), so that the tracker needs no separate fill
// before its first use.  (Until round 6 the launch carried the level-0 maxGradients as extra blocks — hence the name; that plane is a
// keyframe plane now: k_maxgrad_candidates.)
struct GradMaxArgs {
  LSD_G const float* img[LSD_LEVELS];
  LSD_G float4* grad[LSD_LEVELS];
  int w[LSD_LEVELS], h[LSD_LEVELS];
  int blk0[LSD_LEVELS + 1];     // first block of level l's gradient range (levels 1..4); blk0[LSD_LEVELS] = gradBlocks
  LSD_G uint32_t* wasGoodWords;
  int nMaskWords;
};
// Frame::buildMaxGradients (Frame.cpp:682-747) for one pixel: separable 3x3 maximum of |grad| with the reference's linear-index validity
// ranges (the vertical pass covers [w + 1, w (h - 1) - 1), the horizontal pass the same range; the two border values it copies)
__device__ __forceinline__ float max_gradient_at(LSD_G const float* __restrict__ absg, const int w, const int h, const int i) {
  const int lo = w + 1, hi = w * (h - 1) - 1;
  auto vmax = [&](int j) -> float {
    if (j < lo || j >= hi) return 0.f;
    float g1 = absg[j - w];
    float g2 = absg[j];
    if (g1 < g2) g1 = g2;
    float g3 = absg[j + w];
    return (g1 < g3) ? g3 : g1;
  };
  float out = 0.f;
  if (i >= lo && i < hi) {
    float g1 = vmax(i - 1);
    float g2 = vmax(i);
    if (g1 < g2) g1 = g2;
    float g3 = vmax(i + 1);
    out = (g1 < g3) ? g3 : g1;
  } else if (i == w || i == hi) {
    out = absg[i];
  }
  return out;
}
__device__ __forceinline__ void gradients_max_block(const GradMaxArgs& a) {
  const int b = blockIdx.x;
  if (b < a.blk0[LSD_LEVELS]) {
    int l = 1;
#pragma unroll
    for (int k = 2; k < LSD_LEVELS; k++) if (b >= a.blk0[k]) l = k;
    const int w = a.w[l], h = a.h[l];
    const int i = (b - a.blk0[l]) * 256 + threadIdx.x;
    if (l == 1 && i < a.nMaskWords) a.wasGoodWords[i] = 0xFFFFFFFFu;   // the frame's level-1 refPixelWasGood in its "never written" state
    if (i >= w * h) return;
    const float* __restrict__ img = a.img[l];
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool inner = (i >= w) && (i < w * (h - 1));
    if (inner) {
      g.x = 0.5f * (img[i + 1] - img[i - 1]);
      g.y = 0.5f * (img[i + w] - img[i - w]);
      g.z = img[i];
    }
    a.grad[l][i] = g;
  }
}
__global__ __launch_bounds__(256) void k_gradients_max(GradMaxArgs a) { gradients_max_block(a); }
__global__ __launch_bounds__(256) void k_gradients_max_batch(const GradMaxArgs* __restrict__ items) {
  __shared__ GradMaxArgs s_a;     // (a by-value copy of an indexed record would live in scratch: the level tables are indexed dynamically)
  const int* src = (const int*)(items + blockIdx.y);
  for (int i = threadIdx.x; i < (int)(sizeof(GradMaxArgs) / 4); i += 256) ((int*)&s_a)[i] = src[i];
  __syncthreads();
  gradients_max_block(s_a);
}

// Level-0 gradients (gx, gy, I, 0) and |grad| from the level-0 float image (the exact conversion of the 8-bit source): the arithmetic the
// image pyramid kernel did for every frame until round 6 (Frame::buildGradients, Frame.cpp:643-680, rows 1..h-2 by linear index).
// The reference builds Frame::gradients(0) and maxGradients(0) on demand, and only keyframes are ever asked for them (DepthMap's
// observe / regularise / propagate, setDepthFromGroundTruth); a tracked frame needs the levels >= 1.  So do we now: 7.3 of the 12.6 MB a
// 640x480 frame's pyramids moved were these two planes and the |grad| scratch.
struct Level0Item {
  LSD_G const float* img0;
  LSD_G float4* grad0;
  LSD_G float* absgrad;
};
__device__ __forceinline__ void level0_gradients_px(const Level0Item& a, const int w, const int h) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= w * h) return;
  const float v = a.img0[i];
  float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
  const bool inner = (i >= w) && (i < w * (h - 1));
  if (inner) {
    g.x = 0.5f * (a.img0[i + 1] - a.img0[i - 1]);
    g.y = 0.5f * (a.img0[i + w] - a.img0[i - w]);
    g.z = v;
  }
  a.grad0[i] = g;
  a.absgrad[i] = inner ? sqrtf(g.x * g.x + g.y * g.y) : 0.f;
}
__global__ __launch_bounds__(256) void k_level0_gradients(Level0Item a, int w, int h) { level0_gradients_px(a, w, h); }
__global__ __launch_bounds__(256) void k_level0_gradients_batch(const Level0Item* __restrict__ items, int w, int h) {
  const Level0Item a = items[blockIdx.y];
  level0_gradients_px(a, w, h);
}

// Gradient candidates of a keyframe (lsdhip_frame::d_gradCand): one workgroup per group of 1024 consecutive pixels, four per lane; the
// offsets of the group's candidates — inside the 3-pixel border, !(maxGradients < minUseGrad): the two tests of observeDepthRow that
// depend on nothing but the keyframe (DepthMap.cpp:111-131) — compacted in pixel order, and their number.
struct GradCandItem {
  LSD_G const float* maxgrad;
  LSD_G uint16_t* cand;
};
__device__ __forceinline__ void grad_cand_group(const GradCandItem& a, const int w, const int h, const float th) {
  __shared__ int s_w[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n0 = w * h, g = blockIdx.x;
  const int i0 = g * 1024 + tid * 4;
  unsigned m = 0;
  int y = i0 / w, x = i0 - y * w;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int i = i0 + k;
    if (i < n0 && !(x < 3 || x >= w - 3 || y < 3 || y >= h - 3) && !(a.maxgrad[i] < th)) m |= 1u << k;
    if (++x >= w) { x = 0; y++; }
  }
  const int cnt = __popc(m);
  int incl = cnt;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(incl, d);
    if (lane >= d) incl += t;
  }
  if (lane == 63) s_w[wave] = incl;
  __syncthreads();
  int pos = incl - cnt;
#pragma unroll
  for (int q = 0; q < 4; q++) pos += q < wave ? s_w[q] : 0;
  LSD_G uint16_t* out = a.cand + (size_t)g * 1024;
#pragma unroll
  for (int k = 0; k < 4; k++)
    if ((m >> k) & 1u) out[pos++] = (uint16_t)(tid * 4 + k);
  if (tid == 0) a.cand[(size_t)((n0 + 1023) >> 10) * 1024 + g] = (uint16_t)((s_w[0] + s_w[1]) + (s_w[2] + s_w[3]));
}
__global__ __launch_bounds__(256) void k_grad_candidates(GradCandItem a, int w, int h, float th) { grad_cand_group(a, w, h, th); }
__global__ __launch_bounds__(256) void k_grad_candidates_batch(const GradCandItem* __restrict__ items, int w, int h, float th) {
  const GradCandItem a = items[blockIdx.y];
  grad_cand_group(a, w, h, th);
}

// maxGradients(0) and the gradient candidates in one launch (the keyframe planes' second launch): one workgroup of 1024 lanes per group of
// 1024 consecutive pixels, one pixel per lane.
struct MaxCandItem {
  LSD_G const float* absg;
  LSD_G float* maxgrad;
  LSD_G uint16_t* cand;
};
__device__ __forceinline__ void maxgrad_cand_group(const MaxCandItem& a, const int w, const int h, const float th) {
  __shared__ int s_w[16];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n0 = w * h, g = blockIdx.x;
  const int i = g * 1024 + tid;
  bool cand = false;
  if (i < n0) {
    const float mg = max_gradient_at(a.absg, w, h, i);
    a.maxgrad[i] = mg;
    const int y = i / w, x = i - y * w;
    cand = !(x < 3 || x >= w - 3 || y < 3 || y >= h - 3) && !(mg < th);
  }
  const unsigned long long bal = __ballot(cand);
  if (lane == 0) s_w[wave] = __popcll(bal);
  __syncthreads();
  int pos = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u)), total = 0;
#pragma unroll
  for (int q = 0; q < 16; q++) { pos += q < wave ? s_w[q] : 0; total += s_w[q]; }
  if (cand) a.cand[(size_t)g * 1024 + pos] = (uint16_t)tid;
  if (tid == 0) a.cand[(size_t)((n0 + 1023) >> 10) * 1024 + g] = (uint16_t)total;
}
__global__ __launch_bounds__(1024) void k_maxgrad_candidates(MaxCandItem a, int w, int h, float th) { maxgrad_cand_group(a, w, h, th); }
__global__ __launch_bounds__(1024) void k_maxgrad_candidates_batch(const MaxCandItem* __restrict__ items, int w, int h, float th) {
  const MaxCandItem a = items[blockIdx.y];
  maxgrad_cand_group(a, w, h, th);
}

// inverse-variance pooling of one 2x2 block, children in the order idx, idx+1, idx+sw, idx+sw+1
__device__ __forceinline__ void pool4(const float id[4], const float var[4], float& oid, float& ovar) {
  float idepthSumsSum = 0.f, ivarSumsSum = 0.f;
  int num = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (var[k] > 0) {
      float ivar = lsd_rcp_exact(var[k]);
      ivarSumsSum += ivar;
      idepthSumsSum += ivar * id[k];
      num++;
    }
  }
  if (num > 0) {
    float depth = ivarSumsSum / idepthSumsSum;
    oid = lsd_rcp_exact(depth);
    ovar = num / ivarSumsSum;
  } else {
    oid = -1.f;
    ovar = -1.f;
  }
}

struct DepthPyrArgs {
  LSD_G float* id[LSD_LEVELS];
  LSD_G float* var[LSD_LEVELS];
  int w0, h0;
  // optional passenger: one extra workgroup (blockIdx.y == gridDim.y - 1, blockIdx.x == 0 of an extra grid row) folds the
  // (sum, count) partials of the setDepth that produced level 0 into a pinned record (Frame::setDepth's meanIdepth / numPoints)
  LSD_G const double* redPartials;
  int redN;
  LSD_G double* redOut;
  LSD_G uint8_t* blk[LSD_LEVELS];   // reference blocks of levels >= 1 (k_ref_blocks)
};

// Levels 1..4 of (idepth, idepthVar) from level 0, one 32x32 level-0 tile per workgroup: every lane pools one 2x2 block of level 0
// straight from HBM (two 8-byte loads per plane) into its level-1 pixel, the coarser levels follow through LDS (16x16 -> 8x8 -> 4x4 ->
// 2x2).  (Rounds 1-4: 16x16 tiles, one level-0 pixel per lane — a quarter of the bytes per workgroup and four barriers for them: 41 %
// of the HBM peak with 32 maps per launch.)  Image sizes are multiples of 16, so a tile may hang over the right / lower edge by half.
__device__ __forceinline__ void idepth_pyramid_tile(const DepthPyrArgs& a) {
  __shared__ float tid1[16][17], tvar1[16][17];
  __shared__ float tid2[8][9], tvar2[8][9];
  __shared__ float tid3[4][5], tvar3[4][5];
  const int tid = threadIdx.x;
  const int bx = blockIdx.x, by = blockIdx.y;
  const int w0 = a.w0, h0 = a.h0;
  if (a.redPartials && by == (int)gridDim.y - 1) {
    if (bx != 0) return;
    __shared__ double s_a[256], s_b[256];
    double sa = 0, sb = 0;
    for (int i = tid; i < a.redN; i += 256) { sa += a.redPartials[2 * i]; sb += a.redPartials[2 * i + 1]; }
    s_a[tid] = sa;
    s_b[tid] = sb;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if (tid < off) { s_a[tid] += s_a[tid + off]; s_b[tid] += s_b[tid + off]; }
      __syncthreads();
    }
    if (tid == 0) { a.redOut[0] = s_a[0]; a.redOut[1] = s_b[0]; a.redOut[2] = 0.0; }
    return;
  }
  {
    const int ax = tid & 15, ay = tid >> 4;
    const int x = bx * 32 + 2 * ax, y = by * 32 + 2 * ay;         // the block's upper left level-0 pixel
    float oi = -1.f, ov = -1.f;
    if (x < w0 && y < h0) {
      const float2 i0 = *(const float2*)(a.id[0] + (size_t)y * w0 + x), i1 = *(const float2*)(a.id[0] + (size_t)(y + 1) * w0 + x);
      const float2 v0 = *(const float2*)(a.var[0] + (size_t)y * w0 + x), v1 = *(const float2*)(a.var[0] + (size_t)(y + 1) * w0 + x);
      const float i4[4] = {i0.x, i0.y, i1.x, i1.y};
      const float v4[4] = {v0.x, v0.y, v1.x, v1.y};
      pool4(i4, v4, oi, ov);
      const int o = (by * 16 + ay) * (w0 >> 1) + bx * 16 + ax;
      a.id[1][o] = oi; a.var[1][o] = ov;
    }
    tid1[ay][ax] = oi; tvar1[ay][ax] = ov;
  }
  __syncthreads();
  if (tid < 64) {
    const int ax = tid & 7, ay = tid >> 3;
    float i4[4] = {tid1[2 * ay][2 * ax], tid1[2 * ay][2 * ax + 1], tid1[2 * ay + 1][2 * ax], tid1[2 * ay + 1][2 * ax + 1]};
    float v4[4] = {tvar1[2 * ay][2 * ax], tvar1[2 * ay][2 * ax + 1], tvar1[2 * ay + 1][2 * ax], tvar1[2 * ay + 1][2 * ax + 1]};
    float oi, ov;
    pool4(i4, v4, oi, ov);
    tid2[ay][ax] = oi; tvar2[ay][ax] = ov;
    if (bx * 8 + ax < (w0 >> 2) && by * 8 + ay < (h0 >> 2)) {
      const int o = (by * 8 + ay) * (w0 >> 2) + bx * 8 + ax;
      a.id[2][o] = oi; a.var[2][o] = ov;
    }
  }
  __syncthreads();
  if (tid < 16) {
    const int ax = tid & 3, ay = tid >> 2;
    float i4[4] = {tid2[2 * ay][2 * ax], tid2[2 * ay][2 * ax + 1], tid2[2 * ay + 1][2 * ax], tid2[2 * ay + 1][2 * ax + 1]};
    float v4[4] = {tvar2[2 * ay][2 * ax], tvar2[2 * ay][2 * ax + 1], tvar2[2 * ay + 1][2 * ax], tvar2[2 * ay + 1][2 * ax + 1]};
    float oi, ov;
    pool4(i4, v4, oi, ov);
    tid3[ay][ax] = oi; tvar3[ay][ax] = ov;
    if (bx * 4 + ax < (w0 >> 3) && by * 4 + ay < (h0 >> 3)) {
      const int o = (by * 4 + ay) * (w0 >> 3) + bx * 4 + ax;
      a.id[3][o] = oi; a.var[3][o] = ov;
    }
  }
  __syncthreads();
  if (tid < 4) {
    const int ax = tid & 1, ay = tid >> 1;
    float i4[4] = {tid3[2 * ay][2 * ax], tid3[2 * ay][2 * ax + 1], tid3[2 * ay + 1][2 * ax], tid3[2 * ay + 1][2 * ax + 1]};
    float v4[4] = {tvar3[2 * ay][2 * ax], tvar3[2 * ay][2 * ax + 1], tvar3[2 * ay + 1][2 * ax], tvar3[2 * ay + 1][2 * ax + 1]};
    float oi, ov;
    pool4(i4, v4, oi, ov);
    if (bx * 2 + ax < (w0 >> 4) && by * 2 + ay < (h0 >> 4)) {
      const int o = (by * 2 + ay) * (w0 >> 4) + bx * 2 + ax;
      a.id[4][o] = oi; a.var[4][o] = ov;
    }
  }
}
__global__ __launch_bounds__(256) void k_idepth_pyramid(DepthPyrArgs a) { idepth_pyramid_tile(a); }
__global__ __launch_bounds__(256) void k_idepth_pyramid_batch(const DepthPyrArgs* __restrict__ items) {
  const DepthPyrArgs a = items[blockIdx.z];
  idepth_pyramid_tile(a);
}

// Reference blocks of the idepth pyramid's levels >= 1: which pixels of a level are reference points of a tracking job — inside the
// one-pixel border, idepthVar > 0, idepth != 0: the test of TrackingReference::makePointCloud (C/Tracking/TrackingReference.cpp:120-131) —
// depends on the keyframe's planes alone, and a throughput-mode batch asks it of every pixel in every evaluation (8 bytes per pixel, four
// ballots per 1024 pixels, a barrier).  Answered once per pyramid instead: one wave per block of 256 consecutive pixels leaves the
// in-block offsets of the block's valid pixels, in pixel order, in the block's 256 bytes (slot-interleaved, below), and the count in the table behind the blocks;
// strips are multiples of 256 pixels, so a strip's list is the concatenation of its blocks' lists — no scan over the level.
__device__ __forceinline__ void ref_blocks_tile(const DepthPyrArgs& a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int gb = blockIdx.x * 4 + wave;
  int l = 1, w = a.w0 >> 1, h = a.h0 >> 1;
  for (; l < LSD_LEVELS; l++) {
    const int nb = (w * h + 255) >> 8;
    if (gb < nb) break;
    gb -= nb;
    w >>= 1; h >>= 1;
  }
  if (l >= LSD_LEVELS) return;
  const int work = w * h, nblk = (work + 255) >> 8;
  const int i0 = gb * 256 + lane * 4;
  LSD_G const float* id = nullptr;
  LSD_G const float* var = nullptr;
  LSD_G uint8_t* blk = nullptr;
#pragma unroll
  for (int q = 1; q < LSD_LEVELS; q++)          // (no dynamic index into the argument record: it would move to scratch memory)
    if (q == l) { id = a.id[q]; var = a.var[q]; blk = a.blk[q]; }
  unsigned m = 0;
  int y = i0 / w, x = i0 - y * w;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int i = i0 + k;
    if (i < work) {
      const float vv = var[i], dd = id[i];
      const bool ok = !(x < 1 || x >= w - 1 || y < 1 || y >= h - 1) && !(vv <= 0 || dd == 0);
      m |= (ok ? 1u : 0u) << k;
    }
    if (++x >= w) { x = 0; y++; }
  }
  const int cnt = __popc(m);
  int incl = cnt;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(incl, d);
    if (lane >= d) incl += t;
  }
  LSD_G uint8_t* out = blk + (size_t)gb * 256;
  // slot s of the block's list lives in byte (s mod 64) * 4 + s / 64: the reader's lane l takes one 4-byte word = slots l, l + 64, l + 128,
  // l + 192, so the lanes of a wave fill consecutive list entries (no LDS bank conflicts)
  int pos = incl - cnt;
#pragma unroll
  for (int k = 0; k < 4; k++)
    if ((m >> k) & 1u) { out[((pos & 63) << 2) + (pos >> 6)] = (uint8_t)(lane * 4 + k); pos++; }
  if (lane == 63) ((LSD_G int*)(blk + (size_t)nblk * 256))[gb] = incl;
}
__global__ __launch_bounds__(256) void k_ref_blocks(DepthPyrArgs a) { ref_blocks_tile(a); }
__global__ __launch_bounds__(256) void k_ref_blocks_batch(const DepthPyrArgs* __restrict__ items) {
  const DepthPyrArgs a = items[blockIdx.z];
  ref_blocks_tile(a);
}
static int lsd_refblk_grid(const lsdhip_ctx* c) {
  int nb = 0;
  for (int l = 1; l < LSD_LEVELS; l++) nb += lsd_refblk_blocks(c->wl[l] * c->hl[l]);
  return (nb + 3) / 4;
}

// Frame::setDepthFromGroundTruth
__global__ __launch_bounds__(256) void k_set_depth_gt(const float* __restrict__ depth, const float* __restrict__ maxgrad,
                                                       float* __restrict__ id, float* __restrict__ var, int w, int h,
                                                       float cov_scale, float minUseGrad) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= w * h) return;
  int x = i % w, y = i / w;
  float d = depth[i];
  if (x > 0 && x < w - 1 && y > 0 && y < h - 1 && maxgrad[i] >= minUseGrad && !isnan(d) && d > 0) {
    id[i] = 1.0f / d;
    var[i] = 0.01f * 0.01f * cov_scale;  // VAR_GT_INIT_INITIAL * cov_scale (C/util/settings.h:75)
  } else {
    id[i] = -1.f;
    var[i] = -1.f;
  }
}

// ---- K0: TrackingReference::makePointCloud, x outer / y inner, order preserving ------------------------------
__global__ __launch_bounds__(256) void k_pc_count(const float* __restrict__ id, const float* __restrict__ var, int w, int h,
                                                   int* __restrict__ colCount) {
  int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= w) return;
  int c = 0;
  if (x >= 1 && x < w - 1)
    for (int y = 1; y < h - 1; y++) {
      int idx = x + y * w;
      if (!(var[idx] <= 0 || id[idx] == 0)) c++;
    }
  colCount[x] = c;
}
__global__ void k_pc_scan(int* __restrict__ colCount, int w, int* __restrict__ total) {
  // single thread exclusive scan over <= a few thousand columns (keyframe-rate export path, not the hot path)
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    int acc = 0;
    for (int x = 0; x < w; x++) { int c = colCount[x]; colCount[x] = acc; acc += c; }
    *total = acc;
  }
}
__global__ __launch_bounds__(256) void k_pc_write(const float* __restrict__ id, const float* __restrict__ var,
                                                   const float* __restrict__ img, const float4* __restrict__ grad, int w, int h,
                                                   float fxi, float fyi, float cxi, float cyi, const int* __restrict__ colOff,
                                                   float* __restrict__ pos, float* __restrict__ colvar,
                                                   float* __restrict__ gradOut, int* __restrict__ idxOut) {
  int x = blockIdx.x * 256 + threadIdx.x;
  if (x < 1 || x >= w - 1) return;
  int n = colOff[x];
  for (int y = 1; y < h - 1; y++) {
    int idx = x + y * w;
    float v = var[idx], d = id[idx];
    if (v <= 0 || d == 0) continue;
    float inv = 1.0f / d;
    pos[3 * n + 0] = inv * (fxi * x + cxi);
    pos[3 * n + 1] = inv * (fyi * y + cyi);
    pos[3 * n + 2] = inv * 1.0f;
    float4 g = grad[idx];
    gradOut[2 * n + 0] = g.x;
    gradOut[2 * n + 1] = g.y;
    colvar[2 * n + 0] = img[idx];
    colvar[2 * n + 1] = v;
    idxOut[n] = idx;
    n++;
  }
}

// ---------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------
// TrackingReference::importFrame (C/Tracking/TrackingReference.cpp:71-87) as the tracking side's hand-over point: the newest
// Frame::setDepth result of the mapping stream becomes what SE3Tracker jobs read.  A no-op on non-pipelined contexts.
int lsd_frame_publish_depth(lsdhip_frame* f) {
  if (!f->depthPending) return LSDHIP_OK;
  for (int l = 0; l < LSD_LEVELS; l++) { std::swap(f->d_idepth[l], f->d_idepthW[l]); std::swap(f->d_idepthVar[l], f->d_idepthVarW[l]); std::swap(f->d_refBlk[l], f->d_refBlkW[l]); }
  std::swap(f->refBlkValid, f->refBlkValidW);
  f->depthPending = false;
  f->depthSeq = f->depthPendingSeq;
  f->hasIDepth = true;
  f->depthVersion++;
  return LSDHIP_OK;
}
extern "C" int lsdhip_frame_publish_depth(lsdhip_frame* f) {
  if (!f) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(f->ctx);
  return lsd_frame_publish_depth(f);
}
int lsd_frame_resolve(lsdhip_frame* f) {
  if (f->pendStats < 0 && f->pendRescale < 0) return LSDHIP_OK;
  lsdhip_ctx* c = f->ctx;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  // the values are in pinned host memory once the kernels that write them have completed: known without a synchronisation when a
  // tracking job enqueued after them has been seen to finish (the ring of slots wraps onto a retired keyframe's every few keyframes)
  bool landed;
  if (c->pipeline) {
    // the slots are written on the mapping stream: done once the record point behind their DepthMap call has been passed
    landed = (f->pendRescale < 0 || lsd_m_done(c, c->slot_mseq[f->pendRescale])) && (f->pendStats < 0 || lsd_m_done(c, c->slot_mseq[f->pendStats]));
    if (!landed) {
      // (inside an open lane region the slot's record point does not exist yet — it is recorded where the lanes join — and the kernels
      // that write the slot were queued on a lane: drain the lanes in use as well)
      for (int i = 0; i < c->lanes_open; i++) if (c->lane_used[i]) HIPCHK(hipStreamSynchronize(c->lanes[i]));
      HIPCHK(hipStreamSynchronize(c->mstream));
      c->mDoneSeq = c->mSeq;
    }
  } else {
    landed = (f->pendRescale < 0 || c->doneEpoch > c->slot_epoch[f->pendRescale]) &&
             (f->pendStats < 0 || c->doneEpoch > c->slot_epoch[f->pendStats]);
    if (!landed) {
      for (int i = 0; i < c->lanes_open; i++) if (c->lane_used[i]) HIPCHK(hipStreamSynchronize(c->lanes[i]));   // (a slot written on a lane)
      HIPCHK(hipStreamSynchronize(c->stream));
      c->enqEpoch++;
      c->doneEpoch = c->enqEpoch;
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  int rc = LSDHIP_OK;
  if (f->pendRescale >= 0) {
    const DeferredSlot& s = c->h_slots[f->pendRescale];
    // rescaleFactor = numIdepth / sumIdepth in float (DepthMap.cpp:1294), the expression k_rescale evaluated
    const float sumIdepth = (float)s.sum, numIdepth = (float)s.count;
    f->thisToParent_raw.s = numIdepth / sumIdepth;
    if (s.flag != 0) { lsd_set_error("propagateDepth: too many source hypotheses mapped to one target pixel"); rc = LSDHIP_E_CAPACITY; }
    c->slot_rescale_owner[f->pendRescale] = nullptr;
    f->pendRescale = -1;
  }
  if (f->pendStats >= 0) {
    const DeferredSlot& s = c->h_slots[f->pendStats];
    const float sumIdepth = (float)s.sum;
    const int numIdepth = (int)s.count;
    f->meanIdepth = sumIdepth / numIdepth;
    f->numPoints = numIdepth;
    c->slot_stats_owner[f->pendStats] = nullptr;
    f->pendStats = -1;
  }
  return rc;
}

// ---- frames: arena, pyramids, planes on demand ------------------------------------------------------------------------------------------
// One arena per frame, out of the context's pool where it holds one.  Which planes it has and where: lsd_frame_planes (frame_layout.hpp).
static int frame_alloc(lsdhip_ctx* c, int id, lsdhip_frame** out) {
  LSD_CTX_LOCK(c);
  LsdFrameLayout& lay = c->frameLayout;
  if (lay.n == 0) {
    lay = lsd_frame_layout<lsdhip_frame>(c->wl, c->hl);
    c->arena_bytes = lay.bytes;
  }
  if (lay.n > LsdFrameLayout::MAX_PLANES) { lsd_set_error("frame_alloc: %d planes do not fit the layout table", lay.n); return LSDHIP_E_STATE; }
  std::unique_ptr<lsdhip_frame> f(new lsdhip_frame());
  if (!c->free_arenas.empty()) {
    f->arena = std::move(c->free_arenas.back());
    c->free_arenas.pop_back();
  } else if (int rc = lsd_dev_alloc(f->arena, c->arena_bytes)) return rc;
  f->ctx = c;
  f->id = id;
  f->thisToParent_raw.q = {1, 0, 0, 0};
  f->thisToParent_raw.t[0] = f->thisToParent_raw.t[1] = f->thisToParent_raw.t[2] = 0;
  f->thisToParent_raw.s = 1;
  lsd_frame_bind(*f, lay, c->wl, c->hl, f->arena.get());
  *out = f.release();
  return LSDHIP_OK;
}

// The gradient launch of a new frame: levels 1..4 as ranges of 256-pixel blocks, and the level-1 mask words it fills with 0xFF
static GradMaxArgs grad_max_args(const lsdhip_frame* f) {
  const lsdhip_ctx* c = f->ctx;
  GradMaxArgs ga;
  int nb = 0;
  for (int l = 0; l < LSD_LEVELS; l++) {
    ga.img[l] = lsd_g(f->d_image[l]); ga.grad[l] = lsd_g(f->d_grad[l]); ga.w[l] = c->wl[l]; ga.h[l] = c->hl[l];
    ga.blk0[l] = nb;
    if (l >= 1) nb += (c->wl[l] * c->hl[l] + 255) / 256;
  }
  ga.blk0[LSD_LEVELS] = nb;
  ga.wasGoodWords = lsd_g((uint32_t*)f->d_wasGood); ga.nMaskWords = (c->wl[1] * c->hl[1] + 3) / 4;
  return ga;
}
// What the pyramid launches leave: a frame that owns nothing its (recycled) arena held before
static void frame_pyramids_queued(lsdhip_frame* f) {
  f->level0Ready = false; f->gradCandTh = -1.0f;   // keyframe planes and candidates: on demand (lsd_frames_require_level0)
  f->wasGoodPristine = true;                       // the mask holds the gradient launch's 0xFF fill
}

// A camera's rectification on the device (lsdhip_undistorter_create): the remap table of the context's w x h output image, resident, and
// the staging for raw host images — a raw image may be larger than a frame's own uint8 plane (in_w * in_h > w * h), so d_gray cannot take it.
struct lsdhip_undistorter {
  lsdhip_ctx* ctx = nullptr;
  int in_w = 0, in_h = 0;
  LsdDev<float2> d_map;                // (remapX, remapY) interleaved, w * h entries
  // One slot per batch entry (grown by the first batch that is wider; never per frame).  INVARIANT: a slot's upload and the launch that
  // reads it are both queued on the mapping stream (lsd_map_stream), so the next upload into the slot is ordered behind that launch by the
  // stream itself; stageStream remembers the stream, and a call that finds another one current (a lane region, a pipeline switch) drains it first.
  std::vector<LsdDev<uint8_t>> stage;
  hipStream_t stageStream = nullptr;   // (one of the context's streams: not owned)
  LsdDev<uint8_t> d_out;               // lsdhip_undistorter_apply with a host destination
  size_t rawBytes() const { return (size_t)in_w * in_h; }
};
// raw host images -> staging slots 0 .. n - 1 on stream `ms` (see the invariant above); dev[j] = where image j is on the device
static int undistorter_stage(lsdhip_undistorter* u, int n, const uint8_t* const* raw_host, hipStream_t ms, const uint8_t** dev) {
  if (u->stageStream && u->stageStream != ms) HIPCHK(hipStreamSynchronize(u->stageStream));
  u->stageStream = ms;
  while ((int)u->stage.size() < n) {
    LsdDev<uint8_t> p;
    if (int rc = lsd_dev_alloc(p, u->rawBytes())) return rc;
    u->stage.push_back(std::move(p));
  }
  for (int j = 0; j < n; j++) {
    HIPCHK(hipMemcpyAsync(u->stage[j], raw_host[j], u->rawBytes(), hipMemcpyHostToDevice, ms));
    dev[j] = u->stage[j];
  }
  return LSDHIP_OK;
}

// src: the image where it is on the device (null: the frame's own uint8 plane); with an undistorter, a raw image (never null)
static int frame_build_pyramids(lsdhip_frame* f, const uint8_t* src, hipStream_t stream, const lsdhip_undistorter* u) {
  lsdhip_ctx* c = f->ctx;
  LSD_CTX_LOCK(c);
  if (!stream) stream = lsd_map_stream(c);
  lsdhip_host_mark(21);
  if (u)
    hipLaunchKernelGGL(k_image_pyramid_remap, dim3(c->w / 16, c->h / 16), dim3(256), 0, stream, src, (const float2*)u->d_map, u->in_w,
                       f->d_image[0], f->d_image[1], f->d_image[2], f->d_image[3], f->d_image[4], c->w, c->h);
  else
    hipLaunchKernelGGL(k_image_pyramid, dim3(c->w / 16, c->h / 16), dim3(256), 0, stream, src ? src : f->d_gray, f->d_image[0], f->d_image[1],
                       f->d_image[2], f->d_image[3], f->d_image[4], c->w, c->h, (float4*)nullptr, (float*)nullptr);
  const GradMaxArgs ga = grad_max_args(f);
  lsdhip_host_mark(22);
  hipLaunchKernelGGL(k_gradients_max, dim3(ga.blk0[LSD_LEVELS]), dim3(256), 0, stream, ga);   // the gradient blocks only: maxGradients is a keyframe plane (lsd_frames_require_level0)
  lsdhip_host_mark(23);
  HIPCHK(hipGetLastError());
  frame_pyramids_queued(f);
  return LSDHIP_OK;
}
int lsd_frame_build_pyramids(lsdhip_frame* f, const uint8_t* src, hipStream_t stream) { return frame_build_pyramids(f, src, stream, nullptr); }

// Two item arrays in one argument record (one copy for both launches of a pair): A[n] at its start, B[n] from the next 256-byte boundary
// on.  Filled in place between args_pair_begin and lsd_args_commit; lsd_args_release(dev) behind the launches.
template <class A, class B> struct ArgPair {
  A* a; B* b;                      // the pinned record, to be filled
  const A* devA; const B* devB;    // what the launches read
  void* dev;
};
template <class A, class B> static int args_pair_begin(lsdhip_ctx* c, int n, ArgPair<A, B>& p) {
  const size_t bOff = lsd_align_up(sizeof(A) * (size_t)n, 256);
  void* host = nullptr;
  if (int rc = lsd_args_begin(c, bOff + sizeof(B) * (size_t)n, &host, &p.dev)) return rc;
  p.a = (A*)host; p.b = (B*)((uint8_t*)host + bOff);
  p.devA = (const A*)p.dev; p.devB = (const B*)((const uint8_t*)p.dev + bOff);
  return LSDHIP_OK;
}
// ... and one array
template <class T> static int args_items_begin(lsdhip_ctx* c, size_t n, T** items, const T** dev) {
  void *h = nullptr, *d = nullptr;
  if (int rc = lsd_args_begin(c, sizeof(T) * n, &h, &d)) return rc;
  *items = (T*)h; *dev = (const T*)d;
  return LSDHIP_OK;
}

// The pyramids of n new frames in two launches (blockIdx.z / .y = frame).  devGray: the images where they are on the device already
// (else each frame's own uint8 plane, uploaded by the caller).  With an undistorter devGray holds raw images (never null).
static int frames_build_pyramids_batch(lsdhip_ctx* c, lsdhip_frame** fs, int n, const uint8_t* const* devGray, const lsdhip_undistorter* u = nullptr) {
  const hipStream_t ms = lsd_map_stream(c);
  ArgPair<ImagePyrItem, GradMaxArgs> args;
  if (int rc = args_pair_begin(c, n, args)) return rc;
  for (int j = 0; j < n; j++) {
    ImagePyrItem& pi = args.a[j];
    pi.gray = lsd_g(devGray ? devGray[j] : fs[j]->d_gray);
    for (int l = 0; l < LSD_LEVELS; l++) pi.img[l] = lsd_g(fs[j]->d_image[l]);
    pi.grad0 = nullptr; pi.absgrad0 = nullptr;   // keyframe planes: lsd_frames_require_level0
    args.b[j] = grad_max_args(fs[j]);
  }
  const int gradBlocks = args.b[0].blk0[LSD_LEVELS];
  if (int rc = lsd_args_commit(c, ms)) return rc;
  const int bp = lsd_bprof_begin(c, 0, ms);
  if (bp < -1) return bp;
  if (u) hipLaunchKernelGGL(k_image_pyramid_remap_batch, dim3(c->w / 16, c->h / 16, n), dim3(256), 0, ms, args.devA, (const float2*)u->d_map, u->in_w, c->w, c->h);
  else hipLaunchKernelGGL(k_image_pyramid_batch, dim3(c->w / 16, c->h / 16, n), dim3(256), 0, ms, args.devA, c->w, c->h);
  hipLaunchKernelGGL(k_gradients_max_batch, dim3(gradBlocks, n), dim3(256), 0, ms, args.devB);
  if (int rc = lsd_bprof_end(c, bp, ms, (double)n * (c->w * c->h))) return rc;
  HIPCHK(hipGetLastError());
  if (int rc = lsd_args_release(c, args.dev, ms)) return rc;
  for (int j = 0; j < n; j++) frame_pyramids_queued(fs[j]);
  return LSDHIP_OK;
}

// The frames of fs[0 .. n) that still need something, each once (null entries are skipped)
template <class Needs> static std::vector<lsdhip_frame*> frames_that_need(lsdhip_frame** fs, int n, Needs needs) {
  std::vector<lsdhip_frame*> todo;
  for (int j = 0; j < n; j++)
    if (fs[j] && needs(fs[j]) && std::find(todo.begin(), todo.end(), fs[j]) == todo.end()) todo.push_back(fs[j]);
  return todo;
}

// The depth planes of a frame and the reference blocks that go with them: the PUBLISHED set (what the tracking side reads), the set a
// Frame::setDepth WRITES (the second one on pipelined contexts, until lsd_frame_publish_depth swaps them), or the LATEST written,
// published or not
enum class DepthSet { Published, Written, Latest };
struct DepthPlaneSet { float** id; float** var; uint8_t** blk; bool* blkValid; };
static DepthPlaneSet depth_plane_set(lsdhip_frame* f, DepthSet which) {
  const bool second = which == DepthSet::Written ? f->ctx->pipeline : which == DepthSet::Latest ? f->depthPending : false;
  if (second) return {f->d_idepthW, f->d_idepthVarW, f->d_refBlkW, &f->refBlkValidW};
  return {f->d_idepth, f->d_idepthVar, f->d_refBlk, &f->refBlkValid};
}
// The record k_idepth_pyramid and k_ref_blocks (and their batch forms) read; red*: the pyramid's optional passenger
static DepthPyrArgs depth_pyr_args(lsdhip_frame* f, DepthSet which, const double* redPartials = nullptr, int redN = 0, double* redOut = nullptr) {
  const DepthPlaneSet s = depth_plane_set(f, which);
  DepthPyrArgs a;
  for (int l = 0; l < LSD_LEVELS; l++) { a.id[l] = lsd_g(s.id[l]); a.var[l] = lsd_g(s.var[l]); a.blk[l] = lsd_g(s.blk[l]); }
  a.w0 = f->ctx->w; a.h0 = f->ctx->h;
  a.redPartials = lsd_g(redPartials); a.redN = redN; a.redOut = lsd_g(redOut);
  return a;
}
static dim3 depth_pyr_grid(const lsdhip_ctx* c, bool passenger, int n) { return dim3((c->w + 31) / 32, (c->h + 31) / 32 + (passenger ? 1 : 0), n); }
// An idepth pyramid (with the reference blocks, where the context builds them) has been queued into the frame's written set
static void depth_pyramid_queued(lsdhip_frame* f) {
  lsdhip_ctx* c = f->ctx;
  *depth_plane_set(f, DepthSet::Written).blkValid = c->refBlocksWanted;
  if (c->pipeline) {
    f->depthPending = true; f->depthPendingSeq = c->mSeq + 1;   // complete at the caller's record point; the version changes when the planes are published
  } else {
    f->hasIDepth = true;
    f->depthVersion++;   // a tracking job that is topped up from here on would read the new planes (tracker.hip)
  }
}

// The reference blocks of the PUBLISHED depth planes of the keyframes of a throughput-mode tracking batch, where they are missing: a context
// builds them behind every idepth pyramid only once it has run such a batch (a single-sequence loop never reads them and does not pay the
// launch).  Queued on the caller's stream — the tracking stream, which is already ordered behind the planes.
int lsd_frames_require_ref_blocks(lsdhip_frame** kfs, int n, hipStream_t stream) {
  if (n <= 0) return LSDHIP_OK;
  lsdhip_ctx* c = kfs[0]->ctx;
  LSD_CTX_LOCK(c);
  c->refBlocksWanted = true;
  const std::vector<lsdhip_frame*> todo = frames_that_need(kfs, n, [](const lsdhip_frame* f) { return !f->refBlkValid; });
  if (todo.empty()) return LSDHIP_OK;
  DepthPyrArgs* items = nullptr;
  const DepthPyrArgs* dev = nullptr;
  if (int rc = args_items_begin(c, todo.size(), &items, &dev)) return rc;
  for (size_t j = 0; j < todo.size(); j++) items[j] = depth_pyr_args(todo[j], DepthSet::Published);
  if (int rc = lsd_args_commit(c, stream)) return rc;
  hipLaunchKernelGGL(k_ref_blocks_batch, dim3(lsd_refblk_grid(c), 1, (unsigned)todo.size()), dim3(256), 0, stream, dev);
  HIPCHK(hipGetLastError());
  if (int rc = lsd_args_release(c, dev, stream)) return rc;
  for (lsdhip_frame* f : todo) f->refBlkValid = true;
  return LSDHIP_OK;
}

// Frame::gradients(0) / Frame::maxGradients(0) on demand (the reference's Frame::require, Frame.cpp:560-640): the level-0 gradient texels,
// |grad| and its 3x3 maximum, for the frames that are asked for them — the keyframes of a DepthMap, a frame given a ground-truth depth,
// a level-0 tracking job, a download.  Queued on the mapping stream (where the consumers are; a caller on the tracking stream moves the
// frame's readySeq behind them).  One launch pair for all frames of the call that do not have the planes yet.
int lsd_frames_require_level0(lsdhip_frame** fs, int n) {
  if (n <= 0) return LSDHIP_OK;
  lsdhip_ctx* c = fs[0]->ctx;
  LSD_CTX_LOCK(c);
  const std::vector<lsdhip_frame*> todo = frames_that_need(fs, n, [](const lsdhip_frame* f) { return !f->level0Ready; });
  if (todo.empty()) return LSDHIP_OK;
  const hipStream_t ms = lsd_map_stream(c);
  const int n0 = c->w * c->h, m = (int)todo.size();
  auto fill = [&](lsdhip_frame* f, Level0Item& it, MaxCandItem& mc) {
    it.img0 = lsd_g((const float*)f->d_image[0]); it.grad0 = lsd_g(f->d_grad[0]); it.absgrad = lsd_g(f->d_absgrad);
    mc.absg = lsd_g((const float*)f->d_absgrad); mc.maxgrad = lsd_g(f->d_maxgrad); mc.cand = lsd_g(f->d_gradCand);
  };
  if (m == 1) {
    Level0Item it;
    MaxCandItem mc;
    fill(todo[0], it, mc);
    hipLaunchKernelGGL(k_level0_gradients, dim3((n0 + 255) / 256), dim3(256), 0, ms, it, c->w, c->h);
    hipLaunchKernelGGL(k_maxgrad_candidates, dim3(lsd_gradcand_groups(n0)), dim3(1024), 0, ms, mc, c->w, c->h, c->params.minUseGrad);
  } else {
    ArgPair<Level0Item, MaxCandItem> args;
    if (int rc = args_pair_begin(c, m, args)) return rc;
    for (int j = 0; j < m; j++) fill(todo[j], args.a[j], args.b[j]);
    if (int rc = lsd_args_commit(c, ms)) return rc;
    hipLaunchKernelGGL(k_level0_gradients_batch, dim3((n0 + 255) / 256, m), dim3(256), 0, ms, args.devA, c->w, c->h);
    hipLaunchKernelGGL(k_maxgrad_candidates_batch, dim3(lsd_gradcand_groups(n0), m), dim3(1024), 0, ms, args.devB, c->w, c->h, c->params.minUseGrad);
    if (int rc = lsd_args_release(c, args.dev, ms)) return rc;
  }
  HIPCHK(hipGetLastError());
  for (lsdhip_frame* f : todo) { f->level0Ready = true; f->gradCandTh = c->params.minUseGrad; }
  return LSDHIP_OK;
}
int lsd_frame_require_level0(lsdhip_frame* f) { return lsd_frames_require_level0(&f, 1); }
// ... for a consumer on the tracking stream (a level-0 tracking / Sim3 job) or the host (a download): the frame's planes are complete at a
// new point of the mapping stream
int lsd_frame_require_level0_for_tracking(lsdhip_frame* f) {
  if (f->level0Ready) return LSDHIP_OK;
  lsdhip_ctx* c = f->ctx;
  LSD_CTX_LOCK(c);
  if (int rc = lsd_m_begin(c)) return rc;
  if (int rc = lsd_frame_require_level0(f)) return rc;
  if (c->pipeline) {
    const long long seq = lsd_m_record(c);
    if (seq < 0) return LSDHIP_E_HIP;
    if (seq > f->readySeq) f->readySeq = seq;
    if (int rc = lsd_t_wait_m(c, seq)) return rc;   // (the callers have already ordered the tracking stream behind the frame's older readySeq)
  }
  return LSDHIP_OK;
}

// Frame::setDepth's second half: levels 1..4 of the planes being written, on the mapping stream.  One frame's record travels as a kernel
// argument, the records of a batch through the argument ring; everything else is the same.
int lsd_frame_build_idepth_pyramid(lsdhip_frame* f, const double* redPartials, int redN, double* redOut) {
  lsdhip_ctx* c = f->ctx;
  LSD_CTX_LOCK(c);
  const hipStream_t ms = lsd_map_stream(c);
  const DepthPyrArgs a = depth_pyr_args(f, DepthSet::Written, redPartials, redN, redOut);
  hipLaunchKernelGGL(k_idepth_pyramid, depth_pyr_grid(c, redPartials != nullptr, 1), dim3(256), 0, ms, a);
  if (c->refBlocksWanted) hipLaunchKernelGGL(k_ref_blocks, dim3(lsd_refblk_grid(c)), dim3(256), 0, ms, a);
  HIPCHK(hipGetLastError());
  depth_pyramid_queued(f);
  return LSDHIP_OK;
}
int lsd_frame_build_idepth_pyramid_batch(lsdhip_frame** fs, int n, const double* const* redPartials, int redN, double* const* redOut, const int* redNs) {
  if (n <= 0) return LSDHIP_OK;
  lsdhip_ctx* c = fs[0]->ctx;
  LSD_CTX_LOCK(c);
  const hipStream_t ms = lsd_map_stream(c);
  DepthPyrArgs* items = nullptr;
  const DepthPyrArgs* dev = nullptr;
  if (int rc = args_items_begin(c, (size_t)n, &items, &dev)) return rc;
  for (int j = 0; j < n; j++) items[j] = depth_pyr_args(fs[j], DepthSet::Written, redPartials[j], redNs ? redNs[j] : redN, redOut[j]);
  if (int rc = lsd_args_commit(c, ms)) return rc;
  hipLaunchKernelGGL(k_idepth_pyramid_batch, depth_pyr_grid(c, true, n), dim3(256), 0, ms, dev);
  if (c->refBlocksWanted) hipLaunchKernelGGL(k_ref_blocks_batch, dim3(lsd_refblk_grid(c), 1, n), dim3(256), 0, ms, dev);
  HIPCHK(hipGetLastError());
  if (int rc = lsd_args_release(c, dev, ms)) return rc;
  for (int j = 0; j < n; j++) depth_pyramid_queued(fs[j]);
  return LSDHIP_OK;
}


int lsd_frame_ensure_wasgood(lsdhip_frame* f) {
  if (!f->wasGoodValid) {
    if (!f->wasGoodPristine) HIPCHK(hipMemsetAsync(f->d_wasGood, 0xFF, (size_t)f->ctx->wl[1] * f->ctx->hl[1], f->ctx->stream));
    f->wasGoodValid = true;
  }
  f->wasGoodPristine = false;   // the caller is about to write the mask
  return LSDHIP_OK;
}

// ---- frame creation -------------------------------------------------------------------------------------------------------------------------
// The steps every creator shares, on the mapping stream: arenas, upload of host images, pyramids (two launches per frame, or — batched —
// two for all), the record point the frames are complete at, and for host images the wait after which the caller may reuse its buffers.
// gray[j] on the device is read by the pyramid kernel directly (stream-ordered; nothing else needs the uint8 plane).
// With an undistorter (lsdhip_frame_create_undistorted*) gray[j] are raw in_w x in_h images: host ones go to the undistorter's staging
// slots instead of the frames' uint8 planes, and the pyramid kernel fetches its pixels through the remap table.
static int frames_create_steps(lsdhip_ctx* c, int n, const int* ids, const uint8_t* const* gray, bool onDevice, bool batched, bool wait, lsdhip_frame** fs,
                               lsdhip_undistorter* u) {
  HIPCHK(hipSetDevice(c->device));
  for (int j = 0; j < n; j++)
    if (int rc = frame_alloc(c, ids[j], &fs[j])) return rc;
  const hipStream_t ms = lsd_map_stream(c);
  if (int rc = lsd_m_begin(c)) return rc;
  std::vector<const uint8_t*> staged;
  if (u && !onDevice) {
    staged.resize((size_t)n);
    if (int rc = undistorter_stage(u, n, gray, ms, staged.data())) return rc;
    gray = staged.data();
    onDevice = true;
  }
  if (!onDevice)
    for (int j = 0; j < n; j++) HIPCHK(hipMemcpyAsync(fs[j]->d_gray, gray[j], (size_t)c->w * c->h, hipMemcpyHostToDevice, ms));
  if (batched) {
    if (int rc = frames_build_pyramids_batch(c, fs, n, onDevice ? gray : nullptr, u)) return rc;
  } else {
    if (int rc = frame_build_pyramids(fs[0], onDevice ? gray[0] : nullptr, nullptr, u)) return rc;
    if (onDevice) lsd_trace_sum(c, ms, 2, ids[0], fs[0]->d_image[0], (size_t)((char*)fs[0]->d_idepth[0] - (char*)fs[0]->d_image[0]));
  }
  const long long seq = lsd_m_record(c);
  if (seq < 0) return LSDHIP_E_HIP;
  for (int j = 0; j < n; j++) fs[j]->readySeq = seq;
  if (wait) {
    HIPCHK(hipStreamSynchronize(ms));
    if (c->pipeline) c->mDoneSeq = c->mSeq;
  }
  return LSDHIP_OK;
}
// fs[0 .. n) null on entry; a failing call destroys the frames it made and leaves them null
static int frames_create(lsdhip_ctx* c, int n, const int* ids, const uint8_t* const* gray, bool onDevice, bool batched, bool wait, lsdhip_frame** fs,
                         lsdhip_undistorter* u = nullptr) {
  LSD_CTX_LOCK(c);
  const int rc = frames_create_steps(c, n, ids, gray, onDevice, batched, wait, fs, u);
  if (rc)
    for (int j = 0; j < n; j++) { lsdhip_frame_destroy(fs[j]); fs[j] = nullptr; }
  return rc;
}
static int frame_create_one(lsdhip_ctx* c, int id, const uint8_t* gray, bool onDevice, bool wait, lsdhip_frame** out, lsdhip_undistorter* u = nullptr) {
  if (!c || !gray || !out) return LSDHIP_E_ARG;
  lsdhip_frame* f = nullptr;
  const int rc = frames_create(c, 1, &id, &gray, onDevice, false, wait, &f, u);
  if (rc == LSDHIP_OK) *out = f;
  return rc;
}
extern "C" int lsdhip_frame_create_from_device(lsdhip_ctx* c, int id, const uint8_t* gray_dev, lsdhip_frame** out) {
  return frame_create_one(c, id, gray_dev, true, false, out);
}
extern "C" int lsdhip_frame_create(lsdhip_ctx* c, int id, const uint8_t* gray_host, lsdhip_frame** out) {
  return frame_create_one(c, id, gray_host, false, true, out);
}
extern "C" int lsdhip_frame_create_async(lsdhip_ctx* c, int id, const uint8_t* gray_host, lsdhip_frame** out) {
  return frame_create_one(c, id, gray_host, false, false, out);
}
// Frame creation for the new frames of n sequences at once: two launches for all of them instead of two per frame.  Same planes, bit
// for bit, as n lsdhip_frame_create_from_device / lsdhip_frame_create calls.
extern "C" int lsdhip_frame_create_batch(lsdhip_ctx* c, int n, const int* ids, const uint8_t* const* gray, int images_on_device, lsdhip_frame** out) {
  if (!c || n <= 0 || !ids || !gray || !out) return LSDHIP_E_ARG;
  for (int j = 0; j < n; j++) if (!gray[j]) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(c);
  if ((size_t)(2 * n + 8) > c->arena_keep) c->arena_keep = (size_t)(2 * n + 8);   // a round of n frames retires n arenas at once
  for (int j = 0; j < n; j++) out[j] = nullptr;
  return frames_create(c, n, ids, gray, images_on_device != 0, true, !images_on_device, out);
}

// ---- raw camera images: UndistorterPTAM (util/Undistorter.cpp) on the device ----------------------------------------------------------------
extern "C" int lsdhip_undistorter_create(lsdhip_ctx* c, int in_w, int in_h, const float* remapX_host, const float* remapY_host, lsdhip_undistorter** out) {
  if (!c || !remapX_host || !remapY_host || !out) return LSDHIP_E_ARG;
  if (in_w < 2 || in_h < 2 || (long long)in_w * in_h > 0x7fffffffLL) {
    lsd_set_error("lsdhip_undistorter_create: input size %dx%d", in_w, in_h);
    return LSDHIP_E_ARG;
  }
  // The kernels read four taps around every valid entry without a bounds test: the table must keep them inside the raw image
  // (Undistorter.cpp:304: 0 < ix < in_width - 1 and 0 < iy < in_height - 1, everything else is written as -1).
  const size_t n = (size_t)c->w * c->h;
  std::vector<float2> map(n);
  for (size_t i = 0; i < n; i++) {
    const float x = remapX_host[i], y = remapY_host[i];
    if (!(x < 0) && !(x >= 0 && x < (float)(in_w - 1) && y >= 0 && y < (float)(in_h - 1))) {
      lsd_set_error("lsdhip_undistorter_create: remap entry %zu = (%g, %g) is neither negative nor inside the %dx%d input image", i, (double)x, (double)y, in_w, in_h);
      return LSDHIP_E_ARG;
    }
    map[i] = make_float2(x, y);
  }
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  std::unique_ptr<lsdhip_undistorter> u(new lsdhip_undistorter());
  u->ctx = c; u->in_w = in_w; u->in_h = in_h;
  if (int rc = lsd_dev_alloc(u->d_map, n)) return rc;
  HIPCHK(hipMemcpy(u->d_map, map.data(), n * sizeof(float2), hipMemcpyHostToDevice));
  *out = u.release();
  return LSDHIP_OK;
}
extern "C" void lsdhip_undistorter_destroy(lsdhip_undistorter* u) {
  if (!u) return;
  lsdhip_ctx* c = u->ctx;
  LSD_CTX_LOCK(c);
  (void)hipSetDevice(c->device);
  (void)lsd_sync_all(c);     // frames created through it may still be queued
  if (u->stageStream) (void)hipStreamSynchronize(u->stageStream);
  delete u;
}
extern "C" int lsdhip_undistorter_apply(lsdhip_undistorter* u, const uint8_t* raw, int raw_on_device, uint8_t* out_gray, int out_on_device) {
  if (!u || !raw || !out_gray) return LSDHIP_E_ARG;
  lsdhip_ctx* c = u->ctx;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  const hipStream_t ms = lsd_map_stream(c);
  if (int rc = lsd_m_begin(c)) return rc;
  const int n = c->w * c->h;
  const uint8_t* src = raw;
  if (!raw_on_device)
    if (int rc = undistorter_stage(u, 1, &raw, ms, &src)) return rc;
  if (!out_on_device && !u->d_out) { if (int rc = lsd_dev_alloc(u->d_out, (size_t)n)) return rc; }
  uint8_t* dst = out_on_device ? out_gray : u->d_out;
  hipLaunchKernelGGL(k_undistort, dim3((n + 255) / 256), dim3(256), 0, ms, src, (const float2*)u->d_map, u->in_w, dst, n);
  HIPCHK(hipGetLastError());
  if (!out_on_device) HIPCHK(hipMemcpyAsync(out_gray, dst, (size_t)n, hipMemcpyDeviceToHost, ms));
  // host memory on either side: the caller may touch it when the call returns; device to device: queued on the mapping stream, no wait
  if (!out_on_device || !raw_on_device) HIPCHK(hipStreamSynchronize(ms));
  return LSDHIP_OK;
}
extern "C" int lsdhip_frame_create_undistorted(lsdhip_undistorter* u, int id, const uint8_t* raw_host, lsdhip_frame** out) {
  return u ? frame_create_one(u->ctx, id, raw_host, false, true, out, u) : LSDHIP_E_ARG;
}
extern "C" int lsdhip_frame_create_undistorted_async(lsdhip_undistorter* u, int id, const uint8_t* raw_host, lsdhip_frame** out) {
  return u ? frame_create_one(u->ctx, id, raw_host, false, false, out, u) : LSDHIP_E_ARG;
}
extern "C" int lsdhip_frame_create_undistorted_from_device(lsdhip_undistorter* u, int id, const uint8_t* raw_dev, lsdhip_frame** out) {
  return u ? frame_create_one(u->ctx, id, raw_dev, true, false, out, u) : LSDHIP_E_ARG;
}
extern "C" int lsdhip_frame_create_undistorted_batch(lsdhip_undistorter* u, int n, const int* ids, const uint8_t* const* raw, int images_on_device, lsdhip_frame** out) {
  if (!u || n <= 0 || !ids || !raw || !out) return LSDHIP_E_ARG;
  for (int j = 0; j < n; j++) if (!raw[j]) return LSDHIP_E_ARG;
  lsdhip_ctx* c = u->ctx;
  LSD_CTX_LOCK(c);
  if ((size_t)(2 * n + 8) > c->arena_keep) c->arena_keep = (size_t)(2 * n + 8);
  for (int j = 0; j < n; j++) out[j] = nullptr;
  return frames_create(c, n, ids, raw, images_on_device != 0, true, !images_on_device, out, u);
}
// Frame-memory pool (the reference's FrameMemory keeps returned buffers for reuse, util/... FrameMemory.cpp): make sure n arenas are
// allocated and waiting, so that a loop which keeps its keyframes alive does not pay a hipMalloc (0.5 ms for 20 MB) per keyframe.
int lsd_frames_reserve(lsdhip_ctx* c, int n) {
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  if ((size_t)n > c->arena_keep) c->arena_keep = (size_t)n;
  std::vector<lsdhip_frame*> tmp;
  int rc = LSDHIP_OK;
  for (int i = 0; i < n && rc == LSDHIP_OK; i++) {   // the pool's arenas first, the rest are new
    lsdhip_frame* f = nullptr;
    rc = frame_alloc(c, -1, &f);
    if (rc == LSDHIP_OK) tmp.push_back(f);
  }
  for (lsdhip_frame* f : tmp) lsdhip_frame_destroy(f);
  return rc;
}
extern "C" void lsdhip_frame_destroy(lsdhip_frame* f) {
  if (!f) return;
  lsdhip_ctx* c = f->ctx;
  LSD_CTX_LOCK(c);
  if (c->free_arenas.size() < c->arena_keep) {
    c->free_arenas.push_back(std::move(f->arena));   // reuse is ordered by the stream itself
  } else {
    (void)hipSetDevice(c->device);
    (void)lsd_sync_all(c);
    f->arena.reset();
  }
  if (f->pendStats >= 0) c->slot_stats_owner[f->pendStats] = nullptr;
  if (f->pendRescale >= 0) c->slot_rescale_owner[f->pendRescale] = nullptr;
  for (size_t i = 0; i < c->pendingMerges.size();)     // nobody will read this frame's mask any more
    if (c->pendingMerges[i].plane == f->d_wasGood) { *c->pendingMerges[i].doneSeq = 0; c->pendingMerges.erase(c->pendingMerges.begin() + i); }
    else i++;
  lsd_depthmaps_forget_frame(c, f);   // a depth map whose active keyframe this is becomes "no active keyframe"
  delete f;
}
extern "C" int lsdhip_frame_id(lsdhip_frame* f) { return f ? f->id : -1; }

// ---- the host reads and writes planes -----------------------------------------------------------------------------------------------------
// Before the host touches a frame's planes through the tracking stream, what the mapping side has queued for them is drained: both streams
// of a pipelined context.  A one-stream context orders everything on `stream` itself, except inside an open lane region, where the mapping
// calls go to a lane: the entries that may be called there (openLanes) wait for the lane.
static int drain_for_host(lsdhip_ctx* c, bool openLanes = false) {
  if (c->pipeline) return lsd_sync_all(c);
  if (openLanes && lsd_map_stream(c) != c->stream) HIPCHK(hipStreamSynchronize(lsd_map_stream(c)));
  return LSDHIP_OK;
}
static int copy_and_wait(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
  HIPCHK(hipMemcpyAsync(dst, src, bytes, kind, s));
  HIPCHK(hipStreamSynchronize(s));
  return LSDHIP_OK;
}

extern "C" int lsdhip_frame_download(lsdhip_frame* f, int what, int level, float* out) {
  if (!f || !out || level < 0 || level >= LSD_LEVELS) return LSDHIP_E_ARG;
  lsdhip_ctx* c = f->ctx;
  LSD_CTX_LOCK(c);
  const size_t n = (size_t)c->wl[level] * c->hl[level];
  size_t bytes = n * sizeof(float);
  const void* src = nullptr;
  if ((what == 1 && level == 0) || what == 2 || what == 6) { if (int rc = lsd_frame_require_level0_for_tracking(f)) return rc; }   // built on demand
  if (int rc = drain_for_host(c, true)) return rc;
  const bool hasDepth = f->hasIDepth || f->depthPending;
  switch (what) {
    case 0: src = f->d_image[level]; break;
    case 1: src = f->d_grad[level]; bytes *= 4; break;
    case 2: if (level != 0) return LSDHIP_E_ARG; src = f->d_maxgrad; break;
    // Frame::idepth / idepthVar: what the last Frame::setDepth left (on pipelined contexts possibly not yet published to the tracker)
    case 3: if (!hasDepth) return LSDHIP_E_STATE; src = depth_plane_set(f, DepthSet::Latest).id[level]; break;
    case 4: if (!hasDepth) return LSDHIP_E_STATE; src = depth_plane_set(f, DepthSet::Latest).var[level]; break;
    // the level's reference blocks (k_ref_blocks), as bytes: ceil(pixels / 256) x 256 offsets, then one int32 count per block — of the
    // newest planes (published or not), built here if the context has not been building them (everything is drained above)
    case 5: {
      if (!hasDepth) return LSDHIP_E_STATE;
      if (level < 1) return LSDHIP_E_ARG;
      const DepthPlaneSet s = depth_plane_set(f, DepthSet::Latest);
      if (!*s.blkValid) {
        hipLaunchKernelGGL(k_ref_blocks, dim3(lsd_refblk_grid(c)), dim3(256), 0, c->stream, depth_pyr_args(f, DepthSet::Latest));
        *s.blkValid = true;
      }
      src = s.blk[level]; bytes = lsd_refblk_bytes((int)n);
      break;
    }
    // the keyframe planes' gradient candidates (k_grad_candidates), as uint16: ceil(pixels / 1024) groups of 1024 offsets, then one count per group
    case 6: if (level != 0) return LSDHIP_E_ARG; src = f->d_gradCand; bytes = lsd_gradcand_bytes((int)n); break;
    // Frame::takeReActivationData's planes (Frame.cpp:107-145)
    case 7: case 8: case 9:
      if (level != 0) return LSDHIP_E_ARG;
      if (!f->reActValid) return LSDHIP_E_STATE;
      if (what == 7) src = f->d_idepth_reAct;
      else if (what == 8) src = f->d_idepthVar_reAct;
      else { src = f->d_validity_reAct; bytes = n; }
      break;
    default: return LSDHIP_E_ARG;
  }
  return copy_and_wait(out, src, bytes, hipMemcpyDeviceToHost, c->stream);
}

// The tail of the synchronous Frame::setDepth entries: level 0 of the written planes is queued on the mapping stream; the pyramid, the
// wait (the caller may reuse its host buffers), and on pipelined contexts the planes are visible to the tracker at once
static int set_depth_finish(lsdhip_frame* f) {
  lsdhip_ctx* c = f->ctx;
  int rc = lsd_frame_build_idepth_pyramid(f);
  HIPCHK(hipStreamSynchronize(lsd_map_stream(c)));
  if (rc == LSDHIP_OK && c->pipeline) { f->depthPendingSeq = 0; rc = lsd_frame_publish_depth(f); }
  return rc;
}
extern "C" int lsdhip_frame_set_depth_gt(lsdhip_frame* f, const float* depth_host, float cov_scale) {
  if (!f || !depth_host) return LSDHIP_E_ARG;
  lsdhip_ctx* c = f->ctx;
  LSD_CTX_LOCK(c);
  const int n0 = c->w * c->h;
  // staging plane kept by the context (ground-truth depth arrives once per keyframe in the GT-initialised modes)
  if (!c->d_gtStage) { if (int rc = lsd_dev_alloc(c->d_gtStage, (size_t)n0)) return rc; }
  if (int rc = drain_for_host(c)) return rc;
  const hipStream_t ms = lsd_map_stream(c);
  if (int rc = lsd_frame_require_level0(f)) return rc;   // Frame::setDepthFromGroundTruth reads maxGradients(0) (Frame.cpp:259)
  const DepthPlaneSet s = depth_plane_set(f, DepthSet::Written);
  HIPCHK(hipMemcpyAsync(c->d_gtStage, depth_host, (size_t)n0 * 4, hipMemcpyHostToDevice, ms));
  hipLaunchKernelGGL(k_set_depth_gt, dim3((n0 + 255) / 256), dim3(256), 0, ms, c->d_gtStage, f->d_maxgrad, s.id[0], s.var[0], c->w, c->h,
                     cov_scale, c->params.minUseGrad);
  return set_depth_finish(f);
}
extern "C" int lsdhip_frame_set_depth_planes(lsdhip_frame* f, const float* id, const float* var) {
  if (!f || !id || !var) return LSDHIP_E_ARG;
  lsdhip_ctx* c = f->ctx;
  LSD_CTX_LOCK(c);
  const size_t n0 = (size_t)c->w * c->h;
  if (int rc = drain_for_host(c)) return rc;
  const hipStream_t ms = lsd_map_stream(c);
  const DepthPlaneSet s = depth_plane_set(f, DepthSet::Written);
  HIPCHK(hipMemcpyAsync(s.id[0], id, n0 * 4, hipMemcpyHostToDevice, ms));
  HIPCHK(hipMemcpyAsync(s.var[0], var, n0 * 4, hipMemcpyHostToDevice, ms));
  return set_depth_finish(f);
}
// Test / synthetic-benchmark hook: overwrite the level-0 maxGradients plane (scene S3 of SURVEY.md §8(d) generates
// hypothesis maps and gradient masks directly, without images)
extern "C" int lsdhip_frame_set_maxgrad(lsdhip_frame* f, const float* maxgrad_host) {
  if (!f || !maxgrad_host) return LSDHIP_E_ARG;
  lsdhip_ctx* c = f->ctx;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  if (int rc = lsd_frame_require_level0_for_tracking(f)) return rc;   // (the planes count as built from here on: the overwrite below must be the last word)
  if (int rc = drain_for_host(c, true)) return rc;
  HIPCHK(hipMemcpyAsync(f->d_maxgrad, maxgrad_host, (size_t)c->w * c->h * 4, hipMemcpyHostToDevice, c->stream));
  GradCandItem gc;     // the keyframe's gradient candidates follow the plane
  gc.maxgrad = lsd_g((const float*)f->d_maxgrad); gc.cand = lsd_g(f->d_gradCand);
  hipLaunchKernelGGL(k_grad_candidates, dim3(lsd_gradcand_groups(c->w * c->h)), dim3(256), 0, c->stream, gc, c->w, c->h, c->params.minUseGrad);
  f->gradCandTh = c->params.minUseGrad;
  HIPCHK(hipStreamSynchronize(c->stream));
  return LSDHIP_OK;
}
extern "C" int lsdhip_frame_get_wasgood(lsdhip_frame* f, uint8_t* out) {
  if (!f || !out) return LSDHIP_E_ARG;
  if (!f->wasGoodValid) return 0;
  lsdhip_ctx* c = f->ctx;
  LSD_CTX_LOCK(c);
  if (int rc = drain_for_host(c)) return rc;
  if (int rc = copy_and_wait(out, f->d_wasGood, (size_t)c->wl[1] * c->hl[1], hipMemcpyDeviceToHost, c->stream)) return rc;
  return 1;
}
extern "C" int lsdhip_frame_set_wasgood(lsdhip_frame* f, const uint8_t* in) {
  if (!f || !in) return LSDHIP_E_ARG;
  lsdhip_ctx* c = f->ctx;
  LSD_CTX_LOCK(c);
  if (int rc = drain_for_host(c)) return rc;
  if (int rc = copy_and_wait(f->d_wasGood, in, (size_t)c->wl[1] * c->hl[1], hipMemcpyHostToDevice, c->stream)) return rc;
  f->wasGoodValid = true;
  f->wasGoodPristine = false;
  return LSDHIP_OK;
}
extern "C" int lsdhip_frame_clear_wasgood(lsdhip_frame* f) {
  if (!f) return LSDHIP_E_ARG;
  f->wasGoodValid = false;
  return LSDHIP_OK;
}
extern "C" int lsdhip_frame_set_pose(lsdhip_frame* f, const double s[8], lsdhip_frame* parent, float initialTrackedResidual) {
  if (!f || !s) return LSDHIP_E_ARG;
  f->thisToParent_raw.q = {s[0], s[1], s[2], s[3]};
  f->thisToParent_raw.t[0] = s[4]; f->thisToParent_raw.t[1] = s[5]; f->thisToParent_raw.t[2] = s[6];
  f->thisToParent_raw.s = s[7];
  f->trackingParent = parent;
  f->trackingParentID = parent ? parent->id : -1;
  f->initialTrackedResidual = initialTrackedResidual;
  return LSDHIP_OK;
}
extern "C" int lsdhip_frame_get_pose(lsdhip_frame* f, double s[8]) {
  if (!f || !s) return LSDHIP_E_ARG;
  { int rc = lsd_frame_resolve(f); if (rc) return rc; }   // the Sim3 scale of a new keyframe is a deferred result
  s[0] = f->thisToParent_raw.q.w; s[1] = f->thisToParent_raw.q.x; s[2] = f->thisToParent_raw.q.y; s[3] = f->thisToParent_raw.q.z;
  s[4] = f->thisToParent_raw.t[0]; s[5] = f->thisToParent_raw.t[1]; s[6] = f->thisToParent_raw.t[2];
  s[7] = f->thisToParent_raw.s;
  return LSDHIP_OK;
}
// se3FromSim3(reference->getCamToWorld().inverse() * frame->getCamToWorld()) for the two pose-tree shapes the hot path produces
// (C/SlamSystem.cpp:918-920: the initial estimate of SlamSystem::trackFrame): `frame` was tracked on `reference`, or both were tracked
// on the same parent (the frame that followed a keyframe change: tracked on the old keyframe while the mapper promoted `reference`).
extern "C" int lsdhip_frame_relative_pose(lsdhip_frame* reference, lsdhip_frame* frame, double frameToReference[7]) {
  if (!reference || !frame || !frameToReference) return LSDHIP_E_ARG;
  lsdm::Sim3dH rel;
  if (frame->trackingParent == reference && frame->trackingParentID == reference->id) {
    rel = frame->thisToParent_raw;
  } else if (frame->trackingParent && frame->trackingParent == reference->trackingParent && frame->trackingParentID == reference->trackingParentID) {
    { int rc = lsd_frame_resolve(reference); if (rc) return rc; }   // the Sim3 scale of a new keyframe is a deferred result
    const lsdm::Sim3dH inv = lsdm::sim3_inverse(reference->thisToParent_raw);
    rel.q = lsdm::q_mul(inv.q, frame->thisToParent_raw.q);
    rel.s = inv.s * frame->thisToParent_raw.s;
    double rt[3];
    lsdm::q_rotate<lsdm::Quatd, double>(inv.q, frame->thisToParent_raw.t, rt);
    for (int i = 0; i < 3; i++) rel.t[i] = inv.s * rt[i] + inv.t[i];
  } else {
    lsd_set_error("lsdhip_frame_relative_pose: frame %d and frame %d are neither parent and child nor siblings in the pose tree", reference->id, frame->id);
    return LSDHIP_E_STATE;
  }
  lsdm::q_normalize(rel.q);     // se3FromSim3 -> SO3 constructor (so3.hpp:630-633)
  frameToReference[0] = rel.q.w; frameToReference[1] = rel.q.x; frameToReference[2] = rel.q.y; frameToReference[3] = rel.q.z;
  frameToReference[4] = rel.t[0]; frameToReference[5] = rel.t[1]; frameToReference[6] = rel.t[2];
  return LSDHIP_OK;
}
extern "C" int lsdhip_frame_depth_updated(lsdhip_frame* f) { return f ? (f->depthHasBeenUpdatedFlag ? 1 : 0) : LSDHIP_E_ARG; }
extern "C" int lsdhip_frame_clear_depth_updated(lsdhip_frame* f) {
  if (!f) return LSDHIP_E_ARG;
  f->depthHasBeenUpdatedFlag = false;
  return LSDHIP_OK;
}
extern "C" int lsdhip_frame_stats(lsdhip_frame* f, float out[8]) {
  if (!f || !out) return LSDHIP_E_ARG;
  { int rc = lsd_frame_resolve(f); if (rc) return rc; }   // meanIdepth / numPoints are deferred results
  out[0] = f->initialTrackedResidual; out[1] = f->meanIdepth; out[2] = (float)f->numPoints;
  out[3] = (float)f->numFramesTrackedOnThis; out[4] = (float)f->numMappedOnThis; out[5] = (float)f->numMappedOnThisTotal;
  out[6] = f->depthHasBeenUpdatedFlag ? 1.f : 0.f; out[7] = 0.f;
  return LSDHIP_OK;
}
extern "C" int lsdhip_frame_set_counters(lsdhip_frame* f, int a, int b, int c2, int flag) {
  if (!f) return LSDHIP_E_ARG;
  f->numFramesTrackedOnThis = a; f->numMappedOnThis = b; f->numMappedOnThisTotal = c2; f->depthHasBeenUpdatedFlag = flag != 0;
  return LSDHIP_OK;
}

extern "C" int lsdhip_ref_pointcloud(lsdhip_frame* kf, int level, float* pos, float* colvar, float* grad, int* idx) {
  if (!kf || level < 0 || level >= LSD_LEVELS) { lsd_set_error("lsdhip_ref_pointcloud: bad arguments"); return LSDHIP_E_ARG; }
  if (!kf->hasIDepth) { lsd_set_error("lsdhip_ref_pointcloud: keyframe has no depth"); return LSDHIP_E_STATE; }
  lsdhip_ctx* c = kf->ctx;
  LSD_CTX_LOCK(c);
  int w = c->wl[level], h = c->hl[level];
  size_t nmax = (size_t)w * h;
  if (int rc = drain_for_host(c)) return rc;
  size_t bytes = (size_t)(w + 1) * 4 + nmax * (12 + 8 + 8 + 4) + 1024;
  LsdDev<char> scratch;
  if (int rc = lsd_dev_alloc(scratch, bytes)) return rc;
  int* d_col = (int*)scratch.get();
  int* d_total = d_col + w;
  float* d_pos = (float*)(scratch + lsd_align_up((size_t)(w + 1) * 4, 256));
  float* d_cv = d_pos + nmax * 3;
  float* d_gr = d_cv + nmax * 2;
  int* d_idx = (int*)(d_gr + nmax * 2);
  const LevelIntr& in = c->intr[level];
  hipLaunchKernelGGL(k_pc_count, dim3((w + 255) / 256), dim3(256), 0, c->stream, kf->d_idepth[level], kf->d_idepthVar[level], w, h, d_col);
  hipLaunchKernelGGL(k_pc_scan, dim3(1), dim3(64), 0, c->stream, d_col, w, d_total);
  hipLaunchKernelGGL(k_pc_write, dim3((w + 255) / 256), dim3(256), 0, c->stream, kf->d_idepth[level], kf->d_idepthVar[level],
                     kf->d_image[level], kf->d_grad[level], w, h, in.fxi, in.fyi, in.cxi, in.cyi, d_col, d_pos, d_cv, d_gr, d_idx);
  int total = 0;
  if (int rc = copy_and_wait(&total, d_total, 4, hipMemcpyDeviceToHost, c->stream)) return rc;
  if (pos) HIPCHK(hipMemcpy(pos, d_pos, (size_t)total * 12, hipMemcpyDeviceToHost));
  if (colvar) HIPCHK(hipMemcpy(colvar, d_cv, (size_t)total * 8, hipMemcpyDeviceToHost));
  if (grad) HIPCHK(hipMemcpy(grad, d_gr, (size_t)total * 8, hipMemcpyDeviceToHost));
  if (idx) HIPCHK(hipMemcpy(idx, d_idx, (size_t)total * 4, hipMemcpyDeviceToHost));
  return total;
}
