// DepthMap::debugPlotDepthMap on the device (DepthMap.cpp:1400-1428 with DepthMapPixelHypothesis::getVisualizationColor,
// DepthMapPixelHypothesis.cpp:29-90): the keyframe's level-0 image in grey with the valid hypotheses painted over it, for the reference's
// debugDisplay modes 0-5 (any other mode: every valid pixel white).  plotDepthMap of include/lsd_slam_hip_io.hpp is the yardstick: the
// kernel performs the same operations with the same promotions in the same order (-ffp-contract=off), the logarithm of modes 3 / 4 in
// double as the reference's build resolves it.  One streaming launch, blockIdx.y = map; the map is read, never written.
//
// Inputs the reference leaves undefined (a NaN, a negative variance: its byte cast of the result is undefined behaviour) are defined here,
// in the kernel and in plotDepthMap alike: white in modes 0 / 1, (0, 0, 255) in modes 3 / 4, 0 for the byte of modes 2 / 5.
#include "lsdhip_internal.hpp"

#define LSD_PLOT_MIN_BLACKLIST (-1)   // MIN_BLACKLIST, C/util/settings.h:66
#define LSD_PLOT_OTHER 6              // the kernel form of every mode outside 0 .. 5

// one map as the kernel reads it from the argument ring
struct PlotJob {
  LSD_G const uint8_t* valid;
  LSD_G const float* img;           // level-0 image of the active keyframe
  LSD_G const void* plane;          // the plane the mode colours by (float or int32; unused by LSD_PLOT_OTHER)
  LSD_G const int32_t* blacklisted; // mode 2 only
  LSD_G uint8_t* out;               // w * h * 3 bytes
  int refID;                        // referenceFrameByID_offset (mode 5)
};

// ---- device ---------------------------------------------------------------------------------------------------------------------------
// a colour as byte0 | byte1 << 8 | byte2 << 16, bytes in the order of the reference's cv::Vec3b
__device__ __forceinline__ unsigned plot_rgb(unsigned c0, unsigned c1, unsigned c2) { return c0 | (c1 << 8) | (c2 << 16); }
// `uchar v = f < 0 ? 0 : (f > 255 ? 255 : f)`: clamp, then truncate
__device__ __forceinline__ unsigned plot_clamp_byte(float f) { return !(f > 0.f) ? 0u : (f > 255.f ? 255u : (unsigned)(int)f); }

// getVisualizationColor for one hypothesis; `bits` is the 32-bit value of the mode's plane
template <int MODE>
__device__ __forceinline__ unsigned plot_color(unsigned bits, int refID) {
  if (MODE == 0 || MODE == 1) {
    const float id = __uint_as_float(bits);
    if (!(id >= 0.f)) return 0xFFFFFFu;
    // rainbow between 0 and 4
    const unsigned rc = plot_clamp_byte(fabsf((0.f - id) * 255.f)), gc = plot_clamp_byte(fabsf((1.f - id) * 255.f)), bc = plot_clamp_byte(fabsf((2.f - id) * 255.f));
    return plot_rgb(255u - rc, 255u - gc, 255u - bc);
  }
  if (MODE == 2) {
    const float f = (float)((double)(int)bits * (255.0 / (250.0f + 5.0f)));   // VALIDITY_COUNTER_MAX_VARIABLE + VALIDITY_COUNTER_MAX
    const unsigned v = plot_clamp_byte(f);
    return plot_rgb(0u, v, v);
  }
  if (MODE == 3 || MODE == 4) {
    const float idv = __uint_as_float(bits);
    float var = (float)(-0.5 * (idv == 1.0f ? 0.0 : log10((double)idv)));   // (log10(1) is exactly 0, whatever the library's last bits)
    var = (float)((double)(var * 255.f) * 0.333);
    if (var > 255.f) var = 255.f;
    if (!(var >= 0.f)) return plot_rgb(0u, 0u, 255u);
    return plot_rgb((unsigned)(int)(255.f - var), (unsigned)(int)var, 0u);
  }
  if (MODE == 5) {
    const float f = (float)((double)(__uint_as_float(bits) - (float)refID) * (255.0 / 100));
    const unsigned v = plot_clamp_byte(f);
    return plot_rgb(v, 0u, v);
  }
  return 0xFFFFFFu;
}

// cv::Mat::convertTo(CV_8UC1) of a float: round to nearest even, then clamp to 0 .. 255
__device__ __forceinline__ unsigned plot_grey(float g) {
  const int r = __float2int_rn(g);
  const unsigned b = (unsigned)(r < 0 ? 0 : (r > 255 ? 255 : r));
  return b * 0x010101u;
}

// 4 consecutive pixels per lane (w * h is a multiple of 256): validity one 4-byte load, image and the mode's plane one 16-byte load each,
// the 12 output bytes one store
template <int MODE>
__global__ __launch_bounds__(256) void k_depth_plot(const PlotJob* __restrict__ jobs, int npix) {
  const PlotJob& J = jobs[blockIdx.y];
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q * 4 >= npix) return;
  const unsigned v4 = ((LSD_G const unsigned*)J.valid)[q];
  const float4 g4 = ((LSD_G const float4*)J.img)[q];
  uint4 p4 = make_uint4(0u, 0u, 0u, 0u);
  if (MODE != LSD_PLOT_OTHER) p4 = ((LSD_G const uint4*)J.plane)[q];
  int4 b4 = make_int4(0, 0, 0, 0);
  if (MODE == 2) b4 = ((LSD_G const int4*)J.blacklisted)[q];
  const float gk[4] = {g4.x, g4.y, g4.z, g4.w};
  const unsigned pk[4] = {p4.x, p4.y, p4.z, p4.w};
  const int bk[4] = {b4.x, b4.y, b4.z, b4.w};
  const int refID = J.refID;
  unsigned c[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    c[k] = plot_grey(gk[k]);
    if (MODE == 2 && bk[k] < LSD_PLOT_MIN_BLACKLIST) c[k] = plot_rgb(0u, 0u, 255u);
    const unsigned col = plot_color<MODE>(pk[k], refID);      // (for every pixel, selected below: the plane's 16 bytes stay one load)
    c[k] = ((v4 >> (8 * k)) & 0xFFu) ? col : c[k];
  }
  uint3 o;
  o.x = c[0] | (c[1] << 24);
  o.y = (c[1] >> 8) | (c[2] << 16);
  o.z = (c[2] >> 16) | (c[3] << 8);
  ((LSD_G uint3*)J.out)[q] = o;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
static LSD_G const void* plot_plane(const HypPlanes& m, int mode) {
  switch (mode) {
    case 0: return (LSD_G const void*)m.idepth_s;
    case 1: return (LSD_G const void*)m.idepth;
    case 2: return (LSD_G const void*)m.validity;
    case 3: return (LSD_G const void*)m.var_s;
    case 4: return (LSD_G const void*)m.var;
    case 5: return (LSD_G const void*)m.nextID;
    default: return nullptr;
  }
}

// one launch for the n maps (of context c, each with an active keyframe) on the mapping stream; outs[j]: device memory, 4-byte aligned
static int plot_launch(lsdhip_ctx* c, int n, lsdhip_depthmap* const* maps, int debugDisplay, uint8_t* const* outs) {
  HIPCHK(hipSetDevice(c->device));
  if (int rcb = lsd_m_begin(c)) return rcb;
  const hipStream_t ms = lsd_map_stream(c);
  void* hostRec = nullptr;
  void* devRec = nullptr;
  if (int rc = lsd_args_begin(c, sizeof(PlotJob) * (size_t)n, &hostRec, &devRec)) return rc;
  PlotJob* jobs = (PlotJob*)hostRec;
  for (int j = 0; j < n; j++) {
    const lsdhip_depthmap* dm = maps[j];
    PlotJob& J = jobs[j];
    J.valid = dm->cur.valid;
    J.img = lsd_g((const float*)dm->activeKeyFrame->d_image[0]);
    J.plane = plot_plane(dm->cur, debugDisplay);
    J.blacklisted = dm->cur.blacklisted;
    J.out = lsd_g(outs[j]);
    J.refID = dm->referenceFrameByIDOffset;
  }
  if (int rc = lsd_args_commit(c, ms)) return rc;
  const int npix = c->w * c->h;
  const dim3 grid((npix / 4 + 255) / 256, n), block(256);
  const PlotJob* dj = (const PlotJob*)devRec;
  switch (debugDisplay) {
    case 0: hipLaunchKernelGGL(k_depth_plot<0>, grid, block, 0, ms, dj, npix); break;
    case 1: hipLaunchKernelGGL(k_depth_plot<1>, grid, block, 0, ms, dj, npix); break;
    case 2: hipLaunchKernelGGL(k_depth_plot<2>, grid, block, 0, ms, dj, npix); break;
    case 3: hipLaunchKernelGGL(k_depth_plot<3>, grid, block, 0, ms, dj, npix); break;
    case 4: hipLaunchKernelGGL(k_depth_plot<4>, grid, block, 0, ms, dj, npix); break;
    case 5: hipLaunchKernelGGL(k_depth_plot<5>, grid, block, 0, ms, dj, npix); break;
    default: hipLaunchKernelGGL(k_depth_plot<LSD_PLOT_OTHER>, grid, block, 0, ms, dj, npix); break;
  }
  HIPCHK(hipGetLastError());
  return lsd_args_release(c, devRec, ms);
}

extern "C" int lsdhip_depth_debug_plot_batch(int n, lsdhip_depthmap** maps, int debugDisplay, uint8_t* const* out_dev) {
  if (n <= 0 || !maps || !out_dev) return LSDHIP_E_ARG;
  for (int j = 0; j < n; j++) if (!maps[j] || !out_dev[j] || ((uintptr_t)out_dev[j] & 3)) return LSDHIP_E_ARG;
  lsdhip_ctx* c = maps[0]->ctx;
  LSD_CTX_LOCK(c);
  for (int j = 0; j < n; j++) {
    if (maps[j]->ctx != c) { lsd_set_error("debugPlotDepthMap batch: the maps of one batch live on one context"); return LSDHIP_E_ARG; }
    if (!maps[j]->activeKeyFrame) { lsd_set_error("debugPlotDepthMap: depth map %d has no active keyframe", j); return LSDHIP_E_STATE; }
  }
  return plot_launch(c, n, maps, debugDisplay, out_dev);
}

extern "C" int lsdhip_depth_debug_plot_dev(lsdhip_depthmap* dm, int debugDisplay, uint8_t* out_dev) {
  if (!dm || !out_dev) return LSDHIP_E_ARG;
  return lsdhip_depth_debug_plot_batch(1, &dm, debugDisplay, &out_dev);
}

extern "C" int lsdhip_depth_debug_plot(lsdhip_depthmap* dm, int debugDisplay, uint8_t* out_host) {
  if (!dm || !out_host) return LSDHIP_E_ARG;
  lsdhip_ctx* c = dm->ctx;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  const size_t bytes = (size_t)c->w * c->h * 3;
  if (!c->d_plotStage) { if (int rc = lsd_dev_alloc(c->d_plotStage, bytes)) return rc; }
  if (int rc = lsdhip_depth_debug_plot_dev(dm, debugDisplay, c->d_plotStage)) return rc;
  const hipStream_t ms = lsd_map_stream(c);
  HIPCHK(hipMemcpyAsync(out_host, c->d_plotStage, bytes, hipMemcpyDeviceToHost, ms));
  HIPCHK(hipStreamSynchronize(ms));
  return LSDHIP_OK;
}
