// Keyframe export on the device: the keyframeMsg payload (InputPointDense, V/KeyFrameDisplay.h:39-44, filled as
// C/IOWrapper/ROS/ROSOutput3DWrapper.cpp:70-111) and the viewer's point cloud (KeyFrameDisplay::flushPC, V/KeyFrameDisplay.cpp:269-340)
// from the planes a finalised keyframe already holds in HBM.  The host functions of include/lsd_slam_hip_io.hpp (makeKeyframeMsg,
// flushPointCloud) are the yardstick: the kernels perform the same single-precision operations in the same order (-ffp-contract=off:
// every multiply and add rounded on its own), so both sides agree bit for bit.
//
// Cloud append = count -> scan -> write over chunks of 1024 consecutive pixels (4 per lane), blockIdx.y = job:
//   k_cloud_count  the filters of flushPC per pixel -> a 4-bit keep mask per lane (one byte) and one count per chunk
//   k_cloud_scan   exclusive scan of the chunk counts, based on the cloud's device-resident running total; appends the segment
//                  (frame id, first, count) and advances the total — consecutive appends chain in stream order, the host sees no count
//   k_cloud_write  back-projection of the kept pixels to their slots: row-major pixel order within a keyframe, keyframes in call order
// No atomics, no arrival order anywhere: the output is identical from run to run.
#include "lsdhip_internal.hpp"
#include "block_scan.hpp"   // lsd_block_excl_scan: the ordered compaction's scan inside a workgroup
#include "../../include/lsd_slam_hip_cloud_constants.hpp"   // cloudConstants: the per-keyframe constants, the one expression set both paths use

#define LSD_CLOUD_CHUNK 1024

struct CloudState { long long total; int nseg; int unrecorded; };   // points appended so far (also beyond the capacity), segments recorded, keyframes without a row
struct CloudSeg { int id; int count; long long first; };

// one append job as the kernels read it from the argument ring
struct CloudJob {
  LSD_G const float* img;      // level-0 image plane
  LSD_G const float* id;       // lsd_depth_latest(f)[0]
  LSD_G const float* var;      // lsd_depthvar_latest(f)[0]
  LSD_G uint8_t* mask;         // per lane of a chunk: keep bits of its 4 pixels
  LSD_G int* chunkCount;
  LSD_G long long* chunkOff;   // absolute slot of the chunk's first kept point
  LSD_G CloudState* state;
  LSD_G CloudSeg* segs;
  LSD_G float4* pts;
  long long capacity;
  int maxSeg, frameId;
  float fxi, fyi, cxi, cyi, scale, ux, uy, uz, uw, tx, ty, tz;
};

struct lsdhip_cloud {
  lsdhip_ctx* ctx = nullptr;
  long long capacity = 0;
  int maxSeg = 0;
  int nchunks = 0;
  int appended = 0;            // appends queued since creation / the last reset (each takes one segment row while there is room)
  LsdDev<char> base;           // one allocation: points (+ guard) | state | segments | mask | chunk counts | chunk offsets
  float4* d_pts = nullptr;
  CloudState* d_state = nullptr;
  CloudSeg* d_segs = nullptr;
  uint8_t* d_mask = nullptr;
  int* d_chunkCount = nullptr;
  long long* d_chunkOff = nullptr;
};

// ---- device ---------------------------------------------------------------------------------------------------------------------------
// flushPC's filters (V/KeyFrameDisplay.cpp:286-318) for the 4 pixels of a lane
__global__ __launch_bounds__(256) void k_cloud_count(const CloudJob* __restrict__ jobs, int w, int h, float scaledTH, float absTH, int minNearSupport) {
  __shared__ int lds[4];
  const CloudJob& J = jobs[blockIdx.y];
  const int npix = w * h;
  const int i0 = blockIdx.x * LSD_CLOUD_CHUNK + threadIdx.x * 4;
  unsigned keep = 0;
  if (i0 < npix) {
    const int y = i0 / w, x0 = i0 - y * w;      // w is a multiple of 16: the 4 pixels lie in one row
    if (y >= 1 && y < h - 1) {
      const float4 c4 = *(LSD_G const float4*)(J.id + i0);
      const float4 v4 = *(LSD_G const float4*)(J.var + i0);
      const float idc[4] = {c4.x, c4.y, c4.z, c4.w}, vc[4] = {v4.x, v4.y, v4.z, v4.w};
      const float scale = J.scale;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int x = x0 + k;
        if (x < 1 || x > w - 2 || idc[k] <= 0.f) continue;
        const float depth = lsd_rcp_exact(idc[k]);
        float depth4 = depth * depth;
        depth4 *= depth4;
        if (vc[k] * depth4 > scaledTH) continue;
        if (vc[k] * depth4 * scale * scale > absTH) continue;
        keep |= 1u << k;
      }
      if (keep && minNearSupport > 1) {
        // rows y - 1 .. y + 1, columns x0 - 1 .. x0 + 4: the 3x3 neighbourhoods of the lane's pixels (a candidate's are inside the image)
        float win[3][6];
#pragma unroll
        for (int r = 0; r < 3; r++) {
          LSD_G const float* row = J.id + (i0 + (r - 1) * w);
          const float4 m4 = r == 1 ? c4 : *(LSD_G const float4*)row;
          win[r][0] = x0 >= 1 ? row[-1] : 0.f;
          win[r][1] = m4.x; win[r][2] = m4.y; win[r][3] = m4.z; win[r][4] = m4.w;
          win[r][5] = x0 + 4 < w ? row[4] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
          if (!(keep & (1u << k))) continue;
          const float depth = lsd_rcp_exact(idc[k]);
          const float ref = lsd_rcp_exact(depth);     // 1.0f / depth: not idepth again
          const float twoVar = 2.f * vc[k];
          int nearSupport = 0;
#pragma unroll
          for (int r = 0; r < 3; r++)
#pragma unroll
            for (int dx = 0; dx < 3; dx++) {
              const float q = win[r][k + dx];
              if (q > 0.f) {
                const float diff = q - ref;
                if (diff * diff < twoVar) nearSupport++;
              }
            }
          if (nearSupport < minNearSupport) keep &= ~(1u << k);
        }
      }
    }
  }
  J.mask[blockIdx.x * 256 + threadIdx.x] = (uint8_t)keep;
  int total;
  (void)lsd_block_excl_scan(__popc(keep), &total, lds);
  if (threadIdx.x == 0) J.chunkCount[blockIdx.x] = total;
}

// one workgroup per job: chunk offsets from the running total, the segment row, the new total
__global__ __launch_bounds__(256) void k_cloud_scan(const CloudJob* __restrict__ jobs, int nchunks) {
  __shared__ int lds[4];
  const CloudJob& J = jobs[blockIdx.y];
  const long long first = J.state->total;
  int carry = 0;
  for (int c0 = 0; c0 < nchunks; c0 += 256) {
    const int c = c0 + (int)threadIdx.x;
    const int v = c < nchunks ? J.chunkCount[c] : 0;
    int tot;
    const int ex = lsd_block_excl_scan(v, &tot, lds);
    if (c < nchunks) J.chunkOff[c] = first + (long long)(carry + ex);
    carry += tot;
  }
  if (threadIdx.x == 0) {     // (every lane has read `total` before the first barrier above)
    const int ns = J.state->nseg;
    if (ns < J.maxSeg) {
      CloudSeg s;
      s.id = J.frameId; s.count = carry; s.first = first;
      J.segs[ns] = s;
      J.state->nseg = ns + 1;
    } else {
      J.state->unrecorded = J.state->unrecorded + 1;
    }
    J.state->total = first + (long long)carry;
  }
}

// flushPC's back-projection (V/KeyFrameDisplay.cpp:320-332) of the kept pixels, in pixel order; point i is stored iff i < capacity
__global__ __launch_bounds__(256) void k_cloud_write(const CloudJob* __restrict__ jobs, int w, int h) {
  __shared__ int lds[4];
  const CloudJob& J = jobs[blockIdx.y];
  if (J.chunkCount[blockIdx.x] == 0) return;
  const long long chunkFirst = J.chunkOff[blockIdx.x];
  if (chunkFirst >= J.capacity) return;
  const unsigned keep = J.mask[blockIdx.x * 256 + threadIdx.x];
  int total;
  const int ex = lsd_block_excl_scan(__popc(keep), &total, lds);
  if (!keep) return;
  const int i0 = blockIdx.x * LSD_CLOUD_CHUNK + threadIdx.x * 4;
  const int y = i0 / w, x0 = i0 - y * w;
  const float4 c4 = *(LSD_G const float4*)(J.id + i0);
  const float4 g4 = *(LSD_G const float4*)(J.img + i0);
  const float idc[4] = {c4.x, c4.y, c4.z, c4.w}, gc[4] = {g4.x, g4.y, g4.z, g4.w};
  const float scale = J.scale, ux = J.ux, uy = J.uy, uz = J.uz, uw = J.uw;
  long long slot = chunkFirst + ex;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (!(keep & (1u << k))) continue;
    if (slot < J.capacity) {
      const int x = x0 + k;
      const float depth = lsd_rcp_exact(idc[k]);
      const float v0 = ((float)x * J.fxi + J.cxi) * depth * scale, v1 = ((float)y * J.fyi + J.cyi) * depth * scale, v2 = depth * scale;
      const float tx = 2.f * (uy * v2 - uz * v1), ty = 2.f * (uz * v0 - ux * v2), tz = 2.f * (ux * v1 - uy * v0);
      float4 p;
      p.x = v0 + uw * tx + (uy * tz - uz * ty) + J.tx;
      p.y = v1 + uw * ty + (uz * tx - ux * tz) + J.ty;
      p.z = v2 + uw * tz + (ux * ty - uy * tx) + J.tz;
      p.w = (float)(int)(unsigned char)gc[k] / 255.0f;
      J.pts[slot] = p;
    }
    slot++;
  }
}

// publishKeyframe's fill loop (C/IOWrapper/ROS/ROSOutput3DWrapper.cpp:92-104): 12 bytes per pixel, 4 pixels = three 16-byte stores per lane
__global__ __launch_bounds__(256) void k_pack_keyframe_points(const float* __restrict__ id, const float* __restrict__ var, const float* __restrict__ img,
                                                               uint4* __restrict__ out, int npix) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q * 4 >= npix) return;
  const float4 a = ((const float4*)id)[q], v = ((const float4*)var)[q], g = ((const float4*)img)[q];
  const unsigned c0 = (unsigned)(unsigned char)g.x * 0x01010101u, c1 = (unsigned)(unsigned char)g.y * 0x01010101u;
  const unsigned c2 = (unsigned)(unsigned char)g.z * 0x01010101u, c3 = (unsigned)(unsigned char)g.w * 0x01010101u;
  out[3 * q + 0] = make_uint4(__float_as_uint(a.x), __float_as_uint(v.x), c0, __float_as_uint(a.y));
  out[3 * q + 1] = make_uint4(__float_as_uint(v.y), c1, __float_as_uint(a.z), __float_as_uint(v.z));
  out[3 * q + 2] = make_uint4(c2, __float_as_uint(a.w), __float_as_uint(v.w), c3);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
static size_t cloud_align(size_t v) { return (v + 255) / 256 * 256; }

extern "C" int lsdhip_frame_pack_keyframe_points(lsdhip_frame* f, uint8_t* out_host) {
  if (!f || !out_host) return LSDHIP_E_ARG;
  lsdhip_ctx* c = f->ctx;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  if (!f->hasIDepth && !f->depthPending) { lsd_set_error("lsdhip_frame_pack_keyframe_points: frame %d has no depth", f->id); return LSDHIP_E_STATE; }
  const int npix = c->w * c->h;
  if (!c->d_kfPoints) { if (int rc = lsd_dev_alloc(c->d_kfPoints, (size_t)npix * 12)) return rc; }
  if (c->pipeline) { if (int rc = lsd_sync_all(c)) return rc; }
  else if (lsd_map_stream(c) != c->stream) HIPCHK(hipStreamSynchronize(lsd_map_stream(c)));   // (an open lane region)
  hipLaunchKernelGGL(k_pack_keyframe_points, dim3((npix / 4 + 255) / 256), dim3(256), 0, c->stream, (const float*)lsd_depth_latest(f)[0],
                     (const float*)lsd_depthvar_latest(f)[0], (const float*)f->d_image[0], (uint4*)c->d_kfPoints.get(), npix);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out_host, c->d_kfPoints, (size_t)npix * 12, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return LSDHIP_OK;
}

extern "C" int lsdhip_cloud_create(lsdhip_ctx* c, int64_t capacity_points, int max_keyframes, lsdhip_cloud** out) {
  if (!c || !out || capacity_points < 0 || max_keyframes <= 0) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  std::unique_ptr<lsdhip_cloud> q(new lsdhip_cloud());
  q->ctx = c;
  q->capacity = capacity_points;
  q->maxSeg = max_keyframes;
  q->nchunks = (c->w * c->h + LSD_CLOUD_CHUNK - 1) / LSD_CLOUD_CHUNK;
  size_t off = 0, offs[6];
  int k = 0;
  auto take = [&](size_t bytes) { off = cloud_align(off); offs[k++] = off; off += bytes; };
  take(((size_t)capacity_points + LSDHIP_CLOUD_GUARD_POINTS) * sizeof(float4));
  take(sizeof(CloudState));
  take((size_t)max_keyframes * sizeof(CloudSeg));
  take((size_t)q->nchunks * 256);
  take((size_t)q->nchunks * sizeof(int));
  take((size_t)q->nchunks * sizeof(long long));
  if (int rc = lsd_dev_alloc(q->base, cloud_align(off))) return rc;
  q->d_pts = (float4*)(q->base + offs[0]);
  q->d_state = (CloudState*)(q->base + offs[1]);
  q->d_segs = (CloudSeg*)(q->base + offs[2]);
  q->d_mask = (uint8_t*)(q->base + offs[3]);
  q->d_chunkCount = (int*)(q->base + offs[4]);
  q->d_chunkOff = (long long*)(q->base + offs[5]);
  const hipStream_t ms = lsd_map_stream(c);
  // the guard behind the buffer keeps this fill for the life of the cloud: nothing is ever written beyond `capacity`
  HIPCHK(hipMemsetAsync(q->d_pts + capacity_points, 0xFF, (size_t)LSDHIP_CLOUD_GUARD_POINTS * sizeof(float4), ms));
  HIPCHK(hipMemsetAsync(q->d_state, 0, sizeof(CloudState), ms));
  *out = q.release();
  return LSDHIP_OK;
}

extern "C" void lsdhip_cloud_destroy(lsdhip_cloud* q) {
  if (!q) return;
  lsdhip_ctx* c = q->ctx;
  LSD_CTX_LOCK(c);
  (void)hipSetDevice(c->device);
  (void)lsd_sync_all(c);      // appends still queued read and write the allocation
  delete q;
}

extern "C" int lsdhip_cloud_reset(lsdhip_cloud* q) {
  if (!q) return LSDHIP_E_ARG;
  lsdhip_ctx* c = q->ctx;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemsetAsync(q->d_state, 0, sizeof(CloudState), lsd_map_stream(c)));   // stream-ordered behind the appends queued so far
  q->appended = 0;
  return LSDHIP_OK;
}

extern "C" int lsdhip_cloud_append_batch(lsdhip_ctx* c, int n, lsdhip_cloud** clouds, lsdhip_frame** frames, const float* poses, float scaledTH,
                                         float absTH, int minNearSupport) {
  if (!c || n <= 0 || !clouds || !frames || !poses) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(c);
  for (int j = 0; j < n; j++) {
    if (!clouds[j] || !frames[j] || clouds[j]->ctx != c || frames[j]->ctx != c) { lsd_set_error("lsdhip_cloud_append_batch: job %d: null handle or another context's", j); return LSDHIP_E_ARG; }
    for (int i = 0; i < j; i++)
      if (clouds[i] == clouds[j]) { lsd_set_error("lsdhip_cloud_append_batch: jobs %d and %d name one cloud", i, j); return LSDHIP_E_ARG; }
  }
  for (int j = 0; j < n; j++)
    if (!frames[j]->hasIDepth && !frames[j]->depthPending) { lsd_set_error("lsdhip_cloud_append_batch: frame %d has no depth", frames[j]->id); return LSDHIP_E_STATE; }
  HIPCHK(hipSetDevice(c->device));
  const hipStream_t ms = lsd_map_stream(c);
  void* hostRec = nullptr;
  void* devRec = nullptr;
  if (int rc = lsd_args_begin(c, sizeof(CloudJob) * (size_t)n, &hostRec, &devRec)) return rc;
  CloudJob* jobs = (CloudJob*)hostRec;
  const LevelIntr& K = c->intr[0];
  for (int j = 0; j < n; j++) {
    lsdhip_cloud* q = clouds[j];
    lsdhip_frame* f = frames[j];
    const lsd_slam_hip::CloudConstants k = lsd_slam_hip::cloudConstants(K.fx, K.fy, K.cx, K.cy, poses + 7 * j);
    CloudJob& J = jobs[j];
    J.img = lsd_g((const float*)f->d_image[0]);
    J.id = lsd_g((const float*)lsd_depth_latest(f)[0]);
    J.var = lsd_g((const float*)lsd_depthvar_latest(f)[0]);
    J.mask = lsd_g(q->d_mask); J.chunkCount = lsd_g(q->d_chunkCount); J.chunkOff = lsd_g(q->d_chunkOff);
    J.state = lsd_g(q->d_state); J.segs = lsd_g(q->d_segs); J.pts = lsd_g(q->d_pts);
    J.capacity = q->capacity; J.maxSeg = q->maxSeg; J.frameId = f->id;
    J.fxi = k.fxi; J.fyi = k.fyi; J.cxi = k.cxi; J.cyi = k.cyi; J.scale = k.scale;
    J.ux = k.ux; J.uy = k.uy; J.uz = k.uz; J.uw = k.uw; J.tx = k.tx; J.ty = k.ty; J.tz = k.tz;
  }
  if (int rc = lsd_args_commit(c, ms)) return rc;
  const int nchunks = clouds[0]->nchunks;
  const CloudJob* dj = (const CloudJob*)devRec;
  hipLaunchKernelGGL(k_cloud_count, dim3(nchunks, n), dim3(256), 0, ms, dj, c->w, c->h, scaledTH, absTH, minNearSupport);
  hipLaunchKernelGGL(k_cloud_scan, dim3(1, n), dim3(256), 0, ms, dj, nchunks);
  hipLaunchKernelGGL(k_cloud_write, dim3(nchunks, n), dim3(256), 0, ms, dj, c->w, c->h);
  HIPCHK(hipGetLastError());
  if (int rc = lsd_args_release(c, devRec, ms)) return rc;
  int full = 0;
  for (int j = 0; j < n; j++) {
    clouds[j]->appended++;
    if (clouds[j]->appended >= clouds[j]->maxSeg) full = 1;
  }
  return full ? LSDHIP_CLOUD_TABLE_FULL : LSDHIP_OK;
}

extern "C" int lsdhip_cloud_append_keyframe(lsdhip_cloud* q, lsdhip_frame* f, const float camToWorld[7], float scaledTH, float absTH,
                                            int minNearSupport) {
  if (!q || !f || !camToWorld) return LSDHIP_E_ARG;
  return lsdhip_cloud_append_batch(q->ctx, 1, &q, &f, camToWorld, scaledTH, absTH, minNearSupport);
}

static int cloud_read_state(lsdhip_cloud* q, CloudState* st) {
  lsdhip_ctx* c = q->ctx;
  HIPCHK(hipSetDevice(c->device));
  const hipStream_t ms = lsd_map_stream(c);
  HIPCHK(hipMemcpyAsync(st, q->d_state, sizeof(CloudState), hipMemcpyDeviceToHost, ms));
  HIPCHK(hipStreamSynchronize(ms));
  return LSDHIP_OK;
}

extern "C" int lsdhip_cloud_count(lsdhip_cloud* q, int64_t* total, int64_t* stored) {
  if (!q) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(q->ctx);
  CloudState st;
  if (int rc = cloud_read_state(q, &st)) return rc;
  if (total) *total = st.total;
  if (stored) *stored = st.total < q->capacity ? st.total : q->capacity;
  return LSDHIP_OK;
}

extern "C" int lsdhip_cloud_segments(lsdhip_cloud* q, int max, int* ids, int64_t* first, int* count, int* n) {
  if (!q || max < 0 || !n) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(q->ctx);
  CloudState st;
  if (int rc = cloud_read_state(q, &st)) return rc;
  *n = st.nseg;
  const int rows = st.nseg < max ? st.nseg : max;       // only the rows the caller takes travel
  if (rows <= 0) return LSDHIP_OK;
  std::vector<CloudSeg> segs((size_t)rows);
  const hipStream_t ms = lsd_map_stream(q->ctx);
  HIPCHK(hipMemcpyAsync(segs.data(), q->d_segs, sizeof(CloudSeg) * (size_t)rows, hipMemcpyDeviceToHost, ms));
  HIPCHK(hipStreamSynchronize(ms));
  for (int i = 0; i < rows; i++) {
    if (ids) ids[i] = segs[i].id;
    if (first) first[i] = segs[i].first;
    if (count) count[i] = segs[i].count;
  }
  return LSDHIP_OK;
}

extern "C" int lsdhip_cloud_download(lsdhip_cloud* q, int64_t first, int64_t n, float* xyzi_host) {
  if (!q || first < 0 || n < 0 || first + n > q->capacity + LSDHIP_CLOUD_GUARD_POINTS || (n > 0 && !xyzi_host)) return LSDHIP_E_ARG;
  lsdhip_ctx* c = q->ctx;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  const hipStream_t ms = lsd_map_stream(c);
  if (n > 0) HIPCHK(hipMemcpyAsync(xyzi_host, q->d_pts + first, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost, ms));
  HIPCHK(hipStreamSynchronize(ms));
  return LSDHIP_OK;
}
