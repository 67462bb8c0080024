// The keyframe bank: what Frame::setPermaRef (C/DataStructures/Frame.cpp:149-174) keeps per keyframe in host
// vectors — the level-QUICK_KF_CHECK_LVL point cloud of TrackingReference::makePointCloud (C/Tracking/TrackingReference.cpp:96-147) —
// resident in device memory for every keyframe, so that TrackableKeyFrameSearch::findRePositionCandidate
// (C/GlobalMapping/TrackableKeyFrameSearch.cpp:103-172; tracker.hip: lsdhip_tracker_find_reposition_candidate) reads all candidates where
// they lie.  lsdhip_ref_pointcloud (frame.hip: k_pc_count / k_pc_scan / k_pc_write) is the yardstick: k_kfbank_put applies the same test
// and the same single-precision expressions per point (-ffp-contract=off), so both clouds agree bit for bit.
#include "lsdhip_internal.hpp"
#include "block_scan.hpp"

// makePointCloud's loop (TrackingReference.cpp:112-144) for one level in ONE workgroup: lane = column (x outer), rows inside the lane
// (y inner).  Per 256 columns: the lanes count their columns' points, an exclusive scan over the workgroup turns the counts into the
// columns' first slots, the lanes write their points in row order.  No atomics: point i of the cloud is point i of the reference's.
__global__ __launch_bounds__(256) void k_kfbank_put(const float* __restrict__ id, const float* __restrict__ var, const float* __restrict__ img, int w, int h,
                                                    float fxi, float fyi, float cxi, float cyi, float* __restrict__ pos, float* __restrict__ colvar,
                                                    int* __restrict__ count) {
  __shared__ int lds[4];
  int carry = 0;
  for (int x0 = 0; x0 < w; x0 += 256) {
    const int x = x0 + (int)threadIdx.x;
    const bool inside = x >= 1 && x < w - 1;
    int c = 0;
    if (inside)
      for (int y = 1; y < h - 1; y++) {
        const int idx = x + y * w;
        if (!(var[idx] <= 0 || id[idx] == 0)) c++;
      }
    int total;
    int n = carry + lsd_block_excl_scan(c, &total, lds);
    if (c > 0)
      for (int y = 1; y < h - 1; y++) {
        const int idx = x + y * w;
        const float v = var[idx], d = id[idx];
        if (v <= 0 || d == 0) continue;
        const float inv = 1.0f / d;
        pos[3 * n + 0] = inv * (fxi * x + cxi);
        pos[3 * n + 1] = inv * (fyi * y + cyi);
        pos[3 * n + 2] = inv * 1.0f;
        colvar[2 * n + 0] = img[idx];
        colvar[2 * n + 1] = v;
        n++;
      }
    carry += total;
  }
  if (threadIdx.x == 0) *count = carry;
}

extern "C" int lsdhip_kfbank_create(lsdhip_ctx* c, int max_keyframes, lsdhip_kfbank** out) {
  if (!c || !out || max_keyframes <= 0) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  const int L = LSD_QUICK_KF_CHECK_LVL;
  std::unique_ptr<lsdhip_kfbank> b(new lsdhip_kfbank());
  b->ctx = c;
  b->maxSlots = max_keyframes;
  b->capacity = (c->wl[L] - 2) * (c->hl[L] - 2);
  if (b->capacity < 1) b->capacity = 1;
  b->slotFloats = ((size_t)b->capacity * 5 + 63) / 64 * 64;
  b->slots.reserve((size_t)max_keyframes);
  const size_t bytes = (size_t)max_keyframes * b->slotFloats * sizeof(float) + (size_t)max_keyframes * sizeof(int);
  if (int rc = lsd_dev_alloc(b->d_base, bytes / sizeof(float))) return rc;     // (bytes is a multiple of 4: floats, then ints)
  b->d_count = (int*)(b->d_base + (size_t)max_keyframes * b->slotFloats);
  *out = b.release();
  return LSDHIP_OK;
}

extern "C" void lsdhip_kfbank_destroy(lsdhip_kfbank* b) {
  if (!b) return;
  lsdhip_ctx* c = b->ctx;
  LSD_CTX_LOCK(c);
  (void)hipSetDevice(c->device);
  (void)lsd_sync_all(c);      // searches and puts still queued read and write the allocation
  delete b;
}

extern "C" int lsdhip_kfbank_put(lsdhip_kfbank* b, lsdhip_frame* f, int* slot_out) {
  if (!b || !f || f->ctx != b->ctx) return LSDHIP_E_ARG;
  lsdhip_ctx* c = b->ctx;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  if (!f->hasIDepth && !f->depthPending) { lsd_set_error("lsdhip_kfbank_put: frame %d has no depth", f->id); return LSDHIP_E_STATE; }
  int slot = -1;
  for (size_t i = 0; i < b->slots.size(); i++) if (b->slots[i].frameId == f->id) slot = (int)i;
  if (slot < 0 && (int)b->slots.size() >= b->maxSlots) { lsd_set_error("lsdhip_kfbank_put: all %d slots are taken", b->maxSlots); return LSDHIP_E_CAPACITY; }
  if (int rc = lsd_frame_resolve(f)) return rc;      // meanIdepth is a deferred result on an asynchronous context
  const int L = LSD_QUICK_KF_CHECK_LVL;
  const int at = slot >= 0 ? slot : (int)b->slots.size();
  const LevelIntr& in = c->intr[L];
  const hipStream_t ms = lsd_map_stream(c);
  // a search still running on the tracking stream of a pipelined context may be reading the slot that is replaced
  if (slot >= 0 && c->pipeline) HIPCHK(hipStreamSynchronize(c->stream));
  hipLaunchKernelGGL(k_kfbank_put, dim3(1), dim3(256), 0, ms, (const float*)lsd_depth_latest(f)[L], (const float*)lsd_depthvar_latest(f)[L],
                     (const float*)f->d_image[L], c->wl[L], c->hl[L], in.fxi, in.fyi, in.cxi, in.cyi, b->pos(at), b->colvar(at), b->d_count + at);
  HIPCHK(hipGetLastError());
  int n = 0;
  HIPCHK(hipMemcpyAsync(&n, b->d_count + at, sizeof(int), hipMemcpyDeviceToHost, ms));
  HIPCHK(hipStreamSynchronize(ms));
  if (n < 0 || n > b->capacity) { lsd_set_error("lsdhip_kfbank_put: frame %d: %d points for a slot of %d", f->id, n, b->capacity); return LSDHIP_E_STATE; }
  if (slot < 0) {
    lsdhip_kfbank::Slot s = {};
    s.frameId = f->id;
    s.camToWorld[0] = 1.0; s.camToWorld[7] = 1.0;
    b->slots.push_back(s);
  }
  b->slots[(size_t)at].numPoints = n;
  b->slots[(size_t)at].meanIdepth = f->meanIdepth;
  if (slot_out) *slot_out = at;
  return LSDHIP_OK;
}

extern "C" int lsdhip_kfbank_set_meta(lsdhip_kfbank* b, int slot, const double camToWorld[8], float meanIdepth) {
  if (!b || !camToWorld) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(b->ctx);
  if (slot < 0 || slot >= (int)b->slots.size()) { lsd_set_error("lsdhip_kfbank_set_meta: slot %d is not in use", slot); return LSDHIP_E_ARG; }
  lsdhip_kfbank::Slot& s = b->slots[(size_t)slot];
  for (int i = 0; i < 8; i++) s.camToWorld[i] = camToWorld[i];
  if (!(meanIdepth < 0)) s.meanIdepth = meanIdepth;
  return LSDHIP_OK;
}

extern "C" int lsdhip_kfbank_size(lsdhip_kfbank* b) {
  if (!b) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(b->ctx);
  return (int)b->slots.size();
}

extern "C" int lsdhip_kfbank_info(lsdhip_kfbank* b, int slot, int* frameId, int* numPoints, float* meanIdepth, double camToWorld[8]) {
  if (!b) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(b->ctx);
  if (slot < 0 || slot >= (int)b->slots.size()) { lsd_set_error("lsdhip_kfbank_info: slot %d is not in use", slot); return LSDHIP_E_ARG; }
  const lsdhip_kfbank::Slot& s = b->slots[(size_t)slot];
  if (frameId) *frameId = s.frameId;
  if (numPoints) *numPoints = s.numPoints;
  if (meanIdepth) *meanIdepth = s.meanIdepth;
  if (camToWorld) for (int i = 0; i < 8; i++) camToWorld[i] = s.camToWorld[i];
  return LSDHIP_OK;
}

extern "C" int lsdhip_kfbank_download(lsdhip_kfbank* b, int slot, float* pos, float* colvar) {
  if (!b) return LSDHIP_E_ARG;
  lsdhip_ctx* c = b->ctx;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  if (slot < 0 || slot >= (int)b->slots.size()) { lsd_set_error("lsdhip_kfbank_download: slot %d is not in use", slot); return LSDHIP_E_ARG; }
  const int n = b->slots[(size_t)slot].numPoints;
  if (int rc = lsd_sync_all(c)) return rc;
  if (pos && n > 0) HIPCHK(hipMemcpy(pos, b->pos(slot), (size_t)n * 12, hipMemcpyDeviceToHost));
  if (colvar && n > 0) HIPCHK(hipMemcpy(colvar, b->colvar(slot), (size_t)n * 8, hipMemcpyDeviceToHost));
  return n;
}
