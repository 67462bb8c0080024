// The context: what one lsdhip_ctx owns and how its streams are ordered.  Creation and destruction, the tracking / mapping stream
// pair and its M-sequence, lanes, the transport stream, inter-process flags, the deferred-result slot ring, both profilers and the
// kernel-argument ring.  Nothing here is about a frame's planes (frame.hip).  gfx950 only.
#include "lsdhip_internal.hpp"

#define LSD_FLAG_WGS 16
// ---- where device resources are created (the owners' aliases and the typed forms: lsdhip_internal.hpp).  Test hook
// lsdhip_devtest_fail_alloc_after: the creation that finds the countdown at zero is refused as out of memory, the runtime not asked; < 0: off
static std::atomic<int> g_failAllocAfter{-1};
static bool alloc_refused() { return g_failAllocAfter.load(std::memory_order_relaxed) >= 0 && g_failAllocAfter.fetch_sub(1) == 0; }
static int alloc_result(const char* helper, hipError_t e) {
  if (e == hipSuccess) return LSDHIP_OK;
  lsd_set_error("%s failed: %s", helper, hipGetErrorString(e));
  return LSDHIP_E_HIP;
}
int lsd_dev_alloc_bytes(void** out, size_t bytes, bool zeroed) {
  void* p = nullptr;
  if (int rc = alloc_result(zeroed ? "lsd_dev_alloc_zeroed" : "lsd_dev_alloc", alloc_refused() ? hipErrorOutOfMemory : hipMalloc(&p, bytes))) return rc;
  LsdDev<void> block(p);
  if (zeroed) {
    HIPCHK(hipMemset(p, 0, bytes));
    // the memset runs on the null stream, which the (non-blocking) streams of this library do not wait for: without this the first
    // kernel to use the block could see whatever the allocation held — k_flag_set then counts arrivals on top of it, never reaches
    // its grid size and never raises its flag, and every wait of both processes times out at value 1 (seen twice on the GPU box,
    // tests/test_bands_gpu.py)
    HIPCHK(hipStreamSynchronize(nullptr));
  }
  *out = block.release();
  return LSDHIP_OK;
}
int lsd_pinned_alloc_bytes(void** out, size_t bytes, unsigned flags, void** deviceAlias) {
  void* p = nullptr;
  if (int rc = alloc_result("lsd_pinned_alloc", alloc_refused() ? hipErrorOutOfMemory : hipHostMalloc(&p, bytes, flags))) return rc;
  LsdPinned<void> block(p);
  if (deviceAlias) HIPCHK(hipHostGetDevicePointer(deviceAlias, p, 0));
  *out = block.release();
  return LSDHIP_OK;
}
int lsd_event_create(LsdEvent& owner, unsigned flags) {
  hipEvent_t e = nullptr;
  if (int rc = alloc_result("lsd_event_create", alloc_refused() ? hipErrorOutOfMemory : hipEventCreateWithFlags(&e, flags))) return rc;
  owner.reset(e);
  return LSDHIP_OK;
}
int lsd_stream_create(LsdStream& owner) {
  hipStream_t s = nullptr;
  if (int rc = alloc_result("lsd_stream_create", alloc_refused() ? hipErrorOutOfMemory : hipStreamCreateWithFlags(&s, hipStreamNonBlocking))) return rc;
  owner.reset(s);
  return LSDHIP_OK;
}
extern "C" void lsdhip_live_resources(long long out[4]) {
  out[0] = LsdLive<LsdDevRelease>::count.load(); out[1] = LsdLive<LsdPinnedRelease>::count.load();
  out[2] = LsdLive<LsdEventRelease>::count.load(); out[3] = LsdLive<LsdStreamRelease>::count.load();
}
extern "C" void lsdhip_devtest_fail_alloc_after(int n) { g_failAllocAfter.store(n < 0 ? -1 : n); }

extern "C" void lsdhip_default_params(lsdhip_params* p) {
  p->minUseGrad = 5;
  p->cameraPixelNoise2 = 4 * 4;
  p->depthSmoothingFactor = 1;
  p->allowNegativeIdepths = 1;
  p->useSubpixelStereo = 1;
  p->useAffineLightningEstimation = 1;
  p->KFDistWeight = 4;
  p->KFUsageWeight = 3;
}

extern "C" int lsdhip_ctx_create(int device, int w, int h, const float K[4], const lsdhip_params* params, lsdhip_ctx** out) {
  if (!out || !K || w <= 0 || h <= 0 || (w % 16) != 0 || (h % 16) != 0) {
    lsd_set_error("lsdhip_ctx_create: image dimensions must be positive multiples of 16 (got %dx%d)", w, h);
    return LSDHIP_E_ARG;
  }
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) {
    lsd_set_error("lsdhip_ctx_create: device %d not available (%d visible)", device, ndev);
    return LSDHIP_E_HIP;
  }
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<lsdhip_ctx> owner(new lsdhip_ctx());
  lsdhip_ctx* const c = owner.get();
  LSD_CTX_LOCK(c);
  c->device = device;
  c->w = w;
  c->h = h;
  if (params) c->params = *params; else lsdhip_default_params(&c->params);
  // Frame::initialize (Frame.cpp:397-459)
  float fx[LSD_LEVELS], fy[LSD_LEVELS], cx[LSD_LEVELS], cy[LSD_LEVELS];
  fx[0] = K[0]; fy[0] = K[1]; cx[0] = K[2]; cy[0] = K[3];
  for (int l = 0; l < LSD_LEVELS; l++) {
    c->wl[l] = w >> l;
    c->hl[l] = h >> l;
    if (l > 0) {
      fx[l] = fx[l - 1] * 0.5;
      fy[l] = fy[l - 1] * 0.5;
      cx[l] = (cx[0] + 0.5) / ((int)1 << l) - 0.5;
      cy[l] = (cy[0] + 0.5) / ((int)1 << l) - 0.5;
    }
    float Kl[9] = {fx[l], 0.f, cx[l], 0.f, fy[l], cy[l], 0.f, 0.f, 1.f};
    float Ki[9];
    lsdm::inverse3_eigen(Kl, Ki);
    c->intr[l] = {fx[l], fy[l], cx[l], cy[l], Ki[0], Ki[4], Ki[2], Ki[5]};
    if (l == 0) { memcpy(c->K0, Kl, sizeof(Kl)); memcpy(c->K0inv, Ki, sizeof(Ki)); }
  }
  // (the tracking stream at the highest queue priority: 36.3 k against 37.1 k frames/s at S = 32, profiles/r05_notes.md — not kept)
  if (int rc = lsd_stream_create(c->stream)) return rc;
  if (int rc = lsd_event_create(c->ev_a)) return rc;
  if (int rc = lsd_event_create(c->ev_b)) return rc;
  if (int rc = lsd_pinned_alloc(c->h_slots, LSD_NUM_SLOTS, hipHostMallocMapped)) return rc;
  memset(c->h_slots, 0, LSD_NUM_SLOTS * sizeof(DeferredSlot));
  *out = owner.release();
  return LSDHIP_OK;
}
extern "C" void lsdhip_ctx_destroy(lsdhip_ctx* c) {
  if (!c) return;
  lsd_host_trace_print();
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  if (c->mstream) (void)hipStreamSynchronize(c->mstream);
  lsd_trace_dump(c);
  for (int i = 0; i < lsdhip_ctx::MAX_LANES; i++) if (c->lanes[i]) (void)hipStreamSynchronize(c->lanes[i]);
  if (c->aux_stream) (void)hipStreamSynchronize(c->aux_stream);
  delete c;
}
extern "C" void* lsdhip_ctx_stream(lsdhip_ctx* c) { return c ? (void*)c->stream : nullptr; }
extern "C" int lsdhip_ctx_alloc_dev(lsdhip_ctx* c, size_t bytes, void** out) {
  if (!c || !out || bytes == 0) return LSDHIP_E_ARG;
  HIPCHK(hipSetDevice(c->device));
  return lsd_dev_alloc_bytes(out, bytes, false);      // the caller's from here on (lsdhip_ctx_free_dev)
}
extern "C" int lsdhip_ctx_free_dev(lsdhip_ctx* c, void* p) {
  if (!c) return LSDHIP_E_ARG;
  if (!p) return LSDHIP_OK;
  HIPCHK(hipSetDevice(c->device));
  if (int rc = lsd_sync_all(c)) return rc;
  HIPCHK(LsdDevRelease::call(p));      // (handed out by lsdhip_ctx_alloc_dev without an owner: released the same way)
  return LSDHIP_OK;
}
extern "C" int lsdhip_ctx_reserve_frames(lsdhip_ctx* c, int n) { return (!c || n < 0) ? LSDHIP_E_ARG : lsd_frames_reserve(c, n); }
extern "C" int lsdhip_ctx_synchronize(lsdhip_ctx* c) {
  if (!c) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(c);
  for (int i = 0; i < LSD_NUM_SLOTS; i++) {   // pick up every deferred result
    if (c->slot_stats_owner[i]) { int rc = lsd_frame_resolve(c->slot_stats_owner[i]); if (rc) return rc; }
    if (c->slot_rescale_owner[i]) { int rc = lsd_frame_resolve(c->slot_rescale_owner[i]); if (rc) return rc; }
  }
  if (c->aux_stream) HIPCHK(hipStreamSynchronize(c->aux_stream));
  return lsd_sync_all(c);
}
// ---- pipelined contexts: tracking stream beside mapping stream ---------------------------------------------------------------------
extern "C" int lsdhip_ctx_set_pipeline(lsdhip_ctx* c, int on) {
  if (!c) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  if (int rc = lsd_sync_all(c)) return rc;
  if (on && !c->mstream) {
    for (int i = 0; i < LSD_EVR; i++) { if (int rc = lsd_event_create(c->mEv[i], hipEventDisableTiming)) return rc; }
    if (int rc = lsd_stream_create(c->mstream)) return rc;      // last: a context has a mapping stream only once it has all of its events
  }
  if (!on && c->pipeline) {
    // back to one stream: everything is drained, so every recorded point counts as passed and waited for
    c->mDoneSeq = c->tWaitedM = c->mSeq;
  }
  c->pipeline = on != 0;
  return LSDHIP_OK;
}
extern "C" int lsdhip_ctx_pipeline(lsdhip_ctx* c) { return c ? (c->pipeline ? 1 : 0) : LSDHIP_E_ARG; }
extern "C" void* lsdhip_ctx_map_stream(lsdhip_ctx* c) { return c ? (void*)lsd_map_stream(c) : nullptr; }
int lsd_sync_all(lsdhip_ctx* c) {
  if (c->pipeline && !c->pendingMerges.empty()) { if (int rc = lsd_flush_merges(c)) return rc; }
  for (int i = 0; i < c->lanes_open; i++) if (c->lane_used[i]) HIPCHK(hipStreamSynchronize(c->lanes[i]));   // (inside an open lane region)
  if (c->mstream) {
    HIPCHK(hipStreamSynchronize(c->mstream));
    c->mDoneSeq = c->mSeq;
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  return LSDHIP_OK;
}
// Tracking -> mapping ordering.  A mapping-stream operation that consumes a tracking job's results is queued by the host AFTER it has
// seen the job's `done` (pinned memory, written behind a system-scope fence by the finishing launch); what the operation reads — the
// frame's mask, and through the host the pose — was written by launches that had completed before the finishing launch started, and
// the launches still queued behind it touch only the tracker's own state.  So no event is recorded on the tracking stream: a record
// behind every job is a barrier packet in the queue the launch chain runs through (the first form of the pipeline had one, plus a
// hipStreamWaitEvent on the mapping stream; profiles/r04_notes.md).
int lsd_m_begin(lsdhip_ctx* c) {
  if (!c->pendingMerges.empty()) return lsd_flush_merges(c);
  return LSDHIP_OK;
}
long long lsd_m_record(lsdhip_ctx* c) {
  if (!c->pipeline) return 0;
  if (c->lanes_open) { c->lane_record_pending = true; return c->mSeq + 1; }   // recorded once, where the lanes join (lsdhip_ctx_lanes_end)
  const long long s = c->mSeq + 1;
  if (hipEventRecord(c->mEv[s % LSD_EVR], c->mstream) != hipSuccess) { lsd_set_error("hipEventRecord on the mapping stream failed"); return LSDHIP_E_HIP; }
  c->mSeq = s;
  return s;
}
int lsd_t_wait_m(lsdhip_ctx* c, long long seq) {
  if (!c->pipeline || seq <= c->tWaitedM || seq <= c->mDoneSeq) return LSDHIP_OK;
  if (seq > c->mSeq) {
    // a sequence number beyond the last record point: handed out inside an open lane region (recorded where the lanes join) — there is
    // no event to wait for yet
    if (c->lanes_open) { lsd_set_error("tracking job depends on mapping work of an open lane region (call lsdhip_ctx_lanes_end first)"); return LSDHIP_E_STATE; }
    seq = c->mSeq;
  }
  // the ring slot holds the event of `seq` or, once the ring has wrapped, of a later point of the in-order stream: either orders us
  HIPCHK(hipStreamWaitEvent(c->stream, c->mEv[seq % LSD_EVR], 0));
  c->tWaitedM = seq;
  return LSDHIP_OK;
}
bool lsd_m_done(lsdhip_ctx* c, long long seq) {
  if (seq <= c->mDoneSeq) return true;
  if (seq > c->mSeq) return false;
  if (hipEventQuery(c->mEv[seq % LSD_EVR]) != hipSuccess) return false;
  // (after a wrap the slot's event is a later point: then more than `seq` is done, which is still true of `seq`)
  if (c->mSeq - seq < LSD_EVR) c->mDoneSeq = seq;
  return true;
}
extern "C" int lsdhip_ctx_copy_dev(lsdhip_ctx* c, void* dst, const void* src, size_t bytes) {
  if (!c || !dst || !src) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, lsd_transport_stream(c)));
  return LSDHIP_OK;
}
// ---- lanes: the DepthMap call chains of DIFFERENT depth maps are independent of each other; between lanes_begin and lanes_end the
// caller routes each map's calls to one of n extra streams (lane_select), so that the chains of several sequences (finalizeKeyFrame +
// createKeyFrame: ~18 small dependent launches each) run side by side instead of one after the other.  Everything queued on the
// context's stream before lanes_begin is visible to every lane; lanes_end orders the context's stream behind all lanes.
extern "C" int lsdhip_ctx_lanes_begin(lsdhip_ctx* c, int n) {
  if (!c || n < 1 || n > lsdhip_ctx::MAX_LANES) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(c);
  if (c->lanes_open) { lsd_set_error("lsdhip_ctx_lanes_begin: already open"); return LSDHIP_E_STATE; }
  const hipStream_t base = c->pipeline ? c->mstream : c->stream;     // lanes branch off the stream the DepthMap calls run on
  HIPCHK(hipSetDevice(c->device));
  if (!c->lane_fork) { if (int rc = lsd_event_create(c->lane_fork, hipEventDisableTiming)) return rc; }
  for (int i = 0; i < n; i++) {
    if (!c->lanes[i]) {
      if (int rc = lsd_event_create(c->lane_done[i], hipEventDisableTiming)) return rc;
      if (int rc = lsd_stream_create(c->lanes[i])) return rc;
    }
    c->lane_used[i] = false;
  }
  // a lane waits for the fork point only: whatever the lanes' calls read must be queued before it — also the merges of speculative
  // trials' refPixelWasGood planes that the tracking calls have noted but not queued yet (createKeyFrame reads the new keyframe's mask)
  if (c->pipeline && !c->pendingMerges.empty()) { if (int rcf = lsd_flush_merges(c)) return rcf; }
  HIPCHK(hipEventRecord(c->lane_fork, base));
  c->lanes_open = n;
  c->lane_cur = -1;
  c->lane_record_pending = false;
  return LSDHIP_OK;
}
extern "C" int lsdhip_ctx_lane_select(lsdhip_ctx* c, int lane) {
  if (!c) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(c);
  if (!c->lanes_open || lane < -1 || lane >= c->lanes_open) { lsd_set_error("lsdhip_ctx_lane_select: lane %d of %d", lane, c->lanes_open); return LSDHIP_E_ARG; }
  if (lane >= 0 && !c->lane_used[lane]) {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamWaitEvent(c->lanes[lane], c->lane_fork, 0));
    c->lane_used[lane] = true;
  }
  c->lane_cur = lane;
  return LSDHIP_OK;
}
extern "C" int lsdhip_ctx_lanes_end(lsdhip_ctx* c) {
  if (!c) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(c);
  if (!c->lanes_open) return LSDHIP_OK;
  HIPCHK(hipSetDevice(c->device));
  c->lane_cur = -1;
  const hipStream_t base = c->pipeline ? c->mstream : c->stream;
  for (int i = 0; i < c->lanes_open; i++) {
    if (!c->lane_used[i]) continue;
    HIPCHK(hipEventRecord(c->lane_done[i], c->lanes[i]));
    HIPCHK(hipStreamWaitEvent(base, c->lane_done[i], 0));
  }
  c->lanes_open = 0;
  // pipelined contexts: the calls inside the region were all given the mapping-stream sequence number of THIS point (lsd_m_record), the
  // first one at which the mapping stream is behind every lane
  if (c->lane_record_pending) { c->lane_record_pending = false; if (lsd_m_record(c) < 0) return LSDHIP_E_HIP; }
  return LSDHIP_OK;
}
// ---- transport stream: exchange under compute (halo rows of the row-band loop travel while the interior rows are computed) -------
extern "C" int lsdhip_ctx_aux_begin(lsdhip_ctx* c) {
  if (!c) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  if (c->aux_active) { lsd_set_error("lsdhip_ctx_aux_begin: already between begin and end"); return LSDHIP_E_STATE; }
  if (!c->aux_stream) {
    if (int rc = lsd_event_create(c->aux_fork, hipEventDisableTiming)) return rc;
    if (int rc = lsd_event_create(c->aux_done, hipEventDisableTiming)) return rc;
    if (int rc = lsd_stream_create(c->aux_stream)) return rc;
  }
  HIPCHK(hipEventRecord(c->aux_fork, c->stream));
  HIPCHK(hipStreamWaitEvent(c->aux_stream, c->aux_fork, 0));
  c->aux_active = true;
  return LSDHIP_OK;
}
extern "C" int lsdhip_ctx_aux_end(lsdhip_ctx* c) {
  if (!c) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(c);
  if (!c->aux_active) { lsd_set_error("lsdhip_ctx_aux_end without lsdhip_ctx_aux_begin"); return LSDHIP_E_STATE; }
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipEventRecord(c->aux_done, c->aux_stream));
  c->aux_active = false;
  c->aux_pending = true;
  return LSDHIP_OK;
}
extern "C" int lsdhip_ctx_aux_join(lsdhip_ctx* c) {
  if (!c) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(c);
  if (c->aux_active) { lsd_set_error("lsdhip_ctx_aux_join between begin and end"); return LSDHIP_E_STATE; }
  if (!c->aux_pending) return LSDHIP_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamWaitEvent(c->stream, c->aux_done, 0));
  c->aux_pending = false;
  return LSDHIP_OK;
}
extern "C" void* lsdhip_ctx_aux_stream(lsdhip_ctx* c) { return c ? (void*)c->aux_stream : nullptr; }
// ---- inter-process exchange on one node without RCCL (lsdhip_driver's second transport): IPC-mapped device memory + flags ---------
// A flag is an int in device memory that both processes map; values only grow.  Both operations are stream-ordered one-lane kernels:
// set publishes everything the stream did before it (system-scope release), wait spins — bounded — until the flag has reached the
// value and raises *fail otherwise.
// Both run as LSD_FLAG_WGS one-wave workgroups, dealt round-robin over the chip's 8 XCDs: the writes a set publishes may sit dirty in
// any XCD's L2 and the data a wait is followed by may be cached stale in any XCD's L2 — and the other side is another process, whose
// accesses this runtime's own cache bookkeeping between consecutive launches knows nothing about.  So every XCD runs the
// system-scope release (set: before the last arriving workgroup raises the flag) or acquire (wait: after it has seen the flag).
__global__ void k_flag_set(int* flag, int value, unsigned* arrive) {
  if (threadIdx.x != 0) return;
  __threadfence_system();
  const unsigned n = __hip_atomic_fetch_add(arrive, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
  if (n + 1 == gridDim.x) {
    __hip_atomic_store(arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    // the next set on this stream starts from zero
    __hip_atomic_store(flag, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
__global__ void k_flag_wait(const int* flag, int value, int* fail) {
  if (threadIdx.x != 0) return;
  for (unsigned spins = 0; spins < (1u << 26); spins++) {          // ~8 s (2 s proved too tight once for a peer process's first launches on a shared GPU)
    if (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) >= value) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");                // system scope: this XCD's L2 drops what it cached of foreign memory
      return;
    }
    __builtin_amdgcn_s_sleep(8);
  }
  *fail = value;
}
extern "C" int lsdhip_ctx_ipc_export(lsdhip_ctx* c, void* dev, unsigned char handle64[64]) {
  if (!c || !dev || !handle64) return LSDHIP_E_ARG;
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t is 64 bytes");
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  hipIpcMemHandle_t h;
  HIPCHK(hipIpcGetMemHandle(&h, dev));
  memcpy(handle64, &h, 64);
  return LSDHIP_OK;
}
extern "C" int lsdhip_ctx_ipc_open(lsdhip_ctx* c, const unsigned char handle64[64], void** out_dev) {
  if (!c || !handle64 || !out_dev) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  hipIpcMemHandle_t h;
  memcpy(&h, handle64, 64);
  HIPCHK(hipIpcOpenMemHandle(out_dev, h, hipIpcMemLazyEnablePeerAccess));
  return LSDHIP_OK;
}
extern "C" int lsdhip_ctx_ipc_close(lsdhip_ctx* c, void* dev) {
  if (!c || !dev) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipIpcCloseMemHandle(dev));
  return LSDHIP_OK;
}
extern "C" int lsdhip_ctx_flag_set(lsdhip_ctx* c, int* flag_dev, int value) {
  if (!c || !flag_dev) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  if (!c->d_flagArrive) { if (int rc = lsd_dev_alloc_zeroed(c->d_flagArrive, 16)) return rc; }
  // (sets of one context are stream-ordered, on either of its streams in turn: one arrival counter serves them all)
  hipLaunchKernelGGL(k_flag_set, dim3(LSD_FLAG_WGS), dim3(64), 0, lsd_transport_stream(c), flag_dev, value, c->d_flagArrive);
  HIPCHK(hipGetLastError());
  return LSDHIP_OK;
}
extern "C" int lsdhip_ctx_flag_wait(lsdhip_ctx* c, const int* flag_dev, int value, int* fail_dev) {
  if (!c || !flag_dev || !fail_dev) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  hipLaunchKernelGGL(k_flag_wait, dim3(LSD_FLAG_WGS), dim3(64), 0, lsd_transport_stream(c), flag_dev, value, fail_dev);
  HIPCHK(hipGetLastError());
  return LSDHIP_OK;
}
extern "C" int lsdhip_ctx_memset_dev(lsdhip_ctx* c, void* dev, int byte, size_t bytes) {
  if (!c || !dev) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemsetAsync(dev, byte, bytes, c->stream));
  return LSDHIP_OK;
}
extern "C" int lsdhip_ctx_read_dev(lsdhip_ctx* c, void* host, const void* dev, size_t bytes) {
  if (!c || !host || !dev) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  if (c->pipeline) { if (int rc = lsd_sync_all(c)) return rc; }
  HIPCHK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return LSDHIP_OK;
}
extern "C" int lsdhip_ctx_set_async(lsdhip_ctx* c, int on) {
  if (!c) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(c);
  c->async = on != 0;
  return LSDHIP_OK;
}
int lsd_ctx_take_slot(lsdhip_ctx* c) {
  LSD_CTX_LOCK(c);
  const int i = c->slot_next;
  c->slot_next = (c->slot_next + 1) % LSD_NUM_SLOTS;
  if (c->slot_stats_owner[i]) { int rc = lsd_frame_resolve(c->slot_stats_owner[i]); if (rc) return rc; }
  if (c->slot_rescale_owner[i]) { int rc = lsd_frame_resolve(c->slot_rescale_owner[i]); if (rc) return rc; }
  c->slot_epoch[i] = c->enqEpoch;
  c->slot_mseq[i] = c->mSeq + 1;     // pipelined contexts: the calling DepthMap entry ends with the record point of this number
  return i;
}
int lsd_ctx_claim_stats_slot(lsdhip_ctx* c, lsdhip_frame* f) {
  const int slot = lsd_ctx_take_slot(c);
  if (slot < 0) return slot;
  if (f->pendStats >= 0) c->slot_stats_owner[f->pendStats] = nullptr;
  f->pendStats = slot;
  c->slot_stats_owner[slot] = f;
  return slot;
}
int lsd_ctx_claim_rescale_slot(lsdhip_ctx* c, lsdhip_frame* f) {
  const int slot = lsd_ctx_take_slot(c);
  if (slot < 0) return slot;
  if (f->pendRescale >= 0) c->slot_rescale_owner[f->pendRescale] = nullptr;
  f->pendRescale = slot;
  c->slot_rescale_owner[slot] = f;
  return slot;
}
extern "C" int lsdhip_ctx_intrinsics(lsdhip_ctx* c, int level, float out[8]) {
  if (!c || level < 0 || level >= LSD_LEVELS) return LSDHIP_E_ARG;
  memcpy(out, &c->intr[level], sizeof(LevelIntr));
  return LSDHIP_OK;
}
extern "C" int lsdhip_prof_enable(lsdhip_ctx* c, int on) { if (!c) return LSDHIP_E_ARG; c->prof_on = on != 0; return LSDHIP_OK; }
static void bprof_collect(lsdhip_ctx* c, bool wait) {
  for (int i = 0; i < LSD_BPROF_SLOTS; i++) {
    lsdhip_ctx::BProfSlot& p = c->bprof[i];
    if (!p.pending) continue;
    if (wait) (void)hipEventSynchronize(p.b);
    else if (hipEventQuery(p.b) != hipSuccess) continue;
    float ms = 0;
    if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) { c->bprof_ms[p.kind] += ms; c->bprof_units[p.kind] += p.units; c->bprof_calls[p.kind]++; }
    p.pending = false;
  }
}
int lsd_bprof_begin(lsdhip_ctx* c, int kind, hipStream_t s) {
  if (!c->prof_on || kind < 0 || kind >= LSD_BPROF_KINDS) return -1;
  if ((c->bprof_tick[kind]++ % LSD_BPROF_PERIOD) != 0) return -1;
  const int i = c->bprof_next;
  c->bprof_next = (c->bprof_next + 1) % LSD_BPROF_SLOTS;
  lsdhip_ctx::BProfSlot& p = c->bprof[i];
  if (p.pending) { bprof_collect(c, false); if (p.pending) { if (hipEventSynchronize(p.b) != hipSuccess) return LSDHIP_E_HIP; bprof_collect(c, false); } }
  if (!p.b) { if (lsd_event_create(p.a) || lsd_event_create(p.b)) return LSDHIP_E_HIP; }
  p.kind = kind;
  if (hipEventRecord(p.a, s) != hipSuccess) return LSDHIP_E_HIP;
  return i;
}
int lsd_bprof_end(lsdhip_ctx* c, int slot, hipStream_t s, double units) {
  if (slot < 0) return slot == -1 ? LSDHIP_OK : slot;
  lsdhip_ctx::BProfSlot& p = c->bprof[slot];
  if (hipEventRecord(p.b, s) != hipSuccess) return LSDHIP_E_HIP;
  p.units = units;
  p.pending = true;
  return LSDHIP_OK;
}
// ms / calls / units per kind (LSD_BPROF_KINDS of each) of the sampled shared launches since the last reset, and the sampled walk launches'
// work: obs[0] = launches counted, obs[1] = searches, obs[2] = walk steps.  Waits for the brackets still in flight.
extern "C" int lsdhip_ctx_batch_prof_read(lsdhip_ctx* c, double* ms, long long* calls, double* units, double obs[3]) {
  if (!c || !ms || !calls || !units) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  bprof_collect(c, true);
  for (int k = 0; k < LSD_BPROF_KINDS; k++) { ms[k] = c->bprof_ms[k]; calls[k] = c->bprof_calls[k]; units[k] = c->bprof_units[k]; }
  if (obs) {
    obs[0] = obs[1] = obs[2] = 0;
    if (c->d_obsBatchAcc) {
      unsigned long long h[66];
      if (int rc = lsd_sync_all(c)) return rc;
      HIPCHK(hipMemcpy(h, c->d_obsBatchAcc, sizeof(h), hipMemcpyDeviceToHost));
      obs[0] = (double)h[65]; obs[1] = (double)h[0];
      for (int i = 1; i <= 64; i++) obs[2] += (double)h[i];
    }
  }
  return LSDHIP_OK;
}
extern "C" int lsdhip_prof_reset(lsdhip_ctx* c) {
  if (!c) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(c);
  c->prof_ms = 0; c->prof_bytes = 0; c->prof_launches = 0;
  bprof_collect(c, true);
  for (int k = 0; k < LSD_BPROF_KINDS; k++) { c->bprof_ms[k] = 0; c->bprof_units[k] = 0; c->bprof_calls[k] = 0; }
  if (c->d_obsBatchAcc) HIPCHK(hipMemsetAsync(c->d_obsBatchAcc, 0, 66 * 8, lsd_map_stream(c)));
  return LSDHIP_OK;
}
extern "C" int lsdhip_prof_read(lsdhip_ctx* c, double* ms, long long* launches, double* bytes) {
  if (c) { int rc = lsd_prof_collect(c); if (rc) return rc; }
  if (!c) return LSDHIP_E_ARG;
  if (ms) *ms = c->prof_ms;
  if (launches) *launches = c->prof_launches;
  if (bytes) *bytes = c->prof_bytes;
  return LSDHIP_OK;
}

// Kernel-argument records of the batched launches: a ring of pinned slots with device twins.  A slot is handed out again only once the
// event recorded behind its last use has completed: lsd_args_commit records it behind the copy, lsd_args_release — called after the
// launches that read the device twin — moves it behind them (whatever stream they were queued on).
int lsd_args_begin(lsdhip_ctx* c, size_t bytes, void** host_out, void** dev_out) {
  LSD_CTX_LOCK(c);
  lsdhip_ctx::ArgRing& r = c->args;
  constexpr int NS = lsdhip_ctx::ArgRing::NS;
  if (bytes > r.slotBytes) {
    // grow: nothing may still read the old block.  The new pair exists before the old one goes: a failed growth leaves the ring as it was
    HIPCHK(hipDeviceSynchronize());
    const size_t want = lsd_align_up(bytes * 2 > 65536 ? bytes * 2 : 65536, 256);
    LsdPinned<uint8_t> h; LsdDev<uint8_t> d;
    if (int rc = lsd_pinned_alloc(h, want * NS, hipHostMallocDefault)) return rc;
    if (int rc = lsd_dev_alloc(d, want * NS)) return rc;
    for (int i = 0; i < NS; i++) { r.used[i] = false; if (!r.ev[i]) { if (int rc = lsd_event_create(r.ev[i], hipEventDisableTiming)) return rc; } }   // (drained: no slot is in use)
    r.h = std::move(h); r.d = std::move(d);
    r.slotBytes = want;
    r.gen++;
  }
  const int i = r.next;
  r.next = (r.next + 1) % NS;
  r.serial++;
  if (r.used[i]) HIPCHK(hipEventSynchronize(r.ev[i]));   // (NS - 1 uses ago: long finished)
  r.cur = i;
  r.curBytes = bytes;
  *host_out = r.h + (size_t)i * r.slotBytes;
  *dev_out = r.d + (size_t)i * r.slotBytes;
  return LSDHIP_OK;
}
int lsd_args_commit(lsdhip_ctx* c, hipStream_t s) {
  LSD_CTX_LOCK(c);
  lsdhip_ctx::ArgRing& r = c->args;
  const int i = r.cur;
  HIPCHK(hipMemcpyAsync(r.d + (size_t)i * r.slotBytes, r.h + (size_t)i * r.slotBytes, r.curBytes, hipMemcpyHostToDevice, s));
  HIPCHK(hipEventRecord(r.ev[i], s));
  r.used[i] = true;
  return LSDHIP_OK;
}
// `dev`: the device address lsd_args_begin / lsd_args_push handed out — the slot is identified by it, not by "the slot begun last": a
// helper that pushes arguments of its own between a commit and its release (lsd_frame_build_idepth_pyramid_batch inside the keyframe
// change) must not make the release guard the wrong slot
int lsd_args_release(lsdhip_ctx* c, const void* dev, hipStream_t s) {
  LSD_CTX_LOCK(c);
  lsdhip_ctx::ArgRing& r = c->args;
  constexpr int NS = lsdhip_ctx::ArgRing::NS;
  const uint8_t* p = (const uint8_t*)dev;
  if (!r.d || r.slotBytes == 0 || p < (const uint8_t*)r.d || p >= (const uint8_t*)r.d + r.slotBytes * NS) return LSDHIP_OK;   // (the ring was regrown since: the device was drained then)
  const int i = (int)((size_t)(p - (const uint8_t*)r.d) / r.slotBytes);
  if (!r.used[i]) return LSDHIP_OK;
  HIPCHK(hipEventRecord(r.ev[i], s));
  return LSDHIP_OK;
}
int lsd_args_push(lsdhip_ctx* c, const void* src, size_t bytes, hipStream_t s, void** dev_out) {
  LSD_CTX_LOCK(c);
  void* h = nullptr;
  if (int rc = lsd_args_begin(c, bytes, &h, dev_out)) return rc;
  memcpy(h, src, bytes);
  return lsd_args_commit(c, s);
}
