// Developer experiments of the pipeline bug hunt (profiles/r04_notes.md §1a; the switches are listed in lsdhip_internal.hpp): host
// trace, unrelated kernels beside a tracking job, checksum trace, the mapping-stream gate.  Compiled into the LSD_DEVTOOLS build only;
// the default library keeps the no-op lsdhip_host_mark of the C ABI and nothing else of this file.
#include "lsdhip_internal.hpp"

#ifdef LSD_DEVTOOLS
// Developer instrumentation (LSDHIP_HOST_TRACE=1): host-side time between consecutive marks of the calling thread, summed per mark
// id and printed when a context is destroyed.  Costs one steady_clock read per mark when on, one branch when off.
static const bool g_hostTraceOn = getenv("LSDHIP_HOST_TRACE") != nullptr;
static long long g_htNs[32], g_htN[32], g_htHist[32][9];
static thread_local long long g_htLast = 0;
extern "C" void lsdhip_host_mark(int k) {
  if (!g_hostTraceOn) return;
  const long long now = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
  if (k > 0 && k < 32 && g_htLast) {
    const long long d = now - g_htLast;
    g_htNs[k] += d; g_htN[k]++;
    static const long long edges[8] = {2000, 5000, 10000, 20000, 50000, 100000, 200000, 500000};
    int b = 0;
    while (b < 8 && d >= edges[b]) b++;
    g_htHist[k][b]++;
  }
  g_htLast = now;
}
void lsd_host_trace_print() {
  if (!g_hostTraceOn) return;
  for (int k = 0; k < 32; k++)
    if (g_htN[k]) {
      fprintf(stderr, "HOSTTRACE mark %2d: n %6lld  mean %7.2f us   <2 <5 <10 <20 <50 <100 <200 <500 >=500 us:", k, g_htN[k], g_htNs[k] / 1e3 / g_htN[k]);
      for (int b = 0; b < 9; b++) fprintf(stderr, " %lld", g_htHist[k][b]);
      fprintf(stderr, "\n");
    }
}
// Experiment: kernels that touch nothing but their own buffer, queued on the mapping stream right when a tracking job starts.
// kind 1: memory streaming (32 MB read-modify-write), 2: LDS-heavy workgroups (9.6 KB each, like k_reg_fused), 3: ALU spin.
static const int g_pipeDummy = getenv("LSDHIP_PIPE_DUMMY") ? atoi(getenv("LSDHIP_PIPE_DUMMY")) : 0;
__global__ __launch_bounds__(256) void k_dummy_stream(float* p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = p[i] * 1.0001f + 1.0f;
}
__global__ __launch_bounds__(256) void k_dummy_lds(float* p) {
  __shared__ float s[2400];
  for (int i = threadIdx.x; i < 2400; i += 256) s[i] = (float)(i + blockIdx.x);
  __syncthreads();
  float acc = 0;
  for (int r = 0; r < 40; r++) for (int i = threadIdx.x; i < 2400; i += 256) acc += s[(i * 7 + r) % 2400];
  p[(size_t)blockIdx.x * 256 + threadIdx.x] = acc;
}
// kind 4: workgroup barriers, no LDS; kind 5: LDS, no barrier (64-lane workgroups, lane-private slots); kind 6: like 2 with 40 KB
__global__ __launch_bounds__(256) void k_dummy_barrier(float* p) {
  float acc = (float)threadIdx.x;
  for (int r = 0; r < 400; r++) { acc = acc * 1.0001f + 0.5f; __syncthreads(); }
  p[(size_t)blockIdx.x * 256 + threadIdx.x] = acc;
}
__global__ __launch_bounds__(64) void k_dummy_lds_nobar(float* p) {
  __shared__ float s[2400];
  float acc = 0;
  for (int r = 0; r < 60; r++) {
    for (int i = threadIdx.x; i < 2400; i += 64) s[i] = (float)(i + r);
    for (int i = threadIdx.x; i < 2400; i += 64) acc += s[i];
  }
  p[(size_t)blockIdx.x * 64 + threadIdx.x] = acc;
}
__global__ __launch_bounds__(256) void k_dummy_lds_big(float* p) {
  __shared__ float s[10000];
  for (int i = threadIdx.x; i < 10000; i += 256) s[i] = (float)(i + blockIdx.x);
  __syncthreads();
  float acc = 0;
  for (int r = 0; r < 10; r++) for (int i = threadIdx.x; i < 10000; i += 256) acc += s[(i * 7 + r) % 10000];
  p[(size_t)blockIdx.x * 256 + threadIdx.x] = acc;
}
__global__ __launch_bounds__(64) void k_dummy_spin(float* p, long long spin) {
  long long t0 = clock64();
  float a = (float)threadIdx.x;
  while (clock64() - t0 < spin) a = a * 1.0001f + 0.5f;
  p[(size_t)blockIdx.x * 64 + threadIdx.x] = a;
}
int lsd_pipe_dummy(lsdhip_ctx* c) {
  if (!g_pipeDummy || !c->pipeline) return LSDHIP_OK;
  const size_t n = 8u << 20;
  if (!c->dev.dummyBuf) { if (int rc = lsd_dev_alloc_zeroed(c->dev.dummyBuf, n)) return rc; }
  float* buf = c->dev.dummyBuf;
  for (int rep = 0; rep < 4; rep++) {
    if (g_pipeDummy == 1) hipLaunchKernelGGL(k_dummy_stream, dim3(2048), dim3(256), 0, c->mstream, buf, n);
    else if (g_pipeDummy == 2) hipLaunchKernelGGL(k_dummy_lds, dim3(1200), dim3(256), 0, c->mstream, buf);
    else if (g_pipeDummy == 4) hipLaunchKernelGGL(k_dummy_barrier, dim3(1200), dim3(256), 0, c->mstream, buf);
    else if (g_pipeDummy == 5) hipLaunchKernelGGL(k_dummy_lds_nobar, dim3(4800), dim3(64), 0, c->mstream, buf);
    else if (g_pipeDummy == 6) hipLaunchKernelGGL(k_dummy_lds_big, dim3(1200), dim3(256), 0, c->mstream, buf);
    else hipLaunchKernelGGL(k_dummy_spin, dim3(4800), dim3(64), 0, c->mstream, buf, 20000LL);
  }
  return LSDHIP_OK;
}
static const char* g_traceSums = getenv("LSDHIP_TRACE_SUMS");
#define LSD_TRACE_SLOTS 65536
__global__ __launch_bounds__(256) void k_trace_sum(const uint32_t* __restrict__ p, size_t nwords, unsigned long long* out) {
  unsigned long long acc = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nwords; i += (size_t)gridDim.x * 256)
    acc += (unsigned long long)p[i] * (unsigned long long)(i * 2654435761ull + 1ull);
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if ((threadIdx.x & 63) == 0) atomicAdd(out, acc);
}
void lsd_trace_sum(lsdhip_ctx* c, hipStream_t s, int kind, int id, const void* p, size_t bytes) {
  if (!g_traceSums) return;
  if (!c->dev.d_sums) { if (lsd_dev_alloc_zeroed(c->dev.d_sums, LSD_TRACE_SLOTS)) return; }
  const size_t slot = c->dev.sums_meta.size() / 2;
  if (slot >= LSD_TRACE_SLOTS) return;
  c->dev.sums_meta.push_back(kind); c->dev.sums_meta.push_back(id);
  c->dev.sums_host.push_back(0);
  const size_t nwords = bytes / 4;
  int grid = (int)((nwords + 255) / 256); if (grid > 64) grid = 64; if (grid < 1) grid = 1;
  hipLaunchKernelGGL(k_trace_sum, dim3(grid), dim3(256), 0, s, (const uint32_t*)p, nwords, c->dev.d_sums + slot);
}
void lsd_trace_val(lsdhip_ctx* c, int kind, int id, unsigned long long v) {
  if (!g_traceSums) return;
  if (c->dev.sums_meta.size() / 2 >= LSD_TRACE_SLOTS) return;
  c->dev.sums_meta.push_back(-kind); c->dev.sums_meta.push_back(id);
  c->dev.sums_host.push_back(v);
}
void lsd_trace_dump(lsdhip_ctx* c) {
  if (!g_traceSums || c->dev.sums_meta.empty()) return;
  const size_t n = c->dev.sums_meta.size() / 2;
  std::vector<unsigned long long> h(n, 0);
  if (c->dev.d_sums) (void)hipMemcpy(h.data(), c->dev.d_sums, n * 8, hipMemcpyDeviceToHost);
  if (FILE* f = fopen(g_traceSums, "a")) {
    for (size_t i = 0; i < n; i++) {
      const int kind = c->dev.sums_meta[2 * i];
      fprintf(f, "%d %d %016llx\n", kind < 0 ? -kind : kind, c->dev.sums_meta[2 * i + 1], kind < 0 ? c->dev.sums_host[i] : h[i]);
    }
    fclose(f);
  }
}
// Developer hook (LSDHIP_PIPE_GATE=1): forces the overlap the pipelined mode is about, whatever the host's pace — a DepthMap::updateKeyframe
// queued on the mapping stream holds (a one-lane spin, bounded) until the NEXT tracking job's launches are about to start, so that its
// kernels run exactly beside that job's first launches even when the caller is a slow Python loop (tools/pipe_overlap_debug.py).
static const bool g_pipeGate = getenv("LSDHIP_PIPE_GATE") != nullptr;
__global__ void k_gate_wait(const int* flag, int value) {
  if (threadIdx.x != 0) return;
  for (unsigned spins = 0; spins < (1u << 22); spins++) {
    if (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) >= value) return;
    __builtin_amdgcn_s_sleep(4);
  }
}
__global__ void k_gate_open(int* flag, int value) {
  if (threadIdx.x == 0) __hip_atomic_store(flag, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
int lsd_gate_wait(lsdhip_ctx* c) {
  if (!g_pipeGate || !c->pipeline) return LSDHIP_OK;
  if (!c->dev.d_gate) { if (int rc = lsd_dev_alloc_zeroed(c->dev.d_gate, 16)) return rc; }
  c->dev.gateWaited = c->dev.gateSeq + 1;
  hipLaunchKernelGGL(k_gate_wait, dim3(1), dim3(64), 0, c->mstream, c->dev.d_gate, c->dev.gateWaited);
  return LSDHIP_OK;
}
int lsd_gate_open(lsdhip_ctx* c) {
  if (!g_pipeGate || !c->pipeline) return LSDHIP_OK;
  if (!c->dev.d_gate) { if (int rc = lsd_dev_alloc_zeroed(c->dev.d_gate, 16)) return rc; }
  c->dev.gateSeq++;
  hipLaunchKernelGGL(k_gate_open, dim3(1), dim3(64), 0, c->stream, c->dev.d_gate, c->dev.gateSeq);
  return LSDHIP_OK;
}
#else
extern "C" void lsdhip_host_mark(int) {}      // (the C++ loop of include/lsd_slam_hip.hpp marks its phases: a no-op in the default library)
#endif   // LSD_DEVTOOLS
