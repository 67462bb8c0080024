// SE3Tracker on the device.  gfx950 only.
//
// One evaluation = one launch of k_track_step on the context's stream (described in front of the kernel's pieces below): every workgroup
// finishes the *previous* evaluation — the Levenberg-Marquardt decision of SE3Tracker::trackFrame with its 6x6 Gauss-Jordan solve
// (gj6_solve_wave) and SE3 exp, redundantly and identically, so the pose never leaves HBM between evaluations — and evaluates at the pose
// that gives: fused K0 (point generation from the keyframe planes) + K1 (warp / bilinear sample / mask) + K2 (weights) + K3 (normal equations).
// The host enqueues a budget of k_track_step launches back to back and synchronises once; steps launched
// after the job has finished return immediately.  A host-driven LM loop (one evaluation per round trip) is kept behind
// lsdhip_tracker.hostLM for debugging and as the kernel-level parity hook (lsdhip_tracker_evaluate).
//
// Reference behaviour restated:
//   TrackingReference::makePointCloud   C/Tracking/TrackingReference.cpp:128-138
//   SE3Tracker::calcResidualAndBuffers  C/Tracking/SE3Tracker.cpp:885-1029
//   SE3Tracker::calcWeightsAndResidualSSE  :492-575   (op order of the SSE path; _mm_rcp_ps -> IEEE 1/x)
//   SE3Tracker::calculateWarpUpdateSSE  :1033-1130 + LGS6::updateSSE / finish  C/Tracking/LGSX.h:205-386
//   SE3Tracker::trackFrame              :280-486
//   SE3Tracker::trackFrameOnPermaref    :162-272, checkPermaRefOverlap :121-157
//
// Quirks kept on purpose: the SSE loops ignore the last size%4 in-image points (in the reference's
// x-outer point order) for K2/K3 — emulated by the tail drop in front of the LM step (tail_drop, track_device.hpp); LGS6::updateSSE
// counts 6 constraints per group of 4; `LM_lambda <= 0.2` compares a float with a double.
//
// Data layout: keyframe planes idepth/idepthVar/image (3 x 4 B per pixel, row-major, coalesced per wave), tracked-frame
// texels float4 (gx, gy, I, 0) so that one bilinear tap is one 16-byte load.  Algorithmic bytes per evaluation at level l
// (SURVEY.md §8(d)): 20 N_l + [l==1] 5 N_l + 12 min(w_l h_l, 4 N_l).
#include <atomic>
#include <chrono>
#include "track_device.hpp"
#include "reposition_plan.hpp"   // the host stages of findRePositionCandidate (plain C++: tests/cpp/reposition_plan_test.cpp)

// developer build LSD_PHASE_TRACE: the functions that leave timestamps take the traced workgroup's flag and record (TRACE_PARAMS / _ARGS)
#ifdef LSD_PHASE_TRACE
#define PHASE_MARK(k) do { if (trOn_ && threadIdx.x == 0) tr_[k] = clock64(); } while (0)
#define LSD_TRACE_WORDS 32
#define TRACE_PARAMS , const bool trOn_, unsigned long long* const tr_
#define TRACE_ARGS , trOn_, tr_
#define TRACE_PUT(rec, who, k, v) do { if (trOn_ && threadIdx.x == (who)) (rec)[k] = (unsigned long long)(v); } while (0)
#define TRACE_LM_REC (trOn_ ? tr_ : nullptr)
// thread 0 of the traced workgroup takes the launch's record (32 words), clears it and stamps the start; everybody else gets the buffer's base
__device__ __forceinline__ unsigned long long* trace_open(unsigned long long* trace, const bool mine, unsigned long long** s_trp) {
  if (!mine) return trace;
  const unsigned long long n = trace[0];
  trace[0] = n + 1;
  unsigned long long* tr_ = trace + 1 + (n % 4096) * LSD_TRACE_WORDS;
  for (int k = 0; k < LSD_TRACE_WORDS; k++) tr_[k] = 0;
  tr_[8] = wall_clock64();
  tr_[24] = (unsigned long long)gridDim.x; tr_[25] = (unsigned long long)gridDim.y;
  *s_trp = tr_;
  return tr_;
}
#else
#define PHASE_MARK(k) do { } while (0)
#define TRACE_PARAMS
#define TRACE_ARGS
#define TRACE_PUT(rec, who, k, v) do { } while (0)
#define TRACE_LM_REC nullptr
#endif

#ifdef LSD_DEVTOOLS
// one record per launch, written by workgroup 0: which exit the launch took and the state it saw / left
#define LAUNCH_LOG(exitCode, pendingIn, ncandIn, pcUsed) do { \
    if (!BATCH && MODE == TS_FUSED && blockIdx.x == 0 && threadIdx.x == 0 && spec.dbgLog && spec.seq != 0) { \
      int* lg_ = spec.dbgLog + ((spec.seq & 0xFFF) * 16); \
      lg_[0] = spec.seq; lg_[1] = (exitCode); lg_[2] = parity | (first << 1) | (spec.last << 2); lg_[3] = lvlIn_; lg_[4] = (pendingIn); lg_[5] = (ncandIn); \
      lg_[6] = (pcUsed); lg_[7] = S.level; lg_[8] = S.numEvaluations; lg_[9] = S.numLaunches; lg_[10] = S.done; lg_[11] = S.phase; lg_[12] = S.incTry; \
      lg_[13] = S.ncand; lg_[14] = S.pending; lg_[15] = numLaunchesIn_; } } while (0)
#else
#define LAUNCH_LOG(exitCode, pendingIn, ncandIn, pcUsed) do { } while (0)
#endif

// Fused tracking step, one launch per step of the LM loop:
//   (1) every workgroup finishes the *previous* launch's evaluation(s) from the tiles' partial rows: fixed-order column sums
//       (row-major rows, whole rows per wave load, all loads issued before the first add), SSE tail drop, LGS6::finish, then
//       the LM decision in wave 0 — identical inputs, identical code, hence identical state in every workgroup without any
//       inter-workgroup communication inside the launch (no atomics, no fences, run-to-run deterministic).  The waves fetch
//       (or, on multi-pass levels, re-evaluate) the at most 3 tail points of every pending trial while the sums travel;
//   (2) the residual evaluation (K0+K1+K2+K3) of the pose(s) that decision produced, grid-stride over the level's pixels,
//       41 sums reduced lane -> workgroup (LDS, transposed) -> sums[.][trial][tile].
// Reject-chain speculation (single jobs, TS_FUSED; TrackSpec): the LM loop's retries after a rejection depend only on A, b
// and lambda, so (2) evaluates the next `trials` of them side by side — workgroup = (trial, tile); each trial group derives its
// lambda by the closed-form recurrence and solves for its own increment — and (1) of the next launch picks, lane-parallel, the
// first pending trial at which the reference's loop stops (diverged / accepted / step below stepSizeMin), advances lambda,
// incTry and the counters past the plain rejections before it, and runs ONE LM step on that trial's totals.  Same decisions,
// same evaluation counts, same refPixelWasGood as one evaluation per launch, in about half the dependent launches.
// The first launch of a job (first = 1) builds the initial state from the job instead of loading it.
// BATCH: blockIdx.y selects one of several independent jobs (tracking a batch of frames / permanent references in the
// same launches): the job descriptions then live in HBM (`jobs`), and state / scratch / summary are arrays over jobs.
// MODE (batches in throughput mode split a step into two launches, so that the LM replay is paid once per job instead of
// once per workgroup): TS_FUSED = finish + evaluate as described above; TS_LM = finish the pending evaluation and publish the
// state (grid.x = 1); TS_EVAL = evaluate the published state (reads st2[parity], writes scratch[parity]; no state change).
// The step is track_step_impl at the end of this part; the phases it runs, in the order it runs them, come first.
enum { TS_FUSED = 0, TS_LM = 1, TS_EVAL = 2 };
// the state a job's first launch starts from (SE3Tracker.cpp:280-320: the initial estimate, affine parameters of the settings, the top level)
__device__ __forceinline__ void track_state_begin(TrackState& S, const TrackJob& job, const int tid) {
  if (tid == 0) {
    S.T = job.T0;
    set_eval_pose(S, job.T0);
    S.aff_a = job.aff_a0; S.aff_b = job.aff_b0; S.aff_a_lastIt = job.aff_a0; S.aff_b_lastIt = job.aff_b0;
    S.lastErr = 0; S.LM_lambda = 0; S.last_residual = 0;
    S.level = job.topLevel; S.iteration = 0; S.incTry = 0; S.phase = 0; S.pending = 0;
    S.done = 0; S.diverged = 0; S.numEvaluations = 0; S.numWarpUpdates = 0;
    S.pointUsage = 0; S.goodCount = 0; S.badCount = 0; S.meanRes = 0;
    S.bytes = 0;
    for (int l = 0; l < LSD_LEVELS; l++) S.levelEvals[l] = 0;
    S.ncand = 1; S.lastCand = 0; S.numLaunches = 0;
  }
  if (tid < 36) S.A[tid] = 0;
  if (tid < 6) { S.b[tid] = 0; S.inc[tid] = 0; }
}

// Where this launch reads and writes in the scratch arena: the bases of its job and parities (trial 0; trial c sits c slots further).
struct StepAddr {
  const float *sums_in, *topval_in;
  float *sums_out, *topval_out;
  const int4* topkey_in; int4* topkey_out;
  const TrialRecord* recs_in;   // (no arena when cmax == 1: never dereferenced then)
  TrialRecord* recs_out;
  int max_rows, cmax;
};
template <bool BATCH, int MODE>
__device__ __forceinline__ StepAddr step_addr(const TrackScratch& sc, const int parity) {
  // every array is [job][parity][trial slot][...]: the slots this launch reads from and writes to, then each array's words per slot
  const size_t rows = (size_t)sc.max_rows, cm = (size_t)sc.cmax, job0 = BATCH ? (size_t)blockIdx.y * 2 * cm : 0;
  const size_t in = job0 + (size_t)parity * cm, out = job0 + (size_t)(MODE == TS_EVAL ? parity : 1 - parity) * cm;
  constexpr size_t TAIL = TAIL_ROWS * TAIL_STRIDE;
  return {sc.sums + in * RS_COLS * rows, sc.topval + in * rows * TAIL, sc.sums + out * RS_COLS * rows, sc.topval + out * rows * TAIL,
          sc.topkey + in * rows, sc.topkey + out * rows, sc.recs + in, sc.recs + out, sc.max_rows, sc.cmax};
}

// What this workgroup does in the launch: trial `cand` and tile (or strip) `bx` of the pending level; leader = workgroup 0, which publishes
// the state and writes the summary; leaves: nothing to do, gone before the finishing phase.
struct StepRole { int cand, bx; bool leader, leaves; };
template <bool BATCH, int MODE>
__device__ __forceinline__ void step_role(StepRole& r, const TrackJob& job, const TrackSpec& spec, const LevelFacts& lf, const int lvlPending, const int pending) {
  if (MODE == TS_FUSED && !BATCH) {
    // (as below, from the launch's own arguments.  cand = blockIdx.x / nbl without the division: a launch has at most LSD_SPEC_MAX trials, and
    // of a workgroup past the last of them — cand, bx stop at LSD_SPEC_MAX, blockIdx.x - LSD_SPEC_MAX nbl — all that is ever asked is that it is past them)
    const int nbl = lf.tiles_at(lvlPending), tr = lf.trials_at(lvlPending);
    int cand = 0;
#pragma unroll
    for (int k = 1; k <= LSD_SPEC_MAX; k++) cand += (int)blockIdx.x >= k * nbl ? 1 : 0;
    r.cand = cand; r.bx = (int)blockIdx.x - cand * nbl;
    const bool needTrial = pending ? cand < tr : cand == 0;
    const bool needNext = pending && lvlPending > lf.lastLevel && (int)blockIdx.x < lf.tiles_at(lvlPending > 0 ? lvlPending - 1 : 0);
    r.leaves = !r.leader && !needTrial && !needNext;
  }
  if (MODE == TS_FUSED && BATCH) {
    // The launch is sized for the level with the most (tiles x trials).  This one either evaluates trials at S.level —
    // workgroup = (trial, tile) of that level — or, if the pending decision ends the level, the first evaluation of
    // S.level - 1 (workgroup = tile).  Workgroups that have no work either way leave before the finishing phase (whose loads
    // they would only add to everybody else's).
    const int nbl = job.lv[lvlPending].nblocks;
    const int tr = trials_at(spec, lvlPending);
    r.cand = (int)blockIdx.x / nbl; r.bx = (int)blockIdx.x - r.cand * nbl;
    const bool needTrial = pending ? r.cand < tr : r.cand == 0;
    const bool needNext = pending && lvlPending > job.lastLevel && (int)blockIdx.x < job.lv[lvlPending - 1].nblocks;
    r.leaves = !r.leader && !needTrial && !needNext;
  }
  if (BATCH && MODE == TS_LM) {
    // one workgroup per (trial, job): workgroup `cand` proposes the cand-th retry down the reject chain; those without a trial leave
    r.cand = (int)blockIdx.x; r.bx = 0;
    r.leaves = !r.leader && !(pending && r.cand < trials_at(spec, lvlPending));
  }
  if (BATCH && MODE == TS_EVAL) {
    // workgroup = (trial, strip) of the job's level
    const int nbl = job.lv[lvlPending].nblocks;
    r.cand = (int)blockIdx.x / nbl; r.bx = (int)blockIdx.x - r.cand * nbl;
  }
}

// Throughput-mode strips (batches): the strip's list is the concatenation of its reference blocks (k_ref_blocks, frame.hip).  The loads —
// one block count per lane (at most 32 blocks), one word of four offsets per lane and step — depend on the level alone, not on the pose:
// a (trial, strip) workgroup that is going to evaluate at the pending level (the usual case; a level ends three times per job) requests
// them at the head of the finishing phase, so they travel with the previous round's partial sums instead of behind the LM step.
constexpr int STRIP_CHMAX = 8;                   // tilePx <= 8192 (fill_level): 32 blocks, 8 steps of 4 waves
__device__ __forceinline__ void strip_request(const TrackLevel& L, const int tile_, const int wave, const int lane, int& cntv, unsigned (&ow)[STRIP_CHMAX]) {
  const int px = L.w * L.h;
  const int base_ = tile_ * L.tilePx;
  const int b0_ = base_ >> 8;
  const int mblk_ = (min(base_ + L.tilePx, px) - base_ + 255) >> 8;
  const gbyte* offs = (const gbyte*)L.kf_refBlk;
  const __attribute__((address_space(1))) int* cnts = (const __attribute__((address_space(1))) int*)(offs + ((size_t)((px + 255) >> 8) << 8));
  cntv = lane < mblk_ ? cnts[b0_ + lane] : 0;
#pragma unroll
  for (int c = 0; c < STRIP_CHMAX; c++) {
    const int blk = c * 4 + wave;
    ow[c] = blk < mblk_ ? *(const __attribute__((address_space(1))) unsigned*)(offs + ((size_t)(b0_ + blk) << 8) + (lane << 2)) : 0u;
  }
}

// ---- the finishing phase: the tail points of the pending trials ------------------------------------------------------------
// The last (M % 4) in-image points in reference order = the largest keys (x * h + y, or list index) over all tiles' top-3 lists left
// behind by the residual pass — per trial, one wave per trial (two when there are more than four), the last wave first: it has no
// column sums to add.  What a wave finds goes to the trial's tail table: sub[trial] (TAIL_ROWS rows) and nsub[trial] (how many exist).
typedef float (*TailTable)[TAIL_ROWS][TAIL_STRIDE];
// the three largest of a wave's keys (KROWS int4 per lane: lane's rows lane, lane + 64, ...) and where they sit (row * 3 + slot)
template <int KROWS>
__device__ __forceinline__ void top3_of_keys(const int4 (&kv)[KROWS], const int lane, int (&keys)[3], int (&src)[3]) {
  Top3Payload top;
#pragma unroll
  for (int q = 0; q < KROWS; q++) {
    const int e = (lane + 64 * q) * 3;
    const int ks[3] = {kv[q].x, kv[q].y, kv[q].z};
#pragma unroll
    for (int rr = 0; rr < 3; rr++) top.insert(ks[rr], e + rr);
  }
#pragma unroll
  for (int r = 0; r < 3; r++) keys[r] = top.take(src[r]);
}
// a wave takes up to two trials (ca, cb; cb < 0: one): both key loads travel together, the second merge runs while the
// first trial's contributions travel, and on multi-pass levels the (up to 6) tail points are re-evaluated side by side
template <int KROWS>   // rows per lane: KROWS * 64 >= nb
__device__ __forceinline__ void tail_two(const TrackJob& job, const TrackState& S, const int level, const int nb, const StepAddr& A, const TrialRecord* s_rec,
                                         const TailTable s_subT, int* const s_nsubT, const int ca, const int cb, const int lane) {
  const int max_rows = A.max_rows;
  const int cbb = cb < 0 ? ca : cb;
  const int4* tka = A.topkey_in + (size_t)ca * max_rows;
  const int4* tkb = A.topkey_in + (size_t)cbb * max_rows;
  int4 kva[KROWS], kvb[KROWS];
#pragma unroll
  for (int q = 0; q < KROWS; q++) {
    const int row = lane + 64 * q;
    const int4 ka = tka[row < max_rows ? row : 0];   // unconditional, issued together
    const int4 kb = tkb[row < max_rows ? row : 0];
    kva[q] = row < nb ? ka : make_int4(-1, -1, -1, -1);
    kvb[q] = row < nb ? kb : make_int4(-1, -1, -1, -1);
  }
  // the owners of the keys left their K2/K3 contributions next to them: single-pass levels (one point per lane) and the strips of
  // a throughput-mode batch (the three largest keys of a strip are re-evaluated at the end of its launch)
  const bool single = job.lv[level].singlePass != 0 || job.lv[level].tilePx > 0;
  const int j = lane & 31, rj = lane >> 5;
  int keysA[3], srcA[3], keysB[3], srcB[3];
  float a0 = 0.f, a2 = 0.f, b0 = 0.f, b2 = 0.f;
  // word j of the rows the owners of a trial's keys left next to them: rows 0 and 1 in the two half-waves, row 2 in the lower one
  auto request = [&](const int c, const int (&keys)[3], const int (&src)[3], float& v0, float& v2) {
    const float* tv = A.topval_in + (size_t)c * max_rows * (TAIL_ROWS * TAIL_STRIDE);
    if (keys[rj] >= 0) v0 = tv[(size_t)src[rj] * TAIL_STRIDE + j];
    if (rj == 0 && keys[2] >= 0) v2 = tv[(size_t)src[2] * TAIL_STRIDE + j];
  };
  auto deliver = [&](const int c, const int (&keys)[3], const float v0, const float v2) {
    if (keys[rj] >= 0) s_subT[c][rj][j] = v0;
    if (rj == 0 && keys[2] >= 0) s_subT[c][2][j] = v2;
  };
  top3_of_keys(kva, lane, keysA, srcA);
  if (single && j < TAIL_WORDS) request(ca, keysA, srcA, a0, a2);
  if (cb >= 0) {
    top3_of_keys(kvb, lane, keysB, srcB);
    if (single && j < TAIL_WORDS) request(cb, keysB, srcB, b0, b2);
  }
  if (lane == 0) {
    s_nsubT[ca] = (keysA[0] >= 0) + (keysA[1] >= 0) + (keysA[2] >= 0);
    if (cb >= 0) s_nsubT[cb] = (keysB[0] >= 0) + (keysB[1] >= 0) + (keysB[2] >= 0);
  }
  if (single) {
    if (j < TAIL_WORDS) {
      deliver(ca, keysA, a0, a2);
      if (cb >= 0) deliver(cb, keysB, b0, b2);
    }
  } else {
    // multi-pass level: re-evaluate the tail points at their trial's pose: lanes 0..2 trial ca, 3..5 trial cb
    const bool second = lane >= 3;
    const int r = second ? lane - 3 : lane;
    const int c = second ? cb : ca;
    int key = -1;
    if (lane < 6 && c >= 0) key = second ? (r == 0 ? keysB[0] : (r == 1 ? keysB[1] : keysB[2])) : (r == 0 ? keysA[0] : (r == 1 ? keysA[1] : keysA[2]));
    if (key >= 0) {
      EvalCtx a;
      make_ctx_dev(job, S, level, a);
      if (c > 0) ctx_set_pose(a, s_rec[c]);
      const int idx = (a.npts >= 0) ? key : ((key / a.h) + (key % a.h) * a.w);
      float px, py, pz, I_ref, var;
      int maskIdx;
      fetch_point(a, idx, px, py, pz, I_ref, var, maskIdx);
      PointOut o;
      eval_point(a, px, py, pz, I_ref, var, o);
      tail_row(o, s_subT[c][r]);
    }
  }
}
// Strips of a throughput-mode batch, at most 24 per job: a strip's launch leaves one tail row per candidate — its (up to) three
// largest keys' K2/K3 contributions [0..28] and the key itself [31] — so ALL rows of the job travel in the same round trip as the
// partial sums (NQ 16-byte loads per lane), the three largest keys are picked from the rows in registers, and their rows go to the
// tail table: no second, dependent round trip (the keys first, then the owners' contributions) in front of the LM step.
static_assert(TAIL_STRIDE == 32 && TAIL_KEY == 31, "a tail row is eight 16-byte words; the key is the last word of the eighth");
// from the nf4 16-byte words of a job's rows (word f in v[f / 64] of lane f % 64) the three rows with the largest keys -> sub, their number -> nsub
template <int NQ>
__device__ __forceinline__ void tail_rows_pick(const float4 (&v)[NQ], const int nf4, float (*const sub)[TAIL_STRIDE], int* const nsubOut, const int lane) {
  Top3Payload top;
#pragma unroll
  for (int q = 0; q < NQ; q++) {
    const int f = q * 64 + lane;
    top.insert(((lane & 7) == 7 && f < nf4) ? __float_as_int(v[q].w) : -1, f >> 3);   // the row's key sits in its last word
  }
  int nsub = 0;
#pragma unroll
  for (int r = 0; r < 3; r++) {
    int row;
    const int m = top.take(row);
    if (m >= 0) {
      nsub++;
      // the row's 16-byte words sit in v[row / 8] of lanes 8 (row % 8) ..: a scalar branch per q (row is uniform).  (The empty asm
      // keeps the compiler from folding the branches into an indexed read of v[] — scratch memory; a chain of 4 (NQ - 1) selects
      // per candidate was the first form.)
      const int qsel = row >> 3;
#pragma unroll
      for (int q = 0; q < NQ; q++) {
        if (q == qsel) {
          float4 w4 = v[q];
          asm volatile("" : "+v"(w4.x), "+v"(w4.y), "+v"(w4.z), "+v"(w4.w));
          if ((lane >> 3) == (row & 7)) *(float4*)&sub[r][(lane & 7) * 4] = w4;
        }
      }
    }
  }
  if (lane == 0) *nsubOut = nsub;
}
template <int NQ>   // NQ * 64 >= nb * 24 (16-byte words of the rows)
__device__ __forceinline__ void tail_rows(const int nb, const StepAddr& A, const TailTable s_subT, int* const s_nsubT, const int ca, const int cb, const int lane) {
  const int cbb = cb < 0 ? ca : cb;
  const float4* ta = (const float4*)(A.topval_in + (size_t)ca * A.max_rows * (TAIL_ROWS * TAIL_STRIDE));
  const float4* tb = (const float4*)(A.topval_in + (size_t)cbb * A.max_rows * (TAIL_ROWS * TAIL_STRIDE));
  const int nf4 = nb * (TAIL_ROWS * TAIL_STRIDE / 4);
  float4 va[NQ], vb[NQ];
#pragma unroll
  for (int q = 0; q < NQ; q++) {
    const int f = q * 64 + lane;
    va[q] = ta[f < nf4 ? f : 0];   // unconditional, issued together
    vb[q] = tb[f < nf4 ? f : 0];
  }
  tail_rows_pick(va, nf4, s_subT[ca], &s_nsubT[ca], lane);
  if (cb >= 0) tail_rows_pick(vb, nf4, s_subT[cb], &s_nsubT[cb], lane);
}
// this wave's share of the tail work
template <bool BATCH, int WAVES>
__device__ __forceinline__ void gather_tails(const TrackJob& job, const TrackState& S, const int level, const int nb, const int ncandPending, const StepAddr& A,
                                             const TrialRecord* s_rec, const TailTable s_subT, int* const s_nsubT, const int wave, const int lane) {
  // trial c -> wave WAVES-1 - (c mod WAVES): the last wave first (it has no column sums to add)
  const int ca = WAVES - 1 - wave;
  const int cb = ca + WAVES < ncandPending ? ca + WAVES : -1;
  if (ca < ncandPending) {
    if (BATCH && job.lv[level].tilePx > 0 && nb <= 24) {
      if (nb <= 5) tail_rows<2>(nb, A, s_subT, s_nsubT, ca, cb, lane);
      else if (nb <= 13) tail_rows<5>(nb, A, s_subT, s_nsubT, ca, cb, lane);
      else tail_rows<9>(nb, A, s_subT, s_nsubT, ca, cb, lane);
    } else if (nb <= 128) tail_two<2>(job, S, level, nb, A, s_rec, s_subT, s_nsubT, ca, cb, lane);
    else tail_two<5>(job, S, level, nb, A, s_rec, s_subT, s_nsubT, ca, cb, lane);
  }
}

// ---- the finishing phase: column sums ---------------------------------------------------------------------------------------
// Fixed-order column sums over the tiles' partial rows (row-major [tile][RS_COLS]: a wave's load covers whole rows, i.e.
// contiguous memory): thread t < NSLOT * 11 takes columns 4 c4 .. 4 c4 + 3 of rows slot, slot + NSLOT, ... , for every
// trial (the other lanes of these waves run along and store nothing: the tail work behind it is wave-wide).
constexpr int SUM_NSLOT = 16;                                // row slots of the column sums: slot s adds rows s, s + 16, ...
constexpr int SUM_QMAX = 20;                                 // float4 loads per thread: rows per slice <= 80
typedef float (*SumTable)[SUM_NSLOT][RS_COLS];               // per pending trial: column sums by row slot
// Q rows per slot, NT trials from `base` on: the loads are unconditional and issued together (trials past the last one re-read it, rows past
// the last one re-read the slot's first row)
template <int Q, int NT>
__device__ __forceinline__ void colsum(const float4* p, const size_t trialStrideF4, const int nb, const int ncandPending, const int base,
                                       const int slot, const int c4, const bool sumLane, const SumTable s_sumT) {
  constexpr int NSLOT = SUM_NSLOT;
  const int K = (nb + NSLOT - 1) / NSLOT;                // rows per slot
  float4 v[NT][Q];
#pragma unroll
  for (int c = 0; c < NT; c++) {
    const int pc = base + c < ncandPending ? base + c : ncandPending - 1;
    const float4* pp = p + (size_t)pc * trialStrideF4;
#pragma unroll
    for (int q = 0; q < Q; q++) {
      const int r = slot + NSLOT * q;
      v[c][q] = pp[(size_t)(r < nb ? r : slot) * (RS_COLS / 4)];
    }
  }
#pragma unroll
  for (int c = 0; c < NT; c++) {
    float4 a4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int q = 0; q < Q; q++) {
      const bool live = q < K && slot + NSLOT * q < nb;
      a4.x += live ? v[c][q].x : 0.f;
      a4.y += live ? v[c][q].y : 0.f;
      a4.z += live ? v[c][q].z : 0.f;
      a4.w += live ? v[c][q].w : 0.f;
    }
    if (sumLane && base + c < ncandPending) *(float4*)&s_sumT[base + c][slot][c4 * 4] = a4;
  }
}
// coarse levels (few tiles) take the short forms
template <int TRIALS_MAX>
__device__ __forceinline__ void column_sums(const StepAddr& A, const int nb, const int ncandPending, const int t, const SumTable s_sumT) {
  constexpr int NSLOT = SUM_NSLOT, QMAX = SUM_QMAX;
  const int slot_ = t / (RS_COLS / 4); const bool sumLane = slot_ < NSLOT;
  const int slot = sumLane ? slot_ : 0, c4 = sumLane ? t - slot_ * (RS_COLS / 4) : 0;
  const int K = (nb + NSLOT - 1) / NSLOT;                // rows per slot
  const float4* p = (const float4*)A.sums_in + c4;
  const size_t trialStrideF4 = (size_t)RS_COLS * A.max_rows / 4;
  if (ncandPending == 1) {
    if (K <= 2) colsum<2, 1>(p, trialStrideF4, nb, ncandPending, 0, slot, c4, sumLane, s_sumT);
    else if (K <= 5) colsum<5, 1>(p, trialStrideF4, nb, ncandPending, 0, slot, c4, sumLane, s_sumT);
    else if (K <= 10) colsum<10, 1>(p, trialStrideF4, nb, ncandPending, 0, slot, c4, sumLane, s_sumT);
    else colsum<QMAX, 1>(p, trialStrideF4, nb, ncandPending, 0, slot, c4, sumLane, s_sumT);
  } else if (K <= 2) colsum<2, TRIALS_MAX>(p, trialStrideF4, nb, ncandPending, 0, slot, c4, sumLane, s_sumT);
  else if (K <= 5) colsum<5, TRIALS_MAX>(p, trialStrideF4, nb, ncandPending, 0, slot, c4, sumLane, s_sumT);
  else if (K <= 10) { for (int base = 0; base < ncandPending; base += 3) colsum<10, 3>(p, trialStrideF4, nb, ncandPending, base, slot, c4, sumLane, s_sumT); }
  else { for (int base = 0; base < ncandPending; base++) colsum<QMAX, 1>(p, trialStrideF4, nb, ncandPending, base, slot, c4, sumLane, s_sumT); }
}
// the finishing phase's tables in `buf`, per pending trial: column sums by row slot | its (up to 3) tail rows | how many of them exist |
// the column totals over the slots
typedef float (*TotalTable)[RS_COLS];
template <int TRIALS_MAX>
struct FinishTables {
  enum { WORDS = TRIALS_MAX * (SUM_NSLOT * RS_COLS + TAIL_ROWS * TAIL_STRIDE + 1 + RS_COLS) };
  SumTable sum; TailTable sub; int* nsub; TotalTable tot;
  __device__ __forceinline__ explicit FinishTables(float* buf)
      : sum((SumTable)buf), sub((TailTable)(buf + TRIALS_MAX * SUM_NSLOT * RS_COLS)), nsub((int*)(buf + TRIALS_MAX * (SUM_NSLOT * RS_COLS + TAIL_ROWS * TAIL_STRIDE))),
        tot((TotalTable)(buf + TRIALS_MAX * (SUM_NSLOT * RS_COLS + TAIL_ROWS * TAIL_STRIDE + 1))) {}
};
// total of column `col` of trial c over the row slots, in slot order
__device__ __forceinline__ float slot_total(const SumTable s_sumT, const int c, const int col) {
  float s = s_sumT[c][0][col];
#pragma unroll
  for (int k = 1; k < SUM_NSLOT; k++) s += s_sumT[c][k][col];
  return s;
}
// all pending trials' totals at once, thread (trial, column) — TRIALS_MAX x RS_END threads of the workgroup — so that wave 0 reads a total
// where it used to add sixteen slots, three times one behind the other, while the other waves waited for it.  A barrier follows.
template <int TRIALS_MAX, int BLOCK>
__device__ __forceinline__ void slot_totals(const SumTable s_sumT, const TotalTable s_totT, const int ncandPending, const int tid) {
  static_assert(TRIALS_MAX * RS_END <= BLOCK, "a thread per (trial, column)");
  const int c = tid / RS_END, col = tid - c * RS_END;
  if (c < ncandPending) s_totT[c][col] = slot_total(s_sumT, c, col);
}

// ---- the finishing phase: wave 0 ------------------------------------------------------------------------------------------------
// Which pending trial does the LM loop stop at?  Trial c stops it when it diverges (M < minWarped), is accepted
// (error < lastErr) or is rejected with a step below stepSizeMin — each test needs only that trial's own totals and
// increment, so lane c answers for trial c and the first "yes" wins.  The trials before it were plain rejections: they
// leave nothing behind but lambda, incTry and the counters, which are advanced in closed form; then ONE LM step runs,
// on the totals of the trial that stopped the loop (or of the last pending one).
__device__ __forceinline__ int pick_trial(TrackState& S, const LmPar& par, const int level, const int ncandPending, const TotalTable s_totT, const TailTable s_subT,
                                          const int* s_nsubT, const TrialRecord* s_rec, const int tid) {
  if (ncandPending <= 1) return 0;
  const int c = tid < ncandPending ? tid : 0;
  const int Mc = (int)s_totT[c][RS_M];
  const float ws = tail_drop(s_totT[c][RS_WERR], Mc, s_nsubT[c], tail_word(RS_WERR), s_subT[c]);
  const float werrc = lm_werr(ws, Mc);
  const float incdot = inc_norm2(c == 0 ? S.inc : s_rec[c].inc);
  const bool stop = Mc < par.minWarped || werrc < S.lastErr || !(incdot > par.stepSizeMin);
  const unsigned long long sm = __ballot(stop && tid < ncandPending);
  const int pc = sm ? (int)__ffsll((long long)sm) - 1 : ncandPending - 1;
  if (pc > 0) {
    float lam = S.LM_lambda;
    const int it0 = S.incTry;
    double failPow = lambda_fail_pow(it0, par.lambdaFailFac);
    for (int j = 0; j < pc; j++) { lam = lm_lambda_fail_pow(lam, failPow); failPow *= (double)par.lambdaFailFac; }
    // algorithmic bytes of the skipped evaluations (as in lm_wave)
    const float skipped = eval_bytes(s_totT[0][RS_NREF], par);
    const float bytes0 = S.bytes;
    const int ne0 = S.numEvaluations, le0 = S.levelEvals[level];
    float bytes1 = bytes0;
    for (int j = 0; j < pc; j++) bytes1 = bytes1 + skipped;
    S.LM_lambda = lam;
    S.incTry = it0 + pc;
    S.numEvaluations = ne0 + pc;
    if (tid == 0) S.levelEvals[level] = le0 + pc;
    S.bytes = bytes1;
    trial_record_adopt(S, s_rec[pc], tid);
  }
  return pc;
}
// column totals and tail-drop correction of trial pc, one column per lane (0 in the lanes past the columns)
__device__ __forceinline__ float finish_totals(const TotalTable s_totT, const TailTable s_subT, const int* s_nsubT, const int pc, const int tid) {
  const int M = (int)s_totT[pc][RS_M];
  const float s = tid < RS_END ? s_totT[pc][tid] : 0.f;
  return tail_drop(s, M, s_nsubT[pc], tail_word(tid), s_subT[pc]);
}
// the frame's refPixelWasGood must be what the last trial the LM loop executed wrote: trials > 0 wrote side planes
template <int BLOCK>
__device__ __forceinline__ void copy_side_mask(const TrackJob& job, const TrackState& S, const TrackSpec& spec, const int level, const int bx, const int nb, const int tid) {
  const uint8_t* side = spec.wasGoodSide + (size_t)(S.lastCand - 1) * spec.maskStride;
  EvalCtx a;
  make_ctx_dev(job, S, level, a);
  const int work = a.npts >= 0 ? a.npts : a.w * a.h;
  for (int i = bx * BLOCK + tid; i < work; i += nb * BLOCK) {
    float px, py, pz, I_ref, var;
    int maskIdx;
    if (fetch_point(a, i, px, py, pz, I_ref, var, maskIdx) && maskIdx >= 0) job.wasGood[maskIdx] = side[maskIdx];
  }
}

// ---- the residual evaluation, three forms: every lane adds its points' contributions to acc[] and keeps their three largest keys ------
// Throughput mode (batches): the workgroup owns a strip of tilePx consecutive pixels of the keyframe level.  It first
// compacts the strip's valid reference pixels (semi-dense: ~30 %) into an LDS list — fixed order: chunk, then pixel
// slot, then lane, so the result is run-to-run deterministic — and then evaluates the list with all lanes busy.
// The strip's list is the concatenation of its reference blocks (k_ref_blocks, frame.hip: per 256 consecutive pixels the offsets of the
// valid ones, compacted in pixel order, and a count): wave v takes block 4 c + v of the strip in step c, lane l its slots l, l + 64, ...;
// every wave derives the blocks' places in the list from the counts itself (at most 32 blocks: one lane each), so nothing is exchanged
// and the only barrier is the one in front of the evaluation.  (Until round 6 the strip streamed the level's validity planes, 8 bytes per
// pixel, and compacted them with four ballots per 1024 pixels in every evaluation: a quarter of a level-1 round at 64 jobs.)
// cntv / ow: the strip's block counts and offset words (strip_request).  Two barriers: the list is complete | the list is read.
template <int BLOCK>
__device__ __forceinline__ void eval_strip(const EvalCtx& a, const int tilePx, const int tile, const int work, const int cntv, const unsigned (&ow)[STRIP_CHMAX],
                                           unsigned* const s_list /* (x | y << 16) */, gbyte* const wasGood, float (&acc)[RS_END], int& key0, int& key1, int& key2,
                                           const int tid TRACE_PARAMS) {
  const int wave = tid >> 6, lane = tid & 63;
  const int base = tile * tilePx;
  const int stripEnd = min(base + tilePx, work);
  const int b0 = base >> 8;                                  // strips are multiples of 256 pixels
  const int mblk = (stripEnd - base + 255) >> 8;             // <= 32 (tilePx <= 8192, fill_level)
  const float inv_w = 1.0f / (float)a.w;
  // inclusive scan of the (at most 32) block counts over lanes 0..31, the blocks' entries through v_readlane (the
  // wave index is uniform: readfirstlane tells the compiler so)
  const int incl = wave_scan32(cntv);
  const int total = __builtin_amdgcn_readlane(incl, 31);
  const int waveU = __builtin_amdgcn_readfirstlane(wave);
  PHASE_MARK(20);
#pragma unroll
  for (int c = 0; c < STRIP_CHMAX; c++) {
    const int blk = c * 4 + waveU;
    if (blk < mblk) {
      const int cb = __builtin_amdgcn_readlane(cntv, blk);
      const int pb = __builtin_amdgcn_readlane(incl, blk) - cb;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int sl = lane + 64 * k;                       // (the block's bytes are slot-interleaved: k_ref_blocks)
        if (sl < cb) s_list[pb + sl] = pixel_xy16(((b0 + blk) << 8) + (int)((ow[c] >> (8 * k)) & 255u), a.w, inv_w);
      }
    }
  }
  __syncthreads();
  PHASE_MARK(21);
  TRACE_PUT(tr_, 0, 23, total);
  if (total > 0) {
    // three-stage software pipeline over the list entries tid, tid + BLOCK, ...: (A) list entry + keyframe planes,
    // (B) reference point, warp, texel fetch, (C) residual / weights / normal equations.  Stage A of entry r + 2 and
    // stage B of entry r + 1 are issued before stage C of entry r, so two dependent memory round trips overlap the
    // arithmetic.  Lanes past the end of the list run the loads on entry 0 and discard them.
    struct StA { unsigned xy; float var, id, img; bool live; };
    struct StB { unsigned xy; float pz, I_ref, var; PointWarp q; PointTexels t; bool live; };
    auto stageA = [&](int p, StA& A) {
      A.live = p < total;
      A.xy = s_list[A.live ? p : 0];
      const int i = __mul24((int)(A.xy >> 16), a.w) + (int)(A.xy & 0xffffu);
      A.var = a.kf_idepthVar[i];
      A.id = a.kf_idepth[i];
      A.img = a.kf_image[i];
    };
    auto stageB = [&](const StA& A, StB& B) {
      B.live = A.live;
      B.xy = A.xy;
      float px, py;
      ref_point_at(a, (int)(A.xy & 0xffffu), (int)(A.xy >> 16), A.id, px, py, B.pz);
      B.I_ref = A.img; B.var = A.var;
      eval_warp(a, px, py, B.pz, B.q);
      eval_fetch(a, B.q, B.live && B.q.in_image, B.t);
    };
    const int rounds = (total + BLOCK - 1) / BLOCK;
    StA A1, A2;
    StB B0, B1;
    stageA(tid, A1);
    stageB(A1, B0);
    stageA(tid + BLOCK, A1);
    PHASE_MARK(22);
    auto stageC = [&](const StB& B) {
      if (B.live) {
        const int x_ = (int)(B.xy & 0xffffu), y_ = (int)(B.xy >> 16);
        visit_point(a, B.q, B.t, B.pz, B.I_ref, B.var, wasGood, __mul24(y_, a.w) + x_, __mul24(x_, a.h) + y_, acc, key0, key1, key2);
      }
    };
    // two rounds per trip with the roles of (A1, A2) and (B0, B1) swapped in the second half: a rotating pipeline written with
    // struct copies costs ~30 register moves per round
    for (int r = 0; r < rounds; r += 2) {
      stageB(A1, B1);
      stageA(tid + (r + 2) * BLOCK, A2);
      stageC(B0);
      stageB(A2, B0);
      stageA(tid + (r + 3) * BLOCK, A1);
      stageC(B1);                       // entry r + 1: not live past the end of the list
    }
  }
  __syncthreads();   // the list aliases s_red
}
// Multi-pass dense level of a single job (the host sets the flag: plan_job / fill_level): the lane's points i0, i0 + s, ... (s = nb x
// BLOCK) are taken four at a time.  In the plain loop below every load sits behind a branch on the one before it (the validity planes,
// then the keyframe colour, then the four texels behind in_image), so a lane makes 2 - 3 dependent memory round trips per point, one
// point after the other: at 640x480 level 1 that is four points per lane and a third of the launch's body.  Here the
// round trips of a group travel together: (1) the three plane loads of all four points, unconditional — a point past the end of the
// level reads pixel 0 and is dropped; (2) for all four: validity, the reference point, the warp, the texel loads (texel 0 where the
// point is not in the image); (3) in pass order what the plain loop does with a point, so every lane adds the same contributions in
// the same order and the partial rows, keys and mask bytes are those of the plain loop bit for bit.  (x, y) of the later points
// follow from the first by the uniform stride: one integer division per lane instead of one per point.
__device__ __forceinline__ void eval_groups_of_four(const EvalCtx& a, int i, const int stride, const int work, gbyte* const wasGood, float (&acc)[RS_END],
                                                    int& key0, int& key1, int& key2) {
  // (quotient and remainder by w as pixel_xy16 takes them: a float product and a correction, exact for every index of a level, in front of
  // the first plane load where two integer divisions were ~60 dependent instructions)
  const float inv_w = frcp((float)a.w);
  const unsigned sxy = pixel_xy16(stride, a.w, inv_w), ixy = pixel_xy16(i, a.w, inv_w);
  const int sy = (int)(sxy >> 16), sx = (int)(sxy & 0xFFFFu);   // uniform; sx < w: one carry at most
  int x = (int)(ixy & 0xFFFFu), y = (int)(ixy >> 16);
  struct Pt { int i, x, y; bool valid; RefPlanes r; float img, pz; PointWarp q; PointTexels t; };
  while (i < work) {
    Pt P[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      Pt& p = P[k];
      p.i = i; p.x = x; p.y = y;
      p.valid = i < work;
      const int li = p.valid ? i : 0;
      fetch_request(a, li, p.r);
      p.img = a.kf_image[li];
      i += stride; x += sx; y += sy;
      if (x >= a.w) { x -= a.w; y++; }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      Pt& p = P[k];
      float px = 0.f, py = 0.f;
      p.pz = 1.f;
      p.valid = p.valid && ref_pixel_inside(a, p.x, p.y) && fetch_finish(a, p.x, p.y, p.r, px, py, p.pz);
      eval_warp(a, px, py, p.pz, p.q);
      eval_fetch(a, p.q, p.valid && p.q.in_image, p.t);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const Pt& p = P[k];
      if (p.valid) visit_point(a, p.q, p.t, p.pz, p.img, p.r.var, wasGood, p.i, p.x * a.h + p.y, acc, key0, key1, key2);
    }
  }
}
// the plain loop: one point after the other (explicit point lists, single-pass levels, small batches)
__device__ __forceinline__ void eval_plain(const EvalCtx& a, const int i0, const int stride, const int work, gbyte* const wasGood, float (&acc)[RS_END],
                                           int& key0, int& key1, int& key2) {
  for (int i = i0; i < work; i += stride) {
    float px, py, pz, I_ref, var;
    int maskIdx;
    if (fetch_point(a, i, px, py, pz, I_ref, var, maskIdx)) {
      PointWarp q; PointTexels t;
      eval_warp(a, px, py, pz, q);
      if (q.in_image) eval_fetch(a, q, true, t);
      visit_point(a, q, t, pz, I_ref, var, maskIdx >= 0 ? wasGood : nullptr, maskIdx, a.npts >= 0 ? i : (i % a.w) * a.h + (i / a.w), acc, key0, key1, key2);
    }
  }
}

// ---- reduction and publish ----------------------------------------------------------------------------------------------------
// Workgroup reduction through LDS: every lane parks its 41 accumulators in column `tid` of s_red (row stride
// BLOCK + 1: conflict-free both ways), then thread (slice, k) adds a contiguous run of lanes of row k in lane order
// and 41 threads add the slices — ~130 instructions per wave instead of 41 x 7 DPP steps.  The tile's row of sums, its three largest
// keys and (single-pass levels, strips) its tail rows go to the trial's slots sums_out / topkey_out / topval_out.
// The workgroup reduction handles the columns in NPASS batches (2 halves the LDS; measured slower — also for the throughput-mode
// evaluation, where it would let four workgroups share a CU: profiles/r05_notes.md)
constexpr int RED_NPASS = 1;
constexpr int RED_CPP = (RS_END + RED_NPASS - 1) / RED_NPASS;      // columns per batch
template <int BLOCK, bool BATCH, int MODE>
__device__ __forceinline__ void reduce_and_store(const EvalCtx& a, const TrackLevel& L, TrackState& S, const int tile, const float (&acc)[RS_END],
                                                 const int key0, const int key1, const int key2, float* const s_red, float (*const s_sum)[64], int (*const s_wtop)[3],
                                                 int* const s_top, float* const sums_out, int4* const topkey_out, float* const topval_out, const int tid) {
  constexpr int NPASS = RED_NPASS, CPP = RED_CPP;
  constexpr int RSLICE = BLOCK / CPP;                  // slices per row
  constexpr int RRUN = (BLOCK + RSLICE - 1) / RSLICE;  // lanes per slice
  // Strips of a throughput-mode batch: the (up to) three in-image points of the strip with the largest reference-order keys are
  // candidates for the job's tail (the last M % 4 in-image points, which the SSE loops of the reference leave out): three lanes evaluate
  // them once more, alone, and leave their K2/K3 contributions in the strip's candidate rows — the launch that finishes this evaluation
  // then needs no evaluation of its own in front of the LM step (it used to: keys, reference point, texels = three dependent round
  // trips).  The two round trips of this evaluation run under the barriers of the reduction.
  const bool stripRows = BATCH && L.tilePx > 0;
  const bool candLane = tid >= BLOCK - 64 && tid < BLOCK - 61;   // lanes 0..2 of the LAST wave: wave 0 adds the slices and stores the sums meanwhile
  TailCandidate c;
  float cPz = 0.f;
  PointWarp cq; PointTexels ct;
  if (stripRows) {
    block_top3(key0, key1, key2, s_wtop, s_top);
    if (candLane) c.request(a, s_top[tid - (BLOCK - 64)]);
  } else {
    // tiles: the keys need no barriers of their own — every wave's three largest go out before the reduction's first barrier, the last
    // wave merges them between its two (block_top3 in two halves)
    wave_top3(key0, key1, key2, s_wtop);
  }
#pragma unroll
  for (int hp = 0; hp < NPASS; hp++) {
    if (hp > 0) __syncthreads();
#pragma unroll
    for (int k = 0; k < CPP; k++)
      if (hp * CPP + k < RS_END) s_red[k * (BLOCK + 1) + tid] = acc[hp * CPP + k];
    __syncthreads();
    // (S.pending = 1 / S.numLaunches++ for the state this launch publishes are set here, behind the first barrier of the reduction, and not
    // where the evaluation begins: in a job's first launch the finishing phase is skipped, so no barrier separates a wave that is still
    // about to test `S.pending` from wave 0 arriving there — with the write there, a wave held up by LDS traffic of another stream's
    // workgroups on the same CU could read 1, enter the finishing phase alone and pair its barriers with the others' reduction barriers:
    // one tile's sums came out as LDS residue.  Seen only with a second stream active, profiles/r04_notes.md.)
    if (MODE == TS_FUSED && hp == 0 && tid == 0) { S.pending = 1; S.numLaunches = S.numLaunches + 1; }   // every wave is past its reads of S.pending
    if (stripRows && hp == 0 && candLane && c.key >= 0) {
      float px, py;
      ref_point_at(a, c.x, c.y, c.id, px, py, cPz);
      eval_warp(a, px, py, cPz, cq);
      eval_fetch(a, cq, cq.in_image, ct);
    }
    {
      const int slice = tid / CPP, k = tid - slice * CPP;
      if (slice < RSLICE) s_sum[slice][k] = slice_sum<BLOCK + 1, RRUN>(s_red, k, slice);
    }
    if (!stripRows && hp == 0 && tid >= BLOCK - 64) {
      int top[3];
      merge_top3(s_wtop, BLOCK / 64, top);
#pragma unroll
      for (int r = 0; r < 3; r++)
        if (tid == BLOCK - 64) s_top[r] = top[r];
    }
    __syncthreads();
    if (stripRows && hp == 0 && candLane) {
      float* row = topval_out + (size_t)(tile * TAIL_ROWS + (tid - (BLOCK - 64))) * TAIL_STRIDE;
      if (c.key >= 0) {
        PointOut o;
        eval_finish(a, cq, ct, cPz, c.img, c.var, o);
        tail_row(o, row);
      }
      ((int*)row)[TAIL_KEY] = c.key;
    }
    if (tid < CPP && hp * CPP + tid < RS_END) {
      float s = s_sum[0][tid];
#pragma unroll
      for (int sl = 1; sl < RSLICE; sl++) s += s_sum[sl][tid];
      sums_out[(size_t)tile * RS_COLS + (hp * CPP + tid)] = s;
    }
  }
  if (tid == 0) topkey_out[tile] = make_int4(s_top[0], s_top[1], s_top[2], -1);
  if (L.singlePass && key0 >= 0) {
    // one point per lane: its accumulators are exactly its K2/K3 contributions (0 + x == x)
    const int r = key0 == s_top[0] ? 0 : (key0 == s_top[1] ? 1 : (key0 == s_top[2] ? 2 : -1));
    if (r >= 0) tail_row_from_sums(acc, topval_out + (size_t)(tile * TAIL_ROWS + r) * TAIL_STRIDE);
  }
}

#ifdef LSD_ORDER_CHECK
// developer build: do all workgroups of this launch finish the previous evaluation with the same totals?
__device__ __forceinline__ void order_check_totals(const TrackSpec& spec, const float s, const int pc, const int tid) {
  unsigned hv = tid < RS_END ? __float_as_uint(s) * (2654435761u * (unsigned)(tid + 1)) : 0u;
  hv += (unsigned)pc * 97u;
  for (int off = 32; off > 0; off >>= 1) hv += __shfl_xor(hv, off);
  if (tid == 0) {
    const unsigned long long slot = 8 + 2 * ((spec.dbgCum / 400ull) % 8192ull);
    __hip_atomic_fetch_min(&spec.dbgCounters[slot], (unsigned long long)hv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(&spec.dbgCounters[slot + 1], (unsigned long long)hv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
#endif

// The job description travels in the kernel arguments, which the host has just written: the first touch of each of its
// cache lines misses down to HBM (~1 us), and the fields of lv[level] are addressed only once the level is known, i.e. in
// the middle of the dependent chain.  Touch every line now, together with the loads of the prologue.
__device__ __forceinline__ void warm_job_arguments() {
  typedef const unsigned __attribute__((address_space(4))) cuint;
  cuint* ka = (cuint*)__builtin_amdgcn_kernarg_segment_ptr();
  unsigned warm = 0;
#pragma unroll
  for (int i = 0; i < (int)(sizeof(TrackJob) / 4); i += 32) warm ^= ka[i];
  asm volatile("" ::"s"(warm));   // the loads complete here, in the shadow of the prologue's own argument loads
}

// ---- the step ------------------------------------------------------------------------------------------------------------------
// Every early return and every barrier of the finishing phase is in this body; the strip evaluation (eval_strip) has two barriers of its
// own and the reduction (reduce_and_store, block_top3 inside it) has its own: all waves of a workgroup that get past the last return
// reach each of them.
template <int BLOCK, bool BATCH, int MODE>
__device__ __forceinline__ void track_step_impl(const TrackJob& jobv, const TrackJob* __restrict__ jobs, TrackState* __restrict__ st2,
                                                TrackScratch sc, TrackSummary* __restrict__ out, int parity, int first, const TrackSpec& spec) {
  const TrackJob& job = BATCH ? jobs[blockIdx.y] : jobv;
  if (!BATCH) warm_job_arguments();
  if (BATCH) { st2 += 2 * (size_t)blockIdx.y; out += blockIdx.y; }
  const StepAddr A = step_addr<BATCH, MODE>(sc, parity);
  LevelFacts lf = {0ull, 0u, 0};
  if (!BATCH) {
    lf = {spec.levelTiles, spec.levelTrials, job.lastLevel};
    asm volatile("" ::"s"(lf.tiles), "s"(lf.trials), "s"(lf.lastLevel));   // in registers here, with the other argument loads
  }
  constexpr int WAVES = BLOCK / 64, SUMW = WAVES - 1;                       // SUMW waves sum partials (the last one does the tail work)
  constexpr int NSLICE = (SUMW * 64) / RS_END, CPP = RED_CPP, RSLICE_ = BLOCK / CPP;   // row slices per column: of the column sums, of the reduction
  __shared__ TrackState S;
  __shared__ LmShared sh;
  __shared__ LmPar s_par;
  __shared__ float s_sum[(NSLICE > RSLICE_ ? NSLICE : RSLICE_)][64];
  __shared__ __attribute__((aligned(16))) float s_red[CPP * (BLOCK + 1) + 8];
  __shared__ int s_wtop[WAVES][3];
  __shared__ int s_top[3];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  // reject-chain speculation (single jobs): workgroup = (trial `cand`, tile `bx`) of the level of the pending evaluation —
  // fixed below (step_role), once the state says which level that is
  StepRole role = {0, (int)blockIdx.x, blockIdx.x == 0, false};
  const bool leader = role.leader;
  TrackState* next = st2 + (1 - parity);
  // trials a launch can finish: single jobs up to LSD_SPEC_MAX; batches in throughput mode up to LSD_BATCH_SPEC_MAX (the LM launch has one
  // workgroup per (trial, job): each proposes its own retry, as the trial groups of a single job's launch do); small batches one
  constexpr int TRIALS_MAX = BATCH ? (MODE == TS_EVAL ? 1 : LSD_BATCH_SPEC_MAX) : LSD_SPEC_MAX;
  constexpr bool SPEC_LM = MODE != TS_EVAL;
  // The finishing phase's per-trial tables live in the reduction buffer s_red: neither the strip list nor the reduction is live before the
  // barrier that ends the LM step, and nothing of these tables is read after it — so a launch that can finish four (batches) or six
  // (single jobs) trials needs no more LDS than one that finishes one (three workgroups per CU stay three).
  static_assert(FinishTables<TRIALS_MAX>::WORDS <= CPP * (BLOCK + 1) + 8, "the finishing phase's tables must fit the reduction buffer");
  const FinishTables<TRIALS_MAX> ft(s_red);
  __shared__ TrialRecord s_rec[TRIALS_MAX];                 // per pending trial > 0: its increment and pose
#ifdef LSD_PHASE_TRACE
  __shared__ unsigned long long* s_trp;
  // the traced workgroup: workgroup LSDHIP_TRACE_WG (default 0, the leader) of the job (batches: of job 0; tools/phase_trace_batch.py).  A
  // workgroup other than the leader shows what the leader skips: the early return's load in the prologue, and the trials > 0.
  const bool trOn_ = sc.trace != nullptr && (int)blockIdx.x == spec.traceWg && (!BATCH || blockIdx.y == 0);
  unsigned long long* const tr_ = trace_open(sc.trace, trOn_ && tid == 0, &s_trp);
#endif
  PHASE_MARK(0);
  if (!BATCH && MODE == TS_FUSED && leader && tid == 0 && spec.seq != 0) out->seq = spec.seq;   // pinned host memory: fire and forget
  if (first) {
    track_state_begin(S, job, tid);
  } else {
    // One memory round trip: the state, the trial records and (workgroups that are not the leader) the state's `done` word for the early
    // return are all requested before anything waits — unconditional loads at clamped indices into registers, the LDS stores behind the
    // return.  (One after the other they were three cold trips in every workgroup but the leader, which has no early return.)
    constexpr int NSTATE = (int)(sizeof(TrackState) / 4), NREC = (int)(sizeof(s_rec) / 4);
    static_assert(NSTATE <= BLOCK && NREC <= BLOCK, "one word of the state and one of the records per thread");
    const bool haveRecs = SPEC_LM && A.cmax > 1;   // (no record arena when cmax == 1)
    const unsigned stateWord = ((const unsigned*)(st2 + parity))[tid < NSTATE ? tid : 0];
    float recWord = 0.f;
    if (haveRecs) recWord = ((const float*)A.recs_in)[tid < (int)(sizeof(TrialRecord) / 4) * A.cmax && tid < NREC ? tid : 0];
    if (!BATCH && MODE == TS_FUSED && !leader && st2[parity].done) return;   // launches queued behind the finishing one
    if (tid < NSTATE) ((unsigned*)&S)[tid] = stateWord;
    if (haveRecs && tid < NREC) ((float*)s_rec)[tid] = recWord;
  }
  __syncthreads();
  PHASE_MARK(1);
#ifdef LSD_DEVTOOLS
  const int lvlIn_ = S.level, numLaunchesIn_ = S.numLaunches, pendingIn_ = S.pending, ncandIn_ = S.ncand;
#endif
  // A finished job's launches leave here.  The host may have read the summary and gone on already (polled jobs and batches do not drain
  // the stream), so two things must stay true: (a) every workgroup of a launch queued behind the finishing one returns at this point,
  // before it touches frame or keyframe memory — the state and the trial records of the tracker's own scratch are all it has read; (b) the finishing launch requests its next strip
  // (strip_request below) before it knows that it finishes: those loads may read kf_refBlk after the host has seen `done`, and their
  // result is always discarded (the S.done return behind the finishing phase).
  // (the state words the code up to the LM step branches on, in one batch of LDS reads)
  const int doneIn = S.done, lvlPending = S.level, pending = S.pending, ncandIn = S.ncand;
  if (doneIn) {
    LAUNCH_LOG(1, pendingIn_, ncandIn_, -1);
    if (MODE != TS_EVAL && leader) { copy_words<sizeof(TrackState) / 4>(next, &S, tid, BLOCK); }   // keep both buffers "done"
    return;
  }
  // what the finishing launch raises `done` to: the job's tag where the host polls pinned memory for it (single jobs), 1 where it synchronises
  // (batches whose host polls: spec.seq is the batch's tag itself)
  const int doneWord = (MODE == TS_FUSED && spec.seq != 0) ? (BATCH ? spec.seq : (spec.seq >> 12)) : 1;
  step_role<BATCH, MODE>(role, job, spec, lf, lvlPending, pending);
  if (role.leaves) return;
  int cand = role.cand, bx = role.bx;
  PHASE_MARK(20);   // "role": from the state barrier (1) to here

  // the strip's list, requested ahead of time where this workgroup is going to evaluate at the pending level (strip_request)
  int cntv = 0;
  unsigned ow[STRIP_CHMAX];
  bool havePre = false;
  if (BATCH && MODE == TS_FUSED && pending && job.lv[lvlPending].tilePx > 0) {
    havePre = cand < trials_at(spec, lvlPending);
    if (havePre) strip_request(job.lv[lvlPending], xcd_tile(bx, job.lv[lvlPending].nblocks), wave, lane, cntv, ow);
  }

  int levelNow = lvlPending, ncandNow = ncandIn;   // the level and the trials to evaluate: the state's, as the LM step leaves it
  if (MODE != TS_EVAL && pending) {
    // Finish the trials of the previous launch, in the order the LM loop would have run them.  All their partial sums, order
    // keys and tail contributions are fetched TOGETHER (one memory round trip, whatever the number of trials), then wave 0 walks
    // through them without further barriers: totals -> LM decision -> (rejected, retry waiting) next trial, whose increment
    // and pose come from the record the workgroups that evaluated it left behind.
    const int ncandPending = ncandIn < 1 ? 1 : (ncandIn > TRIALS_MAX ? TRIALS_MAX : ncandIn);
    const int level = lvlPending;
    const int nb = BATCH ? job.lv[level].nblocks : lf.tiles_at(level);
    if (tid == SUMW * 64 - 1) stage_lm_par(job, level, s_par, BATCH ? trials_at(spec, level) : lf.trials_at(level));
    if (wave < SUMW) {
      column_sums<TRIALS_MAX>(A, nb, ncandPending, tid, ft.sum);
      TRACE_PUT(tr_, 0, 17, clock64());
    }
    gather_tails<BATCH, WAVES>(job, S, level, nb, ncandPending, A, s_rec, ft.sub, ft.nsub, wave, lane);
    TRACE_PUT(s_trp, SUMW * 64, 18, clock64());
    __syncthreads();
    PHASE_MARK(2);
    slot_totals<TRIALS_MAX, BLOCK>(ft.sum, ft.tot, ncandPending, tid);
    __syncthreads();
    if (wave == 0) {
      const int pc = pick_trial(S, s_par, level, ncandPending, ft.tot, ft.sub, ft.nsub, s_rec, tid);
      // column totals and tail-drop correction, one column per lane; then the LM decision in the same wave
      const float s = finish_totals(ft.tot, ft.sub, ft.nsub, pc, tid);
      if (tid < RS_NUM) sh.tot[tid] = s;
#ifdef LSD_ORDER_CHECK
      if (!BATCH && spec.dbgCounters) order_check_totals(spec, s, pc, tid);
#endif
      PHASE_MARK(3);
      TRACE_PUT(tr_, 0, 19, ncandPending); TRACE_PUT(tr_, 0, 7, pc);
      lm_wave<SPEC_LM>(s_par, S, s, sh, tid, leader ? out : nullptr, TRACE_LM_REC, pc, cand, doneWord);
    }
    __syncthreads();
    PHASE_MARK(4);
    // (what the LM step left of the state, as far as the code up to the evaluation branches on it: one batch of LDS reads)
    const int doneNow = S.done, lastCandNow = S.lastCand, phaseNow = S.phase;
    levelNow = S.level; ncandNow = S.ncand;
    if (doneNow) {
      if (!BATCH && MODE == TS_FUSED && lastCandNow > 0 && spec.copyMask != 0 && job.lv[level].writeMask && cand == 0 && bx < nb)
        copy_side_mask<BLOCK>(job, S, spec, level, bx, nb, tid);
      if (leader) copy_words<sizeof(TrackState) / 4>(next, &S, tid, BLOCK);
      LAUNCH_LOG(2, pendingIn_, ncandIn_, S.lastCand);
      return;
    }
    // a workgroup that evaluates trial c > 0 leaves that trial's increment and pose for the launch that finishes it
    if (cand > 0 && bx == 0 && phaseNow == 1 && cand < ncandNow && tid < TRIAL_RECORD_WORDS) ((float*)&A.recs_out[cand])[tid] = trial_record_word(S, tid);
  }

  if (MODE == TS_LM) {
    __syncthreads();              // (every wave has tested S.pending before it changes: see the note in reduce_and_store)
    if (tid == 0) { S.pending = 1; S.numLaunches = S.numLaunches + 1; }   // (numLaunches of a batch job: its rounds)
    __syncthreads();
    if (leader) copy_words<sizeof(TrackState) / 4>(next, &S, tid, BLOCK);
    return;
  }

  // ---- residual evaluation at S.level / S.R, S.t ------------------------------------------------------------------
  const int level = levelNow;
  const TrackLevel& L = job.lv[level];
  const int nb = BATCH ? L.nblocks : lf.tiles_at(level);
  if (MODE == TS_FUSED && level != lvlPending) { cand = 0; bx = (int)blockIdx.x; }   // first evaluation of the next level
  // everything of lv[level] the evaluation reads is requested here in one batch, unconditionally and in front of the return (the fields
  // depend on nothing but the level; one after the other, behind the branches that use them, each was a wait of its own)
  EvalCtx a;
  make_ctx_dev(job, S, level, a);   // (fetched beside the finishing phase for the pending level: measured, +-0 — the scalar loads are not what the step behind the LM waits for)
  const int writeMask = L.writeMask, evalBatch = L.evalBatch, tilePx = L.tilePx;
  if (bx >= nb || cand >= ncandNow) return;   // workgroup 0 always has work: it publishes the state at the end
  const int tile = xcd_tile(bx, nb);
  // a retry further down the reject chain: its pose is in the record the LM workgroup that proposed it left
  if (BATCH && MODE == TS_EVAL && cand > 0) ctx_set_pose(a, A.recs_in[cand]);
  gbyte* wasGood = (gbyte*)(writeMask ? (cand == 0 ? job.wasGood : spec.wasGoodSide + (size_t)(cand - 1) * spec.maskStride) : nullptr);
  const int work = a.npts >= 0 ? a.npts : a.w * a.h;
  float acc[RS_END];
#pragma unroll
  for (int k = 0; k < RS_END; k++) acc[k] = 0.f;
  int key0 = -1, key1 = -1, key2 = -1;   // reference-order keys of this lane's in-image points (descending)
  PHASE_MARK(21);   // "post-LM glue": from the LM barrier (4) to the evaluation loop
  TRACE_PUT(tr_, 0, 22, cand);
  if (BATCH && tilePx > 0) {
    if (!(havePre && level == lvlPending)) strip_request(L, tile, wave, lane, cntv, ow);   // (else: requested next to the state, at the head of the finishing phase)
    eval_strip<BLOCK>(a, tilePx, tile, work, cntv, ow, (unsigned*)s_red /* not live before the reduction */, wasGood, acc, key0, key1, key2, tid TRACE_ARGS);
  } else if (!BATCH && evalBatch != 0) {
    eval_groups_of_four(a, tile * BLOCK + tid, nb * BLOCK, work, wasGood, acc, key0, key1, key2);
  } else {
    eval_plain(a, tile * BLOCK + tid, nb * BLOCK, work, wasGood, acc, key0, key1, key2);
  }
  PHASE_MARK(5);
  TRACE_PUT(tr_, 0, 10, level); TRACE_PUT(tr_, 0, 11, nb); TRACE_PUT(tr_, 0, 26, lvlPending);
  reduce_and_store<BLOCK, BATCH, MODE>(a, L, S, tile, acc, key0, key1, key2, s_red, s_sum, s_wtop, s_top, A.sums_out + (size_t)cand * RS_COLS * A.max_rows,
                                       A.topkey_out + (size_t)cand * A.max_rows, A.topval_out + (size_t)cand * A.max_rows * (TAIL_ROWS * TAIL_STRIDE), tid);
  if (MODE == TS_FUSED && leader) copy_words<sizeof(TrackState) / 4>(next, &S, tid, BLOCK);   // S.pending was set behind the reduction's first barrier
  // the budget's last launch ends with the job unfinished: tell the host (pinned memory), which polls this next to `done` and
  // appends launches — the stream order makes them follow; no hipStreamQuery in the wait loop (each one puts a marker packet into
  // the queue the chain runs through: ~3 us per frame)
  if (MODE == TS_FUSED && leader && tid == 0 && spec.last != 0) out->exhausted = spec.seq;
  LAUNCH_LOG(3, pendingIn_, ncandIn_, S.lastCand);
  PHASE_MARK(6);
  TRACE_PUT(tr_, 0, 9, wall_clock64());
}

template <int BLOCK, bool BATCH, int MODE = TS_FUSED>
__global__ __launch_bounds__(BLOCK) void k_track_step(TrackJob jobv, const TrackJob* __restrict__ jobs, TrackState* __restrict__ st2,
                                                       TrackScratch sc, TrackSummary* __restrict__ out, int parity, int first, TrackSpec spec) {
#ifdef LSD_ORDER_CHECK
  // developer build: is every workgroup of every earlier launch of this stream finished when a workgroup of this launch starts?
  if (!BATCH && spec.dbgCounters && threadIdx.x == 0) {
    const unsigned long long fin = __hip_atomic_load(&spec.dbgCounters[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (fin < spec.dbgCum) {
      __hip_atomic_fetch_add(&spec.dbgCounters[1], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_max(&spec.dbgCounters[2], spec.dbgCum - fin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
#endif
  track_step_impl<BLOCK, BATCH, MODE>(jobv, jobs, st2, sc, out, parity, first, spec);
#ifdef LSD_ORDER_CHECK
  __syncthreads();
  if (!BATCH && spec.dbgCounters && threadIdx.x == 0) __hip_atomic_fetch_add(&spec.dbgCounters[0], 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
#endif
}

// ---- The coarse levels of a throughput-mode job inside ONE workgroup (round 6) --------------------------------------------------------
// A lock-step round of a batch costs its latency chain (state, partial sums of other workgroups, the LM step, list, pipeline fill,
// reduction: 11-13 us of workgroup time with 1.5-2.5 us of evaluation in it at levels 3 and 4, profiles/r06_notes.md section 9), every
// job pays the rounds of the slowest, and every (trial, strip) workgroup repeats the finishing phase.  A level small enough to be one
// strip and one LDS tile (at most LSD_SOLO_MAX_PX pixels: levels 3 and 4 of a 640x480 job) needs none of that: one workgroup per job runs
// the level's whole LM loop at its own pace and leaves the state at the first larger level for the lock-step rounds
// (k_track_step<.., true, TS_FUSED> with first = 0).  Everything an iteration reads is staged when the workgroup enters the level:
//   * the TRACKED FRAME'S TEXEL PLANE in LDS (gx, gy, I, 0: 16 bytes per pixel, 76.8 KB at 80x60) — the form BASELINE.json's north_star
//     names: LDS-staged image tiles for the bilinear taps (getInterpolatedElement43, C/util/globalFuncs.h:63-77); the tile is the level;
//   * the level's REFERENCE POINTS in registers: lane t owns points t, t + 512, ... of the level's list (the keyframe's reference blocks
//     in pixel order, as a strip of the lock-step rounds builds its own), at most LSD_SOLO_TRIPS of them, 2 registers each: pixel,
//     1 / idepth (= the point's z; x and y follow with the two multiply-adds of makePointCloud, TrackingReference.cpp:128-138); colour and
//     variance, read once per point and iteration, sit in LDS beside the tile — none of it depends on the pose.
// An LM iteration then touches no global memory: warp from registers, four 16-byte taps from LDS, finish, accumulate; the pose in scalar
// registers.  Four barriers per iteration: the upper half parks its sums and
// every wave its top-3 keys | the halves fold, wave 0 merges the top-3 and requests the three tail candidates' reference pixels (the only
// loads of the iteration, three lanes, under two barriers) | runs of columns | wave 0: totals, the candidates from the tile, tail drop,
// lm_wave on its own lanes (no barrier between them) | next iteration.  Same arithmetic per point, same LM step, the sums in this
// kernel's own fixed order; no speculation (a retry is one more iteration of a few microseconds, not a launch).
// Measured (profiles/r06_notes.md section 21): the tile neither gains nor costs against gathering the taps from L2 / HBM — the iteration
// is bound by what one CU can issue — and the launch takes about what the ten rounds it replaces took, on n CUs instead of the chip.
// (LSD_SOLO_MAX_PX and the batch size it pays from, LSD_SOLO_MIN_JOBS: track_plan.hpp)
#define LSD_SOLO_TRIPS 9          // x 512 lanes = 4608 points >= the (w - 2)(h - 2) interior of any level of at most 4800 pixels
#define LSD_SOLO_MAX_PTS (LSD_SOLO_TRIPS * 512)
#define LSD_SOLO_LDS_PTS 4544     // (w - 2)(h - 2) <= w h - 4 sqrt(w h) + 4 <= 4527 interior pixels of a level of at most 4800
static_assert(LSD_SOLO_LDS_PTS <= LSD_SOLO_MAX_PTS, "every point of the LDS lists has a register slot");
// the largest interior (w - 2)(h - 2) of a level of at most LSD_SOLO_MAX_PX pixels (w, h >= 3)
constexpr int lsd_solo_max_interior() {
  int best = 0;
  for (int w = 3; w <= LSD_SOLO_MAX_PX / 3; w++) {
    const int h = LSD_SOLO_MAX_PX / w;
    if ((w - 2) * (h - 2) > best) best = (w - 2) * (h - 2);
  }
  return best;
}
static_assert(lsd_solo_max_interior() <= LSD_SOLO_LDS_PTS, "the dense interior of any level k_track_solo takes fits its LDS lists");
// the four taps of getInterpolatedElement43 (C/util/globalFuncs.h:63-77) out of the tile; `fetch` = false reads texel 0 instead
__device__ __forceinline__ void solo_taps(const v4f* s_tex, const int w, const PointWarp& q, const bool fetch, PointTexels& t) {
  const int ix = fetch ? (int)q.u_new : 0;
  const int iy = fetch ? (int)q.v_new : 0;
  const v4f* bp = s_tex + (ix + __mul24(iy, w));
  const v4f v00 = bp[0], v10 = bp[1], v01 = bp[w], v11 = bp[w + 1];
  t.t00 = Texel3{v00.x, v00.y, v00.z}; t.t10 = Texel3{v10.x, v10.y, v10.z};
  t.t01 = Texel3{v01.x, v01.y, v01.z}; t.t11 = Texel3{v11.x, v11.y, v11.z};
}
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_track_solo(const TrackJob* __restrict__ jobs, TrackState* __restrict__ st2, TrackSummary* __restrict__ outs,
                                                          const int parity, const int doneWord) {
  const TrackJob& job = jobs[blockIdx.x];
  st2 += 2 * (size_t)blockIdx.x;
  TrackSummary* out = outs + blockIdx.x;
  constexpr int WAVES = BLOCK / 64;
  constexpr int HALF = BLOCK / 2;
  constexpr int CPP = RS_END;
  constexpr int RSLICE = BLOCK / CPP;
  constexpr int RRUN = (HALF + RSLICE - 1) / RSLICE;
  constexpr int TRIPS = LSD_SOLO_TRIPS;
  static_assert(WAVES * 3 <= 64, "top-3 merge in one wave");
  static_assert((size_t)TRIPS * BLOCK * 4 <= sizeof(float) * (CPP * (HALF + 1) + RRUN), "the level's list borrows the reduction buffer");
  __shared__ TrackState S;
  __shared__ LmShared sh;
  __shared__ LmPar s_par;
  __shared__ __attribute__((aligned(16))) float s_red[CPP * (HALF + 1) + RRUN];
  __shared__ float s_sum[RSLICE][64];
  __shared__ float s_sub[TAIL_ROWS][TAIL_STRIDE];
  __shared__ int s_wtop[WAVES][3];
  __shared__ v4f s_tex[LSD_SOLO_MAX_PX];
  __shared__ float s_var[LSD_SOLO_LDS_PTS], s_img[LSD_SOLO_LDS_PTS];     // the points' variances and colours, list order (the registers hold the rest of a point)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  track_state_begin(S, job, tid);
  __syncthreads();
  int listLevel = -1, total = 0;
  EvalCtx a;
  // this lane's reference points of the level (trip r: point tid + r BLOCK of the list)
  unsigned pXY[TRIPS];
  float pZ[TRIPS];
  for (int guard = 0; guard < 4096; guard++) {
    const int level = S.level;
    // the same two invariants as at track_step_impl's early-out: once the job is done this workgroup touches no frame or keyframe memory
    // again, and nothing is requested ahead of this check (every load of a level sits behind it), so there is nothing to discard
    if (S.done) break;
    const TrackLevel& L = job.lv[level];
    const int work = L.w * L.h;
    if (L.tilePx <= 0 || work > LSD_SOLO_MAX_PX || L.writeMask) break;     // the larger levels (and the one that writes refPixelWasGood): lock-step rounds of strips
    if (level != listLevel) {
      make_ctx_dev(job, S, level, a);
      if (tid == BLOCK - 1) stage_lm_par(job, level, s_par, 1);
      const int mblk = (work + 255) >> 8;                   // <= 19
      const gbyte* offs = (const gbyte*)L.kf_refBlk;
      const __attribute__((address_space(1))) int* cnts = (const __attribute__((address_space(1))) int*)(offs + ((size_t)mblk << 8));
      const int cntv = lane < mblk ? cnts[lane] : 0;
      const int incl = wave_scan32(cntv);
      total = __builtin_amdgcn_readlane(incl, 31);
      if (total > LSD_SOLO_LDS_PTS) break;                  // (every wave computes the same total) cannot happen below 4800 pixels; strips if it does
      // the tile: the level's texel plane, 16 bytes per lane and step
      {
        gv4f* src = (gv4f*)a.fr_grad;
        for (int i = tid; i < work; i += BLOCK) s_tex[i] = src[i];
      }
      // the level's list (pixel order, as a strip of the lock-step rounds builds its own) in the reduction buffer
      unsigned* s_list = (unsigned*)s_red;
      const int waveU = __builtin_amdgcn_readfirstlane(wave);
      const float inv_w = 1.0f / (float)a.w;
      for (int blk = waveU; blk < mblk; blk += WAVES) {
        const int cb = __builtin_amdgcn_readlane(cntv, blk);
        const int pb = __builtin_amdgcn_readlane(incl, blk) - cb;
        const unsigned ow = *(const __attribute__((address_space(1))) unsigned*)(offs + ((size_t)blk << 8) + (lane << 2));
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int sl = lane + 64 * k;
          if (sl < cb) s_list[pb + sl] = pixel_xy16((blk << 8) + (int)((ow >> (8 * k)) & 255u), a.w, inv_w);
        }
      }
      __syncthreads();
      // this lane's points: everything of the keyframe an evaluation reads, once per level
      {
        float var[TRIPS], id[TRIPS], img[TRIPS];
#pragma unroll
        for (int r = 0; r < TRIPS; r++) {
          const int p = tid + r * BLOCK;
          const unsigned xy = s_list[p < total ? p : 0];
          const int i = __mul24((int)(xy >> 16), a.w) + (int)(xy & 0xffffu);
          pXY[r] = xy;
          var[r] = a.kf_idepthVar[i];
          id[r] = a.kf_idepth[i];
          img[r] = a.kf_image[i];
        }
#pragma unroll
        for (int r = 0; r < TRIPS; r++) {
          const int p = tid + r * BLOCK;
          if (p < total) { s_var[p] = var[r]; s_img[p] = img[r]; }
          pZ[r] = (p < total) ? lsd_rcp_exact(id[r]) * 1.0f : 1.0f;      // ref_point_at's z; x and y per iteration (ref_point_xy)
        }
      }
      listLevel = level;
      __syncthreads();                                      // the list's words become the reduction buffer again
    } else {
      // the pose under evaluation (the LM step of the previous iteration left it in S)
      ctx_set_pose(a, S);
      a.aff_a = S.aff_a; a.aff_b = S.aff_b;
    }
    // (the pose is the same in every lane: scalar registers — the lane's points and the 41 running sums want the vector ones)
    auto uni = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
#pragma unroll
    for (int i = 0; i < 9; i++) a.R[i] = uni(a.R[i]);
#pragma unroll
    for (int i = 0; i < 3; i++) a.t[i] = uni(a.t[i]);
    a.aff_a = uni(a.aff_a); a.aff_b = uni(a.aff_b);
    float acc[RS_END];
#pragma unroll
    for (int k = 0; k < RS_END; k++) acc[k] = 0.f;
    int key0 = -1, key1 = -1, key2 = -1;
    {
      const int rounds = (total + BLOCK - 1) / BLOCK;
#pragma unroll
      for (int r = 0; r < TRIPS; r++) {
        // (uniform branch: every lane sees the same `rounds`.  Requesting the taps of trip r + 1 before trip r is finished — two points in
        // flight — pushed the kernel over its 256 registers; the LDS round trip hides behind the SIMD's other wave)
        if (r < rounds) {
          const bool live = tid + r * BLOCK < total;
          const int x_ = (int)(pXY[r] & 0xffffu), y_ = (int)(pXY[r] >> 16);
          float px, py;
          ref_point_xy(a, x_, y_, pZ[r], px, py);
          PointWarp q; PointTexels t;
          eval_warp(a, px, py, pZ[r], q);
          solo_taps(s_tex, a.w, q, live && q.in_image, t);
          // (no mask at these levels; the key: reference order, x h + y, TrackingReference.cpp:128-138)
          if (live) visit_point(a, q, t, pZ[r], s_img[tid + r * BLOCK], s_var[tid + r * BLOCK], nullptr, 0, __mul24(x_, a.h) + y_, acc, key0, key1, key2);
        }
      }
    }
    // each wave's three largest keys; the upper half parks its sums
    wave_top3(key0, key1, key2, s_wtop);
    if (tid >= HALF) {
#pragma unroll
      for (int k = 0; k < CPP; k++) s_red[k * (HALF + 1) + tid - HALF] = acc[k];
    }
    __syncthreads();
    // wave 0: the level's three largest keys = the candidates for the tail (the last M % 4 in-image points in reference order); lanes
    // 0..2 evaluate them once more — their reference pixel travels under the next two barriers, the taps come out of the tile
    TailCandidate c;
    if (wave == 0) {
      int top[3];
      merge_top3(s_wtop, WAVES, top);
      c.request(a, lane == 0 ? top[0] : (lane == 1 ? top[1] : (lane == 2 ? top[2] : -1)));
    }
    if (tid < HALF) {
#pragma unroll
      for (int k = 0; k < CPP; k++) s_red[k * (HALF + 1) + tid] = acc[k] + s_red[k * (HALF + 1) + tid];
    }
    __syncthreads();
    {
      const int slice = tid / CPP, k = tid - slice * CPP;
      if (slice < RSLICE) s_sum[slice][k] = slice_sum<HALF + 1, RRUN>(s_red, k, slice);
    }
    __syncthreads();
    if (wave == 0) {
      float sv = 0.f;
      if (lane < CPP) {
        sv = s_sum[0][lane];
#pragma unroll
        for (int sl = 1; sl < RSLICE; sl++) sv += s_sum[sl][lane];
      }
      if (c.key >= 0) {
        float px, py, cPz;
        ref_point_at(a, c.x, c.y, c.id, px, py, cPz);
        PointWarp cq; PointTexels ct;
        eval_warp(a, px, py, cPz, cq);
        solo_taps(s_tex, a.w, cq, cq.in_image, ct);
        PointOut o;
        eval_finish(a, cq, ct, cPz, c.img, c.var, o);
        tail_row(o, s_sub[lane]);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const int M = (int)rl(sv, RS_M);
      const int nsub = (__builtin_amdgcn_readlane(c.key, 0) >= 0) + (__builtin_amdgcn_readlane(c.key, 1) >= 0) + (__builtin_amdgcn_readlane(c.key, 2) >= 0);
      sv = tail_drop(sv, M, nsub, tail_word(lane), s_sub);
      if (lane < RS_NUM) sh.tot[lane] = sv;
      lm_wave<false>(s_par, S, sv, sh, lane, out, nullptr, 0, 0, doneWord);
    }
    __syncthreads();
  }
  // what the lock-step rounds load (they read st2[parity of their launch]; a finished job keeps both buffers "done")
  copy_words<sizeof(TrackState) / 4>(st2 + (1 - parity), &S, tid, BLOCK);
  if (S.done) copy_words<sizeof(TrackState) / 4>(st2 + parity, &S, tid, BLOCK);
}

// Pipelined contexts: the frame's refPixelWasGood is what the LAST trial the LM loop executed wrote.  Trial 0 of every launch writes the
// frame's own plane, trials > 0 write side planes — at the same pixels (the valid reference points do not depend on the pose), so the
// pixels the job visited are those whose byte in the frame's plane is no longer the 0xFF of frame creation: there the side plane's byte
// replaces it.  Queued on the mapping stream by lsdhip_tracker_track (one-stream contexts: the finishing launch copies instead).
__global__ __launch_bounds__(256) void k_mask_merge(uint32_t* __restrict__ plane, const uint32_t* __restrict__ side, int nwords) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nwords) return;
  const uint32_t a = plane[i], b = side[i];
  // per byte: visited (a != 0xFF) -> b, else a
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) if (((a >> (8 * k)) & 0xFFu) != 0xFFu) m |= 0xFFu << (8 * k);
  plane[i] = (a & ~m) | (b & m);
}

int lsd_flush_merges(lsdhip_ctx* c) {
  const int nwords = (int)((((size_t)c->wl[LSD_TRACK_MIN_LEVEL] * c->hl[LSD_TRACK_MIN_LEVEL]) + 3) / 4);
  for (const lsdhip_ctx::PendingMerge& m : c->pendingMerges) {
    hipLaunchKernelGGL(k_mask_merge, dim3((nwords + 255) / 256), dim3(256), 0, c->mstream, (uint32_t*)m.plane, (const uint32_t*)m.side, nwords);
    *m.doneSeq = c->mSeq + 1;      // complete at the mapping stream's next record point
  }
  c->pendingMerges.clear();
  HIPCHK(hipGetLastError());
  return LSDHIP_OK;
}

// checkPermaRefOverlap (SE3Tracker.cpp:121-157): usage only, explicit point list.  One 256-lane workgroup sums one cloud: lane-strided
// accumulation, wave sums, the four wave totals in order; lane 0 returns the sum.  k_overlap and k_overlap_bank share it, so a candidate
// is summed in the same order whichever launch it rides in.
__device__ __forceinline__ float overlap_block_sum(const float* __restrict__ pos, int n, const float* R, const float* t, float fx, float fy, float cx,
                                                   float cy, int w, int h, float* s_w) {
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    float px = pos[3 * i], py = pos[3 * i + 1], pz = pos[3 * i + 2];
    float Wx = ((R[0] * px + R[1] * py) + R[2] * pz) + t[0];
    float Wy = ((R[3] * px + R[4] * py) + R[5] * pz) + t[1];
    float Wz = ((R[6] * px + R[7] * py) + R[8] * pz) + t[2];
    float u_new = (Wx / Wz) * fx + cx;
    float v_new = (Wy / Wz) * fy + cy;
    if (u_new > 0 && v_new > 0 && u_new < w - 1 && v_new < h - 1) {
      float depthChange = pz / Wz;
      acc += depthChange < 1 ? depthChange : 1;
    }
  }
  float s = wave_sum_to_lane63(acc);
  if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = s;
  __syncthreads();
  return ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}
__global__ __launch_bounds__(256) void k_overlap(const float* __restrict__ pos, int n, EvalCtx a, float* __restrict__ out) {
  __shared__ float s_w[4];
  const float sum = overlap_block_sum(pos, n, a.R, a.t, a.fx, a.fy, a.cx, a.cy, a.w, a.h, s_w);
  if (threadIdx.x == 0) out[0] = sum;
}
// checkPermaRefOverlap for the (slot, pose) pairs of a keyframe bank (lsdhip_tracker_check_overlap_bank): workgroup = pair
struct OverlapJob { LSD_G const float* pos; int n; float R[9], t[3]; };
__global__ __launch_bounds__(256) void k_overlap_bank(const OverlapJob* __restrict__ jobs, float fx, float fy, float cx, float cy, int w, int h,
                                                      float* __restrict__ out) {
  __shared__ float s_w[4];
  const OverlapJob& J = jobs[blockIdx.x];
  float R[9], t[3];
#pragma unroll
  for (int i = 0; i < 9; i++) R[i] = J.R[i];
#pragma unroll
  for (int i = 0; i < 3; i++) t[i] = J.t[i];
  const float sum = overlap_block_sum((const float*)J.pos, J.n, R, t, fx, fy, cx, cy, w, h, s_w);
  if (threadIdx.x == 0) out[blockIdx.x] = sum;
}

// Test hook (lsdhip_devtest_se3f_lm_step): the proposal of lm_wave on given normal equations, one 64-lane workgroup per case.  A / b
// sit in LDS where lm_wave finds them (TrackState::A / b, LGS6 after finish()), and the step is the same three calls.
__global__ __launch_bounds__(64) void k_devtest_se3f_lm_step(const float* __restrict__ A, const float* __restrict__ b, const float* __restrict__ damp,
                                                              const float* __restrict__ T7, float* __restrict__ inc6, float* __restrict__ Tn7) {
  __shared__ TrackState S;
  __shared__ LmShared sh;
  const int lane = threadIdx.x, c = blockIdx.x;
  if (lane < 36) S.A[lane] = A[c * 36 + lane];
  if (lane < 6) S.b[lane] = b[c * 6 + lane];
  __syncthreads();
  const float* p = T7 + c * 7;
  lsdm::SE3fH T;
  T.q = {p[0], p[1], p[2], p[3]};
  T.t[0] = p[4]; T.t[1] = p[5]; T.t[2] = p[6];
  float inc[6];
  gj6_solve_wave(S.A, S.b, damp[c], sh.gj, lane, inc);
  const lsdm::SE3fH Tn = se3f_mul_wave(se3f_exp_wave(inc, lane), T, lane);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 6; i++) inc6[c * 6 + i] = inc[i];
    float* o = Tn7 + c * 7;
    o[0] = Tn.q.w; o[1] = Tn.q.x; o[2] = Tn.q.y; o[3] = Tn.q.z; o[4] = Tn.t[0]; o[5] = Tn.t[1]; o[6] = Tn.t[2];
  }
}

// ---------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------
// The TrackScratch arena, the one place that knows its layout: four arrays over [job][parity][trial slot], one behind the other — sums
// (RS_COLS floats per tile row) | topkey (an int4 per row) | topval (96 floats per row) | recs (32 floats per slot).  Offsets in floats.
struct ScratchLayout { size_t topkey, topval, recs, end; };
static constexpr ScratchLayout scratch_layout(size_t jobs, size_t trials, size_t rows) {
  const size_t slots = jobs * 2 * trials;
  const size_t topkey = slots * RS_COLS * rows, topval = topkey + slots * 4 * rows, recs = topval + slots * 96 * rows;
  return {topkey, topval, recs, recs + slots * 32};
}
// (the two arenas in use — a single job's LSD_SPEC_MAX slots, a batch's LSD_BATCH_SPEC_MAX per job — sized as they always were)
static_assert(scratch_layout(1, LSD_SPEC_MAX, 304).end * 4 == (size_t)LSD_SPEC_MAX * (2 * RS_COLS * 304 * 4 + 2 * 304 * 16 + 2 * 304 * 96 * 4 + 2 * 32 * 4) &&
              scratch_layout(8, LSD_BATCH_SPEC_MAX, 304).end * 4 == 8 * (size_t)LSD_BATCH_SPEC_MAX * (2 * RS_COLS * 304 * 4 + 2 * 304 * 16 + 2 * 304 * 96 * 4 + 2 * 32 * 4) &&
              scratch_layout(8, LSD_BATCH_SPEC_MAX, 304).recs == 8 * (size_t)LSD_BATCH_SPEC_MAX * (2 * RS_COLS * 304 + 2 * 4 * 304 + 2 * 96 * 304),
              "scratch arena: byte count and offsets");
// the arena at `base` as the kernels take it; cmax = the trial slots per parity they index with (<= trials; 1: no speculation, no recs)
static TrackScratch scratch_at(const lsdhip_tracker* t, float* base, size_t jobs, size_t trials, int cmax) {
  const ScratchLayout lay = scratch_layout(jobs, trials, (size_t)t->max_blocks);
  TrackScratch sc;
  sc.sums = base;
  sc.topkey = (int4*)(base + lay.topkey);
  sc.topval = base + lay.topval;
  sc.recs = cmax > 1 ? (TrialRecord*)(base + lay.recs) : nullptr;
  sc.max_rows = t->max_blocks;
  sc.cmax = cmax;
#ifdef LSD_PHASE_TRACE
  sc.trace = t->d_trace;
#endif
  return sc;
}

extern "C" int lsdhip_tracker_create(lsdhip_ctx* c, lsdhip_tracker** out) {
  if (!c || !out) return LSDHIP_E_ARG;
  HIPCHK(hipSetDevice(c->device));
  std::unique_ptr<lsdhip_tracker> owner(new lsdhip_tracker());
  lsdhip_tracker* t = owner.get();
  t->ctx = c;
  const int maxIterations[6] = {5, 20, 50, 100, 100, 100};
  for (int l = 0; l < LSD_LEVELS; l++) {
    t->lambdaInitial[l] = 0;
    t->stepSizeMin[l] = 1e-8;
    t->convergenceEps[l] = 0.999f;
    t->maxItsPerLvl[l] = maxIterations[l];
  }
  if (const char* e = getenv("LSDHIP_TRACK_BLOCK")) t->block = atoi(e);
  if (const char* e = getenv("LSDHIP_TRACK_CAP")) t->grid_cap = atoi(e);
  if (const char* e = getenv("LSDHIP_EVAL_BATCH")) t->evalBatch = atoi(e) != 0;
  if (t->block != 256) { lsd_set_error("LSDHIP_TRACK_BLOCK must be 256"); return LSDHIP_E_ARG; }
  t->grid_cap = lsd_grid_cap(t->grid_cap, t->block, RS_END);
  t->max_blocks = t->grid_cap;
  const size_t partials_bytes = scratch_layout(1, LSD_SPEC_MAX, (size_t)t->max_blocks).end * sizeof(float);
  if (const char* e = getenv("LSDHIP_SPEC")) t->specC = atoi(e);
  if (t->specC < 1) t->specC = 1;
  if (t->specC > LSD_SPEC_MAX) t->specC = LSD_SPEC_MAX;
  if (const char* e = getenv("LSDHIP_SPEC_CAP")) t->specCap = atoi(e) & ~7;
  if (const char* e = getenv("LSDHIP_SPEC_CAPS")) {
    int v[LSD_LEVELS] = {0, 0, 0, 0, 0};
    sscanf(e, "%d,%d,%d,%d,%d", &v[0], &v[1], &v[2], &v[3], &v[4]);
    for (int l = 0; l < LSD_LEVELS; l++) t->specCaps[l] = v[l] < 0 ? 0 : (v[l] & ~7);
  }
  if (const char* e = getenv("LSDHIP_SPEC_LEVELS")) {
    int v[LSD_LEVELS] = {0, 0, 0, 0, 0};
    sscanf(e, "%d,%d,%d,%d,%d", &v[0], &v[1], &v[2], &v[3], &v[4]);
    for (int l = 0; l < LSD_LEVELS; l++) t->specLevel[l] = v[l] < 0 ? 0 : (v[l] > LSD_SPEC_MAX ? LSD_SPEC_MAX : v[l]);
  }
  t->maskStride = (((size_t)c->wl[LSD_TRACK_MIN_LEVEL] * c->hl[LSD_TRACK_MIN_LEVEL]) + 255) & ~(size_t)255;
  if (int rc = lsd_dev_alloc(t->d_maskSide, 2 * t->maskStride * (LSD_SPEC_MAX - 1))) return rc;
  HIPCHK(hipMemsetAsync(t->d_maskSide, 0, 2 * t->maskStride * (LSD_SPEC_MAX - 1), c->stream));
  if (int rc = lsd_dev_alloc(t->d_partials, partials_bytes / sizeof(float))) return rc;
  HIPCHK(hipMemsetAsync(t->d_partials, 0, partials_bytes, c->stream));
#ifdef LSD_ORDER_CHECK
  {
    const size_t nd = 8 + 2 * 8192;
    if (int rc = lsd_dev_alloc(t->d_dbg, nd)) return rc;
    std::vector<unsigned long long> init(nd, 0);
    for (size_t i = 8; i < nd; i += 2) init[i] = ~0ull;     // (min, max) pairs of the per-launch totals hash
    HIPCHK(hipMemcpy(t->d_dbg, init.data(), nd * 8, hipMemcpyHostToDevice));
  }
#endif
#ifdef LSD_DEVTOOLS
  if (int rc = lsd_dev_alloc(t->d_log, 4096 * 16)) return rc;
  HIPCHK(hipMemset(t->d_log, 0, 4096 * 16 * 4));
#endif
  if (int rc = lsd_dev_alloc(t->d_state, 2)) return rc;
  HIPCHK(hipMemsetAsync(t->d_state, 0, 2 * sizeof(TrackState), c->stream));
#ifdef LSD_PHASE_TRACE
  if (int rc = lsd_dev_alloc(t->d_trace, 1 + 4096 * LSD_TRACE_WORDS)) return rc;
  HIPCHK(hipMemsetAsync(t->d_trace, 0, (1 + 4096 * LSD_TRACE_WORDS) * 8, c->stream));
#endif
  if (int rc = lsd_pinned_alloc(t->h_summary, 1, hipHostMallocMapped, &t->d_summary)) return rc;
  memset(t->h_summary, 0, sizeof(TrackSummary));
  const char* env = getenv("LSDHIP_HOST_LM");
  t->hostLM = env && env[0] == '1';
  if (const char* e = getenv("LSDHIP_SPIN")) t->spinWait = e[0] != '0';
  if (const char* e = getenv("LSDHIP_BUDGET_EXTRA")) { t->budgetExtra = atoi(e); if (t->budgetExtra < 1) t->budgetExtra = 1; }
  if (const char* e = getenv("LSDHIP_BUDGET_FIXED")) { t->budgetFixed = atoi(e); if (t->budgetFixed < 1) t->budgetFixed = 0; }   // test hook: every job runs out of budget
  *out = owner.release();
  return LSDHIP_OK;
}
extern "C" void lsdhip_tracker_destroy(lsdhip_tracker* t) {
  if (!t) return;
  {
    lsdhip_ctx* c = t->ctx;
    LSD_CTX_LOCK(c);
    for (size_t i = 0; i < c->pendingMerges.size();)     // merges out of this tracker's side planes die with it
      if (c->pendingMerges[i].doneSeq == &t->maskMergeSeq[0] || c->pendingMerges[i].doneSeq == &t->maskMergeSeq[1]) c->pendingMerges.erase(c->pendingMerges.begin() + i);
      else i++;
  }
#ifdef LSD_DEVTOOLS
  if (getenv("LSDHIP_TRACK_DEBUG") && t->dbgJobs > 0)
    fprintf(stderr, "TRACKDBG jobs %lld launches enqueued %.2f/job, budget misses %lld, host launch %.1f us/job, host wait %.1f us/job\n", t->dbgJobs,
            (double)t->dbgEnqueued / t->dbgJobs, t->dbgMisses, t->dbgLaunchNs / 1e3 / t->dbgJobs, t->dbgWaitNs / 1e3 / t->dbgJobs);
#endif
  (void)hipSetDevice(t->ctx->device);
  (void)hipStreamSynchronize(t->ctx->stream);
#ifdef LSD_ORDER_CHECK
  {
    std::vector<unsigned long long> h(8 + 2 * 8192, 0);
    (void)hipMemcpy(h.data(), t->d_dbg, h.size() * 8, hipMemcpyDeviceToHost);
    int used = 0, split = 0;
    for (size_t i = 8; i < h.size(); i += 2) if (h[i] != ~0ull) { used++; if (h[i] != h[i + 1]) split++; }
    if (const char* path = getenv("LSDHIP_ORDER_DUMP")) {
      if (FILE* f = fopen(path, "w")) {
        for (size_t i = 8; i < h.size(); i += 2) if (h[i] != ~0ull) fprintf(f, "%zu %llx %llx\n", (i - 8) / 2, h[i], h[i + 1]);
        fclose(f);
      }
    }
    fprintf(stderr, "ORDERCHECK: %llu workgroups finished (%llu launched), %llu started before every earlier workgroup had finished (largest deficit %llu); "
                    "%d launch slots hashed, %d in which the workgroups did NOT all see the same totals\n", h[0], t->dbgCum, h[1], h[2], used, split);
  }
#endif
#ifdef LSD_PHASE_TRACE
  if (const char* path = getenv("LSDHIP_TRACE_FILE")) {
    std::vector<unsigned long long> h(1 + 4096 * LSD_TRACE_WORDS);
    if (hipMemcpy(h.data(), t->d_trace, h.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
      if (FILE* f = fopen(path, "w")) {
        unsigned long long n = h[0] < 4096 ? h[0] : 4096;
        for (unsigned long long i = 0; i < n; i++) {
          for (int k = 0; k < LSD_TRACE_WORDS; k++) fprintf(f, "%llu ", h[1 + i * LSD_TRACE_WORDS + k]);
          fprintf(f, "\n");
        }
        fclose(f);
      }
    }
  }
#endif
  delete t;
}
extern "C" int lsdhip_tracker_set_enqueue_hook(lsdhip_tracker* t, lsdhip_enqueue_hook fn, void* user) {
  if (!t) return LSDHIP_E_ARG;
  t->enqueueHook = fn;
  t->enqueueHookUser = user;
  return LSDHIP_OK;
}
extern "C" int lsdhip_tracker_get_settings(const lsdhip_tracker* t, lsdhip_tracker_settings* o) {
  if (!t || !o) return LSDHIP_E_ARG;
  o->lambdaSuccessFac = t->lambdaSuccessFac; o->lambdaFailFac = t->lambdaFailFac;
  for (int l = 0; l < LSD_LEVELS; l++) {
    o->lambdaInitial[l] = t->lambdaInitial[l]; o->stepSizeMin[l] = t->stepSizeMin[l]; o->convergenceEps[l] = t->convergenceEps[l];
    o->maxItsPerLvl[l] = t->maxItsPerLvl[l];
  }
  o->lambdaInitialTestTrack = t->lambdaInitialTestTrack; o->stepSizeMinTestTrack = t->stepSizeMinTestTrack;
  o->convergenceEpsTestTrack = t->convergenceEpsTestTrack; o->maxItsTestTrack = t->maxItsTestTrack;
  o->huber_d = t->huber_d; o->var_weight = t->var_weight;
  return LSDHIP_OK;
}
extern "C" int lsdhip_tracker_set_settings(lsdhip_tracker* t, const lsdhip_tracker_settings* in) {
  if (!t || !in) return LSDHIP_E_ARG;
  t->lambdaSuccessFac = in->lambdaSuccessFac; t->lambdaFailFac = in->lambdaFailFac;
  for (int l = 0; l < LSD_LEVELS; l++) {
    t->lambdaInitial[l] = in->lambdaInitial[l]; t->stepSizeMin[l] = in->stepSizeMin[l]; t->convergenceEps[l] = in->convergenceEps[l];
    t->maxItsPerLvl[l] = in->maxItsPerLvl[l];
  }
  t->lambdaInitialTestTrack = in->lambdaInitialTestTrack; t->stepSizeMinTestTrack = in->stepSizeMinTestTrack;
  t->convergenceEpsTestTrack = in->convergenceEpsTestTrack; t->maxItsTestTrack = in->maxItsTestTrack;
  t->huber_d = in->huber_d; t->var_weight = in->var_weight;
  return LSDHIP_OK;
}
extern "C" int lsdhip_tracker_exec_stats(const lsdhip_tracker* t, int out[8]) {
  if (!t || !out) return LSDHIP_E_ARG;
  out[0] = 0; out[1] = 0; out[2] = 0;   // (were: cluster-kernel job counts — the kernel was removed in round 4, profiles/r03_notes.md §3)
  for (int l = 0; l < LSD_LEVELS; l++) out[3 + l] = t->levelEvaluations[l];
  return LSDHIP_OK;
}
extern "C" int lsdhip_tracker_set_speculation(lsdhip_tracker* t, int trials, int finestLevelWorkgroups) {
  if (!t || trials < 1 || trials > LSD_SPEC_MAX || finestLevelWorkgroups < 0) { lsd_set_error("lsdhip_tracker_set_speculation: trials must be 1..%d", LSD_SPEC_MAX); return LSDHIP_E_ARG; }
  LSD_CTX_LOCK(t->ctx);
  t->specC = trials;
  t->specAuto = false;                                        // the same number of trials at every level
  if (finestLevelWorkgroups > 0) t->specCap = finestLevelWorkgroups < 8 ? 8 : (finestLevelWorkgroups & ~7);   // multiples of 8 (one tile band per XCD), at least 8
  for (int l = 0; l < LSD_LEVELS; l++) t->specLevel[l] = 0;
  t->recent = LaunchHistory{};
  return LSDHIP_OK;
}
extern "C" int lsdhip_tracker_set_batch_coarse_min_jobs(lsdhip_tracker* t, int minJobs) {
  if (!t || minJobs < 0) { lsd_set_error("lsdhip_tracker_set_batch_coarse_min_jobs: minJobs must be >= 0"); return LSDHIP_E_ARG; }
  LSD_CTX_LOCK(t->ctx);
  t->soloMinJobs = minJobs;
  return LSDHIP_OK;
}
#ifdef LSD_DEVTOOLS
// developer build: the launch log of the last job (LSDHIP_LAUNCH_LOG=1): 16 ints per queued launch, slot = launch ordinal (1-based)
extern "C" int lsdhip_tracker_debug_log(const lsdhip_tracker* t, int* out, int maxInts) {
  if (!t || !out) return -1;
  const int n = (int)t->lastLog.size() < maxInts ? (int)t->lastLog.size() : maxInts;
  memcpy(out, t->lastLog.data(), (size_t)n * 4);
  return n;
}
#endif
extern "C" int lsdhip_tracker_launch_stats(const lsdhip_tracker* t, int out[2]) {
  if (!t || !out) return LSDHIP_E_ARG;
  out[0] = t->numLaunches; out[1] = t->specC;
  return LSDHIP_OK;
}
extern "C" int lsdhip_tracker_step_stats(const lsdhip_tracker* t, int out[4]) {
  if (!t || !out) return LSDHIP_E_ARG;
  out[0] = t->numLaunches; out[1] = 0; out[2] = 0; out[3] = t->specC;
  return LSDHIP_OK;
}
extern "C" int lsdhip_tracker_set_max_its(lsdhip_tracker* t, const int its[LSD_LEVELS]) {
  if (!t || !its) return LSDHIP_E_ARG;
  for (int l = 0; l < LSD_LEVELS; l++) t->maxItsPerLvl[l] = its[l];
  return LSDHIP_OK;
}

static const float MIN_GOODPERGOODBAD_PIXEL = 0.5f;
static const float MIN_GOODPERALL_PIXEL = 0.04f;
static const float MIN_GOODPERALL_PIXEL_ABSMIN = 0.01f;

// Developer switches of the batch path (sweeps and A/Bs; tools/gpu.sh ab sets them per process): read once, at the first batch.
static long long env_num(const char* name, long long dflt) { const char* e = getenv(name); return e ? atoll(e) : dflt; }
struct BatchEnv {
  int specMax = (int)std::clamp<long long>(env_num("LSDHIP_BATCH_SPEC", LSD_BATCH_SPEC_MAX), 1, LSD_BATCH_SPEC_MAX);   // most trials per step (1: off)
  long long specPixels = env_num("LSDHIP_BATCH_SPEC_PIXELS", LSD_BATCH_SPEC_PIXELS);
  int fused = (int)env_num("LSDHIP_BATCH_FUSED", 2);   // 0 = LM launch + evaluation launch per round (round 6), 1 = the fused form without speculation
  int margin = (int)env_num("LSDHIP_BATCH_MARGIN", 3);   // rounds queued beyond what the recent batches needed
  bool poll = !(getenv("LSDHIP_BATCH_POLL") && getenv("LSDHIP_BATCH_POLL")[0] == '0');   // 0: synchronise the stream instead of polling the summaries
  int soloMin = (int)env_num("LSDHIP_BATCH_SOLO_MIN", LSD_SOLO_MIN_JOBS);   // (0: never)
  int stripWgs = (int)env_num("LSDHIP_BATCH_WGS", LSD_BATCH_STRIP_WORKGROUPS);   // strips x jobs of a throughput-mode evaluation launch
  int traceWg = (int)env_num("LSDHIP_TRACE_WG", 0);      // LSD_PHASE_TRACE builds: the traced workgroup
};
static const BatchEnv& batch_env() { static const BatchEnv env; return env; }

// Does a single job's evaluation take the points of this level four at a time (k_track_step, TrackLevel::evalBatch)?  Dense keyframe
// levels on which a lane has more than one point; decided again wherever the level's tiling changes.
static int eval_batch_level(const lsdhip_tracker* t, const TrackLevel& L) { return t->evalBatch && L.npts < 0 && !L.singlePass && L.tilePx == 0 ? 1 : 0; }
// one level of a job: planes, intrinsics, LM settings and its tiling for the batch `shape`.  Fails only if the level-0 planes cannot be built.
static int fill_level(lsdhip_tracker* t, TrackJob& job, BatchShape shape, int level, lsdhip_frame* kf, lsdhip_frame* frame, const float* pts_pos,
                      const float* pts_colvar, int npts) {
  lsdhip_ctx* c = t->ctx;
  LSD_CTX_LOCK(c);
  TrackLevel& L = job.lv[level];
  const LevelIntr& in = c->intr[level];
  L.w = c->wl[level]; L.h = c->hl[level];
  L.fx = in.fx; L.fy = in.fy; L.cx = in.cx; L.cy = in.cy; L.fxi = in.fxi; L.fyi = in.fyi; L.cxi = in.cxi; L.cyi = in.cyi;
  L.fr_grad = frame->d_grad[level];
  if (level == 0) { if (int rc = lsd_frame_require_level0_for_tracking(frame)) return rc; }   // (levels >= 1 are what a tracked frame has: the level-0 texels on demand)
  if (npts >= 0) {
    L.pts_pos = pts_pos; L.pts_colvar = pts_colvar; L.npts = npts;
    L.kf_idepth = L.kf_idepthVar = L.kf_image = nullptr;
    L.kf_refBlk = nullptr;
  } else {
    L.kf_idepth = kf->d_idepth[level]; L.kf_idepthVar = kf->d_idepthVar[level]; L.kf_image = kf->d_image[level];
    L.kf_refBlk = kf->d_refBlk[level];
    L.pts_pos = L.pts_colvar = nullptr; L.npts = -1;
  }
  const int work = npts >= 0 ? npts : L.w * L.h;
  // (strips only where the level has reference blocks: levels >= 1 of a keyframe)
  const LevelTiling T = lsd_level_tiling(work, t->block, t->grid_cap, shape, npts < 0 && L.kf_refBlk != nullptr, batch_env().stripWgs, t->max_blocks);
  L.nblocks = T.nblocks; L.singlePass = T.singlePass; L.tilePx = T.tilePx;
  L.evalBatch = eval_batch_level(t, L);
  L.lambdaInitial = t->lambdaInitial[level]; L.stepSizeMin = t->stepSizeMin[level]; L.convergenceEps = t->convergenceEps[level];
  L.maxIts = t->maxItsPerLvl[level];
  L.minWarped = MIN_GOODPERALL_PIXEL_ABSMIN * (c->w >> level) * (c->h >> level);
  L.writeMask = 0;
  return LSDHIP_OK;
}
static void fill_job_common(lsdhip_tracker* t, TrackJob& job) {
  lsdhip_ctx* c = t->ctx;
  LSD_CTX_LOCK(c);
  memset(&job, 0, sizeof(job));
  job.cameraPixelNoise2 = c->params.cameraPixelNoise2;
  job.var_weight = t->var_weight;
  job.huber_half = t->huber_d / 2;
  job.lambdaSuccessFac = t->lambdaSuccessFac;
  job.lambdaFailFac = t->lambdaFailFac;
  job.useAffine = c->params.useAffineLightningEstimation;
}
// a pose as the C ABI passes it in floats: q (w x y z), t
static lsdm::SE3fH pose_from7(const float* T7) {
  lsdm::SE3fH T;
  T.q = {T7[0], T7[1], T7[2], T7[3]};
  T.t[0] = T7[4]; T.t[1] = T7[5]; T.t[2] = T7[6];
  return T;
}
// referenceToFrame a job ended at
static lsdm::SE3fH pose_of(const TrackSummary* S) {
  const float T7[7] = {S->q[0], S->q[1], S->q[2], S->q[3], S->t[0], S->t[1], S->t[2]};
  return pose_from7(T7);
}
// what a finished LM job leaves in the tracker's public members (SE3Tracker.h:82-93, 185-186)
static void take_summary(lsdhip_tracker* t, const TrackSummary* S) {
  t->numEvaluations = S->numEvaluations;
  t->numWarpUpdates = S->numWarpUpdates;
  t->pointUsage = S->pointUsage; t->lastGoodCount = S->goodCount; t->lastBadCount = S->badCount; t->lastMeanRes = S->meanRes;
  t->affineEstimation_a = S->aff_a; t->affineEstimation_b = S->aff_b;
  t->affineEstimation_a_lastIt = S->aff_a_lastIt; t->affineEstimation_b_lastIt = S->aff_b_lastIt;
  t->lastResidual = S->lastResidual;
}
// the summary of a job whose LM loop ran on the host (debugging path), from the tracker's members: what finish_trackframe expects
static TrackSummary host_lm_summary(const lsdhip_tracker* t, const lsdm::SE3fH& referenceToFrame, float lastResidual) {
  TrackSummary S = *t->h_summary;
  S.diverged = 0;
  S.q[0] = referenceToFrame.q.w; S.q[1] = referenceToFrame.q.x; S.q[2] = referenceToFrame.q.y; S.q[3] = referenceToFrame.q.z;
  S.t[0] = referenceToFrame.t[0]; S.t[1] = referenceToFrame.t[1]; S.t[2] = referenceToFrame.t[2];
  S.lastResidual = lastResidual; S.numEvaluations = t->numEvaluations; S.numWarpUpdates = t->numWarpUpdates;
  S.pointUsage = t->pointUsage; S.goodCount = t->lastGoodCount; S.badCount = t->lastBadCount; S.meanRes = t->lastMeanRes;
  S.aff_a = t->affineEstimation_a; S.aff_b = t->affineEstimation_b;
  S.aff_a_lastIt = t->affineEstimation_a_lastIt; S.aff_b_lastIt = t->affineEstimation_b_lastIt;
  return S;
}
// trackingWasGood of a job that ended at `level` (SE3Tracker.cpp:267-269, 475-477), from the counts the tracker holds
static bool tracking_was_good(const lsdhip_tracker* t, int level) {
  const lsdhip_ctx* c = t->ctx;
  return t->lastGoodCount / (c->wl[level] * c->hl[level]) > MIN_GOODPERALL_PIXEL &&
         t->lastGoodCount / (t->lastGoodCount + t->lastBadCount) > MIN_GOODPERGOODBAD_PIXEL;
}

static TrackScratch scratch_of(lsdhip_tracker* t) { return scratch_at(t, t->d_partials, 1, LSD_SPEC_MAX, LSD_SPEC_MAX); }

// elapsed time of the last profiled launch batch (events are read one call late so that nothing waits for them)
static int prof_collect(lsdhip_ctx* c) {
  if (!c->prof_pending) return LSDHIP_OK;
  HIPCHK(hipEventSynchronize(c->ev_b));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, c->ev_a, c->ev_b));
  c->prof_ms += ms;
  c->prof_pending = false;
  return LSDHIP_OK;
}
int lsd_prof_collect(lsdhip_ctx* c) { return prof_collect(c); }

// ---- developer scaffolding (LSD_DEVTOOLS builds; lsdhip_internal.hpp lists the switches): the functions that run a job call these by
// name, the default library gets the empty stand-ins of the #else branch --------------------------------------------------------------
#ifdef LSD_DEVTOOLS
static int track_device(lsdhip_tracker* t, TrackJob& job, int topLevel, const lsdm::SE3fH& T0, lsdm::SE3fH* Tout);
typedef std::chrono::steady_clock::time_point DevTime;
static DevTime dev_now() { return std::chrono::steady_clock::now(); }
static long long dev_ns_since(DevTime t0) { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(); }
static void dev_log_pointer(lsdhip_tracker* t, TrackSpec& spec) { spec.dbgLog = t->d_log; }
// LSDHIP_TRACK_DEBUG's counters (printed at destroy): jobs, launches queued and the host time that took, budgets that ran out, host time waiting
static void dev_job_begins(lsdhip_tracker* t) { t->dbgJobs++; }
static void dev_launches_queued(lsdhip_tracker* t, int steps, DevTime t0) { t->dbgEnqueued += steps; t->dbgLaunchNs += dev_ns_since(t0); }
static void dev_budget_missed(lsdhip_tracker* t) { t->dbgMisses++; }
struct DevWaitClock {
  lsdhip_tracker* t;
  DevTime t0;
  explicit DevWaitClock(lsdhip_tracker* t_) : t(t_), t0(dev_now()) {}
  ~DevWaitClock() { t->dbgWaitNs += dev_ns_since(t0); }
};
// LSDHIP_DUMP_L0 (with LSDHIP_BUDGET_FIXED=1, after the first budget has drained): what the job's first launch (level `topLevel`, one
// trial) left — it wrote parity 1, trial 0: rows | keys | tail contributions of its tiles, and the state behind them
static int dev_dump_first_launch(lsdhip_tracker* t, const TrackJob& job, int topLevel, int guard) {
  static const bool dumpL0 = getenv("LSDHIP_DUMP_L0") != nullptr;
  if (!dumpL0 || guard != 0 || t->budgetFixed != 1) return LSDHIP_OK;
  const TrackScratch sc = scratch_of(t);
  const size_t rows = (size_t)t->max_blocks;
  const int nb = job.lv[topLevel].nblocks;
  t->dumpL0.assign((size_t)nb * (RS_COLS + 4 + 96) + sizeof(TrackState) / 4, 0u);
  unsigned* d = t->dumpL0.data();
  HIPCHK(hipMemcpy(d, sc.sums + (size_t)(1 * LSD_SPEC_MAX + 0) * RS_COLS * rows, (size_t)nb * RS_COLS * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(d + (size_t)nb * RS_COLS, sc.topkey + (size_t)(1 * LSD_SPEC_MAX + 0) * rows, (size_t)nb * 16, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(d + (size_t)nb * (RS_COLS + 4), sc.topval + (size_t)(1 * LSD_SPEC_MAX + 0) * rows * 96, (size_t)nb * 96 * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(d + (size_t)nb * (RS_COLS + 4 + 96), t->d_state + 1, sizeof(TrackState), hipMemcpyDeviceToHost));
  return LSDHIP_OK;
}
// LSDHIP_LAUNCH_LOG: every launch of the job has been queued; wait for the ones behind the finishing launch too, then keep the log and clear it
static int dev_keep_launch_log(lsdhip_tracker* t) {
  static const bool keepLog = getenv("LSDHIP_LAUNCH_LOG") != nullptr;
  if (!keepLog) return LSDHIP_OK;
  HIPCHK(hipStreamSynchronize(t->ctx->stream));
  const int n = t->launchOrdinal < 4095 ? t->launchOrdinal + 1 : 4096;
  t->lastLog.assign((size_t)n * 16, 0);
  HIPCHK(hipMemcpy(t->lastLog.data(), t->d_log, (size_t)n * 64, hipMemcpyDeviceToHost));
  HIPCHK(hipMemset(t->d_log, 0, (size_t)n * 64));
  return LSDHIP_OK;
}
// LSDHIP_TRACE_SUMS entries of a job.  Its inputs (LSDHIP_TRACE_INPUTS), kinds base + ..:
static void dev_trace_inputs(lsdhip_ctx* c, const lsdhip_frame* kf, const lsdhip_frame* frame, int base) {
  static const bool traceInputs = getenv("LSDHIP_TRACE_INPUTS") != nullptr;
  if (!traceInputs) return;
  for (int l = 1; l <= 4; l++) {
    const size_t nl = (size_t)c->wl[l] * c->hl[l];
    lsd_trace_sum(c, c->stream, base + 10 + l, frame->id, kf->d_idepth[l], nl * 4);
    lsd_trace_sum(c, c->stream, base + 14 + l, frame->id, kf->d_idepthVar[l], nl * 4);
    lsd_trace_sum(c, c->stream, base + 50 + l, frame->id, kf->d_image[l], nl * 4);
    lsd_trace_sum(c, c->stream, base + 54 + l, frame->id, frame->d_grad[l], nl * 16);
  }
}
// ... the pose it starts from and its keyframe (kinds 22, 23)
static void dev_trace_job(lsdhip_ctx* c, const lsdhip_frame* kf, const lsdhip_frame* frame, const double init[7]) {
  dev_trace_inputs(c, kf, frame, 0);
  unsigned long long pv = 0;
  for (int i = 0; i < 7; i++) { unsigned long long u; memcpy(&u, &init[i], 8); pv = pv * 1000003ull + u; }
  lsd_trace_val(c, 22, frame->id, pv);
  lsd_trace_val(c, 23, frame->id, (unsigned long long)kf->id);
}
// ... the workgroups launched before it (in units of a 640x480 job's grid)
static void dev_trace_launched(lsdhip_tracker* t, int kind, const lsdhip_frame* frame) { lsd_trace_val(t->ctx, kind, frame->id, t->dbgCum / 400ull); }
// ... and its result: the hash of the pose's seven words (kind), evaluations and last executed trial (kind + 1)
static void dev_trace_result(lsdhip_tracker* t, int kind, const lsdhip_frame* frame) {
  const TrackSummary* S = t->h_summary;
  unsigned long long pv = 0;
  for (int i = 0; i < 4; i++) { unsigned u; memcpy(&u, &S->q[i], 4); pv = pv * 1000003ull + u; }
  for (int i = 0; i < 3; i++) { unsigned u; memcpy(&u, &S->t[i], 4); pv = pv * 1000003ull + u; }
  lsd_trace_val(t->ctx, kind, frame->id, pv);
  lsd_trace_val(t->ctx, kind + 1, frame->id, (unsigned long long)S->numEvaluations * 1000 + S->lastCand);
}
// LSDHIP_TRACK_REPLAY (pipelined contexts): the job that has just ended with `rc`, once more with the mapping stream drained — identical
// inputs must give the identical result; the first launches' dumps (LSDHIP_DUMP_L0) are compared word by word.  Returns the replay's rc.
static int dev_replay_check(lsdhip_tracker* t, TrackJob& job, const lsdhip_frame* kf, const lsdhip_frame* frame, const lsdm::SE3fH& T0,
                            lsdm::SE3fH* Tout, int rc) {
  static const bool replay = getenv("LSDHIP_TRACK_REPLAY") != nullptr;
  lsdhip_ctx* c = t->ctx;
  if (!replay || !c->pipeline) return rc;
  dev_trace_result(t, 24, frame);
  HIPCHK(hipStreamSynchronize(c->mstream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->mDoneSeq = c->mSeq;
  const std::vector<unsigned> dump1 = t->dumpL0;
  dev_trace_inputs(c, kf, frame, 100);
  dev_trace_launched(t, 27, frame);
  rc = track_device(t, job, LSD_TRACK_MAX_LEVEL - 1, T0, Tout);
  if (rc != LSDHIP_OK && rc != LSDHIP_DIVERGED) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  if (!dump1.empty() && dump1.size() == t->dumpL0.size()) {
    const int nb = job.lv[LSD_TRACK_MAX_LEVEL - 1].nblocks;
    int shown = 0;
    for (size_t i = 0; i < dump1.size(); i++)
      if (dump1[i] != t->dumpL0[i] && shown++ < 12) {
        const size_t a = (size_t)nb * RS_COLS, b = a + (size_t)nb * 4, cst = b + (size_t)nb * 96;
        float f1, f2; memcpy(&f1, &dump1[i], 4); memcpy(&f2, &t->dumpL0[i], 4);
        if (i < a) fprintf(stderr, "L0DIFF frame %d: sums tile %zu column %zu: run %.9g (%08x) replay %.9g (%08x)\n", frame->id, i / RS_COLS, i % RS_COLS, f1, dump1[i], f2, t->dumpL0[i]);
        else if (i < b) fprintf(stderr, "L0DIFF frame %d: topkey tile %zu [%zu]: run %d replay %d\n", frame->id, (i - a) / 4, (i - a) % 4, (int)dump1[i], (int)t->dumpL0[i]);
        else if (i < cst) fprintf(stderr, "L0DIFF frame %d: topval tile %zu slot %zu entry %zu: run %.9g replay %.9g\n", frame->id, (i - b) / 96, ((i - b) % 96) / 32, (i - b) % 32, f1, f2);
        else fprintf(stderr, "L0DIFF frame %d: state word %zu: run %08x (%.9g) replay %08x (%.9g)\n", frame->id, i - cst, dump1[i], f1, t->dumpL0[i], f2);
      }
    if (shown) fprintf(stderr, "L0DIFF frame %d: %d words differ after the first launch\n", frame->id, shown);
  }
  return rc;
}
#else
struct DevTime {};
inline DevTime dev_now() { return {}; }
inline void dev_log_pointer(lsdhip_tracker*, TrackSpec&) {}
inline void dev_job_begins(lsdhip_tracker*) {}
inline void dev_launches_queued(lsdhip_tracker*, int, DevTime) {}
inline void dev_budget_missed(lsdhip_tracker*) {}
struct DevWaitClock { explicit DevWaitClock(lsdhip_tracker*) {} };
inline int dev_dump_first_launch(lsdhip_tracker*, const TrackJob&, int, int) { return LSDHIP_OK; }
inline int dev_keep_launch_log(lsdhip_tracker*) { return LSDHIP_OK; }
inline void dev_trace_job(lsdhip_ctx*, const lsdhip_frame*, const lsdhip_frame*, const double*) {}
inline void dev_trace_launched(lsdhip_tracker*, int, const lsdhip_frame*) {}
inline void dev_trace_result(lsdhip_tracker*, int, const lsdhip_frame*) {}
inline int dev_replay_check(lsdhip_tracker*, TrackJob&, const lsdhip_frame*, const lsdhip_frame*, const lsdm::SE3fH&, lsdm::SE3fH*, int rc) { return rc; }
#endif

// progress tag of the launch queued last (TrackSummary::seq): (job tag << 12) | launch ordinal; 0 for jobs nobody polls for
static int launch_seq(const lsdhip_tracker* t) { return t->jobTag ? ((t->jobTag << 12) | (t->launchOrdinal & 0xFFF)) : 0; }
// one k_track_step launch of a single job; `last`: the last launch of the enqueued budget
static void launch_step(lsdhip_tracker* t, const TrackJob& job, TrackSpec spec, int grid, int parity, int first, int last) {
  lsdhip_ctx* c = t->ctx;
  LSD_CTX_LOCK(c);
  TrackScratch sc = scratch_of(t);
  t->launchOrdinal++;
  spec.seq = launch_seq(t);
  spec.last = last;
  spec.levelTiles = 0; spec.levelTrials = 0;
  for (int l = 0; l < LSD_LEVELS; l++) {
    spec.levelTiles |= (unsigned long long)(job.lv[l].nblocks & 0xFFF) << (12 * l);
    spec.levelTrials |= (unsigned)((spec.specC > 1 && spec.trials[l] > 1) ? spec.trials[l] : 1) << (4 * l);   // (trials_at)
  }
  dev_log_pointer(t, spec);
#ifdef LSD_ORDER_CHECK
  spec.dbgCum = t->dbgCum;
  spec.dbgCounters = t->d_dbg;
  t->dbgCum += (unsigned long long)grid;
#endif
  hipLaunchKernelGGL((k_track_step<256, false>), dim3(grid), dim3(256), 0, c->stream, job, (const TrackJob*)nullptr, t->d_state, sc,
                     t->d_summary, parity, first, spec);
}
// launch `steps` fused k_track_step kernels of `grid` workgroups (alternating parity)
static int launch_steps(lsdhip_tracker* t, const TrackJob& job, const TrackSpec& spec, int grid, int steps, int* parity, int* first) {
  const DevTime tl0 = dev_now();
  for (int i = 0; i < steps; i++) {
    launch_step(t, job, spec, grid, *parity, *first, i + 1 == steps);
    lsdhip_host_mark(20);
    *first = 0;
    *parity ^= 1;
  }
  dev_launches_queued(t, steps, tl0);
  HIPCHK(hipGetLastError());
  return LSDHIP_OK;
}
struct EvalOut {       // what one evaluation leaves behind, in the reference's terms
  int warped_size;
  float retval;        // calcResidualAndBuffers return value
  float weightedError; // calcWeightsAndResidualSSE return value
  float A[36], b[6], lsError;
  double num_constraints;
};

// an evaluation's summary in the reference's terms (the normalisation of LGS6::finish, LGSX.h:319-325)
static void eval_out_of(const TrackSummary* S, EvalOut* eo) {
  const float* r = S->sums;
  int M = (int)r[RS_M];
  eo->warped_size = M;
  eo->retval = r[RS_SUMRES2] / r[RS_GOOD];
  eo->weightedError = r[RS_WERR] / ((M >> 2) << 2);
  size_t num_constraints = (size_t)6 * (size_t)(M >> 2);
  float n = (float)num_constraints;
  int k = RS_A0;
  for (int i = 0; i < 6; i++)
    for (int j = i; j < 6; j++, k++) {
      float v = (0.0f + r[k]) / n;
      eo->A[i * 6 + j] = v;
      eo->A[j * 6 + i] = v;
    }
  for (int i = 0; i < 6; i++) eo->b[i] = (0.0f - r[RS_B0 + i]) / n;
  eo->lsError = (0.0f + r[RS_ERR]) / n;
  eo->num_constraints = (double)num_constraints;
}

// one evaluation with a host round trip (evalOnly job): kernel-level parity hook and host-LM debugging path
static int evaluate_pose(lsdhip_tracker* t, TrackJob& job, const lsdm::SE3fH& T, int level, EvalOut* eo) {
  lsdhip_ctx* c = t->ctx;
  LSD_CTX_LOCK(c);
  job.evalOnly = 1;
  job.lastLevel = level;
  job.topLevel = level;
  job.T0 = T;
  job.aff_a0 = t->affineEstimation_a; job.aff_b0 = t->affineEstimation_b;
  t->h_summary->done = 0;
  t->jobTag = 0;
  const TrackSpec spec = TrackSpec{};                 // one evaluation, one trial
  if (int rcp = prof_collect(c)) return rcp;
  if (c->prof_on) HIPCHK(hipEventRecord(c->ev_a, c->stream));
  launch_step(t, job, spec, job.lv[level].nblocks, 0, 1, 0);   // residual evaluation
  if (c->prof_on) HIPCHK(hipEventRecord(c->ev_b, c->stream));
  launch_step(t, job, spec, 1, 1, 0, 0);                       // finalises the sums (evalOnly)
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  const TrackSummary* S = t->h_summary;
  if (c->prof_on) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->ev_a, c->ev_b));
    c->prof_ms += ms;
    c->prof_launches++;
    c->prof_bytes += S->bytes;
  }
  // (not take_summary: the accepted affine pair, the warp updates and the last residual belong to the host's LM loop around this evaluation)
  t->numEvaluations++;
  t->pointUsage = S->pointUsage; t->lastGoodCount = S->goodCount; t->lastBadCount = S->badCount; t->lastMeanRes = S->meanRes;
  t->affineEstimation_a_lastIt = S->aff_a_lastIt; t->affineEstimation_b_lastIt = S->aff_b_lastIt;
  eval_out_of(S, eo);
  return LSDHIP_OK;
}

// the record of one evaluation (lsdhip_tracker_evaluate, lsdhip_tracker_evaluate_batch)
static void record_of(const TrackSummary* S, lsdhip_residual_record* out) {
  EvalOut ev;
  eval_out_of(S, &ev);
  out->warped_size = ev.warped_size;
  out->goodCount = S->goodCount; out->badCount = S->badCount; out->pointUsage = S->pointUsage;
  out->meanRes = S->meanRes; out->retval = ev.retval;
  out->affine_a_lastIt = S->aff_a_lastIt; out->affine_b_lastIt = S->aff_b_lastIt;
  out->weightedError = ev.weightedError;
  memcpy(out->A, ev.A, sizeof(ev.A)); memcpy(out->b, ev.b, sizeof(ev.b));
  out->lsError = ev.lsError; out->num_constraints = ev.num_constraints;
}

// host-driven LM for one level (debugging path): SE3Tracker.cpp:323-449
static int lm_level_host(lsdhip_tracker* t, TrackJob& job, int lvl, lsdm::SE3fH& referenceToFrame, float* lastResidualOut) {
  lsdhip_ctx* c = t->ctx;
  LSD_CTX_LOCK(c);
  const TrackLevel& L = job.lv[lvl];
  EvalOut ev;
  int rc = evaluate_pose(t, job, referenceToFrame, lvl, &ev);
  if (rc) return rc;
  if (ev.warped_size < L.minWarped) return LSDHIP_DIVERGED;
  if (c->params.useAffineLightningEstimation) {
    t->affineEstimation_a = t->affineEstimation_a_lastIt;
    t->affineEstimation_b = t->affineEstimation_b_lastIt;
  }
  float lastErr = ev.weightedError;
  float LM_lambda = L.lambdaInitial;
  EvalOut cur = ev;
  for (int iteration = 0; iteration < L.maxIts; iteration++) {
    t->numWarpUpdates++;
    int incTry = 0;
    while (true) {
      float b[6], A[36], inc[6];
      for (int i = 0; i < 6; i++) b[i] = -cur.b[i];
      memcpy(A, cur.A, sizeof(A));
      for (int i = 0; i < 6; i++) A[i * 6 + i] *= 1 + LM_lambda;
      lsdm::ldlt6_solve(A, b, inc);
      incTry++;
      lsdm::SE3fH new_referenceToFrame = lsdm::se3f_mul(lsdm::se3f_exp(inc), referenceToFrame);
      EvalOut nev;
      rc = evaluate_pose(t, job, new_referenceToFrame, lvl, &nev);
      if (rc) return rc;
      if (nev.warped_size < L.minWarped) return LSDHIP_DIVERGED;
      float error = nev.weightedError;
      if (error < lastErr) {
        referenceToFrame = new_referenceToFrame;
        cur = nev;
        if (c->params.useAffineLightningEstimation) {
          t->affineEstimation_a = t->affineEstimation_a_lastIt;
          t->affineEstimation_b = t->affineEstimation_b_lastIt;
        }
        if (error / lastErr > L.convergenceEps) iteration = L.maxIts;
        lastErr = error;
        if (job.trackFrameSemantics) *lastResidualOut = error;
        if (LM_lambda <= 0.2) LM_lambda = 0;
        else LM_lambda *= t->lambdaSuccessFac;
        break;
      } else {
        float incdot = (inc[0] * inc[0] + (inc[1] * inc[1] + inc[2] * inc[2])) + (inc[3] * inc[3] + (inc[4] * inc[4] + inc[5] * inc[5]));
        if (!(incdot > L.stepSizeMin)) { iteration = L.maxIts; break; }
        if (LM_lambda == 0) LM_lambda = 0.2;
        else LM_lambda *= std::pow(t->lambdaFailFac, incTry);
      }
    }
  }
  if (!job.trackFrameSemantics) *lastResidualOut = lastErr;
  return LSDHIP_OK;
}

// A polled summary is accepted when its words add up to its `check` word: `done` has arrived, but the record's other words are separate
// posted writes and — one job in a few thousand, measured (profiles/r06_notes.md section 1) — the ones stored last (numLaunches, lastCand,
// levelEvals) still held the previous job's values at that moment.  Spins until the record is whole; counts what it saw.
static int summary_wait_consistent(lsdhip_tracker* t, const int doneWord, const TrackSummary* rec = nullptr) {
  if (!rec) rec = t->h_summary;
  volatile const unsigned* w = (volatile const unsigned*)rec;
  unsigned cur[LSD_SUMMARY_CHECK_WORDS], chk = 0, want = 0;
  auto whole = [&]() {
    chk = (unsigned)doneWord;
    for (unsigned i = 1; i < LSD_SUMMARY_CHECK_WORDS; i++) { cur[i] = w[i]; chk += lsd_summary_term(i, cur[i]); }
    want = *(volatile const unsigned*)&rec->check;
    return chk == want;
  };
  t->sumPolled++;
  if (whole()) { std::atomic_thread_fence(std::memory_order_acquire); return LSDHIP_OK; }
  t->sumLate++;
  unsigned first[LSD_SUMMARY_CHECK_WORDS];
  memcpy(first, cur, sizeof(first));
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = lsd_spin_until(t->ctx, whole, t0 + std::chrono::seconds(LSD_SUMMARY_WAIT_S), LSD_WAIT_RECORD);
  if (rc == LSDHIP_E_STATE) lsd_set_error("tracking summary in pinned memory never became consistent (check %08x, sum %08x)", want, chk);
  if (rc) return rc;
  const long long ns = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
  if (ns > t->sumLateMaxNs) t->sumLateMaxNs = ns;
  for (unsigned i = 1; i < LSD_SUMMARY_CHECK_WORDS; i++)
    if (first[i] != cur[i]) {
      t->sumLateWords++;
      if (t->sumLateFirstWord < 0 || (int)i < t->sumLateFirstWord) t->sumLateFirstWord = (int)i;
      if ((int)i > t->sumLateLastWord) t->sumLateLastWord = (int)i;
    }
  return LSDHIP_OK;
}
extern "C" int lsdhip_tracker_summary_stats(const lsdhip_tracker* t, long long out[6]) {
  if (!t || !out) return LSDHIP_E_ARG;
  out[0] = t->sumPolled; out[1] = t->sumLate; out[2] = t->sumLateMaxNs; out[3] = t->sumLateWords; out[4] = t->sumLateFirstWord; out[5] = t->sumLateLastWord;
  return LSDHIP_OK;
}

// The loop every device-resident job (or batch of jobs) runs through: enqueue a budget of launches, let the caller's hook queue what the
// device can do beside them (once), wait for the reports, and top the budget up while a job needs more.  With `sample`, a budget is
// bracketed by one HIP event pair on the context's stream (read one call late, prof_collect).
//   enqueue(budget) -> rc               queues `budget` launches
//   wait(guard, &finished) -> rc        returns with every job finished, or with the stream drained and some job not
//   topUp(guard) -> the next budget     (a job may start over here: lsdhip_tracker_track's keyframe check)
template <class Enqueue, class Wait, class TopUp>
static int run_budgets(lsdhip_tracker* t, bool sample, bool hook, int budget, const char* what, Enqueue enqueue, Wait wait, TopUp topUp) {
  lsdhip_ctx* c = t->ctx;
  for (int guard = 0; guard <= 200; guard++) {
    if (sample) HIPCHK(hipEventRecord(c->ev_a, c->stream));
    if (int rc = enqueue(budget)) return rc;
    if (sample) { HIPCHK(hipEventRecord(c->ev_b, c->stream)); c->prof_pending = true; }
    if (guard == 0 && hook && t->enqueueHook) t->enqueueHook(t->enqueueHookUser);
    bool finished = false;
    if (int rc = wait(guard, &finished)) return rc;
    if (finished) return LSDHIP_OK;
    if (int rc = prof_collect(c)) return rc;
    budget = topUp(guard);
  }
  lsd_set_error("%s did not terminate", what);
  return LSDHIP_E_STATE;
}

// The side planes (refPixelWasGood of trials 1 ..) the job being launched writes: two sets, alternating by job — on a pipelined context
// the merge of job t's final mask runs on the mapping stream while job t + 1 writes the other set.
static uint8_t* side_planes(const lsdhip_tracker* t) { return t->d_maskSide + (size_t)t->maskSet * t->maskStride * (LSD_SPEC_MAX - 1); }
static int claim_side_planes(lsdhip_tracker* t) {
  lsdhip_ctx* c = t->ctx;
  t->maskSet ^= 1;
  if (c->pipeline && t->maskMergeSeq[t->maskSet] != 0) {
    // the merge that reads this set (noted two jobs ago) must have run before the set is overwritten (in a frame loop a mapping
    // operation has queued it long ago and the job's own frame was created behind it)
    if (t->maskMergeSeq[t->maskSet] < 0) { if (int rcf = lsd_flush_merges(c)) return rcf; }
    if (t->maskMergeSeq[t->maskSet] > c->mSeq && lsd_m_record(c) < 0) return LSDHIP_E_HIP;
    if (int rcw = lsd_t_wait_m(c, t->maskMergeSeq[t->maskSet])) return rcw;
    t->maskMergeSeq[t->maskSet] = 0;
  }
  return LSDHIP_OK;
}
// The plan of a single job's launches (track_plan.hpp) under the tracker's speculation settings; the job's tilings become the plan's.
static SinglePlan plan_job(const lsdhip_tracker* t, TrackJob& job) {
  LevelWork lv[LSD_LEVELS];
  SpecPolicy p;
  p.specC = t->specC; p.specAuto = t->specAuto; p.specCap = t->specCap; p.grid_cap = t->grid_cap; p.block = t->block;
  for (int l = 0; l < LSD_LEVELS; l++) {
    const TrackLevel& L = job.lv[l];
    lv[l] = {L.npts >= 0 ? (long long)L.npts : (long long)L.w * L.h, {L.nblocks, L.singlePass, L.tilePx}};
    p.specLevel[l] = t->specLevel[l]; p.specCaps[l] = t->specCaps[l];
  }
  const SinglePlan P = lsd_single_plan(lv, p, job.lastLevel, job.topLevel);
  for (int l = 0; l < LSD_LEVELS; l++) {
    job.lv[l].nblocks = P.tiling[l].nblocks; job.lv[l].singlePass = P.tiling[l].singlePass;
    job.lv[l].evalBatch = eval_batch_level(t, job.lv[l]);
  }
  return P;
}
// ... and the TrackSpec its launches take (launch_step adds the per-launch fields)
static TrackSpec job_spec(const lsdhip_tracker* t, const SinglePlan& P) {
  TrackSpec spec = TrackSpec{};
  spec.specC = t->specC;
  spec.specGrid = P.specGrid;
  for (int l = 0; l < LSD_LEVELS; l++) spec.trials[l] = P.trials[l];
  spec.wasGoodSide = side_planes(t);
  spec.maskStride = (unsigned)t->maskStride;
  spec.copyMask = t->ctx->pipeline ? 0 : 1;
#ifdef LSD_PHASE_TRACE
  spec.traceWg = batch_env().traceWg;
#endif
  return spec;
}

// device-resident LM over levels topLevel..job.lastLevel; one host synchronisation per budget of launches.  Launches of the k_track_step
// chain a job needs = its evaluating launches + the finalising step; the budget is the most of the recent jobs plus a margin (launches
// queued behind the finishing one leave at once, ~4 us each).  While profiling, every 8th job's budget is timed and charged to the
// launches that did work (two event packets and a host-side event query per job cost ~5 % of a frame).
static int track_device(lsdhip_tracker* t, TrackJob& job, int topLevel, const lsdm::SE3fH& T0, lsdm::SE3fH* Tout) {
  lsdhip_ctx* c = t->ctx;
  // (the caller — an extern "C" entry — holds the context mutex once; it is released below while the host waits)
  job.evalOnly = 0;
  job.topLevel = topLevel;
  job.T0 = T0;
  job.aff_a0 = 1.0f; job.aff_b0 = 0.0f;
  if (int rc = claim_side_planes(t)) return rc;
  const SinglePlan plan = plan_job(t, job);
  const TrackSpec spec = job_spec(t, plan);
  TrackSummary* S = t->h_summary;
  volatile const int* done = &S->done;
  S->done = 0;
  const long long myEpoch = ++c->enqEpoch;   // everything enqueued on the stream so far precedes this job
  const bool sample = c->prof_on && ((c->prof_tick++ & 7) == 0);
  dev_job_begins(t);
  t->jobTag = (t->jobTag % 0x7FFFF) + 1;
  t->launchOrdinal = 0;
  S->seq = 0;
  S->exhausted = 0;
  int parity = 0, first = 1;
  if (int rc = prof_collect(c)) return rc;
  lsdhip_host_mark(2);
  auto enqueue = [&](int budget) {
    const int rc = launch_steps(t, job, spec, plan.grid, budget, &parity, &first);
    lsdhip_host_mark(3);
    return rc;
  };
  // The finishing step writes the summary to pinned host memory and raises `done` last (system-scope fence in between): poll it instead
  // of sleeping in hipStreamSynchronize, whose wake-up costs more than two evaluations; the budget's last launch says so if it leaves the
  // job unfinished (`exhausted`).  Steps of the budget still queued behind the finishing one exit immediately; later work is stream-ordered.
  auto wait = [&](int guard, bool* finished) -> int {
    lsdhip_host_mark(4);
    DevWaitClock waitClock_(t);
    {
      LsdCtxUnlocked unlocked_(c);   // let the mapping thread enqueue
      if (t->spinWait) {
        volatile const int* exhausted = &S->exhausted;
        const int tag = t->jobTag, lastSeq = launch_seq(t);
        if (int rc = lsd_spin_until(c, [=]() { return *done == tag || *exhausted == lastSeq; }, lsd_deadline(LSD_JOB_WAIT_S), LSD_WAIT_JOB)) return rc;
      } else {
        HIPCHK(hipStreamSynchronize(c->stream));
      }
    }
    lsdhip_host_mark(5);
    if (*done != t->jobTag) {
      dev_budget_missed(t);
      HIPCHK(hipStreamSynchronize(c->stream));   // out of budget: rare
      if (int rc = dev_dump_first_launch(t, job, topLevel, guard)) return rc;
    }
    *finished = *done == t->jobTag;
    return LSDHIP_OK;
  };
  auto topUp = [&](int guard) {
    if (t->jobKf && t->jobKf->depthVersion != t->jobKfVersion && guard < 8) {
      // While the host waited without the context lock, the mapping thread rewrote the keyframe's depth planes (setDepth): the
      // launches appended now would read the new planes in the middle of a job that started on the old ones.  The reference's
      // TrackingReference is a snapshot that cannot change under a job, so run the job again, whole, on the planes as they are now.
      t->jobKfVersion = t->jobKf->depthVersion;
      S->done = 0;
      parity = 0; first = 1;
      return 12;
    }
    return t->budgetFixed > 0 ? t->budgetFixed : 6;
  };
  if (int rc = run_budgets(t, sample, job.trackFrameSemantics != 0, t->recent.budget(12, t->budgetExtra, t->budgetFixed), "tracking job", enqueue, wait, topUp))
    return rc;
  // `done` is in; the rest of the record is taken only once it adds up (summary_wait_consistent)
  if (int rcs = summary_wait_consistent(t, t->jobTag)) return rcs;
  if (sample) {
    c->prof_bytes += S->bytes;
    c->prof_launches += S->numLaunches;
  }
  if (myEpoch > c->doneEpoch) c->doneEpoch = myEpoch;
  if (int rc = dev_keep_launch_log(t)) return rc;
  t->numLaunches = S->numLaunches;
  t->recent.note(t->numLaunches);
  for (int l = 0; l < LSD_LEVELS; l++) t->levelEvaluations[l] = S->levelEvals[l];
  take_summary(t, S);
  *Tout = pose_of(S);
  return S->diverged ? LSDHIP_DIVERGED : LSDHIP_OK;
}

static void fill_result(lsdhip_tracker* t, const lsdm::SE3dH& T, lsdhip_track_result* out) {
  lsdm::se3d_to7(T, out->frameToReference);
  out->pointUsage = t->pointUsage; out->lastGoodCount = t->lastGoodCount; out->lastBadCount = t->lastBadCount;
  out->lastMeanRes = t->lastMeanRes; out->lastResidual = t->lastResidual;
  out->affineEstimation_a = t->affineEstimation_a; out->affineEstimation_b = t->affineEstimation_b;
  out->diverged = t->diverged; out->trackingWasGood = t->trackingWasGood;
  out->numEvaluations = t->numEvaluations; out->numWarpUpdates = t->numWarpUpdates;
}
static lsdm::SE3dH identity_d() { lsdm::SE3dH I; I.q = {1, 0, 0, 0}; I.t[0] = I.t[1] = I.t[2] = 0; return I; }
// a diverged job's flags and result: the identity, like the reference (SE3Tracker.cpp:324-329)
static int finish_diverged(lsdhip_tracker* t, lsdhip_track_result* out) {
  t->diverged = true;
  t->trackingWasGood = false;
  fill_result(t, identity_d(), out);
  return LSDHIP_DIVERGED;
}

// trackFrame job description (SE3Tracker.cpp:280-322): levels SE3TRACKING_MAX_LEVEL-1 .. SE3TRACKING_MIN_LEVEL
static int fill_trackframe_job(lsdhip_tracker* t, TrackJob& job, BatchShape shape, lsdhip_frame* kf, lsdhip_frame* frame) {
  fill_job_common(t, job);
  for (int lvl = LSD_TRACK_MIN_LEVEL; lvl < LSD_TRACK_MAX_LEVEL; lvl++)
    if (int rcl = fill_level(t, job, shape, lvl, kf, frame, nullptr, nullptr, -1)) return rcl;
  job.lv[LSD_TRACK_MIN_LEVEL].writeMask = 1;
  int rc = lsd_frame_ensure_wasgood(frame);
  if (rc) return rc;
  job.wasGood = frame->d_wasGood;
  job.lastLevel = LSD_TRACK_MIN_LEVEL;
  job.trackFrameSemantics = 1;
  return LSDHIP_OK;
}
// one evaluation (calcResidualAndBuffers .. calcWeightsAndResidual, the normal equations) at `level`, pose T7 and the affine pair
static int fill_eval_job(lsdhip_tracker* t, TrackJob& job, BatchShape shape, lsdhip_frame* kf, lsdhip_frame* frame, int level, const float T7[7],
                         float aff_a, float aff_b) {
  fill_job_common(t, job);
  if (int rcl = fill_level(t, job, shape, level, kf, frame, nullptr, nullptr, -1)) return rcl;
  if (level == LSD_TRACK_MIN_LEVEL) {
    if (int rc = lsd_frame_ensure_wasgood(frame)) return rc;
    job.wasGood = frame->d_wasGood;
    job.lv[level].writeMask = 1;
  }
  job.trackFrameSemantics = 1;
  job.evalOnly = 1;
  job.lastLevel = level;
  job.topLevel = level;
  job.T0 = pose_from7(T7);
  job.aff_a0 = aff_a; job.aff_b0 = aff_b;
  return LSDHIP_OK;
}
// trackFrameOnPermaref job description (SE3Tracker.cpp:162-272): `npts` reference points against the frame at QUICK_KF_CHECK_LVL, from T0
static int fill_permaref_job(lsdhip_tracker* t, TrackJob& job, BatchShape shape, const float* pts_pos, const float* pts_colvar, int npts,
                             lsdhip_frame* frame, const lsdm::SE3fH& T0) {
  const int L = LSD_QUICK_KF_CHECK_LVL;
  fill_job_common(t, job);
  if (int rcl = fill_level(t, job, shape, L, nullptr, frame, pts_pos, pts_colvar, npts)) return rcl;
  job.lv[L].lambdaInitial = t->lambdaInitialTestTrack; job.lv[L].stepSizeMin = t->stepSizeMinTestTrack;
  job.lv[L].convergenceEps = t->convergenceEpsTestTrack; job.lv[L].maxIts = (int)t->maxItsTestTrack;
  job.lastLevel = L;
  job.topLevel = L;
  job.trackFrameSemantics = 0;
  job.evalOnly = 0;
  job.T0 = T0;
  job.aff_a0 = 1.0f; job.aff_b0 = 0.0f;
  return LSDHIP_OK;
}
// epilogue of trackFrameOnPermaref (SE3Tracker.cpp:254-272) from the counters the job left in the tracker
static int finish_permaref(lsdhip_tracker* t, bool diverged, const lsdm::SE3fH& referenceToFrame, lsdhip_track_result* out) {
  if (diverged) return finish_diverged(t, out);
  t->diverged = false;
  t->trackingWasGood = tracking_was_good(t, LSD_QUICK_KF_CHECK_LVL);   // (the reference's `!diverged &&` is this branch)
  fill_result(t, lsdm::se3d_from_f(referenceToFrame), out);
  return LSDHIP_OK;
}
// epilogue of trackFrame (SE3Tracker.cpp:451-485) from the job's summary: flags, frame / keyframe side effects, result
static int finish_trackframe(lsdhip_tracker* t, const TrackSummary* S, lsdhip_frame* kf, lsdhip_frame* frame, lsdhip_track_result* out) {
  lsdhip_ctx* c = t->ctx;
  LSD_CTX_LOCK(c);
  take_summary(t, S);
  if (S->diverged) return finish_diverged(t, out);
  t->diverged = false;
  t->trackingWasGood = tracking_was_good(t, LSD_TRACK_MIN_LEVEL);
  if (t->trackingWasGood) kf->numFramesTrackedOnThis++;
  frame->initialTrackedResidual = t->lastResidual / t->pointUsage;
  lsdm::SE3dH f2r = lsdm::se3d_from_f(lsdm::se3f_inverse(pose_of(S)));
  frame->thisToParent_raw.q = f2r.q;
  lsdm::q_normalize(frame->thisToParent_raw.q);   // sim3FromSE3 -> Sim3::setScale normalises the quaternion (rxso3.hpp:332-335)
  frame->thisToParent_raw.t[0] = f2r.t[0]; frame->thisToParent_raw.t[1] = f2r.t[1]; frame->thisToParent_raw.t[2] = f2r.t[2];
  frame->thisToParent_raw.s = 1;
  frame->trackingParent = kf;
  frame->trackingParentID = kf->id;
  fill_result(t, f2r, out);
  return LSDHIP_OK;
}

extern "C" int lsdhip_tracker_track(lsdhip_tracker* t, lsdhip_frame* kf, lsdhip_frame* frame, const double init[7],
                                    lsdhip_track_result* out) {
  if (!t || !kf || !frame || !init || !out) return LSDHIP_E_ARG;
  if (!kf->hasIDepth) { lsd_set_error("lsdhip_tracker_track: keyframe %d has no depth", kf->id); return LSDHIP_E_STATE; }
  lsdhip_ctx* c = t->ctx;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  t->diverged = false;
  t->trackingWasGood = true;
  t->affineEstimation_a = 1; t->affineEstimation_b = 0;
  t->numEvaluations = 0; t->numWarpUpdates = 0;
  TrackJob job;
  // pipelined contexts: the job reads the frame's pyramids and the keyframe's image pyramid + published depth planes, all products of
  // the mapping stream; it does NOT wait for mapping work queued behind those points (DepthMap::updateKeyframe of the previous frame)
  LsdTrackJobScope tjob_(c, false);
  if (c->pipeline) {
    long long need = frame->readySeq > kf->readySeq ? frame->readySeq : kf->readySeq;
    if (kf->depthSeq > need) need = kf->depthSeq;
    if (int rcw = lsd_t_wait_m(c, need)) return rcw;
  }
  int rc = fill_trackframe_job(t, job, BatchShape{}, kf, frame);
  if (rc) return rc;
  if (int rcg = lsd_gate_open(c)) return rcg;
  if (int rcd = lsd_pipe_dummy(c)) return rcd;
  dev_trace_job(c, kf, frame, init);
  lsdm::SE3fH referenceToFrame = lsdm::se3f_from_d(lsdm::se3d_inverse(lsdm::se3d_from7(init)));

  if (t->hostLM) {
    float last_residual = 0;
    rc = LSDHIP_OK;
    for (int lvl = LSD_TRACK_MAX_LEVEL - 1; lvl >= LSD_TRACK_MIN_LEVEL && rc == LSDHIP_OK; lvl--)
      rc = lm_level_host(t, job, lvl, referenceToFrame, &last_residual);
    t->lastResidual = last_residual;
    if (rc == LSDHIP_DIVERGED) return finish_diverged(t, out);
    if (rc) return rc;
    const TrackSummary S = host_lm_summary(t, referenceToFrame, last_residual);
    return finish_trackframe(t, &S, kf, frame, out);
  }
  t->jobKf = kf;
  t->jobKfVersion = kf->depthVersion;
  const lsdm::SE3fH T0 = referenceToFrame;
  dev_trace_launched(t, 26, frame);
  rc = track_device(t, job, LSD_TRACK_MAX_LEVEL - 1, T0, &referenceToFrame);
  if (rc == LSDHIP_OK || rc == LSDHIP_DIVERGED) rc = dev_replay_check(t, job, kf, frame, T0, &referenceToFrame, rc);
  t->jobKf = nullptr;
  if (rc != LSDHIP_OK && rc != LSDHIP_DIVERGED) return rc;
  lsdhip_host_mark(6);
  dev_trace_result(t, 20, frame);
  if (c->pipeline && rc == LSDHIP_OK && t->h_summary->lastCand > 0 && t->h_summary->level == LSD_TRACK_MIN_LEVEL) {
    // the final mask sits in a side plane: to be merged into the frame's plane on the mapping stream, ahead of whatever reads the mask
    // next — noted here, queued by the next mapping-stream operation (nothing is launched between two tracking jobs)
    const uint8_t* side = side_planes(t) + (size_t)(t->h_summary->lastCand - 1) * t->maskStride;
    t->maskMergeSeq[t->maskSet] = -1;               // pending
    c->pendingMerges.push_back({frame->d_wasGood, side, &t->maskMergeSeq[t->maskSet]});
  }
  rc = finish_trackframe(t, t->h_summary, kf, frame, out);
  lsdhip_host_mark(7);
  return rc;
}

// ---- batches: n independent jobs in the same launches (job = blockIdx.y) -------------------------------------------
static int batch_reserve(lsdhip_tracker* t, int n) {
  lsdhip_ctx* c = t->ctx;
  LSD_CTX_LOCK(c);
  if (n <= t->batch_capacity) return LSDHIP_OK;
  HIPCHK(hipStreamSynchronize(c->stream));
  // the new set exists before the old one goes: a failed growth leaves the tracker at its old capacity
  const size_t B = n < 8 ? 8 : (size_t)n, floats = scratch_layout(B, LSD_BATCH_SPEC_MAX, (size_t)t->max_blocks).end;
  LsdDev<TrackJob> d_bjobs; LsdDev<TrackState> d_bstate; LsdDev<float> d_bscratch;
  LsdPinned<TrackJob> h_bjobs; LsdPinned<TrackSummary> h_bsummary;
  if (int rc = lsd_dev_alloc(d_bjobs, B)) return rc;
  if (int rc = lsd_dev_alloc(d_bstate, B * 2)) return rc;
  if (int rc = lsd_dev_alloc(d_bscratch, floats)) return rc;
  HIPCHK(hipMemsetAsync(d_bscratch, 0, floats * sizeof(float), c->stream));
  if (int rc = lsd_pinned_alloc(h_bjobs, B, hipHostMallocDefault)) return rc;
  if (int rc = lsd_pinned_alloc(h_bsummary, B, hipHostMallocMapped)) return rc;
  t->d_bjobs = std::move(d_bjobs); t->d_bstate = std::move(d_bstate); t->d_bscratch = std::move(d_bscratch);
  t->h_bjobs = std::move(h_bjobs); t->h_bsummary = std::move(h_bsummary);
  t->batch_capacity = (int)B;
  return LSDHIP_OK;
}
// What every launch of a batch takes besides its shape: the scratch (arrays over [job][parity][trial]; cmax = trial slots per parity, 1: no
// speculation) and the device alias of the pinned summaries.  Built once per batch.
struct BatchLaunch { TrackScratch sc; TrackSummary* d_sum; };
static int batch_launch_record(lsdhip_tracker* t, int cmax, BatchLaunch* out) {
  out->sc = scratch_at(t, t->d_bscratch, (size_t)t->batch_capacity, LSD_BATCH_SPEC_MAX, cmax);
  HIPCHK(hipHostGetDevicePointer((void**)&out->d_sum, t->h_bsummary, 0));
  return LSDHIP_OK;
}
// one k_track_step launch over the n jobs in t->d_bjobs (job = blockIdx.y), `grid` workgroups each
template <int MODE>
static void launch_batch_step(lsdhip_tracker* t, const BatchLaunch& r, int grid, int n, int parity, int first, const TrackSpec& spec) {
  hipLaunchKernelGGL((k_track_step<256, true, MODE>), dim3(grid, n), dim3(256), 0, t->ctx->stream, t->h_bjobs[0], (const TrackJob*)t->d_bjobs, t->d_bstate,
                     r.sc, r.d_sum, parity, first, spec);
}
// the plan (track_plan.hpp) of the batch described in t->h_bjobs[0..n) under the tracker's settings and the developer switches
static BatchPlan plan_batch(const lsdhip_tracker* t, int n) {
  const BatchEnv& env = batch_env();
  BatchPolicy p;
  p.specC = t->specC; p.specMax = env.specMax; p.specPixels = env.specPixels; p.fused = env.fused;
  p.spinWait = t->spinWait; p.poll = env.poll;
  p.soloMin = t->soloMinJobs >= 0 ? t->soloMinJobs : env.soloMin;     // lsdhip_tracker_set_batch_coarse_min_jobs
  return lsd_batch_plan(n, p, [t](int j, int l) {
    const TrackJob& job = t->h_bjobs[j];
    const TrackLevel& L = job.lv[l];
    return BatchLevel{(long long)L.w * L.h, L.nblocks, L.tilePx, L.writeMask, job.lastLevel <= l && l <= job.topLevel};
  });
}
// Runs the n jobs batch_open left in t->d_bjobs to completion; summaries in t->h_bsummary.  record: the rounds it took size the next
// batch's budget and become launch_stats (not for the test hook lsdhip_tracker_evaluate_batch).
// Fused rounds: the host polls the jobs' summaries in pinned memory (as lsdhip_tracker_track does for one job) instead of draining the
// stream: the budget's launches behind the last job's finishing step (~3 us each, a handful per batch) then run while the host is
// already reading the results and queueing what follows.  `done` carries the batch's tag, the record is taken once it adds up to its
// check word; the budget's last launch reports a job it leaves unfinished (`exhausted`).
static int batch_run(lsdhip_tracker* t, int n, bool callHook, bool record) {
  lsdhip_ctx* c = t->ctx;
  LSD_CTX_LOCK(c);
  const BatchEnv& env = batch_env();
  const BatchPlan plan = plan_batch(t, n);
  TrackSpec spec = TrackSpec{};
#ifdef LSD_PHASE_TRACE
  spec.traceWg = env.traceWg;
#endif
  if (plan.speculates) {
    spec.specC = plan.lmGrid;
    for (int l = 0; l < LSD_LEVELS; l++) spec.trials[l] = plan.trials[l];
  }
  BatchLaunch rec;
  if (int rc = batch_launch_record(t, plan.cmax, &rec)) return rc;
  if (int rcp = prof_collect(c)) return rcp;
  if (plan.polled) {
    t->batchTag = t->batchTag >= 0x3FFFFFFF ? 2 : t->batchTag + 1;
    if (t->batchTag < 2) t->batchTag = 2;
    spec.seq = t->batchTag;
    for (int j = 0; j < n; j++) t->h_bsummary[j].exhausted = 0;
  }
  const bool fused = plan.split && env.fused;
  bool soloDue = plan.soloDue;
  int parity = 0, first = 1;
  auto enqueue = [&](int budget) -> int {
    if (soloDue) {
      // the coarse levels of every job inside one workgroup (k_track_solo), then lock-step rounds for the rest
      soloDue = false;
      hipLaunchKernelGGL(k_track_solo<512>, dim3(n), dim3(512), 0, c->stream, (const TrackJob*)t->d_bjobs, t->d_bstate, rec.d_sum, parity, plan.polled ? t->batchTag : 1);
      first = 0;
      parity ^= 1;
    }
    for (int i = 0; i < budget; i++, first = 0, parity ^= 1) {
      spec.last = (plan.polled && i == budget - 1) ? 1 : 0;
      if (fused) {
        launch_batch_step<TS_FUSED>(t, rec, plan.grid, n, parity, first, spec);
      } else if (plan.split) {
        // LSDHIP_BATCH_FUSED=0: one LM workgroup per (trial, job), then a pure evaluation launch over all jobs' (trial, strip) pairs
        launch_batch_step<TS_LM>(t, rec, plan.lmGrid, n, parity, first, spec);
        launch_batch_step<TS_EVAL>(t, rec, plan.grid, n, 1 - parity, 0, spec);
      } else {
        launch_batch_step<TS_FUSED>(t, rec, plan.grid, n, parity, first, TrackSpec{});
      }
    }
    HIPCHK(hipGetLastError());
    return LSDHIP_OK;
  };
  auto wait = [&](int, bool* finished) -> int {
    bool all = true;
    if (plan.polled) {
      const int tag = t->batchTag;
      const LsdDeadline deadline = lsd_deadline(LSD_BATCH_WAIT_S);
      for (int j = 0; j < n && all; j++) {
        volatile const int* done = &t->h_bsummary[j].done;
        volatile const int* exhausted = &t->h_bsummary[j].exhausted;
        if (int rc = lsd_spin_until(c, [=]() { return *done == tag || *exhausted == tag; }, deadline, LSD_WAIT_BATCH)) return rc;
        all = *done == tag;
        if (all) { if (int rcs = summary_wait_consistent(t, tag, &t->h_bsummary[j])) return rcs; }
      }
      if (!all) {
        HIPCHK(hipStreamSynchronize(c->stream));   // out of budget: rare
        all = true;
        for (int j = 0; j < n; j++) { all = all && t->h_bsummary[j].done == tag; t->h_bsummary[j].exhausted = 0; }
      }
    } else {
      HIPCHK(hipStreamSynchronize(c->stream));
      for (int j = 0; j < n; j++) all = all && t->h_bsummary[j].done;
    }
    *finished = all;
    return LSDHIP_OK;
  };
  // budget of rounds: what the recent batches needed (+ the finishing step and a margin); launches behind the last job's finishing step
  // cost ~3 us each
  const int budget = plan.split ? t->batchRecent.budget(26, env.margin, 0) : 26;
  if (int rc = run_budgets(t, c->prof_on, callHook, budget, "tracking batch", enqueue, wait, [](int) { return 6; })) return rc;
  if (c->prof_on)
    for (int j = 0; j < n; j++) { c->prof_bytes += t->h_bsummary[j].bytes; c->prof_launches += t->h_bsummary[j].numEvaluations; }
  if (plan.split && record) {
    int rounds = 0;
    for (int j = 0; j < n; j++) if (t->h_bsummary[j].numLaunches > rounds) rounds = t->h_bsummary[j].numLaunches;
    t->batchRecent.note(rounds);
    t->numLaunches = rounds;
  }
  return LSDHIP_OK;
}

// The shared prologue of the batch entries.  The pairs are complete (a missing frame: LSDHIP_E_ARG; a keyframe without depth:
// LSDHIP_E_STATE), the reference blocks that the strips of throughput mode read exist, the tracker's batch buffers hold n jobs, and
// fill(j, job, shape) -> rc has described job j for the batch's shape; the descriptions are on their way to t->d_bjobs and no summary
// says `done`.  keyframes: nullptr for jobs on point lists.  inputsOnly (lsdhip_tracker_track_batch; the other entries enter behind
// everything the mapping stream holds, LsdTrackJobScope): on a pipelined context the tracking stream waits for the mapping-stream points
// the jobs' inputs were complete at (the frames' pyramids, the keyframes' PUBLISHED depth) and for nothing queued behind them.
struct BatchOpened { int rc; BatchShape shape; };
template <class Fill>
static BatchOpened batch_open(lsdhip_tracker* t, const char* entry, int n, lsdhip_frame** keyframes, lsdhip_frame** frames, bool inputsOnly, Fill fill) {
  lsdhip_ctx* c = t->ctx;
  LSD_CTX_LOCK(c);
  BatchOpened o = {LSDHIP_OK, lsd_batch_shape(t->grid_cap, n)};
  o.rc = [&]() -> int {
    long long need = 0;
    for (int j = 0; j < n; j++) {
      if ((keyframes && !keyframes[j]) || !frames[j]) return LSDHIP_E_ARG;
      if (keyframes && !keyframes[j]->hasIDepth) { lsd_set_error("%s: keyframe %d (job %d) has no depth", entry, keyframes[j]->id, j); return LSDHIP_E_STATE; }
      need = std::max(need, frames[j]->readySeq);
      if (keyframes) need = std::max(need, std::max(keyframes[j]->readySeq, keyframes[j]->depthSeq));
    }
    if (c->pipeline && inputsOnly) { if (int rcw = lsd_t_wait_m(c, need)) return rcw; }
    if (keyframes && n >= LSD_BATCH_THROUGHPUT_MIN_JOBS) { if (int rcb = lsd_frames_require_ref_blocks(keyframes, n, c->stream)) return rcb; }   // the strips read them
    if (int rc = batch_reserve(t, n)) return rc;
    for (int j = 0; j < n; j++) {
      if (int rc = fill(j, t->h_bjobs[j], o.shape)) return rc;
      t->h_bsummary[j].done = 0;
    }
    HIPCHK(hipMemcpyAsync(t->d_bjobs, t->h_bjobs, (size_t)n * sizeof(TrackJob), hipMemcpyHostToDevice, c->stream));
    return LSDHIP_OK;
  }();
  return o;
}
extern "C" void lsdhip_build_defaults(lsdhip_build_defaults_t* out) {
  if (!out) return;
  out->ctx_async = LSD_DEFAULT_ASYNC; out->ctx_pipeline = LSD_DEFAULT_PIPELINE;
  out->spec_trials_small = LSD_SPEC_TRIALS_SMALL; out->spec_small_pixels = LSD_SPEC_SMALL_PX;
  out->spec_trials_mid = LSD_SPEC_TRIALS_MID; out->spec_mid_pixels = LSD_SPEC_MID_PX;
  out->spec_workgroups = LSD_SPEC_CAP_WORKGROUPS; out->spec_workgroups_above_pixels = LSD_SPEC_CAP_ABOVE_PX;
  out->spec_trials_max = LSD_SPEC_MAX;
  out->batch_throughput_min_jobs = LSD_BATCH_THROUGHPUT_MIN_JOBS; out->batch_strip_workgroups = LSD_BATCH_STRIP_WORKGROUPS;
  out->batch_coarse_min_jobs = LSD_SOLO_MIN_JOBS; out->batch_coarse_max_pixels = LSD_SOLO_MAX_PX; out->batch_coarse_max_points = LSD_SOLO_LDS_PTS;
}

// SE3Tracker::trackFrame for n independent (keyframe, frame) pairs in the same launches.  Each job runs the arithmetic
// of lsdhip_tracker_track (same kernel; a batch tiles a level into fewer workgroups, which only changes summation
// order); the point is throughput — n evaluations share one launch and its latency chain.  inits: n x 7, results: n.
// Returns LSDHIP_OK, or LSDHIP_DIVERGED if any job diverged (see results[j].diverged).
extern "C" int lsdhip_tracker_track_batch(lsdhip_tracker* t, int n, lsdhip_frame** keyframes, lsdhip_frame** frames,
                                          const double* inits, lsdhip_track_result* results) {
  if (!t || n <= 0 || !keyframes || !frames || !inits || !results) return LSDHIP_E_ARG;
  lsdhip_ctx* c = t->ctx;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  // (pipelined contexts, as lsdhip_tracker_track: mapping iterations of OTHER sequences run beside this batch — SlamLoopBatch::setOverlapped.
  // When batch_run returns only the summaries are complete: the launches of its budget behind the last job's finishing step may still be
  // queued on the tracking stream; they leave at once, see track_step_impl.)
  const BatchOpened o = batch_open(t, "lsdhip_tracker_track_batch", n, keyframes, frames, true, [&](int j, TrackJob& job, BatchShape shape) {
    if (int rcf = fill_trackframe_job(t, job, shape, keyframes[j], frames[j])) return rcf;
    job.evalOnly = 0;
    job.topLevel = LSD_TRACK_MAX_LEVEL - 1;
    job.T0 = lsdm::se3f_from_d(lsdm::se3d_inverse(lsdm::se3d_from7(inits + 7 * (size_t)j)));
    job.aff_a0 = 1.0f; job.aff_b0 = 0.0f;
    return (int)LSDHIP_OK;
  });
  if (o.rc) return o.rc;
  int rc = batch_run(t, n, true, true);
  if (rc) return rc;
  int rcAll = LSDHIP_OK;
  for (int j = 0; j < n; j++) {
    rc = finish_trackframe(t, &t->h_bsummary[j], keyframes[j], frames[j], &results[j]);
    if (rc == LSDHIP_DIVERGED) rcAll = LSDHIP_DIVERGED;
    else if (rc) return rc;
  }
  return rcAll;
}

// Measurement hook (profiles/r03_sizes.md, bench.py's roofline_throughput_mode): the throughput-mode evaluation launch alone.
// n jobs (keyframes[j], frames[j]) are evaluated at pyramid level `level` at the poses refToFrame[j] (7 floats each: q w x y z, t):
// one LM launch builds the states, then `repeats` identical evaluation launches (k_track_step<.., TS_EVAL>: idempotent — it reads
// the published state and rewrites the same partial rows) are timed with one HIP event pair, and a closing LM launch finalises the
// sums so that the algorithmic bytes of ONE evaluation launch (sum over the jobs, SURVEY.md 8(d) formula as counted by lm_wave)
// can be reported.  Needs n >= 8 (throughput mode).
extern "C" int lsdhip_tracker_eval_throughput(lsdhip_tracker* t, int n, lsdhip_frame** keyframes, lsdhip_frame** frames, const float* refToFrame,
                                              int level, int repeats, double* ms_per_launch, double* bytes_per_launch) {
  if (!t || n < 8 || !keyframes || !frames || !refToFrame || level < 0 || level >= LSD_LEVELS || repeats < 1 || !ms_per_launch || !bytes_per_launch)
    return LSDHIP_E_ARG;
  lsdhip_ctx* c = t->ctx;
  LSD_CTX_LOCK(c);
  LsdTrackJobScope tjob_(c, true);
  if (tjob_.rc) return tjob_.rc;
  HIPCHK(hipSetDevice(c->device));
  for (int j = 0; j < n; j++) if (!keyframes[j] || !frames[j] || !keyframes[j]->hasIDepth) return LSDHIP_E_ARG;
  int grid = 1;
  const BatchOpened o = batch_open(t, "lsdhip_tracker_eval_throughput", n, keyframes, frames, false, [&](int j, TrackJob& job, BatchShape shape) {
    if (int rcf = fill_eval_job(t, job, shape, keyframes[j], frames[j], level, refToFrame + 7 * (size_t)j, 1.0f, 0.0f)) return rcf;
    if (job.lv[level].nblocks > grid) grid = job.lv[level].nblocks;
    if (job.lv[level].tilePx == 0) { lsd_set_error("lsdhip_tracker_eval_throughput: level %d is not in throughput mode", level); return (int)LSDHIP_E_STATE; }
    return (int)LSDHIP_OK;
  });
  if (o.rc) return o.rc;
  BatchLaunch rec;
  if (int rcl = batch_launch_record(t, 1, &rec)) return rcl;
  LsdEvent e0, e1;
  if (int rce = lsd_event_create(e0)) return rce;
  if (int rce = lsd_event_create(e1)) return rce;
  launch_batch_step<TS_LM>(t, rec, 1, n, 0, 1, TrackSpec{});
  launch_batch_step<TS_EVAL>(t, rec, grid, n, 1, 0, TrackSpec{});     // warm-up
  HIPCHK(hipEventRecord(e0, c->stream));
  for (int r = 0; r < repeats; r++) launch_batch_step<TS_EVAL>(t, rec, grid, n, 1, 0, TrackSpec{});
  HIPCHK(hipEventRecord(e1, c->stream));
  launch_batch_step<TS_LM>(t, rec, 1, n, 1, 0, TrackSpec{});
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  double bytes = 0;
  for (int j = 0; j < n; j++) {
    if (!t->h_bsummary[j].done) { lsd_set_error("lsdhip_tracker_eval_throughput: job %d did not finish", j); return LSDHIP_E_STATE; }
    bytes += t->h_bsummary[j].bytes;
  }
  *ms_per_launch = ms / repeats;
  *bytes_per_launch = bytes;
  return LSDHIP_OK;
}

extern "C" int lsdhip_tracker_evaluate(lsdhip_tracker* t, lsdhip_frame* kf, lsdhip_frame* frame, const float T7[7], int level,
                                       float aff_a, float aff_b, lsdhip_residual_record* out) {
  if (!t || !kf || !frame || !T7 || !out || level < 0 || level >= LSD_LEVELS) return LSDHIP_E_ARG;
  if (!kf->hasIDepth) { lsd_set_error("lsdhip_tracker_evaluate: keyframe has no depth"); return LSDHIP_E_STATE; }
  HIPCHK(hipSetDevice(t->ctx->device));
  LSD_CTX_LOCK(t->ctx);
  LsdTrackJobScope tjob_(t->ctx, true);
  if (tjob_.rc) return tjob_.rc;
  t->affineEstimation_a = aff_a; t->affineEstimation_b = aff_b;   // (evaluate_pose evaluates at the tracker's pair)
  TrackJob job;
  int rc = fill_eval_job(t, job, BatchShape{}, kf, frame, level, T7, aff_a, aff_b);
  if (rc) return rc;
  EvalOut ev;
  rc = evaluate_pose(t, job, job.T0, level, &ev);
  if (rc) return rc;
  record_of(t->h_summary, out);
  return LSDHIP_OK;
}

// Test hook: one evaluation per job through the launches of a batch (batch_run: the small-batch form, throughput-mode strips, k_track_solo
// on the levels it takes), each job an evalOnly job at its own pose and affine pair.  The tracker's LM state, its counters and the
// round budget of later batches are left as they were.
extern "C" int lsdhip_tracker_evaluate_batch(lsdhip_tracker* t, int n, lsdhip_frame** keyframes, lsdhip_frame** frames, const float* refToFrame,
                                             const float* affine, int level, lsdhip_residual_record* out, int* form) {
  if (!t || n <= 0 || !keyframes || !frames || !refToFrame || !affine || !out) return LSDHIP_E_ARG;
  if (level < LSD_TRACK_MIN_LEVEL || level >= LSD_TRACK_MAX_LEVEL) {
    lsd_set_error("lsdhip_tracker_evaluate_batch: level %d is not a tracking level (%d..%d)", level, LSD_TRACK_MIN_LEVEL, LSD_TRACK_MAX_LEVEL - 1);
    return LSDHIP_E_ARG;
  }
  lsdhip_ctx* c = t->ctx;
  LSD_CTX_LOCK(c);
  LsdTrackJobScope tjob_(c, true);
  if (tjob_.rc) return tjob_.rc;
  HIPCHK(hipSetDevice(c->device));
  const BatchOpened o = batch_open(t, "lsdhip_tracker_evaluate_batch", n, keyframes, frames, false, [&](int j, TrackJob& job, BatchShape shape) {
    return fill_eval_job(t, job, shape, keyframes[j], frames[j], level, refToFrame + 7 * (size_t)j, affine[2 * (size_t)j], affine[2 * (size_t)j + 1]);
  });
  if (o.rc) return o.rc;
  if (int rc = batch_run(t, n, false, false)) return rc;
  for (int j = 0; j < n; j++) {
    const TrackSummary* S = &t->h_bsummary[j];
    if (!S->done) { lsd_set_error("lsdhip_tracker_evaluate_batch: job %d did not finish", j); return LSDHIP_E_STATE; }
    record_of(S, &out[j]);
    if (form) {
      form[2 * j] = S->numLaunches == 0 ? 1 : 0;   // k_track_solo evaluates without a k_track_step launch (which counts S.numLaunches)
      form[2 * j + 1] = t->h_bjobs[j].lv[level].tilePx;
    }
  }
  return LSDHIP_OK;
}

static int upload_points(lsdhip_tracker* t, const float* pos, const float* colvar, int n) {
  if (n > t->pts_capacity) {
    const int cap = n > 4096 ? n : 4096;
    if (int rc = lsd_dev_alloc(t->d_pts, (size_t)cap * 5)) return rc;
    t->pts_capacity = cap;
  }
  HIPCHK(hipMemcpyAsync(t->d_pts, pos, (size_t)n * 12, hipMemcpyHostToDevice, t->ctx->stream));
  if (colvar) HIPCHK(hipMemcpyAsync(t->d_pts + (size_t)t->pts_capacity * 3, colvar, (size_t)n * 8, hipMemcpyHostToDevice, t->ctx->stream));
  return LSDHIP_OK;
}

// trackFrameOnPermaref as a single job (the launch-per-step chain with its speculation and the polled summary) on a cloud that is
// already on the device: the upload of lsdhip_tracker_track_permaref, or a slot of a keyframe bank
static int permaref_single_run(lsdhip_tracker* t, const float* d_pos, const float* d_colvar, int n, lsdhip_frame* frame, const double refToFrame[7],
                               lsdhip_track_result* out) {
  lsdm::SE3fH referenceToFrame = lsdm::se3f_from_d(lsdm::se3d_from7(refToFrame));
  t->affineEstimation_a = 1; t->affineEstimation_b = 0;
  t->diverged = false; t->trackingWasGood = true;
  t->numEvaluations = 0; t->numWarpUpdates = 0;
  const int L = LSD_QUICK_KF_CHECK_LVL;
  TrackJob job;
  int rc = fill_permaref_job(t, job, BatchShape{}, d_pos, d_colvar, n, frame, referenceToFrame);
  if (rc) return rc;
  if (t->hostLM) {
    float lastErr = 0;
    rc = lm_level_host(t, job, L, referenceToFrame, &lastErr);
    t->lastResidual = lastErr;
  } else {
    rc = track_device(t, job, L, referenceToFrame, &referenceToFrame);
  }
  if (rc != LSDHIP_OK && rc != LSDHIP_DIVERGED) return rc;
  return finish_permaref(t, rc == LSDHIP_DIVERGED, referenceToFrame, out);
}

extern "C" int lsdhip_tracker_track_permaref(lsdhip_tracker* t, const float* pos, const float* colvar, int n, lsdhip_frame* frame,
                                             const double refToFrame[7], lsdhip_track_result* out) {
  if (!t || !pos || !colvar || n <= 0 || !frame || !refToFrame || !out) return LSDHIP_E_ARG;
  lsdhip_ctx* c = t->ctx;
  LSD_CTX_LOCK(c);
  LsdTrackJobScope tjob_(c, true);
  if (tjob_.rc) return tjob_.rc;
  HIPCHK(hipSetDevice(c->device));
  int rc = upload_points(t, pos, colvar, n);
  if (rc) return rc;
  return permaref_single_run(t, t->d_pts, t->d_pts + (size_t)t->pts_capacity * 3, n, frame, refToFrame, out);
}

// SE3Tracker::trackFrameOnPermaref (SE3Tracker.cpp:162-272) for n permanent references against frames[j] in the same
// launches — the shape of TrackableKeyFrameSearch::findRePositionCandidate and of the relocaliser, which test many
// keyframes against one new frame.  pos / colvar: the references' level-4 point clouds
// concatenated (counts[j] points each); refToFrame: n x 7; results: n.
extern "C" int lsdhip_tracker_track_permaref_batch(lsdhip_tracker* t, int n, const float* pos, const float* colvar, const int* counts,
                                                   lsdhip_frame** frames, const double* refToFrame, lsdhip_track_result* results) {
  if (!t || n <= 0 || !pos || !colvar || !counts || !frames || !refToFrame || !results) return LSDHIP_E_ARG;
  lsdhip_ctx* c = t->ctx;
  LSD_CTX_LOCK(c);
  LsdTrackJobScope tjob_(c, true);
  if (tjob_.rc) return tjob_.rc;
  HIPCHK(hipSetDevice(c->device));
  int total = 0;
  for (int j = 0; j < n; j++) { if (counts[j] <= 0 || !frames[j]) return LSDHIP_E_ARG; total += counts[j]; }
  int rc = upload_points(t, pos, colvar, total);
  if (rc) return rc;
  int off = 0;
  const BatchOpened o = batch_open(t, "lsdhip_tracker_track_permaref_batch", n, nullptr, frames, false, [&](int j, TrackJob& job, BatchShape shape) {
    const int at = off;
    off += counts[j];
    return fill_permaref_job(t, job, shape, t->d_pts + (size_t)at * 3, t->d_pts + (size_t)t->pts_capacity * 3 + (size_t)at * 2, counts[j], frames[j],
                             lsdm::se3f_from_d(lsdm::se3d_from7(refToFrame + 7 * (size_t)j)));
  });
  if (o.rc) return o.rc;
  rc = batch_run(t, n, false, true);
  if (rc) return rc;
  int rcAll = LSDHIP_OK;
  for (int j = 0; j < n; j++) {
    const TrackSummary* S = &t->h_bsummary[j];
    take_summary(t, S);   // (with the affine pair of the last iteration, which only the host-LM loop reads, behind an evaluation of its own)
    if (finish_permaref(t, S->diverged != 0, pose_of(S), &results[j]) == LSDHIP_DIVERGED) rcAll = LSDHIP_DIVERGED;
  }
  return rcAll;
}

extern "C" int lsdhip_tracker_check_overlap(lsdhip_tracker* t, const float* pos, int n, const double refToFrame[7], float* usage_out) {
  if (!t || !pos || n <= 0 || !refToFrame || !usage_out) return LSDHIP_E_ARG;
  lsdhip_ctx* c = t->ctx;
  LSD_CTX_LOCK(c);
  LsdTrackJobScope tjob_(c, true);
  if (tjob_.rc) return tjob_.rc;
  HIPCHK(hipSetDevice(c->device));
  int rc = upload_points(t, pos, nullptr, n);
  if (rc) return rc;
  lsdm::SE3fH T = lsdm::se3f_from_d(lsdm::se3d_from7(refToFrame));
  const int L = LSD_QUICK_KF_CHECK_LVL;
  EvalCtx a;
  memset(&a, 0, sizeof(a));
  const LevelIntr& in = c->intr[L];
  a.w = c->wl[L]; a.h = c->hl[L];
  a.fx = in.fx; a.fy = in.fy; a.cx = in.cx; a.cy = in.cy;
  lsdm::quatf_to_rot(T.q, a.R);
  a.t[0] = T.t[0]; a.t[1] = T.t[1]; a.t[2] = T.t[2];
  hipLaunchKernelGGL(k_overlap, dim3(1), dim3(256), 0, c->stream, t->d_pts, n, a, t->d_summary->sums);
  HIPCHK(hipStreamSynchronize(c->stream));
  t->pointUsage = t->h_summary->sums[0] / (float)n;
  *usage_out = t->pointUsage;
  return LSDHIP_OK;
}

// ---- the keyframe bank (kfbank.hip): checkPermaRefOverlap / trackFrameOnPermaref over clouds that stay on the device ------------------
static int bank_slots_ok(const char* entry, const lsdhip_tracker* t, const lsdhip_kfbank* b, int n, const int* slots) {
  if (b->ctx != t->ctx) { lsd_set_error("%s: the bank belongs to another context", entry); return LSDHIP_E_ARG; }
  for (int j = 0; j < n; j++) {
    if (slots[j] < 0 || slots[j] >= (int)b->slots.size()) { lsd_set_error("%s: pair %d: slot %d is not in use", entry, j, slots[j]); return LSDHIP_E_ARG; }
    if (b->slots[(size_t)slots[j]].numPoints <= 0) { lsd_set_error("%s: pair %d: slot %d holds no point", entry, j, slots[j]); return LSDHIP_E_ARG; }
  }
  return LSDHIP_OK;
}
// one launch and one wait for n (slot, pose) pairs; the pairs' records go up in one copy (the context's argument ring).  The caller holds the context lock and a LsdTrackJobScope.
static int overlap_bank_run(lsdhip_tracker* t, lsdhip_kfbank* b, int n, const int* slots, const double* refToFrame, float* usage_out) {
  lsdhip_ctx* c = t->ctx;
  const int L = LSD_QUICK_KF_CHECK_LVL;
  // the sums land in pinned host memory the kernel writes through its device alias (as k_overlap writes the tracker's summary): no copy
  if (n > t->overlapSumsCapacity) {
    HIPCHK(hipStreamSynchronize(c->stream));
    const int cap = n < 256 ? 256 : n * 2;
    if (int rc = lsd_pinned_alloc(t->h_overlapSums, (size_t)cap, hipHostMallocMapped)) return rc;
    t->overlapSumsCapacity = cap;
  }
  float* d_out = nullptr;
  HIPCHK(hipHostGetDevicePointer((void**)&d_out, t->h_overlapSums, 0));
  void* host = nullptr;
  void* dev = nullptr;
  if (int rc = lsd_args_begin(c, sizeof(OverlapJob) * (size_t)n, &host, &dev)) return rc;
  OverlapJob* jobs = (OverlapJob*)host;
  for (int j = 0; j < n; j++) {
    const lsdm::SE3fH T = lsdm::se3f_from_d(lsdm::se3d_from7(refToFrame + 7 * (size_t)j));
    OverlapJob& J = jobs[j];
    J.pos = lsd_g((const float*)b->pos(slots[j]));
    J.n = b->slots[(size_t)slots[j]].numPoints;
    lsdm::quatf_to_rot(T.q, J.R);
    J.t[0] = T.t[0]; J.t[1] = T.t[1]; J.t[2] = T.t[2];
  }
  if (int rc = lsd_args_commit(c, c->stream)) return rc;
  const LevelIntr& in = c->intr[L];
  hipLaunchKernelGGL(k_overlap_bank, dim3(n), dim3(256), 0, c->stream, (const OverlapJob*)dev, in.fx, in.fy, in.cx, in.cy, c->wl[L], c->hl[L], d_out);
  HIPCHK(hipGetLastError());
  if (int rc = lsd_args_release(c, dev, c->stream)) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int j = 0; j < n; j++) usage_out[j] = t->h_overlapSums[j] / (float)b->slots[(size_t)slots[j]].numPoints;
  t->pointUsage = usage_out[n - 1];
  return LSDHIP_OK;
}
// lsdhip_tracker_track_permaref_batch with the jobs' point pointers aimed into the bank: nothing but the job records is uploaded
static int permaref_bank_run(lsdhip_tracker* t, lsdhip_kfbank* b, int n, const int* slots, lsdhip_frame** frames, const double* refToFrame,
                             lsdhip_track_result* results) {
  // one candidate has the chip to itself: the single job's chain (speculation, polled summary) is the shorter way to the same result
  if (n == 1) return permaref_single_run(t, b->pos(slots[0]), b->colvar(slots[0]), b->slots[(size_t)slots[0]].numPoints, frames[0], refToFrame, &results[0]);
  const BatchOpened o = batch_open(t, "lsdhip_tracker_track_permaref_bank", n, nullptr, frames, false, [&](int j, TrackJob& job, BatchShape shape) {
    return fill_permaref_job(t, job, shape, b->pos(slots[j]), b->colvar(slots[j]), b->slots[(size_t)slots[j]].numPoints, frames[j],
                             lsdm::se3f_from_d(lsdm::se3d_from7(refToFrame + 7 * (size_t)j)));
  });
  if (o.rc) return o.rc;
  if (int rc = batch_run(t, n, false, true)) return rc;
  int rcAll = LSDHIP_OK;
  for (int j = 0; j < n; j++) {
    const TrackSummary* S = &t->h_bsummary[j];
    take_summary(t, S);
    if (finish_permaref(t, S->diverged != 0, pose_of(S), &results[j]) == LSDHIP_DIVERGED) rcAll = LSDHIP_DIVERGED;
  }
  return rcAll;
}

extern "C" int lsdhip_tracker_check_overlap_bank(lsdhip_tracker* t, lsdhip_kfbank* b, int n, const int* slots, const double* refToFrame, float* usage_out) {
  if (!t || !b || n <= 0 || !slots || !refToFrame || !usage_out) return LSDHIP_E_ARG;
  lsdhip_ctx* c = t->ctx;
  LSD_CTX_LOCK(c);
  if (int rc = bank_slots_ok("lsdhip_tracker_check_overlap_bank", t, b, n, slots)) return rc;
  LsdTrackJobScope tjob_(c, true);
  if (tjob_.rc) return tjob_.rc;
  HIPCHK(hipSetDevice(c->device));
  return overlap_bank_run(t, b, n, slots, refToFrame, usage_out);
}

extern "C" int lsdhip_tracker_track_permaref_bank(lsdhip_tracker* t, lsdhip_kfbank* b, int n, const int* slots, lsdhip_frame** frames,
                                                  const double* refToFrame, lsdhip_track_result* results) {
  if (!t || !b || n <= 0 || !slots || !frames || !refToFrame || !results) return LSDHIP_E_ARG;
  lsdhip_ctx* c = t->ctx;
  LSD_CTX_LOCK(c);
  if (int rc = bank_slots_ok("lsdhip_tracker_track_permaref_bank", t, b, n, slots)) return rc;
  for (int j = 0; j < n; j++) if (!frames[j] || frames[j]->ctx != c) return LSDHIP_E_ARG;
  LsdTrackJobScope tjob_(c, true);
  if (tjob_.rc) return tjob_.rc;
  HIPCHK(hipSetDevice(c->device));
  return permaref_bank_run(t, b, n, slots, frames, refToFrame, results);
}

// ---- test hooks: one evaluation per explicit point list, in the launches the trackFrameOnPermaref entries run ---------------------------
// The permaref job of the list (fill_permaref_job: the level's description, its tiling for the batch's shape), evalOnly at the given pose
// and affine pair.
static int fill_points_eval_job(lsdhip_tracker* t, TrackJob& job, BatchShape shape, const float* d_pos, const float* d_colvar, int npts,
                                lsdhip_frame* frame, const float T7[7], float aff_a, float aff_b) {
  if (int rc = fill_permaref_job(t, job, shape, d_pos, d_colvar, npts, frame, pose_from7(T7))) return rc;
  job.evalOnly = 1;
  job.aff_a0 = aff_a; job.aff_b0 = aff_b;
  return LSDHIP_OK;
}
// the tracker's public members an evaluation with a host round trip writes (evaluate_pose): the hooks put them back
struct EvalMembers {
  int numEvaluations;
  float pointUsage, lastGoodCount, lastBadCount, lastMeanRes, aff_a, aff_b, aff_a_lastIt, aff_b_lastIt;
  explicit EvalMembers(const lsdhip_tracker* t)
      : numEvaluations(t->numEvaluations), pointUsage(t->pointUsage), lastGoodCount(t->lastGoodCount), lastBadCount(t->lastBadCount),
        lastMeanRes(t->lastMeanRes), aff_a(t->affineEstimation_a), aff_b(t->affineEstimation_b), aff_a_lastIt(t->affineEstimation_a_lastIt),
        aff_b_lastIt(t->affineEstimation_b_lastIt) {}
  void restore(lsdhip_tracker* t) const {
    t->numEvaluations = numEvaluations;
    t->pointUsage = pointUsage; t->lastGoodCount = lastGoodCount; t->lastBadCount = lastBadCount; t->lastMeanRes = lastMeanRes;
    t->affineEstimation_a = aff_a; t->affineEstimation_b = aff_b;
    t->affineEstimation_a_lastIt = aff_a_lastIt; t->affineEstimation_b_lastIt = aff_b_lastIt;
  }
};
static void tiles_of(const TrackJob& job, int* tiles) {
  if (!tiles) return;
  tiles[0] = job.lv[LSD_QUICK_KF_CHECK_LVL].nblocks;
  tiles[1] = job.lv[LSD_QUICK_KF_CHECK_LVL].singlePass;
}
// the single job's evaluation (evaluate_pose) of a list that is already on the device
static int points_eval_single(lsdhip_tracker* t, const float* d_pos, const float* d_colvar, int n, lsdhip_frame* frame, const float T7[7],
                              float aff_a, float aff_b, lsdhip_residual_record* out, int* tiles) {
  const EvalMembers keep(t);
  t->affineEstimation_a = aff_a; t->affineEstimation_b = aff_b;   // (evaluate_pose evaluates at the tracker's pair)
  TrackJob job;
  int rc = fill_points_eval_job(t, job, BatchShape{}, d_pos, d_colvar, n, frame, T7, aff_a, aff_b);
  EvalOut ev;
  if (!rc) rc = evaluate_pose(t, job, job.T0, LSD_QUICK_KF_CHECK_LVL, &ev);
  if (!rc) { record_of(t->h_summary, out); tiles_of(job, tiles); }
  keep.restore(t);
  return rc;
}
// the records of a finished batch of evalOnly jobs
static int points_eval_collect(lsdhip_tracker* t, const char* entry, int n, lsdhip_residual_record* out, int* tiles) {
  for (int j = 0; j < n; j++) {
    const TrackSummary* S = &t->h_bsummary[j];
    if (!S->done) { lsd_set_error("%s: job %d did not finish", entry, j); return LSDHIP_E_STATE; }
    record_of(S, &out[j]);
    tiles_of(t->h_bjobs[j], tiles ? tiles + 2 * (size_t)j : nullptr);
  }
  return LSDHIP_OK;
}

extern "C" int lsdhip_tracker_evaluate_points(lsdhip_tracker* t, const float* pos, const float* colvar, int n, lsdhip_frame* frame,
                                              const float T7[7], float aff_a, float aff_b, lsdhip_residual_record* out, int* tiles) {
  if (!t || !pos || !colvar || n <= 0 || !frame || !T7 || !out) return LSDHIP_E_ARG;
  lsdhip_ctx* c = t->ctx;
  LSD_CTX_LOCK(c);
  LsdTrackJobScope tjob_(c, true);
  if (tjob_.rc) return tjob_.rc;
  HIPCHK(hipSetDevice(c->device));
  if (int rc = upload_points(t, pos, colvar, n)) return rc;
  return points_eval_single(t, t->d_pts, t->d_pts + (size_t)t->pts_capacity * 3, n, frame, T7, aff_a, aff_b, out, tiles);
}

extern "C" int lsdhip_tracker_evaluate_points_batch(lsdhip_tracker* t, int n, const float* pos, const float* colvar, const int* counts,
                                                    lsdhip_frame** frames, const float* refToFrame, const float* affine,
                                                    lsdhip_residual_record* out, int* tiles) {
  if (!t || n <= 0 || !pos || !colvar || !counts || !frames || !refToFrame || !affine || !out) return LSDHIP_E_ARG;
  lsdhip_ctx* c = t->ctx;
  LSD_CTX_LOCK(c);
  LsdTrackJobScope tjob_(c, true);
  if (tjob_.rc) return tjob_.rc;
  HIPCHK(hipSetDevice(c->device));
  int total = 0;
  for (int j = 0; j < n; j++) { if (counts[j] <= 0 || !frames[j]) return LSDHIP_E_ARG; total += counts[j]; }
  if (int rc = upload_points(t, pos, colvar, total)) return rc;
  int off = 0;
  const BatchOpened o = batch_open(t, "lsdhip_tracker_evaluate_points_batch", n, nullptr, frames, false, [&](int j, TrackJob& job, BatchShape shape) {
    const int at = off;
    off += counts[j];
    return fill_points_eval_job(t, job, shape, t->d_pts + (size_t)at * 3, t->d_pts + (size_t)t->pts_capacity * 3 + (size_t)at * 2, counts[j], frames[j],
                                refToFrame + 7 * (size_t)j, affine[2 * (size_t)j], affine[2 * (size_t)j + 1]);
  });
  if (o.rc) return o.rc;
  if (int rc = batch_run(t, n, false, false)) return rc;
  return points_eval_collect(t, "lsdhip_tracker_evaluate_points_batch", n, out, tiles);
}

extern "C" int lsdhip_tracker_evaluate_points_bank(lsdhip_tracker* t, lsdhip_kfbank* b, int n, const int* slots, lsdhip_frame** frames,
                                                   const float* refToFrame, const float* affine, lsdhip_residual_record* out, int* tiles) {
  if (!t || !b || n <= 0 || !slots || !frames || !refToFrame || !affine || !out) return LSDHIP_E_ARG;
  lsdhip_ctx* c = t->ctx;
  LSD_CTX_LOCK(c);
  if (int rc = bank_slots_ok("lsdhip_tracker_evaluate_points_bank", t, b, n, slots)) return rc;
  for (int j = 0; j < n; j++) if (!frames[j] || frames[j]->ctx != c) return LSDHIP_E_ARG;
  LsdTrackJobScope tjob_(c, true);
  if (tjob_.rc) return tjob_.rc;
  HIPCHK(hipSetDevice(c->device));
  // (one candidate: the single job's chain, as permaref_bank_run)
  if (n == 1)
    return points_eval_single(t, b->pos(slots[0]), b->colvar(slots[0]), b->slots[(size_t)slots[0]].numPoints, frames[0], refToFrame, affine[0], affine[1],
                              out, tiles);
  const BatchOpened o = batch_open(t, "lsdhip_tracker_evaluate_points_bank", n, nullptr, frames, false, [&](int j, TrackJob& job, BatchShape shape) {
    return fill_points_eval_job(t, job, shape, b->pos(slots[j]), b->colvar(slots[j]), b->slots[(size_t)slots[j]].numPoints, frames[j],
                                refToFrame + 7 * (size_t)j, affine[2 * (size_t)j], affine[2 * (size_t)j + 1]);
  });
  if (o.rc) return o.rc;
  if (int rc = batch_run(t, n, false, false)) return rc;
  return points_eval_collect(t, "lsdhip_tracker_evaluate_points_bank", n, out, tiles);
}

// TrackableKeyFrameSearch::findRePositionCandidate (TrackableKeyFrameSearch.cpp:103-172): the host stages are reposition_plan.hpp's, the
// two launches stand between them.  Two host waits per search: the score of stage 3's usages decides which tracking jobs exist.
extern "C" int lsdhip_tracker_find_reposition_candidate(lsdhip_tracker* t, lsdhip_kfbank* b, lsdhip_frame* frame, const double frameCamToWorld[8],
                                                        int trackingParentId, float maxScore, lsdhip_reposition_result* res) {
  if (!t || !b || !frame || !frameCamToWorld || !res || b->ctx != t->ctx || frame->ctx != t->ctx) return LSDHIP_E_ARG;
  lsdhip_ctx* c = t->ctx;
  LSD_CTX_LOCK(c);
  LsdTrackJobScope tjob_(c, true);
  if (tjob_.rc) return tjob_.rc;
  HIPCHK(hipSetDevice(c->device));
  std::vector<lsdrp::Keyframe> kfs(b->slots.size());
  for (size_t i = 0; i < kfs.size(); i++) {
    const lsdhip_kfbank::Slot& s = b->slots[i];
    kfs[i] = lsdrp::Keyframe{s.frameId, s.numPoints, s.meanIdepth, lsdrp::sim3_from8(s.camToWorld)};
  }
  const lsdrp::Weights W = {c->params.KFDistWeight, c->params.KFUsageWeight, t->relocalizationTH};
  float fowX, fowY;
  lsdrp::field_of_view(c->w, c->h, c->intr[0].fx, c->intr[0].fy, &fowX, &fowY);
  std::vector<lsdhip_reposition_record>& recs = t->repoRecords;
  memset(res, 0, sizeof(*res));
  res->numPotential = lsdrp::prefilter(kfs, lsdrp::sim3_from8(frameCamToWorld), trackingParentId, maxScore, fowX, fowY, W, &recs);
  // stage 3: one overlap launch for all survivors
  std::vector<int> slots, idx;
  std::vector<double> poses;
  for (size_t i = 0; i < recs.size(); i++)
    if (recs[i].stage == LSDHIP_REPO_SCORE) { idx.push_back((int)i); slots.push_back(recs[i].slot); poses.insert(poses.end(), recs[i].refToFrame, recs[i].refToFrame + 7); }
  res->numChecked = (int)idx.size();
  std::vector<int> tracked;
  if (!idx.empty()) {
    std::vector<float> usage(idx.size());
    if (int rc = overlap_bank_run(t, b, (int)idx.size(), slots.data(), poses.data(), usage.data())) return rc;
    res->overlapLaunches = 1;
    for (size_t k = 0; k < idx.size(); k++)
      if (lsdrp::wants_tracking(recs[(size_t)idx[k]], usage[k], maxScore, W)) tracked.push_back(idx[k]);
  }
  // stage 4: one tracking batch for those below maxScore
  std::vector<lsdhip_track_result> out(tracked.size());
  if (!tracked.empty()) {
    slots.clear(); poses.clear();
    std::vector<lsdhip_frame*> frames(tracked.size(), frame);
    for (int i : tracked) { slots.push_back(recs[(size_t)i].slot); poses.insert(poses.end(), recs[(size_t)i].refToFrame, recs[(size_t)i].refToFrame + 7); }
    const int rc = permaref_bank_run(t, b, (int)tracked.size(), slots.data(), frames.data(), poses.data(), out.data());
    if (rc != LSDHIP_OK && rc != LSDHIP_DIVERGED) return rc;
    res->trackingBatches = 1;
  }
  lsdrp::select(recs, kfs, tracked, out.data(), maxScore, W, res);
  return LSDHIP_OK;
}
extern "C" int lsdhip_tracker_reposition_records(lsdhip_tracker* t, int max, lsdhip_reposition_record* records, int* n) {
  if (!t || max < 0 || !n || (max > 0 && !records)) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(t->ctx);
  *n = (int)t->repoRecords.size();
  for (int i = 0; i < *n && i < max; i++) records[i] = t->repoRecords[(size_t)i];
  return LSDHIP_OK;
}
extern "C" int lsdhip_tracker_set_relocalization_th(lsdhip_tracker* t, float th) {
  if (!t) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(t->ctx);
  t->relocalizationTH = th;
  return LSDHIP_OK;
}

// Test hook: lm_wave's proposal (gj6_solve_wave, se3f_exp_wave, se3f_mul_wave) for n given systems, case k: inc solves
// (A with its diagonal * damp) inc = -b for the LGS6 (A, b) after finish(), Tn = exp(inc) * T.  Reads no image.
extern "C" int lsdhip_devtest_se3f_lm_step(lsdhip_ctx* c, int n, const float* A, const float* b, const float* damp, const float* T,
                                           float* inc, float* Tn) {
  if (!c || n <= 0 || !A || !b || !damp || !T || !inc || !Tn) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  if (c->pipeline) { if (int rc = lsd_sync_all(c)) return rc; }
  const size_t nin = (size_t)n * (36 + 6 + 1 + 7), nout = (size_t)n * (6 + 7);
  LsdDev<float> buf;      // one device buffer for all inputs and outputs of the call, freed on every return path
  if (int rc = lsd_dev_alloc(buf, nin + nout)) return rc;
  float* d = buf;
  float *dA = d, *db = dA + (size_t)n * 36, *ddamp = db + (size_t)n * 6, *dT = ddamp + n, *dinc = dT + (size_t)n * 7, *dTn = dinc + (size_t)n * 6;
  HIPCHK(hipMemcpyAsync(dA, A, (size_t)n * 36 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(db, b, (size_t)n * 6 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(ddamp, damp, (size_t)n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(dT, T, (size_t)n * 7 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_devtest_se3f_lm_step, dim3(n), dim3(64), 0, c->stream, dA, db, ddamp, dT, dinc, dTn);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(inc, dinc, (size_t)n * 6 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(Tn, dTn, (size_t)n * 7 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return LSDHIP_OK;
}
