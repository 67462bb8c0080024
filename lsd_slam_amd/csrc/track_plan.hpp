// How a tracking job is run, as pure functions over plain integers: the tiling of a level, the shape of a batch, the trials and the grid of
// a single job's launches and of a batch's rounds, and the launch budget.  The policy constants live here.  Plain C++ without HIP headers:
// tests/cpp/track_plan_test.cpp checks the arithmetic; tracker.hip turns a plan into a TrackSpec and tilings once per job.
#pragma once
#include "../../include/lsdhip.h"

#define LSD_SPEC_MAX 6                      // most trials a single job's launch evaluates (the scratch arena and the side planes are sized by it)
#define LSD_SPEC_TRIALS_SMALL 6             // automatic speculation policy: trials per step on levels of up to LSD_SPEC_SMALL_PX pixels
#define LSD_SPEC_SMALL_PX 6144
#define LSD_SPEC_TRIALS_MID 5               // ... up to LSD_SPEC_MID_PX pixels; larger levels: one evaluation per step
#define LSD_SPEC_MID_PX 90112
#define LSD_SPEC_CAP_WORKGROUPS 80          // workgroups per trial on speculating levels above LSD_SPEC_CAP_ABOVE_PX pixels
#define LSD_SPEC_CAP_ABOVE_PX 24576
#define LSD_BATCH_THROUGHPUT_MIN_JOBS 8     // lsdhip_tracker_track_batch: throughput mode from this many jobs on
#define LSD_BATCH_SPEC_MAX 4                // reject-chain speculation of batches in throughput mode: most trials per step (levels without a mask)
#define LSD_BATCH_SPEC_PIXELS 500000        // ... trials per step at a level = what keeps jobs x trials x pixels of the level within this (1 M until round 5: 64-job batches lost 12 % to it)
#define LSD_BATCH_STRIP_WORKGROUPS 768      // strips x jobs of a throughput-mode evaluation launch (3 workgroups per CU)
#define LSD_SOLO_MAX_PX 4800                // largest level one workgroup per job walks on its own (k_track_solo: the level is one strip and one LDS tile)
// k_track_solo is worth it from this many jobs per batch: one workgroup per job walks its coarse levels in about the time the lock-step
// rounds take, on n CUs instead of the chip — a gain where other work (the mapping stream of the S-sequence loop) wants the other CUs, a
// small loss for a few jobs that have the chip to themselves (profiles/r06_notes.md section 21).
#define LSD_SOLO_MIN_JOBS 24

constexpr int LSD_PLAN_LEVELS = LSDHIP_PYRAMID_LEVELS;

// Most workgroups one evaluation uses (LSDHIP_TRACK_CAP): a multiple of 8, at least 8, and the rows per column slice must fit the 20
// float4 loads of the column-sum phase: 80 rows x the slices that the waves behind the first hold (`columns` sums each).
inline int lsd_grid_cap(int requested, int block, int columns) {
  int cap = (requested < 8 ? 8 : requested) & ~7;
  const int nslice = ((block / 64 - 1) * 64) / columns;
  if (cap > 80 * nslice) cap = (80 * nslice) & ~7;
  return cap;
}

// The batch a job is described for: how many jobs share its launches, and the workgroups each of them may use at a level.  With many
// jobs in flight the other jobs hide a job's latency, so each job gets fewer, fatter workgroups: the per-workgroup LM replay (the price
// of the launch needing no inter-workgroup communication) shrinks accordingly.  {0, 0}: a single job on the tracker's own grid_cap.
struct BatchShape { int jobs, cap; };
inline BatchShape lsd_batch_shape(int grid_cap, int n) {
  if (n <= 1) return {0, 0};
  const int cap = (grid_cap / n) & ~7;
  return {n, cap < 16 ? 16 : cap};
}

// Tiling of a level of `work` pixels (or points) for workgroups of `block` lanes.  refBlocks: a dense level with reference blocks (levels
// >= 1 of a keyframe), which a batch in throughput mode cuts into strips.
struct LevelTiling {
  int nblocks;      // workgroups (tiles) that have work
  int singlePass;   // nblocks * block >= work: every lane evaluates at most one point
  int tilePx;       // > 0: one strip of tilePx pixels per workgroup, compacted in the workgroup
};
inline int lsd_single_pass(int nblocks, int block, long long work) { return (long long)nblocks * block >= work ? 1 : 0; }
inline LevelTiling lsd_level_tiling(int work, int block, int grid_cap, BatchShape shape, bool refBlocks, int stripWgs, int max_blocks) {
  LevelTiling T;
  T.nblocks = (work + block - 1) / block;
  if (T.nblocks >= 16) T.nblocks = (T.nblocks + 7) & ~7;   // multiples of 8: one contiguous band of tiles per XCD
  const int cap = shape.cap > 0 ? shape.cap : grid_cap;
  if (T.nblocks > cap) T.nblocks = cap;                     // larger levels grid-stride
  if (T.nblocks < 1) T.nblocks = 1;
  T.singlePass = lsd_single_pass(T.nblocks, block, work);
  T.tilePx = 0;
  if (shape.jobs >= LSD_BATCH_THROUGHPUT_MIN_JOBS && refBlocks) {
    // throughput mode: strips x jobs = the chip's 768 workgroup slots (3 per CU) where the level is large enough: one full round of equal
    // strips; a strip is a multiple of 256 pixels (the lanes take 4 consecutive pixels each)
    long long px = (((long long)work * shape.jobs + stripWgs - 1) / stripWgs + 255) & ~255LL;
    if (px < 1024) px = 1024;
    if (px > 8192) px = 8192;                                  // the strip's list lives in the reduction's LDS (10545 words)
    if ((work + px - 1) / px <= max_blocks) {                  // (levels beyond 2.4 Mpixel keep the grid-stride form)
      T.tilePx = (int)px;
      T.nblocks = (int)((work + px - 1) / px);
      T.singlePass = 0;
    }
  }
  return T;
}

// ---- a single job ---------------------------------------------------------------------------------------------------------------------
// Trials per launch and workgroups per trial, per level.  Speculation pays where a level is latency-bound, i.e. small: the automatic
// policy goes by the level's pixel (or point) count — <= 6 K: 6 trials, <= 24 K: 5, <= 88 K: 5 trials on specCap (80) workgroups each
// (multi-pass; 4 x 104 measured 1.5 % slower), larger: one evaluation per launch on the full grid (such levels are work-bound: at
// 1280x1024 speculating on level 1 cost 15 % of the frame rate).  An explicit lsdhip_tracker_set_speculation / the LSDHIP_SPEC_LEVELS /
// _CAPS environment overrides it.
struct SpecPolicy {
  int specC;                           // most trials per launch (1: no speculation)
  bool specAuto;                       // trials from the level's size; false after lsdhip_tracker_set_speculation
  int specLevel[LSD_PLAN_LEVELS];      // per-level trials (0: automatic / specC)
  int specCaps[LSD_PLAN_LEVELS];       // per-level workgroups per trial (0: automatic)
  int specCap;                         // workgroups per trial where the automatic cap applies (0: grid_cap / 2)
  int grid_cap, block;
};
struct LevelWork { long long work; LevelTiling tiling; };
struct SinglePlan {
  int trials[LSD_PLAN_LEVELS];
  LevelTiling tiling[LSD_PLAN_LEVELS];   // as given, nblocks capped (and singlePass derived again) on the levels that speculate under a cap
  int grid;                              // workgroups of a launch: the most tiles x trials of any level the job can still visit
  int specGrid;                          // = grid when the job speculates, else 0
};
inline SinglePlan lsd_single_plan(const LevelWork lv[LSD_PLAN_LEVELS], const SpecPolicy& p, int lastLevel, int topLevel) {
  SinglePlan P;
  for (int l = 0; l < LSD_PLAN_LEVELS; l++) { P.trials[l] = 1; P.tiling[l] = lv[l].tiling; }
  P.grid = 1;
  P.specGrid = 0;
  for (int l = lastLevel; l <= topLevel; l++) {
    if (p.specC > 1) {
      const long long work = lv[l].work;
      int trials, cap = p.specCaps[l];
      if (p.specLevel[l] > 0) trials = p.specLevel[l];
      else if (!p.specAuto) trials = p.specC;
      else trials = work <= LSD_SPEC_SMALL_PX ? LSD_SPEC_TRIALS_SMALL : (work <= LSD_SPEC_MID_PX ? LSD_SPEC_TRIALS_MID : 1);
      if (trials > p.specC) trials = p.specC;
      if (cap <= 0 && trials > 1 && (p.specAuto ? work > LSD_SPEC_CAP_ABOVE_PX : l == lastLevel)) cap = p.specCap > 0 ? p.specCap : ((p.grid_cap / 2 + 7) & ~7);
      P.trials[l] = trials;
      LevelTiling& T = P.tiling[l];
      if (trials > 1 && cap > 0 && T.nblocks > cap && T.tilePx == 0) {
        T.nblocks = cap;
        T.singlePass = lsd_single_pass(T.nblocks, p.block, work);
      }
    }
    // workgroup = (trial, tile) of the level being evaluated
    const int g = P.tiling[l].nblocks * P.trials[l];
    if (g > P.grid) P.grid = g;
  }
  if (p.specC > 1) P.specGrid = P.grid;
  return P;
}

// ---- a batch --------------------------------------------------------------------------------------------------------------------------
// Reject-chain speculation in throughput mode (as single jobs have it, SE3Tracker.cpp:341-447): a step evaluates the next `trials`
// retries of the LM loop side by side, the next step consumes them in the reference's order — same decisions, same evaluation counts,
// fewer dependent rounds.  Per level as many trials as keep jobs x trials x pixels of the level within specPixels (a round must not cost
// more than the rounds it saves); one at the level that writes refPixelWasGood (no side planes in batches).
struct BatchLevel { long long px; int nblocks, tilePx, writeMask, inRange; };   // px = w x h of the level; inRange: lastLevel <= level <= topLevel
struct BatchPolicy {
  int specC;              // the tracker's own most trials per launch (lsdhip_tracker_set_speculation(t, 1, 0): one evaluation per step, batches too)
  int specMax;            // LSDHIP_BATCH_SPEC
  long long specPixels;   // LSDHIP_BATCH_SPEC_PIXELS
  int fused;              // LSDHIP_BATCH_FUSED
  bool spinWait, poll;    // LSDHIP_SPIN, LSDHIP_BATCH_POLL
  int soloMin;            // lsdhip_tracker_set_batch_coarse_min_jobs / LSDHIP_BATCH_SOLO_MIN (0: never)
};
struct BatchPlan {
  bool split;             // some level is cut into strips: throughput mode
  bool speculates;        // the rounds carry trials (else the launches take an empty TrackSpec)
  int trials[LSD_PLAN_LEVELS];
  int lmGrid;             // most trials of any level: the workgroups per job of an LM launch
  int grid;               // workgroups per job of an evaluation launch: the most (trial, strip) pairs of any level
  int cmax;               // trial slots per parity of the scratch
  bool polled;            // the host polls the summaries instead of draining the stream
  bool soloDue;           // the first launch is k_track_solo
};
// level(j, l): the BatchLevel of job j at level l
template <class LevelOf> inline BatchPlan lsd_batch_plan(int n, const BatchPolicy& p, LevelOf level) {
  BatchPlan P = {};
  for (int j = 0; j < n; j++)
    for (int l = 0; l < LSD_PLAN_LEVELS; l++) { const BatchLevel L = level(j, l); P.split = P.split || (L.inRange && L.tilePx > 0); }
  int specMax = p.specMax;
  if (p.specC < specMax) specMax = p.specC;
  if (p.fused == 1) specMax = 1;
  P.speculates = P.split && specMax > 1;
  P.lmGrid = 1;
  for (int l = 0; l < LSD_PLAN_LEVELS; l++) {
    P.trials[l] = 1;
    bool ok = P.speculates;
    for (int j = 0; j < n && ok; j++) { const BatchLevel L = level(j, l); ok = L.inRange && L.tilePx > 0 && !L.writeMask; }
    if (!ok) continue;
    long long tr = p.specPixels / (level(0, l).px * n);
    if (tr > specMax) tr = specMax;
    if (tr < 1) tr = 1;
    P.trials[l] = (int)tr;
    if (tr > P.lmGrid) P.lmGrid = (int)tr;
  }
  P.grid = 1;
  for (int j = 0; j < n; j++)
    for (int l = 0; l < LSD_PLAN_LEVELS; l++) {
      const BatchLevel L = level(j, l);
      if (L.inRange && L.nblocks * P.trials[l] > P.grid) P.grid = L.nblocks * P.trials[l];
    }
  P.cmax = P.split && P.lmGrid > 1 ? LSD_BATCH_SPEC_MAX : 1;
  P.polled = P.split && p.fused && p.spinWait && p.poll;
  // the coarse levels of every job inside one workgroup (k_track_solo) — nothing to walk if no job's top level fits the tile
  // (1280x1024: level 4 is 80x64 = 5120 pixels): the launch would only copy states
  if (P.split && p.fused && p.soloMin > 0 && n >= p.soloMin)
    for (int j = 0; j < n && !P.soloDue; j++) {
      BatchLevel top = {};
      for (int l = 0; l < LSD_PLAN_LEVELS; l++) if (level(j, l).inRange) top = level(j, l);
      P.soloDue = top.tilePx > 0 && !top.writeMask && top.px <= LSD_SOLO_MAX_PX;
    }
  return P;
}

// ---- the launch budget ----------------------------------------------------------------------------------------------------------------
// What the last four jobs (or batches) needed sizes the budget of the next one: their maximum plus a margin, so that few launches run
// empty (a launch queued behind the finishing one leaves at once, 3 - 4 us).  fixed > 0 overrides (LSDHIP_BUDGET_FIXED, a test hook).
struct LaunchHistory {
  int recent[4] = {0, 0, 0, 0};
  int budget(int dflt, int margin, int fixed) const {
    if (fixed > 0) return fixed;
    if (recent[0] <= 0) return dflt;
    int most = 0;
    for (int i = 0; i < 4; i++) if (recent[i] > most) most = recent[i];
    return most + margin;
  }
  void note(int launches) { recent[3] = recent[2]; recent[2] = recent[1]; recent[1] = recent[0]; recent[0] = launches; }
};
