// How a tracking job is run (lsd_slam_amd/csrc/track_plan.hpp), without HIP: level tilings, the shape of a batch, the trials, caps and
// grids of single jobs at 640x480 and 1280x1024, the strips and trials of batches, and the launch budget — against values worked out by
// hand from the formulas.  Block 256, grid_cap 304, default speculation settings, 768 strip workgroups, 500000 speculation pixels.
// Usage: track_plan_test   (exit status 0 = all checks hold; prints "track plan ok")
#include <cstdio>
#include <initializer_list>
#include "../../lsd_slam_amd/csrc/track_plan.hpp"

namespace {
constexpr int L = LSD_PLAN_LEVELS, BLOCK = 256, CAP = 304, WGS = LSD_BATCH_STRIP_WORKGROUPS;
int g_fail = 0;
#define CHECK(cond, ...)                                         \
  do {                                                           \
    if (!(cond)) {                                               \
      g_fail++;                                                  \
      std::printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                                  \
      std::printf("\n");                                         \
    }                                                            \
  } while (0)

SpecPolicy policy(int specC, bool specAuto) {
  SpecPolicy p = {};
  p.specC = specC; p.specAuto = specAuto; p.specCap = LSD_SPEC_CAP_WORKGROUPS; p.grid_cap = CAP; p.block = BLOCK;
  return p;
}
// the dense levels 1..4 of a w x h trackFrame job, tiled for `shape`
void dense_levels(int w, int h, BatchShape shape, LevelWork lv[L]) {
  for (int l = 0; l < L; l++) {
    const int work = (w >> l) * (h >> l);
    lv[l] = {work, lsd_level_tiling(work, BLOCK, CAP, shape, l >= 1, WGS, CAP)};
  }
}
struct Row { int level, trials, nblocks, singlePass; };   // singlePass < 0: not part of the expectation
void check_single(const char* what, int w, int h, const Row* rows, int nrows, int grid) {
  LevelWork lv[L];
  dense_levels(w, h, BatchShape{0, 0}, lv);
  const SinglePlan P = lsd_single_plan(lv, policy(LSD_SPEC_MAX, true), 1, 4);
  for (int i = 0; i < nrows; i++) {
    const Row& r = rows[i];
    CHECK(P.trials[r.level] == r.trials, "%s level %d: %d trials", what, r.level, P.trials[r.level]);
    CHECK(P.tiling[r.level].nblocks == r.nblocks, "%s level %d: %d workgroups", what, r.level, P.tiling[r.level].nblocks);
    if (r.singlePass >= 0) CHECK(P.tiling[r.level].singlePass == r.singlePass, "%s level %d: singlePass %d", what, r.level, P.tiling[r.level].singlePass);
    CHECK(P.tiling[r.level].tilePx == 0, "%s level %d: strips in a single job", what, r.level);
  }
  CHECK(P.grid == grid && P.specGrid == grid, "%s: grid %d, specGrid %d", what, P.grid, P.specGrid);
  CHECK(P.trials[0] == 1, "%s: level 0 is outside the job", what);
}
}  // namespace

int main() {
  // grid_cap: multiples of 8 from 8 to what the column-sum phase holds (80 rows x 4 slices of 41 columns in the 3 waves behind the first)
  CHECK(lsd_grid_cap(304, BLOCK, 41) == 304 && lsd_grid_cap(300, BLOCK, 41) == 296 && lsd_grid_cap(3, BLOCK, 41) == 8 && lsd_grid_cap(1000, BLOCK, 41) == 320, "grid cap");

  // ---- single jobs
  {
    const Row r640[] = {{1, 5, 80, 0}, {2, 5, 80, -1}, {3, 6, 24, -1}, {4, 6, 5, -1}};
    check_single("640x480", 640, 480, r640, 4, 400);
    const Row r1280[] = {{1, 1, 304, 0}, {2, 5, 80, 0}, {3, 5, 80, -1}, {4, 6, 24, -1}};
    check_single("1280x1024", 1280, 1024, r1280, 4, 400);
  }
  {  // lsdhip_tracker_set_speculation(t, 1, 0): one trial everywhere, no cap, the grid of the largest level
    LevelWork lv[L];
    dense_levels(640, 480, BatchShape{0, 0}, lv);
    const SinglePlan P = lsd_single_plan(lv, policy(1, false), 1, 4);
    int most = 1;
    for (int l = 1; l <= 4; l++) {
      CHECK(P.trials[l] == 1, "no speculation: level %d has %d trials", l, P.trials[l]);
      CHECK(P.tiling[l].nblocks == lv[l].tiling.nblocks && P.tiling[l].singlePass == lv[l].tiling.singlePass, "no speculation: level %d capped", l);
      if (lv[l].tiling.nblocks > most) most = lv[l].tiling.nblocks;
    }
    CHECK(most == 304 && P.grid == most && P.specGrid == 0, "no speculation: grid %d, specGrid %d", P.grid, P.specGrid);
  }
  {  // a permaref job: 3000 points at level 4
    LevelWork lv[L] = {};
    lv[4] = {3000, lsd_level_tiling(3000, BLOCK, CAP, BatchShape{0, 0}, false, WGS, CAP)};
    const SinglePlan P = lsd_single_plan(lv, policy(LSD_SPEC_MAX, true), 4, 4);
    CHECK(P.trials[4] == 6 && P.tiling[4].nblocks == 12 && P.tiling[4].singlePass == 1, "permaref: %d trials, %d workgroups", P.trials[4], P.tiling[4].nblocks);
    CHECK(P.grid == 72 && P.specGrid == 72, "permaref: grid %d", P.grid);
  }
  {  // point lists under the three policies tests/test_permaref_loop_gpu.py compares (its single_tiles): the default policy caps lists
     // above LSD_SPEC_CAP_ABOVE_PX points at 80 tiles, lsdhip_tracker_set_speculation(t, 6, 8) caps every list at 8, (t, 1, 0) never caps
    struct List { int n, dflt, dfltPass, one, onePass, six8, six8Pass; };
    const List lists[] = {{255, 1, 1, 1, 1, 1, 1},     {2048, 8, 1, 8, 1, 8, 1},      {2049, 9, 1, 9, 1, 8, 0},     {4097, 24, 1, 24, 1, 8, 0},
                          {4836, 24, 1, 24, 1, 8, 0},  {24576, 96, 1, 96, 1, 8, 0},   {25000, 80, 0, 104, 1, 8, 0}};
    SpecPolicy six8 = policy(6, false);
    six8.specCap = 8;
    for (const List& c : lists) {
      LevelWork lv[L] = {};
      lv[4] = {c.n, lsd_level_tiling(c.n, BLOCK, CAP, BatchShape{0, 0}, false, WGS, CAP)};
      const SinglePlan Pd = lsd_single_plan(lv, policy(LSD_SPEC_MAX, true), 4, 4), P1 = lsd_single_plan(lv, policy(1, false), 4, 4), P6 = lsd_single_plan(lv, six8, 4, 4);
      CHECK(Pd.tiling[4].nblocks == c.dflt && Pd.tiling[4].singlePass == c.dfltPass, "%d points, default policy: %d tiles, singlePass %d", c.n, Pd.tiling[4].nblocks, Pd.tiling[4].singlePass);
      CHECK(P1.tiling[4].nblocks == c.one && P1.tiling[4].singlePass == c.onePass && P1.trials[4] == 1, "%d points, (1, 0): %d tiles, singlePass %d", c.n, P1.tiling[4].nblocks, P1.tiling[4].singlePass);
      CHECK(P6.tiling[4].nblocks == c.six8 && P6.tiling[4].singlePass == c.six8Pass && P6.trials[4] == 6, "%d points, (6, 8): %d tiles, singlePass %d", c.n, P6.tiling[4].nblocks, P6.tiling[4].singlePass);
      CHECK(Pd.trials[4] == (c.n <= LSD_SPEC_SMALL_PX ? 6 : 5), "%d points, default policy: %d trials", c.n, Pd.trials[4]);
    }
  }

  // ---- batches
  {
    const BatchShape s1 = lsd_batch_shape(CAP, 1), s8 = lsd_batch_shape(CAP, 8), s64 = lsd_batch_shape(CAP, 64);
    CHECK(s1.jobs == 0 && s1.cap == 0, "shape of 1: {%d, %d}", s1.jobs, s1.cap);
    CHECK(s8.jobs == 8 && s8.cap == 32, "shape of 8: {%d, %d}", s8.jobs, s8.cap);
    CHECK(s64.jobs == 64 && s64.cap == 16, "shape of 64: {%d, %d}", s64.jobs, s64.cap);
  }
  {
    struct Strip { int w, h, jobs, tilePx, strips; };
    const Strip cases[] = {{160, 128, 8, 1024, 5}, {640, 480, 8, 1024, 75}, {640, 480, 32, 3328, 24}};
    for (const Strip& s : cases) {
      const int work = (s.w >> 1) * (s.h >> 1);
      const LevelTiling T = lsd_level_tiling(work, BLOCK, CAP, lsd_batch_shape(CAP, s.jobs), true, WGS, CAP);
      CHECK(T.tilePx == s.tilePx && T.nblocks == s.strips && T.singlePass == 0, "%dx%d level 1, %d jobs: strips of %d pixels, %d of them", s.w, s.h, s.jobs, T.tilePx, T.nblocks);
    }
    // level 0 has no reference blocks; 7 jobs are not throughput mode
    CHECK(lsd_level_tiling(640 * 480, BLOCK, CAP, lsd_batch_shape(CAP, 8), false, WGS, CAP).tilePx == 0, "level 0 in strips");
    for (int l = 1; l <= 4; l++)
      CHECK(lsd_level_tiling((640 >> l) * (480 >> l), BLOCK, CAP, lsd_batch_shape(CAP, 7), true, WGS, CAP).tilePx == 0, "7 jobs: level %d in strips", l);
  }
  {  // 8 trackFrame jobs at 640x480; level 1 writes the mask
    LevelWork lv[L];
    dense_levels(640, 480, lsd_batch_shape(CAP, 8), lv);
    auto level = [&](int, int l) { return BatchLevel{lv[l].work, lv[l].tiling.nblocks, lv[l].tiling.tilePx, l == 1, l >= 1 && l <= 4}; };
    const BatchPolicy p = {LSD_SPEC_MAX, LSD_BATCH_SPEC_MAX, LSD_BATCH_SPEC_PIXELS, 2, true, true, LSD_SOLO_MIN_JOBS};
    const BatchPlan P = lsd_batch_plan(8, p, level);
    CHECK(P.split && P.speculates && P.polled, "8 jobs: split %d, speculates %d, polled %d", P.split, P.speculates, P.polled);
    CHECK(P.trials[1] == 1 && P.trials[2] == 3 && P.trials[3] == 4 && P.trials[4] == 4, "8 jobs: trials %d %d %d %d", P.trials[1], P.trials[2], P.trials[3], P.trials[4]);
    CHECK(P.lmGrid == 4 && P.cmax == LSD_BATCH_SPEC_MAX, "8 jobs: lmGrid %d, cmax %d", P.lmGrid, P.cmax);
    CHECK(P.grid == 75, "8 jobs: grid %d (75 strips of level 1; 19 x 3, 5 x 4 and 2 x 4 below)", P.grid);
    CHECK(!P.soloDue, "8 jobs: below LSD_SOLO_MIN_JOBS");
    BatchPolicy p24 = p;
    p24.soloMin = 8;
    CHECK(lsd_batch_plan(8, p24, level).soloDue, "k_track_solo from 8 jobs on: level 4 of 640x480 fits");
    BatchPolicy spin0 = p;
    spin0.spinWait = false;
    CHECK(!lsd_batch_plan(8, spin0, level).polled, "LSDHIP_SPIN=0: the batch is not polled");
    BatchPolicy one = p;
    one.specC = 1;
    const BatchPlan P1 = lsd_batch_plan(8, one, level);
    CHECK(!P1.speculates && P1.lmGrid == 1 && P1.cmax == 1 && P1.grid == 75, "one trial per step: lmGrid %d, cmax %d, grid %d", P1.lmGrid, P1.cmax, P1.grid);
  }

  // ---- the shapes of tests/test_dispatch_arms_gpu.py: the arms of k_track_step's finishing phase they are chosen for
  {  // a 352x240 job: 88 tiles at level 1 (81..160: the column sums take ten rows per slot), and lsdhip_tracker_set_speculation(t, 5, 88) keeps them
    LevelWork lv[L];
    dense_levels(352, 240, BatchShape{0, 0}, lv);
    SpecPolicy p = policy(5, false);
    p.specCap = 88;
    const SinglePlan P5 = lsd_single_plan(lv, p, 1, 4), P1 = lsd_single_plan(lv, policy(1, false), 1, 4);
    CHECK(lv[1].tiling.nblocks == 88 && P5.tiling[1].nblocks == 88 && P1.tiling[1].nblocks == 88, "352x240 level 1: %d / %d / %d tiles", lv[1].tiling.nblocks, P5.tiling[1].nblocks, P1.tiling[1].nblocks);
    CHECK(P5.trials[1] == 5 && P1.trials[1] == 1 && P5.grid == 440, "352x240 level 1: %d and %d trials, grid %d", P5.trials[1], P1.trials[1], P5.grid);
  }
  {  // 8 jobs at 352x288: 25 / 7 / 2 / 1 strips per job at levels 1..4 (6..13: the middle form of the tail rows), four trials below level 1
    LevelWork lv[L];
    dense_levels(352, 288, lsd_batch_shape(CAP, 8), lv);
    auto level = [&](int, int l) { return BatchLevel{lv[l].work, lv[l].tiling.nblocks, lv[l].tiling.tilePx, l == 1, l >= 1 && l <= 4}; };
    const BatchPolicy p = {LSD_SPEC_MAX, LSD_BATCH_SPEC_MAX, LSD_BATCH_SPEC_PIXELS, 2, true, true, LSD_SOLO_MIN_JOBS};
    const BatchPlan P = lsd_batch_plan(8, p, level);
    CHECK(lv[1].tiling.nblocks == 25 && lv[2].tiling.nblocks == 7 && lv[3].tiling.nblocks == 2 && lv[4].tiling.nblocks == 1 && lv[2].tiling.tilePx == 1024,
          "352x288, 8 jobs: %d %d %d %d strips", lv[1].tiling.nblocks, lv[2].tiling.nblocks, lv[3].tiling.nblocks, lv[4].tiling.nblocks);
    CHECK(P.trials[1] == 1 && P.trials[2] == 4 && !P.soloDue, "352x288, 8 jobs: trials %d %d", P.trials[1], P.trials[2]);
  }

  // ---- launch budget
  {
    LaunchHistory h;
    CHECK(h.budget(12, 2, 0) == 12 && h.budget(26, 3, 0) == 26, "empty history");
    for (int v : {8, 11, 7, 9}) h.note(v);          // oldest first: recent = {9, 7, 11, 8}
    CHECK(h.recent[0] == 9 && h.recent[1] == 7 && h.recent[2] == 11 && h.recent[3] == 8, "history order");
    CHECK(h.budget(12, 2, 0) == 13, "budget %d", h.budget(12, 2, 0));
    CHECK(h.budget(12, 2, 3) == 3 && LaunchHistory{}.budget(12, 2, 3) == 3, "fixed budget");
    h.note(20);
    CHECK(h.recent[3] == 11 && h.budget(12, 2, 0) == 22, "the oldest entry leaves");
  }
  if (g_fail == 0) std::printf("track plan ok\n");
  return g_fail ? 1 : 0;
}
