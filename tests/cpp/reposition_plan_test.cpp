// The host part of findRePositionCandidate (lsd_slam_amd/csrc/reposition_plan.hpp), without HIP, against values worked out by hand:
// the Euclidean prefilter (distance scaled by meanIdepth / scale, viewing direction, refToFrame), the two skips, an empty slot, the score,
// and the selection loop replayed over given tracking results — including the reference's quirk (the test reads newScore < bestScore,
// the store is bestScore = score: TrackableKeyFrameSearch.cpp:143-146), an empty bank and a bank whose keyframes are all far.
// 640x480 with fx = 320, fy = 240 (fowX = fowY = pi / 2, cosAngleTH = cos(0.375 pi)), KFDistWeight 4, KFUsageWeight 3, maxScore 1:
// distanceTH = 1 / 16.  Usage: reposition_plan_test   (exit status 0 = all checks hold; prints "reposition plan ok")
#include <cmath>
#include <cstdio>
#include <vector>
#include "../../lsd_slam_amd/csrc/reposition_plan.hpp"

namespace {
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
bool near(double a, double b, double tol = 1e-6) { return std::fabs(a - b) <= tol; }

lsdrp::Keyframe kf(int id, double x, int numPoints = 100, float meanIdepth = 0.5f, double scale = 1.0) {
  const double p[8] = {1, 0, 0, 0, x, 0, 0, scale};
  return lsdrp::Keyframe{id, numPoints, meanIdepth, lsdrp::sim3_from8(p)};
}
lsdhip_track_result tracked(double x, double y, float usage, float good, float bad, int wasGood, int diverged = 0) {
  lsdhip_track_result r = {};
  r.frameToReference[0] = 1; r.frameToReference[4] = x; r.frameToReference[5] = y;
  r.pointUsage = usage; r.lastGoodCount = good; r.lastBadCount = bad; r.trackingWasGood = wasGood; r.diverged = diverged;
  return r;
}
}  // namespace

int main() {
  using namespace lsdrp;
  const Weights W = {4.f, 3.f, 0.7f};
  float fowX, fowY;
  field_of_view(640, 480, 320.f, 240.f, &fowX, &fowY);
  CHECK(near(fowX, M_PI / 2) && near(fowY, M_PI / 2), "fow %f %f", fowX, fowY);
  CHECK(near(ref_frame_score(0.04f, 0.5f, W), 2.89), "score %f", ref_frame_score(0.04f, 0.5f, W));

  // ---- pose algebra ----
  {
    const double rz[7] = {std::cos(0.05), 0, 0, std::sin(0.05), 0, 0, 0}, tr[7] = {1, 0, 0, 0, 0.3, 0.4, 0};
    CHECK(near(se3_log_norm(se3_from7(rz)), 0.1, 1e-12), "%f", se3_log_norm(se3_from7(rz)));
    CHECK(near(se3_log_norm(se3_from7(tr)), 0.5, 1e-12), "%f", se3_log_norm(se3_from7(tr)));
    const SE3 a = se3_from7(rz), b = se3_from7(tr);
    CHECK(near(se3_log_norm(se3_mul(se3_mul(a, b), se3_inverse(se3_mul(a, b)))), 0.0, 1e-12), "T T^-1");
    const double s8[8] = {std::cos(0.2), 0, std::sin(0.2), 0, 1, 2, 3, 2.5};
    const Sim3 S = sim3_from8(s8), I = sim3_mul(S, sim3_inverse(S));
    CHECK(near(I.s, 1) && near(I.t[0], 0) && near(I.t[1], 0) && near(I.t[2], 0) && near(I.q.w, 1), "S S^-1");
  }

  // ---- the bank ----
  std::vector<Keyframe> kfs;
  for (int i = 0; i < 5; i++) kfs.push_back(kf(100 + i, 0.1));       // slots 0-4: near, but of the initialisation phase
  kfs.push_back(kf(105, 1.0));                                        // 5: (1 * 0.5)^2 = 0.25 > 1/16: far
  kfs.push_back(kf(106, 0.2));                                        // 6: the tracking parent
  {                                                                   // 7: looks along +x: viewing directions orthogonal
    Keyframe k = kf(107, 0.1);
    k.camToWorld.q = {std::cos(M_PI / 4), 0, std::sin(M_PI / 4), 0};
    kfs.push_back(k);
  }
  kfs.push_back(kf(108, 0.2, 0));                                     // 8: empty cloud
  kfs.push_back(kf(109, 0.4));                                        // 9: d2 = 0.04; usage 0.5 -> score 2.89: not tracked
  kfs.push_back(kf(110, 0.2));                                        // 10: d2 = 0.01; usage 0.9 -> score 0.25
  kfs.push_back(kf(111, 0.1));                                        // 11: d2 = 0.0025; usage 0.8 -> score 0.4
  kfs.push_back(kf(112, 0.3));                                        // 12: d2 = 0.0225; usage 0.9 -> score 0.45
  // 13 - 16: each fails exactly ONE clause of the acceptance test (TrackableKeyFrameSearch.cpp:143) and passes the other three
  kfs.push_back(kf(113, 0.3));                                        // 13: as 12; tracked pose 0.32 off: poseDiscrepancy alone
  kfs.push_back(kf(114, 0.3));                                        // 14: as 12; trackingWasGood false alone
  kfs.push_back(kf(115, 0.8, 100, 0.5f, 2.0));                        // 15: scale 2: distFac 0.25, d2 = 0.04; usage 0.95 -> 0.6625; goodVal alone
  kfs.push_back(kf(116, 0.3));                                        // 16: as 12; newScore against the running best alone
  kfs.push_back(kf(117, 0.3));                                        // 17: as 12; diverges
  const double origin[8] = {1, 0, 0, 0, 0, 0, 0, 1};
  std::vector<lsdhip_reposition_record> recs;
  const int potential = prefilter(kfs, sim3_from8(origin), 106, 1.0f, fowX, fowY, W, &recs);
  CHECK(potential == 16, "potential %d", potential);
  const int wantStage[18] = {3, 3, 3, 3, 3, 0, 2, 1, 4, 5, 5, 5, 5, 5, 5, 5, 5, 5};
  for (int i = 0; i < 18; i++) CHECK(recs[(size_t)i].stage == wantStage[i] && recs[(size_t)i].slot == i && recs[(size_t)i].frameId == 100 + i, "slot %d stage %d", i, recs[(size_t)i].stage);
  CHECK(near(recs[5].dist2, 0.25) && near(recs[9].dist2, 0.04) && near(recs[10].dist2, 0.01) && near(recs[15].dist2, 0.04), "dist2");
  CHECK(near(recs[7].angle, 0.0) && near(recs[9].angle, 1.0), "angle %f", recs[7].angle);
  // refToFrame = (kf^-1 frame)^-1: the keyframe's centre seen from the frame
  CHECK(near(recs[10].refToFrame[4], 0.2) && near(recs[10].refToFrame[0], 1.0), "refToFrame %f", recs[10].refToFrame[4]);
  CHECK(near(recs[15].refToFrame[4], 0.4), "refToFrame under scale 2: %f", recs[15].refToFrame[4]);   // se3FromSim3 drops the scale: t = 0.8 / 2

  // ---- stage 3's verdicts ----
  const float usage[9] = {0.5f, 0.9f, 0.8f, 0.9f, 0.9f, 0.9f, 0.95f, 0.9f, 0.9f};
  const double wantScore[9] = {2.89, 0.25, 0.4, 0.45, 0.45, 0.45, 0.6625, 0.45, 0.45};
  std::vector<int> tr;
  for (int k = 0; k < 9; k++) {
    const bool go = wants_tracking(recs[(size_t)(9 + k)], usage[k], 1.0f, W);
    CHECK(near(recs[(size_t)(9 + k)].score, wantScore[k]), "score %d: %f", 9 + k, recs[(size_t)(9 + k)].score);
    CHECK(go == (k != 0), "slot %d tracked %d", 9 + k, (int)go);
    if (go) tr.push_back(9 + k);
  }

  // ---- the selection ----
  // the running best is 0.45 from slot 12 on (nothing after it is taken)
  const lsdhip_track_result out[8] = {
      tracked(0.2, 0, 0.9f, 90, 10, 1),      // 10: newScore 0.01 * 16 + 0.09 = 0.25 < 1: taken, bestScore = score = 0.25
      tracked(0.1, 0, 0.95f, 95, 5, 1),      // 11: newScore 0.04 + 0.0225 = 0.0625 < 0.25: taken, bestScore = score = 0.4 (not 0.0625)
      tracked(0.25, 0, 0.9f, 90, 10, 1),     // 12: newScore 0.25 + 0.09 = 0.34 < 0.4: taken — under bestScore = newScore it would lose to 0.0625
      tracked(0.1, 0.25, 0.9f, 90, 10, 1),   // 13: newScore 0.018125 * 16 + 0.09 = 0.38 < 0.45, goodVal 0.81, but |(0.2, -0.25)| = 0.3202 >= 0.2
      tracked(0.25, 0, 0.9f, 90, 10, 0),     // 14: newScore 0.34 < 0.45, goodVal 0.81, discrepancy 0.05, but trackingWasGood false
      tracked(0.3, 0, 0.95f, 60, 40, 1),     // 15: newScore 0.36 + 0.0225 = 0.3825 < 0.45, discrepancy 0.1, but goodVal 0.95 * 0.6 = 0.57 <= 0.7
      tracked(0.32, 0, 0.9f, 90, 10, 1),     // 16: goodVal 0.81, discrepancy 0.02, but newScore 0.4096 + 0.09 = 0.4996 >= 0.45
      tracked(0, 0, 0.f, 0, 0, 0, 1)};       // 17: diverged: identity, goodVal 0 / 0
  lsdhip_reposition_result res = {};
  select(recs, kfs, tr, out, 1.0f, W, &res);
  CHECK(res.slot == 12 && res.frameId == 112 && res.numTracked == 8, "winner %d", res.slot);
  CHECK(near(res.bestScore, 0.45) && near(res.bestDist, 0.015625) && near(res.bestUsage, 0.9) && near(res.bestPoseDiscrepancy, 0.05), "best %f %f %f %f",
        res.bestScore, res.bestDist, res.bestUsage, res.bestPoseDiscrepancy);
  CHECK(near(res.refToFrame[4], 0.3) && near(res.refToFrame_tracked[4], 0.25), "winner's poses");
  const int wantFinal[8] = {7, 7, 7, 6, 6, 6, 6, 6};
  for (int k = 0; k < 8; k++) CHECK(recs[(size_t)(10 + k)].stage == wantFinal[k], "slot %d final stage %d", 10 + k, recs[(size_t)(10 + k)].stage);
  CHECK(near(recs[10].newScore, 0.25) && near(recs[11].newScore, 0.0625) && near(recs[12].newScore, 0.34), "newScore");
  CHECK(near(recs[10].goodVal, 0.81) && near(recs[11].goodVal, 0.9025) && near(recs[11].usageTracked, 0.95) && near(recs[11].usage, 0.8), "goodVal");
  CHECK(near(recs[10].poseDiscrepancy, 0.0), "discrepancy %f", recs[10].poseDiscrepancy);
  // the four sole reasons: every other clause of the test holds for the record
  CHECK(near(recs[13].poseDiscrepancy, std::sqrt(0.1025)) && near(recs[13].newScore, 0.38) && near(recs[13].goodVal, 0.81) && recs[13].trackingWasGood == 1,
        "13: %f %f", recs[13].poseDiscrepancy, recs[13].newScore);
  CHECK(recs[14].trackingWasGood == 0 && near(recs[14].newScore, 0.34) && near(recs[14].goodVal, 0.81) && near(recs[14].poseDiscrepancy, 0.05), "14: %f", recs[14].newScore);
  CHECK(near(recs[15].goodVal, 0.57) && near(recs[15].newScore, 0.3825) && near(recs[15].poseDiscrepancy, 0.1) && recs[15].trackingWasGood == 1, "15: %f %f",
        recs[15].goodVal, recs[15].newScore);
  CHECK(near(recs[16].newScore, 0.4996) && near(recs[16].goodVal, 0.81) && near(recs[16].poseDiscrepancy, 0.02) && recs[16].trackingWasGood == 1, "16: %f", recs[16].newScore);
  CHECK(recs[17].diverged == 1 && std::isnan(recs[17].goodVal), "diverged job");

  // ---- an empty bank, and one whose keyframes are all far ----
  {
    std::vector<Keyframe> none;
    std::vector<lsdhip_reposition_record> r0;
    CHECK(prefilter(none, sim3_from8(origin), -1, 1.0f, fowX, fowY, W, &r0) == 0 && r0.empty(), "empty bank");
    lsdhip_reposition_result e = {};
    select(r0, none, std::vector<int>(), nullptr, 1.0f, W, &e);
    CHECK(e.slot == -1 && e.frameId == -1 && e.numTracked == 0 && e.bestScore == 1.0f && e.refToFrame[0] == 1.0, "empty result");
    std::vector<Keyframe> far;
    for (int i = 0; i < 8; i++) far.push_back(kf(i, 0.6 + 0.1 * i));     // 0.3^2 = 0.09 > 1/16 and beyond
    CHECK(prefilter(far, sim3_from8(origin), -1, 1.0f, fowX, fowY, W, &r0) == 0 && r0.size() == 8, "all far");
    for (const lsdhip_reposition_record& r : r0) CHECK(r.stage == LSDHIP_REPO_FAR, "far stage %d", r.stage);
  }
  if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
  std::printf("reposition plan ok\n");
  return 0;
}
