// The per-frame rules of the loops (include/lsd_slam_hip_loop.hpp) as a filter: tests/test_loop_rules_cpu.py feeds it cases, one per
// line, and compares what it prints with a table written from the reference.  Floats travel as the hex of their 32 bits.
//   lost diverged good numKeyframes      -> trackingLost                    (0 / 1)
//   finalise mappedOnKF                  -> finaliseOnLoss                  (0 / 1)
//   every kfEvery sinceKF                -> wantsNewKeyframe, fixed interval (0 / 1)
//   score dist2 usage                    -> keyframeScore                   (bits)
//   scorew dist2 usage distW usageW      -> keyframeScore with explicit weights (bits)
//   threshold numKeyframes | threshold - -> scoreThreshold with / without a kept bank (bits)
//   wants mappedOnKF score threshold     -> wantsNewKeyframe, score rule     (0 / 1)
//   step lost onCurrent wants            -> mappingStep                     (lost / dropped / update / change)
//   constants                            -> INITIALIZATION_PHASE_COUNT MIN_NUM_MAPPED KF_DIST_WEIGHT KF_USAGE_WEIGHT, the iteration table
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/lsd_slam_hip_loop.hpp"

using namespace lsd_slam::loop;

static bool readFloat(float* f) {
  unsigned u;
  if (std::scanf("%x", &u) != 1) return false;
  const std::uint32_t b = u;
  std::memcpy(f, &b, 4);
  return true;
}
static void printFloat(float f) {
  std::uint32_t b;
  std::memcpy(&b, &f, 4);
  std::printf("%08x\n", (unsigned)b);
}

int main() {
  char op[16];
  while (std::scanf("%15s", op) == 1) {
    int a, b, c;
    float x, y;
    if (!std::strcmp(op, "lost")) {
      if (std::scanf("%d %d %d", &a, &b, &c) != 3) return 2;
      std::printf("%d\n", trackingLost(a != 0, b != 0, c) ? 1 : 0);
    } else if (!std::strcmp(op, "finalise")) {
      if (std::scanf("%d", &a) != 1) return 2;
      std::printf("%d\n", finaliseOnLoss(a) ? 1 : 0);
    } else if (!std::strcmp(op, "every")) {
      if (std::scanf("%d %d", &a, &b) != 2) return 2;
      std::printf("%d\n", wantsNewKeyframe(a, b) ? 1 : 0);
    } else if (!std::strcmp(op, "score")) {
      if (!readFloat(&x) || !readFloat(&y)) return 2;
      printFloat(keyframeScore(x, y));
    } else if (!std::strcmp(op, "scorew")) {
      float wd, wu;
      if (!readFloat(&x) || !readFloat(&y) || !readFloat(&wd) || !readFloat(&wu)) return 2;
      printFloat(keyframeScore(x, y, wd, wu));
    } else if (!std::strcmp(op, "threshold")) {
      char arg[16];
      if (std::scanf("%15s", arg) != 1) return 2;
      if (!std::strcmp(arg, "-")) printFloat(scoreThreshold());
      else if (std::sscanf(arg, "%d", &a) == 1) printFloat(scoreThreshold(a));
      else return 2;
    } else if (!std::strcmp(op, "wants")) {
      if (std::scanf("%d", &a) != 1 || !readFloat(&x) || !readFloat(&y)) return 2;
      std::printf("%d\n", wantsNewKeyframe(a, x, y) ? 1 : 0);
    } else if (!std::strcmp(op, "step")) {
      if (std::scanf("%d %d %d", &a, &b, &c) != 3) return 2;
      switch (mappingStep(a != 0, b != 0, c != 0)) {
        case MappingStep::Lost: std::printf("lost\n"); break;
        case MappingStep::Dropped: std::printf("dropped\n"); break;
        case MappingStep::Update: std::printf("update\n"); break;
        case MappingStep::KeyframeChange: std::printf("change\n"); break;
      }
    } else if (!std::strcmp(op, "constants")) {
      std::printf("%d %d %g %g", InitializationPhaseCount, MinNumMapped, (double)KF_DIST_WEIGHT, (double)KF_USAGE_WEIGHT);
      for (int its : TRACKER_MAX_ITS_PER_LVL) std::printf(" %d", its);
      std::printf("\n");
    } else {
      return 2;
    }
  }
  std::printf("loop rules ok\n");
  return 0;
}
