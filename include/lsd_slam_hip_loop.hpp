// The per-frame decisions of SlamSystem for ONE sequence, as the loops of lsd_slam_hip.hpp (SlamLoop, SlamLoopBatch) restate them: what
// follows a tracking result, and when a tracked frame becomes the next keyframe.  Pure decisions on plain numbers: no device code, no
// library call, nothing of lsdhip.h.  tests/cpp/loop_rules_test.cpp holds every rule to a table written from the reference.
#pragma once
#include <cmath>

namespace lsd_slam {
namespace loop {

// INITIALIZATION_PHASE_COUNT and MIN_NUM_MAPPED of the reference (util/settings.h:172, :174).  They are macros there, and the integration
// layer includes this header beside that one: hence the other spelling.
constexpr int InitializationPhaseCount = 5;
constexpr int MinNumMapped = 5;
constexpr float KF_DIST_WEIGHT = 4;             // KFDistWeight, util/settings.cpp:77
constexpr float KF_USAGE_WEIGHT = 3;            // KFUsageWeight, util/settings.cpp:78
// SE3Tracker iterations per pyramid level as SlamSystem sets them (SlamSystem.cpp:80-81); the tracker runs none at level 4
constexpr int TRACKER_MAX_ITS_PER_LVL[5] = {5, 20, 50, 100, 0};

// SlamSystem::trackFrame (SlamSystem.cpp:946-966): tracking is lost when the tracker diverged, or — once the initialisation phase is
// over (more than INITIALIZATION_PHASE_COUNT keyframes in the graph) — when trackingWasGood is false.  The frame is then neither mapped
// nor promoted.
inline bool trackingLost(bool diverged, bool trackingWasGood, int numKeyframesFinished) {
  return diverged || (numKeyframesFinished > InitializationPhaseCount && !trackingWasGood);
}
// doMappingIteration's lost branch (SlamSystem.cpp:809-817): the current keyframe is finalised if it has been mapped on at least
// MIN_NUM_MAPPED times and discarded (discardCurrentKeyframe, :428-456) otherwise; the map is invalidated either way.
inline bool finaliseOnLoss(int mappedOnKF) { return mappedOnKF >= MinNumMapped; }

// TrackableKeyFrameSearch::getRefFrameScore (GlobalMapping/TrackableKeyFrameSearch.h:75-79)
inline float keyframeScore(float distanceSquared, float usage, float distWeight = KF_DIST_WEIGHT, float usageWeight = KF_USAGE_WEIGHT) {
  return distanceSquared * distWeight * distWeight + (1 - usage) * (1 - usage) * usageWeight * usageWeight;
}
// minVal of SlamSystem.cpp:997-1015 for a graph of numKeyframes keyframes (a loop that keeps its finished keyframes: the bank's size)
inline float scoreThreshold(int numKeyframes) {
  float minVal = std::fmin(0.2f + numKeyframes * 0.8f / InitializationPhaseCount, 1.0f);
  if (numKeyframes < InitializationPhaseCount) minVal = (float)(minVal * 0.7);
  return minVal;
}
// ... and for a loop that keeps none: keyframesAll stays empty (SURVEY.md §8(d) driver notes), the product taken in single precision
inline float scoreThreshold() { return 0.2f * 0.7f; }

// A new keyframe every kfEvery > 0 tracked frames, dropped ones included: the deterministic policy of the benchmark and the parity tests
inline bool wantsNewKeyframe(int kfEvery, int sinceKF) { return kfEvery > 0 && sinceKF >= kfEvery; }
// The reference's rule (SlamSystem.cpp:997-1015): only a keyframe mapped on more than MIN_NUM_MAPPED times is left, and only for a
// frame whose score exceeds the threshold
inline bool scoreRuleApplies(int mappedOnKF) { return mappedOnKF > MinNumMapped; }
inline bool wantsNewKeyframe(int mappedOnKF, float score, float threshold) { return scoreRuleApplies(mappedOnKF) && score > threshold; }

// The mapping step a tracked frame leads to (SlamSystem::doMappingIteration, SlamSystem.cpp:739-828)
enum class MappingStep {
  Lost,            // trackingLost: nothing is mapped, the map is given up (:809-817)
  Dropped,         // tracked on a keyframe the mapper has replaced since: updateKeyframe pops it unmapped (:559-566)
  Update,          // updateKeyframe with this frame (:542-614)
  KeyframeChange   // finishCurrentKeyframe + changeKeyframe (:783-791)
};
inline MappingStep mappingStep(bool lost, bool trackedOnCurrentKeyframe, bool wantsKeyframe) {
  if (lost) return MappingStep::Lost;
  if (!trackedOnCurrentKeyframe) return MappingStep::Dropped;
  return wantsKeyframe ? MappingStep::KeyframeChange : MappingStep::Update;
}

}  // namespace loop
}  // namespace lsd_slam
