// The host part of TrackableKeyFrameSearch::findRePositionCandidate (C/GlobalMapping/TrackableKeyFrameSearch.cpp:103-172) as pure
// functions over plain structs: the Euclidean prefilter (findEuclideanOverlapFrames, :56-98), the skips (:118-122), the score
// (getRefFrameScore, TrackableKeyFrameSearch.h:75-79) and the selection loop (:131-152) replayed over the results the device returned.
// Plain C++ without HIP headers: tests/cpp/reposition_plan_test.cpp checks it as a stand-alone program; tracker.hip puts the two
// launches between its stages (lsdhip_tracker_find_reposition_candidate).  Poses in double, scores in float, as the reference.
#pragma once
#include <cmath>
#include <vector>

#include "../../include/lsdhip.h"

namespace lsdrp {
constexpr int INITIALIZATION_PHASE_COUNT = 5;   // C/util/settings.h:172
constexpr float ANGLE_TH = 0.75f;               // findRePositionCandidate's angleTH (TrackableKeyFrameSearch.cpp:106)
constexpr float POSE_DISCREPANCY_TH = 0.2f;     // :143

struct Quat { double w, x, y, z; };
struct SE3 { Quat q; double t[3]; };
struct Sim3 { Quat q; double t[3]; double s; };   // p' = s R(q) p + t

inline Quat q_mul(const Quat& a, const Quat& b) {
  return {a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
          a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z, a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x};
}
inline Quat q_conj(const Quat& a) { return {a.w, -a.x, -a.y, -a.z}; }
inline Quat q_unit(const Quat& a) {
  const double n = std::sqrt(a.w * a.w + a.x * a.x + a.y * a.y + a.z * a.z);
  return {a.w / n, a.x / n, a.y / n, a.z / n};
}
inline void q_rotate(const Quat& q, const double v[3], double out[3]) {
  double ux = q.y * v[2] - q.z * v[1], uy = q.z * v[0] - q.x * v[2], uz = q.x * v[1] - q.y * v[0];
  ux += ux; uy += uy; uz += uz;
  out[0] = v[0] + q.w * ux + (q.y * uz - q.z * uy);
  out[1] = v[1] + q.w * uy + (q.z * ux - q.x * uz);
  out[2] = v[2] + q.w * uz + (q.x * uy - q.y * ux);
}
// third column of the rotation matrix: rotationMatrix().rightCols<1>() (TrackableKeyFrameSearch.cpp:64, :85)
inline void q_viewing_dir(const Quat& q, double out[3]) {
  const double z[3] = {0, 0, 1};
  q_rotate(q, z, out);
}
inline Sim3 sim3_from8(const double p[8]) {
  Sim3 S;
  S.q = q_unit({p[0], p[1], p[2], p[3]});
  S.t[0] = p[4]; S.t[1] = p[5]; S.t[2] = p[6];
  S.s = p[7];
  return S;
}
inline Sim3 sim3_inverse(const Sim3& S) {
  Sim3 r;
  r.q = q_conj(S.q);
  r.s = 1.0 / S.s;
  double rt[3];
  q_rotate(r.q, S.t, rt);
  for (int i = 0; i < 3; i++) r.t[i] = -(rt[i] * r.s);
  return r;
}
inline Sim3 sim3_mul(const Sim3& a, const Sim3& b) {
  Sim3 r;
  r.q = q_unit(q_mul(a.q, b.q));
  r.s = a.s * b.s;
  double rt[3];
  q_rotate(a.q, b.t, rt);
  for (int i = 0; i < 3; i++) r.t[i] = a.s * rt[i] + a.t[i];
  return r;
}
inline SE3 se3_from_sim3(const Sim3& S) { return SE3{S.q, {S.t[0], S.t[1], S.t[2]}}; }   // se3FromSim3 (C/util/SophusUtil.h:60-63)
inline SE3 se3_inverse(const SE3& T) {
  SE3 r;
  r.q = q_conj(T.q);
  const double nt[3] = {-T.t[0], -T.t[1], -T.t[2]};
  q_rotate(r.q, nt, r.t);
  return r;
}
inline SE3 se3_mul(const SE3& a, const SE3& b) {
  SE3 r;
  r.q = q_unit(q_mul(a.q, b.q));
  double rt[3];
  q_rotate(a.q, b.t, rt);
  for (int i = 0; i < 3; i++) r.t[i] = a.t[i] + rt[i];
  return r;
}
inline SE3 se3_from7(const double p[7]) { return SE3{q_unit({p[0], p[1], p[2], p[3]}), {p[4], p[5], p[6]}}; }
inline void se3_to7(const SE3& T, double p[7]) { p[0] = T.q.w; p[1] = T.q.x; p[2] = T.q.y; p[3] = T.q.z; p[4] = T.t[0]; p[5] = T.t[1]; p[6] = T.t[2]; }
// |log(T)| with Sophus' SE3Group::log (sophus/se3.hpp:559-586) over SO3Group::logAndTheta (so3.hpp:490-531): tangent (upsilon, omega)
inline double se3_log_norm(const SE3& T) {
  const double eps = 1e-10;
  const Quat& q = T.q;
  const double n2 = q.x * q.x + q.y * q.y + q.z * q.z, n = std::sqrt(n2), w = q.w;
  double k;   // two_atan_nbyw_by_n
  if (n < eps) k = 2.0 / w - 2.0 * n2 / (w * w * w);
  else if (std::fabs(w) < eps) k = (w > 0 ? M_PI : -M_PI) / n;
  else k = 2.0 * std::atan(n / w) / n;
  const double theta = k * n, o[3] = {k * q.x, k * q.y, k * q.z};
  // V^-1 t = t - 0.5 (o x t) + c (o x (o x t))
  const double c = std::fabs(theta) < eps ? 1.0 / 12.0 : (1.0 - theta / (2.0 * std::tan(theta / 2.0))) / (theta * theta);
  const double* t = T.t;
  const double a[3] = {o[1] * t[2] - o[2] * t[1], o[2] * t[0] - o[0] * t[2], o[0] * t[1] - o[1] * t[0]};
  const double b[3] = {o[1] * a[2] - o[2] * a[1], o[2] * a[0] - o[0] * a[2], o[0] * a[1] - o[1] * a[0]};
  double sum = o[0] * o[0] + o[1] * o[1] + o[2] * o[2];
  for (int i = 0; i < 3; i++) { const double u = t[i] - 0.5 * a[i] + c * b[i]; sum += u * u; }
  return std::sqrt(sum);
}

// one banked keyframe as the search reads it
struct Keyframe { int frameId; int numPoints; float meanIdepth; Sim3 camToWorld; };
struct Weights { float KFDistWeight, KFUsageWeight, relocalizationTH; };
// fowX / fowY of the constructor (TrackableKeyFrameSearch.cpp:37-38)
inline void field_of_view(int w, int h, float fx, float fy, float* fowX, float* fowY) {
  *fowX = 2 * atanf((float)((w / fx) / 2.0f));
  *fowY = 2 * atanf((float)((h / fy) / 2.0f));
}
// getRefFrameScore (TrackableKeyFrameSearch.h:75-79)
inline float ref_frame_score(float distanceSquared, float usage, const Weights& W) {
  return distanceSquared * W.KFDistWeight * W.KFDistWeight + (1 - usage) * (1 - usage) * W.KFUsageWeight * W.KFUsageWeight;
}

// Stages 1 and 2.  One record per keyframe, in slot order: stage = LSDHIP_REPO_FAR / _ANGLE / _PARENT / _INIT_PHASE / _EMPTY, or
// LSDHIP_REPO_SCORE for the survivors (their final stage is set by `select`).  Returns potentialReferenceFrames.size().
inline int prefilter(const std::vector<Keyframe>& kfs, const Sim3& frameCamToWorld, int trackingParentId, float maxScore, float fowX, float fowY,
                     const Weights& W, std::vector<lsdhip_reposition_record>* recs) {
  const float distanceTH = maxScore / (W.KFDistWeight * W.KFDistWeight);        // :106
  const float cosAngleTH = cosf(ANGLE_TH * 0.5f * (fowX + fowY));               // :60
  double viewingDir[3];
  q_viewing_dir(frameCamToWorld.q, viewingDir);
  recs->assign(kfs.size(), lsdhip_reposition_record());
  int potential = 0;
  for (size_t i = 0; i < kfs.size(); i++) {
    const Keyframe& kf = kfs[i];
    lsdhip_reposition_record& r = (*recs)[i];
    r = lsdhip_reposition_record();
    r.slot = (int)i;
    r.frameId = kf.frameId;
    for (int k = 0; k < 7; k++) r.refToFrame[k] = r.refToFrame_tracked[k] = k == 0 ? 1.0 : 0.0;
    const float distFac = (float)(kf.meanIdepth / kf.camToWorld.s);              // :79
    double d2 = 0;
    for (int k = 0; k < 3; k++) { const double d = (frameCamToWorld.t[k] - kf.camToWorld.t[k]) * distFac; d2 += d * d; }
    r.dist2 = (float)d2;
    r.stage = LSDHIP_REPO_FAR;
    if (r.dist2 > distanceTH) continue;                                          // :83
    double otherDir[3];
    q_viewing_dir(kf.camToWorld.q, otherDir);
    r.angle = (float)(otherDir[0] * viewingDir[0] + otherDir[1] * viewingDir[1] + otherDir[2] * viewingDir[2]);
    r.stage = LSDHIP_REPO_ANGLE;
    if (r.angle < cosAngleTH) continue;                                          // :87
    potential++;
    se3_to7(se3_inverse(se3_from_sim3(sim3_mul(sim3_inverse(kf.camToWorld), frameCamToWorld))), r.refToFrame);   // :91
    if (kf.frameId == trackingParentId) r.stage = LSDHIP_REPO_PARENT;            // :118
    else if ((int)i < INITIALIZATION_PHASE_COUNT) r.stage = LSDHIP_REPO_INIT_PHASE;   // :121
    else if (kf.numPoints <= 0) r.stage = LSDHIP_REPO_EMPTY;
    else r.stage = LSDHIP_REPO_SCORE;
  }
  return potential;
}
// Stage 3's verdict: the record's score from its usage (:131); true if the candidate is to be tracked (:133)
inline bool wants_tracking(lsdhip_reposition_record& r, float usage, float maxScore, const Weights& W) {
  r.usage = usage;
  r.score = ref_frame_score(r.dist2, usage, W);
  return r.score < maxScore;
}
// Stage 5: the loop body behind trackFrameOnPermaref (:136-152) for the tracked candidates, in candidate order.  tracked[k] / out[k]:
// record index and tracking result of the k-th tracked candidate.
inline void select(std::vector<lsdhip_reposition_record>& recs, const std::vector<Keyframe>& kfs, const std::vector<int>& tracked,
                   const lsdhip_track_result* out, float maxScore, const Weights& W, lsdhip_reposition_result* res) {
  float bestScore = maxScore, bestDist = 0, bestUsage = 0, bestPoseDiscrepancy = 0;
  int best = -1;
  for (size_t k = 0; k < tracked.size(); k++) {
    lsdhip_reposition_record& r = recs[(size_t)tracked[k]];
    const lsdhip_track_result& o = out[k];
    const SE3 trackedT = se3_from7(o.frameToReference);      // RefToFrame_tracked (the entry's result field carries referenceToFrame here)
    const double mi = kfs[(size_t)r.slot].meanIdepth;
    double d2 = 0;
    for (int i = 0; i < 3; i++) { const double d = trackedT.t[i] * mi; d2 += d * d; }
    r.usageTracked = o.pointUsage;
    r.newScore = ref_frame_score((float)d2, o.pointUsage, W);
    r.poseDiscrepancy = (float)se3_log_norm(se3_mul(se3_from7(r.refToFrame), se3_inverse(trackedT)));
    r.goodVal = o.pointUsage * o.lastGoodCount / (o.lastGoodCount + o.lastBadCount);
    r.trackingWasGood = o.trackingWasGood;
    r.diverged = o.diverged;
    for (int i = 0; i < 7; i++) r.refToFrame_tracked[i] = o.frameToReference[i];
    r.stage = LSDHIP_REPO_REJECTED;
    if (o.trackingWasGood && r.goodVal > W.relocalizationTH && r.newScore < bestScore && r.poseDiscrepancy < POSE_DISCREPANCY_TH) {
      r.stage = LSDHIP_REPO_TAKEN;
      bestPoseDiscrepancy = r.poseDiscrepancy;
      bestScore = r.score;            // the reference stores `score`, not `newScore` (:146)
      best = tracked[k];
      bestDist = (float)d2;
      bestUsage = o.pointUsage;
    }
  }
  res->slot = best >= 0 ? recs[(size_t)best].slot : -1;
  res->frameId = best >= 0 ? recs[(size_t)best].frameId : -1;
  res->numTracked = (int)tracked.size();
  res->bestScore = bestScore; res->bestDist = bestDist; res->bestUsage = bestUsage; res->bestPoseDiscrepancy = bestPoseDiscrepancy;
  for (int i = 0; i < 7; i++) {
    res->refToFrame[i] = best >= 0 ? recs[(size_t)best].refToFrame[i] : (i == 0 ? 1.0 : 0.0);
    res->refToFrame_tracked[i] = best >= 0 ? recs[(size_t)best].refToFrame_tracked[i] : (i == 0 ? 1.0 : 0.0);
  }
}
}  // namespace lsdrp
