// World poses of keyframes and frames on the host, in double as the reference keeps them (FramePoseStruct::getCamToWorld,
// DataStructures/FramePoseStruct.cpp:84-104: camToWorld = parent's camToWorld * thisToParent_raw, the identity without a parent).
// Plain C++, no device code and no library call: the loops of lsd_slam_hip.hpp chain poses with it, tests/cpp/pose_chain_test.cpp holds
// it to float64 products.
//
// A Sim3 is 8 doubles (qw, qx, qy, qz, tx, ty, tz, s) with a unit quaternion — the layout of lsdhip_frame_get_pose and of the keyframe
// bank's metadata — and acts on a point as x -> s R x + t.  An SE3 is its first 7.
#pragma once
#include <cmath>

namespace lsd_slam {
namespace pose {

inline void quat_mul(const double a[4], const double b[4], double out[4]) {
  const double w = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  const double x = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  const double y = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  const double z = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
  out[0] = w; out[1] = x; out[2] = y; out[3] = z;
}
inline void quat_normalize(double q[4]) {
  const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int i = 0; i < 4; i++) q[i] /= n;
}
// R(q) v for a unit quaternion, through the rotation matrix
inline void quat_rotate(const double q[4], const double v[3], double out[3]) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double r00 = 1 - 2 * (y * y + z * z), r01 = 2 * (x * y - w * z), r02 = 2 * (x * z + w * y);
  const double r10 = 2 * (x * y + w * z), r11 = 1 - 2 * (x * x + z * z), r12 = 2 * (y * z - w * x);
  const double r20 = 2 * (x * z - w * y), r21 = 2 * (y * z + w * x), r22 = 1 - 2 * (x * x + y * y);
  const double a = r00 * v[0] + r01 * v[1] + r02 * v[2];
  const double b = r10 * v[0] + r11 * v[1] + r12 * v[2];
  const double c = r20 * v[0] + r21 * v[1] + r22 * v[2];
  out[0] = a; out[1] = b; out[2] = c;
}
inline void sim3_identity(double out[8]) {
  out[0] = 1; out[1] = out[2] = out[3] = 0; out[4] = out[5] = out[6] = 0; out[7] = 1;
}
// out = a * b (first b, then a); out may be a or b
inline void sim3_mul(const double a[8], const double b[8], double out[8]) {
  double q[4], rt[3];
  quat_mul(a, b, q);
  quat_normalize(q);
  quat_rotate(a, b + 4, rt);
  const double t0 = a[7] * rt[0] + a[4], t1 = a[7] * rt[1] + a[5], t2 = a[7] * rt[2] + a[6];
  const double s = a[7] * b[7];
  out[0] = q[0]; out[1] = q[1]; out[2] = q[2]; out[3] = q[3];
  out[4] = t0; out[5] = t1; out[6] = t2; out[7] = s;
}
// out = a^-1; out may be a
inline void sim3_inv(const double a[8], double out[8]) {
  const double qi[4] = {a[0], -a[1], -a[2], -a[3]};
  const double si = 1.0 / a[7];
  double rt[3];
  quat_rotate(qi, a + 4, rt);
  out[0] = qi[0]; out[1] = qi[1]; out[2] = qi[2]; out[3] = qi[3];
  out[4] = -si * rt[0]; out[5] = -si * rt[1]; out[6] = -si * rt[2]; out[7] = si;
}
// sim3FromSE3(se3, scale) (util/SophusUtil.h:53-58)
inline void sim3_from_se3(const double se3[7], double scale, double out[8]) {
  for (int i = 0; i < 7; i++) out[i] = se3[i];
  out[7] = scale;
}
// se3FromSim3 (util/SophusUtil.h:60-63): rotation and translation, the scale dropped
inline void se3_from_sim3(const double a[8], double out[7]) {
  for (int i = 0; i < 7; i++) out[i] = a[i];
}
// se3FromSim3(reference^-1 * frame) (SlamSystem.cpp:922-925): where `frame` stands seen from `reference`, both given by their camToWorld
inline void relative_se3(const double referenceCamToWorld[8], const double frameCamToWorld[8], double out[7]) {
  double inv[8], rel[8];
  sim3_inv(referenceCamToWorld, inv);
  sim3_mul(inv, frameCamToWorld, rel);
  se3_from_sim3(rel, out);
}

}  // namespace pose
}  // namespace lsd_slam
