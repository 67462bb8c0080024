// lsd_slam_hip_cloud_constants.hpp — the per-keyframe constants of the viewer's point-cloud export, computed in ONE place for both paths:
// flushPointCloud of lsd_slam_hip_io.hpp (host) and lsdhip_cloud_append_keyframe (liblsdhip computes them with this function before it
// launches).  Depends on <cmath> only, so that the library does not include the C++ wrapper of its own C ABI.
#ifndef LSD_SLAM_HIP_CLOUD_CONSTANTS_HPP
#define LSD_SLAM_HIP_CLOUD_CONSTANTS_HPP

#include <cmath>

namespace lsd_slam_hip {

// The per-keyframe constants of flushPC (V/KeyFrameDisplay.cpp:276-283 and the Sim3 it transforms by): inverse intrinsics, and camToWorld —
// rotation-and-scale quaternion (x y z w) + translation — split into scale, unit quaternion and translation.  The host loop below and the
// device append (lsdhip_cloud_append_keyframe, which calls this function inside the library) both take them from here.
struct CloudConstants {
  float fxi, fyi, cxi, cyi, scale, ux, uy, uz, uw, tx, ty, tz;
};
inline CloudConstants cloudConstants(float fx, float fy, float cx, float cy, const float camToWorld[7]) {
  CloudConstants k;
  k.fxi = 1 / fx; k.fyi = 1 / fy; k.cxi = -cx / fx; k.cyi = -cy / fy;
  const float qx = camToWorld[0], qy = camToWorld[1], qz = camToWorld[2], qw = camToWorld[3];
  const float n = std::sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
  k.scale = n;
  k.ux = qx / n; k.uy = qy / n; k.uz = qz / n; k.uw = qw / n;
  k.tx = camToWorld[4]; k.ty = camToWorld[5]; k.tz = camToWorld[6];
  return k;
}

}  // namespace lsd_slam_hip
#endif
