// lsd_slam_hip.hpp — header-only C++ host side above the C ABI (include/lsdhip.h).
//
// The reference's boundary for this path is a C++ class API; these classes put the reference's
// signatures back on top of liblsdhip.so so that SlamSystem-style callers read the same:
//
//   reference (lsd_slam_core/src/…)                         here (namespace lsd_slam_hip)
//   Frame(int id,int w,int h,const Eigen::Matrix3f& K,       Frame(int id,int w,int h,const Mat3f& K,double ts,
//         double timestamp,const unsigned char* image)            const unsigned char* image)
//                              DataStructures/Frame.h:43
//   TrackingReference::importFrame(Frame*)                  TrackingReference::importFrame(Frame*)
//                              Tracking/TrackingReference.h:49
//   SE3Tracker(int w,int h,Eigen::Matrix3f K)               SE3Tracker(int w,int h,const Mat3f& K)
//   SE3 trackFrame(TrackingReference*,Frame*,const SE3&)    SE3 trackFrame(TrackingReference*,Frame*,const SE3&)
//   SE3 trackFrameOnPermaref(Frame*,Frame*,SE3)             SE3 trackFrameOnPermaref(Frame*,Frame*,SE3)
//   float checkPermaRefOverlap(Frame*,SE3)                  float checkPermaRefOverlap(Frame*,SE3)
//                              Tracking/SE3Tracker.h:41-93
//   DepthMap(int w,int h,const Eigen::Matrix3f& K)          DepthMap(int w,int h,const Mat3f& K)
//   updateKeyframe(std::deque<std::shared_ptr<Frame>>)      updateKeyframe(std::deque<std::shared_ptr<Frame>>)
//   createKeyFrame(Frame*) / finalizeKeyFrame() / …         same names
//                              DepthEstimation/DepthMap.h:47-98
//
// Only the value types differ: Eigen / Sophus are not part of this repository, so Mat3f and SE3 / Sim3 are plain
// structs with the same content (row-major 3x3; unit quaternion + translation [+ scale], what Sophus::SE3d / Sim3d
// store).  INTEGRATION.md shows the two-line conversions a lsd_slam_core build adds.
//
// Error behaviour: the reference asserts on misuse and reports divergence through flags.  Here divergence is reported
// the same way (diverged = true, identity returned); usage / runtime errors of the C ABI (negative status) throw
// lsd_slam_hip::Error carrying lsdhip_last_error().  Nothing is computed on the host: without liblsdhip.so and a GPU
// every call fails loudly.
#ifndef LSD_SLAM_HIP_HPP
#define LSD_SLAM_HIP_HPP

#include <array>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <deque>
#include <exception>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "lsdhip.h"
#include "lsd_slam_hip_loop.hpp"
#include "lsd_slam_hip_pose.hpp"

namespace lsd_slam_hip {

struct Error : std::runtime_error {
  int status;
  Error(int st, const std::string& what) : std::runtime_error(what), status(st) {}
};
inline int check(int rc, const char* where) {
  if (rc < 0) throw Error(rc, std::string(where) + ": " + lsdhip_last_error());
  return rc;
}

struct Mat3f {
  float m[9];  // row-major
  float fx() const { return m[0]; }
  float fy() const { return m[4]; }
  float cx() const { return m[2]; }
  float cy() const { return m[5]; }
  static Mat3f intrinsics(float fx, float fy, float cx, float cy) { return Mat3f{{fx, 0, cx, 0, fy, cy, 0, 0, 1}}; }
};

// Sophus::SE3d content: unit quaternion (w,x,y,z) + translation
struct SE3 {
  double q[4] = {1, 0, 0, 0};
  double t[3] = {0, 0, 0};
  void to7(double p[7]) const { for (int i = 0; i < 4; i++) p[i] = q[i]; for (int i = 0; i < 3; i++) p[4 + i] = t[i]; }
  static SE3 from7(const double p[7]) { SE3 r; for (int i = 0; i < 4; i++) r.q[i] = p[i]; for (int i = 0; i < 3; i++) r.t[i] = p[4 + i]; return r; }
};
// Sophus::Sim3d content
struct Sim3 {
  double q[4] = {1, 0, 0, 0};
  double t[3] = {0, 0, 0};
  double s = 1;
  static Sim3 from8(const double p[8]) { Sim3 r; for (int i = 0; i < 4; i++) r.q[i] = p[i]; for (int i = 0; i < 3; i++) r.t[i] = p[4 + i]; r.s = p[7]; return r; }
};

// One device context per (device, w, h, K): what the (w, h, K) constructor arguments of Frame / SE3Tracker / DepthMap
// share in the reference.  Objects created with the same arguments use the same context and therefore the same stream.
class Context {
 public:
  static std::shared_ptr<Context> get(int w, int h, const Mat3f& K, int device = defaultDevice()) {
    static std::mutex mu;
    static std::map<std::tuple<int, int, int, float, float, float, float>, std::weak_ptr<Context>> registry;
    std::lock_guard<std::mutex> lock(mu);
    auto key = std::make_tuple(device, w, h, K.fx(), K.fy(), K.cx(), K.cy());
    if (auto sp = registry[key].lock()) return sp;
    std::shared_ptr<Context> sp(new Context(device, w, h, K));
    registry[key] = sp;
    return sp;
  }
  static int& defaultDevice() { static int d = 0; return d; }
  ~Context() { lsdhip_ctx_destroy(h_); }
  lsdhip_ctx* handle() const { return h_; }
  int width() const { return w_; }
  int height() const { return h_px_; }
  const Mat3f& K() const { return K_; }
  lsdhip_params params;  // the hot-path globals of util/settings.cpp:77-88 this context was created with
  void synchronize() { check(lsdhip_ctx_synchronize(h_), "lsdhip_ctx_synchronize"); }
  // mapping calls return after enqueueing; host-side results are picked up lazily (lsdhip.h: lsdhip_ctx_set_async)
  void setAsync(bool on) { check(lsdhip_ctx_set_async(h_, on ? 1 : 0), "lsdhip_ctx_set_async"); }
  // tracking stream beside mapping stream (lsdhip.h: lsdhip_ctx_set_pipeline): the reference's two threads, blockUntilMapped == false
  void setPipeline(bool on) { check(lsdhip_ctx_set_pipeline(h_, on ? 1 : 0), "lsdhip_ctx_set_pipeline"); }
  // lanes: DepthMap call chains of different maps side by side (lsdhip.h: lsdhip_ctx_lanes_begin)
  void lanesBegin(int n) { check(lsdhip_ctx_lanes_begin(h_, n), "lsdhip_ctx_lanes_begin"); }
  void laneSelect(int lane) { check(lsdhip_ctx_lane_select(h_, lane), "lsdhip_ctx_lane_select"); }
  void lanesEnd() { check(lsdhip_ctx_lanes_end(h_), "lsdhip_ctx_lanes_end"); }
  bool pipeline() const { return lsdhip_ctx_pipeline(h_) == 1; }

 private:
  Context(int device, int w, int h, const Mat3f& K) : w_(w), h_px_(h), K_(K) {
    lsdhip_default_params(&params);
    const float k4[4] = {K.fx(), K.fy(), K.cx(), K.cy()};
    check(lsdhip_ctx_create(device, w, h, k4, &params, &h_), "lsdhip_ctx_create");
  }
  lsdhip_ctx* h_ = nullptr;
  int w_, h_px_;
  Mat3f K_;
};

class TrackingReference;

// util/Undistorter.h — UndistorterPTAM's remap tables on the device (lsdhip_undistorter_*), bound to the Context of the OUTPUT size and
// K: one camera serves every frame and loop of that context.  The tables come from lsd_slam_hip::Undistorter (lsd_slam_hip_io.hpp):
//   Undistorter u = Undistorter::fromFile("camera.cfg");
//   DeviceUndistorter d(u.in_width, u.in_height, u.out_width, u.out_height, u.K, u.remapX.data(), u.remapY.data());
// A pass-through calibration (no tables) needs none: its images are the rectified ones.
class DeviceUndistorter {
 public:
  DeviceUndistorter(int inWidth, int inHeight, int width, int height, const Mat3f& K, const float* remapX, const float* remapY)
      : ctx_(Context::get(width, height, K)), inW_(inWidth), inH_(inHeight) {
    check(lsdhip_undistorter_create(ctx_->handle(), inWidth, inHeight, remapX, remapY, &h_), "lsdhip_undistorter_create");
  }
  DeviceUndistorter(const DeviceUndistorter&) = delete;
  DeviceUndistorter& operator=(const DeviceUndistorter&) = delete;
  ~DeviceUndistorter() { lsdhip_undistorter_destroy(h_); }
  // UndistorterPTAM::undistort: inWidth * inHeight raw bytes -> width * height rectified bytes, either side on the host or the device
  void undistort(const unsigned char* raw, bool rawOnDevice, unsigned char* out, bool outOnDevice) const {
    check(lsdhip_undistorter_apply(h_, raw, rawOnDevice ? 1 : 0, out, outOnDevice ? 1 : 0), "lsdhip_undistorter_apply");
  }
  int inputWidth() const { return inW_; }
  int inputHeight() const { return inH_; }
  int width() const { return ctx_->width(); }
  int height() const { return ctx_->height(); }
  const Mat3f& K() const { return ctx_->K(); }
  lsdhip_undistorter* handle() const { return h_; }
  const std::shared_ptr<Context>& context() const { return ctx_; }

 private:
  std::shared_ptr<Context> ctx_;
  lsdhip_undistorter* h_ = nullptr;
  int inW_, inH_;
};

// DataStructures/Frame.h — a frame whose pyramids live on the device
class Frame {
 public:
  Frame(int id, int width, int height, const Mat3f& K, double timestamp, const unsigned char* image)
      : ctx_(Context::get(width, height, K)), id_(id), timestamp_(timestamp) {
    check(lsdhip_frame_create(ctx_->handle(), id, image, &h_), "lsdhip_frame_create");
  }
  // image already resident on the context's GPU (uint8, w*h): no PCIe transfer
  struct DeviceImage { const unsigned char* ptr; };
  Frame(int id, int width, int height, const Mat3f& K, double timestamp, DeviceImage image)
      : ctx_(Context::get(width, height, K)), id_(id), timestamp_(timestamp) {
    check(lsdhip_frame_create_from_device(ctx_->handle(), id, image.ptr, &h_), "lsdhip_frame_create_from_device");
  }
  // host image whose bytes stay unchanged until the frame has been tracked (or the context synchronised): upload and pyramids are
  // queued, nothing waits (lsdhip_frame_create_async)
  struct HostImageAsync { const unsigned char* ptr; };
  Frame(int id, int width, int height, const Mat3f& K, double timestamp, HostImageAsync image)
      : ctx_(Context::get(width, height, K)), id_(id), timestamp_(timestamp) {
    check(lsdhip_frame_create_async(ctx_->handle(), id, image.ptr, &h_), "lsdhip_frame_create_async");
  }
  // Raw camera images (inputWidth * inputHeight bytes of the undistorter's camera), rectified inside frame creation
  // (lsdhip_frame_create_undistorted*): host memory, device memory, host memory without the wait — as the three forms above.
  struct RawImage { const unsigned char* ptr; };
  struct RawDeviceImage { const unsigned char* ptr; };
  struct RawHostImageAsync { const unsigned char* ptr; };
  Frame(int id, const DeviceUndistorter& undistorter, double timestamp, RawImage image)
      : ctx_(undistorter.context()), id_(id), timestamp_(timestamp) {
    check(lsdhip_frame_create_undistorted(undistorter.handle(), id, image.ptr, &h_), "lsdhip_frame_create_undistorted");
  }
  Frame(int id, const DeviceUndistorter& undistorter, double timestamp, RawDeviceImage image)
      : ctx_(undistorter.context()), id_(id), timestamp_(timestamp) {
    check(lsdhip_frame_create_undistorted_from_device(undistorter.handle(), id, image.ptr, &h_), "lsdhip_frame_create_undistorted_from_device");
  }
  Frame(int id, const DeviceUndistorter& undistorter, double timestamp, RawHostImageAsync image)
      : ctx_(undistorter.context()), id_(id), timestamp_(timestamp) {
    check(lsdhip_frame_create_undistorted_async(undistorter.handle(), id, image.ptr, &h_), "lsdhip_frame_create_undistorted_async");
  }
  Frame(const Frame&) = delete;
  Frame& operator=(const Frame&) = delete;
  ~Frame() { lsdhip_frame_destroy(h_); }
  // ... from raw images of the undistorter's camera (lsdhip_frame_create_undistorted_batch)
  static std::vector<std::shared_ptr<Frame>> createBatch(const DeviceUndistorter& undistorter, const std::vector<int>& ids,
                                                         const unsigned char* const* rawImages, bool imagesOnDevice) {
    const int n = (int)ids.size();
    std::vector<lsdhip_frame*> hs((size_t)n, nullptr);
    check(lsdhip_frame_create_undistorted_batch(undistorter.handle(), n, ids.data(), rawImages, imagesOnDevice ? 1 : 0, hs.data()),
          "lsdhip_frame_create_undistorted_batch");
    std::vector<std::shared_ptr<Frame>> out;
    out.reserve((size_t)n);
    for (int j = 0; j < n; j++) out.push_back(std::shared_ptr<Frame>(new Frame(undistorter.context(), ids[j], hs[j])));
    return out;
  }
  // the new frames of n sequences (one context) in two launches instead of two per frame (lsdhip_frame_create_batch)
  static std::vector<std::shared_ptr<Frame>> createBatch(int width, int height, const Mat3f& K, const std::vector<int>& ids,
                                                         const unsigned char* const* images, bool imagesOnDevice) {
    std::shared_ptr<Context> ctx = Context::get(width, height, K);
    const int n = (int)ids.size();
    std::vector<lsdhip_frame*> hs((size_t)n, nullptr);
    check(lsdhip_frame_create_batch(ctx->handle(), n, ids.data(), images, imagesOnDevice ? 1 : 0, hs.data()), "lsdhip_frame_create_batch");
    std::vector<std::shared_ptr<Frame>> out;
    out.reserve((size_t)n);
    for (int j = 0; j < n; j++) out.push_back(std::shared_ptr<Frame>(new Frame(ctx, ids[j], hs[j])));
    return out;
  }

  int id() const { return id_; }
  int width(int level = 0) const { return ctx_->width() >> level; }
  int height(int level = 0) const { return ctx_->height() >> level; }
  double timestamp() const { return timestamp_; }
  lsdhip_frame* handle() const { return h_; }
  const std::shared_ptr<Context>& context() const { return ctx_; }

  // Frame::image / gradients / maxGradients / idepth / idepthVar (Frame.h:357-418), copied to the host
  std::vector<float> image(int level = 0) const { return plane(0, level, 1); }
  std::vector<float> gradients(int level = 0) const { return plane(1, level, 4); }
  std::vector<float> maxGradients(int level = 0) const { return plane(2, level, 1); }
  std::vector<float> idepth(int level = 0) const { return plane(3, level, 1); }
  std::vector<float> idepthVar(int level = 0) const { return plane(4, level, 1); }

  void setDepthFromGroundTruth(const float* depth, float cov_scale = 1.0f) {
    check(lsdhip_frame_set_depth_gt(h_, depth, cov_scale), "lsdhip_frame_set_depth_gt");
  }
  // refPixelWasGood() (Frame.h:421-437): empty vector when the mask does not exist
  std::vector<uint8_t> refPixelWasGoodNoCreate() const {
    std::vector<uint8_t> m((size_t)width(1) * height(1));
    if (check(lsdhip_frame_get_wasgood(h_, m.data()), "lsdhip_frame_get_wasgood") != 1) m.clear();
    return m;
  }
  void clear_refPixelWasGood() { check(lsdhip_frame_clear_wasgood(h_), "lsdhip_frame_clear_wasgood"); }

  // FramePoseStruct::thisToParent_raw / trackingParent (written by trackFrame; settable for callers that track elsewhere)
  Sim3 thisToParent_raw() const {
    double p[8];
    check(lsdhip_frame_get_pose(h_, p), "lsdhip_frame_get_pose");
    Sim3 s;
    for (int i = 0; i < 4; i++) s.q[i] = p[i];
    for (int i = 0; i < 3; i++) s.t[i] = p[4 + i];
    s.s = p[7];
    return s;
  }
  void setPose(const Sim3& thisToParent, Frame* trackingParent, float initialTrackedResidual) {
    const double p[8] = {thisToParent.q[0], thisToParent.q[1], thisToParent.q[2], thisToParent.q[3],
                         thisToParent.t[0], thisToParent.t[1], thisToParent.t[2], thisToParent.s};
    check(lsdhip_frame_set_pose(h_, p, trackingParent ? trackingParent->h_ : nullptr, initialTrackedResidual), "lsdhip_frame_set_pose");
  }

  struct Stats {
    float initialTrackedResidual, meanIdepth;
    int numPoints, numFramesTrackedOnThis, numMappedOnThis, numMappedOnThisTotal;
    bool depthHasBeenUpdatedFlag;
  };
  Stats stats() const {
    float o[8];
    check(lsdhip_frame_stats(h_, o), "lsdhip_frame_stats");
    return Stats{o[0], o[1], (int)o[2], (int)o[3], (int)o[4], (int)o[5], o[6] != 0.0f};
  }
  float initialTrackedResidual() const { return stats().initialTrackedResidual; }
  float meanIdepth() const { return stats().meanIdepth; }
  int numPoints() const { return stats().numPoints; }
  bool depthHasBeenUpdatedFlag() const { return check(lsdhip_frame_depth_updated(h_), "lsdhip_frame_depth_updated") != 0; }
  // currentKeyFrame->depthHasBeenUpdatedFlag = false (SlamSystem.cpp:910)
  void clearDepthHasBeenUpdatedFlag() { check(lsdhip_frame_clear_depth_updated(h_), "lsdhip_frame_clear_depth_updated"); }

  // Frame::setPermaRef (Frame.cpp:149-174): keeps the level-QUICK_KF_CHECK_LVL point cloud of `reference` on the host
  inline void setPermaRef(TrackingReference* reference);
  std::vector<float> permaRef_posData;       // 3 floats per point
  std::vector<float> permaRef_colorAndVarData;  // 2 floats per point
  int permaRefNumPts = 0;
  int idxInKeyframes = -1;   // Frame.h:203: position in the keyframe graph = the frame's slot in a KeyFrameBank (set by KeyFrameBank::put)

 private:
  std::vector<float> plane(int what, int level, int channels) const {
    std::vector<float> v((size_t)width(level) * height(level) * channels);
    check(lsdhip_frame_download(h_, what, level, v.data()), "lsdhip_frame_download");
    return v;
  }
  Frame(std::shared_ptr<Context> ctx, int id, lsdhip_frame* adopted) : ctx_(std::move(ctx)), h_(adopted), id_(id), timestamp_(0.0) {}
  std::shared_ptr<Context> ctx_;
  lsdhip_frame* h_ = nullptr;
  int id_;
  double timestamp_;
};

// The vendored Sophus stores a Sim3 as a non-unit quaternion (x, y, z, w) whose norm is the scale (thirdparty/Sophus/
// sophus/rxso3.hpp:311-313), followed by the translation (sim3.hpp:740-754); ROSOutput3DWrapper memcpys those 7 floats.
inline void sim3ToWire(const Sim3& T, float out[7]) {
  const double r = T.s;
  out[0] = (float)(T.q[1] * r); out[1] = (float)(T.q[2] * r); out[2] = (float)(T.q[3] * r); out[3] = (float)(T.q[0] * r);
  out[4] = (float)T.t[0]; out[5] = (float)T.t[1]; out[6] = (float)T.t[2];
}

// The viewer's accumulated point cloud (KeyFrameDisplay::flushPC per keyframe, lsd_slam_viewer/src/KeyFrameDisplay.cpp:269-340) in device
// memory: appendKeyframe queues the filter + back-projection + ordered compaction of one finalised keyframe on the context's mapping
// stream and returns; nothing waits until total() / stored() / segments() / download() ask.  Points are (x, y, z, intensity), in row-major
// pixel order within a keyframe, keyframes in call order; equal bit for bit to flushPointCloud of lsd_slam_hip_io.hpp on the same planes.
// Points beyond `capacityPoints` are counted (total()) but not stored; keyframes beyond `maxKeyframes` get no segment row.
class PointCloud {
 public:
  struct Segment { int id; int64_t first; int count; };
  PointCloud(std::shared_ptr<Context> ctx, int64_t capacityPoints, int maxKeyframes) : ctx_(std::move(ctx)) {
    check(lsdhip_cloud_create(ctx_->handle(), capacityPoints, maxKeyframes, &h_), "lsdhip_cloud_create");
  }
  PointCloud(const PointCloud&) = delete;
  PointCloud& operator=(const PointCloud&) = delete;
  ~PointCloud() { lsdhip_cloud_destroy(h_); }
  // the viewer's defaults (lsd_slam_viewer/src/settings.cpp:36-40); false once the segment table is full.  `kf` may be dropped right after the call.
  bool appendKeyframe(Frame& kf, const Sim3& camToWorld, float scaledTH = 1.f, float absTH = 1.f, int minNearSupport = 5) {
    float wire[7];
    sim3ToWire(camToWorld, wire);
    return check(lsdhip_cloud_append_keyframe(h_, kf.handle(), wire, scaledTH, absTH, minNearSupport), "lsdhip_cloud_append_keyframe") != LSDHIP_CLOUD_TABLE_FULL;
  }
  // n keyframes into n different clouds of one context in the launches of one (lsdhip_cloud_append_batch)
  static void appendBatch(const std::vector<PointCloud*>& clouds, const std::vector<Frame*>& kfs, const std::vector<Sim3>& camToWorld,
                          float scaledTH = 1.f, float absTH = 1.f, int minNearSupport = 5) {
    const size_t n = clouds.size();
    if (n == 0) return;
    if (kfs.size() != n || camToWorld.size() != n) throw Error(LSDHIP_E_ARG, "PointCloud::appendBatch: one frame and one pose per cloud");
    std::vector<lsdhip_cloud*> cs(n);
    std::vector<lsdhip_frame*> fs(n);
    std::vector<float> poses(7 * n);
    for (size_t j = 0; j < n; j++) { cs[j] = clouds[j]->h_; fs[j] = kfs[j]->handle(); sim3ToWire(camToWorld[j], &poses[7 * j]); }
    check(lsdhip_cloud_append_batch(clouds[0]->ctx_->handle(), (int)n, cs.data(), fs.data(), poses.data(), scaledTH, absTH, minNearSupport),
          "lsdhip_cloud_append_batch");
  }
  int64_t total() const { int64_t t = 0, s = 0; check(lsdhip_cloud_count(h_, &t, &s), "lsdhip_cloud_count"); return t; }
  int64_t stored() const { int64_t t = 0, s = 0; check(lsdhip_cloud_count(h_, &t, &s), "lsdhip_cloud_count"); return s; }
  std::vector<Segment> segments() const {
    int n = 0;
    check(lsdhip_cloud_segments(h_, 0, nullptr, nullptr, nullptr, &n), "lsdhip_cloud_segments");
    std::vector<int> ids((size_t)n), cnt((size_t)n);
    std::vector<int64_t> first((size_t)n);
    int n2 = 0;
    check(lsdhip_cloud_segments(h_, n, ids.data(), first.data(), cnt.data(), &n2), "lsdhip_cloud_segments");
    std::vector<Segment> out;
    for (int i = 0; i < n && i < n2; i++) out.push_back(Segment{ids[(size_t)i], first[(size_t)i], cnt[(size_t)i]});
    return out;
  }
  // stored points [first, first + n) as x y z intensity; n < 0: all from `first`
  std::vector<float> download(int64_t first = 0, int64_t n = -1) const {
    if (n < 0) { n = stored() - first; if (n < 0) n = 0; }
    std::vector<float> v((size_t)n * 4);
    check(lsdhip_cloud_download(h_, first, n, v.data()), "lsdhip_cloud_download");
    return v;
  }
  void reset() { check(lsdhip_cloud_reset(h_), "lsdhip_cloud_reset"); }
  lsdhip_cloud* handle() const { return h_; }

 private:
  std::shared_ptr<Context> ctx_;
  lsdhip_cloud* h_ = nullptr;
};

// Tracking/TrackingReference.h — on the device the point cloud is generated inside the residual kernel, so this object
// only remembers which keyframe it refers to; makePointCloud() exports the compacted arrays in the reference's order.
class TrackingReference {
 public:
  Frame* keyframe = nullptr;
  int frameID = -1;
  // TrackingReference.cpp:71-87.  The reference's object is a snapshot of the keyframe's depth taken here (lazily, at the next
  // trackFrame); on a pipelined context this is the moment the mapping side's newest Frame::setDepth result is handed to the tracker
  // (lsdhip_frame_publish_depth) — until then SE3Tracker jobs keep reading the planes of the previous import.
  void importFrame(Frame* source) {
    keyframe = source;
    frameID = source ? source->id() : -1;
    if (source) check(lsdhip_frame_publish_depth(source->handle()), "lsdhip_frame_publish_depth");
  }
  void invalidate() { keyframe = nullptr; frameID = -1; }
  // returns the number of points; any output may be null (TrackingReference.cpp:96-147)
  int makePointCloud(int level, std::vector<float>* posData, std::vector<float>* colorAndVarData,
                     std::vector<float>* gradData = nullptr, std::vector<int>* pointPosInXYGrid = nullptr) const {
    if (!keyframe) throw Error(LSDHIP_E_STATE, "TrackingReference::makePointCloud: no keyframe");
    const size_t cap = (size_t)keyframe->width(level) * keyframe->height(level);
    std::vector<float> pos(cap * 3), cv(cap * 2), gr(cap * 2);
    std::vector<int> idx(cap);
    const int n = check(lsdhip_ref_pointcloud(keyframe->handle(), level, pos.data(), cv.data(), gr.data(), idx.data()), "lsdhip_ref_pointcloud");
    if (posData) posData->assign(pos.begin(), pos.begin() + (size_t)n * 3);
    if (colorAndVarData) colorAndVarData->assign(cv.begin(), cv.begin() + (size_t)n * 2);
    if (gradData) gradData->assign(gr.begin(), gr.begin() + (size_t)n * 2);
    if (pointPosInXYGrid) pointPosInXYGrid->assign(idx.begin(), idx.begin() + n);
    return n;
  }
};

inline void Frame::setPermaRef(TrackingReference* reference) {
  permaRefNumPts = reference->makePointCloud(4 /* QUICK_KF_CHECK_LVL */, &permaRef_posData, &permaRef_colorAndVarData);
}

// util/settings.h:355-402, every field with the reference's defaults (settings.h:360-400)
struct DenseDepthTrackerSettings {
  float lambdaSuccessFac = 0.5f, lambdaFailFac = 2.0f;
  float lambdaInitial[LSDHIP_PYRAMID_LEVELS] = {0, 0, 0, 0, 0};
  float stepSizeMin[LSDHIP_PYRAMID_LEVELS] = {1e-8f, 1e-8f, 1e-8f, 1e-8f, 1e-8f};
  float convergenceEps[LSDHIP_PYRAMID_LEVELS] = {0.999f, 0.999f, 0.999f, 0.999f, 0.999f};
  int maxItsPerLvl[LSDHIP_PYRAMID_LEVELS] = {5, 20, 50, 100, 100};
  float lambdaInitialTestTrack = 0, stepSizeMinTestTrack = 1e-3f, convergenceEpsTestTrack = 0.98f, maxItsTestTrack = 5;
  float huber_d = 3, var_weight = 1.0f;
};

// Tracking/SE3Tracker.h:41-93
class SE3Tracker {
 public:
  int width, height;
  Mat3f K;
  DenseDepthTrackerSettings settings;

  SE3Tracker(int w, int h, const Mat3f& K_) : width(w), height(h), K(K_), ctx_(Context::get(w, h, K_)) {
    check(lsdhip_tracker_create(ctx_->handle(), &h_), "lsdhip_tracker_create");
  }
  SE3Tracker(const SE3Tracker&) = delete;
  SE3Tracker& operator=(const SE3Tracker&) = delete;
  ~SE3Tracker() { lsdhip_tracker_destroy(h_); }

  SE3 trackFrame(TrackingReference* reference, Frame* frame, const SE3& frameToReference_initialEstimate) {
    pushSettings();
    double init[7];
    frameToReference_initialEstimate.to7(init);
    lsdhip_track_result r;
    hookError_ = nullptr;
    if (!reference || !reference->keyframe || !frame) throw Error(LSDHIP_E_STATE, "SE3Tracker::trackFrame: the tracking reference holds no keyframe");
    check(lsdhip_tracker_track(h_, reference->keyframe->handle(), frame->handle(), init, &r), "lsdhip_tracker_track");
    publish(r);
    if (hookError_) std::rethrow_exception(hookError_);
    return SE3::from7(r.frameToReference);
  }
  // trackFrame for n independent (reference, frame) pairs in the same launches (lsdhip_tracker_track_batch): several sequences sharing
  // one GPU.  results[j] carries what the members above carry after a single call.  A diverged job does not throw: look at
  // results[j].diverged.
  std::vector<SE3> trackFrameBatch(const std::vector<TrackingReference*>& references, const std::vector<Frame*>& frames,
                                   const std::vector<SE3>& inits, std::vector<lsdhip_track_result>& results) {
    pushSettings();
    const int n = (int)frames.size();
    std::vector<lsdhip_frame*> kfs((size_t)n), frs((size_t)n);
    std::vector<double> init((size_t)n * 7);
    for (int j = 0; j < n; j++) {
      if (!references[j] || !references[j]->keyframe || !frames[j]) throw Error(LSDHIP_E_STATE, "SE3Tracker::trackFrameBatch: a tracking reference holds no keyframe");
      kfs[j] = references[j]->keyframe->handle();
      frs[j] = frames[j]->handle();
      inits[j].to7(&init[(size_t)j * 7]);
    }
    results.assign((size_t)n, lsdhip_track_result());
    hookError_ = nullptr;
    const int rc = lsdhip_tracker_track_batch(h_, n, kfs.data(), frs.data(), init.data(), results.data());
    if (rc != LSDHIP_OK && rc != LSDHIP_DIVERGED) check(rc, "lsdhip_tracker_track_batch");
    if (hookError_) std::rethrow_exception(hookError_);
    std::vector<SE3> out((size_t)n);
    for (int j = 0; j < n; j++) out[j] = SE3::from7(results[j].frameToReference);
    return out;
  }
  SE3 trackFrameOnPermaref(Frame* reference, Frame* frame, SE3 referenceToFrame) {
    pushSettings();
    double init[7];
    referenceToFrame.to7(init);
    lsdhip_track_result r;
    check(lsdhip_tracker_track_permaref(h_, reference->permaRef_posData.data(), reference->permaRef_colorAndVarData.data(),
                                        reference->permaRefNumPts, frame->handle(), init, &r), "lsdhip_tracker_track_permaref");
    publish(r);
    return SE3::from7(r.frameToReference);
  }
  // Runs on the calling thread inside trackFrame once the job is queued on the device and before the host waits for it
  // (lsdhip_tracker_set_enqueue_hook): queue independent work here, e.g. the next frame's upload and pyramids.
  // Exceptions thrown by the hook surface from trackFrame after the tracking result has been collected.
  void setEnqueueHook(std::function<void()> fn) {
    hook_ = std::move(fn);
    check(lsdhip_tracker_set_enqueue_hook(h_, hook_ ? &SE3Tracker::hookTrampoline : nullptr, this), "lsdhip_tracker_set_enqueue_hook");
  }
  float checkPermaRefOverlap(Frame* reference, SE3 referenceToFrame) {
    double init[7];
    referenceToFrame.to7(init);
    float usage = 0;
    check(lsdhip_tracker_check_overlap(h_, reference->permaRef_posData.data(), reference->permaRefNumPts, init, &usage), "lsdhip_tracker_check_overlap");
    pointUsage = usage;
    return usage;
  }

  float pointUsage = 0, lastGoodCount = 0, lastMeanRes = 0, lastBadCount = 0, lastResidual = 0;
  float affineEstimation_a = 1, affineEstimation_b = 0;
  bool diverged = false, trackingWasGood = false;
  int numEvaluations = 0, numWarpUpdates = 0;  // instrumentation (residual-kernel launches, LM outer iterations)
  int levelEvaluations[LSDHIP_PYRAMID_LEVELS] = {0, 0, 0, 0, 0};   // evaluations of the last trackFrame per pyramid level
  int numLaunches = 0;                         // evaluating launches of the last job (< numEvaluations: retries share launches)
  void setSpeculation(int trials, int finestLevelWorkgroups = 0) { check(lsdhip_tracker_set_speculation(h_, trials, finestLevelWorkgroups), "lsdhip_tracker_set_speculation"); }
  void setBatchCoarseMinJobs(int minJobs) { check(lsdhip_tracker_set_batch_coarse_min_jobs(h_, minJobs), "lsdhip_tracker_set_batch_coarse_min_jobs"); }
  lsdhip_tracker* handle() const { return h_; }
  const std::shared_ptr<Context>& context() const { return ctx_; }

 private:
  void pushSettings() {   // the public `settings` member is plain data in the reference: hand it over before every job
    lsdhip_tracker_settings st;
    st.lambdaSuccessFac = settings.lambdaSuccessFac; st.lambdaFailFac = settings.lambdaFailFac;
    for (int l = 0; l < LSDHIP_PYRAMID_LEVELS; l++) {
      st.lambdaInitial[l] = settings.lambdaInitial[l]; st.stepSizeMin[l] = settings.stepSizeMin[l];
      st.convergenceEps[l] = settings.convergenceEps[l]; st.maxItsPerLvl[l] = settings.maxItsPerLvl[l];
    }
    st.lambdaInitialTestTrack = settings.lambdaInitialTestTrack; st.stepSizeMinTestTrack = settings.stepSizeMinTestTrack;
    st.convergenceEpsTestTrack = settings.convergenceEpsTestTrack; st.maxItsTestTrack = settings.maxItsTestTrack;
    st.huber_d = settings.huber_d; st.var_weight = settings.var_weight;
    check(lsdhip_tracker_set_settings(h_, &st), "lsdhip_tracker_set_settings");
  }
  void publish(const lsdhip_track_result& r) {
    pointUsage = r.pointUsage; lastGoodCount = r.lastGoodCount; lastMeanRes = r.lastMeanRes; lastBadCount = r.lastBadCount;
    lastResidual = r.lastResidual; affineEstimation_a = r.affineEstimation_a; affineEstimation_b = r.affineEstimation_b;
    diverged = r.diverged != 0; trackingWasGood = r.trackingWasGood != 0;
    numEvaluations = r.numEvaluations; numWarpUpdates = r.numWarpUpdates;
    int st[8];
    if (lsdhip_tracker_exec_stats(h_, st) == 0) for (int l = 0; l < LSDHIP_PYRAMID_LEVELS; l++) levelEvaluations[l] = st[3 + l];
    int ls[2];
    if (lsdhip_tracker_launch_stats(h_, ls) == 0) numLaunches = ls[0];
  }
  static void hookTrampoline(void* self) {
    SE3Tracker* t = static_cast<SE3Tracker*>(self);
    try { if (t->hook_) t->hook_(); } catch (...) { t->hookError_ = std::current_exception(); }
  }
  std::function<void()> hook_;
  std::exception_ptr hookError_;
  std::shared_ptr<Context> ctx_;
  lsdhip_tracker* h_ = nullptr;
};

// The permanent references of all keyframes on the device (lsdhip.h: lsdhip_kfbank_*): Frame::setPermaRef (DataStructures/Frame.cpp:149-174)
// per keyframe, in one allocation made at construction, plus what TrackableKeyFrameSearch reads of a keyframe on the host (frame id,
// meanIdepth, getScaledCamToWorld()).  The host-cloud members (Frame::setPermaRef, SE3Tracker::checkPermaRefOverlap /
// trackFrameOnPermaref) stay as the yardstick.
class KeyFrameBank {
 public:
  struct Info { int frameId, numPoints; float meanIdepth; Sim3 camToWorld; };
  KeyFrameBank(std::shared_ptr<Context> ctx, int maxKeyframes) : ctx_(std::move(ctx)) {
    check(lsdhip_kfbank_create(ctx_->handle(), maxKeyframes, &h_), "lsdhip_kfbank_create");
  }
  KeyFrameBank(const KeyFrameBank&) = delete;
  KeyFrameBank& operator=(const KeyFrameBank&) = delete;
  ~KeyFrameBank() { lsdhip_kfbank_destroy(h_); }
  // Frame::setPermaRef on the device, behind the Frame::setDepth of finalizeKeyFrame; returns the slot = kf.idxInKeyframes
  // (SlamSystem.cpp:408-412).  A keyframe the bank holds (a re-activated one that is finalised again) has its cloud replaced.
  int put(Frame& kf) {
    int slot = -1;
    check(lsdhip_kfbank_put(h_, kf.handle(), &slot), "lsdhip_kfbank_put");
    kf.idxInKeyframes = slot;
    return slot;
  }
  int put(Frame& kf, const Sim3& camToWorld, float meanIdepth = -1.0f) {
    const int slot = put(kf);
    setMeta(slot, camToWorld, meanIdepth);
    return slot;
  }
  // getScaledCamToWorld() / meanIdepth as the search reads them (TrackableKeyFrameSearch.cpp:76-91); meanIdepth < 0 keeps the recorded one
  void setMeta(int slot, const Sim3& camToWorld, float meanIdepth = -1.0f) {
    const double p[8] = {camToWorld.q[0], camToWorld.q[1], camToWorld.q[2], camToWorld.q[3], camToWorld.t[0], camToWorld.t[1], camToWorld.t[2], camToWorld.s};
    check(lsdhip_kfbank_set_meta(h_, slot, p, meanIdepth), "lsdhip_kfbank_set_meta");
  }
  int size() const { return check(lsdhip_kfbank_size(h_), "lsdhip_kfbank_size"); }
  Info info(int slot) const {
    Info o;
    double p[8];
    check(lsdhip_kfbank_info(h_, slot, &o.frameId, &o.numPoints, &o.meanIdepth, p), "lsdhip_kfbank_info");
    for (int i = 0; i < 4; i++) o.camToWorld.q[i] = p[i];
    for (int i = 0; i < 3; i++) o.camToWorld.t[i] = p[4 + i];
    o.camToWorld.s = p[7];
    return o;
  }
  // the slot's cloud as Frame::permaRef_posData / permaRef_colorAndVarData hold it; returns the point count
  int download(int slot, std::vector<float>* posData, std::vector<float>* colorAndVarData) const {
    const int n = info(slot).numPoints;
    std::vector<float> pos((size_t)n * 3 + 1), cv((size_t)n * 2 + 1);
    check(lsdhip_kfbank_download(h_, slot, pos.data(), cv.data()), "lsdhip_kfbank_download");
    if (posData) posData->assign(pos.begin(), pos.begin() + (size_t)n * 3);
    if (colorAndVarData) colorAndVarData->assign(cv.begin(), cv.begin() + (size_t)n * 2);
    return n;
  }
  lsdhip_kfbank* handle() const { return h_; }
  const std::shared_ptr<Context>& context() const { return ctx_; }

 private:
  std::shared_ptr<Context> ctx_;
  lsdhip_kfbank* h_ = nullptr;
};

// GlobalMapping/TrackableKeyFrameSearch.h:58-101, the re-position search: findRePositionCandidate (TrackableKeyFrameSearch.cpp:103-172)
// over a KeyFrameBank in two launches and two host waits (lsdhip_tracker_find_reposition_candidate).  The graph's part — which
// keyframes exist, where they are — is the bank's metadata; the frame's getScaledCamToWorld() and tracking parent are arguments.
class TrackableKeyFrameSearch {
 public:
  // (bank, w, h, K) in the place of the reference's (graph, w, h, K) (TrackableKeyFrameSearch.cpp:32-46); the tracker made from
  // (w, h, K) has to live on the bank's context
  TrackableKeyFrameSearch(KeyFrameBank* bank, int w, int h, const Mat3f& K) : bank_(bank), tracker_(new SE3Tracker(w, h, K)) {
    if (!bank || tracker_->context() != bank->context())
      throw Error(LSDHIP_E_ARG, "TrackableKeyFrameSearch: (w, h, K) name another context than the bank's");
  }
  // returns the slot of the keyframe to re-activate, -1 if none (a new keyframe is to be made); `last` holds what was decided
  int findRePositionCandidate(Frame* frame, const Sim3& frameCamToWorld, int trackingParentId, float maxScore = 1.0f) {
    const double p[8] = {frameCamToWorld.q[0], frameCamToWorld.q[1], frameCamToWorld.q[2], frameCamToWorld.q[3],
                         frameCamToWorld.t[0], frameCamToWorld.t[1], frameCamToWorld.t[2], frameCamToWorld.s};
    check(lsdhip_tracker_set_relocalization_th(tracker_->handle(), relocalizationTH), "lsdhip_tracker_set_relocalization_th");
    check(lsdhip_tracker_find_reposition_candidate(tracker_->handle(), bank_->handle(), frame->handle(), p, trackingParentId, maxScore, &last),
          "lsdhip_tracker_find_reposition_candidate");
    return last.slot;
  }
  // one record per banked keyframe of the last search (what printRelocalizationInfo prints, and the branch each keyframe took)
  std::vector<lsdhip_reposition_record> records() const {
    int n = 0;
    check(lsdhip_tracker_reposition_records(tracker_->handle(), 0, nullptr, &n), "lsdhip_tracker_reposition_records");
    std::vector<lsdhip_reposition_record> r((size_t)n);
    if (n > 0) check(lsdhip_tracker_reposition_records(tracker_->handle(), n, r.data(), &n), "lsdhip_tracker_reposition_records");
    return r;
  }
  // TrackableKeyFrameSearch.h:75-79 with the context's KFDistWeight / KFUsageWeight
  float getRefFrameScore(float distanceSquared, float usage) const {
    const lsdhip_params& p = bank_->context()->params;
    return lsd_slam::loop::keyframeScore(distanceSquared, usage, p.KFDistWeight, p.KFUsageWeight);
  }
  float relocalizationTH = 0.7f;   // util/settings.cpp:101
  lsdhip_reposition_result last = {};
  SE3Tracker& tracker() { return *tracker_; }

 private:
  KeyFrameBank* bank_;
  std::unique_ptr<SE3Tracker> tracker_;
};

// Tracking/Sim3Tracker.h:71-187
class Sim3Tracker {
 public:
  int width, height;
  Mat3f K;
  DenseDepthTrackerSettings settings;

  Sim3Tracker(int w, int h, const Mat3f& K_) : width(w), height(h), K(K_), ctx_(Context::get(w, h, K_)) {
    check(lsdhip_sim3tracker_create(ctx_->handle(), &h_), "lsdhip_sim3tracker_create");
  }
  Sim3Tracker(const Sim3Tracker&) = delete;
  Sim3Tracker& operator=(const Sim3Tracker&) = delete;
  ~Sim3Tracker() { lsdhip_sim3tracker_destroy(h_); }

  Sim3 trackFrameSim3(TrackingReference* reference, Frame* frame, const Sim3& frameToReference_initialEstimate, int startLevel,
                      int finalLevel) {
    check(lsdhip_sim3tracker_set_max_its(h_, settings.maxItsPerLvl), "lsdhip_sim3tracker_set_max_its");
    double init[8] = {frameToReference_initialEstimate.q[0], frameToReference_initialEstimate.q[1], frameToReference_initialEstimate.q[2],
                      frameToReference_initialEstimate.q[3], frameToReference_initialEstimate.t[0], frameToReference_initialEstimate.t[1],
                      frameToReference_initialEstimate.t[2], frameToReference_initialEstimate.s};
    lsdhip_sim3_result r;
    if (!reference || !reference->keyframe || !frame) throw Error(LSDHIP_E_STATE, "Sim3Tracker::trackFrameSim3: the tracking reference holds no keyframe");
    check(lsdhip_sim3tracker_track(h_, reference->keyframe->handle(), frame->handle(), init, startLevel, finalLevel, &r),
          "lsdhip_sim3tracker_track");
    pointUsage = r.pointUsage; lastResidual = r.lastResidual; lastDepthResidual = r.lastDepthResidual;
    lastPhotometricResidual = r.lastPhotometricResidual; affineEstimation_a = r.affineEstimation_a; affineEstimation_b = r.affineEstimation_b;
    diverged = r.diverged != 0; numEvaluations = r.numEvaluations;
    for (int i = 0; i < 49; i++) lastSim3Hessian[i] = r.lastSim3Hessian[i];
    Sim3 out;
    for (int i = 0; i < 4; i++) out.q[i] = r.frameToReference[i];
    for (int i = 0; i < 3; i++) out.t[i] = r.frameToReference[4 + i];
    out.s = r.frameToReference[7];
    return out;
  }

  // n independent jobs in lock step (their evaluations share launches); results[j] as a single call would leave them
  std::vector<Sim3> trackFrameSim3Batch(const std::vector<TrackingReference*>& references, const std::vector<Frame*>& frames,
                                        const std::vector<Sim3>& inits, int startLevel, int finalLevel,
                                        std::vector<lsdhip_sim3_result>* results = nullptr) {
    check(lsdhip_sim3tracker_set_max_its(h_, settings.maxItsPerLvl), "lsdhip_sim3tracker_set_max_its");
    const size_t n = frames.size();
    std::vector<lsdhip_frame*> kfs(n), frs(n);
    std::vector<double> init(8 * n);
    for (size_t j = 0; j < n; j++) {
      kfs[j] = references[j]->keyframe->handle();
      frs[j] = frames[j]->handle();
      for (int i = 0; i < 4; i++) init[8 * j + i] = inits[j].q[i];
      for (int i = 0; i < 3; i++) init[8 * j + 4 + i] = inits[j].t[i];
      init[8 * j + 7] = inits[j].s;
    }
    std::vector<lsdhip_sim3_result> res(n);
    check(lsdhip_sim3tracker_track_batch(h_, (int)n, kfs.data(), frs.data(), init.data(), startLevel, finalLevel, res.data()),
          "lsdhip_sim3tracker_track_batch");
    std::vector<Sim3> out(n);
    for (size_t j = 0; j < n; j++) {
      for (int i = 0; i < 4; i++) out[j].q[i] = res[j].frameToReference[i];
      for (int i = 0; i < 3; i++) out[j].t[i] = res[j].frameToReference[4 + i];
      out[j].s = res[j].frameToReference[7];
    }
    if (results) *results = res;
    return out;
  }

  float pointUsage = 0, lastResidual = 0, lastDepthResidual = 0, lastPhotometricResidual = 0;
  float affineEstimation_a = 1, affineEstimation_b = 0;
  float lastSim3Hessian[49] = {};   // row-major 7x7
  bool diverged = false;
  int numEvaluations = 0;

 private:
  std::shared_ptr<Context> ctx_;
  lsdhip_sim3tracker* h_ = nullptr;
};

// DepthEstimation/DepthMap.h:47-98
class DepthMap {
 public:
  DepthMap(int w, int h, const Mat3f& K) : ctx_(Context::get(w, h, K)) { check(lsdhip_depth_create(ctx_->handle(), &h_), "lsdhip_depth_create"); }
  DepthMap(const DepthMap&) = delete;
  DepthMap& operator=(const DepthMap&) = delete;
  ~DepthMap() { lsdhip_depth_destroy(h_); }

  void reset() { check(lsdhip_depth_reset(h_), "lsdhip_depth_reset"); }
  void updateKeyframe(std::deque<std::shared_ptr<Frame>> referenceFrames) {
    std::vector<lsdhip_frame*> refs;
    refs.reserve(referenceFrames.size());
    for (auto& f : referenceFrames) refs.push_back(f->handle());
    check(lsdhip_depth_update(h_, refs.data(), (int)refs.size()), "lsdhip_depth_update");
    timings();
  }
  // updateKeyframe of several sequences' maps (one context), one tracked frame each, in shared launches (lsdhip_depth_update_batch)
  static void updateKeyframeBatch(const std::vector<DepthMap*>& maps, const std::vector<Frame*>& frames) {
    if (maps.empty()) return;
    std::vector<lsdhip_depthmap*> ms;
    std::vector<lsdhip_frame*> fs;
    for (DepthMap* m : maps) ms.push_back(m->h_);
    for (Frame* f : frames) fs.push_back(f->handle());
    check(lsdhip_depth_update_batch((int)ms.size(), ms.data(), fs.data()), "lsdhip_depth_update_batch");
  }
  void createKeyFrame(Frame* new_keyframe) {
    check(lsdhip_depth_create_keyframe(h_, new_keyframe->handle(), nullptr), "lsdhip_depth_create_keyframe");
    timings();
  }
  // finalizeKeyFrame() + createKeyFrame(newKeyframes[j]) of several sequences' maps (one context) in six shared launches
  // (lsdhip_depth_change_keyframe_batch); one map: the same six launches instead of the two calls' fifteen
  static void changeKeyframeBatch(const std::vector<DepthMap*>& maps, const std::vector<Frame*>& newKeyframes) {
    if (maps.empty()) return;
    std::vector<lsdhip_depthmap*> ms;
    std::vector<lsdhip_frame*> fs;
    for (DepthMap* m : maps) ms.push_back(m->h_);
    for (Frame* f : newKeyframes) fs.push_back(f->handle());
    check(lsdhip_depth_change_keyframe_batch((int)ms.size(), ms.data(), fs.data(), nullptr), "lsdhip_depth_change_keyframe_batch");
  }
  void changeKeyframe(Frame* new_keyframe) { changeKeyframeBatch({this}, {new_keyframe}); timings(); }
  // finalizeKeyFrame() + setFromExistingKF(oldKeyframes[j]) of several sequences' maps (one context) in three shared launches and
  // without a host wait on a pipelined context (lsdhip_depth_reactivate_keyframe_batch): the keyframe change when
  // findRePositionCandidate found a banked keyframe (SlamSystem.cpp:507-540)
  static void reactivateKeyframeBatch(const std::vector<DepthMap*>& maps, const std::vector<Frame*>& oldKeyframes) {
    if (maps.empty()) return;
    std::vector<lsdhip_depthmap*> ms;
    std::vector<lsdhip_frame*> fs;
    for (DepthMap* m : maps) ms.push_back(m->h_);
    for (Frame* f : oldKeyframes) fs.push_back(f->handle());
    check(lsdhip_depth_reactivate_keyframe_batch((int)ms.size(), ms.data(), fs.data()), "lsdhip_depth_reactivate_keyframe_batch");
  }
  void reactivateKeyframe(Frame* old_keyframe) { reactivateKeyframeBatch({this}, {old_keyframe}); timings(); }
  // GPU time (ms, summed) and call counts of updateKeyframe [0] / createKeyFrame [1] / finalizeKeyFrame [2]; synchronises
  void gpuTimes(double ms[3], long long calls[3]) { check(lsdhip_depth_gpu_times(h_, ms, calls), "lsdhip_depth_gpu_times"); }
  void finalizeKeyFrame() { check(lsdhip_depth_finalize(h_), "lsdhip_depth_finalize"); timings(); }
  void invalidate() { check(lsdhip_depth_invalidate(h_), "lsdhip_depth_invalidate"); }
  bool isValid() { return lsdhip_depth_is_valid(h_) != 0; }
  void initializeFromGTDepth(Frame* new_frame) { check(lsdhip_depth_init_gt(h_, new_frame->handle()), "lsdhip_depth_init_gt"); }
  void initializeRandomly(Frame* new_frame) { check(lsdhip_depth_init_random(h_, new_frame->handle()), "lsdhip_depth_init_random"); }
  void setFromExistingKF(Frame* kf) { check(lsdhip_depth_set_from_existing(h_, kf->handle()), "lsdhip_depth_set_from_existing"); }

  // currentDepthMap in the reference's 32-byte AoS layout (DepthMapPixelHypothesis.h:43-60)
  std::vector<lsdhip_hypothesis> currentDepthMap() const {
    std::vector<lsdhip_hypothesis> v((size_t)ctx_->width() * ctx_->height());
    check(lsdhip_depth_download(h_, v.data()), "lsdhip_depth_download");
    return v;
  }
  // DepthMap::debugPlotDepthMap (DepthMap.cpp:1400-1428): the keyframe in grey with the hypotheses painted over it, drawn on the device
  // into debugImageDepth (uint8 [h][w][3]); debugDisplay is the reference's global of that name (util/settings.cpp:35).  Waits for the
  // mapping stream (one launch and a copy of 3 bytes per pixel).  Returns 1, as the reference does.
  int debugPlotDepthMap(int debugDisplay = 0) {
    if (!isValid()) return 1;
    debugImageDepth.resize((size_t)ctx_->width() * ctx_->height() * 3);
    check(lsdhip_depth_debug_plot(h_, debugDisplay, debugImageDepth.data()), "lsdhip_depth_debug_plot");
    return 1;
  }
  // the same image into device memory (3 * w * h bytes, 4-byte aligned): queued behind the map's calls, nothing waits
  void debugPlotDepthMapDevice(unsigned char* dev, int debugDisplay) { check(lsdhip_depth_debug_plot_dev(h_, debugDisplay, dev), "lsdhip_depth_debug_plot_dev"); }
  // ... of several maps of one context in one launch (lsdhip_depth_debug_plot_batch)
  static void debugPlotDepthMapBatch(const std::vector<DepthMap*>& maps, const std::vector<unsigned char*>& devs, int debugDisplay) {
    if (maps.empty()) return;
    if (devs.size() != maps.size()) throw Error(LSDHIP_E_ARG, "DepthMap::debugPlotDepthMapBatch: one device buffer per map");
    std::vector<lsdhip_depthmap*> ms;
    for (DepthMap* m : maps) ms.push_back(m->h_);
    check(lsdhip_depth_debug_plot_batch((int)ms.size(), ms.data(), debugDisplay, devs.data()), "lsdhip_depth_debug_plot_batch");
  }
  std::vector<unsigned char> debugImageDepth;
  // smoothed idepth / variance planes of the active keyframe, device to device (payload of the multi-GPU gather)
  void copyPlanesToDevice(float* idepth_dev, float* idepthVar_dev) { check(lsdhip_depth_copy_planes_dev(h_, idepth_dev, idepthVar_dev), "lsdhip_depth_copy_planes_dev"); }

  float msUpdate = 0, msCreate = 0, msFinalize = 0, msObserve = 0, msRegularize = 0, msPropagate = 0, msFillHoles = 0, msSetDepth = 0;
  lsdhip_depthmap* handle() const { return h_; }

 private:
  void timings() {
    float t[8];
    if (lsdhip_depth_timings(h_, t) == 0) { msUpdate = t[0]; msCreate = t[1]; msFinalize = t[2]; msObserve = t[3]; msRegularize = t[4]; msPropagate = t[5]; msFillHoles = t[6]; msSetDepth = t[7]; }
  }
  std::shared_ptr<Context> ctx_;
  lsdhip_depthmap* h_ = nullptr;
};

// The part of SlamSystem either side of the hot path with doSlam = false (SlamSystem.cpp:890-1040 trackFrame, :739-828
// doMappingIteration, :542-614 updateKeyframe, :458-490 createNewCurrentKeyframe) and a deterministic keyframe policy (a new keyframe
// every `kfEvery` frames) in place of the distance / usage score.  Orchestration only: every per-pixel operation is a liblsdhip.so call.
//
// Two execution models, both the reference's own:
//   * blockUntilMapped = true (default): track frame t, then its mapping iteration, on one stream; frame t + 1 is tracked against what
//     map(t) left (SlamSystem.cpp:1026-1040 with the wait);
//   * pipelined (setPipelined(true); blockUntilMapped = false with the mapper exactly one frame behind): the mapping iteration of frame t
//     is queued on the context's mapping stream when trackFrame(t) ends and runs BESIDE trackFrame(t + 1), which tracks against the
//     keyframe and depth version map(t - 1) left — what the reference's tracking thread does when the mapping thread is still busy
//     (:907-912: it re-imports the tracking reference only when it finds depthHasBeenUpdatedFlag set / the keyframe replaced).  The
//     frame that follows a keyframe change is therefore still tracked on the old keyframe; the mapper drops it (updateKeyframe pops
//     frames whose tracking parent is not the current keyframe, :559-566) and the first frame tracked on the new keyframe starts from
//     se3FromSim3(newKeyframe^-1 * lastTrackedFrame) (:918-920).  The lag is fixed at one frame, so results do not depend on timing.
//
// Both loops hold the same two pieces: the camera their frames come from (LoopCamera) and, per sequence, the state SlamSystem keeps and
// the rules of lsd_slam_hip_loop.hpp applied to it (LoopSequence).  What differs between the loops is stated where it lives.

// The camera of a loop: rectified w x h images, or raw inputWidth x inputHeight images rectified inside frame creation, in host or
// in device memory.  The one place frames of a loop are created.
struct LoopCamera {
  int w, h;
  Mat3f K;
  bool imagesOnDevice;
  std::shared_ptr<DeviceUndistorter> undistorter;    // set: images are raw images of this camera
  std::shared_ptr<Context> context() const { return Context::get(w, h, K); }
  void setUndistorter(std::shared_ptr<DeviceUndistorter> u) {
    if (u && u->context() != context()) throw Error(LSDHIP_E_ARG, "SlamLoop / SlamLoopBatch::setUndistorter: the undistorter belongs to another output size / K");
    undistorter = std::move(u);
  }
  // async: a host image whose upload is queued and not waited for (the caller keeps the bytes unchanged until the frame has been
  // tracked: SlamLoop::step's nextImage contract)
  std::shared_ptr<Frame> frame(int id, const unsigned char* img, bool async) const {
    if (undistorter) {
      if (imagesOnDevice) return std::make_shared<Frame>(id, *undistorter, 0.0, Frame::RawDeviceImage{img});
      if (async) return std::make_shared<Frame>(id, *undistorter, 0.0, Frame::RawHostImageAsync{img});
      return std::make_shared<Frame>(id, *undistorter, 0.0, Frame::RawImage{img});
    }
    if (imagesOnDevice) return std::make_shared<Frame>(id, w, h, K, 0.0, Frame::DeviceImage{img});
    if (async) return std::make_shared<Frame>(id, w, h, K, 0.0, Frame::HostImageAsync{img});
    return std::make_shared<Frame>(id, w, h, K, 0.0, img);
  }
  // one frame of several sequences in shared launches
  std::vector<std::shared_ptr<Frame>> frames(const std::vector<int>& ids, const unsigned char* const* images) const {
    if (undistorter) return Frame::createBatch(*undistorter, ids, images, imagesOnDevice);
    return Frame::createBatch(w, h, K, ids, images, imagesOnDevice);
  }
};
inline void setLoopIterations(SE3Tracker& tracker) {
  static_assert(sizeof(lsd_slam::loop::TRACKER_MAX_ITS_PER_LVL) == sizeof(tracker.settings.maxItsPerLvl), "one entry per pyramid level");
  std::memcpy(tracker.settings.maxItsPerLvl, lsd_slam::loop::TRACKER_MAX_ITS_PER_LVL, sizeof(lsd_slam::loop::TRACKER_MAX_ITS_PER_LVL));
}

// What SlamSystem keeps for ONE sequence, and what happens to it around each tracked frame: SlamLoop is one of these, SlamLoopBatch
// holds S.  The loops own the device work (which call, on which stream, shared with whom, queued when); every counter, flag and pose
// estimate changes here and nowhere else.
struct LoopSequence {
  using MappingStep = lsd_slam::loop::MappingStep;
  LoopSequence(int w, int h, const Mat3f& K) : map(w, h, K) {}
  DepthMap map;
  TrackingReference reference;
  std::shared_ptr<Frame> keyframe;       // the mapper's current keyframe (DepthMap::activeKeyFrame)
  std::shared_ptr<Frame> trackKF;        // the keyframe the tracking reference points at (== keyframe unless a promotion is pending)
  std::shared_ptr<Frame> pendingKF;      // pipelined: made current by the mapping iteration queued last, not yet adopted by the tracker
  SE3 lastFrameToKF;                     // the next frame's initial estimate
  int sinceKF = 0;                       // frames tracked since the keyframe change, dropped ones included
  int mappedOnKF = 0;                    // Frame::numMappedOnThisTotal of the current keyframe: counted here, so that the asynchronous
                                         // pipeline is not drained every frame by Frame::stats()
  int numKeyframesFinished = 0;          // keyFrameGraph->keyframesAll.size()
  long numTracked = 0, numTrackedGood = 0, numUpdates = 0, evaluations = 0;
  long numDropped = 0;                   // frames tracked on a keyframe the mapper had already replaced (pipelined): not mapped
  bool trackingLost = false;             // SlamSystem::trackingIsGood == false: the sequence takes no further frames
  bool newKeyframe = false;              // the last tracked frame led to a keyframe change
  std::vector<std::shared_ptr<Frame>> keyframeLog;   // every frame promoted while the loop's keepKeyframes was on

  // gtDepth0 != null: SlamSystem::gtDepthInit (SlamSystem.cpp:831-854); null: SlamSystem::randomInit (:857-881)
  void start(std::shared_ptr<Frame> first, const float* gtDepth0) {
    keyframe = std::move(first);
    if (gtDepth0) {
      keyframe->setDepthFromGroundTruth(gtDepth0);
      map.initializeFromGTDepth(keyframe.get());
    } else {
      map.initializeRandomly(keyframe.get());
    }
    trackKF = keyframe;
    importReference(*keyframe);
  }
  void importReference(Frame& kf) {
    reference.importFrame(&kf);
    kf.clearDepthHasBeenUpdatedFlag();
  }
  // the tracking thread's re-import when the mapper has changed the keyframe's depth (SlamSystem.cpp:907-912).  A one-stream loop
  // does it before tracking a frame, a pipelined one after (tracked()): there the mapping iteration runs beside the tracking.
  void importIfUpdated(Frame& kf) { if (kf.depthHasBeenUpdatedFlag()) importReference(kf); }
  // se3FromSim3(keyframe^-1 * frame) for a frame tracked on the keyframe's tracking parent (SlamSystem.cpp:918-920)
  static SE3 relativePose(Frame& kf, Frame& frame) {
    double p[7];
    check(lsdhip_frame_relative_pose(kf.handle(), frame.handle(), p), "lsdhip_frame_relative_pose");
    return SE3::from7(p);
  }

  // `frame` has been tracked on `trackedOn` (trackKF as it was when tracking began; the caller keeps it alive for the step) and gave
  // `est`: counts the result and decides the frame's mapping step.
  //   * Lost: the reference is invalidated, the keyframe finalised (finalisedAtLoss() is called then, the map still valid) or discarded,
  //     the map invalidated.  What follows in the reference is the relocaliser (out of scope).
  //   * otherwise a pipelined loop adopts what the mapping iteration queued one frame ago has done meanwhile: a new current keyframe
  //     (the next estimate is estimateOnPending(), SlamSystem.cpp:907-920) or new depth on the old one.
  //   * Dropped: see MappingStep; the frame still counts towards sinceKF.
  //   * Update / KeyframeChange by wantsKeyframe(), which is asked only for a frame tracked on the current keyframe.  A one-stream loop
  //     takes `est` as the next estimate only with an Update: a keyframe change sets its own (install()).
  template <class FinalisedAtLoss, class EstimateOnPending, class WantsKeyframe>
  MappingStep tracked(bool pipelined, const std::shared_ptr<Frame>& trackedOn, Frame& frame, const SE3& est, bool diverged, bool trackingWasGood,
                      int numEvaluations, FinalisedAtLoss&& finalisedAtLoss, EstimateOnPending&& estimateOnPending, WantsKeyframe&& wantsKeyframe) {
    namespace rules = lsd_slam::loop;
    numTracked++;
    evaluations += numEvaluations;
    if (trackingWasGood) numTrackedGood++;
    newKeyframe = false;
    if (rules::trackingLost(diverged, trackingWasGood, numKeyframesFinished)) {
      trackingLost = true;
      reference.invalidate();
      if (map.isValid()) {
        if (rules::finaliseOnLoss(mappedOnKF)) {
          map.finalizeKeyFrame();
          numKeyframesFinished++;
          finalisedAtLoss();
        }
        map.invalidate();
      }
      return MappingStep::Lost;
    }
    if (pipelined) {
      if (pendingKF) {
        lastFrameToKF = estimateOnPending();
        trackKF = pendingKF;
        pendingKF.reset();
        importReference(*trackKF);
      } else {
        lastFrameToKF = est;
        importIfUpdated(*trackKF);
      }
    }
    ++sinceKF;
    const bool onCurrent = trackedOn == keyframe;
    const MappingStep step = rules::mappingStep(false, onCurrent, onCurrent && wantsKeyframe());
    if (step == MappingStep::Dropped) {
      frame.clear_refPixelWasGood();
      numDropped++;
    } else if (step == MappingStep::Update) {
      if (!pipelined) lastFrameToKF = est;
    } else {
      newKeyframe = true;
    }
    return step;
  }
  // updateKeyframe with `frame` has been queued
  void mapped(Frame& frame) {
    mappedOnKF++;
    numUpdates++;
    frame.clear_refPixelWasGood();
  }
  // `kf` is the mapper's current keyframe from now on.  A pipelined loop's tracker keeps the old keyframe for one more frame
  // (tracked() adopts the new one); a one-stream loop tracks the next frame on it, from nextEstimate.
  void install(const std::shared_ptr<Frame>& kf, bool pipelined, const SE3& nextEstimate) {
    keyframe = kf;
    mappedOnKF = 0;
    sinceKF = 0;
    if (pipelined) {
      pendingKF = kf;
    } else {
      trackKF = kf;
      importReference(*kf);
      lastFrameToKF = nextEstimate;
    }
  }
  // createNewCurrentKeyframe (SlamSystem.cpp:458-490): the tracked frame becomes the keyframe, the next frame starts at the identity.
  // countFinished: the keyframe it replaces enters the graph here (a loop that banks its keyframes counts them there)
  void promote(const std::shared_ptr<Frame>& frame, bool pipelined, bool keepLog, bool countFinished) {
    if (countFinished) numKeyframesFinished++;
    if (keepLog) keyframeLog.push_back(frame);
    install(frame, pipelined, SE3());
  }
};

class SlamLoop : public LoopSequence {
 public:
  // gtDepth0: see LoopSequence::start.
  // kfEvery > 0: a new keyframe every kfEvery frames (deterministic; what bench.py and the parity tests use);
  // kfEvery == 0: the reference's distance / usage score (SlamSystem.cpp:997-1015 with doSlam = false).  Only this loop has the score rule.
  SlamLoop(int w, int h, const Mat3f& K, const unsigned char* firstImage, bool imagesOnDevice, const float* gtDepth0, int kfEvery)
      : SlamLoop(w, h, K, nullptr, firstImage, imagesOnDevice, gtDepth0, kfEvery) {}
  // Raw camera images: w, h, K are those of the RECTIFIED images (Undistorter::out_width / out_height / K), firstRawImage and every
  // image given to step() are raw inputWidth x inputHeight images of the undistorter's camera, rectified inside frame creation.
  SlamLoop(int w, int h, const Mat3f& K, std::shared_ptr<DeviceUndistorter> undistorter, const unsigned char* firstRawImage,
           bool imagesOnDevice, const float* gtDepth0, int kfEvery)
      : LoopSequence(w, h, K), tracker(w, h, K), cam_{w, h, K, imagesOnDevice, nullptr}, kfEvery_(kfEvery) {
    cam_.setUndistorter(std::move(undistorter));
    setLoopIterations(tracker);
    start(cam_.frame(0, firstRawImage, false), gtDepth0);
    tracker.setEnqueueHook([this]() {
      // runs once the tracking job's launches are queued: the place for everything the device can do beside it
      flushDeferredMapping();
      if (!pendingNext_) return;
      prefetched_ = cam_.frame(frameId_ + 1, pendingNext_, pipelined_);
      prefetchedSrc_ = pendingNext_;
    });
  }
  // From the next step() on images are raw images of this camera (null: rectified w x h images again).  One camera serves all loops of
  // a context; an image announced as nextImage stays what it was announced as.
  void setUndistorter(std::shared_ptr<DeviceUndistorter> undistorter) { cam_.setUndistorter(std::move(undistorter)); }
  const std::shared_ptr<DeviceUndistorter>& undistorter() const { return cam_.undistorter; }

  SlamLoop(const SlamLoop&) = delete;
  SlamLoop& operator=(const SlamLoop&) = delete;
  // Tracking beside mapping with the mapper one frame behind (see above).  Switch before the first step() call.
  void setPipelined(bool on) {
    if (frameId_ != 0) throw Error(LSDHIP_E_STATE, "SlamLoop::setPipelined: switch before the first frame");
    cam_.context()->setPipeline(on);
    pipelined_ = on;
  }
  bool pipelined() const { return pipelined_; }
  // Only this loop defers ONE frame's update (SlamLoopBatch defers a whole step's mapping work), behind the deferMapping switch:
  // pipelined loops queue a frame's updateKeyframe only once the NEXT frame's tracking launches are queued (from the tracker's enqueue
  // hook: between two tracking jobs the host queues nothing but the next job).  After the last step() of a batch this queues what is
  // still waiting.
  void flushDeferredMapping() {
    if (!deferredMap_) return;
    std::shared_ptr<Frame> frame = std::move(deferredMap_);
    deferredMap_.reset();
    runUpdate(frame);
  }
  // called with the keyframe that has just been finalised (before the next one replaces it): output hook (PLY, messages)
  std::function<void(Frame&, DepthMap&)> onKeyframeFinished;
  // Second output hook: called AFTER the keyframe change (DepthMap::changeKeyframe, or createKeyFrame on the split path) with the keyframe
  // that was just finalised.  Meant for stream-ordered work (PointCloud::appendKeyframe queues three launches and returns): the planes of
  // that keyframe stay as finalised.  A hook that waits for the device (a download, makeKeyframeMsgDevice) is still correct, but stalls the
  // loop for that wait once per keyframe.  Setting the hook leaves the loop on the shared keyframe change.
  std::function<void(Frame&)> onKeyframeFinishedAsync;
  // called right after a frame's mapping iteration (updateKeyframe, or the keyframe change) has been queued: where
  // SlamSystem::doMappingIteration calls debugDisplayDepthMap (SlamSystem.cpp:777-797).  Meant for stream-ordered work
  // (DepthMap::debugPlotDepthMapDevice queues one launch and returns); a hook that waits (debugPlotDepthMap) stalls the loop for that wait
  // once per frame.  Unset, the loop is unchanged.
  std::function<void(DepthMap&)> onMappingIteration;
  // track one frame, then one mapping iteration; returns frameToKeyframe (of the keyframe the frame was tracked on).  Throws when
  // tracking diverges.
  SE3 step(const unsigned char* image) { return step(image, [](double) {}); }
  // same, reporting the wall-clock instant (seconds, steady clock) at which tracking ended and mapping began.
  // nextImage (optional): the image of the following step() call, if it is already available — its upload and pyramids
  // are queued while the host waits for this frame's tracking result, so they fill the device's idle time of that round
  // trip.  The bytes behind nextImage must stay unchanged until that following call (same pointer) has returned.
  template <typename F>
  SE3 step(const unsigned char* image, F&& onTrackEnd, const unsigned char* nextImage = nullptr) {
    // after a tracking loss the keyframe and the map are gone (SlamSystem::trackingIsGood == false until the relocaliser — out of
    // scope — finds a pose again): every further step fails the same way instead of touching the invalidated reference
    if (trackingLost) throw Error(LSDHIP_E_STATE, "SlamLoop: tracking lost (no relocaliser here): create a new loop");
    lsdhip_host_mark(0);
    frameId_++;
    std::shared_ptr<Frame> frame;
    if (prefetched_ && prefetchedSrc_ == image) frame = std::move(prefetched_);
    else frame = cam_.frame(frameId_, image, false);
    prefetched_.reset();
    pendingNext_ = nextImage;
    if (!pipelined_) importIfUpdated(*trackKF);
    lsdhip_host_mark(1);
    const std::shared_ptr<Frame> trackedOn = trackKF;      // == keyframe unless the mapper is promoting a new one right now (pipelined)
    SE3 est = tracker.trackFrame(&reference, frame.get(), lastFrameToKF);
    lsdhip_host_mark(8);
    pendingNext_ = nullptr;
    launches += tracker.numLaunches;
    for (int l = 0; l < LSDHIP_PYRAMID_LEVELS; l++) levelEvaluations[l] += tracker.levelEvaluations[l];
    lastTrackEnd = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    onTrackEnd(lastTrackEnd);
    flushDeferredMapping();      // (normally empty: the tracking job's hook has queued it)
    // ---- this frame's mapping iteration (pipelined: queued on the mapping stream, it runs beside the next frame's tracking) ----------
    const MappingStep next = tracked(
        pipelined_, trackedOn, *frame, est, tracker.diverged, tracker.trackingWasGood, tracker.numEvaluations,
        [&] {   // a keyframe finalised at the loss goes to the output hooks like any other (SlamLoopBatch feeds no sink there)
          if (onKeyframeFinished) onKeyframeFinished(*keyframe, map);
          if (onKeyframeFinishedAsync) onKeyframeFinishedAsync(*keyframe);
        },
        [&] { return estimateOnPending(*frame, est); }, [&] { return wantsNewKeyframe(est); });
    switch (next) {
      case MappingStep::Lost:    // this loop reports the loss (SlamLoopBatch marks the sequence and goes on with the others)
        throw Error(LSDHIP_DIVERGED, std::string("SlamLoop: tracking lost at frame ") + std::to_string(frameId_) +
                                         (tracker.diverged ? " (diverged)" : " (trackingWasGood false)"));
      case MappingStep::Dropped: break;
      case MappingStep::KeyframeChange: changeKeyframe(frame, est); break;
      case MappingStep::Update:
        if (pipelined_ && deferMapping) deferredMap_ = frame;       // queued from the next tracking job's enqueue hook (or flushDeferredMapping)
        else runUpdate(frame);
        break;
    }
    return est;
  }
  SE3Tracker tracker;
  long launches = 0;
  long levelEvaluations[LSDHIP_PYRAMID_LEVELS] = {0, 0, 0, 0, 0};
  double lastTrackEnd = 0;
  int liveQueueLength = 1;                           // frames handed to updateKeyframe per mapping iteration
  bool deferMapping = true;                          // pipelined loops: see flushDeferredMapping
  bool sharedKeyframeChange = true;                  // finalizeKeyFrame + createKeyFrame as DepthMap::changeKeyframe (six launches); false: the two calls
  bool keepKeyframes = false;                        // keep every keyframe alive in keyframeLog (validation: rescale factors)

  // ---- re-activation of banked keyframes: the SLAMEnabled branches of SlamSystem::finishCurrentKeyframe (SlamSystem.cpp:395-426) and
  // SlamSystem::changeKeyframe(false, true, 1.0f) (:507-540).  Off by default: a loop that never calls enableReactivation runs none of it.
  bool reactivateKeyframes = false;
  // one record per keyframe change of a loop with re-activation on: the frame that triggered it, the keyframe finished and the keyframe
  // that follows (the frame itself, or the banked keyframe found), and what the search looked at (lsdhip_reposition_result)
  struct KeyframeChange { int frameId, previousKfId, newKfId; bool reactivated; int numPotential, numChecked, numTracked; };
  std::vector<KeyframeChange> keyframeChanges;
  long numReactivations = 0;                         // changes that went back to a banked keyframe
  long numUnbanked = 0;                              // finished keyframes the full bank could not take: never re-activated
  // Keeps every finished keyframe in a KeyFrameBank of maxKeyframes slots and, at every keyframe change, first looks for a banked
  // keyframe to go back to (TrackableKeyFrameSearch::findRePositionCandidate).  Call before the first step().
  void enableReactivation(int maxKeyframes) {
    if (frameId_ != 0) throw Error(LSDHIP_E_STATE, "SlamLoop::enableReactivation: switch before the first frame");
    if (maxKeyframes <= 0) throw Error(LSDHIP_E_ARG, "SlamLoop::enableReactivation: a bank of at least one keyframe");
    bank_.reset(new KeyFrameBank(cam_.context(), maxKeyframes));
    search_.reset(new TrackableKeyFrameSearch(bank_.get(), cam_.w, cam_.h, cam_.K));
    bankedBySlot_.assign((size_t)maxKeyframes, nullptr);
    std::array<double, 8> I;
    lsd_slam::pose::sim3_identity(I.data());
    worldPoses_[keyframe->id()] = I;                 // the first keyframe is the world frame
    reactivateKeyframes = true;
  }
  const KeyFrameBank* keyframeBank() const { return bank_.get(); }
  const TrackableKeyFrameSearch* keyframeSearch() const { return search_.get(); }
  // camToWorld of a keyframe of this loop (8 doubles, lsd_slam_hip_pose.hpp), in double on the host as the reference keeps it
  const std::array<double, 8>& worldPose(const Frame& kf) const {
    auto it = worldPoses_.find(kf.id());
    if (it == worldPoses_.end()) throw Error(LSDHIP_E_STATE, "SlamLoop::worldPose: not a keyframe of this loop");
    return it->second;
  }

 private:
  // finishCurrentKeyframe's SLAMEnabled part (SlamSystem.cpp:402-422) for the keyframe that has just been finalised: its permanent
  // reference into the bank, queued behind the launches that wrote its planes; a keyframe the bank holds has its slot replaced
  void bankFinishedKeyframe(const std::shared_ptr<Frame>& kf) {
    const bool firstTime = kf->idxInKeyframes < 0;
    int slot = -1;
    const int rc = lsdhip_kfbank_put(bank_->handle(), kf->handle(), &slot);
    if (rc == LSDHIP_E_CAPACITY) {
      numUnbanked++;
      numKeyframesFinished++;        // (never banked, so never finished twice)
      return;
    }
    check(rc, "lsdhip_kfbank_put");
    kf->idxInKeyframes = slot;
    bank_->setMeta(slot, Sim3::from8(worldPose(*kf).data()), kf->meanIdepth());
    bankedBySlot_[(size_t)slot] = kf;
    if (firstTime) numKeyframesFinished++;           // keyframesAll grows for idxInKeyframes < 0 only (SlamSystem.cpp:408-412)
  }
  // pipelined: the next estimate on the keyframe the mapper has made current while `frame` was tracked on the old one
  SE3 estimateOnPending(Frame& frame, const SE3& est) {
    if (!pendingIsReactivated_) return relativePose(*pendingKF, frame);
    // a banked keyframe came back: it is neither this frame's tracking parent nor its parent's child, so the estimate is the
    // general product over the host's world poses, this frame's being camToWorld(its keyframe) * sim3(frameToKeyframe, 1)
    double f2k[8], frameToWorld[8], p[7];
    est.to7(f2k); f2k[7] = 1;
    lsd_slam::pose::sim3_mul(worldPose(*trackKF).data(), f2k, frameToWorld);
    lsd_slam::pose::relative_se3(worldPose(*pendingKF).data(), frameToWorld, p);
    pendingIsReactivated_ = false;
    return SE3::from7(p);
  }
  // the keyframe policy for a frame tracked on the current keyframe (lsd_slam_hip_loop.hpp)
  bool wantsNewKeyframe(const SE3& est) {
    namespace rules = lsd_slam::loop;
    if (kfEvery_ != 0) return rules::wantsNewKeyframe(kfEvery_, sinceKF);
    if (!rules::scoreRuleApplies(mappedOnKF)) return false;
    // SlamSystem.cpp:997-1015: dist = translation * meanIdepth; keyframesAll holds what the bank holds (:1001-1003), nothing without one
    const float mi = keyframe->meanIdepth();
    const float d0 = (float)est.t[0] * mi, d1 = (float)est.t[1] * mi, d2 = (float)est.t[2] * mi;
    const float minVal = reactivateKeyframes ? rules::scoreThreshold(bank_->size()) : rules::scoreThreshold();
    return rules::wantsNewKeyframe(mappedOnKF, rules::keyframeScore(d0 * d0 + d1 * d1 + d2 * d2, tracker.pointUsage), minVal);
  }
  // SlamSystem::doMappingIteration's keyframe change (SlamSystem.cpp:783-791): finishCurrentKeyframe, then `frame` is promoted
  // (createNewCurrentKeyframe) — or, with re-activation on (doKFReActivation), changeKeyframe(false, true, 1.0f) first looks for a
  // banked keyframe to come back (loadNewCurrentKeyframe, :491-505)
  void changeKeyframe(const std::shared_ptr<Frame>& frame, const SE3& est) {
    const std::shared_ptr<Frame> finished = keyframe;
    std::shared_ptr<Frame> found;
    double cw[8];
    if (reactivateKeyframes) {
      // the candidate's getScaledCamToWorld(): camToWorld(current keyframe) * sim3(frameToKeyframe, 1)
      double f2k[8];
      est.to7(f2k); f2k[7] = 1;
      lsd_slam::pose::sim3_mul(worldPose(*keyframe).data(), f2k, cw);
      // The reference searches after finishCurrentKeyframe.  The search reads the bank entries of EARLIER keyframes only — the current
      // keyframe is the candidate's tracking parent and is skipped (TrackableKeyFrameSearch.cpp:118) — so it may run before the current
      // keyframe is finalised and banked, and finalizeKeyFrame can then share its launches with the change that the search decides.
      const int slot = search_->findRePositionCandidate(frame.get(), Sim3::from8(cw), keyframe->id(), 1.0f);
      if (slot >= 0) found = bankedBySlot_[(size_t)slot];
      if (slot >= 0 && !found) throw Error(LSDHIP_E_STATE, "SlamLoop: the search returned a slot this loop did not fill");
    }
    if (onKeyframeFinished || !sharedKeyframeChange) {
      // an output hook reads the finalised map (PLY, keyframe messages, the multi-GPU gather): the two calls, the hook between them
      map.finalizeKeyFrame();
      if (onKeyframeFinished) onKeyframeFinished(*finished, map);
      if (found) map.setFromExistingKF(found.get());
      else map.createKeyFrame(frame.get());
    } else if (found) {
      map.reactivateKeyframe(found.get());
    } else {
      map.changeKeyframe(frame.get());
    }
    // (the put reads the planes the finalise pass and the pyramid launch wrote: queued behind them)
    if (reactivateKeyframes) bankFinishedKeyframe(finished);
    if (onKeyframeFinishedAsync) onKeyframeFinishedAsync(*finished);
    if (reactivateKeyframes) {
      const lsdhip_reposition_result& r = search_->last;
      keyframeChanges.push_back(KeyframeChange{frame->id(), finished->id(), found ? found->id() : frame->id(), found != nullptr,
                                               r.numPotential, r.numChecked, r.numTracked});
    }
    if (found) {
      numReactivations++;
      found->clearDepthHasBeenUpdatedFlag();         // loadNewCurrentKeyframe (SlamSystem.cpp:503)
      // the next frame starts from se3FromSim3(camToWorld(keyframe)^-1 * camToWorld(lastTrackedFrame)) (SlamSystem.cpp:922-925)
      double nextEstimate[7];
      lsd_slam::pose::relative_se3(worldPose(*found).data(), cw, nextEstimate);
      install(found, pipelined_, SE3::from7(nextEstimate));
    } else {
      if (reactivateKeyframes) {
        // camToWorld(new keyframe) = camToWorld(parent) * thisToParent_raw, the scale createKeyFrame gave it included (waits for it once)
        double raw[8];
        check(lsdhip_frame_get_pose(frame->handle(), raw), "lsdhip_frame_get_pose");
        std::array<double, 8> w;
        lsd_slam::pose::sim3_mul(worldPose(*finished).data(), raw, w.data());
        worldPoses_[frame->id()] = w;
      }
      // with re-activation on, numKeyframesFinished grows in bankFinishedKeyframe: for a keyframe banked for the first time or refused
      promote(frame, pipelined_, keepKeyframes, !reactivateKeyframes);
    }
    pendingIsReactivated_ = pipelined_ && found;
    liveQueue_.clear();
    if (onMappingIteration) onMappingIteration(map);
  }
  std::unique_ptr<KeyFrameBank> bank_;
  std::unique_ptr<TrackableKeyFrameSearch> search_;
  std::vector<std::shared_ptr<Frame>> bankedBySlot_;           // every banked keyframe stays alive: its re-activation planes, level-0 image
                                                               // and maxGradients are needed when it comes back
  std::map<int, std::array<double, 8>> worldPoses_;            // camToWorld per keyframe id
  bool pendingIsReactivated_ = false;                          // pipelined: pendingKF is a banked keyframe that came back
  // DepthMap::updateKeyframe for one tracked frame (SlamSystem::updateKeyframe, SlamSystem.cpp:542-614)
  void runUpdate(const std::shared_ptr<Frame>& frame) {
    // blockUntilMapped = true: the unmapped queue holds exactly this frame (SlamSystem.cpp:559-571, :1030-1039).
    // liveQueueLength > 1 restates live operation, where the mapper finds several tracked frames waiting and passes the
    // whole deque (oldest first, at most liveQueueLength of them) to updateKeyframe.
    liveQueue_.push_back(frame);
    while ((int)liveQueue_.size() > (liveQueueLength > 1 ? liveQueueLength : 1)) liveQueue_.pop_front();
    std::deque<std::shared_ptr<Frame>> q(liveQueue_.begin(), liveQueue_.end());
    lsdhip_host_mark(9);
    map.updateKeyframe(q);
    lsdhip_host_mark(13);
    mapped(*frame);
    lsdhip_host_mark(14);
    if (onMappingIteration) onMappingIteration(map);
  }
  std::shared_ptr<Frame> deferredMap_;
  LoopCamera cam_;
  bool pipelined_ = false;
  int kfEvery_, frameId_ = 0;
  std::shared_ptr<Frame> prefetched_;
  const unsigned char* prefetchedSrc_ = nullptr;
  const unsigned char* pendingNext_ = nullptr;
  std::deque<std::shared_ptr<Frame>> liveQueue_;
};

// S independent sequences through ONE GPU, one frame of each per step() (BASELINE.json configs[3] with more sequences than GPUs).
// Per sequence this is SlamLoop with blockUntilMapped = true: track the frame, then its mapping iteration, the next frame tracked against
// what that left.  Across sequences every stage shares its launches: the new frames (Frame::createBatch), the tracking jobs
// (SE3Tracker::trackFrameBatch: throughput mode from 8 jobs on), the updateKeyframe calls (DepthMap::updateKeyframeBatch).  Keyframe
// changes (finalize + createKeyFrame, once every kfEvery frames per sequence) stay per-sequence calls.  A sequence whose tracking is
// lost stops taking part (lost(s) == true, SlamLoop's rules); the others go on.
// Unlike SlamLoop it has the fixed keyframe interval only (kfEvery > 0: no score rule), no re-activation, and no output hooks: a
// sequence's finalised keyframes go to its cloud sink.
class SlamLoopBatch {
 public:
  struct Sequence : LoopSequence {
    using LoopSequence::LoopSequence;
    lsdhip_track_result last = lsdhip_track_result();
    std::shared_ptr<Frame> replacedFirst;              // the keyframe its first keyframe change replaced while keepKeyframes was on (not in the log: it was never promoted)
  };
  // firstImages / gtDepth0: S pointers each (gtDepth0 == null or gtDepth0[s] == null: random initialisation of that sequence)
  SlamLoopBatch(int w, int h, const Mat3f& K, int S, const unsigned char* const* firstImages, bool imagesOnDevice,
                const float* const* gtDepth0, int kfEvery)
      : SlamLoopBatch(w, h, K, nullptr, S, firstImages, imagesOnDevice, gtDepth0, kfEvery) {}
  // Raw camera images of one camera for all sequences: w, h, K are those of the RECTIFIED images, firstRawImages and every image given
  // to step() are raw inputWidth x inputHeight images, rectified inside frame creation (SlamLoop's raw-image constructor).
  SlamLoopBatch(int w, int h, const Mat3f& K, std::shared_ptr<DeviceUndistorter> undistorter, int S, const unsigned char* const* firstRawImages,
                bool imagesOnDevice, const float* const* gtDepth0, int kfEvery)
      : tracker(w, h, K), cam_{w, h, K, imagesOnDevice, nullptr}, kfEvery_(kfEvery) {
    cam_.setUndistorter(std::move(undistorter));
    if (S <= 0 || kfEvery <= 0) throw Error(LSDHIP_E_ARG, "SlamLoopBatch: S > 0 sequences, a fixed keyframe interval > 0");
    setLoopIterations(tracker);
    tracker.setBatchCoarseMinJobs(coarseMinJobs(false));
    std::vector<std::shared_ptr<Frame>> first = cam_.frames(std::vector<int>((size_t)S, idOf(0, 0)), firstRawImages);
    for (int s = 0; s < S; s++) {
      seqs_.emplace_back(new Sequence(w, h, K));
      seqs_.back()->start(first[s], gtDepth0 ? gtDepth0[s] : nullptr);
    }
  }
  // From the next step() on images are raw images of this camera (null: rectified w x h images again); images announced as nextImages
  // stay what they were announced as.
  void setUndistorter(std::shared_ptr<DeviceUndistorter> undistorter) { cam_.setUndistorter(std::move(undistorter)); }

  // Sequences started together change keyframe in the same step; real cameras do not.  phase[s] in [0, kfEvery): sequence s behaves as
  // if its current keyframe were already phase[s] frames old (its first keyframe change comes kfEvery - phase[s] frames in).  Call before
  // the first step().
  void setKeyframePhases(const std::vector<int>& phase) {
    if (frameId_ != 0 || (int)phase.size() != size()) throw Error(LSDHIP_E_STATE, "SlamLoopBatch::setKeyframePhases: one phase per sequence, before the first step");
    for (int s = 0; s < size(); s++) seqs_[s]->sinceKF = phase[s] < 0 ? 0 : phase[s] % kfEvery_;
  }
  SlamLoopBatch(const SlamLoopBatch&) = delete;
  SlamLoopBatch& operator=(const SlamLoopBatch&) = delete;
  int size() const { return (int)seqs_.size(); }
  Sequence& sequence(int s) { return *seqs_[s]; }
  bool lost(int s) const { return seqs_[s]->trackingLost; }
  // frame ids count per sequence, as in S separate SlamLoops (an id is only compared with ids of the same sequence: tracking parent,
  // nextStereoFrameMinID — which is a float, DepthMapPixelHypothesis.h:49: ids beyond 2^24 would round)
  static int idOf(int /*s*/, int t) { return t; }
  // Tracking beside mapping for ALL sequences (the context becomes a pipelined one): per sequence exactly SlamLoop::setPipelined — the
  // mapper one frame behind the tracker, frames tracked on a keyframe the mapper has meanwhile replaced are dropped
  // (SlamSystem.cpp:559-566), the first frame on a new keyframe starts from se3FromSim3(newKeyframe^-1 * lastTrackedFrame) (:913-920).
  // The tracking batch of step t + 1 — a chain of small latency-bound launches — runs beside the shared updateKeyframe launches and the
  // keyframe changes of step t.  Call before the first step().
  // One workgroup per sequence for the coarse levels of a tracking batch (lsdhip_tracker_set_batch_coarse_min_jobs) frees the chip for the
  // mapping launches beside it: worth it from the library's default (24 sequences) where tracking runs beside mapping, from twice as
  // many where nothing runs beside the batch (measured: profiles/r06_notes.md section 21).  tracker.setBatchCoarseMinJobs overrides.
  static int coarseMinJobs(bool pipelined) {
    lsdhip_build_defaults_t d;
    lsdhip_build_defaults(&d);
    return pipelined ? d.batch_coarse_min_jobs : 2 * d.batch_coarse_min_jobs;
  }
  void setPipelined(bool on) {
    if (frameId_ != 0) throw Error(LSDHIP_E_STATE, "SlamLoopBatch::setPipelined: switch before the first step");
    cam_.context()->setPipeline(on);
    pipelined_ = on;
    tracker.setBatchCoarseMinJobs(coarseMinJobs(on));
    for (auto& q : seqs_) { q->trackKF = q->keyframe; q->pendingKF.reset(); }
    if (on) tracker.setEnqueueHook([this]() {
      // the tracking batch's launches are queued: now the mapping work of the previous step, then the next step's frames
      flush();
      if (!pendingNext_) return;
      prefetched_ = makeFrames(pendingNext_, frameId_ + 1);
      prefetchedId_ = frameId_ + 1;
    });
    else tracker.setEnqueueHook(nullptr);
  }
  bool pipelined() const { return pipelined_; }
  // one frame of every sequence that is still tracking (images[s] is ignored for lost ones); returns frameToKeyframe per sequence.
  // nextImages (optional, pipelined loops): the images of the following step() call — their upload / pyramids are queued on the mapping
  // stream AHEAD of this step's mapping work, so that the next tracking batch does not wait behind it
  std::vector<SE3> step(const unsigned char* const* images, const unsigned char* const* nextImages = nullptr) {
    frameId_++;
    std::vector<std::shared_ptr<Frame>> frames;
    if (prefetchedId_ == frameId_ && (int)prefetched_.size() == size()) frames = std::move(prefetched_);
    else frames = makeFrames(images, frameId_);
    prefetched_.clear();
    prefetchedId_ = -1;
    std::vector<SE3> out((size_t)size());
    MapWork work = track(frames, out, nextImages);
    // One stream: the step's mapping iterations follow its tracking batch.  Pipelined: they are queued from the NEXT tracking batch's
    // enqueue hook (or flush()): the host's enqueueing of ~10^2 launches then lies under that batch, and so does the device work
    if (pipelined_) deferred_ = std::move(work);
    else mapGroup(work);
    return out;
  }
  // queues the mapping work the last step left (a pipelined loop keeps it back for the next tracking batch's enqueue hook); call after the
  // last step() before reading maps or statistics
  void flush() { MapWork w = std::move(deferred_); deferred_ = MapWork(); mapGroup(w); }
  // Per-sequence output: sinks[s] (null: none) receives every keyframe sequence s finalises at a keyframe change, with camToWorld =
  // poseOf(s, keyframe).  The keyframes that change in one step go into ONE PointCloud::appendBatch queued behind the keyframe change;
  // nothing waits.  The clouds must be pairwise different and outlive the loop's use of them.
  void setCloudSinks(std::vector<PointCloud*> sinks, std::function<Sim3(int, Frame&)> poseOf) {
    if (!sinks.empty() && ((int)sinks.size() != size() || !poseOf)) throw Error(LSDHIP_E_ARG, "SlamLoopBatch::setCloudSinks: one sink per sequence and a pose function");
    cloudSinks_ = std::move(sinks);
    cloudPoseOf_ = std::move(poseOf);
  }
  float cloudScaledTH = 1.f, cloudAbsTH = 1.f;   // thresholds of the sinks' appends (the viewer's defaults)
  int cloudMinNearSupport = 5;
  SE3Tracker tracker;
  bool keepKeyframes = false;         // keep every promoted keyframe alive in its sequence's keyframeLog (validation: rescale factors, point counts)
  bool sharedKeyframeChange = true;   // the keyframe changes of a step in shared launches (DepthMap::changeKeyframeBatch); false: per-sequence
                                      // finalizeKeyFrame + createKeyFrame call chains, dealt to keyframeLanes streams (rounds 2-4)
  int keyframeLanes = 8;      // (per-sequence chains) streams the keyframe changes of one step are dealt to (1: all on the context's stream)

 private:
  struct MapWork {            // what a tracking batch leaves for the mapping side
    std::vector<DepthMap*> updMaps;
    std::vector<std::shared_ptr<Frame>> updFrames;
    std::vector<int> updSeq;
    std::vector<std::pair<int, std::shared_ptr<Frame>>> kfChange;   // (sequence, its new keyframe)
  };
  // new frames of the sequences that are still tracking (null entries for lost ones)
  std::vector<std::shared_ptr<Frame>> makeFrames(const unsigned char* const* images, int frameId) {
    std::vector<int> ids;
    std::vector<const unsigned char*> imgs;
    for (int s = 0; s < size(); s++) if (!seqs_[s]->trackingLost) { ids.push_back(idOf(s, frameId)); imgs.push_back(images[s]); }
    std::vector<std::shared_ptr<Frame>> out((size_t)size());
    if (ids.empty()) return out;
    std::vector<std::shared_ptr<Frame>> made = cam_.frames(ids, imgs.data());
    size_t k = 0;
    for (int s = 0; s < size(); s++) if (!seqs_[s]->trackingLost) out[(size_t)s] = made[k++];
    return out;
  }
  // SlamSystem::trackFrame for every sequence still tracking in shared launches + the decisions of doMappingIteration; the device work
  // of the mapping iterations is returned, not queued.  The two execution models differ per sequence only in LoopSequence::tracked
  // (import before tracking against adoption after it), and in when the caller queues the returned work.
  MapWork track(const std::vector<std::shared_ptr<Frame>>& groupFrames, std::vector<SE3>& out, const unsigned char* const* nextImages) {
    MapWork work;
    std::vector<int> alive;
    std::vector<std::shared_ptr<Frame>> frames, trackedOn;
    std::vector<TrackingReference*> refs;
    std::vector<Frame*> frs;
    std::vector<SE3> inits;
    for (int s = 0; s < size(); s++) {
      Sequence& q = *seqs_[s];
      if (q.trackingLost || !groupFrames[s]) continue;
      if (!pipelined_) q.importIfUpdated(*q.trackKF);
      alive.push_back(s); frames.push_back(groupFrames[s]); trackedOn.push_back(q.trackKF);
      refs.push_back(&q.reference); frs.push_back(groupFrames[s].get()); inits.push_back(q.lastFrameToKF);
    }
    if (alive.empty()) { flush(); return work; }
    pendingNext_ = nextImages;
    std::vector<lsdhip_track_result> res;
    std::vector<SE3> est = tracker.trackFrameBatch(refs, frs, inits, res);    // (pipelined: the enqueue hook queues the previous step's mapping and the next frames)
    pendingNext_ = nullptr;
    for (size_t k = 0; k < alive.size(); k++) {
      Sequence& q = *seqs_[alive[k]];
      q.last = res[k];
      out[alive[k]] = est[k];
      // a lost sequence is marked and feeds no sink, the others go on (SlamLoop reports the loss and calls its output hooks)
      const LoopSequence::MappingStep next = q.tracked(
          pipelined_, trackedOn[k], *frames[k], est[k], res[k].diverged != 0, res[k].trackingWasGood != 0, res[k].numEvaluations, [] {},
          [&] { return LoopSequence::relativePose(*q.pendingKF, *frames[k]); }, [&] { return lsd_slam::loop::wantsNewKeyframe(kfEvery_, q.sinceKF); });
      if (next == LoopSequence::MappingStep::KeyframeChange) {
        work.kfChange.emplace_back(alive[k], frames[k]);
      } else if (next == LoopSequence::MappingStep::Update) {
        work.updMaps.push_back(&q.map); work.updFrames.push_back(frames[k]); work.updSeq.push_back(alive[k]);
      }
    }
    return work;
  }
  // the mapping iterations a tracking batch left: updateKeyframe of all its sequences in shared launches, then the keyframe changes —
  // per-sequence call chains (finalizeKeyFrame + createKeyFrame, ~18 small dependent launches each), independent of each other: on a
  // one-stream context dealt to `keyframeLanes` streams, and queued AFTER the shared launches so that the host's enqueueing lies under them
  void mapGroup(MapWork& work) {
    if (work.updMaps.empty() && work.kfChange.empty()) return;
    std::shared_ptr<Context> ctx = cam_.context();
    const int nkf = (int)work.kfChange.size();
    const int lanes = !sharedKeyframeChange && keyframeLanes > 1 && nkf > 0 ? (keyframeLanes < nkf ? keyframeLanes : nkf) : 0;
    // (closed by the destructor too: an exception from one of the calls below must not leave the context inside a lane region)
    struct LaneRegion {
      Context* c; bool open;
      LaneRegion(Context* c_, int n) : c(c_), open(n > 0) { if (open) c->lanesBegin(n); }
      void end() { if (open) { open = false; c->lanesEnd(); } }
      ~LaneRegion() { if (open) { try { c->lanesEnd(); } catch (...) {} } }
    } region(ctx.get(), lanes);
    std::vector<Frame*> updFrames;
    for (auto& f : work.updFrames) updFrames.push_back(f.get());
    DepthMap::updateKeyframeBatch(work.updMaps, updFrames);
    if (sharedKeyframeChange && nkf > 0) {
      // all keyframe changes of the step in six launches
      std::vector<DepthMap*> kfMaps;
      std::vector<Frame*> kfFrames;
      for (int i = 0; i < nkf; i++) { kfMaps.push_back(&seqs_[work.kfChange[i].first]->map); kfFrames.push_back(work.kfChange[i].second.get()); }
      DepthMap::changeKeyframeBatch(kfMaps, kfFrames);
    }
    std::vector<std::shared_ptr<Frame>> finished;     // the keyframes this step finalises, for the cloud sinks
    std::vector<PointCloud*> sinkClouds;
    std::vector<Sim3> sinkPoses;
    for (int i = 0; i < nkf; i++) {
      Sequence& q = *seqs_[work.kfChange[i].first];
      const std::shared_ptr<Frame>& frame = work.kfChange[i].second;
      if (!cloudSinks_.empty() && cloudSinks_[(size_t)work.kfChange[i].first]) {
        finished.push_back(q.keyframe);
        sinkClouds.push_back(cloudSinks_[(size_t)work.kfChange[i].first]);
        sinkPoses.push_back(cloudPoseOf_(work.kfChange[i].first, *q.keyframe));
      }
      if (lanes) ctx->laneSelect(i % lanes);
      if (!sharedKeyframeChange) { q.map.finalizeKeyFrame(); q.map.createKeyFrame(frame.get()); }
      if (keepKeyframes && q.keyframeLog.empty() && !q.replacedFirst) q.replacedFirst = q.keyframe;
      q.promote(frame, pipelined_, keepKeyframes, true);
    }
    region.end();
    if (!finished.empty()) {
      std::vector<Frame*> fs;
      for (auto& f : finished) fs.push_back(f.get());
      PointCloud::appendBatch(sinkClouds, fs, sinkPoses, cloudScaledTH, cloudAbsTH, cloudMinNearSupport);
    }
    for (size_t k = 0; k < work.updSeq.size(); k++) seqs_[work.updSeq[k]]->mapped(*work.updFrames[k]);
  }
  std::vector<PointCloud*> cloudSinks_;
  std::function<Sim3(int, Frame&)> cloudPoseOf_;
  bool pipelined_ = false;
  std::vector<std::shared_ptr<Frame>> prefetched_;
  int prefetchedId_ = -1;
  const unsigned char* const* pendingNext_ = nullptr;
  MapWork deferred_;
  LoopCamera cam_;
  int kfEvery_, frameId_ = 0;
  std::vector<std::unique_ptr<Sequence>> seqs_;
};

}  // namespace lsd_slam_hip
#endif  // LSD_SLAM_HIP_HPP
