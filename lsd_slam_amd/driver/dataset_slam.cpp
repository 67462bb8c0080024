// dataset_slam — the image-folder driver of the reference (lsd_slam_core/src/main_on_images.cpp:128-279) without ROS:
// calibration file + list of PGM images -> random initialisation on the first image, trackFrame + mapping for the rest
// (doSlam = false, blockUntilMapped = true, keyframes chosen by the reference's distance / usage score), on the GPU
// through include/lsd_slam_hip.hpp.  Outputs: a trajectory text file, one keyframeMsg (ROS 1 wire format) per finished
// keyframe, and the viewer's PLY point cloud.
//
//   dataset_slam <calib.cfg> <image_list.txt> <out_dir> [--kf-every N] [--device D] [--constraints 1] [--cloud host|device|both]
//                [--cloud-capacity POINTS] [--depth-images DIR [--debug-display N]] [--reactivate N] [--undistort 1 [--rectified-images DIR]]
//
// --undistort 1: the calibration file may be any FOV-model file of the reference (Undistorter::fromFile: distortion, crop / full / explicit
//   output intrinsics, resizing — what UndistorterPTAM reads, C/util/Undistorter.cpp:91-345), the PGMs are RAW camera images of the file's input
//   size, and the loop is fed the raw bytes: every frame is rectified on the device inside frame creation (DeviceUndistorter).  The calibration
//   of the rectified images is written to <out_dir>/rectified.cfg.  Without the flag such a file is refused, as before.
// --rectified-images DIR (with --undistort 1): the rectified image of every frame is also written to DIR/<file name> (one extra launch and a
//   copy per frame: lsdhip_undistorter_apply).
// --cloud host (default): pc.ply and keyframe_<id>.msg from the host functions (three plane downloads and a host loop per keyframe).
// --cloud device: every finished keyframe is appended to one PointCloud on the GPU behind the keyframe change (no split of the change; the
//   append waits for nothing), downloaded once at the end into pc.ply; keyframe_<id>.msg comes from makeKeyframeMsgDevice, which does
//   wait once per keyframe: the file needs the payload on the host (one launch and one copy of 12 bytes per pixel).
// --cloud both: the host path writes pc.ply / keyframe_<id>.msg and the device path pc_device.ply / keyframe_<id>_device.msg, in the same
//   run on the same keyframes: the like-for-like mode (a host run and a device run go through different keyframe-change paths, whose
//   rescale factors differ in the last bits).
// --depth-images DIR: after every mapping iteration the depth map's debug image (DepthMap::debugPlotDepthMap, drawn on the device: the
//   keyframe in grey, the hypotheses in the colours of --debug-display N, the reference's debugDisplay 0 .. 5, default 0) is written to
//   DIR/depth_<frame id>.ppm.  A file writer may wait: this is the host-output form, one launch and a copy of 3 bytes per pixel per frame.
// --reactivate N (default 0 = off): finished keyframes are kept in a device bank of N slots and a keyframe change goes back to a banked
//   keyframe where TrackableKeyFrameSearch::findRePositionCandidate finds one (SlamLoop::enableReactivation; C/SlamSystem.cpp:507-540).
//   One line per re-activation on stdout, and the totals at the end.  A keyframe that is finished a second time is output a second time.
// --constraints 1 additionally aligns every new keyframe with the keyframe it replaces by Sim3Tracker::trackFrameSim3 (the
// tracking-parent edge the reference's constraint search always tests, C/SlamSystem.cpp:1253-1262) and writes constraints.txt.
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>

#include "../../include/lsd_slam_hip_io.hpp"

using namespace lsd_slam_hip;

// camToWorld of a frame = camToWorld(parent keyframe) * thisToParent (Sim3 composition; scale only changes at keyframes)
static Sim3 sim3_mul(const Sim3& a, const Sim3& b) {
  Sim3 r;
  r.q[0] = a.q[0] * b.q[0] - a.q[1] * b.q[1] - a.q[2] * b.q[2] - a.q[3] * b.q[3];
  r.q[1] = a.q[0] * b.q[1] + a.q[1] * b.q[0] + a.q[2] * b.q[3] - a.q[3] * b.q[2];
  r.q[2] = a.q[0] * b.q[2] + a.q[2] * b.q[0] + a.q[3] * b.q[1] - a.q[1] * b.q[3];
  r.q[3] = a.q[0] * b.q[3] + a.q[3] * b.q[0] + a.q[1] * b.q[2] - a.q[2] * b.q[1];
  const double* q = a.q;
  const double v[3] = {b.t[0] * a.s, b.t[1] * a.s, b.t[2] * a.s};
  const double ux = 2 * (q[2] * v[2] - q[3] * v[1]), uy = 2 * (q[3] * v[0] - q[1] * v[2]), uz = 2 * (q[1] * v[1] - q[2] * v[0]);
  r.t[0] = v[0] + q[0] * ux + (q[2] * uz - q[3] * uy) + a.t[0];
  r.t[1] = v[1] + q[0] * uy + (q[3] * ux - q[1] * uz) + a.t[1];
  r.t[2] = v[2] + q[0] * uz + (q[1] * uy - q[2] * ux) + a.t[2];
  r.s = a.s * b.s;
  return r;
}

int main(int argc, char** argv) {
  if (argc < 4) {
    std::cerr << "usage: dataset_slam <calib.cfg> <image_list.txt> <out_dir> [--kf-every N] [--device D] [--constraints 1] [--cloud host|device|both] [--cloud-capacity POINTS] [--depth-images DIR [--debug-display N]] [--reactivate N] [--undistort 1 [--rectified-images DIR]]\n";
    return 2;
  }
  int kfEvery = 0, device = 0, constraints = 0, debugDisplay = 0, reactivate = 0, undistort = 0;
  std::string cloudMode = "host", depthImages, rectifiedImages;
  long long cloudCapacity = 0;
  for (int i = 4; i + 1 < argc; i += 2) {
    if (!strcmp(argv[i], "--kf-every")) kfEvery = atoi(argv[i + 1]);
    if (!strcmp(argv[i], "--device")) device = atoi(argv[i + 1]);
    if (!strcmp(argv[i], "--constraints")) constraints = atoi(argv[i + 1]);
    if (!strcmp(argv[i], "--cloud")) cloudMode = argv[i + 1];
    if (!strcmp(argv[i], "--cloud-capacity")) cloudCapacity = atoll(argv[i + 1]);
    if (!strcmp(argv[i], "--depth-images")) depthImages = argv[i + 1];
    if (!strcmp(argv[i], "--debug-display")) debugDisplay = atoi(argv[i + 1]);
    if (!strcmp(argv[i], "--reactivate")) reactivate = atoi(argv[i + 1]);
    if (!strcmp(argv[i], "--undistort")) undistort = atoi(argv[i + 1]);
    if (!strcmp(argv[i], "--rectified-images")) rectifiedImages = argv[i + 1];
  }
  if (cloudMode != "host" && cloudMode != "device" && cloudMode != "both") { std::cerr << "--cloud takes host, device or both\n"; return 2; }
  const bool hostCloud = cloudMode != "device", devCloud = cloudMode != "host";
  try {
    // --undistort 1: raw images of the file's input size, rectified on the device; cal describes the rectified images either way
    Calibration cal;
    int inW = 0, inH = 0;
    std::shared_ptr<DeviceUndistorter> dundist;
    if (undistort) {
      const Undistorter u = Undistorter::fromFile(argv[1]);
      cal.width = u.out_width; cal.height = u.out_height; cal.K = u.K;
      inW = u.in_width; inH = u.in_height;
      Context::defaultDevice() = device;
      if (!u.passThrough()) dundist = std::make_shared<DeviceUndistorter>(inW, inH, cal.width, cal.height, cal.K, u.remapX.data(), u.remapY.data());
      std::ofstream rc(std::string(argv[3]) + "/rectified.cfg");
      rc << u.rectifiedCalibrationText();
    } else {
      cal = parseCalibration(argv[1]);
      inW = cal.width; inH = cal.height;
    }
    std::vector<std::string> files;
    {
      std::ifstream f(argv[2]);
      std::string line;
      while (std::getline(f, line)) if (!line.empty()) files.push_back(line);
    }
    if (files.empty()) { std::cerr << "no images listed in " << argv[2] << "\n"; return 2; }
    const std::string outDir = argv[3];
    Context::defaultDevice() = device;
    const int w = cal.width, h = cal.height;
    std::vector<unsigned char> img;
    if (!readPGM(files[0], inW, inH, img)) { std::cerr << "cannot read " << files[0] << " as " << inW << "x" << inH << " P5\n"; return 2; }
    // --rectified-images: the rectified bytes of the image just read, under its own file name
    std::vector<unsigned char> rect;
    auto dumpRectified = [&](const std::string& file) {
      if (rectifiedImages.empty() || !undistort) return;
      const unsigned char* bytes = img.data();
      if (dundist) { rect.resize((size_t)w * h); dundist->undistort(img.data(), false, rect.data(), false); bytes = rect.data(); }
      const std::string path = rectifiedImages + "/" + file.substr(file.find_last_of('/') + 1);
      if (!writePGM(path, w, h, bytes)) std::cerr << "dataset_slam: cannot write " << path << "\n";
    };
    dumpRectified(files[0]);
    // The context exists before the seed is set: bringing up the HIP runtime draws from rand() itself, a varying number of times, and a loop
    // whose context was created behind srand(0) started from a different random depth map in every run.
    const std::shared_ptr<Context> ctx = Context::get(w, h, cal.K);
    ctx->synchronize();
    srand(0);   // initializeRandomly draws from rand() in pixel order (DepthMap.cpp:883-916)
    std::unique_ptr<SlamLoop> loopOwner(dundist ? new SlamLoop(w, h, cal.K, dundist, img.data(), false, nullptr, kfEvery)
                                                : new SlamLoop(w, h, cal.K, img.data(), false, nullptr, kfEvery));
    SlamLoop& loop = *loopOwner;
    if (reactivate > 0) loop.enableReactivation(reactivate);
    std::ofstream traj(outDir + "/trajectory.txt");
    traj << "# frame keyframe frameToKeyframe(qw qx qy qz tx ty tz) camToWorld(qw qx qy qz tx ty tz s) pointUsage goodRatio trackingWasGood\n";
    Sim3 kfToWorld;   // identity
    std::vector<float> cloud;
    int nKeyframes = 0;
    int keyframeId = 0;
    auto writeMsg = [&](const KeyframeMsg& m, const std::string& suffix) {
      const std::vector<unsigned char> wire = serializeKeyframeMsg(m);
      std::ofstream f(outDir + "/keyframe_" + std::to_string(m.id) + suffix + ".msg", std::ios::binary);
      f.write((const char*)wire.data(), (std::streamsize)wire.size());
    };
    // device cloud: at most one point per pixel and keyframe; the default capacity covers that up to 2^26 points (1 GiB)
    std::unique_ptr<PointCloud> dcloud;
    if (devCloud) {
      long long cap = cloudCapacity > 0 ? cloudCapacity : (long long)files.size() * w * h;
      if (cloudCapacity <= 0 && cap > (1ll << 26)) cap = 1ll << 26;
      dcloud.reset(new PointCloud(Context::get(w, h, cal.K), cap, (int)files.size()));
    }
    if (hostCloud) loop.onKeyframeFinished = [&](Frame& kf, DepthMap&) {
      KeyframeMsg m = makeKeyframeMsg(kf, kfToWorld, cal.K);
      writeMsg(m, "");
      flushPointCloud(m, cloud);
      nKeyframes++;
    };
    // behind the keyframe change, with the keyframe that was just finalised (kfToWorld is still its pose): the append only queues work;
    // writing the message file WAITS for the device (the payload has to reach the host: one launch and one copy)
    if (devCloud) loop.onKeyframeFinishedAsync = [&](Frame& kf) {
      dcloud->appendKeyframe(kf, kfToWorld);
      writeMsg(makeKeyframeMsgDevice(kf, kfToWorld, cal.K), hostCloud ? "_device" : "");
      if (!hostCloud) nKeyframes++;
    };
    int currentFrame = 0;      // id of the frame whose step() is running
    if (!depthImages.empty()) loop.onMappingIteration = [&](DepthMap& map) {
      map.debugPlotDepthMap(debugDisplay);
      const std::string path = depthImages + "/depth_" + std::to_string(currentFrame) + ".ppm";
      if (!writePPM(path, w, h, map.debugImageDepth.data())) std::cerr << "dataset_slam: cannot write " << path << "\n";
    };
    int good = 0, nConstraints = 0;
    std::unique_ptr<Sim3Tracker> sim3;
    std::ofstream cons;
    if (constraints) {
      sim3.reset(new Sim3Tracker(w, h, cal.K));
      cons.open(outDir + "/constraints.txt");
      cons << "# parentKeyframe newKeyframe init(qw qx qy qz tx ty tz s) estimate(qw qx qy qz tx ty tz s) residual depthResidual photoResidual usage diverged\n";
    }
    for (size_t i = 1; i < files.size(); i++) {
      if (!readPGM(files[i], inW, inH, img)) { std::cerr << "skipping " << files[i] << " (wrong size or unreadable)\n"; continue; }
      dumpRectified(files[i]);
      std::shared_ptr<Frame> parentKF = loop.keyframe;
      currentFrame = (int)i;
      SE3 f2k = loop.step(img.data());
      const bool reactivated = loop.newKeyframe && loop.reactivateKeyframes && loop.keyframeChanges.back().reactivated;
      if (reactivated) {
        const SlamLoop::KeyframeChange& c = loop.keyframeChanges.back();
        std::cout << "reactivated frame " << c.frameId << " keyframe " << c.previousKfId << " -> " << c.newKfId << " potential " << c.numPotential
                  << " checked " << c.numChecked << " tracked " << c.numTracked << "\n";
      }
      if (constraints && loop.newKeyframe && !reactivated) {
        // new keyframe -> replaced keyframe, starting from the tracked pose with the depth rescale as scale
        TrackingReference parentRef;
        parentRef.importFrame(parentKF.get());
        const Sim3 init = loop.keyframe->thisToParent_raw();
        const Sim3 est = sim3->trackFrameSim3(&parentRef, loop.keyframe.get(), init, 3, 1);
        cons << parentKF->id() << " " << loop.keyframe->id();
        for (int k = 0; k < 4; k++) cons << " " << init.q[k];
        for (int k = 0; k < 3; k++) cons << " " << init.t[k];
        cons << " " << init.s;
        for (int k = 0; k < 4; k++) cons << " " << est.q[k];
        for (int k = 0; k < 3; k++) cons << " " << est.t[k];
        cons << " " << est.s << " " << sim3->lastResidual << " " << sim3->lastDepthResidual << " " << sim3->lastPhotometricResidual << " "
             << sim3->pointUsage << " " << (sim3->diverged ? 1 : 0) << "\n";
        nConstraints++;
      }
      Sim3 rel;
      for (int k = 0; k < 4; k++) rel.q[k] = f2k.q[k];
      for (int k = 0; k < 3; k++) rel.t[k] = f2k.t[k];
      Sim3 c2w = sim3_mul(kfToWorld, rel);
      if (reactivated) {
        // a banked keyframe came back: its pose is the one it was finished with
        const std::array<double, 8>& p = loop.worldPose(*loop.keyframe);
        for (int k = 0; k < 4; k++) kfToWorld.q[k] = p[k];
        for (int k = 0; k < 3; k++) kfToWorld.t[k] = p[4 + k];
        kfToWorld.s = p[7];
      } else if (loop.newKeyframe) {
        // the new keyframe's pose relative to its parent now carries the depth rescale (DepthMap.cpp:1305)
        Sim3 tp = loop.keyframe->thisToParent_raw();
        kfToWorld = sim3_mul(kfToWorld, tp);
        c2w = kfToWorld;
      }
      const float gr = loop.tracker.lastGoodCount / (loop.tracker.lastGoodCount + loop.tracker.lastBadCount);
      traj << i << " " << keyframeId << " " << f2k.q[0] << " " << f2k.q[1] << " " << f2k.q[2] << " " << f2k.q[3] << " " << f2k.t[0] << " "
           << f2k.t[1] << " " << f2k.t[2] << " " << c2w.q[0] << " " << c2w.q[1] << " " << c2w.q[2] << " " << c2w.q[3] << " " << c2w.t[0] << " "
           << c2w.t[1] << " " << c2w.t[2] << " " << c2w.s << " " << loop.tracker.pointUsage << " " << gr << " " << (loop.tracker.trackingWasGood ? 1 : 0) << "\n";
      if (loop.newKeyframe) keyframeId = loop.keyframe->id();
      good += loop.tracker.trackingWasGood ? 1 : 0;
    }
    // the last keyframe: SlamSystem::finalize -> finishCurrentKeyframe
    loop.map.finalizeKeyFrame();
    if (hostCloud) loop.onKeyframeFinished(*loop.keyframe, loop.map);
    if (devCloud) loop.onKeyframeFinishedAsync(*loop.keyframe);
    long long points = (long long)cloud.size() / 4;
    if (hostCloud) writePLY(outDir + "/pc.ply", cloud);
    if (devCloud) {
      const long long total = dcloud->total(), stored = dcloud->stored();
      if (total > stored) std::cerr << "dataset_slam: the device cloud holds " << stored << " of " << total << " points (--cloud-capacity)\n";
      writePLY(outDir + (hostCloud ? "/pc_device.ply" : "/pc.ply"), dcloud->download());
      std::ofstream seg(outDir + (hostCloud ? "/segments_device.txt" : "/segments.txt"));
      seg << "# keyframe first count\n";
      for (const PointCloud::Segment& sg : dcloud->segments()) seg << sg.id << " " << sg.first << " " << sg.count << "\n";
      if (!hostCloud) points = stored;
    }
    std::cout << "frames " << files.size() - 1 << " tracked_good " << good << " keyframes " << nKeyframes << " points " << points
              << " constraints " << nConstraints;
    if (reactivate > 0) std::cout << " reactivations " << loop.numReactivations << " unbanked " << loop.numUnbanked;
    std::cout << "\n";
    return 0;
  } catch (const Error& e) {
    std::cerr << "dataset_slam: " << e.what() << "\n";
    return 1;
  }
}
