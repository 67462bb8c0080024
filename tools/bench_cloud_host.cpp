// The existing host export path per keyframe, timed: makeKeyframeMsg (three level-0 plane downloads, each draining the context, and the
// 12-byte fill loop) + flushPointCloud, on a finalised map — leg (a) of tools/bench_cloud.py, which builds and runs this program.
//   bench_cloud_host <input> <regions> <reps>
//   input: int32 w, h, n; float K4[4]; w*h float depth of frame 0; n frames of w*h uint8
// Prints one JSON object: median seconds per keyframe of the whole path and of its two halves.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../include/lsd_slam_hip_io.hpp"
using namespace lsd_slam_hip;
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }
int main(int argc, char** argv) {
  if (argc < 4) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[3];
  float K4[4];
  if (fread(hdr, 4, 3, f) != 3 || fread(K4, 4, 4, f) != 4) return 2;
  const int w = hdr[0], h = hdr[1], n = hdr[2], regions = atoi(argv[2]), reps = atoi(argv[3]);
  const size_t npix = (size_t)w * h;
  std::vector<float> depth0(npix);
  std::vector<unsigned char> imgs(npix * n);
  if (fread(depth0.data(), 4, npix, f) != npix || fread(imgs.data(), 1, imgs.size(), f) != imgs.size()) return 2;
  fclose(f);
  try {
    const Mat3f K = Mat3f::intrinsics(K4[0], K4[1], K4[2], K4[3]);
    SlamLoop loop(w, h, K, imgs.data(), false, depth0.data(), 1 << 20);
    for (int i = 1; i < n; i++) loop.step(imgs.data() + npix * i);
    loop.map.finalizeKeyFrame();
    Context::get(w, h, K)->synchronize();
    Sim3 pose;
    pose.q[0] = 0.97; pose.q[1] = 0.1; pose.q[2] = -0.2; pose.q[3] = 0.05;
    pose.t[0] = 0.5; pose.t[1] = -1.0; pose.t[2] = 2.0;
    std::vector<double> whole, msg, flush;
    std::vector<float> cloud;
    size_t points = 0;
    for (int r = 0; r < regions; r++) {
      double tm = 0, tf = 0;
      for (int k = 0; k < reps; k++) {
        cloud.clear();
        const double t0 = now();
        KeyframeMsg m = makeKeyframeMsg(*loop.keyframe, pose, K);
        const double t1 = now();
        flushPointCloud(m, cloud);
        const double t2 = now();
        tm += t1 - t0; tf += t2 - t1;
        points = cloud.size() / 4;
      }
      msg.push_back(tm / reps); flush.push_back(tf / reps); whole.push_back((tm + tf) / reps);
    }
    printf("{\"host_path_s\": %.9g, \"makeKeyframeMsg_s\": %.9g, \"flushPointCloud_s\": %.9g, \"kept_points\": %zu}\n", median(whole), median(msg),
           median(flush), points);
    return 0;
  } catch (const Error& e) {
    fprintf(stderr, "bench_cloud_host: %s\n", e.what());
    return 1;
  }
}
