// The depth map's debug image without the device plot, timed: lsdhip_depth_download (the 32-byte AoS map, eight plane copies and a wait for
// the mapping stream) + the keyframe's level-0 image (fetched once: it does not change) + plotDepthMap on the host — the "today's path"
// leg of tools/bench_depth_plot.py, which builds and runs this program.  Beside it the device plot through the C++ class, for a like-for-like
// host clock: DepthMap::debugPlotDepthMap (launch + copy of 3 bytes per pixel + wait).
//   bench_depth_plot_host <input> <regions> <reps> <debugDisplay>
//   input: int32 w, h, n; float K4[4]; w*h float depth of frame 0; n frames of w*h uint8
// Prints one JSON object: median seconds per image.
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
  if (argc < 5) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[3];
  float K4[4];
  if (fread(hdr, 4, 3, f) != 3 || fread(K4, 4, 4, f) != 4) return 2;
  const int w = hdr[0], h = hdr[1], n = hdr[2], regions = atoi(argv[2]), reps = atoi(argv[3]), mode = atoi(argv[4]);
  const size_t npix = (size_t)w * h;
  std::vector<float> depth0(npix);
  std::vector<unsigned char> imgs(npix * n);
  if (fread(depth0.data(), 4, npix, f) != npix || fread(imgs.data(), 1, imgs.size(), f) != imgs.size()) return 2;
  fclose(f);
  try {
    const Mat3f K = Mat3f::intrinsics(K4[0], K4[1], K4[2], K4[3]);
    SlamLoop loop(w, h, K, imgs.data(), false, depth0.data(), 1 << 20);
    for (int i = 1; i < n; i++) loop.step(imgs.data() + npix * i);
    Context::get(w, h, K)->synchronize();
    const std::vector<float> image = loop.keyframe->image(0);
    const int refID = n - 1;      // the last update's frame
    std::vector<unsigned char> host(npix * 3);
    std::vector<double> whole, dl, plot, dev;
    for (int r = 0; r < regions; r++) {
      double td = 0, tp = 0, tv = 0;
      for (int k = 0; k < reps; k++) {
        const double t0 = now();
        const std::vector<lsdhip_hypothesis> map = loop.map.currentDepthMap();
        const double t1 = now();
        plotDepthMap(map.data(), image.data(), w, h, mode, refID, host.data());
        const double t2 = now();
        loop.map.debugPlotDepthMap(mode);
        const double t3 = now();
        td += t1 - t0; tp += t2 - t1; tv += t3 - t2;
      }
      dl.push_back(td / reps); plot.push_back(tp / reps); whole.push_back((td + tp) / reps); dev.push_back(tv / reps);
    }
    const bool same = host == loop.map.debugImageDepth;
    printf("{\"host_path_s\": %.9g, \"download_s\": %.9g, \"plotDepthMap_s\": %.9g, \"device_plot_and_copy_s\": %.9g, \"images_equal\": %s}\n", median(whole),
           median(dl), median(plot), median(dev), same ? "true" : "false");
    return same ? 0 : 3;
  } catch (const Error& e) {
    fprintf(stderr, "bench_depth_plot_host: %s\n", e.what());
    return 1;
  }
}
