// Host side of tools/bench_undistort.py: what a raw frame costs until its pyramids are queued, two ways, host wall time per frame.
//   host  : lsd_slam_hip::Undistorter::undistort on one core (the scalar gather of UndistorterPTAM::undistort) + lsdhip_frame_create_async
//           of the rectified bytes — what a user of the library had to do before the device path existed;
//   device: lsdhip_frame_create_undistorted_async of the raw bytes.
// Every region creates `reps` frames and ends with lsdhip_ctx_synchronize (inside the timed window: the device work is part of the cost);
// the host gather alone is timed as well.  Built by the tool with g++ -O3 (the header keeps the gather free of contraction by itself).
//   bench_undistort_host <calib.cfg> <regions> <reps>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "lsd_slam_hip_io.hpp"
using namespace lsd_slam_hip;

static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  try {
    const Undistorter u = Undistorter::fromFile(argv[1]);
    const int regions = atoi(argv[2]), reps = atoi(argv[3]);
    const int w = u.out_width, h = u.out_height;
    std::shared_ptr<Context> ctx = Context::get(w, h, u.K);
    DeviceUndistorter du(u.in_width, u.in_height, w, h, u.K, u.remapX.data(), u.remapY.data());
    check(lsdhip_ctx_reserve_frames(ctx->handle(), 8), "lsdhip_ctx_reserve_frames");
    // one raw and one rectified buffer per frame of a region: the async creators want the bytes untouched until the context is synchronised
    const size_t rawBytes = (size_t)u.in_width * u.in_height, outBytes = (size_t)w * h;
    std::vector<std::vector<unsigned char>> raw((size_t)reps, std::vector<unsigned char>(rawBytes)), rect((size_t)reps, std::vector<unsigned char>(outBytes));
    unsigned s = 12345;
    for (auto& r : raw) for (auto& b : r) { s = s * 1664525u + 1013904223u; b = (unsigned char)(s >> 24); }
    std::vector<double> tHost, tDev, tGather;
    for (int region = -1; region < regions; region++) {      // region -1 warms both paths up
      for (int mode = 0; mode < 2; mode++) {
        std::vector<lsdhip_frame*> frames;
        const double t0 = now();
        double gather = 0;
        for (int k = 0; k < reps; k++) {
          lsdhip_frame* f = nullptr;
          if (mode == 0) {
            const double g0 = now();
            u.undistort(raw[(size_t)k].data(), rect[(size_t)k].data());
            gather += now() - g0;
            check(lsdhip_frame_create_async(ctx->handle(), k, rect[(size_t)k].data(), &f), "lsdhip_frame_create_async");
          } else {
            check(lsdhip_frame_create_undistorted_async(du.handle(), k, raw[(size_t)k].data(), &f), "lsdhip_frame_create_undistorted_async");
          }
          frames.push_back(f);
          if (frames.size() > 4) { lsdhip_frame_destroy(frames.front()); frames.erase(frames.begin()); }
        }
        ctx->synchronize();
        const double dt = now() - t0;
        for (lsdhip_frame* f : frames) lsdhip_frame_destroy(f);
        if (region < 0) continue;
        (mode == 0 ? tHost : tDev).push_back(dt / reps);
        if (mode == 0) tGather.push_back(gather / reps);
      }
    }
    printf("{\"in\": [%d, %d], \"out\": [%d, %d], \"regions\": %d, \"reps\": %d, \"host_undistort_plus_create_async_us\": %.2f, "
           "\"host_undistort_alone_us\": %.2f, \"create_undistorted_async_us\": %.2f, \"host_min_us\": %.2f, \"host_max_us\": %.2f, "
           "\"device_min_us\": %.2f, \"device_max_us\": %.2f}\n",
           u.in_width, u.in_height, w, h, regions, reps, median(tHost) * 1e6, median(tGather) * 1e6, median(tDev) * 1e6,
           *std::min_element(tHost.begin(), tHost.end()) * 1e6, *std::max_element(tHost.begin(), tHost.end()) * 1e6,
           *std::min_element(tDev.begin(), tDev.end()) * 1e6, *std::max_element(tDev.begin(), tDev.end()) * 1e6);
    return 0;
  } catch (const Error& e) {
    fprintf(stderr, "bench_undistort_host: %s\n", e.what());
    return 1;
  }
}
