// Runs plotDepthMap of include/lsd_slam_hip_io.hpp — the host yardstick of DepthMap::debugPlotDepthMap — on a map and an image read from
// a file, without a GPU, for every debugDisplay mode 0 .. 6: what tests/depth_plot_ref.py is pinned to (tests/test_depth_plot_ref_cpu.py).
//   in:  int32 w, h, refID; then w * h hypotheses (32 bytes each), then the image plane (float)
//   out: <prefix>.<mode>.ppm for mode 0 .. 6
#include <cstdio>
#include <string>
#include <vector>
#include "lsd_slam_hip_io.hpp"
using namespace lsd_slam_hip;
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[3];
  if (fread(hdr, 4, 3, f) != 3) return 2;
  const int w = hdr[0], h = hdr[1], refID = hdr[2];
  const size_t n = (size_t)w * h;
  std::vector<lsdhip_hypothesis> map(n);
  std::vector<float> img(n);
  if (fread(map.data(), sizeof(lsdhip_hypothesis), n, f) != n || fread(img.data(), 4, n, f) != n) return 2;
  fclose(f);
  std::vector<unsigned char> out(n * 3);
  for (int mode = 0; mode <= 6; mode++) {
    plotDepthMap(map.data(), img.data(), w, h, mode, refID, out.data());
    if (!writePPM(std::string(argv[2]) + "." + std::to_string(mode) + ".ppm", w, h, out.data())) return 1;
  }
  return 0;
}
