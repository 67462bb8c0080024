// Runs the host export of include/lsd_slam_hip_io.hpp — the payload fill of makeKeyframeMsg, serializeKeyframeMsg, flushPointCloud — on
// planes read from a file, without a GPU: the yardstick tests/cloud_ref.py is pinned to (tests/test_cloud_ref_cpu.py).
//   in:  int32 w, h, minNearSupport; float fx, fy, cx, cy, camToWorld[7], scaledTH, absTH; then idepth, idepthVar, image planes (float)
//   out: <prefix>.msg (wire bytes), <prefix>.pts (x y z intensity floats)
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
  float par[13];
  if (fread(hdr, 4, 3, f) != 3 || fread(par, 4, 13, f) != 13) return 2;
  const int w = hdr[0], h = hdr[1], minNearSupport = hdr[2];
  const size_t n = (size_t)w * h;
  std::vector<float> id(n), var(n), img(n);
  if (fread(id.data(), 4, n, f) != n || fread(var.data(), 4, n, f) != n || fread(img.data(), 4, n, f) != n) return 2;
  fclose(f);
  KeyframeMsg m;
  m.id = 3; m.time = 0.5;
  m.fx = par[0]; m.fy = par[1]; m.cx = par[2]; m.cy = par[3];
  for (int i = 0; i < 7; i++) m.camToWorld[i] = par[4 + i];
  m.width = (uint32_t)w; m.height = (uint32_t)h;
  m.pointcloud.resize(n);
  for (size_t i = 0; i < n; i++) {     // makeKeyframeMsg's loop
    m.pointcloud[i].idepth = id[i];
    m.pointcloud[i].idepth_var = var[i];
    const unsigned char c = (unsigned char)img[i];
    m.pointcloud[i].color[0] = m.pointcloud[i].color[1] = m.pointcloud[i].color[2] = m.pointcloud[i].color[3] = c;
  }
  const std::vector<unsigned char> wire = serializeKeyframeMsg(m);
  const std::string prefix = argv[2];
  f = fopen((prefix + ".msg").c_str(), "wb");
  fwrite(wire.data(), 1, wire.size(), f);
  fclose(f);
  std::vector<float> xyzi;
  const int num = flushPointCloud(m, xyzi, par[11], par[12], minNearSupport);
  f = fopen((prefix + ".pts").c_str(), "wb");
  fwrite(xyzi.data(), 4, xyzi.size(), f);
  fclose(f);
  printf("points %d\n", num);
  return 0;
}
