// Exercises lsd_slam_hip::Undistorter (include/lsd_slam_hip_io.hpp) without a GPU.  Built with -ffp-contract=off by tests/test_undistort_cpu.py.
//   tables <cfg> <dir>             K, relative output calibration, sizes; <dir>/remapX.f32, remapY.f32 (absent: pass-through); the rectified
//                                  calibration file <dir>/rectified.cfg and whether parseCalibration reads it back to the same K
//   undistort <cfg> <raw> <out>    every in_w * in_h image of file <raw> through undistort(), appended to <out>
//   parse <cfg>                    "undistorter: ok | <message>" and "parseCalibration: ok | <message>"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "lsd_slam_hip_io.hpp"
using namespace lsd_slam_hip;

static bool dump(const std::string& path, const void* p, size_t bytes) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = fwrite(p, 1, bytes, f) == bytes;
  fclose(f);
  return ok;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const std::string cmd = argv[1];
  if (cmd == "parse") {
    try { Undistorter::fromFile(argv[2]); printf("undistorter: ok\n"); } catch (const Error& e) { printf("undistorter: %s\n", e.what()); }
    try { parseCalibration(argv[2]); printf("parseCalibration: ok\n"); } catch (const Error& e) { printf("parseCalibration: %s\n", e.what()); }
    return 0;
  }
  const Undistorter u = Undistorter::fromFile(argv[2]);
  if (cmd == "tables" && argc >= 4) {
    const std::string dir = argv[3];
    printf("size %d %d %d %d\n", u.in_width, u.in_height, u.out_width, u.out_height);
    printf("K %.9g %.9g %.9g %.9g\n", u.K.fx(), u.K.fy(), u.K.cx(), u.K.cy());
    printf("outcal %.9g %.9g %.9g %.9g %.9g\n", u.outputCalibration[0], u.outputCalibration[1], u.outputCalibration[2], u.outputCalibration[3], u.outputCalibration[4]);
    printf("passthrough %d\n", u.passThrough() ? 1 : 0);
    if (!u.passThrough()) {
      if (!dump(dir + "/remapX.f32", u.remapX.data(), u.remapX.size() * 4) || !dump(dir + "/remapY.f32", u.remapY.data(), u.remapY.size() * 4)) return 3;
    }
    const std::string text = u.rectifiedCalibrationText();
    if (!dump(dir + "/rectified.cfg", text.data(), text.size())) return 3;
    const Calibration c = parseCalibration(dir + "/rectified.cfg");
    printf("rectified_cfg_same_K %d\n", c.width == u.out_width && c.height == u.out_height && std::memcmp(c.K.m, u.K.m, sizeof(c.K.m)) == 0 ? 1 : 0);
    return 0;
  }
  if (cmd == "undistort" && argc >= 5) {
    FILE* f = fopen(argv[3], "rb");
    FILE* o = fopen(argv[4], "wb");
    if (!f || !o) return 3;
    std::vector<unsigned char> raw((size_t)u.in_width * u.in_height), out((size_t)u.out_width * u.out_height);
    int n = 0;
    while (fread(raw.data(), 1, raw.size(), f) == raw.size()) {
      u.undistort(raw.data(), out.data());
      if (fwrite(out.data(), 1, out.size(), o) != out.size()) return 3;
      n++;
    }
    fclose(f);
    fclose(o);
    printf("images %d\n", n);
    return 0;
  }
  return 2;
}
