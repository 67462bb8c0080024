// Host pose chain (include/lsd_slam_hip_pose.hpp) as a filter: tests/test_pose_chain_cpu.py feeds it operations, one per line, and
// compares what it prints with float64 matrix products.
//   mul a[8] b[8]      -> sim3_mul          (8 numbers)
//   inv a[8]           -> sim3_inv          (8 numbers)
//   rel ref[8] f[8]    -> relative_se3      (7 numbers)
//   chain n p1[8] ...  -> identity * p1 * ... * pn, every prefix (n lines of 8 numbers): camToWorld along a line of keyframes
//   lift se3[7] s      -> sim3_from_se3     (8 numbers)
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/lsd_slam_hip_pose.hpp"

using namespace lsd_slam::pose;

static bool read(double* p, int n) {
  for (int i = 0; i < n; i++) if (std::scanf("%lf", &p[i]) != 1) return false;
  return true;
}
static void print(const double* p, int n) {
  for (int i = 0; i < n; i++) std::printf("%.17g%c", p[i], i + 1 < n ? ' ' : '\n');
}

int main() {
  char op[16];
  while (std::scanf("%15s", op) == 1) {
    double a[8], b[8], out[8];
    if (!std::strcmp(op, "mul")) {
      if (!read(a, 8) || !read(b, 8)) return 2;
      sim3_mul(a, b, out);
      print(out, 8);
      // in place, both ways
      double c[8], d[8];
      std::memcpy(c, a, sizeof(c)); std::memcpy(d, b, sizeof(d));
      sim3_mul(c, b, c);
      sim3_mul(a, d, d);
      if (std::memcmp(c, out, sizeof(c)) || std::memcmp(d, out, sizeof(d))) { std::printf("in-place product differs\n"); return 1; }
    } else if (!std::strcmp(op, "inv")) {
      if (!read(a, 8)) return 2;
      sim3_inv(a, out);
      print(out, 8);
    } else if (!std::strcmp(op, "rel")) {
      if (!read(a, 8) || !read(b, 8)) return 2;
      relative_se3(a, b, out);
      print(out, 7);
    } else if (!std::strcmp(op, "lift")) {
      double s;
      if (!read(a, 7) || !read(&s, 1)) return 2;
      sim3_from_se3(a, s, out);
      print(out, 8);
    } else if (!std::strcmp(op, "chain")) {
      int n = 0;
      if (std::scanf("%d", &n) != 1 || n < 0 || n > 64) return 2;
      double w[8];
      sim3_identity(w);
      for (int i = 0; i < n; i++) {
        if (!read(a, 8)) return 2;
        sim3_mul(w, a, w);
        print(w, 8);
      }
    } else {
      return 2;
    }
  }
  std::printf("pose chain ok\n");
  return 0;
}
