// The arena layout of a frame (lsd_slam_amd/csrc/frame_layout.hpp) on a stand-in frame type, without HIP: plane count, alignment, order,
// no overlap, every plane at least as large as its consumer needs, and the arena total of four image sizes as literals.
// Usage: frame_layout_test   (prints one line per size; exit status 0 = all checks hold)
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../lsd_slam_amd/csrc/frame_layout.hpp"

namespace {
constexpr int L = LSDHIP_PYRAMID_LEVELS;
struct Texel { float x, y, z, w; };
struct Frame {   // the plane members of lsdhip_frame
  uint8_t* d_gray = nullptr;
  float* d_image[L] = {};
  Texel* d_grad[L] = {};
  float* d_absgrad = nullptr;
  float* d_maxgrad = nullptr;
  float* d_idepth[L] = {};
  float* d_idepthVar[L] = {};
  uint8_t* d_wasGood = nullptr;
  float* d_idepth_reAct = nullptr;
  float* d_idepthVar_reAct = nullptr;
  uint8_t* d_validity_reAct = nullptr;
  float* d_idepthW[L] = {};
  float* d_idepthVarW[L] = {};
  uint8_t* d_refBlk[L] = {};
  uint8_t* d_refBlkW[L] = {};
  uint16_t* d_gradCand = nullptr;
};

int g_fail = 0;
#define CHECK(cond, ...)                                         \
  do {                                                           \
    if (!(cond)) {                                               \
      g_fail++;                                                  \
      std::printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                                  \
      std::printf("\n");                                         \
    }                                                            \
  } while (0)

struct Want { std::string name; const void* member; size_t need; };   // member: the frame member in which the bound pointer must turn up

void check_size(int w, int h, size_t wantTotal) {
  int wl[L], hl[L];
  for (int l = 0; l < L; l++) { wl[l] = w >> l; hl[l] = h >> l; }
  auto px = [&](int l) { return (size_t)wl[l] * hl[l]; };
  Frame f;
  // the documented order, with what each plane's consumer needs
  std::vector<Want> want;
  auto one = [&](const char* name, auto& member, size_t need) { want.push_back({name, &member, need}); };
  auto levels = [&](const char* name, auto& members, int from, auto need) {
    for (int l = from; l < L; l++) want.push_back({std::string(name) + "[" + std::to_string(l) + "]", &members[l], need(l)});
  };
  auto blocks = [&](int l) { return (px(l) + 255) / 256 * 260; };
  const size_t groups = (px(0) + 1023) / 1024;
  one("gray", f.d_gray, px(0));
  levels("image", f.d_image, 0, [&](int l) { return px(l) * 4; });
  levels("grad", f.d_grad, 0, [&](int l) { return px(l) * 16; });
  one("absgrad", f.d_absgrad, px(0) * 4);
  one("maxgrad", f.d_maxgrad, px(0) * 4);
  levels("idepth", f.d_idepth, 0, [&](int l) { return px(l) * 4; });
  levels("idepthVar", f.d_idepthVar, 0, [&](int l) { return px(l) * 4; });
  one("wasGood", f.d_wasGood, px(1));
  one("idepth_reAct", f.d_idepth_reAct, px(0) * 4);
  one("idepthVar_reAct", f.d_idepthVar_reAct, px(0) * 4);
  one("validity_reAct", f.d_validity_reAct, px(0));
  levels("idepthW", f.d_idepthW, 0, [&](int l) { return px(l) * 4; });
  levels("idepthVarW", f.d_idepthVarW, 0, [&](int l) { return px(l) * 4; });
  levels("refBlk", f.d_refBlk, 1, blocks);
  levels("refBlkW", f.d_refBlkW, 1, blocks);
  one("gradCand", f.d_gradCand, (groups * 1024 + groups) * 2);
  CHECK(want.size() == 46, "%zu planes expected by the test itself", want.size());

  const LsdFrameLayout lay = lsd_frame_layout<Frame>(wl, hl);
  CHECK(lay.n == 46, "%dx%d: %d planes", w, h, lay.n);
  CHECK(lay.bytes == wantTotal, "%dx%d: arena of %zu bytes, want %zu", w, h, lay.bytes, wantTotal);
  CHECK(lay.bytes % 256 == 0, "%dx%d: arena size %zu", w, h, lay.bytes);
  if (lay.n != (int)want.size()) return;

  // the sizes lsd_frame_planes states, in its order
  std::vector<size_t> stated;
  lsd_frame_planes(f, wl, hl, [&](auto*&, size_t bytes) { stated.push_back(bytes); });
  CHECK(stated.size() == want.size(), "%zu planes visited", stated.size());
  if (stated.size() != want.size()) return;

  // bound into an arena that is never touched: the member each plane backs, its offset and its room
  char* const base = (char*)(uintptr_t)0x100000;
  lsd_frame_bind(f, lay, wl, hl, base);
  CHECK(lay.off[0] == 0, "first plane at %zu", lay.off[0]);
  for (int k = 0; k < lay.n; k++) {
    const Want& q = want[k];
    const size_t end = k + 1 < lay.n ? lay.off[k + 1] : lay.bytes;
    CHECK(lay.off[k] % 256 == 0, "%dx%d %s: offset %zu", w, h, q.name.c_str(), lay.off[k]);
    char* bound = nullptr;
    std::memcpy(&bound, q.member, sizeof(bound));
    CHECK(bound == base + lay.off[k], "%dx%d: plane %d is not %s", w, h, k, q.name.c_str());
    CHECK(end > lay.off[k] || stated[k] == 0, "%dx%d %s: does not ascend", w, h, q.name.c_str());
    CHECK(lay.off[k] + stated[k] <= end, "%dx%d %s: %zu bytes overlap the next plane at %zu", w, h, q.name.c_str(), stated[k], end);
    CHECK(stated[k] >= q.need, "%dx%d %s: %zu bytes, its consumer needs %zu", w, h, q.name.c_str(), stated[k], q.need);
  }
  // nothing else was bound: level 0 has no reference blocks
  CHECK(f.d_refBlk[0] == nullptr && f.d_refBlkW[0] == nullptr, "%dx%d: level-0 reference blocks bound", w, h);
  std::printf("%dx%d: %d planes, %zu bytes\n", w, h, lay.n, lay.bytes);
}
}  // namespace

int main() {
  // totals: the arithmetic of frame_alloc before the layout had an owner, evaluated for these sizes
  check_size(16, 16, 27392);
  check_size(176, 144, 1751552);
  check_size(640, 480, 21161984);
  check_size(656, 496, 22415616);
  // the size helpers at their ragged edges
  CHECK(lsd_refblk_blocks(1) == 1 && lsd_refblk_blocks(256) == 1 && lsd_refblk_blocks(257) == 2, "reference-block count");
  CHECK(lsd_refblk_bytes(257) == 520, "reference-block bytes %zu", lsd_refblk_bytes(257));
  CHECK(lsd_gradcand_groups(1024) == 1 && lsd_gradcand_groups(1025) == 2, "candidate groups");
  CHECK(lsd_gradcand_bytes(1025) == (2 * 1024 + 2) * 2, "candidate bytes %zu", lsd_gradcand_bytes(1025));
  CHECK(lsd_align_up(0, 256) == 0 && lsd_align_up(1, 256) == 256 && lsd_align_up(256, 256) == 256, "align");
  if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
  std::printf("frame layout ok\n");
  return 0;
}
