// The arena of a frame: which planes it holds, in which order, how large each is and which lsdhip_frame member each backs — stated once,
// in lsd_frame_planes.  Plain C++ without HIP headers, templated on the frame type: tests/cpp/frame_layout_test.cpp checks the
// arithmetic with a stand-in frame.
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include "../../include/lsdhip.h"

inline size_t lsd_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// gradient candidates: per group of 1024 consecutive pixels 1024 uint16 offsets, then one uint16 count per group
inline int lsd_gradcand_groups(int pixels) { return (pixels + 1023) >> 10; }
inline size_t lsd_gradcand_bytes(int pixels) { return ((size_t)lsd_gradcand_groups(pixels) * 1024 + (size_t)lsd_gradcand_groups(pixels)) * 2; }
// reference blocks: per 256 consecutive pixels 256 byte offsets, then one int32 count per block
inline int lsd_refblk_blocks(int pixels) { return (pixels + 255) >> 8; }
inline size_t lsd_refblk_bytes(int pixels) { return (size_t)lsd_refblk_blocks(pixels) * (256 + 4); }

// Every plane of the arena, in arena order: plane(member, bytes).  wl / hl: the level sizes of the context.
template <class Frame, class Plane> inline void lsd_frame_planes(Frame& f, const int* wl, const int* hl, Plane&& plane) {
  constexpr int L = LSDHIP_PYRAMID_LEVELS;
  auto px = [&](int l) { return (size_t)wl[l] * hl[l]; };
  plane(f.d_gray, px(0));
  for (int l = 0; l < L; l++) plane(f.d_image[l], px(l) * 4);
  for (int l = 0; l < L; l++) plane(f.d_grad[l], px(l) * 16);
  plane(f.d_absgrad, px(0) * 4);
  plane(f.d_maxgrad, px(0) * 4);
  for (int l = 0; l < L; l++) plane(f.d_idepth[l], px(l) * 4);
  for (int l = 0; l < L; l++) plane(f.d_idepthVar[l], px(l) * 4);
  plane(f.d_wasGood, px(1));
  plane(f.d_idepth_reAct, px(0) * 4);       // re-activation data (Frame::takeReActivationData): idepth, idepthVar, validity
  plane(f.d_idepthVar_reAct, px(0) * 4);
  plane(f.d_validity_reAct, px(0));
  for (int l = 0; l < L; l++) plane(f.d_idepthW[l], px(l) * 4);      // second depth plane set (pipelined contexts)
  for (int l = 0; l < L; l++) plane(f.d_idepthVarW[l], px(l) * 4);
  for (int l = 1; l < L; l++) plane(f.d_refBlk[l], lsd_refblk_bytes((int)px(l)));    // reference blocks of levels >= 1, one set per depth plane set
  for (int l = 1; l < L; l++) plane(f.d_refBlkW[l], lsd_refblk_bytes((int)px(l)));
  plane(f.d_gradCand, lsd_gradcand_bytes((int)px(0)));                               // gradient candidates (keyframes)
}

// Where each plane starts (256-byte aligned, in lsd_frame_planes' order) and what the arena takes: depends on the level sizes only, so a
// context computes it once.
struct LsdFrameLayout {
  static constexpr int MAX_PLANES = 64;
  int n = 0;
  size_t off[MAX_PLANES] = {};
  size_t bytes = 0;
};
template <class Frame> inline LsdFrameLayout lsd_frame_layout(const int* wl, const int* hl) {
  LsdFrameLayout lay;
  Frame f;
  size_t end = 0;
  lsd_frame_planes(f, wl, hl, [&](auto*&, size_t bytes) {
    if (lay.n < LsdFrameLayout::MAX_PLANES) {
      lay.off[lay.n] = lsd_align_up(end, 256);
      end = lay.off[lay.n] + bytes;
    }
    lay.n++;   // (n > MAX_PLANES: the plane list has outgrown the table, and frame_alloc refuses the layout)
  });
  lay.bytes = lsd_align_up(end, 256);
  return lay;
}
// points the frame's plane members into the arena at `base`
template <class Frame> inline void lsd_frame_bind(Frame& f, const LsdFrameLayout& lay, const int* wl, const int* hl, char* base) {
  int k = 0;
  lsd_frame_planes(f, wl, hl, [&](auto*& member, size_t) {
    using P = typename std::remove_reference<decltype(member)>::type;
    member = (P)(base + lay.off[k++]);
  });
}
