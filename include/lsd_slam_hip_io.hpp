// lsd_slam_hip_io.hpp — host-side data formats either side of the hot path, header-only C++:
//   * the camera calibration file of lsd_slam_core (calib/*.cfg, parsed by util/Undistorter.cpp:43-140) in its
//     distortion-free form, with the reference's K convention (Undistorter.cpp:340-344), and — struct Undistorter — in its FOV-model
//     form for raw camera images: output intrinsics, remap tables and the bilinear gather of UndistorterPTAM (Undistorter.cpp:91-411),
//     the yardstick of the device's rectification inside frame creation;
//   * binary PGM (P5) image files for the image-folder driver (the reference reads through OpenCV, which is not here);
//   * the keyframe message of lsd_slam_viewer (msg/keyframeMsg.msg; InputPointDense payload V/KeyFrameDisplay.h:39-44,
//     filled as C/IOWrapper/ROS/ROSOutput3DWrapper.cpp:70-111) in ROS 1 wire serialisation;
//   * the viewer's point-cloud export (V/KeyFrameDisplay.cpp:269-340 flushPC + V/KeyFrameGraphDisplay.cpp:60-94 PLY header);
//   * the depth map's debug image (C/DepthEstimation/DepthMap.cpp:1400-1428 debugPlotDepthMap) as plotDepthMap, and binary PPM (P6) files
//     for it: the yardstick of DepthMap::debugPlotDepthMap (lsdhip_depth_debug_plot), which draws the same bytes on the device.
// The formats and their host-side fill loops (makeKeyframeMsg, flushPointCloud) are plain host code and the yardstick of the device
// export: makeKeyframeMsgDevice packs the payload on the GPU (lsdhip_frame_pack_keyframe_points) and PointCloud (lsd_slam_hip.hpp)
// builds the viewer's cloud there, both held bit for bit to the host functions below; cloudConstants is the one place the per-keyframe
// constants of the cloud are computed, for both paths.
#ifndef LSD_SLAM_HIP_IO_HPP
#define LSD_SLAM_HIP_IO_HPP

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "lsd_slam_hip.hpp"
#include "lsd_slam_hip_cloud_constants.hpp"

namespace lsd_slam_hip {

struct Calibration {
  int width = 0, height = 0;
  Mat3f K;
};

// First line "fx fy cx cy dist", second "in_width in_height", third crop mode, fourth "out_width out_height".
// Values of fx..cy below 1 are relative to the image size.  Only dist == 0 with equal input / output size is
// accepted: undistortion (the rest of Undistorter.cpp) is outside the hot path.
inline Calibration parseCalibration(const std::string& path) {
  std::ifstream f(path);
  if (!f) throw Error(LSDHIP_E_ARG, "cannot open calibration file " + path);
  std::string l1, l2, l3, l4;
  std::getline(f, l1); std::getline(f, l2); std::getline(f, l3); std::getline(f, l4);
  float fx, fy, cx, cy, dist = 0;
  int iw, ih, ow, oh;
  std::istringstream s1(l1), s2(l2), s4(l4);
  if (!(s1 >> fx >> fy >> cx >> cy)) throw Error(LSDHIP_E_ARG, "calibration: cannot read fx fy cx cy");
  s1 >> dist;
  if (!(s2 >> iw >> ih)) throw Error(LSDHIP_E_ARG, "calibration: cannot read the input size");
  if (!(s4 >> ow >> oh)) { ow = iw; oh = ih; }
  if (dist != 0 || ow != iw || oh != ih)
    throw Error(LSDHIP_E_ARG, "calibration needs undistortion / resizing, which is outside the accelerated path: rectify the images first");
  if (iw % 16 || ih % 16) throw Error(LSDHIP_E_ARG, "image size must be a multiple of 16 (C/SlamSystem.cpp:55-59)");
  Calibration c;
  c.width = iw; c.height = ih;
  if (cx < 1 && cy < 1) {  // relative calibration (Undistorter.cpp:340-344)
    fx *= iw; fy *= ih;
    cx = cx * iw - 0.5f; cy = cy * ih - 0.5f;
  }
  c.K = Mat3f::intrinsics(fx, fy, cx, cy);
  return c;
}

// UndistorterPTAM (util/Undistorter.cpp:91-411): the FOV ("ATAN") camera model of the reference's calibration files, for raw camera
// images — what parseCalibration above refuses.  Plain host code: the parser, the output intrinsics, the remap tables and the bilinear
// gather.  undistort() is the yardstick of the device path (lsdhip_undistorter_apply, lsdhip_frame_create_undistorted*: DeviceUndistorter
// of lsd_slam_hip.hpp), which is held to it bit for bit.
//
// What is pinned and what is not:
//   * every expression is evaluated in the reference's types and order (float variables; a double literal or factor promotes the
//     expression it stands in, as in the reference), with the float overloads of tan / atan / sqrt, and without contraction into fused
//     multiply-adds (the functions below carry their own contraction switch; compile test programs with -ffp-contract=off all the same);
//   * undistort() converts the interpolated value to a byte by truncation toward zero with the range clamped to [0, 255] (NaN: 0): the
//     reference's float -> uchar cast is undefined outside that range;
//   * a reference build whose compiler contracts the interpolation into FMAs (-march=native on an FMA machine) can differ from
//     undistort() by one grey level on rare pixels, and one whose <cmath> resolves the unqualified tan / atan to the double functions
//     can differ in the last bits of the tables.  Neither can be pinned from here;
//   * line 3 == "none" with dist != 0 reads an uninitialised outputCalibration in the reference: refused here.
// The OpenCV model (8 parameters on line 1, UndistorterOpenCV, Undistorter.cpp:449-) is refused: cv::remap's fixed-point interpolation
// cannot be restated without OpenCV.  Only the relative form of line 1 is defined (the reference multiplies by the image size
// unconditionally, :177-180): absolute pixel values (fx > 1) are refused.
#if defined(__clang__)
#define LSD_IO_NO_CONTRACT_FN
#define LSD_IO_NO_CONTRACT_BODY _Pragma("clang fp contract(off)")
#elif defined(__GNUC__)
#define LSD_IO_NO_CONTRACT_FN __attribute__((optimize("fp-contract=off")))
#define LSD_IO_NO_CONTRACT_BODY
#else
#define LSD_IO_NO_CONTRACT_FN
#define LSD_IO_NO_CONTRACT_BODY
#endif
struct Undistorter {
  enum Mode { Crop, Full, None, Explicit };
  int in_width = 0, in_height = 0, out_width = 0, out_height = 0;
  float inputCalibration[5] = {0, 0, 0, 0, 0};
  float outputCalibration[5] = {0, 0, 0, 0, 0};   // relative (fx / w, fy / h, (cx + 0.5) / w, (cy + 0.5) / h, 0) of the rectified images (:276-280)
  Mat3f K = Mat3f::intrinsics(0, 0, 0, 0);        // of the rectified images, by the convention of :339-344
  std::vector<float> remapX, remapY;              // out_width * out_height each, -1 outside the input image; empty: pass-through
  // neither distortion nor resize (:370-375): undistort() copies, no tables
  bool passThrough() const { return remapX.empty(); }

  // in5 = fx fy cx cy dist (relative), out5 = the five numbers of line 3 (Explicit only, else ignored / null)
  LSD_IO_NO_CONTRACT_FN Undistorter(const float in5[5], int in_w, int in_h, Mode mode, const float* out5, int out_w, int out_h) {
    LSD_IO_NO_CONTRACT_BODY
    if (in_w < 2 || in_h < 2 || out_w <= 0 || out_h <= 0) throw Error(LSDHIP_E_ARG, "calibration: bad image size");
    if (out_w % 16 || out_h % 16) throw Error(LSDHIP_E_ARG, "image size must be a multiple of 16 (C/SlamSystem.cpp:55-59)");
    if (in5[0] > 1 || in5[1] > 1)
      throw Error(LSDHIP_E_ARG, "calibration: fx fy cx cy must be relative to the image size (the reference's FOV undistorter multiplies them by it, Undistorter.cpp:177-180); absolute pixel values are not supported");
    in_width = in_w; in_height = in_h; out_width = out_w; out_height = out_h;
    for (int i = 0; i < 5; i++) inputCalibration[i] = in5[i];
    const float dist = inputCalibration[4];
    if (mode == None && dist != 0)
      throw Error(LSDHIP_E_ARG, "calibration: 'none' with a distorted camera (dist != 0) is undefined in the reference; use crop, full or explicit output intrinsics");
    if (mode == Explicit && !out5) throw Error(LSDHIP_E_ARG, "calibration: explicit output intrinsics missing");
    const float d2t = 2.0f * std::tan(dist / 2.0f);
    // current camera parameters (:177-188; the scale factors there are 1)
    float fx = inputCalibration[0] * in_width;
    float fy = inputCalibration[1] * in_height;
    float cx = (float)(inputCalibration[2] * in_width - 0.5);
    float cy = (float)(inputCalibration[3] * in_height - 0.5);
    cx = (float)((cx + 0.5) * 1.0 - 0.5);
    cy = (float)((cy + 0.5) * 1.0 - 0.5);
    float ofx, ofy, ocx, ocy;
    if (dist == 0) {                       // :194-200 (whatever line 3 says)
      ofx = inputCalibration[0] * out_width;
      ofy = inputCalibration[1] * out_height;
      ocx = (float)((inputCalibration[2] * out_width) - 0.5);
      ocy = (float)((inputCalibration[3] * out_height) - 0.5);
    } else if (mode == Crop) {             // :201-228
      const float left_radius = (cx) / fx;
      const float right_radius = (in_width - 1 - cx) / fx;
      const float top_radius = (cy) / fy;
      const float bottom_radius = (in_height - 1 - cy) / fy;
      const float trans_left_radius = std::tan(left_radius * dist) / d2t;
      const float trans_right_radius = std::tan(right_radius * dist) / d2t;
      const float trans_top_radius = std::tan(top_radius * dist) / d2t;
      const float trans_bottom_radius = std::tan(bottom_radius * dist) / d2t;
      ofy = fy * ((top_radius + bottom_radius) / (trans_top_radius + trans_bottom_radius)) * ((float)out_height / (float)in_height);
      ocy = (trans_top_radius / top_radius) * ofy * cy / fy;
      ofx = fx * ((left_radius + right_radius) / (trans_left_radius + trans_right_radius)) * ((float)out_width / (float)in_width);
      ocx = (trans_left_radius / left_radius) * ofx * cx / fx;
    } else if (mode == Full) {             // :229-267
      const float left_radius = cx / fx;
      const float right_radius = (in_width - 1 - cx) / fx;
      const float top_radius = cy / fy;
      const float bottom_radius = (in_height - 1 - cy) / fy;
      const float tl_radius = std::sqrt(left_radius * left_radius + top_radius * top_radius);
      const float tr_radius = std::sqrt(right_radius * right_radius + top_radius * top_radius);
      const float bl_radius = std::sqrt(left_radius * left_radius + bottom_radius * bottom_radius);
      const float br_radius = std::sqrt(right_radius * right_radius + bottom_radius * bottom_radius);
      const float trans_tl_radius = std::tan(tl_radius * dist) / d2t;
      const float trans_tr_radius = std::tan(tr_radius * dist) / d2t;
      const float trans_bl_radius = std::tan(bl_radius * dist) / d2t;
      const float trans_br_radius = std::tan(br_radius * dist) / d2t;
      const float hor = std::max(br_radius, tr_radius) + std::max(bl_radius, tl_radius);
      const float vert = std::max(tr_radius, tl_radius) + std::max(bl_radius, br_radius);
      const float trans_hor = std::max(trans_br_radius, trans_tr_radius) + std::max(trans_bl_radius, trans_tl_radius);
      const float trans_vert = std::max(trans_tr_radius, trans_tl_radius) + std::max(trans_bl_radius, trans_br_radius);
      ofy = fy * ((vert) / (trans_vert)) * ((float)out_height / (float)in_height);
      ocy = std::max(trans_tl_radius / tl_radius, trans_tr_radius / tr_radius) * ofy * cy / fy;
      ofx = fx * ((hor) / (trans_hor)) * ((float)out_width / (float)in_width);
      ocx = std::max(trans_bl_radius / bl_radius, trans_tl_radius / tl_radius) * ofx * cx / fx;
    } else {                               // :268-274
      ofx = out5[0] * out_width;
      ofy = out5[1] * out_height;
      ocx = (float)(out5[2] * out_width - 0.5);
      ocy = (float)(out5[3] * out_height - 0.5);
    }
    outputCalibration[0] = ofx / out_width;
    outputCalibration[1] = ofy / out_height;
    outputCalibration[2] = (float)((ocx + 0.5) / out_width);
    outputCalibration[3] = (float)((ocy + 0.5) / out_height);
    outputCalibration[4] = 0;
    // :339-344 (a double matrix there, read back as float by the callers)
    K = Mat3f::intrinsics(outputCalibration[0] * out_width, outputCalibration[1] * out_height,
                          (float)(outputCalibration[2] * out_width - 0.5), (float)(outputCalibration[3] * out_height - 0.5));
    if (in_height == out_height && in_width == out_width && dist == 0) return;   // pass-through (:370-375)
    remapX.resize((size_t)out_width * out_height);
    remapY.resize((size_t)out_width * out_height);
    for (int y = 0; y < out_height; y++)
      for (int x = 0; x < out_width; x++) {      // :285-315
        float ix = (x - ocx) / ofx;
        float iy = (y - ocy) / ofy;
        const float r = std::sqrt(ix * ix + iy * iy);
        const float fac = (r == 0 || dist == 0) ? 1 : std::atan(r * d2t) / (dist * r);
        ix = fx * fac * ix + cx;
        iy = fy * fac * iy + cy;
        // make rounding resistant.
        if (ix == 0) ix = (float)0.01;
        if (iy == 0) iy = (float)0.01;
        if (ix == in_width - 1) ix = (float)(in_width - 1.01);
        if (iy == in_height - 1) ix = (float)(in_height - 1.01);   // sic (:302 assigns ix): iy stays in_height - 1, the pixel is invalid below
        const size_t o = (size_t)x + (size_t)y * out_width;
        if (ix > 0 && iy > 0 && ix < in_width - 1 && iy < in_height - 1) {
          remapX[o] = ix;
          remapY[o] = iy;
        } else {
          remapX[o] = -1;
          remapY[o] = -1;
        }
      }
  }

  // The four lines of a calibration file (:100-166)
  static Undistorter fromLines(const std::string& l1, const std::string& l2, const std::string& l3in, const std::string& l4) {
    float ic[8], in5[5], out5[5];
    int iw, ih, ow, oh;
    if (std::sscanf(l1.c_str(), "%f %f %f %f %f %f %f %f", &ic[0], &ic[1], &ic[2], &ic[3], &ic[4], &ic[5], &ic[6], &ic[7]) == 8)
      throw Error(LSDHIP_E_ARG, "calibration: 8 parameters on the first line are the OpenCV camera model (UndistorterOpenCV), which is not supported: only the FOV model (fx fy cx cy dist)");
    if (std::sscanf(l1.c_str(), "%f %f %f %f %f", &in5[0], &in5[1], &in5[2], &in5[3], &in5[4]) != 5 || std::sscanf(l2.c_str(), "%d %d", &iw, &ih) != 2)
      throw Error(LSDHIP_E_ARG, "calibration: cannot read 'fx fy cx cy dist' and the input size");
    std::string l3 = l3in;
    while (!l3.empty() && isspace((unsigned char)l3.back())) l3.pop_back();
    Mode mode;
    if (l3 == "crop") mode = Crop;
    else if (l3 == "full") mode = Full;
    else if (l3 == "none") mode = None;
    else if (std::sscanf(l3.c_str(), "%f %f %f %f %f", &out5[0], &out5[1], &out5[2], &out5[3], &out5[4]) == 5) mode = Explicit;
    else throw Error(LSDHIP_E_ARG, "calibration: the third line is none of crop, full, none or five output parameters");
    if (std::sscanf(l4.c_str(), "%d %d", &ow, &oh) != 2) throw Error(LSDHIP_E_ARG, "calibration: cannot read the output size");
    return Undistorter(in5, iw, ih, mode, mode == Explicit ? out5 : nullptr, ow, oh);
  }
  static Undistorter fromFile(const std::string& path) {
    std::ifstream f(path);
    if (!f) throw Error(LSDHIP_E_ARG, "cannot open calibration file " + path);
    std::string l1, l2, l3, l4;
    std::getline(f, l1); std::getline(f, l2); std::getline(f, l3); std::getline(f, l4);
    return fromLines(l1, l2, l3, l4);
  }
  // The calibration file of the rectified images (what parseCalibration accepts, and reads back to exactly K)
  std::string rectifiedCalibrationText() const {
    char b[256];
    std::snprintf(b, sizeof(b), "%.9g %.9g %.9g %.9g 0\n%d %d\nnone\n%d %d\n", (double)outputCalibration[0], (double)outputCalibration[1],
                  (double)outputCalibration[2], (double)outputCalibration[3], out_width, out_height, out_width, out_height);
    return b;
  }

  // UndistorterPTAM::undistort (:355-411): raw in_width * in_height bytes -> out out_width * out_height bytes
  LSD_IO_NO_CONTRACT_FN void undistort(const unsigned char* raw, unsigned char* out) const {
    LSD_IO_NO_CONTRACT_BODY
    const int n = out_width * out_height;
    if (passThrough()) { std::memcpy(out, raw, (size_t)n); return; }
    const float* rx = remapX.data();
    const float* ry = remapY.data();
    for (int idx = n - 1; idx >= 0; idx--) {
      float xx = rx[idx];
      float yy = ry[idx];
      if (xx < 0) { out[idx] = 0; continue; }
      const int xxi = (int)xx;
      const int yyi = (int)yy;
      xx -= xxi;
      yy -= yyi;
      const float xxyy = xx * yy;
      const unsigned char* src = raw + xxi + yyi * in_width;
      const float s00 = src[0], s10 = src[1], s01 = src[in_width], s11 = src[1 + in_width];
      const float v = ((xxyy * s11 + (yy - xxyy) * s01) + (xx - xxyy) * s10) + (((1 - xx) - yy) + xxyy) * s00;
      out[idx] = !(v > 0) ? 0 : (v >= 255 ? 255 : (unsigned char)(int)v);
    }
  }
};

inline bool readPGM(const std::string& path, int w, int h, std::vector<unsigned char>& out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  char magic[3] = {0, 0, 0};
  int iw = 0, ih = 0, maxv = 0;
  auto skip = [&]() { int c; while ((c = fgetc(f)) != EOF) { if (c == '#') { while ((c = fgetc(f)) != EOF && c != '\n') {} } else if (!isspace(c)) { ungetc(c, f); break; } } };
  bool ok = fscanf(f, "%2s", magic) == 1 && std::string(magic) == "P5";
  if (ok) { skip(); ok = fscanf(f, "%d", &iw) == 1; }
  if (ok) { skip(); ok = fscanf(f, "%d", &ih) == 1; }
  if (ok) { skip(); ok = fscanf(f, "%d", &maxv) == 1 && maxv == 255; }
  if (ok) { fgetc(f); ok = iw == w && ih == h; }
  if (ok) { out.resize((size_t)w * h); ok = fread(out.data(), 1, out.size(), f) == out.size(); }
  fclose(f);
  return ok;
}
inline bool writePGM(const std::string& path, int w, int h, const unsigned char* data) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return false;
  fprintf(f, "P5\n%d %d\n255\n", w, h);
  bool ok = fwrite(data, 1, (size_t)w * h, f) == (size_t)w * h;
  fclose(f);
  return ok;
}

inline bool writePPM(const std::string& path, int w, int h, const unsigned char* rgb) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return false;
  fprintf(f, "P6\n%d %d\n255\n", w, h);
  bool ok = fwrite(rgb, 1, (size_t)w * h * 3, f) == (size_t)w * h * 3;
  fclose(f);
  return ok;
}

// DepthMapPixelHypothesis::getVisualizationColor (DepthMapPixelHypothesis.cpp:29-90) with the reference's operations, promotions and
// order; debugDisplay is the reference's global (util/settings.cpp:35).  Inputs on which the reference's float -> uchar cast is
// undefined behaviour are defined: a NaN idepth is white (modes 0 / 1), a NaN or negative variance (0, 0, 255) (modes 3 / 4), a NaN
// byte value 0 (modes 2 / 5).
inline void visualizationColor(const lsdhip_hypothesis& hyp, int debugDisplay, int lastFrameID, unsigned char c[3]) {
  auto clampByte = [](float f) -> unsigned char { return !(f > 0) ? 0 : (f > 255 ? 255 : (unsigned char)f); };
  c[0] = c[1] = c[2] = 255;
  if (debugDisplay == 0 || debugDisplay == 1) {
    const float id = debugDisplay == 0 ? hyp.idepth_smoothed : hyp.idepth;
    if (!(id >= 0)) return;
    // rainbow between 0 and 4
    float r = (0 - id) * 255 / 1.0; if (r < 0) r = -r;
    float g = (1 - id) * 255 / 1.0; if (g < 0) g = -g;
    float b = (2 - id) * 255 / 1.0; if (b < 0) b = -b;
    c[0] = (unsigned char)(255 - clampByte(r)); c[1] = (unsigned char)(255 - clampByte(g)); c[2] = (unsigned char)(255 - clampByte(b));
  } else if (debugDisplay == 2) {
    const float f = hyp.validity_counter * (255.0 / (250.0f + 5.0f));   // VALIDITY_COUNTER_MAX_VARIABLE + VALIDITY_COUNTER_MAX
    c[0] = 0; c[1] = c[2] = clampByte(f);
  } else if (debugDisplay == 3 || debugDisplay == 4) {
    const float idv = debugDisplay == 3 ? hyp.idepth_var_smoothed : hyp.idepth_var;
    float var = -0.5 * std::log10((double)idv);     // (the reference's unqualified log10 is the double overload)
    var = var * 255 * 0.333;
    if (var > 255) var = 255;
    if (!(var >= 0)) { c[0] = 0; c[1] = 0; c[2] = 255; return; }
    c[0] = (unsigned char)(255 - var); c[1] = (unsigned char)var; c[2] = 0;
  } else if (debugDisplay == 5) {
    const float f = (hyp.nextStereoFrameMinID - lastFrameID) * (255.0 / 100);
    c[0] = c[2] = clampByte(f); c[1] = 0;
  }
}

// DepthMap::debugPlotDepthMap (DepthMap.cpp:1400-1428): `image` is the keyframe's level-0 image, refID the map's
// referenceFrameByID_offset, out uint8 [h][w][3].  Plain host code: what lsdhip_depth_debug_plot is held to, byte for byte.
inline void plotDepthMap(const lsdhip_hypothesis* map, const float* image, int w, int h, int debugDisplay, int refID, unsigned char* out) {
  for (int idx = 0; idx < w * h; idx++) {
    // cv::Mat::convertTo(CV_8UC1): cvRound (to nearest even), saturated; cvtColor(GRAY2RGB)
    const long r = std::lrint(image[idx]);
    unsigned char* px = out + 3 * (size_t)idx;
    px[0] = px[1] = px[2] = (unsigned char)(r < 0 ? 0 : (r > 255 ? 255 : r));
    if (map[idx].blacklisted < -1 /* MIN_BLACKLIST */ && debugDisplay == 2) { px[0] = 0; px[1] = 0; px[2] = 255; }
    if (!map[idx].isValid) continue;
    visualizationColor(map[idx], debugDisplay, refID, px);
  }
}

// V/KeyFrameDisplay.h:39-44
struct InputPointDense {
  float idepth;
  float idepth_var;
  unsigned char color[4];
};
static_assert(sizeof(InputPointDense) == 12, "InputPointDense is 12 bytes on the wire");

// lsd_slam_viewer/msg/keyframeMsg.msg
struct KeyframeMsg {
  int32_t id = 0;
  double time = 0;
  bool isKeyframe = true;
  float camToWorld[7] = {0, 0, 0, 1, 0, 0, 0};  // Sophus Sim3f::data(): quaternion x y z w with norm = scale, then translation
  float fx = 0, fy = 0, cx = 0, cy = 0;
  uint32_t height = 0, width = 0;
  std::vector<InputPointDense> pointcloud;
};

// (sim3ToWire, the Sim3 -> 7 float conversion of the message, lives in lsd_slam_hip.hpp: PointCloud uses it too)

// ROSOutput3DWrapper::publishKeyframe (ROSOutput3DWrapper.cpp:70-111) at publishLvl 0, from the device planes
inline KeyframeMsg makeKeyframeMsg(const Frame& kf, const Sim3& camToWorld, const Mat3f& K) {
  KeyframeMsg m;
  m.id = kf.id();
  m.time = kf.timestamp();
  sim3ToWire(camToWorld, m.camToWorld);
  m.fx = K.fx(); m.fy = K.fy(); m.cx = K.cx(); m.cy = K.cy();
  m.width = (uint32_t)kf.width(0); m.height = (uint32_t)kf.height(0);
  const std::vector<float> id = kf.idepth(0), var = kf.idepthVar(0), img = kf.image(0);
  m.pointcloud.resize(id.size());
  for (size_t i = 0; i < id.size(); i++) {
    m.pointcloud[i].idepth = id[i];
    m.pointcloud[i].idepth_var = var[i];
    const unsigned char c = (unsigned char)img[i];
    m.pointcloud[i].color[0] = m.pointcloud[i].color[1] = m.pointcloud[i].color[2] = m.pointcloud[i].color[3] = c;
  }
  return m;
}

// The same message with the payload packed on the device (lsdhip_frame_pack_keyframe_points): one launch and one copy of 12 bytes per
// pixel instead of three plane downloads and a host loop; serialises to the same bytes as makeKeyframeMsg's.
inline KeyframeMsg makeKeyframeMsgDevice(const Frame& kf, const Sim3& camToWorld, const Mat3f& K) {
  KeyframeMsg m;
  m.id = kf.id();
  m.time = kf.timestamp();
  sim3ToWire(camToWorld, m.camToWorld);
  m.fx = K.fx(); m.fy = K.fy(); m.cx = K.cx(); m.cy = K.cy();
  m.width = (uint32_t)kf.width(0); m.height = (uint32_t)kf.height(0);
  m.pointcloud.resize((size_t)m.width * m.height);
  check(lsdhip_frame_pack_keyframe_points(kf.handle(), (uint8_t*)m.pointcloud.data()), "lsdhip_frame_pack_keyframe_points");
  return m;
}

// ROS 1 serialisation of keyframeMsg (little-endian fields in declaration order, uint8[] with a uint32 length prefix)
inline std::vector<unsigned char> serializeKeyframeMsg(const KeyframeMsg& m) {
  std::vector<unsigned char> b;
  auto put = [&](const void* p, size_t n) { const unsigned char* c = (const unsigned char*)p; b.insert(b.end(), c, c + n); };
  put(&m.id, 4); put(&m.time, 8);
  const unsigned char kfFlag = m.isKeyframe ? 1 : 0;
  put(&kfFlag, 1);
  put(m.camToWorld, 28);
  put(&m.fx, 4); put(&m.fy, 4); put(&m.cx, 4); put(&m.cy, 4);
  put(&m.height, 4); put(&m.width, 4);
  const uint32_t len = (uint32_t)(m.pointcloud.size() * sizeof(InputPointDense));
  put(&len, 4);
  put(m.pointcloud.data(), len);
  return b;
}

// (CloudConstants / cloudConstants, the per-keyframe constants of flushPC for the host loop below and for the device append, come from
// lsd_slam_hip_cloud_constants.hpp: a header without dependencies, because liblsdhip itself includes it)

// KeyFrameDisplay::flushPC (V/KeyFrameDisplay.cpp:269-340) with the viewer's default thresholds (V/settings.cpp:36-40:
// scaledDepthVarTH = absDepthVarTH = 1, minNearSupport = 5, sparsifyFactor = 1); appends (x, y, z, intensity) floats.
inline int flushPointCloud(const KeyframeMsg& m, std::vector<float>& xyzi, float scaledTH = 1.f, float absTH = 1.f, int minNearSupport = 5) {
  const int w = (int)m.width, h = (int)m.height;
  const CloudConstants k = cloudConstants(m.fx, m.fy, m.cx, m.cy, m.camToWorld);
  const float fxi = k.fxi, fyi = k.fyi, cxi = k.cxi, cyi = k.cyi, scale = k.scale, ux = k.ux, uy = k.uy, uz = k.uz, uw = k.uw;
  int num = 0;
  for (int y = 1; y < h - 1; y++)
    for (int x = 1; x < w - 1; x++) {
      const InputPointDense& p = m.pointcloud[x + y * w];
      if (p.idepth <= 0) continue;
      const float depth = 1 / p.idepth;
      float depth4 = depth * depth;
      depth4 *= depth4;
      if (p.idepth_var * depth4 > scaledTH) continue;
      if (p.idepth_var * depth4 * scale * scale > absTH) continue;
      if (minNearSupport > 1) {
        int nearSupport = 0;
        for (int dx = -1; dx < 2; dx++)
          for (int dy = -1; dy < 2; dy++) {
            const InputPointDense& q = m.pointcloud[x + dx + (y + dy) * w];
            if (q.idepth > 0) {
              const float diff = q.idepth - 1.0f / depth;
              if (diff * diff < 2 * p.idepth_var) nearSupport++;
            }
          }
        if (nearSupport < minNearSupport) continue;
      }
      const float v[3] = {(x * fxi + cxi) * depth * scale, (y * fyi + cyi) * depth * scale, depth * scale};
      // rotate by the unit quaternion, then translate
      const float tx = 2 * (uy * v[2] - uz * v[1]), ty = 2 * (uz * v[0] - ux * v[2]), tz = 2 * (ux * v[1] - uy * v[0]);
      xyzi.push_back(v[0] + uw * tx + (uy * tz - uz * ty) + m.camToWorld[4]);
      xyzi.push_back(v[1] + uw * ty + (uz * tx - ux * tz) + m.camToWorld[5]);
      xyzi.push_back(v[2] + uw * tz + (ux * ty - uy * tx) + m.camToWorld[6]);
      xyzi.push_back(p.color[2] / 255.0f);
      num++;
    }
  return num;
}
// PLY file as KeyFrameGraphDisplay.cpp:74-88 writes it
inline bool writePLY(const std::string& path, const std::vector<float>& xyzi) {
  std::ofstream f(path, std::ios::binary);
  if (!f) return false;
  f << "ply\nformat binary_little_endian 1.0\nelement vertex " << xyzi.size() / 4
    << "\nproperty float x\nproperty float y\nproperty float z\nproperty float intensity\nend_header\n";
  f.write((const char*)xyzi.data(), (std::streamsize)(xyzi.size() * sizeof(float)));
  return (bool)f;
}

}  // namespace lsd_slam_hip
#endif
