// DepthMap on the device: semi-dense inverse-depth estimation kernels K4 (observe / doLineStereo / EKF update),
// K5 (fill holes), K6 (regularise), K7 (propagate to a new keyframe), K8 (setDepth + rescale).  gfx950 only.
//
// Reference behaviour restated (C/ = lsd_slam_core/src/):
//   DepthMap::observeDepthRow / observeDepthCreate / observeDepthUpdate   C/DepthEstimation/DepthMap.cpp:111-146, :237-473
//   DepthMap::makeAndCheckEPL                                             :184-234
//   DepthMap::doLineStereo                                                :1442-1972
//   DepthMap::regularizeDepthMapFillHolesRow + buildRegIntegralBuffer     :656-754
//   DepthMap::regularizeDepthMapRow<removeOcclusions>                     :758-848
//   DepthMap::propagateDepth                                              :475-653
//   DepthMap::updateKeyframe / createKeyFrame / finalizeKeyFrame          :1072-1213, :1222-1327, :1363-1395
//   DepthMap::initializeFromGTDepth / initializeRandomly / setFromExistingKF  :883-1018
//   Frame::setDepth / takeReActivationData / prepareForStereoWith         C/DataStructures/Frame.cpp:199-243, :107-145, :295-317
//
// HBM layout: the 32-byte AoS hypothesis of the reference becomes eight SoA planes (29 B/px).  The reference's
// "memcpy current -> other, read other, write current" snapshot (64 B/px of copy traffic per pass) is replaced by a
// ping-pong of the 1-byte validity plane only: K5 and K6 read every other field in place because neither of them
// modifies a field that a neighbouring pixel reads.  The validity integral image of K5 is replaced by a direct 5x5
// window sum (int32, exact — the integral is only ever used as that window difference).
#include <chrono>
#include <cstdlib>
#include "lsdhip_internal.hpp"
#include "block_scan.hpp"   // lsd_wave_sum, lsd_block_tree_sum, lsd_block_butterfly_sum

// ---- constants, C/util/settings.h:34-35, :50-174 ------------------------------------------------------------------
#define DIVISION_EPS 1e-10f
#define VALIDITY_COUNTER_MAX (5.0f)
#define VALIDITY_COUNTER_MAX_VARIABLE (250.0f)
#define VALIDITY_COUNTER_INC 5
#define VALIDITY_COUNTER_DEC 5
#define VALIDITY_COUNTER_INITIAL_OBSERVE 5
#define VAL_SUM_MIN_FOR_CREATE (30)
#define VAL_SUM_MIN_FOR_KEEP (24)
#define VAL_SUM_MIN_FOR_UNBLACKLIST (100)
#define MIN_BLACKLIST -1
#define SUCC_VAR_INC_FAC (1.01f)
#define FAIL_VAR_INC_FAC 1.1f
#define MAX_VAR (0.5f * 0.5f)
#define VAR_GT_INIT_INITIAL 0.01f * 0.01f
#define VAR_RANDOM_INIT_INITIAL (0.5f * MAX_VAR)
#define MIN_DEPTH 0.05f
#define MAX_EPL_LENGTH_CROP 30.0f
#define MIN_EPL_LENGTH_CROP (3.0f)
#define GRADIENT_SAMPLE_DIST 1.0f
#define SAMPLE_POINT_TO_BORDER 7
#define MAX_ERROR_STEREO (1300.0f)
#define MIN_DISTANCE_ERROR_STEREO (1.5f)
#define STEREO_EPL_VAR_FAC 2.0f
#define DIFF_FAC_SMOOTHING (1.0f * 1.0f)
#define DIFF_FAC_OBSERVE (1.0f * 1.0f)
#define DIFF_FAC_PROP_MERGE (1.0f * 1.0f)
#define MIN_EPL_GRAD_SQUARED (2.0f * 2.0f)
#define MIN_EPL_LENGTH_SQUARED (1.0f * 1.0f)
#define MIN_EPL_ANGLE_SQUARED (0.3f * 0.3f)
#define MAX_DIFF_CONSTANT (40.0f * 40.0f)
#define MAX_DIFF_GRAD_MULT (0.5f * 0.5f)
#define PROP_SLOT_CAP 8

#if defined(LSD_PHASE_TRACE) && defined(__HIP_DEVICE_COMPILE__)
#define OBS_MARK(k) do { if (a.trace && threadIdx.x == 0) a.trace[(blockIdx.x + blockIdx.y * gridDim.x) * 16 + (k)] = clock64(); } while (0)
#define OBS_VAL(k, v) do { if (a.trace && threadIdx.x == 0) a.trace[(blockIdx.x + blockIdx.y * gridDim.x) * 16 + (k)] = (unsigned long long)(v); } while (0)
#else
#define OBS_MARK(k) do { } while (0)
#define OBS_VAL(k, v) do { } while (0)
#endif
// per-pixel arithmetic compiles for the host as well: a developer chasing a parity bit can call it from a scratch program on a CPU
// (nothing in the library or in tests/ does)
#define LSD_HD __host__ __device__ __forceinline__
#define LSD_HD_NOINLINE __host__ __device__

// UNZERO (settings.h:35) evaluates in double in the reference; the float form below returns the same float for every
// float input (|val| is compared against 1e-10, the result is rounded to float either way).
LSD_HD float unzero(float val) {
  return (float)(val < 0 ? (val > -1e-10 ? -1e-10 : (double)val) : (val < 1e-10 ? 1e-10 : (double)val));
}

// getInterpolatedElement, C/util/globalFuncs.h:43-61
LSD_HD float interp1(const float* __restrict__ mat, float x, float y, int width) {
  int ix = (int)x;
  int iy = (int)y;
  float dx = x - ix;
  float dy = y - iy;
  float dxdy = dx * dy;
  const float* bp = mat + ix + iy * width;
  return dxdy * bp[1 + width] + (dy - dxdy) * bp[width] + (dx - dxdy) * bp[1] + (1 - dx - dy + dxdy) * bp[0];
}

// A hypothesis that has just come into being (observeDepthCreate, fill holes, propagateDepth, setFromExistingKF): not blacklisted, no
// reference-frame hint, nothing smoothed yet.  The isValid byte is the caller's (K5 and K6 write the other plane of a ping-pong).
// blacklisted: the fused tile alone passes -1, where K6 drops the hypothesis that K5 created in the same launch.
__device__ __forceinline__ void store_fresh_hypothesis(const HypPlanes& m, const int idx, const float idepth, const float var, const int validity,
                                                       const int blacklisted = 0) {
  m.blacklisted[idx] = blacklisted;
  m.nextID[idx] = 0;
  m.validity[idx] = validity;
  m.idepth[idx] = idepth;
  m.var[idx] = var;
  m.idepth_s[idx] = -1;
  m.var_s[idx] = -1;
}

struct ObserveArgs {
  HypPlanes m;
  LSD_G const float* kfImage;
  LSD_G const float4* kfGrad;
  LSD_G const float* kfMaxGrad;
  LSD_G const StereoRef* refs;
  LSD_G const int* refByID;
  int nByID, byIDOffset, nRefs;
  int reactivated;
  int w, h;
  float fx, fy, cx, cy, fxi, fyi, cxi, cyi;
  float minUseGrad, cameraPixelNoise2;
  int allowNegativeIdepths, useSubpixelStereo;
  int kfNumFramesTrackedOnThis, kfNumMappedOnThis;
#ifdef LSD_PHASE_TRACE
  LSD_G unsigned long long* trace;   // developer build: per-stage timestamps of one traced pixel per workgroup
#endif
  LSD_G unsigned long long* counters;   // null, or (sampled launches while profiling) two words per wave: pixels that entered the search, walk steps
  LSD_G float4* queue;                  // batches, two-launch form: this map's search queue (pixel index bits, epx, epy, -) and its fill count
  LSD_G int* qcount;
  LSD_G const uint16_t* gradCand;       // the keyframe's gradient candidates (lsdhip_frame::d_gradCand; k_observe_select_cand_batch)
  StereoRef one;   // nRefs == 1 (the blockUntilMapped case): the reference travels in the kernel arguments, no staging copy
};

// DepthMap::doLineStereo (DepthMap.cpp:1442-1972) in three parts.  Status codes as in the reference: >= 0 matching error,
// -1 out of bounds, -2 ambiguous / negative, -3 error too large, -4 arithmetic.
//   stereo_setup  (:1449-1611): epipolar segment in the reference image, the five keyframe samples; 0 or a status code;
//   stereo_walk_* (:1622-1744): the walk along the segment -> best / second-best match and their neighbours;
//   stereo_finish (:1746-1972): ambiguity tests, sub-pixel refinement, inverse depth and variance.
// The walk is capped at 1000 steps (the reference loop is unbounded; no finite input reaches the cap).
struct StereoSetup {
  float KinvP0, KinvP1;              // KinvP2 == 1
  float rescaleFactor;
  float realVal_m2, realVal_m1, realVal, realVal_p1, realVal_p2;
  float pFar0, pFar1, pClose0, pClose1, incx, incy, eplLength;
  float gI0, gI1;                    // keyframe gradient at (u, v) (getInterpolatedElement42) for the geometric error term
};
struct WalkResult {
  float best_match_err, second_best_match_err, best_match_errPre, best_match_errPost, best_match_DiffErrPre, best_match_DiffErrPost;
  float best_match_x, best_match_y;
  int loopCBest, loopCSecond, loopCounter;
};

LSD_HD float stereo_setup(const ObserveArgs& a, const StereoRef& rf, const float u, const float v, const float epxn, const float epyn,
                          const float min_idepth, const float prior_idepth, float max_idepth, StereoSetup& S) {
  const int width = a.w, height = a.h;
  const float* __restrict__ kfImg = a.kfImage;
  // the keyframe gradient taps of the geometric-error term (used after the search) depend on (u, v) only: issue their loads
  // now so that they do not add a memory round trip after the walk
  const float4* const gbp = a.kfGrad + (int)u + (int)v * width;
  const float4 gt00 = gbp[0], gt10 = gbp[1], gt01 = gbp[width], gt11 = gbp[1 + width];
  float KinvP0 = a.fxi * u + a.cxi, KinvP1 = a.fyi * v + a.cyi, KinvP2 = 1.0f;
  S.KinvP0 = KinvP0; S.KinvP1 = KinvP1;
  float pInf0 = (rf.K_otherToThis_R[0] * KinvP0 + rf.K_otherToThis_R[1] * KinvP1) + rf.K_otherToThis_R[2] * KinvP2;
  float pInf1 = (rf.K_otherToThis_R[3] * KinvP0 + rf.K_otherToThis_R[4] * KinvP1) + rf.K_otherToThis_R[5] * KinvP2;
  float pInf2 = (rf.K_otherToThis_R[6] * KinvP0 + rf.K_otherToThis_R[7] * KinvP1) + rf.K_otherToThis_R[8] * KinvP2;
  float pReal2 = pInf2 / prior_idepth + rf.K_otherToThis_t[2];
  float rescaleFactor = pReal2 * prior_idepth;
  S.rescaleFactor = rescaleFactor;

  float firstX = u - 2 * epxn * rescaleFactor;
  float firstY = v - 2 * epyn * rescaleFactor;
  float lastX = u + 2 * epxn * rescaleFactor;
  float lastY = v + 2 * epyn * rescaleFactor;
  if (firstX <= 0 || firstX >= width - 2 || firstY <= 0 || firstY >= height - 2 || lastX <= 0 || lastX >= width - 2 ||
      lastY <= 0 || lastY >= height - 2)
    return -1;
  if (!(rescaleFactor > 0.7f && rescaleFactor < 1.4f)) return -1;

  OBS_MARK(2);
  S.realVal_p1 = interp1(kfImg, u + epxn * rescaleFactor, v + epyn * rescaleFactor, width);
  S.realVal_m1 = interp1(kfImg, u - epxn * rescaleFactor, v - epyn * rescaleFactor, width);
  S.realVal = interp1(kfImg, u, v, width);
  S.realVal_m2 = interp1(kfImg, u - 2 * epxn * rescaleFactor, v - 2 * epyn * rescaleFactor, width);
  S.realVal_p2 = interp1(kfImg, u + 2 * epxn * rescaleFactor, v + 2 * epyn * rescaleFactor, width);

  const float Kt0 = rf.K_otherToThis_t[0], Kt1 = rf.K_otherToThis_t[1], Kt2 = rf.K_otherToThis_t[2];
  float pClose0 = pInf0 + Kt0 * max_idepth, pClose1 = pInf1 + Kt1 * max_idepth, pClose2 = pInf2 + Kt2 * max_idepth;
  if (pClose2 < 0.001f) {
    max_idepth = (0.001f - pInf2) / Kt2;
    pClose0 = pInf0 + Kt0 * max_idepth; pClose1 = pInf1 + Kt1 * max_idepth; pClose2 = pInf2 + Kt2 * max_idepth;
  }
  pClose0 = pClose0 / pClose2; pClose1 = pClose1 / pClose2;

  float pFar0 = pInf0 + Kt0 * min_idepth, pFar1 = pInf1 + Kt1 * min_idepth, pFar2 = pInf2 + Kt2 * min_idepth;
  if (pFar2 < 0.001f || max_idepth < min_idepth) return -1;
  pFar0 = pFar0 / pFar2; pFar1 = pFar1 / pFar2;

  if (__builtin_isnan((float)(pFar0 + pClose0))) return -4;

  float incx = pClose0 - pFar0;
  float incy = pClose1 - pFar1;
  float eplLength = sqrtf(incx * incx + incy * incy);
  if (eplLength == 0.0f || __builtin_isinf(eplLength)) return -4;  // `!eplLength > 0 || isinf` of the reference (:1518)

  if (eplLength > MAX_EPL_LENGTH_CROP) {
    pClose0 = pFar0 + incx * MAX_EPL_LENGTH_CROP / eplLength;
    pClose1 = pFar1 + incy * MAX_EPL_LENGTH_CROP / eplLength;
  }
  incx *= GRADIENT_SAMPLE_DIST / eplLength;
  incy *= GRADIENT_SAMPLE_DIST / eplLength;

  pFar0 -= incx; pFar1 -= incy;
  pClose0 += incx; pClose1 += incy;

  if (eplLength < MIN_EPL_LENGTH_CROP) {
    float pad = (MIN_EPL_LENGTH_CROP - (eplLength)) / 2.0f;
    pFar0 -= incx * pad; pFar1 -= incy * pad;
    pClose0 += incx * pad; pClose1 += incy * pad;
  }

  if (pFar0 <= SAMPLE_POINT_TO_BORDER || pFar0 >= width - SAMPLE_POINT_TO_BORDER || pFar1 <= SAMPLE_POINT_TO_BORDER ||
      pFar1 >= height - SAMPLE_POINT_TO_BORDER)
    return -1;

  if (pClose0 <= SAMPLE_POINT_TO_BORDER || pClose0 >= width - SAMPLE_POINT_TO_BORDER || pClose1 <= SAMPLE_POINT_TO_BORDER ||
      pClose1 >= height - SAMPLE_POINT_TO_BORDER) {
    if (pClose0 <= SAMPLE_POINT_TO_BORDER) {
      float toAdd = (SAMPLE_POINT_TO_BORDER - pClose0) / incx;
      pClose0 += toAdd * incx; pClose1 += toAdd * incy;
    } else if (pClose0 >= width - SAMPLE_POINT_TO_BORDER) {
      float toAdd = (width - SAMPLE_POINT_TO_BORDER - pClose0) / incx;
      pClose0 += toAdd * incx; pClose1 += toAdd * incy;
    }
    if (pClose1 <= SAMPLE_POINT_TO_BORDER) {
      float toAdd = (SAMPLE_POINT_TO_BORDER - pClose1) / incy;
      pClose0 += toAdd * incx; pClose1 += toAdd * incy;
    } else if (pClose1 >= height - SAMPLE_POINT_TO_BORDER) {
      float toAdd = (height - SAMPLE_POINT_TO_BORDER - pClose1) / incy;
      pClose0 += toAdd * incx; pClose1 += toAdd * incy;
    }
    float fincx = pClose0 - pFar0;
    float fincy = pClose1 - pFar1;
    float newEplLength = sqrtf(fincx * fincx + fincy * fincy);
    if (pClose0 <= SAMPLE_POINT_TO_BORDER || pClose0 >= width - SAMPLE_POINT_TO_BORDER || pClose1 <= SAMPLE_POINT_TO_BORDER ||
        pClose1 >= height - SAMPLE_POINT_TO_BORDER || newEplLength < 8.0f)
      return -1;
  }
  S.pFar0 = pFar0; S.pFar1 = pFar1; S.pClose0 = pClose0; S.pClose1 = pClose1; S.incx = incx; S.incy = incy; S.eplLength = eplLength;
  {
    // getInterpolatedElement42 on the keyframe gradients (globalFuncs.h:95-109): interpolated here, where the taps have long
    // arrived, so that two values instead of eight stay live across the walk
    const int ix = (int)u, iy = (int)v;
    const float dx = u - ix, dy = v - iy;
    const float dxdy = dx * dy;
    S.gI0 = dxdy * gt11.x + (dy - dxdy) * gt01.x + (dx - dxdy) * gt10.x + (1 - dx - dy + dxdy) * gt00.x;
    S.gI1 = dxdy * gt11.y + (dy - dxdy) * gt01.y + (dx - dxdy) * gt10.y + (1 - dx - dy + dxdy) * gt00.y;
  }
  OBS_MARK(3);
  return 0;
}

// the walk, one lane per search (the reference's loop; two steps of samples kept in flight)
LSD_HD void stereo_walk_serial(const float* __restrict__ refImg, const int width, const StereoSetup& S, WalkResult& W) {
  const float incx = S.incx, incy = S.incy, pClose0 = S.pClose0, pClose1 = S.pClose1;
  const float realVal_p2 = S.realVal_p2, realVal_p1 = S.realVal_p1, realVal = S.realVal, realVal_m1 = S.realVal_m1, realVal_m2 = S.realVal_m2;
  float cpx = S.pFar0;
  float cpy = S.pFar1;
  float val_cp_m2 = interp1(refImg, cpx - 2.0f * incx, cpy - 2.0f * incy, width);
  float val_cp_m1 = interp1(refImg, cpx - incx, cpy - incy, width);
  float val_cp = interp1(refImg, cpx, cpy, width);
  float val_cp_p1 = interp1(refImg, cpx + incx, cpy + incy, width);
  float val_cp_p2;


  int loopCounter = 0;
  float best_match_x = -1;
  float best_match_y = -1;
  float best_match_err = INFINITY;          // `1e50` assigned to a float (:1658)
  float second_best_match_err = INFINITY;
  float best_match_errPre = NAN, best_match_errPost = NAN, best_match_DiffErrPre = NAN, best_match_DiffErrPost = NAN;
  bool bestWasLastLoop = false;
  float eeLast = -1;
  float e1A = NAN, e1B = NAN, e2A = NAN, e2B = NAN, e3A = NAN, e3B = NAN, e4A = NAN, e4B = NAN, e5A = NAN, e5B = NAN;
  int loopCBest = -1, loopCSecond = -1;
  // The sample positions of the walk do not depend on the sampled values, so the loads of the next two steps are kept in
  // flight while a step is evaluated (same positions, formed by the same additions as the loop's own cpx += incx; they stay
  // inside the image: at most 4 samples beyond pClose, which is SAMPLE_POINT_TO_BORDER = 7 pixels away from the border).
  float w1x = cpx + incx, w1y = cpy + incy;
  float w2x = w1x + incx, w2y = w1y + incy;
  float p2_0 = interp1(refImg, cpx + 2 * incx, cpy + 2 * incy, width);
  float p2_1 = interp1(refImg, w1x + 2 * incx, w1y + 2 * incy, width);
  while ((((incx < 0) == (cpx > pClose0) && (incy < 0) == (cpy > pClose1)) || loopCounter == 0) && loopCounter < 1000) {
    const float p2_2 = interp1(refImg, w2x + 2 * incx, w2y + 2 * incy, width);
    val_cp_p2 = p2_0;
    p2_0 = p2_1;
    p2_1 = p2_2;
    w2x += incx;
    w2y += incy;
    float ee = 0;
    if (loopCounter % 2 == 0) {
      e1A = val_cp_p2 - realVal_p2; ee += e1A * e1A;
      e2A = val_cp_p1 - realVal_p1; ee += e2A * e2A;
      e3A = val_cp - realVal;       ee += e3A * e3A;
      e4A = val_cp_m1 - realVal_m1; ee += e4A * e4A;
      e5A = val_cp_m2 - realVal_m2; ee += e5A * e5A;
    } else {
      e1B = val_cp_p2 - realVal_p2; ee += e1B * e1B;
      e2B = val_cp_p1 - realVal_p1; ee += e2B * e2B;
      e3B = val_cp - realVal;       ee += e3B * e3B;
      e4B = val_cp_m1 - realVal_m1; ee += e4B * e4B;
      e5B = val_cp_m2 - realVal_m2; ee += e5B * e5B;
    }
    if (ee < best_match_err) {
      second_best_match_err = best_match_err;
      loopCSecond = loopCBest;
      best_match_err = ee;
      loopCBest = loopCounter;
      best_match_errPre = eeLast;
      best_match_DiffErrPre = e1A * e1B + e2A * e2B + e3A * e3B + e4A * e4B + e5A * e5B;
      best_match_errPost = -1;
      best_match_DiffErrPost = -1;
      best_match_x = cpx;
      best_match_y = cpy;
      bestWasLastLoop = true;
    } else {
      if (bestWasLastLoop) {
        best_match_errPost = ee;
        best_match_DiffErrPost = e1A * e1B + e2A * e2B + e3A * e3B + e4A * e4B + e5A * e5B;
        bestWasLastLoop = false;
      }
      if (ee < second_best_match_err) {
        second_best_match_err = ee;
        loopCSecond = loopCounter;
      }
    }
    eeLast = ee;
    val_cp_m2 = val_cp_m1; val_cp_m1 = val_cp; val_cp = val_cp_p1; val_cp_p1 = val_cp_p2;
    cpx += incx;
    cpy += incy;
    loopCounter++;
  }


  W.best_match_err = best_match_err; W.second_best_match_err = second_best_match_err;
  W.best_match_errPre = best_match_errPre; W.best_match_errPost = best_match_errPost;
  W.best_match_DiffErrPre = best_match_DiffErrPre; W.best_match_DiffErrPost = best_match_DiffErrPost;
  W.best_match_x = best_match_x; W.best_match_y = best_match_y;
  W.loopCBest = loopCBest; W.loopCSecond = loopCSecond; W.loopCounter = loopCounter;
}

LSD_HD float stereo_finish(const ObserveArgs& a, const StereoRef& rf, const float u, const float v, const float epxn, const float epyn,
                           const StereoSetup& S, const WalkResult& W, float& result_idepth, float& result_var, float& result_eplLength) {
  float best_match_err = W.best_match_err, best_match_x = W.best_match_x, best_match_y = W.best_match_y;
  const float second_best_match_err = W.second_best_match_err;
  const float best_match_errPre = W.best_match_errPre, best_match_errPost = W.best_match_errPost;
  const float best_match_DiffErrPre = W.best_match_DiffErrPre, best_match_DiffErrPost = W.best_match_DiffErrPost;
  const int loopCBest = W.loopCBest, loopCSecond = W.loopCSecond;
  const float incx = S.incx, incy = S.incy, rescaleFactor = S.rescaleFactor, eplLength = S.eplLength;
  const float realVal_p2 = S.realVal_p2, realVal_p1 = S.realVal_p1, realVal = S.realVal, realVal_m1 = S.realVal_m1, realVal_m2 = S.realVal_m2;
  const float KinvP0 = S.KinvP0, KinvP1 = S.KinvP1, KinvP2 = 1.0f;
  if (best_match_err > 4.0f * (float)MAX_ERROR_STEREO) return -3;
  if (abs(loopCBest - loopCSecond) > 1.0f && MIN_DISTANCE_ERROR_STEREO * best_match_err > second_best_match_err) return -2;
  bool didSubpixel = false;
  if (a.useSubpixelStereo) {
    float gradPre_pre = -(best_match_errPre - best_match_DiffErrPre);
    float gradPre_this = +(best_match_err - best_match_DiffErrPre);
    float gradPost_this = -(best_match_err - best_match_DiffErrPost);
    float gradPost_post = +(best_match_errPost - best_match_DiffErrPost);
    bool interpPost = false;
    bool interpPre = false;
    if ((gradPost_this < 0) ^ (gradPre_this < 0)) {
    } else if ((gradPre_pre < 0) ^ (gradPre_this < 0)) {
      if ((gradPost_post < 0) ^ (gradPost_this < 0)) {
      } else
        interpPre = true;
    } else if ((gradPost_post < 0) ^ (gradPost_this < 0)) {
      interpPost = true;
    }
    if (interpPre) {
      float d = gradPre_this / (gradPre_this - gradPre_pre);
      best_match_x -= d * incx;
      best_match_y -= d * incy;
      best_match_err = best_match_err - 2 * d * gradPre_this - (gradPre_pre - gradPre_this) * d * d;
      didSubpixel = true;
    } else if (interpPost) {
      float d = gradPost_this / (gradPost_this - gradPost_post);
      best_match_x += d * incx;
      best_match_y += d * incy;
      best_match_err = best_match_err + 2 * d * gradPost_this + (gradPost_post - gradPost_this) * d * d;
      didSubpixel = true;
    }
  }

  float sampleDist = GRADIENT_SAMPLE_DIST * rescaleFactor;
  float gradAlongLine = 0;
  float tmp = realVal_p2 - realVal_p1; gradAlongLine += tmp * tmp;
  tmp = realVal_p1 - realVal;          gradAlongLine += tmp * tmp;
  tmp = realVal - realVal_m1;          gradAlongLine += tmp * tmp;
  tmp = realVal_m1 - realVal_m2;       gradAlongLine += tmp * tmp;
  gradAlongLine /= sampleDist * sampleDist;

  if (best_match_err > (float)MAX_ERROR_STEREO + sqrtf(gradAlongLine) * 20) return -3;

  float idnew_best_match;
  float alpha;
  if (incx * incx > incy * incy) {
    float oldX = a.fxi * best_match_x + a.cxi;
    float nominator = (oldX * rf.otherToThis_t[2] - rf.otherToThis_t[0]);
    // Vector3f::dot — Eigen redux order x0 + (x1 + x2)
    float dot0 = KinvP0 * rf.row0[0] + (KinvP1 * rf.row0[1] + KinvP2 * rf.row0[2]);
    float dot2 = KinvP0 * rf.row2[0] + (KinvP1 * rf.row2[1] + KinvP2 * rf.row2[2]);
    idnew_best_match = (dot0 - oldX * dot2) / nominator;
    alpha = incx * a.fxi * (dot0 * rf.otherToThis_t[2] - dot2 * rf.otherToThis_t[0]) / (nominator * nominator);
  } else {
    float oldY = a.fyi * best_match_y + a.cyi;
    float nominator = (oldY * rf.otherToThis_t[2] - rf.otherToThis_t[1]);
    float dot1 = KinvP0 * rf.row1[0] + (KinvP1 * rf.row1[1] + KinvP2 * rf.row1[2]);
    float dot2 = KinvP0 * rf.row2[0] + (KinvP1 * rf.row2[1] + KinvP2 * rf.row2[2]);
    idnew_best_match = (dot1 - oldY * dot2) / nominator;
    alpha = incy * a.fyi * (dot1 * rf.otherToThis_t[2] - dot2 * rf.otherToThis_t[1]) / (nominator * nominator);
  }

  if (idnew_best_match < 0) {
    if (!a.allowNegativeIdepths) return -2;
  }

  float photoDispError = 4.0f * a.cameraPixelNoise2 / (gradAlongLine + DIVISION_EPS);
  float trackingErrorFac = 0.25f * (1.0f + rf.initialTrackedResidual);
  const float gI0 = S.gI0, gI1 = S.gI1;
  float geoDispError = (gI0 * epxn + gI1 * epyn) + DIVISION_EPS;
  geoDispError = trackingErrorFac * trackingErrorFac * (gI0 * gI0 + gI1 * gI1) / (geoDispError * geoDispError);
  OBS_MARK(6);
  result_var = alpha * alpha * ((didSubpixel ? 0.05f : 0.5f) * sampleDist * sampleDist + geoDispError + photoDispError);
  result_idepth = idnew_best_match;
  result_eplLength = eplLength;
  return best_match_err;
}


LSD_HD_NOINLINE float do_line_stereo(const ObserveArgs& a, const StereoRef& rf, const float u, const float v, const float epxn,
                                const float epyn, const float min_idepth, const float prior_idepth, float max_idepth,
                                float& result_idepth, float& result_var, float& result_eplLength, int& steps) {
  StereoSetup S;
  steps = 0;
  const float st = stereo_setup(a, rf, u, v, epxn, epyn, min_idepth, prior_idepth, max_idepth, S);
  if (st < 0) return st;
  WalkResult W;
  stereo_walk_serial(rf.image, a.w, S, W);
  steps = W.loopCounter;
  return stereo_finish(a, rf, u, v, epxn, epyn, S, W, result_idepth, result_var, result_eplLength);
}

// DepthMap::makeAndCheckEPL (DepthMap.cpp:184-234)
// (the four keyframe-image taps of the gradient travel as arguments: the caller loads them together with the other
// per-pixel inputs, one memory round trip instead of one per check)
LSD_HD bool make_and_check_epl(const ObserveArgs& a, const StereoRef& rf, int x, int y, float kR, float kL, float kD, float kU, float* pepx,
                               float* pepy) {
  float epx = -a.fx * rf.thisToOther_t[0] + rf.thisToOther_t[2] * (x - a.cx);
  float epy = -a.fy * rf.thisToOther_t[1] + rf.thisToOther_t[2] * (y - a.cy);
  if (__builtin_isnan(epx + epy)) return false;
  float eplLengthSquared = epx * epx + epy * epy;
  if (eplLengthSquared < MIN_EPL_LENGTH_SQUARED) return false;
  float gx = kR - kL;
  float gy = kD - kU;
  float eplGradSquared = gx * epx + gy * epy;
  eplGradSquared = eplGradSquared * eplGradSquared / eplLengthSquared;
  if (eplGradSquared < MIN_EPL_GRAD_SQUARED) return false;
  if (eplGradSquared / (gx * gx + gy * gy) < MIN_EPL_ANGLE_SQUARED) return false;
  // the reference calls the C library's double sqrt() here (unqualified sqrt in DepthMap.cpp:229), so the quotient is
  // formed in double and rounded to float once; f64 sqrt / divide are IEEE-exact on gfx950
  float fac = (float)((double)GRADIENT_SAMPLE_DIST / sqrt((double)eplLengthSquared));
  *pepx = epx * fac;
  *pepy = epy * fac;
  return true;
}

// observeDepthRow body for one pixel (DepthMap.cpp:117-143), in two halves:
//   front: everything up to and including makeAndCheckEPL — the cheap rejections every pixel goes through; passes the pixels that go on to
//          the epipolar search (their share is given with each kernel below), with the reference frame and the EPL direction.
//          Its tests, in the reference's order, are the three predicates below; observe_front (one pixel per lane) and
//          observe_front4 (four, their loads staged) differ in how they load, not in what they test;
//   observe_back: doLineStereo and observeDepthCreate / observeDepthUpdate's bookkeeping for such a pixel.
// k_observe runs both in the same lane: for ONE map the select + walk form further down (k_observe_select_batch + k_observe_walk_batch) and a
// form that loads all samples of short walks up front were measured in round 2 and lost, 37-52 us and 28 us against 21 us.
// (1) :121-131: a pixel below the gradient threshold loses its hypothesis (the front half's one store); it and a blacklisted pixel search nothing
LSD_HD bool obs_cheap_pass(const ObserveArgs& a, const int idx, const bool hasHypothesis, const float maxGrad, const int blacklisted) {
  if (hasHypothesis && maxGrad < a.minUseGrad) { a.m.valid[idx] = 0; return false; }
  return !(maxGrad < a.minUseGrad || blacklisted < MIN_BLACKLIST);
}
// (2) the reference frame a pixel searches (observeDepthCreate :243, observeDepthUpdate :311-320); false: nextStereoFrameMinID lies beyond the newest
template <bool ONE>
LSD_HD bool obs_pick_ref(const ObserveArgs& a, const bool hasHypothesis, const float nextID, int& refIdx) {
  refIdx = a.reactivated ? a.nRefs - 1 : 0;
  if (hasHypothesis && !a.reactivated) {
    const int rel = (int)nextID - a.byIDOffset;
    if (rel >= a.nByID) return false;
    refIdx = (ONE || rel < 0) ? 0 : a.refByID[rel];
  }
  return true;
}
// (3) the tracking mask of the reference frame (observeDepthCreate :246-252 / observeDepthUpdate :323-329), then makeAndCheckEPL
LSD_HD bool obs_uses_mask(const StereoRef& rf) { return rf.parentIsKF && rf.wasGood != nullptr; }
LSD_HD bool obs_mask_epl(const ObserveArgs& a, const StereoRef& rf, const int x, const int y, const uint8_t wasGoodHere, const float kR, const float kL,
                         const float kD, const float kU, float* pepx, float* pepy) {
  if (!wasGoodHere) return false;
  return make_and_check_epl(a, rf, x, y, kR, kL, kD, kU, pepx, pepy);
}
template <bool ONE>
LSD_HD bool observe_front(const ObserveArgs& a, const int x, const int y, int& refIdxOut, float& epxOut, float& epyOut) {
  if (x < 3 || x >= a.w - 3 || y < 3 || y >= a.h - 3) return false;
  const int idx = x + y * a.w;
  // The per-pixel inputs are loaded in two batches, each issued before any of its values is tested, so that the checks
  // below cost two memory round trips instead of one each (every plane was last written by a kernel on another XCD):
  // batch 1 = what the cheap rejections need (13 B per pixel, every pixel), batch 2 = everything else of this pixel.
  const bool hasHypothesis = a.m.valid[idx] != 0;
  const float maxGrad = a.kfMaxGrad[idx];
  const int blacklisted0 = a.m.blacklisted[idx];
  const float nextID = a.m.nextID[idx];
  if (!obs_cheap_pass(a, idx, hasHypothesis, maxGrad, blacklisted0)) return false;
  int refIdx = 0;
  if (!obs_pick_ref<ONE>(a, hasHypothesis, nextID, refIdx)) return false;
  const StereoRef& rf = ONE ? a.one : a.refs[refIdx];
  const uint8_t wasGoodHere = obs_uses_mask(rf) ? rf.wasGood[(x >> 1) + (a.w >> 1) * (y >> 1)] : (uint8_t)1;
  const float kR = a.kfImage[idx + 1], kL = a.kfImage[idx - 1], kD = a.kfImage[idx + a.w], kU = a.kfImage[idx - a.w];
  if (!obs_mask_epl(a, rf, x, y, wasGoodHere, kR, kL, kD, kU, &epxOut, &epyOut)) return false;
  refIdxOut = refIdx;
  return true;
}

struct ObsPixel {        // what the back half needs of a pixel's hypothesis
  bool hasHypothesis;
  float maxGrad;
  int blacklisted0, validity0;
  float idepth_smoothed, var_smoothed, var0, idepth0;
  float min_idepth, prior_idepth, max_idepth;    // search interval handed to doLineStereo
};
LSD_HD void observe_back_load(const ObserveArgs& a, const int idx, ObsPixel& P) {
  P.hasHypothesis = a.m.valid[idx] != 0;
  P.maxGrad = a.kfMaxGrad[idx];
  P.blacklisted0 = a.m.blacklisted[idx];
  P.idepth_smoothed = a.m.idepth_s[idx];
  P.var_smoothed = a.m.var_s[idx];
  P.var0 = a.m.var[idx];
  P.idepth0 = a.m.idepth[idx];
  P.validity0 = a.m.validity[idx];
  if (!P.hasHypothesis) {          // observeDepthCreate (DepthMap.cpp:269-270)
    P.min_idepth = 0.0f; P.prior_idepth = 1.0f; P.max_idepth = 1.0f / MIN_DEPTH;
  } else {                         // observeDepthUpdate (:334-341)
    float sv = sqrtf(P.var_smoothed);
    float min_idepth = P.idepth_smoothed - sv * STEREO_EPL_VAR_FAC;
    float max_idepth = P.idepth_smoothed + sv * STEREO_EPL_VAR_FAC;
    if (min_idepth < 0) min_idepth = 0;
    if (max_idepth > 1 / MIN_DEPTH) max_idepth = 1 / MIN_DEPTH;
    P.min_idepth = min_idepth; P.prior_idepth = P.idepth_smoothed; P.max_idepth = max_idepth;
  }
}
// what observeDepthCreate (:272-291) / observeDepthUpdate (:346-471) do with doLineStereo's verdict
LSD_HD void observe_back_store(const ObserveArgs& a, const StereoRef& rf, const int idx, const ObsPixel& P, const float error,
                               float result_idepth, const float result_var, const float result_eplLength) {
  const int blacklisted0 = P.blacklisted0, validity0 = P.validity0;
  const float var0 = P.var0, idepth0 = P.idepth0, idepth_smoothed = P.idepth_smoothed, var_smoothed = P.var_smoothed, maxGrad = P.maxGrad;
  if (!P.hasHypothesis) {
    if (error == -3 || error == -2) a.m.blacklisted[idx] = blacklisted0 - 1;
    if (error < 0 || result_var > MAX_VAR) return;
    a.m.valid[idx] = 1;
    store_fresh_hypothesis(a.m, idx, unzero(result_idepth), result_var, VALIDITY_COUNTER_INITIAL_OBSERVE);
    return;
  }
  float diff = result_idepth - idepth_smoothed;
  if (error == -1) return;
  if (error == -2) {
    int vc = validity0 - VALIDITY_COUNTER_DEC;
    if (vc < 0) vc = 0;
    a.m.validity[idx] = vc;
    a.m.nextID[idx] = 0;
    float nv = var0 * FAIL_VAR_INC_FAC;
    a.m.var[idx] = nv;
    if (nv > MAX_VAR) { a.m.valid[idx] = 0; a.m.blacklisted[idx] = blacklisted0 - 1; }
    return;
  }
  if (error == -3 || error == -4) return;
  if (DIFF_FAC_OBSERVE * diff * diff > result_var + var_smoothed) {
    float nv = var0 * FAIL_VAR_INC_FAC;
    a.m.var[idx] = nv;
    if (nv > MAX_VAR) a.m.valid[idx] = 0;
    return;
  }
  {
    const float old_var = var0;
    float id_var = old_var * SUCC_VAR_INC_FAC;
    float w = result_var / (result_var + id_var);
    float new_idepth = (1 - w) * result_idepth + w * idepth0;
    a.m.idepth[idx] = unzero(new_idepth);
    id_var = id_var * w;
    if (id_var < old_var) a.m.var[idx] = id_var;
    int vc = validity0 + VALIDITY_COUNTER_INC;
    float absGrad = maxGrad;
    if (vc > VALIDITY_COUNTER_MAX + absGrad * (VALIDITY_COUNTER_MAX_VARIABLE) / 255.0f)
      vc = VALIDITY_COUNTER_MAX + absGrad * (VALIDITY_COUNTER_MAX_VARIABLE) / 255.0f;
    a.m.validity[idx] = vc;
    if (result_eplLength < MIN_EPL_LENGTH_CROP) {
      float inc = a.kfNumFramesTrackedOnThis / (float)(a.kfNumMappedOnThis + 5);
      if (inc < 3) inc = 3;
      inc += ((int)(result_eplLength * 10000) % 2);
      if (result_eplLength < 0.5 * MIN_EPL_LENGTH_CROP) inc *= 3;
      a.m.nextID[idx] = rf.id + inc;
    }
  }
}
template <bool ONE>
LSD_HD_NOINLINE int observe_back(const ObserveArgs& a, const int idx, const int refIdx, const float epx, const float epy) {
  const int x = idx % a.w, y = idx / a.w;
  const StereoRef& rf = ONE ? a.one : a.refs[refIdx];
  ObsPixel P;
  observe_back_load(a, idx, P);
  float result_idepth = 0, result_var = 0, result_eplLength = 0;   // uninitialised in the reference (:344)
  int steps;
  const float error = do_line_stereo(a, rf, x, y, epx, epy, P.min_idepth, P.prior_idepth, P.max_idepth, result_idepth, result_var, result_eplLength, steps);
  observe_back_store(a, rf, idx, P, error, result_idepth, result_var, result_eplLength);
  return steps;
}

// returns -1 for a pixel the cheap tests reject, else the number of walk steps of its epipolar search
template <bool ONE>
LSD_HD int observe_pixel(const ObserveArgs& a, const int x, const int y) {
  int refIdx = 0;
  float epx = 0, epy = 0;
  if (observe_front<ONE>(a, x, y, refIdx, epx, epy)) return observe_back<ONE>(a, x + y * a.w, refIdx, epx, epy);
  return -1;
}
// measurement (sampled launches): the wave's number of searches and walk steps -> its slot of a.counters
__device__ __forceinline__ void observe_count(const ObserveArgs& a, const int steps) {
  if (a.counters == nullptr) return;
  const unsigned long long act = __popcll(__ballot(steps >= 0));
  const int s = lsd_wave_sum(steps > 0 ? steps : 0);
  if ((threadIdx.x & 63) == 0) {
    const size_t wv = ((size_t)blockIdx.x + (size_t)blockIdx.y * gridDim.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
    a.counters[2 * wv] = act;
    a.counters[2 * wv + 1] = (unsigned long long)s;
  }
}
__global__ __launch_bounds__(256) void k_obs_count_sum(const unsigned long long* __restrict__ counters, int nwaves, unsigned long long* __restrict__ acc) {
  unsigned long long a0 = 0, b0 = 0;
  for (int i = threadIdx.x; i < nwaves; i += 256) { a0 += counters[2 * i]; b0 += counters[2 * i + 1]; }
  lsd_block_tree_sum(a0, b0);
  if (threadIdx.x == 0) { acc[0] += a0; acc[1] += b0; acc[2] += 1; }
}

// K4: observeDepthRow over the whole map, one pixel per lane.  (Compacting the candidate pixels, about 20 % of the map in
// profiles/r01_notes.md's run, into dense waves, and batching the loads of four walk steps, were both measured and gave nothing: the kernel
// is bound by chains of dependent first-touch loads, not by issue slots — profiles/r01_notes.md.)
// ROWS = rows of the 32-pixel-wide tile a workgroup owns (workgroup size 32 * ROWS).  The kernel has no barriers and no LDS,
// so the workgroup is only a scheduling unit: small workgroups free their wave slots as soon as their own lanes are done
// (ROWS = 2, 64-thread workgroups, measured best: +2.5 % Mpixel/s over 256; the developer build with per-stage timestamps takes 8).
template <bool ONE, int ROWS>
__global__ __launch_bounds__(32 * ROWS) void k_observe(ObserveArgs a) {
  const int x = blockIdx.x * 32 + (threadIdx.x & 31);
  const int y = blockIdx.y * ROWS + (threadIdx.x >> 5);
  OBS_MARK(0);
  const int steps = observe_pixel<ONE>(a, x, y);
  observe_count(a, steps);
  OBS_MARK(7);
}

// the same over the maps of several sequences (blockIdx.z = map; lsdhip_depth_update_batch): one reference frame per map, its
// arguments read from a device array (uniform per workgroup: scalar loads)
template <int ROWS>
__global__ __launch_bounds__(32 * ROWS) void k_observe_batch(const ObserveArgs* __restrict__ items) {
  const ObserveArgs& a = items[blockIdx.z];
  const int x = blockIdx.x * 32 + (threadIdx.x & 31);
  const int y = blockIdx.y * ROWS + (threadIdx.x >> 5);
  (void)observe_pixel<true>(a, x, y);
}

// ---- K7: propagateDepth (DepthMap.cpp:475-653) ---------------------------------------------------------------------
struct PropArgs {
  HypPlanes src;   // currentDepthMap (old keyframe)
  HypPlanes dst;   // otherDepthMap (new keyframe)
  LSD_G const float* oldKFImage;
  LSD_G const float* newKFImage;
  LSD_G const float* newKFMaxGrad;
  LSD_G const uint8_t* trackingWasGood;  // level-1 mask of the new keyframe or nullptr
  LSD_G float4* cand;
  LSD_G int* slotCount;
  LSD_G int* slots;
  LSD_G int* flags;      // [0] error (chain storage exhausted), [1] chain entries handed out
  LSD_G int* ovfHead;    // per target: newest chain entry or -1
  LSD_G int2* ovf;       // (source index, next entry)
  int ovfCap;
  int w, h;
  float fx, fy, cx, cy, fxi, fyi, cxi, cyi;
  float R[9], t[3];
  float minUseGrad;
};
// phase A for one valid source hypothesis (its smoothed inverse depth, variance and validity counter): target pixel and candidate,
// registered in the target's slot list.  The slot lists, chain heads and flags are clean at rest: k_prop_resolve leaves slotCount = 0 /
// ovfHead = -1 behind, the kernel that reads the flags zeroes them.
__device__ __forceinline__ void prop_candidate(const PropArgs& a, const int x, const int y, const int idx, const float ids, const float srcVar,
                                               const int srcValidity) {
  float r0 = x * a.fxi + a.cxi, r1 = y * a.fyi + a.cyi, r2 = 1.0f;
  float Rr0 = (a.R[0] * r0 + a.R[1] * r1) + a.R[2] * r2;
  float Rr1 = (a.R[3] * r0 + a.R[4] * r1) + a.R[5] * r2;
  float Rr2 = (a.R[6] * r0 + a.R[7] * r1) + a.R[8] * r2;
  float pn0 = Rr0 / ids + a.t[0], pn1 = Rr1 / ids + a.t[1], pn2 = Rr2 / ids + a.t[2];
  float new_idepth = lsd_rcp_exact(pn2);
  float u_new = pn0 * new_idepth * a.fx + a.cx;
  float v_new = pn1 * new_idepth * a.fy + a.cy;
  if (!(u_new > 2.1f && v_new > 2.1f && u_new < a.w - 3.1f && v_new < a.h - 3.1f)) return;
  int newIDX = (int)(u_new + 0.5f) + ((int)(v_new + 0.5f)) * a.w;
  float destAbsGrad = a.newKFMaxGrad[newIDX];
  if (a.trackingWasGood != nullptr) {
    if (!a.trackingWasGood[(x >> 1) + (a.w >> 1) * (y >> 1)] || destAbsGrad < a.minUseGrad) return;
  } else {
    float sourceColor = a.oldKFImage[idx];
    float destColor = interp1(a.newKFImage, u_new, v_new, a.w);
    float residual = destColor - sourceColor;
    if (residual * residual / (MAX_DIFF_CONSTANT + MAX_DIFF_GRAD_MULT * destAbsGrad * destAbsGrad) > 1.0f || destAbsGrad < a.minUseGrad) return;
  }
  float idepth_ratio_4 = new_idepth / ids;
  idepth_ratio_4 *= idepth_ratio_4;
  idepth_ratio_4 *= idepth_ratio_4;
  float new_var = idepth_ratio_4 * srcVar;
  a.cand[idx] = make_float4(new_idepth, new_var, __int_as_float(srcValidity), 0.f);
  int pos = atomicAdd(&a.slotCount[newIDX], 1);
  if (pos < PROP_SLOT_CAP) a.slots[(size_t)newIDX * PROP_SLOT_CAP + pos] = idx;
  else {
    // more sources than slots for this target (zoom-out / backward motion): the rest go on a per-target chain
    const int o = atomicAdd(&a.flags[1], 1);
    if (o < a.ovfCap) a.ovf[o] = make_int2(idx, atomicExch(&a.ovfHead[newIDX], o));
    else atomicExch(&a.flags[0], 1);
  }
}

// The same for many maps in TWO launches (lsdhip_depth_update_batch from LSD_OBS_SPLIT_MIN_MAPS maps on).  In k_observe_batch a wave
// that holds a single searching pixel walks the whole dependent chain of doLineStereo at 126 registers per lane with one lane busy, and
// three waves in four hold one (2-7 % of the pixels search in the 32-sequence loop: profiles/r05_notes.md section 2).  With enough maps in a
// launch to fill the chip that is what bounds it, not
// the planes it reads.  So: k_observe_select_batch runs observe_front — the cheap rejections, a streaming pass at few registers — over
// every pixel (four per lane, their loads in flight together) and appends the survivors of a 64x16 tile, compacted, to their map's queue
// (one atomic per tile); k_observe_walk_batch
// runs observe_back over the queues with every lane busy: chunks of 64 consecutive entries (neighbouring tiles: shared lines), dealt to a
// fixed number of one-wave workgroups.  A pixel's update reads and writes nothing but its own hypothesis and constant planes, so the
// order of the queue does not matter: every plane is bit-identical to the one-launch form (tests/test_multiseq_gpu.py).
// (For ONE map the split was measured in round 2 and lost — two latency-bound launches instead of one; it stays one launch there.)
#define LSD_OBS_WALK_MAX_MAPS 256
// observe_front<true> for the four pixels (x, y0 + 4 k) of a lane, staged: the 13 bytes every pixel pays for the cheap rejections of all
// four are requested before the first is looked at, likewise the second batch (mask byte, four keyframe-image taps) of the survivors —
// the pass is a chain of two dependent memory round trips per pixel, and a lane that keeps eight of them in flight needs a quarter of
// the residency rounds (the one-pixel form ran at 1.7 TB/s: 0.84 of its wave cycles waiting, profiles/r05_notes.md).
// The tests are observe_front's: the same three predicates in the same order (incl. the one store of the first).
// CAND: the four pixels come from the keyframe's gradient candidates (k_observe_select_cand_batch): the border and gradient tests are
// already answered (and no hypothesis sits below the threshold: lsdhip_depthmap::lowGradHypPossible), maxGradients is not read: the
// first predicate is handed the threshold itself, which passes its gradient test.
template <bool CAND>
__device__ __forceinline__ void observe_front4(const ObserveArgs& a, const int (&xs)[4], const int (&ys)[4], const bool (&in)[4], bool (&hit)[4],
                                               float (&epx)[4], float (&epy)[4]) {
  const StereoRef& rf = a.one;
  const bool useMask = obs_uses_mask(rf);
  bool hyp[4];
  int idx[4], bl[4];
  float mg[4], nid[4];
  uint8_t val[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    idx[k] = in[k] ? xs[k] + ys[k] * a.w : 0;
    if (CAND) {
      // (a quarter of the slots of a group hold a candidate on a typical keyframe: only those request anything)
      val[k] = 0; bl[k] = 0; nid[k] = 0.f; mg[k] = a.minUseGrad;
      if (in[k]) { val[k] = a.m.valid[idx[k]]; bl[k] = a.m.blacklisted[idx[k]]; nid[k] = a.m.nextID[idx[k]]; }
    } else {
      val[k] = a.m.valid[idx[k]];
      mg[k] = a.kfMaxGrad[idx[k]];
      bl[k] = a.m.blacklisted[idx[k]];
      nid[k] = a.m.nextID[idx[k]];
    }
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    hyp[k] = val[k] != 0;
    int refIdx;      // (one reference: a.one whatever the index)
    hit[k] = in[k] && obs_cheap_pass(a, idx[k], hyp[k], mg[k], bl[k]) && obs_pick_ref<true>(a, hyp[k], nid[k], refIdx);
  }
  uint8_t good[4];
  float kR[4], kL[4], kD[4], kU[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int x = xs[k], y = ys[k];
    const int j = hit[k] ? idx[k] : a.w + 1;                          // (a pixel with all four neighbours inside the plane)
    if (CAND) {
      good[k] = 1; kR[k] = kL[k] = kD[k] = kU[k] = 0.f;
      if (hit[k]) {
        if (useMask) good[k] = rf.wasGood[(x >> 1) + (a.w >> 1) * (y >> 1)];
        kR[k] = a.kfImage[j + 1]; kL[k] = a.kfImage[j - 1]; kD[k] = a.kfImage[j + a.w]; kU[k] = a.kfImage[j - a.w];
      }
    } else {
      good[k] = (useMask && hit[k]) ? rf.wasGood[(x >> 1) + (a.w >> 1) * (y >> 1)] : (uint8_t)1;
      kR[k] = a.kfImage[j + 1]; kL[k] = a.kfImage[j - 1]; kD[k] = a.kfImage[j + a.w]; kU[k] = a.kfImage[j - a.w];
    }
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    epx[k] = 0; epy[k] = 0;
    if (hit[k]) hit[k] = obs_mask_epl(a, rf, xs[k], ys[k], good[k], kR[k], kL[k], kD[k], kU[k], &epx[k], &epy[k]);
  }
}
// the survivors of a workgroup's pixels, compacted, go to their map's queue (one atomic per workgroup and call)
__device__ __forceinline__ void observe_queue_append(const ObserveArgs& a, const int (&xs)[4], const int (&ys)[4], const bool (&hit)[4],
                                                     const float (&epx)[4], const float (&epy)[4], int* s_wcount, int* s_base) {
  const int tid = threadIdx.x, wave = tid >> 6;
  int rank[4], wc = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const unsigned long long bal = __ballot(hit[k]);
    rank[k] = wc + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
    wc += __popcll(bal);
  }
  if ((tid & 63) == 0) s_wcount[wave] = wc;
  __syncthreads();
  if (tid == 0) {
    const int tot = (s_wcount[0] + s_wcount[1]) + (s_wcount[2] + s_wcount[3]);
    *s_base = tot > 0 ? atomicAdd(a.qcount, tot) : 0;
  }
  __syncthreads();
  int off = *s_base;
#pragma unroll
  for (int k = 0; k < 4; k++) off += k < wave ? s_wcount[k] : 0;
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (hit[k]) a.queue[off + rank[k]] = make_float4(__int_as_float(xs[k] + ys[k] * a.w), epx[k], epy[k], 0.f);
}
__global__ __launch_bounds__(256) void k_observe_select_batch(const ObserveArgs* __restrict__ items) {
  const ObserveArgs& a = items[blockIdx.z];
  __shared__ int s_wcount[4];
  __shared__ int s_base;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int x = blockIdx.x * 64 + lane;
  const int y0 = blockIdx.y * 16 + wave;                              // the lane's pixels: rows y0, y0 + 4, y0 + 8, y0 + 12 of the 64x16 tile
  int xs[4], ys[4];
  bool in[4], hit[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    xs[k] = x; ys[k] = y0 + 4 * k;
    in[k] = !(x < 3 || x >= a.w - 3 || ys[k] < 3 || ys[k] >= a.h - 3);
  }
  float epx[4], epy[4];
  observe_front4<false>(a, xs, ys, in, hit, epx, epy);
  observe_queue_append(a, xs, ys, hit, epx, epy, s_wcount, &s_base);
}
// The select pass over the keyframe's gradient candidates (round 6): the two tests that depend on the keyframe alone — the 3-pixel border
// and maxGradients >= minUseGrad, which three pixels in four fail on a typical keyframe — were answered when the frame became a keyframe
// (k_grad_candidates, frame.hip).  One wave per group of 1024 consecutive pixels walks the group's list, 256 candidates per trip, four per
// lane with their loads in flight together (the entries of a trip are requested before the count is known: beyond it they are ignored):
// a quarter of the waves of the every-pixel pass, each with one more (short) round trip, and only candidates request hypothesis planes.
// Used when no map of the call can hold a hypothesis below the threshold (lsdhip_depthmap::lowGradHypPossible); same tests in the same
// order on the same pixels otherwise, and the queue's order is immaterial: every plane bit-identical (tests/test_multiseq_gpu.py).
__global__ __launch_bounds__(256) void k_observe_select_cand_batch(const ObserveArgs* __restrict__ items) {
  const ObserveArgs& a = items[blockIdx.z];
  __shared__ int s_wcount[4];
  __shared__ int s_base;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n0 = a.w * a.h, ngroups = (n0 + 1023) >> 10;
  const int g = blockIdx.x * 4 + wave;
  const bool live = g < ngroups;
  LSD_G const uint16_t* list = a.gradCand + (size_t)(live ? g : 0) * 1024;
  const int count = live ? (int)a.gradCand[(size_t)ngroups * 1024 + g] : 0;
  int maxCount = count;                                                // (the workgroup's waves take the same number of trips: the appends hold barriers)
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int gq = blockIdx.x * 4 + q;
    const int cq = gq < ngroups ? (int)a.gradCand[(size_t)ngroups * 1024 + gq] : 0;
    maxCount = cq > maxCount ? cq : maxCount;
  }
  const float inv_w = 1.0f / (float)a.w;
  for (int e0 = 0; e0 < maxCount; e0 += 256) {
    int xs[4], ys[4];
    bool in[4], hit[4];
    unsigned off[4];
#pragma unroll
    for (int k = 0; k < 4; k++) off[k] = list[e0 + lane + 64 * k];      // (within the group's 1024 slots)
#pragma unroll
    for (int k = 0; k < 4; k++) {
      in[k] = e0 + lane + 64 * k < count;
      const int i = (g << 10) + (int)off[k];
      int y = (int)((float)i * inv_w);
      int x = i - y * a.w;
      if (x < 0) { y--; x += a.w; }
      if (x >= a.w) { y++; x -= a.w; }
      xs[k] = in[k] ? x : 3; ys[k] = in[k] ? y : 3;
    }
    float epx[4], epy[4];
    observe_front4<true>(a, xs, ys, in, hit, epx, epy);
    observe_queue_append(a, xs, ys, hit, epx, epy, s_wcount, &s_base);
    __syncthreads();                                                   // (s_wcount / s_base are reused by the next trip)
  }
}
// (144 registers, three waves per SIMD; capped at 128 — four waves, 32 bytes of scratch per lane — the 32-sequence loop ran the same:
// profiles/r05_notes.md)
__global__ __launch_bounds__(64) void k_observe_walk_batch(const ObserveArgs* __restrict__ items, const int* __restrict__ counts, int n,
                                                           unsigned long long* __restrict__ acc) {
  __shared__ int s_incl[LSD_OBS_WALK_MAX_MAPS];     // chunks of 64 entries of maps 0 .. m (inclusive)
  __shared__ int s_cnt[LSD_OBS_WALK_MAX_MAPS];
  const int lane = threadIdx.x;
  int TC = 0, total = 0;
#pragma unroll
  for (int c = 0; c < LSD_OBS_WALK_MAX_MAPS / 64; c++) {
    const int m = c * 64 + lane;
    const int cnt = m < n ? counts[m < n ? m : 0] : 0;
    total += cnt;
    int v = (cnt + 63) >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int u = __shfl_up(v, off); if (lane >= off) v += u; }
    s_incl[m] = TC + v;
    s_cnt[m] = cnt;
    TC += __builtin_amdgcn_readlane(v, 63);
  }
  __syncthreads();
  if (acc != nullptr && blockIdx.x == 0) {     // sampled launch (profiling): its searches
    total = lsd_wave_sum(total);
    if (lane == 0) { atomicAdd(&acc[0], (unsigned long long)total); atomicAdd(&acc[65], 1ull); }
  }
  for (int ck = (int)blockIdx.x; ck < TC; ck += (int)gridDim.x) {
    int m = 0;
#pragma unroll
    for (int c = 0; c < LSD_OBS_WALK_MAX_MAPS / 64; c++) m += __popcll(__ballot(s_incl[c * 64 + lane] <= ck));
    m = __builtin_amdgcn_readfirstlane(m);
    const int e = ((ck - (m > 0 ? s_incl[m - 1] : 0)) << 6) + lane;
    int steps = 0;
    if (e < s_cnt[m]) {
      const ObserveArgs& a = items[m];
      const float4 q = a.queue[e];
      [[clang::always_inline]] steps = observe_back<true>(a, __float_as_int(q.x), 0, q.y, q.z);   // (as a call the function is compiled without the kernel's register budget)
    }
    if (acc != nullptr) {                         // ... and walk steps
      steps = lsd_wave_sum(steps);
      if (lane == 0) atomicAdd(&acc[1 + (ck & 63)], (unsigned long long)steps);
    }
  }
}

struct RegArgs {
  HypPlanes m;
  LSD_G const uint8_t* validIn;   // snapshot plane (read)
  LSD_G uint8_t* validOut;        // new validity plane (written for every pixel)
  LSD_G const float* kfMaxGrad;
  int w, h;
  float minUseGrad, regDistVar;
  int validityTH;
  int tileRow0;             // k_reg_fused on a range of tile rows (8 rows each): first tile row of the launch (0: whole map)
  int tileRows;             // > 0: the launch's grid may hold more tile rows than this part has (several parts per launch): the rest leave
};

// K5 for one pixel that holds no hypothesis, lies in K5's range of the image and reaches the gradient threshold
// (regularizeDepthMapFillHolesRow, DepthMap.cpp:656-703; the 5x5 sum of validity counters replaces the integral image).  NB is the pre-K5
// snapshot of the pixel's 5x5 neighbourhood: counter(dx, dy) = the validity counter of a valid neighbour (never negative), negative for
// an invalid one; valid(dx, dy); hyp(dx, dy, idepth, var) = a valid neighbour's pair.  True: a hypothesis is created with inverse depth idepthObs,
// variance VAR_RANDOM_INIT_INITIAL and validity counter 0.  The pixel's blacklisted counter is read only where the sum leaves it to decide.
template <typename NB>
__device__ __forceinline__ bool fill_hole_pixel(const NB& nb, LSD_G const int32_t* blacklistedAt, float& idepthObs) {
  int val = 0;
#pragma unroll NB::UNROLL
  for (int dy = -2; dy <= 2; dy++)
#pragma unroll NB::UNROLL
    for (int dx = -2; dx <= 2; dx++) {
      const int pk0 = nb.counter(dx, dy);
      val += pk0 > 0 ? pk0 : 0;
    }
  if (!(val > VAL_SUM_MIN_FOR_UNBLACKLIST || (val > VAL_SUM_MIN_FOR_CREATE && *blacklistedAt >= MIN_BLACKLIST))) return false;
  float sumIdepthObs = 0, sumIVarObs = 0;
#pragma unroll NB::UNROLL
  for (int dy = -2; dy <= 2; dy++)
#pragma unroll NB::UNROLL
    for (int dx = -2; dx <= 2; dx++)
      if (nb.valid(dx, dy)) {
        float id, sv;
        nb.hyp(dx, dy, id, sv);
        sumIdepthObs += id / sv;
        sumIVarObs += lsd_rcp_exact(sv);
      }
  idepthObs = unzero(sumIdepthObs / sumIVarObs);
  return true;
}
struct PlaneNeighbours {     // the neighbourhood read from the planes
  // the 5x5 loops stay loops: unrolled, the 25 validity bytes are kept in registers from the first sum to the second and k_fill_holes
  // needs 58 registers instead of 27 (profiles/r13_depth_device_phases.md)
  static constexpr int UNROLL = 1;
  const RegArgs& a;
  int idx;
  __device__ __forceinline__ int counter(int dx, int dy) const { const int j = idx + dx + dy * a.w; return a.validIn[j] ? a.m.validity[j] : -1; }
  __device__ __forceinline__ bool valid(int dx, int dy) const { return a.validIn[idx + dx + dy * a.w] != 0; }
  __device__ __forceinline__ void hyp(int dx, int dy, float& id, float& var) const { const int j = idx + dx + dy * a.w; id = a.m.idepth[j]; var = a.m.var[j]; }
};
// K5 as a launch of its own (the per-stage test hook, lsdhip_depth_stage)
__global__ __launch_bounds__(256) void k_fill_holes(RegArgs a) {
  const int x = blockIdx.x * 32 + (threadIdx.x & 31);
  const int y = blockIdx.y * 8 + (threadIdx.x >> 5);
  if (x >= a.w || y >= a.h) return;
  const int idx = x + y * a.w;
  const uint8_t wasValid = a.validIn[idx];
  uint8_t nowValid = wasValid;
  float idepthObs;
  if (x >= 3 && x < a.w - 2 && y >= 3 && y < a.h - 2 && !wasValid && !(a.kfMaxGrad[idx] < a.minUseGrad) &&
      fill_hole_pixel(PlaneNeighbours{a, idx}, a.m.blacklisted + idx, idepthObs)) {
    nowValid = 1;
    store_fresh_hypothesis(a.m, idx, idepthObs, VAR_RANDOM_INIT_INITIAL, 0);
  }
  a.validOut[idx] = nowValid;
}

// K5 + K6 (+ K8) fused over one LDS tile: regularizeDepthMapFillHoles -> regularizeDepthMap<removeOcclusions>
// (regularizeDepthMapRow, DepthMap.cpp:758-848) -> Frame::setDepth, in one launch.  A workgroup owns 32x8 pixels; K6 on them needs the
// post-K5 map on a 2-pixel halo, and K5 on that 36x12 region needs the pre-K5 snapshot on a 4-pixel halo, so the tile is 40x16 (36x12
// without K5).  The halo's K5 results are recomputed locally (identical arithmetic => identical values in every workgroup that needs
// them) and only the owner writes them to HBM.  Every neighbour access is an LDS read issued in a fully unrolled batch; the per-pixel
// arithmetic and its order are the reference's.
//
// What a launch does besides is its pass type, named for the place in DepthMap.cpp that the launch stands for:
//   FillHoles         K5 runs before K6;
//   RemoveOcclusions  regularizeDepthMap's template argument;
//   SetDepth          K8: Frame::setDepth on the owned pixels -> the keyframe's level-0 planes (id0, var0) and per-workgroup (sum, count);
//   KeyframeChange    the owner of a pixel goes on with what the reference does next with that pixel's finalised hypothesis —
//                     Frame::takeReActivationData (KfExtra::react*) and phase A of propagateDepth into the new keyframe (prop_candidate
//                     on KfExtra::prop) — while the values are in its registers;
//   SumValid          per-workgroup (sum of idepth_smoothed, count) over the valid pixels after the pass (createKeyFrame's rescale sums).
//   Propagate         with KeyframeChange: the keyframe that follows is a new one (createKeyFrame); without it a banked one comes back
//                     (setFromExistingKF) and nothing steps over;
//   FromReact         the tile is loaded from a keyframe's re-activation planes (ReactSrc) instead of the map, and the owner of a pixel
//                     stores what setFromExistingKF makes of the pixel (DepthMap.cpp:937-959) before K6's outcome.
struct PassBase { static constexpr bool FillHoles = false, RemoveOcclusions = false, SetDepth = false, KeyframeChange = false, SumValid = false,
                                        Propagate = false, FromReact = false; };
struct PassRegOnly : PassBase {};                                               // regularizeDepthMap(false, th) alone (lsdhip_depth_stage)
struct PassRegOcc : PassBase { static constexpr bool RemoveOcclusions = true; };   // regularizeDepthMap(true, th): createKeyFrame :1263
struct PassUpdate : PassBase { static constexpr bool FillHoles = true; };          // updateKeyframe :1135-1143: fill holes + regularizeDepthMap(false, th)
struct PassUpdateSetDepth : PassUpdate { static constexpr bool SetDepth = true; }; // ... + Frame::setDepth where the keyframe is due for it (:1150-1153)
struct PassKfFinalizeOnly : PassUpdateSetDepth { static constexpr bool KeyframeChange = true; };   // finalizeKeyFrame :1363-1395 (KfExtra::prop unused)
struct PassKfFinalize : PassKfFinalizeOnly { static constexpr bool Propagate = true; };        // ... then the step into createKeyFrame
struct PassFromReact : PassBase { static constexpr bool FromReact = true; };       // setFromExistingKF :937-961: the planes + regularizeDepthMap(false, th)
struct PassKfFillSums : PassUpdate { static constexpr bool SumValid = true; };     // createKeyFrame :1270-1294
struct KfExtra {
  LSD_G float* reactId;        // old keyframe's re-activation planes
  LSD_G float* reactVar;
  LSD_G uint8_t* reactVal;
  PropArgs prop;         // (src unused)
};
// one map's (or one part's) record of a pass
struct RegItem {
  RegArgs a;
  LSD_G float* id0;          // SetDepth; batched updates: null = this map's keyframe is not due for Frame::setDepth (depthHasBeenUpdatedFlag still set)
  LSD_G float* var0;
  LSD_G double* partials;    // SetDepth / SumValid: (sum, count) per workgroup
};
struct KfItem : RegItem { KfExtra x; };      // KeyframeChange
// a keyframe's re-activation planes (Frame::takeReActivationData, Frame.cpp:107-145), read-only
struct ReactSrc {
  LSD_G const float* id;
  LSD_G const float* var;      // > 0: a valid pixel's variance; -2: blacklisted; -1: neither
  LSD_G const uint8_t* val;    // a valid pixel's validity counter
};
struct ReactItem : RegItem { ReactSrc src; };      // FromReact
static_assert(sizeof(KfItem) == sizeof(RegItem) + sizeof(KfExtra), "argument records: a KfItem is a RegItem followed by its KfExtra");

// Per tile entry ONE 16-byte word (idepth, idepth_var, (float)pk) with pk = validity_counter of a valid pixel (never negative), -1 for an
// invalid one: a neighbour costs K6 one LDS round trip (round 4: two dependent ones — the validity word, then, behind the branch on
// it, the hypothesis; rounds 1-3: four arrays).  pk0 is the pre-K5 snapshot of pk that K5 reads.
typedef float reg_entry __attribute__((ext_vector_type(4)));
typedef float reg_entry3 __attribute__((ext_vector_type(3)));   // (what K6 reads of an entry: a 12-byte load leaves no dead register behind)
struct TileLds { int* pk0; uint8_t* created; reg_entry* e; };
// PY: pixels per lane = units of 8 map rows a workgroup owns (owned tile 32 x 8 PY).  The taller tile loads (32 + 2 HALO) x (8 PY + 2 HALO)
// entries for 256 PY owned pixels — 2.5x (PY = 1), 1.88x (2), 1.56x (4) with K5 — and recomputes K5 on 1.69x / 1.41x / 1.27x of them; the
// per-pixel arithmetic does not know the tile it runs in, so every shape gives the same planes bit for bit (profiles/r06_notes.md section 5).
template <bool FILL, int PY>
struct RegTile {
  static constexpr bool FILLS = FILL;
  static constexpr int HALO = FILL ? 4 : 2;
  static constexpr int OH = 8 * PY;
  static constexpr int TW = 32 + 2 * HALO, TH = OH + 2 * HALO, TN = TW * TH;
  static constexpr int FW = TW - 4, FH = TH - 4, FN = FW * FH;     // K5's region: the tile without its outer two pixels
  static constexpr int MG = FILL ? (FN + 255) / 256 : 1;           // pixels of that region per lane
  int tIdx, x0, y0, ownedRows;
  // false: the workgroup lies outside the part of the map this launch covers
  __device__ __forceinline__ bool place(const RegArgs& a) {
    // Workgroups are dealt round-robin to the 8 XCDs, each with its own L2, and every tile re-reads a 4-pixel halo of its
    // neighbours: give XCD x the contiguous tile range [x nt/8, (x+1) nt/8) (whole bands of tile rows), so that a halo line is
    // fetched into one L2 instead of into the L2s of up to four XCDs.
    const int nt = gridDim.x * gridDim.y;
    const int lin = blockIdx.x + blockIdx.y * gridDim.x;
    tIdx = (nt & 7) == 0 ? (lin & 7) * (nt >> 3) + (lin >> 3) : lin;
    // tile rows are counted in units of 8 map rows (the C ABI's unit, lsdhip_depth_stage_rows): this workgroup owns PY of them
    const int unit0 = (tIdx / (int)gridDim.x) * PY;
    if (a.tileRows > 0 && unit0 >= a.tileRows) return false;
    const int tbx = tIdx % gridDim.x;
    x0 = tbx * 32 - HALO; y0 = (unit0 + a.tileRow0) * 8 - HALO;
    ownedRows = a.tileRows > 0 ? (a.tileRows - unit0 < PY ? (a.tileRows - unit0) * 8 : OH) : OH;   // a part may end inside the tile
    return true;
  }
};
// Where a tile's entries come from: entry(g, inb, id, var, pk) issues the source's loads of pixel g together (one memory round trip for
// the tile, whichever the source) and forms pk.
struct TileFromMap {         // the map's planes and the snapshot validity plane
  const RegArgs& a;
  __device__ __forceinline__ void entry(const int g, const bool inb, float& id, float& var, int& pk) const {
    const uint8_t v = a.validIn[g];
    const int vc = a.m.validity[g];
    id = a.m.idepth[g];
    var = a.m.var[g];
    pk = (inb && v) ? vc : -1;
  }
};
struct TileFromReact {       // setFromExistingKF's reading of the re-activation planes (DepthMap.cpp:940-958): var > 0 <=> a hypothesis
  const ReactSrc& r;
  __device__ __forceinline__ void entry(const int g, const bool inb, float& id, float& var, int& pk) const {
    const int vc = r.val[g];
    id = r.id[g];
    var = r.var[g];
    pk = (inb && var > 0) ? vc : -1;
  }
};
// tile load (unconditional, clamped addresses; out-of-image entries are invalid)
template <class T, class Src>
__device__ __forceinline__ void tile_load(const RegArgs& a, const Src& src, const T& t, const TileLds& s, float (&mg)[T::MG]) {
  const int tid = threadIdx.x, w = a.w, h = a.h;
#pragma unroll
  for (int it = 0; it < (T::TN + 255) / 256; it++) {
    const int e = tid + it * 256;
    if (e < T::TN) {
      const int gx = t.x0 + e % T::TW, gy = t.y0 + e / T::TW;
      const bool inb = gx >= 0 && gx < w && gy >= 0 && gy < h;
      const int g = inb ? gx + gy * w : 0;
      float id, var;
      int pk;
      src.entry(g, inb, id, var, pk);
      s.pk0[e] = pk;
      s.created[e] = 0;
      s.e[e] = reg_entry{id, var, (float)pk, 0.f};             // (the counter as a float: K6 adds it to a float sum once per neighbour)
    }
  }
  // K5's gradient test reads the keyframe's maxGradients at the pixels of its region: issued with the tile loads (one memory round
  // trip for the workgroup instead of two; the lines are needed by nearly every wave of a semi-dense map anyway)
  if (T::FILLS) {
#pragma unroll
    for (int it = 0; it < (T::FN + 255) / 256; it++) {
      const int f = tid + it * 256;
      const int x = t.x0 + 2 + f % T::FW, y = t.y0 + 2 + f / T::FW;
      const bool inb = f < T::FN && x >= 0 && x < w && y >= 0 && y < h;
      mg[it] = a.kfMaxGrad[inb ? x + y * w : 0];
    }
  }
}
template <int TW>
struct TileNeighbours {      // K5's neighbourhood read from the tile, every read of a sum issued in one batch
  static constexpr int UNROLL = 5;
  const TileLds& s;
  int e;
  __device__ __forceinline__ int counter(int dx, int dy) const { return s.pk0[e + dx + dy * TW]; }
  __device__ __forceinline__ bool valid(int dx, int dy) const { return s.pk0[e + dx + dy * TW] >= 0; }
  __device__ __forceinline__ void hyp(int dx, int dy, float& id, float& var) const { const reg_entry iv = s.e[e + dx + dy * TW]; id = iv.x; var = iv.y; }
};
// K5 on the inner (TW-4) x (TH-4) region
template <class T>
__device__ __forceinline__ void tile_fill_holes(const RegArgs& a, const T& t, const TileLds& s, const float (&mg)[T::MG]) {
  const int tid = threadIdx.x, w = a.w, h = a.h;
#pragma unroll
  for (int it = 0; it < (T::FN + 255) / 256; it++) {
    const int f = tid + it * 256;
    if (f < T::FN) {
      const int lx = 2 + f % T::FW, ly = 2 + f / T::FW;
      const int e = lx + ly * T::TW;
      const int x = t.x0 + lx, y = t.y0 + ly;
      float idepthObs;
      if (x >= 3 && x < w - 2 && y >= 3 && y < h - 2 && s.pk0[e] < 0 && !(mg[it] < a.minUseGrad) &&
          fill_hole_pixel(TileNeighbours<T::TW>{s, e}, a.m.blacklisted + (x + y * w), idepthObs)) {
        s.created[e] = 1;
        // nobody reads these entries during K5 (their snapshot validity is 0)
        s.e[e] = reg_entry{idepthObs, VAR_RANDOM_INIT_INITIAL, 0.f, 0.f};
      }
    }
  }
}
// the six distance terms (dx^2 + dy^2) * regDistVar of the 5x5 window and the reciprocal's class mask, once, in scalar registers: as
// literals inside the loop each costs a move (+ a multiply) per neighbour in a loop of ~17 vector instructions per neighbour
struct RegDist { float df0, df1, df2, df4, df5, df8; int nmask; };
__device__ __forceinline__ RegDist reg_dist_terms(const float regDistVar) {
  auto uni = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
  return RegDist{uni(0.0f * regDistVar), uni(1.0f * regDistVar), uni(2.0f * regDistVar), uni(4.0f * regDistVar), uni(5.0f * regDistVar),
                 uni(8.0f * regDistVar), lsd_rcp_mask()};
}
struct K6Outcome {       // what K6 decides for one pixel
  bool nowValid, smoothed, blacklistDec;      // smoothed: (ids, vars) is the pixel's new smoothed pair
  float ids, vars;
};
// what the owner of a pixel stores after K5 and K6.  blFinal / return value: the pixel's blacklisted counter after the pass, where this
// lane came to know it
__device__ __forceinline__ bool store_outcome(const RegArgs& a, const int idx, const reg_entry c_e, const bool created, const K6Outcome& o, int& blFinal) {
  bool blKnown = false;
  a.validOut[idx] = o.nowValid;
  if (created) {
    blFinal = o.blacklistDec ? -1 : 0; blKnown = true;
    store_fresh_hypothesis(a.m, idx, c_e.x, c_e.y, 0, blFinal);     // (the smoothed pair's -1 gives way to the store below where K6 smoothed)
  } else if (o.blacklistDec) {
    const int b0 = a.m.blacklisted[idx];
    a.m.blacklisted[idx] = b0 - 1;
    blFinal = b0 - 1; blKnown = true;
  }
  if (o.smoothed) { a.m.idepth_s[idx] = o.ids; a.m.var_s[idx] = o.vars; }
  return blKnown;
}
// what the owner of a pixel stores in a pass loaded from re-activation planes: setFromExistingKF's pixel (DepthMap.cpp:940-958; c_e.y is
// the plane's variance entry, sign and all), then K6's outcome on it
__device__ __forceinline__ void store_react_outcome(const RegArgs& a, const int idx, const reg_entry c_e, const int c_pk, const K6Outcome& o) {
  a.validOut[idx] = o.nowValid;
  if (c_pk >= 0) {
    store_fresh_hypothesis(a.m, idx, c_e.x, c_e.y, c_pk, o.blacklistDec ? -1 : 0);
    if (o.smoothed) { a.m.idepth_s[idx] = o.ids; a.m.var_s[idx] = o.vars; }
  } else {
    a.m.blacklisted[idx] = (c_e.y == -2) ? MIN_BLACKLIST - 1 : 0;
  }
}
// Frame::takeReActivationData for one pixel (Frame.cpp:107-145): a valid pixel's hypothesis, else whether it is blacklisted
__device__ __forceinline__ void take_react_pixel(float* id, float* var, uint8_t* val, const int i, const bool valid, const float idepth, const float v,
                                                 const int validity, const int blacklisted) {
  if (valid) { id[i] = idepth; var[i] = v; val[i] = (uint8_t)validity; }
  else var[i] = blacklisted < MIN_BLACKLIST ? -2.f : -1.f;
}
// Frame::setDepth for one pixel (Frame.cpp:199-243); true: the pixel counts in the keyframe's (sum, count) of inverse depths
__device__ __forceinline__ bool set_depth_pixel(float* id0, float* var0, const int i, const bool valid, const float ids, const float vars) {
  if (valid && (double)ids >= -0.05) {
    id0[i] = ids;
    var0[i] = vars;
    return true;
  }
  id0[i] = -1.f;
  var0[i] = -1.f;
  return false;
}

template <class Pass, int PY>
__device__ __forceinline__ void reg_fused_tile(const RegItem& it, const KfExtra* __restrict__ kx = nullptr, const ReactSrc* __restrict__ rs = nullptr) {
  constexpr bool FILL = Pass::FillHoles, SUMS = Pass::SetDepth || Pass::SumValid;
  typedef RegTile<FILL, PY> T;
  __shared__ int s_pk0[T::TN];
  __shared__ uint8_t s_created[T::TN];
  __shared__ reg_entry s_e[T::TN];
  const TileLds s{s_pk0, s_created, s_e};
  const RegArgs& a = it.a;
  const int tid = threadIdx.x, w = a.w, h = a.h;
  T t;
  if (!t.place(a)) return;
  float mg[T::MG];
  if (Pass::FromReact) tile_load<T>(a, TileFromReact{*rs}, t, s, mg);
  else tile_load<T>(a, TileFromMap{a}, t, s, mg);
  __syncthreads();
  if (FILL) {
    tile_fill_holes<T>(a, t, s, mg);
    __syncthreads();
  }
  // K6 on the owned 32 x (8 PY) pixels: lane (tid & 31, tid >> 5) takes rows tid >> 5, + 8, ...
  const RegDist d = reg_dist_terms(a.regDistVar);
  double accS = 0;          // (sum, count) of this lane's pixels: createKeyFrame's rescale sums (SumValid) or Frame::setDepth's statistics (SetDepth)
  int accC = 0;
#pragma unroll
  for (int p = 0; p < PY; p++) {
    const int lx = T::HALO + (tid & 31), ly = T::HALO + (tid >> 5) + 8 * p;
    const int e = lx + ly * T::TW;
    const int x = t.x0 + lx, y = t.y0 + ly;
    const bool inImage = x < w && y < h && ly - T::HALO < t.ownedRows;
    const int idx = inImage ? x + y * w : 0;
    const bool created = FILL && s_created[e] != 0;
    const reg_entry c_e = s_e[e];
    const int c_pk = (int)c_e.z;
    const bool wasValid = c_pk >= 0;
    K6Outcome o{wasValid, false, false, 0.f, 0.f};
    // K6 for a valid pixel with its whole window inside the image (regularizeDepthMapRow, DepthMap.cpp:758-848) -> o.  The block stands
    // here and not in a function of its own: as one (outcome returned, filled in place, or five reference arguments) it cost every tile two
    // registers, profiles/r13_depth_device_phases.md.
    // (the 25-neighbour loop on compacted centres — ballots, a list in LDS, the outcome handed back to the pixel's owner — measured the
    // same as this form at 30 % and at 50 % valid pixels: profiles/r05_notes.md section 5)
    if (inImage && x >= 2 && x < w - 2 && y >= 2 && y < h - 2 && wasValid) {
      const float c_id = c_e.x;
      const float c_var = c_e.y;
      float sum = 0, val_sum = 0, sumIvar = 0;
      int numOccluding = 0, numNotOccluding = 0;
      // (the branches stay: on semi-dense maps whole waves skip most neighbours — the predicated form of this loop, every neighbour's
      // arithmetic for every valid centre, ran the 32-map pass in 214 us against 166, profiles/r05_notes.md section 5.)
      // The next neighbour's entry is requested before the current one is worked on (volatile: the read stays where it is written instead
      // of sinking below the branches to its first use), so an LDS round trip overlaps the arithmetic instead of preceding it.
      auto entry = [&](int k) { const int dx = k / 5 - 2, dy = k % 5 - 2; return *(const volatile __attribute__((address_space(3))) reg_entry3*)&s_e[e + dx + dy * T::TW]; };
      reg_entry3 ej = entry(0);
#pragma unroll
      for (int k = 0; k < 25; k++) {
        const int dx = k / 5 - 2, dy = k % 5 - 2;     // dx outer, dy inner: the reference's order of the sums
        const reg_entry3 en = entry(k < 24 ? k + 1 : 24);
        const float vcj = ej.z;                       // validity counter (small integer, exact) or -1
        const float s_idj = ej.x;
        const float s_varj = ej.y;
        ej = en;
        if (vcj < 0) continue;
        const float diff = s_idj - c_id;
        if (DIFF_FAC_SMOOTHING * diff * diff > s_varj + c_var) {
          if (Pass::RemoveOcclusions) { if (s_idj > c_id) numOccluding++; }
          continue;
        }
        val_sum += vcj;
        if (Pass::RemoveOcclusions) numNotOccluding++;
        const int d2 = dx * dx + dy * dy;             // (float)(d2) * regDistVar, as the reference forms it
        const float distFac = d2 == 0 ? d.df0 : (d2 == 1 ? d.df1 : (d2 == 2 ? d.df2 : (d2 == 4 ? d.df4 : (d2 == 5 ? d.df5 : d.df8))));
        const float ivar = lsd_rcp_exact(s_varj + distFac, d.nmask);
        sum += s_idj * ivar;
        sumIvar += ivar;
      }
      if (val_sum < a.validityTH) {
        o.nowValid = false;
        o.blacklistDec = true;
      } else if (Pass::RemoveOcclusions && numOccluding > numNotOccluding) {
        o.nowValid = false;
      } else {
        sum = sum / sumIvar;
        o.ids = unzero(sum);
        o.vars = lsd_rcp_exact(sumIvar);
        o.smoothed = true;
      }
    }
    if (!inImage) continue;
    int blFinal = 0;
    bool blKnown = false;
    if (Pass::FromReact) store_react_outcome(a, idx, c_e, c_pk, o);
    else blKnown = store_outcome(a, idx, c_e, created, o, blFinal);
    // the pixel's smoothed pair after the pass
    float ids = -1.f, vars = -1.f;
    if (SUMS || Pass::KeyframeChange) {
      if (o.smoothed) { ids = o.ids; vars = o.vars; }
      else if (created || !o.nowValid) { ids = -1.f; vars = -1.f; }    // (not valid: the value is not looked at)
      else { ids = a.m.idepth_s[idx]; vars = a.m.var_s[idx]; }         // valid, not smoothed: the 2-pixel border only
    }
    // createKeyFrame's rescale sums (DepthMap.cpp:1286-1294): idepth_smoothed over the valid pixels
    if (Pass::SumValid && o.nowValid) { accS += ids; accC += 1; }
    // K8
    if (Pass::SetDepth && set_depth_pixel(it.id0, it.var0, idx, o.nowValid, ids, vars)) { accS += ids; accC += 1; }
    if (Pass::KeyframeChange) {
      // the keyframe being finalised hands the pixel to its re-activation planes, then the hypothesis steps into the new keyframe
      if (o.nowValid) {
        take_react_pixel(kx->reactId, kx->reactVar, kx->reactVal, idx, true, c_e.x, c_e.y, c_pk, 0);
        if (Pass::Propagate) prop_candidate(kx->prop, x, y, idx, ids, c_e.y, c_pk);
      } else {
        take_react_pixel(kx->reactId, kx->reactVar, kx->reactVal, idx, false, 0.f, 0.f, 0, blKnown ? blFinal : a.m.blacklisted[idx]);
      }
    }
  }
  if (SUMS) {
    // The sum of at most 256 PY floats of one sign and a dynamic range below 2^20 is exact in double, so its value does not depend on
    // the order: the butterfly order serves.
    lsd_block_butterfly_sum(accS, accC);
    if (tid == 0) { it.partials[2 * t.tIdx] = accS; it.partials[2 * t.tIdx + 1] = (double)accC; }
  }
}
template <class Pass, int PY>
__global__ __launch_bounds__(256) void k_reg_fused(RegItem it) {
  reg_fused_tile<Pass, PY>(it);
}
// the update-time pass (PassUpdate or PassUpdateSetDepth) over the maps of several sequences, blockIdx.z = map: each launch takes the maps
// whose keyframe is / is not due for Frame::setDepth
template <class Pass, int PY>
__global__ __launch_bounds__(256) void k_reg_fused_batch(const RegItem* __restrict__ items) {
  const RegItem& it = items[blockIdx.z];
  if ((it.id0 != nullptr) != Pass::SetDepth) return;
  reg_fused_tile<Pass, PY>(it);
}

// ---- keyframe change of n maps in shared launches (lsdhip_depth_change_keyframe_batch), blockIdx.z = map -------------------------------
//   k_kf_finalize_prop        PassKfFinalize: finalizeKeyFrame's pass (fill holes + regularise + Frame::setDepth of the old keyframe) +
//                             takeReActivationData + phase A of propagateDepth, per owner pixel
//   k_prop_resolve_batch      phase B into the new map
//   k_kf_reg<PassRegOcc>      regularizeDepthMap(true, ...)        (createKeyFrame, DepthMap.cpp:1271)
//   k_kf_reg<PassKfFillSums>  fill holes + regularizeDepthMap(false, ...) + the rescale sums per tile   (:1278-1294)
//   k_kf_rescale_setdepth     mean inverse depth to one (:1296-1304) + Frame::setDepth of the new keyframe
//   k_idepth_pyramid_batch    both keyframes' pyramids and their (sum, count) records
template <int PY>
__global__ __launch_bounds__(256) void k_kf_finalize_prop(const KfItem* __restrict__ items) {
  const KfItem& it = items[blockIdx.z];
  reg_fused_tile<PassKfFinalize, PY>(it, &it.x);
}
template <class Pass, int PY>
__global__ __launch_bounds__(256) void k_kf_reg(const RegItem* __restrict__ items) {
  reg_fused_tile<Pass, PY>(items[blockIdx.z]);
}
// ---- re-activation of n maps' banked keyframes in shared launches (lsdhip_depth_reactivate_keyframe_batch), blockIdx.z = map -------------
//   k_kf_finalize             PassKfFinalizeOnly: finalizeKeyFrame's pass + takeReActivationData per owner pixel; nothing propagates
//   k_kf_from_react           PassFromReact: setFromExistingKF's planes and its regularizeDepthMap(false, ...) in one pass: every read comes
//                             from the old keyframe's re-activation planes, every write goes to the map, so the pass needs neither the
//                             snapshot of the validity plane nor a conversion launch in front of it
//   k_idepth_pyramid_batch    the finalised keyframe's pyramid and its (sum, count) record
template <int PY>
__global__ __launch_bounds__(256) void k_kf_finalize(const KfItem* __restrict__ items) {
  const KfItem& it = items[blockIdx.z];
  reg_fused_tile<PassKfFinalizeOnly, PY>(it, &it.x);
}
template <int PY>
__global__ __launch_bounds__(256) void k_kf_from_react(const ReactItem* __restrict__ items) {
  const ReactItem& it = items[blockIdx.z];
  reg_fused_tile<PassFromReact, PY>(it, nullptr, &it.src);
}
struct RescaleItem {
  HypPlanes m;
  LSD_G const double* sumPartials;   // per-tile (sum, count) of the pass before
  int nSumPartials;
  LSD_G int* flags;                  // propagation flags: [0] -> slot, then both zeroed
  LSD_G double* slot;                // pinned DeferredSlot of the rescale factor: (sum, count, flag)
  LSD_G float* id0;                  // new keyframe's level-0 planes
  LSD_G float* var0;
  LSD_G double* statPartials;        // (sum, count) per workgroup of this launch
  int n;
};
// Tile height of a regulariser launch: workgroups that own 32 x 16 pixels (PY = 2) move a quarter less through LDS per owned pixel and
// recompute a sixth less of K5 than 32 x 8 ones — where the launch has enough of them to fill the chip (several maps, large frames:
// -19 % for the 32-map pass, -6 % at 3840x2160); one 640x480 map is 1200 short workgroups or 600 long ones on 256 CUs, and the short ones
// win there (keyframe change 0.085 against 0.097 ms).  32 x 32 (PY = 4, 33.6 KB of LDS) lost everywhere.  profiles/r06_notes.md section 5.
// (The tests that are there for the PY = 2 arms of single-map and row-part launches take the smallest shapes that reach this threshold —
// 1024x512: tests/test_gpu_parity.py, tests/test_bands_gpu.py — and assert 2048 workgroups themselves: they move with it.)
static inline int lsd_reg_py(long long workgroups_at_py1) { return workgroups_at_py1 >= 2048 ? 2 : 1; }
// grid rows of a regulariser launch over `units` tile rows of 8 map rows each
static inline int lsd_reg_grid_rows(int units, int py) { return (units + py - 1) / py; }
#define LSD_REG_DISPATCH(py, ...) do { if ((py) == 2) { constexpr int PYV = 2; __VA_ARGS__; } else { constexpr int PYV = 1; __VA_ARGS__; } } while (0)
#define LSD_RESCALE_PX 2048    // pixels per workgroup of k_kf_rescale_setdepth
// createKeyFrame's rescale (DepthMap.cpp:1286-1304): the factor numIdepth / sumIdepth with both cast to float first, and a valid pixel's
// four fields under it; (ids, vars) = the rescaled smoothed pair
__device__ __forceinline__ float rescale_factor(const double sumIdepth, const double numIdepth) { return (float)numIdepth / (float)sumIdepth; }
__device__ __forceinline__ void rescale_pixel(const HypPlanes& m, const int i, const float rescaleFactor, float& ids, float& vars) {
  const float rescaleFactor2 = rescaleFactor * rescaleFactor;
  m.idepth[i] *= rescaleFactor;
  ids = m.idepth_s[i] * rescaleFactor;
  m.idepth_s[i] = ids;
  m.var[i] *= rescaleFactor2;
  vars = m.var_s[i] * rescaleFactor2;
  m.var_s[i] = vars;
}
__global__ __launch_bounds__(256) void k_kf_rescale_setdepth(const RescaleItem* __restrict__ items) {
  const RescaleItem& it = items[blockIdx.y];
  const int tid = threadIdx.x;
  // every workgroup adds the tiles' partials in the same fixed order: the same factor everywhere, no second launch, no atomics
  double sumD = 0, cntD = 0;
  for (int i = tid; i < it.nSumPartials; i += 256) { sumD += it.sumPartials[2 * i]; cntD += it.sumPartials[2 * i + 1]; }
  lsd_block_tree_sum(sumD, cntD);
  __syncthreads();
  if (blockIdx.x == 0 && tid == 0) {
    it.slot[0] = sumD; it.slot[1] = cntD; it.slot[2] = (double)it.flags[0];
    it.flags[0] = 0; it.flags[1] = 0;
  }
  const float rescaleFactor = rescale_factor(sumD, cntD);
  double s = 0, c = 0;
#pragma unroll
  for (int k = 0; k < LSD_RESCALE_PX / 256; k++) {
    const int i = blockIdx.x * LSD_RESCALE_PX + k * 256 + tid;
    if (i < it.n) {
      float ids = -1.f, vars = -1.f;
      const bool valid = it.m.valid[i] != 0;
      if (valid) rescale_pixel(it.m, i, rescaleFactor, ids, vars);
      if (set_depth_pixel(it.id0, it.var0, i, valid, ids, vars)) { s += ids; c += 1; }
    }
  }
  lsd_block_tree_sum(s, c);
  if (tid == 0) { it.statPartials[2 * blockIdx.x] = s; it.statPartials[2 * blockIdx.x + 1] = c; }
}

// parts of the fused fill-holes + regularise pass of several maps in one launch (row-band decomposition: the windows of one process),
// blockIdx.z = part
template <int PY>
__global__ __launch_bounds__(256) void k_reg_rows_batch(const RegItem* __restrict__ items) {
  reg_fused_tile<PassUpdate, PY>(items[blockIdx.z]);
}

// K8: Frame::setDepth + per-workgroup (sum, count) partials for meanIdepth / numPoints
__global__ __launch_bounds__(256) void k_set_depth(HypPlanes m, float* __restrict__ id0, float* __restrict__ var0, int n, double* __restrict__ partials) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  double s = 0;
  int c = 0;
  if (i < n) {
    const float ids = m.idepth_s[i];
    if (set_depth_pixel(id0, var0, i, m.valid[i] != 0, ids, m.var_s[i])) { s = ids; c = 1; }
  }
  lsd_block_tree_sum(s, c);
  if (threadIdx.x == 0) { partials[2 * blockIdx.x] = s; partials[2 * blockIdx.x + 1] = (double)c; }
}
// sum of idepth_smoothed over valid pixels (createKeyFrame rescale, DepthMap.cpp:1286-1294)
__global__ __launch_bounds__(256) void k_sum_valid_idepth(HypPlanes m, int n, double* __restrict__ partials) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  double s = 0;
  int c = 0;
  if (i < n && m.valid[i]) { s = m.idepth_s[i]; c = 1; }
  lsd_block_tree_sum(s, c);
  if (threadIdx.x == 0) { partials[2 * blockIdx.x] = s; partials[2 * blockIdx.x + 1] = (double)c; }
}
// out = pinned DeferredSlot (sum, count, flag); dev_out = the same pair in HBM for a kernel that follows (k_rescale)
__global__ __launch_bounds__(256) void k_reduce_pairs(const double* __restrict__ partials, int nblocks, double* __restrict__ out,
                                                       double* __restrict__ dev_out, const int* __restrict__ flag) {
  double a = 0, b = 0;
  for (int i = threadIdx.x; i < nblocks; i += 256) { a += partials[2 * i]; b += partials[2 * i + 1]; }
  lsd_block_tree_sum(a, b);
  if (threadIdx.x == 0) {
    out[0] = a; out[1] = b; out[2] = flag ? (double)flag[0] : 0.0;
    if (dev_out) { dev_out[0] = a; dev_out[1] = b; }
  }
}
__global__ __launch_bounds__(256) void k_rescale(HypPlanes m, int n, const double* __restrict__ sumCount) {
  const float rescaleFactor = rescale_factor(sumCount[0], sumCount[1]);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n || !m.valid[i]) return;
  float ids, vars;
  rescale_pixel(m, i, rescaleFactor, ids, vars);
}

// phase A: every valid source hypothesis computes its target pixel and candidate, and registers in the target's slot list
__global__ __launch_bounds__(256) void k_prop_candidates(PropArgs a) {
  const int x = blockIdx.x * 32 + (threadIdx.x & 31);
  const int y = blockIdx.y * 8 + (threadIdx.x >> 5);
  if (x >= a.w || y >= a.h) return;
  const int idx = x + y * a.w;
  if (!a.src.valid[idx]) return;
  prop_candidate(a, x, y, idx, a.src.idepth_s[idx], a.src.var[idx], a.src.validity[idx]);
}
// one step of the reference's per-target merge (DepthMap.cpp:587-640), sources replayed in the order its double loop visits them
__device__ __forceinline__ void prop_merge(const float4 c, bool& tValid, float& t_idepth, float& t_var, int& t_validity) {
  float new_idepth = c.x, new_var = c.y;
  int src_validity = __float_as_int(c.z);
  if (tValid) {
    float diff = t_idepth - new_idepth;
    if (DIFF_FAC_PROP_MERGE * diff * diff > new_var + t_var) {
      if (new_idepth < t_idepth) return;
      else tValid = false;
    }
  }
  if (!tValid) {
    tValid = true;
    t_idepth = new_idepth; t_var = new_var; t_validity = src_validity;
  } else {
    float w = new_var / (t_var + new_var);
    float merged_new_idepth = w * t_idepth + (1.0f - w) * new_idepth;
    int merged_validity = src_validity + t_validity;
    if (merged_validity > VALIDITY_COUNTER_MAX + (VALIDITY_COUNTER_MAX_VARIABLE))
      merged_validity = VALIDITY_COUNTER_MAX + (VALIDITY_COUNTER_MAX_VARIABLE);
    float mv = 1.0f / (1.0f / t_var + 1.0f / new_var);
    t_idepth = merged_new_idepth; t_var = mv; t_validity = merged_validity;
  }
}
// phase B: per target, replay its candidates in source order (row-major, as the reference's double loop visits them)
__device__ __forceinline__ void prop_resolve_pixel(const PropArgs& a, const int i) {
  const int cnt = a.slotCount[i];
  int n = cnt;
  if (n > PROP_SLOT_CAP) n = PROP_SLOT_CAP;
  int srcs[PROP_SLOT_CAP];
  for (int k = 0; k < PROP_SLOT_CAP; k++) srcs[k] = (k < n) ? a.slots[(size_t)i * PROP_SLOT_CAP + k] : 0x7fffffff;
  for (int p = 1; p < PROP_SLOT_CAP; p++) {  // insertion sort, ascending source index
    int key = srcs[p];
    int q = p - 1;
    while (q >= 0 && srcs[q] > key) { srcs[q + 1] = srcs[q]; q--; }
    srcs[q + 1] = key;
  }
  bool tValid = false;
  float t_idepth = 0, t_var = 0;
  int t_validity = 0;
  if (cnt <= PROP_SLOT_CAP) {
    for (int k = 0; k < n; k++) prop_merge(a.cand[srcs[k]], tValid, t_idepth, t_var, t_validity);
  } else {
    // rare: slots + chain, replayed in ascending source order by repeated selection (no per-thread list needed)
    int last = -1;
    while (true) {
      int best = 0x7fffffff;
      for (int k = 0; k < PROP_SLOT_CAP; k++) if (srcs[k] > last && srcs[k] < best) best = srcs[k];
      for (int o = a.ovfHead[i]; o >= 0;) {
        const int2 e = a.ovf[o];
        if (e.x > last && e.x < best) best = e.x;
        o = e.y;
      }
      if (best == 0x7fffffff) break;
      prop_merge(a.cand[best], tValid, t_idepth, t_var, t_validity);
      last = best;
    }
  }
  a.dst.valid[i] = tValid ? 1 : 0;
  if (tValid) store_fresh_hypothesis(a.dst, i, t_idepth, t_var, t_validity);
  else a.dst.blacklisted[i] = 0;
  // clean at rest: the next propagation into this scratch starts without clears
  if (cnt != 0) a.slotCount[i] = 0;
  if (cnt > PROP_SLOT_CAP) a.ovfHead[i] = -1;      // (a chain exists only where the slots overflowed)
}
__global__ __launch_bounds__(256) void k_prop_resolve(PropArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.w * a.h) return;
  prop_resolve_pixel(a, i);
}
__global__ __launch_bounds__(256) void k_prop_resolve_batch(const KfItem* __restrict__ items) {
  const PropArgs& a = items[blockIdx.y].x.prop;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.w * a.h) return;
  prop_resolve_pixel(a, i);
}

// ---- initialisation / re-activation kernels ------------------------------------------------------------------------
// initializeFromGTDepth (DepthMap.cpp:979-1014)
__global__ __launch_bounds__(256) void k_init_gt(HypPlanes m, const float* __restrict__ idepth0, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float v = idepth0[i];
  if (!isnan(v) && v > 0) {
    m.valid[i] = 1; m.blacklisted[i] = 0; m.nextID[i] = 0; m.validity[i] = 20;
    m.idepth[i] = v; m.idepth_s[i] = v; m.var[i] = VAR_GT_INIT_INITIAL; m.var_s[i] = VAR_GT_INIT_INITIAL;
  } else {
    m.valid[i] = 0; m.blacklisted[i] = 0;
  }
}
// Frame::takeReActivationData (Frame.cpp:107-145)
__global__ __launch_bounds__(256) void k_take_react(HypPlanes m, float* __restrict__ id, float* __restrict__ var, uint8_t* __restrict__ val, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const bool valid = m.valid[i] != 0;
  take_react_pixel(id, var, val, i, valid, valid ? m.idepth[i] : 0.f, valid ? m.var[i] : 0.f, valid ? m.validity[i] : 0, valid ? 0 : m.blacklisted[i]);
}
// setFromExistingKF (DepthMap.cpp:937-959)
__global__ __launch_bounds__(256) void k_from_react(HypPlanes m, const float* __restrict__ id, const float* __restrict__ var, const uint8_t* __restrict__ val, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float v = var[i];
  if (v > 0) {
    m.valid[i] = 1;
    store_fresh_hypothesis(m, i, id[i], v, val[i]);
  } else {
    m.valid[i] = 0;
    m.blacklisted[i] = (v == -2) ? MIN_BLACKLIST - 1 : 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------
static size_t up256(size_t v) { return (v + 255) / 256 * 256; }
// 256-thread workgroups of a launch with one thread per level-0 pixel
static unsigned px_blocks(const lsdhip_ctx* c) { return (unsigned)(((size_t)c->w * c->h + 255) / 256); }
// The launch shape of a regulariser pass over `units` tile rows (8 map rows each) of nMaps maps, one map per grid z.  The tile height is
// chosen for unitsInAll tile rows (lsd_reg_py); where the maps bring different row counts it is their sum, otherwise units x nMaps.
struct RegGrid {
  int tx, units, py;
  dim3 grid;
  int tiles() const { return (int)(grid.x * grid.y); }   // per map: one (sum, count) partial each
};
static int tile_rows(const lsdhip_ctx* c) { return (c->h + 7) / 8; }
static RegGrid reg_grid(const lsdhip_ctx* c, int units, int nMaps, long long unitsInAll = 0) {
  const int tx = (c->w + 31) / 32, py = lsd_reg_py((long long)tx * (unitsInAll ? unitsInAll : (long long)units * nMaps));
  return RegGrid{tx, units, py, dim3(tx, lsd_reg_grid_rows(units, py), nMaps)};
}
// every mapping call ends here: the record point of a pipelined context, and unless the context is asynchronous the call's work is done
static int map_call_end(lsdhip_ctx* c) {
  if (lsd_m_record(c) < 0) return LSDHIP_E_HIP;
  if (!c->async) HIPCHK(hipStreamSynchronize(lsd_map_stream(c)));   // asynchronous contexts: ordered on the stream, see lsdhip_ctx_synchronize
  return LSDHIP_OK;
}

static int alloc_planes(HypPlanes& p, size_t n, LsdDev<char>& arena) {
  if (int rc = lsd_dev_alloc_zeroed(arena, n * 29 + 8 * 256)) return rc;
  char* base = arena;
  size_t off = 0;
  p.blacklisted = lsd_g((int32_t*)(base + off)); off = up256(off + n * 4);
  p.nextID = lsd_g((float*)(base + off)); off = up256(off + n * 4);
  p.validity = lsd_g((int32_t*)(base + off)); off = up256(off + n * 4);
  p.idepth = lsd_g((float*)(base + off)); off = up256(off + n * 4);
  p.var = lsd_g((float*)(base + off)); off = up256(off + n * 4);
  p.idepth_s = lsd_g((float*)(base + off)); off = up256(off + n * 4);
  p.var_s = lsd_g((float*)(base + off)); off = up256(off + n * 4);
  p.valid = lsd_g((uint8_t*)(base + off));
  return LSDHIP_OK;
}

static int depth_create_impl(lsdhip_ctx* c, lsdhip_depthmap* dm) {
  size_t n = (size_t)c->w * c->h;
  if (int rc = alloc_planes(dm->cur, n, dm->arenas[0])) return rc;
  if (int rc = alloc_planes(dm->oth, n, dm->arenas[1])) return rc;
  if (int rc = lsd_dev_alloc_zeroed(dm->arenas[2], n)) return rc;
  dm->d_validSnap = (uint8_t*)dm->arenas[2].get();
  if (int rc = lsd_dev_alloc(dm->d_slotCount, n)) return rc;
  if (int rc = lsd_dev_alloc(dm->d_slots, n * PROP_SLOT_CAP)) return rc;
  if (int rc = lsd_dev_alloc(dm->d_ovfHead, n)) return rc;
  if (int rc = lsd_dev_alloc(dm->d_ovf, n)) return rc;
  if (int rc = lsd_dev_alloc(dm->d_cand, n)) return rc;
  if (int rc = lsd_dev_alloc(dm->d_flags, 16)) return rc;
  HIPCHK(hipMemsetAsync(dm->d_flags, 0, 64, lsd_map_stream(c)));
  const int nb = (int)px_blocks(c);
  const int ntiles = ((c->w + 31) / 32) * tile_rows(c);   // partials of the fused regulariser: one pair per 32x8 tile
  // (sum, count) partials: [16, ...) the setDepth / rescale passes of the single calls; the keyframe change in shared launches keeps
  // three sets alive at once (old keyframe's setDepth | rescale sums | new keyframe's setDepth)
  dm->redStride = (size_t)2 * (nb > ntiles ? nb : ntiles);
  if (int rc = lsd_dev_alloc(dm->d_red, 3 * dm->redStride + 16)) return rc;
  // K7 scratch is clean at rest (k_prop_resolve / the reader of the flags leave it so)
  HIPCHK(hipMemsetAsync(dm->d_slotCount, 0, n * 4, lsd_map_stream(c)));
  HIPCHK(hipMemsetAsync(dm->d_ovfHead, 0xFF, n * 4, lsd_map_stream(c)));
  dm->propClean = true;
  return lsd_pinned_alloc(dm->h_red, 16, hipHostMallocMapped);
}
extern "C" int lsdhip_depth_create(lsdhip_ctx* c, lsdhip_depthmap** out) {
  if (!c || !out) return LSDHIP_E_ARG;
  HIPCHK(hipSetDevice(c->device));
  LSD_CTX_LOCK(c);
  std::unique_ptr<lsdhip_depthmap> dm(new lsdhip_depthmap());
  dm->ctx = c;
  if (int rc = depth_create_impl(c, dm.get())) return rc;
  c->depthmaps.push_back(dm.get());
  *out = dm.release();
  return LSDHIP_OK;
}
// a frame is going away: no depth map may keep it as its active keyframe (a later frame can get the same heap address)
void lsd_depthmaps_forget_frame(lsdhip_ctx* c, lsdhip_frame* f) {
  for (lsdhip_depthmap* dm : c->depthmaps)
    if (dm->activeKeyFrame == f) { dm->activeKeyFrame = nullptr; dm->activeKeyFrameIsReactivated = false; }
}
extern "C" void lsdhip_depth_destroy(lsdhip_depthmap* dm) {
  if (!dm) return;
  {
    LSD_CTX_LOCK(dm->ctx);
    auto& v = dm->ctx->depthmaps;
    for (size_t i = 0; i < v.size(); i++) if (v[i] == dm) { v.erase(v.begin() + i); break; }
  }
  (void)hipSetDevice(dm->ctx->device);
  (void)hipStreamSynchronize(lsd_map_stream(dm->ctx));
#ifdef LSD_PHASE_TRACE
  if (const char* path = getenv("LSDHIP_OBS_TRACE_FILE")) {
    if (dm->d_obs_trace) {
      std::vector<unsigned long long> h(dm->obs_trace_words);
      if (hipMemcpy(h.data(), dm->d_obs_trace, h.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
        if (FILE* f = fopen(path, "w")) {
          for (size_t i = 0; i + 16 <= h.size(); i += 16) { for (int k = 0; k < 16; k++) fprintf(f, "%llu ", h[i + k]); fprintf(f, "\n"); }
          fclose(f);
        }
      }
    }
  }
#endif
  delete dm;
}
extern "C" int lsdhip_depth_is_valid(lsdhip_depthmap* dm) { return dm && dm->activeKeyFrame != nullptr; }
extern "C" int lsdhip_depth_invalidate(lsdhip_depthmap* dm) { if (!dm) return LSDHIP_E_ARG; dm->activeKeyFrame = nullptr; return LSDHIP_OK; }
extern "C" int lsdhip_depth_reset(lsdhip_depthmap* dm) {
  if (!dm) return LSDHIP_E_ARG;
  size_t n = (size_t)dm->ctx->w * dm->ctx->h;
  HIPCHK(hipMemsetAsync(dm->cur.valid, 0, n, lsd_map_stream(dm->ctx)));
  HIPCHK(hipMemsetAsync(dm->oth.valid, 0, n, lsd_map_stream(dm->ctx)));
  return LSDHIP_OK;
}

static int set_depth_finish(lsdhip_depthmap* dm, int nPartials);
// Frame::setDepth on the active keyframe: level-0 planes, idepth pyramid, meanIdepth / numPoints
static int set_depth(lsdhip_depthmap* dm) {
  lsdhip_ctx* c = dm->ctx;
  LSD_CTX_LOCK(c);
  lsdhip_frame* kf = dm->activeKeyFrame;
  const int nb = (int)px_blocks(c);
  hipLaunchKernelGGL(k_set_depth, dim3(nb), dim3(256), 0, lsd_map_stream(c), dm->cur, lsd_depth_w(kf)[0], lsd_depthvar_w(kf)[0], c->w * c->h, dm->d_red + 16);
  return set_depth_finish(dm, nb);
}
// second half of Frame::setDepth: mean inverse depth / point count from the (sum, count) partials, idepth pyramid
static int set_depth_finish(lsdhip_depthmap* dm, int nPartials) {
  lsdhip_ctx* c = dm->ctx;
  LSD_CTX_LOCK(c);
  lsdhip_frame* kf = dm->activeKeyFrame;
  const int slot = lsd_ctx_claim_stats_slot(c, kf);
  if (slot < 0) return slot;
  // the (sum, count) reduction rides on the pyramid launch (one extra workgroup): both depend only on the level-0 planes
  int rc = lsd_frame_build_idepth_pyramid(kf, dm->d_red + 16, nPartials, (double*)&c->h_slots[slot]);
  if (rc) return rc;
  kf->depthHasBeenUpdatedFlag = true;
  if (!c->async) return lsd_frame_resolve(kf);
  return LSDHIP_OK;
}

static RegArgs reg_args(lsdhip_depthmap* dm, int validityTH) {
  lsdhip_ctx* c = dm->ctx;
  LSD_CTX_LOCK(c);
  RegArgs a;
  a.m = dm->cur;
  a.validIn = dm->cur.valid;
  a.validOut = lsd_g(dm->d_validSnap);
  a.kfMaxGrad = lsd_g(dm->activeKeyFrame->d_maxgrad);
  a.w = c->w; a.h = c->h;
  a.minUseGrad = c->params.minUseGrad;
  a.regDistVar = 0.075f * 0.075f * c->params.depthSmoothingFactor * c->params.depthSmoothingFactor;  // REG_DIST_VAR
  a.validityTH = validityTH;
  a.tileRow0 = 0;
  a.tileRows = 0;
  return a;
}
static void swap_valid(lsdhip_depthmap* dm) { uint8_t* v = (uint8_t*)dm->cur.valid; dm->cur.valid = lsd_g(dm->d_validSnap); dm->d_validSnap = v; }
// One map's record of a batched regulariser pass on the planes as they stand (it reads cur.valid and writes the spare plane: the caller
// swaps them, as fill_regularize does).  setDepthOf: the keyframe whose level-0 planes the pass also writes (Frame::setDepth), or null.
static RegItem reg_item(lsdhip_depthmap* dm, lsdhip_frame* setDepthOf, double* partials) {
  RegItem r;
  memset((void*)&r, 0, sizeof(r));
  r.a = reg_args(dm, VAL_SUM_MIN_FOR_KEEP);
  r.id0 = lsd_g(setDepthOf ? lsd_depth_w(setDepthOf)[0] : nullptr);
  r.var0 = lsd_g(setDepthOf ? lsd_depthvar_w(setDepthOf)[0] : nullptr);
  r.partials = lsd_g(partials);
  return r;
}

static int fill_holes(lsdhip_depthmap* dm) {
  lsdhip_ctx* c = dm->ctx;
  LSD_CTX_LOCK(c);
  RegArgs a = reg_args(dm, 0);
  hipLaunchKernelGGL(k_fill_holes, dim3((c->w + 31) / 32, tile_rows(c)), dim3(256), 0, lsd_map_stream(c), a);
  HIPCHK(hipGetLastError());
  swap_valid(dm);
  return LSDHIP_OK;
}
static int regularize(lsdhip_depthmap* dm, bool removeOcclusions, int validityTH) {
  lsdhip_ctx* c = dm->ctx;
  LSD_CTX_LOCK(c);
  RegArgs a = reg_args(dm, validityTH);
  const RegGrid g = reg_grid(c, tile_rows(c), 1);
  LSD_REG_DISPATCH(g.py,
    if (removeOcclusions) hipLaunchKernelGGL((k_reg_fused<PassRegOcc, PYV>), g.grid, dim3(256), 0, lsd_map_stream(c), RegItem{a, nullptr, nullptr, nullptr});
    else hipLaunchKernelGGL((k_reg_fused<PassRegOnly, PYV>), g.grid, dim3(256), 0, lsd_map_stream(c), RegItem{a, nullptr, nullptr, nullptr}));
  HIPCHK(hipGetLastError());
  swap_valid(dm);
  return LSDHIP_OK;
}
// regularizeDepthMapFillHoles + regularizeDepthMap(false, validityTH) [+ Frame::setDepth] in one launch
static int fill_regularize(lsdhip_depthmap* dm, int validityTH, bool setDepth) {
  lsdhip_ctx* c = dm->ctx;
  LSD_CTX_LOCK(c);
  lsdhip_frame* kf = dm->activeKeyFrame;
  RegArgs a = reg_args(dm, validityTH);
  const RegGrid g = reg_grid(c, tile_rows(c), 1);
  LSD_REG_DISPATCH(g.py,
    if (setDepth)
      hipLaunchKernelGGL((k_reg_fused<PassUpdateSetDepth, PYV>), g.grid, dim3(256), 0, lsd_map_stream(c),
                         RegItem{a, lsd_g(lsd_depth_w(kf)[0]), lsd_g(lsd_depthvar_w(kf)[0]), lsd_g(dm->d_red + 16)});
    else
      hipLaunchKernelGGL((k_reg_fused<PassUpdate, PYV>), g.grid, dim3(256), 0, lsd_map_stream(c), RegItem{a, nullptr, nullptr, nullptr}));
  HIPCHK(hipGetLastError());
  swap_valid(dm);
  if (setDepth) return set_depth_finish(dm, g.tiles());
  return LSDHIP_OK;
}

// The fused pass on tile rows [tileRow0, tileRow0 + nTileRows) only (a tile row = 8 map rows).  The parts of one pass may be issued
// in any order and on different streams: every part reads the snapshot validity plane and the pre-pass hypotheses (a pixel K5 creates
// was invalid in the snapshot, so nobody reads the fields its owner rewrites) and writes the other validity plane; `last` swaps the
// two once all parts are queued.  Rows outside the parts keep whatever the second validity plane held: the caller refreshes them
// (row-band decomposition: rows another band owns arrive with the halo exchange).
// a part of a pass names tile rows of the map; minRows = 0 where an empty part is allowed
static int check_tile_rows(const lsdhip_ctx* c, int tileRow0, int nTileRows, int minRows) {
  const int T = tile_rows(c);
  if (tileRow0 >= 0 && nTileRows >= minRows && tileRow0 + nTileRows <= T) return LSDHIP_OK;
  lsd_set_error("depth stage rows: tile rows [%d, %d) outside [0, %d)", tileRow0, tileRow0 + nTileRows, T);
  return LSDHIP_E_ARG;
}
static int fill_regularize_rows(lsdhip_depthmap* dm, int validityTH, int tileRow0, int nTileRows, bool last) {
  lsdhip_ctx* c = dm->ctx;
  LSD_CTX_LOCK(c);
  if (int rcr = check_tile_rows(c, tileRow0, nTileRows, 0)) return rcr;
  if (nTileRows > 0) {
    RegArgs a = reg_args(dm, validityTH);
    a.tileRow0 = tileRow0;
    a.tileRows = nTileRows;
    const RegGrid g = reg_grid(c, nTileRows, 1);
    LSD_REG_DISPATCH(g.py, hipLaunchKernelGGL((k_reg_fused<PassUpdate, PYV>), g.grid, dim3(256), 0, lsd_map_stream(c), RegItem{a, nullptr, nullptr, nullptr}));
    HIPCHK(hipGetLastError());
  }
  if (last) swap_valid(dm);
  return LSDHIP_OK;
}

// Frame::prepareForStereoWith (Frame.cpp:295-317): Sim3 algebra in double, results cast to float
static void prepare_stereo(lsdhip_depthmap* dm, lsdhip_frame* fr, StereoRef& s) {
  lsdhip_ctx* c = dm->ctx;
  LSD_CTX_LOCK(c);
  const lsdm::Sim3dH& thisToOther = fr->thisToParent_raw;
  lsdm::Sim3dH otherToThis = lsdm::sim3_inverse(thisToOther);
  double Rd[9];
  lsdm::quatd_to_rot(otherToThis.q, Rd);
  float Rf[9];
  for (int i = 0; i < 9; i++) Rf[i] = (float)Rd[i];
  const float* K = c->K0;
  float sc = (float)otherToThis.s;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      float acc = K[i * 3 + 0] * Rf[0 * 3 + j];
      acc += K[i * 3 + 1] * Rf[1 * 3 + j];
      acc += K[i * 3 + 2] * Rf[2 * 3 + j];
      s.K_otherToThis_R[i * 3 + j] = acc * sc;
    }
  for (int i = 0; i < 3; i++) s.otherToThis_t[i] = (float)otherToThis.t[i];
  for (int i = 0; i < 3; i++) {
    float acc = K[i * 3 + 0] * s.otherToThis_t[0];
    acc += K[i * 3 + 1] * s.otherToThis_t[1];
    acc += K[i * 3 + 2] * s.otherToThis_t[2];
    s.K_otherToThis_t[i] = acc;
  }
  for (int i = 0; i < 3; i++) s.thisToOther_t[i] = (float)thisToOther.t[i];
  double R2[9];
  lsdm::quatd_to_rot(thisToOther.q, R2);
  float R2f[9];
  for (int i = 0; i < 9; i++) R2f[i] = (float)R2[i] * (float)thisToOther.s;
  for (int i = 0; i < 3; i++) { s.row0[i] = R2f[i * 3 + 0]; s.row1[i] = R2f[i * 3 + 1]; s.row2[i] = R2f[i * 3 + 2]; }
  s.image = lsd_g(fr->d_image[0]);
  // (pointer AND id: a destroyed frame's heap address can be handed out again)
  s.parentIsKF = (fr->trackingParent == dm->activeKeyFrame && fr->trackingParentID == dm->activeKeyFrame->id) ? 1 : 0;
  s.wasGood = lsd_g(fr->wasGoodValid ? fr->d_wasGood : nullptr);
  s.id = fr->id;
  s.initialTrackedResidual = fr->initialTrackedResidual;
}

// the part of k_observe's arguments that does not depend on the reference frames
static void observe_args_common(lsdhip_depthmap* dm, ObserveArgs& a) {
  lsdhip_ctx* c = dm->ctx;
  lsdhip_frame* kf = dm->activeKeyFrame;
  a.m = dm->cur;
  a.kfImage = lsd_g(kf->d_image[0]);
  a.kfGrad = lsd_g(kf->d_grad[0]);
  a.kfMaxGrad = lsd_g(kf->d_maxgrad);
  a.reactivated = dm->activeKeyFrameIsReactivated ? 1 : 0;
  a.w = c->w; a.h = c->h;
  const LevelIntr& in = c->intr[0];
  a.fx = in.fx; a.fy = in.fy; a.cx = in.cx; a.cy = in.cy; a.fxi = in.fxi; a.fyi = in.fyi; a.cxi = in.cxi; a.cyi = in.cyi;
  a.minUseGrad = c->params.minUseGrad;
  a.cameraPixelNoise2 = c->params.cameraPixelNoise2;
  a.allowNegativeIdepths = c->params.allowNegativeIdepths;
  a.useSubpixelStereo = c->params.useSubpixelStereo;
  a.kfNumFramesTrackedOnThis = kf->numFramesTrackedOnThis;
  a.kfNumMappedOnThis = kf->numMappedOnThis;
  a.counters = nullptr;
  a.queue = nullptr;
  a.qcount = nullptr;
}

// a map is updated with frames that were tracked on its active keyframe
static int check_tracked_on(const lsdhip_frame* ref, const lsdhip_frame* kf) {
  if (ref->trackingParentID == kf->id) return LSDHIP_OK;
  // DepthMap.cpp:1099 needs getScaledCamToWorld() from the pose graph, which stays on the host side of the boundary
  lsd_set_error("updateKeyframe: frame %d was tracked on keyframe %d, active keyframe is %d (pose-graph path is out of scope)",
                ref->id, ref->trackingParentID, kf->id);
  return LSDHIP_E_STATE;
}
// k_observe's arguments for one reference frame (blockUntilMapped): it travels inside the record, no staging copy
static void observe_args_one(lsdhip_depthmap* dm, lsdhip_frame* ref, ObserveArgs& a) {
  memset((void*)&a, 0, sizeof(a));
  prepare_stereo(dm, ref, a.one);
  a.nByID = 1; a.byIDOffset = ref->id; a.nRefs = 1;
  observe_args_common(dm, a);
}

// countWork: the launch also counts its searches and walk steps (sampled while profiling)
static int observe(lsdhip_depthmap* dm, lsdhip_frame** refs, int n, bool countWork) {
  lsdhip_ctx* c = dm->ctx;
  LSD_CTX_LOCK(c);
  lsdhip_frame* kf = dm->activeKeyFrame;
  if (n <= 0) { lsd_set_error("updateKeyframe: empty reference deque"); return LSDHIP_E_ARG; }
  for (int i = 0; i < n; i++) if (int rct = check_tracked_on(refs[i], kf)) return rct;
  ObserveArgs a;
  if (n == 1) {
    observe_args_one(dm, refs[0], a);
  } else {
    size_t nByID = 0;
    const int offset = refs[0]->id;
    // host staging lives in one pinned block (refs | refByID); it is reused by the next call, which must not start
    // before this copy has been consumed
    int last = offset - 1;
    for (int i = 0; i < n; i++) if (refs[i]->id > last) last = refs[i]->id;
    const size_t byIDCount = (size_t)(last - offset + 1);
    const size_t refsBytes = up256(sizeof(StereoRef) * (size_t)n);
    const size_t need = refsBytes + sizeof(int) * byIDCount;
    HIPCHK(hipStreamSynchronize(lsd_map_stream(c)));
    if (need > dm->stage_bytes) {
      const size_t want = need > 65536 ? need * 2 : 65536;
      LsdPinned<char> h; LsdDev<char> d;      // (the new pair exists before the old one goes)
      if (int rc = lsd_pinned_alloc(h, want, hipHostMallocDefault)) return rc;
      if (int rc = lsd_dev_alloc(d, want)) return rc;
      dm->h_stage = std::move(h); dm->d_stage = std::move(d);
      dm->stage_bytes = want;
    }
    StereoRef* hrefs = (StereoRef*)dm->h_stage.get();
    int* byID = (int*)(dm->h_stage + refsBytes);
    for (int i = 0; i < n; i++) {
      prepare_stereo(dm, refs[i], hrefs[i]);
      while ((int)nByID + offset <= refs[i]->id) byID[nByID++] = i;
    }
    HIPCHK(hipMemcpyAsync(dm->d_stage, dm->h_stage, refsBytes + sizeof(int) * nByID, hipMemcpyHostToDevice, lsd_map_stream(c)));
    memset((void*)&a, 0, sizeof(a));
    a.refs = lsd_g((const StereoRef*)dm->d_stage.get());
    a.refByID = lsd_g((const int*)(dm->d_stage + refsBytes));
    a.nByID = (int)nByID;
    a.byIDOffset = offset;
    a.nRefs = n;
    observe_args_common(dm, a);
  }
#ifdef LSD_PHASE_TRACE
  {
    const size_t words = (size_t)((c->w + 31) / 32) * tile_rows(c) * 16;
    if (!dm->d_obs_trace) { if (int rc = lsd_dev_alloc(dm->d_obs_trace, words)) return rc; }
    HIPCHK(hipMemsetAsync(dm->d_obs_trace, 0, words * 8, lsd_map_stream(c)));
    a.trace = (decltype(a.trace))dm->d_obs_trace.get();
    dm->obs_trace_words = words;
  }
#endif
  {
#ifdef LSD_PHASE_TRACE
    constexpr int rows = 8;   // the trace buffer is laid out for 32x8 tiles
#else
    constexpr int rows = 2;
#endif
    const dim3 grid((c->w + 31) / 32, (c->h + rows - 1) / rows);
    const int nwaves = (int)(grid.x * grid.y) * (rows * 32 / 64);
    if (countWork) {
      // searches and walk steps, per wave, summed behind the launch (bench.py: stereo_steps_per_s,
      // roofline_depth on the bytes of the pixels that were actually searched)
      if (!dm->d_obsCounters) {
        if (int rc = lsd_dev_alloc(dm->d_obsCounters, (size_t)nwaves * 2 + 4)) return rc;
        dm->d_obsAcc = dm->d_obsCounters + (size_t)nwaves * 2;
        HIPCHK(hipMemsetAsync(dm->d_obsAcc, 0, 32, lsd_map_stream(c)));
        dm->obsCounterWaves = nwaves;
      }
      if (dm->obsCounterWaves == nwaves) a.counters = lsd_g(dm->d_obsCounters);
    }
    if (n == 1) hipLaunchKernelGGL((k_observe<true, rows>), grid, dim3(32 * rows), 0, lsd_map_stream(c), a);
    else hipLaunchKernelGGL((k_observe<false, rows>), grid, dim3(32 * rows), 0, lsd_map_stream(c), a);
    dm->lowGradHypPossible = false;   // (the pass drops a hypothesis on a pixel below the gradient threshold: observe_front)
  }
  if (a.counters) hipLaunchKernelGGL(k_obs_count_sum, dim3(1), dim3(256), 0, lsd_map_stream(c), (const unsigned long long*)dm->d_obsCounters, dm->obsCounterWaves, dm->d_obsAcc);
  HIPCHK(hipGetLastError());
  return LSDHIP_OK;
}

// oldToNew_SE3 = se3FromSim3(new_keyframe->pose->thisToParent_raw).inverse() (DepthMap.cpp:1230), in double
static lsdm::SE3dH old_to_new(const lsdhip_frame* nk) {
  lsdm::SE3dH newToOld;
  // se3FromSim3 = SE3(sim3.quaternion(), translation): the SCALED quaternion, normalised by the SO3 constructor (so3.hpp:630-633)
  newToOld.q = nk->thisToParent_raw.q;
  { const double s_ = nk->thisToParent_raw.s; newToOld.q.w *= s_; newToOld.q.x *= s_; newToOld.q.y *= s_; newToOld.q.z *= s_; }
  lsdm::q_normalize(newToOld.q);
  for (int i = 0; i < 3; i++) newToOld.t[i] = nk->thisToParent_raw.t[i];
  return lsdm::se3d_inverse(newToOld);
}
// the new keyframe's pose becomes sim3FromSE3(oldToNew.inverse()): its scale follows with the rescale factor (DepthMap.cpp:1305, lsd_frame_resolve)
static void drop_pose_scale(lsdhip_frame* nk, const lsdm::SE3dH& oldToNew) {
  const lsdm::SE3dH back = lsdm::se3d_inverse(oldToNew);
  nk->thisToParent_raw.q = back.q;
  lsdm::q_normalize(nk->thisToParent_raw.q);   // sim3FromSE3 -> Sim3::setScale normalises the quaternion (rxso3.hpp:332-335)
  for (int i = 0; i < 3; i++) nk->thisToParent_raw.t[i] = back.t[i];
}

// propagateDepth's arguments for the map's current keyframe -> nk (source = currentDepthMap, target = otherDepthMap)
static void prop_args(lsdhip_depthmap* dm, lsdhip_frame* nk, const lsdm::SE3dH& oldToNew, PropArgs& a) {
  lsdhip_ctx* c = dm->ctx;
  lsdhip_frame* old = dm->activeKeyFrame;
  size_t n = (size_t)c->w * c->h;
  a.src = dm->cur;
  a.dst = dm->oth;
  a.oldKFImage = lsd_g(old->d_image[0]);
  a.newKFImage = lsd_g(nk->d_image[0]);
  a.newKFMaxGrad = lsd_g(nk->d_maxgrad);
  a.trackingWasGood = lsd_g((nk->trackingParent == old && nk->trackingParentID == old->id && nk->wasGoodValid) ? nk->d_wasGood : nullptr);
  a.cand = lsd_g(dm->d_cand);
  a.slotCount = lsd_g(dm->d_slotCount);
  a.slots = lsd_g(dm->d_slots);
  a.flags = lsd_g(dm->d_flags);
  a.ovfHead = lsd_g(dm->d_ovfHead);
  a.ovf = lsd_g(dm->d_ovf);
  a.ovfCap = (int)n;
  a.w = c->w; a.h = c->h;
  const LevelIntr& in = c->intr[0];
  a.fx = in.fx; a.fy = in.fy; a.cx = in.cx; a.cy = in.cy; a.fxi = in.fxi; a.fyi = in.fyi; a.cxi = in.cxi; a.cyi = in.cyi;
  a.minUseGrad = c->params.minUseGrad;
  double Rd[9];   // (computed in double, cast to float)
  lsdm::quatd_to_rot(oldToNew.q, Rd);
  for (int i = 0; i < 9; i++) a.R[i] = (float)Rd[i];
  for (int i = 0; i < 3; i++) a.t[i] = (float)oldToNew.t[i];
}
// the rest state of the K7 scratch: slot counts, chain heads, flags
static int clear_prop_scratch(lsdhip_depthmap* dm, hipStream_t s) {
  const size_t n = (size_t)dm->ctx->w * dm->ctx->h;
  HIPCHK(hipMemsetAsync(dm->d_slotCount, 0, n * 4, s));
  HIPCHK(hipMemsetAsync(dm->d_ovfHead, 0xFF, n * 4, s));
  HIPCHK(hipMemsetAsync(dm->d_flags, 0, 64, s));
  return LSDHIP_OK;
}
static int propagate(lsdhip_depthmap* dm, lsdhip_frame* nk, const lsdm::SE3dH& oldToNew, bool checkOverflowNow) {
  lsdhip_ctx* c = dm->ctx;
  LSD_CTX_LOCK(c);
  PropArgs a;
  prop_args(dm, nk, oldToNew, a);
  if (int rcc = clear_prop_scratch(dm, lsd_map_stream(c))) return rcc;
  dm->propClean = false;      // (the flags stay set until somebody has read them: lsdhip_depth_change_keyframe_batch then clears first)
  hipLaunchKernelGGL(k_prop_candidates, dim3((c->w + 31) / 32, tile_rows(c)), dim3(256), 0, lsd_map_stream(c), a);
  hipLaunchKernelGGL(k_prop_resolve, dim3(px_blocks(c)), dim3(256), 0, lsd_map_stream(c), a);
  if (checkOverflowNow) {
    int flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, dm->d_flags, 4, hipMemcpyDeviceToHost, lsd_map_stream(c)));
    HIPCHK(hipStreamSynchronize(lsd_map_stream(c)));
    if (flag) {
      lsd_set_error("propagateDepth: overflow chains exhausted (more than w*h sources beyond %d per target)", PROP_SLOT_CAP);
      return LSDHIP_E_CAPACITY;
    }
  }   // otherwise the flag travels with the rescale sums of createKeyFrame (one synchronisation for the whole call)
  std::swap(dm->cur, dm->oth);
  return LSDHIP_OK;
}

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// GPU-side duration of a mapping call: an event pair on the stream, read back lazily (kind 0 update, 1 create, 2 finalize)
static void timing_collect(lsdhip_depthmap* dm, bool all) {
  for (int i = 0; i < 8; i++) {
    if (!dm->ev_pending[i]) continue;
    if (!all && hipEventQuery(dm->ev[i][1]) != hipSuccess) continue;
    float ms = 0;
    if (hipEventElapsedTime(&ms, dm->ev[i][0], dm->ev[i][1]) == hipSuccess) {
      dm->gpu_ms[dm->ev_kind[i]] += ms;
      dm->gpu_calls[dm->ev_kind[i]]++;
    }
    dm->ev_pending[i] = false;
  }
}
// GPU time of the DepthMap calls, SAMPLED: an event record is a barrier packet with a completion signal, and the kernel behind it
// starts ~10 us late (rocprofv3 timeline, profiles/r03_notes.md §2b) — two of them around every updateKeyframe cost 9 % of the
// track + map loop.  Every 7th updateKeyframe and every 2nd createKeyFrame / finalizeKeyFrame is bracketed (kind 3, k_observe
// alone, is sampled by its caller); gpu_ms / gpu_calls describe the bracketed calls only.  Returns EV_SKIP when the call is not sampled.
// (7, not 8: a loop with a keyframe every 10 frames runs exactly 8 (pipelined) or 9 updateKeyframe calls per keyframe, and the first
// update on a new keyframe searches 30x more pixels than the eighth — a period of 8 sampled one phase of that cycle only.)
constexpr int EV_SKIP = -1000;
static int timing_begin(lsdhip_depthmap* dm, int kind) {
  if (kind < 3) {
    const unsigned period = kind == 0 ? 7u : 2u;
    if ((dm->ev_tick[kind]++ % period) != 0) return EV_SKIP;
  }
  const int i = dm->ev_next;
  dm->ev_next = (dm->ev_next + 1) % 8;
  if (dm->ev_pending[i]) {
    HIPCHK(hipEventSynchronize(dm->ev[i][1]));
    timing_collect(dm, false);
  }
  if (!dm->ev[i][1]) { if (int rc = lsd_event_create(dm->ev[i][0])) return rc; if (int rc = lsd_event_create(dm->ev[i][1])) return rc; }
  dm->ev_kind[i] = kind;
  HIPCHK(hipEventRecord(dm->ev[i][0], lsd_map_stream(dm->ctx)));
  return i;
}
static int timing_end(lsdhip_depthmap* dm, int i) {
  if (i == EV_SKIP) return LSDHIP_OK;
  HIPCHK(hipEventRecord(dm->ev[i][1], lsd_map_stream(dm->ctx)));
  dm->ev_pending[i] = true;
  return LSDHIP_OK;
}

extern "C" int lsdhip_depth_init_gt(lsdhip_depthmap* dm, lsdhip_frame* kf) {
  if (!dm || !kf) return LSDHIP_E_ARG;
  if (!kf->hasIDepth) { lsd_set_error("initializeFromGTDepth: frame has no depth"); return LSDHIP_E_STATE; }
  lsdhip_ctx* c = dm->ctx;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  if (int rcl = lsd_frame_require_level0(kf)) return rcl;   // a DepthMap's keyframe is asked for gradients(0) / maxGradients(0)
  dm->lowGradHypPossible = true;
  dm->activeKeyFrame = kf;
  dm->activeKeyFrameIsReactivated = false;
  if (int rcb = lsd_m_begin(c)) return rcb;
  hipLaunchKernelGGL(k_init_gt, dim3(px_blocks(c)), dim3(256), 0, lsd_map_stream(c), dm->cur, kf->d_idepth[0], c->w * c->h);
  if (int rc = set_depth(dm)) return rc;
  return map_call_end(c);
}

extern "C" int lsdhip_depth_init_random(lsdhip_depthmap* dm, lsdhip_frame* kf) {
  if (!dm || !kf) return LSDHIP_E_ARG;
  lsdhip_ctx* c = dm->ctx;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  if (int rcl = lsd_frame_require_level0(kf)) return rcl;
  dm->lowGradHypPossible = true;
  dm->activeKeyFrame = kf;
  dm->activeKeyFrameIsReactivated = false;
  // initializeRandomly (DepthMap.cpp:883-916) draws from the C library's rand() in pixel order: a host-side init path.
  int w = c->w, h = c->h;
  size_t n = (size_t)w * h;
  std::vector<float> mg(n);
  if (int rcb = lsd_m_begin(c)) return rcb;
  HIPCHK(hipMemcpyAsync(mg.data(), kf->d_maxgrad, n * 4, hipMemcpyDeviceToHost, lsd_map_stream(c)));
  std::vector<lsdhip_hypothesis> hyp(n);
  HIPCHK(hipStreamSynchronize(lsd_map_stream(c)));
  int rc = lsdhip_depth_download(dm, hyp.data());
  if (rc) return rc;
  for (int y = 1; y < h - 1; y++)
    for (int x = 1; x < w - 1; x++) {
      lsdhip_hypothesis& p = hyp[x + y * w];
      if (mg[x + y * w] > c->params.minUseGrad) {
        float idepth = 0.5f + 1.0f * ((rand() % 100001) / 100000.0f);
        p.isValid = 1; p.blacklisted = 0; p.nextStereoFrameMinID = 0; p.validity_counter = 20;
        p.idepth = idepth; p.idepth_smoothed = idepth; p.idepth_var = VAR_RANDOM_INIT_INITIAL; p.idepth_var_smoothed = VAR_RANDOM_INIT_INITIAL;
      } else {
        p.isValid = 0; p.blacklisted = 0;
      }
    }
  rc = lsdhip_depth_upload(dm, kf, hyp.data(), 0);
  if (rc) return rc;
  rc = set_depth(dm);
  if (rc) return rc;
  return map_call_end(c);
}

extern "C" int lsdhip_depth_set_from_existing(lsdhip_depthmap* dm, lsdhip_frame* kf) {
  if (!dm || !kf) return LSDHIP_E_ARG;
  if (!kf->reActValid) { lsd_set_error("setFromExistingKF: frame %d has no re-activation data", kf->id); return LSDHIP_E_STATE; }
  lsdhip_ctx* c = dm->ctx;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  if (int rcl = lsd_frame_require_level0(kf)) return rcl;
  dm->lowGradHypPossible = true;
  dm->activeKeyFrame = kf;
  kf->numMappedOnThis = 0;
  kf->numFramesTrackedOnThis = 0;
  dm->activeKeyFrameIsReactivated = true;
  if (int rcb = lsd_m_begin(c)) return rcb;
  hipLaunchKernelGGL(k_from_react, dim3(px_blocks(c)), dim3(256), 0, lsd_map_stream(c), dm->cur, kf->d_idepth_reAct, kf->d_idepthVar_reAct,
                     kf->d_validity_reAct, c->w * c->h);
  int rc = regularize(dm, false, VAL_SUM_MIN_FOR_KEEP);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(lsd_map_stream(c)));
  return LSDHIP_OK;
}

static float ema(float old, double sample) { return (float)(0.9 * old + 0.1 * sample); }

extern "C" int lsdhip_depth_update(lsdhip_depthmap* dm, lsdhip_frame** refs, int n) {
  if (!dm || !refs || n <= 0) return LSDHIP_E_ARG;
  if (!dm->activeKeyFrame) { lsd_set_error("updateKeyframe: depth map has no active keyframe"); return LSDHIP_E_STATE; }
  lsdhip_ctx* c = dm->ctx;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  double t0 = now_ms();
  if (int rcb = lsd_m_begin(c)) return rcb;
  if (int rcg = lsd_gate_wait(c)) return rcg;
  const int ev = timing_begin(dm, 0);
  if (ev < 0 && ev != EV_SKIP) return ev;
  // while profiling, every 7th call brackets the observe kernel alone with a second event pair (bench.py roofline_depth)
  const bool sampleObs = c->prof_on && ((dm->obs_tick++ % 7) == 0);
  int evo = -1;
  if (sampleObs) { evo = timing_begin(dm, 3); if (evo < 0) return evo; }
  lsdhip_host_mark(10);
  int rc = observe(dm, refs, n, sampleObs);
  if (rc) return rc;
  lsdhip_host_mark(11);
  if (sampleObs) { rc = timing_end(dm, evo); if (rc) return rc; }
  lsdhip_frame* kf = dm->activeKeyFrame;
  const bool setDepth = !kf->depthHasBeenUpdatedFlag;
  rc = fill_regularize(dm, VAL_SUM_MIN_FOR_KEEP, setDepth);
  if (rc) return rc;
  lsdhip_host_mark(12);
  rc = timing_end(dm, ev);
  if (rc) return rc;
#ifdef LSD_DEVTOOLS
  {
    const size_t npx = (size_t)c->w * c->h;
    const int fid = refs[n - 1]->id;
    lsd_trace_sum(c, lsd_map_stream(c), 30, fid, refs[n - 1]->d_wasGood, (size_t)c->wl[1] * c->hl[1]);
    lsd_trace_sum(c, lsd_map_stream(c), 31, fid, dm->cur.valid, npx);
    lsd_trace_sum(c, lsd_map_stream(c), 32, fid, dm->cur.idepth, npx * 4);
    lsd_trace_sum(c, lsd_map_stream(c), 33, fid, dm->cur.var, npx * 4);
    lsd_trace_sum(c, lsd_map_stream(c), 34, fid, dm->cur.idepth_s, npx * 4);
    lsd_trace_sum(c, lsd_map_stream(c), 35, fid, dm->cur.validity, npx * 4);
    lsd_trace_sum(c, lsd_map_stream(c), 36, fid, dm->cur.blacklisted, npx * 4);
    lsd_trace_sum(c, lsd_map_stream(c), 37, fid, lsd_depth_latest(kf)[0], npx * 4);
    lsd_trace_sum(c, lsd_map_stream(c), 38, fid, lsd_depth_latest(kf)[1], npx);
    lsd_trace_sum(c, lsd_map_stream(c), 39, fid, lsd_depthvar_latest(kf)[1], npx);
  }
#endif
  rc = map_call_end(c);
  if (rc) return rc;
  dm->msUpdate = ema(dm->msUpdate, now_ms() - t0);   // host wall time of the call (enqueue time only in async mode)
  dm->referenceFrameByIDOffset = refs[0]->id;
  kf->numMappedOnThis++;
  kf->numMappedOnThisTotal++;
  return LSDHIP_OK;
}

// The jobs of one lsd_frame_build_idepth_pyramid_batch launch: a keyframe, the (sum, count) partials of its level-0 planes and the
// deferred-result slot its statistics go to
struct PyramidJobs {
  std::vector<lsdhip_frame*> frames; std::vector<const double*> parts; std::vector<int> nParts; std::vector<double*> outs;
  explicit PyramidJobs(size_t n) : frames(n), parts(n), nParts(n), outs(n) {}
  void set(size_t i, lsdhip_frame* f, const double* partials, int nPartials, int slot) {
    frames[i] = f; parts[i] = partials; nParts[i] = nPartials; outs[i] = (double*)&f->ctx->h_slots[slot];
  }
  int launch() { return lsd_frame_build_idepth_pyramid_batch(frames.data(), (int)frames.size(), parts.data(), 0, outs.data(), nParts.data()); }
};

// The argument record of a batched update, sub-records on 256-byte boundaries: ObserveArgs x n | RegItem x n | int x n (the search
// queues' fill counts).  One layout for the pinned host copy and its device twin: the views take either base.
struct UpdateRecord {
  size_t regOff, qcountOff, bytes;
  explicit UpdateRecord(int n)
      : regOff(up256(sizeof(ObserveArgs) * (size_t)n)), qcountOff(regOff + up256(sizeof(RegItem) * (size_t)n)), bytes(qcountOff + sizeof(int) * (size_t)n) {}
  ObserveArgs* obs(void* base) const { return (ObserveArgs*)base; }
  RegItem* reg(void* base) const { return (RegItem*)((uint8_t*)base + regOff); }
  int* qcount(void* base) const { return (int*)((uint8_t*)base + qcountOff); }
};

static int update_batch_check(lsdhip_ctx* c, int n, lsdhip_depthmap** maps, lsdhip_frame** refs) {
  for (int j = 0; j < n; j++) {
    lsdhip_depthmap* dm = maps[j];
    if (dm->ctx != c || refs[j]->ctx != c) { lsd_set_error("updateKeyframe batch: maps and frames of one batch live on one context"); return LSDHIP_E_ARG; }
    if (!dm->activeKeyFrame) { lsd_set_error("updateKeyframe batch: depth map %d has no active keyframe", j); return LSDHIP_E_STATE; }
    for (int i = 0; i < j; i++) if (maps[i] == dm) { lsd_set_error("updateKeyframe batch: depth map %d appears twice", j); return LSDHIP_E_ARG; }
    if (int rct = check_tracked_on(refs[j], dm->activeKeyFrame)) return rct;
  }
  return LSDHIP_OK;
}
// Fills the host copy of the record: per map what observe() and fill_regularize() would pass.  due: the maps whose keyframe is due for
// Frame::setDepth; *candidates is cleared unless every map of the call qualifies for the select pass over the keyframes' gradient candidates.
static void update_batch_items(int n, lsdhip_depthmap** maps, lsdhip_frame** refs, const UpdateRecord& L, void* host, void* dev, bool split,
                               std::vector<int>& due, bool* candidates) {
  for (int j = 0; j < n; j++) {
    lsdhip_depthmap* dm = maps[j];
    lsdhip_frame* kf = dm->activeKeyFrame;
    ObserveArgs& a = L.obs(host)[j];
    observe_args_one(dm, refs[j], a);
    a.queue = lsd_g(split ? dm->d_obsQueue : nullptr);
    a.qcount = lsd_g(L.qcount(dev) + j);
    a.gradCand = lsd_g((const uint16_t*)kf->d_gradCand);
    if (dm->lowGradHypPossible || kf->gradCandTh != a.minUseGrad) *candidates = false;
    L.qcount(host)[j] = 0;       // the queues' fill counts start from the zeros copied here
    const bool setDepth = !kf->depthHasBeenUpdatedFlag;
    L.reg(host)[j] = reg_item(dm, setDepth ? kf : nullptr, dm->d_red + 16);
    if (setDepth) due.push_back(j);
  }
}
// the observe pass in the form `form` names: select + walk (the select over every pixel or over the gradient candidates), or one launch
static int update_batch_observe(lsdhip_ctx* c, int n, const ObserveArgs* dobs, const lsdhip_ctx::BatchForm& form, hipStream_t ms) {
  const int bp = lsd_bprof_begin(c, 1, ms);
  if (bp < -1) return bp;
  if (form.split) {
    unsigned long long* acc = nullptr;
    if (bp >= 0) {     // a sampled call also counts its searches and walk steps
      if (!c->d_obsBatchAcc) { if (int rc = lsd_dev_alloc(c->d_obsBatchAcc, 66)) return rc; HIPCHK(hipMemsetAsync(c->d_obsBatchAcc, 0, 66 * 8, ms)); }
      acc = c->d_obsBatchAcc;
    }
    if (form.candidates) hipLaunchKernelGGL(k_observe_select_cand_batch, dim3((lsd_gradcand_groups(c->w * c->h) + 3) / 4, 1, n), dim3(256), 0, ms, dobs);
    else hipLaunchKernelGGL(k_observe_select_batch, dim3((c->w + 63) / 64, (c->h + 15) / 16, n), dim3(256), 0, ms, dobs);
    hipLaunchKernelGGL(k_observe_walk_batch, dim3(form.walkWorkgroups), dim3(64), 0, ms, dobs, form.qcountDev, n, acc);
  } else {
    hipLaunchKernelGGL((k_observe_batch<2>), dim3((c->w + 31) / 32, (c->h + 1) / 2, n), dim3(64), 0, ms, dobs);
  }
  return lsd_bprof_end(c, bp, ms, (double)n * c->w * c->h);
}
// the regulariser pass: the maps whose keyframe is due for Frame::setDepth in one launch, the others in its twin
static int update_batch_regularize(lsdhip_ctx* c, int n, const RegItem* dreg, const RegGrid& g, int nSet, hipStream_t ms) {
  const int bp = lsd_bprof_begin(c, 2, ms);
  if (bp < -1) return bp;
  LSD_REG_DISPATCH(g.py,
    if (nSet > 0) hipLaunchKernelGGL((k_reg_fused_batch<PassUpdateSetDepth, PYV>), g.grid, dim3(256), 0, ms, dreg);
    if (nSet < n) hipLaunchKernelGGL((k_reg_fused_batch<PassUpdate, PYV>), g.grid, dim3(256), 0, ms, dreg));
  if (int rc = lsd_bprof_end(c, bp, ms, (double)n * c->w * c->h)) return rc;
  HIPCHK(hipGetLastError());
  return LSDHIP_OK;
}
// Frame::setDepth's second half for the keyframes that were due.  At most LSD_NUM_SLOTS keyframes per pyramid launch: claiming a slot that
// still has an owner resolves that owner first, which is only right once the launch that writes the slot has been queued — with more
// keyframes than slots in ONE launch the ring wrapped onto keyframes of the same call, whose statistics were then read before anything had
// written them (numPoints = 0).
static int update_batch_set_depth(lsdhip_ctx* c, lsdhip_depthmap** maps, const std::vector<int>& due, int nPartials, hipStream_t ms) {
  if (due.empty()) return LSDHIP_OK;
  const int bp = lsd_bprof_begin(c, 3, ms);
  if (bp < -1) return bp;
  for (size_t i0 = 0; i0 < due.size(); i0 += LSD_NUM_SLOTS) {
    PyramidJobs pyr(std::min<size_t>(LSD_NUM_SLOTS, due.size() - i0));
    for (size_t i = 0; i < pyr.frames.size(); i++) {
      lsdhip_depthmap* dm = maps[due[i0 + i]];
      const int slot = lsd_ctx_claim_stats_slot(c, dm->activeKeyFrame);
      if (slot < 0) return slot;
      pyr.set(i, dm->activeKeyFrame, dm->d_red + 16, nPartials, slot);
    }
    if (int rc = pyr.launch()) return rc;
    for (lsdhip_frame* kf : pyr.frames) kf->depthHasBeenUpdatedFlag = true;
  }
  return lsd_bprof_end(c, bp, ms, (double)due.size() * c->w * c->h);
}

// DepthMap::updateKeyframe for the maps of n sequences, one tracked frame each (the blockUntilMapped deque), in three launches for
// all of them: k_observe_batch, k_reg_fused_batch (+ its non-setDepth twin if some keyframe is not due), k_idepth_pyramid_batch.
// Per map the arithmetic, the launch geometry inside its z-slice and therefore every plane are those of lsdhip_depth_update.
extern "C" int lsdhip_depth_update_batch(int n, lsdhip_depthmap** maps, lsdhip_frame** refs) {
  if (n <= 0 || !maps || !refs) return LSDHIP_E_ARG;
  for (int j = 0; j < n; j++) if (!maps[j] || !refs[j]) return LSDHIP_E_ARG;
  lsdhip_ctx* c = maps[0]->ctx;
  LSD_CTX_LOCK(c);
  if (int rcv = update_batch_check(c, n, maps, refs)) return rcv;
  HIPCHK(hipSetDevice(c->device));
  double t0 = now_ms();
  if (int rcb = lsd_m_begin(c)) return rcb;
  const hipStream_t ms = lsd_map_stream(c);
  lsdhip_ctx::BatchForm form;     // what this call runs: becomes c->batchForm[0] once everything is queued
  form.n = n;
  form.split = n >= LSD_OBS_SPLIT_MIN_MAPS && n <= LSD_OBS_WALK_MAX_MAPS;
  form.walkWorkgroups = form.split ? LSD_OBS_WALK_WAVES : 0;
  if (form.split)
    for (int j = 0; j < n; j++)
      if (!maps[j]->d_obsQueue) { if (int rc = lsd_dev_alloc(maps[j]->d_obsQueue, (size_t)c->w * c->h)) return rc; }
  const UpdateRecord L(n);
  void *host = nullptr, *dev = nullptr;
  if (int rc = lsd_args_begin(c, L.bytes, &host, &dev)) return rc;
  form.qcountDev = L.qcount(dev); form.argsSerial = c->args.serial; form.argsGen = c->args.gen;   // (the record's place in the ring: lsdhip_ctx_batch_form)
  std::vector<int> due;
  bool candidates = true;
  update_batch_items(n, maps, refs, L, host, dev, form.split, due, &candidates);
  form.nSet = (int)due.size();
  form.candidates = form.split && candidates;
  if (int rc = lsd_args_commit(c, ms)) return rc;
  const RegGrid g = reg_grid(c, tile_rows(c), n);
  form.py = g.py;
  if (int rc = update_batch_observe(c, n, L.obs(dev), form, ms)) return rc;
  if (int rc = update_batch_regularize(c, n, L.reg(dev), g, form.nSet, ms)) return rc;
  if (int rc = lsd_args_release(c, dev, ms)) return rc;
  for (int j = 0; j < n; j++) { swap_valid(maps[j]); maps[j]->lowGradHypPossible = false; }   // (every form of the observe pass drops a hypothesis below the threshold)
  if (int rc = update_batch_set_depth(c, maps, due, g.tiles(), ms)) return rc;
  if (int rc = map_call_end(c)) return rc;
  form.synced = !c->async;
  c->batchForm[0] = form;
  if (!c->async)
    for (int j = 0; j < n; j++) if (int rc = lsd_frame_resolve(maps[j]->activeKeyFrame)) return rc;
  const double dt = now_ms() - t0;
  for (int j = 0; j < n; j++) {
    lsdhip_depthmap* dm = maps[j];
    dm->msUpdate = ema(dm->msUpdate, dt / n);
    dm->referenceFrameByIDOffset = refs[j]->id;
    dm->activeKeyFrame->numMappedOnThis++;
    dm->activeKeyFrame->numMappedOnThisTotal++;
  }
  return LSDHIP_OK;
}

extern "C" int lsdhip_depth_create_keyframe(lsdhip_depthmap* dm, lsdhip_frame* nk, float* rescale_out) {
  if (!dm || !nk) return LSDHIP_E_ARG;
  if (!dm->activeKeyFrame) { lsd_set_error("createKeyFrame: depth map has no active keyframe"); return LSDHIP_E_STATE; }
  if (!nk->trackingParent) { lsd_set_error("createKeyFrame: new keyframe has no tracking parent"); return LSDHIP_E_STATE; }
  lsdhip_ctx* c = dm->ctx;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  double t0 = now_ms();
  const lsdm::SE3dH oldToNew = old_to_new(nk);

  if (int rcb = lsd_m_begin(c)) return rcb;
  const int ev = timing_begin(dm, 1);
  if (ev < 0 && ev != EV_SKIP) return ev;
  if (int rcl = lsd_frame_require_level0(nk)) return rcl;   // the new keyframe's maxGradients(0): propagateDepth reads it (DepthMap.cpp:758)
  int rc = propagate(dm, nk, oldToNew, false);
  if (rc) return rc;
  dm->msPropagate = ema(dm->msPropagate, now_ms() - t0);
  dm->activeKeyFrame = nk;
  dm->activeKeyFrameIsReactivated = false;
  rc = regularize(dm, true, VAL_SUM_MIN_FOR_KEEP);
  if (rc) return rc;
  rc = fill_regularize(dm, VAL_SUM_MIN_FOR_KEEP, false);
  if (rc) return rc;

  // make mean inverse depth be one (DepthMap.cpp:1285-1304): the factor is formed on the device (k_rescale), the host
  // copy of (sum, count) and the propagation overflow flag are a deferred result of the new keyframe
  const int n = c->w * c->h;
  const int nb = (int)px_blocks(c);
  const int slot = lsd_ctx_claim_rescale_slot(c, nk);
  if (slot < 0) return slot;
  hipLaunchKernelGGL(k_sum_valid_idepth, dim3(nb), dim3(256), 0, lsd_map_stream(c), dm->cur, n, dm->d_red + 16);
  hipLaunchKernelGGL(k_reduce_pairs, dim3(1), dim3(256), 0, lsd_map_stream(c), dm->d_red + 16, nb, (double*)&c->h_slots[slot], dm->d_red,
                     (const int*)dm->d_flags);
  hipLaunchKernelGGL(k_rescale, dim3(nb), dim3(256), 0, lsd_map_stream(c), dm->cur, n, dm->d_red);
  drop_pose_scale(nk, oldToNew);
  rc = set_depth(dm);
  if (rc) return rc;
  rc = timing_end(dm, ev);
  if (rc) return rc;
  if (lsd_m_record(c) < 0) return LSDHIP_E_HIP;
  if (!c->async || rescale_out) {
    rc = lsd_frame_resolve(nk);
    if (rc) return rc;
    if (rescale_out) *rescale_out = (float)nk->thisToParent_raw.s;
  }
  dm->msCreate = ema(dm->msCreate, now_ms() - t0);
  return LSDHIP_OK;
}

// A keyframe change edits host-side state of the maps, of both keyframes and of the context's slot ring while it builds the launches'
// arguments, and several steps can fail (a slot, the argument ring, a launch).  The edits are undone unless the call gets as far as its
// last launch: an error leaves every map on its old keyframe with its planes where they were, not half-way.
struct ChangeTxn {
  lsdhip_ctx* c; int n; lsdhip_depthmap** maps; lsdhip_frame** nks;
  struct M { HypPlanes cur, oth; uint8_t* snap; lsdhip_frame* kf; bool react; bool propClean; int oldStats; int nkRescale, nkStats; lsdm::Sim3dH nkPose; };
  std::vector<M> m;
  std::vector<int> slots;      // slots claimed by this call
  int slotNext; int ev = EV_SKIP; bool timing = false; bool done = false;
  ChangeTxn(lsdhip_ctx* c_, int n_, lsdhip_depthmap** maps_, lsdhip_frame** nks_) : c(c_), n(n_), maps(maps_), nks(nks_), m((size_t)n_), slotNext(c_->slot_next) {
    for (int j = 0; j < n; j++) {
      lsdhip_depthmap* dm = maps[j];
      m[j] = M{dm->cur, dm->oth, dm->d_validSnap, dm->activeKeyFrame, dm->activeKeyFrameIsReactivated, dm->propClean, dm->activeKeyFrame->pendStats,
               nks[j]->pendRescale, nks[j]->pendStats, nks[j]->thisToParent_raw};
    }
  }
  int stats_slot(lsdhip_frame* f) { const int s = lsd_ctx_claim_stats_slot(c, f); if (s >= 0) slots.push_back(s); return s; }
  int rescale_slot(lsdhip_frame* f) { const int s = lsd_ctx_claim_rescale_slot(c, f); if (s >= 0) slots.push_back(s); return s; }
  ~ChangeTxn() {
    if (done) return;
    for (int s : slots) { c->slot_stats_owner[s] = nullptr; c->slot_rescale_owner[s] = nullptr; }
    c->slot_next = slotNext;
    for (int j = 0; j < n; j++) {
      lsdhip_depthmap* dm = maps[j];
      dm->cur = m[j].cur; dm->oth = m[j].oth; dm->d_validSnap = m[j].snap; dm->activeKeyFrame = m[j].kf; dm->activeKeyFrameIsReactivated = m[j].react;
      dm->propClean = false;                       // (the K7 scratch may have been written: the next call clears it)
      m[j].kf->pendStats = m[j].oldStats;
      if (m[j].oldStats >= 0) c->slot_stats_owner[m[j].oldStats] = m[j].kf;
      nks[j]->pendRescale = m[j].nkRescale; nks[j]->pendStats = m[j].nkStats;
      if (m[j].nkRescale >= 0) c->slot_rescale_owner[m[j].nkRescale] = nks[j];
      if (m[j].nkStats >= 0) c->slot_stats_owner[m[j].nkStats] = nks[j];
      nks[j]->thisToParent_raw = m[j].nkPose;
    }
    if (timing) (void)timing_end(maps[0], ev);     // (keeps the event pair of the timing sample balanced)
  }
};
// The argument record of a keyframe change, sub-records on 256-byte boundaries: KfItem x n | RegItem x n (the pass that removes
// occlusions) | RegItem x n (fill holes + regularise) | RescaleItem x n.  One layout for the pinned host copy and its device twin.
struct ChangeRecord {
  size_t occOff, fillOff, resOff, bytes;
  explicit ChangeRecord(int n)
      : occOff(up256(sizeof(KfItem) * (size_t)n)), fillOff(occOff + up256(sizeof(RegItem) * (size_t)n)),
        resOff(fillOff + up256(sizeof(RegItem) * (size_t)n)), bytes(resOff + up256(sizeof(RescaleItem) * (size_t)n)) {}
  KfItem* kf(void* base) const { return (KfItem*)base; }
  RegItem* occ(void* base) const { return (RegItem*)((uint8_t*)base + occOff); }
  RegItem* fill(void* base) const { return (RegItem*)((uint8_t*)base + fillOff); }
  RescaleItem* res(void* base) const { return (RescaleItem*)((uint8_t*)base + resOff); }
};

static int change_keyframe_check(lsdhip_ctx* c, int n, lsdhip_depthmap** maps, lsdhip_frame** nks) {
  for (int j = 0; j < n; j++) {
    lsdhip_depthmap* dm = maps[j];
    if (dm->ctx != c || nks[j]->ctx != c) { lsd_set_error("keyframe change batch: maps and frames of one batch live on one context"); return LSDHIP_E_ARG; }
    if (!dm->activeKeyFrame) { lsd_set_error("keyframe change batch: depth map %d has no active keyframe", j); return LSDHIP_E_STATE; }
    if (!nks[j]->trackingParent) { lsd_set_error("createKeyFrame: new keyframe has no tracking parent"); return LSDHIP_E_STATE; }
    if (nks[j] == dm->activeKeyFrame) { lsd_set_error("keyframe change batch: map %d: the new keyframe is the current one", j); return LSDHIP_E_ARG; }
    for (int i = 0; i < j; i++)
      if (maps[i] == dm || nks[i] == nks[j]) { lsd_set_error("keyframe change batch: entry %d appears twice", j); return LSDHIP_E_ARG; }
  }
  return LSDHIP_OK;
}
// Map j's records of the change, and the host-side state of the map and of both keyframes as the six launches will leave it.  The order
// of swap_valid, std::swap(cur, oth) and the three reg_args snapshots is what the launches depend on: each record describes the planes as
// the launch before it leaves them.  pyr: jobs j (old keyframe) and n + j (new keyframe) of the pyramid launch.
static int change_build_map(ChangeTxn& txn, int j, const ChangeRecord& L, void* host, int ntiles, int nwg5, PyramidJobs& pyr) {
  lsdhip_depthmap* dm = txn.maps[j];
  lsdhip_frame* old = dm->activeKeyFrame;
  lsdhip_frame* nk = txn.nks[j];
  double* setA = dm->d_red + 16;
  double* setB = setA + dm->redStride;
  double* setC = setB + dm->redStride;
  const lsdm::SE3dH oldToNew = old_to_new(nk);
  // finalizeKeyFrame: the pass on the old keyframe's map, its Frame::setDepth (level 0 + partials), re-activation data; phase A of
  // propagateDepth into otherDepthMap
  KfItem& k = L.kf(host)[j];
  memset((void*)&k, 0, sizeof(k));
  k.a = reg_args(dm, VAL_SUM_MIN_FOR_KEEP);
  k.id0 = lsd_g(lsd_depth_w(old)[0]); k.var0 = lsd_g(lsd_depthvar_w(old)[0]); k.partials = lsd_g(setA);
  k.x.reactId = lsd_g(old->d_idepth_reAct); k.x.reactVar = lsd_g(old->d_idepthVar_reAct); k.x.reactVal = lsd_g(old->d_validity_reAct);
  prop_args(dm, nk, oldToNew, k.x.prop);
  swap_valid(dm);
  int slot = txn.stats_slot(old);
  if (slot < 0) return slot;
  pyr.set(j, old, setA, ntiles, slot);
  // createKeyFrame: the new keyframe's map becomes the current one
  std::swap(dm->cur, dm->oth);
  dm->activeKeyFrame = nk;
  dm->activeKeyFrameIsReactivated = false;
  L.occ(host)[j] = reg_item(dm, nullptr, nullptr);
  swap_valid(dm);
  L.fill(host)[j] = reg_item(dm, nullptr, setB);
  swap_valid(dm);
  RescaleItem& r = L.res(host)[j];
  memset((void*)&r, 0, sizeof(r));
  r.m = dm->cur;
  r.sumPartials = lsd_g(setB); r.nSumPartials = ntiles;
  r.flags = lsd_g(dm->d_flags);
  slot = txn.rescale_slot(nk);
  if (slot < 0) return slot;
  r.slot = lsd_g((double*)&txn.c->h_slots[slot]);
  r.id0 = lsd_g(lsd_depth_w(nk)[0]); r.var0 = lsd_g(lsd_depthvar_w(nk)[0]);
  r.statPartials = lsd_g(setC);
  r.n = txn.c->w * txn.c->h;
  slot = txn.stats_slot(nk);
  if (slot < 0) return slot;
  pyr.set(txn.n + j, nk, setC, nwg5, slot);
  drop_pose_scale(nk, oldToNew);
  return LSDHIP_OK;
}
// five of the six launches of the change (kernels above); the pyramid launch follows
static int change_launch(lsdhip_ctx* c, int n, const ChangeRecord& L, void* dev, const RegGrid& g, int nwg5, hipStream_t ms) {
  const KfItem* dkf = L.kf(dev);
  LSD_REG_DISPATCH(g.py, hipLaunchKernelGGL(k_kf_finalize_prop<PYV>, g.grid, dim3(256), 0, ms, dkf));
  hipLaunchKernelGGL(k_prop_resolve_batch, dim3(px_blocks(c), n), dim3(256), 0, ms, dkf);
  LSD_REG_DISPATCH(g.py, hipLaunchKernelGGL((k_kf_reg<PassRegOcc, PYV>), g.grid, dim3(256), 0, ms, L.occ(dev)));
  LSD_REG_DISPATCH(g.py, hipLaunchKernelGGL((k_kf_reg<PassKfFillSums, PYV>), g.grid, dim3(256), 0, ms, L.fill(dev)));
  hipLaunchKernelGGL(k_kf_rescale_setdepth, dim3(nwg5, n), dim3(256), 0, ms, L.res(dev));
  HIPCHK(hipGetLastError());
  return LSDHIP_OK;
}
// the change of at most LSD_NUM_SLOTS / 3 maps (validated by the caller)
static int change_keyframe_part(lsdhip_ctx* c, int n, lsdhip_depthmap** maps, lsdhip_frame** new_keyframes, float* rescale_out) {
  HIPCHK(hipSetDevice(c->device));
  const double t0 = now_ms();
  if (int rcb = lsd_m_begin(c)) return rcb;
  const hipStream_t ms = lsd_map_stream(c);
  const RegGrid g = reg_grid(c, tile_rows(c), n);
  const int nwg5 = (c->w * c->h + LSD_RESCALE_PX - 1) / LSD_RESCALE_PX;
  ChangeTxn txn(c, n, maps, new_keyframes);
  for (int j = 0; j < n; j++) {
    lsdhip_depthmap* dm = maps[j];
    // (a single-call propagation, or a failed call, left the K7 scratch in use)
    if (!dm->propClean) { if (int rcc = clear_prop_scratch(dm, ms)) return rcc; }
    dm->propClean = false;
  }
  const int ev = timing_begin(maps[0], 1);
  if (ev < 0 && ev != EV_SKIP) return ev;
  txn.ev = ev; txn.timing = true;
  if (int rcl = lsd_frames_require_level0(new_keyframes, n)) return rcl;   // the new keyframes' gradients(0) / maxGradients(0), one launch pair
  const ChangeRecord L(n);
  void *host = nullptr, *dev = nullptr;
  if (int rc = lsd_args_begin(c, L.bytes, &host, &dev)) return rc;
  PyramidJobs pyr((size_t)2 * n);
  for (int j = 0; j < n; j++) if (int rc = change_build_map(txn, j, L, host, g.tiles(), nwg5, pyr)) return rc;
  if (int rc = lsd_args_commit(c, ms)) return rc;
  const int bp = lsd_bprof_begin(c, 4, ms);
  if (bp < -1) return bp;
  if (int rc = change_launch(c, n, L, dev, g, nwg5, ms)) return rc;
  if (int rc = lsd_args_release(c, dev, ms)) return rc;
  if (int rc = pyr.launch()) return rc;
  if (int rc = lsd_bprof_end(c, bp, ms, (double)n * c->w * c->h)) return rc;
  txn.done = true;            // every launch of the change is queued: the new state stands
  { lsdhip_ctx::BatchForm& bf = c->batchForm[1]; bf = lsdhip_ctx::BatchForm(); bf.n = n; bf.py = g.py; }
  for (int j = 0; j < n; j++) {
    maps[j]->propClean = true;
    txn.m[j].kf->depthHasBeenUpdatedFlag = true;
    txn.m[j].kf->reActValid = true;
    new_keyframes[j]->depthHasBeenUpdatedFlag = true;
  }
  if (int rc = timing_end(maps[0], ev)) return rc;
  if (lsd_m_record(c) < 0) return LSDHIP_E_HIP;
  if (!c->async || rescale_out) {
    for (int j = 0; j < n; j++) {
      if (!c->async) { if (int rc = lsd_frame_resolve(txn.m[j].kf)) return rc; }
      if (int rc = lsd_frame_resolve(new_keyframes[j])) return rc;
      if (rescale_out) rescale_out[j] = (float)new_keyframes[j]->thisToParent_raw.s;
    }
  }
  const double dt = now_ms() - t0;
  for (int j = 0; j < n; j++) maps[j]->msCreate = ema(maps[j]->msCreate, dt / n);
  return LSDHIP_OK;
}

// DepthMap::finalizeKeyFrame (DepthMap.cpp:1363-1395) on the current keyframes of n maps followed by DepthMap::createKeyFrame(new_keyframes[j])
// (:1222-1327), in six launches shared by all maps (kernels above).  Per map every plane, the re-activation data, both keyframes' idepth
// pyramids and the deferred results (mean inverse depth / point counts, rescale factor, overflow flag) are those of
// lsdhip_depth_finalize + lsdhip_depth_create_keyframe (tests/test_multiseq_gpu.py).
extern "C" int lsdhip_depth_change_keyframe_batch(int n, lsdhip_depthmap** maps, lsdhip_frame** new_keyframes, float* rescale_out) {
  if (n <= 0 || !maps || !new_keyframes) return LSDHIP_E_ARG;
  for (int j = 0; j < n; j++) if (!maps[j] || !new_keyframes[j]) return LSDHIP_E_ARG;
  lsdhip_ctx* c = maps[0]->ctx;
  LSD_CTX_LOCK(c);
  if (int rcv = change_keyframe_check(c, n, maps, new_keyframes)) return rcv;
  // A change holds three deferred-result slots per map until its launches are queued, and claiming a slot that still has an owner resolves
  // that owner first — right only once the launch that writes the slot has been queued.  More maps than a third of the ring go in
  // consecutive parts, so that the ring never wraps onto a map of the part being prepared (it did: the first maps of a call of more than
  // 85 read their rescale factor and statistics before anything had written them).
  constexpr int maxPerPart = LSD_NUM_SLOTS / 3;
  for (int j0 = 0; j0 < n; j0 += maxPerPart) {
    const int part = n - j0 < maxPerPart ? n - j0 : maxPerPart;
    if (int rcp = change_keyframe_part(c, part, maps + j0, new_keyframes + j0, rescale_out ? rescale_out + j0 : nullptr)) return rcp;
  }
  c->batchForm[1].n = n;     // (py: that of the last part)
  return LSDHIP_OK;
}

// A re-activating change edits the same kinds of host-side state as a creating one (ChangeTxn), less of it: the maps' validity planes and
// active keyframe, the finalised keyframes' statistics slot, the old keyframes' counters.  Undone unless the last launch gets queued.
struct ReactivateTxn {
  lsdhip_ctx* c; int n; lsdhip_depthmap** maps; lsdhip_frame** olds;
  struct M { HypPlanes cur; uint8_t* snap; lsdhip_frame* kf; bool react, lowGrad; int kfStats; int mapped, tracked; };
  std::vector<M> m;
  std::vector<int> slots;
  int slotNext; int ev = EV_SKIP; bool timing = false; bool done = false;
  ReactivateTxn(lsdhip_ctx* c_, int n_, lsdhip_depthmap** maps_, lsdhip_frame** olds_) : c(c_), n(n_), maps(maps_), olds(olds_), m((size_t)n_), slotNext(c_->slot_next) {
    for (int j = 0; j < n; j++) {
      lsdhip_depthmap* dm = maps[j];
      m[j] = M{dm->cur, dm->d_validSnap, dm->activeKeyFrame, dm->activeKeyFrameIsReactivated, dm->lowGradHypPossible, dm->activeKeyFrame->pendStats,
               olds[j]->numMappedOnThis, olds[j]->numFramesTrackedOnThis};
    }
  }
  int stats_slot(lsdhip_frame* f) { const int s = lsd_ctx_claim_stats_slot(c, f); if (s >= 0) slots.push_back(s); return s; }
  ~ReactivateTxn() {
    if (done) return;
    for (int s : slots) c->slot_stats_owner[s] = nullptr;
    c->slot_next = slotNext;
    for (int j = 0; j < n; j++) {
      lsdhip_depthmap* dm = maps[j];
      dm->cur = m[j].cur; dm->d_validSnap = m[j].snap; dm->activeKeyFrame = m[j].kf; dm->activeKeyFrameIsReactivated = m[j].react;
      dm->lowGradHypPossible = m[j].lowGrad;
      m[j].kf->pendStats = m[j].kfStats;
      if (m[j].kfStats >= 0) c->slot_stats_owner[m[j].kfStats] = m[j].kf;
      olds[j]->numMappedOnThis = m[j].mapped; olds[j]->numFramesTrackedOnThis = m[j].tracked;
    }
    if (timing) (void)timing_end(maps[0], ev);
  }
};
// The argument record of a re-activating change: KfItem x n | ReactItem x n, the second on a 256-byte boundary
struct ReactivateRecord {
  size_t srcOff, bytes;
  explicit ReactivateRecord(int n) : srcOff(up256(sizeof(KfItem) * (size_t)n)), bytes(srcOff + up256(sizeof(ReactItem) * (size_t)n)) {}
  KfItem* kf(void* base) const { return (KfItem*)base; }
  ReactItem* src(void* base) const { return (ReactItem*)((uint8_t*)base + srcOff); }
};
static int reactivate_check(lsdhip_ctx* c, int n, lsdhip_depthmap** maps, lsdhip_frame** olds) {
  for (int j = 0; j < n; j++) {
    lsdhip_depthmap* dm = maps[j];
    if (dm->ctx != c || olds[j]->ctx != c) { lsd_set_error("keyframe re-activation batch: maps and frames of one batch live on one context"); return LSDHIP_E_ARG; }
    for (int i = 0; i < j; i++)
      if (maps[i] == dm || olds[i] == olds[j]) { lsd_set_error("keyframe re-activation batch: entry %d appears twice", j); return LSDHIP_E_ARG; }
    // (a keyframe that another map of the call finalises would have its planes written and read by launches of one call)
    for (int i = 0; i < n; i++)
      if (maps[i] && olds[j] == maps[i]->activeKeyFrame) {
        lsd_set_error("keyframe re-activation batch: entry %d: frame %d is the current keyframe of map %d", j, olds[j]->id, i);
        return LSDHIP_E_ARG;
      }
  }
  for (int j = 0; j < n; j++) {
    if (!maps[j]->activeKeyFrame) { lsd_set_error("keyframe re-activation batch: depth map %d has no active keyframe", j); return LSDHIP_E_STATE; }
    if (!olds[j]->reActValid) { lsd_set_error("setFromExistingKF: frame %d has no re-activation data", olds[j]->id); return LSDHIP_E_STATE; }
  }
  return LSDHIP_OK;
}
// Map j's two records, and the host-side state of the map and of both keyframes as the three launches will leave it.  As in
// change_build_map each record describes the planes as the launch before it leaves them: the finalise pass reads cur.valid and writes the
// spare plane, the pass from the re-activation planes writes the first again, and the map ends on the plane it began on.
static int reactivate_build_map(ReactivateTxn& txn, int j, const ReactivateRecord& L, void* host, int ntiles, PyramidJobs& pyr) {
  lsdhip_depthmap* dm = txn.maps[j];
  lsdhip_frame* cur = dm->activeKeyFrame;
  lsdhip_frame* old = txn.olds[j];
  double* setA = dm->d_red + 16;
  // finalizeKeyFrame (DepthMap.cpp:1363-1395)
  KfItem& k = L.kf(host)[j];
  memset((void*)&k, 0, sizeof(k));
  k.a = reg_args(dm, VAL_SUM_MIN_FOR_KEEP);
  k.id0 = lsd_g(lsd_depth_w(cur)[0]); k.var0 = lsd_g(lsd_depthvar_w(cur)[0]); k.partials = lsd_g(setA);
  k.x.reactId = lsd_g(cur->d_idepth_reAct); k.x.reactVar = lsd_g(cur->d_idepthVar_reAct); k.x.reactVal = lsd_g(cur->d_validity_reAct);
  swap_valid(dm);
  const int slot = txn.stats_slot(cur);
  if (slot < 0) return slot;
  pyr.set(j, cur, setA, ntiles, slot);
  // setFromExistingKF (DepthMap.cpp:920-962)
  dm->lowGradHypPossible = true;
  dm->activeKeyFrame = old;
  old->numMappedOnThis = 0;
  old->numFramesTrackedOnThis = 0;
  dm->activeKeyFrameIsReactivated = true;
  ReactItem& r = L.src(host)[j];
  memset((void*)&r, 0, sizeof(r));
  r.a = reg_args(dm, VAL_SUM_MIN_FOR_KEEP);
  r.src.id = lsd_g((const float*)old->d_idepth_reAct); r.src.var = lsd_g((const float*)old->d_idepthVar_reAct);
  r.src.val = lsd_g((const uint8_t*)old->d_validity_reAct);
  swap_valid(dm);
  return LSDHIP_OK;
}
// the re-activation of at most LSD_NUM_SLOTS maps (validated by the caller): one deferred-result slot per map
static int reactivate_keyframe_part(lsdhip_ctx* c, int n, lsdhip_depthmap** maps, lsdhip_frame** olds) {
  HIPCHK(hipSetDevice(c->device));
  const double t0 = now_ms();
  if (int rcb = lsd_m_begin(c)) return rcb;
  const hipStream_t ms = lsd_map_stream(c);
  const RegGrid g = reg_grid(c, tile_rows(c), n);
  if (int rcl = lsd_frames_require_level0(olds, n)) return rcl;   // a DepthMap's keyframe is asked for gradients(0) / maxGradients(0)
  ReactivateTxn txn(c, n, maps, olds);
  const int ev = timing_begin(maps[0], 2);
  if (ev < 0 && ev != EV_SKIP) return ev;
  txn.ev = ev; txn.timing = true;
  const ReactivateRecord L(n);
  void *host = nullptr, *dev = nullptr;
  if (int rc = lsd_args_begin(c, L.bytes, &host, &dev)) return rc;
  PyramidJobs pyr((size_t)n);
  for (int j = 0; j < n; j++) if (int rc = reactivate_build_map(txn, j, L, host, g.tiles(), pyr)) return rc;
  if (int rc = lsd_args_commit(c, ms)) return rc;
  LSD_REG_DISPATCH(g.py, hipLaunchKernelGGL(k_kf_finalize<PYV>, g.grid, dim3(256), 0, ms, (const KfItem*)L.kf(dev)));
  LSD_REG_DISPATCH(g.py, hipLaunchKernelGGL(k_kf_from_react<PYV>, g.grid, dim3(256), 0, ms, (const ReactItem*)L.src(dev)));
  HIPCHK(hipGetLastError());
  if (int rc = lsd_args_release(c, dev, ms)) return rc;
  if (int rc = pyr.launch()) return rc;
  txn.done = true;            // every launch is queued: the new state stands
  for (int j = 0; j < n; j++) {
    txn.m[j].kf->depthHasBeenUpdatedFlag = true;
    txn.m[j].kf->reActValid = true;
  }
  if (int rc = timing_end(maps[0], ev)) return rc;
  if (lsd_m_record(c) < 0) return LSDHIP_E_HIP;
  if (!c->async)
    for (int j = 0; j < n; j++) { if (int rc = lsd_frame_resolve(txn.m[j].kf)) return rc; }
  const double dt = now_ms() - t0;
  for (int j = 0; j < n; j++) maps[j]->msFinalize = ema(maps[j]->msFinalize, dt / n);
  return LSDHIP_OK;
}

// DepthMap::finalizeKeyFrame (DepthMap.cpp:1363-1395) on the current keyframes of n maps followed by DepthMap::setFromExistingKF(old_keyframes[j])
// (:920-962), in three launches shared by all maps (kernels above) and without a host wait on an asynchronous context.  Per map every
// plane, the finalised keyframe's level-0 planes, pyramid, re-activation data and deferred statistics are those of lsdhip_depth_finalize +
// lsdhip_depth_set_from_existing (tests/test_reactivate_batch_gpu.py).
extern "C" int lsdhip_depth_reactivate_keyframe_batch(int n, lsdhip_depthmap** maps, lsdhip_frame** old_keyframes) {
  if (n <= 0 || !maps || !old_keyframes) return LSDHIP_E_ARG;
  for (int j = 0; j < n; j++) if (!maps[j] || !old_keyframes[j]) return LSDHIP_E_ARG;
  lsdhip_ctx* c = maps[0]->ctx;
  LSD_CTX_LOCK(c);
  if (int rcv = reactivate_check(c, n, maps, old_keyframes)) return rcv;
  // (one slot per map: a part never wraps the ring onto itself, see lsdhip_depth_change_keyframe_batch)
  constexpr int maxPerPart = LSD_NUM_SLOTS;
  for (int j0 = 0; j0 < n; j0 += maxPerPart) {
    const int part = n - j0 < maxPerPart ? n - j0 : maxPerPart;
    if (int rcp = reactivate_keyframe_part(c, part, maps + j0, old_keyframes + j0)) return rcp;
  }
  return LSDHIP_OK;
}

extern "C" int lsdhip_depth_finalize(lsdhip_depthmap* dm) {
  if (!dm) return LSDHIP_E_ARG;
  if (!dm->activeKeyFrame) { lsd_set_error("finalizeKeyFrame: depth map has no active keyframe"); return LSDHIP_E_STATE; }
  lsdhip_ctx* c = dm->ctx;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  double t0 = now_ms();
  if (int rcb = lsd_m_begin(c)) return rcb;
  const int ev = timing_begin(dm, 2);
  if (ev < 0 && ev != EV_SKIP) return ev;
  int rc = fill_regularize(dm, VAL_SUM_MIN_FOR_KEEP, true);
  if (rc) return rc;
  lsdhip_frame* kf = dm->activeKeyFrame;
  hipLaunchKernelGGL(k_take_react, dim3(px_blocks(c)), dim3(256), 0, lsd_map_stream(c), dm->cur, kf->d_idepth_reAct,
                     kf->d_idepthVar_reAct, kf->d_validity_reAct, c->w * c->h);
  rc = timing_end(dm, ev);
  if (rc) return rc;
  rc = map_call_end(c);
  if (rc) return rc;
  kf->reActValid = true;
  dm->msFinalize = ema(dm->msFinalize, now_ms() - t0);
  return LSDHIP_OK;
}

// GPU time (ms, summed) and call counts of updateKeyframe / createKeyFrame / finalizeKeyFrame since creation
extern "C" int lsdhip_depth_observe_time(lsdhip_depthmap* dm, double* ms_out, long long* calls_out) {
  if (!dm || !ms_out || !calls_out) return LSDHIP_E_ARG;
  HIPCHK(hipSetDevice(dm->ctx->device));
  HIPCHK(hipStreamSynchronize(lsd_map_stream(dm->ctx)));
  timing_collect(dm, true);
  *ms_out = dm->gpu_ms[3];
  *calls_out = dm->gpu_calls[3];
  return LSDHIP_OK;
}
// the sampled k_observe launches' work: out[0] = launches counted, out[1] = pixels that entered the epipolar search, out[2] = walk steps
// (sum of doLineStereo's loopCounter); synchronises
extern "C" int lsdhip_depth_observe_work(lsdhip_depthmap* dm, double out[3]) {
  if (!dm || !out) return LSDHIP_E_ARG;
  out[0] = out[1] = out[2] = 0;
  if (!dm->d_obsAcc) return LSDHIP_OK;
  HIPCHK(hipSetDevice(dm->ctx->device));
  HIPCHK(hipStreamSynchronize(lsd_map_stream(dm->ctx)));
  unsigned long long acc[3];
  HIPCHK(hipMemcpy(acc, dm->d_obsAcc, sizeof(acc), hipMemcpyDeviceToHost));
  out[0] = (double)acc[2]; out[1] = (double)acc[0]; out[2] = (double)acc[1];
  return LSDHIP_OK;
}
extern "C" int lsdhip_depth_gpu_times(lsdhip_depthmap* dm, double ms_out[3], long long calls_out[3]) {
  if (!dm || !ms_out || !calls_out) return LSDHIP_E_ARG;
  HIPCHK(hipSetDevice(dm->ctx->device));
  HIPCHK(hipStreamSynchronize(lsd_map_stream(dm->ctx)));
  timing_collect(dm, true);
  for (int i = 0; i < 3; i++) { ms_out[i] = dm->gpu_ms[i]; calls_out[i] = dm->gpu_calls[i]; }
  return LSDHIP_OK;
}

extern "C" int lsdhip_depth_download(lsdhip_depthmap* dm, lsdhip_hypothesis* out) {
  if (!dm || !out) return LSDHIP_E_ARG;
  lsdhip_ctx* c = dm->ctx;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  size_t n = (size_t)c->w * c->h;
  std::vector<uint8_t> v(n);
  std::vector<int32_t> bl(n), vc(n);
  std::vector<float> nid(n), id(n), var(n), ids(n), vars(n);
  if (int rcb = lsd_m_begin(c)) return rcb;
  HIPCHK(hipMemcpyAsync(v.data(), dm->cur.valid, n, hipMemcpyDeviceToHost, lsd_map_stream(c)));
  HIPCHK(hipMemcpyAsync(bl.data(), dm->cur.blacklisted, n * 4, hipMemcpyDeviceToHost, lsd_map_stream(c)));
  HIPCHK(hipMemcpyAsync(vc.data(), dm->cur.validity, n * 4, hipMemcpyDeviceToHost, lsd_map_stream(c)));
  HIPCHK(hipMemcpyAsync(nid.data(), dm->cur.nextID, n * 4, hipMemcpyDeviceToHost, lsd_map_stream(c)));
  HIPCHK(hipMemcpyAsync(id.data(), dm->cur.idepth, n * 4, hipMemcpyDeviceToHost, lsd_map_stream(c)));
  HIPCHK(hipMemcpyAsync(var.data(), dm->cur.var, n * 4, hipMemcpyDeviceToHost, lsd_map_stream(c)));
  HIPCHK(hipMemcpyAsync(ids.data(), dm->cur.idepth_s, n * 4, hipMemcpyDeviceToHost, lsd_map_stream(c)));
  HIPCHK(hipMemcpyAsync(vars.data(), dm->cur.var_s, n * 4, hipMemcpyDeviceToHost, lsd_map_stream(c)));
  HIPCHK(hipStreamSynchronize(lsd_map_stream(c)));
  for (size_t i = 0; i < n; i++) {
    lsdhip_hypothesis& h = out[i];
    h.isValid = v[i]; h.pad_[0] = h.pad_[1] = h.pad_[2] = 0;
    h.blacklisted = bl[i]; h.nextStereoFrameMinID = nid[i]; h.validity_counter = vc[i];
    h.idepth = id[i]; h.idepth_var = var[i]; h.idepth_smoothed = ids[i]; h.idepth_var_smoothed = vars[i];
  }
  return LSDHIP_OK;
}
extern "C" int lsdhip_depth_upload(lsdhip_depthmap* dm, lsdhip_frame* kf, const lsdhip_hypothesis* in, int reactivated) {
  if (!dm || !kf || !in) return LSDHIP_E_ARG;
  lsdhip_ctx* c = dm->ctx;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  size_t n = (size_t)c->w * c->h;
  std::vector<uint8_t> v(n);
  std::vector<int32_t> bl(n), vc(n);
  std::vector<float> nid(n), id(n), var(n), ids(n), vars(n);
  for (size_t i = 0; i < n; i++) {
    const lsdhip_hypothesis& h = in[i];
    // (the fused regulariser packs "invalid" as a negative counter in its LDS tile; the reference never produces a negative one)
    if (h.isValid && h.validity_counter < 0) { lsd_set_error("lsdhip_depth_upload: pixel %zu is valid with validity_counter %d < 0", i, h.validity_counter); return LSDHIP_E_ARG; }
    v[i] = h.isValid ? 1 : 0; bl[i] = h.blacklisted; nid[i] = h.nextStereoFrameMinID; vc[i] = h.validity_counter;
    id[i] = h.idepth; var[i] = h.idepth_var; ids[i] = h.idepth_smoothed; vars[i] = h.idepth_var_smoothed;
  }
  if (int rcb = lsd_m_begin(c)) return rcb;
  HIPCHK(hipMemcpyAsync(dm->cur.valid, v.data(), n, hipMemcpyHostToDevice, lsd_map_stream(c)));
  HIPCHK(hipMemcpyAsync(dm->cur.blacklisted, bl.data(), n * 4, hipMemcpyHostToDevice, lsd_map_stream(c)));
  HIPCHK(hipMemcpyAsync(dm->cur.validity, vc.data(), n * 4, hipMemcpyHostToDevice, lsd_map_stream(c)));
  HIPCHK(hipMemcpyAsync(dm->cur.nextID, nid.data(), n * 4, hipMemcpyHostToDevice, lsd_map_stream(c)));
  HIPCHK(hipMemcpyAsync(dm->cur.idepth, id.data(), n * 4, hipMemcpyHostToDevice, lsd_map_stream(c)));
  HIPCHK(hipMemcpyAsync(dm->cur.var, var.data(), n * 4, hipMemcpyHostToDevice, lsd_map_stream(c)));
  HIPCHK(hipMemcpyAsync(dm->cur.idepth_s, ids.data(), n * 4, hipMemcpyHostToDevice, lsd_map_stream(c)));
  HIPCHK(hipMemcpyAsync(dm->cur.var_s, vars.data(), n * 4, hipMemcpyHostToDevice, lsd_map_stream(c)));
  HIPCHK(hipStreamSynchronize(lsd_map_stream(c)));
  if (int rcl = lsd_frame_require_level0(kf)) return rcl;
  dm->lowGradHypPossible = true;
  dm->activeKeyFrame = kf;
  dm->activeKeyFrameIsReactivated = reactivated != 0;
  return LSDHIP_OK;
}

extern "C" int lsdhip_depth_stage(lsdhip_depthmap* dm, int stage, lsdhip_frame** refs, int n) {
  if (!dm) return LSDHIP_E_ARG;
  if (!dm->activeKeyFrame) { lsd_set_error("depth stage: no active keyframe"); return LSDHIP_E_STATE; }
  lsdhip_ctx* c = dm->ctx;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  int rc = LSDHIP_E_ARG;
  if (int rcb = lsd_m_begin(c)) return rcb;
  switch (stage) {
    case 0: rc = observe(dm, refs, n, false); break;
    case 1: rc = fill_holes(dm); break;
    case 2: rc = regularize(dm, false, VAL_SUM_MIN_FOR_KEEP); break;
    case 3: rc = regularize(dm, true, VAL_SUM_MIN_FOR_KEEP); break;
    case 4:
      if (!refs || n < 1) return LSDHIP_E_ARG;
      rc = lsd_frame_require_level0(refs[0]);
      if (rc == LSDHIP_OK) rc = propagate(dm, refs[0], old_to_new(refs[0]), true);
      if (rc == LSDHIP_OK) { dm->activeKeyFrame = refs[0]; dm->activeKeyFrameIsReactivated = false; }
      break;
    case 5: rc = fill_regularize(dm, VAL_SUM_MIN_FOR_KEEP, false); break;
    default: return LSDHIP_E_ARG;
  }
  if (rc) return rc;
  return map_call_end(c);
}

extern "C" int lsdhip_depth_stage_rows(lsdhip_depthmap* dm, int stage, int tile_row0, int n_tile_rows, int last) {
  if (!dm || stage != 5) return LSDHIP_E_ARG;
  if (!dm->activeKeyFrame) { lsd_set_error("depth stage: no active keyframe"); return LSDHIP_E_STATE; }
  lsdhip_ctx* c = dm->ctx;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  int rc = fill_regularize_rows(dm, VAL_SUM_MIN_FOR_KEEP, tile_row0, n_tile_rows, last != 0);
  if (rc) return rc;
  if (!c->async) HIPCHK(hipStreamSynchronize(lsd_map_stream(c)));
  return LSDHIP_OK;
}

extern "C" int lsdhip_depth_stage_rows_batch(lsdhip_ctx* c, int n, lsdhip_depthmap** maps, const int* tile_row0, const int* n_tile_rows) {
  if (!c || n < 0 || (n > 0 && (!maps || !tile_row0 || !n_tile_rows))) return LSDHIP_E_ARG;
  if (n == 0) return LSDHIP_OK;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  int maxRows = 0;
  long long rowsInAll = 0;
  for (int k = 0; k < n; k++) {
    if (!maps[k] || maps[k]->ctx != c) return LSDHIP_E_ARG;
    if (!maps[k]->activeKeyFrame) { lsd_set_error("depth stage: no active keyframe"); return LSDHIP_E_STATE; }
    if (int rcr = check_tile_rows(c, tile_row0[k], n_tile_rows[k], 1)) return rcr;
    if (n_tile_rows[k] > maxRows) maxRows = n_tile_rows[k];
    rowsInAll += n_tile_rows[k];
  }
  void* host = nullptr;
  void* dev = nullptr;
  int rc = lsd_args_begin(c, sizeof(RegItem) * (size_t)n, &host, &dev);
  if (rc) return rc;
  RegItem* items = (RegItem*)host;
  for (int k = 0; k < n; k++) {
    items[k] = reg_item(maps[k], nullptr, nullptr);
    items[k].a.tileRow0 = tile_row0[k];
    items[k].a.tileRows = n_tile_rows[k];
  }
  const hipStream_t ms = lsd_map_stream(c);
  rc = lsd_args_commit(c, ms);
  if (rc) return rc;
  const RegGrid g = reg_grid(c, maxRows, n, rowsInAll);
  LSD_REG_DISPATCH(g.py, hipLaunchKernelGGL(k_reg_rows_batch<PYV>, g.grid, dim3(256), 0, ms, (const RegItem*)dev));
  HIPCHK(hipGetLastError());
  rc = lsd_args_release(c, dev, ms);
  if (rc) return rc;
  if (!c->async) HIPCHK(hipStreamSynchronize(ms));
  return LSDHIP_OK;
}

extern "C" int lsdhip_depth_copy_planes_dev(lsdhip_depthmap* dm, float* idepth_dev, float* var_dev) {
  if (!dm || !idepth_dev || !var_dev) return LSDHIP_E_ARG;
  if (!dm->activeKeyFrame || !(dm->activeKeyFrame->hasIDepth || dm->activeKeyFrame->depthPending)) return LSDHIP_E_STATE;
  lsdhip_ctx* c = dm->ctx;
  LSD_CTX_LOCK(c);
  size_t n = (size_t)c->w * c->h;
  // what the last Frame::setDepth of the mapping side left (on a pipelined context possibly not yet published to the tracker)
  if (int rcb = lsd_m_begin(c)) return rcb;
  HIPCHK(hipMemcpyAsync(idepth_dev, lsd_depth_latest(dm->activeKeyFrame)[0], n * 4, hipMemcpyDeviceToDevice, lsd_map_stream(c)));
  HIPCHK(hipMemcpyAsync(var_dev, lsd_depthvar_latest(dm->activeKeyFrame)[0], n * 4, hipMemcpyDeviceToDevice, lsd_map_stream(c)));
  return map_call_end(c);
}

// Rows [row0, row0 + nrows) of the eight hypothesis planes <-> one packed device buffer (plane after plane: isValid u8,
// blacklisted i32, nextStereoFrameMinID f32, validity_counter i32, idepth, idepth_var, idepth_smoothed,
// idepth_var_smoothed = 29 bytes per pixel): the halo payload of the row-band decomposition.
extern "C" int lsdhip_depth_copy_rows_dev(lsdhip_depthmap* dm, int row0, int nrows, void* packed_dev, int to_map) {
  if (!dm || !packed_dev || row0 < 0 || nrows <= 0) return LSDHIP_E_ARG;
  lsdhip_ctx* c = dm->ctx;
  LSD_CTX_LOCK(c);
  if (row0 + nrows > c->h) return LSDHIP_E_ARG;
  HIPCHK(hipSetDevice(c->device));
  const size_t px = (size_t)nrows * c->w, off = (size_t)row0 * c->w;
  char* p = (char*)packed_dev;
  struct { void* plane; size_t elt; } planes[8] = {
      {dm->cur.valid, 1}, {dm->cur.blacklisted, 4}, {dm->cur.nextID, 4}, {dm->cur.validity, 4},
      {dm->cur.idepth, 4}, {dm->cur.var, 4}, {dm->cur.idepth_s, 4}, {dm->cur.var_s, 4}};
  for (int k = 0; k < 8; k++) {
    char* mp = (char*)planes[k].plane + off * planes[k].elt;
    const size_t bytes = px * planes[k].elt;
    if (to_map) HIPCHK(hipMemcpyAsync(mp, p, bytes, hipMemcpyDeviceToDevice, lsd_map_stream(c)));
    else HIPCHK(hipMemcpyAsync(p, mp, bytes, hipMemcpyDeviceToDevice, lsd_map_stream(c)));
    p += bytes;
  }
  HIPCHK(hipStreamSynchronize(lsd_map_stream(c)));
  return LSDHIP_OK;
}

// Several row ranges in ONE launch: map rows -> map rows of another window (halo refresh between windows that live on the same
// GPU), map rows -> packed buffer (before an ncclSend), packed buffer -> map rows (after an ncclRecv).  Everything is ordered
// on the context's stream; nothing synchronises the host.
struct CopyPlanes { char* p[8]; };
struct CopyItem { CopyPlanes src, dst; int npx; };
#define LSD_COPY_ITEMS 16
struct CopyBatch { CopyItem it[LSD_COPY_ITEMS]; };
__global__ __launch_bounds__(256) void k_copy_rows(CopyBatch b, int vec) {
  // the item is picked by blockIdx.y: its 16 plane pointers and its size are read from the kernel-argument segment directly
  // (indexing the by-value struct with a runtime index would copy it to scratch)
  typedef const unsigned long long __attribute__((address_space(4))) cu64;
  cu64* q = (cu64*)__builtin_amdgcn_kernarg_segment_ptr() + (size_t)blockIdx.y * (sizeof(CopyItem) / 8);
  const char* s0 = (const char*)q[0]; const char* s1 = (const char*)q[1]; const char* s2 = (const char*)q[2]; const char* s3 = (const char*)q[3];
  const char* s4 = (const char*)q[4]; const char* s5 = (const char*)q[5]; const char* s6 = (const char*)q[6]; const char* s7 = (const char*)q[7];
  char* d0 = (char*)q[8]; char* d1 = (char*)q[9]; char* d2 = (char*)q[10]; char* d3 = (char*)q[11];
  char* d4 = (char*)q[12]; char* d5 = (char*)q[13]; char* d6 = (char*)q[14]; char* d7 = (char*)q[15];
  const int npx = (int)(unsigned)q[16];
  if (vec) {   // 4 pixels per lane: one 4-byte word of the validity plane, one 16-byte vector of each 4-byte plane
    const int n4 = npx >> 2;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
      const unsigned v0 = ((const unsigned*)s0)[i];
      const uint4 v1 = ((const uint4*)s1)[i], v2 = ((const uint4*)s2)[i], v3 = ((const uint4*)s3)[i], v4 = ((const uint4*)s4)[i];
      const uint4 v5 = ((const uint4*)s5)[i], v6 = ((const uint4*)s6)[i], v7 = ((const uint4*)s7)[i];
      ((unsigned*)d0)[i] = v0;
      ((uint4*)d1)[i] = v1; ((uint4*)d2)[i] = v2; ((uint4*)d3)[i] = v3; ((uint4*)d4)[i] = v4;
      ((uint4*)d5)[i] = v5; ((uint4*)d6)[i] = v6; ((uint4*)d7)[i] = v7;
    }
  } else {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npx; i += gridDim.x * 256) {
      d0[i] = s0[i];
      ((unsigned*)d1)[i] = ((const unsigned*)s1)[i]; ((unsigned*)d2)[i] = ((const unsigned*)s2)[i]; ((unsigned*)d3)[i] = ((const unsigned*)s3)[i];
      ((unsigned*)d4)[i] = ((const unsigned*)s4)[i]; ((unsigned*)d5)[i] = ((const unsigned*)s5)[i]; ((unsigned*)d6)[i] = ((const unsigned*)s6)[i];
      ((unsigned*)d7)[i] = ((const unsigned*)s7)[i];
    }
  }
}
static_assert(sizeof(CopyItem) == 17 * 8, "k_copy_rows reads a CopyItem as 17 quadwords");
static bool copy_planes_of(lsdhip_ctx* c, lsdhip_depthmap* dm, int row0, void* packed, int nrows, CopyPlanes& out) {
  const size_t px = (size_t)nrows * c->w;
  if (dm) {
    if (dm->ctx != c || row0 < 0 || row0 + nrows > c->h) return false;
    const size_t off = (size_t)row0 * c->w;
    void* planes[8] = {dm->cur.valid, dm->cur.blacklisted, dm->cur.nextID, dm->cur.validity, dm->cur.idepth, dm->cur.var, dm->cur.idepth_s, dm->cur.var_s};
    for (int k = 0; k < 8; k++) out.p[k] = (char*)planes[k] + off * (k == 0 ? 1 : 4);
  } else {
    if (!packed) return false;
    char* p = (char*)packed;
    for (int k = 0; k < 8; k++) { out.p[k] = p; p += px * (k == 0 ? 1 : 4); }
  }
  return true;
}
extern "C" int lsdhip_depth_copy_rows_batch(lsdhip_ctx* c, int n, const lsdhip_row_copy* items) {
  if (!c || n < 0 || (n > 0 && !items)) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(c);
  HIPCHK(hipSetDevice(c->device));
  for (int base = 0; base < n; base += LSD_COPY_ITEMS) {
    CopyBatch b;
    memset(&b, 0, sizeof(b));
    const int m = n - base < LSD_COPY_ITEMS ? n - base : LSD_COPY_ITEMS;
    int maxpx = 0, vec = 1;
    for (int i = 0; i < m; i++) {
      const lsdhip_row_copy& r = items[base + i];
      if (r.nrows <= 0 || !copy_planes_of(c, r.src_map, r.src_row0, r.src_packed, r.nrows, b.it[i].src) ||
          !copy_planes_of(c, r.dst_map, r.dst_row0, r.dst_packed, r.nrows, b.it[i].dst)) {
        lsd_set_error("lsdhip_depth_copy_rows_batch: item %d is not a row range of a depth map of this context / a packed buffer", base + i);
        return LSDHIP_E_ARG;
      }
      b.it[i].npx = r.nrows * c->w;
      if (b.it[i].npx > maxpx) maxpx = b.it[i].npx;
      if (b.it[i].npx & 3) vec = 0;
      for (int k = 0; k < 8; k++)
        if (((uintptr_t)b.it[i].src.p[k] | (uintptr_t)b.it[i].dst.p[k]) & (k == 0 ? 3 : 15)) vec = 0;
    }
    const int per = vec ? maxpx / 4 : maxpx;
    int gx = (per + 255) / 256;
    if (gx > 512) gx = 512;
    if (gx < 1) gx = 1;
    hipLaunchKernelGGL(k_copy_rows, dim3(gx, m), dim3(256), 0, lsd_transport_stream(c), b, vec);
  }
  HIPCHK(hipGetLastError());
  if (!c->async) HIPCHK(hipStreamSynchronize(lsd_transport_stream(c)));
  return LSDHIP_OK;
}

extern "C" int lsdhip_depth_timings(lsdhip_depthmap* dm, float out[8]) {
  if (!dm || !out) return LSDHIP_E_ARG;
  out[0] = dm->msUpdate; out[1] = dm->msCreate; out[2] = dm->msFinalize; out[3] = dm->msObserve; out[4] = dm->msRegularize;
  out[5] = dm->msPropagate; out[6] = dm->msFillHoles; out[7] = dm->msSetDepth;
  return LSDHIP_OK;
}

// what the last batched update / keyframe change on the context ran (include/lsdhip.h); the queue counts of a split update are read
// from the call's argument record here, on request: the calls themselves keep host-side notes only
extern "C" int lsdhip_ctx_batch_form(lsdhip_ctx* c, int which, int out[8], int* queueCounts, int maxCounts) {
  if (!c || !out || which < 0 || which > 1 || (queueCounts && maxCounts < 0)) return LSDHIP_E_ARG;
  LSD_CTX_LOCK(c);
  const lsdhip_ctx::BatchForm& bf = c->batchForm[which];
  out[0] = bf.n; out[1] = bf.split ? 1 : 0; out[2] = bf.candidates ? 1 : 0; out[3] = bf.py; out[4] = bf.nSet; out[5] = bf.walkWorkgroups;
  out[6] = -1; out[7] = -1;
  const lsdhip_ctx::ArgRing& r = c->args;
  const bool readable = bf.n > 0 && bf.split && bf.synced && bf.qcountDev && r.d && bf.argsGen == r.gen &&
                        r.serial - bf.argsSerial < (unsigned long long)lsdhip_ctx::ArgRing::NS;
  if (!readable) return LSDHIP_OK;
  HIPCHK(hipSetDevice(c->device));
  std::vector<int> cnt((size_t)bf.n);
  HIPCHK(hipMemcpy(cnt.data(), bf.qcountDev, sizeof(int) * (size_t)bf.n, hipMemcpyDeviceToHost));
  long long entries = 0, chunks = 0;
  for (int j = 0; j < bf.n; j++) {
    entries += cnt[j];
    chunks += (cnt[j] + 63) >> 6;
    if (queueCounts && j < maxCounts) queueCounts[j] = cnt[j];
  }
  out[6] = (int)entries; out[7] = (int)chunks;
  return LSDHIP_OK;
}
