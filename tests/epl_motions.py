"""General camera motions for the epipolar search (makeAndCheckEPL + doLineStereo and their callers), and a census of the branches a
motion reaches.  No GPU here.

synth.Scene moves the camera on a small circle in the x-y plane: in the frames the depth tests use, the camera centre keeps C_x < 0,
C_y > 0, C_z ~ 0, so the epipolar direction stays in one quadrant, the walk advances with one pair of signs, segments are clipped at
the same two borders, the epipole is never inside the image and rescaleFactor stays at 1.  FreeScene renders the same surface from
explicit poses; MOTIONS names the poses of the second camera relative to the keyframe (world units of scene S1, depth ~ 2); census()
restates the GEOMETRY of the search in float64 numpy to classify pixels — it is never an expected value: expected values come from the
oracle alone."""
import functools
import math
from collections import OrderedDict

import numpy as np

from common import synth

# C/util/settings.h (the values oracle/lsd_oracle.hpp and csrc/depthmap.hip carry)
MIN_DEPTH = 0.05
STEREO_EPL_VAR_FAC = 2.0
MIN_EPL_LENGTH_SQUARED = 1.0
MIN_EPL_GRAD_SQUARED = 4.0
MIN_EPL_ANGLE_SQUARED = 0.09
MAX_EPL_LENGTH_CROP = 30.0
MIN_EPL_LENGTH_CROP = 3.0
SAMPLE_POINT_TO_BORDER = 7
MIN_BLACKLIST = -1
# stereo_walk_serial (csrc/depthmap.hip; the batched walk runs the same function through observe_back): before the loop it reads
# pFar - 2 inc ... pFar + 3 inc; step k (position pFar + k inc) requests the sample of step k + 2, which lies 2 inc ahead of that
# step's position: pFar + (k + 4) inc.  Every sample is bilinear: taps (int x, int y) and one further in each axis.
WALK_BEHIND = 2
WALK_AHEAD = 4
FID0 = 4          # frame id of motion k (1-based) = FID0 + k: behind the nextStereoFrameMinID = 4.0 that _noisy_hyp plants


class FreeScene(synth.Scene):
    """synth.Scene seen from explicit camera poses: poses[i] = (R, C), rotation and centre of camera i in the world; camera 0 should be
    (I, 0).  render() and frame_to_ref() of the base class work for general poses."""

    def __init__(self, poses, seq_index=0, kind="S1"):
        super().__init__(seq_index, kind, len(poses))
        self.poses = [(np.asarray(R, np.float64), np.asarray(C, np.float64)) for R, C in poses]

    def cam_to_world(self, i):
        return self.poses[i]


def rot(rx, ry, rz):
    """R = Rz(rz) Ry(ry) Rx(rx): pitch about x, yaw about y, roll about the optical axis"""
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


TWIST_TZ = 0.003   # t_z of test_gpu_parity._ref_pose's twist, before its (1 + 0.1 i) factor


def _motions():
    """name -> (rotation (rx, ry, rz), camera centre, seq_index of the scene the second image shows).  Every pose is composed with
    _ref_pose's general twist before use (pose_of): pure axis motions would leave exact zeros in R and t."""
    m = OrderedDict()
    m["x+"] = ((0, 0, 0), (0.08, 0, 0), 0)
    m["x-"] = ((0, 0, 0), (-0.08, 0, 0), 0)
    m["y+"] = ((0, 0, 0), (0, 0.08, 0), 0)
    m["y-"] = ((0, 0, 0), (0, -0.08, 0), 0)
    m["diag++"] = ((0, 0, 0), (0.06, 0.06, 0), 0)       # the two quadrants of C the circle never visits
    m["diag+-"] = ((0, 0, 0), (0.06, -0.06, 0), 0)
    m["forward"] = ((0, 0, 0), (0.005, 0.003, 0.15), 0)     # epipole inside the image, off the pixel centres
    m["backward"] = ((0, 0, 0), (0.004, -0.006, -0.15), 0)
    m["forward-big"] = ((0, 0, 0), (0.003, -0.002, 0.5), 0)  # rescaleFactor leaves [0.7, 1.4]
    m["yaw"] = ((0, 0.03, 0), (0.06, 0, 0.01), 0)
    m["pitch"] = ((0.03, 0, 0), (0, 0.06, -0.01), 0)
    m["roll"] = ((0, 0, 0.05), (0.05, 0.03, 0), 0)
    m["wide"] = ((0, 0, 0), (0.4, 0.1, 0), 0)
    # the second image shows ANOTHER scene under this pose (the construction of test_line_stereo_status_codes_per_pixel): photometric
    # failures (-3) and ambiguity (-2)
    m["other-scene"] = ((0, 0, 0), (-0.06, 0.05, 0.02), 1)
    # near-zero baseline (0.004, 0.001, 0): its z cancels the t_z the twist adds, so that the composed baseline is the one named and
    # makeAndCheckEPL refuses every pixel (|epl|^2 < 1)
    k = len(m) + 1
    m["tiny"] = ((0, 0, 0), (0.004, 0.001, -TWIST_TZ * (1 + 0.1 * k)), 0)
    return m


MOTIONS = _motions()
NAMES = list(MOTIONS)
TINY = "tiny"


def index_of(name):
    """1-based index of a motion = index of its image in frames(); its frame id is FID0 + index"""
    return NAMES.index(name) + 1


@functools.lru_cache(maxsize=4)
def frames(w, h):
    """(images uint8 [1 + len(MOTIONS), h, w], depth0, K, gt double [.., 7]): image 0 is the keyframe, image k motion k; rendered once
    per size"""
    poses = [(np.eye(3), np.zeros(3))] + [(rot(*r), np.array(c, np.float64)) for r, c, _ in MOTIONS.values()]
    scenes = {0: FreeScene(poses, 0)}
    imgs = np.zeros((len(poses), h, w), np.uint8)
    gt = np.zeros((len(poses), 7))
    depth0 = None
    for i in range(len(poses)):
        s = 0 if i == 0 else list(MOTIONS.values())[i - 1][2]
        sc = scenes.setdefault(s, FreeScene(poses, s))
        imgs[i], d = sc.render(i, w, h)
        if i == 0:
            depth0 = d
        gt[i] = synth.pose7(*sc.frame_to_ref(i, 0))
    for a in (imgs, depth0, gt):
        a.setflags(write=False)
    return imgs, depth0, synth.intrinsics(w, h), gt


def pose_of(oracle, w, h, name):
    """(frame id, Sim3 frame -> keyframe, initialTrackedResidual) of a motion: its pose composed with _ref_pose's general twist"""
    from test_gpu_parity import _ref_pose
    k = index_of(name)
    sim3, itr = _ref_pose(oracle, frames(w, h)[3], k)
    return FID0 + k, sim3, itr


def mask_of(w, h, name):
    """the refPixelWasGood mask a motion's frame carries (9 in 10 set)"""
    return (np.random.default_rng(40 + index_of(name)).uniform(size=(h >> 1, w >> 1)) < 0.9).astype(np.uint8)


def oracle_frame(oracle, w, h, name, parent, L=None, mask=True, fid=None):
    imgs, _, K, _ = frames(w, h)
    f, sim3, itr = pose_of(oracle, w, h, name)
    fo = oracle.Frame(f if fid is None else fid, imgs[index_of(name)], K, L=L)
    fo.set_pose(sim3, parent, itr)
    if mask:
        fo.set_wasgood(mask_of(w, h, name))
    return fo


def noisy_map(oracle, w, h, params=None, L=None, seed=1, hyp=None, reactivated=False):
    """(keyframe, map, state): the keyframe with its ground-truth depth and a map holding test_gpu_parity._noisy_hyp's ragged state (or
    `hyp`) — on the oracle, or with L on the reference library"""
    from test_gpu_parity import _noisy_hyp
    imgs, depth0, K, _ = frames(w, h)
    kf = oracle.Frame(0, imgs[0], K, L=L)
    kf.set_depth_gt(depth0)
    dm = oracle.DepthMap(w, h, K, params=params, L=L)
    dm.init_gt(kf)
    if hyp is None:
        hyp = _noisy_hyp(dm.get(), 0.1, seed)
    dm.set(kf, hyp, reactivated=reactivated)
    kf.set_counters(7, 3, 3, 0)
    return kf, dm, hyp


def search_intervals(hyp):
    """(min, prior, max) inverse depth doLineStereo gets per pixel, as float32 planes: observeDepthUpdate's for a valid hypothesis (formed
    in float32, as there), observeDepthCreate's otherwise"""
    v = hyp["isValid"] > 0
    two = np.float32(STEREO_EPL_VAR_FAC)
    ids = hyp["idepth_smoothed"].astype(np.float32)
    with np.errstate(invalid="ignore"):
        sv = np.sqrt(hyp["idepth_var_smoothed"].astype(np.float64)).astype(np.float32)
        lo = np.maximum(ids - sv * two, np.float32(0))
        hi = np.minimum(ids + sv * two, np.float32(1 / MIN_DEPTH))
    one = np.float32(1)
    return (np.where(v, lo, np.float32(0)).astype(np.float32), np.where(v, ids, one).astype(np.float32),
            np.where(v, hi, np.float32(1 / MIN_DEPTH)).astype(np.float32))


def lattice(w, h, step=3):
    """interior pixels, every `step`-th in both axes (odd rows shifted by one); step 1: every interior pixel"""
    return [(x, y) for y in range(3, h - 3, step) for x in range(3 + (y // step) % 2, w - 3, step)]


def code_of(a):
    """line_stereo's 7 floats -> 0 makeAndCheckEPL refused, 1 a match, or the status code -1 ... -4"""
    if not a[0]:
        return 0
    return int(a[3]) if a[3] < 0 else 1


CLASSES = ("incx+", "incx-", "incy+", "incy-", "x-dominant", "y-dominant", "pClose-reclamp", "epl-long", "epl-pad",
           "clip-left", "clip-right", "clip-top", "clip-bottom", "stencil-off", "rescale-out", "pFar-outside", "clipped-short",
           "epipole-inside")


def census(K, w, h, hyp, pose, params, image=None, max_grad=None):
    """Which branches of makeAndCheckEPL / doLineStereo the pixels of a map reach under `pose` (Sim3 frame -> keyframe, 8 doubles), in
    float64, with the search interval of observeDepthCreate (no hypothesis) / observeDepthUpdate (a valid one).  A CLASSIFICATION of the
    inputs, never an expected value: near a threshold float64 and the float32 code may disagree on a pixel.

    Pixels counted: inside the 3-pixel border, not blacklisted below MIN_BLACKLIST, |epl|^2 >= 1; with max_grad, at or above
    params.minUseGrad; with image (the keyframe's level 0), past makeAndCheckEPL's two gradient tests.  (Scheduled skips and tracking
    masks belong to a call, not to the geometry: not applied.)  Each class is counted at the statement that takes the branch, so e.g. a
    clip is counted although the clipped segment may then be refused as too short.

    Returns {"counts": {class: n}, "masks": {class: bool [h, w]}, "candidates": bool [h, w], "searched": bool [h, w] (reach the walk),
    "reads": (xmin, xmax, ymin, ymax) integer tap coordinates the device's walk touches, one entry per searched pixel in row-major
    order, "steps": the walk's step count per searched pixel}."""
    fx, fy, cx, cy = [float(v) for v in K]
    Km = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    fxi, fyi = 1 / fx, 1 / fy
    cxi, cyi = -cx / fx, -cy / fy
    pose = np.asarray(pose, np.float64)
    q = pose[:4] / np.linalg.norm(pose[:4])
    qw, qx, qy, qz = q
    R = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                  [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                  [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])
    s = float(pose[7]) if len(pose) > 7 else 1.0
    t = pose[4:7]                                   # thisToOther_t: the second camera's centre in the keyframe
    Rinv, sinv = R.T, 1.0 / s
    tinv = -(Rinv @ t) * sinv                       # otherToThis_t
    KR = (Km @ Rinv) * sinv                         # K_otherToThis_R
    Kt = Km @ tinv                                  # K_otherToThis_t

    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    inside = np.zeros((h, w), bool)
    inside[3:h - 3, 3:w - 3] = True
    cand = inside & (hyp["blacklisted"] >= MIN_BLACKLIST)
    if max_grad is not None:
        cand &= max_grad >= params.minUseGrad
    # makeAndCheckEPL
    epx = -fx * t[0] + t[2] * (x - cx)
    epy = -fy * t[1] + t[2] * (y - cy)
    len2 = epx * epx + epy * epy
    cand &= len2 >= MIN_EPL_LENGTH_SQUARED
    if image is not None:
        img = np.asarray(image, np.float64)
        gx = np.zeros((h, w))
        gy = np.zeros((h, w))
        gx[:, 1:-1] = img[:, 2:] - img[:, :-2]
        gy[1:-1, :] = img[2:, :] - img[:-2, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            eg = (gx * epx + gy * epy) ** 2 / len2
            cand &= (eg >= MIN_EPL_GRAD_SQUARED) & (eg / (gx * gx + gy * gy) >= MIN_EPL_ANGLE_SQUARED)
    masks = {k: np.zeros((h, w), bool) for k in CLASSES}
    with np.errstate(divide="ignore", invalid="ignore"):
        ln = np.sqrt(len2)
        epxn, epyn = epx / ln, epy / ln
        # search interval
        valid = hyp["isValid"] > 0
        ids = hyp["idepth_smoothed"].astype(np.float64)
        sv = np.sqrt(np.maximum(hyp["idepth_var_smoothed"].astype(np.float64), 0))
        lo = np.where(valid, np.maximum(ids - STEREO_EPL_VAR_FAC * sv, 0.0), 0.0)
        hi = np.where(valid, np.minimum(ids + STEREO_EPL_VAR_FAC * sv, 1 / MIN_DEPTH), 1 / MIN_DEPTH)
        prior = np.where(valid, ids, 1.0)
        # doLineStereo up to the walk
        k0, k1 = fxi * x + cxi, fyi * y + cyi
        pInf = [KR[i, 0] * k0 + KR[i, 1] * k1 + KR[i, 2] for i in range(3)]
        rescale = (pInf[2] / prior + Kt[2]) * prior
        fX, fY, lX, lY = x - 2 * epxn * rescale, y - 2 * epyn * rescale, x + 2 * epxn * rescale, y + 2 * epyn * rescale
        off = (fX <= 0) | (fX >= w - 2) | (fY <= 0) | (fY >= h - 2) | (lX <= 0) | (lX >= w - 2) | (lY <= 0) | (lY >= h - 2)
        masks["stencil-off"] = cand & off
        live = cand & ~off
        bad = ~((rescale > 0.7) & (rescale < 1.4))
        masks["rescale-out"] = live & bad
        live = live & ~bad
        pC = [pInf[i] + Kt[i] * hi for i in range(3)]
        re = pC[2] < 0.001
        masks["pClose-reclamp"] = live & re
        hi2 = np.where(re, (0.001 - pInf[2]) / Kt[2], hi)
        pC = [pInf[i] + Kt[i] * hi2 for i in range(3)]
        pC0, pC1 = pC[0] / pC[2], pC[1] / pC[2]
        pF = [pInf[i] + Kt[i] * lo for i in range(3)]
        live = live & ~((pF[2] < 0.001) | (hi2 < lo))
        pF0, pF1 = pF[0] / pF[2], pF[1] / pF[2]
        incx, incy = pC0 - pF0, pC1 - pF1
        el = np.sqrt(incx * incx + incy * incy)
        live = live & np.isfinite(el) & (el > 0)                       # (-4 otherwise)
        long_ = el > MAX_EPL_LENGTH_CROP
        masks["epl-long"] = live & long_
        pC0 = np.where(long_, pF0 + incx * MAX_EPL_LENGTH_CROP / el, pC0)
        pC1 = np.where(long_, pF1 + incy * MAX_EPL_LENGTH_CROP / el, pC1)
        incx, incy = incx / el, incy / el
        pF0, pF1, pC0, pC1 = pF0 - incx, pF1 - incy, pC0 + incx, pC1 + incy
        short = el < MIN_EPL_LENGTH_CROP
        masks["epl-pad"] = live & short
        pad = np.where(short, (MIN_EPL_LENGTH_CROP - el) / 2, 0.0)
        pF0, pF1, pC0, pC1 = pF0 - incx * pad, pF1 - incy * pad, pC0 + incx * pad, pC1 + incy * pad
        B = SAMPLE_POINT_TO_BORDER

        def outside(a0, a1):
            return (a0 <= B) | (a0 >= w - B) | (a1 <= B) | (a1 >= h - B)

        fo = outside(pF0, pF1)
        masks["pFar-outside"] = live & fo
        live = live & ~fo
        clip = outside(pC0, pC1)
        cl, cr = clip & (pC0 <= B), clip & ~(pC0 <= B) & (pC0 >= w - B)
        masks["clip-left"], masks["clip-right"] = live & cl, live & cr
        add = np.where(cl, (B - pC0) / incx, np.where(cr, (w - B - pC0) / incx, 0.0))
        pC0, pC1 = pC0 + add * incx, pC1 + add * incy
        ct, cb = clip & (pC1 <= B), clip & ~(pC1 <= B) & (pC1 >= h - B)
        masks["clip-top"], masks["clip-bottom"] = live & ct, live & cb
        add = np.where(ct, (B - pC1) / incy, np.where(cb, (h - B - pC1) / incy, 0.0))
        pC0, pC1 = pC0 + add * incx, pC1 + add * incy
        nl = np.sqrt((pC0 - pF0) ** 2 + (pC1 - pF1) ** 2)
        refused = clip & (outside(pC0, pC1) | (nl < 8.0) | ~np.isfinite(nl))
        masks["clipped-short"] = live & refused
        live = live & ~refused
        # the walk: positions pFar + k inc while strictly before pClose in both axes, one step at the least
        nx = np.where(incx != 0, np.ceil((pC0 - pF0) / incx), np.where(pF0 <= pC0, np.inf, 0.0))
        ny = np.where(incy != 0, np.ceil((pC1 - pF1) / incy), np.where(pF1 <= pC1, np.inf, 0.0))
        steps = np.clip(np.nan_to_num(np.minimum(nx, ny), nan=1.0, posinf=1000.0), 1, 1000)
    masks["incx+"], masks["incx-"] = live & (incx >= 0), live & (incx < 0)
    masks["incy+"], masks["incy-"] = live & (incy >= 0), live & (incy < 0)
    xd = incx * incx > incy * incy
    masks["x-dominant"], masks["y-dominant"] = live & xd, live & ~xd
    # the epipoles: where the baseline meets the keyframe's image plane and the second camera's
    ep_in = False
    if abs(t[2]) > 1e-12 and abs(tinv[2]) > 1e-12:
        e_kf = (fx * t[0] / t[2] + cx, fy * t[1] / t[2] + cy)
        e_ref = (Kt[0] / Kt[2], Kt[1] / Kt[2])
        ep_in = all(0 <= e[0] <= w - 1 and 0 <= e[1] <= h - 1 for e in (e_kf, e_ref))
    masks["epipole-inside"] = live if ep_in else np.zeros((h, w), bool)
    # what the device's walk reads (integer taps, the bilinear + 1 included)
    sx0, sy0 = (pF0 - WALK_BEHIND * incx)[live], (pF1 - WALK_BEHIND * incy)[live]
    n = steps[live]
    ex0, ey0 = pF0[live] + (n - 1 + WALK_AHEAD) * incx[live], pF1[live] + (n - 1 + WALK_AHEAD) * incy[live]
    reads = (np.minimum(np.trunc(sx0), np.trunc(ex0)).astype(np.int64), np.maximum(np.trunc(sx0), np.trunc(ex0)).astype(np.int64) + 1,
             np.minimum(np.trunc(sy0), np.trunc(ey0)).astype(np.int64), np.maximum(np.trunc(sy0), np.trunc(ey0)).astype(np.int64) + 1)
    return {"counts": {k: int(v.sum()) for k, v in masks.items()}, "masks": masks, "candidates": cand, "searched": live, "reads": reads,
            "steps": n.astype(np.int64)}


def classes_at(c, x, y):
    """the census classes pixel (x, y) falls in (for naming a differing pixel)"""
    return [k for k in CLASSES if c["masks"][k][y, x]]


def census_table(rows):
    """rows: [(motion, census counts, searched)] -> the table the CPU test prints"""
    short = ("ix+", "ix-", "iy+", "iy-", "xdom", "ydom", "recl", "long", "pad", "cL", "cR", "cT", "cB", "sten", "resc", "pFar", "c<8", "epi")
    out = ["%-12s %6s " % ("motion", "walk") + " ".join("%5s" % s for s in short)]
    for name, counts, searched in rows:
        out.append("%-12s %6d " % (name, searched) + " ".join("%5d" % counts[k] for k in CLASSES))
    return "\n".join(out)
