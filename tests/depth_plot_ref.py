"""numpy restatement of the depth map's debug image — DepthMap::debugPlotDepthMap (C/DepthEstimation/DepthMap.cpp:1400-1428) with
DepthMapPixelHypothesis::getVisualizationColor (DepthMapPixelHypothesis.cpp:29-90) — with every intermediate in the reference's type:
float32 products, the double promotions where the reference's constants are double, the logarithm of modes 3 / 4 in double.
tests/test_depth_plot_ref_cpu.py pins it to the reference's own compiled function, to a committed fixture of that function's output
and to plotDepthMap of include/lsd_slam_hip_io.hpp; tests/test_depth_plot_gpu.py holds the device image to it.
Also the hypotheses and maps those files use, and the ctypes call into the reference's function."""
import ctypes
import math

import numpy as np

from lsd_slam_amd.capi import HYP_DTYPE

F = np.float32
MIN_BLACKLIST = -1            # C/util/settings.h:66
MODES = (0, 1, 2, 3, 4, 5)    # debugDisplay values with a colour scheme; any other value paints white
WHITE_MODE = 6

PLANTED_IDEPTH = [0.0, -0.0, 1.0, 2.0, 3.0, -1e-30]
PLANTED_VAR = [1.0, 0.01, 1e-6, 0.0, 10.0, 100.0]


def _log10(x):
    """log10 of a float64 array through the C library (what the reference's build calls), -inf at 0, nan below"""
    flat = np.asarray(x, np.float64).reshape(-1)
    out = np.array([math.log10(v) if v > 0 and v != math.inf else (-math.inf if v == 0 else (math.inf if v > 0 else math.nan)) for v in flat.tolist()],
                   np.float64)
    return out.reshape(np.shape(x))


def _clamp_byte(f):
    """uchar v = f < 0 ? 0 : (f > 255 ? 255 : f): clamp, then truncate"""
    with np.errstate(invalid="ignore"):
        return np.where(~(f > 0), 0, np.where(f > 255, 255, np.trunc(np.where(np.isfinite(f), f, 0)))).astype(np.uint8)


def color_ref(hyp, mode, last_frame_id, log_scale=1.0):
    """getVisualizationColor for every hypothesis of `hyp` (HYP_DTYPE, any shape) -> uint8 [..., 3] in cv::Vec3b order.
    log_scale multiplies the double logarithm of modes 3 / 4 (the condition test of test_depth_plot_ref_cpu.py)."""
    out = np.full(hyp.shape + (3,), 255, np.uint8)
    with np.errstate(all="ignore"):
        if mode in (0, 1):
            idp = hyp["idepth_smoothed" if mode == 0 else "idepth"].astype(F)
            ok = idp >= 0
            for k in range(3):
                r = np.abs((F(k) - idp) * F(255))               # float32 throughout; "/ 1.0" is exact
                out[..., k] = np.where(ok, 255 - _clamp_byte(r).astype(np.int32), 255).astype(np.uint8)
        elif mode == 2:
            f = (hyp["validity_counter"].astype(np.float64) * (255.0 / float(F(250.0) + F(5.0)))).astype(F)
            v = _clamp_byte(f)
            out[..., 0] = 0
            out[..., 1] = v
            out[..., 2] = v
        elif mode in (3, 4):
            idv = hyp["idepth_var_smoothed" if mode == 3 else "idepth_var"].astype(F)
            var = (-0.5 * (_log10(idv.astype(np.float64)) * log_scale)).astype(F)
            var = ((var * F(255)).astype(np.float64) * 0.333).astype(F)
            var = np.where(var > 255, F(255), var)
            ok = var >= 0
            safe = np.where(ok, var, F(0))
            out[..., 0] = np.where(ok, np.trunc(F(255) - safe), 0).astype(np.uint8)
            out[..., 1] = np.where(ok, np.trunc(safe), 0).astype(np.uint8)
            out[..., 2] = np.where(ok, 0, 255).astype(np.uint8)
        elif mode == 5:
            f = ((hyp["nextStereoFrameMinID"].astype(F) - F(last_frame_id)).astype(np.float64) * (255.0 / 100)).astype(F)
            v = _clamp_byte(f)
            out[..., 0] = v
            out[..., 1] = 0
            out[..., 2] = v
    return out


def plot_ref(hyp, image, mode, ref_id, log_scale=1.0):
    """debugPlotDepthMap: hyp HYP_DTYPE [h, w], image float32 [h, w] (the keyframe's level-0 image) -> uint8 [h, w, 3]"""
    grey = np.clip(np.rint(image.astype(F)), 0, 255).astype(np.uint8)      # convertTo(CV_8UC1): to nearest even, saturated
    out = np.repeat(grey[..., None], 3, axis=2)
    if mode == 2:
        out[hyp["blacklisted"] < MIN_BLACKLIST] = (0, 0, 255)
    valid = hyp["isValid"] != 0
    out[valid] = color_ref(hyp[valid], mode, ref_id, log_scale)
    return out


def log_condition_holds(hyp, image, ref_id=0):
    """Modes 3 / 4 with the double logarithm scaled by (1 +- 2^-44) give the image of the exact one: on such inputs a logarithm a few
    ulps off cannot be told from the correctly rounded one, so an implementation with another log10 can still be asked for equality."""
    for mode in (3, 4):
        exact = plot_ref(hyp, image, mode, ref_id)
        for s in (1.0 + 2.0 ** -44, 1.0 - 2.0 ** -44):
            if not np.array_equal(plot_ref(hyp, image, mode, ref_id, log_scale=s), exact):
                return False
    return True


def _plant(hyp_flat, rng):
    """the planted idepths and variances, each on a few random entries of the flat array (both the raw and the smoothed field)"""
    n = len(hyp_flat)
    for v in PLANTED_IDEPTH:
        i = rng.integers(0, n, 6)
        hyp_flat["idepth"][i] = F(v)
        hyp_flat["idepth_smoothed"][i] = F(v)
    for v in PLANTED_VAR:
        i = rng.integers(0, n, 6)
        hyp_flat["idepth_var"][i] = F(v)
        hyp_flat["idepth_var_smoothed"][i] = F(v)
    return hyp_flat


def random_hypotheses(n, seed, last_frame_id, min_counter=-5):
    """n hypotheses: idepth in [-0.3, 3], variances log-uniform over 1e-7 .. 10, counters min_counter .. 300, next-stereo frame ids
    within +-150 of last_frame_id (half of them whole numbers, as k_observe writes them, half with a fraction), blacklist 0 .. -2, all
    valid; plus the planted values"""
    rng = np.random.default_rng(seed)
    h = np.zeros(n, HYP_DTYPE)
    h["isValid"] = 1
    h["blacklisted"] = rng.integers(-2, 1, n)
    nid = last_frame_id + rng.uniform(-150, 150, n)
    h["nextStereoFrameMinID"] = np.where(rng.random(n) < 0.5, np.rint(nid), nid).astype(F)
    h["validity_counter"] = rng.integers(min_counter, 301, n)
    h["idepth"] = rng.uniform(-0.3, 3, n).astype(F)
    h["idepth_smoothed"] = rng.uniform(-0.3, 3, n).astype(F)
    h["idepth_var"] = (10.0 ** rng.uniform(-7, 1, n)).astype(F)
    h["idepth_var_smoothed"] = (10.0 ** rng.uniform(-7, 1, n)).astype(F)
    return _plant(h, rng)


def make_map(w, h, seed, valid_fraction=0.35, last_frame_id=0):
    """a [h, w] map for the whole-image tests: about 35 % valid pixels, counters >= 0 (lsdhip_depth_upload takes no valid pixel with a
    negative one), blacklist values 0, -1, -2 on valid and on invalid pixels, the planted values on valid pixels"""
    rng = np.random.default_rng(seed)
    m = random_hypotheses(w * h, seed + 1, last_frame_id, min_counter=0)
    m["isValid"] = rng.random(w * h) < valid_fraction
    # planted values again, on valid pixels only (the ones random_hypotheses planted may have become invalid)
    valid_idx = np.flatnonzero(m["isValid"])
    for v in PLANTED_IDEPTH:
        i = valid_idx[rng.integers(0, len(valid_idx), 4)]
        m["idepth"][i] = F(v)
        m["idepth_smoothed"][i] = F(v)
    for v in PLANTED_VAR:
        i = valid_idx[rng.integers(0, len(valid_idx), 4)]
        m["idepth_var"][i] = F(v)
        m["idepth_var_smoothed"][i] = F(v)
    m = m.reshape(h, w)
    for b in (0, -1, -2):
        for val in (0, 1):
            assert ((m["blacklisted"] == b) & (m["isValid"] == val)).any()
    return m


# the maps of tests/test_depth_plot_gpu.py: stated here, so that tests/test_depth_plot_ref_cpu.py can check the condition on them
GPU_SIZES = [(160, 128), (176, 144), (640, 480)]   # 20 full 1024-pixel chunks; rows straddle chunks and the last one is ragged; 300 chunks
GPU_BATCH_SIZE = (160, 128)
GPU_BATCH_MAPS = 33


def gpu_map(w, h, k=0, last_frame_id=0):
    """map k of size w x h of the GPU tests"""
    return make_map(w, h, w * 1000 + h + 17 * k, last_frame_id=last_frame_id)


# ---- the reference's own function (oracle/_ref/liblsd_ref_sse.so) ----------------------------------------------------------------------
REF_COLOR_SYMBOL = "_ZNK8lsd_slam23DepthMapPixelHypothesis21getVisualizationColorEi"    # getVisualizationColor(int) const
REF_DISPLAY_SYMBOL = "_ZN8lsd_slam12debugDisplayE"                                      # int lsd_slam::debugDisplay


def reference_colors(lib_path, hyp, mode, last_frame_id):
    """lsd_slam::DepthMapPixelHypothesis::getVisualizationColor(last_frame_id) of the compiled reference on every 32-byte record of `hyp`
    (1-D, HYP_DTYPE) with lsd_slam::debugDisplay = mode.  The cv::Vec3b comes back in the integer return register."""
    L = ctypes.CDLL(lib_path)
    fn = getattr(L, REF_COLOR_SYMBOL)
    fn.restype = ctypes.c_uint32
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int]
    display = ctypes.c_int.in_dll(L, REF_DISPLAY_SYMBOL)
    hyp = np.ascontiguousarray(hyp, HYP_DTYPE)
    assert hyp.ndim == 1
    before = display.value
    display.value = mode
    try:
        base = hyp.ctypes.data
        raw = np.array([fn(base + 32 * i, last_frame_id) for i in range(len(hyp))], np.uint32)
    finally:
        display.value = before
    return np.stack([raw & 0xFF, (raw >> 8) & 0xFF, (raw >> 16) & 0xFF], axis=1).astype(np.uint8)
