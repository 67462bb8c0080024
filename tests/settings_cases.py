"""Named profiles of the run-time settings the reference lets a user tune live (util/settings.cpp:77-88, cfg/LSDParams.cfg:13-17,34,
written by IOWrapper/ROS/rosReconfigure.h:84-91), as dicts for hip.Context(..., params=) and, through test_gpu_parity.oracle_params, for
the oracle.  Values are float32; the pixel noise is squared in double and then cast, as rosReconfigure.h:90 does.

A test that moves a setting also runs the oracle at the defaults and asserts through differs() that the setting bit: a test in which
neither side reads the value would pass otherwise."""
import numpy as np

f32 = np.float32


def _noise2(sigma):
    return float(f32(np.float64(sigma) * np.float64(sigma)))


def _f(v):
    return float(f32(v))


PROFILES = {
    # what live_slam runs: the cfg's defaults are settings.cpp's pair of keyframe weights swapped, and affine lighting off
    "ros": {"KFUsageWeight": _f(4), "KFDistWeight": _f(3), "useAffineLightningEstimation": 0},
    "noisy-camera": {"minUseGrad": _f(7.3), "cameraPixelNoise2": _noise2(6.5)},
    "clean-camera": {"minUseGrad": _f(2.5), "cameraPixelNoise2": _noise2(2.3)},
    "smooth-more": {"depthSmoothingFactor": _f(0.37)},
    "smooth-less": {"depthSmoothingFactor": _f(2.6)},
    "smooth-zero": {"depthSmoothingFactor": _f(0.0)},      # the cfg's minimum: every distance term of the 5x5 window is zero
    "kf-weights": {"KFDistWeight": _f(2.7), "KFUsageWeight": _f(5.1)},
    "kf-dist-zero": {"KFDistWeight": _f(0.0)},            # the cfg's minimum: maxScore / KFDistWeight^2 is an infinite distance threshold
}
CAMERA = ("noisy-camera", "clean-camera")
SMOOTHING = ("smooth-more", "smooth-less", "smooth-zero")
KF_WEIGHTS = ("ros", "kf-weights", "kf-dist-zero")
DEPTH_MAP = ("ros",) + CAMERA + SMOOTHING           # every profile except the two that move the keyframe weights alone

FLOAT_PLANES = ("idepth", "idepth_var", "idepth_smoothed", "idepth_var_smoothed")


def differs(a, b):
    """{"isValid": number of validity flags that differ, plane: number of float bit patterns that differ where both maps hold a
    hypothesis} of two downloaded maps"""
    va, vb = a["isValid"] > 0, b["isValid"] > 0
    both = va & vb
    out = {"isValid": int((va != vb).sum())}
    for k in FLOAT_PLANES:
        x = np.ascontiguousarray(a[k], dtype=np.float32).view(np.uint32)
        y = np.ascontiguousarray(b[k], dtype=np.float32).view(np.uint32)
        out[k] = int(((x != y) & both).sum())
    return out


def params_of(name):
    return {} if name == "defaults" else PROFILES[name]


def oracle_params(oracle, name):
    """the oracle's parameter block of a profile ("defaults": no override)"""
    op = oracle.default_params()
    for k, v in params_of(name).items():
        setattr(op, k, v)
    return op


# ---- the oracle alone on the depth-map sequence of test_gpu_parity.test_depth_stages_bit_exact, once per profile -------------------------
W, H = 176, 144                     # partial 32-wide tiles, an odd level-4 width
N_FRAMES, REF_IDS = 8, (3, 4, 6, 7)
STAGES = ("observe", "fillholes", "regularize", "regularize_occ", "observe2")
_DEPTH_RUNS = {}


def oracle_depth_stages(oracle, name):
    """{"init_valid": hypotheses initializeFromGTDepth makes, stage: the map behind it} of the oracle at profile `name` from the ragged
    state of test_gpu_parity._noisy_map with reference frames REF_IDS: the inputs of the device tests, so that their counts of what a
    moved setting changes can be checked without a GPU"""
    if name in _DEPTH_RUNS:
        return _DEPTH_RUNS[name]
    from common import sequence
    from test_gpu_parity import _noisy_hyp, _ref_pose
    frames, depth0, K, gt = sequence(W, H, N_FRAMES)
    op = oracle_params(oracle, name)
    kf = oracle.Frame(0, frames[0], K)
    kf.set_depth_gt(depth0, minUseGrad=op.minUseGrad)
    dm = oracle.DepthMap(W, H, K, params=op)
    dm.init_gt(kf)
    out = {"init_valid": int((dm.get()["isValid"] > 0).sum())}
    dm.set(kf, _noisy_hyp(dm.get()))
    kf.set_counters(7, 3, 3, 0)
    rng = np.random.default_rng(5)
    fos = []
    for i in REF_IDS:
        fo = oracle.Frame(i, frames[i], K)
        sim3, itr = _ref_pose(oracle, gt, i)
        fo.set_pose(sim3, kf, itr)
        fo.set_wasgood((rng.uniform(size=(H >> 1, W >> 1)) < 0.9).astype(np.uint8))
        fos.append(fo)
    for stage in STAGES:
        if stage.startswith("observe"):
            dm.stage("observe", fos if stage == "observe" else fos[1:])
        else:
            dm.stage(stage)
        out[stage] = dm.get()
    _DEPTH_RUNS[name] = out
    return out


# what a moved setting must change against the default-settings oracle run, at the least (measured on the CPU with the oracle alone: each
# floor is a quarter or less of the count; tests/test_settings_cpu.py holds them)
MIN_FLOAT_PATTERNS, MIN_VALIDITY_FLAGS = 1000, 100


def assert_depth_setting_bit(name, run, default):
    """run / default: oracle_depth_stages of the profile and of the defaults"""
    p = params_of(name)
    d_obs, d_fill, d_reg = [differs(run[s], default[s]) for s in ("observe", "fillholes", "regularize")]
    if "cameraPixelNoise2" in p:
        assert d_obs["idepth"] >= MIN_FLOAT_PATTERNS, (name, d_obs)
    if "minUseGrad" in p:
        assert d_obs["isValid"] >= MIN_VALIDITY_FLAGS, (name, d_obs)
        assert run["init_valid"] != default["init_valid"], name
    if "depthSmoothingFactor" in p:
        assert not any(d_obs.values()) and not any(d_fill.values()), (name, d_obs, d_fill)      # nothing before the regulariser, as it must be
        assert d_reg["idepth_smoothed"] >= MIN_FLOAT_PATTERNS, (name, d_reg)
        assert d_reg["isValid"] == 0 and np.all(np.isfinite(run["regularize"]["idepth_smoothed"][run["regularize"]["isValid"] > 0])), name
    return d_obs, d_reg


def se3_noise_moves_the_weighted_error(oracle, w, h, K, job, S, bound):
    """the tracking tests' analogue of differs(): `job` = (oracle reference, oracle frame, pose, level, a, b) evaluated at a moved
    cameraPixelNoise2 gave the float64 sums S; the same evaluation at the default settings must give a weighted error further away than
    10 x the tolerance the device is held to (`bound`), or a device that read 16 would pass"""
    from se3_terms import point_terms, sums64
    ro, fo, T, lvl, a, b = job
    tro = oracle.SE3Tracker(w, h, K, mode=oracle.SSE_EXACT_RCP)
    tro.evaluate(ro, fo, T, lvl, a, b)
    S0 = sums64(point_terms(tro, fo, lvl, T))
    gap = abs(S["werr"] - S0["werr"])
    assert gap > 10 * bound, (lvl, S["werr"], S0["werr"], bound)
    return gap / bound
