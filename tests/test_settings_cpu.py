"""The settings profiles of tests/settings_cases.py without a GPU: what tests/test_settings_gpu.py relies on.

  * every moved setting changes what the oracle computes on the device tests' own inputs, by the floors those tests state (a test in which
    neither side reads a value would pass otherwise): the depth-map stages, the SE3 weighted error, the re-position prefilter;
  * the designed sheets of tests/reg_cases.py rebuilt for the moved thresholds: the oracle decides every pixel as the census predicts;
  * keyframeScore (include/lsd_slam_hip_loop.hpp) with explicit weights, as float32 bits against the reference's statement
    (TrackableKeyFrameSearch.h:75-79)."""
import numpy as np
import pytest

import reg_cases as rc
import reposition_ref as rr
import settings_cases as sc
from test_loop_rules_cpu import bits, exe, run  # noqa: F401  (exe: the fixture that compiles tests/cpp/loop_rules_test.cpp)
from test_reg_cases_cpu import oracle_decides_as_the_census_predicts

f32 = np.float32


def test_profiles_are_float32_and_square_the_noise_in_double():
    for name, p in sc.PROFILES.items():
        for k, v in p.items():
            assert float(f32(v)) == v, (name, k)
    assert sc.PROFILES["noisy-camera"]["cameraPixelNoise2"] == float(f32(6.5 * 6.5)) == 42.25
    assert sc.PROFILES["clean-camera"]["cameraPixelNoise2"] == float(f32(np.float64(2.3) * np.float64(2.3)))
    assert set(sc.DEPTH_MAP) | {"kf-weights", "kf-dist-zero"} == set(sc.PROFILES)
    for name in sc.CAMERA:
        assert rc.GRAD_LOW < sc.PROFILES[name]["minUseGrad"] < rc.GRAD_HIGH


def test_differs_counts_flags_and_bit_patterns():
    a = np.zeros((2, 3), rc.HYP_DTYPE)
    a["isValid"] = 1
    b = a.copy()
    assert not any(sc.differs(a, b).values())
    b["isValid"][0, 0] = 0
    b["idepth"][0, 0] = 3.0           # not counted: one side holds no hypothesis there
    b["idepth"][1, 1] = np.nextafter(f32(0), f32(1))
    b["idepth_smoothed"][1, 2] = -0.0      # a bit pattern, not a value
    d = sc.differs(a, b)
    assert d == {"isValid": 1, "idepth": 1, "idepth_var": 0, "idepth_smoothed": 1, "idepth_var_smoothed": 0}


@pytest.mark.parametrize("name", sc.DEPTH_MAP)
def test_depth_map_settings_bite(oracle, name):
    run_, default = sc.oracle_depth_stages(oracle, name), sc.oracle_depth_stages(oracle, "defaults")
    d_obs, d_reg = sc.assert_depth_setting_bit(name, run_, default)
    print("%s against the defaults: after observe %r; after regularize %r; initializeFromGTDepth %d valid (defaults %d)"
          % (name, d_obs, d_reg, run_["init_valid"], default["init_valid"]))
    if name == "ros":        # the keyframe weights and the affine switch are not the depth map's
        assert not any(d_obs.values()) and not any(d_reg.values())


@pytest.mark.parametrize("name", sc.CAMERA)
def test_se3_noise_moves_the_weighted_error_beyond_the_tolerance(oracle, name):
    """at 176x144, levels 3 .. 1, the first pose and keyframe kind of test_track_batch_eval_gpu's jobs: the bound is the widest that file
    ever uses at the level (the small-batch form's depth)"""
    from common import sequence
    from se3_terms import EPS, point_terms, sums64
    from test_track_batch_eval_gpu import C_TERM, depth_of
    w, h = sc.W, sc.H
    frames, depth0, K, gt = sequence(w, h, 4, 0)
    op = sc.oracle_params(oracle, name)
    kf = oracle.Frame(0, frames[0], K)
    kf.set_depth_gt(depth0, minUseGrad=op.minUseGrad)
    ro = oracle.TrackingReference()
    ro.import_frame(kf)
    tro = oracle.SE3Tracker(w, h, K, params=op, mode=oracle.SSE_EXACT_RCP)
    T = oracle.se3_inv(gt[3]).astype(np.float32)
    for lvl in (3, 2, 1):
        fo = oracle.Frame(1, frames[1], K)
        tro.evaluate(ro, fo, T, lvl, 1.03, -2.5)
        S = sums64(point_terms(tro, fo, lvl, T))
        bound = (depth_of("small", (w >> lvl) * (h >> lvl), 0) + 1 + C_TERM["werr"]) * EPS * S["werr_abs"] + 1e-30
        ratio = sc.se3_noise_moves_the_weighted_error(oracle, w, h, K, (ro, fo, T, lvl, 1.03, -2.5), S, bound)
        print("%s level %d: the weighted error moves by %.0f x the tolerance" % (name, lvl, ratio))


# ---- re-position search --------------------------------------------------------------------------------------------------------------
_SEARCH = {}


def reposition_search(oracle, name):
    """scenario A of tests/reposition_ref.py restated over the oracle at a profile's keyframe weights (once per process)"""
    if name not in _SEARCH:
        K, kfs, frame, pose = rr.scenario_a_oracle(oracle)
        op = sc.oracle_params(oracle, name)
        tracker = oracle.SE3Tracker(rr.W, rr.H, K, params=op, mode=oracle.SSE_EXACT_RCP)
        _SEARCH[name] = rr.search(oracle, tracker, kfs, frame, pose, kfs[rr.PARENT_SLOT]["id"], rr.W, rr.H, K, params=op)
    return _SEARCH[name]


def assert_weights_bite(name, run_, default):
    """the prefilter and the scores of a profile against those at the default weights"""
    (_, recs, counts), (_, recs0, counts0) = run_, default
    far, far0 = [r["slot"] for r in recs if r["stage"] == "far"], [r["slot"] for r in recs0 if r["stage"] == "far"]
    assert far0, "the default weights leave no keyframe beyond the distance threshold"
    if name == "kf-dist-zero":
        assert np.isinf(counts["distanceTH"]) and far == []           # every banked keyframe is admitted
    if name in ("kf-weights", "kf-dist-zero"):
        assert len(far) != len(far0), (name, far, far0)
        assert counts["potential"] != counts0["potential"], (name, counts["potential"])
    scored = [(r["slot"], bits(r["score"])) for r in recs if "score" in r]
    scored0 = dict((r["slot"], bits(r["score"])) for r in recs0 if "score" in r)
    assert any(s in scored0 and b != scored0[s] for s, b in scored), name
    return len(far), len(far0)


def assert_scenario_margins(recs, counts):
    """A condition on scenario A at moved weights, so that a device that agrees with the oracle to the permaref tolerances (usage rel 1e-5,
    poses 2e-3) must take the same branches: rr.census's margins for the distance, the score and the pose discrepancy.  The moved weights
    bring more keyframes to the acceptance test, some closer to its thresholds than the 0.05 / 0.01 the default scenario was designed
    for; here goodVal must stay 0.02 from 0.7 and newScore 0.005 from the running best.  goodVal = usage x good / (good + bad): usage
    agrees to 1e-5 and the counts are integers over ~1500 points that can differ only for points within rounding of the isGood test,
    far below 0.02.  newScore's distance term moves by at most 2 |d| (2e-3 meanIdepth) KFDistWeight^2 = 2 x 0.1 x 1e-3 x 16 = 3.2e-3
    for a pose within 2e-3, its usage term by 1e-5 relative."""
    reached, bad = rr.census(recs, counts)
    for b in bad:
        if b[1] == "goodVal":
            assert abs(b[2] - 0.7) >= 0.02, b
        elif b[1] == "newScore":
            assert abs(b[2] - b[3]) >= 0.005, b
        else:
            raise AssertionError(b)
    return reached


@pytest.mark.parametrize("name", sc.KF_WEIGHTS)
def test_keyframe_weights_move_the_prefilter_and_the_scores(oracle, name):
    run_, default = reposition_search(oracle, name), reposition_search(oracle, "defaults")
    assert default[0] == rr.EXPECTED_WINNER and [r["stage"] for r in default[1]] == rr.EXPECTED_STAGES
    n, n0 = assert_weights_bite(name, run_, default)
    assert "taken" in assert_scenario_margins(run_[1], run_[2]) and run_[0] is not None
    print("%s: %d keyframes beyond the distance threshold (defaults %d), stages %s, winner %r" % (name, n, n0, [r["stage"] for r in run_[1]], run_[0]))


# ---- the designed sheets at the moved thresholds ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", range(rc.VARIANTS))
@pytest.mark.parametrize("name", sc.CAMERA)
def test_oracle_decides_as_the_census_predicts_at_a_moved_threshold(oracle, name, variant):
    th = sc.PROFILES[name]["minUseGrad"]
    oracle_decides_as_the_census_predicts(oracle, sc.W, sc.H, variant, min_use_grad=th)
    # the two classes that stand at the threshold follow it
    hyp, mg = rc.build(sc.W, sc.H, variant, th)
    names = {c.name: [(cx, cy) for cx, cy, c2, _ in rc.cells(sc.W, sc.H, variant) if c2 is c] for c in rc.CASES if "maxGrad" in c.name}
    for cx, cy in names["K5 maxGrad == minUseGrad"]:
        assert mg[cy, cx] == f32(th)
    for cx, cy in names["K5 maxGrad just below"]:
        assert mg[cy, cx] == np.nextafter(f32(th), f32(0))


def test_a_sheet_for_one_threshold_fails_the_census_of_another(oracle):
    """the test's own power: the sheet of 7.3 run at the default threshold decides the classes at the threshold differently"""
    th = sc.PROFILES["noisy-camera"]["minUseGrad"]
    hyp, mg = rc.build(sc.W, sc.H, 0, th)
    a, b = rc.census(hyp, mg, th, "fillholes"), rc.census(hyp, mg, rc.MIN_USE_GRAD, "fillholes")
    assert (a["created"] != b["created"]).sum() > 0


# ---- keyframeScore with explicit weights -------------------------------------------------------------------------------------------------
def ref_score(dist2, usage, wd, wu):
    """TrackableKeyFrameSearch.h:77-78, in single precision, left to right"""
    dist2, usage, wd, wu = f32(dist2), f32(usage), f32(wd), f32(wu)
    return f32(f32(f32(dist2 * wd) * wd) + f32(f32(f32((f32(1) - usage) * (f32(1) - usage)) * wu) * wu))


@pytest.mark.parametrize("name", ("defaults",) + sc.KF_WEIGHTS)
def test_score_bits_with_explicit_weights(exe, name):  # noqa: F811
    p = sc.params_of(name)
    wd, wu = f32(p.get("KFDistWeight", 4)), f32(p.get("KFUsageWeight", 3))
    rng = np.random.default_rng(11)
    cases = [(0.0, 1.0), (0.0, 0.0), (1.0, 1.0), (0.01, 0.5), (1e-4, 0.93)] + [(float(d), float(u)) for d, u in zip(rng.uniform(0, 0.2, 40), rng.uniform(0, 1, 40))]
    out = run(exe, ["scorew %s %s %s %s" % (bits(d), bits(u), bits(wd), bits(wu)) for d, u in cases])
    assert out == [bits(ref_score(d, u, wd, wu)) for d, u in cases]
    assert out == [bits(rr.score(d, u, wd, wu)) for d, u in cases]          # the restatement the re-position tests compare with
    assert out[1] == bits(f32(wu * wu)) and out[2] == bits(f32(wd * wd))
    if name == "defaults":
        assert out == run(exe, ["score %s %s" % (bits(d), bits(u)) for d, u in cases])
    else:
        assert out != run(exe, ["score %s %s" % (bits(d), bits(u)) for d, u in cases])
