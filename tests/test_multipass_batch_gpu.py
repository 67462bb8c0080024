"""The batched evaluation loop of k_track_step against the plain grid-stride loop of the same library.

On a dense keyframe level with more than one point per lane a single job takes the lane's points four at a time (their plane loads, then
their texel loads, in flight together; tracker.hip).  Every lane adds the same contributions in the same order as the plain loop, so two
trackers on one context — one created normally, one created with LSDHIP_EVAL_BATCH=0 — must agree BIT FOR BIT in everything they compute.

Frame sizes, levels and workgroup caps (LSDHIP_TRACK_CAP, 256 lanes per workgroup) are chosen for the points per lane they give, i.e.
for the shapes of the groups of four:

    160x128  level 1 (80x64)     cap 8: 2 / 3 points    cap 16: 1 / 2     one ragged group
    176x144  level 1 (88x72)     cap 8: 3 / 4           cap 16: 1 / 2     a full group; ragged last pass; width no power of two
    160x128  level 0             cap 8: 10              cap 16: 5         ragged third / second group
    176x144  level 0             cap 8: 12 / 13         cap 16: 6 / 7     full third and ragged fourth / ragged second group
"""
import numpy as np
import pytest

from common import ODOMETRY_ITS, assert_bit_equal, sequence

pytestmark = pytest.mark.gpu

IDENT7 = np.array([1.0, 0, 0, 0, 0, 0, 0])
SIZES = [(160, 128), (176, 144)]
CAPS = ["8", "16"]
AFFINE = [pytest.param({}, id="affine1"), pytest.param({"useAffineLightningEstimation": 0}, id="affine0")]


@pytest.fixture(scope="module")
def hip():
    import lsd_slam_amd as la
    return la


def _tracker_pair(hip, ctx, cap, monkeypatch):
    """(batched, plain): two trackers on one context under the same workgroup cap"""
    monkeypatch.setenv("LSDHIP_TRACK_CAP", cap)
    tr_batched = hip.SE3Tracker(ctx)
    monkeypatch.setenv("LSDHIP_EVAL_BATCH", "0")
    tr_plain = hip.SE3Tracker(ctx)
    monkeypatch.delenv("LSDHIP_EVAL_BATCH")
    monkeypatch.delenv("LSDHIP_TRACK_CAP")
    return tr_batched, tr_plain


def _keyframe(hip, ctx, frames, depth0):
    kf = hip.Frame(ctx, 0, frames[0])
    kf.setDepthFromGroundTruth(depth0)
    ref = hip.TrackingReference()
    ref.importFrame(kf)
    return ref


def _bits(x):
    return np.array(x, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("params", AFFINE)
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("w,h", SIZES)
def test_batched_evaluation_equals_the_plain_loop_bit_for_bit(oracle, hip, w, h, cap, params, monkeypatch):
    """evaluate() at a fixed non-identity pose, levels 1 and 0: A, b, weightedError, the counts and (level 1) refPixelWasGood of the
    batched loop are those of the plain loop bit for bit; the counts and the mask are the oracle's exactly."""
    frames, depth0, K, gt = sequence(w, h, 4)
    ctx = hip.Context(w, h, K, params=params)
    rg = _keyframe(hip, ctx, frames, depth0)
    kfo = oracle.Frame(0, frames[0], K)
    kfo.set_depth_gt(depth0)
    ro = oracle.TrackingReference()
    ro.import_frame(kfo)
    op = oracle.default_params()
    for k, v in params.items():
        setattr(op, k, v)
    tro = oracle.SE3Tracker(w, h, K, params=op, mode=oracle.SSE_EXACT_RCP)
    tr_batched, tr_plain = _tracker_pair(hip, ctx, cap, monkeypatch)
    T = oracle.se3_exp(np.array([0.03, -0.02, 0.01, 0.01, -0.015, 0.02])).astype(np.float32)
    a, b = (1.03, -2.5) if not params else (1.0, 0.0)
    for lvl in (1, 0):
        f1, f2, fo = hip.Frame(ctx, 3, frames[3]), hip.Frame(ctx, 3, frames[3]), oracle.Frame(3, frames[3], K)
        r1 = tr_batched.evaluate(rg, f1, T, lvl, a, b)
        r2 = tr_plain.evaluate(rg, f2, T, lvl, a, b)
        o = tro.evaluate(ro, fo, T, lvl, a, b)
        tag = "%dx%d cap %s level %d" % (w, h, cap, lvl)
        assert r1.warped_size > 1000, tag
        assert np.array_equal(_bits(r1.A), _bits(r2.A)), tag
        assert np.array_equal(_bits(r1.b), _bits(r2.b)), tag
        for k in ("weightedError", "lsError", "retval", "pointUsage", "meanRes", "affine_a_lastIt", "affine_b_lastIt", "goodCount", "badCount"):
            assert _bits(getattr(r1, k)) == _bits(getattr(r2, k)), (tag, k)
        counts = lambda r: (r.warped_size, r.goodCount, r.badCount, r.num_constraints)
        assert counts(r1) == counts(r2), tag
        assert counts(r1) == counts(o), tag
        if lvl == 1:
            assert_bit_equal(f1.refPixelWasGoodNoCreate(), f2.refPixelWasGoodNoCreate(), "mask batched vs plain " + tag)
            assert_bit_equal(f1.refPixelWasGoodNoCreate(), fo.wasgood(), "mask batched vs oracle " + tag)


@pytest.mark.parametrize("spec", [pytest.param(None, id="spec-default"), pytest.param((1, 0), id="spec-1")])
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("w,h", SIZES)
def test_batched_evaluation_tracks_to_the_same_pose_bit_for_bit(oracle, hip, w, h, cap, spec, monkeypatch):
    """trackFrame with the odometry iterations, under the default speculation and with one evaluation per launch: the same pose, counters,
    mask, evaluations per level and number of launches from both loops."""
    frames, depth0, K, gt = sequence(w, h, 4)
    ctx = hip.Context(w, h, K)
    rg = _keyframe(hip, ctx, frames, depth0)
    tr_batched, tr_plain = _tracker_pair(hip, ctx, cap, monkeypatch)
    for tr in (tr_batched, tr_plain):
        tr.set_maxItsPerLvl(ODOMETRY_ITS)
        if spec is not None:
            tr.set_speculation(*spec)
    init = IDENT7.copy()
    for i in (1, 2, 3):
        f1, f2 = hip.Frame(ctx, i, frames[i]), hip.Frame(ctx, i, frames[i])
        p1 = tr_batched.trackFrame(rg, f1, init)
        p2 = tr_plain.trackFrame(rg, f2, init)
        tag = "%dx%d cap %s frame %d" % (w, h, cap, i)
        assert not tr_batched.diverged, tag
        assert np.array_equal(p1.view(np.uint64), p2.view(np.uint64)), (tag, p1, p2)
        for k in ("numEvaluations", "numWarpUpdates", "lastResidual", "pointUsage", "lastGoodCount", "lastBadCount", "lastMeanRes",
                  "affineEstimation_a", "affineEstimation_b", "diverged", "trackingWasGood"):
            assert getattr(tr_batched.last, k) == getattr(tr_plain.last, k), (tag, k)
        assert tr_batched.exec_stats()[3] == tr_plain.exec_stats()[3], tag          # evaluations per level
        assert tr_batched.exec_stats()[3][1] > 0, tag                               # ... the multi-pass level among them
        assert tr_batched.step_stats() == tr_plain.step_stats(), tag                # launches of the chain, trials per step
        assert tr_batched.launch_stats() == tr_plain.launch_stats(), tag
        assert_bit_equal(f1.refPixelWasGoodNoCreate(), f2.refPixelWasGoodNoCreate(), "refPixelWasGood " + tag)
        init = p1
