"""lsdhip_tracker_find_reposition_candidate on scenario A (tests/reposition_ref.py; its census is tests/test_reposition_cpu.py):

  * the same winner, the same branch per banked keyframe and the same counts as the restatement over the oracle, usage within rel 1e-5 and
    tracked poses within 2e-3 (the tolerances of test_permaref_paths);
  * bit for bit what the same search gives when it is composed from the single host-cloud calls (checkPermaRefOverlap and
    trackFrameOnPermaref per candidate on the downloaded clouds, the restatement's own selection);
  * the C++ classes (KeyFrameBank, TrackableKeyFrameSearch of include/lsd_slam_hip.hpp) run as a stand-alone program and agree with the
    host-cloud members beside them (tests/cpp/kfbank_classes_test.cpp);
  * two launches at most: a query beyond the distance threshold launches nothing, one whose candidates all fail the acceptance test
    still ran one overlap launch and one tracking batch."""
import os
import subprocess

import numpy as np
import pytest

import reposition_ref as rr
from common import ROOT, pose_distance

pytestmark = pytest.mark.gpu

STAGE = {i: n for i, n in enumerate(rr.STAGES)}


@pytest.fixture(scope="module")
def hip():
    import lsd_slam_amd as la
    return la


@pytest.fixture(scope="module")
def restated(oracle):
    K, kfs, frame, pose = rr.scenario_a_oracle(oracle)
    tracker = oracle.SE3Tracker(rr.W, rr.H, K, mode=oracle.SSE_EXACT_RCP)
    return rr.search(oracle, tracker, kfs, frame, pose, kfs[rr.PARENT_SLOT]["id"], rr.W, rr.H, K)


@pytest.fixture(scope="module")
def banked(hip):
    """scenario A on the device: 16 keyframes with ground-truth depth in a bank, their recorded poses and meanIdepth 0.5, the query frame"""
    K, kviews, q = rr.scenario_a_inputs()
    ctx = hip.Context(rr.W, rr.H, K)
    bank = hip.KeyFrameBank(ctx, len(kviews))
    kfs = []
    for i, img, depth, pose in kviews:
        f = hip.Frame(ctx, i, img)
        f.setDepthFromGroundTruth(depth)
        assert bank.put(f, rr.pose8(pose), rr.MEAN_IDEPTH) == len(kfs)
        kfs.append(f)
    return ctx, bank, kfs, hip.Frame(ctx, q[0], q[1]), rr.pose8(q[3]), kviews, q


class SingleCalls:
    """the restatement's tracker, made of the HIP single host-cloud calls"""

    class Result:
        pass

    def __init__(self, hip, ctx, frame):
        self.t, self.frame = hip.SE3Tracker(ctx), frame

    def check_overlap(self, pos, ref_frame, T):
        return self.t.checkPermaRefOverlap(pos, T)

    def track_permaref(self, pos, cv, frame, T):
        r = self.Result()
        r.frameToRef = list(self.t.trackFrameOnPermaref(pos, cv, self.frame, T))
        for k in ("pointUsage", "lastGoodCount", "lastBadCount", "trackingWasGood", "diverged"):
            setattr(r, k, getattr(self.t.last, k))
        return r


def test_scenario_a(hip, oracle, restated, banked):
    ctx, bank, kfs, frame, framePose, kviews, q = banked
    best, orecs, counts = restated
    search = hip.TrackableKeyFrameSearch(ctx, bank)
    assert search.relocalizationTH == pytest.approx(0.7)
    slot = search.findRePositionCandidate(frame, framePose, kviews[rr.PARENT_SLOT][0], 1.0)
    res, recs = search.last, search.records()
    for r in recs:
        print(r.slot, STAGE[r.stage], r.dist2, r.usage, r.score, r.newScore, r.goodVal, r.poseDiscrepancy, r.trackingWasGood)
    # ---- against the restatement over the oracle ----
    assert slot == best == rr.EXPECTED_WINNER and res.frameId == kviews[best][0]
    assert [STAGE[r.stage] for r in recs] == [o["stage"] for o in orecs] == rr.EXPECTED_STAGES
    assert (res.numPotential, res.numChecked, res.numTracked) == (counts["potential"], counts["checked"], counts["tracked"])
    assert (res.overlapLaunches, res.trackingBatches) == (1, 1)
    for r, o in zip(recs, orecs):
        assert r.slot == o["slot"] and r.frameId == o["id"]
        assert r.dist2 == pytest.approx(float(o["dist2"]), rel=1e-5)
        if "usage" in o:
            assert r.usage == pytest.approx(float(o["usage"]), rel=1e-5), r.slot
            assert r.score == pytest.approx(float(o["score"]), rel=1e-4), r.slot
            assert max(pose_distance(np.array(r.refToFrame), o["refToFrame"], oracle)) < 1e-9
        if "tracked" in o:
            dt, dr = pose_distance(np.array(r.refToFrame_tracked), o["tracked"], oracle)
            assert max(dt, dr) < 2e-3, (r.slot, dt, dr)
            assert bool(r.trackingWasGood) == o["trackingWasGood"] and bool(r.diverged) == o["diverged"]
    w = recs[best]
    assert res.bestScore == w.score and res.bestUsage == w.usageTracked and res.bestPoseDiscrepancy == w.poseDiscrepancy
    assert list(res.refToFrame) == list(w.refToFrame) and list(res.refToFrame_tracked) == list(w.refToFrame_tracked)
    assert search.getRefFrameScore(w.dist2, w.usage) == w.score
    # ---- against the same search made of single host-cloud calls on the device ----
    hkfs = []
    for s, (i, img, depth, pose) in enumerate(kviews):
        pos, cv = bank.download(s)
        hkfs.append({"id": i, "pos": pos, "cv": cv, "frame": None, "meanIdepth": rr.MEAN_IDEPTH, "camToWorld": pose})
    hbest, hrecs, hcounts = rr.search(oracle, SingleCalls(hip, ctx, frame), hkfs, None, q[3], kviews[rr.PARENT_SLOT][0], rr.W, rr.H, rr.scenario_a_inputs()[0])
    assert hbest == slot and [h["stage"] for h in hrecs] == [STAGE[r.stage] for r in recs]
    assert (hcounts["potential"], hcounts["checked"], hcounts["tracked"]) == (res.numPotential, res.numChecked, res.numTracked)
    for r, h in zip(recs, hrecs):
        # what the device computed: bit for bit; what the host derives from it in single precision: to the last digits
        assert r.dist2 == pytest.approx(float(h["dist2"]), rel=1e-6), r.slot
        if "usage" in h:
            assert np.float32(r.usage) == h["usage"], (r.slot, r.usage, h["usage"])
            assert r.score == pytest.approx(float(h["score"]), rel=1e-6), r.slot
        if "tracked" in h:
            assert list(r.refToFrame_tracked) == list(h["tracked"]), r.slot
            assert bool(r.trackingWasGood) == h["trackingWasGood"] and bool(r.diverged) == h["diverged"]
            assert r.newScore == pytest.approx(float(h["newScore"]), rel=1e-6) and r.goodVal == pytest.approx(float(h["goodVal"]), rel=1e-6), r.slot
            assert r.poseDiscrepancy == pytest.approx(float(h["poseDiscrepancy"]), abs=1e-6)


def test_queries_without_a_candidate(hip, banked):
    ctx, bank, kfs, frame, framePose, kviews, q = banked
    search = hip.TrackableKeyFrameSearch(ctx, bank)
    away = framePose.copy()
    away[4] += 10.0                     # every keyframe is beyond distanceTH = 1 / 16
    assert search.findRePositionCandidate(frame, away, kviews[rr.PARENT_SLOT][0], 1.0) is None
    r = search.last
    assert (r.slot, r.frameId, r.numPotential, r.numChecked, r.numTracked, r.overlapLaunches, r.trackingBatches) == (-1, -1, 0, 0, 0, 0, 0)
    assert r.bestScore == 1.0 and all(STAGE[x.stage] == "far" for x in search.records()) and len(search.records()) == 16
    # nobody passes an acceptance threshold no goodVal can reach: both launches ran, nothing is taken
    search.relocalizationTH = 1.5
    assert search.findRePositionCandidate(frame, framePose, kviews[rr.PARENT_SLOT][0], 1.0) is None
    r = search.last
    assert (r.overlapLaunches, r.trackingBatches, r.numTracked) == (1, 1, 5) and r.bestScore == 1.0
    assert [STAGE[x.stage] for x in search.records()].count("rejected") == 5
    search.relocalizationTH = 0.7
    assert search.findRePositionCandidate(frame, framePose, kviews[rr.PARENT_SLOT][0], 1.0) == rr.EXPECTED_WINNER


def test_cpp_classes(hip, tmp_path):
    """include/lsd_slam_hip.hpp's KeyFrameBank / TrackableKeyFrameSearch / Frame::idxInKeyframes, compiled with plain g++ against the library"""
    exe, libdir = str(tmp_path / "kfbank_classes_test"), os.path.join(ROOT, "lsd_slam_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "kfbank_classes_test.cpp"), "-o", exe, "-L" + libdir, "-llsdhip", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert r.stdout.splitlines()[-1] == "kfbank classes ok"
