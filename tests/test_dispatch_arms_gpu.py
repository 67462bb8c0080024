"""The arms of the finishing phase's dispatch ladders (k_track_step, tracker.hip) that no other test reaches, each held bit for bit against
a run that takes another arm.

The finishing phase picks its code by the number of tiles (or strips) `nb` of the pending level and by the number of pending trials:

    column sums   rows per slot K = ceil(nb / 16):  K <= 2 | <= 5 | <= 10 | more;  one trial, or all / three / one trial at a time
    tail_two      nb <= 128 | more            (single jobs, small batches, batches of more than 24 strips per job)
    tail_rows     nb <= 5 | <= 13 | <= 24     (strips per job of a throughput-mode batch)

The other tests track at 160x128, 176x144, 320x240, 640x480, 752x480 and 1280x1024: a single job there has 5..80 or 304 tiles at every
level it visits, so nothing finishes a level of 81..160 tiles (K = 6..10) — neither with one pending trial nor with several — and the
only batch with 6..13 strips per job (752x480 level 3, 8 jobs) is held to a tolerance against single calls
(profiles/r11_tracker_device_phases.md has the table, arm by arm).  Here:

    352x240 single job      level 1 = 176x120 = 21120 pixels = 88 tiles: K = 6; one trial per step against 2 and 5 trials on 88 tiles each
                            (three trials at a time: one group of two; one of three and one of two)
    352x288, 8 jobs         level 2 = 88x72 = 6336 pixels = 7 strips of 1024, 4 trials per step, against one trial per step

The tile and strip counts are worked out below as lsd_level_tiling (track_plan.hpp) does; tests/cpp/track_plan_test.cpp holds the same
numbers against the function itself, together with the trials and the cap of lsdhip_tracker_set_speculation.
"""
import numpy as np
import pytest

from common import ODOMETRY_ITS, assert_bit_equal, sequence

pytestmark = pytest.mark.gpu

IDENT7 = np.array([1.0, 0, 0, 0, 0, 0, 0])
BLOCK, GRID_CAP, STRIP_WORKGROUPS = 256, 304, 768


@pytest.fixture(scope="module")
def hip():
    import lsd_slam_amd as la
    return la


def tiles(w, h, level):
    """workgroups of a single job's evaluation at `level` (lsd_level_tiling without a batch)"""
    nb = -(-((w >> level) * (h >> level)) // BLOCK)
    if nb >= 16:
        nb = (nb + 7) & ~7
    return min(nb, GRID_CAP)


def strips(w, h, level, jobs):
    """strips per job of a throughput-mode batch at `level`"""
    work = (w >> level) * (h >> level)
    px = min(max((-(-work * jobs // STRIP_WORKGROUPS) + 255) & ~255, 1024), 8192)
    return -(-work // px)


@pytest.mark.parametrize("trials", [2, 5])
def test_a_level_of_81_to_160_tiles_finishes_the_same_with_one_and_with_several_trials(hip, trials):
    """Column sums of ten rows per slot, for one pending trial (set_speculation(1)) and for several, three at a time."""
    w, h = 352, 240
    nb = tiles(w, h, 1)
    assert nb == 88 and 5 < -(-nb // 16) <= 10 and nb <= 128          # K = 6: the ten-row form; keys of at most 128 tiles
    frames, depth0, K, gt = sequence(w, h, 4)
    ctx = hip.Context(w, h, K)
    kf = hip.Frame(ctx, 0, frames[0])
    kf.setDepthFromGroundTruth(depth0)
    ref = hip.TrackingReference()
    ref.importFrame(kf)
    tr_a, tr_b = hip.SE3Tracker(ctx), hip.SE3Tracker(ctx)
    tr_a.set_maxItsPerLvl(ODOMETRY_ITS)
    tr_b.set_maxItsPerLvl(ODOMETRY_ITS)
    tr_a.set_speculation(1)
    tr_b.set_speculation(trials, nb)        # the single-trial grid of level 1: identical partial-sum tiling
    init = IDENT7.copy()
    saved = 0
    for i in (1, 2, 3):
        fa, fb = hip.Frame(ctx, i, frames[i]), hip.Frame(ctx, i, frames[i])
        pa = tr_a.trackFrame(ref, fa, init)
        pb = tr_b.trackFrame(ref, fb, init)
        assert not tr_a.diverged
        assert np.array_equal(pa.view(np.uint64), pb.view(np.uint64)), (i, pa, pb)
        for k in ("numEvaluations", "numWarpUpdates", "lastResidual", "pointUsage", "lastGoodCount", "lastBadCount", "lastMeanRes",
                  "affineEstimation_a", "affineEstimation_b", "diverged", "trackingWasGood"):
            assert getattr(tr_a.last, k) == getattr(tr_b.last, k), (i, k)
        assert tr_a.exec_stats()[3] == tr_b.exec_stats()[3]                 # evaluations per level
        assert tr_a.exec_stats()[3][1] > 1                                  # ... level 1 among them, more than its first one
        assert_bit_equal(fa.refPixelWasGoodNoCreate(), fb.refPixelWasGoodNoCreate(), "refPixelWasGood")
        ca, sa, ka, _ = tr_a.step_stats()
        cb_, sb, kb, cb = tr_b.step_stats()
        assert cb == trials and ca + sa == tr_a.last.numEvaluations and cb_ + sb <= ca + sa
        saved += (ca + sa) - (cb_ + sb)
        init = pa
    assert saved > 0, saved                  # several trials were pending at some step


def test_a_batch_of_6_to_13_strips_per_job_speculates_to_the_same_bits(hip):
    """The tail rows of 6..13 strips (five 16-byte loads per lane), with up to four pending trials, against one trial per step."""
    w, h, jobs = 352, 288, 8
    assert [strips(w, h, l, jobs) for l in (1, 2, 3, 4)] == [25, 7, 2, 1]       # level 2: the middle form; level 1: keys, not rows (> 24)
    seqs = [sequence(w, h, 5, seq_index=s) for s in range(2)]
    ctx = hip.Context(w, h, seqs[0][2])
    results = []
    for one_trial in (True, False):
        tr = hip.SE3Tracker(ctx)
        tr.set_maxItsPerLvl(ODOMETRY_ITS)
        if one_trial:
            tr.set_speculation(1)
        refs, frs = [], []
        for s, (frames, depth0, K, gt) in enumerate(seqs):
            for k in (1, 2, 3, 4):
                kf = hip.Frame(ctx, 100 * s + 10 * k, frames[0])
                depth = depth0.copy()
                if k == 3:
                    depth[::2, 1::3] = 0
                kf.setDepthFromGroundTruth(depth)
                ref = hip.TrackingReference()
                ref.importFrame(kf)
                refs.append(ref)
                frs.append(hip.Frame(ctx, 100 * s + 10 * k + 1, frames[k]))
        poses, recs = tr.trackFrameBatch(refs, frs, np.tile(IDENT7, (jobs, 1)))
        results.append((np.asarray(poses).copy(), [r.numEvaluations for r in recs], [r.lastResidual for r in recs],
                        [f.refPixelWasGoodNoCreate().copy() for f in frs], tr.launch_stats()[0]))
    (p1, e1, r1, m1, n1), (p0, e0, r0, m0, n0) = results
    assert np.array_equal(p1, p0), np.abs(p1 - p0).max()
    assert e1 == e0 and r1 == r0
    for a, b in zip(m1, m0):
        assert np.array_equal(a, b)
    assert n0 < n1, (n0, n1)                    # the reject chains collapsed: trials were pending
