"""trackFrameOnPermaref's LM loop on the device, by its counts, and what the permaref entries leave behind in the tracker.

The loop.  For each (list, pose, *TestTrack settings) case of permaref_cases.loop_cases the oracle runs trackFrameOnPermaref in
SSE_EXACT_RCP and in SSE mode with a per-trial trace.  A case is clear when every traced comparison (error < lastErr, error / lastErr >
convergenceEpsTestTrack, incdot > stepSizeMinTestTrack, the two trackingWasGood ratios) keeps a relative margin m from its threshold,
m = 10 x the larger of the two modes' relative trial-error difference and the evaluation test's relative weightedError bound
(permaref_cases.loop_margin; tests/test_permaref_cases_cpu.py prints m, holds the unclear cases to a quarter and shows that the clear ones
reach every branch).  On a clear case the device must give, as a single job, as a host-cloud batch and — where the list is a keyframe's own
cloud — from a bank slot (n = 1: the single chain; n > 1: the batch),

  * the oracle's numEvaluations, numWarpUpdates, diverged and trackingWasGood;
  * a pose within 10 x the two modes' pose distance, at least 5e-4 (the floor of test_trackframe_parity);
  * under lsdhip_tracker_set_speculation(1, 0), (6, 8) and the default policy the same: the counts and the pose bound under each, and the
    same result bits wherever two policies tile the list alike (lsd_single_plan: (6, 8) caps the list at 8 tiles, so lists above 2048
    points become multi-pass under trials; the default policy caps lists above LSD_SPEC_CAP_ABOVE_PX points at 80 tiles; (1, 0) never
    caps).  Where the tilings differ the sums are added in another order, and whether the bits still agree is printed (on an MI355X they
    differ in each of those cases — 4097, 4836 and 25000 points — while counts, flags and the pose bound hold).

Unclear cases are reported and skipped.  Only what lsdhip_track_result carries is compared: there is no device-side trace.

Entry state.  A small list, a list large enough to grow the tracker's point buffer, the evaluation hooks, then the small list again on one
tracker: the bits a fresh tracker gives.  One case on a pipelined context: the one-stream context's bits."""
import numpy as np
import pytest

import permaref_cases as pc
from common import pose_distance

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def hip():
    import lsd_slam_amd as la
    return la


@pytest.fixture(scope="module")
def orc(oracle):
    return pc.Oracle(oracle)


@pytest.fixture(scope="module")
def world(hip, orc):
    sc = orc.scene((320, 240))
    ctx = hip.Context(sc.w, sc.h, sc.K)
    frames = {i: hip.Frame(ctx, i, sc.frames[i]) for i in (1, 2, 3)}
    bank = hip.KeyFrameBank(ctx, 2)
    slots = {}
    for k, kind in enumerate(("gt", "dense")):
        kf = hip.Frame(ctx, 100 + k, sc.frames[0])
        d, var = sc.keyframe_planes(kind)
        if var is None:
            kf.setDepthFromGroundTruth(d)
        else:
            kf.setDepthPlanes(d, var)
        slots[kind] = bank.put(kf)
        pos, cv = bank.download(slots[kind])
        opos, ocv = sc.keyframe_cloud(kind, permute=False)[:2]
        assert pos.tobytes() == opos.tobytes() and cv.tobytes() == ocv.tobytes(), kind
    return dict(sc=sc, ctx=ctx, frames=frames, bank=bank, slots=slots)


def field_bits(rec):
    return {name: np.array(getattr(rec, name)).tobytes() for name, _ in rec._fields_}


def tracker_for(hip, ctx, st, policy=None):
    tr = hip.SE3Tracker(ctx)
    s = tr.settings()
    s.lambdaInitialTestTrack, s.stepSizeMinTestTrack = st["lambdaInitial"], st["stepSizeMin"]
    s.convergenceEpsTestTrack, s.maxItsTestTrack = st["convergenceEps"], st["maxIts"]
    tr.set_settings(s)
    if policy is not None:
        tr.set_speculation(*policy)
    return tr


def check_against_oracle(oracle, tag, r, ra, tol):
    assert (r.numEvaluations, r.numWarpUpdates, int(r.diverged), int(r.trackingWasGood)) == \
        (ra.numEvaluations, ra.numWarpUpdates, int(ra.diverged), int(ra.trackingWasGood)), \
        (tag, r.numEvaluations, r.numWarpUpdates, r.diverged, r.trackingWasGood, ra.numEvaluations, ra.numWarpUpdates, ra.diverged, ra.trackingWasGood)
    dt, dr = pose_distance(np.array(r.frameToReference), np.array(ra.frameToRef), oracle)
    assert max(dt, dr) <= tol, (tag, dt, dr, tol)
    return max(dt, dr) / tol


def test_loop_counts_in_every_form(oracle, hip, orc, world):
    sc = world["sc"]
    loops = pc.loop_results(orc)
    skipped, worst, differing_orders = [], 0.0, []
    for case, clear, m, least, (ra, rb), (ta, tb) in loops:
        name, (pos, cv), fi, T0, st = case
        if not clear:
            skipped.append(name)
            continue
        dt, dr = pose_distance(np.array(ra.frameToRef), np.array(rb.frameToRef), oracle)
        tol = max(10 * max(dt, dr), 5e-4)
        frame = world["frames"][fi]
        n = len(pos)
        # the single job under the three policies
        bits = {}
        for policy in (None, (1, 0), (6, 8)):
            tr = tracker_for(hip, world["ctx"], st, policy)
            tr.trackFrameOnPermaref(pos, cv, frame, T0)
            worst = max(worst, check_against_oracle(oracle, "%s single %s" % (name, policy), tr.last, ra, tol))
            bits[policy] = (field_bits(tr.last), pc.single_tiles(n, policy))
        for policy in ((1, 0), (6, 8)):
            same = bits[policy][0] == bits[None][0]
            if bits[policy][1] == bits[None][1]:
                assert same, "%s: set_speculation%s changes the result (%s)" % (name, policy, [k for k in bits[None][0] if bits[None][0][k] != bits[policy][0][k]])
            else:
                differing_orders.append((name, policy, bits[policy][1], bits[None][1], same))
        # the host-cloud batch: the case twice
        tr = tracker_for(hip, world["ctx"], st)
        _, recs = tr.trackFrameOnPermarefBatch([(pos, cv), (pos, cv)], [frame, frame], [T0, T0])
        for j in range(2):
            worst = max(worst, check_against_oracle(oracle, "%s batch job %d" % (name, j), recs[j], ra, tol))
        assert field_bits(recs[0]) == field_bits(recs[1]), name
        # a bank slot: the single chain and the batch
        if name in pc.BANK_KIND:
            slot = world["slots"][pc.BANK_KIND[name]]
            _, one = tr.trackFrameOnPermarefBank(world["bank"], [slot], [frame], [T0])
            worst = max(worst, check_against_oracle(oracle, name + " bank n = 1", one[0], ra, tol))
            assert field_bits(one[0]) == bits[None][0], name + ": the bank's single chain is not the host-cloud call's"
            _, two = tr.trackFrameOnPermarefBank(world["bank"], [slot, slot], [frame, frame], [T0, T0])
            for j in range(2):
                worst = max(worst, check_against_oracle(oracle, "%s bank job %d" % (name, j), two[j], ra, tol))
                assert field_bits(two[j]) == field_bits(recs[j]), name + ": the bank batch is not the host-cloud batch"
    print("clear cases: %d of %d (skipped: %s); worst pose distance / tolerance %.3f" % (len(loops) - len(skipped), len(loops), skipped, worst))
    for name, policy, t1, t0, same in differing_orders:
        print("  %s: set_speculation%s tiles the list %s, the default policy %s: result bits %s" % (name, policy, t1, t0, "equal" if same else "differ"))
    assert len(skipped) * 4 <= len(loops)
    assert any(len(c[0][1][0]) > 2048 for c in loops if c[1]), "no clear case is multi-pass under set_speculation(6, 8)"
    assert sum(1 for c in loops if c[1] and c[0][0] in pc.BANK_KIND) >= 2


def permaref_bits(tr, cloud, frame, T0):
    tr.trackFrameOnPermaref(cloud[0], cloud[1], frame, T0)
    return field_bits(tr.last)


def test_a_grown_point_buffer_and_the_hooks_leave_nothing_behind(oracle, hip, orc, world):
    sc = world["sc"]
    T0 = oracle.se3_exp(np.array([0.01, 0.0, 0.0, 0, 0, 0.002]))
    small, large = sc.synthetic(255), sc.synthetic(25000)                    # 25000 > the 4096 points the buffer starts with
    frame = world["frames"][1]
    fresh = permaref_bits(hip.SE3Tracker(world["ctx"]), small, frame, T0)
    fresh_large = permaref_bits(hip.SE3Tracker(world["ctx"]), large, frame, T0)
    tr = hip.SE3Tracker(world["ctx"])
    assert permaref_bits(tr, small, frame, T0) == fresh
    assert permaref_bits(tr, large, frame, T0) == fresh_large
    assert permaref_bits(tr, small, frame, T0) == fresh, "after the buffer grew"
    ident = np.array([1, 0, 0, 0, 0, 0, 0], f32)
    rec, _ = tr.evaluatePoints(large[0], large[1], frame, sc.poses()["twist"], 1.03, -2.5)
    assert rec.warped_size > 0
    assert permaref_bits(tr, small, frame, T0) == fresh, "after evaluatePoints"
    tr.evaluatePointsBatch([small, large, small], [frame] * 3, np.array([ident, sc.poses()["twist"], sc.poses()["behind"]]),
                           np.array(pc.AFFINE, f32))
    assert permaref_bits(tr, small, frame, T0) == fresh, "after evaluatePointsBatch"
    tr.evaluatePointsBank(world["bank"], [world["slots"]["gt"], world["slots"]["dense"]], [frame] * 2, np.array([ident, sc.poses()["twist"]]))
    assert permaref_bits(tr, small, frame, T0) == fresh, "after evaluatePointsBank"
    _, b1 = tr.trackFrameOnPermarefBatch([small, large], [frame, frame], [T0, T0])
    tr.evaluatePointsBatch([large, small], [frame] * 2, np.array([ident, ident]))
    _, b2 = tr.trackFrameOnPermarefBatch([small, large], [frame, frame], [T0, T0])
    for j in range(2):
        assert field_bits(b1[j]) == field_bits(b2[j]), "batch job %d after evaluatePointsBatch" % j


def test_a_pipelined_context_gives_the_one_stream_bits(oracle, hip, orc, world):
    sc = world["sc"]
    T0 = oracle.se3_exp(np.array([0.01, 0.0, 0.0, 0, 0, 0.002]))
    cloud = sc.keyframe_cloud("gt")[:2]
    one = permaref_bits(hip.SE3Tracker(world["ctx"]), cloud, world["frames"][3], T0)
    rec1, _ = hip.SE3Tracker(world["ctx"]).evaluatePoints(cloud[0], cloud[1], world["frames"][3], sc.poses()["twist"])
    ctx = hip.Context(sc.w, sc.h, sc.K)
    ctx.set_pipeline(True)
    frame = hip.Frame(ctx, 3, sc.frames[3])
    tr = hip.SE3Tracker(ctx)
    assert permaref_bits(tr, cloud, frame, T0) == one
    rec2, _ = tr.evaluatePoints(cloud[0], cloud[1], frame, sc.poses()["twist"])
    assert bytes(rec1) == bytes(rec2)
    u1 = hip.SE3Tracker(world["ctx"]).checkPermaRefOverlap(cloud[0], T0)
    assert f32(tr.checkPermaRefOverlap(cloud[0], T0)).tobytes() == f32(u1).tobytes()
