"""The code between the phases of a tracking launch (k_track_step, tracker.hip): what a launch reads before its first barrier, which
launches leave at once, how a level's trials are found again in the next launch — held by running the same jobs with launch budgets and
speculation settings that move every one of those decisions, and asking for the same bits.

A launch's prologue requests the state, the trial records and (in every workgroup but the leader) the `done` word of the early return in
one round trip; a workgroup finds its trial and tile from five tile counts and five trial counts packed into the launch's arguments, by
comparisons instead of a division; the state words the glue branches on are read in one batch per barrier; the top-3 keys of a tile are
merged under the barriers of the sum reduction; lambda after a chain of rejections is a running product.  None of this may change a
result, whoever queues the launches:

    LSDHIP_BUDGET_FIXED = 1, 2   every launch is (every second launch is) the last of its budget: the host tops up from the state in HBM
    LSDHIP_BUDGET_FIXED = 40     some thirty launches sit behind the finishing one: each workgroup of each must leave at the early return
                                 (workgroups other than the leader) or at the `done` state (the leader), having changed nothing
    unset                        the budget the tracker works out itself
    set_speculation(1) | default one trial per launch (no trial records) | the reject chain's retries side by side, five or six at a time

320x240: level 4 is 20x15 = 300 pixels = two tiles, the second with 44 live lanes.  352x240: level 1 is 88 tiles (the ten-row column
sums of test_dispatch_arms_gpu.py).  Within one speculation setting everything is compared, the number of evaluating launches included;
across the two settings everything but that number, which speculation exists to lower.

The far start (an initial estimate 5 cm and 0.02 rad off, frame 3) is there for a reject chain that does not fit one launch: the oracle
runs 16 evaluations at level 2 from it (found by differencing the oracle's evaluation counts over runs with the finer levels' iterations
set to 0), among them retries beyond the fifth, where lambda's power of two and the trial records of two launches are in play.
"""
import numpy as np
import pytest

from common import ODOMETRY_ITS, assert_bit_equal, sequence

pytestmark = pytest.mark.gpu

IDENT7 = np.array([1.0, 0, 0, 0, 0, 0, 0])
BUDGETS = (None, 1, 2, 40)
RESULT_FIELDS = ("numEvaluations", "numWarpUpdates", "lastResidual", "pointUsage", "lastGoodCount", "lastBadCount", "lastMeanRes",
                 "affineEstimation_a", "affineEstimation_b", "diverged", "trackingWasGood")
FAR_START = [0.02, 0.02, -0.04, 0.0, 0.02, 0.0]


@pytest.fixture(scope="module")
def hip():
    import lsd_slam_amd as la
    return la


def trackers(hip, ctx, monkeypatch):
    """{(trials per launch or None, budget or None): tracker}; the environment is read when a tracker is created"""
    out = {}
    for spec in (1, None):
        for budget in BUDGETS:
            if budget is None:
                monkeypatch.delenv("LSDHIP_BUDGET_FIXED", raising=False)
            else:
                monkeypatch.setenv("LSDHIP_BUDGET_FIXED", str(budget))
            t = hip.SE3Tracker(ctx)
            t.set_maxItsPerLvl(ODOMETRY_ITS)
            if spec is not None:
                t.set_speculation(spec)
            out[(spec, budget)] = t
    monkeypatch.delenv("LSDHIP_BUDGET_FIXED", raising=False)
    return out


def signature(tr, pose, frame):
    fields = tuple(np.float32(getattr(tr.last, k)).tobytes() if isinstance(getattr(tr.last, k), float) else getattr(tr.last, k)
                   for k in RESULT_FIELDS)
    return {"pose": np.asarray(pose, np.float64).tobytes(), "fields": fields, "levelEvals": tuple(tr.exec_stats()[3]),
            "numLaunches": tr.launch_stats()[0], "mask": frame.refPixelWasGoodNoCreate().copy()}


def assert_same(a, b, what, launches):
    assert a["pose"] == b["pose"], (what, np.frombuffer(a["pose"]), np.frombuffer(b["pose"]))
    assert a["fields"] == b["fields"], (what, a["fields"], b["fields"])
    assert a["levelEvals"] == b["levelEvals"], (what, a["levelEvals"], b["levelEvals"])
    if launches:
        assert a["numLaunches"] == b["numLaunches"], (what, a["numLaunches"], b["numLaunches"])
    assert_bit_equal(a["mask"], b["mask"], "refPixelWasGood %r" % (what,))


def track_all(hip, ctx, trs, ref, image, init, what):
    sigs, poses = {}, {}
    for key, tr in trs.items():
        f = hip.Frame(ctx, 1, image)
        poses[key] = tr.trackFrame(ref, f, init)
        sigs[key] = signature(tr, poses[key], f)
    base = sigs[(None, None)]
    for (spec, budget), s in sigs.items():
        assert_same(sigs[(spec, None)], s, (what, spec, budget), launches=True)
        assert_same(base, s, (what, spec, budget, "against the default"), launches=False)
    return base, poses[(None, None)], sigs


@pytest.mark.parametrize("shape", [(320, 240), (352, 240)], ids=["320x240", "352x240"])
def test_budgets_and_speculation_change_nothing(hip, monkeypatch, shape):
    w, h = shape
    assert (w >> 4) * (h >> 4) in (300, 330)                     # level 4: two tiles of 256, the second partly filled
    frames, depth0, K, gt = sequence(w, h, 4)
    ctx = hip.Context(w, h, K)
    kf = hip.Frame(ctx, 0, frames[0])
    kf.setDepthFromGroundTruth(depth0)
    ref = hip.TrackingReference()
    ref.importFrame(kf)
    trs = trackers(hip, ctx, monkeypatch)
    init = IDENT7.copy()
    fewer = 0
    for i in (1, 2, 3):
        base, pose, sigs = track_all(hip, ctx, trs, ref, frames[i], init, i)
        assert not trs[(None, None)].last.diverged
        assert sum(base["levelEvals"]) == trs[(None, None)].last.numEvaluations
        assert base["numLaunches"] <= sigs[(1, None)]["numLaunches"] <= trs[(1, None)].last.numEvaluations
        fewer += sigs[(1, None)]["numLaunches"] - base["numLaunches"]
        init = pose
    assert fewer > 0, fewer                                       # trials were pending: the records were read


def test_a_reject_chain_longer_than_one_launch(hip, oracle, monkeypatch):
    w, h = 320, 240
    frames, depth0, K, gt = sequence(w, h, 4)
    init = oracle.se3_exp(np.array(FAR_START, np.float64))
    kfo = oracle.Frame(0, frames[0], K)
    kfo.set_depth_gt(depth0)
    refo = oracle.TrackingReference()
    refo.import_frame(kfo)
    tro = oracle.SE3Tracker(w, h, K, mode=oracle.SSE)
    tro.set_max_its(ODOMETRY_ITS)
    want = tro.track(refo, oracle.Frame(3, frames[3], K), init)
    assert not want.diverged and want.numEvaluations >= 30, want.numEvaluations

    ctx = hip.Context(w, h, K)
    kf = hip.Frame(ctx, 0, frames[0])
    kf.setDepthFromGroundTruth(depth0)
    ref = hip.TrackingReference()
    ref.importFrame(kf)
    trs = trackers(hip, ctx, monkeypatch)
    base, pose, sigs = track_all(hip, ctx, trs, ref, frames[3], init, "far start")
    print("far start: evaluations per level %r, launches %d (one trial per launch: %d)" % (
        base["levelEvals"], base["numLaunches"], sigs[(1, None)]["numLaunches"]))
    assert max(base["levelEvals"]) >= 7, base["levelEvals"]
    assert trs[(None, None)].last.numEvaluations == want.numEvaluations, (base["levelEvals"], want.numEvaluations)


def test_a_batch_of_eight_jobs_speculates_to_the_same_bits(hip):
    """The batch kernels share the prologue: 8 jobs at 320x240, one trial per step against the default (up to four, with their records).
    (Batches have no launch-budget hook; their rounds queued behind the last job's finishing one leave at the same `done` test.)"""
    w, h, jobs = 320, 240, 8
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
                kf.setDepthFromGroundTruth(depth0)
                ref = hip.TrackingReference()
                ref.importFrame(kf)
                refs.append(ref)
                frs.append(hip.Frame(ctx, 100 * s + 10 * k + 1, frames[k]))
        poses, recs = tr.trackFrameBatch(refs, frs, np.tile(IDENT7, (jobs, 1)))
        results.append((np.asarray(poses).copy(), [tuple(getattr(r, k) for k in RESULT_FIELDS) for r in recs],
                        [f.refPixelWasGoodNoCreate().copy() for f in frs], tr.launch_stats()[0]))
    (p1, r1, m1, n1), (p0, r0, m0, n0) = results
    assert np.array_equal(p1.view(np.uint64), p0.view(np.uint64)), np.abs(p1 - p0).max()
    assert r1 == r0
    for a, b in zip(m1, m0):
        assert np.array_equal(a, b)
    assert n0 < n1, (n0, n1)                    # the reject chains collapsed: trials were pending
