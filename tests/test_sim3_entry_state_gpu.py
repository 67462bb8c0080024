"""What the Sim3 tracker's entry points leave behind, on 160x128 synthetic pairs (level 3 is 20x16), levels 3..1 unless stated.  Every
comparison is == on the bytes of every field of lsdhip_sim3_result / lsdhip_sim3_eval_record, product against product: no tolerances.

  * A refused lsdhip_sim3tracker_track_batch (a frame without depth: LSDHIP_E_STATE; startLevel < finalLevel or no job: LSDHIP_E_ARG)
    writes no byte of results[] — every job is checked before the first result is reset — and the same single track call before and
    after it returns the same bytes.
  * A batch of S3_MAXB + 1 = 13 jobs runs in two chunks, the second one in slot 0 again; every job's record equals its single call's.
    The job that diverges on its first evaluation is alone in the second chunk (index 12) or first of the first (index 0): the other
    jobs go on after it has ended.  (The iteration limits belong to the tracker, not to a job: the whole comparison runs under limits that
    cut level 1 short, so the jobs end after different numbers of evaluations.)
  * lsdhip_sim3tracker_evaluate and the track entries share the tracker's launch counter, scratch rows and keys: interleaved on one
    tracker, each call returns what it returns from a fresh tracker, and a refused evaluation in between changes nothing.
  * The single evaluation and the fused loop describe a level through the same function.  Where nothing moves — keyframe and frame hold
    the same image and the same plane at depth 1, intrinsics that are powers of two, identity pose: every warped point lands on its
    own pixel and every residual is exactly 0 — the loop's only proposal is the zero step, which is not an improvement, and the call
    ends on the system of its FIRST evaluation: lastSim3Hessian, pointUsage and the affine pair are that evaluation's, which
    lsdhip_sim3tracker_evaluate returns at the same pose with (1, 0).  Levels 0 (level-0 planes on demand, 80 strips) and 3 (one strip)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 160, 128
LSDHIP_OK, LSDHIP_E_ARG, LSDHIP_E_STATE = 0, -1, -3
FAR = np.array([1.0, 0, 0, 0, 50.0, 0, 0, 1.0])             # frame far to the side: nothing projects into the image
ITS = [5, 3, 50, 100, 100]                                   # level 1 stops after 3 iterations


@pytest.fixture(scope="module")
def hip():
    import lsd_slam_amd as la
    return la


@pytest.fixture(scope="module")
def world(hip):
    """one keyframe, three frames at their own scales, their ground-truth poses (scale 1: the tracker has to find it), a frame without depth"""
    from lsd_slam_amd import synth
    scn = synth.Scene(0)
    ctx = hip.Context(W, H, synth.intrinsics(W, H))
    imgA, depthA = scn.render(0, W, H)
    kf = hip.Frame(ctx, 0, imgA)
    kf.setDepthFromGroundTruth(depthA)
    frs, inits = [], []
    for k, scale in ((2, 1.0), (3, 1.25), (4, 0.8)):
        img, depth = scn.render(k, W, H)
        f = hip.Frame(ctx, k, img)
        f.setDepthFromGroundTruth((depth / scale).astype(np.float32))
        R, t = scn.frame_to_ref(k, 0)
        frs.append(f)
        inits.append(np.concatenate([synth.rot_to_quat(R), t, [1.0]]))
    bare = hip.Frame(ctx, 9, scn.render(1, W, H)[0])
    return dict(ctx=ctx, kf=kf, frs=frs, inits=inits, bare=bare)


def field_bits(rec):
    return {name: np.array(getattr(rec, name)).tobytes() for name, _ in rec._fields_}


def same(a, b, what):
    a, b = field_bits(a), field_bits(b)
    for name in a:
        assert a[name] == b[name], "%s: %s differs" % (what, name)


def tracker(hip, world, its=ITS):
    tr = hip.Sim3Tracker(world["ctx"])
    tr.setMaxItsPerLvl(its)
    return tr


def batch_rc(tr, kfs, frs, inits, first, last, res, n=None):
    n = len(frs) if n is None else n
    k = (C.c_void_p * len(kfs))(*[f.h_ for f in kfs])
    f = (C.c_void_p * len(frs))(*[f.h_ for f in frs])
    T = np.ascontiguousarray(inits, np.float64)
    return tr.L.lsdhip_sim3tracker_track_batch(tr.h_, n, k, f, T.ctypes.data, first, last, res)


def test_a_refused_batch_changes_nothing(hip, world):
    from lsd_slam_amd import capi
    kf, frs, inits = world["kf"], world["frs"], world["inits"]
    tr = tracker(hip, world)
    before = tr.trackFrameSim3(kf, frs[1], inits[1], 3, 1)[1]
    assert not before.diverged and before.numEvaluations > 3
    res = (capi.Sim3Result * 3)()
    C.memset(res, 0xA5, C.sizeof(res))
    pattern = bytes(res)
    refusals = (("a frame without depth", [frs[0], frs[1], world["bare"]], 3, 1, 3, LSDHIP_E_STATE),
                ("startLevel < finalLevel", frs, 1, 3, 3, LSDHIP_E_ARG),
                ("no job", frs, 3, 1, 0, LSDHIP_E_ARG))
    for what, fs, first, last, n, want in refusals:
        assert batch_rc(tr, [kf] * 3, fs, inits, first, last, res, n) == want, what
        assert bytes(res) == pattern, "%s: the refused batch wrote into results[]" % what
        after = tr.trackFrameSim3(kf, frs[1], inits[1], 3, 1)[1]
        same(after, before, "single call after the refusal (%s)" % what)
        assert after.numEvaluations == before.numEvaluations


def chunk_jobs(world, far_at):
    """13 distinct jobs over the three pairs (the poses of each round a little further off), the diverging one at index far_at"""
    jobs = []
    for j in range(12):
        init = world["inits"][j % 3].copy()
        init[4:7] += 0.001 * (j // 3) * np.array([1.0, -1.0, 0.5])
        jobs.append((j % 3, init))
    jobs.insert(far_at, (0, FAR))
    return jobs


@pytest.fixture(scope="module")
def singles(hip, world):
    """the single-call record of every job of chunk_jobs, each from the one tracker the single calls share (computed once, left unchanged)"""
    tr = tracker(hip, world)
    return [tr.trackFrameSim3(world["kf"], world["frs"][p], init, 3, 1)[1] for p, init in chunk_jobs(world, 12)]


@pytest.mark.parametrize("far_at", [12, 0])
def test_a_chunked_batch_equals_single_calls(hip, world, singles, far_at):
    jobs = chunk_jobs(world, far_at)
    assert len(jobs) == 13
    want = list(singles[:12])
    want.insert(far_at, singles[12])
    tr = tracker(hip, world)
    poses, recs = tr.trackFrameSim3Batch([world["kf"]] * 13, [world["frs"][p] for p, _ in jobs], np.array([i for _, i in jobs]), 3, 1)
    for j in range(13):
        same(recs[j], want[j], "job %d of 13 (diverging job at %d)" % (j, far_at))
    assert recs[far_at].diverged == 1 and recs[far_at].numEvaluations == 1
    others = [r for j, r in enumerate(recs) if j != far_at]
    assert all(r.diverged == 0 and r.numEvaluations > 3 for r in others)
    assert len({r.numEvaluations for r in others}) > 1, "the jobs were meant to end after different numbers of evaluations"
    assert len({field_bits(r)["frameToReference"] for r in recs}) == 13, "13 distinct jobs"


def interleaved_calls(hip, world):
    """(name, call(tracker) -> record or list of records)"""
    kf, frs, inits = world["kf"], world["frs"], world["inits"]
    from oracle.pyoracle import sim3_inv
    T = [sim3_inv(i) for i in inits]
    return [("evaluate 0", lambda tr: [tr.evaluate(kf, frs[0], T[0], 1, 0.97, 1.5)]),
            ("track 1", lambda tr: [tr.trackFrameSim3(kf, frs[1], inits[1], 3, 1)[1]]),
            ("evaluate 2", lambda tr: [tr.evaluate(kf, frs[2], T[2], 1)]),
            ("track_batch of 2", lambda tr: tr.trackFrameSim3Batch([kf, kf], [frs[2], frs[0]], np.array([inits[2], inits[0]]), 3, 1)[1])]


def test_evaluation_and_tracking_interleave(hip, world):
    from lsd_slam_amd import capi
    calls = interleaved_calls(hip, world)
    fresh = [call(tracker(hip, world)) for _, call in calls]
    tr = tracker(hip, world)
    T = np.ascontiguousarray([1.0, 0, 0, 0, 0, 0, 0, 1.0])
    for (name, call), want in zip(calls, fresh):
        got = call(tr)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            same(g, w, "%s on the shared tracker" % name)
        # a refused evaluation between the calls: the record it was given and the calls behind it are as without it
        rec = capi.Sim3EvalRecord()
        C.memset(C.byref(rec), 0x5A, C.sizeof(rec))
        pattern = bytes(rec)
        ev = tr.L.lsdhip_sim3tracker_evaluate
        assert ev(tr.h_, world["kf"].h_, world["bare"].h_, T.ctypes.data, 1, 1.0, 0.0, C.byref(rec)) == LSDHIP_E_STATE
        assert ev(tr.h_, world["kf"].h_, world["frs"][0].h_, T.ctypes.data, 5, 1.0, 0.0, C.byref(rec)) == LSDHIP_E_ARG
        assert bytes(rec) == pattern


@pytest.fixture(scope="module")
def still(hip):
    """keyframe and frame: the same image, the same plane at depth 1; fx = fy = 128 and principal points with a short binary expansion on
    every level, so that the identity pose maps every pixel onto itself without rounding"""
    from lsd_slam_amd import synth
    K = np.array([128.0, 128.0, 79.5, 63.5], np.float32)
    ctx = hip.Context(W, H, K)
    img = synth.Scene(0).render(0, W, H)[0]
    depth = np.ones((H, W), np.float32)
    a, b = hip.Frame(ctx, 0, img), hip.Frame(ctx, 1, img)
    a.setDepthFromGroundTruth(depth)
    b.setDepthFromGroundTruth(depth)
    return dict(ctx=ctx, kf=a, fr=b)


@pytest.mark.parametrize("level", [0, 3])
def test_single_evaluation_and_fused_loop_describe_the_same_level(hip, still, level):
    ident = np.array([1.0, 0, 0, 0, 0, 0, 0, 1.0])
    its = [0] * 5
    its[level] = 1
    ev = hip.Sim3Tracker(still["ctx"]).evaluate(still["kf"], still["fr"], ident, level, 1.0, 0.0)
    assert ev.warped_size >= 100 and ev.sumResP == 0 and ev.sumResD == 0 and ev.numTermsD > 0, "the scene was meant to have no residual at all"
    tr = hip.Sim3Tracker(still["ctx"])
    tr.setMaxItsPerLvl(its)
    pose, r = tr.trackFrameSim3(still["kf"], still["fr"], ident, level, level)
    # first evaluation, then the zero step's (no improvement on a residual of 0, and the step is below stepSizeMin: the level ends)
    assert r.numEvaluations == 2 and r.diverged == 0
    assert np.array_equal(pose, ident)
    assert np.array(r.lastSim3Hessian).tobytes() == np.array(ev.A).tobytes()
    assert np.any(np.array(ev.A) != 0)
    assert np.float32(r.pointUsage).tobytes() == np.float32(ev.pointUsage).tobytes()
    assert np.float32(r.affineEstimation_a).tobytes() == np.float32(ev.affine_a_lastIt).tobytes()
    assert np.float32(r.affineEstimation_b).tobytes() == np.float32(ev.affine_b_lastIt).tobytes()
