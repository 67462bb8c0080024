"""What the tracker's entry points leave behind in the tracker, on 160x128 synthetic pairs and batches of 8 jobs (the smallest count at which
LSD_BATCH_THROUGHPUT_MIN_JOBS puts a batch into throughput mode).

The shape of a batch (jobs, workgroup cap per job) decides how fill_level tiles a level.  It is a value the entry point passes to the job
builders, so a call that is refused half-way cannot leave it behind for the next single-frame job:

  * a refused lsdhip_tracker_eval_throughput (LSDHIP_E_STATE: level 0 has no reference blocks, so it is never in throughput mode; LSDHIP_E_ARG:
    fewer than 8 jobs) or lsdhip_tracker_evaluate_batch (a level outside the tracking range) between two identical lsdhip_tracker_track calls
    changes neither the second call's result (field by field, bit for bit) nor its launch count.  (At this size the per-job cap of an 8-job
    batch, 32 workgroups, is above level 1's 24: a leaked shape would show through the strips of throughput mode.)
  * lsdhip_tracker_eval_throughput — reached from no other test — returns a finite time and byte count and leaves lsdhip_tracker_evaluate_batch's
    records and forms of the same jobs as they were, bit for bit.
  * lsdhip_tracker_evaluate and lsdhip_tracker_evaluate_batch with one job describe the same job (one builder): the integer fields of the record
    agree exactly, the float sums within the bound test_track_batch_eval_gpu.py holds each form to against the float64 sums (its module
    docstring; the single job and the batch of one tile a level alike, so the small-batch depth covers both), the other fields at that
    file's tolerances.
  * a tracker created under LSDHIP_SPIN=0 (the host drains the stream instead of polling the pinned summaries: the branches of the shared
    wait that no other test reaches) gives the results, masks and launch counts of a default tracker, bit for bit, for single jobs and for a
    batch; its summary record is checked all the same (lsdhip_tracker_summary_stats counts it).
  * lsdhip_tracker_evaluate_batch between two identical lsdhip_tracker_track_batch calls leaves the second call's results and
    lsdhip_tracker_launch_stats as they were: the test hook takes no part in the budget history."""
import ctypes as C

import numpy as np
import pytest

from common import sequence
from se3_terms import EPS, point_terms, sums64
from test_track_batch_eval_gpu import AFFINE, C_TERM, IDENT7, Scene, depth_of

pytestmark = pytest.mark.gpu

W, H, JOBS = 160, 128, 8
LSDHIP_OK, LSDHIP_E_ARG, LSDHIP_E_STATE = 0, -1, -3


@pytest.fixture(scope="module")
def hip():
    import lsd_slam_amd as la
    return la


@pytest.fixture(scope="module")
def world(hip):
    """the sequence, a context and a keyframe with ground-truth depth"""
    frames, depth0, K, gt = sequence(W, H, 4, 0)
    ctx = hip.Context(W, H, K)
    kf = hip.Frame(ctx, 1000, frames[0])
    kf.setDepthFromGroundTruth(depth0)
    ref = hip.TrackingReference()
    ref.importFrame(kf)
    return dict(frames=frames, ctx=ctx, ref=ref, gt=gt)


def field_bits(rec):
    return {name: np.array(getattr(rec, name)).tobytes() for name, _ in rec._fields_}


def job_arrays(hip, world, first_id):
    """8 (keyframe, frame) pairs over the sequence's frames 1..3 and their poses"""
    frs = [hip.Frame(world["ctx"], first_id + j, world["frames"][1 + j % 3]) for j in range(JOBS)]
    kfs = (C.c_void_p * JOBS)(*[world["ref"].keyframe.h_] * JOBS)
    fhs = (C.c_void_p * JOBS)(*[f.h_ for f in frs])
    T = np.tile(IDENT7, (JOBS, 1))
    T[1::2, 4] = 0.01                      # every other job a little off
    return frs, kfs, fhs, np.ascontiguousarray(T, np.float32)


def eval_throughput(tr, n, kfs, fhs, T, level, repeats=2):
    ms, nb = C.c_double(float("nan")), C.c_double(float("nan"))
    rc = tr.L.lsdhip_tracker_eval_throughput(tr.h_, n, kfs, fhs, T.ctypes.data, level, repeats, C.byref(ms), C.byref(nb))
    return rc, ms.value, nb.value


def evaluate_batch_rc(tr, n, kfs, fhs, T, level):
    ab = np.ascontiguousarray(np.tile([1.0, 0.0], (n, 1)), np.float32)
    from lsd_slam_amd import capi
    res = (capi.ResidualRecord * n)()
    form = np.zeros((n, 2), np.int32)
    return tr.L.lsdhip_tracker_evaluate_batch(tr.h_, n, kfs, fhs, T.ctypes.data, ab.ctypes.data, level, res, form.ctypes.data)


def track_once(hip, world, tr, frame_id):
    fr = hip.Frame(world["ctx"], frame_id, world["frames"][2])
    tr.trackFrame(world["ref"], fr, IDENT7.astype(np.float64))
    assert not tr.last.diverged
    return field_bits(tr.last), tr.launch_stats()[0]


@pytest.mark.parametrize("refused", ["eval_throughput", "evaluate_batch"])
def test_a_rejected_batch_leaves_nothing_behind(hip, world, refused):
    tr = hip.SE3Tracker(world["ctx"])
    res0, launches0 = track_once(hip, world, tr, 2000)
    frs, kfs, fhs, T = job_arrays(hip, world, 2100)
    if refused == "eval_throughput":
        assert eval_throughput(tr, JOBS, kfs, fhs, T, 0)[0] == LSDHIP_E_STATE       # level 0: no reference blocks, never throughput mode
        assert eval_throughput(tr, JOBS - 1, kfs, fhs, T, 0)[0] == LSDHIP_E_ARG
    else:
        for lvl in (0, 5):                                                           # outside the tracking levels
            assert evaluate_batch_rc(tr, JOBS, kfs, fhs, T, lvl) == LSDHIP_E_ARG
    res1, launches1 = track_once(hip, world, tr, 2001)
    for name in res0:
        assert res0[name] == res1[name], "%s differs after the refused %s" % (name, refused)
    assert launches1 == launches0


def test_eval_throughput_measures_without_disturbing(hip, world):
    tr = hip.SE3Tracker(world["ctx"])
    frs, kfs, fhs, T = job_arrays(hip, world, 2200)
    refs = [world["ref"]] * JOBS
    recs0, form0 = tr.evaluateBatch(refs, frs, T, 1)
    rc, ms, nb = eval_throughput(tr, JOBS, kfs, fhs, T, 1, repeats=2)
    assert rc == LSDHIP_OK
    assert np.isfinite(ms) and ms > 0, ms
    assert np.isfinite(nb) and nb > 0, nb
    recs1, form1 = tr.evaluateBatch(refs, frs, T, 1)
    assert np.array_equal(form0, form1), (form0, form1)
    for j in range(JOBS):
        a, b = field_bits(recs0[j]), field_bits(recs1[j])
        for name in a:
            assert a[name] == b[name], "job %d: %s differs after eval_throughput" % (j, name)


@pytest.fixture(scope="module")
def scene(oracle, hip):
    return Scene(oracle, hip, W, H)


@pytest.mark.parametrize("lvl", [1, 3])
def test_a_single_evaluation_equals_the_batch_of_one(oracle, hip, scene, lvl):
    sc = scene
    tr = hip.SE3Tracker(sc.ctx)
    ro, rg = sc.keyframe("gt", lvl)
    T = sc.poses()[1]
    a, b = AFFINE[1]
    fs = hip.Frame(sc.ctx, 10, sc.frames[1])
    fb = hip.Frame(sc.ctx, 11, sc.frames[1])
    s = tr.evaluate(rg, fs, T, lvl, a, b)
    recs, form = tr.evaluateBatch([rg], [fb], T[None], lvl, np.array([[a, b]], np.float32))
    g = recs[0]
    assert np.all(form == 0), form                               # one job: neither strips nor k_track_solo
    assert s.warped_size == g.warped_size and s.warped_size >= 8
    assert s.goodCount == g.goodCount and s.badCount == g.badCount
    assert s.num_constraints == g.num_constraints
    if lvl == 1:
        assert np.array_equal(fs.refPixelWasGoodNoCreate(), fb.refPixelWasGoodNoCreate())
    fo = oracle.Frame(10, sc.frames[1], sc.K)
    tro = oracle.SE3Tracker(sc.w, sc.h, sc.K, mode=oracle.SSE_EXACT_RCP)
    tro.evaluate(ro, fo, T, lvl, a, b)
    S = sums64(point_terms(tro, fo, lvl, T))
    nc, n4, G = s.num_constraints, S["n4"], S["good"]
    depth = depth_of("small", (W >> lvl) * (H >> lvl), 0) + 1

    def sums(r):
        return {"A": np.array([np.float64(r.A[6 * i + k]) * nc for i in range(6) for k in range(i, 6)]), "b": np.array(r.b, np.float64) * nc,
                "err": np.float64(r.lsError) * nc, "werr": np.float64(r.weightedError) * n4}
    ds, dg = sums(s), sums(g)
    for k in ("A", "b", "err", "werr"):
        bound = (depth + C_TERM[k]) * EPS * S[k + "_abs"] + 1e-30
        ratio = float(np.max(np.abs(ds[k] - dg[k]) / bound))
        print("level %d %s: |single - batch of one| / bound = %.3g" % (lvl, k, ratio))
        assert ratio <= 1, (lvl, k, ratio, ds[k], dg[k])
    bound = (depth + 1) * EPS * S["res2_abs"] + EPS * abs(S["res2"])
    assert abs(np.float64(s.retval) - np.float64(g.retval)) * G <= bound
    M = s.warped_size
    assert g.pointUsage == pytest.approx(s.pointUsage, rel=max(2e-5, 2 * M * EPS))
    assert g.meanRes == pytest.approx(s.meanRes, rel=max(1e-3, 2 * M * EPS), abs=1e-4)
    assert g.affine_a_lastIt == pytest.approx(s.affine_a_lastIt, rel=5e-4)
    assert g.affine_b_lastIt == pytest.approx(s.affine_b_lastIt, abs=0.08)


def spin_pair(hip, world, monkeypatch):
    """a default tracker and one that does not poll (the environment is read when the tracker is created)"""
    tr_a = hip.SE3Tracker(world["ctx"])
    monkeypatch.setenv("LSDHIP_SPIN", "0")
    tr_b = hip.SE3Tracker(world["ctx"])
    monkeypatch.delenv("LSDHIP_SPIN")
    return tr_a, tr_b


def track_batch(hip, world, tr, first_id):
    """trackFrameBatch of the 8 jobs of job_arrays (fresh frames); returns the records' bits, the masks and launch_stats"""
    frs, _, _, T = job_arrays(hip, world, first_id)
    inits = T.astype(np.float64)                       # (the same small offsets, taken as frameToReference)
    _, res = tr.trackFrameBatch([world["ref"]] * JOBS, frs, inits)
    assert not any(r.diverged for r in res)
    return [field_bits(r) for r in res], [f.refPixelWasGoodNoCreate() for f in frs], tr.launch_stats()


def assert_same_batch(a, b, what):
    for j in range(JOBS):
        for name in a[0][j]:
            assert a[0][j][name] == b[0][j][name], "job %d: %s differs %s" % (j, name, what)
        assert np.array_equal(a[1][j], b[1][j]), "job %d: refPixelWasGood differs %s" % (j, what)
    assert a[2] == b[2], (what, a[2], b[2])


def test_polling_off_changes_nothing(hip, world, monkeypatch):
    tr_a, tr_b = spin_pair(hip, world, monkeypatch)
    for i in (1, 2, 3):
        fa, fb = hip.Frame(world["ctx"], 3000 + i, world["frames"][i]), hip.Frame(world["ctx"], 3000 + i, world["frames"][i])
        tr_a.trackFrame(world["ref"], fa, IDENT7.astype(np.float64))
        tr_b.trackFrame(world["ref"], fb, IDENT7.astype(np.float64))
        assert not tr_a.last.diverged
        a, b = field_bits(tr_a.last), field_bits(tr_b.last)
        for name in a:
            assert a[name] == b[name], "frame %d: %s differs without polling" % (i, name)
        assert np.array_equal(fa.refPixelWasGoodNoCreate(), fb.refPixelWasGoodNoCreate()), i
        assert tr_a.launch_stats()[0] == tr_b.launch_stats()[0] > 0, (i, tr_a.launch_stats(), tr_b.launch_stats())
    assert_same_batch(track_batch(hip, world, tr_a, 3100), track_batch(hip, world, tr_b, 3100), "without polling")


def test_batch_evaluation_leaves_launch_stats_alone(hip, world):
    tr = hip.SE3Tracker(world["ctx"])
    first = track_batch(hip, world, tr, 3200)
    assert first[2][0] > 0
    frs, _, _, T = job_arrays(hip, world, 3300)
    tr.evaluateBatch([world["ref"]] * JOBS, frs, T, 2)
    assert tr.launch_stats() == first[2]
    assert_same_batch(first, track_batch(hip, world, tr, 3200), "after evaluateBatch")


def test_a_summary_is_checked_with_and_without_polling(hip, world, monkeypatch):
    for tr in spin_pair(hip, world, monkeypatch):
        assert tr.summary_stats()[0] == 0
        track_once(hip, world, tr, 3400)
        assert tr.summary_stats()[0] == 1, tr.summary_stats()
