"""The keyframe bank (lsdhip_kfbank_*) and the batched entries over it, bit for bit against the host-cloud entries they replace.

  put / download        == lsdhip_ref_pointcloud(kf, 4): count, order (x outer, y inner) and bits
  check_overlap_bank    == lsdhip_tracker_check_overlap on the downloaded cloud, pair by pair
  track_permaref_bank   == lsdhip_tracker_track_permaref_batch on the downloaded clouds, job by job

Sizes cover every lane shape of the compaction (lane = level-4 column) and of the overlap sum (lane-strided over the points): 160x128
(level 4 = 10x8: fewer than 64 points), 176x144 (odd level width 11), 640x480 (40x30: up to 1064 points, five strided passes with a
ragged tail), 1280x1024 (80x64: thousands of points).  The level-0 depth planes are made from a level-4 mask (a 16x16 block per cell), so
that the level-4 pattern is under the test's control: random semi-dense cells, an empty column, valid cells in the first and last interior
column and row, valid cells ON the border (which makePointCloud never takes), a cell with idepth == 0 and positive variance (skipped), an
all-invalid plane (0 points) and an all-valid one (the slot's full capacity).  Each test checks on the downloaded level-4 planes that its
pattern is really there."""
import numpy as np
import pytest

import reposition_ref as rr
from common import assert_bit_equal
from lsd_slam_amd import synth

pytestmark = pytest.mark.gpu

SIZES = [(160, 128), (176, 144), (640, 480), (1280, 1024)]


@pytest.fixture(scope="module")
def hip():
    import lsd_slam_amd as la
    return la


def planes_from_cells(rng, w, h, cells, zero_cell=None):
    """level-0 (idepth, idepthVar) whose level-4 cell (y, x) is valid iff cells[y, x]; inside a valid cell half of the pixels carry a
    hypothesis.  zero_cell: a cell whose hypotheses all have idepth 0 (variance positive)."""
    valid = np.kron(cells.astype(np.uint8), np.ones((16, 16), np.uint8)).astype(bool) & (rng.uniform(size=(h, w)) < 0.5)
    idepth = np.where(valid, rng.uniform(0.2, 2.0, (h, w)), -1.0).astype(np.float32)
    var = np.where(valid, rng.uniform(0.001, 0.1, (h, w)), -1.0).astype(np.float32)
    if zero_cell is not None:
        y, x = zero_cell
        idepth[16 * y:16 * y + 16, 16 * x:16 * x + 16][valid[16 * y:16 * y + 16, 16 * x:16 * x + 16]] = 0.0
    return idepth, var


class World:
    """one context per size with four keyframes: ragged, empty, full, ragged again"""

    def __init__(self, hip, w, h):
        self.w, self.h, self.w4, self.h4 = w, h, w >> 4, h >> 4
        self.ctx = hip.Context(w, h, synth.intrinsics(w, h))
        rng = np.random.default_rng(w * 7 + h)
        w4, h4 = self.w4, self.h4
        ragged = rng.uniform(size=(h4, w4)) < 0.4
        ragged[:, 3] = False                                  # an empty interior column
        ragged[1, 1] = ragged[h4 - 2, w4 - 2] = ragged[1, w4 - 2] = ragged[h4 - 2, 1] = True   # first / last interior column and row
        ragged[0, :] = ragged[h4 - 1, :] = True               # the border is valid and must not be taken
        ragged[:, 0] = ragged[:, w4 - 1] = True
        self.zero_cell = (2, 5)
        ragged[self.zero_cell] = True
        ragged2 = rng.uniform(size=(h4, w4)) < 0.7
        self.cells = [ragged, np.zeros((h4, w4), bool), np.ones((h4, w4), bool), ragged2]
        self.kfs = []
        for k, cells in enumerate(self.cells):
            f = hip.Frame(self.ctx, 10 + k, rng.integers(0, 256, (h, w), dtype=np.uint8))
            f.setDepthPlanes(*planes_from_cells(rng, w, h, cells, self.zero_cell if k == 0 else None))
            self.kfs.append(f)
        self.rng = rng
        self.tracker = hip.SE3Tracker(self.ctx)

    def reference_cloud(self, hip, kf):
        ref = hip.TrackingReference()
        ref.keyframe = kf
        pos, cv, _, _ = ref.makePointCloud(4)
        return pos, cv


WORLDS = {}


@pytest.fixture(params=SIZES, ids=lambda s: "%dx%d" % s)
def world(request, hip):
    if request.param not in WORLDS:
        WORLDS[request.param] = World(hip, *request.param)
    return WORLDS[request.param]


def test_put_equals_ref_pointcloud(hip, world):
    wd = world
    bank = hip.KeyFrameBank(wd.ctx, 4)
    capacity = (wd.w4 - 2) * (wd.h4 - 2)
    counts = []
    for k, kf in enumerate(wd.kfs):
        pos, cv = wd.reference_cloud(hip, kf)
        slot = bank.put(kf)
        assert slot == k == kf.idxInKeyframes
        gpos, gcv = bank.download(slot)
        assert len(gpos) == len(pos), (k, len(gpos), len(pos))
        assert_bit_equal(gpos, pos, "keyframe %d pos" % k)
        assert_bit_equal(gcv, cv, "keyframe %d colorAndVar" % k)
        info = bank.info(slot)
        assert info["frameId"] == kf.id() and info["numPoints"] == len(pos)
        assert info["meanIdepth"] == np.float32(kf.stats()["meanIdepth"])
        assert np.array_equal(info["camToWorld"], [1, 0, 0, 0, 0, 0, 0, 1])
        counts.append(len(pos))
    assert bank.size() == 4
    # the patterns the planes were built for are there
    id4, var4 = wd.kfs[0].idepth(4), wd.kfs[0].idepthVar(4)
    ok = (var4 > 0) & (id4 != 0)
    inner = ok[1:-1, 1:-1]
    assert counts[0] == int(inner.sum()) and counts[1] == 0 and counts[2] == capacity
    assert not inner[:, 2].any() and ok[1, 1] and ok[-2, -2] and ok[1, -2] and ok[-2, 1]
    assert ok[0, :].all() and ok[-1, :].all() and ok[:, 0].all() and ok[:, -1].all()
    assert var4[wd.zero_cell] > 0 and id4[wd.zero_cell] == 0
    if (wd.w, wd.h) == (160, 128):
        assert 0 < counts[0] < 64 and capacity < 64
    if (wd.w, wd.h) == (640, 480):
        assert capacity == 1064 and counts[3] > 512 and counts[3] % 256 != 0
    if (wd.w, wd.h) == (1280, 1024):
        assert counts[3] > 2000
    bank.setMeta(2, [1, 0, 0, 0, 1, 2, 3, 1.5], 0.25)
    assert bank.info(2)["meanIdepth"] == 0.25 and np.array_equal(bank.info(2)["camToWorld"], [1, 0, 0, 0, 1, 2, 3, 1.5])
    bank.setMeta(2, [1, 0, 0, 0, 0, 0, 0, 1], -1.0)
    assert bank.info(2)["meanIdepth"] == 0.25
    bank.close()


def test_slots_are_isolated_and_the_bank_has_an_end(hip, world):
    wd = world
    bank = hip.KeyFrameBank(wd.ctx, 3)
    for k in (0, 2, 3):
        bank.put(wd.kfs[k])
    before = [bank.download(s) for s in range(3)]
    # the full middle slot is replaced by a sparse cloud of the same frame id
    again = hip.Frame(wd.ctx, wd.kfs[2].id(), wd.rng.integers(0, 256, (wd.h, wd.w), dtype=np.uint8))
    again.setDepthPlanes(*planes_from_cells(wd.rng, wd.w, wd.h, wd.cells[3]))
    assert bank.put(again) == 1 and bank.size() == 3
    pos, cv = wd.reference_cloud(hip, again)
    gpos, gcv = bank.download(1)
    assert 0 < len(pos) < len(before[1][0])
    assert_bit_equal(gpos, pos, "replaced slot pos")
    assert_bit_equal(gcv, cv, "replaced slot colorAndVar")
    # back to the full cloud: every point of the slot's capacity is written again
    assert bank.put(wd.kfs[2]) == 1
    with pytest.raises(hip.LsdHipError):
        bank.put(wd.kfs[1])            # a fourth frame id
    assert bank.size() == 3
    for s in range(3):
        gpos, gcv = bank.download(s)
        assert_bit_equal(gpos, before[s][0], "slot %d pos" % s)
        assert_bit_equal(gcv, before[s][1], "slot %d colorAndVar" % s)
    bank.close()


def test_check_overlap_bank_equals_the_single_call(hip, oracle, world):
    wd = world
    bank = hip.KeyFrameBank(wd.ctx, 4)
    for kf in wd.kfs:
        bank.put(kf)
    clouds = [bank.download(s)[0] for s in range(4)]
    rng = np.random.default_rng(11)
    filled = [0, 2, 3]
    for n in (1, 7, 64):
        slots = [filled[j % 3] for j in range(n)]
        poses = [oracle.se3_exp(np.concatenate([rng.normal(0, 0.2, 3), rng.normal(0, 0.05, 3)])) for _ in range(n)]
        if n >= 7:
            slots[:5] = [2, 2, 2, 0, 3]                                   # one slot under several poses
            poses[3] = np.array([1.0, 0, 0, 0, 1e4, 0, 0])                # every point projects outside
            poses[4] = np.array([1.0, 0, 0, 0, 0, 0, -100.0])             # behind the camera
        got = wd.tracker.checkPermaRefOverlapBank(bank, slots, poses)
        want = np.array([wd.tracker.checkPermaRefOverlap(clouds[s], T) for s, T in zip(slots, poses)], np.float32)
        assert_bit_equal(got, want, "n = %d" % n)
        if n >= 7:
            assert got[3] == 0.0 and np.count_nonzero(got) >= n // 2
    with pytest.raises(hip.LsdHipError):
        wd.tracker.checkPermaRefOverlapBank(bank, [0, 1], [poses[0], poses[0]])      # slot 1 holds no point
    with pytest.raises(hip.LsdHipError):
        wd.tracker.checkPermaRefOverlapBank(bank, [4], [poses[0]])
    bank.close()


RESULT_FIELDS = ("pointUsage", "lastGoodCount", "lastBadCount", "lastMeanRes", "lastResidual", "affineEstimation_a", "affineEstimation_b",
                 "diverged", "trackingWasGood", "numEvaluations", "numWarpUpdates")


@pytest.fixture(scope="module")
def scene(hip, oracle):
    """scenario A's views at 640x480: slots 0 .. 7 = its keyframes 8 .. 15 (ground-truth depth), the query frame, refToFrame per slot"""
    K, kviews, q = rr.scenario_a_inputs()
    ctx = hip.Context(rr.W, rr.H, K)
    bank = hip.KeyFrameBank(ctx, 8)
    kfs, T0 = [], []
    for i, img, depth, pose in kviews[8:]:
        f = hip.Frame(ctx, i, img)
        f.setDepthFromGroundTruth(depth)
        bank.put(f)
        kfs.append(f)
        rel = rr.sim3_mul(rr.sim3_inv(pose), q[3])
        T0.append(oracle.se3_inv(synth.pose7(rel[1], rel[2])))
    return ctx, bank, kfs, hip.Frame(ctx, q[0], q[1]), T0


@pytest.mark.parametrize("n", [1, 3, 8, 24, 40])
def test_track_permaref_bank_equals_the_host_cloud_batch(hip, oracle, scene, n):
    ctx, bank, kfs, frame, T0 = scene
    rng = np.random.default_rng(n)
    slots = [(3 * j + 1) % 8 for j in range(n)]
    poses = [oracle.se3_mul(oracle.se3_exp(np.concatenate([rng.normal(0, 0.01, 3), rng.normal(0, 0.003, 3)])), T0[s]) for s in slots]
    clouds = [bank.download(s) for s in slots]
    assert len({len(c[0]) for c in clouds}) > 1 or n == 1            # clouds of different sizes share the launches
    ta, tb = hip.SE3Tracker(ctx), hip.SE3Tracker(ctx)
    gp, gr = ta.trackFrameOnPermarefBank(bank, slots, [frame] * n, poses)
    wp, wr = tb.trackFrameOnPermarefBatch(clouds, [frame] * n, poses)
    assert np.array_equal(gp, wp), np.argwhere(gp != wp)[:4]
    for j in range(n):
        for k in RESULT_FIELDS:
            a, b = getattr(gr[j], k), getattr(wr[j], k)
            assert a == b or (a != a and b != b), (j, k, a, b)
    assert any(r.trackingWasGood for r in gr) and all(r.numEvaluations > 0 for r in gr)
