"""Who owns what on the device: every allocation, pinned block, event and stream the library creates is counted while it lives
(lsdhip_live_resources), and a creation can be refused from the outside without the runtime being asked
(lsdhip_devtest_fail_alloc_after).  On 160x128 images, the smallest size of the suite:

  * round trip: a context, one object of every kind and one call of every kind that creates storage on first use; after the objects and
    the context are destroyed the four counts are back where they started, and a second round in the same process peaks where the first did
  * every creator, refused at its first, second, ... creation until it succeeds: LSDHIP_E_HIP, *out untouched, counts unchanged
  * a growth refused half-way (the Sim3 tracker's job storage, the kernel-argument ring): counts unchanged, and the same call repeated
    gives bit for bit what an object that never saw a refusal gives.

The counts are process-wide, so each test measures against a baseline it takes itself, with the garbage collector held off (the wrappers of
other tests' objects free their handles when they are collected)."""
import ctypes as C
import gc

import numpy as np
import pytest

from common import sequence
from lsd_slam_amd import capi

pytestmark = pytest.mark.gpu

W, H = 160, 128
S = 4                      # maps: from LSD_OBS_SPLIT_MIN_MAPS on a batched update takes its two-launch observe (queues, sampled counters)
WIDE = 320                 # frames whose argument records (224 bytes each) need more than the ring's first 64 KiB slots
E_HIP = -2
SENTINEL = 0xDEAD0


@pytest.fixture(scope="module")
def hip():
    import lsd_slam_amd as la
    return la


@pytest.fixture(autouse=True)
def quiet_collector():
    gc.collect()
    gc.disable()
    yield
    capi.lib().lsdhip_devtest_fail_alloc_after(-1)
    gc.enable()


def live():
    out = (C.c_longlong * 4)()
    capi.lib().lsdhip_live_resources(C.byref(out))
    return tuple(out)


def remap_tables():
    """a camera 8 pixels larger each way, every output pixel between four raw ones"""
    x, y = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    return W + 8, H + 8, x + 2.5, y + 3.25


def round_trip(hip):
    """-> the counts at the peak, just before anything is destroyed"""
    L = capi.lib()
    seqs = [sequence(W, H, 3, j) for j in range(S)]
    ctx = hip.Context(W, H, seqs[0][2])
    ctx.set_pipeline(True)                     # the mapping stream and its event ring ...
    ctx.set_pipeline(False)                    # ... which the context keeps
    ctx.lanes_begin(2)
    ctx.lane_select(1)
    ctx.lanes_end()
    capi.check(L.lsdhip_ctx_aux_begin(ctx.h_))
    capi.check(L.lsdhip_ctx_aux_end(ctx.h_))
    capi.check(L.lsdhip_ctx_aux_join(ctx.h_))
    flag = C.c_void_p()
    capi.check(L.lsdhip_ctx_alloc_dev(ctx.h_, 64, C.byref(flag)))
    capi.check(L.lsdhip_ctx_memset_dev(ctx.h_, flag, 0, 64))
    capi.check(L.lsdhip_ctx_flag_set(ctx.h_, flag, 1))
    ctx.synchronize()
    capi.check(L.lsdhip_ctx_free_dev(ctx.h_, flag))
    ctx.prof_enable(True)

    tracker, sim3, bank = hip.SE3Tracker(ctx), hip.Sim3Tracker(ctx), hip.KeyFrameBank(ctx, 4)
    tracker.set_maxItsPerLvl([5, 20, 50, 100, 0])
    cloud = hip.PointCloud(ctx, 4096, 4)
    in_w, in_h, rx, ry = remap_tables()
    und = hip.Undistorter(ctx, in_w, in_h, rx, ry)
    maps, refs, kfs = [], [], []
    for frames, depth0, _, _ in seqs:
        kf = hip.Frame(ctx, 0, frames[0])
        kf.setDepthFromGroundTruth(depth0)     # staging plane of set_depth_gt
        dm = hip.DepthMap(ctx)
        dm.initializeFromGTDepth(kf)
        ref = hip.TrackingReference()
        ref.importFrame(kf)
        maps.append(dm), refs.append(ref), kfs.append(kf)
    keep = []
    f1 = hip.Frame.createBatch(ctx, [1] * S, images=[s[0][1] for s in seqs])
    poses, _ = tracker.trackFrameBatch(refs, f1, [hip.slam.IDENTITY] * S)      # a tracker batch
    hip.DepthMap.updateKeyframeBatch(maps, f1)                                   # one batched update, sampled
    f2 = hip.Frame.createBatch(ctx, [2] * S, images=[s[0][2] for s in seqs])
    tracker.trackFrameBatch(refs, f2, poses)
    hip.DepthMap.changeKeyframeBatch(maps, f2)                                   # one keyframe change
    keep += f1 + f2
    kfs[0].keyframePoints()
    maps[0].debugPlotDepthMap()
    sim3.trackFrameSim3(kfs[0], f2[0], np.array([1.0, 0, 0, 0, 0, 0, 0, 1.0]), 3, 1)
    tracker.trackFrame(refs[1], f1[1], hip.slam.IDENTITY)
    slot = bank.put(kfs[0])
    tracker.checkPermaRefOverlapBank(bank, [slot], [hip.slam.IDENTITY])
    cloud.appendKeyframe(kfs[0], np.array([0, 0, 0, 1, 0, 0, 0], np.float32))
    raw = np.random.default_rng(3).integers(0, 256, (in_h, in_w), dtype=np.uint8)
    keep.append(und.frame(7, raw))
    und.apply(raw)
    keep += hip.Frame.createBatch(ctx, list(range(100, 100 + WIDE)), images=[seqs[0][0][j % 3] for j in range(WIDE)])
    ctx.synchronize()
    peak = live()

    for f in keep + kfs:
        f.close()
    for o in maps + [und, cloud, bank, tracker]:
        o.close()
    del sim3
    ctx.close()
    return peak


def test_round_trip_returns_every_resource(hip):
    base = live()
    first = round_trip(hip)
    assert live() == base, "after the first round"
    assert all(p > b for p, b in zip(first, base)), (first, base)       # device, pinned, events and streams were all in play
    second = round_trip(hip)
    assert live() == base, "after the second round"
    assert second == first


def _creators(L, ctx, world):
    """name -> (create(out) -> rc, destroy(handle)) on the context `ctx`; `world` keeps the creators' inputs alive"""
    K, img = world["K"], world["img"]
    in_w, in_h, rx, ry = world["remap"]
    return {
        "ctx": (lambda out: L.lsdhip_ctx_create(0, W, H, K.ctypes.data, None, C.byref(out)), L.lsdhip_ctx_destroy),
        "frame": (lambda out: L.lsdhip_frame_create(ctx, 5, img.ctypes.data, C.byref(out)), L.lsdhip_frame_destroy),
        "tracker": (lambda out: L.lsdhip_tracker_create(ctx, C.byref(out)), L.lsdhip_tracker_destroy),
        "sim3tracker": (lambda out: L.lsdhip_sim3tracker_create(ctx, C.byref(out)), L.lsdhip_sim3tracker_destroy),
        "depthmap": (lambda out: L.lsdhip_depth_create(ctx, C.byref(out)), L.lsdhip_depth_destroy),
        "kfbank": (lambda out: L.lsdhip_kfbank_create(ctx, 4, C.byref(out)), L.lsdhip_kfbank_destroy),
        "cloud": (lambda out: L.lsdhip_cloud_create(ctx, 4096, 4, C.byref(out)), L.lsdhip_cloud_destroy),
        "undistorter": (lambda out: L.lsdhip_undistorter_create(ctx, in_w, in_h, rx.ctypes.data, ry.ctypes.data, C.byref(out)), L.lsdhip_undistorter_destroy),
    }


@pytest.fixture(scope="module")
def world(hip):
    frames, depth0, K, _ = sequence(W, H, 3, 0)
    in_w, in_h, rx, ry = remap_tables()
    wd = {"ctx": hip.Context(W, H, K), "K": np.ascontiguousarray(K, np.float32), "img": np.ascontiguousarray(frames[0]),
          "remap": (in_w, in_h, np.ascontiguousarray(rx), np.ascontiguousarray(ry)), "frames": frames, "depth0": depth0}
    yield wd
    wd["ctx"].close()


@pytest.mark.parametrize("name", ["ctx", "frame", "tracker", "sim3tracker", "depthmap", "kfbank", "cloud", "undistorter"])
def test_a_refused_create_leaves_nothing_behind(hip, world, name):
    L = capi.lib()
    base = live()
    own = hip.Context(W, H, world["K"])       # a context of the test's own: its frame pool is empty
    create, destroy = _creators(L, own.h_, world)[name]
    before = live()
    k = 0
    while True:
        out = C.c_void_p(SENTINEL)
        L.lsdhip_devtest_fail_alloc_after(k)
        rc = create(out)
        L.lsdhip_devtest_fail_alloc_after(-1)
        if rc == 0:
            break
        assert rc == E_HIP, "refused at creation %d: rc %d" % (k, rc)
        assert out.value == SENTINEL, "refused at creation %d: *out written" % k
        assert live() == before, "refused at creation %d" % k
        k += 1
        assert k < 64
    assert k >= 1, "the creator made nothing through the library's helpers"
    assert out.value not in (None, SENTINEL) and live() != before
    destroy(out)
    # (a destroyed frame's arena waits in its context's pool: one device allocation, which goes with the context)
    assert live() == ((before[0] + 1,) + before[1:] if name == "frame" else before)
    own.close()
    assert live() == base


def _sim3_bits(r):
    return bytes(r)


def test_a_refused_sim3_job_storage_growth(hip, world):
    """the first trackFrameSim3 of a tracker makes its job storage (four blocks): refused at each of them in turn"""
    ctx, frames, depth0 = world["ctx"], world["frames"], world["depth0"]
    kf, fr = hip.Frame(ctx, 0, frames[0]), hip.Frame(ctx, 1, frames[1])
    kf.setDepthFromGroundTruth(depth0)
    fr.setDepthFromGroundTruth(depth0)
    init = np.array([1.0, 0, 0, 0, 0, 0, 0, 1.0])
    fresh = hip.Sim3Tracker(ctx)
    want = _sim3_bits(fresh.trackFrameSim3(kf, fr, init, 3, 1)[1])
    tr = hip.Sim3Tracker(ctx)
    before = live()
    L = capi.lib()
    for k in range(4):
        L.lsdhip_devtest_fail_alloc_after(k)
        with pytest.raises(capi.LsdHipError, match="failed: "):
            tr.trackFrameSim3(kf, fr, init, 3, 1)
        L.lsdhip_devtest_fail_alloc_after(-1)
        assert live() == before, "refused at block %d" % k
    assert _sim3_bits(tr.trackFrameSim3(kf, fr, init, 3, 1)[1]) == want
    assert live() != before
    del tr, fresh
    kf.close(), fr.close()


def test_a_refused_argument_ring_growth(hip, world):
    """a frame batch whose records outgrow the ring's slots: the growth makes a pinned block and its device twin"""
    frames, K = world["frames"], world["K"]
    images = [frames[j % 3] for j in range(WIDE)]
    ids = list(range(WIDE))

    def planes(fs):
        return [fs[j].image(l).tobytes() for j in (0, 1, WIDE // 2, WIDE - 1) for l in (0, 4)] + [fs[WIDE - 1].gradients(1).tobytes()]

    fresh_ctx = hip.Context(W, H, K)
    fresh = hip.Frame.createBatch(fresh_ctx, ids, images=images)
    want = planes(fresh)
    for f in fresh:
        f.close()
    fresh_ctx.close()

    ctx = hip.Context(W, H, K)
    ctx.reserve_frames(WIDE)                   # the arenas are there: only the ring has anything to create
    for f in hip.Frame.createBatch(ctx, [0, 1], images=images[:2]):      # the ring at its first size, with its events
        f.close()
    before = live()
    L = capi.lib()
    for k in range(2):
        L.lsdhip_devtest_fail_alloc_after(k)
        with pytest.raises(capi.LsdHipError, match="failed: "):
            hip.Frame.createBatch(ctx, ids, images=images)
        L.lsdhip_devtest_fail_alloc_after(-1)
        assert live() == before, "refused at block %d" % k
    small = hip.Frame.createBatch(ctx, [0, 1], images=images[:2])         # the old ring still serves
    assert small[1].image(4).tobytes() == want[3]
    for f in small:
        f.close()
    fs = hip.Frame.createBatch(ctx, ids, images=images)
    assert planes(fs) == want
    assert live() == before        # the new pair took the old one's place
    for f in fs:
        f.close()
    ctx.close()

