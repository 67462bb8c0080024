"""DepthMap::debugPlotDepthMap on the device (lsdhip_depth_debug_plot*, csrc/plot.hip) against tests/depth_plot_ref.py, the numpy
restatement that tests/test_depth_plot_ref_cpu.py pins to the reference's compiled colour function and to plotDepthMap of
include/lsd_slam_hip_io.hpp.  Maps are planted with lsdhip_depth_upload; every comparison is == on the bytes (for modes 3 / 4 the CPU file
checks that no pixel of these maps depends on the last bits of the double logarithm)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import depth_plot_ref as dp
from common import ROOT, sequence, synth

pytestmark = pytest.mark.gpu

K_OF = lambda w, h: np.array([0.8 * w, 0.82 * w, 0.5 * w - 0.5, 0.5 * h - 0.5], np.float32)
ALL_MODES = dp.MODES + (dp.WHITE_MODE,)
E_ARG, E_STATE = -1, -3

_CTX, _IMG, _REF = {}, {}, {}


def ctx_of(w, h):
    import lsd_slam_amd as la
    if (w, h) not in _CTX:
        _CTX[(w, h)] = la.Context(w, h, K_OF(w, h))
    return _CTX[(w, h)]


def image_of(w, h):
    if (w, h) not in _IMG:
        _IMG[(w, h)] = np.ascontiguousarray(synth.make_sequence(w, h, 1)[0][0])
    return _IMG[(w, h)]


def planted(ctx, k=0, frame_id=1):
    """a depth map holding dp.gpu_map(w, h, k) on a keyframe with the size's test image -> (DepthMap, Frame, hypotheses)"""
    import lsd_slam_amd as la
    w, h = ctx.w, ctx.h
    hyp = dp.gpu_map(w, h, k)
    kf = la.Frame(ctx, frame_id, image_of(w, h))
    dm = la.DepthMap(ctx)
    dm.setCurrentDepthMap(kf, hyp)
    return dm, kf, hyp


def expected(w, h, mode, k=0, ref_id=0):
    """the restatement on map k (computed once per case, shared by the tests)"""
    key = (w, h, mode, k, ref_id)
    if key not in _REF:
        _REF[key] = dp.plot_ref(dp.gpu_map(w, h, k), image_of(w, h).astype(np.float32), mode, ref_id)
    return _REF[key]


def assert_same_image(got, want, what=""):
    ne = (got != want).any(axis=2)
    assert got.shape == want.shape and not ne.any(), "%s: %d pixels differ, first at %s: %r vs %r" % (
        what, int(ne.sum()), np.argwhere(ne)[0], got[ne][0], want[ne][0])


class DeviceImages:
    """n device buffers of 3 * w * h bytes on a context (lsdhip_ctx_alloc_dev), read back with lsdhip_ctx_read_dev"""

    def __init__(self, ctx, n):
        from lsd_slam_amd.capi import check
        self.ctx, self.check, self.ptrs = ctx, check, []
        for _ in range(n):
            p = ctypes.c_void_p()
            check(ctx.L.lsdhip_ctx_alloc_dev(ctx.h_, 3 * ctx.w * ctx.h, ctypes.byref(p)), False)
            self.ptrs.append(p.value)

    def read(self, j):
        out = np.zeros((self.ctx.h, self.ctx.w, 3), np.uint8)
        self.check(self.ctx.L.lsdhip_ctx_read_dev(self.ctx.h_, out.ctypes.data, ctypes.c_void_p(self.ptrs[j]), out.nbytes), False)
        return out

    def free(self):
        for p in self.ptrs:
            self.check(self.ctx.L.lsdhip_ctx_free_dev(self.ctx.h_, ctypes.c_void_p(p)), False)
        self.ptrs = []


CASES = [(size, mode) for size in dp.GPU_SIZES[:2] for mode in ALL_MODES] + [(dp.GPU_SIZES[2], 0), (dp.GPU_SIZES[2], 3)]


@pytest.fixture(scope="module")
def maps():
    """one planted map per size, shared by the per-mode cases (the call reads only: test_the_call_only_reads)"""
    held = {}

    def get(w, h):
        if (w, h) not in held:
            dm, kf, hyp = planted(ctx_of(w, h))
            assert dm.currentDepthMap().tobytes() == hyp.tobytes()        # the planted bytes are what the map holds
            held[(w, h)] = (dm, kf, hyp)
        return held[(w, h)]
    yield get
    held.clear()


@pytest.mark.parametrize("size,mode", CASES)
def test_image_equals_the_restatement(maps, size, mode):
    w, h = size
    dm, kf, hyp = maps(w, h)
    valid = hyp["isValid"] != 0
    assert 0.33 < valid.mean() < 0.37
    for b in (0, -1, -2):
        assert ((hyp["blacklisted"] == b) & valid).any() and ((hyp["blacklisted"] == b) & ~valid).any()
    for v in dp.PLANTED_IDEPTH:
        assert (hyp["idepth"][valid].view(np.uint32) == np.float32(v).view(np.uint32)).any()
    for v in dp.PLANTED_VAR:
        assert (hyp["idepth_var"][valid] == np.float32(v)).any()
    want = expected(w, h, mode)
    got = dm.debugPlotDepthMap(mode)
    assert got.dtype == np.uint8 and got.shape == (h, w, 3)
    assert_same_image(got, want, "%dx%d mode %d" % (w, h, mode))
    # the image is what the mode is for: grey where nothing is valid, colour (or white) on the hypotheses
    grey = image_of(w, h)
    plain = ~valid if mode != 2 else ~valid & ~(hyp["blacklisted"] < dp.MIN_BLACKLIST)
    assert (got[plain] == grey[plain][:, None]).all()
    if mode == dp.WHITE_MODE:
        assert (got[valid] == 255).all()
    else:
        assert len(np.unique(got[valid], axis=0)) > 50


def test_ref_id_is_the_oldest_frame_of_the_last_update():
    import lsd_slam_amd as la
    w, h = 160, 128
    frames, depth0, K, gt = sequence(w, h, 3)
    ctx = la.Context(w, h, K)
    kf = la.Frame(ctx, 0, frames[0])
    kf.setDepthFromGroundTruth(depth0)
    dm = la.DepthMap(ctx)
    dm.initializeFromGTDepth(kf)
    img0 = np.ascontiguousarray(frames[0]).astype(np.float32)
    # before any update: refID = 0
    before = dm.currentDepthMap()
    assert_same_image(dm.debugPlotDepthMap(5), dp.plot_ref(before, img0, 5, 0), "before the first update")
    ref = la.TrackingReference()
    ref.importFrame(kf)
    tracker = la.SE3Tracker(ctx)
    tracker.set_maxItsPerLvl([5, 20, 50, 100, 0])
    f = la.Frame(ctx, 37, frames[2])
    tracker.trackFrame(ref, f, la.IDENTITY)
    dm.updateKeyframe([f])
    after = dm.currentDepthMap()
    nid = after["nextStereoFrameMinID"][after["isValid"] != 0]
    assert (nid > 37).sum() > 100           # the update scheduled next stereo frames behind frame 37: mode 5 has something to show
    got = dm.debugPlotDepthMap(5)
    want = dp.plot_ref(after, img0, 5, 37)
    assert_same_image(got, want, "after an update with frame 37")
    assert (want != dp.plot_ref(after, img0, 5, 0)).any()      # (refID = 0 would show)
    # the batched update keeps it too
    g = la.Frame(ctx, 41, frames[1])
    tracker.trackFrame(ref, g, la.IDENTITY)
    la.DepthMap.updateKeyframeBatch([dm], [g])
    after2 = dm.currentDepthMap()
    assert_same_image(dm.debugPlotDepthMap(5), dp.plot_ref(after2, img0, 5, 41), "after a batched update with frame 41")


@pytest.mark.parametrize("n", [1, 3, 33])
def test_batch_equals_the_single_calls(n):
    import lsd_slam_amd as la
    w, h = dp.GPU_BATCH_SIZE
    assert n <= dp.GPU_BATCH_MAPS
    ctx = ctx_of(w, h)
    held = [planted(ctx, k, frame_id=k + 1) for k in range(n)]
    dms = [x[0] for x in held]
    bufs = DeviceImages(ctx, n + 1)
    try:
        for mode in (0, 2) if n > 1 else (4,):
            la.DepthMap.debugPlotDepthMapBatch(dms, bufs.ptrs[:n], mode)
            singles = [dm.debugPlotDepthMap(mode) for dm in dms]
            for k in range(n):
                assert_same_image(bufs.read(k), singles[k], "batch of %d, map %d, mode %d" % (n, k, mode))
                assert_same_image(singles[k], expected(w, h, mode, k), "map %d, mode %d" % (k, mode))
            if n > 1:
                assert (singles[0] != singles[1]).any()
        # the device-output form of the single call
        assert dms[0].debugPlotDepthMap(3, out_dev_ptr=bufs.ptrs[n]) is None
        assert_same_image(bufs.read(n), dms[0].debugPlotDepthMap(3), "device-output form")
    finally:
        bufs.free()


def test_the_call_only_reads():
    w, h = 176, 144
    dm, kf, hyp = planted(ctx_of(w, h))
    before = dm.currentDepthMap().tobytes()
    assert before == hyp.tobytes()
    for mode in ALL_MODES:
        dm.debugPlotDepthMap(mode)
    assert dm.currentDepthMap().tobytes() == before
    assert np.array_equal(kf.image(0), image_of(w, h).astype(np.float32))


def test_pipelined_context_gives_the_same_image():
    """on a pipelined context the plot runs on the mapping stream, behind an update queued there"""
    import lsd_slam_amd as la
    w, h = 160, 128
    frames, depth0, K, gt = sequence(w, h, 3)
    images = {}
    for pipelined in (False, True):
        ctx = la.Context(w, h, K)
        if pipelined:
            ctx.set_pipeline(True)
        ctx.set_async(True)                  # mapping calls return once queued
        kf = la.Frame(ctx, 0, frames[0])
        kf.setDepthFromGroundTruth(depth0)
        dm = la.DepthMap(ctx)
        dm.initializeFromGTDepth(kf)
        ref = la.TrackingReference()
        ref.importFrame(kf)
        kf.clearDepthHasBeenUpdatedFlag()
        tracker = la.SE3Tracker(ctx)
        tracker.set_maxItsPerLvl([5, 20, 50, 100, 0])
        f = la.Frame(ctx, 5, frames[2])
        tracker.trackFrame(ref, f, la.IDENTITY)
        dm.updateKeyframe([f])
        images[pipelined] = [dm.debugPlotDepthMap(mode) for mode in (0, 5)]
        want = [dp.plot_ref(dm.currentDepthMap(), np.ascontiguousarray(frames[0]).astype(np.float32), mode, 5) for mode in (0, 5)]
        for got, w_ in zip(images[pipelined], want):
            assert_same_image(got, w_, "pipelined %s" % pipelined)
        del tracker, dm, f, kf
        if pipelined:
            ctx.set_pipeline(False)
        ctx.close()
    for a, b in zip(images[False], images[True]):
        assert_same_image(a, b, "one-stream vs pipelined")


def test_error_codes():
    import lsd_slam_amd as la
    w, h = 160, 128
    ctx = ctx_of(w, h)
    L = ctx.L
    bare = la.DepthMap(ctx)
    out = np.zeros((h, w, 3), np.uint8)
    assert L.lsdhip_depth_debug_plot(bare.h_, 0, out.ctypes.data) == E_STATE
    dm, kf, hyp = planted(ctx)
    assert L.lsdhip_depth_debug_plot(dm.h_, 0, None) == E_ARG
    assert L.lsdhip_depth_debug_plot(None, 0, out.ctypes.data) == E_ARG
    assert L.lsdhip_depth_debug_plot_dev(dm.h_, 0, None) == E_ARG
    bufs = DeviceImages(ctx, 2)
    try:
        ma = (ctypes.c_void_p * 2)(dm.h_, bare.h_)
        oa = (ctypes.c_void_p * 2)(*bufs.ptrs)
        assert L.lsdhip_depth_debug_plot_batch(2, ma, 0, oa) == E_STATE
        assert L.lsdhip_depth_debug_plot_batch(2, ma, 0, None) == E_ARG
        assert L.lsdhip_depth_debug_plot_batch(0, ma, 0, oa) == E_ARG
        other = la.Context(w, h, K_OF(w, h) * np.float32(1.01))
        dm2, kf2, _ = planted(other)
        mb = (ctypes.c_void_p * 2)(dm.h_, dm2.h_)
        assert L.lsdhip_depth_debug_plot_batch(2, mb, 0, oa) == E_ARG          # maps of two contexts
    finally:
        bufs.free()


def test_dataset_slam_writes_depth_images(tmp_path):
    w, h, n = 160, 128, 8
    frames, depth0, K, gt = sequence(w, h, n)
    lst = []
    for i in range(n):
        p = tmp_path / ("f%04d.pgm" % i)
        p.write_bytes(b"P5\n%d %d\n255\n" % (w, h) + frames[i].tobytes())
        lst.append(str(p))
    (tmp_path / "files.txt").write_text("\n".join(lst) + "\n")
    (tmp_path / "calib.cfg").write_text("%f %f %f %f 0\n%d %d\nnone\n%d %d\n" % (K[0], K[1], K[2], K[3], w, h, w, h))
    out = tmp_path / "depth"
    out.mkdir()
    exe = os.path.join(ROOT, "lsd_slam_amd", "dataset_slam")
    subprocess.check_call([exe, str(tmp_path / "calib.cfg"), str(tmp_path / "files.txt"), str(tmp_path), "--depth-images", str(out)], timeout=120)
    assert sorted(os.listdir(out)) == ["depth_%d.ppm" % i for i in range(1, n)]       # one per mapped frame
    head = b"P6\n%d %d\n255\n" % (w, h)
    kf_bytes = np.ascontiguousarray(frames[0])
    for i in range(1, n):
        raw = (out / ("depth_%d.ppm" % i)).read_bytes()
        assert raw.startswith(head) and len(raw) == len(head) + 3 * w * h
        img = np.frombuffer(raw[len(head):], np.uint8).reshape(h, w, 3)
        is_grey = (img[..., 0] == img[..., 1]) & (img[..., 1] == img[..., 2])
        assert (~is_grey).any()                                               # hypotheses in colour
        # frame 0 is the keyframe throughout (default keyframe selection, 7 frames): every grey pixel is its byte
        assert (img[..., 0][is_grey] == kf_bytes[is_grey]).all()
