"""Host-side mirror of the reference's class interface for the hot path, on top of the C ABI (include/lsdhip.h).

Same names, argument meaning and error behaviour as the reference so that parity tests read like the reference's
call sites (`C/` = lsd_slam_core/src/):

    Frame(id, image, ctx)                          C/DataStructures/Frame.h:43
    TrackingReference.importFrame(kf)              C/Tracking/TrackingReference.h:49
    SE3Tracker.trackFrame(reference, frame, init)  C/Tracking/SE3Tracker.h:65-68
    DepthMap.updateKeyframe / createKeyFrame / finalizeKeyFrame / initializeFromGTDepth …
                                                   C/DepthEstimation/DepthMap.h:47-98

Poses are numpy double[7] = (qw,qx,qy,qz,tx,ty,tz).  All per-pixel work happens in liblsdhip.so on the GPU; this
file only marshals arguments (no numerical fallback of any kind).
"""
import ctypes as C

import numpy as np

from . import capi
from .capi import HYP_DTYPE, check

IDENTITY = np.array([1.0, 0, 0, 0, 0, 0, 0])
KEYFRAME_POINT_DTYPE = np.dtype([("idepth", "<f4"), ("idepth_var", "<f4"), ("color", "u1", 4)])   # InputPointDense, 12 bytes
assert KEYFRAME_POINT_DTYPE.itemsize == 12


class Context:
    """(w, h, K) + device + stream shared by Frame / SE3Tracker / DepthMap objects."""

    def __init__(self, w, h, K, device=0, params=None):
        self.L = capi.lib()
        self.w, self.h = int(w), int(h)
        self.K = np.ascontiguousarray(K, dtype=np.float32)
        self.params = capi.Params()
        self.L.lsdhip_default_params(C.byref(self.params))
        if params:
            for k, v in params.items():
                setattr(self.params, k, v)
        h_ = C.c_void_p()
        check(self.L.lsdhip_ctx_create(device, self.w, self.h, self.K.ctypes.data, C.byref(self.params), C.byref(h_)),
              allow_positive=False)
        self.h_ = h_

    @classmethod
    def view(cls, handle, w, h):
        """a context owned by somebody else (the C++ driver loops), for Frame.view / PointCloud.view: never destroyed from here"""
        c = cls.__new__(cls)
        c.L, c.w, c.h, c.h_, c._borrowed = capi.lib(), int(w), int(h), C.c_void_p(handle if isinstance(handle, int) else handle.value), True
        return c

    def close(self):
        if getattr(self, "h_", None) and not getattr(self, "_borrowed", False):
            self.L.lsdhip_ctx_destroy(self.h_)
        self.h_ = None

    def synchronize(self):
        check(self.L.lsdhip_ctx_synchronize(self.h_))

    def set_async(self, on=True):
        """DepthMap calls return once queued (lsdhip_ctx_set_async)"""
        check(self.L.lsdhip_ctx_set_async(self.h_, int(bool(on))))

    def set_pipeline(self, on=True):
        """tracking stream beside mapping stream (lsdhip_ctx_set_pipeline): the reference's two threads with blockUntilMapped == false"""
        check(self.L.lsdhip_ctx_set_pipeline(self.h_, int(bool(on))))

    def lanes_begin(self, n):
        """open a lane region: independent call chains (per-sequence keyframe changes) go to n side streams (lsdhip_ctx_lanes_begin)"""
        check(self.L.lsdhip_ctx_lanes_begin(self.h_, int(n)))

    def lane_select(self, lane):
        check(self.L.lsdhip_ctx_lane_select(self.h_, int(lane)))

    def lanes_end(self):
        check(self.L.lsdhip_ctx_lanes_end(self.h_))

    def reserve_frames(self, n):
        """frame-memory pool: n arenas allocated ahead (lsdhip_ctx_reserve_frames)"""
        check(self.L.lsdhip_ctx_reserve_frames(self.h_, int(n)), False)

    def intrinsics(self, level):
        out = np.zeros(8, np.float32)
        check(self.L.lsdhip_ctx_intrinsics(self.h_, level, out.ctypes.data))
        return out

    def batchForm(self, which="update"):
        """the form the last DepthMap.updateKeyframeBatch ("update") / changeKeyframeBatch ("change") on this context took
        (lsdhip_ctx_batch_form): dict with n, split, candidates, py, nSet, walkWorkgroups, queued, chunks and queueCounts (entries queued
        per map; None where the counts are not available: not split, asynchronous context, or asked too late)"""
        out = np.zeros(8, np.int32)
        counts = np.zeros(512, np.int32)
        check(self.L.lsdhip_ctx_batch_form(self.h_, {"update": 0, "change": 1}[which], out.ctypes.data, counts.ctypes.data, len(counts)))
        n = int(out[0])
        return {"n": n, "split": bool(out[1]), "candidates": bool(out[2]), "py": int(out[3]), "nSet": int(out[4]),
                "walkWorkgroups": int(out[5]), "queued": int(out[6]), "chunks": int(out[7]),
                "queueCounts": counts[:n].copy() if out[6] >= 0 else None}

    def stream(self):
        return self.L.lsdhip_ctx_stream(self.h_)

    def prof_enable(self, on=True):
        check(self.L.lsdhip_prof_enable(self.h_, int(on)))

    def prof_reset(self):
        check(self.L.lsdhip_prof_reset(self.h_))

    def prof_read(self):
        ms, n, b = C.c_double(), C.c_longlong(), C.c_double()
        check(self.L.lsdhip_prof_read(self.h_, C.byref(ms), C.byref(n), C.byref(b)))
        return ms.value, n.value, b.value


class Frame:
    """Device-resident frame: pyramids are built on the GPU at construction."""
    idxInKeyframes = -1     # Frame::idxInKeyframes (C/DataStructures/Frame.h:203): the frame's slot once KeyFrameBank.put has taken it

    def __init__(self, ctx, id_, image=None, device_ptr=None):
        self.ctx = ctx
        self.L = ctx.L
        h_ = C.c_void_p()
        if device_ptr is not None:
            check(self.L.lsdhip_frame_create_from_device(ctx.h_, id_, C.c_void_p(device_ptr), C.byref(h_)), False)
        else:
            img = np.ascontiguousarray(image, dtype=np.uint8)
            if img.shape != (ctx.h, ctx.w):
                raise ValueError("image must be %dx%d uint8" % (ctx.w, ctx.h))
            check(self.L.lsdhip_frame_create(ctx.h_, id_, img.ctypes.data, C.byref(h_)), False)
        self.h_ = h_
        self._id = id_
        self._parent = None

    @classmethod
    def createBatch(cls, ctx, ids, images=None, device_ptrs=None):
        """the new frames of several sequences in two launches (lsdhip_frame_create_batch) -> list of Frame"""
        n = len(ids)
        ida = (C.c_int * n)(*[int(v) for v in ids])
        out = (C.c_void_p * n)()
        if device_ptrs is not None:
            ptrs = (C.c_void_p * n)(*[int(p) for p in device_ptrs])
            check(ctx.L.lsdhip_frame_create_batch(ctx.h_, n, ida, ptrs, 1, out), False)
        else:
            imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
            for im in imgs:
                if im.shape != (ctx.h, ctx.w):
                    raise ValueError("image must be %dx%d uint8" % (ctx.w, ctx.h))
            ptrs = (C.c_void_p * n)(*[im.ctypes.data for im in imgs])
            check(ctx.L.lsdhip_frame_create_batch(ctx.h_, n, ida, ptrs, 0, out), False)
        frames = []
        for j in range(n):
            f = cls.__new__(cls)
            f.ctx, f.L, f.h_, f._id, f._parent = ctx, ctx.L, C.c_void_p(out[j]), int(ids[j]), None
            frames.append(f)
        return frames

    @classmethod
    def view(cls, ctx, handle):
        """a frame owned by somebody else (a keyframe a C++ driver loop keeps): never destroyed from here"""
        f = cls.__new__(cls)
        f.ctx, f.L, f.h_, f._parent, f._borrowed = ctx, ctx.L, C.c_void_p(handle), None, True
        f._id = ctx.L.lsdhip_frame_id(f.h_)
        return f

    def __del__(self):
        self.close()

    def close(self):
        if getattr(self, "h_", None) and getattr(self.ctx, "h_", None) and not getattr(self, "_borrowed", False):
            self.L.lsdhip_frame_destroy(self.h_)
        self.h_ = None

    def id(self):
        return self._id

    def width(self, level=0):
        return self.ctx.w >> level

    def height(self, level=0):
        return self.ctx.h >> level

    def _plane(self, what, level):
        shape = (self.height(level), self.width(level), 4) if what == 1 else (self.height(level), self.width(level))
        out = np.zeros(shape, np.float32)
        check(self.L.lsdhip_frame_download(self.h_, what, level, out.ctypes.data), False)
        return out

    def image(self, level=0):
        return self._plane(0, level)

    def gradients(self, level=0):
        return self._plane(1, level)

    def maxGradients(self, level=0):
        return self._plane(2, level)

    def idepth(self, level=0):
        return self._plane(3, level)

    def idepthVar(self, level=0):
        return self._plane(4, level)

    def reActivationData(self):
        """(idepth_reAct f4, idepthVar_reAct f4, validity_reAct u1) [h, w] as Frame::takeReActivationData left them (Frame.cpp:107-145;
        lsdhip_frame_download what = 7, 8, 9); the first and the last are defined where idepthVar_reAct > 0"""
        val = np.zeros((self.height(0), self.width(0)), np.uint8)
        check(self.L.lsdhip_frame_download(self.h_, 9, 0, val.ctypes.data), False)
        return self._plane(7, 0), self._plane(8, 0), val

    def keyframePoints(self):
        """the keyframeMsg payload packed on the device (lsdhip_frame_pack_keyframe_points): structured array [h, w] of
        (idepth f4, idepth_var f4, color u1 x 4), the InputPointDense records of V/KeyFrameDisplay.h:39-44"""
        out = np.zeros((self.height(0), self.width(0)), KEYFRAME_POINT_DTYPE)
        check(self.L.lsdhip_frame_pack_keyframe_points(self.h_, out.ctypes.data), False)
        return out

    def referenceBlocks(self, level):
        """(offsets uint8 [blocks, 256], counts int32 [blocks]) of the level's reference blocks (lsdhip_frame_download what = 5): per 256
        consecutive pixels the in-block offsets of the valid reference pixels, compacted in pixel order (returned in list order: on the device
        slot s of a block sits in byte (s mod 64) * 4 + s // 64, so that a lane's 4-byte word holds slots l, l + 64, l + 128, l + 192)."""
        nblk = (self.width(level) * self.height(level) + 255) // 256
        raw = np.zeros(nblk * 260, np.uint8)
        check(self.L.lsdhip_frame_download(self.h_, 5, level, raw.ctypes.data), False)
        offs = raw[:nblk * 256].reshape(nblk, 64, 4).transpose(0, 2, 1).reshape(nblk, 256)
        return offs.copy(), raw[nblk * 256:].view(np.int32).copy()

    def gradientCandidates(self):
        """(offsets uint16 [groups, 1024], counts uint16 [groups]) of the frame's gradient candidates (lsdhip_frame_download what = 6)."""
        ng = (self.width(0) * self.height(0) + 1023) // 1024
        raw = np.zeros(ng * 1025, np.uint16)
        check(self.L.lsdhip_frame_download(self.h_, 6, 0, raw.ctypes.data), False)
        return raw[:ng * 1024].reshape(ng, 1024).copy(), raw[ng * 1024:].copy()

    def setDepthFromGroundTruth(self, depth, cov_scale=1.0):
        d = np.ascontiguousarray(depth, dtype=np.float32)
        check(self.L.lsdhip_frame_set_depth_gt(self.h_, d.ctypes.data, cov_scale), False)

    def setDepthPlanes(self, idepth, idepthVar):
        a = np.ascontiguousarray(idepth, dtype=np.float32)
        b = np.ascontiguousarray(idepthVar, dtype=np.float32)
        check(self.L.lsdhip_frame_set_depth_planes(self.h_, a.ctypes.data, b.ctypes.data), False)

    def setMaxGradients(self, plane):
        p = np.ascontiguousarray(plane, dtype=np.float32)
        check(self.L.lsdhip_frame_set_maxgrad(self.h_, p.ctypes.data), False)

    def refPixelWasGoodNoCreate(self):
        out = np.zeros((self.height(1), self.width(1)), np.uint8)
        rc = check(self.L.lsdhip_frame_get_wasgood(self.h_, out.ctypes.data))
        return out if rc == 1 else None

    def set_refPixelWasGood(self, m):
        m = np.ascontiguousarray(m, dtype=np.uint8)
        check(self.L.lsdhip_frame_set_wasgood(self.h_, m.ctypes.data), False)

    def clear_refPixelWasGood(self):
        check(self.L.lsdhip_frame_clear_wasgood(self.h_))

    def setPose(self, thisToParent_sim3, trackingParent, initialTrackedResidual=0.0):
        s = np.ascontiguousarray(thisToParent_sim3, dtype=np.float64)
        self._parent = trackingParent
        check(self.L.lsdhip_frame_set_pose(self.h_, s.ctypes.data, trackingParent.h_ if trackingParent else None,
                                           initialTrackedResidual), False)

    def thisToParent_raw(self):
        out = np.zeros(8, np.float64)
        check(self.L.lsdhip_frame_get_pose(self.h_, out.ctypes.data))
        return out

    def relativePoseTo(self, reference):
        """se3FromSim3(reference.camToWorld^-1 * self.camToWorld) (C/SlamSystem.cpp:918-920) for a frame tracked on `reference` or on
        the same parent as `reference` (lsdhip_frame_relative_pose)"""
        out = np.zeros(7, np.float64)
        check(self.L.lsdhip_frame_relative_pose(reference.h_, self.h_, out.ctypes.data))
        return out

    def depthHasBeenUpdatedFlag(self):
        return check(self.L.lsdhip_frame_depth_updated(self.h_)) != 0

    def clearDepthHasBeenUpdatedFlag(self):
        check(self.L.lsdhip_frame_clear_depth_updated(self.h_))

    def stats(self):
        out = np.zeros(8, np.float32)
        check(self.L.lsdhip_frame_stats(self.h_, out.ctypes.data))
        keys = ["initialTrackedResidual", "meanIdepth", "numPoints", "numFramesTrackedOnThis", "numMappedOnThis",
                "numMappedOnThisTotal", "depthHasBeenUpdatedFlag", "reserved"]
        return dict(zip(keys, out.tolist()))

    def clearDepthHasBeenUpdatedFlag(self):
        """currentKeyFrame->depthHasBeenUpdatedFlag = false (C/SlamSystem.cpp:910, when the tracking reference is re-imported)"""
        s = self.stats()
        self.setCounters(int(s["numFramesTrackedOnThis"]), int(s["numMappedOnThis"]), int(s["numMappedOnThisTotal"]), False)

    def setCounters(self, numFramesTrackedOnThis, numMappedOnThis, numMappedOnThisTotal, depthHasBeenUpdatedFlag):
        check(self.L.lsdhip_frame_set_counters(self.h_, numFramesTrackedOnThis, numMappedOnThis, numMappedOnThisTotal,
                                               int(depthHasBeenUpdatedFlag)))


class Undistorter:
    """A camera's rectification on the device (lsdhip_undistorter_*; UndistorterPTAM, C/util/Undistorter.cpp:282-411): the remap tables
    of the context's w x h output image — built on the host by lsd_slam_hip::Undistorter of include/lsd_slam_hip_io.hpp — resident on the
    GPU.  Raw images are uint8 [in_h, in_w] arrays, or device pointers to as many bytes."""

    def __init__(self, ctx, in_w, in_h, remapX, remapY):
        self.ctx, self.L = ctx, ctx.L
        self.in_w, self.in_h = int(in_w), int(in_h)
        rx = np.ascontiguousarray(remapX, dtype=np.float32)
        ry = np.ascontiguousarray(remapY, dtype=np.float32)
        if rx.size != ctx.w * ctx.h or ry.size != ctx.w * ctx.h:
            raise ValueError("remap tables must hold %dx%d entries" % (ctx.w, ctx.h))
        h_ = C.c_void_p()
        check(self.L.lsdhip_undistorter_create(ctx.h_, self.in_w, self.in_h, rx.ctypes.data, ry.ctypes.data, C.byref(h_)), False)
        self.h_ = h_

    def __del__(self):
        self.close()

    def close(self):
        if getattr(self, "h_", None) and getattr(self.ctx, "h_", None):
            self.L.lsdhip_undistorter_destroy(self.h_)
        self.h_ = None

    def _raw(self, raw):
        img = np.ascontiguousarray(raw, dtype=np.uint8)
        if img.shape != (self.in_h, self.in_w):
            raise ValueError("raw image must be %dx%d uint8" % (self.in_w, self.in_h))
        return img

    def apply(self, raw=None, device_ptr=None, out_device_ptr=None):
        """the rectified uint8 image (lsdhip_undistorter_apply) -> [h, w] array, or None when written to out_device_ptr"""
        img = None if device_ptr is not None else self._raw(raw)
        out = None if out_device_ptr is not None else np.empty((self.ctx.h, self.ctx.w), np.uint8)
        src = C.c_void_p(device_ptr) if img is None else img.ctypes.data
        dst = C.c_void_p(out_device_ptr) if out is None else out.ctypes.data
        check(self.L.lsdhip_undistorter_apply(self.h_, src, int(img is None), dst, int(out is None)), False)
        return out

    def _adopt(self, handle, id_):
        f = Frame.__new__(Frame)
        f.ctx, f.L, f.h_, f._id, f._parent = self.ctx, self.L, C.c_void_p(handle), int(id_), None
        return f

    def frame(self, id_, raw=None, device_ptr=None, wait=True):
        """a Frame of a raw image (lsdhip_frame_create_undistorted / _async / _from_device).  wait=False: the raw host array must stay
        alive and unchanged until the frame has been tracked or the context synchronised; it is kept on the frame."""
        h_ = C.c_void_p()
        if device_ptr is not None:
            check(self.L.lsdhip_frame_create_undistorted_from_device(self.h_, id_, C.c_void_p(device_ptr), C.byref(h_)), False)
            return self._adopt(h_.value, id_)
        img = self._raw(raw)
        fn = self.L.lsdhip_frame_create_undistorted if wait else self.L.lsdhip_frame_create_undistorted_async
        check(fn(self.h_, id_, img.ctypes.data, C.byref(h_)), False)
        f = self._adopt(h_.value, id_)
        if not wait:
            f._raw_keepalive = img
        return f

    def createBatch(self, ids, raws=None, device_ptrs=None):
        """the new frames of several sequences from raw images in two launches (lsdhip_frame_create_undistorted_batch) -> list of Frame"""
        n = len(ids)
        ida = (C.c_int * n)(*[int(v) for v in ids])
        out = (C.c_void_p * n)()
        if device_ptrs is not None:
            ptrs = (C.c_void_p * n)(*[int(p) for p in device_ptrs])
            check(self.L.lsdhip_frame_create_undistorted_batch(self.h_, n, ida, ptrs, 1, out), False)
        else:
            imgs = [self._raw(im) for im in raws]
            ptrs = (C.c_void_p * n)(*[im.ctypes.data for im in imgs])
            check(self.L.lsdhip_frame_create_undistorted_batch(self.h_, n, ida, ptrs, 0, out), False)
        return [self._adopt(out[j], ids[j]) for j in range(n)]


class PointCloud:
    """The viewer's accumulated point cloud in device memory (lsdhip_cloud_*; KeyFrameDisplay::flushPC per keyframe,
    V/KeyFrameDisplay.cpp:269-340).  appendKeyframe only queues work on the context's mapping stream; total / stored / segments /
    download wait for it.  camToWorld: the 7 floats of the keyframeMsg (quaternion x y z w with norm = scale, translation)."""
    GUARD_POINTS = 64     # LSDHIP_CLOUD_GUARD_POINTS
    TABLE_FULL = 2        # LSDHIP_CLOUD_TABLE_FULL

    def __init__(self, ctx, capacity_points, max_keyframes):
        self.ctx = ctx
        self.L = ctx.L
        self.capacity = int(capacity_points)
        h_ = C.c_void_p()
        check(self.L.lsdhip_cloud_create(ctx.h_, self.capacity, int(max_keyframes), C.byref(h_)), False)
        self.h_ = h_

    def __del__(self):
        self.close()

    @classmethod
    def view(cls, ctx, handle, capacity_points):
        """a cloud owned by somebody else (the sinks of a C++ driver loop): never destroyed from here"""
        q = cls.__new__(cls)
        q.ctx, q.L, q.capacity, q.h_, q._borrowed = ctx, ctx.L, int(capacity_points), C.c_void_p(handle), True
        return q

    def close(self):
        if getattr(self, "h_", None) and getattr(self.ctx, "h_", None) and not getattr(self, "_borrowed", False):
            self.L.lsdhip_cloud_destroy(self.h_)
        self.h_ = None

    def appendKeyframe(self, frame, camToWorld, scaledTH=1.0, absTH=1.0, minNearSupport=5):
        """returns False once the segment table is full"""
        p = np.ascontiguousarray(camToWorld, dtype=np.float32)
        assert p.shape == (7,)
        return check(self.L.lsdhip_cloud_append_keyframe(self.h_, frame.h_, p.ctypes.data, scaledTH, absTH, int(minNearSupport))) != self.TABLE_FULL

    @staticmethod
    def appendBatch(clouds, frames, camToWorlds, scaledTH=1.0, absTH=1.0, minNearSupport=5):
        n = len(clouds)
        p = np.ascontiguousarray(camToWorlds, dtype=np.float32).reshape(n, 7)
        cs = (C.c_void_p * n)(*[c.h_.value for c in clouds])
        fs = (C.c_void_p * n)(*[f.h_.value for f in frames])
        ctx = clouds[0].ctx
        return check(ctx.L.lsdhip_cloud_append_batch(ctx.h_, n, cs, fs, p.ctypes.data, scaledTH, absTH, int(minNearSupport)))

    def _count(self):
        t, s = C.c_int64(), C.c_int64()
        check(self.L.lsdhip_cloud_count(self.h_, C.byref(t), C.byref(s)), False)
        return t.value, s.value

    def total(self):
        return self._count()[0]

    def stored(self):
        return self._count()[1]

    def segments(self, max_rows=4096):
        """list of (frame id, first, count) per appended keyframe"""
        ids, cnt, first, n = np.zeros(max_rows, np.int32), np.zeros(max_rows, np.int32), np.zeros(max_rows, np.int64), C.c_int()
        check(self.L.lsdhip_cloud_segments(self.h_, max_rows, ids.ctypes.data, first.ctypes.data, cnt.ctypes.data, C.byref(n)), False)
        k = min(n.value, max_rows)
        return [(int(ids[i]), int(first[i]), int(cnt[i])) for i in range(k)]

    def download(self, first=0, n=None):
        """points [first, first + n) as float32 [n, 4] (x, y, z, intensity); n = None: the stored points from `first`.  Reading up to
        capacity + GUARD_POINTS is allowed (the guard behind the buffer keeps its 0xFF fill)."""
        if n is None:
            n = max(self.stored() - first, 0)
        out = np.zeros((int(n), 4), np.float32)
        check(self.L.lsdhip_cloud_download(self.h_, int(first), int(n), out.ctypes.data), False)
        return out

    def reset(self):
        check(self.L.lsdhip_cloud_reset(self.h_), False)


class TrackingReference:
    """C/Tracking/TrackingReference.h — on the device the point cloud is generated on the fly inside the residual
    kernel, so this object only remembers which keyframe it refers to; makePointCloud() exports the compacted arrays
    in the reference's order for callers that want them (permaref, Sim3 tracker)."""

    def __init__(self):
        self.keyframe = None

    def importFrame(self, kf):
        """TrackingReference.cpp:71-87; on a pipelined context the hand-over of the mapping side's newest Frame::setDepth result to
        the tracker (lsdhip_frame_publish_depth)"""
        self.keyframe = kf
        if kf is not None:
            check(kf.L.lsdhip_frame_publish_depth(kf.h_))

    def invalidate(self):
        self.keyframe = None

    def makePointCloud(self, level):
        kf = self.keyframe
        n_max = kf.width(level) * kf.height(level)
        pos = np.zeros((n_max, 3), np.float32)
        cv = np.zeros((n_max, 2), np.float32)
        gr = np.zeros((n_max, 2), np.float32)
        idx = np.zeros(n_max, np.int32)
        n = check(kf.L.lsdhip_ref_pointcloud(kf.h_, level, pos.ctypes.data, cv.ctypes.data, gr.ctypes.data, idx.ctypes.data))
        return pos[:n].copy(), cv[:n].copy(), gr[:n].copy(), idx[:n].copy()


class SE3Tracker:
    def __init__(self, ctx):
        self.ctx = ctx
        self.L = ctx.L
        h_ = C.c_void_p()
        check(self.L.lsdhip_tracker_create(ctx.h_, C.byref(h_)), False)
        self.h_ = h_
        self.last = None

    def __del__(self):
        self.close()

    def close(self):
        if getattr(self, "h_", None) and getattr(self.ctx, "h_", None):
            self.L.lsdhip_tracker_destroy(self.h_)
        self.h_ = None

    def set_maxItsPerLvl(self, its):
        its = np.ascontiguousarray(its, dtype=np.int32)
        check(self.L.lsdhip_tracker_set_max_its(self.h_, its.ctypes.data))

    def settings(self):
        """DenseDepthTrackerSettings of this tracker (a copy; write back with set_settings)"""
        st = capi.TrackerSettings()
        check(self.L.lsdhip_tracker_get_settings(self.h_, C.byref(st)))
        return st

    def set_settings(self, st):
        check(self.L.lsdhip_tracker_set_settings(self.h_, C.byref(st)))


    def set_speculation(self, trials, finest_level_workgroups=0):
        """LM retries evaluated per launch (1 = one evaluation per launch); see include/lsdhip.h"""
        check(self.L.lsdhip_tracker_set_speculation(self.h_, int(trials), int(finest_level_workgroups)))

    def set_batch_coarse_min_jobs(self, min_jobs):
        """throughput-mode batches of at least `min_jobs` jobs walk their coarse levels in one workgroup per job (0: never); see include/lsdhip.h"""
        check(self.L.lsdhip_tracker_set_batch_coarse_min_jobs(self.h_, int(min_jobs)))

    def launch_stats(self):
        """(evaluating launches of the last job, trials per launch)"""
        out = np.zeros(2, np.int32)
        check(self.L.lsdhip_tracker_launch_stats(self.h_, out.ctypes.data))
        return int(out[0]), int(out[1])

    def summary_stats(self):
        """(jobs polled, records incomplete when `done` arrived, longest wait ns, stale words, lowest / highest stale word index)"""
        out = np.zeros(6, np.int64)
        check(self.L.lsdhip_tracker_summary_stats(self.h_, out.ctypes.data))
        return [int(v) for v in out]

    def step_stats(self):
        """(k_track_step launches of the last job, steps inside the cluster kernel, cluster-kernel launches, most trials per step)"""
        out = np.zeros(4, np.int32)
        check(self.L.lsdhip_tracker_step_stats(self.h_, out.ctypes.data))
        return tuple(int(v) for v in out)

    def exec_stats(self):
        """diagnostics: (cluster-kernel jobs, give-ups rerun on the chain, switched off, evaluations per level 0..4)"""
        out = np.zeros(8, np.int32)
        check(self.L.lsdhip_tracker_exec_stats(self.h_, out.ctypes.data))
        return int(out[0]), int(out[1]), bool(out[2]), out[3:8].tolist()

    def _publish(self, r):
        self.last = r
        self.pointUsage = r.pointUsage
        self.lastGoodCount = r.lastGoodCount
        self.lastBadCount = r.lastBadCount
        self.lastMeanRes = r.lastMeanRes
        self.lastResidual = r.lastResidual
        self.affineEstimation_a = r.affineEstimation_a
        self.affineEstimation_b = r.affineEstimation_b
        self.diverged = bool(r.diverged)
        self.trackingWasGood = bool(r.trackingWasGood)

    def trackFrame(self, reference, frame, frameToReference_initialEstimate):
        """Returns frameToReference (double[7]); identity when diverged, like the reference (SE3Tracker.cpp:324-329)."""
        init = np.ascontiguousarray(frameToReference_initialEstimate, dtype=np.float64)
        r = capi.TrackResult()
        check(self.L.lsdhip_tracker_track(self.h_, reference.keyframe.h_, frame.h_, init.ctypes.data, C.byref(r)))
        self._publish(r)
        if not r.diverged:
            frame._parent = reference.keyframe
        return np.array(r.frameToReference)

    def trackFrameBatch(self, references, frames, inits):
        """trackFrame for independent (reference, frame) pairs in the same kernel launches; returns (poses n x 7,
        list of result records)."""
        n = len(frames)
        kfs = (C.c_void_p * n)(*[r.keyframe.h_ for r in references])
        frs = (C.c_void_p * n)(*[f.h_ for f in frames])
        init = np.ascontiguousarray(inits, dtype=np.float64).reshape(n, 7)
        res = (capi.TrackResult * n)()
        check(self.L.lsdhip_tracker_track_batch(self.h_, n, kfs, frs, init.ctypes.data, res))
        for f, r, ref in zip(frames, res, references):
            if not r.diverged:
                f._parent = ref.keyframe
        return np.array([list(r.frameToReference) for r in res]), list(res)

    def evalThroughput(self, references, frames, referenceToFrames, level, repeats=20):
        """measurement hook: the throughput-mode evaluation launch at `level` for n >= 8 jobs; returns (ms per launch, algorithmic
        bytes per launch)"""
        n = len(frames)
        kfs = (C.c_void_p * n)(*[r.keyframe.h_ for r in references])
        frs = (C.c_void_p * n)(*[f.h_ for f in frames])
        T = np.ascontiguousarray(referenceToFrames, dtype=np.float32).reshape(n, 7)
        ms, nb = C.c_double(), C.c_double()
        check(self.L.lsdhip_tracker_eval_throughput(self.h_, n, kfs, frs, T.ctypes.data, int(level), int(repeats), C.byref(ms), C.byref(nb)))
        return ms.value, nb.value

    def evaluate(self, reference, frame, referenceToFrame, level, a=1.0, b=0.0):
        T = np.ascontiguousarray(referenceToFrame, dtype=np.float32)
        r = capi.ResidualRecord()
        check(self.L.lsdhip_tracker_evaluate(self.h_, reference.keyframe.h_, frame.h_, T.ctypes.data, level, a, b, C.byref(r)), False)
        return r

    def evaluateBatch(self, references, frames, referenceToFrames, level, affine=None):
        """test hook: `evaluate` for n jobs through the launches of a batch (lsdhip_tracker_evaluate_batch); affine: n x 2 (a, b),
        default (1, 0).  Returns (list of n records, form n x 2: [ran in k_track_solo, strip size in pixels or 0])."""
        n = len(frames)
        kfs = (C.c_void_p * n)(*[r.keyframe.h_ for r in references])
        frs = (C.c_void_p * n)(*[f.h_ for f in frames])
        T = np.ascontiguousarray(referenceToFrames, dtype=np.float32).reshape(n, 7)
        ab = np.ascontiguousarray(np.tile([1.0, 0.0], (n, 1)) if affine is None else affine, dtype=np.float32).reshape(n, 2)
        res = (capi.ResidualRecord * n)()
        form = np.zeros((n, 2), np.int32)
        check(self.L.lsdhip_tracker_evaluate_batch(self.h_, n, kfs, frs, T.ctypes.data, ab.ctypes.data, int(level), res, form.ctypes.data), False)
        return list(res), form

    def evaluatePoints(self, permaRef_pos, permaRef_colVar, frame, referenceToFrame, a=1.0, b=0.0):
        """test hook: `evaluate` on an explicit level-4 point list, the single job's evaluation (lsdhip_tracker_evaluate_points).
        Returns (record, [workgroups, single pass])."""
        pos = np.ascontiguousarray(permaRef_pos, np.float32)
        cv = np.ascontiguousarray(permaRef_colVar, np.float32)
        T = np.ascontiguousarray(referenceToFrame, dtype=np.float32)
        r = capi.ResidualRecord()
        tiles = np.zeros(2, np.int32)
        check(self.L.lsdhip_tracker_evaluate_points(self.h_, pos.ctypes.data, cv.ctypes.data, len(pos), frame.h_, T.ctypes.data, a, b, C.byref(r),
                                                    tiles.ctypes.data), False)
        return r, tiles

    @staticmethod
    def _poses_and_affine(n, referenceToFrames, affine):
        T = np.ascontiguousarray(referenceToFrames, dtype=np.float32).reshape(n, 7)
        ab = np.ascontiguousarray(np.tile([1.0, 0.0], (n, 1)) if affine is None else affine, dtype=np.float32).reshape(n, 2)
        return T, ab

    def evaluatePointsBatch(self, clouds, frames, referenceToFrames, affine=None):
        """test hook: evaluatePoints for n lists in the launches of trackFrameOnPermarefBatch (lsdhip_tracker_evaluate_points_batch);
        clouds: list of (pos n_j x 3, colVar n_j x 2); affine: n x 2.  Returns (list of n records, tiles n x 2)."""
        n = len(clouds)
        pos = np.ascontiguousarray(np.concatenate([c[0] for c in clouds]), np.float32)
        cv = np.ascontiguousarray(np.concatenate([c[1] for c in clouds]), np.float32)
        counts = np.array([len(c[0]) for c in clouds], np.int32)
        frs = (C.c_void_p * n)(*[f.h_ for f in frames])
        T, ab = self._poses_and_affine(n, referenceToFrames, affine)
        res = (capi.ResidualRecord * n)()
        tiles = np.zeros((n, 2), np.int32)
        check(self.L.lsdhip_tracker_evaluate_points_batch(self.h_, n, pos.ctypes.data, cv.ctypes.data, counts.ctypes.data, frs, T.ctypes.data,
                                                          ab.ctypes.data, res, tiles.ctypes.data), False)
        return list(res), tiles

    def evaluatePointsBank(self, bank, slots, frames, referenceToFrames, affine=None):
        """test hook: evaluatePointsBatch with the lists read where they lie in the bank (lsdhip_tracker_evaluate_points_bank)"""
        n = len(slots)
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        frs = (C.c_void_p * n)(*[f.h_ for f in frames])
        T, ab = self._poses_and_affine(n, referenceToFrames, affine)
        res = (capi.ResidualRecord * n)()
        tiles = np.zeros((n, 2), np.int32)
        check(self.L.lsdhip_tracker_evaluate_points_bank(self.h_, bank.h_, n, sl.ctypes.data, frs, T.ctypes.data, ab.ctypes.data, res,
                                                         tiles.ctypes.data), False)
        return list(res), tiles

    def trackFrameOnPermaref(self, permaRef_pos, permaRef_colVar, frame, referenceToFrame):
        pos = np.ascontiguousarray(permaRef_pos, np.float32)
        cv = np.ascontiguousarray(permaRef_colVar, np.float32)
        T = np.ascontiguousarray(referenceToFrame, np.float64)
        r = capi.TrackResult()
        check(self.L.lsdhip_tracker_track_permaref(self.h_, pos.ctypes.data, cv.ctypes.data, len(pos), frame.h_, T.ctypes.data, C.byref(r)))
        self._publish(r)
        return np.array(r.frameToReference)

    def trackFrameOnPermarefBatch(self, clouds, frames, referenceToFrames):
        """clouds: list of (pos n_j x 3, colVar n_j x 2); each tracked against frames[j]; returns (poses, records)"""
        n = len(clouds)
        pos = np.ascontiguousarray(np.concatenate([c[0] for c in clouds]), np.float32)
        cv = np.ascontiguousarray(np.concatenate([c[1] for c in clouds]), np.float32)
        counts = np.array([len(c[0]) for c in clouds], np.int32)
        frs = (C.c_void_p * n)(*[f.h_ for f in frames])
        T = np.ascontiguousarray(referenceToFrames, np.float64).reshape(n, 7)
        res = (capi.TrackResult * n)()
        check(self.L.lsdhip_tracker_track_permaref_batch(self.h_, n, pos.ctypes.data, cv.ctypes.data, counts.ctypes.data, frs, T.ctypes.data, res))
        return np.array([list(r.frameToReference) for r in res]), list(res)

    def checkPermaRefOverlap(self, permaRef_pos, referenceToFrame):
        pos = np.ascontiguousarray(permaRef_pos, np.float32)
        T = np.ascontiguousarray(referenceToFrame, np.float64)
        u = C.c_float()
        check(self.L.lsdhip_tracker_check_overlap(self.h_, pos.ctypes.data, len(pos), T.ctypes.data, C.byref(u)), False)
        self.pointUsage = u.value
        return u.value

    def checkPermaRefOverlapBank(self, bank, slots, referenceToFrames):
        """checkPermaRefOverlap for (slot, pose) pairs of a KeyFrameBank in one launch -> usages float32 [n]"""
        n = len(slots)
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        T = np.ascontiguousarray(referenceToFrames, np.float64).reshape(n, 7)
        u = np.zeros(n, np.float32)
        check(self.L.lsdhip_tracker_check_overlap_bank(self.h_, bank.h_, n, sl.ctypes.data, T.ctypes.data, u.ctypes.data), False)
        return u

    def trackFrameOnPermarefBank(self, bank, slots, frames, referenceToFrames):
        """trackFrameOnPermarefBatch with the clouds read where they lie in the bank; returns (poses, records)"""
        n = len(slots)
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        frs = (C.c_void_p * n)(*[f.h_ for f in frames])
        T = np.ascontiguousarray(referenceToFrames, np.float64).reshape(n, 7)
        res = (capi.TrackResult * n)()
        check(self.L.lsdhip_tracker_track_permaref_bank(self.h_, bank.h_, n, sl.ctypes.data, frs, T.ctypes.data, res))
        return np.array([list(r.frameToReference) for r in res]), list(res)


class KeyFrameBank:
    """The permanent references of all keyframes on the device (lsdhip_kfbank_*): Frame::setPermaRef (C/DataStructures/Frame.cpp:149-174)
    per keyframe plus the metadata TrackableKeyFrameSearch reads (frame id, meanIdepth, world pose as Sim3 (qw,qx,qy,qz,tx,ty,tz,scale))."""

    def __init__(self, ctx, max_keyframes):
        self.ctx = ctx
        self.L = ctx.L
        h_ = C.c_void_p()
        check(self.L.lsdhip_kfbank_create(ctx.h_, int(max_keyframes), C.byref(h_)), False)
        self.h_ = h_

    def __del__(self):
        self.close()

    def close(self):
        if getattr(self, "h_", None) and getattr(self.ctx, "h_", None):
            self.L.lsdhip_kfbank_destroy(self.h_)
        self.h_ = None

    def put(self, frame, camToWorld=None, meanIdepth=-1.0):
        """Frame::setPermaRef on the device; returns the slot (= frame.idxInKeyframes).  camToWorld / meanIdepth: setMeta right away."""
        slot = C.c_int(-1)
        check(self.L.lsdhip_kfbank_put(self.h_, frame.h_, C.byref(slot)), False)
        frame.idxInKeyframes = slot.value
        if camToWorld is not None:
            self.setMeta(slot.value, camToWorld, meanIdepth)
        return slot.value

    def setMeta(self, slot, camToWorld, meanIdepth=-1.0):
        p = np.ascontiguousarray(camToWorld, dtype=np.float64)
        assert p.shape == (8,)
        check(self.L.lsdhip_kfbank_set_meta(self.h_, int(slot), p.ctypes.data, float(meanIdepth)), False)

    def size(self):
        return check(self.L.lsdhip_kfbank_size(self.h_))

    def info(self, slot):
        fid, n, mi, pose = C.c_int(), C.c_int(), C.c_float(), np.zeros(8, np.float64)
        check(self.L.lsdhip_kfbank_info(self.h_, int(slot), C.byref(fid), C.byref(n), C.byref(mi), pose.ctypes.data), False)
        return {"frameId": fid.value, "numPoints": n.value, "meanIdepth": mi.value, "camToWorld": pose}

    def download(self, slot):
        """(pos n x 3, colorAndVar n x 2) of the slot's cloud"""
        cap = max((self.ctx.w >> 4) - 2, 1) * max((self.ctx.h >> 4) - 2, 1)
        pos, cv = np.zeros((cap, 3), np.float32), np.zeros((cap, 2), np.float32)
        n = check(self.L.lsdhip_kfbank_download(self.h_, int(slot), pos.ctypes.data, cv.ctypes.data))
        return pos[:n].copy(), cv[:n].copy()


class TrackableKeyFrameSearch:
    """TrackableKeyFrameSearch::findRePositionCandidate (C/GlobalMapping/TrackableKeyFrameSearch.cpp:103-172) over a KeyFrameBank: the
    prefilter and the selection on the host, the overlap check of all candidates in one launch, the tracking of those that pass in one
    batch (lsdhip_tracker_find_reposition_candidate)."""

    def __init__(self, ctx, bank, tracker=None):
        self.ctx, self.bank = ctx, bank
        self.tracker = tracker or SE3Tracker(ctx)
        self._relocalizationTH = 0.7
        self.last = None

    @property
    def relocalizationTH(self):
        return self._relocalizationTH

    @relocalizationTH.setter
    def relocalizationTH(self, v):
        check(self.ctx.L.lsdhip_tracker_set_relocalization_th(self.tracker.h_, float(v)), False)
        self._relocalizationTH = float(v)

    def getRefFrameScore(self, distanceSquared, usage):
        """TrackableKeyFrameSearch.h:75-79, in single precision"""
        f = np.float32
        wd, wu = f(self.ctx.params.KFDistWeight), f(self.ctx.params.KFUsageWeight)
        return float(f(distanceSquared) * wd * wd + (f(1) - f(usage)) * (f(1) - f(usage)) * wu * wu)

    def findRePositionCandidate(self, frame, frameCamToWorld, trackingParentId=-1, maxScore=1.0):
        """-> slot of the keyframe to re-activate, or None.  frameCamToWorld: the frame's getScaledCamToWorld() as Sim3[8]; trackingParentId:
        frame id of its tracking parent.  self.last holds the result record, records() the per-keyframe ones."""
        p = np.ascontiguousarray(frameCamToWorld, dtype=np.float64)
        assert p.shape == (8,)
        r = capi.RepositionResult()
        check(self.ctx.L.lsdhip_tracker_find_reposition_candidate(self.tracker.h_, self.bank.h_, frame.h_, p.ctypes.data, int(trackingParentId),
                                                                  float(maxScore), C.byref(r)), False)
        self.last = r
        return r.slot if r.slot >= 0 else None

    def records(self):
        n = C.c_int()
        check(self.ctx.L.lsdhip_tracker_reposition_records(self.tracker.h_, 0, None, C.byref(n)), False)
        recs = (capi.RepositionRecord * max(n.value, 1))()
        check(self.ctx.L.lsdhip_tracker_reposition_records(self.tracker.h_, n.value, recs, C.byref(n)), False)
        return list(recs)[:n.value]


class Sim3Tracker:
    """Sim3Tracker (C/Tracking/Sim3Tracker.h:71-187).  Sim3 = (qw,qx,qy,qz,tx,ty,tz,scale)."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.L = ctx.L
        h_ = C.c_void_p()
        check(self.L.lsdhip_sim3tracker_create(ctx.h_, C.byref(h_)))
        self.h_ = h_
        self.diverged = False
        self.last = None

    def __del__(self):
        if getattr(self, "h_", None):
            self.L.lsdhip_sim3tracker_destroy(self.h_)
            self.h_ = None

    def setMaxItsPerLvl(self, its):
        a = np.ascontiguousarray(its, np.int32)
        check(self.L.lsdhip_sim3tracker_set_max_its(self.h_, a.ctypes.data))

    def trackFrameSim3(self, keyframe, frame, frameToReference_initialEstimate, startLevel, finalLevel):
        """-> (frameToReference[8], result record); self.diverged mirrors the reference's flag"""
        T = np.ascontiguousarray(frameToReference_initialEstimate, np.float64)
        r = capi.Sim3Result()
        check(self.L.lsdhip_sim3tracker_track(self.h_, keyframe.h_, frame.h_, T.ctypes.data, startLevel, finalLevel, C.byref(r)))
        self.diverged = bool(r.diverged)
        self.last = r
        return np.array(list(r.frameToReference)), r

    def trackFrameSim3Batch(self, keyframes, frames, inits, startLevel, finalLevel):
        """n independent (keyframe, frame, init) jobs in lock step -> (n x 8 poses, list of result records)"""
        n = len(frames)
        kfs = (C.c_void_p * n)(*[k.h_ for k in keyframes])
        frs = (C.c_void_p * n)(*[f.h_ for f in frames])
        T = np.ascontiguousarray(inits, np.float64).reshape(n, 8)
        res = (capi.Sim3Result * n)()
        check(self.L.lsdhip_sim3tracker_track_batch(self.h_, n, kfs, frs, T.ctypes.data, startLevel, finalLevel, res))
        return np.array([list(r.frameToReference) for r in res]), list(res)

    def evaluate(self, keyframe, frame, referenceToFrame, level, a=1.0, b=0.0):
        T = np.ascontiguousarray(referenceToFrame, np.float64)
        r = capi.Sim3EvalRecord()
        check(self.L.lsdhip_sim3tracker_evaluate(self.h_, keyframe.h_, frame.h_, T.ctypes.data, level, a, b, C.byref(r)))
        return r


class DepthMap:
    STAGES = {"observe": 0, "fillholes": 1, "regularize": 2, "regularize_occ": 3, "propagate": 4, "fill_regularize": 5}

    def __init__(self, ctx):
        self.ctx = ctx
        self.L = ctx.L
        h_ = C.c_void_p()
        check(self.L.lsdhip_depth_create(ctx.h_, C.byref(h_)), False)
        self.h_ = h_
        self._keep = []

    def __del__(self):
        self.close()

    def close(self):
        if getattr(self, "h_", None) and getattr(self.ctx, "h_", None):
            self.L.lsdhip_depth_destroy(self.h_)
        self.h_ = None

    def _arr(self, frames):
        return (C.c_void_p * len(frames))(*[f.h_ for f in frames])

    def isValid(self):
        return bool(self.L.lsdhip_depth_is_valid(self.h_))

    def invalidate(self):
        check(self.L.lsdhip_depth_invalidate(self.h_))

    def reset(self):
        check(self.L.lsdhip_depth_reset(self.h_))

    def initializeFromGTDepth(self, frame):
        self._keep.append(frame)
        check(self.L.lsdhip_depth_init_gt(self.h_, frame.h_), False)

    def initializeRandomly(self, frame):
        self._keep.append(frame)
        check(self.L.lsdhip_depth_init_random(self.h_, frame.h_), False)

    def setFromExistingKF(self, frame):
        self._keep.append(frame)
        check(self.L.lsdhip_depth_set_from_existing(self.h_, frame.h_), False)

    def updateKeyframe(self, referenceFrames):
        frames = list(referenceFrames)
        check(self.L.lsdhip_depth_update(self.h_, self._arr(frames), len(frames)), False)

    @staticmethod
    def updateKeyframeBatch(maps, frames):
        """updateKeyframe of several sequences' maps, one tracked frame each, in shared launches (lsdhip_depth_update_batch)"""
        n = len(maps)
        ma = (C.c_void_p * n)(*[m.h_ for m in maps])
        fa = (C.c_void_p * n)(*[f.h_ for f in frames])
        check(maps[0].L.lsdhip_depth_update_batch(n, ma, fa), False)

    def createKeyFrame(self, new_keyframe):
        self._keep.append(new_keyframe)
        s = C.c_float()
        check(self.L.lsdhip_depth_create_keyframe(self.h_, new_keyframe.h_, C.byref(s)), False)
        return s.value

    def finalizeKeyFrame(self):
        check(self.L.lsdhip_depth_finalize(self.h_), False)

    @staticmethod
    def changeKeyframeBatch(maps, new_keyframes):
        """finalizeKeyFrame() + createKeyFrame(new_keyframes[j]) of several sequences' maps in shared launches
        (lsdhip_depth_change_keyframe_batch); returns the rescale factors"""
        n = len(maps)
        for m, f in zip(maps, new_keyframes):
            m._keep.append(f)
        ma = (C.c_void_p * n)(*[m.h_ for m in maps])
        fa = (C.c_void_p * n)(*[f.h_ for f in new_keyframes])
        s = (C.c_float * n)()
        check(maps[0].L.lsdhip_depth_change_keyframe_batch(n, ma, fa, s), False)
        return [float(v) for v in s]

    @staticmethod
    def reactivateKeyframeBatch(maps, old_keyframes):
        """finalizeKeyFrame() + setFromExistingKF(old_keyframes[j]) of several sequences' maps in three shared launches
        (lsdhip_depth_reactivate_keyframe_batch)"""
        n = len(maps)
        for m, f in zip(maps, old_keyframes):
            m._keep.append(f)
        ma = (C.c_void_p * n)(*[m.h_ for m in maps])
        fa = (C.c_void_p * n)(*[f.h_ for f in old_keyframes])
        check(maps[0].L.lsdhip_depth_reactivate_keyframe_batch(n, ma, fa), False)

    def reactivateKeyframe(self, old_keyframe):
        DepthMap.reactivateKeyframeBatch([self], [old_keyframe])

    def currentDepthMap(self):
        out = np.zeros((self.ctx.h, self.ctx.w), dtype=HYP_DTYPE)
        check(self.L.lsdhip_depth_download(self.h_, out.ctypes.data), False)
        return out

    def setCurrentDepthMap(self, kf, hyp, reactivated=False):
        self._keep.append(kf)
        hyp = np.ascontiguousarray(hyp, dtype=HYP_DTYPE)
        check(self.L.lsdhip_depth_upload(self.h_, kf.h_, hyp.ctypes.data, int(reactivated)), False)

    def debugPlotDepthMap(self, debugDisplay=0, out_dev_ptr=None):
        """DepthMap::debugPlotDepthMap (DepthMap.cpp:1400-1428) drawn on the device: uint8 [h, w, 3], the keyframe in grey with the valid
        hypotheses in the colours of mode `debugDisplay` (the reference's global of that name).  out_dev_ptr: a device buffer of
        3 * w * h bytes instead; the call then only queues the launch and returns None."""
        if out_dev_ptr is not None:
            check(self.L.lsdhip_depth_debug_plot_dev(self.h_, int(debugDisplay), C.c_void_p(out_dev_ptr)), False)
            return None
        out = np.zeros((self.ctx.h, self.ctx.w, 3), np.uint8)
        check(self.L.lsdhip_depth_debug_plot(self.h_, int(debugDisplay), out.ctypes.data), False)
        return out

    @staticmethod
    def debugPlotDepthMapBatch(maps, out_dev_ptrs, debugDisplay=0):
        """the debug images of several maps of one context in one launch, each into its own device buffer (lsdhip_depth_debug_plot_batch);
        queued, nothing waits"""
        n = len(maps)
        ma = (C.c_void_p * n)(*[m.h_ for m in maps])
        oa = (C.c_void_p * n)(*[int(p) for p in out_dev_ptrs])
        check(maps[0].L.lsdhip_depth_debug_plot_batch(n, ma, int(debugDisplay), oa), False)

    def stage(self, name, frames=()):
        frames = list(frames)
        self._keep.extend(frames)
        check(self.L.lsdhip_depth_stage(self.h_, self.STAGES[name], self._arr(frames) if frames else None, len(frames)), False)

    def copyRows(self, row0, nrows, packed_dev_ptr, to_map):
        """rows of the 8 hypothesis planes <-> packed device buffer (29 B/px), see lsdhip_depth_copy_rows_dev"""
        check(self.L.lsdhip_depth_copy_rows_dev(self.h_, row0, nrows, C.c_void_p(packed_dev_ptr), int(to_map)), False)

    def copyPlanesToDevice(self, idepth_ptr, var_ptr):
        check(self.L.lsdhip_depth_copy_planes_dev(self.h_, C.c_void_p(idepth_ptr), C.c_void_p(var_ptr)), False)

    def timings(self):
        out = np.zeros(8, np.float32)
        check(self.L.lsdhip_depth_timings(self.h_, out.ctypes.data))
        keys = ["msUpdate", "msCreate", "msFinalize", "msObserve", "msRegularize", "msPropagate", "msFillHoles", "msSetDepth"]
        return dict(zip(keys, out.tolist()))


class SlamLoop:
    """Minimal single-sequence driver: the part of SlamSystem either side of the hot path, with doSlam=false and
    blockUntilMapped=true semantics (C/SlamSystem.cpp:890-1040 trackFrame, :739-828 doMappingIteration, :542-614
    updateKeyframe, :458-490 createNewCurrentKeyframe), and a deterministic keyframe policy (new keyframe every
    `kf_every` frames) instead of the distance/usage score.  Orchestration only — every per-pixel operation is a
    liblsdhip.so call."""

    def __init__(self, ctx, first_image_or_ptr, depth0, kf_every=10, device_frames=False):
        self.ctx = ctx
        self.device_frames = device_frames
        self.kf_every = kf_every
        self.tracker = SE3Tracker(ctx)
        self.tracker.set_maxItsPerLvl([5, 20, 50, 100, 0])  # C/SlamSystem.cpp:80-81
        self.map = DepthMap(ctx)
        self.reference = TrackingReference()
        self.keyframe = self._frame(0, first_image_or_ptr)
        self.keyframe.setDepthFromGroundTruth(depth0)     # SlamSystem::gtDepthInit (SlamSystem.cpp:831-854)
        self.map.initializeFromGTDepth(self.keyframe)
        self.reference.importFrame(self.keyframe)
        self.keyframe.clearDepthHasBeenUpdatedFlag()
        self.last_frameToKF = IDENTITY.copy()
        self.n_since_kf = 0
        self.frame_id = 0
        self.t_track = 0.0
        self.t_map = 0.0
        self.n_track = 0
        self.n_update = 0
        self.evaluations = 0

    def _frame(self, id_, img):
        if self.device_frames:
            return Frame(self.ctx, id_, device_ptr=img)
        return Frame(self.ctx, id_, image=img)

    def step(self, image_or_ptr, clock):
        """track one frame, then one mapping iteration; returns frameToKeyframe"""
        self.frame_id += 1
        t0 = clock()
        frame = self._frame(self.frame_id, image_or_ptr)
        if self.keyframe.stats()["depthHasBeenUpdatedFlag"]:
            self.reference.importFrame(self.keyframe)
            self.keyframe.clearDepthHasBeenUpdatedFlag()
        est = self.tracker.trackFrame(self.reference, frame, self.last_frameToKF)
        t1 = clock()
        self.t_track += t1 - t0
        self.n_track += 1
        self.evaluations += self.tracker.last.numEvaluations
        if self.tracker.diverged:
            raise RuntimeError("tracking diverged at frame %d" % self.frame_id)
        self.n_since_kf += 1
        if self.n_since_kf >= self.kf_every:
            self.map.finalizeKeyFrame()
            self.map.createKeyFrame(frame)
            self.keyframe = frame
            self.reference.importFrame(frame)
            self.keyframe.clearDepthHasBeenUpdatedFlag()
            self.last_frameToKF = IDENTITY.copy()
            self.n_since_kf = 0
            self.new_keyframe = True
        else:
            self.map.updateKeyframe([frame])
            frame.clear_refPixelWasGood()
            self.last_frameToKF = est
            self.n_update += 1
            self.new_keyframe = False
        self.t_map += clock() - t1
        return est
