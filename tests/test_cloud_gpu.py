"""Keyframe export on the device (lsdhip_frame_pack_keyframe_points, lsdhip_cloud_*) against tests/cloud_ref.py, the float32
restatement of the host functions of include/lsd_slam_hip_io.hpp that tests/test_cloud_ref_cpu.py pins to the header: both sides
perform the same IEEE single-precision operations in the same order, so every comparison is == on the raw bits."""
import os
import subprocess

import numpy as np
import pytest

import cloud_ref as cr
from common import ROOT, sequence, synth

pytestmark = pytest.mark.gpu

SIZES = [(160, 128), (176, 144), (640, 480)]          # 176: rows straddle the 1024-pixel chunks, ragged last chunk; 640x480: 300 chunks
K_OF = lambda w, h: np.array([0.8 * w, 0.82 * w, 0.5 * w - 0.5, 0.5 * h - 0.5], np.float32)
# identity with a tighter absolute threshold (at scale 1 the two thresholds test the same number), and a scale-2 rotated pose with the
# viewer's defaults, where absTH cuts what scaledTH lets through
POSES = {"identity": (cr.IDENTITY_POSE, 1.0, 0.5), "rot2": (cr.POSE_ROT2, 1.0, 1.0)}

_CTX, _IMG, _REF = {}, {}, {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ctx_of(w, h):
    import lsd_slam_amd as la
    if (w, h) not in _CTX:
        _CTX[(w, h)] = la.Context(w, h, K_OF(w, h))
    return _CTX[(w, h)]


def image_of(w, h, i=0):
    if (w, h) not in _IMG:
        _IMG[(w, h)] = np.ascontiguousarray(synth.make_sequence(w, h, 3)[0])
    return _IMG[(w, h)][i]


def map_of(w, h, seed=0):
    return cr.make_map(w, h, seed=w * 1000 + h + seed)


def keyframe(ctx, id_, idepth, var, i=0):
    import lsd_slam_amd as la
    f = la.Frame(ctx, id_, image_of(ctx.w, ctx.h, i))
    f.setDepthPlanes(idepth, var)
    return f


def ref_cloud(w, h, pose, near, seed=0, i=0):
    """restatement of one append (computed once per case, shared by the tests)"""
    key = (w, h, pose, near, seed, i)
    if key not in _REF:
        idepth, var = map_of(w, h, seed)
        c2w, sTH, aTH = POSES[pose]
        _REF[key] = cr.flush_ref(cr.pack_ref(idepth, var, image_of(w, h, i).astype(np.float32)), K_OF(w, h), c2w, sTH, aTH, near)
    return _REF[key]


def test_payload_equals_the_restatement_and_needs_depth():
    import lsd_slam_amd as la
    w, h = 176, 144
    ctx = ctx_of(w, h)
    idepth, var = map_of(w, h)
    assert (idepth <= 0).sum() > 100 and (idepth < 0).sum() > 100 and np.log10(var.max() / var.min()) > 6
    f = keyframe(ctx, 1, idepth, var)
    got = f.keyframePoints()
    ref = cr.pack_ref(idepth, var, image_of(w, h).astype(np.float32))
    assert got.dtype.itemsize == 12 and got.tobytes() == ref.tobytes()
    bare = la.Frame(ctx, 2, image_of(w, h))
    with pytest.raises(la.LsdHipError) as e:
        bare.keyframePoints()
    assert "(-3)" in str(e.value)          # LSDHIP_E_STATE


SINGLE_CASES = [(size, pose, near) for size in SIZES[:2] for pose in ("identity", "rot2") for near in (1, 5, 9)] + [(SIZES[2], "rot2", 5)]


@pytest.mark.parametrize("size,pose,near", SINGLE_CASES)
def test_single_append_equals_the_restatement(size, pose, near):
    import lsd_slam_amd as la
    w, h = size
    ctx = ctx_of(w, h)
    idepth, var = map_of(w, h)
    ref, info = ref_cloud(w, h, pose, near)
    keep = info["keep"]
    print(size, pose, near, {k: v for k, v in info.items() if k != "keep"})
    # every branch fires and passes, by the restatement's own counts
    assert info["kept"] > 0 and info["rej_scaled"] > 0 and info["rej_abs"] > 0 and (info["rej_support"] > 0 or near == 1)
    assert keep[1].any() and keep[h - 2].any() and keep[:, 1].any() and keep[:, w - 2].any()
    assert not (keep[0].any() or keep[h - 1].any() or keep[:, 0].any() or keep[:, w - 1].any())
    assert (idepth[0] > 0).all() and (idepth[h - 1] > 0).all() and (idepth[:, 0] > 0).all() and (idepth[:, w - 1] > 0).all()
    flat = keep.reshape(-1)
    assert any(flat[b - 1] and flat[b] for b in range(1024, w * h, 1024))          # kept neighbours on both sides of a chunk boundary
    c2w, sTH, aTH = POSES[pose]
    f = keyframe(ctx, 7, idepth, var)
    cloud = la.PointCloud(ctx, w * h, 4)
    cloud.appendKeyframe(f, c2w, sTH, aTH, near)
    f.close()                              # dropped right after the call: the append stays valid
    assert (cloud.total(), cloud.stored()) == (len(ref), len(ref))
    got = cloud.download()
    assert got.shape == ref.shape and np.array_equal(bits(got), bits(ref))
    assert cloud.segments() == [(7, 0, len(ref))]


def test_degenerate_maps():
    import lsd_slam_amd as la
    w, h = 176, 144
    ctx = ctx_of(w, h)
    cloud = la.PointCloud(ctx, 2 * w * h, 4)
    idepth, var = cr.dense_map(w, h)
    ref, info = cr.flush_ref(cr.pack_ref(idepth, var, image_of(w, h).astype(np.float32)), K_OF(w, h), cr.POSE_ROT1, 1.0, 1.0, 9)
    assert info["kept"] == (w - 2) * (h - 2)
    cloud.appendKeyframe(keyframe(ctx, 1, idepth, var), cr.POSE_ROT1, 1.0, 1.0, 9)
    assert cloud.total() == (w - 2) * (h - 2) and np.array_equal(bits(cloud.download()), bits(ref))
    cloud.appendKeyframe(keyframe(ctx, 2, *cr.invalid_map(w, h)), cr.POSE_ROT1, 1.0, 1.0, 5)
    assert cloud.total() == (w - 2) * (h - 2)
    assert cloud.segments() == [(1, 0, (w - 2) * (h - 2)), (2, (w - 2) * (h - 2), 0)]


def _three(w, h):
    return [("identity", 5, 0, 0), ("rot2", 5, 1, 1), ("rot2", 1, 2, 2)]       # (pose, near, map seed, image)


def test_chained_appends_segments_and_reset():
    import lsd_slam_amd as la
    w, h = 176, 144
    ctx = ctx_of(w, h)
    jobs = _three(w, h)
    refs = [ref_cloud(w, h, p, n, s, i)[0] for p, n, s, i in jobs]
    frames = [keyframe(ctx, 10 + k, *map_of(w, h, s), i=i) for k, (p, n, s, i) in enumerate(jobs)]
    cloud = la.PointCloud(ctx, w * h * 3, 3)
    rcs = []
    for f, (p, n, s, i) in zip(frames, jobs):          # back to back: no call that waits in between
        c2w, sTH, aTH = POSES[p]
        rcs.append(cloud.appendKeyframe(f, c2w, sTH, aTH, n))
    assert rcs == [True, True, False]                  # the third append takes the last row of the segment table
    cat = np.concatenate(refs)
    assert cloud.total() == len(cat) and np.array_equal(bits(cloud.download()), bits(cat))
    firsts = np.cumsum([0] + [len(r) for r in refs])
    assert cloud.segments() == [(10 + k, int(firsts[k]), len(refs[k])) for k in range(3)]
    # a fourth keyframe: its points are appended, the full table keeps its three rows
    c2w, sTH, aTH = POSES["identity"]
    assert cloud.appendKeyframe(frames[0], c2w, sTH, aTH, 5) is False
    assert cloud.total() == len(cat) + len(refs[0]) and len(cloud.segments()) == 3
    cloud.reset()
    assert (cloud.total(), cloud.stored(), cloud.segments()) == (0, 0, [])
    cloud.appendKeyframe(frames[1], *POSES["rot2"], 5)
    assert cloud.segments() == [(11, 0, len(refs[1]))] and np.array_equal(bits(cloud.download()), bits(refs[1]))


def test_overflow_is_counted_not_written():
    import lsd_slam_amd as la
    w, h = 176, 144
    ctx = ctx_of(w, h)
    jobs = _three(w, h)
    refs = [ref_cloud(w, h, p, n, s, i)[0] for p, n, s, i in jobs]
    cap = len(refs[0]) + len(refs[1]) // 2
    cloud = la.PointCloud(ctx, cap, 8)
    for k, (p, n, s, i) in enumerate(jobs):
        c2w, sTH, aTH = POSES[p]
        cloud.appendKeyframe(keyframe(ctx, k, *map_of(w, h, s), i=i), c2w, sTH, aTH, n)
    ctx.synchronize()                                  # a HIP error of the launches would surface here
    cat = np.concatenate(refs)
    assert cloud.stored() == cap and cloud.total() == len(cat) > cap
    assert np.array_equal(bits(cloud.download(0, cap)), bits(cat[:cap]))
    guard = cloud.download(cap, la.PointCloud.GUARD_POINTS)
    assert (guard.view(np.uint32) == 0xFFFFFFFF).all()               # the fill of creation, untouched
    assert [s[2] for s in cloud.segments()] == [len(r) for r in refs]


@pytest.mark.parametrize("n", [1, 3, 9])
def test_batch_equals_single(n):
    import lsd_slam_amd as la
    w, h = 160, 128
    ctx = ctx_of(w, h)
    poses = [cr.wire_pose([0.1 * j - 0.3, 1.0, 0.2], 0.2 + 0.1 * j, 1.0 + 0.25 * (j % 3), [j, -0.5 * j, 1.0]) for j in range(n)]
    maps = [map_of(w, h, seed=j) for j in range(n)]
    if n > 1:
        maps[1] = cr.invalid_map(w, h)                 # one job without a single point
    frames = [keyframe(ctx, 20 + j, *maps[j], i=j % 3) for j in range(n)]
    single = []
    for j in range(n):
        c = la.PointCloud(ctx, w * h, 2)
        c.appendKeyframe(frames[j], poses[j], 1.0, 1.0, 5)
        single.append((c.total(), c.segments(), c.download().tobytes()))
    clouds = [la.PointCloud(ctx, w * h, 2) for _ in range(n)]
    la.PointCloud.appendBatch(clouds, frames, poses, 1.0, 1.0, 5)
    for j in range(n):
        assert (clouds[j].total(), clouds[j].segments(), clouds[j].download().tobytes()) == single[j], j
    assert sum(s[0] for s in single) > 0 and (n == 1 or single[1][0] == 0)
    if n > 1:                                          # one cloud named twice: an argument error, nothing changes
        with pytest.raises(la.LsdHipError) as e:
            la.PointCloud.appendBatch([clouds[0], clouds[1], clouds[0]], frames[:3], poses[:3], 1.0, 1.0, 5)
        assert "(-1)" in str(e.value)
        for j in range(n):
            assert (clouds[j].total(), clouds[j].segments(), clouds[j].download().tobytes()) == single[j], j


def test_append_is_deterministic_run_to_run():
    import lsd_slam_amd as la
    w, h = 640, 480
    ctx = ctx_of(w, h)
    c2w, sTH, aTH = POSES["rot2"]
    f = keyframe(ctx, 1, *map_of(w, h))
    out = []
    for _ in range(2):
        c = la.PointCloud(ctx, w * h, 2)
        c.appendKeyframe(f, c2w, sTH, aTH, 5)
        out.append(c.download().tobytes())
    assert out[0] == out[1] and len(out[0]) == 16 * len(ref_cloud(w, h, "rot2", 5)[0])


def test_pipelined_context_reads_the_latest_planes():
    """after a Frame::setDepth on the mapping stream that has not been published to the tracker yet, the cloud is built from the planes
    Frame.idepth(0) returns at that moment"""
    import lsd_slam_amd as la
    w, h = 160, 128
    frames, depth0, K, gt = sequence(w, h, 3)
    ctx = la.Context(w, h, K)
    ctx.set_pipeline(True)
    ctx.set_async(True)
    kf = la.Frame(ctx, 0, frames[0])
    kf.setDepthFromGroundTruth(depth0)
    published = kf.idepth(0).copy()
    dm = la.DepthMap(ctx)
    dm.initializeFromGTDepth(kf)
    tracker = la.SE3Tracker(ctx)
    ref = la.TrackingReference()
    ref.importFrame(kf)
    kf.clearDepthHasBeenUpdatedFlag()
    f1 = la.Frame(ctx, 1, frames[1])
    tracker.trackFrame(ref, f1, la.IDENTITY)
    dm.updateKeyframe([f1])                            # Frame::setDepth into the second plane set: pending, not published
    cloud = la.PointCloud(ctx, w * h, 2)
    cloud.appendKeyframe(kf, cr.POSE_ROT2, 1.0, 1.0, 5)
    idepth, var = kf.idepth(0), kf.idepthVar(0)
    assert not np.array_equal(idepth, published)       # the update changed the map, and the tracker has not been handed the planes
    want, info = cr.flush_ref(cr.pack_ref(idepth, var, kf.image(0)), K, cr.POSE_ROT2, 1.0, 1.0, 5)
    got = cloud.download()
    assert info["kept"] > 100 and np.array_equal(bits(got), bits(want))
    assert kf.keyframePoints().tobytes() == cr.pack_ref(idepth, var, kf.image(0)).tobytes()
    del cloud, tracker, dm, f1, kf
    ctx.set_pipeline(False)
    ctx.close()


def _ply(path):
    head, body = open(path, "rb").read().split(b"end_header\n", 1)
    n = int(head.split(b"element vertex ")[1].split(b"\n")[0])
    assert len(body) == 16 * n
    return n, body


def test_dataset_slam_cloud_modes(tmp_path):
    w, h, n = 160, 128, 20
    frames, depth0, K, gt = sequence(w, h, n)
    lst = []
    for i in range(n):
        p = tmp_path / ("f%04d.pgm" % i)
        with open(p, "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (w, h))
            f.write(frames[i].tobytes())
        lst.append(str(p))
    (tmp_path / "files.txt").write_text("\n".join(lst) + "\n")
    (tmp_path / "calib.cfg").write_text("%f %f %f %f 0\n%d %d\nnone\n%d %d\n" % (K[0], K[1], K[2], K[3], w, h, w, h))
    exe = os.path.join(ROOT, "lsd_slam_amd", "dataset_slam")
    both = tmp_path / "both"
    both.mkdir()
    out = subprocess.check_output([exe, str(tmp_path / "calib.cfg"), str(tmp_path / "files.txt"), str(both), "--kf-every", "5", "--cloud", "both"],
                                  timeout=120).decode()
    s = dict(zip(out.split()[0::2], map(int, out.split()[1::2])))
    assert s["keyframes"] == 4 and s["points"] > 0
    assert (both / "pc_device.ply").read_bytes() == (both / "pc.ply").read_bytes()
    msgs = sorted(p for p in os.listdir(both) if p.startswith("keyframe_") and not p.endswith("_device.msg"))
    assert len(msgs) == 4
    for m in msgs:
        assert (both / m.replace(".msg", "_device.msg")).read_bytes() == (both / m).read_bytes(), m
    dev = tmp_path / "dev"
    dev.mkdir()
    r = subprocess.run([exe, str(tmp_path / "calib.cfg"), str(tmp_path / "files.txt"), str(dev), "--kf-every", "5", "--cloud", "device"],
                       timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    nv, _ = _ply(dev / "pc.ply")
    seg = np.loadtxt(dev / "segments.txt", dtype=np.int64).reshape(-1, 3)
    assert nv == int(seg[:, 2].sum()) > 0 and len(seg) == 4
    assert len([p for p in os.listdir(dev) if p.startswith("keyframe_")]) == 4


def test_batch_loop_cloud_sinks():
    """SlamLoopBatch::setCloudSinks: the keyframes that change in a step go into one appendBatch behind the keyframe change; every
    sequence's cloud equals single appends on its kept keyframes with the same poses"""
    import lsd_slam_amd as la
    from lsd_slam_amd.driver import DriverLoopBatch
    w, h, S, steps, every = 160, 128, 4, 12, 4
    seqs = [sequence(w, h, steps + 1, s) for s in range(S)]
    K = seqs[0][2]
    imgs = [[np.ascontiguousarray(seqs[s][0][t]) for s in range(S)] for t in range(steps + 1)]
    drv = DriverLoopBatch(w, h, K, [im.ctypes.data for im in imgs[0]], [seqs[s][1] for s in range(S)], kf_every=every, images_on_device=False)
    drv.keep_keyframes(True)
    drv.set_cloud_sinks(w * h * 4, 8)
    done, _ = drv.run([[im.ctypes.data for im in imgs[t]] for t in range(1, steps + 1)])
    assert done == steps
    ctx = la.Context.view(drv.ctx_handle(), w, h)
    for s in range(S):
        cloud = drv.cloud(s, ctx)
        segs = cloud.segments()
        assert [g[0] for g in segs] == [0, 4, 8] and all(g[2] > 0 for g in segs), segs      # the keyframes finalised at steps 4, 8, 12
        assert cloud.total() == sum(g[2] for g in segs) == segs[-1][1] + segs[-1][2]
        for k, (id_, first, count) in enumerate(segs):          # k - 1 = -1: the initial keyframe, replaced at step 4; 0, 1: keyframes 4 and 8 of the log
            kf = drv.kept_keyframe(s, k - 1, ctx)
            assert kf.id() == id_
            one = la.PointCloud(ctx, w * h, 2)
            one.appendKeyframe(kf, drv.cloud_pose(s, id_), 1.0, 1.0, 5)
            assert one.total() == count and one.download().tobytes() == cloud.download(first, count).tobytes(), (s, id_)
            one.close()
    drv.close()
