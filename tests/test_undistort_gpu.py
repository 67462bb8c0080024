"""Raw FOV-camera images on the device: lsdhip_undistorter_apply and the lsdhip_frame_create_undistorted* creators against the host
yardstick lsd_slam_hip::Undistorter (include/lsd_slam_hip_io.hpp, run through tests/cpp/undistort_test.cpp), byte for byte and bit for
bit; the sequence loops and dataset_slam fed raw images against the same loops fed the host-rectified ones.  Camera: the reference's FOV
example with dist = 0.93 (undistort_ref.FOV_EXAMPLE); shapes: the 160x128 / 176x144 outputs of the suite from 176x144, 160x128 and 208x160 raw images."""
import os
import subprocess

import numpy as np
import pytest

from common import ROOT, assert_bit_equal
import undistort_ref as ur

pytestmark = pytest.mark.gpu

CAM = ur.FOV_EXAMPLE
PINHOLE = CAM[:4] + (0.0,)
# (mode, input size, output size): every mode at the three input shapes
APPLY_CASES = [(m, i, o) for m, shapes in (
    ("crop", [((176, 144), (160, 128)), ((160, 128), (160, 128)), ((208, 160), (160, 128))]),
    ("full", [((176, 144), (160, 128)), ((160, 128), (160, 128)), ((208, 160), (160, 128))]),
    ("explicit", [((176, 144), (160, 128)), ((160, 128), (176, 144)), ((208, 160), (176, 144))]),
    ("none", [((176, 144), (160, 128)), ((160, 128), (176, 144)), ((208, 160), (160, 128))])) for i, o in shapes]


@pytest.fixture(scope="module")
def hip():
    import lsd_slam_amd as la
    return la


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """the host yardstick: (program, directory, cache of cameras)"""
    d = tmp_path_factory.mktemp("undist_gpu")
    return {"exe": ur.compile_cpp(ROOT, d), "dir": d, "cams": {}}


def camera(host, mode, in_size, out_size, in5=None):
    """tables and K of the C++ builder for one camera, built once per module"""
    if in5 is None:
        in5 = PINHOLE if mode == "none" else CAM
    key = (mode, in_size, out_size, in5)
    if key not in host["cams"]:
        name = "%s_%dx%d_%dx%d_%d" % (mode, in_size[0], in_size[1], out_size[0], out_size[1], len(host["cams"]))
        t = ur.cpp_tables(host["exe"], host["dir"] / name, ur.cfg_text(in5, in_size, ur.line3_of(mode), out_size), out_size)
        t["K32"] = t["K"].astype(np.float32)
        assert not t["passthrough"]
        host["cams"][key] = t
    return host["cams"][key]


def host_undistort(host, cam, imgs, out_size):
    return ur.cpp_undistort(host["exe"], cam, imgs, out_size)


# ---- 4. lsdhip_undistorter_apply -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("mode,in_size,out_size", APPLY_CASES + [("crop", (752, 480), (640, 480))])
def test_apply_equals_host_undistort(hip, host, mode, in_size, out_size, on_device):
    in5 = (0.527334, 0.827306, 0.473568, 0.499436, 0.928161) if in_size == (752, 480) else None
    cam = camera(host, mode, in_size, out_size, in5)
    imgs = ur.random_images(2, in_size[0], in_size[1], seed=in_size[0] + out_size[0])
    want = host_undistort(host, cam, imgs, out_size)
    ctx = hip.Context(out_size[0], out_size[1], cam["K32"])
    u = hip.Undistorter(ctx, in_size[0], in_size[1], cam["remapX"], cam["remapY"])
    for k in range(2):
        if on_device:
            import torch
            d = torch.from_numpy(imgs[k]).cuda()
            o = torch.full((out_size[1], out_size[0]), 77, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            assert u.apply(device_ptr=d.data_ptr(), out_device_ptr=o.data_ptr()) is None
            ctx.synchronize()
            got = o.cpu().numpy()
        else:
            got = u.apply(raw=imgs[k])
        assert np.array_equal(got, want[k]), "%d bytes differ" % int((got != want[k]).sum())
    if mode == "full":
        assert (want[:, cam["remapX"] < 0] == 0).all() and (cam["remapX"] < 0).mean() > 0.3
    u.close()
    ctx.close()


def test_undistorter_refuses_a_table_that_leaves_the_image(hip, host):
    """the kernels read four taps around an entry without a bounds test: a table that would take them outside the raw image is refused"""
    cam = camera(host, "crop", (176, 144), (160, 128))
    ctx = hip.Context(160, 128, cam["K32"])
    for x, y in ((175.0, 10.0), (10.0, 143.0), (np.nan, 10.0), (10.0, -1.0), (1e9, 1.0)):
        rx, ry = cam["remapX"].copy(), cam["remapY"].copy()
        rx[5, 7], ry[5, 7] = x, y
        with pytest.raises(hip.LsdHipError):
            hip.Undistorter(ctx, 176, 144, rx, ry)
    ctx.close()


# ---- 5. frame creation ------------------------------------------------------------------------------------------------------------------
def assert_frames_equal(a, b, what, depth):
    for lvl in range(5):
        assert_bit_equal(a.image(lvl), b.image(lvl), "%s: image level %d" % (what, lvl))
    for lvl in range(1, 5):
        assert_bit_equal(a.gradients(lvl), b.gradients(lvl), "%s: gradients level %d" % (what, lvl))
    assert a.refPixelWasGoodNoCreate() is None
    # as a keyframe: the level-0 planes are built on demand
    a.setDepthFromGroundTruth(depth)
    assert_bit_equal(a.gradients(0), b.gradients(0), "%s: gradients level 0" % what)
    assert_bit_equal(a.maxGradients(0), b.maxGradients(0), "%s: maxGradients" % what)
    for lvl in range(5):
        assert_bit_equal(a.idepth(lvl), b.idepth(lvl), "%s: idepth level %d" % (what, lvl))


@pytest.mark.parametrize("mode,in_size,out_size", [("crop", (176, 144), (160, 128)), ("full", (208, 160), (176, 144))])
def test_frames_of_raw_images_equal_frames_of_host_rectified_images(hip, host, mode, in_size, out_size):
    """lsdhip_frame_create_undistorted, _async, _from_device and _batch (n = 3: two raw images and the first repeated; host and device)
    against lsdhip_frame_create on the bytes Undistorter::undistort wrote on the host"""
    import torch
    cam = camera(host, mode, in_size, out_size)
    raws = ur.random_images(2, in_size[0], in_size[1], seed=11)
    # smooth content as well: the noise of random_images saturates every gradient
    yy, xx = np.mgrid[0:in_size[1], 0:in_size[0]]
    raws[1] = (128 + 100 * np.sin(xx / 7.0) * np.cos(yy / 5.0)).astype(np.uint8)
    rect = host_undistort(host, cam, raws, out_size)
    ctx = hip.Context(out_size[0], out_size[1], cam["K32"])
    u = hip.Undistorter(ctx, in_size[0], in_size[1], cam["remapX"], cam["remapY"])
    depth = np.full((out_size[1], out_size[0]), 2.0, np.float32)
    want = []
    for k in range(2):
        f = hip.Frame(ctx, 100 + k, rect[k])
        f.setDepthFromGroundTruth(depth)
        want.append(f)
    dev = torch.from_numpy(raws).cuda()
    torch.cuda.synchronize()
    for k in range(2):
        assert_frames_equal(u.frame(1 + k, raw=raws[k]), want[k], "create_undistorted %d" % k, depth)
        fa = u.frame(3 + k, raw=raws[k], wait=False)
        assert_frames_equal(fa, want[k], "create_undistorted_async %d" % k, depth)
        assert_frames_equal(u.frame(5 + k, device_ptr=dev[k].data_ptr()), want[k], "create_undistorted_from_device %d" % k, depth)
    order = [0, 1, 0]
    for on_device in (False, True):
        if on_device:
            batch = u.createBatch([20, 21, 22], device_ptrs=[dev[j].data_ptr() for j in order])
        else:
            batch = u.createBatch([20, 21, 22], raws=[raws[j] for j in order])
        for j, k in enumerate(order):
            assert batch[j].id() == 20 + j
            assert_frames_equal(batch[j], want[k], "create_undistorted_batch %s entry %d" % ("device" if on_device else "host", j), depth)
    # two async creations in a row share the undistorter's staging slot: the stream orders the second upload behind the first launch
    f0 = u.frame(30, raw=raws[0], wait=False)
    f1 = u.frame(31, raw=raws[1], wait=False)
    assert_frames_equal(f0, want[0], "back-to-back async 0", depth)
    assert_frames_equal(f1, want[1], "back-to-back async 1", depth)
    del batch, f0, f1, fa, want
    u.close()
    ctx.close()


# ---- 6. loops ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loop_data(host):
    """13 raw 176x144 frames of two scenes, their host-rectified 160x128 images and the depth of frame 0, made once"""
    in_size, out_size, n = (176, 144), (160, 128), 13
    cam = camera(host, "crop", in_size, out_size)
    seqs = []
    for s in range(2):
        raws, depth0 = ur.raw_sequence(s, n, cam["K32"], CAM, in_size, out_size)
        rect = host_undistort(host, cam, raws, out_size)
        seqs.append({"raw": [np.ascontiguousarray(r) for r in raws], "rect": [np.ascontiguousarray(r) for r in rect], "depth0": depth0})
    return cam, in_size, out_size, n, seqs


HYP_FIELDS = ("isValid", "blacklisted", "nextStereoFrameMinID", "validity_counter", "idepth", "idepth_var", "idepth_smoothed", "idepth_var_smoothed")


def assert_maps_identical(a, b, what):
    assert (a["isValid"] > 0).sum() > 500, "%s: the map is nearly empty" % what
    for k in HYP_FIELDS:
        if k in ("isValid", "blacklisted", "nextStereoFrameMinID", "validity_counter"):
            assert np.array_equal(a[k], b[k]), "%s: %s differs at %d pixels" % (what, k, int((a[k] != b[k]).sum()))
        else:
            v = a["isValid"] > 0
            assert_bit_equal(a[k][v], b[k][v], "%s: %s" % (what, k))


@pytest.mark.parametrize("pipelined", [False, True])
def test_slam_loop_on_raw_images_equals_loop_on_rectified_images(loop_data, pipelined):
    """12 frames: lsd_slam_hip::SlamLoop with a DeviceUndistorter fed raw images against the same loop fed the host-rectified images —
    poses and final map bit-identical, nothing lost, in both execution models"""
    from lsd_slam_amd.driver import DriverLoop
    cam, (iw, ih), (w, h), n, seqs = loop_data
    q = seqs[0]
    runs = []
    for raw in (False, True):
        imgs = q["raw"] if raw else q["rect"]
        drv = DriverLoop(w, h, cam["K32"], imgs[0].ctypes.data, q["depth0"], kf_every=5, images_on_device=False,
                         undistort=(iw, ih, cam["remapX"], cam["remapY"]) if raw else None)
        drv.set_pipeline(pipelined)
        done, poses = drv.run([imgs[t].ctypes.data for t in range(1, n)], want_poses=True)
        st = drv.stats()
        m = drv.download_map()
        drv.close()
        assert done == n - 1 and int(st.tracked_good) == n - 1 and int(st.keyframes) == 2, (raw, done, int(st.tracked_good), int(st.keyframes))
        runs.append((np.asarray(poses), m, int(st.dropped)))
    assert np.array_equal(runs[0][0], runs[1][0]), "poses differ"
    assert runs[0][2] == runs[1][2]
    assert_maps_identical(runs[0][1].reshape(-1), runs[1][1].reshape(-1), "final map")


def test_slam_loop_batch_on_raw_images_equals_batch_on_rectified_images(loop_data):
    """the same with lsd_slam_hip::SlamLoopBatch at S = 3 (scenes 0, 1, 0)"""
    from lsd_slam_amd.driver import DriverLoopBatch
    cam, (iw, ih), (w, h), n, seqs = loop_data
    S = 3
    qs = [seqs[s % 2] for s in range(S)]
    runs = []
    for raw in (False, True):
        imgs = [q["raw"] if raw else q["rect"] for q in qs]
        bl = DriverLoopBatch(w, h, cam["K32"], [imgs[s][0].ctypes.data for s in range(S)], [q["depth0"] for q in qs], kf_every=5,
                             images_on_device=False, undistort=(iw, ih, cam["remapX"], cam["remapY"]) if raw else None)
        done, poses = bl.run([[imgs[s][t].ctypes.data for s in range(S)] for t in range(1, n)], want_poses=True)
        st = bl.stats()
        maps = [bl.download_map(s, w, h) for s in range(S)]
        bl.close()
        assert done == n - 1
        for s in range(S):
            assert st[s]["tracked_good"] == n - 1 and st[s]["lost"] == 0 and st[s]["keyframes"] == 2, (raw, s, st[s])
        runs.append((np.asarray(poses), maps))
    assert np.array_equal(runs[0][0], runs[1][0]), "poses differ"
    for s in range(S):
        assert_maps_identical(runs[0][1][s].reshape(-1), runs[1][1][s].reshape(-1), "final map of sequence %d" % s)


# ---- 7. dataset_slam --undistort 1 ----------------------------------------------------------------------------------------------------
def write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(img.tobytes())


def test_dataset_slam_undistort_equals_run_on_rectified_images(loop_data, tmp_path):
    """dataset_slam --undistort 1 on raw PGMs with the FOV calibration file writes the pose file that dataset_slam writes on the rectified
    PGMs with the rectified calibration file of the first run; the rectified PGMs it dumps are the host's bytes; without the flag the
    FOV file is refused as before"""
    cam, (iw, ih), (w, h), n, seqs = loop_data
    q = seqs[0]
    exe = os.path.join(ROOT, "lsd_slam_amd", "dataset_slam")
    rawdir, rectdir, out1, out2 = (tmp_path / d for d in ("raw", "rect", "out1", "out2"))
    for d in (rawdir, rectdir, out1, out2):
        d.mkdir()
    for i in range(n):
        write_pgm(rawdir / ("f%04d.pgm" % i), q["raw"][i])
    (tmp_path / "raw.txt").write_text("".join("%s\n" % (rawdir / ("f%04d.pgm" % i)) for i in range(n)))
    (tmp_path / "rect.txt").write_text("".join("%s\n" % (rectdir / ("f%04d.pgm" % i)) for i in range(n)))
    o1 = subprocess.check_output([exe, cam["cfg"], str(tmp_path / "raw.txt"), str(out1), "--kf-every", "5", "--undistort", "1",
                                  "--rectified-images", str(rectdir)], timeout=120).decode()
    for i in range(n):
        got = np.fromfile(rectdir / ("f%04d.pgm" % i), np.uint8)[-w * h:].reshape(h, w)
        assert np.array_equal(got, q["rect"][i]), "rectified image %d" % i
    o2 = subprocess.check_output([exe, str(out1 / "rectified.cfg"), str(tmp_path / "rect.txt"), str(out2), "--kf-every", "5"], timeout=120).decode()
    s1 = dict(zip(o1.split()[0::2], map(int, o1.split()[1::2])))
    assert s1["frames"] == n - 1 and s1["keyframes"] >= 2
    assert o1 == o2
    t1, t2 = (out1 / "trajectory.txt").read_bytes(), (out2 / "trajectory.txt").read_bytes()
    assert len(t1.splitlines()) == n and t1 == t2
    r = subprocess.run([exe, cam["cfg"], str(tmp_path / "raw.txt"), str(out2)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 1 and b"rectify the images first" in r.stderr
