"""lsd_slam_hip::Undistorter (include/lsd_slam_hip_io.hpp: the reference's UndistorterPTAM, util/Undistorter.cpp:91-411) without a GPU:
the float32 table builder against a float64 restatement, the bilinear gather against a float32 restatement on the same tables, and the
calibration-file forms it accepts and refuses.  The camera is the reference's FOV example with dist = 0.93."""
import os
import subprocess

import numpy as np
import pytest

from common import ROOT
import undistort_ref as ur

CAM = ur.FOV_EXAMPLE
EXPLICIT = ur.EXPLICIT
# name -> (first-line values, input size, line 3, output size)
CASES = {
    "crop": (CAM, (176, 144), "crop", (160, 128)),
    "crop_same_size": (CAM, (160, 128), "crop", (160, 128)),
    "full": (CAM, (176, 144), "full", (160, 128)),
    "full_same_size": (CAM, (160, 128), "full", (160, 128)),
    "explicit": (CAM, (208, 160), ur.line3_of("explicit"), (176, 144)),
    "none_resize": (CAM[:4] + (0.0,), (208, 160), "none", (160, 128)),
    "passthrough": (CAM[:4] + (0.0,), (160, 128), "none", (160, 128)),
}


def cfg_text(case):
    in5, in_size, l3, out_size = CASES[case]
    return ur.cfg_text(in5, in_size, l3, out_size)


def restated(case, dtype=np.float64):
    in5, (iw, ih), l3, (ow, oh) = CASES[case]
    mode = l3 if l3 in ("crop", "full", "none") else "explicit"
    return ur.build(in5, iw, ih, mode, ow, oh, out5=EXPLICIT, dtype=dtype)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from lsd_slam_amd import build
    build.build()
    d = tmp_path_factory.mktemp("undist")
    return ur.compile_cpp(ROOT, d), d


@pytest.fixture(scope="module")
def built(exe):
    """every case through the C++ builder once: name -> dict(dir, cfg, K, outcal, passthrough, remapX, remapY, same_K)"""
    prog, d = exe
    return {name: ur.cpp_tables(prog, d / name, cfg_text(name), CASES[name][3]) for name in CASES}


@pytest.mark.parametrize("case", ["crop", "crop_same_size", "full", "full_same_size", "explicit", "none_resize"])
def test_tables_and_K_against_float64(built, case):
    """The float32 builder against the float64 restatement.  Bound on a coordinate: 16 ulp32(in_width) pixels (the chain from x to ix has at
    most 16 float32 roundings of values no larger than in_width); K: the same bound relative to its value.  The valid masks may differ
    only where the float64 coordinate lies within that bound of 0, in_w - 1 or in_h - 1; such pixels must stay below 0.5 % of the image.
    Counted with the float64 restatement for this camera (pixels within the bound of a border / mask differences float32 against float64):
    crop 1 / 0, crop_same_size 4 / 0, full 0 / 0, full_same_size 1 / 0, explicit 0 / 0, none_resize 0 / 0 of 20480 pixels (explicit:
    25344) — at most 0.02 %, and the masks are equal everywhere; the largest coordinate error is 3.7e-5 px against a bound of 2.4e-4.
    The largest valid coordinates of crop_same_size are 158.9998 of 159 and 126.99999 of 127: the border clauses are exercised."""
    in5, (iw, ih), l3, (ow, oh) = CASES[case]
    ref = restated(case)
    got = built[case]
    bound = 16.0 * float(np.spacing(np.float32(iw)))
    for k in range(4):
        assert abs(got["K"][k] - float(ref["K"][k])) <= 16.0 * float(np.spacing(np.float32(abs(float(ref["K"][k]))))), ("K", k, got["K"], ref["K"])
        assert abs(got["outcal"][k] - float(ref["out_cal"][k])) <= 16.0 * float(np.spacing(np.float32(abs(float(ref["out_cal"][k]))))), ("outcal", k)
    assert got["same_K"], "the rectified calibration file does not read back to K"
    valid32 = ~(got["remapX"] < 0)
    assert np.array_equal(valid32, ~(got["remapY"] < 0))
    cx, cy = ref["coordX"], ref["coordY"]
    near = (np.abs(cx) <= bound) | (np.abs(cy) <= bound) | (np.abs(cx - (iw - 1)) <= bound) | (np.abs(cy - (ih - 1)) <= bound)
    differ = valid32 != ref["valid"]
    print("%s: bound %.3g px, %d pixels near a border, %d mask differences, %d invalid of %d, max valid coordinate (%.4f, %.4f)" % (
        case, bound, int(near.sum()), int(differ.sum()), int((~valid32).sum()), valid32.size, float(got["remapX"].max()), float(got["remapY"].max())))
    assert not (differ & ~near).any(), "valid masks differ away from the borders"
    assert near.sum() <= 0.005 * near.size
    both = valid32 & ref["valid"]
    ex = np.abs(got["remapX"].astype(np.float64) - cx)[both].max()
    ey = np.abs(got["remapY"].astype(np.float64) - cy)[both].max()
    print("%s: max coordinate error %.3g / %.3g px" % (case, ex, ey))
    assert ex <= bound and ey <= bound
    # invalid entries are written as -1 in both planes
    assert (got["remapX"][~valid32] == -1).all() and (got["remapY"][~valid32] == -1).all()
    if case.startswith("crop"):
        assert valid32.all()                                    # crop leaves no invalid pixel at these shapes
    if case.startswith("full"):
        assert 0.30 < (~valid32).mean() < 0.40                  # full: about 34.8 % of the output lies outside the input image


def test_passthrough_has_no_tables(built):
    got = built["passthrough"]
    assert got["passthrough"] and got["same_K"]
    iw, ih = CASES["passthrough"][1]
    want = [CAM[0] * iw, CAM[1] * ih, CAM[2] * iw - 0.5, CAM[3] * ih - 0.5]
    assert np.allclose(got["K"], want, rtol=1e-6)
    assert not built["none_resize"]["passthrough"]


@pytest.mark.parametrize("case", ["crop", "full", "explicit", "none_resize", "passthrough", "crop_same_size"])
def test_undistort_bytes_against_float32(exe, built, case):
    """Undistorter::undistort against the float32 restatement on the tables the C++ program dumped: equal bytes."""
    prog, _ = exe
    (iw, ih), (ow, oh) = CASES[case][1], CASES[case][3]
    imgs = ur.random_images(3, iw, ih, seed=len(case))
    got = ur.cpp_undistort(prog, built[case], imgs, (ow, oh))
    if case == "passthrough":
        assert np.array_equal(got, imgs)
        return
    rx, ry = built[case]["remapX"], built[case]["remapY"]
    for k in range(3):
        want = ur.undistort_f32(imgs[k], rx, ry)
        assert np.array_equal(got[k], want), "image %d: %d bytes differ" % (k, int((got[k] != want).sum()))
    assert (got == 0).any() and (got == 255).any()
    if case == "full":
        outside = rx < 0
        assert outside.sum() > 0.3 * outside.size and (got[:, outside] == 0).all()
        assert (got[1][~outside] != 0).mean() > 0.9


def parse(exe, tmp_path, text):
    prog, _ = exe
    p = tmp_path / "c.cfg"
    p.write_text(text)
    out = subprocess.check_output([prog, "parse", str(p)]).decode().splitlines()
    return out[0].split(": ", 1)[1], out[1].split(": ", 1)[1]


def test_parsing_reference_forms(exe, tmp_path):
    # the three example files of the reference's calib/ folder, written out here
    fov = "0.527334 0.827306 0.473568 0.499436 0.928161\n752 480\ncrop\n640 480\n"
    opencv = "500 500 350 240 0 0 0 0\n752 480\ncrop\n640 480\n"
    pinhole = "0.527334 0.827306 0.473568 0.499436 0\n752 480\nnone\n752 480\n"
    u, p = parse(exe, tmp_path, fov)
    assert u == "ok" and "rectify the images first" in p            # parseCalibration still refuses the FOV file
    u, p = parse(exe, tmp_path, pinhole)
    assert u == "ok" and p == "ok"
    u, p = parse(exe, tmp_path, opencv)
    assert "OpenCV camera model" in u and "not supported" in u
    # the other forms of line 3
    assert parse(exe, tmp_path, fov.replace("crop", "full"))[0] == "ok"
    assert parse(exe, tmp_path, fov.replace("crop", "0.4 0.53 0.5 0.5 0"))[0] == "ok"
    assert "third line" in parse(exe, tmp_path, fov.replace("crop", "something"))[0]
    # refusals
    assert "multiple of 16" in parse(exe, tmp_path, fov.replace("640 480", "650 480"))[0]
    assert "multiple of 16" in parse(exe, tmp_path, pinhole.replace("752 480\nnone\n752 480", "750 480\nnone\n750 480"))[1]   # "the same error as today"
    assert "relative" in parse(exe, tmp_path, "400 400 320 240 0.9\n752 480\ncrop\n640 480\n")[0]
    assert "undefined in the reference" in parse(exe, tmp_path, fov.replace("crop", "none"))[0]


def test_fov_example_output_intrinsics(exe, tmp_path):
    """752x480 -> 640x480 crop of the reference's example: the C++ K against the float64 restatement, and a sane field of view"""
    prog, _ = exe
    p = tmp_path / "fov.cfg"
    p.write_text("0.527334 0.827306 0.473568 0.499436 0.928161\n752 480\ncrop\n640 480\n")
    rows = {l.split()[0]: l.split()[1:] for l in subprocess.check_output([prog, "tables", str(p), str(tmp_path)]).decode().splitlines()}
    K = np.array(rows["K"], np.float64)
    ref = ur.build((0.527334, 0.827306, 0.473568, 0.499436, 0.928161), 752, 480, "crop", 640, 480)
    for k in range(4):
        assert abs(K[k] - float(ref["K"][k])) <= 16.0 * float(np.spacing(np.float32(float(ref["K"][k]))))
    assert 200 < K[0] < 400 and 200 < K[1] < 400 and 250 < K[2] < 390 and 190 < K[3] < 290
    rx = np.fromfile(tmp_path / "remapX.f32", np.float32)
    assert (rx > 0).all() and rx.max() < 751
