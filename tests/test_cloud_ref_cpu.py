"""tests/cloud_ref.py (the float32 numpy restatement the device export is held to) against the product's own host code: a small program
runs include/lsd_slam_hip_io.hpp's payload fill, serializeKeyframeMsg and flushPointCloud on planes from a file, built with plain
g++ -O1 (no FMA), and every output bit must agree.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import cloud_ref as cr
from common import ROOT, synth

K_OF = lambda w, h: np.array([0.8 * w, 0.82 * w, 0.5 * w - 0.5, 0.5 * h - 0.5], np.float32)
HEADER_BYTES = 4 + 8 + 1 + 28 + 16 + 8 + 4


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from lsd_slam_amd import build
    build.build()
    d = tmp_path_factory.mktemp("cloudref")
    out = str(d / "cloud_ref_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "cloud_ref_test.cpp"),
                           "-o", out, "-L" + os.path.join(ROOT, "lsd_slam_amd"), "-llsdhip", "-Wl,-rpath," + os.path.join(ROOT, "lsd_slam_amd")])
    return out


_MAPS = {}


def planes(w, h):
    if (w, h) not in _MAPS:
        idepth, var = cr.make_map(w, h, seed=w * 1000 + h)
        image = synth.make_sequence(w, h, 1)[0][0].astype(np.float32)
        _MAPS[(w, h)] = (idepth, var, image)
    return _MAPS[(w, h)]


@pytest.mark.parametrize("size", [(48, 32), (176, 144)])
@pytest.mark.parametrize("pose", ["rot1", "rot2"])
@pytest.mark.parametrize("near", [1, 5, 9])
def test_restatement_equals_the_header_bit_for_bit(exe, tmp_path, size, pose, near):
    w, h = size
    idepth, var, image = planes(w, h)
    c2w = {"rot1": cr.POSE_ROT1, "rot2": cr.POSE_ROT2}[pose]
    K = K_OF(w, h)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([w, h, near], np.int32).tobytes())
        f.write(np.concatenate([K, c2w, [1.0, 1.0]]).astype(np.float32).tobytes())
        for p in (idepth, var, image):
            f.write(np.ascontiguousarray(p, np.float32).tobytes())
    out = subprocess.check_output([exe, str(tmp_path / "in.bin"), str(tmp_path / "out")]).decode()
    packed = cr.pack_ref(idepth, var, image)
    wire = (tmp_path / "out.msg").read_bytes()
    assert len(wire) == HEADER_BYTES + w * h * 12
    assert wire[HEADER_BYTES:] == packed.tobytes()
    got = np.fromfile(tmp_path / "out.pts", np.float32).reshape(-1, 4)
    ref, info = cr.flush_ref(packed, K, c2w, 1.0, 1.0, near)
    print(size, pose, near, {k: v for k, v in info.items() if k != "keep"})
    assert ("points %d" % len(ref)) in out and len(got) == len(ref) > 0
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    # the map exercises the branches the GPU tests lean on
    assert info["rej_scaled"] > 0 and (info["rej_abs"] > 0 or pose == "rot1") and (info["rej_support"] > 0 or near == 1)
