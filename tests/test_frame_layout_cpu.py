"""The arena layout of a frame (lsd_slam_amd/csrc/frame_layout.hpp: every plane named once, with its size and the lsdhip_frame member it
backs) checked by a stand-alone program built with plain g++ — no HIP headers, no library: 46 planes, 256-byte aligned, ascending in the
documented order without overlap, each at least as large as its consumer needs, and the arena totals of 16x16, 176x144, 640x480 and
656x496 as literals.  No GPU."""
import os
import subprocess

import pytest

from common import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("framelayout") / "frame_layout_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "frame_layout_test.cpp"), "-o", out])
    return out


def test_frame_arena_layout(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.splitlines()
    assert lines[-1] == "frame layout ok"
    assert lines[:4] == ["16x16: 46 planes, 27392 bytes", "176x144: 46 planes, 1751552 bytes", "640x480: 46 planes, 21161984 bytes",
                         "656x496: 46 planes, 22415616 bytes"]
