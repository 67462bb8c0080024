"""How a tracking job is run (lsd_slam_amd/csrc/track_plan.hpp: level tilings, the shape of a batch, trials, caps and grids of single jobs
and batches, the launch budget — pure functions over plain integers) checked by a stand-alone program built with plain g++ — no HIP
headers, no library — against values worked out by hand: the 640x480 and 1280x1024 single jobs level by level (launch grid 400), one trial
everywhere after set_speculation(1, 0), a permaref job of 3000 points, batch shapes of 1 / 8 / 64 jobs, the strips of 160x128 and 640x480
levels, the trials 1, 3, 4, 4 of an 8-job batch, and the four-entry launch history.  No GPU."""
import os
import subprocess

import pytest

from common import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("trackplan") / "track_plan_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "track_plan_test.cpp"), "-o", out])
    return out


def test_track_plan(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert r.stdout.splitlines()[-1] == "track plan ok"
