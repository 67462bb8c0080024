"""The owner of device resources (lsd_slam_amd/csrc/owned.hpp) with fake release functions that count their calls: one release per
value whatever path it took (destructor, move, move-assignment over a live value, self-move, a vector's reallocation), none after
release(), and a creator in the library's pattern (unique_ptr + owner members) failed at each of its steps gives back exactly what it
had acquired.  The header is compiled into tests/cpp/owned_test.cpp, a stand-alone program, with the address and undefined-behaviour
sanitizers on."""
import os
import subprocess

import pytest

from common import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("owned") / "owned_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-self-move", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "owned_test.cpp"), "-o", out])
    return out


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.splitlines() == ["ok"], r.stdout


@pytest.mark.parametrize("case", ["destructor", "move", "move_assign_over_live", "self_move", "release", "vector"])
def test_owner(exe, case):
    """every case ends with a live count of zero and no value released twice (checked by the program itself)"""
    run(exe, case)


@pytest.mark.parametrize("steps", [1, 2, 5, 8])
def test_creator_failed_at_every_step(exe, steps):
    run(exe, "creator", steps)
