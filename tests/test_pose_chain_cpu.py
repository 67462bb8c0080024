"""The host pose chain of the loops (include/lsd_slam_hip_pose.hpp: Sim3 product, inverse, se3FromSim3, the relative pose of a frame seen
from a keyframe) against float64 numpy products of the 4 x 4 matrices [s R | t].  Both sides work in double, so they agree to 1e-12
relative.  The header is compiled into tests/cpp/pose_chain_test.cpp, a stand-alone program, with the address and undefined-behaviour
sanitizers on."""
import os
import subprocess

import numpy as np
import pytest

from common import ROOT

RTOL = 1e-12


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pose_chain") / "pose_chain_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "pose_chain_test.cpp"), "-o", out])
    return out


def run(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    out = r.stdout.splitlines()
    assert out[-1] == "pose chain ok"
    return [np.array(l.split(), np.float64) for l in out[:-1]]


def fmt(*vals):
    return " ".join("%.17g" % v for a in vals for v in np.atleast_1d(a))


def rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def mat(p):
    """8 doubles (unit quaternion w x y z, translation, scale) -> 4 x 4; 7 doubles: scale 1"""
    M = np.eye(4)
    M[:3, :3] = (p[7] if len(p) == 8 else 1.0) * rot(p[:4])
    M[:3, 3] = p[4:7]
    return M


def close(p, M, what):
    assert abs(np.linalg.norm(p[:4]) - 1) < 1e-14, what
    err = np.linalg.norm(mat(p) - M) / np.linalg.norm(M)
    assert err <= RTOL, (what, err)


def random_sim3(rng, scale=True):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return np.concatenate([q, rng.normal(size=3) * 2.0, [np.exp(rng.uniform(-0.7, 0.7)) if scale else 1.0]])


def small_motion(rng, scale):
    """a keyframe seen from its parent: a few degrees, a few centimetres, the depth rescale as scale"""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(0.01, 0.08)
    q = np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * axis])
    return np.concatenate([q, rng.normal(size=3) * 0.05, [scale]])


def test_identity(exe):
    I = np.array([1.0, 0, 0, 0, 0, 0, 0, 1])
    a = random_sim3(np.random.default_rng(1))
    out = run(exe, ["mul " + fmt(I, I), "inv " + fmt(I), "rel " + fmt(I, I), "chain 0", "mul " + fmt(I, a), "mul " + fmt(a, I), "rel " + fmt(a, a)])
    assert np.array_equal(out[0], I) and np.array_equal(out[1], I) and np.array_equal(out[2], I[:7])
    close(out[3], mat(a), "identity * a")
    close(out[4], mat(a), "a * identity")
    close(np.concatenate([out[5], [1.0]]), np.eye(4), "a seen from a")
    assert np.abs(out[5][4:7]).max() <= 1e-12 * max(1.0, np.abs(a[4:7]).max())


def test_products_and_inverses(exe):
    rng = np.random.default_rng(2)
    cases = [(random_sim3(rng), random_sim3(rng)) for _ in range(50)]
    out = run(exe, [l for a, b in cases for l in ("mul " + fmt(a, b), "inv " + fmt(a), "lift " + fmt(a[:7], b[7]))])
    for k, (a, b) in enumerate(cases):
        close(out[3 * k], mat(a) @ mat(b), "product %d" % k)
        assert abs(out[3 * k][7] - a[7] * b[7]) <= RTOL * a[7] * b[7]
        close(out[3 * k + 1], np.linalg.inv(mat(a)), "inverse %d" % k)
        assert np.array_equal(out[3 * k + 2], np.concatenate([a[:7], [b[7]]]))


def test_chain_of_six_keyframes_and_a_frame_on_a_reactivated_parent(exe):
    """camToWorld along six keyframes whose thisToParent carries the depth rescale (scales != 1); then keyframe 2 comes back while the
    loop stands on keyframe 5: the frame tracked on keyframe 5 seen from keyframe 2, and the frame tracked next on keyframe 2 in the world"""
    rng = np.random.default_rng(3)
    scales = [1.07, 0.93, 1.21, 0.88, 1.02, 0.97]
    steps = [small_motion(rng, s) for s in scales]
    world = run(exe, ["chain 6 " + fmt(*steps)])
    M = np.eye(4)
    Ms = []
    for k, s in enumerate(steps):
        M = M @ mat(s)
        Ms.append(M.copy())
        close(world[k], M, "camToWorld of keyframe %d" % (k + 1))
    assert abs(world[5][7] - np.prod(scales)) <= RTOL * np.prod(scales)
    # the candidate frame, tracked on keyframe 5 (index 4) with frameToKeyframe f2k: camToWorld = camToWorld(kf) * sim3(f2k, 1)
    f2k = small_motion(rng, 1.0)
    cand = run(exe, ["mul " + fmt(world[4], f2k)])[0]
    close(cand, Ms[4] @ mat(f2k), "candidate frame")
    est = run(exe, ["rel " + fmt(world[1], cand)])[0]
    R = np.linalg.inv(Ms[1]) @ Ms[4] @ mat(f2k)
    sc = np.cbrt(np.linalg.det(R[:3, :3]))
    E = np.eye(4)
    E[:3, :3] = R[:3, :3] / sc                      # se3FromSim3 keeps rotation and translation and drops the scale
    E[:3, 3] = R[:3, 3]
    close(np.concatenate([est, [1.0]]), E, "the frame seen from the re-activated keyframe")
    # a frame tracked on the re-activated keyframe 2 stands in the world where that keyframe's chain puts it
    f2k2 = small_motion(rng, 1.0)
    w2 = run(exe, ["mul " + fmt(world[1], f2k2)])[0]
    close(w2, Ms[1] @ mat(f2k2), "frame on the re-activated keyframe")
    assert abs(w2[7] - scales[0] * scales[1]) <= RTOL
