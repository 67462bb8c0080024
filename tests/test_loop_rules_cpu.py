"""The per-frame rules of the loops (include/lsd_slam_hip_loop.hpp) against a table written here from the reference's own statements:
the tracking-loss test (SlamSystem.cpp:946-966), what becomes of the keyframe at a loss (:809-817), the frames the mapper drops
(:559-566), the keyframe selection by score (:997-1015) and the score itself (TrackableKeyFrameSearch.h:75-79).  Decisions are
compared exactly, scores and thresholds as float32 bit patterns against numpy float32 arithmetic done in the reference's order.  The
header is compiled into tests/cpp/loop_rules_test.cpp, a stand-alone program, with the address and undefined-behaviour sanitizers on."""
import os
import subprocess

import numpy as np
import pytest

from common import ROOT

f32 = np.float32
INITIALIZATION_PHASE_COUNT = 5      # util/settings.h:172
MIN_NUM_MAPPED = 5                  # util/settings.h:174
KFDistWeight, KFUsageWeight = f32(4), f32(3)   # util/settings.cpp:77-78


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("loop_rules") / "loop_rules_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "loop_rules_test.cpp"), "-o", out])
    return out


def run(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    out = r.stdout.splitlines()
    assert out[-1] == "loop rules ok" and len(out) == len(lines) + 1, out
    return out[:-1]


def bits(x):
    return "%08x" % int(np.array([x], np.float32).view(np.uint32)[0])


# ---- the reference's rules, restated independently ----------------------------------------------------------------------------------
def ref_lost(diverged, good, nkf):
    """SlamSystem.cpp:948 (manualTrackingLossIndicated aside)"""
    return bool(diverged or (nkf > INITIALIZATION_PHASE_COUNT and not good))


def ref_score(dist2, usage):
    """TrackableKeyFrameSearch.h:77-78, in single precision, left to right"""
    dist2, usage = f32(dist2), f32(usage)
    return f32(f32(f32(dist2 * KFDistWeight) * KFDistWeight) + f32(f32(f32((f32(1) - usage) * (f32(1) - usage)) * KFUsageWeight) * KFUsageWeight))


def ref_threshold(size):
    """SlamSystem.cpp:1001-1003: float minVal = fmin(0.2f + size * 0.8f / 5, 1.0f); below 5 keyframes `minVal *= 0.7` — a float times a
    double constant, the product taken in double and rounded back"""
    v = min(f32(f32(0.2) + f32(f32(f32(size) * f32(0.8)) / f32(INITIALIZATION_PHASE_COUNT))), f32(1.0))
    if size < INITIALIZATION_PHASE_COUNT:
        v = f32(np.float64(v) * 0.7)
    return f32(v)


def test_constants(exe):
    assert run(exe, ["constants"]) == ["5 5 4 3 5 20 50 100 0"]      # settings.h:172,174, settings.cpp:77-78, SlamSystem.cpp:80-81


def test_tracking_loss_on_both_sides_of_the_initialisation_phase(exe):
    cases = [(d, g, n) for n in (0, 4, 5, 6, 7, 100) for d in (0, 1) for g in (0, 1)]
    out = run(exe, ["lost %d %d %d" % c for c in cases])
    assert [int(o) for o in out] == [int(ref_lost(*c)) for c in cases]
    # the rule's edge: exactly 5 finished keyframes is still the initialisation phase, 6 is not
    assert run(exe, ["lost 0 0 5", "lost 0 0 6", "lost 1 1 0"]) == ["0", "1", "1"]


def test_keyframe_at_a_loss_and_mapping_steps(exe):
    out = run(exe, ["finalise %d" % m for m in (0, 4, 5, 6)])
    assert out == [str(int(m >= MIN_NUM_MAPPED)) for m in (0, 4, 5, 6)] == ["0", "0", "1", "1"]       # SlamSystem.cpp:809
    # lost beats everything; a frame tracked on a replaced keyframe is dropped whatever the keyframe policy says (:559-566)
    want = {(1, 0, 0): "lost", (1, 1, 1): "lost", (1, 0, 1): "lost", (1, 1, 0): "lost", (0, 0, 0): "dropped", (0, 0, 1): "dropped",
            (0, 1, 0): "update", (0, 1, 1): "change"}
    keys = sorted(want)
    assert run(exe, ["step %d %d %d" % k for k in keys]) == [want[k] for k in keys]


def test_fixed_interval(exe):
    cases = [(10, 8), (10, 9), (10, 10), (10, 11), (1, 0), (1, 1), (3, 2), (3, 3), (0, 0), (0, 50), (-1, 50)]
    out = run(exe, ["every %d %d" % c for c in cases])
    assert [int(o) for o in out] == [int(k > 0 and s >= k) for k, s in cases]
    assert out[1:3] == ["0", "1"]                          # sinceKF == kfEvery - 1, sinceKF == kfEvery


def test_score_bits(exe):
    rng = np.random.default_rng(7)
    cases = [(0.0, 1.0), (0.0, 0.0), (1.0, 1.0), (0.01, 0.5), (1e-4, 0.93)] + [(float(d), float(u)) for d, u in zip(rng.uniform(0, 0.2, 40), rng.uniform(0, 1, 40))]
    out = run(exe, ["score %s %s" % (bits(d), bits(u)) for d, u in cases])
    assert out == [bits(ref_score(d, u)) for d, u in cases]
    assert out[0] == bits(0.0) and out[1] == bits(9.0) and out[2] == bits(16.0)


def test_threshold_bits(exe):
    sizes = [0, 1, 4, 5, 6, 100]
    out = run(exe, ["threshold %d" % s for s in sizes] + ["threshold -"])
    assert out[:-1] == [bits(ref_threshold(s)) for s in sizes]
    # x 0.7 below five keyframes, none from five on, the clamp to 1 reached at five
    assert out[2] == bits(f32(np.float64(f32(f32(0.2) + f32(f32(f32(4) * f32(0.8)) / f32(5)))) * 0.7))
    assert out[3] == bits(1.0) and out[4] == bits(1.0) and out[5] == bits(1.0)
    # a loop that keeps no keyframes: keyframesAll stays empty; the loops take that product in single precision
    assert out[-1] == bits(f32(0.2) * f32(0.7))
    assert abs(float(f32(0.2) * f32(0.7)) - float(ref_threshold(0))) <= 2 ** -26      # one float32 rounding apart at the most


def test_score_rule_gate_and_edge(exe):
    lines, want = [], []
    for th in (ref_threshold(0), ref_threshold(4), ref_threshold(5), f32(0.2) * f32(0.7)):
        under, over = np.nextafter(f32(th), f32(0)), np.nextafter(f32(th), f32(2))
        for mapped in (0, 5, 6, 7):
            for sc in (under, th, over):
                lines.append("wants %d %s %s" % (mapped, bits(sc), bits(th)))
                want.append(int(mapped > MIN_NUM_MAPPED and f32(sc) > f32(th)))       # SlamSystem.cpp:998, :1007
    assert [int(o) for o in run(exe, lines)] == want
    assert want[:12] == [0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1]         # mapped 5: never; mapped 6: only the score just over
