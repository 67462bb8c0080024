"""The re-position search without a GPU.

1. The host part of lsdhip_tracker_find_reposition_candidate (lsd_slam_amd/csrc/reposition_plan.hpp: prefilter, skips, scores, the
   selection replayed with the reference's `bestScore = score` quirk, an empty bank, a bank that is all far) as a stand-alone g++ program
   against hand-worked values, built with -fsanitize=address,undefined and run as its own process.
2. The census of scenario A (tests/reposition_ref.py) on the oracle — and on oracle/_ref where it is built, with identical decisions:
   the scenario reaches every branch of TrackableKeyFrameSearch::findRePositionCandidate (C/GlobalMapping/TrackableKeyFrameSearch.cpp:
   103-172), and every quantity that decides a branch stays clear of its threshold (dist2 1 % of distanceTH, score 0.01, goodVal 0.05,
   poseDiscrepancy 0.02, newScore 0.01 from the running best), so that the GPU test may demand the same decisions from a path that agrees
   with the oracle only to the permaref tolerances (usage rel 1e-5, poses 2e-3).  These are conditions on the inputs.
"""
import os
import subprocess

import pytest

import reposition_ref as rr
from common import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("reposition") / "reposition_plan_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "reposition_plan_test.cpp"), "-o", out])
    return out


def test_reposition_plan(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert r.stdout.splitlines()[-1] == "reposition plan ok"


def run_scenario(oracle, L=None):
    K, kfs, frame, pose = rr.scenario_a_oracle(oracle, L)
    tracker = oracle.SE3Tracker(rr.W, rr.H, K, mode=oracle.SSE_EXACT_RCP, L=L)
    return rr.search(oracle, tracker, kfs, frame, pose, kfs[rr.PARENT_SLOT]["id"], rr.W, rr.H, K)


@pytest.fixture(scope="module")
def scenario(oracle):
    return run_scenario(oracle)


def test_scenario_a_reaches_every_branch_with_margins(scenario):
    best, recs, counts = scenario
    for r in recs:
        print({k: (round(float(v), 5) if k not in ("stage", "slot", "id", "trackingWasGood", "diverged") else v) for k, v in r.items()
               if k not in ("refToFrame", "tracked")})
    reached, bad = rr.census(recs, counts)
    assert not bad, bad
    assert reached == rr.ALL_BRANCHES, rr.ALL_BRANCHES - reached
    assert best == rr.EXPECTED_WINNER
    assert [r["stage"] for r in recs] == rr.EXPECTED_STAGES
    # the drifted slot is rejected by its discrepancy alone
    d = recs[rr.DRIFT_SLOT]
    assert d["stage"] == "rejected" and d["poseDiscrepancy"] > 0.2 and d["trackingWasGood"] and d["goodVal"] > 0.7 and d["newScore"] < d["bestScoreBefore"]
    # slot 14 loses only to the stored bestScore = score of slot 13; under bestScore = newScore it would have won
    assert recs[14]["newScore"] > recs[13]["score"] and recs[14]["newScore"] < recs[13]["newScore"] + 1 and recs[14]["poseDiscrepancy"] < 0.2


def test_scenario_a_on_the_reference(oracle, scenario):
    if not oracle.have_ref() and not oracle.build_ref():
        pytest.skip("oracle/_ref needs the reference sources, which this machine does not have")
    best, recs, counts = run_scenario(oracle, oracle.lib(ref="sse"))
    reached, bad = rr.census(recs, counts)
    assert not bad, bad
    assert best == scenario[0] and [r["stage"] for r in recs] == [r["stage"] for r in scenario[1]]
    assert {k: counts[k] for k in ("potential", "checked", "tracked")} == {k: scenario[2][k] for k in ("potential", "checked", "tracked")}
