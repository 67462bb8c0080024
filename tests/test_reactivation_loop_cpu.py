"""The loop with re-activation of banked keyframes (tests/reactivation_loop.py::run_loop), on the ORACLE alone: the scenario the GPU tests
run (test_reactivation_loop_gpu.py) does what it is there for — a banked keyframe comes back, keyframes are still created once the
bank is past the initialisation phase, a keyframe is finalised a second time — every search of the run decides clear of its thresholds,
the map a re-activation leaves is setFromExistingKF's, and the trajectory stays on the scene's ground truth."""
import numpy as np
import pytest

import reactivation_loop as rl
import reposition_ref as rr
import seq_loops as sl


@pytest.fixture(scope="module")
def runs(oracle):
    frames, depth0, K, gt = rl.scenario_inputs()
    out = {}
    for lag in (0, 1):
        side = rl.OracleSide(oracle, frames, depth0, K, rl.BANK_CAPACITY)
        out[lag] = (rl.run_loop(side, rl.N_FRAMES, lag=lag, keep_maps=True), side)
    return out


@pytest.mark.parametrize("lag", [0, 1])
def test_scenario_reactivates_creates_and_refinishes(runs, lag):
    rec, side = runs[lag]
    print(rec.changes)
    assert not any(rec.diverged) and all(rec.good) and len(rec.frameToKF) == rl.N_FRAMES
    assert sum(c[3] for c in rec.changes) >= 1                                                       # a re-activation
    assert any(not c[3] and size > 5 for c, size in zip(rec.changes, rec.bank_size_at_change))       # a keyframe created past the initialisation phase
    assert len(rec.refinished) >= 1                                                                  # a bank slot replaced
    assert rec.changes == rl.EXPECTED_CHANGES
    assert rec.refinished == rl.EXPECTED_REFINISHED and rec.unbanked == 0
    assert rec.dropped == (rl.EXPECTED_DROPPED_LAG1 if lag else [])
    # a re-activated keyframe is past the initialisation phase and was finished before (TrackableKeyFrameSearch.cpp:118-122)
    ids = [e["id"] for e in side.bank]
    for c in rec.changes:
        if c[3]:
            assert ids.index(c[2]) >= rr.INITIALIZATION_PHASE_COUNT and c[2] != c[1] and c[2] < c[0]


@pytest.mark.parametrize("lag", [0, 1])
def test_every_search_decides_clear_of_its_thresholds(runs, lag):
    rec, side = runs[lag]
    assert len(side.searches) == len(rec.changes)
    for k, (recs, counts) in enumerate(side.searches):
        reached, bad = rr.census(recs, counts)
        assert not bad, (k, bad)
        assert (counts["potential"], counts["checked"], counts["tracked"]) == rec.changes[k][4:]


def test_reactivated_map_is_set_from_existing(oracle, runs):
    """the map right after a re-activation against DepthMap::setFromExistingKF of the same keyframe on a fresh oracle map"""
    rec, side = runs[0]
    assert rec.reactivated_maps
    frames, depth0, K, gt = rl.scenario_inputs()
    # the run's last re-activation: that keyframe was not finalised again, so it still holds the planes the map was made from
    assert rec.changes[-1][3] == 1
    for got, kf in rec.reactivated_maps[-1:]:
        dm = oracle.DepthMap(rl.W, rl.H, K)
        dm.set_from_existing(kf)
        want = dm.get()
        v = want["isValid"] > 0
        assert np.array_equal(got["isValid"] > 0, v) and v.sum() > 10000
        for k in ("idepth", "idepth_var", "idepth_smoothed", "idepth_var_smoothed", "validity_counter"):
            assert np.array_equal(got[k][v], want[k][v]), k
        assert np.array_equal(got["blacklisted"], want["blacklisted"])


@pytest.mark.parametrize("lag", [0, 1])
def test_trajectory_stays_on_the_ground_truth(runs, lag):
    rec, side = runs[lag]
    frames, depth0, K, gt = rl.scenario_inputs()
    step = np.linalg.norm(np.diff(gt, axis=0), axis=1).mean()
    err = sl.rmse(rec.trajectory(), gt[1:])
    print("trajectory RMSE against the ground truth %.3e, inter-frame motion %.3e" % (err, step))
    assert err < 0.5 * step


def test_pose_chain_of_the_helper_is_the_float64_product():
    """the helper's pose functions (the header's expressions in Python) against 4 x 4 products"""
    rng = np.random.default_rng(0)

    def mat(p):
        M = np.eye(4)
        M[:3, :3] = p[7] * sl.quat_to_rot(p[:4])
        M[:3, 3] = p[4:7]
        return M
    for _ in range(20):
        a, b = (np.concatenate([q / np.linalg.norm(q), rng.normal(size=3), [np.exp(rng.uniform(-0.5, 0.5))]]) for q in rng.normal(size=(2, 4)))
        assert np.allclose(mat(rl.pose_mul(a, b)), mat(a) @ mat(b), rtol=0, atol=1e-12)
        assert np.allclose(mat(rl.pose_inv(a)), np.linalg.inv(mat(a)), rtol=0, atol=1e-12)
