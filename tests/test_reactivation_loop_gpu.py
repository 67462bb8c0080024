"""lsd_slam_hip::SlamLoop with enableReactivation (the C++ loop behind lsdloop_*: findRePositionCandidate before every keyframe change,
DepthMap::reactivateKeyframe — the fused three-launch change — where it finds a banked keyframe) on the scenario of
tests/reactivation_loop.py:
  * against the same schedule driven from Python over the single calls (finalizeKeyFrame + setFromExistingKF / createKeyFrame): poses
    equal with ==, the same change log, the final map bit for bit — one-stream and pipelined;
  * the HIP schedule against the oracle run of tests/test_reactivation_loop_cpu.py: the same decisions, trajectory and final map
    under the bounds of tests/test_sequence_gpu.py;
  * with re-activation off the loop is the loop it was;
  * dataset_slam --reactivate."""
import os
import subprocess

import numpy as np
import pytest

import reactivation_loop as rl
import seq_loops as sl
from common import ROOT, assert_bit_equal

pytestmark = pytest.mark.gpu

HYP_FIELDS = ("isValid", "blacklisted", "nextStereoFrameMinID", "validity_counter", "idepth", "idepth_var", "idepth_smoothed", "idepth_var_smoothed")


def python_schedule(lag, fused=False):
    import lsd_slam_amd as la
    frames, depth0, K, gt = rl.scenario_inputs()
    ctx = la.Context(rl.W, rl.H, K)
    if lag:
        ctx.set_pipeline(True)
    ctx.set_async(True)              # as lsdloop_create sets it: mapping calls only queue their work
    return rl.run_loop(rl.HipSide(la, ctx, frames, depth0, rl.BANK_CAPACITY, fused=fused), rl.N_FRAMES, lag=lag)


_SCHEDULE = {}


def schedule(lag):
    if lag not in _SCHEDULE:
        _SCHEDULE[lag] = python_schedule(lag)
    return _SCHEDULE[lag]


def cpp_loop(pipelined, reactivate, n, kf_every=rl.KF_EVERY):
    import torch
    from lsd_slam_amd.driver import DriverLoop
    frames, depth0, K, gt = rl.scenario_inputs()
    dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    torch.cuda.synchronize()
    drv = DriverLoop(rl.W, rl.H, K, dev[0].data_ptr(), depth0, kf_every=kf_every, images_on_device=True)
    try:
        if pipelined:
            drv.set_pipeline(True)
        if reactivate:
            drv.enable_reactivation(rl.BANK_CAPACITY)
        done, poses = drv.run([dev[i].data_ptr() for i in range(1, n + 1)], want_poses=True)
        assert done == n
        changes = [tuple(int(v) for v in row) for row in drv.keyframe_changes()]
        return np.asarray(poses).copy(), changes, drv.download_map(), drv.reactivation_counts(), int(drv.stats().dropped)
    finally:
        drv.close()


@pytest.mark.parametrize("pipelined", [False, True], ids=["one-stream", "pipelined"])
def test_cpp_loop_with_reactivation_equals_the_python_schedule(pipelined):
    poses, changes, final, (nreact, unbanked), dropped = cpp_loop(pipelined, True, rl.N_FRAMES)
    g = schedule(1 if pipelined else 0)
    print(changes)
    assert changes == g.changes
    assert nreact == sum(c[3] for c in changes) >= 1 and unbanked == 0
    assert dropped == len(g.dropped)
    for i, (a, b) in enumerate(zip(poses, g.frameToKF)):
        assert np.array_equal(a, b), ("frame %d" % (i + 1), a, b)
    for k in HYP_FIELDS:
        assert_bit_equal(final[k], g.final_map[k], "final map: %s" % k)


def test_python_schedule_over_the_fused_calls_equals_the_split_form():
    """DepthMap.reactivateKeyframe / changeKeyframeBatch in the place of the two calls each, same schedule: same poses, same map"""
    a, b = schedule(0), python_schedule(0, fused=True)
    assert a.changes == b.changes
    for i, (x, y) in enumerate(zip(a.frameToKF, b.frameToKF)):
        assert np.array_equal(x, y), i + 1
    for k in ("isValid", "blacklisted", "validity_counter"):
        assert np.array_equal(a.final_map[k], b.final_map[k]), k
    v = a.final_map["isValid"] > 0
    for k in ("idepth", "idepth_var", "idepth_smoothed", "idepth_var_smoothed"):
        assert_bit_equal(a.final_map[k][v], b.final_map[k][v], "final map: %s" % k)


@pytest.mark.parametrize("lag", [0, 1], ids=["one-stream", "pipelined"])
def test_hip_schedule_against_the_oracle(oracle, lag):
    """the decisions of the oracle run (tests/test_reactivation_loop_cpu.py), and trajectory / final map within the bounds
    tests/test_sequence_gpu.py::_compare applies to the HIP-against-oracle comparison of a sequence: 10 x the oracle's own scalar-against-SSE
    spread (floors 1e-4 trajectory, 2e-3 mask), 5e-4 per pose, 3 x its spread on the inverse depths (floors 1e-4 median, 5e-3 p99)"""
    frames, depth0, K, gt = rl.scenario_inputs()
    g = schedule(lag)
    run_o = lambda mode: rl.run_loop(rl.OracleSide(oracle, frames, depth0, K, rl.BANK_CAPACITY, mode=mode), rl.N_FRAMES, lag=lag)
    o_sse, o_sc = run_o(oracle.SSE), run_o(oracle.SCALAR)
    assert o_sse.changes == rl.EXPECTED_CHANGES
    assert g.changes == o_sse.changes
    assert g.dropped == o_sse.dropped and g.refinished == o_sse.refinished
    assert g.diverged == o_sse.diverged and not any(g.diverged) and g.good == o_sse.good
    spread = sl.rmse(o_sse.trajectory(), o_sc.trajectory())
    err = sl.rmse(g.trajectory(), o_sse.trajectory())
    err_gt_g, err_gt_o = sl.rmse(g.trajectory(), gt[1:]), sl.rmse(o_sse.trajectory(), gt[1:])
    print("trajectory RMSE: HIP vs oracle-SSE %.3e, oracle scalar vs SSE %.3e, vs GT: HIP %.3e oracle %.3e" % (err, spread, err_gt_g, err_gt_o))
    assert err <= max(10.0 * spread, 1e-4), (err, spread)
    assert err_gt_g <= 1.5 * err_gt_o + 1e-4, (err_gt_g, err_gt_o)
    for i, (a, b) in enumerate(zip(g.frameToKF, o_sse.frameToKF)):
        assert np.linalg.norm(a[4:7] - b[4:7]) < 5e-4 and min(np.linalg.norm(a[:4] - b[:4]), np.linalg.norm(a[:4] + b[:4])) < 5e-4, i
    ham = float((g.final_valid != o_sse.final_valid).mean())
    ham_ref = float((o_sc.final_valid != o_sse.final_valid).mean())
    print("final map: %d valid (oracle %d), mask Hamming %.2e (oracle scalar vs SSE %.2e)" % (g.final_semidense, o_sse.final_semidense, ham, ham_ref))
    assert ham <= max(10 * ham_ref, 2e-3)
    both = g.final_valid & o_sse.final_valid
    d = np.abs(g.final_map["idepth"][both] - o_sse.final_map["idepth"][both])
    both_ref = o_sc.final_valid & o_sse.final_valid
    d_ref = np.abs(o_sc.final_map["idepth"][both_ref] - o_sse.final_map["idepth"][both_ref])
    print("final idepth |diff|: median %.2e p99 %.2e (oracle scalar vs SSE: %.2e, %.2e)" % (np.median(d), np.percentile(d, 99), np.median(d_ref), np.percentile(d_ref, 99)))
    assert np.median(d) <= max(3 * np.median(d_ref), 1e-4)
    assert np.percentile(d, 99) <= max(3 * np.percentile(d_ref, 99), 5e-3)


def test_loop_without_reactivation_is_unchanged():
    """12 frames with re-activation off against seq_loops.run_hip — the schedule over the single calls that this change does not touch"""
    import lsd_slam_amd as la
    n = 12
    poses, changes, final, counts, dropped = cpp_loop(False, False, n)
    assert changes == [] and counts == (0, 0) and dropped == 0
    frames, depth0, K, gt = rl.scenario_inputs()
    ctx = la.Context(rl.W, rl.H, K)
    g = sl.run_hip(la, ctx, frames, depth0, n, kf_every=rl.KF_EVERY, clear_flag=True)
    assert g.kf_frames == [3, 6, 9, 12]
    for i, (a, b) in enumerate(zip(poses, g.frameToKF)):
        assert np.array_equal(a, b), ("frame %d" % (i + 1), a, b)


def test_dataset_slam_reports_its_reactivations(tmp_path):
    """dataset_slam --reactivate 32 on the scenario's frames as PGM files (random depth initialisation, so its own decisions): one line
    per re-activation, each naming an earlier keyframe, and totals that count those lines; without the option the output is as before"""
    frames, depth0, K, gt = rl.scenario_inputs()
    lst = []
    for i in range(rl.N_FRAMES + 1):
        p = tmp_path / ("f%04d.pgm" % i)
        with open(p, "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (rl.W, rl.H))
            f.write(frames[i].tobytes())
        lst.append(str(p))
    (tmp_path / "files.txt").write_text("\n".join(lst) + "\n")
    (tmp_path / "calib.cfg").write_text("%f %f %f %f 0\n%d %d\nnone\n%d %d\n" % (K[0], K[1], K[2], K[3], rl.W, rl.H, rl.W, rl.H))
    exe = os.path.join(ROOT, "lsd_slam_amd", "dataset_slam")
    outs = {}
    for name, extra in (("on", ["--reactivate", "32"]), ("off", [])):
        d = tmp_path / name
        d.mkdir()
        outs[name] = subprocess.check_output([exe, str(tmp_path / "calib.cfg"), str(tmp_path / "files.txt"), str(d), "--kf-every", str(rl.KF_EVERY)] + extra,
                                             timeout=120).decode().splitlines()
    assert len(outs["off"]) == 1 and "reactivations" not in outs["off"][0]
    lines, totals = outs["on"][:-1], outs["on"][-1].split()
    s = dict(zip(totals[0::2], map(int, totals[1::2])))
    assert s["frames"] == rl.N_FRAMES and s["unbanked"] == 0
    print(outs["on"])
    assert s["reactivations"] == len(lines) >= 1
    # the depth starts from random values here (srand(0): the same in every run), and the run still makes the scenario's decisions
    assert [tuple(int(l.split()[k]) for k in (2, 4, 6)) for l in lines] == [c[:3] for c in rl.EXPECTED_CHANGES if c[3]]
    for l in lines:
        t = l.split()
        assert t[0] == "reactivated" and t[1] == "frame" and t[3] == "keyframe" and t[5] == "->"
        frame, prev, new = int(t[2]), int(t[4]), int(t[6])
        assert frame % rl.KF_EVERY == 0 and new < frame and new != prev and new % rl.KF_EVERY == 0
        assert int(t[t.index("tracked") + 1]) >= 1
    traj = np.loadtxt(tmp_path / "on" / "trajectory.txt")
    assert traj.shape == (rl.N_FRAMES, 20) and np.allclose(np.linalg.norm(traj[:, 2:6], axis=1), 1.0, atol=1e-6)
    assert np.allclose(np.linalg.norm(traj[:, 9:13], axis=1), 1.0, atol=1e-5)
