"""Tracking where one degree of freedom gets no constraint, against the oracle.

A fronto-parallel plane at constant depth carries a texture that varies along one world axis only, and the camera moves only in ways
that keep it so: texture f(Y) with moves in ty, tz and pitch renders frames whose rows are constant (gx = 0 inside every level, so the
tx column of the Jacobian is zero), and its transpose f(X) with moves in tx, tz and yaw renders constant columns (gy = 0).  The LM
system then has an exactly zero row and column; the reference's A.ldlt().solve(b) leaves that unknown at 0, and so must the device
solves (gj6_solve_wave for SE3, gj7_solve_wave for Sim3).  Every tracking path is held to test_trackframe_parity's rule against the
oracle: pose within 10x the oracle's own SSE-vs-scalar spread (floor 5e-4), finite pose and residual, same diverged and
trackingWasGood."""
import numpy as np
import pytest

from common import ODOMETRY_ITS, pose_distance

pytestmark = pytest.mark.gpu

IDENT7 = np.array([1, 0, 0, 0, 0, 0, 0], np.float64)
Z0 = 2.0


@pytest.fixture(scope="module")
def hip():
    import lsd_slam_amd as la
    return la


def texture(s):
    """sum of sines of one world coordinate, grey values 20 ... 235 (about the same per-pixel gradients at every image size: the
    coordinate comes scaled by w / 320)"""
    v = 0.45 * np.sin(2.1 * s + 0.3) + 0.3 * np.sin(5.3 * s + 1.1) + 0.25 * np.sin(11.7 * s - 0.4)
    return 127.5 + 107.5 * v


def rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    if axis == "x":
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def render(w, h, K, R, t, along):
    """camera-to-world (R, t) looking at the plane Z = Z0: uint8 image and the camera-frame depth of every pixel"""
    fx, fy, cx, cy = [float(v) for v in K]
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    dw = d @ R.T
    s = (Z0 - t[2]) / dw[..., 2]
    P = t + s[..., None] * dw
    img = np.clip(np.rint(texture((P[..., 1] if along == "Y" else P[..., 0]) * (w / 320.0))), 0, 255).astype(np.uint8)
    return img, s.astype(np.float32)


def scene(w, h, along, n=4):
    """frames 0..n-1 and their depths; frame i moved by (ty or tx) = 0.006 i, tz = 0.01 i, pitch or yaw = 0.004 i"""
    from lsd_slam_amd import synth
    K = synth.intrinsics(w, h)
    frames, depths, poses = [], [], []
    for i in range(n):
        if along == "Y":
            R, t = rot("x", 0.004 * i), np.array([0.0, 0.006 * i, 0.01 * i])
        else:
            R, t = rot("y", 0.004 * i), np.array([0.006 * i, 0.0, 0.01 * i])
        img, dep = render(w, h, K, R, t, along)
        frames.append(img)
        depths.append(dep)
        poses.append(np.concatenate([synth.rot_to_quat(R), t]))
    return frames, depths, K, poses


SIZES = [(320, 240), (640, 480)]
ALONG = [pytest.param("Y", id="rows-constant-gx0"), pytest.param("X", id="columns-constant-gy0")]


def test_scene_is_degenerate():
    frames, _, _, _ = scene(320, 240, "Y")
    assert all(np.all(f == f[:, :1]) for f in frames)
    frames, _, _, _ = scene(320, 240, "X")
    assert all(np.all(f == f[:1, :]) for f in frames)


def oracle_track(oracle, w, h, K, ro, img, i, init):
    out = []
    for mode in (oracle.SSE, oracle.SCALAR):
        tr = oracle.SE3Tracker(w, h, K, mode=mode)
        tr.set_max_its(ODOMETRY_ITS)
        out.append(tr.track(ro, oracle.Frame(i, img, K), init))
    return out


def check_like_oracle(oracle, est, lastResidual, diverged, good, r_sse, r_sc, what):
    assert np.all(np.isfinite(est)) and np.isfinite(lastResidual), (what, est, lastResidual)
    assert not r_sse.diverged, (what, "the scene must stay trackable for the reference")
    p_sse, p_sc = np.array(r_sse.frameToRef), np.array(r_sc.frameToRef)
    spread = max(max(pose_distance(p_sse, p_sc, oracle)), 1e-5)
    dt, dr = pose_distance(est, p_sse, oracle)
    assert max(dt, dr) <= max(10 * spread, 5e-4), (what, dt, dr, spread)
    assert bool(diverged) == bool(r_sse.diverged) and bool(good) == bool(r_sse.trackingWasGood), (what, diverged, good)


def setup(oracle, hip, w, h, along):
    frames, depths, K, _ = scene(w, h, along)
    ctx = hip.Context(w, h, K)
    kfo = oracle.Frame(0, frames[0], K)
    kfo.set_depth_gt(depths[0])
    ro = oracle.TrackingReference()
    ro.import_frame(kfo)
    kfg = hip.Frame(ctx, 0, frames[0])
    kfg.setDepthFromGroundTruth(depths[0])
    rg = hip.TrackingReference()
    rg.importFrame(kfg)
    return frames, depths, K, ctx, kfo, ro, kfg, rg


@pytest.mark.parametrize("host_lm", [False, True], ids=["device-lm", "host-lm"])
@pytest.mark.parametrize("along", ALONG)
@pytest.mark.parametrize("w,h", SIZES)
def test_trackframe_on_a_degenerate_scene(oracle, hip, w, h, along, host_lm, monkeypatch):
    if host_lm:
        monkeypatch.setenv("LSDHIP_HOST_LM", "1")      # read in lsdhip_tracker_create
    frames, depths, K, ctx, kfo, ro, kfg, rg = setup(oracle, hip, w, h, along)
    trg = hip.SE3Tracker(ctx)
    trg.set_maxItsPerLvl(ODOMETRY_ITS)
    for i in range(1, len(frames)):
        r_sse, r_sc = oracle_track(oracle, w, h, K, ro, frames[i], i, IDENT7)
        est = trg.trackFrame(rg, hip.Frame(ctx, i, frames[i]), IDENT7)
        check_like_oracle(oracle, est, trg.lastResidual, trg.diverged, trg.trackingWasGood, r_sse, r_sc, (along, i))


@pytest.mark.parametrize("coarse_min_jobs", [None, 1], ids=["default", "coarse-min-jobs-1"])
@pytest.mark.parametrize("along", ALONG)
@pytest.mark.parametrize("w,h", SIZES)
def test_trackframe_batch_on_a_degenerate_scene(oracle, hip, w, h, along, coarse_min_jobs):
    """9 jobs (the strips of the throughput mode; with set_batch_coarse_min_jobs(1) the coarse levels run in k_track_solo)"""
    frames, depths, K, ctx, kfo, ro, kfg, rg = setup(oracle, hip, w, h, along)
    trg = hip.SE3Tracker(ctx)
    trg.set_maxItsPerLvl(ODOMETRY_ITS)
    if coarse_min_jobs is not None:
        trg.set_batch_coarse_min_jobs(coarse_min_jobs)
    idx = [1 + j % (len(frames) - 1) for j in range(9)]
    want = {i: oracle_track(oracle, w, h, K, ro, frames[i], i, IDENT7) for i in set(idx)}
    fgs = [hip.Frame(ctx, 100 + j, frames[i]) for j, i in enumerate(idx)]
    poses, recs = trg.trackFrameBatch([rg] * len(idx), fgs, np.tile(IDENT7, (len(idx), 1)))
    for j, i in enumerate(idx):
        r = recs[j]
        check_like_oracle(oracle, poses[j], r.lastResidual, r.diverged, r.trackingWasGood, *want[i], (along, j, i))


@pytest.mark.parametrize("along", ALONG)
@pytest.mark.parametrize("w,h", SIZES)
def test_permaref_on_a_degenerate_scene(oracle, hip, w, h, along):
    frames, depths, K, ctx, kfo, ro, kfg, rg = setup(oracle, hip, w, h, along)
    pos, cv, _, _ = ro.pointcloud(4)
    T0 = IDENT7
    trg = hip.SE3Tracker(ctx)
    for i in range(1, len(frames)):
        r_sse = oracle.SE3Tracker(w, h, K, mode=oracle.SSE).track_permaref(pos, cv, oracle.Frame(i, frames[i], K), T0)
        r_sc = oracle.SE3Tracker(w, h, K, mode=oracle.SCALAR).track_permaref(pos, cv, oracle.Frame(i, frames[i], K), T0)
        est = trg.trackFrameOnPermaref(pos, cv, hip.Frame(ctx, i, frames[i]), T0)
        check_like_oracle(oracle, est, trg.lastResidual, trg.diverged, trg.trackingWasGood, r_sse, r_sc, (along, i))


@pytest.mark.parametrize("along", ALONG)
@pytest.mark.parametrize("w,h", SIZES)
def test_sim3_on_a_degenerate_scene(oracle, hip, w, h, along):
    """the 7x7 system has the same zero row and column: guards gj7_solve_wave's zero-pivot handling"""
    frames, depths, K, ctx, kfo, ro, kfg, rg = setup(oracle, hip, w, h, along)
    init = np.concatenate([IDENT7, [1.0]])
    for i in range(1, len(frames)):
        fo = oracle.Frame(i, frames[i], K)
        fo.set_depth_gt(depths[i])
        fg = hip.Frame(ctx, i, frames[i])
        fg.setDepthFromGroundTruth(depths[i])
        r_sse = oracle.Sim3Tracker(w, h, K, mode=oracle.SSE).track(ro, fo, init, 3, 1)
        r_sc = oracle.Sim3Tracker(w, h, K, mode=oracle.SCALAR).track(ro, fo, init, 3, 1)
        tg = hip.Sim3Tracker(ctx)
        got, rg3 = tg.trackFrameSim3(kfg, fg, init, 3, 1)
        assert np.all(np.isfinite(got)) and np.isfinite(rg3.lastResidual), (along, i, got)
        assert bool(tg.diverged) == bool(r_sse.diverged), (along, i, tg.diverged, r_sse.diverged)
        assert not r_sse.diverged
        p_sse, p_sc = np.array(r_sse.frameToRef), np.array(r_sc.frameToRef)
        spread = max(float(np.abs(p_sse - p_sc).max()), 1e-5)
        assert float(np.abs(got - p_sse).max()) <= max(10 * spread, 5e-4), (along, i, got, p_sse, spread)
