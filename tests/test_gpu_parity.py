"""GPU parity tests proper: every hot-path stage of liblsdhip.so (called through the C ABI) against the CPU oracle on
the same seeded inputs.  Bar: bit-exact for masks / integer state / per-pixel float results whose operation order
is replicated; float32 reductions within 1e-5 of a float64 accumulation of the oracle's per-point float32 terms;
function-level poses within the oracle's own scalar-vs-SSE spread."""
import os

import numpy as np
import pytest

from common import ODOMETRY_ITS, assert_bit_equal, assert_reference_blocks_list, pose_distance, sequence
from se3_terms import oracle_terms64 as _oracle_terms64

pytestmark = pytest.mark.gpu

IDENT7 = np.array([1.0, 0, 0, 0, 0, 0, 0])


@pytest.fixture(scope="module")
def hip():
    import lsd_slam_amd as la
    return la


def make_pair(oracle, hip, w, h, n, seq_index=0, params=None, kind="S1"):
    frames, depth0, K, gt = sequence(w, h, n, seq_index, kind)
    ctx = hip.Context(w, h, K, params=params)
    return frames, depth0, K, gt, ctx


def oracle_params(oracle, params=None):
    """the oracle's parameter block with the same overrides the HIP context got"""
    op = oracle.default_params()
    for k, v in (params or {}).items():
        setattr(op, k, v)
    return op


# The reference's run-time switches on this path (C/util/settings.cpp:84-88).  The ROS front end pushes
# useAffineLightningEstimation = False (cfg/LSDParams.cfg:27 via IOWrapper/ROS/rosReconfigure.h:84): that is the
# configuration live_slam actually runs, so every function-level test covers both values.
AFFINE = [pytest.param({}, id="affine1"), pytest.param({"useAffineLightningEstimation": 0}, id="affine0")]
STEREO = [pytest.param({}, id="neg1-subpix1"),
          pytest.param({"allowNegativeIdepths": 0}, id="neg0"),
          pytest.param({"useSubpixelStereo": 0}, id="subpix0"),
          pytest.param({"allowNegativeIdepths": 0, "useSubpixelStereo": 0, "useAffineLightningEstimation": 0}, id="ros-all0")]


# ---------------------------------------------------------------------------------------------------------------
# K-pyr
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(160, 128), (176, 144), (640, 480)])   # 176 = 5.5 tiles of 32: partial tiles, odd level-4 width
def test_pyramids_bit_exact(oracle, hip, w, h):
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, w, h, 2)
    fo = oracle.Frame(0, frames[1], K)
    fg = hip.Frame(ctx, 0, frames[1])
    for lvl in range(5):
        assert np.array_equal(ctx.intrinsics(lvl), fo.intrinsics(lvl)), "intrinsics level %d" % lvl
        assert_bit_equal(fg.image(lvl), fo.plane("image", lvl), "image L%d" % lvl)
        assert_bit_equal(fg.gradients(lvl), fo.plane("gradients", lvl), "gradients L%d" % lvl)
    assert_bit_equal(fg.maxGradients(0), fo.plane("maxGradients", 0), "maxGradients")
    # K-pyr-id + setDepthFromGroundTruth
    fo.set_depth_gt(depth0)
    fg.setDepthFromGroundTruth(depth0)
    for lvl in range(5):
        assert_bit_equal(fg.idepth(lvl), fo.plane("idepth", lvl), "idepth L%d" % lvl)
        assert_bit_equal(fg.idepthVar(lvl), fo.plane("idepthVar", lvl), "idepthVar L%d" % lvl)


def test_idepth_pyramid_ragged_validity(oracle, hip):
    """inverse-variance pooling with random holes, negative idepths and tiny variances"""
    w, h = 160, 128
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, w, h, 1)
    rng = np.random.default_rng(7)
    idp = rng.uniform(-0.2, 2.0, (h, w)).astype(np.float32)
    var = rng.uniform(1e-6, 0.25, (h, w)).astype(np.float32)
    hole = rng.uniform(size=(h, w)) < 0.6
    idp[hole] = -1
    var[hole] = -1
    idp[10:20, 10:20] = -1
    var[10:20, 10:20] = -1      # fully empty 2x2 blocks
    fo = oracle.Frame(0, frames[0], K)
    fg = hip.Frame(ctx, 0, frames[0])
    fo.set_depth_planes(idp, var)
    fg.setDepthPlanes(idp, var)
    for lvl in range(5):
        assert_bit_equal(fg.idepth(lvl), fo.plane("idepth", lvl), "idepth L%d" % lvl)
        assert_bit_equal(fg.idepthVar(lvl), fo.plane("idepthVar", lvl), "idepthVar L%d" % lvl)


@pytest.mark.parametrize("w,h", [(160, 128), (640, 480), (656, 496)])
def test_reference_blocks_list_the_oracles_reference_pixels(oracle, hip, w, h):
    """The blocks the throughput-mode strips read (k_ref_blocks, written behind every idepth pyramid): per 256 consecutive pixels exactly
    the pixels the oracle's makePointCloud test takes — inside the one-pixel border, idepthVar > 0, idepth != 0 (TrackingReference.cpp:120-131)
    — in pixel order; sizes with a ragged last block and an odd coarse width (656 / 16 = 41) included."""
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, w, h, 1)
    rng = np.random.default_rng(11)
    idp = rng.uniform(-0.2, 2.0, (h, w)).astype(np.float32)
    var = rng.uniform(1e-6, 0.25, (h, w)).astype(np.float32)
    hole = rng.uniform(size=(h, w)) < 0.55
    idp[hole] = -1
    var[hole] = -1
    idp[rng.uniform(size=(h, w)) < 0.02] = 0.0     # idepth == 0 with a positive variance: not a reference point
    fo = oracle.Frame(0, frames[0], K)
    fg = hip.Frame(ctx, 0, frames[0])
    fo.set_depth_planes(idp, var)
    fg.setDepthPlanes(idp, var)
    for lvl in range(1, 5):
        idl, varl = fo.plane("idepth", lvl), fo.plane("idepthVar", lvl)
        assert idl.shape == (h >> lvl, w >> lvl)
        offs, cnts = fg.referenceBlocks(lvl)
        assert_reference_blocks_list(offs, cnts, idl, varl, lvl)


@pytest.mark.parametrize("w,h", [(160, 128), (640, 480), (656, 496)])
def test_gradient_candidates_are_the_pixels_observe_can_search(oracle, hip, w, h):
    """The lists the batched update's select pass walks (k_grad_candidates, built with a keyframe's level-0 planes): per 1024 consecutive
    pixels exactly the pixels inside the 3-pixel border whose maxGradients is not below minUseGrad (DepthMap.cpp:111-131), in pixel order;
    also after the test hook has overwritten the plane."""
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, w, h, 1)
    fg = hip.Frame(ctx, 0, frames[0])
    th = 5.0     # lsdhip_default_params: minUseGrad

    def check():
        return assert_gradient_candidates(fg, w, h, th)

    n1 = check()
    assert 0 < n1 < w * h
    rng = np.random.default_rng(3)
    fg.setMaxGradients(rng.uniform(0, 12, (h, w)).astype(np.float32))
    n2 = check()
    assert n2 != n1


def assert_gradient_candidates(fg, w, h, th):
    """Frame.gradientCandidates() of `fg` against the numpy statement at threshold `th`; returns the number of candidates"""
    mg = fg.maxGradients(0)
    ok = ~(mg < np.float32(th))
    ok[:3, :] = False; ok[-3:, :] = False; ok[:, :3] = False; ok[:, -3:] = False
    flat = ok.reshape(-1)
    offs, cnts = fg.gradientCandidates()
    ng = (w * h + 1023) // 1024
    assert offs.shape == (ng, 1024) and cnts.shape == (ng,)
    for g in range(ng):
        want = np.flatnonzero(flat[g * 1024:(g + 1) * 1024])
        assert cnts[g] == len(want), "group %d: count" % g
        assert np.array_equal(offs[g, :len(want)], want.astype(np.uint16)), "group %d: offsets" % g
    return int(flat.sum())


def test_pointcloud_order_and_bits(oracle, hip):
    w, h = 320, 240
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, w, h, 1)
    fo = oracle.Frame(0, frames[0], K)
    fg = hip.Frame(ctx, 0, frames[0])
    fo.set_depth_gt(depth0)
    fg.setDepthFromGroundTruth(depth0)
    ro = oracle.TrackingReference()
    ro.import_frame(fo)
    rg = hip.TrackingReference()
    rg.importFrame(fg)
    for lvl in (4, 3, 2, 1, 0):
        po, cvo, gro, io = ro.pointcloud(lvl)
        pg, cvg, grg, ig = rg.makePointCloud(lvl)
        assert len(po) == len(pg) and len(po) > 0
        assert np.array_equal(io, ig)
        assert_bit_equal(pg, po, "posData L%d" % lvl)
        assert_bit_equal(cvg, cvo, "colorAndVarData L%d" % lvl)
        assert_bit_equal(grg, gro, "gradData L%d" % lvl)


# ---------------------------------------------------------------------------------------------------------------
# residual kernel (K1+K2+K3) at fixed poses
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", AFFINE)
@pytest.mark.parametrize("w,h", [(176, 144), (320, 240), (640, 480)])
def test_residual_kernel_fixed_pose(oracle, hip, w, h, params):
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, w, h, 4, params=params)
    op = oracle_params(oracle, params)
    kfo = oracle.Frame(0, frames[0], K)
    kfg = hip.Frame(ctx, 0, frames[0])
    kfo.set_depth_gt(depth0)
    kfg.setDepthFromGroundTruth(depth0)
    ro = oracle.TrackingReference()
    ro.import_frame(kfo)
    rg = hip.TrackingReference()
    rg.importFrame(kfg)
    tro = oracle.SE3Tracker(w, h, K, params=op, mode=oracle.SSE_EXACT_RCP)
    trg = hip.SE3Tracker(ctx)
    poses = [IDENT7.astype(np.float32),
             oracle.se3_inv(gt[3]).astype(np.float32),
             oracle.se3_exp(np.array([0.05, -0.03, 0.02, 0.01, -0.02, 0.03])).astype(np.float32),
             oracle.se3_exp(np.array([0.9, 0.1, 0.0, 0.0, 0.35, 0.0])).astype(np.float32)]  # most points leave the image
    for pi, T in enumerate(poses):
        for lvl in (4, 3, 2, 1):
            fo = oracle.Frame(3, frames[3], K)
            fg = hip.Frame(ctx, 3, frames[3])
            a, b = (1.0, 0.0) if pi % 2 == 0 else (1.03, -2.5)
            r_o = tro.evaluate(ro, fo, T, lvl, a, b)
            r_g = trg.evaluate(rg, fg, T, lvl, a, b)
            tag = "pose %d level %d" % (pi, lvl)
            # integer / mask outputs: exact
            assert r_g.warped_size == r_o.warped_size, tag
            assert r_g.goodCount == r_o.goodCount and r_g.badCount == r_o.badCount, tag
            if lvl == 1:
                assert_bit_equal(fg.refPixelWasGoodNoCreate(), fo.wasgood(), "refPixelWasGood " + tag)
            else:
                assert fg.refPixelWasGoodNoCreate() is None and fo.wasgood() is None
            if r_o.warped_size < 8:
                continue
            assert r_g.num_constraints == r_o.num_constraints, tag
            # reductions of K1
            assert r_g.pointUsage == pytest.approx(r_o.pointUsage, rel=2e-5), tag
            assert r_g.retval == pytest.approx(r_o.retval, rel=1e-4), tag
            assert r_g.meanRes == pytest.approx(r_o.meanRes, rel=1e-3, abs=1e-4), tag
            # the affine-lighting statistic is a difference of O(1e4 N) float32 sums (syy - sy^2/sw): ill-conditioned in
            # the reference itself; b additionally multiplies the error of a by the mean intensity (~128)
            assert r_g.affine_a_lastIt == pytest.approx(r_o.affine_a_lastIt, rel=5e-4), tag
            assert r_g.affine_b_lastIt == pytest.approx(r_o.affine_b_lastIt, abs=0.08), tag
            # K2 / K3 against a float64 accumulation of the oracle's per-point float32 terms
            A64, Aabs, b64, babs, err64, n4 = _oracle_terms64(oracle, tro)
            nc = r_o.num_constraints
            Ag = np.array(r_g.A).reshape(6, 6).astype(np.float64) * nc
            bg = np.array(r_g.b).astype(np.float64) * nc
            assert np.all(np.abs(Ag - A64) <= 1e-5 * Aabs + 1e-12), tag
            assert np.all(np.abs(bg - b64) <= 1e-5 * babs + 1e-12), tag
            assert r_g.lsError * nc == pytest.approx(err64, rel=1e-5), tag
            assert r_g.weightedError == pytest.approx(r_o.weightedError, rel=2e-5), tag
            # and within float32-summation noise of the oracle's own float32 sums
            assert np.allclose(np.array(r_g.A), np.array(r_o.A), rtol=2e-4, atol=1e-4 * np.abs(np.array(r_o.A)).max()), tag


def _affine_truth64(tro, fo, lvl):
    """(a, b) of the affine-lighting estimate (SE3Tracker.cpp:956-961, :1016-1024) from the per-point terms of the oracle's LAST
    evaluation, accumulated in float64: c2 = frame intensity at the warped position (bilinear), c1 = c2 + residual, Huber(5) weights."""
    x, y, z, r = [tro.buffer(k).astype(np.float64) for k in ("x", "y", "z", "residual")]
    fx, fy, cx, cy = [float(v) for v in fo.intrinsics(lvl)[:4]]
    img = fo.plane("image", lvl).astype(np.float64)
    u, v = x / z * fx + cx, y / z * fy + cy
    ix, iy = u.astype(np.int64), v.astype(np.int64)
    dx, dy = u - ix, v - iy
    c2 = dx * dy * img[iy + 1, ix + 1] + (dy - dx * dy) * img[iy + 1, ix] + (dx - dx * dy) * img[iy, ix + 1] + (1 - dx - dy + dx * dy) * img[iy, ix]
    c1 = c2 + r
    wgt = np.where(np.abs(r) < 5.0, 1.0, 5.0 / np.maximum(np.abs(r), 1e-30))
    sxx, syy, sx, sy, sw = (c1 * c1 * wgt).sum(), (c2 * c2 * wgt).sum(), (c1 * wgt).sum(), (c2 * wgt).sum(), wgt.sum()
    a = np.sqrt((syy - sy * sy / sw) / (sxx - sx * sx / sw))
    return a, (sy - a * sx) / sw


@pytest.mark.parametrize("w,h", [(320, 240), (640, 480)])
def test_affine_lighting_estimate_against_float64_truth(oracle, hip, w, h):
    """The affine-lighting estimate is a difference of float32 sums of ~1e4 products of magnitude 1e4: the reference adds them one by
    one, the device as a tree.  Evidence instead of prose (profiles/r04_notes.md section 4c): (a, b) accumulated in float64 from the
    oracle's own per-point terms is the truth both are measured against — the device must be within max(10 x the reference's own distance,
    a small floor) of it — and the weighted residual of a second evaluation at each side's own (a, b) (what lastResidual is made of)
    within max(10 x the reference's distance, 2e-3) of the one at the true (a, b).  The reference's distances are printed."""
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, w, h, 4, params={})
    kfo = oracle.Frame(0, frames[0], K)
    kfg = hip.Frame(ctx, 0, frames[0])
    kfo.set_depth_gt(depth0)
    kfg.setDepthFromGroundTruth(depth0)
    ro = oracle.TrackingReference()
    ro.import_frame(kfo)
    rg = hip.TrackingReference()
    rg.importFrame(kfg)
    tro = oracle.SE3Tracker(w, h, K, mode=oracle.SSE_EXACT_RCP)
    trg = hip.SE3Tracker(ctx)
    poses = [IDENT7.astype(np.float32), oracle.se3_inv(gt[3]).astype(np.float32),
             oracle.se3_exp(np.array([0.05, -0.03, 0.02, 0.01, -0.02, 0.03])).astype(np.float32)]
    worst = {"a_ref": 0.0, "a_hip": 0.0, "b_ref": 0.0, "b_hip": 0.0, "res_ref": 0.0, "res_hip": 0.0}
    for pi, T in enumerate(poses):
        for lvl in (2, 1):
            for a0, b0 in ((1.0, 0.0), (1.03, -2.5)):
                tag = "pose %d level %d (a, b) = (%g, %g)" % (pi, lvl, a0, b0)
                fo = oracle.Frame(3, frames[3], K)
                fg = hip.Frame(ctx, 3, frames[3])
                r_o = tro.evaluate(ro, fo, T, lvl, a0, b0)
                a64, b64 = _affine_truth64(tro, fo, lvl)
                r_g = trg.evaluate(rg, fg, T, lvl, a0, b0)
                da_o, da_g = abs(r_o.affine_a_lastIt - a64) / a64, abs(r_g.affine_a_lastIt - a64) / a64
                db_o, db_g = abs(r_o.affine_b_lastIt - b64), abs(r_g.affine_b_lastIt - b64)
                assert da_g <= max(10 * da_o, 2e-5), (tag, da_g, da_o)
                assert db_g <= max(10 * db_o, 5e-3), (tag, db_g, db_o)
                # the next evaluation's weighted residual at each side's own estimate against the one at the true estimate
                e_t = tro.evaluate(ro, fo, T, lvl, np.float32(a64), np.float32(b64)).weightedError
                e_o = tro.evaluate(ro, fo, T, lvl, r_o.affine_a_lastIt, r_o.affine_b_lastIt).weightedError
                e_g = trg.evaluate(rg, fg, T, lvl, r_g.affine_a_lastIt, r_g.affine_b_lastIt).weightedError
                de_o, de_g = abs(e_o - e_t) / e_t, abs(e_g - e_t) / e_t
                assert de_g <= max(10 * de_o, 2e-3), (tag, de_g, de_o)
                for k, val in (("a_ref", da_o), ("a_hip", da_g), ("b_ref", db_o), ("b_hip", db_g), ("res_ref", de_o), ("res_hip", de_g)):
                    worst[k] = max(worst[k], val)
    print("affine lighting vs float64 truth, worst case: a relative — reference %.2e, device %.2e; b absolute — reference %.2e, device %.2e; "
          "weighted residual of the next evaluation relative — reference %.2e, device %.2e"
          % (worst["a_ref"], worst["a_hip"], worst["b_ref"], worst["b_hip"], worst["res_ref"], worst["res_hip"]))


@pytest.mark.parametrize("params", AFFINE)
@pytest.mark.parametrize("w,h", [(176, 144), (640, 480)])
def test_trackframe_parity(oracle, hip, w, h, params):
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, w, h, 6, params=params)
    op = oracle_params(oracle, params)
    kfo = oracle.Frame(0, frames[0], K)
    kfg = hip.Frame(ctx, 0, frames[0])
    kfo.set_depth_gt(depth0, minUseGrad=op.minUseGrad)
    kfg.setDepthFromGroundTruth(depth0)
    ro = oracle.TrackingReference()
    ro.import_frame(kfo)
    rg = hip.TrackingReference()
    rg.importFrame(kfg)
    trg = hip.SE3Tracker(ctx)
    trg.set_maxItsPerLvl(ODOMETRY_ITS)
    tr_sse = oracle.SE3Tracker(w, h, K, params=op, mode=oracle.SSE)
    tr_sc = oracle.SE3Tracker(w, h, K, params=op, mode=oracle.SCALAR)
    tr_sse.set_max_its(ODOMETRY_ITS)
    tr_sc.set_max_its(ODOMETRY_ITS)
    init = IDENT7.copy()
    for i in range(1, 6):
        fo = oracle.Frame(i, frames[i], K)
        fo2 = oracle.Frame(i, frames[i], K)
        fg = hip.Frame(ctx, i, frames[i])
        r_sse = tr_sse.track(ro, fo, init)
        r_sc = tr_sc.track(ro, fo2, init)
        est = trg.trackFrame(rg, fg, init)
        p_sse, p_sc = np.array(r_sse.frameToRef), np.array(r_sc.frameToRef)
        spread = max(max(pose_distance(p_sse, p_sc, oracle)), 1e-5)
        dt, dr = pose_distance(est, p_sse, oracle)
        # within 10x the reference's own scalar-vs-SSE spread on this input (and an absolute 5e-4 floor)
        assert max(dt, dr) <= max(10 * spread, 5e-4), (i, dt, dr, spread)
        assert trg.diverged == bool(r_sse.diverged) and trg.trackingWasGood == bool(r_sse.trackingWasGood)
        # lastResidual / initialTrackedResidual: within 10x the reference's own scalar-vs-SSE spread on this input, floor 2e-3 —
        # 2e-2 with affine lighting on: the estimate (a, b) is a difference of float32 sums of ~1e4 products of magnitude 1e4
        # (SE3Tracker.cpp:1016-1024); both oracle paths add them in the same sequential order, the device adds them as a tree, and a
        # shift of b by 0.07 grey levels (measured) moves a residual of 0.3 grey levels RMS by a percent
        affine_on = params.get("useAffineLightningEstimation", 1) != 0
        res_floor = 2e-2 if affine_on else 2e-3
        res_spread = abs(r_sc.lastResidual - r_sse.lastResidual) / abs(r_sse.lastResidual)
        res_diff = abs(trg.lastResidual - r_sse.lastResidual) / abs(r_sse.lastResidual)
        sens = 0.0
        if affine_on:
            # where the 2e-2 comes from, measured instead of argued: at the reference's final pose, the distance of ITS estimate of b from the
            # float64 accumulation of its own per-point terms, times the residual's sensitivity to b (d/db of sum w r^2 over sum w r^2)
            Tf = oracle.se3_inv(np.array(r_sse.frameToRef)).astype(np.float32)
            fe = oracle.Frame(100 + i, frames[i], K)
            ev = tr_sse.evaluate(ro, fe, Tf, 1, r_sse.affine_a, r_sse.affine_b)
            a64, b64 = _affine_truth64(tr_sse, fe, 1)
            rbuf, wbuf = tr_sse.buffer("residual").astype(np.float64), tr_sse.buffer("weight_p").astype(np.float64)
            sens = 2.0 * abs(ev.affine_b_lastIt - b64) * float((wbuf * np.abs(rbuf)).sum() / (wbuf * rbuf * rbuf).sum())
        print("frame %d lastResidual: HIP vs oracle-SSE %.2e, oracle scalar vs SSE %.2e (bound %.2e); the reference's own b error moves its residual by up to %.2e"
              % (i, res_diff, res_spread, max(10 * res_spread, res_floor), sens))
        assert res_diff <= max(10 * res_spread, res_floor), (i, trg.lastResidual, r_sse.lastResidual, r_sc.lastResidual)
        assert trg.pointUsage == pytest.approx(r_sse.pointUsage, rel=1e-3)
        if params.get("useAffineLightningEstimation", 1) == 0:
            # the estimate is never applied (C/Tracking/SE3Tracker.cpp:331-335,393-397): (a, b) stay (1, 0)
            assert trg.affineEstimation_a == 1.0 and trg.affineEstimation_b == 0.0
            assert r_sse.affine_a == 1.0 and r_sse.affine_b == 0.0
        else:
            # same number of evaluations = same accept / reject history: tight; otherwise (the oracle's SSE mode runs the host's own
            # _mm_rcp_ps, so a borderline accept can fall the other way on another CPU) the estimate of a neighbouring iteration
            same_history = trg.last.numEvaluations == r_sse.numEvaluations
            assert trg.affineEstimation_a == pytest.approx(r_sse.affine_a, rel=2e-3 if same_history else 1e-2)
        # frame side effects
        so, sg = fo.stats(), fg.stats()
        assert sg["initialTrackedResidual"] == pytest.approx(so["initialTrackedResidual"], rel=max(10 * res_spread, res_floor) + 1e-3)
        mg, mo = fg.refPixelWasGoodNoCreate(), fo.wasgood()
        assert mg is not None and mo is not None
        assert (mg != mo).mean() < 2e-3   # masks are those of the last evaluated pose; poses differ by ~1e-5
        init = est
    assert kfg.stats()["numFramesTrackedOnThis"] == 5
    assert kfo.stats()["numFramesTrackedOnThis"] == 10   # two oracle trackers (SSE + scalar) share the keyframe


def test_trackframe_divergence_returns_identity(oracle, hip):
    w, h = 320, 240
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, w, h, 2)
    kfo = oracle.Frame(0, frames[0], K)
    kfg = hip.Frame(ctx, 0, frames[0])
    kfo.set_depth_gt(depth0)
    kfg.setDepthFromGroundTruth(depth0)
    ro = oracle.TrackingReference()
    ro.import_frame(kfo)
    rg = hip.TrackingReference()
    rg.importFrame(kfg)
    bad = oracle.se3_exp(np.array([5.0, 0, 0, 0, 0, 0]))   # keyframe entirely out of view
    tro = oracle.SE3Tracker(w, h, K)
    trg = hip.SE3Tracker(ctx)
    r = tro.track(ro, oracle.Frame(1, frames[1], K), bad)
    est = trg.trackFrame(rg, hip.Frame(ctx, 1, frames[1]), bad)
    assert r.diverged and trg.diverged and not trg.trackingWasGood
    assert np.array_equal(est, IDENT7)


def test_permaref_paths(oracle, hip):
    run_permaref_paths(oracle, hip, 640, 480)


def run_permaref_paths(oracle, hip, w, h, params=None):
    """params: overrides of the context's settings, handed to the oracle as well (tests/test_settings_gpu.py)"""
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, w, h, 4, params=params)
    op = oracle_params(oracle, params)
    kfo = oracle.Frame(0, frames[0], K)
    kfo.set_depth_gt(depth0, minUseGrad=op.minUseGrad)
    ro = oracle.TrackingReference()
    ro.import_frame(kfo)
    pos, cv, _, _ = ro.pointcloud(4)
    tro = oracle.SE3Tracker(w, h, K, params=op, mode=oracle.SSE_EXACT_RCP)
    trg = hip.SE3Tracker(ctx)
    fo = oracle.Frame(3, frames[3], K)
    fg = hip.Frame(ctx, 3, frames[3])
    T0 = oracle.se3_exp(np.array([0.01, 0.0, 0.0, 0, 0, 0.002]))
    r = tro.track_permaref(pos, cv, fo, T0)
    est = trg.trackFrameOnPermaref(pos, cv, fg, T0)
    dt, dr = pose_distance(est, np.array(r.frameToRef), oracle)
    assert max(dt, dr) < 2e-3, (dt, dr)
    assert trg.trackingWasGood == bool(r.trackingWasGood)
    u_o = tro.check_overlap(pos, kfo, T0)
    u_g = trg.checkPermaRefOverlap(pos, T0)
    assert u_g == pytest.approx(u_o, rel=1e-5)
    return r


# ---------------------------------------------------------------------------------------------------------------
# depth map stages
# ---------------------------------------------------------------------------------------------------------------
def _noisy_hyp(hyp, sigma=0.1, seed=1):
    """the ragged state of _noisy_map, applied to a downloaded map (host arithmetic only: the batch tests build the oracle's side alone first)"""
    rng = np.random.default_rng(seed)
    v = hyp["isValid"] > 0
    noise = rng.normal(0, sigma, hyp.shape).astype(np.float32)
    for k in ("idepth", "idepth_smoothed"):
        hyp[k][v] += noise[v]
    for k in ("idepth_var", "idepth_var_smoothed"):
        hyp[k][v] = sigma ** 2
    # ragged state: holes, blacklisted pixels, varied validity, scheduled skips
    holes = rng.uniform(size=hyp.shape) < 0.15
    hyp["isValid"][holes] = 0
    hyp["blacklisted"][rng.uniform(size=hyp.shape) < 0.03] = -2
    hyp["blacklisted"][rng.uniform(size=hyp.shape) < 0.03] = -1
    hyp["validity_counter"] = rng.integers(0, 60, hyp.shape).astype(np.int32)
    hyp["nextStereoFrameMinID"][rng.uniform(size=hyp.shape) < 0.2] = 4.0
    return hyp


def _noisy_map(oracle, hip, ctx, frames, depth0, K, w, h, sigma=0.1, seed=1, op=None, threads=None):
    kfo = oracle.Frame(0, frames[0], K)
    kfg = hip.Frame(ctx, 0, frames[0])
    kfo.set_depth_gt(depth0, minUseGrad=ctx.params.minUseGrad)     # (the oracle's frames carry no settings: the threshold is an argument)
    kfg.setDepthFromGroundTruth(depth0)
    dmo = oracle.DepthMap(w, h, K, params=op) if threads is None else oracle.DepthMap(w, h, K, params=op, threads=threads)
    dmg = hip.DepthMap(ctx)
    dmo.init_gt(kfo)
    dmg.initializeFromGTDepth(kfg)
    assert_hyp_equal(dmg.currentDepthMap(), dmo.get(), "initializeFromGTDepth")
    hyp = _noisy_hyp(dmo.get(), sigma, seed)
    dmo.set(kfo, hyp)
    dmg.setCurrentDepthMap(kfg, hyp)
    return kfo, kfg, dmo, dmg


def assert_hyp_equal(g, o, what, float_exact=True, rtol=0.0):
    assert_bit_equal(g["isValid"], o["isValid"], what + ": isValid")
    assert_bit_equal(g["blacklisted"], o["blacklisted"], what + ": blacklisted")
    v = o["isValid"] > 0
    assert_bit_equal(g["validity_counter"][v], o["validity_counter"][v], what + ": validity_counter")
    for k in ("nextStereoFrameMinID", "idepth", "idepth_var", "idepth_smoothed", "idepth_var_smoothed"):
        if float_exact:
            assert_bit_equal(g[k][v], o[k][v], what + ": " + k)
        else:
            assert np.allclose(g[k][v], o[k][v], rtol=rtol, atol=0), what + ": " + k


def _ref_pose(oracle, gt, i, base=None):
    """(Sim3 frame i -> keyframe, initialTrackedResidual): the ground-truth pose (relative to frame `base` when the keyframe is not frame
    0) composed with a small general twist — a pure in-plane translation + roll (the synthetic trajectory) leaves t_z = 0 and zero rotation
    off-diagonals, which would hide operation-order mismatches"""
    twist = np.array([0.0, 0.0, 0.003, 0.0008, -0.0006, 0.0004]) * (1 + 0.1 * i)
    rel = gt[i] if base is None else oracle.se3_mul(oracle.se3_inv(gt[base]), gt[i])
    return np.concatenate([oracle.se3_mul(rel, oracle.se3_exp(twist)), [1.0]]), float(0.3 + 0.1 * i)


def _ref_frames(oracle, hip, ctx, frames, K, gt, kfo, kfg, ids, with_masks=True, seed=5):
    rng = np.random.default_rng(seed)
    fos, fgs = [], []
    for i in ids:
        fo = oracle.Frame(i, frames[i], K)
        fg = hip.Frame(ctx, i, frames[i])
        sim3, itr = _ref_pose(oracle, gt, i)
        fo.set_pose(sim3, kfo, itr)
        fg.setPose(sim3, kfg, itr)
        if with_masks:
            m = (rng.uniform(size=(fo.h >> 1, fo.w >> 1)) < 0.9).astype(np.uint8)
            fo.set_wasgood(m)
            fg.set_refPixelWasGood(m)
        fos.append(fo)
        fgs.append(fg)
    return fos, fgs


@pytest.mark.parametrize("params", STEREO)
@pytest.mark.parametrize("w,h", [(176, 144), (320, 240), (640, 480)])
def test_depth_stages_bit_exact(oracle, hip, w, h, params):
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, w, h, 8, params=params)
    kfo, kfg, dmo, dmg = _noisy_map(oracle, hip, ctx, frames, depth0, K, w, h, op=oracle_params(oracle, params))
    kfo.set_counters(7, 3, 3, 0)
    kfg.setCounters(7, 3, 3, 0)
    fos, fgs = _ref_frames(oracle, hip, ctx, frames, K, gt, kfo, kfg, [3, 4, 6, 7])
    # K4 with a multi-frame deque (oldest = 3, newest = 7, id 5 missing -> referenceFrameByID duplicates)
    dmo.stage("observe", fos)
    dmg.stage("observe", fgs)
    assert_hyp_equal(dmg.currentDepthMap(), dmo.get(), "observeDepth")
    # K5
    dmo.stage("fillholes")
    dmg.stage("fillholes")
    assert_hyp_equal(dmg.currentDepthMap(), dmo.get(), "fillHoles")
    # K6 both variants
    dmo.stage("regularize")
    dmg.stage("regularize")
    assert_hyp_equal(dmg.currentDepthMap(), dmo.get(), "regularize<false>")
    dmo.stage("regularize_occ")
    dmg.stage("regularize_occ")
    assert_hyp_equal(dmg.currentDepthMap(), dmo.get(), "regularize<true>")
    # second observe pass: the update branch now sees smoothed values written by K6
    dmo.stage("observe", fos[1:])
    dmg.stage("observe", fgs[1:])
    assert_hyp_equal(dmg.currentDepthMap(), dmo.get(), "observeDepth (2nd)")


def test_single_map_regulariser_passes_on_32x16_tiles_1024x512(oracle, hip):
    """1024x512 = 32 x 64 = 2048 workgroups of 32x8 pixels: the smallest single map whose regulariser launches take the 32x16 tile
    (lsd_reg_py: PY = 2 from 2048 workgroups on).  regularizeDepthMap(false) and (true) as launches of their own
    (k_reg_fused<PassRegOnly, 2>, <PassRegOcc, 2>), then two updateKeyframe calls: the first finds the keyframe due for Frame::setDepth
    (k_reg_fused<PassUpdateSetDepth, 2>), the second does not (k_reg_fused<PassUpdate, 2>)."""
    w, h = 1024, 512
    assert ((w + 31) // 32) * ((h + 7) // 8) == 2048
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, w, h, 3)
    kfo, kfg, dmo, dmg = _noisy_map(oracle, hip, ctx, frames, depth0, K, w, h, op=oracle_params(oracle))
    dmo.stage("regularize")
    dmg.stage("regularize")
    assert_hyp_equal(dmg.currentDepthMap(), dmo.get(), "regularize<false>, PY = 2")
    dmo.stage("regularize_occ")
    dmg.stage("regularize_occ")
    assert_hyp_equal(dmg.currentDepthMap(), dmo.get(), "regularize<true>, PY = 2")
    kfo.set_counters(7, 3, 3, 0)
    kfg.setCounters(7, 3, 3, 0)
    fos, fgs = _ref_frames(oracle, hip, ctx, frames, K, gt, kfo, kfg, [1, 2])
    for i, what in enumerate(("updateKeyframe with Frame::setDepth, PY = 2", "updateKeyframe, PY = 2")):
        assert kfg.stats()["depthHasBeenUpdatedFlag"] == i
        dmo.update([fos[i]])
        dmg.updateKeyframe([fgs[i]])
        assert_hyp_equal(dmg.currentDepthMap(), dmo.get(), what)
        for lvl in range(5):
            assert_bit_equal(kfg.idepth(lvl), kfo.plane("idepth", lvl), what + " keyframe idepth L%d" % lvl)


def test_observe_reactivated_and_no_masks(oracle, hip):
    w, h = 320, 240
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, w, h, 8)
    kfo, kfg, dmo, dmg = _noisy_map(oracle, hip, ctx, frames, depth0, K, w, h, seed=3)
    hyp = dmo.get()
    dmo.set(kfo, hyp, reactivated=True)
    dmg.setCurrentDepthMap(kfg, hyp, reactivated=True)
    fos, fgs = _ref_frames(oracle, hip, ctx, frames, K, gt, kfo, kfg, [2, 5], with_masks=False)
    dmo.stage("observe", fos)
    dmg.stage("observe", fgs)
    assert_hyp_equal(dmg.currentDepthMap(), dmo.get(), "observeDepth reactivated")


@pytest.mark.parametrize("allow", [1, 0])
def test_observe_far_scene_negative_idepths(oracle, hip, allow):
    """allowNegativeIdepths (C/DepthEstimation/DepthMap.cpp:1904-1909; the ROS cfg offers it, cfg/LSDParams.cfg:25): a
    prior 50x too far puts the search at the infinity end of the epipolar line, where the matched position gives
    idepth_new < 0 for a few hundred pixels.  With the switch off those return -2 (validity -= 5, var *= 1.1, possibly
    invalidate + blacklist); with it on they are fused.  Both settings bit-exact, and the two settings must differ (the
    branch is really taken)."""
    w, h = 320, 240
    params = {"allowNegativeIdepths": allow}
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, w, h, 8, params=params)

    def far_map(op, with_hip):
        kfo, kfg, dmo, dmg = _noisy_map(oracle, hip, ctx, frames, depth0, K, w, h, op=op)
        hyp = dmo.get()
        for k in ("idepth", "idepth_smoothed"):
            hyp[k] *= np.float32(0.02)
        for k in ("idepth_var", "idepth_var_smoothed"):
            hyp[k] *= np.float32(0.02 * 0.02)
        dmo.set(kfo, hyp)
        dmg.setCurrentDepthMap(kfg, hyp)
        fos, fgs = _ref_frames(oracle, hip, ctx, frames, K, gt, kfo, kfg, [3, 4, 6, 7])
        dmo.stage("observe", fos)
        if with_hip:
            dmg.stage("observe", fgs)
            assert_hyp_equal(dmg.currentDepthMap(), dmo.get(), "observeDepth far scene allowNegativeIdepths=%d" % allow)
        return dmo.get()

    mine = far_map(oracle_params(oracle, params), True)
    other = far_map(oracle_params(oracle, {"allowNegativeIdepths": 1 - allow}), False)
    assert int((mine["validity_counter"] != other["validity_counter"]).sum()) > 50, "the negative-idepth branch was not exercised"


@pytest.mark.parametrize("params", STEREO)
@pytest.mark.parametrize("w,h", [(176, 144), (640, 480)])
def test_update_keyframe_end_to_end(oracle, hip, w, h, params):
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, w, h, 6, params=params)
    kfo, kfg, dmo, dmg = _noisy_map(oracle, hip, ctx, frames, depth0, K, w, h, seed=11, op=oracle_params(oracle, params))
    for i in range(1, 6):
        fos, fgs = _ref_frames(oracle, hip, ctx, frames, K, gt, kfo, kfg, [i], seed=i)
        dmo.update(fos)
        dmg.updateKeyframe(fgs)
        assert_hyp_equal(dmg.currentDepthMap(), dmo.get(), "updateKeyframe %d" % i)
    so, sg = kfo.stats(), kfg.stats()
    assert sg["numMappedOnThis"] == so["numMappedOnThis"] == 5
    # setDepth ran on the first update only (depthHasBeenUpdatedFlag, DepthMap.cpp:1150)
    assert sg["depthHasBeenUpdatedFlag"] == so["depthHasBeenUpdatedFlag"] == 1
    assert sg["numPoints"] == so["numPoints"]
    # the reference accumulates sumIdepth sequentially in float32 (Frame.cpp:222); the device sums in float64
    assert sg["meanIdepth"] == pytest.approx(so["meanIdepth"], rel=2e-4)
    for lvl in range(5):
        assert_bit_equal(kfg.idepth(lvl), kfo.plane("idepth", lvl), "kf idepth L%d" % lvl)
        assert_bit_equal(kfg.idepthVar(lvl), kfo.plane("idepthVar", lvl), "kf idepthVar L%d" % lvl)


def test_initialize_randomly_draws_the_same_rand_sequence(oracle, hip):
    """DepthMap::initializeRandomly (DepthMap.cpp:883-916) consumes the C library's rand() once per pixel above minUseGrad,
    in row-major order: with the same seed both sides must produce the same map, and the keyframe planes setDepth derives."""
    import ctypes
    libc = ctypes.CDLL(None)
    w, h = 320, 240
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, w, h, 1)
    kfo, kfg = oracle.Frame(0, frames[0], K), hip.Frame(ctx, 0, frames[0])
    dmo, dmg = oracle.DepthMap(w, h, K), hip.DepthMap(ctx)
    libc.srand(12345)
    dmo.init_random(kfo)
    libc.srand(12345)
    dmg.initializeRandomly(kfg)
    ho = dmo.get()
    assert int(ho["isValid"].sum()) > 1000
    assert_hyp_equal(dmg.currentDepthMap(), ho, "initializeRandomly")
    for lvl in range(5):
        assert_bit_equal(kfg.idepth(lvl), kfo.plane("idepth", lvl), "kf idepth L%d" % lvl)
        assert_bit_equal(kfg.idepthVar(lvl), kfo.plane("idepthVar", lvl), "kf idepthVar L%d" % lvl)


def oracle_prerescale_after_propagate(dmo):
    """createKeyFrame behind propagateDepth up to the rescale (oracle/orc_depthmap.cpp DepthMap::createKeyFrame): regularizeDepthMap(true),
    fill holes, regularizeDepthMap(false) -> the pre-rescale map"""
    dmo.stage("regularize_occ")
    dmo.stage("fillholes")
    dmo.stage("regularize")
    return dmo.get()


def expected_rescale(pre, what=""):
    """(f, allowed, N): f = float32(N) / float32(S64), S64 the float64 sum of the pre-rescale idepth_smoothed over the N valid pixels.  The
    device's float64 tree sum lies within N * 2^-53 relative of S64; only if float32(S64) changes inside that interval (S64 that close to a
    float32 rounding tie) is a neighbouring factor allowed too — reported when it happens."""
    v = pre["isValid"] > 0
    N = int(v.sum())
    assert N > 0, what
    S64 = float(pre["idepth_smoothed"][v].astype(np.float64).sum())
    n32 = np.float32(N)
    f = n32 / np.float32(S64)
    eps = N * 2.0 ** -53
    lo, hi = np.float32(S64 * (1 - eps)), np.float32(S64 * (1 + eps))
    allowed = {float(f)}
    if lo != hi:
        print("%s: the float64 sum %.17g lies within N * 2^-53 of a float32 rounding tie: both neighbouring factors are accepted" % (what, S64))
        allowed |= {float(n32 / lo), float(n32 / hi)}
    return f, allowed, N


def assert_created_keyframe_exact(oracle, what, pre, s_g, s_o, gg, nkg, pose_o, K, nk_image):
    """createKeyFrame's result against the oracle's PRE-rescale map `pre` (all valid pixels, bit for bit): s_g the device's factor, s_o the
    oracle's own (sequential float32 sum), gg the device's new map, nkg the device's new keyframe, pose_o the oracle's new keyframe pose."""
    f_exp, allowed, N = expected_rescale(pre, what)
    f = np.float32(s_g)
    assert float(f) == float(s_g) and float(f) in allowed, "%s: rescale factor %r, expected %r (N = %d)" % (what, s_g, sorted(allowed), N)
    # the oracle's own factor: its float32 running sum is within N * 2^-24 relative of the float64 sum (holds the construction to the oracle)
    assert abs(float(s_o) - float(f_exp)) <= N * 2.0 ** -24 * float(f_exp), (what, s_o, f_exp, N)
    assert_bit_equal(gg["isValid"], pre["isValid"], what + ": isValid")
    assert_bit_equal(gg["blacklisted"], pre["blacklisted"], what + ": blacklisted")
    v = pre["isValid"] > 0
    assert_bit_equal(gg["validity_counter"][v], pre["validity_counter"][v], what + ": validity_counter")
    assert_bit_equal(gg["nextStereoFrameMinID"][v], pre["nextStereoFrameMinID"][v], what + ": nextStereoFrameMinID")
    f2 = np.float32(f * f)
    want = {}
    for k, fac in (("idepth", f), ("idepth_smoothed", f), ("idepth_var", f2), ("idepth_var_smoothed", f2)):
        want[k] = (pre[k].astype(np.float32) * fac).astype(np.float32)      # one rounded multiply each
        assert_bit_equal(gg[k][v], want[k][v], what + ": " + k)
    # the new keyframe: Frame::setDepth's rule on level 0, the pyramid an oracle frame builds from those planes above it
    ok = v & (want["idepth_smoothed"].astype(np.float64) >= -0.05)
    id0 = np.where(ok, want["idepth_smoothed"], np.float32(-1)).astype(np.float32)
    var0 = np.where(ok, want["idepth_var_smoothed"], np.float32(-1)).astype(np.float32)
    fo = oracle.Frame(0, nk_image, K)
    fo.set_depth_planes(id0, var0)
    assert_bit_equal(nkg.idepth(0), id0, what + ": new keyframe idepth L0")
    assert_bit_equal(nkg.idepthVar(0), var0, what + ": new keyframe idepthVar L0")
    for lvl in range(1, 5):
        assert_bit_equal(nkg.idepth(lvl), fo.plane("idepth", lvl), what + ": new keyframe idepth L%d" % lvl)
        assert_bit_equal(nkg.idepthVar(lvl), fo.plane("idepthVar", lvl), what + ": new keyframe idepthVar L%d" % lvl)
    sg = nkg.stats()
    assert sg["numPoints"] == int(ok.sum()), what
    mean64 = float(id0[ok].astype(np.float64).sum()) / max(int(ok.sum()), 1)
    assert abs(sg["meanIdepth"] - mean64) <= int(ok.sum()) * 2.0 ** -24 * abs(mean64), (what, sg["meanIdepth"], mean64)
    pg = np.asarray(nkg.thisToParent_raw())
    assert np.allclose(pg[:7], np.asarray(pose_o)[:7], atol=1e-12, rtol=0), (what, pg, pose_o)
    assert pg[7] == float(f), (what, pg[7], f)
    return want


@pytest.mark.parametrize("use_mask", [True, False])
def test_propagate_and_create_keyframe(oracle, hip, use_mask):
    w, h = 640, 480
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, w, h, 10)
    kfo, kfg, dmo, dmg = _noisy_map(oracle, hip, ctx, frames, depth0, K, w, h, sigma=0.05, seed=21)
    dmo.stage("regularize")
    dmg.stage("regularize")
    fos, fgs = _ref_frames(oracle, hip, ctx, frames, K, gt, kfo, kfg, [9], with_masks=use_mask)
    nko, nkg = fos[0], fgs[0]
    # K7 alone
    hyp0 = dmo.get()
    dmo.stage("propagate", [nko])
    dmg.stage("propagate", [nkg])
    assert_hyp_equal(dmg.currentDepthMap(), dmo.get(), "propagateDepth")
    # ... and on through createKeyFrame's passes up to the rescale: the oracle's pre-rescale map
    pre = oracle_prerescale_after_propagate(dmo)
    # full createKeyFrame from the same starting state
    dmo.set(kfo, hyp0)
    dmg.setCurrentDepthMap(kfg, hyp0)
    s_o = dmo.create_keyframe(nko)
    s_g = dmg.createKeyFrame(nkg)
    assert_created_keyframe_exact(oracle, "createKeyFrame", pre, s_g, s_o, dmg.currentDepthMap(), nkg, nko.pose(), K, frames[9])
    assert nkg.stats()["numPoints"] == nko.stats()["numPoints"]


def test_propagate_zoom_out_more_sources_than_slots(oracle, hip):
    """propagateDepth when the new keyframe looks at the scene from much further away: up to ~16 source hypotheses land on one
    target pixel, more than the 8 slots a target has — the rest travel on per-target chains and the merge still replays them in
    the reference's order (bit-exact; round 1 reported LSDHIP_E_CAPACITY here)."""
    w, h = 320, 240
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, w, h, 4)
    kfo, kfg, dmo, dmg = _noisy_map(oracle, hip, ctx, frames, depth0, K, w, h, sigma=0.02, seed=33)
    dmo.stage("regularize")
    dmg.stage("regularize")
    fo, fg = oracle.Frame(2, frames[2], K), hip.Frame(ctx, 2, frames[2])
    # camera of the new keyframe 3.5 depth units behind the old one (scene depth ~2): image of the old map shrinks ~2.7x
    back = oracle.se3_exp(np.array([0.0, 0.0, -3.5, 0.0, 0.0, 0.0]))
    sim3 = np.concatenate([back, [1.0]])
    fo.set_pose(sim3, kfo, 0.5)
    fg.setPose(sim3, kfg, 0.5)
    n_src = int((dmo.get()["isValid"] > 0).sum())
    dmo.stage("propagate", [fo])
    dmg.stage("propagate", [fg])
    go, gg = dmo.get(), dmg.currentDepthMap()
    n_dst = int((go["isValid"] > 0).sum())
    assert n_dst > 1000 and n_src > 8 * n_dst, (n_src, n_dst)     # more than 8 sources per target on average: the chains are in use
    assert_hyp_equal(gg, go, "propagateDepth (zoom-out)")


def test_finalize_and_reactivation(oracle, hip):
    w, h = 320, 240
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, w, h, 3)
    kfo, kfg, dmo, dmg = _noisy_map(oracle, hip, ctx, frames, depth0, K, w, h, seed=4)
    dmo.finalize()
    dmg.finalizeKeyFrame()
    assert_hyp_equal(dmg.currentDepthMap(), dmo.get(), "finalizeKeyFrame")
    for lvl in range(5):
        assert_bit_equal(kfg.idepth(lvl), kfo.plane("idepth", lvl), "finalize idepth L%d" % lvl)
    # wipe and re-activate from the keyframe's own re-activation data (setFromExistingKF)
    dmo.set_from_existing(kfo)
    dmg.setFromExistingKF(kfg)
    assert_hyp_equal(dmg.currentDepthMap(), dmo.get(), "setFromExistingKF")


def test_usage_errors_are_loud(hip):
    frames, depth0, K, gt = sequence(160, 128, 2)
    with pytest.raises(hip.LsdHipError):
        hip.Context(150, 128, K)              # not a multiple of 16 (C/SlamSystem.cpp:55-59)
    ctx = hip.Context(160, 128, K)
    f = hip.Frame(ctx, 0, frames[0])
    ref = hip.TrackingReference()
    ref.importFrame(f)
    tr = hip.SE3Tracker(ctx)
    with pytest.raises(hip.LsdHipError):
        tr.trackFrame(ref, hip.Frame(ctx, 1, frames[1]), IDENT7)   # keyframe without depth
    dm = hip.DepthMap(ctx)
    with pytest.raises(hip.LsdHipError):
        dm.updateKeyframe([f])                # no active keyframe


@pytest.mark.gpu
def test_cpp_driver_loop_matches_python_loop(hip):
    """The C++ host loop (liblsdhip_driver.so, include/lsd_slam_hip.hpp) and the Python mirror issue the same C-ABI
    calls: identical poses, frame for frame, across two keyframe changes."""
    import time
    import lsd_slam_amd as la
    from lsd_slam_amd.driver import DriverLoop
    w, h = 320, 240
    frames, depth0, K, gt = sequence(w, h, 26)
    ctx = la.Context(w, h, K)
    loop = la.SlamLoop(ctx, frames[0], depth0, kf_every=10)
    py = [loop.step(frames[i], time.perf_counter) for i in range(1, 26)]
    imgs = [np.ascontiguousarray(f) for f in frames]
    drv = DriverLoop(w, h, K, imgs[0].ctypes.data, depth0, kf_every=10, images_on_device=False)
    done, poses = drv.run([imgs[i].ctypes.data for i in range(1, 26)], want_poses=True)
    assert done == 25
    st = drv.stats()
    assert st.frames == 25 and st.keyframes == 2 and st.updates == 23 and st.evaluations > 0
    assert np.array_equal(np.array(py), poses)
    # stop_at_keyframe returns right after the frame that became a keyframe
    drv2 = DriverLoop(w, h, K, imgs[0].ctypes.data, depth0, kf_every=10, images_on_device=False)
    done2, _ = drv2.run([imgs[i].ctypes.data for i in range(1, 26)], stop_at_keyframe=True)
    assert done2 == 10


@pytest.mark.gpu
@pytest.mark.parametrize("cap", ["8", "16"])
def test_multipass_levels_match_single_pass(oracle, hip, cap, monkeypatch):
    """Levels larger than the workgroup cap are evaluated grid-stride (several points per lane) and take the
    re-evaluation path for the SSE tail drop.  Forcing a tiny cap at 320x240 must reproduce the single-pass results of
    the same kernel: integer outputs and the mask exactly, reductions within float-summation noise, and the oracle
    contract of test_residual_kernel_fixed_pose."""
    w, h = 320, 240
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, w, h, 4)
    kfg = hip.Frame(ctx, 0, frames[0])
    kfg.setDepthFromGroundTruth(depth0)
    rg = hip.TrackingReference()
    rg.importFrame(kfg)
    kfo = oracle.Frame(0, frames[0], K)
    kfo.set_depth_gt(depth0)
    ro = oracle.TrackingReference()
    ro.import_frame(kfo)
    tro = oracle.SE3Tracker(w, h, K, mode=oracle.SSE_EXACT_RCP)
    tr_single = hip.SE3Tracker(ctx)
    monkeypatch.setenv("LSDHIP_TRACK_CAP", cap)
    tr_multi = hip.SE3Tracker(ctx)
    monkeypatch.delenv("LSDHIP_TRACK_CAP")
    T = oracle.se3_exp(np.array([0.03, -0.02, 0.01, 0.01, -0.015, 0.02])).astype(np.float32)
    for lvl in (3, 2, 1):
        f1, f2, fo = hip.Frame(ctx, 3, frames[3]), hip.Frame(ctx, 3, frames[3]), oracle.Frame(3, frames[3], K)
        a = tr_single.evaluate(rg, f1, T, lvl)
        b = tr_multi.evaluate(rg, f2, T, lvl)
        o = tro.evaluate(ro, fo, T, lvl)
        assert (b.warped_size, b.goodCount, b.badCount, b.num_constraints) == (a.warped_size, a.goodCount, a.badCount, a.num_constraints)
        assert (b.warped_size, b.goodCount, b.badCount, b.num_constraints) == (o.warped_size, o.goodCount, o.badCount, o.num_constraints)
        assert b.warped_size % 4 != 0 or lvl != 1 or True   # (the tail path runs whenever warped_size % 4 != 0)
        assert np.allclose(np.array(b.A), np.array(a.A), rtol=2e-5, atol=2e-6 * np.abs(np.array(a.A)).max())
        assert np.allclose(np.array(b.b), np.array(a.b), rtol=2e-5, atol=2e-6 * np.abs(np.array(a.b)).max())
        assert b.weightedError == pytest.approx(a.weightedError, rel=2e-5)
        assert b.weightedError == pytest.approx(o.weightedError, rel=2e-5)
        if lvl == 1:
            assert_bit_equal(f2.refPixelWasGoodNoCreate(), f1.refPixelWasGoodNoCreate(), "mask multi vs single")
            assert_bit_equal(f2.refPixelWasGoodNoCreate(), fo.wasgood(), "mask multi vs oracle")
    # and the whole LM loop lands on the same pose
    tr_single.set_maxItsPerLvl(ODOMETRY_ITS)
    tr_multi.set_maxItsPerLvl(ODOMETRY_ITS)
    f1, f2 = hip.Frame(ctx, 2, frames[2]), hip.Frame(ctx, 2, frames[2])
    p1 = tr_single.trackFrame(rg, f1, IDENT7)
    p2 = tr_multi.trackFrame(rg, f2, IDENT7)
    dt, dr = pose_distance(p1, p2, oracle)
    assert max(dt, dr) < 2e-4, (dt, dr)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["S1", "S2"])
def test_large_frame_1280x1024_track_and_update(oracle, hip, kind):
    """BASELINE.json configs[2]: 1280x1024, scene S2 (Voronoi edge texture, ~300 k semi-dense pixels) — and S1 at the same
    size.  Level 1 is 640x512 = 1280 tiles > the workgroup cap (multi-pass path)."""
    w, h = 1280, 1024
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, w, h, 3, kind=kind)
    kfo, kfg = oracle.Frame(0, frames[0], K), hip.Frame(ctx, 0, frames[0])
    kfo.set_depth_gt(depth0)
    kfg.setDepthFromGroundTruth(depth0)
    for lvl in range(5):
        assert_bit_equal(kfg.gradients(lvl), kfo.plane("gradients", lvl), "gradients L%d" % lvl)
        assert_bit_equal(kfg.idepth(lvl), kfo.plane("idepth", lvl), "idepth L%d" % lvl)
    ro, rg = oracle.TrackingReference(), hip.TrackingReference()
    ro.import_frame(kfo)
    rg.importFrame(kfg)
    tro, trg = oracle.SE3Tracker(w, h, K, mode=oracle.SSE), hip.SE3Tracker(ctx)
    tro.set_max_its(ODOMETRY_ITS)
    trg.set_maxItsPerLvl(ODOMETRY_ITS)
    fo, fg = oracle.Frame(1, frames[2], K), hip.Frame(ctx, 1, frames[2])
    r = tro.track(ro, fo, IDENT7)
    est = trg.trackFrame(rg, fg, IDENT7)
    dt, dr = pose_distance(est, np.array(r.frameToRef), oracle)
    assert max(dt, dr) < 5e-4, (dt, dr)
    assert (fg.refPixelWasGoodNoCreate() != fo.wasgood()).mean() < 2e-3
    # depth update with identical pose and mask: bit-exact
    pose = np.concatenate([np.array(r.frameToRef), [1.0]])
    fg.setPose(pose, kfg, fo.stats()["initialTrackedResidual"])
    fg.set_refPixelWasGood(fo.wasgood())
    dmo, dmg = oracle.DepthMap(w, h, K), hip.DepthMap(ctx)
    dmo.init_gt(kfo)
    dmg.initializeFromGTDepth(kfg)
    dmo.update([fo])
    dmg.updateKeyframe([fg])
    assert_hyp_equal(dmg.currentDepthMap(), dmo.get(), "updateKeyframe 1280x1024")
    if kind == "S2":
        n = int((dmo.get()["isValid"] > 0).sum())
        assert 200_000 < n < 420_000, n     # configs[2]: ~300 k semi-dense pixels


@pytest.mark.gpu
def test_track_batch_equals_single_calls(oracle, hip):
    """lsdhip_tracker_track_batch: n jobs in the same launches give the poses, flags, masks and side effects of n single
    trackFrame calls (same kernel; a batch may tile a level into fewer workgroups, which only changes summation order)."""
    w, h = 320, 240
    seqs = [sequence(w, h, 4, seq_index=s) for s in range(3)]
    ctx = hip.Context(w, h, seqs[0][2])
    singles, batch_in = [], []
    for s, (frames, depth0, K, gt) in enumerate(seqs):
        for copy in range(2):
            kf = hip.Frame(ctx, 100 * s, frames[0])
            kf.setDepthFromGroundTruth(depth0)
            ref = hip.TrackingReference()
            ref.importFrame(kf)
            fr = hip.Frame(ctx, 100 * s + 1, frames[1 + s])
            (singles if copy == 0 else batch_in).append((ref, fr, kf))
    tr = hip.SE3Tracker(ctx)
    tr.set_maxItsPerLvl(ODOMETRY_ITS)
    single_res = []
    for ref, fr, kf in singles:
        pose = tr.trackFrame(ref, fr, IDENT7)
        single_res.append((pose, tr.last.numEvaluations, tr.lastResidual, tr.pointUsage, tr.trackingWasGood, fr.refPixelWasGoodNoCreate(),
                           fr.stats()["initialTrackedResidual"], kf.stats()["numFramesTrackedOnThis"]))
    poses, recs = tr.trackFrameBatch([b[0] for b in batch_in], [b[1] for b in batch_in], np.tile(IDENT7, (3, 1)))
    for j, (ref, fr, kf) in enumerate(batch_in):
        sp, sev, sres, suse, sgood, smask, sitr, sntr = single_res[j]
        dtj, drj = pose_distance(poses[j], sp, oracle)
        assert max(dtj, drj) < 2e-4, (j, dtj, drj)   # a batch uses fewer, fatter workgroups per job: other summation order
        assert abs(recs[j].numEvaluations - sev) <= 2
        assert recs[j].lastResidual == pytest.approx(sres, rel=5e-2) and recs[j].pointUsage == pytest.approx(suse, rel=1e-3)
        assert bool(recs[j].trackingWasGood) == sgood
        assert (fr.refPixelWasGoodNoCreate() != smask).mean() < 2e-3
        assert fr.stats()["initialTrackedResidual"] == pytest.approx(sitr, rel=5e-2) and kf.stats()["numFramesTrackedOnThis"] == sntr


@pytest.mark.gpu
@pytest.mark.parametrize("coarse", [None, 1])
def test_track_batch_throughput_mode_matches_single_calls(oracle, hip, coarse):
    """>= 8 jobs switch the batch to its throughput mode (strips of the keyframe level compacted to their valid pixels in
    LDS, tail points re-evaluated): same points, same per-point arithmetic, another summation order.
    coarse = 1: the levels of at most 4800 pixels (here 4, 3 and 2) walked by one workgroup per job with the level's texel plane staged in
    LDS (k_track_solo, the default from 24 jobs per batch): the same bounds."""
    w, h = 320, 240
    seqs = [sequence(w, h, 4, seq_index=s) for s in range(3)]
    ctx = hip.Context(w, h, seqs[0][2])
    tr = hip.SE3Tracker(ctx)
    tr.set_maxItsPerLvl(ODOMETRY_ITS)
    if coarse is not None:
        tr.set_batch_coarse_min_jobs(coarse)
    refs, frs, want = [], [], []
    for s, (frames, depth0, K, gt) in enumerate(seqs):
        for k in (1, 2, 3):
            pair = []
            for copy in range(2):
                kf = hip.Frame(ctx, 100 * s + 10 * k, frames[0])
                depth = depth0.copy()
                if k == 3:
                    depth[::2, 1::3] = 0          # ragged validity
                kf.setDepthFromGroundTruth(depth)
                ref = hip.TrackingReference()
                ref.importFrame(kf)
                pair.append((ref, hip.Frame(ctx, 100 * s + 10 * k + 1, frames[k]), kf))
            (ref, fr, kf) = pair[0]
            pose = tr.trackFrame(ref, fr, IDENT7)
            want.append((pose, tr.last.numEvaluations, tr.lastResidual, tr.pointUsage, tr.trackingWasGood, fr.refPixelWasGoodNoCreate()))
            refs.append(pair[1][0]); frs.append(pair[1][1])
    assert len(refs) == 9
    poses, recs = tr.trackFrameBatch(refs, frs, np.tile(IDENT7, (9, 1)))
    for j in range(9):
        sp, sev, sres, suse, sgood, smask = want[j]
        dtj, drj = pose_distance(poses[j], sp, oracle)
        assert max(dtj, drj) < 2e-4, (j, dtj, drj)
        assert abs(recs[j].numEvaluations - sev) <= 2
        assert recs[j].lastResidual == pytest.approx(sres, rel=5e-2) and recs[j].pointUsage == pytest.approx(suse, rel=1e-3)
        assert bool(recs[j].trackingWasGood) == sgood
        assert (frs[j].refPixelWasGoodNoCreate() != smask).mean() < 2e-3
    # run-to-run deterministic
    frs2 = [hip.Frame(ctx, 900 + j, seqs[j // 3][0][1 + j % 3]) for j in range(9)]
    poses2, _ = tr.trackFrameBatch(refs, frs2, np.tile(IDENT7, (9, 1)))
    assert np.array_equal(poses, poses2)


@pytest.mark.gpu
def test_track_batch_coarse_levels_fall_back_to_strips_when_a_level_does_not_fit(oracle, hip):
    """k_track_solo holds the texel plane of a level of at most 4800 pixels in LDS and at most 4608 of its reference points in registers.
    At 752x480 level 4 (47x30) fits and level 3 (94x60 = 5640 pixels, 5336 valid points on a dense keyframe) does not: the workgroup walks
    level 4 and hands the job — state at level 3, nothing pending — to the lock-step rounds.  Same bounds against single calls as the other
    batch tests."""
    w, h = 752, 480
    seqs = [sequence(w, h, 3, seq_index=s) for s in range(4)]
    ctx = hip.Context(w, h, seqs[0][2])
    tr = hip.SE3Tracker(ctx)
    tr.set_maxItsPerLvl(ODOMETRY_ITS)
    with pytest.raises(hip.LsdHipError):
        tr.set_batch_coarse_min_jobs(-1)
    tr.set_batch_coarse_min_jobs(1)
    refs, frs, want = [], [], []
    for s, (frames, depth0, K, gt) in enumerate(seqs):
        for k in (1, 2):
            pair = []
            for copy in range(2):
                kf = hip.Frame(ctx, 100 * s + 10 * k, frames[0])
                depth = depth0.copy()
                depth[~(depth > 0)] = np.median(depth0[depth0 > 0])
                kf.setDepthPlanes(1.0 / depth, np.full_like(depth, 1e-4))     # a hypothesis on every pixel
                ref = hip.TrackingReference()
                ref.importFrame(kf)
                pair.append((ref, hip.Frame(ctx, 100 * s + 10 * k + 1, frames[k])))
            assert pair[0][0].keyframe.idepthVar(3).size > 4800 and int((pair[0][0].keyframe.idepthVar(3)[1:-1, 1:-1] > 0).sum()) > 4608     # too large either way
            pose = tr.trackFrame(pair[0][0], pair[0][1], IDENT7)
            want.append((pose, tr.last.numEvaluations, tr.lastResidual, pair[0][1].refPixelWasGoodNoCreate()))
            refs.append(pair[1][0]); frs.append(pair[1][1])
    poses, recs = tr.trackFrameBatch(refs, frs, np.tile(IDENT7, (8, 1)))
    for j in range(8):
        sp, sev, sres, smask = want[j]
        dtj, drj = pose_distance(poses[j], sp, oracle)
        assert max(dtj, drj) < 2e-4, (j, dtj, drj)
        assert abs(recs[j].numEvaluations - sev) <= 2
        assert recs[j].lastResidual == pytest.approx(sres, rel=5e-2)
        assert (frs[j].refPixelWasGoodNoCreate() != smask).mean() < 2e-3


def test_permaref_batch_matches_single_and_oracle(oracle, hip):
    """several keyframes' permanent references (level-4 clouds) tracked against one new frame in the same
    launches give what single trackFrameOnPermaref calls and the oracle give."""
    w, h = 640, 480
    K = sequence(w, h, 4, seq_index=0)[2]
    ctx = hip.Context(w, h, K)
    clouds, singles, oracles = [], [], []
    target_frames = sequence(w, h, 4, seq_index=0)[0]
    fg = hip.Frame(ctx, 50, target_frames[2])
    T0s = []
    for s in range(3):
        frames, depth0, K_, gt = sequence(w, h, 4, seq_index=0)
        kfo = oracle.Frame(s, frames[s], K)      # keyframes = frames 0, 1, 2 of the sequence, all with GT depth of frame 0's view
        kfo.set_depth_gt(depth0)
        ro = oracle.TrackingReference()
        ro.import_frame(kfo)
        pos, cv, _, _ = ro.pointcloud(4)
        clouds.append((pos, cv))
        T0 = oracle.se3_exp(np.array([0.005 * (s + 1), 0.0, 0.0, 0, 0, 0.001 * s]))
        T0s.append(T0)
        tro = oracle.SE3Tracker(w, h, K, mode=oracle.SSE_EXACT_RCP)
        r = tro.track_permaref(pos, cv, oracle.Frame(50, target_frames[2], K), T0)
        oracles.append(r)
        trs = hip.SE3Tracker(ctx)
        singles.append((trs.trackFrameOnPermaref(pos, cv, fg, T0), trs.trackingWasGood, trs.lastResidual))
    trb = hip.SE3Tracker(ctx)
    poses, recs = trb.trackFrameOnPermarefBatch(clouds, [fg] * 3, np.array(T0s))
    for j in range(3):
        # level 4 is a single tile either way: identical arithmetic to the single call
        assert np.array_equal(poses[j], singles[j][0]), j
        assert bool(recs[j].trackingWasGood) == singles[j][1] and recs[j].lastResidual == singles[j][2]
        if not oracles[j].diverged:
            dt, dr = pose_distance(poses[j], np.array(oracles[j].frameToRef), oracle)
            assert max(dt, dr) < 2e-3, (j, dt, dr)
        assert bool(recs[j].diverged) == bool(oracles[j].diverged)


@pytest.mark.gpu
def test_tracker_settings_block_reaches_the_device(oracle, hip):
    """lsdhip_tracker_set_settings: every DenseDepthTrackerSettings field (C/util/settings.h:355-402).  Defaults equal the
    reference's; changed fields change the run the way they change the oracle's."""
    w, h = 320, 240
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, w, h, 4)
    kfo, kfg = oracle.Frame(0, frames[0], K), hip.Frame(ctx, 0, frames[0])
    kfo.set_depth_gt(depth0)
    kfg.setDepthFromGroundTruth(depth0)
    ro, rg = oracle.TrackingReference(), hip.TrackingReference()
    ro.import_frame(kfo)
    rg.importFrame(kfg)
    trg = hip.SE3Tracker(ctx)
    st = trg.settings()
    assert (st.lambdaSuccessFac, st.lambdaFailFac, st.huber_d, st.var_weight) == (0.5, 2.0, 3.0, 1.0)
    assert list(st.maxItsPerLvl) == [5, 20, 50, 100, 100] and list(st.convergenceEps) == [pytest.approx(0.999)] * 5
    assert (st.stepSizeMinTestTrack, st.convergenceEpsTestTrack, st.maxItsTestTrack) == (pytest.approx(1e-3), pytest.approx(0.98), 5.0)
    # one iteration per level, Huber threshold 1: fewer evaluations, another (but oracle-consistent) pose
    for l in range(5):
        st.maxItsPerLvl[l] = 1
    st.huber_d = 1.0
    trg.set_settings(st)
    tro = oracle.SE3Tracker(w, h, K, mode=oracle.SSE)
    tro.set_max_its([1, 1, 1, 1, 1])
    L = oracle.lib()
    import ctypes
    if hasattr(L, "orc_tracker_set_huber"):
        L.orc_tracker_set_huber.argtypes = [ctypes.c_void_p, ctypes.c_float]
        L.orc_tracker_set_huber(tro.h_, 1.0)
    est = trg.trackFrame(rg, hip.Frame(ctx, 2, frames[2]), IDENT7)
    if hasattr(L, "orc_tracker_set_huber"):
        r = tro.track(ro, oracle.Frame(2, frames[2], K), IDENT7)
        dt, dr = pose_distance(est, np.array(r.frameToRef), oracle)
        assert max(dt, dr) < 5e-4, (dt, dr)
        assert abs(r.numEvaluations - trg.last.numEvaluations) <= 2
        full = hip.SE3Tracker(ctx)
        full.trackFrame(rg, hip.Frame(ctx, 2, frames[2]), IDENT7)
        assert full.last.numWarpUpdates > trg.last.numWarpUpdates      # the iteration caps were really applied


@pytest.mark.gpu
@pytest.mark.parametrize("trials,params", [(2, {}), (5, {}), (6, {}), (6, {"useAffineLightningEstimation": 0})])
def test_speculative_retries_give_the_one_evaluation_per_launch_run(oracle, hip, trials, params):
    """lsdhip_tracker_set_speculation: a step evaluates the next `trials` poses of the LM loop's retry chain side by side and the
    next step consumes them in the reference's order.  With the same workgroups per trial as the one-evaluation-per-step run
    (identical partial-sum tiling) every output is the same BIT FOR BIT — pose, counters, residual, the frame's refPixelWasGood
    (which must be what the last trial the LM loop executed wrote, not what a later speculative one did) — in fewer dependent steps."""
    w, h = 640, 480
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, w, h, 8, params=params)
    kf = hip.Frame(ctx, 0, frames[0])
    kf.setDepthFromGroundTruth(depth0)
    ref = hip.TrackingReference()
    ref.importFrame(kf)
    tr_a, tr_b = hip.SE3Tracker(ctx), hip.SE3Tracker(ctx)
    tr_a.set_maxItsPerLvl(ODOMETRY_ITS)
    tr_b.set_maxItsPerLvl(ODOMETRY_ITS)
    tr_a.set_speculation(1)
    tr_b.set_speculation(trials, 304)       # 304 = the single-trial grid at 320x240 (level 1)
    init = IDENT7.copy()
    saved = 0
    for i in range(1, 8):
        fa, fb = hip.Frame(ctx, i, frames[i]), hip.Frame(ctx, i, frames[i])
        pa = tr_a.trackFrame(ref, fa, init)
        pb = tr_b.trackFrame(ref, fb, init)
        assert np.array_equal(pa, pb), (i, pa, pb)
        for k in ("numEvaluations", "numWarpUpdates", "lastResidual", "pointUsage", "lastGoodCount", "lastBadCount", "lastMeanRes",
                  "affineEstimation_a", "affineEstimation_b", "diverged", "trackingWasGood"):
            assert getattr(tr_a.last, k) == getattr(tr_b.last, k), (i, k)
        assert tr_a.exec_stats()[3] == tr_b.exec_stats()[3]
        assert_bit_equal(fa.refPixelWasGoodNoCreate(), fb.refPixelWasGoodNoCreate(), "refPixelWasGood")
        ca, sa, ka, _ = tr_a.step_stats()
        cb_, sb, kb, cb = tr_b.step_stats()
        la, lb = ca + sa, cb_ + sb                  # dependent steps = chain launches
        # one evaluation per launch: launches == evaluations
        assert cb == trials and la == tr_a.last.numEvaluations and lb <= la and ka == kb == 0
        saved += la - lb
        init = pa
    assert saved >= 7 * 3, saved           # the retry chains that end every level collapse into single launches
    # divergence: the trial that diverges first in the reference's order decides, not a speculative one
    bad = oracle.se3_exp(np.array([5.0, 0, 0, 0, 0, 0]))
    est = tr_b.trackFrame(ref, hip.Frame(ctx, 9, frames[1]), bad)
    assert tr_b.diverged and not tr_b.trackingWasGood and np.array_equal(est, IDENT7)
    # permanent-reference path (no mask) through the same chain
    kfo = oracle.Frame(0, frames[0], K)
    kfo.set_depth_gt(depth0)
    ro = oracle.TrackingReference()
    ro.import_frame(kfo)
    pos, cv, _, _ = ro.pointcloud(4)
    T0 = oracle.se3_exp(np.array([0.01, 0.0, 0.0, 0, 0, 0.002]))
    ua = tr_a.trackFrameOnPermaref(pos, cv, hip.Frame(ctx, 3, frames[3]), T0)
    ub = tr_b.trackFrameOnPermaref(pos, cv, hip.Frame(ctx, 3, frames[3]), T0)
    assert np.array_equal(ua, ub) and tr_a.last.numEvaluations == tr_b.last.numEvaluations


@pytest.mark.gpu
@pytest.mark.parametrize("budget", [1, 3])
def test_running_out_of_launch_budget_changes_nothing(oracle, hip, budget, monkeypatch):
    """A job that needs more k_track_step launches than the host enqueued: the budget's last launch reports it (TrackSummary::exhausted,
    pinned memory — the wait loop polls that next to `done`, no hipStreamQuery), the host appends launches and the chain continues
    from the state in HBM.  LSDHIP_BUDGET_FIXED makes every job run out several times; pose, counters, residual and the frame's
    refPixelWasGood are those of the normally budgeted run, bit for bit."""
    w, h = 640, 480
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, w, h, 5)
    kf = hip.Frame(ctx, 0, frames[0])
    kf.setDepthFromGroundTruth(depth0)
    ref = hip.TrackingReference()
    ref.importFrame(kf)
    tr_a = hip.SE3Tracker(ctx)
    monkeypatch.setenv("LSDHIP_BUDGET_FIXED", str(budget))
    tr_b = hip.SE3Tracker(ctx)                  # the environment is read when the tracker is created
    monkeypatch.delenv("LSDHIP_BUDGET_FIXED")
    tr_a.set_maxItsPerLvl(ODOMETRY_ITS)
    tr_b.set_maxItsPerLvl(ODOMETRY_ITS)
    init = IDENT7.copy()
    for i in range(1, 5):
        fa, fb = hip.Frame(ctx, i, frames[i]), hip.Frame(ctx, i, frames[i])
        pa = tr_a.trackFrame(ref, fa, init)
        pb = tr_b.trackFrame(ref, fb, init)
        assert np.array_equal(pa, pb), (i, pa, pb)
        for k in ("numEvaluations", "numWarpUpdates", "lastResidual", "pointUsage", "lastGoodCount", "lastBadCount", "lastMeanRes",
                  "affineEstimation_a", "affineEstimation_b", "diverged", "trackingWasGood"):
            assert getattr(tr_a.last, k) == getattr(tr_b.last, k), (i, k)
        assert_bit_equal(fa.refPixelWasGoodNoCreate(), fb.refPixelWasGoodNoCreate(), "refPixelWasGood")
        la, lb = tr_a.launch_stats()[0], tr_b.launch_stats()[0]
        # launches that did work: more than two budgets' worth, and the same number in both runs (the round-5 allowance of one is gone:
        # what differed was not the count but the host's view of it — the tail of the pinned summary record landing after its `done`
        # word, profiles/r06_notes.md section 1; the record now carries a check word, test_polled_summary_is_taken_whole)
        assert la == lb and la > 2 * budget, (la, lb)
        init = pa


@pytest.mark.gpu
def test_polled_summary_is_taken_whole(oracle, hip, monkeypatch):
    """The root cause of round 5's launch-count off-by-one (VERDICT r05 next #1a): a polled job's summary lives in pinned host memory; the
    finishing launch stores ~80 words, a system-scope release fence and then the `done` word — and about one job in a thousand the words
    stored last (levelEvals, numLaunches, lastCand; once lastResidual and the raw sums) were still the PREVIOUS job's when `done` had
    arrived (3 - 19 us late; tools/launch_count_stress.py, profiles/r06_notes.md section 1).  The record now carries a position-weighted
    check word and the host takes it only when it adds up.  Here: the same four jobs 300 times on trackers with launch budgets
    normal / 1 / 1 / 2 / 3 — launch counts, evaluation counts and poses equal every time, across trackers and across repeats."""
    w, h = 640, 480
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, w, h, 5)
    kf = hip.Frame(ctx, 0, frames[0])
    kf.setDepthFromGroundTruth(depth0)
    ref = hip.TrackingReference()
    ref.importFrame(kf)
    trackers = []
    for budget in (0, 1, 1, 2, 3):
        if budget:
            monkeypatch.setenv("LSDHIP_BUDGET_FIXED", str(budget))
        else:
            monkeypatch.delenv("LSDHIP_BUDGET_FIXED", raising=False)
        t = hip.SE3Tracker(ctx)
        t.set_maxItsPerLvl(ODOMETRY_ITS)
        trackers.append(t)
    monkeypatch.delenv("LSDHIP_BUDGET_FIXED", raising=False)
    expect = {}
    for rep in range(300):
        fi = 1 + rep % 4
        for t in trackers:
            f = hip.Frame(ctx, 10 + rep, frames[fi])
            p = t.trackFrame(ref, f, IDENT7)
            sig = (np.asarray(p).tobytes(), t.last.numEvaluations, t.launch_stats()[0], t.last.lastResidual)
            assert expect.setdefault(fi, sig) == sig, (rep, fi, sig[1:], expect[fi][1:])
            f.close()
    polled = sum(t.summary_stats()[0] for t in trackers)
    late = sum(t.summary_stats()[1] for t in trackers)
    assert polled == 300 * len(trackers)
    print("polled summaries: %d, incomplete when `done` arrived: %d (longest wait %d ns)" % (polled, late, max(t.summary_stats()[2] for t in trackers)))


@pytest.mark.gpu
def test_speculation_default_matches_oracle_sequence(oracle, hip):
    """the library default (5 / 5 / 6 trials at levels 1 / 2 / 3 of a 640x480 frame) against the oracle over a few frames"""
    w, h = 640, 480
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, w, h, 6)
    kfo, kfg = oracle.Frame(0, frames[0], K), hip.Frame(ctx, 0, frames[0])
    kfo.set_depth_gt(depth0)
    kfg.setDepthFromGroundTruth(depth0)
    ro, rg = oracle.TrackingReference(), hip.TrackingReference()
    ro.import_frame(kfo)
    rg.importFrame(kfg)
    tro, trg = oracle.SE3Tracker(w, h, K, mode=oracle.SSE), hip.SE3Tracker(ctx)
    tro.set_max_its(ODOMETRY_ITS)
    trg.set_maxItsPerLvl(ODOMETRY_ITS)
    assert trg.launch_stats()[1] == 6          # most trials per launch; per level by its size
    init = IDENT7.copy()
    for i in range(1, 6):
        fo, fg = oracle.Frame(i, frames[i], K), hip.Frame(ctx, i, frames[i])
        r = tro.track(ro, fo, init)
        est = trg.trackFrame(rg, fg, init)
        dt, dr = pose_distance(est, np.array(r.frameToRef), oracle)
        assert max(dt, dr) < 5e-4, (i, dt, dr)
        assert abs(r.numEvaluations - trg.last.numEvaluations) <= 3
        assert (fo.wasgood() != fg.refPixelWasGoodNoCreate()).mean() < 2e-3
        assert trg.launch_stats()[0] < trg.last.numEvaluations
        init = np.array(r.frameToRef)


@pytest.mark.gpu
@pytest.mark.parametrize("coarse", [None, 1])
def test_track_batch_speculation_is_bit_identical_to_one_trial_per_step(oracle, hip, coarse):
    """Throughput-mode batches evaluate the next retries of a job's reject chain side by side (levels without a mask) and consume them
    in the reference's order: same decisions, same evaluation counts, the same poses and masks bit for bit as one evaluation per step
    (lsdhip_tracker_set_speculation(t, 1, 0)) — in fewer rounds.  coarse = 1: levels 4..2 of these 320x240 jobs in one workgroup per job
    (k_track_solo, no speculation there), level 1 — the one that writes refPixelWasGood, one trial per round — in lock-step rounds: the
    same bits, the same number of rounds."""
    w, h = 320, 240
    seqs = [sequence(w, h, 5, seq_index=s) for s in range(4)]
    ctx = hip.Context(w, h, seqs[0][2])
    results = []
    for trials in (1, 0):
        tr = hip.SE3Tracker(ctx)
        tr.set_maxItsPerLvl(ODOMETRY_ITS)
        if trials == 1:
            tr.set_speculation(1)
        if coarse is not None:
            tr.set_batch_coarse_min_jobs(coarse)
        refs, frs = [], []
        for s, (frames, depth0, K, gt) in enumerate(seqs):
            for k in (1, 2, 3, 4):
                kf = hip.Frame(ctx, 100 * s + 10 * k, frames[0])
                depth = depth0.copy()
                if k == 3:
                    depth[::2, 1::3] = 0
                kf.setDepthFromGroundTruth(depth)
                ref = hip.TrackingReference()
                ref.importFrame(kf)
                refs.append(ref)
                frs.append(hip.Frame(ctx, 100 * s + 10 * k + 1, frames[k]))
        poses, recs = tr.trackFrameBatch(refs, frs, np.tile(IDENT7, (16, 1)))
        rounds = tr.launch_stats()[0]
        results.append((np.asarray(poses).copy(), [r.numEvaluations for r in recs], [r.lastResidual for r in recs],
                        [f.refPixelWasGoodNoCreate().copy() for f in frs], rounds))
    (p1, e1, r1, m1, n1), (p0, e0, r0, m0, n0) = results
    assert np.array_equal(p1, p0), np.abs(p1 - p0).max()
    assert e1 == e0 and r1 == r0
    for a, b in zip(m1, m0):
        assert np.array_equal(a, b)
    assert (n0 < n1) if coarse is None else (n0 == n1), (n0, n1)          # the reject chains collapsed: fewer rounds for the same evaluations


@pytest.mark.gpu
def test_unfused_build_holds_the_same_parity():
    """eval_finish fuses the multiply-adds of K2's weights and K3's Jacobian (LSD_EVAL_FMA = 1, the default).  The build with
    the reference's separately rounded operation order (liblsdhip_nofma.so: lsd_slam_amd/build.py build_variant("nofma", ["LSD_EVAL_FMA=0"]),
    built by __graft_entry__.build()) runs the kernel-level residual parity and the trackFrame parity tests in a fresh interpreter:
    both builds meet the same bounds, and a future regression in one of them can be bisected against the other."""
    import subprocess
    import sys
    lib = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lsd_slam_amd", "liblsdhip_nofma.so")
    if not os.path.exists(lib):
        pytest.skip("liblsdhip_nofma.so not built (python -c 'import __graft_entry__ as g; g.build()')")
    env = dict(os.environ, LSDHIP_LIB=lib)
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.abspath(__file__), "-k",
                        "residual_kernel_fixed_pose or trackframe_parity or affine_lighting_estimate"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in r.stdout
