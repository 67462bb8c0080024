"""Every device stage against the oracle at run-time settings other than the defaults (tests/settings_cases.py): minUseGrad,
cameraPixelNoise2, depthSmoothingFactor, KFDistWeight and KFUsageWeight, which lsdhip_params carries into a context and which the rest
of the suite leaves at util/settings.cpp's values.  A kernel or an argument builder that read 5.0f, 16.0f or 0.075f * 0.075f instead of
the context's value passes every other test; it fails here.

The checks are the existing ones, imported and run on a context (and an oracle) that hold a profile: bit-exact maps and pyramids, the
per-entry float64 bounds of the tracking and Sim3 evaluations, the pose bars of the function-level tests.  Every test also holds, from the
oracle alone, that the moved setting changes the result on these inputs by far more than the comparison allows (settings_cases.differs
against the default-settings oracle run; tests/test_settings_cpu.py holds the same conditions without a GPU).

The size is 176x144 (partial 32-wide tiles, an odd level-4 width); 320x240 only where a launch form needs it (the candidate-select batch
form, the strips, k_track_solo's coarse levels) and for the two function-level Sim3 cases, which run at the size their own files use."""
import ctypes

import numpy as np
import pytest

import reg_cases as rc
import reposition_ref as rr
import seq_loops as sl
import settings_cases as sc
import test_depth_batch_gpu as db
import test_reg_cases_gpu as rg
import test_sim3_eval_gpu as s3e
import test_sim3_gpu as s3
import test_track_batch_eval_gpu as tb
from common import assert_bit_equal, pose_distance, sequence
from test_gpu_parity import (_noisy_map, _ref_frames, assert_created_keyframe_exact, assert_gradient_candidates, assert_hyp_equal, make_pair,
                             oracle_params, oracle_prerescale_after_propagate, run_permaref_paths, test_trackframe_parity as trackframe_parity)
from test_sequence_gpu import _compare as compare_loops
from test_settings_cpu import assert_scenario_margins, assert_weights_bite, reposition_search

pytestmark = pytest.mark.gpu
W, H = sc.W, sc.H
f32 = np.float32


@pytest.fixture(scope="module")
def hip():
    import lsd_slam_amd as la
    return la


def profile(name, **more):
    return dict(sc.PROFILES[name], **more)


def interior(h, w, b):
    m = np.zeros((h, w), bool)
    m[b:h - b, b:w - b] = True
    return m


def threshold_plane(th, h, w, seed):
    """a maxGradients plane with entries exactly at the threshold, one ulp below and one ulp above it among random ones"""
    rng = np.random.default_rng(seed)
    plane = rng.uniform(0, 12, (h, w)).astype(np.float32)
    pick = rng.integers(0, 4, (h, w))
    th = f32(th)
    at, below, above = pick == 1, pick == 2, pick == 3
    plane[at], plane[below], plane[above] = th, np.nextafter(th, f32(0)), np.nextafter(th, f32(100))
    return plane, at, below, above


# ---------------------------------------------------------------------------------------------------------------
# 1. frames: k_set_depth_gt, the candidate builders
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.CAMERA)
def test_frames(oracle, hip, name):
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, W, H, 3, params=profile(name))
    th = ctx.params.minUseGrad
    assert th == f32(sc.PROFILES[name]["minUseGrad"])
    fo, fd, fg = oracle.Frame(0, frames[0], K), oracle.Frame(0, frames[0], K), hip.Frame(ctx, 0, frames[0])
    fo.set_depth_gt(depth0, minUseGrad=th)
    fd.set_depth_gt(depth0)
    fg.setDepthFromGroundTruth(depth0)
    for lvl in range(5):
        assert_bit_equal(fg.idepth(lvl), fo.plane("idepth", lvl), "idepth L%d" % lvl)
        assert_bit_equal(fg.idepthVar(lvl), fo.plane("idepthVar", lvl), "idepthVar L%d" % lvl)
    moved = int(((fo.plane("idepthVar", 0) > 0) != (fd.plane("idepthVar", 0) > 0)).sum())
    assert moved >= sc.MIN_VALIDITY_FLAGS, moved          # the threshold bites: the default-settings oracle keeps other pixels
    # the lists of a frame made alone, of frames made by lsdhip_frame_create_batch, and behind setMaxGradients
    n_alone = assert_gradient_candidates(fg, W, H, th)
    assert n_alone != assert_gradient_candidates_count(fg.maxGradients(0), 5.0)
    for j, f in enumerate(hip.Frame.createBatch(ctx, [10, 11, 12], images=[frames[0], frames[1], frames[2]])):
        n = assert_gradient_candidates(f, W, H, th)
        assert 0 < n < W * H and (j > 0 or n == n_alone)
    plane, at, below, above = threshold_plane(th, H, W, 3)
    fg.setMaxGradients(plane)
    n = assert_gradient_candidates(fg, W, H, th)
    inner = interior(H, W, 3)
    assert (at & inner).sum() > 100 and (below & inner).sum() > 100
    # >= : the entries at the threshold are candidates, those one ulp below are not
    assert n == int((inner & ~(plane < th)).sum()) and n >= int(((at | above) & inner).sum())


def assert_gradient_candidates_count(mg, th):
    ok = ~(mg < f32(th)) & interior(mg.shape[0], mg.shape[1], 3)
    return int(ok.sum())


# ---------------------------------------------------------------------------------------------------------------
# 2. the depth map, single calls
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.DEPTH_MAP)
def test_depth_map_single(oracle, hip, name):
    """the sequence of test_depth_stages_bit_exact, three updateKeyframe calls (the fused PassUpdateSetDepth tile twice, PassUpdate once),
    createKeyFrame with and without a mask, finalizeKeyFrame: assert_hyp_equal's bar, bit for bit"""
    params = profile(name)
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, W, H, sc.N_FRAMES, params=params)
    op = oracle_params(oracle, params)
    kfo, kfg, dmo, dmg = _noisy_map(oracle, hip, ctx, frames, depth0, K, W, H, op=op)
    kfo.set_counters(7, 3, 3, 0)
    kfg.setCounters(7, 3, 3, 0)
    fos, fgs = _ref_frames(oracle, hip, ctx, frames, K, gt, kfo, kfg, list(sc.REF_IDS))
    run = {}
    for stage in sc.STAGES:
        real = "observe" if stage.startswith("observe") else stage
        fr = {"observe": (fos, fgs), "observe2": (fos[1:], fgs[1:])}.get(stage, ((), ()))
        dmo.stage(real, fr[0])
        dmg.stage(real, fr[1])
        run[stage] = dmo.get()
        assert_hyp_equal(dmg.currentDepthMap(), run[stage], "%s: %s" % (name, stage))
    # the setting bit: this oracle run against the default-settings one (tests/test_settings_cpu.py computes both without a GPU)
    mine = sc.oracle_depth_stages(oracle, name)
    for stage in sc.STAGES:
        assert not any(sc.differs(run[stage], mine[stage]).values()), stage       # (the shared oracle-only run is this run)
    sc.assert_depth_setting_bit(name, mine, sc.oracle_depth_stages(oracle, "defaults"))
    for i, due in ((1, True), (2, False), (5, True)):
        what = "%s: updateKeyframe with frame %d (%s for Frame::setDepth)" % (name, i, "due" if due else "not due")
        if due:
            kfo.set_counters(7, 3, 3, 0)
            kfg.setCounters(7, 3, 3, 0)
        assert kfg.stats()["depthHasBeenUpdatedFlag"] == (0 if due else 1)
        uo, ug = _ref_frames(oracle, hip, ctx, frames, K, gt, kfo, kfg, [i], seed=i)
        dmo.update(uo)
        dmg.updateKeyframe(ug)
        assert_hyp_equal(dmg.currentDepthMap(), dmo.get(), what)
        for lvl in range(5):
            assert_bit_equal(kfg.idepth(lvl), kfo.plane("idepth", lvl), what + " keyframe idepth L%d" % lvl)
            assert_bit_equal(kfg.idepthVar(lvl), kfo.plane("idepthVar", lvl), what + " keyframe idepthVar L%d" % lvl)
    hyp0 = dmo.get()
    for use_mask in (True, False):
        what = "%s: createKeyFrame %s a mask" % (name, "with" if use_mask else "without")
        dmo.set(kfo, hyp0)
        dmg.setCurrentDepthMap(kfg, hyp0)
        no, ng = _ref_frames(oracle, hip, ctx, frames, K, gt, kfo, kfg, [7], with_masks=use_mask)
        dmo.stage("propagate", no)
        pre = oracle_prerescale_after_propagate(dmo)
        dmo.set(kfo, hyp0)
        s_o = dmo.create_keyframe(no[0])
        s_g = dmg.createKeyFrame(ng[0])
        assert_created_keyframe_exact(oracle, what, pre, s_g, s_o, dmg.currentDepthMap(), ng[0], no[0].pose(), K, frames[7])
    dmo.set(kfo, hyp0)
    dmg.setCurrentDepthMap(kfg, hyp0)
    dmo.finalize()
    dmg.finalizeKeyFrame()
    assert_hyp_equal(dmg.currentDepthMap(), dmo.get(), name + ": finalizeKeyFrame")
    for lvl in range(5):
        assert_bit_equal(kfg.idepth(lvl), kfo.plane("idepth", lvl), name + ": finalize idepth L%d" % lvl)
        assert_bit_equal(kfg.idepthVar(lvl), kfo.plane("idepthVar", lvl), name + ": finalize idepthVar L%d" % lvl)


@pytest.mark.parametrize("name", ("defaults",) + sc.CAMERA)
def test_initialize_randomly_at_the_threshold(oracle, hip, name):
    """DepthMap::initializeRandomly takes maxGradients > minUseGrad (DepthMap.cpp:883-916), where every other stage takes >=: a plane with
    entries at the threshold, one ulp below and one ulp above it; both sides draw the same rand() sequence"""
    libc = ctypes.CDLL(None)
    params = sc.params_of(name)
    frames, depth0, K, gt, ctx = make_pair(oracle, hip, W, H, 1, params=params)
    th = ctx.params.minUseGrad
    plane, at, below, above = threshold_plane(th, H, W, 17)
    kfo, kfg = oracle.Frame(0, frames[0], K), hip.Frame(ctx, 0, frames[0])
    kfo.set_maxgrad(plane)
    kfg.setMaxGradients(plane)
    dmo, dmg = oracle.DepthMap(W, H, K, params=oracle_params(oracle, params)), hip.DepthMap(ctx)
    libc.srand(4321)
    dmo.init_random(kfo)
    libc.srand(4321)
    dmg.initializeRandomly(kfg)
    ho = dmo.get()
    inner = interior(H, W, 1)
    assert (at & inner).sum() > 1000 and not ho["isValid"][at].any() and not ho["isValid"][below].any()      # > : not at the threshold
    assert ho["isValid"][above & inner].all()
    assert_hyp_equal(dmg.currentDepthMap(), ho, name + ": initializeRandomly")
    for lvl in range(5):
        assert_bit_equal(kfg.idepth(lvl), kfo.plane("idepth", lvl), "kf idepth L%d" % lvl)
        assert_bit_equal(kfg.idepthVar(lvl), kfo.plane("idepthVar", lvl), "kf idepthVar L%d" % lvl)


# ---------------------------------------------------------------------------------------------------------------
# 3. the depth map, batched
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.CAMERA)
def test_update_batch_both_observe_forms(oracle, hip, name):
    """lsdhip_depth_update_batch against the oracle bit for bit (and so against the single calls, which test_depth_map_single holds to the
    same oracle): 176x144, n = 3 in one launch; 320x240, n = 5 as select + walk — the every-pixel select on the first call (hypotheses
    planted below the PROFILE's threshold, dropped by the call), the candidate select on the second.  update_pair asserts each form
    from lsdhip_ctx_batch_form."""
    params = profile(name)
    db.update_pair(oracle, hip, W, H, 3, py=1, params=params, calls=1)
    forms = db.update_pair(oracle, hip, 320, 240, 5, py=1, params=params)
    assert forms[0]["split"] and not forms[0]["candidates"] and forms[1]["split"] and forms[1]["candidates"], forms


@pytest.mark.parametrize("name", sc.CAMERA)
def test_change_and_reactivate_keyframe_batch(oracle, hip, name):
    """lsdhip_depth_change_keyframe_batch and lsdhip_depth_reactivate_keyframe_batch on three maps: the designed sheets rebuilt for the
    profile's threshold (decisions by class, maps and keyframes against the oracle bit for bit), and the change flow of ragged rendered
    maps (update, change, update behind the change), with three maps and with four"""
    params = profile(name)
    rg.run_change_batch(oracle, hip, W, H, (1, 2, 3), py=1, params=params)
    rg.run_reactivate_batch(oracle, hip, W, H, (5, 0, 2), params=params)
    db.change_flow(oracle, hip, W, H, 3, 1, params=params)
    # four maps: the updates behind each change take the candidate select, on lists that k_maxgrad_candidates_batch built for the new
    # keyframes inside the change (change_round holds those lists to the numpy statement at the profile's threshold)
    db.change_flow(oracle, hip, 320, 240, 4, 1, params=params)


# ---------------------------------------------------------------------------------------------------------------
# 4. the decision sheets at the moved thresholds
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", range(rc.VARIANTS))
@pytest.mark.parametrize("name", sc.CAMERA)
def test_decision_sheets(oracle, hip, name, v):
    """tests/reg_cases.py with 'K5 maxGrad == minUseGrad' and 'K5 maxGrad just below' rebuilt from the profile's value, through
    k_fill_holes and every single-map form of the fused tile"""
    params = profile(name)
    rg.run_stages(oracle, hip, v, params)
    rg.run_update_keyframe_due_and_not_due(oracle, hip, v, params)
    rg.run_finalize_then_set_from_existing(oracle, hip, v, params)
    rg.run_create_keyframe(oracle, hip, v, params)


# ---------------------------------------------------------------------------------------------------------------
# 5. SE3 tracking
# ---------------------------------------------------------------------------------------------------------------
SE3 = [pytest.param(n, a, id="%s-affine%d" % (n, a)) for n in sc.CAMERA for a in (1, 0)]


def hold_se3_form(oracle, hip, scene, n, levels, coarse, want_form):
    stats, seen = {}, set()
    for lvl in levels:
        witness = []
        form = tb.run_batch(oracle, hip, scene, n, lvl, coarse, stats, want_form, witness=witness)
        for fname, job, S, bound in witness[:3]:
            seen.add(fname)
            sc.se3_noise_moves_the_weighted_error(oracle, scene.w, scene.h, scene.K, job, S, bound)
        yield lvl, form
    assert want_form in seen, (want_form, seen)
    print("form %s: worst |device - sum64| / bound = %.3f" % (want_form, stats[want_form]["ratio"]))


@pytest.mark.parametrize("name,affine", SE3)
def test_se3_evaluation_per_entry(oracle, hip, name, affine):
    """the per-entry evaluation of test_track_batch_eval_gpu.py (every summary field against float64 sums of the oracle's float32 terms, at
    that file's bounds, which are relative to the float64 sums of |terms| and so follow the weights' size) in each form: the single
    launch shape of fewer than 8 jobs, the strips, one workgroup per job on coarse levels.  The oracle's weighted error at the default
    noise lies more than 10 x the bound away (settings_cases.se3_noise_moves_the_weighted_error)."""
    params = profile(name, useAffineLightningEstimation=affine)
    small, mid = tb.Scene(oracle, hip, W, H, params), tb.Scene(oracle, hip, 320, 240, params)
    for lvl, form in hold_se3_form(oracle, hip, small, 3, (4, 3, 2, 1), None, "small"):
        assert np.all(form == 0), form
    for lvl, form in hold_se3_form(oracle, hip, mid, 8, (3, 1), 0, "strips"):
        assert np.all(form[:, 0] == 0) and np.all(form[:, 1] >= 1024), form
    for lvl, form in hold_se3_form(oracle, hip, mid, 8, (4, 3, 2), 1, "solo"):
        assert np.all(form[:, 0] == 1), form


@pytest.mark.parametrize("name,affine", SE3)
def test_trackframe_and_permaref(oracle, hip, name, affine):
    """trackFrame at the bars of test_trackframe_parity, trackFrameOnPermaref and checkPermaRefOverlap at those of test_permaref_paths"""
    params = profile(name, useAffineLightningEstimation=affine)
    trackframe_parity(oracle, hip, W, H, params)
    r = run_permaref_paths(oracle, hip, W, H, params)
    # the noise reaches the permaref path: the default-settings oracle ends on another residual
    frames, depth0, K, gt = sequence(W, H, 4)
    kfo = oracle.Frame(0, frames[0], K)
    kfo.set_depth_gt(depth0, minUseGrad=params["minUseGrad"])
    ro = oracle.TrackingReference()
    ro.import_frame(kfo)
    pos, cv, _, _ = ro.pointcloud(4)
    op0 = oracle_params(oracle, {"useAffineLightningEstimation": affine})
    r0 = oracle.SE3Tracker(W, H, K, params=op0, mode=oracle.SSE_EXACT_RCP).track_permaref(pos, cv, oracle.Frame(3, frames[3], K),
                                                                                       oracle.se3_exp(np.array([0.01, 0.0, 0.0, 0, 0, 0.002])))
    assert abs(r0.lastResidual - r.lastResidual) > 0.05 * abs(r.lastResidual), (r0.lastResidual, r.lastResidual)


# ---------------------------------------------------------------------------------------------------------------
# 6. Sim3
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.CAMERA)
def test_sim3_evaluation_per_entry(oracle, hip, name):
    C = s3e.Case(oracle, hip, W, H, 2, 0.8, params=profile(name))
    T = s3e.pose_of(C.P["exp"], "roll")
    tr0 = oracle.Sim3Tracker(W, H, C.P["K"], mode=oracle.SSE_EXACT_RCP)
    worst, levels = {}, []
    for level in range(5):
        r = s3e.evaluate_and_hold(C, T, level, 0.97, 1.5, "%s L%d" % (name, level), worst)
        if r is None:
            continue
        levels.append(level)
        r0 = tr0.evaluate(C.ra, C.fb, T, level, 0.97, 1.5)
        assert abs(r0.sumResP - r[0].sumResP) > 1e-2 * abs(r[0].sumResP), (level, r0.sumResP, r[0].sumResP)     # the noise bites
    assert 4 in levels and 0 in levels, levels
    print("%s: worst |device - sum64| / (EPS sum|terms|) per level %r" % (name, {k: round(v, 1) for k, v in worst.items()}))


@pytest.mark.parametrize("name", sc.CAMERA)
def test_sim3_fused_hessian_and_track(oracle, hip, name):
    """k_sim3_fused: lastSim3Hessian per entry (test_sim3_fused_hessian_per_entry, with the reference's own spread of the affine pair
    behind the system added to the bound: see there), and one whole trackFrameSim3 at the bars of
    test_sim3_track_recovers_pose_and_scale_like_the_oracle (levels 3-1, scale 1.25)"""
    params = profile(name)
    s3e.test_sim3_fused_hessian_per_entry(oracle, hip, 320, 240, 3, 1, params=params, affine_spread=True)
    s3.test_sim3_track_recovers_pose_and_scale_like_the_oracle(oracle, hip, 1.25, params=params, only=("levels 3-1",))


# ---------------------------------------------------------------------------------------------------------------
# 7. the re-position search
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.KF_WEIGHTS)
def test_reposition_search(oracle, hip, name):
    """scenario A of test_reposition_gpu.py on a context with the profile's keyframe weights against reposition_ref.search(..., params=):
    the same candidates behind the prefilter, the same branch per keyframe, the same winner; every score the float32 bits of
    TrackableKeyFrameSearch.h:75-79 at the profile's weights from the record's own distance and usage; getRefFrameScore of the Python
    class the same bits"""
    params = profile(name)
    K, kviews, q = rr.scenario_a_inputs()
    ctx = hip.Context(rr.W, rr.H, K, params=params)
    bank = hip.KeyFrameBank(ctx, len(kviews))
    keep = []
    for i, img, depth, pose in kviews:
        f = hip.Frame(ctx, i, img)
        f.setDepthFromGroundTruth(depth)
        assert bank.put(f, rr.pose8(pose), rr.MEAN_IDEPTH) == len(keep)
        keep.append(f)
    frame, framePose = hip.Frame(ctx, q[0], q[1]), rr.pose8(q[3])
    best, orecs, counts = reposition_search(oracle, name)
    default = reposition_search(oracle, "defaults")
    n_far, n_far0 = assert_weights_bite(name, (best, orecs, counts), default)
    assert_scenario_margins(orecs, counts)      # every deciding quantity clear of its threshold at these weights too
    search = hip.TrackableKeyFrameSearch(ctx, bank)
    slot = search.findRePositionCandidate(frame, framePose, kviews[rr.PARENT_SLOT][0], 1.0)
    res, recs = search.last, search.records()
    stage = {i: n for i, n in enumerate(rr.STAGES)}
    assert slot == best and best is not None
    assert [stage[r.stage] for r in recs] == [o["stage"] for o in orecs]
    assert [r.slot for r in recs if stage[r.stage] != "far"] == [o["slot"] for o in orecs if o["stage"] != "far"]
    assert (res.numPotential, res.numChecked, res.numTracked) == (counts["potential"], counts["checked"], counts["tracked"])
    assert res.numPotential != default[2]["potential"] or name == "ros"
    if name == "kf-dist-zero":
        assert all(stage[r.stage] != "far" for r in recs) and len(recs) == len(kviews)
    wd, wu = f32(ctx.params.KFDistWeight), f32(ctx.params.KFUsageWeight)
    bits = lambda x: int(np.array([x], np.float32).view(np.uint32)[0])
    scored = 0
    for r, o in zip(recs, orecs):
        assert r.dist2 == pytest.approx(float(o["dist2"]), rel=1e-5)
        if "usage" in o:
            assert r.usage == pytest.approx(float(o["usage"]), rel=1e-5), r.slot
            assert r.score == pytest.approx(float(o["score"]), rel=1e-4), r.slot
            assert bits(r.score) == bits(rr.score(r.dist2, r.usage, wd, wu)), (r.slot, r.score)
            assert bits(search.getRefFrameScore(r.dist2, r.usage)) == bits(r.score), r.slot
            scored += 1
        if "tracked" in o:
            dt, dr = pose_distance(np.array(r.refToFrame_tracked), o["tracked"], oracle)
            assert max(dt, dr) < 2e-3, (r.slot, dt, dr)
            assert bool(r.trackingWasGood) == o["trackingWasGood"] and bool(r.diverged) == o["diverged"]
            assert r.newScore == pytest.approx(float(o["newScore"]), rel=1e-3), r.slot
    assert scored >= 5
    assert res.bestScore == recs[best].score


# ---------------------------------------------------------------------------------------------------------------
# 8. one short loop: the settings survive a keyframe change
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("ros", "noisy-camera"))
def test_short_loop(oracle, hip, name):
    """12 frames at 160x128 with a keyframe change every 5: trackFrame -> updateKeyframe -> finalizeKeyFrame + createKeyFrame, each side
    feeding its own results forward, at the bars of test_sequence_gpu.py"""
    w, h, n = 160, 128, 12
    params = profile(name)
    frames, depth0, K, gt = sequence(w, h, n)
    op = oracle_params(oracle, params)
    o_sse = sl.run_oracle(oracle, frames, depth0, K, n, kf_every=5, mode=oracle.SSE, params=op)
    o_sc = sl.run_oracle(oracle, frames, depth0, K, n, kf_every=5, mode=oracle.SCALAR, params=op)
    g = sl.run_hip(hip, hip.Context(w, h, K, params=params), frames, depth0, n, kf_every=5)
    compare_loops(g, o_sse, o_sc, gt, affine_on=params.get("useAffineLightningEstimation", 1) != 0, n_frames=n, kf_frames=(5, 10))
    if name == "noisy-camera":      # the settings bite in the loop: the default-settings oracle maps other pixels
        o_def = sl.run_oracle(oracle, frames, depth0, K, n, kf_every=5, mode=oracle.SSE)
        assert sc.differs(o_def.final_map, o_sse.final_map)["isValid"] >= sc.MIN_VALIDITY_FLAGS
