"""The batched mapping path (lsdhip_depth_update_batch, lsdhip_depth_change_keyframe_batch: what SlamLoopBatch runs) against the CPU
oracle, per pixel and bit for bit, from ragged states: holes, both blacklist values, random validity counters, scheduled skips, planted
hypotheses on pixels below minUseGrad, explicit poses (ground truth composed with a general twist) and explicit masks, so that no
tracker result enters and both sides see identical inputs.  Every case asserts, through lsdhip_ctx_batch_form, the form of the launches
it is there for (one observe launch / select + walk, every-pixel or candidate select, PY of the regulariser tiles, nSet, queue chunks).

Each flow computes the oracle's side first and asserts from the oracle alone that the case has power (pixels changed per map, planted
low-gradient hypotheses present before / absent after, both far-scene settings differ, zoom-out sources per target); run with
dev = None the flows do only that, without a GPU.

The keyframe change is held to the oracle's PRE-rescale map: the factor must be float32(N) / float32(S64) with S64 the float64 sum of
the oracle's pre-rescale idepth_smoothed (test_gpu_parity.expected_rescale), the planes pre * f and pre * (f * f) in float32."""
import concurrent.futures as cf

import numpy as np
import pytest

from common import assert_bit_equal, sequence
from test_gpu_parity import (STEREO, _noisy_hyp, _ref_pose, assert_created_keyframe_exact, assert_gradient_candidates, assert_hyp_equal,
                             expected_rescale, oracle_params, oracle_prerescale_after_propagate)

pytestmark = pytest.mark.gpu

MIN_USE_GRAD = 5.0          # lsdhip_default_params
N_FRAMES = 8
FLOAT_PLANES = ("idepth", "idepth_smoothed", "idepth_var", "idepth_var_smoothed")
PLANES = ("isValid", "blacklisted", "nextStereoFrameMinID", "validity_counter") + FLOAT_PLANES
POOL = cf.ThreadPoolExecutor(max_workers=16)     # the oracle's calls release the GIL; its own pools stay off (threads=1)


@pytest.fixture(scope="module")
def hip():
    import lsd_slam_amd as la
    return la


class Twin:
    """one sequence's oracle side: images, current keyframe (frame index `base`), depth map; `dev` = {"kf", "dm"} on the device"""


def interior(h, w, b=3):
    m = np.zeros((h, w), bool)
    m[b:h - b, b:w - b] = True
    return m


def low_grad_valid(hyp, maxgrad, min_use_grad=MIN_USE_GRAD):
    """valid hypotheses on pixels the observe pass would drop (inside the 3-pixel border, maxGradients below minUseGrad)"""
    return int(((hyp["isValid"] > 0) & (maxgrad < np.float32(min_use_grad)) & interior(*hyp.shape)).sum())


def changed_pixels(a, b):
    d = np.zeros(a.shape, bool)
    for k in PLANES:
        d |= a[k] != b[k]
    return int(d.sum())


def build_twins(oracle, w, h, n, kind="S1", params=None, seed0=100, sigma=0.1, far=False, reactivated=(), regularize=False, nseq=4,
                nframes=N_FRAMES, source=sequence):
    """n ragged oracle maps (test_gpu_parity._noisy_hyp with a per-map seed) on keyframes of `nseq` rendered sequences, plus hypotheses
    planted on 2 % of the pixels below minUseGrad (initializeFromGTDepth leaves none there: without them nothing would tell an
    every-pixel select pass, which drops them, from the candidate select, which never sees them).  source: common.sequence or another
    callable with its arguments and results (tests/test_observe_motions_gpu.py: frames of general camera motions)."""
    op = oracle_params(oracle, params)
    th = np.float32(op.minUseGrad)
    for s in range(min(n, nseq)):
        source(w, h, nframes, s, kind)      # (rendered once per size, before the pool asks for them)

    def one(j):
        t = Twin()
        t.frames, t.depth0, t.K, t.gt = source(w, h, nframes, j % nseq, kind)
        t.w, t.h, t.base, t.react, t.op = w, h, 0, j in reactivated, op
        t.kf = oracle.Frame(0, t.frames[0], t.K)
        t.kf.set_depth_gt(t.depth0, minUseGrad=op.minUseGrad)
        t.dm = oracle.DepthMap(w, h, t.K, params=op, threads=1)
        t.dm.init_gt(t.kf)
        hyp = _noisy_hyp(t.dm.get(), sigma, seed0 + j)
        if far:       # the construction of test_observe_far_scene_negative_idepths: a prior 50x too far
            for k in ("idepth", "idepth_smoothed"):
                hyp[k] *= np.float32(0.02)
            for k in ("idepth_var", "idepth_var_smoothed"):
                hyp[k] *= np.float32(0.02 * 0.02)
        rng = np.random.default_rng(7000 + seed0 + j)
        mg = t.kf.plane("maxGradients", 0)
        plant = (mg < th) & (rng.uniform(size=mg.shape) < 0.02) & interior(h, w) & np.isfinite(t.depth0) & (t.depth0 > 0)
        idp = (np.float32(1) / np.where(plant, t.depth0, np.float32(1))).astype(np.float32)
        hyp["isValid"][plant] = 1
        hyp["blacklisted"][plant] = 0
        hyp["validity_counter"][plant] = 20
        hyp["nextStereoFrameMinID"][plant] = 0
        for k in ("idepth", "idepth_smoothed"):
            hyp[k][plant] = idp[plant]
        for k in ("idepth_var", "idepth_var_smoothed"):
            hyp[k][plant] = np.float32(sigma * sigma)
        t.dm.set(t.kf, hyp, reactivated=t.react)
        if regularize:
            t.dm.stage("regularize")
            hyp = t.dm.get()
        t.planted = low_grad_valid(hyp, mg, th)
        assert t.planted > 0, "map %d: no hypothesis below minUseGrad in the uploaded state" % j
        t.hyp0 = hyp
        t.dev = None
        return t

    return list(POOL.map(one, range(n)))


def fresh_map(oracle, t, kf, hyp, reactivated=False):
    """a new oracle map standing on keyframe `kf` with the state `hyp` (initializeFromGTDepth on empty planes first: it is what makes the map
    cache the keyframe's image, which a raw overwrite alone does not)"""
    none = np.full((t.h, t.w), -1, np.float32)
    kf.set_depth_planes(none, none)
    dm = oracle.DepthMap(t.w, t.h, t.K, params=t.op, threads=1)
    dm.init_gt(kf)
    dm.set(kf, hyp, reactivated=reactivated)
    return dm


def upload_twins(hip, ctx, twins):
    for t in twins:
        kfg = hip.Frame(ctx, 0, t.frames[0])
        kfg.setDepthFromGroundTruth(t.depth0)
        dmg = hip.DepthMap(ctx)
        dmg.setCurrentDepthMap(kfg, t.hyp0, reactivated=t.react)
        t.dev = {"kf": kfg, "dm": dmg}


def frame_inputs(oracle, t, fid, with_mask, seed, pose=None):
    """(Sim3 pose to the current keyframe, initialTrackedResidual, mask or None) of frame `fid` of the twin's sequence"""
    sim3, itr = _ref_pose(oracle, t.gt, fid, base=t.base if t.base else None)
    if pose is not None:
        sim3 = pose
    m = None
    if with_mask:
        m = (np.random.default_rng(seed).uniform(size=(t.h >> 1, t.w >> 1)) < 0.9).astype(np.uint8)
    return sim3, itr, m


def oracle_frame(oracle, t, fid, inp, parent):
    fo = oracle.Frame(fid, t.frames[fid], t.K)
    fo.set_pose(inp[0], parent, inp[1])
    if inp[2] is not None:
        fo.set_wasgood(inp[2])
    return fo


def device_frame(hip, ctx, t, fid, inp, parent):
    fg = hip.Frame(ctx, fid, t.frames[fid])
    fg.setPose(inp[0], parent, inp[1])
    if inp[2] is not None:
        fg.set_refPixelWasGood(inp[2])
    return fg


def assert_mean_idepth(stats, plane0, var0, what):
    """numPoints exact; meanIdepth within N * 2^-24 relative of the float64 mean of the level-0 plane (the oracle's own value is a
    sequential float32 sum: not the yardstick)"""
    ok = var0 > 0
    N = int(ok.sum())
    assert int(stats["numPoints"]) == N, (what, stats["numPoints"], N)
    mean64 = float(plane0[ok].astype(np.float64).sum()) / N
    assert abs(stats["meanIdepth"] - mean64) <= N * 2.0 ** -24 * abs(mean64), (what, stats["meanIdepth"], mean64)


def assert_form(ctx, which, want, what):
    got = ctx.batchForm(which)
    for k, v in want.items():
        assert got[k] == v, "%s: the call ran another form than the case is there for: %s = %r, expected %r (%r)" % (what, k, got[k], v, got)
    return got


def update_round(oracle, hip, ctx, twins, fids, what, masks=None, due=None, form=None, expect_low_grad=None, min_changed=1000):
    """one updateKeyframeBatch over `twins` with frame fids[j] each; due[j]: the keyframe is due for Frame::setDepth.  Oracle first (and the
    power conditions from it alone), then — with a context — the device call and the comparison of everything the call leaves."""
    n = len(twins)
    masks = masks or [True] * n
    due = due or [True] * n
    inputs = [frame_inputs(oracle, t, fids[j], masks[j], 31 * fids[j] + j) for j, t in enumerate(twins)]
    before = [t.dm.get() for t in twins]
    mgs = [t.kf.plane("maxGradients", 0) for t in twins]
    low = [low_grad_valid(before[j], mgs[j], twins[j].op.minUseGrad) for j in range(n)]
    if expect_low_grad is True:
        assert all(v > 0 for v in low), (what, low)
    if expect_low_grad is False:     # a candidate-select call: nothing below the threshold is left, and only because an earlier pass removed it
        assert all(v == 0 for v in low), "%s: valid hypotheses below minUseGrad before a candidate-select call: %r" % (what, low)
        assert all(t.planted > 0 for t in twins), what
    fos = []
    for j, t in enumerate(twins):
        t.kf.set_counters(7, 3, 3, not due[j])
        fos.append(oracle_frame(oracle, t, fids[j], inputs[j], t.kf))
    list(POOL.map(lambda j: twins[j].dm.update([fos[j]]), range(n)))
    after = [t.dm.get() for t in twins]
    for j in range(n):
        ch = changed_pixels(before[j], after[j])
        assert ch >= min_changed, "%s map %d: the update changed %d pixels only" % (what, j, ch)
    if ctx is None:
        return after
    fgs, pyr0 = [], []
    for j, t in enumerate(twins):
        kfg = t.dev["kf"]
        kfg.setCounters(7, 3, 3, not due[j])
        fgs.append(device_frame(hip, ctx, t, fids[j], inputs[j], kfg))
        pyr0.append(None if due[j] else [(kfg.idepth(l), kfg.idepthVar(l)) for l in range(5)])
    hip.DepthMap.updateKeyframeBatch([t.dev["dm"] for t in twins], fgs)
    want = {"n": n, "nSet": int(sum(due))}
    want.update(form or {})
    got = assert_form(ctx, "update", want, what)
    if got["split"]:
        assert got["queued"] >= 0 and got["walkWorkgroups"] > 0 and got["chunks"] == int(((got["queueCounts"] + 63) // 64).sum()), (what, got)
    for j, t in enumerate(twins):
        tag = "%s map %d" % (what, j)
        kfg, kfo = t.dev["kf"], t.kf
        assert_hyp_equal(t.dev["dm"].currentDepthMap(), after[j], tag)
        so, sg = kfo.stats(), kfg.stats()
        assert sg["depthHasBeenUpdatedFlag"] == so["depthHasBeenUpdatedFlag"] == 1, tag
        assert sg["numMappedOnThis"] == so["numMappedOnThis"] == 4 and sg["numMappedOnThisTotal"] == so["numMappedOnThisTotal"] == 4, tag
        for lvl in range(5):
            if due[j]:
                assert_bit_equal(kfg.idepth(lvl), kfo.plane("idepth", lvl), tag + " keyframe idepth L%d" % lvl)
                assert_bit_equal(kfg.idepthVar(lvl), kfo.plane("idepthVar", lvl), tag + " keyframe idepthVar L%d" % lvl)
            else:
                assert_bit_equal(kfg.idepth(lvl), pyr0[j][lvl][0], tag + " keyframe idepth L%d (not due: untouched)" % lvl)
                assert_bit_equal(kfg.idepthVar(lvl), pyr0[j][lvl][1], tag + " keyframe idepthVar L%d (not due: untouched)" % lvl)
        if due[j]:
            assert_mean_idepth(sg, kfo.plane("idepth", 0), kfo.plane("idepthVar", 0), tag)
    return got


# ---------------------------------------------------------------------------------------------------------------
# updateKeyframeBatch
# ---------------------------------------------------------------------------------------------------------------
SPLIT_ALL = {"split": True, "candidates": False}      # select + walk, every-pixel select (a map of the call may hold a low-gradient hypothesis)
SPLIT_CAND = {"split": True, "candidates": True}
ONE_LAUNCH = {"split": False, "candidates": False, "walkWorkgroups": 0}


def update_pair(oracle, hip, w, h, n, py, params=None, kind="S1", calls=2, nseq=4, nframes=N_FRAMES, extra=None, dev=True):
    """first call after upload (lowGradHypPossible: every-pixel select from 4 maps on), second call with the next frame (candidate select);
    frame ids 3 and 5 lie on both sides of the nextStereoFrameMinID = 4.0 that _noisy_hyp plants"""
    twins = build_twins(oracle, w, h, n, kind=kind, params=params, nseq=nseq, nframes=nframes)
    ctx = None
    if dev:
        ctx = hip.Context(w, h, twins[0].K, params=params)
        upload_twins(hip, ctx, twins)
    split = 4 <= n <= 256
    out = []
    for call, fid in enumerate((3, 5)[:calls]):
        form = dict(ONE_LAUNCH if not split else (SPLIT_ALL if call == 0 else SPLIT_CAND), py=py)
        got = update_round(oracle, hip, ctx, twins, [fid] * n, "%dx%d n=%d call %d" % (w, h, n, call), form=form,
                           expect_low_grad=(call == 0) if split else None)
        if dev and extra:
            extra(call, got)
        out.append(got)
    return out


@pytest.mark.parametrize("n", [1, 2, 3])
def test_update_batch_one_launch_form(oracle, hip, n):
    """fewer than LSD_OBS_SPLIT_MIN_MAPS maps: k_observe_batch<2>, PY = 1; 176 = 2.75 select tiles, 5.5 regulariser tiles"""
    update_pair(oracle, hip, 176, 144, n, py=1)


@pytest.mark.parametrize("params", STEREO)
def test_update_batch_split_then_candidates(oracle, hip, params):
    """320x240, n = 5: every-pixel select on the first call after upload, candidate select on the second — under each STEREO switch set"""
    update_pair(oracle, hip, 320, 240, 5, py=1, params=params)


@pytest.mark.parametrize("nset", ["none", "mixed", "all"])
def test_update_batch_falls_back_when_one_map_is_fresh(oracle, hip, nset, dev=True):
    """320x240, n = 6: three maps updated once before (they would qualify for the candidate lists), three freshly uploaded — the whole call
    takes the every-pixel select, and the planted low-gradient hypotheses of the fresh maps are dropped.  nSet = 0 / 3 / 6: no keyframe, some,
    all due for Frame::setDepth (k_reg_fused_batch<false> alone, both twins in one call, <true> alone)."""
    w, h, n = 320, 240, 6
    twins = build_twins(oracle, w, h, n)
    ctx = None
    if dev:
        ctx = hip.Context(w, h, twins[0].K)
        upload_twins(hip, ctx, twins)
    update_round(oracle, hip, ctx, twins[:3], [3] * 3, "n=6 fallback: first update of maps 0..2", form=dict(ONE_LAUNCH, py=1))
    due = {"none": [False] * 6, "mixed": [True, False, True, False, True, False], "all": [True] * 6}[nset]
    update_round(oracle, hip, ctx, twins, [5] * 6, "n=6 fallback (nSet %s)" % nset, due=due, form=dict(SPLIT_ALL, py=1))
    # the fallback row tests something: the fresh maps held low-gradient hypotheses (counted in build_twins), the call removed them
    for t in twins[3:]:
        assert t.planted > 0 and low_grad_valid(t.dm.get(), t.kf.plane("maxGradients", 0)) == 0


def test_update_batch_py2_partial_select_tile_and_candidate_group(oracle, hip):
    """176x144, n = 24: 6 x 18 x 24 = 2592 workgroups -> PY = 2; 176 = 2.75 select tiles; 25 344 px = 24.75 candidate groups"""
    assert (176 * 144) % 1024 != 0 and 176 % 64 != 0
    update_pair(oracle, hip, 176, 144, 24, py=2)


def test_update_batch_py2_width_656(oracle, hip):
    """656x496, n = 4: 10.25 select tiles, 20.5 regulariser tiles, 21 x 62 x 4 workgroups -> PY = 2"""
    update_pair(oracle, hip, 656, 496, 4, py=2)


def test_update_batch_benchmark_size_more_chunks_than_walk_workgroups(oracle, hip):
    """640x480, n = 16: PY = 2 at the benchmark size, and the queues hold more 64-entry chunks than the walk launch has workgroups (second
    trip of its grid-stride loop)"""
    def extra(call, got):
        print("640x480 n=16 call %d: %d entries queued, %d chunks, %d walk workgroups" % (call, got["queued"], got["chunks"], got["walkWorkgroups"]))
        assert got["chunks"] > got["walkWorkgroups"], got
    update_pair(oracle, hip, 640, 480, 16, py=2, extra=extra)


def test_update_batch_maps_beyond_the_first_scan_chunk(oracle, hip):
    """160x128, n = 70: maps 64.. sit in the second 64-lane chunk of the walk kernel's s_incl scan"""
    def extra(call, got):
        assert int((got["queueCounts"][64:] > 0).sum()) == 6 and int((got["queueCounts"][:64] > 0).sum()) == 64, got
    update_pair(oracle, hip, 160, 128, 70, py=2, calls=1, extra=extra)


@pytest.mark.parametrize("n", [256, 257])
def test_update_batch_walk_max_maps_edge(oracle, hip, n):
    """160x128, n = 256 (LSD_OBS_WALK_MAX_MAPS: still select + walk, every s_incl slot in use) and n = 257 (one launch again)"""
    def extra(call, got):
        if n == 256:
            assert int((got["queueCounts"] > 0).sum()) == 256, got
    update_pair(oracle, hip, 160, 128, n, py=2, calls=1, extra=extra)


def test_update_batch_per_map_switches(oracle, hip, dev=True):
    """one 320x240, n = 6 call: maps 1 and 4 re-activated (no scheduled skips), frames of maps 2 and 4 without a mask, frame ids 2, 3 (before)
    and 5, 6 (behind the planted nextStereoFrameMinID = 4.0)"""
    w, h, n = 320, 240, 6
    twins = build_twins(oracle, w, h, n, reactivated=(1, 4), seed0=300)
    ctx = None
    if dev:
        ctx = hip.Context(w, h, twins[0].K)
        upload_twins(hip, ctx, twins)
    update_round(oracle, hip, ctx, twins, [2, 3, 5, 6, 3, 5], "per-map switches", masks=[True, True, False, True, False, True],
                 form=dict(SPLIT_ALL, py=1))


@pytest.mark.parametrize("allow", [1, 0])
def test_update_batch_far_scene_negative_idepths(oracle, hip, allow, dev=True):
    """the far-scene construction of test_observe_far_scene_negative_idepths as a batch of 4: both settings bit-exact, and the two settings
    differ on more than 50 pixels of every map (the branch is taken)"""
    w, h, n = 320, 240, 4
    res = {}
    for a in (allow, 1 - allow):
        params = {"allowNegativeIdepths": a}
        twins = build_twins(oracle, w, h, n, params=params, far=True, seed0=500)
        ctx = None
        if dev and a == allow:
            ctx = hip.Context(w, h, twins[0].K, params=params)
            upload_twins(hip, ctx, twins)
        update_round(oracle, hip, ctx, twins, [7] * n, "far scene allowNegativeIdepths=%d" % a, form=dict(SPLIT_ALL, py=1))
        res[a] = [t.dm.get() for t in twins]
    for j in range(n):
        d = int((res[0][j]["validity_counter"] != res[1][j]["validity_counter"]).sum())
        assert d > 50, "map %d: the negative-idepth branch was not exercised (%d pixels differ)" % (j, d)


def test_update_batch_1280x1024(oracle, hip):
    """1280x1024, scene S2, n = 4, one call (a single map is PY = 2 there already)"""
    update_pair(oracle, hip, 1280, 1024, 4, py=2, kind="S2", calls=1, nseq=2, nframes=4)


# ---------------------------------------------------------------------------------------------------------------
# changeKeyframeBatch
# ---------------------------------------------------------------------------------------------------------------
def change_round(oracle, hip, ctx, twins, nk, what, masks, change_py, zoom_out=(), poses=None):
    """finalizeKeyFrame + createKeyFrame(frame nk of each sequence; a list: frame nk[j] for map j) of every twin.  poses[j], where given,
    is map j's Sim3 new keyframe -> old keyframe instead of the sequence's own.  Oracle per map: A = finalize, then propagate,
    regularize_occ, fillholes, regularize -> the pre-rescale map; B = finalize + create_keyframe from the same start -> its own factor and
    pose.  Afterwards the twins stand on the new keyframes with the map the device must hold (pre-rescale map times the device's factor)."""
    n = len(twins)
    nks = [int(nk)] * n if np.isscalar(nk) else [int(v) for v in nk]
    poses = list(poses) if poses is not None else [None] * n
    start = [t.dm.get() for t in twins]
    back = np.concatenate([oracle.se3_exp(np.array([0.0, 0.0, -3.5, 0.0, 0.0, 0.0])), [1.0]])   # camera 3.5 depth units behind: image shrinks ~2.7x
    inputs = [frame_inputs(oracle, t, nks[j], masks[j], 977 * nks[j] + j, pose=back if j in zoom_out else poses[j]) for j, t in enumerate(twins)]

    def one(j):
        t, r = twins[j], {}
        img = t.frames[t.base]
        kfA, kfB = oracle.Frame(t.base, img, t.K), oracle.Frame(t.base, img, t.K)
        dmA, dmB = fresh_map(oracle, t, kfA, start[j], t.react), fresh_map(oracle, t, kfB, start[j], t.react)
        dmA.finalize()
        dmB.finalize()
        r["fin"] = dmA.get()
        r["old"] = kfA
        dmR = oracle.DepthMap(t.w, t.h, t.K, params=t.op, threads=1)
        dmR.set_from_existing(kfA)
        r["react"] = dmR.get()
        nkA, nkB = oracle_frame(oracle, t, nks[j], inputs[j], kfA), oracle_frame(oracle, t, nks[j], inputs[j], kfB)
        dmA.stage("propagate", [nkA])
        r["prop"] = dmA.get()
        r["n_src"], r["n_dst"] = int((r["fin"]["isValid"] > 0).sum()), int((r["prop"]["isValid"] > 0).sum())
        r["pre"] = oracle_prerescale_after_propagate(dmA)
        r["s_o"] = dmB.create_keyframe(nkB)
        r["pose_o"] = nkB.pose()
        r["keep"] = (kfA, kfB, nkA, nkB, dmA, dmB)
        return r

    res = list(POOL.map(one, range(n)))
    for j in zoom_out:
        assert res[j]["n_dst"] > 1000 and res[j]["n_src"] > 8 * res[j]["n_dst"], (what, j, res[j]["n_src"], res[j]["n_dst"])   # overflow chains in use
    scales = None
    if ctx is not None:
        olds = [t.dev["kf"] for t in twins]
        nkgs = [device_frame(hip, ctx, t, nks[j], inputs[j], t.dev["kf"]) for j, t in enumerate(twins)]
        scales = hip.DepthMap.changeKeyframeBatch([t.dev["dm"] for t in twins], nkgs)
        assert_form(ctx, "change", {"n": n} if change_py is None else {"n": n, "py": change_py}, what)
    for j, t in enumerate(twins):
        tag, r = "%s map %d" % (what, j), res[j]
        pre = r["pre"]
        if ctx is not None:
            # the old keyframe: finalizeKeyFrame's map (through its re-activation data), Frame::setDepth's pyramids and statistics
            m2 = hip.DepthMap(ctx)
            m2.setFromExistingKF(olds[j])
            assert_hyp_equal(m2.currentDepthMap(), r["react"], tag + " old keyframe re-activation")
            for lvl in range(5):
                assert_bit_equal(olds[j].idepth(lvl), r["old"].plane("idepth", lvl), tag + " old keyframe idepth L%d" % lvl)
                assert_bit_equal(olds[j].idepthVar(lvl), r["old"].plane("idepthVar", lvl), tag + " old keyframe idepthVar L%d" % lvl)
            assert_mean_idepth(olds[j].stats(), r["old"].plane("idepth", 0), r["old"].plane("idepthVar", 0), tag + " old keyframe")
            want = assert_created_keyframe_exact(oracle, tag, pre, scales[j], r["s_o"], t.dev["dm"].currentDepthMap(), nkgs[j], r["pose_o"], t.K,
                                                 t.frames[nks[j]])
            # the new keyframe's gradient candidates, built with its level-0 planes inside the call (k_maxgrad_candidates, or its batch
            # form from two maps on): the pixels the next candidate-select update may search, at the context's threshold
            assert_gradient_candidates(nkgs[j], t.w, t.h, t.op.minUseGrad)
            t.dev["kf"] = nkgs[j]
            t.dev.setdefault("old", []).append(olds[j])
        else:
            f, _, N = expected_rescale(pre, tag)
            assert abs(float(r["s_o"]) - float(f)) <= N * 2.0 ** -24 * float(f), (tag, r["s_o"], f)
            f2 = np.float32(f * f)
            want = {k: (pre[k] * (f if "var" not in k else f2)).astype(np.float32) for k in FLOAT_PLANES}
        nxt = pre.copy()
        for k in FLOAT_PLANES:
            nxt[k] = want[k]
        t.base, t.react = nks[j], False
        t.kf = oracle.Frame(nks[j], t.frames[nks[j]], t.K)
        t.dm = fresh_map(oracle, t, t.kf, nxt)
    return res


def change_flow(oracle, hip, w, h, n, py, zoom_out=(), mixed_masks=True, dev=True, min_changed=1000, change_py="same", params=None):
    """update with frame 1, change to frame 2, update with frame 3, change to frame 4 (starts from the propagation scratch the first left), update with frame 5.
    From 4 maps on the updates behind a change take the candidate select on lists built for the NEW keyframes while lowGradHypPossible is
    still false: the oracle's new map must hold no hypothesis below minUseGrad then (asserted from the oracle), and the device must agree
    bit for bit."""
    twins = build_twins(oracle, w, h, n, sigma=0.03, regularize=True, seed0=900, params=params)
    ctx = None
    if dev:
        ctx = hip.Context(w, h, twins[0].K, params=params)
        upload_twins(hip, ctx, twins)
    masks = [(j % 2 == 0) or not mixed_masks for j in range(n)]
    split = 4 <= n <= 256
    # (as in the loop: an update has run on the uploaded maps before their first change — it is what clears lowGradHypPossible)
    update_round(oracle, hip, ctx, twins, [1] * n, "%dx%d n=%d update before the first change" % (w, h, n),
                 form=dict(SPLIT_ALL if split else ONE_LAUNCH, py=py), expect_low_grad=True if split else None, min_changed=min_changed)
    for rnd, (nk, zo) in enumerate(((2, zoom_out), (4, ()))):
        change_round(oracle, hip, ctx, twins, nk, "%dx%d n=%d change %d" % (w, h, n, rnd), masks, py if change_py == "same" else change_py, zoom_out=zo)
        form = dict(SPLIT_CAND if split else ONE_LAUNCH, py=py)
        update_round(oracle, hip, ctx, twins, [nk + 1] * n, "%dx%d n=%d update behind change %d" % (w, h, n, rnd), form=form,
                     expect_low_grad=False if split else None, min_changed=min_changed)
        masks = [not m for m in masks] if mixed_masks else masks


@pytest.mark.parametrize("n,py,zoom_out", [(1, 1, ()), (3, 1, (1,)), (8, 2, (5,))])
def test_change_keyframe_batch_320x240(oracle, hip, n, py, zoom_out):
    """320x240: n = 1 and 3 (PY = 1), n = 8 (2400 workgroups: PY = 2); masks on and off within one call; one map in the zoom-out pose of
    test_propagate_zoom_out_more_sources_than_slots among ordinary ones (overflow chains inside the fused finalize + phase A launch)"""
    change_flow(oracle, hip, 320, 240, n, py, zoom_out=zoom_out)


def test_change_keyframe_batch_176x144_n24(oracle, hip):
    change_flow(oracle, hip, 176, 144, 24, 2)


@pytest.mark.parametrize("n", [2, 8])
def test_change_keyframe_batch_640x480(oracle, hip, n):
    """640x480, n = 2 (20 x 60 x 2 = 2400 workgroups: PY = 2 already) and n = 8"""
    change_flow(oracle, hip, 640, 480, n, 2)


def test_change_keyframe_batch_more_maps_than_result_slots(oracle, hip):
    """160x128, n = 100: three deferred-result slots per map against the context's ring of 256 — the call goes in parts of at most 85 maps
    (the ring used to wrap inside the call: the first maps read a rescale factor and statistics that nothing had written yet)"""
    change_flow(oracle, hip, 160, 128, 100, 2, change_py=None)


def test_batch_form_query_reports_unavailable_counts(oracle, hip):
    """lsdhip_ctx_batch_form: nothing before the first call; after a split call on an asynchronous context the queue counts are withheld"""
    w, h, n = 160, 128, 4
    twins = build_twins(oracle, w, h, n)
    ctx = hip.Context(w, h, twins[0].K)
    assert ctx.batchForm("update")["n"] == 0 and ctx.batchForm("change")["n"] == 0
    upload_twins(hip, ctx, twins)
    ctx.set_async(True)
    fgs = [device_frame(hip, ctx, t, 3, frame_inputs(oracle, t, 3, True, j), t.dev["kf"]) for j, t in enumerate(twins)]
    hip.DepthMap.updateKeyframeBatch([t.dev["dm"] for t in twins], fgs)
    got = ctx.batchForm("update")
    ctx.synchronize()
    ctx.set_async(False)
    assert got["n"] == n and got["split"] and got["queued"] == -1 and got["chunks"] == -1 and got["queueCounts"] is None, got


def test_observe_work_of_one_update_counts_what_the_split_call_queues(oracle, hip):
    """176x144, a synchronous context under lsdhip_prof_enable: one lsdhip_depth_update with one reference frame is sampled, so k_observe<true, 2>
    counts its searches and walk steps per wave (observe_count) and k_obs_count_sum adds them up behind it — the path that only the benchmark
    reads.  The search count is held to the queue count of a map in the same state that a 4-map select + walk call updates with the same
    frame: both count the pixels that pass the front half's tests."""
    from lsd_slam_amd import capi
    w, h, n = 176, 144, 4
    twins = build_twins(oracle, w, h, n)
    ctx = hip.Context(w, h, twins[0].K)
    upload_twins(hip, ctx, twins)
    t = twins[0]
    inputs = [frame_inputs(oracle, tj, 3, True, 31 * 3 + j) for j, tj in enumerate(twins)]
    kf1 = hip.Frame(ctx, 0, t.frames[0])
    kf1.setDepthFromGroundTruth(t.depth0)
    dm1 = hip.DepthMap(ctx)
    dm1.setCurrentDepthMap(kf1, t.hyp0, reactivated=t.react)
    ctx.prof_enable(True)
    dm1.updateKeyframe([device_frame(hip, ctx, t, 3, inputs[0], kf1)])
    ctx.prof_enable(False)
    work = np.zeros(3, np.float64)
    capi.check(dm1.L.lsdhip_depth_observe_work(dm1.h_, work.ctypes.data))
    fgs = [device_frame(hip, ctx, tj, 3, inputs[j], tj.dev["kf"]) for j, tj in enumerate(twins)]
    hip.DepthMap.updateKeyframeBatch([tj.dev["dm"] for tj in twins], fgs)
    got = assert_form(ctx, "update", dict(SPLIT_ALL, n=n), "observe work")
    print("observe work: launches %d, searches %d, walk steps %d; queue counts %r" % (work[0], work[1], work[2], got["queueCounts"][:n]))
    assert work[0] == 1, work
    assert got["queueCounts"][0] > 0 and work[1] == got["queueCounts"][0], (work, got)
    assert work[2] > 0, work
