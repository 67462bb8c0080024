"""The designed sheet of tests/reg_cases.py through every entry of liblsdhip.so that hosts fill-holes (k_fill_holes) and the fused
regulariser tile (reg_fused_tile): each entry is compared with the CPU oracle the way the existing test of that entry compares (the map
with assert_hyp_equal, the keyframe's five idepth / idepthVar levels bit for bit, numPoints and the mean inverse depth, the re-activation
planes where the entry writes them).  Ahead of each such comparison the device's per-pixel DECISIONS are held to reg_cases.census class by
class, so that a wrong decision is reported as "class 'K5 sum=100 bl=-2' at x%32=31" instead of a pixel index.  tests/test_reg_cases_cpu.py proves on the CPU that the sheet reaches
the classes it claims and that the oracle equals the compiled reference on it.

The observe stage is not under test: the update calls get a tracked frame whose refPixelWasGood mask is all zero, and every hypothesis of
the sheet sits on a pixel above minUseGrad, so observeDepth changes nothing on either side."""
import ctypes as C

import numpy as np
import pytest

import reg_cases as rc
from common import assert_bit_equal
from test_depth_batch_gpu import assert_form, assert_mean_idepth
from test_gpu_parity import assert_created_keyframe_exact, assert_hyp_equal, oracle_prerescale_after_propagate
from test_reg_cases_cpu import IDENT8, Side, camera, image

pytestmark = pytest.mark.gpu
W, H = 176, 144          # 5 1/2 tiles wide (a partial last tile column), 18 tile rows of 8
VARIANTS = list(range(rc.VARIANTS))
NEW_KF_TWIST = np.array([0.01, -0.008, 0.012, 0.002, -0.0015, 0.001])      # a small general pose: no axis of it is zero


@pytest.fixture(scope="module")
def hip():
    import lsd_slam_amd as la
    return la


def workgroups(w, h, n=1):
    return ((w + 31) // 32) * ((h + 7) // 8) * n


# ---------------------------------------------------------------------------------------------------------------
# the oracle's side, computed once per (size, variant, entry) and shared
# ---------------------------------------------------------------------------------------------------------------
_TRUTH = {}


def truth(oracle, w, h, v, entry, th=rc.MIN_USE_GRAD):
    """th: the minUseGrad the sheet is built for and the oracle's map runs at"""
    key = (w, h, v, entry, float(th))
    if key not in _TRUTH:
        _TRUTH[key] = _compute(oracle, w, h, v, entry, th)
    return _TRUTH[key]


def kf_planes(kf):
    return [(kf.plane("idepth", l), kf.plane("idepthVar", l)) for l in range(5)]


def new_keyframe_inputs(oracle, w, h):
    sim3 = np.concatenate([oracle.se3_exp(NEW_KF_TWIST), [1.0]])
    return image(w, h, 1), sim3, 0.4, np.ones((h >> 1, w >> 1), np.uint8), np.full((h, w), rc.GRAD_HIGH, np.float32)


def oracle_new_keyframe(oracle, side):
    img, sim3, itr, mask, mg = new_keyframe_inputs(oracle, side.w, side.h)
    f = oracle.Frame(1, img, side.K)
    f.set_maxgrad(mg)
    f.set_pose(sim3, side.kf, itr)
    f.set_wasgood(mask)
    return f


def react_sheet(fin):
    """the map setFromExistingKF makes of a finalised map's re-activation planes before its own K6 (DepthMap.cpp:937-958)"""
    hyp = fin.copy()
    v = fin["isValid"] > 0
    hyp["blacklisted"] = np.where(v, 0, np.where(fin["blacklisted"] < rc.MIN_BLACKLIST, rc.MIN_BLACKLIST - 1, 0))
    return hyp


def _compute(oracle, w, h, v, entry, th=rc.MIN_USE_GRAD):
    hyp, mg = rc.build(w, h, v, th)
    moved = None if th == rc.MIN_USE_GRAD else th
    s = Side(oracle, w, h, hyp, mg, min_use_grad=moved)
    r = {"side": s}
    if entry in ("fillholes", "regularize", "regularize_occ"):
        r["map"] = s.run(entry)
    elif entry == "fill_regularize":
        s.run("fillholes")
        r["map"] = s.run("regularize")
    elif entry in ("update_due", "update_not_due"):
        s.kf.set_counters(7, 3, 3, entry == "update_not_due")
        s.dm.update([s.tracked()])
        r["map"], r["planes"], r["stats"] = s.dm.get(), kf_planes(s.kf), s.kf.stats()
    elif entry == "finalize":
        r["map"], r["planes"], r["stats"] = s.run("finalize"), kf_planes(s.kf), s.kf.stats()
        dm2 = oracle.DepthMap(w, h, s.K, params=s.op, threads=1)
        dm2.set_from_existing(s.kf)
        r["react_map"] = dm2.get()
    elif entry == "create":          # createKeyFrame from the sheet: propagate -> pre-rescale map; and the whole call for its factor and pose
        nk = oracle_new_keyframe(oracle, s)
        s.dm.stage("propagate", [nk])
        r["prop"] = s.dm.get()
        r["pre"] = oracle_prerescale_after_propagate(s.dm)
        b = Side(oracle, w, h, hyp, mg, min_use_grad=moved)
        nkb = oracle_new_keyframe(oracle, b)
        r["s_o"], r["pose_o"], r["keep"] = b.dm.create_keyframe(nkb), nkb.pose(), (nk, nkb, b)
    elif entry == "change":          # finalizeKeyFrame + createKeyFrame
        s.run("finalize")
        nk = oracle_new_keyframe(oracle, s)
        s.dm.stage("propagate", [nk])
        r["prop"] = s.dm.get()
        r["pre"] = oracle_prerescale_after_propagate(s.dm)
        b = Side(oracle, w, h, hyp, mg, min_use_grad=moved)
        b.run("finalize")
        nkb = oracle_new_keyframe(oracle, b)
        r["s_o"], r["pose_o"], r["keep"] = b.dm.create_keyframe(nkb), nkb.pose(), (nk, nkb, b)
    else:
        raise KeyError(entry)
    return r


# ---------------------------------------------------------------------------------------------------------------
# the device's side
# ---------------------------------------------------------------------------------------------------------------
class Dev:
    def __init__(self, hip, ctx, w, h, v, kf_id=0):
        self.hip, self.ctx, self.w, self.h, self.v = hip, ctx, w, h, v
        self.th = float(ctx.params.minUseGrad)        # the context's threshold: the sheet and the census follow it
        self.hyp, self.mg = rc.build(w, h, v, self.th)
        self.cells = rc.cells(w, h, v)
        self.kf = hip.Frame(ctx, kf_id, image(w, h))
        self.kf.setMaxGradients(self.mg)
        none = np.full((h, w), -1, np.float32)
        self.kf.setDepthPlanes(none, none)
        self.dm = hip.DepthMap(ctx)
        self.reset()

    def reset(self):
        self.dm.setCurrentDepthMap(self.kf, self.hyp)

    def tracked(self, id_=1):
        f = self.hip.Frame(self.ctx, id_, image(self.w, self.h, id_))
        f.setPose(IDENT8, self.kf, 0.3)
        f.set_refPixelWasGood(np.zeros((self.h >> 1, self.w >> 1), np.uint8))
        return f

    def new_keyframe(self, oracle):
        img, sim3, itr, mask, mg = new_keyframe_inputs(oracle, self.w, self.h)
        f = self.hip.Frame(self.ctx, 1, img)
        f.setMaxGradients(mg)
        f.setPose(sim3, self.kf, itr)
        f.set_refPixelWasGood(mask)
        return f


def context(hip, w, h, params=None):
    ctx = hip.Context(w, h, camera(w, h), params=params)
    assert ctx.params.minUseGrad == np.float32((params or {}).get("minUseGrad", rc.MIN_USE_GRAD))
    return ctx


def check_map(d, got, t, stage, what):
    """the device's decisions against the census of the sheet (first: a wrong decision is then reported by class and position), and its map
    against the oracle's"""
    want = rc.census(d.hyp, d.mg, d.th, stage)
    rc.assert_decisions(rc.decisions_from_maps(d.hyp, got, stage), want, d.cells, what)
    assert_hyp_equal(got, t["map"], what)
    return want


def check_set_depth(d, kf, t, want, what):
    sd = rc.setdepth_from_planes(kf.idepth(0), kf.idepthVar(0), d.hyp["idepth_smoothed"])
    rc.assert_decisions({"setdepth": sd}, want, d.cells, what + " Frame::setDepth", keys=("setdepth",))
    for lvl in range(5):
        assert_bit_equal(kf.idepth(lvl), t["planes"][lvl][0], what + " keyframe idepth L%d" % lvl)
        assert_bit_equal(kf.idepthVar(lvl), t["planes"][lvl][1], what + " keyframe idepthVar L%d" % lvl)
    st = kf.stats()
    assert st["numPoints"] == t["stats"]["numPoints"], what
    assert_mean_idepth(st, t["planes"][0][0], t["planes"][0][1], what)
    for k in (rc.SD_NOT_COUNTED, rc.SD_SMOOTHED, rc.SD_STORED):
        assert (want["setdepth"] == k).sum() > 0, what


def check_react_planes(d, kf, t, want, what):
    """Frame::takeReActivationData of the finalised keyframe: the hypotheses of the oracle's finalised map, the blacklist codes of the census"""
    rid, rvar, rval = kf.reActivationData()
    rc.assert_decisions({"react": rc.react_from_planes(rvar)}, want, d.cells, what + " re-activation planes", keys=("react",))
    fin = t["map"]
    v = fin["isValid"] > 0
    assert_bit_equal(rvar[v], fin["idepth_var"][v], what + " idepthVar_reAct")
    assert_bit_equal(rid[v], fin["idepth"][v], what + " idepth_reAct")
    assert np.array_equal(rval[v].astype(np.int32), fin["validity_counter"][v]), what + " validity_reAct"
    assert int(rval[v].max()) == 255, what + ": the validity counter 255 did not survive the uint8 plane"
    assert np.array_equal(rvar[~v], np.where(fin["blacklisted"][~v] < rc.MIN_BLACKLIST, np.float32(-2), np.float32(-1))), what + " idepthVar_reAct codes"
    assert (want["react"] == -2).sum() > 0 and (want["react"] == -1).sum() > 0, what


def check_from_react(cells_, got, t_fin, what):
    """a map made by setFromExistingKF of a keyframe finalised on a sheet: the oracle's, and the census of the planes' reading"""
    hyp2 = react_sheet(t_fin["map"])
    want = rc.census(hyp2, np.zeros(hyp2.shape, np.float32), rc.MIN_USE_GRAD, "regularize", near="mask")
    rc.assert_decisions(rc.decisions_from_maps(hyp2, got, "regularize"), want, cells_, what, skip=want["uncertain"])
    assert_hyp_equal(got, t_fin["react_map"], what)
    assert want["uncertain"].mean() < 0.01 and (want["k6"] == rc.K6_REJECTED).sum() > 0, what


def check_created(oracle, d, got, nkg, s_g, t, what):
    """createKeyFrame's result: the oracle's pre-rescale map times the device's factor; the decisions of regularizeDepthMap(true) ->
    fill holes -> regularizeDepthMap(false) on the oracle's PROPAGATED map (values off the dyadic grid: comparisons near equality are
    left to the oracle)"""
    img, sim3, itr, mask, mg = new_keyframe_inputs(oracle, d.w, d.h)
    assert_created_keyframe_exact(oracle, what, t["pre"], s_g, t["s_o"], got, nkg, t["pose_o"], camera(d.w, d.h), img)
    want = rc.census(t["prop"], mg, d.th, "regularize_occ+fill_regularize", near="mask")
    ok = ~want["uncertain"]
    assert ok.mean() > 0.9, what
    for k, plane in (("valid", got["isValid"] > 0), ("blacklisted", got["blacklisted"])):
        bad = (plane != want[k]) & ok
        assert not bad.any(), "%s: decision '%s' differs from the census at %r (%d pixels)" % (what, k, np.argwhere(bad)[0][::-1], int(bad.sum()))
    assert want["created"].sum() > 0 and ((t["prop"]["isValid"] > 0) & ~want["valid"]).sum() > 0, what


# ---------------------------------------------------------------------------------------------------------------
# 176x144, 32x8 tiles (PY = 1)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", VARIANTS)
def test_stages(oracle, hip, v):
    """k_fill_holes, k_reg_fused<PassRegOnly, 1>, <PassRegOcc, 1>, <PassUpdate, 1>, each on the sheet itself"""
    run_stages(oracle, hip, v)


def run_stages(oracle, hip, v, params=None):
    """params: overrides of the context's settings (tests/test_settings_gpu.py runs the sheets at moved thresholds)"""
    assert workgroups(W, H) < 2048
    d = Dev(hip, context(hip, W, H, params), W, H, v)
    for stage in ("fillholes", "regularize", "regularize_occ", "fill_regularize"):
        d.reset()
        d.dm.stage(stage)
        check_map(d, d.dm.currentDepthMap(), truth(oracle, W, H, v, stage, d.th), stage, "variant %d minUseGrad %g stage %s" % (v, d.th, stage))


@pytest.mark.parametrize("v", VARIANTS)
def test_update_keyframe_due_and_not_due(oracle, hip, v):
    """k_reg_fused<PassUpdateSetDepth, 1> (the keyframe is due for Frame::setDepth) and <PassUpdate, 1> (it is not)"""
    run_update_keyframe_due_and_not_due(oracle, hip, v)


def run_update_keyframe_due_and_not_due(oracle, hip, v, params=None):
    d = Dev(hip, context(hip, W, H, params), W, H, v)
    for entry, flag in (("update_due", 0), ("update_not_due", 1)):
        what = "variant %d minUseGrad %g %s" % (v, d.th, entry)
        t = truth(oracle, W, H, v, entry, d.th)
        d.reset()
        d.kf.setCounters(7, 3, 3, flag)
        before = [(d.kf.idepth(l), d.kf.idepthVar(l)) for l in range(5)]
        d.dm.updateKeyframe([d.tracked()])
        want = check_map(d, d.dm.currentDepthMap(), t, "fill_regularize", what)
        assert d.kf.stats()["depthHasBeenUpdatedFlag"] == 1 and d.kf.stats()["numMappedOnThis"] == t["stats"]["numMappedOnThis"] == 4
        if flag == 0:
            check_set_depth(d, d.kf, t, want, what)
        else:
            for lvl in range(5):
                assert_bit_equal(d.kf.idepth(lvl), before[lvl][0], what + " keyframe idepth L%d (not due: untouched)" % lvl)
                assert_bit_equal(d.kf.idepthVar(lvl), before[lvl][1], what + " keyframe idepthVar L%d (not due: untouched)" % lvl)


@pytest.mark.parametrize("v", VARIANTS)
def test_finalize_then_set_from_existing(oracle, hip, v):
    run_finalize_then_set_from_existing(oracle, hip, v)


def run_finalize_then_set_from_existing(oracle, hip, v, params=None):
    d = Dev(hip, context(hip, W, H, params), W, H, v)
    what = "variant %d minUseGrad %g finalizeKeyFrame" % (v, d.th)
    t = truth(oracle, W, H, v, "finalize", d.th)
    d.dm.finalizeKeyFrame()
    want = check_map(d, d.dm.currentDepthMap(), t, "fill_regularize", what)
    check_set_depth(d, d.kf, t, want, what)
    check_react_planes(d, d.kf, t, want, what)
    d.dm.setFromExistingKF(d.kf)
    check_from_react(d.cells, d.dm.currentDepthMap(), t, "variant %d setFromExistingKF" % v)


@pytest.mark.parametrize("v", VARIANTS)
def test_create_keyframe(oracle, hip, v):
    """createKeyFrame into a second frame at a small general pose: k_reg_fused<PassRegOcc, 1> and the fill + regularise pass with the rescale
    sums on the propagated sheet"""
    run_create_keyframe(oracle, hip, v)


def run_create_keyframe(oracle, hip, v, params=None):
    d = Dev(hip, context(hip, W, H, params), W, H, v)
    nkg = d.new_keyframe(oracle)
    s_g = d.dm.createKeyFrame(nkg)
    check_created(oracle, d, d.dm.currentDepthMap(), nkg, s_g, truth(oracle, W, H, v, "create", d.th), "variant %d minUseGrad %g createKeyFrame" % (v, d.th))


def run_change_batch(oracle, hip, w, h, variants, py, params=None):
    """changeKeyframeBatch = finalizeKeyFrame + createKeyFrame per map in shared launches: k_kf_finalize_prop (PassKfFinalize), k_kf_reg<PassRegOcc>,
    k_kf_reg<PassKfFillSums>"""
    ctx = context(hip, w, h, params)
    n = len(variants)
    devs = [Dev(hip, ctx, w, h, v, kf_id=10 * j) for j, v in enumerate(variants)]
    nkgs = [d.new_keyframe(oracle) for d in devs]
    scales = hip.DepthMap.changeKeyframeBatch([d.dm for d in devs], nkgs)
    assert_form(ctx, "change", {"n": n, "py": py}, "changeKeyframeBatch n = %d" % n)
    for j, d in enumerate(devs):
        what = "changeKeyframeBatch n = %d map %d (variant %d)" % (n, j, d.v)
        tf, tc = truth(oracle, w, h, d.v, "finalize", d.th), truth(oracle, w, h, d.v, "change", d.th)
        want = rc.census(d.hyp, d.mg, d.th, "fill_regularize")
        check_set_depth(d, d.kf, tf, want, what + " old keyframe")
        check_react_planes(d, d.kf, tf, want, what + " old keyframe")
        m2 = hip.DepthMap(ctx)
        m2.setFromExistingKF(d.kf)
        assert_hyp_equal(m2.currentDepthMap(), tf["react_map"], what + " old keyframe re-activation")
        check_created(oracle, d, d.dm.currentDepthMap(), nkgs[j], scales[j], tc, what)


def run_reactivate_batch(oracle, hip, w, h, variants, params=None):
    """reactivateKeyframeBatch = finalizeKeyFrame of the current keyframe (k_kf_finalize: PassKfFinalizeOnly) + setFromExistingKF of a banked
    one (k_kf_from_react: PassFromReact).  Map j stands on variant v_j of the sheet; the banked keyframe it goes back to was finalised on
    variant v_j + 1, so the planes PassFromReact reads are a designed sheet's too."""
    ctx = context(hip, w, h, params)
    n = len(variants)
    olds = []
    for j, v in enumerate(variants):
        o = Dev(hip, ctx, w, h, (v + 1) % rc.VARIANTS, kf_id=1000 + j)
        o.dm.finalizeKeyFrame()
        olds.append(o)
    devs = [Dev(hip, ctx, w, h, v, kf_id=10 * j) for j, v in enumerate(variants)]
    hip.DepthMap.reactivateKeyframeBatch([d.dm for d in devs], [o.kf for o in olds])
    for j, d in enumerate(devs):
        what = "reactivateKeyframeBatch n = %d map %d (variant %d)" % (n, j, d.v)
        tf = truth(oracle, w, h, d.v, "finalize", d.th)
        want = rc.census(d.hyp, d.mg, d.th, "fill_regularize")
        check_set_depth(d, d.kf, tf, want, what + " finalised keyframe")
        check_react_planes(d, d.kf, tf, want, what + " finalised keyframe")
        check_from_react(olds[j].cells, d.dm.currentDepthMap(), truth(oracle, w, h, olds[j].v, "finalize", d.th), what + " re-activated map")


@pytest.mark.parametrize("variants", [(0,), (1, 2, 3)], ids=["n1", "n3"])
def test_change_keyframe_batch(oracle, hip, variants):
    assert workgroups(W, H, len(variants)) < 2048
    run_change_batch(oracle, hip, W, H, variants, py=1)


@pytest.mark.parametrize("variants", [(4,), (5, 0, 2)], ids=["n1", "n3"])
def test_reactivate_keyframe_batch(oracle, hip, variants):
    assert workgroups(W, H, len(variants)) < 2048
    run_reactivate_batch(oracle, hip, W, H, variants)


def run_row_parts(hip, d, parts):
    """the fused pass as parts of tile rows in ONE k_reg_rows_batch launch, then the swap of the validity planes: the calls the row-band loop
    of tests/test_bands_gpu.py issues (lsdhip_depth_stage_rows_batch, lsdhip_depth_stage_rows), with part boundaries of the test's choosing"""
    from lsd_slam_amd import capi
    L = capi.lib()
    n = len(parts)
    assert sorted(parts)[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(sorted(parts), sorted(parts)[1:])) and \
        sorted(parts)[-1][0] + sorted(parts)[-1][1] == (d.h + 7) // 8
    ma = (C.c_void_p * n)(*[d.dm.h_ for _ in parts])
    t0 = (C.c_int * n)(*[p[0] for p in parts])
    nr = (C.c_int * n)(*[p[1] for p in parts])
    capi.check(L.lsdhip_depth_stage_rows_batch(d.ctx.h_, n, ma, t0, nr), False)
    capi.check(L.lsdhip_depth_stage_rows(d.dm.h_, 5, 0, 0, 1), False)


@pytest.mark.parametrize("v", VARIANTS)
def test_row_parts(oracle, hip, v):
    """k_reg_rows_batch<1>: three parts issued out of order; the boundaries (tile rows 7 | 8 and 10 | 11) cut through cells"""
    d = Dev(hip, context(hip, W, H), W, H, v)
    run_row_parts(hip, d, [(11, 7), (0, 7), (7, 4)])
    check_map(d, d.dm.currentDepthMap(), truth(oracle, W, H, v, "fill_regularize"), "fill_regularize", "variant %d row parts" % v)


# ---------------------------------------------------------------------------------------------------------------
# 32x16 tiles (PY = 2)
# ---------------------------------------------------------------------------------------------------------------
def test_single_map_32x16_tiles_1024x512(oracle, hip):
    """1024x512 = 2048 workgroups of 32x8: the smallest single map that lsd_reg_py gives the 32x16 tile.  The sheet's lattice runs over the whole
    map; rows 7 | 8 now lie inside a tile, rows 15 | 16 at a seam.  k_reg_fused<PassRegOnly, 2>, <PassRegOcc, 2>, <PassUpdate, 2>,
    <PassUpdateSetDepth, 2>, and k_reg_rows_batch<2> with parts of 21 + 1 + 42 tile rows: the first two end inside a 32x16 tile."""
    w, h = 1024, 512
    assert workgroups(w, h) == 2048
    d = Dev(hip, context(hip, w, h), w, h, 0)
    for stage in ("regularize", "regularize_occ", "fill_regularize"):
        d.reset()
        d.dm.stage(stage)
        check_map(d, d.dm.currentDepthMap(), truth(oracle, w, h, 0, stage), stage, "1024x512 stage %s" % stage)
    for entry, flag in (("update_due", 0), ("update_not_due", 1)):
        t = truth(oracle, w, h, 0, entry)
        d.reset()
        d.kf.setCounters(7, 3, 3, flag)
        d.dm.updateKeyframe([d.tracked()])
        want = check_map(d, d.dm.currentDepthMap(), t, "fill_regularize", "1024x512 " + entry)
        if flag == 0:
            check_set_depth(d, d.kf, t, want, "1024x512 " + entry)
    d.reset()
    run_row_parts(hip, d, [(22, 42), (0, 21), (21, 1)])
    check_map(d, d.dm.currentDepthMap(), truth(oracle, w, h, 0, "fill_regularize"), "fill_regularize", "1024x512 row parts")


N_TALL = 19     # 19 x 108 = 2052 workgroups: the fewest pixels of any n x size of the suite's sizes that reaches 2048 (7 x 320x240 = 2100 has more)
TALL = tuple(j % rc.VARIANTS for j in range(N_TALL))


def test_batch_32x16_tiles_update(oracle, hip):
    """updateKeyframeBatch of 19 maps of 176x144: k_reg_fused_batch<PassUpdateSetDepth, 2> for the maps due for Frame::setDepth and
    <PassUpdate, 2> for the others in one call; 144 rows = 9 tiles of 16"""
    assert workgroups(W, H, N_TALL) >= 2048 > workgroups(W, H, N_TALL - 1)
    ctx = context(hip, W, H)
    devs = [Dev(hip, ctx, W, H, v, kf_id=10 * j) for j, v in enumerate(TALL)]
    due = [j % 3 != 1 for j in range(N_TALL)]
    for d, is_due in zip(devs, due):
        d.kf.setCounters(7, 3, 3, not is_due)
    before = [None if is_due else [(d.kf.idepth(l), d.kf.idepthVar(l)) for l in range(5)] for d, is_due in zip(devs, due)]
    hip.DepthMap.updateKeyframeBatch([d.dm for d in devs], [d.tracked(100 + j) for j, d in enumerate(devs)])
    assert_form(ctx, "update", {"n": N_TALL, "py": 2, "nSet": int(sum(due))}, "updateKeyframeBatch n = 19")
    for j, d in enumerate(devs):
        what = "updateKeyframeBatch n = 19 map %d (variant %d, %s)" % (j, d.v, "due" if due[j] else "not due")
        t = truth(oracle, W, H, d.v, "update_due" if due[j] else "update_not_due")
        want = check_map(d, d.dm.currentDepthMap(), t, "fill_regularize", what)
        if due[j]:
            check_set_depth(d, d.kf, t, want, what)
        else:
            for lvl in range(5):
                assert_bit_equal(d.kf.idepth(lvl), before[j][lvl][0], what + " keyframe idepth L%d (untouched)" % lvl)


def test_batch_32x16_tiles_change_keyframe(oracle, hip):
    run_change_batch(oracle, hip, W, H, TALL, py=2)


def test_batch_32x16_tiles_reactivate_keyframe(oracle, hip):
    assert workgroups(W, H, N_TALL) >= 2048 > workgroups(W, H, N_TALL - 1)
    run_reactivate_batch(oracle, hip, W, H, TALL)
