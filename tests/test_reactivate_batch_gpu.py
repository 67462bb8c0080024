"""lsdhip_depth_reactivate_keyframe_batch: DepthMap::finalizeKeyFrame (DepthMap.cpp:1363-1395) on each map's keyframe followed by
DepthMap::setFromExistingKF (DepthMap.cpp:920-962) of a banked keyframe, for n maps in three shared launches.  The yardstick is the pair of
single calls lsdhip_depth_finalize + lsdhip_depth_set_from_existing, which this change does not touch: every plane the fused call
leaves must equal theirs BIT for bit — the maps, the finalised keyframes' level-0 planes, pyramids, statistics and re-activation planes,
and the maps after one further updateKeyframe on the re-activated keyframe."""
import numpy as np
import pytest

from common import ODOMETRY_ITS, assert_bit_equal, sequence

pytestmark = pytest.mark.gpu

IDENT7 = np.array([1.0, 0, 0, 0, 0, 0, 0])
HYP_FIELDS = ("isValid", "blacklisted", "nextStereoFrameMinID", "validity_counter", "idepth", "idepth_var", "idepth_smoothed", "idepth_var_smoothed")
W, H = 176, 144          # 5 1/2 tiles wide, 18 tile rows: every tile's halo reaches an image edge or a neighbour
VARIANTS = ("twice", "blacklisted", "holes")


@pytest.fixture(scope="module")
def hip():
    import lsd_slam_amd as la
    from lsd_slam_amd import capi
    assert hasattr(capi.lib(), "lsdhip_depth_reactivate_keyframe_batch"), "liblsdhip.so has no lsdhip_depth_reactivate_keyframe_batch"
    return la


def assert_maps_identical(a, b, what):
    """every field of every pixel: the fused call must also leave what the two calls leave in the pixels that hold no hypothesis"""
    for k in HYP_FIELDS:
        assert_bit_equal(a[k], b[k], "%s: %s" % (what, k))


class World:
    """one sequence's keyframe, map and tracking reference, driven by the single calls"""

    def __init__(self, hip, ctx, tr, s, seq, variant):
        self.hip, self.ctx, self.tr, self.s, self.variant = hip, ctx, tr, s, variant
        self.frames, depth0 = seq[0], seq[1]
        self.t = 0
        self.kf = hip.Frame(ctx, 1000 * s, self.frames[0])
        self.kf.setDepthFromGroundTruth(depth0)
        self.map = hip.DepthMap(ctx)
        self.map.initializeFromGTDepth(self.kf)
        self.ref = hip.TrackingReference()
        self._adopt(self.kf)
        self.keep = []

    def _adopt(self, kf):
        self.kf = kf
        self.ref.importFrame(kf)
        kf.clearDepthHasBeenUpdatedFlag()
        self.pose = IDENT7.copy()

    def track(self):
        self.t += 1
        fr = self.hip.Frame(self.ctx, 1000 * self.s + self.t, self.frames[self.t])
        self.pose = self.tr.trackFrame(self.ref, fr, self.pose)
        return fr

    def update(self):
        self.map.updateKeyframe([self.track()])
        self.ref.importFrame(self.kf)
        self.kf.clearDepthHasBeenUpdatedFlag()

    def new_keyframe(self):
        fr = self.track()
        self.map.finalizeKeyFrame()
        self.map.createKeyFrame(fr)
        self.keep.append(self.kf)
        self._adopt(fr)

    def edit_map(self):
        """the variant's state, put into the map before its first keyframe is finalised (Frame::takeReActivationData then records it)"""
        h, w = self.ctx.h, self.ctx.w
        hyp = self.map.currentDepthMap()
        if self.variant == "blacklisted":
            # pixels without a hypothesis and a blacklist counter below MIN_BLACKLIST = -1: idepthVar_reAct = -2 (Frame.cpp:107-145)
            inv = hyp["isValid"] == 0
            assert inv.sum() > 200
            sel = inv & ((np.arange(w)[None, :] + np.arange(h)[:, None]) % 3 == 0)
            hyp["blacklisted"][sel] = -4
            # ... and hypotheses inside blacklisted surroundings, at the image border too
            hyp["isValid"][5:9, :] = 0
            hyp["blacklisted"][5:9, :] = -2
        elif self.variant == "holes":
            # large regions without hypotheses, cutting through tiles and along the image edges
            hyp["isValid"][:, : w // 3 + 5] = 0
            hyp["isValid"][h // 2 - 13: h // 2 + 30, :] = 0
            hyp["isValid"][h - 11:, w // 2:] = 0
        self.map.setCurrentDepthMap(self.kf, hyp)

    def prepare(self):
        """-> the banked keyframe to go back to; the map stands on a later keyframe with two updates on it"""
        self.update()
        if self.variant != "twice":
            self.edit_map()
        self.update()
        old = self.kf
        self.new_keyframe()
        self.update()
        if self.variant == "twice":
            # the banked keyframe comes back once by the single calls, is mapped on and finalised a second time
            self.map.finalizeKeyFrame()
            self.map.setFromExistingKF(old)
            self.keep.append(self.kf)
            self._adopt(old)
            self.update()
            self.new_keyframe()
            self.update()
        return old


def build(hip, ctx, variants, seq_of):
    tr = hip.SE3Tracker(ctx)
    tr.set_maxItsPerLvl(ODOMETRY_ITS)
    worlds = [World(hip, ctx, tr, s, seq_of(s), v) for s, v in enumerate(variants)]
    olds = [wd.prepare() for wd in worlds]
    return worlds, olds


def compare_after_change(A, B, finA, finB, tag):
    for s, (a, b) in enumerate(zip(A, B)):
        what = "%s map %d (%s)" % (tag, s, a.variant)
        assert_maps_identical(a.map.currentDepthMap(), b.map.currentDepthMap(), what)
        fa, fb = finA[s], finB[s]
        for lvl in range(5):
            assert_bit_equal(fa.idepth(lvl), fb.idepth(lvl), "%s finalised keyframe idepth level %d" % (what, lvl))
            assert_bit_equal(fa.idepthVar(lvl), fb.idepthVar(lvl), "%s finalised keyframe idepthVar level %d" % (what, lvl))
        (ia, va, ca), (ib, vb, cb) = fa.reActivationData(), fb.reActivationData()
        assert_bit_equal(va, vb, "%s idepthVar_reAct" % what)
        m = va > 0
        assert m.sum() > 100, what
        assert_bit_equal(ia[m], ib[m], "%s idepth_reAct" % what)
        assert np.array_equal(ca[m], cb[m]), "%s validity_reAct" % what
        sa, sb = fa.stats(), fb.stats()
        assert sa == sb, (what, sa, sb)
        assert sa["numPoints"] > 100 and sa["depthHasBeenUpdatedFlag"] == 1.0
        so_a, so_b = a.kf.stats(), b.kf.stats()
        assert so_a == so_b and so_a["numMappedOnThis"] == 0 and so_a["numFramesTrackedOnThis"] == 0, (what, so_a, so_b)


def run_case(hip, ctx, variants, seq_of, tag):
    A, oldA = build(hip, ctx, variants, seq_of)
    B, oldB = build(hip, ctx, variants, seq_of)
    for a, b in zip(A, B):      # the two sets start from the same bits
        assert_maps_identical(a.map.currentDepthMap(), b.map.currentDepthMap(), "%s before" % tag)
    if "blacklisted" in variants:
        s = variants.index("blacklisted")
        var = oldB[s].reActivationData()[1]
        assert (var == -2).sum() > 100 and (var == -1).sum() > 100 and (var > 0).sum() > 100
    finA, finB = [a.kf for a in A], [b.kf for b in B]
    for a, old in zip(A, oldA):
        a.map.finalizeKeyFrame()
        a.map.setFromExistingKF(old)
    hip.DepthMap.reactivateKeyframeBatch([b.map for b in B], oldB)
    for wd, old in list(zip(A, oldA)) + list(zip(B, oldB)):
        wd._adopt(old)
    compare_after_change(A, B, finA, finB, tag)
    # the re-activated keyframe's updateKeyframe (DepthMap.cpp:1072-1213 with activeKeyFrameIsReactivated set)
    for wd in A + B:
        wd.update()
    for s, (a, b) in enumerate(zip(A, B)):
        assert_maps_identical(a.map.currentDepthMap(), b.map.currentDepthMap(), "%s map %d after an update on the re-activated keyframe" % (tag, s))
        for lvl in range(5):
            assert_bit_equal(a.kf.idepth(lvl), b.kf.idepth(lvl), "%s map %d re-activated keyframe idepth level %d" % (tag, s, lvl))
    return A, B


def seq_small(s):
    return sequence(W, H, 9, seq_index=s % 3)


@pytest.mark.parametrize("variants", [("blacklisted",), VARIANTS], ids=["n1", "n3"])
def test_reactivate_batch_equals_finalize_plus_set_from_existing(hip, variants):
    ctx = hip.Context(W, H, seq_small(0)[2])
    assert ((W + 31) // 32) * ((H + 7) // 8) * len(variants) < 2048        # the 32 x 8 tiles (PY = 1)
    run_case(hip, ctx, variants, seq_small, "n = %d" % len(variants))


def test_reactivate_batch_tall_tiles(hip):
    """the launch shape with 32 x 16 tiles (lsd_reg_py: from 2048 workgroups of 32 x 8 on): 19 maps of 176 x 144 are 19 x 108 = 2052, fewer
    pixels than any other n x size of the suite's sizes that reaches the threshold (7 x 320 x 240 = 2100 workgroups, 1 x 1024 x 512 = 2048)"""
    n = 19
    wg = ((W + 31) // 32) * ((H + 7) // 8)
    assert wg * n >= 2048 and wg * (n - 1) < 2048
    ctx = hip.Context(W, H, seq_small(0)[2])
    run_case(hip, ctx, tuple(VARIANTS[s % 3] for s in range(n)), seq_small, "n = 19")


def test_reactivate_batch_on_a_pipelined_context(hip):
    """mapping stream beside tracking stream, mapping calls asynchronous: the call returns with its launches queued; the downloads of the
    comparison drain the streams"""
    ctx = hip.Context(W, H, seq_small(0)[2])
    ctx.set_pipeline(True)
    ctx.set_async(True)
    run_case(hip, ctx, ("blacklisted",), seq_small, "pipelined")


def test_reactivate_batch_rejects_bad_arguments(hip):
    import ctypes as C
    ctx = hip.Context(W, H, seq_small(0)[2])
    worlds, olds = build(hip, ctx, ("holes", "blacklisted"), seq_small)
    a, b = worlds
    from lsd_slam_amd import capi
    L = capi.lib()
    before = [wd.map.currentDepthMap() for wd in worlds]
    kfs = [wd.kf for wd in worlds]
    never = hip.Frame(ctx, 7777, a.frames[0])                    # never finalised: no re-activation data
    empty = hip.DepthMap(ctx)                                    # no active keyframe

    def call(maps, frames):
        n = len(maps)
        ma = (C.c_void_p * n)(*[m.h_ if m is not None else None for m in maps])
        fa = (C.c_void_p * n)(*[f.h_ if f is not None else None for f in frames])
        return L.lsdhip_depth_reactivate_keyframe_batch(n, ma, fa)

    E_ARG, E_STATE = -1, -3          # LSDHIP_E_ARG, LSDHIP_E_STATE (include/lsdhip.h)
    cases = [
        ("no re-activation data", [a.map, b.map], [olds[0], never], E_STATE),
        ("no active keyframe", [a.map, empty], [olds[0], olds[1]], E_STATE),
        ("the current keyframe", [a.map, b.map], [olds[0], b.kf], E_ARG),
        ("a null frame", [a.map, b.map], [olds[0], None], E_ARG),
        ("a null map", [a.map, None], [olds[0], olds[1]], E_ARG),
        ("the same map twice", [a.map, a.map], [olds[0], olds[1]], E_ARG),
    ]
    for what, maps, frames, want in cases:
        assert call(maps, frames) == want, what
        for wd, kf, hyp in zip(worlds, kfs, before):
            assert_maps_identical(wd.map.currentDepthMap(), hyp, "after the rejected call (%s)" % what)
        # ... and still on their keyframes: the next update is accepted and the fused call still works afterwards (below)
    assert L.lsdhip_depth_reactivate_keyframe_batch(0, None, None) == E_ARG
    with pytest.raises(Exception):
        hip.DepthMap.reactivateKeyframeBatch([a.map], [never])
    hip.DepthMap.reactivateKeyframeBatch([a.map, b.map], olds)
    for wd, old in zip(worlds, olds):
        wd._adopt(old)
        wd.update()
        assert wd.map.currentDepthMap()["isValid"].sum() > 100
