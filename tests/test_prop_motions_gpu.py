"""DepthMap::propagateDepth on the device under general camera motion (tests/prop_motions.py: all four borders, both directions of the
occlusion branch, sources behind the new camera, the validity cap, targets with exactly 8, 9, 10 and up to ~17 sources under a rotated
pose, a thisToParent_raw with a Sim3 scale, a photometric test that rejects most sources) against the CPU oracle, per pixel and BIT FOR
BIT: k_prop_candidates + k_prop_resolve alone, the whole createKeyFrame, a second propagation on one map, and changeKeyframeBatch
(k_kf_finalize_prop -> k_prop_resolve_batch -> ...) with every map of a call under another motion and start state, followed by an update
and a second change that starts from the propagation scratch the first left.  Both sides get identical explicit poses, masks and
counters.  tests/test_prop_motions_cpu.py shows on the CPU that these inputs reach every branch and that the oracle is DepthMap.cpp's own
arithmetic under them.

A failing map comparison names the first differing target pixel, the census classes it falls in and the number of sources it had."""
import numpy as np
import pytest

import prop_motions as pm
from test_depth_batch_gpu import ONE_LAUNCH, SPLIT_ALL, build_twins, change_round, update_round, upload_twins
from test_gpu_parity import assert_created_keyframe_exact, assert_hyp_equal, oracle_prerescale_after_propagate

pytestmark = pytest.mark.gpu

PLANES = ("isValid", "blacklisted", "validity_counter", "nextStereoFrameMinID", "idepth", "idepth_var", "idepth_smoothed", "idepth_var_smoothed")
SMALL, LARGE = (176, 144), (320, 240)        # 176 = 5.5 tiles of 32, 144 = 4.5 rows of tiles
LARGE_MOTIONS = ("forward-big", "far-back-roll", "back-1.5", "wide", "other-scene", "scaled")


@pytest.fixture(scope="module")
def hip():
    import lsd_slam_amd as la
    return la


def assert_map(oracle, w, h, g, o, what, before, name, use_mask):
    """assert_hyp_equal (bit for bit); on a mismatch the message also names the first differing pixel, both records, its census classes
    as a target under the motion and the number of sources it had"""
    try:
        assert_hyp_equal(g, o, what)
    except AssertionError as e:
        d = g["isValid"] != o["isValid"]
        v = o["isValid"] > 0
        for k in PLANES[1:]:
            d |= (g[k].view(np.uint32 if g[k].dtype == np.float32 else g[k].dtype) != o[k].view(np.uint32 if o[k].dtype == np.float32 else o[k].dtype)) \
                & (v | (k == "blacklisted"))
        y, x = [int(a) for a in np.argwhere(d)[0]]
        c = pm.case_census(oracle, w, h, name, use_mask, False, hyp=before)
        cls, nsrc = pm.classes_at(c, x, y)
        raise AssertionError("%s\nfirst differing pixel (x=%d, y=%d): device %r, oracle %r\ncensus under %s: %d sources, classes %r"
                             % (e, x, y, g[y, x].tolist(), o[y, x].tolist(), name, nsrc, cls)) from None


CTX = {}


def make_pair(oracle, hip, w, h, hyp):
    """the same map on both sides, on the keyframe of pm.frames (counters 7, 3, 3, depth not yet published); one context per size"""
    imgs, depth0, K, _ = pm.frames(w, h)
    if (w, h) not in CTX:
        CTX[(w, h)] = hip.Context(w, h, K)
    ctx = CTX[(w, h)]
    kfo, dmo = pm.oracle_map(oracle, w, h, hyp)
    kfg = hip.Frame(ctx, 0, imgs[0])
    kfg.setDepthFromGroundTruth(depth0)
    dmg = hip.DepthMap(ctx)
    dmg.setCurrentDepthMap(kfg, hyp)
    kfg.setCounters(7, 3, 3, 0)
    return ctx, kfo, kfg, dmo, dmg


def device_frame(oracle, hip, ctx, w, h, name, parent, mask=True):
    f, sim3, itr = pm.pose_of(oracle, w, h, name)
    fg = hip.Frame(ctx, f, pm.frames(w, h)[0][pm.index_of(name)])
    fg.setPose(sim3, parent, itr)
    if mask:
        fg.set_refPixelWasGood(pm.mask_of(w, h, name))
    return fg


def is_chain_case(w, h, name):
    return name == "far-back-roll" or (name == "back-1.5" and (w, h) == LARGE)


def propagate_alone(oracle, hip, w, h, name, use_mask, plant):
    hyp = pm.start_state(w, h, plant)
    ctx, kfo, kfg, dmo, dmg = make_pair(oracle, hip, w, h, hyp)
    fo = pm.oracle_frame(oracle, w, h, name, kfo, mask=use_mask)
    fg = device_frame(oracle, hip, ctx, w, h, name, kfg, mask=use_mask)
    dmo.stage("propagate", [fo])
    after = dmo.get()
    # from the oracle (and, for the chains, the census) alone: the case does something
    assert int((after["isValid"] > 0).sum()) >= 1000, (name, w, h)
    if is_chain_case(w, h, name):
        c = pm.case_census(oracle, w, h, name, use_mask, plant)
        assert c["counts"]["targets-over-cap"] > 0, (name, w, h, c["max_sources"])
    dmg.stage("propagate", [fg])
    assert_map(oracle, w, h, dmg.currentDepthMap(), after, "%s %dx%d propagateDepth" % (name, w, h), hyp, name, use_mask)


@pytest.mark.parametrize("use_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("name", pm.NAMES)
def test_propagate_every_motion_planted_state(oracle, hip, name, use_mask):
    propagate_alone(oracle, hip, *SMALL, name, use_mask, True)


@pytest.mark.parametrize("use_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("name", LARGE_MOTIONS)
def test_propagate_320x240_planted_state(oracle, hip, name, use_mask):
    propagate_alone(oracle, hip, *LARGE, name, use_mask, True)


@pytest.mark.parametrize("use_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("w,h", [SMALL, LARGE])
@pytest.mark.parametrize("name", pm.CHAINS)
def test_propagate_chains_plain_state(oracle, hip, name, w, h, use_mask):
    """the start state of the zoom-out test (no planting) under the two backward motions with a rotation: exactly 8, 9 and 10 sources
    on the fullest targets of "back-1.5", up to ~17 on those of "far-back-roll" """
    propagate_alone(oracle, hip, w, h, name, use_mask, False)


CREATE = [("forward-big", True, True), ("far-back-roll", True, False), ("back-1.5", True, False), ("other-scene", False, False),
          ("scaled", True, False), ("x-", True, True)]


@pytest.mark.parametrize("w,h", [SMALL, LARGE])
@pytest.mark.parametrize("name,use_mask,plant", CREATE, ids=[c[0] for c in CREATE])
def test_create_keyframe_under_motion(oracle, hip, name, use_mask, plant, w, h):
    """the whole createKeyFrame from the same start: the map against the oracle's pre-rescale map times the factor of
    test_gpu_parity.expected_rescale, the new keyframe's pyramids and statistics, its pose and the pose's scale"""
    hyp = pm.start_state(w, h, plant)
    ctx, kfo, kfg, dmo, dmg = make_pair(oracle, hip, w, h, hyp)
    nko = pm.oracle_frame(oracle, w, h, name, kfo, mask=use_mask)
    dmo.stage("propagate", [nko])
    pre = oracle_prerescale_after_propagate(dmo)
    assert int((pre["isValid"] > 0).sum()) >= 1000
    kfo, dmo = pm.oracle_map(oracle, w, h, hyp)
    nko = pm.oracle_frame(oracle, w, h, name, kfo, mask=use_mask)
    s_o = dmo.create_keyframe(nko)
    nkg = device_frame(oracle, hip, ctx, w, h, name, kfg, mask=use_mask)
    s_g = dmg.createKeyFrame(nkg)
    assert_created_keyframe_exact(oracle, "%s %dx%d createKeyFrame" % (name, w, h), pre, s_g, s_o, dmg.currentDepthMap(), nkg, nko.pose(),
                                  pm.frames(w, h)[2], pm.frames(w, h)[0][pm.index_of(name)])
    assert nkg.stats()["numPoints"] == nko.stats()["numPoints"]


@pytest.mark.parametrize("w,h", [SMALL, LARGE])
def test_second_propagation_on_one_map(oracle, hip, w, h):
    """"far-back-roll" (chains in use), then "forward" relative to the new keyframe, on ONE DepthMap: the second call must find slot
    counts and chain heads as a first call does"""
    hyp = pm.start_state(w, h, False)
    ctx, kfo, kfg, dmo, dmg = make_pair(oracle, hip, w, h, hyp)
    before = hyp
    for name in ("far-back-roll", "forward"):
        fo = pm.oracle_frame(oracle, w, h, name, kfo)
        fg = device_frame(oracle, hip, ctx, w, h, name, kfg)
        dmo.stage("propagate", [fo])
        dmg.stage("propagate", [fg])
        after = dmo.get()
        assert int((after["isValid"] > 0).sum()) >= 1000, name
        assert_map(oracle, w, h, dmg.currentDepthMap(), after, "%s %dx%d propagateDepth" % (name, w, h), before, name, True)
        kfo, kfg, before = fo, fg, after


def motion_source(w, h, nframes, seq, kind):
    return pm.frames(w, h)


# per call shape: (new keyframe's motion, planted start state, frame of the update behind the change) per map
BATCH = {(320, 240, 3): (("forward-big", True, "forward"), ("far-back-roll", False, "back-1.5"), ("x-", True, "x+")),
         (320, 240, 8): (("x+", False, "diag++"), ("forward-big", True, "forward"), ("yaw", False, "x+"), ("far-back-roll", False, "back-1.5"),
                         ("back-1.5", False, "backward"), ("other-scene", False, "x-"), ("scaled", False, "x+"), ("wide", True, "x+")),
         (176, 144, 4): (("far-back-roll", False, "back-1.5"), ("forward-big", True, "forward"), ("scaled-up", False, "x+"), ("y-", True, "y+"))}


def change_batch(oracle, hip, w, h, n, py, dev=True):
    plan = BATCH[(w, h, n)]
    twins = build_twins(oracle, w, h, n, sigma=0.02, regularize=True, seed0=1300, source=motion_source, nseq=1, nframes=len(pm.NAMES) + 1)
    for j, t in enumerate(twins):
        if plan[j][1]:
            t.hyp0 = pm.planted(t.hyp0, 7 + j)
            t.dm.set(t.kf, t.hyp0, reactivated=t.react)
    ctx = None
    if dev:
        ctx = hip.Context(w, h, twins[0].K)
        upload_twins(hip, ctx, twins)
    masks = [j % 2 == 0 for j in range(n)]        # ("other-scene" sits on an odd place: no mask, the photometric test decides)
    names = [p[0] for p in plan]
    what = "%dx%d n=%d change under %r" % (w, h, n, names)
    res = change_round(oracle, hip, ctx, twins, [pm.index_of(m) for m in names], what, masks, py,
                       poses=[pm.pose_of(oracle, w, h, m)[1] for m in names])
    # from the oracle and the census alone: the maps of the call that are there for a rare branch take it
    for j, (name, plant, _) in enumerate(plan):
        r = res[j]
        assert r["n_dst"] >= 1000, (what, j, r["n_dst"])
        if name == "forward-big":
            neg = int(((r["prop"]["isValid"] > 0) & (r["prop"]["idepth"] < 0)).sum())
            assert plant and neg >= 50, (what, j, neg)
        if name == "far-back-roll":
            c = pm.case_census(oracle, w, h, name, masks[j], False, hyp=r["fin"])
            assert c["counts"]["targets-over-cap"] > 0 and c["max_sources"] > pm.PROP_SLOT_CAP + 2, (what, j, c["max_sources"])
    # negative and capped hypotheses flow on into observe (the maps were never updated since upload: every-pixel select from 4 maps on)
    split = n >= 4
    update_round(oracle, hip, ctx, twins, [pm.index_of(p[2]) for p in plan], what + ", update behind it", form=dict(SPLIT_ALL if split else ONE_LAUNCH, py=py))
    # a second change of every map, from the scratch the first left (chains were in use): "forward" relative to each new keyframe
    change_round(oracle, hip, ctx, twins, pm.index_of("forward"), what + ", second change", [not m for m in masks], py,
                 poses=[pm.pose_of(oracle, w, h, "forward")[1]] * n)


@pytest.mark.parametrize("w,h,n,py", [(320, 240, 3, 1), (320, 240, 8, 2), (176, 144, 4, 1)])
def test_change_keyframe_batch_a_motion_per_map(oracle, hip, w, h, n, py):
    change_batch(oracle, hip, w, h, n, py)
