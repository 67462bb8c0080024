"""The epipolar search on the device under general camera motion (tests/epl_motions.py: both signs of both walk increments, x- and
y-dominant lines, every border clip, epipole inside the image, rescaleFactor outside [0.7, 1.4], wide and near-zero baselines, a second
image of another scene) against the CPU oracle, per pixel and BIT FOR BIT: k_observe with one reference, a mixed deque that sends
neighbouring lanes to references of opposite motions, partial tiles, the batched forms (one launch; select + walk with the every-pixel and
the candidate select) and updateKeyframe end to end.  Both sides get identical explicit poses, masks, initialTrackedResidual and
counters.  tests/test_epl_motions_cpu.py shows on the CPU that these inputs reach every branch, that the walk's reads stay inside the
image, and that the oracle is DepthMap.cpp's own arithmetic under these motions.

A failing comparison names the first differing pixel and the census classes it falls in."""
import numpy as np
import pytest

import epl_motions as em
from common import assert_bit_equal
from test_depth_batch_gpu import (ONE_LAUNCH, SPLIT_ALL, SPLIT_CAND, assert_mean_idepth, build_twins, changed_pixels, update_round,
                                  upload_twins)
from test_gpu_parity import STEREO, assert_hyp_equal, oracle_params

pytestmark = pytest.mark.gpu

PLANES = ("isValid", "blacklisted", "validity_counter", "nextStereoFrameMinID", "idepth", "idepth_var", "idepth_smoothed", "idepth_var_smoothed")


@pytest.fixture(scope="module")
def hip():
    import lsd_slam_amd as la
    return la


def assert_map(oracle, w, h, g, o, what, before=None, motions=()):
    """assert_hyp_equal (bit for bit); on a mismatch the message also names the first differing pixel, both records, and the census
    classes of that pixel under the motions involved"""
    try:
        assert_hyp_equal(g, o, what)
    except AssertionError as e:
        d = g["isValid"] != o["isValid"]
        v = o["isValid"] > 0
        for k in PLANES[1:]:
            d |= (g[k].view(np.uint32 if g[k].dtype == np.float32 else g[k].dtype) != o[k].view(np.uint32 if o[k].dtype == np.float32 else o[k].dtype)) \
                & (v | (k == "blacklisted"))
        y, x = [int(a) for a in np.argwhere(d)[0]]
        msg = ["%s" % e, "first differing pixel (x=%d, y=%d): device %r, oracle %r" % (x, y, g[y, x].tolist(), o[y, x].tolist())]
        if before is not None:
            msg.append("before the stage: %r" % (before[y, x].tolist(),))
            for name in motions:
                c = em.census(em.frames(w, h)[2], w, h, before, em.pose_of(oracle, w, h, name)[1], oracle.default_params())
                msg.append("census classes under %s: %r" % (name, em.classes_at(c, x, y)))
        raise AssertionError("\n".join(msg)) from None


def make_pair(oracle, hip, w, h, params=None, seed=1, reactivated=False, hyp=None):
    """the same ragged map on both sides, on the keyframe of em.frames (counters 7, 3, 3, depth not yet published)"""
    imgs, depth0, K, _ = em.frames(w, h)
    ctx = hip.Context(w, h, K, params=params)
    kfo, dmo, hyp = em.noisy_map(oracle, w, h, params=oracle_params(oracle, params), seed=seed, reactivated=reactivated, hyp=hyp)
    kfg = hip.Frame(ctx, 0, imgs[0])
    kfg.setDepthFromGroundTruth(depth0)
    dmg = hip.DepthMap(ctx)
    dmg.setCurrentDepthMap(kfg, hyp, reactivated=reactivated)
    kfg.setCounters(7, 3, 3, 0)
    return ctx, kfo, kfg, dmo, dmg, hyp


def device_frame(oracle, hip, ctx, w, h, name, parent, mask=True, fid=None):
    f, sim3, itr = em.pose_of(oracle, w, h, name)
    fg = hip.Frame(ctx, f if fid is None else fid, em.frames(w, h)[0][em.index_of(name)])
    fg.setPose(sim3, parent, itr)
    if mask:
        fg.set_refPixelWasGood(em.mask_of(w, h, name))
    return fg


def observe_stages(oracle, hip, w, h, name, params):
    """observe with the motion's frame as the only reference, fillholes, regularize, and a second observe that sees smoothed values:
    compared after each stage"""
    ctx, kfo, kfg, dmo, dmg, hyp = make_pair(oracle, hip, w, h, params=params)
    fo = em.oracle_frame(oracle, w, h, name, kfo)
    fg = device_frame(oracle, hip, ctx, w, h, name, kfg)
    before = hyp
    for i, st in enumerate(("observe", "fillholes", "regularize", "observe")):
        dmo.stage(st, [fo] if st == "observe" else [])
        dmg.stage(st, [fg] if st == "observe" else [])
        after = dmo.get()
        assert_map(oracle, w, h, dmg.currentDepthMap(), after, "%s %dx%d: %s (stage %d)" % (name, w, h, st, i), before, [name])
        if st == "observe" and name != em.TINY:
            assert changed_pixels(before, after) >= 1000, (name, st, i)      # (from the oracle alone: the stage did something)
        before = after


@pytest.mark.parametrize("name", em.NAMES)
def test_observe_one_reference_every_motion(oracle, hip, name):
    observe_stages(oracle, hip, 320, 240, name, None)


@pytest.mark.parametrize("params", STEREO[1:])
@pytest.mark.parametrize("name", ["forward", "backward", "x-", "y+"])
def test_observe_one_reference_switch_sets(oracle, hip, name, params):
    """the three switch sets besides the defaults (which test_observe_one_reference_every_motion runs on every motion)"""
    observe_stages(oracle, hip, 320, 240, name, params)


@pytest.mark.parametrize("name", ["x-", "backward"])
def test_observe_partial_tiles(oracle, hip, name):
    """176x144: 5.5 tiles of 32 pixels"""
    observe_stages(oracle, hip, 176, 144, name, None)


DEQUE = ("x+", "y-", "forward", "yaw")       # frame ids 10 .. 13, oldest first
DEQUE_ID0 = 10


@pytest.mark.parametrize("reactivated", [False, True])
def test_observe_mixed_deque(oracle, hip, reactivated):
    """One observe call with four references of different motions.  nextStereoFrameMinID cycles through 0 (before the deque: the oldest),
    10 .. 13 (one reference each) and 14 (behind the deque: skipped) along x, shifted by two per row, so that neighbouring lanes of a wave
    walk along lines of opposite directions.  Re-activated, every pixel takes the newest reference."""
    w, h = 320, 240
    _, _, hyp0 = em.noisy_map(oracle, w, h)
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    cycle = np.array([0, 10, 11, 12, 13, 14], np.float32)
    hyp0 = hyp0.copy()
    hyp0["nextStereoFrameMinID"] = cycle[(xs + 2 * ys) % 6]
    ctx, kfo, kfg, dmo, dmg, hyp = make_pair(oracle, hip, w, h, hyp=hyp0, reactivated=reactivated)
    fos = [em.oracle_frame(oracle, w, h, n, kfo, fid=DEQUE_ID0 + i) for i, n in enumerate(DEQUE)]
    fgs = [device_frame(oracle, hip, ctx, w, h, n, kfg, fid=DEQUE_ID0 + i) for i, n in enumerate(DEQUE)]
    dmo.stage("observe", fos)
    after = dmo.get()
    # power, from the oracle alone: the references matter — with every hypothesis sent to the oldest (or, re-activated, with the
    # deque reversed) more than 1000 pixels end differently
    alt = hyp0.copy()
    alt["nextStereoFrameMinID"] = 0
    kf2, dm2, _ = em.noisy_map(oracle, w, h, hyp=alt, reactivated=reactivated)
    names2 = DEQUE[::-1] if reactivated else DEQUE
    dm2.stage("observe", [em.oracle_frame(oracle, w, h, n, kf2, fid=DEQUE_ID0 + i) for i, n in enumerate(names2)])
    got2 = dm2.get()
    differ = int(((got2["idepth"] != after["idepth"]) | (got2["isValid"] != after["isValid"])).sum())
    assert differ >= 1000, differ
    assert changed_pixels(hyp0, after) >= 1000
    dmg.stage("observe", fgs)
    assert_map(oracle, w, h, dmg.currentDepthMap(), after, "mixed deque (reactivated=%r)" % reactivated, hyp0, DEQUE)


def motion_source(w, h, nframes, seq, kind):
    return em.frames(w, h)


BATCH = {3: (("diag++", "forward-big", "pitch"), ("y-", "roll", "backward")),
         4: (("x-", "backward", "diag+-", "wide"), ("forward", "y+", "x+", "yaw")),
         8: (("x+", "x-", "y+", "y-", "forward", "backward", "yaw", "roll"),
             ("backward", "diag+-", "forward", "wide", "pitch", "x+", "other-scene", "diag++"))}


@pytest.mark.parametrize("w,h,n,py", [(320, 240, 3, 1), (320, 240, 8, 2), (176, 144, 4, 1)])
def test_update_batch_a_motion_per_map(oracle, hip, w, h, n, py):
    """updateKeyframeBatch, every map of a call with another motion; two calls: n = 3 takes the one-launch form, n = 4 and 8 select + walk
    with the every-pixel select on the first call after upload and the candidate select on the second"""
    twins = build_twins(oracle, w, h, n, source=motion_source, nseq=1, nframes=len(em.NAMES) + 1)
    ctx = hip.Context(w, h, twins[0].K)
    upload_twins(hip, ctx, twins)
    split = n >= 4
    for call, names in enumerate(BATCH[n]):
        form = dict(ONE_LAUNCH if not split else (SPLIT_ALL if call == 0 else SPLIT_CAND), py=py)
        update_round(oracle, hip, ctx, twins, [em.index_of(m) for m in names], "%dx%d n=%d call %d %r" % (w, h, n, call, names), form=form,
                     expect_low_grad=(call == 0) if split else None)


SEQUENCE = ("x+", "forward", "y-", "backward", "roll")


def test_update_keyframe_end_to_end_through_motions(oracle, hip):
    """updateKeyframe over five frames whose poses walk through +x, forward, -y, backward and a roll (ids 5 .. 9): the map after each
    call, then the keyframe's pyramid planes and statistics"""
    w, h = 320, 240
    ctx, kfo, kfg, dmo, dmg, hyp = make_pair(oracle, hip, w, h, seed=11)
    before = hyp
    for i, name in enumerate(SEQUENCE):
        fo = em.oracle_frame(oracle, w, h, name, kfo, fid=5 + i)
        fg = device_frame(oracle, hip, ctx, w, h, name, kfg, fid=5 + i)
        dmo.update([fo])
        dmg.updateKeyframe([fg])
        after = dmo.get()
        assert changed_pixels(before, after) >= 1000, (i, name)
        assert_map(oracle, w, h, dmg.currentDepthMap(), after, "updateKeyframe %d (%s)" % (i, name), before, [name])
        before = after
    so, sg = kfo.stats(), kfg.stats()
    for k in ("numFramesTrackedOnThis", "numMappedOnThis", "numMappedOnThisTotal", "depthHasBeenUpdatedFlag", "numPoints"):
        assert sg[k] == so[k], (k, sg[k], so[k])
    assert so["numMappedOnThis"] == 3 + len(SEQUENCE) and so["depthHasBeenUpdatedFlag"] == 1
    for lvl in range(5):
        assert_bit_equal(kfg.idepth(lvl), kfo.plane("idepth", lvl), "keyframe idepth L%d" % lvl)
        assert_bit_equal(kfg.idepthVar(lvl), kfo.plane("idepthVar", lvl), "keyframe idepthVar L%d" % lvl)
    # meanIdepth: the oracle's is a sequential float32 sum, the yardstick is the float64 mean of the (bit-equal) level-0 plane
    assert_mean_idepth(sg, kfo.plane("idepth", 0), kfo.plane("idepthVar", 0), "keyframe")
