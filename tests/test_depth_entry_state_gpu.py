"""What the batched DepthMap entries (lsdhip_depth_update_batch, lsdhip_depth_change_keyframe_batch) leave behind on the host side, on
176x144 maps (the smallest size of test_depth_batch_gpu.py) and batches of two.

Both entries validate the whole batch before they touch a map: the item builders swap validity planes, move maps to their new keyframes and
claim deferred-result slots, so a builder that ran for map 0 before map 1 was validated would leave map 0 half-way.

  * every refusal the two entries make (the offending entry is always the SECOND one of the batch) leaves currentDepthMap() of every map
    named in the call byte for byte as it was, isValid() unchanged and the context's batch-form record (lsdhip_ctx_batch_form) unchanged;
    the valid call that follows gives the planes, keyframe statistics and rescale factors — compared with == on the bits — of a twin
    context that never saw the refusal.
  * single and batched calls interleave on one map (the propClean hand-off of the propagation scratch: a single createKeyFrame leaves it in
    use, the batched change behind it must clear first, and leaves it clean for the next): batched change, finalizeKeyFrame +
    createKeyFrame, batched change, with an update behind each, against a twin that takes the single-map entries throughout — all eight
    hypothesis planes, both keyframes' level-0 idepth and variance and the rescale factor after every step, with ==.

The tracked frames carry explicit poses and masks (frame_inputs / device_frame of test_depth_batch_gpu.py): no tracker result enters."""
import numpy as np
import pytest

from lsd_slam_amd.capi import LsdHipError
from test_depth_batch_gpu import PLANES, build_twins, device_frame, frame_inputs
from test_gpu_parity import _ref_pose

pytestmark = pytest.mark.gpu

W, H, N = 176, 144, 2


@pytest.fixture(scope="module")
def hip():
    import lsd_slam_amd as la
    return la


@pytest.fixture(scope="module")
def twins(oracle):
    """two ragged maps (oracle side: read only here) with their sequences"""
    return build_twins(oracle, W, H, N)


class World:
    """a context with the twins' maps uploaded, plus a map that never got a keyframe"""

    def __init__(self, hip, twins):
        self.ctx = hip.Context(W, H, twins[0].K)
        self.kfs, self.maps = [], []
        for t in twins:
            kf = hip.Frame(self.ctx, 0, t.frames[0])
            kf.setDepthFromGroundTruth(t.depth0)
            dm = hip.DepthMap(self.ctx)
            dm.setCurrentDepthMap(kf, t.hyp0, reactivated=t.react)
            self.kfs.append(kf)
            self.maps.append(dm)
        self.empty = hip.DepthMap(self.ctx)


def tracked(oracle, hip, world, twins, j, fid, parent=None, base=None):
    """frame `fid` of sequence j with a mask and its ground-truth pose relative to frame `base` of the sequence (the twins' keyframe when
    None), tracked on map j's keyframe (or on `parent`)"""
    pose = None if base is None else _ref_pose(oracle, twins[j].gt, fid, base=base)[0]
    inp = frame_inputs(oracle, twins[j], fid, True, 31 * fid + j, pose=pose)
    return device_frame(hip, world.ctx, twins[j], fid, inp, parent or world.kfs[j])


def form_bits(ctx):
    out = {}
    for which in ("update", "change"):
        for k, v in ctx.batchForm(which).items():
            out[which, k] = v.tobytes() if isinstance(v, np.ndarray) else v
    return out


def stats_bits(frame):
    return np.array(list(frame.stats().values()), np.float32).tobytes()


def refused(call, message, maps, ctx, frames=()):
    """`call` is refused with `message`, and leaves the maps, the frames (statistics, pose) and the batch-form record as they were"""
    before = [(m.currentDepthMap().tobytes(), m.isValid()) for m in maps]
    fbefore = [(stats_bits(f), f.thisToParent_raw().tobytes()) for f in frames]
    form = form_bits(ctx)
    with pytest.raises(LsdHipError, match=message):
        call()
    assert [(stats_bits(f), f.thisToParent_raw().tobytes()) for f in frames] == fbefore, "a frame changed by the refused call"
    for j, m in enumerate(maps):
        assert m.isValid() == before[j][1], "map %d: isValid() changed by the refused call" % j
        assert m.currentDepthMap().tobytes() == before[j][0], "map %d: currentDepthMap() changed by the refused call" % j
    assert form_bits(ctx) == form, "the batch-form record changed by the refused call"


UPDATE_REFUSALS = ["never_tracked", "tracked_on_another_keyframe", "no_active_keyframe", "same_map_twice"]


@pytest.mark.parametrize("case", UPDATE_REFUSALS)
def test_a_refused_update_batch_leaves_nothing_behind(oracle, hip, twins, case):
    results = []
    for sees_refusal in (True, False):
        wd = World(hip, twins)
        A, B = wd.maps
        fa, fb = tracked(oracle, hip, wd, twins, 0, 3), tracked(oracle, hip, wd, twins, 1, 3)
        hip.DepthMap.updateKeyframeBatch([A, B], [fa, fb])        # (the record of an earlier call is there to be kept)
        fa, fb = tracked(oracle, hip, wd, twins, 0, 5), tracked(oracle, hip, wd, twins, 1, 5)
        if sees_refusal:
            if case == "never_tracked":
                bad = hip.Frame(wd.ctx, 6, twins[1].frames[6])
                refused(lambda: hip.DepthMap.updateKeyframeBatch([A, B], [fa, bad]), "was tracked on keyframe -1", [A, B], wd.ctx, wd.kfs)
            elif case == "tracked_on_another_keyframe":
                other = hip.Frame(wd.ctx, 50, twins[1].frames[1])
                bad = tracked(oracle, hip, wd, twins, 1, 6, parent=other)
                refused(lambda: hip.DepthMap.updateKeyframeBatch([A, B], [fa, bad]), "was tracked on keyframe 50", [A, B], wd.ctx, wd.kfs)
            elif case == "no_active_keyframe":
                refused(lambda: hip.DepthMap.updateKeyframeBatch([A, wd.empty], [fa, fb]), "depth map 1 has no active keyframe", [A, wd.empty], wd.ctx, wd.kfs)
            else:
                refused(lambda: hip.DepthMap.updateKeyframeBatch([A, A], [fa, fb]), "depth map 1 appears twice", [A], wd.ctx, wd.kfs)
        hip.DepthMap.updateKeyframeBatch([A, B], [fa, fb])
        results.append([m.currentDepthMap().tobytes() for m in wd.maps] + [stats_bits(kf) for kf in wd.kfs] + [form_bits(wd.ctx)])
    for k, (a, b) in enumerate(zip(*results)):
        assert a == b, "item %d of (maps, keyframe statistics, form) differs behind the refused call (%s)" % (k, case)


CHANGE_REFUSALS = ["no_tracking_parent", "no_active_keyframe", "new_keyframe_is_current", "same_map_twice", "same_new_keyframe_twice"]


@pytest.mark.parametrize("case", CHANGE_REFUSALS)
def test_a_refused_keyframe_change_batch_leaves_nothing_behind(oracle, hip, twins, case):
    results = []
    for sees_refusal in (True, False):
        wd = World(hip, twins)
        A, B = wd.maps
        fa, fb = tracked(oracle, hip, wd, twins, 0, 1), tracked(oracle, hip, wd, twins, 1, 1)
        hip.DepthMap.updateKeyframeBatch([A, B], [fa, fb])
        # (a keyframe has a tracking parent in the loop — it was tracked on its predecessor: this is what lets map B's own keyframe get as
        # far as the "is the current one" check; in both worlds)
        wd.kfs[1].setPose(np.array([1.0, 0, 0, 0, 0, 0, 0, 1.0]), wd.kfs[0], 0.0)
        na, nb = tracked(oracle, hip, wd, twins, 0, 2), tracked(oracle, hip, wd, twins, 1, 2)
        change = hip.DepthMap.changeKeyframeBatch
        if sees_refusal:
            if case == "no_tracking_parent":
                bad = hip.Frame(wd.ctx, 4, twins[1].frames[4])
                refused(lambda: change([A, B], [na, bad]), "no tracking parent", [A, B], wd.ctx, wd.kfs + [na])
            elif case == "no_active_keyframe":
                refused(lambda: change([A, wd.empty], [na, nb]), "depth map 1 has no active keyframe", [A, wd.empty], wd.ctx, wd.kfs + [na])
            elif case == "new_keyframe_is_current":
                refused(lambda: change([A, B], [na, wd.kfs[1]]), "map 1: the new keyframe is the current one", [A, B], wd.ctx, wd.kfs + [na])
            elif case == "same_map_twice":
                refused(lambda: change([A, A], [na, nb]), "entry 1 appears twice", [A], wd.ctx, wd.kfs + [na])
            else:
                refused(lambda: change([A, B], [na, na]), "entry 1 appears twice", [A, B], wd.ctx, wd.kfs + [na])
        scales = change([A, B], [na, nb])
        results.append([m.currentDepthMap().tobytes() for m in wd.maps] + [stats_bits(f) for f in wd.kfs + [na, nb]] +
                       [np.array(scales, np.float32).tobytes(), na.thisToParent_raw().tobytes(), nb.thisToParent_raw().tobytes(), form_bits(wd.ctx)])
    for k, (a, b) in enumerate(zip(*results)):
        assert a == b, "item %d of (maps, keyframe statistics, rescale factors, poses, form) differs behind the refused call (%s)" % (k, case)


def test_single_and_batched_calls_interleave_on_one_map(oracle, hip, twins):
    def run(batched):
        """the steps' results; batched[k]: step k of the three keyframe changes and of the updates behind them takes the batched entry"""
        wd = World(hip, twins[:1])
        dm, out = wd.maps[0], []
        for k, nk_id in enumerate((2, 4, 6)):
            old = wd.kfs[0]
            nk = tracked(oracle, hip, wd, twins, 0, nk_id, base=nk_id - 2 if k else None)
            if batched[k]:
                scale = hip.DepthMap.changeKeyframeBatch([dm], [nk])[0]
            else:
                dm.finalizeKeyFrame()
                scale = dm.createKeyFrame(nk)
            wd.kfs[0] = nk
            fr = tracked(oracle, hip, wd, twins, 0, nk_id + 1, base=nk_id)
            out.append(("change %d" % k, dm.currentDepthMap(), [old.idepth(0), old.idepthVar(0), nk.idepth(0), nk.idepthVar(0)], np.float32(scale)))
            if batched[k]:
                hip.DepthMap.updateKeyframeBatch([dm], [fr])
            else:
                dm.updateKeyframe([fr])
            out.append(("update %d" % k, dm.currentDepthMap(), [nk.idepth(0), nk.idepthVar(0)], np.float32(nk.thisToParent_raw()[7])))
        return out

    mixed, single = run([True, False, True]), run([False, False, False])
    for (what, hyp_m, planes_m, s_m), (_, hyp_s, planes_s, s_s) in zip(mixed, single):
        assert int((hyp_s["isValid"] > 0).sum()) > 500, (what, "the map is nearly empty: the comparison has no power")
        for k in PLANES:
            assert hyp_m[k].tobytes() == hyp_s[k].tobytes(), "%s: plane %s differs from the single-map entries'" % (what, k)
        for i, (a, b) in enumerate(zip(planes_m, planes_s)):
            assert a.tobytes() == b.tobytes(), "%s: keyframe plane %d differs from the single-map entries'" % (what, i)
        assert s_m.tobytes() == s_s.tobytes(), (what, s_m, s_s)
