"""What the frame entry points leave behind, on 176x144 frames (the smallest size of the depth-batch tests: 24.75 gradient-candidate groups of
1024 pixels, a ragged last reference block on every level, an odd coarse width of 11).  HIP contexts are compared with each other and with
the numpy expectation test_gpu_parity.py ties to the oracle; no oracle here.

  * A frame in a recycled arena is a fresh frame, whichever creator made it (single host image, single device image, createBatch of host
    images, createBatch of device images): two keyframes are given everything a frame can own — depth planes, level-0 planes and gradient
    candidates, a written refPixelWasGood mask, reference blocks — and closed, which returns their arenas to the context's pool (it keeps
    16, last in first out).  Two frames of other images created next equal, bit for bit, frames of those images in a context that never
    recycled anything; they have no mask and no depth; and after the same setDepthPlanes both sides hold the same pyramids and blocks.
  * The reference blocks of a keyframe are the same lists whichever route built them — on download (a context that never ran a throughput-mode
    batch), behind the idepth pyramid (a context that has), or by lsd_frames_require_ref_blocks for the keyframes of an 8-job batch
    (deduplicated: every job names the same keyframe) — on one-stream and on pipelined contexts, and they are the lists the numpy
    expectation derives from the downloaded planes.
  * setDepthFromGroundTruth and setDepthPlanes leave the same planes and statistics on a one-stream and on a pipelined context, where they are
    visible to the tracker at once: TrackingReference.importFrame + makePointCloud(1) gives the one-stream context's points.

Of reference blocks and gradient candidates every block's (group's) count and its listed offsets are compared; the slots behind a count are
written by no kernel and read by no consumer."""
import numpy as np
import pytest

from common import assert_bit_equal, assert_reference_blocks_list, sequence

pytestmark = pytest.mark.gpu

W, H = 176, 144
JOBS = 8          # LSD_BATCH_THROUGHPUT_MIN_JOBS
IDENT7 = np.array([1.0, 0, 0, 0, 0, 0, 0], np.float32)


@pytest.fixture(scope="module")
def hip():
    import lsd_slam_amd as la
    return la


@pytest.fixture(scope="module")
def world():
    frames, depth0, K, gt = sequence(W, H, 6)
    return dict(frames=frames, depth0=depth0, K=K)


def ragged_planes(seed):
    """random holes, negative idepths, tiny variances, idepth == 0 with a positive variance (not a reference point), empty 2x2 blocks"""
    rng = np.random.default_rng(seed)
    idp = rng.uniform(-0.2, 2.0, (H, W)).astype(np.float32)
    var = rng.uniform(1e-6, 0.25, (H, W)).astype(np.float32)
    hole = rng.uniform(size=(H, W)) < 0.55
    idp[hole] = -1
    var[hole] = -1
    idp[rng.uniform(size=(H, W)) < 0.02] = 0.0
    idp[10:20, 10:20] = -1
    var[10:20, 10:20] = -1
    return idp, var


def listed(blocks):
    """(offsets with the slots behind each block's count zeroed, counts)"""
    offs, cnts = blocks
    keep = np.arange(256)[None, :] < cnts[:, None]
    return np.where(keep, offs, 0).astype(np.uint8), cnts


def frame_planes(f):
    out = {}
    for l in range(5):
        out["image L%d" % l] = f.image(l)
        out["gradients L%d" % l] = f.gradients(l)
    out["maxGradients"] = f.maxGradients(0)
    out["candidate offsets"], out["candidate counts"] = f.gradientCandidates()
    return out


def depth_planes(f):
    out = {}
    for l in range(5):
        out["idepth L%d" % l] = f.idepth(l)
        out["idepthVar L%d" % l] = f.idepthVar(l)
    for l in range(1, 5):
        out["block offsets L%d" % l], out["block counts L%d" % l] = listed(f.referenceBlocks(l))
    return out


def assert_same(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        assert_bit_equal(got[k], want[k], "%s: %s" % (what, k))


def candidates_listed(planes):
    """the candidate lists up to each group's count (the slots behind it are not written)"""
    offs, cnts = planes["candidate offsets"], planes["candidate counts"]
    keep = np.arange(1024)[None, :] < cnts[:, None].astype(np.int64)
    out = dict(planes)
    out["candidate offsets"] = np.where(keep, offs, 0).astype(np.uint16)
    return out


# -----------------------------------------------------------------------------------------------------------------------------------------
# a frame in a recycled arena is a fresh frame
# -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fresh(hip, world):
    """frames of images 2 and 3 in a context that never recycled an arena: their planes before, and their depth planes after setDepthPlanes"""
    ctx = hip.Context(W, H, world["K"])
    idp, var = ragged_planes(21)
    both = [hip.Frame(ctx, 100 + j, world["frames"][j]) for j in (2, 3)]     # (both alive: each in an arena of its own)
    want = []
    for f in both:
        planes = candidates_listed(frame_planes(f))
        f.setDepthPlanes(idp, var)
        want.append((planes, depth_planes(f)))
    for f in both:
        f.close()
    ctx.close()
    return want


def create_two(hip, ctx, images, creator):
    if creator in ("single-device", "batch-device"):
        import torch
        d = torch.from_numpy(np.ascontiguousarray(np.stack(images))).cuda()
        torch.cuda.synchronize()
        if creator == "single-device":
            return [hip.Frame(ctx, 200 + j, device_ptr=d[j].data_ptr()) for j in range(2)], d
        return hip.Frame.createBatch(ctx, [200, 201], device_ptrs=[d[j].data_ptr() for j in range(2)]), d
    if creator == "single-host":
        return [hip.Frame(ctx, 200 + j, images[j]) for j in range(2)], None
    return hip.Frame.createBatch(ctx, [200, 201], images=images), None


@pytest.mark.parametrize("creator", ["single-host", "single-device", "batch-host", "batch-device"])
def test_a_frame_in_a_recycled_arena_is_a_fresh_frame(hip, world, fresh, creator):
    ctx = hip.Context(W, H, world["K"])
    rng = np.random.default_rng(5)
    for j in (0, 1):                                   # two keyframes that own everything a frame can own
        kf = hip.Frame(ctx, j, world["frames"][j])
        kf.setDepthPlanes(*ragged_planes(40 + j))
        assert kf.maxGradients(0).max() > 0            # builds the level-0 planes and the candidates
        kf.set_refPixelWasGood(rng.integers(0, 2, (H // 2, W // 2)).astype(np.uint8))
        assert kf.referenceBlocks(1)[1].sum() > 0
        kf.close()                                     # ... and hand their arenas to the pool
    new, keep_alive = create_two(hip, ctx, [world["frames"][2], world["frames"][3]], creator)
    idp, var = ragged_planes(21)
    for j, f in enumerate(new):
        what = "%s frame %d" % (creator, j)
        want_planes, want_depth = fresh[j]
        assert f.refPixelWasGoodNoCreate() is None, what
        with pytest.raises(hip.LsdHipError):
            f.idepth(0)
        assert_same(candidates_listed(frame_planes(f)), want_planes, what)
        f.setDepthPlanes(idp, var)
        assert_same(depth_planes(f), want_depth, what)
    del keep_alive


# -----------------------------------------------------------------------------------------------------------------------------------------
# the reference blocks are the same whichever route built them
# -----------------------------------------------------------------------------------------------------------------------------------------
def throughput_batch(hip, ctx, tr, kf, frames):
    """one 8-job evaluation that names kf as every job's keyframe (throughput mode: the strips read the reference blocks)"""
    ref = hip.TrackingReference()
    ref.importFrame(kf)
    frs = [hip.Frame(ctx, 300 + j, frames[1 + j % 3]) for j in range(JOBS)]
    recs, form = tr.evaluateBatch([ref] * JOBS, frs, np.tile(IDENT7, (JOBS, 1)), 2)
    assert len(recs) == JOBS
    return frs


@pytest.mark.parametrize("pipelined", [False, True], ids=["one-stream", "pipelined"])
def test_reference_blocks_are_the_same_whichever_route_built_them(hip, world, pipelined):
    frames = world["frames"]
    idp, var = ragged_planes(11)

    def context():
        ctx = hip.Context(W, H, world["K"])
        if pipelined:
            ctx.set_pipeline(True)
        return ctx

    # (a) a context that never ran a throughput-mode batch: built on download
    ctx_a = context()
    kf_a = hip.Frame(ctx_a, 1, frames[0])
    kf_a.setDepthPlanes(idp, var)
    # (c) depth before the first 8-job call, which builds the blocks of its keyframes where they are missing
    ctx_b = context()
    tr = hip.SE3Tracker(ctx_b)
    kf_c = hip.Frame(ctx_b, 3, frames[0])
    kf_c.setDepthPlanes(idp, var)
    jobs = throughput_batch(hip, ctx_b, tr, kf_c, frames)
    # (b) the same context afterwards: built behind the single idepth pyramid
    kf_b = hip.Frame(ctx_b, 2, frames[0])
    kf_b.setDepthPlanes(idp, var)
    got = {}
    for name, kf in (("on download", kf_a), ("behind the pyramid", kf_b), ("for the batch", kf_c)):
        got[name] = depth_planes(kf)
        for l in range(1, 5):
            offs, cnts = kf.referenceBlocks(l)
            assert_reference_blocks_list(offs, cnts, kf.idepth(l), kf.idepthVar(l), l)
    assert got["on download"]["block counts L1"].sum() > 0
    for name in ("behind the pyramid", "for the batch"):
        assert_same(got[name], got["on download"], name)
    del jobs


# -----------------------------------------------------------------------------------------------------------------------------------------
# the set-depth entries agree between the execution models
# -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["setDepthFromGroundTruth", "setDepthPlanes"])
def test_set_depth_entries_agree_between_execution_models(hip, world, entry):
    got = {}
    for model in ("one-stream", "pipelined"):
        ctx = hip.Context(W, H, world["K"])
        if model == "pipelined":
            ctx.set_pipeline(True)
        kf = hip.Frame(ctx, 7, world["frames"][0])
        if entry == "setDepthFromGroundTruth":
            kf.setDepthFromGroundTruth(world["depth0"])
        else:
            kf.setDepthPlanes(*ragged_planes(33))
        ref = hip.TrackingReference()
        ref.importFrame(kf)
        cloud = ref.makePointCloud(1)                  # what a tracker would read, right behind the call
        planes = {}
        for l in range(5):
            planes["idepth L%d" % l] = kf.idepth(l)
            planes["idepthVar L%d" % l] = kf.idepthVar(l)
        got[model] = (planes, kf.stats(), cloud)
    planes1, stats1, cloud1 = got["one-stream"]
    planes2, stats2, cloud2 = got["pipelined"]
    assert (planes1["idepthVar L0"] > 0).sum() > 0 and len(cloud1[0]) > 0
    assert_same(planes2, planes1, entry)
    assert stats2 == stats1
    for a, b, what in zip(cloud2, cloud1, ("positions", "colour and variance", "gradients", "indices")):
        assert_bit_equal(a, b, "%s: point cloud %s" % (entry, what))
