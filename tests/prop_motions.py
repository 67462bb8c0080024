"""General camera motions for DepthMap::propagateDepth (phase A / phase B of K7, the fused finalize + phase A launch and the batched
phase B), start states that reach its rare branches, and a census of the branches a case reaches.  No GPU here.

The motions are those of tests/epl_motions.py plus four of this module's own (EXTRA): two backward motions under a rotation, which put
exactly the slot capacity, one or two more, and many more sources on one target with the sources arriving out of raster order, and two
poses whose thisToParent_raw carries a Sim3 scale.  planted() adds validity counters up to 200 (their sums reach the merge's clamp) and
near points that a forward motion of 0.5 puts BEHIND the new camera (a negative new_idepth that still projects inside the image; the
reference keeps it as a candidate).

census() restates propagateDepth's branches in float64 numpy to classify sources and targets — it is never an expected value: expected
values come from the oracle alone."""
import functools
from collections import OrderedDict

import numpy as np

import epl_motions as em
from common import synth

# C/DepthEstimation/DepthMapPixelHypothesis.h and C/util/settings.h (the values oracle/orc_depthmap.cpp and csrc/depthmap.hip carry)
MAX_DIFF_CONSTANT = 40.0 * 40.0
MAX_DIFF_GRAD_MULT = 0.5 * 0.5
VALIDITY_CAP = 5 + 250            # VALIDITY_COUNTER_MAX + VALIDITY_COUNTER_MAX_VARIABLE
DIFF_FAC_PROP_MERGE = 1.0
PROP_SLOT_CAP = 8                 # csrc/depthmap.hip: sources a target holds in its slot list; the rest travel on a chain


def _extra():
    """name -> (rotation, camera centre, seq_index of the scene shown, Sim3 scale of thisToParent_raw)"""
    m = OrderedDict()
    m["far-back-roll"] = ((0, 0.02, 0.05), (0.1, -0.05, -3.5), 0, 1.0)     # up to ~17 sources per target, under a rotation
    m["back-1.5"] = ((0.01, 0, 0.03), (0.05, 0.02, -1.5), 0, 1.0)          # 7 .. 10 sources on the fullest targets: the 8 / 9 edge
    m["scaled"] = em.MOTIONS["yaw"][:2] + (0, 0.8)
    m["scaled-up"] = em.MOTIONS["roll"][:2] + (0, 1.25)
    return m


EXTRA = _extra()
NAMES = em.NAMES + list(EXTRA)
CHAINS = ("far-back-roll", "back-1.5")     # more sources than slots on some target (back-1.5: at 320x240 only)


def index_of(name):
    """1-based index of a motion = index of its image in frames(); the motions of epl_motions keep theirs"""
    return NAMES.index(name) + 1


def scale_of(name):
    return EXTRA[name][3] if name in EXTRA else 1.0


@functools.lru_cache(maxsize=4)
def frames(w, h):
    """(images uint8 [1 + len(NAMES), h, w], depth0, K, gt double [.., 7]): em.frames followed by the images of EXTRA"""
    imgs0, depth0, K, gt0 = em.frames(w, h)
    poses = [(np.eye(3), np.zeros(3))] + [(em.rot(*r), np.array(c, np.float64)) for r, c, _, _ in EXTRA.values()]
    sc = em.FreeScene(poses, 0)
    imgs = np.zeros((len(EXTRA), h, w), np.uint8)
    gt = np.zeros((len(EXTRA), 7))
    for i in range(len(EXTRA)):
        imgs[i], _ = sc.render(i + 1, w, h)
        gt[i] = synth.pose7(*sc.frame_to_ref(i + 1, 0))
    imgs, gt = np.concatenate([imgs0, imgs]), np.concatenate([gt0, gt])
    for a in (imgs, gt):
        a.setflags(write=False)
    return imgs, depth0, K, gt


def pose_of(oracle, w, h, name):
    """(frame id, Sim3 new keyframe -> old keyframe, initialTrackedResidual): the motion's pose composed with _ref_pose's general twist,
    with the motion's Sim3 scale"""
    from test_gpu_parity import _ref_pose
    k = index_of(name)
    sim3, itr = _ref_pose(oracle, frames(w, h)[3], k)
    sim3[7] = scale_of(name)
    return em.FID0 + k, sim3, itr


def mask_of(w, h, name):
    """the refPixelWasGood mask a motion's frame carries (9 in 10 set)"""
    return (np.random.default_rng(40 + index_of(name)).uniform(size=(h >> 1, w >> 1)) < 0.9).astype(np.uint8)


def oracle_frame(oracle, w, h, name, parent, L=None, mask=True):
    f, sim3, itr = pose_of(oracle, w, h, name)
    fo = oracle.Frame(f, frames(w, h)[0][index_of(name)], frames(w, h)[2], L=L)
    fo.set_pose(sim3, parent, itr)
    if mask:
        fo.set_wasgood(mask_of(w, h, name))
    return fo


def planted(hyp, seed):
    """on top of a ragged state: validity counters uniform in [0, 200), and on about 8 % of the valid pixels a near point (inverse depth
    uniform in [1.2, 6.0], scene ~0.5)"""
    rng = np.random.default_rng(seed)
    hyp = hyp.copy()
    hyp["validity_counter"] = rng.integers(0, 200, hyp.shape).astype(np.int32)
    near = (hyp["isValid"] > 0) & (rng.uniform(size=hyp.shape) < 0.08)
    val = rng.uniform(1.2, 6.0, hyp.shape).astype(np.float32)
    for k in ("idepth", "idepth_smoothed"):
        hyp[k][near] = val[near]
    return hyp


@functools.lru_cache(maxsize=8)
def _start(w, h, plant):
    from oracle import pyoracle
    from test_gpu_parity import _noisy_hyp
    imgs, depth0, K, _ = frames(w, h)
    kf = pyoracle.Frame(0, imgs[0], K)
    kf.set_depth_gt(depth0)
    dm = pyoracle.DepthMap(w, h, K)
    dm.init_gt(kf)
    dm.set(kf, _noisy_hyp(dm.get(), 0.02, 33))
    dm.stage("regularize")
    hyp = dm.get()
    if plant:
        hyp = planted(hyp, 7)
    hyp.setflags(write=False)
    return hyp


def start_state(w, h, plant):
    """the map a case starts from: _noisy_hyp (sigma 0.02, seed 33) regularised once (the start of the zoom-out test), then planted(.., 7)
    or not.  Computed once per size on the oracle; read-only."""
    return _start(w, h, bool(plant))


def oracle_map(oracle, w, h, hyp, params=None, L=None, threads=4):
    """(keyframe, map) holding `hyp` on the keyframe of frames() — on the oracle, or with L on the reference library"""
    imgs, depth0, K, _ = frames(w, h)
    kf = oracle.Frame(0, imgs[0], K, L=L)
    kf.set_depth_gt(depth0)
    dm = oracle.DepthMap(w, h, K, params=params, L=L, threads=threads)
    dm.init_gt(kf)
    dm.set(kf, hyp)
    kf.set_counters(7, 3, 3, 0)
    return kf, dm


SOURCE_CLASSES = ("out-left", "out-top", "out-right", "out-bottom", "behind", "behind-in-image", "mask-reject", "grad-reject", "photo-reject")
TARGET_CLASSES = ("targets", "targets-2+", "targets-eq-cap", "targets-cap+1..2", "targets-over-cap", "occ-keep-old", "occ-replace", "fused",
                  "validity-capped")
CLASSES = SOURCE_CLASSES + TARGET_CLASSES


def census(K, w, h, hyp, pose, mask, new_maxgrad, old_image, new_image, params):
    """Which branches of propagateDepth the sources and targets of a map reach under `pose` (Sim3 new keyframe -> old keyframe, 8
    doubles), in float64.  mask: the new keyframe's refPixelWasGood (level 1) or None — then the photometric test with the two level-0
    images decides.  A CLASSIFICATION of the inputs, never an expected value: near a threshold float64 and the float32 code may disagree
    on a pixel.

    Source classes (masks over SOURCE pixels; a source is counted at the first test that rejects it, the four borders in the order the
    condition names them): out-*, mask-reject / photo-reject, grad-reject; behind = negative new_idepth, behind-in-image = behind and
    inside the border test.  Target classes (masks over TARGET pixels) come from replaying each target's candidates in raster order:
    occ-keep-old (the candidate lies behind the target's hypothesis and is dropped), occ-replace (it lies in front and replaces it), fused,
    validity-capped (the merged counter exceeded the cap).

    Returns {"counts", "masks", "nsrc": int [h, w] candidates per target, "max_sources": the largest of them}."""
    fx, fy, cx, cy = [float(v) for v in K]
    pose = np.asarray(pose, np.float64)
    q = pose[:4] * (pose[7] if len(pose) > 7 else 1.0)
    q = q / np.linalg.norm(q)                        # se3FromSim3: the scaled quaternion, normalised; the translation as it is
    qw, qx, qy, qz = q
    Rn = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                   [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                   [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])
    R = Rn.T                                         # old -> new
    t = -(R @ pose[4:7])
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    src = hyp["isValid"] > 0
    ids = hyp["idepth_smoothed"].astype(np.float64)
    masks = {k: np.zeros((h, w), bool) for k in CLASSES}
    with np.errstate(divide="ignore", invalid="ignore"):
        r0, r1 = (x - cx) / fx, (y - cy) / fy
        pn = [(R[i, 0] * r0 + R[i, 1] * r1 + R[i, 2]) / ids + t[i] for i in range(3)]
        nid = 1.0 / pn[2]
        u, v = pn[0] * nid * fx + cx, pn[1] * nid * fy + cy
        live = src
        for k, ok in (("out-left", u > 2.1), ("out-top", v > 2.1), ("out-right", u < w - 3.1), ("out-bottom", v < h - 3.1)):
            masks[k] = live & ~ok
            live = live & ok
        masks["behind"] = src & (nid < 0)
        masks["behind-in-image"] = live & (nid < 0)
        ui = np.where(live, u + 0.5, 0).astype(np.int64)
        vi = np.where(live, v + 0.5, 0).astype(np.int64)
        tgt = ui + vi * w
        grad = np.asarray(new_maxgrad, np.float64).reshape(-1)[tgt]
        if mask is not None:
            bad = np.asarray(mask)[(y.astype(np.int64) >> 1), (x.astype(np.int64) >> 1)] == 0
            masks["mask-reject"] = live & bad
        else:
            img = np.asarray(new_image, np.float64)
            ix, iy = np.where(live, u, 0).astype(np.int64), np.where(live, v, 0).astype(np.int64)
            dx, dy = np.where(live, u, 0) - ix, np.where(live, v, 0) - iy
            ix1, iy1 = np.minimum(ix + 1, w - 1), np.minimum(iy + 1, h - 1)
            dest = (dx * dy * img[iy1, ix1] + (dy - dx * dy) * img[iy1, ix] + (dx - dx * dy) * img[iy, ix1]
                    + (1 - dx - dy + dx * dy) * img[iy, ix])
            res = dest - np.asarray(old_image, np.float64)
            bad = res * res / (MAX_DIFF_CONSTANT + MAX_DIFF_GRAD_MULT * grad * grad) > 1.0
            masks["photo-reject"] = live & bad
        live = live & ~bad
        masks["grad-reject"] = live & (grad < params.minUseGrad)
        live = live & ~(grad < params.minUseGrad)
        ratio = nid / ids
        nvar = ratio ** 4 * hyp["idepth_var"].astype(np.float64)
    # candidates in raster order of their sources, grouped by target
    s_idx = np.flatnonzero(live.reshape(-1))
    c_t = tgt.reshape(-1)[s_idx]
    order = np.argsort(c_t, kind="stable")            # (stable: sources stay in raster order within a target)
    s_idx, c_t = s_idx[order], c_t[order]
    c_id, c_var = nid.reshape(-1)[s_idx], nvar.reshape(-1)[s_idx]
    c_val = hyp["validity_counter"].reshape(-1)[s_idx].astype(np.int64)
    nsrc = np.bincount(c_t, minlength=w * h)
    first = np.concatenate([[0], np.cumsum(nsrc)])[:-1]
    rank = np.arange(len(c_t)) - first[c_t]
    T = w * h
    tv = np.zeros(T, bool)
    tid, tvar, tval = np.zeros(T), np.zeros(T), np.zeros(T, np.int64)
    ev = {k: np.zeros(T, bool) for k in ("occ-keep-old", "occ-replace", "fused", "validity-capped")}
    for k in range(int(nsrc.max()) if len(c_t) else 0):
        sel = rank == k
        j, ni, nv, nc = c_t[sel], c_id[sel], c_var[sel], c_val[sel]
        had = tv[j]
        diff = tid[j] - ni
        occ = had & (DIFF_FAC_PROP_MERGE * diff * diff > nv + tvar[j])
        keep = occ & (ni < tid[j])
        repl = occ & ~keep
        fuse = had & ~occ
        ev["occ-keep-old"][j[keep]] = True
        ev["occ-replace"][j[repl]] = True
        ev["fused"][j[fuse]] = True
        new = ~had | repl
        wgt = np.where(fuse, nv / np.where(fuse, tvar[j] + nv, 1.0), 0.0)
        m_id = wgt * tid[j] + (1 - wgt) * ni
        with np.errstate(divide="ignore"):
            m_var = 1.0 / (1.0 / np.where(fuse, tvar[j], 1.0) + 1.0 / nv)
        m_val = nc + tval[j]
        ev["validity-capped"][j[fuse & (m_val > VALIDITY_CAP)]] = True
        m_val = np.minimum(m_val, VALIDITY_CAP)
        tid[j] = np.where(new, ni, np.where(fuse, m_id, tid[j]))
        tvar[j] = np.where(new, nv, np.where(fuse, m_var, tvar[j]))
        tval[j] = np.where(new, nc, np.where(fuse, m_val, tval[j]))
        tv[j] = True
    nsrc2 = nsrc.reshape(h, w)
    masks["targets"] = nsrc2 > 0
    masks["targets-2+"] = nsrc2 >= 2
    masks["targets-eq-cap"] = nsrc2 == PROP_SLOT_CAP
    masks["targets-cap+1..2"] = (nsrc2 > PROP_SLOT_CAP) & (nsrc2 <= PROP_SLOT_CAP + 2)
    masks["targets-over-cap"] = nsrc2 > PROP_SLOT_CAP
    for k, m in ev.items():
        masks[k] = m.reshape(h, w)
    return {"counts": {k: int(m.sum()) for k, m in masks.items()}, "masks": masks, "nsrc": nsrc2, "max_sources": int(nsrc.max())}


def case_census(oracle, w, h, name, use_mask, plant, hyp=None):
    """the census of one case: motion, mask setting, start state (or an explicit map on the keyframe of frames())"""
    imgs, _, K, _ = frames(w, h)
    hyp = start_state(w, h, plant) if hyp is None else hyp
    nk = oracle.Frame(1, imgs[index_of(name)], K)
    kf = oracle.Frame(0, imgs[0], K)
    return census(K, w, h, hyp, pose_of(oracle, w, h, name)[1], mask_of(w, h, name) if use_mask else None, nk.plane("maxGradients", 0),
                  kf.plane("image", 0), nk.plane("image", 0), oracle.default_params())


def classes_at(c, x, y):
    """the census classes pixel (x, y) falls in as a target, and the number of sources it had (for naming a differing pixel)"""
    return [k for k in TARGET_CLASSES if c["masks"][k][y, x]], int(c["nsrc"][y, x])


def census_table(rows):
    """rows: [(case label, census)] -> the table the CPU test prints"""
    short = ("oL", "oT", "oR", "oB", "behd", "b-in", "mask", "grad", "phot", "tgt", "2+", "=8", "9-10", ">8", "keep", "repl", "fuse", "vcap")
    out = ["%-28s " % "case" + " ".join("%5s" % s for s in short) + "   max"]
    for label, c in rows:
        out.append("%-28s " % label + " ".join("%5d" % c["counts"][k] for k in CLASSES) + " %5d" % c["max_sources"])
    return "\n".join(out)
